"""CPU: the C-ABI library builds/loads, exports every symbol include/gpsgs.h declares, and the host shims refuse to run
without a GPU (there is no CPU fallback in the product path)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import gps_gaussian_amd
from gps_gaussian_amd import _capi

import capi_run
from capi_run import call, pointers, spec


def test_library_exports_every_declared_symbol():
    lib = capi_run.lib()
    declared = capi_run.declared("gsr_", "cs_", "gpsgs_", "fl_", "up_", "cv_", "cu_")
    assert len(declared) >= 9
    assert sorted(_capi.SYMBOLS) == declared
    raw = capi_run.raw()
    for name in declared:
        assert hasattr(raw, name), name
    assert lib.gpsgs_abi_version() == 4
    assert b"gfx950" in lib.gpsgs_build_info()


def test_every_listed_symbol_has_its_prototype():
    """The prototype table is the sections' symbol tuples end to end and holds every function the header declares, whatever its section, and
    lib() leaves no symbol on ctypes' default conversion (which would pass a 64-bit device pointer as a C int)."""
    names = sum(_capi.SECTIONS, ())
    assert tuple(_capi.PROTOTYPES) == names
    assert sorted(_capi.PROTOTYPES) == capi_run.declared()
    lib = _capi.lib()
    assert [n for n in names if getattr(lib, n).argtypes is None] == []


def test_python_constants_mirror_the_header():
    """Every GSR_FLAG_* / GPSGS_E_* the ctypes shim uses has the value include/gpsgs.h gives it (a flag added on one side only would
    silently select a different kernel path)."""
    src = capi_run.header()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(GSR_FLAG_[A-Z_]+)\s+(\d+)u\b", src)}
    assert {"GSR_FLAG_DEBUG", "GSR_FLAG_TIMING", "GSR_FLAG_NO_LARGE_SORT", "GSR_FLAG_COMPOSITE_TILES", "GSR_FLAG_NO_COLOR_GRAD", "GSR_FLAG_WAVE_PRIORITY"} <= set(flags)
    for name, value in flags.items():
        assert getattr(_capi, name) == value, name
    vals = sorted(flags.values())
    assert all(v & (v - 1) == 0 for v in vals) and len(set(vals)) == len(vals)   # distinct single bits
    assert not any(v & 0xf0 for v in vals)                                       # bits 4..7 carry the stage of GSR_FLAG_TIMING_STAGE
    errs = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(GPSGS_E_[A-Z_]+)\s*=\s*(-?\d+)", src)}
    assert errs and all(getattr(_capi, k) == v for k, v in errs.items() if hasattr(_capi, k))
    assert _capi.GPSGS_E_INTERNAL == errs["GPSGS_E_INTERNAL"]


def test_code_object_targets_gfx950():
    out = subprocess.run(["strings", "-a", _capi.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert "gfx950" in out


def test_workspace_bytes_monotone_and_aligned():
    lib = _capi.lib()
    a = lib.gsr_workspace_bytes(1000, 256, 256, 10000)
    b = lib.gsr_workspace_bytes(1000, 256, 256, 20000)
    c = lib.gsr_workspace_bytes(2000, 256, 256, 20000)
    assert 0 < a < b < c and a % 256 == 0
    # 600k Gaussians, 1024^2, 4M instances: a few hundred MB at most
    assert lib.gsr_workspace_bytes(600000, 1024, 1024, 4_000_000) < 512 << 20
    assert lib.gsr_workspace_bytes(-1, 16, 16, 1) == 0


# (P, W, H, cap, bin_cap, forward_only, F) -> gsr_workspace_bytes, _forward_only, _ex, _depth_alpha, _features, _contrib, _absgrad, recorded from the library
# of commit 346b1f4 (before the seven functions shared one helper): bin_cap 0 / 1024 (and 64), F = 1 / 64, images that cannot have direct lists
# (4096^2), the largest capacity, and arguments each function refuses (0): a bin capacity no direct list can have, F = 0 / 65, a negative P / width /
# height / capacity
_RECORDED_SIZES = [
    ((30000, 256, 256, 1048576, 0, 0, 3), (54450688, 15533056, 54450688, 58644992, 71227904, 75422208, 67033600)),
    ((30000, 256, 256, 1048576, 0, 1, 3), (54450688, 15533056, 15533056, 15533056, 15533056, 75422208, 67033600)),
    ((30000, 256, 256, 1048576, 1024, 0, 1), (54450688, 15533056, 54450944, 58645248, 62839552, 75422464, 67033856)),
    ((30000, 256, 256, 1048576, 1024, 1, 64), (54450688, 15533056, 15533056, 15533056, 15533056, 75422464, 67033856)),
    ((600000, 1024, 1024, 5242880, 1024, 0, 64), (316044032, 119652352, 454462464, 475433984, 1817611264, 559320064, 517377024)),
    ((600000, 1024, 1024, 5242880, 0, 0, 1), (316044032, 119652352, 316044032, 337015552, 357987072, 420901632, 378958592)),
    ((200, 44, 28, 65536, 1024, 0, 3), (3246080, 819968, 2853120, 3115264, 3901696, 4163840, 3639552)),
    ((200, 44, 28, 65536, 0, 1, 3), (3246080, 819968, 819968, 819968, 819968, 4556800, 4032512)),
    ((1, 8, 8, 1024, 0, 0, 3), (61952, 23552, 61952, 66048, 78336, 82432, 74240)),
    ((0, 8, 8, 0, 0, 0, 1), (13056, 11776, 13056, 13312, 13568, 13568, 13568)),
    ((0, 0, 0, 0, 0, 0, 1), (13056, 11776, 13056, 13312, 13568, 13568, 13568)),
    ((1, 1, 1, 1, 64, 0, 64), (13056, 11776, 15872, 16128, 16384, 16384, 16384)),
    ((288, 24, 20, 65536, 1024, 0, 3), (3245568, 819200, 2606848, 2868992, 3655424, 3917568, 3393280)),
    ((100000, 2048, 2048, 4194304, 1024, 0, 8), (248799232, 93208832, 1003781120, 1020558336, 1154776064, 1087667200, 1054112768)),
    ((100000, 4096, 4096, 4194304, 1024, 0, 8), (353400832, 197810432, 0, 0, 0, 0, 0)),
    ((100000, 4096, 4096, 4194304, 0, 0, 8), (353400832, 197810432, 353400832, 370178048, 504395776, 437286912, 403732480)),
    ((5, 1000, 7, 2147483647, 0, 1, 2), (105226768128, 25769872640, 25769872640, 25769872640, 25769872640, 148176441088, 130996571904)),
    ((30000, 256, 256, 1048576, 100, 0, 3), (54450688, 15533056, 0, 0, 0, 0, 0)),
    ((30000, 256, 256, 1048576, 2048, 0, 3), (54450688, 15533056, 0, 0, 0, 0, 0)),
    ((30000, 256, 256, 1048576, 0, 0, 0), (54450688, 15533056, 54450688, 58644992, 0, 75422208, 67033600)),
    ((30000, 256, 256, 1048576, 0, 0, 65), (54450688, 15533056, 54450688, 58644992, 0, 75422208, 67033600)),
    ((-1, 256, 256, 1048576, 0, 0, 3), (0, 0, 0, 0, 0, 0, 0)),
    ((30000, -1, 256, 1048576, 1024, 0, 3), (0, 0, 0, 0, 0, 0, 0)),
    ((30000, 256, -1, 1048576, 0, 1, 3), (0, 0, 0, 0, 0, 0, 0)),
    ((30000, 256, 256, -1, 0, 0, 3), (0, 0, 0, 0, 0, 0, 0)),
]


def test_workspace_sizes_are_the_recorded_ones():
    lib = _capi.lib()
    for (P, W, H, cap, bcap, fo, F), want in _RECORDED_SIZES:
        got = (lib.gsr_workspace_bytes(P, W, H, cap), lib.gsr_workspace_bytes_forward_only(P, W, H, cap), lib.gsr_workspace_bytes_ex(P, W, H, cap, bcap, fo),
               lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, bcap, fo), lib.gsr_workspace_bytes_features(P, W, H, cap, bcap, F, fo),
               lib.gsr_workspace_bytes_contrib(P, W, H, cap, bcap, fo), lib.gsr_workspace_bytes_absgrad(P, W, H, cap, bcap))
        assert got == want, (P, W, H, cap, bcap, fo, F)
    for k in range(7):  # every function has a case it sizes and one it refuses
        assert any(w[k] > 0 for _, w in _RECORDED_SIZES) and any(w[k] == 0 for _, w in _RECORDED_SIZES)


def test_workspace_bytes_ex_and_the_limits_of_direct_lists():
    lib = _capi.lib()
    for args in ((1000, 256, 256, 10000), (600000, 1024, 1024, 4_000_000), (0, 16, 16, 0)):
        assert lib.gsr_workspace_bytes_ex(*args, 0, 0) == lib.gsr_workspace_bytes(*args)
        assert lib.gsr_workspace_bytes_ex(*args, 0, 1) == lib.gsr_workspace_bytes_forward_only(*args)
    # direct lists: bins x capacity list entries (12 bytes each) instead of instance_capacity of them
    d = lib.gsr_workspace_bytes_ex(600000, 1024, 1024, 4_000_000, 1024, 0)
    s_ = lib.gsr_workspace_bytes(600000, 1024, 1024, 4_000_000)
    assert d % 256 == 0 and 100 << 20 < d - s_ < 200 << 20
    assert lib.gsr_direct_lists_ok(1024, 1024, 1024) == 1 and lib.gsr_direct_lists_ok(2048, 2048, 512) == 1
    assert lib.gsr_direct_lists_ok(4096, 2104, 1024) == 0      # more than 65,536 bins
    assert lib.gsr_direct_lists_ok(1024, 1024, 2048) == 0 and lib.gsr_direct_lists_ok(1024, 1024, 100) == 0 and lib.gsr_direct_lists_ok(1024, 1024, 0) == 0
    assert lib.gsr_workspace_bytes_ex(1000, 4096, 2104, 10000, 1024, 0) == 0


def test_invalid_arguments_are_rejected_without_touching_the_gpu():
    lib = _capi.lib()
    null = dict({k: None for k in pointers("gsr_forward")}, P=10, H=16, cap=0)  # every pointer NULL, no workspace
    assert call(lib, "gsr_forward", spec("gsr_forward", W=0, **null)) == _capi.GPSGS_E_INVALID
    assert call(lib, "gsr_forward", spec("gsr_forward", W=16, **null)) == _capi.GPSGS_E_INVALID
    assert lib.cs_forward(None, None, None, 1, 2, 3, 4, 4, 7, None) == _capi.GPSGS_E_INVALID
    assert lib.cs_forward(None, None, None, 0, 2, 3, 4, 4, 0, None) == _capi.GPSGS_OK  # empty batch: nothing to do


def test_no_cpu_fallback():
    import torch
    from gps_gaussian_amd import corr, rasterizer as RZ

    rs, kw = capi_run.cpu_view()
    r = RZ.GaussianRasterizer(rs)
    with pytest.raises(RuntimeError, match="GPU"):
        r(**kw)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(**{k: v for k, v in kw.items() if k != "colors_precomp"})
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(**{k: v for k, v in kw.items() if k not in ("scales", "rotations")})
    with pytest.raises(RuntimeError, match="GPU"):
        corr.forward(torch.zeros(1, 2, 3, 4), torch.zeros(1, 1, 2, 3), 4)


def test_dropin_import_names_resolve():
    code = ("import sys; sys.path.insert(0, %r); import diff_gaussian_rasterization as d, corr_sampler as c; "
            "assert d.GaussianRasterizationSettings._fields[0] == 'image_height' and len(d.GaussianRasterizationSettings._fields) == 12; "
            "assert callable(c.forward) and callable(c.backward); print('ok')") % gps_gaussian_amd.DROPIN_DIR
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd="/tmp")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_product_path_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gps-gaussian_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "gsr_oracle" not in txt, os.path.join(dp, f)
                # ... nor the reference build under oracle/_ref (test infrastructure: the CALLER of the product in tests/ and tools/ only)
                assert "_ref" not in txt and "stage_ref" not in txt and "refenv" not in txt, os.path.join(dp, f)


def test_nothing_of_the_reference_travels_to_the_gpu_box():
    """The reference is Python: it may be imported in the build container (golden vectors, the CPU tests that drive its Trainer) but does not travel in any
    form.  Through round 5 a sourceless-bytecode build of it was staged under oracle/_ref for the -m gpu reference tests; the recipe is gone, the directory
    is ignored by git and nothing under it is tracked, and no file of the repository carries bytecode."""
    assert not os.path.exists(os.path.join(ROOT, "oracle", "stage_ref.py"))
    with open(os.path.join(ROOT, ".gitignore")) as f:
        assert "oracle/_ref/" in f.read().split()
    tracked = subprocess.run(["git", "-C", ROOT, "ls-files"], stdout=subprocess.PIPE, text=True).stdout.split()
    assert not [n for n in tracked if n.endswith((".pyc", ".pyo"))]
    assert not [n for n in tracked if n.startswith("oracle/_ref/")]


def test_list_form_policy_hysteresis_and_the_compiled_host_path_declines_what_it_does_not_take(monkeypatch):
    """CPU: (a) rasterizer._note_longest -- one bin list beyond 768 entries puts a device on scanned lists (and the large-list sorts), eight views in a
    row below 512 bring direct lists back, anything in between resets the streak; GPSGS_LISTS overrides.  (b) lib/_gpsgs_fast.so loads without a GPU,
    reports the library's ABI version, and rasterize() returns None -- "not mine, take the Python path" -- for CPU tensors instead of touching them."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    st = dict(ratio=4.0, floor=1 << 16, pending=[])
    monkeypatch.delenv("GPSGS_LISTS", raising=False)
    assert RZ._bin_capacity(st, 1024, 1024) == RZ._DIRECT_CAP and RZ._bin_capacity(st, 4096, 2104) == 0   # (more than 65,536 bins: scanned)
    RZ._note_longest(st, 700)
    assert not st.get("big_bins", False)
    RZ._note_longest(st, 769)
    assert st["big_bins"] is True and RZ._bin_capacity(st, 1024, 1024) == 0
    for k in range(7):
        RZ._note_longest(st, 300)
    assert st["big_bins"] is True
    RZ._note_longest(st, 600)          # neither long nor short: the streak starts over
    for k in range(7):
        RZ._note_longest(st, 300)
    assert st["big_bins"] is True
    RZ._note_longest(st, 512)
    assert st["big_bins"] is False and RZ._bin_capacity(st, 1024, 1024) == RZ._DIRECT_CAP
    monkeypatch.setenv("GPSGS_LISTS", "scanned")
    assert RZ._bin_capacity(st, 1024, 1024) == 0
    monkeypatch.setenv("GPSGS_LISTS", "direct")
    RZ._note_longest(st, 5000)
    assert st["big_bins"] is True and RZ._bin_capacity(st, 1024, 1024) == RZ._DIRECT_CAP   # forced: the repair run of a too-long list still takes scanned lists
    monkeypatch.setenv("GPSGS_LISTS", "nonsense")
    with pytest.raises(ValueError):
        RZ._bin_capacity(st, 1024, 1024)
    monkeypatch.delenv("GPSGS_LISTS")
    monkeypatch.setenv("GPSGS_FAST", "0")
    assert RZ._fast_module() is False
    monkeypatch.setenv("GPSGS_FAST", "1")
    F = RZ._fast_module()
    assert F and F.abi_version() == _capi.lib().gpsgs_abi_version() and F.slots_in_flight(0) == 0
    z = torch.zeros
    assert F.rasterize(z(4, 3), z(4, 3), z(4, 3), z(4, 1), z(4, 3), z(4, 4), z(3), z(16), z(16), 8, 8, 1.0, 1.0, 1.0, 100, 0, 0, 0) is None
    assert len(F.last_header()) == 7
