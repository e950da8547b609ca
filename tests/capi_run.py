"""What the C-ABI contract tests share (tests/test_capi*.py; none of them needs a GPU): the header's text and its declarations, the library, the C
program behind the struct-layout tests, a by-name builder for calls of the rasteriser's entry points, the section check of the op families, the
CPU-only view that must be refused, and the pinned default workspace sizes.

A call here is made from named fields (spec / call), never from a positional list: an argument added in the middle of the C-ABI then fails here,
in one place, instead of shifting every pointer of a hand-counted list."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

import gps_gaussian_amd
from gps_gaussian_amd import _capi

HEADER = os.path.join(ROOT, "include", "gpsgs.h")
D = 0x1000  # a 16-byte aligned dummy device address: never dereferenced, every call made with it returns before any HIP call


# ---- the header -------------------------------------------------------------------------------------------------------------------------------------

def header():
    with open(HEADER) as f:
        return f.read()


def header_code():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", header(), flags=re.S)


def declared(*prefixes):
    """Sorted names of the functions the header declares with one of the prefixes ("gn_", ...); without a prefix, all of them."""
    return sorted(set(re.findall(r"\b(?:int|size_t|const char \*)\s*\*?\s*((?:%s)[a-z0-9_]+)\s*\(" % "|".join(prefixes or ("[a-z0-9]+_",)), header_code())))


def declared_arg_count(name):
    args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header_code()).group(1)
    return len([a for a in args.split(",") if a.strip()])


# ---- the library --------------------------------------------------------------------------------------------------------------------------------------

_built = False


def lib():
    """The built library with its prototypes set (the build runs once per process)."""
    global _built
    if not _built:
        gps_gaussian_amd.build()
        _built = True
    return _capi.lib()


def raw():
    """The library as ctypes loads it, no prototype set: what it exports."""
    return C.CDLL(_capi.LIB_PATH)


def c_values(tmp_path, expressions):
    """The integers a C11 program that includes gpsgs.h prints for the expressions (sizeof / offsetof / constants)."""
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpsgs.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n'
                   % (" ".join(["%lld"] * len(expressions)), ", ".join("(long long)(%s)" % e for e in expressions)))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]


# ---- calls of the rasteriser's entry points, by field name ---------------------------------------------------------------------------------------------

VIEW_PTRS = ("means3D", "colors", "opacities", "scales", "rotations", "viewmatrix", "projmatrix", "bg", "workspace")
FWD_PTRS = ("out_color", "radii")
BWD_PTRS = ("radii", "dL_dpix", "dL_dmeans3D", "dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dscales", "dL_drotations")
CAM_PTRS = ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos", "scratch")
OPTIONS = {"features": _capi.GsrFeatures, "contrib": _capi.GsrContrib, "absgrad": _capi.GsrAbsGrad, "distort": _capi.GsrDistort}
# every entry point's own option, switched on
_OPT_ON = {"gsr_forward_features": dict(channels=3, features=D, out_features=D), "gsr_forward_contrib": dict(weight_sum=D, weight_max=D, pixel_count=D),
           "gsr_backward_features": dict(channels=3, features=D, dL_dfeaturemap=D, dL_dfeatures=D), "gsr_backward_absgrad": dict(absgrad=D),
           "gsr_forward_distort": dict(out_distort=D, totals=D + 0x1000), "gsr_backward_distort": dict(dL_ddistort=D, totals=D + 0x1000)}


def is_forward(entry):
    return entry.startswith("gsr_forward")


def has_ext(entry):
    return entry not in ("gsr_forward", "gsr_forward_notify", "gsr_backward")


def has_cam(entry):
    return not is_forward(entry) and entry not in ("gsr_backward", "gsr_backward_ex")


def pointers(entry):
    """The names of the entry point's own pointer arguments (those of ext / cam / opt are fields of theirs)."""
    return VIEW_PTRS + (FWD_PTRS if is_forward(entry) else BWD_PTRS)


def spec(entry, **over):
    """A valid call of `entry` with its own option switched on and a workspace of 0 bytes; `over` replaces fields (ext / opt / cam: merged)."""
    s = dict(P=1, W=8, H=8, cap=1024, flags=0, ws=0, ext={}, cam={}, **{k: D for k in pointers(entry)})
    s["opt"] = dict(_OPT_ON.get(entry, {}))
    for k, v in over.items():
        if k in ("ext", "opt", "cam"):
            s[k] = None if v is None else dict(s[k], **v)
        else:
            s[k] = v
    return s


def _struct(cls, fields):
    if fields is None:
        return None
    x = cls()
    for k, v in fields.items():
        setattr(x, k, v)
    return C.byref(x)


def call(lib, entry, s):
    a = [s["P"], s["W"], s["H"]] + [s[k] for k in VIEW_PTRS[:5]] + [1.0, 0.5, 0.5] + [s[k] for k in VIEW_PTRS[5:8]]
    a += [s[k] for k in (FWD_PTRS if is_forward(entry) else BWD_PTRS)] + [s["workspace"], s["ws"], s["cap"], s["flags"], None]
    if is_forward(entry) and entry != "gsr_forward":
        a += [None, 0]  # no host header
    if has_ext(entry):
        a.append(_struct(_capi.GsrViewExt, s["ext"] or None))
    if has_cam(entry):
        a += [s["cam"].get(k) for k in CAM_PTRS] + [s["cam"].get("scratch_bytes", 0)]
    option = OPTIONS.get(entry.rsplit("_", 1)[1])
    if option is not None:
        a.append(_struct(option, s["opt"]))
    fn = getattr(lib, entry)
    assert len(a) == len(fn.argtypes), entry  # (ctypes itself lets a cdecl call carry more arguments than prototypes)
    return fn(*a)


def need(lib, entry, s):
    """What the matching workspace query reports for the call `s` of `entry`."""
    g = (s["P"], s["W"], s["H"], s["cap"], (s["ext"] or {}).get("bin_capacity", 0))
    if is_forward(entry):
        return lib.gsr_workspace_bytes_contrib(*g, 1) if entry == "gsr_forward_contrib" and s["opt"] else lib.gsr_workspace_bytes_ex(*g, 1)
    if entry == "gsr_backward_absgrad" and s["opt"] and s["opt"].get("absgrad"):
        return lib.gsr_workspace_bytes_absgrad(*g)
    if entry == "gsr_backward_features" and s["opt"] and s["opt"].get("dL_dfeaturemap") and s["opt"].get("dL_dfeatures") and 1 <= s["opt"]["channels"] <= 64:
        return lib.gsr_workspace_bytes_features(*g, s["opt"]["channels"], 0)
    if (s["ext"] or {}).get("out_depth") or (s["ext"] or {}).get("out_alpha") or (entry == "gsr_backward_distort" and s["opt"] and s["opt"].get("dL_ddistort")):
        return lib.gsr_workspace_bytes_depth_alpha(*g, 0)
    return lib.gsr_workspace_bytes_ex(*g, 0)


# ---- the op families -----------------------------------------------------------------------------------------------------------------------------------

def check_section(prefix, symbols, expected):
    """The functions the header declares with `prefix` are `symbols` (the _capi tuple) and `expected`, the list at the top of the header names them,
    the library exports every one, lib() has set each one's prototype from the table, and the ABI version is 4.  -> lib()"""
    names = declared(prefix)
    assert names == sorted(symbols) == expected
    assert "%sforward / %sbackward" % (prefix, prefix) in header().split("#ifndef GPSGS_H")[0]
    l, exported = lib(), raw()
    for name in names:
        assert hasattr(exported, name), name
        assert name in _capi.PROTOTYPES, name
        assert getattr(l, name).argtypes == _capi.PROTOTYPES[name][1] and getattr(l, name).restype is _capi.PROTOTYPES[name][0], name
    assert l.gpsgs_abi_version() == 4
    return l


# ---- the Python API without a GPU ----------------------------------------------------------------------------------------------------------------------

def cpu_view(grad=False):
    """-> (settings, kwargs) of GaussianRasterizer for four points in front of an 8 x 8 camera, every tensor on the CPU: a call the rasteriser must
    refuse before anything is launched.  grad: means3D and the camera tensors are leaves that require a gradient."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    view, proj, campos = torch.eye(4, requires_grad=grad), torch.eye(4, requires_grad=grad), torch.zeros(3, requires_grad=grad)
    rs = RZ.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, view, proj, 3, campos, False, False)
    x = torch.zeros(4, 3)
    return rs, dict(means3D=torch.zeros(4, 3, requires_grad=grad), means2D=x, opacities=torch.ones(4, 1), colors_precomp=x, scales=x, rotations=torch.zeros(4, 4))


# ---- the default workspace layout ----------------------------------------------------------------------------------------------------------------------

def assert_default_sizes(lib):
    """The default layout did not move: the training workspace sizes byte for byte, and each option's tail behind the depth / alpha size."""
    big = (600000, 1024, 1024, 5 << 20, 1024)
    assert lib.gsr_workspace_bytes(30000, 256, 256, 1 << 20) == 54450688
    assert lib.gsr_workspace_bytes_ex(*big, 0) == 454462464
    assert lib.gsr_workspace_bytes_ex(*big, 1) == 258065920
    da = lib.gsr_workspace_bytes_depth_alpha(*big, 0)
    assert da == lib.gsr_workspace_bytes_features(*big, 1, 0) - (5 << 20) * 4
    assert da == lib.gsr_workspace_bytes_contrib(*big, 0) - (5 << 20) * 16
    assert da == lib.gsr_workspace_bytes_absgrad(*big) - (5 << 20) * 8
