"""CPU: the C-ABI of the opt-in per-Gaussian contribution statistics -- GsrContrib as the C compiler lays it out equals the ctypes mirror, the new
entry points are exported and mirrored at ABI 4, the statistics workspace is the depth / alpha one plus an aligned 16-byte-per-slot tail (for a
forward-only caller too), the default sizes did not move, and the Python keywords are opt-in and refuse bad input before anything is launched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi


def test_contrib_struct_layout_is_mirrored(tmp_path):
    """The C compiler's offsets of GsrContrib equal the ctypes ones; GsrViewExt is still 80 bytes."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpsgs.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(GsrContrib), offsetof(GsrContrib, weight_sum), offsetof(GsrContrib, weight_max), offsetof(GsrContrib, pixel_count), "
                   "offsetof(GsrContrib, reserved), sizeof(GsrViewExt)); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    Cs = _capi.GsrContrib
    assert got == [C.sizeof(Cs), Cs.weight_sum.offset, Cs.weight_max.offset, Cs.pixel_count.offset, Cs.reserved.offset, C.sizeof(_capi.GsrViewExt)]
    assert got == [32, 0, 8, 16, 24, 80]
    c = Cs()
    assert c.weight_sum is None and c.weight_max is None and c.pixel_count is None and c.reserved is None  # zero-initialised = nothing wanted


def test_abi_version_and_symbols():
    lib = _capi.lib()
    assert lib.gpsgs_abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "gpsgs.h")).read()
    assert re.search(r"#define GPSGS_ABI_VERSION 4\b", hdr)
    for name in ("gsr_workspace_bytes_contrib", "gsr_forward_contrib"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, hdr)
    assert re.search(r"size_t gsr_workspace_bytes_contrib\(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, "
                     r"int forward_only\);", hdr)
    # the forward extends gsr_forward_ex's argument list by one GsrContrib pointer
    assert lib.gsr_forward_contrib.argtypes[:-1] == lib.gsr_forward_ex.argtypes
    assert lib.gsr_forward_contrib.argtypes[-1] == C.POINTER(_capi.GsrContrib)


@pytest.mark.parametrize("P,W,H,cap,bcap", [(30000, 256, 256, 1 << 20, 0), (600000, 1024, 1024, 5 << 20, 1024), (1, 8, 8, 1, 0), (0, 17, 9, 0, 0)])
def test_workspace_sizes(P, W, H, cap, bcap):
    lib = _capi.lib()
    da = lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, bcap, 0)
    full = lib.gsr_workspace_bytes_contrib(P, W, H, cap, bcap, 0)
    assert full >= da > 0 and full >= lib.gsr_workspace_bytes_ex(P, W, H, cap, bcap, 0)
    assert full - da == (max(cap, 1) * 16 + 255) // 256 * 256  # the contribution tail behind everything else
    # a forward-only caller needs the same: the gather reads the slot prefix of the backward tail
    assert lib.gsr_workspace_bytes_contrib(P, W, H, cap, bcap, 1) == full
    assert lib.gsr_workspace_bytes_contrib(P, W, H, 2 * cap + 4096, bcap, 0) > full  # grows with the capacity
    assert lib.gsr_workspace_bytes_contrib(-1, W, H, cap, bcap, 0) == 0
    assert lib.gsr_workspace_bytes_contrib(P, W, H, -1, bcap, 0) == 0
    assert lib.gsr_workspace_bytes_contrib(P, W, H, cap, 100, 0) == 0  # not a valid direct-list capacity


def test_default_workspace_sizes_are_pinned():
    """The default layout did not move (the parent commit's sizes, byte for byte)."""
    lib = _capi.lib()
    assert lib.gsr_workspace_bytes(30000, 256, 256, 1 << 20) == 54450688
    assert lib.gsr_workspace_bytes_ex(600000, 1024, 1024, 5 << 20, 1024, 0) == 454462464
    assert lib.gsr_workspace_bytes_ex(600000, 1024, 1024, 5 << 20, 1024, 1) == 258065920
    da = lib.gsr_workspace_bytes_depth_alpha(600000, 1024, 1024, 5 << 20, 1024, 0)
    assert da == lib.gsr_workspace_bytes_features(600000, 1024, 1024, 5 << 20, 1024, 1, 0) - (5 << 20) * 4


# P = 1, an 8 x 8 image, every pointer set (never dereferenced: each call returns before anything is launched) and a workspace of 0 bytes: a
# VALID statistics set gets as far as the workspace check (GPSGS_E_WORKSPACE), so GPSGS_E_INVALID can only come from the statistics' validation
_D = 0x1000  # a 4-byte aligned dummy device address


def _fwd_args(ws_bytes=0):
    return [1, 8, 8] + [_D] * 5 + [1.0, 0.5, 0.5] + [_D] * 6 + [ws_bytes, 1024, 0, None, None, 0, None]


def _contrib(s=_D, m=_D, n=_D, reserved=None):
    c = _capi.GsrContrib()
    c.weight_sum, c.weight_max, c.pixel_count, c.reserved = s, m, n, reserved
    return c


@pytest.mark.parametrize("bad", [dict(s=_D + 2), dict(m=_D + 1), dict(n=_D + 3), dict(s=None, m=None, n=_D + 2), dict(reserved=_D)])
def test_forward_validates_before_launch(bad):
    lib = _capi.lib()
    assert lib.gsr_forward_contrib(*_fwd_args(), C.byref(_contrib())) == _capi.GPSGS_E_WORKSPACE  # the valid control
    assert lib.gsr_forward_contrib(*_fwd_args(), C.byref(_contrib(**bad))) == _capi.GPSGS_E_INVALID


def test_forward_needs_the_contribution_tail():
    """With any statistic wanted, a workspace of the depth / alpha size (no tail) is too small, and so is one byte short of the statistics size."""
    lib = _capi.lib()
    da = lib.gsr_workspace_bytes_depth_alpha(1, 8, 8, 1024, 0, 0)
    full = lib.gsr_workspace_bytes_contrib(1, 8, 8, 1024, 0, 0)
    assert full > da
    for nbytes in (da, full - 1):
        assert lib.gsr_forward_contrib(*_fwd_args(nbytes), C.byref(_contrib(s=None, m=None))) == _capi.GPSGS_E_WORKSPACE


def test_python_api_is_opt_in():
    """The keywords default to off; a CPU tensor and the combination with features are refused before anything is launched."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import render_api
    assert inspect.signature(RZ.rasterize_gaussians).parameters["return_contrib"].default is False
    assert inspect.signature(RZ.GaussianRasterizer.forward).parameters["return_contrib"].default is False
    assert inspect.signature(render_api.render_ex).parameters["contrib"].default is False
    assert inspect.signature(render_api.pts2render).parameters["with_contrib"].default is False
    assert list(inspect.signature(render_api.render_ex).parameters)[:8] == ["data", "idx", "pts_xyz", "pts_rgb", "rotations", "scales", "opacity", "bg_color"]
    assert list(inspect.signature(render_api.pts2render).parameters)[:2] == ["data", "bg_color"]
    rs = RZ.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3), False, False)
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        RZ.GaussianRasterizer(rs)(means3D=x, means2D=x, opacities=torch.ones(4, 1), colors_precomp=x, scales=x, rotations=torch.zeros(4, 4),
                                  return_contrib=True)
    with pytest.raises(RuntimeError, match="with_contrib cannot be combined with feature_key"):
        render_api.pts2render({"lmain": {"img": torch.zeros(1, 3, 8, 8)}}, [0, 0, 0], feature_key="sem", with_contrib=True)
