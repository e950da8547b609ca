"""CPU: the C-ABI of the opt-in absolute screen-space gradient -- GsrAbsGrad as the C compiler lays it out equals the ctypes mirror, the new entry
points are exported and mirrored at ABI 4, the absgrad workspace is the depth / alpha one plus an aligned 8-byte-per-slot tail that fits inside a
statistics workspace, the default sizes did not move, and the Python keywords are opt-in and refuse bad input before anything is launched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi


def test_absgrad_struct_layout_is_mirrored(tmp_path):
    """The C compiler's offsets of GsrAbsGrad equal the ctypes ones; GsrViewExt is still 80 bytes."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpsgs.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   "sizeof(GsrAbsGrad), offsetof(GsrAbsGrad, absgrad), offsetof(GsrAbsGrad, reserved), sizeof(GsrViewExt)); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    A = _capi.GsrAbsGrad
    assert got == [C.sizeof(A), A.absgrad.offset, A.reserved.offset, C.sizeof(_capi.GsrViewExt)]
    assert got == [16, 0, 8, 80]
    a = A()
    assert a.absgrad is None and a.reserved is None  # zero-initialised = nothing wanted


def test_abi_version_and_symbols():
    lib = _capi.lib()
    assert lib.gpsgs_abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "gpsgs.h")).read()
    assert re.search(r"#define GPSGS_ABI_VERSION 4\b", hdr)
    for name in ("gsr_workspace_bytes_absgrad", "gsr_backward_absgrad"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, hdr)
    assert re.search(r"size_t gsr_workspace_bytes_absgrad\(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity\);", hdr)
    assert not re.search(r"GSR_FLAG_\w*ABS", hdr)  # no new flag: the request is the pointer
    # the backward extends gsr_backward_camera's argument list by one GsrAbsGrad pointer
    assert lib.gsr_backward_absgrad.argtypes[:-1] == lib.gsr_backward_camera.argtypes
    assert lib.gsr_backward_absgrad.argtypes[-1] == C.POINTER(_capi.GsrAbsGrad)


@pytest.mark.parametrize("P,W,H,cap,bcap", [(30000, 256, 256, 1 << 20, 0), (600000, 1024, 1024, 5 << 20, 1024), (1, 8, 8, 1, 0), (0, 17, 9, 0, 0)])
def test_workspace_sizes(P, W, H, cap, bcap):
    lib = _capi.lib()
    da = lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, bcap, 0)
    full = lib.gsr_workspace_bytes_absgrad(P, W, H, cap, bcap)
    assert full > da > 0 and full > lib.gsr_workspace_bytes_ex(P, W, H, cap, bcap, 0)
    assert full - da == (max(cap, 1) * 8 + 255) // 256 * 256  # the absgrad tail behind everything else
    assert full <= lib.gsr_workspace_bytes_contrib(P, W, H, cap, bcap, 0)  # a statistics workspace serves an absgrad backward
    assert lib.gsr_workspace_bytes_absgrad(P, W, H, 2 * cap + 4096, bcap) > full  # grows with the capacity
    assert lib.gsr_workspace_bytes_absgrad(-1, W, H, cap, bcap) == 0
    assert lib.gsr_workspace_bytes_absgrad(P, W, H, -1, bcap) == 0
    assert lib.gsr_workspace_bytes_absgrad(P, W, H, cap, 100) == 0  # not a valid direct-list capacity


def test_default_workspace_sizes_are_pinned():
    """The default layout did not move (the parent commit's sizes, byte for byte)."""
    lib = _capi.lib()
    assert lib.gsr_workspace_bytes(30000, 256, 256, 1 << 20) == 54450688
    assert lib.gsr_workspace_bytes_ex(600000, 1024, 1024, 5 << 20, 1024, 0) == 454462464
    assert lib.gsr_workspace_bytes_ex(600000, 1024, 1024, 5 << 20, 1024, 1) == 258065920
    da = lib.gsr_workspace_bytes_depth_alpha(600000, 1024, 1024, 5 << 20, 1024, 0)
    assert da == lib.gsr_workspace_bytes_features(600000, 1024, 1024, 5 << 20, 1024, 1, 0) - (5 << 20) * 4
    assert da == lib.gsr_workspace_bytes_contrib(600000, 1024, 1024, 5 << 20, 1024, 0) - (5 << 20) * 16


# P = 1, an 8 x 8 image, every pointer set (never dereferenced: each call returns before anything is launched) and a workspace of 0 bytes: a VALID
# GsrAbsGrad gets as far as the workspace check (GPSGS_E_WORKSPACE), so GPSGS_E_INVALID can only come from its validation
_D = 0x1000  # a 4-byte aligned dummy device address


def _bwd_args(ws_bytes=0):
    # P W H | means3D colors opacities scales rotations | modifier tanfovx tanfovy | view proj bg radii dL_dpix | six gradient arrays | workspace,
    # bytes, capacity, flags, stream, ext | three camera gradients, scratch, scratch bytes
    return [1, 8, 8] + [_D] * 5 + [1.0, 0.5, 0.5] + [_D] * 5 + [_D] * 6 + [_D, ws_bytes, 1024, 0, None, None] + [None, None, None, None, 0]


def _abs(p=_D, reserved=None):
    a = _capi.GsrAbsGrad()
    a.absgrad, a.reserved = p, reserved
    return a


@pytest.mark.parametrize("bad", [dict(p=_D + 2), dict(p=_D + 1), dict(reserved=_D), dict(p=None, reserved=_D)])
def test_backward_validates_before_launch(bad):
    lib = _capi.lib()
    assert len(_bwd_args()) == len(lib.gsr_backward_camera.argtypes)
    assert lib.gsr_backward_absgrad(*_bwd_args(), C.byref(_abs())) == _capi.GPSGS_E_WORKSPACE  # the valid control
    assert lib.gsr_backward_absgrad(*_bwd_args(), C.byref(_abs(**bad))) == _capi.GPSGS_E_INVALID


def test_backward_needs_the_absgrad_tail():
    """With absgrad wanted, a workspace of the depth / alpha size (no tail) is too small, and so is one byte short of the absgrad size; a NULL struct or
    a NULL pointer asks for nothing more than gsr_backward_camera does."""
    lib = _capi.lib()
    da = lib.gsr_workspace_bytes_depth_alpha(1, 8, 8, 1024, 0, 0)
    full = lib.gsr_workspace_bytes_absgrad(1, 8, 8, 1024, 0)
    assert full > da
    for nbytes in (da, full - 1):
        assert lib.gsr_backward_absgrad(*_bwd_args(nbytes), C.byref(_abs())) == _capi.GPSGS_E_WORKSPACE
    plain = lib.gsr_workspace_bytes_ex(1, 8, 8, 1024, 0, 0)
    for a in (None, C.byref(_abs(p=None))):
        assert lib.gsr_backward_absgrad(*_bwd_args(plain - 1), a) == _capi.GPSGS_E_WORKSPACE
        assert lib.gsr_backward_camera(*_bwd_args(plain - 1)) == _capi.GPSGS_E_WORKSPACE


def test_python_api_is_opt_in():
    """The keywords default to off on all four entry points; a CPU tensor and the combination with features are refused before anything is launched."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import render_api
    assert inspect.signature(RZ.rasterize_gaussians).parameters["return_absgrad"].default is False
    assert inspect.signature(RZ.GaussianRasterizer.forward).parameters["return_absgrad"].default is False
    assert inspect.signature(render_api.render_ex).parameters["absgrad"].default is False
    assert inspect.signature(render_api.pts2render).parameters["with_absgrad"].default is False
    assert list(inspect.signature(render_api.render_ex).parameters)[:8] == ["data", "idx", "pts_xyz", "pts_rgb", "rotations", "scales", "opacity", "bg_color"]
    assert list(inspect.signature(render_api.pts2render).parameters)[:2] == ["data", "bg_color"]
    rs = RZ.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3), False, False)
    x = torch.zeros(4, 3)
    kw = dict(means3D=x, means2D=x, opacities=torch.ones(4, 1), colors_precomp=x, scales=x, rotations=torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        RZ.GaussianRasterizer(rs)(**kw, return_absgrad=True)
    with pytest.raises(RuntimeError, match="features"):
        RZ.GaussianRasterizer(rs)(**kw, return_absgrad=True, features=torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="features"):
        render_api.pts2render({"lmain": {"img": torch.zeros(1, 3, 8, 8)}}, [0, 0, 0], feature_key="sem", with_absgrad=True)
