"""CPU: the C-ABI of the opt-in absolute screen-space gradient -- GsrAbsGrad as the C compiler lays it out equals the ctypes mirror, the new entry
points are exported and mirrored at ABI 4, the absgrad workspace is the depth / alpha one plus an aligned 8-byte-per-slot tail that fits inside a
statistics workspace, the default sizes did not move, and the Python keywords are opt-in and refuse bad input before anything is launched."""
import ctypes as C
import inspect
import re

import pytest

from gps_gaussian_amd import _capi

import capi_run
from capi_run import D, call, spec


def test_absgrad_struct_layout_is_mirrored(tmp_path):
    """The C compiler's offsets of GsrAbsGrad equal the ctypes ones; GsrViewExt is still 80 bytes."""
    got = capi_run.c_values(tmp_path, ["sizeof(GsrAbsGrad)", "offsetof(GsrAbsGrad, absgrad)", "offsetof(GsrAbsGrad, reserved)", "sizeof(GsrViewExt)"])
    A = _capi.GsrAbsGrad
    assert got == [C.sizeof(A), A.absgrad.offset, A.reserved.offset, C.sizeof(_capi.GsrViewExt)]
    assert got == [16, 0, 8, 80]
    a = A()
    assert a.absgrad is None and a.reserved is None  # zero-initialised = nothing wanted


def test_abi_version_and_symbols():
    lib = capi_run.lib()
    assert lib.gpsgs_abi_version() == 4
    hdr = capi_run.header()
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
    lib = capi_run.lib()
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
    capi_run.assert_default_sizes(capi_run.lib())


# spec("gsr_backward_absgrad"): P = 1, an 8 x 8 image, every pointer set (never dereferenced: each call returns before anything is launched) and a
# workspace of 0 bytes: a VALID GsrAbsGrad gets as far as the workspace check (GPSGS_E_WORKSPACE), so GPSGS_E_INVALID can only come from its validation
def _absgrad(lib, ws=0, **opt):
    return call(lib, "gsr_backward_absgrad", spec("gsr_backward_absgrad", ws=ws, opt=opt))


@pytest.mark.parametrize("bad", [dict(absgrad=D + 2), dict(absgrad=D + 1), dict(reserved=D), dict(absgrad=None, reserved=D)])
def test_backward_validates_before_launch(bad):
    lib = capi_run.lib()
    assert _absgrad(lib) == _capi.GPSGS_E_WORKSPACE  # the valid control
    assert _absgrad(lib, **bad) == _capi.GPSGS_E_INVALID


def test_backward_needs_the_absgrad_tail():
    """With absgrad wanted, a workspace of the depth / alpha size (no tail) is too small, and so is one byte short of the absgrad size; a NULL struct or
    a NULL pointer asks for nothing more than gsr_backward_camera does."""
    lib = capi_run.lib()
    da = lib.gsr_workspace_bytes_depth_alpha(1, 8, 8, 1024, 0, 0)
    full = lib.gsr_workspace_bytes_absgrad(1, 8, 8, 1024, 0)
    assert full > da
    for nbytes in (da, full - 1):
        assert _absgrad(lib, nbytes) == _capi.GPSGS_E_WORKSPACE
    plain = lib.gsr_workspace_bytes_ex(1, 8, 8, 1024, 0, 0)
    for opt in (None, dict(absgrad=None)):
        assert call(lib, "gsr_backward_absgrad", spec("gsr_backward_absgrad", ws=plain - 1, opt=opt)) == _capi.GPSGS_E_WORKSPACE
        assert call(lib, "gsr_backward_camera", spec("gsr_backward_camera", ws=plain - 1)) == _capi.GPSGS_E_WORKSPACE


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
    rs, kw = capi_run.cpu_view()
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        RZ.GaussianRasterizer(rs)(**kw, return_absgrad=True)
    with pytest.raises(RuntimeError, match="features"):
        RZ.GaussianRasterizer(rs)(**kw, return_absgrad=True, features=torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="features"):
        render_api.pts2render({"lmain": {"img": torch.zeros(1, 3, 8, 8)}}, [0, 0, 0], feature_key="sem", with_absgrad=True)
