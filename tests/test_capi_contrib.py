"""CPU: the C-ABI of the opt-in per-Gaussian contribution statistics -- GsrContrib as the C compiler lays it out equals the ctypes mirror, the new
entry points are exported and mirrored at ABI 4, the statistics workspace is the depth / alpha one plus an aligned 16-byte-per-slot tail (for a
forward-only caller too), the default sizes did not move, and the Python keywords are opt-in and refuse bad input before anything is launched."""
import ctypes as C
import inspect
import re

import pytest

from gps_gaussian_amd import _capi

import capi_run
from capi_run import D, call, spec


def test_contrib_struct_layout_is_mirrored(tmp_path):
    """The C compiler's offsets of GsrContrib equal the ctypes ones; GsrViewExt is still 80 bytes."""
    got = capi_run.c_values(tmp_path, ["sizeof(GsrContrib)", "offsetof(GsrContrib, weight_sum)", "offsetof(GsrContrib, weight_max)",
                                       "offsetof(GsrContrib, pixel_count)", "offsetof(GsrContrib, reserved)", "sizeof(GsrViewExt)"])
    Cs = _capi.GsrContrib
    assert got == [C.sizeof(Cs), Cs.weight_sum.offset, Cs.weight_max.offset, Cs.pixel_count.offset, Cs.reserved.offset, C.sizeof(_capi.GsrViewExt)]
    assert got == [32, 0, 8, 16, 24, 80]
    c = Cs()
    assert c.weight_sum is None and c.weight_max is None and c.pixel_count is None and c.reserved is None  # zero-initialised = nothing wanted


def test_abi_version_and_symbols():
    lib = capi_run.lib()
    assert lib.gpsgs_abi_version() == 4
    hdr = capi_run.header()
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
    lib = capi_run.lib()
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
    capi_run.assert_default_sizes(capi_run.lib())


# spec("gsr_forward_contrib"): P = 1, an 8 x 8 image, every pointer set (never dereferenced: each call returns before anything is launched) and a
# workspace of 0 bytes: a VALID statistics set gets as far as the workspace check (GPSGS_E_WORKSPACE), so GPSGS_E_INVALID can only come from the
# statistics' validation
def _contrib(lib, ws=0, **opt):
    return call(lib, "gsr_forward_contrib", spec("gsr_forward_contrib", ws=ws, opt=opt))


@pytest.mark.parametrize("bad", [dict(weight_sum=D + 2), dict(weight_max=D + 1), dict(pixel_count=D + 3),
                                 dict(weight_sum=None, weight_max=None, pixel_count=D + 2), dict(reserved=D)])
def test_forward_validates_before_launch(bad):
    lib = capi_run.lib()
    assert _contrib(lib) == _capi.GPSGS_E_WORKSPACE  # the valid control
    assert _contrib(lib, **bad) == _capi.GPSGS_E_INVALID


def test_forward_needs_the_contribution_tail():
    """With any statistic wanted, a workspace of the depth / alpha size (no tail) is too small, and so is one byte short of the statistics size."""
    lib = capi_run.lib()
    da = lib.gsr_workspace_bytes_depth_alpha(1, 8, 8, 1024, 0, 0)
    full = lib.gsr_workspace_bytes_contrib(1, 8, 8, 1024, 0, 0)
    assert full > da
    for nbytes in (da, full - 1):
        assert _contrib(lib, nbytes, weight_sum=None, weight_max=None) == _capi.GPSGS_E_WORKSPACE


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
    rs, kw = capi_run.cpu_view()
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        RZ.GaussianRasterizer(rs)(**kw, return_contrib=True)
    with pytest.raises(RuntimeError, match="with_contrib cannot be combined with feature_key"):
        render_api.pts2render({"lmain": {"img": torch.zeros(1, 3, 8, 8)}}, [0, 0, 0], feature_key="sem", with_contrib=True)
