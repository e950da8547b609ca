"""CPU: the C-ABI of the opt-in depth / alpha maps -- GsrViewExt keeps its 80-byte layout (the maps take the former reserved words, ABI 4),
the ctypes mirror matches the header, and the workspace of the depth / alpha backward is the default one plus one float per instance slot."""
import ctypes as C
import re

import pytest

from gps_gaussian_amd import _capi

import capi_run


def test_view_ext_layout_is_unchanged_and_mirrored(tmp_path):
    """The C compiler's offsets of the new fields equal the ctypes ones; the struct is still 80 bytes; forward outputs and backward gradients share
    their slots."""
    got = capi_run.c_values(tmp_path, ["sizeof(GsrViewExt)", "offsetof(GsrViewExt, dL_dcov3D)", "offsetof(GsrViewExt, out_depth)",
                                       "offsetof(GsrViewExt, dL_ddepth)", "offsetof(GsrViewExt, out_alpha)", "offsetof(GsrViewExt, dL_dalpha)"])
    E = _capi.GsrViewExt
    assert got == [80, 56, 64, 64, 72, 72]
    assert [C.sizeof(E), E.dL_dcov3D.offset, E._depth.offset, E._alpha.offset] == [80, 56, 64, 72]
    e = E()
    assert e.out_depth is None and e.out_alpha is None  # zero-initialised = no maps (what every existing caller passes)
    e.out_depth, e.dL_dalpha = 0x1000, 0x2000
    assert e.dL_ddepth == 0x1000 and e.out_alpha == 0x2000


def test_abi_version_and_symbols():
    lib = capi_run.lib()
    assert lib.gpsgs_abi_version() == 4
    assert "gsr_workspace_bytes_depth_alpha" in _capi.SYMBOLS
    hdr = capi_run.header()
    assert re.search(r"size_t gsr_workspace_bytes_depth_alpha\(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, "
                     r"int forward_only\);", hdr)


@pytest.mark.parametrize("P,W,H,cap,bcap", [(30000, 256, 256, 1 << 20, 0), (600000, 1024, 1024, 5 << 20, 1024), (2400000, 2048, 2048, 30 << 20, 1024),
                                              (1, 8, 8, 1, 0), (0, 17, 9, 0, 0)])
def test_workspace_sizes(P, W, H, cap, bcap):
    lib = capi_run.lib()
    plain = lib.gsr_workspace_bytes_ex(P, W, H, cap, bcap, 0)
    extra = lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, bcap, 0)
    assert plain > 0
    assert extra - plain == (max(cap, 1) * 4 + 255) // 256 * 256  # inst_ddepth behind everything else
    assert lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, bcap, 1) == lib.gsr_workspace_bytes_ex(P, W, H, cap, bcap, 1)
    if bcap == 0:
        assert plain == lib.gsr_workspace_bytes(P, W, H, cap)
    assert lib.gsr_workspace_bytes_depth_alpha(-1, W, H, cap, bcap, 0) == 0
    assert lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, 100, 0) == 0  # not a valid direct-list capacity


def test_default_workspace_sizes_are_pinned():
    """The default layout did not move: the training workspace sizes of the parent commit, byte for byte."""
    capi_run.assert_default_sizes(capi_run.lib())


def test_python_api_is_opt_in():
    """rasterize_gaussians / GaussianRasterizer.forward / render_api take the maps as keyword opt-ins; the default signatures still work as before
    (no GPU: the call is refused for CPU tensors before anything is launched)."""
    import inspect
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import render_api
    assert inspect.signature(RZ.rasterize_gaussians).parameters["return_depth_alpha"].default is False
    assert inspect.signature(RZ.GaussianRasterizer.forward).parameters["return_depth_alpha"].default is False
    assert inspect.signature(render_api.pts2render).parameters["with_depth_alpha"].default is False
    assert list(inspect.signature(render_api.render_ex).parameters)[:8] == ["data", "idx", "pts_xyz", "pts_rgb", "rotations", "scales", "opacity", "bg_color"]
    rs, kw = capi_run.cpu_view()
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        RZ.GaussianRasterizer(rs)(**kw, return_depth_alpha=True)
