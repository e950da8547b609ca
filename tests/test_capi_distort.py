"""CPU: the C-ABI of the opt-in depth-distortion map -- GsrDistort as the C compiler lays it out equals the ctypes mirror, the two new entry points are
exported and mirrored at ABI 4 with GsrViewExt still 80 bytes, a valid struct gets as far as the workspace check while every bad one is refused
before it, the workspace asked for is the depth / alpha one (no new tail, no new size function), the default sizes did not move, and the Python
keywords are opt-in, come last and refuse bad input before anything is launched."""
import ctypes as C
import inspect
import re

import pytest

from gps_gaussian_amd import _capi

import capi_run
from capi_run import D, call, need, spec

FWD, BWD = "gsr_forward_distort", "gsr_backward_distort"


def test_distort_struct_layout_is_mirrored(tmp_path):
    """The C compiler's offsets of GsrDistort equal the ctypes ones; the map pointers share their slot; GsrViewExt is still 80 bytes."""
    got = capi_run.c_values(tmp_path, ["sizeof(GsrDistort)", "offsetof(GsrDistort, out_distort)", "offsetof(GsrDistort, dL_ddistort)",
                                       "offsetof(GsrDistort, totals)", "offsetof(GsrDistort, reserved)", "sizeof(GsrViewExt)"])
    Ds = _capi.GsrDistort
    assert got == [C.sizeof(Ds), Ds._map.offset + _capi._DistortSlot.out_distort.offset, Ds._map.offset + _capi._DistortSlot.dL_ddistort.offset,
                   Ds.totals.offset, Ds.reserved.offset, C.sizeof(_capi.GsrViewExt)]
    assert got == [32, 0, 0, 8, 16, 80]
    d = Ds()
    assert d.out_distort is None and d.dL_ddistort is None and d.totals is None and list(d.reserved) == [None, None]  # zero-initialised = nothing wanted
    d.out_distort = 0x1000
    assert d.dL_ddistort == 0x1000  # one slot


def test_abi_version_and_symbols():
    lib = capi_run.lib()
    assert lib.gpsgs_abi_version() == 4
    hdr = capi_run.header()
    assert re.search(r"#define GPSGS_ABI_VERSION 4\b", hdr)
    for name in (FWD, BWD):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, hdr)
    assert not re.search(r"gsr_workspace_bytes_distort", hdr) and not hasattr(lib, "gsr_workspace_bytes_distort")  # no new size function
    assert not re.search(r"GSR_FLAG_\w*DIST", hdr)  # no new flag: the request is the pointer
    # the entry points extend gsr_forward_ex's and gsr_backward_camera's argument lists by one GsrDistort pointer
    assert lib.gsr_forward_distort.argtypes[:-1] == lib.gsr_forward_ex.argtypes
    assert lib.gsr_backward_distort.argtypes[:-1] == lib.gsr_backward_camera.argtypes
    assert lib.gsr_forward_distort.argtypes[-1] == lib.gsr_backward_distort.argtypes[-1] == C.POINTER(_capi.GsrDistort)


def test_default_workspace_sizes_are_pinned():
    """The layout did not move: the constants and the tails behind the depth / alpha size."""
    capi_run.assert_default_sizes(capi_run.lib())


# spec(FWD) / spec(BWD): P = 1, an 8 x 8 image, every pointer set (never dereferenced: each call returns before anything is launched) and a workspace
# of 0 bytes: a VALID GsrDistort gets as far as the workspace check (GPSGS_E_WORKSPACE), so GPSGS_E_INVALID can only come from its validation
def _distort(lib, entry, ws=0, **opt):
    """`map`: the entry point's own name of the shared slot, out_distort (forward) / dL_ddistort (backward)."""
    if "map" in opt:
        opt["out_distort" if entry == FWD else "dL_ddistort"] = opt.pop("map")
    return call(lib, entry, spec(entry, ws=ws, opt=opt))


_BAD = [dict(map=D + 2), dict(map=D + 1), dict(totals=D + 0x1002), dict(totals=None), dict(reserved=(D, None)), dict(reserved=(None, D)),
        dict(map=None, reserved=(D, None)), dict(map=None, totals=D + 1)]


@pytest.mark.parametrize("bad", _BAD)
def test_forward_validates_before_launch(bad):
    lib = capi_run.lib()
    assert _distort(lib, FWD) == _capi.GPSGS_E_WORKSPACE  # the valid control
    assert _distort(lib, FWD, **bad) == _capi.GPSGS_E_INVALID


@pytest.mark.parametrize("bad", _BAD)
def test_backward_validates_before_launch(bad):
    lib = capi_run.lib()
    assert _distort(lib, BWD) == _capi.GPSGS_E_WORKSPACE  # the valid control
    assert _distort(lib, BWD, **bad) == _capi.GPSGS_E_INVALID


def test_the_depth_alpha_workspace_is_required():
    """With the map's gradient wanted the backward needs gsr_workspace_bytes_depth_alpha(..., 0) -- the plain size is too small, and so is one byte
    less; the forward needs the forward-only size; a NULL struct or a NULL map pointer asks for nothing more than the call without the option."""
    lib = capi_run.lib()
    dims = (1, 8, 8, 1024, 0)
    da, plain = lib.gsr_workspace_bytes_depth_alpha(*dims, 0), lib.gsr_workspace_bytes_ex(*dims, 0)
    assert da > plain and need(lib, BWD, spec(BWD)) == da
    for nbytes in (plain, da - 1):
        assert _distort(lib, BWD, nbytes) == _capi.GPSGS_E_WORKSPACE
    for opt in (None, dict(dL_ddistort=None), dict(dL_ddistort=None, totals=None)):
        assert need(lib, BWD, spec(BWD, opt=opt)) == plain
        assert call(lib, BWD, spec(BWD, ws=plain - 1, opt=opt)) == _capi.GPSGS_E_WORKSPACE
        assert call(lib, "gsr_backward_camera", spec("gsr_backward_camera", ws=plain - 1)) == _capi.GPSGS_E_WORKSPACE
    fwd = lib.gsr_workspace_bytes_depth_alpha(*dims, 1)
    assert fwd == lib.gsr_workspace_bytes_ex(*dims, 1) == need(lib, FWD, spec(FWD))
    assert _distort(lib, FWD, fwd - 1) == _capi.GPSGS_E_WORKSPACE
    assert call(lib, "gsr_forward_ex", spec("gsr_forward_ex", ws=fwd - 1)) == _capi.GPSGS_E_WORKSPACE


def test_python_api_is_opt_in():
    """The keywords default to off and come last on all four entry points; a CPU tensor and the combinations with features, the statistics and
    absgrad are refused before anything is launched."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import render_api
    for fn, name in ((RZ.rasterize_gaussians, "return_distortion"), (RZ.GaussianRasterizer.forward, "return_distortion"),
                     (render_api.render_ex, "distortion"), (render_api.pts2render, "with_distortion")):
        params = inspect.signature(fn).parameters
        assert params[name].default is False and list(params)[-1] == name
    assert list(inspect.signature(render_api.render_ex).parameters)[:8] == ["data", "idx", "pts_xyz", "pts_rgb", "rotations", "scales", "opacity", "bg_color"]
    assert list(inspect.signature(render_api.pts2render).parameters)[:2] == ["data", "bg_color"]
    assert RZ._ViewOptions._fields[-1] == "distortion" and RZ._DEFAULT_OPTIONS.distortion is False
    assert RZ._Outputs._fields[-1] == "distortion"
    rs, kw = capi_run.cpu_view()
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        RZ.GaussianRasterizer(rs)(**kw, return_distortion=True)
    with pytest.raises(RuntimeError, match="return_distortion cannot be combined with features"):
        RZ.GaussianRasterizer(rs)(**kw, return_distortion=True, features=torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="return_distortion cannot be combined with return_contrib"):
        RZ.GaussianRasterizer(rs)(**kw, return_distortion=True, return_contrib=True)
    with pytest.raises(RuntimeError, match="return_distortion cannot be combined with return_absgrad"):
        RZ.GaussianRasterizer(rs)(**kw, return_distortion=True, return_absgrad=True)
    data = {"lmain": {"img": torch.zeros(1, 3, 8, 8)}}
    for kw2, what in ((dict(feature_key="sem"), "features"), (dict(with_contrib=True), "with_contrib"), (dict(with_absgrad=True), "with_absgrad")):
        with pytest.raises(RuntimeError, match="with_distortion cannot be combined with .*%s" % what):
            render_api.pts2render(data, [0, 0, 0], with_distortion=True, **kw2)
