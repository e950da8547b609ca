"""CPU: the opt-in camera gradients (include/gpsgs.h gsr_backward_camera) -- declarations, exports, the Python keywords and their defaults."""
import inspect
import re

import pytest

import capi_run
from capi_run import call, pointers, spec

NEW = ("gsr_camera_grad_scratch_bytes", "gsr_backward_camera")


def test_new_symbols_are_declared_exported_and_mirrored():
    from gps_gaussian_amd import _capi
    src = capi_run.header()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _capi.SYMBOLS, name
    lib = _capi.lib()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.gsr_backward_camera.argtypes[:-5] == lib.gsr_backward_ex.argtypes
    assert len(lib.gsr_backward_camera.argtypes) == len(lib.gsr_backward_ex.argtypes) + 5


def test_abi_and_view_ext_are_unchanged():
    import ctypes as C
    from gps_gaussian_amd import _capi
    assert re.search(r"#define GPSGS_ABI_VERSION 4\b", capi_run.header())
    assert _capi.lib().gpsgs_abi_version() == 4
    assert C.sizeof(_capi.GsrViewExt) == 80


def test_scratch_size():
    from gps_gaussian_amd import _capi
    f = _capi.lib().gsr_camera_grad_scratch_bytes
    assert f(0) == 0
    assert f(1) == 27 * 4
    assert f(256) == 27 * 4
    assert f(257) == 2 * 27 * 4
    assert f(600000) == 27 * 4 * ((600000 + 255) // 256)


def test_invalid_arguments_are_refused_without_a_device():
    from gps_gaussian_amd import _capi
    lib = _capi.lib()
    # every pointer NULL, a 16 x 16 image, no workspace, a zeroed GsrViewExt
    null = dict({k: None for k in pointers("gsr_backward_camera")}, W=16, H=16, cap=0, ext=dict(bin_capacity=0))
    # negative P / sizes: GPSGS_E_INVALID before anything touches a device
    assert call(lib, "gsr_backward_camera", spec("gsr_backward_camera", P=-1, **null)) == _capi.GPSGS_E_INVALID
    # misaligned output pointer
    assert call(lib, "gsr_backward_camera", spec("gsr_backward_camera", P=0, cam=dict(dL_dviewmatrix=2), **null)) == _capi.GPSGS_E_INVALID


@pytest.mark.parametrize("where", ["rasterize_gaussians", "GaussianRasterizer.forward", "render", "render_ex", "pts2render"])
def test_keyword_defaults_to_off(where):
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import render_api
    fn = {"rasterize_gaussians": RZ.rasterize_gaussians, "GaussianRasterizer.forward": RZ.GaussianRasterizer.forward,
          "render": render_api.render, "render_ex": render_api.render_ex, "pts2render": render_api.pts2render}[where]
    p = inspect.signature(fn).parameters
    assert "camera_grad" in p and p["camera_grad"].default is False


def test_settings_keep_twelve_fields():
    from gps_gaussian_amd import rasterizer as RZ
    assert len(RZ.GaussianRasterizationSettings._fields) == 12
    assert "camera_grad" not in RZ.GaussianRasterizationSettings._fields


def test_cpu_tensors_are_refused():
    from gps_gaussian_amd import rasterizer as RZ
    rs, kw = capi_run.cpu_view(grad=True)
    with pytest.raises(RuntimeError, match="GPU"):
        RZ.GaussianRasterizer(rs)(**kw, camera_grad=True)
