"""CPU: the opt-in camera gradients (include/gpsgs.h gsr_backward_camera) -- declarations, exports, the Python keywords and their defaults."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpsgs.h")
NEW = ("gsr_camera_grad_scratch_bytes", "gsr_backward_camera")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_new_symbols_are_declared_exported_and_mirrored():
    from gps_gaussian_amd import _capi
    src = _header()
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
    assert re.search(r"#define GPSGS_ABI_VERSION 4\b", _header())
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
    import ctypes as C
    from gps_gaussian_amd import _capi
    lib = _capi.lib()
    ext = _capi.GsrViewExt()
    null = [None] * 19
    # negative P / sizes: GPSGS_E_INVALID before anything touches a device
    rc = lib.gsr_backward_camera(-1, 16, 16, *null[:5], 1.0, 0.5, 0.5, *null[:3], None, *null[:7], None, 0, 0, 0, None, C.byref(ext),
                                 None, None, None, None, 0)
    assert rc == _capi.GPSGS_E_INVALID
    # misaligned output pointer
    rc = lib.gsr_backward_camera(0, 16, 16, *null[:5], 1.0, 0.5, 0.5, *null[:3], None, *null[:7], None, 0, 0, 0, None, C.byref(ext),
                                 2, None, None, None, 0)
    assert rc == _capi.GPSGS_E_INVALID


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
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    P = 4
    view = torch.eye(4, requires_grad=True)
    proj = torch.eye(4, requires_grad=True)
    campos = torch.zeros(3, requires_grad=True)
    rs = RZ.GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, view, proj, 3, campos, False, False)
    m3 = torch.zeros(P, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU"):
        RZ.GaussianRasterizer(rs)(means3D=m3, means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1), colors_precomp=torch.ones(P, 3),
                                  scales=torch.ones(P, 3), rotations=torch.ones(P, 4), camera_grad=True)
