"""CPU: the C-ABI of the opt-in depth-distortion map -- GsrDistort as the C compiler lays it out equals the ctypes mirror, the two new entry points are
exported and mirrored at ABI 4 with GsrViewExt still 80 bytes, a valid struct gets as far as the workspace check while every bad one is refused
before it, the workspace asked for is the depth / alpha one (no new tail, no new size function), the default sizes did not move, and the Python
keywords are opt-in, come last and refuse bad input before anything is launched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

import gps_gaussian_amd  # noqa: F401
from gps_gaussian_amd import _capi


def test_distort_struct_layout_is_mirrored(tmp_path):
    """The C compiler's offsets of GsrDistort equal the ctypes ones; the map pointers share their slot; GsrViewExt is still 80 bytes."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpsgs.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(GsrDistort), offsetof(GsrDistort, out_distort), offsetof(GsrDistort, dL_ddistort), offsetof(GsrDistort, totals), "
                   "offsetof(GsrDistort, reserved), sizeof(GsrViewExt)); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    D = _capi.GsrDistort
    assert got == [C.sizeof(D), D._map.offset + _capi._DistortSlot.out_distort.offset, D._map.offset + _capi._DistortSlot.dL_ddistort.offset,
                   D.totals.offset, D.reserved.offset, C.sizeof(_capi.GsrViewExt)]
    assert got == [32, 0, 0, 8, 16, 80]
    d = D()
    assert d.out_distort is None and d.dL_ddistort is None and d.totals is None and list(d.reserved) == [None, None]  # zero-initialised = nothing wanted
    d.out_distort = 0x1000
    assert d.dL_ddistort == 0x1000  # one slot


def test_abi_version_and_symbols():
    lib = _capi.lib()
    assert lib.gpsgs_abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "gpsgs.h")).read()
    assert re.search(r"#define GPSGS_ABI_VERSION 4\b", hdr)
    for name in ("gsr_forward_distort", "gsr_backward_distort"):
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
    """The layout did not move: the constants tests/test_capi_absgrad.py pins, and the tails behind the depth / alpha size."""
    lib = _capi.lib()
    assert lib.gsr_workspace_bytes(30000, 256, 256, 1 << 20) == 54450688
    assert lib.gsr_workspace_bytes_ex(600000, 1024, 1024, 5 << 20, 1024, 0) == 454462464
    assert lib.gsr_workspace_bytes_ex(600000, 1024, 1024, 5 << 20, 1024, 1) == 258065920
    da = lib.gsr_workspace_bytes_depth_alpha(600000, 1024, 1024, 5 << 20, 1024, 0)
    assert da == lib.gsr_workspace_bytes_features(600000, 1024, 1024, 5 << 20, 1024, 1, 0) - (5 << 20) * 4
    assert da == lib.gsr_workspace_bytes_contrib(600000, 1024, 1024, 5 << 20, 1024, 0) - (5 << 20) * 16
    assert da == lib.gsr_workspace_bytes_absgrad(600000, 1024, 1024, 5 << 20, 1024) - (5 << 20) * 8


# P = 1, an 8 x 8 image, every pointer set (never dereferenced: each call returns before anything is launched) and a workspace of 0 bytes: a VALID
# GsrDistort gets as far as the workspace check (GPSGS_E_WORKSPACE), so GPSGS_E_INVALID can only come from its validation
_D = 0x1000  # a 4-byte aligned dummy device address


def _fwd_args(ws_bytes=0):
    # P W H | means3D colors opacities scales rotations | modifier tanfovx tanfovy | view proj bg out_color radii | workspace, bytes, capacity, flags,
    # stream | host header, sequence | ext
    return [1, 8, 8] + [_D] * 5 + [1.0, 0.5, 0.5] + [_D] * 5 + [_D, ws_bytes, 1024, 0, None] + [None, 0] + [None]


def _bwd_args(ws_bytes=0):
    # P W H | means3D colors opacities scales rotations | modifier tanfovx tanfovy | view proj bg radii dL_dpix | six gradient arrays | workspace,
    # bytes, capacity, flags, stream, ext | three camera gradients, scratch, scratch bytes
    return [1, 8, 8] + [_D] * 5 + [1.0, 0.5, 0.5] + [_D] * 5 + [_D] * 6 + [_D, ws_bytes, 1024, 0, None, None] + [None, None, None, None, 0]


def _dis(p=_D, totals=_D + 0x1000, r0=None, r1=None):
    d = _capi.GsrDistort()
    d.out_distort, d.totals = p, totals
    d.reserved[0], d.reserved[1] = r0, r1
    return d


_BAD = [dict(p=_D + 2), dict(p=_D + 1), dict(totals=_D + 0x1002), dict(totals=None), dict(r0=_D), dict(r1=_D), dict(p=None, r0=_D), dict(p=None, totals=_D + 1)]


@pytest.mark.parametrize("bad", _BAD)
def test_forward_validates_before_launch(bad):
    lib = _capi.lib()
    assert len(_fwd_args()) == len(lib.gsr_forward_ex.argtypes)
    assert lib.gsr_forward_distort(*_fwd_args(), C.byref(_dis())) == _capi.GPSGS_E_WORKSPACE  # the valid control
    assert lib.gsr_forward_distort(*_fwd_args(), C.byref(_dis(**bad))) == _capi.GPSGS_E_INVALID


@pytest.mark.parametrize("bad", _BAD)
def test_backward_validates_before_launch(bad):
    lib = _capi.lib()
    assert len(_bwd_args()) == len(lib.gsr_backward_camera.argtypes)
    assert lib.gsr_backward_distort(*_bwd_args(), C.byref(_dis())) == _capi.GPSGS_E_WORKSPACE  # the valid control
    assert lib.gsr_backward_distort(*_bwd_args(), C.byref(_dis(**bad))) == _capi.GPSGS_E_INVALID


def test_the_depth_alpha_workspace_is_required():
    """With the map's gradient wanted the backward needs gsr_workspace_bytes_depth_alpha(..., 0) -- the plain size is too small, and so is one byte
    less; the forward needs the forward-only size; a NULL struct or a NULL map pointer asks for nothing more than the call without the option."""
    lib = _capi.lib()
    dims = (1, 8, 8, 1024, 0)
    da, plain = lib.gsr_workspace_bytes_depth_alpha(*dims, 0), lib.gsr_workspace_bytes_ex(*dims, 0)
    assert da > plain
    for nbytes in (plain, da - 1):
        assert lib.gsr_backward_distort(*_bwd_args(nbytes), C.byref(_dis())) == _capi.GPSGS_E_WORKSPACE
    for d in (None, C.byref(_dis(p=None)), C.byref(_dis(p=None, totals=None))):
        assert lib.gsr_backward_distort(*_bwd_args(plain - 1), d) == _capi.GPSGS_E_WORKSPACE
        assert lib.gsr_backward_camera(*_bwd_args(plain - 1)) == _capi.GPSGS_E_WORKSPACE
    fwd = lib.gsr_workspace_bytes_depth_alpha(*dims, 1)
    assert fwd == lib.gsr_workspace_bytes_ex(*dims, 1)
    assert lib.gsr_forward_distort(*_fwd_args(fwd - 1), C.byref(_dis())) == _capi.GPSGS_E_WORKSPACE
    assert lib.gsr_forward_ex(*_fwd_args(fwd - 1)) == _capi.GPSGS_E_WORKSPACE


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
    rs = RZ.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3), False, False)
    x = torch.zeros(4, 3)
    kw = dict(means3D=x, means2D=x, opacities=torch.ones(4, 1), colors_precomp=x, scales=x, rotations=torch.zeros(4, 4))
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
