"""CPU: the C-ABI of the opt-in F-channel feature maps -- GsrFeatures as the C compiler lays it out equals the ctypes mirror, the new entry points
are exported and mirrored at ABI 4, the feature workspace is the depth / alpha one plus an aligned cap x F float tail, the default sizes did not
move, and the Python keyword is opt-in and refuses bad input before anything is launched."""
import ctypes as C
import inspect
import re

import pytest

from gps_gaussian_amd import _capi

import capi_run
from capi_run import D, call, spec


def test_features_struct_layout_is_mirrored(tmp_path):
    """The C compiler's offsets of GsrFeatures equal the ctypes ones; the forward output and the backward map gradient share their slot;
    GsrViewExt is still 80 bytes."""
    got = capi_run.c_values(tmp_path, ["sizeof(GsrFeatures)", "offsetof(GsrFeatures, channels)", "offsetof(GsrFeatures, reserved0)",
                                       "offsetof(GsrFeatures, features)", "offsetof(GsrFeatures, out_features)", "offsetof(GsrFeatures, dL_dfeaturemap)",
                                       "offsetof(GsrFeatures, dL_dfeatures)", "sizeof(GsrViewExt)", "GSR_MAX_FEATURES"])
    Fs = _capi.GsrFeatures
    assert got == [C.sizeof(Fs), Fs.channels.offset, Fs.reserved0.offset, Fs.features.offset, Fs._map.offset, Fs._map.offset,
                   Fs.dL_dfeatures.offset, C.sizeof(_capi.GsrViewExt), _capi.GSR_MAX_FEATURES]
    assert got == [32, 0, 4, 8, 16, 16, 24, 80, 64]
    f = Fs()
    assert f.channels == 0 and f.features is None and f.out_features is None and f.dL_dfeatures is None  # zero-initialised = no features
    f.out_features = 0x1000
    assert f.dL_dfeaturemap == 0x1000


def test_abi_version_and_symbols():
    lib = capi_run.lib()
    assert lib.gpsgs_abi_version() == 4
    hdr = capi_run.header()
    for name in ("gsr_workspace_bytes_features", "gsr_forward_features", "gsr_backward_features"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, hdr)
    assert re.search(r"size_t gsr_workspace_bytes_features\(int P, int width, int height, int64_t instance_capacity, uint32_t bin_capacity, "
                     r"int channels, int forward_only\);", hdr)
    # the new entry points extend the existing argument lists by one GsrFeatures pointer
    assert lib.gsr_forward_features.argtypes[:-1] == lib.gsr_forward_ex.argtypes
    assert lib.gsr_backward_features.argtypes[:-1] == lib.gsr_backward_camera.argtypes
    assert lib.gsr_forward_features.argtypes[-1] == C.POINTER(_capi.GsrFeatures)


@pytest.mark.parametrize("P,W,H,cap,bcap", [(30000, 256, 256, 1 << 20, 0), (600000, 1024, 1024, 5 << 20, 1024), (1, 8, 8, 1, 0), (0, 17, 9, 0, 0)])
@pytest.mark.parametrize("F", [1, 3, 17, 64])
def test_workspace_sizes(P, W, H, cap, bcap, F):
    lib = capi_run.lib()
    da = lib.gsr_workspace_bytes_depth_alpha(P, W, H, cap, bcap, 0)
    feat = lib.gsr_workspace_bytes_features(P, W, H, cap, bcap, F, 0)
    assert feat >= da > 0
    assert feat - da == (max(cap, 1) * F * 4 + 255) // 256 * 256  # the feature tail behind everything else
    assert lib.gsr_workspace_bytes_features(P, W, H, cap, bcap, F, 1) == lib.gsr_workspace_bytes_ex(P, W, H, cap, bcap, 1)
    assert lib.gsr_workspace_bytes_features(-1, W, H, cap, bcap, F, 0) == 0
    assert lib.gsr_workspace_bytes_features(P, W, H, cap, 100, F, 0) == 0  # not a valid direct-list capacity


@pytest.mark.parametrize("F", [0, -1, 65, 1000])
def test_workspace_size_rejects_channel_counts(F):
    lib = capi_run.lib()
    assert lib.gsr_workspace_bytes_features(30000, 256, 256, 1 << 20, 0, F, 0) == 0
    assert lib.gsr_workspace_bytes_features(30000, 256, 256, 1 << 20, 0, F, 1) == 0


def test_default_workspace_sizes_are_pinned():
    """The default layout did not move (the parent commit's sizes, byte for byte)."""
    capi_run.assert_default_sizes(capi_run.lib())


# spec("gsr_forward_features") / spec("gsr_backward_features"): P = 1, an 8 x 8 image, every pointer set (never dereferenced: each call returns
# before anything is launched) and a workspace of 0 bytes: a VALID feature set of three channels gets as far as the workspace check
# (GPSGS_E_WORKSPACE), so GPSGS_E_INVALID can only come from the feature validation
def _features(lib, entry, ws=0, **opt):
    """`map`: the entry point's own name of the shared slot, out_features (forward) / dL_dfeaturemap (backward)."""
    if "map" in opt:
        opt["out_features" if entry == "gsr_forward_features" else "dL_dfeaturemap"] = opt.pop("map")
    return call(lib, entry, spec(entry, ws=ws, opt=opt))


@pytest.mark.parametrize("bad", [dict(channels=65), dict(channels=-1), dict(features=None), dict(features=D + 2), dict(map=D + 1)])
def test_forward_validates_before_launch(bad):
    lib = capi_run.lib()
    assert _features(lib, "gsr_forward_features") == _capi.GPSGS_E_WORKSPACE  # the valid control
    assert _features(lib, "gsr_forward_features", **bad) == _capi.GPSGS_E_INVALID


@pytest.mark.parametrize("bad", [dict(channels=65), dict(channels=-1), dict(features=None), dict(features=D + 2), dict(map=D + 1),
                                 dict(dL_dfeatures=D + 3)])
def test_backward_validates_before_launch(bad):
    lib = capi_run.lib()
    assert _features(lib, "gsr_backward_features") == _capi.GPSGS_E_WORKSPACE
    assert _features(lib, "gsr_backward_features", **bad) == _capi.GPSGS_E_INVALID


def test_backward_needs_the_feature_tail():
    """With both feature gradients wanted, a workspace of the depth / alpha size (no feature tail) is too small; one byte short of the feature size
    is too small too."""
    lib = capi_run.lib()
    da = lib.gsr_workspace_bytes_depth_alpha(1, 8, 8, 1024, 0, 0)
    full = lib.gsr_workspace_bytes_features(1, 8, 8, 1024, 0, 3, 0)
    assert full > da
    for nbytes in (da, full - 1):
        assert _features(lib, "gsr_backward_features", nbytes) == _capi.GPSGS_E_WORKSPACE


def test_python_api_is_opt_in():
    """The keywords default to None; a wrong shape, F = 65 or a CPU tensor is refused before anything is launched."""
    import torch
    from gps_gaussian_amd import rasterizer as RZ
    from gps_gaussian_amd import render_api
    assert inspect.signature(RZ.rasterize_gaussians).parameters["features"].default is None
    assert inspect.signature(RZ.GaussianRasterizer.forward).parameters["features"].default is None
    assert inspect.signature(render_api.render_ex).parameters["features"].default is None
    assert list(inspect.signature(render_api.render_ex).parameters)[:8] == ["data", "idx", "pts_xyz", "pts_rgb", "rotations", "scales", "opacity", "bg_color"]
    rs, kw = capi_run.cpu_view()
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        RZ.GaussianRasterizer(rs)(**kw, features=torch.zeros(4, 5))
    dev = torch.device("cpu")
    with pytest.raises(RuntimeError, match=r"\(num_points, F\)"):
        RZ._features(torch.zeros(4, 65), 4, dev)
    with pytest.raises(RuntimeError, match=r"\(num_points, F\)"):
        RZ._features(torch.zeros(3, 5), 4, dev)
    with pytest.raises(RuntimeError, match=r"\(num_points, F\)"):
        RZ._features(torch.zeros(4), 4, dev)
    with pytest.raises(RuntimeError, match=r"\(num_points, F\)"):
        RZ._features(torch.zeros(4, 0), 4, dev)
    with pytest.raises(TypeError):
        RZ._features([[0.0]], 1, dev)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RZ._features(torch.zeros(4, 5), 4, torch.device("cuda", 0))
