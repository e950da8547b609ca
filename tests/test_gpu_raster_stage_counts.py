"""GPU (-m gpu): the per-stage launch bookkeeping of the rasteriser's C layer (GSR_FLAG_TIMING, _capi.timing_read): one forward + backward of a 16 x 16
view brackets each stage once -- the scan only with scanned lists -- the gather of the contribution statistics counts as a second composite_fwd, the
gathers of absgrad and of the feature gradients as a second preprocess_bwd, and GSR_FLAG_TIMING_STAGE brackets the one stage it names.  The VALU
family (the opt-ins have no other kernels); both list forms."""
import numpy as np
import pytest

from conftest import gaussians, simple_scene
from raster_run import output_table

pytestmark = pytest.mark.gpu

F = 3
PLAIN = dict(preprocess=1, scatter=1, sort=1, composite_fwd=1, composite_bwd=1, preprocess_bwd=1)  # (+ scan: 1 with scanned lists, 0 with direct ones)


def _counts(options, stage=None):
    """Stage -> bracketed launches of one forward + backward of the view with `options` (keywords of rasterize_gaussians)."""
    import torch
    from gps_gaussian_amd import _capi
    from gps_gaussian_amd import rasterizer as RZ
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    n = 40
    scene = simple_scene(16, 16, 16.0)
    g = gaussians(np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), rng.uniform(1.5, 3.0, n)], 1), rng.uniform(0, 1, (n, 3)), rng.uniform(0.3, 0.9, n), 0.1)
    t = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in g.items()}
    m2 = torch.zeros_like(t["means3D"], requires_grad=True)
    if options.get("features"):
        options = dict(options, features=torch.from_numpy(rng.uniform(-1, 1, (n, F)).astype(np.float32)).to(dev).requires_grad_(True))
    rs = RZ.GaussianRasterizationSettings(16, 16, scene["tanfovx"], scene["tanfovy"], torch.from_numpy(scene["bg"]).to(dev), 1.0, torch.from_numpy(scene["view"]).to(dev),
                                          torch.from_numpy(scene["proj"]).to(dev), 3, torch.from_numpy(scene["campos"]).to(dev), False, False)
    RZ.set_stage_timing(True, stage)
    try:
        _capi.timing_read()  # (drop what earlier calls recorded)
        out = RZ.rasterize_gaussians(t["means3D"], m2, None, t["colors"], t["opacities"], t["scales"], t["rotations"], None, rs, **options)
        fmap = [row[0] for row in output_table(n, 16, 16, F=F)].index("feat")
        loss = out[0].sum() + (out[fmap].sum() if options.get("features") is not None else 0.0)
        loss.backward()
        torch.cuda.synchronize()
        assert int((out[1] > 0).sum()) > 20  # the view is not empty
        return {k: v[1] for k, v in _capi.timing_read().items()}
    finally:
        RZ.set_stage_timing(False)


@pytest.mark.parametrize("lists", ["direct", "scanned"])
def test_stage_launch_counts(lists, monkeypatch):
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    monkeypatch.setenv("GPSGS_LISTS", lists)
    plain = dict(PLAIN, scan=1 if lists == "scanned" else 0)
    assert _counts({}) == plain
    assert _counts(dict(return_contrib=True)) == dict(plain, composite_fwd=2)
    assert _counts(dict(return_absgrad=True)) == dict(plain, preprocess_bwd=2)
    assert _counts(dict(features=True)) == dict(plain, preprocess_bwd=2)
    assert _counts(dict(return_depth_alpha=True)) == plain
    assert _counts({}, stage="sort") == dict({k: 0 for k in plain}, sort=1)
    assert _counts(dict(return_contrib=True), stage="composite_fwd") == dict({k: 0 for k in plain}, composite_fwd=2)
