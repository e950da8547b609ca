"""The shared view runner of the opt-in tests (tests/raster_run.py) itself: its output table against the product's decoder, on the CPU; on the GPU,
the runner with everything off against conftest.hip_render, and with several options on at once."""
import itertools

import numpy as np
import pytest

from conftest import hip_render
from raster_run import output_table, run_view, small

OPTIONS = ("depth_alpha", "antialiasing", "camera_grad", "features", "contrib", "absgrad")


def _combinations():
    """The 40 of tests/test_gpu_raster_option_matrix.py, and the distortion map with and without each of depth / alpha, antialiasing, camera_grad."""
    combos = [frozenset(o for o, on in zip(OPTIONS, bits) if on) for bits in itertools.product((False, True), repeat=len(OPTIONS))]
    combos = [c for c in combos if not ("features" in c and ("contrib" in c or "absgrad" in c))]
    assert len(combos) == 40
    return combos + [frozenset(o for o, on in zip(OPTIONS[:3], bits) if on) | {"distortion"} for bits in itertools.product((False, True), repeat=3)]


def test_the_output_table_names_what_the_product_decodes():
    from gps_gaussian_amd import rasterizer as RZ
    combos = _combinations()
    assert len(combos) == 48 and len(set(combos)) == 48
    for c in combos:
        table = output_table(7, 5, 6, extras="depth_alpha" in c, F=3 if "features" in c else 0, contrib="contrib" in c, absgrad="absgrad" in c,
                             distortion="distortion" in c)
        opts = RZ._ViewOptions("depth_alpha" in c, "antialiasing" in c, "camera_grad" in c, "features" in c, "contrib" in c, "absgrad" in c, None,
                               "distortion" in c)
        o = RZ._unpack_outputs(opts, range(len(table)))
        mine = [row[0] for row in table]
        assert mine == [k for k in o._fields if getattr(o, k) is not None], sorted(c)
        assert [getattr(o, k) for k in mine] == list(range(len(table))), sorted(c)  # equally many, in the same order


@pytest.mark.gpu
def test_everything_off_is_hip_render_bit_for_bit():
    g = small()
    dpix = np.random.default_rng(1).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    img, radii, grads, _ = hip_render(g, dpix)
    r = run_view(g, dict(img=dpix))
    assert set(r) == {"img", "radii", "grads"}
    np.testing.assert_array_equal(r["img"], img)
    np.testing.assert_array_equal(r["radii"], radii)
    assert set(r["grads"]) == set(grads)
    for k in grads:
        np.testing.assert_array_equal(r["grads"][k], grads[k], err_msg=k)
    assert (radii > 0).sum() > 100 and all(np.abs(v).max() > 0 for v in grads.values())  # (the comparison is not one of zeros)


@pytest.mark.gpu
def test_several_options_at_once(monkeypatch):
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")
    g = small()
    dpix = np.random.default_rng(1).standard_normal((3, g["H"], g["W"])).astype(np.float32)
    off = run_view(g, dict(img=dpix))
    on = run_view(g, dict(img=dpix), extras=True, cam=True, contrib=True, absgrad=True)  # (its decode assertions run inside)
    assert set(on) == {"img", "radii", "depth", "alpha", "w", "m", "n", "abs0", "abs", "grads"}
    assert set(on["grads"]) == set(off["grads"]) | {"view", "proj"}
    np.testing.assert_array_equal(on["img"], off["img"])
    np.testing.assert_array_equal(on["radii"], off["radii"])
    assert not on["abs0"].any() and (on["abs"] > 0).any() and (on["n"] > 0).any()
