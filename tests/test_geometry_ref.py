"""CPU: the references of tests/geometry_ref.py against the fixtures the upstream code produced, the float32 restatement against the float64 bounds
on every input the GPU tests use (so the bounds are known to be reachable by correct float32 arithmetic), and mutants: one error each, applied to a
reference, that the GPU tests' own comparison helpers must report."""
import os

import numpy as np
import pytest

import geometry_ref as G
from conftest import GOLDEN

UNPROJ_ARGS = ("flow", "mask", "ref_intr", "intr", "extr", "Tf_x")


def _f32(inp, **kw):
    return G.unproject_f32(*(inp[k] for k in UNPROJ_ARGS), **kw)


def _case(B, S, seed):
    inp = G.unproject_inputs(B, S, seed)
    gd, gx = G.unproject_grads(B, S, seed)
    return inp, gd, gx


# ---- the references reproduce the fixtures ------------------------------------------------------------------------------------------------------------
def test_float32_restatement_gives_the_unproject_fixture_its_depth_and_valid_bits():
    g = np.load(os.path.join(GOLDEN, "unproject_golden.npz"))
    r = _f32(g)
    assert G.bits_fault("depth", r["depth"], g["depth"]) is None
    assert G.bits_fault("valid", r["valid"], g["valid"]) is None


def test_float64_formulas_match_the_unproject_fixture_within_the_bounds():
    """The fixture's xyz and g_flow are torch float32 values: they, and the float32 restatement, sit within the bounds of the float64 formulas
    (measured here: below 3 units of 2^-24 x magnitude for xyz, below 5 for d_flow)."""
    g = np.load(os.path.join(GOLDEN, "unproject_golden.npz"))
    r64 = G.unproject_f64(g["depth"], g["mask"], g["intr"], g["extr"], g["Tf_x"], g_depth=g["g_depth"], g_xyz=g["g_xyz"])
    np.testing.assert_allclose(G.depth_f64(g["flow"], g["mask"], g["ref_intr"], g["intr"], g["Tf_x"]), g["depth"], rtol=3 * G.U, atol=0)
    assert G.bits_fault("valid", r64["valid"], g["valid"]) is None
    assert G.xyz_fault(g["xyz"], r64) is None
    assert G.dflow_fault(g["g_flow"], r64, g["mask"]) is None
    r32 = _f32(g, g_depth=g["g_depth"], g_xyz=g["g_xyz"])
    print("fixture xyz %.2f d_flow %.2f | float32 restatement xyz %.2f d_flow %.2f (units of 2^-24 x magnitude)" % (
        G.error_units(g["xyz"], r64["xyz"], r64["xyz_mag"]), G.error_units(g["g_flow"], r64["d_flow"], r64["d_flow_mag"]),
        G.error_units(r32["xyz"], r64["xyz"], r64["xyz_mag"]), G.error_units(r32["d_flow"], r64["d_flow"], r64["d_flow_mag"])))
    assert G.xyz_fault(r32["xyz"], r64) is None and G.dflow_fault(r32["d_flow"], r64, g["mask"]) is None


def test_float64_formulas_match_the_depth2pc_fixture_within_the_xyz_bound():
    g = np.load(os.path.join(GOLDEN, "depth2pc_golden.npz"))
    r64 = G.unproject_f64(g["inv_depth"][None, None], np.ones((1, 1) + g["inv_depth"].shape, np.float32), g["intr"][None], g["extr"][None], np.ones(1))
    assert G.xyz_fault(g["xyz"][None], r64) is None
    assert not r64["valid"].reshape(g["inv_depth"].shape)[:3].any() and r64["valid"].reshape(g["inv_depth"].shape)[3:].all()


def _golden_pack():
    g = np.load(os.path.join(GOLDEN, "pts2render_golden.npz"))
    maps = [{k: g["%s_%s" % (v, k)] for k, _ in G.PACK_KEYS} for v in ("lmain", "rmain")]
    valid = np.stack([g["lmain_pts_valid"], g["rmain_pts_valid"]], 1)
    return g, maps, valid


def test_pack_ref_gives_the_pts2render_fixture_its_bits():
    g, maps, valid = _golden_pack()
    for ref in (G.pack_ref(maps, valid), G.pack_by_scan(maps, valid)):
        offs = ref["offsets"]
        assert len(offs) == 3 and offs[0] == 0
        for i in range(2):
            for k in G.OUT_KEYS:
                assert G.bits_fault("out%d_%s" % (i, k), ref[k][offs[i]:offs[i + 1]], g["out%d_%s" % (i, k)]) is None


# ---- the bounds are reachable: float32 restatement vs float64 on the GPU tests' inputs ------------------------------------------------------------------
@pytest.mark.parametrize("B,S,seed", G.UNPROJECT_CASES + G.HOST_CASES + [(G.CHAIN_CASE["B"], G.CHAIN_CASE["S"], G.CHAIN_CASE["seed"] + v)
                                                                         for v in range(G.CHAIN_CASE["V"])])
def test_float32_restatement_stays_within_the_float64_bounds_on_every_gpu_input(B, S, seed):
    inp, gd, gx = _case(B, S, seed)
    assert G.zero_disparity_pixels(inp).sum() >= (B if S > 1 else (B + 2) // 3)      # the generator's special pixels are there
    assert (inp["mask"][:, 0] == 0).any() or S == 1
    worst = [0.0, 0.0]
    for g_depth, g_xyz in ((gd, gx), (None, gx), (gd, None)):
        r = _f32(inp, g_depth=g_depth, g_xyz=g_xyz)
        assert G.unproject_fault(r, inp, g_depth, g_xyz, want_bits=("xyz", "d_flow")) is None
        ux, ud = G.unproject_units(r, inp, g_depth, g_xyz)
        worst = [max(worst[0], ux), max(worst[1], ud)]
    print("B %d S %d: float32 restatement off by xyz %.2f, d_flow %.2f x 2^-24 x magnitude" % (B, S, worst[0], worst[1]))
    zd = G.zero_disparity_pixels(inp)
    r = _f32(inp, g_xyz=gx)
    assert not r["valid"][zd].any() and (r["d_flow"].reshape(B, -1)[zd] != 0).all()   # invalid, and still a gradient


def test_inputs_give_every_sample_its_own_cameras():
    inp = G.unproject_inputs(33, 5, 233)
    K, Kr, E = inp["intr"], inp["ref_intr"], inp["extr"]
    assert (K[:, 0, 0] != K[:, 1, 1]).all() and (K[:, 0, 2] != K[:, 1, 2]).all() and (Kr[:, 0, 2] != K[:, 0, 2]).all()
    assert (np.abs(E[:, :, :3] - np.transpose(E[:, :, :3], (0, 2, 1))).max(axis=(1, 2)) > 0.1).all() and (np.abs(E[:, :, 3]) > 0.1).all()
    for k in G.CHUNK_FIELDS:
        flat = inp[k].reshape(33, -1)
        assert len({flat[b].tobytes() for b in range(33)}) == 33, k
    assert (inp["mask"][:, 1] != inp["mask"][:, 0]).all() and (inp["mask"][:, 2] != inp["mask"][:, 0]).any()


# ---- mutants: unprojection ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", G.CHUNK_FIELDS)
@pytest.mark.parametrize("B,S,seed", [c for c in G.HOST_CASES if c[0] > G.MAXB])
def test_a_chunk_that_reads_one_input_from_chunk_0_is_rejected(B, S, seed, field):
    inp, gd, gx = _case(B, S, seed)
    assert G.unproject_fault(_f32(inp, g_depth=gd, g_xyz=gx), inp, gd, gx) is None
    bad = _f32(G.chunk_mutant(inp, field), g_depth=gd, g_xyz=gx)
    assert G.unproject_fault(bad, inp, gd, gx) is not None
    for b0 in range(G.MAXB, B, G.MAXB):       # ... and every later chunk on its own gives the mismatch away
        sl = slice(b0, min(b0 + G.MAXB, B))
        sub = lambda d: {k: v[sl] for k, v in d.items()}
        assert G.unproject_fault(sub(bad), sub(inp), gd[sl], gx[sl]) is not None, b0


@pytest.mark.parametrize("field", G.CHUNK_FIELDS)
def test_the_fixture_tiled_with_arange_37_mod_2_does_not_see_the_chunk_mutants(field):
    """Why HOST_CASES exists: test_gpu_unproject.py's batch of 37 repeats the fixture's two samples, 16 is even, so sample 16 + k IS sample k and an
    input offset that stays at chunk 0 changes no bit."""
    g = np.load(os.path.join(GOLDEN, "unproject_golden.npz"))
    idx = np.arange(37) % g["flow"].shape[0]
    inp = {k: g[k][idx] for k in UNPROJ_ARGS}
    gd, gx = g["g_depth"][idx], g["g_xyz"][idx]
    assert G.unproject_fault(_f32(G.chunk_mutant(inp, field), g_depth=gd, g_xyz=gx), inp, gd, gx) is None


@pytest.mark.parametrize("B,S,seed", [c for c in G.UNPROJECT_CASES if c[1] > 1])
def test_swapped_uv_r_for_rt_wrong_mask_channel_and_stride_1_gradient_are_rejected(B, S, seed):
    inp, gd, gx = _case(B, S, seed)
    assert G.unproject_fault(_f32(inp, g_depth=gd, g_xyz=gx, _swap_uv=True), inp, gd, gx) is not None
    assert G.unproject_fault(_f32(G.r_for_rt_mutant(inp), g_depth=gd, g_xyz=gx), inp, gd, gx) is not None
    assert G.unproject_fault(_f32(G.mask_channel_mutant(inp), g_depth=gd, g_xyz=gx), inp, gd, gx) is not None
    bad = _f32(inp, g_depth=gd, g_xyz=G.stride1_gradient_mutant(gx))
    assert "d_flow" in G.unproject_fault(bad, inp, gd, gx)


def test_one_pixel_maps_still_reject_the_mutants_that_can_show_there():
    """S = 1: u = v = 0, so a u/v swap is invisible; R for R^T and the mask channel are not."""
    for B, S, seed in [c for c in G.UNPROJECT_CASES if c[1] == 1]:
        inp, gd, gx = _case(B, S, seed)
        assert G.unproject_fault(_f32(G.r_for_rt_mutant(inp), g_depth=gd, g_xyz=gx), inp, gd, gx) is not None
        assert G.unproject_fault(_f32(G.mask_channel_mutant(inp), g_depth=gd, g_xyz=gx), inp, gd, gx) is not None


def test_the_bound_helpers_reject_an_error_just_over_the_bound_and_accept_one_under():
    inp, gd, gx = _case(3, 17, 999)
    r = _f32(inp, g_depth=gd, g_xyz=gx)
    r64 = G.unproject_f64(r["depth"], inp["mask"], inp["intr"], inp["extr"], inp["Tf_x"], g_depth=gd, g_xyz=gx)
    for key, mag, k, fault in (("xyz", "xyz_mag", G.XYZ_ROUNDINGS, lambda a: G.xyz_fault(a, r64)),
                               ("d_flow", "d_flow_mag", G.DFLOW_ROUNDINGS, lambda a: G.dflow_fault(a, r64, inp["mask"]))):
        i = np.unravel_index(np.argmax(r64[mag]), r64[mag].shape)
        for factor, rejected in ((0.9, False), (1.1, True)):
            a = r64[key].copy()
            a[i] += factor * k * G.U * r64[mag][i]
            assert (fault(a) is not None) == rejected, (key, factor)
    leak = r["d_flow"].copy()
    leak[inp["mask"][:, :1] == 0] = 1e-30
    assert G.dflow_fault(leak, r64, inp["mask"]) is not None        # a masked pixel has magnitude 0: nothing but 0 passes


# ---- mutants: pack ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.pack_cases(), ids=lambda c: "B%d-V%d-%dx%d-%s" % c[:5])
def test_the_two_pack_formulations_agree_on_every_gpu_case(case):
    maps, valid = G.pack_inputs(*case)
    B, V, H, W, pattern, _ = case
    ref = G.pack_ref(maps, valid)
    assert G.pack_fault(G.pack_by_scan(maps, valid), ref) is None
    assert ref["offsets"][-1] == valid.sum() and (ref["row_of_pixel"] >= 0).sum() == valid.sum()
    if pattern == "all":
        assert valid.all()
    if pattern in ("none_in_view0", "empty_sample", "hole_block", "alternate_64", "random") and H * W > 1:
        assert valid.any() and not valid.all()
    if V > 1 and valid[:, 0].any() and valid[:, 1].any():
        assert G.pack_fault(G.pack_ref(maps, valid, _view_order=range(V)[::-1]), ref) is not None      # views in the wrong order
    if valid.reshape(-1, H * W)[:, :-1].any() and H * W > 1 and pattern not in ("first_only", "last_only"):
        assert G.pack_fault(G.pack_by_scan(maps, valid, inclusive_rank=True), ref) is not None          # rank off by one lane


def test_pack_values_are_distinct_within_a_kind():
    maps, _ = G.pack_inputs(3, 4, 48, 64, "random", 1)
    for k, _ in G.PACK_KEYS:
        allv = np.concatenate([m[k].reshape(-1) for m in maps])
        assert len(np.unique(allv.view(np.uint32))) == allv.size and np.isfinite(allv).all()


def test_pack_mutants_are_rejected_on_the_multi_chunk_case():
    maps, valid = G.pack_inputs(**G.BIG_PACK)
    B, V, S2 = valid.shape
    nblk = (S2 + G.PB - 1) // G.PB
    assert B * V * nblk > G.SCAN and 5 * V * nblk > G.SCAN and 4 * V * nblk < G.SCAN       # sample 5's offset is written in the second scan chunk
    assert not valid[3].any() and all(valid[b].any() for b in (0, 1, 2, 4, 5))
    ref = G.pack_ref(maps, valid)
    assert G.pack_fault(G.pack_by_scan(maps, valid), ref) is None
    assert "offsets" in G.pack_fault(G.pack_by_scan(maps, valid, drop_carry=True), ref)
    dropped = G.pack_by_scan(maps, valid, drop_carry=True)
    dropped["offsets"] = ref["offsets"]                                                     # even with the offsets right the rows give it away
    assert "row_of_pixel" in G.pack_fault(dropped, ref)
    assert G.pack_fault(G.pack_by_scan(maps, valid, inclusive_rank=True), ref) is not None
    assert "offsets" in G.pack_fault(G.pack_by_scan(maps, valid, skip_empty_offset=True), ref)
    assert G.pack_fault(G.pack_ref(maps, valid, _view_order=(1, 0)), ref) is not None


def test_an_offset_not_advanced_past_an_empty_sample_is_rejected_on_the_small_case_too():
    case = next(c for c in G.pack_cases() if c[4] == "empty_sample" and c[0] == 3)
    maps, valid = G.pack_inputs(*case)
    assert not valid[1].any() and valid[0].any() and valid[2].any()
    assert "offsets" in G.pack_fault(G.pack_by_scan(maps, valid, skip_empty_offset=True), G.pack_ref(maps, valid))


def test_an_img_gradient_that_is_not_halved_is_rejected():
    B, V, H, W, pattern, seed = 3, 2, 25, 41, "random", 448
    maps, valid = G.pack_inputs(B, V, H, W, pattern, seed)
    ref = G.pack_ref(maps, valid)
    g = G.pack_row_grads(int(ref["offsets"][-1]), seed)
    want = G.pack_bwd_ref(ref["row_of_pixel"], g, (H, W))
    assert G.pack_bwd_fault(want, want) is None
    assert "d_img" in G.pack_bwd_fault(G.pack_bwd_ref(ref["row_of_pixel"], g, (H, W), halve_img=False), want)
    for v in range(V):                        # zero exactly where invalid, the row's value elsewhere
        ok = valid[:, v]
        assert (want[v]["xyz"][~ok] == 0).all() and (want[v]["xyz"][ok] == g["xyz"][ref["row_of_pixel"][:, v][ok]]).all()
        assert (want[v]["opacity_maps"].reshape(B, -1)[~ok] == 0).all()
        assert (want[v]["img"].reshape(B, 3, -1).transpose(0, 2, 1)[ok] == g["rgb"][ref["row_of_pixel"][:, v][ok]] * np.float32(0.5)).all()
    none = G.pack_bwd_ref(ref["row_of_pixel"], {"xyz": g["xyz"]}, (H, W))
    assert all((none[v][k] == 0).all() for v in range(V) for k in ("img", "rot_maps", "scale_maps", "opacity_maps"))
