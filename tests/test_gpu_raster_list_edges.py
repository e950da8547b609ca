"""The per-bin sorts and the compositing walks at their exact lengths: one deterministic 16 x 16 scene whose four bin lists all hold exactly N entries.

Every length-dependent decision of the rasteriser is an integer comparison; each is listed here next to the cases that land on either side of it.

  decision (where)                                                              | one side                          | other side
  ------------------------------------------------------------------------------+-----------------------------------+----------------------------------
  n == 1 shortcut (gsr_sort_wave.h sort_wave_list)                              | N = 1                             | N = 2, 3
  keys per lane 1 / 2 / 4 / 8 / 16 at n <= 64 / 128 / 256 / 512 (sort_wave_list)| N = 63, 64; 127, 128; 255, 256;   | N = 65; 129; 257; 513
                                                                                |   511, 512                        |
  32-bit composite keys iff dmax - dmin < (0xffffffff >> L), L = bits of n - 1  | layout `below`: spread T - 1      | layout `at`: spread T, the first
    (sort_wave_regs32), else the 64-bit network                                 |   (every N from 63 to 1024)       |   that must fall back (same N)
  k_sort_wave takes n <= 1024 (gsr_binning.hip)                                 | N = 1023, 1024                    | N = 1025 (scanned)
  k_sort_multi<1/2/4> takes LO < n <= HI for 1024 / 2048 / 4096 / 8192          | N = 1025, 2047, 2048; 4095, 4096; | N = 2049; 4097; 8193
                                                                                |   8191, 8192                      |
  k_sort_large takes n > 8192: LDS workgroup up to 16384, global memory beyond  | N = 8193, 16383, 16384            | N = 16385
  the scan reports tot_max > 1024 as an overflow when the large sort launch was | scanned N = 1024 on a fresh       | scanned N = 1025 on a fresh
    skipped (gsr_binning.hip, GSR_FLAG_NO_LARGE_SORT)                           |   device: rendered at once        |   device: reported, repaired
  a direct bin holds _DIRECT_CAP = 1024 entries; overflow is                    | direct / default policy N = 1024: | direct / default policy N = 1025:
    max_tile_count > bin_capacity (rasterizer.py)                               |   bin_cap stays 1024              |   repaired with scanned lists
  compositing walks a list in rounds of 64 entries, in groups of 8; the         | full walks N = 7, 8; 63, 64; 127, | N = 9; 65; 129; 1025; pixels that
    backward finishes 8 splats at a time, from each pixel's last contributor    |   128; 1023, 1024                 |   stop at 63 / 64 / 65 and at
                                                                                |                                   |   127 / 128 / 129 inside one bin

The scene: conftest.simple_scene(16, 16, fx=16) -- 2 x 2 real bins of 8 x 8 pixels in a bin grid padded to 4 columns -- and N isotropic Gaussians on the
optical axis.  Gaussian i sits at the depth whose float32 bit pattern is bits(0.25f) + off_i, so the sort keys' depth words are chosen exactly, and its
scale is 1.5 x its depth: every footprint is a 24-pixel sigma whatever the depth, every Gaussian reaches every pixel of every bin, and every list is the
whole cloud.  The expected list is therefore known in closed form -- ids[lexsort((ids, bits))], upstream's stable (depth, id) order -- and is compared
element for element: a dropped, duplicated or misplaced id cannot hide behind "ascending".

The unmarked tests at the end hold the scene to its own validity conditions on the CPU oracle, and show that the list check rejects a swapped tie, a
duplicated id and a missing id.
"""
import functools

import numpy as np
import pytest

from conftest import assert_grad_parity, fragile_bounds, gaussians, hip_render, oracle_render, simple_scene
from raster_run import GEOM, check_absgrad_structure, check_against_plain, check_contrib_structure, close, close_each, pad, run_view

RGB_TOL = 1e-4
SIZE = 16
BASE_BITS = int(np.float32(0.25).view(np.uint32))
OPACITY_FULL = 0.0045  # alpha >= 0.0040 > 1/255 at the image corners; T after 1,025 splats ~ 0.0099 > 1e-4: every pixel walks every list to its end
# opacity 1 - 10^(-4/k): T reaches 1e-4 after ~k splats at the image centre and a few later towards the corners
STOPS = {"stop64": (1.0 - 10.0 ** (-4.0 / 60.0), (63, 64, 65)), "stop128": (1.0 - 10.0 ** (-4.0 / 124.0), (127, 128, 129))}
N_STOP = 200

N_WAVE = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024]
N_LARGE = [1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385]
N_WALK = [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]
OPT_IN_SCENES = [("full", 63), ("full", 64), ("full", 65), ("full", 1024), ("stop64", N_STOP), ("stop128", N_STOP)]
LAYOUTS = ("below", "at", "narrow", "ties3", "one_depth")


# ---- the scene ------------------------------------------------------------------------------------------------------------------------------------

def _threshold(n):
    """T of sort_wave_regs32: the 32-bit composite key is used iff dmax - dmin < T = 0xffffffff >> L, L = the bits of n - 1."""
    return 0xffffffff >> (n - 1).bit_length()


def _layouts_for(n):
    """`below` / `at` need a spread of T: with base 0.25 and depths up to 64 (offsets up to 2^26) that exists from L = 6 on; lists beyond 1,024 keys are
    not sorted on composite keys at all."""
    return LAYOUTS if 33 <= n <= 1024 else LAYOUTS[2:]


def _offsets(layout, n, rng):
    """off_i (int64 [n]) of a depth layout, in random order relative to the ids."""
    if layout in ("below", "at"):
        top = _threshold(n) - (1 if layout == "below" else 0)   # the largest offset; the smallest is 0
        off = np.concatenate([[0, top], 1 + rng.choice(top - 1, size=n - 2, replace=False)])   # distinct, strictly inside (0, top)
    elif layout == "narrow":
        off = rng.choice(1 << (20 if n <= 1024 else 22), size=n, replace=False)
    elif layout == "ties3":
        levels = max(1, (n + 2) // 3)
        off = rng.integers(0, levels, size=n) * ((1 << 20) // levels)
    elif layout == "one_depth":
        off = np.full(n, 4097)
    else:
        raise KeyError(layout)
    return rng.permutation(np.asarray(off, np.int64))


def _scene(n, layout, opacity=OPACITY_FULL):
    """-> (scene dict for hip_render / oracle_render, depth bits uint32 [n])."""
    rng = np.random.default_rng(100 * n + LAYOUTS.index(layout))
    bits = (BASE_BITS + _offsets(layout, n, rng)).astype(np.uint32)
    z = bits.view(np.float32)
    xyz = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)
    scale = (np.float32(1.5) * z)[:, None]
    g = dict(simple_scene(SIZE, SIZE, fx=16.0), **gaussians(xyz, rng.uniform(0.0, 1.0, (n, 3)), opacity, scale))
    return g, bits


# ---- the list check -------------------------------------------------------------------------------------------------------------------------------

def _expected_list(bits):
    """A bin that lists every Gaussian: ids in upstream's stable order, depth bits first, then id."""
    ids = np.arange(len(bits))
    return ids[np.lexsort((ids, np.asarray(bits, np.int64)))]


def _list_fault(got, bits):
    """None when `got` is exactly the expected list, else what is wrong with it."""
    want = _expected_list(bits)
    got = np.asarray(got, np.int64).reshape(-1)
    if got.shape != want.shape:
        return "%d entries instead of %d" % (got.size, want.size)
    bad = np.nonzero(got != want)[0]
    if bad.size:
        return "%d of %d entries differ, the first at position %d: id %d instead of %d" % (bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])
    return None


def _assert_lists(info, bits, what):
    """The exported state of one forward of _scene(): the chosen depth bits, exactly four lists -- the real bins of the padded 4 x 2 grid -- of exactly N
    entries each (the case's validity condition), and each of them the expected permutation.  -> the exported state."""
    from gps_gaussian_amd import rasterizer as RZ
    n = len(bits)
    st = RZ.export_state(info["ws"], n, SIZE, SIZE, info["cap"], info["bin_cap"])
    assert st["overflow"] == 0, what
    np.testing.assert_array_equal(st["depth"].cpu().numpy().view(np.uint32), bits, err_msg=what)
    assert (st["bx"], st["by"]) == (4, 2)
    rg = st["ranges"].cpu().numpy().astype(np.int64)
    lengths = rg[:, 1] - rg[:, 0]
    assert np.nonzero(lengths)[0].tolist() == [0, 1, 4, 5], (what, lengths.tolist())   # the padded bins stay empty
    assert lengths[[0, 1, 4, 5]].tolist() == [n] * 4, (what, lengths.tolist())
    assert st["num_rendered"] == 4 * n, what
    plist = st["point_list"].cpu().numpy()
    for b in (0, 1, 4, 5):
        fault = _list_fault(plist[rg[b, 0]:rg[b, 1]], bits)
        assert fault is None, "%s, bin %d: %s" % (what, b, fault)
    return st


def _forget_long_lists():
    """The state conftest's per-test fixture starts a GPU test from ("no long list seen"), again before a further render of the same test."""
    from gps_gaussian_amd import rasterizer as RZ
    for st in list(RZ._state.values()):
        for k in ("big_bins", "short_streak", "longest"):
            st.pop(k, None)


def _sorted_lists_case(n, direct):
    """Every layout of this N: the forward with debug=True first (it validates every list before compositing and raises instead of reading a wild id),
    then without.  Both from fresh device state, so that the skipped large-sort launch and its repair are met on both host paths."""
    from gps_gaussian_amd import rasterizer as RZ
    dpix = np.ones((3, SIZE, SIZE), np.float32)
    for layout in _layouts_for(n):
        g, bits = _scene(n, layout)
        imgs = []
        for debug in (True, False):
            what = "N=%d %s debug=%s" % (n, layout, debug)
            _forget_long_lists()
            img, radii, _, info = hip_render(g, dpix, debug=debug)
            assert (radii > 0).all(), what
            assert info["bin_cap"] == (RZ._DIRECT_CAP if direct else 0), what   # direct: no repair happened, N <= 1,024 entries fit
            _assert_lists(info, bits, what)
            imgs.append(img)
        np.testing.assert_array_equal(imgs[0], imgs[1], err_msg="N=%d %s: debug and plain forward" % (n, layout))


# ---- 1. sorted lists are exactly the expected permutation ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("form,fam", [("direct", "tiles"), ("direct", "valu"), ("scanned", "tiles")],
                         ids=["direct-tiles_sorts_in_the_forward", "direct-valu_sort_direct_launch", "scanned_sort_wave_launch"])
@pytest.mark.parametrize("n", N_WAVE)
def test_one_wave_sorts_lists_of_exactly_n_keys(n, form, fam, monkeypatch):
    """Lists of up to 1,024 keys, one wave each: sorted by the forward compositing wave itself (direct lists, tile family, no debug flag), by
    k_sort_wave over direct bins (debug, and the VALU family) and by k_sort_wave over scanned lists.  Scanned N = 1024 on fresh device state is the
    non-overflow side of the scan's `longest > 1024 while the large sort launch was skipped`."""
    monkeypatch.setenv("GPSGS_LISTS", form)
    monkeypatch.setenv("GPSGS_COMPOSITE", fam)
    _sorted_lists_case(n, direct=form == "direct")


@pytest.mark.gpu
@pytest.mark.parametrize("n", N_LARGE)
def test_multi_wave_and_large_sorts_lists_of_exactly_n_keys(n, monkeypatch):
    """k_sort_multi<1 / 2 / 4> (1,025 .. 8,192 keys) and k_sort_large (LDS up to 16,384, global memory beyond) on either side of every class limit.
    Each render starts from fresh device state: the large sort launch is skipped, the scan reports the long list like an overflow and the view is
    repaired (N = 1025 is the first length that is)."""
    monkeypatch.setenv("GPSGS_LISTS", "scanned")
    _sorted_lists_case(n, direct=False)


# ---- 2. capacity and capacity + 1 with the default policy -----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_direct_bin_holds_exactly_its_capacity_and_one_more_entry_is_repaired(monkeypatch):
    """No GPSGS_LISTS: a device that has rendered nothing gives the view direct lists.  Four bins of exactly 1,024 entries are not an overflow
    (max_tile_count > bin_capacity); four of 1,025 are, and come back exact from the repair run with scanned lists.  Each half starts from a device
    state of its own, since the first one leaves `big_bins` set."""
    from gps_gaussian_amd import rasterizer as RZ
    import torch
    monkeypatch.delenv("GPSGS_LISTS", raising=False)
    dev = torch.device("cuda:0")
    RZ._state.clear()
    try:
        ref = _reference("full", 1024)
        img, _, _, info = hip_render(ref["g"], ref["dpix"])
        assert info["bin_cap"] == RZ._DIRECT_CAP == 1024          # 1,024 entries fit: rendered with direct lists, nothing repaired
        _assert_lists(info, ref["bits"], "default policy, N=1024")
        assert np.abs(img - ref["oimg"]).max(0)[ref["solid"]].max() <= RGB_TOL
        assert RZ._dev_state(dev).get("big_bins") is True         # (longer than 768: the next view gets scanned lists)
        RZ._state.clear()
        ref = _reference("full", 1025)
        img, _, _, info = hip_render(ref["g"], ref["dpix"])
        assert info["bin_cap"] == 0                               # one entry too many: reported, repaired with scanned lists
        _assert_lists(info, ref["bits"], "default policy, N=1025")
        assert np.abs(img - ref["oimg"]).max(0)[ref["solid"]].max() <= RGB_TOL
        assert RZ._dev_state(dev).get("big_bins") is True
    finally:
        RZ._state.clear()


# ---- 3. image, per-pixel state and gradients across round boundaries ------------------------------------------------------------------------------

def _dpix(n):
    """dL/dpix of the walk cases: random, but positive and tilted -- uniform(0.5, 1.5) times a ramp across the image whose direction differs per channel.
    Every Gaussian of this scene is centred on the image and covers all of it, so every gradient is a sum over the same 256 pixels.  With a
    sign-symmetric dL/dpix (standard normal) those sums cancel and the REFERENCE is no reference: the fp32 oracle's own gradients are then 1e-3 to
    3e-3 (normalised as assert_grad_parity does) away from the fp64 oracle's under the same decisions at N = 128 and from N = 1023 on -- up to three
    times the tolerance -- and the kernels sit as far from both (measured: 1.8e-3 at N = 64, 1.1e-2 at N = 1023).  Positive but without the tilt, the
    on-axis splats' screen-space gradients cancel by symmetry instead (fp32 against fp64 oracle: 9.4e-3 at N = 1024).  With this one the fp32 oracle
    stays within 3e-4 of the fp64 one in every case (6e-5 up to N = 129; what remains beyond is the rounding of a 1,024-deep blend in fp32), and
    test_walk_scenes_stop_where_they_claim_... asserts half the tolerance, so that the 1e-3 of the GPU tests measures the kernels and not the oracle."""
    yy, xx = np.meshgrid(np.arange(SIZE) - 0.5 * (SIZE - 1), np.arange(SIZE) - 0.5 * (SIZE - 1), indexing="ij")
    sx, sy = np.array([1, -1, 1])[:, None, None], np.array([1, 1, -1])[:, None, None]
    u = np.random.default_rng(7 * n + 4).uniform(0.5, 1.5, (3, SIZE, SIZE))
    return (u * (1.0 + 0.5 * sx * xx / 8.0 + 0.4 * sy * yy / 8.0)).astype(np.float32)


def _norm_err(a, ref):
    """assert_grad_parity's normalised error, its maximum."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(a - ref) / (np.abs(ref) + 1e-3 * (np.abs(ref).max() + 1e-30))).max())


@functools.lru_cache(maxsize=None)
def _reference(kind, n):
    """One walk scene and everything the fp32 oracle says about it, computed once and shared (read only).  kind "full": every pixel walks all n
    entries; "stop64" / "stop128": the pixels of one bin saturate on both sides of the end of a 64-entry round."""
    g, bits = _scene(n, "narrow", OPACITY_FULL if kind == "full" else STOPS[kind][0])
    dpix = _dpix(n)
    o, oimg, oradii = oracle_render(g, "f32")
    solid, touched, bounds = fragile_bounds(o, dpix)
    return dict(g=g, bits=bits, dpix=dpix, o=o, oimg=oimg, oradii=oradii, og=o.backward(dpix), solid=solid, touched=touched, bounds=bounds,
                n_contrib=o.binning()["n_contrib"].astype(np.int64))


def _assert_scene_is_valid(kind, n, ref):
    """What a walk case rests on: a solid image and the list positions the pixels stop at."""
    assert ref["solid"].mean() >= 0.95
    assert (ref["oradii"] > 0).all()
    if kind == "full":
        assert (ref["n_contrib"] == n).all()
    else:
        assert set(STOPS[kind][1]) <= set(ref["n_contrib"].reshape(-1).tolist()), sorted(set(ref["n_contrib"].reshape(-1).tolist()))


def _walk_case(kind, n, lists):
    from gps_gaussian_amd import rasterizer as RZ
    ref = _reference(kind, n)
    _assert_scene_is_valid(kind, n, ref)
    img, radii, grads, info = hip_render(ref["g"], ref["dpix"])
    np.testing.assert_array_equal(radii, ref["oradii"])
    assert info["bin_cap"] == (RZ._DIRECT_CAP if lists == "direct" and n <= RZ._DIRECT_CAP else 0)
    st = _assert_lists(info, ref["bits"], "%s N=%d" % (kind, n))
    solid = ref["solid"]
    err = np.abs(img - ref["oimg"]).max(0)
    print("%s N=%d: RGB max err %.3e on solid pixels (%.3f of the image); gradients, max normalised error: %s" % (
        kind, n, err[solid].max(), solid.mean(), ", ".join("%s %.1e" % (k, _norm_err(grads[k], ref["og"][k])) for k in grads)))
    assert err[solid].max() <= RGB_TOL, "max err %.3e" % err[solid].max()
    np.testing.assert_array_equal(st["n_contrib"].cpu().numpy().astype(np.int64)[solid], ref["n_contrib"][solid])
    # strict_min = 0: every splat covers the whole 16 x 16 image, so one fragile pixel touches the whole cloud (the budget then bounds it)
    assert_grad_parity(grads, ref["og"], ref["touched"], ref["oradii"] > 0, bounds=ref["bounds"], strict_min=0.0)


@pytest.fixture(params=["valu", "tiles"])
def family(request, monkeypatch):
    """Both compositing kernel families: exponents on the vector ALUs / from bf16 matrix-core tiles."""
    monkeypatch.setenv("GPSGS_COMPOSITE", request.param)
    return request.param


@pytest.fixture(params=["direct", "scanned"])
def lists(request, monkeypatch):
    """Both forms of the per-bin lists; a list longer than a direct bin comes back repaired with scanned lists."""
    monkeypatch.setenv("GPSGS_LISTS", request.param)
    return request.param


@pytest.mark.gpu
@pytest.mark.parametrize("n", N_WALK)
def test_every_pixel_walks_a_list_of_exactly_n_entries(n, family, lists):
    """Forward and backward over lists that end one entry before, at and after the end of a group of 8 and of a round of 64, against the fp32 oracle."""
    _walk_case("full", n, lists)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(STOPS))
def test_pixels_of_one_bin_saturate_on_both_sides_of_a_round_boundary(kind, family, lists):
    """200 entries, opaque enough for T to reach 1e-4 around entry 64 (128): inside every bin some lanes end in one round and others in the next,
    and the backward starts from last contributors 63, 64 and 65 (127, 128 and 129)."""
    _walk_case(kind, N_STOP, lists)


# ---- 4. the opt-in walks --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _replays(kind, n):
    """The suite's own replays of the oracle's blend for a walk scene (tests/contrib_ref.py, tests/absgrad_ref.py), computed once."""
    from absgrad_ref import absgrad_replay
    from contrib_ref import contrib_stats
    ref = _reference(kind, n)
    return contrib_stats(ref["o"]), absgrad_replay(ref["o"], ref["dpix"])[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", OPT_IN_SCENES, ids=["%s_%d" % s for s in OPT_IN_SCENES])
def test_opt_in_walks_at_round_boundaries(kind, n, lists, monkeypatch):
    """The feature-map, depth / alpha, contribution and absgrad kernels have walk loops of their own: the identities and replays their own tests rely
    on (through the runner and the checks those tests share, tests/raster_run.py), on lists that end at a round boundary and on pixels that stop on
    either side of one."""
    monkeypatch.setenv("GPSGS_COMPOSITE", "valu")   # (what the opt-in kernels are compared with; they always are VALU kernels)
    ref = _reference(kind, n)
    _assert_scene_is_valid(kind, n, ref)
    g, dpix = ref["g"], ref["dpix"]
    assert (g["bg"] == 0).all()
    rng = np.random.default_rng(n)
    dpix2 = _dpix(n + 1)   # the feature map's gradient: positive, like dL/dpix
    dd, da = rng.standard_normal((2, SIZE, SIZE)).astype(np.float32)

    (rw, rm, rn), aref = _replays(kind, n)

    # F = 3 features equal to the colours (background 0): the feature map has the image's bits; dL/dfeatures is a plain run's dL/dcolours
    plain = run_view(g, dict(img=dpix))
    plain2 = run_view(g, dict(img=dpix2))
    feat = run_view(g, dict(img=dpix, feat=dpix2), feats=g["colors"])
    np.testing.assert_array_equal(feat["img"], plain["img"])
    np.testing.assert_array_equal(feat["radii"], plain["radii"])
    np.testing.assert_array_equal(feat["feat"], plain["img"])
    # (both are fp32 sums of the same 256 positive products w_p g_p per Gaussian, added in the order of two different kernels: whatever the orders,
    #  each is within (256 + 1) 2^-24 of the exact sum, element by element.  One pair left out of a sum moves it by ~1/256.)
    a, b = feat["grads"]["features"].astype(np.float64), plain2["grads"]["colors"].astype(np.float64)
    reached = rn > 0   # (a Gaussian behind every pixel's stop is blended nowhere: both gradients are exactly zero)
    assert (b[reached] > 0).all() and not b[~reached].any() and reached.sum() >= ref["n_contrib"].max() - (~ref["solid"]).sum()
    assert (np.abs(a - b) <= 2 * 257 * 2.0 ** -24 * b).all(), float((np.abs(a - b)[reached] / b[reached]).max())
    for k in GEOM:
        close(feat["grads"][k], plain["grads"][k].astype(np.float64) + plain2["grads"][k], 1e-5, k)

    # depth / alpha maps and their gradients equal a plain run with colours (z, 1, 0)
    _, alp, _, _, _ = check_against_plain(g, dd, da)
    assert 0.0 <= alp.min() and alp.max() <= 1.0

    # contribution statistics and absgrad on / off: image, maps and every gradient keep their bits
    cot = dict(img=dpix, depth=dd[None], alpha=da[None])
    off = run_view(g, cot, extras=True)
    on = run_view(g, cot, extras=True, contrib=True, absgrad=True)
    np.testing.assert_array_equal(off["img"], plain["img"])
    for k in ("img", "radii", "depth", "alpha"):
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
    assert set(on["grads"]) == set(off["grads"])
    for k in off["grads"]:
        np.testing.assert_array_equal(on["grads"][k], off["grads"][k], err_msg=k)
    check_absgrad_structure(on)
    check_contrib_structure(on)
    s_w, s_a = float(on["w"].astype(np.float64).sum()), float(on["alpha"].astype(np.float64).sum())
    assert abs(s_w - s_a) <= 1e-5 * s_a

    # ... and against the replays of the oracle's blend (the image's gradient alone, as the replays take it)
    both = run_view(g, dict(img=dpix), contrib=True, absgrad=True)
    for k in plain["grads"]:
        np.testing.assert_array_equal(both["grads"][k], plain["grads"][k], err_msg=k)
    ok = ~ref["touched"]
    np.testing.assert_array_equal(both["n"][ok], rn[ok])
    assert close_each(both["w"][ok], rw[ok]).all() and close_each(both["m"][ok], rm[ok]).all()
    if kind == "full":
        assert ok.all() and (both["n"] == SIZE * SIZE).all()   # every Gaussian is blended into every pixel
    assert_grad_parity({"means2D": pad(both["abs"])}, {"means2D": pad(aref)}, ref["touched"], ref["oradii"] > 0, bounds=ref["bounds"],
                       strict_min=0.0)
    # one pixel in the loss: one term per Gaussian, so the absolute sum is the magnitude of the signed one
    one = np.zeros_like(dpix)
    one[:, 5, 9] = (0.7, -1.3, 0.4)
    s = run_view(g, dict(img=one), absgrad=True)
    sref = np.abs(s["grads"]["means2D"][:, :2])
    assert (sref > 0).any()
    assert (np.abs(s["abs"] - sref) <= 1e-4 * sref + 1e-6 * sref.max()).all(), np.abs(s["abs"] - sref).max()


# ---- 5. CPU: the scene's validity conditions on the oracle, and the list check's teeth -------------------------------------------------------------

@pytest.mark.parametrize("n", N_WAVE + N_LARGE)
def test_scene_layouts_put_the_chosen_depth_bits_on_either_side_of_the_threshold(n):
    """Every layout of every N: the oracle's view-space depths carry exactly the chosen bits and every Gaussian is listed; `below` and `at` sit one
    ulp either side of the composite-key threshold; `ties3` has runs of equal depths, `one_depth` one run, the others none."""
    for layout in _layouts_for(n):
        g, bits = _scene(n, layout)
        o, _, oradii = oracle_render(g, "f32")
        np.testing.assert_array_equal(o.geom()["depth"].astype(np.float32).view(np.uint32), bits)
        assert (oradii > 0).all() and o.num_rendered == n
        assert float(g["means3D"][:, 2].max()) <= 64.0
        spread, distinct = int(bits.max()) - int(bits.min()), len(np.unique(bits))
        if layout in ("below", "at"):
            assert distinct == n and spread == _threshold(n) - (1 if layout == "below" else 0)
            assert (spread < _threshold(n)) == (layout == "below")   # sort_wave_regs32's own test
        elif layout == "narrow":
            assert distinct == n and (n < 2 or n > 1024 or spread < _threshold(n))
        elif layout == "ties3":
            assert distinct <= max(1, (n + 2) // 3) and spread < (1 << 20)
        else:
            assert distinct == 1
        if n >= 63 and layout != "one_depth":
            assert not np.array_equal(_expected_list(bits), np.arange(n))   # ids are not in depth order to begin with


@pytest.mark.parametrize("kind,n", [("full", n) for n in N_WALK] + [(k, N_STOP) for k in sorted(STOPS)])
def test_walk_scenes_stop_where_they_claim_on_the_fp32_and_fp64_oracles(kind, n):
    ref = _reference(kind, n)
    _assert_scene_is_valid(kind, n, ref)
    np.testing.assert_array_equal(ref["o"].geom()["depth"].astype(np.float32).view(np.uint32), ref["bits"])
    o64, _, _ = oracle_render(ref["g"], "f64")
    np.testing.assert_array_equal(o64.binning()["n_contrib"].astype(np.int64), ref["n_contrib"])
    # the reference of the gradient check is itself well inside the tolerance (see _dpix): fp32 oracle against the fp64 oracle under the same decisions
    o64d, _, _ = oracle_render(ref["g"], "f64", decisions=ref["o"].geom())
    og64 = o64d.backward(ref["dpix"])
    for k in ref["og"]:
        assert _norm_err(ref["og"][k], og64[k]) <= 0.5e-3, (k, _norm_err(ref["og"][k], og64[k]))
        assert k == "rotations" or np.abs(og64[k]).max() > 0, k
    if kind == "full":
        assert float(ref["o"].binning()["final_T"].min()) > 1e-4 * 10   # far from the stop
    else:
        rows = ref["n_contrib"].reshape(2, 8, 2, 8).transpose(0, 2, 1, 3).reshape(4, 64)   # the four 8 x 8 bins
        edge = STOPS[kind][1][1]
        assert all((r <= edge).any() and (r > edge).any() for r in rows)   # in every bin some lanes end in one round, others in the next


def test_the_list_check_rejects_a_swapped_tie_a_duplicated_id_and_a_missing_id():
    bits = np.array([7, 5, 5, 9, 5, 7], np.uint32)
    good = np.array([1, 2, 4, 0, 5, 3])
    np.testing.assert_array_equal(_expected_list(bits), good)
    assert _list_fault(good, bits) is None
    swapped_tie = np.array([1, 4, 2, 0, 5, 3])      # still ascending in depth: only the id rule catches it
    assert (np.diff(bits[swapped_tie].astype(np.int64)) >= 0).all()
    assert "differ" in _list_fault(swapped_tie, bits)
    duplicated = np.array([1, 2, 2, 0, 5, 3])       # ... and still ascending in (depth, id), not strictly
    assert "differ" in _list_fault(duplicated, bits)
    missing = np.array([1, 2, 4, 0, 3])
    assert "entries instead of" in _list_fault(missing, bits)
    for n, layout in ((65, "ties3"), (64, "one_depth"), (129, "at")):
        _, b = _scene(n, layout)
        want = _expected_list(b)
        assert _list_fault(want, b) is None
        assert _list_fault(want[::-1], b) is not None
        assert _list_fault(np.concatenate([want[:-1], want[:1]]), b) is not None
