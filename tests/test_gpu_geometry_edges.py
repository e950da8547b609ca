"""GPU (-m gpu): the geometry path in front of the rasteriser at its kernel edges -- flow -> inverse depth -> world points (unproject.hip) and the
mask compaction + pack (pack_views.hip) -- against the plain references of tests/geometry_ref.py.  The inputs, the case lists and the comparison
helpers are the ones tests/test_geometry_ref.py runs on the CPU (float32 restatement within the float64 bounds, mutants rejected).

Unprojection: depth and valid must equal the float32 restatement bit for bit; xyz and d_flow must sit within the rounding-count bounds of the
float64 formulas (geometry_ref.xyz_fault / dflow_fault), and -- since the kernels are built without contraction and with correctly rounded
divisions -- they equal the float32 restatement bit for bit as well (BIT_EQUAL).  The pack moves values and does one multiply and one add per
colour: everything about it is bit-equal."""
import ctypes as C

import numpy as np
import pytest

import geometry_ref as G

pytestmark = pytest.mark.gpu

BIT_EQUAL = ("xyz", "d_flow")      # keys that must ALSO equal unproject_f32's bits (on top of the float64 bounds, which stay the criterion)
ARGS = ("ref_intr", "intr", "extr", "Tf_x")


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a, dev=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev() if dev is None else dev)


def _np(t):
    return t.detach().cpu().numpy()


def _report(tag, got, inp, gd=None, gx=None):
    ux, ud = G.unproject_units(got, inp, gd, gx)
    print("%s: xyz %.2f%s x 2^-24 x magnitude" % (tag, ux, "" if ud is None else ", d_flow %.2f" % ud))


# ---- unprojection through unproject() -----------------------------------------------------------------------------------------------------------------
def _wrapper(inp, mask=None, flow=None, loss="both", gd=None, gx=None):
    """unproject() + backward -> dict of numpy results.  loss: both | xyz | depth | permuted | expanded."""
    import torch
    from gps_gaussian_amd.unproject import unproject
    flow = (_t(inp["flow"]) if flow is None else flow).requires_grad_(True)
    mask = _t(inp["mask"]) if mask is None else mask
    depth, xyz, valid = unproject(flow, mask, *(_t(inp[k]) for k in ARGS))
    B, S2, _ = xyz.shape
    if loss == "both":
        l = (depth * _t(gd)).sum() + (xyz * _t(gx)).sum()
    elif loss == "xyz":
        l = (xyz * _t(gx)).sum()
    elif loss == "depth":
        l = (depth * _t(gd)).sum()
    elif loss == "permuted":       # the consumer works on the [B,3,S2] view: the gradient comes back as a permuted view of [B,3,S2] memory
        l = (xyz.permute(0, 2, 1) * _t(np.transpose(gx, (0, 2, 1)))).sum()
    elif loss == "expanded":       # sum(): the gradient is one element expanded with all-zero strides
        l = xyz.sum()
    l.backward()
    torch.cuda.synchronize()
    return dict(depth=_np(depth), xyz=_np(xyz), valid=_np(valid), d_flow=_np(flow.grad).astype(np.float32))


@pytest.mark.parametrize("B,S,seed", G.UNPROJECT_CASES)
def test_unproject_matches_both_references_at_every_size(B, S, seed):
    inp = G.unproject_inputs(B, S, seed)
    gd, gx = G.unproject_grads(B, S, seed)
    got = _wrapper(inp, gd=gd, gx=gx)
    _report("unproject() B %d S %d" % (B, S), got, inp, gd, gx)
    assert G.unproject_fault(got, inp, gd, gx, want_bits=BIT_EQUAL) is None
    zd = G.zero_disparity_pixels(inp)
    assert zd.any() or S == 1
    assert not got["valid"][zd].any() and (got["d_flow"].reshape(B, -1)[zd] != 0).all()      # d = 0 under mask 1: invalid, and still a gradient


@pytest.mark.parametrize("loss", ["xyz", "depth", "permuted", "expanded"])
@pytest.mark.parametrize("B,S,seed", [c for c in G.UNPROJECT_CASES if c[1] in (16, 17)])
def test_unproject_gradient_layouts_autograd_delivers(B, S, seed, loss):
    inp = G.unproject_inputs(B, S, seed)
    gd, gx = G.unproject_grads(B, S, seed)
    got = _wrapper(inp, loss=loss, gd=gd, gx=gx)
    # autograd materialises the gradient of the output the loss does not use as zeros
    g_depth = gd if loss == "depth" else np.zeros_like(gd)
    g_xyz = {"depth": np.zeros_like(gx), "expanded": np.ones_like(gx)}.get(loss, gx)
    _report("unproject() %s B %d S %d" % (loss, B, S), got, inp, g_depth, g_xyz)
    assert G.unproject_fault(got, inp, g_depth, g_xyz, want_bits=BIT_EQUAL) is None


@pytest.mark.parametrize("variant", ["mask_1ch", "mask_bool", "mask_bool_1ch", "mask_cpu", "flow_fp16"])
def test_unproject_mask_and_flow_variants(variant):
    import torch
    B, S, seed = 3, 17, 273
    inp = G.unproject_inputs(B, S, seed)
    gd, gx = G.unproject_grads(B, S, seed)
    mask, flow = None, None
    if variant == "mask_1ch":
        mask = _t(inp["mask"][:, :1])
    elif variant == "mask_bool":
        mask = _t(inp["mask"] != 0)
    elif variant == "mask_bool_1ch":
        mask = _t(inp["mask"][:, :1] != 0)
    elif variant == "mask_cpu":
        mask = torch.from_numpy(inp["mask"])
    elif variant == "flow_fp16":
        # 6e4 survives fp16, the zero-disparity value does not.  The gradient of a half input is handed back as half by autograd, so the
        # float32 leaf sits in front of the cast and d_flow is compared after the same rounding to fp16.
        from gps_gaussian_amd.unproject import unproject
        leaf = _t(inp["flow"]).requires_grad_(True)
        depth, xyz, valid = unproject(leaf.half(), _t(inp["mask"]), *(_t(inp[k]) for k in ARGS))
        ((depth * _t(gd)).sum() + (xyz * _t(gx)).sum()).backward()
        torch.cuda.synchronize()
        inp = dict(inp, flow=inp["flow"].astype(np.float16).astype(np.float32))
        got = dict(depth=_np(depth), xyz=_np(xyz), valid=_np(valid))
        assert G.unproject_fault(got, inp, want_bits=BIT_EQUAL[:1]) is None
        r64 = G.unproject_f64(got["depth"], inp["mask"], inp["intr"], inp["extr"], inp["Tf_x"], g_depth=gd, g_xyz=gx)
        with np.errstate(over="ignore"):
            lo, hi = ((r64["d_flow"] + s * G.DFLOW_ROUNDINGS * G.U * r64["d_flow_mag"]).astype(np.float16) for s in (-1, 1))
        d16 = _np(leaf.grad).astype(np.float16)
        assert (np.minimum(lo, hi) <= d16).all() and (d16 <= np.maximum(lo, hi)).all()       # rounding to fp16 is monotonic
        return
    got = _wrapper(inp, mask=mask, flow=flow, gd=gd, gx=gx)
    assert G.unproject_fault(got, inp, gd, gx, want_bits=BIT_EQUAL) is None


# ---- unprojection through the C entry points: device-array and host-array cameras, NULL gradients, explicit strides -----------------------------------
def _c_call(inp, form, grads):
    """up_unproject_forward[_dev] + one backward per entry of grads [(g_depth | None, g_xyz | None, layout)] -> (forward dict, [d_flow])."""
    import torch
    from gps_gaussian_amd import _capi
    lib = _capi.lib()
    dev = _dev()
    B, _, S, _ = inp["flow"].shape
    S2 = S * S
    flow, mask = _t(inp["flow"]), _t(inp["mask"])
    depth = torch.full((B, 1, S, S), 7.5, device=dev)
    xyz = torch.full((B, S2, 3), 7.5, device=dev)
    valid = torch.full((B, S2), 9, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if form == "host":
        host = [np.ascontiguousarray(a, np.float32) for a in (inp["ref_intr"].reshape(B, 9), inp["intr"].reshape(B, 9), inp["extr"][:, :3, :4].reshape(B, 12),
                                                               inp["Tf_x"].reshape(B))]
        cams = [a.ctypes.data_as(C.c_void_p) for a in host]
        fwd, bwd = lib.up_unproject_forward, lib.up_unproject_backward
    else:
        cam_t = _t(np.concatenate([inp["ref_intr"].reshape(B, 9), inp["intr"].reshape(B, 9), inp["extr"][:, :3, :4].reshape(B, 12),
                                   inp["Tf_x"].reshape(B, 1)], 1).astype(np.float32))
        cams = [p(cam_t)]
        fwd, bwd = lib.up_unproject_forward_dev, lib.up_unproject_backward_dev
    assert fwd(B, S, p(flow), p(mask), mask.stride(0), *cams, p(depth), p(xyz), p(valid), st) == 0
    outs = []
    for g_depth, g_xyz, layout in grads:
        gd = _t(g_depth) if g_depth is not None else None
        gx, strides = None, (0, 0, 0)
        if g_xyz is not None:
            if layout == "contiguous":
                gx, strides = _t(g_xyz), (3 * S2, 3, 1)
            elif layout == "permuted":      # memory [B,3,S2]: channel stride S2, pixel stride 1
                gx, strides = _t(np.transpose(g_xyz, (0, 2, 1))), (3 * S2, 1, S2)
            elif layout == "expanded":      # one element, all strides zero
                gx, strides = _t(g_xyz.reshape(-1)[:1]), (0, 0, 0)
        d_flow = torch.full((B, 1, S, S), 7.5, device=dev)
        assert bwd(B, S, p(depth), p(mask), mask.stride(0), *cams, p(gd), p(gx), *strides, p(d_flow), st) == 0
        outs.append(d_flow)
    torch.cuda.synchronize()
    return dict(depth=_np(depth), xyz=_np(xyz), valid=_np(valid)), [_np(o) for o in outs]


def _c_check(tag, inp, gd, gx, forms):
    grads = [(gd, gx, "contiguous"), (None, gx, "permuted"), (gd, None, None), (None, np.ones_like(gx), "expanded"), (gd, gx, "permuted")]
    res = {}
    for form in forms:
        fwd, dflows = _c_call(inp, form, grads)
        assert set(np.unique(fwd["valid"]).tolist()) <= {0, 1}                              # one byte per pixel, 0 or 1, every one written
        res[form] = (fwd, dflows)
        for (g_depth, g_xyz, layout), d_flow in zip(grads, dflows):
            got = dict(fwd, d_flow=d_flow)
            what = "%s %s-array form, g_depth %s, g_xyz %s" % (tag, form, "NULL" if g_depth is None else "given", layout or "NULL")
            _report(what, got, inp, g_depth, g_xyz)
            fault = G.unproject_fault(got, inp, g_depth, g_xyz, want_bits=BIT_EQUAL)
            assert fault is None, "%s: %s" % (what, fault)
    if len(forms) == 2:                                                                       # same arithmetic: same bits
        (f0, d0), (f1, d1) = res[forms[0]], res[forms[1]]
        for k in f0:
            assert G.bits_fault(k, f0[k], f1[k]) is None
        for a, b in zip(d0, d1):
            assert G.bits_fault("d_flow", a, b) is None


@pytest.mark.parametrize("B,S,seed", G.UNPROJECT_CASES)
def test_unproject_c_entry_points_null_gradients_and_strides(B, S, seed):
    inp = G.unproject_inputs(B, S, seed)
    gd, gx = G.unproject_grads(B, S, seed)
    _c_check("B %d S %d" % (B, S), inp, gd, gx, ("device", "host"))


@pytest.mark.parametrize("B,S,seed", G.HOST_CASES)
def test_host_form_chunks_read_their_own_samples(B, S, seed):
    """Every sample has its own cameras, flow and mask, so a launch chunk that reads any input from chunk 0 fails here
    (tests/test_geometry_ref.py shows that each such error is rejected, and that the fixture tiled with arange(n) % 2 cannot see them)."""
    inp = G.unproject_inputs(B, S, seed)
    gd, gx = G.unproject_grads(B, S, seed)
    _c_check("B %d S %d" % (B, S), inp, gd, gx, ("host", "device"))
    got = _wrapper(inp, gd=gd, gx=gx)
    assert G.unproject_fault(got, inp, gd, gx, want_bits=BIT_EQUAL) is None


# ---- pack ---------------------------------------------------------------------------------------------------------------------------------------------------
LEAVES = ("xyz", "img", "rot_maps", "scale_maps", "opacity_maps")


def _pack_data(maps, valid, valid_kind="bool", permuted_xyz=False, requires=LEAVES):
    import torch
    B, V, S2 = valid.shape
    names = tuple("view%d" % v for v in range(V))
    if valid_kind == "bool":
        val = _t(valid)                                          # each view a [B,S2] slice of [B,V,S2]: batch stride V S2
    elif valid_kind == "uint8":
        val = _t(np.where(valid, np.where(np.arange(S2) % 2 == 0, 2, 255), 0).astype(np.uint8))
    elif valid_kind == "float":
        val = _t(np.where(valid, np.where(np.arange(S2) % 2 == 0, 0.5, 1.0), 0.0).astype(np.float32))
    data = {}
    for v, name in enumerate(names):
        d = {k: _t(maps[v][k]) for k in LEAVES}
        if permuted_xyz:
            d["xyz"] = d["xyz"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
            assert not d["xyz"].is_contiguous() or S2 == 1
        for k in requires:
            d[k].requires_grad_(True)
        d["pts_valid"] = val[:, v]
        data[name] = d
    return data, names


def _packed(out):
    return dict(zip(G.OUT_KEYS + ("offsets", "row_of_pixel"), (_np(t) for t in out)))


def _pack_fwd_bwd(case, valid_kind="bool", permuted_xyz=False, requires=LEAVES, empty_samples=()):
    """pack_views forward + backward on one case, compared with pack_ref / pack_bwd_ref; -> (data, names, out tensors, ref)."""
    import torch
    from gps_gaussian_amd.pack import pack_views
    B, V, H, W, pattern, seed = case
    maps, valid = G.pack_inputs(B, V, H, W, pattern, seed, empty_samples=empty_samples)
    ref = G.pack_ref(maps, valid)
    data, names = _pack_data(maps, valid, valid_kind, permuted_xyz, requires)
    out = pack_views(data, views=names, return_rows=True)
    got = _packed(out)
    assert all(got[k].shape[0] == B * V * H * W for k in G.OUT_KEYS)
    fault = G.pack_fault(got, ref)
    assert fault is None, fault
    total = int(ref["offsets"][-1])
    if requires:
        g = G.pack_row_grads(total, seed)
        diff = [(t, k) for t, k in zip(out[:5], G.OUT_KEYS) if t.requires_grad]
        assert ("rgb" in [k for _, k in diff]) == ("img" in requires)
        loss = sum((t[:total] * _t(g[k])).sum() for t, k in diff)
        loss.backward()
        torch.cuda.synchronize()
        want = G.pack_bwd_ref(ref["row_of_pixel"], {k: g[k] for _, k in diff}, (H, W))
        grads = [{k: _np(data[n][k].grad) for k in requires} for n in names]
        assert all(data[n][k].grad is None for n in names for k in LEAVES if k not in requires)
        fault = G.pack_bwd_fault(grads, want, keys=requires)
        assert fault is None, fault
    return data, names, out, ref


@pytest.mark.parametrize("case", G.pack_cases(), ids=lambda c: "B%d-V%d-%dx%d-%s" % c[:5])
def test_pack_forward_and_backward_are_bit_exact(case):
    _pack_fwd_bwd(case)


@pytest.mark.parametrize("valid_kind,permuted_xyz", [("uint8", False), ("float", True), ("bool", True), ("uint8", True)])
@pytest.mark.parametrize("case", [(3, 2, 25, 41, "random", 501), (1, 3, 48, 64, "alternate_64", 502), (3, 4, 7, 9, "random", 503)],
                         ids=lambda c: "B%d-V%d-%dx%d-%s" % c[:5])
def test_pack_validity_types_and_permuted_xyz(case, valid_kind, permuted_xyz):
    _pack_fwd_bwd(case, valid_kind=valid_kind, permuted_xyz=permuted_xyz)


@pytest.mark.parametrize("requires", [("opacity_maps",), ("xyz", "rot_maps", "scale_maps", "opacity_maps"), ()], ids=["opacity-only", "all-but-img", "none"])
@pytest.mark.parametrize("case", [(3, 2, 25, 41, "random", 511), (3, 3, 48, 64, "hole_block", 512)], ids=lambda c: "B%d-V%d-%dx%d-%s" % c[:5])
def test_pack_backward_with_some_leaves_only(case, requires):
    _pack_fwd_bwd(case, requires=requires)


def test_pack_scan_over_more_than_one_chunk():
    """B V nblk = 1248 > 1024: the scan's carry loop runs twice, sample 5's offset is written in the second chunk, sample 3 is empty."""
    b = G.BIG_PACK
    _pack_fwd_bwd((b["B"], b["V"], b["H"], b["W"], b["pattern"], b["seed"]), empty_samples=b["empty_samples"])


@pytest.mark.parametrize("case", [(3, 3, 25, 41, "random", 521), (1, 2, 48, 64, "hole_block", 522), (3, 2, 1, 1, "random", 523), (3, 2, 25, 41, "none", 524)],
                         ids=lambda c: "B%d-V%d-%dx%d-%s" % c[:5])
def test_pack_features_and_unpack_rows_follow_the_row_map(case):
    import torch
    from gps_gaussian_amd.pack import pack_features, unpack_rows
    B, V, H, W, _, seed = case
    data, names, out, ref = _pack_fwd_bwd(case, requires=())
    rows = out[6]
    total = int(ref["offsets"][-1])
    rng = np.random.default_rng(seed)
    for F in (1, 5):
        feats = [rng.standard_normal((B, F, H, W)).astype(np.float32) for _ in names]
        for n, f in zip(names, feats):
            data[n]["feat"] = _t(f).requires_grad_(True)
        packed = pack_features(data, "feat", rows, views=names)
        want = G.pack_features_ref(feats, ref["row_of_pixel"])
        assert G.bits_fault("pack_features F=%d" % F, _np(packed), want) is None
        assert (want[total:] == 0).all()
        w = rng.standard_normal(want.shape).astype(np.float32)
        (packed * _t(w)).sum().backward()
        for v, n in enumerate(names):                            # each valid pixel gets its row's weight, an invalid one zero
            r = ref["row_of_pixel"][:, v]
            g_want = np.where((r >= 0)[..., None], w[np.maximum(r, 0)], 0).astype(np.float32)
            assert G.bits_fault("d_feat view %d" % v, _np(data[n]["feat"].grad).reshape(B, F, -1).transpose(0, 2, 1), g_want) is None
    for dtype in (np.float32, np.int32):
        vals = (rng.standard_normal(B * V * H * W) * 100).astype(dtype)
        got = unpack_rows(_t(vals), rows)
        assert G.bits_fault("unpack_rows", _np(got), G.unpack_rows_ref(vals, ref["row_of_pixel"])) is None
    torch.cuda.synchronize()


def test_pack_backward_c_call_with_null_gradients_and_null_outputs():
    """gsr_pack_views_backward called directly: NULL g_* (autograd never produces them) give exactly zero, NULL d_* -- a whole kind or one view of
    it -- are skipped, and what was not requested keeps its sentinel although it lies between requested tensors in one allocation."""
    import torch
    from gps_gaussian_amd import _capi
    lib = _capi.lib()
    dev = _dev()
    B, V, H, W, seed = 3, 3, 25, 41, 531
    S2 = H * W
    maps, valid = G.pack_inputs(B, V, H, W, "random", seed)
    ref = G.pack_ref(maps, valid)
    rop = _t(ref["row_of_pixel"])
    g = G.pack_row_grads(int(ref["offsets"][-1]), seed)
    given = {"xyz": g["xyz"], "opacity": g["opacity"], "rot": g["rot"]}                      # g_rgb and g_scale are NULL
    gt = {k: _t(a) for k, a in given.items()}
    chans = dict(zip(LEAVES, (3, 3, 4, 3, 1)))
    # which (kind, view) outputs are requested: xyz not for view 1; img for all (g_rgb NULL: zeros); rot_maps: the whole pointer array is NULL;
    # scale_maps for view 0 only (g_scale NULL: zeros); opacity_maps for all
    wanted = {"xyz": (0, 2), "img": (0, 1, 2), "rot_maps": None, "scale_maps": (0,), "opacity_maps": (0, 1, 2)}
    SENT = 7.5
    arena = torch.full((sum(chans.values()) * V * B * S2,), SENT, device=dev)
    slot, pos = {}, 0
    for k in LEAVES:
        for v in range(V):
            slot[k, v] = arena[pos:pos + B * S2 * chans[k]]
            pos += B * S2 * chans[k]
    arrays = {}
    for k in LEAVES:
        if wanted[k] is None:
            arrays[k] = None
        else:
            arrays[k] = (C.c_void_p * V)(*[slot[k, v].data_ptr() if v in wanted[k] else None for v in range(V)])
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rc = lib.gsr_pack_views_backward(B, V, S2, p(rop), p(gt["xyz"]), None, p(gt["rot"]), None, p(gt["opacity"]), arrays["xyz"], arrays["img"],
                                     arrays["rot_maps"], arrays["scale_maps"], arrays["opacity_maps"], C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    want = G.pack_bwd_ref(ref["row_of_pixel"], given, (H, W))
    for k in LEAVES:
        for v in range(V):
            got = _np(slot[k, v])
            if wanted[k] is not None and v in wanted[k]:
                assert G.bits_fault("d_%s view %d" % (k, v), got, want[v][k].reshape(-1)) is None
                if k in ("img", "scale_maps"):
                    assert (got == 0).all()
            else:
                assert (got == SENT).all(), (k, v)


# ---- chain: unproject -> pack -----------------------------------------------------------------------------------------------------------------------------
def test_unproject_feeds_pack_bits_and_gradient():
    import torch
    from gps_gaussian_amd.pack import pack_views
    from gps_gaussian_amd.unproject import unproject
    c = G.CHAIN_CASE
    B, S, V = c["B"], c["S"], c["V"]
    S2 = S * S
    names = tuple("view%d" % v for v in range(V))
    inps = [G.unproject_inputs(B, S, c["seed"] + v) for v in range(V)]
    maps, _ = G.pack_inputs(B, V, S, S, "all", c["seed"])
    data, flows, ups = {}, [], []
    for v, n in enumerate(names):
        flow = _t(inps[v]["flow"]).requires_grad_(True)
        depth, xyz, valid = unproject(flow, _t(inps[v]["mask"]), *(_t(inps[v][k]) for k in ARGS))
        flows.append(flow)
        ups.append(dict(depth=_np(depth), xyz=_np(xyz), valid=_np(valid)))
        data[n] = dict(xyz=xyz, pts_valid=valid, img=_t(maps[v]["img"]), rot_maps=_t(maps[v]["rot_maps"]), scale_maps=_t(maps[v]["scale_maps"]),
                       opacity_maps=_t(maps[v]["opacity_maps"]))
    out = pack_views(data, views=names, return_rows=True)
    valid = np.stack([u["valid"] for u in ups], 1)
    for v in range(V):
        maps[v]["xyz"] = ups[v]["xyz"]
    ref = G.pack_ref(maps, valid)                                 # the unprojected xyz gathered by the unprojected valid mask
    fault = G.pack_fault(_packed(out), ref)
    assert fault is None, fault
    total = int(ref["offsets"][-1])
    assert 0 < total < B * V * S2
    w = np.random.default_rng(c["seed"]).standard_normal((total, 3)).astype(np.float32)
    (out[0][:total] * _t(w)).sum().backward()
    torch.cuda.synchronize()
    g_views = G.pack_bwd_ref(ref["row_of_pixel"], {"xyz": w}, (S, S))
    for v in range(V):
        got = dict(ups[v], d_flow=_np(flows[v].grad))
        gd0, gx = np.zeros((B, 1, S, S), np.float32), g_views[v]["xyz"]
        _report("chain view %d" % v, got, inps[v], gd0, gx)
        fault = G.unproject_fault(got, inps[v], gd0, gx, want_bits=BIT_EQUAL)
        assert fault is None, fault
