"""CPU: what the rasteriser's forward and backward entry points RETURN for calls that end before anything is launched, and what the workspace queries
report, pinned against a recording (tests/golden/capi_return_codes.json) made with the library as it stood before the C layer got its call records.

Every case has P = 1 (or 0), an 8 x 8 image and dummy device addresses that are never dereferenced: either an argument is invalid, or the workspace is 0
bytes or one byte short of what the matching gsr_workspace_bytes_* query reports -- so the call ends at GPSGS_E_INVALID, at GPSGS_E_WORKSPACE, or (a
backward of an empty view without camera outputs) at GPSGS_OK.  The cases are single faults per entry point -- every pointer NULL and misaligned, the
input-exclusivity rules, the SH bounds, bin capacities, negative sizes, an over-wide image, the reserved fields, channel counts, a short camera scratch --
and pairs of faults that pin which check comes first.  (The exported entry points take at most one of GsrFeatures / GsrContrib / GsrAbsGrad, so the refusal
of two tails in one call cannot be reached from here; the pairs with a workspace sized for ANOTHER option's tail stand in for it.)

Re-record (only when a return code changes on purpose):  GPSGS_LIB=<library to record> python tests/test_capi_return_codes.py"""
import json
import os

from conftest import ROOT

from gps_gaussian_amd import _capi

# the by-name call builder, under the names the case generator below was written with
from capi_run import BWD_PTRS, CAM_PTRS, FWD_PTRS, VIEW_PTRS, D as _D, call as _call, has_cam as _has_cam, has_ext as _has_ext, need as _need, spec as _spec

GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_return_codes.json")
FORWARDS = ("gsr_forward", "gsr_forward_notify", "gsr_forward_ex", "gsr_forward_features", "gsr_forward_contrib")
BACKWARDS = ("gsr_backward", "gsr_backward_ex", "gsr_backward_camera", "gsr_backward_features", "gsr_backward_absgrad")
EXT_PTRS = ("row_range", "shs", "campos", "cov3D_precomp", "dL_dsh", "dL_dcov3D", "out_depth", "out_alpha")  # (the map slots: dL_ddepth / dL_dalpha in a backward)
OPT_PTRS = {"gsr_forward_features": ("features", "out_features"), "gsr_backward_features": ("features", "dL_dfeaturemap", "dL_dfeatures"),
            "gsr_forward_contrib": ("weight_sum", "weight_max", "pixel_count"), "gsr_backward_absgrad": ("absgrad",)}
BAD_OPT = {"gsr_forward_features": dict(channels=65), "gsr_backward_features": dict(channels=65), "gsr_forward_contrib": dict(reserved=_D),
           "gsr_backward_absgrad": dict(reserved=_D)}  # an invalid option struct per entry point that takes one
W_MAX = 65535 * 16


def _cases(lib):
    """[(id, entry, spec)]: every spec ends before a HIP call (see the module docstring)."""
    out = []

    def add(entry, name, **over):
        out.append(("%s:%s" % (entry, name), entry, _spec(entry, **over)))

    for e in FORWARDS + BACKWARDS:
        fwd, sh_ext = e in FORWARDS, dict(shs=_D, campos=_D, sh_degree=3, sh_coeffs=16, dL_dsh=_D)
        add(e, "valid")
        add(e, "one byte short", ws=_need(lib, e, _spec(e)) - 1)
        add(e, "no option", opt=None)
        for k in VIEW_PTRS + (FWD_PTRS if fwd else BWD_PTRS):
            add(e, k + " NULL", **{k: None})
            add(e, k + " misaligned", **{k: _D + 2})
            add(e, k + " NULL, one byte short", ws=_need(lib, e, _spec(e)) - 1, **{k: None})
        for k in OPT_PTRS.get(e, ()):
            add(e, k + " NULL", opt={k: None})
            add(e, k + " misaligned", opt={k: _D + 2})
            add(e, k + " alone", opt=dict({j: None for j in OPT_PTRS[e]}, **{k: _D}))
        for bad in (dict(P=-1), dict(cap=-1), dict(cap=1 << 31), dict(W=0), dict(H=0), dict(W=-8), dict(W=W_MAX + 1), dict(H=W_MAX + 1), dict(W=W_MAX), dict(flags=1024, opacities=None)):
            add(e, "bad %r" % sorted(bad.items()), **bad)
        add(e, "empty view", P=0, cap=0)  # a backward: GPSGS_OK, nothing to do (no camera outputs asked for)
        if not fwd:
            add(e, "empty view, NULL inputs", P=0, cap=0, means3D=None, workspace=None)
        if e == "gsr_forward_contrib" or e == "gsr_backward_absgrad":
            add(e, "reserved set", opt=dict(reserved=_D))
            add(e, "reserved set, nothing wanted", opt=dict({k: None for k in OPT_PTRS[e]}, reserved=_D))
            add(e, "workspace of the 1-channel feature size", ws=lib.gsr_workspace_bytes_features(1, 8, 8, 1024, 0, 1, 0))  # another option's (shorter) tail
        if e.endswith("_features"):
            for ch in (0, 65, -1, 1, 64):
                add(e, "channels %d" % ch, opt=dict(channels=ch))
            add(e, "channels 65, one byte short", opt=dict(channels=65), ws=_need(lib, e, _spec(e, opt=None)) - 1)
        if e == "gsr_backward_features":
            add(e, "workspace of the absgrad size", ws=lib.gsr_workspace_bytes_absgrad(1, 8, 8, 1024, 0))  # 8 bytes per slot where 3 channels need 12
            add(e, "map gradient only: no feature tail", opt=dict(dL_dfeatures=None), ws=lib.gsr_workspace_bytes_ex(1, 8, 8, 1024, 0, 0) - 1)
            add(e, "feature gradient only: no feature tail", opt=dict(dL_dfeaturemap=None), ws=lib.gsr_workspace_bytes_ex(1, 8, 8, 1024, 0, 0) - 1)
        if _has_ext(e):
            for k in EXT_PTRS:
                add(e, "ext " + k, ext={k: _D})
                add(e, "ext %s misaligned" % k, ext={k: _D + 2})
            add(e, "colours and SH", ext=sh_ext)
            add(e, "SH", colors=None, dL_dcolors=None, ext=sh_ext)
            for k, v in (("sh_degree", 4), ("sh_coeffs", 17), ("sh_coeffs", 15), ("campos", None), ("dL_dsh", None)):
                add(e, "SH %s %r" % (k, v), colors=None, ext=dict(sh_ext, **{k: v}))
            add(e, "SH degree 2 of 8 coefficients", colors=None, ext=dict(sh_ext, sh_degree=2, sh_coeffs=8))
            cov = dict(cov3D_precomp=_D, dL_dcov3D=_D)
            add(e, "covariances", scales=None, rotations=None, ext=cov)
            add(e, "covariances and scales + rotations", ext=cov)
            add(e, "covariances and scales", rotations=None, ext=cov)
            add(e, "covariances, no gradient output", scales=None, rotations=None, ext=dict(cov3D_precomp=_D))
            add(e, "neither covariances nor scales", scales=None, rotations=None)
            for bc in (100, 2048, 63, 64, 1024):
                add(e, "bin capacity %d" % bc, ext=dict(bin_capacity=bc))
            add(e, "bin capacity 100, one byte short", ext=dict(bin_capacity=100), ws=_need(lib, e, _spec(e)) - 1)
            both = dict(out_depth=_D, out_alpha=_D)
            add(e, "depth and alpha maps, one byte short", ext=both, ws=_need(lib, e, _spec(e, ext=both)) - 1)
            add(e, "depth and alpha maps, the plain size", ext=both, ws=_need(lib, e, _spec(e, opt=None)) - (1 if fwd else 0))
            add(e, "depth map misaligned, reserved / channels bad too", ext=dict(out_depth=_D + 1), opt=BAD_OPT.get(e))
        if _has_cam(e):
            need = lib.gsr_camera_grad_scratch_bytes(1)
            for k in CAM_PTRS[:3]:
                add(e, "camera %s" % k, cam={k: _D, "scratch": _D, "scratch_bytes": need})
                add(e, "camera %s misaligned" % k, cam={k: _D + 2, "scratch": _D, "scratch_bytes": need})
                add(e, "camera %s, scratch one byte short" % k, cam={k: _D, "scratch": _D, "scratch_bytes": need - 1})
                add(e, "camera %s, no scratch" % k, cam={k: _D, "scratch_bytes": need})
            cam = dict(dL_dviewmatrix=_D, dL_dprojmatrix=_D, dL_dcampos=_D, scratch=_D, scratch_bytes=need)
            add(e, "camera, scratch misaligned", cam=dict(cam, scratch=_D + 2))
            add(e, "no camera, scratch misaligned and short", cam=dict(scratch=_D + 2, scratch_bytes=1))
            short = dict(cam, scratch_bytes=need - 1)  # the short scratch wins over whatever else is invalid ...
            add(e, "short scratch, means3D NULL", cam=short, means3D=None)
            add(e, "short scratch, P negative", cam=short, P=-1)
            add(e, "short scratch, bad option", cam=short, opt=BAD_OPT.get(e), ext=dict(out_depth=_D + 2))
            add(e, "short scratch, camera output misaligned", cam=dict(short, dL_dcampos=_D + 2))  # ... except a misaligned camera output
            add(e, "short scratch for P = 257", P=257, cam=dict(cam, scratch_bytes=lib.gsr_camera_grad_scratch_bytes(257) - 1))
            add(e, "scratch of P = 256 for P = 257", P=257, cam=dict(cam, scratch_bytes=lib.gsr_camera_grad_scratch_bytes(256)))
    for cid, e, s in out:  # belt and braces: no workspace here is large enough for a launch (an invalid bin capacity sizes nothing: taken as 0)
        scanned = dict(s, P=max(s["P"], 0), W=max(s["W"], 0), H=max(s["H"], 0), cap=max(s["cap"], 0), ext=dict(s["ext"] or {}, bin_capacity=0))
        assert s["ws"] < max(_need(lib, e, s), _need(lib, e, scanned)), cid
    assert len({c[0] for c in out}) == len(out)
    return out


SIZE_TUPLES = ((1, 8, 8, 1, 0), (0, 17, 9, 0, 0), (30000, 256, 256, 1 << 20, 0), (30000, 256, 256, 1 << 20, 1024), (600000, 1024, 1024, 5 << 20, 1024))


def _sizes(lib):
    out = {}
    for P, W, H, cap, bcap in SIZE_TUPLES:
        key = "%d %dx%d cap %d bins %d" % (P, W, H, cap, bcap)
        out[key + " gsr_workspace_bytes"] = lib.gsr_workspace_bytes(P, W, H, cap)
        out[key + " gsr_workspace_bytes_forward_only"] = lib.gsr_workspace_bytes_forward_only(P, W, H, cap)
        out[key + " gsr_workspace_bytes_absgrad"] = lib.gsr_workspace_bytes_absgrad(P, W, H, cap, bcap)
        for fo in (0, 1):
            for name in ("ex", "depth_alpha", "contrib"):
                out["%s gsr_workspace_bytes_%s forward_only %d" % (key, name, fo)] = getattr(lib, "gsr_workspace_bytes_" + name)(P, W, H, cap, bcap, fo)
            for F in (3, 64):
                out["%s gsr_workspace_bytes_features F %d forward_only %d" % (key, F, fo)] = lib.gsr_workspace_bytes_features(P, W, H, cap, bcap, F, fo)
    return out


def _record(lib):
    return {"codes": {cid: _call(lib, e, s) for cid, e, s in _cases(lib)}, "sizes": _sizes(lib)}


def test_return_codes_are_the_recorded_ones():
    want = json.load(open(GOLDEN))["codes"]
    got = _record(_capi.lib())["codes"]
    assert list(got) == list(want)  # the same cases, in the same order
    assert {k: v for k, v in got.items() if v != want[k]} == {}
    assert set(want.values()) == {_capi.GPSGS_OK, _capi.GPSGS_E_INVALID, _capi.GPSGS_E_WORKSPACE}  # (nothing reached a launch)
    for e in BACKWARDS:
        assert got[e + ":empty view"] == _capi.GPSGS_OK
    assert len(want) > 900


def test_workspace_sizes_are_the_recorded_ones():
    want = json.load(open(GOLDEN))["sizes"]
    got = _sizes(_capi.lib())
    assert got == want and len(want) == 5 * (3 + 2 * 5)
    assert all(v > 0 and v % 256 == 0 for v in want.values())


def test_each_option_demands_exactly_what_its_query_reports():
    """One byte below the size the option's query reports: GPSGS_E_WORKSPACE.  At that size the call would launch, which this test must not do, so there an
    argument is invalid as well: GPSGS_E_INVALID, i.e. the size no longer decides."""
    lib = _capi.lib()
    g = (1, 8, 8, 1024, 0)
    maps, cam = dict(out_depth=_D, out_alpha=_D), dict(dL_dviewmatrix=_D, scratch=_D, scratch_bytes=lib.gsr_camera_grad_scratch_bytes(1))
    fo = lib.gsr_workspace_bytes_ex(*g, 1)
    options = [(e, {}, fo) for e in ("gsr_forward", "gsr_forward_notify", "gsr_forward_ex")]
    options += [("gsr_forward_ex", dict(ext=maps), lib.gsr_workspace_bytes_depth_alpha(*g, 1)), ("gsr_forward_features", {}, lib.gsr_workspace_bytes_features(*g, 3, 1)),
                ("gsr_forward_contrib", {}, lib.gsr_workspace_bytes_contrib(*g, 1)), ("gsr_forward_contrib", dict(ext=maps), lib.gsr_workspace_bytes_contrib(*g, 0))]
    options += [(e, {}, lib.gsr_workspace_bytes_ex(*g, 0)) for e in ("gsr_backward", "gsr_backward_ex", "gsr_backward_camera")]
    options += [("gsr_backward_ex", dict(ext=maps), lib.gsr_workspace_bytes_depth_alpha(*g, 0)), ("gsr_backward_camera", dict(cam=cam), lib.gsr_workspace_bytes_ex(*g, 0)),
                ("gsr_backward_features", {}, lib.gsr_workspace_bytes_features(*g, 3, 0)), ("gsr_backward_features", dict(ext=maps, cam=cam), lib.gsr_workspace_bytes_features(*g, 3, 0)),
                ("gsr_backward_features", dict(opt=dict(dL_dfeatures=None)), lib.gsr_workspace_bytes_ex(*g, 0)),
                ("gsr_backward_features", dict(opt=dict(dL_dfeatures=None), ext=maps), lib.gsr_workspace_bytes_depth_alpha(*g, 0)),
                ("gsr_backward_absgrad", {}, lib.gsr_workspace_bytes_absgrad(*g)), ("gsr_backward_absgrad", dict(ext=maps, cam=cam), lib.gsr_workspace_bytes_absgrad(*g))]
    assert lib.gsr_workspace_bytes_contrib(*g, 0) == lib.gsr_workspace_bytes_contrib(*g, 1) > lib.gsr_workspace_bytes_absgrad(*g) > lib.gsr_workspace_bytes_depth_alpha(*g, 0) > fo
    for entry, over, size in options:
        assert size > 0 and size == _need(lib, entry, _spec(entry, **over)), (entry, over)
        assert _call(lib, entry, _spec(entry, ws=size - 1, **over)) == _capi.GPSGS_E_WORKSPACE, (entry, over)
        assert _call(lib, entry, _spec(entry, ws=size, means3D=None, **over)) == _capi.GPSGS_E_INVALID, (entry, over)
    short = dict(cam, scratch_bytes=cam["scratch_bytes"] - 1)  # a short camera scratch: GPSGS_E_WORKSPACE whatever the workspace, ahead of any invalid argument
    assert _call(lib, "gsr_backward_camera", _spec("gsr_backward_camera", ws=lib.gsr_workspace_bytes_ex(*g, 0), cam=short, means3D=None)) == _capi.GPSGS_E_WORKSPACE


if __name__ == "__main__":
    recorded = _record(_capi.lib())
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=0)
        f.write("\n")
    print("recorded", _capi.LIB_PATH, "->", GOLDEN)
