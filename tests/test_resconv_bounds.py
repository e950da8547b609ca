"""CPU: the bounds of test_gpu_resconv.py (resconv_cases.bounds) are not vacuous.  For the inputs of three of its cases, a correct fp32 restatement
of the convolution and its gradients (torch's CPU kernels) stays inside every bound, and the same restatement with ONE error leaves the bound of the
key the error touches (error / bound > 1): the last input channel dropped, one tap dropped, the taps not flipped in dx, the last pixel tile left out
of dw, the bias left out."""
import pytest
import torch
import torch.nn.functional as F

import gps_gaussian_amd

import convop_run as R
import resconv_cases as K

CASES = ["tile_2T+1_T-1", "ragged_37x41", "pair_192_96"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    gps_gaussian_amd.build()      # the case table asks the library for its tile and partition counts


def _restate(c, error=None):
    """y, dx, dw, db in fp32 from the case's fp32 inputs, written out from the definition: dx as the convolution of dy with the flipped, transposed
    weight; dw and db from autograd over a dy that the error may have cut."""
    x, w, b, dy = c["x"], c["w"], c["b"], c["dy"]
    xf, wf, bf = x, w, b
    if error == "last_input_channel":
        xf, wf = x[:, :-1], w[:, :-1]
    elif error == "one_tap":
        wf = w.clone()
        wf[:, :, 2, 2] = 0.0
    elif error == "bias":
        bf = None
    y = F.conv2d(xf, wf, bf, padding=1)
    wt = w.transpose(0, 1)
    dx = F.conv2d(dy, wt if error == "taps_not_flipped" else wt.flip(2, 3), padding=1)
    g = dy
    if error == "last_pixel_tile":          # the last tile of the weight gradient's walk: the last sample's bottom-right 4 x 32 tile
        H, W = dy.shape[2:]
        g = dy.clone()
        g[-1, :, (H - 1) // K.WTILE[0] * K.WTILE[0]:, (W - 1) // K.WTILE[1] * K.WTILE[1]:] = 0.0
    wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    F.conv2d(x, wl, bl, padding=1).backward(g)
    return dict(y=y, dx=dx, dw=wl.grad, db=bl.grad)


def _ratios(c, got):
    return {k: R.ratio(got[k], c["ref"][k], c["bounds"][k]) for k in R.KEYS}


@pytest.mark.parametrize("name", CASES)
def test_the_correct_restatement_is_inside_every_bound(name):
    c = K.case(name)
    r = _ratios(c, _restate(c))
    R.emit(dict(test="bounds", case=name, error=None, ratios=r))
    assert all(0.0 < v <= 1.0 for v in r.values()), r       # inside, and not by being exact: fp32 rounds


@pytest.mark.parametrize("error,keys", [("last_input_channel", ("y",)), ("one_tap", ("y",)), ("taps_not_flipped", ("dx",)),
                                        ("last_pixel_tile", ("dw", "db")), ("bias", ("y",))])
@pytest.mark.parametrize("name", CASES)
def test_one_error_leaves_the_bound(name, error, keys):
    c = K.case(name)
    r = _ratios(c, _restate(c, error))
    R.emit(dict(test="bounds", case=name, error=error, ratios=r))
    for k in keys:
        assert r[k] > 1.0, (k, r[k])
    for k in set(R.KEYS) - set(keys):
        assert r[k] <= 1.0, (k, r[k])                         # and the error touches nothing else
