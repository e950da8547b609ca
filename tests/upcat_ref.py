"""What the decoder-glue tests share (test_upcat_ref.py on the CPU, test_gpu_upcat.py on the GPU): the case table, the seeded inputs, an fp64
restatement of the op -- out = cat([bilinear 2x upsample of a, *skips]) and da, the gradient of a -- with its error bounds, and the single-error
mutants of that restatement.  NumPy only.

The restatement is one matrix per axis: U [2n, n] with
    U[2i, max(i-1, 0)] += 0.25   U[2i, i] += 0.75          U[2i+1, i] += 0.75   U[2i+1, min(i+1, n-1)] += 0.25
so up(a) = Uy a Ux^T and da = Uy^T dout[:, :Ca] Ux (the clamped taps fold onto the border element by the +=).  The bounds are the same products
over absolute values, times k u with u = 2^-24: bound = k u sum_i w_i |a_i|, element by element (k: test_gpu_upcat.py derives it from the evaluation
order csrc/upcat.hip states; K_FWD = 2, K_BWD = 4)."""
import numpy as np

U32 = 2.0 ** -24
K_FWD, K_BWD = 2, 4

FORWARD_MUTANTS = ("weights_swapped", "low_clamp_missing", "high_clamp_off_by_one", "even_odd_exchanged", "skip_offset_off_by_one", "skips_reversed")
BACKWARD_MUTANTS = ("weights_swapped", "low_clamp_missing", "high_clamp_off_by_one", "even_odd_exchanged", "da_missing_folded_tap")


def cases(TH, TW):
    """name -> (N, Ca, h, w, skip channels).  TH x TW is the forward's output tile (uc_tile); an output axis is even, so the sizes that sit on a tile
    edge are TH - 2, TH + 2, 2 TH + 2 rows and TW - 2, TW + 2, 2 TW + 2 columns (w odd: the 4-byte path) and TW - 4, TW + 4, 2 TW + 4 columns (w
    even: the 16-byte path).  Two of them carry a skip longer than one copy workgroup's 4096 elements."""
    h2, w2 = TH // 2, TW // 2
    return {
        "1x1": (1, 1, 1, 1, ()),
        "1x5": (2, 3, 1, 5, (1,)),
        "5x1": (2, 3, 5, 1, (3, 1)),
        "3x3-odd-w": (1, 2, 3, 3, (2,)),
        "4x6-three-skips": (2, 4, 4, 6, (1, 3, 2)),
        "rows-below-tile": (1, 2, h2 - 1, 6, (1,)),
        "rows-above-tile": (1, 2, h2 + 1, 66, (2,)),
        "rows-above-two-tiles": (1, 2, 2 * h2 + 1, 33, (3,)),
        "cols-below-tile": (1, 2, 3, w2 - 1, ()),
        "cols-above-tile": (1, 2, 3, w2 + 1, (1,)),
        "cols-above-two-tiles": (1, 2, 2, 2 * w2 + 1, ()),
        "cols-below-tile-vec": (1, 2, 3, w2 - 2, (1,)),
        "cols-above-tile-vec": (1, 2, 3, w2 + 2, ()),
        "cols-above-two-tiles-vec": (1, 2, 2, 2 * w2 + 2, (1,)),
        "9x10-no-skips": (2, 5, 9, 10, ()),
        "reference-shaped": (2, 48, 16, 16, (3, 1)),
    }


def make_case(name, TH, TW, integers=False):
    """The seeded inputs of a case: a, skips, dout (fp32).  integers: whole numbers in [-8, 8], on which the op is exact."""
    N, Ca, h, w, sk = cases(TH, TW)[name]
    rng = np.random.default_rng(sorted(cases(TH, TW)).index(name) * 2 + int(integers))
    new = (lambda *s: rng.integers(-8, 9, size=s).astype(np.float32)) if integers else (lambda *s: rng.standard_normal(s).astype(np.float32))
    return dict(a=new(N, Ca, h, w), skips=[new(N, c, 2 * h, 2 * w) for c in sk], dout=new(N, Ca + sum(sk), 2 * h, 2 * w))


def taps(n, mutant=None, fold=True):
    """U [2n, n] in fp64.  fold=False: the clamped taps are dropped instead of folded onto the border element (the backward's mutant)."""
    near, far = (0.25, 0.75) if mutant == "weights_swapped" else (0.75, 0.25)
    U = np.zeros((2 * n, n))
    for i in range(n):
        lo, hi = i - 1, i + 1
        even, odd = (2 * i + 1, 2 * i) if mutant == "even_odd_exchanged" else (2 * i, 2 * i + 1)
        U[even, i] += near
        U[odd, i] += near
        if lo >= 0:
            U[even, lo] += far
        elif mutant != "low_clamp_missing" and fold:
            U[even, 0] += far
        if hi <= n - 1:
            U[odd, hi] += far
        elif fold:
            U[odd, max(n - 2, 0) if mutant == "high_clamp_off_by_one" else n - 1] += far
    return U


def forward(a, skips, mutant=None):
    """out in fp64."""
    N, Ca, h, w = a.shape
    up = np.einsum("yi,ncij,xj->ncyx", taps(h, mutant), a.astype(np.float64), taps(w, mutant))
    sk = [s.astype(np.float64) for s in (skips[::-1] if mutant == "skips_reversed" else skips)]
    out = np.concatenate([up] + sk, axis=1)
    if mutant == "skip_offset_off_by_one" and sk:     # the skips land one channel early; the last channel is never written
        out[:, Ca - 1:-1] = out[:, Ca:].copy()
        out[:, -1] = 0.0
    return out


def forward_bound(a):
    """K_FWD u sum_i w_i |a_i| for the upsampled channels."""
    N, Ca, h, w = a.shape
    return K_FWD * U32 * np.einsum("yi,ncij,xj->ncyx", taps(h), np.abs(a.astype(np.float64)), taps(w))


def backward(dout, Ca, mutant=None):
    """da in fp64."""
    h, w = dout.shape[2] // 2, dout.shape[3] // 2
    fold = mutant != "da_missing_folded_tap"
    return np.einsum("yi,ncyx,xj->ncij", taps(h, mutant, fold), dout[:, :Ca].astype(np.float64), taps(w, mutant, fold))


def backward_bound(dout, Ca):
    h, w = dout.shape[2] // 2, dout.shape[3] // 2
    return K_BWD * U32 * np.einsum("yi,ncyx,xj->ncij", taps(h), np.abs(dout[:, :Ca].astype(np.float64)), taps(w))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is zero the values must be equal (else inf)."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0
