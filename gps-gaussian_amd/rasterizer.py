"""Drop-in replacement for the `diff_gaussian_rasterization` Python module on MI355X.

Mirrors the interface the reference binds at /root/reference/gaussian_renderer/__init__.py:14,36-62:
`GaussianRasterizationSettings` (12-field NamedTuple, no `antialiasing`), `GaussianRasterizer(raster_settings)` whose
call returns the 2-tuple `(color[3,H,W], radii[P])`, and the autograd contract of upstream's `_RasterizeGaussians`
(gradients for means3D, means2D, colors_precomp, opacities, scales, rotations; None for the rest) -- SURVEY.md section 8b.
Opt-in antialiasing (the opacity-compensated 2D filter of the newer upstream interface, include/gpsgs.h GSR_FLAG_ANTIALIAS):
`antialiasing=True` on rasterize_gaussians / GaussianRasterizer.forward, or a settings object with a truthy `antialiasing` attribute.
Opt-in camera gradients (include/gpsgs.h gsr_backward_camera): `camera_grad=True` on rasterize_gaussians / GaussianRasterizer.forward makes
raster_settings.viewmatrix, projmatrix and campos differentiable; without it they are constants, as upstream.

All arithmetic happens in libgpsgs_hip.so (hand-written gfx950 kernels) through the C-ABI of include/gpsgs.h.
There is NO eager/CPU fallback: non-GPU tensors or a missing library raise.

Host-side design notes (MI355X-first, not a translation of upstream's C++ glue):
  * one workspace tensor per forward replaces upstream's three resizable byte buffers and travels to backward in ctx;
  * upstream blocks on a D2H copy of `num_rendered` in the middle of every forward to size its sort buffers.  Here the
    whole forward is enqueued against an instance capacity learnt from previous calls; the kernels record the R they
    needed + an overflow flag in the workspace header.  `GPSGS_CHECK=sync` (default) has the binning scan kernel store
    that header straight into pinned host memory (gsr_forward_notify) and spins on it: the host learns R ~40 us into the
    forward, while scatter / sort / compositing are still running, so the check costs no GPU idle time; on overflow it
    transparently re-runs with a larger capacity, so results are always exact.  `GPSGS_CHECK=deferred` never blocks:
    the header lands in pinned memory and is examined on the next call into this module; an overflow then raises
    (capacity grows for later calls).  `GPSGS_CHECK=none` never looks at the header at all: the call sequence is then a pure
    stream of kernel launches only, which is what a HIP graph capture (torch.cuda.graph) needs; the caller owns the
    capacity question (run the step once eagerly in sync mode first: the learnt capacity is reused), an overflowing view is
    simply not rendered (the workspace header says so).
  * one policy for every host that launches views (this module's forward, defer_capacity_checks(), the compiled path, session.RasterSession):
    `_plan` picks capacity, list form and flags for each attempt, `_settle` reads a notification into a `_Header` and learns from it,
    `_repair_loop` decides what an overflow means and re-runs the view.
"""
import ctypes as C
import math
import os
import sys
import threading
import time
from collections import namedtuple
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _capi
from ._ops import device_guard as _device_guard, ptr as _ptr


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


_extra_flags = 0  # bench.py sets GSR_FLAG_TIMING here to bracket every kernel with hipEvents


def set_stage_timing(on, stage=None):
    """Turn hipEvent bracketing of the kernels on/off for subsequent calls (read with _capi.timing_read()).
    stage: name from _capi.STAGES to bracket only that kernel (2 events per call instead of ~20)."""
    global _extra_flags
    if not on:
        _extra_flags = 0
    elif stage is None:
        _extra_flags = _capi.GSR_FLAG_TIMING
    else:
        _extra_flags = _capi.GSR_FLAG_TIMING | ((_capi.STAGES.index(stage) + 1) << 4)


# ---- capacity policy --------------------------------------------------------------------------------------------
_MIN_CAP = 1 << 16
_state = {}  # device index -> dict(ratio=instances per Gaussian seen so far, floor, pending=[(note, stream, P)]: deferred-mode checks, ...)
_lock = threading.Lock()  # the per-device capacity state and the pinned header rings may be used from several host threads


def _dev_state(dev):
    st = _state.get(dev.index)
    if st is None:
        with _lock:
            st = _state.setdefault(dev.index, dict(ratio=4.0, floor=_MIN_CAP, pending=[]))
    return st


def _capacity_for(st, P):
    # generous: 288 GB of HBM3E means 12 B/instance of slack is free; 2x the worst ratio seen, never below the floor
    return int(min(max(st["floor"], int(P * st["ratio"] * 2.0) + 4096), 0x7fffffff))


_DIRECT_CAP = 1024  # entries per bin of direct lists (GSR_DIRECT_MAX_CAP: one wave sorts a bin's list)


def _bin_capacity(st, W, H):
    """Per-bin capacity of DIRECT bin lists for the next view on this device, or 0 = scanned lists (include/gpsgs.h GsrViewExt.bin_capacity).
    Direct lists drop two dependent launches from the forward (scan -> scatter) but a bin holds at most `capacity` entries: they are used until
    this device sees bin lists longer than 768 entries (`big_bins`, _note_longest -- the untrained-heads regime, lists of 1,000-3,000), and for images
    of up to 65,536 bins (2048^2).  A view that turns out to need longer lists is reported like an overflow and repaired by _repair_loop with
    scanned lists.  GPSGS_LISTS=scanned / direct forces the form (direct: still subject to the size limits)."""
    m = os.environ.get("GPSGS_LISTS", "auto")
    if m not in ("auto", "scanned", "direct"):
        raise ValueError("GPSGS_LISTS must be 'auto', 'scanned' or 'direct'")
    if m == "scanned" or (m == "auto" and st.get("big_bins", False)):
        return 0
    key = ("direct_ok", W, H)
    ok = st.get(key)
    if ok is None:
        ok = st[key] = bool(_capi.lib().gsr_direct_lists_ok(W, H, _DIRECT_CAP))
    return _DIRECT_CAP if ok else 0


def _plan(st, P, W, H, mode, scanned_only):
    """One launch attempt of a view with P Gaussians (or a row range's estimate) -> (instance capacity, per-bin capacity, extra flags).
    scanned_only: this view has shown a list too long for direct bins (its repair run).  The large-list sort launch is left out
    (GSR_FLAG_NO_LARGE_SORT) as long as this device has seen no long list -- only where a repair loop exists (mode "sync": the module's sync
    mode, also inside defer_capacity_checks(), the compiled path and RasterSession), because a surprise is reported like an overflow.
    Deferred mode cannot re-run the view, so it always launches them (they return at once when the longest list is short: ADVICE r04)."""
    cap = _capacity_for(st, P)
    bin_cap = 0 if scanned_only else _bin_capacity(st, W, H)
    flags = _capi.GSR_FLAG_NO_LARGE_SORT if (mode == "sync" and P > 0 and not st.get("big_bins", False)) else 0
    return cap, bin_cap, flags


_DEFAULT_FAMILY = "tiles"


def _composite_flag():
    """GPSGS_COMPOSITE=valu: the compositing kernels that evaluate every (pixel, splat) exponent on the vector ALUs (gsr_composite.hip).
    GPSGS_COMPOSITE=tiles: the kernels that take the exponents from bf16 matrix-core tiles (gsr_composite_tiles.hip; exact split
    evaluation, same results within rounding)."""
    m = os.environ.get("GPSGS_COMPOSITE", _DEFAULT_FAMILY)
    if m not in ("valu", "tiles"):
        raise ValueError("GPSGS_COMPOSITE must be 'valu' or 'tiles'")
    return _capi.GSR_FLAG_COMPOSITE_TILES if m == "tiles" else 0


def _wave_priority_flag(st=None, stream=None, deterministic=False):
    """GSR_FLAG_WAVE_PRIORITY (include/gpsgs.h: hardware wave priorities in the tile compositing kernels; results unchanged) for a view that has
    the chip to itself.  GPSGS_WAVE_PRIORITY=0 / 1 forces it off / on; default (unset): on, unless this device saw rasteriser calls on MORE THAN ONE
    stream within the last 50 ms -- user code that spreads views over streams overlaps their kernels, where the scheme costs ~2 % of the
    aggregate rate instead of gaining 4 - 8 %.  deterministic (graph capture, GPSGS_CHECK=none): the wall-clock history is
    not consulted -- a captured graph, and a run that is meant to be reproducible launch for launch, must not pick a kernel variant from timing
    (ADVICE r05): on, unless the environment says otherwise."""
    env = os.environ.get("GPSGS_WAVE_PRIORITY")
    if env == "0":
        return 0
    if env is None and not deterministic and st is not None and stream is not None:
        now = time.perf_counter()
        with _lock:  # forwards may run from several host threads
            seen = st.setdefault("streams", {})
            seen[stream] = now
            if len(seen) > 1:
                for k in [k for k, t in seen.items() if now - t > 0.05]:
                    del seen[k]
            several = len(seen) > 1
        if several:
            return 0
    return _capi.GSR_FLAG_WAVE_PRIORITY


def _check_mode():
    m = os.environ.get("GPSGS_CHECK", "sync")
    if m not in ("sync", "deferred", "none"):
        raise ValueError("GPSGS_CHECK must be 'sync', 'deferred' or 'none'")
    return m


class _Header(NamedTuple):
    """What the host learns from a forward's header."""
    R: int         # (Gaussian, bin) instances the view needed
    overflow: int  # non-zero: nothing was rendered (capacity, a list too long for its direct bin, or a row range beyond its capacity)
    need: int      # the capacity it needed: max(R, gradient-record slots)
    longest: int   # longest bin list
    npts: int      # Gaussians of the view (a row range's count)


def _header(w32):
    """A notify slot's uint32[8] view (GsrHeader: u64 R, overflow, max_tile_count, num_busy_wgs, num_slots, num_points; word 7 = sequence) -> _Header."""
    w = w32.tolist()
    R = w[0] | w[1] << 32
    return _Header(R, w[2], max(R, w[5]), w[3], w[6])


def _learn(st, h, P):
    """Learn from a view's header (P: its Gaussian count): capacity ratio and floor (monotone maxima), the work-order hint, the list-form regime."""
    with _lock:  # read-modify-write of monotone maxima
        st["last_R"] = h.R
        if P > 0:
            st["ratio"] = max(st["ratio"], h.need / P)
            st["last_points"] = P
        st["floor"] = max(st["floor"], min(int(h.need * 1.25) + 4096, 0x7fffffff))
        st["longest"] = h.longest  # the next view's work-order hint (GsrViewExt.order_hint): longest bin list of this one
    _note_longest(st, h.longest)


def _note_longest(st, longest):
    """`big_bins` -- this device renders views with long bin lists (the untrained-heads regime): the large-list sort launches are issued and the lists are
    SCANNED, not direct.  Set by one list beyond 768 entries (three quarters of what one sorting wave / one direct bin holds); cleared again after eight
    views in a row whose longest list stayed below 512 (stage-2 training leaves the regime as the scales shrink: the fast path must come back)."""
    with _lock:
        if longest > 768:
            st["big_bins"], st["short_streak"] = True, 0
        elif longest <= 512 and st.get("big_bins", False):
            st["short_streak"] = st.get("short_streak", 0) + 1
            if st["short_streak"] >= 8:
                st["big_bins"], st["short_streak"] = False, 0
        else:
            st["short_streak"] = 0


def _settle(st, note, stream, P=None):
    """Wait for the header of a notify `note` (ring, slot, uint32[8] view, sequence) launched on `stream`, hand its slot back to the ring
    (also when the wait fails) and learn from it.  P: the view's Gaussian count, None = the header's (a row range).  -> _Header"""
    ring, slot, w32, seq = note
    try:
        _wait_notify(w32, seq, stream)
        h = _header(w32)
    finally:
        ring.release(slot)  # the host has seen the sequence word (or gave up): the slot may be reissued
    _learn(st, h, h.npts if P is None else P)
    return h


def _repair_loop(st, note, stream, P, rows, cap, bin_cap, relaunch):
    """The exact (sync-mode) capacity check of one view: settle its notification and, while the view overflowed, re-run it through
    relaunch(scanned_only) -> (note, cap, bin_cap) of the new attempt.  An overflow means, in this order: a row range (rows: P is its row
    capacity) holding more Gaussians than that -> raise; a list longer than the direct bins hold -> re-run with scanned lists (_learn has set
    big_bins); a capacity already at 2^31 - 1 -> raise; otherwise -> re-run with the capacity _learn has grown.  The in-flight kernels of a failed
    attempt exit at once on the overflow flag."""
    scanned_only = False
    while True:
        h = _settle(st, note, stream, None if rows else P)
        if not h.overflow:
            return
        if rows and h.npts > P:
            raise RuntimeError("gps_gaussian_amd: the row range holds %d Gaussians, more than the capacity of %d rows the view was sized for" % (h.npts, P))
        if bin_cap and h.longest > bin_cap:
            scanned_only = True
        elif cap >= 0x7fffffff:
            raise _too_many(h.R)
        note, cap, bin_cap = relaunch(scanned_only)


def _drain_pending(st, block=False):
    """Look at the capacity results of earlier GPSGS_CHECK=deferred forwards: the binning scan stores each one's header straight into a pinned slot
    ~40 us into the forward.  block: wait for those that have not arrived yet (else they stay pending)."""
    keep = []
    with _lock:  # the swap is atomic with respect to other threads' drains and appends (an autograd thread's backward drains too)
        pending, st["pending"] = st["pending"], []
    try:
        for i, ent in enumerate(pending):
            note, stream, P = ent
            if not block and int(note[2][7]) != note[3]:
                keep.append(ent)
                continue
            try:
                h = _settle(st, note, stream, P)
            except Exception:
                keep.extend(pending[i + 1:])  # the entries behind this one stay pending: their slots and capacity results are not lost
                raise
            if h.overflow:
                keep.extend(pending[i + 1:])  # (their slots are looked at -- and released -- by the next call)
                raise RuntimeError(
                    "gps_gaussian_amd: a previous rasteriser call (GPSGS_CHECK=deferred) was not rendered: it needed %d (Gaussian, bin) instances / "
                    "gradient slots -- more than the capacity of its workspace -- and its longest bin list was %d entries. The capacity has been raised; re-run, "
                    "or use GPSGS_CHECK=sync." % (h.need, h.longest))
    finally:
        with _lock:
            st["pending"] = keep + st["pending"]


class _HeaderRing:
    """Pinned 32-byte header slots the scan kernel writes directly (gsr_forward_notify), allocated in chunks (allocating pinned memory per call
    costs tens of us).  `acquire_notify()` / `release()` hand them out with IN-FLIGHT ACCOUNTING: a slot goes back to the free list only after the
    host has seen its sequence word, and when every slot is out (a batch of more forwards than slots inside one defer_capacity_checks(), nested
    callers, many threads) the ring GROWS by another pinned chunk instead of reissuing a slot that is still being polled."""

    def __init__(self, n=64):
        self.n = n
        self.chunks = []  # (uint32 [n,8] view: word 7 of a slot = sequence number, base address, the pinned tensor)
        self.free = []
        self.seq = 0
        self._grow()

    def acquire_notify(self):
        """-> (note = (ring, slot handle, uint32[8] view, sequence number the device will store in word 7), pointer to the slot)."""
        while True:
            with _lock:  # slot and sequence number are handed out together: two host threads never share either
                if self.free:
                    c, k = slot = self.free.pop()
                    seq = self.seq = self.seq % 0x7fffffff + 1  # never 0, never equal to what the slot holds from its previous use
                    a32, base, _ = self.chunks[c]
                    return (self, slot, a32[k], seq), C.c_void_p(base + 32 * k)
            self._grow()

    def _grow(self):
        buf = torch.zeros((self.n, 4), dtype=torch.int64).pin_memory()  # 32-byte header prefix per slot (allocates pinned memory: outside the lock)
        a32 = buf.numpy().view("uint32")  # same memory; plain numpy scalars are much cheaper to read than 0-d tensors
        with _lock:
            c = len(self.chunks)
            self.chunks.append((a32, buf.data_ptr(), buf))
            self.free.extend((c, k) for k in reversed(range(self.n)))

    def release(self, slot):
        with _lock:
            self.free.append(slot)

    def in_flight(self):
        with _lock:
            return len(self.chunks) * self.n - len(self.free)


def _wait_notify(w32, seq, cur_stream):
    """Spin until the device has stored `seq` (gsr_forward_notify): typically the preprocess + scan time, ~40 us."""
    n = 0
    while int(w32[7]) != seq:
        n += 1
        if n & 0x3ff == 0:  # ~every 100 us of spinning (the store normally lands within the first ~40 us)
            if cur_stream.query():  # the stream drained without the store: surface the device error
                if int(w32[7]) == seq:
                    break
                torch.cuda.synchronize()
                raise RuntimeError("gps_gaussian_amd: the rasteriser forward finished without publishing its header")
            if n & 0x3fff == 0:
                time.sleep(0)  # a very long wait (> ~1.5 ms: the stream is backed up): give the core to another thread of this rank


# ---- several forwards in flight (pts2render: one stream per sample of the batch) ---------------------------------------------------
_tls = threading.local()  # .deferred: list collecting the capacity checks of forwards this THREAD enqueued inside `defer_capacity_checks()`
# (per thread: the autograd engine runs backwards -- and recomputed forwards -- on its own threads, and multi-threaded hosts are supported)


def _deferred_list():
    return getattr(_tls, "deferred", None)


class defer_capacity_checks:
    """Context: sync-mode forwards enqueued inside it do not wait for their capacity notification one by one; all of them are checked
    (and, on overflow, re-rendered in place) when the context exits.  Lets a caller enqueue independent views on several streams back
    to back so that they run concurrently, with the same exactness guarantee as the blocking form.  Their images must not be consumed
    before the context has exited."""

    def __enter__(self):
        self.prev, _tls.deferred = _deferred_list(), []
        return self

    def __exit__(self, et, ev, tb):
        todo, _tls.deferred = _tls.deferred, self.prev
        # EVERY finish() runs, whatever the others do: each one waits for its header (capacity is learnt, the pinned slot returns to the ring,
        # an overflowed forward is repaired).  Stopping at the first failure would leak the remaining slots for good.  The first
        # error is re-raised afterwards -- unless an exception is already on its way out of the block, which then wins.
        first = None
        for finish in todo:
            try:
                finish()
            except Exception as e:  # noqa: BLE001
                if first is None:
                    first = e
        if et is None and first is not None:
            raise first
        return False


_rings = {}


def _ring(dev):
    """The pinned notify slots of a device."""
    r = _rings.get(dev.index)
    if r is None:
        ring = _HeaderRing()  # (allocates pinned memory: outside the lock)
        with _lock:
            r = _rings.setdefault(dev.index, ring)
    return r


def _prep(t, name, shape_tail, device):
    # fast path (what the reference's callers pass): fp32, contiguous, on the device, right shape -- used as is (only its address is needed)
    if (isinstance(t, torch.Tensor) and t.dtype is torch.float32 and t.device == device and t.is_contiguous()
            and (shape_tail is None or (t.dim() == 2 and tuple(t.shape[1:]) == shape_tail)) and (shape_tail != (4,) or t.data_ptr() % 16 == 0)):
        return t
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a tensor" % name)
    if t.device != device:
        raise RuntimeError("gps_gaussian_amd: %s is on %s but means3D is on %s (no CPU path exists)" % (name, t.device, device))
    if t.requires_grad:
        t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if not t.is_contiguous():
        t = t.contiguous()
    if shape_tail == (4,) and t.data_ptr() % 16:  # only the quaternions are read as float4 (row slices of packed buffers stay aligned)
        t = t.clone()
    if shape_tail is not None and (t.dim() < 1 or tuple(t.shape[1:]) != shape_tail):
        raise RuntimeError("%s must have dimensions (num_points, %s)" % (name, ", ".join(map(str, shape_tail))))
    return t


def _cam(t, n, device):
    # H1: in training the camera tensors arrive as pinned CPU tensors, in the test scripts as GPU tensors
    if t.device != device or t.dtype != torch.float32 or t.requires_grad or not t.is_contiguous():
        t = t.detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous()
    if t.numel() != n:
        raise RuntimeError("camera tensor must have %d elements" % n)
    return t


class _Rows:
    """A view whose Gaussians are a ROW RANGE of batch-wide arrays (GsrViewExt.row_range): `offsets` is an int32 device tensor, the view's
    rows are [offsets[index], offsets[index + 1]); `capacity` bounds their number (it sizes the workspace and the launches).  The host
    never learns the count: the kernels read the range from the device."""

    __slots__ = ("offsets", "index", "capacity", "ptr")

    def __init__(self, offsets, index, capacity):
        if offsets.dtype is not torch.int32 or not offsets.is_cuda or not offsets.is_contiguous() or offsets.numel() < index + 2:
            raise RuntimeError("gps_gaussian_amd: row offsets must be a contiguous int32 GPU tensor with index + 2 entries")
        self.offsets, self.index, self.capacity = offsets, int(index), int(capacity)
        self.ptr = offsets.data_ptr() + 4 * self.index


def _ext(rows, hint, appear=None, bin_cap=0, depth_alpha=None):
    """appear: None, or (shs, sh_degree, campos, cov3D_precomp, dL_dsh, dL_dcov3D) tensors / None -- the SH-colour and precomputed-covariance
    inputs (and, for the backward, their gradient arrays).  depth_alpha: None, or two [H, W] tensors / None -- the forward's depth and alpha
    outputs, or the backward's gradients of them (the two share their GsrViewExt slots)."""
    e = _capi.GsrViewExt()
    if depth_alpha is not None:
        e.out_depth, e.out_alpha = _ptr(depth_alpha[0]), _ptr(depth_alpha[1])
    e.row_range = rows.ptr if rows is not None else None
    e.order_hint = int(hint) & 0xffffffff
    e.bin_capacity = int(bin_cap)
    if appear is not None:
        shs, deg, campos, cov, d_sh, d_cov = appear
        if shs is not None:
            e.shs, e.sh_degree, e.sh_coeffs, e.campos = shs.data_ptr(), int(deg), int(shs.shape[1]), campos.data_ptr()
            e.dL_dsh = d_sh.data_ptr() if d_sh is not None else None
        if cov is not None:
            e.cov3D_precomp = cov.data_ptr()
            e.dL_dcov3D = d_cov.data_ptr() if d_cov is not None else None
    return e


def _antialias(rs, antialiasing):
    """Antialiasing for this view: the keyword, or a truthy `antialiasing` attribute of the settings (the newer upstream settings' field; the
    12-field GaussianRasterizationSettings has none).  Raises if the loaded library does not honour GSR_FLAG_ANTIALIAS -- an older one would
    silently render without the filter."""
    on = bool(antialiasing) or bool(getattr(rs, "antialiasing", False))
    if on and not (_capi.lib().gsr_supported_flags() & _capi.GSR_FLAG_ANTIALIAS):
        raise RuntimeError("gps_gaussian_amd: the loaded rasteriser library does not support antialiasing (GSR_FLAG_ANTIALIAS); rebuild it")
    return on


_ABSGRAD_FEATURES = "gps_gaussian_amd: return_absgrad cannot be combined with features in one call (the feature backward is another kernel family)"
_DISTORTION_ALONE = "gps_gaussian_amd: return_distortion cannot be combined with %s in one call (the C-ABI's entry points take one option struct each)"


# The opt-ins of one view, resolved once from the public keywords (_view_options) and carried as ONE value to the forward, its backward and whoever
# distributes the outputs.  A further opt-in is a further field.
#   depth_alpha   also the depth and alpha maps
#   antialiasing  GSR_FLAG_ANTIALIAS in the forward and the backward
#   camera_grad   viewmatrix / projmatrix / campos are differentiable inputs
#   features      a feature array is given: also the feature map
#   contrib       also the three per-Gaussian contribution statistics
#   absgrad       the backward also writes the absolute screen-space gradient ...
#   absgrad_sink  ... and then calls this with it, on the backward's stream (internal to pts2render); None = nobody to call
#   distortion    also the depth-distortion map (differentiable)
_ViewOptions = namedtuple("_ViewOptions", "depth_alpha antialiasing camera_grad features contrib absgrad absgrad_sink distortion",
                          defaults=(False,) * 6 + (None, False))
_DEFAULT_OPTIONS = _ViewOptions()


def _view_options(rs, depth_alpha=False, antialiasing=False, camera_grad=False, features=None, contrib=False, absgrad=False, distortion=False):
    """The public keywords (and the settings object, for its `antialiasing` attribute: _antialias) -> _ViewOptions.  absgrad: True, or the sink
    callable.  Features cannot be combined with the statistics or absgrad, the distortion map with none of the three: refused here, before anything
    is launched."""
    if distortion and (features is not None or contrib or absgrad):
        raise RuntimeError(_DISTORTION_ALONE % ("features" if features is not None else "return_contrib" if contrib else "return_absgrad"))
    if absgrad and features is not None:
        raise RuntimeError(_ABSGRAD_FEATURES)
    if contrib and features is not None:
        raise RuntimeError("gps_gaussian_amd: the contribution statistics cannot be combined with features in one call")
    return _ViewOptions(bool(depth_alpha), _antialias(rs, antialiasing), bool(camera_grad), features is not None, bool(contrib), bool(absgrad),
                        absgrad if callable(absgrad) else None, bool(distortion))


# What a view returns, in the documented order; None = not part of this call.  The autograd nodes (here and render_api._RenderBatch, whose batch-wide
# outputs have no radii) return _pack_outputs() of one and decode outputs, or incoming gradients, with _unpack_outputs().
_Outputs = namedtuple("_Outputs", "color radii depth alpha feat contrib_weight contrib_max contrib_pixels absgrad distortion", defaults=(None,) * 10)


def _pack_outputs(o):
    """_Outputs -> the tuple of the members that are present."""
    return tuple(t for t in o if t is not None)


def _unpack_outputs(opts, values, radii=True):
    """The inverse of _pack_outputs for a call made with `opts` (radii=False: a batch, which returns none): a tuple of outputs, or of the gradients
    autograd hands a backward for them (None for the non-differentiable ones) -> _Outputs."""
    # one entry per field of _Outputs, in its order: is the output part of this call?
    present = (True, radii, opts.depth_alpha, opts.depth_alpha, opts.features, opts.contrib, opts.contrib, opts.contrib, opts.absgrad, opts.distortion)
    it = iter(values)
    return _Outputs(*[next(it) if p else None for p in present])


def _non_differentiable(o):
    """The members of an _Outputs that carry no gradient: radii, the statistics, absgrad."""
    return tuple(t for t in (o.radii, o.contrib_weight, o.contrib_max, o.contrib_pixels, o.absgrad) if t is not None)


def _too_many(R):
    return RuntimeError("gps_gaussian_amd: this view needs %d (Gaussian, bin) instances, more than the 2^31 - 1 the workspace layout can address" % R)


def _features(features, N, dev):
    """features [P, F] -> fp32 contiguous on the device (as _prep does), 1 <= F <= GSR_MAX_FEATURES; raises before anything is launched."""
    if not isinstance(features, torch.Tensor):
        raise TypeError("features must be a tensor")
    if features.dim() != 2 or not 1 <= features.shape[1] <= _capi.GSR_MAX_FEATURES or features.shape[0] != N:
        raise RuntimeError("features must have dimensions (num_points, F) with 1 <= F <= %d" % _capi.GSR_MAX_FEATURES)
    return _prep(features, "features", (int(features.shape[1]),), dev)


def _out_tensor(given, shape, dtype, dev, bad, exact=False, missing=None, zero=False):
    """One output of a view: the caller's preallocated tensor after its checks -- dtype, device, contiguity and `shape` (exact: the very shape,
    otherwise its element count), any failure raises `bad` -- or, when none was given, a fresh one (zero: zero-filled), unless the view cannot do
    without the caller's (`missing`: the message to raise then)."""
    if given is None:
        if missing is not None:
            raise RuntimeError(missing)
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=dev)
    if (given.dtype is not dtype or given.device != dev or not given.is_contiguous()
            or (tuple(given.shape) != shape if exact else given.numel() != math.prod(shape))):
        raise RuntimeError(bad)
    return given


# What a forward leaves on its ctx (ctx.view) for its backward, beside the tensors of ctx.saved.
#   family       the backward must repeat the forward's per-pixel decisions: same kernel family
#   extra_flags  _extra_flags as the forward read it (the backward runs on an autograd thread)
#   rows         the view's _Rows, or None
#   absgrad_out  the absgrad tensor the backward overwrites, or None
#   ws_box       inside defer_capacity_checks(): [workspace, cap, bin_cap] of the latest attempt (an overflow repair replaces them), else None
_ViewState = namedtuple("_ViewState", "raster_settings cap bin_cap family extra_flags rows opts absgrad_out ws_box")


# The tensors a view's backward reads (ctx.saved); None where the other form of an input was given, and for `fea` without features.
# `tot`: the distortion map's per-pixel totals [2, H, W] (None without it).
_Saved = namedtuple("_Saved", "m3 col opa sca rot view proj bg radii ws sh cov campos fea tot", defaults=(None,))


def _workspace_bytes(lib, opts, fwd_only, feat_grad, F, dims):
    """Bytes of the workspace of a view with these options; dims = (P, W, H, instance capacity, per-bin capacity)."""
    if opts.contrib:  # the statistics need the slot prefix of the backward tail and the contribution tail (also for inference)
        return lib.gsr_workspace_bytes_contrib(*dims, fwd_only)
    if opts.features and feat_grad and not fwd_only:  # the per-slot feature sums need the feature tail
        return lib.gsr_workspace_bytes_features(*dims, F, fwd_only)
    if opts.absgrad and not fwd_only:  # the backward's absolute sums need the absgrad tail (with statistics: inside their larger tail)
        return lib.gsr_workspace_bytes_absgrad(*dims)
    # (the distortion map's dL/dz rides in the depth / alpha slot array: the same size, no tail of its own)
    return (lib.gsr_workspace_bytes_depth_alpha if opts.depth_alpha or opts.distortion else lib.gsr_workspace_bytes_ex)(*dims, fwd_only)


def _distort_struct(dmap, totals):
    """The GsrDistort of a forward (dmap: the map to write) or a backward (dmap: the map's gradient) with the view's totals plane."""
    d = _capi.GsrDistort()
    d.out_distort, d.totals = dmap.data_ptr(), totals.data_ptr()
    return d


def _forward_entry(cst, feat, dst=None):
    """-> (name of the forward entry point, the option struct it takes behind the common arguments)."""
    if dst is not None:
        return "gsr_forward_distort", (C.byref(dst),)
    if cst is not None:
        return "gsr_forward_contrib", (C.byref(cst),)
    if feat is not None:
        return "gsr_forward_features", (C.byref(feat),)
    return "gsr_forward_ex", ()


def _backward_entry(lib, P, dev, cam_out, feat, agrad, dst=None):
    """-> (name of the backward entry point, the arguments it takes behind the common ones, the camera scratch slab or None: the caller holds it until
    the call is enqueued).  The three entry points with camera outputs accept NULLs for them (and then need no scratch); the slab is one per view in
    flight (the stream-ordered allocator keeps it alive until this stream's kernels are done)."""
    if cam_out is None and feat is None and agrad is None and dst is None:
        return "gsr_backward_ex", (), None
    nbytes = lib.gsr_camera_grad_scratch_bytes(P) if cam_out is not None else 0
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if cam_out is not None else None
    cam = tuple(_ptr(t) for t in (cam_out if cam_out is not None else (None, None, None))) + (_ptr(scratch), nbytes)
    if feat is not None:
        return "gsr_backward_features", cam + (C.byref(feat),), scratch
    if agrad is not None:
        ab = _capi.GsrAbsGrad()
        ab.absgrad = agrad.data_ptr()
        return "gsr_backward_absgrad", cam + (C.byref(ab),), scratch
    if dst is not None:
        return "gsr_backward_distort", cam + (C.byref(dst),), scratch
    return "gsr_backward_camera", cam, scratch


_NO_OUTPUTS = {}
_BAD_OUTPUT = dict(  # what _forward_impl raises for a preallocated output it cannot use (and for one a row-range view needs but was not given)
    color="gps_gaussian_amd: out_color must be a contiguous fp32 [3, H, W] tensor on the inputs' device",
    maps="gps_gaussian_amd: out_depth / out_alpha must be contiguous fp32 [H, W] tensors on the inputs' device",
    distortion="gps_gaussian_amd: the distortion output must be a contiguous fp32 [H, W] tensor on the inputs' device",
    feat="gps_gaussian_amd: out_feat must be a contiguous fp32 [F, H, W] tensor on the inputs' device",
    contrib="gps_gaussian_amd: out_contrib must be contiguous [rows] tensors (fp32, fp32, int32) on the inputs' device",
    no_contrib="gps_gaussian_amd: a row-range view needs its batch-wide statistics arrays (out_contrib)",
    absgrad="gps_gaussian_amd: out_absgrad must be a contiguous fp32 [rows, 2] tensor on the inputs' device",
    no_absgrad="gps_gaussian_amd: a row-range view needs its batch-wide absgrad array (out_absgrad)",
    radii="gps_gaussian_amd: a row-range view needs radii_out: contiguous int32 [rows of the arrays] on the inputs' device")


def _forward_impl(ctx, means3D, colors_precomp, opacities, scales, rotations, raster_settings, needs_grad, opts=_DEFAULT_OPTIONS, out=None, rows=None,
                  shs=None, cov3D_precomp=None, features=None, feat_grad=True):
    """One view's forward through the C-ABI (capacity policy, early notification, overflow repair).  `ctx` is any attribute holder: the
    autograd ctx of _RasterizeGaussians, or a plain namespace when a caller drives several views itself (render_api._RenderBatch).
    Leaves on it: view (a _ViewState) and saved (a _Saved).
    shs [P, M, 3] (M <= 16, evaluated up to raster_settings.sh_degree towards raster_settings.campos) INSTEAD of colors_precomp;
    cov3D_precomp [P, 6] INSTEAD of scales + rotations.
    rows (a _Rows): the five inputs are batch-wide packed arrays, this view is the row range rows.offsets[rows.index : rows.index + 2] of
    them (read on the DEVICE).
    opts (a _ViewOptions, antialiasing already resolved by _view_options):
    depth_alpha: also render the depth map (sum z_i alpha_i T_i, unnormalised) and the alpha map (sum alpha_i T_i), background 0, with the VALU
    compositing family (include/gpsgs.h GsrViewExt.out_depth).  antialiasing: GSR_FLAG_ANTIALIAS, each splat's opacity scaled by
    sqrt(det(cov2D) / det(cov2D + 0.3 I)) (include/gpsgs.h), carried to the backward in ctx.  features [P, F] (1 <= F <= 64; opts.features): also
    render the feature map [F,H,W] = sum_i f_i alpha_i T_i, background 0, with the VALU family (include/gpsgs.h GsrFeatures); feat_grad=False: the
    backward will not form dL/dfeatures (the workspace gets no feature tail).  contrib: also the per-Gaussian contribution statistics
    (include/gpsgs.h GsrContrib), weight_sum, weight_max fp32 [P] and pixel_count int32 [P], with the VALU family; not with features.  absgrad: the
    view's backward will also write the absolute screen-space gradient (include/gpsgs.h GsrAbsGrad) -- the VALU family, a workspace with the absgrad
    tail, and a zero-filled fp32 [rows, 2] tensor left in ctx.view.absgrad_out; not with features.  distortion: also the depth-distortion map
    [1,H,W] = sum_i sum_j w_i w_j |z_i - z_j| (include/gpsgs.h GsrDistort), with the VALU family; its per-pixel totals [2,H,W] go to ctx.saved.tot for
    the backward; not with features, contrib or absgrad.
    out: optional dict of preallocated contiguous outputs -- color fp32 [3,H,W]; depth, alpha fp32 [H,W] (or [1,H,W]); feat fp32 [F,H,W];
    radii int32 [rows of the arrays]; contrib: the three statistics tensors; absgrad fp32 [rows, 2], ALREADY zeroed.  A row-range view's radii,
    contrib and absgrad are REQUIRED and batch-wide (its rows are written).
    -> _Outputs (None for what the options leave out)"""
    rs = raster_settings
    lib = _capi.lib()
    given = _NO_OUTPUTS if out is None else out
    if not means3D.is_cuda:
        raise RuntimeError("gps_gaussian_amd: rasteriser inputs must live on a GPU (no CPU fallback)")
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    dev = means3D.device
    N = means3D.shape[0]                      # rows of the arrays
    P = N if rows is None else rows.capacity  # Gaussians of the view, or their upper bound
    H, W = int(rs.image_height), int(rs.image_width)
    m3 = _prep(means3D, "means3D", (3,), dev)
    opa = _prep(opacities, "opacities", None, dev).reshape(-1)
    col = sca = rot = sh = cov = campos = None
    if shs is None:
        col = _prep(colors_precomp, "colors_precomp", (3,), dev)
    else:
        sh = _prep(shs, "shs", None, dev)
        deg = int(rs.sh_degree)
        if sh.dim() != 3 or sh.shape[2] != 3 or sh.shape[1] > 16 or not 0 <= deg <= 3 or (deg + 1) ** 2 > sh.shape[1]:
            raise RuntimeError("shs must have dimensions (num_points, M, 3) with (sh_degree + 1)^2 <= M <= 16 and sh_degree in 0..3")
        campos = _cam(rs.campos, 3, dev)
    if cov3D_precomp is None:
        sca = _prep(scales, "scales", (3,), dev)
        rot = _prep(rotations, "rotations", (4,), dev)
    else:
        cov = _prep(cov3D_precomp, "cov3D_precomp", (6,), dev)
    if not all(t is None or t.shape[0] == N for t in (col, opa, sca, rot, sh, cov)):
        raise RuntimeError("all per-Gaussian inputs must have num_points rows")
    appear = (sh, int(rs.sh_degree), campos, cov, None, None) if (sh is not None or cov is not None) else None
    fea = _features(features, N, dev) if opts.features else None
    F = int(fea.shape[1]) if fea is not None else 0
    view = _cam(rs.viewmatrix, 16, dev)
    proj = _cam(rs.projmatrix, 16, dev)
    bg = _cam(rs.bg, 3, dev)
    # the compositing family and, for a view rendered on its own (the GaussianRasterizer module: no row range), the wave-priority scheme --
    # it pays when the view's kernels have the chip to themselves; a batch spreads its views over several streams and leaves it off
    st = _dev_state(dev)
    mode = _check_mode()
    family = _composite_flag() | (_wave_priority_flag(st, torch._C._cuda_getCurrentRawStream(dev.index), deterministic=(mode == "none")) if rows is None else 0)
    if opts.depth_alpha or opts.features or opts.contrib or opts.absgrad or opts.distortion:
        family = 0  # the depth / alpha and feature maps, the statistics and absgrad are made by the VALU kernels (forward and backward must agree on it)
    extra = _extra_flags  # read ONCE per view and carried to its backward in ctx (the backward runs on an autograd thread)
    base_flags = (_capi.GSR_FLAG_DEBUG if rs.debug else 0) | extra | family | (_capi.GSR_FLAG_ANTIALIAS if opts.antialiasing else 0)
    if mode != "none" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("gps_gaussian_amd: the capacity check reads a header back on the host and cannot run under graph capture; "
                           "warm up eagerly, then capture with GPSGS_CHECK=none")
    with _device_guard(dev):
        if mode != "none":
            _drain_pending(st)
        cur_stream = torch.cuda.current_stream(dev)
        stream = cur_stream.cuda_stream
        f32, bad = torch.float32, _BAD_OUTPUT
        batch_wide = rows is not None  # a row-range view writes its rows of the caller's batch-wide radii / statistics / absgrad arrays
        color = _out_tensor(given.get("color"), (3, H, W), f32, dev, bad["color"], exact=True)
        depth = alpha = fmap = feat = cstats = cst = agrad = dist = tot = dst = None
        if opts.depth_alpha:
            depth = _out_tensor(given.get("depth"), (1, H, W), f32, dev, bad["maps"])
            alpha = _out_tensor(given.get("alpha"), (1, H, W), f32, dev, bad["maps"])
        if fea is not None:
            fmap = _out_tensor(given.get("feat"), (F, H, W), f32, dev, bad["feat"])
            feat = _capi.GsrFeatures()
            feat.channels, feat.features, feat.out_features = F, fea.data_ptr(), fmap.data_ptr()
        if opts.contrib:
            missing = bad["no_contrib"] if batch_wide else None
            cstats = tuple(_out_tensor(t, (N,), dt, dev, bad["contrib"], missing=missing)
                           for t, dt in zip(given.get("contrib") or (None, None, None), (f32, f32, torch.int32)))
            cst = _capi.GsrContrib()
            cst.weight_sum, cst.weight_max, cst.pixel_count = (t.data_ptr() for t in cstats)
        if opts.absgrad:
            missing = bad["no_absgrad"] if batch_wide else None
            agrad = _out_tensor(given.get("absgrad"), (N, 2), f32, dev, bad["absgrad"], exact=True, zero=True, missing=missing)
        if opts.distortion:  # (the totals are written by every attempt, the repair included, like the map)
            dist = _out_tensor(given.get("distortion"), (1, H, W), f32, dev, bad["distortion"])
            tot = torch.empty((2, H, W), dtype=f32, device=dev)
            dst = _distort_struct(dist, tot)
        # (only a row-range view takes the caller's radii array: it is batch-wide; a view on its own always gets a fresh one)
        radii = _out_tensor(given.get("radii") if batch_wide else None, (N,), torch.int32, dev, bad["radii"], missing=bad["radii"] if batch_wide else None)
        # inference (no input needs a gradient): skip the backward tail of the workspace (37 B per instance slot)
        fwd_only = 0 if needs_grad else 1
        # a row-range view's P is only a bound: the instance capacity follows the Gaussian counts seen so far on this device
        p_est = P if rows is None else min(P, int(st.get("last_points", P) * 1.25) + 4096)
        # the device publishes the header to pinned memory right after the binning scan: the host checks capacity while scatter / sort /
        # compositing are still running (no GPU idle time)
        ring = _ring(dev) if (mode != "none" and P > 0) else None
        box = [None, 0, 0]  # the workspace, capacity and per-bin capacity of the view's latest attempt
        what, opt_args = _forward_entry(cst, feat, dst)
        entry = getattr(lib, what)
        dmaps = (depth, alpha) if opts.depth_alpha else None

        def launch(cap, bin_cap, plan_flags):
            """Enqueue the whole forward (one _plan).  -> (notify note or None, cap, bin_cap)"""
            nbytes = _workspace_bytes(lib, opts, fwd_only, feat_grad, F, (P, W, H, cap, bin_cap))
            st["last_ws_bytes"] = nbytes  # reported by last_stats(): what one view in flight holds (forward-only workspaces are ~3x smaller)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            note, hdr_ptr = ring.acquire_notify() if ring is not None else (None, None)
            # (every attempt, the repair included, writes the maps) work order: longest lists first, relative to the longest list seen on this device
            ext = _ext(rows, st.get("longest", 0), appear, bin_cap, dmaps)
            # (every attempt, the repair included, writes the feature map and the statistics too)
            rc = entry(P, W, H, _ptr(m3), _ptr(col), _ptr(opa), _ptr(sca), _ptr(rot), float(rs.scale_modifier), float(rs.tanfovx),
                       float(rs.tanfovy), _ptr(view), _ptr(proj), _ptr(bg), _ptr(color), _ptr(radii), _ptr(ws), nbytes, cap,
                       base_flags | plan_flags, stream, hdr_ptr, note[3] if note is not None else 0, C.byref(ext), *opt_args)
            if rc != 0 and note is not None:
                ring.release(note[1])
            _capi.check(rc, what)
            box[:] = ws, cap, bin_cap
            return note, cap, bin_cap

        def relaunch(scanned_only):
            return launch(*_plan(st, p_est, W, H, mode, scanned_only))

        plan = _plan(st, p_est, W, H, mode, False)
        dump = os.environ.get("GPSGS_DUMP_INPUTS")  # debugging aid: the inputs of the LAST forward entered, as an .npz (synchronises)
        if dump and rows is None:
            import numpy as _np
            _np.savez(dump, means3D=m3.cpu().numpy(), opacities=opa.cpu().numpy(),
                      **{k: v.cpu().numpy() for k, v in (("colors", col), ("scales", sca), ("rotations", rot), ("shs", sh), ("cov3D_precomp", cov)) if v is not None},
                      view=view.cpu().numpy(), proj=proj.cpu().numpy(), bg=bg.cpu().numpy(), W=W, H=H,
                      tanfovx=float(rs.tanfovx), tanfovy=float(rs.tanfovy), scale_modifier=float(rs.scale_modifier), cap=plan[0], needs_grad=bool(needs_grad))
        note, cap, bin_cap = launch(*plan)
        ws_box = None
        if note is None:
            pass  # GPSGS_CHECK=none, or nothing to render
        elif _deferred_list() is not None:
            # checked when the enclosing defer_capacity_checks() exits (several views in flight); an overflow is repaired there, in place: same
            # output tensors, a larger workspace in ctx.view.ws_box
            def finish(note=note, cap=cap, bin_cap=bin_cap):
                with torch.cuda.stream(cur_stream):
                    _repair_loop(st, note, cur_stream, P, rows is not None, cap, bin_cap, relaunch)

            _deferred_list().append(finish)
            ws_box = box
        elif mode == "deferred":
            # never blocks: the notification (it lands ~40 us into this forward) is looked at by the next call on this device
            with _lock:
                st["pending"].append((note, cur_stream, P if rows is None else None))
        else:
            _repair_loop(st, note, cur_stream, P, rows is not None, cap, bin_cap, relaunch)
        ws, cap, bin_cap = box  # (inside defer_capacity_checks(): still the first attempt's, a repair replaces them in ctx.view.ws_box)
    ctx.view = _ViewState(rs, cap, bin_cap, family, extra, rows, opts, agrad, ws_box)
    ctx.saved = _Saved(m3, col, opa, sca, rot, view, proj, bg, radii, ws, sh, cov, campos, fea, tot)
    return _Outputs(color, radii, depth, alpha, fmap, *(cstats or (None, None, None)), agrad, dist)


def _map_grad(g):
    if g is None or (g.dtype is torch.float32 and g.is_contiguous() and not g.requires_grad):
        return g
    return g.detach().to(dtype=torch.float32).contiguous()


def _backward_impl(ctx, saved, grads, arena, color_grad=True, cam_out=None, feat_out=None):
    """One view's backward through the C-ABI.  color_grad=False: the caller does not need dL/dcolours (GSR_FLAG_NO_COLOR_GRAD: the tile
    family leaves the colour sums out; the returned colour gradient is zeros / not meaningful).  ctx: the holder the forward left its ctx.view on;
    saved: the _Saved the forward left in ctx.saved; arena: optional five preallocated gradient tensors (means3D, colours, opacities, scales,
    rotations) -- for a row-range view (ctx.view.rows) they are REQUIRED and batch-wide, the view's rows of them are written.
    -> (d_m3, d_m2, d_col, d_op, d_sc, d_rot, d_sh, d_cov); d_sh / d_cov are None unless the forward was given SH coefficients / precomputed
    covariances (d_sc, d_rot are then not meaningful).  grads (an _Outputs): the gradients of the image (color), of the depth and alpha maps of a
    depth_alpha forward ([H,W] or [1,H,W]), of the feature map ([F,H,W]) and of the distortion map ([H,W] or [1,H,W]: gsr_backward_distort with the
    forward's totals, saved.tot); None = zero, and all of them may be None.  cam_out: None, or three
    contiguous fp32 device tensors / None -- dL/d(viewmatrix [16], projmatrix [16], campos [3]) are WRITTEN into them (gsr_backward_camera: the
    per-Gaussian gradients keep their bits).  Features (the forward was given some: saved.fea): feat_out None, or a contiguous fp32 [rows, F] device
    tensor that dL/dfeatures is WRITTEN into (a row-range view: batch-wide, its rows written).  A forward with absgrad (ctx.view.absgrad_out): the
    view's rows of that tensor are OVERWRITTEN with the absolute screen-space gradient (gsr_backward_absgrad: every other gradient keeps its bits)."""
    v = ctx.view
    rs = v.raster_settings
    lib = _capi.lib()
    m3, col, opa, sca, rot, view, proj, bg, radii, ws, sh, cov, campos, fea, tot = saved
    cap, bin_cap, rows = v.cap, v.bin_cap, v.rows
    if v.ws_box is not None:  # forward ran inside defer_capacity_checks(): the workspace may have been replaced by the overflow repair
        ws, cap, bin_cap = v.ws_box
    dev = m3.device
    N = m3.shape[0]
    P = N if rows is None else rows.capacity
    H, W = int(rs.image_height), int(rs.image_width)
    g = grads.color  # H3: may arrive non-contiguous (or in another dtype); the common case -- fp32, contiguous -- is used as it is
    if g is None:  # only the depth / alpha maps took part in the loss
        g = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
    elif g.dtype is not torch.float32 or not g.is_contiguous() or g.requires_grad:
        g = g.detach().to(dtype=torch.float32).contiguous()
    agrad = v.absgrad_out
    feat = None
    if fea is not None:
        F = int(fea.shape[1])
        gf = _map_grad(grads.feat)
        if gf is not None and (gf.numel() != F * H * W or gf.device != dev):
            raise RuntimeError("gps_gaussian_amd: the feature map's gradient must have F x H x W elements on the inputs' device")
        if feat_out is not None and (feat_out.dtype is not torch.float32 or not feat_out.is_contiguous() or feat_out.device != dev
                                     or tuple(feat_out.shape) != (N, F)):
            raise RuntimeError("gps_gaussian_amd: the features' gradient array must be contiguous fp32 [rows, F] on the inputs' device")
        feat = _capi.GsrFeatures()
        feat.channels, feat.features, feat.dL_dfeaturemap, feat.dL_dfeatures = F, fea.data_ptr(), _ptr(gf), _ptr(feat_out)
    dmaps = None
    if grads.depth is not None or grads.alpha is not None:
        dmaps = (_map_grad(grads.depth), _map_grad(grads.alpha))
        if any(t is not None and (t.numel() != H * W or t.device != dev) for t in dmaps):
            raise RuntimeError("gps_gaussian_amd: depth / alpha gradients must have H x W elements on the inputs' device")
    dst = None
    if grads.distortion is not None and tot is not None:
        gd = _map_grad(grads.distortion)
        if gd.numel() != H * W or gd.device != dev:
            raise RuntimeError("gps_gaussian_amd: the distortion map's gradient must have H x W elements on the inputs' device")
        dst = _distort_struct(gd, tot)
    with _device_guard(dev):
        st = _dev_state(dev)
        if _check_mode() != "none":
            _drain_pending(st, block=(_check_mode() == "deferred"))
        stream = torch._C._cuda_getCurrentRawStream(dev.index)  # the raw handle: torch.cuda.current_stream() builds a Stream object (~3 us)
        if arena is not None and all(a.dtype == torch.float32 and a.is_contiguous() and a.device == dev and tuple(a.shape) == (N, c)
                                     for a, c in zip(arena[:5], (3, 3, 1, 3, 4))):
            d_m3, d_col, d_op, d_sc, d_rot = arena[:5]
            d_m2 = arena[5] if len(arena) > 5 else torch.empty((N, 3), dtype=torch.float32, device=dev)
        elif rows is not None:
            raise RuntimeError("gps_gaussian_amd: a row-range view needs its batch-wide gradient arrays")
        else:
            # one allocation, six contiguous gradient arrays carved out of it (quaternion gradient first: it is stored as float4)
            # (ONE split + six views: the slice-then-view form was twelve tensor operations, ~25 us of host time on the path between the capacity
            #  notification and the backward's launch -- the stretch that decides whether a slower host keeps the GPU fed, profiles/r05_host_timeline.md)
            buf = torch.empty((P * 17,), dtype=torch.float32, device=dev)
            b_rot, b_m3, b_m2, b_col, b_sc, b_op = buf.split_with_sizes((4 * P, 3 * P, 3 * P, 3 * P, 3 * P, P))
            d_rot, d_m3, d_m2 = b_rot.view(P, 4), b_m3.view(P, 3), b_m2.view(P, 3)
            d_col, d_sc, d_op = b_col.view(P, 3), b_sc.view(P, 3), b_op.view(P, 1)
        d_sh = torch.empty_like(sh) if sh is not None else None
        d_cov = torch.empty_like(cov) if cov is not None else None
        if cam_out is not None and not any(t is not None for t in cam_out):
            cam_out = None
        if P > 0:
            ext = _ext(rows, 0, (sh, int(rs.sh_degree), campos, cov, d_sh, d_cov) if (sh is not None or cov is not None) else None, bin_cap, dmaps)
            # one entry point for every combination of the opt-ins it serves: camera outputs may be NULL
            what, opt_args, _scratch = _backward_entry(lib, P, dev, cam_out, feat, agrad, dst)
            rc = getattr(lib, what)(P, W, H, _ptr(m3), _ptr(col), _ptr(opa), _ptr(sca), _ptr(rot), float(rs.scale_modifier),
                                    float(rs.tanfovx), float(rs.tanfovy), _ptr(view), _ptr(proj), _ptr(bg), _ptr(radii), _ptr(g),
                                    _ptr(d_m3), _ptr(d_m2), _ptr(d_col), _ptr(d_op), _ptr(d_sc), _ptr(d_rot), _ptr(ws),
                                    ws.numel(), cap, (_capi.GSR_FLAG_DEBUG if rs.debug else 0) | v.extra_flags | v.family
                                    | (0 if color_grad else _capi.GSR_FLAG_NO_COLOR_GRAD) | (_capi.GSR_FLAG_ANTIALIAS if v.opts.antialiasing else 0),
                                    stream, C.byref(ext), *opt_args)
            _capi.check(rc, what)
        elif cam_out is not None:
            for t in cam_out:
                if t is not None:
                    t.zero_()
    return d_m3, d_m2, d_col, d_op, d_sc, d_rot, d_sh, d_cov


# ---- the compiled host path (csrc/host_shim.cpp -> lib/_gpsgs_fast.so) -----------------------------------------------------------------------------
# The call shape the reference uses, in sync mode, goes through a C++ torch::autograd::Function that performs the same steps as _forward_impl /
# _backward_impl against the same C-ABI; everything else -- and every overflow -- takes the Python path below.  The capacity POLICY stays here.
_fast = None   # the module, or False when it is switched off / not built


def _fast_module():
    """lib/_gpsgs_fast.so, or False.  GPSGS_FAST=0 switches it off (the Python host path is then used for everything); on a machine where the
    library was built the module must load -- a missing or stale one is an ImportError, not a silent fallback."""
    global _fast
    if os.environ.get("GPSGS_FAST", "1") == "0":
        return False
    if _fast is None:
        import importlib.util
        path = os.path.join(os.path.dirname(_capi.LIB_PATH), "_gpsgs_fast.so")
        if not os.path.exists(path):
            raise ImportError("gps_gaussian_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` (or set GPSGS_FAST=0 "
                              "to use the Python host path)." % path)
        _capi.lib()  # libgpsgs_hip.so first: the extension links against it
        spec = importlib.util.spec_from_file_location("_gpsgs_fast", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if mod.abi_version() != _capi.lib().gpsgs_abi_version():
            raise ImportError("gps_gaussian_amd: %s was built against another ABI version" % path)
        _fast = mod
    return _fast


def _fast_forward(means3D, means2D, opacities, colors_precomp, scales, rotations, rs):
    """-> (color, radii) through the compiled host path, or None: not its call shape / mode, or the view overflowed (the caller then takes the
    Python path, which repairs it).  Policy decisions (capacity, list form, flags) are taken here, from the same per-device state."""
    F = _fast_module()
    env = os.environ
    if (not F or rs.debug or _extra_flags or _deferred_list() is not None or env.get("GPSGS_CHECK", "sync") != "sync"
            or env.get("GPSGS_DUMP_INPUTS") or not isinstance(means3D, torch.Tensor) or not means3D.is_cuda or torch.cuda.is_current_stream_capturing()):
        return None  # (under graph capture the Python path says what to do instead of spinning on a header that never arrives)
    dev = means3D.device
    st = _dev_state(dev)
    if st["pending"]:
        return None
    H, W = int(rs.image_height), int(rs.image_width)
    P = means3D.shape[0]
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    flags = _composite_flag() | _wave_priority_flag(st, stream)
    cap, bin_cap, plan_flags = _plan(st, P, W, H, "sync", False)
    out = F.rasterize(means3D, means2D, colors_precomp, opacities, scales, rotations, rs.bg, rs.viewmatrix, rs.projmatrix, H, W, float(rs.tanfovx),
                      float(rs.tanfovy), float(rs.scale_modifier), cap, bin_cap, st.get("longest", 0), flags | plan_flags)
    if out is None:
        return None
    R, overflow, longest, slots, npts, nbytes, _wait_us = F.last_header()
    st["last_ws_bytes"] = nbytes
    _learn(st, _Header(R, overflow, max(R, slots), longest, npts), P)
    if overflow:
        return None  # nothing was rendered (the kernels exit on the flag): the Python path re-renders with what was just learnt
    if _debug_keep_ws:
        _tls.last_ws = dict(ws=out[2], cap=cap, bin_cap=bin_cap)
    return out[0], out[1]


_debug_keep_ws = False  # tests: both host paths leave {ws, cap, bin_cap} of the last forward in _tls.last_ws (export_state needs them)


def _cam_grads(need, like, dev):
    """Device outputs for the camera gradients whose inputs need one: [16], [16], [3] fp32 (None where not needed)."""
    return tuple(torch.empty((n,), dtype=torch.float32, device=dev) if w and t is not None else None for w, t, n in zip(need, like, (16, 16, 3)))


def _cam_grad_as(g, t):
    """A camera gradient in the input's own shape, dtype and device (a pinned CPU camera tensor gets a CPU gradient)."""
    if g is None or t is None:
        return None
    return g.reshape(t.shape).to(device=t.device, dtype=t.dtype)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, grad_arena=None,
                opts=_DEFAULT_OPTIONS, viewmatrix=None, projmatrix=None, campos=None, features=None):
        # grad_arena (optional, internal to pts2render): five preallocated fp32 tensors [P,3],[P,3],[P,1],[P,3],[P,4] -- row slices
        # of batch-wide buffers -- that the backward writes dL/d(means3D, colours, opacities, scales, rotations) into instead of
        # fresh allocations, so that the batch's gradients arrive already concatenated (render_api._SplitRows)
        ctx.grad_arena = grad_arena
        # opts.camera_grad: viewmatrix / projmatrix / campos are the settings' own tensors, passed again as inputs so that autograd hands them their
        # gradients (the forward itself reads them from raster_settings, as always)
        ctx.cams = (viewmatrix, projmatrix, campos) if opts.camera_grad else None
        # stage 2 never differentiates the colours (they are input pixels, lib/GaussianRender.py:30-31): the backward then skips their sums
        ctx.color_grad = bool(ctx.needs_input_grad[3]) or sh is not None  # (dL/dsh is formed from dL/dcolour)
        # features [P, F]: dL/dfeatures is formed only when they require a gradient
        out = _forward_impl(ctx, means3D, colors_precomp, opacities, scales, rotations, raster_settings, any(ctx.needs_input_grad), opts,
                            shs=sh, cov3D_precomp=cov3Ds_precomp, features=features, feat_grad=opts.features and ctx.needs_input_grad[14])
        if _debug_keep_ws:
            _tls.last_ws = dict(ws=ctx.saved.ws, cap=ctx.view.cap, bin_cap=ctx.view.bin_cap)
        ctx.save_for_backward(*ctx.saved)
        ctx.saved = None
        # radii and the statistics are not differentiable; neither is absgrad: zero-filled here, overwritten in place by every backward
        ctx.mark_non_differentiable(*_non_differentiable(out))
        ctx.set_materialize_grads(False)  # otherwise autograd fills a zero int32 [P] "gradient" for radii on every backward
        return _pack_outputs(out)

    @staticmethod
    def backward(ctx, *grads):
        opts = ctx.view.opts
        g = _unpack_outputs(opts, grads)
        if g.color is None and g.depth is None and g.alpha is None and g.feat is None and g.distortion is None:  # no output took part in the loss
            return (None,) * len(ctx.needs_input_grad)
        saved = _Saved(*ctx.saved_tensors)
        cam_out = _cam_grads(ctx.needs_input_grad[11:14], ctx.cams, saved.m3.device) if opts.camera_grad else None
        d_feat = None
        if opts.features and ctx.needs_input_grad[14]:
            d_feat = torch.empty(tuple(saved.fea.shape), dtype=torch.float32, device=saved.fea.device)
        d_m3, d_m2, d_col, d_op, d_sc, d_rot, d_sh, d_cov = _backward_impl(ctx, saved, g, ctx.grad_arena, ctx.color_grad, cam_out, d_feat)
        if opts.absgrad_sink is not None:
            opts.absgrad_sink(ctx.view.absgrad_out)
        has_sh, has_cov = saved.sh is not None, saved.cov is not None
        d_cam = (None, None, None) if cam_out is None else tuple(_cam_grad_as(g, t) for g, t in zip(cam_out, ctx.cams))
        # (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, grad_arena, opts, viewmatrix, projmatrix,
        #  campos, features)
        return (d_m3, d_m2, d_sh, (d_col if ctx.color_grad and not has_sh else None), d_op, (None if has_cov else d_sc), (None if has_cov else d_rot),
                d_cov, None, None, None, *d_cam, d_feat)[:len(ctx.needs_input_grad)]  # (the default call passes the first ten only)


def _rasterize(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, grad_arena, opts, features):
    """The call into the autograd node.  Only tensors that may need a gradient are arguments of their own -- the three camera tensors (with
    opts.camera_grad) and the features; every other opt-in rides in `opts`.  The default call keeps the ten arguments it always had: with the
    fifteen-argument shape for it too, the benchmark's Python-host-path rate fell below the slowest of the parent's runs in two runs of three (2,553 and
    3,573 views/s against 3,858 .. 4,205), with this plain shape it did not (3,775 / 4,206 / 4,240); it is also the call the reference makes."""
    rs = raster_settings
    if opts == _DEFAULT_OPTIONS:
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, grad_arena)
    cams = tuple(t if isinstance(t, torch.Tensor) else None for t in (rs.viewmatrix, rs.projmatrix, rs.campos)) if opts.camera_grad else (None, None, None)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, grad_arena, opts, *cams,
                                     features)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, grad_arena=None,
                        return_depth_alpha=False, antialiasing=False, camera_grad=False, features=None, return_contrib=False, return_absgrad=False,
                        return_distortion=False):
    """-> (color [3,H,W], radii [P]); with return_depth_alpha=True (color, radii, depth [1,H,W], alpha [1,H,W]): the depth map sum_i z_i alpha_i T_i
    (view-space z, NOT normalised: divide by alpha for the expected depth) and the accumulated opacity sum_i alpha_i T_i, both with background 0
    and differentiable (include/gpsgs.h GsrViewExt.out_depth).  They are rendered by the VALU compositing kernels whatever GPSGS_COMPOSITE says.
    antialiasing=True (or a truthy raster_settings.antialiasing): the opacity-compensated 2D filter, include/gpsgs.h GSR_FLAG_ANTIALIAS.
    camera_grad=True: raster_settings.viewmatrix, projmatrix and campos become differentiable inputs -- each that requires a gradient gets
    dL/d(itself) in its own shape, dtype and device (include/gpsgs.h gsr_backward_camera; without the keyword they are constants, as upstream).
    features [P, F] (1 <= F <= 64, on means3D's device): also returns the feature map [F,H,W] = sum_i f_i alpha_i T_i, background 0, LAST --
    (color, radii, feat) or (color, radii, depth, alpha, feat) -- rendered by the VALU kernels with the image's blend weights, differentiable in
    the features and, through the weights, in the geometry (include/gpsgs.h GsrFeatures).
    return_contrib=True: also returns the per-Gaussian contribution statistics LAST -- contrib_weight (fp32 [P], the sum over pixels of the blend
    weight alpha T), contrib_max (fp32 [P], its maximum) and contrib_pixels (int32 [P], the pixels the Gaussian is blended into) -- from the image's
    own blend (the VALU kernels; zeros for culled Gaussians and for a view that overflowed unrepaired), not differentiable, bitwise reproducible
    (include/gpsgs.h GsrContrib).  Combines with everything above except features (RuntimeError before anything is launched).
    return_absgrad=True: also returns, LAST of all, absgrad (fp32 [P, 2]): the absolute screen-space gradient sum_p |dL_p/dmean2D_i| in the units of
    means2D.grad[:, :2] (AbsGS's homodirectional gradient, gsplat's absgrad; include/gpsgs.h GsrAbsGrad).  The tensor is zero-filled by the forward, not
    differentiable, and every backward through the node OVERWRITES it in place (it does not accumulate): read it after backward().  Zeros for culled
    Gaussians and for a view that overflowed unrepaired; bitwise reproducible; every other output and gradient keeps the bits of the call without it
    (VALU kernels).  Combines with everything above except features (RuntimeError before anything is launched).
    return_distortion=True: also returns, LAST, distortion (fp32 [1,H,W]): the depth-distortion map sum_i sum_j w_i w_j |z_i - z_j| over the splats
    blended into each pixel (w = alpha T; the distortion term of Mip-NeRF 360 / 2DGS, gsplat's distloss; include/gpsgs.h GsrDistort), in RAW
    view-space depth units, not normalised -- like the depth map -- with background 0.  Differentiable (opacities, means, scales, rotations and, with
    camera_grad, the camera); from the image's own blend (the VALU kernels), bitwise reproducible; every other output keeps its bits.  The depth and
    alpha maps are returned only if return_depth_alpha asks for them too.  Combines with return_depth_alpha, antialiasing, camera_grad, shs and
    cov3D_precomp; not with features, return_contrib or return_absgrad (RuntimeError before anything is launched)."""
    opts = _view_options(raster_settings, return_depth_alpha, antialiasing, camera_grad, features, return_contrib, return_absgrad, return_distortion)
    return _rasterize(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, grad_arena, opts, features)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings
        acc = sys.modules.get("gps_gaussian_amd.accelerate")  # present only when GPSGS_ACCELERATE is set (opt-in, accelerate.py)
        if acc is not None:
            acc.late_apply()                                  # a flag test once everything requested is rebound

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
                grad_arena=None, return_depth_alpha=False, antialiasing=False, camera_grad=False, features=None, return_contrib=False,
                return_absgrad=False, return_distortion=False):
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (
                (scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        opts = _view_options(self.raster_settings, return_depth_alpha, antialiasing, camera_grad, features, return_contrib, return_absgrad,
                             return_distortion)
        if opts == _DEFAULT_OPTIONS and shs is None and cov3D_precomp is None and grad_arena is None:
            # the reference's call shape (gaussian_renderer/__init__.py:54-62): the compiled host path, when it applies
            out = _fast_forward(means3D, means2D, opacities, colors_precomp, scales, rotations, self.raster_settings)
            if out is not None:
                return out
        # shs [P, M, 3] are evaluated up to raster_settings.sh_degree towards raster_settings.campos (upstream computeColorFromSH); cov3D_precomp
        # [P, 6] replaces scale + rotation.  The reference passes neither (gaussian_renderer/__init__.py:54-62) but constructs the settings
        # with sh_degree = 3 and campos (:46-47): both inputs are part of the module it imports.
        # return_depth_alpha=True: (color, radii, depth, alpha), see rasterize_gaussians; antialiasing and camera_grad: the Python host path (not
        # the compiled one)
        # features [P, F]: the feature map is appended to the outputs; return_contrib: the three statistics after it; return_absgrad: the absolute
        # screen-space gradient last of all, filled by the backward; return_distortion: the depth-distortion map, last (rasterize_gaussians)
        return _rasterize(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, self.raster_settings, grad_arena, opts,
                          features)


    def markVisible(self, positions):
        """Upstream GaussianRasterizer.markVisible: boolean [P] mask of the points that pass the frustum test of the preprocess -- view-space
        z > 0.2, the only test upstream's in_frustum() applies (the reference never calls it; part of the class it imports,
        /root/reference/gaussian_renderer/__init__.py:14).  Not differentiable, like upstream (torch.no_grad)."""
        rs = self.raster_settings
        if not isinstance(positions, torch.Tensor) or not positions.is_cuda:
            raise RuntimeError("gps_gaussian_amd: markVisible needs a GPU tensor of positions (no CPU fallback)")
        if positions.dim() != 2 or positions.shape[1] != 3:
            raise RuntimeError("positions must have dimensions (num_points, 3)")
        with torch.no_grad():
            dev = positions.device
            pos = _prep(positions, "positions", (3,), dev)
            view, proj = _cam(rs.viewmatrix, 16, dev), _cam(rs.projmatrix, 16, dev)
            present = torch.empty((pos.shape[0],), dtype=torch.bool, device=dev)
            with _device_guard(dev):
                rc = _capi.lib().gsr_mark_visible(pos.shape[0], _ptr(pos), _ptr(view), _ptr(proj), _ptr(present), torch._C._cuda_getCurrentRawStream(dev.index))
            _capi.check(rc, "gsr_mark_visible")
        return present


def last_stats(device=None):
    """Capacity-policy state (instances-per-Gaussian ratio seen, capacity floor, bytes of the last workspace = what one view in flight holds)
    for diagnostics."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return dict(_dev_state(dev), pending=len(_dev_state(dev)["pending"]))


def export_state(ws, P, W, H, cap, bin_cap=0):
    """Debug/parity helper: unpack a forward's workspace into tensors: depth, xy, conic_opacity, rect (the 8x8-BIN rect
    bx0,by0,bx1,by1 each Gaussian is listed in), ranges [bx*by, 2] (per-bin list range), point_list, final_T, n_contrib.
    bin_cap: the per-bin capacity the forward used (ctx.view.bin_cap; 0 = scanned lists) -- with direct lists point_list holds every bin's segment
    (bins x bin_cap entries, indexed by `ranges`)."""
    lib = _capi.lib()
    dev = ws.device
    hdr = _header(ws[:32].cpu().numpy().view("uint32"))
    R = hdr.R
    bx, by = ((W + 7) // 8 + 3) // 4 * 4, (H + 7) // 8   # padded bin grid (gsr_common.h)
    out = dict(
        depth=torch.empty(P, device=dev), xy=torch.empty(P, 2, device=dev), conic_opacity=torch.empty(P, 4, device=dev),
        rect=torch.empty(P, 4, dtype=torch.int32, device=dev), ranges=torch.empty(bx * by, 2, dtype=torch.int64, device=dev),
        point_list=torch.empty(max(bx * by * bin_cap if bin_cap else cap, 1), dtype=torch.int32, device=dev), final_T=torch.empty(H, W, device=dev),
        n_contrib=torch.empty(H, W, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        rc = lib.gsr_export_state(_ptr(ws), P, W, H, cap, int(bin_cap), _ptr(out["depth"]), _ptr(out["xy"]), _ptr(out["conic_opacity"]),
                                  _ptr(out["rect"]), _ptr(out["ranges"]), _ptr(out["point_list"]), _ptr(out["final_T"]),
                                  _ptr(out["n_contrib"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _capi.check(rc, "gsr_export_state")
    torch.cuda.synchronize(dev)
    if not bin_cap:
        out["point_list"] = out["point_list"][:R]
    out["num_rendered"] = R
    out["bx"], out["by"] = bx, by
    out["overflow"] = hdr.overflow
    return out
