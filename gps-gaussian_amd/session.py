"""RasterSession -- a torch-autograd-free host for the rasteriser C-ABI (include/gpsgs.h), for callers that drive forward and
backward themselves (inference servers, C++/other-language hosts mirror it 1:1 -- tests/capi_host/capi_host_smoke.cpp -- and
bench.py's headline step).

What it is NOT: a different code path.  It enqueues exactly the kernels `rasterizer._RasterizeGaussians` enqueues, through the same
two C-ABI entry points (gsr_forward_notify, gsr_backward), with the same exact capacity policy (the binning scan publishes the
instance count to pinned host memory; an overflow is repaired by a transparent re-run).  What it leaves out is what PyTorch adds
around them per call: the autograd Function / engine round trip (~120 us per forward+backward on an idle MI355X host, measured
round 3; tools/host_time.py measures the module paths today), tensor allocations (outputs, workspace and gradient buffers are allocated once per (P, W, H)) and
argument normalisation.  Host cost per forward+backward: two ctypes calls (~35 us, almost all of it the HIP launches themselves).

Semantics follow the reference call at /root/reference/gaussian_renderer/__init__.py:36-62 (precomputed colours, scales + rotations).
"""
import ctypes as C

import torch

from . import _capi
from . import rasterizer as RZ


class RasterSession:
    def __init__(self, P, width, height, device, training=True, wave_priority=True, antialiasing=False):
        self.P, self.W, self.H = int(P), int(width), int(height)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("gps_gaussian_amd: RasterSession needs a GPU device (no CPU path exists)")
        self.training = bool(training)
        # GSR_FLAG_WAVE_PRIORITY (include/gpsgs.h): on for a session that renders on its own; a caller that keeps several sessions in
        # flight on different streams passes False (the kernels of different views then share the SIMDs and the scheme costs ~2 %)
        self.wave_priority = bool(wave_priority)
        self.lib = _capi.lib()
        # antialiasing: every forward and backward of the session carries GSR_FLAG_ANTIALIAS (the opacity-compensated 2D filter, include/gpsgs.h)
        self.aa_flag = _capi.GSR_FLAG_ANTIALIAS if RZ._antialias(None, antialiasing) else 0
        d, f32 = self.dev, torch.float32
        self.color = torch.empty((3, self.H, self.W), dtype=f32, device=d)
        self.radii = torch.empty((self.P,), dtype=torch.int32, device=d)
        self.ws, self.cap, self.nbytes = None, 0, 0
        self.allocations = 0  # workspace (re)allocations so far: 1 in steady state
        self._in, self._pending, self._cur = None, None, None
        self._ws_streams = []  # streams that have launched on the current workspace (see _ensure_ws)
        if self.training:
            # one buffer, six contiguous gradient arrays carved out of it
            P_ = max(self.P, 1)
            self._gbuf = torch.empty((P_ * 17 + 64,), dtype=f32, device=d)
            o, self.grads = 0, {}
            for name, c in (("rotations", 4), ("means3D", 3), ("means2D", 3), ("colors", 3), ("scales", 3), ("opacities", 1)):
                o = (o + 3) // 4 * 4  # 16-byte alignment (the quaternion gradient is stored as float4)
                self.grads[name] = self._gbuf[o:o + self.P * c].view(self.P, c)
                o += P_ * c
        self.bin_cap = 0  # per-bin capacity of the current workspace's lists (0 = scanned lists; rasterizer._bin_capacity)

    def _ensure_ws(self, cap, stream, bin_cap=0):
        """The workspace for `cap` instances, allocated on `stream` -- the stream its kernels are launched on.  (allocated under PyTorch's
        ambient current stream, the block belonged to THAT stream's pool while its kernels ran on `stream`; on replacement it went straight back to the
        pool and a later ambient-stream allocation could reuse it under the in-flight forward / backward.)  A replaced workspace is handed back with
        record_stream() for every stream the session ever launched on it, so the allocator waits for those kernels before reusing the block."""
        if self.ws is None or cap != self.cap or bin_cap != self.bin_cap:
            old = self.ws
            if old is not None:
                for st in self._ws_streams:
                    old.record_stream(st)
            self.nbytes = self.lib.gsr_workspace_bytes_ex(self.P, self.W, self.H, cap, bin_cap, 0 if self.training else 1)
            self.bin_cap = bin_cap
            with torch.cuda.stream(stream):
                self.ws = torch.empty((self.nbytes,), dtype=torch.uint8, device=self.dev)
            self._ws_streams = [stream]
            self.cap = cap
            self.allocations += 1
        elif not any(st is stream or st == stream for st in self._ws_streams):
            self._ws_streams.append(stream)

    @staticmethod
    def _chk(t, n, name):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != n:
            raise RuntimeError("gps_gaussian_amd: RasterSession expects %s as a contiguous fp32 GPU tensor of %d elements" % (name, n))
        return t.data_ptr()

    def forward(self, means3D, colors, opacities, scales, rotations, viewmatrix, projmatrix, bg, tanfovx, tanfovy, scale_modifier=1.0, stream=None):
        """-> (color[3,H,W], radii[P]) (the session's own buffers: valid until the next forward).  Enqueues on `stream` (a
        torch.cuda.Stream), default: PyTorch's current stream."""
        self.forward_begin(means3D, colors, opacities, scales, rotations, viewmatrix, projmatrix, bg, tanfovx, tanfovy, scale_modifier, stream)
        return self.forward_end()

    def forward_begin(self, means3D, colors, opacities, scales, rotations, viewmatrix, projmatrix, bg, tanfovx, tanfovy, scale_modifier=1.0, stream=None):
        """First half of forward(): enqueue the forward kernels and return at once.  forward_end() then waits for the capacity
        notification (and repairs an overflow).  Several sessions on several streams can so be started back to back -- independent views
        rendered concurrently -- before the host waits for any of them.  stream: the torch.cuda.Stream to enqueue on (the session only
        hands its raw handle to the C-ABI and owns all its buffers, so PyTorch's current stream need not be switched: ~8 us of host time per
        `with torch.cuda.stream(...)` saved, three times per view); default: the current stream.  The INPUTS (and, for backward(), dL_dpix)
        must already be ordered against that stream by the caller -- the session never inserts a wait; its own workspace is allocated on, and
        tied to, the streams it launches on."""
        P = self.P
        ptrs = (self._chk(means3D, 3 * P, "means3D"), self._chk(colors, 3 * P, "colors"), self._chk(opacities, P, "opacities"),
                self._chk(scales, 3 * P, "scales"), self._chk(rotations, 4 * P, "rotations"))
        cam = (self._chk(viewmatrix, 16, "viewmatrix"), self._chk(projmatrix, 16, "projmatrix"), self._chk(bg, 3, "bg"))
        fl = (float(scale_modifier), float(tanfovx), float(tanfovy))
        family = RZ._composite_flag() | (RZ._wave_priority_flag() if self.wave_priority else 0)
        self._in = (ptrs, fl, cam, family, (means3D, colors, opacities, scales, rotations, viewmatrix, projmatrix, bg))  # keeps the inputs alive
        self._cur = stream if stream is not None else torch.cuda.current_stream(self.dev)
        cap, bin_cap, plan_flags = self._plan(P == 0)  # (an empty view has no lists)
        self._pending = self._enqueue(max(self.cap, cap), bin_cap, plan_flags)  # the workspace is reused while it is large enough

    def _plan(self, scanned_only):
        return RZ._plan(RZ._dev_state(self.dev), self.P, self.W, self.H, "sync", scanned_only)

    def _enqueue(self, cap, bin_cap, plan_flags):
        """Enqueue the forward on self._cur.  -> its notify note (None: an empty view, nothing to check)"""
        P, W, H, lib = self.P, self.W, self.H, self.lib
        ptrs, fl, cam, family, _ = self._in
        stream = self._cur.cuda_stream
        flags = RZ._extra_flags | family | plan_flags | self.aa_flag
        self._ensure_ws(cap, self._cur, bin_cap)
        if P == 0:
            _capi.check(lib.gsr_forward(P, W, H, *ptrs, *fl, *cam, self.color.data_ptr(), self.radii.data_ptr(), self.ws.data_ptr(),
                                        self.nbytes, cap, flags, stream), "gsr_forward")
            return None
        ring = RZ._ring(self.dev)
        note, hdr_ptr = ring.acquire_notify()
        ext = RZ._ext(None, RZ._dev_state(self.dev).get("longest", 0), None, bin_cap)  # work order: longest lists first, relative to the longest list seen on this device
        rc = lib.gsr_forward_ex(P, W, H, *ptrs, *fl, *cam, self.color.data_ptr(), self.radii.data_ptr(), self.ws.data_ptr(),
                                self.nbytes, cap, flags, stream, hdr_ptr, note[3], C.byref(ext))
        if rc != 0:
            ring.release(note[1])
        _capi.check(rc, "gsr_forward_ex")
        return note

    def forward_end(self):
        """Second half of forward(): wait until the binning scan has published the instance count (typically well before the forward has
        finished), re-render with a larger workspace if it overflowed (rasterizer._repair_loop).  -> (color, radii)"""
        note, self._pending = self._pending, None
        if note is not None:
            RZ._repair_loop(RZ._dev_state(self.dev), note, self._cur, self.P, False, self.cap, self.bin_cap,
                            lambda scanned_only: (self._enqueue(*self._plan(scanned_only)), self.cap, self.bin_cap))
        return self.color, self.radii

    def backward(self, dL_dpix, color_grad=True, stream=None):
        """dL_dpix[3,H,W] fp32 contiguous -> dict of gradient tensors (the session's own buffers: valid until the next backward).
        color_grad=False: dL/dcolours is not needed (stage 2: the colours are input pixels) -- GSR_FLAG_NO_COLOR_GRAD, its buffer holds zeros."""
        if not self.training:
            raise RuntimeError("gps_gaussian_amd: this RasterSession was created with training=False (no backward workspace)")
        if self._in is None:
            raise RuntimeError("gps_gaussian_amd: RasterSession.backward() without a forward()")
        ptrs, fl, cam, family, _keep = self._in
        g = self._chk(dL_dpix, 3 * self.W * self.H, "dL_dpix")
        G = self.grads
        bstream = stream if stream is not None else torch.cuda.current_stream(self.dev)
        if not any(st is bstream or st == bstream for st in self._ws_streams):
            self._ws_streams.append(bstream)  # (the caller orders this stream against the forward's; the workspace must outlive both)
        if self.P > 0:
            ext = RZ._ext(None, 0, None, self.bin_cap)
            rc = self.lib.gsr_backward_ex(self.P, self.W, self.H, *ptrs, *fl, *cam, self.radii.data_ptr(), g, G["means3D"].data_ptr(),
                                          G["means2D"].data_ptr(), G["colors"].data_ptr(), G["opacities"].data_ptr(), G["scales"].data_ptr(),
                                          G["rotations"].data_ptr(), self.ws.data_ptr(), self.nbytes, self.cap,
                                          RZ._extra_flags | family | (0 if color_grad else _capi.GSR_FLAG_NO_COLOR_GRAD) | self.aa_flag,
                                          bstream.cuda_stream, C.byref(ext))
            _capi.check(rc, "gsr_backward_ex")
        return G
