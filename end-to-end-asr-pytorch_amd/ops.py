"""Operator layer: torch.autograd.Functions over the libasrk C ABI.

PyTorch is used for device memory (caching allocator), the current HIP stream and autograd
bookkeeping only; every tensor that reaches this module is turned into a raw device pointer and
handed to a hand-written gfx950 kernel.  Nothing here falls back to ATen math.
"""
import collections
import contextlib
import ctypes

import numpy as np
import torch
from torch.autograd import Function

from . import _lib

_ws_cache = {}


def _L():
    return _lib.load()


def _require_gpu(t):
    if not t.is_cuda:
        raise _lib.AsrkError("asrk ops need tensors on the MI355X (got %s); the product path has no "
                             "CPU fallback" % t.device)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """the current torch stream of the current device as a raw hipStream_t.  torch.cuda.current_stream() builds a Stream
    object through several Python layers (~9 us; ~40 launches per decode position: a fifth of a one-utterance position);
    the raw query is the same lookup without the object."""
    if _raw_stream is not None and _raw_device is not None:
        return ctypes.c_void_p(_raw_stream(_raw_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    """contiguous float32 view/copy (copy only when the caller handed something exotic)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def lstm_workspace(device):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    ws = _ws_cache.get(key)
    if ws is None:
        ws = torch.zeros(int(_L().asrk_lstm_ws_bytes()), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


# ---- per-call arithmetic / launch flags (include/asrk.h).  The library keeps no mode state; the HOST layer
# does, exactly like torch.backends.* switches: the split mode starts from ASRK_GEMM_SPLIT (0 = f32-input
# MFMA everywhere, 1 = exact bf16x6 operand splitting where it pays (default), 2 = wherever the shape
# allows) and bench.py / the tests flip it with set_gemm_split(); ASRK_REC_BF / ASRK_REC_BF_BWD = 0 select the
# f32-MFMA recurrence kernels.
import os as _os
_GEMM_SPLIT_FLAG = {0: 1, 1: 0, 2: 2}          # host mode -> ASRK_GEMM_SPLIT_{OFF, AUTO, ALWAYS}
_gemm_state = {"split": max(0, min(2, int(_os.environ.get("ASRK_GEMM_SPLIT", "1")))), "lds_hint": 0}


def set_gemm_split(mode):
    """0 = never split (v_mfma_f32_32x32x2_f32 everywhere), 1 = where it pays (default), 2 = always"""
    _gemm_state["split"] = max(0, min(2, int(mode)))


def get_gemm_split():
    return _gemm_state["split"]


def gemm_flags():
    return _GEMM_SPLIT_FLAG[_gemm_state["split"]] | ((_gemm_state["lds_hint"] & 0xff) << 8)


def gemm_takes_split(M, N, K):
    return bool(_L().asrk_gemm_takes_split(M, N, K, gemm_flags()))


def rec_flags(backward):
    """ASRK_REC_F32_MFMA when the environment asks for the f32-MFMA recurrence (read per call: the tests and
    bench.py's exact-f32 comparison toggle it)"""
    return 1 if _os.environ.get("ASRK_REC_BF_BWD" if backward else "ASRK_REC_BF", "1") == "0" else 0


ASRK_REC_REARM = 2            # include/asrk.h: the launch hands the exchange buffer back sentinel-filled
ASRK_REC_BWD_NO_DG = 4        # include/asrk.h: the BPTT launch stores dG in its panels only, not as f32 over the gates
_XCHG_REARM = _os.environ.get("ASRK_XCHG_REARM", "1") != "0"
_XCHG_POOL_CAP = int(float(_os.environ.get("ASRK_XCHG_POOL_GB", "24")) * (1 << 30))
# free[(device, stream)] = [[buffer, armed_bytes, last_use_tick], ...]; "stats" counts launches served without / with a
# fill pass (bench.py reports them)
_xchg_pool = {"free": {}, "bytes": 0, "tick": 0, "stats": {"hit": 0, "miss": 0, "evicted": 0}}


def _size_class(n):
    """n rounded up to four classes per octave (<= 25 % slack): utterance lengths differ from batch to batch, and a
    pool keyed by the exact footprint would miss on almost every launch of a real epoch"""
    if n <= 4096:
        return 4096
    q = 1 << (int(n - 1).bit_length() - 3)
    return (n + q - 1) // q * q


def _pool_evict(pool, need):
    """drop least-recently-used free buffers until `need` more bytes fit under the cap"""
    while pool["bytes"] + need > _XCHG_POOL_CAP:
        victim = None
        for key, lst in pool["free"].items():
            for i, e in enumerate(lst):
                if victim is None or e[2] < victim[2][2]:
                    victim = (key, i, e)
        if victim is None:
            return
        key, i, e = victim
        pool["free"][key].pop(i)
        pool["bytes"] -= e[0].numel()
        pool["stats"]["evicted"] += 1


class _Exchange:
    """Scratch for the in-kernel h / dG exchange of ONE recurrence launch.

    The kernels need it pre-filled with a NaN sentinel.  Rounds 1-4 took stream-ordered scratch and let every launch
    fill it first (eight fills per cfg3 step: 1.0 ms of stores in front of latency-bound kernels).  Now the launch is
    asked to hand the buffer back ARMED (ASRK_REC_REARM: the workgroups refill the region of step s - 2 while they
    compute step s) and the buffer goes into a pool.  An armed buffer is all 0xFF bytes whatever layout the launch that
    armed it used, so the pool is keyed by (device, stream) only and any free buffer that is large enough serves any
    shape: buffers come in size classes (four per octave), each remembers how many of its leading bytes have ever been
    armed (a launch that needs more than that runs its fill pass once and extends the extent), and the pool is bounded
    by evicting least-recently-used buffers (ASRK_XCHG_POOL_GB, default 24 of 288).  ASRK_XCHG_REARM=0 restores
    fill-per-launch.  A hand-off timeout leaves buffers dirty: check_errors() drops the pool before it raises.

        x = _Exchange(L, T, B, H, ndir, backward, device)
        check(L.asrk_..._rec_...(..., _p(x.buf), x.prefilled, ..., x.flags, stream));  x.done()"""

    __slots__ = ("buf", "prefilled", "flags", "key", "need", "armed")

    def __init__(self, L, T, B, H, ndir, backward, device):
        base = rec_flags(backward)
        n = int(L.asrk_lstm_xchg_bytes(T, B, H, ndir, backward, base))
        if n == 0:
            raise _lib.AsrkError("LSTM shape T=%d B=%d H=%d ndir=%d is not supported by the persistent "
                                 "gfx950 recurrence kernels" % (T, B, H, ndir))
        self.flags = base | (ASRK_REC_REARM if _XCHG_REARM else 0)
        self.need = n
        self.key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        if not _XCHG_REARM:
            self.buf, self.prefilled, self.armed = torch.empty(n, dtype=torch.uint8, device=device), 0, 0
            return
        free = _xchg_pool["free"].get(self.key, ())
        best = None
        for i, e in enumerate(free):       # the smallest buffer that is big enough; one armed far enough first
            if e[0].numel() >= n:
                rank = (e[1] < n, e[0].numel())
                if best is None or rank < best[0]:
                    best = (rank, i)
        if best is not None:
            e = free.pop(best[1])
            _xchg_pool["bytes"] -= e[0].numel()
            self.buf, self.armed = e[0], e[1]
        else:
            self.buf, self.armed = torch.empty(_size_class(n), dtype=torch.uint8, device=device), 0
        self.prefilled = 1 if self.armed >= n else 0
        _xchg_pool["stats"]["hit" if self.prefilled else "miss"] += 1

    def done(self):
        """the launch is enqueued: the first max(need, armed) bytes are armed for whoever comes next on this stream"""
        if not _XCHG_REARM:
            return
        n = self.buf.numel()
        if n > _XCHG_POOL_CAP:
            return
        _pool_evict(_xchg_pool, n)
        _xchg_pool["tick"] += 1
        _xchg_pool["free"].setdefault(self.key, []).append([self.buf, max(self.armed, self.need), _xchg_pool["tick"]])
        _xchg_pool["bytes"] += n


def drop_exchange_pool():
    _xchg_pool["free"].clear()
    _xchg_pool["bytes"] = 0


def pool_stats():
    """launches served from the exchange pool without / with a fill pass, panels emitted from the pool / skipped"""
    return {"exchange": dict(_xchg_pool["stats"], held_bytes=_xchg_pool["bytes"]),
            "panels": dict(_panel_pool["stats"], held_bytes=_panel_pool["bytes"])}


def check_errors(device=None):
    """Synchronises the current stream and raises if a persistent kernel's grid sync timed out."""
    for key, ws in list(_ws_cache.items()):
        rc = _L().asrk_lstm_check_error(_p(ws), _stream())
        if rc != 0:
            drop_exchange_pool()        # an aborted launch did not re-arm its exchange buffer
        _lib.check(rc, "lstm grid sync")


# --------------------------------------------------------------------------- deferred weight gradients
# Weight-gradient GEMMs (dW = dY^T X) are off the critical path of back-propagation: nothing
# downstream in the backward pass reads them.  They are therefore launched on a second HIP stream
# and run on the CUs the latency-bound kernels on the main stream leave idle (the persistent BPTT
# kernel of a 512-unit layer occupies 128 of 256 CUs; the attention-decoder loop far fewer).  The
# main stream re-joins the side stream at the end of the backward pass (autograd engine callback),
# so every consumer after `loss.backward()` sees finished gradients.  Deferral is only used when the
# gradient's consumer is a plain AccumulateGrad into an empty `.grad` (leaf weight, grad None).
_defer = {"enabled": True, "side": {}, "pending": {}, "cb_armed": False, "release": []}


def set_deferred_weight_grads(flag):
    """Enable/disable launching weight-gradient GEMMs on the side stream (default: enabled)."""
    join_deferred()
    _defer["enabled"] = bool(flag)


def join_deferred():
    """Make the current stream wait for all deferred weight-gradient work (no host sync)."""
    for dev, ev in list(_defer["pending"].items()):
        torch.cuda.current_stream(dev).wait_event(ev)
    _defer["pending"].clear()


def deferred_stream(device):
    """the side stream if weight-gradient work has been deferred onto it in this backward pass (so a
    gradient consumer can order itself after that work without stalling the main stream), else None"""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    return _defer["side"].get(dev) if dev in _defer["pending"] else None


def _end_of_backward():
    _defer["cb_armed"] = False
    join_deferred()
    rel, _defer["release"] = _defer["release"], []
    for pnl in rel:                  # pooled panels that side-stream GEMMs were still reading
        pnl.release()


def _can_defer(*weights):
    return _defer["enabled"] and all(w is None or (w.is_leaf and w.grad is None) for w in weights)


# LDS KiB requested by side-stream GEMMs (> 80 = one workgroup per CU: they hand CUs back sooner to the
# main stream's BPTT / dX kernels; 27.5 -> 25.9 ms/step at cfg2).  Only useful when the BPTT kernels
# leave CUs free (H=512 plans use 128 of 256); when they fill the chip (H=1024) the hint just slows
# the background work (cfg3 229 -> 233 ms), so it follows the last BPTT plan seen.  ASRK_SIDE_BG
# forces a value (0 = never).
_BG_FORCED = _os.environ.get("ASRK_SIDE_BG")
_BG_HINT = int(_BG_FORCED) if _BG_FORCED is not None else 0


# ---- phase hooks: callables run right after a persistent BPTT kernel has been enqueued on the main stream, i.e.
# at the start of that layer's GEMM phase (dX / dW).  parallel.DataParallelEngine uses it to launch its ready
# gradient buckets THERE: ordered behind the recurrence kernel (which owns every CU and cannot share one with a
# collective kernel) and beside the GEMMs that follow, instead of racing the next BPTT launch.
_gemm_phase_hooks = []


def on_gemm_phase(fn):
    _gemm_phase_hooks.append(fn)
    return fn


def remove_gemm_phase_hook(fn):
    if fn in _gemm_phase_hooks:
        _gemm_phase_hooks.remove(fn)


def _gemm_phase_begins():
    for fn in list(_gemm_phase_hooks):
        fn()


def _defer_beside_bptt():
    """Weight-gradient GEMMs of a layer may go to the side stream only if the BPTT kernel that follows them on
    the main stream leaves CUs free (H = 512 plans: 128 of 256).  The bf16x6 plans of the wide layers own every
    CU (one workgroup each, 132-143 KiB of LDS): a GEMM launched beside them is not overlapped but PARKED - its
    remaining tiles wait for the whole recurrence launch while the recurrence's workgroups wait for the CUs the
    GEMM still holds (profiles/r02_cfg3_step_timeline.log) - so there the GEMMs run in stream order.
    ASRK_DEFER_WIDE=1 restores the old behaviour for A/B."""
    return _BG_HINT > 0 or _os.environ.get("ASRK_DEFER_WIDE", "0") == "1"


def _note_bptt_plan(L, T, B, H, ndir):
    global _BG_HINT
    if _BG_FORCED is None:
        wgs = int(L.asrk_lstm_plan_workgroups(T, B, H, ndir, 1, rec_flags(1)))
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        _BG_HINT = 96 if 0 < 2 * wgs <= cus else 0


class _SideStream:
    """with _SideStream(device, inputs): kernels launched inside run on the side stream, ordered after
    everything already enqueued on the main stream; `inputs` (main-stream allocations read inside)
    are protected from early reuse by the caching allocator."""

    def __init__(self, device, inputs, background=True):
        self.device = torch.device(device)
        self.inputs = inputs
        self.hint = _BG_HINT if background else 0      # background: something latency-critical follows

    def __enter__(self):
        dev = self.device
        side = _defer["side"].get(dev)
        if side is None:
            side = torch.cuda.Stream(device=dev)
            _defer["side"][dev] = side
        main = torch.cuda.current_stream(dev)
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        for t in self.inputs:
            if t is not None:
                t.record_stream(side)
        self.main, self.side = main, side
        self.ctx = torch.cuda.stream(side)
        self.ctx.__enter__()
        self.prev_hint = _gemm_state["lds_hint"]
        if self.hint:
            _gemm_state["lds_hint"] = self.hint
        return self

    def keep(self, *outs):
        """outputs allocated on the side stream that the main stream will consume after the join"""
        for t in outs:
            if t is not None:
                t.record_stream(self.main)

    def __exit__(self, *exc):
        _gemm_state["lds_hint"] = self.prev_hint
        self.ctx.__exit__(*exc)
        done = torch.cuda.Event()
        done.record(self.side)
        _defer["pending"][self.device] = done
        if not _defer["cb_armed"]:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(_end_of_backward)
                _defer["cb_armed"] = True
            except RuntimeError:        # not inside a backward pass: join right away
                join_deferred()
        return False


# ---- gradient destinations.  A data-parallel engine reduces gradients in flat bucket buffers (parallel.py); an op
# that produces the gradient of a LEAF weight asks here where to write it, so the weight-gradient GEMM's output IS the
# bucket slice and no copy into the bucket is needed (692 MB per cfg3 step).  Without an engine: plain scratch.
_grad_dest = {"fn": None}


def set_grad_destination(fn):
    """fn(weight, shape) -> f32 tensor of `shape` to write that leaf's gradient into, or None; None unregisters"""
    _grad_dest["fn"] = fn


def grad_out(weight, shape, device):
    fn = _grad_dest["fn"]
    if fn is not None and weight is not None:
        t = fn(weight, tuple(shape))
        if t is not None:
            return t
    return torch.empty(shape, dtype=torch.float32, device=device)


def grad_has_destination(*weights):
    fn = _grad_dest["fn"]
    return fn is not None and all(w is not None and fn(w, tuple(w.shape)) is not None for w in weights)


# --------------------------------------------------------------------------- raw wrappers
def gemm(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, alpha=1.0, beta=0.0, bias=None, bias2=None,
         splitk=0):
    _require_gpu(C)
    # operand extents must cover what the kernel will touch (A: M x K, B: K x N as stored, C: M x N)
    ra, ca = (K, M) if transA else (M, K)
    rb, cb = (N, K) if transB else (K, N)
    for name, t, r, c, ld in (("A", A, ra, ca, lda), ("B", B, rb, cb, ldb), ("C", C, M, N, ldc)):
        avail = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        if r > 0 and c > 0 and (ld < c or avail < (r - 1) * ld + c):
            raise _lib.AsrkError("gemm: operand {} ({} elements behind the pointer) too small for {}x{} "
                                 "with ld {}".format(name, avail, r, c, ld))
    L = _L()
    flags = gemm_flags()
    # split panels of both operands: scratch from torch's caching allocator (stream-ordered, so the block is
    # safe to hand out again as soon as this call's kernels are enqueued)
    nws = int(L.asrk_gemm_ws_bytes(M, N, K, flags)) if splitk <= 0 else 0
    ws = torch.empty((nws,), dtype=torch.uint8, device=C.device) if nws else None
    _lib.check(L.asrk_gemm_f32(int(transA), int(transB), M, N, K, alpha, _p(A), lda, _p(B), ldb,
                               beta, _p(C), ldc, _p(bias), _p(bias2), splitk, flags, _p(ws), nws, _stream()),
               "gemm")


class SplitPanel:
    """bf16x3 split panel of a logical [rows][K] f32 operand (csrc/gemm_split.hip): built once, usable as
    either operand of several gemm_panels calls.  trans: `src` is stored [K][rows] with leading dimension ld."""

    def __init__(self, src, ld, rows, K, trans):
        _require_gpu(src)
        L = _L()
        need = (K - 1) * ld + rows if trans else (rows - 1) * ld + K
        avail = src.untyped_storage().nbytes() // src.element_size() - src.storage_offset()
        if ld < (rows if trans else K) or avail < need:
            raise _lib.AsrkError("split panel: source too small for {}x{} (trans={}) with ld {}".format(
                rows, K, trans, ld))
        self.rows, self.K = rows, K
        self.flags = 0                            # reserved (include/asrk.h)
        self.buf = torch.empty((L.asrk_split_panel_bytes(rows, K, self.flags),), dtype=torch.uint8,
                               device=src.device)
        _lib.check(L.asrk_split_panel_f32(_p(src), ld, rows, K, int(trans), _p(self.buf), self.flags, _stream()),
                   "split_panel")


# ---- panels written by their producers (round 5).  A recurrence launch can store its output (forward) / dG (BPTT) as
# the row-major split panel the GEMM that follows multiplies, so that GEMM needs no split pass over the tensor: 183 M + 367 M
# elements x 10 B per cfg3 step.  The buffers are pooled (zero-initialised ONCE: the kernels overwrite the real extent, the
# padding stays zero) per (device, stream, rows, K).  A forward panel travels from the layer that wrote it to the layer that
# reads it through a one-slot hand-over keyed by the IDENTITY of the output tensor (weak reference + version counter):
# whatever sits between two layers (LayerNorm, dropout, projection) makes a new tensor and the consumer falls back to
# splitting its input itself.  ASRK_REC_PANELS=0 turns both off.
import weakref as _weakref
_REC_PANELS = _os.environ.get("ASRK_REC_PANELS", "1") != "0"
# a BPTT launch whose dG is read from its panels alone does not store the f32 dG (LSTMLayerFn.backward, include/asrk.h:
# ASRK_REC_BWD_NO_DG); False: always store
_REC_SKIP_DG = True
# free[(device, stream, rows, K)] = [[buffer, 0, last_use_tick], ...]; "seen" = shapes asked for before
_panel_pool = {"free": {}, "bytes": 0, "tick": 0, "seen": {}, "stats": {"hit": 0, "miss": 0, "skipped": 0, "evicted": 0}}
_panel_state = {"hint": False, "handover": None,
                "stats": {"emitted": 0, "consumed": 0, "dg": 0, "dgt": 0, "no_dg": 0, "dw_ih_splitk": 0}}


class _BlankPanel:
    """a pooled, zero-initialised panel buffer of a logical [rows][K] operand, to be filled by a recurrence kernel.

    A new buffer costs a zero fill over the whole panel (the kernels write the real extent, the padding must be zero),
    which is what the emission saves downstream - so a panel is only worth emitting for a shape that comes back.
    `_BlankPanel.take` therefore returns None the FIRST time a (rows, K) is asked for (the consumer splits its operand
    itself, as without the feature) and allocates on the second; fixed-shape training pays two steps of split passes,
    an epoch of ever-changing lengths pays no fills at all.  The pool is bounded like the exchange pool (LRU)."""
    __slots__ = ("buf", "rows", "K", "flags", "key")

    @staticmethod
    def take(rows, K, device):
        key = (device.index, torch.cuda.current_stream(device).cuda_stream, rows, K)
        free = _panel_pool["free"].get(key)
        if free:
            e = free.pop()
            _panel_pool["bytes"] -= e[0].numel()
            _panel_pool["stats"]["hit"] += 1
            return _BlankPanel(rows, K, key, e[0])
        seen = _panel_pool["seen"]
        if key not in seen:
            if len(seen) > 4096:
                seen.clear()
            seen[key] = 1
            _panel_pool["stats"]["skipped"] += 1
            return None
        _panel_pool["stats"]["miss"] += 1
        n = int(_L().asrk_split_panel_bytes(rows, K, 0))
        buf = torch.empty((n,), dtype=torch.uint8, device=device)
        _lib.check(_L().asrk_fill_f32(_p(buf), n // 4, 0.0, _stream()), "fill")      # panel sizes are multiples of 16 B
        return _BlankPanel(rows, K, key, buf)

    def __init__(self, rows, K, key, buf):
        self.rows, self.K, self.flags, self.key, self.buf = rows, K, 0, key, buf

    def release(self):
        n = self.buf.numel()
        if n > _XCHG_POOL_CAP:
            return
        _pool_evict(_panel_pool, n)
        _panel_pool["tick"] += 1
        _panel_pool["free"].setdefault(self.key, []).append([self.buf, 0, _panel_pool["tick"]])
        _panel_pool["bytes"] += n


def set_panel_hint(flag):
    """the caller (Encoder.forward) knows that the NEXT consumer of the coming LSTM layer's output is another LSTM layer's
    input projection with nothing in between: worth emitting that output as a panel"""
    _panel_state["hint"] = bool(flag)


def _take_handover(x):
    h, _panel_state["handover"] = _panel_state["handover"], None
    if h is None:
        return None
    ref, version, panel = h
    if ref() is x and x._version == version and panel.rows == x.shape[0] * x.shape[1] and panel.K == x.shape[2]:
        return panel
    panel.release()
    return None


def gemm_panels(M, N, K, A, a_row0, a_k0, B, b_row0, b_k0, C, ldc, alpha=1.0, beta=0.0, bias=None, bias2=None,
                splitk=None):
    """C[M,N] = alpha * A[a_row0:+M, a_k0:+K] B[b_row0:+N, b_k0:+K]^T + beta C (+ biases), A / B SplitPanels.
    splitk: None = one workgroup per output tile; n >= 1 = K cut into n slices summed in a fixed order (few tiles, deep
    K); 0 = the library chooses n"""
    _require_gpu(C)
    avail = C.untyped_storage().nbytes() // C.element_size() - C.storage_offset()
    if ldc < N or avail < (M - 1) * ldc + N:
        raise _lib.AsrkError("gemm_panels: C too small for {}x{} with ld {}".format(M, N, ldc))
    if A.flags != B.flags:
        raise _lib.AsrkError("gemm_panels: the two panels were built in different layouts")
    L = _L()
    if splitk is None:
        _lib.check(L.asrk_gemm_panels_f32(M, N, K, alpha, _p(A.buf), A.rows, A.K, a_row0, a_k0, _p(B.buf), B.rows,
                                          B.K, b_row0, b_k0, beta, _p(C), ldc, _p(bias), _p(bias2), A.flags,
                                          _stream()), "gemm_panels")
        return
    # the slices' partial sums: scratch from torch's caching allocator (stream-ordered, like ops.gemm's panels)
    nws = int(L.asrk_gemm_panels_splitk_ws_bytes(M, N, splitk))
    ws = torch.empty((nws,), dtype=torch.uint8, device=C.device)
    _lib.check(L.asrk_gemm_panels_splitk_f32(M, N, K, alpha, _p(A.buf), A.rows, A.K, a_row0, a_k0, _p(B.buf), B.rows,
                                             B.K, b_row0, b_k0, beta, _p(C), ldc, _p(bias), _p(bias2), splitk, _p(ws),
                                             nws, A.flags, _stream()), "gemm_panels")


def zeros(shape, device):
    """float32 zeros through asrk_fill_f32 (no ATen fill kernel on the hot path)"""
    t = torch.empty(shape, dtype=torch.float32, device=device)
    if t.numel():
        _lib.check(_L().asrk_fill_f32(_p(t), t.numel(), 0.0, _stream()), "fill")
    return t


def copy_flat(dst, src):
    """dst[:] = src for contiguous f32 tensors of equal size (asrk_copy3d_f32)"""
    n = src.numel()
    if n:
        copy3d(src, dst, 1, 1, n, 0, 0, 0, 0)


def copy3d(src, dst, n0, n1, n2, ss0, ss1, ds0, ds1, accumulate=False):
    _require_gpu(dst)
    _lib.check(_L().asrk_copy3d_f32(_p(src), _p(dst), n0, n1, n2, ss0, ss1, ds0, ds1,
                                    int(accumulate), _stream()), "copy3d")


def colsum(X, M, N, ldx, out, accumulate=False):
    _lib.check(_L().asrk_colsum_f32(_p(X), M, N, ldx, _p(out), int(accumulate), _stream()), "colsum")


# --------------------------------------------------------------------------- Linear (+ tanh)
class LinearFn(Function):
    """y = x W^T + b  (torch.nn.Linear semantics; reference: src/asr.py:29,179,243-248)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_gpu(x)
        x2 = _f32c(x).reshape(-1, x.shape[-1])
        w = _f32c(weight)
        M, K = x2.shape
        N = w.shape[0]
        if w.dim() != 2 or w.shape[1] != K or (bias is not None and bias.numel() != N):
            # torch.nn.functional.linear raises the same way; never let the kernel read out of bounds
            raise RuntimeError("linear: input [..., {}] cannot be multiplied with weight {} (bias {})".format(
                K, tuple(w.shape), None if bias is None else tuple(bias.shape)))
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        gemm(0, 1, M, N, K, x2, K, w, K, y, N, bias=bias)
        ctx.save_for_backward(x2, w)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        ctx.in_shape = x.shape
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        M, K = x2.shape
        N = w.shape[0]
        dy2 = _f32c(dy).reshape(M, N)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((M, K), dtype=torch.float32, device=dy.device)
            gemm(0, 0, M, K, N, dy2, N, w, K, dx, K)
            dx = dx.reshape(ctx.in_shape)
        def param_grads():
            dw_ = db_ = None
            if ctx.needs_input_grad[1]:
                dw_ = grad_out(w, (N, K), dy.device)
                gemm(1, 0, N, K, M, dy2, N, x2, K, dw_, K)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                db_ = torch.empty((N,), dtype=torch.float32, device=dy.device)
                colsum(dy2, M, N, N, db_)
            return dw_, db_

        if M >= 1024 and _can_defer(w, ctx.bias_ref) and _defer_beside_bptt():
            with _SideStream(dy.device, (dy2, x2)) as side:
                dw, db = param_grads()
                side.keep(dw, db)
        else:
            dw, db = param_grads()
        return dx, dw, db


def linear(x, weight, bias=None):
    if not torch.is_grad_enabled():              # inference: no autograd node (decode positions are launch-bound)
        _require_gpu(x)
        x2 = _f32c(x).reshape(-1, x.shape[-1])
        w = _f32c(weight)
        M, K = x2.shape
        N = w.shape[0]
        if w.dim() != 2 or w.shape[1] != K or (bias is not None and bias.numel() != N):
            raise RuntimeError("linear: input [..., {}] cannot be multiplied with weight {} (bias {})".format(
                K, tuple(w.shape), None if bias is None else tuple(bias.shape)))
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        gemm(0, 1, M, N, K, x2, K, w, K, y, N, bias=bias)
        return y.reshape(*x.shape[:-1], N)
    return LinearFn.apply(x, weight, bias)


class TanhFn(Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        xc = _f32c(x)
        y = torch.empty_like(xc)
        _lib.check(_L().asrk_tanh_fwd_f32(_p(xc), _p(y), xc.numel(), _stream()), "tanh")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dyc = _f32c(dy)
        dx = torch.empty_like(y)
        _lib.check(_L().asrk_tanh_bwd_f32(_p(y), _p(dyc), _p(dx), y.numel(), _stream()), "tanh_bwd")
        return dx


def tanh(x):
    return TanhFn.apply(x)


def tanh_(x):
    """in place, no autograd (inference buffers); x contiguous float32"""
    _require_gpu(x)
    assert x.is_contiguous() and x.dtype == torch.float32
    _lib.check(_L().asrk_tanh_fwd_f32(_p(x), _p(x), x.numel(), _stream()), "tanh")
    return x


# --------------------------------------------------------------------------- log-softmax
class LogSoftmaxFn(Function):
    """F.log_softmax(x, dim=-1) (reference: src/asr.py:96, src/decode.py:93,121)."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        xc = _f32c(x)
        V = xc.shape[-1]
        rows = xc.numel() // V
        y = torch.empty_like(xc)
        _lib.check(_L().asrk_log_softmax_fwd_f32(_p(xc), _p(y), rows, V, V, _stream()), "log_softmax")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        V = y.shape[-1]
        rows = y.numel() // V
        dyc = _f32c(dy)
        dx = torch.empty_like(y)
        _lib.check(_L().asrk_log_softmax_bwd_f32(_p(y), _p(dyc), _p(dx), rows, V, V, _stream()),
                   "log_softmax_bwd")
        return dx


def log_softmax(x):
    if not torch.is_grad_enabled():              # inference: the kernel call without the autograd node around it
        _require_gpu(x)
        xc = _f32c(x)
        V = xc.shape[-1]
        y = torch.empty_like(xc)
        _lib.check(_L().asrk_log_softmax_fwd_f32(_p(xc), _p(y), xc.numel() // V, V, V, _stream()), "log_softmax")
        return y
    return LogSoftmaxFn.apply(x)


def topk(x, k):
    """(values, indices) of the k largest entries along the last axis, descending; ties -> smaller
    index.  No gradient (selection only: greedy feedback, beam pruning, hypothesis read-out)."""
    _require_gpu(x)
    xc = _f32c(x.detach())
    V = xc.shape[-1]
    rows = xc.numel() // V
    vals = torch.empty(xc.shape[:-1] + (k,), dtype=torch.float32, device=x.device)
    idx = torch.empty(xc.shape[:-1] + (k,), dtype=torch.int64, device=x.device)
    _lib.check(_L().asrk_topk_f32(_p(xc), rows, V, V, k, _p(vals), _p(idx), _stream()), "topk")
    return vals, idx


def argmax(x):
    """torch.argmax(x, dim=-1) (first maximum)"""
    return topk(x, 1)[1].squeeze(-1)


def token_crop(ids, pad_idx=0, eos_idx=1, ignore_repeat=False):
    """rows of token ids [B, T] int64 on the device -> (compacted ids [B, T], lengths [B] int32): everything
    before the first <eos>, pads dropped, CTC repeats merged on request - the crop of every reference text
    encoder's decode() (src/text.py:61-71), for the whole batch in one launch"""
    _require_gpu(ids)
    x = ids.to(torch.int64)
    if x.dim() != 2:
        raise _lib.AsrkError("token_crop expects [B, T] ids")
    if x.stride(1) != 1:
        x = x.contiguous()
    B, T = x.shape
    out = torch.zeros((B, max(T, 1)), dtype=torch.int64, device=x.device)
    n = torch.zeros((B,), dtype=torch.int32, device=x.device)
    _lib.check(_L().asrk_token_crop_i64(_p(x), x.stride(0) if B else T, B, T, pad_idx, eos_idx, int(ignore_repeat),
                                        _p(out), out.stride(0), _p(n), _stream()), "token_crop")
    return out, n


def edit_distance(a, a_len, b, b_len):
    """Levenshtein distances [B] int32 of B pairs of int64 symbol rows (a [B, La], b [B, Lb], lengths int32) on
    the device (replaces editdistance.eval, src/util.py:126)"""
    _require_gpu(a)
    a, b = a.to(torch.int64).contiguous(), b.to(torch.int64).contiguous()
    a_len, b_len = a_len.to(torch.int32).contiguous(), b_len.to(torch.int32).contiguous()
    B = a.shape[0]
    if b.shape[0] != B or a_len.numel() != B or b_len.numel() != B:
        raise _lib.AsrkError("edit_distance: batch sizes differ")
    if b.shape[1] > 4096 and a.shape[1] <= 4096:      # the kernel keeps rows of the SECOND sequence in LDS; the
        a, a_len, b, b_len = b, b_len, a, a_len       # distance is symmetric, so put the shorter one there
    d = torch.empty((B,), dtype=torch.int32, device=a.device)
    _lib.check(_L().asrk_edit_distance_i64(_p(a), a.shape[1], _p(a_len), _p(b), b.shape[1], _p(b_len), B,
                                           b.shape[1], _p(d), _stream()), "edit_distance")
    return d


# --------------------------------------------------------------------------- layout moves
class SwapBTFn(Function):
    """[A,B,F] -> [B,A,F] (batch-major <-> time-major); its own inverse."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        xc = _f32c(x)
        A, B, F = xc.shape
        y = torch.empty((B, A, F), dtype=torch.float32, device=x.device)
        copy3d(xc, y, A, B, F, B * F, F, F, A * F)
        return y

    @staticmethod
    def backward(ctx, dy):
        return SwapBTFn.apply(dy)


def swap_bt(x):
    return SwapBTFn.apply(x)


class PyramidFn(Function):
    """Time reduction of src/module.py:141-153 on a time-major tensor [T,B,F].

    'concat': drop T % r trailing frames, out[t'] = cat(x[r t'], ..., x[r t' + r - 1]) -> [T//r,B,rF]
    'drop'  : out[t'] = x[r t']                                                   -> [ceil(T/r),B,F]
    """

    @staticmethod
    def forward(ctx, x, rate, style):
        _require_gpu(x)
        xc = _f32c(x)
        T, B, F = xc.shape
        ctx.meta = (T, B, F, rate, style)
        if style == "concat":
            To = T // rate
            y = torch.empty((To, B, rate * F), dtype=torch.float32, device=x.device)
            for j in range(rate):
                copy3d(xc[j:], y[:, :, j * F:], To, B, F, rate * B * F, F, B * rate * F, rate * F)
        else:
            To = (T + rate - 1) // rate
            y = torch.empty((To, B, F), dtype=torch.float32, device=x.device)
            copy3d(xc, y, To, B, F, rate * B * F, F, B * F, F)
        return y

    @staticmethod
    def backward(ctx, dy):
        T, B, F, rate, style = ctx.meta
        dyc = _f32c(dy)
        # 'concat' with T % rate == 0 overwrites every element; otherwise dropped frames get zero
        if style == "concat" and T % rate == 0:
            dx = torch.empty((T, B, F), dtype=torch.float32, device=dy.device)
        else:
            dx = zeros((T, B, F), dy.device)
        if style == "concat":
            To = T // rate
            for j in range(rate):
                copy3d(dyc[:, :, j * F:], dx[j:], To, B, F, B * rate * F, rate * F, rate * B * F, F)
        else:
            To = (T + rate - 1) // rate
            copy3d(dyc, dx, To, B, F, B * F, F, rate * B * F, F)
        return dx, None, None


def pyramid(x_tm, rate, style):
    return PyramidFn.apply(x_tm, rate, style)


# --------------------------------------------------------------------------- LSTM layer
def _pyramid_out(T, B, F, rate, style, dev, zero=False):
    """-> (mode, Y2): the recurrence kernels' time-reduction mode (0 none, 1 'concat', 2 'drop'; src/module.py:141-153)
    and the reduced output [T', B, F'] they store beside the layer output [T, B, F] (None for mode 0)"""
    mode = {None: 0, 'concat': 1, 'drop': 2}[style if rate > 1 else None]
    if mode == 0:
        return 0, None
    shape = (T // rate, B, rate * F) if mode == 1 else ((T + rate - 1) // rate, B, F)
    return mode, zeros(shape, dev) if zero else torch.empty(shape, dtype=torch.float32, device=dev)


def _db_in_kernel(has_bias, B):
    # The bias gradient (column sums of dG) comes out of the BPTT kernel itself.  In-kernel accumulation adds one partial
    # sum per BATCH GROUP (16 or 32 rows) to each element with a float atomic: with <= 2 groups (B <= 32, every BASELINE
    # workload) the result does not depend on the arrival order (a + b == b + a, the first add lands on an exact 0), i.e.
    # it is bit-reproducible; with more groups the order would matter, so those shapes take the deterministic column-sum
    # pass.
    return has_bias and B <= 32


@contextlib.contextmanager
def _bptt_launch(L, T, B, H, ndir, has_bias, G, dev):
    """What surrounds the persistent BPTT launch of an LSTM or GRU layer (G [T*B, ndir*4H]: gates in, dG out):
        with _bptt_launch(...) as (x, db_all):  enqueue the kernel with the exchange x, bias sums to db_all if _db_in_kernel
    On exit the exchange goes back to its pool, the bias sums the kernel did not take are column sums of dG, and the
    layer's GEMM phase begins."""
    _note_bptt_plan(L, T, B, H, ndir)
    x = _Exchange(L, T, B, H, ndir, 1, dev)
    db_all = torch.empty((ndir, 4 * H), dtype=torch.float32, device=dev) if has_bias else None
    yield x, db_all
    x.done()
    if has_bias and not _db_in_kernel(has_bias, B):
        colsum(G, T * B, ndir * 4 * H, ndir * 4 * H, db_all)
    _gemm_phase_begins()


# What one LSTM layer backward launches is decided by lstm_bwd_plan and executed by LSTMLayerFn.backward.  The schedules
# of the weight-gradient GEMMs:
STREAM = "STREAM"                                 # both directions on the main stream
SIDE_ALL = "SIDE_ALL"                             # both directions on the side stream, as background work
SIDE_REVERSE_SHARED = "SIDE_REVERSE_SHARED"       # reverse on the side stream; both read the ONE dG^T panel
SIDE_REVERSE = "SIDE_REVERSE"                     # reverse on the side stream, f32 GEMMs
IH_PANELS, IH_SPLITK, IH_F32 = "panels", "panels_splitk", "f32"      # dW_ih: each stacked (rows_ih = 8H) or per direction
# defer_release: the pooled dG^T panel goes back at the end of the backward pass whatever else is pending (otherwise right
# after the launches, unless side-stream work of this pass is pending then)
LstmBwdPlan = collections.namedtuple("LstmBwdPlan", "pG pGT db_in_kernel skip_dg rows_ih dw_ih_route dw_hh_panels "
                                                    "schedule defer_release")


def lstm_bwd_plan(T, B, Din, H, ndir, has_bias, needs_dx, stacked, can_defer, to_scratch, beside_bptt, bf_bwd, share_env,
                  skip_dg_switch, takes_split, take_panel):
    """Pure: no tensor, stream, device or environment variable is touched.  stacked: the forward kept a w_stack;
    to_scratch: no gradient destination is registered for w_ih; beside_bptt: _defer_beside_bptt() after _note_bptt_plan;
    bf_bwd: _REC_PANELS and a bf16x6 BPTT plan; share_env: ASRK_SHARE_PANELS != "0"; skip_dg_switch: _REC_SKIP_DG;
    takes_split(M, N, K): the split GEMM's routing rule; take_panel(rows, K) -> a pooled panel or None."""
    M = T * B
    # the input-gradient GEMM dX = dG [W_ih_f; W_ih_r] multiplies dG as its row-major A panel, the weight-gradient GEMMs
    # multiply dG^T as theirs: the BPTT kernel writes both itself where its plan can (bf16x6) and the GEMMs run in
    # stream order (the wide layers; side-stream consumers would outlive the pooled buffer)
    pG = pGT = None
    if bf_bwd and needs_dx and stacked and takes_split(M, Din, 8 * H):
        pG = take_panel(M, 8 * H)
    # Weight gradients contract over the tokens with dG^T as the left operand three times (dW_ih, dW_hh of both
    # directions): on the split-GEMM path dG^T (and Y^T, X^T) are split ONCE into bf16 panels and the GEMMs take row / k
    # ranges of them.  Needs every direction's GEMMs to see the one set of panels (not SIDE_REVERSE).
    share0 = share_env and T > 1 and H % 128 == 0 and B % 8 == 0 and takes_split(4 * H, H, (T - 1) * B)
    if bf_bwd and share0 and B % 16 == 0 and not beside_bptt:
        pGT = take_panel(ndir * 4 * H, M)
    # both directions' dW_ih share one launch only when they are computed on the same stream - and only into scratch:
    # with a data-parallel engine each direction's GEMM writes its rows straight into that weight's slice of the
    # gradient bucket (two launches of 4H rows: still >= 2 full rounds of tiles on the wide layers)
    rows_ih = 8 * H if stacked and (needs_dx or not can_defer) and to_scratch else 4 * H
    wide_ih = Din % 4 == 0 and takes_split(rows_ih, Din, M)
    # A NARROW input (cfg3's bottom layer: Din = 80) leaves dW_ih = dG^T X too few output tiles for the split GEMM's
    # routing rule, yet its K is as deep as the wide layers': it multiplies the dG^T panel too, K cut into slices that a
    # second kernel sums in a fixed order, one launch over both directions' rows where the result goes to scratch.
    # (Until round 6 it ran as exact-f32 GEMMs that read the f32 dG again: 3.4 ms of kernels per cfg3 step.)
    narrow_ih = pGT is not None and Din % 4 == 0 and not wide_ih
    if narrow_ih and stacked and to_scratch:
        rows_ih = 8 * H
    # Does anything read the f32 dG?  Not when every weight gradient multiplies dG^T (with pGT no schedule is
    # SIDE_REVERSE; dW_ih takes panels when Din % 4 == 0), dX is not wanted or multiplies the dG panel, and the bias
    # gradient was summed in the kernel: then the kernel keeps its four 4-byte stores per cell and step.
    db_in_kernel = _db_in_kernel(has_bias, B)
    skip_dg = bool(skip_dg_switch and pGT is not None and Din % 4 == 0 and (not needs_dx or pG is not None)
                   and (db_in_kernel or not has_bias))
    if not (can_defer and (beside_bptt or not needs_dx)):
        # a BPTT kernel that owns every CU follows (_defer_beside_bptt: a GEMM beside it is PARKED), or the gradients'
        # consumer is no plain AccumulateGrad
        schedule = STREAM
    elif needs_dx or ndir == 1:
        schedule = SIDE_ALL        # off the critical path: the next layer's BPTT does not need dW / db
    elif pGT is None:
        # bottom layer (no input gradient wanted): no BPTT follows, nothing to hide behind.  Its small GEMMs (dW_ih with
        # Din = 80, column sums) leave CUs idle one at a time, so the two directions run side by side: reverse on the
        # side stream, forward on the main stream.
        schedule = SIDE_REVERSE
    elif Din % 4 == 0:
        # bottom layer with the dG^T panel from the kernel: every weight gradient multiplies panels (dW_ih with a wide
        # input like the layers above, with a narrow one through the split-K launch) and fills the chip on its own.
        # (Until round 6 the narrow-input case ran its directions on two streams beside each other for the sake of the
        # small f32 dW_ih GEMMs; the 256-tile dW_hh launches only serialised there.)
        schedule = STREAM
    else:
        # the same with an input width no panel takes: dW_hh multiplies row ranges of the ONE dG^T panel (and of Y^T,
        # split before the streams fork), dW_ih reads the f32 dG; the directions run side by side, the pooled panel
        # goes back at the end of the backward pass (after the streams re-join)
        schedule = SIDE_REVERSE_SHARED
    panels = bool(share0) and schedule != SIDE_REVERSE
    route = IH_SPLITK if narrow_ih else IH_PANELS if panels and wide_ih else IH_F32
    return LstmBwdPlan(pG, pGT, db_in_kernel, skip_dg, rows_ih, route, panels, schedule, schedule == SIDE_REVERSE_SHARED)


class LSTMLayerFn(Function):
    """One (bi)directional LSTM layer on a time-major sequence [T,B,Din] -> [T,B,ndir*H].

    Same math as nn.LSTM(Din, H, bidirectional, num_layers=1) with zero initial state over the full
    padded length (reference: src/module.py:112-113,131).  Input projection = MFMA GEMM, time loop =
    persistent recurrence kernel; backward = persistent BPTT kernel + 4 GEMMs + column sums.
    """

    @staticmethod
    def forward(ctx, x, w_ih_f, w_hh_f, b_ih_f, b_hh_f, w_ih_r, w_hh_r, b_ih_r, b_hh_r, pyr_rate=1,
                pyr_style=None):
        """pyr_style 'concat' / 'drop' with pyr_rate > 1: the time reduction that follows the layer
        (src/module.py:141-153) is fused into the recurrence kernel's output store and the returned
        tensor is already the next layer's input [T', B, D']; backward reads the gradient in that
        layout directly."""
        _require_gpu(x)
        L = _L()
        xc = _f32c(x)
        T, B, Din = xc.shape
        H = w_hh_f.shape[1]
        ndir = 2 if w_ih_r is not None else 1
        dev = x.device
        M = T * B
        G = torch.empty((M, ndir * 4 * H), dtype=torch.float32, device=dev)
        w_ih_f, w_hh_f = _f32c(w_ih_f), _f32c(w_hh_f)
        w_stack = None
        if ndir == 2:
            w_ih_r, w_hh_r = _f32c(w_ih_r), _f32c(w_hh_r)
        # stacking pays where the GEMMs own the chip (wide layers: the persistent kernels fill every CU, so
        # nothing co-runs); at H = 512 the weight-gradient GEMMs run throttled beside the BPTT kernels and
        # two smaller launches interleave better (cfg2: 22.4 ms/step unstacked, 23.0 stacked)
        if ndir == 2 and H >= 768 and _os.environ.get("ASRK_STACK_DIRS", "1") != "0":
            # both directions read the same X: ONE GEMM with N = 8H over the stacked weights (a device
            # copy of 2 x 4H x Din floats) instead of two - better tile quantisation, X panels fetched
            # once; the same stack serves dX (one K = 8H contraction) and dW_ih in the backward pass
            if (w_ih_f.untyped_storage().data_ptr() == w_ih_r.untyped_storage().data_ptr()
                    and w_ih_r.storage_offset() == w_ih_f.storage_offset() + 4 * H * Din):
                # the parameter container keeps the two directions adjacent (RNNParams.colocate_directions): a view
                w_stack = w_ih_f.as_strided((8 * H, Din), (Din, 1))
            else:
                w_stack = torch.empty((8 * H, Din), dtype=torch.float32, device=dev)
                copy_flat(w_stack[:4 * H], w_ih_f)
                copy_flat(w_stack[4 * H:], w_ih_r)
            if b_ih_f is not None:
                b1 = torch.empty((2, 8 * H), dtype=torch.float32, device=dev)   # rows: b_ih | b_hh, both directions
                for row, (bf_, br_) in enumerate(((b_ih_f, b_ih_r), (b_hh_f, b_hh_r))):
                    copy_flat(b1[row, :4 * H], _f32c(bf_.detach()))
                    copy_flat(b1[row, 4 * H:], _f32c(br_.detach()))
                b1, b2 = b1[0], b1[1]
            else:
                b1 = b2 = None
            x_panel = _take_handover(x) if x is xc else None
            if x_panel is not None and gemm_takes_split(M, 8 * H, Din):
                # the layer below wrote this input as a split panel already: only the weights are split here
                pW = SplitPanel(w_stack, Din, 8 * H, Din, False)
                gemm_panels(M, 8 * H, Din, x_panel, 0, 0, pW, 0, 0, G, 8 * H, bias=b1, bias2=b2)
                del pW
                _panel_state["stats"]["consumed"] += 1
            else:
                gemm(0, 1, M, 8 * H, Din, xc, Din, w_stack, Din, G, 8 * H, bias=b1, bias2=b2)
            if x_panel is not None:
                x_panel.release()
        else:
            gemm(0, 1, M, 4 * H, Din, xc, Din, w_ih_f, Din, G, ndir * 4 * H, bias=b_ih_f, bias2=b_hh_f)
            if ndir == 2:
                gemm(0, 1, M, 4 * H, Din, xc, Din, w_ih_r, Din, G[:, 4 * H:], ndir * 4 * H, bias=b_ih_r,
                     bias2=b_hh_r)
        Y = torch.empty((M, ndir * H), dtype=torch.float32, device=dev)
        C = torch.empty((M, ndir * H), dtype=torch.float32, device=dev)
        ws = lstm_workspace(dev)
        xc_ = _Exchange(L, T, B, H, ndir, 0, dev)
        mode, Y2 = _pyramid_out(T, B, ndir * H, pyr_rate, pyr_style, dev)
        rate = max(1, pyr_rate)
        out_panel = None
        if (_REC_PANELS and _panel_state["hint"] and mode in (0, 1) and (mode == 0 or T // rate > 0) and
                (ndir * H) % 8 == 0 and L.asrk_lstm_plan_is_bf(T, B, H, ndir, 0, rec_flags(0))):
            r_ = rate if mode == 1 else 1
            out_panel = _BlankPanel.take((T // r_) * B, r_ * ndir * H, dev)
        if out_panel is not None:
            _panel_state["stats"]["emitted"] += 1
            _lib.check(L.asrk_lstm_rec_fwd_pyr_panel_f32(_p(G), _p(w_hh_f), _p(w_hh_r), _p(Y), _p(C), T, B, H, ndir,
                                                         _p(xc_.buf), xc_.prefilled, _p(ws), _p(Y2), mode, rate,
                                                         _p(out_panel.buf), xc_.flags, _stream()), "lstm_rec_fwd")
        else:
            _lib.check(L.asrk_lstm_rec_fwd_pyr_f32(_p(G), _p(w_hh_f), _p(w_hh_r), _p(Y), _p(C), T, B, H, ndir,
                                                   _p(xc_.buf), xc_.prefilled, _p(ws), _p(Y2), mode, rate,
                                                   xc_.flags, _stream()), "lstm_rec_fwd")
        xc_.done()
        ctx.pyr = (mode, max(1, pyr_rate))
        ctx.dims = (T, B, Din, H, ndir)
        ctx.has_bias = b_ih_f is not None
        ctx.bias_refs = (b_ih_f, b_hh_f, b_ih_r, b_hh_r)
        ctx.save_for_backward(xc, w_ih_f, w_hh_f, w_ih_r, w_hh_r, G, C, Y, w_stack)
        ctx.consumed = False
        out = Y2 if mode else Y.view(T, B, ndir * H)
        if _panel_state["handover"] is not None:         # a panel nobody came for
            _panel_state["handover"][2].release()
            _panel_state["handover"] = None
        if out_panel is not None:
            _panel_state["handover"] = (_weakref.ref(out), out._version, out_panel)
        return out

    @staticmethod
    def backward(ctx, dY):
        L = _L()
        xc, w_ih_f, w_hh_f, w_ih_r, w_hh_r, G, C, Y, w_stack = ctx.saved_tensors
        if ctx.consumed:
            raise RuntimeError("LSTMLayerFn: backward twice (the gate buffer is reused in place)")
        ctx.consumed = True
        T, B, Din, H, ndir = ctx.dims
        dev = dY.device
        M = T * B
        ldg, ldy = ndir * 4 * H, ndir * H
        mode, rate = ctx.pyr
        dYc = _f32c(dY)        # plain: [T,B,ldy]; fused time reduction: the reduced layout, read in place
        ws = lstm_workspace(dev)
        needs_dx = ctx.needs_input_grad[0]
        w_ih, w_hh = (w_ih_f, w_ih_r), (w_hh_f, w_hh_r)
        # G (activated gates) -> dG (pre-activation gradients), in place.  The facts are gathered inside the frame:
        # _defer_beside_bptt() answers for the BPTT plan that _bptt_launch has just noted.
        with _bptt_launch(L, T, B, H, ndir, ctx.has_bias, G, dev) as (xc_, db_all):
            plan = lstm_bwd_plan(T, B, Din, H, ndir, ctx.has_bias, needs_dx, w_stack is not None,
                                 _can_defer(w_ih_f, w_hh_f, w_ih_r, w_hh_r, *ctx.bias_refs),
                                 not grad_has_destination(*w_ih[:ndir]), _defer_beside_bptt(),
                                 bool(_REC_PANELS and L.asrk_lstm_plan_is_bf(T, B, H, ndir, 1, rec_flags(1))),
                                 _os.environ.get("ASRK_SHARE_PANELS", "1") != "0", _REC_SKIP_DG, gemm_takes_split,
                                 lambda rows, K: _BlankPanel.take(rows, K, dev))
            pG, pGT = plan.pG, plan.pGT
            stats = _panel_state["stats"]
            stats["dg"] += pG is not None
            stats["dgt"] += pGT is not None
            stats["no_dg"] += plan.skip_dg
            stats["dw_ih_splitk"] += (plan.dw_ih_route == IH_SPLITK) * (1 if plan.rows_ih == 8 * H else ndir)
            db = db_all if plan.db_in_kernel else None
            if pG is not None or pGT is not None:
                _lib.check(L.asrk_lstm_rec_bwd_pyr_panel_f32(_p(G), _p(w_hh_f), _p(w_hh_r), _p(C), _p(dYc), T, B, H,
                                                             ndir, _p(xc_.buf), xc_.prefilled, _p(ws), _p(db), mode, rate,
                                                             _p(pG.buf if pG is not None else None),
                                                             _p(pGT.buf if pGT is not None else None),
                                                             xc_.flags | (ASRK_REC_BWD_NO_DG if plan.skip_dg else 0),
                                                             _stream()), "lstm_rec_bwd")
            else:
                _lib.check(L.asrk_lstm_rec_bwd_pyr_f32(_p(G), _p(w_hh_f), _p(w_hh_r), _p(C), _p(dYc), T, B, H,
                                                       ndir, _p(xc_.buf), xc_.prefilled, _p(ws), _p(db), mode, rate,
                                                       xc_.flags, _stream()), "lstm_rec_bwd")
        dG = G
        f32 = dict(dtype=torch.float32, device=dev)
        dx = None
        if needs_dx:
            dx = torch.empty((M, Din), **f32)
            if pG is not None:            # dG arrived as a panel: only the (transposed) weight stack is split here
                pWT = SplitPanel(w_stack, Din, Din, 8 * H, True)
                gemm_panels(M, Din, 8 * H, pG, 0, 0, pWT, 0, 0, dx, Din)
                del pWT
                pG.release()
            elif w_stack is not None:     # one contraction over both directions' gate gradients (K = 8H)
                gemm(0, 0, M, Din, 8 * H, dG, ldg, w_stack, Din, dx, Din)
            else:
                gemm(0, 0, M, Din, 4 * H, dG, ldg, w_ih_f, Din, dx, Din)
                if ndir == 2:
                    gemm(0, 0, M, Din, 4 * H, dG[:, 4 * H:], ldg, w_ih_r, Din, dx, Din, beta=1.0)
            dx = dx.view(T, B, Din)
        panels = {} if pGT is None else {"dGT": pGT}      # written by the BPTT kernel: no transposed split pass over dG
        dw_ih_stack = []         # the stacked dW_ih [8H, Din]: one launch, on the stream of the direction that runs first

        def panel(name, src, ld, rows):
            if name not in panels:
                panels[name] = SplitPanel(src, ld, rows, M, True)
            return panels[name]

        def dg_gemm(Mo, No, Ko, m0, k0, pB, b_row0, b_k0, out, ldo, splitk=None):
            """out[Mo, No] = dG[k0 : k0 + Ko, m0 : m0 + Mo]^T  B-panel rows, through the transposed panel dG^T"""
            gemm_panels(Mo, No, Ko, panel("dGT", dG, ldg, ldg), m0, k0, pB, b_row0, b_k0, out, ldo, splitk=splitk)

        def dw_ih_of(d):
            stacked = plan.rows_ih == 8 * H
            if not (stacked and dw_ih_stack):
                out = torch.empty((8 * H, Din), **f32) if stacked else grad_out(w_ih[d], (4 * H, Din), dev)
                m0 = 0 if stacked else d * 4 * H
                if plan.dw_ih_route == IH_F32:
                    gemm(1, 0, plan.rows_ih, Din, M, dG[:, m0:], ldg, xc, Din, out, Din)
                else:                     # splitk = 0: K cut into slices summed in a fixed order, their count by the library
                    dg_gemm(plan.rows_ih, Din, M, m0, 0, panel("XT", xc, Din, Din), 0, 0, out, Din,
                            0 if plan.dw_ih_route == IH_SPLITK else None)
                if not stacked:
                    return out
                dw_ih_stack.append(out)
            return dw_ih_stack[0][d * 4 * H:(d + 1) * 4 * H]

        def dw_hh_of(d):
            if T <= 1:
                return zeros((4 * H, H), dev)
            out, Mh = grad_out(w_hh[d], (4 * H, H), dev), (T - 1) * B
            # direction 0: dG rows of t >= 1 against h_{t-1} = Y[t-1]; direction 1 (reverse): rows of t <= T-2 against Y[t+1]
            if plan.dw_hh_panels:
                dg_gemm(4 * H, H, Mh, d * 4 * H, B if d == 0 else 0, panel("YT", Y, ldy, ldy), d * H, 0 if d == 0 else B,
                        out, H)
            elif d == 0:
                gemm(1, 0, 4 * H, H, Mh, dG[B:], ldg, Y, ldy, out, H)
            else:
                gemm(1, 0, 4 * H, H, Mh, dG[:, 4 * H:], ldg, Y[B:, H:], ldy, out, H)
            return out

        def param_grads(d):
            # launch order: where dW_hh multiplies panels it goes first (Y^T and dG^T are split before X^T)
            if plan.dw_hh_panels:
                dw_hh = dw_hh_of(d)
                dw_ih = dw_ih_of(d)
            else:
                dw_ih = dw_ih_of(d)
                dw_hh = dw_hh_of(d)
            db = db2 = None
            if ctx.has_bias:
                db = db_all[d]
                db2 = db.clone()
            return dw_ih, dw_hh, db, db2

        if plan.schedule == STREAM:
            grads = [param_grads(d) for d in range(ndir)]
        elif plan.schedule == SIDE_ALL:
            with _SideStream(dev, (dG, xc, Y, db_all)) as side:
                grads = [param_grads(d) for d in range(ndir)]
                side.keep(*[t for g in grads for t in g])
        else:
            inputs = (dG, xc, Y, db_all)
            if plan.schedule == SIDE_REVERSE_SHARED:
                inputs += (pGT.buf, panel("YT", Y, ldy, ldy).buf)         # Y^T: split here, before the streams fork
            with _SideStream(dev, inputs, background=False) as side:
                g1 = param_grads(1)
                side.keep(*g1)
            grads = [param_grads(0), g1]
        if pGT is not None:
            if plan.defer_release or _defer["pending"]:
                _defer["release"].append(pGT)     # side-stream GEMMs may still read it: back at the end of the backward pass
            else:
                pGT.release()                     # every consumer was enqueued on this stream
        if ndir == 1:
            grads.append((None, None, None, None))
        return (dx,) + grads[0] + grads[1] + (None, None)


class Copy3dFn(Function):
    """Differentiable strided block copy into a zero-filled tensor of `out_shape` (zero padding /
    slicing without ATen math): dst[i0*ds0 + i1*ds1 + e] = src[i0*ss0 + i1*ss1 + e]."""

    @staticmethod
    def forward(ctx, src, out_shape, n0, n1, n2, ss0, ss1, ds0, ds1):
        _require_gpu(src)
        s = _f32c(src)
        dst = zeros(out_shape, src.device)
        copy3d(s, dst, n0, n1, n2, ss0, ss1, ds0, ds1)
        ctx.meta = (tuple(src.shape), n0, n1, n2, ss0, ss1, ds0, ds1)
        return dst

    @staticmethod
    def backward(ctx, g):
        shape, n0, n1, n2, ss0, ss1, ds0, ds1 = ctx.meta
        gs = zeros(shape, g.device)
        copy3d(_f32c(g), gs, n0, n1, n2, ds0, ds1, ss0, ss1)
        return (gs,) + (None,) * 8


def _pad_lstm_params(params, H, Hp):
    """nn.LSTM-layout (w_ih [4H,Din], w_hh [4H,H], b_ih, b_hh) -> the same with H zero-padded to Hp
    per gate.  Padded units see pre-activation 0 and zero initial state:
    c stays 0 and h = o * tanh(0) = 0 at every step, and their W_hh columns are zero, so the real
    units are untouched — exact, not approximate."""
    w_ih, w_hh, b_ih, b_hh = params
    Din = w_ih.shape[1]
    w_ih_p = Copy3dFn.apply(w_ih, (4 * Hp, Din), 4, H, Din, H * Din, Din, Hp * Din, Din)
    w_hh_p = Copy3dFn.apply(w_hh, (4 * Hp, Hp), 4, H, H, H * H, H, Hp * Hp, Hp)
    b_ih_p = Copy3dFn.apply(b_ih, (4 * Hp,), 1, 4, H, 0, H, 0, Hp)
    b_hh_p = Copy3dFn.apply(b_hh, (4 * Hp,), 1, 4, H, 0, H, 0, Hp)
    return w_ih_p, w_hh_p, b_ih_p, b_hh_p


def lstm_layer(x_tm, params_f, params_r=None, pyramid=None):
    """params_* = (w_ih, w_hh, b_ih, b_hh) in torch nn.LSTM layout.  pyramid = (rate, style): also
    apply the time reduction of src/module.py:141-153 (fused into the kernel when the shape allows)."""
    H = params_f[1].shape[1]
    if pyramid is not None and pyramid[0] > 1:
        if H % 4 != 0 or _os.environ.get("ASRK_FUSE_PYRAMID", "1") == "0":
            return PyramidFn.apply(lstm_layer(x_tm, params_f, params_r), pyramid[0], pyramid[1])
        pr = params_r if params_r is not None else (None, None, None, None)
        return LSTMLayerFn.apply(x_tm, *params_f, *pr, pyramid[0], pyramid[1])
    if H % 4 != 0:
        # the persistent recurrence kernels want H % 4 == 0 (16-B h rows): run on zero-padded units
        Hp = (H + 3) // 4 * 4
        ndir = 2 if params_r is not None else 1
        pf = _pad_lstm_params(params_f, H, Hp)
        pr = _pad_lstm_params(params_r, H, Hp) if params_r is not None else (None,) * 4
        T, B = x_tm.shape[0], x_tm.shape[1]
        yp = LSTMLayerFn.apply(x_tm, *pf, *pr)                               # [T,B,ndir*Hp]
        return Copy3dFn.apply(yp, (T, B, ndir * H), T * B, ndir, H, ndir * Hp, Hp, ndir * H, H)
    pr = params_r if params_r is not None else (None, None, None, None)
    return LSTMLayerFn.apply(x_tm, *params_f, *pr)


def lstm_layer_packed(x_tm, params_f, params_r, lens, pyramid=None):
    """Inference-only (bi)LSTM layer over a zero-padded time-major batch [T,B,Din] in which row b is a sequence of
    lens[b] frames: every row is computed exactly as if it had been run ALONE and unpadded (the reverse direction starts
    at its own last frame) - the reference decodes utterance by utterance (src/decode.py:64,88; bin/test_asr.py:163-167),
    this is what lets several utterances share one encoder pass.  Output frames t >= lens[b] are zero.  pyramid =
    (rate, style) fuses the time reduction ('concat' trims lens[b] % rate frames of every row by itself).
    Returns the layer output [T',B,D']; the caller divides the lengths."""
    _require_gpu(x_tm)
    if torch.is_grad_enabled() and x_tm.requires_grad:
        raise _lib.AsrkError("lstm_layer_packed is inference-only")
    L = _L()
    xc = _f32c(x_tm)
    T, B, Din = xc.shape
    w_ih_f, w_hh_f, b_ih_f, b_hh_f = (None if t is None else _f32c(t.detach()) for t in params_f)
    H = w_hh_f.shape[1]
    if H % 4 != 0:
        raise _lib.AsrkError("lstm_layer_packed: hidden size must be a multiple of 4")
    ndir = 2 if params_r is not None else 1
    dev = xc.device
    M = T * B
    G = torch.empty((M, ndir * 4 * H), dtype=torch.float32, device=dev)
    gemm(0, 1, M, 4 * H, Din, xc, Din, w_ih_f, Din, G, ndir * 4 * H, bias=b_ih_f, bias2=b_hh_f)
    w_hh_r = None
    if ndir == 2:
        w_ih_r, w_hh_r, b_ih_r, b_hh_r = (None if t is None else _f32c(t.detach()) for t in params_r)
        gemm(0, 1, M, 4 * H, Din, xc, Din, w_ih_r, Din, G[:, 4 * H:], ndir * 4 * H, bias=b_ih_r, bias2=b_hh_r)
    lens_d = torch.as_tensor(lens).to(device=dev, dtype=torch.int64).contiguous()
    Y = zeros((M, ndir * H), dev)
    C = torch.empty((M, ndir * H), dtype=torch.float32, device=dev)
    rate, style = pyramid if pyramid is not None else (1, None)
    mode, Y2 = _pyramid_out(T, B, ndir * H, rate, style, dev, zero=True)
    ws = lstm_workspace(dev)
    xc_ = _Exchange(L, T, B, H, ndir, 0, dev)
    _lib.check(L.asrk_lstm_rec_fwd_len_f32(_p(G), _p(w_hh_f), _p(w_hh_r), _p(Y), _p(C), _p(lens_d), T, B, H, ndir,
                                           _p(xc_.buf), xc_.prefilled, _p(ws), _p(Y2), mode, max(1, rate), xc_.flags,
                                           _stream()), "lstm_rec_fwd_len")
    xc_.done()
    return Y2 if mode else Y.view(T, B, ndir * H)


# --------------------------------------------------------------------------- CTC loss
CTC_ZERO_INFINITY = 1      # ASRK_CTC_ZERO_INFINITY (include/asrk.h)


class CTCLossFn(Function):
    """torch.nn.CTCLoss(blank, reduction='mean') (reference: bin/train_asr.py:49,123-124).  zero_infinity=True: an
    utterance with no path through its frames (nll = +inf) contributes loss 0 and an all-zero gradient; 'mean' still
    divides by all B utterances.  `count_out`: optional int32 device scalar that receives the number zeroed.
    zero_infinity=False: its loss is +inf and its gradient is not finite - NaN in the columns of its labels and of the
    blank for t < input_length, exp(log_probs) * scale in the other columns (torch makes those NaN too), 0 beyond.
    A target outside [0,V) (torch raises): loss NaN, gradient NaN for t < input_length and 0 beyond, with either setting.
    Lengths are clamped as the kernels clamp them, input_lengths to T and target_lengths to targets.shape[1], the
    'mean' divisor included.  The gradient comes back in the layout of log_probs: backed by a [B,T,V] tensor where
    log_probs is the transposed view of one, a contiguous [T,B,V] otherwise."""

    @staticmethod
    def forward(ctx, log_probs, targets, input_lengths, target_lengths, blank, reduction, zero_infinity=False,
                count_out=None):
        _require_gpu(log_probs)
        L = _L()
        if log_probs.dtype != torch.float32:
            log_probs = log_probs.float()
        if log_probs.stride(2) != 1:
            log_probs = log_probs.contiguous()
        T, B, V = log_probs.shape
        dev = log_probs.device
        targets = torch.as_tensor(targets).to(device=dev, dtype=torch.int64)
        if targets.dim() != 2:
            raise _lib.AsrkError("CTCLoss: only padded 2-D targets [B, L] are supported "
                                 "(reference passes txt [B,L], bin/train_asr.py:123)")
        targets = targets.contiguous()
        il = torch.as_tensor(input_lengths).to(device=dev, dtype=torch.int64).contiguous()
        tl = torch.as_tensor(target_lengths).to(device=dev, dtype=torch.int64).contiguous()
        Lmax = targets.shape[1]
        S = 2 * Lmax + 1
        alpha = torch.empty((B, T, S), dtype=torch.float32, device=dev)
        lpg = torch.empty((B, T, S), dtype=torch.float32, device=dev)
        # training: the beta lattice runs concurrently with alpha in the same launch
        beta = torch.empty((B, T, S), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        nll = torch.empty((B,), dtype=torch.float32, device=dev)
        if zero_infinity:
            # nll keeps +inf as the marker for the backward; `loss` is what the caller sees
            loss = torch.empty((B,), dtype=torch.float32, device=dev)
            if count_out is not None and B == 0:
                count_out.zero_()
            _lib.check(L.asrk_ctc_loss_fwd_ex_f32(_p(log_probs), log_probs.stride(0), log_probs.stride(1), T,
                                                  B, V, _p(targets), targets.stride(0), Lmax, _p(il),
                                                  _p(tl), blank, _p(alpha), _p(beta), _p(lpg), _p(nll),
                                                  CTC_ZERO_INFINITY, _p(loss), _p(count_out), _stream()), "ctc_fwd")
        else:
            loss = nll
            _lib.check(L.asrk_ctc_loss_fwd_f32(_p(log_probs), log_probs.stride(0), log_probs.stride(1), T,
                                               B, V, _p(targets), targets.stride(0), Lmax, _p(il),
                                               _p(tl), blank, _p(alpha), _p(beta), _p(lpg), _p(nll),
                                               _stream()), "ctc_fwd")
        ctx.save_for_backward(log_probs, targets, il, tl, alpha, beta, lpg, nll)
        ctx.meta = (T, B, V, Lmax, blank, reduction, bool(zero_infinity))
        if reduction == "mean":
            return (loss / tl.clamp(min=1, max=max(Lmax, 1)).to(torch.float32)).mean()
        if reduction == "sum":
            return loss.sum()
        return loss

    @staticmethod
    def backward(ctx, gout):
        L = _L()
        log_probs, targets, il, tl, alpha, beta, lpg, nll = ctx.saved_tensors
        T, B, V, Lmax, blank, reduction, zero_infinity = ctx.meta
        dev = log_probs.device
        if reduction == "mean":
            gscale = gout.to(torch.float32) / (tl.clamp(min=1, max=max(Lmax, 1)).to(torch.float32) * B)
        elif reduction == "sum":
            gscale = gout.to(torch.float32).expand(B)
        else:
            gscale = gout.to(torch.float32)
        gscale = gscale.contiguous()
        # the gradient takes the memory layout of the input: the solver passes ctc_output.transpose(0, 1)
        # (a [T,B,V] view of a [B,T,V] tensor), so autograd's transpose-back is then a free view and the
        # log-softmax backward reads a contiguous tensor (no 160 MB re-layout copy)
        if log_probs.stride(1) > log_probs.stride(0):
            grad = torch.empty((B, T, V), dtype=torch.float32, device=dev).transpose(0, 1)
        else:
            grad = torch.empty((T, B, V), dtype=torch.float32, device=dev)
        if zero_infinity:
            _lib.check(L.asrk_ctc_loss_bwd_ex_f32(_p(log_probs), log_probs.stride(0), log_probs.stride(1), T,
                                                  B, V, _p(targets), targets.stride(0), Lmax, _p(il),
                                                  _p(tl), blank, _p(alpha), _p(beta), _p(lpg), _p(nll), _p(gscale),
                                                  _p(grad), grad.stride(0), grad.stride(1), CTC_ZERO_INFINITY,
                                                  _stream()), "ctc_bwd")
        else:
            _lib.check(L.asrk_ctc_loss_bwd_f32(_p(log_probs), log_probs.stride(0), log_probs.stride(1), T,
                                               B, V, _p(targets), targets.stride(0), Lmax, _p(il),
                                               _p(tl), blank, _p(alpha), _p(beta), _p(lpg), _p(nll), _p(gscale),
                                               _p(grad), grad.stride(0), grad.stride(1), _stream()),
                       "ctc_bwd")
        return grad, None, None, None, None, None, None, None


class CTCLoss(torch.nn.Module):
    """Drop-in for torch.nn.CTCLoss(blank=0, zero_infinity=...) on the MI355X path.  After a forward with
    zero_infinity=True, `n_infeasible` is an int32 device scalar: the number of utterances whose loss was zeroed
    (reading it is the caller's synchronisation, the forward does none)."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super().__init__()
        if reduction not in ("none", "mean", "sum"):
            raise ValueError("CTCLoss: unknown reduction %r" % (reduction,))
        self.blank = blank
        self.reduction = reduction
        self.zero_infinity = bool(zero_infinity)
        self.n_infeasible = None

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        if not self.zero_infinity:
            return CTCLossFn.apply(log_probs, targets, input_lengths, target_lengths, self.blank,
                                   self.reduction)
        _require_gpu(log_probs)
        self.n_infeasible = torch.empty((), dtype=torch.int32, device=log_probs.device)
        return CTCLossFn.apply(log_probs, targets, input_lengths, target_lengths, self.blank,
                               self.reduction, True, self.n_infeasible)


# --------------------------------------------------------------------------- CTC forced alignment
ALIGN_BP_AUTO, ALIGN_BP_LDS, ALIGN_BP_GLOBAL = 0, 1, 2      # ASRK_ALIGN_BP_* (include/asrk.h), per call

CTCAlignment = collections.namedtuple("CTCAlignment", ["states", "tokens", "spans", "score"])


@torch.no_grad()
def ctc_align(log_probs, targets, input_lengths, target_lengths, blank=0, flags=ALIGN_BP_AUTO, stamps=None):
    """Best CTC path of every utterance (asrk_ctc_align_f32): log_probs [T,B,V] (any (stride_t, stride_b), e.g. the
    transposed view of a [B,T,V] tensor), targets [B,L] padded, lengths [B] -> CTCAlignment of device tensors:
    states / tokens int32 [B,T] (-1 beyond an utterance's frames), spans int32 [B,L,2] (first frame, last frame + 1 of
    every target token; -1 beyond its targets), score f32 [B] (log-probability of the path; -inf and -1 everywhere
    when the target does not fit the frames).  `flags`: where the backpointers live (ALIGN_BP_*).  `stamps`: optional
    int64 [B,4] device tensor that receives the kernel's phase clocks."""
    _require_gpu(log_probs)
    L = _L()
    if log_probs.dim() != 3:
        raise _lib.AsrkError("ctc_align: log_probs must be [T, B, V]")
    if log_probs.dtype != torch.float32:
        log_probs = log_probs.float()
    if log_probs.stride(2) != 1:
        log_probs = log_probs.contiguous()
    T, B, V = log_probs.shape
    dev = log_probs.device
    targets = torch.as_tensor(targets).to(device=dev, dtype=torch.int64)
    if targets.dim() != 2:
        raise _lib.AsrkError("ctc_align: only padded 2-D targets [B, L] are supported")
    targets = targets.contiguous()
    il = torch.as_tensor(input_lengths).to(device=dev, dtype=torch.int64).contiguous()
    tl = torch.as_tensor(target_lengths).to(device=dev, dtype=torch.int64).contiguous()
    if targets.shape[0] != B or il.numel() != B or tl.numel() != B:
        raise _lib.AsrkError("ctc_align: targets / lengths do not match the batch of log_probs")
    Lmax = targets.shape[1]
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    spans = torch.empty((B, Lmax, 2), dtype=torch.int32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    need = L.asrk_ctc_align_ws_bytes(B, T, Lmax, flags)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
    _lib.check(L.asrk_ctc_align_f32(_p(log_probs), log_probs.stride(0), log_probs.stride(1), T, B, V, _p(targets),
                                    targets.stride(0), Lmax, _p(il), _p(tl), blank, flags, _p(states), _p(tokens),
                                    _p(spans), _p(score), _p(stamps), _p(ws), need, _stream()), "ctc_align")
    return CTCAlignment(states, tokens, spans, score)


# --------------------------------------------------------------------------- second-pass scoring (inference only)
SEQ_LOGP_NORMALIZED = 1      # ASRK_SEQ_LOGP_NORMALIZED (include/asrk.h)


@torch.no_grad()
def seq_logp(x, target, seg_off=None, normalized=False):
    """Log-probability of target[m] under row m of the logits x [M, V] (asrk_seq_logp_f32: no [M, V] log_softmax is
    written) -> (tok_logp f32 [M], seq_logp f64 [R] or None).  A row with target < 0 is skipped (0, never read);
    target >= V gives NaN.  `seg_off` [R+1]: seq_logp[r] = the float64 sum of tok_logp[seg_off[r]:seg_off[r+1]], added
    in ascending order.  `normalized`: x already holds log-probabilities, the value is gathered as it is.  x may be
    a row-strided view (stride(1) == 1)."""
    _require_gpu(x)
    L = _L()
    if x.dim() != 2:
        raise _lib.AsrkError("seq_logp: x must be [M, V]")
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    M, V = x.shape
    dev = x.device
    ldx = x.stride(0) if M > 1 else max(x.stride(0), V)
    target = torch.as_tensor(target).to(device=dev, dtype=torch.int64).contiguous()
    if target.numel() != M:
        raise _lib.AsrkError("seq_logp: one target per row of x")
    tok = torch.empty((M,), dtype=torch.float32, device=dev)
    seq, R = None, 0
    if seg_off is not None:
        seg_off = torch.as_tensor(seg_off).to(device=dev, dtype=torch.int64).contiguous()
        if seg_off.dim() != 1 or seg_off.numel() < 1:
            raise _lib.AsrkError("seq_logp: seg_off must be [R + 1]")
        R = seg_off.numel() - 1
        seq = torch.empty((R,), dtype=torch.float64, device=dev)
    _lib.check(L.asrk_seq_logp_f32(_p(x), ldx, _p(target), _p(seg_off), M, V, R,
                                   SEQ_LOGP_NORMALIZED if normalized else 0, _p(tok), _p(seq), _stream()), "seq_logp")
    return tok, seq


@torch.no_grad()
def ctc_score_rows(lp, mem_len, row_mem, targets, tgt_len, blank=0):
    """log p_ctc of R hypotheses against the posteriors of U utterances (asrk_ctc_score_rows_f32): lp [U, Tmax, V]
    log-probabilities, mem_len [U] frames of every utterance (frames beyond are never read), row r scores
    targets[r, :tgt_len[r]] against utterance row_mem[r] -> score f32 [R] (-inf: no path; NaN: a label or a row_mem out
    of range)."""
    _require_gpu(lp)
    L = _L()
    if lp.dim() != 3:
        raise _lib.AsrkError("ctc_score_rows: lp must be [U, Tmax, V]")
    if lp.dtype != torch.float32:
        lp = lp.float()
    if lp.stride(2) != 1:
        lp = lp.contiguous()
    U, Tmax, V = lp.shape
    dev = lp.device
    targets = torch.as_tensor(targets).to(device=dev, dtype=torch.int64)
    if targets.dim() != 2:
        raise _lib.AsrkError("ctc_score_rows: only padded 2-D targets [R, L] are supported")
    targets = targets.contiguous()
    ml = torch.as_tensor(mem_len).to(device=dev, dtype=torch.int64).contiguous()
    rm = torch.as_tensor(row_mem).to(device=dev, dtype=torch.int64).contiguous()
    tl = torch.as_tensor(tgt_len).to(device=dev, dtype=torch.int64).contiguous()
    R, Lmax = targets.shape
    if ml.numel() != U or rm.numel() != R or tl.numel() != R:
        raise _lib.AsrkError("ctc_score_rows: lengths / row_mem do not match lp and targets")
    score = torch.empty((R,), dtype=torch.float32, device=dev)
    need = L.asrk_ctc_score_rows_ws_bytes(R, Tmax, Lmax)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
    _lib.check(L.asrk_ctc_score_rows_f32(_p(lp), lp.stride(0), lp.stride(1), U, Tmax, V, _p(ml), _p(rm), _p(targets),
                                         max(targets.stride(0), Lmax), Lmax, _p(tl), R, blank, _p(score), _p(ws), need,
                                         _stream()), "ctc_score_rows")
    return score


# --------------------------------------------------------------------------- MWER training (csrc/mwer.hip)
class SeqLogpFn(Function):
    """seq_logp with a gradient: SeqLogpFn.apply(logits [M,V], target [M], seg_off [R+1], inplace=False) -> seq f64 [R]
    (asrk_seq_logp_lse_f32: ops.seq_logp's values bit for bit).  The backward is asrk_seq_logp_bwd_f32; with
    inplace=True it writes the gradient over the saved logits - only for a caller whose logits have no other reader
    (the MWER scoring pass)."""

    @staticmethod
    def forward(ctx, logits, target, seg_off, inplace=False):
        _require_gpu(logits)
        if logits.dim() != 2:
            raise _lib.AsrkError("SeqLogpFn: logits must be [M, V]")
        x = _f32c(logits)
        M, V = x.shape
        dev = x.device
        tg = torch.as_tensor(target).to(device=dev, dtype=torch.int64).contiguous()
        seg = torch.as_tensor(seg_off).to(device=dev, dtype=torch.int64).contiguous()
        if tg.numel() != M:
            raise _lib.AsrkError("SeqLogpFn: one target per row of the logits")
        if seg.dim() != 1 or seg.numel() < 1:
            raise _lib.AsrkError("SeqLogpFn: seg_off must be [R + 1]")
        R = seg.numel() - 1
        tok = torch.empty((M,), dtype=torch.float32, device=dev)
        lse = torch.empty((M,), dtype=torch.float32, device=dev)
        seq = torch.empty((R,), dtype=torch.float64, device=dev)
        _lib.check(_L().asrk_seq_logp_lse_f32(_p(x), V, _p(tg), _p(seg), M, V, R, 0, _p(tok), _p(lse), _p(seq),
                                              _stream()), "seq_logp_lse")
        ctx.inplace = bool(inplace)
        ctx.save_for_backward(x, tg, seg, lse)
        return seq

    @staticmethod
    def backward(ctx, gseq):
        x, tg, seg, lse = ctx.saved_tensors
        M, V = x.shape
        R = seg.numel() - 1
        g = gseq.to(torch.float64).contiguous()
        dx = x if ctx.inplace else torch.empty_like(x)
        _lib.check(_L().asrk_seq_logp_bwd_f32(_p(x), V, _p(tg), _p(lse), _p(seg), _p(g), M, V, R, _p(dx), V,
                                              _stream()), "seq_logp_bwd")
        return dx, None, None, None


class MWERLossFn(Function):
    """MWERLossFn.apply(s f64 [N,U], err int32 [N,U], count int32 [U]) -> (loss_u f64 [U], exp_err_u f64 [U]),
    differentiable in s through loss_u (asrk_mwer_loss_f64: the closed-form derivative comes out of the forward
    launch); exp_err_u is a statistic and carries no gradient."""

    @staticmethod
    def forward(ctx, s, err, count):
        _require_gpu(s)
        if s.dim() != 2:
            raise _lib.AsrkError("MWERLossFn: s must be [N, U]")
        N, U = s.shape
        dev = s.device
        s64 = s.to(torch.float64).contiguous()
        err = torch.as_tensor(err).to(device=dev, dtype=torch.int32).contiguous()
        count = torch.as_tensor(count).to(device=dev, dtype=torch.int32).contiguous()
        if err.numel() != N * U or count.numel() != U:
            raise _lib.AsrkError("MWERLossFn: err must be [N, U] and count [U]")
        loss = torch.empty((U,), dtype=torch.float64, device=dev)
        ee = torch.empty((U,), dtype=torch.float64, device=dev)
        g = torch.empty((N, U), dtype=torch.float64, device=dev)
        _lib.check(_L().asrk_mwer_loss_f64(_p(s64), _p(err), _p(count), N, U, _p(loss), _p(ee), _p(g), _stream()),
                   "mwer_loss")
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(ee)
        return loss, ee

    @staticmethod
    def backward(ctx, gloss, _gee):
        g, = ctx.saved_tensors
        return g * gloss.to(torch.float64).unsqueeze(0), None, None


# --------------------------------------------------------------------------- RNN-transducer (csrc/rnnt.hip)
class RNNTLossFn(Function):
    """RNNTLossFn.apply(logits [B,T,U+1,V], targets [B,L], enc_len [B], txt_len [B], blank, reduction,
    consume_logits=False): the transducer loss (Graves 2012) on unnormalised joint logits.  The forward reads the logits
    once (asrk_rnnt_rows_f32) and runs the lattice; it saves lse, the blank / label log-probabilities, alpha, beta and
    nll, never a [.., V] log_softmax.  The backward reads them once more and writes the closed-form gradient
    (asrk_rnnt_grad_f32); with consume_logits=True it writes over the logits' own storage and returns that tensor: the
    logits are dead afterwards, so only a caller whose logits have no other reader may ask for it."""

    @staticmethod
    def forward(ctx, logits, targets, enc_len, txt_len, blank=0, reduction="mean", consume_logits=False):
        _require_gpu(logits)
        if logits.dim() != 4:
            raise _lib.AsrkError("RNNTLoss: logits must be [B, T, U + 1, V]")
        x = _f32c(logits)
        B, T, U1, V = x.shape
        dev = x.device
        txt = torch.as_tensor(targets).to(device=dev, dtype=torch.int64)
        if txt.dim() != 2 or txt.shape[0] != B or txt.shape[1] < U1 - 1:
            raise _lib.AsrkError("RNNTLoss: targets must be [B, L] with L >= U")
        txt = txt.contiguous()
        el = torch.as_tensor(enc_len).to(device=dev, dtype=torch.int64).contiguous()
        tl = torch.as_tensor(txt_len).to(device=dev, dtype=torch.int64).contiguous()
        if el.numel() != B or tl.numel() != B:
            raise _lib.AsrkError("RNNTLoss: one enc_len and one txt_len per utterance")
        L = _L()
        lse = torch.empty((B, T, U1), dtype=torch.float32, device=dev)
        lpb, lpl, alpha = torch.empty_like(lse), torch.empty_like(lse), torch.empty_like(lse)
        beta = torch.empty_like(lse) if ctx.needs_input_grad[0] else None   # alpha alone when no gradient is wanted
        nll = torch.empty((B,), dtype=torch.float32, device=dev)
        _lib.check(L.asrk_rnnt_rows_f32(_p(x), V, _p(txt), txt.shape[1], _p(el), _p(tl), B, T, U1, V, blank, _p(lse),
                                        _p(lpb), _p(lpl), _stream()), "rnnt_rows")
        _lib.check(L.asrk_rnnt_lattice_f32(_p(lpb), _p(lpl), _p(el), _p(tl), B, T, U1, _p(alpha), _p(beta), _p(nll),
                                           _stream()), "rnnt_lattice")
        ctx.save_for_backward(x, txt, el, tl, lse, lpb, lpl, alpha, beta, nll)
        ctx.meta = (blank, reduction, bool(consume_logits))
        if reduction == "mean":
            return nll.mean()
        if reduction == "sum":
            return nll.sum()
        return nll

    @staticmethod
    def backward(ctx, gout):
        x, txt, el, tl, lse, lpb, lpl, alpha, beta, nll = ctx.saved_tensors
        blank, reduction, consume = ctx.meta
        B, T, U1, V = x.shape
        g = gout.to(torch.float32)
        if reduction == "mean":
            gscale = (g / B).expand(B)
        elif reduction == "sum":
            gscale = g.expand(B)
        else:
            gscale = g
        gscale = gscale.contiguous()
        dz = x if consume else torch.empty_like(x)
        _lib.check(_L().asrk_rnnt_grad_f32(_p(x), V, _p(txt), txt.shape[1], _p(el), _p(tl), B, T, U1, V, blank, _p(lse),
                                           _p(lpb), _p(lpl), _p(alpha), _p(beta), _p(nll), _p(gscale), _p(dz), V,
                                           _stream()), "rnnt_grad")
        return dz, None, None, None, None, None, None


class RNNTLoss(torch.nn.Module):
    """Transducer loss on joint logits [B, T, U+1, V] (not log-probabilities: the normalisation happens inside).
    'mean' is the mean over the B utterances of nll_b, not length-normalised.  forward(..., consume_logits=True) lets
    the backward overwrite the logits with their gradient: the logits are dead after backward()."""

    def __init__(self, blank=0, reduction="mean"):
        super().__init__()
        if reduction not in ("none", "mean", "sum"):
            raise ValueError("RNNTLoss: unknown reduction %r" % (reduction,))
        self.blank = blank
        self.reduction = reduction

    def forward(self, logits, targets, enc_len, txt_len, consume_logits=False):
        return RNNTLossFn.apply(logits, targets, enc_len, txt_len, self.blank, self.reduction, consume_logits)


class RNNTJointFn(Function):
    """RNNTJointFn.apply(E [B,T,J], P [B,U+1,J]) -> H [B,T,U+1,J] = tanh(E[b,t] + P[b,u]) (asrk_rnnt_joint_f32); the
    backward sums dH * (1 - H^2) over u into dE and over t into dP (asrk_rnnt_joint_bwd_f32)."""

    @staticmethod
    def forward(ctx, E, P):
        _require_gpu(E)
        E, P = _f32c(E), _f32c(P)
        if E.dim() != 3 or P.dim() != 3 or E.shape[0] != P.shape[0] or E.shape[2] != P.shape[2]:
            raise _lib.AsrkError("RNNTJointFn: E must be [B, T, J] and P [B, U + 1, J]")
        B, T, J = E.shape
        U1 = P.shape[1]
        H = torch.empty((B, T, U1, J), dtype=torch.float32, device=E.device)
        _lib.check(_L().asrk_rnnt_joint_f32(_p(E), J, _p(P), J, None, B, T, U1, J, _p(H), J, _stream()), "rnnt_joint")
        ctx.save_for_backward(H)
        return H

    @staticmethod
    def backward(ctx, dH):
        H, = ctx.saved_tensors
        B, T, U1, J = H.shape
        dH = _f32c(dH)
        dE = torch.empty((B, T, J), dtype=torch.float32, device=H.device)
        dP = torch.empty((B, U1, J), dtype=torch.float32, device=H.device)
        _lib.check(_L().asrk_rnnt_joint_bwd_f32(_p(H), J, _p(dH), J, B, T, U1, J, _p(dE), J, _p(dP), J, _stream()),
                   "rnnt_joint_bwd")
        return dE, dP


@torch.no_grad()
def rnnt_joint_step(E, P, t_idx):
    """the decode form of the joint: tanh(E[b, t_idx[b]] + P[b]) -> [B, J]; E [B,T,J], P [B,J], t_idx int32 [B]
    (clamped to the last frame by the kernel)"""
    _require_gpu(E)
    E, P = _f32c(E), _f32c(P)
    B, T, J = E.shape
    if P.shape != (B, J) or t_idx.dtype != torch.int32 or t_idx.numel() != B:
        raise _lib.AsrkError("rnnt_joint_step: P must be [B, J] and t_idx int32 [B]")
    H = torch.empty((B, J), dtype=torch.float32, device=E.device)
    _lib.check(_L().asrk_rnnt_joint_f32(_p(E), J, _p(P), J, _p(t_idx), B, T, 1, J, _p(H), J, _stream()),
               "rnnt_joint_step")
    return H


@torch.no_grad()
def rnnt_rows(logits, targets, enc_len, txt_len, blank=0, out=None):
    """The row pass alone (asrk_rnnt_rows_f32) on joint logits [B, T, U+1, V] -> (lpb, lpl) f32 [B, T, U+1]: the
    log-probabilities of blank and of the cell's label, zeros outside every lattice.  `out`: (lpb, lpl) contiguous
    [B, T, U+1] tensors (or slices along the batch of larger ones) to write into."""
    _require_gpu(logits)
    if logits.dim() != 4:
        raise _lib.AsrkError("rnnt_rows: logits must be [B, T, U + 1, V]")
    x = _f32c(logits)
    B, T, U1, V = x.shape
    dev = x.device
    txt = torch.as_tensor(targets).to(device=dev, dtype=torch.int64)
    if txt.dim() != 2 or txt.shape[0] != B or txt.shape[1] < U1 - 1:
        raise _lib.AsrkError("rnnt_rows: targets must be [B, L] with L >= U")
    txt = txt.contiguous()
    el = torch.as_tensor(enc_len).to(device=dev, dtype=torch.int64).contiguous()
    tl = torch.as_tensor(txt_len).to(device=dev, dtype=torch.int64).contiguous()
    if el.numel() != B or tl.numel() != B:
        raise _lib.AsrkError("rnnt_rows: one enc_len and one txt_len per utterance")
    if out is None:
        out = (torch.empty((B, T, U1), dtype=torch.float32, device=dev),
               torch.empty((B, T, U1), dtype=torch.float32, device=dev))
    lpb, lpl = out
    for o in out:
        if o.shape != (B, T, U1) or o.dtype != torch.float32 or o.device != dev or not o.is_contiguous():
            raise _lib.AsrkError("rnnt_rows: out must be two contiguous f32 [B, T, U + 1] tensors on the logits' device")
    lse = torch.empty((B, T, U1), dtype=torch.float32, device=dev)
    _lib.check(_L().asrk_rnnt_rows_f32(_p(x), V, _p(txt), txt.shape[1], _p(el), _p(tl), B, T, U1, V, blank, _p(lse),
                                       _p(lpb), _p(lpl), _stream()), "rnnt_rows")
    return lpb, lpl


@torch.no_grad()
def rnnt_lattice(lpb, lpl, enc_len, txt_len):
    """alpha, beta [B, T, U+1] and nll [B] of the transducer lattice (asrk_rnnt_lattice_f32) on the row pass's lpb /
    lpl: what ops.rnnt_align's `lattice` argument takes."""
    _require_gpu(lpb)
    lpb, lpl = _f32c(lpb), _f32c(lpl)
    if lpb.dim() != 3 or lpl.shape != lpb.shape:
        raise _lib.AsrkError("rnnt_lattice: lpb and lpl must be [B, T, U + 1]")
    B, T, U1 = lpb.shape
    dev = lpb.device
    el = torch.as_tensor(enc_len).to(device=dev, dtype=torch.int64).contiguous()
    tl = torch.as_tensor(txt_len).to(device=dev, dtype=torch.int64).contiguous()
    if el.numel() != B or tl.numel() != B:
        raise _lib.AsrkError("rnnt_lattice: one enc_len and one txt_len per utterance")
    alpha, beta = torch.empty_like(lpb), torch.empty_like(lpb)
    nll = torch.empty((B,), dtype=torch.float32, device=dev)
    _lib.check(_L().asrk_rnnt_lattice_f32(_p(lpb), _p(lpl), _p(el), _p(tl), B, T, U1, _p(alpha), _p(beta), _p(nll),
                                          _stream()), "rnnt_lattice")
    return alpha, beta, nll


RNNTAlignment = collections.namedtuple("RNNTAlignment", ["frames", "labels_done", "tok_logp", "tok_post", "score"])


@torch.no_grad()
def rnnt_align(lpb, lpl, enc_len, txt_len, flags=ALIGN_BP_AUTO, lattice=None, stamps=None):
    """Best transducer path of every utterance (asrk_rnnt_align_f32) on the row pass's lpb / lpl f32 [B, T, U+1] ->
    RNNTAlignment of device tensors: frames int32 [B, U] (the encoder frame at which label u + 1 was emitted, -1 beyond
    an utterance's labels), labels_done int32 [B, T] (labels emitted through frame t, -1 beyond its frames), tok_logp
    f32 [B, U] (the label's log-probability at the emitting cell), tok_post f32 [B, U] or None (the posterior of that
    emission, with `lattice` = (alpha, beta, nll) of ops.rnnt_lattice on the same lpb / lpl), score f32 [B] (the
    path's log-probability; -inf, with -1 / 0 everywhere, when the transcript does not fit).  Ties emit as early as
    possible.  `flags`: where the backpointers live (ALIGN_BP_*); the workspace of the global route is allocated
    here.  `stamps`: optional int64 [B, 4] device tensor that receives the kernel's phase clocks."""
    _require_gpu(lpb)
    L = _L()
    if lpb.dim() != 3 or lpl.shape != lpb.shape:
        raise _lib.AsrkError("rnnt_align: lpb and lpl must be [B, T, U + 1]")
    if lpb.dtype != torch.float32 or lpl.dtype != torch.float32:
        raise _lib.AsrkError("rnnt_align: lpb and lpl must be float32")
    if lpl.device != lpb.device:
        raise _lib.AsrkError("rnnt_align: lpb and lpl must be on one device")
    lpb, lpl = lpb.contiguous(), lpl.contiguous()
    B, T, U1 = lpb.shape
    if T < 1 or U1 < 1:
        raise _lib.AsrkError("rnnt_align: T and U + 1 must be at least 1")
    dev = lpb.device
    el = torch.as_tensor(enc_len).to(device=dev, dtype=torch.int64).contiguous()
    tl = torch.as_tensor(txt_len).to(device=dev, dtype=torch.int64).contiguous()
    if el.numel() != B or tl.numel() != B:
        raise _lib.AsrkError("rnnt_align: one enc_len and one txt_len per utterance")
    alpha = beta = nll = None
    if lattice is not None:
        alpha, beta, nll = lattice
        for a in (alpha, beta):
            if a.shape != lpb.shape or a.dtype != torch.float32 or a.device != dev or not a.is_contiguous():
                raise _lib.AsrkError("rnnt_align: lattice alpha / beta must be contiguous f32 [B, T, U + 1] on lpb's device")
        if nll.shape != (B,) or nll.dtype != torch.float32 or nll.device != dev or not nll.is_contiguous():
            raise _lib.AsrkError("rnnt_align: lattice nll must be f32 [B] on lpb's device")
    if stamps is not None and (stamps.shape != (B, 4) or stamps.dtype != torch.int64 or stamps.device != dev
                               or not stamps.is_contiguous()):
        raise _lib.AsrkError("rnnt_align: stamps must be a contiguous int64 [B, 4] tensor on lpb's device")
    frames = torch.empty((B, U1 - 1), dtype=torch.int32, device=dev)
    done = torch.empty((B, T), dtype=torch.int32, device=dev)
    tok_logp = torch.empty((B, U1 - 1), dtype=torch.float32, device=dev)
    tok_post = torch.empty((B, U1 - 1), dtype=torch.float32, device=dev) if lattice is not None else None
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    need = L.asrk_rnnt_align_ws_bytes(B, T, U1, flags)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
    _lib.check(L.asrk_rnnt_align_f32(_p(lpb), _p(lpl), _p(el), _p(tl), B, T, U1, flags, _p(alpha), _p(beta), _p(nll),
                                     _p(frames), _p(done), _p(tok_logp), _p(tok_post), _p(score), _p(stamps), _p(ws),
                                     need, _stream()), "rnnt_align")
    return RNNTAlignment(frames, done, tok_logp, tok_post, score)


RNNTGreedyState = collections.namedtuple("RNNTGreedyState",
                                         ["t_ptr", "n_sym", "n_tok", "tokens", "last_tok", "emit", "done"])


def rnnt_greedy_state(B, max_len, device):
    """the device-resident bookkeeping of the greedy search, at its start: frame 0, nothing emitted, <sos> = 0 last"""
    i32 = lambda: torch.zeros((B,), dtype=torch.int32, device=device)   # noqa: E731
    return RNNTGreedyState(i32(), i32(), i32(), torch.zeros((B, max(max_len, 1)), dtype=torch.int64, device=device),
                           torch.zeros((B,), dtype=torch.int64, device=device), i32(), i32())


@torch.no_grad()
def rnnt_greedy_step(logits, enc_len, T, state, max_symbols, max_len, blank=0):
    """one lock-step iteration (asrk_rnnt_greedy_step_f32) on logits [B, V]: updates `state` in place, reads nothing
    back.  enc_len int64 [B] on the device; T the padded frame count."""
    _require_gpu(logits)
    x = _f32c(logits)
    B, V = x.shape
    s = state
    _lib.check(_L().asrk_rnnt_greedy_step_f32(_p(x), V, _p(enc_len), B, T, V, blank, max_symbols, max_len, _p(s.t_ptr),
                                              _p(s.n_sym), _p(s.n_tok), _p(s.tokens), s.tokens.shape[1],
                                              _p(s.last_tok), _p(s.emit), _p(s.done), _stream()), "rnnt_greedy_step")
    return state


# --------------------------------------------------------------------------- transducer beam search (csrc/rnnt_beam.hip)
RNNT_BEAM_MAX = 32          # RB_MAX_BEAM of csrc/rnnt_beam.inc

RNNTBeamState = collections.namedtuple(
    "RNNTBeamState", ["B", "W", "K", "max_len", "n_live", "t_ptr", "n_sym", "n_tok", "score", "tokens", "fin_n",
                      "fin_len", "fin_score", "fin_tok", "parent", "last_tok", "emit", "sel", "lm_sel", "lse", "lpb",
                      "val", "lab"])


def rnnt_beam_state(B, W, K, max_len, device):
    """the device-resident bookkeeping of the beam search at its start: buffer 0 holds one live hypothesis per utterance
    (empty sequence, frame 0, score 0), the finished lists are empty.  Every state array is double buffered [2, B, ...]."""
    if not (1 <= W <= RNNT_BEAM_MAX and 1 <= K <= W and max_len >= 0):
        raise _lib.AsrkError("rnnt_beam_state: 1 <= K <= W <= %d and max_len >= 0" % RNNT_BEAM_MAX)
    Lc = max(int(max_len), 1)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)   # noqa: E731
    n_live = z((2, B), torch.int32)
    n_live[0].fill_(1)
    return RNNTBeamState(
        B, W, K, int(max_len), n_live, z((2, B, W), torch.int32), z((2, B, W), torch.int32), z((2, B, W), torch.int32),
        z((2, B, W), torch.float64), z((2, B, W, Lc), torch.int32), z((2, B), torch.int32), z((2, B, W), torch.int32),
        z((2, B, W), torch.float64), z((2, B, W, Lc), torch.int32), z((B * W,), torch.int64), z((B * W,), torch.int64),
        z((B * W,), torch.int32), z((B * W,), torch.int64), z((B * W,), torch.int64), z((B * W,), torch.float32),
        z((B * W,), torch.float32), z((B * W, K), torch.float32), z((B * W, K), torch.int32))


@torch.no_grad()
def rnnt_joint_slots(E, P, t_ptr, W):
    """the joint of the beam search: tanh(E[r // W, t_ptr[r]] + P[r]) -> [B*W, J]; E [B,T,J] is not repeated per slot,
    P [B*W, J], t_ptr int32 [B*W] (clamped to the last frame by the kernel)"""
    _require_gpu(E)
    E, P = _f32c(E), _f32c(P)
    B, T, J = E.shape
    if P.shape != (B * W, J) or t_ptr.dtype != torch.int32 or t_ptr.numel() != B * W or not t_ptr.is_contiguous():
        raise _lib.AsrkError("rnnt_joint_slots: P must be [B*W, J] and t_ptr int32 [B*W]")
    H = torch.empty((B * W, J), dtype=torch.float32, device=E.device)
    _lib.check(_L().asrk_rnnt_joint_slots_f32(_p(E), J, _p(P), J, _p(t_ptr), B, T, W, J, _p(H), J, _stream()),
               "rnnt_joint_slots")
    return H


@torch.no_grad()
def rnnt_beam_rows(logits, W, K, lm=None, lm_weight=0.0, n_live=None, blank=0, out=None):
    """row pass of the beam search (asrk_rnnt_beam_rows_f32) on logits [B*W, V] (a row-strided 2-d view is taken as it
    is) and optional LM log-probabilities [B*W, V] -> (lse [B*W], lpb [B*W], val [B*W, K], lab int32 [B*W, K]);
    n_live int32 [B]: rows w >= n_live[b] are not read"""
    _require_gpu(logits)
    x = logits
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        x = _f32c(logits)
    M, V = x.shape
    if M % W:
        raise _lib.AsrkError("rnnt_beam_rows: the logits must hold B*W rows")
    l, ldl = None, 0
    if lm is not None:
        l = lm if (lm.dtype == torch.float32 and lm.dim() == 2 and lm.stride(1) == 1) else _f32c(lm).view(M, -1)
        if l.shape != (M, V):
            raise _lib.AsrkError("rnnt_beam_rows: the LM rows must be [B*W, V]")
        ldl = l.stride(0)
    if n_live is not None and (n_live.dtype != torch.int32 or n_live.numel() != M // W or not n_live.is_contiguous()):
        raise _lib.AsrkError("rnnt_beam_rows: n_live must be int32 [B]")
    if out is None:
        dev = x.device
        out = (torch.empty((M,), dtype=torch.float32, device=dev), torch.empty((M,), dtype=torch.float32, device=dev),
               torch.empty((M, K), dtype=torch.float32, device=dev), torch.empty((M, K), dtype=torch.int32, device=dev))
    lse, lpb, val, lab = out
    _lib.check(_L().asrk_rnnt_beam_rows_f32(_p(x), x.stride(0), _p(l), ldl, float(lm_weight), _p(n_live), M // W, W, V,
                                            K, blank, _p(lse), _p(lpb), _p(val), _p(lab), _stream()), "rnnt_beam_rows")
    return out


@torch.no_grad()
def rnnt_beam_select(state, enc_len, T, max_symbols, cur):
    """one select step (asrk_rnnt_beam_select) on the table state.lpb / val / lab: reads beam buffer `cur`, writes the
    other one and the gather indices; nothing is read back.  enc_len int64 [B] on the device."""
    s = state
    _require_gpu(s.score)
    R, Lc = s.B * s.W, s.tokens.shape[3]
    want = [(s.n_live, torch.int32, (2, s.B)), (s.t_ptr, torch.int32, (2, s.B, s.W)),
            (s.n_sym, torch.int32, (2, s.B, s.W)), (s.n_tok, torch.int32, (2, s.B, s.W)),
            (s.score, torch.float64, (2, s.B, s.W)), (s.tokens, torch.int32, (2, s.B, s.W, Lc)),
            (s.fin_n, torch.int32, (2, s.B)), (s.fin_len, torch.int32, (2, s.B, s.W)),
            (s.fin_score, torch.float64, (2, s.B, s.W)), (s.fin_tok, torch.int32, (2, s.B, s.W, Lc)),
            (s.parent, torch.int64, (R,)), (s.last_tok, torch.int64, (R,)), (s.emit, torch.int32, (R,)),
            (s.sel, torch.int64, (R,)), (s.lm_sel, torch.int64, (R,)), (s.lpb, torch.float32, (R,)),
            (s.val, torch.float32, (R, s.K)), (s.lab, torch.int32, (R, s.K)), (enc_len, torch.int64, (s.B,))]
    for t, dt, shape in want:
        if (not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()
                or t.device != s.score.device):
            raise _lib.AsrkError("rnnt_beam_select: state, table and enc_len must be contiguous device tensors of the "
                                 "shapes and types of rnnt_beam_state (enc_len int64 [B])")
    _lib.check(_L().asrk_rnnt_beam_select(
        _p(s.lpb), _p(s.val), _p(s.lab), _p(enc_len), s.B, T, s.W, s.K, max_symbols, s.max_len, s.tokens.shape[3],
        int(cur), _p(s.n_live), _p(s.t_ptr), _p(s.n_sym), _p(s.n_tok), _p(s.score), _p(s.tokens), _p(s.fin_n),
        _p(s.fin_len), _p(s.fin_score), _p(s.fin_tok), _p(s.parent), _p(s.last_tok), _p(s.emit), _p(s.sel),
        _p(s.lm_sel), _stream()), "rnnt_beam_select")
    return state


# --------------------------------------------------------------------------- pruned transducer training (csrc/rnnt_prune.hip)
RNNT_PRUNE_MAX_RANGE = 32   # PRUNE_MAX_S of csrc/rnnt_prune.hip


def _rnnt_lengths(what, targets, enc_len, txt_len, B, U1, dev):
    txt = torch.as_tensor(targets).to(device=dev, dtype=torch.int64)
    if txt.dim() != 2 or txt.shape[0] != B or txt.shape[1] < U1 - 1:
        raise _lib.AsrkError(what + ": targets must be [B, L] with L >= U")
    el = torch.as_tensor(enc_len).to(device=dev, dtype=torch.int64).contiguous()
    tl = torch.as_tensor(txt_len).to(device=dev, dtype=torch.int64).contiguous()
    if el.numel() != B or tl.numel() != B:
        raise _lib.AsrkError(what + ": one enc_len and one txt_len per utterance")
    return txt.contiguous(), el, tl


def _band_starts(what, s, B, T, dev):
    if not torch.is_tensor(s) or s.dtype != torch.int32 or tuple(s.shape) != (B, T) or s.device != dev:
        raise _lib.AsrkError(what + ": s must be an int32 [B, T] device tensor (ops.rnnt_prune_ranges)")
    return s.contiguous()


class RNNTSimpleLossFn(Function):
    """RNNTSimpleLossFn.apply(am [B,T,V], lm [B,U+1,V], targets [B,L], enc_len [B], txt_len [B], blank=0) ->
    (nll [B], occ [B,T,U+1]): the transducer loss of the additive joiner am[b,t,v] + lm[b,u,v], whose [B,T,U+1,V] sum is
    never stored (asrk_rnnt_simple_rows_f32, the dense lattice, asrk_rnnt_simple_occ_f32), and, detached, the occupation
    occ = eb + el of the arcs leaving every cell, which ops.rnnt_prune_ranges turns into the band.  The backward
    (asrk_rnnt_simple_grad_f32) gives dam and dlm without atomics."""

    @staticmethod
    def forward(ctx, am, lm, targets, enc_len, txt_len, blank=0):
        _require_gpu(am)
        am, lm = _f32c(am), _f32c(lm)
        if am.dim() != 3 or lm.dim() != 3 or am.shape[0] != lm.shape[0] or am.shape[2] != lm.shape[2]:
            raise _lib.AsrkError("RNNTSimpleLossFn: am must be [B, T, V] and lm [B, U + 1, V]")
        B, T, V = am.shape
        U1 = lm.shape[1]
        dev = am.device
        txt, el, tl = _rnnt_lengths("RNNTSimpleLossFn", targets, enc_len, txt_len, B, U1, dev)
        L = _L()
        lse = torch.empty((B, T, U1), dtype=torch.float32, device=dev)
        lpb, lpl, alpha, beta = (torch.empty_like(lse) for _ in range(4))
        c, eb, el_ = (torch.empty_like(lse) for _ in range(3))
        nll = torch.empty((B,), dtype=torch.float32, device=dev)
        _lib.check(L.asrk_rnnt_simple_rows_f32(_p(am), V, _p(lm), V, _p(txt), txt.shape[1], _p(el), _p(tl), B, T, U1, V,
                                               blank, _p(lse), _p(lpb), _p(lpl), _stream()), "rnnt_simple_rows")
        _lib.check(L.asrk_rnnt_lattice_f32(_p(lpb), _p(lpl), _p(el), _p(tl), B, T, U1, _p(alpha), _p(beta), _p(nll),
                                           _stream()), "rnnt_lattice")
        _lib.check(L.asrk_rnnt_simple_occ_f32(_p(lpb), _p(lpl), _p(alpha), _p(beta), _p(nll), _p(el), _p(tl), B, T, U1,
                                              _p(c), _p(eb), _p(el_), _stream()), "rnnt_simple_occ")
        occ = eb + el_
        ctx.save_for_backward(am, lm, txt, el, tl, lse, c, eb, el_)
        ctx.blank = blank
        ctx.mark_non_differentiable(occ)
        return nll, occ

    @staticmethod
    def backward(ctx, gnll, _gocc):
        am, lm, txt, el, tl, lse, c, eb, el_ = ctx.saved_tensors
        B, T, V = am.shape
        U1 = lm.shape[1]
        gscale = gnll.to(torch.float32).contiguous()
        dam, dlm = torch.empty_like(am), torch.empty_like(lm)
        _lib.check(_L().asrk_rnnt_simple_grad_f32(_p(am), V, _p(lm), V, _p(txt), txt.shape[1], _p(el), _p(tl), B, T, U1,
                                                  V, ctx.blank, _p(lse), _p(c), _p(eb), _p(el_), _p(gscale), _p(dam), V,
                                                  _p(dlm), V, _stream()), "rnnt_simple_grad")
        return dam, dlm, None, None, None, None


@torch.no_grad()
def rnnt_prune_ranges(occ, enc_len, txt_len, prune_range):
    """occ [B,T,U+1] (RNNTSimpleLossFn's second result) -> s int32 [B,T], the first of the `prune_range` label positions
    kept at every frame (asrk_rnnt_prune_ranges_f32; the rule: csrc/rnnt_prune.inc)."""
    _require_gpu(occ)
    occ = _f32c(occ)
    S = int(prune_range)
    if occ.dim() != 3 or not 1 <= S <= RNNT_PRUNE_MAX_RANGE:
        raise _lib.AsrkError("rnnt_prune_ranges: occ must be [B, T, U + 1] and 1 <= prune_range <= %d"
                             % RNNT_PRUNE_MAX_RANGE)
    B, T, U1 = occ.shape
    dev = occ.device
    el = torch.as_tensor(enc_len).to(device=dev, dtype=torch.int64).contiguous()
    tl = torch.as_tensor(txt_len).to(device=dev, dtype=torch.int64).contiguous()
    if el.numel() != B or tl.numel() != B:
        raise _lib.AsrkError("rnnt_prune_ranges: one enc_len and one txt_len per utterance")
    s = torch.empty((B, T), dtype=torch.int32, device=dev)
    _lib.check(_L().asrk_rnnt_prune_ranges_f32(_p(occ), _p(el), _p(tl), B, T, U1, S, _p(s), _stream()),
               "rnnt_prune_ranges")
    return s


class RNNTJointBandFn(Function):
    """RNNTJointBandFn.apply(E [B,T,J], P [B,U+1,J], s int32 [B,T], S) -> H [B,T,S,J] = tanh(E[b,t] + P[b, min(s[b,t] + k,
    U)]) (asrk_rnnt_joint_band_f32); the backward sums dH * (1 - H^2) over k into dE and over the (t, k) that read row u
    into dP (asrk_rnnt_joint_band_bwd_f32)."""

    @staticmethod
    def forward(ctx, E, P, s, S):
        _require_gpu(E)
        E, P = _f32c(E), _f32c(P)
        S = int(S)
        if E.dim() != 3 or P.dim() != 3 or E.shape[0] != P.shape[0] or E.shape[2] != P.shape[2]:
            raise _lib.AsrkError("RNNTJointBandFn: E must be [B, T, J] and P [B, U + 1, J]")
        if not 1 <= S <= RNNT_PRUNE_MAX_RANGE:
            raise _lib.AsrkError("RNNTJointBandFn: 1 <= S <= %d" % RNNT_PRUNE_MAX_RANGE)
        B, T, J = E.shape
        U1 = P.shape[1]
        s = _band_starts("RNNTJointBandFn", s, B, T, E.device)
        H = torch.empty((B, T, S, J), dtype=torch.float32, device=E.device)
        _lib.check(_L().asrk_rnnt_joint_band_f32(_p(E), J, _p(P), J, _p(s), B, T, S, U1, J, _p(H), J, _stream()),
                   "rnnt_joint_band")
        ctx.save_for_backward(H, s)
        ctx.U1 = U1
        return H

    @staticmethod
    def backward(ctx, dH):
        H, s = ctx.saved_tensors
        B, T, S, J = H.shape
        U1 = ctx.U1
        dH = _f32c(dH)
        dE = torch.empty((B, T, J), dtype=torch.float32, device=H.device)
        dP = torch.empty((B, U1, J), dtype=torch.float32, device=H.device)
        _lib.check(_L().asrk_rnnt_joint_band_bwd_f32(_p(H), J, _p(dH), J, _p(s), B, T, S, U1, J, _p(dE), J, _p(dP), J,
                                                     _stream()), "rnnt_joint_band_bwd")
        return dE, dP, None, None


class RNNTBandLossFn(Function):
    """RNNTBandLossFn.apply(logits [B,T,S,V], targets [B,L], enc_len, txt_len, s int32 [B,T], U1, blank, reduction,
    consume_logits): the dense transducer loss with lpb = lpl = -inf at every cell outside the band u in [s[b,t], s[b,t]
    + S).  Row pass on the band (asrk_rnnt_rows_band_f32), its lpb / lpl scattered into -inf-filled [B,T,U1] arrays, the
    dense lattice, and the gradient pass on the band (asrk_rnnt_grad_band_f32), in place with consume_logits.  An
    utterance whose band holds no path has nll = +inf and an all-zero gradient."""

    @staticmethod
    def forward(ctx, logits, targets, enc_len, txt_len, s, U1, blank=0, reduction="mean", consume_logits=False):
        _require_gpu(logits)
        if logits.dim() != 4:
            raise _lib.AsrkError("RNNTBandLoss: logits must be [B, T, S, V]")
        x = _f32c(logits)
        B, T, S, V = x.shape
        U1 = int(U1)
        dev = x.device
        txt, el, tl = _rnnt_lengths("RNNTBandLoss", targets, enc_len, txt_len, B, U1, dev)
        s = _band_starts("RNNTBandLoss", s, B, T, dev)
        L = _L()
        lse = torch.empty((B, T, S), dtype=torch.float32, device=dev)
        lpb_b, lpl_b = torch.empty_like(lse), torch.empty_like(lse)
        lpb = torch.empty((B, T, U1), dtype=torch.float32, device=dev)
        lpl, alpha, beta = torch.empty_like(lpb), torch.empty_like(lpb), torch.empty_like(lpb)
        nll = torch.empty((B,), dtype=torch.float32, device=dev)
        _lib.check(L.asrk_rnnt_rows_band_f32(_p(x), V, _p(txt), txt.shape[1], _p(el), _p(tl), _p(s), B, T, S, U1, V, blank,
                                             _p(lse), _p(lpb_b), _p(lpl_b), _stream()), "rnnt_rows_band")
        _lib.check(L.asrk_rnnt_band_scatter_f32(_p(lpb_b), _p(lpl_b), _p(s), _p(el), _p(tl), B, T, S, U1, _p(lpb), _p(lpl),
                                                _stream()), "rnnt_band_scatter")
        _lib.check(L.asrk_rnnt_lattice_f32(_p(lpb), _p(lpl), _p(el), _p(tl), B, T, U1, _p(alpha), _p(beta), _p(nll),
                                           _stream()), "rnnt_lattice")
        ctx.save_for_backward(x, txt, el, tl, s, lse, lpb, lpl, alpha, beta, nll)
        ctx.meta = (U1, blank, reduction, bool(consume_logits))
        if reduction == "mean":
            return nll.mean()
        if reduction == "sum":
            return nll.sum()
        return nll

    @staticmethod
    def backward(ctx, gout):
        x, txt, el, tl, s, lse, lpb, lpl, alpha, beta, nll = ctx.saved_tensors
        U1, blank, reduction, consume = ctx.meta
        B, T, S, V = x.shape
        g = gout.to(torch.float32)
        if reduction == "mean":
            gscale = (g / B).expand(B)
        elif reduction == "sum":
            gscale = g.expand(B)
        else:
            gscale = g
        gscale = gscale.contiguous()
        dz = x if consume else torch.empty_like(x)
        _lib.check(_L().asrk_rnnt_grad_band_f32(_p(x), V, _p(txt), txt.shape[1], _p(el), _p(tl), _p(s), B, T, S, U1, V,
                                                blank, _p(lse), _p(lpb), _p(lpl), _p(alpha), _p(beta), _p(nll),
                                                _p(gscale), _p(dz), V, _stream()), "rnnt_grad_band")
        return (dz,) + (None,) * 8


class RNNTBandLoss(torch.nn.Module):
    """Transducer loss on band logits [B, T, S, V] (RNNTJointBandFn -> lin_out): forward(logits, targets, enc_len,
    txt_len, s, consume_logits=False), `s` from ops.rnnt_prune_ranges; U + 1 is targets.shape[1] + 1 unless U1 is
    given.  Reductions as ops.RNNTLoss."""

    def __init__(self, blank=0, reduction="mean"):
        super().__init__()
        if reduction not in ("none", "mean", "sum"):
            raise ValueError("RNNTBandLoss: unknown reduction %r" % (reduction,))
        self.blank = blank
        self.reduction = reduction

    def forward(self, logits, targets, enc_len, txt_len, s, consume_logits=False, U1=None):
        U1 = int(torch.as_tensor(targets).shape[1]) + 1 if U1 is None else int(U1)
        return RNNTBandLossFn.apply(logits, targets, enc_len, txt_len, s, U1, self.blank, self.reduction, consume_logits)


# --------------------------------------------------------------------------- stateless prediction network (csrc/rnnt_ctx.hip)
RNNT_CTX_MAX = 8            # CTX_MAX_C of csrc/rnnt_ctx.hip


def _ctx_rows(what, t, D):
    """t [B, U1, D] f32 as rows of D floats with one row stride: (tensor, ld); a copy unless t is such a view already"""
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != D:
        raise _lib.AsrkError(what + ": expected a float32 [B, U1, %d] tensor" % D)
    if t.is_contiguous():
        return t, D
    ld = t.stride(1)
    if t.stride(2) == 1 and ld >= D and t.stride(0) == t.shape[1] * ld:
        return t, ld
    return t.contiguous(), D


def _ctx_weight(what, w, D):
    if w.dim() != 3 or w.shape[0] != D or w.shape[1] != 1 or not 1 <= w.shape[2] <= RNNT_CTX_MAX:
        raise _lib.AsrkError(what + ": w must be [D, 1, C] with 1 <= C <= %d" % RNNT_CTX_MAX)
    return _f32c(w)


@torch.no_grad()
def rnnt_ctx_fwd(X, w, out=None):
    """Y[b,u,d] = relu(sum_j w[d,0,j] X[b, u-(C-1)+j, d]) (asrk_rnnt_ctx_fwd_f32): X [B,U1,D] and `out` may be row-strided
    views (last stride 1, one stride between consecutive rows of [B*U1]); w [D,1,C]"""
    _require_gpu(X)
    if X.dim() != 3:
        raise _lib.AsrkError("rnnt_ctx_fwd: X must be [B, U1, D]")
    B, U1, D = X.shape
    w = _ctx_weight("rnnt_ctx_fwd", w, D)
    x, ldx = _ctx_rows("rnnt_ctx_fwd", X if X.dtype == torch.float32 else X.float(), D)
    if out is None:
        out = torch.empty((B, U1, D), dtype=torch.float32, device=X.device)
    y, ldy = _ctx_rows("rnnt_ctx_fwd", out, D)
    if y is not out:
        raise _lib.AsrkError("rnnt_ctx_fwd: out must be a row-strided [B, U1, D] view")
    _lib.check(_L().asrk_rnnt_ctx_fwd_f32(_p(x), ldx, _p(w), B, U1, D, w.shape[2], _p(y), ldy, _stream()), "rnnt_ctx_fwd")
    return out


class RNNTContextFn(Function):
    """RNNTContextFn.apply(X [B,U1,D], w [D,1,C]) -> Y [B,U1,D]: the stateless prediction network on the embedded labels,
    a causal depthwise convolution over the last C positions and a ReLU (asrk_rnnt_ctx_fwd_f32).  The backward
    (asrk_rnnt_ctx_bwd_f32) takes the derivative at a pre-activation of exactly 0 as 0 and reduces dw in a fixed order."""

    @staticmethod
    def forward(ctx, X, w):
        _require_gpu(X)
        X, w = _f32c(X), _f32c(w)
        Y = rnnt_ctx_fwd(X, w)
        ctx.save_for_backward(X, w, Y)
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, w, Y = ctx.saved_tensors
        B, U1, D = X.shape
        C = w.shape[2]
        dY = _f32c(dY)
        dX, dw = torch.empty_like(X), torch.empty_like(w)
        if B * U1 == 0:
            return dX, dw.zero_()
        L = _L()
        nbytes = int(L.asrk_rnnt_ctx_bwd_ws_bytes(B, U1, D, C))
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=X.device)
        _lib.check(L.asrk_rnnt_ctx_bwd_f32(_p(X), _p(w), _p(Y), _p(dY), B, U1, D, C, _p(dX), _p(dw), _p(ws), nbytes,
                                           _stream()), "rnnt_ctx_bwd")
        return dX, dw


@torch.no_grad()
def rnnt_ctx_step(tokens, n_tok, emb_weight, w, out=None):
    """the decode form (asrk_rnnt_ctx_step_f32): row r of tokens [R, Lc] (int64: the greedy state's; int32: one buffer of
    the beam state's [B, W, Lc], taken as [B*W, Lc]) with n_tok[r] labels -> [R, D], the prediction-network output after
    <sos> and those labels, gathered straight from the embedding matrix emb_weight [V, D]; w [D,1,C]"""
    _require_gpu(emb_weight)
    if tokens.dtype not in (torch.int32, torch.int64) or tokens.dim() < 2 or not tokens.is_contiguous():
        raise _lib.AsrkError("rnnt_ctx_step: tokens must be a contiguous int32 / int64 [..., Lc] tensor")
    Lc = tokens.shape[-1]
    R = tokens.numel() // Lc if Lc else 0
    if n_tok.dtype != torch.int32 or n_tok.numel() != R or not n_tok.is_contiguous():
        raise _lib.AsrkError("rnnt_ctx_step: n_tok must be contiguous int32, one per row of tokens")
    if emb_weight.dim() != 2:
        raise _lib.AsrkError("rnnt_ctx_step: emb_weight must be [V, D]")
    emb = _f32c(emb_weight)
    V, D = emb.shape
    w = _ctx_weight("rnnt_ctx_step", w, D)
    if out is None:
        out = torch.empty((R, D), dtype=torch.float32, device=emb.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (R, D) or (D > 1 and out.stride(1) != 1):
        raise _lib.AsrkError("rnnt_ctx_step: out must be a float32 [R, D] tensor with unit last stride")
    ldy = out.stride(0) if R > 1 else max(out.stride(0), D)
    _lib.check(_L().asrk_rnnt_ctx_step_f32(_p(tokens), tokens.element_size(), Lc, _p(n_tok), R, Lc, _p(emb), V, D, _p(w),
                                           w.shape[2], _p(out), ldy, _stream()), "rnnt_ctx_step")
    return out


# --------------------------------------------------------------------------- cross entropy
def _check_label_smoothing(eps):
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps < 1.0:
        raise ValueError("label_smoothing must be a number in [0, 1), got %r" % (eps,))
    return float(eps)


class CrossEntropyFn(Function):
    """CrossEntropyLoss(ignore_index, reduction='mean') on logits [R,V], targets [R]
    (reference: bin/train_asr.py:47,130-131)."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index, label_smoothing=0.0):
        _require_gpu(logits)
        eps = _check_label_smoothing(label_smoothing)
        x = _f32c(logits)
        R, V = x.shape
        tg = targets.to(device=x.device, dtype=torch.int64).contiguous()
        lse = torch.empty((R,), dtype=torch.float32, device=x.device)
        ctx.ignore_index = ignore_index
        ctx.label_smoothing = eps
        if eps == 0.0:      # the plain kernels: bit-identical to a caller that never heard of smoothing
            sums = torch.empty((2,), dtype=torch.float32, device=x.device)
            _lib.check(_L().asrk_cross_entropy_fwd_f32(_p(x), R, V, V, _p(tg), ignore_index, _p(lse),
                                                       _p(sums), _stream()), "cross_entropy")
            ctx.save_for_backward(x, tg, lse, sums)
            return sums[0] / sums[1]
        smooth = torch.empty((R,), dtype=torch.float32, device=x.device)
        sums = torch.empty((3,), dtype=torch.float32, device=x.device)     # sum nll, count, sum (lse - mean x)
        _lib.check(_L().asrk_cross_entropy_ls_fwd_f32(_p(x), R, V, V, _p(tg), ignore_index, _p(lse), _p(smooth),
                                                      _p(sums), _stream()), "cross_entropy_ls")
        ctx.save_for_backward(x, tg, lse, sums)
        return ((1.0 - eps) * sums[0] + eps * sums[2]) / sums[1]

    @staticmethod
    def backward(ctx, gout):
        x, tg, lse, sums = ctx.saved_tensors
        R, V = x.shape
        gscale = (gout.to(torch.float32) / sums[1]).reshape(1).contiguous()
        dx = torch.empty_like(x)
        if ctx.label_smoothing == 0.0:
            _lib.check(_L().asrk_cross_entropy_bwd_f32(_p(x), R, V, V, _p(tg), ctx.ignore_index, _p(lse),
                                                       _p(gscale), _p(dx), _stream()), "cross_entropy_bwd")
        else:
            _lib.check(_L().asrk_cross_entropy_ls_bwd_f32(_p(x), R, V, V, _p(tg), ctx.ignore_index,
                                                          ctx.label_smoothing, _p(lse), _p(gscale), _p(dx),
                                                          _stream()), "cross_entropy_ls_bwd")
        return dx, None, None, None


class CrossEntropyLoss(torch.nn.Module):
    """Drop-in for torch.nn.CrossEntropyLoss(ignore_index=0, label_smoothing=...) on the MI355X path (uniform
    smoothing, no class weights)."""

    def __init__(self, ignore_index=-100, reduction="mean", label_smoothing=0.0):
        super().__init__()
        assert reduction == "mean"
        self.ignore_index = ignore_index
        self.label_smoothing = _check_label_smoothing(label_smoothing)

    def forward(self, logits, targets):
        if self.label_smoothing == 0.0:
            return CrossEntropyFn.apply(logits, targets, self.ignore_index)
        return CrossEntropyFn.apply(logits, targets, self.ignore_index, self.label_smoothing)


class NLLLossFn(Function):
    """NLLLoss(ignore_index, reduction='mean') on log-probabilities [R,V], targets [R] (reference:
    bin/train_asr.py:62, the attention loss under embedding fusion)."""

    @staticmethod
    def forward(ctx, logp, targets, ignore_index):
        _require_gpu(logp)
        x = _f32c(logp)
        R, V = x.shape
        tg = targets.to(device=x.device, dtype=torch.int64).contiguous()
        if tg.numel() != R:
            raise RuntimeError("nll_loss: %d targets for %d rows" % (tg.numel(), R))
        sums = torch.empty((2,), dtype=torch.float32, device=x.device)
        _lib.check(_L().asrk_nll_loss_fwd_f32(_p(x), R, V, V, _p(tg), ignore_index, _p(sums), _stream()), "nll_loss")
        ctx.ignore_index, ctx.shape = ignore_index, (R, V)
        ctx.save_for_backward(tg, sums)
        return sums[0] / sums[1]

    @staticmethod
    def backward(ctx, gout):
        tg, sums = ctx.saved_tensors
        R, V = ctx.shape
        gscale = (gout.to(torch.float32) / sums[1]).reshape(1).contiguous()
        dx = torch.empty((R, V), dtype=torch.float32, device=tg.device)
        _lib.check(_L().asrk_nll_loss_bwd_f32(R, V, V, _p(tg), ctx.ignore_index, _p(gscale), _p(dx), _stream()),
                   "nll_loss_bwd")
        return dx, None, None


class NLLLoss(torch.nn.Module):
    """Drop-in for torch.nn.NLLLoss(ignore_index=0) on the MI355X path (no class weights)."""

    def __init__(self, ignore_index=-100, reduction="mean"):
        super().__init__()
        assert reduction == "mean"
        self.ignore_index = ignore_index

    def forward(self, logp, targets):
        return NLLLossFn.apply(logp, targets, self.ignore_index)


# --------------------------------------------------------------------------- LayerNorm / dropout
class LayerNormFn(Function):
    """torch.nn.LayerNorm(D) over the last axis (reference: src/module.py:116-117,135-136)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        _require_gpu(x)
        xc = _f32c(x)
        D = xc.shape[-1]
        if weight.numel() != D or bias.numel() != D:
            raise RuntimeError("layer_norm: normalized_shape {} does not match input [..., {}]".format(
                tuple(weight.shape), D))
        rows = xc.numel() // D
        w, b = _f32c(weight), _f32c(bias)
        y = torch.empty_like(xc)
        mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
        rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
        _lib.check(_L().asrk_layer_norm_fwd_f32(_p(xc), _p(w), _p(b), _p(y), _p(mean), _p(rstd), rows, D,
                                                float(eps), _stream()), "layer_norm")
        ctx.save_for_backward(xc, w, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, w, mean, rstd = ctx.saved_tensors
        D = xc.shape[-1]
        rows = xc.numel() // D
        dyc = _f32c(dy)
        dx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        want_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dw = torch.empty((D,), dtype=torch.float32, device=dy.device) if want_p else None
        db = torch.empty((D,), dtype=torch.float32, device=dy.device) if want_p else None
        _lib.check(_L().asrk_layer_norm_bwd_f32(_p(xc), _p(w), _p(dyc), _p(mean), _p(rstd), _p(dx), _p(dw),
                                                _p(db), rows, D, _stream()), "layer_norm_bwd")
        return dx, dw, db, None


def layer_norm(x, weight, bias, eps):
    return LayerNormFn.apply(x, weight, bias, eps)


class DropoutFn(Function):
    """Inverted dropout whose mask is a pure function of (seed, element index): nothing but the
    64-bit seed is kept for the backward (reference: nn.Dropout at src/module.py:118-119,137-138,
    src/asr.py:36,162; the RNG stream necessarily differs from torch's)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        _require_gpu(x)
        xc = _f32c(x)
        y = torch.empty_like(xc)
        _lib.check(_L().asrk_dropout_f32(_p(xc), _p(y), xc.numel(), float(p), seed, 0, _stream()), "dropout")
        ctx.p, ctx.seed = float(p), seed
        return y

    @staticmethod
    def backward(ctx, dy):
        dyc = _f32c(dy)
        dx = torch.empty_like(dyc)
        _lib.check(_L().asrk_dropout_f32(_p(dyc), _p(dx), dyc.numel(), ctx.p, ctx.seed, 0, _stream()),
                   "dropout_bwd")
        return dx, None, None


def dropout(x, p, training, seed=None):
    """nn.Dropout(p)(x).  `seed` (optional, 64-bit) pins the mask; by default it is drawn from torch's
    CPU generator, so torch.manual_seed() makes runs reproducible without a device sync."""
    if not training or p == 0:
        return x
    if p >= 1:
        raise ValueError("dropout probability has to be in [0, 1), got {}".format(p))
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return DropoutFn.apply(x, p, seed)


def spec_augment(x, lens, params, n_fmask, n_tmask, fill=0.0, channels=1):
    """SpecAugment of a padded feature batch in one launch (csrc/spec_augment.hip; semantics: include/asrk.h
    asrk_spec_augment_f32).  x [B, T, channels * D] f32 on the GPU; lens [B] int64 and params
    [B, 2 + 2*n_fmask + 2*n_tmask] int32 (rows c, w, f0_0, fw_0, .., t0_0, tw_0, ..), both on x's device.  Returns a new
    tensor of x's shape.  No autograd: an augmentation of the INPUT, applied under no_grad."""
    _require_gpu(x)
    xc = _f32c(x.detach())
    if xc.dim() != 3:
        raise ValueError("spec_augment expects [B, T, F] features, got %s" % (tuple(xc.shape),))
    B, T, F = xc.shape
    P = 2 + 2 * int(n_fmask) + 2 * int(n_tmask)
    if channels <= 0 or F % channels != 0:
        raise ValueError("feature width %d is no multiple of %d channels" % (F, channels))
    if (lens.dtype != torch.int64 or lens.device != xc.device or tuple(lens.shape) != (B,)
            or not lens.is_contiguous()):
        raise ValueError("lens must be a contiguous int64 [B] tensor on x's device")
    if (params.dtype != torch.int32 or params.device != xc.device or tuple(params.shape) != (B, P)
            or not params.is_contiguous()):
        raise ValueError("params must be a contiguous int32 [B, %d] tensor on x's device" % P)
    y = torch.empty_like(xc)
    _lib.check(_L().asrk_spec_augment_f32(_p(xc), _p(y), B, T, F, F // channels, channels, _p(lens), _p(params),
                                          int(n_fmask), int(n_tmask), float(fill), _stream()), "spec_augment")
    return y


_RESAMPLE_TAPS = {}
RESAMPLE_LOWPASS_WIDTH = 6
RESAMPLE_ROLLOFF = 0.99


def resample_width(orig, new):
    """half-width of the polyphase filter in input samples: ceil(W * orig / (min(orig, new) * rolloff)), taken exactly
    (the library derives the same number: include/asrk.h, asrk_resample_rows_f32)"""
    return -(-100 * RESAMPLE_LOWPASS_WIDTH * orig // (99 * min(orig, new)))


def resample_taps(orig, new):
    """the tap table h [new, 2*width + orig] of one ratio in float64 (torchaudio's sinc_interp_hann kernel)"""
    W = float(RESAMPLE_LOWPASS_WIDTH)
    base = min(orig, new) * RESAMPLE_ROLLOFF
    width = resample_width(orig, new)
    j = np.arange(new, dtype=np.float64)[:, None]
    k = np.arange(2 * width + orig, dtype=np.float64)[None, :]
    t = np.clip((-j / new + (k - width) / orig) * base, -W, W)
    return np.sinc(t) * np.cos(np.pi * t / (2.0 * W)) ** 2 * (base / orig)      # np.sinc(t) = sin(pi t) / (pi t)


def _resample_taps_dev(orig, new, device):
    key = (orig, new, str(device))
    tab = _RESAMPLE_TAPS.get(key)
    if tab is None:
        tab = torch.from_numpy(np.ascontiguousarray(resample_taps(orig, new), dtype=np.float32)).to(device)
        _RESAMPLE_TAPS[key] = tab
    return tab


def resample_rows(x, n_host, ratio_idx, ratios, scale=1.0):
    """Polyphase resampling of every row of a padded waveform batch by its own ratio, in one launch
    (csrc/resample.hip; semantics: include/asrk.h asrk_resample_rows_f32).  x [B, ld_in] int16 or float32 on the GPU;
    n_host [B] the rows' sample counts and ratio_idx [B] their indices into `ratios`, a list of coprime (orig, new)
    pairs, all ON THE HOST.  Row b is slowed down / sped up by speed = orig / new.  -> (y [B, ld_out] float32, already
    multiplied by `scale`, columns beyond a row's own length left unwritten; n_out int64 numpy [B]).  The output
    lengths are computed here on the host: nothing is read back from the device."""
    _require_gpu(x)
    if x.dim() != 2 or x.dtype not in (torch.int16, torch.float32) or not x.is_contiguous():
        raise ValueError("resample_rows expects a contiguous [B, ld_in] int16 or float32 batch")
    B, ld_in = x.shape
    n = np.ascontiguousarray(np.asarray(n_host, dtype=np.int64).reshape(-1))
    idx = np.ascontiguousarray(np.asarray(ratio_idx, dtype=np.int32).reshape(-1))
    rat = np.ascontiguousarray(np.asarray(ratios, dtype=np.int32).reshape(-1, 2))
    if n.shape[0] != B or idx.shape[0] != B:
        raise ValueError("resample_rows: %d rows, %d lengths, %d ratio indices" % (B, n.shape[0], idx.shape[0]))
    if B and (rat.shape[0] == 0 or idx.min() < 0 or idx.max() >= rat.shape[0] or rat.min() < 1):
        raise ValueError("resample_rows: ratio index outside the %d ratio(s) given, or a non-positive ratio"
                         % rat.shape[0])
    n_out = (rat[idx, 1].astype(np.int64) * n + rat[idx, 0] - 1) // rat[idx, 0] if B else np.zeros(0, np.int64)
    ld_out = (int(n_out.max()) + 3) // 4 * 4 if B else 0
    y = torch.empty((B, ld_out), dtype=torch.float32, device=x.device)
    if B == 0:
        return y, n_out
    tabs = [None if (o, w) == (1, 1) else _resample_taps_dev(int(o), int(w), x.device) for o, w in rat.tolist()]
    taps = (ctypes.c_void_p * len(tabs))(*[None if t is None else t.data_ptr() for t in tabs])
    # the kernel's copies of the lengths and indices: one pinned buffer, one non-blocking upload
    meta = torch.empty(B + (B + 1) // 2, dtype=torch.int64).pin_memory()
    meta[:B] = torch.from_numpy(n)
    meta[B:].view(torch.int32)[:B] = torch.from_numpy(idx)
    meta_dev = meta.to(x.device, non_blocking=True)
    _lib.check(_L().asrk_resample_rows_f32(_p(x), x.element_size(), ld_in, n.ctypes.data, meta_dev.data_ptr(),
                                           idx.ctypes.data, meta_dev.data_ptr() + 8 * B, B, rat.ctypes.data, taps,
                                           rat.shape[0], _p(y), ld_out, float(scale), _stream()), "resample_rows")
    return y, n_out


REVERB_MAX_TAPS = 8192          # RM_MAX_TAPS of csrc/reverb_mix.hip


class RirBank:
    """Room impulse responses resident on the device: taps [R, ld_r] float32 (rows zero padded), with every response's
    length and peak - the first index of its largest |h| - on the host and, in one int32 tensor, on the device.  Built
    once from a list of 1-D arrays of 1..8192 samples; ops.reverb_mix reads rows of it."""

    def __init__(self, responses, device="cuda"):
        hs = [np.ascontiguousarray(np.asarray(h, dtype=np.float32).reshape(-1)) for h in responses]
        if not hs:
            raise ValueError("RirBank: no impulse response")
        for h in hs:
            if not 1 <= h.shape[0] <= REVERB_MAX_TAPS or not np.all(np.isfinite(h)):
                raise ValueError("RirBank: an impulse response has 1..%d finite samples, got %d"
                                 % (REVERB_MAX_TAPS, h.shape[0]))
        self.lens = np.asarray([h.shape[0] for h in hs], dtype=np.int32)
        self.peaks = np.asarray([int(np.argmax(np.abs(h))) for h in hs], dtype=np.int32)
        self.ld = (int(self.lens.max()) + 3) // 4 * 4
        host = np.zeros((len(hs), self.ld), dtype=np.float32)
        for r, h in enumerate(hs):
            host[r, :h.shape[0]] = h
        self.taps = torch.from_numpy(host).to(device)
        self.meta = torch.from_numpy(np.concatenate([self.lens, self.peaks])).to(device)      # lens | peaks

    def __len__(self):
        return int(self.lens.shape[0])


def reverb_mix(x, n_host, bank=None, rir_idx=None, noise=None, m_host=None, snr_lin=None, scale=1.0):
    """Reverberation and additive noise for every row of a padded waveform batch (csrc/reverb_mix.hip; semantics:
    include/asrk.h asrk_reverb_mix_f32).  x [B, ld_in] int16 or float32 on the GPU, n_host [B] the rows' sample counts;
    bank: a RirBank (None: no reverberation) and rir_idx [B] the rows' responses, -1 for none; noise [B, ld_v] of x's
    dtype on x's device (None: no noise), m_host [B] the samples each noise row holds (0: none; shorter than the
    utterance: tiled circularly) and snr_lin [B] = 10^(snr_dB / 10); all index and length arrays ON THE HOST.
    -> out [B, roundup4(max n)] float32, already multiplied by `scale`, columns beyond a row's length left unwritten.
    Nothing is read back from the device."""
    _require_gpu(x)
    if x.dim() != 2 or x.dtype not in (torch.int16, torch.float32) or not x.is_contiguous():
        raise ValueError("reverb_mix expects a contiguous [B, ld_in] int16 or float32 batch")
    B, ld_in = x.shape
    n = np.ascontiguousarray(np.asarray(n_host, dtype=np.int64).reshape(-1))
    idx = np.full(B, -1, dtype=np.int32) if rir_idx is None else \
        np.ascontiguousarray(np.asarray(rir_idx, dtype=np.int32).reshape(-1))
    m = np.zeros(B, dtype=np.int64) if m_host is None else \
        np.ascontiguousarray(np.asarray(m_host, dtype=np.int64).reshape(-1))
    snr = np.ones(B, dtype=np.float32) if snr_lin is None else \
        np.ascontiguousarray(np.asarray(snr_lin, dtype=np.float32).reshape(-1))
    if not (n.shape[0] == idx.shape[0] == m.shape[0] == snr.shape[0] == B):
        raise ValueError("reverb_mix: %d rows, %d lengths, %d response indices, %d noise lengths, %d ratios"
                         % (B, n.shape[0], idx.shape[0], m.shape[0], snr.shape[0]))
    if bank is None and B and idx.max() >= 0:
        raise ValueError("reverb_mix: a row asks for an impulse response and no bank was given")
    if bank is not None and bank.taps.device != x.device:
        raise ValueError("reverb_mix: the bank lives on %s, the batch on %s" % (bank.taps.device, x.device))
    if noise is None:
        if B and m.max() > 0:
            raise ValueError("reverb_mix: a row asks for noise and no noise batch was given")
        ld_v = 0
    else:
        _require_gpu(noise)
        if (noise.dim() != 2 or noise.shape[0] != B or noise.dtype != x.dtype or not noise.is_contiguous()
                or noise.device != x.device):
            raise ValueError("reverb_mix: noise must be a contiguous [B, ld_v] batch of x's dtype on x's device")
        ld_v = noise.shape[1]
    if B and not (np.all(np.isfinite(snr)) and snr.min() > 0.0):
        raise ValueError("reverb_mix: snr_lin must be positive and finite")
    ld_out = (int(n.max()) + 3) // 4 * 4 if B else 0
    out = torch.empty((B, ld_out), dtype=torch.float32, device=x.device)
    if B == 0:
        return out
    L = _L()
    ws_bytes = int(L.asrk_reverb_mix_ws_bytes(B, int(max(n.max(), 0))))
    ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device=x.device)
    # the kernels' copies of the lengths, indices and ratios: one pinned buffer, one non-blocking upload
    meta = torch.empty(3 * B, dtype=torch.int64).pin_memory()
    meta[:B] = torch.from_numpy(n)
    meta[B:2 * B] = torch.from_numpy(m)
    meta[2 * B:].view(torch.int32)[:B] = torch.from_numpy(idx)
    meta[2 * B:].view(torch.float32)[B:2 * B] = torch.from_numpy(snr)
    md = meta.to(x.device, non_blocking=True)
    base = md.data_ptr()
    R = 0 if bank is None else len(bank)
    _lib.check(L.asrk_reverb_mix_f32(
        _p(x), x.element_size(), ld_in, n.ctypes.data, base,
        None if bank is None else _p(bank.taps), 0 if bank is None else bank.ld,
        None if bank is None else bank.lens.ctypes.data, None if bank is None else bank.meta.data_ptr(),
        None if bank is None else bank.peaks.ctypes.data, None if bank is None else bank.meta.data_ptr() + 4 * R, R,
        idx.ctypes.data, base + 16 * B, _p(noise), ld_v, m.ctypes.data, base + 8 * B, base + 20 * B, B, _p(out), ld_out,
        float(scale), _p(ws), ws_bytes, _stream()), "reverb_mix")
    return out
