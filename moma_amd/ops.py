"""torch-facing wrappers of the C ABI (include/moma_hip.h): device pointers and the current HIP stream
are handed to libmoma_hip.so; autograd Functions wire the hand-written backward kernels in.

PyTorch is plumbing here (memory, streams, autograd graph); all arithmetic of the hot path happens in
the HIP library.  Every wrapper refuses CPU tensors: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import torch

from . import _lib
from ._lib import DT_BF16, DT_F32, PREC_BF16, PREC_F32, EMA_BLOCK_ELEMS, MomaHipError, check

_PREC = {"fp32": PREC_F32, "f32": PREC_F32, "float32": PREC_F32, PREC_F32: PREC_F32,
         "bf16": PREC_BF16, "bfloat16": PREC_BF16, PREC_BF16: PREC_BF16}


def prec_code(p) -> int:
    try:
        return _PREC[p]
    except KeyError:
        raise ValueError(f"unknown precision {p!r}; use 'fp32' or 'bf16'")


def _qdtype(queue: torch.Tensor) -> int:
    if queue.dtype == torch.float32:
        return DT_F32
    if queue.dtype == torch.bfloat16:
        return DT_BF16
    raise TypeError(f"queue dtype must be float32 or bfloat16, got {queue.dtype}")


def _dev(t: torch.Tensor, name: str, dtype=torch.float32, contiguous=True) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise MomaHipError(f"{name}: the MoMA hot path runs only on the GPU (HIP library); got a "
                           f"{'CPU tensor' if isinstance(t, torch.Tensor) else type(t)}. No CPU fallback exists.")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _dense_pair(p: torch.Tensor, e: torch.Tensor) -> None:
    """Element-wise kernels walk the raw storage: both tensors must be dense with identical strides
    (row-major or channels_last -- the memory format only permutes the walk order)."""
    for t, nm in ((p, "param"), (e, "param_ema")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise MomaHipError(f"{nm}: the MoMA hot path runs only on the GPU (HIP library). No CPU fallback exists.")
        if t.dtype != torch.float32:
            raise TypeError(f"{nm}: expected float32, got {t.dtype}")
    dense = p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))
    if not dense or p.stride() != e.stride():
        raise ValueError("momentum_update: parameter pair must be dense with identical strides "
                         f"(got {p.stride()} vs {e.stride()})")


# Optional instrumentation (bench.py): a callable (name) -> context manager recording HIP events on the
# current stream around a C-ABI call.  None in normal operation.
_EVENT_RECORDER = None


def set_event_recorder(rec) -> None:
    global _EVENT_RECORDER
    _EVENT_RECORDER = rec


# Optional (bench.py): a callable returning three raw hipEvent_t handles that the library records on the dispatches of the next
# moma_infonce_fused call: begin / end of its dominant kernel and end of its last kernel (see moma_infonce_fused_q).
_KERNEL_EVENTS = None


def set_kernel_event_provider(fn) -> None:
    global _KERNEL_EVENTS
    _KERNEL_EVENTS = fn


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# Optional tracing (MOMA_ROCTX=1): a roctx range (torch.cuda.nvtx = roctx on ROCm) around every C-ABI call of K1 - K4 and around the
# phases of the graph-served step (helper/step_graph.py), for `rocprofv3 --marker-trace --kernel-trace -- python ...`.  The
# reference has no tracing of its own; off by default: a range is two more host calls per library call.
_ROCTX = __import__("os").environ.get("MOMA_ROCTX", "0") == "1"


class _Range:
    def __init__(self, name, inner=None):
        self.name, self.inner = name, inner

    def __enter__(self):
        torch.cuda.nvtx.range_push(self.name)
        if self.inner is not None:
            self.inner.__enter__()
        return self

    def __exit__(self, *a):
        if self.inner is not None:
            self.inner.__exit__(*a)
        torch.cuda.nvtx.range_pop()
        return False


def trace_range(name):
    """context manager: a roctx range when MOMA_ROCTX=1, nothing otherwise"""
    return _Range(name) if _ROCTX else _NullCtx()


def _timed(name):
    # (no events inside a stream capture: an event recorded there becomes a graph node and carries no timestamp)
    if _EVENT_RECORDER is None or torch.cuda.is_current_stream_capturing():
        return _Range(name) if _ROCTX else _NullCtx()
    return _Range(name, _EVENT_RECORDER(name)) if _ROCTX else _EVENT_RECORDER(name)


_DEBUG = __import__("os").environ.get("MOMA_DEBUG", "0") == "1"
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)       # the handle without building a Stream object


def _stream() -> C.c_void_p:
    # (called once per library call, ~1000x per training step: torch.cuda.current_stream() costs ~12 us of host time each)
    if _RAW_STREAM is not None:
        return C.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


# ------------------------------------------------------------------------------------------------
# K4 multi-tensor EMA   (learning/contrast_trainer.py:207-211)
# ------------------------------------------------------------------------------------------------
class EmaTable:
    """Device-side pointer table for one (model, model_ema) pair; rebuilt if any tensor moves."""

    def __init__(self, params: Sequence[torch.Tensor], params_ema: Sequence[torch.Tensor]):
        params, params_ema = list(params), list(params_ema)
        # zip() semantics of the reference: stops at the shorter list; shapes must match pairwise
        n = min(len(params), len(params_ema))
        rows, first = [], 0
        self.keys = []
        for p, e in zip(params[:n], params_ema[:n]):
            if p.shape != e.shape:
                raise RuntimeError(f"The size of tensor a {tuple(e.shape)} must match the size of tensor b "
                                   f"{tuple(p.shape)} (momentum_update needs identical architectures)")
            _dense_pair(p, e)
            if e.numel() == 0:
                continue
            rows.append((e.data_ptr(), p.data_ptr(), e.numel(), first))
            first += (e.numel() + EMA_BLOCK_ELEMS - 1) // EMA_BLOCK_ELEMS
            self.keys.append((e.data_ptr(), p.data_ptr(), e.numel()))
        self.n = len(rows)
        self.total_blocks = first
        dev = params[0].device if n else torch.device("cuda")
        self.table = (torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).to(dev) if rows
                      else torch.zeros(0, 4, dtype=torch.int64, device=dev))

    def matches(self, params, params_ema) -> bool:
        keys = [(e.data_ptr(), p.data_ptr(), e.numel()) for p, e in zip(params, params_ema) if e.numel()]
        return keys == self.keys


def ema_update_(table: EmaTable, m: float) -> None:
    """ema <- fma(fl32(1-m), p, ema*fl32(m)) for every tensor of the table, one launch."""
    lib = _lib.load()
    if table.n == 0:
        return
    with _timed("moma_ema_multi"):
        check(lib.moma_ema_multi(_ptr(table.table), table.n, table.total_blocks, float(m), float(1.0 - m), _stream()),
              "moma_ema_multi")


# ------------------------------------------------------------------------------------------------
# K3 ring-buffer enqueue   (MoMA/mem_moco.py:17-27)
# ------------------------------------------------------------------------------------------------
def enqueue_(queue: torch.Tensor, rows: torch.Tensor, index: int) -> None:
    lib = _lib.load()
    _dev(queue, "queue", None); _dev(rows, "rows")
    K, d = queue.shape
    if rows.dim() != 2 or rows.shape[1] != d:
        raise ValueError(f"rows must be [n,{d}], got {tuple(rows.shape)}")
    with trace_range("moma_enqueue"):
        check(lib.moma_enqueue(_ptr(queue), _ptr(rows), rows.shape[0], int(index), K, d, _qdtype(queue), _stream()),
              "moma_enqueue")


def queue_prefetch(queue: torch.Tensor, stream=None) -> None:
    """Cache hint (moma_queue_prefetch): sweep the queue into the Infinity Cache on `stream` (default: current)."""
    lib = _lib.load()
    _dev(queue, "queue", None)
    st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    check(lib.moma_queue_prefetch(_ptr(queue), queue.numel() * queue.element_size(), st), "moma_queue_prefetch")


def enqueue_mirror_(queue: torch.Tensor, mirror: torch.Tensor, rows: torch.Tensor, index: int) -> None:
    """fp32 queue + its bf16 mirror, one launch (moma_enqueue_mirror)."""
    lib = _lib.load()
    _dev(queue, "queue"); _dev(mirror, "mirror", torch.bfloat16); _dev(rows, "rows")
    K, d = queue.shape
    if mirror.shape != queue.shape or rows.dim() != 2 or rows.shape[1] != d:
        raise ValueError(f"rows must be [n,{d}] and mirror {tuple(queue.shape)}, got {tuple(rows.shape)} / {tuple(mirror.shape)}")
    with trace_range("moma_enqueue_mirror"):
        check(lib.moma_enqueue_mirror(_ptr(queue), _ptr(mirror), _ptr(rows), rows.shape[0], int(index), K, d, _stream()),
              "moma_enqueue_mirror")


# ------------------------------------------------------------------------------------------------
# K2 InfoNCE
# ------------------------------------------------------------------------------------------------
def _check_qk(q, k, queue):
    _dev(q, "q"); _dev(k, "k"); _dev(queue, "queue", None)
    if q.dim() != 2 or q.shape != k.shape or queue.dim() != 2 or queue.shape[1] != q.shape[1]:
        raise ValueError(f"shape mismatch: q {tuple(q.shape)} k {tuple(k.shape)} queue {tuple(queue.shape)}")


class _InfoNCELogits(torch.autograd.Function):
    """[B,K+1] logits of BaseMoCo._compute_logit (MoMA/mem_moco.py:29-49) with the backward w.r.t. q."""

    @staticmethod
    def forward(ctx, q, k, queue, T, prec):
        lib = _lib.load()
        q = q.contiguous(); k = k.contiguous()
        _check_qk(q, k, queue)
        B, d = q.shape
        K = queue.shape[0]
        out = torch.empty(B, K + 1, device=q.device, dtype=torch.float32)
        check(lib.moma_infonce_logits(_ptr(q), _ptr(k), _ptr(queue), _ptr(out), B, d, K, float(1.0 / T),
                                      _qdtype(queue), prec, _stream()), "moma_infonce_logits")
        ctx.save_for_backward(q, k, queue)
        ctx.T, ctx.prec = T, prec
        return out

    @staticmethod
    def backward(ctx, dlogits):
        lib = _lib.load()
        q, k, queue = ctx.saved_tensors
        dlogits = dlogits.contiguous()
        B, d = k.shape
        K = queue.shape[0]
        dq = dk = dqueue = None
        if ctx.needs_input_grad[0]:
            dq = torch.empty(B, d, device=k.device, dtype=torch.float32)
            # (the form with a workspace: the split-K partials are added in a fixed order -- bitwise reproducible)
            ws = torch.empty(lib.moma_infonce_logits_bwd_workspace_bytes(B, d, K), device=k.device, dtype=torch.uint8)
            check(lib.moma_infonce_logits_bwd_ws(_ptr(dlogits), _ptr(k), _ptr(queue), _ptr(dq), B, d, K,
                                                 float(1.0 / ctx.T), _qdtype(queue), ctx.prec, _ptr(ws), ws.numel(), _stream()),
                  "moma_infonce_logits_bwd_ws")
        # k / queue carry gradient only in the MoCoAtt cross-attention variants (they are attention outputs there)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            if ctx.needs_input_grad[1]:
                dk = torch.empty(B, d, device=k.device, dtype=torch.float32)
            if ctx.needs_input_grad[2]:
                if queue.dtype != torch.float32:
                    raise TypeError("a queue that requires grad must be float32")
                dqueue = torch.empty(K, d, device=k.device, dtype=torch.float32)
            check(lib.moma_infonce_logits_bwd_kq(_ptr(dlogits), _ptr(q), _ptr(dk), _ptr(dqueue), B, d, K,
                                                 float(1.0 / ctx.T), ctx.prec, _stream()), "moma_infonce_logits_bwd_kq")
        return dq, dk, dqueue, None, None


def infonce_logits(q, k, queue, T: float, prec="fp32") -> torch.Tensor:
    return _InfoNCELogits.apply(q, k, queue, float(T), prec_code(prec))


class QPack:
    """The query of K2 in the packed bf16 MFMA-operand layout (moma_infonce_fused_q), written by the producer of q -- the proj
    epilogue of the attention module atts_q (moma_mha_fwd_fast) -- so that K2 runs no pre-pack launch.  One persistent buffer
    per (B, d): its pad rows stay zero.  `src` remembers which q tensor / temperature the image was made from; K2 ignores
    the image unless it is handed exactly that tensor.
    Caveat (as for the weight packs, Attention.invalidate_pack): the identity check is (data_ptr, autograd version, shape, T).  A
    write to q that bypasses the version counter -- arithmetic on `q.data`, a raw-pointer kernel -- between the producer and K2
    leaves a stale image that K2 would pair with the new fp32 q (positive logit and dq come from the fp32 tensor).  Nothing in
    the loop does that; a caller that does must drop the image (`qpack.src = None`) or pass `qpack=None` to K2.  MOMA_DEBUG=1
    re-packs q inside infonce_fused and compares (a test hook, costs a launch and a sync)."""

    def __init__(self):
        self.buf, self.shape, self.scale, self.src = None, None, None, None

    def prepare(self, B: int, d: int, T: float, device):
        """-> this holder, ready to be handed to Attention.forward(x, qpack=...) and then to infonce_fused(..., qpack=...); None
        when K2 takes no pre-packed query at this width (d not in {128, 256, 384, 512})."""
        lib = _lib.load()
        nbytes = lib.moma_infonce_qpack_bytes(B, d)
        if nbytes == 0:
            return None
        if self.buf is None or self.shape != (B, d) or self.buf.device != device:
            self.buf = torch.zeros(nbytes, device=device, dtype=torch.uint8)
            self.shape = (B, d)
        self.scale, self.T = (1.0 / T) * 1.4426950408889634, float(T)
        self.src = None
        return self

    def written_from(self, q: torch.Tensor, T: float):
        self.src = (q.data_ptr(), q._version, tuple(q.shape), float(T))

    def matches(self, q: torch.Tensor, T: float) -> bool:
        return self.buf is not None and self.src == (q.data_ptr(), q._version, tuple(q.shape), float(T))


class K2Buffers:
    """Caller-owned outputs + workspace of one moma_infonce_fused call at a fixed shape: what a step replayed from HIP graphs
    (helper/step_graph.py) hands to K2 every step -- the graphs on either side of the call read / write these addresses."""

    def __init__(self, B: int, d: int, K: int, queue_dtype, prec, device):
        lib = _lib.load()
        self.shape = (B, d, K)
        self.loss_rows = torch.empty(B, device=device, dtype=torch.float32)
        self.lse = torch.empty(B, device=device, dtype=torch.float32)
        self.top1 = torch.empty(B, device=device, dtype=torch.int32)
        self.dq = torch.empty(B, d, device=device, dtype=torch.float32)
        qd = DT_BF16 if queue_dtype == torch.bfloat16 else DT_F32
        self.ws = torch.empty(max(lib.moma_infonce_fused_workspace_bytes(B, d, K, qd, prec_code(prec)), 16), device=device,
                              dtype=torch.uint8)


def _infonce_fused_launch(q, k, queue, T, prec, qpack_buf, loss_rows, lse, top1, dq, ws, enq=None):
    """enq: None, or (rows [n,d] fp32, ring pointer, fp32 queue whose bf16 mirror `queue` is | None) -- the enqueue that follows
    the call (MoMA/mem_moco.py:97-99) rides on the call's last launch (moma_infonce_fused_enqueue)"""
    lib = _lib.load()
    B, d = q.shape
    K = queue.shape[0]
    ev0, ev1, ev2 = _KERNEL_EVENTS() if _KERNEL_EVENTS is not None else (None, None, None)
    with _timed("moma_infonce_fused"):
        if enq is None:
            check(lib.moma_infonce_fused_q(_ptr(q), _ptr(qpack_buf), _ptr(k), _ptr(queue), B, d, K, float(1.0 / T),
                                           _ptr(loss_rows), _ptr(lse), _ptr(top1), _ptr(dq), _ptr(ws), ws.numel(), _qdtype(queue), prec,
                                           _stream(), C.c_void_p(ev0), C.c_void_p(ev1), C.c_void_p(ev2)),
                  "moma_infonce_fused")
        else:
            rows, index, queue_f32 = enq
            _dev(rows, "rows")
            if rows.dim() != 2 or rows.shape[1] != d or not rows.is_contiguous():
                raise ValueError(f"rows must be contiguous [n,{d}], got {tuple(rows.shape)}")
            if queue_f32 is not None:
                _dev(queue_f32, "queue_f32")
                if queue_f32.shape != queue.shape or queue.dtype != torch.bfloat16:
                    raise ValueError("queue_f32 goes with its bf16 mirror of the same shape as `queue`")
            check(lib.moma_infonce_fused_enqueue(_ptr(q), _ptr(qpack_buf), _ptr(k), _ptr(queue), B, d, K, float(1.0 / T),
                                                 _ptr(loss_rows), _ptr(lse), _ptr(top1), _ptr(dq), _ptr(ws), ws.numel(), _qdtype(queue),
                                                 prec, _ptr(rows), rows.shape[0], int(index), _ptr(queue_f32), _stream(),
                                                 C.c_void_p(ev0), C.c_void_p(ev1), C.c_void_p(ev2)),
                  "moma_infonce_fused_enqueue")


def infonce_fused_into(q, k, queue, T: float, prec, qpack_buf, out: K2Buffers, enq=None) -> None:
    """moma_infonce_fused into caller-owned buffers, no autograd: loss_rows / lse / top1 / dq (= d sum(loss_rows) / dq) land in
    `out`.  qpack_buf: the packed image of q its producer wrote (or None: K2 packs q itself).  enq: see _infonce_fused_launch."""
    q = q.detach(); k = k.detach()
    _check_qk(_dev(q, "q"), _dev(k, "k"), queue)
    if (q.shape[0], q.shape[1], queue.shape[0]) != out.shape:
        raise ValueError(f"K2Buffers were made for (B, d, K) = {out.shape}, got {(q.shape[0], q.shape[1], queue.shape[0])}")
    pc = prec_code(prec)
    if qpack_buf is not None and not (queue.dtype == torch.bfloat16 and pc == PREC_BF16):
        qpack_buf = None
    _infonce_fused_launch(q, k, queue, float(T), pc, qpack_buf, out.loss_rows, out.lse, out.top1, out.dq, out.ws, enq)


class StaticK2Loss(torch.autograd.Function):
    """The autograd node that stands for a K2 call made OUTSIDE the captured graphs: forward hands out the loss rows K2 left in
    its static buffer, backward is K2's own (dq * upstream, as _InfoNCEFused.backward)."""

    @staticmethod
    def forward(ctx, q, loss_rows_buf, dq_buf):
        ctx.save_for_backward(dq_buf)
        return loss_rows_buf.view_as(loss_rows_buf)

    @staticmethod
    def backward(ctx, g_loss):
        (dq,) = ctx.saved_tensors
        return dq * g_loss.unsqueeze(1), None, None


class _InfoNCEFused(torch.autograd.Function):
    """One pass over the queue: per-row CE(label 0) loss, lse, top-1 flag and d(sum loss)/dq."""

    @staticmethod
    def forward(ctx, q, k, queue, T, prec, qpack=None, enq=None):
        lib = _lib.load()
        q = q.contiguous(); k = k.contiguous()
        _check_qk(q, k, queue)
        B, d = q.shape
        K = queue.shape[0]
        dev = q.device
        need_grad = ctx.needs_input_grad[0]
        loss_rows = torch.empty(B, device=dev, dtype=torch.float32)
        lse = torch.empty(B, device=dev, dtype=torch.float32)
        top1 = torch.empty(B, device=dev, dtype=torch.int32)
        dq = torch.empty(B, d, device=dev, dtype=torch.float32) if need_grad else None
        ws_bytes = lib.moma_infonce_fused_workspace_bytes(B, d, K, _qdtype(queue), prec)
        ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)
        _infonce_fused_launch(q, k, queue, T, prec, qpack, loss_rows, lse, top1, dq, ws, enq)
        if need_grad:
            ctx.save_for_backward(dq)
        ctx.mark_non_differentiable(lse, top1)
        return loss_rows, lse, top1

    @staticmethod
    def backward(ctx, g_loss, g_lse, g_top1):
        (dq,) = ctx.saved_tensors
        return dq * g_loss.unsqueeze(1), None, None, None, None, None, None


def debug_set_k2_target_wg(n: int) -> int:
    """Plan sweeps only (scripts/sweep_k2_plan.sh): cut K2's passes over the queue into about n workgroups (0 = the product's own
    plan).  Set it BEFORE the first call of the process: cached workspaces are sized under the plan in force when they were made.
    -> the previous value."""
    prev = lib.moma_debug_set_k2_target_wg(int(n))
    if prev < 0:
        raise ValueError(f"moma_debug_set_k2_target_wg({n}): refused (0, or 8 .. 1024)")
    return prev


def infonce_fused(q, k, queue, T: float, prec="fp32", qpack: "QPack | None" = None, enq=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (loss_rows [B], lse [B], top1 [B] int32).  loss_kd = loss_rows.mean().
    qpack: a QPack that the producer of q filled (ignored unless it was written from exactly this q and T).
    enq: None, or (rows, ring pointer, fp32 queue | None): the enqueue behind the pass rides on the call (_infonce_fused_launch)."""
    buf = None
    if qpack is not None and q.is_contiguous() and qpack.matches(q, T) and queue.dtype == torch.bfloat16 \
            and prec_code(prec) == PREC_BF16:
        buf = qpack.buf
        if _DEBUG:
            # the image K2 is about to trust against one made from q as it stands now (own pre-pack: a forward-only call without it)
            with torch.no_grad():
                a = _InfoNCEFused.apply(q.detach(), k.detach(), queue, float(T), prec_code(prec), buf)[1]
                b = _InfoNCEFused.apply(q.detach(), k.detach(), queue, float(T), prec_code(prec), None)[1]
            if not torch.equal(a, b):
                raise MomaHipError("QPack: the packed image of q does not match q (written behind autograd's version counter?)")
    return _InfoNCEFused.apply(q, k, queue, float(T), prec_code(prec), buf, enq)


class _InfoNCEFusedMulti(torch.autograd.Function):
    """n InfoNCE terms (q_i, k_i, queue_i) in one sweep (moma_infonce_fused_multi): inputs q_0, k_0, queue_0, q_1, ...;
    outputs loss_rows_0, lse_0, top1_0, loss_rows_1, ..."""

    @staticmethod
    def forward(ctx, T, prec, *tensors):
        lib = _lib.load()
        n = len(tensors) // 3
        qs = [tensors[3 * i].contiguous() for i in range(n)]
        ks = [tensors[3 * i + 1].contiguous() for i in range(n)]
        queues = [tensors[3 * i + 2] for i in range(n)]
        for q, k, queue in zip(qs, ks, queues):
            _check_qk(q, k, queue)
        B, d = qs[0].shape
        K = queues[0].shape[0]
        dev = qs[0].device
        need_grad = any(ctx.needs_input_grad[2 + 3 * i] for i in range(n))
        qd = _qdtype(queues[0])
        ws = torch.empty(max(lib.moma_infonce_fused_multi_workspace_bytes(n, B, d, K, qd, prec), 16), device=dev, dtype=torch.uint8)
        terms = (_lib.InfoNCETerm * n)()
        outs, dqs = [], []
        for i in range(n):
            # (two terms with the same query tensor share its packed image: the library dedupes by pointer)
            loss_rows = torch.empty(B, device=dev, dtype=torch.float32)
            lse = torch.empty(B, device=dev, dtype=torch.float32)
            top1 = torch.empty(B, device=dev, dtype=torch.int32)
            dq = torch.empty(B, d, device=dev, dtype=torch.float32) if need_grad else None
            t = terms[i]
            t.q, t.k, t.queue = qs[i].data_ptr(), ks[i].data_ptr(), queues[i].data_ptr()
            t.loss_rows, t.lse, t.top1, t.dq = loss_rows.data_ptr(), lse.data_ptr(), top1.data_ptr(), (0 if dq is None else dq.data_ptr())
            outs += [loss_rows, lse, top1]
            dqs.append(dq)
        with _timed("moma_infonce_fused_multi"):
            check(lib.moma_infonce_fused_multi(C.cast(terms, C.c_void_p), n, B, d, K, float(1.0 / T), _ptr(ws), ws.numel(), qd,
                                               prec, _stream()), "moma_infonce_fused_multi")
        if need_grad:
            ctx.save_for_backward(*dqs)
        ctx.n = n
        ctx.mark_non_differentiable(*[o for i, o in enumerate(outs) if i % 3 != 0])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        dqs = ctx.saved_tensors
        res = [None, None]
        for i in range(ctx.n):
            g_loss = grads[3 * i]
            res += [dqs[i] * g_loss.unsqueeze(1) if (ctx.needs_input_grad[2 + 3 * i] and g_loss is not None) else None, None, None]
        return tuple(res)


def infonce_fused_multi(terms, T: float, prec="fp32"):
    """terms = [(q, k, queue), ...] over queues of one shape and dtype -> [(loss_rows, lse, top1), ...] through ONE library call
    (moma_infonce_fused_multi): one sweep where the one-pass bf16 kernel takes the configuration, term by term inside the
    library otherwise (wide rows, exact fp32).  Terms of different shapes: one moma_infonce_fused call each."""
    pc = prec_code(prec)
    q0, _, queue0 = terms[0]
    same = all(q.shape == q0.shape and queue.shape == queue0.shape and queue.dtype == queue0.dtype for q, _, queue in terms)
    if len(terms) > 1 and len(terms) <= 4 and same and q0.is_cuda:
        flat = _InfoNCEFusedMulti.apply(float(T), pc, *[t for term in terms for t in term])
        return [tuple(flat[3 * i:3 * i + 3]) for i in range(len(terms))]
    return [infonce_fused(q, k, queue, T, prec) for q, k, queue in terms]


# ------------------------------------------------------------------------------------------------
# K1 batch-token multi-head attention   (MoMA/criterion_moco_att.py:153-167)
# ------------------------------------------------------------------------------------------------
class MhaPack:
    """bf16 weight pack of one attention module for the fast path ([Wqkv | Wproj | Wqkv^T | Wproj^T], moma_mha_pack_weights):
    rebuilt -- into a NEW buffer, a pending backward keeps the one its forward used -- when the fp32 weights were replaced or
    modified in place (optimizer.step(), load_state_dict: the tensors' version counters move).  A writer that bypasses
    autograd's version counter (a raw-pointer kernel) must call invalidate()."""

    def __init__(self):
        self.buf, self.key, self.has_t = None, None, False

    def invalidate(self):
        self.buf = None

    def get(self, w_qkv: torch.Tensor, w_proj: torch.Tensor, need_t: bool) -> torch.Tensor:
        key = (w_qkv.data_ptr(), w_qkv._version, w_proj.data_ptr(), w_proj._version, w_qkv.device)
        if self.buf is None or key != self.key or (need_t and not self.has_t):
            lib = _lib.load()
            d = w_proj.shape[0]
            buf = torch.empty(lib.moma_mha_pack_bytes(d), device=w_qkv.device, dtype=torch.uint8)
            check(lib.moma_mha_pack_weights(_ptr(w_qkv), _ptr(w_proj), _ptr(buf), d, int(need_t), _stream()),
                  "moma_mha_pack_weights")
            self.buf, self.key, self.has_t = buf, key, bool(need_t)
        return self.buf


def _mha_check(x, w_qkv, b_qkv, w_proj, b_proj, H):
    _dev(x, "x", None)
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"x: expected float32 or bfloat16, got {x.dtype}")
    for t, nm in ((w_qkv, "qkv.weight"), (w_proj, "proj.weight"), (b_proj, "proj.bias")):
        _dev(t, nm)
    if b_qkv is not None:
        _dev(b_qkv, "qkv.bias")
    N, d = x.shape
    if w_qkv.shape != (3 * d, d) or w_proj.shape != (d, d) or d % H:
        raise ValueError(f"bad attention shapes: x {tuple(x.shape)} Wqkv {tuple(w_qkv.shape)} H={H}")
    return N, d


def _mha_fast_fwd(items, H, want_lse, qpacks=None):
    """One grouped moma_mha_fwd_fast call.  items: [(x, pack, b_qkv, b_proj)], equal shapes.  -> [(y, qkv16, attn16, lse)]"""
    lib = _lib.load()
    N, d = items[0][0].shape
    dev = items[0][0].device
    mods = (_lib.MhaModule * len(items))()
    outs = []
    for i, (x, pack, b_qkv, b_proj) in enumerate(items):
        y = torch.empty(N, d, device=dev, dtype=torch.float32)
        qkv16 = torch.empty(N, 3 * d, device=dev, dtype=torch.bfloat16)
        attn16 = torch.empty(N, d, device=dev, dtype=torch.bfloat16)
        lse = torch.empty(H, N, device=dev, dtype=torch.float32) if want_lse else None
        qp = qpacks[i] if qpacks is not None else None       # a prepared QPack
        m = mods[i]
        m.x, m.pack, m.b_qkv, m.b_proj = x.data_ptr(), pack.data_ptr(), (0 if b_qkv is None else b_qkv.data_ptr()), b_proj.data_ptr()
        m.y, m.qkv16, m.attn16, m.lse = y.data_ptr(), qkv16.data_ptr(), attn16.data_ptr(), (0 if lse is None else lse.data_ptr())
        m.qpack, m.qpack_scale = (0, 0.0) if qp is None else (qp.buf.data_ptr(), float(qp.scale))
        m.x_dtype = DT_BF16 if x.dtype == torch.bfloat16 else DT_F32
        outs.append((y, qkv16, attn16, lse))
    with _timed("moma_mha_fwd" if len(items) == 1 else f"moma_mha_fwd_group{len(items)}"):
        check(lib.moma_mha_fwd_fast(C.cast(mods, C.c_void_p), len(items), N, d, H, _stream()), "moma_mha_fwd_fast")
    return outs


class _MHA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_qkv, b_qkv, w_proj, b_proj, H, prec, grad_mode, holder, qpack):
        lib = _lib.load()
        x = x.contiguous()
        N, d = _mha_check(x, w_qkv, b_qkv, w_proj, b_proj, H)
        dev = x.device
        ctx.x_dtype = x.dtype
        need_bwd = grad_mode and any(ctx.needs_input_grad)      # (grad mode is always off inside forward)
        fast = lib.moma_mha_saved_state(N, d, H, prec) == _lib.MHA_SAVE_LSE
        ctx.H, ctx.prec, ctx.has_bqkv, ctx.fast = H, prec, b_qkv is not None, fast
        if fast:
            # bf16 fast path: the forward keeps qkv / attn_out as bf16 and the row log-sum-exp [H,N]; P is recomputed per tile
            pack = (holder if holder is not None else MhaPack()).get(w_qkv, w_proj, need_bwd)
            (y, qkv16, attn16, lse), = _mha_fast_fwd([(x, pack, b_qkv, b_proj)], H, need_bwd,
                                                     None if qpack is None else [qpack])
            if need_bwd:
                ctx.save_for_backward(x, pack, qkv16, attn16, lse)
            if qpack is not None:
                qpack.written_from(y, qpack.T)
            return y
        x = x.float()                       # (a bf16 x is consumed as it stands by the fast path only; a packed-q request is dropped)
        # staged path (exact fp32, odd head dims): keeps the probabilities [H,N,N]
        y = torch.empty(N, d, device=dev, dtype=torch.float32)
        qkv = torch.empty(N, 3 * d, device=dev, dtype=torch.float32)
        probs = torch.empty(H, N, N, device=dev, dtype=torch.float32)
        attn_out = torch.empty(N, d, device=dev, dtype=torch.float32)
        with _timed("moma_mha_fwd"):
            check(lib.moma_mha_fwd(_ptr(x), _ptr(w_qkv), _ptr(b_qkv), _ptr(w_proj), _ptr(b_proj), _ptr(y), _ptr(qkv),
                                   _ptr(probs), _ptr(attn_out), N, d, H, prec, _stream()), "moma_mha_fwd")
        if need_bwd:
            ctx.save_for_backward(x, w_qkv, w_proj, qkv, probs, attn_out)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        dy = dy.contiguous()
        H = ctx.H
        need = ctx.needs_input_grad
        if ctx.fast:
            x, pack, qkv16, attn16, lse = ctx.saved_tensors
        else:
            x, w_qkv, w_proj, qkv, probs, attn_out = ctx.saved_tensors
        N, d = x.shape
        dev = x.device
        dx = torch.empty(N, d, device=dev, dtype=torch.float32) if need[0] else None
        dw_qkv = torch.empty(3 * d, d, device=dev, dtype=torch.float32) if need[1] else None
        db_qkv = torch.empty(3 * d, device=dev, dtype=torch.float32) if (need[2] and ctx.has_bqkv) else None
        dw_proj = torch.empty(d, d, device=dev, dtype=torch.float32) if need[3] else None
        db_proj = torch.empty(d, device=dev, dtype=torch.float32) if need[4] else None
        if ctx.fast:
            # a bias gradient rides on its weight gradient's launch: compute the weight gradient too if only the bias wants one
            t_wq = dw_qkv if (dw_qkv is not None or db_qkv is None) else torch.empty(3 * d, d, device=dev, dtype=torch.float32)
            t_wp = dw_proj if (dw_proj is not None or db_proj is None) else torch.empty(d, d, device=dev, dtype=torch.float32)
            ws = torch.empty(lib.moma_mha_bwd_fast_workspace_bytes(N, d, H), device=dev, dtype=torch.uint8)
            with _timed("moma_mha_bwd"):
                check(lib.moma_mha_bwd_fast(_ptr(pack), _ptr(x), DT_BF16 if x.dtype == torch.bfloat16 else DT_F32, _ptr(qkv16), _ptr(attn16), _ptr(lse), _ptr(dy), _ptr(dx),
                                            _ptr(t_wq), _ptr(db_qkv), _ptr(t_wp), _ptr(db_proj), _ptr(ws), ws.numel(), N, d, H,
                                            _stream()), "moma_mha_bwd_fast")
        else:
            ws = torch.empty(lib.moma_mha_bwd_workspace_bytes(N, d, H, ctx.prec), device=dev, dtype=torch.uint8)
            with _timed("moma_mha_bwd"):
                check(lib.moma_mha_bwd(_ptr(x), _ptr(w_qkv), _ptr(w_proj), _ptr(qkv), _ptr(probs), _ptr(attn_out),
                                       _ptr(dy), _ptr(dx), _ptr(dw_qkv), _ptr(db_qkv), _ptr(dw_proj), _ptr(db_proj), _ptr(ws),
                                       ws.numel(), N, d, H, ctx.prec, _stream()), "moma_mha_bwd")
        if dx is not None and dx.dtype != ctx.x_dtype:
            dx = dx.to(ctx.x_dtype)
        return dx, dw_qkv, db_qkv, dw_proj, db_proj, None, None, None, None, None


def mha(x, w_qkv, b_qkv, w_proj, b_proj, num_heads: int, prec="fp32", pack: "MhaPack | None" = None, qpack=None) -> torch.Tensor:
    """Attention.forward.  pack: the module's MhaPack (bf16 weight cache of the fast path; a throw-away one is built when
    omitted).  qpack: None, or a QPack prepared for (N, d, T): the fast path also writes y in K2's packed-Q layout (on the
    staged path the request is dropped and K2 packs q itself)."""
    return _MHA.apply(x, w_qkv, b_qkv, w_proj, b_proj, int(num_heads), prec_code(prec), torch.is_grad_enabled(), pack, qpack)


def mha_group(calls, num_heads: int, prec="fp32"):
    """Forward of several attention modules in ONE group of launches (no autograd): calls = [(x, w_qkv, b_qkv, w_proj,
    b_proj, pack)].  Falls back to one call per module when the fast path does not take the configuration, the shapes
    differ, or a gradient is wanted."""
    lib = _lib.load()
    pc = prec_code(prec)
    xs = [c[0].contiguous() for c in calls]
    same = all(x.shape == xs[0].shape for x in xs) and 1 < len(calls) <= 4
    wants_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for c in calls for t in c[:5])
    if not same or wants_grad or lib.moma_mha_saved_state(xs[0].shape[0], xs[0].shape[1], int(num_heads), pc) != _lib.MHA_SAVE_LSE:
        return [mha(c[0], c[1], c[2], c[3], c[4], num_heads, prec, c[5]) for c in calls]
    items = []
    for x, c in zip(xs, calls):
        _mha_check(x, c[1], c[2], c[3], c[4], int(num_heads))
        holder = c[5] if c[5] is not None else MhaPack()
        items.append((x, holder.get(c[1], c[3], False), c[2], c[4]))
    return [o[0] for o in _mha_fast_fwd(items, int(num_heads), False)]


# ------------------------------------------------------------------------------------------------
# BatchNorm2d + fused activation on NCHW activations (backbone helper, include/moma_hip.h "BN")
# ------------------------------------------------------------------------------------------------
ACT_CODES = {None: 0, "none": 0, "silu": 1, "relu": 2}
_DT_CODES = {torch.float32: 0, torch.bfloat16: 1}


class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, act, want_mean):
        lib = _lib.load()
        _dev(x, "x", dtype=None, contiguous=False)
        if x.dim() < 2 or x.dtype not in _DT_CODES:
            raise ValueError(f"bn_act: expects [N, C, ...] float32 / bfloat16, got {tuple(x.shape)} {x.dtype}")
        x = x.contiguous()
        N, Cc = x.shape[0], x.shape[1]
        HW = x.numel() // (N * Cc)
        dev = x.device
        out = torch.empty_like(x)
        save_mean = torch.empty(Cc, device=dev, dtype=torch.float32)
        save_invstd = torch.empty(Cc, device=dev, dtype=torch.float32)
        ws = torch.empty(lib.moma_bn_workspace_bytes(Cc), device=dev, dtype=torch.uint8)
        pmean = torch.empty(N, Cc, 1, 1, device=dev, dtype=x.dtype) if want_mean else None
        check(lib.moma_bn_fwd(_ptr(x), _ptr(out), _ptr(weight), _ptr(bias), _ptr(running_mean), _ptr(running_var),
                              _ptr(save_mean), _ptr(save_invstd), _ptr(ws), ws.numel(), N, Cc, HW, _DT_CODES[x.dtype],
                              act, int(training), float(momentum), float(eps), _ptr(pmean), _stream()), "moma_bn_fwd")
        ctx.save_for_backward(x, weight, bias, save_mean, save_invstd)
        ctx.cfg = (N, Cc, HW, act, int(training))
        ctx.set_materialize_grads(False)
        return (out, pmean) if want_mean else out

    @staticmethod
    def backward(ctx, dout, dmean=None):
        lib = _lib.load()
        x, weight, bias, save_mean, save_invstd = ctx.saved_tensors
        N, Cc, HW, act, training = ctx.cfg
        if dout is None:
            dout = torch.zeros_like(x)
        dout = dout.contiguous()
        if dout.dtype != x.dtype:
            dout = dout.to(x.dtype)
        if dmean is not None:
            dmean = dmean.to(x.dtype).contiguous()
        dev = x.device
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dgamma = torch.empty(Cc, device=dev, dtype=torch.float32) if (weight is not None and ctx.needs_input_grad[1]) else None
        dbeta = torch.empty(Cc, device=dev, dtype=torch.float32) if (bias is not None and ctx.needs_input_grad[2]) else None
        ws = torch.empty(lib.moma_bn_workspace_bytes(Cc), device=dev, dtype=torch.uint8)
        check(lib.moma_bn_bwd(_ptr(x), _ptr(dout), _ptr(weight), _ptr(bias), _ptr(save_mean), _ptr(save_invstd), _ptr(dx),
                              _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel(), N, Cc, HW, _DT_CODES[x.dtype], act,
                              training, _ptr(dmean), _stream()), "moma_bn_bwd")
        return dx, dgamma, dbeta, None, None, None, None, None, None, None


def bn_act(x, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float, act=None,
           want_mean: bool = False):
    """act(batch_norm(x)) on a contiguous NCHW tensor; running statistics are updated in place when training.
    want_mean: also return the [N,C,1,1] per-plane mean of the result (the squeeze of a squeeze-excite block)."""
    return _BNAct.apply(x, weight, bias, running_mean, running_var, bool(training), momentum, eps, ACT_CODES[act],
                        bool(want_mean))


# ------------------------------------------------------------------------------------------------
# Depthwise convolution on NCHW activations (backbone helper, include/moma_hip.h "DW")
# ------------------------------------------------------------------------------------------------
class _DWConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, pad_top, pad_left, out_h, out_w):
        lib = _lib.load()
        _dev(x, "x", dtype=None, contiguous=False)
        _dev(w, "weight")
        if x.dim() != 4 or x.dtype not in _DT_CODES or w.dim() != 4 or w.shape[1] != 1 or w.shape[0] != x.shape[1] \
                or w.shape[2] != w.shape[3]:
            raise ValueError(f"dwconv: x {tuple(x.shape)} {x.dtype}, weight {tuple(w.shape)}")
        x = x.contiguous()
        w = w.contiguous()
        N, Cc, H, W = x.shape
        K = w.shape[2]
        y = torch.empty(N, Cc, out_h, out_w, device=x.device, dtype=x.dtype)
        check(lib.moma_dwconv_fwd(_ptr(x), _ptr(w), _ptr(y), N, Cc, H, W, out_h, out_w, K, stride, pad_top, pad_left,
                                  _DT_CODES[x.dtype], _stream()), "moma_dwconv_fwd")
        ctx.save_for_backward(x, w)
        ctx.cfg = (N, Cc, H, W, out_h, out_w, K, stride, pad_top, pad_left)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        N, Cc, H, W, OH, OW, K, stride, pt, pl = ctx.cfg
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(lib.moma_dwconv_bwd_data(_ptr(dy), _ptr(w), _ptr(dx), N, Cc, H, W, OH, OW, K, stride, pt, pl,
                                           _DT_CODES[x.dtype], _stream()), "moma_dwconv_bwd_data")
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            ws = torch.empty(lib.moma_dwconv_workspace_bytes(Cc, K), device=x.device, dtype=torch.uint8)
            check(lib.moma_dwconv_bwd_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), ws.numel(), N, Cc, H, W, OH, OW, K,
                                             stride, pt, pl, _DT_CODES[x.dtype], _stream()), "moma_dwconv_bwd_weight")
        return dx, dw, None, None, None, None, None


def dwconv_supported(kernel: int, stride: int) -> bool:
    return kernel in (3, 5) and stride in (1, 2)


def dwconv(x, weight, stride: int, pad_top: int, pad_left: int, out_h: int, out_w: int):
    """Depthwise conv2d, weight [C,1,K,K] fp32, explicit (possibly asymmetric) zero padding given by the top/left pad
    and the output size."""
    return _DWConv.apply(x, weight, int(stride), int(pad_top), int(pad_left), int(out_h), int(out_w))


# ------------------------------------------------------------------------------------------------
# Pointwise (1 x 1) convolution on NCHW activations: the weight gradient on the library's split-K MFMA kernel, forward and
# input gradient of the bias-free layers on its streaming MFMA kernel (backbone helper, include/moma_hip.h "PW")
# ------------------------------------------------------------------------------------------------
def pwconv_native(N: int, Cin: int, Cout: int, HW: int) -> bool:
    """Shape classes whose weight gradient the native kernel takes; the others keep MIOpen's solver.  By the layer table of
    DESIGN.md 5a (profiles/pw_layer_microbench.txt): planes whose rows allow 8- or 16-byte loads (HW a multiple of 4: 112^2 ..
    14^2) and the 1 x 1 planes of the squeeze-excite layers win 1.3 - 4 x; the 7 x 7 layers (49-pixel rows, 2-byte aligned:
    element loads) lose 2.5 - 4.5 x and stay with MIOpen."""
    return HW == 1 or HW % 4 == 0


def pwconv_bwd_weight(x, dy):
    """dw [Cout, Cin, 1, 1] bf16 = sum over images and pixels of dy (x) x for x [N, Cin, H, W], dy [N, Cout, H, W] (bf16, any
    strides: both are made dense NCHW).  Bitwise reproducible; no host synchronisation (safe under graph capture)."""
    lib = _lib.load()
    _dev(x, "x", dtype=torch.bfloat16, contiguous=False)
    _dev(dy, "dy", dtype=torch.bfloat16, contiguous=False)
    if x.dim() != 4 or dy.dim() != 4 or x.shape[0] != dy.shape[0] or x.shape[2:] != dy.shape[2:]:
        raise ValueError(f"pwconv_bwd_weight: x {tuple(x.shape)}, dy {tuple(dy.shape)}")
    x = x.contiguous()
    dy = dy.contiguous()
    N, Cin, H, W = x.shape
    Cout = dy.shape[1]
    dw = torch.empty(Cout, Cin, 1, 1, device=x.device, dtype=torch.bfloat16)
    ws = torch.empty(lib.moma_pwconv_workspace_bytes(N, Cin, Cout, H * W), device=x.device, dtype=torch.uint8)
    check(lib.moma_pwconv_bwd_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), ws.numel(), N, Cin, Cout, H * W, DT_BF16, _stream()),
          "moma_pwconv_bwd_weight")
    return dw


def pwconv_fwd_native(N: int, Cin: int, Cout: int, HW: int) -> bool:
    """Shape classes whose bias-free forward and input gradient (Cin and Cout as the layer has them: one table serves both) the
    streaming kernel takes; the others keep MIOpen's GEMMs.  By the layer table of DESIGN.md 5a
    (profiles/pwfwd_layer_microbench.txt, B = 256): planes whose rows allow 8- or 16-byte accesses (HW a multiple of 4: 112^2 ..
    14^2) win 1.4 - 3.7 x forward (672 -> 112: 1.09 x) and 1.3 - 3.9 x backward (112 -> 672: at parity, 1.02 x); the 7 x 7 layers
    (49-pixel rows: element accesses) lose up to 1.7 x and stay with MIOpen, as do the 1 x 1 planes of the squeeze-excite layers
    (a bias, negligible bytes).  The batch does not enter: the class is the layer's, smaller batches were not timed.
    Layers of at most 16 output channels (32 -> 16 on 112^2) stay although the kernel is 3 x faster there: MIOpen's solver for
    them is the one whose results differ from the kernel's (every other routed layer agrees with MIOpen bit for bit on the
    table's data), and with it replaced the seeded step's outputs moved by eight times their run-to-run difference."""
    return HW > 1 and HW % 4 == 0 and Cout > 16


def _pw_stream(entry, x, w, transposed):
    lib = _lib.load()
    _dev(x, "x", dtype=torch.bfloat16, contiguous=False)
    _dev(w, "weight", dtype=torch.bfloat16, contiguous=False)
    if x.dim() != 4 or w.dim() != 4 or w.shape[2:] != (1, 1):
        raise ValueError(f"{entry}: x {tuple(x.shape)}, weight {tuple(w.shape)}")
    x = x.contiguous()
    w = w.contiguous()
    N, _, H, W = x.shape
    Cout, Cin = w.shape[:2]
    if x.shape[1] != (Cout if transposed else Cin):
        raise ValueError(f"{entry}: x {tuple(x.shape)}, weight {tuple(w.shape)}")
    y = torch.empty(N, Cin if transposed else Cout, H, W, device=x.device, dtype=torch.bfloat16)
    check(getattr(lib, entry)(_ptr(x), _ptr(w), _ptr(y), N, Cin, Cout, H * W, DT_BF16, _stream()), entry)
    return y


def pwconv_fwd(x, w):
    """y [N, Cout, H, W] bf16 = conv2d(x, w) for w [Cout, Cin, 1, 1], no bias, on the streaming kernel (x, w bf16).  A dense NCHW
    x is read where it lies; any other layout (channels-last, a strided view) is first copied dense, an activation-sized pass of
    its own.  Bitwise reproducible; no host synchronisation (safe under graph capture)."""
    return _pw_stream("moma_pwconv_fwd", x, w, False)


def pwconv_bwd_data(dy, w):
    """dx [N, Cin, H, W] bf16 of the same convolution from dy [N, Cout, H, W]; the weight is read transposed in place."""
    return _pw_stream("moma_pwconv_bwd_data", dy, w, True)


class _PWConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, native_fwd, native_wgrad):
        _dev(x, "x", dtype=torch.bfloat16, contiguous=False)
        _dev(w, "weight", dtype=torch.bfloat16, contiguous=False)
        if x.dim() != 4 or w.dim() != 4 or w.shape[1] != x.shape[1] or w.shape[2:] != (1, 1):
            raise ValueError(f"pwconv: x {tuple(x.shape)}, weight {tuple(w.shape)}")
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        ctx.native_wgrad = bool(native_wgrad)
        N, Cin, H, W = x.shape
        # forward and input gradient on the streaming kernel: bias-free layers of the shape classes that win there
        ctx.native_fwd = bool(native_fwd) and b is None and pwconv_fwd_native(N, Cin, w.shape[0], H * W)
        if ctx.native_fwd:
            return pwconv_fwd(x, w)
        return torch.nn.functional.conv2d(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if ctx.native_fwd:
                dx = pwconv_bwd_data(dy, w)
            else:
                dx = torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                         [True, False, False])[0]
        if ctx.needs_input_grad[1]:
            N, Cin, H, W = x.shape
            if ctx.native_wgrad and pwconv_native(N, Cin, w.shape[0], H * W):
                dw = pwconv_bwd_weight(x, dy)
            else:
                dw = torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                         [False, True, False])[1]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum((0, 2, 3))
        return dx, dw, db, None, None


def pwconv(x, w, b=None, native_fwd=True, native_wgrad=True):
    """conv2d with a [Cout, Cin, 1, 1] weight (stride 1, no padding) on bf16 NCHW activations.  With `native_wgrad` the weight
    gradient runs on the split-K kernel (pwconv_native); without a bias and with `native_fwd`, forward and input gradient run on
    the streaming kernel where pwconv_fwd_native holds.  Everything else is the stock path."""
    return _PWConv.apply(x, w, b, native_fwd, native_wgrad)


# ------------------------------------------------------------------------------------------------
# BatchNorm2d + activation applied INSIDE the depthwise convolution that consumes it (the _bn0 -> _depthwise_conv
# pair of an MBConv block): the activation tensor between the two is never written
# ------------------------------------------------------------------------------------------------
class _BNActDWConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, act, w, stride, pad_top,
                pad_left, out_h, out_w):
        lib = _lib.load()
        _dev(x, "x", dtype=None, contiguous=False)
        _dev(w, "weight")
        if x.dim() != 4 or x.dtype not in _DT_CODES or w.dim() != 4 or w.shape[1] != 1 or w.shape[0] != x.shape[1] \
                or w.shape[2] != w.shape[3]:
            raise ValueError(f"bn_act_dwconv: x {tuple(x.shape)} {x.dtype}, weight {tuple(w.shape)}")
        x = x.contiguous()
        w = w.contiguous()
        N, Cc, H, W = x.shape
        K = w.shape[2]
        dev = x.device
        save_mean = torch.empty(Cc, device=dev, dtype=torch.float32)
        save_invstd = torch.empty(Cc, device=dev, dtype=torch.float32)
        scale_shift = torch.empty(Cc, 2, device=dev, dtype=torch.float32)
        ws = torch.empty(lib.moma_bn_workspace_bytes(Cc), device=dev, dtype=torch.uint8)
        check(lib.moma_bn_prepare(_ptr(x), _ptr(weight), _ptr(bias), _ptr(running_mean), _ptr(running_var), _ptr(save_mean),
                                  _ptr(save_invstd), _ptr(scale_shift), _ptr(ws), ws.numel(), N, Cc, H * W,
                                  _DT_CODES[x.dtype], int(training), float(momentum), float(eps), _stream()), "moma_bn_prepare")
        y = torch.empty(N, Cc, out_h, out_w, device=dev, dtype=x.dtype)
        check(lib.moma_dwconv_fwd_pre(_ptr(x), _ptr(w), _ptr(y), N, Cc, H, W, out_h, out_w, K, stride, pad_top, pad_left,
                                      _DT_CODES[x.dtype], _ptr(scale_shift), act, _stream()), "moma_dwconv_fwd_pre")
        ctx.save_for_backward(x, weight, bias, save_mean, save_invstd, scale_shift, w)
        ctx.cfg = (N, Cc, H, W, out_h, out_w, K, stride, pad_top, pad_left, act, int(training))
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, weight, bias, save_mean, save_invstd, scale_shift, w = ctx.saved_tensors
        N, Cc, H, W, OH, OW, K, stride, pt, pl, act, training = ctx.cfg
        dx = dgamma = dbeta = dw = None
        if dy is None:
            return (None,) * 15
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        dev, dt = x.device, _DT_CODES[x.dtype]
        want_gamma = weight is not None and ctx.needs_input_grad[1]
        want_beta = bias is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[0] or want_gamma or want_beta:
            da = torch.empty_like(x)            # gradient w.r.t. the activation that was never stored
            check(lib.moma_dwconv_bwd_data(_ptr(dy), _ptr(w), _ptr(da), N, Cc, H, W, OH, OW, K, stride, pt, pl, dt,
                                           _stream()), "moma_dwconv_bwd_data")
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            dgamma = torch.empty(Cc, device=dev, dtype=torch.float32) if want_gamma else None
            dbeta = torch.empty(Cc, device=dev, dtype=torch.float32) if want_beta else None
            ws = torch.empty(lib.moma_bn_workspace_bytes(Cc), device=dev, dtype=torch.uint8)
            check(lib.moma_bn_bwd(_ptr(x), _ptr(da), _ptr(weight), _ptr(bias), _ptr(save_mean), _ptr(save_invstd), _ptr(dx),
                                  _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel(), N, Cc, H * W, dt, act, training, None,
                                  _stream()), "moma_bn_bwd")
        if ctx.needs_input_grad[9]:
            dw = torch.empty_like(w)
            ws = torch.empty(lib.moma_dwconv_workspace_bytes(Cc, K), device=dev, dtype=torch.uint8)
            check(lib.moma_dwconv_bwd_weight_pre(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), ws.numel(), N, Cc, H, W, OH, OW, K,
                                                 stride, pt, pl, dt, _ptr(scale_shift), act, _stream()),
                  "moma_dwconv_bwd_weight_pre")
        return dx, dgamma, dbeta, None, None, None, None, None, None, dw, None, None, None, None, None


def bn_act_dwconv(x, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float, act, w_dw,
                  stride: int, pad_top: int, pad_left: int, out_h: int, out_w: int):
    """dwconv(bn_act(x, ...), w_dw, ...) bit for bit, in one pass less over x and without the tensor in between: the
    depthwise kernels normalise and activate every element as they read it.  Running statistics are updated in place
    when training; the backward keeps x and the statistics only."""
    return _BNActDWConv.apply(x, weight, bias, running_mean, running_var, bool(training), momentum, eps, ACT_CODES[act],
                              w_dw, int(stride), int(pad_top), int(pad_left), int(out_h), int(out_w))


# ------------------------------------------------------------------------------------------------
# Squeeze-excite helpers (include/moma_hip.h "SE")
# ------------------------------------------------------------------------------------------------
class _PlaneMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        _dev(x, "x", dtype=None, contiguous=False)
        if x.dim() != 4 or x.dtype not in _DT_CODES:
            raise ValueError(f"plane_mean: expects [N,C,H,W] float32 / bfloat16, got {tuple(x.shape)} {x.dtype}")
        x = x.contiguous()
        N, Cc, H, W = x.shape
        out = torch.empty(N, Cc, 1, 1, device=x.device, dtype=x.dtype)
        check(lib.moma_plane_mean(_ptr(x), _ptr(out), N * Cc, H * W, _DT_CODES[x.dtype], _stream()), "moma_plane_mean")
        ctx.shape = (N, Cc, H, W)
        return out

    @staticmethod
    def backward(ctx, dmean):
        N, Cc, H, W = ctx.shape
        return (dmean / (H * W)).expand(N, Cc, H, W)          # a stride-0 view: nothing is materialised here


class _SEGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        lib = _lib.load()
        _dev(x, "x", dtype=None, contiguous=False)
        _dev(s, "s", dtype=None, contiguous=False)
        if x.dim() != 4 or x.dtype not in _DT_CODES or s.numel() != x.shape[0] * x.shape[1]:
            raise ValueError(f"se_gate: x {tuple(x.shape)} {x.dtype}, s {tuple(s.shape)}")
        x = x.contiguous()
        s = s.to(x.dtype).contiguous()
        N, Cc, H, W = x.shape
        out = torch.empty_like(x)
        check(lib.moma_se_gate_fwd(_ptr(x), _ptr(s), _ptr(out), N * Cc, H * W, _DT_CODES[x.dtype], _stream()), "moma_se_gate_fwd")
        ctx.save_for_backward(x, s)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, s = ctx.saved_tensors
        N, Cc, H, W = x.shape
        dout = dout.contiguous()
        if dout.dtype != x.dtype:
            dout = dout.to(x.dtype)
        dx = torch.empty_like(x)
        ds = torch.empty_like(s)
        check(lib.moma_se_gate_bwd(_ptr(x), _ptr(s), _ptr(dout), _ptr(dx), _ptr(ds), N * Cc, H * W, _DT_CODES[x.dtype],
                                   _stream()), "moma_se_gate_bwd")
        return dx, ds


def plane_mean(x):
    """[N,C,H,W] -> [N,C,1,1] mean over each plane (F.adaptive_avg_pool2d(x, 1))."""
    return _PlaneMean.apply(x)


def se_gate(x, s):
    """x * sigmoid(s) with s [N,C,1,1]."""
    return _SEGate.apply(x, s)


# ------------------------------------------------------------------------------------------------
# BatchNorm2d + activation applied INSIDE the squeeze-excite gate that consumes it (the _bn1 -> SE pair of an MBConv
# block, include/moma_hip.h "BN"): the activation between the two is neither written nor kept for the backward
# ------------------------------------------------------------------------------------------------
class _BNSELink:
    """What bn_act_mean hands to bn_act_gate next to the scale / shift tensor, and where the gate's backward parks the gate's
    gradient until the BatchNorm's backward (which always runs after it: the link tensor is one of its outputs) picks it up."""

    __slots__ = ("act", "training", "save_mean", "save_invstd", "pending")

    def __init__(self, act, training, save_mean, save_invstd):
        self.act, self.training, self.save_mean, self.save_invstd = act, training, save_mean, save_invstd
        self.pending = None                 # (dG, s, workspace with the plane sums)

    def clear(self):
        self.pending = None


def _cuda_act(x, name, op):
    _dev(x, name, dtype=None, contiguous=False)
    if x.dim() != 4 or x.dtype not in _DT_CODES:
        raise ValueError(f"{op}: expects [N,C,H,W] float32 / bfloat16, got {tuple(x.shape)} {x.dtype}")


class _BNActMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, weight, bias, running_mean, running_var, momentum, eps, meta):
        lib = _lib.load()
        d = d.contiguous()
        N, Cc, H, W = d.shape
        dev = d.device
        scale_shift = torch.empty(Cc, 2, device=dev, dtype=torch.float32)
        pooled = torch.empty(N, Cc, 1, 1, device=dev, dtype=d.dtype)
        ws = torch.empty(lib.moma_bn_workspace_bytes(Cc), device=dev, dtype=torch.uint8)
        check(lib.moma_bn_act_mean(_ptr(d), _ptr(weight), _ptr(bias), _ptr(running_mean), _ptr(running_var),
                                   _ptr(meta.save_mean), _ptr(meta.save_invstd), _ptr(scale_shift), _ptr(pooled), _ptr(ws),
                                   ws.numel(), N, Cc, H * W, _DT_CODES[d.dtype], meta.act, meta.training, float(momentum),
                                   float(eps), _stream()), "moma_bn_act_mean")
        ctx.save_for_backward(d, weight, bias, scale_shift)
        ctx.meta = meta
        ctx.set_materialize_grads(False)
        return pooled, scale_shift

    @staticmethod
    def backward(ctx, dpl, _dlink):
        lib = _lib.load()
        d, weight, bias, scale_shift = ctx.saved_tensors
        meta = ctx.meta
        N, Cc, H, W = d.shape
        dev, dt = d.device, _DT_CODES[d.dtype]
        pending, meta.pending = meta.pending, None
        if dpl is not None:
            dpl = dpl.to(d.dtype).contiguous()
        dx = torch.empty_like(d) if ctx.needs_input_grad[0] else None
        dgamma = torch.empty(Cc, device=dev, dtype=torch.float32) if (weight is not None and ctx.needs_input_grad[1]) else None
        dbeta = torch.empty(Cc, device=dev, dtype=torch.float32) if (bias is not None and ctx.needs_input_grad[2]) else None
        if pending is None:
            # the gate took no part in the loss: only the plane means carry a gradient -- the plain BatchNorm backward
            if dpl is None:
                return (None,) * 8
            ws = torch.empty(lib.moma_bn_workspace_bytes(Cc), device=dev, dtype=torch.uint8)
            check(lib.moma_bn_bwd(_ptr(d), _ptr(torch.zeros_like(d)), _ptr(weight), _ptr(bias), _ptr(meta.save_mean),
                                  _ptr(meta.save_invstd), _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel(), N, Cc, H * W,
                                  dt, meta.act, meta.training, _ptr(dpl), _stream()), "moma_bn_bwd")
            return dx, dgamma, dbeta, None, None, None, None, None
        dG, s, ws = pending
        check(lib.moma_bn_gate_bwd(_ptr(d), _ptr(dG), _ptr(s), _ptr(dpl), _ptr(scale_shift), _ptr(meta.save_mean),
                                   _ptr(meta.save_invstd), _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel(), N, Cc,
                                   H * W, dt, meta.act, meta.training, _stream()), "moma_bn_gate_bwd")
        return dx, dgamma, dbeta, None, None, None, None, None


class _BNActGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, link, s, meta):
        lib = _lib.load()
        d = d.contiguous()
        s_in_dtype = s.dtype
        s = s.to(d.dtype).contiguous()
        N, Cc, H, W = d.shape
        out = torch.empty_like(d)
        check(lib.moma_bn_act_gate_fwd(_ptr(d), _ptr(link), _ptr(s), _ptr(out), N, Cc, H * W, _DT_CODES[d.dtype], meta.act,
                                       _stream()), "moma_bn_act_gate_fwd")
        ctx.save_for_backward(d, link, s)
        ctx.meta, ctx.s_dtype = meta, s_in_dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        d, link, s = ctx.saved_tensors
        meta = ctx.meta
        N, Cc, H, W = d.shape
        dout = dout.contiguous()
        if dout.dtype != d.dtype:
            dout = dout.to(d.dtype)
        ds = torch.empty_like(s) if ctx.needs_input_grad[2] else None
        ws = torch.empty(lib.moma_bn_gate_workspace_bytes(N, Cc), device=d.device, dtype=torch.uint8)
        check(lib.moma_bn_gate_bwd_sums(_ptr(d), _ptr(dout), _ptr(s), _ptr(link), _ptr(meta.save_mean), _ptr(meta.save_invstd),
                                        _ptr(ds), _ptr(ws), ws.numel(), N, Cc, H * W, _DT_CODES[d.dtype], meta.act, _stream()),
              "moma_bn_gate_bwd_sums")
        dlink = None
        if ctx.needs_input_grad[1]:
            # the BatchNorm's backward finishes the job (dD comes out once, there, with the gradient of the plane means folded in);
            # the link's "gradient" only makes autograd run it: a zero-stride view, its values are never read
            meta.pending = (dout, s, ws)
            # should this pass never reach the BatchNorm's node (a gradient asked of s alone), nothing stays parked behind it
            torch.autograd.Variable._execution_engine.queue_callback(meta.clear)
            dlink = meta.save_mean[:1].expand(Cc, 2)
        if ds is not None and ds.dtype != ctx.s_dtype:
            ds = ds.to(ctx.s_dtype)
        return None, dlink, ds, None


def bn_se_native(HW: int, records_grad: bool) -> bool:
    """Plane sizes at which an MBConv block takes the fused pair below instead of bn_act + se_gate.  By the layer table of
    DESIGN.md 5a (profiles/bnse_layer_microbench.txt, B = 256): one wave walks one plane, which streams at 3.4 - 4 TB/s on planes
    of 56 x 56 and up (forward x 1.33 - 1.39, forward + backward x 1.34 - 1.38) and still wins forward + backward at 28 x 28
    (x 1.06 - 1.15; the forward alone is a tie there); on the 14 x 14 and 7 x 7 planes a wave has at most one vector per lane, the
    five wave-wide sums of the backward outweigh the passes they save (forward x 0.90 - 1.00, forward + backward x 0.77 - 0.96)
    and the two calls stay."""
    return HW >= (28 * 28 if records_grad else 56 * 56)


def bn_act_mean(d, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float, act=None):
    """The squeeze of act(batch_norm(d)) without the activation tensor: (pooled [N,C,1,1], link).  `pooled` and the running
    statistics (updated in place when training) are those of bn_act(..., want_mean=True) bit for bit; `link` (the per-channel
    scale / shift, [C, 2] fp32) goes to bn_act_gate together with the same d."""
    _cuda_act(d, "d", "bn_act_mean")
    Cc = d.shape[1]
    meta = _BNSELink(ACT_CODES[act], int(bool(training)), torch.empty(Cc, device=d.device, dtype=torch.float32),
                     torch.empty(Cc, device=d.device, dtype=torch.float32))
    pooled, link = _BNActMean.apply(d, weight, bias, running_mean, running_var, momentum, eps, meta)
    link._moma_bnse = meta
    return pooled, link


def bn_act_gate(d, link, s):
    """act(batch_norm(d)) * sigmoid(s) for the (d, link) of bn_act_mean and s [N,C,1,1]: bit for bit
    se_gate(bn_act(d, ...), s), in one pass less forward and three less backward."""
    _cuda_act(d, "d", "bn_act_gate")
    _dev(s, "s", dtype=None, contiguous=False)
    meta = getattr(link, "_moma_bnse", None)
    if meta is None or s.numel() != d.shape[0] * d.shape[1] or tuple(link.shape) != (d.shape[1], 2):
        raise ValueError(f"bn_act_gate: d {tuple(d.shape)}, s {tuple(s.shape)}, link {tuple(link.shape)} (from bn_act_mean: "
                         f"{meta is not None})")
    return _BNActGate.apply(d, link, s, meta)


# ------------------------------------------------------------------------------------------------
# CRD: gather-contrast over two sample-indexed memory banks   (crd/memory.py:23-79, crd/criterion.py:57-74)
# ------------------------------------------------------------------------------------------------
def _crd_check(v1, v2, memory_v1, memory_v2, idx, n_data, Z, bad):
    _dev(v1, "v1"); _dev(v2, "v2"); _dev(memory_v1, "memory_v1"); _dev(memory_v2, "memory_v2")
    _dev(idx, "idx", torch.int64); _dev(Z, "Z"); _dev(bad, "bad_index", torch.int32)
    if (v1.dim() != 2 or v1.shape != v2.shape or memory_v1.dim() != 2 or memory_v1.shape != memory_v2.shape
            or memory_v1.shape[1] != v1.shape[1] or idx.dim() != 2 or idx.shape[0] != v1.shape[0]):
        raise ValueError(f"shape mismatch: v1 {tuple(v1.shape)} v2 {tuple(v2.shape)} memory_v1 {tuple(memory_v1.shape)} "
                         f"memory_v2 {tuple(memory_v2.shape)} idx {tuple(idx.shape)}")
    if int(n_data) != memory_v1.shape[0]:
        raise ValueError(f"n_data {n_data} != rows of the banks {memory_v1.shape[0]}")
    if Z.numel() != 2 or bad.numel() != 1:
        raise ValueError("Z must hold 2 floats (side 1, side 2) and bad_index one int32")


def _crd_workspace(lib, B, d, K1, dev):
    n = lib.moma_crd_workspace_bytes(B, d, K1)
    if n == 0:
        raise MomaHipError(f"moma_crd: unsupported shape B={B} d={d} K1={K1} (d a multiple of 4 up to 2048, nce_k >= 1)")
    return torch.empty(n, device=dev, dtype=torch.uint8), n


class _CRDFused(torch.autograd.Function):
    """Both sides in one gather pass: loss [2] and d loss / d v1, d loss / d v2 from the rows the pass already holds."""

    @staticmethod
    def forward(ctx, v1, v2, memory_v1, memory_v2, idx, T, n_data, Z, set_z, bad):
        lib = _lib.load()
        v1 = v1.contiguous() if isinstance(v1, torch.Tensor) else v1
        v2 = v2.contiguous() if isinstance(v2, torch.Tensor) else v2
        _crd_check(v1, v2, memory_v1, memory_v2, idx, n_data, Z, bad)
        B, d = v1.shape
        K1 = idx.shape[1]
        dev = v1.device
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss = torch.empty(2, device=dev, dtype=torch.float32)
        dv1 = torch.empty(B, d, device=dev, dtype=torch.float32) if need_grad else None
        dv2 = torch.empty(B, d, device=dev, dtype=torch.float32) if need_grad else None
        ws, ws_bytes = _crd_workspace(lib, B, d, K1, dev)
        with _timed("moma_crd_fused"):
            check(lib.moma_crd_fused(_ptr(v1), _ptr(v2), _ptr(memory_v1), _ptr(memory_v2), _ptr(idx), B, d, K1, int(n_data),
                                     float(T), _ptr(Z), int(bool(set_z)), _ptr(loss), _ptr(dv1), _ptr(dv2), _ptr(bad), _ptr(ws),
                                     ws_bytes, _stream()), "moma_crd_fused")
        if need_grad:
            ctx.save_for_backward(dv1, dv2)
        return loss

    @staticmethod
    def backward(ctx, g):
        dv1, dv2 = ctx.saved_tensors
        return (dv1 * g[0] if ctx.needs_input_grad[0] else None, dv2 * g[1] if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None, None, None)


def crd_fused(v1, v2, memory_v1, memory_v2, idx, T: float, n_data: int, Z, set_z: bool, bad=None) -> torch.Tensor:
    """-> loss [2] (side 1: v1 against memory_v2, side 2: v2 against memory_v1); the CRD loss is loss.sum().
    Z [2] float32 on the device: written first when set_z, read otherwise.  bad: int32 [1] on the device, set to 1 when an entry
    of idx is not a row of the banks (a fresh zero when None: the caller cannot read it then)."""
    if bad is None and isinstance(v1, torch.Tensor) and v1.is_cuda:
        bad = torch.zeros(1, device=v1.device, dtype=torch.int32)
    return _CRDFused.apply(v1, v2, memory_v1, memory_v2, idx, float(T), int(n_data), Z, bool(set_z), bad)


class _CRDScores(torch.autograd.Function):
    """The materialised scores ContrastMemory.forward returns, [B, K1] per side, with their backward."""

    @staticmethod
    def forward(ctx, v1, v2, memory_v1, memory_v2, idx, T, n_data, Z, set_z, bad, update_y):
        lib = _lib.load()
        v1 = v1.contiguous() if isinstance(v1, torch.Tensor) else v1
        v2 = v2.contiguous() if isinstance(v2, torch.Tensor) else v2
        _crd_check(v1, v2, memory_v1, memory_v2, idx, n_data, Z, bad)
        B, d = v1.shape
        K1 = idx.shape[1]
        dev = v1.device
        out_v1 = torch.empty(B, K1, device=dev, dtype=torch.float32)
        out_v2 = torch.empty(B, K1, device=dev, dtype=torch.float32)
        ws, ws_bytes = _crd_workspace(lib, B, d, K1, dev)
        with _timed("moma_crd_scores"):
            check(lib.moma_crd_scores(_ptr(v1), _ptr(v2), _ptr(memory_v1), _ptr(memory_v2), _ptr(idx), B, d, K1, int(n_data),
                                      float(T), _ptr(Z), int(bool(set_z)), _ptr(out_v1), _ptr(out_v2), _ptr(bad), _ptr(ws),
                                      ws_bytes, _stream()), "moma_crd_scores")
        # The reference's autograd keeps the gathered [B, K1, d] copy for the backward; here the backward gathers again, and the
        # banks are rewritten in between at the rows `update_y` (crd_update_ behind this call).  So the pre-update value of those
        # B rows is kept (B d floats per bank) and put back around the backward's gather.
        ctx.save_for_backward(out_v1, out_v2)
        ctx.banks, ctx.idx, ctx.bad, ctx.T, ctx.n_data = (memory_v1, memory_v2), idx, bad, T, n_data
        ctx.rows_at = ctx.old_rows = None
        if update_y is not None:
            ctx.rows_at = update_y.clamp(0, int(n_data) - 1)        # (an index that is no row never becomes an address)
            ctx.old_rows = (memory_v1.index_select(0, ctx.rows_at), memory_v2.index_select(0, ctx.rows_at))
        return out_v1, out_v2

    @staticmethod
    def backward(ctx, dout_v1, dout_v2):
        lib = _lib.load()
        out_v1, out_v2 = ctx.saved_tensors
        (memory_v1, memory_v2), idx, bad = ctx.banks, ctx.idx, ctx.bad
        B, K1 = out_v1.shape
        d = memory_v1.shape[1]
        dev = out_v1.device
        dout_v1 = dout_v1.contiguous(); dout_v2 = dout_v2.contiguous()
        dv1 = torch.empty(B, d, device=dev, dtype=torch.float32)
        dv2 = torch.empty(B, d, device=dev, dtype=torch.float32)
        ws, ws_bytes = _crd_workspace(lib, B, d, K1, dev)
        new_rows = None
        if ctx.old_rows is not None:
            with torch.no_grad():
                new_rows = (memory_v1.index_select(0, ctx.rows_at), memory_v2.index_select(0, ctx.rows_at))
                memory_v1.index_copy_(0, ctx.rows_at, ctx.old_rows[0]); memory_v2.index_copy_(0, ctx.rows_at, ctx.old_rows[1])
        with _timed("moma_crd_scores_bwd"):
            check(lib.moma_crd_scores_bwd(_ptr(dout_v1), _ptr(dout_v2), _ptr(out_v1), _ptr(out_v2), _ptr(memory_v1),
                                          _ptr(memory_v2), _ptr(idx), B, d, K1, int(ctx.n_data), float(ctx.T), _ptr(dv1), _ptr(dv2),
                                          _ptr(bad), _ptr(ws), ws_bytes, _stream()), "moma_crd_scores_bwd")
        if new_rows is not None:
            with torch.no_grad():
                memory_v1.index_copy_(0, ctx.rows_at, new_rows[0]); memory_v2.index_copy_(0, ctx.rows_at, new_rows[1])
        return dv1, dv2, None, None, None, None, None, None, None, None, None


def crd_scores(v1, v2, memory_v1, memory_v2, idx, T: float, n_data: int, Z, set_z: bool, bad=None, update_y=None):
    """-> (out_v1, out_v2), [B, K1] fp32: x of side 1 and of side 2.  The backward gathers the rows again from the banks;
    update_y: the rows (int64 [B]) that crd_update_ rewrites between this call and its backward -- their pre-update value is kept
    and stands in for them during the backward's gather."""
    if bad is None and isinstance(v1, torch.Tensor) and v1.is_cuda:
        bad = torch.zeros(1, device=v1.device, dtype=torch.int32)
    return _CRDScores.apply(v1, v2, memory_v1, memory_v2, idx, float(T), int(n_data), Z, bool(set_z), bad, update_y)


def crd_update_(memory_v1, memory_v2, v1, v2, y, momentum: float, bad=None) -> None:
    """Momentum update of both banks in one launch (moma_crd_update); issue it behind the gather of the same step."""
    lib = _lib.load()
    _dev(memory_v1, "memory_v1"); _dev(memory_v2, "memory_v2"); _dev(v1, "v1"); _dev(v2, "v2"); _dev(y, "y", torch.int64)
    if bad is None:
        bad = torch.zeros(1, device=v1.device, dtype=torch.int32)
    _dev(bad, "bad_index", torch.int32)
    B, d = v1.shape
    if v2.shape != v1.shape or memory_v1.shape != memory_v2.shape or memory_v1.shape[1] != d or y.shape != (B,):
        raise ValueError(f"shape mismatch: v1 {tuple(v1.shape)} v2 {tuple(v2.shape)} banks {tuple(memory_v1.shape)} / "
                         f"{tuple(memory_v2.shape)} y {tuple(y.shape)}")
    with trace_range("moma_crd_update"):
        check(lib.moma_crd_update(_ptr(memory_v1), _ptr(memory_v2), _ptr(v1), _ptr(v2), _ptr(y), B, d, memory_v1.shape[0],
                                  float(momentum), _ptr(bad), _stream()), "moma_crd_update")


# ------------------------------------------------------------------------------------------------
# Attention Transfer: spatial attention maps of a feature pair   (distiller_zoo/AT.py, helper/loops_moma.py:287-292)
# ------------------------------------------------------------------------------------------------
def _at_side(f, name, op="attention_loss"):
    """-> (dense tensor, layout code): contiguous NCHW and channels_last are taken as they are, any other dense layout is copied"""
    _dev(f, name, dtype=None, contiguous=False)
    if f.dim() != 4 or f.dtype not in _DT_CODES:
        raise TypeError(f"{op}: {name} must be a 4-D float32 / bfloat16 tensor, got {tuple(f.shape)} {f.dtype}")
    if f.is_contiguous():
        return f, _lib.LAYOUT_NCHW
    if f.is_contiguous(memory_format=torch.channels_last):
        return f, _lib.LAYOUT_NHWC
    return f.contiguous(), _lib.LAYOUT_NCHW


def _at_map(lib, f, layout, oh, ow):
    B, Cc, H, W = f.shape
    a = torch.empty(B, oh * ow, device=f.device, dtype=torch.float32)
    dt = _DT_CODES[f.dtype]
    n = lib.moma_at_workspace_bytes(B, Cc, H, W, oh, ow, dt, layout)
    ws = torch.empty(n, device=f.device, dtype=torch.uint8) if n else None
    check(lib.moma_at_map(_ptr(f), _ptr(a), B, Cc, H, W, oh, ow, dt, layout, _ptr(ws), n, _stream()), "moma_at_map")
    return a


class _AttentionLoss(torch.autograd.Function):
    """at_map x 2 -> at_pair in the forward; at_bwd per side that needs a gradient in the backward."""

    @staticmethod
    def forward(ctx, f_s, f_t, oh, ow):
        lib = _lib.load()
        f_s, lay_s = _at_side(f_s, "f_s")
        f_t, lay_t = _at_side(f_t, "f_t")
        B = f_s.shape[0]
        if f_t.shape[0] != B or f_s.shape[2] % oh or f_s.shape[3] % ow or f_t.shape[2] % oh or f_t.shape[3] % ow:
            raise ValueError(f"attention_loss: f_s {tuple(f_s.shape)} and f_t {tuple(f_t.shape)} have no common {oh} x {ow} grid")
        dev, n = f_s.device, oh * ow
        need_s, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        with _timed("moma_at_fwd"):
            a_s, a_t = _at_map(lib, f_s, lay_s, oh, ow), _at_map(lib, f_t, lay_t, oh, ow)
            norms = torch.empty(B, 2, device=dev, dtype=torch.float32)
            partials = torch.empty(B, device=dev, dtype=torch.float32)
            loss = torch.empty((), device=dev, dtype=torch.float32)
            g_s = torch.empty(B, n, device=dev, dtype=torch.float32) if need_s else None
            g_t = torch.empty(B, n, device=dev, dtype=torch.float32) if need_t else None
            check(lib.moma_at_pair(_ptr(a_s), _ptr(a_t), B, n, _ptr(norms), _ptr(partials), _ptr(loss), _ptr(g_s), _ptr(g_t),
                                   _ptr(None), _ptr(None), _stream()), "moma_at_pair")
        ctx.save_for_backward(*[t for t, need in ((f_s, need_s), (g_s, need_s), (f_t, need_t), (g_t, need_t)) if need])
        ctx.sides = (need_s, need_t)
        ctx.grid, ctx.layouts = (oh, ow), (lay_s, lay_t)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        saved = list(ctx.saved_tensors)
        oh, ow = ctx.grid
        g = g.to(torch.float32).contiguous()          # the upstream gradient stays on the device (a GradScaler factor rides in it)
        out = [None, None]
        with _timed("moma_at_bwd"):
            for side, need in enumerate(ctx.sides):
                if not need:
                    continue
                f, g_a = saved.pop(0), saved.pop(0)
                B, Cc, H, W = f.shape
                dF = torch.empty_like(f)               # (same dtype, same strides: NCHW or channels_last)
                check(lib.moma_at_bwd(_ptr(f), _ptr(g_a), _ptr(g), _ptr(dF), B, Cc, H, W, oh, ow, _DT_CODES[f.dtype],
                                      ctx.layouts[side], _stream()), "moma_at_bwd")
                out[side] = dF
        return out[0], out[1], None, None


def attention_loss(f_s, f_t) -> torch.Tensor:
    """Attention Transfer loss (p = 2) of one feature pair, f_s [B,Cs,Hs,Ws] and f_t [B,Ct,Ht,Wt] (float32 or bfloat16, contiguous
    or channels_last, independently per side) -> scalar float32:  mean((ah_s - ah_t)^2) with a = mean_c f^2, ah = a / max(|a|, 1e-12).
    Heights that differ: the larger map is average-pooled to (h, h), h = min(Hs, Ht) -- inside the kernels when h divides its H and
    W, with stock adaptive_avg_pool2d in front of them otherwise.  Gradients flow to whichever side requires one."""
    for t, nm in ((f_s, "f_s"), (f_t, "f_t")):
        _dev(t, nm, dtype=None, contiguous=False)
        if t.dim() != 4:
            raise ValueError(f"attention_loss: {nm} must be [B,C,H,W], got {tuple(t.shape)}")
    Hs, Ht = f_s.shape[2], f_t.shape[2]
    if Hs == Ht:
        oh, ow = Hs, f_s.shape[3]
        if f_t.shape[3] != ow:
            raise ValueError(f"attention_loss: equal heights but widths {ow} and {f_t.shape[3]}: the maps have no common grid")
    else:
        oh = ow = min(Hs, Ht)
        if Hs > Ht and (Hs % oh or f_s.shape[3] % ow):
            f_s = torch.nn.functional.adaptive_avg_pool2d(f_s, (oh, ow))
        elif Ht > Hs and (Ht % oh or f_t.shape[3] % ow):
            f_t = torch.nn.functional.adaptive_avg_pool2d(f_t, (oh, ow))
        small = f_t if Hs > Ht else f_s
        if small.shape[3] != ow:
            raise ValueError(f"attention_loss: the smaller map {tuple(small.shape)} is not square: no common {oh} x {ow} grid")
    return _AttentionLoss.apply(f_s, f_t, int(oh), int(ow))


# ------------------------------------------------------------------------------------------------
# Neuron Selectivity Transfer: per-image normalised Gram of a feature pair   (distiller_zoo/NST.py, helper/loops_moma.py:150-154)
# ------------------------------------------------------------------------------------------------
class _NSTLoss(torch.autograd.Function):
    """nst_gram (G, norms, row sums, loss) in the forward; nst_bwd (dF_s from the raw maps and G) in the backward."""

    @staticmethod
    def forward(ctx, f_s, f_t):
        lib = _lib.load()
        f_s, lay_s = _at_side(f_s, "f_s", "nst_loss")
        f_t, lay_t = _at_side(f_t, "f_t", "nst_loss")
        B, Cs, H, W = f_s.shape
        Ct = f_t.shape[1]
        if f_t.shape[0] != B or tuple(f_t.shape[2:]) != (H, W):
            raise ValueError(f"nst_loss: f_s {tuple(f_s.shape)} and f_t {tuple(f_t.shape)} are not on a common grid")
        dev, P = f_s.device, H * W
        codes = (_DT_CODES[f_s.dtype], lay_s, _DT_CODES[f_t.dtype], lay_t)
        with _timed("moma_nst_fwd"):
            n = lib.moma_nst_workspace_bytes(B, Cs, Ct)
            if n == 0:
                raise ValueError(f"nst_loss: the kernels take at most {_lib.NST_MAX_C} channels per side, got {Cs} and {Ct}")
            G = torch.empty(n // 4, device=dev, dtype=torch.float32)
            norms = torch.empty(B, Cs + Ct, device=dev, dtype=torch.float32)
            rows = torch.empty(B, Cs, 2, device=dev, dtype=torch.float32)
            partials = torch.empty(B, -(-Cs // _lib.NST_ROW_BLOCK), 2, device=dev, dtype=torch.float32)
            terms = torch.empty(2, device=dev, dtype=torch.float32)
            loss = torch.empty((), device=dev, dtype=torch.float32)
            check(lib.moma_nst_gram(_ptr(f_s), _ptr(f_t), B, Cs, Ct, P, *codes, _ptr(G), n, _ptr(norms), _ptr(rows), _ptr(partials),
                                    _ptr(terms), _ptr(loss), _stream()), "moma_nst_gram")
        # (nst_loss, the only caller, refuses an f_t that wants a gradient: backward runs only where f_s does, with these saved)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(f_s, f_t, G, norms, rows)
        ctx.codes = codes
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        f_s, f_t, G, norms, rows = ctx.saved_tensors
        B, Cs, H, W = f_s.shape
        g = g.to(torch.float32).contiguous()          # the upstream gradient stays on the device (a GradScaler factor rides in it)
        with _timed("moma_nst_bwd"):
            dF = torch.empty_like(f_s)                # (same dtype, same strides: NCHW or channels_last)
            check(lib.moma_nst_bwd(_ptr(f_s), _ptr(f_t), _ptr(G), G.numel() * 4, _ptr(norms), _ptr(rows), _ptr(g), _ptr(dF), B, Cs,
                                   f_t.shape[1], H * W, *ctx.codes, _stream()), "moma_nst_bwd")
        return dF, None


def nst_loss(f_s, f_t) -> torch.Tensor:
    """Neuron Selectivity Transfer loss of one feature pair, f_s [B,Cs,Hs,Ws] and f_t [B,Ct,Ht,Wt] (float32 or bfloat16, contiguous
    or channels_last, independently per side; at most 256 channels each) -> scalar float32:
    mean_(b,i,j) Gss^2 - 2 mean_(b,i,j) Gst^2 with Gss / Gst the Gram of the L2-normalised channel rows of f_s with themselves / with
    those of f_t.  Heights that differ: the larger map goes through stock adaptive_avg_pool2d to (h, h), h = min(Hs, Ht), in front
    of the kernels (its autograd carries that part of the gradient).  The gradient flows to f_s only."""
    for t, nm in ((f_s, "f_s"), (f_t, "f_t")):
        _dev(t, nm, dtype=None, contiguous=False)
        if t.dim() != 4:
            raise ValueError(f"nst_loss: {nm} must be [B,C,H,W], got {tuple(t.shape)}")
    if f_t.requires_grad and torch.is_grad_enabled():
        raise ValueError("nst_loss: the kernels give no gradient to f_t (detach it, or use distiller_zoo.NSTLoss.composite)")
    Hs, Ht = f_s.shape[2], f_t.shape[2]
    if Hs > Ht:
        f_s = torch.nn.functional.adaptive_avg_pool2d(f_s, (Ht, Ht))
    elif Hs < Ht:
        f_t = torch.nn.functional.adaptive_avg_pool2d(f_t, (Hs, Hs))
    if f_s.shape[3] != f_t.shape[3]:
        raise ValueError(f"nst_loss: widths {f_s.shape[3]} and {f_t.shape[3]} at height {min(Hs, Ht)}: the maps have no common grid")
    return _NSTLoss.apply(f_s, f_t)


# ------------------------------------------------------------------------------------------------
# Variational Information Distillation: per-channel Gaussian NLL of a regressor's output   (distiller_zoo/VID.py, helper/loops_moma.py:145-149)
# ------------------------------------------------------------------------------------------------
def _map_side(f, name, op, composite):
    """-> layout code of a dense [B,C,H,W] float32 / bfloat16 device tensor (contiguous or channels_last, taken as it lies); the
    messages name `op` and distiller_zoo's `composite`.  For the ops on csrc/mapwalk.hpp: vid_nll, hint_bn_relu_mse."""
    _dev(f, name, dtype=None, contiguous=False)
    if f.dim() != 4 or f.dtype not in _DT_CODES:
        raise TypeError(f"{op}: {name} must be a 4-D float32 / bfloat16 tensor, got {tuple(f.shape)} {f.dtype}")
    if f.is_contiguous():
        return _lib.LAYOUT_NCHW
    if f.is_contiguous(memory_format=torch.channels_last):
        return _lib.LAYOUT_NHWC
    raise ValueError(f"{op}: {name} {tuple(f.shape)} with strides {tuple(f.stride())} is neither contiguous nor channels_last "
                     f"(use distiller_zoo.{composite}.composite)")


class _VIDNLL(torch.autograd.Function):
    """vid_nll (S, var, d loss / d log_scale, loss) in the forward; vid_bwd (d_mean from the two maps and var) in the backward."""

    @staticmethod
    def forward(ctx, mean, target, log_scale, eps):
        lib = _lib.load()
        lay_m, lay_t = (_map_side(f, nm, "vid_nll", "VIDLoss") for f, nm in ((mean, "mean"), (target, "target")))
        _dev(log_scale, "log_scale", torch.float32)
        B, Cc, H, W = mean.shape
        if tuple(target.shape) != (B, Cc, H, W) or tuple(log_scale.shape) != (Cc,):
            raise ValueError(f"vid_nll: mean {tuple(mean.shape)}, target {tuple(target.shape)} and log_scale {tuple(log_scale.shape)} "
                             "do not agree")
        dev, P = mean.device, H * W
        codes = (_DT_CODES[mean.dtype], lay_m, _DT_CODES[target.dtype], lay_t)
        with _timed("moma_vid_fwd"):
            n = lib.moma_vid_workspace_bytes(B, Cc, P, *codes)
            if n == 0:
                raise ValueError(f"vid_nll: no workspace for mean {tuple(mean.shape)}")
            ws = torch.empty(n // 8, device=dev, dtype=torch.float64)
            sq, var, g_ls = (torch.empty(Cc, device=dev, dtype=torch.float32) for _ in range(3))
            loss = torch.empty((), device=dev, dtype=torch.float32)
            check(lib.moma_vid_nll(_ptr(mean), _ptr(target), _ptr(log_scale), float(eps), B, Cc, P, *codes, _ptr(ws), n, _ptr(sq),
                                   _ptr(var), _ptr(g_ls), _ptr(loss), _stream()), "moma_vid_nll")
        ctx.save_for_backward(mean, target, var, g_ls)
        ctx.codes = codes
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        mean, target, var, g_ls = ctx.saved_tensors
        B, Cc, H, W = mean.shape
        g = g.to(torch.float32).contiguous()          # the upstream gradient stays on the device (a GradScaler factor rides in it)
        d_mean = None
        if ctx.needs_input_grad[0]:
            with _timed("moma_vid_bwd"):
                d_mean = torch.empty_like(mean)       # (same dtype, same strides: NCHW or channels_last)
                check(lib.moma_vid_bwd(_ptr(mean), _ptr(target), _ptr(var), _ptr(g), _ptr(d_mean), B, Cc, H * W, *ctx.codes,
                                       _stream()), "moma_vid_bwd")
        return d_mean, None, (g * g_ls if ctx.needs_input_grad[2] else None), None


def vid_nll(mean, target, log_scale, eps=1e-5) -> torch.Tensor:
    """Gaussian negative log-likelihood of Variational Information Distillation: mean (the regressor's output) and target, both
    [B,C,H,W] (float32 or bfloat16, contiguous or channels_last, independently per side), log_scale [C] float32 -> scalar float32:
    0.5 mean_(b,c,p) ((mean - target)^2 / var_c + log var_c), var_c = softplus(log_scale_c) + eps.  Gradients flow to mean (in its
    dtype and strides) and to log_scale; the target gets none."""
    for t, nm in ((mean, "mean"), (target, "target")):
        _dev(t, nm, dtype=None, contiguous=False)
        if t.dim() != 4:
            raise ValueError(f"vid_nll: {nm} must be [B,C,H,W], got {tuple(t.shape)}")
    if target.requires_grad and torch.is_grad_enabled():
        raise ValueError("vid_nll: the kernels give no gradient to the target (detach it, or use distiller_zoo.VIDLoss.composite)")
    return _VIDNLL.apply(mean, target, log_scale, float(eps))


# ------------------------------------------------------------------------------------------------
# FitNets hint: training-mode BatchNorm -> ReLU -> MSE behind the regressor's convolution   (models/util.py ConvReg, distiller_zoo/FitNet.py)
# ------------------------------------------------------------------------------------------------
def hint_native(B: int, C: int, P: int, dtype=None, channels_last=None) -> bool:
    """Shapes [B, C, H W = P] whose BatchNorm -> ReLU -> MSE tail runs on csrc/hint.hip; the others take ConvReg.composite.
    By profiles/hint_layer_microbench.txt (the five hint_layer maps of EfficientNet-B0 at B = 256, both layouts, fp32 and bf16;
    verdict: fused <= stock ops + the stock form's own spread; two series) 19 of 20 rows hold at 1.2 - 10 x; 112 x 14 x 14 in fp32
    NCHW loses in both series, 161.2 against 151.8 us and 209.4 against 178.9 us: the two C-ABI calls take 54 us there, the rest is
    host work of the op (allocations, argument checks, four launches), which the stock form's three ops undercut on a 135 MB map.
    That class -- fp32 storage, NCHW, planes of 64 to 255 pixels -- goes to the composite; the same map in bf16 (1.5 - 1.6 x) or
    channels_last (3.0 x) holds and stays.  `dtype` and `channels_last` describe the convolution's output; asked without them the
    table answers for the shape alone (True).
    A shape BatchNorm itself refuses (one value per channel) is not asked here: the op raises for it."""
    if dtype == torch.float32 and channels_last is False and 64 <= P < 256:
        return False
    return True


class _HintBNReLUMSE(torch.autograd.Function):
    """hint_fwd (statistics, running statistics, loss, A and B) in the forward; hint_bwd (dx from the two maps and the saved [C]
    vectors, d weight and d bias from A and B) in the backward.  conv_bias only moves running_mean: its gradient is exact zeros."""

    @staticmethod
    def forward(ctx, x, target, weight, bias, running_mean, running_var, momentum, eps, conv_bias):
        lib = _lib.load()
        lay_x, lay_t = (_map_side(f, nm, "hint_bn_relu_mse", "ConvReg") for f, nm in ((x, "x"), (target, "target")))
        B, Cc, H, W = x.shape
        vecs = [("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var), ("conv_bias", conv_bias)]
        for nm, v in vecs:
            if v is None and nm in ("running_mean", "running_var", "conv_bias"):
                continue
            _dev(v, nm, torch.float32)
            if tuple(v.shape) != (Cc,):
                raise ValueError(f"hint_bn_relu_mse: {nm} {tuple(v.shape)} for {Cc} channels")
        if tuple(target.shape) != (B, Cc, H, W):
            raise ValueError(f"hint_bn_relu_mse: x {tuple(x.shape)} and target {tuple(target.shape)} do not agree")
        P = H * W
        if B * P < 2:
            raise ValueError(f"hint_bn_relu_mse: expected more than 1 value per channel when training, got x {tuple(x.shape)}")
        dev = x.device
        codes = (_DT_CODES[x.dtype], lay_x, _DT_CODES[target.dtype], lay_t)
        with _timed("moma_hint_fwd"):
            n = lib.moma_hint_workspace_bytes(B, Cc, P, *codes)
            if n == 0:
                raise ValueError(f"hint_bn_relu_mse: no workspace for x {tuple(x.shape)}")
            buf = torch.empty(n // 8 + 4 * Cc, device=dev, dtype=torch.float64)      # (one allocation: workspace, mean, invstd, A and B)
            ws, mean, invstd, sums = buf[:n // 8], buf[n // 8:n // 8 + Cc], buf[n // 8 + Cc:n // 8 + 2 * Cc], buf[n // 8 + 2 * Cc:]
            loss = torch.empty((), device=dev, dtype=torch.float32)
            check(lib.moma_hint_fwd(_ptr(x), _ptr(target), _ptr(weight), _ptr(bias), _ptr(conv_bias), _ptr(running_mean),
                                    _ptr(running_var), float(momentum), float(eps), B, Cc, P, *codes, _ptr(ws), n, _ptr(mean),
                                    _ptr(invstd), _ptr(sums), _ptr(loss), _stream()), "moma_hint_fwd")
        ctx.save_for_backward(x, target, weight, bias, mean, invstd, sums)
        ctx.codes = codes
        ctx.has_conv_bias = conv_bias is not None
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        x, target, weight, bias, mean, invstd, sums = ctx.saved_tensors
        B, Cc, H, W = x.shape
        g = g.to(torch.float32).contiguous()          # the upstream gradient stays on the device (a GradScaler factor rides in it)
        need = ctx.needs_input_grad
        dx = d_w = d_b = None
        if need[0] or need[2] or need[3]:
            with _timed("moma_hint_bwd"):
                if need[0]:
                    dx = torch.empty_like(x)          # (same dtype, same strides: NCHW or channels_last)
                if need[2]:
                    d_w = torch.empty_like(weight)
                if need[3]:
                    d_b = torch.empty_like(bias)
                check(lib.moma_hint_bwd(_ptr(x), _ptr(target), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(invstd), _ptr(sums), _ptr(g),
                                        _ptr(dx), _ptr(d_w), _ptr(d_b), B, Cc, H * W, *ctx.codes, _stream()), "moma_hint_bwd")
        d_cb = torch.zeros_like(weight) if (ctx.has_conv_bias and need[8]) else None
        return dx, None, d_w, d_b, None, None, None, None, d_cb


def hint_bn_relu_mse(x, target, weight, bias, running_mean, running_var, momentum, eps, conv_bias=None) -> torch.Tensor:
    """FitNets hint behind the regressor's convolution: mean((relu(batch_norm(x)) - target)^2) with the BatchNorm in training mode
    (batch statistics; running_mean / running_var, each optional, updated in place with `momentum`, the variance unbiased).  x (the
    convolution's output WITHOUT its bias) and target are [B,C,H,W], float32 or bfloat16, contiguous or channels_last, independently
    per side; weight, bias, the running statistics and conv_bias are [C] float32 -> scalar float32.  conv_bias is the convolution's
    bias: in front of a training-mode BatchNorm it moves running_mean and nothing else, so it is added there only and its gradient
    is exact zeros.  Gradients flow to x (in its dtype and strides), weight, bias and conv_bias; the target gets none."""
    for t, nm in ((x, "x"), (target, "target")):
        _dev(t, nm, dtype=None, contiguous=False)
        if t.dim() != 4:
            raise ValueError(f"hint_bn_relu_mse: {nm} must be [B,C,H,W], got {tuple(t.shape)}")
    if target.requires_grad and torch.is_grad_enabled():
        raise ValueError("hint_bn_relu_mse: the kernels give no gradient to the target (detach it, or use "
                         "distiller_zoo.ConvReg.composite)")
    if momentum is None:
        raise ValueError("hint_bn_relu_mse: momentum=None (cumulative average) is served by distiller_zoo.ConvReg.composite")
    return _HintBNReLUMSE.apply(x, target, weight, bias, running_mean, running_var, float(momentum), float(eps), conv_bias)


# ------------------------------------------------------------------------------------------------
# SRRL: training-mode BatchNorm -> ReLU -> MSE, the teacher's classifier -> MSE behind the connector's convolution   (models/util.py SRRL)
# ------------------------------------------------------------------------------------------------
def srrl_native(B: int, C: int, K: int, dtype=None) -> bool:
    """Shapes (batch B, teacher channels C = t_n, classes K) whose tail behind the connector's convolution runs on csrc/srrl.hip; the
    others take distiller_zoo.SRRL.composite.  The kernels serve 2 <= B <= 1024, 1 <= C <= 4096, 1 <= K <= 1024 (the C ABI's caps);
    anything past them is refused here, so the module never asks the library for a shape it returns an error for.
    By profiles/srrl_microbench.txt (B = 256; (C, K) in (1280, 4), (1280, 8), (1280, 1000), (256, 100), (2048, 1000), (768, 1000);
    fp32 and bf16 storage; verdict: fused <= stock ops + the stock form's own spread; two series) all 12 rows hold in both series at
    1.3 - 1.7 x (151 - 214 us against 234 - 308 us per forward + backward), so no measured row is turned away.  The rows that lost
    did so on the first version of the GEMM kernel (32 x 32 tiles, no prefetch): (2048, 1000) at 298.8 against 257.8 us and 301.9
    against 268.8 us in fp32, 292.5 against 254.9 us and 280.0 against 212.1 us in bf16; with the 64 x 64 tile they hold at 178.2 /
    209.2 against 304.9 / 306.1 us (fp32) and 185.2 / 214.4 against 244.2 / 304.3 us (bf16).  `dtype` describes the convolution's
    output; asked without it the table answers for the shape alone."""
    if not (2 <= B <= _lib.SRRL_MAX_B and 1 <= C <= _lib.SRRL_MAX_C and 1 <= K <= _lib.SRRL_MAX_K):
        return False
    return True


def _rows_side(op, f, name):
    """-> dense [B, C] float32 / bfloat16 device tensor (the per-side guard of srrl_bn_relu_dual_mse, cc_embed_neighbour and kd_head)"""
    _dev(f, name, dtype=None, contiguous=False)
    if f.dim() != 2 or f.dtype not in _DT_CODES:
        raise TypeError(f"{op}: {name} must be a 2-D float32 / bfloat16 tensor, got {tuple(f.shape)} {f.dtype}")
    if not f.is_contiguous():
        raise ValueError(f"{op}: {name} {tuple(f.shape)} with strides {tuple(f.stride())} is not contiguous")
    return f


class _SRRLTail(torch.autograd.Function):
    """srrl_fwd (statistics, running statistics, both products, the loss, A, B and dx for an upstream gradient of 1) in the forward;
    srrl_bwd (one launch: everything scaled by the upstream gradient) in the backward."""

    @staticmethod
    def forward(ctx, x, target, cls_weight, cls_bias, logits, weight, bias, running_mean, running_var, momentum, eps):
        lib = _lib.load()
        _rows_side("srrl_bn_relu_dual_mse", x, "x")
        _rows_side("srrl_bn_relu_dual_mse", target, "target")
        B, Cc = x.shape
        K = cls_weight.shape[0] if isinstance(cls_weight, torch.Tensor) and cls_weight.dim() == 2 else -1
        for nm, v, shape in (("cls_weight", cls_weight, (K, Cc)), ("cls_bias", cls_bias, (K,)), ("logits", logits, (B, K)),
                             ("weight", weight, (Cc,)), ("bias", bias, (Cc,)), ("running_mean", running_mean, (Cc,)),
                             ("running_var", running_var, (Cc,))):
            if v is None and nm in ("cls_bias", "running_mean", "running_var"):
                continue
            _dev(v, nm, torch.float32)
            if tuple(v.shape) != shape:
                raise ValueError(f"srrl_bn_relu_dual_mse: {nm} {tuple(v.shape)}, expected {shape}")
        if tuple(target.shape) != (B, Cc):
            raise ValueError(f"srrl_bn_relu_dual_mse: x {tuple(x.shape)} and target {tuple(target.shape)} do not agree")
        if B < 2:
            raise ValueError(f"srrl_bn_relu_dual_mse: expected more than 1 value per channel when training, got x {tuple(x.shape)}")
        dev = x.device
        codes = (_DT_CODES[x.dtype], _DT_CODES[target.dtype])
        with _timed("moma_srrl_fwd"):
            n = lib.moma_srrl_workspace_bytes(B, Cc, K)
            if n == 0:
                raise ValueError(f"srrl_bn_relu_dual_mse: x {tuple(x.shape)} with {K} classes is past the kernels' caps "
                                 f"(B <= {_lib.SRRL_MAX_B}, C <= {_lib.SRRL_MAX_C}, K <= {_lib.SRRL_MAX_K})")
            nd, nw = (B * Cc + 1) // 2, (n + 7) // 8
            buf = torch.empty(2 * Cc + nd + nw, device=dev, dtype=torch.float64)    # (one allocation: A and B, dx for g = 1, workspace)
            sums, dxu, ws = buf[:2 * Cc], buf[2 * Cc:2 * Cc + nd].view(torch.float32)[:B * Cc], buf[2 * Cc + nd:]
            loss = torch.empty((), device=dev, dtype=torch.float32)
            check(lib.moma_srrl_fwd(_ptr(x), _ptr(target), _ptr(cls_weight), _ptr(cls_bias), _ptr(logits), _ptr(weight), _ptr(bias),
                                    _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), B, Cc, K, *codes, _ptr(ws),
                                    nw * 8, _ptr(sums), _ptr(dxu), _ptr(loss), None, None, _stream()), "moma_srrl_fwd")
        ctx.save_for_backward(sums, dxu, weight, bias)
        ctx.x_meta = (B, Cc, x.dtype, codes[0])
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        sums, dxu, weight, bias = ctx.saved_tensors
        B, Cc, dtype, code = ctx.x_meta
        g = g.to(torch.float32).contiguous()          # the upstream gradient stays on the device (a GradScaler factor rides in it)
        need = ctx.needs_input_grad
        dx = d_w = d_b = None
        if need[0] or need[5] or need[6]:
            with _timed("moma_srrl_bwd"):
                if need[0]:
                    dx = torch.empty((B, Cc), device=dxu.device, dtype=dtype)
                if need[5]:
                    d_w = torch.empty_like(weight)
                if need[6]:
                    d_b = torch.empty_like(bias)
                check(lib.moma_srrl_bwd(_ptr(dxu), _ptr(sums), _ptr(g), _ptr(dx), _ptr(d_w), _ptr(d_b), B, Cc, code, _stream()),
                      "moma_srrl_bwd")
        return dx, None, None, None, None, d_w, d_b, None, None, None, None


def srrl_bn_relu_dual_mse(x, target, cls_weight, cls_bias, logits, weight, bias, running_mean, running_var, momentum, eps) -> torch.Tensor:
    """SRRL behind the connector's convolution: with y = relu(batch_norm(x)) (training mode: batch statistics; running_mean /
    running_var, each optional, updated in place with `momentum`, the variance unbiased),
    mean((y - target)^2) + mean((y @ cls_weight.T + cls_bias - logits)^2).  x (the convolution's output) and target are [B, C],
    float32 or bfloat16 independently per side and contiguous; cls_weight [K, C], cls_bias [K] (optional) -- the TEACHER'S classifier
    -- , logits [B, K], weight, bias and the running statistics [C] are float32 -> scalar float32.  Gradients flow to x (in its
    dtype), weight and bias; the target, the logits and the classifier get none."""
    for t, nm in ((x, "x"), (target, "target"), (logits, "logits")):
        _dev(t, nm, dtype=None, contiguous=False)
    if x.dim() != 2 or target.dim() != 2:
        raise ValueError(f"srrl_bn_relu_dual_mse: x and target must be [B, C], got {tuple(x.shape)} and {tuple(target.shape)}")
    if torch.is_grad_enabled() and (target.requires_grad or logits.requires_grad):
        raise ValueError("srrl_bn_relu_dual_mse: the kernels give no gradient to the target or the logits (detach them, or use "
                         "distiller_zoo.SRRL.composite)")
    if momentum is None:
        raise ValueError("srrl_bn_relu_dual_mse: momentum=None (cumulative average) is served by distiller_zoo.SRRL.composite")
    return _SRRLTail.apply(x, target, cls_weight, cls_bias, logits, weight, bias, running_mean, running_var, float(momentum), float(eps))


# ------------------------------------------------------------------------------------------------
# Correlation Congruence: both LinearEmbed heads, |difference|, the neighbouring-row product and every gradient   (distiller_zoo/CC.py)
# ------------------------------------------------------------------------------------------------
def cc_native(B: int, Cs: int, Ct: int, D: int, dtype=None) -> bool:
    """Shapes (batch B, student width Cs, teacher width Ct, embedding width D = --feat_dim) whose two heads and criterion run on
    csrc/cc.hip; the others take distiller_zoo.Correlation.composite.  The kernels serve 2 <= B <= 1024, 1 <= Cs, Ct <= 4096,
    1 <= D <= 4096 (the C ABI's caps); anything past them is refused here, so the module never asks the library for a shape it returns
    an error for.  By profiles/cc_microbench.txt (B in (64, 256); widths 256, 768, 1280, 2048 on both sides; D in (128, 512); fp32 and
    bf16 storage -- the two series; verdict: fused <= stock ops + the stock form's own spread) all 32 rows hold at 1.4 - 3.7 x
    (90 - 258 us against 268 - 398 us per forward + backward), so no measured shape class is turned away.  The rows that came
    nearest did so on the first version of the finalize kernel (16 columns per workgroup): (256, 2048, 2048, 128) at 294.6 against
    358.9 us in fp32 and 281.4 against 289.7 us in bf16; with 4 columns per workgroup they hold at 161.8 against 268.6 us and 204.6
    against 350.1 us.  `dtype` describes x_s; asked without it the table answers for the shape alone."""
    if not (2 <= B <= _lib.CC_MAX_B and 1 <= Cs <= _lib.CC_MAX_C and 1 <= Ct <= _lib.CC_MAX_C and 1 <= D <= _lib.CC_MAX_D):
        return False
    return True


class _CCEmbedNeighbour(torch.autograd.Function):
    """cc_fwd (the difference of both heads, the loss, G = d loss / d difference) in the forward; cc_bwd (one grouped launch: the three
    products on G and the bias sums, scaled by the upstream gradient) in the backward."""

    @staticmethod
    def forward(ctx, x_s, x_t, w_s, b_s, w_t, b_t):
        lib = _lib.load()
        _rows_side("cc_embed_neighbour", x_s, "x_s")
        _rows_side("cc_embed_neighbour", x_t, "x_t")
        B, Cs = x_s.shape
        Ct = x_t.shape[1]
        D = w_s.shape[0] if isinstance(w_s, torch.Tensor) and w_s.dim() == 2 else -1
        for nm, v, shape in (("w_s", w_s, (D, Cs)), ("b_s", b_s, (D,)), ("w_t", w_t, (D, Ct)), ("b_t", b_t, (D,))):
            _dev(v, nm, torch.float32)
            if tuple(v.shape) != shape:
                raise ValueError(f"cc_embed_neighbour: {nm} {tuple(v.shape)}, expected {shape}")
        if x_t.shape[0] != B:
            raise ValueError(f"cc_embed_neighbour: x_s {tuple(x_s.shape)} and x_t {tuple(x_t.shape)} do not agree in the batch")
        if B < 2:
            raise ValueError(f"cc_embed_neighbour: no pair of neighbouring rows in x_s {tuple(x_s.shape)} (the reference's mean over an "
                             "empty slice is NaN: distiller_zoo.Correlation.composite)")
        dev = x_s.device
        codes = (_DT_CODES[x_s.dtype], _DT_CODES[x_t.dtype])
        with _timed("moma_cc_fwd"):
            n = lib.moma_cc_workspace_bytes(B, Cs, Ct, D)
            if n == 0:
                raise ValueError(f"cc_embed_neighbour: x_s {tuple(x_s.shape)}, x_t {tuple(x_t.shape)} with {D} outputs is past the kernels' "
                                 f"caps (B <= {_lib.CC_MAX_B}, Cs, Ct <= {_lib.CC_MAX_C}, D <= {_lib.CC_MAX_D})")
            nw = (n + 7) // 8
            ws = torch.empty(nw, device=dev, dtype=torch.float64)
            gu = torch.empty((B, D), device=dev, dtype=torch.float32)
            loss = torch.empty((), device=dev, dtype=torch.float32)
            check(lib.moma_cc_fwd(_ptr(x_s), _ptr(x_t), _ptr(w_s), _ptr(b_s), _ptr(w_t), _ptr(b_t), B, Cs, Ct, D, *codes, _ptr(ws), nw * 8,
                                  _ptr(gu), _ptr(loss), None, _stream()), "moma_cc_fwd")
        ctx.save_for_backward(gu, x_s, x_t, w_s)
        ctx.meta = (B, Cs, Ct, D, codes)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        gu, x_s, x_t, w_s = ctx.saved_tensors
        B, Cs, Ct, D, codes = ctx.meta
        g = g.to(torch.float32).contiguous()          # the upstream gradient stays on the device (a GradScaler factor rides in it)
        need = ctx.needs_input_grad
        dx = dws = dbs = dwt = dbt = None
        if need[0] or need[2] or need[3] or need[4] or need[5]:
            with _timed("moma_cc_bwd"):
                dev = gu.device
                if need[0]:
                    dx = torch.empty((B, Cs), device=dev, dtype=x_s.dtype)
                if need[2]:
                    dws = torch.empty((D, Cs), device=dev, dtype=torch.float32)
                if need[3]:
                    dbs = torch.empty((D,), device=dev, dtype=torch.float32)
                if need[4]:
                    dwt = torch.empty((D, Ct), device=dev, dtype=torch.float32)
                if need[5]:
                    dbt = torch.empty((D,), device=dev, dtype=torch.float32)
                check(lib.moma_cc_bwd(_ptr(gu), _ptr(x_s), _ptr(x_t), _ptr(w_s), _ptr(g), _ptr(dx), _ptr(dws), _ptr(dbs), _ptr(dwt),
                                      _ptr(dbt), B, Cs, Ct, D, *codes, _stream()), "moma_cc_bwd")
        return dx, None, dws, dbs, dwt, dbt


def cc_embed_neighbour(x_s, x_t, w_s, b_s, w_t, b_t) -> torch.Tensor:
    """Correlation Congruence behind both backbones: with d = x_s @ w_s.T + b_s - (x_t @ w_t.T + b_t),
    mean over the B - 1 pairs of neighbouring rows of sum_k |d[i, k]| |d[i + 1, k]|.  x_s [B, Cs] and x_t [B, Ct] are float32 or
    bfloat16 independently per side and contiguous; w_s [D, Cs], b_s [D], w_t [D, Ct], b_t [D] are float32 -> scalar float32.
    Gradients flow to x_s (in its dtype) and to BOTH heads' weights and biases; x_t gets none."""
    for t, nm in ((x_s, "x_s"), (x_t, "x_t")):
        _dev(t, nm, dtype=None, contiguous=False)
    if x_s.dim() != 2 or x_t.dim() != 2:
        raise ValueError(f"cc_embed_neighbour: x_s and x_t must be [B, C], got {tuple(x_s.shape)} and {tuple(x_t.shape)}")
    if torch.is_grad_enabled() and x_t.requires_grad:
        raise ValueError("cc_embed_neighbour: the kernels give no gradient to x_t (detach it, or use distiller_zoo.Correlation.composite)")
    return _CCEmbedNeighbour.apply(x_s, x_t, w_s, b_s, w_t, b_t)


# ------------------------------------------------------------------------------------------------
# The classification head of the teacher trainer: cross-entropy, top-1 and the confusion matrix   (helper/loops_moma.py:13-65, :376-444)
# ------------------------------------------------------------------------------------------------
def ce_native(B: int, K: int, dtype=None) -> bool:
    """Shapes (batch B, classes K) whose cross-entropy, top-1 count and confusion matrix run on csrc/ce.hip; the others take
    helper.ce_head.CrossEntropyHead.composite.  The kernels serve 1 <= B <= 16384 and 1 <= K <= 32768 (the C ABI's caps); anything
    past them is refused here, so the module never asks the library for a shape it returns an error for.  By
    profiles/ce_microbench.txt (B in (64, 256) x K in (4, 9, 100, 1000), fp32 and bf16 logits, the training and the validation
    series; verdict: fused <= stock ops + the stock form's own spread in BOTH series) all 8 bf16 rows hold (training 1.03 - 1.64 x,
    validation 4.6 - 6.0 x), and 7 of the 8 fp32 rows LOSE their training series: 127 - 139 us against 119 - 129 us per forward +
    backward, although the same rows win validation 3.5 - 6.0 x and the three launches take 25 - 30 us.  The loss is host time: the
    stock chain on fp32 logits has no casts (11 launches against 13 for bf16) and a backward made of C++ nodes, while the fused
    backward is a Python node that the autograd thread must take the interpreter lock for.  That class -- fp32 logits, every shape --
    goes to the composite; bf16 logits, what `--amp bf16` hands the head, stay on the kernels.  `dtype` describes the logits; asked
    without it the table answers for the shape alone."""
    if not (1 <= B <= _lib.CE_MAX_B and 1 <= K <= _lib.CE_MAX_K):
        return False
    if dtype == torch.float32:
        return False
    return True


class _CEHead(torch.autograd.Function):
    """ce_fwd (the loss, lse and 1 / n_valid; the meter's sums and the confusion matrix where asked for) in the forward; ce_bwd (one
    launch, no reduction) in the backward."""

    @staticmethod
    def forward(ctx, logits, labels, stats, conf):
        lib = _lib.load()
        B, K = logits.shape
        dev = logits.device
        code = _DT_CODES[logits.dtype]
        ctx.set_materialize_grads(False)
        with _timed("moma_ce_fwd"):
            n = lib.moma_ce_workspace_bytes(B, K)
            if n == 0:
                raise ValueError(f"ce_head: logits {tuple(logits.shape)} are past the kernels' caps (B <= {_lib.CE_MAX_B}, "
                                 f"K <= {_lib.CE_MAX_K})")
            nw = (n + 7) // 8
            # (one allocation: workspace, lse [B], 1 / n_valid; handed over as addresses -- three views of it would cost the host
            #  more than the head's two launches take)
            buf = torch.empty(nw + B + 1, device=dev, dtype=torch.float64)
            loss = torch.empty((), device=dev, dtype=torch.float32)
            base = buf.data_ptr()
            check(lib.moma_ce_fwd(_ptr(logits), _ptr(labels), B, K, code, base, nw * 8, _ptr(loss), base + nw * 8, base + (nw + B) * 8,
                                  None, _ptr(stats), _ptr(conf), _stream()), "moma_ce_fwd")
        ctx.save_for_backward(logits, labels, buf)
        ctx.meta = (code, nw)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        lib = _lib.load()
        logits, labels, buf = ctx.saved_tensors
        B, K = logits.shape
        code, nw = ctx.meta
        if g.dtype != torch.float32:                  # the upstream gradient stays on the device (a GradScaler factor rides in it)
            g = g.to(torch.float32)
        with _timed("moma_ce_bwd"):
            dz = torch.empty((B, K), device=logits.device, dtype=logits.dtype)
            base = buf.data_ptr()
            check(lib.moma_ce_bwd(_ptr(logits), _ptr(labels), base + nw * 8, base + (nw + B) * 8, _ptr(g), _ptr(dz), B, K, code,
                                  _stream()), "moma_ce_bwd")
        return dz, None, None, None


def ce_head(logits, labels, stats=None, conf=None) -> torch.Tensor:
    """nn.CrossEntropyLoss()(logits, labels) -- the mean over the rows whose label is not -100 -- with the head's metrics from the same
    two launches.  logits [B, K] float32 or bfloat16, contiguous; labels [B] int64 -> scalar float32.  stats (optional, [4] float64,
    device): the call ADDS (sum of the valid rows' losses, top-1 hits, valid rows, rows with a bad label).  conf (optional, [K, K] int64,
    device, row = label, column = prediction): the call adds 1 at [label, argmax] for every valid row; the argmax is the lowest index
    of the row's maximum.  A label outside [0, K) other than -100 is never used as an index: the loss is NaN, the row's gradient zero
    and stats[3] counts it (stock torch asserts on the device).  The gradient flows to the logits, in their dtype."""
    # (the head's two launches take less than a dozen tensor queries do: one pass over the usual case, the reasons only when it fails)
    ok = (torch.is_tensor(logits) and logits.is_cuda and logits.dim() == 2 and logits.dtype in _DT_CODES and logits.is_contiguous()
          and logits.numel() > 0 and torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int64
          and labels.shape == logits.shape[:1] and labels.is_contiguous())
    if not ok:
        _dev(logits, "logits", dtype=None, contiguous=False)
        if logits.dim() != 2 or logits.dtype not in _DT_CODES:
            raise TypeError(f"ce_head: logits must be a 2-D float32 / bfloat16 tensor, got {tuple(logits.shape)} {logits.dtype}")
        if not logits.is_contiguous():
            raise ValueError(f"ce_head: logits {tuple(logits.shape)} with strides {tuple(logits.stride())} are not contiguous")
        _dev(labels, "labels", torch.int64)
        if tuple(labels.shape) != (logits.shape[0],):
            raise ValueError(f"ce_head: labels {tuple(labels.shape)} for logits {tuple(logits.shape)}")
        raise ValueError(f"ce_head: empty logits {tuple(logits.shape)}")
    K = logits.shape[1]
    if stats is not None:
        _dev(stats, "stats", torch.float64)
        if tuple(stats.shape) != (4,):
            raise ValueError(f"ce_head: stats {tuple(stats.shape)}, expected (4,)")
    if conf is not None:
        _dev(conf, "conf", torch.int64)
        if tuple(conf.shape) != (K, K):
            raise ValueError(f"ce_head: conf {tuple(conf.shape)}, expected {(K, K)}")
    return _CEHead.apply(logits, labels, stats, conf)


# ------------------------------------------------------------------------------------------------
# The student's head: cross-entropy, the KD divergence at temperature T and top-1   (helper/loops_moma.py:278-279, distiller_zoo/KD.py)
# ------------------------------------------------------------------------------------------------
def kd_head_native(B: int, K: int, dtype_s=None, dtype_t=None) -> bool:
    """Shapes (batch B, classes K) whose cross-entropy, KD divergence and top-1 run on csrc/kdhead.hip; the others take
    helper.kd_head.StudentHead.composite.  The kernels serve 1 <= B <= 16384 and 1 <= K <= 32768 (the C ABI's caps, the CE head's);
    anything past them is refused here, so the module never asks the library for a shape it returns an error for.  By
    profiles/kdhead_microbench.txt (B in (64, 256) x K in (4, 9, 100, 1000), fp32 and bf16 student logits against fp32 teacher logits,
    forward + backward of the head against the stock chain with its .float() cast and accuracy; verdict: fused <= stock ops + the
    stock form's own spread) all 16 rows hold, fp32 student logits included: 100 - 215 us against 234 - 351 us, 1.6 - 2.6 x.  The
    stock chain here is 33 - 36 launches against the fused route's 9, so the Python backward node that cost the CE head its fp32 rows
    is paid for several times over: no dtype pair is turned away.  `dtype_s` / `dtype_t`
    describe the student's and the teacher's logits; asked without them the table answers for the shape alone."""
    if not (1 <= B <= _lib.KDHEAD_MAX_B and 1 <= K <= _lib.KDHEAD_MAX_K):
        return False
    for dt in (dtype_s, dtype_t):
        if dt is not None and dt not in _DT_CODES:
            return False
    return True


class _KDHead(torch.autograd.Function):
    """kdhead_fwd (loss_cls, loss_div, acc; the three lse and 1 / n_valid) in the forward; kdhead_bwd (one launch, no reduction) in the
    backward, with the two upstream gradients as device scalars (None: a NULL pointer, that part is not evaluated)."""

    @staticmethod
    def forward(ctx, logit_s, logit_t, labels, T):
        lib = _lib.load()
        B, K = logit_s.shape
        dev = logit_s.device
        codes = (_DT_CODES[logit_s.dtype], _DT_CODES[logit_t.dtype])
        ctx.set_materialize_grads(False)
        with _timed("moma_kdhead_fwd"):
            n = lib.moma_kdhead_workspace_bytes(B, K)
            if n == 0:
                raise ValueError(f"kd_head: logits {tuple(logit_s.shape)} are past the kernels' caps (B <= {_lib.KDHEAD_MAX_B}, "
                                 f"K <= {_lib.KDHEAD_MAX_K})")
            nw = (n + 7) // 8
            # (one allocation: workspace, then lse, lseS, lseT [B] each and 1 / n_valid; handed over as addresses, as _CEHead does)
            buf = torch.empty(nw + 3 * B + 1, device=dev, dtype=torch.float64)
            out = torch.empty(3, device=dev, dtype=torch.float32)
            base = buf.data_ptr()
            check(lib.moma_kdhead_fwd(_ptr(logit_s), _ptr(logit_t), _ptr(labels), B, K, *codes, T, base, nw * 8, _ptr(out), base + nw * 8,
                                      _stream()), "moma_kdhead_fwd")
        ctx.save_for_backward(logit_s, logit_t, labels, buf)
        ctx.meta = (codes, nw, T)
        loss_cls, loss_div, acc = out.unbind(0)
        ctx.mark_non_differentiable(acc)
        return loss_cls, loss_div, acc

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls, g_div, _g_acc):
        if (g_cls is None and g_div is None) or not ctx.needs_input_grad[0]:
            return None, None, None, None
        lib = _lib.load()
        logit_s, logit_t, labels, buf = ctx.saved_tensors
        B, K = logit_s.shape
        codes, nw, T = ctx.meta
        # (the upstream gradients stay on the device: the loss weights and a GradScaler's factor ride in them)
        if g_cls is not None and g_cls.dtype != torch.float32:
            g_cls = g_cls.to(torch.float32)
        if g_div is not None and g_div.dtype != torch.float32:
            g_div = g_div.to(torch.float32)
        with _timed("moma_kdhead_bwd"):
            dz = torch.empty((B, K), device=logit_s.device, dtype=logit_s.dtype)
            check(lib.moma_kdhead_bwd(_ptr(logit_s), _ptr(logit_t), _ptr(labels), buf.data_ptr() + nw * 8, _ptr(g_cls), _ptr(g_div), _ptr(dz),
                                      B, K, *codes, T, _stream()), "moma_kdhead_bwd")
        return dz, None, None, None


def kd_head(logit_s, logit_t, labels, T):
    """(nn.CrossEntropyLoss()(logit_s, labels), DistillKL(T)(logit_s, logit_t), helper.util.accuracy(logit_s, labels)[0]) from one
    kernel pair.  logit_s, logit_t [B, K] float32 or bfloat16 (independently), contiguous; labels [B] int64; T a finite host float > 0
    -> (loss_cls, loss_div, acc), scalar float32 each.  loss_cls is the mean over the rows whose label is not -100; a label outside
    [0, K) other than -100 is never used as an index: loss_cls is NaN and that row's cross-entropy gradient zero (stock torch asserts
    on the device).  loss_div = T^2 KL(softmax(logit_t / T) || softmax(logit_s / T)) summed over the rows and divided by B; it does
    not look at labels.  acc = 100 x (rows whose lowest argmax equals their label) / B.  The gradients of loss_cls and loss_div flow to
    logit_s, in its dtype; logit_t gets none and acc is not differentiable."""
    # (one pass over the usual case, the reasons only when it fails: see ce_head)
    ok = (torch.is_tensor(logit_s) and logit_s.is_cuda and logit_s.dim() == 2 and logit_s.dtype in _DT_CODES and logit_s.is_contiguous()
          and logit_s.numel() > 0 and torch.is_tensor(logit_t) and logit_t.is_cuda and logit_t.dtype in _DT_CODES
          and logit_t.shape == logit_s.shape and logit_t.is_contiguous() and torch.is_tensor(labels) and labels.is_cuda
          and labels.dtype == torch.int64 and labels.shape == logit_s.shape[:1] and labels.is_contiguous())
    if not ok:
        _rows_side("kd_head", logit_s, "logit_s")
        _rows_side("kd_head", logit_t, "logit_t")
        if logit_t.shape != logit_s.shape:
            raise ValueError(f"kd_head: logit_t {tuple(logit_t.shape)} for logit_s {tuple(logit_s.shape)}")
        _dev(labels, "labels", torch.int64)
        if tuple(labels.shape) != (logit_s.shape[0],):
            raise ValueError(f"kd_head: labels {tuple(labels.shape)} for logits {tuple(logit_s.shape)}")
        raise ValueError(f"kd_head: empty logits {tuple(logit_s.shape)}")
    T = float(T)
    if not (0.0 < T < float("inf")):
        raise ValueError(f"kd_head: the temperature must be finite and > 0, got {T}")
    if logit_t.requires_grad and torch.is_grad_enabled():
        raise ValueError("kd_head: the kernels give no gradient to logit_t (detach it, or use helper.kd_head.StudentHead.composite)")
    return _KDHead.apply(logit_s, logit_t, labels, T)


# ------------------------------------------------------------------------------------------------
# What the losses on a B x B batch relation (rkd, sp, pkt: below) share: guards, the [B, D] view, the backward call
# ------------------------------------------------------------------------------------------------
def _rel_side(op, f, name):
    """-> [B, D] view of a contiguous [B, D] or [B, C, 1, 1] (any [B, ...]) float32 / bfloat16 device tensor (copied when not dense)"""
    _dev(f, name, dtype=None, contiguous=False)
    if f.dim() < 2 or f.dtype not in _DT_CODES:
        raise TypeError(f"{op}: {name} must be a float32 / bfloat16 tensor [B, ...], got {tuple(f.shape)} {f.dtype}")
    return f.contiguous().view(f.shape[0], -1)


def _rel_contiguous_sides(op, f_s, f_t):
    """the per-side guards of rkd_loss and pkt_loss: on the device, [B, ...] with at least two dimensions, contiguous"""
    for t, nm in ((f_s, "f_s"), (f_t, "f_t")):
        _dev(t, nm, dtype=None, contiguous=False)
        if t.dim() < 2:
            raise ValueError(f"{op}: {nm} must be [B, D] or [B, C, 1, 1], got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{op}: {nm} must be contiguous, got strides {tuple(t.stride())} for {tuple(t.shape)}")


def _rel_pair_guards(op, composite, f_s, f_t):
    """behind the per-side guards of the three losses: no gradient to f_t, equal batch sizes"""
    if f_t.requires_grad and torch.is_grad_enabled():
        raise ValueError(f"{op}: the kernels give no gradient to f_t (detach it, or use distiller_zoo.{composite}.composite)")
    if f_s.shape[0] != f_t.shape[0]:
        raise ValueError(f"{op}: batch sizes {f_s.shape[0]} and {f_t.shape[0]} differ")


def _rel_backward(entry, x, M, g, shape, strides):
    """the backward of the three losses: moma_<entry>_bwd(x read as [B, numel / B], M [B, B], g) -> dF_s in x's dtype with the
    input's shape and strides (the order the kernels read; extents of 1 may carry any stride: the input's)"""
    lib = _lib.load()
    B, name = x.shape[0], f"moma_{entry}_bwd"
    g = g.to(torch.float32).contiguous()              # the upstream gradient stays on the device (a GradScaler factor rides in it)
    with _timed(name):
        dF = torch.empty_strided(shape, strides, device=x.device, dtype=x.dtype)
        check(getattr(lib, name)(_ptr(x), _ptr(M), _ptr(g), _ptr(dF), B, x.numel() // B, _DT_CODES[x.dtype], _stream()), name)
    return dF


# ------------------------------------------------------------------------------------------------
# Relational Knowledge Distillation: pairwise distances and angles of a batch   (distiller_zoo/RKD.py, helper/loops_moma.py:155-158)
# ------------------------------------------------------------------------------------------------


class _RKDLoss(torch.autograd.Function):
    """rkd_dist x 2 -> rkd_terms (Q = d loss / d S_s, loss) in the forward; rkd_bwd (dF_s from f_s and Q) in the backward."""

    @staticmethod
    def forward(ctx, f_s, f_t, w_d, w_a):
        lib = _lib.load()
        shape = f_s.shape
        x, y = _rel_side("rkd_loss", f_s, "f_s"), _rel_side("rkd_loss", f_t, "f_t")
        B, dev = x.shape[0], x.device
        with _timed("moma_rkd_fwd"):
            n = lib.moma_rkd_workspace_bytes(B)
            if n == 0:
                raise ValueError(f"rkd_loss: the kernels take 2 .. {_lib.RKD_MAX_B} rows, got {B}")
            S = torch.empty(2, B, B, device=dev, dtype=torch.float64)
            Q = torch.empty(B, B, device=dev, dtype=torch.float64)
            ws = torch.empty(n // 8, device=dev, dtype=torch.float64)
            terms = torch.empty(2, device=dev, dtype=torch.float32)
            loss = torch.empty((), device=dev, dtype=torch.float32)
            for side, t in enumerate((x, y)):
                check(lib.moma_rkd_dist(_ptr(t), B, t.shape[1], _DT_CODES[t.dtype], _ptr(S[side]), _stream()), "moma_rkd_dist")
            check(lib.moma_rkd_terms(_ptr(S[0]), _ptr(S[1]), B, float(w_d), float(w_a), _ptr(ws), n, _ptr(Q), _ptr(terms), _ptr(loss),
                                     _stream()), "moma_rkd_terms")
        # (rkd_loss, the only caller, refuses an f_t that wants a gradient: backward runs only where f_s does, with these saved)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, Q)
        ctx.shape, ctx.strides = shape, f_s.stride()
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, Q = ctx.saved_tensors
        return _rel_backward("rkd", x, Q, g, ctx.shape, ctx.strides), None, None, None


def rkd_loss(f_s, f_t, w_d=25.0, w_a=50.0) -> torch.Tensor:
    """Relational Knowledge Distillation loss of one pair of feature batches, f_s [B, Ds] and f_t [B, Dt] (or [B, C, 1, 1]; float32
    or bfloat16, contiguous, independently per side; 2 <= B <= 1024) -> scalar float32:
    w_d * smooth_l1 of the mean-normalised pairwise distances + w_a * smooth_l1 of the angles at every anchor, both from the B x B
    matrices of squared distances in double (no [B, B, D] temporary).  The gradient flows to f_s only."""
    _rel_contiguous_sides("rkd_loss", f_s, f_t)
    _rel_pair_guards("rkd_loss", "RKDLoss", f_s, f_t)
    if f_s.shape[0] < 2:
        raise ValueError("rkd_loss: relations need at least two rows, got B = 1")
    return _RKDLoss.apply(f_s, f_t, float(w_d), float(w_a))


# ------------------------------------------------------------------------------------------------
# Similarity-Preserving distillation: row-normalised batch Gram of a feature pair   (distiller_zoo/SP.py, helper/loops_moma.py:140-144)
# ------------------------------------------------------------------------------------------------
def sp_dense(f) -> bool:
    """True where f [B, ...] can be read in storage order as [B, K] with row stride K: sample 0 is dense (its dimensions, in some
    order, are contiguous) and the batch stride is K -- contiguous and channels_last tensors alike"""
    K = 1
    for extent, stride in sorted(((e, s) for e, s in zip(f.shape[1:], f.stride()[1:]) if e != 1), key=lambda es: es[1]):
        if stride != K:
            return False
        K *= extent
    return f.shape[0] == 1 or f.stride(0) == K


def _sp_side(f, name):
    _dev(f, name, dtype=None, contiguous=False)
    if f.dim() < 2 or f.dtype not in _DT_CODES:
        raise TypeError(f"sp_loss: {name} must be a float32 / bfloat16 tensor [B, ...], got {tuple(f.shape)} {f.dtype}")
    if f.numel() == 0:
        raise ValueError(f"sp_loss: {name} is empty: {tuple(f.shape)}")
    if not sp_dense(f):
        raise ValueError(f"sp_loss: {name} must be dense with the same strides in every sample (contiguous or channels_last), got "
                         f"strides {tuple(f.stride())} for {tuple(f.shape)}")


class _SPLoss(torch.autograd.Function):
    """sp_gram x 2 -> sp_terms (G, H, M = Q + Q^T, loss) in the forward; sp_bwd (dF_s = g M f_s, in storage order) in the backward."""

    @staticmethod
    def forward(ctx, f_s, f_t):
        lib = _lib.load()
        B, dev = f_s.shape[0], f_s.device
        Ks, Kt = f_s.numel() // B, f_t.numel() // B
        with _timed("moma_sp_fwd"):
            n_s, n_t = lib.moma_sp_workspace_bytes(B, Ks), lib.moma_sp_workspace_bytes(B, Kt)
            if n_s == 0 or n_t == 0:
                raise ValueError(f"sp_loss: the kernels take 1 .. {_lib.SP_MAX_B} rows, got {B}")
            ws_s = torch.empty(n_s // 4, device=dev, dtype=torch.float32)
            ws_t = torch.empty(n_t // 4, device=dev, dtype=torch.float32)
            G = torch.empty(2, B, B, device=dev, dtype=torch.float64)
            H = torch.empty(2, B, B, device=dev, dtype=torch.float64)
            rows = torch.empty(4, B, device=dev, dtype=torch.float64)
            M = torch.empty(B, B, device=dev, dtype=torch.float64)
            loss = torch.empty((), device=dev, dtype=torch.float32)
            check(lib.moma_sp_gram(_ptr(f_s), B, Ks, _DT_CODES[f_s.dtype], _ptr(ws_s), n_s, _stream()), "moma_sp_gram")
            check(lib.moma_sp_gram(_ptr(f_t), B, Kt, _DT_CODES[f_t.dtype], _ptr(ws_t), n_t, _stream()), "moma_sp_gram")
            check(lib.moma_sp_terms(_ptr(ws_s), n_s, Ks, _ptr(ws_t), n_t, Kt, B, _ptr(G), _ptr(H), _ptr(rows), _ptr(M), _ptr(loss),
                                    _stream()), "moma_sp_terms")
        # (sp_loss, the only caller, refuses an f_t that wants a gradient: backward runs only where f_s does, with these saved)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(f_s, M)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        f_s, M = ctx.saved_tensors
        return _rel_backward("sp", f_s, M, g, f_s.shape, f_s.stride()), None


def sp_loss(f_s, f_t) -> torch.Tensor:
    """Similarity-Preserving loss of one pair of feature batches, f_s [B, ...] and f_t [B, ...] (float32 or bfloat16, contiguous or
    channels_last, independently per side; any sizes behind the batch; 1 <= B <= 1024) -> scalar float32:
    mean_ij (H^t_ij - H^s_ij)^2 with H the row-normalised B x B Gram matrix of a side's flattened samples.  The maps are read in
    storage order (the Gram matrix does not depend on the order of the columns); the gradient flows to f_s only, in f_s's strides."""
    for t, nm in ((f_s, "f_s"), (f_t, "f_t")):
        _sp_side(t, nm)
    _rel_pair_guards("sp_loss", "Similarity", f_s, f_t)
    if f_s.shape[0] > _lib.SP_MAX_B:
        raise ValueError(f"sp_loss: the kernels take 1 .. {_lib.SP_MAX_B} rows, got {f_s.shape[0]}")
    return _SPLoss.apply(f_s, f_t)


# ------------------------------------------------------------------------------------------------
# SemCKD: batch Gram of one map, and the attention-weighted per-sample MSE of all (student, teacher) pairs as one grouped call
# (models/util.py SelfA, distiller_zoo/SemCKD.py, helper/loops_moma.py:177-179)
# ------------------------------------------------------------------------------------------------
class _BatchGram(torch.autograd.Function):
    """sp_gram -> sp_gram_sum (G = X X^T, fp32) in the forward; sp_bwd with M = dG + dG^T in double and a device scalar 1 in the
    backward (dX = (dG + dG^T) X, in storage order)."""

    @staticmethod
    def forward(ctx, f):
        lib = _lib.load()
        B, dev = f.shape[0], f.device
        K = f.numel() // B
        with _timed("moma_batch_gram_fwd"):
            n = lib.moma_sp_workspace_bytes(B, K)
            if n == 0:
                raise ValueError(f"batch_gram: the kernels take 1 .. {_lib.SP_MAX_B} rows, got {B}")
            ws = torch.empty(n // 4, device=dev, dtype=torch.float32)
            G = torch.empty(B, B, device=dev, dtype=torch.float32)
            check(lib.moma_sp_gram(_ptr(f), B, K, _DT_CODES[f.dtype], _ptr(ws), n, _stream()), "moma_sp_gram")
            check(lib.moma_sp_gram_sum(_ptr(ws), n, K, B, _ptr(G), _stream()), "moma_sp_gram_sum")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(f)
        return G

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dG):
        f, = ctx.saved_tensors
        dG = dG.to(torch.float64)
        M = (dG + dG.t()).contiguous()
        one = torch.ones((), device=f.device, dtype=torch.float32)
        return _rel_backward("sp", f, M, one, f.shape, f.stride())


def batch_gram(f) -> torch.Tensor:
    """G = X X^T [B, B] float32 of f [B, ...] read as X [B, K] (float32 or bfloat16, contiguous or channels_last, 1 <= B <= 1024): the
    split-K Gram kernel of csrc/sp.hip and the sum of its partials in double.  The map is read in storage order (G does not depend
    on the order of the columns); the gradient (dG + dG^T) X comes in f's dtype and strides."""
    _dev(f, "f", dtype=None, contiguous=False)
    if f.dim() < 2 or f.dtype not in _DT_CODES:
        raise TypeError(f"batch_gram: f must be a float32 / bfloat16 tensor [B, ...], got {tuple(f.shape)} {f.dtype}")
    if f.numel() == 0:
        raise ValueError(f"batch_gram: f is empty: {tuple(f.shape)}")
    if not sp_dense(f):
        raise ValueError("batch_gram: f must be dense with the same strides in every sample (contiguous or channels_last), got "
                         f"strides {tuple(f.stride())} for {tuple(f.shape)}")
    if f.shape[0] > _lib.SP_MAX_B:
        raise ValueError(f"batch_gram: the kernels take 1 .. {_lib.SP_MAX_B} rows, got {f.shape[0]}")
    return _BatchGram.apply(f)


def _semckd_table(xs, ts, dxs):
    """-> the host array of moma_semckd_pair_t for the pairs (xs[p], ts[p]) with the gradients dxs[p] (None: no gradient wanted)"""
    tab = (_lib.SemckdPair * len(xs))()
    for p, (x, t, dx) in enumerate(zip(xs, ts, dxs)):
        tab[p] = _lib.SemckdPair(x.data_ptr(), t.data_ptr(), 0 if dx is None else dx.data_ptr(), x.numel() // x.shape[0],
                                 _DT_CODES[x.dtype], _DT_CODES[t.dtype])
    return tab


class _SemCKDWeightedMSE(torch.autograd.Function):
    """semckd_fwd (ind, loss) over all pairs in the forward; semckd_bwd (every dx) in the backward, d weight = g ind / (B S)."""

    @staticmethod
    def forward(ctx, weight, n_pairs, *maps):
        lib = _lib.load()
        xs, ts = maps[:n_pairs], maps[n_pairs:]
        B, S, T = weight.shape
        dev = weight.device
        with _timed("moma_semckd_fwd"):
            tab = _semckd_table(xs, ts, [None] * n_pairs)
            n = lib.moma_semckd_workspace_bytes(tab, n_pairs, B)
            if n == 0:
                raise ValueError(f"semckd_weighted_mse: no workspace for {n_pairs} pairs at B = {B}")
            buf = torch.empty(n // 8 + (B * n_pairs + 2) // 2, device=dev, dtype=torch.float64)   # (one allocation: workspace, ind, loss)
            ws, tail = buf[:n // 8], buf[n // 8:].view(torch.float32)
            ind, loss = tail[:B * n_pairs].view(B, S, T), tail[B * n_pairs:B * n_pairs + 1].view(())
            check(lib.moma_semckd_fwd(tab, n_pairs, S, B, _ptr(weight), _ptr(ws), n, _ptr(ind), _ptr(loss), _stream()),
                  "moma_semckd_fwd")
        ctx.save_for_backward(weight, ind, *maps)
        ctx.n_pairs = n_pairs
        ctx.mark_non_differentiable(ind)
        return loss, ind

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_ind):
        lib = _lib.load()
        weight, ind = ctx.saved_tensors[:2]
        n_pairs = ctx.n_pairs
        maps = ctx.saved_tensors[2:]
        xs, ts = maps[:n_pairs], maps[n_pairs:]
        B, S, T = weight.shape
        g = g.to(torch.float32).contiguous()          # the upstream gradient stays on the device (a GradScaler factor rides in it)
        need = ctx.needs_input_grad
        dxs = [torch.empty_like(x) if need[2 + p] else None for p, x in enumerate(xs)]   # (same dtype, same strides)
        if any(dx is not None for dx in dxs):
            with _timed("moma_semckd_bwd"):
                tab = _semckd_table(xs, ts, dxs)
                check(lib.moma_semckd_bwd(tab, n_pairs, S, B, _ptr(weight), _ptr(g), _stream()), "moma_semckd_bwd")
        dw = ind * (g / float(B * S)) if need[0] else None
        return (dw, None, *dxs, *([None] * n_pairs))


def semckd_native(n_pairs: int) -> bool:
    """Whether a group of `n_pairs` pairs runs on csrc/semckd.hip (one call): up to MOMA_SEMCKD_MAX_PAIRS; larger groups take
    distiller_zoo.SelfA.composite."""
    return 1 <= n_pairs <= _lib.SEMCKD_MAX_PAIRS


def semckd_weighted_mse(s_values, targets, weight):
    """The tail of SemCKD over ALL pairs in one call: s_values[i][j] (the projection of student map i for teacher map j) and
    targets[i][j] (teacher map j on the common grid), S lists of T tensors [B, C, h, w] each (float32 or bfloat16 per tensor, the two
    maps of a pair of one shape and one memory format, contiguous or channels_last), weight [B, S, T] float32 ->
    (loss, ind): ind[b,i,j] = mean_k (s - t)^2 float32, loss = sum(weight * ind) / (B S) scalar float32.
    Gradients flow to every s_value (in its dtype and strides) and to weight; targets get none, ind is not differentiable."""
    S, T = len(s_values), len(s_values[0])
    xs = [x for row in s_values for x in row]
    ts = [t for row in targets for t in row]
    if len(targets) != S or any(len(r) != T for r in s_values) or any(len(r) != T for r in targets):
        raise ValueError("semckd_weighted_mse: s_values and targets must be S lists of T tensors each")
    _dev(weight, "weight", torch.float32)
    if tuple(weight.shape[1:]) != (S, T) or weight.dim() != 3:
        raise ValueError(f"semckd_weighted_mse: weight {tuple(weight.shape)} for {S} x {T} pairs")
    if not semckd_native(S * T):
        raise ValueError(f"semckd_weighted_mse: the kernels take 1 .. {_lib.SEMCKD_MAX_PAIRS} pairs, got {S * T} (use "
                         "distiller_zoo.SelfA.composite)")
    B = weight.shape[0]
    for p, (x, t) in enumerate(zip(xs, ts)):
        for f, nm in ((x, f"s_values[{p // T}][{p % T}]"), (t, f"targets[{p // T}][{p % T}]")):
            _dev(f, nm, dtype=None, contiguous=False)
            if f.dtype not in _DT_CODES or f.dim() < 2 or f.shape[0] != B or f.numel() == 0:
                raise TypeError(f"semckd_weighted_mse: {nm} must be a float32 / bfloat16 tensor [{B}, ...], got {tuple(f.shape)} {f.dtype}")
            if not sp_dense(f):
                raise ValueError(f"semckd_weighted_mse: {nm} must be contiguous or channels_last, got strides {tuple(f.stride())} "
                                 f"for {tuple(f.shape)} (use distiller_zoo.SelfA.composite)")
        if x.shape != t.shape or any(e != 1 and a != b for e, a, b in zip(x.shape, x.stride(), t.stride())):
            raise ValueError(f"semckd_weighted_mse: pair {p}: s_value {tuple(x.shape)} / {tuple(x.stride())} and target "
                             f"{tuple(t.shape)} / {tuple(t.stride())} must share shape and memory format")
        if t.requires_grad and torch.is_grad_enabled():
            raise ValueError("semckd_weighted_mse: the kernels give no gradient to a target (detach it, or use "
                             "distiller_zoo.SelfA.composite)")
    return _SemCKDWeightedMSE.apply(weight, S * T, *xs, *ts)


# ------------------------------------------------------------------------------------------------
# Probabilistic Knowledge Transfer: cosine Gram of a batch as row distributions, their KL   (distiller_zoo/PKT.py, helper/loops_moma.py:159-162)
# ------------------------------------------------------------------------------------------------
class _PKTLoss(torch.autograd.Function):
    """pkt_gram_pair (both sides, one launch) -> pkt_terms (M with dF_s = g M f_s, loss; two launches) in the forward; pkt_bwd in the
    backward: one."""

    @staticmethod
    def forward(ctx, f_s, f_t):
        lib = _lib.load()
        shape = f_s.shape
        x, y = _rel_side("pkt_loss", f_s, "f_s"), _rel_side("pkt_loss", f_t, "f_t")
        B, dev = x.shape[0], x.device
        with _timed("moma_pkt_fwd"):
            n = lib.moma_pkt_workspace_bytes(B)
            if n == 0:
                raise ValueError(f"pkt_loss: the kernels take 1 .. {_lib.PKT_MAX_B} rows, got {B}")
            G = torch.empty(2, B, B, device=dev, dtype=torch.float64)
            M = torch.empty(B, B, device=dev, dtype=torch.float64)
            ws = torch.empty(n // 8, device=dev, dtype=torch.float64)
            loss = torch.empty((), device=dev, dtype=torch.float32)
            check(lib.moma_pkt_gram_pair(_ptr(x), x.shape[1], _DT_CODES[x.dtype], _ptr(y), y.shape[1], _DT_CODES[y.dtype], B, _ptr(G[0]),
                                         _ptr(G[1]), _stream()), "moma_pkt_gram_pair")
            check(lib.moma_pkt_terms(_ptr(G[0]), _ptr(G[1]), B, _ptr(ws), n, _ptr(M), _ptr(loss), _stream()), "moma_pkt_terms")
        # (pkt_loss, the only caller, refuses an f_t that wants a gradient: backward runs only where f_s does, with these saved)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, M)
        ctx.shape, ctx.strides = shape, f_s.stride()
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, M = ctx.saved_tensors
        return _rel_backward("pkt", x, M, g, ctx.shape, ctx.strides), None


def pkt_loss(f_s, f_t) -> torch.Tensor:
    """Probabilistic Knowledge Transfer loss of one pair of feature batches, f_s [B, Ds] and f_t [B, Dt] (or [B, C, 1, 1]; float32
    or bfloat16, contiguous, independently per side; 1 <= B <= 1024) -> scalar float32:
    mean_ij T_ij log((T_ij + 1e-7) / (P_ij + 1e-7)), P and T the row-normalised (cosine + 1) / 2 matrices of the student's and the
    teacher's batch, from the raw B x B Gram matrices in double (no normalised copy of either side).  The gradient flows to f_s only;
    an all-zero student row gets a finite gradient (the reference's autograd: NaN)."""
    _rel_contiguous_sides("pkt_loss", f_s, f_t)
    _rel_pair_guards("pkt_loss", "PKT", f_s, f_t)
    if f_s.shape[0] > _lib.PKT_MAX_B:
        raise ValueError(f"pkt_loss: the kernels take 1 .. {_lib.PKT_MAX_B} rows, got {f_s.shape[0]}")
    return _PKTLoss.apply(f_s, f_t)


# ------------------------------------------------------------------------------------------------
# The input batch: uint8 rows of a data pack -> the tensor the backbones read   (dataset/histo_dataset.py:194-239, :1054-1058)
# ------------------------------------------------------------------------------------------------
def input_lut(mean, std, device=None) -> torch.Tensor:
    """lut [3, 256] float32: lut[c][v] is what ToTensor + Normalize make of level v in channel c, in their order of operations
    (v / 255, minus the mean, over the std; each rounded to float32), so the kernel's outputs equal theirs bit for bit."""
    v = torch.arange(256, dtype=torch.float32)
    rows = [v.div(255).sub(float(m)).div(float(s)) for m, s in zip(mean, std)]
    if len(rows) != 3:
        raise ValueError("input_lut: mean and std have three entries each")
    lut = torch.stack(rows).contiguous()
    return lut if device is None else lut.to(device)


def input_batch(src, lut, size, idx=None, flip=None, box=None, resample=False, batch=None, dtype=torch.float32,
                channels_last=False, out=None) -> torch.Tensor:
    """src uint8 [N, H, W, 3] (device, contiguous) -> [B, 3, S_h, S_w] of `dtype` (float32 or bfloat16), contiguous or, with
    `channels_last`, in torch.channels_last strides; one launch of csrc/input.hip.  `size` is S or (S_h, S_w).  idx int64 [B]: the
    rows of src (None: rows 0 .. B - 1, B = `batch` or N); flip uint8 / bool [B] (None: none); box int32 [B, 4] = (top, left, h, w)
    (None: the centred window, CenterCrop's offsets).  resample False: the S_h x S_w window at (top, left); True: the box resampled
    bilinearly onto S_h x S_w.  `out`: a destination of that shape, dtype and memory format instead of a new tensor.  See
    include/moma_hip.h (IN) for the arithmetic."""
    lib = _lib.load()
    _dev(src, "src", torch.uint8)
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f"input_batch: src must be [N, H, W, 3], got {tuple(src.shape)}")
    _dev(lut, "lut", torch.float32)
    if tuple(lut.shape) != (3, 256):
        raise ValueError(f"input_batch: lut must be [3, 256], got {tuple(lut.shape)}")
    if dtype not in _DT_CODES:
        raise TypeError(f"input_batch: dtype must be float32 or bfloat16, got {dtype}")
    N, H, W = src.shape[:3]
    Sh, Sw = (size, size) if isinstance(size, int) else size
    B = None
    for t, name, dt, shape in ((idx, "idx", torch.int64, None), (flip, "flip", None, None), (box, "box", torch.int32, 4)):
        if t is None:
            continue
        _dev(t, name, dt)
        if name == "flip" and t.dtype not in (torch.uint8, torch.bool):
            raise TypeError(f"input_batch: flip must be uint8 or bool, got {t.dtype}")
        if t.dim() != (1 if shape is None else 2) or (shape is not None and t.shape[1] != shape):
            raise ValueError(f"input_batch: {name} has shape {tuple(t.shape)}")
        if B is not None and t.shape[0] != B:
            raise ValueError(f"input_batch: {name} has {t.shape[0]} rows, the batch {B}")
        B = t.shape[0]
    if batch is not None:
        if B is not None and B != batch:
            raise ValueError(f"input_batch: batch = {batch} but the operands have {B} rows")
        B = batch
    if B is None:
        B = N
    if idx is None and B > N:
        raise ValueError(f"input_batch: a batch of {B} from {N} rows needs idx")
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    if out is None:
        out = torch.empty((B, 3, Sh, Sw), device=src.device, dtype=dtype, memory_format=fmt)
    else:
        _dev(out, "out", dtype, contiguous=False)
        if tuple(out.shape) != (B, 3, Sh, Sw) or not out.is_contiguous(memory_format=fmt):
            raise ValueError(f"input_batch: out must be a dense [{B}, 3, {Sh}, {Sw}] tensor in the requested memory format")
    with _timed("moma_input_batch"):
        check(lib.moma_input_batch(_ptr(src), _ptr(idx), _ptr(flip), _ptr(box), _ptr(lut), _ptr(out), N, H, W, B, Sh, Sw,
                                   1 if resample else 0, _DT_CODES[dtype], _lib.LAYOUT_NHWC if channels_last else _lib.LAYOUT_NCHW,
                                   _stream()), "moma_input_batch")
    return out
