"""The generic GEMM (csrc/gemm.hip) and the row kernels around it (rowops.hip) against float64, on the two chains that are built from
them alone: the materialised InfoNCE logits with all three gradients, and the staged attention path where the fused K1 kernels do
not take over.  `launch_gemm` picks its kernel from shape, alignment, dtype and policy only, so every case below is a shape that was
derived -- from linear_ksplit_ok, vec_ok, tiles64 < 192 and logits_bwd_splitk -- to reach one variant; the variant is written next
to the shape.  Notation: ksplit<TRA,TRB> = linear_ksplit_kernel (bf16 policy only; `ragged` = M or N no multiple of 32, so the
clamped rows arow / brow are read; `rem r` = (K/16) % 4, the k-steps left over after the even split over the four waves),
tiled TM VA/VB = gemm_kernel with the 32 x 32 (BK = 128) or 64 x 64 (BK = 32) tile and 16-byte (1) or element (0) loads per operand.

The yardstick and the allowance are those of tests/gemm_ref.py: float64 on operands rounded exactly as the policy rounds them,
and 4 x the distance of the same evaluation in float32 (never less than 2^-21) -- the bf16 policy gets the fp32-class bound, not
2e-2 of the largest element, so a dropped K-tail term or a tail row read from its clamped neighbour (about 1e-2 of a result) fails.
Every test prints `ratio` lines: measured error / allowance per tensor."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import gemm_ref as R
from tests.test_gpu_kernels import _t, ops  # noqa: F401  (`ops` is the module-scoped fixture)

gpu = pytest.mark.gpu
T = 0.15
INV_T = float(np.float32(1.0 / T))            # what the library is handed: the C ABI takes inv_T as a float


def _check(what, got, ref, f32, names):
    worst = 0.0
    bad = []
    for nm in names:
        g = got[nm].detach().cpu()
        assert torch.isfinite(g).all(), (what, nm)
        err, allow = R.dist(g, ref[nm]), R.allowance(f32[nm], ref[nm])
        print(f"ratio {what} {nm}: err {err:.3e} allowance {allow:.3e} ratio {err / allow:.3f}")
        worst = max(worst, err / allow)
        if not err <= allow:
            bad.append((nm, err, allow))
    print(f"ratio {what} WORST {worst:.3f}")
    assert not bad, (what, bad)


# ================================================================================================ A: materialised logits
# (B, d, K).  Products: fwd = q . queue^T [B x K over d]; dq = dlogits[:,1:] . queue [B x d over K, A = dlogits + 1 is never
# 16-byte aligned: VA = 0, split-K]; dqueue = dlogits[:,1:]^T . q [K x d over B, transposed A with lda = K + 1].
LOGITS_CASES = [
    # the golden's size.  fwd tiled TM32 VA1 VB1; dq splitk = 1 WITH a workspace: the atomic branch over the initialised dq;
    # dqueue tiled TM32 VA0 VB1 tA tB (B = 6 < 64: not ksplit)
    (6, 32, 24),
    # bf16: fwd ksplit<0,0> ragged rem 0 (d = 64: one k-step per wave).  dq splitk = 2, but the TM32 kernel's BK = 128 covers K = 40
    # in its first split: the second writes an all-zero partial.  dqueue tiled TM32
    (8, 64, 40),
    # bf16: fwd ksplit<0,0> full tiles, dqueue ksplit<1,1> full tiles rem 0 (B = 64: one k-step per wave); dq splitk = 3.  fp32: all tiled TM32
    (64, 128, 96),
    # bf16: fwd ksplit<0,0> ragged (M = 80, N = 100), dqueue ksplit<1,1> ragged M = K = 100 (clamped arow) rem 1 (B/16 = 5); dq splitk = 4
    (80, 128, 100),
    # B % 16 != 0: dqueue falls back to tiled TM32 VA0 VB1 tA tB under bf16 too; d = 100 keeps 16-byte loads with a 4-wide tail
    # (100 = 3 x 32 + 4); fwd tiled (d % 16 != 0); dq splitk = 5
    (72, 100, 130),
    # d % 4 != 0: element loads on every operand of every product (VA0 VB0), everything ragged; dq splitk = 9
    (33, 50, 257),
    # one row.  bf16: fwd ksplit<0,0> with M = 1 (31 clamped rows); dqueue tiled (contraction over B = 1); dq splitk = 4
    (1, 64, 100),
    # exactly 1024 tiles of 32 x 32 for dqueue (64 x 16): the last shape linear_ksplit_ok accepts -> ksplit<1,1> under bf16;
    # fp32: tiled TM64 (256 tiles of 64 x 64).  fwd bf16 ksplit<0,0> (512 tiles).  dq splitk = 32 at TM64
    (256, 512, 2048),
    # 1040 tiles: the first shape it refuses -> the tiled bf16 kernel at TM64 with VA0 (dlogits + 1, lda = K + 1) VB1, tA tB
    (256, 512, 2080),
    # dqueue at 191 tiles of 64 x 64 -> TM32 under fp32 (bf16: ksplit<1,1>, 764 tiles, rem 0); fwd tiled TM64 VA1 VB1 under either
    # policy (4 x 382 = 1528 tiles of 32 x 32: past linear_ksplit_ok); dq splitk = 382 at TM64
    (128, 64, 12224),
    # dqueue at 192 tiles -> TM64 under fp32 (bf16: ksplit<1,1>, 768 tiles); dq splitk = 384
    (128, 64, 12288),
    # d % 4 == 0 with d < 64 (never ksplit), everything ragged; lda = K + 1 = 132 is a multiple of 4, and the last 16-byte vector
    # along K would hold three elements -- but through ops dlogits + 1 is never 16-byte aligned (VA0): the vector loader's tail is
    # reached by test_logits_bwd_vector_loader_tail below, which places dlogits so that dlogits + 1 is aligned
    (67, 36, 131),
]


@functools.lru_cache(maxsize=None)
def _logits_inputs(B, d, K, qdt):
    g = torch.Generator().manual_seed(7 * B + 3 * d + K)
    q = torch.nn.functional.normalize(torch.randn(B, d, generator=g))
    k = torch.nn.functional.normalize(torch.randn(B, d, generator=g))
    queue = torch.nn.functional.normalize(torch.randn(K, d, generator=g))
    if qdt == "bf16":
        queue = queue.bfloat16()
    w = torch.randn(B, K + 1, generator=g)
    return q, k, queue, w


@functools.lru_cache(maxsize=None)
def _logits_ref(B, d, K, qdt, prec):
    """(float64 reference, float32 evaluation) of the four results: computed once per case, shared, never modified"""
    q, k, queue, w = _logits_inputs(B, d, K, qdt)
    rnd = R.rnd_of(prec)
    return (R.logits_chain(q, k, queue.float(), w, INV_T, rnd, torch.float64),
            R.logits_chain(q, k, queue.float(), w, INV_T, rnd, torch.float32))


@gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("B,d,K", LOGITS_CASES)
def test_logits_and_all_three_gradients(ops, B, d, K, prec):
    """fp32 queue; q, k and the queue require grad: logits, dq (moma_infonce_logits_bwd_ws), dk and dqueue (moma_infonce_logits_bwd_kq)"""
    q0, k0, queue0, w0 = _logits_inputs(B, d, K, "fp32")
    q, k, queue = (_t(a.numpy()).requires_grad_(True) for a in (q0, k0, queue0))
    logits = ops.infonce_logits(q, k, queue, T, prec)
    (logits * _t(w0.numpy())).sum().backward()
    ref, f32 = _logits_ref(B, d, K, "fp32", prec)
    _check(f"logits {(B, d, K)} {prec}", dict(logits=logits, dq=q.grad, dk=k.grad, dqueue=queue.grad), ref, f32,
           ("logits", "dq", "dk", "dqueue"))


@gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("B,d,K", LOGITS_CASES)
def test_logits_over_a_bf16_stored_queue(ops, B, d, K, prec):
    """bf16 B operand (gemm_kernel<.., bf16_raw, ..>: element loads on B, never ksplit); only q requires grad"""
    q0, k0, queue0, w0 = _logits_inputs(B, d, K, "bf16")
    q = _t(q0.numpy()).requires_grad_(True)
    logits = ops.infonce_logits(q, _t(k0.numpy()), queue0.cuda(), T, prec)
    (logits * _t(w0.numpy())).sum().backward()
    ref, f32 = _logits_ref(B, d, K, "bf16", prec)
    _check(f"logits bf16-queue {(B, d, K)} {prec}", dict(logits=logits, dq=q.grad), ref, f32, ("logits", "dq"))


def _p(t, off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("B,d,K", [(80, 128, 100), (256, 512, 2080)])      # splitk = 4 at TM32, 32 at TM64
def test_logits_bwd_atomic_form_and_ws_form_repeatable(ops, B, d, K, prec):
    """moma_infonce_logits_bwd (no workspace: the K splits meet in fp32 atomics over the initialised dq) against the same reference
    under the same allowance -- not bitwise equal to the _ws form, whose partials are added in split order; that form gives the
    same bits in three calls"""
    from moma_amd import _lib
    lib = _lib.load()
    q0, k0, queue0, w0 = _logits_inputs(B, d, K, "fp32")
    k, queue, dl = _t(k0.numpy()), _t(queue0.numpy()), _t(w0.numpy())
    code = ops.prec_code(prec)
    dq = torch.full((B, d), float("nan"), device="cuda")
    assert lib.moma_infonce_logits_bwd(_p(dl), _p(k), _p(queue), _p(dq), B, d, K, INV_T, _lib.DT_F32, code, _st()) == 0
    ref, f32 = _logits_ref(B, d, K, "fp32", prec)
    _check(f"logits_bwd atomic {(B, d, K)} {prec}", dict(dq=dq), ref, f32, ("dq",))
    nbytes = lib.moma_infonce_logits_bwd_workspace_bytes(B, d, K)
    outs = []
    for _ in range(3):
        ws = torch.full((nbytes,), 0xFF, device="cuda", dtype=torch.uint8)
        o = torch.full((B, d), float("nan"), device="cuda")
        assert lib.moma_infonce_logits_bwd_ws(_p(dl), _p(k), _p(queue), _p(o), B, d, K, INV_T, _lib.DT_F32, code, _p(ws), nbytes, _st()) == 0
        outs.append(o)
    _check(f"logits_bwd ws {(B, d, K)} {prec}", dict(dq=outs[0]), ref, f32, ("dq",))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_logits_bwd_vector_loader_tail(ops, prec):
    """The 1-3 element tail of load_tile's 16-byte variant needs a vector dimension that is no multiple of 4 under a leading
    dimension that is one: only A = dlogits + 1 (lda = K + 1) with K % 4 == 3 qualifies, and only when dlogits + 1 is 16-byte
    aligned -- a dlogits that starts 12 bytes into a vector, which the C ABI accepts (alignment to the element size).  (67, 36, 131):
    dq tiled TM32 VA1 VB1, splitk = 5 of which the second holds K = 128..130 (lim = 3 along K); dqueue tiled TM32 VA1 VB1 tA tB
    with lim = 3 along the rows M = K = 131 at row 128"""
    from moma_amd import _lib
    lib = _lib.load()
    B, d, K = 67, 36, 131
    q0, k0, queue0, w0 = _logits_inputs(B, d, K, "fp32")
    q, k, queue = _t(q0.numpy()), _t(k0.numpy()), _t(queue0.numpy())
    buf = torch.full((B * (K + 1) + 8,), float("nan"), device="cuda")
    dl = buf[3:3 + B * (K + 1)].view(B, K + 1)
    dl.copy_(w0)
    assert buf.data_ptr() % 16 == 0 and (dl.data_ptr() + 4) % 16 == 0
    code = ops.prec_code(prec)
    nbytes = lib.moma_infonce_logits_bwd_workspace_bytes(B, d, K)
    ws = torch.full((nbytes,), 0xFF, device="cuda", dtype=torch.uint8)
    dq, dk, dqueue = (torch.full(s, float("nan"), device="cuda") for s in ((B, d), (B, d), (K, d)))
    assert lib.moma_infonce_logits_bwd_ws(_p(dl), _p(k), _p(queue), _p(dq), B, d, K, INV_T, _lib.DT_F32, code, _p(ws), nbytes, _st()) == 0
    assert lib.moma_infonce_logits_bwd_kq(_p(dl), _p(q), _p(dk), _p(dqueue), B, d, K, INV_T, code, _st()) == 0
    ref, f32 = _logits_ref(B, d, K, "fp32", prec)
    _check(f"logits_bwd aligned dlogits+1 {(B, d, K)} {prec}", dict(dq=dq, dk=dk, dqueue=dqueue), ref, f32, ("dq", "dk", "dqueue"))


@gpu
def test_logits_bwd_argument_checks(ops):
    """all refused (or accepted as nothing to do) before any launch"""
    from moma_amd import _lib
    lib = _lib.load()
    B, d, K = 80, 128, 100
    q0, k0, queue0, w0 = _logits_inputs(B, d, K, "fp32")
    q, k, queue, dl = _t(q0.numpy()), _t(k0.numpy()), _t(queue0.numpy()), _t(w0.numpy())
    nbytes = lib.moma_infonce_logits_bwd_workspace_bytes(B, d, K)
    assert nbytes >= 4 * B * d * 4                                           # splitk = 4 partials
    ws = torch.zeros(nbytes + 16, device="cuda", dtype=torch.uint8)
    dq = torch.full((B, d), 7.0, device="cuda")
    args = (_p(dl), _p(k), _p(queue), _p(dq), B, d, K, INV_T, _lib.DT_F32, _lib.PREC_BF16)
    assert lib.moma_infonce_logits_bwd_ws(*args, _p(ws), nbytes - 1, _st()) == -5            # MOMA_E_WORKSPACE
    assert lib.moma_infonce_logits_bwd_ws(*args, _p(ws, 4), nbytes, _st()) == -4             # MOMA_E_ALIGN
    assert lib.moma_infonce_logits_bwd_kq(_p(dl), _p(q), None, None, B, d, K, INV_T, _lib.PREC_BF16, _st()) == 0     # nothing asked
    assert lib.moma_infonce_logits_bwd_kq(_p(dl), _p(q), _p(dq), _p(dq), 0, d, K, INV_T, _lib.PREC_BF16, _st()) == -2   # MOMA_E_SHAPE
    torch.cuda.synchronize()
    assert bool((dq == 7.0).all()) and bool((ws == 0).all())
    assert torch.equal(dl.cpu(), w0) and torch.equal(q.cpu(), q0)


# ================================================================================================ B: staged attention
# (N, d, H, scale of w_qkv).  Twelve products per case (see gemm_ref.staged_mha_chain); S = q k^T and dP = dA v^T contract over
# hd < 64 and are tiled under either policy; under fp32 every product is tiled.
MHA_CASES = [
    # hd = 12.  bf16: everything else in linear_ksplit: qkv, proj <0,0> rem 2 (d/16 = 6); dA, dx <0,1>; P V, dQ <0,1> x 8 heads
    # (N = hd-ragged: brow clamped); dW_proj, dW_qkv <1,1> with the fused column sum; dV, dK <1,1> x 8 heads; N/16 = 4: rem 0
    (64, 96, 8, 1.0),
    # hd = 24.  ragged 32-row tiles, 80 = 2 x 32 + 16 (arow clamped in qkv / proj / dA / dx); N/16 = 5: rem 1 in the products over N
    (80, 192, 8, 1.0),
    # N > 256, N % 16 == 0: N/16 = 19 k-steps -> 5, 5, 5, 4 per wave (rem 3); d/16 = 6: rem 2; S / dP at TM64 (25 tiles x 8 heads)
    (304, 96, 8, 1.0),
    # N % 16 != 0 and d % 16 != 0: every product in the tiled kernel under bf16 too (VA1 VB1), bias gradients from colsum_vec_kernel
    (300, 72, 6, 1.0),
    # hd = 25: head stride % 4 != 0 -> S, dP with element loads (VA0 VB0); the linears stay 16-byte (d = 100, d % 16 != 0: tiled);
    # bf16: products over N = 128 in ksplit (<0,1> / <1,1> take a K-major B at any stride), column sums fused
    (128, 100, 4, 1.0),
    # hd = 10, d % 4 != 0: element loads throughout, bias gradients from colsum_kernel
    (37, 50, 5, 1.0),
    # a single token (softmax over one column; workspace offsets of dP / dqkv not 16-byte aligned: VA0, colsum_kernel for db_qkv)
    (1, 24, 2, 1.0),
    # w_qkv x 8: peaked softmax rows, scores in the tens -- the row-max subtraction matters
    (64, 96, 8, 8.0),
]
OLD_BOUND = {"bf16": 3e-2, "fp32": 3e-5}      # test_mha_vs_oracle's


@functools.lru_cache(maxsize=None)
def _mha_ref(N, d, H, wscale, prec):
    inp = R.mha_inputs(N, d, H, wscale)
    rnd = R.rnd_of(prec)
    return (inp, R.staged_mha_chain(H=H, rnd=rnd, dtype=torch.float64, **inp), R.staged_mha_chain(H=H, rnd=rnd, dtype=torch.float32, **inp))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("N,d,H,wscale", MHA_CASES)
def test_staged_mha_yardstick_on_the_cpu(N, d, H, wscale, prec):
    """the float32 restatement alone: finite at every shape, and the allowance it yields is inside the bound test_mha_vs_oracle
    uses for the policy -- the new bound is never looser than that one"""
    _, ref, f32 = _mha_ref(N, d, H, wscale, prec)
    for nm in R.MHA_NAMES:
        assert torch.isfinite(f32[nm]).all() and torch.isfinite(ref[nm]).all(), nm
        assert R.FLOOR <= R.allowance(f32[nm], ref[nm]) <= OLD_BOUND[prec], (nm, R.allowance(f32[nm], ref[nm]))


@gpu
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("N,d,H,wscale", MHA_CASES)
def test_staged_mha_all_six_results(ops, N, d, H, wscale, prec):
    from moma_amd import _lib
    assert _lib.load().moma_mha_saved_state(N, d, H, ops.prec_code(prec)) == _lib.MHA_SAVE_PROBS       # the staged path takes it
    inp, ref, f32 = _mha_ref(N, d, H, wscale, prec)
    x = _t(inp["x"].numpy()).requires_grad_(True)
    ws = [_t(inp[nm].numpy()).requires_grad_(True) for nm in ("w_qkv", "b_qkv", "w_proj", "b_proj")]
    y = ops.mha(x, *ws, H, prec)
    (y * _t(inp["dy"].numpy())).sum().backward()
    got = dict(zip(R.MHA_NAMES, [y] + [t.grad for t in [x] + ws]))
    _check(f"mha {(N, d, H)} x{wscale:g} {prec}", got, ref, f32, R.MHA_NAMES)
