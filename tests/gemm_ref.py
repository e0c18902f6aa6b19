"""torch-CPU restatements of what the generic GEMM stages compute (csrc/gemm.hip, rowops.hip, and the chains api.hip builds from
them), evaluated in float64 -- the yardstick of tests/test_gpu_gemm_paths.py -- or in float32 -- the measure of how much fp32
accumulation alone costs at a given shape.

Under the bf16 policy the GEMM rounds BOTH operands of a product to bf16 (round to nearest even) at fragment load, accumulates in
fp32 and applies alpha in fp32; under the fp32 policy the operands stay as they are.  Every product here therefore takes a `rnd`
hook applied to both operands: `bf16_rt` for the bf16 policy, `ident` for fp32.  What remains between a kernel and the float64
evaluation is fp32 accumulation error under either policy, so both policies get the same allowance:

    4 x (distance of the float32 evaluation from the float64 one), never less than 2^-21

distances being max|a - ref| / max|ref| per tensor.  The factor 4 is for the other summation order (MFMA blocks of 4 or 32, four
K quarters, split-K partials: both orders grow like sqrt(L) * 2^-24); the floor is about three fp32 roundings per element
(accumulate, alpha, partial sum) with a margin under 3.  Row reductions that the kernels do in plain fp32 on unrounded operands
(the positive logit, dk, the bias gradients) are restated unrounded."""
import math

import torch

FLOOR = 2.0 ** -21
FACTOR = 4.0


def ident(t):
    return t


def bf16_rt(t):
    """bf16 round trip (round to nearest even) in the tensor's own dtype"""
    return t.float().bfloat16().to(t.dtype)


def rnd_of(prec):
    return bf16_rt if prec == "bf16" else ident


def dist(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def allowance(f32_eval, ref):
    return max(FACTOR * dist(f32_eval, ref), FLOOR)


# ------------------------------------------------------------------------------------------------ materialised logits
def logits_chain(q, k, queue, w, inv_T, rnd, dtype):
    """moma_infonce_logits and the three gradients of (logits * w).sum(): logits [B,K+1], dq, dk [B,d], dqueue [K,d].
    inv_T is the fp32 value the library is handed."""
    q, k, queue, w = (t.to(dtype) for t in (q, k, queue, w))
    pos = (q * k).sum(1, keepdim=True)                                     # pos_logit_kernel: fp32 fma chain, unrounded
    neg = rnd(q) @ rnd(queue).T
    logits = torch.cat([pos, neg], 1) * inv_T
    w0, w1 = w[:, :1], w[:, 1:]
    dq = w0 * k * inv_T + (rnd(w1) @ rnd(queue)) * inv_T                   # pos_grad_init, then the split-K product on top
    dk = w0 * q * inv_T                                                    # pos_grad_init alone
    dqueue = (rnd(w1).T @ rnd(q)) * inv_T
    return dict(logits=logits, dq=dq, dk=dk, dqueue=dqueue)


# ------------------------------------------------------------------------------------------------ staged attention
def _heads(t, H):
    N, d = t.shape
    return t.reshape(N, H, d // H).permute(1, 0, 2)                        # [H,N,hd]


def _unheads(t):
    H, N, hd = t.shape
    return t.permute(1, 0, 2).reshape(N, H * hd)


def staged_mha_chain(x, w_qkv, b_qkv, w_proj, b_proj, H, dy, rnd, dtype):
    """moma_mha_fwd + moma_mha_bwd as api.hip stages them: the same products in the same association (four forward, eight
    backward), `rnd` on both operands of each, softmax and its backward as rowops.hip writes them, bias gradients as plain column
    sums of the unrounded operand."""
    x, w_qkv, b_qkv, w_proj, b_proj, dy = (t.to(dtype) for t in (x, w_qkv, b_qkv, w_proj, b_proj, dy))
    N, d = x.shape
    hd = d // H
    scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hd), dtype=torch.float32).sqrt())

    def mm(a, b):
        return rnd(a) @ rnd(b)

    qkv = mm(x, w_qkv.T) + b_qkv
    q, k, v = _heads(qkv[:, :d], H), _heads(qkv[:, d:2 * d], H), _heads(qkv[:, 2 * d:], H)
    s = mm(q, k.transpose(1, 2)) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e * (1.0 / e.sum(-1, keepdim=True))
    a = _unheads(mm(p, v))
    y = mm(a, w_proj.T) + b_proj

    d_wproj = mm(dy.T, a)
    d_bproj = dy.sum(0)
    dA = _heads(mm(dy, w_proj), H)
    dv = mm(p.transpose(1, 2), dA)
    dp = mm(dA, v.transpose(1, 2))
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
    dq = mm(ds, k)
    dk = mm(ds.transpose(1, 2), q)
    dqkv = torch.cat([_unheads(dq), _unheads(dk), _unheads(dv)], 1)
    d_wqkv = mm(dqkv.T, x)
    d_bqkv = dqkv.sum(0)
    dx = mm(dqkv, w_qkv)
    return dict(y=y, dx=dx, d_wqkv=d_wqkv, d_bqkv=d_bqkv, d_wproj=d_wproj, d_bproj=d_bproj)


MHA_NAMES = ("y", "dx", "d_wqkv", "d_bqkv", "d_wproj", "d_bproj")


def mha_inputs(N, d, H, wscale=1.0, seed=None):
    """x of unit rows, weights and biases as nn.Linear initialises them (w_qkv times `wscale`), dy ~ N(0,1)"""
    g = torch.Generator().manual_seed(1000 * N + 10 * d + H if seed is None else seed)
    bound = 1.0 / math.sqrt(d)

    def uni(*shape):
        return (torch.rand(*shape, generator=g) * 2 - 1) * bound

    x = torch.nn.functional.normalize(torch.randn(N, d, generator=g))
    return dict(x=x, w_qkv=uni(3 * d, d) * wscale, b_qkv=uni(3 * d), w_proj=uni(d, d), b_proj=uni(d),
                dy=torch.randn(N, d, generator=g))
