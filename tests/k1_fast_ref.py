"""torch-CPU restatements of the K1 fast attention path (moma_amd/csrc/k1_fast.hip), one function per launch, evaluated in float64 -- the
yardstick of tests/test_gpu_k1_fast_paths.py -- or in float32 -- the measure of what fp32 accumulation alone costs at a shape.

Every function rounds to bf16 (round to nearest even) exactly where the kernels store or load bf16, and nowhere else.  The
rounding points, read from k1_fast.hip (line numbers of that file):

  forward
    x at fragment load             kc_body, fp32 A operand packed into the LDS image: 165-166 (a bf16 x is consumed as it stands)
    the weight pack                k1_pack_kernel: 414-415 (W), 424-425 (W^T, the same values transposed)
    qkv16                          kc_body epilogue: fp32 accumulator + fp32 bias, the Q third times hd^-1/2 * log2(e) in fp32
                                   (launch_mha_fwd_fast: 1231, 1239), then the bf16 store: 222-225
    P before P . V                 tile_as_a: 85-86, called at 541 (narrow cores) and 719-720 (wide cores).  P = 2^(S - lse) is
                                   ALREADY normalised when it is rounded: the cores subtract the merged row log-sum-exp (563, 585,
                                   718); there is no division by a row sum after the product
    attn16                         the fp32 sum of the eight waves' partial O, stored as bf16: 611 (narrow), 768 (wide)
    y, lse                         fp32, never rounded (220, 590 / 713); qpack = bf16(y * qpack_scale), the product in fp32: 244-245
  backward
    dy at fragment load            kc_body (dA = dy Wproj): 165-166; ks_load_pair (dWproj = dy^T a, dbproj): 258
    dA                             kc_body epilogue, bf16 store with no scale: 222-225
    D = rowsum(dA o a)             the FP32 dA accumulators times the bf16 attn16, partial sums per 16 columns: 229-237, added up
                                   in fp32 by the core: 866 / 883 (narrow), 1005 / 1012 (wide)
    P (for dV) and dS              P = 2^(S - lse) stays fp32 inside dS = P (dP - D) c; c = hd^-1/2 for dQ, ln 2 for dK (whose other
                                   operand is the pre-scaled Q): 914-916 / 1085-1087.  Rounded by tile_as_a: dS at 925 and 945, P at
                                   936 (narrow); 1090, 1093 (wide)
    dqkv16                         reduce_store16: 818
    x at fragment load             ks_load_pair (dWqkv = dqkv^T x): 258
    the bias gradients             column sums of the ROUNDED bf16 values the product loads (bf16(dy) for dbproj, dqkv16 for dbqkv):
                                   288-289; see the comment above ks_load_pair

Two kinds of comparison are built on these (see the test module): a single launch fed the bf16 state the launch before it
actually wrote has no rounding between its inputs and a fp32 result, so gemm_ref.allowance (4 x the float32 evaluation's distance
from float64, floor 2^-21) applies as it stands; the backward from the saved state to dx / d_wqkv / d_bqkv passes four internal
roundings (dA, P, dS, dqkv16) and is measured in the Frobenius norm against a quarter of what those roundings move (`rnd_mid`)."""
import math

import numpy as np
import torch

from tests.gemm_ref import _heads, _unheads, bf16_rt, ident  # noqa: F401

LN2_F32 = float(np.float32(0.6931471805599453))


def q_prescale(hd):
    """hd^-1/2 * log2(e) as launch_mha_fwd_fast forms it in fp32"""
    return float(np.float32(1.4426950408889634) / np.sqrt(np.float32(hd)))


def bwd_scale(hd):
    return float(np.float32(1.0) / np.sqrt(np.float32(hd)))


def bf16_half_ulp(t):
    """half a bf16 ulp (8 significant bits) at the magnitude of each element of t, as float64"""
    a = t.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 8.0)


def frob(got, ref):
    ref = ref.double()
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ forward, launch by launch
def pack_weights(w_qkv, w_proj):
    """k1_pack_kernel: the bf16 values of the pack as float32 tensors (the transposed halves hold the same values)"""
    return bf16_rt(w_qkv.float()), bf16_rt(w_proj.float())


def qkv_linear(x, wqkv16, b_qkv, H, dtype):
    """launch 1 of the forward: what qkv16 holds BEFORE its bf16 store"""
    d = x.shape[1]
    acc = bf16_rt(x.float()).to(dtype) @ wqkv16.to(dtype).T
    if b_qkv is not None:
        acc = acc + b_qkv.to(dtype)
    acc[:, :d] = acc[:, :d] * q_prescale(d // H)
    return acc


def core_fwd(qkv16, H, dtype, rnd=bf16_rt):
    """launch 2: lse [H,N] in log2 units, and attn [N,d] BEFORE its bf16 store"""
    d = qkv16.shape[1] // 3
    t = qkv16.to(dtype)
    q, k, v = _heads(t[:, :d], H), _heads(t[:, d:2 * d], H), _heads(t[:, 2 * d:], H)
    s = q @ k.transpose(1, 2)
    m = s.max(-1, keepdim=True).values
    lse = m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))
    p = rnd(torch.exp2(s - lse))
    return lse[..., 0], _unheads(p @ v)


def proj_linear(attn16, wproj16, b_proj, dtype):
    """launch 3"""
    return attn16.to(dtype) @ wproj16.to(dtype).T + b_proj.to(dtype)


def forward_state(x, w_qkv, b_qkv, w_proj, b_proj, H, dtype):
    """the whole forward, every store rounded: the saved state a backward starts from (CPU checks of the yardstick)"""
    wqkv16, wproj16 = pack_weights(w_qkv, w_proj)
    qkv16 = bf16_rt(qkv_linear(x, wqkv16, b_qkv, H, dtype).float())
    lse, attn = core_fwd(qkv16, H, dtype)
    attn16 = bf16_rt(attn.float())
    return dict(wqkv16=wqkv16, wproj16=wproj16, qkv16=qkv16, attn16=attn16, lse=lse.float(),
                y=proj_linear(attn16, wproj16, b_proj, dtype))


# ------------------------------------------------------------------------------------------------ backward, launch by launch
def bwd_launch1(dy, attn16, wproj16, H, dtype):
    """dA (before its bf16 store), D [H,N], d_wproj, d_bproj"""
    dy16, a = bf16_rt(dy.float()).to(dtype), attn16.to(dtype)
    dA = dy16 @ wproj16.to(dtype)
    return dict(dA=dA, D=_heads(dA * a, H).sum(-1), d_wproj=dy16.T @ a, d_bproj=dy16.sum(0))


def core_bwd_mid(qkv16, dA16, lse, D, H, dtype):
    """what tile_as_a rounds: P [H,N,N], dS for dQ (times hd^-1/2) and dS for dK (times ln 2), all BEFORE the rounding"""
    d = qkv16.shape[1] // 3
    t = qkv16.to(dtype)
    qs, k, v = _heads(t[:, :d], H), _heads(t[:, d:2 * d], H), _heads(t[:, 2 * d:], H)
    p = torch.exp2(qs @ k.transpose(1, 2) - lse.to(dtype)[..., None])
    g = p * (_heads(dA16.to(dtype), H) @ v.transpose(1, 2) - D.to(dtype)[..., None])
    return dict(p=p, ds_q=g * bwd_scale(d // H), ds_k=g * LN2_F32)


def core_bwd_products(qkv16, dA16, p16, ds_q16, ds_k16, H, dtype):
    """dqkv [N,3d] before its bf16 store, from the rounded P and dS"""
    d = qkv16.shape[1] // 3
    t = qkv16.to(dtype)
    qs, k, dA = _heads(t[:, :d], H), _heads(t[:, d:2 * d], H), _heads(dA16.to(dtype), H)
    dq = ds_q16.to(dtype) @ k
    dk = ds_k16.to(dtype).transpose(1, 2) @ qs
    dv = p16.to(dtype).transpose(1, 2) @ dA
    return torch.cat([_unheads(dq), _unheads(dk), _unheads(dv)], 1)


def core_bwd(qkv16, dA16, lse, D, H, dtype, rnd):
    """launch 2 of the backward; `rnd` is applied to P and dS where tile_as_a rounds them"""
    m = core_bwd_mid(qkv16, dA16, lse, D, H, dtype)
    return core_bwd_products(qkv16, dA16, rnd(m["p"]), rnd(m["ds_q"]), rnd(m["ds_k"]), H, dtype)


def bwd_launch3(dqkv16, x, wqkv16, dtype):
    g = dqkv16.to(dtype)
    return dict(d_wqkv=g.T @ bf16_rt(x.float()).to(dtype), d_bqkv=g.sum(0), dx=g @ wqkv16.to(dtype))


BWD_NAMES = ("dx", "d_wqkv", "d_bqkv")


def backward(state, x, dy, H, dtype, rnd_mid=bf16_rt):
    """the three launches chained from a saved state (wqkv16, wproj16, qkv16, attn16, lse).  rnd_mid = bf16_rt: every rounding of
    the kernels; rnd_mid = ident: only the input roundings (x, weights, dy) and the saved state itself are kept"""
    l1 = bwd_launch1(dy, state["attn16"], state["wproj16"], H, dtype)
    dqkv = core_bwd(state["qkv16"], rnd_mid(l1["dA"]), state["lse"], l1["D"], H, dtype, rnd_mid)
    out = bwd_launch3(rnd_mid(dqkv), x, state["wqkv16"], dtype)
    out.update(d_wproj=l1["d_wproj"], d_bproj=l1["d_bproj"])
    return out


def inputs(N, d, H, qk_scale=1.0):
    """gemm_ref.mha_inputs with the Q and K thirds of w_qkv times `qk_scale` (peaked softmax rows)"""
    from tests.gemm_ref import mha_inputs
    inp = mha_inputs(N, d, H)
    inp["w_qkv"][:2 * d] *= qk_scale
    return inp


def row_max_p(qkv16, H):
    """the largest probability of every softmax row [H,N]: how peaked a case is"""
    d = qkv16.shape[1] // 3
    t = qkv16.double()
    sc = _heads(t[:, :d], H) @ _heads(t[:, d:2 * d], H).transpose(1, 2)
    return torch.softmax(sc * math.log(2.0), -1).max(-1).values
