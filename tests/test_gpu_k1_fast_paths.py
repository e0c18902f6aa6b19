"""The K1 fast attention path (moma_amd/csrc/k1_fast.hip: weight pack, grouped job-list GEMM, narrow and wide per-head cores, the backward of
each) launch by launch against float64, through the C ABI (moma_mha_pack_weights / moma_mha_fwd_fast / moma_mha_bwd_fast).  The
restatements, and the list of rounding points with their source lines, are in tests/k1_fast_ref.py.

The path hands its saved state to the caller -- the pack, qkv16, attn16, lse -- so every launch is checked from the bf16 values the
launch before it ACTUALLY wrote.  Between such inputs and a result there is no rounding boundary an intermediate could land on
the other side of, which is what keeps an end-to-end bound at 3e-2.

A.  One launch, no internal rounding.
    fp32 results (lse from qkv16; y from attn16 and the pack; d_wproj, d_bproj from dy and attn16): max|err| / max|ref| within
    gemm_ref.allowance = 4 x the float32 evaluation's distance from the float64 one, floor 2^-21.
    bf16 results (qkv16 from x and the pack; attn16 from qkv16), element by element:
        |got - ref64| <= half a bf16 ulp of ref64 + that allowance x max|ref64|
    with at most one element in 1000 off by one further ulp (ties; a P of attn16 rounded the other way).  The share is a cap, not
    a measurement; test_yardstick_on_the_cpu confirms the float32 evaluation stays inside it at every case.
B.  The backward from the saved state and dy to dx, d_wqkv, d_bqkv passes dA, P, dS and dqkv16, which are not exposed: an
    intermediate may round the other way than in float64 ("flip", one bf16 ulp of one element).  Measure: the relative Frobenius
    distance, which sparse flips do not move.  Allowance, from the reference alone: a QUARTER of the Frobenius distance between
    the float64 restatement with every rounding and the float64 restatement with the intermediate roundings removed (the
    "intermediate-rounding effect", 1.5e-3 .. 2.8e-3 here).  fp32 accumulation alone costs at most 1/4 of that allowance, 1/16 of
    the effect (test_float32_cost_of_the_backward_is_a_small_part_of_the_allowance); what a kernel is left with is flips, which
    cascade from stage to stage and were measured at up to 0.513 of the allowance: a margin of about 2.  A dropped k-step, a
    clamped tail row, a wrong tile pairing cost several times the effect, a truncating store about the effect itself.

Every GPU test prints `ratio` lines (error / allowance).  Worst measured on an MI355X, all 21 cases, no fault found:
    test_single_launch_results (A)      fp32 results: 0.359 (lse at (304, 128, 8)); y <= 0.24, d_wproj <= 0.20, d_bproj <= 0.09.
                                        bf16 results: qkv16 never over its bound (worst element 1.000 of it); attn16 over the bound
                                        in at most 5 of 81920 elements ((256, 320, 1), 1/16 of the cap; 4 of 33024 at
                                        (129, 256, 2)), none beyond one further ulp
    test_backward_from_saved_state (B)  0.513 (dx at (64, 48, 1)), then 0.505 (d_wqkv, same case), 0.324 (dx at (260, 256, 2));
                                        every other case <= 0.24

Cases: derived from launch_mha_fwd_fast / launch_mha_bwd_fast / mha_fast_supported (k1_fast.hip) and checked against
moma_mha_saved_state; the variant a case reaches is written next to it.  Notation: fwd<ONE_TILE,FULL> = k1_core_fwd_kernel,
bwd<FULL> = k1_core_bwd_kernel, wide<TW> = k1_core_fwd_wide_kernel<TW> + k1_core_bwd_wide_kernel<TW> (TW = ceil(N / 256) key tiles
per wave), kc = kc_body (32 x 32 tiles: token rows x output columns), ks = ks_body (64 x 64 tiles of a weight gradient, k-steps
of 16 tokens split over four waves: `rem` = ceil(N / 16) & 3 k-steps left after the even split)."""
import ctypes as C
import functools

import pytest
import torch

from tests import gemm_ref as R
from tests import k1_fast_ref as K

gpu = pytest.mark.gpu
OLD_BOUND = 3e-2                                  # test_mha_vs_oracle's, the tightest of the five end-to-end tests
OUTLIER_SHARE = 1000                              # one element in 1000 ...
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def ops():
    """the loaded library; the GPU tests take it so that a machine without a GPU skips them"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _lib()[1]

# (N, d, H, scale of the Q and K thirds of w_qkv)
CASES = [
    # ---- narrow cores (hd <= 128)
    # hd = 16, fwd<1,0> with 2 of 8 waves holding keys, the second a tile of ONE key; bwd<0>.  kc: M = 33 (tile of one row), ks:
    # 3 k-steps, the last with one live token (tokens past K zeroed), rem 3, base 0: wave 3 idle.  d_bproj / d_bqkv: tn == 0 of 2 / 2
    (33, 128, 8, 1.0),
    # hd = 48: kse = 3, nct = 2 with a half-used column tile; fwd<1,0>.  d = 192: ks tiles 3 x 3 (M = 192), N = 77: 5 k-steps, rem 1,
    # the last with 13 live tokens
    (77, 192, 4, 1.0),
    # hd = 128: fwd<1,1>, bwd<1>, N = 32 * 4 + 1: the fifth wave's tile holds one key, three waves run fully masked; 9 k-steps, rem 1
    (129, 256, 2, 1.0),
    # N > 256: fwd<0,0> (two passes; waves 0, 1 take two key tiles, tile 9 has 12 keys); bwd<0> with two tiles on waves 0, 1;
    # 19 k-steps (rem 3), the last with 12 live tokens
    (300, 128, 8, 1.0),
    # hd = 128 at N > 256: fwd<0,1> -- the fourth instantiation; 17 k-steps, rem 1, N = 260: the last key tile holds 4 keys
    (260, 256, 2, 1.0),
    # one token: softmax over one key (lse = the score), 31 clamped rows in every image, one k-step with one live token
    (1, 64, 4, 1.0),
    # ---- ks_body: rem = 0, 1, 2, 3 at whole k-steps (N / 16 = 4, 5, 6, 19).  base >= 1 only at N = 64 x 4 / 304: the straight-line
    # chunk of four k-steps is reached by the 19-step case (wave 0..2: 5 steps = one chunk + 1)
    # d = 48, H = 1: ks M = 48 / 144, no multiple of 64 -> columns 2c >= M - 2 clamp to M - 2 (through the C ABI M = d or 3d is
    # always a multiple of 16, so an odd M does not exist; the clamp is what a ragged 64-tile reaches); kc N = 48 / 144: a 16-column
    # tile, the dpart epilogue with gcol >> 4 = 2 only half a tile; column sums with tn == 0 the only tile (N = 48 < 64)
    (64, 48, 1, 1.0),
    (80, 128, 8, 1.0),                            # rem 1; column sums: tn == 0 of two (d_wproj) / two (d_wqkv) column tiles
    (96, 64, 4, 1.0),                             # rem 2; hd = 16, d = 64: one ks tile per 64 rows, tn == 0 only
    (304, 128, 8, 1.0),                           # rem 3 with full k-steps, base 4: the chunked loop, N > 256
    # ---- peaked rows: rows dominated by one or two keys, so that a key tile paired with another tile's values cannot average out.
    # N = 200: 7 key tiles on 7 waves.  With these inputs a score has standard deviation s^2 / (3 d) before log2(e): Q and K
    # thirds x 8 give 0.17 and leave the rows flat (kept as one more flat case at another weight scale); x 60 gives 9.4 -- the largest
    # P of a row is 0.77 on average (asserted in test_yardstick_on_the_cpu): this is the peaked case
    (200, 128, 8, 8.0),
    (200, 128, 8, 60.0),
    # ---- wide cores (hd > 128)
    # hd = 160: wide<1>, one full segment and one of 32 columns (kse = 2, nct = 1)
    (37, 320, 2, 1.0),
    # hd = 144 / 272: the last segment is a single 16-column k-step (nch = 2, nct = 1 half used)
    (100, 288, 2, 1.0),
    (64, 1088, 4, 1.0),
    # hd = 320 at N = 256: wide<1> with every wave's tile full, segments 128 + 128 + 64; one head, the smallest shape that reaches
    # it, and the `--head None` configuration itself (d = 1280, four heads; kc: 10 K segments, 3 / 3 / 2 / 2 per wave)
    (256, 320, 1, 1.0),
    (256, 1280, 4, 1.0),
    # hd = 512 (d = 2048, the one case at this width): four full segments; kc: 16 K segments, 4 per wave
    (130, 2048, 4, 1.0),
    # wide<2>, <3>, <4>: N = 256 (TW - 1) + 1, the smallest N of each (N <= 304 does not reach them); the last tile of wave 0
    # holds one key, the other waves' last tiles are fully masked
    (257, 288, 2, 1.0),
    (513, 288, 2, 1.0),
    (769, 288, 2, 1.0),
]
IDS = [f"{N}x{d}h{H}" + ("" if s == 1.0 else f"x{s:g}") for N, d, H, s in CASES]


# ------------------------------------------------------------------------------------------------ comparison helpers
def _maxnorm(what, nm, got, ref, f32, bad):
    assert torch.isfinite(got).all(), (what, nm)
    err, allow = R.dist(got, ref), R.allowance(f32, ref)
    print(f"ratio {what} {nm}: err {err:.3e} allowance {allow:.3e} ratio {err / allow:.3f}")
    if not err <= allow:
        bad.append((nm, err, allow))
    return err / allow


def _elementwise(got16, ref64, f32):
    """the bf16-stored results of A -> (largest err / bound over the elements, elements over the bound, elements over bound + 1 ulp)"""
    half = K.bf16_half_ulp(ref64)
    bound = half + R.allowance(f32, ref64) * ref64.abs().max()
    err = (got16.double() - ref64).abs()
    return float((err / bound).max()), int((err > bound).sum()), int((err > bound + 2 * half).sum())


def _bf16_result(what, nm, got16, ref64, f32, bad):
    assert torch.isfinite(got16).all(), (what, nm)
    worst, over, far = _elementwise(got16, ref64, f32)
    cap = got16.numel() // OUTLIER_SHARE
    print(f"ratio {what} {nm}: worst element err / bound {worst:.3f}, over the bound {over} of {got16.numel()} (cap {cap}), beyond one more ulp {far}")
    if over > cap or far:
        bad.append((nm, worst, over, cap, far))
    return worst


def _frob(what, nm, got, ref_all, ref_inputs_only, bad):
    assert torch.isfinite(got).all(), (what, nm)
    err, allow = K.frob(got, ref_all), 0.25 * K.frob(ref_inputs_only, ref_all)
    print(f"ratio {what} {nm}: frobenius err {err:.3e} allowance {allow:.3e} ratio {err / allow:.3f}")
    if not err <= allow:
        bad.append((nm, err, allow))
    return err / allow


# ------------------------------------------------------------------------------------------------ the yardstick itself (CPU)
@functools.lru_cache(maxsize=None)
def _inputs(N, d, H, s):
    return K.inputs(N, d, H, s)


@pytest.mark.parametrize("N,d,H,s", CASES, ids=IDS)
def test_yardstick_on_the_cpu(N, d, H, s):
    """No kernel: the saved state is the float64 restatement's own.  Both evaluations finite; the float32 evaluation inside the
    element cap of A; every allowance, in the measure of the five end-to-end tests
    (max|err| / max|ref|; for B: a quarter of the intermediate-rounding effect in that measure), below a quarter of their
    tightest bound"""
    inp = _inputs(N, d, H, s)
    x, dy = inp["x"], inp["dy"]
    st = K.forward_state(inp["x"], inp["w_qkv"], inp["b_qkv"], inp["w_proj"], inp["b_proj"], H, F64)
    a64, a32 = {}, {}
    for dt, o in ((F64, a64), (F32, a32)):
        o["qkv16"] = K.qkv_linear(x, st["wqkv16"], inp["b_qkv"], H, dt)
        o["lse"], o["attn16"] = K.core_fwd(st["qkv16"], H, dt)
        o["y"] = K.proj_linear(st["attn16"], st["wproj16"], inp["b_proj"], dt)
        l1 = K.bwd_launch1(dy, st["attn16"], st["wproj16"], H, dt)
        o["d_wproj"], o["d_bproj"] = l1["d_wproj"], l1["d_bproj"]
    for nm in a64:
        assert torch.isfinite(a64[nm]).all() and torch.isfinite(a32[nm]).all(), nm
        allow = R.allowance(a32[nm], a64[nm])
        if nm in ("qkv16", "attn16"):
            worst, over, far = _elementwise(R.bf16_rt(a32[nm]), a64[nm], a32[nm])
            assert over <= a64[nm].numel() // OUTLIER_SHARE and far == 0, (nm, worst, over, far)
            allow += 2.0 ** -8                                             # half a bf16 ulp, relative, at its largest
        assert R.FLOOR <= allow < OLD_BOUND / 4, (nm, allow)
    b_all, b_in = (K.backward(st, x, dy, H, F64, rnd) for rnd in (R.bf16_rt, R.ident))
    for nm in K.BWD_NAMES:
        assert torch.isfinite(b_all[nm]).all() and torch.isfinite(b_in[nm]).all(), nm
        assert 0 < 0.25 * R.dist(b_in[nm], b_all[nm]) < OLD_BOUND / 4, nm
    if s >= 60:
        assert float(torch.exp2(a64["lse"]).max()) < 1e30 and float(K.row_max_p(st["qkv16"], H).mean()) > 0.7


def _f32_stages(N, d, H, s):
    """float32 against float64 with no flip possible -> ({result: (distance, B allowance)}, {stage: distance}, least B allowance).
    Results: the whole backward with NO intermediate rounding in either evaluation.  Stages: launch by launch, every launch of
    BOTH evaluations fed the float64 chain's rounded intermediates, each output taken before its own store."""
    inp = _inputs(N, d, H, s)
    x, dy = inp["x"], inp["dy"]
    st = K.forward_state(x, inp["w_qkv"], inp["b_qkv"], inp["w_proj"], inp["b_proj"], H, F64)
    b_all, b_in, u32 = (K.backward(st, x, dy, H, dt, rnd) for dt, rnd in ((F64, R.bf16_rt), (F64, R.ident), (F32, R.ident)))
    results = {nm: (K.frob(u32[nm], b_in[nm]), 0.25 * K.frob(b_in[nm], b_all[nm])) for nm in K.BWD_NAMES}
    l1 = {dt: K.bwd_launch1(dy, st["attn16"], st["wproj16"], H, dt) for dt in (F64, F32)}
    dA16, D = R.bf16_rt(l1[F64]["dA"]), l1[F64]["D"]
    mid = {dt: K.core_bwd_mid(st["qkv16"], dA16, st["lse"], D, H, dt) for dt in (F64, F32)}
    r16 = {nm: R.bf16_rt(t) for nm, t in mid[F64].items()}
    dqkv = {dt: K.core_bwd_products(st["qkv16"], dA16, r16["p"], r16["ds_q"], r16["ds_k"], H, dt) for dt in (F64, F32)}
    l3 = {dt: K.bwd_launch3(R.bf16_rt(dqkv[F64]), x, st["wqkv16"], dt) for dt in (F64, F32)}
    stages = {nm: K.frob(l1[F32][nm], l1[F64][nm]) for nm in ("dA", "D")}
    stages.update({nm: K.frob(mid[F32][nm], mid[F64][nm]) for nm in ("p", "ds_q", "ds_k")})
    stages["dqkv"] = K.frob(dqkv[F32], dqkv[F64])
    stages.update({nm: K.frob(l3[F32][nm], l3[F64][nm]) for nm in K.BWD_NAMES})
    return results, stages, min(allow for _, allow in results.values())


@pytest.mark.parametrize("N,d,H,s", CASES, ids=IDS)
def test_float32_cost_of_the_backward_is_a_small_part_of_the_allowance(N, d, H, s):
    """What fp32 accumulation alone costs the backward, measured where no intermediate can round the other way, is at most 1/4 of
    the allowance of B (1/16 of the intermediate-rounding effect): for dx, d_wqkv, d_bqkv through the whole chain with the
    intermediate roundings removed from both evaluations, and for every launch's outputs before their store (dA, D; P and both
    dS; dqkv; the three results) with the launch fed the float64 chain's rounded intermediates.  Measured: at most 0.004 of that
    quarter at every case but the one-token case, 0.18 there (dS = P (dP - D) is all cancellation at N = 1).

    NOT asserted: the float32 evaluation of the chain WITH its roundings.  Its distance from float64 was measured at 0.00 .. 0.34 of
    the allowance of B, erratic from case to case and from one BLAS to another ((260, 256, 2): 0.15 and 0.33), so no bound on it
    can be checked reliably.  It consists of flips alone, as the figures above show, and flips cascade: a dA or P rounded the other
    way is an error of 2^-9 .. 2^-8 in an operand of the next product, which moves a whole row or column of the next stage's
    results and rounds some of those the other way in turn (at (256, 1280, 4): 0.015 % of dA16 differ, and the three results by
    1.9e-4).  A kernel is subject to the same flips: the allowance of B leaves them a margin of about 2 (largest measured share
    0.513), not more."""
    results, stages, least = _f32_stages(N, d, H, s)
    what, bad = f"k1 f32 {(N, d, H)} x{s:g}", []
    for nm, (err, allow) in results.items():
        print(f"ratio {what} unrounded chain {nm}: frobenius {err:.3e} quarter of the allowance {allow / 4:.3e} ratio {4 * err / allow:.3f}")
        if not err <= allow / 4:
            bad.append((nm, err, allow / 4))
    for nm, err in stages.items():
        print(f"ratio {what} launch by launch {nm}: frobenius {err:.3e} quarter of the least allowance {least / 4:.3e} ratio {4 * err / least:.3f}")
        if not err <= least / 4:
            bad.append((nm, err, least / 4))
    assert least > 0 and not bad, (what, bad)


def test_bf16_half_ulp():
    t = torch.tensor([1.0, 1.5, 1.9999, 2.0, -3.0, 0.75, 2.0 ** -20])
    assert torch.equal(K.bf16_half_ulp(t), torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -9, 2.0 ** -28], dtype=F64))
    # the largest rounding error of a bf16 store is exactly that: 1 + 2^-8 is a tie between 1 and 1 + 2^-7
    v = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20])
    assert float((R.bf16_rt(v) - v).abs()) <= float(K.bf16_half_ulp(v))


# ------------------------------------------------------------------------------------------------ C ABI plumbing
def _p(t, off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from moma_amd import _lib as L
    return L, L.load()


def _pack(w_qkv, w_proj, with_t=1):
    L, lib = _lib()
    d = w_proj.shape[0]
    assert lib.moma_mha_pack_bytes(d) == 16 * d * d
    buf = torch.zeros(8 * d * d, device="cuda", dtype=torch.bfloat16)
    assert lib.moma_mha_pack_weights(_p(w_qkv), _p(w_proj), _p(buf), d, with_t, _st()) == 0
    return buf


class _Mod:
    """the buffers of one module of a moma_mha_fwd_fast call (outputs pre-filled with NaN)"""

    def __init__(self, x, pack, b_qkv, b_proj, H, lse=True, qpack=None, qscale=0.0):
        N, d = x.shape
        self.x, self.pack, self.b_qkv, self.b_proj, self.qpack, self.qscale = x, pack, b_qkv, b_proj, qpack, qscale
        self.y = torch.full((N, d), float("nan"), device="cuda")
        self.qkv16 = torch.full((N, 3 * d), float("nan"), device="cuda", dtype=torch.bfloat16)
        self.attn16 = torch.full((N, d), float("nan"), device="cuda", dtype=torch.bfloat16)
        self.lse = torch.full((H, N), float("nan"), device="cuda") if lse else None

    def fill(self, m, L):
        m.x, m.pack, m.b_qkv, m.b_proj = _p(self.x), _p(self.pack), _p(self.b_qkv), _p(self.b_proj)
        m.y, m.qkv16, m.attn16, m.lse = _p(self.y), _p(self.qkv16), _p(self.attn16), _p(self.lse)
        m.qpack, m.qpack_scale = _p(self.qpack), self.qscale
        m.x_dtype = L.DT_BF16 if self.x.dtype == torch.bfloat16 else L.DT_F32

    def bits(self):
        return [self.y, self.qkv16.view(torch.int16), self.attn16.view(torch.int16)] + ([] if self.lse is None else [self.lse])


def _fwd(mods, N, d, H, n=None):
    L, lib = _lib()
    arr = (L.MhaModule * max(len(mods), 1))()
    for m, mod in zip(arr, mods):
        mod.fill(m, L)
    return lib.moma_mha_fwd_fast(C.cast(arr, C.c_void_p), len(mods) if n is None else n, N, d, H, _st())


BWD_OUT = ("dx", "dw_qkv", "db_qkv", "dw_proj", "db_proj")


def _bwd(mod, dy, H, skip=(), fill=float("nan"), ws_short=0, pack_off=0):
    """moma_mha_bwd_fast over the saved state of `mod`: workspace of exactly the advertised size, poisoned; outputs pre-filled"""
    L, lib = _lib()
    N, d = mod.x.shape
    nbytes = lib.moma_mha_bwd_fast_workspace_bytes(N, d, H)
    assert nbytes >= (4 * N * d) * 2 + (d // 16) * N * 4
    ws = torch.full((nbytes,), 0xFF, device="cuda", dtype=torch.uint8)
    shapes = dict(dx=(N, d), dw_qkv=(3 * d, d), db_qkv=(3 * d,), dw_proj=(d, d), db_proj=(d,))
    out = {nm: None if nm in skip else torch.full(shapes[nm], fill, device="cuda") for nm in BWD_OUT}
    rc = lib.moma_mha_bwd_fast(_p(mod.pack, pack_off), _p(mod.x), L.DT_BF16 if mod.x.dtype == torch.bfloat16 else L.DT_F32, _p(mod.qkv16),
                               _p(mod.attn16), _p(mod.lse), _p(dy), *[_p(out[nm]) for nm in BWD_OUT], _p(ws), nbytes - ws_short, N, d, H, _st())
    return rc, out


def _module_for(inp, H, x_bf16=False, **kw):
    x = inp["x"].bfloat16().cuda() if x_bf16 else inp["x"].cuda()
    g = {nm: inp[nm].cuda() for nm in ("w_qkv", "b_qkv", "w_proj", "b_proj")}
    return _Mod(x, _pack(g["w_qkv"], g["w_proj"]), g["b_qkv"], g["b_proj"], H, **kw)


@functools.lru_cache(maxsize=None)
def _gpu_run(N, d, H, s):
    """one forward and one backward of a case on the GPU, shared by A and B; everything returned on the CPU, never modified"""
    L, lib = _lib()
    assert lib.moma_mha_saved_state(N, d, H, L.PREC_BF16) == L.MHA_SAVE_LSE           # the fast path takes it
    inp = _inputs(N, d, H, s)
    mod = _module_for(inp, H)
    assert _fwd([mod], N, d, H) == 0
    rc, out = _bwd(mod, inp["dy"].cuda(), H)
    assert rc == 0
    torch.cuda.synchronize()
    pk = mod.pack.float().cpu()
    got = dict(wqkv16=pk[:3 * d * d].view(3 * d, d), wproj16=pk[3 * d * d:4 * d * d].view(d, d), qkv16=mod.qkv16.float().cpu(),
               attn16=mod.attn16.float().cpu(), lse=mod.lse.cpu(), y=mod.y.cpu())
    got.update(dx=out["dx"].cpu(), d_wqkv=out["dw_qkv"].cpu(), d_bqkv=out["db_qkv"].cpu(), d_wproj=out["dw_proj"].cpu(),
               d_bproj=out["db_proj"].cpu())
    return got


# ------------------------------------------------------------------------------------------------ A
@gpu
@pytest.mark.parametrize("N,d,H,s", CASES, ids=IDS)
def test_single_launch_results(ops, N, d, H, s):
    """A: qkv16 from x and the pack, lse and attn16 from the kernel's qkv16, y from its attn16, d_wproj and d_bproj from dy and its
    attn16.  Worst ratios measured: see "Worst measured on an MI355X" in the module docstring"""
    inp, g = _inputs(N, d, H, s), _gpu_run(N, d, H, s)
    what, bad, worst = f"k1 A {(N, d, H)} x{s:g}", [], {}
    wq, wp = K.pack_weights(inp["w_qkv"], inp["w_proj"])
    assert torch.equal(g["wqkv16"], wq) and torch.equal(g["wproj16"], wp)                # the pack itself is exact
    ref, f32 = ({}, {})
    for dt, o in ((F64, ref), (F32, f32)):
        o["qkv16"] = K.qkv_linear(inp["x"], g["wqkv16"], inp["b_qkv"], H, dt)
        o["lse"], o["attn16"] = K.core_fwd(g["qkv16"], H, dt)
        o["y"] = K.proj_linear(g["attn16"], g["wproj16"], inp["b_proj"], dt)
        l1 = K.bwd_launch1(inp["dy"], g["attn16"], g["wproj16"], H, dt)
        o["d_wproj"], o["d_bproj"] = l1["d_wproj"], l1["d_bproj"]
    for nm in ("qkv16", "attn16"):
        worst[nm] = _bf16_result(what, nm, g[nm], ref[nm], f32[nm], bad)
    for nm in ("lse", "y", "d_wproj", "d_bproj"):
        worst[nm] = _maxnorm(what, nm, g[nm], ref[nm], f32[nm], bad)
    print(f"ratio {what} WORST {max(worst.values()):.3f}")
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------ B
@gpu
@pytest.mark.parametrize("N,d,H,s", CASES, ids=IDS)
def test_backward_from_saved_state(ops, N, d, H, s):
    """B: dx, d_wqkv, d_bqkv from the kernel's own pack, qkv16, attn16, lse, and dy.  (ks_body<false, true> for d_wqkv; the
    <false, false> form is pinned to it bit for bit by test_bf16_x_equals_fp32_x.)  Worst ratios measured: see "Worst measured on an MI355X" in the module
    docstring"""
    inp, g = _inputs(N, d, H, s), _gpu_run(N, d, H, s)
    what, bad = f"k1 B {(N, d, H)} x{s:g}", []
    ref_all = K.backward(g, inp["x"], inp["dy"], H, F64, R.bf16_rt)
    ref_in = K.backward(g, inp["x"], inp["dy"], H, F64, R.ident)
    worst = max(_frob(what, nm, g[nm], ref_all[nm], ref_in[nm], bad) for nm in K.BWD_NAMES)
    print(f"ratio {what} WORST {worst:.3f}")
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------ exact checks
def _tie_weights(rows, cols, seed):
    """fp32 weights of which every fourth sits exactly on a bf16 tie (low half 0x8000), with even and odd kept mantissas"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(rows, cols, generator=g) * 2 - 1) / 8
    bits = w.view(torch.int32)
    bits[:, ::4] = (bits[:, ::4] & -65536) | 0x8000
    return w


@gpu
@pytest.mark.parametrize("d", [48, 128])                   # 48: the 32 x 32 tiles of the pack kernel are ragged in both directions
def test_pack_weights_bit_exact(ops, d):
    L, lib = _lib()
    w_qkv, w_proj = _tie_weights(3 * d, d, d), _tie_weights(d, d, d + 1)
    assert bool(((w_qkv.view(torch.int32) & 0xFFFF) == 0x8000).any())
    e_qkv, e_proj = w_qkv.bfloat16(), w_proj.bfloat16()                                  # torch-CPU: round to nearest even
    want = torch.cat([e_qkv.reshape(-1), e_proj.reshape(-1), e_qkv.T.reshape(-1), e_proj.T.reshape(-1)]).view(torch.int16)
    g_qkv, g_proj = w_qkv.cuda(), w_proj.cuda()
    full = _pack(g_qkv, g_proj, 1)
    assert torch.equal(full.view(torch.int16).cpu(), want)
    poisoned = torch.full((8 * d * d,), 0x7A5A, device="cuda", dtype=torch.int16)
    assert lib.moma_mha_pack_weights(_p(g_qkv), _p(g_proj), _p(poisoned), d, 0, _st()) == 0
    got = poisoned.cpu()
    assert torch.equal(got[:4 * d * d], want[:4 * d * d]) and bool((got[4 * d * d:] == 0x7A5A).all())


@gpu
@pytest.mark.parametrize("N,d,H", [(100, 128, 4), (8, 256, 2)])
def test_qpack_bit_exact(ops, N, d, H):
    """qpack = bf16(y * qpack_scale) of the kernel's own y in the unit layout of include/moma_hip.h; pad rows stay zero, bytes
    outside moma_infonce_qpack_bytes stay untouched"""
    L, lib = _lib()
    nbytes = lib.moma_infonce_qpack_bytes(N, d)
    bpad = nbytes // (2 * d)
    assert nbytes > 0 and bpad * 2 * d == nbytes and bpad % 32 == 0 and bpad >= N
    CAN = 256                                                                           # int16 elements of canary on each side
    buf = torch.full((2 * CAN + nbytes // 2,), 0x5A5A, device="cuda", dtype=torch.int16)
    buf[CAN:CAN + nbytes // 2] = 0
    qp = buf[CAN:CAN + nbytes // 2]
    assert qp.data_ptr() % 16 == 0
    scale = float(torch.tensor(1.0 / 0.15 * 1.4426950408889634, dtype=F32))
    mod = _module_for(_inputs(N, d, H, 1.0), H, qpack=qp, qscale=scale)
    assert _fwd([mod], N, d, H) == 0
    ypad = torch.zeros(bpad, d)
    ypad[:N] = mod.y.cpu()
    want = (ypad * torch.tensor(scale, dtype=F32)).bfloat16().view(bpad // 32, 32, d // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(-1)
    got = buf.cpu()
    assert torch.equal(got[CAN:CAN + nbytes // 2], want.contiguous().view(torch.int16))
    assert bool((got[:CAN] == 0x5A5A).all()) and bool((got[CAN + nbytes // 2:] == 0x5A5A).all())
    plain = _module_for(_inputs(N, d, H, 1.0), H)                                       # the qpack epilogue changes nothing else
    assert _fwd([plain], N, d, H) == 0
    assert all(torch.equal(a, b) for a, b in zip(mod.bits(), plain.bits()))


@gpu
@pytest.mark.parametrize("N,d,H", [(77, 192, 4), (37, 320, 2)])        # narrow and wide cores
def test_grouped_modules_equal_their_single_calls(ops, N, d, H):
    """n_modules = 2, 3, 4 over different x and weights: blockIdx picks the module in all three launches (core_block deals the
    workgroups in the XCD order when their number is a multiple of 8, in the plain order otherwise: both occur here)"""
    inps = [R.mha_inputs(N, d, H, seed=900 + i) for i in range(4)]
    single = []
    for inp in inps:
        m = _module_for(inp, H)
        assert _fwd([m], N, d, H) == 0
        single.append(m)
    for n in (2, 3, 4):
        group = [_module_for(inp, H) for inp in inps[:n]]
        assert _fwd(group, N, d, H) == 0
        for i in range(n):
            for a, b in zip(group[i].bits(), single[i].bits()):
                assert torch.equal(a, b), (n, i)
    assert not torch.equal(single[0].y, single[1].y)


@gpu
@pytest.mark.parametrize("N,d,H", [(77, 192, 4), (37, 320, 2)])
def test_forward_optional_arguments(ops, N, d, H):
    inp = _inputs(N, d, H, 1.0)
    base = _module_for(inp, H)
    assert _fwd([base], N, d, H) == 0
    no_lse = _module_for(inp, H, lse=False)                                             # lse = NULL: the same y bits
    assert _fwd([no_lse], N, d, H) == 0
    assert all(torch.equal(a, b) for a, b in zip(no_lse.bits(), base.bits()[:3]))
    zero = dict(inp, b_qkv=torch.zeros(3 * d))                                          # b_qkv = NULL equals a zero bias
    zb, nb = _module_for(zero, H), _module_for(zero, H)
    nb.b_qkv = None
    assert _fwd([zb], N, d, H) == 0 and _fwd([nb], N, d, H) == 0
    assert all(torch.equal(a, b) for a, b in zip(nb.bits(), zb.bits()))
    assert not torch.equal(zb.y, base.y)


@gpu
@pytest.mark.parametrize("N,d,H", [(77, 192, 4), (37, 320, 2)])
def test_bf16_x_equals_fp32_x(ops, N, d, H):
    """x_dtype = BF16 against the fp32 call on the same (bf16-representable) values: forward and backward bit for bit -- kc_body's
    DMA A operand against its converting loads, ks_body<false, false> against <false, true>"""
    inp = _inputs(N, d, H, 1.0)
    inp = dict(inp, x=R.bf16_rt(inp["x"]))
    dy = inp["dy"].cuda()
    m32, m16 = _module_for(inp, H), _module_for(inp, H, x_bf16=True)
    assert _fwd([m32], N, d, H) == 0 and _fwd([m16], N, d, H) == 0
    assert all(torch.equal(a, b) for a, b in zip(m16.bits(), m32.bits()))
    (rc32, o32), (rc16, o16) = _bwd(m32, dy, H), _bwd(m16, dy, H)
    assert rc32 == 0 and rc16 == 0
    for nm in BWD_OUT:
        assert torch.isfinite(o32[nm]).all() and torch.equal(o16[nm], o32[nm]), nm


@gpu
@pytest.mark.parametrize("N,d,H", [(77, 192, 4), (37, 320, 2)])
def test_backward_null_outputs_and_repeatability(ops, N, d, H):
    """each documented NULL combination leaves the other outputs bit-equal; the workspace is exactly
    moma_mha_bwd_fast_workspace_bytes and poisoned with 0xFF, the outputs start as NaN; two calls give the same bits"""
    inp = _inputs(N, d, H, 1.0)
    dy = inp["dy"].cuda()
    mod = _module_for(inp, H)
    assert _fwd([mod], N, d, H) == 0
    rc, full = _bwd(mod, dy, H)
    assert rc == 0 and all(torch.isfinite(full[nm]).all() for nm in BWD_OUT)
    rc, again = _bwd(mod, dy, H)
    assert rc == 0 and all(torch.equal(again[nm], full[nm]) for nm in BWD_OUT)
    for skip in (("dx",), ("dw_qkv", "db_qkv"), ("dw_proj", "db_proj"), ("db_qkv",), ("db_proj",),
                 ("dx", "dw_qkv", "db_qkv"), ("dx", "dw_qkv", "db_qkv", "dw_proj", "db_proj")):
        rc, part = _bwd(mod, dy, H, skip=skip)
        assert rc == 0, skip
        for nm in BWD_OUT:
            assert part[nm] is None if nm in skip else torch.equal(part[nm], full[nm]), (skip, nm)


@gpu
def test_argument_checks_return_before_any_launch(ops):
    """the MOMA_E_* codes of the entry points in api.hip; canaried outputs unchanged"""
    L, lib = _lib()
    E_SHAPE, E_ALIGN, E_WORKSPACE, E_UNSUPPORTED = -2, -4, -5, -6

    def canaried(N, d, H):
        inp = {nm: torch.zeros(s) for nm, s in dict(x=(N, d), w_qkv=(3 * d, d), b_qkv=(3 * d,), w_proj=(d, d), b_proj=(d,)).items()}
        g = {nm: t.cuda() for nm, t in inp.items()}
        mod = _Mod(g["x"], torch.zeros(8 * d * d + 8, device="cuda", dtype=torch.bfloat16), g["b_qkv"], g["b_proj"], H)
        for t in mod.bits():
            t.fill_(7)
        return mod

    def untouched(mod, out=None):
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in mod.bits())
        assert out is None or all(bool((t == 7.0).all()) for t in out.values() if t is not None)

    def refused_both(N, d, H, code):
        mod = canaried(N, d, H)
        assert _fwd([mod], N, d, H) == code
        rc, out = _bwd(mod, torch.zeros(N, d, device="cuda"), H, fill=7.0)
        assert rc == code
        untouched(mod, out)

    # hd % 16 != 0 (hd = 12): the staged path's configuration
    assert lib.moma_mha_saved_state(64, 96, 8, L.PREC_BF16) == L.MHA_SAVE_PROBS
    refused_both(64, 96, 8, E_UNSUPPORTED)
    # a wide head past its last N: mha_fast_supported takes hd > 128 up to N = 32 * 8 * 4 = 1024 (four key tiles per wave)
    assert lib.moma_mha_saved_state(1024, 288, 2, L.PREC_BF16) == L.MHA_SAVE_LSE
    assert lib.moma_mha_saved_state(1025, 288, 2, L.PREC_BF16) == L.MHA_SAVE_PROBS
    assert lib.moma_mha_saved_state(1025, 256, 2, L.PREC_BF16) == L.MHA_SAVE_LSE       # hd = 128: any N
    refused_both(1025, 288, 2, E_UNSUPPORTED)
    # the pack kernel takes d % 16 == 0 only
    w = torch.zeros(3 * 24, 24, device="cuda")
    pk = torch.full((8 * 24 * 24,), 7, device="cuda", dtype=torch.bfloat16)
    assert lib.moma_mha_pack_weights(_p(w), _p(w), _p(pk), 24, 1, _st()) == E_SHAPE
    N, d, H = 33, 128, 8
    mods = [canaried(N, d, H) for _ in range(5)]
    assert _fwd(mods[:1], N, d, H, n=0) == E_SHAPE and _fwd(mods, N, d, H, n=5) == E_SHAPE
    # a pack that starts inside a 16-byte piece
    mod = mods[0]
    whole = mod.pack
    mod.pack = whole[1:]
    assert _fwd([mod], N, d, H) == E_ALIGN
    mod.pack = whole
    assert lib.moma_mha_pack_weights(_p(w), _p(w), _p(pk, 2), 16, 1, _st()) == E_ALIGN
    dy = torch.zeros(N, d, device="cuda")
    rc, out = _bwd(mod, dy, H, fill=7.0, pack_off=2)
    assert rc == E_ALIGN
    untouched(mod, out)
    rc, out = _bwd(mod, dy, H, fill=7.0, ws_short=1)
    assert rc == E_WORKSPACE
    untouched(mod, out)
    rc, out = _bwd(mod, dy, H, fill=7.0, skip=("dw_qkv",))                               # a bias gradient without its weight gradient
    assert rc == E_UNSUPPORTED
    untouched(mod, out)
    for m in mods:
        untouched(m)
    assert bool((pk == 7).all())
