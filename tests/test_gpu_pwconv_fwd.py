"""moma_pwconv_fwd / moma_pwconv_bwd_data on the GPU -- forward and input gradient of the pointwise convolutions on the streaming
bf16 MFMA kernel (csrc/pwstream.hip) -- and their wiring (ops.pwconv, SamePadConv2d under MOMA_PWFWD).

Per shape of tests/pwfwd_ref.SHAPES and per direction:
  (a) integer data, asymmetric between the operands, every output an integer of magnitude <= 256: the result must equal the
      float64 product bit for bit;
  (b) random bf16 data against the float64 product of the same stored values: |got - ref| <= 2^-8 |ref| + K 2^-23 S, S = sum |w x|
      (twice the worst case of one bf16 rounding plus any-order fp32 accumulation of K exact products);
  (c) the stock F.conv2d / aten.convolution_backward is held to the same bound on the same data, and the native error is never more
      than twice the stock error wherever the stock error is above one bf16 ulp of the reference;
  (d) two calls give identical bits;
  (e) canaries in front of and behind the output are unchanged;
  (f) refused calls (fp32, an output that is not 2-byte aligned) write nothing.  Every shape class is implemented.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import pwfwd_ref as R

pytestmark = pytest.mark.gpu
GUARD = 4096
CANARY = 0xFF
CASES = [(s, t) for s in R.SHAPES for t in R.DIRECTIONS]


def _carve(nbytes):
    raw = torch.full((GUARD + nbytes + (-nbytes) % 256 + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    return raw, raw[GUARD:GUARD + nbytes]


def _intact(raw, nbytes):
    return bool((raw[:GUARD] == CANARY).all()) and bool((raw[GUARD + nbytes:] == CANARY).all())


def _call(a, w, shape, transposed, dtype=None, out_offset=0):
    """the raw entry point on a guarded output -> (rc, result bf16, canaries intact, output bytes untouched)"""
    from moma_amd import _lib, ops
    lib = _lib.load()
    N, Cin, Cout, H, W = shape
    Co = Cin if transposed else Cout
    nbytes = N * Co * H * W * 2
    raw, out = _carve(nbytes + 16)
    fn = lib.moma_pwconv_bwd_data if transposed else lib.moma_pwconv_fwd
    rc = fn(ops._ptr(a), ops._ptr(w), C.c_void_p(out.data_ptr() + out_offset), N, Cin, Cout, H * W,
            ops.DT_BF16 if dtype is None else dtype, ops._stream())
    torch.cuda.synchronize()
    ok = _intact(raw, nbytes + 16) and bool((out[nbytes:] == CANARY).all())
    untouched = bool((out == CANARY).all())
    return rc, out[:nbytes].view(torch.bfloat16).view(N, Co, H, W).clone(), ok, untouched


def _stock(a, w4, shape, transposed):
    N, Cin, Cout, H, W = shape
    if not transposed:
        return F.conv2d(a, w4)
    x = torch.zeros(N, Cin, H, W, dtype=torch.bfloat16, device="cuda")
    return torch.ops.aten.convolution_backward(a, x, w4, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [True, False, False])[0]


@pytest.mark.parametrize("shape,transposed", CASES)
def test_exact_data_bit_for_bit(shape, transposed):
    a, w = R.exact_data(shape, transposed)
    exact = R.product_f64(a, w, transposed).float().bfloat16()
    ag, wg = a.bfloat16().cuda(), w.bfloat16().cuda()
    rc, y, ok, _ = _call(ag, wg, shape, transposed)
    assert rc == 0 and ok
    assert torch.equal(y.cpu().view(torch.int16), exact.view(torch.int16)), (y.cpu().float() - exact.float()).abs().max()
    rc, again, ok, _ = _call(ag, wg, shape, transposed)
    assert rc == 0 and ok and torch.equal(again.view(torch.int16), y.view(torch.int16))


_RANDOM = {}


def _random_case(shape, transposed):
    """native and stock results on the random data of one case, their errors against float64 and the bound: computed once"""
    key = (shape, transposed)
    if key not in _RANDOM:
        N, Cin, Cout, H, W = shape
        a, w = R.random_data(shape, transposed)
        ref, S = R.product_f64(a, w, transposed), R.product_abs_f64(a, w, transposed)
        lim = R.bound(ref, S, R.depth(shape, transposed))
        ag, wg = a.cuda(), w.cuda()
        rc, y, ok, _ = _call(ag, wg, shape, transposed)
        rc2, again, ok2, _ = _call(ag, wg, shape, transposed)
        stock = _stock(ag, wg.view(Cout, Cin, 1, 1), shape, transposed)
        err, stock_err = (y.cpu().double() - ref).abs(), (stock.cpu().double() - ref).abs()
        print(f"{shape} transposed={transposed}: native max err / bound = {float((err / lim).max()):.3f}, "
              f"stock = {float((stock_err / lim).max()):.3f}")
        _RANDOM[key] = dict(rc=(rc, rc2), ok=ok and ok2, same=torch.equal(again.view(torch.int16), y.view(torch.int16)), ref=ref,
                            lim=lim, err=err, stock_err=stock_err)
    return _RANDOM[key]


@pytest.mark.parametrize("shape,transposed", CASES)
def test_random_data_against_float64(shape, transposed):
    r = _random_case(shape, transposed)
    assert r["rc"] == (0, 0) and r["ok"] and r["same"]
    assert bool((r["err"] <= r["lim"]).all()), float((r["err"] / r["lim"]).max())


@pytest.mark.parametrize("shape,transposed", CASES)
def test_native_error_is_within_twice_the_stock_error(shape, transposed):
    r = _random_case(shape, transposed)
    above = r["stock_err"] > R.bf16_ulp(r["ref"])
    assert bool((r["err"][above] <= 2 * r["stock_err"][above]).all())


@pytest.mark.parametrize("shape,transposed", CASES)
def test_stock_meets_the_same_bound(shape, transposed):
    """MIOpen / ATen held to the bound the kernel is held to.  Whether it holds depends on the solver MIOpen picks in the process
    at hand (MI355X, ROCm 7.2): inside a run of the whole GPU suite all sixteen cases have passed every time (three runs); in a
    process that runs this file alone seven or eight of them, all with few output channels or tiny planes, come out truncated
    instead of rounded to nearest (error / bound 1.48 .. 1.98, mean signed error -2.8e-3 of the value, half of the elements differ
    from the kernel's).  The kernel is at 0.81 .. 0.995 in all sixteen in every run.  Recorded figures: profiles/pwfwd_rounding_vs_float64.txt.  The bound
    is the one the kernel's contract sets and is not widened for the stock path."""
    r = _random_case(shape, transposed)
    assert bool((r["stock_err"] <= r["lim"]).all()), float((r["stock_err"] / r["lim"]).max())


@pytest.mark.parametrize("transposed", R.DIRECTIONS)
def test_refused_calls_write_nothing(transposed):
    from moma_amd import ops
    shape = (3, 16, 96, 8, 8)
    a, w = R.exact_data(shape, transposed)
    a, w = a.bfloat16().cuda(), w.bfloat16().cuda()
    for kw, code in ((dict(dtype=ops.DT_F32), -3), (dict(dtype=7), -3), (dict(out_offset=1), -4)):
        rc, _, ok, untouched = _call(a, w, shape, transposed, **kw)
        assert rc == code and ok and untouched, kw               # MOMA_E_DTYPE: fp32 keeps the stock path; MOMA_E_ALIGN


def test_views_channels_last_and_offset_give_the_dense_result():
    from moma_amd import ops
    shape = (2, 24, 144, 14, 14)
    assert ops.pwconv_fwd_native(*shape[:3], 196)
    N, Cin, Cout, H, W = shape
    x, w = R.random_data(shape, False)
    dy, _ = R.random_data(shape, True)
    w4 = w.cuda().view(Cout, Cin, 1, 1)
    xd = x.cuda().requires_grad_(True)
    yd = ops.pwconv(xd, w4.clone().requires_grad_(True))
    yd.backward(dy.cuda())
    big = torch.zeros(x.numel() + 8, dtype=torch.bfloat16, device="cuda")
    x_off = big[1:1 + x.numel()].view(x.shape)                                            # starts 2 bytes into the buffer
    x_off.copy_(x)
    assert x_off.data_ptr() % 4 == 2 and x_off.is_contiguous()
    x_off.requires_grad_(True)
    y = ops.pwconv(x_off, w4.clone().requires_grad_(True))
    dy_cl = dy.cuda().contiguous(memory_format=torch.channels_last)                      # NCHW shape, NHWC memory
    assert not dy_cl.is_contiguous()
    y.backward(dy_cl)
    assert torch.equal(y.view(torch.int16), yd.view(torch.int16))
    assert torch.equal(x_off.grad.view(torch.int16), xd.grad.view(torch.int16))
    x_cl = x.cuda().contiguous(memory_format=torch.channels_last)
    assert torch.equal(ops.pwconv_fwd(x_cl, w4).view(torch.int16), yd.view(torch.int16))
    ref = R.product_f64(x, w, False)
    assert bool(((yd.detach().cpu().double() - ref).abs() <= R.bound(ref, R.product_abs_f64(x, w, False), Cin)).all())


def test_graph_capture_replays_equal_eager():
    from moma_amd import ops
    shape = (2, 24, 144, 14, 14)
    assert ops.pwconv_fwd_native(*shape[:3], 196)
    N, Cin, Cout, H, W = shape
    w = R.random_data(shape, False)[1].cuda().view(Cout, Cin, 1, 1).requires_grad_(True)
    sx = torch.zeros(N, Cin, H, W, dtype=torch.bfloat16, device="cuda").requires_grad_(True)
    sdy = torch.zeros(N, Cout, H, W, dtype=torch.bfloat16, device="cuda")

    def step(x, dy):
        x.grad = w.grad = None
        y = ops.pwconv(x, w)
        y.backward(dy)
        return y.detach(), x.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sdy)                                             # warm-up outside the capture (library load)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gdx = step(sx, sdy)
    for seed in (1, 2):
        x = R.random_data(shape, False, seed)[0]
        dy = R.random_data(shape, True, seed)[0]
        with torch.no_grad():
            sx.copy_(x.cuda())
            sdy.copy_(dy.cuda())
        graph.replay()
        torch.cuda.synchronize()
        got_y, got_dx = gy.clone(), gdx.clone()
        ey, edx = step(x.cuda().requires_grad_(True), dy.cuda())
        assert torch.equal(got_y.view(torch.int16), ey.view(torch.int16))
        assert torch.equal(got_dx.view(torch.int16), edx.view(torch.int16))


def _count_native(monkeypatch):
    """counts the calls that reach the streaming kernel's two wrappers"""
    from moma_amd import ops
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = ops.pwconv_fwd, ops.pwconv_bwd_data
    monkeypatch.setattr(ops, "pwconv_fwd", lambda *a: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a))[1])
    monkeypatch.setattr(ops, "pwconv_bwd_data", lambda *a: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a))[1])
    return calls


# (kernel, stride, expand, cin, cout, se), batch: the block of tests/test_gpu_pwconv.py at its small size, and a stage-4 repeat
# block of EfficientNet-B0 as the benchmark runs it (80 -> 480 -> 80 on 14 x 14 planes at batch 256: two layers of the layer table)
BLOCKS = {"small": ((3, 1, 6, 16, 16, 0.25), 4, {"fwd": 1, "bwd": 1}),      # (the 96 -> 16 projection keeps MIOpen: 16 output channels)
          "bench": ((3, 1, 6, 80, 80, 0.25), 256, {"fwd": 2, "bwd": 2})}


def _block_run(flag, case, monkeypatch):
    from moma_amd.backbones import efficientnet as E
    cfg, batch, _ = BLOCKS[case]
    monkeypatch.setattr(E, "_PW_MODE", "hip")
    monkeypatch.setattr(E, "_PW_FWD", flag)
    calls = _count_native(monkeypatch)
    torch.manual_seed(11)
    blk = E.MBConvBlock(*cfg).cuda().train()
    convs = [m for m in blk.modules() if isinstance(m, E.SamePadConv2d) and m.groups == 1]
    g = torch.Generator().manual_seed(12)
    x = torch.randn(batch, cfg[3], 14, 14, generator=g).cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for m in convs:                                           # the weight cache, live as inside a model forward
            m._wc = m.weight.detach().bfloat16()
            m._bc = m.bias.detach().bfloat16() if m.bias is not None else None
            m._wc_live = True
        y = blk(x)
        for m in convs:
            m._wc_live = False
    y.float().square().mean().backward()
    out = {"y": y.detach().float().cpu(), "dx": x.grad.detach().float().cpu()}
    out.update({n: p.grad.detach().float().cpu() for n, p in blk.named_parameters()})
    return out, calls


@pytest.mark.parametrize("case", list(BLOCKS))
def test_mbconv_block_agrees_with_the_switch_on_and_off(case, monkeypatch):
    """the forward within 2^-7 of the largest value; the gradients are printed and must be finite (they have no bound of their own
    here: tests/test_gpu_pwconv.py holds the parameter gradients of the small block to 2^-7 between MOMA_PW=hip and miopen)"""
    on, calls = _block_run("1", case, monkeypatch)
    assert calls == BLOCKS[case][2]                               # the squeeze-excite pair keeps the stock path
    off, calls = _block_run("0", case, monkeypatch)
    assert calls == {"fwd": 0, "bwd": 0}
    assert on.keys() == off.keys() and len(on) >= 14
    for n in on:
        scale = float(off[n].abs().max())
        diff = float((on[n] - off[n]).abs().max())
        print(f"{case} {n}: max |diff| / max |value| = {diff / max(scale, 1e-30):.2e}")
        assert bool(torch.isfinite(on[n]).all()), n
    assert float((on["y"] - off["y"]).abs().max()) <= 2.0 ** -7 * float(off["y"].abs().max())


# batch, image size, routed layers: at 64 x 64 every plane (32^2 .. 2^2) has rows of 4 k pixels, so all 32 bias-free pointwise
# convolutions but 32 -> 16 go to the kernel; at the benchmark's shapes the 7 x 7 planes keep MIOpen
MODELS = {"small": (4, 64, 31), "bench": (256, 224, 21)}


def _model_run(flag, case, monkeypatch):
    from moma_amd.backbones import efficientnet as E
    batch, size, _ = MODELS[case]
    monkeypatch.setattr(E, "_PW_MODE", "hip")
    monkeypatch.setattr(E, "_PW_FWD", flag)
    calls = _count_native(monkeypatch)
    torch.manual_seed(31)
    model = E.efficientnet_b0(num_classes=10).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(32)
    x = torch.randn(batch, 3, size, size, generator=g, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):   # a forward that records no gradient: the teacher's pass
        feats, logits = model(x, is_feat=True)
    return [f.float().cpu() for f in feats[-3:]] + [logits.float().cpu()], calls


@pytest.mark.parametrize("case", list(MODELS))
def test_efficientnet_b0_forward_agrees_with_the_switch_on_and_off(case, monkeypatch):
    """The whole backbone, one no-grad forward per setting: the last three features and the logits within 2^-7 of the largest
    value.  `bench` (the benchmark's shapes) has agreed bit for bit in every run so far.  `small` depends on which solver
    MIOpen picks for the switch-off side in that process: inside a run of the whole GPU suite it has passed every time; in a
    process that runs this file alone MIOpen truncates the bf16 result of 14 of the 32 layers instead of rounding it
    (profiles/pwfwd_rounding_vs_float64.txt: layer by layer on this very input, the kernel and MIOpen against float64; the other
    18 layers agree with the kernel bit for bit), and max |on - off| / max |off| comes to 0.75e-2 .. 1.5e-2 against the 7.8e-3
    asked here.  The bound stands as the issue states it."""
    on, calls = _model_run("1", case, monkeypatch)
    assert calls == {"fwd": MODELS[case][2], "bwd": 0}
    off, calls = _model_run("0", case, monkeypatch)
    assert calls == {"fwd": 0, "bwd": 0}
    assert len(on) == len(off) == 4
    for i, (a, b) in enumerate(zip(on, off)):
        scale = float(b.abs().max())
        diff = float((a - b).abs().max())
        print(f"{case} output {i} {tuple(b.shape)}: max |diff| / max |value| = {diff / max(scale, 1e-30):.2e}")
        assert diff <= 2.0 ** -7 * scale, i
