"""moma_pwconv_bwd_weight on the GPU -- the weight gradient of the pointwise convolutions on the split-K bf16 MFMA kernel
(csrc/pwconv.hip) -- and its wiring (ops.pwconv, SamePadConv2d under MOMA_PW).

Per shape of tests/pw_ref.SHAPES:
  (a) integer data, asymmetric between the operands: every sum is exact in fp32, dw must equal exact.to(bfloat16) bit for bit;
  (b) random bf16 data against the float64 sum of the same inputs: |got - ref| <= 2^-8 |ref| + L 2^-23 S, L = N HW,
      S = sum |dy x| per output (products of two bf16 are exact in fp32; any-order fp32 accumulation errs by at most L 2^-24 S; the
      one bf16 rounding by 2^-9 |ref|; the bound is twice that worst case);
  (c) two calls give identical bits;
  (d) canaries in front of and behind dw and the workspace are unchanged.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import pw_ref as R

pytestmark = pytest.mark.gpu
GUARD = 4096
CANARY = 0xFF


def _carve(nbytes):
    raw = torch.full((GUARD + nbytes + (-nbytes) % 256 + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    return raw, raw[GUARD:GUARD + nbytes]


def _intact(raw, nbytes):
    return bool((raw[:GUARD] == CANARY).all()) and bool((raw[GUARD + nbytes:] == CANARY).all())


def _call(x, dy, ws_bytes=None, ws_offset=0, dtype=None):
    """the raw entry point on guarded dw / workspace -> (rc, dw [Cout, Cin] bf16, canaries intact)"""
    from moma_amd import _lib, ops
    lib = _lib.load()
    N, Cin, H, W = x.shape
    Cout = dy.shape[1]
    need = lib.moma_pwconv_workspace_bytes(N, Cin, Cout, H * W)
    assert need > 0 and need % 256 == 0
    n_ws = need if ws_bytes is None else ws_bytes
    raw_dw, dw = _carve(Cout * Cin * 2)
    raw_ws, ws = _carve(n_ws + 16)
    rc = lib.moma_pwconv_bwd_weight(ops._ptr(x), ops._ptr(dy), ops._ptr(dw), C.c_void_p(ws.data_ptr() + ws_offset), n_ws, N, Cin,
                                    Cout, H * W, ops.DT_BF16 if dtype is None else dtype, ops._stream())
    torch.cuda.synchronize()
    ok = _intact(raw_dw, Cout * Cin * 2) and _intact(raw_ws, n_ws + 16)
    return rc, dw.view(torch.bfloat16).view(Cout, Cin).clone(), ok


@pytest.mark.parametrize("shape", R.SHAPES)
def test_exact_data_bit_for_bit(shape):
    x, dy = R.exact_data(shape)
    exact = R.wgrad_f64(x, dy).float().bfloat16()
    rc, dw, ok = _call(x.bfloat16().cuda(), dy.bfloat16().cuda())
    assert rc == 0 and ok
    assert torch.equal(dw.cpu().view(torch.int16), exact.view(torch.int16)), (dw.cpu().float() - exact.float()).abs().max()
    rc, again, ok = _call(x.bfloat16().cuda(), dy.bfloat16().cuda())
    assert rc == 0 and ok and torch.equal(again.view(torch.int16), dw.view(torch.int16))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_random_data_against_float64(shape):
    N, Cin, Cout, H, W = shape
    x, dy = R.random_data(shape)
    ref, S = R.wgrad_f64(x, dy), R.wgrad_abs_f64(x, dy)
    xg, dyg = x.cuda(), dy.cuda()
    rc, dw, ok = _call(xg, dyg)
    assert rc == 0 and ok
    err, lim = (dw.cpu().double() - ref).abs(), R.bound(ref, S, N * H * W)
    print(f"{shape}: max err / bound = {float((err / lim).max()):.3f}")
    assert bool((err <= lim).all()), float((err / lim).max())
    rc, again, ok = _call(xg, dyg)
    assert rc == 0 and ok and torch.equal(again.view(torch.int16), dw.view(torch.int16))


def test_views_channels_last_dy_and_offset_x():
    from moma_amd import ops
    shape = (3, 16, 96, 8, 8)
    x, dy = R.exact_data(shape)
    exact = R.wgrad_f64(x, dy).float().bfloat16()
    dy_cl = dy.bfloat16().cuda().contiguous(memory_format=torch.channels_last)          # NCHW shape, NHWC memory
    assert not dy_cl.is_contiguous()
    big = torch.zeros(x.numel() + 8, dtype=torch.bfloat16, device="cuda")
    x_off = big[1:1 + x.numel()].view(x.shape)                                            # starts 2 bytes into the buffer
    x_off.copy_(x)
    assert x_off.data_ptr() % 4 == 2 and x_off.is_contiguous()
    dw = ops.pwconv_bwd_weight(x_off, dy_cl)
    assert dw.shape == (96, 16, 1, 1)
    assert torch.equal(dw.cpu().view(96, 16).view(torch.int16), exact.view(torch.int16))


def test_error_codes():
    from moma_amd import _lib, ops
    shape = (3, 16, 96, 8, 8)
    x, dy = R.exact_data(shape)
    x, dy = x.bfloat16().cuda(), dy.bfloat16().cuda()
    need = _lib.load().moma_pwconv_workspace_bytes(3, 16, 96, 64)
    assert _call(x, dy, dtype=ops.DT_F32)[0] == -3                # MOMA_E_DTYPE: fp32 keeps the stock path
    assert _call(x, dy, dtype=7)[0] == -3
    assert _call(x, dy, ws_bytes=need - 256)[0] == -5             # MOMA_E_WORKSPACE
    assert _call(x, dy, ws_offset=4)[0] == -4                     # MOMA_E_ALIGN
    for rc, _, ok in (_call(x, dy, dtype=ops.DT_F32), _call(x, dy, ws_bytes=need - 256), _call(x, dy, ws_offset=4)):
        assert ok                                                 # a refused call writes nothing


def _stock_backward(x, w, dy, mask):
    return torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, mask)


def test_op_input_gradient_is_the_stock_one_and_weight_gradient_is_the_kernels():
    from moma_amd import ops
    shape = (3, 24, 40, 14, 14)
    N, Cin, Cout, H, W = shape
    x, dy = R.random_data(shape)
    x, dy = x.cuda().requires_grad_(True), dy.cuda()
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) * 0.2).bfloat16().cuda().requires_grad_(True)
    b = torch.randn(Cout, generator=g).bfloat16().cuda().requires_grad_(True)
    y = ops.pwconv(x, w, b)
    assert torch.equal(y, F.conv2d(x.detach(), w.detach(), b.detach()))
    y.backward(dy)
    dx_stock = _stock_backward(x.detach(), w.detach(), dy, [True, False, False])[0]
    assert torch.equal(x.grad.view(torch.int16), dx_stock.view(torch.int16))
    rc, dw, ok = _call(x.detach(), dy)
    assert rc == 0 and torch.equal(w.grad.view(Cout, Cin).view(torch.int16), dw.view(torch.int16))
    assert torch.equal(b.grad, dy.sum((0, 2, 3)))


def _block_grads(mode, monkeypatch):
    from moma_amd.backbones import efficientnet as E
    monkeypatch.setattr(E, "_PW_MODE", mode)
    torch.manual_seed(11)
    blk = E.MBConvBlock(3, 1, 6, 16, 16, 0.25).cuda().train()
    convs = [m for m in blk.modules() if isinstance(m, E.SamePadConv2d) and m.groups == 1]
    g = torch.Generator().manual_seed(12)
    x = torch.randn(4, 16, 14, 14, generator=g).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for m in convs:                                           # the weight cache, live as inside a model forward
            m._wc = m.weight.detach().bfloat16()
            m._bc = m.bias.detach().bfloat16() if m.bias is not None else None
            m._wc_live = True
        assert all(m._takes_pwconv(True, torch.bfloat16) == (mode == "hip") for m in convs)
        y = blk(x)
        for m in convs:
            m._wc_live = False
    y.float().square().mean().backward()
    return {n: p.grad.detach().float().cpu() for n, p in blk.named_parameters()}


def test_mbconv_block_gradients_agree_between_hip_and_miopen(monkeypatch):
    hip = _block_grads("hip", monkeypatch)
    stock = _block_grads("miopen", monkeypatch)
    assert hip.keys() == stock.keys() and len(hip) >= 12
    for n in hip:
        scale = float(stock[n].abs().max())
        diff = float((hip[n] - stock[n]).abs().max())
        print(f"{n}: max |diff| / max |grad| = {diff / max(scale, 1e-30):.2e}")
        assert diff <= 2.0 ** -7 * scale, n


def test_graph_capture_replays_equal_eager():
    from moma_amd import ops
    shape = (3, 24, 40, 14, 14)
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(21)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) * 0.2).bfloat16().cuda().requires_grad_(True)
    sx = torch.zeros(N, Cin, H, W, dtype=torch.bfloat16, device="cuda").requires_grad_(True)
    sdy = torch.zeros(N, Cout, H, W, dtype=torch.bfloat16, device="cuda")

    def step(x, dy):
        x.grad = w.grad = None
        ops.pwconv(x, w).backward(dy)
        return x.grad, w.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sdy)                                             # warm-up outside the capture (library load, MIOpen's find)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gdx, gdw = step(sx, sdy)
    for seed in (1, 2):
        x, dy = R.random_data(shape, seed)
        with torch.no_grad():
            sx.copy_(x.cuda())
            sdy.copy_(dy.cuda())
        graph.replay()
        torch.cuda.synchronize()
        got_dx, got_dw = gdx.clone(), gdw.clone()
        ex = x.cuda().requires_grad_(True)
        edx, edw = step(ex, dy.cuda())
        assert torch.equal(got_dx.view(torch.int16), edx.view(torch.int16))
        assert torch.equal(got_dw.view(torch.int16), edw.view(torch.int16))
