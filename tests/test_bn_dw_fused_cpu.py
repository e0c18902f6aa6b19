"""CPU-side contract of the fused BN0 + SiLU -> depthwise path: the op refuses CPU tensors like its neighbours (there is no
CPU fallback inside moma_amd.ops), and the backbone never reaches for it off the GPU."""
import pytest
import torch


@pytest.fixture(scope="module")
def lib_path():
    from moma_amd import build
    return build.build(verbose=False)


def _cpu_args():
    C = 4
    return (torch.zeros(2, C, 8, 8), torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C), True, 0.1, 1e-3, "silu",
            torch.zeros(C, 1, 3, 3), 1, 1, 1, 8, 8)


def test_bn_act_dwconv_refuses_cpu_tensors(lib_path):
    from moma_amd import _lib, ops
    with pytest.raises(_lib.MomaHipError):
        ops.bn_act_dwconv(*_cpu_args())
    with pytest.raises(_lib.MomaHipError):                      # ... as the two ops it stands for do
        ops.bn_act(*_cpu_args()[:9])
    with pytest.raises(_lib.MomaHipError):
        ops.dwconv(torch.zeros(2, 4, 8, 8), torch.zeros(4, 1, 3, 3), 1, 1, 1, 8, 8)


def test_block_on_the_cpu_does_not_take_the_fused_path(monkeypatch):
    from moma_amd import ops
    from moma_amd.backbones import efficientnet as E

    def boom(*a, **k):
        raise AssertionError("the fused op was called for a CPU tensor")
    monkeypatch.setattr(ops, "bn_act_dwconv", boom)
    torch.manual_seed(0)
    blk = E.MBConvBlock(5, 2, 6, 8, 12, 0.25).eval()
    x = torch.randn(2, 8, 18, 18)
    outs = []
    for fuse in ("grad", "1", "0"):
        monkeypatch.setattr(E, "_BNDW_FUSE", fuse)
        with torch.no_grad():
            outs.append(blk(x))
    assert outs[0].shape == (2, 12, 9, 9) and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_same_padding_helper():
    from moma_amd.backbones.efficientnet import _same_pad
    assert _same_pad(112, 112, 3, 3, 2, 2) == (1, 1)            # asymmetric: 0 on top, 1 below
    assert _same_pad(56, 56, 5, 5, 2, 2) == (3, 3)
    assert _same_pad(14, 14, 5, 5, 1, 1) == (4, 4)
    assert _same_pad(7, 9, 1, 1, 1, 1) == (0, 0)
