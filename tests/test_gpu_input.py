"""ops.input_batch (csrc/input.hip) against the restatement of tests/input_ref.py on the fixture of tests/input_cases.py: window mode bit
for bit in both dtypes and layouts, bilinear mode by its level rule, writes inside the destination, and both trainers on a pack.

Bilinear rule: the level equals floor(v + 0.5) of the float64 restatement, except where that value lies within 1e-4 of a half-integer
without being one (there +-1 level is allowed; at most 1 % of a case's values, asserted on the CPU in test_input_cpu.py too).  The
kernel keeps the tap weights as integers and rounds a value <= 255 five times in float32: at most 5 * 2^-24 * 255 = 7.6e-5."""
import os

import numpy as np
import pytest
import torch

from tests import input_cases as CASES, input_ref as R

pytestmark = pytest.mark.gpu
GUARD, CANARY = 4096, 0xFF
FORMATS = [(torch.float32, False), (torch.float32, True), (torch.bfloat16, False), (torch.bfloat16, True)]
FORMAT_IDS = ["fp32-nchw", "fp32-nhwc", "bf16-nchw", "bf16-nhwc"]


@pytest.fixture(scope="module")
def fx():
    from moma_amd import ops
    dev = torch.device("cuda", 0)
    src = CASES.source()
    return {"dev": dev, "src": src, "dsrc": src.to(dev), "lut": ops.input_lut(R.MEAN, R.STD, dev),
            "idx": torch.tensor(CASES.IDX, device=dev), "flip": torch.tensor(CASES.FLIP, dtype=torch.uint8, device=dev)}


def _same(x, ref, channels_last):
    x = x.cpu()
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    return x.dtype == ref.dtype and x.shape == ref.shape and x.is_contiguous(memory_format=fmt) and x.stride() == ref.stride() and \
        torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32), ref.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("case", list(CASES.WINDOW_CASES))
def test_window_mode_is_bit_equal(fx, case, fmt):
    from moma_amd import ops
    dtype, cl = fmt
    Sh, Sw, boxes = CASES.WINDOW_CASES[case]
    box = None if boxes is None else torch.tensor(boxes, dtype=torch.int32, device=fx["dev"])
    ref = R.input_batch(fx["src"], None, (Sh, Sw), idx=CASES.IDX, flip=CASES.FLIP, box=boxes, dtype=dtype, channels_last=cl)
    x = ops.input_batch(fx["dsrc"], fx["lut"], (Sh, Sw), idx=fx["idx"], flip=fx["flip"], box=box, dtype=dtype, channels_last=cl)
    assert _same(x, ref, cl)
    if boxes is None:                                                             # box = NULL is the centred box
        top, left = R.centre_box(CASES.H, CASES.W, Sh, Sw)
        cb = torch.tensor([[top, left, Sh, Sw]] * 5, dtype=torch.int32, device=fx["dev"])
        assert torch.equal(x, ops.input_batch(fx["dsrc"], fx["lut"], (Sh, Sw), idx=fx["idx"], flip=fx["flip"], box=cb, dtype=dtype, channels_last=cl))
        # a NULL box with resample = 1 is that window too
        assert torch.equal(x, ops.input_batch(fx["dsrc"], fx["lut"], (Sh, Sw), idx=fx["idx"], flip=fx["flip"], resample=True, dtype=dtype, channels_last=cl))


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_null_operands_are_their_defaults(fx, fmt):
    from moma_amd import ops
    dtype, cl = fmt
    dev = fx["dev"]
    kw = dict(dtype=dtype, channels_last=cl)
    box = torch.tensor(CASES.WINDOW_CASES["13x13"][2], dtype=torch.int32, device=dev)
    a = ops.input_batch(fx["dsrc"], fx["lut"], 13, box=box, flip=fx["flip"], **kw)                     # idx = NULL: rows 0 .. 4
    assert torch.equal(a, ops.input_batch(fx["dsrc"], fx["lut"], 13, idx=torch.arange(5, device=dev), box=box, flip=fx["flip"], **kw))
    assert _same(a, R.input_batch(fx["src"], None, 13, idx=list(range(5)), flip=CASES.FLIP, box=box.cpu(), **kw), cl)
    b = ops.input_batch(fx["dsrc"], fx["lut"], 13, idx=fx["idx"], box=box, **kw)                       # flip = NULL: none
    assert torch.equal(b, ops.input_batch(fx["dsrc"], fx["lut"], 13, idx=fx["idx"], box=box, flip=torch.zeros(5, dtype=torch.uint8, device=dev), **kw))
    assert _same(b, R.input_batch(fx["src"], None, 13, idx=CASES.IDX, box=box.cpu(), **kw), cl)
    c = ops.input_batch(fx["dsrc"], fx["lut"], (20, 28), batch=7, **kw)                                  # everything NULL: the whole split
    assert _same(c, R.input_batch(fx["src"], None, (20, 28), **kw), cl)
    # a box that leaves the image reads the clamped pixel, never another sample
    out_of = torch.tensor([[-3, -2, 16, 16], [9, 20, 16, 16], [0, 0, 16, 16], [30, 40, 16, 16], [-20, 5, 16, 16]], dtype=torch.int32, device=dev)
    d = ops.input_batch(fx["dsrc"], fx["lut"], 16, idx=fx["idx"], box=out_of, flip=fx["flip"], **kw)
    assert _same(d, R.input_batch(fx["src"], None, 16, idx=CASES.IDX, box=out_of.cpu(), flip=CASES.FLIP, **kw), cl)


def _mask_like_output(mask, flip):
    """a [B, S, S, 3] mask carried to the output's [B, 3, S, S] positions"""
    f = torch.as_tensor(flip).bool()
    return torch.where(f[:, None, None, None], mask.flip(2), mask).permute(0, 3, 1, 2)


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("case", list(CASES.BILINEAR_CASES))
def test_bilinear_mode_meets_the_level_rule(fx, case, fmt):
    from moma_amd import ops
    dtype, cl = fmt
    S, boxes, dyadic = CASES.BILINEAR_CASES[case]
    values = R.bilinear_values(fx["src"], torch.tensor(CASES.IDX), torch.tensor(boxes), S, S)
    exempt = R.near_tie(values, CASES.TIE_EPS)
    levels = R.to_levels(values)
    ref = R.finish(levels, CASES.FLIP, dtype, cl)
    lower = R.finish((levels.int() - 1).clamp(0, 255).to(torch.uint8), CASES.FLIP, dtype, cl)
    upper = R.finish((levels.int() + 1).clamp(0, 255).to(torch.uint8), CASES.FLIP, dtype, cl)
    x = ops.input_batch(fx["dsrc"], fx["lut"], S, idx=fx["idx"], flip=fx["flip"], box=torch.tensor(boxes, dtype=torch.int32, device=fx["dev"]),
                        resample=True, dtype=dtype, channels_last=cl)
    assert x.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    x = x.cpu()
    hit = x == ref
    ex = _mask_like_output(exempt, CASES.FLIP)
    share = float(exempt.double().mean())
    print(f"{case}: {int((~hit).sum())} of {hit.numel()} values off the float64 level, near-tie share {share:.4%}")
    assert share <= CASES.TIE_SHARE
    assert bool((hit | (ex & ((x == lower) | (x == upper)))).all())
    if dyadic:
        assert not bool(exempt.any()) and bool(hit.all())                         # exact arithmetic: everywhere, ties included


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("resample", [False, True], ids=["window", "bilinear"])
def test_writes_stay_inside_the_destination_and_reads_inside_the_source(fx, fmt, resample):
    """`out` lies in a buffer of 0xFF bytes (NaN in both dtypes), one element off a 16-byte boundary, with canaries on both sides; src
    is the tail of its allocation at an odd address, and the batch takes the last row of the last sample"""
    from moma_amd import ops
    dtype, cl = fmt
    dev = fx["dev"]
    es = 2 if dtype == torch.bfloat16 else 4
    raw_src = torch.empty(5 + fx["src"].numel(), dtype=torch.uint8, device=dev)
    src = raw_src[5:].view(fx["src"].shape)
    src.copy_(fx["dsrc"])
    if resample:
        S, boxes = (17, 17), torch.tensor(CASES.BILINEAR_CASES["general onto 17"][1], dtype=torch.int32, device=dev)
    else:
        S, boxes = (13, 28), torch.tensor([[7, 0, 13, 28], [0, 0, 13, 28], [7, 0, 13, 28], [3, 0, 13, 28], [5, 0, 13, 28]], dtype=torch.int32, device=dev)
    B, nbytes = 5, 5 * 3 * S[0] * S[1] * es
    raw = torch.full((GUARD + es + nbytes + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    out = raw[GUARD + es:GUARD + es + nbytes].view(dtype)
    out = out.view(B, S[0], S[1], 3).permute(0, 3, 1, 2) if cl else out.view(B, 3, S[0], S[1])
    kw = dict(idx=fx["idx"], flip=fx["flip"], box=boxes, resample=resample, dtype=dtype, channels_last=cl)
    ops.input_batch(src, fx["lut"], S, out=out, **kw)
    torch.cuda.synchronize()
    assert bool((raw[:GUARD + es] == CANARY).all()) and bool((raw[GUARD + es + nbytes:] == CANARY).all())
    assert not bool(torch.isnan(out.float()).any())
    plain = ops.input_batch(fx["dsrc"], fx["lut"], S, **kw)
    assert torch.equal(out, plain) and out.stride() == plain.stride()
    if not resample:
        assert _same(plain, R.input_batch(fx["src"], None, S, idx=CASES.IDX, flip=CASES.FLIP, box=boxes.cpu(), dtype=dtype, channels_last=cl), cl)


def test_refused_calls(fx):
    from moma_amd import _lib, ops
    with pytest.raises(_lib.MomaHipError):
        ops.input_batch(fx["dsrc"], fx["lut"], 21, idx=fx["idx"])                  # S_h > H in window mode
    with pytest.raises(ValueError):
        ops.input_batch(fx["dsrc"], fx["lut"], 16, idx=fx["idx"], flip=fx["flip"][:4])
    with pytest.raises(TypeError):
        ops.input_batch(fx["dsrc"].float(), fx["lut"], 16)


# ---- both trainers on a pack ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pack_path(tmp_path_factory):
    """24 train and 8 val images of 32 x 32, 4 classes, as PNG files through the builder"""
    from PIL import Image
    from moma_amd.dataset import pack
    root = tmp_path_factory.mktemp("input_pack")
    rng = np.random.default_rng(11)
    for split, per_class in (("train", 6), ("val", 2)):
        for c in range(4):
            d = root / "src" / split / f"class{c}"
            d.mkdir(parents=True)
            for i in range(per_class):
                Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(d / f"{i}.png")
    pack.build_pack(str(root / "src"), str(root / "pack"), resize=32)
    return str(root / "pack")


T_ARGV = ["--model", "resnet8", "--dataset", "cifar100", "--n_cls", "4", "--epochs", "1", "--print_freq", "1000", "--learning_rate", "0.01",
          "--num_workers", "0", "--miopen_find", "off", "--skip_test", "--seed", "7"]
S_ARGV = ["--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4", "--epochs", "1", "--print_freq", "1000",
          "--learning_rate", "0.01", "--num_workers", "0", "--miopen_find", "off", "--skip_test", "--seed", "7", "--no_graph_teacher",
          "--no_graph_student"]


def _run(which, pack_path, tmp_path, monkeypatch, extra):
    """one main_worker; returns (the batches the training loop is handed, its (acc, loss), opt)"""
    from moma_amd import train_student_moma as TS, train_teacher as TT
    mod, argv, name = (TS, S_ARGV, "train_distill_moma") if which == "student" else (TT, T_ARGV, "train")
    real = getattr(mod, name)
    seen = {}

    def spy(epoch, loader, *a, **kw):
        seen["batches"] = [tuple(t.clone() for t in data) for data in loader]     # (an epoch's batches repeat: seeded by the epoch)
        seen["result"] = real(epoch, loader, *a, **kw)
        return seen["result"]
    monkeypatch.setattr(mod, name, spy)
    opt = mod.parse_option(argv + ["--save_root", str(tmp_path), "--data_pack", pack_path, "--aug_train", "NULL"] + extra)
    opt.world_size, opt.ngpus_per_node = 1, 1
    mod.main_worker(0, 1, opt)
    return seen["batches"], seen["result"], opt


def _first_batch_ref(pack_path, batch, seed=7, epoch=1, **kw):
    from moma_amd.dataset import pack
    src = torch.from_numpy(np.load(os.path.join(pack_path, "train_images.npy")))
    labels = torch.from_numpy(np.load(os.path.join(pack_path, "train_labels.npy")))
    ids = R.sampler_indices(len(src), 1, 0, epoch, seed)[:batch]
    flip = torch.rand(batch, generator=torch.Generator().manual_seed(pack._rng_seed(seed, 0, epoch))) < 0.5
    return R.input_batch(src, None, 32, idx=ids, flip=flip, **kw), labels[ids], torch.tensor(ids)


@pytest.mark.parametrize("which,extra", [("teacher", []), ("student", ["--distill", "kd"])], ids=["teacher", "student-kd"])
def test_an_epoch_from_a_pack_on_both_placements(which, extra, pack_path, tmp_path, monkeypatch):
    runs = {}
    for place in ("gpu", "host"):
        runs[place] = _run(which, pack_path, tmp_path / place, monkeypatch, extra + ["--batch_size", "8", "--data_device", place])
        monkeypatch.undo()
    ref_x, ref_y, _ids = _first_batch_ref(pack_path, 8)
    for place, (batches, (acc, loss), opt) in runs.items():
        assert len(batches) == 3 and opt.steps_per_epoch == 3 and all(x.is_cuda and x.shape == (8, 3, 32, 32) for x, _ in batches)
        assert _same(batches[0][0], ref_x, False) and torch.equal(batches[0][1].cpu(), ref_y), place
        assert np.isfinite(loss) and np.isfinite(acc), place
    for (xa, ya), (xb, yb) in zip(runs["gpu"][0], runs["host"][0]):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)                        # placement does not change a batch


def test_a_ragged_last_batch_bf16_channels_last(pack_path, tmp_path, monkeypatch):
    batches, (acc, loss), opt = _run("teacher", pack_path, tmp_path, monkeypatch,
                                     ["--batch_size", "10", "--amp", "bf16", "--input_dtype", "bf16", "--channels_last"])
    assert [x.shape[0] for x, _ in batches] == [10, 10, 4] and np.isfinite(loss)
    ref_x, ref_y, _ids = _first_batch_ref(pack_path, 10, dtype=torch.bfloat16, channels_last=True)
    assert _same(batches[0][0], ref_x, True) and torch.equal(batches[0][1].cpu(), ref_y)


def test_a_crd_epoch_from_a_pack(pack_path, tmp_path, monkeypatch):
    from moma_amd.dataset.pack import PackSampleLoader
    batches, (acc, loss), opt = _run("student", pack_path, tmp_path, monkeypatch,
                                     ["--distill", "crd", "--batch_size", "8", "--nce_k", "16", "--feat_dim", "64", "-b", "0.8"])
    assert opt.n_data == 24 and len(batches) == 3 and np.isfinite(loss)
    ref_x, ref_y, ids = _first_batch_ref(pack_path, 8)
    x, y, index, cidx = batches[0]
    assert _same(x, ref_x, False) and torch.equal(y.cpu(), ref_y) and torch.equal(index.cpu(), ids)
    labels = torch.from_numpy(np.load(os.path.join(pack_path, "train_labels.npy")))
    assert cidx.shape == (8, 17) and torch.equal(cidx[:, 0], index) and bool((labels[cidx[:, 1:].cpu()] != y.cpu()[:, None]).all())
    assert PackSampleLoader is not None
