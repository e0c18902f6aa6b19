"""Host side of the data-pack path (no GPU): the pack builder against PIL, the loaders' order / shards / batches / boxes with the kernel
call replaced by the restatement (tests/input_ref.py), the shared contrast-index helper, the CLI of both trainers, and the new
entry point's place in the C ABI."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import input_cases as CASES, input_ref as R


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _png_tree(root):
    """8 small PNGs: train a (30x42, 45x33, 40x40), train b (33x45, 50x31), val a (30x42, 36x36), val b (45x33)"""
    from PIL import Image
    rng = np.random.default_rng(5)
    sizes = {("train", "a"): [(30, 42), (45, 33), (40, 40)], ("train", "b"): [(33, 45), (50, 31)],
             ("val", "a"): [(30, 42), (36, 36)], ("val", "b"): [(45, 33)]}
    files = {}
    for (split, cls), whs in sizes.items():
        d = root / split / cls
        d.mkdir(parents=True)
        for i, (w, h) in enumerate(whs):
            p = d / f"im{i}.png"
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
            files.setdefault(split, []).append((str(p), 0 if cls == "a" else 1))
    return files


def _write_pack(root, n_train=10, n_val=6, H=20, W=28, n_cls=3, seed=3):
    """a pack written directly (no image files): labels cycle through the classes"""
    root.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    sizes = {}
    for split, n in (("train", n_train), ("val", n_val)):
        np.save(root / f"{split}_images.npy", rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8))
        np.save(root / f"{split}_labels.npy", (np.arange(n) % n_cls).astype(np.int64))
        sizes[split] = n
    meta = {"n_cls": n_cls, "classes": [f"c{i}" for i in range(n_cls)], "mean": list(R.MEAN), "std": list(R.STD), "H": H, "W": W,
            "splits": sizes, "args": {}}
    (root / "meta.json").write_text(json.dumps(meta))
    return str(root)


def _stub(loader, seen=None):
    def call(src, lut, size, **kw):
        if seen is not None:
            seen.append(dict(kw, src=src, size=size))
        return R.input_batch(src, lut, size, **kw)
    loader.input_batch = call
    return loader


# ---- the builder ----------------------------------------------------------------------------------------------------------------
def test_pack_equals_pil_resize_and_centre_crop(tmp_path):
    from PIL import Image
    from moma_amd.dataset import pack
    files = _png_tree(tmp_path / "src")
    meta = pack.build_pack(str(tmp_path / "src"), str(tmp_path / "pack"), resize=24)
    assert meta["n_cls"] == 2 and meta["classes"] == ["a", "b"] and (meta["H"], meta["W"]) == (24, 24)
    assert meta["splits"] == {"train": 5, "val": 3} and meta == pack.read_meta(str(tmp_path / "pack"))
    for split in ("train", "val"):
        images, labels = pack.open_split(str(tmp_path / "pack"), split)
        assert isinstance(images, np.memmap) and images.flags["C_CONTIGUOUS"] and images.dtype == np.uint8 and labels.dtype == np.int64
        assert labels.tolist() == [y for _, y in files[split]]                    # sorted class names, sorted files
        for k, (path, _y) in enumerate(files[split]):
            im = Image.open(path).convert("RGB")
            w, h = im.size
            ow, oh = (24, int(24 * h / w)) if w <= h else (int(24 * w / h), 24)    # Resize(24): the smaller edge
            a = np.asarray(im.resize((ow, oh), Image.BILINEAR))
            top, left = int(round((oh - 24) / 2.0)), int(round((ow - 24) / 2.0))    # CenterCrop(24)
            assert np.array_equal(images[k], a[top:top + 24, left:left + 24]), path


def test_pack_refuses_a_too_small_image_by_name_and_chunks_do_not_matter(tmp_path):
    from moma_amd.dataset import make_pack, pack
    _png_tree(tmp_path / "src")
    with pytest.raises(ValueError, match=r"im0\.png.*smaller"):                   # 30 x 42 -> 24 x 33 < 32
        pack.build_pack(str(tmp_path / "src"), str(tmp_path / "bad"), resize=24, center_crop=32)
    make_pack.main(["--src", str(tmp_path / "src"), "--out", str(tmp_path / "one"), "--resize", "30", "--center_crop", "22"])
    make_pack.main(["--src", str(tmp_path / "src"), "--out", str(tmp_path / "three"), "--resize", "30", "--center_crop", "22",
                    "--chunk", "3"])
    for name in ("train_images.npy", "train_labels.npy", "val_images.npy", "val_labels.npy"):
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "three" / name).read_bytes(), name
    assert np.load(tmp_path / "one" / "train_images.npy").shape == (5, 22, 22, 3)


# ---- the loaders ----------------------------------------------------------------------------------------------------------------
def test_epoch_permutations_and_shards_follow_the_sampler_rule(tmp_path):
    from moma_amd.dataset.pack import PackLoader, epoch_indices
    path = _write_pack(tmp_path / "p")
    for world, rank, epoch in ((1, 0, 0), (1, 0, 4), (3, 0, 1), (3, 2, 1), (4, 3, 7)):
        assert epoch_indices(10, world, rank, epoch, 11, True).tolist() == R.sampler_indices(10, world, rank, epoch, 11), (world, rank)
    assert epoch_indices(10, 3, 1, 5, 11, False).tolist() == R.sampler_indices(10, 3, 1, 5, 11, shuffle=False) == [1, 4, 7, 0]
    shards = [_stub(PackLoader(path, "train", 4, 20, aug="RRC", seed=11, rank=r, world=3)) for r in range(3)]
    for s in shards:
        s.set_epoch(2)
    ids = [s._indices.tolist() for s in shards]
    assert [len(i) for i in ids] == [4, 4, 4] and set(sum(ids, [])) == set(range(10))
    perm = R.sampler_indices(10, 1, 0, 2, 11)
    assert [ids[k % 3][k // 3] for k in range(12)] == perm + perm[:2]              # padded by wrap-around
    one = _stub(PackLoader(path, "train", 4, 20, aug="RRC", seed=11))
    one.set_epoch(1)
    e1 = one._indices.tolist()
    one.set_epoch(2)
    e2 = one._indices.tolist()
    one.set_epoch(1)
    assert e1 != e2 and one._indices.tolist() == e1 and sorted(e1) == list(range(10))
    val = PackLoader(path, "val", 4, 20)
    val.set_epoch(3)
    assert val._indices.tolist() == list(range(6))                                # fixed order for val / test


def test_batches_ragged_tail_random_state_and_placement(tmp_path):
    from moma_amd.dataset.pack import PackLoader
    path = _write_pack(tmp_path / "p", H=20, W=20)
    src = torch.from_numpy(np.load(os.path.join(path, "train_images.npy")))
    labels = torch.from_numpy(np.load(os.path.join(path, "train_labels.npy")))
    seen = []
    ld = _stub(PackLoader(path, "train", 4, 20, aug="NULL", seed=5, data_device="gpu"), seen)
    ld.set_epoch(1)
    got = list(ld)
    assert len(ld) == 3 and [x.shape[0] for x, _ in got] == [4, 4, 2]              # the short last batch is kept
    ids = ld._indices
    for k, (x, y) in enumerate(got):
        i = ids[4 * k:4 * k + 4]
        assert torch.equal(y, labels[i]) and seen[k]["box"] is None and not seen[k]["resample"]
        assert torch.equal(seen[k]["idx"], i) and seen[k]["flip"].dtype == torch.uint8 and len(seen[k]["flip"]) == len(i)
        assert torch.equal(x, R.input_batch(src, None, 20, idx=i, flip=seen[k]["flip"]))
    ld.set_epoch(1)
    again = list(ld)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(got, again))               # (seed, rank, epoch) repeats
    assert all(torch.equal(a["flip"], b["flip"]) for a, b in zip(seen[:3], seen[3:]))
    host = _stub(PackLoader(path, "train", 4, 20, aug="NULL", seed=5, data_device="host"), seen2 := [])
    host.set_epoch(1)
    other = list(host)
    assert all(s["idx"] is None for s in seen2) and [s["batch"] for s in seen2] == [4, 4, 2]
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, other))      # host = gpu placement
    # val: the centred window, no flip
    v = _stub(PackLoader(path, "val", 4, 16), seen3 := [])
    xs = list(v)
    assert [x.shape for x, _ in xs] == [(4, 3, 16, 16), (2, 3, 16, 16)] and all(s["flip"] is None and s["box"] is None for s in seen3)
    vsrc = torch.from_numpy(np.load(os.path.join(path, "val_images.npy")))
    assert torch.equal(xs[0][0], R.normalize(vsrc[:4, 2:18, 2:18]))
    # dtype and layout reach the call
    c = _stub(PackLoader(path, "val", 4, 16, dtype=torch.bfloat16, channels_last=True))
    x = next(iter(c))[0]
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="NULL"):
        PackLoader(path, "train", 4, 16, aug="NULL")
    with pytest.raises(NotImplementedError, match="NULL.*RRC"):
        PackLoader(path, "train", 4, 16, aug="RA")


def test_crd_tuples_from_a_pack(tmp_path):
    from moma_amd.dataset.pack import PackSampleLoader
    path = _write_pack(tmp_path / "p", n_train=12, H=20, W=20)
    labels = torch.from_numpy(np.load(os.path.join(path, "train_labels.npy")))
    ld = _stub(PackSampleLoader(path, "train", 5, 20, 16, "exact", aug="NULL", seed=2))
    assert ld.n_data == 12
    ld.set_epoch(1)
    n = 0
    for x, y, index, cidx in ld:
        assert cidx.shape == (len(index), 17) and torch.equal(cidx[:, 0], index) and torch.equal(y, labels[index])
        assert bool((labels[cidx[:, 1:]] != y[:, None]).all())                    # exact: no negative of the sample's own class
        assert int(cidx.min()) >= 0 and int(cidx.max()) < 12
        n += len(index)
    assert n == 12
    relax = _stub(PackSampleLoader(path, "train", 5, 20, 16, "relax", aug="NULL", seed=2))
    for _x, _y, index, cidx in relax:
        assert bool((cidx[:, 1:] != index[:, None]).all())


def test_boxes_follow_get_params(tmp_path):
    from moma_amd.dataset.pack import RATIO, rrc_boxes
    g = torch.Generator().manual_seed(9)
    for (Hh, Ww, crop) in ((20, 28, 0.2), (32, 32, 0.08), (20, 28, 0.6)):
        u = torch.rand(64, 10, 4, generator=g, dtype=torch.float64)
        boxes = rrc_boxes(Hh, Ww, crop, u)
        assert boxes.dtype == torch.int32 and boxes.shape == (64, 4)
        for b in range(64):
            top, left, h, w = boxes[b].tolist()
            assert (top, left, h, w) == R.rrc_box(Hh, Ww, crop, u[b])
            assert top >= 0 and left >= 0 and 1 <= h and top + h <= Hh and 1 <= w and left + w <= Ww
            slack = 0.5 * (h + w) + 0.25                                          # w and h are each rounded to an integer
            assert crop * Hh * Ww - slack <= h * w <= Hh * Ww + slack
            assert (w + 0.5) / (h - 0.5) >= RATIO[0] and (w - 0.5) / (h + 0.5) <= RATIO[1]
    # the fallback: nearly the whole area of a 20 x 28 image at ratios below 1.15 fits in no try -> the centred 20 x 27 (ratio 4/3)
    u = torch.rand(16, 10, 4, generator=g, dtype=torch.float64)
    u[..., 1] *= 0.5
    boxes = rrc_boxes(20, 28, 0.999, u)
    assert boxes.tolist() == [[0, 0, 20, 27]] * 16 and all(R.rrc_box(20, 28, 0.999, u[b]) == (0, 0, 20, 27) for b in range(16))
    assert RATIO[0] <= 27 / 20 + 1e-9 and 27 / 20 <= RATIO[1] + 0.5 / 20
    # a tall image: the fallback keeps the width
    assert rrc_boxes(28, 20, 0.999, u).tolist() == [[0, 0, 27, 20]] * 16


def test_synthetic_sample_loader_is_unchanged_by_the_shared_helper():
    """the tensors SyntheticSampleLoader yields, against its formula written out here (one seed, both modes)"""
    from moma_amd.dataset.synthetic import SyntheticSampleLoader
    for mode in ("exact", "relax"):
        B, n_cls, nce_k, seed = 6, 4, 9, 123                                      # n_data = 3 batches of 6 = 18
        ld = SyntheticSampleLoader(3, B, 8, n_cls, nce_k, mode, seed)
        g = torch.Generator().manual_seed(seed)
        images = [torch.randn(B, 3, 8, 8, generator=g) for _ in range(2)]
        sample_labels = torch.randint(0, n_cls, (18,), generator=g)
        perm = torch.randperm(18, generator=g)
        counts = torch.bincount(sample_labels, minlength=n_cls)
        starts, order = torch.cumsum(counts, 0) - counts, torch.argsort(sample_labels, stable=True)
        gen = torch.Generator().manual_seed(seed + 1)
        for i, (x, y, index, cidx) in enumerate(ld):
            ref_index = perm[(torch.arange(B) + i * B) % 18]
            ref_y = sample_labels[ref_index]
            u = torch.rand(B, nce_k, generator=gen, dtype=torch.float64)
            if mode == "exact":
                cnt, start = counts[ref_y].unsqueeze(1), starts[ref_y].unsqueeze(1)
                r = torch.minimum((u * (18 - cnt)).long().clamp_(max=17), 18 - cnt - 1)
                neg = order[torch.where(r < start, r, r + cnt)]
            else:
                r = (u * 17).long().clamp_(max=16)
                neg = torch.where(r < ref_index.unsqueeze(1), r, r + 1)
            assert torch.equal(x, images[i % 2]) and torch.equal(index, ref_index) and torch.equal(y, ref_y)
            assert torch.equal(cidx, torch.cat([ref_index.unsqueeze(1), neg], dim=1))


# ---- the bilinear rule on the fixture --------------------------------------------------------------------------------------------
def _header_arithmetic_levels(src, idx, box, S):
    """include/moma_hip.h (IN, resample = 1) restated: integer tap weights over 2 S, the four products summed in float32"""
    f32 = torch.float32
    out = []
    for b, n in enumerate(idx):
        top, left, h, w = box[b]
        img = src[n].to(f32)

        def taps(extent, first, full):
            d = 2 * S
            num = ((2 * torch.arange(S) + 1) * extent - S).clamp(0, (extent - 1) * d)
            i0 = num // d
            return (i0 + first).clamp(0, full - 1), ((i0 + 1).clamp(max=extent - 1) + first).clamp(0, full - 1), (num - i0 * d)
        y0, y1, ry = taps(h, top, src.shape[1])
        x0, x1, rx = taps(w, left, src.shape[2])
        fx, gx = rx.to(f32)[None, :, None], (2 * S - rx).to(f32)[None, :, None]
        fy, gy = ry.to(f32)[:, None, None], (2 * S - ry).to(f32)[:, None, None]
        ht = img[y0][:, x0] * gx + img[y0][:, x1] * fx                            # exact: integers below 2^24
        hb = img[y1][:, x0] * gx + img[y1][:, x1] * fx
        num = (ht.double() * gy.double() + (hb * fy).double()).to(f32)            # fmaf(ht, gy, hb * fy)
        v = num / (torch.tensor(2.0 * S, dtype=f32) * torch.tensor(2.0 * S, dtype=f32))
        out.append(torch.floor(v + 0.5).clamp(0, 255).to(torch.uint8))
    return torch.stack(out)


@pytest.mark.parametrize("name", list(CASES.BILINEAR_CASES))
def test_bilinear_fixture_has_few_near_ties_and_the_float32_rule_meets_them(name):
    """the share of values the GPU test may forgive (within 1e-4 of a half-integer without being one) is at most 1 % per case, none
    in the dyadic case; and the header's float32 arithmetic gives the float64 restatement's level everywhere else.  Five float32
    roundings of a value <= 255 are at most 5 * 2^-24 * 255 = 7.6e-5 < 1e-4, so the rule holds for any source."""
    S, boxes, dyadic = CASES.BILINEAR_CASES[name]
    src = CASES.source()
    values = R.bilinear_values(src, torch.tensor(CASES.IDX), torch.tensor(boxes), S, S)
    exempt = R.near_tie(values, CASES.TIE_EPS)
    share = float(exempt.double().mean())
    print(f"{name}: near-tie share {share:.4%} of {values.numel()} values")
    assert share <= CASES.TIE_SHARE
    if dyadic:
        assert share == 0.0 and bool(((values * 1024) == torch.floor(values * 1024)).all())
        assert int((values - values.floor() == 0.5).sum()) > 0                    # exact ties are there to be met
    want, got = R.to_levels(values).int(), _header_arithmetic_levels(src, CASES.IDX, boxes, S).int()
    diff = (got - want).abs()
    assert int(diff.max()) <= 1 and bool((diff[~exempt] == 0).all())


def test_lut_is_totensor_and_normalize_bit_for_bit():
    from moma_amd import ops
    lut = ops.input_lut(R.MEAN, R.STD)
    levels = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3)
    ref = R.normalize(levels)[0].reshape(3, 256)
    assert lut.dtype == torch.float32 and torch.equal(lut, ref)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------
S_ARGV = ["--distill", "kd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "3",
          "--batch_size", "4", "--epochs", "1", "--print_freq", "1000", "--seed", "7", "--num_workers", "0"]
T_ARGV = ["--model", "resnet8", "--dataset", "cifar100", "--n_cls", "3", "--batch_size", "4", "--epochs", "1", "--print_freq", "1000",
          "--learning_rate", "0.01", "--num_workers", "0", "--no_fused"]


def test_both_parsers_take_the_new_flags():
    from moma_amd import train_student_moma as TS, train_teacher as TT
    for mod, argv in ((TS, S_ARGV), (TT, T_ARGV)):
        opt = mod.parse_option(argv)
        assert opt.data_pack is None and opt.data_device is None and opt.input_dtype == "fp32" and opt.aug_train == "RA"
        opt = mod.parse_option(argv + ["--data_pack", "/some/pack", "--data_device", "host", "--input_dtype", "bf16", "--aug_train", "RRC"])
        assert (opt.data_pack, opt.data_device, opt.input_dtype, opt.aug_train) == ("/some/pack", "host", "bf16", "RRC")
        with pytest.raises(SystemExit):
            mod.parse_option(argv + ["--data_device", "disk"])


@pytest.mark.parametrize("which", ["student", "teacher"])
def test_a_pack_refuses_ra_a_size_mismatch_and_a_wrong_class_count(which, tmp_path, monkeypatch):
    from moma_amd import train_student_moma as TS, train_teacher as TT
    mod, argv = (TS, S_ARGV) if which == "student" else (TT, T_ARGV)
    monkeypatch.setattr(mod, "_REQUIRE_GPU", False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    path = _write_pack(tmp_path / "p", H=20, W=28)                                # not 32 x 32

    def run(extra):
        opt = mod.parse_option(argv + ["--save_root", str(tmp_path / "save"), "--data_pack", path] + extra)
        opt.world_size, opt.ngpus_per_node = 1, 1
        mod.main_worker(0, 1, opt)
    with pytest.raises(NotImplementedError, match="NULL.*RRC"):
        run([])                                                                   # RA is the default
    with pytest.raises(ValueError, match="NULL.*20 x 28"):
        run(["--aug_train", "NULL"])
    with pytest.raises(ValueError, match="n_cls"):
        run(["--aug_train", "RRC", "--n_cls", "5"])
    with pytest.raises(ValueError, match="window"):
        run(["--aug_train", "RRC"])                                               # validation's 32 x 32 window does not fit


@pytest.mark.parametrize("which", ["student", "teacher"])
def test_without_the_flag_the_synthetic_loaders_are_built(which, tmp_path, monkeypatch):
    from moma_amd import train_student_moma as TS, train_teacher as TT
    from moma_amd.dataset import pack
    mod, argv = (TS, S_ARGV) if which == "student" else (TT, T_ARGV)
    monkeypatch.setattr(mod, "_REQUIRE_GPU", False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    built = []

    class Spy(mod.SyntheticLoader):
        def __init__(self, *a, **kw):
            built.append(a[:5])
            super().__init__(*a, **kw)

    def never(*a, **kw):
        raise AssertionError("the pack path was entered without --data_pack")
    monkeypatch.setattr(mod, "SyntheticLoader", Spy)
    monkeypatch.setattr(pack, "prepare", never)
    monkeypatch.setattr(pack, "build_loaders", never)
    opt = mod.parse_option(argv + ["--save_root", str(tmp_path), "--steps_per_epoch", "1"])
    opt.world_size, opt.ngpus_per_node = 1, 1
    mod.main_worker(0, 1, opt)
    assert built == [(1, 4, 32, 3, opt.seed), (1, 4, 32, 3, opt.seed + 1)] and opt.steps_per_epoch == 1      # train, val


def test_teacher_trains_from_a_pack_on_the_restatement(tmp_path, monkeypatch):
    """host logic end to end without a GPU: prepare, the loaders, set_epoch, a ragged last batch, validation and test on the val split"""
    from moma_amd import ops, train_teacher as TT
    monkeypatch.setattr(TT, "_REQUIRE_GPU", False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(ops, "input_batch", R.input_batch)
    path = _write_pack(tmp_path / "p", n_train=10, n_val=6, H=32, W=32)
    seen = []
    real = TT.train

    def spy(epoch, loader, *a, **kw):
        seen.append((epoch, loader.epoch, len(loader), [x.shape[0] for x, _ in loader]))
        return real(epoch, loader, *a, **kw)
    monkeypatch.setattr(TT, "train", spy)
    opt = TT.parse_option(T_ARGV + ["--save_root", str(tmp_path / "save"), "--data_pack", path, "--aug_train", "NULL", "--epochs", "2",
                                    "--steps_per_epoch", "77"])
    opt.world_size, opt.ngpus_per_node = 1, 1
    TT.main_worker(0, 1, opt)
    assert seen == [(1, 1, 3, [4, 4, 2]), (2, 2, 3, [4, 4, 2])] and opt.steps_per_epoch == 3
    assert os.path.exists(os.path.join(opt.save_folder, "stat.json")) and os.path.exists(os.path.join(opt.save_folder, "ckpt_last.pth"))


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_input_batch_is_declared_bound_exported_and_checks_its_shapes():
    from moma_amd import _lib, build
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "moma_hip.h")).read()
    assert "int moma_input_batch(" in header and "moma_input_batch" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.moma_version() == 4
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    call = lambda N, H, W, B, Sh, Sw, resample=0, dtype=0, layout=0, src=p, lut=p, out=p, box=None: lib.moma_input_batch(
        src, None, None, box, lut, out, N, H, W, B, Sh, Sw, resample, dtype, layout, None)
    assert call(2, 8, 8, 2, 9, 8) < 0 and call(2, 8, 8, 2, 8, 9) < 0              # S > H, S > W: refused, nothing launched
    assert call(2, 8, 8, 2, 9, 9, resample=1) < 0                                 # (no box: the centred window, the same rule)
    assert call(2, 8, 8, 0, 4, 4) == 0                                            # an empty batch
    assert call(2, 8, 8, 2, 4, 4, src=None) == -1 and call(2, 8, 8, 2, 4, 4, lut=None) == -1 and call(2, 8, 8, 2, 4, 4, out=None) == -1
    assert call(2, 8, 8, 2, 4, 4, dtype=2) == -3 and call(2, 8, 8, 2, 4, 4, layout=2) == -3 and call(2, 8, 8, 2, 4, 4, resample=2) == -2
    assert call(2, 8, 8, 2, 0, 4) == -2 and call(0, 8, 8, 2, 4, 4) == -2
    assert call(2, 8, 1 << 15, 2, 4, 4) == -6 and call(2, 8192, 8192, 2, 4097, 4097, resample=1, box=p) == -6
    with pytest.raises(_lib.MomaHipError):
        from moma_amd import ops
        ops.input_batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(3, 256), 4)      # CPU tensors: no fallback
