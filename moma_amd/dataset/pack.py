"""Data packs: real images for both trainers (`--data_pack PATH`).

A pack is a directory written once by `python -m moma_amd.dataset.make_pack`:
    {split}_images.npy   uint8 [N, H, W, 3], C-contiguous, opened with np.load(mmap_mode="r")     split in train, val, test (optional)
    {split}_labels.npy   int64 [N]
    meta.json            n_cls, classes, mean, std, H, W, the splits' sizes and the builder's arguments
The builder applies the DETERMINISTIC part of the reference's transforms (dataset/histo_dataset.py:194-239): `Resize(size)` as
torchvision does it on a PIL image (smaller edge to `size`, the other to int(size * long / short), Image.BILINEAR) and a centre
crop to one common size.  Everything random or per batch -- the flip, the crop window (CenterCrop for val / test), RandomResizedCrop
(:1054-1058), ToTensor, Normalize, the layout and the dtype -- is one launch of csrc/input.hip per batch (ops.input_batch).
RandAugment is chains of PIL operations and is not built.

The loaders yield what dataset/synthetic.py's yield, on the device, with the reference's epoch behaviour (:387-410): a seeded
permutation per epoch, DistributedSampler's shards (the permutation padded by wrap-around to a multiple of the world size, rank r
takes every W-th from r) and the short last batch kept.  Flips and boxes come from a generator seeded by (seed, rank, epoch), so a
resumed epoch repeats."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from .contrast import class_segments, contrast_indices

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)         # (histo_dataset.py:200: ImageNet's)
SPLITS = ("train", "val", "test")
RATIO = (3.0 / 4.0, 4.0 / 3.0)                                   # RandomResizedCrop's default ratio range
GPU_SHARE = 0.25        # --data_device unset: the split lives on the device when it takes at most this share of the free memory


# ---- the builder ----------------------------------------------------------------------------------------------------------------
def resize_size(w, h, size):
    """(ow, oh) of torchvision's Resize(size) on a w x h image: the smaller edge becomes `size`"""
    if (w <= h and w == size) or (h <= w and h == size):
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


def centre_offset(full, s):
    """CenterCrop's offset"""
    return int(round((full - s) / 2.0))


def load_image(path, resize, crop):
    """one file -> uint8 [crop, crop, 3]: convert('RGB'), Resize(resize), centre crop; refuses an image that comes out smaller"""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        ow, oh = resize_size(im.width, im.height, resize)
        if (ow, oh) != im.size:
            im = im.resize((ow, oh), Image.BILINEAR)
        if ow < crop or oh < crop:
            raise ValueError(f"{path}: {ow} x {oh} after Resize({resize}) is smaller than the pack's {crop} x {crop}")
        a = np.asarray(im, dtype=np.uint8)
    top, left = centre_offset(oh, crop), centre_offset(ow, crop)
    return a[top:top + crop, left:left + crop]


def list_split(root, split, classes=None):
    """([(path, label)], classes) of ROOT/split/<class name>/*, sorted; classes numbered by sorted name (those of `classes` if given)"""
    d = os.path.join(root, split)
    names = sorted(n for n in os.listdir(d) if os.path.isdir(os.path.join(d, n)))
    if classes is None:
        classes = names
    unknown = [n for n in names if n not in classes]
    if unknown:
        raise ValueError(f"{d}: classes {unknown} are not in the train split")
    files = []
    for n in names:
        for f in sorted(os.listdir(os.path.join(d, n))):
            p = os.path.join(d, n, f)
            if os.path.isfile(p):
                files.append((p, classes.index(n)))
    return files, classes


def build_pack(src, out, resize=512, center_crop=None, chunk=256):
    """Write the pack of the image tree `src` into `out`; at most `chunk` images are in memory at a time."""
    crop = int(center_crop) if center_crop else int(resize)
    os.makedirs(out, exist_ok=True)
    classes, sizes = None, {}
    for split in SPLITS:
        if not os.path.isdir(os.path.join(src, split)):
            if split == "test":
                continue
            raise FileNotFoundError(f"{src}: no {split}/ folder")
        files, classes = list_split(src, split, classes)
        if not files:
            raise ValueError(f"{os.path.join(src, split)}: no images")
        n = len(files)
        images = np.lib.format.open_memmap(os.path.join(out, f"{split}_images.npy"), mode="w+", dtype=np.uint8, shape=(n, crop, crop, 3))
        for i0 in range(0, n, chunk):
            block = np.stack([load_image(p, resize, crop) for p, _ in files[i0:i0 + chunk]])
            images[i0:i0 + len(block)] = block
            images.flush()
        del images
        np.save(os.path.join(out, f"{split}_labels.npy"), np.asarray([y for _, y in files], dtype=np.int64))
        sizes[split] = n
    meta = {"n_cls": len(classes), "classes": classes, "mean": list(MEAN), "std": list(STD), "H": crop, "W": crop, "splits": sizes,
            "args": {"src": os.path.abspath(src), "resize": int(resize), "center_crop": center_crop}}
    with open(os.path.join(out, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    return meta


def read_meta(pack):
    with open(os.path.join(pack, "meta.json")) as f:
        return json.load(f)


def open_split(pack, split):
    """(images memmap uint8 [N, H, W, 3], labels int64 [N]) of one split"""
    images = np.load(os.path.join(pack, f"{split}_images.npy"), mmap_mode="r")
    labels = np.load(os.path.join(pack, f"{split}_labels.npy"))
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3 or not images.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{pack}: {split}_images.npy is not a C-contiguous uint8 [N, H, W, 3] array")
    if labels.dtype != np.int64 or labels.shape != (images.shape[0],):
        raise ValueError(f"{pack}: {split}_labels.npy is not int64 [{images.shape[0]}]")
    return images, labels


# ---- order, shards, boxes ---------------------------------------------------------------------------------------------------------
def epoch_indices(n, world, rank, epoch, seed, shuffle):
    """The sample ids of rank `rank` in epoch `epoch`, by DistributedSampler's rule (one rank: the whole permutation)."""
    if shuffle:
        order = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) + int(epoch)))
    else:
        order = torch.arange(n)
    per_rank = math.ceil(n / world)
    pad = per_rank * world - n
    if pad:
        order = torch.cat([order, order.repeat(math.ceil(pad / n))[:pad]])
    return order[rank::world]


def rrc_boxes(H, W, crop, u):
    """RandomResizedCrop.get_params for a batch, vectorised: u float64 [B, 10, 4] uniform draws (area, log-ratio, top, left) of the ten
    tries.  area = H W (crop + u (1 - crop)); ratio = exp(log 3/4 + u log(16/9)); w = round(sqrt(area ratio)), h = round(sqrt(area /
    ratio)); the FIRST try with 0 < w <= W and 0 < h <= H wins, at top = floor(u (H - h + 1)), left likewise; none: the centred
    whole image, cut to the ratio range.  -> int32 [B, 4] = (top, left, h, w)."""
    area = H * W * (crop + u[..., 0] * (1.0 - crop))
    ratio = torch.exp(math.log(RATIO[0]) + u[..., 1] * (math.log(RATIO[1]) - math.log(RATIO[0])))
    w = torch.round(torch.sqrt(area * ratio)).long()
    h = torch.round(torch.sqrt(area / ratio)).long()
    ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    first = torch.argmax(ok.to(torch.int8), dim=1, keepdim=True)                   # (the first True; 0 where there is none)
    pick = lambda t: torch.gather(t, 1, first).squeeze(1)
    w, h, found = pick(w), pick(h), ok.any(dim=1)
    top = torch.minimum((pick(u[..., 2]) * (H - h + 1).double()).long(), H - h)    # (rows without a fitting try: replaced below)
    left = torch.minimum((pick(u[..., 3]) * (W - w + 1).double()).long(), W - w)
    in_ratio = W / H
    if in_ratio < RATIO[0]:
        fw, fh = W, int(round(W / RATIO[0]))
    elif in_ratio > RATIO[1]:
        fh, fw = H, int(round(H * RATIO[1]))
    else:
        fw, fh = W, H
    fb = torch.tensor([(H - fh) // 2, (W - fw) // 2, fh, fw])
    return torch.where(found.unsqueeze(1), torch.stack([top, left, h, w], dim=1), fb.unsqueeze(0)).to(torch.int32)


def _rng_seed(seed, rank, epoch):
    return ((int(seed) * 1000003 + int(rank)) * 1000003 + int(epoch)) % (1 << 62)


# ---- the loaders ------------------------------------------------------------------------------------------------------------------
class PackLoader:
    """(images [B, 3, S, S], labels int64 [B]) batches of one split of a pack, on `device`.

    aug: None -- the centred S x S window, no flip, fixed order (val / test); 'NULL' -- flip only (the pack's images must be S x S);
    'RRC' -- RandomResizedCrop(S, scale=(crop, 1)) + flip.  data_device: 'gpu' -- the split's uint8 rows live on `device` and the
    kernel gathers through idx; 'host' -- a batch's rows are gathered from the memmap into pinned memory, copied asynchronously,
    and the kernel reads them in place; None -- 'gpu' when the split takes at most GPU_SHARE of the free device memory."""

    def __init__(self, pack, split, batch_size, image_size, aug=None, crop=0.2, seed=0, rank=0, world=1, device="cpu",
                 data_device=None, dtype=torch.float32, channels_last=False):
        from .. import ops
        self.input_batch = ops.input_batch                        # (host-logic tests put the restatement here)
        self.meta = read_meta(pack)
        self.memmap, labels = open_split(pack, split)
        self.N, self.H, self.W = self.memmap.shape[:3]
        self.S, self.B, self.aug, self.crop = int(image_size), int(batch_size), aug, float(crop)
        if aug not in (None, "NULL", "RRC"):
            raise NotImplementedError(f"--aug_train {aug} is not built for a data pack (RandAugment is chains of PIL operations): "
                                      "use NULL (flip) or RRC (random-resized-crop + flip)")
        if aug == "NULL" and (self.H != self.S or self.W != self.S):
            raise ValueError(f"--aug_train NULL feeds the pack's images as they are: the pack is {self.H} x {self.W}, --image_size "
                             f"{self.S}; build the pack at that size or use --aug_train RRC")
        if aug != "RRC" and (self.S > self.H or self.S > self.W):
            raise ValueError(f"the {self.S} x {self.S} window does not fit the pack's {self.H} x {self.W} images")
        self.seed, self.rank, self.world, self.epoch = int(seed), int(rank), int(world), 0
        self.device = torch.device(device)
        self.dtype, self.channels_last = dtype, channels_last
        nbytes = self.memmap.size
        if data_device is None:
            if self.device.type == "cuda":
                free, _total = torch.cuda.mem_get_info(self.device)
                data_device = "gpu" if nbytes <= GPU_SHARE * free else "host"
            else:
                data_device = "gpu"
        if data_device not in ("gpu", "host"):
            raise ValueError(f"data_device must be 'gpu' or 'host', got {data_device!r}")
        self.data_device = data_device
        self.labels = torch.from_numpy(labels).to(self.device)
        self.lut = ops.input_lut(self.meta["mean"], self.meta["std"], self.device)
        if data_device == "gpu":
            self.resident = torch.from_numpy(np.array(self.memmap)).to(self.device)
        else:
            pin = self.device.type == "cuda"
            self._stage = [torch.empty((self.B, self.H, self.W, 3), dtype=torch.uint8, pin_memory=pin) for _ in range(2)]
            self._landed = [torch.empty((self.B, self.H, self.W, 3), dtype=torch.uint8, device=self.device) for _ in range(2)]
            self._copied = [None, None]
        self._indices = epoch_indices(self.N, self.world, self.rank, 0, self.seed, aug is not None)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        self._indices = epoch_indices(self.N, self.world, self.rank, self.epoch, self.seed, self.aug is not None)

    def __len__(self):
        return math.ceil(len(self._indices) / self.B)

    def _images(self, step, ids, flip, box):
        kw = dict(flip=flip, box=box, resample=box is not None, dtype=self.dtype, channels_last=self.channels_last)
        if self.data_device == "gpu":
            return self.input_batch(self.resident, self.lut, self.S, idx=ids.to(self.device), **kw)
        k, n = step % 2, len(ids)
        if self._copied[k] is not None:
            self._copied[k].synchronize()                         # the copy that last read this pinned buffer has finished
        rows = ids.numpy()
        order = np.argsort(rows, kind="stable")                   # (ascending file offsets; written back in the batch's order)
        stage = self._stage[k].numpy()
        stage[order] = self.memmap[rows[order]]
        self._landed[k][:n].copy_(self._stage[k][:n], non_blocking=True)
        if self.device.type == "cuda":
            self._copied[k] = torch.cuda.Event()
            self._copied[k].record()
        return self.input_batch(self._landed[k], self.lut, self.S, idx=None, batch=n, **kw)

    def _batches(self):
        g = torch.Generator().manual_seed(_rng_seed(self.seed, self.rank, self.epoch))
        ids_all = self._indices
        for step, i0 in enumerate(range(0, len(ids_all), self.B)):
            ids = ids_all[i0:i0 + self.B]
            n = len(ids)
            flip = box = None
            if self.aug is not None:
                flip = (torch.rand(n, generator=g) < 0.5).to(torch.uint8).to(self.device)
            if self.aug == "RRC":
                u = torch.rand(n, 10, 4, generator=g, dtype=torch.float64)
                box = rrc_boxes(self.H, self.W, self.crop, u).to(self.device)
            yield ids, self._images(step, ids, flip, box)

    def __iter__(self):
        for ids, images in self._batches():
            yield images, self.labels[ids.to(self.device)]


class PackSampleLoader(PackLoader):
    """Sample mode for `--distill crd` (reference dataset/dataset.py:89-151): (images, labels, index, contrast_idx); `index` is the
    sample's row in the split, contrast_idx [B, nce_k + 1] follows dataset/contrast.py on the pack's own labels."""

    def __init__(self, pack, split, batch_size, image_size, nce_k, mode="exact", **kw):
        super().__init__(pack, split, batch_size, image_size, **kw)
        if mode not in ("exact", "relax"):
            raise ValueError(f"mode must be 'exact' or 'relax', got {mode!r}")
        self.nce_k, self.mode, self.n_data = int(nce_k), mode, self.N
        order, counts, starts = class_segments(self.labels.cpu(), self.meta["n_cls"])
        if mode == "exact" and int(counts.max()) >= self.N:
            raise ValueError("mode 'exact' needs samples of at least two classes")
        self.order, self.counts, self.starts = order.to(self.device), counts.to(self.device), starts.to(self.device)

    def __iter__(self):
        gen = torch.Generator(device=self.device).manual_seed(_rng_seed(self.seed, self.rank, self.epoch) + 1)
        for ids, images in self._batches():
            index = ids.to(self.device)
            labels = self.labels[index]
            yield images, labels, index, contrast_indices(index, labels, self.order, self.counts, self.starts, self.n_data,
                                                          self.nce_k, self.mode, gen, self.device)


# ---- the trainers' side -----------------------------------------------------------------------------------------------------------
def add_arguments(p):
    """the flags both CLIs share"""
    p.add_argument("--data_pack", type=str, default=None,
                   help="directory written by `python -m moma_amd.dataset.make_pack`: train on its images instead of the synthetic set")
    p.add_argument("--data_device", default=None, choices=["gpu", "host"],
                   help="where a pack's uint8 rows live: gpu = resident on the device, host = memmap -> pinned staging -> asynchronous "
                        "copy per batch (default: gpu when the split takes at most a quarter of the free device memory)")
    p.add_argument("--input_dtype", default="fp32", choices=["fp32", "bf16"],
                   help="dtype of the image batches of a pack; bf16 only together with --amp bf16")


def prepare(opt, size):
    """Check the options against the pack before anything is built; returns its meta.  Sets opt.n_data for --distill crd."""
    meta = read_meta(opt.data_pack)
    if opt.aug_train == "RA":
        raise NotImplementedError("--aug_train RA (RandAugment) is not built for --data_pack: use --aug_train NULL (flip) or RRC "
                                  "(random-resized-crop + flip)")
    if meta["n_cls"] != opt.n_cls:
        raise ValueError(f"--n_cls {opt.n_cls}, but {opt.data_pack} has {meta['n_cls']} classes ({', '.join(meta['classes'])})")
    if opt.aug_train == "NULL" and (meta["H"] != size or meta["W"] != size):
        raise ValueError(f"--aug_train NULL feeds the pack's images as they are: the pack is {meta['H']} x {meta['W']}, the image size "
                         f"{size}; build the pack at that size or use --aug_train RRC")
    if size > meta["H"] or size > meta["W"]:
        raise ValueError(f"validation takes the centred {size} x {size} window: the pack's images are {meta['H']} x {meta['W']}")
    if opt.input_dtype == "bf16" and opt.amp != "bf16":
        raise ValueError("--input_dtype bf16 needs --amp bf16")
    if getattr(opt, "distill", None) == "crd":
        opt.n_data = int(meta["splits"]["train"])
    return meta


def build_loaders(opt, size, device, sample=False):
    """(train, val, test) loaders of opt.data_pack; test is val where the pack has no test split.  len(train) replaces
    opt.steps_per_epoch."""
    world = getattr(opt, "world_size", 1) if opt.multiprocessing_distributed else 1
    kw = dict(device=device, data_device=opt.data_device, channels_last=bool(opt.channels_last),
              dtype=torch.bfloat16 if opt.input_dtype == "bf16" and opt.amp == "bf16" else torch.float32)
    tkw = dict(aug=opt.aug_train, crop=opt.crop, seed=opt.seed or 0, rank=opt.rank if world > 1 else 0, world=world, **kw)
    if sample:
        train = PackSampleLoader(opt.data_pack, "train", opt.batch_size, size, opt.nce_k, opt.mode, **tkw)
    else:
        train = PackLoader(opt.data_pack, "train", opt.batch_size, size, **tkw)
    val = PackLoader(opt.data_pack, "val", opt.batch_size, size, **kw)
    test = PackLoader(opt.data_pack, "test", opt.batch_size, size, **kw) if "test" in train.meta["splits"] else val
    opt.steps_per_epoch = len(train)
    return train, val, test
