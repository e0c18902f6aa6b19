"""Restatement, in torch on the CPU, of what the reference does to an image between the file and the backbone, for the data-pack
path (moma_amd/dataset/pack.py, csrc/input.hip).  torchvision is not installed here, so its transforms are written out:

  reference dataset/histo_dataset.py:194-239 (`prostate_hv`; the other branches have the same shape)
      train  Resize(512) . RandomHorizontalFlip . [RandAugment] . ToTensor . Normalize(mean=[0.485,0.456,0.406], std=[0.229,0.224,0.225])
      val    Resize . CenterCrop(image_size) . ToTensor . Normalize
  :1054-1058 (`get_histo_dataloader_448`)   RandomResizedCrop(image_size, scale=(opt.crop, 1.)) + flip in place of the bare flip
  :387-410   loaders: shuffle per epoch, no drop_last; DistributedSampler under --multiprocessing-distributed

  Resize(size)       smaller edge to `size`, the other to int(size * long / short), PIL's Image.BILINEAR (the pack builder's part)
  CenterCrop(S)      offsets int(round((H - S) / 2.0)), int(round((W - S) / 2.0))
  ToTensor           uint8 HWC -> float32 CHW, .div(255)
  Normalize          .sub_(mean[:, None, None]).div_(std[:, None, None]) with float32 mean / std
  RandomResizedCrop  get_params (ten tries, then the centred fallback) -> crop (top, left, h, w) -> resize to S x S, bilinear: on a
                     tensor, half-pixel centres (align_corners=False) without antialiasing: source coordinate (o + 0.5) h / S - 0.5
                     clamped to [0, h - 1], second tap clamped to h - 1; the uint8 result is the value rounded to a level
  DistributedSampler indices = randperm(n, seed + epoch); padded by wrap-around to a multiple of the world size; rank r takes r::W
"""
import math

import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def centre_box(H, W, Sh, Sw):
    return int(round((H - Sh) / 2.0)), int(round((W - Sw) / 2.0))


def window_levels(src, idx, box, Sh, Sw):
    """uint8 [B, Sh, Sw, 3]: source pixel (top + y, left + x) of image idx[b], every read clamped into that image"""
    N, H, W, _ = src.shape
    out = []
    for b, n in enumerate(idx.tolist()):
        top, left = (int(box[b][0]), int(box[b][1])) if box is not None else centre_box(H, W, Sh, Sw)
        rows = (torch.arange(Sh) + top).clamp(0, H - 1)
        cols = (torch.arange(Sw) + left).clamp(0, W - 1)
        out.append(src[n][rows][:, cols])
    return torch.stack(out)


def bilinear_values(src, idx, box, Sh, Sw):
    """float64 [B, Sh, Sw, 3]: the box of image idx[b] resampled onto Sh x Sw, half-pixel centres, before rounding to a level"""
    N, H, W, _ = src.shape
    out = []
    for b, n in enumerate(idx.tolist()):
        top, left, h, w = (int(v) for v in box[b])
        img = src[n].to(torch.float64)

        def taps(S, extent, first, full):
            s = ((torch.arange(S, dtype=torch.float64) + 0.5) * extent / S - 0.5).clamp(0, extent - 1)
            i0 = s.floor().long()
            i1 = (i0 + 1).clamp(max=extent - 1)
            return (i0 + first).clamp(0, full - 1), (i1 + first).clamp(0, full - 1), s - i0
        y0, y1, wy = taps(Sh, h, top, H)
        x0, x1, wx = taps(Sw, w, left, W)
        wy, wx = wy[:, None, None], wx[None, :, None]
        t = img[y0][:, x0] * (1 - wx) + img[y0][:, x1] * wx
        u = img[y1][:, x0] * (1 - wx) + img[y1][:, x1] * wx
        out.append(t * (1 - wy) + u * wy)
    return torch.stack(out)


def to_levels(values):
    """the uint8 result of a resize: floor(v + 0.5)"""
    return torch.floor(values + 0.5).clamp(0, 255).to(torch.uint8)


def near_tie(values, eps=1e-4):
    """where a float64 value lies within eps of a half-integer without being one: the level may differ by one there"""
    d = (values - torch.floor(values) - 0.5).abs()
    return (d < eps) & (d != 0)


def normalize(levels, mean=MEAN, std=STD):
    """ToTensor + Normalize: uint8 [B, S_h, S_w, 3] -> float32 [B, 3, S_h, S_w]"""
    x = levels.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32)[None, :, None, None]
    s = torch.as_tensor(std, dtype=torch.float32)[None, :, None, None]
    return x.sub_(m).div_(s)


def finish(levels, flip, dtype=torch.float32, channels_last=False, mean=MEAN, std=STD):
    """levels uint8 [B, S_h, S_w, 3] -> flip -> ToTensor / Normalize -> dtype -> layout"""
    if flip is not None:
        f = torch.as_tensor(flip).bool()
        levels = torch.where(f[:, None, None, None], levels.flip(2), levels)
    x = normalize(levels, mean, std).to(dtype)
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()


def input_batch(src, lut=None, size=None, idx=None, flip=None, box=None, resample=False, batch=None, dtype=torch.float32,
                channels_last=False, mean=MEAN, std=STD):
    """What ops.input_batch returns (same signature; `lut` is not read: the arithmetic is ToTensor's and Normalize's)."""
    src = src.cpu()
    Sh, Sw = (size, size) if isinstance(size, int) else size
    if idx is None:
        n = batch if batch is not None else (len(flip) if flip is not None else len(box) if box is not None else src.shape[0])
        idx = torch.arange(n)
    idx = torch.as_tensor(idx).cpu()
    box = None if box is None else torch.as_tensor(box).cpu()
    if resample and box is not None:
        levels = to_levels(bilinear_values(src, idx, box, Sh, Sw))
    else:
        levels = window_levels(src, idx, box, Sh, Sw)
    return finish(levels, None if flip is None else torch.as_tensor(flip).cpu(), dtype, channels_last, mean, std)


def torch_chain(resident, idx, flip, top, left, S, mean, std, dtype=torch.float32, channels_last=False, scale=None):
    """The same batch by stock torch operators on the device of `resident` (window mode, one box for the batch): the launches and
    passes ops.input_batch replaces -- index_select, where / flip, slicing, permute, .float(), div, sub, div, the layout, the cast.
    mean, std: float32 [1, 3, 1, 1] on that device; scale: a 0-dim float32 255 there (a TENSOR divisor: by a Python scalar the device
    kernel multiplies by the reciprocal, which is not ToTensor's division)."""
    if scale is None:
        scale = torch.full((), 255.0, device=resident.device)
    x = resident.index_select(0, idx)
    x = x[:, top:top + S, left:left + S]
    x = torch.where(flip[:, None, None, None], x.flip(2), x)
    x = x.permute(0, 3, 1, 2).float().div(scale).sub(mean).div(std)
    x = x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()
    return x.to(dtype)


def sampler_indices(n, world, rank, epoch, seed, shuffle=True):
    """DistributedSampler.__iter__ (world 1: the whole permutation)"""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        indices = torch.randperm(n, generator=g).tolist()
    else:
        indices = list(range(n))
    total = math.ceil(n / world) * world
    pad = total - len(indices)
    if pad <= len(indices):
        indices += indices[:pad]
    else:
        indices += (indices * math.ceil(pad / len(indices)))[:pad]
    return indices[rank:total:world]


def rrc_box(H, W, crop, u, ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCrop.get_params for ONE image, its random draws replaced by the uniforms u [10, 4] (area, log-ratio, top, left):
    uniform(a, b) = a + u (b - a), randint(0, n) = floor(u n).  -> (top, left, h, w)"""
    area = H * W
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for k in range(10):
        target = area * (crop + float(u[k][0]) * (1.0 - crop))
        aspect = math.exp(log_ratio[0] + float(u[k][1]) * (log_ratio[1] - log_ratio[0]))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return min(int(float(u[k][2]) * (H - h + 1)), H - h), min(int(float(u[k][3]) * (W - w + 1)), W - w), h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w
