"""The negatives of a sample-mode batch (`--distill crd`; reference dataset/dataset.py:89-151, `is_sample=True`): ONE rule for the
synthetic set (dataset/synthetic.py) and for a data pack (dataset/pack.py), drawn with whole-batch tensor operations on the device
of the generator."""
import torch


def class_segments(sample_labels, n_cls):
    """(order, counts, starts) of a set's labels: the sample ids grouped by class, the classes' sizes, and where each class's
    segment of `order` begins -- what `contrast_indices` walks in mode 'exact'."""
    counts = torch.bincount(sample_labels, minlength=n_cls)
    order = torch.argsort(sample_labels, stable=True)
    return order, counts, torch.cumsum(counts, 0) - counts


def contrast_indices(index, labels, order, counts, starts, n_data, nce_k, mode, gen, device):
    """contrast_idx [B, nce_k + 1] int64: column 0 = `index`, then nce_k draws with replacement from the samples of the OTHER
    classes (mode 'exact') or from all OTHER samples (mode 'relax').  One torch.rand(B, nce_k) of `gen` per call."""
    B = index.shape[0]
    u = torch.rand(B, nce_k, device=device, generator=gen, dtype=torch.float64)
    if mode == "exact":
        cnt, start = counts[labels].unsqueeze(1), starts[labels].unsqueeze(1)
        r = (u * (n_data - cnt)).long().clamp_(max=n_data - 1)
        r = torch.minimum(r, n_data - cnt - 1)
        neg = order[torch.where(r < start, r, r + cnt)]                      # skip the segment of the sample's own class
    else:
        r = (u * (n_data - 1)).long().clamp_(max=n_data - 2)
        neg = torch.where(r < index.unsqueeze(1), r, r + 1)                  # skip the sample itself
    return torch.cat([index.unsqueeze(1), neg], dim=1)
