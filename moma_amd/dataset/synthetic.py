"""Synthetic loader: yields `(images fp32 [B,3,S,S], labels int64 [B])` like the reference's
DatasetSerial.__getitem__ batches (dataset/dataset.py:27-44).  The real loaders need author-local folders /
network downloads (out of scope); benchmarks and smoke runs use this one.  Batches are
pre-generated on the target device so the loader never sits in the timed region."""
import torch

from .contrast import contrast_indices


class SyntheticLoader:
    def __init__(self, n_batches, batch_size, image_size, n_cls, seed=12345, device="cpu", distinct=2,
                 last_batch=None):
        g = torch.Generator().manual_seed(seed)
        self.n_batches = n_batches
        self.last_batch = last_batch            # optional smaller final batch (drop_last=False behaviour)
        self.images = [torch.randn(batch_size, 3, image_size, image_size, generator=g).to(device)
                       for _ in range(distinct)]
        self.labels = [torch.randint(0, n_cls, (batch_size,), generator=g).to(device) for _ in range(distinct)]

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        for i in range(self.n_batches):
            x, y = self.images[i % len(self.images)], self.labels[i % len(self.labels)]
            if self.last_batch and i == self.n_batches - 1:
                x, y = x[:self.last_batch], y[:self.last_batch]
            yield x, y


class SyntheticSampleLoader:
    """Synthetic counterpart of the reference's sample-mode datasets (dataset/histo_dataset.py:60-117, `is_sample=True`): yields
    `(images, labels, index, contrast_idx)` for `--distill crd`.

    The set has `n_data` samples (default n_batches * batch_size), each with a fixed class label.  `index` [B] int64 walks a seeded
    permutation of range(n_data), so it is distinct inside a batch; `contrast_idx` [B, nce_k + 1] int64 has column 0 = `index` and
    nce_k draws with replacement from the samples of the OTHER classes (mode 'exact') or from all OTHER samples (mode 'relax').
    Everything is drawn on `device` from a seeded generator with whole-batch tensor operations: no host loop over the batch."""

    def __init__(self, n_batches, batch_size, image_size, n_cls, nce_k, mode="exact", seed=12345, device="cpu", distinct=2,
                 n_data=None):
        if mode not in ("exact", "relax"):
            raise ValueError(f"mode must be 'exact' or 'relax', got {mode!r}")
        g = torch.Generator().manual_seed(seed)
        self.n_batches, self.batch_size, self.nce_k, self.mode = n_batches, batch_size, int(nce_k), mode
        self.n_data = int(n_data) if n_data is not None else n_batches * batch_size
        if self.n_data < max(batch_size, 2):
            raise ValueError(f"n_data {self.n_data} is smaller than one batch ({batch_size}): index could not be distinct inside it")
        self.device = torch.device(device)
        self.images = [torch.randn(batch_size, 3, image_size, image_size, generator=g).to(device) for _ in range(distinct)]
        sample_labels = torch.randint(0, n_cls, (self.n_data,), generator=g)
        perm = torch.randperm(self.n_data, generator=g)
        counts = torch.bincount(sample_labels, minlength=n_cls)
        if mode == "exact" and int(counts.max()) >= self.n_data:
            raise ValueError("mode 'exact' needs samples of at least two classes")
        self.sample_labels = sample_labels.to(device)
        self.perm = perm.to(device)
        self.order = torch.argsort(sample_labels, stable=True).to(device)       # sample ids grouped by class
        self.counts = counts.to(device)
        self.starts = (torch.cumsum(counts, 0) - counts).to(device)
        self.gen = torch.Generator(device=self.device).manual_seed(seed + 1)

    def __len__(self):
        return self.n_batches

    def _contrast_idx(self, index, labels):
        return contrast_indices(index, labels, self.order, self.counts, self.starts, self.n_data, self.nce_k, self.mode, self.gen,
                                self.device)

    def __iter__(self):
        B = self.batch_size
        for i in range(self.n_batches):
            pos = (torch.arange(B, device=self.device) + i * B) % self.n_data
            index = self.perm[pos]
            labels = self.sample_labels[index]
            yield self.images[i % len(self.images)], labels, index, self._contrast_idx(index, labels)
