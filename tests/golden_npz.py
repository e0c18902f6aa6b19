"""Reading and writing the golden fixtures of tests/golden/.

A fixture whose .npz would exceed the size limit of a committed file (1 MiB) is stored as `<name>.part0.npz`,
`<name>.part1.npz`, ...: consecutive runs of its arrays, each part a compressed .npz below the limit.  `load()` takes the
fixture's logical path (`.../g5_step_trace.npz`) and returns its arrays whichever way they are stored."""
import glob
import os
import zlib

import numpy as np

LIMIT = 1 << 20            # bytes per committed file
_PART_BUDGET = 900 << 10   # estimated compressed bytes per part (zip headers and estimate error stay under LIMIT)


class Fixture(dict):
    """name -> array, with the `.files` of an NpzFile."""

    @property
    def files(self):
        return list(self.keys())


def _parts(path):
    stem = path[:-len(".npz")] if path.endswith(".npz") else path
    return sorted(glob.glob(glob.escape(stem) + ".part*.npz"), key=lambda p: int(p[len(stem) + len(".part"):-len(".npz")]))


def load(path):
    if os.path.exists(path):
        return np.load(path)
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(path)
    out = Fixture()
    for p in parts:
        with np.load(p) as z:
            out.update((k, z[k]) for k in z.files)
    return out


def save(path, arrays):
    """np.savez_compressed(path, **arrays), split into parts when one file would exceed LIMIT."""
    for p in _parts(path):
        os.remove(p)
    np.savez_compressed(path, **arrays)
    if os.path.getsize(path) <= LIMIT:
        return [path]
    os.remove(path)
    groups, cur, size = [], {}, 0
    for k, v in arrays.items():
        est = len(zlib.compress(np.ascontiguousarray(v).tobytes(), 6)) + 512
        if cur and size + est > _PART_BUDGET:
            groups.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += est
    groups.append(cur)
    stem = path[:-len(".npz")]
    written = []
    for i, g in enumerate(groups):
        p = f"{stem}.part{i}.npz"
        np.savez_compressed(p, **g)
        assert os.path.getsize(p) <= LIMIT, (p, os.path.getsize(p))   # one array alone above the limit: store it differently
        written.append(p)
    return written
