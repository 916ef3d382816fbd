"""Golden fixtures as a set of small archives: ``<name>.<i>.npz`` parts of at most PART_BYTES each (the
repository keeps every file under 1 MiB).  An array whose own archive entry would not fit a part is stored as
flat chunks ``<key>//<j>`` with its shape in ``<key>//shape``.  ``load_fixture`` reads a part set (or a single
``<name>.npz``) back as one mapping with the arrays' original keys, shapes and dtypes; entries load lazily."""
import glob
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 900 * 1024
CHUNK_BYTES = 256 * 1024      # raw bytes per chunk of a split array
SEP = "//"


def _packed_size(key, a):
    buf = io.BytesIO()
    np.savez_compressed(buf, **{key: a})
    return len(buf.getvalue())


def save_fixture(name, arrays, folder=HERE):
    """Write ``arrays`` (key -> array) as <folder>/<name>.<i>.npz parts; replaces an earlier set."""
    entries = []
    for k, a in arrays.items():
        a = np.asarray(a)
        assert SEP not in k, k
        if a.nbytes > CHUNK_BYTES and a.dtype.kind in "fiub":
            flat = a.reshape(-1)
            per = max(1, CHUNK_BYTES // a.dtype.itemsize)
            entries.append((k + SEP + "shape", np.asarray(a.shape, dtype=np.int64)))
            entries += [(f"{k}{SEP}{j}", flat[o:o + per]) for j, o in enumerate(range(0, flat.size, per))]
        else:
            entries.append((k, a))
    for old in glob.glob(os.path.join(folder, name + ".*.npz")) + glob.glob(os.path.join(folder, name + ".npz")):
        os.remove(old)
    parts, cur, size = [], {}, 0
    for k, a in entries:
        n = _packed_size(k, a)
        assert n <= PART_BYTES, (k, n)
        if cur and size + n > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += n
    parts.append(cur)
    for i, p in enumerate(parts):
        np.savez_compressed(os.path.join(folder, f"{name}.{i}.npz"), **p)
    return len(parts)


class Fixture:
    """Read-only mapping over the parts of one fixture (``files``, ``[key]``, ``in``, iteration over keys)."""

    def __init__(self, paths):
        self._where, self._chunks = {}, {}
        for p in paths:
            z = np.load(p, allow_pickle=False)
            for k in z.files:
                if SEP in k:
                    base, tail = k.rsplit(SEP, 1)
                    self._chunks.setdefault(base, {})[tail] = z
                else:
                    self._where[k] = z
        self.files = sorted(set(self._where) | set(self._chunks))

    def __getitem__(self, key):
        if key in self._where:
            return self._where[key][key]
        ch = self._chunks[key]
        n = len(ch) - 1
        flat = np.concatenate([ch[str(j)][f"{key}{SEP}{j}"] for j in range(n)])
        return flat.reshape(tuple(ch["shape"][key + SEP + "shape"]))

    def __contains__(self, key):
        return key in self._where or key in self._chunks

    def __iter__(self):
        return iter(self.files)

    def __len__(self):
        return len(self.files)

    def keys(self):
        return list(self.files)


def load_fixture(name, folder=HERE):
    parts = glob.glob(os.path.join(folder, name + ".*.npz"))
    parts.sort(key=lambda p: int(p.rsplit(".", 2)[1]))
    if not parts:
        parts = [os.path.join(folder, name + ".npz")]
    return Fixture(parts)
