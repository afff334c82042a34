"""The definition of ``dvg_packed_distinct`` ("DVG distinct v1", include/dvg.h) in numpy -- a helper of the distinct tests, not
a test module.  Mask the pad bits, ``first`` through a dict of row bytes, then ``rep``, ``id``, ``count`` and, for a second
set that is looked up and never inserted, ``other_id`` and ``other_hits``."""
import collections

import numpy as np

Result = collections.namedtuple("Result", "first id rep count other_id other_hits")


def keys(bits, n):
    """(rows, W) uint32: the rows' words with the bits of spins >= n cleared."""
    W = (n + 31) // 32
    b = np.ascontiguousarray(np.asarray(bits).reshape(-1, np.asarray(bits).shape[-1])).view(np.uint32).copy()
    assert b.shape[1] == W, (b.shape, n)
    if n % 32:
        b[:, -1] &= np.uint32((1 << (n % 32)) - 1)
    return b


def distinct(bits, n, other=None):
    """``bits`` (T, W) or (C, M, W) int32 / uint32, pooled under the flattened index; ``other`` (rows, W) or None."""
    k = keys(bits, n)
    T = k.shape[0]
    seen = {}
    first = np.empty(T, dtype=np.int32)
    for t in range(T):
        first[t] = seen.setdefault(k[t].tobytes(), t)
    rep = np.flatnonzero(first == np.arange(T)).astype(np.int32)  # increasing: the order of first occurrence
    cls = np.full(T, -1, dtype=np.int32)
    cls[rep] = np.arange(rep.size, dtype=np.int32)
    ident = cls[first]
    count = np.bincount(ident, minlength=rep.size).astype(np.int64)
    other_id = other_hits = None
    if other is not None:
        ko = keys(other, n)
        other_id = np.array([cls[seen[r.tobytes()]] if r.tobytes() in seen else -1 for r in ko], dtype=np.int32)
        other_hits = np.bincount(other_id[other_id >= 0], minlength=rep.size).astype(np.int64)
    return Result(first, ident, rep, count, other_id, other_hits)


def estimates(count):
    """``sampler.Distinct``'s numbers from the class sizes, float64."""
    c = np.asarray(count, dtype=np.int64)
    T = int(c.sum())
    p = c.astype(np.float64) / T
    singles = int((c == 1).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        collision = np.float64((c * (c - 1)).sum()) / np.float64(T * (T - 1))
    return dict(entropy=float(-(p * np.log(p)).sum()), collision_share=float(collision), unseen_mass=singles / T, singletons=singles)
