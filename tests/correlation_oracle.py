"""The definition of the full pair-correlation sums of bit-packed rows ("DVG corr v1", include/dvg.h) and of the estimates of
``sampler.Correlations``, in numpy -- a helper of the correlation tests, not a test.  Written from the definitions: rows are
unpacked to +-1 and multiplied as int64 matrices; the estimates are loops and plain array expressions."""
import numpy as np


def unpack(bits, n):
    """(..., W) int32 / uint32 packed rows -> (T, n) int64 +-1, all leading dimensions pooled; bits of spins >= n ignored."""
    words = np.ascontiguousarray(bits).view(np.uint32) if np.asarray(bits).dtype == np.int32 else np.asarray(bits, dtype=np.uint32)
    words = words.reshape(-1, words.shape[-1])
    assert words.shape[1] == (n + 31) // 32
    b = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return 2 * b.reshape(words.shape[0], -1)[:, :n].astype(np.int64) - 1


def sums(bits, n):
    """``(spin_sum (n,), pair_sum (n, n))`` int64 over all rows of ``bits``: sum of s_i, and X^T X."""
    x = unpack(bits, n)
    return x.sum(axis=0), x.T @ x


def estimates(spin_sum, pair_sum, T):
    """The float64 members of ``sampler.Correlations`` that need no graph, by name."""
    n = len(spin_sum)
    m = np.asarray(spin_sum, dtype=np.float64) / T
    P = np.asarray(pair_sum, dtype=np.float64) / T
    C = P - np.outer(m, m)
    with np.errstate(invalid="ignore", divide="ignore"):
        pearson = C / np.sqrt(np.outer(np.diag(C), np.diag(C)))
    return dict(mean_spin=m, mean_pair=P, connected=C, pearson=pearson, chi_sg=np.float64((C * C).sum() / n))


def _edge_set(edge_i, edge_j):
    return {(min(int(a), int(b)), max(int(a), int(b))) for a, b in zip(edge_i, edge_j)}


def on_edges(C, edge_i, edge_j):
    return np.array([C[int(a), int(b)] for a, b in zip(edge_i, edge_j)], dtype=np.float64)


def off_edge_share(C, edge_i, edge_j):
    edges, n = _edge_set(edge_i, edge_j), C.shape[0]
    off = sum(C[i, j] ** 2 for i in range(n) for j in range(i + 1, n) if (i, j) not in edges)
    every = sum(C[i, j] ** 2 for i in range(n) for j in range(i + 1, n))
    return np.float64(off / every) if every != 0 else np.float64("nan")


def top_pairs(C, k, edge_i=None, edge_j=None):
    """``(i, j, value)`` of the k pairs i < j of largest |C_ij|, edges excluded when an edge list is given; among equal |C_ij|
    the smaller flat index i n + j first."""
    n = C.shape[0]
    edges = _edge_set(edge_i, edge_j) if edge_i is not None else set()
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if (i, j) not in edges]
    pairs.sort(key=lambda p: (-abs(C[p]), p[0] * n + p[1]))
    pairs = pairs[:k]
    return (np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int64),
            np.array([C[p] for p in pairs], dtype=np.float64))


def gap(a, b, edge_i=None, edge_j=None):
    """``a``, ``b``: ``estimates`` dicts.  Root mean squares of the differences of the means: spins, pairs i < j, and with an
    edge list the listed edges / the pairs i < j that are no edge (NaN over no pairs)."""
    n = len(a["mean_spin"])
    d = a["mean_pair"] - b["mean_pair"]
    rms = lambda v: np.float64(np.sqrt(np.mean(np.square(v)))) if len(v) else np.float64("nan")  # noqa: E731
    res = dict(spin_rms=rms(a["mean_spin"] - b["mean_spin"]), pair_rms=rms([d[i, j] for i in range(n) for j in range(i + 1, n)]))
    if edge_i is not None:
        edges = _edge_set(edge_i, edge_j)
        res["edge_rms"] = rms([d[int(p), int(q)] for p, q in zip(edge_i, edge_j)])
        res["off_edge_rms"] = rms([d[i, j] for i in range(n) for j in range(i + 1, n) if (i, j) not in edges])
    return res
