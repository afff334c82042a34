"""The definition of ``dvg_packed_overlap`` ("DVG overlap v1", include/dvg.h) in numpy -- a helper of the overlap tests, not
a test.  Rows are unpacked with ``trace_oracle.unpack`` (bits of spins >= n dropped); per group the int64 Gram matrix G of the
+-1 rows gives the Hamming distances d = (n - G) / 2, ``np.bincount`` their histogram and ``argmin`` -- which takes the first
minimum -- every row's nearest partner.  In self mode the histogram counts r < r' and the diagonal is set above n before the
minimum is taken.  The estimators of ``sampler.Overlap`` are restated next to it."""
import numpy as np

import trace_oracle


def _groups(bits, n):
    """(rows, W) or (C, M, W) packed -> (groups, rows, n) int64 spins: a 3-D set is M groups of C rows."""
    bits = np.asarray(bits)
    s = trace_oracle.unpack(bits.view(np.uint32) if bits.dtype == np.int32 else bits, n).astype(np.int64)
    return s[None] if s.ndim == 2 else s.transpose(1, 0, 2)


def overlap(a, b, n):
    """``(hist (n + 1,) int64, nearest (groups, rows_a) int64)`` of packed ``a`` against packed ``b`` (None: self mode;
    2-D with a 3-D ``a``: shared by every group).  ``nearest`` holds d_min 2^32 + r_min, or -1 without a partner."""
    A = _groups(a, n)
    B = None if b is None else _groups(b, n)
    if B is not None and B.shape[0] == 1 and A.shape[0] > 1:
        B = np.broadcast_to(B, (A.shape[0],) + B.shape[1:])
    hist = np.zeros(n + 1, dtype=np.int64)
    nearest = np.full(A.shape[:2], -1, dtype=np.int64)
    for g in range(A.shape[0]):
        other = A[g] if B is None else B[g]
        d = (n - A[g] @ other.T) // 2
        assert ((n - A[g] @ other.T) % 2 == 0).all() and d.min() >= 0 and d.max() <= n
        if B is None:
            hist += np.bincount(d[np.triu_indices(d.shape[0], 1)], minlength=n + 1)
            if d.shape[0] == 1:
                continue
            d = d.copy()
            np.fill_diagonal(d, n + 1)
        else:
            hist += np.bincount(d.reshape(-1), minlength=n + 1)
        r_min = d.argmin(axis=1)
        nearest[g] = (d[np.arange(d.shape[0]), r_min] << 32) + r_min
    return hist, nearest


def split(nearest):
    """The int64 elements as ``(dist, row)`` int32, -1 where there is no partner."""
    nearest = np.asarray(nearest)
    none = nearest < 0
    return (np.where(none, -1, nearest >> 32).astype(np.int32), np.where(none, -1, nearest & 0xFFFFFFFF).astype(np.int32))


# ---------------------------------------------------------------------------------------------------- the estimators
def q_grid(n):
    return 1.0 - 2.0 * np.arange(n + 1, dtype=np.float64) / n


def pairs(hist):
    return np.asarray(hist, dtype=np.float64).sum()


def mean(hist, f):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.asarray(hist, dtype=np.float64) * f).sum() / pairs(hist)


def density(hist):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(hist, dtype=np.float64) / pairs(hist)


def estimates(hist, n):
    """Every scalar property of ``sampler.Overlap`` as a dict of float64."""
    q = q_grid(n)
    q2, q4 = mean(hist, q ** 2), mean(hist, q ** 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        binder = (3.0 - q4 / q2 ** 2) / 2.0
    return dict(pairs=pairs(hist), mean_q=mean(hist, q), mean_abs_q=mean(hist, np.abs(q)), q2=q2, q4=q4, binder=binder,
                hamming_mean=mean(hist, np.arange(n + 1, dtype=np.float64)))


def mass(hist, n, lo, hi):
    aq = np.abs(q_grid(n))
    return mean(hist, ((aq >= lo) & (aq <= hi)).astype(np.float64))
