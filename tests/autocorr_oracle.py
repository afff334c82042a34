"""The definition of the autocorrelation sums of a bit-packed trace ("DVG acf v1", include/dvg.h) and of the estimators built
on them (``sampler.Autocorrelation``), restated in numpy over ``trace_oracle.unpack`` -- a helper of the autocorrelation
tests, not a test.

Sums: int64 products of the unpacked +-1 spins, one lag at a time.  Estimators: float64, lag by lag and spin by spin where
the product code uses a cumulative product."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trace_oracle  # noqa: E402


def sums_of_spins(s, L):
    """(C, M, n) +-1 -> (lag_sum (L + 1, n) int64, spin_sum (n,) int64, chain_sum (C, n) int32)."""
    s = np.asarray(s, dtype=np.int64)
    C, M, n = s.shape
    assert 0 <= L < M
    lag_sum = np.zeros((L + 1, n), dtype=np.int64)
    for t in range(L + 1):
        lag_sum[t] = (s[:, :M - t] * s[:, t:]).sum(axis=(0, 1))
    return lag_sum, s.sum(axis=(0, 1)), s.sum(axis=1).astype(np.int32)


def lag_sums(bits, n, L):
    """The same from packed records (C, M, W) uint32; bits of spins >= n are ignored."""
    return sums_of_spins(trace_oracle.unpack(np.asarray(bits), n), L)


def counts(C, M, L):
    return np.array([C * (M - t) for t in range(L + 1)], dtype=np.int64)


def mean_spin(spin_sum, C, M):
    return np.asarray(spin_sum, dtype=np.float64) / (C * M)


def rho(lag_sum, spin_sum, C, M):
    lag_sum = np.asarray(lag_sum, dtype=np.float64)
    mu = mean_spin(spin_sum, C, M)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (lag_sum / counts(C, M, lag_sum.shape[0] - 1)[:, None] - mu ** 2) / (1.0 - mu ** 2)


def tau_int(lag_sum, spin_sum, C, M):
    """(tau_int (n,) in records, truncated (n,) bool): 1 + 2 sum of rho over the leading lags 1, 2, .. at which rho > 0."""
    r = rho(lag_sum, spin_sum, C, M)
    L, n = r.shape[0] - 1, r.shape[1]
    tau, truncated = np.empty(n, dtype=np.float64), np.zeros(n, dtype=bool)
    for i in range(n):
        if np.isnan(r[0, i]):
            tau[i] = np.nan
            continue
        acc, t = 0.0, 1
        while t <= L and r[t, i] > 0:
            acc += r[t, i]
            t += 1
        tau[i] = 1.0 + 2.0 * acc
        truncated[i] = L >= 1 and t == L + 1
    return tau, truncated


def ess(lag_sum, spin_sum, C, M):
    with np.errstate(divide="ignore", invalid="ignore"):
        return C * M / tau_int(lag_sum, spin_sum, C, M)[0]


def overlap(lag_sum, C, M):
    lag_sum = np.asarray(lag_sum, dtype=np.int64)
    return lag_sum.sum(axis=1).astype(np.float64) / (lag_sum.shape[1] * counts(C, M, lag_sum.shape[0] - 1))


def r_hat(chain_sum, M):
    """Gelman-Rubin over the chains' means; IEEE division as it falls (inf where Wv == 0 < Bm, NaN where both are 0)."""
    m_c = np.asarray(chain_sum, dtype=np.float64) / M
    C = m_c.shape[0]
    Wv = (1.0 - m_c ** 2).mean(axis=0) * M / (M - 1)
    Bm = ((m_c - m_c.mean(axis=0)) ** 2).sum(axis=0) / (C - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(((M - 1) / M * Wv + Bm) / Wv)
