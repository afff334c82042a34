"""The definition of ``dvg_grbm_fields_packed`` ("DVG fields v1", include/dvg.h) and of ``sampler.PseudoLikelihood`` in numpy -- a
helper of the fields tests, not a test.

The rows unpacked with ``trace_oracle.unpack``; ``hs`` / ``Js`` the float32 fields of ``oracle.gibbs.scaled_fields``; the CSR of
``oracle.gibbs.build_csr``; the local field by the float32 loop of ``oracle.gibbs.gibbs_sweeps`` (start from ``hs_i``, add ``+-Js``
per CSR entry in row order, every sum rounded to float32); ``z = clamp(rn(two_beta f), -87, 87)``; then float64 numpy for
``nlp = max(s z, 0) + log1p(exp(-|z|))`` and ``m = -sign(z) (1 - e) / (1 + e)``, ``e = exp(-|z|)``."""
from collections import namedtuple

import numpy as np

import trace_oracle
from oracle import gibbs

f32 = np.float32
U = 2.0 ** -53
Fields = namedtuple("Fields", "f z s nlp m log_pl unstable cond_sum cond_pair S")


def local_fields(s, hs, Js, adj_ptr, adj_idx, adj_eid):
    """(T, n) float32: the sampler's local field of every spin of every +-1 row (T, n)."""
    T, n = s.shape
    f = np.empty((T, n), dtype=f32)
    for i in range(n):
        fi = np.full(T, hs[i], dtype=f32)
        for q in range(adj_ptr[i], adj_ptr[i + 1]):
            w = Js[adj_eid[q]]
            fi = (fi + np.where(s[:, adj_idx[q]] > 0, w, -w).astype(f32)).astype(f32)
        f[:, i] = fi
    return f


def pooled(x):
    """The sum over the rows (axis 0) accumulated in extended precision and rounded to float64 once: numpy adds the rows of a
    matrix one after another, and on rows that repeat (a frozen chain) such a chain of T float64 additions gathers an error of
    order T^2 u / 2 of its own -- more than the bound the device is held to."""
    return np.sum(np.asarray(x, np.float64), axis=0, dtype=np.longdouble).astype(np.float64)


def fields(bits, n, hs, Js, edge_i, edge_j, beta):
    """Everything the entry returns for packed rows (..., W), the rows flattened to T: ``f`` (T, n) float32, ``z`` float32,
    ``s`` int8, ``nlp`` and ``m`` (T, n) float64, ``log_pl`` (T,) float64, ``unstable`` (T,) int32, ``cond_sum`` (n,),
    ``cond_pair`` (E,) float64, and ``S`` (T,) = sum_i nlp, the scale of log_pl's bound."""
    hs, Js = np.asarray(hs), np.asarray(Js)
    assert hs.dtype == f32 and Js.dtype == f32 and hs.shape == (n,)
    bits = np.asarray(bits)
    bits = bits.view(np.uint32) if bits.dtype == np.int32 else bits
    s = trace_oracle.unpack(bits.reshape(-1, bits.shape[-1]), n)
    ei, ej = np.asarray(edge_i, dtype=np.int64), np.asarray(edge_j, dtype=np.int64)
    adj_ptr, adj_idx, adj_eid = gibbs.build_csr(n, ei, ej)
    f = local_fields(s, hs, Js, adj_ptr, adj_idx, adj_eid)
    two_beta = f32(f32(2.0) * f32(beta))
    z = np.minimum(np.maximum((two_beta * f).astype(f32), -gibbs.Z_CLAMP), gibbs.Z_CLAMP)
    zd, sd = z.astype(np.float64), s.astype(np.float64)
    a = sd * zd
    e = np.exp(-np.abs(zd))
    nlp = np.maximum(a, 0.0) + np.log1p(e)
    m = -np.sign(zd) * (1.0 - e) / (1.0 + e)
    unstable = ((s.astype(f32) * f) > 0).sum(axis=1).astype(np.int32)
    cond_sum = pooled(m)
    cond_pair = pooled(m[:, ei] * sd[:, ej] + m[:, ej] * sd[:, ei])
    S = nlp.sum(axis=1)
    return Fields(f, z, s, nlp, m, -S, unstable, cond_sum, cond_pair, S)


def bound_log_pl(n, S):
    """(2 n + 16) u S: two orderings of n positive addends, and twice the budget of an exp and a log1p good to 2 ulp each."""
    return (2.0 * n + 16.0) * U * np.asarray(S)


def bound_cond_sum(T):
    return 10.0 * T * U


def bound_cond_pair(T):
    return 20.0 * T * U


# ------------------------------------------------------------------------------------------------ sampler.PseudoLikelihood
def estimates(log_pl, unstable, cond_sum, cond_pair, spin_sum, pair_sum):
    """Every property of ``PseudoLikelihood`` by name, float64 numpy; ``log_pl`` (T,) or (C, M)."""
    log_pl = np.asarray(log_pl, np.float64)
    T, n = log_pl.size, len(cond_sum)
    x = log_pl.mean(axis=1) if log_pl.ndim == 2 else log_pl
    return dict(mean=log_pl.mean(), per_spin=log_pl.mean() / n,
                std_err=x.std(ddof=1) / np.sqrt(len(x)) if len(x) > 1 else np.float64("nan"),
                local_minimum_share=(np.asarray(unstable) == 0).mean(),
                mean_spin=np.asarray(cond_sum, np.float64) / T, mean_pair=np.asarray(cond_pair, np.float64) / (2.0 * T),
                residual_linear=np.asarray(spin_sum, np.float64) - cond_sum,
                residual_quadratic=2.0 * np.asarray(pair_sum, np.float64) - cond_pair)


def enumerate_states(n):
    """All 2^n states as (2^n, n) int8 +-1."""
    return (((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1) * 2 - 1).astype(np.int8)


def boltzmann(s, hs, Js, edge_i, edge_j, beta):
    """p(s) over the given states under exp(-beta E), float64."""
    sd = s.astype(np.float64)
    E = sd @ np.asarray(hs, np.float64) + (sd[:, np.asarray(edge_i)] * sd[:, np.asarray(edge_j)]) @ np.asarray(Js, np.float64)
    a = -np.float64(beta) * E
    p = np.exp(a - a.max())
    return p / p.sum()
