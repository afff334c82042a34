"""The definition of ``dvg_grbm_energy_packed`` ("DVG energy v1", include/dvg.h) and of ``sampler.EnergySeries`` in numpy float64
-- a helper of the energy tests, not a test.

Energies: the rows unpacked with ``trace_oracle.unpack``, ``hs`` / ``Js`` the float32 fields of ``oracle.gibbs.scaled_fields``
converted to float64 (exactly), ``E = s . hs + sum_e Js_e s_i s_j``.  Every addend is exact; numpy's order of the additions is
its own, so two orderings of N addends whose magnitudes sum to A differ by at most 4 N 2^-53 A (the form ``tests/ais_oracle.py``
uses), and not at all where every partial sum is exact (fields on a dyadic grid)."""
import numpy as np

import trace_oracle


def energies(bits, n, hs, Js, edge_i, edge_j):
    """``(E, A)``: the float64 energies of packed rows (..., W) -> (...), and A = sum |hs| + sum |Js|."""
    hs, Js = np.asarray(hs), np.asarray(Js)
    assert hs.dtype == np.float32 and Js.dtype == np.float32 and hs.shape == (n,)
    bits = np.asarray(bits)
    s = trace_oracle.unpack(bits.view(np.uint32) if bits.dtype == np.int32 else bits, n).astype(np.float64)
    h64, J64 = hs.astype(np.float64), Js.astype(np.float64)
    E = s @ h64 + (s[..., np.asarray(edge_i)] * s[..., np.asarray(edge_j)]) @ J64
    return E, float(np.abs(h64).sum() + np.abs(J64).sum())


def bound(n, n_edges, A):
    """Two orderings of the same n + n_edges exact addends."""
    return 4.0 * (n + n_edges) * 2.0 ** -53 * A


def exact_energy_moments(n, hs, Js, edge_i, edge_j, beta):
    """``(<E>, Var E)`` under exp(-beta E) over all 2^n states, float64."""
    s = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64) * 2.0 - 1.0
    E = s @ np.asarray(hs, np.float64) + (s[:, np.asarray(edge_i)] * s[:, np.asarray(edge_j)]) @ np.asarray(Js, np.float64)
    a = -np.float64(beta) * E
    p = np.exp(a - a.max())
    p /= p.sum()
    mean = p @ E
    return float(mean), float(p @ (E - mean) ** 2)


# ------------------------------------------------------------------------------------------------ the estimators of EnergySeries
def default_max_lag(M):
    return min(M - 1, 512)


def rho(E, max_lag):
    """rho[t] = [sum_c sum_{m < M - t} d(c, m) d(c, m + t) / (C (M - t))] / var around the pooled mean; NaN where var = 0."""
    E = np.asarray(E, np.float64)
    C, M = E.shape
    d = E - E.mean()
    var = (d * d).mean()
    cov = np.array([(d[:, :M - t] * d[:, t:]).sum() / (C * (M - t)) for t in range(max_lag + 1)])
    with np.errstate(invalid="ignore", divide="ignore"):
        return cov / var


def estimates(E, thin=1, max_lag=None, beta=1.0):
    """Every property of ``EnergySeries.from_energies(E, thin, max_lag)`` by name (``r_hat`` left out where C < 2 or M < 2),
    ``heat_capacity`` at ``beta``."""
    E = np.asarray(E, np.float64)
    C, M = E.shape
    L = default_max_lag(M) if max_lag is None else max_lag
    mean = E.mean()
    var = ((E - mean) ** 2).mean()
    chain_mean = E.mean(axis=1)
    r = rho(E, L)
    if np.isnan(r[0]):
        tau = np.float64("nan")
    else:
        tau = np.float64(1.0)
        for t in range(1, L + 1):  # the initial positive sequence
            if not r[t] > 0:
                break
            tau += 2.0 * r[t]
    out = dict(mean=mean, var=var, chain_mean=chain_mean, rho=r, tau_int=tau, truncated=bool(L >= 1 and (r[1:] > 0).all()),
               tau_int_sweeps=tau * thin, ess=np.float64(C * M) / tau, heat_capacity=np.float64(beta) ** 2 * var,
               std_err=chain_mean.std(ddof=1) / np.sqrt(C) if C > 1 else np.float64("nan"))
    if C >= 2 and M >= 2:
        W = E.var(axis=1, ddof=1).mean()
        B = chain_mean.var(ddof=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["r_hat"] = np.sqrt(((M - 1.0) / M * W + B) / W)
    return out
