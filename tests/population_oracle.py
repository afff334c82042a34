"""The definition of population annealing's resampling step ("DVG PA v1", include/dvg.h) and of the population draw on top
of it, restated in numpy uint64 and Python integers over the unchanged oracle -- a helper of the population tests, not a
test.

``weights`` and ``resample`` are the definition's steps 1 - 6: ``oracle.gibbs.spec_exp`` is the float32 exp (the array
form of ``cref.spec_exp``), ``cref.philox`` the offset's word; the prefix sums and the children's pointers are numpy uint64
-- every term is asserted to stay below 2^53 -- and the offset's 128-bit product is a Python integer.  ``anneal`` is ``GibbsSampler.sample_population``: per temperature step one weighed annealed draw
(``ais_oracle.ais`` with ``start=`` and ``beta_from=``), the populations' log Z increments, one resampling."""
from collections import namedtuple

import numpy as np

import ais_oracle
from oracle import cref, gibbs

f32, f64 = np.float32, np.float64
STREAM_RESAMPLE = 5

Resampled = namedtuple("Resampled", "parents weights K V")
Annealed = namedtuple("Annealed", "state families log_z_populations log_weights parents ess")


def weights(lw):
    """k_c of one population: (R,) uint64 in 0 .. 2^32."""
    lw = np.asarray(lw, dtype=f64)
    with np.errstate(invalid="ignore", over="ignore"):
        z = (lw - lw.max()).astype(f32)  # one float64 subtraction, rounded to the nearest float32
    z = np.minimum(np.maximum(z, f32(-87.0)), f32(0.0))
    w = gibbs.spec_exp(z)  # (the vectorised statement of cref.spec_exp: the host test holds the two together)
    return (w.astype(f64) * 4294967296.0).astype(np.uint64)  # exact scaling; the conversion truncates


def offset(K, seed, first_chain_id, step):
    o = cref.philox([0, int(first_chain_id) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, STREAM_RESAMPLE],
                    [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    r64 = (int(o[0]) << 32) | int(o[1])
    return (r64 * int(K)) >> 64


def resample_one(lw, seed, first_chain_id, step):
    """One population: (parents (R,) local indices, k (R,) uint64, K, V); K and V Python integers."""
    k = weights(lw)
    R = int(k.size)
    S = np.cumsum(k, dtype=np.uint64)  # R <= 2^20 weights of at most 2^32: below 2^53
    K = int(S[-1])
    V = offset(K, seed, first_chain_id, step)
    q, rem = divmod(K, R)
    assert R <= 2 ** 20 and (R - 1) * q < 2 ** 53 and (R - 1) * rem + V < 2 ** 53
    j = np.arange(R, dtype=np.uint64)
    t = j * np.uint64(q) + (j * np.uint64(rem) + np.uint64(V)) // np.uint64(R)
    assert t.dtype == np.uint64 and int(t[-1]) == ((R - 1) * K + V) // R < K
    parents = np.searchsorted(S, t, side="right")  # the smallest c with S_c > t_j
    return parents.astype(np.int64), k, K, V


def resample(lw, P, seed, chain_id0, step):
    """The whole call: ``parents`` (C,) int32 global indices, ``weights`` (C,) uint64, and per population K and V."""
    lw = np.asarray(lw, dtype=f64)
    C = lw.size
    assert C % P == 0
    R = C // P
    parents, ks, Ks, Vs = [], [], [], []
    for p in range(P):
        par, k, K, V = resample_one(lw[p * R:(p + 1) * R], seed, (int(chain_id0) + p * R) & 0xFFFFFFFF, step)
        parents.append(p * R + par)
        ks.append(k)
        Ks.append(K)
        Vs.append(V)
    return Resampled(np.concatenate(parents).astype(np.int32), np.concatenate(ks), Ks, Vs)


def logsumexp(a, axis=-1):
    a = np.asarray(a, dtype=f64)
    m = a.max(axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.exp(a - m).sum(axis=axis))


def step_ess(lw, P):
    """(P,) effective sample sizes (sum w)^2 / sum w^2 of one step's float64 weights."""
    lw = np.asarray(lw, dtype=f64).reshape(P, -1)
    return np.exp(2.0 * logsumexp(lw) - logsumexp(2.0 * lw))


def estimates(n, log_weights, families, P):
    """What ``sampler.Population.from_history`` computes, in numpy: a dict of log_z_populations, log_z, std_err, survivors,
    rho_t, ess."""
    log_weights = np.asarray(log_weights, dtype=f64)
    T, C = log_weights.shape
    R = C // P
    lzp = n * np.log(2.0) + (logsumexp(log_weights.reshape(T, P, R)) - np.log(R)).sum(axis=0)
    log_z = logsumexp(lzp) - np.log(P)
    z = np.exp(lzp - lzp.max())
    std_err = z.std(ddof=1) / z.mean() / np.sqrt(P) if P > 1 else np.nan
    fam = np.asarray(families).reshape(P, R)
    survivors = np.array([np.unique(row).size for row in fam])
    rho_t = np.array([R * ((np.unique(row, return_counts=True)[1] / R) ** 2).sum() for row in fam])
    ess = np.stack([step_ess(log_weights[t], P) for t in range(T)])
    return dict(log_z_populations=lzp, log_z=log_z, std_err=std_err, survivors=survivors, rho_t=rho_t, ess=ess)


def anneal(plan, hs, Js, betas, ids, seed, sweep0, theta, P):
    """The population draw: fresh chains ``ids`` (consecutive), ``theta`` sweeps at each of ``betas`` (T,), resampled after
    every step with ``step = sweep0 + (t + 1) theta``.  Returns ``Annealed``: the final state (C, n) int8, the founders'
    indices, log Z per population, and the histories log_weights (T, C), parents (T, C), ess (T, P)."""
    ids = np.asarray(ids, dtype=np.uint32)
    betas = np.asarray(betas, dtype=f32)
    C, T = ids.size, betas.size
    R = C // P
    state, prev = None, 0.0
    families = np.arange(C, dtype=np.int32)
    log_z = np.full(P, plan.n * np.log(2.0))
    lws, pars, esss = [], [], []
    for t in range(T):
        r = ais_oracle.ais(plan, hs, Js, np.full(theta, betas[t], dtype=f32), ids, seed, sweep0 + t * theta, start=state,
                           beta_from=prev)
        prev = float(betas[t])
        log_z = log_z + logsumexp(r.log_w.reshape(P, R)) - np.log(R)
        res = resample(r.log_w, P, seed, int(ids[0]), sweep0 + (t + 1) * theta)
        state, families = r.spins[res.parents], families[res.parents]
        lws.append(r.log_w)
        pars.append(res.parents)
        esss.append(step_ess(r.log_w, P))
    return Annealed(state, families, log_z, np.stack(lws), np.stack(pars), np.stack(esss))
