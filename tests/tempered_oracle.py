"""The definition of the exchange draw ("DVG PT v1", ``dvg_gibbs_sample_tempered`` in include/dvg.h) on top of the unchanged
oracle -- a helper of the tempered tests, not a test.

Chains come in ladders of R consecutive chains; a chain sweeps at the beta of the rung it holds: per sweep ``cref.gibbs_sweeps``
is called once per distinct beta, on the chains holding it (that beta, ``sweep0 + k``, one sweep).  The energy of a chain is
AIS v1's (``ais_oracle``): the start addends 1/2 s_i (hs_i + f_i), then -- the colour classes walked in order on the mixed
state -- (s_new - s_old) f_i per update, f the float32 CSR-order field.  After sweep t with (t + 1) % swap_every == 0,
exchange x = (t + 1) / swap_every: the pairs of rungs (r, r + 1), r = x & 1, (x & 1) + 2, ..., of every ladder change hands iff
d >= 0 or u < exp(d), d = (beta_{r+1} - beta_r) (E_b - E_a) in float64, u from philox(ctr = (r, id of the ladder's first chain,
x, 4), key = seed).  Everything but the fields is float64."""
from collections import namedtuple

import numpy as np

from ais_oracle import fields
from oracle import cref

f32, f64 = np.float32, np.float64
STREAM_SWAP = 4

# by chain: spins (C, n) int8, rungs (C,) int32, energy (C,), A (C,);  by rung: samples (C, n) int8, energy_by_rung (C,);
# accepted (Q, R) uint32 (element R - 1 of a ladder: 0); attempts (R - 1,): the exchanges that had the pair (r, r + 1);
# N = n (S + 2); coins: one (|u - exp(d)|, bound of the decision's error, accepted) per decision with d < 0
Tempered = namedtuple("Tempered", "spins rungs energy A samples energy_by_rung accepted attempts N coins")


def attempts(R, sweep0, n_sweeps, swap_every):
    """How many exchanges of sweeps sweep0 .. sweep0 + n_sweeps - 1 have the pair (r, r + 1), r = 0 .. R - 2."""
    out = np.zeros(R - 1, dtype=np.int64)
    for t in range(sweep0, sweep0 + n_sweeps):
        if (t + 1) % swap_every == 0:
            out[((t + 1) // swap_every) & 1::2] += 1
    return out


def tempered(plan, hs, Js, ladder, ids, seed, sweep0, n_sweeps, swap_every, start=None, rungs=None, flip_sign=False):
    """``ladder``: (R,) betas; ``ids``: the Q R chain ids, ladder q = chains q R .. q R + R - 1; ``start`` (C, n) int8 with
    ``rungs`` (C,), or neither: fresh chains from the INIT stream at ``sweep0``, chain c on rung c % R.  ``flip_sign``: the
    rule with the sign of d flipped -- NOT the definition; the sampling test shows with it that it would notice."""
    ids = np.asarray(ids, dtype=np.uint32)
    ladder = np.asarray(ladder, dtype=f32)
    R, C, n, S = ladder.size, ids.size, plan.n, int(n_sweeps)
    assert C % R == 0 and (start is None) == (rungs is None)
    Q = C // R
    hs, Js = np.asarray(hs, dtype=f32), np.asarray(Js, dtype=f32)
    order, class_ptr = np.asarray(plan.order), np.asarray(plan.class_ptr)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    st = cref.init_state(ids, n, seed, sweep0) if start is None else np.array(start, dtype=np.int8, copy=True)
    rung = (np.arange(C) % R).astype(np.int32) if rungs is None else np.array(rungs, dtype=np.int32, copy=True)
    N = n * (S + 2)
    unit = 4.0 * N * 2.0 ** -53

    add0 = 0.5 * st.astype(f64) * (hs.astype(f64)[None, :] + fields(st, np.arange(n), hs, Js, plan).astype(f64))
    energy, A = add0.sum(axis=1), np.abs(add0).sum(axis=1)
    accepted = np.zeros((Q, R), dtype=np.uint32)
    coins = []
    for t in range(sweep0, sweep0 + S):
        beta = ladder[rung]
        new = np.empty_like(st)
        for b in np.unique(beta):
            sel = np.flatnonzero(beta == b)
            new[sel] = cref.gibbs_sweeps(st[sel], ids[sel], hs, Js, float(b), plan.order, plan.class_ptr, plan.adj_ptr,
                                         plan.adj_idx, plan.adj_eid, seed, t, 1)
        cur = st.copy()
        for c in range(class_ptr.size - 1):
            sp = order[class_ptr[c]:class_ptr[c + 1]].astype(np.int64)
            f = fields(cur, sp, hs, Js, plan)
            d = ((new[:, sp].astype(f32) - cur[:, sp].astype(f32)) * f).astype(f32).astype(f64)  # (+-2 f or 0: exact)
            energy = energy + d.sum(axis=1)
            A = A + np.abs(d).sum(axis=1)
            cur[:, sp] = new[:, sp]
        assert np.array_equal(cur, new)
        st = new
        if (t + 1) % swap_every:
            continue
        x = (t + 1) // swap_every
        for q in range(Q):
            holder = np.empty(R, dtype=np.int64)  # the chain of the ladder that holds rung r
            holder[rung[q * R:(q + 1) * R]] = np.arange(q * R, (q + 1) * R)
            for r in range(x & 1, R - 1, 2):
                a, b = holder[r], holder[r + 1]
                db = f64(ladder[r + 1]) - f64(ladder[r])
                d = db * (energy[b] - energy[a])
                if flip_sign:
                    d = -d
                accept = d >= 0
                if not accept:
                    word = cref.philox([r, int(ids[q * R]), x & 0xFFFFFFFF, STREAM_SWAP], key)[0]
                    u = f64(int(word) >> 8) * 2.0 ** -24
                    ed = np.exp(d)
                    accept = u < ed
                    coins.append((abs(u - ed), unit * abs(db) * (A[a] + A[b]) * ed, bool(accept)))
                if accept:
                    rung[a], rung[b] = r + 1, r
                    accepted[q, r] += 1
    by_rung = (np.arange(C) // R) * R + rung
    samples, energy_by_rung = np.empty_like(st), np.empty_like(energy)
    samples[by_rung], energy_by_rung[by_rung] = st, energy
    return Tempered(st, rung, energy, A, samples, energy_by_rung, accepted, attempts(R, sweep0, S, swap_every), N, coins)


def boltzmann_energy_moments(n, hs, Js, edge_i, edge_j, beta):
    """(mean, standard deviation) of E(s) = hs.s + sum_e Js_e s_i s_j under exp(-beta E) over all 2^n states, float64."""
    s = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(f64) * 2.0 - 1.0
    E = s @ np.asarray(hs, dtype=f64) + (s[:, edge_i] * s[:, edge_j]) @ np.asarray(Js, dtype=f64)
    a = -f64(beta) * E
    w = np.exp(a - a.max())
    w /= w.sum()
    mean = (w * E).sum()
    return mean, np.sqrt((w * (E - mean) ** 2).sum())
