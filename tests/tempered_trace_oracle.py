"""The definition of the traced exchange draw ("DVG PT trace v1", ``dvg_gibbs_sample_tempered_traced`` in include/dvg.h) on top of
the unchanged oracle -- a helper of the traced tempered tests, not a test.

It is ``tempered_oracle.tempered``'s loop restated (the sweeps by ``cref.gibbs_sweeps`` per distinct beta, the energies walked
class by class, the exchanges), with the three records taken at the defined point: sweep k of the call (0-based) is recorded
iff ``k + 1 > burn_in`` and ``(k + 1 - burn_in) % thin == 0``, AFTER the exchange that follows the sweep if one is due.  A record
holds, BY RUNG, the packed state (``trace_oracle.pack``) and the carried energy of the chain that holds the rung then, and, BY
CHAIN, the rung.  Its non-record outputs equal ``tempered_oracle.tempered``'s exactly (a host test)."""
from collections import namedtuple

import numpy as np

from ais_oracle import fields
from oracle import cref
from tempered_oracle import STREAM_SWAP, Tempered, attempts
from trace_oracle import pack, recorded_sweeps

f32, f64 = np.float32, np.float64

# draw: the ``tempered_oracle.Tempered`` of the same draw;  by rung: bits (Q, R, M, W) uint32, energies (Q, R, M) float64 and A
# (Q, R, M), the absolute sum of the addends each recorded energy has had so far;  by chain: walk (Q, R, M) uint8;
# sweeps (M,) int64, the recorded k + 1
TemperedTrace = namedtuple("TemperedTrace", "draw bits energies A walk sweeps")


def tempered_traced(plan, hs, Js, ladder, ids, seed, sweep0, n_sweeps, swap_every, burn_in=0, thin=1, start=None, rungs=None):
    """The arguments of ``tempered_oracle.tempered`` plus the record rule's ``burn_in`` and ``thin``."""
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
    first = (np.arange(C) // R) * R  # the first chain of each chain's ladder
    sweeps = recorded_sweeps(S, burn_in, thin)
    M, W = sweeps.size, (n + 31) // 32
    assert M == max(0, (S - burn_in) // thin)
    bits = np.zeros((C, M, W), dtype=np.uint32)
    e_rec, a_rec = np.zeros((C, M), dtype=f64), np.zeros((C, M), dtype=f64)
    walk = np.zeros((C, M), dtype=np.uint8)
    m = 0

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
        if (t + 1) % swap_every == 0:
            x = (t + 1) // swap_every
            for q in range(Q):
                holder = np.empty(R, dtype=np.int64)  # the chain of the ladder that holds rung r
                holder[rung[q * R:(q + 1) * R]] = np.arange(q * R, (q + 1) * R)
                for r in range(x & 1, R - 1, 2):
                    a, b = holder[r], holder[r + 1]
                    db = f64(ladder[r + 1]) - f64(ladder[r])
                    d = db * (energy[b] - energy[a])
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
        # the record: behind the exchange, so that it shows who holds each rung as the next sweep finds it
        if m < M and t - sweep0 + 1 == sweeps[m]:
            row = first + rung
            bits[row, m] = pack(st)
            e_rec[row, m], a_rec[row, m] = energy, A
            walk[:, m] = rung
            m += 1
    assert m == M
    by_rung = first + rung
    samples, energy_by_rung = np.empty_like(st), np.empty_like(energy)
    samples[by_rung], energy_by_rung[by_rung] = st, energy
    draw = Tempered(st, rung, energy, A, samples, energy_by_rung, accepted, attempts(R, sweep0, S, swap_every), N, coins)
    return TemperedTrace(draw, bits.reshape(Q, R, M, W), e_rec.reshape(Q, R, M), a_rec.reshape(Q, R, M), walk.reshape(Q, R, M), sweeps)
