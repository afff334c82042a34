"""The definition of the weighed annealed draw ("DVG AIS v1", include/dvg.h) on top of the unchanged oracle -- a helper
of the AIS tests, not a test.

The spins are the annealed draw's: ``cref.gibbs_sweeps`` called once per sweep (that sweep's beta, ``sweep0 + k``, one
sweep) on the chains that share the beta.  Between two sweeps the colour classes are walked in order: the float32
CSR-order fields of the class's spins on the current MIXED state (classes before it already updated) are the fields the
decisions used, so ``(s_new - s_old) f`` is the energy change of each update; then the oracle's new values are applied.
Everything but the fields is float64."""
from collections import namedtuple

import numpy as np

from oracle import cref

f32, f64 = np.float32, np.float64

Ais = namedtuple("Ais", "spins log_w energy A N states energies")


def fields(state, spins, hs, Js, plan):
    """The float32 field of every spin of ``spins`` in every chain of ``state`` (C, n), as v1 computes it: hs_i, then the
    signed couplings of the CSR row in row order, each add rounded.  Vectorised over chains and spins; the loop is over
    the position in the row.  Returns (C, len(spins)) float32."""
    spins = np.asarray(spins, dtype=np.int64)
    adj_ptr, adj_idx, adj_eid = np.asarray(plan.adj_ptr), np.asarray(plan.adj_idx), np.asarray(plan.adj_eid)
    f = np.broadcast_to(np.asarray(hs, dtype=f32)[spins], (state.shape[0], spins.size)).copy()
    if spins.size == 0 or adj_idx.size == 0:
        return f
    first, deg = adj_ptr[spins], adj_ptr[spins + 1] - adj_ptr[spins]
    for q in range(int(deg.max())):
        has = q < deg
        pos = np.where(has, first + q, 0)
        w = np.asarray(Js, dtype=f32)[adj_eid[pos]]
        stepped = (f + np.where(state[:, adj_idx[pos]] > 0, w, -w).astype(f32)).astype(f32)
        f = np.where(has[None, :], stepped, f)
    return f


def ais(plan, hs, Js, betas, ids, seed, sweep0, start=None, beta_from=0.0, trace=False):
    """``betas``: (S,) for all chains or (C, S); ``ids``: the chain ids; ``start``: (C, n) int8, or None for fresh chains
    (the INIT stream at ``sweep0``).  Returns ``Ais``: the final spins (C, n) int8; ``log_w`` and ``energy`` (C,) float64;
    ``A`` (C,): the sum of the absolute values of every energy addend of the chain (the n start addends and every
    update's); ``N = n + n S + S``: their number plus the S multiply-adds of the weight.  ``trace``: also ``states``
    (S + 1, C, n) -- the state before each sweep, and the final one -- and ``energies`` (S + 1, C), the definition's
    running energy at those points."""
    ids = np.asarray(ids, dtype=np.uint32)
    C, n = ids.size, plan.n
    table = np.asarray(betas, dtype=f32)
    S = int(table.shape[-1])
    table = np.ascontiguousarray(np.broadcast_to(table, (C, S)))
    hs, Js = np.asarray(hs, dtype=f32), np.asarray(Js, dtype=f32)
    order, class_ptr = np.asarray(plan.order), np.asarray(plan.class_ptr)
    st = cref.init_state(ids, n, seed, sweep0) if start is None else np.array(start, dtype=np.int8, copy=True)

    add0 = 0.5 * st.astype(f64) * (hs.astype(f64)[None, :] + fields(st, np.arange(n), hs, Js, plan).astype(f64))
    energy, A = add0.sum(axis=1), np.abs(add0).sum(axis=1)
    log_w = np.zeros(C, dtype=f64)
    prev = np.full(C, f64(f32(beta_from)))
    states, energies = [st.copy()], [energy.copy()]
    for k in range(S):
        beta = table[:, k].astype(f64)
        log_w -= (beta - prev) * energy
        prev = beta
        new = np.empty_like(st)
        values, inv = np.unique(table[:, k], return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        for r, b in enumerate(values):
            sel = np.flatnonzero(inv == r)
            new[sel] = cref.gibbs_sweeps(st[sel], ids[sel], hs, Js, float(b), plan.order, plan.class_ptr, plan.adj_ptr,
                                         plan.adj_idx, plan.adj_eid, seed, sweep0 + k, 1)
        cur = st.copy()
        for c in range(class_ptr.size - 1):
            sp = order[class_ptr[c]:class_ptr[c + 1]].astype(np.int64)
            f = fields(cur, sp, hs, Js, plan)
            # (+-2 f or 0: the float32 product is exact)
            d = ((new[:, sp].astype(f32) - cur[:, sp].astype(f32)) * f).astype(f32).astype(f64)
            energy = energy + d.sum(axis=1)
            A = A + np.abs(d).sum(axis=1)
            cur[:, sp] = new[:, sp]
        assert np.array_equal(cur, new)
        st = new
        if trace:
            states.append(st.copy())
            energies.append(energy.copy())
    return Ais(st, log_w, energy, A, n + n * S + S, np.stack(states) if trace else None, np.stack(energies) if trace else None)


def log_z_estimate(n, log_w):
    """(estimate, ess, std_err) of log Z from the log weights of chains annealed from beta = 0 (log Z(0) = n log 2)."""
    log_w = np.asarray(log_w, dtype=f64)
    m = log_w.max()
    w = np.exp(log_w - m)
    ess = w.sum() ** 2 / (w ** 2).sum()
    return n * np.log(2.0) + m + np.log(w.mean()), ess, np.sqrt(max(1.0 / ess - 1.0 / log_w.size, 0.0))


def exact_log_z(n, hs, Js, edge_i, edge_j, beta):
    """log sum_s exp(-beta E(s)) over all 2^n states, float64."""
    s = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(f64) * 2.0 - 1.0
    a = -f64(beta) * (s @ np.asarray(hs, dtype=f64) + (s[:, edge_i] * s[:, edge_j]) @ np.asarray(Js, dtype=f64))
    m = a.max()
    return m + np.log(np.exp(a - m).sum())
