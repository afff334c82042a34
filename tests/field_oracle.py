"""The per-chain-field draw ("DVG field v1", ``dvg_gibbs_sample_fields`` in include/dvg.h), restated for the tests with every
chain carrying its own row of scaled, clamped linear terms.

``oracle.gibbs.gibbs_sweeps`` takes one ``hs`` for all chains, so the definition -- that function called once per chain with
``scaled_fields(linear + fields[c], ...)`` -- costs a Python pass over the graph per chain.  ``field_sweeps`` below is the
same arithmetic walked ONCE with ``hs`` of shape (C, n): a colour class at a time, chains and spins side by side, the
neighbours of a spin added in CSR order, each add rounded to float32.  It borrows the oracle's ``spec_exp`` and Philox and
restates the sweep; ``tests/test_gibbs_fields_host.py`` pins it to the oracle called chain by chain."""
import numpy as np

from oracle import gibbs
from oracle.philox import STREAM_GIBBS, philox4x32_10, u32_to_unit_float

f32 = np.float32


def chain_fields(linear, fields, prefactor, h_range):
    """``hs`` (C, n): ``clamp(rn(prefactor * rn(linear + fields[c])))``; ``fields`` (C, n), or (n,) for one shared row (then (1, n))."""
    lin = (np.asarray(linear, dtype=f32)[None, :] + np.atleast_2d(np.asarray(fields, dtype=f32))).astype(f32)
    hs = (lin * f32(prefactor)).astype(f32)
    if h_range is not None:
        hs = np.minimum(np.maximum(hs, f32(h_range[0])), f32(h_range[1]))
    return hs


def field_sweeps(state, chain_ids, hs, Js, beta, plan, seed, sweep0, nsweeps):
    """``nsweeps`` sweeps from global index ``sweep0`` on a copy of ``state`` (C, n) int8, chain c under ``hs[c]``; ``plan``: a
    ``graphs.GibbsPlan`` (order, class_ptr, adj_ptr, adj_idx, adj_eid).  Returns the new state."""
    state = np.array(state, dtype=np.int8, copy=True)
    C, n = state.shape
    hs = np.asarray(hs, dtype=f32)
    assert hs.shape == (C, n)
    ids = np.asarray(chain_ids, dtype=np.uint32)[:, None]
    Js = np.asarray(Js, dtype=f32)
    order, class_ptr = np.asarray(plan.order), np.asarray(plan.class_ptr)
    adj_ptr, adj_idx, adj_eid = np.asarray(plan.adj_ptr), np.asarray(plan.adj_idx), np.asarray(plan.adj_eid)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    two_beta = f32(f32(2.0) * f32(beta))
    for t in range(sweep0, sweep0 + nsweeps):
        for k in range(len(class_ptr) - 1):
            spins = order[class_ptr[k]:class_ptr[k + 1]].astype(np.int64)
            if spins.size == 0:
                continue
            first, deg = adj_ptr[spins].astype(np.int64), (adj_ptr[spins + 1] - adj_ptr[spins]).astype(np.int64)
            f = hs[:, spins].copy()
            for q in range(int(deg.max())):  # the q-th CSR neighbour of every spin of the class that has one
                has = np.flatnonzero(deg > q)
                at = first[has] + q
                w = Js[adj_eid[at]][None, :]
                f[:, has] = (f[:, has] + np.where(state[:, adj_idx[at]] > 0, w, -w).astype(f32)).astype(f32)
            z = np.minimum(np.maximum((two_beta * f).astype(f32), -gibbs.Z_CLAMP), gibbs.Z_CLAMP)
            tt = gibbs.spec_exp(z)
            r = philox4x32_10(spins.astype(np.uint32)[None, :], ids, np.uint32(t >> 2), np.uint32(STREAM_GIBBS), k0, k1)[t & 3]
            u = u32_to_unit_float(r)
            acc = (u * (f32(1.0) + tt).astype(f32)).astype(f32) < f32(1.0)
            state[:, spins] = np.where(acc, 1, -1)
    return state
