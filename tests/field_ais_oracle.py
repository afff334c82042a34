"""The definition of the weighed per-chain-field draw ("DVG field AIS v1", ``dvg_gibbs_sample_fields_ais`` in include/dvg.h)
on top of the helpers of the two draws it joins -- a helper of the field-AIS tests, not a test.

Rows: ``field_oracle.chain_fields`` on ``rn(lambda_k * fields[row of c])``, one call per sweep.  Spins: ``field_oracle.field_sweeps``
called once per sweep (that sweep's beta, ``sweep0 + k``, one sweep, ``hs = row_k``) on the chains that share the beta.  Energy:
as ``ais_oracle.ais`` carries it -- between two sweeps the colour classes are walked in order, the float32 CSR-order fields of the
class's spins on the current MIXED state are the fields the decisions used -- with ``local_fields`` below, which is
``ais_oracle.fields`` with a row of hs per chain (``tests/test_gibbs_field_ais_host.py`` pins the two to each other).  New: the
step of the row's change at the head of a sweep.  Everything but the rows and the fields is float64."""
from collections import namedtuple

import numpy as np

import ais_oracle
import field_oracle
from oracle import cref

f32, f64 = np.float32, np.float64

FieldAis = namedtuple("FieldAis", "spins log_w energy A N")


def local_fields(state, spins, hs, Js, plan):
    """``ais_oracle.fields`` with ``hs`` of shape (C, n): the float32 field of every spin of ``spins`` in every chain of ``state``
    (C, n), chain c starting from ``hs[c, i]``, then the signed couplings of the CSR row in row order, each add rounded.
    Returns (C, len(spins)) float32."""
    spins = np.asarray(spins, dtype=np.int64)
    adj_ptr, adj_idx, adj_eid = np.asarray(plan.adj_ptr), np.asarray(plan.adj_idx), np.asarray(plan.adj_eid)
    f = np.asarray(hs, dtype=f32)[:, spins].copy()
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


def chain_rows(linear, fields, lam, prefactor, h_range, row_chains=1):
    """``row[c] = clamp(rn(prefactor * rn(linear + rn(lam[c] * fields[c // row_chains]))))`` (C, n) float32; ``fields`` (rows, n), or
    (n,) for one row shared by all chains; ``lam`` (C,) float32."""
    lam = np.asarray(lam, dtype=f32)
    fields = np.asarray(fields, dtype=f32)
    per_chain = fields[np.arange(lam.size) // row_chains] if fields.ndim == 2 else np.broadcast_to(fields, (lam.size, fields.size))
    return field_oracle.chain_fields(linear, (lam[:, None] * per_chain).astype(f32), prefactor, h_range)


def field_ais(plan, linear, fields, prefactor, h_range, Js, betas, scales, ids, seed, sweep0, start=None, beta_from=0.0,
              scale_from=1.0, row_chains=1):
    """``betas``: (S,) or (C, S); ``scales``: None (strength 1 throughout, ``scale_from`` ignored), (S,) or (C, S); ``ids``: the
    chain ids; ``start``: (C, n) int8, or None for fresh chains (the INIT stream at ``sweep0``); ``Js``: the scaled, clamped
    couplings.  Returns ``FieldAis``: the final spins (C, n) int8; ``log_w`` and ``energy`` (C,) float64; ``A`` (C,): the sum of
    the absolute values of every energy addend of the chain -- the n start addends, every update's and, with ``scales``, the
    ``|row_k[i] - row_{k-1}[i]|`` of every sweep; ``N``: their number, ``n + n S`` or ``n + 2 n S``, plus the ``2 S``
    multiply-adds of the weight."""
    ids = np.asarray(ids, dtype=np.uint32)
    C, n = ids.size, plan.n
    table = np.asarray(betas, dtype=f32)
    S = int(table.shape[-1])
    table = np.ascontiguousarray(np.broadcast_to(table, (C, S)))
    lams = None if scales is None else np.ascontiguousarray(np.broadcast_to(np.asarray(scales, dtype=f32), (C, S)))
    Js = np.asarray(Js, dtype=f32)
    order, class_ptr = np.asarray(plan.order), np.asarray(plan.class_ptr)
    st = cref.init_state(ids, n, seed, sweep0) if start is None else np.array(start, dtype=np.int8, copy=True)

    row = chain_rows(linear, fields, np.full(C, f32(scale_from) if lams is not None else f32(1.0)), prefactor, h_range, row_chains)
    add0 = 0.5 * st.astype(f64) * (row.astype(f64) + local_fields(st, np.arange(n), row, Js, plan).astype(f64))
    energy, A = add0.sum(axis=1), np.abs(add0).sum(axis=1)
    log_w = np.zeros(C, dtype=f64)
    prev = np.full(C, f64(f32(beta_from)))
    for k in range(S):
        beta = table[:, k].astype(f64)
        d = np.zeros(C, dtype=f64)
        if lams is not None:
            new_row = chain_rows(linear, fields, lams[:, k], prefactor, h_range, row_chains)
            add = (new_row.astype(f64) - row.astype(f64)) * st.astype(f64)
            d, A, row = add.sum(axis=1), A + np.abs(add).sum(axis=1), new_row
        log_w -= (beta - prev) * energy + beta * d
        energy = energy + d
        prev = beta
        new = np.empty_like(st)
        values, inv = np.unique(table[:, k], return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        for r, b in enumerate(values):
            sel = np.flatnonzero(inv == r)
            new[sel] = field_oracle.field_sweeps(st[sel], ids[sel], row[sel], Js, float(b), plan, seed, sweep0 + k, 1)
        cur = st.copy()
        for c in range(class_ptr.size - 1):
            sp = order[class_ptr[c]:class_ptr[c + 1]].astype(np.int64)
            f = local_fields(cur, sp, row, Js, plan)
            # (+-2 f or 0: the float32 product is exact)
            step = ((new[:, sp].astype(f32) - cur[:, sp].astype(f32)) * f).astype(f32).astype(f64)
            energy = energy + step.sum(axis=1)
            A = A + np.abs(step).sum(axis=1)
            cur[:, sp] = new[:, sp]
        assert np.array_equal(cur, new)
        st = new
    return FieldAis(st, log_w, energy, A, n + n * S * (2 if lams is not None else 1) + 2 * S)


def log_ratio_estimate(log_w):
    """(estimate, ess, std_err) of log(Z_to / Z_from) from the log weights of the chains of one row, as
    ``ais_oracle.log_z_estimate`` makes them of log Z."""
    est, ess, std_err = ais_oracle.log_z_estimate(0, log_w)
    return est, ess, std_err
