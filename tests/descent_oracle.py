"""The definition of ``dvg_grbm_descend_packed`` ("DVG descent v1", include/dvg.h) and of ``sampler.Minima`` in numpy -- a helper
of the descent tests, not a test.

The rows unpacked with ``trace_oracle.unpack``; ``hs`` / ``Js`` the float32 fields of ``oracle.gibbs.scaled_fields``; the CSR of
``oracle.gibbs.build_csr``; the local field by the float32 loop of ``oracle.gibbs.gibbs_sweeps`` (start from ``hs_i``, add ``+-Js``
per CSR entry in row order, every sum rounded to float32); the classes from the plan's ``order`` and ``class_ptr``.  A spin is
unstable iff ``s_i f_i > 0`` in float32; a sweep flips the unstable spins class by class; a row stops after its first sweep
without a flip, or after ``max_sweeps``."""
from collections import namedtuple

import numpy as np

import trace_oracle
from oracle import gibbs

f32 = np.float32
Descent = namedtuple("Descent", "bits sweeps flips unstable s")


def fields_of(s, spins, hs, Js, adj_ptr, adj_idx, adj_eid):
    """(T, len(spins)) float32: the sampler's local field of the given spins of every +-1 row (T, n) -- entry q of every
    spin's CSR row at once, in row order, every sum rounded to float32; a spin with fewer entries is left alone."""
    spins = np.asarray(spins, dtype=np.int64)
    f = np.repeat(hs[spins][None, :], s.shape[0], axis=0).astype(f32)
    deg = adj_ptr[spins + 1] - adj_ptr[spins]
    for q in range(int(deg.max()) if len(spins) else 0):
        sel = np.nonzero(deg > q)[0]
        pos = adj_ptr[spins[sel]] + q
        w = Js[adj_eid[pos]][None, :]
        f[:, sel] = (f[:, sel] + np.where(s[:, adj_idx[pos]] > 0, w, -w).astype(f32)).astype(f32)
    return f


def count_unstable(s, hs, Js, adj_ptr, adj_idx, adj_eid):
    """(T,) int32: the unstable spins of every row, as "DVG fields v1" counts them."""
    f = fields_of(s, np.arange(s.shape[1]), hs, Js, adj_ptr, adj_idx, adj_eid)
    return ((s.astype(f32) * f) > 0).sum(axis=1).astype(np.int32)


def descend(bits, n, hs, Js, edge_i, edge_j, order, class_ptr, max_sweeps):
    """Everything the entry returns for packed rows (..., W), the rows flattened to T: ``bits`` (T, W) uint32 with zero pad
    bits, ``sweeps``, ``flips``, ``unstable`` (T,) int32, and ``s`` (T, n) int8, the final rows unpacked."""
    hs, Js = np.asarray(hs), np.asarray(Js)
    assert hs.dtype == f32 and Js.dtype == f32 and hs.shape == (n,) and max_sweeps >= 1
    bits = np.asarray(bits)
    bits = bits.view(np.uint32) if bits.dtype == np.int32 else bits
    s = trace_oracle.unpack(bits.reshape(-1, bits.shape[-1]), n).copy()
    T = s.shape[0]
    adj_ptr, adj_idx, adj_eid = gibbs.build_csr(n, np.asarray(edge_i, dtype=np.int64), np.asarray(edge_j, dtype=np.int64))
    order, class_ptr = np.asarray(order), np.asarray(class_ptr)
    sweeps, flips = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32)
    active = np.arange(T)  # the rows whose every sweep so far flipped something
    for _sweep in range(max_sweeps):
        if active.size == 0:
            break
        sub = s[active]
        moved = np.zeros(active.size, dtype=np.int32)
        for k in range(len(class_ptr) - 1):
            spins = order[class_ptr[k]:class_ptr[k + 1]]  # (an independent set: one after another == together)
            flip = (sub[:, spins].astype(f32) * fields_of(sub, spins, hs, Js, adj_ptr, adj_idx, adj_eid)) > 0
            sub[:, spins] = np.where(flip, -sub[:, spins], sub[:, spins])
            moved += flip.sum(axis=1).astype(np.int32)
        s[active] = sub
        flips[active] += moved
        sweeps[active] += moved > 0
        active = active[moved > 0]
    unstable = np.zeros(T, dtype=np.int32)
    if active.size:  # cut off by max_sweeps: their last permitted sweep still flipped something
        unstable[active] = count_unstable(s[active], hs, Js, adj_ptr, adj_idx, adj_eid)
    return Descent(trace_oracle.pack(s), sweeps, flips, unstable, s)


def energy(s, hs, Js, edge_i, edge_j):
    """Float64 energies of +-1 rows under (hs, Js)."""
    return gibbs.energy(s, hs, Js, np.asarray(edge_i), np.asarray(edge_j))


# ------------------------------------------------------------------------------------------------ sampler.Minima
def unique_minima(bits):
    """The distinct rows of (T, W) words by falling multiplicity, ties in the order of ``numpy.unique(axis=0)`` on the words
    read as int32 (what ``torch.unique(dim=0)`` sorts by): ``(rows, counts, inverse)``."""
    words = np.asarray(bits).reshape(-1, np.asarray(bits).shape[-1]).view(np.int32)
    rows, inverse, counts = np.unique(words, axis=0, return_inverse=True, return_counts=True)
    inverse = np.asarray(inverse).reshape(-1)
    perm = np.argsort(-counts, kind="stable")
    rank = np.empty_like(perm)
    rank[perm] = np.arange(len(perm))
    return rows[perm], counts[perm], rank[inverse]


def estimates(start_bits, bits, sweeps, flips, unstable, energy_start, energy, n):
    """Every scalar and per-row property of ``Minima`` by name, numpy."""
    a = trace_oracle.unpack(np.asarray(start_bits).view(np.uint32).reshape(-1, np.asarray(bits).shape[-1]), n)
    b = trace_oracle.unpack(np.asarray(bits).view(np.uint32).reshape(-1, np.asarray(bits).shape[-1]), n)
    un = np.asarray(unstable).reshape(-1)
    _rows, counts, _inv = unique_minima(bits)
    p = counts / counts.sum()
    return dict(converged=un == 0, converged_share=(un == 0).mean(),
                energy_drop=np.asarray(energy_start, np.float64).reshape(-1) - np.asarray(energy, np.float64).reshape(-1),
                distance=(a != b).sum(axis=1).astype(np.int32), mean_flips=np.asarray(flips, np.float64).mean(),
                mean_sweeps=np.asarray(sweeps, np.float64).mean(), basin_entropy=-(p * np.log(p)).sum())
