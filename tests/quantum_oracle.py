"""The definition of the simulated-quantum-annealing draw ("DVG SQA v1", include/dvg.h) in numpy -- a helper of the quantum
tests, not a test.  Written from the definition, vectorised over (chains, slices).

A chain is P slices of n spins, ``s[c, k, i] = +-1``; the slices are periodic.  ``hs`` / ``Js`` are the float32 fields of
``oracle.gibbs.scaled_fields``, the CSR that of ``oracle.gibbs.build_csr``.  Site (i, k) of chain id c in global sweep t = sweep0 +
q, every operation float32 and rounded by itself:

    f  = hs_i, then for each CSR entry of spin i in row order  f = f + (s[k][j] > 0 ? Js : -Js)
    nb = s[k-1][i] + s[k+1][i]
    z0 = beta_slice[q] f - kappa[q] nb;   z = clamp(2 z0, -87, 87);   tt = spec_exp(z)
    u  = u32_to_unit(philox4x32_10(i, c, t, STREAM_SQA | (k << 8), key)[0])
    s[k][i] = +1  iff  u (1 + tt) < 1

Inside a sweep: for each colour class in order, first the even slices of all its spins, then the odd ones.  Fresh chains:
``s[k][i] = +1`` iff bit 31 of ``philox4x32_10(i, c, sweep0, STREAM_INIT | (k << 8), key)[0]``."""
from collections import namedtuple

import numpy as np

import trace_oracle
from oracle import gibbs
from oracle.philox import STREAM_INIT, philox4x32_10, u32_to_unit_float

f32 = np.float32
STREAM_SQA = 6
Sliced = namedtuple("Sliced", "s bits samples")  # (C, P, n) int8; (C, P, W) uint32, pad bits 0; (C, n) float32 = slice 0


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def init_slices(ids, P, n, seed, sweep0):
    """(C, P, n) int8: the INIT stream's start state of chains ``ids``."""
    ids = np.asarray(ids, dtype=np.uint32)
    k0, k1 = _key(seed)
    tag = (np.uint32(STREAM_INIT) | (np.arange(P, dtype=np.uint32) << np.uint32(8)))[None, :, None]
    r0 = philox4x32_10(np.arange(n, dtype=np.uint32)[None, None, :], ids[:, None, None], np.uint32(int(sweep0) & 0xFFFFFFFF), tag, k0, k1)[0]
    return np.where((r0 >> np.uint32(31)) != 0, 1, -1).astype(np.int8)


def fields_of(s, spins, hs, Js, adj_ptr, adj_idx, adj_eid):
    """(C, P, len(spins)) float32: the local field of the given spins in every slice, entry q of every spin's CSR row at once, in
    row order, every sum rounded to float32."""
    spins = np.asarray(spins, dtype=np.int64)
    f = np.broadcast_to(hs[spins], s.shape[:2] + (len(spins),)).astype(f32)
    deg = adj_ptr[spins + 1] - adj_ptr[spins]
    for q in range(int(deg.max()) if len(spins) else 0):
        sel = np.nonzero(deg > q)[0]
        pos = adj_ptr[spins[sel]] + q
        w = Js[adj_eid[pos]]
        f[:, :, sel] = (f[:, :, sel] + np.where(s[:, :, adj_idx[pos]] > 0, w, -w).astype(f32)).astype(f32)
    return f


def sweeps(s, ids, hs, Js, beta_slice, kappa, order, class_ptr, adj_ptr, adj_idx, adj_eid, seed, sweep0):
    """``len(beta_slice)`` sweeps on a copy of ``s`` (C, P, n) int8; returns it."""
    s = np.array(s, dtype=np.int8, copy=True)
    C, P, n = s.shape
    assert P >= 2 and P & (P - 1) == 0 and P <= 64
    ids = np.asarray(ids, dtype=np.uint32)
    hs, Js = np.asarray(hs), np.asarray(Js)
    assert hs.dtype == f32 and Js.dtype == f32
    beta_slice, kappa = np.asarray(beta_slice, dtype=f32), np.asarray(kappa, dtype=f32)
    assert beta_slice.shape == kappa.shape and beta_slice.ndim == 1
    k0, k1 = _key(seed)
    tag = (np.uint32(STREAM_SQA) | (np.arange(P, dtype=np.uint32) << np.uint32(8)))[None, :, None]
    parity = np.arange(P) & 1
    for q in range(len(beta_slice)):
        t = np.uint32((int(sweep0) + q) & 0xFFFFFFFF)
        bs, kp = beta_slice[q], kappa[q]
        for c in range(len(class_ptr) - 1):
            spins = np.asarray(order[class_ptr[c]:class_ptr[c + 1]], dtype=np.int64)
            if len(spins) == 0:
                continue
            bf = (bs * fields_of(s, spins, hs, Js, adj_ptr, adj_idx, adj_eid)).astype(f32)
            u = u32_to_unit_float(philox4x32_10(spins.astype(np.uint32)[None, None, :], ids[:, None, None], t, tag, k0, k1)[0])
            for half in (0, 1):
                col = s[:, :, spins]
                nb = (np.roll(col, 1, axis=1).astype(np.int32) + np.roll(col, -1, axis=1)).astype(f32)  # s[k-1] + s[k+1]
                z0 = (bf - (kp * nb).astype(f32)).astype(f32)
                z = (f32(2.0) * z0).astype(f32)
                z = np.minimum(np.maximum(z, -gibbs.Z_CLAMP), gibbs.Z_CLAMP)
                tt = gibbs.spec_exp(z)
                up = (u * (f32(1.0) + tt).astype(f32)).astype(f32) < f32(1.0)
                new = np.where(up, 1, -1).astype(np.int8)
                col = np.where((parity == half)[None, :, None], new, col)
                s[:, :, spins] = col
    return s


def draw(plan, hs, Js, beta_slice, kappa, ids, P, seed, sweep0, start_bits=None):
    """The whole entry: fresh chains (``start_bits=None``) or (C, P, W) packed rows to continue from (pad bits ignored)."""
    n = plan.n
    adj_ptr, adj_idx, adj_eid = gibbs.build_csr(n, np.asarray(plan.edge_i, dtype=np.int64), np.asarray(plan.edge_j, dtype=np.int64))
    if start_bits is None:
        s = init_slices(ids, P, n, seed, sweep0)
    else:
        b = np.asarray(start_bits)
        s = trace_oracle.unpack(b.view(np.uint32) if b.dtype == np.int32 else b, n)
        assert s.shape == (len(ids), P, n)
    s = sweeps(s, ids, hs, Js, beta_slice, kappa, np.asarray(plan.order), np.asarray(plan.class_ptr), adj_ptr, adj_idx, adj_eid,
               seed, sweep0)
    return Sliced(s, trace_oracle.pack(s), s[:, 0].astype(f32))


def slice_overlap(s):
    """The mean over chains and neighbouring slice pairs (k, k + 1 mod P) of (1 / n) sum_i s[k][i] s[k+1][i], float64."""
    s = np.asarray(s, dtype=np.float64)
    return float((s * np.roll(s, -1, axis=1)).mean())


def exact_law(hs, Js, edge_i, edge_j, P, beta_slice, kappa):
    """All 2^(P n) states of one chain and their probabilities under exp(-beta_slice sum_k E(s[k]) + kappa sum_k sum_i s[k][i]
    s[k+1][i]), float64: ``(states (2^(P n), P, n), p)``.  Site (k, i) is bit k n + i of the state's index."""
    n = len(hs)
    bits = (np.arange(1 << (P * n))[:, None] >> np.arange(P * n)[None, :]) & 1
    s = (2.0 * bits - 1.0).reshape(-1, P, n)
    hs64, Js64 = np.asarray(hs, dtype=np.float64), np.asarray(Js, dtype=np.float64)
    e = s @ hs64 + (s[:, :, np.asarray(edge_i)] * s[:, :, np.asarray(edge_j)]) @ Js64  # (states, P)
    along = (s * np.roll(s, -1, axis=1)).sum(axis=(1, 2))  # every (k, k + 1 mod P) pair once: for P = 2 the pair counts twice
    a = -float(beta_slice) * e.sum(axis=1) + float(kappa) * along
    p = np.exp(a - a.max())
    return s, p / p.sum()
