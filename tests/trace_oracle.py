"""The definition of the traced draw ("DVG trace v1", include/dvg.h) on top of the unchanged oracle -- a helper of the
trace tests, not a test.

The spins are the plain draw's: ``oracle/gibbs.py::gibbs_sweeps`` called one sweep at a time (the beta, ``sweep0 + k``, one
sweep).  Sweep k of the call (0-based) is recorded iff ``k + 1 > burn_in`` and ``(k + 1 - burn_in) % thin == 0``; a record is
the state packed with numpy, bit b of word w = spin 32 w + b is +1, bits of spins >= n zero.  Moments are integer sums."""
from collections import namedtuple

import numpy as np

from oracle import gibbs

History = namedtuple("History", "states")          # (S + 1, C, n) int8: the start state, then the state after every sweep
Trace = namedtuple("Trace", "spins bits sweeps")   # (C, n) int8 final; (C, M, W) uint32; (M,) int64: the recorded k + 1


def pack(states):
    """(..., n) +-1 -> (..., W = ceil(n / 32)) uint32."""
    states = np.asarray(states)
    n = states.shape[-1]
    W = (n + 31) // 32
    up = np.zeros(states.shape[:-1] + (32 * W,), dtype=np.uint64)
    up[..., :n] = states > 0
    words = (up.reshape(states.shape[:-1] + (W, 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return words.astype(np.uint32)


def unpack(bits, n):
    """(..., W) uint32 -> (..., n) int8 +-1."""
    bits = np.asarray(bits, dtype=np.uint32)
    b = (bits[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return (2 * b.reshape(bits.shape[:-1] + (-1,))[..., :n].astype(np.int8) - 1).astype(np.int8)


def recorded_sweeps(n_sweeps, burn_in, thin):
    """The recorded sweeps as k + 1, by the rule itself (a loop over the sweeps, no closed form)."""
    return np.array([k + 1 for k in range(n_sweeps) if k + 1 > burn_in and (k + 1 - burn_in) % thin == 0], dtype=np.int64)


def history(plan, hs, Js, beta, ids, seed, sweep0, n_sweeps, start=None, sweeper=gibbs.gibbs_sweeps, init_state=gibbs.init_state):
    """The chains' states before the first sweep and after every sweep, one oracle call per sweep.  ``start``: (C, n) int8,
    or None for fresh chains (the INIT stream at ``sweep0``)."""
    ids = np.asarray(ids, dtype=np.uint32)
    st = init_state(ids, plan.n, seed, sweep0) if start is None else np.array(start, dtype=np.int8, copy=True)
    states = [st.copy()]
    for k in range(n_sweeps):
        st = sweeper(st.copy(), ids, np.asarray(hs, np.float32), np.asarray(Js, np.float32), float(beta), plan.order, plan.class_ptr,
                     plan.adj_ptr, plan.adj_idx, plan.adj_eid, seed, sweep0 + k, 1)
        states.append(np.array(st, dtype=np.int8, copy=True))
    return History(np.stack(states))


def trace_of(hist, burn_in, thin):
    """The traced draw whose sweeps are ``hist``'s: which states are recorded, packed."""
    S = hist.states.shape[0] - 1
    sweeps = recorded_sweeps(S, burn_in, thin)
    assert sweeps.size == (S - burn_in) // thin
    bits = pack(hist.states[sweeps]).transpose(1, 0, 2)  # (C, M, W)
    return Trace(hist.states[-1], np.ascontiguousarray(bits), sweeps)


def trace(plan, hs, Js, beta, ids, seed, sweep0, n_sweeps, burn_in=0, thin=1, start=None, **kw):
    return trace_of(history(plan, hs, Js, beta, ids, seed, sweep0, n_sweeps, start=start, **kw), burn_in, thin)


def moments(rows, edge_i, edge_j):
    """(rows, n) +-1 -> (spin_sum (n,), pair_sum (E,)) int64."""
    s = np.asarray(rows, dtype=np.int64).reshape(-1, np.shape(rows)[-1])
    return s.sum(axis=0), (s[:, np.asarray(edge_i)] * s[:, np.asarray(edge_j)]).sum(axis=0)


def moments_of_bits(bits, n, edge_i, edge_j):
    """The same from packed rows (..., W); bits of spins >= n are ignored."""
    return moments(unpack(np.asarray(bits).reshape(-1, np.shape(bits)[-1]), n), edge_i, edge_j)


def exact_moments(n, hs, Js, edge_i, edge_j, beta):
    """<s_i> (n,) and <s_i s_j> (E,) under exp(-beta E) over all 2^n states, float64."""
    s = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64) * 2.0 - 1.0
    pairs = s[:, np.asarray(edge_i)] * s[:, np.asarray(edge_j)]
    a = -np.float64(beta) * (s @ np.asarray(hs, dtype=np.float64) + pairs @ np.asarray(Js, dtype=np.float64))
    p = np.exp(a - a.max())
    p /= p.sum()
    return p @ s, p @ pairs
