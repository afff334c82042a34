"""The definition of the isoenergetic cluster move ("DVG ICM v1", ``dvg_gibbs_cluster_move`` in include/dvg.h) in numpy, and of
the composed draw (``GibbsSampler.sample_tempered_cluster``) on top of the unchanged ``tempered_oracle`` -- a helper of the
cluster tests, not a test.

Chains come in ladders of R consecutive chains, the ladders 2p and 2p + 1 are twins.  The holder of rung r in a ladder is its
lowest chain whose rung, clamped into 0 .. R-1, is r.  Job (p, r), r >= rung_from, with a, b the two holders: D = the sites where
the signs of the rows differ, ascending, k = |D|; root = element ((uint64)word k) >> 32 of D, word = philox(ctr = (r, id of the
first chain of ladder 2p, move, 7), key = seed)[0]; the cluster = the connected component of root in the graph induced on D
(every edge, whatever its coupling); on the cluster the two rows change places.

The composed draw: in front of every sweep t with t % cluster_every == 0 -- never in front of the first sweep of fresh chains --
move t // cluster_every; between two moves one ``tempered_oracle.tempered`` call that is handed spins and rungs."""
from collections import namedtuple

import numpy as np

import tempered_oracle
from oracle.philox import philox4x32_10

STREAM_ICM = 7

# spins (C, n) int8 after the move; sizes, differ (pairs, R) uint32
Move = namedtuple("Move", "spins sizes differ")
# tempered: the last segment's tempered_oracle.Tempered; accepted (Q, R), attempts (R - 1,) summed over the segments; sizes, differ
# (moves, pairs, R); moves: the move indices; coins: every segment's coins
Composed = namedtuple("Composed", "tempered accepted attempts sizes differ moves coins")


_ROWS = {}


def holders(rungs, R, ladder):
    """(R,) the chain of ``ladder`` that holds each rung, -1 where none does."""
    out = np.full(R, -1, dtype=np.int64)
    for c in range(ladder * R + R - 1, ladder * R - 1, -1):
        out[min(max(int(rungs[c]), 0), R - 1)] = c
    return out


def component(plan, member, root):
    """The connected component of ``root`` in the graph induced on the sites with ``member`` set: a sorted index array."""
    if _ROWS.get("plan") is not plan:  # (the CSR rows as lists, made once per graph)
        adj_ptr, adj_idx = np.asarray(plan.adj_ptr), np.asarray(plan.adj_idx)
        _ROWS.update(plan=plan, rows=[adj_idx[adj_ptr[i]:adj_ptr[i + 1]].tolist() for i in range(plan.n)])
    rows, member = _ROWS["rows"], member.tolist()
    seen = {int(root)}
    stack = [int(root)]
    while stack:
        for j in rows[stack.pop()]:
            if member[j] and j not in seen:
                seen.add(j)
                stack.append(j)
    return np.array(sorted(seen), dtype=np.int64)


def cluster_move(plan, spins, rungs, R, rung_from, id0, seed, move, one_sided=False):
    """``spins`` (C, n) int8, ``rungs`` (C,) or None (R == 1), ``id0`` the id of chain 0.  ``one_sided``: the cluster is
    flipped in twin a only -- NOT the definition; the invariant tests show with it that they would notice."""
    st = np.array(spins, dtype=np.int8, copy=True)
    C, n = st.shape
    assert C % (2 * R) == 0 and (rungs is not None or R == 1)
    rungs = np.zeros(C, dtype=np.int64) if rungs is None else np.asarray(rungs)
    P = C // (2 * R)
    k0, k1 = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    sizes, differ = np.zeros((P, R), dtype=np.uint32), np.zeros((P, R), dtype=np.uint32)
    for p in range(P):
        ha, hb = holders(rungs, R, 2 * p), holders(rungs, R, 2 * p + 1)
        for r in range(rung_from, R):
            a, b = ha[r], hb[r]
            if a < 0 or b < 0:
                continue
            member = (st[a] < 0) != (st[b] < 0)
            D = np.flatnonzero(member)
            k = differ[p, r] = D.size
            if k == 0:
                continue
            ctr = [np.uint32(v & 0xFFFFFFFF) for v in (r, int(id0) + 2 * p * R, int(move), STREAM_ICM)]
            word = int(philox4x32_10(*ctr, k0, k1)[0])
            cl = component(plan, member, D[(word * int(k)) >> 32])
            sizes[p, r] = cl.size
            if one_sided:
                st[a, cl] = -st[a, cl]
            else:
                st[a, cl], st[b, cl] = st[b, cl].copy(), st[a, cl].copy()
    return Move(st, sizes, differ)


def schedule(sweep0, n_sweeps, cluster_every, fresh):
    """[(move or None, first sweep, sweeps)]: written from the rule, sweep by sweep."""
    out = []
    for t in range(sweep0, sweep0 + n_sweeps):
        moved = t % cluster_every == 0 and not (fresh and t == sweep0)
        if moved or not out:
            out.append([t // cluster_every if moved else None, t, 0])
        out[-1][2] += 1
    return [tuple(s) for s in out]


def tempered_cluster(plan, hs, Js, ladder, ids, seed, sweep0, n_sweeps, swap_every, cluster_every, rung_from=0, start=None,
                     rungs=None, one_sided=False, watch=None):
    """The composed draw; ``ids``: the Q R chain ids, Q even.  ``start`` with ``rungs``, or neither (fresh chains).
    ``watch(spins_before, rungs, move_index, Move)`` is called at every move."""
    ids = np.asarray(ids, dtype=np.uint32)
    R = np.asarray(ladder).size
    assert ids.size % (2 * R) == 0 and (start is None) == (rungs is None)
    spins, rung = start, rungs
    accepted, attempts, sizes, differ, moves, coins, last = 0, 0, [], [], [], [], None
    for move, first, sweeps in schedule(sweep0, n_sweeps, cluster_every, start is None):
        if move is not None:
            m = cluster_move(plan, spins, rung, R, rung_from, int(ids[0]), seed, move, one_sided)
            if watch is not None:
                watch(spins, rung, move, m)
            spins = m.spins
            sizes.append(m.sizes)
            differ.append(m.differ)
            moves.append(move)
        last = tempered_oracle.tempered(plan, hs, Js, ladder, ids, seed, first, sweeps, swap_every, start=spins, rungs=rung)
        spins, rung = last.spins, last.rungs
        accepted, attempts = accepted + last.accepted, attempts + last.attempts
        coins += last.coins
    shape = (0, ids.size // (2 * R), R)
    return Composed(last, accepted, attempts, np.array(sizes, dtype=np.uint32).reshape((len(sizes),) + shape[1:]),
                    np.array(differ, dtype=np.uint32).reshape((len(differ),) + shape[1:]), np.array(moves, dtype=np.int64), coins)


def energies(plan, hs, Js, spins):
    """E(s) = hs.s + sum_e Js_e s_i s_j per row, float64."""
    s = np.asarray(spins, dtype=np.float64)
    return s @ np.asarray(hs, dtype=np.float64) + (s[:, np.asarray(plan.edge_i)] * s[:, np.asarray(plan.edge_j)]) @ np.asarray(Js, dtype=np.float64)
