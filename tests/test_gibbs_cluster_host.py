"""CPU-side checks of the isoenergetic cluster move ("DVG ICM v1", ``dvg_gibbs_cluster_move`` in include/dvg.h) and of the draw
composed of it and the exchange draw (``GibbsSampler.sample_tempered_cluster``): the symbol, every rejection of the C entry point
(before any HIP call, nothing written) and of the Python surface (before the library is touched), the schedule of the moves by
counting, and the definition itself (``tests/cluster_oracle.py``): the law against enumeration, and the exact invariants -- which
a move that flips the cluster in one twin only breaks."""
import ctypes
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as co  # noqa: E402
import tempered_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dvg_gibbs_cluster_move"


# ------------------------------------------------------------------------------------------------ the symbol and its checks
def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported(NAME, markers=["DVG ICM v1", "STREAM_ICM = 7"], kernels=["gibbs_quantum_kernel"])
    assert "STREAM_ICM = 7" in open(os.path.join(ROOT, "image-generation_amd", "csrc", "philox.h")).read()
    assert support.prof_kernel_names()[-1] == "gibbs_cluster_kernel"


def test_argument_validation_without_gpu():
    """Everything the header lists is rejected with a message before any HIP call, and nothing is written: state, rung and the
    two outputs are host memory here, and keep their bytes."""
    L = _lib.lib()
    graph = ctypes.create_string_buffer(4096)  # a host-memory stand-in for the graph handle (first field: the spin count)
    ctypes.c_int32.from_buffer(graph).value = 64
    g = ctypes.cast(graph, ctypes.c_void_p)
    bufs = [ctypes.create_string_buffer(bytes([7]) * 4096) for _ in range(4)]
    state, rung, sizes, differ = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]

    def call(g=g, state=state, rung=rung, n_chains=8, R=4, rung_from=0):
        rc = L.dvg_gibbs_cluster_move(g, state, rung, n_chains, R, rung_from, 0, 0, 0, sizes, differ, None)
        return rc, L.dvg_last_error()

    rc, msg = call(g=None)
    assert rc == -1 and b"g is null" in msg
    rc, msg = call(state=None)
    assert rc == -1 and b"state is null" in msg
    for R in (-1, 0, 17, 64):
        rc, msg = call(R=R, n_chains=2 * max(R, 1))
        assert rc == -1 and b"n_replicas" in msg, (R, rc, msg)
    for R in (2, 4, 16):
        rc, msg = call(rung=None, R=R, n_chains=2 * R)
        assert rc == -1 and b"rung is null" in msg, (R, rc, msg)
    for n_chains in (1, 0, -8):
        rc, msg = call(n_chains=n_chains, R=1)
        assert rc == -1 and b"n_chains" in msg, (n_chains, rc, msg)
    for R, C in ((4, 4), (4, 12), (3, 8), (1, 3), (16, 16)):
        rc, msg = call(R=R, n_chains=C)
        assert rc == -1 and b"multiple" in msg, (R, C, rc, msg)
    for R, rung_from in ((4, -1), (4, 4), (1, 1), (16, 100)):
        rc, msg = call(R=R, n_chains=2 * R, rung_from=rung_from)
        assert rc == -1 and b"rung_from" in msg, (R, rung_from, rc, msg)
    ctypes.c_int32.from_buffer(graph).value = 65537  # beyond the LDS image: unsupported, not invalid
    rc, msg = call()
    assert rc == -4 and b"LDS" in msg
    rc, msg = call(rung=None, R=1, n_chains=2)
    assert rc == -4
    assert all(b.raw[:4096] == bytes([7]) * 4096 for b in bufs), "a rejected call wrote something"


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture
def untouched(monkeypatch):
    """A sampler on a 12-spin ring, with the library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch)
    plan = support.ring_plan()
    n = plan.n
    s = smp.GibbsSampler(plan, list(range(n)), beta=2.0, sweeps=5, seed=3, device="cuda")
    lin, quad = torch.zeros(n), torch.zeros(plan.n_edges)
    return s, lin, quad


def test_sample_tempered_cluster_rejects_bad_arguments(untouched):
    s, lin, quad = untouched
    n, ok = s.plan.n, [0.1, 1.0, 2.0]
    call = lambda **kw: s.sample_tempered_cluster(lin, quad, 1.0, None, None, ok, **kw)  # noqa: E731
    with pytest.raises(TypeError):
        call(num_ladders=2)  # how often?
    for bad in (1, 3, 7, 0, -2, 2.5, True, None):
        with pytest.raises((ValueError, TypeError), match="num_ladders"):
            call(num_ladders=bad, cluster_every=2)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="cluster_every"):
            call(num_ladders=2, cluster_every=bad)
    for bad in (-1, 3, 16, 0.5, True):
        with pytest.raises(ValueError, match="rung_from"):
            call(num_ladders=2, cluster_every=2, rung_from=bad)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="swap_every"):
            call(num_ladders=2, cluster_every=2, swap_every=bad)
        with pytest.raises(ValueError, match="num_sweeps"):
            call(num_ladders=2, cluster_every=2, num_sweeps=bad)
    start, rungs = torch.ones((6, n), dtype=torch.int8), torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="start and rungs"):
        call(num_ladders=2, cluster_every=2, start=start)
    with pytest.raises(ValueError, match="start and rungs"):
        call(num_ladders=2, cluster_every=2, rungs=rungs)
    with pytest.raises(_lib.DvgError, match="num_ladders"):
        call(num_ladders=4, cluster_every=2, start=start, rungs=rungs)
    with pytest.raises(_lib.DvgError, match="GPU"):
        call(num_ladders=2, cluster_every=2, start=start, rungs=rungs)  # a CPU start state
    with pytest.raises(_lib.DvgError):  # valid arguments, CPU parameters: the HIP path has no CPU fallback
        call(num_ladders=2, cluster_every=2)
    with pytest.raises(ValueError):
        s.sample_tempered_cluster(lin, quad, 1.0, None, None, [0.1, -1.0], num_ladders=2, cluster_every=2)
    assert (s.pt_sweep_count, s.ais_sweep_count, s.anneal_sweep_count, s.sweep_count, s.calls, s.cond_sweep_count) == (0,) * 6


def test_cluster_move_rejects_bad_arguments(untouched):
    s, _lin, _quad = untouched
    n = s.plan.n
    state, rungs = torch.ones((8, n), dtype=torch.int8), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(TypeError):
        s.cluster_move(state)  # which move?
    for bad in (0, 17, -1, 1.5, True):
        with pytest.raises(ValueError, match="replicas"):
            s.cluster_move(state, rungs, replicas=bad, move=0)
    for bad in (-1, 4, 0.5):
        with pytest.raises(ValueError, match="rung_from"):
            s.cluster_move(state, rungs, replicas=4, rung_from=bad, move=0)
    for bad in (-1, 2 ** 32, 0.5, None):
        with pytest.raises((ValueError, TypeError), match="move"):
            s.cluster_move(state, rungs, replicas=4, move=bad)
    with pytest.raises(ValueError, match="rungs"):
        s.cluster_move(state, None, replicas=4, move=0)
    with pytest.raises(_lib.DvgError, match="state"):
        s.cluster_move(state.float(), rungs, replicas=4, move=0)  # (in place: no copy is made for the caller)
    with pytest.raises(_lib.DvgError, match="state"):
        s.cluster_move(torch.ones((8, n + 1), dtype=torch.int8), rungs, replicas=4, move=0)
    with pytest.raises(_lib.DvgError, match="state"):
        s.cluster_move(torch.ones((12, n), dtype=torch.int8), torch.zeros(12, dtype=torch.int32), replicas=4, move=0)
    with pytest.raises(_lib.DvgError, match="state"):
        s.cluster_move(torch.ones((3, n), dtype=torch.int8), replicas=1, move=0)
    with pytest.raises(_lib.DvgError, match="state"):
        s.cluster_move(torch.ones((8, 2 * n), dtype=torch.int8)[:, ::2], rungs, replicas=4, move=0)
    with pytest.raises(_lib.DvgError, match="rungs"):
        s.cluster_move(state, rungs[:7], replicas=4, move=0)
    with pytest.raises(_lib.DvgError, match="rungs"):
        s.cluster_move(state, rungs.float(), replicas=4, move=0)
    with pytest.raises(_lib.DvgError, match="GPU"):
        s.cluster_move(state, rungs, replicas=4, move=0)
    with pytest.raises(_lib.DvgError, match="GPU"):
        s.cluster_move(state, replicas=1, move=0)
    assert s.pt_sweep_count == 0


def test_grbm_sample_tempered_cluster_takes_the_local_sampler_only(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    s, _lin, _quad = untouched
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for other in (object(), smp.GibbsSampler(s.plan, [f"q{i}" for i in range(12)], beta=2.0, sweeps=5, seed=3, device="cuda")):
        with pytest.raises(TypeError):
            grbm.sample_tempered_cluster(other, [0.5, 1.0], prefactor=1.0, num_ladders=2, cluster_every=2)
    with pytest.raises(ValueError, match="num_ladders"):
        grbm.sample_tempered_cluster(s, [0.5, 1.0], prefactor=1.0, num_ladders=3, cluster_every=2)


def test_result_objects():
    sizes, differ = torch.tensor([3, 0, 2, 0, 0, 4], dtype=torch.int32), torch.tensor([6, 0, 2, 0, 1, 8], dtype=torch.int32)
    m = smp.ClusterMoves.from_outputs(sizes, differ, 3)
    assert m.sizes.shape == (2, 3) and m.sizes.dtype == torch.int64 and torch.equal(m.differ, differ.view(2, 3).long())
    assert np.array_equal(m.moved_share.numpy(), np.array([3 / 6, 0 / 1, 6 / 10]))
    assert np.array_equal(m.mean_size.numpy(), np.array([3 / 1, 0 / 1, 6 / 2]))
    none = smp.ClusterMoves.from_outputs(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), 2)
    assert torch.isnan(none.moved_share).all() and torch.isnan(none.mean_size).all()


# ------------------------------------------------------------------------------------------------ the schedule, by counting
SCHEDULES = [(0, 12, 3), (3, 12, 3), (3, 12, 4), (8, 7, 4), (5, 60, 2), (7, 3, 10), (10, 1, 10), (9, 1, 10), (4, 9, 1), (0, 1, 1), (6, 5, 100)]


@pytest.mark.parametrize("sweep0,S,every", SCHEDULES)
@pytest.mark.parametrize("fresh", [True, False])
def test_the_moves_come_before_the_expected_sweeps(sweep0, S, every, fresh):
    """The rule, written out: a move of index t / every before sweep t iff t % every == 0, but never before the first sweep of
    fresh chains; between the moves one exchange draw each; every call ends on sweeps."""
    got = smp.cluster_schedule(sweep0, S, every, fresh)
    before = [t for t in range(sweep0, sweep0 + S) if t % every == 0 and not (fresh and t == sweep0)]
    assert [first for move, first, _n in got if move is not None] == before
    assert [move for move, _first, _n in got if move is not None] == [t // every for t in before]
    assert all(move is None for move, first, _n in got if first not in before) and sum(move is None for move, _f, _n in got) <= 1
    assert got[0][1] == sweep0 and all(n >= 1 for _m, _f, n in got) and sum(n for _m, _f, n in got) == S
    assert all(a[1] + a[2] == b[1] for a, b in zip(got, got[1:]))  # (the segments follow each other without a gap)
    assert got == co.schedule(sweep0, S, every, fresh)


@pytest.mark.parametrize("sweep0,S,every", SCHEDULES[:8])
@pytest.mark.parametrize("fresh", [True, False])
def test_the_draw_makes_the_scheduled_calls_in_order(monkeypatch, sweep0, S, every, fresh):
    """sample_tempered_cluster with the move and the exchange draw replaced by counters: the calls, their order, the sweeps of each
    draw, what is handed on, and the counter."""
    n, R, Q = 12, 3, 4
    ei = np.arange(n, dtype=np.int64)
    s = smp.GibbsSampler(graphs.build_plan(n, ei[:-1], ei[1:]), list(range(n)), beta=2.0, sweeps=5, seed=3, device="cuda")
    s.pt_sweep_count = sweep0
    start = None if fresh else torch.ones((Q * R, n), dtype=torch.int8)
    rungs = None if fresh else torch.arange(Q * R, dtype=torch.int32) % R
    log, returned = [], []

    def arguments(_lin, _quad, betas, num_ladders, num_sweeps, swap_every, start, rungs):
        return SimpleNamespace(ladder=np.asarray(betas, np.float32), R=R, Q=num_ladders, S=num_sweeps, swap_every=swap_every, burn_in=0,
                               thin=1, M=None, start=start, rungs=rungs, lin=torch.zeros(n), quad=torch.zeros(n - 1))

    def draw(a, _prefactor, _lr, _qr):
        log.append(("sweeps", s.pt_sweep_count, a.S, a.start, a.rungs))
        first = s.pt_sweep_count
        s.pt_sweep_count += a.S
        state, rung = torch.full((Q * R, n), len(log), dtype=torch.int8), torch.full((Q * R,), len(log), dtype=torch.int32)
        returned.append((state, rung))
        out =smp.Tempered.from_draw(n, R, torch.zeros((Q * R, n)), torch.zeros(Q * R, dtype=torch.float64),
                                     torch.ones(Q * R, dtype=torch.int32), first, a.S, a.swap_every, state, rung)
        return out, None, None, None

    def move(state, rungs, *, replicas, rung_from, move):
        log.append(("move", move, state, rungs, replicas, rung_from))
        return smp.ClusterMoves.from_outputs(torch.full((Q // 2 * R,), move, dtype=torch.int32), torch.zeros(Q // 2 * R, dtype=torch.int32), R)

    monkeypatch.setattr(s, "_tempered_arguments", arguments)
    monkeypatch.setattr(s, "_tempered_draw", draw)
    monkeypatch.setattr(s, "cluster_move", move)
    res = s.sample_tempered_cluster(None, None, 1.0, None, None, [0.5, 1.0, 2.0], num_ladders=Q, num_sweeps=S, swap_every=2,
                                    cluster_every=every, rung_from=1, start=start, rungs=rungs)
    want = co.schedule(sweep0, S, every, fresh)
    flat = [("move", m) if kind == "move" else ("sweeps", f, k) for m, f, k in want for kind in (("move", "sweeps") if m is not None else ("sweeps",))]
    assert [e[:2] if e[0] == "move" else e[:3] for e in log] == flat
    assert log[-1][0] == "sweeps" and s.pt_sweep_count == sweep0 + S
    prev, moved, draws = None, None, iter(returned)
    for e in log:  # (a move changes, in place, the state of the draw before it or its own copy of `start`; the next draw gets it)
        if e[0] == "move":
            _kind, _m, st, rg, reps, first_rung = e
            assert (reps, first_rung) == (R, 1) and (st.dtype, tuple(st.shape)) == (torch.int8, (Q * R, n))
            if prev is None:
                assert st is not start and torch.equal(st, start) and rg is rungs
            else:
                assert st is prev[0] and rg is prev[1]
            moved = st
        else:
            _kind, _t, _k, st, rg = e
            assert st is (moved if moved is not None else start if prev is None else prev[0])
            assert rg is (rungs if prev is None else prev[1])
            prev, moved = next(draws), None
    moves =[m for m, _f, _k in want if m is not None]
    assert np.array_equal(res.moves, np.asarray(moves, dtype=np.int64)) and res.moves.dtype == np.int64
    assert tuple(res.sizes.shape) == (len(moves), Q // 2, R) == tuple(res.differ.shape)
    assert all(int(res.sizes[k, 0, 0]) == m for k, m in enumerate(moves))
    assert np.array_equal(res.tempered.attempts, tempered_oracle.attempts(R, sweep0, S, 2))
    assert torch.equal(res.tempered.accepted, torch.full((Q, R - 1), len(want), dtype=torch.int64))
    assert int(res.tempered.state[0, 0]) == len(log) and int(res.tempered.rungs[0]) == len(log)


# ------------------------------------------------------------------------------------------------ the definition, sampled
@functools.lru_cache(maxsize=None)
def _case16(sixteenths=False):
    """The 16-spin random graph of the exchange draw's host test with its normal (h, J), ladder (0.2, 0.5, 1, 2), 512 ladders:
    256 twin pairs.  ``sixteenths``: h and J rounded to multiples of 1/16 -- every float64 energy sum is exact in any order."""
    n = 16
    rng = np.random.default_rng(16)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.uniform(size=iu.size) < 0.3
    plan = graphs.build_plan(n, iu[keep].astype(np.int64), ju[keep].astype(np.int64))
    h = (0.5 * rng.normal(size=n)).astype(np.float32)
    J = rng.normal(size=plan.n_edges).astype(np.float32)
    if sixteenths:
        h, J = (np.round(h * 16) / 16).astype(np.float32), (np.round(J * 16) / 16).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 1.0, (-4, 4), (-1, 1))
    ladder = np.array([0.2, 0.5, 1.0, 2.0], dtype=np.float32)
    Q = 512
    ids = np.arange(Q * ladder.size, dtype=np.uint32) + 11
    exact = [tempered_oracle.boltzmann_energy_moments(n, hs, Js, np.asarray(plan.edge_i), np.asarray(plan.edge_j), float(b))
             for b in ladder]
    return plan, hs, Js, ladder, Q, ids, exact


def _pair_energies(plan, hs, Js, spins, rungs, R):
    """(pairs, R): the mean of the two twins' energies at every rung, float64."""
    E = co.energies(plan, hs, Js, spins)
    P = spins.shape[0] // (2 * R)
    out = np.empty((P, R))
    for p in range(P):
        out[p] = 0.5 * (E[co.holders(rungs, R, 2 * p)] + E[co.holders(rungs, R, 2 * p + 1)])
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_composed_draw_samples_the_boltzmann_distribution_of_every_rung(seed):
    """60 sweeps from sweep 5, an exchange after each, a move in front of every second, one more move behind the last: the mean
    over the 256 twin pairs of the pair's mean energy at rung r lies within 5 exact sigma / sqrt(256) of the enumerated Boltzmann
    mean at beta_r.  (The variance of a pair's mean is at most sigma^2 however the twins are correlated.)"""
    plan, hs, Js, ladder, Q, ids, exact = _case16()
    R = ladder.size
    r = co.tempered_cluster(plan, hs, Js, ladder, ids, seed, 5, 60, 1, 2, 0)
    assert np.array_equal(r.moves, np.arange(3, 33)) and r.sizes.shape == (30, Q // 2, R)
    last = co.cluster_move(plan, r.tempered.spins, r.tempered.rungs, R, 0, int(ids[0]), seed, 33)
    means = _pair_energies(plan, hs, Js, last.spins, r.tempered.rungs, R).mean(axis=0)
    z = np.array([(means[k] - m) / (sd / np.sqrt(Q // 2)) for k, (m, sd) in enumerate(exact)])
    print(f"seed {seed}: per-rung mean pair energy off by {np.round(z, 2)} exact sigma / sqrt(pairs); mean cluster per rung "
          f"{np.round(r.sizes.sum(axis=(0, 1)) / np.maximum((r.differ > 0).sum(axis=(0, 1)), 1), 2)} of {plan.n} spins")
    assert (np.abs(z) <= 5.0).all(), z
    assert (r.sizes <= r.differ).all() and ((r.sizes > 0) == (r.differ > 0)).all() and (r.sizes > 1).any()
    assert (np.sort(r.tempered.rungs.reshape(-1, R), axis=1) == np.arange(R)).all() and r.accepted.sum() > 0


def _invariants(one_sided):
    """The composed draw of the law test (seed 1) on (h, J) in sixteenths, watched at every move.  Returns the largest change of
    a pair's energy sum over all moves, whether D ever changed, and whether the same move again ever failed to restore."""
    plan, hs, Js, ladder, Q, ids, _exact = _case16(True)
    R = ladder.size
    worst = dict(energy=0.0, differ=False, undo=False, moves=0)

    def watch(before, rungs, move, m):
        e0 = _pair_energies(plan, hs, Js, before, rungs, R)
        e1 = _pair_energies(plan, hs, Js, m.spins, rungs, R)
        worst["energy"] = max(worst["energy"], float(np.abs(e1 - e0).max()) * 2.0)
        a = np.concatenate([co.holders(rungs, R, 2 * p) for p in range(Q // 2)])
        b = np.concatenate([co.holders(rungs, R, 2 * p + 1) for p in range(Q // 2)])
        worst["differ"] |= not np.array_equal((before[a] < 0) != (before[b] < 0), (m.spins[a] < 0) != (m.spins[b] < 0))
        back = co.cluster_move(plan, m.spins, rungs, R, 0, int(ids[0]), 1, move, one_sided)
        worst["undo"] |= not (np.array_equal(back.spins, before) and np.array_equal(back.sizes, m.sizes))
        worst["moves"] += 1

    co.tempered_cluster(plan, hs, Js, ladder, ids, 1, 5, 60, 1, 2, 0, one_sided=one_sided, watch=watch)
    assert worst["moves"] == 30
    return worst


def test_every_move_keeps_the_pair_energy_and_the_disagreement_set_and_undoes_itself():
    """Exactly: with (h, J) in sixteenths every energy is a sum of multiples of 1/16 far below 2^53 / 16, exact in any order."""
    w = _invariants(False)
    assert w["energy"] == 0.0 and not w["differ"] and not w["undo"], w


def test_the_invariants_have_teeth():
    """The move that flips the cluster in one twin only -- which the law test cannot tell from the definition within its
    margin -- changes a pair's energy sum."""
    w = _invariants(True)
    assert w["energy"] > 0.0, w
