"""CPU-side checks of the traced exchange draw ("DVG PT trace v1", ``dvg_gibbs_sample_tempered_traced`` in include/dvg.h): the
symbol, every argument error of the C entry point (before any HIP call) and of ``GibbsSampler.sample_tempered_trace`` (before
the library is touched), the ladder diagnostics of ``sampler.TemperedTrace`` on hand-written walks, the definition helper
(``tests/tempered_trace_oracle.py``) against ``tests/tempered_oracle.py`` on the shapes of the GPU tests, and the statistics of
the helper's records on a 12-spin ring against enumeration."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tempered_oracle  # noqa: E402
import tempered_trace_oracle as tto  # noqa: E402
import test_gpu_gibbs_tempered as shapes  # noqa: E402  (TABLE, parameters, SEED, SWEEP0: no GPU is touched by importing it)
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

NAME = "dvg_gibbs_sample_tempered_traced"


# ------------------------------------------------------------------------------------------------ the symbol and its checks
def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported(NAME, markers=["DVG PT trace v1"], arity={NAME: 29})
    assert "No traced form of" not in support.header_text()  # (the sentence that said there was none)


def _call(g, lin, quad, state, ladder, rung, trace, *, R=4, swap_every=1, n_chains=8, n_sweeps=7, burn_in=0, thin=1, dyn=None,
          energy_trace=None, rung_trace=None):
    L = _lib.lib()
    rc = L.dvg_gibbs_sample_tempered_traced(g, lin, quad, 1.0, -1, 1, -1, 1, ladder, R, swap_every, state, rung, n_chains, 0, 0, 0,
                                            n_sweeps, 1, None, None, None, trace, energy_trace, rung_trace, burn_in, thin, dyn, None)
    return rc, L.dvg_last_error()


def test_argument_validation_without_gpu():
    """Everything the header lists is DVG_E_INVALID (-1) with a message under the entry point's own name, before any HIP call:
    the pointers are host-memory stand-ins."""
    rc, msg = _call(None, None, None, None, None, None, None)
    assert rc == -1 and b"null" in msg and b"gibbs_tempered_traced" in msg
    graph = ctypes.create_string_buffer(4096)  # a host-memory stand-in for the graph handle (first field: the spin count)
    ctypes.c_int32.from_buffer(graph).value = 64
    g = ctypes.cast(graph, ctypes.c_void_p)
    dummy = ctypes.create_string_buffer(16)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    # what the exchange draw rejects
    for lin, quad, state in ((None, p, p), (p, None, p), (p, p, None)):
        rc, msg = _call(g, lin, quad, state, p, p, p)
        assert rc == -1 and b"null" in msg
    rc, msg = _call(g, p, p, p, None, p, p)
    assert rc == -1 and b"ladder" in msg
    rc, msg = _call(g, p, p, p, p, None, p)
    assert rc == -1 and b"rung" in msg
    for R in (-1, 0, 1, 17, 64):
        rc, msg = _call(g, p, p, p, p, p, p, R=R, n_chains=max(R, 1) * 2)
        assert rc == -1 and b"n_replicas" in msg, (R, rc, msg)
    for R, C in ((4, 6), (3, 8), (16, 8), (2, 7)):
        rc, msg = _call(g, p, p, p, p, p, p, R=R, n_chains=C)
        assert rc == -1 and b"multiple" in msg, (R, C, rc, msg)
    for n_chains in (0, -4):
        rc, msg = _call(g, p, p, p, p, p, p, n_chains=n_chains)
        assert rc == -1 and b"n_chains" in msg
    for swap_every in (0, -1):
        rc, msg = _call(g, p, p, p, p, p, p, swap_every=swap_every)
        assert rc == -1 and b"swap_every" in msg
    for n_sweeps in (0, -1):
        rc, msg = _call(g, p, p, p, p, p, p, n_sweeps=n_sweeps)
        assert rc == -1 and b"n_sweeps" in msg
    rc, msg = _call(g, p, p, p, p, p, p, dyn=p)
    assert rc == -1 and b"dyn" in msg
    # its own
    rc, msg = _call(g, p, p, p, p, p, None, energy_trace=p, rung_trace=p)
    assert rc == -1 and b"trace_out" in msg and b"dvg_gibbs_sample_tempered" in msg
    for burn_in in (-1, -100):
        rc, msg = _call(g, p, p, p, p, p, p, burn_in=burn_in)
        assert rc == -1 and b"burn_in" in msg
    for thin in (0, -1):
        rc, msg = _call(g, p, p, p, p, p, p, thin=thin)
        assert rc == -1 and b"thin" in msg
    for S, burn_in, thin in ((7, 7, 1), (7, 8, 1), (7, 0, 8), (7, 5, 3), (7, 2 ** 31 - 1, 2 ** 31 - 1), (3, 0, 2 ** 31 - 1)):
        rc, msg = _call(g, p, p, p, p, p, p, n_sweeps=S, burn_in=burn_in, thin=thin)
        assert rc == -1 and b"record nothing" in msg and b"gibbs_tempered_traced" in msg, (S, burn_in, thin, rc, msg)
    ctypes.c_int32.from_buffer(graph).value = 40000
    rc, msg = _call(g, p, p, p, p, p, p)
    assert rc == -1 and b"too large" in msg


# ------------------------------------------------------------------------------------------------ the Python surface
_ring_plan = support.ring_plan


@pytest.fixture
def untouched(monkeypatch):
    """A sampler on a 12-spin ring, with the library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch)
    plan = _ring_plan()
    s = smp.GibbsSampler(plan, list(range(plan.n)), beta=2.0, sweeps=5, seed=3, device="cuda")
    return s, torch.zeros(plan.n), torch.zeros(plan.n_edges)


def _counters(s):
    return (s.pt_sweep_count, s.trace_sweep_count, s.ais_sweep_count, s.anneal_sweep_count, s.sweep_count, s.calls, s.cond_sweep_count)


BAD_LADDERS = [
    ([0.1, -0.5, 1.0], ValueError), ([0.1, float("nan")], ValueError), ([0.1, float("inf")], ValueError),
    (np.array([1e39, 1.0]), ValueError), (torch.tensor([0.5, -1.0]), ValueError), ([], _lib.DvgError), ([1.0], _lib.DvgError),
    (np.linspace(0.1, 2.0, 17), _lib.DvgError), (np.ones((2, 4)), _lib.DvgError), (3.0, _lib.DvgError), (["a", "b"], ValueError),
]


@pytest.mark.parametrize("betas,exc", BAD_LADDERS)
def test_sample_tempered_trace_rejects_bad_ladders(untouched, betas, exc):
    s, lin, quad = untouched
    with pytest.raises(exc):
        s.sample_tempered_trace(lin, quad, 1.0, None, None, betas, num_ladders=4)
    assert _counters(s) == (0,) * 7


def test_sample_tempered_trace_rejects_bad_arguments(untouched):
    s, lin, quad = untouched
    n, ok = s.plan.n, [0.1, 1.0, 2.0]
    call = lambda **kw: s.sample_tempered_trace(lin, quad, 1.0, None, None, ok, **kw)  # noqa: E731
    with pytest.raises(TypeError):
        call()  # how many ladders?
    # sample_tempered's
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises((ValueError, TypeError), match="num_ladders"):
            call(num_ladders=bad)
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="swap_every"):
            call(num_ladders=2, swap_every=bad)
        with pytest.raises(ValueError, match="num_sweeps"):
            call(num_ladders=2, num_sweeps=bad)
    start, rungs = torch.ones((6, n), dtype=torch.int8), torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="start and rungs"):
        call(num_ladders=2, start=start)
    with pytest.raises(ValueError, match="start and rungs"):
        call(num_ladders=2, rungs=rungs)
    with pytest.raises(_lib.DvgError, match="start"):
        call(num_ladders=2, start=torch.ones((6, n + 1), dtype=torch.int8), rungs=rungs)
    with pytest.raises(_lib.DvgError, match="start"):
        call(num_ladders=2, start=torch.ones((7, n), dtype=torch.int8), rungs=torch.zeros(7, dtype=torch.int32))
    with pytest.raises(_lib.DvgError, match="start"):
        call(num_ladders=2, start=start.double(), rungs=rungs)
    with pytest.raises(_lib.DvgError, match="rungs"):
        call(num_ladders=2, start=start, rungs=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(_lib.DvgError, match="rungs"):
        call(num_ladders=2, start=start, rungs=rungs.float())
    with pytest.raises(_lib.DvgError, match="num_ladders"):
        call(num_ladders=3, start=start, rungs=rungs)
    with pytest.raises(_lib.DvgError, match="GPU"):
        call(num_ladders=2, start=start, rungs=rungs)  # a CPU start state
    # sample_trace's
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="burn_in"):
            call(num_ladders=2, burn_in=bad)
    for bad in (0, -2, 2.5, True, None):
        with pytest.raises(ValueError, match="thin"):
            call(num_ladders=2, thin=bad)
    for S, burn_in, thin in ((5, 5, 1), (5, 6, 1), (5, 0, 6), (5, 3, 3), (None, 5, 1)):
        with pytest.raises(ValueError, match="record nothing"):
            call(num_ladders=2, num_sweeps=S, burn_in=burn_in, thin=thin)
    with pytest.raises(_lib.DvgError):  # valid arguments, CPU parameters: the HIP path has no CPU fallback
        call(num_ladders=2, burn_in=1, thin=2)
    assert _counters(s) == (0,) * 7


def test_grbm_traced_entries_take_the_local_sampler_only(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    s, _lin, _quad = untouched
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for other in (object(), smp.GibbsSampler(s.plan, [f"q{i}" for i in range(12)], beta=2.0, sweeps=5, seed=3, device="cuda")):
        with pytest.raises(TypeError):
            grbm.sample_tempered_trace(other, [0.5, 1.0], prefactor=1.0, num_ladders=2)
        with pytest.raises(TypeError):
            grbm.tempered_mixing(other, [0.5, 1.0], prefactor=1.0, num_ladders=2)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="max_lag"):
            grbm.tempered_mixing(s, [0.5, 1.0], prefactor=1.0, num_ladders=2, max_lag=bad)
    with pytest.raises(ValueError, match="rung_walk"):
        grbm.tempered_mixing(s, [0.5, 1.0], prefactor=1.0, num_ladders=2, rung_walk=False)


# ------------------------------------------------------------------------------------------------ the ladder diagnostics
def _trace_of_walks(walks, R):
    """A TemperedTrace around hand-written walks: (Q, R, M) rungs by chain (bits and energies are not looked at)."""
    w = torch.tensor(walks, dtype=torch.uint8)
    Q, _R, M = w.shape
    assert _R == R
    return smp.TemperedTrace(torch.zeros((Q, R, M, 1), dtype=torch.int32), None, w, trace_oracle.recorded_sweeps(M, 0, 1), None,
                             np.linspace(0.5, 1.0, R), 12)


def _flow(tt):
    return [None if np.isnan(v) else v for v in tt.flow().tolist()]


def test_a_chain_that_never_leaves_its_rung():
    tt = _trace_of_walks([[[0] * 5, [1] * 5, [2] * 5]], 3)
    assert tt.occupancy().tolist() == [[[5, 0, 0], [0, 5, 0], [0, 0, 5]]] and tt.occupancy().dtype == torch.int64
    assert tt.round_trips().tolist() == [[0, 0, 0]] and tt.round_trips().dtype == torch.int64
    # rung 0 only by an up chain, rung 2 only by a down chain, rung 1 by a chain nobody labelled
    assert _flow(tt) == [1.0, None, 0.0] and tt.flow().dtype == torch.float64


def test_one_clean_round_trip_of_two_rungs():
    tt = _trace_of_walks([[[0, 1, 0], [1, 0, 1]]], 2)
    assert tt.occupancy().tolist() == [[[2, 1], [1, 2]]]
    assert tt.round_trips().tolist() == [[1, 1]]
    assert _flow(tt) == [1.0, 0.0]
    # half a trip is none
    assert _trace_of_walks([[[0, 1], [1, 0]]], 2).round_trips().tolist() == [[0, 0]]


def test_one_clean_round_trip_of_four_rungs():
    #        chain 0: 0 up to 3 and back;  chain 1: starts unlabelled on rung 1, is labelled from rung 0 on
    walk = [[[0, 1, 2, 3, 2, 1, 0], [1, 0, 1, 2, 3, 3, 3], [2, 2, 0, 0, 0, 0, 1], [3, 3, 3, 1, 1, 2, 2]]]
    tt = _trace_of_walks(walk, 4)
    assert tt.occupancy()[0].tolist() == [[2, 2, 2, 1], [1, 2, 1, 3], [4, 1, 2, 0], [0, 2, 2, 3]]
    # labels: chain 0 uuuDDDu (2 changes); chain 1 -uuuDDD (1); chain 2 --uuuuu (0); chain 3 DDDDDDD (0)
    assert tt.round_trips().tolist() == [[1, 0, 0, 0]]
    # rung 0: up x (2 + 1 + 4); rung 1: up 1 + 1 + 1 (chains 0, 1, 2), down 1 + 2 (chains 0, 3);  rung 2: up 1 + 1, down 1 + 2;
    # rung 3: down 1 + 3 + 3 (chain 1's unlabelled record on rung 1 is not counted)
    assert _flow(tt) == [1.0, 3 / 6, 2 / 5, 0.0]


def test_a_chain_that_touches_one_end_only():
    tt = _trace_of_walks([[[1, 0, 1, 1, 0, 1], [0, 1, 0, 0, 1, 0], [2, 2, 2, 2, 2, 2]]], 3)
    assert tt.round_trips().tolist() == [[0, 0, 0]]
    assert tt.occupancy()[0].tolist() == [[2, 4, 0], [4, 2, 0], [0, 0, 6]]
    assert _flow(tt) == [1.0, 1.0, 0.0]  # (rung 1: 3 + 2 labelled records, all up)


def test_a_single_record():
    tt = _trace_of_walks([[[1], [0], [2]], [[2], [1], [0]]], 3)
    assert tt.occupancy().tolist() == [[[0, 1, 0], [1, 0, 0], [0, 0, 1]], [[0, 0, 1], [0, 1, 0], [1, 0, 0]]]
    assert tt.round_trips().tolist() == [[0, 0, 0], [0, 0, 0]]
    assert _flow(tt) == [1.0, None, 0.0] and tt.thin == 1


def test_diagnostics_need_what_they_are_computed_from():
    tt = smp.TemperedTrace(torch.zeros((2, 3, 4, 1), dtype=torch.int32), None, None, trace_oracle.recorded_sweeps(8, 0, 2), None,
                           [0.5, 1.0, 2.0], 12)
    for f in (tt.occupancy, tt.round_trips, tt.flow, tt.energy_series):
        with pytest.raises(ValueError):
            f()
    assert tt.thin == 2 and tt.rung(1).bits.shape == (2, 4, 1) and tt.target.bits.is_contiguous()
    for bad in (3, -4, 1.0, True):
        with pytest.raises(ValueError):
            tt.rung(bad)


def test_diagnostics_against_a_loop_over_the_records():
    """Random walks (not permutations: the counts do not care) against the label rule spelled out as a loop."""
    rng = np.random.default_rng(5)
    Q, R, M = 3, 5, 200
    step = rng.integers(-1, 2, size=(Q, R, M))
    walk = np.clip(np.cumsum(step, axis=2) + rng.integers(0, R, size=(Q, R, 1)), 0, R - 1)
    tt = _trace_of_walks(walk.tolist(), R)
    trips, up, down = np.zeros((Q, R), np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    for q in range(Q):
        for j in range(R):
            label, changes = 0, 0
            for m in range(M):
                new = 1 if walk[q, j, m] == 0 else -1 if walk[q, j, m] == R - 1 else label
                changes += int(label != 0 and new != label)
                label = new
                up[walk[q, j, m]] += label == 1
                down[walk[q, j, m]] += label == -1
            trips[q, j] = changes // 2
    assert trips.sum() > 0 and np.array_equal(tt.round_trips().numpy(), trips)
    assert np.array_equal(tt.flow().numpy(), up / (up + down))
    assert np.array_equal(tt.occupancy().numpy(), (walk[..., None] == np.arange(R)).sum(axis=2))


# ------------------------------------------------------------------------------------------------ the helper is the definition's
RECORD_RULES = ((0, 1), (1, 2), (3, 4))


@functools.lru_cache(maxsize=None)
def traced_definition(name, burn_in, thin):
    """The helper's traced draw of a shape of ``tests/test_gpu_gibbs_tempered.py`` (fresh chains), computed once and shared."""
    plan, _R, _Q, every, sweeps, _generic, _p, _h, _J, hs, Js, ladder, ids = shapes.parameters(name)
    return tto.tempered_traced(plan, hs, Js, ladder, ids, shapes.SEED, shapes.SWEEP0, sweeps, every, burn_in, thin)


@pytest.mark.parametrize("name", shapes.SHAPES)
def test_the_helper_draws_what_the_definition_draws(name):
    """Every non-record output equals ``tempered_oracle.tempered``'s exactly, whatever is recorded; the records are consistent
    with them: the last record of a draw whose last sweep is recorded is the final state, energy and rungs."""
    plan, R, Q, every, sweeps, _generic, _p, _h, _J, hs, Js, ladder, ids = shapes.parameters(name)
    want = tempered_oracle.tempered(plan, hs, Js, ladder, ids, shapes.SEED, shapes.SWEEP0, sweeps, every)
    for burn_in, thin in RECORD_RULES:
        got = traced_definition(name, burn_in, thin)
        for field in ("spins", "rungs", "energy", "A", "samples", "energy_by_rung", "accepted", "attempts"):
            assert np.array_equal(getattr(got.draw, field), getattr(want, field)), (name, field)
        assert got.draw.N == want.N and got.draw.coins == want.coins
        M = (sweeps - burn_in) // thin
        assert got.bits.shape == (Q, R, M, (plan.n + 31) // 32) and got.walk.shape == (Q, R, M) and got.energies.shape == (Q, R, M)
        assert np.array_equal(got.sweeps, trace_oracle.recorded_sweeps(sweeps, burn_in, thin))
        assert (np.sort(got.walk, axis=1) == np.arange(R)[None, :, None]).all()  # a permutation at every record
        if (sweeps - burn_in) % thin == 0:
            assert np.array_equal(got.bits[:, :, -1].reshape(Q * R, -1), trace_oracle.pack(want.samples))
            assert np.array_equal(got.energies[:, :, -1].reshape(-1), want.energy_by_rung)
            assert np.array_equal(got.walk[:, :, -1].reshape(-1), want.rungs)
    # thin = 1 from the first sweep: a chain's records, read by chain through the walk, are its states sweep by sweep
    full = traced_definition(name, 0, 1)
    assert not (full.walk == full.walk[:, :, :1]).all()  # (rungs change hands within the draw)
    q, j = np.divmod(np.arange(Q * R), R)
    last = full.bits[q, full.walk[q, j, -1], -1]
    assert np.array_equal(last, trace_oracle.pack(want.spins))


def test_the_coins_of_the_shapes_are_far_from_ties():
    """The condition of the GPU comparison, on the CPU: every |u - exp(d)| is at least 10^6 times its bound."""
    worst = {}
    for name in shapes.SHAPES:
        coins = traced_definition(name, 0, 1).draw.coins
        assert all(margin >= 1e6 * bound for margin, bound, _a in coins), name
        worst[name] = max([b / m for m, b, _a in coins], default=0.0)
    print("largest bound / margin per shape:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 1e-6


# ------------------------------------------------------------------------------------------------ the records are samples at their rung's beta
RING_SEED = 20261019


def test_ring_records_sample_every_rung_and_ladders_make_round_trips():
    """The 12-spin ring of ``test_energy_packed_host.py`` on the helper alone: 16 ladders of 4 rungs, 400 sweeps with an exchange
    after each, burn_in 100.  A record taken AFTER the exchange is a sample at betas[r]: every rung's mean recorded energy lies
    within 6 standard errors (between ladders) of the enumerated Boltzmann mean at that rung's beta.  Were a record taken before
    the exchange, the rows would be filed under rungs their chains no longer hold.  And ladders wander: round trips happen."""
    plan = _ring_plan()
    rng = np.random.default_rng(12)
    h = (0.5 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = rng.uniform(-1, 1, plan.n_edges).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 1.0, (-4, 4), (-1, 1))
    betas = np.geomspace(0.4, 3.0, 4).astype(np.float32)
    Q, R = 16, 4
    ids = np.arange(Q * R, dtype=np.uint32) + 11
    got = tto.tempered_traced(plan, hs, Js, betas, ids, RING_SEED ^ 0x70743031, 0, 400, 1, burn_in=100, thin=1)
    tt = smp.TemperedTrace(torch.from_numpy(got.bits.astype(np.int32)), torch.from_numpy(got.energies), torch.from_numpy(got.walk),
                           got.sweeps, None, betas, plan.n)
    assert tt.bits.shape == (Q, R, 300, 1) and tt.thin == 1
    # the carried energies are the energies of the recorded states (float32 fields: to rounding)
    spins = trace_oracle.unpack(got.bits, plan.n).astype(np.float64)
    exact_E = spins @ hs.astype(np.float64) + (spins[..., np.asarray(plan.edge_i)] * spins[..., np.asarray(plan.edge_j)]) @ Js.astype(np.float64)
    assert np.abs(exact_E - got.energies).max() <= 1e-4
    for r in range(R):
        s = tt.energy_series(r, max_lag=32)
        mean, _sd = tempered_oracle.boltzmann_energy_moments(plan.n, hs, Js, np.asarray(plan.edge_i), np.asarray(plan.edge_j), float(betas[r]))
        z = (float(s.mean) - mean) / float(s.std_err)
        print(f"rung {r} (beta {betas[r]:.3f}): mean recorded energy {float(s.mean):.4f} against {mean:.4f} exact, {z:+.2f} std_err of "
              f"{float(s.std_err):.4f}; tau_int {float(s.tau_int):.2f} records")
        assert float(s.std_err) > 0 and abs(z) <= 6.0
    trips, flow, occ = tt.round_trips(), tt.flow(), tt.occupancy()
    print(f"round trips per ladder {trips.sum(1).tolist()}; flow {np.round(flow.numpy(), 3).tolist()}; acceptance "
          f"{(got.draw.accepted.sum(axis=0)[:-1] / (Q * got.draw.attempts)).round(3).tolist()}")
    assert int((trips.sum(1) > 0).sum()) >= 1
    assert (occ.sum(2) == 300).all() and (occ.sum(1) == 300).all()  # a permutation at every record
    assert flow[0] == 1.0 and flow[-1] == 0.0 and bool((flow[1:-1] > 0).all()) and bool((flow[1:-1] < 1).all())
