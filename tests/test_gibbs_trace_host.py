"""CPU-side checks of the traced draw ("DVG trace v1", ``dvg_gibbs_sample_traced`` in include/dvg.h) and of the moments of
packed rows (``dvg_grbm_moments_packed``): the symbols, every argument error of the two C entry points (before any HIP
call) and of the Python surface (before the library is touched), the draw's own key and counter, which sweeps a call
records, the bit layout's round trip, ``Moments``, the plan a traced draw takes, and the estimator the trace is for -- time
averages over the helper's history (``tests/trace_oracle.py``) against enumeration."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, dev, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

NAMES = ("dvg_gibbs_sample_traced", "dvg_grbm_moments_packed")


# ------------------------------------------------------------------------------------------------ the symbols and their checks
def test_symbols_are_declared_bound_and_exported():
    support.assert_declared_bound_exported(NAMES, markers=["DVG trace v1"])


_stand_in = support.graph_stand_in


def _traced(g, lin, quad, state, trace, *, n_chains=8, n_sweeps=7, burn_in=0, thin=1, dyn=None):
    L = _lib.lib()
    rc = L.dvg_gibbs_sample_traced(g, lin, quad, 1.0, -1, 1, -1, 1, 1.0, state, n_chains, 0, 0, 0, n_sweeps, 1, None, trace, burn_in,
                                   thin, dyn, None)
    return rc, L.dvg_last_error()


def test_traced_draw_argument_validation_without_gpu():
    """Everything the header lists is DVG_E_INVALID (-1) with a message, before any HIP call."""
    rc, msg = _traced(None, None, None, None, None)
    assert rc == -1 and b"null" in msg
    graph, g, p, _keep = _stand_in()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p)):
        rc, msg = _traced(g, *args)
        assert rc == -1 and b"null" in msg
    rc, msg = _traced(g, p, p, p, None)
    assert rc == -1 and b"trace_out" in msg and b"dvg_gibbs_sample" in msg
    for n_chains in (0, -4):
        rc, msg = _traced(g, p, p, p, p, n_chains=n_chains)
        assert rc == -1 and b"n_chains" in msg
    rc, msg = _traced(g, p, p, p, p, n_sweeps=-1)
    assert rc == -1 and b"n_sweeps" in msg
    for burn_in in (-1, -100):
        rc, msg = _traced(g, p, p, p, p, burn_in=burn_in)
        assert rc == -1 and b"burn_in" in msg
    for thin in (0, -1):
        rc, msg = _traced(g, p, p, p, p, thin=thin)
        assert rc == -1 and b"thin" in msg
    # M < 1: nothing recorded
    for S, burn_in, thin in ((0, 0, 1), (7, 7, 1), (7, 8, 1), (7, 0, 8), (7, 5, 3), (7, 2 ** 31 - 1, 2 ** 31 - 1), (3, 0, 2 ** 31 - 1)):
        rc, msg = _traced(g, p, p, p, p, n_sweeps=S, burn_in=burn_in, thin=thin)
        assert rc == -1 and b"record nothing" in msg and b"dvg_gibbs_sample" in msg, (S, burn_in, thin, rc, msg)
    rc, msg = _traced(g, p, p, p, p, dyn=p)
    assert rc == -1 and b"dyn" in msg
    ctypes.c_int32.from_buffer(graph).value = 40000
    rc, msg = _traced(g, p, p, p, p)
    assert rc == -1 and b"too large" in msg


def test_moments_argument_validation_without_gpu():
    L = _lib.lib()
    _graph, g, p, _keep = _stand_in()
    for args in ((None, p, 5, p, p), (g, None, 5, p, p), (g, p, 5, None, p), (g, p, 5, p, None)):
        rc = L.dvg_grbm_moments_packed(*args, 0, None)
        assert rc == -1 and b"null" in L.dvg_last_error()
    for rows in (0, -1, -2 ** 40):
        rc = L.dvg_grbm_moments_packed(g, p, rows, p, p, 0, None)
        assert rc == -1 and b"rows" in L.dvg_last_error()


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture
def untouched(monkeypatch):
    """A sampler on a 12-spin ring, with the library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch)
    plan = _ring_plan()
    s = smp.GibbsSampler(plan, list(range(plan.n)), beta=2.0, sweeps=5, seed=3, device="cuda")
    return s, torch.zeros(plan.n), torch.zeros(plan.n_edges)


_ring_plan = support.ring_plan


def test_sample_trace_rejects_bad_arguments(untouched):
    s, lin, quad = untouched
    n = s.plan.n
    call = lambda **kw: s.sample_trace(lin, quad, 1.0, None, None, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="num_reads"):
        call()  # how many chains?
    for bad in (0, -1, 2.5, True, "4"):
        with pytest.raises(ValueError, match="num_reads"):
            call(num_reads=bad)
    for bad in (0, -3, 1.5, True, "7"):
        with pytest.raises(ValueError, match="num_sweeps"):
            call(num_reads=2, num_sweeps=bad)
        with pytest.raises(ValueError, match="thin"):
            call(num_reads=2, thin=bad)
    for bad in (-1, 0.5, True, None):
        with pytest.raises(ValueError, match="burn_in"):
            call(num_reads=2, burn_in=bad)
    # nothing recorded (the sampler's own sweeps: 5)
    for kw in (dict(burn_in=5), dict(burn_in=6), dict(thin=6), dict(burn_in=3, thin=3), dict(num_sweeps=7, burn_in=5, thin=3)):
        with pytest.raises(ValueError, match="record nothing"):
            call(num_reads=2, **kw)
    start = torch.ones((6, n), dtype=torch.int8)
    with pytest.raises(_lib.DvgError, match="start"):
        call(start=np.ones((6, n), dtype=np.int8))
    with pytest.raises(_lib.DvgError, match="start"):
        call(start=torch.ones((6, n + 1), dtype=torch.int8))
    with pytest.raises(_lib.DvgError, match="start"):
        call(start=torch.ones((n,), dtype=torch.int8))
    with pytest.raises(_lib.DvgError, match="start"):
        call(start=torch.ones((0, n), dtype=torch.int8))
    with pytest.raises(_lib.DvgError, match="start"):
        call(start=start.double())
    with pytest.raises(_lib.DvgError, match="num_reads"):
        call(start=start, num_reads=5)
    with pytest.raises(_lib.DvgError, match="GPU"):
        call(start=start)  # a CPU start state
    with pytest.raises(_lib.DvgError):  # valid arguments, CPU parameters: the HIP path has no CPU fallback
        call(num_reads=2)
    assert (s.trace_sweep_count, s.pt_sweep_count, s.ais_sweep_count, s.anneal_sweep_count, s.sweep_count, s.calls,
            s.cond_sweep_count) == (0,) * 7


def test_traced_draws_have_their_own_key_and_counter(untouched):
    s, _lin, _quad = untouched
    assert s.trace_seed == 3 ^ 0x74726163 and s.trace_sweep_count == 0
    assert s.trace_seed not in (s.seed, s.cond_seed, s.anneal_seed, s.ais_seed, s.pt_seed)
    s.trace_sweep_count, s.pt_sweep_count, s.sweep_count = 5, 6, 7
    s.reset()
    assert (s.trace_sweep_count, s.pt_sweep_count, s.sweep_count) == (0, 0, 0)


def test_grbm_trace_methods_take_the_local_sampler_only(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    s, _lin, _quad = untouched
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for other in (object(), smp.GibbsSampler(s.plan, [f"q{i}" for i in range(12)], beta=2.0, sweeps=5, seed=3, device="cuda")):
        with pytest.raises(TypeError):
            grbm.sample_trace(other, prefactor=1.0, num_reads=2)
        with pytest.raises(TypeError):
            grbm.model_moments(other, prefactor=1.0, num_reads=2)


def test_functional_wrapper_rejects_bad_rows(untouched):
    from image_generation_amd import functional as F

    class Handle:  # (what the wrapper reads before the library: the plan)
        plan = _ring_plan()
        ptr = None

    for bad in (torch.zeros((4, 2), dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int64), torch.zeros((0, 1), dtype=torch.int32),
                torch.zeros((4,), dtype=torch.int32), np.zeros((4, 1), dtype=np.int32)):
        with pytest.raises(_lib.DvgError, match="bits"):
            F.grbm_moments_packed(bad, Handle)
    with pytest.raises(_lib.DvgError):  # a CPU tensor of the right shape: the HIP path has no CPU fallback
        F.grbm_moments_packed(torch.zeros((4, 1), dtype=torch.int32), Handle)


# ------------------------------------------------------------------------------------------------ which sweeps are recorded
@pytest.mark.parametrize("S,burn_in,thin,M,last", [(7, 0, 1, 7, True), (7, 1, 2, 3, True), (7, 2, 3, 1, False), (7, 6, 1, 1, True)])
def test_records_and_recorded_sweeps(S, burn_in, thin, M, last):
    by_rule = trace_oracle.recorded_sweeps(S, burn_in, thin)
    got = smp.trace_sweeps(S, burn_in, thin)
    assert got.dtype == np.int64 and got.shape == (M,) and np.array_equal(got, by_rule)
    assert M == (S - burn_in) // thin
    assert (got[-1] == S) == last
    if not last:
        assert S - got[-1] == 2  # two trailing sweeps unrecorded
    # record m holds the state after sweep k = burn_in + thin (m + 1) - 1
    assert np.array_equal(got - 1, burn_in + thin * (np.arange(M) + 1) - 1)
    t = smp.Trace(torch.zeros((3, M, 1), dtype=torch.int32), None, None, got, 12)
    assert np.array_equal(t.sweeps, by_rule) and t.unpack().shape == (3, M, 12)


# ------------------------------------------------------------------------------------------------ the layout
@pytest.mark.parametrize("n", [1, 31, 32, 33, 77])
def test_pack_unpack_round_trip_on_cpu(n):
    rng = np.random.default_rng(n)
    states = np.where(rng.uniform(size=(3, 4, n)) < 0.5, -1, 1).astype(np.int8)
    states[0, 0], states[0, 1] = 1, -1
    words = trace_oracle.pack(states)
    W = (n + 31) // 32
    assert words.shape == (3, 4, W) and words.dtype == np.uint32
    # bit b of word w is spin 32 w + b; bits of spins >= n are 0
    for i in range(n):
        assert np.array_equal((words[..., i // 32] >> np.uint32(i % 32)) & 1, (states[..., i] > 0).astype(np.uint32))
    if n % 32:
        assert (words[..., -1] >> np.uint32(n % 32) == 0).all()
    bits = torch.from_numpy(words.view(np.int32))
    t = smp.Trace(bits, None, None, np.arange(1, 5), n)
    got = t.unpack()
    assert got.dtype == torch.float32 and got.shape == (3, 4, n) and not got.is_cuda
    assert np.array_equal(got.numpy(), states.astype(np.float32))
    assert torch.equal(smp.pack_spins(torch.from_numpy(states.astype(np.float32))), bits)
    assert np.array_equal(trace_oracle.unpack(words, n), states)
    # bits of spins >= n set at random are ignored by unpack
    if n % 32:
        noisy = words.copy()
        noisy[..., -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
        assert np.array_equal(smp.unpack_spins(torch.from_numpy(noisy.view(np.int32)), n).numpy(), states.astype(np.float32))


def test_moments_from_sums_on_cpu():
    rng = np.random.default_rng(5)
    plan = _ring_plan()
    rows = np.where(rng.uniform(size=(37, plan.n)) < 0.4, -1, 1).astype(np.int8)
    spin_sum, pair_sum = trace_oracle.moments(rows, plan.edge_i, plan.edge_j)
    assert spin_sum.dtype == np.int64 and pair_sum.dtype == np.int64
    assert np.array_equal(spin_sum, rows.astype(np.int64).sum(0))
    assert np.array_equal(pair_sum, np.array([(rows[:, i].astype(np.int64) * rows[:, j]).sum() for i, j in zip(plan.edge_i, plan.edge_j)]))
    again = trace_oracle.moments_of_bits(trace_oracle.pack(rows), plan.n, plan.edge_i, plan.edge_j)
    assert np.array_equal(again[0], spin_sum) and np.array_equal(again[1], pair_sum)
    m = smp.Moments.from_sums(torch.from_numpy(spin_sum), torch.from_numpy(pair_sum), 37)
    assert m.count == 37 and m.mean_spin.dtype == torch.float64 and m.mean_pair.dtype == torch.float64
    assert np.array_equal(m.mean_spin.numpy(), spin_sum / 37.0) and np.array_equal(m.mean_pair.numpy(), pair_sum / 37.0)
    assert m.spin_sum.dtype == torch.int64 and m.pair_sum.shape == (plan.n_edges,)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            smp.Moments.from_sums(torch.from_numpy(spin_sum), torch.from_numpy(pair_sum), bad)
    with pytest.raises(ValueError):
        smp.Moments.from_sums(torch.from_numpy(spin_sum).float(), torch.from_numpy(pair_sum), 37)


# ------------------------------------------------------------------------------------------------ the plan
_solver_plan = support.solver_plan


_random_plan = functools.partial(support.random_plan, isolated=3)


_clique_plan = support.clique_plan


# the nine shapes of tests/test_gpu_gibbs_ais.py: graph, chains, gibbs_generic, the form its draw takes
NINE = [
    ("pegasus64", lambda: _solver_plan("pegasus", 64), 5, 0, ("lane", dict(LPC=32, WAVES=1, MB=4, NR=1, MAXS=12))),
    ("zephyr128", lambda: _solver_plan("zephyr", 128), 5, 0, ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12))),
    ("zephyr512", lambda: _solver_plan("zephyr", 512), 9, 0, ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=12))),
    ("zephyr512-one-row", lambda: _solver_plan("zephyr", 512), 9, 2, ("lane", dict(LPC=64, WAVES=4, MB=5, NR=1, MAXS=12))),
    ("zephyr512-rolled", lambda: _solver_plan("zephyr", 512), 9, 1, ("rolled", dict(LPC=64, WAVES=4))),
    ("zephyr1024x41", lambda: _solver_plan("zephyr", 1024), 41, 0, ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20))),
    ("zephyr1024x530", lambda: _solver_plan("zephyr", 1024), 530, 0, ("rolled", dict(LPC=64, WAVES=16))),
    ("random77", _random_plan, 19, 0, ("rolled", dict(LPC=16, WAVES=1))),
    ("cliques", _clique_plan, 21, 0, ("lane", dict(LPC=64, WAVES=4, MB=4, NR=1, MAXS=20))),
]


@pytest.mark.parametrize("name,make,C,generic,form", NINE, ids=[s[0] for s in NINE])
def test_trace_plan_is_the_table_plan(name, make, C, generic, form):
    plan = make()
    for option in sorted({generic, 0, 1, 2, 3, 4}):
        with _lib.option_scope(gibbs_generic=option):
            trace, table = dev.gibbs_draw_plan(plan, C, "trace"), dev.gibbs_draw_plan(plan, C, "table")
        assert trace == table, (option, trace, table)  # field for field
        if option == generic:
            assert (trace["form"], trace["params"]) == form, trace
    with pytest.raises(KeyError):
        dev.gibbs_draw_plan(plan, C, "exchange")  # (planned by gibbs_exchange_plan)


# ------------------------------------------------------------------------------------------------ the estimator
RING_SEED = 20261019


@functools.lru_cache(maxsize=None)
def _ring_case():
    """A 12-spin ring with uniform (h, J) at beta = 0.8: 64 chains, 250 sweeps, burn_in 50, thin 2 -> 100 records a chain."""
    plan = _ring_plan()
    rng = np.random.default_rng(12)
    h = (0.5 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = rng.uniform(-1, 1, plan.n_edges).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 1.0, (-4, 4), (-1, 1))
    ids = np.arange(64, dtype=np.uint32) + 11
    return plan, hs, Js, 0.8, ids


def test_time_averages_of_a_trace_estimate_the_model_moments():
    """Each of the 24 moments (12 <s_i>, 12 <s_i s_j>) of the time average over all records lies within 6 standard errors of
    enumeration over the 2^12 states.  The standard error: the between-chain standard deviation of the per-chain time
    averages over sqrt(64) -- the chains are independent, so this holds whatever the autocorrelation within a chain."""
    plan, hs, Js, beta, ids = _ring_case()
    tr = trace_oracle.trace(plan, hs, Js, beta, ids, RING_SEED ^ 0x74726163, 0, 250, burn_in=50, thin=2)
    C, M = 64, 100
    assert tr.bits.shape == (C, M, 1) and tr.sweeps[0] == 52 and tr.sweeps[-1] == 250
    s = trace_oracle.unpack(tr.bits, plan.n).astype(np.float64)  # (C, M, n)
    per_chain = np.concatenate([s.mean(axis=1), (s[..., plan.edge_i] * s[..., plan.edge_j]).mean(axis=1)], axis=1)  # (C, 24)
    est, se = per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(C)
    exact = np.concatenate(trace_oracle.exact_moments(plan.n, hs, Js, plan.edge_i, plan.edge_j, beta))
    z = (est - exact) / se
    print(f"24 moments off by {np.round(z, 2)} standard errors; the largest standard error {se.max():.4f}")
    assert est.shape == (24,) and (se > 0).all() and (np.abs(z) <= 6.0).all(), z
    # the integer sums over all records are the same estimate
    spin_sum, pair_sum = trace_oracle.moments_of_bits(tr.bits, plan.n, plan.edge_i, plan.edge_j)
    m = smp.Moments.from_sums(torch.from_numpy(spin_sum), torch.from_numpy(pair_sum), C * M)
    assert np.allclose(np.concatenate([m.mean_spin.numpy(), m.mean_pair.numpy()]), est, rtol=0, atol=1e-12)
    # (teeth: the moments are not trivially 0 -- the exact values are many standard errors from it)
    assert (np.abs(exact) > 6.0 * se).sum() >= 12
