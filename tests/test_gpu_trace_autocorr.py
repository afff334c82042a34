"""GPU checks of ``dvg_trace_autocorr`` ("DVG acf v1") -- per spin the sums over chains of s(m) s(m + t), of s(m), and per chain
of s(m), over bit-packed records -- against numpy int64 sums (``tests/autocorr_oracle.py``): exact equality, the results are
integers.  Records: traced draws (``dvg_gibbs_sample_traced``) on ``pegasus64`` (two whole words) and ``zephyr1024`` (32
words), and random words with noise in the bits of spins >= n for n = 77, 33 and 1.  (records, max_lag): below, at and over one
64-record word, several words with a partial last one, lags that are multiples of 64; chains 1, 3 and 41 (several per
workgroup).  A guard element behind each output; ``accumulate = 1`` adds onto nonzero outputs; ``chain_sum = NULL``.  And the
Python surface built on it, with two checks of the estimates themselves: chains at beta = 0 are white noise, chains at
beta = 20 are at least four times slower."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import autocorr_oracle as ao  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -0x0123456789ABCDEF
GUARD32 = -0x01234567
SHAPES = [(1, 0), (2, 1), (63, 62), (64, 63), (65, 64), (130, 129), (200, 70), (200, 128)]  # (records M, max_lag L)
CHAINS = [1, 3, 41]
P = dict(h_scale=0.05, j_scale=5.0, prefactor=0.05)


_solver_plan = functools.partial(support.solver_plan, with_nodes=True)


def _fields(plan):
    rng = np.random.default_rng(plan.n)
    h = (P["h_scale"] * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (P["j_scale"] * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    return torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()


@functools.lru_cache(maxsize=None)
def _case(name):
    """``(n, bits (C, M, W) int32 on the device)``, computed once: a traced draw at beta = 20 of 41 chains x 200 records
    (``pegasus64``) or 3 chains x 130 records (``zephyr1024``), or 41 x 200 records of random words (``random77``,
    ``random33``, ``random1``).  The tests take the first chains and records of it."""
    if name.startswith("random"):
        n = int(name[6:])
        W = (n + 31) // 32
        noise = np.random.default_rng(n).integers(0, 2 ** 32, size=(41, 200, W), dtype=np.uint64).astype(np.uint32)
        if n % 32:
            assert (noise[..., -1] >> np.uint32(n % 32)).any()  # bits of spins >= n are set
        return n, torch.from_numpy(noise.view(np.int32)).cuda()
    plan = _solver_plan("pegasus", 64)[0] if name == "pegasus64" else _solver_plan("zephyr", 1024)[0]
    C, S = (41, 200) if name == "pegasus64" else (3, 130)
    gh = smp.GraphHandle(plan, "cuda")
    lin, quad = _fields(plan)
    state = torch.empty((C, plan.n), dtype=torch.int8, device="cuda")
    traced = torch.empty((C, S, (plan.n + 31) // 32), dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().dvg_gibbs_sample_traced(gh.ptr, lin.data_ptr(), quad.data_ptr(), P["prefactor"], -4.0, 4.0, -1.0, 1.0, 20.0,
                                                  state.data_ptr(), C, 1000, SEED, 6, S, 1, None, traced.data_ptr(), 0, 1, None,
                                                  _lib.stream_ptr()), "dvg_gibbs_sample_traced")
    torch.cuda.synchronize()
    return plan.n, traced


def _outputs(C, n, L, rng=None):
    """``lag_sum``, ``spin_sum``, ``chain_sum`` with a guard element behind each; ``rng``: None (a fill to be overwritten) or a
    generator (nonzero int64 values to add onto)."""
    outs = []
    for k in ((L + 1) * n, n):
        v = np.full(k + 1, 0x7777777777, dtype=np.int64) if rng is None else rng.integers(-10 ** 12, 10 ** 12, size=k + 1)
        v[k] = GUARD
        outs.append(torch.from_numpy(v).cuda())
    v = np.full(C * n + 1, 0x777777, dtype=np.int32)
    v[C * n] = GUARD32
    return outs + [torch.from_numpy(v).cuda()]


def _raw(bits, C, M, n, L, lag_sum, spin_sum, chain_sum, accumulate):
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    rc = _lib.lib().dvg_trace_autocorr(ptr(bits), C, M, n, L, ptr(lag_sum), ptr(spin_sum), ptr(chain_sum), accumulate, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _check_exact(name, C, M, L):
    n, full = _case(name)
    bits = full[:C, :M].contiguous()
    want = ao.lag_sums(bits.cpu().numpy().view(np.uint32), n, L)
    assert np.array_equal(want[0][0], np.full(n, C * M)) and want[2].dtype == np.int32
    lag_sum, spin_sum, chain_sum = _outputs(C, n, L)
    assert _raw(bits, C, M, n, L, lag_sum, spin_sum, chain_sum, 0) == 0, _lib.lib().dvg_last_error()
    got = lag_sum.cpu().numpy(), spin_sum.cpu().numpy(), chain_sum.cpu().numpy()
    assert got[0][-1] == GUARD and got[1][-1] == GUARD and got[2][-1] == GUARD32, "written past an output"
    assert np.array_equal(got[0][:-1].reshape(L + 1, n), want[0])
    assert np.array_equal(got[1][:-1], want[1]) and np.array_equal(got[2][:-1].reshape(C, n), want[2])
    # accumulate = 1 adds onto nonzero lag_sum and spin_sum; chain_sum = NULL is accepted
    lag_sum, spin_sum, _unused = _outputs(C, n, L, rng=np.random.default_rng(M))
    base = lag_sum.cpu().numpy().copy(), spin_sum.cpu().numpy().copy()
    assert _raw(bits, C, M, n, L, lag_sum, spin_sum, None, 1) == 0, _lib.lib().dvg_last_error()
    got = lag_sum.cpu().numpy(), spin_sum.cpu().numpy()
    assert got[0][-1] == GUARD and got[1][-1] == GUARD
    assert np.array_equal(got[0][:-1], base[0][:-1] + want[0].reshape(-1)) and np.array_equal(got[1][:-1], base[1][:-1] + want[1])


@pytest.mark.parametrize("C", CHAINS)
@pytest.mark.parametrize("M,L", SHAPES)
@pytest.mark.parametrize("name", ["pegasus64", "random77"])
def test_sums_are_exact(name, M, L, C):
    _check_exact(name, C, M, L)


@pytest.mark.parametrize("name,C,M,L", [("random33", 3, 65, 64), ("random33", 41, 200, 128), ("random33", 1, 130, 129),
                                        ("random1", 1, 1, 0), ("random1", 3, 64, 63), ("random1", 41, 200, 70),
                                        ("zephyr1024", 3, 130, 129)])
def test_sums_are_exact_on_other_widths(name, C, M, L):
    _check_exact(name, C, M, L)


def test_the_trace_rows_are_the_draws_records():
    """The traced cases hold spins that move: some but not all of a chain's records differ from its first."""
    for name in ("pegasus64", "zephyr1024"):
        _n, bits = _case(name)
        moved = (bits != bits[:, :1]).any(-1)
        assert moved.any() and not moved.all()


def test_invalid_arguments_launch_nothing():
    n, bits = _case("pegasus64")
    C, M, L = 3, 10, 4
    bits = bits[:C, :M].contiguous()
    lag_sum, spin_sum, chain_sum = _outputs(C, n, L)
    before = lag_sum.clone(), spin_sum.clone(), chain_sum.clone()
    for args, code in (((None, C, M, n, L, lag_sum, spin_sum), -1), ((bits, C, M, n, L, None, spin_sum), -1),
                       ((bits, C, M, n, L, lag_sum, None), -1), ((bits, 0, M, n, L, lag_sum, spin_sum), -1),
                       ((bits, C, 0, n, 0, lag_sum, spin_sum), -1), ((bits, C, M, 0, L, lag_sum, spin_sum), -1),
                       ((bits, C, M, n, -1, lag_sum, spin_sum), -1), ((bits, C, M, n, M, lag_sum, spin_sum), -1),
                       ((bits, C, 16385, n, L, lag_sum, spin_sum), -4)):
        assert _raw(*args, chain_sum, 0) == code, args[1:5]
    assert torch.equal(lag_sum, before[0]) and torch.equal(spin_sum, before[1]) and torch.equal(chain_sum, before[2])


# ------------------------------------------------------------------------------------------------ the Python surface
def _sampler(plan, nodes, beta=20.0, sweeps=4):
    return smp.GibbsSampler(plan, nodes, beta=beta, sweeps=sweeps, seed=SEED, persistent=True, chain_offset=5, h_range=(-4, 4),
                            j_range=(-1, 1))


def _same(a, b):
    assert (a.chains, a.records, a.thin, a.max_lag) == (b.chains, b.records, b.thin, b.max_lag)
    assert torch.equal(a.lag_sum, b.lag_sum) and torch.equal(a.spin_sum, b.spin_sum)
    assert (a.chain_sum is None) == (b.chain_sum is None) and (a.chain_sum is None or torch.equal(a.chain_sum, b.chain_sum))


def _sums_of(a, bits, n):
    want = ao.lag_sums(bits.cpu().numpy().view(np.uint32), n, a.max_lag)
    assert np.array_equal(a.lag_sum.cpu().numpy(), want[0]) and np.array_equal(a.spin_sum.cpu().numpy(), want[1])
    if a.chain_sum is not None:
        assert np.array_equal(a.chain_sum.cpu().numpy(), want[2])
    return want


def test_trace_autocorrelation_and_the_functional_wrapper():
    plan, nodes = _solver_plan("zephyr", 128)
    lin, quad = _fields(plan)
    s = _sampler(plan, nodes)
    trace = s.sample_trace(lin, quad, P["prefactor"], (-4, 4), (-1, 1), num_reads=9, num_sweeps=32, burn_in=2, thin=3)
    assert trace.bits.shape == (9, 10, 4) and trace.thin == 3
    a = trace.autocorrelation()
    assert isinstance(a, smp.Autocorrelation) and (a.chains, a.records, a.thin, a.max_lag) == (9, 10, 3, 9)
    assert a.lag_sum.is_cuda and a.lag_sum.dtype == torch.int64 and a.chain_sum.dtype == torch.int32 and a.chain_sum.shape == (9, 128)
    want = _sums_of(a, trace.bits, plan.n)
    assert a.rho.is_cuda and a.rho.dtype == torch.float64 and a.rho.shape == (10, 128) and a.r_hat.shape == (128,)
    assert np.allclose(a.tau_int.cpu().numpy(), ao.tau_int(want[0], want[1], 9, 10)[0], rtol=1e-12, atol=0, equal_nan=True)
    assert torch.equal(a.tau_int_sweeps, a.tau_int * 3)
    b = trace.autocorrelation(max_lag=4, chain_sums=False)
    assert b.max_lag == 4 and b.chain_sum is None and torch.equal(b.lag_sum, a.lag_sum[:5])
    with pytest.raises(ValueError, match="r_hat"):
        b.r_hat
    with pytest.raises(ValueError, match="max_lag"):
        trace.autocorrelation(10)
    # out= adds onto existing sums (pooling traces); chain_sum stays this trace's own
    lag_sum, spin_sum, chain_sum = F.trace_autocorr(trace.bits, plan.n, 9)
    again = F.trace_autocorr(trace.bits, plan.n, 9, out=(lag_sum, spin_sum))
    assert again[0] is lag_sum and again[1] is spin_sum and torch.equal(again[2], chain_sum)
    assert torch.equal(lag_sum, 2 * a.lag_sum) and torch.equal(spin_sum, 2 * a.spin_sum)
    with pytest.raises(_lib.DvgError, match="lag_sum"):
        F.trace_autocorr(trace.bits, plan.n, 4, out=(lag_sum, spin_sum))
    # the sampler's other counters and chains are untouched
    assert (s.trace_sweep_count, s.sweep_count, s.calls, s.ais_sweep_count, s.pt_sweep_count) == (32, 0, 0, 0, 0) and s._state is None


def test_grbm_mixing_is_the_autocorrelation_of_the_same_trace():
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    plan, nodes = _solver_plan("zephyr", 128)
    lin, quad = _fields(plan)
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                           np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    with torch.no_grad():
        grbm._linear.copy_(lin)
        grbm._quadratic.copy_(quad)
    kw = dict(prefactor=P["prefactor"], linear_range=(-4, 4), quadratic_range=(-1, 1), num_reads=9, num_sweeps=40, burn_in=4, thin=2)
    s1, s2 = _sampler(plan, nodes), _sampler(plan, nodes)
    want = grbm.sample_trace(s1, **kw).autocorrelation(7)
    got = grbm.mixing(s2, max_lag=7, **kw)
    assert isinstance(got, smp.Autocorrelation) and (got.chains, got.records, got.thin, got.max_lag) == (9, 18, 2, 7)
    _same(got, want)
    assert s2.trace_sweep_count == 40 and (s2.sweep_count, s2.calls) == (0, 0) and s2._state is None
    _same(grbm.mixing(_sampler(plan, nodes), **kw), grbm.sample_trace(_sampler(plan, nodes), **kw).autocorrelation())  # max_lag: M - 1
    with pytest.raises(TypeError):
        grbm.mixing(object(), prefactor=0.05, num_reads=2)


def test_model_wrapper_prior_mixing():
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    m.overlap_sampler = False  # (as in the moments file: this test takes no stream from the process's pool)
    a = m.prior_mixing(max_lag=5, num_reads=33, num_sweeps=20, burn_in=6, thin=2)
    s = m.sampler
    assert (s.trace_sweep_count, s.sweep_count, s.calls, s.ais_sweep_count) == (20, 0, 0, 0) and s._state is None
    assert isinstance(a, smp.Autocorrelation) and (a.chains, a.records, a.thin, a.max_lag) == (33, 7, 2, 5)
    assert a.lag_sum.is_cuda and a.tau_int.shape == (64,) and a.tau_int.dtype == torch.float64
    s.reset()  # the same draw again, by hand
    trace = m._grbm.sample_trace(s, prefactor=m.PREFACTOR, linear_range=m.linear_range, quadratic_range=m.quadratic_range,
                                 num_reads=33, num_sweeps=20, burn_in=6, thin=2)
    assert trace.bits.shape == (33, 7, 2)
    _same(a, trace.autocorrelation(5))
    _sums_of(a, trace.bits, 64)


# ------------------------------------------------------------------------------------------------ the estimates themselves
@functools.lru_cache(maxsize=None)
def _chains_at(beta):
    """``pegasus64``: 32 chains, 128 sweeps, every sweep recorded, lags 0 .. 16."""
    plan, nodes = _solver_plan("pegasus", 64)
    lin, quad = _fields(plan)
    s = _sampler(plan, nodes, beta=beta, sweeps=128)
    return s.sample_trace(lin, quad, P["prefactor"], (-4, 4), (-1, 1), num_reads=32).autocorrelation(16)


def test_hot_chains_are_white_noise():
    """At beta = 0 every sweep redraws every spin uniformly: rho[t, i] is, up to the pooled mean's O(1 / (C M)), a mean of
    C (M - t) independent +-1, so |rho[t, i]| <= 6 / sqrt(C (M - t)) -- six standard deviations -- at each of the 8 x 64
    (lag, spin) pairs t = 1 .. 8."""
    a = _chains_at(0.0)
    assert (a.chains, a.records, a.thin) == (32, 128, 1)
    rho = a.rho.cpu().numpy()
    z = np.abs(rho[1:9]) * np.sqrt(a.counts[1:9].astype(np.float64))[:, None]
    print(f"hot chains: the largest |rho| in standard deviations {z.max():.2f}; tau_int <= {float(a.tau_int.max()):.3f}")
    assert z.shape == (8, 64) and (z <= 6.0).all()


def test_cold_chains_are_slower():
    """At beta = 20 the same chains barely move: the smallest tau_int is at least 4 times the largest at beta = 0 (over the
    spins whose tau_int is not NaN) -- a condition a broken estimator fails, not a measurement."""
    hot, cold = _chains_at(0.0).tau_int.cpu().numpy(), _chains_at(20.0).tau_int.cpu().numpy()
    hot, cold = hot[~np.isnan(hot)], cold[~np.isnan(cold)]
    print(f"tau_int at beta = 0: <= {hot.max():.3f}; at beta = 20: >= {cold.min():.3f} ({cold.size} spins, "
          f"{int(_chains_at(20.0).truncated.sum())} truncated)")
    assert hot.size == 64 and cold.size >= 1 and cold.min() >= 4.0 * hot.max()
