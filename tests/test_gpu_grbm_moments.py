"""GPU checks of ``dvg_grbm_moments_packed`` -- the sums over bit-packed rows of s_i and, per edge, of s_i s_j -- against
numpy int64 sums (``tests/trace_oracle.py``): exact equality, the results are integers.  Rows: traced draws' records
(``dvg_gibbs_sample_traced``) and rows of random words whose bits of spins >= n are set at random and must be ignored.
Row counts 1, 35, 63, 64, 65, 287 = 41 x 7 (a tile is 64 rows: below one, one short, exact, one over, several with a tail) on
``pegasus64`` (two whole words a row), ``random77`` (a partial last word) and ``zephyr1024`` (32 words).  A guard
element behind each output; ``accumulate = 1`` adds onto nonzero outputs.  And the Python surface built on it."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -0x0123456789ABCDEF
ROWS = [1, 35, 63, 64, 65, 287]
GRAPHS = ["pegasus64", "random77", "zephyr1024"]


_solver_plan = functools.partial(support.solver_plan, with_nodes=True)


_random_plan = functools.partial(support.random_plan, isolated=3)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The graph, its handle, and 287 rows of each kind on the device: a traced draw of 41 chains x 7 records, and random
    words.  Computed once per graph; the tests take the first ``rows`` rows."""
    plan = {"pegasus64": lambda: _solver_plan("pegasus", 64)[0], "random77": _random_plan,
            "zephyr1024": lambda: _solver_plan("zephyr", 1024)[0]}[name]()
    p = dict(h_scale=0.5, j_scale=2.0, prefactor=0.3, beta=1.5) if name == "random77" else dict(h_scale=0.05, j_scale=5.0,
                                                                                               prefactor=0.05, beta=20.0)
    rng = np.random.default_rng(plan.n)
    h = (p["h_scale"] * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (p["j_scale"] * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    gh = smp.GraphHandle(plan, "cuda")
    C, S, W = 41, 7, (plan.n + 31) // 32
    state = torch.empty((C, plan.n), dtype=torch.int8, device="cuda")
    traced = torch.empty((C * S, W), dtype=torch.int32, device="cuda")
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    _lib.check(_lib.lib().dvg_gibbs_sample_traced(gh.ptr, lin.data_ptr(), quad.data_ptr(), p["prefactor"], -4.0, 4.0, -1.0, 1.0,
                                                  p["beta"], state.data_ptr(), C, 1000, SEED, 6, S, 1, None, traced.data_ptr(), 0, 1,
                                                  None, _lib.stream_ptr()), "dvg_gibbs_sample_traced")
    torch.cuda.synchronize()
    noise = rng.integers(0, 2 ** 32, size=(C * S, W), dtype=np.uint64).astype(np.uint32)
    if plan.n % 32:
        assert (noise[:, -1] >> np.uint32(plan.n % 32)).any()  # bits of spins >= n are set
    return plan, gh, {"trace": traced, "noise": torch.from_numpy(noise.view(np.int32)).cuda()}


def _outputs(plan, rng=None):
    """``spin_sum`` and ``pair_sum`` with a guard element behind each; ``rng``: None (a fill to be overwritten) or a generator
    (nonzero values to add onto)."""
    outs = []
    for k in (plan.n, plan.n_edges):
        v = np.full(k + 1, 0x7777777777, dtype=np.int64) if rng is None else rng.integers(-10 ** 12, 10 ** 12, size=k + 1)
        v[k] = GUARD
        outs.append(torch.from_numpy(v).cuda())
    return outs


def _raw(gh, bits, rows, spin_sum, pair_sum, accumulate):
    rc = _lib.lib().dvg_grbm_moments_packed(gh.ptr, bits.data_ptr() if bits is not None else None, rows,
                                            spin_sum.data_ptr() if spin_sum is not None else None,
                                            pair_sum.data_ptr() if pair_sum is not None else None, accumulate, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("kind", ["trace", "noise"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", GRAPHS)
def test_moments_of_packed_rows_are_exact(name, rows, kind):
    plan, gh, inputs = _case(name)
    bits = inputs[kind][:rows].contiguous()
    want = trace_oracle.moments_of_bits(bits.cpu().numpy().view(np.uint32), plan.n, plan.edge_i, plan.edge_j)
    spin_sum, pair_sum = _outputs(plan)
    assert _raw(gh, bits, rows, spin_sum, pair_sum, 0) == 0, _lib.lib().dvg_last_error()
    got = spin_sum.cpu().numpy(), pair_sum.cpu().numpy()
    assert got[0][plan.n] == GUARD and got[1][plan.n_edges] == GUARD, "written past an output"
    assert np.array_equal(got[0][:plan.n], want[0]) and np.array_equal(got[1][:plan.n_edges], want[1])
    assert np.abs(want[0]).max() <= rows and (want[0] % 2 == rows % 2).all()  # (sums of `rows` values +-1)
    # accumulate = 1 adds onto nonzero outputs
    rng = np.random.default_rng(rows)
    spin_sum, pair_sum = _outputs(plan, rng=rng)
    base = spin_sum.cpu().numpy().copy(), pair_sum.cpu().numpy().copy()
    assert _raw(gh, bits, rows, spin_sum, pair_sum, 1) == 0
    got = spin_sum.cpu().numpy(), pair_sum.cpu().numpy()
    assert got[0][plan.n] == GUARD and got[1][plan.n_edges] == GUARD
    assert np.array_equal(got[0][:plan.n], base[0][:plan.n] + want[0]) and np.array_equal(got[1][:plan.n_edges], base[1][:plan.n_edges] + want[1])


def test_the_trace_rows_are_the_draws_records():
    """The rows of the `trace` kind are spins, not noise: their moments over all 287 rows equal the sums over the unpacked
    records, and a chain's spins do move between records."""
    plan, _gh, inputs = _case("random77")
    words = inputs["trace"].cpu().numpy().view(np.uint32)
    assert (words[:, -1] >> np.uint32(plan.n % 32) == 0).all()
    s = trace_oracle.unpack(words, plan.n)
    assert set(np.unique(s).tolist()) == {-1, 1} and len({r.tobytes() for r in s}) > 41


def test_invalid_arguments_launch_nothing():
    plan, gh, inputs = _case("pegasus64")
    bits = inputs["trace"]
    spin_sum, pair_sum = _outputs(plan)
    before = spin_sum.clone(), pair_sum.clone()
    for args in ((None, 5, spin_sum, pair_sum), (bits, 5, None, pair_sum), (bits, 5, spin_sum, None), (bits, 0, spin_sum, pair_sum),
                 (bits, -3, spin_sum, pair_sum)):
        assert _raw(gh, *args, 0) == -1, args[1]
    assert torch.equal(spin_sum, before[0]) and torch.equal(pair_sum, before[1])


def test_functional_wrapper_and_suffstats_agree():
    """``functional.grbm_moments_packed`` is the entry point; its means agree with ``dvg_grbm_suffstats(scale = 1 / rows)`` over
    the same rows unpacked to float32 -- within the float32 rounding of THAT call's output (its sums are exact in float64;
    scale = fl32(1 / rows) and the product's rounding to float32 are 2^-24 relative each): the packed result is the exact one."""
    plan, gh, inputs = _case("zephyr1024")
    rows = 287
    bits = inputs["trace"][:rows]
    spin_sum, pair_sum = F.grbm_moments_packed(bits, gh)
    want = trace_oracle.moments_of_bits(bits.cpu().numpy().view(np.uint32), plan.n, plan.edge_i, plan.edge_j)
    assert spin_sum.dtype == torch.int64 and spin_sum.shape == (plan.n,) and pair_sum.shape == (plan.n_edges,) and spin_sum.is_cuda
    assert np.array_equal(spin_sum.cpu().numpy(), want[0]) and np.array_equal(pair_sum.cpu().numpy(), want[1])
    again = F.grbm_moments_packed(bits, gh, out=(spin_sum, pair_sum))  # adds onto them
    assert again[0] is spin_sum and np.array_equal(spin_sum.cpu().numpy(), 2 * want[0]) and np.array_equal(pair_sum.cpu().numpy(), 2 * want[1])
    m = smp.Moments.from_sums(*F.grbm_moments_packed(bits, gh), rows)

    x = smp.unpack_spins(bits, plan.n).contiguous()
    L = _lib.lib()
    acc_l = torch.empty(plan.n, dtype=torch.float32, device="cuda")
    acc_q = torch.empty(plan.n_edges, dtype=torch.float32, device="cuda")
    ws = torch.empty(L.dvg_grbm_suffstats_workspace_bytes(gh.ptr), dtype=torch.uint8, device="cuda")
    _lib.check(L.dvg_grbm_suffstats(gh.ptr, x.data_ptr(), rows, None, 1.0 / rows, acc_l.data_ptr(), acc_q.data_ptr(), 0, ws.data_ptr(),
                                    ws.numel(), _lib.stream_ptr()), "dvg_grbm_suffstats")
    torch.cuda.synchronize()
    for exact, f32 in ((m.mean_spin, acc_l), (m.mean_pair, acc_q)):
        exact, f32 = exact.cpu().numpy(), f32.cpu().numpy().astype(np.float64)
        err, tol = np.abs(f32 - exact), 2.0 ** -23 * (1.0 + 2.0 ** -20) * np.abs(exact)
        print(f"suffstats against the exact means: worst error {err.max():.3e}, its tolerance {tol[err.argmax()]:.3e}")
        assert (err <= tol).all()


def _moments_of(trace, gh):
    m = trace.moments(gh)
    want = trace_oracle.moments_of_bits(trace.bits.cpu().numpy().view(np.uint32), gh.plan.n, gh.plan.edge_i, gh.plan.edge_j)
    C, M, _W = trace.bits.shape
    assert m.count == C * M and np.array_equal(m.spin_sum.cpu().numpy(), want[0]) and np.array_equal(m.pair_sum.cpu().numpy(), want[1])
    return m


def test_grbm_model_moments_are_the_moments_of_the_same_trace():
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    plan, nodes = _solver_plan("zephyr", 128)
    rng = np.random.default_rng(2)
    h = (0.05 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    mk = lambda: smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5,  # noqa: E731
                                  h_range=(-4, 4), j_range=(-1, 1))
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                           np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    with torch.no_grad():
        grbm._linear.copy_(torch.from_numpy(h).cuda())
        grbm._quadratic.copy_(torch.from_numpy(J).cuda())
    kw = dict(prefactor=0.05, linear_range=(-4, 4), quadratic_range=(-1, 1), num_reads=9, num_sweeps=12, burn_in=2, thin=3)
    s1, s2 = mk(), mk()
    trace = grbm.sample_trace(s1, **kw)
    assert isinstance(trace, smp.Trace) and trace.bits.shape == (9, 3, 4) and s1.trace_sweep_count == 12
    m = _moments_of(trace, grbm.graph_handle("cuda"))
    mean_spin, mean_pair = grbm.model_moments(s2, **kw)
    assert mean_spin.shape == grbm._linear.shape and mean_pair.shape == grbm._quadratic.shape and mean_spin.dtype == torch.float64
    assert torch.equal(mean_spin, m.mean_spin) and torch.equal(mean_pair, m.mean_pair) and s2.trace_sweep_count == 12
    assert (s2.sweep_count, s2.calls) == (0, 0) and s2._state is None
    with pytest.raises(TypeError):
        grbm.model_moments(object(), prefactor=0.05, num_reads=2)


def test_model_wrapper_prior_moments():
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    m.overlap_sampler = False  # (as in the AIS file: this test takes no stream from the process's pool)
    mean_spin, mean_pair = m.prior_moments(num_reads=33, num_sweeps=20, burn_in=6, thin=2)
    s = m.sampler
    assert (s.trace_sweep_count, s.sweep_count, s.calls, s.ais_sweep_count) == (20, 0, 0, 0) and s._state is None
    assert mean_spin.shape == m._grbm._linear.shape and mean_pair.shape == m._grbm._quadratic.shape
    assert mean_spin.dtype == torch.float64 and mean_spin.is_cuda and (mean_spin.abs() <= 1).all() and (mean_pair.abs() <= 1).all()
    s.reset()  # the same draw again, by hand
    trace = m._grbm.sample_trace(s, prefactor=m.PREFACTOR, linear_range=m.linear_range, quadratic_range=m.quadratic_range,
                                 num_reads=33, num_sweeps=20, burn_in=6, thin=2)
    assert trace.bits.shape == (33, 7, 2)
    want = _moments_of(trace, m._grbm.graph_handle(trace.bits.device))
    assert torch.equal(mean_spin.reshape(-1), want.mean_spin) and torch.equal(mean_pair.reshape(-1), want.mean_pair)
