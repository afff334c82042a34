"""GPU parity of the weighed annealed draw (``dvg_gibbs_sample_ais``, "DVG AIS v1": the annealed draw plus, per chain, the
log importance weight of annealed importance sampling and the energy of the returned state) against the definition in
``tests/ais_oracle.py``, and of the Python surface built on it.

Spins: equal to the helper's, bit for bit (they are the annealed draw's).  Weights and energies: the kernel and the helper
add the same N = n + n S + S float64 addends -- the n start addends and the n S updates, of absolute sum A, all exact -- in
two different orders, and round S products dbeta_k E^(k); a float64 sum of N addends in any order is off by at most (N - 1)
2^-53 A, so two orders differ by at most 2 N 2^-53 A, and the products add at most 2^-53 |dbeta_k| A each.  Hence
|energy - helper| <= 4 N 2^-53 A and |log_w - helper| <= 4 N 2^-53 (sum_k |dbeta_k|) A per chain (the S - 1 additions
of the weight's terms fit in as well: N + S + 1 <= 2 N): ~1e-11 relative to A, orders below the 2 |f| of one dropped update.

Shapes, dispatch and conventions: those of ``tests/test_gpu_gibbs_annealed.py`` (rebuilt here) -- sweeps 6 .. 12, h_range
(-4, 4), j_range (-1, 1), a nonzero first chain id, chain counts one more than a multiple of the chains per workgroup, and
a guard row (``state``, ``samples_out``) or element (``log_weight_out``, ``energy_out``) behind the last chain."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, dev, graphs, sampler as smp  # noqa: E402
from oracle import cref, gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP0, SWEEPS = 6, 7
GUARD_STATE, GUARD_OUT, GUARD_W, GUARD_E = 55, 7.0, -3.5, 11.25
EXACT_LOG_Z_16 = 24.417731


# ------------------------------------------------------------------------------------------------ graphs
_solver_plan = functools.partial(support.solver_plan, with_nodes=True)


# degrees beyond 20 (two rounds of the neighbour sum), spin 3 isolated, an odd spin count
_random_plan = functools.partial(support.random_plan, isolated=3, max_degree_above=20)


_clique_plan = support.clique_plan


# name: (plan, chains, sweeps, gibbs_generic, h scale, J scale, prefactor, beta, first chain id)
def _shape(name):
    solver = dict(h_scale=0.05, j_scale=5.0, prefactor=0.05, beta=20.0, id0=1000)
    table = {
        "pegasus64": (lambda: _solver_plan("pegasus", 64)[0], 5, SWEEPS, 0, solver),
        "zephyr128": (lambda: _solver_plan("zephyr", 128)[0], 5, SWEEPS, 0, solver),
        "zephyr512": (lambda: _solver_plan("zephyr", 512)[0], 9, SWEEPS, 0, solver),
        "zephyr512-one-row": (lambda: _solver_plan("zephyr", 512)[0], 9, SWEEPS, 2, solver),
        "zephyr512-rolled": (lambda: _solver_plan("zephyr", 512)[0], 9, SWEEPS, 1, solver),
        "zephyr1024x41": (lambda: _solver_plan("zephyr", 1024)[0], 41, SWEEPS, 0, solver),
        "zephyr1024x530": (lambda: _solver_plan("zephyr", 1024)[0], 530, 3, 0, solver),
        "random77": (_random_plan, 19, SWEEPS, 0, dict(h_scale=0.5, j_scale=2.0, prefactor=0.3, beta=1.5, id0=7)),
        "cliques": (_clique_plan, 21, SWEEPS, 0, dict(h_scale=0.5, j_scale=1.0, prefactor=0.4, beta=1.2, id0=3)),
    }
    make, C, sweeps, generic, p = table[name]
    return make(), C, sweeps, generic, p


SHAPES = ["pegasus64", "zephyr128", "zephyr512", "zephyr512-one-row", "zephyr512-rolled", "zephyr1024x41", "zephyr1024x530",
          "random77", "cliques"]
# the kernel form each shape's draw takes (the module docstring), as the draw's plan names it: _setup asserts it
FORMS = {
    "pegasus64": ("lane", dict(LPC=32, WAVES=1, MB=4, NR=1, MAXS=12)),
    "zephyr128": ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12)),
    "zephyr512": ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=12)),
    "zephyr512-one-row": ("lane", dict(LPC=64, WAVES=4, MB=5, NR=1, MAXS=12)),
    "zephyr512-rolled": ("rolled", dict(LPC=64, WAVES=4)),
    "zephyr1024x41": ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20)),
    "zephyr1024x530": ("rolled", dict(LPC=64, WAVES=16)),
    "random77": ("rolled", dict(LPC=16, WAVES=1)),
    "cliques": ("lane", dict(LPC=64, WAVES=4, MB=4, NR=1, MAXS=20)),
}


# ------------------------------------------------------------------------------------------------ the raw ABI
class _Draw:
    """dvg_gibbs_sample_ais / dvg_gibbs_sample on one graph and one (h, J)."""

    def __init__(self, plan, h, J, prefactor):
        self.plan, self.prefactor = plan, float(prefactor)
        self.gh = smp.GraphHandle(plan, "cuda")
        self.lin, self.quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()

    def buffers(self, start):
        """``state``, ``samples_out`` with a guard row and ``log_weight_out``, ``energy_out`` with a guard element behind
        the last chain; ``start``: (C, n) int8."""
        C = start.shape[0]
        state = torch.full((C + 1, self.plan.n), GUARD_STATE, dtype=torch.int8, device="cuda")
        state[:C] = torch.from_numpy(start).cuda()
        out = torch.full((C + 1, self.plan.n), GUARD_OUT, dtype=torch.float32, device="cuda")
        log_w = torch.full((C + 1,), GUARD_W, dtype=torch.float64, device="cuda")
        energy = torch.full((C + 1,), GUARD_E, dtype=torch.float64, device="cuda")
        return state, out, log_w, energy

    def raw(self, betas_ptr, stride, beta_from, state_ptr, C, id0, seed, sweep0, sweeps, init, out_ptr, log_w_ptr, energy_ptr):
        return _lib.lib().dvg_gibbs_sample_ais(self.gh.ptr, self.lin.data_ptr(), self.quad.data_ptr(), self.prefactor, -4.0, 4.0,
                                               -1.0, 1.0, betas_ptr, stride, float(beta_from), state_ptr, C, id0, seed, sweep0,
                                               sweeps, init, out_ptr, log_w_ptr, energy_ptr, None, _lib.stream_ptr())

    def ais(self, bufs, betas, beta_from, id0, seed, sweep0, init, with_energy=True):
        """``betas``: float32 array, (S,) or (C, S); ``bufs``: what :meth:`buffers` returned."""
        state, out, log_w, energy = bufs
        C = int(state.shape[0]) - 1
        t = torch.from_numpy(np.ascontiguousarray(betas, dtype=np.float32)).cuda()
        S = int(t.shape[-1])
        _lib.check(self.raw(t.data_ptr(), S if t.dim() == 2 else 0, beta_from, state.data_ptr(), C, id0, seed, sweep0, S, init,
                            out.data_ptr(), log_w.data_ptr(), energy.data_ptr() if with_energy else None), "dvg_gibbs_sample_ais")
        torch.cuda.synchronize()

    def plain(self, state, out, beta, id0, seed, sweep0, sweeps, init):
        C = int(state.shape[0]) - 1
        _lib.check(_lib.lib().dvg_gibbs_sample(self.gh.ptr, self.lin.data_ptr(), self.quad.data_ptr(), self.prefactor, -4.0,
                                               4.0, -1.0, 1.0, float(beta), state.data_ptr(), C, id0, seed, sweep0, sweeps,
                                               init, out.data_ptr(), None, _lib.stream_ptr()), "dvg_gibbs_sample")
        torch.cuda.synchronize()


def _setup(name):
    plan, C, sweeps, generic, p = _shape(name)
    with _lib.option_scope(gibbs_generic=generic):
        got = dev.gibbs_draw_plan(plan, C, "weigh")
    assert (got["form"], got["params"]) == FORMS[name], got
    rng = np.random.default_rng(plan.n + C)
    h = (p["h_scale"] * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (p["j_scale"] * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, p["prefactor"], (-4, 4), (-1, 1))
    ids = np.arange(C, dtype=np.uint32) + p["id0"]
    prepared = np.where(rng.uniform(size=(C, plan.n)) < 0.5, -1, 1).astype(np.int8)
    return plan, C, sweeps, generic, p, rng, _Draw(plan, h, J, p["prefactor"]), hs, Js, ids, prepared


def _sum_abs_dbeta(betas, beta_from, C):
    table = np.broadcast_to(np.asarray(betas, dtype=np.float32), (C, np.shape(betas)[-1])).astype(np.float64)
    return np.abs(np.diff(np.concatenate([np.full((C, 1), np.float64(np.float32(beta_from))), table], axis=1), axis=1)).sum(axis=1)


def _check(bufs, want, betas, beta_from, where, with_energy=True):
    """Every spin of ``state`` and ``samples_out`` equals the helper's; weights and energies within the float64 bound; the
    guards are untouched."""
    state, out, log_w, energy = bufs
    C = want.spins.shape[0]
    got, got_state = out.cpu().numpy(), state.cpu().numpy()
    got_w, got_e = log_w.cpu().numpy(), energy.cpu().numpy()
    assert (got_state[C] == GUARD_STATE).all() and (got[C] == GUARD_OUT).all(), f"written past the last chain ({where})"
    assert got_w[C] == GUARD_W and got_e[C] == GUARD_E, f"weights or energies written past the last chain ({where})"
    assert set(np.unique(got[:C]).tolist()) <= {-1.0, 1.0}
    mism = int((got[:C] != want.spins.astype(np.float32)).sum())
    assert mism == 0, f"{mism} spin mismatches in samples_out ({where})"
    assert int((got_state[:C] != want.spins).sum()) == 0, f"state differs from the helper ({where})"
    unit = 4.0 * want.N * 2.0 ** -53 * want.A
    bound_w = unit * _sum_abs_dbeta(betas, beta_from, C)
    err_w = np.abs(got_w[:C] - want.log_w)
    print(f"{where}: |log_w| up to {np.abs(want.log_w).max():.4g}, worst error {err_w.max():.3e} (its bound {bound_w[err_w.argmax()]:.3e})")
    assert np.isfinite(got_w[:C]).all() and (err_w <= bound_w).all(), (where, err_w.max(), bound_w.min())
    if with_energy:
        err_e = np.abs(got_e[:C] - want.energy)
        print(f"{where}: |energy| up to {np.abs(want.energy).max():.4g}, worst error {err_e.max():.3e} (its bound {unit[err_e.argmax()]:.3e})")
        assert np.isfinite(got_e[:C]).all() and (err_e <= unit).all(), (where, err_e.max(), unit.min())
    else:
        assert (got_e == GUARD_E).all(), f"energy_out = NULL, yet the buffer beside it changed ({where})"


def _ladder(C, sweeps, beta, rng):
    """Per-chain rows: chain 0 constant ``beta``, chain 1 all zeros (every spin a fair coin), chain 2 at 200 (the +-87 clamp
    of z is reached), the others random."""
    table = rng.uniform(0.0, 2.0 * beta, size=(C, sweeps)).astype(np.float32)
    table[0], table[1], table[2] = beta, 0.0, 200.0
    return table


@pytest.mark.parametrize("name", SHAPES)
def test_shared_table_fresh_chains(name):
    """One linear schedule from 0 to the shape's beta for all chains, init = 1, beta_from = 0."""
    plan, C, sweeps, generic, p, _rng, d, hs, Js, ids, prepared = _setup(name)
    betas = np.linspace(0.0, p["beta"], sweeps + 1)[1:].astype(np.float32)
    bufs = d.buffers(prepared)  # (init = 1: what `state` holds is not read)
    with _lib.option_scope(gibbs_generic=generic):
        d.ais(bufs, betas, 0.0, p["id0"], SEED, SWEEP0, 1)
    want = ais_oracle.ais(plan, hs, Js, betas, ids, SEED, SWEEP0)
    _check(bufs, want, betas, 0.0, "shared table, init = 1")
    assert np.abs(want.log_w).min() > 0


@pytest.mark.parametrize("name", SHAPES)
def test_shared_table_from_a_prepared_state(name):
    """init = 0 from a prepared state with beta_from = 0.3: the first beta difference is taken from there."""
    plan, C, sweeps, generic, p, _rng, d, hs, Js, ids, prepared = _setup(name)
    betas = smp.beta_schedule(0.05, p["beta"], sweeps)
    bufs = d.buffers(prepared)
    with _lib.option_scope(gibbs_generic=generic):
        d.ais(bufs, betas, 0.3, p["id0"], SEED, SWEEP0, 0)
    want = ais_oracle.ais(plan, hs, Js, betas, ids, SEED, SWEEP0, start=prepared, beta_from=0.3)
    _check(bufs, want, betas, 0.3, "shared table, init = 0, beta_from = 0.3")
    assert not np.array_equal(want.spins, prepared)


@pytest.mark.parametrize("name", SHAPES)
def test_per_chain_ladder(name):
    plan, C, sweeps, generic, p, rng, d, hs, Js, ids, prepared = _setup(name)
    table = _ladder(C, sweeps, p["beta"], rng)
    bufs = d.buffers(prepared)
    with _lib.option_scope(gibbs_generic=generic):
        d.ais(bufs, table, 0.0, p["id0"], SEED, SWEEP0, 1)
    want = ais_oracle.ais(plan, hs, Js, table, ids, SEED, SWEEP0)
    _check(bufs, want, table, 0.0, "per-chain ladder, init = 1")
    assert want.log_w[1] == 0.0 and bufs[2][1].item() == 0.0  # the all-zero row: no beta difference, no weight


@pytest.mark.parametrize("name", SHAPES)
def test_constant_table_weighs_nothing_and_is_the_plain_draw(name):
    """A constant table with beta_from equal to it: every beta difference is 0, so log_w == 0.0 exactly, and the spins are
    those of dvg_gibbs_sample with the same arguments (GPU against GPU)."""
    plan, C, sweeps, generic, p, _rng, d, _hs, _Js, _ids, prepared = _setup(name)
    with _lib.option_scope(gibbs_generic=generic):
        s_plain, o_plain, _w, _e = d.buffers(prepared)
        d.plain(s_plain, o_plain, p["beta"], p["id0"], SEED, SWEEP0, sweeps, 0)
        for table in (np.full(sweeps, p["beta"], np.float32), np.full((C, sweeps), p["beta"], np.float32)):
            bufs = d.buffers(prepared)
            d.ais(bufs, table, p["beta"], p["id0"], SEED, SWEEP0, 0)
            assert torch.equal(bufs[1], o_plain) and torch.equal(bufs[0], s_plain), f"table {table.shape}"
            assert (bufs[2][:C] == 0.0).all() and bufs[2][C].item() == GUARD_W
            assert torch.isfinite(bufs[3][:C]).all() and bufs[3][C].item() == GUARD_E
    assert not torch.equal(s_plain[:C], torch.from_numpy(prepared).cuda())


@pytest.mark.parametrize("name", ["zephyr128", "zephyr512", "zephyr1024x530", "random77"])
def test_energy_out_may_be_null(name):
    plan, C, sweeps, generic, p, _rng, d, hs, Js, ids, prepared = _setup(name)
    betas = np.linspace(0.0, p["beta"], sweeps + 1)[1:].astype(np.float32)
    bufs = d.buffers(prepared)
    with _lib.option_scope(gibbs_generic=generic):
        d.ais(bufs, betas, 0.0, p["id0"], SEED, SWEEP0, 1, with_energy=False)
    _check(bufs, ais_oracle.ais(plan, hs, Js, betas, ids, SEED, SWEEP0), betas, 0.0, "energy_out = NULL", with_energy=False)


def test_invalid_arguments_launch_nothing():
    """A NULL table, a NULL log_weight_out, a bad stride, n_sweeps = 0, fresh chains with beta_from != 0 and a negative or
    non-finite beta_from are DVG_E_INVALID; all four outputs keep their fill."""
    plan, C, _sweeps, _generic, p, _rng, d, _hs, _Js, _ids, prepared = _setup("zephyr128")
    state, out, log_w, energy = d.buffers(prepared)
    before = state.clone()
    t = torch.full((C, SWEEPS), 1.0, dtype=torch.float32, device="cuda")
    tp, wp = t.data_ptr(), log_w.data_ptr()
    #        betas stride  beta_from sweeps init log_w
    cases = [(None, 0, 0.0, SWEEPS, 1, wp), (tp, 0, 0.0, SWEEPS, 1, None), (tp, 3, 0.0, SWEEPS, 1, wp), (tp, 0, 0.0, 0, 1, wp),
             (tp, SWEEPS + 1, 0.0, SWEEPS, 1, wp), (tp, plan.n, 0.0, SWEEPS, 1, wp), (tp, 0, 0.3, SWEEPS, 1, wp),
             (tp, SWEEPS, 1.0, SWEEPS, 1, wp), (tp, 0, -0.5, SWEEPS, 0, wp), (tp, 0, float("nan"), SWEEPS, 0, wp),
             (tp, 0, float("inf"), SWEEPS, 0, wp), (tp, 0, float("nan"), SWEEPS, 1, wp)]
    for betas_ptr, stride, beta_from, sweeps, init, w_ptr in cases:
        rc = d.raw(betas_ptr, stride, beta_from, state.data_ptr(), C, p["id0"], SEED, SWEEP0, sweeps, init, out.data_ptr(), w_ptr,
                   energy.data_ptr())
        assert rc == -1, (stride, beta_from, sweeps, init, rc, _lib.lib().dvg_last_error())
    torch.cuda.synchronize()
    assert torch.equal(state, before) and (out == GUARD_OUT).all() and (log_w == GUARD_W).all() and (energy == GUARD_E).all()


# ------------------------------------------------------------------------------------------------ the estimate
def _zephyr16(beta=1.0):
    """The 16-spin case of tests/test_gibbs_ais_host.py (b)."""
    plan, nodes = _solver_plan("zephyr", 16)
    assert plan.n_edges == 72
    rng = np.random.default_rng(16)
    h = (0.5 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = rng.uniform(-1, 1, plan.n_edges).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 1.0, (-4, 4), (-1, 1))
    betas = np.linspace(0.0, beta, 65)[1:].astype(np.float32)
    ids = np.arange(1024, dtype=np.uint32) + 11
    return plan, nodes, h, J, hs, Js, betas, ids, SEED ^ 0x616E6E6C, 5


def test_enumeration_case_through_the_entry_point():
    """Zephyr 16, 1024 fresh chains, 64 sweeps to beta = 1: the kernel's weights are the helper's within the bound, and the
    log Z they give lies within 3 standard errors of the sum over all 2^16 states."""
    plan, _nodes, h, J, hs, Js, betas, ids, key, sweep0 = _zephyr16()
    exact = ais_oracle.exact_log_z(plan.n, hs, Js, np.asarray(plan.edge_i), np.asarray(plan.edge_j), 1.0)
    assert abs(exact - EXACT_LOG_Z_16) < 1e-6
    d = _Draw(plan, h, J, 1.0)
    bufs = d.buffers(np.ones((ids.size, plan.n), dtype=np.int8))
    d.ais(bufs, betas, 0.0, int(ids[0]), key, sweep0, 1)
    _check(bufs, ais_oracle.ais(plan, hs, Js, betas, ids, key, sweep0), betas, 0.0, "zephyr16 x 1024 x 64")
    est, ess, std_err = ais_oracle.log_z_estimate(plan.n, bufs[2][:ids.size].cpu().numpy())
    print(f"log Z: exact {exact:.6f}, from the kernel's weights {est:.6f}, ESS {ess:.0f}, 3 std_err {3 * std_err:.3f}")
    assert abs(est - EXACT_LOG_Z_16) <= 3.0 * std_err


def _sampler16(beta=1.0):
    plan, nodes, h, J, hs, Js, _betas, _ids, _key, _sweep0 = _zephyr16()
    s = smp.GibbsSampler(plan, nodes, beta=beta, sweeps=4, seed=SEED, persistent=True, chain_offset=11, h_range=(-4, 4),
                         j_range=(-1, 1))
    return plan, nodes, h, J, hs, Js, s


@pytest.mark.parametrize("schedule", ["linear", "geometric"])
def test_log_partition_of_the_sampler(schedule):
    plan, _nodes, h, J, _hs, _Js, s = _sampler16()
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    res = s.log_partition(lin, quad, 1.0, (-4, 4), (-1, 1), num_sweeps=64, num_reads=1024, schedule=schedule)
    assert res.log_z.is_cuda and res.log_z.dtype == torch.float64 and res.log_z.dim() == 0
    assert res.log_weights.shape == (1024,) and res.log_weights.dtype == torch.float64 and res.samples.shape == (1024, plan.n)
    assert s.ais_sweep_count == 64
    est, ess, std_err = ais_oracle.log_z_estimate(plan.n, res.log_weights.cpu().numpy())
    assert abs(float(res.log_z) - est) < 1e-9 and abs(float(res.ess) - ess) < 1e-6 * ess and abs(float(res.std_err) - std_err) < 1e-9
    print(f"{schedule}: {res!r}, exact {EXACT_LOG_Z_16}")
    assert 1.0 < float(res.ess) <= 1024.0 and abs(float(res.log_z) - EXACT_LOG_Z_16) <= 3.0 * float(res.std_err)


def test_sample_ais_leaves_the_other_streams_alone():
    plan, nodes = _solver_plan("zephyr", 128)
    rng = np.random.default_rng(2)
    h = (0.05 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    mk = lambda: smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5,  # noqa: E731
                                  h_range=(-4, 4), j_range=(-1, 1))
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    hs, Js = gibbs.scaled_fields(h, J, 0.05, (-4, 4), (-1, 1))
    C, n, R = 24, plan.n, 9
    ids = np.arange(R, dtype=np.uint32) + 5

    ref = mk()
    ref_draws = [ref.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone() for _ in range(2)]

    s = mk()
    assert s.ais_seed == SEED ^ 0x61697331 and s.ais_sweep_count == 0
    first = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone()
    before = (s._state.clone(), s._state.data_ptr(), s.sweep_count, s.calls, s.cond_sweep_count, s.anneal_sweep_count)

    def check(got, want, betas, beta_from, where):
        samples, log_w, energy = got
        assert samples.shape == (R, n) and samples.dtype == torch.float32 and samples.is_cuda
        assert log_w.shape == (R,) and log_w.dtype == torch.float64 and log_w.is_cuda and energy.shape == (R,) and energy.dtype == torch.float64
        assert np.array_equal(samples.cpu().numpy(), want.spins.astype(np.float32)), where
        unit = 4.0 * want.N * 2.0 ** -53 * want.A
        assert (np.abs(energy.cpu().numpy() - want.energy) <= unit).all(), where
        assert (np.abs(log_w.cpu().numpy() - want.log_w) <= unit * _sum_abs_dbeta(betas, beta_from, R)).all(), where

    # (S,) host schedule, fresh chains: sweeps 0 .. 5 under the AIS key
    shared = smp.beta_schedule(0.0, 20.0, 6, "linear")
    got = s.sample_ais(lin, quad, 0.05, (-4, 4), (-1, 1), shared, num_reads=R)
    assert s.ais_sweep_count == 6
    check(got, ais_oracle.ais(plan, hs, Js, shared, ids, s.ais_seed, 0), shared, 0.0, "fresh chains")

    # (C, S) device table from a float32 start state, beta_from = 0.3: sweeps 6 .. 10
    ladder = _ladder(R, 5, 20.0, rng)
    start = np.where(rng.uniform(size=(R, n)) < 0.5, -1, 1).astype(np.int8)
    start_t = torch.from_numpy(start.astype(np.float32)).cuda()
    got = s.sample_ais(lin, quad, 0.05, (-4, 4), (-1, 1), torch.from_numpy(ladder).cuda(), start=start_t, beta_from=0.3)
    assert s.ais_sweep_count == 11 and torch.equal(start_t, torch.from_numpy(start.astype(np.float32)).cuda())
    check(got, ais_oracle.ais(plan, hs, Js, ladder, ids, s.ais_seed, 6, start=start, beta_from=0.3), ladder, 0.3, "from a state")

    # the training, conditional and annealed streams never noticed
    assert s._state.data_ptr() == before[1] and torch.equal(s._state, before[0])
    assert (s.sweep_count, s.calls, s.cond_sweep_count, s.anneal_sweep_count) == before[2:]
    second = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)
    assert torch.equal(first, ref_draws[0]) and torch.equal(second, ref_draws[1])
    s.reset()
    assert s.ais_sweep_count == 0

    with pytest.raises(ValueError):
        s.sample_ais(lin, quad, 0.05, (-4, 4), (-1, 1), shared, num_reads=R, beta_from=0.3)
    assert s.ais_sweep_count == 0


def test_grbm_log_likelihood_against_enumeration():
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    plan, nodes, h, J, hs, Js, s = _sampler16()
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                           np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    with torch.no_grad():
        grbm._linear.copy_(torch.from_numpy(h).cuda())
        grbm._quadratic.copy_(torch.from_numpy(J).cuda())
    kw = dict(prefactor=1.0, linear_range=(-4, 4), quadratic_range=(-1, 1))
    res = grbm.log_partition(s, num_sweeps=64, num_reads=1024, **kw)
    x = np.where(np.random.default_rng(5).uniform(size=(7, plan.n)) < 0.5, -1, 1).astype(np.int8)
    xt = torch.from_numpy(x.astype(np.float32)).cuda()
    want = -1.0 * gibbs.energy(x, hs, Js, np.asarray(plan.edge_i), np.asarray(plan.edge_j)) - EXACT_LOG_Z_16
    tol = 3.0 * float(res.std_err)
    ll = grbm.log_likelihood(xt, s, log_z=res.log_z, **kw)
    assert ll.shape == (7,) and ll.dtype == torch.float64 and ll.is_cuda
    assert (np.abs(ll.cpu().numpy() - want) <= tol).all(), (ll, want, tol)
    # log_z = None: estimated on the way (the next sweeps of the AIS stream: another estimate, the same condition)
    ll2 = grbm.log_likelihood(xt, s, num_sweeps=64, num_reads=1024, **kw)
    assert s.ais_sweep_count == 128 and (np.abs(ll2.cpu().numpy() - want) <= tol + 3.0 * float(res.std_err)).all()
    with pytest.raises(TypeError):
        grbm.log_likelihood(xt, object(), **kw)


def test_model_wrapper_prior_log_likelihood():
    import gen
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    m.overlap_sampler = False  # (as in the annealed file: this test takes no stream from the process's pool)
    B = 6
    images = torch.from_numpy(gen.make_images(B, seed=4)).reshape(B, 1, 32, 32).cuda()
    ll, res = m.prior_log_likelihood(images, num_sweeps=40, num_reads=128)
    assert ll.shape == (B,) and ll.dtype == torch.float64 and ll.is_cuda and torch.isfinite(ll).all()
    assert torch.isfinite(res.log_z) and res.log_weights.shape == (128,) and float(res.ess) >= 1.0
    s = m.sampler
    assert (s.ais_sweep_count, s.sweep_count, s.calls, s.anneal_sweep_count) == (40, 0, 0, 0) and s._state is None
