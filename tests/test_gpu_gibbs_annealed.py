"""GPU parity of the annealed block-Gibbs draw (``dvg_gibbs_sample_annealed``: beta looked up per sweep, shared by all
chains or a row per chain) against the oracle, bit for bit, and of the Python surface built on it.

The oracle is the existing one, unchanged: per distinct row of the table, ``cref.gibbs_sweeps`` called once per sweep --
that sweep's beta, ``sweep0 + k``, one sweep -- on the chains that share the row IS the annealed draw.

Dispatch each shape takes (gibbs_generic = 0; FORMS below, asserted against the draw's plan beside the bits): Pegasus 64
-- the lane-major form, one-wave workgroups, one row per step; Zephyr 128 -- the same in four-wave workgroups (its tables
are beyond the one-wave rule's 16 KiB); Zephyr 512 -- lane-major, four waves, two rows side by side (gibbs_generic = 2: one at a time; 1: the rolled
kernel); Zephyr 1024 x 41 -- lane-major, four waves, 20 rows; Zephyr 1024 x 530 -- the rolled kernel in 16-wave workgroups
(the plain draw runs its chains-side-by-side kernel there); the 77-spin random graph -- no lane image: rolled, one wave;
the clique graph -- lane-major, one row per step, 14 rows.

Unless a case says otherwise: sweeps 6 .. 12 (an unaligned start that crosses a Philox word boundary twice), h_range
(-4, 4), j_range (-1, 1), a nonzero first chain id, and a guard row behind the last chain in ``state`` and ``samples_out``
that must come back untouched (the chain counts are one more than a multiple of the chains per workgroup)."""
import functools
import os

import numpy as np
import pytest
import torch

import support
from image_generation_amd import _lib, dev, graphs, sampler as smp
from oracle import cref, gibbs

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP0, SWEEPS = 6, 7
GUARD_STATE, GUARD_OUT = 55, 7.0


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


# ------------------------------------------------------------------------------------------------ the oracle
def _oracle(state, ids, table, hs, Js, plan, seed, sweep0):
    """The annealed draw.  ``table``: (C, S) float32, a row per chain (a shared schedule broadcast)."""
    out = np.array(state, dtype=np.int8, copy=True)
    table = np.ascontiguousarray(table, dtype=np.float32)
    rows, inv = np.unique(table, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    for r in range(rows.shape[0]):
        sel = np.flatnonzero(inv == r)
        st = out[sel]
        for k in range(rows.shape[1]):
            st = cref.gibbs_sweeps(st, ids[sel], hs, Js, float(rows[r, k]), plan.order, plan.class_ptr, plan.adj_ptr,
                                   plan.adj_idx, plan.adj_eid, seed, sweep0 + k, 1)
        out[sel] = st
    return out


# ------------------------------------------------------------------------------------------------ the raw ABI
class _Draw:
    """dvg_gibbs_sample_annealed / dvg_gibbs_sample on one graph and one (h, J)."""

    def __init__(self, plan, h, J, prefactor):
        self.plan, self.prefactor = plan, float(prefactor)
        self.gh = smp.GraphHandle(plan, "cuda")
        self.lin, self.quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()

    def buffers(self, start):
        """``state`` and ``samples_out`` with a guard row behind the last chain; ``start``: (C, n) int8."""
        C = start.shape[0]
        state = torch.full((C + 1, self.plan.n), GUARD_STATE, dtype=torch.int8, device="cuda")
        state[:C] = torch.from_numpy(start).cuda()
        out = torch.full((C + 1, self.plan.n), GUARD_OUT, dtype=torch.float32, device="cuda")
        return state, out

    def raw(self, betas_ptr, stride, state_ptr, C, id0, seed, sweep0, sweeps, init, out_ptr):
        return _lib.lib().dvg_gibbs_sample_annealed(self.gh.ptr, self.lin.data_ptr(), self.quad.data_ptr(), self.prefactor,
                                                    -4.0, 4.0, -1.0, 1.0, betas_ptr, stride, state_ptr, C, id0, seed, sweep0,
                                                    sweeps, init, out_ptr, None, _lib.stream_ptr())

    def annealed(self, state, out, betas, id0, seed, sweep0, init):
        """``betas``: float32 array, (S,) or (C, S); ``state`` / ``out``: (C + 1, n) with the guard row."""
        C = int(state.shape[0]) - 1
        t = torch.from_numpy(np.ascontiguousarray(betas, dtype=np.float32)).cuda()
        S = int(t.shape[-1])
        _lib.check(self.raw(t.data_ptr(), S if t.dim() == 2 else 0, state.data_ptr(), C, id0, seed, sweep0, S, init,
                            out.data_ptr()), "dvg_gibbs_sample_annealed")
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
        got = dev.gibbs_draw_plan(plan, C, "table")
    assert (got["form"], got["params"]) == FORMS[name], got
    rng = np.random.default_rng(plan.n + C)
    h = (p["h_scale"] * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (p["j_scale"] * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, p["prefactor"], (-4, 4), (-1, 1))
    ids = np.arange(C, dtype=np.uint32) + p["id0"]
    prepared = np.where(rng.uniform(size=(C, plan.n)) < 0.5, -1, 1).astype(np.int8)
    return plan, C, sweeps, generic, p, rng, _Draw(plan, h, J, p["prefactor"]), hs, Js, ids, prepared


def _check(state, out, want, where):
    """Every spin of ``state`` and ``samples_out`` equals the oracle's; the guard rows are untouched."""
    C = want.shape[0]
    got, got_state = out.cpu().numpy(), state.cpu().numpy()
    assert (got_state[C] == GUARD_STATE).all() and (got[C] == GUARD_OUT).all(), f"written past the last chain ({where})"
    assert set(np.unique(got[:C]).tolist()) <= {-1.0, 1.0}
    mism = int((got[:C] != want.astype(np.float32)).sum())
    assert mism == 0, f"{mism} spin mismatches in samples_out ({where})"
    assert int((got_state[:C] != want).sum()) == 0, f"state differs from the oracle ({where})"


@pytest.mark.parametrize("name", SHAPES)
def test_shared_schedule_fresh_chains(name):
    """One geometric schedule from 0.05 to 20 for all chains, init = 1."""
    plan, C, sweeps, generic, p, _rng, d, hs, Js, ids, prepared = _setup(name)
    betas = smp.beta_schedule(0.05, 20.0, sweeps)
    state, out = d.buffers(prepared)  # (init = 1: what `state` holds is not read)
    with _lib.option_scope(gibbs_generic=generic):
        d.annealed(state, out, betas, p["id0"], SEED, SWEEP0, 1)
    want = _oracle(cref.init_state(ids, plan.n, SEED, SWEEP0), ids, np.broadcast_to(betas, (C, sweeps)), hs, Js, plan, SEED, SWEEP0)
    _check(state, out, want, "init = 1")


@pytest.mark.parametrize("name", SHAPES)
def test_shared_schedule_from_a_state_and_continued(name):
    """init = 0 from a prepared state; a second call goes on from the first call's ``state`` at sweep0 + sweeps."""
    plan, C, sweeps, generic, p, _rng, d, hs, Js, ids, prepared = _setup(name)
    betas = smp.beta_schedule(0.05, 20.0, sweeps)
    state, out = d.buffers(prepared)
    want = prepared
    with _lib.option_scope(gibbs_generic=generic):
        for call in range(2):
            sweep0 = SWEEP0 + call * sweeps
            d.annealed(state, out, betas, p["id0"], SEED, sweep0, 0)
            want = _oracle(want, ids, np.broadcast_to(betas, (C, sweeps)), hs, Js, plan, SEED, sweep0)
            _check(state, out, want, f"call {call}")
    assert not np.array_equal(want, prepared)


def _ladder(C, sweeps, beta, rng):
    """Per-chain rows: chain 0 constant ``beta``, chain 1 all zeros (every spin a fair coin), chain 2 at 200 (the +-87 clamp
    of z is reached), the others random."""
    table = rng.uniform(0.0, 2.0 * beta, size=(C, sweeps)).astype(np.float32)
    table[0], table[1], table[2] = beta, 0.0, 200.0
    return table


@pytest.mark.parametrize("init", [0, 1])
@pytest.mark.parametrize("name", SHAPES)
def test_per_chain_tables(name, init):
    plan, C, sweeps, generic, p, rng, d, hs, Js, ids, prepared = _setup(name)
    table = _ladder(C, sweeps, p["beta"], rng)
    state, out = d.buffers(prepared)
    with _lib.option_scope(gibbs_generic=generic):
        d.annealed(state, out, table, p["id0"], SEED, SWEEP0, init)
    start = cref.init_state(ids, plan.n, SEED, SWEEP0) if init else prepared
    want = _oracle(start, ids, table, hs, Js, plan, SEED, SWEEP0)
    _check(state, out, want, f"per-chain table, init = {init}")
    # beta = 0: the field drops out -- the chain's spins are the fair coins of its last sweep's random words, whatever (h, J)
    zero = _oracle(start[1:2], ids[1:2], table[1:2], np.zeros_like(hs), np.zeros_like(Js), plan, SEED, SWEEP0)
    assert np.array_equal(state[1].cpu().numpy(), zero[0])


@pytest.mark.parametrize("init", [0, 1])
@pytest.mark.parametrize("name", SHAPES)
def test_constant_table_is_the_plain_draw(name, init):
    """A table whose entries all equal beta, shared and a row per chain, gives the bits of dvg_gibbs_sample with the same
    arguments (GPU against GPU; 1024 x 530: the plain draw runs the chains-side-by-side kernel, the annealed one the rolled
    kernel)."""
    plan, C, sweeps, generic, p, _rng, d, _hs, _Js, _ids, prepared = _setup(name)
    with _lib.option_scope(gibbs_generic=generic):
        s_plain, o_plain = d.buffers(prepared)
        d.plain(s_plain, o_plain, p["beta"], p["id0"], SEED, SWEEP0, sweeps, init)
        for table in (np.full(sweeps, p["beta"], np.float32), np.full((C, sweeps), p["beta"], np.float32)):
            state, out = d.buffers(prepared)
            d.annealed(state, out, table, p["id0"], SEED, SWEEP0, init)
            assert torch.equal(out, o_plain) and torch.equal(state, s_plain), f"table {table.shape}"
    assert not torch.equal(s_plain[:C], torch.from_numpy(prepared).cuda())
    assert (o_plain[C] == GUARD_OUT).all()


@pytest.mark.parametrize("name,C", [("pegasus64", 5), ("pegasus64", 4), ("zephyr512", 9), ("zephyr512-rolled", 5),
                                     ("zephyr1024x530", 529), ("random77", 2)])
def test_nothing_is_written_past_the_last_chain(name, C):
    """Chain counts one more than a multiple of the chains per workgroup (and, once, an exact multiple): the rows behind
    the last chain of ``state`` and ``samples_out`` keep their sentinel, with a per-chain table (which has no row behind
    the last chain: it is exactly (C, sweeps))."""
    plan, _C, _sweeps, generic, p, rng, d, hs, Js, _ids, _prepared = _setup(name)
    sweeps = 3
    ids = np.arange(C, dtype=np.uint32) + p["id0"]
    table = rng.uniform(0.0, 2.0 * p["beta"], size=(C, sweeps)).astype(np.float32)
    state, out = d.buffers(np.ones((C, plan.n), dtype=np.int8))
    with _lib.option_scope(gibbs_generic=generic):
        d.annealed(state, out, table, p["id0"], SEED, SWEEP0, 1)
    _check(state, out, _oracle(cref.init_state(ids, plan.n, SEED, SWEEP0), ids, table, hs, Js, plan, SEED, SWEEP0), f"{C} chains")


def test_invalid_arguments_launch_nothing():
    """A NULL table, stride 3 (neither 0 nor n_sweeps = 7) and n_sweeps = 0 are DVG_E_INVALID; state and output keep their
    sentinels."""
    plan, C, _sweeps, _generic, p, _rng, d, _hs, _Js, _ids, prepared = _setup("zephyr128")
    state, out = d.buffers(prepared)
    before = state.clone()
    t = torch.full((C, SWEEPS), 1.0, dtype=torch.float32, device="cuda")
    for betas_ptr, stride, sweeps in ((None, 0, SWEEPS), (t.data_ptr(), 3, SWEEPS), (t.data_ptr(), 0, 0), (t.data_ptr(), SWEEPS, 0),
                                      (t.data_ptr(), SWEEPS + 1, SWEEPS), (t.data_ptr(), plan.n, SWEEPS)):
        rc = d.raw(betas_ptr, stride, state.data_ptr(), C, p["id0"], SEED, SWEEP0, sweeps, 1, out.data_ptr())
        assert rc == -1, (stride, sweeps, rc, _lib.lib().dvg_last_error())
    torch.cuda.synchronize()
    assert torch.equal(state, before) and (out == GUARD_OUT).all()


# ------------------------------------------------------------------------------------------------ the Python surface
def _sampler_fixture():
    plan, nodes = _solver_plan("zephyr", 128)
    rng = np.random.default_rng(2)
    h = (0.05 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    mk = lambda: smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5,  # noqa: E731
                                  h_range=(-4, 4), j_range=(-1, 1))
    return plan, nodes, rng, h, J, mk


def test_sample_annealed_leaves_the_training_stream_alone():
    plan, _nodes, rng, h, J, mk = _sampler_fixture()
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    hs, Js = gibbs.scaled_fields(h, J, 0.05, (-4, 4), (-1, 1))
    C, n, R = 24, plan.n, 9
    ids = np.arange(R, dtype=np.uint32) + 5

    ref = mk()
    ref_draws = [ref.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone() for _ in range(2)]

    s = mk()
    assert s.anneal_seed == SEED ^ 0x616E6E6C and s.anneal_sweep_count == 0
    first = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone()
    before = (s._state.clone(), s._state.data_ptr(), s.sweep_count, s.calls, s.cond_sweep_count)

    # (S,) host schedule, fresh chains: sweeps 0 .. 5 under the annealing key
    shared = smp.beta_schedule(0.05, 20.0, 6)
    out = s.sample_annealed(lin, quad, 0.05, (-4, 4), (-1, 1), shared, num_reads=R)
    assert out.shape == (R, n) and out.dtype == torch.float32 and out.is_cuda and s.anneal_sweep_count == 6
    want = _oracle(cref.init_state(ids, n, s.anneal_seed, 0), ids, np.broadcast_to(shared, (R, 6)), hs, Js, plan, s.anneal_seed, 0)
    assert np.array_equal(out.cpu().numpy(), want.astype(np.float32))

    # (C, S) table as a CUDA float32 tensor, from a float32 start state: sweeps 6 .. 10
    ladder = _ladder(R, 5, 20.0, rng)
    start = np.where(rng.uniform(size=(R, n)) < 0.5, -1, 1).astype(np.int8)
    start_t = torch.from_numpy(start.astype(np.float32)).cuda()
    out2 = s.sample_annealed(lin, quad, 0.05, (-4, 4), (-1, 1), torch.from_numpy(ladder).cuda(), start=start_t)
    assert s.anneal_sweep_count == 11 and torch.equal(start_t, torch.from_numpy(start.astype(np.float32)).cuda())
    assert np.array_equal(out2.cpu().numpy(), _oracle(start, ids, ladder, hs, Js, plan, s.anneal_seed, 6).astype(np.float32))

    # (C, S) host table on fresh chains, the chain count read off the table; an int8 start with a list schedule
    out3 = s.sample_annealed(lin, quad, 0.05, (-4, 4), (-1, 1), ladder)
    want3 = _oracle(cref.init_state(ids, n, s.anneal_seed, 11), ids, ladder, hs, Js, plan, s.anneal_seed, 11)
    assert s.anneal_sweep_count == 16 and np.array_equal(out3.cpu().numpy(), want3.astype(np.float32))
    out4 = s.sample_annealed(lin, quad, 0.05, (-4, 4), (-1, 1), [0.5, 1.0, 20.0], start=torch.from_numpy(start).cuda())
    want4 = _oracle(start, ids, np.broadcast_to(np.float32([0.5, 1.0, 20.0]), (R, 3)), hs, Js, plan, s.anneal_seed, 16)
    assert s.anneal_sweep_count == 19 and np.array_equal(out4.cpu().numpy(), want4.astype(np.float32))

    # the training draws never noticed
    assert s._state.data_ptr() == before[1] and torch.equal(s._state, before[0])
    assert (s.sweep_count, s.calls, s.cond_sweep_count) == before[2:]
    second = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)
    assert torch.equal(first, ref_draws[0]) and torch.equal(second, ref_draws[1])
    s.reset()
    assert s.anneal_sweep_count == 0

    with pytest.raises(_lib.DvgError):
        s.sample_annealed(lin, quad, 0.05, (-4, 4), (-1, 1), shared, start=start_t.cpu())
    with pytest.raises(_lib.DvgError):
        s.sample_annealed(lin, quad, 0.05, (-4, 4), (-1, 1), torch.from_numpy(ladder).cuda().double(), num_reads=R)
    with pytest.raises(ValueError):
        s.sample_annealed(lin, quad, 0.05, (-4, 4), (-1, 1), [0.5, -1.0], num_reads=R)


def test_set_beta_schedule_drives_the_training_draw():
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    plan, nodes, _rng, _h, _J, mk = _sampler_fixture()
    n, C = plan.n, 24
    torch.manual_seed(1)
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                            np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    h, J = grbm._linear.detach().cpu().numpy(), grbm._quadratic.detach().cpu().numpy()
    hs, Js = gibbs.scaled_fields(h, J, 0.05, (-4, 4), (-1, 1))
    ids = np.arange(C, dtype=np.uint32) + 5
    draw = lambda s: grbm.sample(s, prefactor=0.05, linear_range=(-4, 4), quadratic_range=(-1, 1),  # noqa: E731
                                 sample_params=dict(num_reads=C)).cpu().numpy()

    s = mk()
    betas = smp.beta_schedule(0.3, 20.0, 7)
    s.set_beta_schedule(betas)
    assert s.sweeps == 7 and s._betas.is_cuda and s._betas.dtype == torch.float32 and np.array_equal(s._betas.cpu().numpy(), betas)
    want = cref.init_state(ids, n, SEED, 0)
    for call in range(2):  # persistent chains under the training key: init on the first draw only, the sweep index running on
        got = draw(s)
        want = _oracle(want, ids, np.broadcast_to(betas, (C, 7)), hs, Js, plan, SEED, 7 * call)
        assert np.array_equal(got, want.astype(np.float32)), f"draw {call}"
        assert (s.sweep_count, s.calls, s.anneal_sweep_count) == (7 * (call + 1), call + 1, 0)
        assert np.array_equal(s._state.cpu().numpy(), want)

    # another schedule: a new table (a captured step would notice), another length
    old_ptr = s._betas.data_ptr()
    dev_betas = torch.from_numpy(smp.beta_schedule(1.0, 20.0, 3, "linear")).cuda()
    s.set_beta_schedule(dev_betas)
    assert s.sweeps == 3 and s._betas.data_ptr() not in (old_ptr, dev_betas.data_ptr())
    got = draw(s)
    want = _oracle(want, ids, np.broadcast_to(dev_betas.cpu().numpy(), (C, 3)), hs, Js, plan, SEED, 14)
    assert np.array_equal(got, want.astype(np.float32)) and s.sweep_count == 17

    # None: the fixed-beta draw again, with the sweeps per draw it had
    s.set_beta_schedule(None)
    assert s._betas is None and s.sweeps == 4
    got = draw(s)
    want = cref.gibbs_sweeps(want, ids, hs, Js, 20.0, plan.order, plan.class_ptr, plan.adj_ptr, plan.adj_idx, plan.adj_eid,
                             SEED, 17, 4)
    assert np.array_equal(got, want.astype(np.float32)) and (s.sweep_count, s.calls) == (21, 4)


def _ising_problem():
    plan, nodes, rng, _h, _J, mk = _sampler_fixture()
    h = (0.4 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (0.8 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    hd = {nodes[i]: float(h[i]) for i in range(plan.n)}
    Jd = {(nodes[int(a)], nodes[int(b)]): float(J[e]) for e, (a, b) in enumerate(zip(plan.edge_i, plan.edge_j))}
    bound = (plan.n + plan.n_edges) * 2.0 ** -24 * (float(np.abs(h.astype(np.float64)).sum()) + float(np.abs(J.astype(np.float64)).sum()))
    return plan, nodes, h, J, hd, Jd, bound, mk


def test_sample_ising_annealed_reads_and_energies():
    plan, nodes, h, J, hd, Jd, bound, mk = _ising_problem()
    s = mk()
    ss = s.sample_ising(hd, Jd, num_reads=8, beta_range=(0.1, 3.0), num_sweeps=9, annealing_time=5.0)
    assert len(ss) == 8 and ss.variables == list(nodes) and ss.vartype == "SPIN"
    assert ss._energy is None and ss.device_energy.is_cuda  # not on the host until .record is read
    rec = ss.record
    assert rec.sample.dtype == np.int8 and rec.sample.shape == (8, plan.n) and rec.energy.shape == (8,)
    # fresh chains under the annealing key, geometric by default, (h, J) as given (prefactor 1, no clamp)
    ids = np.arange(8, dtype=np.uint32) + 5
    hs, Js = gibbs.scaled_fields(h, J, 1.0, None, None)
    betas = smp.beta_schedule(0.1, 3.0, 9, "geometric")
    want = _oracle(cref.init_state(ids, plan.n, s.anneal_seed, 0), ids, np.broadcast_to(betas, (8, 9)), hs, Js, plan, s.anneal_seed, 0)
    assert np.array_equal(rec.sample, want)
    assert (s.anneal_sweep_count, s.sweep_count, s.calls) == (9, 0, 0) and s._state is None
    exact = gibbs.energy(want, h, J, np.asarray(plan.edge_i), np.asarray(plan.edge_j))
    err = float(np.abs(rec.energy.astype(np.float64) - exact).max())
    print(f"annealed sample_ising: max |energy error| {err:.3e}, bound {bound:.3e}")
    assert err <= bound

    # neal's other spellings: a linear range, an explicit schedule ("custom"), a row per read
    lin_ss = s.sample_ising(hd, Jd, num_reads=8, beta_range=(0.1, 3.0), num_sweeps=9, beta_schedule_type="linear")
    via = mk(); via.anneal_sweep_count = 9
    direct = via.sample_annealed(torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda(), 1.0, None, None,
                                 smp.beta_schedule(0.1, 3.0, 9, "linear"), num_reads=8)
    assert torch.equal(lin_ss.device_tensor, direct)
    ladder = _ladder(8, 4, 2.0, np.random.default_rng(0))
    lad_ss = s.sample_ising(hd, Jd, num_reads=8, beta_schedule=ladder, beta_schedule_type="custom")
    want = _oracle(cref.init_state(ids, plan.n, s.anneal_seed, 18), ids, ladder, hs, Js, plan, s.anneal_seed, 18)
    assert np.array_equal(lad_ss.record.sample, want) and s.anneal_sweep_count == 22


def test_plain_sample_ising_now_has_energies():
    plan, _nodes, h, J, hd, Jd, bound, mk = _ising_problem()
    s = mk()
    ss = s.sample_ising(hd, Jd, num_reads=8)
    rec = ss.record
    ids = np.arange(8, dtype=np.uint32) + 5
    hs, Js = gibbs.scaled_fields(h, J, 1.0, None, None)
    want = cref.gibbs_sweeps(cref.init_state(ids, plan.n, SEED, 0), ids, hs, Js, 20.0, plan.order, plan.class_ptr, plan.adj_ptr,
                             plan.adj_idx, plan.adj_eid, SEED, 0, 4)
    assert np.array_equal(rec.sample, want) and (s.sweep_count, s.calls, s.anneal_sweep_count) == (4, 1, 0)
    exact = gibbs.energy(want, h, J, np.asarray(plan.edge_i), np.asarray(plan.edge_j))
    err = float(np.abs(rec.energy.astype(np.float64) - exact).max())
    print(f"plain sample_ising: max |energy error| {err:.3e}, bound {bound:.3e}")
    assert rec.energy.shape == (8,) and err <= bound


# ------------------------------------------------------------------------------------------------ ModelWrapper
def _annealed_yaml(tmp_path, extra="GIBBS_BETA_START: 0.5\n"):
    text = open(os.path.join(ROOT, "tests", "golden", "step_params.yaml")).read()
    path = tmp_path / "step_params_annealed.yaml"
    path.write_text(text + "\n" + extra)
    return str(path)


def test_model_wrapper_annealed_graph_replay_is_bit_identical_to_eager(tmp_path):
    """GIBBS_BETA_START in the YAML: every training draw anneals 0.5 -> 1 / PREFACTOR over its GIBBS_SWEEPS sweeps.  12 steps
    eagerly and 12 replayed from the captured step: the same losses per step, the same weights.  Then the schedule is
    changed: the captured step holds the old table's address, so the step is captured again -- six more steps, still equal.
    (``overlap_sampler`` off: the annealed draw is captured on the main stream, with its sweep index read from the device.)"""
    import gen
    from image_generation_amd.model_wrapper import ModelWrapper

    params = _annealed_yaml(tmp_path)
    steps, more = 12, 6

    def run(use_graph):
        torch.manual_seed(0)
        m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=params)
        B = m.BATCH_SIZE
        imgs = torch.from_numpy(gen.make_images(B * (steps + more), seed=4)).reshape(steps + more, B, 1, 32, 32).cuda()
        m.set_dataloader([(imgs[k], None) for k in range(steps + more)])
        m.train_init(1)
        m.sync_losses = False
        m.use_graph = use_graph
        # the draw in line on the main stream: a wrapper's side stream is taken from the process's stream pool for good, and
        # which hardware queue a LATER test's side stream lands on depends on how many were taken before it
        # (test_gpu_step.py::test_mmd_join_position_is_measured_per_shape needs its two streams on different queues)
        m.overlap_sampler = False
        want = smp.beta_schedule(0.5, 1.0 / m.PREFACTOR, 3, "geometric")
        assert m.sampler.sweeps == 3 and np.array_equal(m.sampler._betas.cpu().numpy(), want)
        out = []
        for k in range(steps):
            m.step((imgs[k], None), epoch=0)
            out.append((float(m.last["mse"]), float(m.last["mmd"])))
        torch.cuda.synchronize()
        sd = {k: v.clone() for k, v in m._dvae.state_dict().items()}
        sd.update({"grbm." + k: v.clone() for k, v in m._grbm.state_dict().items()})
        captured = m._graph is not None and not m._graph_failed
        replays = m._replays
        m.sampler.set_beta_schedule(smp.beta_schedule(2.0, 1.0 / m.PREFACTOR, 3, "linear"))
        for k in range(steps, steps + more):
            m.step((imgs[k], None), epoch=0)
            out.append((float(m.last["mse"]), float(m.last["mmd"])))
        torch.cuda.synchronize()
        sd2 = {k: v.clone() for k, v in m._dvae.state_dict().items()}
        return out, sd, sd2, m, captured, replays

    eager, sd_e, sd2_e, me, _cap, _rep = run(False)
    graphed, sd_g, sd2_g, mg, captured, replays = run(True)
    assert captured and replays > 0, "the step was not captured"
    assert mg._graph is not None and not mg._graph_failed and 0 < mg._replays < more, "the step was not captured again"
    assert eager == graphed and len(set(e[0] for e in eager)) > 8
    assert me.sampler.sweep_count == mg.sampler.sweep_count and me.sampler.calls == mg.sampler.calls
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    for k in sd2_e:
        assert torch.equal(sd2_e[k], sd2_g[k]), k


def test_model_wrapper_yaml_keys(tmp_path):
    from image_generation_amd.model_wrapper import ModelWrapper

    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=_annealed_yaml(
        tmp_path, "GIBBS_BETA_START: 2.0\nGIBBS_BETA_SCHEDULE: linear\n"))
    m.setup()
    assert np.array_equal(m.sampler._betas.cpu().numpy(), smp.beta_schedule(2.0, 20.0, 3, "linear"))
    assert m._graph_addresses()[-1] == m.sampler._betas.data_ptr()
    plain = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    plain.setup()
    assert plain.sampler._betas is None and plain.sampler.sweeps == 3 and plain._graph_addresses()[-1] == 0
    with pytest.raises(ValueError):
        bad = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=_annealed_yaml(
            tmp_path, "GIBBS_BETA_START: 2.0\nGIBBS_BETA_SCHEDULE: cosine\n"))
        bad.setup()


def test_generate_images_from_annealed_chains():
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    s, plan, n, R = m.sampler, m.sampler.plan, 64, 16
    h, J = m._grbm._linear.detach().cpu().numpy(), m._grbm._quadratic.detach().cpu().numpy()
    hs, Js = gibbs.scaled_fields(h, J, m.PREFACTOR, m.linear_range, m.quadratic_range)
    ids = np.arange(R, dtype=np.uint32) + s.chain_offset
    at = 0
    for betas in (smp.beta_schedule(0.5, 20.0, 6), _ladder(R, 5, 20.0, np.random.default_rng(3))):
        imgs = m.generate_images(betas=betas)
        S = betas.shape[-1]
        table = np.broadcast_to(betas, (R, S))
        want = _oracle(cref.init_state(ids, n, s.anneal_seed, at), ids, table, hs, Js, plan, s.anneal_seed, at)
        at += S
        with torch.no_grad():
            decoded = m._dvae.decoder(torch.from_numpy(want.astype(np.float32)).cuda().unsqueeze(1)).squeeze(1).clip(0.0, 1.0)
        assert imgs.shape == (R, 1, 32, 32) and torch.equal(imgs, decoded)
        assert (s.anneal_sweep_count, s.sweep_count, s.calls) == (at, 0, 0) and s._state is None
    # betas=None is today's draw: the sampler's own chains
    m.generate_images()
    assert (s.sweep_count, s.calls, s.anneal_sweep_count) == (3, 1, at)
