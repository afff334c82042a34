"""GPU parity of the exchange draw (``dvg_gibbs_sample_tempered``, "DVG PT v1": ladders of chains that sweep at the beta of the
rung they hold and exchange rungs inside the kernel) against the definition in ``tests/tempered_oracle.py``, against the
existing draws where the definition makes them equal, and of the Python surface built on it.

Spins, rungs and accept counts: equal to the helper's, bit for bit.  Energies: the kernel and the helper add the same at most
N = n (S + 2) float64 addends of absolute sum A in two orders, so |energy - helper| <= 4 N 2^-53 A (the argument of
``tests/test_gpu_gibbs_ais.py``).  An exchange decided on a coin (d < 0) compares u with exp(d): d carries the two energies'
errors times |dbeta|, so the two sides can decide differently only if |u - exp(d)| <= 4 N 2^-53 |dbeta| (A_a + A_b) exp(d) -- plus
an ulp of exp.  No decision is left out of the comparison: the test asserts that the helper's every |u - exp(d)| is at least 10^6
times that bound.

Conventions of ``tests/test_gpu_gibbs_ais.py``: sweeps 6 .. 17, a nonzero first chain id, a guard row or element behind every
output, and the plan's form asserted per shape.  12 sweeps from sweep 6 are the exchanges 7 .. 18 at swap_every = 1: both
parities.  (h, J) are normal-distributed; per shape the seed of the generator was picked, with the helper alone, so that on the
first five shapes every pair of rungs sees both an accepted and a rejected exchange."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_oracle  # noqa: E402
import tempered_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, dev, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP0 = 6
GUARD_STATE, GUARD_RUNG, GUARD_OUT, GUARD_E, GUARD_ACC = 55, -77, 7.0, 11.25, 123456


# ------------------------------------------------------------------------------------------------ graphs
_solver_plan = functools.partial(support.solver_plan, with_nodes=True)


# degrees beyond 20 (two rounds of the neighbour sum), spin 3 isolated, an odd spin count
_random_plan = functools.partial(support.random_plan, isolated=3, max_degree_above=20)


_clique_plan = support.clique_plan


SOLVER = dict(h_scale=0.05, j_scale=5.0, prefactor=0.05, beta=20.0, id0=1000)
# name: (plan, replicas, ladders, swap_every, sweeps, gibbs_generic, lo of the ladder, seed of (h, J), parameters)
TABLE = {
    "pegasus64": (lambda: _solver_plan("pegasus", 64)[0], 4, 3, 1, 12, 0, 0.8, 0, SOLVER),
    "zephyr128": (lambda: _solver_plan("zephyr", 128)[0], 8, 2, 2, 12, 0, 0.5, 2, SOLVER),
    "zephyr512": (lambda: _solver_plan("zephyr", 512)[0], 4, 3, 1, 12, 0, 0.8, 0, SOLVER),
    "zephyr512x8": (lambda: _solver_plan("zephyr", 512)[0], 8, 3, 3, 12, 0, 0.8, 0, SOLVER),
    "zephyr512-rolled": (lambda: _solver_plan("zephyr", 512)[0], 4, 3, 1, 12, 1, 0.8, 0, SOLVER),
    "random77": (_random_plan, 3, 5, 1, 12, 0, 0.5, 0, dict(h_scale=0.5, j_scale=2.0, prefactor=0.3, beta=1.5, id0=7)),
    "cliques": (_clique_plan, 4, 2, 2, 12, 0, 0.8, 0, dict(h_scale=0.5, j_scale=1.0, prefactor=0.4, beta=1.2, id0=3)),
    "zephyr1024": (lambda: _solver_plan("zephyr", 1024)[0], 16, 2, 1, 4, 0, 0.8, 0, SOLVER),
    "pegasus64x5": (lambda: _solver_plan("pegasus", 64)[0], 5, 3, 1, 12, 0, 0.5, 0, SOLVER),
}
SHAPES = list(TABLE)
BOTH_OUTCOMES = SHAPES[:5]  # every pair of rungs sees an accepted and a rejected exchange
# the kernel form, the chain slots and whole ladders of a workgroup, and the workgroups of each shape's draw
FORMS = {
    "pegasus64": ("lane", dict(LPC=32, WAVES=4, MB=4, NR=1, MAXS=12), 8, 2, 2),   # second workgroup: one ladder, four idle slots
    "zephyr128": ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 8, 1, 2),
    "zephyr512": ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=12), 4, 1, 3),
    "zephyr512x8": ("rolled", dict(LPC=64, WAVES=16), 16, 2, 2),                 # second workgroup half empty: idle waves
    "zephyr512-rolled": ("rolled", dict(LPC=64, WAVES=4), 4, 1, 3),
    "random77": ("rolled", dict(LPC=16, WAVES=1), 4, 1, 5),                       # an idle slot in every workgroup
    "cliques": ("lane", dict(LPC=64, WAVES=4, MB=4, NR=1, MAXS=20), 4, 1, 2),
    "zephyr1024": ("rolled", dict(LPC=64, WAVES=16), 16, 1, 2),
    # lane-major with three idle slots per workgroup: an idle wave, and a wave whose second chain slot idles
    "pegasus64x5": ("lane", dict(LPC=32, WAVES=4, MB=4, NR=1, MAXS=12), 8, 1, 3),
}


def parameters(name, seed=None, lo=None):
    """The shape's graph, normal-distributed (h, J) and their scaled, clamped fields, the ladder and the chain ids -- no GPU
    (the seeds of TABLE were picked with this function and the helper)."""
    make, R, Q, every, sweeps, generic, lo, hj_seed, p = TABLE[name][:6] + (TABLE[name][6] if lo is None else lo,) + TABLE[name][7:]
    plan = make()
    rng = np.random.default_rng([plan.n, R * Q, hj_seed if seed is None else seed])
    h = (p["h_scale"] * rng.normal(size=plan.n)).astype(np.float32)
    J = (p["j_scale"] * rng.normal(size=plan.n_edges)).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, p["prefactor"], (-4, 4), (-1, 1))
    ladder = np.geomspace(lo * p["beta"], p["beta"], R).astype(np.float32)
    ids = np.arange(Q * R, dtype=np.uint32) + p["id0"]
    return plan, R, Q, every, sweeps, generic, p, h, J, hs, Js, ladder, ids


@functools.lru_cache(maxsize=None)
def definition(name):
    """The helper's draw of the shape (fresh chains), computed once and shared; nothing changes it."""
    plan, R, Q, every, sweeps, _generic, _p, _h, _J, hs, Js, ladder, ids = parameters(name)
    return tempered_oracle.tempered(plan, hs, Js, ladder, ids, SEED, SWEEP0, sweeps, every)


# ------------------------------------------------------------------------------------------------ the raw ABI
class _Draw:
    def __init__(self, plan, h, J, prefactor):
        self.plan, self.prefactor = plan, float(prefactor)
        self.gh = smp.GraphHandle(plan, "cuda")
        self.lin, self.quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()

    def buffers(self, C, start=None, rungs=None):
        """state, rung, samples_out, energy_out, accept_out, each with a guard row or element behind the last chain"""
        n = self.plan.n
        state = torch.full((C + 1, n), GUARD_STATE, dtype=torch.int8, device="cuda")
        rung = torch.full((C + 1,), GUARD_RUNG, dtype=torch.int32, device="cuda")
        if start is not None:
            state[:C] = torch.from_numpy(np.ascontiguousarray(start, dtype=np.int8)).cuda()
            rung[:C] = torch.from_numpy(np.ascontiguousarray(rungs, dtype=np.int32)).cuda()
        out = torch.full((C + 1, n), GUARD_OUT, dtype=torch.float32, device="cuda")
        energy = torch.full((C + 1,), GUARD_E, dtype=torch.float64, device="cuda")
        accept = torch.full((C + 1,), GUARD_ACC, dtype=torch.int32, device="cuda")
        return state, rung, out, energy, accept

    def raw(self, ladder_ptr, R, every, state_ptr, rung_ptr, C, id0, seed, sweep0, sweeps, init, out_ptr, energy_ptr, accept_ptr, dyn=None):
        return _lib.lib().dvg_gibbs_sample_tempered(self.gh.ptr, self.lin.data_ptr(), self.quad.data_ptr(), self.prefactor, -4.0,
                                                    4.0, -1.0, 1.0, ladder_ptr, R, every, state_ptr, rung_ptr, C, id0, seed, sweep0,
                                                    sweeps, init, out_ptr, energy_ptr, accept_ptr, dyn, _lib.stream_ptr())

    def tempered(self, bufs, ladder, every, id0, seed, sweep0, sweeps, init, outputs=(True, True, True)):
        state, rung, out, energy, accept = bufs
        C = int(state.shape[0]) - 1
        t = torch.from_numpy(np.ascontiguousarray(ladder, dtype=np.float32)).cuda()
        ptrs = [b.data_ptr() if on else None for b, on in zip((out, energy, accept), outputs)]
        _lib.check(self.raw(t.data_ptr(), int(t.shape[0]), every, state.data_ptr(), rung.data_ptr(), C, id0, seed, sweep0, sweeps,
                            init, *ptrs), "dvg_gibbs_sample_tempered")
        torch.cuda.synchronize()
        return [b.cpu().numpy() for b in bufs]


def _setup(name):
    plan, R, Q, every, sweeps, generic, p, h, J, hs, Js, ladder, ids = parameters(name)
    with _lib.option_scope(gibbs_generic=generic):
        got = dev.gibbs_exchange_plan(plan, Q, R)
    assert (got["form"], got["params"], got["chains_per_workgroup"], got["ladders_per_workgroup"], got["workgroups"]) == FORMS[name], got
    return plan, R, Q, every, sweeps, generic, p, hs, Js, ladder, ids, _Draw(plan, h, J, p["prefactor"])


def _guards(res, C, where):
    state, rung, out, energy, accept = res
    assert (state[C] == GUARD_STATE).all() and (out[C] == GUARD_OUT).all(), f"a row written past the last chain ({where})"
    assert rung[C] == GUARD_RUNG and energy[C] == GUARD_E and accept[C] == GUARD_ACC, f"an element written past the last chain ({where})"


# ------------------------------------------------------------------------------------------------ against the definition
@pytest.mark.parametrize("name", SHAPES)
def test_against_the_definition(name):
    plan, R, Q, every, sweeps, generic, p, _hs, _Js, ladder, _ids, d = _setup(name)
    C = Q * R
    want = definition(name)
    # no decision is left out: every coin of the helper's run is far from a tie
    for margin, bound, _accepted in want.coins:
        assert margin >= 1e6 * bound, (name, margin, bound)
    coins = len(want.coins)
    print(f"{name}: {coins} coin decisions, smallest |u - exp(d)| {min([c[0] for c in want.coins], default=np.nan):.3e}, largest "
          f"bound / margin {max([c[1] / c[0] for c in want.coins], default=np.nan):.3e}; accepted {want.accepted.sum(axis=0)[:-1]} of "
          f"{Q * want.attempts}")
    if name in BOTH_OUTCOMES:
        acc = want.accepted.sum(axis=0)[:-1]
        assert (acc > 0).all() and (acc < Q * want.attempts).all(), (name, acc, want.attempts)
    with _lib.option_scope(gibbs_generic=generic):
        res = d.tempered(d.buffers(C), ladder, every, p["id0"], SEED, SWEEP0, sweeps, 1)
    state, rung, out, energy, accept = res
    _guards(res, C, name)
    assert np.array_equal(rung[:C], want.rungs), f"rungs differ from the helper ({name})"
    assert int((state[:C] != want.spins).sum()) == 0, f"state differs from the helper ({name})"
    assert set(np.unique(out[:C]).tolist()) <= {-1.0, 1.0}
    assert int((out[:C] != want.samples.astype(np.float32)).sum()) == 0, f"samples_out (by rung) differs from the helper ({name})"
    assert np.array_equal(accept[:C].astype(np.int64).reshape(Q, R), want.accepted.astype(np.int64)), f"accept counts ({name})"
    by_rung = (np.arange(C) // R) * R + want.rungs
    unit = np.empty(C)
    unit[by_rung] = 4.0 * want.N * 2.0 ** -53 * want.A
    err = np.abs(energy[:C] - want.energy_by_rung)
    print(f"{name}: |energy| up to {np.abs(want.energy).max():.4g}, worst error {err.max():.3e} (its bound {unit[err.argmax()]:.3e})")
    assert np.isfinite(energy[:C]).all() and (err <= unit).all(), (name, err.max(), unit.min())
    assert (np.sort(rung[:C].reshape(Q, R), axis=1) == np.arange(R)).all() and not np.array_equal(rung[:C], np.arange(C) % R)


@pytest.mark.parametrize("name", ["pegasus64", "zephyr512x8", "random77"])
def test_outputs_may_be_null(name):
    plan, R, Q, every, sweeps, generic, p, _hs, _Js, ladder, _ids, d = _setup(name)
    C = Q * R
    want = definition(name)
    with _lib.option_scope(gibbs_generic=generic):
        res = d.tempered(d.buffers(C), ladder, every, p["id0"], SEED, SWEEP0, sweeps, 1, outputs=(False, False, False))
    state, rung, out, energy, accept = res
    assert np.array_equal(state[:C], want.spins) and np.array_equal(rung[:C], want.rungs) and state[C, 0] == GUARD_STATE
    assert (out == GUARD_OUT).all() and (energy == GUARD_E).all() and (accept == GUARD_ACC).all()


# ------------------------------------------------------------------------------------------------ against the other draws
@pytest.mark.parametrize("name", SHAPES)
def test_without_an_exchange_it_is_the_annealed_draw(name):
    """swap_every beyond the last sweep: no exchange, every chain keeps its rung -- the spins of dvg_gibbs_sample_annealed with
    a constant row per chain, the energies of dvg_gibbs_sample_ais (within the bound; A from the AIS helper), zero counts."""
    plan, R, Q, _every, sweeps, generic, p, hs, Js, ladder, ids, d = _setup(name)
    C, n = Q * R, plan.n
    table = np.repeat(np.tile(ladder, Q)[:, None], sweeps, axis=1).astype(np.float32)
    with _lib.option_scope(gibbs_generic=generic):
        res = d.tempered(d.buffers(C), ladder, SWEEP0 + sweeps + 1, p["id0"], SEED, SWEEP0, sweeps, 1)
        t = torch.from_numpy(table).cuda()
        st_a = torch.empty((C, n), dtype=torch.int8, device="cuda")
        out_a = torch.empty((C, n), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().dvg_gibbs_sample_annealed(d.gh.ptr, d.lin.data_ptr(), d.quad.data_ptr(), d.prefactor, -4.0, 4.0, -1.0, 1.0,
                                                        t.data_ptr(), sweeps, st_a.data_ptr(), C, p["id0"], SEED, SWEEP0, sweeps, 1,
                                                        out_a.data_ptr(), None, _lib.stream_ptr()), "dvg_gibbs_sample_annealed")
        st_w = torch.empty((C, n), dtype=torch.int8, device="cuda")
        log_w = torch.empty((C,), dtype=torch.float64, device="cuda")
        e_w = torch.empty((C,), dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib().dvg_gibbs_sample_ais(d.gh.ptr, d.lin.data_ptr(), d.quad.data_ptr(), d.prefactor, -4.0, 4.0, -1.0, 1.0,
                                                   t.data_ptr(), sweeps, 0.0, st_w.data_ptr(), C, p["id0"], SEED, SWEEP0, sweeps, 1, None,
                                                   log_w.data_ptr(), e_w.data_ptr(), None, _lib.stream_ptr()), "dvg_gibbs_sample_ais")
        torch.cuda.synchronize()
    state, rung, out, energy, accept = res
    _guards(res, C, name)
    assert np.array_equal(state[:C], st_a.cpu().numpy()) and np.array_equal(out[:C], out_a.cpu().numpy())
    assert np.array_equal(rung[:C], np.arange(C) % R) and (accept[:C] == 0).all()
    want = ais_oracle.ais(plan, hs, Js, table, ids, SEED, SWEEP0)
    assert np.array_equal(state[:C], want.spins)
    unit = 4.0 * want.N * 2.0 ** -53 * want.A
    assert (np.abs(energy[:C] - e_w.cpu().numpy()) <= unit).all() and (np.abs(energy[:C] - want.energy) <= unit).all()


def _odd_even(R, sweep0, sweeps, every):
    """The rungs of a ladder whose every exchange is accepted, and the accepted exchanges per pair."""
    rung, acc = np.arange(R), np.zeros(R, dtype=np.int64)
    for t in range(sweep0, sweep0 + sweeps):
        if (t + 1) % every == 0:
            for r in range(((t + 1) // every) & 1, R - 1, 2):
                a, b = np.flatnonzero(rung == r)[0], np.flatnonzero(rung == r + 1)[0]
                rung[a], rung[b] = r + 1, r
                acc[r] += 1
    return rung, acc


@pytest.mark.parametrize("name", SHAPES)
def test_equal_betas_accept_every_exchange_and_are_the_plain_draw(name):
    """All R betas equal: d = 0 at every exchange, all accepted.  The rungs follow the odd-even transposition pattern, the
    accept counts are the attempts, and the spins are dvg_gibbs_sample's at that beta."""
    plan, R, Q, every, sweeps, generic, p, _hs, _Js, _ladder, _ids, d = _setup(name)
    C, n = Q * R, plan.n
    with _lib.option_scope(gibbs_generic=generic):
        res = d.tempered(d.buffers(C), np.full(R, p["beta"], np.float32), every, p["id0"], SEED, SWEEP0, sweeps, 1)
        st_p = torch.empty((C, n), dtype=torch.int8, device="cuda")
        _lib.check(_lib.lib().dvg_gibbs_sample(d.gh.ptr, d.lin.data_ptr(), d.quad.data_ptr(), d.prefactor, -4.0, 4.0, -1.0, 1.0,
                                               p["beta"], st_p.data_ptr(), C, p["id0"], SEED, SWEEP0, sweeps, 1, None, None,
                                               _lib.stream_ptr()), "dvg_gibbs_sample")
        torch.cuda.synchronize()
    state, rung, out, _energy, accept = res
    _guards(res, C, name)
    want_rung, want_acc = _odd_even(R, SWEEP0, sweeps, every)
    assert np.array_equal(want_acc[:-1], tempered_oracle.attempts(R, SWEEP0, sweeps, every)) and want_acc.sum() > 0
    assert np.array_equal(rung[:C].reshape(Q, R), np.tile(want_rung, (Q, 1)))
    assert np.array_equal(accept[:C].reshape(Q, R), np.tile(want_acc, (Q, 1)))
    plain = st_p.cpu().numpy()
    assert np.array_equal(state[:C], plain)
    by_rung = (np.arange(C) // R) * R + rung[:C]
    assert np.array_equal(out[:C][by_rung], plain.astype(np.float32))


@pytest.mark.parametrize("name,first", [("pegasus64", 5), ("zephyr512x8", 4)])
def test_two_calls_continue_the_draw(name, first):
    """One call of S sweeps against two calls that hand state and rung on with sweep0 advanced: the same spins, rungs and
    samples, the accept counts add up.  The second call sums its start energies afresh, from float32 fields, where the one call
    carries them: the helper gives how far the two lie apart at the hand-over (delta; the same updates follow on both routes),
    which moves a d by at most 2 |dbeta| delta -- the margins of this shape's coins are asserted to be 1000 times that."""
    plan, R, Q, every, sweeps, generic, p, hs, Js, ladder, ids, d = _setup(name)
    C = Q * R
    want = definition(name)
    half = tempered_oracle.tempered(plan, hs, Js, ladder, ids, SEED, SWEEP0, first, every)
    fresh = tempered_oracle.tempered(plan, hs, Js, ladder, ids, SEED, SWEEP0 + first, 0, every, start=half.spins, rungs=half.rungs)
    delta = float(np.abs(half.energy - fresh.energy).max())
    slack = 2.0 * float(np.abs(np.diff(ladder.astype(np.float64))).max()) * delta
    print(f"{name}: carried and fresh energies up to {delta:.3e} apart at the hand-over; smallest margin {min(c[0] for c in want.coins):.3e}")
    assert all(margin > 1e3 * slack for margin, _b, _a in want.coins)
    with _lib.option_scope(gibbs_generic=generic):
        one = d.tempered(d.buffers(C), ladder, every, p["id0"], SEED, SWEEP0, sweeps, 1)
        a = d.tempered(d.buffers(C), ladder, every, p["id0"], SEED, SWEEP0, first, 1)
        b = d.tempered(d.buffers(C, start=a[0][:C], rungs=a[1][:C]), ladder, every, p["id0"], SEED, SWEEP0 + first, sweeps - first, 0)
    _guards(b, C, name)
    assert np.array_equal(one[0][:C], want.spins) and np.array_equal(one[1][:C], want.rungs)
    assert np.array_equal(b[0], one[0]) and np.array_equal(b[1], one[1]) and np.array_equal(b[2], one[2])
    assert np.array_equal(a[4][:C] + b[4][:C], one[4][:C]) and not np.array_equal(a[1][:C], np.arange(C) % R)
    assert (np.abs(b[3][:C] - one[3][:C]) <= 2.0 * delta + 4.0 * want.N * 2.0 ** -53 * want.A.max()).all()


def test_invalid_arguments_launch_nothing():
    plan, R, Q, every, sweeps, _generic, p, _hs, _Js, ladder, _ids, d = _setup("zephyr128")
    C = Q * R
    state, rung, out, energy, accept = bufs = d.buffers(C, start=np.ones((C, plan.n), np.int8), rungs=np.arange(C) % R)
    before = [b.clone() for b in bufs]
    t = torch.from_numpy(ladder).cuda()
    lp, sp, rp = t.data_ptr(), state.data_ptr(), rung.data_ptr()
    #        ladder R every state rung chains sweeps dyn
    cases = [(None, R, 1, sp, rp, C, sweeps, None), (lp, R, 1, sp, None, C, sweeps, None), (lp, 1, 1, sp, rp, C, sweeps, None),
             (lp, 17, 1, sp, rp, 34, sweeps, None), (lp, R, 1, sp, rp, C - 1, sweeps, None), (lp, R, 0, sp, rp, C, sweeps, None),
             (lp, R, 1, sp, rp, C, 0, None), (lp, R, 1, sp, rp, C, sweeps, out.data_ptr()), (lp, R, 1, None, rp, C, sweeps, None)]
    for ladder_ptr, reps, ev, state_ptr, rung_ptr, chains, s, dyn in cases:
        rc = d.raw(ladder_ptr, reps, ev, state_ptr, rung_ptr, chains, p["id0"], SEED, SWEEP0, s, 0, out.data_ptr(), energy.data_ptr(),
                   accept.data_ptr(), dyn)
        assert rc == -1, (reps, ev, chains, s, rc, _lib.lib().dvg_last_error())
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(bufs, before))


# ------------------------------------------------------------------------------------------------ the Python surface
def test_sample_tempered_of_the_sampler():
    plan, nodes = _solver_plan("zephyr", 128)
    _plan, R, Q, _every, _sweeps, _generic, p, h, J, hs, Js, ladder, _ids = parameters("zephyr128")
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5, h_range=(-4, 4), j_range=(-1, 1))
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    first = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=16).clone()
    before = (s._state.clone(), s.sweep_count, s.calls, s.cond_sweep_count, s.anneal_sweep_count, s.ais_sweep_count)
    ids = np.arange(Q * R, dtype=np.uint32) + 5
    assert s.pt_seed == SEED ^ 0x70743031 and s.pt_sweep_count == 0

    res = s.sample_tempered(lin, quad, 0.05, (-4, 4), (-1, 1), ladder, num_ladders=Q, num_sweeps=7, swap_every=2)
    n = plan.n
    assert res.samples.shape == (Q, R, n) and res.samples.dtype == torch.float32 and res.samples.is_cuda
    assert res.energies.shape == (Q, R) and res.energies.dtype == torch.float64 and res.accepted.shape == (Q, R - 1)
    assert res.attempts.shape == (R - 1,) and res.acceptance_rate.shape == (R - 1,) and res.target.shape == (Q, n)
    assert torch.equal(res.target, res.samples[:, -1]) and res.state.shape == (Q * R, n) and res.rungs.shape == (Q * R,)
    assert s.pt_sweep_count == 7
    want = tempered_oracle.tempered(plan, hs, Js, ladder, ids, s.pt_seed, 0, 7, 2)
    assert all(margin >= 1e6 * bound for margin, bound, _a in want.coins)
    assert np.array_equal(res.samples.cpu().numpy().reshape(Q * R, n), want.samples.astype(np.float32))
    assert np.array_equal(res.state.cpu().numpy(), want.spins) and np.array_equal(res.rungs.cpu().numpy(), want.rungs)
    assert np.array_equal(res.accepted.cpu().numpy(), want.accepted[:, :-1].astype(np.int64)) and np.array_equal(res.attempts, want.attempts)
    rate = want.accepted[:, :-1].sum(axis=0) / (Q * want.attempts)
    assert np.allclose(res.acceptance_rate.cpu().numpy(), rate, rtol=0, atol=1e-15)

    # continue: sweeps 7 .. 11 from the result's state and rungs (int64 rungs and a float32 state are taken as well)
    more = s.sample_tempered(lin, quad, 0.05, (-4, 4), (-1, 1), ladder, num_ladders=Q, num_sweeps=5, swap_every=2,
                             start=res.state.float(), rungs=res.rungs.long())
    assert s.pt_sweep_count == 12
    want2 = tempered_oracle.tempered(plan, hs, Js, ladder, ids, s.pt_seed, 7, 5, 2, start=want.spins, rungs=want.rungs)
    assert all(margin >= 1e6 * bound for margin, bound, _a in want2.coins)
    assert np.array_equal(more.state.cpu().numpy(), want2.spins) and np.array_equal(more.rungs.cpu().numpy(), want2.rungs)
    assert np.array_equal(res.state.cpu().numpy(), want.spins)  # (the first result's tensors are its own)

    # the other streams never noticed
    assert torch.equal(s._state, before[0]) and (s.sweep_count, s.calls, s.cond_sweep_count, s.anneal_sweep_count, s.ais_sweep_count) == before[1:]
    ref = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5, h_range=(-4, 4), j_range=(-1, 1))
    ref_draws = [ref.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=16).clone() for _ in range(2)]
    assert torch.equal(first, ref_draws[0]) and torch.equal(s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=16), ref_draws[1])
    s.reset()
    assert s.pt_sweep_count == 0


def test_generate_images_from_tempered_ladders():
    from image_generation_amd.model_wrapper import ModelWrapper

    def wrapper():
        torch.manual_seed(0)
        m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
        m.setup()
        return m

    default = wrapper().generate_images()
    m = wrapper()
    s, reads = m.sampler, int(m.sampler_kwargs.get("num_reads", 1))
    ladder = smp.beta_schedule(10.0, 20.0, 4)
    imgs = m.generate_images(tempered=dict(betas=ladder, num_sweeps=6, swap_every=2))
    assert imgs.shape == (reads, 1, 32, 32) and torch.isfinite(imgs).all()
    assert (s.pt_sweep_count, s.sweep_count, s.calls, s.anneal_sweep_count) == (6, 0, 0, 0) and s._state is None
    # the target rung of the same ladders, drawn directly (the next sweeps of the stream would differ: a sampler of its own)
    other = wrapper()
    res = other._grbm.sample_tempered(other.sampler, ladder, prefactor=other.PREFACTOR, linear_range=other.linear_range,
                                      quadratic_range=other.quadratic_range, num_ladders=reads, num_sweeps=6, swap_every=2)
    with torch.no_grad():
        decoded = m._dvae.decoder(res.target.unsqueeze(1)).squeeze(1).clip(0.0, 1.0)  # (m: in evaluation mode, the same weights)
    assert torch.equal(imgs, decoded)
    with pytest.raises(ValueError):
        m.generate_images(betas=[1.0, 2.0], tempered=dict(betas=ladder))
    with pytest.raises(ValueError):
        m.generate_images(tempered=dict(num_sweeps=3))
    # the default call is what it was: the sampler's own chains, untouched by the ladders drawn before it
    assert torch.equal(m.generate_images(), default)
