"""CPU-side checks of the exchange draw ("DVG PT v1", ``dvg_gibbs_sample_tempered`` in include/dvg.h): the symbol, every
argument error of the C entry point (before any launch) and of the Python surface (before the library is touched), the
draw's own key and counter, the definition itself (``tests/tempered_oracle.py``) against enumeration, its continuation, and
the plan an exchange draw takes on the graphs the GPU tests use."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tempered_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, dev, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dvg_gibbs_sample_tempered"
SEED = 775321899904


# ------------------------------------------------------------------------------------------------ the symbol and its checks
def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported(NAME, markers=["DVG PT v1", "STREAM_SWAP = 4"])
    assert "STREAM_SWAP = 4" in open(os.path.join(ROOT, "image-generation_amd", "csrc", "philox.h")).read()


def _call(g, lin, quad, state, ladder, rung, *, R=4, swap_every=1, n_chains=8, n_sweeps=3, dyn=None):
    L = _lib.lib()
    rc = L.dvg_gibbs_sample_tempered(g, lin, quad, 1.0, -1, 1, -1, 1, ladder, R, swap_every, state, rung, n_chains, 0, 0, 0,
                                     n_sweeps, 1, None, None, None, dyn, None)
    return rc, L.dvg_last_error()


def test_argument_validation_without_gpu():
    """Everything the header lists is DVG_E_INVALID (-1) with a message, before any HIP call."""
    rc, msg = _call(None, None, None, None, None, None)
    assert rc == -1 and b"null" in msg
    graph = ctypes.create_string_buffer(4096)  # a host-memory stand-in for the graph handle (first field: the spin count)
    ctypes.c_int32.from_buffer(graph).value = 64
    g = ctypes.cast(graph, ctypes.c_void_p)
    dummy = ctypes.create_string_buffer(16)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    rc, msg = _call(g, p, p, None, p, p)
    assert rc == -1 and b"null" in msg
    rc, msg = _call(g, p, p, p, None, p)
    assert rc == -1 and b"ladder" in msg
    rc, msg = _call(g, p, p, p, p, None)
    assert rc == -1 and b"rung" in msg
    for R in (-1, 0, 1, 17, 64):
        rc, msg = _call(g, p, p, p, p, p, R=R, n_chains=max(R, 1) * 2)
        assert rc == -1 and b"n_replicas" in msg, (R, rc, msg)
    for R, C in ((4, 6), (3, 8), (16, 8), (2, 7)):
        rc, msg = _call(g, p, p, p, p, p, R=R, n_chains=C)
        assert rc == -1 and b"multiple" in msg, (R, C, rc, msg)
    for n_chains in (0, -4):
        rc, msg = _call(g, p, p, p, p, p, n_chains=n_chains)
        assert rc == -1 and b"n_chains" in msg
    for swap_every in (0, -1):
        rc, msg = _call(g, p, p, p, p, p, swap_every=swap_every)
        assert rc == -1 and b"swap_every" in msg
    for n_sweeps in (0, -1):
        rc, msg = _call(g, p, p, p, p, p, n_sweeps=n_sweeps)
        assert rc == -1 and b"n_sweeps" in msg
    rc, msg = _call(g, p, p, p, p, p, dyn=p)
    assert rc == -1 and b"dyn" in msg
    ctypes.c_int32.from_buffer(graph).value = 40000
    rc, msg = _call(g, p, p, p, p, p)
    assert rc == -1 and b"too large" in msg


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


BAD_LADDERS = [
    ([0.1, -0.5, 1.0], ValueError), ([0.1, float("nan")], ValueError), ([0.1, float("inf")], ValueError),
    (np.array([1e39, 1.0]), ValueError), (torch.tensor([0.5, -1.0]), ValueError), ([], _lib.DvgError), ([1.0], _lib.DvgError),
    (np.linspace(0.1, 2.0, 17), _lib.DvgError), (np.ones((2, 4)), _lib.DvgError), (3.0, _lib.DvgError), (["a", "b"], ValueError),
]


@pytest.mark.parametrize("betas,exc", BAD_LADDERS)
def test_sample_tempered_rejects_bad_ladders(untouched, betas, exc):
    s, lin, quad = untouched
    with pytest.raises(exc):
        s.sample_tempered(lin, quad, 1.0, None, None, betas, num_ladders=4)
    assert s.pt_sweep_count == 0


def test_sample_tempered_rejects_bad_arguments(untouched):
    s, lin, quad = untouched
    n, ok = s.plan.n, [0.1, 1.0, 2.0]
    call = lambda **kw: s.sample_tempered(lin, quad, 1.0, None, None, ok, **kw)  # noqa: E731
    with pytest.raises(TypeError):
        call()  # how many ladders?
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
    with pytest.raises(_lib.DvgError):  # valid arguments, CPU parameters: the HIP path has no CPU fallback
        call(num_ladders=2)
    assert (s.pt_sweep_count, s.ais_sweep_count, s.anneal_sweep_count, s.sweep_count, s.calls, s.cond_sweep_count) == (0,) * 6


def test_tempered_draws_have_their_own_key_and_counter(untouched):
    s, _lin, _quad = untouched
    assert s.pt_seed == 3 ^ 0x70743031 and s.pt_seed not in (s.seed, s.cond_seed, s.anneal_seed, s.ais_seed) and s.pt_sweep_count == 0
    s.pt_sweep_count, s.ais_sweep_count, s.sweep_count = 5, 6, 7
    s.reset()
    assert (s.pt_sweep_count, s.ais_sweep_count, s.sweep_count) == (0, 0, 0)


def test_grbm_sample_tempered_takes_the_local_sampler_only(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    s, _lin, _quad = untouched
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for other in (object(), smp.GibbsSampler(s.plan, [f"q{i}" for i in range(12)], beta=2.0, sweeps=5, seed=3, device="cuda")):
        with pytest.raises(TypeError):
            grbm.sample_tempered(other, [0.5, 1.0], prefactor=1.0, num_ladders=2)


@pytest.mark.parametrize("R,sweep0,S,every", [(4, 6, 12, 1), (8, 6, 12, 2), (8, 6, 12, 3), (3, 0, 5, 1), (2, 7, 9, 4), (16, 6, 4, 1), (5, 6, 12, 100)])
def test_result_object_counts_the_attempts_as_the_definition_does(R, sweep0, S, every):
    Q, n = 3, 5
    out, energy = torch.zeros((Q * R, n)), torch.zeros(Q * R, dtype=torch.float64)
    accept = torch.arange(Q * R, dtype=torch.int32)
    res = smp.Tempered.from_draw(n, R, out, energy, accept, sweep0, S, every, None, None)
    assert np.array_equal(res.attempts, tempered_oracle.attempts(R, sweep0, S, every)) and res.attempts.shape == (R - 1,)
    assert res.samples.shape == (Q, R, n) and res.energies.shape == (Q, R) and res.accepted.shape == (Q, R - 1)
    assert res.target.shape == (Q, n) and res.acceptance_rate.shape == (R - 1,)
    assert torch.equal(res.accepted, accept.view(Q, R)[:, :R - 1].long())


# ------------------------------------------------------------------------------------------------ the definition, sampled
@functools.lru_cache(maxsize=None)
def _case16():
    """A 16-spin random graph with normal (h, J), ladder (0.2, 0.5, 1, 2), 512 ladders."""
    n = 16
    rng = np.random.default_rng(16)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.uniform(size=iu.size) < 0.3
    plan = graphs.build_plan(n, iu[keep].astype(np.int64), ju[keep].astype(np.int64))
    h = (0.5 * rng.normal(size=n)).astype(np.float32)
    J = rng.normal(size=plan.n_edges).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 1.0, (-4, 4), (-1, 1))
    ladder = np.array([0.2, 0.5, 1.0, 2.0], dtype=np.float32)
    Q = 512
    ids = np.arange(Q * ladder.size, dtype=np.uint32) + 11
    exact = [tempered_oracle.boltzmann_energy_moments(n, hs, Js, np.asarray(plan.edge_i), np.asarray(plan.edge_j), float(b))
             for b in ladder]
    return plan, hs, Js, ladder, Q, ids, exact


def _sigmas(flip):
    plan, hs, Js, ladder, Q, ids, exact = _case16()
    r = tempered_oracle.tempered(plan, hs, Js, ladder, ids, SEED ^ 0x70743031, 5, 60, 1, flip_sign=flip)
    means = r.energy_by_rung.reshape(Q, ladder.size).mean(axis=0)
    z = np.array([(means[k] - m) / (sd / np.sqrt(Q)) for k, (m, sd) in enumerate(exact)])
    print(f"flip_sign={flip}: per-rung mean energy off by {np.round(z, 2)} exact sigma / sqrt(Q); accepted {r.accepted.sum(axis=0)[:-1]} "
          f"of {Q * r.attempts}")
    return z, r


def test_the_definition_samples_the_boltzmann_distribution_of_every_rung():
    """60 sweeps with an exchange after each: the mean energy of the 512 chains that end on rung r lies within 5 exact
    sigma / sqrt(Q) of the enumerated Boltzmann mean at beta_r (2^16 states)."""
    z, r = _sigmas(False)
    assert (np.abs(z) <= 5.0).all(), z
    assert (r.accepted[:, -1] == 0).all() and (r.accepted.sum(axis=0)[:-1] > 0).all()
    # (the rungs of a ladder stay a permutation)
    assert (np.sort(r.rungs.reshape(-1, 4), axis=1) == np.arange(4)).all()


def test_the_sampling_test_has_teeth():
    """The same rule with the sign of d flipped misses by far more than 5."""
    z, _r = _sigmas(True)
    assert np.abs(z).max() > 5.0, z


def test_two_calls_continue_the_draw():
    """S1 + S2 sweeps in two calls that hand state and rungs on, sweep0 advanced by S1, are the one-call draw: spins, rungs,
    accept counts; the energies agree as far as float32 fields let a carried energy and a fresh start sum agree."""
    plan, hs, Js, ladder, _Q, ids, _exact = _case16()
    ids = ids[:24]
    key, sweep0 = SEED ^ 0x70743031, 6
    for every, s1 in ((1, 5), (2, 5), (3, 4)):
        one = tempered_oracle.tempered(plan, hs, Js, ladder, ids, key, sweep0, 12, every)
        a = tempered_oracle.tempered(plan, hs, Js, ladder, ids, key, sweep0, s1, every)
        start = tempered_oracle.cref.init_state(ids, plan.n, key, sweep0)  # (a fresh draw starts where the one call did)
        assert np.array_equal(tempered_oracle.tempered(plan, hs, Js, ladder, ids, key, sweep0, s1, every, start=start,
                                                       rungs=np.arange(24) % 4).spins, a.spins)
        b = tempered_oracle.tempered(plan, hs, Js, ladder, ids, key, sweep0 + s1, 12 - s1, every, start=a.spins, rungs=a.rungs)
        assert np.array_equal(b.spins, one.spins) and np.array_equal(b.rungs, one.rungs) and np.array_equal(b.samples, one.samples)
        assert np.array_equal(a.accepted + b.accepted, one.accepted) and np.array_equal(a.attempts + b.attempts, one.attempts)
        # (the carried energy and the fresh start sum both lie within B of the exact energy: a float32 field of degree d is
        # off by at most g = d u / (1 - d u) times F_i = |hs_i| + sum_j |Js_ij|, u = 2^-24; the start sum has n addends
        # 1/2 s_i (hs_i + f_i), every one of the at most n S updates adds +-2 f_i)
        deg = np.diff(np.asarray(plan.adj_ptr))
        F = np.abs(hs.astype(np.float64)) + np.add.reduceat(np.append(np.abs(Js.astype(np.float64))[np.asarray(plan.adj_eid)], 0.0),
                                                            np.asarray(plan.adj_ptr)[:-1]) * (deg > 0)
        g = deg.max() * 2.0 ** -24 / (1.0 - deg.max() * 2.0 ** -24)
        B = g * (0.5 * plan.n + 2.0 * plan.n * 12) * F.max()
        assert np.abs(b.energy - one.energy).max() <= 2.0 * B
        assert one.accepted.sum() > 0 and not np.array_equal(one.rungs, np.arange(24) % 4)


# ------------------------------------------------------------------------------------------------ the plan
_solver_plan = support.solver_plan


_random_plan = functools.partial(support.random_plan, isolated=3)


def _lane(lpc, waves, mb, nr, maxs):
    return "lane", dict(LPC=lpc, WAVES=waves, MB=mb, NR=nr, MAXS=maxs)


def _rolled(lpc, waves):
    return "rolled", dict(LPC=lpc, WAVES=waves)


# graph, ladders, replicas, gibbs_generic -> form, chain slots per workgroup, ladders per workgroup: written from the rule
# (the table kind's plan if its workgroup holds a ladder; else that family at 4 waves; else rolled (64, 16))
PLANS = [
    ("pegasus64", 3, 2, 0, _lane(32, 1, 4, 1, 12), 2, 1),
    ("pegasus64", 3, 4, 0, _lane(32, 4, 4, 1, 12), 8, 2),
    ("pegasus64", 3, 8, 0, _lane(32, 4, 4, 1, 12), 8, 1),
    ("pegasus64", 3, 16, 0, _rolled(64, 16), 16, 1),
    ("pegasus64", 300, 4, 0, _lane(32, 4, 4, 1, 12), 8, 2),
    ("zephyr512", 3, 2, 0, _lane(64, 4, 5, 2, 12), 4, 2),
    ("zephyr512", 3, 4, 0, _lane(64, 4, 5, 2, 12), 4, 1),
    ("zephyr512", 3, 4, 2, _lane(64, 4, 5, 1, 12), 4, 1),
    ("zephyr512", 3, 4, 3, _lane(64, 4, 5, 2, 12), 4, 1),
    ("zephyr512", 3, 4, 4, _lane(64, 4, 5, 2, 12), 4, 1),
    ("zephyr512", 3, 4, 1, _rolled(64, 4), 4, 1),
    ("zephyr512", 3, 5, 0, _rolled(64, 16), 16, 3),
    ("zephyr512", 3, 8, 0, _rolled(64, 16), 16, 2),
    ("zephyr512", 3, 8, 1, _rolled(64, 16), 16, 2),
    ("zephyr512", 256, 4, 0, _lane(64, 4, 5, 2, 12), 4, 1),
    ("zephyr1024", 2, 4, 0, _lane(64, 4, 5, 2, 20), 4, 1),
    ("zephyr1024", 128, 4, 0, _lane(64, 4, 5, 2, 20), 4, 1),
    ("zephyr1024", 2, 16, 0, _rolled(64, 16), 16, 1),
    ("zephyr1024", 2, 8, 0, _rolled(64, 16), 16, 2),
    ("zephyr1024", 129, 4, 0, _rolled(64, 16), 16, 4),
    ("random77", 5, 3, 0, _rolled(16, 1), 4, 1),
    ("random77", 5, 16, 0, _rolled(16, 4), 16, 1),
]


@pytest.mark.parametrize("name,Q,R,generic,form,slots,per_block", PLANS)
def test_exchange_plans(name, Q, R, generic, form, slots, per_block):
    plan = {"pegasus64": lambda: _solver_plan("pegasus", 64), "zephyr512": lambda: _solver_plan("zephyr", 512),
            "zephyr1024": lambda: _solver_plan("zephyr", 1024), "random77": _random_plan}[name]()
    with _lib.option_scope(gibbs_generic=generic):
        p = dev.gibbs_exchange_plan(plan, Q, R)
        table = dev.gibbs_draw_plan(plan, Q * R, "table")
    assert (p["form"], p["params"]) == form, p
    assert (p["chains_per_workgroup"], p["ladders_per_workgroup"]) == (slots, per_block) and slots // R == per_block
    assert p["workgroups"] == -(-Q // per_block) and p["threads"] == 64 * form[1]["WAVES"]
    # the form's own image (a table draw of that form with as many slots) plus the exchange's: two float64 mailboxes and a
    # uint32 counter per slot, sixteen float32 betas, behind the image rounded up to 8 bytes
    if form[0] == "lane":
        li = p["lane_image"]
        own = 24 * li["rows"] * form[1]["MB"] * form[1]["LPC"] + 2 * slots * ((plan.n + 15) & ~15) + 128 * ((slots * form[1]["LPC"] + 63) // 64)
    else:
        front = 4 * ((plan.n + 3) & ~3) + 16 * (p["n_batches"] + 1) + 4 * plan.n + 4 * (plan.n_colours + 1)
        front = ((front + 7) & ~7) + 8 * (p["n_batches"] + 1) + 2 * ((plan.n + 1) & ~1)
        own = front + 2 * slots * ((plan.n + 15) & ~15)
    if (table["form"], table["params"]) == form:
        assert own == table["lds_bytes"]  # (the table kind's plan, kept: the same image)
    assert p["lds_bytes"] == ((own + 7) & ~7) + 16 * slots + 4 * slots + 64 and p["lds_bytes"] <= 160 * 1024


def test_the_other_kinds_plan_as_before_and_bad_arguments_are_rejected():
    plan = _solver_plan("pegasus", 64)
    assert dev.GIBBS_KINDS == ("plain", "held", "table", "weigh")
    assert dev.gibbs_draw_plan(plan, 12, "table")["params"] == dict(LPC=32, WAVES=1, MB=4, NR=1, MAXS=12)
    for Q, R in ((0, 4), (3, 1), (3, 17), (3, 0)):
        with pytest.raises(_lib.DvgError):
            dev.gibbs_exchange_plan(plan, Q, R)
