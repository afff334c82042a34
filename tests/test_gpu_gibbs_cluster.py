"""GPU checks of the isoenergetic cluster move (``dvg_gibbs_cluster_move``, "DVG ICM v1") and of the draw composed of it and the
exchange draw (``GibbsSampler.sample_tempered_cluster``) against the numpy definition (``tests/cluster_oracle.py``).

The move is integers only: ``state``, ``sizes`` and ``differ`` equal the definition bit for bit, with a guard row or element behind
every buffer.  ``random70``: n = 70 (two 64-spin chunks, the second of 6 spins), spin 0 a hub of degree 66; R = 3 with 5 twin pairs,
rungs permuted per ladder.  ``path200``: a path with b = -a -- D is every site and the cluster the whole path, grown over the
order of n passes -- and two disjoint paths, of which only the root's moves.  ``random33``: R = 1 without a rung table, 70 pairs, some
of them identical twins.  ``zephyr128``: the project's Zephyr subgraph, R = 16, states after 20 sweeps of the exchange draw.
``tiling``: more jobs (4200) than the launch has workgroups (4096).

The composed draw is held to the composed definition under the exchange tests' own condition: the seed of (h, J) was picked, with
the definition alone, so that every exchange coin of its run is at least 10^6 error bounds from a tie -- asserted here."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as co  # noqa: E402
import tempered_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
KEY = SEED ^ 0x70743031  # the exchange draw's key, which is the move's
MAX_GRID = 4096  # CL_MAX_GRID, csrc/cluster.hip
GUARD_STATE, GUARD_OUT = 55, 123456


# ------------------------------------------------------------------------------------------------ graphs
@functools.lru_cache(maxsize=None)
def _zephyr_plan(n=128):
    mg, _ = graphs.get_graph_mapping(graphs.greedy_get_subgraph(n, SEED, graphs.zephyr_graph(12)))
    nodes, ei, ej = graphs.edges_of(mg)
    return graphs.build_plan(n, ei, ej), nodes


def _random_plan(n, hub_degree=0, p_edge=0.08):
    return support.random_plan(n, p_edge, hub_degree=hub_degree, with_nodes=True)


@functools.lru_cache(maxsize=None)
def _path_plan(n, cut=None):
    """The path 0 - 1 - .. - n-1; with ``cut`` the edge (cut - 1, cut) is left out: two disjoint paths."""
    i = np.array([k for k in range(n - 1) if k + 1 != cut], dtype=np.int64)
    return graphs.build_plan(n, i, i + 1), list(range(n))


def _sampler(plan, nodes, chain_offset=0, **kw):
    return smp.GibbsSampler(plan, nodes, beta=kw.pop("beta", 1.0), sweeps=4, seed=SEED, device="cuda", chain_offset=chain_offset, **kw)


def _permuted_rungs(rng, Q, R):
    return np.concatenate([rng.permutation(R) for _ in range(Q)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the move alone
def _moved(plan, nodes, spins, rungs, R, rung_from, move, id0=0):
    """The sampler's cluster_move on device copies with a guard row / element behind each buffer.  Returns (state, sizes, differ)
    as numpy, the outputs through the ClusterMoves object."""
    C, n = spins.shape
    s = _sampler(plan, nodes, chain_offset=id0)
    state = torch.full((C + 1, n), GUARD_STATE, dtype=torch.int8, device="cuda")
    state[:C] = torch.from_numpy(np.ascontiguousarray(spins, dtype=np.int8)).cuda()
    rung = None if rungs is None else torch.from_numpy(np.ascontiguousarray(rungs, dtype=np.int32)).cuda()
    before = None if rung is None else rung.clone()
    m = s.cluster_move(state[:C], rung, replicas=R, rung_from=rung_from, move=move)
    torch.cuda.synchronize()
    assert (state[C] == GUARD_STATE).all(), "a row written past the last chain"
    assert rung is None or torch.equal(rung, before), "the rung table is read only"
    assert tuple(m.sizes.shape) == (C // (2 * R), R) == tuple(m.differ.shape) and m.sizes.dtype == torch.int64 and m.sizes.is_cuda
    assert (s.pt_sweep_count, s.sweep_count, s.calls) == (0, 0, 0) and s._state is None
    return state[:C].cpu().numpy(), m.sizes.cpu().numpy(), m.differ.cpu().numpy()


def _same(got, want, where):
    state, sizes, differ = got
    assert np.array_equal(differ, want.differ.astype(np.int64)), f"differ_out differs from the definition ({where})"
    assert np.array_equal(sizes, want.sizes.astype(np.int64)), f"size_out differs from the definition ({where})"
    bad = np.argwhere(state != want.spins)
    assert bad.size == 0, f"{len(bad)} spins differ from the definition ({where}), the first at (chain, spin) {bad[0]}"


@pytest.mark.parametrize("rung_from", [0, 2])
def test_random_graph_with_a_hub_equals_the_definition(rung_from):
    (plan, nodes), R, P, id0 = _random_plan(70, 66), 3, 5, 4294967290  # (the ladders' ids wrap round 2^32)
    rng = np.random.default_rng(70)
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(2 * P * R, plan.n))
    rungs = _permuted_rungs(rng, 2 * P, R)
    want = co.cluster_move(plan, spins, rungs, R, rung_from, id0, KEY, 9)
    assert (want.sizes[:, rung_from:] > 1).any() and (want.sizes < want.differ)[:, rung_from:].any() and not want.sizes[:, :rung_from].any()
    _same(_moved(plan, nodes, spins, rungs, R, rung_from, 9, id0), want, f"random70 from rung {rung_from}")


def test_the_raw_entry_point_with_null_outputs_and_guards():
    """The C entry point itself: either output may be NULL; nothing is written behind size_out, differ_out or state."""
    (plan, _nodes), R, P = _random_plan(70, 66), 3, 5
    rng = np.random.default_rng(71)
    C, jobs = 2 * P * R, P * R
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(C, plan.n))
    rungs = _permuted_rungs(rng, 2 * P, R)
    want = co.cluster_move(plan, spins, rungs, R, 1, 7, KEY, 3)
    gh = smp.GraphHandle(plan, "cuda")
    rung = torch.from_numpy(rungs).cuda()
    for with_sizes, with_differ in ((True, True), (False, True), (True, False), (False, False)):
        state = torch.full((C + 1, plan.n), GUARD_STATE, dtype=torch.int8, device="cuda")
        state[:C] = torch.from_numpy(spins).cuda()
        sizes = torch.full((jobs + 1,), GUARD_OUT, dtype=torch.int32, device="cuda")
        differ = torch.full((jobs + 1,), GUARD_OUT, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib().dvg_gibbs_cluster_move(gh.ptr, state.data_ptr(), rung.data_ptr(), C, R, 1, 7, KEY, 3,
                                                     sizes.data_ptr() if with_sizes else None, differ.data_ptr() if with_differ else None,
                                                     _lib.stream_ptr()), "dvg_gibbs_cluster_move")
        torch.cuda.synchronize()
        assert np.array_equal(state[:C].cpu().numpy(), want.spins) and (state[C] == GUARD_STATE).all()
        assert np.array_equal(sizes.cpu().numpy()[:jobs], want.sizes.ravel()) if with_sizes else (sizes == GUARD_OUT).all()
        assert np.array_equal(differ.cpu().numpy()[:jobs], want.differ.ravel()) if with_differ else (differ == GUARD_OUT).all()
        assert int(sizes[jobs]) == GUARD_OUT and int(differ[jobs]) == GUARD_OUT


@pytest.mark.parametrize("cut", [None, 77])
def test_a_path_grows_to_the_whole_component(cut):
    """b = -a on a path: D is every site.  Whole: the cluster is all 200 sites, whatever the root -- the growth takes the order of
    n passes.  Cut in two: the root's path moves, the other stays."""
    n, P = 200, 3
    plan, nodes = _path_plan(n, cut)
    rng = np.random.default_rng(200)
    a = rng.choice(np.array([-1, 1], dtype=np.int8), size=(P, n))
    spins = np.stack([a, -a], axis=1).reshape(2 * P, n)
    want = co.cluster_move(plan, spins, None, 1, 0, 0, KEY, 1)
    assert (want.differ == n).all()
    if cut is None:
        assert (want.sizes == n).all() and np.array_equal(want.spins, -spins)
    else:
        assert set(want.sizes.ravel().tolist()) == {cut, n - cut}  # (both parts are drawn as the root's among the three pairs)
    _same(_moved(plan, nodes, spins, None, 1, 0, 1), want, f"path200 cut={cut}")


def test_single_chains_without_a_rung_table_and_identical_twins():
    """n = 33 (a bit past a 32-bit word), R = 1, rung == NULL, 70 pairs.  Pairs 3, 40 and 69 are identical twins: k = 0, size 0, and
    their rows are bit-identical on exit."""
    (plan, nodes), P = _random_plan(33, p_edge=0.12), 70
    rng = np.random.default_rng(33)
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(2 * P, plan.n))
    same = [3, 40, 69]
    for p in same:
        spins[2 * p + 1] = spins[2 * p]
    want = co.cluster_move(plan, spins, None, 1, 0, 5, KEY, 2)
    assert not want.differ[same].any() and not want.sizes[same].any() and (np.delete(want.sizes, same) > 0).all()
    got = _moved(plan, nodes, spins, None, 1, 0, 2, 5)
    _same(got, want, "random33")
    assert all(np.array_equal(got[0][2 * p], spins[2 * p]) and np.array_equal(got[0][2 * p + 1], spins[2 * p]) for p in same)


@functools.lru_cache(maxsize=None)
def _zephyr_case(R, Q, hj_seed, lo=0.5):
    """The exchange tests' solver-like parameters on the Zephyr subgraph: normal (h, J), a geometric ladder up to beta = 20."""
    plan, nodes = _zephyr_plan()
    rng = np.random.default_rng([plan.n, R * Q, hj_seed])
    h = (0.05 * rng.normal(size=plan.n)).astype(np.float32)
    J = (5.0 * rng.normal(size=plan.n_edges)).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 0.05, (-4, 4), (-1, 1))
    return plan, nodes, h, J, hs, Js, np.geomspace(lo * 20.0, 20.0, R).astype(np.float32), 0.05


@functools.lru_cache(maxsize=None)
def _random70_case(R, Q, hj_seed):
    plan, nodes = _random_plan(70, 66)
    rng = np.random.default_rng([plan.n, R * Q, hj_seed])
    h = (0.5 * rng.normal(size=plan.n)).astype(np.float32)
    J = (2.0 * rng.normal(size=plan.n_edges)).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 0.3, (-4, 4), (-1, 1))
    return plan, nodes, h, J, hs, Js, np.geomspace(0.5 * 1.5, 1.5, R).astype(np.float32), 0.3


def test_zephyr_subgraph_sixteen_rungs_after_exchange_sweeps():
    R, Q = 16, 8
    plan, nodes, h, J, _hs, _Js, ladder, prefactor = _zephyr_case(R, Q, 0)
    s = _sampler(plan, nodes, chain_offset=1000)
    res = s.sample_tempered(torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda(), prefactor, (-4, 4), (-1, 1), ladder, num_ladders=Q,
                            num_sweeps=20)
    spins, rungs = res.state.cpu().numpy(), res.rungs.cpu().numpy()
    assert not np.array_equal(rungs, np.arange(Q * R) % R)
    want = co.cluster_move(plan, spins, rungs, R, 0, 1000, KEY, 4)
    assert (want.sizes > 0).all() and (want.sizes > 1).any()
    m = s.cluster_move(res.state, res.rungs, replicas=R, move=4)
    torch.cuda.synchronize()
    _same((res.state.cpu().numpy(), m.sizes.cpu().numpy(), m.differ.cpu().numpy()), want, "zephyr128")
    share, mean = m.moved_share.cpu().numpy(), m.mean_size.cpu().numpy()
    assert np.array_equal(share, want.sizes.sum(0) / want.differ.sum(0)) and np.array_equal(mean, want.sizes.sum(0) / (want.differ > 0).sum(0))


def test_more_jobs_than_workgroups():
    (plan, nodes), P = _random_plan(33, p_edge=0.12), MAX_GRID + 104
    rng = np.random.default_rng(34)
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(2 * P, plan.n))
    want = co.cluster_move(plan, spins, None, 1, 0, 0, KEY, 6)
    _same(_moved(plan, nodes, spins, None, 1, 0, 6), want, "tiling")


def test_a_rung_table_that_is_no_permutation():
    """Doubled, missing and out-of-range rungs: the holder is the lowest chain whose clamped rung is r; a rung without a holder in
    either twin reports 0, 0 and moves nothing; no fault."""
    (plan, nodes), R = _random_plan(70, 66), 3
    rng = np.random.default_rng(72)
    rungs = np.array([0, 0, 7,   -5, 1, 1,    2, 2, 2,   1, 0, 0,    1, 1, 1,   2147483647, -2147483648, 1], dtype=np.int32)
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(rungs.size, plan.n))
    want = co.cluster_move(plan, spins, rungs, R, 0, 3, KEY, 8)
    # pair 0: rungs (0, 0, 2) and (0, 1, 1): 0 and 2 are held in the first, 0 and 1 in the second; pair 1: 2 / 0, 1; pair 2: 1 / 0, 1, 2
    assert np.array_equal(want.differ > 0, np.array([[True, False, False], [False, False, False], [False, True, False]]))
    got = _moved(plan, nodes, spins, rungs, R, 0, 8, 3)
    _same(got, want, "bad rung table")
    untouched = [1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16]  # every chain but the four holders that moved
    assert np.array_equal(got[0][untouched], spins[untouched])


def test_the_same_move_again_restores_the_state():
    (plan, nodes), R, P = _random_plan(70, 66), 3, 5
    rng = np.random.default_rng(73)
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(2 * P * R, plan.n))
    rungs = _permuted_rungs(rng, 2 * P, R)
    s = _sampler(plan, nodes)
    state, rung = torch.from_numpy(spins).cuda(), torch.from_numpy(rungs).cuda()
    first = s.cluster_move(state, rung, replicas=R, move=12)
    assert not torch.equal(state.cpu(), torch.from_numpy(spins)) and int(first.sizes.sum()) > 0
    second = s.cluster_move(state, rung, replicas=R, move=12)
    assert torch.equal(state.cpu(), torch.from_numpy(spins))
    assert torch.equal(first.sizes, second.sizes) and torch.equal(first.differ, second.differ)


# ------------------------------------------------------------------------------------------------ the composed draw
# name: (case, replicas, ladders, seed of (h, J): picked with the definition alone, see the module's docstring)
COMPOSED = {"random70": (_random70_case, 3, 6, 0), "zephyr128": (_zephyr_case, 8, 4, 0)}
SWEEP0, SWEEPS, SWAP_EVERY, ID0 = 3, 12, 2, 5


@functools.lru_cache(maxsize=None)
def _composed_definition(name, every):
    make, R, Q, hj_seed = COMPOSED[name]
    plan, _nodes, _h, _J, hs, Js, ladder, _prefactor = make(R, Q, hj_seed)
    ids = np.arange(Q * R, dtype=np.uint32) + ID0
    return co.tempered_cluster(plan, hs, Js, ladder, ids, KEY, SWEEP0, SWEEPS, SWAP_EVERY, every)


def _equal_draws(got, want, Q, R, n, where):
    t = got.tempered
    assert np.array_equal(t.state.cpu().numpy(), want.tempered.spins), f"spins differ from the definition ({where})"
    assert np.array_equal(t.rungs.cpu().numpy(), want.tempered.rungs), f"rungs differ from the definition ({where})"
    assert np.array_equal(t.samples.cpu().numpy().reshape(Q * R, n), want.tempered.samples.astype(np.float32)), f"samples ({where})"
    assert np.array_equal(got.sizes.cpu().numpy(), want.sizes.astype(np.int64)), f"sizes ({where})"
    assert np.array_equal(got.differ.cpu().numpy(), want.differ.astype(np.int64)), f"differ ({where})"
    assert np.array_equal(got.moves, want.moves)


@pytest.mark.parametrize("every", [3, 4])
@pytest.mark.parametrize("name", list(COMPOSED))
def test_the_composed_draw_equals_the_composed_definition(name, every):
    """S = 12 from sweep 3, an exchange after every second sweep, a move in front of every third (sweeps 6, 9, 12) or fourth (4, 8,
    12) -- none in front of sweep 3 of the fresh chains.  Then the same draw in two calls of 5 + 7 sweeps: at cluster_every = 4 the
    second call begins with the move in front of sweep 8."""
    make, R, Q, hj_seed = COMPOSED[name]
    plan, nodes, h, J, _hs, _Js, ladder, prefactor = make(R, Q, hj_seed)
    want = _composed_definition(name, every)
    # no decision is left out: every coin of the definition's run is far from a tie
    assert all(margin >= 1e6 * bound for margin, bound, _accepted in want.coins), (name, every)
    assert want.moves.tolist() == {3: [2, 3, 4], 4: [1, 2, 3]}[every] and want.accepted.sum() > 0 and (want.sizes > 0).any()
    print(f"{name} every {every}: {len(want.coins)} coin decisions, smallest |u - exp(d)| {min([c[0] for c in want.coins], default=np.nan):.3e}; "
          f"accepted {want.accepted.sum(axis=0)[:-1]} of {Q * want.attempts}; clusters {want.sizes.sum(axis=(1, 2))} of {want.differ.sum(axis=(1, 2))}")
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    kw = dict(num_ladders=Q, swap_every=SWAP_EVERY, cluster_every=every)

    s = _sampler(plan, nodes, chain_offset=ID0)
    s.pt_sweep_count = SWEEP0
    one = s.sample_tempered_cluster(lin, quad, prefactor, (-4, 4), (-1, 1), ladder, num_sweeps=SWEEPS, **kw)
    torch.cuda.synchronize()
    assert s.pt_sweep_count == SWEEP0 + SWEEPS and (s.sweep_count, s.calls, s.anneal_sweep_count, s.sqa_sweep_count) == (0,) * 4 and s._state is None
    _equal_draws(one, want, Q, R, plan.n, f"{name}, one call")
    assert np.array_equal(one.tempered.accepted.cpu().numpy(), want.accepted[:, :-1].astype(np.int64))
    assert np.array_equal(one.tempered.attempts, want.attempts) and tuple(one.sizes.shape) == (3, Q // 2, R)
    # (the energies are the last exchange draw's own: the bound of the exchange tests, on that segment)
    last = want.tempered
    by_rung = (np.arange(Q * R) // R) * R + last.rungs
    unit = np.empty(Q * R)
    unit[by_rung] = 4.0 * last.N * 2.0 ** -53 * last.A
    assert (np.abs(one.tempered.energies.cpu().numpy().ravel() - last.energy_by_rung) <= unit).all()

    s = _sampler(plan, nodes, chain_offset=ID0)
    s.pt_sweep_count = SWEEP0
    a = s.sample_tempered_cluster(lin, quad, prefactor, (-4, 4), (-1, 1), ladder, num_sweeps=5, **kw)
    kept = a.tempered.state.clone()
    b = s.sample_tempered_cluster(lin, quad, prefactor, (-4, 4), (-1, 1), ladder, num_sweeps=SWEEPS - 5, start=a.tempered.state,
                                  rungs=a.tempered.rungs, **kw)
    torch.cuda.synchronize()
    assert s.pt_sweep_count == SWEEP0 + SWEEPS and torch.equal(a.tempered.state, kept)  # (the first result's tensors are its own)
    assert a.moves.tolist() + b.moves.tolist() == want.moves.tolist()
    both = smp.TemperedCluster(b.tempered, torch.cat([a.sizes, b.sizes]), torch.cat([a.differ, b.differ]), np.concatenate([a.moves, b.moves]))
    _equal_draws(both, want, Q, R, plan.n, f"{name}, two calls")
    assert np.array_equal((a.tempered.accepted + b.tempered.accepted).cpu().numpy(), want.accepted[:, :-1].astype(np.int64))
    assert np.array_equal(a.tempered.attempts + b.tempered.attempts, want.attempts)


def test_grbm_pass_through_and_the_exchange_draw_is_what_it_was():
    """GraphRestrictedBoltzmannMachine.sample_tempered_cluster is the sampler's method; and sample_tempered, before and after the
    moves ran in this process, gives the bits of the exchange draw's own definition: nothing moved."""
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    make, R, Q, hj_seed = COMPOSED["zephyr128"]
    plan, nodes, h, J, hs, Js, ladder, prefactor = make(R, Q, hj_seed)
    ids = np.arange(Q * R, dtype=np.uint32) + ID0
    plain = tempered_oracle.tempered(plan, hs, Js, ladder, ids, KEY, 0, 7, 2)
    assert all(margin >= 1e6 * bound for margin, bound, _a in plain.coins)
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()

    def exchange_draw():
        s = _sampler(plan, nodes, chain_offset=ID0)
        r = s.sample_tempered(lin, quad, prefactor, (-4, 4), (-1, 1), ladder, num_ladders=Q, num_sweeps=7, swap_every=2)
        return r.state.cpu().numpy(), r.rungs.cpu().numpy(), r.samples.cpu().numpy().reshape(Q * R, plan.n), r.accepted.cpu().numpy()

    before = exchange_draw()
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                           np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    with torch.no_grad():
        grbm._linear.copy_(lin)
        grbm._quadratic.copy_(quad)
    s = _sampler(plan, nodes, chain_offset=ID0)
    s.pt_sweep_count = SWEEP0
    got = grbm.sample_tempered_cluster(s, ladder, prefactor=prefactor, linear_range=(-4, 4), quadratic_range=(-1, 1), num_ladders=Q,
                                       num_sweeps=SWEEPS, swap_every=SWAP_EVERY, cluster_every=3)
    torch.cuda.synchronize()
    _equal_draws(got, _composed_definition("zephyr128", 3), Q, R, plan.n, "through the GRBM")
    after = exchange_draw()
    for x, y, w in zip(before, after, (plain.spins, plain.rungs, plain.samples.astype(np.float32), plain.accepted[:, :-1].astype(np.int64))):
        assert np.array_equal(x, w) and np.array_equal(y, w)
