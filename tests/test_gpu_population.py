"""GPU parity of population annealing ("DVG PA v1" in include/dvg.h): ``dvg_population_resample`` against the definition
in ``tests/population_oracle.py`` -- every output exactly equal, ``weight_out`` included -- and the driver
``GibbsSampler.sample_population`` replayed step by step on the CPU.

The call alone.  Populations of up to 1024 chains take one workgroup each (256 threads, four consecutive chains per thread);
larger ones separate launches over tiles of 1024 chains.  Beside the sizes of the issue's list the cases hold the smallest R
that first takes each further path of the implementation:
  1025     the first population on separate launches (two tiles, the second holding one chain) -- in the list already;
  262145   = 256 x 1024 + 1: 257 tiles, the first size at which a thread of the block-sum kernels folds a second block maximum;
  1048576  = 2^20, the largest R (1024 tiles: the scan of the block sums is full); without states.
The gather copies 16-, 4- or 1-byte units as the rows' width and the pointers allow, 2048 x 256 units per pass of its
grid-stride loop: (2, 8200) x 1024 bytes, (3, 7000) x 100 bytes and (1, 4097) x 513 bytes are the first listed sizes whose 16-,
4- and 1-byte forms go round that loop more than once.

Every output carries a guard row or element behind the last chain; ``log_weight`` and ``state_in`` are compared with their
copies afterwards.

The driver.  The spins of a step are the AIS draw's, bit for bit; its log weights are held to the bound of
``tests/test_gpu_gibbs_ais.py``, 4 N 2^-53 |dbeta| A per chain (N addends of absolute sum A, from the helper); the resampling is
checked by feeding the DEVICE's own log weights of the step to the helper, which removes every near tie: parents, the final
state and the families are then exactly equal."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_oracle  # noqa: E402
import population_oracle as po  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402
from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine  # noqa: E402
from oracle import gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
GUARD_STATE, GUARD_I32, GUARD_K = 55, -77, -9
WIDTHS = (1, 15, 16, 17, 100, 512, 513)
LISTED = [(1, 1), (1, 2), (3, 63), (1, 64), (8, 65), (3, 255), (1, 256), (2, 257), (8, 128), (1, 1024), (3, 1025), (1, 4097)]
WEIGHT_SETS = ("normal", "equal", "heavy", "minus-inf", "across-the-clamp")


def _weights(kind, P, R, rng):
    C = P * R
    if kind == "normal":
        return rng.normal(700.0, 3.0, size=C)
    if kind == "equal":
        return np.full(C, -12.5)
    if kind == "heavy":  # one chain per population, the others 1000 below
        lw = np.full(C, -1000.0)
        lw[np.arange(P) * R + rng.integers(0, R, size=P)] = 0.0
        return lw
    lw = rng.normal(0.0, 3.0, size=C)
    top = np.arange(P) * R + rng.integers(0, R, size=P)
    if kind == "minus-inf":
        lw[rng.uniform(size=C) < 0.3] = -np.inf
        lw[top] = 9.0  # (a finite maximum in every population)
        return lw
    assert kind == "across-the-clamp"  # 60 .. 100 below the maximum: across the -87 clamp and the k = 0 threshold
    lw = -rng.uniform(60.0, 100.0, size=C)
    lw[::3] = -rng.uniform(0.0, 30.0, size=lw[::3].size)  # (and some on either side of k = 0 at 32 log 2)
    lw[top] = 0.0
    return lw + 41.0


def _resample(lw, P, *, id0, seed, step, state=None, family=None, want_family=True, want_weights=True):
    """The raw entry on guarded buffers.  Returns (parents, state_out, family_out, weights) as numpy, guards checked."""
    C = lw.size
    n = 0 if state is None else state.shape[1]
    d_lw = torch.from_numpy(lw).cuda()
    d_state = torch.from_numpy(state).cuda() if state is not None else None
    d_family = torch.from_numpy(family).cuda() if family is not None else None
    parents = torch.full((C + 1,), GUARD_I32, dtype=torch.int32, device="cuda")
    family_out = torch.full((C + 1,), GUARD_I32, dtype=torch.int32, device="cuda")
    k = torch.full((C + 1,), GUARD_K, dtype=torch.int64, device="cuda")
    state_out = torch.full((C + 1, n), GUARD_STATE, dtype=torch.int8, device="cuda") if state is not None else None
    L = _lib.lib()
    ws = torch.empty((int(L.dvg_population_resample_workspace_bytes(C)) + 64,), dtype=torch.uint8, device="cuda")
    ws[-64:] = 0xA5
    _lib.check(L.dvg_population_resample(d_lw.data_ptr(), C, P, id0, seed, step, _lib.ptr(d_state), _lib.ptr(state_out), n,
                                         _lib.ptr(d_family), family_out.data_ptr() if want_family else None, parents.data_ptr(),
                                         k.data_ptr() if want_weights else None, ws.data_ptr(), ws.numel() - 64, _lib.stream_ptr()),
               "dvg_population_resample")
    torch.cuda.synchronize()
    assert (ws[-64:] == 0xA5).all(), "written past the workspace"
    assert parents[C].item() == GUARD_I32 and family_out[C].item() == GUARD_I32 and k[C].item() == GUARD_K, "written past the last chain"
    assert np.array_equal(d_lw.cpu().numpy(), lw, equal_nan=True), "log_weight changed"
    if state is not None:
        assert (state_out[C] == GUARD_STATE).all(), "a state row written past the last chain"
        assert np.array_equal(d_state.cpu().numpy(), state), "state_in changed"
    if family is not None:
        assert np.array_equal(d_family.cpu().numpy(), family), "family_in changed"
    if not want_family:
        assert (family_out == GUARD_I32).all(), "family_out = NULL, yet the buffer beside it changed"
    if not want_weights:
        assert (k == GUARD_K).all(), "weight_out = NULL, yet the buffer beside it changed"
    return (parents[:C].cpu().numpy(), state_out[:C].cpu().numpy() if state is not None else None, family_out[:C].cpu().numpy(),
            k[:C].cpu().numpy())


def _check_case(P, R, kind, n, rng, *, id0=1000, step=17, with_family=True):
    C = P * R
    lw = _weights(kind, P, R, rng)
    state = rng.integers(-128, 128, size=(C, n), dtype=np.int8) if n else None
    family = rng.integers(0, 2 ** 31 - 1, size=C, dtype=np.int32) if with_family else None
    want = po.resample(lw, P, SEED, id0, step)
    parents, state_out, family_out, k = _resample(lw, P, id0=id0, seed=SEED, step=step, state=state, family=family)
    where = f"P={P} R={R} {kind} n={n}"
    assert np.array_equal(k.astype(np.uint64), want.weights), f"weight_out differs ({where})"
    assert np.array_equal(parents, want.parents), f"{int((parents != want.parents).sum())} parents differ ({where})"
    assert np.array_equal(family_out, family[want.parents] if with_family else want.parents), f"family_out differs ({where})"
    if n:
        assert np.array_equal(state_out, state[want.parents]), f"state_out differs ({where})"
    return want


@pytest.mark.parametrize("P,R", LISTED)
def test_every_output_equals_the_definition(P, R):
    rng = np.random.default_rng(P * 10007 + R)
    for i, kind in enumerate(WEIGHT_SETS):
        n = WIDTHS[(i + R) % len(WIDTHS)]
        want = _check_case(P, R, kind, n, rng, with_family=bool(i % 2))
        if kind == "equal":
            assert np.array_equal(want.parents, np.arange(P * R))
        if kind == "heavy":
            assert (np.diff(want.parents.reshape(P, R), axis=1) == 0).all()
        if kind in ("minus-inf", "across-the-clamp") and R > 2:
            assert (want.weights == 0).any() and (want.weights[want.parents] > 0).all()


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("P,R", [(3, 63), (2, 257), (3, 1025)])
def test_every_state_width(P, R, n):
    _check_case(P, R, "normal", n, np.random.default_rng(n * 31 + R))


@pytest.mark.parametrize("P,R,n", [(2, 8200, 1024), (3, 7000, 100), (1, 4097, 513)])
def test_the_gather_goes_round_its_loop(P, R, n):
    assert P * R * (n // (16 if n % 16 == 0 else 4 if n % 4 == 0 else 1)) > 2048 * 256
    _check_case(P, R, "normal", n, np.random.default_rng(n + R))


@pytest.mark.parametrize("P,R", [(1, 262145), (1, 1 << 20)])
def test_the_largest_populations_without_states(P, R):
    rng = np.random.default_rng(R)
    for kind in ("normal", "across-the-clamp"):
        want = _check_case(P, R, kind, 0, rng, with_family=False)
        assert max(want.K) < 2 ** 53


def test_optional_outputs_may_be_null():
    rng = np.random.default_rng(3)
    for P, R in ((3, 63), (2, 1025)):
        C = P * R
        lw = _weights("normal", P, R, rng)
        state = rng.integers(-128, 128, size=(C, 17), dtype=np.int8)
        family = rng.integers(0, 1000, size=C, dtype=np.int32)
        want = po.resample(lw, P, SEED, 5, 2)
        for wf, ww, st in ((False, False, None), (True, False, None), (False, True, state), (False, False, state)):
            parents, state_out, family_out, k = _resample(lw, P, id0=5, seed=SEED, step=2, state=st, family=family, want_family=wf,
                                                          want_weights=ww)
            assert np.array_equal(parents, want.parents)
            assert st is None or np.array_equal(state_out, state[want.parents])
            assert not wf or np.array_equal(family_out, family[want.parents])
            assert not ww or np.array_equal(k.astype(np.uint64), want.weights)


def test_a_call_on_some_populations_is_that_slice_of_the_whole_call():
    rng = np.random.default_rng(8)
    for P, R in ((6, 37), (4, 1030)):
        lw = _weights("normal", P, R, rng)
        whole = _resample(lw, P, id0=2 ** 32 - 40, seed=SEED, step=2 ** 32 - 1)  # (the chain ids wrap round)
        assert np.array_equal(whole[0], po.resample(lw, P, SEED, 2 ** 32 - 40, 2 ** 32 - 1).parents)
        for a, b in ((0, P), (2, P - 1), (P - 1, P)):
            part = _resample(lw[a * R:b * R].copy(), b - a, id0=(2 ** 32 - 40 + a * R) % 2 ** 32, seed=SEED, step=2 ** 32 - 1)
            assert np.array_equal(part[0] + a * R, whole[0][a * R:b * R]) and np.array_equal(part[3], whole[3][a * R:b * R])


def test_functional_wrapper():
    rng = np.random.default_rng(12)
    P, R, n = 3, 100, 48
    lw = _weights("normal", P, R, rng)
    state = rng.integers(-1, 1, size=(P * R, n), dtype=np.int8) * 2 + 1
    want = po.resample(lw, P, SEED, 7, 9)
    d_lw, d_state = torch.from_numpy(lw).cuda(), torch.from_numpy(state).cuda()
    res = F.population_resample(d_lw, populations=P, chain_id0=7, seed=SEED, step=9, state=d_state, weights=True)
    assert np.array_equal(res.parents.cpu().numpy(), want.parents) and np.array_equal(res.family.cpu().numpy(), want.parents)
    assert np.array_equal(res.state.cpu().numpy(), state[want.parents]) and res.state.data_ptr() != d_state.data_ptr()
    assert np.array_equal(res.weights.cpu().numpy().astype(np.uint64), want.weights)
    again = F.population_resample(d_lw, populations=P, chain_id0=7, seed=SEED, step=9, family=res.family)
    assert again.state is None and again.weights is None and np.array_equal(again.family.cpu().numpy(), want.parents[want.parents])


# ------------------------------------------------------------------------------------------------ the driver
@functools.lru_cache(maxsize=None)
def _zephyr(n):
    mg, _ = graphs.get_graph_mapping(graphs.greedy_get_subgraph(n, SEED, graphs.zephyr_graph(12)))
    nodes, ei, ej = graphs.edges_of(mg)
    return graphs.build_plan(n, ei, ej), nodes


def _case(name):
    """(plan, nodes, h, J, prefactor, betas, chains, P): the 16-spin case of tests/test_gibbs_ais_host.py, or 512 spins with the
    solver's recipe."""
    if name == "zephyr16":
        plan, nodes = _zephyr(16)
        rng = np.random.default_rng(16)
        h = (0.5 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
        J = rng.uniform(-1, 1, plan.n_edges).astype(np.float32)
        return plan, nodes, h, J, 1.0, np.linspace(0.0, 1.0, 65)[1:].astype(np.float32), 1024, 8
    plan, nodes = _zephyr(512)
    rng = np.random.default_rng(512)
    h = (0.05 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    return plan, nodes, h, J, 0.05, np.linspace(0.0, 20.0, 9)[1:].astype(np.float32), 256, 2


def _sampler(plan, nodes, beta=1.0):
    s = smp.GibbsSampler(plan, nodes, beta=beta, sweeps=4, seed=SEED, persistent=True, chain_offset=11, h_range=(-4, 4),
                         j_range=(-1, 1))
    s.pa_sweep_count = 5
    return s


@pytest.mark.parametrize("name,theta", [("zephyr16", 2), ("zephyr512", 1), ("zephyr512", 3)])
def test_the_population_draw_replayed_step_by_step(name, theta):
    plan, nodes, h, J, prefactor, betas, C, P = _case(name)
    hs, Js = gibbs.scaled_fields(h, J, prefactor, (-4, 4), (-1, 1))
    s = _sampler(plan, nodes)
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    pop = s.sample_population(lin, quad, prefactor, (-4, 4), (-1, 1), betas, num_reads=C, num_populations=P, sweeps_per_beta=theta,
                              history=True)
    T = betas.size
    assert s.pa_sweep_count == 5 + T * theta and (s.ais_sweep_count, s.anneal_sweep_count, s.sweep_count, s.calls) == (0, 0, 0, 0)
    assert tuple(pop.log_weights.shape) == (T, C) and tuple(pop.parents.shape) == (T, C) and tuple(pop.ess.shape) == (T, P)
    dev_lw, dev_par = pop.log_weights.cpu().numpy(), pop.parents.cpu().numpy()
    ids = np.arange(C, dtype=np.uint32) + 11
    state, families, prev, worst = None, np.arange(C, dtype=np.int32), 0.0, 0.0
    for t in range(T):
        r = ais_oracle.ais(plan, hs, Js, np.full(theta, betas[t], dtype=np.float32), ids, s.pa_seed, 5 + t * theta, start=state,
                           beta_from=prev)
        bound = 4.0 * r.N * 2.0 ** -53 * r.A * abs(float(betas[t]) - prev)
        err = np.abs(dev_lw[t] - r.log_w)
        worst = max(worst, float((err / bound).max()))
        assert np.isfinite(dev_lw[t]).all() and (err <= bound).all(), (t, err.max(), bound.min())
        want = po.resample(dev_lw[t], P, s.pa_seed, 11, 5 + (t + 1) * theta)  # the device's own weights: no near ties
        assert np.array_equal(dev_par[t], want.parents), (t, int((dev_par[t] != want.parents).sum()))
        state, families, prev = r.spins[want.parents], families[want.parents], float(betas[t])
    print(f"{name} theta={theta}: worst log weight error / bound {worst:.3f}")
    assert np.array_equal(pop.state.cpu().numpy(), state) and np.array_equal(pop.samples.cpu().numpy(), state.astype(np.float32))
    assert np.array_equal(pop.families.cpu().numpy(), families)
    est = po.estimates(plan.n, dev_lw, families, P)
    assert np.abs(pop.log_z_populations.cpu().numpy() - est["log_z_populations"]).max() <= 1e-9
    assert abs(float(pop.log_z) - est["log_z"]) <= 1e-9 and abs(float(pop.std_err) - est["std_err"]) <= 1e-9
    assert np.array_equal(pop.survivors.cpu().numpy(), est["survivors"]) and np.allclose(pop.rho_t.cpu().numpy(), est["rho_t"], rtol=1e-12)
    assert np.allclose(pop.ess.cpu().numpy(), est["ess"], rtol=1e-9, atol=0)


def test_the_draw_composed_by_hand_is_bit_identical():
    """``sample_ais`` calls under the population draw's key and counter and ``functional.population_resample`` between them."""
    plan, nodes, h, J, prefactor, betas, C, P = _case("zephyr512")
    theta = 2
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    s = _sampler(plan, nodes)
    pop = s.sample_population(lin, quad, prefactor, (-4, 4), (-1, 1), betas, num_reads=C, num_populations=P, sweeps_per_beta=theta,
                              history=True)
    assert pop.log_weights is not None
    quiet = _sampler(plan, nodes).sample_population(lin, quad, prefactor, (-4, 4), (-1, 1), betas, num_reads=C, num_populations=P,
                                                    sweeps_per_beta=theta)
    assert quiet.log_weights is None and quiet.parents is None and torch.equal(quiet.state, pop.state)
    assert torch.equal(quiet.families, pop.families) and (quiet.log_z_populations - pop.log_z_populations).abs().max() <= 1e-9
    assert torch.allclose(quiet.ess, pop.ess, rtol=1e-12, atol=0)
    ringed = _sampler(plan, nodes)
    ringed.PA_BLOCK_BYTES = 8 * C * 3  # the estimates in blocks of 3, 3 and 2 steps over a ring of three rows
    ringed = ringed.sample_population(lin, quad, prefactor, (-4, 4), (-1, 1), betas, num_reads=C, num_populations=P, sweeps_per_beta=theta)
    assert torch.equal(ringed.state, pop.state) and torch.equal(ringed.families, pop.families)
    assert (ringed.log_z_populations - pop.log_z_populations).abs().max() <= 1e-9 and torch.allclose(ringed.ess, pop.ess, rtol=1e-12, atol=0)
    hand = _sampler(plan, nodes)
    hand.ais_seed, hand.ais_sweep_count = hand.pa_seed, 5
    state, family, prev = None, None, 0.0
    for t in range(betas.size):
        samples, lw, _e = hand.sample_ais(lin, quad, prefactor, (-4, 4), (-1, 1), np.full(theta, betas[t], dtype=np.float32),
                                          num_reads=C, start=state, beta_from=prev)
        res = F.population_resample(lw, populations=P, chain_id0=11, seed=hand.pa_seed, step=hand.ais_sweep_count,
                                    state=samples.to(torch.int8), family=family)
        assert torch.equal(lw, pop.log_weights[t]) and torch.equal(res.parents, pop.parents[t]), t
        state, family, prev = res.state, res.family, float(betas[t])
    assert torch.equal(state, pop.state) and torch.equal(family, pop.families)


def test_through_the_model():
    """``log_partition(method="population")`` on the Zephyr-16 model lies within 3 ``std_err`` of enumeration; the default
    method returns what a direct ``GibbsSampler.log_partition`` call returns, bit for bit."""
    plan, nodes, h, J, prefactor, _betas, _C, _P = _case("zephyr16")
    hs, Js = gibbs.scaled_fields(h, J, prefactor, (-4, 4), (-1, 1))
    exact = ais_oracle.exact_log_z(plan.n, hs, Js, np.asarray(plan.edge_i), np.asarray(plan.edge_j), 1.0)
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                           np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    with torch.no_grad():
        grbm._linear.copy_(torch.from_numpy(h).cuda())
        grbm._quadratic.copy_(torch.from_numpy(J).cuda())
    kw = dict(prefactor=1.0, linear_range=(-4, 4), quadratic_range=(-1, 1))
    s = _sampler(plan, nodes)
    pop = grbm.log_partition(s, method="population", num_sweeps=64, num_reads=1024, **kw)
    assert isinstance(pop, smp.Population) and tuple(pop.log_z_populations.shape) == (8,) and s.pa_sweep_count == 5 + 64
    print(f"log Z: exact {exact:.6f}, population annealing {float(pop.log_z):.6f}, std_err {float(pop.std_err):.4f}, survivors "
          f"{pop.survivors.tolist()}, worst step ess {float(pop.ess.min()):.1f}")
    assert abs(float(pop.log_z) - exact) <= 3.0 * float(pop.std_err)
    a, b = _sampler(plan, nodes), _sampler(plan, nodes)
    through = grbm.log_partition(a, num_sweeps=64, num_reads=256, **kw)
    direct = b.log_partition(grbm._linear, grbm._quadratic, 1.0, (-4, 4), (-1, 1), num_sweeps=64, num_reads=256)
    assert isinstance(through, smp.LogPartition) and torch.equal(through.log_z, direct.log_z)
    assert torch.equal(through.log_weights, direct.log_weights) and torch.equal(through.samples, direct.samples)
    assert a.ais_sweep_count == 64 and a.pa_sweep_count == 5
