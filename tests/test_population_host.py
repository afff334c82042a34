"""CPU-side checks of population annealing ("DVG PA v1", ``dvg_population_resample`` in include/dvg.h): the symbols, every
argument error of the C entry point (before any HIP call) and of the Python surface (before the library is touched), the
draw's own key and counter, the properties of the definition as ``tests/population_oracle.py`` restates it -- in exact
integer arithmetic -- the population estimate of log Z against enumeration, and ``sampler.Population.from_history`` on CPU
tensors against the oracle's numpy."""
import ctypes
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_oracle  # noqa: E402
import population_oracle as po  # noqa: E402
from test_gibbs_ais_host import zephyr16_case  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, sampler as smp  # noqa: E402
from oracle import cref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 775321899904
NAMES = ("dvg_population_resample", "dvg_population_resample_workspace_bytes")


# ------------------------------------------------------------------------------------------------ the symbols and their checks
def test_symbols_are_declared_bound_and_exported():
    support.assert_declared_bound_exported(dict(zip(NAMES, ("int", "size_t"))), markers=["DVG PA v1", "STREAM_RESAMPLE = 5"])
    assert "STREAM_RESAMPLE = 5" in open(os.path.join(ROOT, "image-generation_amd", "csrc", "philox.h")).read()


def _call(lw, parent, ws, *, n_chains=12, P=3, state_in=None, state_out=None, n=5, family_in=None, family_out=None,
          weight_out=None, ws_bytes=1 << 40):
    L = _lib.lib()
    rc = L.dvg_population_resample(lw, n_chains, P, 0, SEED, 0, state_in, state_out, n, family_in, family_out, parent, weight_out,
                                   ws, ws_bytes, None)
    return rc, L.dvg_last_error()


def test_c_argument_validation_without_gpu():
    """Every error of the header's list, with its code (DVG_E_INVALID = -1, DVG_E_WORKSPACE = -3, DVG_E_UNSUPPORTED = -4)
    and a message that names the argument, on host stand-in pointers: nothing reaches HIP."""
    keep = [ctypes.create_string_buffer(16) for _ in range(2)]
    p, q = (ctypes.cast(k, ctypes.c_void_p) for k in keep)
    for args, word in (((None, p, p), b"log_weight"), ((p, None, p), b"parent_out"), ((p, p, None), rb"\bws\b")):
        rc, msg = _call(*args)
        assert rc == -1 and re.search(word, msg), (rc, msg)
    for bad in (0, -1, -2 ** 31):
        rc, msg = _call(p, p, p, n_chains=bad)
        assert rc == -1 and b"n_chains" in msg, (bad, rc, msg)
        rc, msg = _call(p, p, p, P=bad)
        assert rc == -1 and b"n_populations" in msg, (bad, rc, msg)
    for C, P in ((12, 5), (12, 24), (7, 2)):
        rc, msg = _call(p, p, p, n_chains=C, P=P)
        assert rc == -1 and b"multiple" in msg and b"n_populations" in msg, (C, P, rc, msg)
    rc, msg = _call(p, p, p, state_in=p)
    assert rc == -1 and b"state_out is null" in msg, (rc, msg)
    rc, msg = _call(p, p, p, state_out=p)
    assert rc == -1 and b"state_in is null" in msg, (rc, msg)
    for bad in (0, -1):
        rc, msg = _call(p, p, p, state_in=p, state_out=q, n=bad)
        assert rc == -1 and re.search(rb"\bn=", msg), (bad, rc, msg)
    rc, msg = _call(p, p, p, state_in=p, state_out=p)
    assert rc == -1 and b"state_in == state_out" in msg, (rc, msg)
    rc, msg = _call(p, p, p, family_in=p, family_out=p)
    assert rc == -1 and b"family_in == family_out" in msg, (rc, msg)
    # the workspace: below the query is refused, and the query grows with the chains
    query = _lib.lib().dvg_population_resample_workspace_bytes
    assert query(0) == 0 and query(-3) == 0 and 8 * 12 <= query(12) and 8 * (1 << 20) <= query(1 << 20) <= 9 * (1 << 20)
    for C in (12, 1 << 20):
        rc, msg = _call(p, p, p, n_chains=C, P=1, ws_bytes=query(C) - 1)
        assert rc == -3 and b"workspace" in msg, (C, rc, msg)
    # R = n_chains / n_populations above 2^20
    for C, P in (((1 << 20) + 1, 1), (3 * ((1 << 20) + 1), 3), (2 ** 31 - 1, 1)):
        rc, msg = _call(p, p, p, n_chains=C, P=P)
        assert rc == -4 and re.search(rb"\bR\b", msg) and str(C // P).encode() in msg and str(1 << 20).encode() in msg, (C, P, rc, msg)


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture
def untouched(monkeypatch):
    """A sampler on a 12-spin ring, with the library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch, F)
    plan = support.ring_plan()
    n = plan.n
    s = smp.GibbsSampler(plan, list(range(n)), beta=2.0, sweeps=5, seed=3, device="cuda")
    return s, torch.zeros(n), torch.zeros(plan.n_edges)


def test_functional_wrapper_rejects_bad_arguments(untouched):
    lw = torch.zeros(12, dtype=torch.float64)
    ok = dict(seed=1, step=0)
    for bad in (lw.float(), lw.view(3, 4), lw[:0], lw.numpy(), None, lw.long()):
        with pytest.raises(_lib.DvgError, match="log_weight must"):
            F.population_resample(bad, **ok)
    for name, values in (("populations", (0, -1, 2.0, True, None, 2 ** 31)), ("chain_id0", (-1, 2 ** 32, 1.0, None)),
                         ("seed", (-1, 2 ** 64, 1.5, None)), ("step", (-1, 2 ** 32, "0", None))):
        for bad in values:
            with pytest.raises(ValueError, match=name + " must"):
                F.population_resample(lw, **{**ok, name: bad})
    for bad in (5, 24):
        with pytest.raises(ValueError, match="does not divide"):
            F.population_resample(lw, populations=bad, **ok)
    with pytest.raises(ValueError, match="2\\^20"):
        F.population_resample(torch.zeros((1 << 20) + 1, dtype=torch.float64), **ok)
    state = torch.ones((12, 5), dtype=torch.int8)
    for bad in (state.float(), state[:11], state[0], state[:, :0], state.numpy()):
        with pytest.raises(_lib.DvgError, match="state must"):
            F.population_resample(lw, state=bad, **ok)
    family = torch.arange(12, dtype=torch.int32)
    for bad in (family.long(), family[:11], family.view(3, 4), family.numpy()):
        with pytest.raises(_lib.DvgError, match="family must"):
            F.population_resample(lw, family=bad, **ok)
    for kw in ({}, dict(state=state), dict(family=family), dict(populations=3, state=state, family=family, weights=True)):
        with pytest.raises(_lib.DvgError, match="GPU"):  # valid arguments on CPU tensors: the HIP path has no CPU fallback
            F.population_resample(lw, **kw, **ok)


def test_sample_population_rejects_bad_arguments(untouched):
    s, lin, quad = untouched
    call = lambda betas=(0.5, 1.0), **kw: s.sample_population(lin, quad, 1.0, None, None, betas, **{"num_reads": 8, **kw})  # noqa: E731
    for bad in ([0.1, -0.5], [0.1, float("nan")], [float("inf")], np.array([1e39]), torch.tensor([0.5, -1.0]), ["a"]):
        with pytest.raises(ValueError):
            call(bad)
    for bad in ([], np.ones((2, 2)), 3.0, np.ones((8, 3))):
        with pytest.raises(_lib.DvgError, match="betas must"):
            call(bad)
    for name in ("num_reads", "num_populations", "sweeps_per_beta"):
        for bad in (0, -1, 2.5, True, None, "4"):
            with pytest.raises(ValueError, match=name + " must"):
                call(**{name: bad})
    with pytest.raises(ValueError, match="does not divide"):
        call(num_populations=3)
    with pytest.raises(ValueError, match="2\\^20"):
        call(num_reads=(1 << 21) + 2, num_populations=2)
    with pytest.raises(TypeError):
        call(start=torch.ones((8, 12), dtype=torch.int8))  # fresh chains only
    with pytest.raises(_lib.DvgError, match="GPU"):  # valid arguments, CPU parameters: the HIP path has no CPU fallback
        call(num_populations=2, sweeps_per_beta=3, history=True)
    assert (s.pa_sweep_count, s.ais_sweep_count, s.anneal_sweep_count, s.sweep_count, s.calls) == (0, 0, 0, 0, 0)


def test_population_draws_have_their_own_key_and_counter(untouched):
    s, _lin, _quad = untouched
    others = (s.seed, s.cond_seed, s.anneal_seed, s.ais_seed, s.pt_seed, s.trace_seed)
    assert s.pa_seed == 3 ^ 0x70613031 and s.pa_seed not in others and len(set(others)) == 6 and s.pa_sweep_count == 0
    s.pa_sweep_count, s.ais_sweep_count, s.sweep_count = 5, 6, 7
    s.reset()
    assert (s.pa_sweep_count, s.ais_sweep_count, s.sweep_count) == (0, 0, 0)


def test_grbm_population_surface_takes_the_local_sampler_only_and_checks_the_method(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    s, _lin, _quad = untouched
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    with pytest.raises(TypeError):
        grbm.sample_population(object(), [0.5, 1.0], prefactor=1.0, num_reads=8)
    with pytest.raises(TypeError):
        grbm.log_partition(object(), prefactor=1.0, method="population")
    for bad in ("smc", None, 3):
        with pytest.raises(ValueError, match="method"):
            grbm.log_partition(s, prefactor=1.0, method=bad)
    for kw in (dict(num_sweeps=0), dict(num_sweeps=2.5), dict(beta=0.0), dict(beta=float("nan")), dict(num_populations=3),
               dict(num_reads=0)):
        with pytest.raises(ValueError):
            grbm.log_partition(s, prefactor=1.0, method="population", **kw)
    assert s.pa_sweep_count == 0


# ------------------------------------------------------------------------------------------------ the definition's properties
def _normal(R, seed=0):
    return np.random.default_rng(1000 + R + seed).normal(0.0, 3.0, size=R)


def test_oracle_exp_is_the_c_restatement():
    """``population_oracle.weights`` takes the array form of the bit-specified exp: held against ``cref.spec_exp``."""
    lw = np.concatenate([_normal(1000), [-np.inf, -95.0, -87.0, -86.99, -22.2, -22.1, 0.0, 9.5]])
    k = po.weights(lw)
    m = lw.max()
    for v, got in zip(lw, k):
        z = np.float32(min(max(np.float32(v - m), np.float32(-87.0)), np.float32(0.0)))
        assert int(got) == int(np.float64(cref.spec_exp(z)) * 4294967296.0), (v, got)
    assert int(k.max()) == 2 ** 32 and int(k[1000]) == 0 and k.dtype == np.uint64


@pytest.mark.parametrize("R", [1, 2, 7, 128, 1000])
def test_children_are_floor_or_ceil_and_parents_do_not_decrease(R):
    for step in range(3):
        lw = _normal(R, step)
        par, k, K, V = po.resample_one(lw, SEED, 40 + R, step)
        assert 0 <= V < K and 2 ** 32 <= K <= R * 2 ** 32 and K == sum(int(v) for v in k) and int(max(k)) == 2 ** 32
        assert (np.diff(par) >= 0).all() and par.min() >= 0 and par.max() < R
        children = np.bincount(par, minlength=R)
        S = np.cumsum([int(v) for v in k], dtype=object)
        for c in range(R):
            share = Fraction(R * int(k[c]), K)  # exact
            assert children[c] in (math.floor(share), math.ceil(share)), (c, children[c], share)
        for j in range(R):  # the definition, child by child, in Python integers
            t = (j * K + V) // R
            assert S[par[j]] > t and (par[j] == 0 or S[par[j] - 1] <= t), (j, par[j])


def test_chains_of_weight_zero_are_never_chosen():
    rng = np.random.default_rng(5)
    for R in (7, 128, 1000):
        lw = _normal(R)
        dead = rng.permutation(R)[:max(2, R // 3)]
        keep = np.setdiff1d(np.arange(R), dead)
        lw[dead[::2]] = -np.inf
        lw[dead[1::2]] = lw[keep].max() - rng.uniform(90.0, 200.0, size=dead[1::2].size)  # more than 90 below the maximum
        for step in range(4):
            par, k, _K, _V = po.resample_one(lw, SEED, 3, step)
            assert (k[dead] == 0).all() and not np.isin(par, dead).any()
            assert not np.isin(par, np.flatnonzero(k == 0)).any()


def test_equal_weights_give_the_identity_and_one_heavy_chain_takes_all():
    for R in (1, 2, 7, 128, 1000):
        for value in (0.0, 700.0, -3.25e5):
            for step in range(3):
                par, k, K, _V = po.resample_one(np.full(R, value), SEED, 9, step)
                assert np.array_equal(par, np.arange(R)) and K == R * 2 ** 32 and (k == 2 ** 32).all()
        for at in sorted({0, R // 2, R - 1}):
            lw = np.full(R, -1000.0)
            lw[at] = 0.0
            for step in range(3):
                par, _k, K, _V = po.resample_one(lw, SEED, 9, step)
                assert (par == at).all() and K == 2 ** 32


def test_a_call_on_some_populations_is_that_slice_of_the_whole_call():
    P, R = 6, 37
    lw = _normal(P * R)
    whole = po.resample(lw, P, SEED, 100, 17)
    for a, b in ((0, 6), (2, 5), (5, 6), (0, 1)):
        part = po.resample(lw[a * R:b * R], b - a, SEED, 100 + a * R, 17)
        assert np.array_equal(part.parents + a * R, whole.parents[a * R:b * R])
        assert np.array_equal(part.weights, whole.weights[a * R:b * R]) and part.V == whole.V[a:b]
    other = po.resample(lw[2 * R:5 * R], 3, SEED, 100, 17)  # (chain_id0 not advanced: other offsets)
    assert other.V != whole.V[2:5]


def test_the_number_of_children_is_unbiased_over_the_steps():
    """R = 8, the 4096 offsets of step = 0 .. 4095: a chain has floor(x) or floor(x) + 1 children, x = R k_c / K, the
    latter with probability f = frac(x); its mean over the steps lies within 5 standard errors sqrt(f (1 - f) / 4096) of x."""
    R, N = 8, 4096
    lw = _normal(R)
    k = [int(v) for v in po.weights(lw)]
    K = sum(k)
    counts = np.zeros(R)
    for step in range(N):
        counts += np.bincount(po.resample_one(lw, SEED, 21, step)[0], minlength=R)
    for c in range(R):
        x = R * k[c] / K
        f = x - np.floor(x)
        assert abs(counts[c] / N - x) <= 5.0 * np.sqrt(f * (1.0 - f) / N), (c, counts[c] / N, x)


# ------------------------------------------------------------------------------------------------ against enumeration
@pytest.mark.parametrize("beta", [1.0, 2.0])
def test_the_population_estimate_against_enumeration(beta):
    """The 16-spin Zephyr case of the AIS tests, 1024 chains in 8 populations, 64 betas at 2 sweeps each: the estimate lies
    within 3 standard errors of the sum over all 2^16 states."""
    plan, _nodes, _h, _J, hs, Js, betas, ids, key, sweep0 = zephyr16_case(beta)
    exact = ais_oracle.exact_log_z(plan.n, hs, Js, np.asarray(plan.edge_i), np.asarray(plan.edge_j), float(betas[-1]))
    r = po.anneal(plan, hs, Js, betas, ids, key, sweep0, 2, 8)
    est = po.estimates(plan.n, r.log_weights, r.families, 8)
    assert np.allclose(est["log_z_populations"], r.log_z_populations, rtol=0, atol=1e-9) and np.array_equal(est["ess"], r.ess)
    print(f"beta {beta}: exact {exact:.6f}, estimate {est['log_z']:.6f}, off by {abs(est['log_z'] - exact):.4f}, std_err "
          f"{est['std_err']:.4f}, survivors {est['survivors'].min()} .. {est['survivors'].max()} of 128, worst step ess {r.ess.min():.1f}")
    assert abs(est["log_z"] - exact) <= 3.0 * est["std_err"]
    assert r.state.shape == (1024, 16) and set(np.unique(r.state)) <= {-1, 1}
    assert (r.families.reshape(8, 128) // 128 == np.arange(8)[:, None]).all()  # a family stays in its population


# ------------------------------------------------------------------------------------------------ the estimates
@pytest.mark.parametrize("P,R,T", [(1, 9, 3), (4, 33, 5), (8, 128, 2)])
def test_population_estimates_match_the_oracle(P, R, T):
    rng = np.random.default_rng(P + R + T)
    lw = rng.normal(-40.0, 3.0, size=(T, P * R))
    families = (np.arange(P)[:, None] * R + rng.integers(0, max(1, R // 3), size=(P, R))).reshape(-1).astype(np.int32)
    want = po.estimates(23, lw, families, P)
    got = smp.Population.from_history(23, torch.from_numpy(lw), torch.from_numpy(families), populations=P)
    for name in ("log_z_populations", "log_z", "survivors", "rho_t", "ess"):
        a, b = np.asarray(getattr(got, name), dtype=np.float64), np.asarray(want[name], dtype=np.float64)
        assert a.shape == b.shape and np.all(np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b))), (name, a, b)
    if P == 1:
        assert np.isnan(float(got.std_err)) and np.isnan(want["std_err"])
    else:
        assert abs(float(got.std_err) - want["std_err"]) <= 1e-12
    assert got.log_z_populations.dtype == torch.float64 and got.survivors.dtype == torch.int64 and tuple(got.ess.shape) == (T, P)
    assert got.log_weights is not None and got.parents is None and got.samples is None
    for bad in (dict(populations=0), dict(populations=P + 1 if (P * R) % (P + 1) else 2 * P * R)):
        with pytest.raises(ValueError):
            smp.Population.from_history(23, torch.from_numpy(lw), torch.from_numpy(families), **bad)
    with pytest.raises(ValueError):
        smp.Population.from_history(23, torch.from_numpy(lw[0]), torch.from_numpy(families), populations=P)
