"""CPU-side checks of the energies of bit-packed rows ("DVG energy v1", ``dvg_grbm_energy_packed`` in include/dvg.h) and of the
energy mixing statistics built on them: the symbol, every argument error of the C entry point (before any HIP call) and of
the Python surface (before the library is touched), the estimators of ``sampler.EnergySeries`` on CPU tensors against their
numpy restatement (``tests/energy_oracle.py``) -- to 1e-12 relative and on known series by value -- and what the statistics
say about CPU draws of the unchanged oracle (``trace_oracle.trace``, which the GPU reproduces bit for bit): the time-averaged
energy and its variance against enumeration, and a cold ring mixing several times slower than a warm one."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_oracle as eo  # noqa: E402
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

NAME = "dvg_grbm_energy_packed"


# ------------------------------------------------------------------------------------------------ the symbol and its checks
def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported(NAME, markers=["DVG energy v1"])


_stand_in = support.graph_stand_in


def _call(g, lin, quad, bits, out, *, prefactor=1.0, rows=5, row_stride=2, groups=1, group_stride=0):
    L = _lib.lib()
    rc = L.dvg_grbm_energy_packed(g, lin, quad, prefactor, -4.0, 4.0, -1.0, 1.0, bits, rows, row_stride, groups, group_stride, out, None)
    return rc, L.dvg_last_error()


def test_c_argument_validation_without_gpu():
    """Every error of the header's list, with its code (DVG_E_INVALID = -1, DVG_E_UNSUPPORTED = -4) and a message that names
    the argument, on host stand-in pointers: nothing reaches HIP."""
    graph, g, p, _keep = _stand_in()
    for k, word in enumerate((rb"\bg\b", rb"\blinear\b", rb"\bquadratic\b", rb"\bbits\b", rb"\benergy_out\b")):
        args = [g, p, p, p, p]
        args[k] = None
        rc, msg = _call(*args)
        assert rc == -1 and re.search(word, msg) and b"null" in msg, (k, rc, msg)
    for name in ("rows", "groups"):
        for bad in (0, -1, -2 ** 40):
            rc, msg = _call(g, p, p, p, p, **{name: bad})
            assert rc == -1 and re.search(rb"\b" + name.encode() + rb"\b", msg), (name, bad, rc, msg)
    for bad in (1, 0, -1, -2 ** 40):  # n = 64: two words a row
        rc, msg = _call(g, p, p, p, p, row_stride=bad)
        assert rc == -1 and b"row_stride" in msg, (bad, rc, msg)
    for bad in (-1, -2 ** 40):
        rc, msg = _call(g, p, p, p, p, groups=3, group_stride=bad)
        assert rc == -1 and b"group_stride" in msg, (bad, rc, msg)
    for bad in (float("nan"), float("inf"), -float("inf")):
        rc, msg = _call(g, p, p, p, p, prefactor=bad)
        assert rc == -1 and b"prefactor" in msg, (bad, rc, msg)
    # a row stride is measured against W = ceil(n / 32): n = 65 needs three words
    ctypes.c_int32.from_buffer(graph).value = 65
    rc, msg = _call(g, p, p, p, p, row_stride=2)
    assert rc == -1 and b"row_stride" in msg, (rc, msg)
    ctypes.c_int32.from_buffer(graph).value = 64
    # 2^62 energies or more; one fewer would launch, so it is not tried here
    for rows, groups in ((2 ** 31, 2 ** 31), (2 ** 62, 1), (1, 2 ** 62), (2 ** 40, 2 ** 40), (2 ** 63 - 1, 2 ** 63 - 1)):
        rc, msg = _call(g, p, p, p, p, rows=rows, groups=groups)
        assert rc == -4 and b"groups" in msg and b"rows" in msg and b"2^62" in msg, (rows, groups, rc, msg)
    # n above what the LDS holds: the documented limit is 8192
    for n, row_stride in ((8193, 257), (2 ** 31 - 1, 2 ** 26)):
        ctypes.c_int32.from_buffer(graph).value = n
        rc, msg = _call(g, p, p, p, p, row_stride=row_stride)
        assert rc == -4 and re.search(rb"\bn=", msg) and b"8192" in msg and b"LDS" in msg, (n, rc, msg)


# ------------------------------------------------------------------------------------------------ the Python surface
_ring_plan = support.ring_plan


_random_plan = support.random_plan


@pytest.fixture
def untouched(monkeypatch):
    """A sampler on a 12-spin ring, with the library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch, F)
    plan = _ring_plan()
    s = smp.GibbsSampler(plan, list(range(plan.n)), beta=2.0, sweeps=5, seed=3, device="cuda")
    return s, torch.zeros(plan.n), torch.zeros(plan.n_edges)


class _Handle:  # (what the wrapper reads before the library: the plan)
    def __init__(self, plan):
        self.plan, self.ptr = plan, None


def test_functional_wrapper_rejects_bad_arguments(untouched):
    plan = _random_plan()  # n = 77: three words
    gh = _Handle(plan)
    lin, quad = torch.zeros(plan.n), torch.zeros(plan.n_edges)
    flat = torch.zeros((5, 3), dtype=torch.int32)
    trace = torch.zeros((4, 6, 3), dtype=torch.int32)
    for bad in (flat.long(), flat.float(), flat[0], flat[None, None], torch.zeros((5, 2), dtype=torch.int32),
                torch.zeros((5, 4), dtype=torch.int32), torch.zeros((0, 3), dtype=torch.int32),
                torch.zeros((4, 0, 3), dtype=torch.int32), flat.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\bbits must"):
            F.grbm_energy_packed(bad, gh, lin, quad)
    # strides: the last dimension must be dense, a row must not overlap the next
    wide = torch.zeros((5, 6), dtype=torch.int32)
    with pytest.raises(_lib.DvgError, match="bits: the last dimension"):
        F.grbm_energy_packed(wide[:, ::2], gh, lin, quad)
    with pytest.raises(_lib.DvgError, match="bits: a row stride"):
        F.grbm_energy_packed(flat[:1].expand(5, 3), gh, lin, quad)
    with pytest.raises(_lib.DvgError, match="bits: a row stride"):
        F.grbm_energy_packed(torch.zeros((30,), dtype=torch.int32).as_strided((2, 4, 3), (12, 2, 1)), gh, lin, quad)
    for bad in (lin.double(), lin[:-1], torch.zeros(plan.n + 1), lin.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\blinear must"):
            F.grbm_energy_packed(flat, gh, bad, quad)
    for bad in (quad.double(), quad[:-1], quad.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\bquadratic must"):
            F.grbm_energy_packed(flat, gh, lin, bad)
    for bad in (float("nan"), float("inf"), -float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="prefactor"):
            F.grbm_energy_packed(flat, gh, lin, quad, prefactor=bad)
    for bad in ((1.0,), (1.0, 2.0, 3.0), 4.0, "ab", (float("nan"), 1.0), (None, 1.0), (True, 2.0)):
        with pytest.raises(ValueError, match="linear_range"):
            F.grbm_energy_packed(flat, gh, lin, quad, linear_range=bad)
        with pytest.raises(ValueError, match="quadratic_range"):
            F.grbm_energy_packed(flat, gh, lin, quad, quadratic_range=bad)
    for ok in (flat, flat[::2], flat[:1], trace, trace[:, 1:], trace[::2], trace[:, ::3], trace[:1].expand(3, 6, 3)):
        with pytest.raises(_lib.DvgError, match="GPU"):  # valid arguments on CPU tensors: the HIP path has no CPU fallback
            F.grbm_energy_packed(ok, gh, lin, quad, prefactor=0.3, linear_range=(-4, 4), quadratic_range=(-1.0, float("inf")))


def test_trace_energy_reaches_the_device_check_only(untouched):
    _s, lin, quad = untouched
    gh = _Handle(_ring_plan())
    t = smp.Trace(torch.zeros((3, 10, 1), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    with pytest.raises(_lib.DvgError, match="GPU"):
        t.energy(gh, lin, quad)
    with pytest.raises(_lib.DvgError, match="GPU"):
        t.energy(gh, lin, quad, 0.5, (-4, 4), (-1, 1))
    with pytest.raises(_lib.DvgError, match="GPU"):
        t.energy_series(gh, lin, quad, max_lag=9)
    with pytest.raises(_lib.DvgError, match=r"\blinear must"):
        t.energy(gh, lin[:-1], quad)
    with pytest.raises(ValueError, match="prefactor"):
        t.energy(gh, lin, quad, prefactor=float("nan"))
    with pytest.raises(ValueError, match="quadratic_range"):
        t.energy(gh, lin, quad, quadratic_range=(1.0,))
    for bad in (10, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="max_lag"):
            t.energy_series(gh, lin, quad, max_lag=bad)
    wrong = smp.Trace(torch.zeros((3, 10, 2), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    with pytest.raises(_lib.DvgError, match=r"\bbits must"):
        wrong.energy(gh, lin, quad)


def test_grbm_energy_methods_check_before_the_library(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    s, _lin, _quad = untouched
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for other in (object(), smp.GibbsSampler(s.plan, [f"q{i}" for i in range(12)], beta=2.0, sweeps=5, seed=3, device="cuda")):
        with pytest.raises(TypeError):
            grbm.energy_mixing(other, prefactor=1.0, num_reads=2)
    for bad in (-1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="max_lag"):
            grbm.energy_mixing(s, prefactor=1.0, num_reads=2, max_lag=bad)
    # mixing's checks: the traced draw's own
    with pytest.raises(ValueError, match="num_reads"):
        grbm.energy_mixing(s, prefactor=1.0)
    with pytest.raises(ValueError, match="record nothing"):
        grbm.energy_mixing(s, prefactor=1.0, num_reads=2, burn_in=5)
    with pytest.raises(ValueError, match="thin"):
        grbm.energy_mixing(s, prefactor=1.0, num_reads=2, thin=0)
    with pytest.raises(_lib.DvgError):  # valid arguments, CPU parameters: the HIP path has no CPU fallback
        grbm.energy_mixing(s, prefactor=1.0, num_reads=2)
    assert (s.trace_sweep_count, s.sweep_count, s.calls) == (0, 0, 0)
    for bad in (torch.zeros((4, 1), dtype=torch.int32), np.zeros((4, 1), dtype=np.int32), None):
        with pytest.raises(_lib.DvgError, match="GPU"):
            grbm.energy_packed(bad, prefactor=1.0)


def test_from_energies_validates():
    e = torch.zeros((3, 7), dtype=torch.float64)
    s = smp.EnergySeries.from_energies(e)
    assert (s.chains, s.records, s.thin, s.max_lag) == (3, 7, 1, 6) and "EnergySeries(" in repr(s)
    assert smp.EnergySeries.from_energies(torch.zeros((2, 1000), dtype=torch.float64)).max_lag == 512
    assert smp.EnergySeries.from_energies(e, thin=np.int64(4), max_lag=np.int64(0)).thin == 4
    for bad in (e.float(), e[0], e[None], e.numpy(), torch.zeros((0, 7), dtype=torch.float64), torch.zeros((3, 0), dtype=torch.float64), None):
        with pytest.raises(ValueError, match="energies"):
            smp.EnergySeries.from_energies(bad)
    for bad in (0, -1, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="thin"):
            smp.EnergySeries.from_energies(e, thin=bad)
    for bad in (7, 8, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="max_lag"):
            smp.EnergySeries.from_energies(e, max_lag=bad)


# ------------------------------------------------------------------------------------------------ the estimators
def _close(got, want, what):
    got = got.numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    if want.dtype == np.bool_:
        assert got.dtype == np.bool_ and got.shape == want.shape and np.array_equal(got, want), (what, got, want)
        return
    assert got.shape == want.shape and got.dtype == np.float64 and want.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    assert np.allclose(got, want, rtol=1e-12, atol=0.0, equal_nan=True), (what, got, want)


def _check_all(E, thin=1, max_lag=None, beta=1.7):
    s = smp.EnergySeries.from_energies(torch.from_numpy(E), thin=thin, max_lag=max_lag)
    want = eo.estimates(E, thin=thin, max_lag=max_lag, beta=beta)
    for name, value in want.items():
        _close(s.heat_capacity(beta) if name == "heat_capacity" else getattr(s, name), value, name)
    C, M = E.shape
    if C < 2 or M < 2:
        assert "r_hat" not in want
        with pytest.raises(ValueError, match="r_hat"):
            s.r_hat
    assert s.rho.shape == (s.max_lag + 1,) and s.chain_mean.shape == (C,) and s.mean.dim() == 0 and not s.rho.is_cuda
    return s


@pytest.mark.parametrize("C,M", [(1, 1), (1, 5), (2, 2), (7, 33)])
def test_properties_equal_the_numpy_restatement(C, M):
    rng = np.random.default_rng(100 * C + M)
    E = -40.0 + 3.0 * rng.standard_normal((C, M))
    s = _check_all(E)
    assert s.max_lag == M - 1
    if M > 1:
        assert float(s.rho[0]) == pytest.approx(1.0, abs=1e-15)
        _check_all(E, thin=3, max_lag=0)
        _check_all(E, thin=2, max_lag=(M - 1) // 2)
    if C == 1:
        assert np.isnan(float(s.std_err))
    if M == 1 and C == 1:  # one energy: no variance
        assert np.isnan(s.rho.numpy()).all() and np.isnan(float(s.tau_int)) and not bool(s.truncated)


def test_known_series():
    # constant: var = 0, rho and tau_int NaN
    s = _check_all(np.full((3, 8), -2.5))
    assert float(s.var) == 0.0 and float(s.mean) == -2.5 and np.isnan(s.rho.numpy()).all() and np.isnan(float(s.tau_int))
    assert np.isnan(float(s.ess)) and not bool(s.truncated) and float(s.std_err) == 0.0 and float(s.heat_capacity(2.0)) == 0.0
    # alternating +-1 over an even number of records: mean 0, var 1, rho[t] = (-1)^t, nothing in the initial positive sequence
    E = np.tile(np.array([1.0, -1.0] * 6), (4, 1))
    s = _check_all(E, thin=5)
    assert float(s.mean) == 0.0 and float(s.var) == 1.0 and float(s.rho[1]) == -1.0 and float(s.rho[2]) == 1.0
    assert float(s.tau_int) == 1.0 and float(s.tau_int_sweeps) == 5.0 and float(s.ess) == 48.0 and not bool(s.truncated)
    assert float(s.heat_capacity(3.0)) == 9.0
    # a slow ramp: rho > 0 at every lag of a short window -- truncated, tau_int a lower bound
    E = np.tile(np.arange(40, dtype=np.float64), (2, 1)) + np.array([[0.0], [0.5]])
    s = _check_all(E, max_lag=4)
    assert bool(s.truncated) and (s.rho.numpy() > 0).all() and float(s.tau_int) > 1.0 + 2.0 * 4 * 0.5
    assert not bool(_check_all(E, max_lag=0).truncated) and float(_check_all(E, max_lag=0).tau_int) == 1.0
    # chains in different basins: r_hat far above 1
    E = np.stack([np.array([0.0, 1.0] * 10), 100.0 + np.array([0.0, 1.0] * 10)])
    assert float(_check_all(E).r_hat) > 10.0


# ------------------------------------------------------------------------------------------------ the statistics mean what they claim
RING_SEED = 20261019


@functools.lru_cache(maxsize=None)
def _ring_series(beta):
    """The 12-spin ring of ``test_gibbs_trace_host.py``: 64 chains, 250 sweeps, burn_in 50, thin 2 -> 100 records a chain; their
    energies by the helper, and the exact mean and variance by enumeration."""
    plan = _ring_plan()
    rng = np.random.default_rng(12)
    h = (0.5 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = rng.uniform(-1, 1, plan.n_edges).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 1.0, (-4, 4), (-1, 1))
    ids = np.arange(64, dtype=np.uint32) + 11
    tr = trace_oracle.trace(plan, hs, Js, beta, ids, RING_SEED ^ 0x74726163, 0, 250, burn_in=50, thin=2)
    assert tr.bits.shape == (64, 100, 1)
    E, _A = eo.energies(tr.bits, plan.n, hs, Js, plan.edge_i, plan.edge_j)
    series = smp.EnergySeries.from_energies(torch.from_numpy(E), thin=2, max_lag=16)
    return series, eo.exact_energy_moments(plan.n, hs, Js, plan.edge_i, plan.edge_j, beta)


def test_energy_statistics_of_a_warm_and_a_cold_ring():
    """At beta = 0.8 the chains mix within a record or two: the time-averaged energy lies within 6 standard errors of
    enumeration over the 2^12 states, its variance (the heat capacity over beta^2) within 10 %, R-hat below 1.01.  At beta = 3
    the same chains still estimate the mean, and their energy decorrelates at least four times more slowly."""
    warm, (mean_w, var_w) = _ring_series(0.8)
    cold, (mean_c, _var_c) = _ring_series(3.0)
    for name, s, exact in (("beta 0.8", warm, mean_w), ("beta 3.0", cold, mean_c)):
        z = (float(s.mean) - exact) / float(s.std_err)
        print(f"{name}: mean {float(s.mean):.4f} against {exact:.4f} exact, {z:+.2f} std_err of {float(s.std_err):.4f}; var "
              f"{float(s.var):.3f}; tau_int {float(s.tau_int):.2f} records (truncated: {bool(s.truncated)}); r_hat {float(s.r_hat):.4f}")
        assert float(s.std_err) > 0 and abs(z) <= 6.0
    print(f"beta 0.8: var {float(warm.var):.3f} against {var_w:.3f} exact")
    assert abs(float(warm.var) / var_w - 1.0) <= 0.1
    assert float(warm.heat_capacity(0.8)) == pytest.approx(0.64 * float(warm.var), rel=1e-15)
    assert float(cold.tau_int) >= 4.0 * float(warm.tau_int)
    assert float(warm.r_hat) < 1.01
    assert float(warm.tau_int_sweeps) == 2.0 * float(warm.tau_int) and float(warm.ess) == pytest.approx(6400.0 / float(warm.tau_int), rel=1e-15)
