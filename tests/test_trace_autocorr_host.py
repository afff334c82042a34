"""CPU-side checks of the autocorrelation of bit-packed traces ("DVG acf v1", ``dvg_trace_autocorr`` in include/dvg.h): the
symbol, every argument error of the C entry point (before any HIP call) and of the Python surface (before the library is
touched), and the estimators of ``sampler.Autocorrelation`` on CPU tensors against their numpy restatement
(``tests/autocorr_oracle.py``) -- to 1e-12 relative, on the edge cases by value, and on a series whose answer is known."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import autocorr_oracle as ao  # noqa: E402
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402



# ------------------------------------------------------------------------------------------------ the symbol and its checks
def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported("dvg_trace_autocorr", markers=["DVG acf v1"])


def _call(bits, lag_sum, spin_sum, *, n_chains=3, n_records=10, n=64, max_lag=4, chain_sum=None):
    L = _lib.lib()
    rc = L.dvg_trace_autocorr(bits, n_chains, n_records, n, max_lag, lag_sum, spin_sum, chain_sum, 0, None)
    return rc, L.dvg_last_error()


def test_c_argument_validation_without_gpu():
    """Every error of the header's list, with its code (DVG_E_INVALID = -1, DVG_E_UNSUPPORTED = -4) and a message that names
    the argument, on host stand-in pointers: nothing reaches HIP."""
    keep = ctypes.create_string_buffer(16)
    p = ctypes.cast(keep, ctypes.c_void_p)
    for args, word in (((None, p, p), b"bits"), ((p, None, p), b"lag_sum"), ((p, p, None), b"spin_sum")):
        rc, msg = _call(*args)
        assert rc == -1 and word in msg, (rc, msg)
    for name in ("n_chains", "n_records", "n"):
        for bad in (0, -1, -2 ** 31):
            kw = {name: bad}
            if name == "n_records":
                kw["max_lag"] = 0  # (so that the message is about n_records, whichever check comes first)
            rc, msg = _call(p, p, p, **kw)
            assert rc == -1 and re.search(rb"\b" + name.encode() + rb"\b", msg), (name, bad, rc, msg)
    for n_records, max_lag in ((10, -1), (10, -2 ** 31), (10, 10), (10, 11), (1, 1), (16384, 16384), (10, 2 ** 31 - 1)):
        rc, msg = _call(p, p, p, n_records=n_records, max_lag=max_lag)
        assert rc == -1 and b"max_lag" in msg, (n_records, max_lag, rc, msg)
    for n_records in (16385, 2 ** 31 - 1):
        rc, msg = _call(p, p, p, n_records=n_records, max_lag=4)
        assert rc == -4 and b"n_records" in msg and b"LDS" in msg, (n_records, rc, msg)
    # an index past what one launch takes: 2^31 x 2^14 x 2^26 words of bits
    rc, msg = _call(p, p, p, n_chains=2 ** 31 - 1, n_records=16384, n=2 ** 31 - 1, max_lag=4)
    assert rc == -4 and b"n_chains" in msg and b"launch" in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture
def untouched(monkeypatch):
    """The library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch, F)


def test_functional_wrapper_rejects_bad_arguments(untouched):
    good = torch.zeros((3, 10, 3), dtype=torch.int32)  # n = 77: three words
    for bad in (good.long(), good.float(), good[0], good[None], torch.zeros((3, 10, 2), dtype=torch.int32),
                torch.zeros((3, 10, 4), dtype=torch.int32), torch.zeros((0, 10, 3), dtype=torch.int32),
                torch.zeros((3, 0, 3), dtype=torch.int32), good.numpy()):
        with pytest.raises(_lib.DvgError, match="bits"):
            F.trace_autocorr(bad, 77, 4)
    for bad in (0, -5, 2.0, True, "77", None):
        with pytest.raises(ValueError, match="n must"):
            F.trace_autocorr(good, bad, 4)
    for bad in (-1, 10, 11, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="max_lag"):
            F.trace_autocorr(good, 77, bad)
    with pytest.raises(_lib.DvgError, match="GPU"):  # valid arguments on a CPU tensor: the HIP path has no CPU fallback
        F.trace_autocorr(good, 77, 9)


def test_trace_autocorrelation_rejects_bad_max_lag(untouched):
    sweeps = smp.trace_sweeps(32, 2, 3)
    t = smp.Trace(torch.zeros((3, 10, 1), dtype=torch.int32), None, None, sweeps, 12)
    assert len(sweeps) == 10 and t.thin == 3
    assert smp.Trace(torch.zeros((3, 1, 1), dtype=torch.int32), None, None, smp.trace_sweeps(5, 4, 1), 12).thin == 1
    assert smp.Trace(torch.zeros((3, 7, 1), dtype=torch.int32), None, None, smp.trace_sweeps(7, 0, 1), 12).thin == 1
    for bad in (-1, 10, 400, 2.5, 3.0, True, "3"):
        with pytest.raises(ValueError, match="max_lag"):
            t.autocorrelation(bad)
    for ok in (None, 0, 9, np.int64(4)):  # valid lags on a CPU trace get as far as the device check, not the library
        with pytest.raises(_lib.DvgError, match="GPU"):
            t.autocorrelation(ok)


def test_grbm_mixing_takes_the_local_sampler_only(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    ei = np.arange(12, dtype=np.int64)
    plan = graphs.build_plan(12, np.minimum(ei, (ei + 1) % 12), np.maximum(ei, (ei + 1) % 12))
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for other in (object(), smp.GibbsSampler(plan, [f"q{i}" for i in range(12)], beta=2.0, sweeps=5, seed=3, device="cuda")):
        with pytest.raises(TypeError):
            grbm.mixing(other, prefactor=1.0, num_reads=2)


# ------------------------------------------------------------------------------------------------ the estimators
def _from_spins(s, L, thin=1, chain_sums=True):
    """``Autocorrelation`` on CPU tensors from the numpy helper's sums of (C, M, n) spins, and those sums."""
    C, M, _n = s.shape
    lag_sum, spin_sum, chain_sum = ao.lag_sums(trace_oracle.pack(s), s.shape[2], L)
    a = smp.Autocorrelation.from_sums(torch.from_numpy(lag_sum), torch.from_numpy(spin_sum),
                                      torch.from_numpy(chain_sum) if chain_sums else None, C, M, thin)
    return a, (lag_sum, spin_sum, chain_sum)


def _close(got, want, what):
    got = got.numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.allclose(got, want, rtol=1e-12, atol=0.0, equal_nan=True), (what, np.nanmax(np.abs(got - want)))


def _sticky(rng, C, M, n, p_flip):
    flips = rng.random((C, M, n)) < p_flip
    s0 = rng.integers(0, 2, (C, 1, n))
    return (1 - 2 * ((np.cumsum(flips, 1) + s0) % 2)).astype(np.int8)


@pytest.mark.parametrize("C,M,n,L,thin", [(5, 40, 7, 12, 1), (2, 2, 3, 1, 4), (3, 9, 33, 0, 2), (4, 70, 5, 69, 1)])
def test_properties_equal_the_numpy_restatement(C, M, n, L, thin):
    rng = np.random.default_rng(C * 1000 + M)
    s = _sticky(rng, C, M, n, rng.uniform(0.05, 0.6, size=(1, 1, n)))
    a, (lag_sum, spin_sum, chain_sum) = _from_spins(s, L, thin)
    assert np.array_equal(lag_sum[0], np.full(n, C * M)) and "Autocorrelation(" in repr(a) and f"max_lag={L}" in repr(a)
    assert isinstance(a.counts, np.ndarray) and a.counts.dtype == np.int64 and np.array_equal(a.counts, ao.counts(C, M, L))
    tau, truncated = ao.tau_int(lag_sum, spin_sum, C, M)
    _close(a.mean_spin, ao.mean_spin(spin_sum, C, M), "mean_spin")
    _close(a.rho, ao.rho(lag_sum, spin_sum, C, M), "rho")
    _close(a.tau_int, tau, "tau_int")
    _close(a.tau_int_sweeps, tau * thin, "tau_int_sweeps")
    _close(a.ess, ao.ess(lag_sum, spin_sum, C, M), "ess")
    _close(a.overlap, ao.overlap(lag_sum, C, M), "overlap")
    _close(a.r_hat, ao.r_hat(chain_sum, M), "r_hat")
    assert a.truncated.dtype == torch.bool and np.array_equal(a.truncated.numpy(), truncated)
    if L == 0:
        assert not a.truncated.any() and (a.tau_int == 1).all()
    assert a.rho.dtype == torch.float64 and a.max_lag == L and a.thin == thin


def test_alternating_frozen_and_all_positive_spins():
    """Spin 0 alternates (rho[1] = -1: the window is empty, tau_int = 1 exactly), spin 1 is frozen (mu^2 = 1: NaN), spin 2
    flips once in the middle of every chain (rho > 0 at every lag up to L = 3: truncated)."""
    C, M, L = 4, 40, 3
    s = np.empty((C, M, 3), dtype=np.int8)
    s[:, :, 0] = np.where((np.arange(M)[None, :] + np.arange(C)[:, None]) % 2, -1, 1)
    s[:, :, 1] = 1
    s[:, :, 2] = np.where(np.arange(M)[None, :] < M // 2, 1, -1) * np.array([1, -1, 1, -1])[:, None]
    a, _sums = _from_spins(s, L)
    rho, tau = a.rho.numpy(), a.tau_int.numpy()
    assert a.mean_spin[0] == 0 and rho[1, 0] == -1.0 and rho[2, 0] == 1.0 and tau[0] == 1.0 and not a.truncated[0]
    assert np.isnan(rho[:, 1]).all() and np.isnan(tau[1]) and np.isnan(a.ess.numpy()[1]) and not a.truncated[1]
    assert (rho[1:, 2] > 0).all() and a.truncated[2] and np.isclose(tau[2], 1.0 + 2.0 * rho[1:, 2].sum(), rtol=1e-14, atol=0)
    assert np.array_equal(a.truncated.numpy(), [False, False, True])
    # a window that closes before max_lag is not truncated: the same spin with every lag up to M - 1
    wide, _sums = _from_spins(s, M - 1)
    assert not wide.truncated[2] and wide.tau_int[2] > a.tau_int[2]


def test_r_hat_singular_values_and_errors():
    M = 6
    chain_sum = torch.tensor([[M, M, 2], [M, -M, 0], [M, M, -2]], dtype=torch.int32)  # all frozen alike; frozen apart; regular
    lag_sum = torch.full((1, 3), 3 * M, dtype=torch.int64)
    a = smp.Autocorrelation.from_sums(lag_sum, chain_sum.sum(0).long(), chain_sum, 3, M)
    r = a.r_hat.numpy()
    assert np.isnan(r[0]) and np.isposinf(r[1]) and np.isfinite(r[2])
    _close(a.r_hat, ao.r_hat(chain_sum.numpy(), M), "r_hat")
    with pytest.raises(ValueError, match="r_hat"):
        smp.Autocorrelation.from_sums(lag_sum, chain_sum.sum(0).long(), None, 3, M).r_hat
    one = smp.Autocorrelation.from_sums(torch.full((1, 3), M, dtype=torch.int64), chain_sum[0].long(), chain_sum[:1], 1, M)
    with pytest.raises(ValueError, match="r_hat"):
        one.r_hat
    single = smp.Autocorrelation.from_sums(torch.full((1, 3), 3, dtype=torch.int64), torch.tensor([3, 1, 1]),
                                           torch.tensor([[1, 1, 1], [1, -1, 1], [1, 1, -1]], dtype=torch.int32), 3, 1)
    with pytest.raises(ValueError, match="r_hat"):
        single.r_hat


def test_from_sums_validates_dtypes_and_shapes():
    lag_sum, spin_sum = torch.zeros((4, 5), dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    chain_sum = torch.zeros((3, 5), dtype=torch.int32)
    ok = smp.Autocorrelation.from_sums(lag_sum, spin_sum, chain_sum, 3, 8, 2)
    assert (ok.chains, ok.records, ok.thin, ok.max_lag) == (3, 8, 2, 3)
    for bad in (dict(lag_sum=lag_sum.float()), dict(lag_sum=lag_sum[0]), dict(lag_sum=lag_sum.numpy()), dict(spin_sum=spin_sum.int()),
                dict(spin_sum=spin_sum[:4]), dict(chain_sum=chain_sum.long()), dict(chain_sum=chain_sum[:2]),
                dict(chain_sum=chain_sum[:, :4]), dict(chains=0), dict(chains=2.5), dict(chains=True), dict(records=0),
                dict(records=3), dict(thin=0), dict(thin=1.5)):
        kw = dict(dict(lag_sum=lag_sum, spin_sum=spin_sum, chain_sum=chain_sum, chains=3, records=8, thin=2), **bad)
        with pytest.raises(ValueError):
            smp.Autocorrelation.from_sums(**kw)


# ------------------------------------------------------------------------------------------------ a known answer
@functools.lru_cache(maxsize=None)
def _two_state_series():
    rng = np.random.default_rng(0)
    flips = rng.random((64, 4096, 48)) < 0.2
    s0 = rng.integers(0, 2, (64, 1, 48))
    return (1 - 2 * ((np.cumsum(flips, 1) + s0) % 2)).astype(np.int8)


def test_two_state_chains_have_tau_4():
    """48 independent two-state chains per "spin" that flip with probability 0.2 per record: rho(t) = 0.6^t, tau_int =
    1 + 2 * 0.6 / 0.4 = 4.  With the numpy definition this series gave tau_int in 3.93 .. 4.37 (worst 9.3 % off), no spin
    truncated at L = 64 and r_hat <= 1.001; the bounds here (20 %, 1.01) are there to catch a dropped factor 2 (2.5) or a sum
    that starts at lag 0 (6), not to measure the estimator."""
    s = _two_state_series()
    lag_sum, spin_sum, chain_sum = ao.sums_of_spins(s, 64)
    a = smp.Autocorrelation.from_sums(torch.from_numpy(lag_sum), torch.from_numpy(spin_sum), torch.from_numpy(chain_sum), 64, 4096)
    tau = a.tau_int.numpy()
    print(f"tau_int in {tau.min():.3f} .. {tau.max():.3f}; r_hat <= {float(a.r_hat.max()):.5f}; truncated {int(a.truncated.sum())}")
    assert tau.shape == (48,) and (np.abs(tau - 4.0) <= 0.2 * 4.0).all(), tau
    assert not a.truncated.any() and (a.r_hat < 1.01).all()
    _close(a.tau_int, ao.tau_int(lag_sum, spin_sum, 64, 4096)[0], "tau_int")
    assert np.allclose(a.ess.numpy(), 64 * 4096 / tau, rtol=1e-12) and np.allclose(a.rho.numpy()[1], 0.6, atol=0.02)
