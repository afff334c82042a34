"""CPU-side checks of the simulated-quantum-annealing draw ("DVG SQA v1", ``dvg_gibbs_sample_quantum`` in include/dvg.h): the
symbol and the profiler name, every argument error of the C entry point (before any HIP call, on host stand-in pointers) and of
the Python surface (before the library is touched), the LAW of the numpy definition (``tests/quantum_oracle.py``) against the
exact distribution of a triangle with four slices, ``sampler.transverse_schedule``, and ``sampler.Sliced`` on CPU tensors."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quantum_oracle as qo  # noqa: E402
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402

NAME = "dvg_gibbs_sample_quantum"


# ------------------------------------------------------------------------------------------------ the symbol and its checks
def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported(NAME, markers=["DVG SQA v1"], kernels=["gibbs_quantum_kernel"], arity={NAME: 20})
    assert "sqa" not in _lib.options() and len(_lib.options()) <= 8  # (no switch of its own)


def _call(g, lin, quad, bs, kp, slices, *, prefactor=1.0, n_chains=5, n_slices=16, n_sweeps=6, init=1):
    L = _lib.lib()
    p = lambda v: None if v is None else ctypes.c_void_p(v) if isinstance(v, int) else v  # noqa: E731
    rc = L.dvg_gibbs_sample_quantum(p(g), p(lin), p(quad), prefactor, -4.0, 4.0, -1.0, 1.0, p(bs), p(kp), p(slices), n_chains,
                                    n_slices, 0, 7, 3, n_sweeps, init, None, None)
    return rc, L.dvg_last_error()


def test_c_argument_validation_without_gpu():
    """Every error of the header's list, with its code (DVG_E_INVALID = -1, DVG_E_UNSUPPORTED = -4) and a message that names
    the argument, on host stand-in pointers: nothing reaches HIP."""
    graph, g, base, _keep = support.graph_stand_in(70)
    ptrs = [g, base, base + 1024, base + 2048, base + 3072, base + 8192]
    for k, word in enumerate((rb"\bg\b", rb"\blinear\b", rb"\bquadratic\b", rb"\bbeta_slice\b", rb"\bkappa\b", rb"\bslices\b")):
        args = list(ptrs)
        args[k] = None
        rc, msg = _call(*args)
        assert rc == -1 and re.search(word, msg) and b"null" in msg, (k, rc, msg)
    for name in ("n_chains", "n_sweeps"):
        for bad in (0, -1, -2 ** 31):
            rc, msg = _call(*ptrs, **{name: bad})
            assert rc == -1 and re.search(rb"\b" + name.encode() + rb"\b", msg), (name, bad, rc, msg)
    for bad in (0, 1, 3, 6, 12, 48, 63, 65, 128, -2, -2 ** 31, 2 ** 30):
        rc, msg = _call(*ptrs, n_slices=bad)
        assert rc == -1 and re.search(rb"\bn_slices\b", msg) and b"power of two" in msg, (bad, rc, msg)
    for bad in (float("nan"), float("inf"), -float("inf")):
        rc, msg = _call(*ptrs, prefactor=bad)
        assert rc == -1 and b"prefactor" in msg, (bad, rc, msg)
    for n in (8193, 32768, 2 ** 31 - 1):
        (ctypes.c_int32 * 2).from_buffer(graph)[:] = [n, 0]
        rc, msg = _call(*ptrs)
        assert rc == -4 and re.search(rb"\bn=", msg) and b"8192" in msg and b"LDS" in msg, (n, rc, msg)
    (ctypes.c_int32 * 2).from_buffer(graph)[:] = [70, 0]
    for n_chains, n_slices in ((2 ** 30, 2), (2 ** 25, 64), (2 ** 31 - 1, 64), (2 ** 31 - 1, 2)):
        rc, msg = _call(*ptrs, n_chains=n_chains, n_slices=n_slices)
        assert rc == -4 and b"n_chains" in msg and b"n_slices" in msg and b"2^31" in msg, (n_chains, n_slices, rc, msg)


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture
def untouched(monkeypatch):
    """The library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch, F)


def _triangle_plan():
    return graphs.build_plan(3, np.array([0, 0, 1], dtype=np.int64), np.array([1, 2, 2], dtype=np.int64))


def _sampler(plan, **kw):
    return smp.GibbsSampler(plan, list(range(plan.n)), beta=kw.pop("beta", 2.0), sweeps=kw.pop("sweeps", 5), seed=11, **kw)


def test_sample_quantum_checks_before_the_library(untouched):
    plan = _triangle_plan()
    s = _sampler(plan)
    lin, quad = torch.zeros(3), torch.zeros(3)
    ok = dict(slices=4, num_reads=2)
    call = lambda bs=(0.25, 0.25), kp=(0.3, 0.2), **kw: s.sample_quantum(lin, quad, 1.0, None, None, bs, kp, **{**ok, **kw})  # noqa: E731
    for bad in (0, 1, 3, 12, 128, 4.0, "4", None, True):
        with pytest.raises(ValueError, match="slices"):
            call(slices=bad)
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match="num_reads"):
            call(num_reads=bad)
    with pytest.raises(ValueError, match="num_reads"):
        call(num_reads=None)
    with pytest.raises(ValueError, match="2\\^31"):
        call(num_reads=2 ** 29)
    for bad in ((0.25, float("nan")), (0.25, -0.1), (float("inf"), 0.25), "ab", ()):
        with pytest.raises((ValueError, _lib.DvgError), match="beta_slice"):
            call(bs=bad)
        with pytest.raises((ValueError, _lib.DvgError), match="kappa"):
            call(kp=bad)
    with pytest.raises(_lib.DvgError, match="kappa must be"):
        call(kp=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="beta_slice has 2 sweeps, kappa 3"):
        call(kp=(0.3, 0.2, 0.1))
    good = torch.zeros((2, 4, 1), dtype=torch.int32)
    for bad in (good.long(), good.float(), good[0], torch.zeros((2, 8, 1), dtype=torch.int32), torch.zeros((2, 4, 2), dtype=torch.int32),
                torch.zeros((0, 4, 1), dtype=torch.int32), good.numpy()):
        with pytest.raises(_lib.DvgError, match=r"\bstart must"):
            call(start=bad, num_reads=None)
    with pytest.raises(_lib.DvgError, match="num_reads=3 but start has 2"):
        call(start=good, num_reads=3)
    with pytest.raises(_lib.DvgError, match="GPU"):
        call(start=good, num_reads=None)  # (start on the CPU)
    with pytest.raises(_lib.DvgError, match="GPU"):
        call()  # valid arguments, CPU parameters: the HIP path has no CPU fallback
    assert s.sqa_sweep_count == 0 and s.sqa_seed == 11 ^ 0x73716131
    s.sqa_sweep_count = 9
    s.reset()
    assert s.sqa_sweep_count == 0
    # the model's method hands on to the sampler's
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    grbm = GraphRestrictedBoltzmannMachine([0, 1, 2], [(0, 1), (0, 2), (1, 2)])
    with pytest.raises(ValueError, match="slices"):
        grbm.sample_quantum(s, (0.25,), (0.3,), slices=5, prefactor=1.0, num_reads=2)
    with pytest.raises(_lib.DvgError, match="GPU"):
        grbm.sample_quantum(s, (0.25,), (0.3,), slices=4, prefactor=1.0, num_reads=2)


def test_sample_ising_quantum_keywords_check_before_the_library(untouched):
    s = _sampler(_triangle_plan())
    h, J = {0: 0.1, 1: 0.0, 2: -0.1}, {(0, 1): 0.5}
    for kw in (dict(beta_range=(0.1, 1.0)), dict(beta_schedule=[0.1, 0.2])):
        with pytest.raises(ValueError, match="transverse_field_range"):
            s.sample_ising(h, J, num_reads=2, transverse_field_range=(3.0, 0.05), num_slices=4, **kw)
        with pytest.raises(ValueError, match="num_slices"):
            s.sample_ising(h, J, num_reads=2, num_slices=4, **kw)
    with pytest.raises(ValueError, match="both transverse_field_range and num_slices"):
        s.sample_ising(h, J, num_reads=2, transverse_field_range=(3.0, 0.05))
    with pytest.raises(ValueError, match="both transverse_field_range and num_slices"):
        s.sample_ising(h, J, num_reads=2, num_slices=4)
    for bad in (3.0, (3.0,), (3.0, 1.0, 0.5), "abc"):
        with pytest.raises(ValueError, match="transverse_field_range"):
            s.sample_ising(h, J, num_reads=2, transverse_field_range=bad, num_slices=4)
    with pytest.raises(ValueError, match="gamma_end"):
        s.sample_ising(h, J, num_reads=2, transverse_field_range=(3.0, 0.0), num_slices=4)
    with pytest.raises(ValueError, match="gamma_start"):
        s.sample_ising(h, J, num_reads=2, transverse_field_range=(float("nan"), 0.1), num_slices=4)
    with pytest.raises(ValueError, match="slices"):
        s.sample_ising(h, J, num_reads=2, transverse_field_range=(3.0, 0.05), num_slices=5)
    with pytest.raises(ValueError, match="num_sweeps"):
        s.sample_ising(h, J, num_reads=2, transverse_field_range=(3.0, 0.05), num_slices=4, num_sweeps=0)
    with pytest.raises(ValueError, match="num_reads"):
        s.sample_ising(h, J, num_reads=0, transverse_field_range=(3.0, 0.05), num_slices=4)
    with pytest.raises(ValueError, match="num_sweeps needs beta_range"):  # (as before: a fixed-beta draw has no num_sweeps)
        s.sample_ising(h, J, num_reads=2, num_sweeps=3)


# ------------------------------------------------------------------------------------------------ the law of the definition
TRIANGLE = dict(hs=np.array([0.3, -0.2, 0.1], dtype=np.float32), Js=np.array([0.5, -0.4, 0.3], dtype=np.float32), P=4,
                beta_slice=0.25, kappa=0.35, C=8192, S=40)


@pytest.fixture(scope="module")
def triangle_law():
    plan = _triangle_plan()
    assert list(zip(plan.edge_i, plan.edge_j)) == [(0, 1), (0, 2), (1, 2)]
    s, p = qo.exact_law(TRIANGLE["hs"], TRIANGLE["Js"], plan.edge_i, plan.edge_j, TRIANGLE["P"], TRIANGLE["beta_slice"], TRIANGLE["kappa"])
    assert s.shape == (4096, 4, 3)
    code = ((s[:, 0] > 0) * (1 << np.arange(3))).sum(axis=1).astype(np.int64)  # slice 0's configuration, 0 .. 7
    marginal = np.bincount(code, weights=p, minlength=8)
    corr = float((p * s[:, 0, 0] * s[:, 1, 0]).sum())
    return plan, marginal, corr


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_samples_the_exact_law_of_the_sliced_triangle(triangle_law, seed):
    """What a kernel-against-oracle comparison cannot catch -- a wrong sign, a missing factor 2: C independent chains of the
    definition, S sweeps from the INIT stream, against the enumeration of all 2^12 states.  The chains are independent, so the
    bounds are binomial (6 standard deviations) and nothing is fitted."""
    plan, marginal, corr = triangle_law
    C, S, P = TRIANGLE["C"], TRIANGLE["S"], TRIANGLE["P"]
    d = qo.draw(plan, TRIANGLE["hs"], TRIANGLE["Js"], np.full(S, TRIANGLE["beta_slice"], np.float32),
                np.full(S, TRIANGLE["kappa"], np.float32), np.arange(C), P, seed, 0)
    code = ((d.s[:, 0] > 0) * (1 << np.arange(3))).sum(axis=1)
    freq = np.bincount(code, minlength=8) / C
    bound = 6.0 * np.sqrt(marginal * (1.0 - marginal) / C)
    print("slice-0 frequencies", freq, "exact", marginal, "bounds", bound)
    assert (np.abs(freq - marginal) <= bound).all(), (freq, marginal, bound)
    got = float((d.s[:, 0, 0].astype(np.float64) * d.s[:, 1, 0]).mean())
    print("<s[0][0] s[1][0]>", got, "exact", corr, "bound", 6.0 * np.sqrt((1.0 - corr ** 2) / C))
    assert abs(got - corr) <= 6.0 * np.sqrt((1.0 - corr ** 2) / C), (got, corr)
    assert corr > 0.2 and marginal.max() - marginal.min() > 0.05  # (the case tells a missing coupling and a flat law apart)


def test_oracle_init_slice_zero_is_the_plain_start_state_and_halves_are_ordered():
    from oracle import gibbs

    ids = np.array([5, 6, 4000000000], dtype=np.uint32)
    s0 = qo.init_slices(ids, 8, 37, 99, 12)
    assert np.array_equal(s0[:, 0], gibbs.init_state(ids, 37, 99, 12))
    assert len({s0[0, k].tobytes() for k in range(8)}) == 8  # (the slices start apart)
    # a huge kappa locks equal slices; kappa = 0 makes a slice the plain conditional of its own neighbours only
    plan = _triangle_plan()
    start = np.repeat(gibbs.init_state(np.arange(6), 3, 5, 0)[:, None, :], 4, axis=1)
    d = qo.draw(plan, TRIANGLE["hs"], TRIANGLE["Js"], np.full(4, 0.25, np.float32), np.full(4, 20.0, np.float32), np.arange(6), 4, 5, 0,
                start_bits=trace_oracle.pack(start))
    assert np.array_equal(d.s, start) and qo.slice_overlap(d.s) == 1.0


# ------------------------------------------------------------------------------------------------ transverse_schedule
@pytest.mark.parametrize("kind", ["linear", "geometric"])
def test_transverse_schedule_is_the_float64_formula_rounded_once(kind):
    beta, g0, g1, S, P = 2.0, 3.0, 0.05, 12, 16
    bs, kp = smp.transverse_schedule(beta, g0, g1, S, P, kind=kind)
    assert bs.dtype == np.float32 and kp.dtype == np.float32 and bs.shape == kp.shape == (S,)
    gam = np.linspace(g0, g1, S) if kind == "linear" else np.geomspace(g0, g1, S)
    gam[0], gam[-1] = g0, g1
    assert np.array_equal(kp, (-0.5 * np.log(np.tanh(beta * gam / P))).astype(np.float32))
    assert np.array_equal(bs, np.full(S, np.float32(beta / P)))
    assert (np.diff(kp) > 0).all()  # the field falls, the coupling along imaginary time grows
    up = smp.transverse_schedule(beta, g1, g0, S, P, kind=kind)[1]
    assert (np.diff(up) < 0).all()  # kappa decreases as the field grows
    one = smp.transverse_schedule(beta, g0, g1, 1, P, kind=kind)
    assert np.array_equal(one[1], kp[-1:]) and np.array_equal(one[0], bs[-1:])
    assert smp.transverse_schedule(1.0, 1e6, 1e6, 2, 2)[1].tolist() == [0.0, 0.0]  # (tanh = 1: exactly no coupling, not -0.0)


def test_transverse_schedule_rejects_what_it_cannot_tabulate():
    with pytest.raises(ValueError, match="gamma_end"):
        smp.transverse_schedule(2.0, 3.0, 0.0, 10, 16)
    with pytest.raises(ValueError, match="gamma_start"):
        smp.transverse_schedule(2.0, -1.0, 0.5, 10, 16)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma_start"):
            smp.transverse_schedule(2.0, bad, 0.5, 10, 16)
        with pytest.raises(ValueError, match="gamma_end"):
            smp.transverse_schedule(2.0, 0.5, bad, 10, 16)
        with pytest.raises(ValueError, match="beta"):
            smp.transverse_schedule(bad, 3.0, 0.5, 10, 16)
    with pytest.raises(ValueError, match="beta"):
        smp.transverse_schedule(0.0, 3.0, 0.5, 10, 16)
    with pytest.raises(ValueError, match="gamma_end.*too small"):  # beta Gamma / P underflows: tanh = 0, kappa = inf
        smp.transverse_schedule(1e-10, 3.0, 1e-320, 10, 64)
    for bad in (0, 1, 3, 65, 16.0, None):
        with pytest.raises(ValueError, match="slices"):
            smp.transverse_schedule(2.0, 3.0, 0.5, 10, bad)
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="num_sweeps"):
            smp.transverse_schedule(2.0, 3.0, 0.5, bad, 16)
    with pytest.raises(ValueError, match="kind"):
        smp.transverse_schedule(2.0, 3.0, 0.5, 10, 16, kind="cubic")


# ------------------------------------------------------------------------------------------------ sampler.Sliced on CPU tensors
def test_sliced_best_and_slice_overlap_on_hand_made_rows():
    n, C, P = 37, 3, 4  # two words, 27 pad bits
    rng = np.random.default_rng(4)
    s = rng.choice(np.array([-1, 1], dtype=np.int8), size=(C, P, n))
    s[1] = s[1, 0]  # chain 1: every slice the same
    bits = torch.from_numpy(trace_oracle.pack(s).view(np.int32))
    sl = smp.Sliced(bits, torch.from_numpy(s[:, 0].astype(np.float32)), n)
    assert sl.slices == P and sl.n == n and "3 chains x 4 slices" in repr(sl)
    assert np.array_equal(smp.unpack_spins(sl.bits, n).numpy(), s.astype(np.float32))
    want = qo.slice_overlap(s)
    assert abs(float(sl.slice_overlap()) - want) < 1e-15 and sl.slice_overlap().dtype == torch.float64
    dirty = bits.clone()
    dirty[..., -1] |= np.int32(-1) << (n % 32)  # set pad bits are ignored
    dirty[0, 2, -1] ^= np.int32(-1) << (n % 32)
    assert float(smp.Sliced(dirty, None, n).slice_overlap()) == float(sl.slice_overlap())
    assert float(smp.Sliced(bits[1:2], None, n).slice_overlap()) == 1.0
    # best: the lowest energy of each chain, ties to the lowest slice
    e = torch.tensor([[3.0, -1.0, 2.0, -1.0], [0.5, 0.5, 0.5, 0.5], [4.0, 3.0, 2.0, 1.0]], dtype=torch.float64)
    best = sl.best(energies=e)
    assert best.dtype == torch.float32 and tuple(best.shape) == (C, n)
    assert np.array_equal(best.numpy(), np.stack([s[0, 1], s[1, 0], s[2, 3]]).astype(np.float32))
    with pytest.raises(ValueError, match="energies"):
        sl.best(energies=e[:, :3])
    # P = 2: the one neighbour pair counts from either side
    two = smp.Sliced(bits[:, :2], None, n)
    assert abs(float(two.slice_overlap()) - qo.slice_overlap(s[:, :2])) < 1e-15
