"""CPU-side checks of the overlap statistics of bit-packed rows ("DVG overlap v1", ``dvg_packed_overlap`` in include/dvg.h):
the symbol, every argument error of the C entry point (before any HIP call) and of the Python surface (before the library is
touched), the estimators of ``sampler.Overlap`` on CPU tensors against their numpy restatement (``tests/overlap_oracle.py``)
-- to 1e-12 relative and on known cases by value -- and what the measure says about CPU draws of the unchanged oracle
(``trace_oracle.trace``, which the GPU reproduces bit for bit): hot chains overlap like fair coins, cold ferromagnetic
chains sit in one mode or its mirror."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_oracle as oo  # noqa: E402
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402

SEED = 775321899904


# ------------------------------------------------------------------------------------------------ the symbol and its checks
def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported("dvg_packed_overlap", markers=["DVG overlap v1"])


def _call(a, b, hist, *, rows_a=5, a_rs=2, a_gs=0, rows_b=7, b_rs=2, b_gs=0, groups=1, n=64, nearest=None):
    L = _lib.lib()
    rc = L.dvg_packed_overlap(a, rows_a, a_rs, a_gs, b, rows_b, b_rs, b_gs, groups, n, hist, nearest, 0, None)
    return rc, L.dvg_last_error()


def test_c_argument_validation_without_gpu():
    """Every error of the header's list, with its code (DVG_E_INVALID = -1, DVG_E_UNSUPPORTED = -4) and a message that names
    the argument, on host stand-in pointers: nothing reaches HIP."""
    keep = ctypes.create_string_buffer(16)
    p = ctypes.cast(keep, ctypes.c_void_p)
    for args, word in (((None, p, p), rb"\ba\b"), ((p, p, None), rb"\bhist\b"), ((None, None, p), rb"\ba\b"), ((p, None, None), rb"\bhist\b")):
        rc, msg = _call(*args)
        assert rc == -1 and re.search(word, msg), (rc, msg)
    for b in (p, None):  # cross and self mode
        for name in ("rows_a", "groups", "n"):
            for bad in (0, -1, -2 ** 31):
                rc, msg = _call(p, b, p, **{name: bad})
                assert rc == -1 and re.search(rb"\b" + name.encode() + rb"\b", msg), (name, bad, rc, msg)
        for bad in (1, 0, -1, -2 ** 40):  # n = 64: two words a row
            rc, msg = _call(p, b, p, a_rs=bad)
            assert rc == -1 and b"a_row_stride" in msg, (bad, rc, msg)
        for bad in (-1, -2 ** 40):
            rc, msg = _call(p, b, p, a_gs=bad)
            assert rc == -1 and b"a_group_stride" in msg, (bad, rc, msg)
    for bad in (0, -1, -2 ** 40):
        rc, msg = _call(p, p, p, rows_b=bad)
        assert rc == -1 and b"rows_b" in msg, (bad, rc, msg)
    for bad in (1, 0, -3):
        rc, msg = _call(p, p, p, b_rs=bad)
        assert rc == -1 and b"b_row_stride" in msg, (bad, rc, msg)
    rc, msg = _call(p, p, p, b_gs=-1)
    assert rc == -1 and b"b_group_stride" in msg, (rc, msg)
    # a row stride is measured against W = ceil(n / 32): n = 65 needs three words
    rc, msg = _call(p, p, p, n=65, a_rs=2, b_rs=3)
    assert rc == -1 and b"a_row_stride" in msg, (rc, msg)
    rc, msg = _call(p, p, p, n=65, a_rs=3, b_rs=2)
    assert rc == -1 and b"b_row_stride" in msg, (rc, msg)
    # self mode ignores rows_b and the strides of B
    for kw in (dict(n=8193, a_rs=257), dict(n=2 ** 31 - 1, a_rs=2 ** 26)):
        rc, msg = _call(p, None, p, rows_b=0, b_rs=-5, b_gs=-5, **kw)
        assert rc == -4 and re.search(rb"\bn\b", msg) and b"LDS" in msg, (kw, rc, msg)
    for b in (p, None):
        for bad in (2 ** 31, 2 ** 40):
            rc, msg = _call(p, b, p, rows_a=bad)
            assert rc == -4 and b"rows_a" in msg, (bad, rc, msg)
    for bad in (2 ** 31, 2 ** 40):
        rc, msg = _call(p, p, p, rows_b=bad)
        assert rc == -4 and b"rows_b" in msg, (bad, rc, msg)
    # 2 x 2^31 x 2^30 = 2^62 pairs; one fewer group is below the limit and would launch, so it is not tried here
    rc, msg = _call(p, p, p, rows_a=2 ** 31 - 1, rows_b=2 ** 31 - 1, groups=2 ** 31 - 1)
    assert rc == -4 and b"groups" in msg and b"2^62" in msg, (rc, msg)
    rc, msg = _call(p, p, p, rows_a=2 ** 30, rows_b=2 ** 30, groups=4)
    assert rc == -4 and b"groups" in msg and b"2^62" in msg, (rc, msg)
    rc, msg = _call(p, None, p, rows_a=2 ** 30, groups=4)
    assert rc == -4 and b"groups" in msg and b"2^62" in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture
def untouched(monkeypatch):
    """The library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch, F)


def test_functional_wrapper_rejects_bad_arguments(untouched):
    flat = torch.zeros((5, 3), dtype=torch.int32)  # n = 77: three words
    trace = torch.zeros((4, 6, 3), dtype=torch.int32)
    for bad in (flat.long(), flat.float(), flat[0], flat[None, None], torch.zeros((5, 2), dtype=torch.int32),
                torch.zeros((5, 4), dtype=torch.int32), torch.zeros((0, 3), dtype=torch.int32),
                torch.zeros((4, 0, 3), dtype=torch.int32), flat.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\ba must"):
            F.packed_overlap(bad, n=77)
        with pytest.raises(_lib.DvgError, match=r"\bb must"):
            F.packed_overlap(flat, bad if bad is not None else "rows", n=77)
    for bad in (0, -5, 2.0, True, "77", None):
        with pytest.raises(ValueError, match="n must"):
            F.packed_overlap(flat, n=bad)
    # strides: the last dimension must be dense, a row must not overlap the next
    wide = torch.zeros((5, 6), dtype=torch.int32)
    with pytest.raises(_lib.DvgError, match="a: the last dimension"):
        F.packed_overlap(wide[:, ::2], n=77)
    with pytest.raises(_lib.DvgError, match="b: the last dimension"):
        F.packed_overlap(flat, wide[:, ::2], n=77)
    with pytest.raises(_lib.DvgError, match="a: a row stride"):
        F.packed_overlap(flat[:1].expand(5, 3), n=77)
    with pytest.raises(_lib.DvgError, match="b: a row stride"):
        F.packed_overlap(flat, torch.zeros((9,), dtype=torch.int32).as_strided((4, 3), (2, 1)), n=77)
    # groups: a 3-D b needs a 3-D a with the same M
    with pytest.raises(_lib.DvgError, match="b: a 3-D b"):
        F.packed_overlap(flat, trace, n=77)
    with pytest.raises(_lib.DvgError, match="b: a 3-D b"):
        F.packed_overlap(trace, trace[:, :5], n=77)
    for ok in ((flat, None), (flat, flat[::2]), (trace, None), (trace, flat), (trace, trace[:2]), (trace[:, 1:], trace[:, :-1])):
        with pytest.raises(_lib.DvgError, match="GPU"):  # valid arguments on CPU tensors: the HIP path has no CPU fallback
            F.packed_overlap(*ok, n=77, nearest=True)


def test_trace_overlap_reaches_the_device_check_only(untouched):
    t = smp.Trace(torch.zeros((3, 10, 1), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    other = smp.Trace(torch.zeros((5, 10, 1), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    for args in ((), (other,), (other.bits,), (torch.zeros((7, 1), dtype=torch.int32),)):
        with pytest.raises(_lib.DvgError, match="GPU"):
            t.overlap(*args)
    with pytest.raises(_lib.DvgError, match="b: a 3-D b"):
        t.overlap(smp.Trace(torch.zeros((5, 9, 1), dtype=torch.int32), None, None, smp.trace_sweeps(9, 0, 1), 12))


def test_grbm_replica_overlap_takes_the_local_sampler_only(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    ei = np.arange(12, dtype=np.int64)
    plan = graphs.build_plan(12, np.minimum(ei, (ei + 1) % 12), np.maximum(ei, (ei + 1) % 12))
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for other in (object(), smp.GibbsSampler(plan, [f"q{i}" for i in range(12)], beta=2.0, sweeps=5, seed=3, device="cuda")):
        with pytest.raises(TypeError):
            grbm.replica_overlap(other, prefactor=1.0, num_reads=2)


# ------------------------------------------------------------------------------------------------ the estimators
def _close(got, want, what):
    got = got.numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64 and want.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.allclose(got, want, rtol=1e-12, atol=0.0, equal_nan=True), (what, got, want)


def _check_all(hist, n):
    o = smp.Overlap.from_hist(torch.from_numpy(hist), n)
    want = oo.estimates(hist, n)
    for name, value in want.items():
        _close(getattr(o, name), value, name)
    _close(o.q, oo.q_grid(n), "q")
    _close(o.density, oo.density(hist), "density")
    for lo, hi in ((0.0, 1.0), (0.5, 1.0), (0.0, 0.25), (0.3, 0.2), (1.0, 1.0), (0.0, 0.0)):
        _close(o.mass(lo, hi), oo.mass(hist, n, lo, hi), f"mass({lo}, {hi})")
    assert "Overlap(" in repr(o) and o.n == n
    return o


@pytest.mark.parametrize("n,scale", [(1, 10), (2, 1000), (33, 10 ** 6), (64, 10 ** 12), (77, 3), (512, 10 ** 9)])
def test_properties_equal_the_numpy_restatement(n, scale):
    rng = np.random.default_rng(n)
    hist = rng.integers(0, scale, size=n + 1, dtype=np.int64)
    hist[rng.random(n + 1) < 0.3] = 0
    hist[n // 2] += 1  # (never empty)
    o = _check_all(hist, n)
    assert float(o.pairs) == float(hist.sum()) and abs(float(o.density.sum()) - 1.0) < 1e-12 and float(o.mass(0.0, 1.0)) == 1.0


def test_known_histograms():
    n = 12
    one = np.zeros(n + 1, dtype=np.int64)
    one[0] = 1  # one pair of equal rows
    o = _check_all(one, n)
    assert float(o.q[0]) == 1.0 and float(o.q[n]) == -1.0 and float(o.q[n // 2]) == 0.0
    assert (float(o.pairs), float(o.mean_q), float(o.q2), float(o.q4), float(o.binder), float(o.hamming_mean)) == (1.0, 1.0, 1.0, 1.0, 1.0, 0.0)
    two = np.zeros(n + 1, dtype=np.int64)
    two[0], two[n] = 5, 5  # a mode and its mirror, equally weighted
    o = _check_all(two, n)
    assert (float(o.mean_q), float(o.mean_abs_q), float(o.q2), float(o.binder), float(o.hamming_mean)) == (0.0, 1.0, 1.0, 1.0, n / 2)
    assert float(o.mass(0.5, 1.0)) == 1.0 and float(o.mass(0.0, 0.5)) == 0.0
    empty = _check_all(np.zeros(n + 1, dtype=np.int64), n)
    assert float(empty.pairs) == 0.0
    for name in ("mean_q", "mean_abs_q", "q2", "q4", "binder", "hamming_mean"):
        assert np.isnan(float(getattr(empty, name))), name
    assert np.isnan(empty.density.numpy()).all() and np.isnan(float(empty.mass(0.0, 1.0)))


def test_from_hist_validates():
    hist = torch.zeros(13, dtype=torch.int64)
    assert smp.Overlap.from_hist(hist, 12).n == 12 and smp.Overlap.from_hist(hist, np.int64(12)).n == 12
    for bad in (dict(hist=hist.float()), dict(hist=hist[:12]), dict(hist=hist[None]), dict(hist=hist.numpy()), dict(n=13), dict(n=0),
                dict(n=12.0), dict(n=True)):
        with pytest.raises(ValueError):
            smp.Overlap.from_hist(**dict(dict(hist=hist, n=12), **bad))


def test_the_helper_on_rows_known_by_hand():
    """The numpy definition itself, on four rows of n = 5: distances by hand, the tie to the smaller index, the diagonal out."""
    s = np.array([[1, 1, 1, 1, 1], [1, 1, 1, 1, -1], [-1, -1, -1, -1, -1], [1, 1, 1, 1, 1]], dtype=np.int8)
    bits = trace_oracle.pack(s) | np.uint32(0xFFFFFFE0)  # noise in the bits of spins >= n
    hist, nearest = oo.overlap(bits, None, 5)
    assert hist.tolist() == [1, 2, 0, 0, 1, 2]  # d(0,3)=0; d(0,1)=d(1,3)=1; d(1,2)=4; d(0,2)=d(2,3)=5
    assert oo.split(nearest)[0].tolist() == [[0, 1, 4, 0]] and oo.split(nearest)[1].tolist() == [[3, 0, 1, 0]]
    hist, nearest = oo.overlap(bits[:3], bits[2:], 5)
    assert hist.tolist() == [2, 1, 0, 0, 1, 2] and oo.split(nearest)[0].tolist() == [[0, 1, 0]] and oo.split(nearest)[1].tolist() == [[1, 1, 0]]
    hist, nearest = oo.overlap(bits[:1], None, 5)
    assert hist.sum() == 0 and nearest.tolist() == [[-1]] and oo.split(nearest)[1].tolist() == [[-1]]


# ------------------------------------------------------------------------------------------------ the measure means what it claims
@functools.lru_cache(maxsize=None)
def _pegasus64():
    mg, _ = graphs.get_graph_mapping(graphs.greedy_get_subgraph(64, SEED, graphs.pegasus_graph(16)))
    _nodes, ei, ej = graphs.edges_of(mg)
    plan = graphs.build_plan(64, ei, ej)
    assert plan.n == 64 and plan.n_edges == 346
    return plan


def _draw(Js, beta, sweeps, burn_in, thin):
    plan = _pegasus64()
    ids = np.arange(48, dtype=np.uint32) + 1000
    tr = trace_oracle.trace(plan, np.zeros(64, np.float32), np.full(plan.n_edges, Js, np.float32), beta, ids, SEED, 6, sweeps,
                            burn_in=burn_in, thin=thin)
    hist, _nearest = oo.overlap(tr.bits, None, 64)
    return smp.Overlap.from_hist(torch.from_numpy(hist), 64), tr.bits.shape[1]


def test_hot_chains_overlap_like_fair_coins():
    """beta = 0: every record is 64 fair coins per chain, so E q^2 = 1 / n, and the q^2 of distinct pairs are independent:
    Var q^2 = E q^4 - 1 / n^2 = (3 n - 2) / n^3 - 1 / n^2 ~ 2 / n^2, standard error sqrt(2 / (n^2 pairs)).  6 of them."""
    o, M = _draw(0.0, 0.0, 12, 4, 1)
    n, pairs = 64, 8 * 48 * 47 // 2
    assert M == 8 and float(o.pairs) == pairs == 9024
    se = np.sqrt(2.0 / (n * n * pairs))
    z = (float(o.q2) - 1.0 / n) / se
    print(f"hot chains: q2 = {float(o.q2):.6f} against 1 / n = {1.0 / n:.6f}: {z:+.2f} standard errors; binder {float(o.binder):.3f}")
    assert abs(z) <= 6.0


def test_cold_ferromagnetic_chains_sit_in_one_mode_or_its_mirror():
    """J = -1 on every edge (ferromagnetic in this sign convention) at beta = 1: the chains have ordered, all up or all down,
    so |q| is near 1 for every pair.  The draws are deterministic: with the numpy definition they gave q2 = 0.815, binder =
    0.893, mass(0.5, 1) = 0.815; the bounds are margin over those values, not statistics."""
    o, M = _draw(-1.0, 1.0, 60, 40, 5)
    assert M == 4 and float(o.pairs) == 4 * 48 * 47 // 2 == 4512
    q2, binder, mass = float(o.q2), float(o.binder), float(o.mass(0.5, 1.0))
    print(f"cold chains: q2 = {q2:.3f}, binder = {binder:.3f}, mass(0.5, 1) = {mass:.3f}")
    assert q2 >= 0.5 and binder >= 0.6 and mass >= 0.5
