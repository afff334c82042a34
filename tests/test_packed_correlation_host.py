"""CPU-side checks of the full pair-correlation sums of bit-packed rows ("DVG corr v1", ``dvg_packed_correlation`` in
include/dvg.h): the symbols, every argument error of the C entry point (before any HIP call, on host stand-in pointers) and
of the Python surface (before the library is touched), the workspace query, the estimates of ``sampler.Correlations`` on CPU
tensors against their numpy restatement (``tests/correlation_oracle.py``) -- to 1e-12 relative and on known cases by value --
and what the measure says about CPU draws of the unchanged oracle (``trace_oracle.trace``): a cold ferromagnetic chain's
neighbours are correlated, a hot one's are not."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correlation_oracle as co  # noqa: E402
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 775321899904


# ------------------------------------------------------------------------------------------------ the symbols and their checks
def test_symbols_are_declared_bound_and_exported():
    support.assert_declared_bound_exported({"dvg_packed_correlation": "int", "dvg_packed_correlation_workspace_bytes": "size_t"}, markers=["DVG corr v1"],
                                           kernels=["packed_correlation_transpose_kernel", "packed_correlation_kernel"])
    # the slab bound the wrap argument rests on, where the tests can read it
    src = open(os.path.join(ROOT, "image-generation_amd", "csrc", "correlation.hip")).read()
    assert "static_assert(CR_SLAB_ROWS == 1 << 18" in src and F.PACKED_CORRELATION_SLAB_ROWS == 1 << 18


class _Host:
    """Host stand-ins for the device pointers, 16-byte aligned, filled with a pattern that must survive every rejected call."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(b"\x5a" * 4096, 4096)
        base = (ctypes.addressof(self.buf) + 15) & ~15
        self.bits, self.spin, self.pair, self.ws = (ctypes.c_void_p(base + 1024 * k) for k in range(4))

    def intact(self):
        return self.buf.raw == b"\x5a" * 4096


def _call(h, *, bits=True, pair=True, spin=True, ws=True, rows=5, rs=2, groups=1, gs=0, n=64, ws_bytes=None, accumulate=0):
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = max(int(L.dvg_packed_correlation_workspace_bytes(rows, groups, n)), 1 << 20)
    wsp = h.ws if ws is True else ws
    rc = L.dvg_packed_correlation(h.bits if bits else None, rows, rs, groups, gs, n, h.spin if spin else None,
                                  h.pair if pair else None, accumulate, wsp if ws else None, ws_bytes, None)
    return rc, L.dvg_last_error()


def test_c_argument_validation_without_gpu():
    """Every error of the header's list, with its code (DVG_E_INVALID = -1, DVG_E_WORKSPACE = -3, DVG_E_UNSUPPORTED = -4) and
    a message that names the argument: nothing reaches HIP, nothing is written."""
    h = _Host()
    for spin in (True, False):
        for kw, word in ((dict(bits=False), rb"\bbits\b"), (dict(pair=False), rb"\bpair_sum\b"), (dict(ws=False), rb"\bws\b")):
            rc, msg = _call(h, spin=spin, **kw)
            assert rc == -1 and re.search(word, msg) and b"null" in msg, (kw, rc, msg)
        for name in ("rows", "groups", "n"):
            for bad in (0, -1, -2 ** 31):
                rc, msg = _call(h, spin=spin, **{name: bad})
                assert rc == -1 and re.search(rb"\b" + name.encode() + rb"=", msg), (name, bad, rc, msg)
        for bad in (1, 0, -1, -2 ** 40):  # n = 64: two words a row
            rc, msg = _call(h, spin=spin, rs=bad)
            assert rc == -1 and b"row_stride" in msg, (bad, rc, msg)
        for bad in (-1, -2 ** 40):
            rc, msg = _call(h, spin=spin, gs=bad)
            assert rc == -1 and b"group_stride" in msg, (bad, rc, msg)
    rc, msg = _call(h, n=65, rs=2)  # a row stride is measured against W = ceil(n / 32): n = 65 needs three words
    assert rc == -1 and b"row_stride" in msg, (rc, msg)
    rc, msg = _call(h, ws=ctypes.c_void_p(h.ws.value + 8))
    assert rc == -1 and re.search(rb"\bws\b", msg) and b"aligned" in msg, (rc, msg)
    for kw in (dict(n=8193, rs=257), dict(n=2 ** 31 - 1, rs=2 ** 26)):
        rc, msg = _call(h, ws_bytes=1 << 40, **kw)
        assert rc == -4 and re.search(rb"\bn=", msg) and b"8192" in msg, (kw, rc, msg)
    for kw in (dict(rows=2 ** 31, groups=2 ** 31), dict(rows=2 ** 62), dict(groups=2 ** 62), dict(rows=2 ** 63 - 1, groups=2 ** 63 - 1)):
        rc, msg = _call(h, ws_bytes=1 << 62, **kw)
        assert rc == -4 and b"groups" in msg and b"rows" in msg and b"2^62" in msg, (kw, rc, msg)
    rc, msg = _call(h, rows=2 ** 50, ws_bytes=1 << 62)  # below 2^62 rows, but more slabs than a grid has workgroups
    assert rc == -4 and b"rows" in msg and b"launch" in msg, (rc, msg)
    L = _lib.lib()
    for rows, groups, n in ((5, 1, 64), (1, 1, 1), (1025, 3, 77), (300000, 1, 33)):
        need = int(L.dvg_packed_correlation_workspace_bytes(rows, groups, n))
        for short in (0, 1, need - 1):
            rc, msg = _call(h, rows=rows, groups=groups, n=n, rs=(n + 31) // 32, ws_bytes=short)
            assert rc == -3 and b"ws_bytes" in msg, (rows, groups, n, short, rc, msg)
    assert h.intact()


def test_workspace_query():
    """> 0, monotone in rows, the documented size -- n columns of ceil(T / 1024) 128 bytes, T = groups rows -- and 0 for
    arguments the entry rejects."""
    q = _lib.lib().dvg_packed_correlation_workspace_bytes
    for n in (1, 33, 64, 77, 512, 8192):
        last = 0
        for rows in (1, 63, 64, 65, 1023, 1024, 1025, 4096, 51200, 300000, 2 ** 24 + 1):
            got = int(q(rows, 1, n))
            assert got == n * ((rows + 1023) // 1024) * 128 and got > 0 and got >= last, (n, rows, got)
            last = got
    assert int(q(130, 7, 77)) == int(q(910, 1, 77)) == int(q(7, 130, 77)) == 77 * 128
    assert int(q(1, 1025, 5)) == 5 * 2 * 128
    for rows, groups, n in ((0, 1, 5), (1, 0, 5), (1, 1, 0), (-3, 1, 5), (1, 1, 8193), (2 ** 31, 2 ** 31, 5), (2 ** 50, 1, 5)):
        assert int(q(rows, groups, n)) == 0, (rows, groups, n)


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
        with pytest.raises(_lib.DvgError, match=r"\bbits must"):
            F.packed_correlation(bad, n=77)
    for bad in (0, -5, 2.0, True, "77", None):
        with pytest.raises(ValueError, match="n must"):
            F.packed_correlation(flat, n=bad)
    wide = torch.zeros((5, 6), dtype=torch.int32)
    with pytest.raises(_lib.DvgError, match="bits: the last dimension"):
        F.packed_correlation(wide[:, ::2], n=77)
    with pytest.raises(_lib.DvgError, match="bits: a row stride"):
        F.packed_correlation(flat[:1].expand(5, 3), n=77)
    spin, pair = torch.zeros(77, dtype=torch.int64), torch.zeros((77, 77), dtype=torch.int64)
    for bad, word in (((spin, pair[:76]), "pair_sum"), ((spin, pair.int()), "pair_sum"), ((spin[:76], pair), "spin_sum"),
                      ((spin.float(), pair), "spin_sum"), ((None, pair), "spin_sum"), ((spin, None), "pair_sum"), (pair, "a pair"),
                      ((spin, pair, pair), "a pair")):
        with pytest.raises(_lib.DvgError, match=word):
            F.packed_correlation(flat, n=77, out=bad)
    with pytest.raises(_lib.DvgError, match="spin_sum"):
        F.packed_correlation(flat, n=77, spin_sums=False, out=(spin, pair))
    with pytest.raises(_lib.DvgError, match="pair_sum"):
        F.packed_correlation(flat, n=77, out=(spin, torch.zeros((154, 77), dtype=torch.int64)[::2]))
    for ok in (flat, flat[::2], trace, trace[:, 1:], trace[:2, ::2]):
        for kw in ({}, dict(spin_sums=False), dict(out=(spin, pair)), dict(spin_sums=False, out=(None, pair))):
            with pytest.raises(_lib.DvgError, match="GPU"):  # valid arguments on CPU tensors: the HIP path has no CPU fallback
                F.packed_correlation(ok, n=77, **kw)


def test_trace_correlations_reaches_the_device_check_only(untouched):
    t = smp.Trace(torch.zeros((3, 10, 1), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    with pytest.raises(_lib.DvgError, match="GPU"):
        t.correlations()


def test_grbm_model_correlations_takes_the_local_sampler_only(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    ei = np.arange(12, dtype=np.int64)
    plan = graphs.build_plan(12, np.minimum(ei, (ei + 1) % 12), np.maximum(ei, (ei + 1) % 12))
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for other in (object(), smp.GibbsSampler(plan, [f"q{i}" for i in range(12)], beta=2.0, sweeps=5, seed=3, device="cuda")):
        with pytest.raises(TypeError):
            grbm.model_correlations(other, prefactor=1.0, num_reads=2)


# ------------------------------------------------------------------------------------------------ the estimates
def _close(got, want, what):
    got = got.numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64 and want.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.allclose(got, want, rtol=1e-12, atol=0.0, equal_nan=True), (what, got, want)


def _path_plan(n):
    ei = np.arange(n - 1, dtype=np.int64)
    return graphs.build_plan(n, ei, ei + 1)


def _random_plan(n, edges, seed):
    return support.random_plan(n, edges=edges, seed=seed)


def _correlations(x):
    """``sampler.Correlations`` and the oracle's estimates of (T, n) +-1 rows, through packed bits and the oracle's sums."""
    bits = trace_oracle.pack(x)
    n, T = x.shape[1], x.shape[0]
    spin_sum, pair_sum = co.sums(bits, n)
    assert np.array_equal(pair_sum, pair_sum.T) and (np.diag(pair_sum) == T).all()
    c = smp.Correlations.from_sums(torch.from_numpy(spin_sum), torch.from_numpy(pair_sum), T)
    return c, co.estimates(spin_sum, pair_sum, T)


def _check_all(c, want, plan, other=None, want_other=None):
    for name, value in want.items():
        _close(getattr(c, name), value, name)
    C, n = want["connected"], c.n
    assert "Correlations(" in repr(c) and f"n={n}" in repr(c)
    _close(c.on_edges(plan), co.on_edges(C, plan.edge_i, plan.edge_j), "on_edges")
    assert tuple(c.on_edges(plan).shape) == (plan.n_edges,)
    _close(c.off_edge_share(plan), co.off_edge_share(C, plan.edge_i, plan.edge_j), "off_edge_share")
    for k in (0, 1, 5, n * n):
        for edges in ((None, None), (plan.edge_i, plan.edge_j)):
            i, j, v = c.top_pairs(k, None if edges[0] is None else plan)
            wi, wj, wv = co.top_pairs(C, k, *edges)
            assert i.dtype == j.dtype == torch.int64 and np.array_equal(i.numpy(), wi) and np.array_equal(j.numpy(), wj), (k, i, wi)
            _close(v, wv, "top_pairs")
    if other is not None:
        for edges in ((None, None), (plan.edge_i, plan.edge_j)):
            got = c.gap(other, None if edges[0] is None else plan)
            want_gap = co.gap(want, want_other, *edges)
            assert set(got) == set(want_gap) == ({"spin_rms", "pair_rms"} | ({"edge_rms", "off_edge_rms"} if edges[0] is not None else set()))
            for name, value in want_gap.items():
                _close(got[name], value, name)


@pytest.mark.parametrize("n,T", [(1, 7), (2, 100), (5, 3), (33, 1000), (64, 4097), (77, 50)])
def test_members_equal_the_numpy_restatement(n, T):
    rng = np.random.default_rng(n * 1000 + T)
    bias = rng.uniform(0.2, 0.8, n)
    x = np.where(rng.random((T, n)) < bias, 1, -1)
    y = np.where(rng.random((T + 3, n)) < 0.5, 1, -1)
    if n >= 5:
        x[:, 3] = x[:, 1] * np.where(rng.random(T) < 0.9, 1, -1)  # a strongly correlated pair
    plan = _random_plan(n, min(2 * n, n * (n - 1) // 2), n) if n > 1 else graphs.build_plan(1, [], [])
    (c, want), (d, want_d) = _correlations(x), _correlations(y)
    _check_all(c, want, plan, d, want_d)
    # GraphHandle-like objects are read through their plan
    holder = type("Holder", (), {"plan": plan})()
    _close(c.off_edge_share(holder), co.off_edge_share(want["connected"], plan.edge_i, plan.edge_j), "off_edge_share")


def test_independent_fair_coins_have_chi_sg_near_one():
    """n fair-coin columns over T rows: C_ii = 1 - m_i^2 and, for i != j, C_ij has mean 0 and variance about 1 / T, so
    chi_sg = (1 / n) sum_ij C_ij^2 is about 1 + (n - 3) / T (the diagonal gives 1 - 2 / T, the n - 1 partners of a spin 1 / T
    each).  The n (n - 1) / 2 distinct off-diagonal squares are nearly independent with variance 2 / T^2 each and enter twice:
    standard error (2 / n) sqrt(n (n - 1)) / T.  Six of them."""
    n, T = 32, 4096
    x = np.where(np.random.default_rng(7).random((T, n)) < 0.5, 1, -1)
    c, _want = _correlations(x)
    se = 2.0 / n * np.sqrt(n * (n - 1)) / T
    z = (float(c.chi_sg) - (1.0 + (n - 3) / T)) / se
    print(f"fair coins: chi_sg = {float(c.chi_sg):.6f} against {1.0 + (n - 3) / T:.6f}: {z:+.2f} standard errors")
    assert abs(z) <= 6.0


def test_copies_negations_and_frozen_spins():
    rng = np.random.default_rng(3)
    x = np.where(rng.random((200, 6)) < 0.4, 1, -1)
    x[:, 2] = x[:, 0]   # a copy
    x[:, 3] = -x[:, 1]  # a negation
    x[:, 5] = 1         # frozen
    c, want = _correlations(x)
    _check_all(c, want, _path_plan(6))
    p = c.pearson.numpy()
    assert abs(p[0, 2] - 1.0) <= 1e-15 and abs(p[2, 0] - 1.0) <= 1e-15 and abs(p[1, 3] + 1.0) <= 1e-15
    assert np.isnan(p[5]).all() and np.isnan(p[:, 5]).all() and not np.isnan(p[:5, :5]).any()
    assert np.allclose(np.diag(p)[:5], 1.0, rtol=0, atol=1e-15)
    assert (c.connected.numpy()[5] == 0).all() and float(c.mean_spin[5]) == 1.0


def test_top_pairs_tie_rule():
    """|C| by hand on n = 4: (0, 1), (0, 3), (2, 3) tie at 0.5, (1, 2) holds 0.75, the rest 0.25: the largest first, then the
    ties in the order of their flat index i n + j, whatever the sign."""
    T = 8
    pair = np.full((4, 4), 2, dtype=np.int64)
    for (i, j), v in {(0, 1): 4, (0, 3): -4, (2, 3): 4, (1, 2): -6, (0, 2): 2, (1, 3): -2}.items():
        pair[i, j] = pair[j, i] = v
    np.fill_diagonal(pair, T)
    c = smp.Correlations.from_sums(torch.zeros(4, dtype=torch.int64), torch.from_numpy(pair), T)
    i, j, v = c.top_pairs(4)
    assert list(zip(i.tolist(), j.tolist())) == [(1, 2), (0, 1), (0, 3), (2, 3)] and v.tolist() == [-0.75, 0.5, -0.5, 0.5]
    i, j, v = c.top_pairs(10)
    assert list(zip(i.tolist(), j.tolist())) == [(1, 2), (0, 1), (0, 3), (2, 3), (0, 2), (1, 3)]
    plan = graphs.build_plan(4, [1, 0], [2, 1])  # edges (1, 2) and (0, 1) are left out
    i, j, v = c.top_pairs(3, plan)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 3), (2, 3), (0, 2)]
    i, j, v = c.top_pairs(10, plan)
    assert len(i) == 4 and (1, 2) not in set(zip(i.tolist(), j.tolist()))
    for bad in (-1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must"):
            c.top_pairs(bad)


def test_off_edge_share_of_a_path_whose_only_correlated_pair_is_no_edge():
    """The path 0 - 1 - 2 - 3 and the 8 rows of every (s_0, s_1, s_3) with s_2 = s_0: all means are 0, every pair is
    uncorrelated but (0, 2), which is no edge of the path."""
    x = np.array([[a, b, a, d] for a in (1, -1) for b in (1, -1) for d in (1, -1)])
    c, want = _correlations(x)
    plan = _path_plan(4)
    assert float(c.off_edge_share(plan)) == 1.0 and (c.on_edges(plan) == 0).all() and float(c.connected[0, 2]) == 1.0
    i, j, v = c.top_pairs(1, plan)
    assert (int(i[0]), int(j[0]), float(v[0])) == (0, 2, 1.0)
    full = graphs.build_plan(4, [0, 0, 0, 1, 1, 2], [1, 2, 3, 2, 3, 3])
    assert float(c.off_edge_share(full)) == 0.0 and len(c.top_pairs(3, full)[0]) == 0
    # nothing is correlated at all: 0 / 0
    flat = smp.Correlations.from_sums(torch.zeros(4, dtype=torch.int64), 8 * torch.eye(4, dtype=torch.int64), 8)
    assert np.isnan(float(flat.off_edge_share(plan)))
    g = c.gap(c, plan)
    assert all(float(g[k]) == 0.0 for k in ("spin_rms", "pair_rms", "edge_rms", "off_edge_rms"))
    assert np.isnan(float(c.gap(c, full)["off_edge_rms"]))


def test_from_sums_validates():
    spin, pair = torch.zeros(5, dtype=torch.int64), torch.zeros((5, 5), dtype=torch.int64)
    assert smp.Correlations.from_sums(spin, pair, 3).n == 5 and smp.Correlations.from_sums(spin, pair, np.int64(3)).count == 3
    for bad in (dict(spin_sum=spin.float()), dict(spin_sum=spin[:4]), dict(spin_sum=spin.numpy()), dict(pair_sum=pair.float()),
                dict(pair_sum=pair[:4]), dict(pair_sum=pair.reshape(-1)), dict(pair_sum=None), dict(count=0), dict(count=-2),
                dict(count=2.0), dict(count=True)):
        with pytest.raises(ValueError):
            smp.Correlations.from_sums(**dict(dict(spin_sum=spin, pair_sum=pair, count=3), **bad))
    c = smp.Correlations.from_sums(spin, pair, 3)
    with pytest.raises(ValueError):
        c.gap(smp.Correlations.from_sums(spin[:4], pair[:4, :4], 3))
    with pytest.raises(ValueError):
        c.on_edges(_path_plan(6))


# ------------------------------------------------------------------------------------------------ the measure means what it claims
def _chain_draw(Js, beta):
    plan = _path_plan(12)
    ids = np.arange(48, dtype=np.uint32) + 1000
    tr = trace_oracle.trace(plan, np.zeros(12, np.float32), np.full(plan.n_edges, Js, np.float32), beta, ids, SEED, 6, 60, burn_in=20,
                            thin=5)
    assert tr.bits.shape == (48, 8, 1)
    spin_sum, pair_sum = co.sums(tr.bits, 12)
    c = smp.Correlations.from_sums(torch.from_numpy(spin_sum), torch.from_numpy(pair_sum), 48 * 8)
    _check_all(c, co.estimates(spin_sum, pair_sum, 48 * 8), plan)
    return c, plan


def test_cold_neighbours_are_correlated_and_hot_ones_are_not():
    """An open chain of 12 spins, J = -1 on every bond (ferromagnetic in this sign convention), no field.  At beta = 1 the
    exact neighbour correlation is tanh(1) = 0.76 and a pair k bonds apart has tanh(1)^k; at beta = 0 every spin is a fair
    coin.  384 records each: the cold chain's mean connected correlation over the bonds exceeds the hot one's by far, and its
    correlation spills onto pairs that are no bonds."""
    cold, plan = _chain_draw(-1.0, 1.0)
    hot, _plan = _chain_draw(-1.0, 0.0)
    c_cold, c_hot = float(cold.on_edges(plan).mean()), float(hot.on_edges(plan).mean())
    print(f"bonds: cold {c_cold:.3f}, hot {c_hot:.3f}; chi_sg cold {float(cold.chi_sg):.3f}, hot {float(hot.chi_sg):.3f}; "
          f"off-edge share cold {float(cold.off_edge_share(plan)):.3f}")
    assert c_cold > c_hot and c_cold >= 0.5 and abs(c_hot) <= 0.1
    assert float(cold.chi_sg) > float(hot.chi_sg) and float(cold.off_edge_share(plan)) >= 0.3
    g = cold.gap(hot, plan)
    assert float(g["edge_rms"]) >= 0.5 and float(g["edge_rms"]) > float(g["off_edge_rms"]) > 0.0
