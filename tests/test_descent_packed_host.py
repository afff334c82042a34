"""CPU-side checks of the zero-temperature descent of bit-packed rows ("DVG descent v1", ``dvg_grbm_descend_packed`` in
include/dvg.h): the symbol and the profiler name, every argument error of the C entry point (before any HIP call, on host
stand-in pointers) and of the Python surface (before the library is touched), the numpy definition itself
(``tests/descent_oracle.py``) on all 4096 states of a 12-spin ring, and ``sampler.Minima`` on CPU tensors against hand-built
outputs."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descent_oracle as do  # noqa: E402
import fields_oracle as fo  # noqa: E402
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

NAME = "dvg_grbm_descend_packed"


# ------------------------------------------------------------------------------------------------ the symbol and its checks
def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported(NAME, markers=["DVG descent v1"], kernels=["grbm_descend_packed_kernel"], arity={NAME: 19})


_stand_in = support.graph_stand_in


def _set_n(graph, n, n_edges=0):
    (ctypes.c_int32 * 2).from_buffer(graph)[:] = [n, n_edges]


def _call(g, lin, quad, bits, out, *, prefactor=1.0, rows=5, row_stride=2, groups=1, group_stride=0, max_sweeps=10, counts=None):
    L = _lib.lib()
    p = lambda v: None if v is None else ctypes.c_void_p(v) if isinstance(v, int) else v  # noqa: E731
    rc = L.dvg_grbm_descend_packed(p(g), p(lin), p(quad), prefactor, -4.0, 4.0, -1.0, 1.0, p(bits), rows, row_stride, groups,
                                   group_stride, max_sweeps, p(out), p(counts), p(counts), p(counts), None)
    return rc, L.dvg_last_error()


def test_c_argument_validation_without_gpu():
    """Every error of the header's list, with its code (DVG_E_INVALID = -1, DVG_E_UNSUPPORTED = -4) and a message that names
    the argument, on host stand-in pointers: nothing reaches HIP."""
    graph, g, base, _keep = _stand_in()  # n = 64: two words a row
    lin, quad, bits, out = base, base + 64, base + 8192, base + 32768
    for k, word in enumerate((rb"\bg\b", rb"\blinear\b", rb"\bquadratic\b", rb"\bbits\b", rb"\bbits_out\b")):
        args = [g, lin, quad, bits, out]
        args[k] = None
        rc, msg = _call(*args)
        assert rc == -1 and re.search(word, msg) and b"null" in msg, (k, rc, msg)
    for name in ("rows", "groups"):
        for bad in (0, -1, -2 ** 40):
            rc, msg = _call(g, lin, quad, bits, out, **{name: bad})
            assert rc == -1 and re.search(rb"\b" + name.encode() + rb"\b", msg), (name, bad, rc, msg)
    for bad in (1, 0, -1, -2 ** 40):
        rc, msg = _call(g, lin, quad, bits, out, row_stride=bad)
        assert rc == -1 and b"row_stride" in msg, (bad, rc, msg)
    for bad in (-1, -2 ** 40):
        rc, msg = _call(g, lin, quad, bits, out, groups=3, group_stride=bad)
        assert rc == -1 and b"group_stride" in msg, (bad, rc, msg)
    for bad in (float("nan"), float("inf"), -float("inf")):
        rc, msg = _call(g, lin, quad, bits, out, prefactor=bad)
        assert rc == -1 and b"prefactor" in msg, (bad, rc, msg)
    for bad in (0, 65537, -1, -2 ** 31, 2 ** 31 - 1):
        rc, msg = _call(g, lin, quad, bits, out, max_sweeps=bad)
        assert rc == -1 and b"max_sweeps" in msg and b"65536" in msg, (bad, rc, msg)
    _set_n(graph, 65)  # a row stride is measured against W = ceil(n / 32): n = 65 needs three words
    rc, msg = _call(g, lin, quad, bits, out, row_stride=2)
    assert rc == -1 and b"row_stride" in msg, (rc, msg)
    _set_n(graph, 64)
    # overlap (5 rows of 2 words = 40 bytes out).  (a) the output starts inside the input, or the input inside the output
    for delta in (4, 8, 36, -4, -36):
        rc, msg = _call(g, lin, quad, bits, bits + delta)
        assert rc == -1 and b"bits_out" in msg and b"overlap" in msg, (delta, rc, msg)
    # (b) bits_out == bits, but the input is not dense: padded rows, a padded group, a broadcast group
    for kw in (dict(row_stride=3), dict(groups=2, group_stride=12), dict(groups=2, group_stride=0), dict(groups=2, group_stride=9)):
        rc, msg = _call(g, lin, quad, bits, bits, **kw)
        assert rc == -1 and b"bits_out" in msg and b"overlap" in msg and b"dense" in msg, (kw, rc, msg)
    # (c) a strided input reaches further than its rows' words: 5 rows at stride 100 end 402 words on
    rc, msg = _call(g, lin, quad, bits, bits + 4 * 401, row_stride=100)
    assert rc == -1 and b"overlap" in msg, (rc, msg)
    # not overlapping, and the exact alias: these pass the checks above and are refused later, as unsupported
    _set_n(graph, 8193)  # 257 words a row: 5 rows at stride 400 end 1857 words on
    for o, kw in ((bits + 4 * 1857, dict(row_stride=400)), (bits - 4 * 5 * 257, dict(row_stride=257)), (bits, dict(row_stride=257)),
                  (bits, dict(row_stride=257, groups=2, group_stride=5 * 257))):
        rc, msg = _call(g, lin, quad, bits, o, **kw)
        assert rc == -4 and re.search(rb"\bn=", msg) and b"8192" in msg and b"LDS" in msg, (kw, rc, msg)
    _set_n(graph, 2 ** 31 - 1)
    rc, msg = _call(g, lin, quad, bits, bits, row_stride=2 ** 26)
    assert rc == -4 and re.search(rb"\bn=", msg), (rc, msg)
    _set_n(graph, 64)
    for rows, groups in ((2 ** 31, 2 ** 31), (2 ** 62, 1), (1, 2 ** 62)):  # (in place and dense: past the overlap check)
        rc, msg = _call(g, lin, quad, bits, bits, rows=rows, groups=groups, group_stride=2 * rows if groups > 1 else 0)
        assert rc == -4 and b"groups" in msg and b"rows" in msg and b"2^62" in msg, (rows, groups, rc, msg)


# ------------------------------------------------------------------------------------------------ the Python surface
_ring_plan = support.ring_plan


_random_plan = support.random_plan


@pytest.fixture
def untouched(monkeypatch):
    """The library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch, F)


class _Handle:  # (what the wrapper reads before the library: the plan)
    def __init__(self, plan):
        self.plan, self.ptr = plan, None


def test_functional_wrapper_rejects_bad_arguments(untouched):
    plan = _random_plan()  # n = 77: three words
    gh = _Handle(plan)
    lin, quad = torch.zeros(plan.n), torch.zeros(plan.n_edges)
    flat = torch.zeros((5, 3), dtype=torch.int32)
    trace = torch.zeros((4, 6, 3), dtype=torch.int32)
    call = lambda b=flat, l=lin, q=quad, **kw: F.grbm_descend_packed(b, gh, l, q, **kw)  # noqa: E731,E741
    for bad in (flat.long(), flat.float(), flat[0], flat[None, None], torch.zeros((5, 2), dtype=torch.int32),
                torch.zeros((5, 4), dtype=torch.int32), torch.zeros((0, 3), dtype=torch.int32),
                torch.zeros((4, 0, 3), dtype=torch.int32), flat.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\bbits must"):
            call(bad)
    wide = torch.zeros((5, 6), dtype=torch.int32)
    with pytest.raises(_lib.DvgError, match="bits: the last dimension"):
        call(wide[:, ::2])
    with pytest.raises(_lib.DvgError, match="bits: a row stride"):
        call(flat[:1].expand(5, 3))
    for bad in (lin.double(), lin[:-1], torch.zeros(plan.n + 1), lin.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\blinear must"):
            call(l=bad)
    for bad in (quad.double(), quad[:-1], quad.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\bquadratic must"):
            call(q=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="prefactor"):
            call(prefactor=bad)
    for bad in ((1.0,), (1.0, 2.0, 3.0), 4.0, "ab", (float("nan"), 1.0), (None, 1.0), (True, 2.0)):
        with pytest.raises(ValueError, match="linear_range"):
            call(linear_range=bad)
        with pytest.raises(ValueError, match="quadratic_range"):
            call(quadratic_range=bad)
    for bad in (0, -1, 65537, 2 ** 40, 1.0, 10.5, "10", None, True):
        with pytest.raises(ValueError, match="max_sweeps"):
            call(max_sweeps=bad)
    for bad in (flat.long(), flat[:-1], flat.numpy(), torch.zeros((5, 6), dtype=torch.int32)[:, :3], torch.zeros((1, 5, 3), dtype=torch.int32)):
        with pytest.raises(_lib.DvgError, match=r"\bout must"):
            call(out=bad)
    # sharing memory: only bits itself, contiguous
    pool = torch.zeros((40,), dtype=torch.int32)
    with pytest.raises(_lib.DvgError, match="out shares memory"):
        call(pool[:15].view(5, 3), out=pool[3:18].view(5, 3))
    with pytest.raises(_lib.DvgError, match="out shares memory"):
        call(pool[3:18].view(5, 3), out=pool[:15].view(5, 3))
    with pytest.raises(_lib.DvgError, match="out shares memory"):
        call(pool.as_strided((5, 3), (6, 1)), out=pool[:15].view(5, 3))  # (same start, padded rows)
    with pytest.raises(_lib.DvgError, match="out shares memory"):
        call(pool.as_strided((5, 3), (6, 1)), out=pool[20:35].view(5, 3))  # (the padded rows end at word 27)
    for ok, out in ((flat, None), (flat, flat), (flat, torch.zeros_like(flat)), (flat[::2], None), (flat[:1], flat[:1]), (trace, trace),
                    (trace[:, 1:], None), (trace[::2], torch.zeros((2, 6, 3), dtype=torch.int32)), (trace[:1].expand(3, 6, 3), None),
                    (pool.as_strided((5, 3), (4, 1)), pool[20:35].view(5, 3))):  # (the last: rows that end at word 19)
        with pytest.raises(_lib.DvgError, match="GPU"):  # valid arguments on CPU tensors: the HIP path has no CPU fallback
            call(ok, prefactor=0.3, linear_range=(-4, 4), quadratic_range=(-1.0, float("inf")), max_sweeps=np.int64(65536), out=out)


def test_trace_model_and_sampler_methods_check_before_the_library(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    gh = _Handle(_ring_plan())
    lin, quad = torch.zeros(12), torch.zeros(12)
    t = smp.Trace(torch.zeros((3, 10, 1), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    with pytest.raises(_lib.DvgError, match="GPU"):
        t.descend(gh, lin, quad)
    with pytest.raises(_lib.DvgError, match="GPU"):
        t.descend(gh, lin, quad, prefactor=0.5, linear_range=(-4, 4), quadratic_range=(-1, 1), max_sweeps=3)
    with pytest.raises(_lib.DvgError, match=r"\blinear must"):
        t.descend(gh, lin[:-1], quad)
    with pytest.raises(ValueError, match="max_sweeps"):
        t.descend(gh, lin, quad, max_sweeps=0)
    with pytest.raises(ValueError, match="max_sweeps"):
        smp.descend(t.bits, gh, lin, quad, max_sweeps=65537)
    wrong = smp.Trace(torch.zeros((3, 10, 2), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    with pytest.raises(_lib.DvgError, match=r"\bbits must"):
        wrong.descend(gh, lin, quad)
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for bad in (torch.zeros((4, 1), dtype=torch.int32), torch.ones((4, 12)), np.zeros((4, 1), dtype=np.int32), None):
        with pytest.raises(_lib.DvgError, match="GPU"):
            grbm.descend(bad, prefactor=1.0)
    from image_generation_amd.model_wrapper import ModelWrapper
    assert callable(ModelWrapper.prior_minima)


# ------------------------------------------------------------------------------------------------ the definition itself
def _ring_fields(seed=12, scale=1.0):
    """The 12-spin ring with (h, J) on the 2^-10 grid: every float32 field sum is exact."""
    plan = _ring_plan()
    rng = np.random.default_rng(seed)
    h = (scale * rng.integers(-1024, 1025, plan.n) / 1024.0).astype(np.float32)
    J = (scale * rng.integers(-1024, 1025, plan.n_edges) / 1024.0).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 1.0, None, None)
    return plan, hs, Js


@functools.lru_cache(maxsize=None)
def _ring_descent(seed=12):
    plan, hs, Js = _ring_fields(seed)
    start = fo.enumerate_states(plan.n)
    d = do.descend(trace_oracle.pack(start), plan.n, hs, Js, plan.edge_i, plan.edge_j, plan.order, plan.class_ptr, 64)
    return plan, hs, Js, start, d


@pytest.mark.parametrize("seed", [12, 13])
def test_oracle_on_every_state_of_the_ring(seed):
    """All 4096 states at max_sweeps = 64: every returned row has no unstable spin (by the oracle's count and by the fields
    helper's, which shares no code with it); a second descent leaves it alone with sweeps = flips = 0; on the 2^-10 grid the
    float64 energy falls strictly for every row that flipped."""
    plan, hs, Js, start, d = _ring_descent(seed)
    assert d.bits.shape == (4096, 1) and d.bits.dtype == np.uint32 and (d.bits >> np.uint32(12) == 0).all()
    assert (d.unstable == 0).all() and (d.sweeps < 64).all()
    assert (fo.fields(d.bits, plan.n, hs, Js, plan.edge_i, plan.edge_j, 1.0).unstable == 0).all()
    again = do.descend(d.bits, plan.n, hs, Js, plan.edge_i, plan.edge_j, plan.order, plan.class_ptr, 64)
    assert np.array_equal(again.bits, d.bits) and not again.sweeps.any() and not again.flips.any() and not again.unstable.any()
    e0, e1 = do.energy(start, hs, Js, plan.edge_i, plan.edge_j), do.energy(d.s, hs, Js, plan.edge_i, plan.edge_j)
    moved = d.flips > 0
    assert moved.any() and (~moved).any()
    assert (e1[moved] < e0[moved]).all() and np.array_equal(d.s[~moved], start[~moved]) and (d.sweeps[~moved] == 0).all()
    assert ((d.sweeps > 0) == moved).all() and (d.flips >= d.sweeps).all() and (d.flips >= (d.s != start).sum(axis=1)).all()
    # the rows that did not move are exactly the start states without an unstable spin
    assert np.array_equal(~moved, fo.fields(trace_oracle.pack(start), plan.n, hs, Js, plan.edge_i, plan.edge_j, 1.0).unstable == 0)
    # cut off after one sweep: what is left unstable is what the fields helper counts on the returned rows
    cut = do.descend(trace_oracle.pack(start), plan.n, hs, Js, plan.edge_i, plan.edge_j, plan.order, plan.class_ptr, 1)
    assert (cut.sweeps <= 1).all() and (cut.unstable > 0).any() and (cut.unstable[cut.sweeps == 0] == 0).all()
    assert np.array_equal(cut.unstable, fo.fields(cut.bits, plan.n, hs, Js, plan.edge_i, plan.edge_j, 1.0).unstable)
    print(f"ring {seed}: {len(np.unique(d.bits))} minima, sweeps up to {d.sweeps.max()}, flips up to {d.flips.max()}; "
          f"after one sweep {int((cut.unstable > 0).sum())} rows still unstable")


def test_oracle_leaves_an_exact_zero_field_alone():
    """Two spins, one edge, J = 0.5, h_0 = 0.5.  With h_1 = 2 spin 1 rests at -1 and f_0 = 0.5 - 0.5 is exactly 0: spin 0 stays
    as it is, up or down.  With h_1 = -2 spin 1 goes up, f_0 becomes 1 and sends an up spin 0 down: two flips."""
    plan = graphs.build_plan(2, np.array([0], dtype=np.int64), np.array([1], dtype=np.int64))
    Js = np.array([0.5], np.float32)
    for bits in (0b00, 0b01):
        d = do.descend(np.array([[bits]], np.uint32), 2, np.array([0.5, 2.0], np.float32), Js, plan.edge_i, plan.edge_j, plan.order,
                       plan.class_ptr, 8)
        assert d.bits[0, 0] == bits and d.flips[0] == 0 and d.sweeps[0] == 0 and d.unstable[0] == 0
    d = do.descend(np.array([[0b01]], np.uint32), 2, np.array([0.5, -2.0], np.float32), Js, plan.edge_i, plan.edge_j, plan.order,
                   plan.class_ptr, 8)
    assert d.bits[0, 0] == 0b10 and d.flips[0] == 2 and d.unstable[0] == 0


# ------------------------------------------------------------------------------------------------ Minima
def _hand_built(T, shape=None):
    """T rows of the ring taken through the oracle from random starts (pad bits set in the start), as CPU tensors."""
    plan, hs, Js = _ring_fields()
    rng = np.random.default_rng(T)
    start = rng.integers(0, 2 ** 32, size=(T, 1), dtype=np.uint64).astype(np.uint32)
    d = do.descend(start, plan.n, hs, Js, plan.edge_i, plan.edge_j, plan.order, plan.class_ptr, 2)
    e0 = do.energy(trace_oracle.unpack(start, plan.n), hs, Js, plan.edge_i, plan.edge_j)
    e1 = do.energy(d.s, hs, Js, plan.edge_i, plan.edge_j)
    lead = shape or (T,)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    m = smp.Minima.from_outputs(t(start.view(np.int32)).view(*lead, 1), t(d.bits.view(np.int32)).view(*lead, 1), t(d.sweeps).view(lead),
                                t(d.flips).view(lead), t(d.unstable).view(lead), t(e0).view(lead), t(e1).view(lead), plan.n)
    return m, start, d, e0, e1


@pytest.mark.parametrize("T", [1, 5, 33])
def test_minima_properties_equal_the_numpy_restatement(T):
    for shape in [None] + ([(3, 11)] if T == 33 else []) + ([(1, 5)] if T == 5 else []):
        m, start, d, e0, e1 = _hand_built(T, shape)
        lead = shape or (T,)
        want = do.estimates(start, d.bits, d.sweeps, d.flips, d.unstable, e0, e1, 12)
        assert m.count == T and m.n == 12 and "Minima(" in repr(m)
        assert m.converged.dtype == torch.bool and np.array_equal(m.converged.numpy().reshape(-1), want["converged"])
        assert m.distance.dtype == torch.int32 and m.distance.shape == lead and np.array_equal(m.distance.numpy().reshape(-1), want["distance"])
        assert m.energy_drop.dtype == torch.float64 and np.array_equal(m.energy_drop.numpy().reshape(-1), want["energy_drop"])
        for name in ("converged_share", "mean_flips", "mean_sweeps", "basin_entropy"):
            got = getattr(m, name)
            assert torch.is_tensor(got) and got.dtype == torch.float64 and got.dim() == 0, name
            assert np.allclose(float(got), want[name], rtol=1e-12, atol=1e-15), (name, got, want[name])
        rows, counts, index = m.unique()
        wr, wc, wi = do.unique_minima(d.bits)
        assert rows.dtype == torch.int32 and np.array_equal(rows.numpy(), wr) and np.array_equal(counts.numpy(), wc)
        assert index.shape == lead and np.array_equal(index.numpy().reshape(-1), wi)
        assert np.array_equal(rows.numpy()[index.numpy().reshape(-1)], d.bits.view(np.int32))  # the index leads back to the rows
        assert (np.diff(counts.numpy()) <= 0).all() and int(counts.sum()) == T
        for k in (1, 2, 1000):
            lr, le, lc = m.lowest(k)
            eu = np.array([e1[wi == u][0] for u in range(len(wr))])
            pick = np.argsort(eu, kind="stable")[:k]
            assert np.array_equal(lr.numpy(), wr[pick]) and np.array_equal(le.numpy(), eu[pick]) and np.array_equal(lc.numpy(), wc[pick])
        for bad in (0, -1, 1.5, None, True):
            with pytest.raises(ValueError, match="k must"):
                m.lowest(bad)


def test_minima_unique_orders_by_multiplicity_then_by_the_words():
    """Hand-written rows, n = 40 (two words, eight pad bits): multiplicities 3, 2, 2, 1; the tie keeps the order of
    torch.unique(dim=0) -- signed words, first word first -- and the word 0x80000000 sorts as negative."""
    a, b, c, e = [5, 1], [-2 ** 31, 0], [5, 0], [7, 7]
    bits = torch.tensor([c, a, b, a, e, c, a, b], dtype=torch.int32)
    T = bits.shape[0]
    z = torch.zeros(T, dtype=torch.int32)
    energy = torch.tensor([-1.0, -3.0, -2.0, -3.0, -5.0, -1.0, -3.0, -2.0], dtype=torch.float64)
    start = bits.clone()
    start[:, 1] |= 0x7F000000  # pad bits set in the start only: they are no distance
    start[0, 0] ^= 0b1011      # three spins of row 0 differ
    start[4, 1] ^= 0x80        # spin 39 of row 4 differs
    m = smp.Minima.from_outputs(start, bits, z, z, z, energy + 1.0, energy, 40)
    rows, counts, index = m.unique()
    assert rows.tolist() == [a, b, c, e] and counts.tolist() == [3, 2, 2, 1] and index.tolist() == [2, 0, 1, 0, 3, 2, 0, 1]
    p = np.array([3, 2, 2, 1]) / 8.0
    assert abs(float(m.basin_entropy) + (p * np.log(p)).sum()) < 1e-15
    assert m.distance.tolist() == [3, 0, 0, 0, 1, 0, 0, 0]
    lr, le, lc = m.lowest(3)
    assert lr.tolist() == [e, a, b] and le.tolist() == [-5.0, -3.0, -2.0] and lc.tolist() == [1, 3, 2]
    assert float(m.converged_share) == 1.0 and m.energy_drop.tolist() == [1.0] * 8
    one = smp.Minima.from_outputs(start[:1], bits[:1], z[:1], z[:1], z[:1] + 2, energy[:1], energy[:1], 40)
    assert float(one.basin_entropy) == 0.0 and float(one.converged_share) == 0.0 and one.unique()[1].tolist() == [1]


def test_minima_from_outputs_validates():
    b, z, e = torch.zeros((5, 1), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.float64)
    smp.Minima.from_outputs(b, b, z, z, z, e, e, 12)
    for k, bad in ((0, b.long()), (0, b[:-1]), (0, None), (1, b.float()), (1, b[:0]), (1, b[0]), (1, torch.zeros((5, 2), dtype=torch.int32)),
                   (2, z.long()), (2, z[:-1]), (3, z[None]), (4, None), (5, e.float()), (5, e[:-1]), (6, z), (7, 0), (7, 33), (7, 12.0),
                   (7, True), (7, None)):
        args = [b, b, z, z, z, e, e, 12]
        args[k] = bad
        with pytest.raises(ValueError):
            smp.Minima.from_outputs(*args)
