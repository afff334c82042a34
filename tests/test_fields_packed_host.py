"""CPU-side checks of the local-field statistics of bit-packed rows ("DVG fields v1", ``dvg_grbm_fields_packed`` in
include/dvg.h): the symbols and profiler names, every argument error of the C entry point (before any HIP call, on host
stand-in pointers) and of the Python surface (before the library is touched), the workspace query, ``sampler.PseudoLikelihood``
on CPU tensors against its numpy restatement (``tests/fields_oracle.py``) to 1e-12, its gradient against torch autograd of the
textbook pseudo-likelihood, and what the residuals and the Rao-Blackwellised moments say on enumerated states and on CPU draws
of the unchanged oracle (``trace_oracle.trace``)."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_oracle as fo  # noqa: E402
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

NAME, QUERY = "dvg_grbm_fields_packed", "dvg_grbm_fields_packed_workspace_bytes"


# ------------------------------------------------------------------------------------------------ the symbols and their checks
def test_symbols_are_declared_bound_and_exported():
    support.assert_declared_bound_exported({NAME: "int", QUERY: "size_t"}, markers=["DVG fields v1"],
                                           kernels=["grbm_fields_packed_kernel", "grbm_fields_reduce_kernel"])


_stand_in = support.graph_stand_in


def _set_n(graph, n, n_edges=0):
    (ctypes.c_int32 * 2).from_buffer(graph)[:] = [n, n_edges]


OUT = ("log_pl", "unstable", "cond_sum", "cond_pair", "field_out")


def _call(g, lin, quad, bits, outs, *, prefactor=1.0, beta=1.0, rows=5, row_stride=2, groups=1, group_stride=0, accumulate=0, ws=None,
          ws_bytes=1 << 40):
    L = _lib.lib()
    rc = L.dvg_grbm_fields_packed(g, lin, quad, prefactor, -4.0, 4.0, -1.0, 1.0, beta, bits, rows, row_stride, groups, group_stride,
                                  *[outs.get(k) for k in OUT], accumulate, ws, ws_bytes, None)
    return rc, L.dvg_last_error()


def test_c_argument_validation_without_gpu():
    """Every error of the header's list, with its code (DVG_E_INVALID = -1, DVG_E_UNSUPPORTED = -4, DVG_E_WORKSPACE = -3)
    and a message that names the argument, on host stand-in pointers: nothing reaches HIP."""
    graph, g, p, _keep = _stand_in()
    every = {k: p for k in OUT}
    for k, word in enumerate((rb"\bg\b", rb"\blinear\b", rb"\bquadratic\b", rb"\bbits\b")):
        args = [g, p, p, p]
        args[k] = None
        rc, msg = _call(*args, every, ws=p)
        assert rc == -1 and re.search(word, msg) and b"null" in msg, (k, rc, msg)
    rc, msg = _call(g, p, p, p, {})
    assert rc == -1 and b"no output" in msg, (rc, msg)
    rc, msg = _call(g, p, p, p, dict(cond_sum=p))
    assert rc == -1 and b"cond_pair" in msg and b"cond_sum" in msg, (rc, msg)
    rc, msg = _call(g, p, p, p, dict(log_pl=p, cond_pair=p))
    assert rc == -1 and b"cond_pair" in msg and b"cond_sum" in msg, (rc, msg)
    rc, msg = _call(g, p, p, p, every, ws=None)
    assert rc == -1 and re.search(rb"\bws\b", msg) and b"null" in msg, (rc, msg)
    rc, msg = _call(g, p, p, p, every, ws=p + 8)
    assert rc == -1 and re.search(rb"\bws\b", msg) and b"aligned" in msg, (rc, msg)
    for name in ("rows", "groups"):
        for bad in (0, -1, -2 ** 40):
            rc, msg = _call(g, p, p, p, dict(log_pl=p), **{name: bad})
            assert rc == -1 and re.search(rb"\b" + name.encode() + rb"\b", msg), (name, bad, rc, msg)
    for bad in (1, 0, -1, -2 ** 40):  # n = 64: two words a row
        rc, msg = _call(g, p, p, p, dict(unstable=p), row_stride=bad)
        assert rc == -1 and b"row_stride" in msg, (bad, rc, msg)
    for bad in (-1, -2 ** 40):
        rc, msg = _call(g, p, p, p, dict(field_out=p), groups=3, group_stride=bad)
        assert rc == -1 and b"group_stride" in msg, (bad, rc, msg)
    for bad in (float("nan"), float("inf"), -float("inf")):
        rc, msg = _call(g, p, p, p, dict(log_pl=p), prefactor=bad)
        assert rc == -1 and b"prefactor" in msg, (bad, rc, msg)
    for bad in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-30):
        rc, msg = _call(g, p, p, p, dict(log_pl=p), beta=bad)
        assert rc == -1 and b"beta" in msg, (bad, rc, msg)
    _set_n(graph, 65)  # a row stride is measured against W = ceil(n / 32): n = 65 needs three words
    rc, msg = _call(g, p, p, p, dict(log_pl=p), row_stride=2)
    assert rc == -1 and b"row_stride" in msg, (rc, msg)
    _set_n(graph, 64)
    for rows, groups in ((2 ** 31, 2 ** 31), (2 ** 62, 1), (1, 2 ** 62), (2 ** 63 - 1, 2 ** 63 - 1)):
        rc, msg = _call(g, p, p, p, dict(log_pl=p), rows=rows, groups=groups)
        assert rc == -4 and b"groups" in msg and b"rows" in msg and b"2^62" in msg, (rows, groups, rc, msg)
    for n, row_stride in ((8193, 257), (2 ** 31 - 1, 2 ** 26)):
        _set_n(graph, n)
        rc, msg = _call(g, p, p, p, dict(log_pl=p), row_stride=row_stride)
        assert rc == -4 and re.search(rb"\bn=", msg) and b"8192" in msg and b"LDS" in msg, (n, rc, msg)
    # a short workspace: one byte below the query, pooled sums asked for
    _set_n(graph, 64, 100)
    need = _lib.lib().dvg_grbm_fields_packed_workspace_bytes(g, 5, 1)
    assert need == (64 + 200) * 8
    rc, msg = _call(g, p, p, p, every, ws=p, ws_bytes=need - 1)
    assert rc == -3 and b"ws_bytes" in msg, (rc, msg)
    rc, msg = _call(g, p, p, p, every, ws=p, ws_bytes=0)
    assert rc == -3 and b"ws_bytes" in msg, (rc, msg)


def test_workspace_query_is_monotone_and_zero_for_rejected_arguments():
    graph, g, _p, _keep = _stand_in(77, 1000)
    q = _lib.lib().dvg_grbm_fields_packed_workspace_bytes
    per_slab = (77 + 2000) * 8
    assert q(g, 1, 1) == per_slab and q(g, 64, 1) == per_slab and q(g, 65, 1) == 2 * per_slab and q(g, 7, 41) == 5 * per_slab
    last = 0
    for rows in (1, 2, 63, 64, 65, 1000, 32768, 32769, 40000, 10 ** 6, 2 ** 40):
        now = q(g, rows, 1)
        assert now >= last > -1 and now > 0 and q(g, 1, rows) == now, rows
        last = now
    assert last == 512 * per_slab  # never more than the fixed number of slabs
    for rows, groups in ((0, 1), (1, 0), (-5, 1), (2 ** 62, 1), (2 ** 31, 2 ** 31)):
        assert q(g, rows, groups) == 0, (rows, groups)
    assert q(None, 5, 1) == 0
    for n in (0, -1, 8193):
        _set_n(graph, n, 1000)
        assert q(g, 5, 1) == 0, n
    _set_n(graph, 8192, 0)
    assert q(g, 5, 1) == 8192 * 8


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
    call = lambda b=flat, l=lin, q=quad, **kw: F.grbm_fields_packed(b, gh, l, q, **{"beta": 1.0, **kw})  # noqa: E731,E741
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
    with pytest.raises(_lib.DvgError, match="bits: a row stride"):
        call(torch.zeros((30,), dtype=torch.int32).as_strided((2, 4, 3), (12, 2, 1)))
    for bad in (lin.double(), lin[:-1], torch.zeros(plan.n + 1), lin.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\blinear must"):
            call(l=bad)
    for bad in (quad.double(), quad[:-1], quad.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\bquadratic must"):
            call(q=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="prefactor"):
            call(prefactor=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.5, "1", None, True):
        with pytest.raises(ValueError, match="beta"):
            call(beta=bad)
    with pytest.raises(TypeError):
        F.grbm_fields_packed(flat, gh, lin, quad)  # beta has no default
    for bad in ((1.0,), (1.0, 2.0, 3.0), 4.0, "ab", (float("nan"), 1.0), (None, 1.0), (True, 2.0)):
        with pytest.raises(ValueError, match="linear_range"):
            call(linear_range=bad)
        with pytest.raises(ValueError, match="quadratic_range"):
            call(quadratic_range=bad)
    for name in ("log_pl", "unstable", "conditional", "fields"):
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match=name):
                call(**{name: bad})
    with pytest.raises(ValueError, match="no output"):
        call(log_pl=False, unstable=False, conditional=False, fields=False)
    cs, cp = torch.zeros(plan.n, dtype=torch.float64), torch.zeros(plan.n_edges, dtype=torch.float64)
    with pytest.raises(_lib.DvgError, match="out"):
        call(out=(cs, cp), conditional=False)
    for bad in (cs, (cs,), (cs, cp, cp), (cs.float(), cp), (cs, cp[:-1]), (cs[:-1], cp), (cs, cp.long()), (None, cp), (cs, None),
                (torch.zeros(2 * plan.n, dtype=torch.float64)[::2], cp)):
        with pytest.raises(_lib.DvgError, match="out"):
            call(out=bad)
    for ok in (flat, flat[::2], flat[:1], trace, trace[:, 1:], trace[::2], trace[:, ::3], trace[:1].expand(3, 6, 3)):
        with pytest.raises(_lib.DvgError, match="GPU"):  # valid arguments on CPU tensors: the HIP path has no CPU fallback
            call(ok, prefactor=0.3, beta=0, linear_range=(-4, 4), quadratic_range=(-1.0, float("inf")), fields=True, out=(cs, cp))


def test_trace_and_model_methods_check_before_the_library(untouched):
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    gh = _Handle(_ring_plan())
    lin, quad = torch.zeros(12), torch.zeros(12)
    t = smp.Trace(torch.zeros((3, 10, 1), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    with pytest.raises(_lib.DvgError, match="GPU"):
        t.pseudo_likelihood(gh, lin, quad, beta=0.5)
    with pytest.raises(_lib.DvgError, match="GPU"):
        t.pseudo_likelihood(gh, lin, quad, beta=0.5, prefactor=0.5, linear_range=(-4, 4), quadratic_range=(-1, 1))
    with pytest.raises(_lib.DvgError, match=r"\blinear must"):
        t.pseudo_likelihood(gh, lin[:-1], quad, beta=0.5)
    with pytest.raises(ValueError, match="beta"):
        t.pseudo_likelihood(gh, lin, quad, beta=-1.0)
    with pytest.raises(TypeError):
        t.pseudo_likelihood(gh, lin, quad)
    wrong = smp.Trace(torch.zeros((3, 10, 2), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    with pytest.raises(_lib.DvgError, match=r"\bbits must"):
        wrong.pseudo_likelihood(gh, lin, quad, beta=0.5)
    grbm = GraphRestrictedBoltzmannMachine(list(range(12)), [(i, (i + 1) % 12) for i in range(12)])
    for bad in (torch.zeros((4, 1), dtype=torch.int32), torch.ones((4, 12)), np.zeros((4, 1), dtype=np.int32), None):
        with pytest.raises(_lib.DvgError, match="GPU"):
            grbm.pseudo_likelihood(bad, beta=0.5, prefactor=1.0)
        with pytest.raises(_lib.DvgError, match="GPU"):
            grbm.pseudo_likelihood_grad(bad, beta=0.5, prefactor=1.0)


# ------------------------------------------------------------------------------------------------ PseudoLikelihood
def _ring_fields(prefactor=1.0, h_range=None, j_range=None, scale=1.0):
    """The 12-spin ring with (h, J) on the 2^-10 grid."""
    plan = _ring_plan()
    rng = np.random.default_rng(12)
    h = (scale * rng.integers(-1024, 1025, plan.n) / 1024.0).astype(np.float32)
    J = (scale * rng.integers(-1024, 1025, plan.n_edges) / 1024.0).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, prefactor, h_range, j_range)
    return plan, h, J, hs, Js


def _pl_of(o, plan, beta, shape=None):
    """``PseudoLikelihood`` on CPU tensors from the helper's outputs and the exact integer sums of the same rows."""
    spin_sum, pair_sum = trace_oracle.moments(o.s, plan.edge_i, plan.edge_j)
    lp, un = torch.from_numpy(o.log_pl), torch.from_numpy(o.unstable)
    if shape is not None:
        lp, un = lp.view(shape), un.view(shape)
    return smp.PseudoLikelihood.from_outputs(lp, un, torch.from_numpy(o.cond_sum), torch.from_numpy(o.cond_pair),
                                             torch.from_numpy(spin_sum), torch.from_numpy(pair_sum), beta), spin_sum, pair_sum


@pytest.mark.parametrize("T", [1, 5, 33])
def test_properties_equal_the_numpy_restatement(T):
    plan, _h, _J, hs, Js = _ring_fields()
    rng = np.random.default_rng(T)
    bits = rng.integers(0, 2 ** 32, size=(T, 1), dtype=np.uint64).astype(np.uint32)
    o = fo.fields(bits, plan.n, hs, Js, plan.edge_i, plan.edge_j, 0.7)
    shapes = [None] + ([(3, 11)] if T == 33 else []) + ([(1, 5)] if T == 5 else [])
    for shape in shapes:
        pl, spin_sum, pair_sum = _pl_of(o, plan, 0.7, shape)
        want = fo.estimates(o.log_pl.reshape(shape) if shape else o.log_pl, o.unstable, o.cond_sum, o.cond_pair, spin_sum, pair_sum)
        assert pl.count == T and pl.n == 12 and "PseudoLikelihood(" in repr(pl)
        for name, value in want.items():
            got = getattr(pl, name)
            assert torch.is_tensor(got) and got.dtype == torch.float64 and not got.is_cuda, name
            assert np.allclose(got.numpy(), value, rtol=1e-12, atol=1e-12, equal_nan=True), (name, got, value)
        if T == 1 or shape == (1, 5):
            assert np.isnan(float(pl.std_err))
    # the definitions by value on one row: all spins up, no couplings, h > 0 -> every spin unstable, m = -tanh(beta h)
    hs1, Js0 = np.full(12, 0.5, np.float32), np.zeros(12, np.float32)
    o = fo.fields(np.array([[0xFFF]], np.uint32), 12, hs1, Js0, plan.edge_i, plan.edge_j, 1.0)
    assert o.unstable[0] == 12 and np.allclose(o.m, -np.tanh(0.5), rtol=1e-15) and np.allclose(o.log_pl, 12 * np.log(1 / (1 + np.e)), rtol=1e-14)
    pl, _s, _p = _pl_of(o, plan, 1.0)
    assert float(pl.local_minimum_share) == 0.0 and np.allclose(pl.residual_linear.numpy(), 1.0 + np.tanh(0.5))


def test_from_outputs_validates():
    lp, un = torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.int32)
    cs, cp = torch.zeros(12, dtype=torch.float64), torch.zeros(12, dtype=torch.float64)
    ss, ps = torch.zeros(12, dtype=torch.int64), torch.zeros(12, dtype=torch.int64)
    smp.PseudoLikelihood.from_outputs(lp, un, cs, cp, ss, ps, 0.5)
    for k, bad in ((0, lp.float()), (0, lp[:0]), (0, lp[None, None]), (0, None), (1, un.long()), (1, un[:-1]), (2, cs.float()), (2, cs[None]),
                   (3, cp.long()), (4, ss.double()), (4, ss[:-1]), (5, ps[:-1]), (5, ps.double()), (6, -1.0), (6, float("nan")), (6, "1"),
                   (6, True)):
        args = [lp, un, cs, cp, ss, ps, 0.5]
        args[k] = bad
        with pytest.raises(ValueError):
            smp.PseudoLikelihood.from_outputs(*args)


def test_grad_equals_autograd_of_the_textbook_pseudo_likelihood():
    """The 12-spin ring, (h, J) on the 2^-10 grid, prefactor 0.5, beta 0.5: every float32 sum and z is exact, so the float64
    textbook form -- mean_r sum_i -softplus(2 beta s_i f_i), f from torch.clamp(prefactor (h, J)) -- and the kernel's
    definition are the same function and their gradients agree to 1e-12.  The linear clamp (+-0.25) and the quadratic clamp
    (+-0.375) are both active."""
    beta, prefactor, h_range, j_range = 0.5, 0.5, (-0.25, 0.25), (-0.375, 0.375)
    plan, h, J, hs, Js = _ring_fields(prefactor, h_range, j_range)
    assert 0 < (np.abs(hs) == 0.25).sum() < 12 and 0 < (np.abs(Js) == 0.375).sum() < 12
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 12, size=(33, 1), dtype=np.uint64).astype(np.uint32)
    o = fo.fields(bits, plan.n, hs, Js, plan.edge_i, plan.edge_j, beta)
    pl, _s, _p = _pl_of(o, plan, beta)
    gl, gq = pl.grad(prefactor, torch.from_numpy(h), torch.from_numpy(J), h_range, j_range)
    ht, Jt = torch.tensor(h, dtype=torch.float64, requires_grad=True), torch.tensor(J, dtype=torch.float64, requires_grad=True)
    hc, Jc = torch.clamp(prefactor * ht, *h_range), torch.clamp(prefactor * Jt, *j_range)
    s = torch.from_numpy(o.s.astype(np.float64))
    ei, ej = torch.from_numpy(np.asarray(plan.edge_i, np.int64)), torch.from_numpy(np.asarray(plan.edge_j, np.int64))
    f = hc[None, :].expand(33, 12).clone()
    f = f.index_add(1, ei, s[:, ej] * Jc[None, :]).index_add(1, ej, s[:, ei] * Jc[None, :])
    assert np.array_equal(f.detach().numpy(), o.f.astype(np.float64))  # (exact: the two are the same numbers)
    mean = (-torch.nn.functional.softplus(2.0 * beta * s * f)).sum(1).mean()
    mean.backward()
    assert abs(float(mean.detach()) - float(pl.mean)) <= 1e-12 * abs(float(mean.detach()))
    assert gl.shape == ht.shape and gq.shape == Jt.shape and gl.dtype == torch.float64
    assert np.allclose(gl.numpy(), ht.grad.numpy(), rtol=1e-12, atol=1e-12) and np.allclose(gq.numpy(), Jt.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert (gl.numpy()[np.abs(hs) == 0.25] == 0).all() and (gl.numpy()[np.abs(hs) < 0.25] != 0).all()  # the clamp's mask
    assert (gq.numpy()[np.abs(prefactor * J) > 0.375] == 0).all()
    gl0, _gq0 = pl.grad(prefactor, torch.from_numpy(h), torch.from_numpy(J))  # no ranges: no mask
    assert (gl0.numpy() != 0).all()
    for bad in (float("nan"), "1", None, True):
        with pytest.raises(ValueError, match="prefactor"):
            pl.grad(bad, torch.from_numpy(h), torch.from_numpy(J))
    with pytest.raises(ValueError, match="linear"):
        pl.grad(1.0, torch.from_numpy(h[:-1]), torch.from_numpy(J))


def test_residuals_have_zero_mean_under_the_model():
    """By enumeration of the ring's 2^12 states: sum_s p(s) (s_i - m_i(s)) = 0 and sum_s p(s) (2 s_i s_j - m_i s_j - m_j s_i) = 0,
    to 1e-12 -- the pseudo-likelihood's score has zero mean at the model's own parameters."""
    for beta, prefactor in ((0.5, 1.0), (1.0, 0.5)):
        plan, _h, _J, hs, Js = _ring_fields(prefactor)
        s = fo.enumerate_states(plan.n)
        o = fo.fields(trace_oracle.pack(s), plan.n, hs, Js, plan.edge_i, plan.edge_j, beta)
        assert np.array_equal(o.s, s)
        p = fo.boltzmann(s, hs, Js, plan.edge_i, plan.edge_j, beta)
        sd, ei, ej = s.astype(np.float64), np.asarray(plan.edge_i), np.asarray(plan.edge_j)
        lin = p @ (sd - o.m)
        quad = p @ (2.0 * sd[:, ei] * sd[:, ej] - o.m[:, ei] * sd[:, ej] - o.m[:, ej] * sd[:, ei])
        print(f"beta {beta}: largest |mean residual| {np.abs(lin).max():.2e} (spins), {np.abs(quad).max():.2e} (edges)")
        assert np.abs(lin).max() <= 1e-12 and np.abs(quad).max() <= 1e-12
        assert np.abs(p @ np.abs(sd - o.m)).min() > 1e-3  # (teeth: the residuals themselves are not small)


RING_SEED = 20261020


@functools.lru_cache(maxsize=None)
def _ring_draw(beta=0.8):
    """The ring of ``test_energy_packed_host.py``: 64 chains, 250 sweeps, burn_in 50, thin 2 -> 100 records a chain."""
    plan = _ring_plan()
    rng = np.random.default_rng(12)
    h = (0.5 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = rng.uniform(-1, 1, plan.n_edges).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 1.0, (-4, 4), (-1, 1))
    ids = np.arange(64, dtype=np.uint32) + 11
    tr = trace_oracle.trace(plan, hs, Js, beta, ids, RING_SEED ^ 0x74726163, 0, 250, burn_in=50, thin=2)
    assert tr.bits.shape == (64, 100, 1)
    return plan, hs, Js, tr.bits, fo.fields(tr.bits, plan.n, hs, Js, plan.edge_i, plan.edge_j, beta)


def test_statistics_of_cpu_draws_of_the_oracle():
    """64 chains x 100 records at beta 0.8.  The chains are independent, so the standard error of a pooled mean is the
    standard deviation of the 64 chain means over 8.  (a) The mean residual of every spin and edge lies within 6 such
    standard errors of 0.  (b) The Rao-Blackwellised ``mean_spin`` lies within 6 standard errors of the enumerated <s_i>.
    (c) Its between-chain variance, summed over the spins, is not above that of the plain mean of the same records -- summed,
    because a variance estimated from 64 chains is itself uncertain by sqrt(2 / 63) = 18 %, too much to order two variances
    spin by spin."""
    beta = 0.8
    plan, hs, Js, bits, o = _ring_draw(beta)
    C, M, n = 64, 100, plan.n
    sd, m = o.s.astype(np.float64).reshape(C, M, n), o.m.reshape(C, M, n)
    ei, ej = np.asarray(plan.edge_i), np.asarray(plan.edge_j)
    se = lambda x: x.std(axis=0, ddof=1) / np.sqrt(C)  # noqa: E731
    r_lin = (sd - m).mean(axis=1)
    r_quad = (2.0 * sd[..., ei] * sd[..., ej] - m[..., ei] * sd[..., ej] - m[..., ej] * sd[..., ei]).mean(axis=1)
    z_lin, z_quad = r_lin.mean(axis=0) / se(r_lin), r_quad.mean(axis=0) / se(r_quad)
    exact_spin, _exact_pair = trace_oracle.exact_moments(n, hs, Js, plan.edge_i, plan.edge_j, beta)
    rb, plain = m.mean(axis=1), sd.mean(axis=1)
    z_rb = (rb.mean(axis=0) - exact_spin) / se(rb)
    var_rb, var_plain = rb.var(axis=0, ddof=1), plain.var(axis=0, ddof=1)
    print(f"residual z: spins up to {np.abs(z_lin).max():.2f}, edges up to {np.abs(z_quad).max():.2f}; Rao-Blackwellised mean_spin z up to "
          f"{np.abs(z_rb).max():.2f}; between-chain variance {var_rb.sum():.4e} (Rao-Blackwellised) against {var_plain.sum():.4e} (plain), "
          f"per spin ratio {np.round(var_rb / var_plain, 2)}")
    assert np.abs(z_lin).max() <= 6.0 and np.abs(z_quad).max() <= 6.0
    assert np.abs(z_rb).max() <= 6.0
    assert var_rb.sum() <= var_plain.sum()
    # and PseudoLikelihood says the same from the pooled sums
    pl, _s, _p = _pl_of(o, plan, beta, (C, M))
    assert np.allclose(pl.mean_spin.numpy(), rb.mean(axis=0), rtol=1e-12, atol=1e-14)
    assert np.allclose(pl.residual_linear.numpy() / (C * M), r_lin.mean(axis=0), rtol=1e-10, atol=1e-13)
    assert np.allclose(pl.residual_quadratic.numpy() / (C * M), r_quad.mean(axis=0), rtol=1e-10, atol=1e-13)
    assert float(pl.std_err) > 0 and 0.0 <= float(pl.local_minimum_share) <= 1.0
