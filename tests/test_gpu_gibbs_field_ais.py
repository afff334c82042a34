"""GPU parity of the weighed per-chain-field draw (``dvg_gibbs_sample_fields_ais``, "DVG field AIS v1": the per-chain-field draw
along a path in (beta, field strength), with the AIS draw's log weight and energy per chain) against its definition in
``tests/field_ais_oracle.py``, against the two draws it joins, and of the Python surface built on it.

Spins: equal to the helper's, bit for bit.  Weights and energies: the bound of ``tests/test_gpu_gibbs_ais.py``, with the helper's
own A and N.  The kernel and the helper add the same energy addends -- the n start addends, the n S updates and, with a table of
strengths, the n S row steps, all exact, of absolute sum A -- in two orders, so |energy - helper| <= 4 N 2^-53 A as there.  The
weight is -sum_k [dbeta_k E^(k) + beta_k d_k]: 2 S products, each of a beta (difference) with a sum of those addends, so the unit
4 N 2^-53 A is scaled by sum_k |dbeta_k| as in that file, plus sum_k beta_k where there is a table of strengths (without one d_k
is identically 0 and not computed); the 2 S - 1 additions of the products fit in as there (N counts the 2 S multiply-adds).

Graphs: the builders of ``tests/test_gpu_gibbs_conditional.py``; conventions: those of ``tests/test_gpu_gibbs_fields.py`` (its
PARITY rows, 3 sweeps from sweep 5, a nonzero first chain id) with the guard row / element of the AIS file behind the last chain."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_oracle  # noqa: E402
import field_ais_oracle as fao  # noqa: E402
import test_gpu_gibbs_conditional as cond  # noqa: E402  (the graph builders)
from image_generation_amd import _lib, dev, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
GUARD_STATE, GUARD_OUT, GUARD_W, GUARD_E = 55, 7.0, -3.5, 11.25


def _plan(name):
    return cond._random_plan(77, 0.35) if name == "random77" else cond._solver_plan("zephyr", int(name[len("zephyr"):]))[0]


def _start(rng, C, n):
    return np.where(rng.uniform(size=(C, n)) < 0.5, -1, 1).astype(np.int8)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


class _Draw:
    """dvg_gibbs_sample_fields_ais, and the two draws it joins, on one graph and one (h, J); ``h_range``: the linear range."""

    def __init__(self, plan, h, J, prefactor, h_range=(-4.0, 4.0)):
        self.plan, self.prefactor, self.h_range = plan, float(prefactor), h_range
        self.gh = smp.GraphHandle(plan, "cuda")
        self.lin, self.quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()

    def _head(self):
        return (self.gh.ptr, self.lin.data_ptr(), self.quad.data_ptr(), self.prefactor, self.h_range[0], self.h_range[1], -1.0, 1.0)

    def buffers(self, start):
        """``state``, ``samples_out`` with a guard row and ``log_weight_out``, ``energy_out`` with a guard element behind the last
        chain; ``start``: (C, n) int8."""
        C, n = start.shape
        state = torch.full((C + 1, n), GUARD_STATE, dtype=torch.int8, device="cuda")
        state[:C] = torch.from_numpy(start).cuda()
        out = torch.full((C + 1, n), GUARD_OUT, dtype=torch.float32, device="cuda")
        log_w = torch.full((C + 1,), GUARD_W, dtype=torch.float64, device="cuda")
        energy = torch.full((C + 1,), GUARD_E, dtype=torch.float64, device="cuda")
        return state, out, log_w, energy

    def raw(self, bufs, fields, stride, R, betas, beta_stride, beta_from, scales, scale_stride, scale_from, id0, seed, sweep0, sweeps, init,
            C=None, dyn=None, with_w=True, with_e=True):
        state, out, log_w, energy = bufs
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return _lib.lib().dvg_gibbs_sample_fields_ais(
            *self._head(), ptr(betas), beta_stride, float(beta_from), ptr(scales), scale_stride, float(scale_from), state.data_ptr(),
            int(state.shape[0]) - 1 if C is None else C, id0, seed, sweep0, sweeps, init, ptr(fields), stride, R, out.data_ptr(),
            log_w.data_ptr() if with_w else None, energy.data_ptr() if with_e else None, dyn, _lib.stream_ptr())

    def fields_ais(self, bufs, fields, betas, scales, id0, seed, sweep0, init, beta_from=0.0, scale_from=1.0, R=1, **kw):
        """``fields`` (rows, n) or (n,), ``betas`` and ``scales`` (S,) or (C, S) (``scales`` may be None): float32 arrays."""
        f, b, s = _dev(fields), _dev(betas), _dev(scales)
        S = int(b.shape[-1])
        rc = self.raw(bufs, f, self.plan.n if f.dim() == 2 else 0, R, b, S if b.dim() == 2 else 0, beta_from, s,
                      S if s is not None and s.dim() == 2 else 0, scale_from, id0, seed, sweep0, S, init, **kw)
        _lib.check(rc, "dvg_gibbs_sample_fields_ais")
        torch.cuda.synchronize()

    def field(self, bufs, fields, beta, id0, seed, sweep0, sweeps, init):
        state, out = bufs[0], bufs[1]
        f = _dev(fields)
        _lib.check(_lib.lib().dvg_gibbs_sample_fields(*self._head(), float(beta), state.data_ptr(), int(state.shape[0]) - 1, id0, seed, sweep0,
                                                      sweeps, init, f.data_ptr(), self.plan.n if f.dim() == 2 else 0, out.data_ptr(), None,
                                                      _lib.stream_ptr()), "dvg_gibbs_sample_fields")
        torch.cuda.synchronize()

    def ais(self, bufs, betas, beta_from, id0, seed, sweep0, init):
        state, out, log_w, energy = bufs
        b = _dev(betas)
        S = int(b.shape[-1])
        _lib.check(_lib.lib().dvg_gibbs_sample_ais(*self._head(), b.data_ptr(), S if b.dim() == 2 else 0, float(beta_from), state.data_ptr(),
                                                   int(state.shape[0]) - 1, id0, seed, sweep0, S, init, out.data_ptr(), log_w.data_ptr(),
                                                   energy.data_ptr(), None, _lib.stream_ptr()), "dvg_gibbs_sample_ais")
        torch.cuda.synchronize()


def _weight_scale(betas, scales, beta_from, C):
    """What the unit 4 N 2^-53 A of a weight is scaled by (the module docstring)."""
    table = np.broadcast_to(np.asarray(betas, dtype=np.float32), (C, np.shape(betas)[-1])).astype(np.float64)
    dbeta = np.abs(np.diff(np.concatenate([np.full((C, 1), np.float64(np.float32(beta_from))), table], axis=1), axis=1)).sum(axis=1)
    return dbeta + (table.sum(axis=1) if scales is not None else 0.0)


def _check(bufs, want, betas, scales, beta_from, where, spins=True):
    """Every spin of ``state`` and ``samples_out`` equals the helper's; weights and energies within the float64 bound; the guards
    are untouched."""
    state, out, log_w, energy = bufs
    C = want.spins.shape[0]
    got, got_state = out.cpu().numpy(), state.cpu().numpy()
    got_w, got_e = log_w.cpu().numpy(), energy.cpu().numpy()
    assert (got_state[C] == GUARD_STATE).all() and (got[C] == GUARD_OUT).all(), f"written past the last chain ({where})"
    assert got_w[C] == GUARD_W and got_e[C] == GUARD_E, f"weights or energies written past the last chain ({where})"
    if spins:
        mism = int((got[:C] != want.spins.astype(np.float32)).sum())
        assert mism == 0, f"{mism} spin mismatches in samples_out ({where})"
        assert np.array_equal(got_state[:C], want.spins), f"state differs from the helper ({where})"
    unit = 4.0 * want.N * 2.0 ** -53 * want.A
    bound_w = unit * _weight_scale(betas, scales, beta_from, C)
    err_w, err_e = np.abs(got_w[:C] - want.log_w), np.abs(got_e[:C] - want.energy)
    print(f"{where}: |log_w| up to {np.abs(want.log_w).max():.4g}, worst error {err_w.max():.3e} (its bound {bound_w[err_w.argmax()]:.3e}); "
          f"|energy| up to {np.abs(want.energy).max():.4g}, worst error {err_e.max():.3e} (its bound {unit[err_e.argmax()]:.3e})")
    assert np.isfinite(got_w[:C]).all() and (err_w <= bound_w).all(), (where, err_w.max(), bound_w.min())
    assert np.isfinite(got_e[:C]).all() and (err_e <= unit).all(), (where, err_e.max(), unit.min())


# ------------------------------------------------------------------------------------------------ bit parity with the helper
# the rows of tests/test_gpu_gibbs_fields.py: graph, chains, (LPC, WAVES) of the plan, h scale, J scale, prefactor, linear range, beta
PARITY = [
    ("random77", 19, (16, 1), 0.5, 2.0, 0.3, (-0.35, 0.35), 1.5),
    ("zephyr128", 5, (32, 1), 0.05, 5.0, 0.05, (-0.06, 0.06), 20.0),
    ("zephyr512", 9, (64, 4), 0.05, 5.0, 0.05, (-0.06, 0.06), 20.0),
    ("zephyr1024", 5, (64, 4), 0.05, 5.0, 0.05, (-0.06, 0.06), 20.0),
]
SWEEP0, SWEEPS = 5, 3


def _tables(variant, C, beta, rng):
    shared = np.linspace(0.0, beta, SWEEPS + 1)[1:].astype(np.float32)
    if variant == "shared-betas":
        return shared, None
    if variant == "shared-both":
        return shared, np.array([0.25, 1.5, 0.75], dtype=np.float32)
    return rng.uniform(0.0, 2.0 * beta, (C, SWEEPS)).astype(np.float32), rng.uniform(0.0, 1.5, (C, SWEEPS)).astype(np.float32)


@pytest.mark.parametrize("variant", ["shared-betas", "shared-both", "per-chain"])
@pytest.mark.parametrize("init", [1, 0])
@pytest.mark.parametrize("name,C,form,h_scale,j_scale,prefactor,h_range,beta", PARITY, ids=[p[0] for p in PARITY])
def test_fields_ais_bit_exact(name, C, form, h_scale, j_scale, prefactor, h_range, beta, init, variant):
    """3 sweeps from sweep 5, N(0, 1) fields per chain, a prefactor that is not 1 and a linear range that clamps some row entries
    at some strengths and not at others; fresh chains (the INIT stream at sweep 5, beta_from = 0) and a given start (beta_from =
    0.3); scale_from = 0.5."""
    plan = _plan(name)
    n, id0 = plan.n, 1000
    p = dev.gibbs_draw_plan(plan, C, "field_weigh")
    assert p["form"] == "rolled" and p["params"] == dict(LPC=form[0], WAVES=form[1]), p
    rng = np.random.default_rng(n + C)
    h, J = cond._params(plan, rng, h_scale, j_scale)
    fields = rng.standard_normal((C, n)).astype(np.float32)
    edge = lambda lam: np.isin(fao.chain_rows(h, fields, np.full(C, lam, np.float32), prefactor, h_range),  # noqa: E731
                               np.asarray(h_range, dtype=np.float32))
    assert 0.05 < edge(1.5).mean() < 0.95 and 0.05 < edge(1.0).mean() < 0.95 and 0.05 < (edge(1.5) != edge(0.25)).mean()
    Js = gibbs.scaled_fields(h, J, prefactor, None, (-1, 1))[1]
    ids = np.arange(C, dtype=np.uint32) + id0
    given = _start(rng, C, n)
    betas, scales = _tables(variant, C, beta, rng)
    beta_from = 0.0 if init else 0.3
    want = fao.field_ais(plan, h, fields, prefactor, h_range, Js, betas, scales, ids, SEED, SWEEP0, start=None if init else given,
                         beta_from=beta_from, scale_from=0.5)
    d = _Draw(plan, h, J, prefactor, h_range)
    bufs = d.buffers(given)
    d.fields_ais(bufs, fields, betas, scales, id0, SEED, SWEEP0, init, beta_from=beta_from, scale_from=0.5)
    _check(bufs, want, betas, scales, beta_from, f"{name} {variant} init={init}")
    assert not np.array_equal(want.spins, given) and np.abs(want.log_w).min() > 0


# ------------------------------------------------------------------------------------------------ identities, bit for bit
IDENTITY = [("zephyr128", 1025, 0.05, 5.0, 0.05, (-0.06, 0.06), 20.0), ("random77", 19, 0.5, 2.0, 0.3, (-0.35, 0.35), 1.5)]


def _identity(name, C, h_scale, j_scale, prefactor, h_range, beta, seed_off):
    plan = _plan(name)
    rng = np.random.default_rng(plan.n + seed_off)
    h, J = cond._params(plan, rng, h_scale, j_scale)
    return plan, rng, h, J, _Draw(plan, h, J, prefactor, h_range), _start(rng, C, plan.n)


def _equal(a, b, what=(0, 1, 2, 3)):
    return all(torch.equal(a[k], b[k]) for k in what)


@pytest.mark.parametrize("init", [1, 0])
@pytest.mark.parametrize("name,C,h_scale,j_scale,prefactor,h_range,beta", IDENTITY, ids=[p[0] for p in IDENTITY])
def test_no_scales_and_a_constant_beta_are_the_field_draw(name, C, h_scale, j_scale, prefactor, h_range, beta, init):
    """Zephyr 128 x 1025 chains: 129 workgroups of 8, the last one with a single chain.  Spins and state are
    dvg_gibbs_sample_fields', log_w == 0 exactly.  (init = 1 needs beta_from = 0: there the first weight step is -beta E_0, and
    only the spins are compared.)"""
    plan, rng, h, J, d, start = _identity(name, C, h_scale, j_scale, prefactor, h_range, beta, 1)
    if name == "zephyr128":
        assert dev.gibbs_draw_plan(plan, C, "field_weigh")["chains_per_workgroup"] == 8
    fields = rng.standard_normal((C, plan.n)).astype(np.float32)
    want = d.buffers(start)
    d.field(want, fields, beta, 11, SEED, 3, 5, init)
    for table in (np.full(5, beta, np.float32), np.full((C, 5), beta, np.float32)):
        got = d.buffers(start)
        d.fields_ais(got, fields, table, None, 11, SEED, 3, init, beta_from=0.0 if init else beta, scale_from=0.25)
        assert _equal(got, want, (0, 1)), table.shape
        assert init or bool((got[2][:C] == 0.0).all())
        assert got[2][C].item() == GUARD_W and got[3][C].item() == GUARD_E and bool(torch.isfinite(got[3][:C]).all())
    assert not torch.equal(want[0][:C], torch.from_numpy(start).cuda())


@pytest.mark.parametrize("name,C,h_scale,j_scale,prefactor,h_range,beta", IDENTITY, ids=[p[0] for p in IDENTITY])
def test_zero_fields_are_the_ais_draw(name, C, h_scale, j_scale, prefactor, h_range, beta):
    """Spins: dvg_gibbs_sample_ais' (GPU against GPU; on Zephyr 128 that draw runs the lane-major form).  Weights and energies:
    the AIS helper's, which the field-AIS helper reproduces exactly at zero fields (tests/test_gibbs_field_ais_host.py), within the
    bound.  With a table of strengths as well: zero fields times anything."""
    plan, rng, h, J, d, start = _identity(name, C, h_scale, j_scale, prefactor, h_range, beta, 2)
    n = plan.n
    hs, Js = gibbs.scaled_fields(h, J, prefactor, h_range, (-1, 1))
    ids = np.arange(C, dtype=np.uint32) + 11
    betas = np.linspace(0.0, beta, 6)[1:].astype(np.float32)
    for init in (1, 0):
        beta_from = 0.0 if init else 0.3
        ref = d.buffers(start)
        d.ais(ref, betas, beta_from, 11, SEED, 3, init)
        helper = ais_oracle.ais(plan, hs, Js, betas, ids, SEED, 3, start=None if init else start, beta_from=beta_from)
        for zeros, scales in ((np.zeros((C, n), np.float32), None), (np.zeros(n, np.float32), None),
                              (np.zeros((C, n), np.float32), np.linspace(0.2, 1.0, 5).astype(np.float32))):
            got = d.buffers(start)
            d.fields_ais(got, zeros, betas, scales, 11, SEED, 3, init, beta_from=beta_from, scale_from=0.0)
            assert _equal(got, ref, (0, 1)), (init, zeros.shape)
            want = fao.FieldAis(helper.spins, helper.log_w, helper.energy, helper.A,
                                helper.N + (1 + (n if scales is not None else 0)) * betas.size)
            _check(got, want, betas, scales, beta_from, f"{name} zero fields init={init}")


@pytest.mark.parametrize("name,C,h_scale,j_scale,prefactor,h_range,beta", IDENTITY, ids=[p[0] for p in IDENTITY])
def test_scales_of_one_are_no_scales_and_the_weights_may_go_unwritten(name, C, h_scale, j_scale, prefactor, h_range, beta):
    plan, rng, h, J, d, start = _identity(name, C, h_scale, j_scale, prefactor, h_range, beta, 3)
    fields = rng.standard_normal((C, plan.n)).astype(np.float32)
    betas = rng.uniform(0.0, 2.0 * beta, (C, 4)).astype(np.float32)
    for init in (1, 0):
        beta_from = 0.0 if init else 0.3
        none = d.buffers(start)
        d.fields_ais(none, fields, betas, None, 11, SEED, 3, init, beta_from=beta_from, scale_from=0.5)
        for ones in (np.ones(4, np.float32), np.ones((C, 4), np.float32)):
            got = d.buffers(start)
            d.fields_ais(got, fields, betas, ones, 11, SEED, 3, init, beta_from=beta_from, scale_from=1.0)
            assert _equal(got, none), (init, ones.shape)
        assert bool((none[2][:C] != 0.0).all())
        # log_weight_out == NULL: the same spins, the same energies, the buffer untouched; energy_out == NULL as well
        for with_e in (True, False):
            got = d.buffers(start)
            d.fields_ais(got, fields, betas, None, 11, SEED, 3, init, beta_from=beta_from, with_w=False, with_e=with_e)
            assert _equal(got, none, (0, 1, 3) if with_e else (0, 1)) and bool((got[2] == GUARD_W).all())
            assert with_e or bool((got[3] == GUARD_E).all())


@pytest.mark.parametrize("C", [21, 20])
@pytest.mark.parametrize("name", ["zephyr128", "random77"])
def test_rows_shared_by_r_chains_are_the_replicated_rows(name, C):
    """R = 3: 7 rows; with 20 chains the last row serves two."""
    _n, _c, h_scale, j_scale, prefactor, h_range, beta = next(p for p in IDENTITY if p[0] == name)
    plan, rng, h, J, d, start = _identity(name, C, h_scale, j_scale, prefactor, h_range, beta, 4)
    R, rows = 3, 7
    fields = rng.standard_normal((rows, plan.n)).astype(np.float32)
    betas, scales = rng.uniform(0.0, 2.0 * beta, (C, 4)).astype(np.float32), rng.uniform(0.0, 1.5, (C, 4)).astype(np.float32)
    for init in (1, 0):
        beta_from = 0.0 if init else 0.3
        want, got = d.buffers(start), d.buffers(start)
        d.fields_ais(want, np.repeat(fields, R, axis=0)[:C], betas, scales, 11, SEED, 3, init, beta_from=beta_from, scale_from=0.5)
        d.fields_ais(got, fields, betas, scales, 11, SEED, 3, init, beta_from=beta_from, scale_from=0.5, R=R)
        assert _equal(got, want), init
        # one shared row: R is not read
        one, other = d.buffers(start), d.buffers(start)
        d.fields_ais(one, fields[0], betas, scales, 11, SEED, 3, init, beta_from=beta_from, scale_from=0.5, R=1)
        d.fields_ais(other, fields[0], betas, scales, 11, SEED, 3, init, beta_from=beta_from, scale_from=0.5, R=5)
        assert _equal(other, one) and not _equal(one, want, (1,))


# ------------------------------------------------------------------------------------------------ placement and continuation
@pytest.mark.parametrize("name", ["random77", "zephyr512"])
def test_a_chain_does_not_depend_on_where_it_is_placed(name):
    """21 chains in one call, and the same chains as calls of 8 and 13 with chain_id0 advanced: other workgroups, other slots.
    R = 4: the split falls on a row boundary, the second call starts at row 2."""
    plan = _plan(name)
    n, C, R = plan.n, 21, 4
    rng = np.random.default_rng(n + 2)
    h, J = cond._params(plan, rng, 0.5, 2.0)
    fields = rng.standard_normal((6, n)).astype(np.float32)
    betas, scales = rng.uniform(0.0, 3.0, (C, 3)).astype(np.float32), rng.uniform(0.0, 1.5, (C, 3)).astype(np.float32)
    d = _Draw(plan, h, J, 0.3, (-0.35, 0.35))
    for init in (1, 0):
        start = _start(rng, C, n)
        kw = dict(beta_from=0.0 if init else 0.3, scale_from=0.5, R=R)
        whole, a, b = d.buffers(start), d.buffers(start[:8]), d.buffers(start[8:])
        d.fields_ais(whole, fields, betas, scales, 40, SEED, 5, init, **kw)
        d.fields_ais(a, fields[:2], betas[:8], scales[:8], 40, SEED, 5, init, **kw)
        d.fields_ais(b, fields[2:], betas[8:], scales[8:], 48, SEED, 5, init, **kw)
        for k in range(4):
            assert torch.equal(torch.cat([a[k][:8], b[k][:13]]), whole[k][:C]), (init, k)


@pytest.mark.parametrize("name,C", [("zephyr1024", 7), ("random77", 19)])
def test_two_calls_that_hand_the_state_on_are_one_call(name, C):
    """2 + 3 sweeps: the second call starts where the first ended, beta_from / scale_from the first call's last entries.  The
    spins are equal and the weights add up within the bound of the one call.  The second call walks its start energy afresh where
    the one call carries it on, and the carried energy is built from the ROUNDED float32 fields the decisions used: the two agree
    up to the order of the float64 additions only where those sums are exact, so h, J, the fields and the strengths sit on a binary
    grid here (multiples of 1/16, 1/8 and 1/4; prefactor 1/2; a range that clamps on the grid), as in
    tests/test_gibbs_field_ais_host.py.  The betas do not: they enter in float64 alone."""
    plan = _plan(name)
    n, S1, S = plan.n, 2, 5
    rng = np.random.default_rng(n + 3)
    h = (rng.integers(-8, 9, n) / 16.0).astype(np.float32)
    J = (rng.integers(-8, 9, plan.n_edges) / 16.0).astype(np.float32)
    fields = (rng.integers(-16, 17, (C, n)) / 8.0).astype(np.float32)
    betas, scales = rng.uniform(0.0, 2.0, S).astype(np.float32), (rng.integers(0, 7, S) / 4.0).astype(np.float32)
    d = _Draw(plan, h, J, 0.5, (-0.75, 0.75))
    Js = gibbs.scaled_fields(h, J, 0.5, None, (-1, 1))[1]
    ids = np.arange(C, dtype=np.uint32) + 3
    start = _start(rng, C, n)
    one, two = d.buffers(start), d.buffers(start)
    d.fields_ais(one, fields, betas, scales, 3, SEED, 3, 1, scale_from=0.0)
    d.fields_ais(two, fields, betas[:S1], scales[:S1], 3, SEED, 3, 1, scale_from=0.0)
    w_first, mid = two[2].clone(), two[1].clone()
    d.fields_ais(two, fields, betas[S1:], scales[S1:], 3, SEED, 3 + S1, 0, beta_from=betas[S1 - 1], scale_from=scales[S1 - 1])
    assert _equal(two, one, (0, 1)) and not torch.equal(mid, one[1])
    want = fao.field_ais(plan, h, fields, 0.5, (-0.75, 0.75), Js, betas, scales, ids, SEED, 3, scale_from=0.0)
    _check(one, want, betas, scales, 0.0, f"{name} one call")
    summed = (two[0], two[1], torch.cat([w_first[:C] + two[2][:C], two[2][C:]]), two[3])
    _check(summed, want, betas, scales, 0.0, f"{name} two calls")


# ------------------------------------------------------------------------------------------------ a rejected call
def test_a_rejected_call_writes_nothing():
    plan = _plan("random77")
    n, C, S = plan.n, 6, 4
    rng = np.random.default_rng(n + 5)
    h, J = cond._params(plan, rng, 0.5, 2.0)
    d = _Draw(plan, h, J, 0.3)
    fields = torch.zeros((C, n), device="cuda")
    table = torch.ones((C, S), device="cuda")
    dyn = torch.zeros(64, dtype=torch.int32, device="cuda")
    start = _start(rng, C, n)
    bufs = d.buffers(start)
    before = [t.clone() for t in bufs]
    ok = dict(fields=fields, stride=n, R=1, betas=table, beta_stride=0, beta_from=0.0, scales=table, scale_stride=0, scale_from=1.0,
              sweeps=S, init=1, C=C, dyn=None)
    nan = float("nan")
    cases = [dict(fields=None), dict(stride=n + 1), dict(stride=1), dict(stride=-n), dict(dyn=dyn.data_ptr()), dict(C=0),  # _fields'
             dict(betas=None), dict(sweeps=0), dict(sweeps=-1), dict(beta_stride=3), dict(beta_stride=S + 1), dict(beta_stride=n),  # _ais'
             dict(beta_from=0.3), dict(beta_from=-0.5, init=0), dict(beta_from=nan, init=0), dict(beta_from=INF, init=0),
             dict(scale_stride=3), dict(scale_stride=S + 1), dict(scale_stride=n), dict(scale_stride=-S),  # its own
             dict(R=0), dict(R=-3), dict(scale_from=nan), dict(scale_from=INF), dict(scale_from=-INF), dict(scale_from=nan, scales=None)]
    for case in cases:
        a = dict(ok, **case)
        rc = d.raw(bufs, a["fields"], a["stride"], a["R"], a["betas"], a["beta_stride"], a["beta_from"], a["scales"], a["scale_stride"],
                   a["scale_from"], 0, SEED, 0, a["sweeps"], a["init"], C=a["C"], dyn=a["dyn"])
        assert rc == -1, (case, rc, _lib.lib().dvg_last_error())
    torch.cuda.synchronize()
    assert all(torch.equal(t, b) for t, b in zip(bufs, before))
    a = ok
    assert d.raw(bufs, a["fields"], a["stride"], a["R"], a["betas"], a["beta_stride"], a["beta_from"], a["scales"], a["scale_stride"],
                 a["scale_from"], 0, SEED, 0, a["sweeps"], a["init"], C=a["C"]) == 0
    torch.cuda.synchronize()
    assert not bool((bufs[1][:C] == GUARD_OUT).any()) and not bool((bufs[2][:C] == GUARD_W).any())


# ------------------------------------------------------------------------------------------------ the estimate
EVIDENCE_SEED = SEED
ROWS, PER_ROW, BURN, RAMP, OFFSET = 4, 256, 64, 64, 11


@functools.lru_cache(maxsize=None)
def _evidence_case(seed=EVIDENCE_SEED):
    """Zephyr 16 (72 edges) at beta 1, prefactor 1, no linear range: 4 rows of N(0, 1) logits, 256 chains per row, under the
    streams a GibbsSampler of this seed and chain_offset 11 gives them.  CPU only: the exact log ratios by enumeration, and the
    helper's draw -- the start from 64 field-draw sweeps with a zero row (field_seed, sweeps 0 ..), then the strengths ramped over
    64 sweeps (field_ais_seed, sweeps 0 ..).

    h is 0.5 U(-1, 1) as in the 16-spin case of tests/test_gpu_gibbs_ais.py, J a QUARTER of that case's U(-1, 1).  With the full
    couplings the model is bimodal at beta 1 and Gibbs chains do not cross between the modes: after 64 sweeps from the INIT stream
    the chains' mean of spin 0 is 0.03 where enumeration gives 0.37 (0.23 after 1000 sweeps), so the start is no sample of the prior
    and every row's estimate sits 2 to 10 standard errors off -- the bias GibbsSampler.log_evidence's docstring warns of, which is
    the sampler's and not the estimator's.  With these couplings 64 sweeps reach equilibrium (the means agree to 0.05)."""
    plan, nodes = cond._solver_plan("zephyr", 16)
    assert plan.n_edges == 72
    rng = np.random.default_rng(16)
    h = (0.5 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (0.25 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    logits = rng.standard_normal((ROWS, plan.n)).astype(np.float32)
    fields = smp.logit_fields(logits, 1.0, 1.0)
    seed &= 0xFFFFFFFFFFFFFFFF
    field_seed, field_ais_seed = seed ^ 0x666C6431, seed ^ 0x66616931
    C = ROWS * PER_ROW
    ids = np.arange(C, dtype=np.uint32) + OFFSET
    hs, Js = gibbs.scaled_fields(h, J, 1.0, None, (-1, 1))
    start = fao.field_oracle.field_sweeps(gibbs.init_state(ids, plan.n, field_seed, 0), ids, np.broadcast_to(hs, (C, plan.n)), Js, 1.0, plan,
                                          field_seed, 0, BURN)
    scales = np.linspace(0.0, 1.0, RAMP + 1)[1:].astype(np.float32)
    betas = np.full(RAMP, 1.0, np.float32)
    want = fao.field_ais(plan, h, fields, 1.0, None, Js, betas, scales, ids, field_ais_seed, 0, start=start, beta_from=1.0, scale_from=0.0,
                         row_chains=PER_ROW)
    ei, ej = np.asarray(plan.edge_i), np.asarray(plan.edge_j)
    rows = fao.chain_rows(h, fields, np.ones(ROWS, np.float32), 1.0, None)
    exact = np.array([ais_oracle.exact_log_z(plan.n, rows[r], Js, ei, ej, 1.0) for r in range(ROWS)]) - \
        ais_oracle.exact_log_z(plan.n, hs, Js, ei, ej, 1.0)
    return dict(plan=plan, nodes=nodes, h=h, J=J, logits=logits, fields=fields, ids=ids, start=start, betas=betas, scales=scales, want=want,
                exact=exact, field_seed=field_seed, field_ais_seed=field_ais_seed, seed=seed)


def _within_three_standard_errors(log_w, exact, where):
    ok = True
    for r in range(ROWS):
        est, ess, std_err = fao.log_ratio_estimate(log_w[r])
        print(f"{where} row {r}: exact {exact[r]:.6f}, estimate {est:.6f}, ESS {ess:.0f} of {PER_ROW}, 3 std_err {3 * std_err:.4f}")
        ok &= abs(est - exact[r]) <= 3.0 * std_err
    return ok


def test_log_evidence_against_enumeration():
    """Each row's log ratio lies within 3 standard errors of exact_log_z(row) - exact_log_z(prior), and the draw is the helper's
    bit for bit.  The helper was run on the CPU with this seed before the test went to the GPU, and the seed kept is one for which
    the helper itself satisfies the condition on all four rows (the first one tried): the draw being bit-exact, the condition is
    decided there.  The same condition through GraphRestrictedBoltzmannMachine.log_evidence: the sampler's streams are the ones the
    case was built under, so it is the same draw."""
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    c = _evidence_case()
    plan, want, C = c["plan"], c["want"], ROWS * PER_ROW
    assert _within_three_standard_errors(want.log_w.reshape(ROWS, PER_ROW), c["exact"], "helper")
    d = _Draw(plan, c["h"], c["J"], 1.0, (-INF, INF))
    prior = d.buffers(np.ones((C, plan.n), dtype=np.int8))
    d.field(prior, np.zeros(plan.n, np.float32), 1.0, OFFSET, c["field_seed"], 0, BURN, 1)
    assert np.array_equal(prior[0][:C].cpu().numpy(), c["start"])
    bufs = d.buffers(c["start"])
    d.fields_ais(bufs, c["fields"], c["betas"], c["scales"], OFFSET, c["field_ais_seed"], 0, 0, beta_from=1.0, scale_from=0.0, R=PER_ROW)
    _check(bufs, want, c["betas"], c["scales"], 1.0, "zephyr16, 4 rows x 256 chains x 64 sweeps")
    assert _within_three_standard_errors(bufs[2][:C].cpu().numpy().reshape(ROWS, PER_ROW), c["exact"], "kernel")

    nodes = c["nodes"]
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                           np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    with torch.no_grad():
        grbm._linear.copy_(torch.from_numpy(c["h"]).cuda())
        grbm._quadratic.copy_(torch.from_numpy(c["J"]).cuda())
    s = smp.GibbsSampler(plan, nodes, beta=1.0, sweeps=BURN, seed=c["seed"], persistent=True, chain_offset=OFFSET, h_range=(-4, 4),
                         j_range=(-1, 1))
    res = grbm.log_evidence(s, torch.from_numpy(c["logits"]).cuda(), prefactor=1.0, linear_range=None, quadratic_range=(-1, 1),
                            chains_per_row=PER_ROW, num_sweeps=RAMP)
    assert isinstance(res, smp.LogEvidence) and res.log_ratio.shape == (ROWS,) and res.log_ratio.dtype == torch.float64 and res.log_ratio.is_cuda
    assert res.log_weights.shape == (ROWS, PER_ROW) and res.samples.shape == (C, plan.n)
    assert (s.field_sweep_count, s.field_ais_sweep_count, s.sweep_count, s.calls) == (BURN, RAMP, 0, 0)
    assert torch.equal(res.samples, bufs[1][:C]) and torch.equal(res.log_weights.reshape(-1), bufs[2][:C])
    err = (res.log_ratio.cpu().numpy() - c["exact"])
    assert (np.abs(err) <= 3.0 * res.std_err.cpu().numpy()).all(), (err, res.std_err)
    for r in range(ROWS):
        est, ess, std_err = fao.log_ratio_estimate(res.log_weights[r].cpu().numpy())
        assert abs(float(res.log_ratio[r]) - est) < 1e-9 and abs(float(res.ess[r]) - ess) < 1e-6 * ess and abs(float(res.std_err[r]) - std_err) < 1e-9
    # a start of the caller's own: no burn-in draw
    again = grbm.log_evidence(s, torch.from_numpy(c["logits"]).cuda(), prefactor=1.0, quadratic_range=(-1, 1), chains_per_row=PER_ROW,
                              num_sweeps=RAMP, start=res.samples)
    assert (s.field_sweep_count, s.field_ais_sweep_count) == (BURN, 2 * RAMP) and not torch.equal(again.log_weights, res.log_weights)
    with pytest.raises(TypeError):
        grbm.log_evidence(object(), torch.from_numpy(c["logits"]).cuda(), prefactor=1.0)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_sample_fields_ais_leaves_the_other_streams_alone():
    plan, nodes = cond._solver_plan("zephyr", 128)
    rng = np.random.default_rng(2)
    h, J = cond._params(plan, rng, 0.05, 5.0)
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    C, n, rows, R = 24, plan.n, 3, 3
    K = rows * R
    mk = lambda: smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5,  # noqa: E731
                                  h_range=(-4, 4), j_range=(-1, 1))
    fields_np = rng.standard_normal((rows, n)).astype(np.float32)
    fields = torch.from_numpy(fields_np).cuda()
    h_range = (-0.06, 0.06)
    Js = gibbs.scaled_fields(h, J, 0.05, None, (-1, 1))[1]
    ids = np.arange(K, dtype=np.uint32) + 5

    ref = mk()
    ref_draws = [ref.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone() for _ in range(2)]

    s = mk()
    assert s.field_ais_seed == SEED ^ 0x66616931 and s.field_ais_sweep_count == 0
    first = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone()
    before = (s._state.clone(), s._state.data_ptr(), s.sweep_count, s.calls, s.cond_sweep_count, s.anneal_sweep_count, s.ais_sweep_count,
              s.field_sweep_count, s.pt_sweep_count, s.trace_sweep_count)

    def check(got, want, betas, scales, beta_from, where):
        samples, log_w, energy = got
        assert samples.shape == (K, n) and samples.dtype == torch.float32 and samples.is_cuda
        assert log_w.shape == (K,) and log_w.dtype == torch.float64 and log_w.is_cuda and energy.shape == (K,) and energy.dtype == torch.float64
        assert np.array_equal(samples.cpu().numpy(), want.spins.astype(np.float32)), where
        unit = 4.0 * want.N * 2.0 ** -53 * want.A
        assert (np.abs(energy.cpu().numpy() - want.energy) <= unit).all(), where
        assert (np.abs(log_w.cpu().numpy() - want.log_w) <= unit * _weight_scale(betas, scales, beta_from, K)).all(), where

    # host tables, fresh chains, three chains per row: sweeps 0 .. 4 under the draw's own key
    betas, scales = smp.beta_schedule(0.0, 20.0, 5, "linear"), np.linspace(0.0, 1.0, 6)[1:].astype(np.float32)
    got = s.sample_fields_ais(lin, quad, 0.05, h_range, (-1, 1), fields, betas, scales, chains_per_row=R, scale_from=0.0)
    assert s.field_ais_sweep_count == 5
    check(got, fao.field_ais(plan, h, fields_np, 0.05, h_range, Js, betas, scales, ids, s.field_ais_seed, 0, scale_from=0.0, row_chains=R),
          betas, scales, 0.0, "fresh chains")
    # the same call again takes other words: sweeps 5 .. 9
    again = s.sample_fields_ais(lin, quad, 0.05, h_range, (-1, 1), fields, betas, scales, chains_per_row=R, scale_from=0.0)
    assert s.field_ais_sweep_count == 10 and not torch.equal(again[0], got[0])
    check(again, fao.field_ais(plan, h, fields_np, 0.05, h_range, Js, betas, scales, ids, s.field_ais_seed, 5, scale_from=0.0, row_chains=R),
          betas, scales, 0.0, "the second call")
    # betas = None: the sampler's own beta on every sweep, the sweeps named by a (C, S) device table of strengths; a float32 start
    ladder = rng.uniform(-0.5, 1.5, (K, 4)).astype(np.float32)
    start = _start(rng, K, n)
    start_t = torch.from_numpy(start.astype(np.float32)).cuda()
    got = s.sample_fields_ais(lin, quad, 0.05, h_range, (-1, 1), fields, None, torch.from_numpy(ladder).cuda(), chains_per_row=R,
                              start=start_t, beta_from=20.0, scale_from=0.25)
    assert s.field_ais_sweep_count == 14 and torch.equal(start_t, torch.from_numpy(start.astype(np.float32)).cuda())
    const = np.full(4, 20.0, np.float32)
    check(got, fao.field_ais(plan, h, fields_np, 0.05, h_range, Js, const, ladder, ids, s.field_ais_seed, 10, start=start, beta_from=20.0,
                             scale_from=0.25, row_chains=R), const, ladder, 20.0, "from a state")
    # scales = None, one shared row, num_reads naming the chains
    got = s.sample_fields_ais(lin, quad, 0.05, h_range, (-1, 1), fields[0], betas, num_reads=K)
    assert s.field_ais_sweep_count == 19
    check(got, fao.field_ais(plan, h, fields_np[0], 0.05, h_range, Js, betas, None, ids, s.field_ais_seed, 14), betas, None, 0.0, "one row")

    # the training, conditional, annealed, AIS, field, exchange and traced streams never noticed
    assert s._state.data_ptr() == before[1] and torch.equal(s._state, before[0])
    assert (s.sweep_count, s.calls, s.cond_sweep_count, s.anneal_sweep_count, s.ais_sweep_count, s.field_sweep_count, s.pt_sweep_count,
            s.trace_sweep_count) == before[2:]
    second = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)
    assert torch.equal(first, ref_draws[0]) and torch.equal(second, ref_draws[1])
    with pytest.raises(_lib.DvgError):
        s.sample_fields_ais(lin, quad, 0.05, h_range, (-1, 1), fields, betas, chains_per_row=R, num_reads=K + 1)
    with pytest.raises(_lib.DvgError):
        s.sample_fields_ais(lin, quad, 0.05, h_range, (-1, 1), fields, betas, chains_per_row=R, start=start_t[:4])
    assert s.field_ais_sweep_count == 19
    s.reset()
    assert s.field_ais_sweep_count == 0


def test_grbm_sample_fields_is_the_samplers():
    plan, nodes = cond._solver_plan("zephyr", 128)
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                           np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    mk = lambda: smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, chain_offset=5)  # noqa: E731
    fields = torch.randn((6, plan.n), generator=torch.Generator().manual_seed(1)).cuda()
    a, b = mk(), mk()
    got = grbm.sample_fields(a, fields, prefactor=0.05, linear_range=(-0.06, 0.06), quadratic_range=(-1, 1), sweeps=3)
    want = b.sample_fields(grbm._linear, grbm._quadratic, 0.05, (-0.06, 0.06), (-1, 1), fields, sweeps=3)
    assert torch.equal(got, want) and a.field_sweep_count == 3


def test_model_wrapper_prior_log_evidence():
    import gen
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    m.overlap_sampler = False  # (as in the AIS file: this test takes no stream from the process's pool)
    B = 6
    images = torch.from_numpy(gen.make_images(B, seed=4)).reshape(B, 1, 32, 32).cuda()
    value, res = m.prior_log_evidence(images, chains_per_image=32, num_sweeps=20, burn_in=10)
    assert value.shape == (B,) and value.dtype == torch.float64 and value.is_cuda and torch.isfinite(value).all()
    assert isinstance(res, smp.LogEvidence) and res.log_weights.shape == (B, 32) and torch.isfinite(res.log_ratio).all()
    assert float(res.ess.min()) >= 1.0
    s = m.sampler
    assert (s.field_sweep_count, s.field_ais_sweep_count) == (10, 20)
    assert (s.sweep_count, s.calls, s.ais_sweep_count, s.anneal_sweep_count, s.cond_sweep_count) == (0, 0, 0, 0, 0) and s._state is None
