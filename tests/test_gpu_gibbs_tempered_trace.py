"""GPU parity of the traced exchange draw (``dvg_gibbs_sample_tempered_traced``, "DVG PT trace v1": the exchange draw with a
history by rung -- packed states, carried energies -- and the rung walk by chain written from inside the kernel) against the
definition in ``tests/tempered_trace_oracle.py``, against ``dvg_gibbs_sample_tempered``, ``dvg_gibbs_sample_traced`` and
``dvg_grbm_energy_packed`` where the definition makes them equal, and of the Python surface built on it.

The shapes, (h, J), seeds and ``SWEEP0 = 6`` are those of ``tests/test_gpu_gibbs_tempered.py``, by import: nine shapes, every
kernel form and idle-slot case.  Records and rungs: equal to the helper's, bit for bit.  Recorded energies: the kernel and the
helper add the same at most N = n (S + 2) float64 addends of absolute sum A (at the record) in two orders, so
|energy - helper| <= 4 N 2^-53 A.  The five "DVG PT v1" outputs: equal to ``dvg_gibbs_sample_tempered``'s on the same arguments
bit for bit, the energies too -- the records must not perturb them.  No exchange decision is left out of the comparison: every
test that compares with the helper asserts that the helper's every |u - exp(d)| is at least 10^6 times its bound.

Record rules per shape: (burn_in, thin) = (0, 1), (1, 2), (3, 4) and (1, S - 2), which records once (after sweep S - 1).  A rule
that records nothing on a shape (``zephyr1024`` has 4 sweeps: (3, 4)) must be rejected there.  Conventions of that file: a guard
row or element behind every output, the plan's form asserted per shape, a nonzero first chain id."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_oracle as eo  # noqa: E402
import tempered_oracle  # noqa: E402
import tempered_trace_oracle as tto  # noqa: E402
import test_gpu_gibbs_tempered as shapes  # noqa: E402
import trace_oracle  # noqa: E402
from image_generation_amd import _lib, functional as F, sampler as smp  # noqa: E402
from test_gpu_gibbs_tempered import SEED, SHAPES, SWEEP0, parameters  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_WORD, GUARD_ET, GUARD_RT = 0x5A5A5A5A, -4321.5, 0xEE
NAME = "dvg_gibbs_sample_tempered_traced"


def rules(sweeps):
    return ((0, 1), (1, 2), (3, 4), (1, sweeps - 2))


RULE_IDS = ["every", "b1t2", "b3t4", "once"]


@functools.lru_cache(maxsize=None)
def definition(name, burn_in, thin):
    """The helper's traced draw of the shape (fresh chains), computed once and shared; nothing changes it."""
    plan, _R, _Q, every, sweeps, _generic, _p, _h, _J, hs, Js, ladder, ids = parameters(name)
    want = tto.tempered_traced(plan, hs, Js, ladder, ids, SEED, SWEEP0, sweeps, every, burn_in, thin)
    # no decision is left out: every coin of the helper's run is far from a tie
    for margin, bound, _accepted in want.draw.coins:
        assert margin >= 1e6 * bound, (name, margin, bound)
    return want


# ------------------------------------------------------------------------------------------------ the raw ABI
def trace_buffers(C, M, W):
    """trace_out, energy_trace_out, rung_trace_out, each with a guard row or element behind the last record"""
    bits = torch.full((C * M + 1, W), GUARD_WORD, dtype=torch.int32, device="cuda")
    e_trace = torch.full((C * M + 1,), GUARD_ET, dtype=torch.float64, device="cuda")
    r_trace = torch.full((C * M + 1,), GUARD_RT, dtype=torch.uint8, device="cuda")
    return bits, e_trace, r_trace


def raw(d, ladder_ptr, R, every, state_ptr, rung_ptr, C, id0, seed, sweep0, sweeps, init, out_ptr, energy_ptr, accept_ptr, trace_ptr,
        e_trace_ptr, r_trace_ptr, burn_in, thin, dyn=None):
    return _lib.lib().dvg_gibbs_sample_tempered_traced(d.gh.ptr, d.lin.data_ptr(), d.quad.data_ptr(), d.prefactor, -4.0, 4.0, -1.0, 1.0,
                                                       ladder_ptr, R, every, state_ptr, rung_ptr, C, id0, seed, sweep0, sweeps, init,
                                                       out_ptr, energy_ptr, accept_ptr, trace_ptr, e_trace_ptr, r_trace_ptr, burn_in,
                                                       thin, dyn, _lib.stream_ptr())


def traced(d, bufs, tbufs, ladder, every, id0, seed, sweep0, sweeps, init, burn_in, thin, outputs=(True, True, True), records=(True, True)):
    """One call on the buffers; returns the five draw outputs and the three records as numpy (guards included)."""
    state, rung, out, energy, accept = bufs
    bits, e_trace, r_trace = tbufs
    C = int(state.shape[0]) - 1
    t = torch.from_numpy(np.ascontiguousarray(ladder, dtype=np.float32)).cuda()
    ptrs = [b.data_ptr() if on else None for b, on in zip((out, energy, accept), outputs)]
    rptrs = [b.data_ptr() if on else None for b, on in zip((e_trace, r_trace), records)]
    _lib.check(raw(d, t.data_ptr(), int(t.shape[0]), every, state.data_ptr(), rung.data_ptr(), C, id0, seed, sweep0, sweeps, init, *ptrs,
                   bits.data_ptr(), *rptrs, burn_in, thin), NAME)
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in bufs], [bits.cpu().numpy().view(np.uint32), e_trace.cpu().numpy(), r_trace.cpu().numpy()]


def split(recs, Q, R, M, where):
    """The records without their guards, shaped (Q, R, M, ...); the guards asserted."""
    bits, e_trace, r_trace = recs
    C = Q * R
    assert (bits[C * M] == GUARD_WORD).all(), f"a record written past the last one ({where})"
    assert e_trace[C * M] == GUARD_ET and r_trace[C * M] == GUARD_RT, f"an element written past the last record ({where})"
    return bits[:C * M].reshape(Q, R, M, -1), e_trace[:C * M].reshape(Q, R, M), r_trace[:C * M].reshape(Q, R, M)


@functools.lru_cache(maxsize=None)
def plain_draw(name):
    """``dvg_gibbs_sample_tempered`` on the shape's arguments: what the traced draw's five outputs must equal bit for bit."""
    _plan, R, Q, every, sweeps, generic, p, _hs, _Js, ladder, _ids, d = shapes._setup(name)
    with _lib.option_scope(gibbs_generic=generic):
        return d.tempered(d.buffers(Q * R), ladder, every, p["id0"], SEED, SWEEP0, sweeps, 1)


@functools.lru_cache(maxsize=None)
def traced_draw(name, burn_in, thin):
    """The traced draw of the shape under a record rule, run once and shared; nothing changes it."""
    plan, R, Q, every, sweeps, generic, p, _hs, _Js, ladder, _ids, d = shapes._setup(name)
    M = (sweeps - burn_in) // thin
    with _lib.option_scope(gibbs_generic=generic):
        res, recs = traced(d, d.buffers(Q * R), trace_buffers(Q * R, M, (plan.n + 31) // 32), ladder, every, p["id0"], SEED, SWEEP0,
                           sweeps, 1, burn_in, thin)
    shapes._guards(res, Q * R, name)
    return res, split(recs, Q, R, M, name)


def same_draw(res, ref, where):
    for got, want, what in zip(res, ref, ("state", "rung", "samples_out", "energy_out", "accept_out")):
        assert np.array_equal(got, want), f"{what} differs from dvg_gibbs_sample_tempered's ({where})"


# ------------------------------------------------------------------------------------------------ 1. against the helper
@pytest.mark.parametrize("rule", range(4), ids=RULE_IDS)
@pytest.mark.parametrize("name", SHAPES)
def test_against_the_definition(name, rule):
    plan, R, Q, every, sweeps, generic, p, _hs, _Js, ladder, _ids, d = shapes._setup(name)
    burn_in, thin = rules(sweeps)[rule]
    C, M = Q * R, (sweeps - burn_in) // thin
    if M < 1:  # the rule records nothing on this shape: the call is rejected, nothing is written
        bufs, tbufs = d.buffers(C), trace_buffers(C, 1, (plan.n + 31) // 32)
        before = [b.clone() for b in bufs + tbufs]
        t = torch.from_numpy(ladder).cuda()
        with _lib.option_scope(gibbs_generic=generic):
            rc = raw(d, t.data_ptr(), R, every, bufs[0].data_ptr(), bufs[1].data_ptr(), C, p["id0"], SEED, SWEEP0, sweeps, 1,
                     bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), tbufs[0].data_ptr(), tbufs[1].data_ptr(),
                     tbufs[2].data_ptr(), burn_in, thin)
        torch.cuda.synchronize()
        assert rc == -1 and b"record nothing" in _lib.lib().dvg_last_error()
        assert all(torch.equal(x, y) for x, y in zip(bufs + tbufs, before))
        return
    want = definition(name, burn_in, thin)
    res, (bits, e_trace, walk) = traced_draw(name, burn_in, thin)
    assert np.array_equal(want.sweeps, smp.trace_sweeps(sweeps, burn_in, thin)) and want.bits.shape == bits.shape
    assert np.array_equal(walk, want.walk), f"the rung walk differs from the helper ({name})"
    assert int((bits != want.bits).sum()) == 0, f"the records differ from the helper ({name})"
    unit = 4.0 * want.draw.N * 2.0 ** -53 * want.A
    err = np.abs(e_trace - want.energies)
    print(f"{name} ({burn_in}, {thin}): {M} records, |energy| up to {np.abs(want.energies).max():.4g}, worst error {err.max():.3e} "
          f"(its bound {unit.reshape(-1)[err.argmax()]:.3e}); {len(want.draw.coins)} coin decisions, largest bound / margin "
          f"{max([c[1] / c[0] for c in want.draw.coins], default=np.nan):.3e}")
    assert np.isfinite(e_trace).all() and (err <= unit).all(), (name, err.max(), unit.min())
    # the draw is dvg_gibbs_sample_tempered's, and the helper's
    same_draw(res, plain_draw(name), name)
    assert np.array_equal(res[0][:C], want.draw.spins) and np.array_equal(res[1][:C], want.draw.rungs)
    assert (np.sort(walk, axis=1) == np.arange(R)[None, :, None]).all()
    if M > 1 and thin == 1:
        assert not (walk == walk[:, :, :1]).all()  # (rungs change hands between records)


# ------------------------------------------------------------------------------------------------ 2. the last sweep recorded
@pytest.mark.parametrize("name", SHAPES)
def test_a_record_of_the_last_sweep_is_the_final_output(name):
    plan, R, Q, _every, sweeps, _generic, _p, _hs, _Js, _ladder, _ids, _d = shapes._setup(name)
    C = Q * R
    for burn_in, thin in ((0, 1), (sweeps - 2, 2)):  # (the second: one record, of the last sweep)
        (_state, rung, out, energy, _accept), (bits, e_trace, walk) = traced_draw(name, burn_in, thin)
        packed = smp.pack_spins(torch.from_numpy(out[:C]).cuda()).cpu().numpy().view(np.uint32)
        assert np.array_equal(bits[:, :, -1].reshape(C, -1), packed), name
        assert np.array_equal(e_trace[:, :, -1].reshape(-1), energy[:C]), name  # exactly: the same sum of the same shares
        assert np.array_equal(walk[:, :, -1].reshape(-1), rung[:C]), name
        same_draw(traced_draw(name, burn_in, thin)[0], plain_draw(name), name)


# ------------------------------------------------------------------------------------------------ 3. optional outputs
@pytest.mark.parametrize("name", ["pegasus64", "zephyr512x8", "random77"])
def test_outputs_may_be_null(name):
    plan, R, Q, every, sweeps, generic, p, _hs, _Js, ladder, _ids, d = shapes._setup(name)
    C, burn_in, thin = Q * R, 1, 2
    M, W = (sweeps - burn_in) // thin, (plan.n + 31) // 32
    full_res, (bits, e_trace, walk) = traced_draw(name, burn_in, thin)
    for outputs, records in (((True, True, True), (False, True)), ((True, True, True), (True, False)),
                             ((False, False, False), (True, True)), ((False, False, False), (False, False))):
        with _lib.option_scope(gibbs_generic=generic):
            res, recs = traced(d, d.buffers(C), trace_buffers(C, M, W), ladder, every, p["id0"], SEED, SWEEP0, sweeps, 1, burn_in, thin,
                               outputs=outputs, records=records)
        assert np.array_equal(res[0], full_res[0]) and np.array_equal(res[1], full_res[1])
        if outputs[0]:
            same_draw(res, full_res, name)
        else:
            assert (res[2] == shapes.GUARD_OUT).all() and (res[3] == shapes.GUARD_E).all() and (res[4] == shapes.GUARD_ACC).all()
        assert np.array_equal(recs[0][:C * M].reshape(bits.shape), bits) and (recs[0][C * M] == GUARD_WORD).all()
        if records[0]:
            assert np.array_equal(recs[1][:C * M].reshape(e_trace.shape), e_trace) and recs[1][C * M] == GUARD_ET
        else:
            assert (recs[1] == GUARD_ET).all()
        if records[1]:
            assert np.array_equal(recs[2][:C * M].reshape(walk.shape), walk) and recs[2][C * M] == GUARD_RT
        else:
            assert (recs[2] == GUARD_RT).all()


# ------------------------------------------------------------------------------------------------ 4. equal betas
@pytest.mark.parametrize("name", SHAPES)
def test_equal_betas_record_the_plain_traced_draw(name):
    """All R betas equal: every exchange is accepted (d = 0) and the spins are dvg_gibbs_sample's at that beta, so the records of
    chain c -- read BY CHAIN through the walk -- are dvg_gibbs_sample_traced's, and the walk is the odd-even transposition's."""
    plan, R, Q, every, sweeps, generic, p, _hs, _Js, _ladder, _ids, d = shapes._setup(name)
    C, n, W = Q * R, plan.n, (plan.n + 31) // 32
    burn_in, thin = (1, 2) if sweeps > 4 else (0, 1)
    M = (sweeps - burn_in) // thin
    with _lib.option_scope(gibbs_generic=generic):
        res, recs = traced(d, d.buffers(C), trace_buffers(C, M, W), np.full(R, p["beta"], np.float32), every, p["id0"], SEED, SWEEP0,
                           sweeps, 1, burn_in, thin)
        st_p = torch.empty((C, n), dtype=torch.int8, device="cuda")
        bits_p = torch.full((C * M + 1, W), GUARD_WORD, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib().dvg_gibbs_sample_traced(d.gh.ptr, d.lin.data_ptr(), d.quad.data_ptr(), d.prefactor, -4.0, 4.0, -1.0, 1.0,
                                                      p["beta"], st_p.data_ptr(), C, p["id0"], SEED, SWEEP0, sweeps, 1, None,
                                                      bits_p.data_ptr(), burn_in, thin, None, _lib.stream_ptr()), "dvg_gibbs_sample_traced")
        torch.cuda.synchronize()
    shapes._guards(res, C, name)
    bits, _e, walk = split(recs, Q, R, M, name)
    assert np.array_equal(res[0][:C], st_p.cpu().numpy())
    plain = bits_p.cpu().numpy().view(np.uint32)[:C * M].reshape(Q, R, M, W)  # by chain
    q, j, m = np.meshgrid(np.arange(Q), np.arange(R), np.arange(M), indexing="ij")
    assert np.array_equal(bits[q, walk, m], plain), f"records read by chain differ from the plain traced draw ({name})"
    for k, rec in enumerate(smp.trace_sweeps(sweeps, burn_in, thin)):
        want_rung, _acc = shapes._odd_even(R, SWEEP0, int(rec), every)
        assert np.array_equal(walk[:, :, k], np.tile(want_rung, (Q, 1))), (name, k)


# ------------------------------------------------------------------------------------------------ 5. recorded against exact energies
def energy_tolerance(plan, hs, Js, want, ids, seed, sweep0):
    """The bound ``tests/test_gpu_energy_packed.py`` holds the AIS draw's energy to, per record (``want``: the helper's trace at
    burn_in = 0, thin = 1): a carried energy -- start sum from float32 fields, then (s_new - s_old) f per update -- lies within
    1/2 sum_i g_i + 2 (sum of g_i over the chain's flips so far) of the float64 energy of the same state, g_i = gamma_d (|hs_i| +
    sum_j |Js_ij|), gamma_d = d u / (1 - d u), u = 2^-24; plus the float64 slack 4 N 2^-53 A of its additions and the packed
    entry's own 4 (n + n_edges) 2^-53 A.  By rung, (Q, R, M)."""
    Q, R, M, _W = want.bits.shape
    adj_ptr = np.asarray(plan.adj_ptr)
    deg = np.diff(adj_ptr).astype(np.float64)
    u = 2.0 ** -24
    gamma = deg * u / (1.0 - deg * u)
    absrow = np.zeros(plan.n)
    np.add.at(absrow, np.repeat(np.arange(plan.n), np.diff(adj_ptr)), np.abs(Js.astype(np.float64))[np.asarray(plan.adj_eid)])
    g = gamma * (np.abs(hs.astype(np.float64)) + absrow)
    q, j, m = np.meshgrid(np.arange(Q), np.arange(R), np.arange(M), indexing="ij")
    by_chain = trace_oracle.unpack(want.bits[q, want.walk, m], plan.n)  # (Q, R, M, n): chain j's state after every sweep
    start = tempered_oracle.cref.init_state(np.asarray(ids, dtype=np.uint32), plan.n, seed, sweep0).reshape(Q, R, 1, plan.n)
    states = np.concatenate([start, by_chain], axis=2)
    flipped = np.cumsum(((states[:, :, 1:] != states[:, :, :-1]) * g).sum(axis=3), axis=2)  # (Q, R, M) by chain
    by_rung = np.empty_like(flipped)
    by_rung[q, want.walk, m] = flipped
    A = float(np.abs(hs.astype(np.float64)).sum() + np.abs(Js.astype(np.float64)).sum())
    return 0.5 * g.sum() + 2.0 * by_rung + 4.0 * want.draw.N * 2.0 ** -53 * want.A + eo.bound(plan.n, plan.n_edges, A)


@pytest.mark.parametrize("name", SHAPES)
def test_recorded_energies_are_the_energies_of_the_recorded_states(name):
    plan, R, Q, _every, sweeps, _generic, p, hs, Js, _ladder, ids, d = shapes._setup(name)
    want = definition(name, 0, 1)
    _res, (bits, e_trace, _walk) = traced_draw(name, 0, 1)
    rows = torch.from_numpy(bits.view(np.int32).reshape(Q * R, sweeps, -1)).cuda()
    got = F.grbm_energy_packed(rows, d.gh, d.lin, d.quad, prefactor=p["prefactor"], linear_range=(-4.0, 4.0),
                               quadratic_range=(-1.0, 1.0)).cpu().numpy().reshape(Q, R, sweeps)
    tol = energy_tolerance(plan, hs, Js, want, ids, SEED, SWEEP0)
    err = np.abs(e_trace - got)
    print(f"{name}: recorded energies off the exact ones by up to {err.max():.3e} (tolerance {tol.reshape(-1)[err.argmax()]:.3e}), |E| up to "
          f"{np.abs(got).max():.4g}")
    assert (err <= tol).all()


# ------------------------------------------------------------------------------------------------ 6. two calls continue a draw
@pytest.mark.parametrize("name,first", [("pegasus64", 5), ("zephyr512x8", 4)])
def test_two_calls_continue_the_draw(name, first):
    """One call of S sweeps against two calls that hand state and rung on with sweep0 advanced, every sweep recorded: the same
    records and walk.  The second call sums its start energies afresh: the hand-over margin assertion of
    ``tests/test_gpu_gibbs_tempered.py`` -- the helper gives how far carried and fresh energies lie apart at the hand-over
    (delta), which moves a d by at most 2 |dbeta| delta; the margins of this shape's coins are asserted to be 1000 times that."""
    plan, R, Q, every, sweeps, generic, p, hs, Js, ladder, ids, d = shapes._setup(name)
    C, W = Q * R, (plan.n + 31) // 32
    want = definition(name, 0, 1)
    half = tempered_oracle.tempered(plan, hs, Js, ladder, ids, SEED, SWEEP0, first, every)
    fresh = tempered_oracle.tempered(plan, hs, Js, ladder, ids, SEED, SWEEP0 + first, 0, every, start=half.spins, rungs=half.rungs)
    delta = float(np.abs(half.energy - fresh.energy).max())
    slack = 2.0 * float(np.abs(np.diff(ladder.astype(np.float64))).max()) * delta
    print(f"{name}: carried and fresh energies up to {delta:.3e} apart at the hand-over; smallest margin {min(c[0] for c in want.draw.coins):.3e}")
    assert all(margin > 1e3 * slack for margin, _b, _a in want.draw.coins)
    one, (bits, e_trace, walk) = traced_draw(name, 0, 1)
    with _lib.option_scope(gibbs_generic=generic):
        a, ra = traced(d, d.buffers(C), trace_buffers(C, first, W), ladder, every, p["id0"], SEED, SWEEP0, first, 1, 0, 1)
        b, rb = traced(d, d.buffers(C, start=a[0][:C], rungs=a[1][:C]), trace_buffers(C, sweeps - first, W), ladder, every, p["id0"], SEED,
                       SWEEP0 + first, sweeps - first, 0, 0, 1)
    shapes._guards(b, C, name)
    pa, pb = split(ra, Q, R, first, name), split(rb, Q, R, sweeps - first, name)
    assert np.array_equal(np.concatenate([pa[0], pb[0]], axis=2), bits), f"the two calls' records are not the one call's ({name})"
    assert np.array_equal(np.concatenate([pa[2], pb[2]], axis=2), walk)
    assert np.array_equal(pa[1], e_trace[:, :, :first])  # (the first call carries what the one call carries)
    bound = 2.0 * delta + 4.0 * want.draw.N * 2.0 ** -53 * want.draw.A.max()
    assert (np.abs(pb[1] - e_trace[:, :, first:]) <= bound).all()
    assert np.array_equal(b[0], one[0]) and np.array_equal(b[1], one[1]) and np.array_equal(b[2], one[2])
    assert np.array_equal(a[4][:C] + b[4][:C], one[4][:C])


# ------------------------------------------------------------------------------------------------ 7. rejected calls
def test_invalid_arguments_launch_nothing():
    plan, R, Q, every, sweeps, _generic, p, _hs, _Js, ladder, _ids, d = shapes._setup("zephyr128")
    C, W = Q * R, (plan.n + 31) // 32
    bufs = d.buffers(C, start=np.ones((C, plan.n), np.int8), rungs=np.arange(C) % R)
    tbufs = trace_buffers(C, sweeps, W)
    state, rung, out, energy, accept = bufs
    before = [b.clone() for b in bufs + tbufs]
    t = torch.from_numpy(ladder).cuda()
    lp, sp, rp, tp = t.data_ptr(), state.data_ptr(), rung.data_ptr(), tbufs[0].data_ptr()
    #        ladder R every state rung chains sweeps trace burn_in thin dyn
    cases = [(None, R, 1, sp, rp, C, sweeps, tp, 0, 1, None), (lp, R, 1, sp, None, C, sweeps, tp, 0, 1, None),
             (lp, 1, 1, sp, rp, C, sweeps, tp, 0, 1, None), (lp, 17, 1, sp, rp, 34, sweeps, tp, 0, 1, None),
             (lp, R, 1, sp, rp, C - 1, sweeps, tp, 0, 1, None), (lp, R, 0, sp, rp, C, sweeps, tp, 0, 1, None),
             (lp, R, 1, sp, rp, C, 0, tp, 0, 1, None), (lp, R, 1, sp, rp, C, sweeps, tp, 0, 1, out.data_ptr()),
             (lp, R, 1, None, rp, C, sweeps, tp, 0, 1, None), (lp, R, 1, sp, rp, C, sweeps, None, 0, 1, None),
             (lp, R, 1, sp, rp, C, sweeps, tp, -1, 1, None), (lp, R, 1, sp, rp, C, sweeps, tp, 0, 0, None),
             (lp, R, 1, sp, rp, C, sweeps, tp, 0, -2, None), (lp, R, 1, sp, rp, C, sweeps, tp, sweeps, 1, None),
             (lp, R, 1, sp, rp, C, sweeps, tp, 0, sweeps + 1, None), (lp, R, 1, sp, rp, C, sweeps, tp, sweeps - 2, 3, None)]
    for ladder_ptr, reps, ev, state_ptr, rung_ptr, chains, s, trace_ptr, burn_in, thin, dyn in cases:
        rc = raw(d, ladder_ptr, reps, ev, state_ptr, rung_ptr, chains, p["id0"], SEED, SWEEP0, s, 0, out.data_ptr(), energy.data_ptr(),
                 accept.data_ptr(), trace_ptr, tbufs[1].data_ptr(), tbufs[2].data_ptr(), burn_in, thin, dyn)
        assert rc == -1, (reps, ev, chains, s, burn_in, thin, rc, _lib.lib().dvg_last_error())
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(bufs + tbufs, before))


# ------------------------------------------------------------------------------------------------ 8. the Python layers
def test_sample_tempered_trace_of_the_sampler():
    plan, nodes = shapes._solver_plan("zephyr", 128)
    _plan, R, Q, _every, _sweeps, _generic, p, h, J, hs, Js, ladder, _ids = parameters("zephyr128")
    mk = lambda: smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5,  # noqa: E731
                                  h_range=(-4, 4), j_range=(-1, 1))
    s = mk()
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    first = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=16).clone()
    counters = lambda: (s.sweep_count, s.calls, s.cond_sweep_count, s.anneal_sweep_count, s.ais_sweep_count, s.trace_sweep_count)  # noqa: E731
    before = (s._state.clone(), counters())
    ids = np.arange(Q * R, dtype=np.uint32) + 5
    n, W = plan.n, (plan.n + 31) // 32

    tt = s.sample_tempered_trace(lin, quad, 0.05, (-4, 4), (-1, 1), ladder, num_ladders=Q, num_sweeps=9, swap_every=2, burn_in=1, thin=2)
    assert isinstance(tt, smp.TemperedTrace) and s.pt_sweep_count == 9 and np.array_equal(tt.sweeps, [3, 5, 7, 9]) and tt.thin == 2
    assert tt.bits.shape == (Q, R, 4, W) and tt.bits.dtype == torch.int32 and tt.bits.is_cuda
    assert tt.energies.shape == (Q, R, 4) and tt.energies.dtype == torch.float64 and tt.walk.shape == (Q, R, 4) and tt.walk.dtype == torch.uint8
    assert np.array_equal(tt.betas, ladder) and tt.n == n and isinstance(tt.final, smp.Tempered)
    # the raw call on the same arguments
    d = shapes._Draw(plan, h, J, 0.05)
    res, recs = traced(d, d.buffers(Q * R), trace_buffers(Q * R, 4, W), ladder, 2, 5, s.pt_seed, 0, 9, 1, 1, 2)
    bits, e_trace, walk = split(recs, Q, R, 4, "sampler")
    assert np.array_equal(tt.bits.cpu().numpy().view(np.uint32), bits) and np.array_equal(tt.energies.cpu().numpy(), e_trace)
    assert np.array_equal(tt.walk.cpu().numpy(), walk)
    assert np.array_equal(tt.final.state.cpu().numpy(), res[0][:-1]) and np.array_equal(tt.final.rungs.cpu().numpy(), res[1][:-1])
    assert np.array_equal(tt.final.samples.cpu().numpy().reshape(Q * R, n), res[2][:-1])
    assert np.array_equal(tt.final.energies.cpu().numpy().reshape(-1), res[3][:-1])
    # ... and the helper
    want = tto.tempered_traced(plan, hs, Js, ladder, ids, s.pt_seed, 0, 9, 2, 1, 2)
    assert all(margin >= 1e6 * bound for margin, bound, _a in want.draw.coins)
    assert np.array_equal(bits, want.bits) and np.array_equal(walk, want.walk)
    assert np.array_equal(tt.final.accepted.cpu().numpy(), want.draw.accepted[:, :-1].astype(np.int64))
    # the last sweep is recorded: the final outputs
    assert torch.equal(tt.bits[:, :, -1], smp.pack_spins(tt.final.samples)) and torch.equal(tt.energies[:, :, -1], tt.final.energies)
    assert torch.equal(tt.walk[:, :, -1].reshape(-1).to(torch.int32), tt.final.rungs)

    # records off; continued from the result
    more = s.sample_tempered_trace(lin, quad, 0.05, (-4, 4), (-1, 1), ladder, num_ladders=Q, num_sweeps=3, swap_every=2,
                                   start=tt.final.state, rungs=tt.final.rungs, energies=False, rung_walk=False)
    assert s.pt_sweep_count == 12 and more.energies is None and more.walk is None and more.bits.shape == (Q, R, 3, W)
    ref = mk()
    ref.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=16)
    r1 = ref.sample_tempered(lin, quad, 0.05, (-4, 4), (-1, 1), ladder, num_ladders=Q, num_sweeps=9, swap_every=2)
    r2 = ref.sample_tempered(lin, quad, 0.05, (-4, 4), (-1, 1), ladder, num_ladders=Q, num_sweeps=3, swap_every=2, start=r1.state, rungs=r1.rungs)
    for x, y in ((tt.final, r1), (more.final, r2)):  # the same stream as sample_tempered
        assert torch.equal(x.state, y.state) and torch.equal(x.rungs, y.rungs) and torch.equal(x.samples, y.samples)
        assert torch.equal(x.energies, y.energies) and torch.equal(x.accepted, y.accepted)
    assert torch.equal(more.bits[:, :, -1], smp.pack_spins(r2.samples))
    with pytest.raises(ValueError):
        more.flow()

    # rung(r) feeds the statistics of a Trace unchanged
    gh = s.graph
    for r in range(R):
        tr = tt.rung(r)
        assert isinstance(tr, smp.Trace) and tr.bits.is_contiguous() and tr.bits.shape == (Q, 4, W) and torch.equal(tr.bits, tt.bits[:, r])
        assert torch.equal(tr.samples, tt.final.samples[:, r])
    target = tt.target
    assert torch.equal(target.bits, tt.bits[:, -1])
    ac = target.autocorrelation(2)
    assert ac.thin == 2 and ac.chains == Q and ac.records == 4 and ac.rho.shape == (3, n)
    assert isinstance(target.overlap(), smp.Overlap) and isinstance(target.overlap(tt.rung(0)), smp.Overlap)
    m = target.moments(gh)
    assert int(m.count) == 4 * Q
    series = tt.energy_series(max_lag=2)
    assert torch.equal(series.energies, tt.energies[:, -1]) and (series.thin, series.max_lag, series.chains, series.records) == (2, 2, Q, 4)
    assert tt.occupancy().shape == (Q, R, R) and bool((tt.occupancy().sum(2) == 4).all()) and tt.round_trips().shape == (Q, R)
    assert tt.flow().shape == (R,) and tt.flow().is_cuda
    # target.energy(...) against the carried energies, within the bound of the exact-energy test: a draw of every sweep gives it
    s2 = mk()
    every_sweep = s2.sample_tempered_trace(lin, quad, 0.05, (-4, 4), (-1, 1), ladder, num_ladders=Q, num_sweeps=9, swap_every=2)
    full = tto.tempered_traced(plan, hs, Js, ladder, ids, s2.pt_seed, 0, 9, 2, 0, 1)
    assert all(margin >= 1e6 * bound for margin, bound, _a in full.draw.coins)
    assert np.array_equal(every_sweep.bits.cpu().numpy().view(np.uint32), full.bits)
    tol = energy_tolerance(plan, hs, Js, full, ids, s2.pt_seed, 0)
    exact = every_sweep.target.energy(gh, lin, quad, 0.05, (-4, 4), (-1, 1))
    err = (exact - every_sweep.energies[:, -1]).abs().cpu().numpy()
    print(f"target.energy against the carried energies: off by up to {err.max():.3e} (tolerance {tol[:, -1].reshape(-1)[err.argmax()]:.3e})")
    assert exact.shape == (Q, 9) and (err <= tol[:, -1]).all()

    # the other streams never noticed
    assert torch.equal(s._state, before[0]) and counters() == before[1]
    ref2 = mk()
    ref_draws = [ref2.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=16).clone() for _ in range(2)]
    assert torch.equal(first, ref_draws[0]) and torch.equal(s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=16), ref_draws[1])
    with pytest.raises(ValueError):
        s.sample_tempered_trace(lin, quad, 0.05, (-4, 4), (-1, 1), ladder, num_ladders=Q, num_sweeps=4, burn_in=4)
    assert s.pt_sweep_count == 12


def test_model_wrapper_prior_tempered_mixing():
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    m.overlap_sampler = False  # (as in the AIS file: this test takes no stream from the process's pool)
    s = m.sampler
    beta = s.beta
    ladder = smp.beta_schedule(10.0, 20.0, 4)
    res = m.prior_tempered_mixing(ladder, max_lag=4, num_ladders=8, num_sweeps=60, swap_every=2, burn_in=10, thin=2)
    assert set(res) == {"tempered_autocorrelation", "tempered_energy", "plain_autocorrelation", "plain_energy", "acceptance_rate",
                        "round_trips", "flow"}
    assert (s.pt_sweep_count, s.trace_sweep_count, s.sweep_count, s.calls, s.ais_sweep_count) == (60, 60, 0, 0, 0) and s._state is None
    assert s.beta == beta
    for kind in ("tempered", "plain"):
        ac, es = res[kind + "_autocorrelation"], res[kind + "_energy"]
        assert isinstance(ac, smp.Autocorrelation) and isinstance(es, smp.EnergySeries)
        assert (ac.chains, ac.records, ac.thin, ac.max_lag) == (8, 25, 2, 4) and (es.chains, es.records, es.thin, es.max_lag) == (8, 25, 2, 4)
        assert bool(torch.isfinite(ac.tau_int).all()) and bool(torch.isfinite(es.tau_int))
        print(f"{kind}: spin tau_int (mean over spins) {float(ac.tau_int.mean()):.3f} records, energy tau_int {float(es.tau_int):.3f} records")
    rate = res["acceptance_rate"]
    assert rate.shape == (3,) and bool(((rate >= 0) & (rate <= 1)).all())
    assert res["round_trips"].shape == (8, 4) and res["round_trips"].dtype == torch.int64 and res["flow"].shape == (4,)
    print(f"acceptance {rate.cpu().numpy().round(3).tolist()}, round trips {int(res['round_trips'].sum())}, flow {res['flow'].cpu().numpy().round(3).tolist()}")
    # the plain draw is sample_trace's at betas[-1]; the exchange draw sample_tempered_trace's: the same numbers by hand
    s.reset()
    ranges = dict(prefactor=m.PREFACTOR, linear_range=m.linear_range, quadratic_range=m.quadratic_range)
    tt = m._grbm.sample_tempered_trace(s, ladder, num_ladders=8, num_sweeps=60, swap_every=2, burn_in=10, thin=2, **ranges)
    assert torch.equal(tt.energies[:, -1], res["tempered_energy"].energies) and torch.equal(tt.round_trips(), res["round_trips"])
    assert float(ladder[-1]) == 20.0
    s.beta = 20.0
    plain = m._grbm.sample_trace(s, num_reads=8, num_sweeps=60, burn_in=10, thin=2, **ranges)
    s.beta = beta
    e = plain.energy(m._grbm.graph_handle(plain.bits.device), m._grbm._linear.detach(), m._grbm._quadratic.detach(), m.PREFACTOR,
                     m.linear_range, m.quadratic_range)
    assert torch.equal(e, res["plain_energy"].energies)
    with pytest.raises(ValueError):
        m.prior_tempered_mixing(ladder, num_sweeps=5, burn_in=5)
