"""GPU parity of the per-chain-field draw (``dvg_gibbs_sample_fields``, "DVG field v1": ``dvg_gibbs_sample`` with chain c
sampling the model whose linear vector is ``rn(linear + fields[c])``) against its definition, bit for bit, and of
``GibbsSampler.sample_fields`` built on it.

The definition is the oracle called once per chain with that chain's hs and id; ``tests/field_oracle.py`` walks the same
arithmetic once with hs of shape (C, n), and ``tests/test_gibbs_fields_host.py`` pins it to the oracle.  The graphs are those
of ``tests/test_gpu_gibbs_conditional.py`` (its builders, imported).  The draw takes the rolled kernel on every graph, a float32
row of hs per chain slot beside the state rows: one-wave workgroups on the 77-spin graph (four chains) and on Zephyr 128 at
few chains (two), four-wave workgroups on Zephyr 128 at many chains, Zephyr 512 and Zephyr 1024 -- there stepped down from the
sixteen waves the other kinds run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_oracle  # noqa: E402
import test_gpu_gibbs_conditional as cond  # noqa: E402  (the graph builders)
from image_generation_amd import _lib, dev, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
INF = float("inf")


def _plan(name):
    return cond._random_plan(77, 0.35) if name == "random77" else cond._solver_plan("zephyr", int(name[len("zephyr"):]))[0]


class _Draw:
    """dvg_gibbs_sample_fields / dvg_gibbs_sample on one graph and one (h, J); ``h_range``: the linear range of both."""

    def __init__(self, plan, h, J, prefactor, beta, h_range=(-4.0, 4.0)):
        self.plan, self.prefactor, self.beta, self.h_range = plan, float(prefactor), float(beta), h_range
        self.gh = smp.GraphHandle(plan, "cuda")
        self.lin, self.quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()

    def _args(self, lin, state, id0, seed, sweep0, sweeps, init):
        return (self.gh.ptr, lin.data_ptr(), self.quad.data_ptr(), self.prefactor, self.h_range[0], self.h_range[1], -1.0, 1.0,
                self.beta, state.data_ptr(), int(state.shape[0]), id0, seed, sweep0, sweeps, init)

    def fields_rc(self, state, fields, stride, out, id0, seed, sweep0, sweeps, init, dyn=None):
        return _lib.lib().dvg_gibbs_sample_fields(*self._args(self.lin, state, id0, seed, sweep0, sweeps, init),
                                                  None if fields is None else fields.data_ptr(), stride,
                                                  out.data_ptr(), dyn, _lib.stream_ptr())

    def fields(self, state, fields, id0, seed, sweep0, sweeps, init):
        """``state`` (C, n) int8 device tensor, updated in place; ``fields`` float32 device tensor, (C, n) or (n,)."""
        out = torch.full(tuple(state.shape), 7.0, dtype=torch.float32, device="cuda")
        stride = self.plan.n if fields.dim() == 2 else 0
        _lib.check(self.fields_rc(state, fields, stride, out, id0, seed, sweep0, sweeps, init), "dvg_gibbs_sample_fields")
        return out

    def plain(self, state, id0, seed, sweep0, sweeps, init, lin=None):
        out = torch.full(tuple(state.shape), 7.0, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().dvg_gibbs_sample(*self._args(self.lin if lin is None else lin, state, id0, seed, sweep0, sweeps, init),
                                               out.data_ptr(), None, _lib.stream_ptr()), "dvg_gibbs_sample")
        return out


def _start(rng, C, n):
    return np.where(rng.uniform(size=(C, n)) < 0.5, -1, 1).astype(np.int8)


# ------------------------------------------------------------------------------------------------ bit parity with the oracle
# graph, chains, (LPC, WAVES) of the plan, h scale, J scale, prefactor, linear range, beta
PARITY = [
    ("random77", 19, (16, 1), 0.5, 2.0, 0.3, (-0.35, 0.35), 1.5),     # degrees above 20, an isolated spin, one wave
    ("zephyr128", 5, (32, 1), 0.05, 5.0, 0.05, (-0.06, 0.06), 20.0),   # two chains per wave
    ("zephyr512", 9, (64, 4), 0.05, 5.0, 0.05, (-0.06, 0.06), 20.0),
    ("zephyr1024", 5, (64, 4), 0.05, 5.0, 0.05, (-0.06, 0.06), 20.0),  # the stepped-down workgroup
]


@pytest.mark.parametrize("init", [1, 0])
@pytest.mark.parametrize("name,C,form,h_scale,j_scale,prefactor,h_range,beta", PARITY, ids=[p[0] for p in PARITY])
def test_fields_bit_exact(name, C, form, h_scale, j_scale, prefactor, h_range, beta, init):
    """3 sweeps from sweep 5, N(0, 1) fields per chain, a prefactor that is not 1 and a linear range that clamps some hs_c and
    not others; fresh chains (the INIT stream at sweep 5) and a given start."""
    plan = _plan(name)
    n, id0, sweep0, sweeps = plan.n, 1000, 5, 3
    p = dev.gibbs_draw_plan(plan, C, "field")
    assert p["form"] == "rolled" and p["params"] == dict(LPC=form[0], WAVES=form[1]), p
    rng = np.random.default_rng(n + C)
    h, J = cond._params(plan, rng, h_scale, j_scale)
    fields = rng.standard_normal((C, n)).astype(np.float32)
    hs = field_oracle.chain_fields(h, fields, prefactor, h_range)
    at_edge = (hs == np.float32(h_range[0])) | (hs == np.float32(h_range[1]))
    assert 0.05 < at_edge.mean() < 0.95
    Js = gibbs.scaled_fields(h, J, prefactor, None, (-1, 1))[1]
    ids = np.arange(C, dtype=np.uint32) + id0
    given = _start(rng, C, n)
    want = field_oracle.field_sweeps(gibbs.init_state(ids, n, SEED, sweep0) if init else given, ids, hs, Js, beta, plan, SEED, sweep0, sweeps)
    d = _Draw(plan, h, J, prefactor, beta, h_range)
    state = torch.from_numpy(given).cuda()
    out = d.fields(state, torch.from_numpy(fields).cuda(), id0, SEED, sweep0, sweeps, init)
    got, got_state = out.cpu().numpy(), state.cpu().numpy()
    mism = int((got != want.astype(np.float32)).sum())
    assert mism == 0, f"{mism} spin mismatches in samples_out"
    assert np.array_equal(got_state, want), "state differs from the oracle"
    assert not np.array_equal(want, given)


# ------------------------------------------------------------------------------------------------ against the plain draw
@pytest.mark.parametrize("init", [1, 0])
def test_zero_fields_are_the_plain_draw(init):
    """Zephyr 128 x 1025 chains: 129 workgroups of 8, the last one with a single chain.  (The plain draw runs the lane-major form.)"""
    plan = _plan("zephyr128")
    n, C = plan.n, 1025
    assert dev.gibbs_draw_plan(plan, C, "field")["chains_per_workgroup"] == 8 and dev.gibbs_draw_plan(plan, C, "plain")["form"] == "lane"
    rng = np.random.default_rng(n)
    h, J = cond._params(plan, rng, 0.05, 5.0)
    d = _Draw(plan, h, J, 0.05, 20.0)
    start = torch.from_numpy(_start(rng, C, n)).cuda()
    s_plain, s_field = start.clone(), start.clone()
    want = d.plain(s_plain, 11, SEED, 3, 5, init)
    for zeros in (torch.zeros((C, n), device="cuda"), torch.zeros(n, device="cuda")):
        s_field.copy_(start)
        got = d.fields(s_field, zeros, 11, SEED, 3, 5, init)
        assert torch.equal(got, want) and torch.equal(s_field, s_plain)
    assert not torch.equal(s_plain, start)


@pytest.mark.parametrize("name,C", [("random77", 19), ("zephyr1024", 6)])
def test_a_shared_row_is_the_plain_draw_on_the_sum(name, C):
    """Stride 0: dvg_gibbs_sample on rn(linear + row), with a range that clamps."""
    plan = _plan(name)
    n = plan.n
    rng = np.random.default_rng(n + 1)
    h, J = cond._params(plan, rng, 0.5, 2.0)
    row = rng.standard_normal(n).astype(np.float32)
    d = _Draw(plan, h, J, 0.3, 1.5, (-0.35, 0.35))
    start = torch.from_numpy(_start(rng, C, n)).cuda()
    s_plain, s_field = start.clone(), start.clone()
    want = d.plain(s_plain, 5, SEED, 6, 3, 0, lin=torch.from_numpy((h + row).astype(np.float32)).cuda())
    got = d.fields(s_field, torch.from_numpy(row).cuda(), 5, SEED, 6, 3, 0)
    assert torch.equal(got, want) and torch.equal(s_field, s_plain)
    assert not torch.equal(d.plain(start.clone(), 5, SEED, 6, 3, 0), want)  # the row matters


# ------------------------------------------------------------------------------------------------ chains do not know of each other
@pytest.mark.parametrize("name", ["random77", "zephyr512"])
def test_a_chain_does_not_depend_on_where_it_is_placed(name):
    """21 chains in one call, and the same chains as calls of 8 and 13 with chain_id0 advanced: other workgroups, other slots."""
    plan = _plan(name)
    n, C = plan.n, 21
    rng = np.random.default_rng(n + 2)
    h, J = cond._params(plan, rng, 0.5, 2.0)
    fields = torch.from_numpy(rng.standard_normal((C, n)).astype(np.float32)).cuda()
    d = _Draw(plan, h, J, 0.3, 1.5, (-0.35, 0.35))
    for init in (1, 0):
        start = torch.from_numpy(_start(rng, C, n)).cuda()
        whole = start.clone()
        out = d.fields(whole, fields, 40, SEED, 5, 3, init)
        a, b = start[:8].clone(), start[8:].clone()
        out_a = d.fields(a, fields[:8].contiguous(), 40, SEED, 5, 3, init)
        out_b = d.fields(b, fields[8:].contiguous(), 48, SEED, 5, 3, init)
        assert torch.equal(torch.cat([out_a, out_b]), out) and torch.equal(torch.cat([a, b]), whole)


def test_two_calls_that_hand_the_state_on_are_one_call():
    plan = _plan("zephyr1024")
    n, C = plan.n, 7
    rng = np.random.default_rng(n + 3)
    h, J = cond._params(plan, rng, 0.05, 5.0)
    fields = torch.from_numpy(rng.standard_normal((C, n)).astype(np.float32)).cuda()
    d = _Draw(plan, h, J, 0.05, 20.0, (-0.06, 0.06))
    one = torch.zeros((C, n), dtype=torch.int8, device="cuda")
    out_one = d.fields(one, fields, 3, SEED, 3, 5, 1)
    two = torch.zeros((C, n), dtype=torch.int8, device="cuda")
    mid = d.fields(two, fields, 3, SEED, 3, 2, 1)
    out_two = d.fields(two, fields, 3, SEED, 5, 3, 0)
    assert torch.equal(out_two, out_one) and torch.equal(two, one) and not torch.equal(mid, out_one)


# ------------------------------------------------------------------------------------------------ what a field does
def test_strong_fields_pin_every_spin():
    """Fields of +-50, no ranges, prefactor 1, beta 1: |f_i| >= 50 - 0.5 - 20 x 0.2 = 45.5, so z = 2 f clamps to +-87 and a
    spin opposes -sign(field) with probability below e^-80 -- after one sweep from any start every spin of every chain is
    -sign(field_i)."""
    plan = _plan("zephyr128")
    n, C = plan.n, 33
    assert np.diff(plan.adj_ptr).max() <= 20
    rng = np.random.default_rng(n + 4)
    h, J = cond._params(plan, rng, 0.5, 0.2)
    sign = np.where(rng.uniform(size=(C, n)) < 0.5, -1.0, 1.0).astype(np.float32)
    d = _Draw(plan, h, J, 1.0, 1.0, (-INF, INF))
    for init in (1, 0):
        state = torch.from_numpy(_start(rng, C, n)).cuda()
        out = d.fields(state, torch.from_numpy(50.0 * sign).cuda(), 0, SEED, 9, 1, init)
        assert np.array_equal(out.cpu().numpy(), -sign) and np.array_equal(state.cpu().numpy(), -sign.astype(np.int8))


# ------------------------------------------------------------------------------------------------ a rejected call
def test_a_rejected_call_writes_nothing():
    plan = _plan("random77")
    n, C = plan.n, 6
    rng = np.random.default_rng(n + 5)
    h, J = cond._params(plan, rng, 0.5, 2.0)
    d = _Draw(plan, h, J, 0.3, 1.5)
    fields = torch.zeros((C, n), device="cuda")
    start = torch.from_numpy(_start(rng, C, n)).cuda()
    dyn = torch.zeros(64, dtype=torch.int32, device="cuda")
    for kw in (dict(fields=None, stride=n), dict(stride=n + 1), dict(stride=1), dict(stride=-n), dict(stride=n, dyn=dyn.data_ptr()),
               dict(stride=n, sweeps=-1)):
        state = start.clone()
        out = torch.full((C, n), 7.0, device="cuda")
        rc = d.fields_rc(state, kw.get("fields", fields), kw["stride"], out, 0, SEED, 0, kw.get("sweeps", 2), 1, kw.get("dyn"))
        torch.cuda.synchronize()
        assert rc == -1, kw
        assert torch.equal(state, start) and bool((out == 7.0).all()), kw
    state = start.clone()
    out = torch.full((C, n), 7.0, device="cuda")
    assert d.fields_rc(state, fields, n, out, 0, SEED, 0, 2, 1) == 0 and not bool((out == 7.0).any())


# ------------------------------------------------------------------------------------------------ the Python surface
def test_sample_fields_leaves_the_training_stream_alone():
    plan, nodes = cond._solver_plan("zephyr", 128)
    rng = np.random.default_rng(2)
    h, J = cond._params(plan, rng, 0.05, 5.0)
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    C, n, K = 24, plan.n, 9
    mk = lambda: smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5,  # noqa: E731
                                  h_range=(-4, 4), j_range=(-1, 1))
    fields_np = rng.standard_normal((K, n)).astype(np.float32)
    fields = torch.from_numpy(fields_np).cuda()

    ref = mk()
    ref_draws = [ref.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone() for _ in range(2)]

    s = mk()
    assert s.field_seed == SEED ^ 0x666C6431 and s.field_sweep_count == 0
    first = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone()
    state_before, sweeps_before, calls_before = s._state.clone(), s.sweep_count, s.calls
    state_ptr = s._state.data_ptr()
    out = s.sample_fields(lin, quad, 0.05, (-0.06, 0.06), (-1, 1), fields, sweeps=3)
    assert out.shape == (K, n) and out.dtype == torch.float32 and out.is_cuda and set(out.unique().tolist()) <= {-1.0, 1.0}
    assert s._state.data_ptr() == state_ptr and torch.equal(s._state, state_before)
    assert (s.sweep_count, s.calls, s.field_sweep_count, s.cond_sweep_count) == (sweeps_before, calls_before, 3, 0)
    again = s.sample_fields(lin, quad, 0.05, (-0.06, 0.06), (-1, 1), fields, sweeps=3)  # other words: the counter moved on
    assert s.field_sweep_count == 6 and not torch.equal(again, out)
    second = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)
    assert torch.equal(first, ref_draws[0]) and torch.equal(second, ref_draws[1])

    # bit-exact against the oracle under the draw's own key, chain ids chain_offset + arange, sweeps 0..2 and 3..5
    hs = field_oracle.chain_fields(h, fields_np, 0.05, (-0.06, 0.06))
    Js = gibbs.scaled_fields(h, J, 0.05, None, (-1, 1))[1]
    ids = np.arange(K, dtype=np.uint32) + 5
    want = field_oracle.field_sweeps(gibbs.init_state(ids, n, s.field_seed, 0), ids, hs, Js, 20.0, plan, s.field_seed, 0, 3)
    assert np.array_equal(out.cpu().numpy(), want.astype(np.float32))
    want = field_oracle.field_sweeps(gibbs.init_state(ids, n, s.field_seed, 3), ids, hs, Js, 20.0, plan, s.field_seed, 3, 3)
    assert np.array_equal(again.cpu().numpy(), want.astype(np.float32))

    # one shared row with num_reads or a start naming the chains; the sampler's own sweep count; a start is not written to
    start = torch.from_numpy(_start(rng, K, n)).cuda()
    kept = start.clone()
    shared = s.sample_fields(lin, quad, 0.05, (-4, 4), (-1, 1), fields[0], start=start)
    assert s.field_sweep_count == 6 + 4 and shared.shape == (K, n) and torch.equal(start, kept)
    hs0 = np.broadcast_to(field_oracle.chain_fields(h, fields_np[0], 0.05, (-4, 4)), (K, n))
    want = field_oracle.field_sweeps(kept.cpu().numpy(), ids, hs0, Js, 20.0, plan, s.field_seed, 6, 4)
    assert np.array_equal(shared.cpu().numpy(), want.astype(np.float32))
    assert s.sample_fields(lin, quad, 0.05, (-4, 4), (-1, 1), fields[0], num_reads=3).shape == (3, n)
    for bad in (fields.cpu(), fields.double(), fields[:, :-1]):
        with pytest.raises(_lib.DvgError):
            s.sample_fields(lin, quad, 0.05, (-4, 4), (-1, 1), bad)
    with pytest.raises(_lib.DvgError):
        s.sample_fields(lin, quad, 0.05, (-4, 4), (-1, 1), fields, start=start[:4])
    assert s.field_sweep_count == 6 + 4 + 4

    # logit_fields: overwhelming logits are overwhelming evidence.  Logits of +-800 are fields of -+400 here, hs = -+20 against
    # at most 20 couplings of 0.25 and |prefactor h| <= 0.0025: z = 2 beta f clamps to -+87, the draw returns sign(logit)
    logits = torch.from_numpy(np.where(rng.uniform(size=(K, n)) < 0.5, -800.0, 800.0).astype(np.float32)).cuda()
    f = smp.logit_fields(logits, s.beta, 0.05)
    assert f.is_cuda and f.dtype == torch.float32 and torch.equal(f, -logits / 2)
    assert torch.equal(s.sample_fields(lin, quad, 0.05, None, (-1, 1), f, sweeps=1), torch.sign(logits))
