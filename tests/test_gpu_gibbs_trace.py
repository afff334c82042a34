"""GPU parity of the traced draw (``dvg_gibbs_sample_traced``, "DVG trace v1": the plain draw with the chains' states after
chosen sweeps written out one bit per spin from inside the kernel) against the definition in ``tests/trace_oracle.py``, and
of the Python surface built on it.

Everything is integers: the trace equals the helper's word for word, ``state`` and ``samples_out`` equal
``dvg_gibbs_sample``'s under the same key bit for bit; no tolerance anywhere.

Shapes, dispatch and conventions: those of ``tests/test_gpu_gibbs_ais.py`` (rebuilt here) -- sweeps 6 .. 12, h_range (-4, 4),
j_range (-1, 1), a nonzero first chain id, chain counts one more than a multiple of the chains per workgroup, a guard row
behind ``state`` and ``samples_out``, and here a guard record of a sentinel word behind the last chain's trace.  The shapes
cover the lane forms at LPC 32 and 64, one and four waves, NR 1 and 2, MAXS 12 and 20; the rolled forms at 16 x 1, 64 x 4
and 64 x 16; ``random77`` (n % 32 = 13, n_pad = 80: the last word's row ends in mid-word with another chain's row behind
it); ``cliques`` (n = 700).  The helper's history of a (graph, chains, start) is computed once and shared by the cases."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, dev, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP0, SWEEPS = 6, 7
GUARD_STATE, GUARD_OUT, GUARD_WORD = 55, 7.0, 0x5A5A5A5A
RECORD_RULES = [(0, 1), (1, 2), (2, 3)]  # (burn_in, thin)


# ------------------------------------------------------------------------------------------------ graphs
_solver_plan = functools.partial(support.solver_plan, with_nodes=True)


def _random_plan(n=77, p_edge=0.35):
    """Degrees beyond 20 (two rounds of the neighbour sum), spin 3 isolated, an odd spin count."""
    assert n % 32 == 13 and ((n + 15) & ~15) == 80
    return support.random_plan(n, p_edge, isolated=3, max_degree_above=20)


_clique_plan = support.clique_plan


# name: (graph key, plan, chains, sweeps, gibbs_generic, parameters); the 530-chain shape runs 5 sweeps (the helper's time):
# enough for every record rule to record
def _shape(name):
    solver = dict(h_scale=0.05, j_scale=5.0, prefactor=0.05, beta=20.0, id0=1000)
    table = {
        "pegasus64": ("pegasus64", lambda: _solver_plan("pegasus", 64)[0], 5, SWEEPS, 0, solver),
        "zephyr128": ("zephyr128", lambda: _solver_plan("zephyr", 128)[0], 5, SWEEPS, 0, solver),
        "zephyr512": ("zephyr512", lambda: _solver_plan("zephyr", 512)[0], 9, SWEEPS, 0, solver),
        "zephyr512-one-row": ("zephyr512", lambda: _solver_plan("zephyr", 512)[0], 9, SWEEPS, 2, solver),
        "zephyr512-rolled": ("zephyr512", lambda: _solver_plan("zephyr", 512)[0], 9, SWEEPS, 1, solver),
        "zephyr1024x41": ("zephyr1024", lambda: _solver_plan("zephyr", 1024)[0], 41, SWEEPS, 0, solver),
        "zephyr1024x530": ("zephyr1024", lambda: _solver_plan("zephyr", 1024)[0], 530, 5, 0, solver),
        "random77": ("random77", _random_plan, 19, SWEEPS, 0, dict(h_scale=0.5, j_scale=2.0, prefactor=0.3, beta=1.5, id0=7)),
        "cliques": ("cliques", _clique_plan, 21, SWEEPS, 0, dict(h_scale=0.5, j_scale=1.0, prefactor=0.4, beta=1.2, id0=3)),
    }
    key, make, C, sweeps, generic, p = table[name]
    return key, make(), C, sweeps, generic, p


SHAPES = ["pegasus64", "zephyr128", "zephyr512", "zephyr512-one-row", "zephyr512-rolled", "zephyr1024x41", "zephyr1024x530",
          "random77", "cliques"]
# the kernel form each shape's draw takes, as the draw's plan names it: _setup asserts it
FORMS = {
    "pegasus64": ("lane", dict(LPC=32, WAVES=1, MB=4, NR=1, MAXS=12)),
    "zephyr128": ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12)),
    "zephyr512": ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=12)),
    "zephyr512-one-row": ("lane", dict(LPC=64, WAVES=4, MB=5, NR=1, MAXS=12)),
    "zephyr512-rolled": ("rolled", dict(LPC=64, WAVES=4)),
    "zephyr1024x41": ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20)),
    "zephyr1024x530": ("rolled", dict(LPC=64, WAVES=16)),
    "random77": ("rolled", dict(LPC=16, WAVES=1)),
    "cliques": ("lane", dict(LPC=64, WAVES=4, MB=4, NR=1, MAXS=20)),
}


# ------------------------------------------------------------------------------------------------ the raw ABI
class _Draw:
    """dvg_gibbs_sample_traced / dvg_gibbs_sample on one graph and one (h, J)."""

    def __init__(self, plan, h, J, prefactor):
        self.plan, self.prefactor = plan, float(prefactor)
        self.W = (plan.n + 31) // 32
        self.gh = smp.GraphHandle(plan, "cuda")
        self.lin, self.quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()

    def buffers(self, start, M=0):
        """``state``, ``samples_out`` with a guard row behind the last chain and the trace of M records per chain with a guard
        record behind the last chain's; ``start``: (C, n) int8."""
        C = start.shape[0]
        state = torch.full((C + 1, self.plan.n), GUARD_STATE, dtype=torch.int8, device="cuda")
        state[:C] = torch.from_numpy(start).cuda()
        out = torch.full((C + 1, self.plan.n), GUARD_OUT, dtype=torch.float32, device="cuda")
        trace = torch.full((C * M + 1, self.W), GUARD_WORD, dtype=torch.int32, device="cuda")
        return state, out, trace

    def raw(self, beta, state_ptr, C, id0, seed, sweep0, sweeps, init, out_ptr, trace_ptr, burn_in, thin, dyn=None):
        return _lib.lib().dvg_gibbs_sample_traced(self.gh.ptr, self.lin.data_ptr(), self.quad.data_ptr(), self.prefactor, -4.0, 4.0,
                                                  -1.0, 1.0, float(beta), state_ptr, C, id0, seed, sweep0, sweeps, init, out_ptr,
                                                  trace_ptr, burn_in, thin, dyn, _lib.stream_ptr())

    def traced(self, bufs, beta, id0, seed, sweep0, sweeps, init, burn_in, thin):
        state, out, trace = bufs
        C = int(state.shape[0]) - 1
        _lib.check(self.raw(beta, state.data_ptr(), C, id0, seed, sweep0, sweeps, init, out.data_ptr(), trace.data_ptr(), burn_in, thin),
                   "dvg_gibbs_sample_traced")
        torch.cuda.synchronize()

    def plain(self, state, out, beta, id0, seed, sweep0, sweeps, init):
        C = int(state.shape[0]) - 1
        _lib.check(_lib.lib().dvg_gibbs_sample(self.gh.ptr, self.lin.data_ptr(), self.quad.data_ptr(), self.prefactor, -4.0,
                                               4.0, -1.0, 1.0, float(beta), state.data_ptr(), C, id0, seed, sweep0, sweeps,
                                               init, out.data_ptr(), None, _lib.stream_ptr()), "dvg_gibbs_sample")
        torch.cuda.synchronize()


def _fields(key, plan, C, p):
    rng = np.random.default_rng(plan.n + C)
    h = (p["h_scale"] * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (p["j_scale"] * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    prepared = np.where(rng.uniform(size=(C, plan.n)) < 0.5, -1, 1).astype(np.int8)
    return h, J, prepared


def _setup(name):
    key, plan, C, sweeps, generic, p = _shape(name)
    with _lib.option_scope(gibbs_generic=generic):
        got = dev.gibbs_draw_plan(plan, C, "trace")
    assert (got["form"], got["params"]) == FORMS[name], got
    assert C % got["chains_per_workgroup"] != 0  # (the last workgroup is partly idle)
    h, J, prepared = _fields(key, plan, C, p)
    return plan, C, sweeps, generic, p, _Draw(plan, h, J, p["prefactor"]), prepared


_HISTORIES = {}


def _history(name, init):
    """The helper's history of a shape's draw (one oracle call per sweep), computed once and left unchanged: the three shapes
    on zephyr512 share theirs, every record rule selects from it."""
    key, plan, C, sweeps, _generic, p = _shape(name)
    if (key, C, sweeps, init) not in _HISTORIES:
        h, J, prepared = _fields(key, plan, C, p)
        hs, Js = gibbs.scaled_fields(h, J, p["prefactor"], (-4, 4), (-1, 1))
        ids = np.arange(C, dtype=np.uint32) + p["id0"]
        hist = trace_oracle.history(plan, hs, Js, p["beta"], ids, SEED, SWEEP0, sweeps, start=None if init else prepared)
        hist.states.setflags(write=False)
        _HISTORIES[(key, C, sweeps, init)] = hist
    return _HISTORIES[(key, C, sweeps, init)]


def _check(d, bufs, want, C, where):
    """The trace equals the helper's word for word, the guards are untouched, the final spins are the helper's."""
    state, out, trace = bufs
    M, W = want.bits.shape[1], d.W
    got = trace.cpu().numpy().view(np.uint32)
    assert got.shape == (C * M + 1, W)
    assert (got[C * M] == GUARD_WORD).all(), f"written past the last chain's trace ({where})"
    got_state, got_out = state.cpu().numpy(), out.cpu().numpy()
    assert (got_state[C] == GUARD_STATE).all() and (got_out[C] == GUARD_OUT).all(), f"written past the last chain ({where})"
    mism = int((got[:C * M].reshape(C, M, W) != want.bits).sum())
    assert mism == 0, f"{mism} of {C * M * W} trace words differ from the helper ({where})"
    assert np.array_equal(got_state[:C], want.spins) and np.array_equal(got_out[:C], want.spins.astype(np.float32)), where
    if d.plan.n % 32:
        assert (got[:C * M, -1] >> np.uint32(d.plan.n % 32) == 0).all(), f"bits of spins >= n set ({where})"
    return got[:C * M].reshape(C, M, W)


@pytest.mark.parametrize("burn_in,thin", RECORD_RULES)
@pytest.mark.parametrize("name", SHAPES)
def test_trace_matches_the_helper(name, burn_in, thin):
    """init = 1 (fresh chains) and init = 0 (from a prepared state): the trace word for word, state and samples_out those of
    dvg_gibbs_sample under the same key (GPU against GPU), the last record the packed samples_out when the last sweep is
    recorded."""
    plan, C, sweeps, generic, p, d, prepared = _setup(name)
    M = (sweeps - burn_in) // thin
    assert M >= 1
    for init in (1, 0):
        where = f"{name}, burn_in={burn_in}, thin={thin}, init={init}"
        want = trace_oracle.trace_of(_history(name, init), burn_in, thin)
        assert want.bits.shape == (C, M, d.W)
        bufs = d.buffers(prepared, M)
        s_plain, o_plain, _t = d.buffers(prepared)
        with _lib.option_scope(gibbs_generic=generic):
            d.traced(bufs, p["beta"], p["id0"], SEED, SWEEP0, sweeps, init, burn_in, thin)
            d.plain(s_plain, o_plain, p["beta"], p["id0"], SEED, SWEEP0, sweeps, init)
        got = _check(d, bufs, want, C, where)
        assert torch.equal(bufs[0], s_plain) and torch.equal(bufs[1], o_plain), f"not the plain draw's spins ({where})"
        last_recorded = (sweeps - burn_in) % thin == 0
        assert last_recorded == (want.sweeps[-1] == sweeps)
        if last_recorded:
            assert np.array_equal(got[:, M - 1], trace_oracle.pack(bufs[1][:C].cpu().numpy())), where
        else:  # (the chains moved in the unrecorded sweeps behind it)
            assert not np.array_equal(got[:, M - 1], trace_oracle.pack(bufs[1][:C].cpu().numpy())), where
        assert len({want.bits[:, m].tobytes() for m in range(M)}) == M  # (the records differ: the chains move)


@pytest.mark.parametrize("name", ["pegasus64", "zephyr512", "zephyr512-rolled", "zephyr1024x41", "random77"])
def test_two_calls_continue_the_trace(name):
    """4 sweeps, then 3 with sweep0 advanced and state handed on, at thin = 1: the concatenation of the two traces is the
    one-call trace of 7 (and the helper's)."""
    plan, C, sweeps, generic, p, d, prepared = _setup(name)
    assert sweeps == 7
    want = trace_oracle.trace_of(_history(name, 1), 0, 1)
    one = d.buffers(prepared, 7)
    a = d.buffers(prepared, 4)
    with _lib.option_scope(gibbs_generic=generic):
        d.traced(one, p["beta"], p["id0"], SEED, SWEEP0, 7, 1, 0, 1)
        d.traced(a, p["beta"], p["id0"], SEED, SWEEP0, 4, 1, 0, 1)
        b = d.buffers(a[0][:C].cpu().numpy(), 3)
        d.traced(b, p["beta"], p["id0"], SEED, SWEEP0 + 4, 3, 0, 0, 1)
    whole = _check(d, one, want, C, f"{name}, one call")
    parts = []
    for bufs, M in ((a, 4), (b, 3)):
        words = bufs[2].cpu().numpy().view(np.uint32)
        assert (words[C * M] == GUARD_WORD).all()
        parts.append(words[:C * M].reshape(C, M, d.W))
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    assert torch.equal(b[0], one[0]) and torch.equal(b[1], one[1])


def test_invalid_arguments_launch_nothing():
    """A NULL trace, a negative burn_in, thin < 1, a rule that records nothing and a non-NULL dyn are DVG_E_INVALID; all three
    buffers keep their fill."""
    plan, C, _sweeps, _generic, p, d, prepared = _setup("zephyr128")
    state, out, trace = d.buffers(prepared, SWEEPS)
    before = state.clone()
    tp = trace.data_ptr()
    dyn = torch.zeros(64, dtype=torch.uint8, device="cuda")
    #        trace sweeps burn_in thin dyn
    cases = [(None, SWEEPS, 0, 1, None), (tp, SWEEPS, -1, 1, None), (tp, SWEEPS, 0, 0, None), (tp, SWEEPS, 0, -2, None),
             (tp, SWEEPS, SWEEPS, 1, None), (tp, SWEEPS, 0, SWEEPS + 1, None), (tp, SWEEPS, 5, 3, None), (tp, 0, 0, 1, None),
             (tp, SWEEPS, 0, 1, dyn.data_ptr())]
    for trace_ptr, sweeps, burn_in, thin, dyn_ptr in cases:
        rc = d.raw(p["beta"], state.data_ptr(), C, p["id0"], SEED, SWEEP0, sweeps, 1, out.data_ptr(), trace_ptr, burn_in, thin, dyn_ptr)
        assert rc == -1, (sweeps, burn_in, thin, rc, _lib.lib().dvg_last_error())
    torch.cuda.synchronize()
    assert torch.equal(state, before) and (out == GUARD_OUT).all() and (trace == GUARD_WORD).all()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_sample_trace_and_the_other_streams():
    """``sample_trace`` -> ``Trace`` whose ``unpack()`` is the helper's history; ``trace_sweep_count`` advances; a training
    draw made before and one made after traced draws are bit for bit what they are without them."""
    plan, nodes = _solver_plan("zephyr", 128)
    rng = np.random.default_rng(2)
    h = (0.05 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    mk = lambda: smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5,  # noqa: E731
                                  h_range=(-4, 4), j_range=(-1, 1))
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    hs, Js = gibbs.scaled_fields(h, J, 0.05, (-4, 4), (-1, 1))
    C, n, R = 24, plan.n, 9
    ids = np.arange(R, dtype=np.uint32) + 5

    ref = mk()
    ref_draws = [ref.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone() for _ in range(2)]

    s = mk()
    assert s.trace_seed == SEED ^ 0x74726163 and s.trace_sweep_count == 0
    first = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone()
    before = (s._state.clone(), s._state.data_ptr(), s.sweep_count, s.calls, s.cond_sweep_count, s.anneal_sweep_count,
              s.ais_sweep_count, s.pt_sweep_count)

    # fresh chains, the sampler's own 4 sweeps, every sweep recorded: sweeps 0 .. 3 under the trace key
    t = s.sample_trace(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=R)
    assert isinstance(t, smp.Trace) and s.trace_sweep_count == 4
    assert t.bits.shape == (R, 4, 4) and t.bits.dtype == torch.int32 and t.bits.is_cuda
    assert t.samples.shape == (R, n) and t.samples.dtype == torch.float32 and t.state.dtype == torch.int8
    assert np.array_equal(t.sweeps, [1, 2, 3, 4]) and t.sweeps.dtype == np.int64
    want = trace_oracle.history(plan, hs, Js, 20.0, ids, s.trace_seed, 0, 4)
    assert np.array_equal(t.unpack().cpu().numpy(), want.states[1:].transpose(1, 0, 2).astype(np.float32))
    assert np.array_equal(t.samples.cpu().numpy(), want.states[-1].astype(np.float32))
    assert np.array_equal(t.state.cpu().numpy(), want.states[-1])
    assert torch.equal(smp.Trace(t.bits.cpu(), None, None, t.sweeps, n).unpack(), t.unpack().cpu())

    # continued from its state (float32 start), 9 sweeps, burn_in 2, thin 3: sweeps 4 .. 12, records after k + 1 = 5, 8
    start = t.samples.clone()
    t2 = s.sample_trace(lin, quad, 0.05, (-4, 4), (-1, 1), start=start, num_sweeps=9, burn_in=2, thin=3)
    assert s.trace_sweep_count == 13 and np.array_equal(t2.sweeps, [5, 8]) and torch.equal(start, t.samples)
    want2 = trace_oracle.history(plan, hs, Js, 20.0, ids, s.trace_seed, 4, 9, start=want.states[-1])
    assert np.array_equal(t2.unpack().cpu().numpy(), want2.states[[5, 8]].transpose(1, 0, 2).astype(np.float32))
    assert np.array_equal(t2.state.cpu().numpy(), want2.states[-1])

    # the training, conditional, annealed, AIS and exchange streams never noticed
    assert s._state.data_ptr() == before[1] and torch.equal(s._state, before[0])
    assert (s.sweep_count, s.calls, s.cond_sweep_count, s.anneal_sweep_count, s.ais_sweep_count, s.pt_sweep_count) == before[2:]
    second = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)
    assert torch.equal(first, ref_draws[0]) and torch.equal(second, ref_draws[1])
    s.reset()
    assert s.trace_sweep_count == 0
    with pytest.raises(ValueError):
        s.sample_trace(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=R, burn_in=4)
    assert s.trace_sweep_count == 0
