"""GPU checks of the simulated-quantum-annealing draw (``dvg_gibbs_sample_quantum``, "DVG SQA v1") against the numpy definition
(``tests/quantum_oracle.py``): ``Sliced.bits`` and ``Sliced.samples`` equal it bit for bit in every case.

``random70``: n = 70 (three words a row, 26 pad bits), spin 0 a hub of degree 66 (the second 64-entry chunk of the field sum);
P = 2 (the doubled neighbour), 16 (four chains a tile; with C = 5 the second tile is partial) and 64 (the 31 / 32 half boundary
and the 63 -> 0 wrap); S = 6 from sweep 3 under a falling kappa and a rising beta_slice.  ``zephyr128``: the project's Zephyr
subgraph, P = 32, prefactor and ranges that clamp couplings.  ``random40``: more tiles than the launch has workgroups (1024)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quantum_oracle as qo  # noqa: E402
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
H_RANGE, J_RANGE = (-4.0, 4.0), (-1.0, 1.0)
MAX_GRID = 1024  # QA_MAX_GRID, csrc/quantum.hip


@functools.lru_cache(maxsize=None)
def _zephyr_plan(n=128):
    mg, _ = graphs.get_graph_mapping(graphs.greedy_get_subgraph(n, SEED, graphs.zephyr_graph(12)))
    nodes, ei, ej = graphs.edges_of(mg)
    return graphs.build_plan(n, ei, ej), nodes


def _random_plan(n, hub_degree=0, p_edge=0.08):
    return support.random_plan(n, p_edge, hub_degree=hub_degree, with_nodes=True)


class _Case:
    """A graph with float32 fields h = 4 U(-1, 1), J = 5 U(-1, 1) on the device and on the host, and a sampler factory."""

    def __init__(self, name):
        self.plan, self.nodes = {"random70": lambda: _random_plan(70, 66), "random40": lambda: _random_plan(40),
                                 "zephyr128": _zephyr_plan}[name]()
        rng = np.random.default_rng(self.plan.n + 1)
        self.h = (4.0 * rng.uniform(-1, 1, self.plan.n)).astype(np.float32)
        self.J = (5.0 * rng.uniform(-1, 1, self.plan.n_edges)).astype(np.float32)
        self.lin, self.quad = torch.from_numpy(self.h).cuda(), torch.from_numpy(self.J).cuda()
        self.W = (self.plan.n + 31) // 32

    def sampler(self, sweep0=0, chain_offset=0, **kw):
        s = smp.GibbsSampler(self.plan, self.nodes, beta=kw.pop("beta", 1.0), sweeps=kw.pop("sweeps", 4), seed=SEED, device="cuda",
                             chain_offset=chain_offset, **kw)
        s.sqa_sweep_count = sweep0
        return s

    def draw(self, s, bs, kp, P, prefactor, **kw):
        return s.sample_quantum(self.lin, self.quad, prefactor, H_RANGE, J_RANGE, bs, kp, slices=P, **kw)

    def want(self, bs, kp, P, C, prefactor, sweep0=0, chain_offset=0, start_bits=None):
        hs, Js = gibbs.scaled_fields(self.h, self.J, prefactor, H_RANGE, J_RANGE)
        ids = (chain_offset + np.arange(C)).astype(np.uint32)
        return qo.draw(self.plan, hs, Js, bs, kp, ids, P, SEED ^ 0x73716131, sweep0, start_bits=start_bits)


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


def _tables(S, beta_slice=(0.05, 0.4), kappa=(1.2, 0.05)):
    """A rising beta_slice and a falling kappa, float32."""
    return np.linspace(*beta_slice, S).astype(np.float32), np.linspace(*kappa, S).astype(np.float32)


def _same(got, want, C, P, case):
    torch.cuda.synchronize()
    assert tuple(got.bits.shape) == (C, P, case.W) and got.bits.dtype == torch.int32 and got.bits.is_cuda
    assert tuple(got.samples.shape) == (C, case.plan.n) and got.samples.dtype == torch.float32
    assert got.slices == P and got.n == case.plan.n
    bits = got.bits.cpu().numpy().view(np.uint32)
    bad = np.argwhere(bits != want.bits)
    assert bad.size == 0, f"{len(bad)} words differ, the first at (chain, slice, word) {bad[0]}"
    assert np.array_equal(got.samples.cpu().numpy(), want.samples)
    if case.plan.n % 32:
        assert not (bits[..., -1] >> np.uint32(case.plan.n % 32)).any()  # pad bits are written as 0


@pytest.mark.parametrize("P", [2, 16, 64])
def test_random_graph_with_a_hub_equals_the_definition(P):
    case, C, S, sweep0, off = _case("random70"), 5, 6, 3, 4294967293  # (the chain ids wrap round 2^32)
    bs, kp = _tables(S)
    s = case.sampler(sweep0, off)
    got = case.draw(s, bs, kp, P, 0.3, num_reads=C)
    _same(got, case.want(bs, kp, P, C, 0.3, sweep0, off), C, P, case)
    assert s.sqa_sweep_count == sweep0 + S and s.sweep_count == 0 and s.calls == 0 and s._state is None


def test_zephyr_subgraph_with_clamped_couplings_energy_and_best():
    case, C, S, P = _case("zephyr128"), 6, 8, 32
    hs, Js = gibbs.scaled_fields(case.h, case.J, 0.3, H_RANGE, J_RANGE)
    assert (np.abs(Js) == 1.0).any() and (np.abs(Js) < 1.0).any()  # some couplings clamp
    bs, kp = _tables(S)
    got = case.draw(case.sampler(), torch.from_numpy(bs).cuda(), torch.from_numpy(kp).cuda(), P, 0.3, num_reads=C)  # device tables
    want = case.want(bs, kp, P, C, 0.3)
    _same(got, want, C, P, case)
    gh = smp.GraphHandle(case.plan, "cuda")
    e = got.energy(gh, case.lin, case.quad, prefactor=0.3, linear_range=H_RANGE, quadratic_range=J_RANGE)
    e_want = gibbs.energy(want.s.reshape(C * P, -1), hs, Js, np.asarray(case.plan.edge_i), np.asarray(case.plan.edge_j)).reshape(C, P)
    assert tuple(e.shape) == (C, P) and np.allclose(e.cpu().numpy(), e_want, rtol=0, atol=1e-9)
    best = got.best(gh, case.lin, case.quad, prefactor=0.3, linear_range=H_RANGE, quadratic_range=J_RANGE)
    first = np.array([int(np.flatnonzero(row == row.min())[0]) for row in e.cpu().numpy()])
    assert np.array_equal(best.cpu().numpy(), want.s[np.arange(C), first].astype(np.float32))
    assert abs(float(got.slice_overlap()) - qo.slice_overlap(want.s)) < 1e-12


def test_more_tiles_than_workgroups():
    case, P, S = _case("random40"), 2, 2
    C = 32 * MAX_GRID + 5  # 1025 tiles, the last one partial
    assert (C * P + 63) // 64 > MAX_GRID
    bs, kp = _tables(S)
    got = case.draw(case.sampler(), bs, kp, P, 0.3, num_reads=C)
    _same(got, case.want(bs, kp, P, C, 0.3), C, P, case)


def test_continuation_and_pad_bits():
    case, C, P, S = _case("random70"), 5, 16, 8
    bs, kp = _tables(S)
    whole = case.want(bs, kp, P, C, 0.3)
    s = case.sampler()
    half = case.draw(s, bs[:4], kp[:4], P, 0.3, num_reads=C)
    before = half.bits.clone()
    rest = case.draw(s, bs[4:], kp[4:], P, 0.3, start=half.bits)
    _same(rest, whole, C, P, case)
    assert torch.equal(half.bits, before) and rest.bits.data_ptr() != half.bits.data_ptr()  # (the call's own copy)
    assert s.sqa_sweep_count == 8
    # set pad bits on input are ignored
    dirty = before.clone()
    dirty[..., -1] |= torch.tensor(np.int32(-1) << (case.plan.n % 32), dtype=torch.int32, device="cuda")
    assert not torch.equal(dirty, before)
    s.sqa_sweep_count = 4
    _same(case.draw(s, bs[4:], kp[4:], P, 0.3, start=dirty, num_reads=C), whole, C, P, case)


def test_kappa_zero_leaves_the_slices_independent():
    case, C, P, S = _case("random70"), 24, 16, 6
    bs, kp = np.full(S, 0.1, np.float32), np.zeros(S, np.float32)
    got = case.draw(case.sampler(), bs, kp, P, 0.3, num_reads=C)
    want = case.want(bs, kp, P, C, 0.3)
    _same(got, want, C, P, case)
    q, q_want = float(got.slice_overlap()), qo.slice_overlap(want.s)
    print("slice overlap", q, "oracle", q_want)
    assert abs(q - q_want) <= 6.0 / np.sqrt(C * P * case.plan.n)
    rows = got.bits.cpu().numpy()
    assert all(len({rows[c, k].tobytes() for k in range(P)}) == P for c in range(C))  # the slices differ from one another
    assert q < 0.5


def test_large_kappa_locks_equal_slices():
    case, C, P, S = _case("random70"), 5, 16, 4
    bs, kp = np.full(S, 0.1, np.float32), np.full(S, 20.0, np.float32)
    one = gibbs.init_state(np.arange(C), case.plan.n, 5, 0)
    start = trace_oracle.pack(np.repeat(one[:, None, :], P, axis=1))
    got = case.draw(case.sampler(), bs, kp, P, 0.3, start=torch.from_numpy(start.view(np.int32)).cuda())
    _same(got, case.want(bs, kp, P, C, 0.3, start_bits=start), C, P, case)
    assert np.array_equal(got.bits.cpu().numpy().view(np.uint32), start)  # they stay equal, and where they were
    assert float(got.slice_overlap()) == 1.0


def test_sample_ising_quantum_reads_and_unchanged_plain_reads():
    case = _case("random70")
    p = case.plan
    rng = np.random.default_rng(9)
    h = {v: float(x) for v, x in zip(case.nodes, rng.uniform(-1, 1, p.n))}
    J = {(int(a), int(b)): float(x) for a, b, x in zip(p.edge_i, p.edge_j, rng.uniform(-1, 1, p.n_edges))}
    lin = torch.tensor([h[v] for v in case.nodes], dtype=torch.float32, device="cuda")
    quad = torch.tensor([J[(int(a), int(b))] for a, b in zip(p.edge_i, p.edge_j)], dtype=torch.float32, device="cuda")
    s = case.sampler(beta=2.0, sweeps=5)
    ss = s.sample_ising(h, J, num_reads=8, transverse_field_range=(3.0, 0.05), num_slices=16, num_sweeps=12)
    assert s.sqa_sweep_count == 12 and s.sweep_count == 0 and s.anneal_sweep_count == 0
    t = case.sampler(beta=2.0, sweeps=5)
    bs, kp = smp.transverse_schedule(2.0, 3.0, 0.05, 12, 16)
    ref = t.sample_quantum(lin, quad, 1.0, None, None, bs, kp, slices=16, num_reads=8)
    assert torch.equal(ss.device_tensor, ref.samples)
    e = F.grbm_energy(ref.samples, lin, quad, s.graph)
    assert torch.equal(ss.device_energy, e) and np.array_equal(ss.record.energy, e.cpu().numpy())
    assert np.array_equal(ss.record.sample, ref.samples.cpu().numpy().astype(np.int8))
    hs, Js = gibbs.scaled_fields(lin.cpu().numpy(), quad.cpu().numpy(), 1.0, None, None)
    want = qo.draw(p, hs, Js, bs, kp, np.arange(8), 16, SEED ^ 0x73716131, 0)
    assert np.array_equal(ref.samples.cpu().numpy(), want.samples)
    # the default of num_sweeps is the sampler's own
    again = case.sampler(beta=2.0, sweeps=5).sample_ising(h, J, num_reads=8, transverse_field_range=(3.0, 0.05), num_slices=16)
    b5, k5 = smp.transverse_schedule(2.0, 3.0, 0.05, 5, 16)
    assert np.array_equal(again.device_tensor.cpu().numpy(), qo.draw(p, hs, Js, b5, k5, np.arange(8), 16, SEED ^ 0x73716131, 0).samples)
    # without the new names: the plain draw, as before
    plain = case.sampler(beta=2.0, sweeps=5).sample_ising(h, J, num_reads=8)
    adj_ptr, adj_idx, adj_eid = gibbs.build_csr(p.n, np.asarray(p.edge_i, np.int64), np.asarray(p.edge_j, np.int64))
    st = gibbs.gibbs_sweeps(gibbs.init_state(np.arange(8), p.n, SEED, 0), np.arange(8), hs, Js, 2.0, p.order, p.class_ptr, adj_ptr,
                            adj_idx, adj_eid, SEED, 0, 5)
    assert np.array_equal(plain.record.sample, st)


def test_rejected_call_leaves_the_slices_untouched():
    case, C, P = _case("random70"), 5, 16
    gh = smp.GraphHandle(case.plan, "cuda")
    rng = np.random.default_rng(3)
    words = rng.integers(-2 ** 31, 2 ** 31, size=(C, P, case.W), dtype=np.int64).astype(np.int32)
    bits = torch.from_numpy(words).cuda()
    out = torch.full((C, case.plan.n), 7.0, dtype=torch.float32, device="cuda")
    tb, tk = torch.full((4,), 0.1, device="cuda"), torch.full((4,), 0.3, device="cuda")
    L = _lib.lib()
    for kw in (dict(n_slices=12), dict(n_slices=128), dict(n_sweeps=0), dict(n_chains=0), dict(prefactor=float("nan")),
               dict(n_chains=2 ** 27, n_slices=16)):
        a = dict(prefactor=0.3, n_chains=C, n_slices=P, n_sweeps=4)
        a.update(kw)
        for init in (0, 1):
            rc = L.dvg_gibbs_sample_quantum(gh.ptr, case.lin.data_ptr(), case.quad.data_ptr(), a["prefactor"], -4.0, 4.0, -1.0, 1.0,
                                            tb.data_ptr(), tk.data_ptr(), bits.data_ptr(), a["n_chains"], a["n_slices"], 0, SEED, 0,
                                            a["n_sweeps"], init, out.data_ptr(), _lib.stream_ptr())
            assert rc in (-1, -4), (kw, rc)
    torch.cuda.synchronize()
    assert np.array_equal(bits.cpu().numpy(), words) and bool((out == 7.0).all())
