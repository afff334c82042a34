"""GPU checks of ``dvg_packed_correlation`` ("DVG corr v1") -- the sums of s_i s_j over bit-packed rows for EVERY pair of spins,
and of s_i -- against the numpy definition (``tests/correlation_oracle.py``): exact equality, the results are integers.  Rows:
traced draws (``dvg_gibbs_sample_traced``) on ``pegasus64`` (one column tile) and ``zephyr1024`` (16 tiles, 136 tile pairs),
and random words with noise in the bits of spins >= n for n = 77 (two tiles, the second partial), 33 and 1.  Row counts
below, at and over one 64-row word, several words with a partial last one; flat sets, the (C, M, W) layout as a view of a
larger trace with sliced chains and records, padded rows.  Per case a guard element behind each output, ``accumulate = 1``
onto random contents, ``spin_sum = NULL``, the diagonal and the symmetry, and two calls compared.  Rows beyond one slab and
one chunk: slabs of one chunk, of several chunks, and of the most a slab may hold.  And the Python surface built on it."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correlation_oracle as co  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -0x0123456789ABCDEF
FILL = 0x7777777777
CONTENTS = ["pegasus64", "zephyr1024", "random77", "random33", "random1"]
ROWS = [1, 63, 64, 65, 129, 287, 910]
TRACES = [(1, 5), (2, 1), (41, 6), (65, 3), (127, 2)]  # (chains C, records M) of a view into the (130, 7, W) case
P = dict(h_scale=0.05, j_scale=5.0, prefactor=0.05)


_solver_plan = functools.partial(support.solver_plan, with_nodes=True)


def _fields(plan):
    rng = np.random.default_rng(plan.n)
    h = (P["h_scale"] * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (P["j_scale"] * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    return torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()


@functools.lru_cache(maxsize=None)
def _case(name):
    """``(n, bits (130, 7, W) int32 on the device)``, computed once: a traced draw at beta = 2 of 130 chains x 7 records
    (``pegasus64``, ``zephyr1024``) or as many random words (``random77``, ``random33``, ``random1``).  Flat tests take rows of
    its (910, W) view, trace tests views of its chains and records."""
    if name.startswith("random"):
        n = int(name[6:])
        W = (n + 31) // 32
        noise = np.random.default_rng(n).integers(0, 2 ** 32, size=(130, 7, W), dtype=np.uint64).astype(np.uint32)
        if n % 32:
            assert (noise[..., -1] >> np.uint32(n % 32)).any()  # bits of spins >= n are set
        return n, torch.from_numpy(noise.view(np.int32)).cuda()
    plan = _solver_plan("pegasus", 64)[0] if name == "pegasus64" else _solver_plan("zephyr", 1024)[0]
    C, S = 130, 7
    gh = smp.GraphHandle(plan, "cuda")
    lin, quad = _fields(plan)
    state = torch.empty((C, plan.n), dtype=torch.int8, device="cuda")
    traced = torch.empty((C, S, (plan.n + 31) // 32), dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().dvg_gibbs_sample_traced(gh.ptr, lin.data_ptr(), quad.data_ptr(), P["prefactor"], -4.0, 4.0, -1.0, 1.0, 2.0,
                                                  state.data_ptr(), C, 1000, SEED, 6, S, 1, None, traced.data_ptr(), 0, 1, None,
                                                  _lib.stream_ptr()), "dvg_gibbs_sample_traced")
    torch.cuda.synchronize()
    return plan.n, traced


@functools.lru_cache(maxsize=None)
def _unpacked(name):
    """The case's 910 pooled rows as (910, n) int64 +-1 on the host, unpacked once."""
    n, full = _case(name)
    return co.unpack(full.cpu().numpy(), n)


def _want_of_rows(x):
    return x.sum(axis=0), x.T @ x


def _outputs(n, rng=None):
    """``spin_sum`` and ``pair_sum`` with a guard element behind each; ``rng``: None (a fill to be overwritten) or a generator
    (random int64 contents to add onto)."""
    outs = []
    for elems in (n, n * n):
        v = np.full(elems + 1, FILL, dtype=np.int64) if rng is None else rng.integers(-10 ** 12, 10 ** 12, size=elems + 1)
        v[elems] = GUARD
        outs.append(torch.from_numpy(v).cuda())
    return outs


def _layout(t, W):
    """``(rows, row_stride, groups, group_stride)`` of a 2-D or 3-D tensor of packed rows, as the C entry takes them."""
    rows = int(t.shape[-2])
    rs = int(t.stride(-2)) if rows > 1 else W
    if t.dim() == 2:
        return rows, rs, 1, 0
    return rows, rs, int(t.shape[0]), int(t.stride(0)) if t.shape[0] > 1 else 0


def _raw(bits, spins, spin, pair, accumulate=0, ws=None, ws_bytes=None, **over):
    """The C entry on tensors, the layout taken from them; ``over`` replaces single arguments (``n`` among them)."""
    n = spins
    W = (n + 31) // 32
    rows, rs, groups, gs = _layout(bits, W) if bits is not None else (1, W, 1, 0)
    kw = dict(rows=rows, rs=rs, groups=groups, gs=gs, n=n)
    kw.update(over)
    L = _lib.lib()
    if ws is None:  # (the query gives 0 for arguments the entry rejects)
        need = int(L.dvg_packed_correlation_workspace_bytes(kw["rows"], kw["groups"], kw["n"]))
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    rc = L.dvg_packed_correlation(ptr(bits), kw["rows"], kw["rs"], kw["groups"], kw["gs"], kw["n"], ptr(spin), ptr(pair), accumulate,
                                  ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _dense(t):
    return t.contiguous().cpu().numpy()


def _check_exact(bits, n, want=None, seed=0):
    """The C entry on (a view of) a device tensor against the helper on its dense copy (or ``want``): both outputs with
    guards, the diagonal and the symmetry; a second call compared with the first; ``accumulate = 1`` onto random contents;
    ``spin_sum = NULL``.  Returns the expected pair."""
    want_spin, want_pair = co.sums(_dense(bits), n) if want is None else want
    T = int(np.prod(bits.shape[:-1]))
    err = lambda: _lib.lib().dvg_last_error()  # noqa: E731
    spin, pair = _outputs(n)
    assert _raw(bits, n, spin, pair) == 0, err()
    got_spin, got_pair = spin.cpu().numpy(), pair.cpu().numpy()
    assert got_spin[-1] == GUARD and got_pair[-1] == GUARD, "written past an output"
    square = got_pair[:-1].reshape(n, n)
    assert (np.diag(square) == T).all() and np.array_equal(square, square.T)
    assert np.array_equal(got_spin[:-1], want_spin) and np.array_equal(square, want_pair)
    spin2, pair2 = _outputs(n)
    assert _raw(bits, n, spin2, pair2) == 0, err()
    assert torch.equal(spin2, spin) and torch.equal(pair2, pair)  # the same bits on every call
    rng = np.random.default_rng(seed + T)
    spin, pair = _outputs(n, rng)
    base_spin, base_pair = spin.cpu().numpy().copy(), pair.cpu().numpy().copy()
    assert _raw(bits, n, spin, pair, accumulate=1) == 0, err()
    got_spin, got_pair = spin.cpu().numpy(), pair.cpu().numpy()
    assert got_spin[-1] == GUARD and got_pair[-1] == GUARD
    assert np.array_equal(got_spin[:-1], base_spin[:-1] + want_spin) and np.array_equal(got_pair[:-1], base_pair[:-1] + want_pair.reshape(-1))
    spin, pair = _outputs(n, rng)
    base_spin, base_pair = spin.clone(), pair.cpu().numpy().copy()
    assert _raw(bits, n, None, pair, accumulate=1) == 0, err()
    got_pair = pair.cpu().numpy()
    assert got_pair[-1] == GUARD and np.array_equal(got_pair[:-1], base_pair[:-1] + want_pair.reshape(-1))
    assert torch.equal(spin, base_spin)  # (untouched: NULL was passed)
    spin, pair = _outputs(n)
    assert _raw(bits, n, None, pair) == 0, err()
    got_pair = pair.cpu().numpy()
    assert got_pair[-1] == GUARD and np.array_equal(got_pair[:-1], want_pair.reshape(-1))
    return want_spin, want_pair


# ------------------------------------------------------------------------------------------------ flat sets
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", CONTENTS)
def test_flat_sets_are_exact(name, rows):
    n, full = _case(name)
    a = full.reshape(-1, full.shape[-1])[:rows].contiguous()
    want_spin, want_pair = _check_exact(a, n, want=_want_of_rows(_unpacked(name)[:rows]))
    assert want_pair.shape == (n, n) and want_spin.shape == (n,)


def test_the_traced_rows_are_the_draws_records():
    """The traced cases hold spins that move and pairs that are correlated: the matrix is not T times a sign pattern."""
    for name in ("pegasus64", "zephyr1024"):
        n, bits = _case(name)
        assert (bits != bits[:, :1]).any()
        _spin, pair = _want_of_rows(_unpacked(name))
        off = np.abs(pair[~np.eye(n, dtype=bool)])
        assert (off < 910).any() and len(np.unique(off)) >= 8


# ------------------------------------------------------------------------------------------------ views of a trace
@pytest.mark.parametrize("C,M", TRACES)
@pytest.mark.parametrize("name", ["pegasus64", "random77"])
def test_trace_layout_as_a_view_with_sliced_chains_and_records(name, C, M):
    n, full = _case(name)
    a = full[3:3 + C, 1:1 + M]  # (a view: group stride 7 W, row stride W)
    assert a.data_ptr() != full.data_ptr() and (a.is_contiguous() == (C == 1 or M == 7))
    x = _unpacked(name).reshape(130, 7, n)[3:3 + C, 1:1 + M].reshape(-1, n)
    _check_exact(a, n, want=_want_of_rows(x))
    b = full[1::3, ::2][:C]  # every third chain, every second record
    x = _unpacked(name).reshape(130, 7, n)[1::3, ::2][:C].reshape(-1, n)
    _check_exact(b, n, want=_want_of_rows(x))


def test_padded_rows():
    """``row_stride = W + 3`` with the padding words set at random, flat and as groups."""
    for name, rows in (("random77", 129), ("pegasus64", 65), ("random1", 70), ("random33", 910)):
        n, full = _case(name)
        W = full.shape[-1]
        a = full.reshape(-1, W)[:rows]
        pa = torch.from_numpy(np.random.default_rng(rows).integers(-2 ** 31, 2 ** 31, size=(rows, W + 3)).astype(np.int32)).cuda()
        pa[:, :W] = a
        assert pa[:, :W].stride(0) == W + 3
        _check_exact(pa[:, :W], n, want=_want_of_rows(_unpacked(name)[:rows]))
    n, full = _case("random77")
    W = full.shape[-1]
    padded = torch.from_numpy(np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, size=(41, 5, W + 3)).astype(np.int32)).cuda()
    padded[:, :, :W] = full[:41, :5]
    _check_exact(padded[:, :, :W], n, want=_want_of_rows(_unpacked("random77").reshape(130, 7, n)[:41, :5].reshape(-1, n)))


# ------------------------------------------------------------------------------------------------ slabs and the wrap bound
def test_more_rows_than_a_slab_may_hold():
    """n = 33, 300 000 rows of patterned words: more than the 2^18 rows one slab may hold (``CR_SLAB_ROWS``, DESIGN.md: the
    bound under which a 32-bit count cannot wrap), 293 chunks in as many slabs of one tile pair.  Expected from numpy."""
    n, T = 33, 300000
    assert T > F.PACKED_CORRELATION_SLAB_ROWS == 1 << 18
    r = np.arange(T, dtype=np.uint64)
    words = np.stack([(r * np.uint64(2654435761) ^ (r >> np.uint64(3)) * np.uint64(40503)) & np.uint64(0xFFFFFFFF),
                      (r // np.uint64(7) + r * r) & np.uint64(0xFFFFFFFF)], axis=1).astype(np.uint32)
    x = co.unpack(words, n)
    assert (np.abs(x.sum(axis=0)) < T).all()
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    spin, pair = _outputs(n)
    assert _raw(bits, n, spin, pair) == 0, _lib.lib().dvg_last_error()
    got_spin, got_pair = spin.cpu().numpy(), pair.cpu().numpy()
    assert got_spin[-1] == GUARD and got_pair[-1] == GUARD
    assert np.array_equal(got_spin[:-1], x.sum(axis=0)) and np.array_equal(got_pair[:-1].reshape(n, n), x.T @ x)


@pytest.mark.parametrize("n,repeats", [(512, 40), (2048, 300), (77, 9)])
def test_slabs_of_several_chunks(n, repeats):
    """A block of 1000 random rows repeated: the sums are ``repeats`` times the block's, which numpy multiplies exactly in
    float64.  n = 512, 40 000 rows: 36 tile pairs, 40 chunks in 14 slabs of 3 (the last of 1).  n = 2048, 300 000 rows: 528
    tile pairs, 293 chunks in 2 slabs, the first of the 256 chunks = 2^18 rows a slab may hold at the most.  n = 77, 9000
    rows: 3 tile pairs, 9 slabs of one chunk, the last of 808 rows."""
    W = (n + 31) // 32
    block = np.random.default_rng(n).integers(0, 2 ** 32, size=(1000, W), dtype=np.uint64).astype(np.uint32)
    x = co.unpack(block, n).astype(np.float64)
    want_spin = (repeats * x.sum(axis=0)).astype(np.int64)
    want_pair = (repeats * (x.T @ x)).astype(np.int64)  # (exact: integers far below 2^53)
    assert 1000 * repeats > (F.PACKED_CORRELATION_SLAB_ROWS if n == 2048 else 1024)
    bits = torch.from_numpy(np.tile(block, (repeats, 1)).view(np.int32)).cuda()
    spin, pair = _outputs(n)
    assert _raw(bits, n, spin, pair) == 0, _lib.lib().dvg_last_error()
    assert int(spin[-1]) == GUARD and int(pair[-1]) == GUARD
    assert torch.equal(spin[:-1].cpu(), torch.from_numpy(want_spin))
    assert torch.equal(pair[:-1].cpu().view(n, n), torch.from_numpy(want_pair))
    # the same rows as `repeats` groups of one block, the group stride 0: every group reads the same 1000 rows
    small = torch.from_numpy(block.view(np.int32)).cuda()
    spin2, pair2 = _outputs(n)
    assert _raw(small, n, spin2, pair2, groups=repeats, gs=0) == 0, _lib.lib().dvg_last_error()
    assert torch.equal(spin2, spin) and torch.equal(pair2, pair)


# ------------------------------------------------------------------------------------------------ identities with shipped kernels
@pytest.mark.parametrize("name,rows", [("pegasus64", 287), ("pegasus64", 64), ("zephyr1024", 130), ("zephyr1024", 910)])
def test_identities_with_the_moments_kernel_and_the_row_sums(name, rows):
    """On the same rows: ``pair_sum[edge_i, edge_j]`` and ``spin_sum`` are ``dvg_grbm_moments_packed``'s sums, and
    sum_ij pair_sum = sum_r (sum_i s_ri)^2 from the unpacked rows.  Exact."""
    plan = _solver_plan("pegasus", 64)[0] if name == "pegasus64" else _solver_plan("zephyr", 1024)[0]
    n, full = _case(name)
    a = full.reshape(-1, full.shape[-1])[:rows].contiguous()
    spin_sum, pair_sum = F.packed_correlation(a, n=n)
    m_spin, m_pair = F.grbm_moments_packed(a, smp.GraphHandle(plan, "cuda"))
    ei, ej = torch.from_numpy(np.asarray(plan.edge_i, dtype=np.int64)).cuda(), torch.from_numpy(np.asarray(plan.edge_j, dtype=np.int64)).cuda()
    assert torch.equal(spin_sum, m_spin) and torch.equal(pair_sum[ei, ej], m_pair) and torch.equal(pair_sum[ej, ei], m_pair)
    row_sums = smp.unpack_spins(a, n).to(torch.int64).sum(1)
    assert int(pair_sum.sum()) == int((row_sums ** 2).sum())


# ------------------------------------------------------------------------------------------------ guards
def test_rejected_calls_leave_the_outputs_and_the_workspace_intact():
    n, full = _case("pegasus64")
    a = full.reshape(-1, 2)[:65].contiguous()
    spin, pair = _outputs(n)
    need = int(_lib.lib().dvg_packed_correlation_workspace_bytes(65, 1, n))
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    before = spin.clone(), pair.clone(), ws.clone()
    for args, over, code in (((None, n, spin, pair), {}, -1), ((a, n, spin, None), {}, -1), ((a, n, spin, pair), dict(rows=0), -1),
                             ((a, n, spin, pair), dict(groups=0), -1), ((a, n, spin, pair), dict(n=0), -1),
                             ((a, n, spin, pair), dict(rs=1), -1), ((a, n, spin, pair), dict(gs=-1), -1),
                             ((a, n, spin, pair), dict(n=8193, rs=300), -4), ((a, n, spin, pair), dict(rows=2 ** 31, groups=2 ** 31), -4),
                             ((a, n, spin, pair), dict(ws_bytes=need - 1), -3), ((a, n, spin, pair), dict(ws_bytes=0), -3),
                             ((a, n, spin, pair), dict(rows=1025), -3)):
        for acc in (0, 1):
            assert _raw(*args, accumulate=acc, ws=ws, **over) == code, (over, _lib.lib().dvg_last_error())
    assert torch.equal(spin, before[0]) and torch.equal(pair, before[1]) and torch.equal(ws, before[2])
    assert _raw(a, n, spin, pair, ws=ws) == 0 and int(pair[0]) == 65 and not torch.equal(ws, before[2])


# ------------------------------------------------------------------------------------------------ the Python surface
def _sampler(plan, nodes, beta=2.0, sweeps=4):
    return smp.GibbsSampler(plan, nodes, beta=beta, sweeps=sweeps, seed=SEED, persistent=True, chain_offset=5, h_range=(-4, 4),
                            j_range=(-1, 1))


def _equals_helper(got, a, n, spin_sums=True):
    spin_sum, pair_sum = got
    want_spin, want_pair = co.sums(_dense(a), n)
    assert pair_sum.dtype == torch.int64 and pair_sum.shape == (n, n) and pair_sum.is_cuda and np.array_equal(pair_sum.cpu().numpy(), want_pair)
    if spin_sums:
        assert spin_sum.dtype == torch.int64 and spin_sum.shape == (n,) and np.array_equal(spin_sum.cpu().numpy(), want_spin)
    else:
        assert spin_sum is None
    return want_spin, want_pair


def test_functional_wrapper_slices_and_out():
    n, full = _case("random77")
    pool = full.reshape(-1, full.shape[-1])
    for a in (pool[:200], pool[:200:2], pool[5:6], full[:41], full[:41, 1:], full[50:, :6], full[:41:2, ::2], full[:1], full[:, 3]):
        at = a.data_ptr()
        _equals_helper(F.packed_correlation(a, n=n), a, n)
        _equals_helper(F.packed_correlation(a, n=n, spin_sums=False), a, n, spin_sums=False)
        assert a.data_ptr() == at
    assert not pool[:200:2].is_contiguous() and not full[:41, 1:].is_contiguous()
    # out= adds onto existing sums: pooling two calls is one call on all rows
    spin, pair = F.packed_correlation(pool[:100], n=n)
    again = F.packed_correlation(pool[100:150], n=n, out=(spin, pair))
    assert again[0] is spin and again[1] is pair
    _equals_helper((spin, pair), pool[:150], n)
    none, pair_only = F.packed_correlation(pool[:100], n=n, spin_sums=False)
    assert none is None
    again = F.packed_correlation(pool[100:150], n=n, spin_sums=False, out=(None, pair_only))
    assert again[0] is None and again[1] is pair_only and torch.equal(pair_only, pair)
    for bad, word in (((spin, pair[:-1]), "pair_sum"), ((spin.int(), pair), "spin_sum"), ((spin, pair.cpu()), "pair_sum"),
                      ((spin.cpu(), pair), "spin_sum")):
        with pytest.raises(_lib.DvgError, match=word):
            F.packed_correlation(pool[:10], n=n, out=bad)


def test_trace_correlations_and_model_correlations():
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    plan, nodes = _solver_plan("zephyr", 128)
    lin, quad = _fields(plan)
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                           np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    with torch.no_grad():
        grbm._linear.copy_(lin)
        grbm._quadratic.copy_(quad)
    kw = dict(prefactor=P["prefactor"], linear_range=(-4, 4), quadratic_range=(-1, 1), num_reads=9, num_sweeps=40, burn_in=4, thin=2)
    s1, s2 = _sampler(plan, nodes), _sampler(plan, nodes)
    trace = grbm.sample_trace(s1, **kw)
    assert trace.bits.shape == (9, 18, 4)
    c = trace.correlations()
    assert isinstance(c, smp.Correlations) and c.n == 128 and c.count == 9 * 18 and c.pair_sum.is_cuda
    want_spin, want_pair = _equals_helper((c.spin_sum, c.pair_sum), trace.bits, 128)
    want = co.estimates(want_spin, want_pair, 9 * 18)
    for name, value in want.items():
        got = getattr(c, name)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == np.shape(value), name
        assert np.allclose(got.cpu().numpy(), value, rtol=1e-12, atol=0, equal_nan=True), name
    gh = grbm.graph_handle("cuda")
    for graph in (gh, plan):
        assert np.allclose(c.on_edges(graph).cpu().numpy(), co.on_edges(want["connected"], plan.edge_i, plan.edge_j), rtol=1e-12, atol=0)
        assert np.isclose(float(c.off_edge_share(graph)), co.off_edge_share(want["connected"], plan.edge_i, plan.edge_j), rtol=1e-12, atol=0)
    assert c.on_edges(gh).shape == grbm._quadratic.shape and c.on_edges(gh).is_cuda
    i, j, v = c.top_pairs(7, gh)
    wi, wj, wv = co.top_pairs(want["connected"], 7, plan.edge_i, plan.edge_j)
    assert i.is_cuda and np.array_equal(i.cpu().numpy(), wi) and np.array_equal(j.cpu().numpy(), wj) and np.allclose(v.cpu().numpy(), wv, rtol=1e-12, atol=0)
    # the moments of the trace are the matrix's edges
    m = trace.moments(gh)
    assert torch.equal(m.spin_sum, c.spin_sum)
    assert torch.equal(m.pair_sum, c.pair_sum[torch.as_tensor(plan.edge_i, device="cuda"), torch.as_tensor(plan.edge_j, device="cuda")])
    # model_correlations is the correlations of the same traced draw; only trace_sweep_count moves
    got = grbm.model_correlations(s2, **kw)
    assert isinstance(got, smp.Correlations) and got.count == c.count
    assert torch.equal(got.pair_sum, c.pair_sum) and torch.equal(got.spin_sum, c.spin_sum)
    assert s2.trace_sweep_count == 40 and (s2.sweep_count, s2.calls, s2.ais_sweep_count, s2.pt_sweep_count) == (0, 0, 0, 0)
    assert s2._state is None
    # a hotter draw differs: gap against it, by the oracle
    other = grbm.sample_trace(_sampler(plan, nodes, beta=0.5), **dict(kw, num_reads=5)).correlations()
    os_, op = co.sums(_dense(grbm.sample_trace(_sampler(plan, nodes, beta=0.5), **dict(kw, num_reads=5)).bits), 128)
    want_gap = co.gap(want, co.estimates(os_, op, 5 * 18), plan.edge_i, plan.edge_j)
    got_gap = c.gap(other, gh)
    assert set(got_gap) == {"spin_rms", "pair_rms", "edge_rms", "off_edge_rms"}
    for name, value in want_gap.items():
        assert got_gap[name].is_cuda and np.isclose(float(got_gap[name]), value, rtol=1e-12, atol=0), name
    with pytest.raises(TypeError):
        grbm.model_correlations(object(), prefactor=0.05, num_reads=2)


def test_model_wrapper_prior_correlations_and_latent_correlation_gap():
    from image_generation_amd.data import synthetic_images
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    m.overlap_sampler = False  # (as in the moments file: this test takes no stream from the process's pool)
    draw = dict(num_reads=33, num_sweeps=20, burn_in=6, thin=2)
    prior = m.prior_correlations(**draw)
    s = m.sampler
    assert (s.trace_sweep_count, s.sweep_count, s.calls, s.ais_sweep_count) == (20, 0, 0, 0) and s._state is None
    assert isinstance(prior, smp.Correlations) and prior.n == 64 and prior.count == 7 * 33 and prior.pair_sum.is_cuda
    s.reset()  # the same draw again, by hand
    trace = m._grbm.sample_trace(s, prefactor=m.PREFACTOR, linear_range=m.linear_range, quadratic_range=m.quadratic_range, **draw)
    want_spin, want_pair = _equals_helper((prior.spin_sum, prior.pair_sum), trace.bits, 64)
    # the gap between the latents of a small batch and the prior
    B, k = 6, 5
    images = synthetic_images(B, seed=3, device="cuda").reshape(B, 1, 32, 32)
    s.reset()
    out = m.latent_correlation_gap(images, k=k, **draw)
    assert set(out) == {"data", "prior", "spin_rms", "pair_rms", "edge_rms", "off_edge_rms", "off_edge_share_data", "top_pairs"}
    with torch.no_grad():
        spins = F.heaviside_latent_to_discrete(m._dvae.encoder(images)).squeeze(1)
    data = out["data"]
    assert isinstance(data, smp.Correlations) and data.count == B and data.n == 64
    d_spin, d_pair = _equals_helper((data.spin_sum, data.pair_sum), smp.pack_spins(spins), 64)
    assert isinstance(out["prior"], smp.Correlations) and torch.equal(out["prior"].pair_sum, prior.pair_sum)
    plan = m._grbm.plan
    want_data, want_prior = co.estimates(d_spin, d_pair, B), co.estimates(want_spin, want_pair, 7 * 33)
    for name, value in co.gap(want_data, want_prior, plan.edge_i, plan.edge_j).items():
        got = out[name]
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == () and np.isclose(float(got), value, rtol=1e-12, atol=0), name
    share = out["off_edge_share_data"]
    assert share.dtype == torch.float64 and share.shape == ()
    assert np.isclose(float(share), co.off_edge_share(want_data["connected"], plan.edge_i, plan.edge_j), rtol=1e-12, atol=0, equal_nan=True)
    i, j, v = out["top_pairs"]
    assert i.dtype == j.dtype == torch.int64 and v.dtype == torch.float64 and i.shape == j.shape == v.shape == (k,)
    edges = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in zip(plan.edge_i, plan.edge_j)}
    assert all(a < b and (a, b) not in edges for a, b in zip(i.tolist(), j.tolist()))
    wi, wj, wv = co.top_pairs(want_data["connected"], k, plan.edge_i, plan.edge_j)
    assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(j.cpu().numpy(), wj) and np.allclose(v.cpu().numpy(), wv, rtol=1e-12, atol=0)
