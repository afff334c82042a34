"""GPU checks of ``dvg_packed_overlap`` ("DVG overlap v1") -- the histogram of Hamming distances between bit-packed rows and
every row's nearest partner -- against the numpy definition (``tests/overlap_oracle.py``): exact equality, the results are
integers.  Rows: traced draws (``dvg_gibbs_sample_traced``) on ``pegasus64`` (two whole words) and ``zephyr1024`` (32 words:
two staging chunks), and random words with noise in the bits of spins >= n for n = 77, 33 and 1.  Row counts below, at and
over one 64-row tile, several tiles with a partial last one; B split over workgroups (few rows of A) and not; flat sets and
the (C, M, W) layout of a trace at equal times; padded rows; duplicated and complemented rows for the ends of the histogram
and the tie rule.  A guard element behind each output; ``accumulate = 1`` adds onto nonzero contents; ``nearest = NULL``.
And the Python surface built on it."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_oracle as oo  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -0x0123456789ABCDEF
FILL = 0x7777777777
CONTENTS = ["pegasus64", "random77", "zephyr1024", "random33", "random1"]
SELF_ROWS = [1, 2, 63, 64, 65, 129, 287]
CROSS_ROWS = [(1, 1), (1, 287), (287, 1), (65, 130), (200, 3), (64, 64)]
TRACES = [(1, 5), (2, 1), (41, 7), (65, 3), (130, 2)]  # (chains C, records M)
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
    its (910, W) view, trace tests its first chains and records."""
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


def _flat(name, rows_a, rows_b=None):
    """Contiguous A = the first rows of the case's flat view, B = its last rows (both hold whole chains' records)."""
    n, full = _case(name)
    pool = full.reshape(-1, full.shape[-1])
    a = pool[:rows_a].contiguous()
    return n, a, (None if rows_b is None else pool[pool.shape[0] - rows_b:].contiguous())


def _outputs(n, elems, rng=None):
    """``hist`` and ``nearest`` with a guard element behind each; ``rng``: None (a fill to be overwritten) or a generator
    (nonzero int64 values in ``hist`` to add onto)."""
    h = np.full(n + 2, FILL, dtype=np.int64) if rng is None else rng.integers(-10 ** 12, 10 ** 12, size=n + 2)
    h[n + 1] = GUARD
    v = np.full(elems + 1, FILL, dtype=np.int64)
    v[elems] = GUARD
    return torch.from_numpy(h).cuda(), torch.from_numpy(v).cuda()


def _layout(t, W):
    """``(rows, row_stride, groups, group_stride)`` of a 2-D or 3-D tensor of packed rows, as the C entry takes them."""
    if t.dim() == 2:
        return int(t.shape[0]), int(t.stride(0)) if t.shape[0] > 1 else W, 1, 0
    return int(t.shape[0]), int(t.stride(0)) if t.shape[0] > 1 else W, int(t.shape[1]), int(t.stride(1)) if t.shape[1] > 1 else 0


def _raw(a, b, spins, hist, nearest, accumulate=0, **over):
    """The C entry on tensors, the layout taken from them; ``over`` replaces single arguments (``n`` among them)."""
    n = spins
    W = (n + 31) // 32
    ra, ars, groups, ags = _layout(a, W) if a is not None else (1, W, 1, 0)
    rb, brs, _g, bgs = _layout(b, W) if b is not None else (0, 0, 1, 0)
    kw = dict(rows_a=ra, a_rs=ars, a_gs=ags, rows_b=rb, b_rs=brs, b_gs=bgs, groups=groups, n=n)
    kw.update(over)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    rc = _lib.lib().dvg_packed_overlap(ptr(a), kw["rows_a"], kw["a_rs"], kw["a_gs"], ptr(b), kw["rows_b"], kw["b_rs"], kw["b_gs"],
                                       kw["groups"], kw["n"], ptr(hist), ptr(nearest), accumulate, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _dense(t):
    return t.contiguous().cpu().numpy()


def _check_exact(a, b, n, seed=0):
    """The C entry on (views of) device tensors ``a`` / ``b`` against the helper on their dense copies: both outputs with
    guards, then ``accumulate = 1`` onto random contents with ``nearest = NULL``.  Returns the expected pair."""
    want_hist, want_near = oo.overlap(_dense(a), None if b is None else _dense(b), n)
    groups, rows_a = want_near.shape
    pairs = groups * (rows_a * (rows_a - 1) // 2 if b is None else rows_a * int(b.shape[0]))
    assert want_hist.sum() == pairs
    hist, near = _outputs(n, groups * rows_a)
    assert _raw(a, b, n, hist, near) == 0, _lib.lib().dvg_last_error()
    got_hist, got_near = hist.cpu().numpy(), near.cpu().numpy()
    assert got_hist[-1] == GUARD and got_near[-1] == GUARD, "written past an output"
    assert np.array_equal(got_hist[:-1], want_hist)
    assert np.array_equal(got_near[:-1].reshape(groups, rows_a), want_near)
    hist, near = _outputs(n, groups * rows_a, rng=np.random.default_rng(seed + rows_a))
    base = hist.cpu().numpy().copy()
    assert _raw(a, b, n, hist, None, accumulate=1) == 0, _lib.lib().dvg_last_error()
    got_hist = hist.cpu().numpy()
    assert got_hist[-1] == GUARD and np.array_equal(got_hist[:-1], base[:-1] + want_hist)
    assert torch.equal(near, _outputs(n, groups * rows_a)[1])  # (untouched: NULL was passed)
    return want_hist, want_near


# ------------------------------------------------------------------------------------------------ flat sets
@pytest.mark.parametrize("rows", SELF_ROWS)
@pytest.mark.parametrize("name", CONTENTS)
def test_flat_self_mode_is_exact(name, rows):
    n, a, _b = _flat(name, rows)
    _hist, near = _check_exact(a, None, n)
    assert (near == -1).all() == (rows == 1)


@pytest.mark.parametrize("rows_a,rows_b", CROSS_ROWS)
@pytest.mark.parametrize("name", CONTENTS)
def test_flat_cross_mode_is_exact(name, rows_a, rows_b):
    n, a, b = _flat(name, rows_a, rows_b)
    _check_exact(a, b, n)


def test_the_traced_rows_are_the_draws_records():
    """The traced cases hold spins that move, and rows that differ: the histogram is not one bin."""
    for name in ("pegasus64", "zephyr1024"):
        n, bits = _case(name)
        moved = (bits != bits[:, :1]).any(-1)
        assert moved.any()
        hist, _near = oo.overlap(_dense(bits.reshape(-1, bits.shape[-1])[:64]), None, n)
        assert (hist > 0).sum() >= 4


# ------------------------------------------------------------------------------------------------ traces at equal times
@pytest.mark.parametrize("C,M", TRACES)
@pytest.mark.parametrize("name", ["pegasus64", "random77"])
def test_trace_layout_at_equal_times(name, C, M):
    n, full = _case(name)
    a = full[:C, :M]  # (a view: row stride 7 W, group stride W)
    hist, near = _check_exact(a, None, n)
    if C == 1:
        assert hist.sum() == 0 and (near == -1).all() and near.shape == (M, 1)
    other = full[130 - 37:, 7 - M:]  # a second trace: 37 chains, the last M records
    _check_exact(a, other, n)
    shared = full.reshape(-1, full.shape[-1])[300:300 + 67]  # one flat B for every group: b_group_stride = 0
    want_hist, _near = _check_exact(a, shared, n)
    assert want_hist.sum() == M * C * 67


def test_padded_rows():
    """``row_stride = W + 3`` with the padding words set at random, flat and as groups."""
    for name, rows_a, rows_b in (("random77", 129, 70), ("pegasus64", 65, 200), ("random1", 70, 3)):
        n, a, b = _flat(name, rows_a, rows_b)
        W = a.shape[1]
        rng = np.random.default_rng(rows_a)
        pa = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(rows_a, W + 3)).astype(np.int32)).cuda()
        pb = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(rows_b, W + 3)).astype(np.int32)).cuda()
        pa[:, :W], pb[:, :W] = a, b
        assert pa[:, :W].stride(0) == W + 3
        _check_exact(pa[:, :W], None, n)
        _check_exact(pa[:, :W], pb[:, :W], n)
    n, full = _case("random77")
    W = full.shape[-1]
    padded = torch.from_numpy(np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, size=(41, 5, W + 3)).astype(np.int32)).cuda()
    padded[:, :, :W] = full[:41, :5]
    _check_exact(padded[:, :, :W], None, n)


# ------------------------------------------------------------------------------------------------ ends of the histogram, ties
def _with_twins(name, rows):
    """Rows of the case with row 3 repeated at 70 and 200, and row 5's complement (noise bits too) at 6."""
    n, a, _b = _flat(name, rows)
    a = a.clone()
    a[70], a[200], a[6] = a[3], a[3], ~a[5]
    return n, a


@pytest.mark.parametrize("name", ["random77", "pegasus64", "zephyr1024"])
def test_ends_of_the_histogram_and_the_tie_rule(name):
    n, a = _with_twins(name, 287)
    host = _dense(a)
    twins = np.flatnonzero((host == host[3]).all(1))  # 3, 70, 200 (and any row of the draw that happens to equal them)
    assert {3, 70, 200} <= set(twins.tolist())
    hist, near = _check_exact(a, None, n)  # (five tiles: B is split over workgroups, the minima are combined by atomics)
    dist, row = oo.split(near)
    assert hist[0] >= 3 and hist[n] >= 1  # three pairs of twins; a row and its complement
    assert (dist[0, twins] == 0).all() and row[0, twins[0]] == twins[1] and (row[0, twins[1:]] == twins[0]).all()  # the smallest index
    # cross mode, the twins in B
    hist, near = _check_exact(a[:200].contiguous(), a, n)
    dist, row = oo.split(near)
    assert hist[0] >= 200 and (dist[0, [3, 70]] == 0).all() and (row[0, [3, 70]] == twins[0]).all() and hist[n] >= 2
    # two rows of A against 287 of B
    probe = torch.stack([a[70], ~a[3]])
    hist, near = _check_exact(probe, a, n)
    dist, row = oo.split(near)
    assert dist[0, 0] == 0 and row[0, 0] == twins[0] and hist[0] == len(twins) and hist[n] == len(twins)
    # 64 rows of B: one workgroup sees all of B and stores the minimum itself
    b = a[137:201].contiguous()  # (row 200 of a is row 63 here)
    hist, near = _check_exact(a[:130].contiguous(), b, n)
    assert oo.split(near)[0][0, 3] == 0 and oo.split(near)[1][0, 3] <= 63


def test_many_groups_take_all_of_b_in_one_unit():
    """1100 records of 65 chains: 2200 (group, A tile) units, more than the grid's workgroups, each walking both tiles of B
    and storing its rows' minima itself -- no atomics on ``nearest``."""
    n = 77
    noise = np.random.default_rng(1100).integers(0, 2 ** 32, size=(65, 1100, 3), dtype=np.uint64).astype(np.uint32)
    a = torch.from_numpy(noise.view(np.int32)).cuda()
    _check_exact(a, None, n)
    _check_exact(a[:3], a[:, 5], n)  # few rows in many groups against one shared B of 65 rows


# ------------------------------------------------------------------------------------------------ guards
def test_rejected_calls_leave_the_outputs_intact():
    n, a, b = _flat("pegasus64", 65, 130)
    hist, near = _outputs(n, 65)
    before = hist.clone(), near.clone()
    for mode_b in (b, None):
        for args, over, code in (((None, mode_b, n, hist, near), {}, -1), ((a, mode_b, n, None, near), {}, -1),
                                 ((a, mode_b, n, hist, near), dict(rows_a=0), -1), ((a, mode_b, n, hist, near), dict(groups=0), -1),
                                 ((a, mode_b, n, hist, near), dict(n=0), -1), ((a, mode_b, n, hist, near), dict(a_rs=1), -1),
                                 ((a, mode_b, n, hist, near), dict(a_gs=-1), -1), ((a, mode_b, n, hist, near), dict(n=8193, a_rs=300, b_rs=300), -4),
                                 ((a, mode_b, n, hist, near), dict(rows_a=2 ** 31), -4)):
            assert _raw(*args, **over) == code, (over, _lib.lib().dvg_last_error())
    for over, code in ((dict(rows_b=0), -1), (dict(b_rs=1), -1), (dict(b_gs=-1), -1), (dict(rows_b=2 ** 31), -4),
                       (dict(rows_a=2 ** 30, rows_b=2 ** 30, groups=4), -4)):
        assert _raw(a, b, n, hist, near, **over) == code, (over, _lib.lib().dvg_last_error())
    assert torch.equal(hist, before[0]) and torch.equal(near, before[1])


def test_a_workgroup_flushes_before_a_counter_can_wrap():
    """n = 1, 531 264 x 531 200 rows: 8301 units of 8300 tile pairs over the 1024 workgroups of the grid, eight or nine units
    each -- more than the 65 536 tiles (2^28 pairs) after which a workgroup flushes its 32-bit LDS counters in the middle of
    its work.  The expected histogram is a product of counts: pairs of equal bits, pairs of different bits."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 2 ** 32, size=(531264, 1), dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 2 ** 32, size=(531200, 1), dtype=np.uint64).astype(np.uint32)
    ua, ub = int((a & 1).sum()), int((b & 1).sum())
    want = np.array([ua * ub + (len(a) - ua) * (len(b) - ub), ua * (len(b) - ub) + (len(a) - ua) * ub], dtype=np.int64)
    assert want.sum() == len(a) * len(b) > 2 ** 38 and (len(a) // 64 // 1024) * (len(b) // 64) > 65536
    hist, _near = _outputs(1, 1)
    assert _raw(torch.from_numpy(a.view(np.int32)).cuda(), torch.from_numpy(b.view(np.int32)).cuda(), 1, hist, None) == 0
    got = hist.cpu().numpy()
    assert got[-1] == GUARD and np.array_equal(got[:-1], want)


# ------------------------------------------------------------------------------------------------ two kernels, one identity
@pytest.mark.parametrize("name,rows", [("pegasus64", 287), ("pegasus64", 64), ("zephyr1024", 130)])
def test_identity_with_the_moments_kernel(name, rows):
    """sum_{r < r'} s_r . s_r' = ((sum_r s_r)^2 - R n) / 2 spin by spin: the left side from this kernel's histogram, the
    right side from ``dvg_grbm_moments_packed``'s spin sums over the same rows.  Exact."""
    plan = _solver_plan("pegasus", 64)[0] if name == "pegasus64" else _solver_plan("zephyr", 1024)[0]
    n, a, _b = _flat(name, rows)
    hist, _none = F.packed_overlap(a, n=n)
    spin_sum, _pair_sum = F.grbm_moments_packed(a, smp.GraphHandle(plan, "cuda"))
    left = int(((n - 2 * np.arange(n + 1, dtype=np.int64)) * hist.cpu().numpy()).sum())
    right = int((spin_sum.cpu().numpy() ** 2).sum()) - rows * n
    assert right % 2 == 0 and left == right // 2


# ------------------------------------------------------------------------------------------------ the Python surface
def _sampler(plan, nodes, beta=2.0, sweeps=4):
    return smp.GibbsSampler(plan, nodes, beta=beta, sweeps=sweeps, seed=SEED, persistent=True, chain_offset=5, h_range=(-4, 4),
                            j_range=(-1, 1))


def _equals_helper(got, a, b, n):
    """``functional.packed_overlap``'s result against the helper on dense copies."""
    hist, near = got
    want_hist, want_near = oo.overlap(_dense(a), None if b is None else _dense(b), n)
    assert hist.dtype == torch.int64 and hist.shape == (n + 1,) and np.array_equal(hist.cpu().numpy(), want_hist)
    if near is not None:
        dist, row = near
        shape = want_near.shape if a.dim() == 3 else want_near.shape[1:]
        assert dist.dtype == torch.int32 and row.dtype == torch.int32 and tuple(dist.shape) == tuple(row.shape) == shape
        wd, wr = oo.split(want_near)
        assert np.array_equal(dist.cpu().numpy(), wd.reshape(shape)) and np.array_equal(row.cpu().numpy(), wr.reshape(shape))


def test_functional_wrapper_and_slices():
    n, full = _case("random77")
    pool = full.reshape(-1, full.shape[-1])
    for a, b in ((pool[:200], None), (pool[:200:2], None), (pool[:65], pool[1:400:3]), (full[:41], None), (full[:41, 1:], None),
                 (full[:41, 1:], full[50:, :6]), (full[:41:2, ::2], pool[7:77]), (pool[:1], None), (full[:1], None)):
        at = a.data_ptr()
        _equals_helper(F.packed_overlap(a, b, n=n, nearest=True), a, b, n)
        _equals_helper(F.packed_overlap(a, b, n=n), a, b, n)
        assert a.data_ptr() == at
    assert not pool[:200:2].is_contiguous() and not full[:41, 1:].is_contiguous()
    # out= adds onto an existing histogram
    hist, none = F.packed_overlap(pool[:100], n=n)
    assert none is None
    again, _none = F.packed_overlap(pool[:100], pool[100:150], n=n, out=hist)
    assert again is hist
    want = oo.overlap(_dense(pool[:100]), None, n)[0] + oo.overlap(_dense(pool[:100]), _dense(pool[100:150]), n)[0]
    assert np.array_equal(hist.cpu().numpy(), want)
    for bad in (hist[:-1], hist.int(), hist.cpu()):
        with pytest.raises(_lib.DvgError, match="hist"):
            F.packed_overlap(pool[:10], n=n, out=bad)
    with pytest.raises(_lib.DvgError, match="device"):
        F.packed_overlap(pool[:10], pool[:10].cpu(), n=n)
    # no partner: -1 in both halves
    _h, (dist, row) = F.packed_overlap(full[:1, :3], n=n, nearest=True)
    assert dist.shape == (3, 1) and (dist == -1).all() and (row == -1).all()


def test_trace_overlap_replica_overlap_and_the_estimates():
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
    o = trace.overlap()
    assert isinstance(o, smp.Overlap) and o.n == 128 and o.hist.is_cuda
    want_hist, want_near = oo.overlap(_dense(trace.bits), None, 128)
    assert np.array_equal(o.hist.cpu().numpy(), want_hist) and float(o.pairs) == 18 * 36
    for name, value in oo.estimates(want_hist, 128).items():
        got = getattr(o, name)
        assert got.is_cuda and got.dtype == torch.float64 and np.isclose(float(got), value, rtol=1e-12, atol=0), name
    assert np.isclose(float(o.mass(0.25, 1.0)), oo.mass(want_hist, 128, 0.25, 1.0), rtol=1e-12, atol=0)
    o2, (dist, row) = trace.overlap(nearest=True)
    assert torch.equal(o2.hist, o.hist) and dist.shape == (18, 9)
    wd, wr = oo.split(want_near)
    assert np.array_equal(dist.cpu().numpy(), wd) and np.array_equal(row.cpu().numpy(), wr)
    # against another trace, its bits, and a flat set: the same call three ways
    other = grbm.sample_trace(_sampler(plan, nodes, beta=0.5), **dict(kw, num_reads=5))
    cross = trace.overlap(other)
    assert np.array_equal(cross.hist.cpu().numpy(), oo.overlap(_dense(trace.bits), _dense(other.bits), 128)[0])
    assert torch.equal(trace.overlap(other.bits).hist, cross.hist)
    flat = other.bits[:, 0]
    assert np.array_equal(trace.overlap(flat).hist.cpu().numpy(), oo.overlap(_dense(trace.bits), _dense(flat), 128)[0])
    # replica_overlap is the overlap of the same traced draw; only trace_sweep_count moves
    got = grbm.replica_overlap(s2, **kw)
    assert isinstance(got, smp.Overlap) and torch.equal(got.hist, o.hist)
    assert s2.trace_sweep_count == 40 and (s2.sweep_count, s2.calls, s2.ais_sweep_count, s2.pt_sweep_count) == (0, 0, 0, 0)
    assert s2._state is None
    with pytest.raises(TypeError):
        grbm.replica_overlap(object(), prefactor=0.05, num_reads=2)


def test_model_wrapper_prior_overlap_and_latent_novelty():
    from image_generation_amd.data import synthetic_images
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    m.overlap_sampler = False  # (as in the moments file: this test takes no stream from the process's pool)
    o = m.prior_overlap(num_reads=33, num_sweeps=20, burn_in=6, thin=2)
    s = m.sampler
    assert (s.trace_sweep_count, s.sweep_count, s.calls, s.ais_sweep_count) == (20, 0, 0, 0) and s._state is None
    assert isinstance(o, smp.Overlap) and o.n == 64 and o.hist.is_cuda and float(o.pairs) == 7 * 33 * 16
    s.reset()  # the same draw again, by hand
    trace = m._grbm.sample_trace(s, prefactor=m.PREFACTOR, linear_range=m.linear_range, quadratic_range=m.quadratic_range,
                                 num_reads=33, num_sweeps=20, burn_in=6, thin=2)
    assert torch.equal(trace.overlap().hist, o.hist)
    assert np.array_equal(o.hist.cpu().numpy(), oo.overlap(_dense(trace.bits), None, 64)[0])
    # novelty: given samples against the latents of a small batch
    B = 6
    images = synthetic_images(B, seed=3, device="cuda").reshape(B, 1, 32, 32)
    with torch.no_grad():
        spins = F.heaviside_latent_to_discrete(m._dvae.encoder(images)).squeeze(1)
    samples = trace.unpack()[:, -1]  # (33, 64) +-1
    samples[4] = spins[2]  # a copy of a data latent
    out = m.latent_novelty(images, samples)
    assert set(out) == {"nearest_dist", "nearest_row", "overlap", "data_nearest_dist"}
    data, drawn = _dense(smp.pack_spins(spins)), _dense(smp.pack_spins(samples))
    want_hist, want_near = oo.overlap(drawn, data, 64)
    wd, wr = oo.split(want_near)
    assert np.array_equal(out["nearest_dist"].cpu().numpy(), wd[0]) and np.array_equal(out["nearest_row"].cpu().numpy(), wr[0])
    assert int(out["nearest_dist"][4]) == 0 and (spins[int(out["nearest_row"][4])] == spins[2]).all()
    assert isinstance(out["overlap"], smp.Overlap) and np.array_equal(out["overlap"].hist.cpu().numpy(), want_hist)
    assert np.array_equal(out["data_nearest_dist"].cpu().numpy(), oo.split(oo.overlap(data, None, 64)[1])[0][0])
    assert out["data_nearest_dist"].shape == (B,) and out["nearest_dist"].dtype == torch.int32
    # samples=None draws one sample set as generate_images does
    drew = m.latent_novelty(images)
    assert drew["nearest_dist"].shape == drew["nearest_row"].shape == (int(m.sampler_kwargs.get("num_reads", 1)),)
    assert float(drew["overlap"].pairs) == B * drew["nearest_dist"].shape[0]
    assert torch.equal(drew["data_nearest_dist"], out["data_nearest_dist"])
