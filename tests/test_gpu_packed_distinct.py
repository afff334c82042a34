"""GPU checks of ``dvg_packed_distinct`` ("DVG distinct v1") -- the equivalence classes of bit-packed rows under equality on
the spins < n -- against the numpy definition (``tests/distinct_oracle.py``): every comparison is exact, the results are
integers.  Rows of n = 1 .. 1056 spins with random garbage in the pad bits; T = 1, 63, 64, 65, 1000 rows and the sizes at
which the compaction scan takes another level; all rows equal, all distinct, skewed pools, rows that differ in one bit (the
first, the last valid one, a pad bit); pooled (C, M, W) traces, padded rows, group slices; a second set that is looked up;
every optional output absent; sentinels behind the D classes; the hash cut down to 0 and 3 bits; permutations.  And the
Python surface built on it."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distinct_oracle as do  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 775321899904
WIDTHS = [1, 31, 32, 33, 77, 256, 1000, 1024, 1056]
COUNTS = [1, 63, 64, 65, 1000]
CONTENTS = ["equal", "distinct", "pool7", "pool300", "bit0", "lastbit", "padbit", "ends"]
HASH_BITS = [-1, 0, 3]
S32, S64 = -0x01234567, -0x0123456789ABCDEF  # sentinels: no output ever holds them


# ------------------------------------------------------------------------------------------------ rows
def _garbage(rows, n, rng):
    """Random bits into the pad bits (the bits of spins >= n) of every row, in place."""
    if n % 32:
        noise = rng.integers(0, 2 ** 32, size=rows.shape[0], dtype=np.uint64).astype(np.uint32)
        rows[:, -1] = (rows[:, -1] & np.uint32((1 << (n % 32)) - 1)) | (noise & ~np.uint32((1 << (n % 32)) - 1))
    return rows


def _random_rows(count, n, rng):
    return rng.integers(0, 2 ** 32, size=(count, (n + 31) // 32), dtype=np.uint64).astype(np.uint32)


def _content(kind, T, n, seed=0):
    """(T, W) uint32 rows of one kind, the pad bits of every row random."""
    rng = np.random.default_rng([seed, T, n, CONTENTS.index(kind)])
    W = (n + 31) // 32
    if kind == "equal":
        rows = np.repeat(_random_rows(1, n, rng), T, axis=0)
    elif kind == "distinct":  # the low bits hold t: distinct wherever n spins can tell T rows apart
        rows = _random_rows(T, n, rng)
        k = min(n, 20, 32)
        rows[:, 0] = (rows[:, 0] & ~np.uint32((1 << k) - 1)) | (np.arange(T, dtype=np.uint32) & np.uint32((1 << k) - 1))
    elif kind in ("pool7", "pool300"):  # skewed multiplicities: state floor(P u^3)
        P = int(kind[4:])
        rows = _random_rows(P, n, rng)[(P * rng.random(T) ** 3).astype(np.int64)]
    elif kind in ("bit0", "lastbit", "padbit"):
        rows = np.repeat(_random_rows(1, n, rng), T, axis=0)
        w, b = {"bit0": (0, 0), "lastbit": ((n - 1) // 32, (n - 1) % 32), "padbit": (W - 1, 31)}[kind]
        flip = rng.integers(0, 2, size=T).astype(np.uint32) << np.uint32(b)
        rows[:, w] ^= flip
        if kind == "padbit" and n % 32:
            return rows  # (no other garbage: the pad bit is the only difference, and the rows are equal)
        if kind == "padbit":
            rows[:, w] ^= flip  # no pad bit at this width: equal rows
    else:  # "ends": a class that first occurs at t = 0 and recurs, a class that first occurs at t = T - 1
        rows = _random_rows(5, n, rng)[rng.integers(0, 5, size=T)]
        rows[T - 1] = rows[0]
        if T > 1:
            rows[T - 1] = ~rows[T // 2]
    return _garbage(rows, n, rng)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _layout(t, W):
    """``(rows, row_stride, groups, group_stride)`` of a 2-D or 3-D tensor of packed rows, as the C entry takes them."""
    if t.dim() == 2:
        return int(t.shape[0]), int(t.stride(0)) if t.shape[0] > 1 else W, 1, 0
    return int(t.shape[1]), int(t.stride(1)) if t.shape[1] > 1 else W, int(t.shape[0]), int(t.stride(0)) if t.shape[0] > 1 else 0


OUTPUTS = ("first", "id", "rep", "count", "other_id", "other_hits")


def _raw(bits, n, other=None, absent=()):
    """The C entry on (views of) device tensors, the layout taken from them; every output but those named in ``absent`` is
    given, filled with sentinels.  Returns ``(D, dict of host arrays)``."""
    W = (n + 31) // 32
    rows, rs, groups, gs = _layout(bits, W)
    T = rows * groups
    ro, ors = (int(other.shape[0]), int(other.stride(0)) if other.shape[0] > 1 else W) if other is not None else (0, 0)
    out = {}
    for name in OUTPUTS:
        if name in absent or (other is None and name.startswith("other")):
            continue
        wide = name in ("count", "other_hits")
        size = ro if name == "other_id" else T
        out[name] = torch.full((size + 1,), S64 if wide else S32, dtype=torch.int64 if wide else torch.int32, device="cuda")
    nd = torch.full((2,), S64, dtype=torch.int64, device="cuda")
    L = _lib.lib()
    nbytes = L.dvg_packed_distinct_workspace_bytes(rows, groups, n)
    assert nbytes > 0
    ws = torch.empty((nbytes + 16,), dtype=torch.uint8, device="cuda")
    ws[nbytes:] = 0xA5
    p = lambda name: out[name].data_ptr() if name in out else None  # noqa: E731
    rc = L.dvg_packed_distinct(bits.data_ptr(), rows, rs, groups, gs, n, other.data_ptr() if other is not None else None, ro, ors,
                               p("first"), p("id"), p("rep"), p("count"), nd.data_ptr(), p("other_id"), p("other_hits"), ws.data_ptr(),
                               nbytes, _lib.stream_ptr())
    assert rc == 0, L.dvg_last_error()
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xA5).all(), "the workspace was written beyond the query"
    nd = nd.cpu().numpy()
    assert nd[1] == S64
    return int(nd[0]), {k: v.cpu().numpy() for k, v in out.items()}


def _check(bits, n, other=None, absent=(), want=None):
    """The entry against the oracle on dense copies: every given output, and sentinels behind the D classes and each array."""
    if want is None:
        want = do.distinct(bits.contiguous().cpu().numpy(), n, None if other is None else other.contiguous().cpu().numpy())
    D, got = _raw(bits, n, other, absent)
    T = want.first.size
    assert D == want.rep.size and int(want.count.sum()) == T
    for name in OUTPUTS:
        if name not in got:
            continue
        w = getattr(want, name)
        sentinel = S64 if name in ("count", "other_hits") else S32
        assert got[name].dtype == w.dtype and np.array_equal(got[name][:w.size], w), (name, got[name][:8], w[:8])
        assert (got[name][w.size:] == sentinel).all(), f"{name} was written beyond its {w.size} elements"
    return want, got


# ------------------------------------------------------------------------------------------------ widths x counts x contents x hash
@pytest.mark.parametrize("n", WIDTHS)
def test_every_content_at_every_count_under_every_hash(n):
    """Exact equality with the oracle, and the same bits with the full hash, with no hash (every row starts at slot 0: one
    probe chain through the whole table) and with 3 bits of it (8 chains that run into each other)."""
    for T in COUNTS:
        for kind in CONTENTS:
            bits = _dev(_content(kind, T, n))
            want = do.distinct(bits.cpu().numpy(), n)
            if kind in ("equal", "padbit"):
                assert want.rep.size == 1 and want.count[0] == T
            if kind == "distinct" and (n >= 20 or 2 ** n >= T):
                assert want.rep.size == T
            if kind in ("bit0", "lastbit") and T >= 63:
                assert want.rep.size == 2
            if kind == "ends" and n >= 8 and T > 1:
                assert want.first[T - 1] == T - 1 and want.count[0] > 1
            first = None
            for k in HASH_BITS:
                with _lib.option_scope(distinct_hash_bits=k):
                    _w, got = _check(bits, n, want=want)
                if first is None:
                    first = got
                for name in first:
                    assert np.array_equal(first[name], got[name]), (name, k)


def test_the_longest_probe_chain():
    """2000 distinct rows with every row starting at slot 0, then on 8 start slots."""
    n, T = 77, 2000
    bits = _dev(_content("distinct", T, n))
    want = do.distinct(bits.cpu().numpy(), n)
    assert want.rep.size == T
    other = bits[torch.arange(T - 1, -1, -7, device="cuda")].contiguous()
    want = do.distinct(bits.cpu().numpy(), n, other.cpu().numpy())
    for k in (0, 3, -1):
        with _lib.option_scope(distinct_hash_bits=k):
            _check(bits, n, other, want=want)


@pytest.mark.parametrize("T", [1024, 1025, 2 ** 20 + 1])
def test_every_level_of_the_compaction_scan(T):
    """The scan takes 1024 elements a workgroup: one workgroup up to T = 1024, block sums and one scan of them from 1025,
    sums of the sums from 2^20 + 1.  n = 32: a word a row; ~0.3 T classes whose first rows lie in every block."""
    rng = np.random.default_rng(T)
    rows = rng.integers(0, 2 ** 32, size=(max(1, T // 3), 1), dtype=np.uint64).astype(np.uint32)[rng.integers(0, max(1, T // 3), size=T)]
    want, _got = _check(_dev(rows), 32)
    assert 1 < want.rep.size < T and want.rep[-1] > T - 1025


# ------------------------------------------------------------------------------------------------ views
@pytest.mark.parametrize("n", [33, 256, 1000])
def test_views_need_no_copy(n):
    rng = np.random.default_rng(n)
    W = (n + 31) // 32
    C, M = 5, 37
    pool = _random_rows(40, n, rng)
    trace = _dev(_garbage(pool[rng.integers(0, 40, size=C * M)], n, rng)).view(C, M, W)
    want, _got = _check(trace, n)  # pooled through groups and strides
    assert np.array_equal(want.first, do.distinct(trace.reshape(-1, W).cpu().numpy(), n).first)
    # a group slice: chains 1..3, records 2.. -- the base moves, both strides stay
    view = trace[1:4, 2:]
    assert view.data_ptr() != trace.data_ptr() and not view.is_contiguous()
    _check(view, n)
    _check(trace[:, ::3], n)  # every third record: row_stride = 3 W
    _check(trace[2], n)
    # row_stride > W with garbage between the rows: 3 words (rows off 16-byte alignment) and 4 words
    for pad in (3, 4):
        wide = _dev(rng.integers(0, 2 ** 32, size=(C * M, W + pad), dtype=np.uint64).astype(np.uint32))
        wide[:, :W] = trace.reshape(-1, W)
        view = wide[:, :W]
        assert view.stride(0) == W + pad
        w2, _g = _check(view, n, other=trace[0])
        assert np.array_equal(w2.first, want.first)
        if pad == 4:  # a base off 16-byte alignment under an aligned stride
            _check(wide[:, 1:W + 1], 32 * W)


def test_pack_spins_of_real_draws():
    plan, nodes = _ring16()
    s = _sampler(plan, nodes, beta=1.5, sweeps=6)
    lin = torch.zeros(16, device="cuda")
    quad = torch.full((plan.n_edges,), -1.0, device="cuda")
    x = s.sample_native(lin, quad, 1.0, None, None, 500)
    bits = smp.pack_spins(x)
    assert bits.shape == (500, 1) and bits.dtype == torch.int32
    want, _got = _check(bits, 16)
    assert 1 < want.rep.size < 500  # cold ferromagnetic ring: few states, many copies
    keys = {tuple(r) for r in (x > 0).cpu().numpy().tolist()}
    assert len(keys) == want.rep.size


# ------------------------------------------------------------------------------------------------ other
@pytest.mark.parametrize("n", [1, 33, 256, 1024])
def test_other_rows_are_looked_up_never_inserted(n):
    rng = np.random.default_rng(n + 1)
    T = 300
    rows = _content("pool300", T, n, seed=1)
    absent = _random_rows(20, n, rng)
    picked = rows[rng.integers(0, T, size=40)]
    other = _garbage(np.concatenate([picked, absent, picked[:10], absent[:3]]), n, rng)
    bits, od = _dev(rows), _dev(other)
    alone, _g = _check(bits, n)
    want, got = _check(bits, n, od)
    for name in ("first", "id", "rep", "count"):
        assert np.array_equal(getattr(alone, name), getattr(want, name))
    found = int((want.other_id >= 0).sum())
    assert found >= 50 and int(got["other_hits"][:want.rep.size].sum()) == found
    if n > 32:
        assert found == 50 and (want.other_id[40:60] == -1).all()
    # one row, present and absent; a strided other
    for u in (0, 45):
        w1, _g = _check(bits, n, od[u:u + 1])
        assert w1.other_id[0] == want.other_id[u]
    _check(bits, n, od[::2])
    # other against a pooled trace
    _check(bits[:294].view(6, 49, -1), n, od)


def test_each_optional_output_alone_absent():
    n, T = 77, 130
    bits = _dev(_content("pool7", T, n))
    other = _dev(_content("pool7", 9, n))
    want = do.distinct(bits.cpu().numpy(), n, other.cpu().numpy())
    for name in OUTPUTS:
        _check(bits, n, other, absent=(name,), want=want)
    _check(bits, n, other, absent=OUTPUTS, want=want)  # n_distinct alone
    _check(bits, n, None, absent=("first", "id", "rep", "count"), want=want)
    _check(bits, n, other, absent=("first", "id", "rep", "count", "other_hits"), want=want)
    _check(bits, n, other, absent=("first", "id", "rep", "count", "other_id"), want=want)


# ------------------------------------------------------------------------------------------------ determinism
def test_two_calls_agree_and_permutations_permute():
    n, T = 256, 1000
    rows = _content("pool300", T, n)
    bits = _dev(rows)
    want, a = _check(bits, n)
    _w, b = _check(bits, n)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    perm = np.random.default_rng(3).permutation(T)
    wp, got = _check(_dev(rows[perm]), n)  # id and first of the permuted input equal the oracle on the permuted input
    assert sorted(got["count"][:wp.rep.size].tolist()) == sorted(want.count.tolist())
    assert not np.array_equal(wp.first, want.first)


# ------------------------------------------------------------------------------------------------ Python
def _same(d, want, bits_host, n, lead):
    assert isinstance(d, smp.Distinct) and d.n == n and d.count == want.first.size and d.distinct == want.rep.size
    assert d.rows.is_cuda and d.counts.dtype == torch.int64 and d.index.dtype == torch.int32
    assert np.array_equal(d.counts.cpu().numpy(), want.count) and tuple(d.index.shape) == tuple(lead) == tuple(d.first.shape)
    assert np.array_equal(d.index.cpu().numpy().reshape(-1), want.id) and np.array_equal(d.first.cpu().numpy().reshape(-1), want.first)
    assert np.array_equal(d.rows.cpu().numpy().view(np.uint32), do.keys(bits_host, n)[want.rep])
    est = do.estimates(want.count)
    for name, value in est.items():
        got = float(getattr(d, name))
        assert got == value or abs(got - value) <= 1e-12 * abs(value), (name, got, value)


def test_functional_and_distinct_equal_the_oracle():
    n = 77
    rows = _content("pool300", 1000, n)
    other = _garbage(np.concatenate([rows[5:30], _random_rows(7, n, np.random.default_rng(0))]), n, np.random.default_rng(1))
    bits, od = _dev(rows), _dev(other)
    want = do.distinct(rows, n, other)
    r = F.packed_distinct(bits, od, n=n)
    D = want.rep.size
    assert r.rep.shape == (D,) and r.count.shape == (D,) and r.other_hits.shape == (D,) and r.first.shape == (1000,)
    for name in OUTPUTS:
        assert np.array_equal(getattr(r, name).cpu().numpy(), getattr(want, name)), name
    r0 = F.packed_distinct(bits, n=n)
    assert r0.other_id is None and r0.other_hits is None and torch.equal(r0.id, r.id)
    d = smp.distinct(bits, od, n=n)
    _same(d, want, rows, n, (1000,))
    found, hit = d.coverage
    assert float(found) == 25 / 32 and float(hit) == float((want.other_hits > 0).mean())
    rows_k, counts_k, classes_k = d.top(5)
    order = np.argsort(-want.count, kind="stable")[:5]
    assert np.array_equal(classes_k.cpu().numpy(), order) and np.array_equal(counts_k.cpu().numpy(), want.count[order])
    assert torch.equal(rows_k, d.rows[classes_k])
    with pytest.raises(_lib.DvgError, match="device"):
        F.packed_distinct(bits, od.cpu(), n=n)
    # a view goes in as it is
    wide = torch.zeros((1000, 8), dtype=torch.int32, device="cuda")
    wide[:, 2:5] = bits
    _same(smp.distinct(wide[:, 2:5], n=n), do.distinct(rows, n), rows, n, (1000,))


@functools.lru_cache(maxsize=None)
def _ring16():
    ei = np.arange(16, dtype=np.int64)
    nodes = [f"q{i}" for i in range(16)]
    return graphs.build_plan(16, np.minimum(ei, (ei + 1) % 16), np.maximum(ei, (ei + 1) % 16)), nodes


def _sampler(plan, nodes, beta=2.0, sweeps=4):
    return smp.GibbsSampler(plan, nodes, beta=beta, sweeps=sweeps, seed=SEED, persistent=True, chain_offset=5, h_range=(-4, 4),
                            j_range=(-1, 1))


def test_trace_distinct_pooled_and_per_chain():
    plan, nodes = _ring16()
    s = _sampler(plan, nodes, beta=1.0)
    lin = torch.zeros(16, device="cuda")
    quad = torch.full((plan.n_edges,), -1.0, device="cuda")
    trace = s.sample_trace(lin, quad, 1.0, None, None, num_reads=7, num_sweeps=60, burn_in=10, thin=1)
    assert trace.bits.shape == (7, 50, 1)
    host = trace.bits.cpu().numpy()
    want = do.distinct(host, 16)
    d = trace.distinct()
    _same(d, want, host, 16, (7, 50))
    assert 1 < d.distinct < 350
    per = trace.distinct(pooled=False)
    assert per.is_cuda and per.dtype == torch.int64 and per.shape == (7,)
    assert per.cpu().numpy().tolist() == [do.distinct(host[c], 16).rep.size for c in range(7)]
    # a slice of the records, no copy
    cut = smp.Trace(trace.bits[:, 5:], None, None, trace.sweeps[5:], 16)
    _same(cut.distinct(), do.distinct(host[:, 5:], 16), host[:, 5:], 16, (7, 45))
    assert cut.distinct(pooled=False).cpu().numpy().tolist() == [do.distinct(host[c, 5:], 16).rep.size for c in range(7)]


def test_minima_distinct_is_the_partition_of_unique():
    n = 40
    rows = _content("pool300", 27 * 11, n, seed=2)
    rows[:, -1] &= np.uint32((1 << (n % 32)) - 1)  # (a descent clears the pad bits of what it returns)
    bits = _dev(rows).view(27, 11, 2)
    z32 = torch.zeros((27, 11), dtype=torch.int32, device="cuda")
    z64 = torch.zeros((27, 11), dtype=torch.float64, device="cuda")
    m = smp.Minima.from_outputs(bits, bits, z32, z32, z32, z64, z64, n)
    d = m.distinct()
    _same(d, do.distinct(rows, n), rows, n, (27, 11))
    u_rows, u_counts, u_index = m.unique()
    assert sorted(u_counts.cpu().numpy().tolist()) == sorted(d.counts.cpu().numpy().tolist())
    # the same partition: the two labellings are a bijection of each other, and the labelled rows agree
    pairs = {(int(a), int(b)) for a, b in zip(d.index.cpu().numpy().reshape(-1), u_index.cpu().numpy().reshape(-1))}
    assert len(pairs) == d.distinct == int(u_rows.shape[0])
    assert torch.equal(d.rows[d.index.reshape(-1).long()], u_rows[u_index.reshape(-1)])
    assert abs(float(d.entropy) - float(m.basin_entropy)) <= 1e-12


def test_sample_set_aggregate_and_the_histogram_answer_mode():
    plan, nodes = _ring16()
    h = {v: 0.1 * ((i % 3) - 1) for i, v in enumerate(nodes)}
    J = {(nodes[i], nodes[(i + 1) % 16]): -1.0 for i in range(16)}
    reads = 400
    raw = _sampler(plan, nodes, beta=1.0, sweeps=8).sample_ising(h, J, num_reads=reads, answer_mode="raw")
    hist = _sampler(plan, nodes, beta=1.0, sweeps=8).sample_ising(h, J, num_reads=reads, answer_mode="histogram")
    assert len(raw) == reads and raw.record.num_occurrences.tolist() == [1] * reads
    samples, energy = raw.record.sample, raw.record.energy
    want = do.distinct(smp.pack_spins(torch.from_numpy(samples)).numpy(), 16)
    D = want.rep.size
    assert 1 < D < reads
    # aggregate(): first-occurrence order
    agg = raw.aggregate()
    assert len(agg) == D and agg.device_tensor.is_cuda and agg.variables == raw.variables
    assert np.array_equal(agg.record.sample, samples[want.rep]) and np.array_equal(agg.record.num_occurrences, want.count)
    assert np.array_equal(agg.record.energy, energy[want.rep]) and agg.record.num_occurrences.dtype == np.int64
    assert np.array_equal(agg.aggregate().record.num_occurrences, want.count)
    host_only = smp.SampleSet(samples, raw.variables, energy=energy).aggregate()
    assert np.array_equal(host_only.record.sample, agg.record.sample) and np.array_equal(host_only.record.num_occurrences, want.count)
    # histogram: by rising energy, ties by first occurrence
    order = np.argsort(energy[want.rep], kind="stable")
    rec = hist.record
    assert len(hist) == D and int(rec.num_occurrences.sum()) == reads
    assert len({tuple(r) for r in rec.sample.tolist()}) == D and np.all(np.diff(rec.energy) >= 0)
    assert np.array_equal(rec.sample, samples[want.rep][order]) and np.array_equal(rec.num_occurrences, want.count[order])
    assert np.array_equal(rec.energy, energy[want.rep][order])
    # every other value behaves as "raw"
    other = _sampler(plan, nodes, beta=1.0, sweeps=8).sample_ising(h, J, num_reads=reads, answer_mode="anything")
    assert np.array_equal(other.record.sample, samples) and other.record.num_occurrences.tolist() == [1] * reads


def test_model_wrapper_latent_usage_and_prior_distinct():
    from image_generation_amd.data import synthetic_images
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    m.overlap_sampler = False  # (as in the overlap file: this test takes no stream from the process's pool)
    B = 6
    images = synthetic_images(B, seed=3, device="cuda").reshape(B, 1, 32, 32)
    images = torch.cat([images, images[1:3]])  # two images twice: equal codes among the data
    m._dvae.eval()  # (as latent_usage encodes)
    with torch.no_grad():
        spins = F.heaviside_latent_to_discrete(m._dvae.encoder(images)).squeeze(1)
    samples = torch.where(torch.rand((33, 64), device="cuda") < 0.5, -1.0, 1.0)
    samples[4], samples[9], samples[20] = spins[2], spins[2], spins[5]  # copies of data latents
    use = m.latent_usage(images, samples)
    nov = m.latent_novelty(images, samples)
    assert set(use) == {"data", "drawn", "copied_share", "data_found_share"}
    data, drawn = smp.pack_spins(spins).cpu().numpy(), smp.pack_spins(samples).cpu().numpy()
    _same(use["data"], do.distinct(data, 64), data, 64, (B + 2,))
    want = do.distinct(drawn, 64, data)
    _same(use["drawn"], want, drawn, 64, (33,))
    assert np.array_equal(use["drawn"].other_id.cpu().numpy(), want.other_id)
    copied = (nov["nearest_dist"] == 0).to(torch.float64).mean()
    assert float(use["copied_share"]) == float(copied) and float(copied) >= 3 / 33
    found = float(use["data_found_share"])
    assert found == float((want.other_id >= 0).mean()) and found >= 3 / (B + 2)
    # the data codes that occur more than once are the ones at distance 0 from another data code
    twice = use["data"].counts[use["data"].index.long()] > 1
    assert torch.equal(twice, nov["data_nearest_dist"] == 0) and int(twice.sum()) >= 4
    # samples=None draws one sample set as generate_images does; prior_distinct is the Distinct of such a draw
    reads = int(m.sampler_kwargs.get("num_reads", 1))
    drew = m.latent_usage(images)
    assert drew["drawn"].count == reads and drew["data"].distinct == use["data"].distinct
    p = m.prior_distinct()
    assert isinstance(p, smp.Distinct) and p.count == reads and p.n == 64 and 1 <= p.distinct <= reads
    assert m.prior_distinct(num_reads=17).count == 17
