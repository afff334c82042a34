"""CPU-side checks of the distinct-row counts of bit-packed rows ("DVG distinct v1", ``dvg_packed_distinct`` in include/dvg.h):
the symbols, every argument error of the C entry (before any HIP call: null stream, no device) and of the Python surface
(before the library is touched), the workspace query, the arithmetic of ``sampler.Distinct`` on hand-made counts,
``SampleSet.aggregate()`` on a host-only set against the numpy definition (``tests/distinct_oracle.py``), and the dev option."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distinct_oracle as do  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4


# ------------------------------------------------------------------------------------------------ the symbols and their checks
def test_symbols_are_declared_bound_and_exported():
    support.assert_declared_bound_exported({"dvg_packed_distinct": "int", "dvg_packed_distinct_workspace_bytes": "size_t"}, markers=["DVG distinct v1"])


def test_error_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "dvg.h")).read()
    for name, value in (("DVG_E_INVALID", INVALID), ("DVG_E_WORKSPACE", WORKSPACE), ("DVG_E_UNSUPPORTED", UNSUPPORTED)):
        assert re.search(r"#define\s+" + name + r"\s+\(" + str(value) + r"\)", text), name


_KEEP = ctypes.create_string_buffer(64)
P = ctypes.cast(_KEEP, ctypes.c_void_p)  # a host stand-in pointer: nothing reaches HIP


def _call(*, bits=P, rows=5, rs=2, groups=1, gs=0, n=64, other=None, rows_other=0, o_rs=0, first=None, id=None, rep=None, count=None,
          n_distinct=P, other_id=None, other_hits=None, ws=P, ws_bytes=1 << 40):
    L = _lib.lib()
    rc = L.dvg_packed_distinct(bits, rows, rs, groups, gs, n, other, rows_other, o_rs, first, id, rep, count, n_distinct, other_id,
                               other_hits, ws, ws_bytes, None)
    return rc, L.dvg_last_error()


def test_c_argument_validation_without_gpu():
    """Every error of the header's list with its code and a message that names the argument."""
    for name in ("bits", "n_distinct", "ws"):
        rc, msg = _call(**{name: None})
        assert rc == INVALID and re.search(rb"\b" + name.encode() + rb"\b", msg), (name, rc, msg)
    for name in ("rows", "groups", "n"):
        for bad in (0, -1, -2 ** 31):
            rc, msg = _call(**{name: bad})
            assert rc == INVALID and re.search(rb"\b" + name.encode() + rb"\b", msg), (name, bad, rc, msg)
    for bad in (1, 0, -1, -2 ** 40):  # n = 64: two words a row
        rc, msg = _call(rs=bad)
        assert rc == INVALID and b"row_stride" in msg and b"other" not in msg, (bad, rc, msg)
    rc, msg = _call(n=65, rs=2)  # a row stride is measured against W = ceil(n / 32)
    assert rc == INVALID and b"row_stride" in msg, (rc, msg)
    for bad in (-1, -2 ** 40):
        rc, msg = _call(groups=3, gs=bad)
        assert rc == INVALID and b"group_stride" in msg, (bad, rc, msg)
    for bad in (0, -1, -2 ** 40):
        rc, msg = _call(other=P, rows_other=bad, o_rs=2)
        assert rc == INVALID and b"rows_other" in msg, (bad, rc, msg)
    for bad in (1, 0, -3):
        rc, msg = _call(other=P, rows_other=4, o_rs=bad)
        assert rc == INVALID and b"other_row_stride" in msg, (bad, rc, msg)
    for name in ("other_id", "other_hits"):
        rc, msg = _call(**{name: P})
        assert rc == INVALID and name.encode() in msg and b"without other" in msg, (name, rc, msg)
    # without `other`, rows_other and its stride are ignored: this reaches the workspace check
    rc, msg = _call(rows_other=-7, o_rs=-7, ws_bytes=0)
    assert rc == WORKSPACE, (rc, msg)
    # int32 indices
    for kw in (dict(rows=2 ** 31), dict(rows=2 ** 40), dict(rows=2 ** 16, rs=2, groups=2 ** 15), dict(rows=2 ** 62, groups=2 ** 62)):
        rc, msg = _call(**kw)
        assert rc == UNSUPPORTED and b"2^31" in msg and b"rows" in msg, (kw, rc, msg)
    for bad in (2 ** 31, 2 ** 40):
        rc, msg = _call(other=P, rows_other=bad, o_rs=2)
        assert rc == UNSUPPORTED and b"rows_other" in msg, (bad, rc, msg)
    # the workspace: one byte short is an error, and an error comes before any launch
    L = _lib.lib()
    need = L.dvg_packed_distinct_workspace_bytes(5, 3, 64)
    for short in (0, 16, need - 1):
        rc, msg = _call(groups=3, gs=10, ws_bytes=short)
        assert rc == WORKSPACE and b"workspace" in msg and str(need).encode() in msg, (short, rc, msg)


def test_workspace_query():
    L = _lib.lib()
    q = L.dvg_packed_distinct_workspace_bytes
    for bad in ((0, 1, 64), (-1, 1, 64), (5, 0, 64), (5, -2, 64), (5, 1, 0), (5, 1, -3), (2 ** 31, 1, 64), (2 ** 16, 2 ** 15, 64),
                (2 ** 62, 2 ** 62, 64)):
        assert q(*bad) == 0, bad
    sizes = [q(r, 1, 256) for r in (1, 2, 3, 63, 64, 65, 1000, 1024, 1025, 4096, 2 ** 20, 2 ** 20 + 1, 2 ** 24, 2 ** 31 - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] > sizes[0]
    # the table holds at least 2 T int32 slots, and the pooled rows of groups count like rows
    assert q(1000, 1, 33) >= 2 * 1000 * 4 and q(10, 100, 33) == q(1000, 1, 33) and q(1000, 1, 33) == q(1000, 1, 1024)


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture
def untouched(monkeypatch):
    """The library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch, F)


def test_functional_wrapper_rejects_bad_arguments(untouched):
    flat = torch.zeros((5, 3), dtype=torch.int32)  # n = 77: three words
    trace = torch.zeros((4, 6, 3), dtype=torch.int32)
    for bad in (flat.long(), flat.float(), flat[0], flat[None, None], torch.zeros((5, 2), dtype=torch.int32),
                torch.zeros((5, 4), dtype=torch.int32), torch.zeros((0, 3), dtype=torch.int32),
                torch.zeros((4, 0, 3), dtype=torch.int32), flat.numpy(), None):
        with pytest.raises(_lib.DvgError, match=r"\bbits must"):
            F.packed_distinct(bad, n=77)
        with pytest.raises(_lib.DvgError, match=r"\bother must"):
            F.packed_distinct(flat, bad if bad is not None else "rows", n=77)
    with pytest.raises(_lib.DvgError, match=r"\bother must"):  # other is a flat set
        F.packed_distinct(flat, trace, n=77)
    for bad in (0, -5, 2.0, True, "77", None):
        with pytest.raises(ValueError, match="n must"):
            F.packed_distinct(flat, n=bad)
    # an n that does not match the row width, an other of another width
    for n in (64, 96 + 1, 1):
        with pytest.raises(_lib.DvgError, match=r"\bbits must"):
            F.packed_distinct(flat, n=n)
    with pytest.raises(_lib.DvgError, match=r"\bother must"):
        F.packed_distinct(flat, torch.zeros((5, 1), dtype=torch.int32), n=77)
    # strides: the last dimension must be dense, a row must not overlap the next, no stride is negative
    wide = torch.zeros((5, 6), dtype=torch.int32)
    with pytest.raises(_lib.DvgError, match="bits: the last dimension"):
        F.packed_distinct(wide[:, ::2], n=77)
    with pytest.raises(_lib.DvgError, match="other: the last dimension"):
        F.packed_distinct(flat, wide[:, ::2], n=77)
    with pytest.raises(_lib.DvgError, match="bits: a row stride"):
        F.packed_distinct(flat[:1].expand(5, 3), n=77)
    with pytest.raises(_lib.DvgError, match="bits: a row stride"):
        F.packed_distinct(torch.zeros((9,), dtype=torch.int32).as_strided((4, 3), (2, 1)), n=77)
    with pytest.raises(_lib.DvgError, match="other: a row stride"):
        F.packed_distinct(flat, torch.zeros((9,), dtype=torch.int32).as_strided((4, 3), (2, 1)), n=77)
    with pytest.raises(_lib.DvgError, match="bits: a row stride"):
        F.packed_distinct(trace[:, :1].expand(4, 6, 3), n=77)
    with pytest.raises((RuntimeError, _lib.DvgError)):  # torch itself refuses a negative stride
        F.packed_distinct(torch.zeros((15,), dtype=torch.int32).as_strided((4, 3), (-3, 1), 12), n=77)
    for ok in ((flat, None), (flat, flat[::2]), (trace, None), (trace, flat), (trace[:, 1:], flat), (trace[1:3], None), (wide[:, :3], None)):
        with pytest.raises(_lib.DvgError, match="GPU"):  # valid arguments on CPU tensors: the HIP path has no CPU fallback
            F.packed_distinct(*ok, n=77)
    with pytest.raises(_lib.DvgError, match="GPU"):
        F.packed_distinct_counts(trace, n=77)
    with pytest.raises(_lib.DvgError, match=r"\bbits must"):
        F.packed_distinct_counts(flat, n=77)


def test_consumers_reach_the_device_check_only(untouched):
    t = smp.Trace(torch.zeros((3, 10, 1), dtype=torch.int32), None, None, smp.trace_sweeps(10, 0, 1), 12)
    for pooled in (True, False):
        with pytest.raises(_lib.DvgError, match="GPU"):
            t.distinct(pooled=pooled)
    with pytest.raises(_lib.DvgError, match="GPU"):
        smp.distinct(torch.zeros((7, 1), dtype=torch.int32), n=12)
    z32, z64 = torch.zeros((7,), dtype=torch.int32), torch.zeros((7,), dtype=torch.float64)
    m = smp.Minima.from_outputs(torch.zeros((7, 1), dtype=torch.int32), torch.zeros((7, 1), dtype=torch.int32), z32, z32, z32, z64, z64, 12)
    with pytest.raises(_lib.DvgError, match="GPU"):
        m.distinct()


def test_sample_ising_answer_mode_goes_no_further_than_argument_handling(untouched):
    """``answer_mode`` is not validated and is looked at only after the draw: with it, every argument error is raised as before,
    in front of anything that touches the library."""
    ei = np.arange(12, dtype=np.int64)
    plan = graphs.build_plan(12, np.minimum(ei, (ei + 1) % 12), np.maximum(ei, (ei + 1) % 12))
    s = smp.GibbsSampler(plan, [f"q{i}" for i in range(12)], beta=2.0, sweeps=5, seed=3, device="cuda")
    for mode in ("histogram", "raw", "anything", None):
        with pytest.raises(ValueError, match="auto_scale"):
            s.sample_ising({}, {}, num_reads=4, answer_mode=mode, auto_scale=True)
        with pytest.raises(ValueError, match="num_sweeps needs"):
            s.sample_ising({}, {}, num_reads=4, answer_mode=mode, num_sweeps=5)
        with pytest.raises(ValueError, match="not an edge"):
            s.sample_ising({}, {("q0", "q5"): 1.0}, num_reads=4, answer_mode=mode)


# ------------------------------------------------------------------------------------------------ Distinct's arithmetic
def _distinct_of(ident, n=40):
    """A Distinct of rows whose classes are ``ident`` (numbered by first occurrence), each class a row of its own bits."""
    ident = np.asarray(ident)
    words = np.stack([ident.astype(np.int64) * 7 + 1, np.zeros_like(ident, dtype=np.int64)], axis=1).astype(np.int32)
    o = do.distinct(words, n)
    assert np.array_equal(o.id, ident)
    d = smp.Distinct.from_outputs(torch.from_numpy(words), torch.from_numpy(o.first), torch.from_numpy(o.id), torch.from_numpy(o.rep),
                                  torch.from_numpy(o.count), n)
    return d, o, words


def test_distinct_arithmetic_on_hand_made_counts():
    d, o, words = _distinct_of([0, 1, 0, 2, 0, 1, 3])  # counts 3, 2, 1, 1
    assert (d.n, d.count, d.distinct) == (40, 7, 4) and "Distinct(" in repr(d)
    assert d.counts.tolist() == [3, 2, 1, 1] and d.index.tolist() == [0, 1, 0, 2, 0, 1, 3] and d.first.tolist() == [0, 1, 0, 3, 0, 1, 6]
    assert torch.equal(d.rows, torch.from_numpy(words[[0, 1, 3, 6]]))
    assert int(d.singletons) == 2 and d.singletons.dtype == torch.int64
    p = np.array([3, 2, 1, 1]) / 7.0
    assert d.entropy.dtype == torch.float64 and abs(float(d.entropy) - float(-(p * np.log(p)).sum())) < 1e-15
    assert float(d.collision_share) == (3 * 2 + 2 * 1) / (7 * 6) and d.collision_share.dtype == torch.float64
    assert float(d.unseen_mass) == 2 / 7 and d.coverage is None
    want = do.estimates(o.count)
    for name in ("entropy", "collision_share", "unseen_mass", "singletons"):
        assert abs(float(getattr(d, name)) - want[name]) <= 1e-15, name
    # all equal, all distinct, one row
    d, _o, _w = _distinct_of([0] * 9)
    assert (d.distinct, float(d.entropy), float(d.collision_share), float(d.unseen_mass)) == (1, 0.0, 1.0, 0.0)
    d, _o, _w = _distinct_of(list(range(8)))
    assert d.distinct == 8 and abs(float(d.entropy) - np.log(8.0)) < 1e-15 and float(d.collision_share) == 0.0 and float(d.unseen_mass) == 1.0
    d, _o, _w = _distinct_of([0])
    assert d.distinct == 1 and float(d.entropy) == 0.0 and np.isnan(float(d.collision_share)) and float(d.unseen_mass) == 1.0


def test_top_sorts_by_count_and_breaks_ties_by_first_occurrence():
    d, _o, words = _distinct_of([0, 1, 2, 1, 3, 2, 4, 3, 3])  # counts 1, 2, 2, 3, 1
    rows, counts, classes = d.top(3)
    assert counts.tolist() == [3, 2, 2] and classes.tolist() == [3, 1, 2]
    assert torch.equal(rows, d.rows[classes])
    rows, counts, classes = d.top(100)
    assert counts.tolist() == [3, 2, 2, 1, 1] and classes.tolist() == [3, 1, 2, 0, 4]
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="k must"):
            d.top(bad)


def test_distinct_from_outputs_on_a_trace_shape_masks_pad_bits_and_carries_coverage():
    rng = np.random.default_rng(5)
    n, C, M = 40, 3, 5
    pool = rng.integers(0, 2 ** 32, size=(4, 2), dtype=np.uint64).astype(np.uint32)
    bits = pool[rng.integers(0, 4, size=C * M)]
    bits[:, 1] = (bits[:, 1] & np.uint32(0xFF)) | (rng.integers(0, 2 ** 24, size=C * M, dtype=np.uint64).astype(np.uint32) << np.uint32(8))
    other = np.concatenate([bits[[2, 2, 7]], ~bits[:1]])
    o = do.distinct(bits.reshape(C, M, 2), n, other)
    tb = torch.from_numpy(bits.view(np.int32).reshape(C, M, 2))
    d = smp.Distinct.from_outputs(tb, *(torch.from_numpy(x) for x in (o.first, o.id, o.rep, o.count)), n, torch.from_numpy(o.other_id),
                                  torch.from_numpy(o.other_hits))
    assert d.index.shape == (C, M) and d.first.shape == (C, M) and d.count == C * M
    assert np.array_equal(d.rows.numpy().view(np.uint32), do.keys(bits, n)[o.rep])
    found, hit = d.coverage
    assert float(found) == 3 / 4 and float(hit) == float((o.other_hits > 0).mean()) and int(o.other_hits.sum()) == 3
    for bad in (dict(n=0), dict(n=True), dict(n=64 + 1), dict(first=torch.from_numpy(o.first).long()), dict(rep=torch.from_numpy(o.rep)[:0]),
                dict(count=torch.from_numpy(o.count)[:-1]), dict(other_hits=None)):
        kw = dict(bits=tb, first=torch.from_numpy(o.first), id=torch.from_numpy(o.id), rep=torch.from_numpy(o.rep),
                  count=torch.from_numpy(o.count), n=n, other_id=torch.from_numpy(o.other_id), other_hits=torch.from_numpy(o.other_hits))
        kw.update(bad)
        with pytest.raises(ValueError):
            smp.Distinct.from_outputs(**kw)


# ------------------------------------------------------------------------------------------------ SampleSet.aggregate on the host
def test_raw_sets_count_every_read_once():
    s = smp.SampleSet(np.ones((5, 3), dtype=np.int8), ["a", "b", "c"], energy=np.zeros(5))
    assert s.record.num_occurrences.tolist() == [1] * 5 and s.record.num_occurrences.dtype == np.int64


def test_host_only_aggregate_equals_the_oracle():
    rng = np.random.default_rng(11)
    n, reads = 37, 200
    pool = (2 * rng.integers(0, 2, size=(9, n)) - 1).astype(np.int8)
    pick = rng.integers(0, 9, size=reads)
    samples = pool[pick]
    energy = rng.standard_normal(9)[pick]
    s = smp.SampleSet(samples, list(range(n)), energy=energy)
    agg = s.aggregate()
    packed = smp.pack_spins(torch.from_numpy(samples)).numpy()
    o = do.distinct(packed, n)
    assert len(agg) == o.rep.size == len(np.unique(pick)) and agg.variables == s.variables and agg.vartype == s.vartype
    assert np.array_equal(agg.record.sample, samples[o.rep]) and agg.record.sample.dtype == np.int8
    assert np.array_equal(agg.record.num_occurrences, o.count) and agg.record.num_occurrences.dtype == np.int64
    assert np.array_equal(agg.record.energy, energy[o.rep]) and int(agg.record.num_occurrences.sum()) == reads
    assert s.record.num_occurrences.tolist() == [1] * reads and len(s) == reads  # (the raw set is left as it was)
    # aggregating twice changes nothing; aggregating a set with occurrences adds them up
    again = agg.aggregate()
    assert np.array_equal(again.record.sample, agg.record.sample) and np.array_equal(again.record.num_occurrences, o.count)
    weighed = smp.SampleSet(samples, list(range(n)), energy=energy, num_occurrences=np.arange(1, reads + 1)).aggregate()
    assert np.array_equal(weighed.record.num_occurrences, np.bincount(o.id, weights=np.arange(1, reads + 1)).astype(np.int64))
    # by energy, ties in first-occurrence order
    by_e = agg._sorted_by_energy()
    order = np.argsort(energy[o.rep], kind="stable")
    assert np.array_equal(by_e.record.sample, samples[o.rep][order]) and np.array_equal(by_e.record.num_occurrences, o.count[order])
    assert np.all(np.diff(by_e.record.energy) >= 0)


# ------------------------------------------------------------------------------------------------ the dev option
def test_the_hash_knob_is_a_dev_option_with_default_minus_one():
    opts, dev = _lib.options(), _lib.dev_options()
    assert "distinct_hash_bits" in dev and "distinct_hash_bits" not in opts and len(opts) <= 8
    value, doc = dev["distinct_hash_bits"]
    assert value == -1 and doc
    assert _lib.lib().dvg_set_option(b"distinct_hash_bits", 0) != 0  # not reachable through the public switches
    with _lib.option_scope(distinct_hash_bits=3):
        assert _lib.get_option("distinct_hash_bits") == 3
    assert _lib.get_option("distinct_hash_bits") == -1
