"""CPU-side checks of the weighed per-chain-field draw ("DVG field AIS v1", ``dvg_gibbs_sample_fields_ais`` in include/dvg.h):
the symbol, the helper the GPU tests hold the kernel to (``tests/field_ais_oracle.py``) against the helpers of the two draws it
joins, every argument error of the C entry point (before any HIP call) and of ``GibbsSampler.sample_fields_ais`` /
``log_evidence`` (before the library is touched), the plan of the new kind -- the field kind's -- and ``LogEvidence`` against the
estimator of ``tests/ais_oracle.py``."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_oracle  # noqa: E402
import field_ais_oracle as fao  # noqa: E402
import field_oracle  # noqa: E402
import test_gibbs_plan_host as pinned  # noqa: E402  (its graphs)
import support  # noqa: E402
from image_generation_amd import _lib, dev, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

SEED = 775321899904
# (graph, chains) of tests/test_gpu_gibbs_field_ais.py
GPU_ROWS = (("random77", 19), ("random77", 20), ("random77", 21), ("zephyr128", 5), ("zephyr128", 1025), ("zephyr512", 9),
            ("zephyr1024", 5))


# ------------------------------------------------------------------------------------------------ the symbol
def test_symbol_is_declared_bound_and_exported():
    name = "dvg_gibbs_sample_fields_ais"
    support.assert_declared_bound_exported(name, markers=["DVG field AIS v1"])
    assert "No held, annealed, weighed, exchange or traced form of this draw" not in support.header_text()
    # dvg_gibbs_sample_fields' arguments without the fixed beta, the two tables in its place, R behind the stride and the two
    # float64 outputs behind samples_out
    c = ctypes
    field, got = _lib.SIGNATURES["dvg_gibbs_sample_fields"][1], _lib.SIGNATURES[name][1]
    tables = [c.c_void_p, c.c_int64, c.c_float, c.c_void_p, c.c_int64, c.c_float]
    assert got == field[:8] + tables + field[9:18] + [c.c_int] + field[18:19] + [c.c_void_p, c.c_void_p] + field[19:]
    # appended: the ids the other kinds had stay theirs
    assert dev.GIBBS_WEIGHED_KIND_IDS == dict(field_weigh=7) and 7 not in dev.GIBBS_KIND_IDS.values()


# ------------------------------------------------------------------------------------------------ the helper and its parents
def _small(n=24, p_edge=0.3, seed=24):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.uniform(size=iu.size) < p_edge
    plan = graphs.build_plan(n, iu[keep].astype(np.int64), ju[keep].astype(np.int64))
    h = rng.uniform(-1, 1, n).astype(np.float32)
    J = rng.uniform(-1, 1, plan.n_edges).astype(np.float32)
    return plan, h, J, rng


def test_local_fields_are_the_ais_helpers_chain_by_chain():
    plan, h, J, rng = _small()
    C, n = 5, plan.n
    hs = rng.standard_normal((C, n)).astype(np.float32)
    Js = gibbs.scaled_fields(h, J, 0.7, None, (-0.5, 0.5))[1]
    st = np.where(rng.uniform(size=(C, n)) < 0.5, -1, 1).astype(np.int8)
    spins = np.array([0, 5, 7, n - 1])
    got = fao.local_fields(st, spins, hs, Js, plan)
    for c in range(C):
        assert np.array_equal(got[c], ais_oracle.fields(st[c:c + 1], spins, hs[c], Js, plan)[0])


def test_zero_fields_and_no_scales_are_the_ais_helper():
    """The same spins; log_w and energy equal (the same float64 operations in the same order); N counts S more multiply-adds."""
    plan, h, J, rng = _small()
    C, n, S, sweep0, prefactor, h_range = 6, plan.n, 4, 5, 0.7, (-0.4, 0.4)
    hs, Js = gibbs.scaled_fields(h, J, prefactor, h_range, (-0.5, 0.5))
    ids = np.arange(C, dtype=np.uint32) + 11
    start = np.where(rng.uniform(size=(C, n)) < 0.5, -1, 1).astype(np.int8)
    for betas in (np.linspace(0.2, 1.5, S).astype(np.float32), rng.uniform(0, 2, (C, S)).astype(np.float32)):
        for st, beta_from in ((None, 0.0), (start, 0.3)):
            want = ais_oracle.ais(plan, hs, Js, betas, ids, SEED, sweep0, start=st, beta_from=beta_from)
            for zeros in (np.zeros(n, np.float32), np.zeros((C, n), np.float32)):
                got = fao.field_ais(plan, h, zeros, prefactor, h_range, Js, betas, None, ids, SEED, sweep0, start=st,
                                    beta_from=beta_from)
                assert np.array_equal(got.spins, want.spins)
                assert np.array_equal(got.log_w, want.log_w) and np.array_equal(got.energy, want.energy)
                assert np.array_equal(got.A, want.A) and got.N == want.N + S
            assert np.abs(want.log_w).min() > 0


def test_a_constant_beta_without_scales_is_the_field_helper_and_weighs_nothing():
    plan, h, J, rng = _small()
    C, n, S, sweep0, prefactor, h_range, beta = 6, plan.n, 3, 5, 0.7, (-1.0, 1.0), 1.3
    fields = rng.standard_normal((C, n)).astype(np.float32)
    Js = gibbs.scaled_fields(h, J, prefactor, None, (-0.5, 0.5))[1]
    ids = np.arange(C, dtype=np.uint32) + 11
    start = gibbs.init_state(ids, n, SEED, sweep0)
    hs = field_oracle.chain_fields(h, fields, prefactor, h_range)
    want = field_oracle.field_sweeps(start, ids, hs, Js, beta, plan, SEED, sweep0, S)
    for kw in (dict(start=start, beta_from=beta), dict(start=start, beta_from=beta, scale_from=0.25)):  # (no scales: scale_from is not read)
        got = fao.field_ais(plan, h, fields, prefactor, h_range, Js, np.full(S, beta, np.float32), None, ids, SEED, sweep0, **kw)
        assert np.array_equal(got.spins, want) and (got.log_w == 0.0).all() and got.N == n + n * S + 2 * S
    # scales of 1 given explicitly: the same rows, so the same draw, d_k == 0
    one = fao.field_ais(plan, h, fields, prefactor, h_range, Js, np.full(S, beta, np.float32), np.ones(S, np.float32), ids, SEED,
                        sweep0, start=start, beta_from=beta, scale_from=1.0)
    assert np.array_equal(one.spins, want) and (one.log_w == 0.0).all() and np.array_equal(one.energy, got.energy)
    assert one.N == n + 2 * n * S + 2 * S and np.array_equal(one.A, got.A)
    # rows shared by R chains are the replicated rows
    R = 3
    shared = fao.field_ais(plan, h, fields[:2], prefactor, h_range, Js, np.full(S, beta, np.float32), None, ids, SEED, sweep0,
                           start=start, beta_from=beta, row_chains=R)
    rep = fao.field_ais(plan, h, np.repeat(fields[:2], R, axis=0), prefactor, h_range, Js, np.full(S, beta, np.float32), None, ids,
                        SEED, sweep0, start=start, beta_from=beta)
    assert np.array_equal(shared.spins, rep.spins) and np.array_equal(shared.energy, rep.energy)


def _grid(plan, rng, C):
    """Parameters on a coarse binary grid: h, J multiples of 1/16, fields of 1/8, to go with strengths that are multiples of 1/4 and
    a prefactor of 1/2 -- every float32 product and sum of the rows and of the local fields is then exact."""
    h = (rng.integers(-8, 9, plan.n) / 16.0).astype(np.float32)
    J = (rng.integers(-8, 9, plan.n_edges) / 16.0).astype(np.float32)
    return h, J, (rng.integers(-16, 17, (C, plan.n)) / 8.0).astype(np.float32)


@pytest.mark.parametrize("per_chain", [False, True])
def test_two_calls_that_hand_the_state_on_are_one_call(per_chain):
    """S1 + S2 sweeps in one call, and in two with beta_from / scale_from the first call's last entries: the same spins, the log
    weights summed.  The second call walks its start energy afresh where the one call carries it on; the two agree up to the
    order of the float64 additions only where the float32 field sums are exact (the carried energy is built from the rounded
    fields the decisions used), so the parameters sit on a binary grid; the betas do not (they enter in float64 alone)."""
    plan, _h, _J, rng = _small()
    C, n, S1, S2, sweep0, prefactor, h_range = 5, plan.n, 3, 4, 6, 0.5, (-0.75, 0.75)
    S = S1 + S2
    h, J, fields = _grid(plan, rng, C)
    Js = gibbs.scaled_fields(h, J, prefactor, None, (-0.25, 0.25))[1]
    ids = np.arange(C, dtype=np.uint32) + 3
    shape = (C, S) if per_chain else (S,)
    betas, scales = rng.uniform(0, 2, shape).astype(np.float32), (rng.integers(0, 7, shape) / 4.0).astype(np.float32)
    rows = fao.chain_rows(h, fields, np.ones(C, np.float32), prefactor, h_range)
    assert 0.05 < (np.abs(rows) == 0.75).mean() < 0.95
    one = fao.field_ais(plan, h, fields, prefactor, h_range, Js, betas, scales, ids, SEED, sweep0, scale_from=0.0)
    a = fao.field_ais(plan, h, fields, prefactor, h_range, Js, betas[..., :S1], scales[..., :S1], ids, SEED, sweep0, scale_from=0.0)
    last_b, last_s = betas[..., S1 - 1], scales[..., S1 - 1]
    if per_chain:  # beta_from and scale_from are scalars: chain by chain
        parts = [fao.field_ais(plan, h, fields[c:c + 1], prefactor, h_range, Js, betas[c:c + 1, S1:], scales[c:c + 1, S1:], ids[c:c + 1],
                               SEED, sweep0 + S1, start=a.spins[c:c + 1], beta_from=last_b[c], scale_from=last_s[c]) for c in range(C)]
        b_spins = np.concatenate([p.spins for p in parts])
        b_w, b_e = np.concatenate([p.log_w for p in parts]), np.concatenate([p.energy for p in parts])
    else:
        b = fao.field_ais(plan, h, fields, prefactor, h_range, Js, betas[S1:], scales[S1:], ids, SEED, sweep0 + S1, start=a.spins,
                          beta_from=last_b, scale_from=last_s)
        b_spins, b_w, b_e = b.spins, b.log_w, b.energy
    assert np.array_equal(b_spins, one.spins) and not np.array_equal(a.spins, one.spins)
    tol = 4.0 * one.N * 2.0 ** -53 * one.A
    table = np.broadcast_to(betas, (C, S)).astype(np.float64)
    assert (np.abs(b_e - one.energy) <= tol).all()
    assert (np.abs(a.log_w + b_w - one.log_w) <= tol * (np.abs(np.diff(table, axis=1, prepend=0.0)).sum(1) + table.sum(1))).all()
    assert np.abs(one.log_w).min() > 0


def test_the_weight_is_the_ais_weight_along_the_path():
    """log_w = -sum_k [beta_k E_k(s^(k)) - beta_{k-1} E_{k-1}(s^(k))] with the energies recomputed from scratch in float64, on a
    graph whose float32 field sums are exact (parameters on a coarse binary grid): the carried energy is then the exact one."""
    plan, _h, _J, rng = _small()
    C, n, S, sweep0 = 4, plan.n, 5, 2
    h = (rng.integers(-8, 9, n) / 16.0).astype(np.float32)
    J = (rng.integers(-8, 9, plan.n_edges) / 16.0).astype(np.float32)
    fields = (rng.integers(-16, 17, (C, n)) / 8.0).astype(np.float32)
    betas = (rng.integers(0, 9, S) / 4.0).astype(np.float32)
    scales = (np.arange(1, S + 1) / 4.0).astype(np.float32)
    ids = np.arange(C, dtype=np.uint32)
    ei, ej = np.asarray(plan.edge_i), np.asarray(plan.edge_j)

    def energy(st, lam):
        row = fao.chain_rows(h, fields, np.full(C, lam, np.float32), 1.0, None).astype(np.float64)
        s = st.astype(np.float64)
        return (row * s).sum(1) + ((s[:, ei] * s[:, ej]) * J.astype(np.float64)).sum(1)

    st = gibbs.init_state(ids, n, SEED, sweep0)
    want, b_prev, l_prev = np.zeros(C), 0.0, 0.5
    for k in range(S):
        want -= float(betas[k]) * energy(st, scales[k]) - b_prev * energy(st, l_prev)
        st = fao.field_ais(plan, h, fields, 1.0, None, J, betas[k:k + 1], scales[k:k + 1], ids, SEED, sweep0 + k, start=st,
                           beta_from=b_prev, scale_from=l_prev).spins
        b_prev, l_prev = float(betas[k]), float(scales[k])
    got = fao.field_ais(plan, h, fields, 1.0, None, J, betas, scales, ids, SEED, sweep0, scale_from=0.5)
    assert np.array_equal(got.spins, st)
    np.testing.assert_allclose(got.log_w, want, rtol=0, atol=1e-11)
    np.testing.assert_allclose(got.energy, energy(st, scales[-1]), rtol=0, atol=1e-11)


# ------------------------------------------------------------------------------------------------ the C entry point's checks
_stand_in = support.graph_stand_in


def _call(g, lin, quad, state, fields, betas, *, scales=None, stride=64, beta_stride=0, scale_stride=0, beta_from=0.0, scale_from=1.0,
          n_chains=8, n_sweeps=7, init=1, R=1, dyn=None):
    L = _lib.lib()
    rc = L.dvg_gibbs_sample_fields_ais(g, lin, quad, 1.0, -1, 1, -1, 1, betas, beta_stride, beta_from, scales, scale_stride, scale_from,
                                       state, n_chains, 0, 0, 0, n_sweeps, init, fields, stride, R, None, None, None, dyn, None)
    return rc, L.dvg_last_error()


def test_argument_validation_without_gpu():
    """Everything the header lists is DVG_E_INVALID (-1) with a message, before any HIP call (there is no device here, and the
    pointers are host memory: a launch would not return -1)."""
    rc, msg = _call(None, None, None, None, None, None)
    assert rc == -1 and b"null" in msg
    graph, g, p, _keep = _stand_in()
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p)):  # what dvg_gibbs_sample rejects
        rc, msg = _call(g, *args)
        assert rc == -1 and b"null" in msg
    for n_chains in (0, -4):
        rc, msg = _call(g, p, p, p, p, p, n_chains=n_chains)
        assert rc == -1 and b"n_chains" in msg
    rc, msg = _call(g, p, p, p, None, p)  # what dvg_gibbs_sample_fields rejects
    assert rc == -1 and b"null fields" in msg
    for stride in (1, 63, 65, 128, -64, 2 ** 40):
        rc, msg = _call(g, p, p, p, p, p, stride=stride)
        assert rc == -1 and b"field_chain_stride" in msg, stride
    for kw in (dict(), dict(stride=0)):
        rc, msg = _call(g, p, p, p, p, p, dyn=p, **kw)
        assert rc == -1 and b"dyn" in msg
    rc, msg = _call(g, p, p, p, p, None)  # what dvg_gibbs_sample_ais rejects
    assert rc == -1 and b"null betas" in msg
    for n_sweeps in (0, -1):
        rc, msg = _call(g, p, p, p, p, p, n_sweeps=n_sweeps)
        assert rc == -1 and b"n_sweeps" in msg
    for bad in (1, 6, 8, 64, -7):
        rc, msg = _call(g, p, p, p, p, p, beta_stride=bad)
        assert rc == -1 and b"beta_chain_stride" in msg, bad
    for bad in (-0.5, float("nan"), float("inf")):
        rc, msg = _call(g, p, p, p, p, p, beta_from=bad, init=0)
        assert rc == -1 and b"beta_from" in msg, bad
    rc, msg = _call(g, p, p, p, p, p, beta_from=0.3, init=1)
    assert rc == -1 and b"fresh chains" in msg
    for bad in (1, 6, 8, 64, -7):  # its own
        rc, msg = _call(g, p, p, p, p, p, scales=p, scale_stride=bad)
        assert rc == -1 and b"scale_chain_stride" in msg, bad
    for bad in (0, -1, -64):
        rc, msg = _call(g, p, p, p, p, p, R=bad)
        assert rc == -1 and b"field_row_chains" in msg, bad
    for bad in (float("nan"), float("inf"), -float("inf")):
        for scales in (None, p):
            rc, msg = _call(g, p, p, p, p, p, scales=scales, scale_from=bad)
            assert rc == -1 and b"scale_from" in msg, bad
    ctypes.c_int32.from_buffer(graph).value = 40000
    rc, msg = _call(g, p, p, p, p, p, stride=40000)
    assert rc == -1 and b"too large" in msg


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture
def untouched(monkeypatch):
    """A sampler on a 12-spin ring, with the library out of reach: any call into it fails the test.  The parameters are CPU
    tensors, as is every tensor a machine without a GPU can make: a call whose other arguments pass ends at the first of them."""
    support.out_of_reach(monkeypatch)
    plan = support.ring_plan()
    n = plan.n
    s = smp.GibbsSampler(plan, list(range(n)), beta=2.0, sweeps=5, seed=3, device="cuda")
    return s, torch.zeros(n), torch.zeros(plan.n_edges)


def _counters(s):
    return (s.sweep_count, s.cond_sweep_count, s.anneal_sweep_count, s.ais_sweep_count, s.field_sweep_count, s.field_ais_sweep_count,
            s.calls)


def test_sample_fields_ais_rejects_bad_arguments(untouched):
    s, lin, quad = untouched
    n = s.plan.n
    assert s.field_ais_seed == 3 ^ 0x66616931
    assert s.field_ais_seed not in (s.seed, s.cond_seed, s.anneal_seed, s.ais_seed, s.trace_seed, s.field_seed, s.pt_seed, s.pa_seed,
                                    s.sqa_seed)
    call = lambda fields, *a, **kw: s.sample_fields_ais(lin, quad, 1.0, None, None, fields, *a, **kw)  # noqa: E731
    good, row, betas = torch.zeros((4, n)), torch.zeros(n), [0.5, 1.0, 2.0]
    with pytest.raises(_lib.DvgError, match="fields must be a tensor"):
        call(np.zeros((4, n), dtype=np.float32), betas)
    for bad in (good.double(), good.to(torch.int8), good.half()):
        with pytest.raises(_lib.DvgError, match="fields must be float32"):
            call(bad, betas)
    for bad in (torch.zeros((4, n + 1)), torch.zeros((0, n)), torch.zeros((2, 2, n)), torch.zeros(n - 1), torch.zeros(())):
        with pytest.raises(_lib.DvgError, match="fields must be"):
            call(bad, betas)
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="chains_per_row"):
            call(good, betas, chains_per_row=bad)
    with pytest.raises(ValueError, match="betas, scales or both"):
        call(good)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta_from"):
            call(good, betas, beta_from=bad, start=torch.ones((4, n), dtype=torch.int8))
    with pytest.raises(ValueError, match="fresh chains"):
        call(good, betas, beta_from=0.3)
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="scale_from"):
            call(good, betas, scale_from=bad)
    with pytest.raises(ValueError, match="start or num_reads"):
        call(row, betas)
    for bad in ([], "4", True, 2.5, 0):
        with pytest.raises(ValueError, match="num_reads"):
            call(row, betas, num_reads=bad)
    # a start or num_reads that disagrees with rows * chains_per_row
    with pytest.raises(_lib.DvgError, match="fields has 4 rows of 1 chains each but the draw has 5 chains"):
        call(good, betas, num_reads=5)
    with pytest.raises(_lib.DvgError, match="fields has 4 rows of 3 chains each but the draw has 4 chains"):
        call(good, betas, chains_per_row=3, num_reads=4)
    # the one order of the start checks, as in every draw: a tensor, its dtype, its shape, the count, on the GPU
    with pytest.raises(_lib.DvgError, match="start must be a tensor"):
        call(good, betas, start=np.ones((4, n), dtype=np.int8))
    with pytest.raises(_lib.DvgError, match="start must be float32 or int8"):
        call(good, betas, start=torch.ones((4, n), dtype=torch.float64))
    with pytest.raises(_lib.DvgError, match="start must be"):
        call(good, betas, start=torch.ones((4, n + 1), dtype=torch.int8))
    with pytest.raises(_lib.DvgError, match="num_reads=5 but start has 4 chains"):
        call(row, betas, start=torch.ones((4, n), dtype=torch.int8), num_reads=5)
    with pytest.raises(_lib.DvgError, match="start must live on the GPU"):
        call(good, betas, start=torch.ones((4, n), dtype=torch.int8))
    # the tables: _annealed_arguments' rules; a table of strengths may be negative, a table of betas not
    for bad in ([], [[0.5, 1.0]] * 3, np.zeros((2, 2, 2)), "ab"):
        with pytest.raises((_lib.DvgError, ValueError), match="betas"):
            call(good, bad)
        with pytest.raises((_lib.DvgError, ValueError), match="scales"):
            call(good, betas, bad)
    for bad in ([0.5, -1.0], [0.5, float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="betas"):
            call(good, bad)
    for bad in ([0.5, float("nan"), 1.0], [float("inf"), 0.0, 0.0], [1e39, 0.0, 0.0]):
        with pytest.raises(ValueError, match="scales"):
            call(good, betas, bad)
    with pytest.raises(_lib.DvgError, match="betas names 3 sweeps, scales 2"):
        call(good, betas, [0.5, 1.0])
    # everything else in order (negative strengths, a table per chain over rows * chains_per_row chains): the call ends at the
    # first tensor that is not on the GPU -- a CPU tensor of fields is an error, the HIP path has no CPU fallback
    for a, kw in (((betas, [-0.5, 0.0, 1.0]), {}), ((None, [0.5, 1.0]), {}), ((np.ones((8, 3)), np.ones((8, 3))), dict(chains_per_row=2)),
                  ((betas,), dict(num_reads=8, chains_per_row=2))):
        with pytest.raises(_lib.DvgError, match="fields must live on the GPU"):
            call(good, *a, **kw)
    with pytest.raises(_lib.DvgError, match="fields must live on the GPU"):
        call(row, betas, num_reads=4)
    assert _counters(s) == (0,) * 7 and s._state is None
    s.field_ais_sweep_count = 9
    s.reset()
    assert s.field_ais_sweep_count == 0


def test_log_evidence_rejects_bad_arguments(untouched):
    s, lin, quad = untouched
    n = s.plan.n
    call = lambda fields, **kw: s.log_evidence(lin, quad, 1.0, None, None, fields, **kw)  # noqa: E731
    for bad in (np.zeros((4, n), np.float32), torch.zeros(n), torch.zeros((4, n + 1)), torch.zeros((0, n))):
        with pytest.raises(_lib.DvgError, match="fields must be a"):
            call(bad)
    for kw in (dict(chains_per_row=0), dict(chains_per_row=1.5), dict(num_sweeps=0), dict(num_sweeps=True), dict(burn_in=-1), dict(burn_in="3")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            call(torch.zeros((4, n)), **kw)
    with pytest.raises(_lib.DvgError, match="must live on the GPU"):
        call(torch.zeros((4, n)))
    assert _counters(s) == (0,) * 7


def test_log_evidence_reduces_each_row_as_the_ais_estimator_does():
    rng = np.random.default_rng(7)
    lw = rng.normal(0.0, 2.0, (5, 64))
    res = smp.LogEvidence.from_weights(torch.from_numpy(lw), samples=None)
    assert res.log_ratio.shape == (5,) and res.log_ratio.dtype == torch.float64 and res.log_weights.shape == (5, 64)
    for r in range(5):
        est, ess, std_err = fao.log_ratio_estimate(lw[r])
        assert abs(float(res.log_ratio[r]) - est) < 1e-12 and abs(float(res.ess[r]) - ess) < 1e-9 * ess
        assert abs(float(res.std_err[r]) - std_err) < 1e-12
    assert "rows=5" in repr(res)
    equal = smp.LogEvidence.from_weights(torch.full((2, 8), -3.0, dtype=torch.float64))
    assert torch.allclose(equal.log_ratio, torch.full((2,), -3.0, dtype=torch.float64)) and torch.allclose(equal.ess, torch.full((2,), 8.0, dtype=torch.float64))
    assert float(equal.std_err.max()) < 1e-7


# ------------------------------------------------------------------------------------------------ the plan
@pytest.fixture(scope="module")
def plans():
    return {name: pinned.grid.build_graph(name) for name in sorted({name for name, _c in GPU_ROWS})}


@pytest.mark.parametrize("name,C", GPU_ROWS)
def test_the_weighed_field_kind_takes_the_field_kinds_plan(plans, name, C):
    _lib.check(_lib.lib().dvg_reset_options(), "dvg_reset_options")
    for option in (0, 1, 2, 3, 4):
        with _lib.option_scope(gibbs_generic=option):
            want, got = dev.gibbs_draw_plan(plans[name], C, "field"), dev.gibbs_draw_plan(plans[name], C, "field_weigh")
        assert got == want and got["form"] == "rolled", (name, C, option, got, want)
    with pytest.raises(KeyError):
        dev.gibbs_draw_plan(plans[name], C, "field_weighed")


def test_the_dev_hook_knows_kinds_up_to_the_new_one():
    plan = pinned.grid.build_graph("random77")
    class_ptr = np.ascontiguousarray(plan.class_ptr, dtype=np.int32)
    adj_ptr = np.ascontiguousarray(plan.adj_ptr, dtype=np.int32)
    o = (ctypes.c_int64 * 19)()
    hook = lambda kind: _lib.lib().dvg_dev_gibbs_draw_plan(int(plan.n), int(plan.n_colours), class_ptr.ctypes.data,  # noqa: E731
                                                           adj_ptr.ctypes.data, 19, kind, o)
    assert hook(7) == 0 and hook(8) == -1 and hook(4) == -1 and hook(-1) == -1


# ------------------------------------------------------------------------------------------------ the layers above
def test_the_layers_above_have_the_methods():
    from image_generation_amd.model_wrapper import ModelWrapper
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    grbm = GraphRestrictedBoltzmannMachine([0, 1, 2], [(0, 1), (1, 2)])
    for name in ("sample_fields", "log_evidence"):
        assert callable(getattr(grbm, name))
        with pytest.raises(TypeError, match="local GibbsSampler"):
            getattr(grbm, name)(object(), torch.zeros((1, 3)), prefactor=1.0)
    assert callable(ModelWrapper.prior_log_evidence)
    assert "log sum_z p(z) q(z | x)" in ModelWrapper.prior_log_evidence.__doc__ and "linear_range" in ModelWrapper.prior_log_evidence.__doc__
    assert "equilibrium" in smp.GibbsSampler.log_evidence.__doc__
