"""CPU-side checks of the per-chain-field draw ("DVG field v1", ``dvg_gibbs_sample_fields`` in include/dvg.h): the symbol, the
helper the GPU tests hold the kernel to (``tests/field_oracle.py``) against the oracle called chain by chain, every argument
error of the C entry point (before any HIP call) and of ``GibbsSampler.sample_fields`` (before the library is touched), the
plan the draw takes -- rolled on every graph, a float32 row of hs per chain slot in the LDS, the workgroup stepped down to what
fits -- with the other kinds' plans where they were, and ``logit_fields`` against enumeration."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_oracle  # noqa: E402
import test_gibbs_plan_host as pinned  # noqa: E402  (the table of the existing kinds' plans, and its graphs)
import support  # noqa: E402
from image_generation_amd import _lib, dev, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

SEED = 775321899904
# (graph, chains) of tests/test_gpu_gibbs_fields.py
GPU_ROWS = (("random77", 19), ("zephyr128", 5), ("zephyr128", 1025), ("zephyr512", 9), ("zephyr1024", 5), ("zephyr1024", 512))
ROLLED_WAVES = {16: (1, 4), 32: (1, 4), 64: (1, 4, 16)}  # DVG_GIBBS_ROLLED_KERNELS, by lanes per chain
LDS_MAX = 160 * 1024


# ------------------------------------------------------------------------------------------------ the symbol
def test_symbol_is_declared_bound_and_exported():
    name = "dvg_gibbs_sample_fields"
    support.assert_declared_bound_exported(name, markers=["DVG field v1"])
    # the draw's arguments are dvg_gibbs_sample's with (fields, stride) in front of samples_out
    plain, field = _lib.SIGNATURES["dvg_gibbs_sample"][1], _lib.SIGNATURES[name][1]
    assert field == plain[:16] + [ctypes.c_void_p, ctypes.c_int64] + plain[16:]
    # appended: the ids the other kinds had stay theirs
    assert dev.GIBBS_KIND_IDS == dict(plain=0, held=1, table=2, weigh=3, trace=5, field=6)


# ------------------------------------------------------------------------------------------------ the helper is the oracle
def test_field_oracle_is_the_oracle_chain_by_chain():
    """24 spins at p = 0.3, 6 chains, 3 sweeps from sweep 5: the oracle once per chain with that chain's hs and id."""
    n, C, sweeps, sweep0, beta, prefactor = 24, 6, 3, 5, 1.3, 0.7
    rng = np.random.default_rng(24)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.uniform(size=iu.size) < 0.3
    plan = graphs.build_plan(n, iu[keep].astype(np.int64), ju[keep].astype(np.int64))
    h = rng.uniform(-1, 1, n).astype(np.float32)
    J = rng.uniform(-1, 1, plan.n_edges).astype(np.float32)
    fields = rng.standard_normal((C, n)).astype(np.float32)
    ids = np.arange(C, dtype=np.uint32) + 11
    start = gibbs.init_state(ids, n, SEED, sweep0)
    hs = field_oracle.chain_fields(h, fields, prefactor, (-1.0, 1.0))
    assert ((hs == 1.0) | (hs == -1.0)).any() and not ((hs == 1.0) | (hs == -1.0)).all()  # the range clamps some, not all
    got = field_oracle.field_sweeps(start, ids, hs, gibbs.scaled_fields(h, J, prefactor, None, (-0.5, 0.5))[1], beta, plan, SEED, sweep0,
                                    sweeps)
    for c in range(C):
        hs_c, Js = gibbs.scaled_fields((h + fields[c]).astype(np.float32), J, prefactor, (-1.0, 1.0), (-0.5, 0.5))
        assert np.array_equal(hs_c, hs[c])
        want = gibbs.gibbs_sweeps(start[c:c + 1].copy(), ids[c:c + 1], hs_c, Js, beta, plan.order, plan.class_ptr, plan.adj_ptr,
                                  plan.adj_idx, plan.adj_eid, SEED, sweep0, sweeps)
        assert np.array_equal(got[c], want[0]), c
    assert not np.array_equal(got, start)
    # one shared row: (1, n), the same for every chain
    assert np.array_equal(field_oracle.chain_fields(h, fields[0], prefactor, None), ((h + fields[0]) * np.float32(prefactor))[None, :])


# ------------------------------------------------------------------------------------------------ the C entry point's checks
_stand_in = support.graph_stand_in


def _fields(g, lin, quad, state, fields, *, stride=64, n_chains=8, n_sweeps=7, dyn=None):
    L = _lib.lib()
    rc = L.dvg_gibbs_sample_fields(g, lin, quad, 1.0, -1, 1, -1, 1, 1.0, state, n_chains, 0, 0, 0, n_sweeps, 1, fields, stride, None, dyn,
                                   None)
    return rc, L.dvg_last_error()


def test_argument_validation_without_gpu():
    """Everything the header lists is DVG_E_INVALID (-1) with a message, before any HIP call (there is no device here, and
    the pointers are host memory: a launch would not return -1)."""
    rc, msg = _fields(None, None, None, None, None)
    assert rc == -1 and b"null" in msg
    graph, g, p, _keep = _stand_in()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p)):  # what dvg_gibbs_sample rejects
        rc, msg = _fields(g, *args)
        assert rc == -1 and b"null" in msg
    for n_chains in (0, -4):
        rc, msg = _fields(g, p, p, p, p, n_chains=n_chains)
        assert rc == -1 and b"n_chains" in msg
    rc, msg = _fields(g, p, p, p, p, n_sweeps=-1)
    assert rc == -1 and b"n_sweeps" in msg
    rc, msg = _fields(g, p, p, p, None)  # its own
    assert rc == -1 and b"null fields" in msg and b"dvg_gibbs_sample" in msg
    for stride in (1, 63, 65, 128, -64, 2 ** 40):
        rc, msg = _fields(g, p, p, p, p, stride=stride)
        assert rc == -1 and b"field_chain_stride" in msg, stride
    rc, msg = _fields(g, p, p, p, p, dyn=p)
    assert rc == -1 and b"dyn" in msg
    rc, msg = _fields(g, p, p, p, p, stride=0, dyn=p)
    assert rc == -1 and b"dyn" in msg
    ctypes.c_int32.from_buffer(graph).value = 40000
    rc, msg = _fields(g, p, p, p, p, stride=40000)
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
    return (s.sweep_count, s.cond_sweep_count, s.field_sweep_count, s.calls)


def test_sample_fields_rejects_bad_arguments(untouched):
    s, lin, quad = untouched
    n = s.plan.n
    assert s.field_seed == 3 ^ 0x666C6431 and s.field_seed not in (s.seed, s.cond_seed, s.anneal_seed, s.trace_seed)
    call = lambda fields, **kw: s.sample_fields(lin, quad, 1.0, None, None, fields, **kw)  # noqa: E731
    good, row = torch.zeros((4, n)), torch.zeros(n)
    with pytest.raises(_lib.DvgError, match="fields must be a tensor"):
        call(np.zeros((4, n), dtype=np.float32))
    for bad in (good.double(), good.to(torch.int8), good.half()):
        with pytest.raises(_lib.DvgError, match="fields must be float32"):
            call(bad)
    for bad in (torch.zeros((4, n + 1)), torch.zeros((0, n)), torch.zeros((2, 2, n)), torch.zeros(n - 1), torch.zeros(())):
        with pytest.raises(_lib.DvgError, match="fields must be"):
            call(bad)
    with pytest.raises(ValueError, match="start or num_reads"):
        call(row)
    for bad in ([], "4", True, 2.5, 0):
        with pytest.raises(ValueError, match="num_reads"):
            call(row, num_reads=bad)
    with pytest.raises(_lib.DvgError, match="fields has 4 rows but the draw has 5 chains"):
        call(good, num_reads=5)
    for bad in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError, match="sweeps"):
            call(good, sweeps=bad)
    # the one order of the start checks, as in every draw: a tensor, its dtype, its shape, the count, on the GPU
    with pytest.raises(_lib.DvgError, match="start must be a tensor"):
        call(good, start=np.ones((4, n), dtype=np.int8))
    with pytest.raises(_lib.DvgError, match="start must be float32 or int8"):
        call(good, start=torch.ones((4, n), dtype=torch.float64))
    with pytest.raises(_lib.DvgError, match="start must be"):
        call(good, start=torch.ones((4, n + 1), dtype=torch.int8))
    with pytest.raises(_lib.DvgError, match="num_reads=5 but start has 4 chains"):
        call(row, start=torch.ones((4, n), dtype=torch.int8), num_reads=5)
    with pytest.raises(_lib.DvgError, match="start must live on the GPU"):
        call(good, start=torch.ones((4, n), dtype=torch.int8))
    # a CPU tensor of fields is an error: the HIP path has no CPU fallback
    with pytest.raises(_lib.DvgError, match="fields must live on the GPU"):
        call(good)
    with pytest.raises(_lib.DvgError, match="fields must live on the GPU"):
        call(row, num_reads=4)
    assert _counters(s) == (0, 0, 0, 0) and s._state is None


# ------------------------------------------------------------------------------------------------ the plan
@pytest.fixture(scope="module")
def plans():
    return {name: pinned.grid.build_graph(name) for name in sorted({name for name, _c in GPU_ROWS})}


def _n_pad(n):
    return (n + 15) & ~15


def _rolled_lds(plan, chains):
    """gibbs_lds_bytes of csrc/gibbs_plan.h, from the layout it documents: hs [n up to 4] float | couplings [4 (batches + 1)]
    float | row [n] uint32 | classes [colours + 1] int32 | (to 8 bytes) | offsets [4 (batches + 1)] uint16 | order [n up to 2]
    uint16 | state [chains][n_pad] float16; a row of ceil(degree / 4) batches per spin."""
    n = plan.n
    batches = int(((np.diff(np.asarray(plan.adj_ptr)) + 3) // 4).sum())
    b = 4 * ((n + 3) & ~3) + 4 * 4 * (batches + 1) + 4 * n + 4 * (plan.n_colours + 1)
    b = (b + 7) & ~7
    b += 2 * 4 * (batches + 1) + 2 * ((n + 1) & ~1)
    return b + 2 * chains * _n_pad(n)


@pytest.mark.parametrize("name,C", GPU_ROWS)
def test_the_field_kind_is_rolled_with_a_row_of_hs_per_chain(plans, name, C):
    """The rule of the issue, worked out here: the rolled instantiation the table kind takes under gibbs_generic = 1, WAVES
    stepped down within the list until tables + chains x (2 + 4) n_pad bytes fit 160 KiB -- whatever the option."""
    _lib.check(_lib.lib().dvg_reset_options(), "dvg_reset_options")
    plan = plans[name]
    with _lib.option_scope(gibbs_generic=1):
        table = dev.gibbs_draw_plan(plan, C, "table")
    assert table["form"] == "rolled"
    lpc, per_wave = table["params"]["LPC"], 64 // table["params"]["LPC"]
    assert table["lds_bytes"] == _rolled_lds(plan, table["chains_per_workgroup"])  # (the formula above is the layout's)
    fits = [w for w in ROLLED_WAVES[lpc]
            if w <= table["params"]["WAVES"] and _rolled_lds(plan, w * per_wave) + 4 * w * per_wave * _n_pad(plan.n) <= LDS_MAX]
    assert fits, (name, "nothing fits")
    waves = max(fits)
    for option in (0, 1, 2, 3, 4):
        with _lib.option_scope(gibbs_generic=option):
            p = dev.gibbs_draw_plan(plan, C, "field")
        where = (name, C, option, p)
        assert p["form"] == "rolled" and p["params"] == dict(LPC=lpc, WAVES=waves), where
        cpw = p["chains_per_workgroup"]
        assert cpw == waves * per_wave and p["threads"] == 64 * waves and p["workgroups"] == -(-C // cpw), where
        assert p["lds_bytes"] == _rolled_lds(plan, cpw) + 4 * cpw * _n_pad(plan.n), where
        assert p["lds_bytes"] <= LDS_MAX, where


def test_the_large_graph_steps_its_workgroup_down(plans):
    """Zephyr 1024: 124 KB of tables; 16 chains x 6 KiB do not fit beside them, 4 chains do."""
    _lib.check(_lib.lib().dvg_reset_options(), "dvg_reset_options")
    plan = plans["zephyr1024"]
    with _lib.option_scope(gibbs_generic=1):
        assert dev.gibbs_draw_plan(plan, 512, "table")["params"] == dict(LPC=64, WAVES=16)
    assert _rolled_lds(plan, 16) + 4 * 16 * 1024 > LDS_MAX
    for C in (5, 512, 513):
        p = dev.gibbs_draw_plan(plan, C, "field")
        assert p["params"] == dict(LPC=64, WAVES=4) and p["chains_per_workgroup"] == 4 and p["workgroups"] == -(-C // 4), p
    # the small ones keep the workgroup the table kind has
    assert dev.gibbs_draw_plan(plans["random77"], 19, "field")["params"] == dict(LPC=16, WAVES=1)
    assert dev.gibbs_draw_plan(plans["zephyr512"], 9, "field")["params"] == dict(LPC=64, WAVES=4)


def test_the_step_down_reaches_one_wave_and_then_reports():
    """9000 spins without edges: 90 KB of tables; sixteen or four chains of 54 KB do not fit, one does.  11000: not even one --
    DVG_E_UNSUPPORTED with the message the other kinds give."""
    _lib.check(_lib.lib().dvg_reset_options(), "dvg_reset_options")
    g = pinned._synthetic([1500] * 6, 0)
    with pytest.raises(_lib.DvgError, match="> 160 KiB"):  # (a graph of this size takes (64, 16), and the other kinds stay there)
        dev.gibbs_draw_plan(g, 40, "table")
    p = dev.gibbs_draw_plan(g, 40, "field")
    assert p["form"] == "rolled" and p["params"] == dict(LPC=64, WAVES=1) and p["workgroups"] == 40, p
    assert p["lds_bytes"] == _rolled_lds(g, 1) + 4 * _n_pad(9000) <= LDS_MAX < _rolled_lds(g, 4) + 16 * _n_pad(9000)
    with pytest.raises(_lib.DvgError, match=r"needs \d+ B of LDS.*field rows.*> 160 KiB"):
        dev.gibbs_draw_plan(pinned._synthetic([1100] * 10, 0), 40, "field")


def test_the_other_kinds_plans_are_where_they_were(plans):
    """Every row of the pinned table on these graphs (tests/test_gibbs_plan_host.py, imported), with the field kind planned
    in between."""
    _lib.check(_lib.lib().dvg_reset_options(), "dvg_reset_options")
    rows = [(key, want) for key, want in pinned._GIBBS_PLANS.items() if key[0] in plans]
    assert len(rows) >= 4 * (3 + 3 + 12 + 1)
    for (name, c, kind, option), (form, params, workgroups, threads, lds) in rows:
        with _lib.option_scope(gibbs_generic=option):
            dev.gibbs_draw_plan(plans[name], c, "field")
            p = dev.gibbs_draw_plan(plans[name], c, kind)
        assert (p["form"], p["params"], p["workgroups"], p["threads"], p["lds_bytes"]) == (form, params, workgroups, threads, lds), \
            (name, c, kind, option, p)


# ------------------------------------------------------------------------------------------------ logit_fields
def test_logit_fields_against_enumeration_on_two_spins():
    """p(z) prod_i sigmoid(l_i z_i), normalised over the four states, against the model with fields = logit_fields(l)."""
    h, J, prefactor, beta = np.array([0.3, -0.2]), 0.7, 0.5, 1.7
    logits = np.array([1.1, -0.4], dtype=np.float32)
    f = smp.logit_fields(logits, beta, prefactor)
    assert isinstance(f, np.ndarray) and f.dtype == np.float32 and f.shape == (2,)
    np.testing.assert_allclose(f, -logits.astype(np.float64) / (2 * beta * prefactor), rtol=3e-7)
    states = np.array([[a, b] for a in (-1.0, 1.0) for b in (-1.0, 1.0)])
    prior = np.exp(-beta * prefactor * (states @ h + J * states[:, 0] * states[:, 1]))
    want = prior * (1.0 / (1.0 + np.exp(-logits.astype(np.float64)[None, :] * states))).prod(1)
    want /= want.sum()
    got = np.exp(-beta * prefactor * (states @ (h + f.astype(np.float64)) + J * states[:, 0] * states[:, 1]))
    got /= got.sum()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)  # (float32 fields: 6e-8 relative on exponents of order 1)
    assert abs(want - prior / prior.sum()).max() > 0.05  # the evidence moves the law
    # a tensor in, a float32 tensor of the same shape out
    t = smp.logit_fields(torch.tensor([[1.1, -0.4], [0.0, 2.0]], dtype=torch.float64), beta, prefactor)
    assert torch.is_tensor(t) and t.dtype == torch.float32 and t.shape == (2, 2) and t.is_contiguous()
    np.testing.assert_allclose(t[0].numpy(), f, rtol=3e-7)
    assert float(t[1, 0]) == 0.0
    for beta_bad, pre_bad in ((0.0, 1.0), (1.0, 0.0), (float("inf"), 1.0), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            smp.logit_fields(logits, beta_bad, pre_bad)
