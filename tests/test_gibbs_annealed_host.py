"""CPU-side checks of the annealed block-Gibbs draw (``dvg_gibbs_sample_annealed``, include/dvg.h): the schedule
builder, the symbol, and every argument error of the Python surface -- raised before the library is touched."""
import ctypes

import numpy as np
import pytest
import torch

import support
from image_generation_amd import _lib, sampler as smp

NAME = "dvg_gibbs_sample_annealed"


# ------------------------------------------------------------------------------------------------ beta_schedule
@pytest.mark.parametrize("kind", ["geometric", "linear"])
@pytest.mark.parametrize("b0,b1,S", [(0.05, 20.0, 7), (0.1, 3.0, 9), (20.0, 0.3, 5), (0.7, 0.7, 4), (0.1, 1.0 / 3.0, 2)])
def test_beta_schedule_endpoints_monotonicity_dtype(kind, b0, b1, S):
    b = smp.beta_schedule(b0, b1, S, kind)
    assert isinstance(b, np.ndarray) and b.dtype == np.float32 and b.shape == (S,)
    assert b[0] == np.float32(b0) and b[-1] == np.float32(b1)
    d = np.diff(b.astype(np.float64))
    assert (d >= 0).all() if b1 >= b0 else (d <= 0).all()
    want = (np.geomspace(b0, b1, S) if kind == "geometric" else np.linspace(b0, b1, S)).astype(np.float32)
    assert np.array_equal(b[1:-1], want[1:-1])  # float64 points, rounded once
    if kind == "geometric" and S > 2 and b0 != b1:  # constant ratio, constant step
        r = b[1:].astype(np.float64) / b[:-1]
        assert np.allclose(r, r[0], rtol=1e-6)
    if kind == "linear" and S > 2:
        assert np.allclose(d, d[0], rtol=1e-5, atol=1e-7)


def test_beta_schedule_default_is_geometric_and_one_sweep_is_the_target():
    assert np.array_equal(smp.beta_schedule(0.05, 20.0, 7), smp.beta_schedule(0.05, 20.0, 7, "geometric"))
    for kind in ("geometric", "linear"):
        one = smp.beta_schedule(0.5, 3.0, 1, kind)
        assert one.dtype == np.float32 and one.tolist() == [3.0]
    assert smp.beta_schedule(0.0, 2.0, 5, "linear")[0] == 0.0  # a linear schedule may start at beta = 0


@pytest.mark.parametrize("args", [(0.0, 1.0, 4, "geometric"), (1.0, 0.0, 4, "geometric"), (0.0, 1.0, 1, "geometric"),
                                  (-0.1, 1.0, 4, "linear"), (0.1, float("inf"), 4, "linear"), (0.1, float("nan"), 4, "geometric"),
                                  (0.1, 1.0, 0, "geometric"), (0.1, 1.0, -3, "linear"), (0.1, 1.0, 2.5, "linear"),
                                  (0.1, 1.0, 4, "cosine")])
def test_beta_schedule_rejects(args):
    with pytest.raises(ValueError):
        smp.beta_schedule(*args)


# ------------------------------------------------------------------------------------------------ the symbol and its checks
def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported(NAME)


def _call(g, lin, quad, state, betas, stride, n_sweeps, n_chains=4):
    L = _lib.lib()
    rc = L.dvg_gibbs_sample_annealed(g, lin, quad, 1.0, -1, 1, -1, 1, betas, stride, state, n_chains, 0, 0, 0, n_sweeps, 1,
                                     None, None, None)
    return rc, L.dvg_last_error()


def test_argument_validation_without_gpu():
    """Null pointers, a null table, a chain stride that is neither 0 nor n_sweeps and a draw of no sweeps are
    DVG_E_INVALID (-1) with a message, before any HIP call (safe on a CPU-only box)."""
    rc, msg = _call(None, None, None, None, None, 0, 3)
    assert rc == -1 and b"null" in msg
    # as in test_gibbs_conditional_host.py: a host-memory stand-in for the graph handle (first field: the spin count);
    # the other pointers are never dereferenced on the host
    graph = ctypes.create_string_buffer(4096)
    ctypes.c_int32.from_buffer(graph).value = 64
    g = ctypes.cast(graph, ctypes.c_void_p)
    dummy = ctypes.create_string_buffer(16)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    rc, msg = _call(g, p, p, p, None, 0, 3)
    assert rc == -1 and b"betas" in msg
    for stride in (3, 1, 6, 8, 14, -7, 64):
        rc, msg = _call(g, p, p, p, p, stride, 7)
        assert rc == -1 and b"beta_chain_stride" in msg, (stride, rc, msg)
    for n_sweeps in (0, -1):
        rc, msg = _call(g, p, p, p, p, 0, n_sweeps)
        assert rc == -1 and b"n_sweeps" in msg
    rc, msg = _call(g, p, p, p, p, 0, 3, n_chains=0)
    assert rc == -1 and b"n_chains" in msg


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture
def untouched(monkeypatch):
    """A sampler on a 12-spin ring, with the library out of reach: any call into it fails the test."""
    support.out_of_reach(monkeypatch)
    plan = support.ring_plan()
    n = plan.n
    s = smp.GibbsSampler(plan, list(range(n)), beta=2.0, sweeps=5, seed=3, device="cuda")
    lin, quad = torch.zeros(n), torch.zeros(plan.n_edges)
    return s, lin, quad


BAD_TABLES = [
    ([0.1, -0.5, 1.0], ValueError), ([0.1, float("nan")], ValueError), ([0.1, float("inf")], ValueError),
    (np.array([1e39, 1.0]), ValueError),  # finite in float64, not in float32
    (torch.tensor([0.5, -1.0]), ValueError), ([], _lib.DvgError), (np.zeros((2, 0)), _lib.DvgError),
    (np.ones((2, 2, 2)), _lib.DvgError), (3.0, _lib.DvgError), (["a", "b"], ValueError),
]


@pytest.mark.parametrize("betas,exc", BAD_TABLES)
def test_sample_annealed_rejects_bad_tables(untouched, betas, exc):
    s, lin, quad = untouched
    with pytest.raises(exc):
        s.sample_annealed(lin, quad, 1.0, None, None, betas, num_reads=4)
    assert s.anneal_sweep_count == 0


def test_sample_annealed_rejects_bad_shapes_and_starts(untouched):
    s, lin, quad = untouched
    n, ok = s.plan.n, [0.1, 1.0, 2.0]
    call = lambda betas, **kw: s.sample_annealed(lin, quad, 1.0, None, None, betas, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="num_reads"):
        call(ok)  # how many chains?
    with pytest.raises(_lib.DvgError, match="betas"):
        call(np.ones((3, 5)), num_reads=4)  # a row per chain, but three rows
    for bad in (0, -2, 2.5, True):
        with pytest.raises(ValueError, match="num_reads"):
            call(ok, num_reads=bad)
    with pytest.raises(_lib.DvgError, match="GPU"):
        call(ok, start=torch.ones((4, n), dtype=torch.int8))  # a CPU start state
    with pytest.raises(_lib.DvgError, match="float32 or int8"):
        call(ok, start=torch.ones((4, n), dtype=torch.float64))
    with pytest.raises(_lib.DvgError, match="start must be"):
        call(ok, start=torch.ones((4, n + 1)))
    with pytest.raises(_lib.DvgError, match="start must be"):
        call(ok, start=torch.ones(n))
    with pytest.raises(_lib.DvgError):
        call(ok, start=np.ones((4, n), dtype=np.int8))
    with pytest.raises(_lib.DvgError):  # valid table, CPU parameters: the HIP path has no CPU fallback
        call(ok, num_reads=4)
    assert (s.anneal_sweep_count, s.sweep_count, s.calls, s.cond_sweep_count) == (0, 0, 0, 0)


@pytest.mark.parametrize("betas,exc", BAD_TABLES + [(np.ones((4, 3)), _lib.DvgError)])
def test_set_beta_schedule_rejects(untouched, betas, exc):
    s, _lin, _quad = untouched
    with pytest.raises(exc):
        s.set_beta_schedule(betas)
    assert s._betas is None and s.sweeps == 5
    s.set_beta_schedule(None)  # nothing set: nothing to restore
    assert s._betas is None and s.sweeps == 5


def test_annealed_draws_have_their_own_key_and_counter(untouched):
    s, _lin, _quad = untouched
    assert s.anneal_seed == 3 ^ 0x616E6E6C and s.anneal_seed != s.cond_seed and s.anneal_sweep_count == 0
    s.anneal_sweep_count, s.sweep_count, s.cond_sweep_count = 5, 6, 7
    s.reset()
    assert (s.anneal_sweep_count, s.sweep_count, s.cond_sweep_count) == (0, 0, 0)


@pytest.mark.parametrize("kwargs,exc", [
    (dict(beta_range=(0.1, 3.0), beta_schedule=[0.1, 1.0]), ValueError),
    (dict(num_sweeps=9), ValueError),  # a sweep count without a range
    (dict(beta_range=(0.0, 3.0), num_sweeps=9), ValueError),  # geometric from zero
    (dict(beta_range=(0.1, 3.0), num_sweeps=0), ValueError),
    (dict(beta_range=(0.1, float("nan"))), ValueError),
    (dict(beta_range=(0.1, -3.0), beta_schedule_type="linear"), ValueError),
    (dict(beta_range=0.5), ValueError),
    (dict(beta_range=(0.1, 1.0, 2.0)), ValueError),
    (dict(beta_range=(0.1, 3.0), beta_schedule_type="custom"), ValueError),
    (dict(beta_range=(0.1, 3.0), beta_schedule_type="cosine"), ValueError),
    (dict(beta_schedule=[0.1, 1.0], beta_schedule_type="cosine"), ValueError),
    (dict(beta_schedule=[0.1, -1.0]), ValueError),
    (dict(beta_schedule=[0.1, float("inf")]), ValueError),
    (dict(beta_schedule=[0.1, 1.0], num_sweeps=3), ValueError),
    (dict(beta_schedule=np.ones((3, 5))), _lib.DvgError),  # eight reads, three rows
    (dict(beta_schedule=[]), _lib.DvgError),
    (dict(beta_range=(0.1, 3.0), num_reads=0), ValueError),
])
def test_sample_ising_rejects_bad_annealing_arguments(untouched, kwargs, exc):
    s, _lin, _quad = untouched
    h = {v: 0.1 for v in s.nodes}
    J = {(int(a), int(b)): -0.2 for a, b in zip(s.plan.edge_i, s.plan.edge_j)}
    kw = dict(num_reads=8)
    kw.update(kwargs)
    with pytest.raises(exc):
        s.sample_ising(h, J, **kw)
    assert (s.anneal_sweep_count, s.sweep_count, s.calls) == (0, 0, 0)
