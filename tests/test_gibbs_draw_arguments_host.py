"""CPU-side checks of the one argument path the seven one-off Gibbs draws share (``GibbsSampler._check_start``, ``_whole``,
``_parameters`` in sampler.py): the same bad ``start`` is the same error in every draw that takes one, the checks of
``start`` come in one order, every count argument is the documented ``ValueError`` whatever it is handed -- all before the
library is touched and with every counter left where it was."""
import numpy as np
import pytest
import torch

import support
from image_generation_amd import _lib, sampler as smp

N, R = 12, 3
LADDER = [0.1, 1.0, 2.0]  # R rungs
SCHEDULE = [0.5, 1.0, 2.0]


@pytest.fixture
def untouched(monkeypatch):
    """A sampler on a 12-spin ring, with the library out of reach: any call into it fails the test.  The parameters are
    CPU tensors, so a call whose other arguments pass ends at them, still before the library."""
    support.out_of_reach(monkeypatch)
    plan = support.ring_plan(N)
    s = smp.GibbsSampler(plan, list(range(N)), beta=2.0, sweeps=5, seed=3, device="cuda")
    return s, torch.zeros(N), torch.zeros(plan.n_edges)


def _rungs(start):
    return torch.zeros(np.shape(start)[0] if np.ndim(start) else 0, dtype=torch.int32)


class Draw:
    """One draw: ``call(s, lin, quad, **kw)`` with ``base`` filled in; ``with_start(start)``: the keywords that hand it a start
    state (None: the draw takes none); ``chains``: the count argument a start is held against and how many chains one of it
    is; ``counts``: its count arguments; ``burn_in``: whether it records."""

    def __init__(self, method, head, base, with_start=None, chains=None, counts=(), burn_in=False):
        self.method, self.head, self.base, self.with_start, self.chains, self.counts, self.burn_in = (method, head, base, with_start,
                                                                                                      chains, counts, burn_in)

    def call(self, untouched, **kw):
        s, lin, quad = untouched
        kw = {**self.base, **kw}
        positional = [kw.pop(name) for name in self.head]
        return getattr(s, self.method)(lin, quad, 1.0, None, None, *positional, **kw)


_tempered_start = lambda start: dict(start=start, rungs=_rungs(start))  # noqa: E731
DRAWS = {
    "conditional": Draw("sample_conditional", ("start", "clamp"),
                        dict(start=torch.ones((4, N), dtype=torch.int8), clamp=torch.zeros(N, dtype=torch.bool)),
                        with_start=lambda start: dict(start=start)),
    "annealed": Draw("sample_annealed", ("betas",), dict(betas=SCHEDULE), with_start=lambda start: dict(start=start),
                     chains=("num_reads", 1), counts=("num_reads",)),
    "ais": Draw("sample_ais", ("betas",), dict(betas=SCHEDULE), with_start=lambda start: dict(start=start, beta_from=0.5),
                chains=("num_reads", 1), counts=("num_reads",)),
    "population": Draw("sample_population", ("betas",), dict(betas=SCHEDULE, num_reads=4),
                       counts=("num_reads", "num_populations", "sweeps_per_beta")),
    "tempered": Draw("sample_tempered", ("betas",), dict(betas=LADDER, num_ladders=2), with_start=_tempered_start,
                     chains=("num_ladders", R), counts=("num_ladders", "num_sweeps", "swap_every")),
    "tempered_trace": Draw("sample_tempered_trace", ("betas",), dict(betas=LADDER, num_ladders=2), with_start=_tempered_start,
                           chains=("num_ladders", R), counts=("num_ladders", "num_sweeps", "swap_every", "thin"), burn_in=True),
    "trace": Draw("sample_trace", (), dict(), with_start=lambda start: dict(start=start), chains=("num_reads", 1),
                  counts=("num_reads", "num_sweeps", "thin"), burn_in=True),
}
WITH_START = [name for name, d in DRAWS.items() if d.with_start]
C = 2 * R  # chains of a good start: two ladders of the exchange draws
BAD_STARTS = {
    "numpy array": np.ones((C, N), dtype=np.int8),
    "float64": torch.ones((C, N), dtype=torch.float64),
    "(C, n + 1)": torch.ones((C, N + 1), dtype=torch.int8),
    "1-D": torch.ones((N,), dtype=torch.int8),
    "zero rows": torch.ones((0, N), dtype=torch.int8),
    "CPU tensor": torch.ones((C, N), dtype=torch.int8),
}


def _counters(s):
    return (s.sweep_count, s.cond_sweep_count, s.anneal_sweep_count, s.ais_sweep_count, s.pt_sweep_count, s.trace_sweep_count,
            s.pa_sweep_count, s.calls)


@pytest.mark.parametrize("bad", list(BAD_STARTS))
@pytest.mark.parametrize("name", WITH_START)
def test_the_same_bad_start_is_the_same_error_in_every_draw(untouched, name, bad):
    draw = DRAWS[name]
    with pytest.raises(_lib.DvgError, match="start"):
        draw.call(untouched, **draw.with_start(BAD_STARTS[bad]))
    assert _counters(untouched[0]) == (0,) * 8 and untouched[0]._state is None


@pytest.mark.parametrize("name", [name for name in WITH_START if DRAWS[name].chains])
def test_the_chain_count_is_checked_before_the_device(untouched, name):
    """A start on the CPU that also has another chain count than the call names: the count is reported (the one order)."""
    draw = DRAWS[name]
    count_name, per = draw.chains
    with pytest.raises(_lib.DvgError, match=rf"{count_name}={C // per + 1} but start has {C} chains"):
        draw.call(untouched, **draw.with_start(BAD_STARTS["CPU tensor"]), **{count_name: C // per + 1})
    with pytest.raises(_lib.DvgError, match="start must live on the GPU"):
        draw.call(untouched, **draw.with_start(BAD_STARTS["CPU tensor"]), **{count_name: C // per})
    assert _counters(untouched[0]) == (0,) * 8


@pytest.mark.parametrize("name", list(DRAWS))
def test_every_count_argument_is_a_value_error(untouched, name):
    draw = DRAWS[name]
    for count_name in draw.counts:
        for bad in ([], "4", True, 2.5, 0):
            with pytest.raises(ValueError, match=count_name):
                draw.call(untouched, **{count_name: bad})
    if draw.burn_in:
        for bad in (-1, 0.5, True, None):
            with pytest.raises(ValueError, match="burn_in"):
                draw.call(untouched, burn_in=bad)
    # good arguments end at the CPU parameters (the conditional draw, which has no fresh chains, at its CPU start)
    with pytest.raises(_lib.DvgError, match=("start" if name == "conditional" else "linear") + " must live on the GPU"):
        draw.call(untouched, **({"num_reads": 4} if draw.chains == ("num_reads", 1) else {}))
    assert _counters(untouched[0]) == (0,) * 8 and untouched[0]._state is None
