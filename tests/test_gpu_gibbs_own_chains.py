"""GPU check of the chains a one-off draw makes its own (``GibbsSampler._own_chains``): every draw that takes ``start`` -- the
conditional, annealed, AIS, exchange, traced exchange and traced draws -- copies it into a contiguous int8 buffer of the
call's.  On a ring of 33 spins (two words a packed row, one live bit in the second) the same start state, once as a contiguous
int8 tensor and once as every other column of a float32 buffer twice as wide, gives the same bytes in every output, leaves
the caller's buffers as they were and never touches the persistent chains."""
import functools

import numpy as np
import pytest
import torch

from image_generation_amd import graphs, sampler as smp

pytestmark = pytest.mark.gpu
N, SWEEPS, SEED = 33, 4, 20251
H_RANGE, J_RANGE, PREFACTOR = (-4.0, 4.0), (-1.0, 1.0), 0.3
LADDER = [0.5, 1.0, 2.0]  # the exchange draws: 2 ladders x 3 rungs
SCHEDULE = [0.5, 1.0, 1.5, 2.0]


@functools.lru_cache(maxsize=None)
def _model():
    ei, ej = np.arange(N, dtype=np.int64), (np.arange(N, dtype=np.int64) + 1) % N
    plan = graphs.build_plan(N, np.minimum(ei, ej), np.maximum(ei, ej))
    rng = np.random.default_rng(N)
    h = torch.from_numpy((20.0 * rng.uniform(-1, 1, N)).astype(np.float32)).cuda()
    J = torch.from_numpy((5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)).cuda()
    return plan, h, J


def _draw(name, s, h, J, start):
    """The draw's outputs by name, from ``start`` (C, n)."""
    model, C = (h, J, PREFACTOR, H_RANGE, J_RANGE), int(start.shape[0])
    rungs = (torch.arange(C, dtype=torch.int32, device="cuda") % len(LADDER)).flip(0).contiguous()
    kept = rungs.clone()
    if name == "conditional":
        clamp = (torch.arange(N, device="cuda") % 3 == 0)
        out = dict(samples=s.sample_conditional(*model, start, clamp, init_free=False))
    elif name == "annealed":
        out = dict(samples=s.sample_annealed(*model, SCHEDULE, start=start))
    elif name == "ais":
        samples, log_w, energy = s.sample_ais(*model, SCHEDULE, start=start, beta_from=0.25)
        out = dict(samples=samples, log_weights=log_w, energies=energy)
    elif name == "tempered":
        r = s.sample_tempered(*model, LADDER, num_ladders=C // len(LADDER), start=start, rungs=rungs)
        out = dict(samples=r.samples, energies=r.energies, accepted=r.accepted, state=r.state, rungs=r.rungs)
    elif name == "tempered_trace":
        r = s.sample_tempered_trace(*model, LADDER, num_ladders=C // len(LADDER), thin=2, start=start, rungs=rungs)
        out = dict(bits=r.bits, energies=r.energies, walk=r.walk, samples=r.final.samples, final_energies=r.final.energies,
                   accepted=r.final.accepted, state=r.final.state, rungs=r.final.rungs)
    else:
        r = s.sample_trace(*model, start=start, thin=2)
        out = dict(bits=r.bits, samples=r.samples, state=r.state)
    assert torch.equal(rungs, kept)
    return out


@pytest.mark.parametrize("name,C", [("conditional", 5), ("annealed", 5), ("ais", 5), ("tempered", 6), ("tempered_trace", 6),
                                    ("trace", 5)])
def test_a_strided_float32_start_is_the_contiguous_int8_one(name, C):
    plan, h, J = _model()
    rng = np.random.default_rng(C)
    spins = torch.from_numpy((2 * rng.integers(0, 2, (C, N)) - 1).astype(np.int8)).cuda()
    wide = torch.full((C, 2 * N), 7.0, dtype=torch.float32, device="cuda")  # (the odd columns: never a spin)
    wide[:, ::2] = spins.to(torch.float32)
    view = wide[:, ::2]
    assert not view.is_contiguous() and spins.is_contiguous()
    kept_spins, kept_wide = spins.clone(), wide.clone()
    results = []
    for start in (spins, view):
        s = smp.GibbsSampler(plan, list(range(N)), beta=1.0, sweeps=SWEEPS, seed=SEED, device="cuda")
        results.append(_draw(name, s, h, J, start))
        assert s._state is None and s.sweep_count == 0 and s.calls == 0
    torch.cuda.synchronize()
    assert torch.equal(spins, kept_spins) and torch.equal(wide, kept_wide)
    a, b = results
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert a[key].contiguous().cpu().numpy().tobytes() == b[key].contiguous().cpu().numpy().tobytes(), (name, key)
    # the draw moved the chains: the state it returns is not the start it was handed
    assert not torch.equal(a["samples"].reshape(C, N), spins.to(torch.float32))
