"""GPU check that the two chain-per-lanes forms of the Gibbs kernels -- lane-major (``gibbs_fast_kernel``, the default where
the graph has a lane image) and rolled (``gibbs_kernel``, option ``gibbs_generic=1``) -- run the same draw: every tensor a
draw returns is the same bytes under both, for each of the seven draw modes the kernels carry (csrc/gibbs.hip, "the sweep
loop's control").

Two graphs.  A ring of 33 spins: odd, three colour classes, fewer than 64 lanes per chain, so a wave holds several chains and
the exchange draw's workgroup has idle slots.  A ring of 200 spins: two classes of 100, 64 lanes per chain and two rows of a
class side by side (``gibbs_generic=2`` walks them one at a time: a third form); its state rows are 208 halfwords and
208 % 32 == 16, the record step's mid-word case.

The parameters make every float64 output exact, so that the sums do not depend on which lane added what: h and J are
multiples of 1/16 (J nonzero) under prefactor 1 and the ranges (-1.5, 1.5), (-0.75, 0.75) -- both clamps bite, the clamped
values stay sixteenths -- and every beta is a multiple of 1/8.  Then every local field is exact in float32, every energy
addend is a multiple of 1/32 and every log-weight addend a multiple of 1/256, far inside 53 bits."""
import functools

import numpy as np
import pytest
import torch

from image_generation_amd import _lib, dev, graphs, sampler as smp

pytestmark = pytest.mark.gpu
SWEEPS, SWAP_EVERY, BURN_IN, THIN = 6, 2, 1, 2
# a seed under which each of the file's four exchange draws accepts an exchange (tests/tempered_oracle.py tells: the 200-ring's
# three ladders, a factor two in beta apart, go without one in six sweeps under most seeds)
SEED = 77012
SWEEP0 = 5  # (not a multiple of four: the draws start inside a Philox counter's four words)
H_RANGE, J_RANGE, PREFACTOR, BETA = (-1.5, 1.5), (-0.75, 0.75), 1.0, 1.0
SCHEDULE = [0.25, 0.5, 1.0, 1.5, 2.0, 2.0]
LADDER = [0.5, 1.0, 2.0]
CHAINS, LADDERS = 7, 3  # (seven chains: the last workgroup is partly filled)
DRAWS = ("native", "conditional", "annealed", "ais", "tempered", "tempered_trace", "trace")
# the forms beside the default one: (option gibbs_generic, form, rows of a class side by side or None)
GRAPHS = {33: ((1, "rolled", None),), 200: ((1, "rolled", None), (2, "lane", 1))}


@functools.lru_cache(maxsize=None)
def _model(n):
    ei, ej = np.arange(n, dtype=np.int64), (np.arange(n, dtype=np.int64) + 1) % n
    plan = graphs.build_plan(n, np.minimum(ei, ej), np.maximum(ei, ej))
    rng = np.random.default_rng(n)
    h = rng.integers(-32, 33, n).astype(np.float32) / 16.0
    J = (rng.integers(1, 17, plan.n_edges) * rng.choice([-1, 1], plan.n_edges)).astype(np.float32) / 16.0
    assert (np.abs(h) > H_RANGE[1]).any() and (np.abs(J) > J_RANGE[1]).any() and (J != 0).all()
    start = torch.from_numpy((2 * rng.integers(0, 2, (LADDERS * len(LADDER), n)) - 1).astype(np.int8)).cuda()
    return plan, torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda(), start


def _draw(name, n):
    """The draw's outputs by name, as host bytes, under the options in force."""
    plan, h, J, start = _model(n)
    model = (h, J, PREFACTOR, H_RANGE, J_RANGE)
    s = smp.GibbsSampler(plan, list(range(n)), beta=BETA, sweeps=SWEEPS, seed=SEED, device="cuda")
    for counter in ("sweep_count", "cond_sweep_count", "anneal_sweep_count", "ais_sweep_count", "pt_sweep_count", "trace_sweep_count"):
        setattr(s, counter, SWEEP0)
    rungs = (torch.arange(start.shape[0], dtype=torch.int32, device="cuda") % len(LADDER)).flip(0).contiguous()
    if name == "native":  # (fresh chains, then the same chains again)
        first = s.sample_native(*model, num_reads=CHAINS)
        out = dict(first=first, second=s.sample_native(*model, num_reads=CHAINS), state=s._state)
    elif name == "conditional":
        out = dict(samples=s.sample_conditional(*model, start[:CHAINS], torch.arange(n, device="cuda") % 3 == 0))
    elif name == "annealed":
        out = dict(samples=s.sample_annealed(*model, SCHEDULE, num_reads=CHAINS))
    elif name == "ais":
        samples, log_w, energy = s.sample_ais(*model, SCHEDULE, start=start[:CHAINS], beta_from=0.25)
        out = dict(samples=samples, log_weights=log_w, energies=energy)
    elif name == "tempered":
        r = s.sample_tempered(*model, LADDER, num_ladders=LADDERS, swap_every=SWAP_EVERY)
        out = dict(samples=r.samples, energies=r.energies, accepted=r.accepted, state=r.state, rungs=r.rungs)
    elif name == "tempered_trace":
        r = s.sample_tempered_trace(*model, LADDER, num_ladders=LADDERS, swap_every=SWAP_EVERY, burn_in=BURN_IN, thin=THIN,
                                    start=start, rungs=rungs)
        out = dict(bits=r.bits, energies=r.energies, walk=r.walk, samples=r.final.samples, final_energies=r.final.energies,
                   accepted=r.final.accepted, state=r.final.state, rungs=r.final.rungs)
    else:
        r = s.sample_trace(*model, start=start[:CHAINS], burn_in=BURN_IN, thin=THIN)
        out = dict(bits=r.bits, samples=r.samples, state=r.state)
    torch.cuda.synchronize()
    return {k: (str(v.dtype), tuple(v.shape), v.contiguous().cpu().numpy().tobytes()) for k, v in out.items()}, out


@pytest.mark.parametrize("n", sorted(GRAPHS))
def test_the_options_take_the_forms(n):
    plan = _model(n)[0]
    assert int(plan.n_colours) == (3 if n % 2 else 2)

    def plans():
        ps = [dev.gibbs_draw_plan(plan, CHAINS, kind) for kind in ("plain", "held", "table", "weigh", "trace")]
        return ps + [dev.gibbs_exchange_plan(plan, LADDERS, len(LADDER))]

    for p in plans():
        assert p["form"] == "lane" and p["params"]["LPC"] == (16 if n == 33 else 64) and p["params"]["NR"] == (1 if n == 33 else 2), p
    for generic, form, nr in GRAPHS[n]:
        with _lib.option_scope(gibbs_generic=generic):
            for p in plans():
                assert p["form"] == form and (nr is None or p["params"]["NR"] == nr), (generic, p)
    # the exchange draw's workgroups have slots that idle (on the 200-ring a whole wave), the others' last one is partly filled
    p = dev.gibbs_exchange_plan(plan, LADDERS, len(LADDER))
    assert p["chains_per_workgroup"] % len(LADDER) != 0, p
    assert CHAINS % dev.gibbs_draw_plan(plan, CHAINS)["chains_per_workgroup"] != 0


@pytest.mark.parametrize("name", DRAWS)
@pytest.mark.parametrize("n", sorted(GRAPHS))
def test_every_form_returns_the_same_bytes(n, name):
    want, tensors = _draw(name, n)
    if "accepted" in tensors:
        assert int(tensors["accepted"].sum()) >= 1  # the exchange block decided, not only met
    if "bits" in tensors:
        assert int((tensors["bits"][..., -1] != 0).sum()) >= 1  # the record's last word: its live bits, mid-word on the 200-ring
    for generic, _form, _nr in GRAPHS[n]:
        with _lib.option_scope(gibbs_generic=generic):
            got, _ = _draw(name, n)
        assert got.keys() == want.keys()
        for key in want:
            assert got[key][:2] == want[key][:2], (generic, key)
            assert got[key][2] == want[key][2], (generic, name, key)
