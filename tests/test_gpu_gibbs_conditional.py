"""GPU parity of the conditional block-Gibbs draw (``dvg_gibbs_sample_clamped``: some spins of a chain held, the others
redrawn) against the oracle, bit for bit, and of the Python surface built on it.

The oracle is the existing one, unchanged: a held spin is a spin left out of its colour class, so ``cref.gibbs_sweeps``
called with the held spins filtered out of ``order`` / ``class_ptr`` (empty classes kept) IS the conditional draw.

Dispatch each shape takes (gibbs_generic = 0; asserted against the draw's plan, dev.gibbs_draw_plan, beside the bits):
Pegasus 64 -- the lane-major form, one-wave workgroups, one row per step; Zephyr 128 -- the same in four-wave workgroups
(its tables are beyond the one-wave rule's 16 KiB); Zephyr / Pegasus 512 -- lane-major, four waves, two rows side by side (gibbs_generic = 2: one at a time); Zephyr
1024 x 41 -- lane-major, four waves, 20 rows; Zephyr 1024 x 530 -- the rolled kernel in 16-wave workgroups (the plain draw
runs its chains-side-by-side kernel there); the 77-spin random graph -- no lane image: rolled, one wave; the clique graph
-- lane-major, one row per step, 14 rows.  gibbs_generic = 1 is the rolled kernel everywhere."""
import functools
import os

import numpy as np
import pytest
import torch

import support
from image_generation_amd import _lib, dev, graphs, sampler as smp
from oracle import cref, gibbs

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ graphs
_solver_plan = functools.partial(support.solver_plan, with_nodes=True)


# as in test_gpu_gibbs.py: degrees beyond 20, spin 3 isolated
_random_plan = functools.partial(support.random_plan, isolated=3, max_degree_above=20)


_clique_plan = support.clique_plan


def _takes(plan, C, kind, form, **params):
    """The draw's plan under the current options names this kernel form (and these template parameters of it)."""
    p = dev.gibbs_draw_plan(plan, C, kind)
    assert p["form"] == form and all(p["params"][k] == v for k, v in params.items()), p


# the form the module docstring claims for a solver graph's conditional draw: (n, more than 512 chains, gibbs_generic)
def _solver_form(n, C, generic):
    if n == 1024 and (generic == 1 or C > 512):
        return "rolled", dict(LPC=64, WAVES=16)
    if generic == 1:
        return "rolled", {}
    if n <= 128:
        return "lane", dict(LPC=32, WAVES=1 if n == 64 else 4, NR=1, MAXS=12)
    return "lane", dict(LPC=64, WAVES=4, NR=1 if generic == 2 else 2, MAXS=20 if n == 1024 else 12)


# ------------------------------------------------------------------------------------------------ the oracle
def _filtered_classes(plan, held_row):
    """(order, class_ptr) with the held spins taken out of every class, classes in their original order, empty ones kept."""
    order, ptr = [], [0]
    for k in range(plan.n_colours):
        cls = np.asarray(plan.order[plan.class_ptr[k]:plan.class_ptr[k + 1]])
        order.extend(int(i) for i in cls if not held_row[i])
        ptr.append(len(order))
    return np.asarray(order, dtype=np.int32), np.asarray(ptr, dtype=np.int32)


def _oracle(state, ids, mask, hs, Js, beta, plan, seed, sweep0, sweeps):
    """The conditional draw: per distinct mask row, cref.gibbs_sweeps with the filtered class lists on the chains that share
    the row, under their own chain ids.  ``mask``: (C, n) bool."""
    out = np.array(state, dtype=np.int8, copy=True)
    rows, inv = np.unique(mask, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    for r in range(rows.shape[0]):
        sel = np.flatnonzero(inv == r)
        order, ptr = _filtered_classes(plan, rows[r])
        out[sel] = cref.gibbs_sweeps(out[sel], ids[sel], hs, Js, beta, order, ptr, plan.adj_ptr, plan.adj_idx, plan.adj_eid,
                                     seed, sweep0, sweeps)
    return out


# ------------------------------------------------------------------------------------------------ the raw ABI
class _Draw:
    """dvg_gibbs_sample_clamped / dvg_gibbs_sample on one graph and one (h, J)."""

    def __init__(self, plan, h, J, prefactor, beta):
        self.plan, self.prefactor, self.beta = plan, float(prefactor), float(beta)
        self.gh = smp.GraphHandle(plan, "cuda")
        self.lin, self.quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()

    def _args(self, state, id0, seed, sweep0, sweeps, init):
        return (self.gh.ptr, self.lin.data_ptr(), self.quad.data_ptr(), self.prefactor, -4.0, 4.0, -1.0, 1.0, self.beta,
                state.data_ptr(), int(state.shape[0]), id0, seed, sweep0, sweeps, init)

    def clamped(self, state, clamp, id0, seed, sweep0, sweeps, init):
        """``state`` (C, n) int8 device tensor, updated in place; ``clamp`` uint8 device tensor, (C, n) or (n,)."""
        out = torch.full(tuple(state.shape), 7.0, dtype=torch.float32, device="cuda")
        stride = self.plan.n if clamp.dim() == 2 else 0
        _lib.check(_lib.lib().dvg_gibbs_sample_clamped(*self._args(state, id0, seed, sweep0, sweeps, init), clamp.data_ptr(),
                                                       stride, out.data_ptr(), None, _lib.stream_ptr()),
                   "dvg_gibbs_sample_clamped")
        return out

    def plain(self, state, id0, seed, sweep0, sweeps, init):
        out = torch.full(tuple(state.shape), 7.0, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().dvg_gibbs_sample(*self._args(state, id0, seed, sweep0, sweeps, init), out.data_ptr(), None,
                                               _lib.stream_ptr()), "dvg_gibbs_sample")
        return out


def _params(plan, rng, h_scale, j_scale):
    h = (h_scale * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (j_scale * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    return h, J


def _masks(plan, C, rng):
    """Per-chain masks random at 50 %; chain 0: one whole colour class held, chain 1: everything, chain 2: nothing."""
    mask = rng.uniform(size=(C, plan.n)) < 0.5
    mask[0] = False
    mask[0, np.asarray(plan.order[plan.class_ptr[0]:plan.class_ptr[1]])] = True
    mask[1] = True
    mask[2] = False
    return mask


def _bit_exact(plan, C, sweeps, *, h_scale, j_scale, prefactor, beta, id0, shared=False):
    n = plan.n
    rng = np.random.default_rng(n + C)
    h, J = _params(plan, rng, h_scale, j_scale)
    hs, Js = gibbs.scaled_fields(h, J, prefactor, (-4, 4), (-1, 1))
    ids = np.arange(C, dtype=np.uint32) + id0
    mask = np.broadcast_to(rng.uniform(size=n) < 0.5, (C, n)).copy() if shared else _masks(plan, C, rng)
    prepared = np.where(rng.uniform(size=(C, n)) < 0.5, -1, 1).astype(np.int8)
    # init = 1 on the first call: free spins from the INIT stream, held ones from the prepared state
    want = np.where(mask, prepared, cref.init_state(ids, n, SEED))
    d = _Draw(plan, h, J, prefactor, beta)
    state = torch.from_numpy(prepared).cuda()
    clamp = torch.from_numpy(np.ascontiguousarray(mask[0] if shared else mask).astype(np.uint8)).cuda()
    for call in range(3):  # persistent chains over three draws, the sweep index running on
        out = d.clamped(state, clamp, id0, SEED, call * sweeps, sweeps, 1 if call == 0 else 0)
        want = _oracle(want, ids, mask, hs, Js, beta, plan, SEED, call * sweeps, sweeps)
        got, got_state = out.cpu().numpy(), state.cpu().numpy()
        assert set(np.unique(got).tolist()) <= {-1.0, 1.0}
        mism = int((got != want.astype(np.float32)).sum())
        assert mism == 0, f"{mism} spin mismatches in samples_out at call {call}"
        assert int((got_state != want).sum()) == 0, f"state differs from the oracle at call {call}"
        assert np.array_equal(got_state[mask], prepared[mask]), f"held spins moved at call {call}"


SOLVER_CASES = [
    # fam, n, C, sweeps, gibbs_generic, shared mask
    ("pegasus", 64, 37, 3, 0, False), ("pegasus", 64, 37, 3, 1, False),
    ("zephyr", 128, 256, 5, 0, False), ("zephyr", 128, 256, 5, 1, False), ("zephyr", 128, 256, 5, 0, True),
    ("zephyr", 512, 70, 6, 0, False), ("zephyr", 512, 70, 6, 2, False), ("zephyr", 512, 70, 6, 0, True),
    ("pegasus", 512, 256, 5, 0, False), ("pegasus", 512, 256, 5, 2, False), ("pegasus", 512, 256, 5, 0, True),
    ("zephyr", 1024, 41, 5, 0, False),
    ("zephyr", 1024, 530, 5, 0, False), ("zephyr", 1024, 530, 5, 1, False),
]


@pytest.mark.parametrize("fam,n,C,sweeps,generic,shared", SOLVER_CASES)
def test_conditional_bit_exact(fam, n, C, sweeps, generic, shared):
    plan, _nodes = _solver_plan(fam, n)
    with _lib.option_scope(gibbs_generic=generic):
        form, params = _solver_form(n, C, generic)
        _takes(plan, C, "held", form, **params)
        _bit_exact(plan, C, sweeps, h_scale=0.05, j_scale=5.0, prefactor=0.05, beta=20.0, id0=1000, shared=shared)


@pytest.mark.parametrize("generic", [0, 1, 2])
def test_conditional_bit_exact_on_arbitrary_graph(generic):
    """77 spins at p = 0.35: degrees beyond 20 (two rounds of the neighbour sum), an isolated spin, an odd spin count."""
    with _lib.option_scope(gibbs_generic=generic):
        _takes(_random_plan(77, 0.35), 19, "held", "rolled", LPC=16, WAVES=1)  # (no lane image)
        _bit_exact(_random_plan(77, 0.35), 19, 6, h_scale=0.5, j_scale=2.0, prefactor=0.3, beta=1.5, id0=7)


@pytest.mark.parametrize("generic", [0, 1])
def test_conditional_bit_exact_many_small_classes(generic):
    """50 disjoint 14-cliques: the lane-major schedule's one-row form at more than 12 rows."""
    with _lib.option_scope(gibbs_generic=generic):
        if generic == 0:
            _takes(_clique_plan(), 21, "held", "lane", LPC=64, WAVES=4, NR=1, MAXS=20)
            assert dev.gibbs_draw_plan(_clique_plan(), 21, "held")["lane_image"]["rows"] == 14
        else:
            _takes(_clique_plan(), 21, "held", "rolled")
        _bit_exact(_clique_plan(), 21, 5, h_scale=0.5, j_scale=1.0, prefactor=0.4, beta=1.2, id0=3)


# ------------------------------------------------------------------------------------------------ nothing / everything held
@pytest.mark.parametrize("n,C", [(128, 256), (1024, 530)])
@pytest.mark.parametrize("init", [0, 1])
def test_nothing_held_is_the_plain_draw(n, C, init):
    """An all-zero mask gives the bits of dvg_gibbs_sample from the same state, seed and sweep index (1024 x 530: the plain
    draw runs the chains-side-by-side kernel, the conditional one the rolled kernel)."""
    plan, _nodes = _solver_plan("zephyr", n)
    if n == 1024:
        _takes(plan, C, "plain", "slots", CH=16)
        _takes(plan, C, "held", "rolled", LPC=64, WAVES=16)
    rng = np.random.default_rng(n)
    h, J = _params(plan, rng, 0.05, 5.0)
    d = _Draw(plan, h, J, 0.05, 20.0)
    start = torch.from_numpy(np.where(rng.uniform(size=(C, n)) < 0.5, -1, 1).astype(np.int8)).cuda()
    s_plain, s_cond = start.clone(), start.clone()
    want = d.plain(s_plain, 11, SEED, 3, 5, init)  # (sweeps 3..7: starts off the multiples of four)
    for clamp in (torch.zeros((C, n), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")):
        s_cond.copy_(start)
        got = d.clamped(s_cond, clamp, 11, SEED, 3, 5, init)
        assert torch.equal(got, want) and torch.equal(s_cond, s_plain)
    assert not torch.equal(s_plain, start)


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("init", [0, 1])
def test_everything_held_returns_the_input(generic, init):
    plan, _nodes = _solver_plan("zephyr", 128)
    rng = np.random.default_rng(5)
    h, J = _params(plan, rng, 0.05, 5.0)
    d = _Draw(plan, h, J, 0.05, 20.0)
    C, n = 37, plan.n
    start = torch.from_numpy(np.where(rng.uniform(size=(C, n)) < 0.5, -1, 1).astype(np.int8)).cuda()
    with _lib.option_scope(gibbs_generic=generic):
        for clamp in (torch.ones((C, n), dtype=torch.uint8, device="cuda"), torch.full((n,), 255, dtype=torch.uint8, device="cuda")):
            state = start.clone()
            out = d.clamped(state, clamp, 0, SEED, 0, 4, init)
            assert torch.equal(state, start) and torch.equal(out, start.float())


# ------------------------------------------------------------------------------------------------ the conditional law
def test_conditional_law_against_exact_enumeration():
    """12 spins, 4 of them held: the free spins' means and all their pair correlations over 4096 chains after 40 sweeps
    against the exact conditional distribution (the 256 free configurations enumerated in float64).  Bound: five standard
    errors of a +-1 mean over 4096 chains, 5 / sqrt(4096) = 0.078, on both.  (The CPU oracle with these inputs is off by
    0.015 on the means and 0.029 on the correlations, and the kernel is bit-exact to it.)"""
    n, C, beta = 12, 4096, 0.8
    rng = np.random.default_rng(12)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.uniform(size=iu.size) < 0.4
    ei, ej = iu[keep].astype(np.int64), ju[keep].astype(np.int64)
    plan = graphs.build_plan(n, ei, ej)
    h = (0.5 * rng.uniform(-1, 1, n)).astype(np.float32)
    J = (1.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    hs, Js = gibbs.scaled_fields(h, J, 1.0, (-4, 4), (-1, 1))
    held = np.array([1, 4, 7, 10]); held_val = np.array([1, -1, -1, 1], dtype=np.int8)
    free = np.array([i for i in range(n) if i not in set(held.tolist())])

    ids = np.arange(C, dtype=np.uint32)
    start = cref.init_state(ids, n, SEED)
    start[:, held] = held_val
    mask = np.zeros(n, dtype=np.uint8); mask[held] = 1
    d = _Draw(plan, h, J, 1.0, beta)
    state = torch.from_numpy(start).cuda()
    got = d.clamped(state, torch.from_numpy(mask).cuda(), 0, SEED, 0, 40, 0).cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:, held], np.broadcast_to(held_val.astype(np.float64), (C, 4)))

    # exact: p(s_free | s_held) ~ exp(-beta (hs.s + sum_e Js_e s_i s_j)) over the 256 free configurations
    conf = np.empty((256, n), dtype=np.float64)
    conf[:, held] = held_val
    conf[:, free] = 1.0 - 2.0 * ((np.arange(256)[:, None] >> np.arange(8)[None, :]) & 1)
    pe_i, pe_j = np.asarray(plan.edge_i), np.asarray(plan.edge_j)
    energy = conf @ hs.astype(np.float64) + (conf[:, pe_i] * conf[:, pe_j]) @ Js.astype(np.float64)
    p = np.exp(-beta * (energy - energy.min())); p /= p.sum()
    mean_exact = p @ conf[:, free]
    corr_exact = np.einsum("c,ci,cj->ij", p, conf[:, free], conf[:, free])
    mean_got = got[:, free].mean(0)
    corr_got = got[:, free].T @ got[:, free] / C
    err_mean = float(np.abs(mean_got - mean_exact).max())
    err_corr = float(np.abs(corr_got - corr_exact).max())
    print(f"conditional law: max |mean error| {err_mean:.4f}, max |correlation error| {err_corr:.4f}")
    bound = 5.0 / np.sqrt(C)
    assert err_mean <= bound and err_corr <= bound, (err_mean, err_corr, bound)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_sampler_surface_leaves_the_training_stream_alone():
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    plan, nodes = _solver_plan("zephyr", 128)
    rng = np.random.default_rng(2)
    h, J = _params(plan, rng, 0.05, 5.0)
    lin, quad = torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()
    C, n = 24, plan.n
    mk = lambda: smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=4, seed=SEED, persistent=True, chain_offset=5,  # noqa: E731
                                  h_range=(-4, 4), j_range=(-1, 1))
    start = torch.from_numpy(np.where(rng.uniform(size=(9, n)) < 0.5, -1.0, 1.0).astype(np.float32)).cuda()
    clamp = torch.from_numpy(rng.uniform(size=(9, n)) < 0.5).cuda()

    ref = mk()
    ref_draws = [ref.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone() for _ in range(2)]

    s = mk()
    assert s.cond_seed == SEED ^ 0x636F6E64 and s.cond_sweep_count == 0
    first = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C).clone()
    state_before, sweeps_before, calls_before = s._state.clone(), s.sweep_count, s.calls
    state_ptr = s._state.data_ptr()
    out = s.sample_conditional(lin, quad, 0.05, (-4, 4), (-1, 1), start, clamp, sweeps=3)
    assert out.shape == (9, n) and out.dtype == torch.float32 and out.is_cuda
    assert torch.equal(out[clamp], start[clamp]) and set(out.unique().tolist()) <= {-1.0, 1.0}
    assert s._state.data_ptr() == state_ptr and torch.equal(s._state, state_before)
    assert (s.sweep_count, s.calls, s.cond_sweep_count) == (sweeps_before, calls_before, 3)
    second = s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)
    assert torch.equal(first, ref_draws[0]) and torch.equal(second, ref_draws[1])

    # bit-exact against the oracle under the conditional key, chain ids chain_offset + arange, sweeps 0..2
    hs, Js = gibbs.scaled_fields(h, J, 0.05, (-4, 4), (-1, 1))
    ids = np.arange(9, dtype=np.uint32) + 5
    m = clamp.cpu().numpy()
    want = np.where(m, start.cpu().numpy().astype(np.int8), cref.init_state(ids, n, s.cond_seed))
    want = _oracle(want, ids, m, hs, Js, 20.0, plan, s.cond_seed, 0, 3)
    assert np.array_equal(out.cpu().numpy(), want.astype(np.float32))

    # int8 start, uint8 (n,) mask, the sampler's own sweep count; a CPU tensor is an error
    out2 = s.sample_conditional(lin, quad, 0.05, (-4, 4), (-1, 1), start.to(torch.int8), clamp[0].to(torch.uint8), init_free=False)
    assert s.cond_sweep_count == 3 + 4 and torch.equal(out2[:, clamp[0]], start[:, clamp[0]])
    with pytest.raises(_lib.DvgError):
        s.sample_conditional(lin, quad, 0.05, (-4, 4), (-1, 1), start, clamp.cpu())
    with pytest.raises(_lib.DvgError):
        s.sample_conditional(lin, quad, 0.05, (-4, 4), (-1, 1), start.cpu(), clamp)

    # GRBM.sample_conditional is the sampler call
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                            np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    a, b = mk(), mk()
    via_grbm = grbm.sample_conditional(a, start, clamp, prefactor=0.05, linear_range=(-4, 4), quadratic_range=(-1, 1), sweeps=3)
    direct = b.sample_conditional(grbm._linear, grbm._quadratic, 0.05, (-4, 4), (-1, 1), start, clamp, sweeps=3, init_free=True)
    assert torch.equal(via_grbm, direct)
    with pytest.raises(TypeError):
        grbm.sample_conditional(object(), start, clamp, prefactor=0.05)


def test_generate_variations():
    from image_generation_amd import functional as F
    from image_generation_amd.data import synthetic_images
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()  # fresh-init parameters
    n, B, V = 64, 4, 3
    images = synthetic_images(B, seed=3, device="cuda").reshape(B, 1, 32, 32)
    out, spins, mask = m.generate_variations(images, n_variations=V, keep=0.5, return_latents=True)
    assert out.shape == (B, V, 1, 32, 32) and spins.shape == (B * V, n) and mask.shape == (B, n)
    assert mask.dtype == torch.bool and (mask.sum(1) == 32).all()
    with torch.no_grad():
        encoded = F.heaviside_latent_to_discrete(m._dvae.encoder(images)).squeeze(1)
    rep_enc, rep_mask = encoded.repeat_interleave(V, 0), mask.repeat_interleave(V, 0)
    assert torch.equal(spins[rep_mask], rep_enc[rep_mask])
    assert set(spins.unique().tolist()) <= {-1.0, 1.0}
    assert not torch.equal(spins, rep_enc)  # 96 free spins per image redrawn from the prior: some moved
    with torch.no_grad():
        decoded = m._dvae.decoder(spins.unsqueeze(1)).squeeze(1).clip(0.0, 1.0)
    assert torch.equal(out.reshape(B * V, 1, 32, 32), decoded)
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0

    # the same mask_seed gives the same mask, another one another
    _o, _s, mask_again = m.generate_variations(images, n_variations=V, keep=0.5, return_latents=True)
    _o, _s, mask_other = m.generate_variations(images, n_variations=V, keep=0.5, mask_seed=1, return_latents=True)
    assert torch.equal(mask_again, mask) and not torch.equal(mask_other, mask)

    # keep = 1: exactly the encoded spins
    _o, spins_all, mask_all = m.generate_variations(images, n_variations=V, keep=1.0, return_latents=True)
    assert bool(mask_all.all()) and torch.equal(spins_all, rep_enc)

    # keep = 0: the mask all false, and the spins of a conditional draw with nothing held
    at = m.sampler.cond_sweep_count
    _o, spins_none, mask_none = m.generate_variations(images, n_variations=V, keep=0.0, return_latents=True)
    assert not bool(mask_none.any())
    m.sampler.cond_sweep_count = at
    want = m.sampler.sample_conditional(m._grbm._linear, m._grbm._quadratic, m.PREFACTOR, m.linear_range, m.quadratic_range,
                                        rep_enc, torch.zeros((B * V, n), dtype=torch.bool, device="cuda"))
    assert torch.equal(spins_none, want)

    # sharpening as generate_images does it
    sharp = m.generate_variations(images, n_variations=V, keep=1.0, sharpen=True, lower=0.3, upper=0.7)
    plain = m.generate_variations(images, n_variations=V, keep=1.0)
    over, under = (plain > 0.7).float(), (plain > 0.3).float()
    assert torch.equal(sharp, (over + (1 - over) * plain) * under)
