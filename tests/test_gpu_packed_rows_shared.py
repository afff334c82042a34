"""GPU checks of what the packed-row entries share (csrc/packed_rows.h) on one input none of the per-entry files has: a ring of
33 spins -- W = 2 words a row with ONE live bit in the last word -- and a (C, M, W) = (5, 13, 2) view cut from a larger
padded tensor of noise: 65 pooled rows, two tiles, the second of one row; every pad bit (bits 1..31 of a row's last word)
and every word around the view is noise.  Energies, local-field statistics and descents are held to their numpy definitions
(``energy_oracle``, ``fields_oracle``, ``descent_oracle``) as in the per-entry files -- exactly wherever a result is exact by
construction, within the helper's bound where two orderings of a float64 sum may differ -- the moments and correlation sums
to the integer sums of the unpacked rows, and the descent's ``unstable`` to the fields entry's count on the descended rows."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descent_oracle as do  # noqa: E402
import energy_oracle as eo  # noqa: E402
import fields_oracle as fo  # noqa: E402
import trace_oracle  # noqa: E402
from image_generation_amd import functional as F, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
N, W, C, M = 33, 2, 5, 13
H_RANGE, J_RANGE = (-4.0, 4.0), (-1.0, 1.0)
PREFACTOR = 0.3  # both clamps active
DYADIC = dict(prefactor=0.5, linear_range=(-1.0, 1.0), quadratic_range=(-0.5, 0.5))


class _Case:
    def __init__(self):
        ei, ej = np.arange(N, dtype=np.int64), (np.arange(N, dtype=np.int64) + 1) % N
        self.plan = plan = graphs.build_plan(N, np.minimum(ei, ej), np.maximum(ei, ej))
        self.gh = smp.GraphHandle(plan, "cuda")
        rng = np.random.default_rng(N)
        self.h = (20.0 * rng.uniform(-1, 1, N)).astype(np.float32)
        self.J = (5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
        self.h_dyadic = (rng.integers(-2048, 2049, N) / 1024.0).astype(np.float32)
        self.J_dyadic = (rng.integers(-2048, 2049, plan.n_edges) / 1024.0).astype(np.float32)
        noise = rng.integers(0, 2 ** 32, size=(C + 2, M + 3, W + 3), dtype=np.uint64).astype(np.uint32)
        self.padded = torch.from_numpy(noise.view(np.int32)).cuda()
        self.view = self.padded[1:1 + C, 2:2 + M, 1:1 + W]  # strides (80, 5, 1) words
        assert tuple(self.view.shape) == (C, M, W) and not self.view.is_contiguous()
        self.host = noise[1:1 + C, 2:2 + M, 1:1 + W].reshape(C * M, W).copy()  # the pooled rows, group by group
        assert ((self.host[:, 1] >> np.uint32(1)) != 0).all()  # the pad bits are set
        self.x = trace_oracle.unpack(self.host, N).astype(np.int64)  # (65, 33) +-1

    def dev(self, h, J):
        return torch.from_numpy(h).cuda(), torch.from_numpy(J).cuda()


@functools.lru_cache(maxsize=None)
def _case():
    return _Case()


def test_energies():
    case, p = _case(), _case().plan
    hs, Js = gibbs.scaled_fields(case.h, case.J, PREFACTOR, H_RANGE, J_RANGE)
    assert (np.abs(hs) == 4.0).any() and (np.abs(Js) == 1.0).any()
    want, A = eo.energies(case.host, N, hs, Js, p.edge_i, p.edge_j)
    got = F.grbm_energy_packed(case.view, case.gh, *case.dev(case.h, case.J), prefactor=PREFACTOR, linear_range=H_RANGE,
                               quadratic_range=J_RANGE)
    assert got.shape == (C, M) and got.dtype == torch.float64
    err, bound = np.abs(got.cpu().numpy().ravel() - want), eo.bound(N, p.n_edges, A)
    print(f"ring33 energies: |E| up to {np.abs(want).max():.4g}, worst error {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all() and np.abs(want).max() > 1e3 * bound
    # dyadic fields: every partial sum is exact whatever the order -- the helper's energies bit for bit
    hs, Js = gibbs.scaled_fields(case.h_dyadic, case.J_dyadic, DYADIC["prefactor"], DYADIC["linear_range"], DYADIC["quadratic_range"])
    assert np.array_equal(hs * 2048, np.round(hs * 2048)) and np.array_equal(Js * 2048, np.round(Js * 2048)) and (np.abs(Js) == 0.5).any()
    want, _A = eo.energies(case.host, N, hs, Js, p.edge_i, p.edge_j)
    got = F.grbm_energy_packed(case.view, case.gh, *case.dev(case.h_dyadic, case.J_dyadic), **DYADIC)
    assert np.array_equal(got.cpu().numpy().ravel(), want) and len(np.unique(want)) > 32


def test_fields():
    case, p = _case(), _case().plan
    hs, Js = gibbs.scaled_fields(case.h, case.J, PREFACTOR, H_RANGE, J_RANGE)
    ei, ej = np.asarray(p.edge_i), np.asarray(p.edge_j)
    for beta in (0.0, 0.4):
        o = fo.fields(case.host, N, hs, Js, p.edge_i, p.edge_j, beta)
        got = F.grbm_fields_packed(case.view, case.gh, *case.dev(case.h, case.J), beta=beta, prefactor=PREFACTOR, linear_range=H_RANGE,
                                   quadratic_range=J_RANGE, fields=True)
        assert got.fields.shape == (C, M, N) and got.log_pl.shape == got.unstable.shape == (C, M)
        assert np.array_equal(got.fields.cpu().numpy().reshape(C * M, N), o.f), "fields differ from the sampler's field"
        assert np.array_equal(got.unstable.cpu().numpy().ravel(), o.unstable) and o.unstable.max() > 0
        sd = o.s.astype(np.float64)
        ratios = dict(
            log_pl=(np.abs(got.log_pl.cpu().numpy().ravel() - o.log_pl) / fo.bound_log_pl(N, o.S)).max(),
            cond_sum=np.abs(got.cond_sum.cpu().numpy() - fo.pooled(o.m)).max() / fo.bound_cond_sum(C * M),
            cond_pair=np.abs(got.cond_pair.cpu().numpy() - fo.pooled(o.m[:, ei] * sd[:, ej] + o.m[:, ej] * sd[:, ei])).max()
            / fo.bound_cond_pair(C * M))
        print(f"FIELDS-RATIO ring33 beta={beta}: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(ratios.items())))
        assert all(v <= 1.0 for v in ratios.values()), ratios
        assert o.S.min() > 0.0 and (beta == 0 or np.abs(o.m).max() > 0.5)


def test_descents_and_their_unstable_counts():
    case, p = _case(), _case().plan
    hs, Js = gibbs.scaled_fields(case.h, case.J, PREFACTOR, H_RANGE, J_RANGE)
    lin, quad = case.dev(case.h, case.J)
    kw = dict(prefactor=PREFACTOR, linear_range=H_RANGE, quadratic_range=J_RANGE)
    before = case.padded.clone()
    for cap in (1, 2, 64):
        want = do.descend(case.host, N, hs, Js, p.edge_i, p.edge_j, p.order, p.class_ptr, cap)
        got = F.grbm_descend_packed(case.view, case.gh, lin, quad, max_sweeps=cap, **kw)
        assert got.bits.shape == (C, M, W) and got.bits.is_contiguous() and got.sweeps.shape == (C, M)
        assert np.array_equal(got.bits.cpu().numpy().view(np.uint32).reshape(C * M, W), want.bits)  # (pad bits 0)
        for k in ("sweeps", "flips", "unstable"):
            assert np.array_equal(getattr(got, k).cpu().numpy().ravel(), getattr(want, k)), (cap, k)
        f = F.grbm_fields_packed(got.bits, case.gh, lin, quad, beta=1.0, log_pl=False, conditional=False, **kw)
        assert torch.equal(f.unstable, got.unstable), cap
        # (teeth: one sweep leaves unstable spins; two cut rows off that still moved, with the counting pass finding none)
        assert bool(want.unstable.any()) == (cap == 1) and want.sweeps.max() == min(cap, 2)
    assert torch.equal(case.padded, before)  # the input and the words around it are left alone


def test_moments_and_correlation_sums():
    case, p = _case(), _case().plan
    x = case.x
    spin, pair = F.grbm_moments_packed(case.view.reshape(C * M, W).contiguous(), case.gh)
    assert np.array_equal(spin.cpu().numpy(), x.sum(axis=0))
    assert np.array_equal(pair.cpu().numpy(), (x[:, np.asarray(p.edge_i)] * x[:, np.asarray(p.edge_j)]).sum(axis=0))
    spin, full = F.packed_correlation(case.view, n=N)
    assert np.array_equal(spin.cpu().numpy(), x.sum(axis=0)) and np.array_equal(full.cpu().numpy(), x.T @ x)
    assert (np.diag(x.T @ x) == C * M).all() and np.abs(x.sum(axis=0)).max() < C * M
