"""GPU checks of ``dvg_grbm_fields_packed`` ("DVG fields v1") -- local fields, pseudo-log-likelihoods, unstable-spin counts
and Rao-Blackwellised moment sums of bit-packed rows -- against the numpy definition (``tests/fields_oracle.py``).

Exact outputs: ``field_out`` equals the helper's float32 values (the sampler's field, bit for bit), ``unstable`` equals it.
Bounds, u = 2^-53, every one computed from the helper's values: |log_pl - ref| <= (2 n + 16) u S_r with S_r = sum_i nlp_ri (two
orderings of n positive addends, and twice the budget of an exp and a log1p good to 2 ulp each); |cond_sum_i - ref| <= 10 T u
and |cond_pair_e - ref| <= 20 T u (|m| <= 1 with an absolute error of at most 8 u, and 2 T u per unit addend for the orderings).
Each test prints the largest error / bound ratio it saw (profiles/gibbs_fields.txt keeps them).

Rows: traced draws' records and rows of random words whose bits of spins >= n are set at random and must be ignored; 1, 35, 63,
64, 65, 287 = 41 x 7 of them on ``pegasus64`` (two whole words a row), ``random77`` (a partial last word, spin 3 isolated) and
``zephyr1024``; prefactor 0.05 (clamps idle) and 0.3 (both active); beta 0.5, 1.5 and 0."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_oracle as fo  # noqa: E402
import trace_oracle  # noqa: E402
import support  # noqa: E402
from image_generation_amd import _lib, functional as F, graphs, sampler as smp  # noqa: E402
from oracle import gibbs  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 775321899904
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, IGUARD = -1234.56789, -77
ROWS = [1, 35, 63, 64, 65, 287]
GRAPHS = ["pegasus64", "random77", "zephyr1024"]
H_RANGE, J_RANGE = (-4.0, 4.0), (-1.0, 1.0)
PREFACTORS, BETAS = (0.05, 0.3), (0.5, 1.5, 0.0)
OUT = ("log_pl", "unstable", "cond_sum", "cond_pair", "field_out")
U = fo.U


_solver_plan = functools.partial(support.solver_plan, with_nodes=True)


_random_plan = functools.partial(support.random_plan, isolated=3)


@functools.lru_cache(maxsize=None)
def _grid_plan(a=8, b=9):
    idx = np.arange(a * b).reshape(a, b)
    ei = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]).astype(np.int64)
    ej = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()]).astype(np.int64)
    return graphs.build_plan(a * b, ei, ej)


class _Case:
    """The graph, its handle, 287 rows of each kind on the device -- a traced draw of 41 chains x 7 records, and random words
    -- and ``generic`` float32 fields whose clamps are active at prefactor 0.3 and idle at 0.05.  Built once per graph; the
    references are computed once per (kind, prefactor, beta) over all 287 rows (``want``), the tests take the first ``rows``."""

    def __init__(self, name, plan=None):
        self.name = name
        self.plan = plan = plan or {"pegasus64": lambda: _solver_plan("pegasus", 64)[0], "random77": _random_plan,
                                    "zephyr1024": lambda: _solver_plan("zephyr", 1024)[0]}[name]()
        rng = np.random.default_rng(plan.n)
        self.h = (20.0 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
        self.J = (5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
        self.lin, self.quad = torch.from_numpy(self.h).cuda(), torch.from_numpy(self.J).cuda()
        self.gh = gh = smp.GraphHandle(plan, "cuda")
        C, S, self.W = 41, 7, (plan.n + 31) // 32
        state = torch.empty((C, plan.n), dtype=torch.int8, device="cuda")
        traced = torch.empty((C * S, self.W), dtype=torch.int32, device="cuda")
        # (the draw: prefactor 0.3, both clamps active, beta 20 -- cold chains, 1000 sweeps before the 7 records)
        _lib.check(_lib.lib().dvg_gibbs_sample_traced(gh.ptr, self.lin.data_ptr(), self.quad.data_ptr(), 0.3, -4.0, 4.0, -1.0, 1.0,
                                                      20.0, state.data_ptr(), C, 1000, SEED, 6, 1000 + S, 1, None, traced.data_ptr(), 1000,
                                                      1, None, _lib.stream_ptr()), "dvg_gibbs_sample_traced")
        torch.cuda.synchronize()
        noise = rng.integers(0, 2 ** 32, size=(C * S, self.W), dtype=np.uint64).astype(np.uint32)
        if plan.n % 32:
            assert (noise[:, -1] >> np.uint32(plan.n % 32)).any()  # bits of spins >= n are set
        self.rows = {"trace": traced, "noise": torch.from_numpy(noise.view(np.int32)).cuda()}
        self.host = {k: v.cpu().numpy().view(np.uint32) for k, v in self.rows.items()}
        self.pad_noise = rng.integers(0, 2 ** 32, size=(C * S, 3), dtype=np.uint64).astype(np.uint32)

    @functools.lru_cache(maxsize=None)
    def scaled(self, prefactor):
        return gibbs.scaled_fields(self.h, self.J, prefactor, H_RANGE, J_RANGE)

    @functools.lru_cache(maxsize=None)
    def want(self, kind, prefactor, beta):
        hs, Js = self.scaled(prefactor)
        return fo.fields(self.host[kind], self.plan.n, hs, Js, self.plan.edge_i, self.plan.edge_j, beta)


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


class _Got:
    pass


def _run(case, bits, rows, row_stride, groups, group_stride, prefactor, beta, which=OUT, *, accumulate=0, into=None, lin=None,
         quad=None, null=None, ws_short=False, expect=0):
    """The C entry on device pointers with a guard element behind every output; returns the outputs as numpy (guards
    checked).  ``which``: the outputs asked for; ``into``: (cond_sum, cond_pair) device tensors (with their guards) to use."""
    n, E, T = case.plan.n, case.plan.n_edges, rows * groups
    dev = {}
    if "log_pl" in which:
        dev["log_pl"] = torch.full((T + 1,), GUARD, dtype=torch.float64, device="cuda")
    if "unstable" in which:
        dev["unstable"] = torch.full((T + 1,), IGUARD, dtype=torch.int32, device="cuda")
    if "cond_sum" in which:
        dev["cond_sum"] = into[0] if into else torch.full((n + 1,), GUARD, dtype=torch.float64, device="cuda")
    if "cond_pair" in which:
        dev["cond_pair"] = into[1] if into else torch.full((E + 1,), GUARD, dtype=torch.float64, device="cuda")
    if "field_out" in which:
        dev["field_out"] = torch.full((T * n + 1,), GUARD, dtype=torch.float32, device="cuda")
    L = _lib.lib()
    need = L.dvg_grbm_fields_packed_workspace_bytes(case.gh.ptr, rows, groups)
    ws = torch.full((need // 8 + 3,), GUARD, dtype=torch.float64, device="cuda")
    before = {k: v.clone() for k, v in dev.items()}
    ptr = dict(g=case.gh.ptr, linear=(lin if lin is not None else case.lin).data_ptr(),
               quadratic=(quad if quad is not None else case.quad).data_ptr(), bits=bits.data_ptr())
    if null is not None:
        ptr[null] = None
    rc = L.dvg_grbm_fields_packed(ptr["g"], ptr["linear"], ptr["quadratic"], prefactor, H_RANGE[0], H_RANGE[1], J_RANGE[0],
                                  J_RANGE[1], beta, ptr["bits"], rows, row_stride, groups, group_stride,
                                  *[_lib.ptr(dev.get(k)) for k in OUT], accumulate, ws.data_ptr(), (need - 8) if ws_short else need,
                                  _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.dvg_last_error())
    assert (ws[need // 8:] == GUARD).all(), "written past the workspace"
    got = _Got()
    got.dev = dev
    if rc != 0:
        for k, v in dev.items():
            assert torch.equal(v, before[k]), f"a rejected call wrote {k}"
        return got
    size = dict(log_pl=T, unstable=T, cond_sum=n, cond_pair=E, field_out=T * n)
    for k in OUT:
        a = dev[k].cpu().numpy() if k in dev else None
        if a is not None:
            assert a[size[k]] == (IGUARD if k == "unstable" else np.float32(GUARD) if k == "field_out" else GUARD), f"written past {k}"
            a = a[:size[k]]
        setattr(got, k, a)
    if got.field_out is not None:
        got.field_out = got.field_out.reshape(T, n)
    return got


def _ratios(case, got, o, sel):
    """The largest error / bound ratios of the outputs in ``got`` against the helper's rows ``sel`` (an index array)."""
    n, T = case.plan.n, len(sel)
    ei, ej = np.asarray(case.plan.edge_i), np.asarray(case.plan.edge_j)
    res = {}
    if got.field_out is not None:
        assert got.field_out.dtype == np.float32 and np.array_equal(got.field_out, o.f[sel]), "field_out differs from the sampler's field"
    if got.unstable is not None:
        assert np.array_equal(got.unstable, o.unstable[sel])
    if got.log_pl is not None:
        assert np.isfinite(got.log_pl).all()
        res["log_pl"] = float((np.abs(got.log_pl - o.log_pl[sel]) / fo.bound_log_pl(n, o.S[sel])).max())
    if got.cond_sum is not None:
        m, sd = o.m[sel], o.s[sel].astype(np.float64)
        res["cond_sum"] = float(np.abs(got.cond_sum - fo.pooled(m)).max() / fo.bound_cond_sum(T))
        if len(ei):
            ref = fo.pooled(m[:, ei] * sd[:, ej] + m[:, ej] * sd[:, ei])
            res["cond_pair"] = float(np.abs(got.cond_pair - ref).max() / fo.bound_cond_pair(T))
    return res


def _worst(into, res):
    for k, v in res.items():
        into[k] = max(into.get(k, 0.0), v)


# ------------------------------------------------------------------------------------------------ 1. exact outputs and the bounds
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", GRAPHS)
def test_outputs_against_the_definition(name, rows):
    case = _case(name)
    worst, sel = {}, np.arange(rows)
    for prefactor in PREFACTORS:
        hs, Js = case.scaled(prefactor)
        active = bool((np.abs(hs) == 4.0).any() and (np.abs(Js) == 1.0).any())
        assert active == (prefactor == 0.3)  # the clamps bite at 0.3 and are idle at 0.05
        for beta in BETAS:
            for kind in ("trace", "noise"):
                o = case.want(kind, prefactor, beta)
                got = _run(case, case.rows[kind][:rows].contiguous(), rows, case.W, 1, 0, prefactor, beta)
                _worst(worst, _ratios(case, got, o, sel))
                if beta > 0:
                    assert np.abs(o.m).max() > 0.5 and o.S[sel].min() > 0.0  # (teeth: there is something to compare)
    print(f"FIELDS-RATIO {name} rows={rows}: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------ 2. identities
@pytest.mark.parametrize("name", GRAPHS)
def test_fields_give_the_energy(name):
    """sum_i s_i (hs_i + f_i) / 2 = E: every coupling is met from both ends.  f is a float32 sum of deg + 1 terms, so the
    two differ by float32 field rounding, at most (n + n_edges) 2^-23 A with A = sum |hs| + sum |Js|."""
    case = _case(name)
    n, E = case.plan.n, case.plan.n_edges
    for prefactor in PREFACTORS:
        hs, Js = case.scaled(prefactor)
        A = float(np.abs(hs.astype(np.float64)).sum() + np.abs(Js.astype(np.float64)).sum())
        for kind in ("trace", "noise"):
            got = _run(case, case.rows[kind], 287, case.W, 1, 0, prefactor, 1.5, ("field_out",))
            s = trace_oracle.unpack(case.host[kind], n).astype(np.float64)
            mine = (s * (hs.astype(np.float64)[None, :] + got.field_out.astype(np.float64))).sum(axis=1) / 2.0
            energy = F.grbm_energy_packed(case.rows[kind], case.gh, case.lin, case.quad, prefactor=prefactor, linear_range=H_RANGE,
                                          quadratic_range=J_RANGE).cpu().numpy()
            err = np.abs(mine - energy).max()
            print(f"{name} {kind} prefactor {prefactor}: |E| up to {np.abs(energy).max():.4g}, off by {err:.3e}, bound {(n + E) * 2.0 ** -23 * A:.3e}")
            assert err <= (n + E) * 2.0 ** -23 * A and np.abs(energy).max() > 10 * (n + E) * 2.0 ** -23 * A


def test_flipping_an_isolated_spin_changes_only_its_own_term():
    case = _case("random77")
    bits = case.rows["noise"][:65].contiguous()
    flipped = bits.clone()
    flipped[:, 0] ^= 8  # spin 3
    hs, _Js = case.scaled(0.05)
    a, b = (_run(case, x, 65, case.W, 1, 0, 0.05, 1.5) for x in (bits, flipped))
    assert np.array_equal(a.field_out, b.field_out) and (a.field_out[:, 3] == hs[3]).all() and hs[3] != 0
    assert np.array_equal(a.cond_sum, b.cond_sum) and np.array_equal(a.cond_pair, b.cond_pair)  # m does not depend on s_i itself
    assert (np.abs(a.unstable - b.unstable) == 1).all()  # f_3 = hs_3 != 0: one of the two orientations is unstable
    z = np.float64(np.float32(np.float32(3.0) * hs[3]))
    s3 = trace_oracle.unpack(case.host["noise"][:65], 77)[:, 3].astype(np.float64)
    sp = lambda x: np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))  # noqa: E731
    want = -(sp(-s3 * z) - sp(s3 * z))  # log_pl(flipped) - log_pl: the change of spin 3's own nlp
    o = case.want("noise", 0.05, 1.5)
    assert (np.abs((b.log_pl - a.log_pl) - want) <= 2.0 * fo.bound_log_pl(77, o.S[:65] + abs(z))).all() and np.abs(want).min() > 1e-3


@pytest.mark.parametrize("name", GRAPHS)
def test_beta_zero(name):
    """z = 0 for every spin: nlp = log 2, m = 0.  log_pl lies within n u (relative: one ordering of n equal addends, each
    partial sum rounded once) of -n log 2, and every pooled sum is exactly 0."""
    case = _case(name)
    n = case.plan.n
    for kind in ("trace", "noise"):
        got = _run(case, case.rows[kind], 287, case.W, 1, 0, 0.3, 0.0)
        assert (np.abs(got.log_pl + n * np.log(2.0)) <= n * U * n * np.log(2.0)).all()
        assert (got.cond_sum == 0).all() and (got.cond_pair == 0).all()
        assert (got.unstable > 0).any()  # (stability does not depend on beta)


def test_aligned_states_of_a_ferromagnetic_grid():
    """An 8 x 9 grid with J = -1 (aligned neighbours lower the energy).  h = 0: all up and all down are local minima.  h = 2.5:
    all down is one; all up has f_i = 2.5 - deg_i > 0 at the 4 corners (deg 2) only, whose flip lowers the energy."""
    plan = _grid_plan()
    case = _Case("grid72", plan)
    W = case.W
    up = trace_oracle.pack(np.ones((1, plan.n), np.int8))
    bits = torch.from_numpy(np.concatenate([up, np.zeros_like(up)]).view(np.int32)).cuda()
    J = torch.full((plan.n_edges,), -1.0, device="cuda")
    for h, want in ((0.0, [0, 0]), (2.5, [4, 0]), (-2.5, [0, 4]), (3.5, [4 + 2 * 6 + 2 * 7, 0])):
        got = _run(case, bits, 2, W, 1, 0, 1.0, 1.0, ("unstable", "field_out"), lin=torch.full((plan.n,), h, device="cuda"), quad=J)
        assert got.unstable.tolist() == want, (h, got.unstable)
        deg = np.diff(plan.adj_ptr).astype(np.float32)
        assert np.array_equal(got.field_out[0], np.float32(h) - deg) and np.array_equal(got.field_out[1], np.float32(h) + deg)


def test_cold_chains_sit_in_local_minima_random_rows_do_not():
    """pegasus64, drawn at beta 20 under prefactor 0.3 (|Js| up to 1, fields of order 1: an unstable spin survives a sweep with
    probability exp(-40 |f|)) and scored under the same fields: most records are local minima and hardly a spin is unstable,
    while a random row has half its spins unstable and is a local minimum with probability 2^-64."""
    case = _case("pegasus64")
    pl = {k: smp.pseudo_likelihood(case.rows[k].view(41, 7, case.W), case.gh, case.lin, case.quad, beta=20.0, prefactor=0.3,
                                   linear_range=H_RANGE, quadratic_range=J_RANGE) for k in ("trace", "noise")}
    share = {k: float(v.local_minimum_share) for k, v in pl.items()}
    frac = {k: float(v.unstable.double().mean()) / 64 for k, v in pl.items()}
    print(f"local_minimum_share {share}, unstable spins per spin {frac}, per-spin log PL " + str({k: float(v.per_spin) for k, v in pl.items()}))
    assert share["trace"] >= 0.5 and share["noise"] == 0.0
    assert frac["trace"] <= 0.05 and 0.4 <= frac["noise"] <= 0.6
    assert float(pl["trace"].per_spin) > float(pl["noise"].per_spin)


# ------------------------------------------------------------------------------------------------ 3. layouts and robustness
@pytest.mark.parametrize("C,M", [(1, 5), (41, 7), (130, 2)])
@pytest.mark.parametrize("name", GRAPHS)
def test_trace_layout(name, C, M):
    """groups = C, group_stride = M W, rows = M, row_stride = W: element c M + m is record m of chain c."""
    case = _case(name)
    worst = {}
    for kind in ("trace", "noise"):
        bits = case.rows[kind][:C * M].contiguous()
        got = _run(case, bits, M, case.W, C, M * case.W, 0.3, 0.5)
        _worst(worst, _ratios(case, got, case.want(kind, 0.3, 0.5), np.arange(C * M)))
        flat = _run(case, bits, C * M, case.W, 1, 0, 0.3, 0.5)
        for k in OUT:  # the same rows as a flat set: the same bits
            assert np.array_equal(getattr(got, k), getattr(flat, k)), k
        via = F.grbm_fields_packed(bits.view(C, M, case.W), case.gh, case.lin, case.quad, beta=0.5, prefactor=0.3, linear_range=H_RANGE,
                                   quadratic_range=J_RANGE, fields=True)
        assert via.log_pl.shape == (C, M) and via.unstable.shape == (C, M) and via.fields.shape == (C, M, case.plan.n)
        assert via.log_pl.dtype == torch.float64 and via.unstable.dtype == torch.int32 and via.fields.dtype == torch.float32
        for k, t in zip(OUT, via):
            assert t.is_cuda and np.array_equal(t.cpu().numpy().ravel(), getattr(got, k).ravel()), k
    print(f"FIELDS-RATIO {name} trace {C}x{M}: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", GRAPHS)
def test_views_and_padded_rows_need_no_copy(name):
    case = _case(name)
    W, n = case.W, case.plan.n
    call = lambda b: F.grbm_fields_packed(b, case.gh, case.lin, case.quad, beta=1.5, prefactor=0.05, linear_range=H_RANGE,  # noqa: E731
                                          quadratic_range=J_RANGE, fields=True)
    worst = {}
    for kind in ("trace", "noise"):
        o = case.want(kind, 0.05, 1.5)
        flat, trace = case.rows[kind], case.rows[kind].view(41, 7, W)
        idx = np.arange(287).reshape(41, 7)
        padded = torch.from_numpy(np.concatenate([case.host[kind], case.pad_noise], axis=1).view(np.int32)).cuda()  # rows of W + 3 words
        for view, sel in ((trace[:, 1:], idx[:, 1:]), (trace[::2], idx[::2]), (trace[:, ::3], idx[:, ::3]), (flat[5::7], idx.ravel()[5::7]),
                          (padded[:, :W], idx.ravel()), (padded.view(41, 7, W + 3)[:, :, :W], idx)):
            assert not view.is_contiguous() or view.shape[0] == 1
            f = call(view)
            got = _Got()
            got.log_pl, got.unstable = f.log_pl.cpu().numpy().ravel(), f.unstable.cpu().numpy().ravel()
            got.cond_sum, got.cond_pair, got.field_out = f.cond_sum.cpu().numpy(), f.cond_pair.cpu().numpy(), f.fields.cpu().numpy().reshape(-1, n)
            assert f.log_pl.shape == sel.shape
            _worst(worst, _ratios(case, got, o, sel.ravel()))
            same = call(view.contiguous())
            for a, b in zip(f, same):  # the view and its copy: the same bits
                assert torch.equal(a, b)
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", GRAPHS)
def test_each_output_alone_gives_the_same_bits_and_two_calls_agree(name):
    case = _case(name)
    for kind, rows in (("trace", 287), ("noise", 65)):
        bits = case.rows[kind][:rows].contiguous()
        both = [_run(case, bits, rows, case.W, 1, 0, 0.3, 1.5) for _ in range(2)]
        for k in OUT:
            assert np.array_equal(getattr(both[0], k), getattr(both[1], k)), k
        for which in (("log_pl",), ("unstable",), ("cond_sum", "cond_pair"), ("field_out",), ("log_pl", "field_out")):
            alone = _run(case, bits, rows, case.W, 1, 0, 0.3, 1.5, which)
            for k in OUT:
                assert (getattr(alone, k) is None) == (k not in which)
                if k in which:
                    assert np.array_equal(getattr(alone, k), getattr(both[0], k)), (which, k)


@pytest.mark.parametrize("name", GRAPHS)
def test_accumulate_adds_onto_the_pooled_sums(name):
    """Two calls over two parts of the rows, the second accumulating, against one call over all of them.  Parts cut at a tile
    boundary with a last part of one tile (256 + 31 rows) add the same partial sums in the same order but for the last one:
    one rounding per element, |diff| <= u |value|.  Parts cut at row 100 regroup the addends: both results are orderings of the
    same T addends (the m are the same bits), each within the 2 T u per unit addend that the bounds above allow an ordering
    of the exact sum, so within 4 T u of each other (|m| <= 1 for a spin; 8 T u for an edge's two unit addends a row)."""
    case = _case(name)
    n, E, T = case.plan.n, case.plan.n_edges, 287
    bits = case.rows["trace"]
    full = _run(case, bits, T, case.W, 1, 0, 0.3, 0.5, ("cond_sum", "cond_pair"))
    for cut, tol_s, tol_p in ((256, U * np.abs(full.cond_sum), U * np.abs(full.cond_pair)), (100, 4 * T * U, 8 * T * U)):
        into = (torch.full((n + 1,), GUARD, dtype=torch.float64, device="cuda"), torch.full((E + 1,), GUARD, dtype=torch.float64, device="cuda"))
        _run(case, bits[:cut].contiguous(), cut, case.W, 1, 0, 0.3, 0.5, ("cond_sum", "cond_pair"), into=into)
        two = _run(case, bits[cut:].contiguous(), T - cut, case.W, 1, 0, 0.3, 0.5, ("cond_sum", "cond_pair"), into=into, accumulate=1)
        ds, dp = np.abs(two.cond_sum - full.cond_sum), np.abs(two.cond_pair - full.cond_pair)
        print(f"{name} cut at {cut}: cond_sum differs by up to {ds.max():.3e} (allowed {np.max(tol_s):.3e}), cond_pair by {dp.max():.3e} "
              f"(allowed {np.max(tol_p):.3e})")
        assert (ds <= tol_s).all() and (dp <= tol_p).all(), cut
    assert np.abs(full.cond_sum).max() > 1.0
    # the Python surface: out= adds onto a pair
    kw = dict(beta=0.5, prefactor=0.3, linear_range=H_RANGE, quadratic_range=J_RANGE, log_pl=False, unstable=False)
    first = F.grbm_fields_packed(bits[:256], case.gh, case.lin, case.quad, **kw)
    assert first.log_pl is None and first.unstable is None and first.fields is None
    second = F.grbm_fields_packed(bits[256:], case.gh, case.lin, case.quad, out=(first.cond_sum, first.cond_pair), **kw)
    assert second.cond_sum is first.cond_sum and (np.abs(second.cond_sum.cpu().numpy() - full.cond_sum) <= U * np.abs(full.cond_sum)).all()


def test_rejected_calls_leave_the_outputs_intact():
    case = _case("random77")
    bits, W = case.rows["noise"][:35].contiguous(), case.W
    for kw in (dict(null="g"), dict(null="linear"), dict(null="quadratic"), dict(null="bits")):
        _run(case, bits, 35, W, 1, 0, 0.3, 0.5, expect=-1, **kw)
    _run(case, bits, 35, W, 1, 0, 0.3, 0.5, (), expect=-1)
    _run(case, bits, 35, W, 1, 0, 0.3, 0.5, ("log_pl", "cond_sum"), expect=-1)
    _run(case, bits, 35, W, 1, 0, 0.3, 0.5, ("cond_pair",), expect=-1)
    _run(case, bits, 0, W, 1, 0, 0.3, 0.5, expect=-1)
    _run(case, bits, 35, W - 1, 1, 0, 0.3, 0.5, expect=-1)
    _run(case, bits, 5, W, 7, -1, 0.3, 0.5, expect=-1)
    _run(case, bits, 35, W, 1, 0, float("nan"), 0.5, expect=-1)
    for beta in (float("nan"), float("inf"), -0.5):
        _run(case, bits, 35, W, 1, 0, 0.3, beta, expect=-1)
    _run(case, bits, 35, W, 1, 0, 0.3, 0.5, ws_short=True, expect=-3)
    assert _run(case, bits, 35, W, 1, 0, 0.3, 0.5, ("log_pl",), ws_short=True).log_pl is not None  # (no pooled sums: no workspace)


def test_python_layers_equal_the_c_entry():
    from image_generation_amd.plugin import GraphRestrictedBoltzmannMachine

    plan, nodes = _solver_plan("zephyr", 128)
    rng = np.random.default_rng(2)
    h = (20.0 * rng.uniform(-1, 1, plan.n)).astype(np.float32)
    J = (5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)
    grbm = GraphRestrictedBoltzmannMachine(nodes, list(zip(np.asarray(nodes)[plan.edge_i].tolist(),
                                                           np.asarray(nodes)[plan.edge_j].tolist()))).cuda()
    with torch.no_grad():
        grbm._linear.copy_(torch.from_numpy(h).cuda())
        grbm._quadratic.copy_(torch.from_numpy(J).cuda())
    ranges = dict(prefactor=0.3, linear_range=H_RANGE, quadratic_range=J_RANGE)
    s = smp.GibbsSampler(plan, nodes, beta=1.5, sweeps=4, seed=SEED, persistent=True, h_range=H_RANGE, j_range=J_RANGE)
    trace = grbm.sample_trace(s, num_reads=9, num_sweeps=12, burn_in=2, thin=3, **ranges)
    gh, lin, quad = grbm.graph_handle("cuda"), grbm._linear.detach(), grbm._quadratic.detach()
    f = F.grbm_fields_packed(trace.bits, gh, lin, quad, beta=1.5, **ranges)
    hs, Js = gibbs.scaled_fields(h, J, 0.3, H_RANGE, J_RANGE)
    o = fo.fields(trace.bits.cpu().numpy(), plan.n, hs, Js, plan.edge_i, plan.edge_j, 1.5)
    assert f.log_pl.shape == (9, 3) and (np.abs(f.log_pl.cpu().numpy().ravel() - o.log_pl) <= fo.bound_log_pl(plan.n, o.S)).all()
    assert np.array_equal(f.unstable.cpu().numpy().ravel(), o.unstable)
    spin_sum, pair_sum = trace_oracle.moments(o.s, plan.edge_i, plan.edge_j)
    for pl in (trace.pseudo_likelihood(gh, lin, quad, beta=1.5, **ranges), grbm.pseudo_likelihood(trace.bits, beta=1.5, **ranges),
               grbm.pseudo_likelihood(trace.unpack(), beta=1.5, **ranges)):
        assert isinstance(pl, smp.PseudoLikelihood) and pl.count == 27 and pl.n == plan.n and pl.beta == 1.5
        assert torch.equal(pl.log_pl, f.log_pl) and torch.equal(pl.unstable, f.unstable)
        assert torch.equal(pl.cond_sum, f.cond_sum) and torch.equal(pl.cond_pair, f.cond_pair)
        assert np.array_equal(pl.spin_sum.cpu().numpy(), spin_sum) and np.array_equal(pl.pair_sum.cpu().numpy(), pair_sum)
        assert pl.mean.is_cuda and pl.std_err.is_cuda and float(pl.std_err) > 0
    flat = grbm.pseudo_likelihood(trace.bits.view(27, -1), beta=1.5, **ranges)
    assert torch.equal(flat.log_pl, f.log_pl.view(27)) and torch.equal(flat.cond_pair, f.cond_pair)
    mean, gl, gq = grbm.pseudo_likelihood_grad(trace.bits, beta=1.5, **ranges)
    want = fo.estimates(o.log_pl.reshape(9, 3), o.unstable, o.cond_sum, o.cond_pair, spin_sum, pair_sum)
    assert gl.shape == grbm._linear.shape and gq.shape == grbm._quadratic.shape and gl.dtype == torch.float64 and gl.is_cuda
    assert abs(float(mean) - want["mean"]) <= 1e-12 * abs(want["mean"])
    mask_h = (np.float32(0.3) * h >= -4) & (np.float32(0.3) * h <= 4)
    assert 0 < mask_h.sum() < plan.n
    assert np.allclose(gl.cpu().numpy().ravel(), -1.5 * 0.3 / 27 * want["residual_linear"] * mask_h, rtol=1e-9, atol=1e-12)
    mask_j = (np.float32(0.3) * J >= -1) & (np.float32(0.3) * J <= 1)
    assert np.allclose(gq.cpu().numpy().ravel(), -1.5 * 0.3 / 27 * want["residual_quadratic"] * mask_j, rtol=1e-9, atol=1e-12)
    with pytest.raises(_lib.DvgError, match="device of bits"):
        F.grbm_fields_packed(trace.bits, gh, lin.cpu(), quad, beta=1.5, **ranges)


def test_model_wrapper_prior_pseudo_likelihood():
    from image_generation_amd.data import synthetic_images
    from image_generation_amd.model_wrapper import ModelWrapper

    torch.manual_seed(0)
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(ROOT, "tests", "golden", "step_params.yaml"))
    m.setup()
    m.overlap_sampler = False  # (as in the AIS file: this test takes no stream from the process's pool)
    images = synthetic_images(5, seed=3, device="cuda").reshape(5, 1, 32, 32)
    res = m.prior_pseudo_likelihood(images, num_reads=33, num_sweeps=20, burn_in=6, thin=2)
    s = m.sampler
    assert (s.trace_sweep_count, s.sweep_count, s.calls, s.ais_sweep_count) == (20, 0, 0, 0) and s._state is None
    assert set(res) == {"data", "prior", "gap", "local_minimum_share_prior"}
    data, prior = res["data"], res["prior"]
    assert isinstance(data, smp.PseudoLikelihood) and data.log_pl.shape == (5,) and prior.log_pl.shape == (33, 7)
    assert data.beta == prior.beta == float(s.beta)
    assert float(res["gap"]) == float(data.per_spin - prior.per_spin) and 0.0 <= float(res["local_minimum_share_prior"]) <= 1.0
    s.reset()  # the same draw again, by hand
    trace = m._grbm.sample_trace(s, prefactor=m.PREFACTOR, linear_range=m.linear_range, quadratic_range=m.quadratic_range,
                                 num_reads=33, num_sweeps=20, burn_in=6, thin=2)
    again = trace.pseudo_likelihood(m._grbm.graph_handle(trace.bits.device), m._grbm._linear.detach(), m._grbm._quadratic.detach(),
                                    beta=float(s.beta), prefactor=m.PREFACTOR, linear_range=m.linear_range, quadratic_range=m.quadratic_range)
    assert torch.equal(again.log_pl, prior.log_pl) and torch.equal(again.cond_pair, prior.cond_pair)
    h, J = m._grbm._linear.detach().cpu().numpy().reshape(-1), m._grbm._quadratic.detach().cpu().numpy().reshape(-1)
    hs, Js = gibbs.scaled_fields(h, J, m.PREFACTOR, m.linear_range, m.quadratic_range)
    plan = m._grbm.plan
    o = fo.fields(trace.bits.cpu().numpy(), plan.n, hs, Js, plan.edge_i, plan.edge_j, float(s.beta))
    assert (np.abs(prior.log_pl.cpu().numpy().ravel() - o.log_pl) <= fo.bound_log_pl(plan.n, o.S)).all()
    assert np.array_equal(prior.unstable.cpu().numpy().ravel(), o.unstable)
