"""The block-Gibbs draw ALONE (nothing else on the chip): `python tools/gibbs_bench.py [n chains sweeps]` on an MI355X.
Prints the draw time per kernel form -- inside a training step the same draw shares its CUs
with the encoder's GEMMs and takes longer (bench.py's `sampler` entry is that in-situ number).
`clamped`: also the conditional draw (per-chain masks) at held fractions 0, 0.5 and 0.9 -- timed as the call
GibbsSampler.sample_conditional with int8 / uint8 tensors: the kernel plus the call's own copy of the start state (a
(chains, n) int8 device copy), where the plain rows time the kernel on the sampler's persistent chains.
`annealed`: also the annealed draw (dvg_gibbs_sample_annealed) on the sampler's persistent chains, as the plain rows are
timed: a geometric schedule 0.05 -> 20 shared by all chains (GibbsSampler.set_beta_schedule), and the same kernel with a
table row per chain (a ladder: chain c ends at beta 20 (c + 1) / chains).
`ais`: also the weighed annealed draw (dvg_gibbs_sample_ais: the annealed draw plus each chain's log importance weight and
energy, accumulated in the kernel), timed as the annealed rows are -- the raw call on persistent chains, the same shared
schedule and the same ladder; a second line gives the sums of the last draw's log weights and energies.
`tempered`: also the exchange draw (dvg_gibbs_sample_tempered: ladders of `replicas=R` chains, default 4, `chains` / R of them, on a
geometric ladder 10 -> 20), timed as the ais rows are -- the raw call on persistent chains and rungs: once with no exchange due
(swap_every beyond every sweep: the weighed draw's work per update, nothing else) and once with an exchange after every sweep; a
second line gives the last draw's accepted exchanges per pair of rungs.
`tempered_trace`: also the traced exchange draw (dvg_gibbs_sample_tempered_traced: the exchange draw plus, per rung and recorded
sweep, the packed state and energy of the chain holding it, and per chain the rung), `replicas=R` as above, `thin=T` (default 1),
swap_every=1: the raw exchange call, the traced call with all three records and with the states alone, the cost per record; then
the two routes to a history of the ladder through the sampler -- a sample_tempered call per record that hands state and rungs on
plus a pack_spins of its samples, against one sample_tempered_trace -- and whether the two record the same states.
`trace`: also the traced draw (dvg_gibbs_sample_traced: the plain draw plus the chains' states after every `thin`-th sweep, one bit
per spin), timed as the ais rows are -- the raw call on persistent chains -- at thin=10 and thin=1 (burn_in 0); then
dvg_grbm_moments_packed over the thin=1 records (chains x sweeps rows of n / 8 bytes) and, next to it, dvg_grbm_suffstats over the
same rows unpacked to float32 (the unpacking is not timed); a last line says whether the two give the same moments.
`autocorr`: also dvg_trace_autocorr (the exact sums over chains and records of s_i(m) s_i(m + t), t = 0 .. 64, of bit-packed records)
over the thin=1 trace of that draw (chains x sweeps records), timed as the moments row is; next to it the same sums by torch over the
same records unpacked to float32, one product and one reduction per lag (the unpacking is not timed); a last line says whether the
two agree.
`overlap`: also dvg_packed_overlap (the exact histogram of Hamming distances between bit-packed rows, and every row's nearest
partner) twice: over the thin=1 trace of that draw in self mode at equal times (`sweeps` groups of `chains` rows), and as a novelty
call, `novelty=AxB` (default 1024x60000) random rows of n spins in cross mode with `nearest`; next to each the same by torch on
the rows unpacked to float32 -- a (batched) matmul, (n - G) / 2, torch.bincount, and min for the nearest row (the unpacking is not
timed); a last line each says whether the two agree element by element.
`energy`: also dvg_grbm_energy_packed (the float64 energies of bit-packed rows under the scaled, clamped fields, "DVG energy v1")
over the thin=1 trace of that draw (chains x sweeps rows), timed as the moments row is; next to it the stock path -- sampler.unpack_spins
to float32 followed by dvg_grbm_energy on the scaled, clamped fields -- timed with the unpacking and without it; a last line gives the
largest deviation of the float32 energies from the float64 ones against the float32 rounding of that call's output.
`correlation`: also dvg_packed_correlation (the exact sums of s_i s_j over bit-packed rows for EVERY pair of spins, "DVG corr v1")
against the stock path -- sampler.unpack_spins -> .float() -> x.T @ x, exact below 2^24 rows -- in this one process, at three sizes
of its own (the n, chains and sweeps of the command line do not enter): the thin=1 traces of 256 chains x 200 sweeps on the Zephyr
sub-graphs of 512 and of 1024 spins (51 200 rows each) and of 32 chains x 32 sweeps on the latter (1024 rows).  The two paths
alternate, five timings of five calls each, medians; the raw entry with its workspace allocated once, functional.packed_correlation
(which allocates workspace and outputs per call) beside it, and the stock product alone (the unpacking not timed); a last line each
says whether the integers of the two paths are equal.
`fields`: also dvg_grbm_fields_packed (pseudo-log-likelihoods, unstable-spin counts and Rao-Blackwellised moment sums of bit-packed
rows through the sampler's local fields, "DVG fields v1") over the thin=1 trace of that draw (chains x sweeps rows) at beta 1, the
raw entry with outputs and workspace allocated once; next to it the stock path in torch -- sampler.unpack_spins to float32, x @
J_dense + h, float64 softplus and tanh, the pooled products over the edge list -- timed with the unpacking and without it; a last line
gives the largest deviations of the stock path's values (its float32 fields come from a matmul, in another order) from the entry's.
`descend`: also dvg_grbm_descend_packed (zero-temperature descent of bit-packed rows to local minima, "DVG descent v1") over chains x
sweeps rows of two kinds -- the thin=1 trace of that draw, and random words -- max_sweeps 1000, the raw entry with its outputs
allocated once; next to it the stock path in torch with its unpack and repack -- sampler.unpack_spins to float32, per colour class
x @ J_dense[:, class] + h[class] and a masked sign flip, swept until no row moves (one host read per sweep), sampler.pack_spins
-- and a last line each that says whether the two paths return equal rows, and what the descent did (sweeps, flips, minima).
`population`: also population annealing ("DVG PA v1").  (a) dvg_population_resample alone, `resample=PxR,...` (default 8x128,1x65536)
populations x chains of n spins with normal(0, 3) log weights, states gathered, against the same operation by torch: exp of the
shifted weights, cumsum, searchsorted, index_select (float64: its parents may differ at near ties; the line says how many do).
(b) GibbsSampler.sample_population of `chains` chains in 8 populations over `sweeps` betas 0 -> 20 at one sweep each, against ONE
dvg_gibbs_sample_ais call of the same sweeps, against the draw's AIS calls alone (one call per step: launches plus the
start-energy walk each call repeats) and its resample calls alone: the per-step overhead and the resample's share of it.  (c)
std_err of log Z at equal sweeps, `seeds=K` (default 4) seeds each: population annealing (between its 8 populations), AIS by its
effective sample size, and AIS between 8 groups of its chains -- the populations' formula on the same footing.
`chain_fields`: also the draw with a linear field per chain (dvg_gibbs_sample_fields, "DVG field v1"), timed as the ais rows are -- the
raw call on persistent chains -- with N(0, 1) fields, a row per chain, and with one shared row; it runs the rolled kernel, so the
row to hold it against is `rolled reference`; a second line gives the plans of the two (workgroup, LDS).
`distinct`: also dvg_packed_distinct (the equivalence classes of bit-packed rows under equality, "DVG distinct v1": first, id, rep and
count) on 65 536 rows of n = 256 and 16 384 rows of n = 1024, all rows distinct and rows drawn from a pool of 256 states, against
torch.unique(dim=0, return_inverse=True, return_counts=True) on the same device rows; a second line says whether the two agree.
`link`: also dvg_packed_bonds ("DVG bonds v1") and dvg_packed_overlap_link ("DVG link overlap v1", self mode at equal times) on the thin =
1 trace, against the stock torch path on the same rows (unpack to float32, gather the bonds, two batched matmuls, bincount and
index_add); further lines say whether the four sums agree and what the link overlap of the draw is.
`repeat=K`: K timings of each row instead of one (the spread of a row is max - min of its K)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from image_generation_amd import _lib, graphs, sampler as smp

n, C, sweeps = (int(v) for v in (sys.argv[1:4] if len(sys.argv) > 3 else (512, 256, 200)))
seed = 775321899904
topology = graphs.pegasus_graph(16) if "pegasus" in sys.argv else graphs.zephyr_graph(12)  # (bench.py: c1 / c2 Pegasus, c3 / c5 Zephyr)
mg, _ = graphs.get_graph_mapping(graphs.greedy_get_subgraph(n, seed, topology))
nodes, ei, ej = graphs.edges_of(mg)
plan = graphs.build_plan(n, ei, ej)
rng = np.random.default_rng(1)
lin = torch.from_numpy((0.05 * rng.uniform(-1, 1, n)).astype(np.float32)).cuda()
quad = torch.from_numpy((5.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)).cuda()
print(f"n={n} chains={C} sweeps={sweeps} colours={plan.n_colours} max class={max(np.diff(plan.class_ptr))} "
      f"max degree={int(np.diff(plan.adj_ptr).max())}")
only_default = "default" in sys.argv  # (PMC passes: the product's form only)
repeat = max([int(a.split("=")[1]) for a in sys.argv if a.startswith("repeat=")] + [1])


def timed(draw):
    """us per draw, five draws per timing, `repeat` timings after one warm-up draw; the last draw's output"""
    out = draw()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            out = draw()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 5 * 1e3)
    return ts, out


def row(name, ts, updates, out):
    t = float(np.median(ts))
    spread = f"  (median of {len(ts)}: min {min(ts):.1f} max {max(ts):.1f})" if len(ts) > 1 else ""
    print(f"  {name:26s} {t:9.1f} us per draw  {updates/t/1e3:8.2f} G spin updates/s  checksum {float(out.sum()):.0f}{spread}")


forms = (("default", dict()), ("one row at a time", dict(gibbs_generic=2)), ("rolled reference", dict(gibbs_generic=1)),
         ("chains side by side, 8-chain workgroups", dict(gibbs_generic=4)))
for name, opts in forms[:1] if only_default else forms:
    with _lib.option_scope(**opts):
        s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
        ts, out = timed(lambda: s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C))
        row(name, ts, C * n * sweeps, out)
if "clamped" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    start = torch.from_numpy(np.where(rng.uniform(size=(C, n)) < 0.5, -1, 1).astype(np.int8)).cuda()
    for frac in (0.0, 0.5, 0.9):
        clamp = torch.from_numpy((rng.uniform(size=(C, n)) < frac).astype(np.uint8)).cuda()
        ts, out = timed(lambda: s.sample_conditional(lin, quad, 0.05, (-4, 4), (-1, 1), start, clamp))
        row("cond. call, %.0f %% held" % (100 * frac), ts, (C * n - int(clamp.sum())) * sweeps, out)
if "chain_fields" in sys.argv:
    from image_generation_amd import dev

    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    per_chain = torch.from_numpy(rng.standard_normal((C, n)).astype(np.float32)).cuda()
    for name, rows, stride in (("fields, a row per chain", per_chain, n), ("fields, one shared row", per_chain[0].contiguous(), 0)):
        state = torch.empty((C, n), dtype=torch.int8, device="cuda")
        out = torch.empty((C, n), dtype=torch.float32, device="cuda")
        at = [0]

        def with_fields():
            _lib.check(_lib.lib().dvg_gibbs_sample_fields(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0, 20.0,
                                                          state.data_ptr(), C, 0, seed, at[0], sweeps, int(at[0] == 0), rows.data_ptr(),
                                                          stride, out.data_ptr(), None, _lib.stream_ptr()), "dvg_gibbs_sample_fields")
            at[0] += sweeps
            return out

        ts, out = timed(with_fields)
        row(name, ts, C * n * sweeps, out)
    with _lib.option_scope(gibbs_generic=1):
        rolled = dev.gibbs_draw_plan(plan, C, "plain")
    field = dev.gibbs_draw_plan(plan, C, "field")
    for name, p in (("rolled reference", rolled), ("fields", field)):
        print(f"  {'':26s} {name}: gibbs_kernel<{p['params']['LPC']}, {p['params']['WAVES']}>, {p['workgroups']} workgroups of "
              f"{p['chains_per_workgroup']} chains, {p['lds_bytes']} B of LDS")
if "annealed" in sys.argv:
    shared = smp.beta_schedule(0.05, 20.0, sweeps)
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    s.set_beta_schedule(shared)
    ts, out = timed(lambda: s.sample_native(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C))
    row("annealed, shared table", ts, C * n * sweeps, out)
    # a row per chain, on persistent chains like the rows above: the raw call (sample_annealed draws one-off chains)
    ladder = torch.from_numpy(np.stack([smp.beta_schedule(0.05, 20.0 * (c + 1) / C, sweeps) for c in range(C)])).cuda()
    state = torch.empty((C, n), dtype=torch.int8, device="cuda")
    out = torch.empty((C, n), dtype=torch.float32, device="cuda")
    at = [0]

    def per_chain():
        _lib.check(_lib.lib().dvg_gibbs_sample_annealed(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0,
                                                        ladder.data_ptr(), sweeps, state.data_ptr(), C, 0, seed, at[0], sweeps,
                                                        int(at[0] == 0), out.data_ptr(), None, _lib.stream_ptr()),
                   "dvg_gibbs_sample_annealed")
        at[0] += sweeps
        return out

    ts, out = timed(per_chain)
    row("annealed, table per chain", ts, C * n * sweeps, out)
if "ais" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    shared = torch.from_numpy(smp.beta_schedule(0.05, 20.0, sweeps)).cuda()
    ladder = torch.from_numpy(np.stack([smp.beta_schedule(0.05, 20.0 * (c + 1) / C, sweeps) for c in range(C)])).cuda()
    for name, table, stride in (("ais, shared table", shared, 0), ("ais, table per chain", ladder, sweeps)):
        state = torch.empty((C, n), dtype=torch.int8, device="cuda")
        out = torch.empty((C, n), dtype=torch.float32, device="cuda")
        log_w = torch.empty((C,), dtype=torch.float64, device="cuda")
        energy = torch.empty((C,), dtype=torch.float64, device="cuda")
        at = [0]

        def weighed():
            # (the first draw starts fresh chains, at beta 0; the later ones go on from the chains' states, each a sample at
            # its table's last entry or near it: the weights of those draws are timed, not used)
            _lib.check(_lib.lib().dvg_gibbs_sample_ais(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0,
                                                       table.data_ptr(), stride, 0.0 if at[0] == 0 else 20.0, state.data_ptr(), C, 0,
                                                       seed, at[0], sweeps, int(at[0] == 0), out.data_ptr(), log_w.data_ptr(),
                                                       energy.data_ptr(), None, _lib.stream_ptr()),
                       "dvg_gibbs_sample_ais")
            at[0] += sweeps
            return out

        ts, out = timed(weighed)
        row(name, ts, C * n * sweeps, out)
        print(f"  {'':26s} sum of log weights {float(log_w.sum()):.6e}  sum of energies {float(energy.sum()):.6e}")
if "tempered" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    R = max([int(a.split("=")[1]) for a in sys.argv if a.startswith("replicas=")] + [4])
    Q = C // R
    ladder = torch.from_numpy(smp.beta_schedule(10.0, 20.0, R)).cuda()
    for name, every in (("tempered, no exchange due", 1 << 30), ("tempered, swap_every=1", 1)):
        state = torch.empty((Q * R, n), dtype=torch.int8, device="cuda")
        rung = torch.empty((Q * R,), dtype=torch.int32, device="cuda")
        out = torch.empty((Q * R, n), dtype=torch.float32, device="cuda")
        energy = torch.empty((Q * R,), dtype=torch.float64, device="cuda")
        accept = torch.empty((Q * R,), dtype=torch.int32, device="cuda")
        at = [0]

        def exchange():
            _lib.check(_lib.lib().dvg_gibbs_sample_tempered(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0,
                                                            ladder.data_ptr(), R, every, state.data_ptr(), rung.data_ptr(), Q * R, 0,
                                                            seed, at[0], sweeps, int(at[0] == 0), out.data_ptr(), energy.data_ptr(),
                                                            accept.data_ptr(), None, _lib.stream_ptr()),
                       "dvg_gibbs_sample_tempered")
            at[0] += sweeps
            return out

        ts, out = timed(exchange)
        row(name, ts, Q * R * n * sweeps, out)
        print(f"  {'':26s} {Q} ladders x {R}: accepted per pair {accept.view(Q, R).sum(0)[:-1].tolist()} of {Q * (sweeps // every // 2)}"
              f"  sum of energies {float(energy.sum()):.6e}")
if "tempered_trace" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    R = max([int(a.split("=")[1]) for a in sys.argv if a.startswith("replicas=")] + [4])
    thin = max([int(a.split("=")[1]) for a in sys.argv if a.startswith("thin=")] + [1])
    Q, W, M = C // R, (n + 31) // 32, sweeps // thin
    ladder_host = smp.beta_schedule(10.0, 20.0, R)
    ladder = torch.from_numpy(ladder_host).cuda()
    state = torch.empty((Q * R, n), dtype=torch.int8, device="cuda")
    rung = torch.empty((Q * R,), dtype=torch.int32, device="cuda")
    out = torch.empty((Q * R, n), dtype=torch.float32, device="cuda")
    energy = torch.empty((Q * R,), dtype=torch.float64, device="cuda")
    accept = torch.empty((Q * R,), dtype=torch.int32, device="cuda")
    bits = torch.empty((Q, R, M, W), dtype=torch.int32, device="cuda")
    e_trace = torch.empty((Q, R, M), dtype=torch.float64, device="cuda")
    walk = torch.empty((Q, R, M), dtype=torch.uint8, device="cuda")
    at = [0]

    def exchange():
        _lib.check(_lib.lib().dvg_gibbs_sample_tempered(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0,
                                                        ladder.data_ptr(), R, 1, state.data_ptr(), rung.data_ptr(), Q * R, 0, seed,
                                                        at[0], sweeps, int(at[0] == 0), out.data_ptr(), energy.data_ptr(),
                                                        accept.data_ptr(), None, _lib.stream_ptr()), "dvg_gibbs_sample_tempered")
        at[0] += sweeps
        return out

    def recorded(with_energies, with_walk):
        def draw():
            _lib.check(_lib.lib().dvg_gibbs_sample_tempered_traced(
                s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0, ladder.data_ptr(), R, 1, state.data_ptr(),
                rung.data_ptr(), Q * R, 0, seed, at[0], sweeps, int(at[0] == 0), out.data_ptr(), energy.data_ptr(), accept.data_ptr(),
                bits.data_ptr(), e_trace.data_ptr() if with_energies else None, walk.data_ptr() if with_walk else None, 0, thin, None,
                _lib.stream_ptr()), "dvg_gibbs_sample_tempered_traced")
            at[0] += sweeps
            return out
        return draw

    ts, o = timed(exchange)
    t_plain = float(np.median(ts))
    row(f"tempered, {Q} x {R}, swap_every=1", ts, Q * R * n * sweeps, o)
    at[0] = 0
    ts, o = timed(recorded(True, True))
    t_all = float(np.median(ts))
    row(f"... traced, thin={thin}, all three", ts, Q * R * n * sweeps, o)
    at[0] = 0
    ts, o = timed(recorded(False, False))
    t_bits = float(np.median(ts))
    row(f"... traced, thin={thin}, states only", ts, Q * R * n * sweeps, o)
    print(f"  {'':26s} {M} records: {(t_all - t_plain) / M:.3f} us per record with energies and walk, {(t_bits - t_plain) / M:.3f} us the "
          f"states alone ({Q * R * (4 * W + 9)} B a record)")

    # the route without the entry: a call per record that hands state and rungs on, and a pack_spins per call
    def by_calls():
        res, rows = None, []
        for m in range(M):
            res = s.sample_tempered(lin, quad, 0.05, (-4, 4), (-1, 1), ladder_host, num_ladders=Q, num_sweeps=thin, swap_every=1,
                                    start=None if res is None else res.state, rungs=None if res is None else res.rungs)
            rows.append(smp.pack_spins(res.samples))
        return torch.stack(rows, 2)

    def by_entry():
        return s.sample_tempered_trace(lin, quad, 0.05, (-4, 4), (-1, 1), ladder_host, num_ladders=Q, num_sweeps=sweeps,
                                       swap_every=1, thin=thin).bits

    ts, a = timed(by_calls)
    t_calls = float(np.median(ts))
    print(f"  {'a call per record + pack':26s} {t_calls:9.1f} us per draw  ({t_calls / M:.2f} us per record; min {min(ts):.1f} max {max(ts):.1f})")
    ts, b = timed(by_entry)
    t_entry = float(np.median(ts))
    print(f"  {'sample_tempered_trace':26s} {t_entry:9.1f} us per draw  ({t_calls / t_entry:.2f} x faster; min {min(ts):.1f} max {max(ts):.1f})")
    s.reset()  # (the streams advanced while timing: compared from the same start)
    a = by_calls()
    s.reset()
    b = by_entry()
    print(f"  {'':26s} from the same start the two routes record the same states: {bool(torch.equal(a, b))} (but for near ties: the route by "
          f"calls sums its start energies afresh every call)")
if "trace" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    W = (n + 31) // 32
    for thin in (10, 1):
        M = sweeps // thin
        state = torch.empty((C, n), dtype=torch.int8, device="cuda")
        out = torch.empty((C, n), dtype=torch.float32, device="cuda")
        bits = torch.empty((C, M, W), dtype=torch.int32, device="cuda")
        at = [0]

        def traced():
            _lib.check(_lib.lib().dvg_gibbs_sample_traced(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0, 20.0,
                                                          state.data_ptr(), C, 0, seed, at[0], sweeps, int(at[0] == 0), out.data_ptr(),
                                                          bits.data_ptr(), 0, thin, None, _lib.stream_ptr()),
                       "dvg_gibbs_sample_traced")
            at[0] += sweeps
            return out

        ts, out = timed(traced)
        row(f"traced, thin={thin} ({M} records)", ts, C * n * sweeps, out)
    # the moments of the last draw's C x sweeps records: packed, and through the float32 kernel over the same rows unpacked
    rows = C * sweeps
    spin_sum = torch.empty((n,), dtype=torch.int64, device="cuda")
    pair_sum = torch.empty((plan.n_edges,), dtype=torch.int64, device="cuda")

    def packed():
        _lib.check(_lib.lib().dvg_grbm_moments_packed(s.graph.ptr, bits.data_ptr(), rows, spin_sum.data_ptr(), pair_sum.data_ptr(), 0,
                                                      _lib.stream_ptr()), "dvg_grbm_moments_packed")
        return spin_sum

    ts, _ = timed(packed)
    t = float(np.median(ts))
    print(f"  {'moments, packed rows':26s} {t:9.1f} us per call  {rows} rows x {4 * W} B  (min {min(ts):.1f} max {max(ts):.1f})")
    x = smp.unpack_spins(bits.view(rows, W), n).contiguous()
    acc_l = torch.empty((n,), dtype=torch.float32, device="cuda")
    acc_q = torch.empty((plan.n_edges,), dtype=torch.float32, device="cuda")
    ws = torch.empty(_lib.lib().dvg_grbm_suffstats_workspace_bytes(s.graph.ptr), dtype=torch.uint8, device="cuda")

    def unpacked():
        _lib.check(_lib.lib().dvg_grbm_suffstats(s.graph.ptr, x.data_ptr(), rows, None, 1.0, acc_l.data_ptr(), acc_q.data_ptr(), 0,
                                                 ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "dvg_grbm_suffstats")
        return acc_l

    ts, _ = timed(unpacked)
    t = float(np.median(ts))
    print(f"  {'suffstats, float32 rows':26s} {t:9.1f} us per call  {rows} rows x {4 * n} B  (min {min(ts):.1f} max {max(ts):.1f})")
    same = bool((acc_l.double() == spin_sum.double()).all()) and bool((acc_q.double() == pair_sum.double()).all())
    print(f"  {'':26s} the two give the same sums: {same}  (sum of spin sums {int(spin_sum.sum())}, of pair sums {int(pair_sum.sum())})")
if "autocorr" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    trace = s.sample_trace(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)  # burn_in 0, thin 1: chains x sweeps records
    L, M = min(64, sweeps - 1), sweeps
    lag_sum = torch.empty((L + 1, n), dtype=torch.int64, device="cuda")
    spin_sum = torch.empty((n,), dtype=torch.int64, device="cuda")
    chain_sum = torch.empty((C, n), dtype=torch.int32, device="cuda")

    def packed():
        _lib.check(_lib.lib().dvg_trace_autocorr(trace.bits.data_ptr(), C, M, n, L, lag_sum.data_ptr(), spin_sum.data_ptr(),
                                                 chain_sum.data_ptr(), 0, _lib.stream_ptr()), "dvg_trace_autocorr")
        return lag_sum

    ts, _ = timed(packed)
    t_packed = float(np.median(ts))
    print(f"  {'autocorr, packed records':26s} {t_packed:9.1f} us per call  {C} x {M} records x {4 * ((n + 31) // 32)} B, lags 0..{L}"
          f"  (min {min(ts):.1f} max {max(ts):.1f})")
    x = trace.unpack().contiguous()  # (C, M, n) float32
    by_torch = torch.empty((L + 1, n), dtype=torch.float32, device="cuda")

    def unpacked():
        for t in range(L + 1):
            by_torch[t] = (x[:, :M - t] * x[:, t:]).sum((0, 1))
        return by_torch

    ts, _ = timed(unpacked)
    t_torch = float(np.median(ts))
    print(f"  {'the same by torch, float32':26s} {t_torch:9.1f} us per call  {C} x {M} records x {4 * n} B, {L + 1} lags one at a time"
          f"  (min {min(ts):.1f} max {max(ts):.1f})   {t_torch / t_packed:.1f} x the packed call")
    same = bool((by_torch.double() == lag_sum.double()).all()) and bool((x.sum((0, 1)).double() == spin_sum.double()).all()) and \
        bool((x.sum(1).double() == chain_sum.double()).all())
    print(f"  {'':26s} the two give the same sums: {same}  (sum of lag sums {int(lag_sum.sum())}, of spin sums {int(spin_sum.sum())})")
if "overlap" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    trace = s.sample_trace(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)  # burn_in 0, thin 1: chains x sweeps records
    W, M = (n + 31) // 32, sweeps
    hist = torch.empty((n + 1,), dtype=torch.int64, device="cuda")

    def report(name, ts, what):
        t = float(np.median(ts))
        print(f"  {name:26s} {t:9.1f} us per call  {what}  (min {min(ts):.1f} max {max(ts):.1f})")
        return t

    def packed_self():
        _lib.check(_lib.lib().dvg_packed_overlap(trace.bits.data_ptr(), C, M * W, W, None, 0, 0, 0, M, n, hist.data_ptr(), None, 0,
                                                 _lib.stream_ptr()), "dvg_packed_overlap")
        return hist

    ts, _ = timed(packed_self)
    t_packed = report("overlap, packed trace", ts, f"{M} groups x {C} rows x {4 * W} B, {M * C * (C - 1) // 2} pairs")
    x = trace.unpack().transpose(0, 1).contiguous()  # (M, C, n) float32
    iu = torch.triu_indices(C, C, 1, device="cuda")

    def torch_self():
        d = (n - torch.bmm(x, x.transpose(1, 2))) / 2
        return torch.bincount(d[:, iu[0], iu[1]].reshape(-1).long(), minlength=n + 1)

    ts, by_torch = timed(torch_self)
    t_torch = report("the same by torch, float32", ts, f"{M} x {C} rows x {4 * n} B   {float(np.median(ts)) / t_packed:.1f} x the packed call")
    print(f"  {'':26s} the two give the same histogram: {bool(torch.equal(by_torch, hist))}  (pairs {int(hist.sum())}, "
          f"sum of d {int((hist * torch.arange(n + 1, device='cuda')).sum())})")
    RA, RB = ([tuple(int(v) for v in a.split("=")[1].split("x")) for a in sys.argv if a.startswith("novelty=")] + [(1024, 60000)])[0]
    g = torch.Generator(device="cuda").manual_seed(seed % 2 ** 31)
    # rows round two centres, as codes of one data set are: the distances spread and the nearest row is not at n / 2
    flip = lambda rows, p: torch.where(torch.rand((rows, n), device="cuda", generator=g) < p, -1.0, 1.0)  # noqa: E731
    centre = flip(2, 0.5)
    xa = centre[torch.arange(RA, device="cuda") % 2] * flip(RA, 0.2)
    xb = centre[torch.arange(RB, device="cuda") % 2] * flip(RB, 0.2)
    a, b = smp.pack_spins(xa), smp.pack_spins(xb)
    near = torch.empty((RA,), dtype=torch.int64, device="cuda")

    def packed_cross():
        _lib.check(_lib.lib().dvg_packed_overlap(a.data_ptr(), RA, W, 0, b.data_ptr(), RB, W, 0, 1, n, hist.data_ptr(), near.data_ptr(), 0,
                                                 _lib.stream_ptr()), "dvg_packed_overlap")
        return hist

    ts, _ = timed(packed_cross)
    t_packed = report("novelty, packed rows", ts, f"{RA} x {RB} rows x {4 * W} B, with nearest")

    def torch_cross():
        d = (n - xa @ xb.T) / 2
        return torch.bincount(d.reshape(-1).long(), minlength=n + 1), d.min(1)

    ts, (by_torch, (dmin, _at)) = timed(torch_cross)
    report("the same by torch, float32", ts, f"{RA} x {RB} rows x {4 * n} B   {float(np.median(ts)) / t_packed:.1f} x the packed call")
    d = (n - xa @ xb.T) / 2
    first = torch.where(d == dmin[:, None], torch.arange(RB, device="cuda")[None, :], RB).min(1).values  # the smallest row at d_min
    same = bool(torch.equal(by_torch, hist)) and bool(torch.equal(near >> 32, dmin.long())) and bool(torch.equal(near & 0xFFFFFFFF, first))
    print(f"  {'':26s} the two give the same histogram and nearest rows: {same}  (pairs {int(hist.sum())}, "
          f"sum of nearest d {int((near >> 32).sum())})")
if "energy" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    trace = s.sample_trace(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)  # burn_in 0, thin 1: chains x sweeps records
    W, M = (n + 31) // 32, sweeps
    rows = C * M
    energy = torch.empty((rows,), dtype=torch.float64, device="cuda")

    def report(name, ts, what):
        t = float(np.median(ts))
        print(f"  {name:26s} {t:9.1f} us per call  {what}  (min {min(ts):.1f} max {max(ts):.1f})")
        return t

    def packed():
        _lib.check(_lib.lib().dvg_grbm_energy_packed(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0,
                                                     trace.bits.data_ptr(), M, W, C, M * W, energy.data_ptr(), _lib.stream_ptr()),
                   "dvg_grbm_energy_packed")
        return energy

    ts, _ = timed(packed)
    t_packed = report("energy, packed rows", ts, f"{C} x {M} rows x {4 * W} B, {n} + {plan.n_edges} terms a row")
    hs, Js = (0.05 * lin).clamp(-4.0, 4.0), (0.05 * quad).clamp(-1.0, 1.0)  # (float32: one rounding each, as the kernel's)
    e32 = torch.empty((rows,), dtype=torch.float32, device="cuda")

    def stock(x):
        _lib.check(_lib.lib().dvg_grbm_energy(s.graph.ptr, x.data_ptr(), rows, hs.data_ptr(), Js.data_ptr(), e32.data_ptr(),
                                              _lib.stream_ptr()), "dvg_grbm_energy")
        return e32

    ts, _ = timed(lambda: stock(smp.unpack_spins(trace.bits.view(rows, W), n).contiguous()))
    t_stock = report("unpack + float32 energy", ts, f"{rows} rows x {4 * n} B   {float(np.median(ts)) / t_packed:.1f} x the packed call")
    x = smp.unpack_spins(trace.bits.view(rows, W), n).contiguous()
    ts, _ = timed(lambda: stock(x))
    report("float32 energy alone", ts, f"the unpacking not timed   {float(np.median(ts)) / t_packed:.1f} x the packed call")
    dev = (e32.double() - energy).abs()
    print(f"  {'':26s} float32 energies off by up to {float(dev.max()):.3e}, 2^-23 |E| up to {float(energy.abs().max()) * 2.0 ** -23:.3e}  "
          f"(sum of energies {float(energy.sum()):.6e})")
if "correlation" in sys.argv:
    from image_generation_amd import functional as F

    def time_of(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            call()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 5 * 1e3

    def report(name, ts, what):
        t = float(np.median(ts))
        print(f"  {name:34s} {t:9.1f} us per call  {what}  (min {min(ts):.1f} max {max(ts):.1f})")
        return t

    for nc, Cc, Mc in ((512, 256, 200), (1024, 256, 200), (1024, 32, 32)):
        mgc, _ = graphs.get_graph_mapping(graphs.greedy_get_subgraph(nc, seed, graphs.zephyr_graph(12)))
        nodes_c, eic, ejc = graphs.edges_of(mgc)
        plan_c = graphs.build_plan(nc, eic, ejc)
        rc = np.random.default_rng(1)
        lin_c = torch.from_numpy((0.05 * rc.uniform(-1, 1, nc)).astype(np.float32)).cuda()
        quad_c = torch.from_numpy((5.0 * rc.uniform(-1, 1, plan_c.n_edges)).astype(np.float32)).cuda()
        sc = smp.GibbsSampler(plan_c, nodes_c, beta=20.0, sweeps=Mc, seed=seed, persistent=True)
        bits = sc.sample_trace(lin_c, quad_c, 0.05, (-4, 4), (-1, 1), num_reads=Cc).bits  # burn_in 0, thin 1: (chains, sweeps, W)
        Wc, rows = (nc + 31) // 32, Cc * Mc
        spin_sum = torch.empty((nc,), dtype=torch.int64, device="cuda")
        pair_sum = torch.empty((nc, nc), dtype=torch.int64, device="cuda")
        ws = torch.empty((int(_lib.lib().dvg_packed_correlation_workspace_bytes(Mc, Cc, nc)),), dtype=torch.uint8, device="cuda")

        def packed():
            _lib.check(_lib.lib().dvg_packed_correlation(bits.data_ptr(), Mc, Wc, Cc, Mc * Wc, nc, spin_sum.data_ptr(), pair_sum.data_ptr(), 0,
                                                         ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "dvg_packed_correlation")

        def stock():
            x = smp.unpack_spins(bits.view(rows, Wc), nc).float()
            return x.T @ x

        x_kept = smp.unpack_spins(bits.view(rows, Wc), nc).float()
        calls = (packed, lambda: F.packed_correlation(bits, n=nc), stock, lambda: x_kept.T @ x_kept)
        for call in calls:
            call()
        torch.cuda.synchronize()
        ts = [[] for _ in calls]
        for _ in range(5):  # the paths alternate
            for k, call in enumerate(calls):
                ts[k].append(time_of(call))
        print(f" correlation: {rows} rows ({Cc} chains x {Mc} records) of {nc} spins, {4 * Wc} B a row packed, {4 * nc} B unpacked")
        t_packed = report("dvg_packed_correlation", ts[0], f"{nc} x {nc} sums, workspace {ws.numel()} B")
        report("functional.packed_correlation", ts[1], f"allocating per call   {float(np.median(ts[1])) / t_packed:.2f} x the raw entry")
        t_stock = report("unpack_spins + float32 x.T @ x", ts[2], f"{float(np.median(ts[2])) / t_packed:.2f} x the raw entry")
        report("float32 x.T @ x alone", ts[3], f"the unpacking not timed   {float(np.median(ts[3])) / t_packed:.2f} x the raw entry")
        by_torch = stock()
        same = bool(torch.equal(by_torch.long(), pair_sum)) and bool(torch.equal(x_kept.sum(0).long(), spin_sum))
        print(f"  {'':34s} the two paths give the same integers: {same}  (sum of pair sums {int(pair_sum.sum())}, of spin sums "
              f"{int(spin_sum.sum())}); not slower than the stock path with its unpack: {t_packed <= t_stock}")
if "fields" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    trace = s.sample_trace(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)  # burn_in 0, thin 1: chains x sweeps records
    W, M, E, beta = (n + 31) // 32, sweeps, plan.n_edges, 1.0
    rows = C * M
    log_pl = torch.empty((rows,), dtype=torch.float64, device="cuda")
    unstable = torch.empty((rows,), dtype=torch.int32, device="cuda")
    cond_sum, cond_pair = torch.empty((n,), dtype=torch.float64, device="cuda"), torch.empty((E,), dtype=torch.float64, device="cuda")
    ws = torch.empty((_lib.lib().dvg_grbm_fields_packed_workspace_bytes(s.graph.ptr, M, C),), dtype=torch.uint8, device="cuda")

    def report(name, ts, what):
        t = float(np.median(ts))
        print(f"  {name:26s} {t:9.1f} us per call  {what}  (min {min(ts):.1f} max {max(ts):.1f})")
        return t

    def packed(want_cond=True):
        _lib.check(_lib.lib().dvg_grbm_fields_packed(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0, beta,
                                                     trace.bits.data_ptr(), M, W, C, M * W, log_pl.data_ptr(), unstable.data_ptr(),
                                                     cond_sum.data_ptr() if want_cond else None, cond_pair.data_ptr() if want_cond else None,
                                                     None, 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "dvg_grbm_fields_packed")
        return log_pl

    ts, _ = timed(packed)
    t_packed = report("fields, packed rows", ts, f"{C} x {M} rows x {4 * W} B, {n} spins + {2 * E} CSR entries a row")
    ts, _ = timed(lambda: packed(False))
    report("  without the pooled sums", ts, "log_pl and unstable only")
    hs, Js = (0.05 * lin).clamp(-4.0, 4.0), (0.05 * quad).clamp(-1.0, 1.0)  # (float32: one rounding each, as the kernel's)
    ei_t, ej_t = torch.from_numpy(np.asarray(plan.edge_i, np.int64)).cuda(), torch.from_numpy(np.asarray(plan.edge_j, np.int64)).cuda()
    Jd = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    Jd[ei_t, ej_t] = Js
    Jd = Jd + Jd.T

    def stock(x):
        f = x @ Jd + hs
        z = (2.0 * beta * f).clamp(-87.0, 87.0).double()
        xd = x.double()
        lp = -torch.nn.functional.softplus(xd * z).sum(1)
        m = -torch.tanh(0.5 * z)
        un = ((x * f) > 0).sum(1, dtype=torch.int32)
        return lp, un, m.sum(0), (m[:, ei_t] * xd[:, ej_t] + m[:, ej_t] * xd[:, ei_t]).sum(0)

    ts, _ = timed(lambda: stock(smp.unpack_spins(trace.bits.view(rows, W), n).contiguous())[0])
    report("unpack + torch", ts, f"{rows} rows x {4 * n} B   {float(np.median(ts)) / t_packed:.1f} x the packed call")
    x = smp.unpack_spins(trace.bits.view(rows, W), n).contiguous()
    ts, _ = timed(lambda: stock(x)[0])
    report("torch alone", ts, f"the unpacking not timed   {float(np.median(ts)) / t_packed:.1f} x the packed call")
    packed()
    lp, un, cs, cp = stock(x)
    print(f"  {'':26s} stock path off by up to {float((lp - log_pl).abs().max()):.3e} in log_pl (|log_pl| up to {float(log_pl.abs().max()):.4g}), "
          f"{int((un != unstable).sum())} of {rows} unstable counts, {float((cs - cond_sum).abs().max()):.3e} in cond_sum, "
          f"{float((cp - cond_pair).abs().max()) if E else 0.0:.3e} in cond_pair  (mean log_pl {float(log_pl.mean()):.6f}, "
          f"local minima {float((unstable == 0).double().mean()):.4f})")
if "descend" in sys.argv:
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    trace = s.sample_trace(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)  # burn_in 0, thin 1: chains x sweeps records
    W, M, cap = (n + 31) // 32, sweeps, 1000
    rows = C * M
    noise = torch.from_numpy(np.random.default_rng(2).integers(0, 2 ** 32, size=(rows, W), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    out = torch.empty((rows, W), dtype=torch.int32, device="cuda")
    n_sweeps, n_flips, left = (torch.empty((rows,), dtype=torch.int32, device="cuda") for _ in range(3))

    def report(name, ts, what):
        t = float(np.median(ts))
        print(f"  {name:26s} {t:9.1f} us per call  {what}  (min {min(ts):.1f} max {max(ts):.1f})")
        return t

    hs, Js = (0.05 * lin).clamp(-4.0, 4.0), (0.05 * quad).clamp(-1.0, 1.0)  # (float32: one rounding each, as the kernel's)
    ei_t, ej_t = torch.from_numpy(np.asarray(plan.edge_i, np.int64)).cuda(), torch.from_numpy(np.asarray(plan.edge_j, np.int64)).cuda()
    Jd = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    Jd[ei_t, ej_t] = Js
    Jd = Jd + Jd.T
    classes = [torch.from_numpy(np.asarray(plan.order[plan.class_ptr[k]:plan.class_ptr[k + 1]], np.int64)).cuda() for k in range(plan.n_colours)]
    Jc, hc = [Jd[:, c].contiguous() for c in classes], [hs[c] for c in classes]

    def stock(bits):
        x = smp.unpack_spins(bits, n)
        for _ in range(cap):
            moved = torch.zeros((), dtype=torch.bool, device="cuda")
            for c, J_c, h_c in zip(classes, Jc, hc):
                xc = x[:, c]
                flip = (xc * (x @ J_c + h_c)) > 0
                x[:, c] = torch.where(flip, -xc, xc)
                moved |= flip.any()
            if not bool(moved):
                break
        return smp.pack_spins(x)

    for kind, bits in (("trace", trace.bits.view(rows, W)), ("random", noise)):
        def packed():
            _lib.check(_lib.lib().dvg_grbm_descend_packed(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0,
                                                          bits.data_ptr(), rows, W, 1, 0, cap, out.data_ptr(), n_sweeps.data_ptr(),
                                                          n_flips.data_ptr(), left.data_ptr(), _lib.stream_ptr()), "dvg_grbm_descend_packed")
            return out

        ts, _ = timed(packed)
        t_packed = report(f"descend, {kind} rows", ts, f"{rows} rows x {4 * W} B, {n} spins + {2 * plan.n_edges} CSR entries a row and sweep")
        ts, by_torch = timed(lambda: stock(bits))
        t_stock = report("unpack + torch + pack", ts, f"{rows} rows x {4 * n} B   {float(np.median(ts)) / t_packed:.1f} x the packed call")
        packed()
        print(f"  {'':26s} the two paths return equal rows: {bool(torch.equal(by_torch, out))} ({int((by_torch != out).any(1).sum())} of {rows} "
              f"differ); sweeps up to {int(n_sweeps.max())} (mean {float(n_sweeps.double().mean()):.2f}), flips a row {float(n_flips.double().mean()):.1f}, "
              f"{int((left > 0).sum())} rows cut off, {int(torch.unique(out, dim=0).shape[0])} distinct minima; not slower than the stock path: "
              f"{t_packed <= t_stock}")
if "population" in sys.argv:
    def report(name, ts, what):
        t = float(np.median(ts))
        print(f"  {name:30s} {t:9.1f} us  {what}  (min {min(ts):.1f} max {max(ts):.1f})")
        return t

    shapes = ([a.split("=")[1] for a in sys.argv if a.startswith("resample=")] + ["8x128,1x65536"])[0]
    for P, R in (tuple(int(v) for v in item.split("x")) for item in shapes.split(",")):
        Cr = P * R
        lw = torch.from_numpy(np.random.default_rng(Cr).normal(0.0, 3.0, Cr)).cuda()
        state = torch.where(torch.rand((Cr, n), device="cuda") < 0.5, -1, 1).to(torch.int8)
        other, parents = torch.empty_like(state), torch.empty((Cr,), dtype=torch.int32, device="cuda")
        ws = torch.empty((int(_lib.lib().dvg_population_resample_workspace_bytes(Cr)),), dtype=torch.uint8, device="cuda")

        def by_hip():
            _lib.check(_lib.lib().dvg_population_resample(lw.data_ptr(), Cr, P, 0, seed, 7, state.data_ptr(), other.data_ptr(), n, None,
                                                          None, parents.data_ptr(), None, ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                       "dvg_population_resample")
            return parents

        offset = torch.rand((P, 1), dtype=torch.float64, device="cuda")
        j = torch.arange(R, dtype=torch.float64, device="cuda")[None, :]
        first = (torch.arange(P, device="cuda") * R)[:, None]

        def by_torch():
            w = torch.exp(lw.view(P, R) - lw.view(P, R).max(1, keepdim=True).values)
            S = torch.cumsum(w, 1)
            at = (j + offset) * (S[:, -1:] / R)
            par = (torch.searchsorted(S, at, right=True).clamp_(max=R - 1) + first).view(-1)
            return par, torch.index_select(state, 0, par)

        ts, _ = timed(by_hip)
        t_hip = report(f"resample {P} x {R}, HIP", ts, f"{Cr} chains x {n} B")
        ts, (par, _rows) = timed(by_torch)
        report(f"resample {P} x {R}, torch", ts, f"{float(np.median(ts)) / t_hip:.1f} x the HIP call")
        # the same offset through both: V / K of the HIP call is not exported, so only the shape of the result is compared
        kids_hip = torch.bincount(parents.long(), minlength=Cr)
        kids_torch = torch.bincount(par.long(), minlength=Cr)
        print(f"  {'':30s} children per chain differ by at most {int((kids_hip - kids_torch).abs().max())} (other offsets); "
              f"gathered rows equal their parents': {bool(torch.equal(other, state[parents.long()]))}")

    betas = np.linspace(0.0, 20.0, sweeps + 1)[1:].astype(np.float32)
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    ts, pop = timed(lambda: s.sample_population(lin, quad, 0.05, (-4, 4), (-1, 1), betas, num_reads=C, num_populations=8).samples)
    t_pop = report("population draw", ts, f"{C} chains, 8 populations, {sweeps} steps of one sweep")
    table = torch.from_numpy(betas).cuda()
    state = torch.empty((C, n), dtype=torch.int8, device="cuda")
    other, parents = torch.empty_like(state), torch.empty((C,), dtype=torch.int32, device="cuda")
    log_w = torch.empty((C,), dtype=torch.float64, device="cuda")
    ws = torch.empty((int(_lib.lib().dvg_population_resample_workspace_bytes(C)),), dtype=torch.uint8, device="cuda")

    def ais(first, count, init):
        _lib.check(_lib.lib().dvg_gibbs_sample_ais(s.graph.ptr, lin.data_ptr(), quad.data_ptr(), 0.05, -4.0, 4.0, -1.0, 1.0,
                                                   table.data_ptr() + 4 * first, 0, float(betas[first - 1]) if first else 0.0,
                                                   state.data_ptr(), C, 0, seed, first, count, init, None, log_w.data_ptr(), None, None,
                                                   _lib.stream_ptr()), "dvg_gibbs_sample_ais")

    def one_call():
        ais(0, sweeps, 1)
        return log_w

    def per_step():
        for t in range(sweeps):
            ais(t, 1, int(t == 0))
        return log_w

    def resamples():
        for t in range(sweeps):
            _lib.check(_lib.lib().dvg_population_resample(log_w.data_ptr(), C, 8, 0, seed, t + 1, state.data_ptr(), other.data_ptr(), n,
                                                          None, None, parents.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                                          _lib.stream_ptr()), "dvg_population_resample")
        return parents

    ts, _ = timed(one_call)
    t_one = report("one AIS call", ts, f"{C} chains, {sweeps} sweeps")
    ts, _ = timed(per_step)
    t_steps = report("an AIS call per step", ts, f"{(float(np.median(ts)) - t_one) / sweeps:.2f} us per step beyond the one call")
    ts, _ = timed(resamples)
    t_res = report("the resample calls alone", ts, f"{float(np.median(ts)) / sweeps:.2f} us per step")
    over = (t_pop - t_one) / sweeps
    print(f"  {'':30s} per-step overhead of the population draw {over:.2f} us: AIS call per step {(t_steps - t_one) / sweeps:.2f}, "
          f"resample {t_res / sweeps:.2f} ({100 * t_res / sweeps / over:.0f} %), log Z and ess by torch "
          f"{over - (t_steps - t_one + t_res) / sweeps:.2f}")

    K = max([int(a.split("=")[1]) for a in sys.argv if a.startswith("seeds=")] + [4])
    print(f"  std_err of log Z at beta 20, {C} chains, {sweeps} sweeps, {K} seeds:")
    for k in range(K):
        sk = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed + k, persistent=True)
        pa = sk.sample_population(lin, quad, 0.05, (-4, 4), (-1, 1), betas, num_reads=C, num_populations=8)
        lp = sk.log_partition(lin, quad, 0.05, (-4, 4), (-1, 1), num_sweeps=sweeps, num_reads=C)
        groups = torch.logsumexp(lp.log_weights.view(8, -1), 1)
        z = torch.exp(groups - groups.max())
        print(f"    seed + {k}: population log_z {float(pa.log_z):.4f} std_err {float(pa.std_err):.4f} (survivors "
              f"{int(pa.survivors.min())} .. {int(pa.survivors.max())} of {C // 8}, worst step ess {float(pa.ess.min()):.1f});  AIS log_z "
              f"{float(lp.log_z):.4f} std_err by ess {float(lp.std_err):.4f} (ess {float(lp.ess):.1f}), between 8 groups "
              f"{float(z.std(unbiased=True) / z.mean() / 8 ** 0.5):.4f}")
if "distinct" in sys.argv:
    # dvg_packed_distinct ("DVG distinct v1") against torch.unique(dim=0, return_inverse=True, return_counts=True) on the same
    # device rows: 65 536 rows of n = 256 and 16 384 rows of n = 1024, all rows distinct and rows drawn from a pool of 256 states
    def report(name, ts, what):
        t = float(np.median(ts))
        print(f"  {name:34s} {t:9.1f} us per call  {what}  (min {min(ts):.1f} max {max(ts):.1f})")
        return t

    g = torch.Generator(device="cuda").manual_seed(seed % 2 ** 31)
    for Td, nd in ((65536, 256), (16384, 1024)):
        Wd = nd // 32
        fresh = torch.randint(-2 ** 31, 2 ** 31, (Td, Wd), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
        pooled = fresh[:256][torch.randint(0, 256, (Td,), device="cuda", generator=g)].contiguous()
        for what, rows_d in (("all rows distinct", fresh), ("a pool of 256 states", pooled)):
            first, ident, rep = (torch.empty((Td,), dtype=torch.int32, device="cuda") for _ in range(3))
            count = torch.empty((Td,), dtype=torch.int64, device="cuda")
            n_distinct = torch.empty((1,), dtype=torch.int64, device="cuda")
            ws = torch.empty((int(_lib.lib().dvg_packed_distinct_workspace_bytes(Td, 1, nd)),), dtype=torch.uint8, device="cuda")

            def entry():
                _lib.check(_lib.lib().dvg_packed_distinct(rows_d.data_ptr(), Td, Wd, 1, 0, nd, None, 0, 0, first.data_ptr(), ident.data_ptr(),
                                                          rep.data_ptr(), count.data_ptr(), n_distinct.data_ptr(), None, None, ws.data_ptr(),
                                                          ws.numel(), _lib.stream_ptr()), "dvg_packed_distinct")
                return count

            ts, _ = timed(entry)
            t_entry = report(f"distinct, {Td} x n={nd}", ts, what)
            ts, (u_rows, u_inverse, u_counts) = timed(lambda: torch.unique(rows_d, dim=0, return_inverse=True, return_counts=True))
            report("the same by torch.unique(dim=0)", ts, f"{float(np.median(ts)) / t_entry:.2f} x the entry")
            D = int(n_distinct.item())
            same = D == int(u_rows.shape[0]) and sorted(count[:D].tolist()) == sorted(u_counts.tolist()) and \
                bool(torch.equal(rows_d[rep[:D].long()][ident.long()], u_rows[u_inverse]))
            print(f"  {'':34s} the two give the same classes: {same}  (D = {D})")
if "link" in sys.argv:
    # dvg_packed_bonds ("DVG bonds v1") and dvg_packed_overlap_link ("DVG link overlap v1") on the thin = 1 trace, in self mode at
    # equal times, against the stock torch path on the same rows: unpack to float32, gather the bonds, two batched matmuls,
    # bincount and index_add
    s = smp.GibbsSampler(plan, nodes, beta=20.0, sweeps=sweeps, seed=seed, persistent=True)
    trace = s.sample_trace(lin, quad, 0.05, (-4, 4), (-1, 1), num_reads=C)  # burn_in 0, thin 1: chains x sweeps records
    E, W, M = plan.n_edges, (n + 31) // 32, sweeps
    WE = (E + 31) // 32
    bonds = torch.empty((C, M, WE), dtype=torch.int32, device="cuda")
    sums = [torch.empty((k + 1,), dtype=torch.int64, device="cuda") for k in (n, E, n, n)]

    def report(name, ts, what):
        t = float(np.median(ts))
        print(f"  {name:34s} {t:9.1f} us per call  {what}  (min {min(ts):.1f} max {max(ts):.1f})")
        return t

    def packed_bonds():
        _lib.check(_lib.lib().dvg_packed_bonds(s.graph.ptr, None, trace.bits.data_ptr(), M, W, C, M * W, bonds.data_ptr(), _lib.stream_ptr()),
                   "dvg_packed_bonds")
        return bonds

    def packed_link():
        _lib.check(_lib.lib().dvg_packed_overlap_link(trace.bits.data_ptr(), bonds.data_ptr(), C, M * W, W, M * WE, WE, None, None, 0, 0, 0, 0,
                                                      0, M, n, E, *(t.data_ptr() for t in sums), 0, _lib.stream_ptr()),
                   "dvg_packed_overlap_link")
        return sums[0]

    ts, _ = timed(packed_bonds)
    t_bonds = report("bonds, packed trace", ts, f"{C} x {M} rows x {4 * W} B -> {4 * WE} B, E = {E}")
    ts, _ = timed(packed_link)
    pairs = M * C * (C - 1) // 2
    t_link = report("link overlap, packed trace", ts, f"{M} groups x {C} rows x {4 * (W + WE)} B, {pairs} pairs, "
                    f"{pairs * (W + WE) / float(np.median(ts)) / 1e3:.1f} G popcounts/s")
    ei_d, ej_d = torch.from_numpy(plan.edge_i).cuda(), torch.from_numpy(plan.edge_j).cuda()
    iu = torch.triu_indices(C, C, 1, device="cuda")

    def stock():
        x = smp.unpack_spins(trace.bits, n).transpose(0, 1).contiguous()  # (M, C, n) float32
        t = x[:, :, ei_d] * x[:, :, ej_d]                                   # (M, C, E)
        d = ((n - torch.bmm(x, x.transpose(1, 2))) / 2)[:, iu[0], iu[1]].reshape(-1).long()
        l = ((E - torch.bmm(t, t.transpose(1, 2))) / 2)[:, iu[0], iu[1]].reshape(-1).long()
        zero = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
        return (torch.bincount(d, minlength=n + 1), torch.bincount(l, minlength=E + 1), zero.index_add(0, d, l),
                zero.index_add(0, d, l * l))

    ts, by_torch = timed(stock)
    t_stock = report("the same by torch, float32", ts, f"{M} x {C} rows x {4 * (n + E)} B   {float(np.median(ts)) / (t_bonds + t_link):.1f} x the two entries")
    same = all(bool(torch.equal(a, b)) for a, b in zip(by_torch, sums))
    print(f"  {'':34s} the two give the same four sums: {same}; not slower than the stock path: {t_bonds + t_link <= t_stock}  "
          f"(pairs {int(sums[0].sum())}, sum of l {int(sums[2].sum())}, of l^2 {int(sums[3].sum())})")
    lo = smp.LinkOverlap.from_sums(*sums, n, E)
    a_fit, b_fit = lo.fit()
    print(f"  {'':34s} mean q_l {float(lo.mean_link):.4f}, spin q2 {float(lo.spin.q2):.4f}, corr(q^2, q_l) {float(lo.corr_q2_link):.4f}, "
          f"fit q_l = {float(a_fit):.4f} + {float(b_fit):.4f} q^2")
