"""What an isoenergetic cluster move costs and what it buys: the exchange draw with moves between twin ladders
(``sample_tempered_cluster``) beside the exchange draw alone (``sample_tempered``) on a +-J glass, in one run.

    python tools/cluster_rate.py [--n 512] [--chains 1024] [--replicas 16] [--beta-hot 0.05] [--beta-cold 1.0] [--sweeps 4000]
                                 [--burn 1000] [--thin 4] [--cluster-every 4] [--rung-from 0] [--repeats 21] [--cost-only]

The project's Zephyr subgraph (``get_sampler_and_sampler_kwargs``, MI355X_gibbs_zephyr) at n spins; h = 0, J = +-1 with equal odds,
prefactor 1, no clamp; Q = chains / replicas ladders (Q / 2 twin pairs) on a geometric ladder beta-hot .. beta-cold.

Cost.  From the state after ``burn`` sweeps of the exchange draw: one move over all rungs (``cluster_move``, rung_from = 0), timed
``repeats`` times with device events, move numbers 0, 1, ..; beside it one call of 100 sweeps of ``sample_tempered`` from the same
state, per sweep.  Median (fastest .. slowest).

Benefit.  Two draws from the same fresh chains, ``burn`` sweeps first, then ``sweeps`` sweeps in calls of ``thin`` sweeps that hand
``state`` and ``rungs`` on (``thin`` = ``cluster-every``: one move in front of each call), a record after each call: the rung
every row holds and the energies by rung.  From the records, with ``TemperedTrace``'s own rules: round trips per ladder, tau_int of
the target rung's energy (in sweeps), and its mean.  A move that exchanges all of D only renames the twins, and a walk or an
energy series read by row would take that for mixing.  So each is given twice: round trips BY CONFIGURATION (a move that exchanges
more than half of D is read as the two configurations changing rows) beside those by row, and tau_int of the twin pair's MEAN
target energy, which no move changes, beside that of each ladder's.  The first of each is the figure to judge by.  Needs the GPU:
there is no fallback.  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--beta-hot", type=float, default=0.05)
    ap.add_argument("--beta-cold", type=float, default=1.0)
    ap.add_argument("--sweeps", type=int, default=4000)
    ap.add_argument("--burn", type=int, default=1000)
    ap.add_argument("--thin", type=int, default=4)
    ap.add_argument("--cluster-every", type=int, default=4)
    ap.add_argument("--rung-from", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--cost-only", action="store_true")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from image_generation_amd import _lib, sampler as smp

    if not torch.cuda.is_available():
        raise SystemExit("cluster_rate: no GPU; a rate is measured on the MI355X or not at all")
    R, Q = a.replicas, a.chains // a.replicas
    if Q < 2 or Q % 2 or a.chains % a.replicas or a.sweeps % a.thin or a.burn % a.thin or a.thin != a.cluster_every:
        raise SystemExit("cluster_rate: chains = an even number of ladders x replicas; sweeps and burn multiples of thin = cluster-every")
    ladder = smp.beta_schedule(a.beta_hot, a.beta_cold, R)
    rng = np.random.default_rng(1)

    def sampler():
        s = smp.get_sampler_and_sampler_kwargs(1, 1.0, a.n, 0, "MI355X_gibbs_zephyr", sweeps=a.thin, beta=float(ladder[-1]))[0]
        return s

    s = sampler()
    plan = s.plan
    lin = torch.zeros(plan.n, dtype=torch.float32, device="cuda")
    quad = torch.from_numpy(rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=plan.n_edges)).cuda()
    out = dict(n=plan.n, edges=int(plan.n_edges), chains=Q * R, replicas=R, ladders=Q, betas=[float(b) for b in ladder], sweeps=a.sweeps,
               burn=a.burn, thin=a.thin, cluster_every=a.cluster_every, rung_from=a.rung_from, source_hash=_lib.lib().dvg_source_hash().decode())

    def timed(f):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r = f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1), r

    # ---- cost
    burnt = s.sample_tempered(lin, quad, 1.0, None, None, ladder, num_ladders=Q, num_sweeps=a.burn)
    state = burnt.state.clone()
    for k in range(3):
        s.cluster_move(state, burnt.rungs, replicas=R, move=1000 + k)
        s.sample_tempered(lin, quad, 1.0, None, None, ladder, num_ladders=Q, num_sweeps=100, start=state, rungs=burnt.rungs)
    move_ms, sweep_ms, last = [], [], None
    for k in range(a.repeats):  # (alternating: both see the same machine)
        ms, last = timed(lambda: s.cluster_move(state, burnt.rungs, replicas=R, move=k))
        move_ms.append(ms)
        ms, _r = timed(lambda: s.sample_tempered(lin, quad, 1.0, None, None, ladder, num_ladders=Q, num_sweeps=100, start=state,
                                                  rungs=burnt.rungs))
        sweep_ms.append(ms / 100.0)
    out["move_us"] = dict(median=1e3 * statistics.median(move_ms), min=1e3 * min(move_ms), max=1e3 * max(move_ms))
    out["sweep_us"] = dict(median=1e3 * statistics.median(sweep_ms), min=1e3 * min(sweep_ms), max=1e3 * max(sweep_ms))
    out["move_over_sweep"] = out["move_us"]["median"] / out["sweep_us"]["median"]
    out["mean_size_by_rung"] = [round(float(v), 2) for v in last.mean_size.cpu()]
    out["mean_differ_by_rung"] = [round(float(v), 2) for v in (last.differ.sum(0).double() / last.differ.shape[0]).cpu()]
    print(f"one move over {Q // 2} pairs x {R} rungs, n={plan.n}: median {out['move_us']['median']:.1f} us ({out['move_us']['min']:.1f} .. "
          f"{out['move_us']['max']:.1f}); one sweep of sample_tempered on the {Q * R} chains: {out['sweep_us']['median']:.1f} us "
          f"({out['sweep_us']['min']:.1f} .. {out['sweep_us']['max']:.1f}); a move costs {out['move_over_sweep']:.2f} sweeps")
    print(f"  after {a.burn} sweeps: differing sites by rung {out['mean_differ_by_rung']}")
    print(f"                      mean cluster by rung   {out['mean_size_by_rung']}")
    if a.cost_only:
        print(json.dumps(out))
        return out

    # ---- benefit
    def run(with_moves):
        s = sampler()
        kw = dict(num_ladders=Q, swap_every=1)
        if with_moves:
            kw.update(cluster_every=a.cluster_every, rung_from=a.rung_from)
        draw = s.sample_tempered_cluster if with_moves else s.sample_tempered
        res = draw(lin, quad, 1.0, None, None, ladder, num_sweeps=a.burn, **kw)
        walk, walk_of, energy, sizes, differ = [], [], [], [], []
        # whose configuration a row holds: a move that exchanges more than half of D is read as the two configurations
        # changing rows (the rest of D went the other way), so a configuration's walk survives a move that only renames
        who, base = torch.arange(Q * R, device="cuda"), (torch.arange(Q, device="cuda") * R)[:, None]
        for _ in range(a.sweeps // a.thin):
            t = res.tempered if with_moves else res
            holder = (torch.argsort(t.rungs.view(Q, R).long(), dim=1) + base).view(Q // 2, 2, R)  # [p, twin, r]: the row that holds r
            res = draw(lin, quad, 1.0, None, None, ladder, num_sweeps=a.thin, start=t.state, rungs=t.rungs, **kw)
            t = res.tempered if with_moves else res
            if with_moves:  # (one move, in front of the call's first sweep: thin = cluster_every)
                most = res.sizes[0] * 2 > res.differ[0]
                ra, rb = holder[:, 0][most], holder[:, 1][most]
                who[ra], who[rb] = who[rb].clone(), who[ra].clone()
                sizes.append(res.sizes.sum((0, 1)))
                differ.append(res.differ.sum((0, 1)))
            walk.append(t.rungs.view(Q, R).to(torch.uint8))
            by_configuration = torch.empty(Q * R, dtype=torch.uint8, device="cuda")
            by_configuration[who] = t.rungs.to(torch.uint8)
            walk_of.append(by_configuration.view(Q, R))
            energy.append(t.energies)
        sweeps = np.arange(1, a.sweeps // a.thin + 1, dtype=np.int64) * a.thin
        E = torch.stack(energy, dim=2)
        tt = smp.TemperedTrace(None, E, torch.stack(walk, dim=2), sweeps, None, ladder, plan.n)
        tc = smp.TemperedTrace(None, E, torch.stack(walk_of, dim=2), sweeps, None, ladder, plan.n)
        es = tt.energy_series(-1)
        pair = smp.EnergySeries.from_energies(E[:, -1].view(Q // 2, 2, -1).mean(1).contiguous(), a.thin)  # (a move leaves it as it is)
        r = dict(round_trips_per_ladder_by_row=float(tt.round_trips().sum()) / Q,
                 round_trips_per_ladder_by_configuration=float(tc.round_trips().sum()) / Q, tau_int_sweeps_by_ladder=float(es.tau_int_sweeps),
                 tau_int_sweeps_of_pair_mean=float(pair.tau_int_sweeps), tau_truncated=bool(es.truncated) or bool(pair.truncated),
                 mean_energy=float(es.mean), std_err=float(es.std_err), flow_by_configuration=[round(float(v), 3) for v in tc.flow().cpu()])
        if sizes:
            r["moved_share_by_rung"] = [round(float(v), 3) for v in (torch.stack(sizes).sum(0).double() / torch.stack(differ).sum(0).double()).cpu()]
        return r

    for name, with_moves in (("exchange", False), ("exchange+moves", True)):
        ms, out[name] = timed(lambda: run(with_moves))
        out[name]["wall_ms"] = ms
        r = out[name]
        print(f"{name:15s} {a.sweeps} sweeps behind {a.burn}: round trips / ladder {r['round_trips_per_ladder_by_configuration']:.3f} by "
              f"configuration ({r['round_trips_per_ladder_by_row']:.3f} by row); target energy tau_int {r['tau_int_sweeps_of_pair_mean']:.1f} sweeps "
              f"of the pair mean ({r['tau_int_sweeps_by_ladder']:.1f} by ladder){' (window hit max_lag: a lower bound)' if r['tau_truncated'] else ''}; "
              f"target mean energy {r['mean_energy']:.3f} +- {r['std_err']:.3f}")
        if "moved_share_by_rung" in r:
            print(f"{'':15s} exchanged / differing sites by rung {r['moved_share_by_rung']}")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
