"""What a Trotter slice costs: the site-update rate of the simulated-quantum-annealing draw beside the spin-update rate of the
annealed draw on as many classical chains, in one run.

    python tools/quantum_rate.py [--n 512] [--slices 32] [--chains 1024] [--sweeps 100] [--repeats 9] [--warmup 3]

The project's Zephyr subgraph (``get_sampler_and_sampler_kwargs``, MI355X_gibbs_zephyr) at n spins; h = 0.2 U(-1, 1), J = U(-1, 1),
prefactor 1, the solver's ranges.  ``sample_quantum``: C chains x P slices, S sweeps down a linear transverse-field schedule
(Gamma 3 -> 0.05 at beta 2) -- C P n S site updates a draw.  ``sample_annealed``: C P fresh chains, S sweeps along a geometric beta
schedule -- C P n S spin updates a draw.  Both tables are on the device before the clock starts.  After ``warmup`` draws of each,
``repeats`` draws of each are timed with device events, the two alternating; the median, the fastest and the slowest are
reported (the spread), rates from the median.  Needs the GPU: there is no fallback.  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--slices", type=int, default=32)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch

    from image_generation_amd import _lib, sampler as smp

    if not torch.cuda.is_available():
        raise SystemExit("quantum_rate: no GPU; a rate is measured on the MI355X or not at all")
    s, _kw, _g, h_range, j_range = smp.get_sampler_and_sampler_kwargs(1, 1.0, a.n, 0, "MI355X_gibbs_zephyr", sweeps=a.sweeps, beta=2.0)
    plan = s.plan
    rng = np.random.default_rng(1)
    lin = torch.from_numpy((0.2 * rng.uniform(-1, 1, plan.n)).astype(np.float32)).cuda()
    quad = torch.from_numpy(rng.uniform(-1, 1, plan.n_edges).astype(np.float32)).cuda()
    C, P, S = a.chains, a.slices, a.sweeps
    bs, kp = (torch.from_numpy(t).cuda() for t in smp.transverse_schedule(s.beta, 3.0, 0.05, S, P))
    betas = torch.from_numpy(smp.beta_schedule(0.1, s.beta, S)).cuda()

    def quantum():
        return s.sample_quantum(lin, quad, 1.0, h_range, j_range, bs, kp, slices=P, num_reads=C)

    def annealed():
        return s.sample_annealed(lin, quad, 1.0, h_range, j_range, betas, num_reads=C * P)

    draws = (("quantum", quantum), ("annealed", annealed))
    for _ in range(a.warmup):
        for _name, f in draws:
            f()
    torch.cuda.synchronize()
    ms = {name: [] for name, _f in draws}
    for _ in range(a.repeats):
        for name, f in draws:  # (alternating: both see the same machine)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1))
    work = float(C) * P * plan.n * S
    out = dict(n=plan.n, colours=int(plan.n_colours), chains=C, slices=P, sweeps=S, repeats=a.repeats,
               source_hash=_lib.lib().dvg_source_hash().decode())
    for name, _f in draws:
        med = statistics.median(ms[name])
        out[name] = dict(ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]), updates_per_second=work / (med * 1e-3))
        print(f"{name:9s} {C} x {P} x n={plan.n} x {S} sweeps: median {med:.3f} ms (min {min(ms[name]):.3f}, max {max(ms[name]):.3f}) "
              f"-> {out[name]['updates_per_second']:.4g} {'site' if name == 'quantum' else 'spin'} updates / s")
    out["quantum_over_annealed_time"] = out["quantum"]["ms_median"] / out["annealed"]["ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
