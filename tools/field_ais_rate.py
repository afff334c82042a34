"""What weighing costs the per-chain-field draw: ``dvg_gibbs_sample_fields`` beside ``dvg_gibbs_sample_fields_ais`` without and
with a table of field strengths, on the same chains, in one run.

    python tools/field_ais_rate.py [--n 512] [--chains 2048] [--sweeps 100] [--repeats 9] [--warmup 3]

The project's Zephyr subgraph (``get_sampler_and_sampler_kwargs``, MI355X_gibbs_zephyr) at n spins; h = 0.2 U(-1, 1), J = U(-1, 1),
prefactor 1, the solver's ranges, N(0, 1) fields, a row per chain.  ``fields``: ``sample_fields``, S sweeps at the sampler's beta.
``weighed``: ``sample_fields_ais`` with a constant beta table and no strengths -- the energy and the weight carried, the rows
untouched.  ``ramped``: the same with ``scales = linspace(0, 1, S + 1)[1:]`` -- every lane recomputes its row entries at the head
of every sweep.  All three from the same given start states; the tables are on the device before the clock starts.  After
``warmup`` draws of each, ``repeats`` draws of each are timed with device events, the three alternating; the median, the fastest
and the slowest are reported (the spread), rates from the median.  Needs the GPU: there is no fallback.  Reported, not gated."""
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
    ap.add_argument("--chains", type=int, default=2048)
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch

    from image_generation_amd import _lib, dev, sampler as smp

    if not torch.cuda.is_available():
        raise SystemExit("field_ais_rate: no GPU; a rate is measured on the MI355X or not at all")
    s, _kw, _g, h_range, j_range = smp.get_sampler_and_sampler_kwargs(1, 1.0, a.n, 0, "MI355X_gibbs_zephyr", sweeps=a.sweeps, beta=2.0)
    plan = s.plan
    rng = np.random.default_rng(1)
    lin = torch.from_numpy((0.2 * rng.uniform(-1, 1, plan.n)).astype(np.float32)).cuda()
    quad = torch.from_numpy(rng.uniform(-1, 1, plan.n_edges).astype(np.float32)).cuda()
    C, S = a.chains, a.sweeps
    fields = torch.from_numpy(rng.standard_normal((C, plan.n)).astype(np.float32)).cuda()
    start = torch.from_numpy(np.where(rng.uniform(size=(C, plan.n)) < 0.5, -1, 1).astype(np.int8)).cuda()
    betas = torch.full((S,), s.beta, dtype=torch.float32, device="cuda")
    scales = torch.from_numpy(np.linspace(0.0, 1.0, S + 1)[1:].astype(np.float32)).cuda()

    def plain():
        return s.sample_fields(lin, quad, 1.0, h_range, j_range, fields, start=start, sweeps=S)

    def weighed():
        return s.sample_fields_ais(lin, quad, 1.0, h_range, j_range, fields, betas, None, start=start, beta_from=s.beta)

    def ramped():
        return s.sample_fields_ais(lin, quad, 1.0, h_range, j_range, fields, betas, scales, start=start, beta_from=s.beta, scale_from=0.0)

    draws = (("fields", plain), ("weighed", weighed), ("ramped", ramped))
    for _ in range(a.warmup):
        for _name, f in draws:
            f()
    torch.cuda.synchronize()
    ms = {name: [] for name, _f in draws}
    for _ in range(a.repeats):
        for name, f in draws:  # (alternating: all three see the same machine)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1))
    work = float(C) * plan.n * S
    out = dict(n=plan.n, colours=int(plan.n_colours), chains=C, sweeps=S, repeats=a.repeats, plan=dev.gibbs_draw_plan(plan, C, "field_weigh"),
               source_hash=_lib.lib().dvg_source_hash().decode())
    for name, _f in draws:
        med = statistics.median(ms[name])
        out[name] = dict(ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]), updates_per_second=work / (med * 1e-3))
        print(f"{name:8s} {C} x n={plan.n} x {S} sweeps: median {med:.3f} ms (min {min(ms[name]):.3f}, max {max(ms[name]):.3f}) "
              f"-> {out[name]['updates_per_second']:.4g} spin updates / s")
    out["weighed_over_fields_time"] = out["weighed"]["ms_median"] / out["fields"]["ms_median"]
    out["ramped_over_fields_time"] = out["ramped"]["ms_median"] / out["fields"]["ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
