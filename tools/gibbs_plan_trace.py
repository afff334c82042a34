"""The kernels the Gibbs draws actually launch over the grid of tools/gibbs_plan_sweep.py, from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/gibbs_plan_trace.py run KIND
    python tools/gibbs_plan_trace.py rows KIND OUT/.../*_kernel_trace.csv

`run` does one 1-sweep draw of KIND (plain, held, table, weigh) per grid row on the GPU, in grid order, and nothing else
from the sampler; for the plain kind it also prints dvg_gibbs_launch_info of each row (which launches nothing).  `rows`
pairs the trace's Gibbs dispatches, in order, with the grid rows and prints one line per row: kernel name with its
template arguments, workgroups, workgroup size, LDS bytes as the trace reports them.  One trace per kind, each in a run
of its own.  profiles/r09_gibbs_trace_parent.txt holds the output at the commit before the draw got its plan: the source
of the table in tests/test_gibbs_plan_host.py.
"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gibbs_plan_sweep as grid  # noqa: E402


def run(kind):
    import numpy as np
    import torch

    from image_generation_amd import _lib, sampler as smp

    plans = {}
    for name, c, k, option in grid.rows():
        if k != kind:
            continue
        if name not in plans:
            plans[name] = grid.build_graph(name)
        plan = plans[name]
        rng = np.random.default_rng(1)
        lin = torch.from_numpy((0.05 * rng.uniform(-1, 1, plan.n)).astype(np.float32)).cuda()
        quad = torch.from_numpy((1.0 * rng.uniform(-1, 1, plan.n_edges)).astype(np.float32)).cuda()
        with _lib.option_scope(gibbs_generic=option):
            s = smp.GibbsSampler(plan, list(range(plan.n)), beta=1.0, sweeps=1, seed=grid.SEED, persistent=True)
            info = ""
            if kind == "plain":
                s.sample_native(lin, quad, 1.0, (-4, 4), (-1, 1), num_reads=c)
                i = s.launch_info(c)
                info = f" | launch_info workgroups {i['workgroups']} threads {i['threads']} lds {i['lds_bytes']}"
            elif kind == "held":
                start = torch.ones((c, plan.n), dtype=torch.int8, device="cuda")
                clamp = torch.zeros((c, plan.n), dtype=torch.uint8, device="cuda")
                clamp[:, ::3] = 1
                s.sample_conditional(lin, quad, 1.0, (-4, 4), (-1, 1), start, clamp, sweeps=1)
            elif kind == "table":
                s.sample_annealed(lin, quad, 1.0, (-4, 4), (-1, 1), [1.0], num_reads=c)
            else:
                s.sample_ais(lin, quad, 1.0, (-4, 4), (-1, 1), [1.0], num_reads=c)
            torch.cuda.synchronize()
        print(f"{name} {c} {kind} {option}{info}", flush=True)


def rows(kind, path):
    with open(path) as f:
        trace = [r for r in csv.DictReader(f) if "gibbs" in r["Kernel_Name"]]
    trace.sort(key=lambda r: int(r["Start_Timestamp"]))
    want = [r for r in grid.rows() if r[2] == kind]
    assert len(trace) == len(want), (len(trace), len(want))
    for (name, c, k, option), r in zip(want, trace):
        kernel = r["Kernel_Name"].replace("void dvg::", "").replace("dvg::", "")
        kernel = kernel.split("(")[0]
        wg = int(r["Workgroup_Size_X"])
        print(f"{name} {c} {k} {option} | {kernel} | workgroups {int(r['Grid_Size_X']) // wg} threads {wg} "
              f"lds {r['LDS_Block_Size']} scratch {r.get('Scratch_Size', '?')}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        rows(sys.argv[2], sys.argv[3])
