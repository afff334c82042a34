"""Prints what the Gibbs draw plan (csrc/gibbs_plan.h) decides: one line per (graph, chains, kind, gibbs_generic) of the
grid below -- the form, its template parameters, workgroups, threads per workgroup and LDS bytes.  Needs no GPU.

The grid is the one tests/test_gibbs_plan_host.py pins: the graphs of the GPU Gibbs tests (same constructions, same
seeds), chain counts on both sides of every threshold, the four draw kinds, and the option values the GPU tests use on
each graph.  A change that is meant to leave the plan alone is checked by running this against both builds
(DVG_LIBRARY=... selects a library) and comparing the two outputs line for line, or against the kernel-trace rows of
tools/gibbs_plan_trace.py (profiles/r09_gibbs_trace_parent.txt); profiles/r09_gibbs_plan_sweep.txt holds the output.

    python tools/gibbs_plan_sweep.py > sweep.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from image_generation_amd import _lib, graphs  # noqa: E402

SEED = 775321899904
KINDS = ("plain", "held", "table", "weigh")
# (graph, chain counts, gibbs_generic values)
GRID = (
    ("pegasus64", (5,), (0,)),
    ("zephyr128", (5, 1024, 1025), (0,)),
    ("zephyr512", (9,), (0, 1, 2)),
    ("zephyr1024", (41, 512, 513), (0, 1, 3, 4)),
    ("pegasus1024", (513,), (0,)),
    ("random77", (19,), (0,)),
    ("random700", (45,), (0,)),
    ("cliques50x14", (21,), (0,)),
)


def _solver(fam, n):
    g = graphs.pegasus_graph(16) if fam == "pegasus" else graphs.zephyr_graph(12)
    mg, _ = graphs.get_graph_mapping(graphs.greedy_get_subgraph(n, SEED, g))
    _nodes, ei, ej = graphs.edges_of(mg)
    return graphs.build_plan(n, ei, ej)


def _random(n, p_edge, isolated=None):
    rng = np.random.default_rng(n)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.uniform(size=iu.size) < p_edge
    if isolated is not None:
        keep &= (iu != isolated) & (ju != isolated)
    return graphs.build_plan(n, iu[keep].astype(np.int64), ju[keep].astype(np.int64))


def _cliques(m, k):
    ei, ej = [], []
    for c in range(m):
        for a in range(k):
            for b in range(a + 1, k):
                ei.append(c * k + a); ej.append(c * k + b)
    return graphs.build_plan(m * k, np.asarray(ei, np.int64), np.asarray(ej, np.int64))


def build_graph(name):
    """The host plan (graphs.GibbsPlan) of a grid graph, built as tests/test_gpu_gibbs.py builds it."""
    if name.startswith("pegasus") or name.startswith("zephyr"):
        fam = "pegasus" if name.startswith("pegasus") else "zephyr"
        return _solver(fam, int(name[len(fam):]))
    return {"random77": lambda: _random(77, 0.35, isolated=3), "random700": lambda: _random(700, 0.02),
            "cliques50x14": lambda: _cliques(50, 14)}[name]()


def rows():
    """(graph, chains, kind, gibbs_generic) in the order both tools walk them"""
    for name, chains, options in GRID:
        for c in chains:
            for option in options:
                for kind in KINDS:
                    yield name, c, kind, option


def format_plan(p):
    params = " ".join(f"{k}={int(v)}" for k, v in p["params"].items())
    return f"{p['form']} {params} | workgroups {p['workgroups']} threads {p['threads']} lds {p['lds_bytes']}"


def main():
    from image_generation_amd import dev

    plans = {}
    print("# graph chains kind gibbs_generic | form and its template parameters | workgroups, threads per workgroup, LDS bytes")
    for name, c, kind, option in rows():
        if name not in plans:
            plans[name] = build_graph(name)
        with _lib.option_scope(gibbs_generic=option):
            print(f"{name} {c} {kind} {option} | {format_plan(dev.gibbs_draw_plan(plans[name], c, kind))}")


if __name__ == "__main__":
    main()
