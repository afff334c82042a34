"""The Gibbs draw's plan (csrc/gibbs_plan.h) without a device: which kernel form a draw takes, its template parameters and
its launch, over the graphs of the GPU Gibbs tests -- and that the lane-major shapes a graph can be given and the list of
lane-major instantiations agree."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gibbs_plan_sweep as grid  # noqa: E402  (the graphs, built as the GPU tests build them, and the grid of rows)

from image_generation_amd import _lib, dev  # noqa: E402

# What every draw of the grid launches.  Transcribed from the behaviour of the commit BEFORE the draw got its plan, not from
# the code under test: profiles/r09_gibbs_trace_parent.txt -- that commit's kernel-trace rows (one trace per kind, one 1-sweep
# draw per row: kernel name with its template arguments, workgroups, workgroup size) and its dvg_gibbs_launch_info (plain
# kind: workgroups, threads, LDS bytes).  The trace reports static LDS only (0 for these kernels), so the LDS bytes of the
# other kinds are that commit's dvg_gibbs_launch_info for a plain row that launched the same instantiation on the same
# graph (LDS does not depend on kind or chain count: gibbs_kernel under gibbs_generic = 1, the others under 0 / 2 / 3), plus,
# for the held rolled rows, the flag words that commit's launch_gibbs adds: 4 x chains per workgroup x ceil(n / 32).
# A threshold edit that moves a row to another form has to change this table knowingly.
# (graph, chains, kind, gibbs_generic): form, its template parameters, workgroups, threads per workgroup, LDS bytes
_GIBBS_PLANS = {
    ("pegasus64", 5, "plain", 0): ("lane", dict(LPC=32, WAVES=1, MB=4, NR=1, MAXS=12), 3, 64, 12672),
    ("zephyr128", 5, "plain", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 1, 256, 21760),
    ("zephyr128", 1024, "plain", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 128, 256, 21760),
    ("zephyr128", 1025, "plain", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 129, 256, 21760),
    ("zephyr512", 9, "plain", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=12), 3, 256, 81408),
    ("zephyr512", 9, "plain", 1): ("rolled", dict(LPC=64, WAVES=4), 3, 256, 66096),
    ("zephyr512", 9, "plain", 2): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=1, MAXS=12), 3, 256, 81408),
    ("zephyr1024", 41, "plain", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 41, "plain", 1): ("rolled", dict(LPC=64, WAVES=16), 3, 1024, 159312),
    ("zephyr1024", 41, "plain", 3): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 41, "plain", 4): ("slots", dict(MAXS=18, CH=8, FIX=True), 6, 1024, 145408),
    ("zephyr1024", 512, "plain", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 512, "plain", 1): ("rolled", dict(LPC=64, WAVES=16), 32, 1024, 159312),
    ("zephyr1024", 512, "plain", 3): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 512, "plain", 4): ("slots", dict(MAXS=18, CH=8, FIX=True), 64, 1024, 145408),
    ("zephyr1024", 513, "plain", 0): ("slots", dict(MAXS=18, CH=16, FIX=True), 33, 1024, 161792),
    ("zephyr1024", 513, "plain", 1): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 159312),
    ("zephyr1024", 513, "plain", 3): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 129, 256, 146944),
    ("zephyr1024", 513, "plain", 4): ("slots", dict(MAXS=18, CH=8, FIX=True), 65, 1024, 145408),
    ("pegasus1024", 513, "plain", 0): ("slots", dict(MAXS=18, CH=16, FIX=True), 33, 1024, 161792),
    ("random77", 19, "plain", 0): ("rolled", dict(LPC=16, WAVES=1), 5, 64, 14196),
    ("random700", 45, "plain", 0): ("slots", dict(MAXS=18, CH=16, FIX=False), 3, 1024, 94624),
    ("cliques50x14", 21, "plain", 0): ("lane", dict(LPC=64, WAVES=4, MB=4, NR=1, MAXS=20), 6, 256, 92160),
    ("pegasus64", 5, "held", 0): ("lane", dict(LPC=32, WAVES=1, MB=4, NR=1, MAXS=12), 3, 64, 12672),
    ("zephyr128", 5, "held", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 1, 256, 21760),
    ("zephyr128", 1024, "held", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 128, 256, 21760),
    ("zephyr128", 1025, "held", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 129, 256, 21760),
    ("zephyr512", 9, "held", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=12), 3, 256, 81408),
    ("zephyr512", 9, "held", 1): ("rolled", dict(LPC=64, WAVES=4), 3, 256, 66352),
    ("zephyr512", 9, "held", 2): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=1, MAXS=12), 3, 256, 81408),
    ("zephyr1024", 41, "held", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 41, "held", 1): ("rolled", dict(LPC=64, WAVES=16), 3, 1024, 161360),
    ("zephyr1024", 41, "held", 3): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 41, "held", 4): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 512, "held", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 512, "held", 1): ("rolled", dict(LPC=64, WAVES=16), 32, 1024, 161360),
    ("zephyr1024", 512, "held", 3): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 512, "held", 4): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 513, "held", 0): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 161360),
    ("zephyr1024", 513, "held", 1): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 161360),
    ("zephyr1024", 513, "held", 3): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 161360),
    ("zephyr1024", 513, "held", 4): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 161360),
    ("pegasus1024", 513, "held", 0): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 138224),
    ("random77", 19, "held", 0): ("rolled", dict(LPC=16, WAVES=1), 5, 64, 14244),
    ("random700", 45, "held", 0): ("rolled", dict(LPC=64, WAVES=16), 3, 1024, 96032),
    ("cliques50x14", 21, "held", 0): ("lane", dict(LPC=64, WAVES=4, MB=4, NR=1, MAXS=20), 6, 256, 92160),
    ("pegasus64", 5, "table", 0): ("lane", dict(LPC=32, WAVES=1, MB=4, NR=1, MAXS=12), 3, 64, 12672),
    ("zephyr128", 5, "table", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 1, 256, 21760),
    ("zephyr128", 1024, "table", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 128, 256, 21760),
    ("zephyr128", 1025, "table", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 129, 256, 21760),
    ("zephyr512", 9, "table", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=12), 3, 256, 81408),
    ("zephyr512", 9, "table", 1): ("rolled", dict(LPC=64, WAVES=4), 3, 256, 66096),
    ("zephyr512", 9, "table", 2): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=1, MAXS=12), 3, 256, 81408),
    ("zephyr1024", 41, "table", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 41, "table", 1): ("rolled", dict(LPC=64, WAVES=16), 3, 1024, 159312),
    ("zephyr1024", 41, "table", 3): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 41, "table", 4): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 512, "table", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 512, "table", 1): ("rolled", dict(LPC=64, WAVES=16), 32, 1024, 159312),
    ("zephyr1024", 512, "table", 3): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 512, "table", 4): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 513, "table", 0): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 159312),
    ("zephyr1024", 513, "table", 1): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 159312),
    ("zephyr1024", 513, "table", 3): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 159312),
    ("zephyr1024", 513, "table", 4): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 159312),
    ("pegasus1024", 513, "table", 0): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 136176),
    ("random77", 19, "table", 0): ("rolled", dict(LPC=16, WAVES=1), 5, 64, 14196),
    ("random700", 45, "table", 0): ("rolled", dict(LPC=64, WAVES=16), 3, 1024, 94624),
    ("cliques50x14", 21, "table", 0): ("lane", dict(LPC=64, WAVES=4, MB=4, NR=1, MAXS=20), 6, 256, 92160),
    ("pegasus64", 5, "weigh", 0): ("lane", dict(LPC=32, WAVES=1, MB=4, NR=1, MAXS=12), 3, 64, 12672),
    ("zephyr128", 5, "weigh", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 1, 256, 21760),
    ("zephyr128", 1024, "weigh", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 128, 256, 21760),
    ("zephyr128", 1025, "weigh", 0): ("lane", dict(LPC=32, WAVES=4, MB=5, NR=1, MAXS=12), 129, 256, 21760),
    ("zephyr512", 9, "weigh", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=12), 3, 256, 81408),
    ("zephyr512", 9, "weigh", 1): ("rolled", dict(LPC=64, WAVES=4), 3, 256, 66096),
    ("zephyr512", 9, "weigh", 2): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=1, MAXS=12), 3, 256, 81408),
    ("zephyr1024", 41, "weigh", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 41, "weigh", 1): ("rolled", dict(LPC=64, WAVES=16), 3, 1024, 159312),
    ("zephyr1024", 41, "weigh", 3): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 41, "weigh", 4): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 11, 256, 146944),
    ("zephyr1024", 512, "weigh", 0): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 512, "weigh", 1): ("rolled", dict(LPC=64, WAVES=16), 32, 1024, 159312),
    ("zephyr1024", 512, "weigh", 3): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 512, "weigh", 4): ("lane", dict(LPC=64, WAVES=4, MB=5, NR=2, MAXS=20), 128, 256, 146944),
    ("zephyr1024", 513, "weigh", 0): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 159312),
    ("zephyr1024", 513, "weigh", 1): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 159312),
    ("zephyr1024", 513, "weigh", 3): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 159312),
    ("zephyr1024", 513, "weigh", 4): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 159312),
    ("pegasus1024", 513, "weigh", 0): ("rolled", dict(LPC=64, WAVES=16), 33, 1024, 136176),
    ("random77", 19, "weigh", 0): ("rolled", dict(LPC=16, WAVES=1), 5, 64, 14196),
    ("random700", 45, "weigh", 0): ("rolled", dict(LPC=64, WAVES=16), 3, 1024, 94624),
    ("cliques50x14", 21, "weigh", 0): ("lane", dict(LPC=64, WAVES=4, MB=4, NR=1, MAXS=20), 6, 256, 92160),
}


@pytest.fixture(scope="module")
def graphs_of_the_grid():
    return {name: grid.build_graph(name) for name, _chains, _options in grid.GRID}


def test_the_pinned_table_covers_the_grid():
    assert sorted(_GIBBS_PLANS) == sorted(grid.rows())


@pytest.mark.parametrize("name,chains,options", grid.GRID)
def test_draws_take_the_pinned_kernel_forms(graphs_of_the_grid, name, chains, options):
    _lib.check(_lib.lib().dvg_reset_options(), "dvg_reset_options")
    plan = graphs_of_the_grid[name]
    for c in chains:
        for option in options:
            with _lib.option_scope(gibbs_generic=option):
                for kind in grid.KINDS:
                    form, params, workgroups, threads, lds = _GIBBS_PLANS[(name, c, kind, option)]
                    p = dev.gibbs_draw_plan(plan, c, kind)
                    where = (name, c, kind, option, p)
                    assert (p["form"], p["params"]) == (form, params), where
                    assert (p["workgroups"], p["threads"], p["lds_bytes"]) == (workgroups, threads, lds), where
                    assert p["workgroups"] == -(-c // p["chains_per_workgroup"]), where
                # the held rolled form: the flag words, one bit per spin and a row per chain of the workgroup, are in the LDS
                held, table = dev.gibbs_draw_plan(plan, c, "held"), dev.gibbs_draw_plan(plan, c, "table")
                if held["form"] == "rolled":
                    assert table["form"] == "rolled" and table["params"] == held["params"]
                    assert held["lds_bytes"] == table["lds_bytes"] + 4 * held["chains_per_workgroup"] * ((plan.n + 31) // 32)
                else:
                    assert held["lds_bytes"] == table["lds_bytes"]


# ---------------------------------------------------------------------------------------------- lane shapes and instantiations
def _synthetic(sizes, degree):
    """A graph shape of these colour-class sizes whose first spin has `degree` neighbours (the draw's plan reads class sizes
    and row lengths only: a shape, not a colourable graph)."""
    n = int(sum(sizes))
    adj_ptr = np.full(n + 1, degree, dtype=np.int32)
    adj_ptr[0] = 0
    return types.SimpleNamespace(n=n, n_colours=len(sizes), class_ptr=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                                 adj_ptr=adj_ptr)


def _class_size_vectors():
    """Class-size vectors whose lane images cover every (lanes per chain, rows per step, rows) the rule can give."""
    for lpc, top in ((16, 16), (32, 32), (64, 64)):  # one pass per class: one row per step
        for classes in range(1, 22):
            yield [top] + [max(1, top // 2)] * (classes - 1)
    for steps in range(1, 12):  # 64 lanes, classes of two to four passes: two rows per step
        yield [65] * steps
        yield [128] + [65] * (steps - 1)
        if steps >= 2:
            yield [256] + [100] * (steps - 2)
            yield [193] + [1] * (steps - 2)


# lane images the lane-major form does not serve at default options, by the reading of the commit before the plan
# (has_kernel: two rows per step need four-wave workgroups; the one-wave rule takes graphs of at most 16 KiB of tables and 12
# rows at up to 1024 chains): they take the rolled form.  (LPC, MB, NR, rows) at up to 1024 chains
_ROLLED_LANE_SHAPES = {(64, 4, 2, 2), (64, 5, 2, 2)}


def test_every_lane_shape_a_graph_can_get_has_an_instantiation():
    _lib.check(_lib.lib().dvg_reset_options(), "dvg_reset_options")
    seen = set()
    for sizes in _class_size_vectors():
        for degree in (0, 16, 17, 20, 21):
            g = _synthetic(sizes, degree)
            for chains in (1, 512, 513, 1024, 1025):
                p = dev.gibbs_draw_plan(g, chains)
                image = p["lane_image"]
                if image is None:  # beyond the caps: more rows than the widest instantiation walks, or more than 20 neighbours
                    lpc = 16 if max(sizes) <= 16 else 32 if max(sizes) <= 32 else 64
                    nr = 2 if max(sizes) > 64 else 1
                    rows = sum(nr * -(-(-(-s // lpc)) // nr) for s in sizes)
                    assert degree > 20 or rows > (20 if lpc == 64 else 12), (sizes, degree)
                    assert p["form"] in ("rolled", "slots"), (sizes, degree, chains, p)
                    continue
                shape = (image["LPC"], image["MB"], image["NR"], image["rows"])
                seen.add(shape)
                assert image["LPC"] in (16, 32, 64) and image["MB"] == (4 if degree <= 16 else 5) and image["NR"] in (1, 2)
                assert 1 <= image["rows"] <= (20 if image["LPC"] == 64 else 12)
                if image["rows"] > 12 and chains > 512:  # (the 12-row / 512-chain rule, not a missing kernel)
                    assert p["form"] in ("rolled", "slots"), (shape, chains, p)
                elif shape in _ROLLED_LANE_SHAPES and chains <= 1024:
                    assert p["form"] == "rolled", (shape, chains, p)
                else:
                    assert p["form"] == "lane", (shape, chains, p)
                    assert (p["params"]["LPC"], p["params"]["MB"], p["params"]["NR"]) == shape[:3]
                    assert p["params"]["MAXS"] >= image["rows"]
                    assert p["lds_bytes"] <= 160 * 1024
    # the enumeration reached every shape the rule can give
    want = {(lpc, mb, 1, rows) for lpc in (16, 32) for mb in (4, 5) for rows in range(1, 13)}
    want |= {(64, mb, 1, rows) for mb in (4, 5) for rows in range(1, 21)}
    want |= {(64, mb, 2, rows) for mb in (4, 5) for rows in range(2, 21, 2)}
    assert seen == want


def test_a_lane_image_beyond_the_lds_takes_the_rolled_form():
    """20 rows of 5 batches at more than 1216 spins: 150 KiB of tables and four state rows are over 160 KiB."""
    g = _synthetic([250] * 5, 20)
    p = dev.gibbs_draw_plan(g, 9)
    assert p["lane_image"] == dict(LPC=64, MB=5, NR=2, rows=20) and p["form"] == "rolled", p
    assert dev.gibbs_draw_plan(_synthetic([240] * 5, 20), 9)["form"] == "lane"
