"""Scaffolding the per-feature tests share: the graph plans they draw on, a host-memory stand-in for a graph handle, the
patch that puts the library out of reach, and the check that a feature's symbols are declared, bound and exported."""
import ctypes
import functools
import os
import re

import numpy as np

from image_generation_amd import _lib, graphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 775321899904


# ------------------------------------------------------------------ graph plans
# Every builder is cached on its normalised arguments: a graph is built once per test session and must not be modified.

@functools.lru_cache(maxsize=None)
def ring_plan(n=12):
    ei, ej = np.arange(n, dtype=np.int64), (np.arange(n, dtype=np.int64) + 1) % n
    return graphs.build_plan(n, np.minimum(ei, ej), np.maximum(ei, ej))


@functools.lru_cache(maxsize=None)
def _solver_plan(fam, n, seed):
    g = graphs.pegasus_graph(16) if fam == "pegasus" else graphs.zephyr_graph(12)
    mg, _ = graphs.get_graph_mapping(graphs.greedy_get_subgraph(n, seed, g))
    nodes, ei, ej = graphs.edges_of(mg)
    return graphs.build_plan(n, ei, ej), nodes


def solver_plan(fam, n, seed=SEED, with_nodes=False):
    """An n-spin subgraph of a solver topology (``"pegasus"`` or ``"zephyr"``); ``with_nodes``: ``(plan, nodes)``."""
    plan, nodes = _solver_plan(fam, n, seed)
    return (plan, nodes) if with_nodes else plan


@functools.lru_cache(maxsize=None)
def clique_plan(k=14, m=50):
    """m disjoint k-cliques: k colour classes of m spins each."""
    ei, ej = [], []
    for c in range(m):
        for a in range(k):
            for b in range(a + 1, k):
                ei.append(c * k + a); ej.append(c * k + b)
    plan = graphs.build_plan(k * m, np.asarray(ei, np.int64), np.asarray(ej, np.int64))
    assert plan.n_colours == k and np.diff(plan.class_ptr).max() == m
    return plan


@functools.lru_cache(maxsize=None)
def _random_plan(n, p_edge, isolated, hub_degree, edges, seed):
    if edges is not None:  # exactly `edges` edges, a seeded choice among all pairs
        rng = np.random.default_rng(seed)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
        pick = [pairs[k] for k in rng.permutation(len(pairs))[:edges]]
        return graphs.build_plan(n, np.array([p[0] for p in pick], dtype=np.int64), np.array([p[1] for p in pick], dtype=np.int64))
    rng = np.random.default_rng(n)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.uniform(size=iu.size) < p_edge
    if isolated is not None:
        keep &= (iu != isolated) & (ju != isolated)
    if hub_degree:
        keep = (keep & (iu != 0)) | ((iu == 0) & (ju <= hub_degree))
    plan = graphs.build_plan(n, iu[keep].astype(np.int64), ju[keep].astype(np.int64))
    deg = np.diff(plan.adj_ptr)
    assert isolated is None or deg[isolated] == 0
    assert not hub_degree or deg[0] == hub_degree
    return plan


def random_plan(n=77, p_edge=0.35, *, isolated=None, hub_degree=0, edges=None, seed=None, max_degree_above=None,
                with_nodes=False):
    """An Erdos-Renyi graph on n spins drawn from ``default_rng(n)``; ``isolated``: that spin gets no edge; ``hub_degree``:
    spin 0 is joined to spins 1 .. hub_degree and to no other; ``edges`` with ``seed``: exactly that many edges instead, a
    choice of ``default_rng(seed)``.  ``max_degree_above``: the degree the graph's largest must exceed (20: two rounds of the
    sampler's neighbour sum).  ``with_nodes``: ``(plan, list(range(n)))``."""
    plan = _random_plan(n, None if edges is not None else p_edge, isolated, hub_degree, edges, seed)
    assert max_degree_above is None or np.diff(plan.adj_ptr).max() > max_degree_above
    return (plan, list(range(n))) if with_nodes else plan


# ------------------------------------------------------------------ the library at arm's length

def graph_stand_in(n=64, n_edges=0):
    """A host-memory stand-in for a graph handle (first fields: n, n_edges), for calls that must fail on their arguments
    before anything is read: ``(graph, its address, base, arena)`` with ``base`` the 16-byte aligned address of 64 KiB of
    host words that dummy pointers point into; nothing reads or writes them."""
    graph = ctypes.create_string_buffer(4096)
    (ctypes.c_int32 * 2).from_buffer(graph)[:] = [n, n_edges]
    arena = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.cast(arena, ctypes.c_void_p).value + 15) & ~15
    return graph, ctypes.cast(graph, ctypes.c_void_p), base, arena


def out_of_reach(monkeypatch, *modules):
    """Put the library out of reach of ``_lib`` and of every module given: any call into it fails the test."""
    def boom(*_a, **_k):
        raise AssertionError("the library was touched before the argument error was raised")

    for module in (_lib,) + modules:
        monkeypatch.setattr(module, "lib", boom)


def header_text():
    with open(os.path.join(ROOT, "include", "dvg.h")) as f:
        return f.read()


def prof_kernel_names():
    L = _lib.lib()
    return [L.dvg_prof_kernel_name(i).decode() for i in range(L.dvg_prof_num_kernels())]


def assert_declared_bound_exported(names, *, markers=(), kernels=(), arity=None):
    """Every name of ``names`` (a name, or a mapping name -> return type; ``int`` where a plain sequence is given) is declared
    in include/dvg.h with that return type, present in the binding table and exported by the built library; the header's
    text carries the version ``markers``; the profiler knows the ``kernels``; ``arity``: name -> argument count bound."""
    names = {names: "int"} if isinstance(names, str) else names if isinstance(names, dict) else dict.fromkeys(names, "int")
    text = header_text()
    for marker in markers:
        assert marker in text, f"{marker!r} is not in include/dvg.h"
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    _lib.build()
    for name, ret in names.items():
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", text), f"{name} is not declared in include/dvg.h"
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name), f"{name} is not exported by the built library"
    for name, count in (arity or {}).items():
        assert len(_lib.SIGNATURES[name][1]) == count
    assert set(kernels) <= set(prof_kernel_names())
