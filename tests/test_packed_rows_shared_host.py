"""CPU-side checks of what the strided packed-row entries share (csrc/packed_rows.h, ``functional._packed_rows``): the same
bad row layout meets the same answer at ``dvg_grbm_energy_packed``, ``dvg_grbm_fields_packed``, ``dvg_grbm_descend_packed``
and ``dvg_packed_correlation`` -- the same code, a message that starts with the entry's own name and names the offending
argument -- on host stand-in pointers, before any HIP call; and at their four Python wrappers, before the library is
touched."""
import ctypes
import re

import numpy as np
import pytest
import torch

import support
from image_generation_amd import _lib, functional as F, graphs

ENTRIES = ("grbm_energy_packed", "grbm_fields_packed", "grbm_descend_packed", "packed_correlation")
W = 2  # n = 64: two words a row

# (layout, the arguments it changes, the code, what the message must name); DVG_E_INVALID = -1, DVG_E_UNSUPPORTED = -4
C_LAYOUTS = (
    ("rows 0", dict(rows=0), -1, (rb"\brows=0\b",)),
    ("groups 0", dict(groups=0), -1, (rb"\bgroups=0\b",)),
    ("row_stride W - 1", dict(row_stride=W - 1), -1, (rb"\brow_stride=1\b",)),
    ("group_stride -1", dict(groups=3, group_stride=-1), -1, (rb"\bgroup_stride=-1\b",)),
    # (dense, so that an entry with an output over its input gets as far as the count)
    ("groups x rows = 2^62", dict(rows=2 ** 31, groups=2 ** 31, group_stride=W * 2 ** 31), -4, (rb"\bgroups=", rb"\brows=", rb"2\^62")),
    ("n = 8193", dict(n=8193, row_stride=257), -4, (rb"\bn=8193\b", rb"8192")),
)


def _c_call(entry, *, n=64, rows=5, row_stride=W, groups=1, group_stride=0):
    """The entry on host stand-ins for its pointers (a graph handle's first fields are n, n_edges); nothing reads the rest."""
    L = _lib.lib()
    graph, _g, base, _keep = support.graph_stand_in(n)
    g, lin, quad, bits, out, ws = (ctypes.c_void_p(v) for v in (ctypes.addressof(graph), base, base + 64, base + 8192, base + 32768, base + 49152))
    model = (g, lin, quad, 1.0, -4.0, 4.0, -1.0, 1.0)
    geometry = (bits, rows, row_stride, groups, group_stride)
    if entry == "grbm_energy_packed":
        rc = L.dvg_grbm_energy_packed(*model, *geometry, out, None)
    elif entry == "grbm_fields_packed":
        rc = L.dvg_grbm_fields_packed(*model, 1.0, *geometry, out, None, None, None, None, 0, None, 0, None)
    elif entry == "grbm_descend_packed":  # in place: the one meeting of input and output the entry permits
        rc = L.dvg_grbm_descend_packed(*model, *geometry, 10, bits, None, None, None, None)
    else:
        rc = L.dvg_packed_correlation(*geometry, n, None, out, 0, ws, 1 << 62, None)
    return rc, L.dvg_last_error()


@pytest.mark.parametrize("layout,kw,code,words", C_LAYOUTS, ids=[c[0] for c in C_LAYOUTS])
def test_c_entries_agree_on_a_bad_row_layout(layout, kw, code, words):
    _lib.build()
    answers = {entry: _c_call(entry, **kw) for entry in ENTRIES}
    assert {rc for rc, _msg in answers.values()} == {code}, (layout, answers)
    for entry, (_rc, msg) in answers.items():
        assert msg.startswith(entry.encode() + b": "), (layout, entry, msg)
        for word in words:
            assert re.search(word, msg), (layout, entry, word, msg)
    # and beyond the name the entries say the same -- but for the reason behind the limit on n, which is each entry's own
    tails = {msg[len(entry):].split(b" (")[0] for entry, (_rc, msg) in answers.items()}
    assert len(tails) == 1, (layout, answers)


class _Handle:  # (what a wrapper reads before the library: the plan)
    def __init__(self, plan):
        self.plan, self.ptr = plan, None


def _wrappers():
    n = 77  # three words
    ei = np.arange(n - 1, dtype=np.int64)
    gh = _Handle(graphs.build_plan(n, ei, ei + 1))
    lin, quad = torch.zeros(n), torch.zeros(n - 1)
    return {
        "grbm_energy_packed": lambda b: F.grbm_energy_packed(b, gh, lin, quad),
        "grbm_fields_packed": lambda b: F.grbm_fields_packed(b, gh, lin, quad, beta=1.0),
        "grbm_descend_packed": lambda b: F.grbm_descend_packed(b, gh, lin, quad),
        "packed_correlation": lambda b: F.packed_correlation(b, n=n),
    }


def _zeros(*shape):
    return torch.zeros(shape, dtype=torch.int32)


# (layout, the tensor, how the message starts: the argument first); what a tensor's shape and strides can express
PY_LAYOUTS = (
    ("rows 0", lambda: _zeros(0, 3), "bits must"),
    ("rows 0 of a trace", lambda: _zeros(4, 0, 3), "bits must"),
    ("groups 0", lambda: _zeros(0, 6, 3), "bits must"),
    ("the wrong W: too few", lambda: _zeros(5, 2), "bits must"),
    ("the wrong W: too many", lambda: _zeros(4, 6, 4), "bits must"),
    ("a non-unit last stride", lambda: _zeros(5, 6)[:, ::2], "bits: the last dimension"),
    ("a non-unit last stride of a trace", lambda: _zeros(4, 6, 6)[:, :, ::2], "bits: the last dimension"),
    ("row_stride 0 < W", lambda: _zeros(1, 3).expand(5, 3), "bits: a row stride"),
    ("row_stride 2 < W", lambda: torch.as_strided(_zeros(16), (5, 3), (2, 1)), "bits: a row stride"),
    ("row_stride 0 < W of a trace", lambda: _zeros(4, 1, 3).expand(4, 6, 3), "bits: a row stride"),
)


@pytest.mark.parametrize("layout,make,start", PY_LAYOUTS, ids=[c[0] for c in PY_LAYOUTS])
def test_python_wrappers_agree_on_a_bad_row_layout(layout, make, start, monkeypatch):
    support.out_of_reach(monkeypatch, F)
    messages = set()
    for entry, call in _wrappers().items():
        with pytest.raises(_lib.DvgError) as err:
            call(make())
        assert str(err.value).startswith(start), (layout, entry, str(err.value))
        messages.add(str(err.value))
    assert len(messages) == 1, (layout, messages)


def test_python_wrappers_agree_on_good_row_layouts(monkeypatch):
    """Every layout the entries take -- rows, a slice of rows, a trace, slices of a trace along either dimension, a broadcast
    group -- gets past the early checks of all four and stops at the device check."""
    monkeypatch.setattr(F, "lib", lambda: pytest.fail("the library was touched on CPU tensors"))
    flat, trace = _zeros(5, 3), _zeros(4, 6, 3)
    for ok in (flat, flat[::2], flat[:1], trace, trace[:, 1:], trace[:2, ::2], trace[:1].expand(3, 6, 3)):
        for entry, call in _wrappers().items():
            with pytest.raises(_lib.DvgError, match="GPU"):
                call(ok)
