"""Prints what the MMD plan decides over a grid of shapes and options: dvg_mmd_workspace_bytes and the three outputs of
dvg_mmd_spin_flops, for every (nx, ny, d, mmd_w128, mmd_d256, mmd_gram_fp4) of the grid below; one line per shape, the option
combinations that agree sharing an entry.  Needs no GPU.

A change that is meant to leave the plan alone is checked by running this against both builds (DVG_LIBRARY=... selects
a library) and comparing the two outputs line for line; profiles/r08_mmd_plan_sweep.txt holds the output.

    python tools/mmd_plan_sweep.py > sweep.txt
"""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from image_generation_amd import _lib  # noqa: E402

NX = (2, 33, 97, 128, 300, 513, 1000, 2048, 2053, 4096, 32768, 65536)
NY = (2, 5, 77, 130, 256, 1000, 2048)
D = (32, 64, 96, 128, 160, 256, 384, 512, 544, 1024, 1056, 2048)
TRI = (-1, 0, 1)


def _ranges(ids):
    """[0, 1, 2, 5] -> '0-2,5'"""
    out, i = [], 0
    while i < len(ids):
        j = i
        while j + 1 < len(ids) and ids[j + 1] == ids[j] + 1:
            j += 1
        out.append(str(ids[i]) if i == j else f"{ids[i]}-{ids[j]}")
        i = j + 1
    return ",".join(out)


def main():
    L = _lib.lib()
    combos = list(itertools.product(TRI, TRI, (0, 1)))
    print("# One line per shape: nx ny d | <option combinations> : workspace_bytes int8_flops bf16_flops bf16_terms | ...")
    print("# Option combinations that give the same four numbers share an entry; combination k = (mmd_w128, mmd_d256, mmd_gram_fp4):")
    print("# " + "  ".join(f"{k}={c}" for k, c in enumerate(combos)))
    results = {}
    for k, (w128, d256, fp4) in enumerate(combos):
        with _lib.option_scope(mmd_w128=w128, mmd_d256=d256, mmd_gram_fp4=fp4):
            for shape in itertools.product(NX, NY, D):
                i8, b16, terms = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
                _lib.check(L.dvg_mmd_spin_flops(*shape, ctypes.byref(i8), ctypes.byref(b16), ctypes.byref(terms)),
                           "dvg_mmd_spin_flops")
                value = f"{L.dvg_mmd_workspace_bytes(*shape)} {i8.value:.0f} {b16.value:.0f} {terms.value}"
                results.setdefault(shape, {}).setdefault(value, []).append(k)
    for (nx, ny, d), groups in results.items():
        print(f"{nx} {ny} {d} | " + " | ".join(f"{_ranges(ids)} : {value}" for value, ids in groups.items()))


if __name__ == "__main__":
    main()
