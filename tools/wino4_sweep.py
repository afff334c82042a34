#!/usr/bin/env python3
"""Where the F(4x4,3x3) kernel's time goes: launch time against the number of 4-channel chunks per tile block (Cin / 4) at
a fixed number of tile blocks per workgroup -- slope = time per chunk, intercept = time per tile block beside its chunks --
for both block shapes of the kernel side by side: 64 tiles x 32 output channels, and 32 tiles x 64 (dev option enc_wino4_mask,
bits 16-21; a chunk of either is the same 72 MFMAs per SIMD, so the figures compare directly).

    python tools/wino4_sweep.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import image_generation_amd  # noqa: E402,F401
from image_generation_amd import _lib, dev  # noqa: E402

MASK = _lib.get_option("enc_wino4_mask") & 0xFFFF


def timeit(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for side, B, Cout in ((16, 4096, 64), (8, 16384, 64), (4, 65536, 64), (16, 4096, 32)):
    L, M = side.bit_length() - 1, B * side * side
    nblk, ny = M // 1024, Cout // 32
    per_wg = nblk * ny / 256   # stages of 72 MFMAs per SIMD and chunk a workgroup runs, in either shape
    shapes = (("64x32", 0), ("32x64", 0x3F << 16)) if Cout % 64 == 0 else (("64x32", 0),)
    rows = {name: [] for name, _ in shapes}
    for Cin in (8, 32, 128, 256):
        x = torch.randn(M, Cin, device="cuda")
        w = torch.randn(Cout, Cin, 3, 3, device="cuda") / 30
        ts = {}
        for _ in range(2):   # (the shapes alternate)
            for name, bits in shapes:
                _lib.set_option("enc_wino4_mask", MASK | bits)
                ts[name] = min(ts.get(name, 1e30), timeit(lambda: dev.conv_wino4(x, w, 0, M, Cin, Cout, L)))
        _lib.set_option("enc_wino4_mask", MASK)
        for name, _ in shapes:
            rows[name].append((Cin // 4, ts[name]))
        del x
    for name, _ in shapes:
        (c0, t0), (c1, t1) = rows[name][-3], rows[name][-1]
        slope = (t1 - t0) / (c1 - c0) / per_wg
        print(f"side {side:2d} Cout {Cout:3d} block {name} stages per workgroup {per_wg:.0f}: " + "  ".join(f"{c} chunks {t:7.1f} us" for c, t in rows[name]) +
              f"   -> {slope:.2f} us per chunk (ideal 0.98 at 2.4 GHz), {(t0 / per_wg - c0 * slope):.1f} us per stage beside its chunks", flush=True)
