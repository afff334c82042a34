"""SHA-256 of every output of the Winograd kernels on seeded inputs, for comparing two builds of the library bit for bit:

  DVG_LIBRARY=/path/to/other/libdvg.so timeout -k 10 300 python tools/wino_digests.py > a.txt \
      && timeout -k 10 300 python tools/wino_digests.py > b.txt && cmp a.txt b.txt

(each run a process of its own, under its own time limit; the second starts only if the first ended well).

The cases are the smallest at which each piece the four translation units share (csrc/conv_wino_common.h) can go wrong,
taken from the parametrisations of tests/test_gpu_kernels.py, tests/test_gpu_wino4_block64.py and tests/test_gpu_nets.py.
Every case runs twice in the process and the two runs must agree (the dynamic deal's re-zeroed counters)."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from image_generation_amd import _lib, dev  # noqa: E402

BLOCK64_BITS = 0x3F << 16


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def case(name, fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for k in sorted(a):
        assert torch.equal(a[k], b[k]), f"{name} {k}: two runs in one process differ"
        print(f"{name:60s} {k:12s} {tuple(a[k].shape)!s:18s} {sha(a[k])}")


def wino4(L, M, Cin, Cout, cus, mode, block64):
    side = 1 << L
    N = M // (side * side)
    assert dev.conv_wino4_shape(M, Cin, Cout, L)
    torch.manual_seed(1000 * L + M + Cin + mode)
    x = torch.randn(N, Cin, side, side)
    w = (torch.randn(Cout, Cin, 3, 3) / (3 * Cin**0.5) if mode == 0 else torch.randn(Cin, Cout, 3, 3) / (3 * Cout**0.5)).cuda()
    b = torch.randn(Cout).cuda() if mode == 0 else None
    xm = dev.nchw_to_morton(x).cuda()

    def run():
        saved = _lib.get_option("enc_wino4_mask")
        try:
            _lib.set_option("enc_wino4_mask", (saved & ~BLOCK64_BITS) | (BLOCK64_BITS if block64 else 0))
            r = dev.conv_wino4(xm, w, mode, M, Cin, Cout, L, bias=b, stats=(mode == 0), cus=cus)
        finally:
            _lib.set_option("enc_wino4_mask", saved)
        return dict(out=r[0], stats=r[1]) if mode == 0 else dict(out=r)
    case(f"wino4 L={L} M={M} {Cin}->{Cout} cus={cus} mode={mode} block64={int(block64)}", run)


def wino4_ups(N, Cin, Cout, side):
    L, M = side.bit_length() - 1, N * side * side
    assert dev.conv_wino4_shape(M, Cin, Cout, L) and dev.conv_wino4_shape(M, Cout, Cin, L)
    torch.manual_seed(N + Cin + side)
    xs = torch.randn(N, Cin, side // 2, side // 2)
    w = (torch.randn(Cin, Cout, 3, 3) / (3 * Cin**0.5)).cuda()
    b = torch.randn(Cout).cuda()
    gy = torch.randn(N, Cout, side, side)
    xm, gym = dev.nchw_to_morton(xs).cuda(), dev.nchw_to_morton(gy).cuda()

    def fwd():
        out, st = dev.conv_wino4(xm, w, 2, M, Cin, Cout, L, bias=b, stats=True, um=1)
        return dict(out=out, stats=st)
    case(f"wino4 um=1 N={N} {Cin}->{Cout} @{side}", fwd)
    case(f"wino4 um=2 N={N} {Cout}->{Cin} @{side}", lambda: dict(out=dev.conv_wino4(gym, w, 3, M, Cout, Cin, L, um=2)))


def wino2(N, Cin, Cout, side, dgrad=True):
    L, M = side.bit_length() - 1, N * side * side
    torch.manual_seed(N + Cin)
    x = torch.randn(N, Cin, side, side)
    w = (torch.randn(Cout, Cin, 3, 3) / (3 * Cin**0.5)).cuda()
    b = torch.randn(Cout).cuda()
    gy = torch.randn(N, Cout, side, side)
    xm, gym = dev.nchw_to_morton(x).cuda(), dev.nchw_to_morton(gy).cuda()
    with _lib.option_scope(enc_wino=1):
        assert dev.conv_wino_ok(M, Cin, Cout, L) and (not dgrad or dev.conv_wino_ok(M, Cout, Cin, L))

        def fwd():
            out, st = dev.conv_wino(xm, w, 0, M, Cin, Cout, L, bias=b, stats=True)
            return dict(out=out, stats=st)
        case(f"wino2 fwd N={N} {Cin}->{Cout} @{side}", fwd)
        if dgrad:
            case(f"wino2 dgrad N={N} {Cout}->{Cin} @{side}", lambda: dict(out=dev.conv_wino(gym, w, 1, M, Cout, Cin, L)))


def wgrad(which, N, Cin, Cout, side, ups=0, cus=0, one_slab=False):
    L, M = side.bit_length() - 1, N * side * side
    torch.manual_seed(N + Cin + side)
    gy = torch.randn(N, Cout, side, side)
    if ups:
        x, shape, mode = torch.randn(N, Cin, side // 2, side // 2), (Cin, Cout, 3, 3), 2
    else:
        x, shape, mode = torch.randn(N, Cin, side, side), (Cout, Cin, 3, 3), 0
    xm, gym = dev.nchw_to_morton(x).cuda(), dev.nchw_to_morton(gy).cuda()
    if which == 2:
        floats = _lib.lib().dvg_dev_wino_wgrad_slab_floats(M, Cin, Cout, L)  # (of the largest split any budget gives)
        assert floats > 0 and (not one_slab or floats == 16 * Cin * Cout)
        fn = lambda: dict(grad_w=dev.conv_wino_wgrad(xm, gym, mode, shape, M, Cin, Cout, L, ups=ups, cus=cus))  # noqa: E731
    else:
        assert _lib.lib().dvg_dev_wino4_wgrad_slab_floats(M, Cin, Cout, L) > 0
        fn = lambda: dict(grad_w=dev.conv_wino4_wgrad(xm, gym, 0, shape, M, Cin, Cout, L, cus=cus))  # noqa: E731
    case(f"wgrad F({which}x{which}) N={N} {Cin}->{Cout} @{side} ups={ups} cus={cus}", fn)


def decoder(n, B, R):
    """The F(2x2) kernels behind the upsample (no dev entry point): the decoder's forward and backward with option dec_wino = 1,
    through the calls of tests/test_gpu_nets.py::test_decoder_winograd_forms_match_oracle_full_gradients."""
    import gen
    from image_generation_amd.modules import Decoder

    params = gen.make_params(n, "decoder", 21 + n)
    spins = torch.from_numpy(gen.make_spins(B, R, n, 7))
    masks = [torch.from_numpy(m).cuda() for m in gen.make_masks(B * R, 8)]
    go = torch.randn(B, R, 1, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()

    def run():
        dec = Decoder(n)
        dec.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
        dec = dec.cuda().train()
        sg = spins.cuda().requires_grad_(True)
        dec.inject_dropout_masks(masks)
        got = dec(sg)
        (got * go).sum().backward()
        out = {"output": got, "grad_spins": sg.grad}
        out.update({"g." + k: p.grad for k, p in dec.named_parameters()})
        return out
    with _lib.option_scope(dec_wino=1):
        case(f"decoder dec_wino=1 n={n} B={B} R={R}", run)


def main():
    print(f"# library {_lib.LIB_PATH} source hash {_lib.lib().dvg_source_hash().decode()}", file=sys.stderr)
    # F(4x4) forward / data gradient, both block shapes: the cases of tests/test_gpu_wino4_block64.py ((2, 3072, 24, 128, cus=2):
    # three items on a one-wide grid -- the dynamic deal, the pending stores, an odd number of chunk pairs), and one
    # shape under the static deal: five blocks in one round, and in two rounds on a grid shrunk from 4 to 3 (64 x 32: budget 8)
    for L, M, Cin, Cout, cus in [(2, 1024, 8, 64, 0), (2, 3072, 24, 128, 2), (3, 2048, 16, 64, 0), (4, 2048, 8, 64, 0), (2, 5120, 16, 64, 0),
                                 (2, 5120, 16, 64, 8)]:
        for mode in (0, 1):
            for block64 in (False, True):
                wino4(L, M, Cin, Cout, cus, mode, block64)
    # ... behind the upsample (um = 1 and its data gradient um = 2)
    wino4_ups(64, 32, 32, 4)
    wino4_ups(64, 64, 32, 8)
    # F(2x2) forward with BatchNorm partials and data gradient: the 64 x 64 tile, 4x4 images, 768 blocks of 256 pixels on 256
    # workgroups (the dynamic deal), the 32-channel tile
    wino2(64, 32, 64, 16)
    wino2(512, 128, 512, 4)
    wino2(768, 16, 64, 16, dgrad=False)  # (its data gradient would have 16 output channels: no Winograd shape)
    wino2(64, 64, 32, 16)
    # F(2x2) weight gradient: plain, behind the upsample, with a budget of one CU (16 slabs: the position groups and K
    # groups remain), and a 64 x 64 tile of 4x4 images too shallow to split: ONE slab, which the unconditional sum copies
    # onto itself (-0 becomes +0)
    wgrad(2, 5, 32, 64, 4)
    wgrad(2, 24, 64, 64, 4, ups=1)
    wgrad(2, 64, 32, 64, 16, cus=1)
    wgrad(2, 8, 64, 64, 4, cus=1, one_slab=True)
    # F(4x4) weight gradient: one slab and several, per channel tile (32 x 64 and 64 x 32)
    wgrad(4, 4, 32, 64, 4, cus=0)
    wgrad(4, 64, 32, 64, 16, cus=1)
    wgrad(4, 64, 32, 64, 16, cus=256)
    wgrad(4, 8, 64, 32, 16, cus=1)
    wgrad(4, 8, 64, 32, 16, cus=256)
    decoder(256, 16, 2)


if __name__ == "__main__":
    main()
