"""The 64-channel block shape of the Winograd F(4x4,3x3) forward / data-gradient kernel (csrc/conv_wino4.hip, W = 1: a work
item of 64 tiles x 64 output channels run as two passes of 32 tiles, four waves transforming half an input patch each)
against the 64-tile x 32-channel shape -- bit for bit, outputs and BatchNorm partials -- and against float64 convolutions at
the bars tests/test_gpu_kernels.py holds the F(4x4,3x3) form to.  Both shapes run through dev.conv_wino4; which one is the
launch's block-shape bit of dev option enc_wino4_mask (bits 16-18 the forwards of layers 1-3, 19-21 their data gradients)."""
import pytest
import torch
import torch.nn.functional as F

from image_generation_amd import _lib, dev

pytestmark = pytest.mark.gpu

BLOCK64_BITS = 0x3F << 16

# L, M, Cin, Cout (of the launch), cus:
#   one item, one pass pair, two chunks (the first stage pair is the last)
#   several items per workgroup (the pending-store path, the dynamic deal), an odd number of chunk pairs, two channel blocks
#   8x8 images: haloed pictures
#   16x16 images: the fifth-cell picture pitch
CASES = [(2, 1024, 8, 64, 0), (2, 3072, 24, 128, 2), (3, 2048, 16, 64, 0), (4, 2048, 8, 64, 0)]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def _rms(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


def _run(mask_bits, fn):
    saved = _lib.get_option("enc_wino4_mask")
    try:
        _lib.set_option("enc_wino4_mask", (saved & ~BLOCK64_BITS) | mask_bits)
        return fn()
    finally:
        _lib.set_option("enc_wino4_mask", saved)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("L,M,Cin,Cout,cus", CASES)
def test_block64_same_bits_and_float64(L, M, Cin, Cout, cus, mode):
    side = 1 << L
    N = M // (side * side)
    # (CPU) the shapes qualify: conv_wino4_shape's conditions and the 64-channel block's
    assert Cin % 8 == 0 and Cout % 64 == 0 and M % 1024 == 0 and N * side * side == M
    torch.manual_seed(1000 * L + M + Cin + mode)
    x = torch.randn(N, Cin, side, side)
    if mode == 0:
        w = torch.randn(Cout, Cin, 3, 3) / (3 * Cin**0.5); b = torch.randn(Cout)
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    else:  # the data gradient: x is the output gradient, the weight is the forward layer's (launch Cout -> launch Cin)
        w = torch.randn(Cin, Cout, 3, 3) / (3 * Cout**0.5); b = None
        ref = F.conv_transpose2d(x.double(), w.double(), padding=1)
    assert ref.shape == (N, Cout, side, side)
    assert dev.conv_wino4_shape(M, Cin, Cout, L)
    xm, wd = dev.nchw_to_morton(x).cuda(), w.cuda()
    bd = b.cuda() if mode == 0 else None

    def launch():
        r = dev.conv_wino4(xm, wd, mode, M, Cin, Cout, L, bias=bd, stats=(mode == 0), cus=cus)
        return r if mode == 0 else (r, None)

    out32, st32 = _run(0, launch)
    out64, st64 = _run(BLOCK64_BITS, launch)
    out64b, st64b = _run(BLOCK64_BITS, launch)
    assert torch.equal(out64, out32) and torch.equal(out64, out64b)
    if mode == 0:
        assert st64.shape == (M // 1024, Cout, 2)
        assert torch.equal(st64, st32) and torch.equal(st64, st64b)
    o = dev.morton_to_nchw(out64.cpu(), N, Cout, side)
    e_max, e_rms = _rel(o, ref), _rms(o, ref)
    print(f"block64 vs float64 [L={L} M={M} {Cin}->{Cout} mode {mode}]: max {e_max:.2e} rms {e_rms:.2e}")
    assert e_max < 3e-5 and e_rms < 8e-6, (e_max, e_rms)
    if mode == 0:
        s = st64.sum(0).cpu().double()
        assert _rel(s[:, 0], ref.sum((0, 2, 3))) < 1e-4 and _rel(s[:, 1], (ref ** 2).sum((0, 2, 3))) < 1e-5
