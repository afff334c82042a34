"""The LDS-DMA ring kernels under memory load: each kernel once on an idle device, then several times while an HBM-bound
copy loop runs on a second stream, and every loaded run bit for bit equal to the idle one.

The kernels' rings (global -> LDS by buffer_load ... lds, consumed by ds_read a stage or more later) are correct only if
every read of a stage comes behind a vmcnt wait covering the DMA that filled it and a workgroup barrier.  A missing wait
is invisible on an idle device, where the DMA round trip is short; in the training step these kernels share HBM and L2
with the other stream (the MMD runs beside the decoder's backward) and with whatever else the machine runs.  The kernels
are deterministic (no float atomics, fixed reduction orders), so any difference between runs is a fault, not noise.
The idle run is held against float64 at the bars of the existing parity tests."""
import math

import pytest
import torch
import torch.nn.functional as tF

import halfstep_oracle as ho
from image_generation_amd import _lib, dev, functional as F

pytestmark = pytest.mark.gpu

LOADED_RUNS = 10
LOAD_FACTOR = 32  # the copy loop is sized to this many times the kernel's idle time (at least 10x is required)


class _Hog:
    """HBM-bound load on its own stream: repeated copies between two 1 GiB buffers.  The kernels under test run on a
    stream of higher priority (``kstream``): HIP spreads streams over a few hardware queues per priority, and a second
    stream of the current one's priority may share its queue -- the load then simply runs ahead of the kernel (seen
    after the rest of the suite had created its streams), which the overlap check below reports."""

    def __init__(self, nbytes=1 << 30):
        self.src = torch.ones(nbytes // 4, device="cuda")
        self.dst = torch.empty_like(self.src)
        self.stream = torch.cuda.Stream()
        self.kstream = torch.cuda.Stream(priority=-1)
        self.dst.copy_(self.src)  # (warm: first use of the copy path)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(4):
            self.dst.copy_(self.src)
        t1.record()
        torch.cuda.synchronize()
        self.copy_ms = t0.elapsed_time(t1) / 4


@pytest.fixture(scope="module")
def hog():
    h = _Hog()
    yield h
    del h
    torch.cuda.empty_cache()


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1)


def _under_load(hog, fn, idle_ms):
    """fn() on the current stream (where the library launches) while the copy loop runs on hog's stream.  The current
    stream waits for the loop's first two copies, and the loop lasts LOAD_FACTOR times fn's idle time beyond them; the
    events around both must show that the load started before fn and ended after it, or the run proves nothing."""
    cur = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    l0, head, l1, k0, k1 = ev
    copies = 2 + max(4, math.ceil(LOAD_FACTOR * idle_ms / max(hog.copy_ms, 1e-3)))
    hog.stream.wait_stream(cur)
    with torch.cuda.stream(hog.stream):
        l0.record()
        for i in range(copies):
            hog.dst.copy_(hog.src)
            if i == 1:
                head.record()
        l1.record()
    cur.wait_event(head)
    k0.record(cur)
    out = fn()
    k1.record(cur)
    torch.cuda.synchronize()
    lead, kern, tail = l0.elapsed_time(k0), k0.elapsed_time(k1), k1.elapsed_time(l1)
    assert lead > 0 and tail > 0, (
        f"the load did not overlap the kernel: load start -> kernel start {lead:.3f} ms, kernel end -> load end "
        f"{tail:.3f} ms (both must be > 0; kernel {kern:.3f} ms under load, {idle_ms:.3f} ms idle, {copies} copies of "
        f"{hog.copy_ms:.3f} ms)")
    return out, kern


def _flat(out):
    return [t for t in (out if isinstance(out, (tuple, list)) else (out,)) if t is not None]


def _idle_and_loaded(hog, fn, what):
    """(idle outputs, number of loaded runs that differ from them in any bit); every run on hog.kstream."""
    hog.kstream.wait_stream(torch.cuda.current_stream())  # (the inputs were made on the current stream)
    with torch.cuda.stream(hog.kstream):
        fn()  # warm-up: code objects, workspaces
        idle, idle_ms = _timed(fn)
        idle = [t.clone() for t in _flat(idle)]
        bad, loaded_ms = 0, []
        for _ in range(LOADED_RUNS):
            got, ms = _under_load(hog, fn, idle_ms)
            loaded_ms.append(ms)
            bad += any(not torch.equal(a, b) for a, b in zip(_flat(got), idle))
    torch.cuda.synchronize()
    print(f"{what}: {bad} of {LOADED_RUNS} loaded runs differ from the idle run ({idle_ms:.3f} ms idle, "
          f"{min(loaded_ms):.3f}-{max(loaded_ms):.3f} ms under load)")
    return idle, bad


def _spins(g, rows, d, p):
    return ((torch.rand(rows, d, generator=g) < p).float() * 2 - 1).cuda()


def _mmd_form(nx, ny, d):
    """(bf16 terms, int8 Gram passes) of the spin pair kernel dvg_mmd_fwd_bwd launches for this shape: 2 terms = the
    128-row-block kernel, whose passes are its feature slices (grid z)."""
    plan = dev.mmd_plan(nx, ny, d)
    assert (plan["pair"] == "w128") == (plan["bf16_terms"] == 2) and (plan["pair"] != "w128" or plan["gram_passes"] == plan["slices"])
    return plan["bf16_terms"], plan["gram_passes"]


@pytest.mark.parametrize("nx,ny,d,slices", [
    (2048, 2048, 1024, 4),   # c5's slice: mmd_pair_w128_kernel<32, 8, true> (64 + 64 chunks in 4 column splits of 32), 256 gradient blocks
    (4096, 1000, 1024, 8),   # mmd_pair_w128_kernel<32, 4>: 128 x chunks are not whole splits of 80 -> eight feature slices, 256 gradient blocks
    (32768, 256, 512, 1),    # control, GPT = 1: c3's mmd_pair_w128_kernel<16, 16>, 256 row blocks
])
def test_mmd_under_load_is_bit_identical_and_matches_float64(hog, nx, ny, d, slices):
    """F.mmd_loss_and_grad (loss and gradient).  The d = 1024 forms run NST / NFT > 1 Gram k-steps per feature tile and
    pre-read the next chunk's first operands inside the current chunk -- the path whose ring wait must cover the DMA one
    chunk back; the d = 512 form (one Gram k-step per tile, vmcnt(0) at every chunk) is the control.  The form each shape
    takes is asserted through the library's own plan (dev.mmd_plan)."""
    assert _mmd_form(nx, ny, d) == (2, slices)
    g = torch.Generator().manual_seed(nx + d)
    x = _spins(g, nx, d, 0.4)
    x[40:44] = x[39]  # duplicated rows: zero distances off the diagonal
    y = _spins(g, ny, d, 0.55)
    (loss, grad), bad = _idle_and_loaded(hog, lambda: F.mmd_loss_and_grad(x, y), f"mmd {nx} x {ny} x {d}")
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run (nx={nx} ny={ny} d={d})"
    want, gwant = ho.chunked_mmd(x.double(), y.double(), chunk=1024)
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
    assert float((grad.double() - gwant).abs().max()) <= 2e-5 * float(gwant.abs().max())


# c3's encoder layer 2: 4096 images, 64 -> 128 channels on 8x8 maps (262144 rows: thousands of tiles)
CONV = dict(N=4096, Cin=64, Cout=128, side=8)


@pytest.fixture(scope="module")
def conv_case():
    N, Cin, Cout, side = CONV["N"], CONV["Cin"], CONV["Cout"], CONV["side"]
    torch.manual_seed(29)
    x = torch.randn(N, Cin, side, side)
    w = torch.randn(Cout, Cin, 3, 3) / (3 * Cin**0.5)
    b = torch.randn(Cout)
    gy = torch.randn(N, Cout, side, side)
    x64, w64, gy64 = x.double(), w.double(), gy.double()
    ref = dict(y=tF.conv2d(x64, w64, b.double(), padding=1), dx=tF.conv_transpose2d(gy64, w64, padding=1),
               dw=torch.nn.grad.conv2d_weight(x64, w.shape, gy64, padding=1))
    L, M = side.bit_length() - 1, N * side * side
    dv = dict(xm=dev.nchw_to_morton(x).cuda(), gym=dev.nchw_to_morton(gy).cuda(), w=w.cuda(), b=b.cuda(), L=L, M=M)
    return dv, ref


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def _rms(a, b):
    return float((a.double() - b).norm() / b.norm())


def _nchw(t, C, side=CONV["side"]):
    return dev.morton_to_nchw(t.cpu(), CONV["N"], C, side)


def test_conv_igemm_dma_under_load(hog, conv_case):
    """conv_igemm forward (with bias and BatchNorm partial sums) and data gradient, LDS-DMA staging (igemm_dma = 1)."""
    dv, ref = conv_case
    Cin, Cout, M, L = CONV["Cin"], CONV["Cout"], dv["M"], dv["L"]
    with _lib.option_scope(igemm_dma=1):
        (out, st), bad_f = _idle_and_loaded(hog, lambda: dev.conv_igemm(dv["xm"], dv["w"], 0, M, Cin, Cout, L, bias=dv["b"], stats=True),
                                            "conv_igemm forward")
        (dx,), bad_d = _idle_and_loaded(hog, lambda: dev.conv_igemm(dv["gym"], dv["w"], 1, M, Cout, Cin, L), "conv_igemm dgrad")
    assert bad_f == 0 and bad_d == 0, f"loaded runs differing from the idle run: forward {bad_f}, data gradient {bad_d} of {LOADED_RUNS}"
    y = ref["y"]
    assert _rel(_nchw(out, Cout), y) < 2e-6
    s = st.sum(0).cpu().double()
    assert _rel(s[:, 0], y.sum((0, 2, 3))) < 1e-4 and _rel(s[:, 1], (y ** 2).sum((0, 2, 3))) < 1e-5
    assert _rel(_nchw(dx, Cin), ref["dx"]) < 2e-6


def test_conv_wgrad_dma_under_load(hog, conv_case):
    """The 3x3 weight gradient, LDS-DMA staging (wgrad_dma = 1)."""
    dv, ref = conv_case
    Cin, Cout, M, L = CONV["Cin"], CONV["Cout"], dv["M"], dv["L"]
    shape = (Cout, Cin, 3, 3)
    with _lib.option_scope(wgrad_dma=1):
        (gw,), bad = _idle_and_loaded(hog, lambda: dev.conv_wgrad(dv["xm"], dv["gym"], 0, shape, M, Cin, Cout, L), "conv_wgrad")
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run"
    assert _rel(gw.cpu(), ref["dw"]) < 3e-6


def test_winograd_f2x2_under_load(hog, conv_case):
    """Winograd F(2x2,3x3) forward and data gradient (csrc/conv_wino.hip: its chunk barrier relies on the compiler's own
    vmcnt for the ring)."""
    dv, ref = conv_case
    Cin, Cout, M, L = CONV["Cin"], CONV["Cout"], dv["M"], dv["L"]
    with _lib.option_scope(enc_wino=1):
        assert dev.conv_wino_ok(M, Cin, Cout, L) and dev.conv_wino_ok(M, Cout, Cin, L)
        (out, st), bad_f = _idle_and_loaded(hog, lambda: dev.conv_wino(dv["xm"], dv["w"], 0, M, Cin, Cout, L, bias=dv["b"], stats=True),
                                            "F(2x2) forward")
        (dx,), bad_d = _idle_and_loaded(hog, lambda: dev.conv_wino(dv["gym"], dv["w"], 1, M, Cout, Cin, L), "F(2x2) dgrad")
    assert bad_f == 0 and bad_d == 0, f"loaded runs differing from the idle run: forward {bad_f}, data gradient {bad_d} of {LOADED_RUNS}"
    y = ref["y"]
    assert _rel(_nchw(out, Cout), y) < 2e-6
    s = st.sum(0).cpu().double()
    assert _rel(s[:, 0], y.sum((0, 2, 3))) < 1e-4 and _rel(s[:, 1], (y ** 2).sum((0, 2, 3))) < 1e-5
    assert _rel(_nchw(dx, Cin), ref["dx"]) < 2e-6


def test_winograd_f4x4_under_load(hog, conv_case):
    """Winograd F(4x4,3x3) forward and data gradient (csrc/conv_wino4.hip)."""
    dv, ref = conv_case
    Cin, Cout, M, L = CONV["Cin"], CONV["Cout"], dv["M"], dv["L"]
    assert dev.conv_wino4_shape(M, Cin, Cout, L) and dev.conv_wino4_shape(M, Cout, Cin, L)
    (out, st), bad_f = _idle_and_loaded(hog, lambda: dev.conv_wino4(dv["xm"], dv["w"], 0, M, Cin, Cout, L, bias=dv["b"], stats=True),
                                        "F(4x4) forward")
    (dx,), bad_d = _idle_and_loaded(hog, lambda: dev.conv_wino4(dv["gym"], dv["w"], 1, M, Cout, Cin, L), "F(4x4) dgrad")
    assert bad_f == 0 and bad_d == 0, f"loaded runs differing from the idle run: forward {bad_f}, data gradient {bad_d} of {LOADED_RUNS}"
    y, o4, g4 = ref["y"], _nchw(out, Cout), _nchw(dx, Cin)
    assert _rel(o4, y) < 3e-5 and _rms(o4, y) < 8e-6
    assert _rel(g4, ref["dx"]) < 3e-5 and _rms(g4, ref["dx"]) < 8e-6
    s = st.sum(0).cpu().double()
    assert _rel(s[:, 0], y.sum((0, 2, 3))) < 1e-4 and _rel(s[:, 1], (y ** 2).sum((0, 2, 3))) < 1e-5
