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


# ------------------------------------------------------------------------------------------------------------------------
# The matrix: one case per LDS-DMA ring instantiation.  Every case first asserts, through the library's own form hooks, that
# its launch is the instantiation it names; its shape wraps the ring at least twice (four or more chunks), gives a persistent
# workgroup three or more items and launches enough workgroups to run beside the load.  The idle run is held to float64 at the
# bar of the kernel's parity test; the printed lines are profiles/r11_under_load_matrix.txt.

KINDS = {"fwd": 0, "dgrad": 1, "ups_fwd": 2, "ups_dgrad": 3}  # the hooks' weight modes (include/dvg_dev.h)


def _layer(kind, N, Ci, Co, side, seed, pm1=False, rounded=False):
    """One 3x3 layer launch of channels Ci -> Co on a fine grid of side x side and its float64 reference: the Conv2d forward,
    its data gradient, the Upsample(x2) + ConvTranspose2d forward (the input lives at side / 2) or that layer's data gradient
    onto the source map (the 2x2 sums of the adjoint).  pm1: +-1 inputs; rounded: the reference of the bf16-rounded operands."""
    g = torch.Generator().manual_seed(seed)
    src = side // 2 if kind == "ups_fwd" else side
    x = torch.randn(N, Ci, src, src, generator=g)
    if pm1:
        x = torch.where(x < 0, -1.0, 1.0)
    w = torch.randn((Co, Ci, 3, 3) if kind in ("fwd", "ups_dgrad") else (Ci, Co, 3, 3), generator=g) / (3 * Ci**0.5)
    b = torch.randn(Co, generator=g) if kind in ("fwd", "ups_fwd") else None
    rd = (lambda t: t.to(torch.bfloat16).double()) if rounded else (lambda t: t.double())
    x64, w64 = rd(x), rd(w)
    if kind == "fwd":
        ref = tF.conv2d(x64, w64, b.double(), padding=1)
    elif kind == "dgrad":
        ref = tF.conv_transpose2d(x64, w64, padding=1)
    elif kind == "ups_fwd":
        ref = tF.conv_transpose2d(tF.interpolate(x64, scale_factor=2, mode="nearest"), w64, b.double(), padding=1)
    else:
        ref = tF.conv2d(x64, w64, padding=1).reshape(N, Co, side // 2, 2, side // 2, 2).sum((3, 5))
    return dict(xm=dev.nchw_to_morton(x).cuda(), w=w.cuda(), b=None if b is None else b.cuda(), ref=ref, N=N, Co=Co,
                mode=KINDS[kind], out_side=side // 2 if kind == "ups_dgrad" else side, L=side.bit_length() - 1, M=N * side * side)


def _out_nchw(c, out):
    return dev.morton_to_nchw(out.cpu(), c["N"], c["Co"], c["out_side"])


def _stats_ok(st, ref):
    s = st.sum(0).cpu().double()
    dims = tuple(d for d in range(ref.dim()) if d != 1)
    return _rel(s[:, 0], ref.sum(dims)) < 1e-4 and _rel(s[:, 1], (ref ** 2).sum(dims)) < 1e-5


def _record(inst, shape, bad, dist):
    print(f"  [matrix] {inst} | {shape} | {bad} of {LOADED_RUNS} differ | vs float64 {dist}")


def _tile_counters():
    _lib.lib().dvg_decoder_workspace_bytes(64, 64)  # (creates the device's tile counters: without them every deal is static)


def _persistent_ok(nblk, ny, cus, chunks):
    """The shape rules for a persistent Winograd grid of cus / ny workgroups per column block: four or more chunks, three or
    more tile blocks per workgroup (from there the deal is dynamic), sixteen or more workgroups."""
    gx = cus // ny
    return chunks >= 4 and gx >= 1 and nblk >= 3 * gx and gx * ny >= 16


# kind, N, Ci, Co, side, cus: conv_wino8_kernel<2,2,8,UM> at Co % 64 == 0 (tile blocks of 256 rows, chunks of 8 channels),
# <4,1,4,UM> otherwise (512 rows, 4 channels); UM = 1 / 2 behind the upsample
WINO2_MATRIX = [
    ("fwd", 512, 32, 96, 8, 48), ("dgrad", 2048, 64, 32, 4, 16),                   # <4,1,4>
    ("ups_fwd", 2048, 64, 64, 4, 32), ("ups_fwd", 512, 64, 64, 8, 32),             # <2,2,8,1> at L = 2, 3
    ("ups_dgrad", 2048, 64, 64, 4, 32), ("ups_dgrad", 512, 64, 64, 8, 32),         # <2,2,8,2>
    ("ups_fwd", 2048, 32, 96, 4, 48), ("ups_fwd", 512, 32, 32, 8, 16),             # <4,1,4,1,0>
    ("ups_dgrad", 2048, 32, 32, 4, 16), ("ups_dgrad", 512, 32, 96, 8, 48),         # <4,1,4,2,0>
]


@pytest.mark.parametrize("kind,N,Ci,Co,side,cus", WINO2_MATRIX)
def test_winograd_f2x2_matrix_under_load(hog, kind, N, Ci, Co, side, cus):
    """Every conv_wino8_kernel instantiation launch_conv_wino can take (csrc/conv_wino.hip: no explicit vmcnt at the chunk
    barrier, the compiler counts each instantiation's DMA pieces)."""
    c = _layer(kind, N, Ci, Co, side, seed=N + Ci + Co + side)
    um = {"fwd": 0, "dgrad": 0, "ups_fwd": 1, "ups_dgrad": 2}[kind]
    wide = Co % 64 == 0
    inst = f"conv_wino8_kernel<{'2,2,8' if wide else '4,1,4'},{um}>"
    assert dev.conv_wino_shape(c["M"], Ci, Co, c["L"])
    assert _persistent_ok(c["M"] // (256 if wide else 512), Co // (64 if wide else 32), cus, Ci // (8 if wide else 4))
    _tile_counters()
    stats = c["b"] is not None
    out, bad = _idle_and_loaded(hog, lambda: dev.conv_wino(c["xm"], c["w"], c["mode"], c["M"], Ci, Co, c["L"], bias=c["b"], stats=stats,
                                                           cus=cus, um=um), inst)
    e = _rel(_out_nchw(c, out[0]), c["ref"])
    _record(inst, f"{kind} N={N} {Ci}->{Co} @{side} cus={cus}", bad, f"{e:.2e}")
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run"
    assert e < (3e-6 if kind == "ups_dgrad" else 2e-6)
    assert not stats or _stats_ok(out[1], c["ref"])


BLOCK64_BITS = 0x3F << 16  # dev option enc_wino4_mask: the block-shape bits of the six encoder launches

# kind, L, block64, N, Ci, Co, cus: tile blocks of 1024 rows, chunks of 4 channels, column blocks of 32 (64: block64) channels
WINO4_MATRIX = [
    ("fwd", 2, 0, 2048, 32, 64, 16), ("fwd", 4, 0, 128, 32, 64, 16),                                                # conv_wino4_kernel<L>
    ("fwd", 2, 1, 4096, 32, 64, 16), ("fwd", 3, 1, 1024, 32, 64, 16), ("fwd", 4, 1, 256, 32, 64, 16),                 # <L,0,1>
    ("dgrad", 2, 1, 4096, 32, 64, 16), ("dgrad", 3, 1, 1024, 32, 64, 16), ("dgrad", 4, 1, 256, 32, 64, 16),
    ("ups_fwd", 2, 0, 2048, 32, 64, 16), ("ups_fwd", 3, 0, 512, 32, 64, 16),                                         # <L,1>
    ("ups_dgrad", 2, 0, 2048, 32, 64, 16), ("ups_dgrad", 3, 0, 512, 32, 64, 16),                                     # <L,2>
]


@pytest.mark.parametrize("kind,L,block64,N,Ci,Co,cus", WINO4_MATRIX)
def test_winograd_f4x4_matrix_under_load(hog, kind, L, block64, N, Ci, Co, cus):
    """Every conv_wino4_kernel instantiation (csrc/conv_wino4.hip) but <3>, which test_winograd_f4x4_under_load runs.  The
    64-channel block shape also gives the bits of the 64 x 32 shape's idle run."""
    side = 1 << L
    c = _layer(kind, N, Ci, Co, side, seed=N + L + Co + block64)
    um = {"fwd": 0, "dgrad": 0, "ups_fwd": 1, "ups_dgrad": 2}[kind]
    inst = f"conv_wino4_kernel<{L},{um},{block64}>"
    assert dev.conv_wino4_shape(c["M"], Ci, Co, L) and (not block64 or (um == 0 and Co % 64 == 0))
    assert _persistent_ok(c["M"] // 1024, Co // (64 if block64 else 32), cus, Ci // 4)
    _tile_counters()
    stats = c["b"] is not None
    launch = lambda: dev.conv_wino4(c["xm"], c["w"], c["mode"], c["M"], Ci, Co, L, bias=c["b"], stats=stats, cus=cus, um=um)  # noqa: E731
    mask = _lib.get_option("enc_wino4_mask") & ~BLOCK64_BITS
    with _lib.option_scope(enc_wino4_mask=mask | (BLOCK64_BITS if block64 else 0)):
        assert ((_lib.get_option("enc_wino4_mask") >> 16) & 0x3F) == (0x3F if block64 else 0)
        out, bad = _idle_and_loaded(hog, launch, inst)
    e, r = _rel(_out_nchw(c, out[0]), c["ref"]), _rms(_out_nchw(c, out[0]), c["ref"])
    _record(inst, f"{kind} N={N} {Ci}->{Co} @{side} cus={cus}", bad, f"max {e:.2e} rms {r:.2e}")
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run"
    assert e < 3e-5 and r < 8e-6
    assert not stats or _stats_ok(out[1], c["ref"])
    if block64:
        with _lib.option_scope(enc_wino4_mask=mask):
            narrow = _flat(launch())
        assert all(torch.equal(a, b) for a, b in zip(narrow, out)), "the 64-channel block shape and the 64 x 32 shape differ"


def _one_tap_gemm(rows, Ci, Co, seed, pm1=False, rounded=False):
    """out = x w^T + b through the 1-tap implicit GEMM (the matrix sits at tap 0 of a Conv2d weight) and its float64 reference."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, Ci, generator=g)
    if pm1:
        x = torch.where(x < 0, -1.0, 1.0)
    w = torch.randn(Co, Ci, generator=g) / Ci**0.5
    b = torch.randn(Co, generator=g)
    rd = (lambda t: t.to(torch.bfloat16).double()) if rounded else (lambda t: t.double())
    w9 = torch.zeros(Co, Ci, 3, 3)
    w9[:, :, 0, 0] = w
    return dict(xm=x.cuda(), w=w9.cuda(), b=b.cuda(), ref=rd(x) @ rd(w).T + b.double(), mode=0, L=0, M=rows)


# name, operand mode, options, expected form (the entries of dev.conv_igemm_form that the case is about), layer
# 9-tap layers: (kind, N, Ci, Co, side); 1-tap GEMMs: (rows, Ci, Co) -- test_gpu_spin_gemm.py's 512 x 512 GEMM at the
# 16384 rows from which 128 x 128 tiles serve it
IGEMM_MATRIX = [
    ("form 4 (f32x3), 9 taps", "f32x3", {}, dict(pm=4), ("fwd", 256, 64, 128, 8)),
    ("form 5 (bf16), 9 taps", "bf16", {}, dict(pm=5), ("fwd", 256, 64, 128, 8)),
    ("form 6 (spin A), 9 taps", "f32", dict(dev_spin_operand=1), dict(pm=6), ("fwd", 256, 64, 128, 8)),
    ("form 4 (f32x3), 1 tap", "f32x3", {}, dict(pm=4, tile=(128, 128)), (16384, 512, 512)),
    ("form 5 (bf16), 1 tap", "bf16", {}, dict(pm=5, tile=(128, 128)), (16384, 512, 512)),
    ("form 6 (spin A), 1 tap", "f32", dict(dev_spin_operand=1), dict(pm=6, tile=(128, 128)), (16384, 512, 512)),
    ("form 3, tile 128x64", "f32", {}, dict(pm=3, tile=(128, 64), ksplit=1), ("fwd", 1024, 32, 64, 8)),
    ("form 3, tile 64x64", "f32", {}, dict(pm=3, tile=(64, 64), ksplit=1, posmajor=True), ("fwd", 256, 64, 64, 8)),
    ("form 3, tile 32x64, split K", "f32", {}, dict(pm=3, tile=(32, 64), ksplit=8), ("fwd", 128, 256, 64, 4)),
    ("form 3, tile 128x32", "f32", {}, dict(pm=3, tile=(128, 32), ksplit=1), ("fwd", 256, 64, 96, 8)),
    ("form 3, pixel-major tiles", "f32", dict(igemm_posmajor=0), dict(pm=3, tile=(64, 64), posmajor=False), ("fwd", 256, 64, 64, 8)),
    ("form 3, upsample gather", "f32", {}, dict(pm=3, tile=(64, 64)), ("ups_fwd", 256, 64, 64, 8)),
    ("form 3, quad-sum epilogue", "f32", {}, dict(pm=3, tile=(64, 64)), ("ups_dgrad", 256, 64, 64, 8)),
]


@pytest.mark.parametrize("name,precision,opts,form,layer", IGEMM_MATRIX, ids=[m[0] for m in IGEMM_MATRIX])
def test_conv_igemm_matrix_under_load(hog, name, precision, opts, form, layer):
    """The LDS-DMA forms of conv_igemm_kernel beyond form 3 at one shape: the operand forms that issue the next chunk late
    (4, 5, 6), every block tile, the split-K range, pixel-major tiles, the upsample gather, the quad-sum epilogue, the 1-tap
    GEMM.  Forms 4 and 6 are held to the split mode's bar (as close to float64 as form 3 on the same inputs, or 1e-6), form 5
    to the reference of the bf16-rounded operands, form 3 to its parity bars."""
    pm, taps9 = form["pm"], len(layer) == 5
    pm1, rounded = pm == 6, pm == 5
    if taps9:
        kind, N, Ci, Co, side = layer
        c = _layer(kind, N, Ci, Co, side, seed=N + Ci + Co + pm, pm1=pm1, rounded=rounded)
        ups, poolsum, ntaps = int(kind == "ups_fwd"), int(kind == "ups_dgrad"), 9
    else:
        (rows, Ci, Co), kind, ups, poolsum, ntaps = layer, "fwd", 0, 0, 1
        c = _one_tap_gemm(rows, Ci, Co, seed=rows + pm, pm1=pm1, rounded=rounded)
    stats = kind == "fwd"
    launch = lambda: dev.conv_igemm(c["xm"], c["w"], c["mode"], c["M"], Ci, Co, c["L"], ntaps=ntaps, ups=ups, poolsum=poolsum,  # noqa: E731
                                    bias=c["b"], stats=stats)
    to_ref = (lambda o: _out_nchw(c, o)) if taps9 else (lambda o: o.cpu())
    e_f = _rel(to_ref(_flat(launch())[0]), c["ref"]) if pm in (4, 6) else None  # (form 3, same inputs)
    _lib.set_conv_precision(precision)
    try:
        with _lib.option_scope(**opts):
            got = dev.conv_igemm_form(c["M"], Ci, Co, c["L"], ntaps=ntaps, ups=ups, poolsum=poolsum)
            assert {k: got[k] for k in form} == form, got
            out, bad = _idle_and_loaded(hog, launch, name)
    finally:
        _lib.set_conv_precision("f32")
    e = _rel(to_ref(out[0]), c["ref"])
    _record(f"conv_igemm_kernel<{got['tile'][0]},{got['tile'][1]},PM={pm}> {name}",
            f"{kind} M={c['M']} {Ci}->{Co} taps={ntaps} ksplit={got['ksplit']} posmajor={int(got['posmajor'])}", bad,
            f"{e:.2e}" + (f" (form 3: {e_f:.2e})" if e_f is not None else " (of the bf16-rounded operands)" if rounded else ""))
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run"
    if pm in (4, 6):
        assert e < max(1e-6, 1.5 * e_f), (e, e_f)
    else:
        assert e < (3e-6 if rounded or kind == "ups_dgrad" else 2e-6)
    assert not stats or _stats_ok(out[1], c["ref"])


# Cin, Cout, ups, ntaps, spin, the kernel: 256 images of 8x8 (16384 rows; 1 tap: 16384 rows of a 256 x 256 matrix, the fewest
# that the 128 x 128 DMA kernel serves)
WGRAD_MATRIX = [
    (128, 96, 0, 9, 0, "conv_wgrad9_dma_kernel<2,1,2>"), (96, 128, 0, 9, 0, "conv_wgrad9_dma_kernel<1,2,2>"),
    (96, 96, 0, 9, 0, "conv_wgrad9_dma_kernel<1,1,4>"), (128, 128, 1, 9, 0, "conv_wgrad9_dma_kernel<2,2,2> behind the upsample"),
    (256, 256, 0, 1, 0, "conv_wgrad1_dma_kernel<false>"), (256, 256, 0, 1, 1, "conv_wgrad1_dma_kernel<true>"),
]


@pytest.mark.parametrize("Cin,Cout,ups,ntaps,spin,inst", WGRAD_MATRIX, ids=[m[5] for m in WGRAD_MATRIX])
def test_conv_wgrad_matrix_under_load(hog, Cin, Cout, ups, ntaps, spin, inst):
    """The LDS-DMA weight-gradient kernels beyond conv_wgrad9_dma_kernel<2,2,2>: the three other channel tiles, the gather
    behind the upsample, and both forms of the 1-tap 128 x 128 kernel (the spin form on +-1 rows, at the split mode's bar)."""
    N, side, M = 256, 8, 16384
    g = torch.Generator().manual_seed(Cin + Cout + ups + ntaps)
    if ntaps == 9:
        src = side // 2 if ups else side
        x = torch.randn(N, Cin, src, src, generator=g)
        gy = torch.randn(N, Cout, side, side, generator=g)
        xf = tF.interpolate(x.double(), scale_factor=2, mode="nearest") if ups else x.double()
        ref = torch.nn.grad.conv2d_weight(xf, (Cout, Cin, 3, 3), gy.double(), padding=1)
        shape, mode, L = (Cout, Cin, 3, 3), 0, 3
        if ups:  # (the ConvTranspose2d layer's weight: (Cin, Cout, 3, 3), taps mirrored)
            ref, shape, mode = ref.flip(2, 3).transpose(0, 1).contiguous(), (Cin, Cout, 3, 3), 2
        xm, gym = dev.nchw_to_morton(x).cuda(), dev.nchw_to_morton(gy).cuda()
    else:
        x = torch.randn(M, Cin, generator=g)
        if spin:
            x = torch.where(x < 0, -1.0, 1.0)
        gy = torch.randn(M, Cout, generator=g)
        ref, shape, mode, L = gy.double().T @ x.double(), (Cout, Cin, 3, 3), 0, 0
        xm, gym = x.cuda(), gy.cuda()
    # (a 1-tap launch writes tap 0 of the checkpoint-layout gradient and leaves the other eight as they were allocated)
    pick = (lambda t: t) if ntaps == 9 else (lambda t: t[:, :, 0, 0])
    launch = lambda: pick(dev.conv_wgrad(xm, gym, mode, shape, M, Cin, Cout, L, ntaps=ntaps, ups=ups))  # noqa: E731
    e_f = _rel(launch().cpu(), ref) if spin else None  # (the plain form, same inputs)
    with _lib.option_scope(dev_spin_operand=spin):
        f = dev.conv_wgrad_form(M, Cin, Cout, ntaps=ntaps, ups=ups)
        want = (128, 128) if ntaps == 1 else (64 if Cin % 64 == 0 else 32, 64 if Cout % 64 == 0 else 32)
        assert f == dict(tile=want, dma=True, tap1_dma=ntaps == 1, spin=bool(spin)), f
        assert inst.startswith("conv_wgrad1_dma_kernel<" + ("true" if spin else "false") if ntaps == 1 else
                               f"conv_wgrad9_dma_kernel<{want[0] // 32},{want[1] // 32},")
        (gw,), bad = _idle_and_loaded(hog, launch, inst)
    e = _rel(gw.cpu(), ref)
    _record(inst, f"M={M} {Cin}x{Cout} taps={ntaps} ups={ups}", bad, f"{e:.2e}" + (f" (plain form: {e_f:.2e})" if spin else ""))
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run"
    assert e < (max(1e-6, 1.5 * e_f) if spin else 3e-6)


def _mmd_run(hog, d, what, **opts):
    nx, ny = 4096, 256
    g = torch.Generator().manual_seed(nx + d)
    x, y = _spins(g, nx, d, 0.4), _spins(g, ny, d, 0.55)
    x[40:44] = x[39]  # duplicated rows: zero distances off the diagonal
    with _lib.option_scope(mmd_w128=1, mmd_d256=1, **opts):
        plan = dev.mmd_plan(nx, ny, d)
        assert plan["pair"] == "w128" and plan["dist"] == "spin256", plan
        (loss, grad), bad = _idle_and_loaded(hog, lambda: F.mmd_loss_and_grad(x, y), what)
    want, gwant = ho.chunked_mmd(x.double(), y.double(), chunk=1024)
    e_l, e_g = abs(float(loss) - float(want)) / abs(float(want)), float((grad.double() - gwant).abs().max()) / float(gwant.abs().max())
    _record(f"mmd_pair_w128_kernel<{plan['pair_params']['NST']},{plan['pair_params']['NFT']}> + mmd_distsum_spin256_kernel<"
            f"{plan['dist_ns']}>, {plan['gram']} Gram", f"{nx} x {ny} x {d}", bad, f"loss {e_l:.2e} gradient {e_g:.2e}")
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run (d={d})"
    assert e_l <= 1e-5 and e_g <= 2e-5
    return plan, loss, grad


@pytest.mark.parametrize("d", [128, 384])
def test_mmd_int8_gram_under_load(hog, d):
    """The 128-row-block pair kernel and the 256-row distance sum (forced: options mmd_w128, mmd_d256) at the feature widths
    whose exact spin Gram runs on the int8 pipe."""
    plan, _loss, _grad = _mmd_run(hog, d, f"mmd int8 d={d}")
    assert plan["gram"] == "int8"


def test_mmd_fp4_gram_under_load_and_same_bits_as_int8(hog):
    """d = 256: the exact spin Gram on the FP4 pipe; with option mmd_gram_fp4 = 0 the same kernels on the int8 pipe, under load
    too, and the same bits."""
    plan, loss, grad = _mmd_run(hog, 256, "mmd fp4 d=256")
    assert plan["gram"] == "fp4"
    plan8, loss8, grad8 = _mmd_run(hog, 256, "mmd int8 d=256", mmd_gram_fp4=0)
    assert plan8["gram"] == "int8"
    assert torch.equal(loss, loss8) and torch.equal(grad, grad8)


# ------------------------------------------------------------------------------------------------------------------------
# Whole calls: the forms no hook reaches (the decoder's folded upsample: conv_wgrad9_dma_kernel<1,1,4,true>, igemm fold = 1 / 2)
# and the default plans as the training step launches them, side stream included.  Float64 parity of these shapes is
# tests/test_gpu_fullsize.py's.

def _np_state(params):
    import numpy as np
    return {k: torch.from_numpy(np.array(v)) for k, v in params.items()}


def _decoder_call(n, state, spins, masks, go):
    from image_generation_amd.modules import Decoder
    dec = Decoder(n)
    dec.load_state_dict(state)
    dec = dec.cuda().train()
    dec.inject_dropout_masks(masks)
    sg = spins.clone().requires_grad_(True)
    out = dec(sg)
    (out * go).sum().backward()
    return [out.detach(), sg.grad] + [p.grad for p in dec.parameters()] + [b.detach() for b in dec.buffers()]


@pytest.mark.parametrize("opts,forms", [({}, ("wino2", "wino4")), (dict(dec_wino=0), ("fold",))], ids=["default plan", "folded upsample"])
def test_decoder_training_call_under_load(hog, opts, forms):
    """Forward + backward of the decoder at 8192 rows (n = 128) with injected dropout masks, rebuilt from the same state for
    every run: the output, the spin gradient, every parameter gradient and the BatchNorm buffers bit for bit.  Under the
    default plan the layers behind the upsample run in the Winograd forms; with option dec_wino = 0 they take their base
    form, the folded upsample, in all three passes."""
    import gen
    n, B, R = 128, 1024, 8
    state = _np_state(gen.make_params(n, "decoder", 31))
    spins = torch.from_numpy(gen.make_spins(B, R, n, 17)).cuda()
    masks = [torch.from_numpy(m).cuda() for m in gen.make_masks(B * R, 19)]
    go = torch.randn(B, R, 1, 32, 32, generator=torch.Generator().manual_seed(23)).cuda()
    with _lib.option_scope(**opts):
        layers, _flags = dev.plan_forms("decoder", B * R, n)
        assert all(f in forms for l in (1, 2) for f in layers[l]) and all(any(f in layers[l] for l in (1, 2)) for f in forms), layers
        outs, bad = _idle_and_loaded(hog, lambda: _decoder_call(n, state, spins, masks, go), f"decoder call {layers[1]} {layers[2]}")
    _record(f"decoder training call, layers 1-2 {layers[1]} {layers[2]}", f"N={B * R} n={n}", bad, "(tests/test_gpu_fullsize.py)")
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run"
    assert all(bool(torch.isfinite(t.float()).all()) for t in outs)


def _encoder_call(n, state, images, go):
    from image_generation_amd.modules import Encoder
    enc = Encoder(n)
    enc.load_state_dict(state)
    enc = enc.cuda().train()
    out = enc(images)
    (out * go).sum().backward()
    return [out.detach()] + [p.grad for p in enc.parameters()] + [b.detach() for b in enc.buffers()]


def test_encoder_training_call_under_load(hog):
    """Forward + backward of the encoder at a batch whose default plan mixes direct and Winograd layers, rebuilt from the same
    state for every run: the logits, every parameter gradient and the BatchNorm buffers bit for bit."""
    import gen
    n, B = 128, 1024
    layers, _flags = dev.plan_forms("encoder", B, n)
    used = {f for l in (1, 2, 3) for f in layers[l]}
    assert "direct" in used and used & {"wino2", "wino4"}, layers
    state = _np_state(gen.make_params(n, "encoder", 37))
    images = torch.from_numpy(gen.make_images(B, 41)).cuda()
    go = torch.randn(B, n, generator=torch.Generator().manual_seed(43)).cuda()
    outs, bad = _idle_and_loaded(hog, lambda: _encoder_call(n, state, images, go), f"encoder call {layers[1:]}")
    _record(f"encoder training call, layers 1-3 {layers[1:]}", f"B={B} n={n}", bad, "(tests/test_gpu_fullsize.py)")
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run"
    assert all(bool(torch.isfinite(t.float()).all()) for t in outs)
