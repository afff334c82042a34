"""The MMD's exact spin Gram on the FP4 matrix pipe (dev option mmd_gram_fp4) against the int8 form of the same kernels.

Rows of +-1 are exact e2m1 values, the E8M0 scale 127 is 1.0 and the float32 accumulator of the scaled 32x32x64 MFMA holds
the integer dot products exactly, so the Gram is the same integers on both pipes.  Everything behind it (table index,
distance sum, bandwidth, pair table, weights, loss, gradient) must therefore come out bit for bit: every case below runs
once with mmd_gram_fp4 = 0 and once with 1 and is compared with torch.equal on the loss AND the gradient."""
import ctypes
import math

import pytest
import torch

from image_generation_amd import _lib, dev, functional as F

gpu = pytest.mark.gpu

LOADED_RUNS = 10
LOAD_FACTOR = 32


def _spins(g, rows, d, p):
    return ((torch.rand(rows, d, generator=g) < p).float() * 2 - 1).cuda()


def _both(fn, force, shape):
    """fn() (an MMD call on `shape` = (nx, ny, d)) with the int8 Gram and with the FP4 Gram (force: the 128-row pair kernel and the 256-row distance-sum kernel
    whatever the size, as test_gpu_losses.py forces them on small shapes)."""
    out = {}
    for fp4 in (0, 1):
        opts = dict(mmd_gram_fp4=fp4)
        if force:
            opts.update(mmd_w128=1, mmd_d256=1)
        with _lib.option_scope(**opts):
            assert dev.mmd_plan(*shape)["gram"] == ("fp4" if fp4 else "int8")  # the pipe under test is the one that runs
            out[fp4] = fn()
        torch.cuda.synchronize()
    return out[0], out[1]


def _assert_same(a, b, what):
    for u, v in zip(a, b):
        assert torch.equal(u, v), f"{what}: int8 and FP4 Gram differ ({float((u.double() - v.double()).abs().max()):.3e})"


# (2053, 256, 512), (128, 130, 512), (160, 130, 512): a partial row block, partial last chunks of x and of y, the diagonal
# inside a chunk, several column splits; d = 256 (the other converted width): the shapes test_gpu_losses.py uses for it
RAGGED = [(2053, 256, 512), (128, 130, 512), (160, 130, 512), (1000, 256, 256), (97, 5, 256)]


@gpu
def test_c3_shape_with_duplicated_rows_is_bit_identical():
    nx, ny, d = 32768, 256, 512
    g = torch.Generator().manual_seed(nx + d)
    x = _spins(g, nx, d, 0.4)
    x[40:44] = x[39]
    y = _spins(g, ny, d, 0.55)
    a, b = _both(lambda: F.mmd_loss_and_grad(x, y), force=False, shape=(nx, ny, d))
    _assert_same(a, b, "c3")
    assert torch.isfinite(a[0]) and float(a[1].abs().max()) > 0


@gpu
@pytest.mark.parametrize("nx,ny,d", RAGGED)
@pytest.mark.parametrize("kw", [dict(), dict(biased=True), dict(squared=True), dict(bandwidth=37.5)])
def test_ragged_shapes_are_bit_identical(nx, ny, d, kw):
    g = torch.Generator().manual_seed(nx + d)
    x = _spins(g, nx, d, 0.35)
    x[: nx // 4] = x[0]  # duplicated rows: Hamming distance 0 off the diagonal
    y = _spins(g, ny, d, 0.6)
    a, b = _both(lambda: F.mmd_loss_and_grad(x, y, **kw), force=True, shape=(nx, ny, d))  # (bandwidth given: no distance-sum pass)
    _assert_same(a, b, f"{(nx, ny, d)} {kw}")
    assert torch.isfinite(a[0]) and float(a[1].abs().max()) > 0


@gpu
@pytest.mark.parametrize("nx,ny,d", RAGGED)
def test_loss_only_is_bit_identical(nx, ny, d):
    g = torch.Generator().manual_seed(nx + d + 1)
    x, y = _spins(g, nx, d, 0.4), _spins(g, ny, d, 0.5)

    def run():
        with torch.no_grad():
            return (F.mmd_loss(x, y),)

    a, b = _both(run, force=True, shape=(nx, ny, d))
    _assert_same(a, b, f"loss only {(nx, ny, d)}")


@gpu
@pytest.mark.parametrize("nx,ny,d", [(2053, 256, 512), (1000, 256, 256)])
def test_rows_that_are_not_spins_take_the_float_kernels(nx, ny, d):
    """One entry that is not +-1: the spin kernels stand down on the device flag, whichever pipe their Gram is on."""
    g = torch.Generator().manual_seed(7)
    x, y = _spins(g, nx, d, 0.4), _spins(g, ny, d, 0.5)
    x[3, 7] = 0.25
    a, b = _both(lambda: F.mmd_loss_and_grad(x, y), force=True, shape=(nx, ny, d))
    _assert_same(a, b, "float rows")
    assert torch.isfinite(a[0])


# ---- under HBM load (the helper of test_gpu_under_load.py): the chunk ring's size and piece counts changed ------------------
class _Hog:
    """HBM-bound load on its own stream: repeated copies between two 1 GiB buffers; the kernels under test run on a
    stream of higher priority (see test_gpu_under_load.py)."""

    def __init__(self, nbytes=1 << 30):
        self.src = torch.ones(nbytes // 4, device="cuda")
        self.dst = torch.empty_like(self.src)
        self.stream = torch.cuda.Stream()
        self.kstream = torch.cuda.Stream(priority=-1)
        self.dst.copy_(self.src)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(4):
            self.dst.copy_(self.src)
        t1.record()
        torch.cuda.synchronize()
        self.copy_ms = t0.elapsed_time(t1) / 4


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1)


def _under_load(hog, fn, idle_ms):
    cur = torch.cuda.current_stream()
    l0, head, l1, k0, k1 = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
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
    lead, tail = l0.elapsed_time(k0), k1.elapsed_time(l1)
    assert lead > 0 and tail > 0, f"the load did not overlap the kernel (lead {lead:.3f} ms, tail {tail:.3f} ms)"
    return out


@gpu
def test_c3_shape_under_load_equals_the_idle_run():
    nx, ny, d = 32768, 256, 512
    assert _lib.get_option("mmd_gram_fp4") == 1
    g = torch.Generator().manual_seed(nx + d)
    x = _spins(g, nx, d, 0.4)
    x[40:44] = x[39]
    y = _spins(g, ny, d, 0.55)
    hog = _Hog()
    try:
        fn = lambda: F.mmd_loss_and_grad(x, y)  # noqa: E731
        hog.kstream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(hog.kstream):
            fn()
            idle, idle_ms = _timed(fn)
            idle = [t.clone() for t in idle]
            bad = 0
            for _ in range(LOADED_RUNS):
                got = _under_load(hog, fn, idle_ms)
                bad += any(not torch.equal(u, v) for u, v in zip(got, idle))
        torch.cuda.synchronize()
    finally:
        del hog
        torch.cuda.empty_cache()
    assert bad == 0, f"{bad} of {LOADED_RUNS} loaded runs differ from the idle run"


# ---- no GPU needed: the plan's bookkeeping -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,d,slices,ws_before", [
    (2048, 2048, 1024, 4, 46203648),
    (4096, 1000, 1024, 8, 15770112),
    (32768, 256, 512, 1, 50903040),
])
def test_flop_counts_keep_their_values_and_the_workspace_grows_by_the_fp4_copy(nx, ny, d, slices, ws_before):
    """dvg_mmd_spin_flops prices the Gram as before whatever pipe runs it (bench.py derives the kernel
    form from it); dvg_mmd_workspace_bytes grew by at most the packed copy (ws_before: the int8-only library)."""
    L = _lib.lib()
    for fp4 in (1, 0):
        with _lib.option_scope(mmd_gram_fp4=fp4):
            i8, b16, terms = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
            _lib.check(L.dvg_mmd_spin_flops(nx, ny, d, ctypes.byref(i8), ctypes.byref(b16), ctypes.byref(terms)), "dvg_mmd_spin_flops")
            assert terms.value == 2
            assert i8.value == 2.0 * (slices * nx * (nx + ny) + ny * ny) * d
            assert b16.value == 2 * 2.0 * nx * (nx + ny) * d
            ws = L.dvg_mmd_workspace_bytes(nx, ny, d)
            assert ws_before <= ws <= ws_before + (nx + ny) * d // 2 + 256, (ws, ws_before)
