"""The decoder input layer's GEMMs on declared +-1 spins (conv_igemm_kernel operand form 6, conv_wgrad1_dma_kernel's spin
form): the spins as exact bf16 values, the float32 operand as three bf16 pieces, three exact products per k-step on the bf16
MFMA, float32 accumulation.  The bar is the split mode's own (tests/test_gpu_kernels.py): against float64 the form must be
as close as the f32-MFMA form is on the same inputs.  Without the promise, or with option dec_spin_gemm = 0, nothing
changes, bit for bit."""
import numpy as np
import pytest
import torch

import gen
from image_generation_amd import _lib, dev
from image_generation_amd.modules import Decoder

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def _pm1(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (rows, cols), generator=g).float() * 2 - 1).contiguous()


def _one_tap(x, w, b=None, stats=False):
    """out = x @ w^T (+ b) through the 1-tap implicit GEMM: the (Cout, Cin) matrix sits at tap 0 of a Conv2d weight."""
    Cout, Cin = w.shape
    w9 = torch.zeros(Cout, Cin, 3, 3)
    w9[:, :, 0, 0] = w
    return dev.conv_igemm(x.cuda(), w9.cuda(), 0, x.shape[0], Cin, Cout, 0, ntaps=1, bias=None if b is None else b.cuda(),
                          stats=stats)


def _one_tap_wgrad(x, dy):
    """dW[co][ci] = sum_m dy[m][co] x[m][ci] through the 1-tap weight-gradient GEMM (read back from tap 0)."""
    (M, Cin), Cout = x.shape, dy.shape[1]
    gw = dev.conv_wgrad(x.cuda(), dy.cuda(), 0, (Cout, Cin, 3, 3), M, Cin, Cout, 0, ntaps=1)
    return gw[:, :, 0, 0].cpu()


SHAPES = [(37, 64, 256), (200, 32, 32), (1000, 96, 64), (300, 128, 128), (4100, 512, 512), (8100, 32, 512)]
# (37, 64, 256): 32x64 tiles, two chunks; (200, 32, 32): the 128x32 tile, a single chunk; (1000, 96, 64): three chunks (odd);
# (300, 128, 128): 32x64 tiles; (4100, 512, 512): 64x64 tiles, ragged last row block; (8100, 32, 512): 512 blocks of the
# 128x64 tile -- and the 128x128 tile forced (igemm_thr128 = 1) on those whose Cout allows it; with it (4100, 512, 512)
# also runs split over K (132 blocks): raw slabs, bias and BatchNorm partials from the reduce pass
CASES = [(s, 0) for s in SHAPES] + [(s, 1) for s in SHAPES[:5] if s[2] % 128 == 0]


@pytest.mark.parametrize("shape,thr128", CASES)
def test_spin_operand_gemm_is_float32_class(shape, thr128):
    rows, Cin, Cout = shape
    torch.manual_seed(rows + Cin)
    x = _pm1(rows, Cin, rows)
    w = torch.randn(Cout, Cin) / Cin**0.5
    b = torch.randn(Cout)
    y64 = x.double() @ w.double().T + b.double()
    opts = dict(igemm_thr128=1) if thr128 else {}
    with _lib.option_scope(**opts):
        out_f, _st_f = _one_tap(x, w, b, stats=True)
        with _lib.option_scope(dev_spin_operand=1):
            out, st = _one_tap(x, w, b, stats=True)
    e_s, e_f = _rel(out.cpu(), y64), _rel(out_f.cpu(), y64)
    print(f"spin form {e_s:.3e}  float32 form {e_f:.3e}")
    assert e_s < max(1e-6, 1.5 * e_f), (e_s, e_f)
    s = st.sum(0).cpu()
    assert _rel(s[:, 0], y64.sum(0)) < 1e-4 and _rel(s[:, 1], (y64 ** 2).sum(0)) < 1e-5


def test_spin_operand_gemm_under_the_split_mode_and_never_under_bf16_inputs():
    """Under f32x3 a promised launch goes from six products to three (same bar); bf16 inputs and the register-staged float32
    form never switch: their outputs with the promise are their outputs without it, bit for bit."""
    rows, Cin, Cout = 300, 128, 128
    torch.manual_seed(5)
    x, w = _pm1(rows, Cin, 5), torch.randn(Cout, Cin) / Cin**0.5
    y64 = x.double() @ w.double().T
    e_f = _rel(_one_tap(x, w).cpu(), y64)
    _lib.set_conv_precision("f32x3")
    try:
        with _lib.option_scope(dev_spin_operand=1):
            e_s = _rel(_one_tap(x, w).cpu(), y64)
    finally:
        _lib.set_conv_precision("f32")
    print(f"spin form under f32x3 {e_s:.3e}  float32 form {e_f:.3e}")
    assert e_s < max(1e-6, 1.5 * e_f), (e_s, e_f)
    _lib.set_conv_precision("bf16")
    try:
        plain = _one_tap(x, w)
        with _lib.option_scope(dev_spin_operand=1):
            assert torch.equal(_one_tap(x, w), plain)
    finally:
        _lib.set_conv_precision("f32")
    with _lib.option_scope(igemm_dma=0):
        plain = _one_tap(x, w)
        with _lib.option_scope(dev_spin_operand=1):
            assert torch.equal(_one_tap(x, w), plain)


@pytest.mark.parametrize("rows", [37, 1000, 4100])
@pytest.mark.parametrize("Cin,Cout", [(128, 128), (512, 512)])
def test_spin_operand_weight_gradient_is_float32_class(rows, Cin, Cout):
    """(4100 rows of 512 x 512 is where the 128 x 128 LDS-DMA kernel -- the one with a spin form -- serves the launch; the
    smaller launches take the kernels they always took, promise or not)"""
    torch.manual_seed(rows + Cout)
    x = _pm1(rows, Cin, rows + 1)
    dy = torch.randn(rows, Cout)
    g64 = dy.double().T @ x.double()
    g_f = _one_tap_wgrad(x, dy)
    with _lib.option_scope(dev_spin_operand=1):
        g_s = _one_tap_wgrad(x, dy)
    e_s, e_f = _rel(g_s, g64), _rel(g_f, g64)
    print(f"spin form {e_s:.3e}  float32 form {e_f:.3e}")
    assert e_s < max(1e-6, 1.5 * e_f), (e_s, e_f)


@pytest.mark.parametrize("pm1_data", [True, False])
def test_without_the_promise_or_with_dec_spin_gemm_off_nothing_changes(pm1_data):
    rows, Cin, Cout = 4100, 512, 512
    torch.manual_seed(11)
    x = _pm1(rows, Cin, 3) if pm1_data else torch.randn(rows, Cin)
    w, b, dy = torch.randn(Cout, Cin) / Cin**0.5, torch.randn(Cout), torch.randn(rows, Cout)
    out_f, g_f = _one_tap(x, w, b), _one_tap_wgrad(x, dy)
    assert _lib.get_option("dev_spin_operand") == 0 and _lib.get_option("dec_spin_gemm") == 1
    assert torch.equal(_one_tap(x, w, b), out_f)  # (no promise)
    with _lib.option_scope(dec_spin_gemm=0, dev_spin_operand=1):  # (a promise, ignored)
        assert torch.equal(_one_tap(x, w, b), out_f)
        assert torch.equal(_one_tap_wgrad(x, dy), g_f)
    with _lib.option_scope(dev_spin_operand=1):  # (the promise changes the arithmetic: the forms differ in the last bits)
        assert not torch.equal(_one_tap(x, w, b), out_f)


def _run_decoder(n, params, spins, masks, go, images, pm1, mse):
    dec = Decoder(n)
    dec.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    dec = dec.cuda().train()
    dec.inject_dropout_masks(masks)
    sg = spins.clone().requires_grad_(True)
    if mse:
        loss = dec.forward_mse(sg, images, spins_pm1=pm1)
        loss.backward()
        out = loss.detach().cpu()
    else:
        out = dec(sg, spins_pm1=pm1)
        (out * go).sum().backward()
        out = out.detach().cpu()
    return out, sg.grad.cpu(), {k: v.grad.cpu() for k, v in dec.named_parameters()}


def _close(got, want, rtol, name):
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max() + 1e-30
    err = np.abs(got - want).max()
    assert err <= rtol * scale + 1e-8, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("n,B,R,composed", [(512, 256, 8, True), (64, 16, 4, False)])
def test_decoder_with_and_without_the_promise(n, B, R, composed):
    """Forward + backward on +-1 spins with and without ``spins_pm1``, the head composed (N = 2048, n = 512) and layer by
    layer (N = 64, n = 64): reconstruction, spin gradient and every parameter gradient within the 2e-5 the project holds
    two equivalent head forms to; the ``forward`` and ``forward_mse`` routes agree with each other as they do without the
    promise (every gradient bit for bit); and with option dec_spin_gemm = 0 the promise changes nothing."""
    N = B * R
    assert dev.plan_forms("decoder", N, n)[1]["lc0"] == composed
    params = gen.make_params(n, "decoder", 31 + n)
    spins = torch.from_numpy(gen.make_spins(B, R, n, 17)).cuda()
    assert bool((spins.abs() == 1).all())
    masks = [torch.from_numpy(m).cuda() for m in gen.make_masks(N, 19)]
    go = torch.randn(B, R, 1, 32, 32, generator=torch.Generator().manual_seed(23)).cuda()
    images = torch.from_numpy(gen.make_images(B, 29)).cuda()
    plain = _run_decoder(n, params, spins, masks, go, images, False, False)
    spin = _run_decoder(n, params, spins, masks, go, images, True, False)
    assert not torch.equal(spin[0], plain[0]), "the promise did not reach the kernels"
    _close(spin[0], plain[0], 2e-5, "reconstruction")
    _close(spin[1], plain[1], 2e-5, "grad spins")
    for k, g in plain[2].items():
        if k.startswith("convtrans") and k.endswith("bias") and k.split(".")[1] in ("0", "5", "10", "15"):
            continue  # (zero true gradient in front of a BatchNorm: rounding noise only)
        _close(spin[2][k], g, 2e-5, k)
    # the two routes, both with the promise: what they share is bit for bit what it is without it
    spin_mse = _run_decoder(n, params, spins, masks, go, images, True, True)
    from image_generation_amd import functional as F
    dec = Decoder(n)
    dec.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    dec = dec.cuda().train()
    dec.inject_dropout_masks(masks)
    sg = spins.clone().requires_grad_(True)
    loss = F.replicated_mse_loss(dec(sg, spins_pm1=True), images)
    loss.backward()
    loss = float(loss.detach())
    assert abs(loss - float(spin_mse[0])) <= 2e-7 * abs(loss)
    assert torch.equal(sg.grad.cpu(), spin_mse[1])
    for k, v in dec.named_parameters():
        assert torch.equal(v.grad.cpu(), spin_mse[2][k]), k
    with _lib.option_scope(dec_spin_gemm=0):
        off = _run_decoder(n, params, spins, masks, go, images, True, False)
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
    for k, g in plain[2].items():
        assert torch.equal(off[2][k], g), k


def _rel_l2(got, want):
    got, want = got.double(), want.double()
    return float((got - want).norm() / (want.norm() + 1e-300))


@pytest.mark.parametrize("n,B,R", [(128, 256, 8), (512, 1024, 8), (1024, 64, 8)])
def test_decoder_full_size_with_the_promise_matches_float64_oracle_on_device(n, B, R):
    """``test_decoder_full_size_matches_float64_oracle_on_device`` (tests/test_gpu_fullsize.py: c2's, c3's and c5's
    networks against the oracle in float64 on the device) with ``spins_pm1=True``, held to that test's own bars: 2e-6 on
    the reconstruction, its L2 bars on the gradients."""
    from oracle import nets

    params = gen.make_params(n, "decoder", 77)
    dec = Decoder(n)
    dec.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    dec = dec.cuda().train()
    p = {k: (torch.from_numpy(np.array(v)).double().cuda().requires_grad_("running" not in k)
             if np.array(v).dtype == np.float32 else torch.from_numpy(np.array(v)).cuda()) for k, v in params.items()}
    spins = torch.from_numpy(gen.make_spins(B, R, n, 3)).cuda()
    masks = [torch.from_numpy(m).cuda() for m in gen.make_masks(B * R, 4)]
    go = torch.randn(B, R, 1, 32, 32, generator=torch.Generator().manual_seed(9)).cuda()
    s64 = spins.double().requires_grad_(True)
    want = nets.decoder_forward(p, s64, training=True, dropout_masks=[m.double() for m in masks])
    (want * go.double()).sum().backward()
    sg = spins.clone().requires_grad_(True)
    dec.inject_dropout_masks(masks)
    got = dec(sg, spins_pm1=True)
    (got * go).sum().backward()
    e = _rel_l2(got.detach(), want.detach())
    print(f"reconstruction against float64, promise on: {e:.3e}")
    assert e < 2e-6
    assert float((got.detach().double() - want.detach()).abs().max()) < 3e-5 * float(want.detach().abs().max())
    assert _rel_l2(sg.grad, s64.grad) < 2e-3
    for name, prm in dec.named_parameters():
        if name.startswith("convtrans") and name.endswith("bias") and name.split(".")[1] in ("0", "5", "10", "15"):
            continue  # bias in front of a BatchNorm: true gradient is zero, ours is rounding noise
        assert _rel_l2(prm.grad, p[name].grad) < (2e-3 if n <= 128 else 5e-3), name
