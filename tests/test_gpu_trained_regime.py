"""Network gradients against float64 at TRAINED-checkpoint parameters.

Every other gradient test draws its parameters from ``gen.make_params``: He-scale weights, BatchNorm weight 1 +- 0.1,
running variance about 1 -- the first step of a fresh run.  The one trained model in the tree
(tests/golden/ckpt_adv2_40*.npz, 18720 updates under weight decay) sits elsewhere: BatchNorm weights 0.31-0.55, weights of
standard deviation 3e-4 - 1e-2, batch / running variances at or below BatchNorm's eps of 1e-5 (the inverse standard
deviation is then set by eps: about 316), weight gradients of 300-800.  The shortcuts of the hot path (layer 0's patch
moments, zhat reconstructed from the pooled activations, the dense / composed first decoder layers, the fused decoder tail,
the Winograd transforms, the f32x3 split) were derived and had their bars measured on fresh values only.

Here: the encoder and the decoder in training mode on the checkpoint, every kernel form, both float32-class operand modes,
forward + every gradient + running statistics against oracle/nets.py in float64; synthetic regimes of the same kind at the
other latent sizes; the BatchNorm-backward guard just above its threshold; one whole training step from the loaded
checkpoint; Adam at trained magnitudes.  The bars are the ones of tests/test_gpu_nets.py and tests/test_gpu_headline.py,
unchanged, and the unmarked tests hold the float32 CPU oracle to ONE TENTH of each on the same inputs -- so a miss on the GPU
is the kernels', not the inputs'.
"""
import functools
import os

import numpy as np
import pytest
import torch

import gen
import test_gpu_nets as tgn
from image_generation_amd import _lib, dev
from image_generation_amd.modules import Decoder, Encoder
from image_generation_amd.plugin import DiscreteVariationalAutoencoder
from oracle import nets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the bars of test_gpu_nets.py (fractions of each tensor's largest magnitude in float64)
BAR_OUT, BAR_ENC_GRAD, BAR_DEC_GRAD, BAR_STAT = 3e-5, 1e-4, 2e-4, 1e-5
# a conv bias in front of a BatchNorm has a true gradient of exactly zero; what comes back is rounding noise of the sums
# behind the SAME convolution's weight gradient: held to this fraction of that weight gradient's largest entry
BAR_ZERO_BIAS = 1e-4


# ------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _ckpt_state_dict():
    fx = gen.load_npz_parts(os.path.join(GOLDEN, "ckpt_adv2_40.npz"))
    return {k[3:]: np.array(v) for k, v in fx.items() if k.startswith("sd/")}


def _ckpt_params(which):
    prefix = "_encoder." if which == "encoder" else "_decoder."
    return {k[len(prefix):]: v for k, v in _ckpt_state_dict().items() if k.startswith(prefix)}


def _rescaled_params(n, which, seed, s):
    """``gen.make_params`` moved to a trained-like regime by a power of two ``s`` (exact in float32): conv / convT / Linear
    weights and the conv biases in front of a BatchNorm x s, running mean x s, running variance x s^2 -- the pre-BatchNorm
    activations and their variance scale with them, against an eps that does not -- BatchNorm weight 0.31 (1 +- 0.03) and
    bias +- 0.01 as in the shipped checkpoint."""
    p = gen.make_params(n, which, seed)
    rng = np.random.default_rng(seed + 7)
    bn = {f"{'conv' if which == 'encoder' else 'convtrans'}.{(4 if which == 'encoder' else 5) * l + 1}" for l in range(4)}
    pre_bn = {f"{'conv' if which == 'encoder' else 'convtrans'}.{(4 if which == 'encoder' else 5) * l}" for l in range(4)}
    for k, v in p.items():
        mod, leaf = k.rsplit(".", 1)
        if mod in bn:
            if leaf == "weight":
                p[k] = (0.31 * (1.0 + 0.03 * rng.standard_normal(v.shape))).astype(np.float32)
            elif leaf == "bias":
                p[k] = (0.01 * rng.standard_normal(v.shape)).astype(np.float32)
            elif leaf == "running_mean":
                p[k] = (v * np.float32(s)).astype(np.float32)
            elif leaf == "running_var":
                p[k] = (v * np.float32(s) * np.float32(s)).astype(np.float32)
        elif leaf == "weight" or (leaf == "bias" and mod in pre_bn):
            p[k] = (v * np.float32(s)).astype(np.float32)
    return p


# name -> (parameters, n, B, min_gap of the tie-free search).  The synthetic encoder cases sit at s = 2^-6, not 2^-8: with
# BatchNorm weights of 0.31 and an inverse standard deviation capped by eps the activations shrink layer by layer, at
# s = 2^-8 the batch variances are 1e-6, 7e-8, 5e-9, 5e-10 (far below eps, not at it) and no batch has its pooling windows
# 3e-6 apart -- the widest smallest gap over 25 batches x 20 parameter seeds was 5.4e-7 at n = 64 and 4.0e-7 at n = 512, so
# float64 routes some windows otherwise than any float32 code (at 2^-7: 40 batches x 6 seeds, none).  At s = 2^-6 the batch
# variances are 2e-5, 7e-6, 4e-6, 3e-6 -- around eps -- and tie-free batches exist (parameter seeds chosen so that the search
# ends within 20 batches: index 15, 2 and 17).
ENC_CASES = {
    "ckpt": (lambda: _ckpt_params("encoder"), 256, 16, 3e-6),
    "s-6,n64": (lambda: _rescaled_params(64, "encoder", 77, 2.0 ** -6), 64, 16, 3e-6),
    "s-6,n512": (lambda: _rescaled_params(512, "encoder", 525, 2.0 ** -6), 512, 8, 3e-6),
    "s+6,n64": (lambda: _rescaled_params(64, "encoder", 76, 2.0 ** 6), 64, 24, 3e-6),
}
# name -> (parameters, n, B, R)
DEC_CASES = {
    "ckpt": (lambda: _ckpt_params("decoder"), 256, 8, 2),
    "s-8,n512": (lambda: _rescaled_params(512, "decoder", 21 + 512, 2.0 ** -8), 512, 4, 2),
    "s-10,n64": (lambda: _rescaled_params(64, "decoder", 21 + 64, 2.0 ** -10), 64, 5, 3),
    "s+6,n128": (lambda: _rescaled_params(128, "decoder", 21 + 128, 2.0 ** 6), 128, 8, 2),
}


def _oracle_dict(params, dtype):
    out = {}
    for k, v in params.items():
        t = torch.from_numpy(np.array(v))
        if t.dtype.is_floating_point:
            t = t.to(dtype)
            if "running" not in k:
                t.requires_grad_(True)
        out[k] = t
    return out


def _collect(out, p, spins_grad=None):
    """One call's results under flat names: the output, every gradient, the BatchNorm buffers afterwards."""
    r = {"out": out.detach().double().cpu()}
    for k, v in p.items():
        if "running" in k:
            r["stat/" + k] = v.detach().double().cpu()
        elif "num_batches" in k:
            r["nbt/" + k] = v.detach().cpu()
        else:
            r["grad/" + k] = v.grad.detach().double().cpu()
    if spins_grad is not None:
        r["grad/spins"] = spins_grad.detach().double().cpu()
    return r


def _encoder_oracle(params, x, gl, dtype):
    p = _oracle_dict(params, dtype)
    y = nets.encoder_forward(p, x.to(dtype), training=True)
    (y * gl.to(dtype)).sum().backward()
    return _collect(y, p)


def _decoder_oracle(params, spins, masks, go, dtype):
    p = _oracle_dict(params, dtype)
    sp = spins.detach().to(dtype).clone().requires_grad_(True)  # (a leaf of its own: the case's spins are shared)
    y = nets.decoder_forward(p, sp, training=True, dropout_masks=[m.to(dtype) for m in masks])
    (y * go.to(dtype)).sum().backward()
    return _collect(y, p, sp.grad)


@functools.lru_cache(maxsize=None)
def _enc_case(name):
    """Parameters, inputs and the float64 / float32 CPU oracle of an encoder case: computed once per process, shared."""
    make, n, B, min_gap = ENC_CASES[name]
    params = make()
    x = tgn._tie_free_images(params, n, B, min_gap=min_gap)
    gl = torch.randn(B, n, generator=torch.Generator().manual_seed(1))
    return dict(params=params, n=n, B=B, x=x, gl=gl, want=_encoder_oracle(params, x, gl, torch.float64),
                cpu32=_encoder_oracle(params, x, gl, torch.float32))


@functools.lru_cache(maxsize=None)
def _dec_case(name):
    make, n, B, R = DEC_CASES[name]
    params = make()
    spins = torch.from_numpy(gen.make_spins(B, R, n, 7))
    masks = [torch.from_numpy(m) for m in gen.make_masks(B * R, 8)]
    go = torch.randn(B, R, 1, 32, 32, generator=torch.Generator().manual_seed(2))
    return dict(params=params, n=n, B=B, R=R, spins=spins, masks=masks, go=go,
                want=_decoder_oracle(params, spins, masks, go, torch.float64),
                cpu32=_decoder_oracle(params, spins, masks, go, torch.float32))


# ------------------------------------------------------------------------------------------------------------ compare
def _zero_true_gradient(network, key):
    """``grad/conv.4.bias`` -> ``grad/conv.4.weight`` for the conv biases in front of a BatchNorm, else None."""
    parts = key.split(".")
    if not key.endswith(".bias") or len(parts) != 3:
        return None
    if network == "encoder" and parts[0] == "grad/conv" and int(parts[1]) % 4 == 0:
        return key[:-len("bias")] + "weight"
    if network == "decoder" and parts[0] == "grad/convtrans" and parts[1] in ("0", "5", "10", "15"):
        return key[:-len("bias")] + "weight"
    return None


def _errors(network, got, want):
    """name -> (error, bar, compared), error and bar as fractions of the float64 tensor's largest magnitude (no absolute
    term: a running variance here is 1e-7).  Zero-true-gradient biases (compared = False: there is nothing to compare
    with): of the largest weight gradient of their convolution."""
    grad_bar = BAR_ENC_GRAD if network == "encoder" else BAR_DEC_GRAD
    out = {}
    for k, w in want.items():
        g = got[k]
        assert tuple(g.shape) == tuple(w.shape), k
        if k.startswith("nbt/"):
            out[k] = (float(abs(int(g) - int(w))), 0.0, True)
            continue
        ref = _zero_true_gradient(network, k)
        if ref is not None:
            out[k] = (float(g.abs().max() / want[ref].abs().max()), BAR_ZERO_BIAS, False)
            continue
        bar = BAR_OUT if k == "out" else BAR_STAT if k.startswith("stat/") else grad_bar
        out[k] = (float((g - w).abs().max() / w.abs().max()), bar, True)
    return out


def _report(title, errs, beside=None):
    print(f"[trained-regime] {title}")
    for k, (e, bar, _) in errs.items():
        side = f"  float32 CPU oracle {beside[k][0]:.2e}" if beside is not None else ""
        print(f"[trained-regime]   {k:42s} {e:.2e}  bar {bar:.0e}{side}")


def _assert_within(errs, fraction=1.0):
    """``fraction`` of the bar for every tensor that is COMPARED with float64.  A zero-true-gradient bias is not: its exact
    value is zero whatever the inputs, so no input can be blamed for what comes back, and the whole bar holds for it on
    either device (float32 on the CPU leaves 1.2e-5 of the 1e-4 on the checkpoint's conv.0.bias, more where the variance
    is far below eps: the tests print it)."""
    bad = {k: (e, bar) for k, (e, bar, compared) in errs.items() if not e <= (fraction * bar if compared else bar)}
    assert not bad, bad


# ----------------------------------------------------------------------------- 1. CPU pins (these run without a GPU)
def test_fixture_is_in_the_trained_regime():
    sd = _ckpt_state_dict()
    bn_w = [v for k, v in sd.items() if v.ndim == 1 and k.endswith(".weight") and k[:-len("weight")] + "running_var" in sd]
    assert len(bn_w) == 8
    for w in bn_w:
        assert float(w.min()) > 0.25 and float(w.max()) < 0.6
    dec_var = [v for k, v in sd.items() if k.startswith("_decoder.") and k.endswith("running_var")]
    assert sum(float(np.median(v)) < 1e-5 for v in dec_var) >= 3  # (BatchNorm's eps: 1e-5)
    for k, v in sd.items():
        if k.startswith("_encoder.") and k.endswith("running_var"):
            assert float(v.max()) < 1e-3, k
        if v.ndim == 4 and v.size > 9:  # (every conv / convT but the decoder's last, 1 -> 1: nine numbers, 0.086)
            assert float(v.std()) < 2e-2, k
    assert float(sd["_decoder.increase_latent_dim.weight"].std()) < 2e-2


@pytest.mark.parametrize("s,which,n", [(2.0 ** -8, "encoder", 64), (2.0 ** -10, "decoder", 64), (2.0 ** 6, "decoder", 128)])
def test_rescaled_parameters_are_the_fresh_ones_moved_by_a_power_of_two(s, which, n):
    base, p = gen.make_params(n, which, 5), _rescaled_params(n, which, 5, s)
    stem = "conv" if which == "encoder" else "convtrans"
    step = 4 if which == "encoder" else 5
    for l in range(4):
        assert np.array_equal(p[f"{stem}.{step * l}.weight"], base[f"{stem}.{step * l}.weight"] * np.float32(s))
        assert np.array_equal(p[f"{stem}.{step * l}.bias"], base[f"{stem}.{step * l}.bias"] * np.float32(s))
        assert np.array_equal(p[f"{stem}.{step * l + 1}.running_var"], base[f"{stem}.{step * l + 1}.running_var"] * np.float32(s * s))
        assert np.array_equal(p[f"{stem}.{step * l + 1}.running_mean"], base[f"{stem}.{step * l + 1}.running_mean"] * np.float32(s))
        g, b = p[f"{stem}.{step * l + 1}.weight"], p[f"{stem}.{step * l + 1}.bias"]
        assert 0.25 < float(g.min()) and float(g.max()) < 0.37 and float(np.abs(b).max()) < 0.05
    lin = "projection" if which == "encoder" else "increase_latent_dim"
    assert np.array_equal(p[lin + ".weight"], base[lin + ".weight"] * np.float32(s))
    assert np.array_equal(p[lin + ".bias"], base[lin + ".bias"])  # (not in front of a BatchNorm)


@pytest.mark.parametrize("name", list(ENC_CASES))
def test_float32_cpu_oracle_is_within_a_tenth_of_the_encoder_bars(name):
    c = _enc_case(name)
    errs = _errors("encoder", c["cpu32"], c["want"])
    _report(f"encoder {name}: float32 CPU oracle against float64", errs)
    _assert_within(errs, 0.1)


@pytest.mark.parametrize("name", list(DEC_CASES))
def test_float32_cpu_oracle_is_within_a_tenth_of_the_decoder_bars(name):
    c = _dec_case(name)
    errs = _errors("decoder", c["cpu32"], c["want"])
    _report(f"decoder {name}: float32 CPU oracle against float64", errs)
    _assert_within(errs, 0.1)


# -------------------------------------------------------------------- 2. / 3. the networks on the GPU against float64
def _gpu_module(which, name, params, n):
    if name != "ckpt":
        return tgn._load(Encoder(n) if which == "encoder" else Decoder(n), params).train()
    dvae = DiscreteVariationalAutoencoder(Encoder(n), Decoder(n))
    missing, unexpected = dvae.load_state_dict({k: torch.from_numpy(v) for k, v in _ckpt_state_dict().items()}, strict=True)
    assert not missing and not unexpected
    return (dvae.encoder if which == "encoder" else dvae.decoder).cuda().train()


def _gpu_results(module, out, spins_grad=None):
    r = {"out": out.detach().double().cpu()}
    r.update({"grad/" + k: v.grad.detach().double().cpu() for k, v in module.named_parameters()})
    for k, v in module.state_dict().items():
        if "running" in k:
            r["stat/" + k] = v.detach().double().cpu()
        elif "num_batches" in k:
            r["nbt/" + k] = v.detach().cpu()
    if spins_grad is not None:
        r["grad/spins"] = spins_grad.detach().double().cpu()
    return r


def _encoder_gpu(name):
    c = _enc_case(name)
    enc = _gpu_module("encoder", name, c["params"], c["n"])
    y = enc(c["x"].cuda())
    (y * c["gl"].cuda()).sum().backward()
    torch.cuda.synchronize()
    return _gpu_results(enc, y)


def _decoder_gpu(name):
    c = _dec_case(name)
    dec = _gpu_module("decoder", name, c["params"], c["n"])
    dec.inject_dropout_masks([m.cuda() for m in c["masks"]])
    sg = c["spins"].detach().cuda().requires_grad_(True)
    y = dec(sg)
    (y * c["go"].cuda()).sum().backward()
    torch.cuda.synchronize()
    return _gpu_results(dec, y, sg.grad)


class _mode:
    """The process-wide operand mode for a block, put back afterwards."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.saved = _lib.get_conv_precision()
        _lib.set_conv_precision(self.mode)

    def __exit__(self, *exc):
        _lib.set_conv_precision(self.saved)
        return False


def _forms_taken(layers):
    return {f for layer in layers if layer is not None for f in layer}


def _wino(f):
    return f in ("wino2", "wino4")


# option set -> what dev.plan_forms must report for it at the checkpoint's shapes (16 rows, n = 256)
ENC_OPTION_SETS = {
    "default": (dict(), lambda L, F: all(L[l] == ("direct",) * 3 for l in (1, 2, 3))),  # (16 images: below the Winograd sizes)
    "enc_wino=0": (dict(enc_wino=0), lambda L, F: all(L[l] == ("direct",) * 3 for l in (1, 2, 3))),
    "enc_wino=1": (dict(enc_wino=1), lambda L, F: all(_wino(f) for l in (1, 2, 3) for f in L[l])
                   and {"wino2", "wino4"} <= _forms_taken(L) and L[1][1] == L[2][1] == L[3][2] == "wino4"),
    "enc_bn_reduce_pooled=1": (dict(enc_bn_reduce_pooled=1), lambda L, F: _lib.get_option("enc_bn_reduce_pooled") == 1),
    "enc_bn_reduce_pooled=0": (dict(enc_bn_reduce_pooled=0), lambda L, F: _lib.get_option("enc_bn_reduce_pooled") == 0),
    "enc_l0_fused=1": (dict(enc_l0_fused=1), lambda L, F: _lib.get_option("enc_l0_fused") == 1),
    "enc_l0_fused=0": (dict(enc_l0_fused=0), lambda L, F: _lib.get_option("enc_l0_fused") == 0),
}
DEC_OPTION_SETS = {
    "default": (dict(), lambda L, F: L[0] == ("d22",) * 3 and L[2] == ("fold",) * 3 and F == dict(d22=True, lc0=False, tail=True)),
    "dec_wino=1": (dict(dec_wino=1), lambda L, F: all(_wino(f) for l in (1, 2) for f in L[l]) and L[2][0] == "wino4"),
    "dec_lc0=0": (dict(dec_lc0=0), lambda L, F: L[0] == ("d22",) * 3 and not F["lc0"]),
    "dec_lc0=1": (dict(dec_lc0=1), lambda L, F: L[0] == ("lc0",) * 3 and F["lc0"]),
    "dec_d22=0": (dict(dec_d22=0), lambda L, F: L[0] == ("direct",) * 3 and not F["d22"]),
    "dec_fold=0": (dict(dec_fold=0), lambda L, F: L[2] == ("direct",) * 3 and L[1] == ("direct",) * 3),
    "dec_tail_fused=0": (dict(dec_tail_fused=0), lambda L, F: not F["tail"]),
}
X3_ENC = ("default", "enc_wino=1", "enc_l0_fused=0")
X3_DEC = ("default", "dec_lc0=1", "dec_d22=0", "dec_fold=0")
ENC_RUNS = [("f32", k) for k in ENC_OPTION_SETS] + [("f32x3", k) for k in X3_ENC]
DEC_RUNS = [("f32", k) for k in DEC_OPTION_SETS] + [("f32x3", k) for k in X3_DEC]


def _planned(network, rows, n, mode, options):
    """dev.plan_forms under an operand mode and an option set, both put back (no device needed)."""
    with _mode(mode), _lib.option_scope(**options):
        return dev.plan_forms(network, rows, n)


def test_the_checkpoint_runs_take_every_kernel_form():
    """(CPU: the planner needs no device.)  Across the option sets of the two checkpoint tests every name of ``dev.FORMS``
    is taken by some layer, and each option set selects the form it is there for."""
    taken = set()
    for mode, key in ENC_RUNS:
        layers, flags = _planned("encoder", 16, 256, mode, ENC_OPTION_SETS[key][0])
        with _lib.option_scope(**ENC_OPTION_SETS[key][0]):
            assert ENC_OPTION_SETS[key][1](layers, flags), (mode, key, layers, flags)
        taken |= _forms_taken(layers)
    for mode, key in DEC_RUNS:
        layers, flags = _planned("decoder", 16, 256, mode, DEC_OPTION_SETS[key][0])
        assert DEC_OPTION_SETS[key][1](layers, flags), (mode, key, layers, flags)
        taken |= _forms_taken(layers)
    assert taken == set(dev.FORMS), taken


@pytest.mark.gpu
@pytest.mark.parametrize("mode,key", ENC_RUNS)
def test_encoder_on_the_checkpoint_matches_float64(mode, key):
    """Training-mode forward, every parameter gradient and the BatchNorm buffers afterwards, on the shipped checkpoint
    (n = 256, strict load) and a tie-free batch of 16 continuous images."""
    c = _enc_case("ckpt")
    options, intended = ENC_OPTION_SETS[key]
    with _mode(mode), _lib.option_scope(**options):
        layers, flags = dev.plan_forms("encoder", c["B"], c["n"])
        assert intended(layers, flags), (layers, flags)
        got = _encoder_gpu("ckpt")
    errs = _errors("encoder", got, c["want"])
    _report(f"encoder ckpt [{mode}] {key}: forms {layers[1:]}", errs, _errors("encoder", c["cpu32"], c["want"]))
    _assert_within(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,key", DEC_RUNS)
def test_decoder_on_the_checkpoint_matches_float64(mode, key):
    """The same for the decoder (B = 8, R = 2, injected dropout masks), with the gradient wrt the spins."""
    c = _dec_case("ckpt")
    options, intended = DEC_OPTION_SETS[key]
    with _mode(mode), _lib.option_scope(**options):
        layers, flags = dev.plan_forms("decoder", c["B"] * c["R"], c["n"])
        assert intended(layers, flags), (layers, flags)
        got = _decoder_gpu("ckpt")
    errs = _errors("decoder", got, c["want"])
    _report(f"decoder ckpt [{mode}] {key}: forms {layers[:3]} {flags}", errs, _errors("decoder", c["cpu32"], c["want"]))
    _assert_within(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("network,options", [("encoder", dict(enc_wino=1, enc_wino4_mask=0x1ff)),
                                             ("decoder", dict(dec_wino=1, dec_wino4_mask=0xf))])
def test_non_default_winograd_masks_on_the_checkpoint_are_recorded(network, options):
    """The F(4x4,3x3) launches the default masks leave out (options.cpp says why, per bit: their bars are the full-size
    tests'): run and printed beside the others, held to finiteness only."""
    c = _enc_case("ckpt") if network == "encoder" else _dec_case("ckpt")
    with _lib.option_scope(**options):
        layers, flags = dev.plan_forms(network, c["B"] * c.get("R", 1), c["n"])
        got = _encoder_gpu("ckpt") if network == "encoder" else _decoder_gpu("ckpt")
    errs = _errors(network, got, c["want"])
    _report(f"{network} ckpt [f32] {options} (recorded only): forms {layers}", errs, _errors(network, c["cpu32"], c["want"]))
    assert all(np.isfinite(e) for e, _, _ in errs.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in ENC_CASES if k != "ckpt"])
@pytest.mark.parametrize("wino", [-1, 1])
def test_encoder_in_synthetic_trained_regimes_matches_float64(name, wino):
    """Fresh parameters moved by a power of two so that the batch variances sit at eps (s = 2^-6: see ENC_CASES) or far
    above it (s = 2^6), at latent sizes the checkpoint does not exist at; default forms and the Winograd forms."""
    c = _enc_case(name)
    with _lib.option_scope(enc_wino=wino):
        layers, _ = dev.plan_forms("encoder", c["B"], c["n"])
        assert (wino == 1) == any(_wino(f) for f in _forms_taken(layers)), layers
        got = _encoder_gpu(name)
    errs = _errors("encoder", got, c["want"])
    _report(f"encoder {name} [f32] enc_wino={wino}: forms {layers[1:]}", errs, _errors("encoder", c["cpu32"], c["want"]))
    _assert_within(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in DEC_CASES if k != "ckpt"])
@pytest.mark.parametrize("wino", [-1, 1])
def test_decoder_in_synthetic_trained_regimes_matches_float64(name, wino):
    """s = 2^-8 (variances about eps), 2^-10 (far below: the decoder has no pooling, so no tie-free batch is needed) and
    2^6 (the first layer's variance about 1e6)."""
    c = _dec_case(name)
    with _lib.option_scope(dec_wino=wino):
        layers, flags = dev.plan_forms("decoder", c["B"] * c["R"], c["n"])
        assert (wino == 1) == any(_wino(f) for f in _forms_taken(layers)), layers
        got = _decoder_gpu(name)
    errs = _errors("decoder", got, c["want"])
    _report(f"decoder {name} [f32] dec_wino={wino}: forms {layers[:3]} {flags}", errs, _errors("decoder", c["cpu32"], c["want"]))
    _assert_within(errs)


# -------------------------------------------------------------- 4. the BatchNorm-backward guard above its threshold
GUARD_KS = (1.2e-3, 5e-3, 5e-2)
# (layer, channels of that layer's BatchNorm): a whole channel quad (the kernel's guard is per quad of channels), and two
# quads with one such channel each
GUARD_CHANNELS = {1: ((8, 9, 10, 11), (21,), (34,)), 2: ((40, 41, 42, 43), (5,), (66,)), 3: ((16, 17, 18, 19), (2,), (61,))}


def _guard_params(k):
    """n = 64 encoder with, on a few channels of layers 1-3, BatchNorm bias +-3 and weight +-k (1 + |bias|): |bias / weight|
    is 0.75 / k, up to 625 -- zhat rebuilt from the pooled activation carries 6e-8 of that."""
    params = gen.make_params(64, "encoder", 31)
    for l, groups in GUARD_CHANNELS.items():
        w = np.array(params[f"conv.{4 * l + 1}.weight"], dtype=np.float32)
        b = np.array(params[f"conv.{4 * l + 1}.bias"], dtype=np.float32)
        for gi, group in enumerate(groups):
            for ci, ch in enumerate(group):
                b[ch] = 3.0 if (gi + ci) % 2 == 0 else -3.0
                w[ch] = k * 4.0 * (-1.0 if (gi + ci) % 3 == 1 else 1.0)
        params[f"conv.{4 * l + 1}.weight"], params[f"conv.{4 * l + 1}.bias"] = w, b
    return params


@pytest.mark.parametrize("k", GUARD_KS)
def test_guard_inputs_sit_just_above_the_threshold(k):
    """(CPU) the edited channels pass the guard, |weight| >= 1e-3 (1 + |bias|) -- so their zhat IS rebuilt from the pooled
    activation -- include negative weights, whole quads and lone channels, and leave the network finite in float32 and
    float64."""
    params = _guard_params(k)
    for l, groups in GUARD_CHANNELS.items():
        w, b = params[f"conv.{4 * l + 1}.weight"], params[f"conv.{4 * l + 1}.bias"]
        edited = [ch for group in groups for ch in group]
        assert all(abs(w[ch]) >= 1e-3 * (1 + abs(b[ch])) and abs(abs(b[ch] / w[ch]) - 0.75 / k) < 1e-3 / k for ch in edited)
        assert any(w[ch] < 0 for ch in edited) and any(b[ch] < 0 for ch in edited)
        assert len(groups[0]) == 4 and groups[0][0] % 4 == 0 and all(len(g) == 1 for g in groups[1:])
    x = (torch.rand(24, 1, 32, 32, generator=torch.Generator().manual_seed(3)) < 0.3).float()
    gl = torch.randn(24, 64, generator=torch.Generator().manual_seed(1))
    for dtype in (torch.float32, torch.float64):
        r = _encoder_oracle(params, x, gl, dtype)
        assert all(bool(torch.isfinite(v.double()).all()) for v in r.values())


@pytest.mark.gpu
@pytest.mark.parametrize("k", GUARD_KS)
def test_encoder_bn_backward_pooled_form_just_above_its_guard(k):
    """The pooled-activation form of the BatchNorm/pool backward sums (enc_bn_pool_bwd_reduce_p_kernel) against the window
    form on the same inputs, 2e-5 (the bar of test_encoder_bn_backward_sums_from_the_pooled_activations), with channels
    whose |bias / weight| reaches 625.  Such channels round pooling gaps away in float32, so float64 routes some windows
    differently; both forms read the same float32 activations and route alike, and the window form is held to float64 by
    test_encoder_on_the_checkpoint_matches_float64[enc_bn_reduce_pooled=0].  Measured on an MI355X: the BatchNorm weight
    gradients 1.0e-5 / 4.8e-6 / 4.6e-6 (layers 1-3) at k = 1.2e-3, everything else below 5e-7."""
    n, B = 64, 24
    params = _guard_params(k)
    x = (torch.rand(B, 1, 32, 32, generator=torch.Generator().manual_seed(3)) < 0.3).float()
    gl = torch.randn(B, n, generator=torch.Generator().manual_seed(1))
    grads = {}
    for form in (1, 0):
        with _lib.option_scope(enc_bn_reduce_pooled=form):
            enc = tgn._load(Encoder(n), params).train()
            (enc(x.cuda()) * gl.cuda()).sum().backward()
            grads[form] = {name: v.grad.detach().double().cpu() for name, v in enc.named_parameters()}
    errs = {}
    for name, g1 in grads[1].items():
        if _zero_true_gradient("encoder", "grad/" + name) is not None:
            continue
        errs[name] = (float((g1 - grads[0][name]).abs().max() / grads[0][name].abs().max()), 2e-5, True)
    _report(f"encoder BN-backward guard, k = {k:g}: pooled form against window form", errs)
    _assert_within(errs)


# ------------------------------------------------------------------- 5. one whole step from the loaded checkpoint
@pytest.mark.gpu
def test_one_training_step_from_the_shipped_checkpoint_matches_float64(tmp_path):
    """``ModelWrapper.load`` of the shipped Advantage2_system1 checkpoint (trained networks AND the trained GRBM on its
    own 2059-edge Zephyr sub-graph, |J| up to 4.9), then ONE noise-injected training step (B = 32, R = 2, 64 reads, 5
    sweeps) against the float64 oracle with the checks of the headline test: losses 1e-5, gradients 5e-3 relative L2
    (or stock float32's distance, capped), the GRBM's sufficient statistics."""
    import test_gpu_headline as tgh

    ck = gen.load_npz_parts(os.path.join(GOLDEN, "ckpt_adv2_40.npz"))
    fx = dict(np.load(os.path.join(GOLDEN, "grbm_ckpt.npz")))
    folder = tmp_path / "Advantage2_system1_40_epochs"
    folder.mkdir()
    torch.save({k[3:]: torch.from_numpy(np.array(v)) for k, v in ck.items() if k.startswith("sd/")}, folder / "dvae.pth")
    ei, ej = fx["zephyr/edge_i"].astype(np.int64), fx["zephyr/edge_j"].astype(np.int64)
    empty = torch.zeros(0, dtype=torch.int64)
    torch.save({"_linear": torch.from_numpy(fx["zephyr/linear"]), "_quadratic": torch.from_numpy(fx["zephyr/quadratic"]),
                "_edge_idx_i": torch.from_numpy(ei), "_edge_idx_j": torch.from_numpy(ej), "_visible_idx": torch.arange(256),
                "_hidden_idx": empty, "_flat_adj": empty, "_flat_j_idx": empty, "_bin_idx": empty}, folder / "grbm.pth")

    def prepare(m):
        m.load(folder)
        assert m.sampler.plan.n_edges == 2059 and int(m._dvae.state_dict()["_encoder.conv.1.num_batches_tracked"]) == 18720
        assert float(m._grbm._quadratic.abs().max()) > 4.5

    cfg = dict(B=32, n=256, R=2, C=64, sweeps=5, qpu="Advantage2_system1")
    worst = tgh._check_step_against_float64(tmp_path, cfg, 5e-3, prepare=prepare)
    print("[trained-regime] whole step from the checkpoint: gradient rel-L2 against float64:",
          {k: f"{v:.2e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])})


# ----------------------------------------------------------------------------------- 6. Adam at trained magnitudes
@pytest.mark.gpu
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adam_matches_torch_at_trained_magnitudes(grad_scale, weight_decay):
    """Parameters of 1e-3 and, in ONE tensor, gradients from 1e-12 to 1e3 -- the trained networks' 300-800 beside the 1e-11
    noise of a zero-true-gradient bias, where sqrt(v) sits below Adam's eps -- five steps against torch.optim.Adam in
    float64 on pre-scaled gradients: each parameter to 1e-6 relative plus 1e-6 of the step size."""
    n, lr0 = 4099, 1e-4
    gen_ = torch.Generator().manual_seed(6)
    p0 = (1e-3 * torch.randn(n, generator=gen_)).float()
    ladder = 10.0 ** torch.linspace(-12.0, 3.0, n, dtype=torch.float64)
    assert int(((ladder > 3e-12) & (ladder < 3e-11)).sum()) > 100 and float(ladder[-1]) == 1e3
    ref = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=lr0, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    p = p0.clone().cuda(); m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    L = _lib.lib()
    for step in range(1, 6):
        sign = torch.where(torch.rand(n, generator=gen_) < 0.5, -1.0, 1.0).double()
        g = (ladder * sign * (0.5 + torch.rand(n, generator=gen_).double())).float()  # (what the kernel reads: float32)
        ref.grad = g.double() * grad_scale
        lr = lr0 * 0.9 ** step
        for grp in opt.param_groups:
            grp["lr"] = lr
        opt.step()
        gd = g.cuda()
        _lib.check(L.dvg_adam_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, 0.9, 0.999, 1e-8,
                                   weight_decay, step, grad_scale, None, 0, _lib.stream_ptr()))
    torch.cuda.synchronize()
    want = ref.detach()
    err = (p.cpu().double() - want).abs()
    bound = 1e-6 * want.abs() + 1e-6 * lr
    print(f"[trained-regime] Adam grad_scale={grad_scale} weight_decay={weight_decay}: worst error / bound "
          f"{float((err / bound).max()):.3f}, moved by up to {float((want - p0.double()).abs().max()):.2e}")
    assert bool((err <= bound).all()), float((err / bound).max())
