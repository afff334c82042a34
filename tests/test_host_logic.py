"""Host-side logic that needs no GPU: the picture grid of the generation entry points, the data-parallel sharding of
the input pipeline, the reference-named ``ModelWrapper`` entry points (/root/reference/src/model_wrapper.py:355-491)."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from image_generation_amd import data, viz
from image_generation_amd.model_wrapper import ModelWrapper


def test_make_grid_layout():
    imgs = torch.arange(5 * 2 * 3, dtype=torch.float32).reshape(5, 1, 2, 3)
    g = viz.make_grid(imgs, nrow=4, padding=1, pad_value=-1.0)
    assert g.shape == (3, 2 * 3 + 1, 4 * 4 + 1)  # 2 rows x 4 columns of (2+1) x (3+1) cells, + the closing frame
    assert torch.equal(g[0], g[1]) and torch.equal(g[1], g[2])  # single channel replicated
    assert torch.equal(g[0, 1:3, 1:4], imgs[0, 0]) and torch.equal(g[0, 1:3, 13:16], imgs[3, 0])
    assert torch.equal(g[0, 4:6, 1:4], imgs[4, 0])
    assert bool((g[0, 0] == -1).all()) and bool((g[0, :, 0] == -1).all()) and bool((g[0, 4:6, 5:] == -1).all())
    g0 = viz.make_grid(imgs[:4], nrow=16, padding=0)
    assert g0.shape == (3, 2, 12) and torch.equal(g0[0, :, 3:6], imgs[1, 0])


def test_sharpen_rule():
    x = torch.tensor([0.0, 0.39, 0.4, 0.41, 0.6, 0.61, 1.0])
    assert viz.LOWER_THRESHOLD == 0.4 and viz.UPPER_THRESHOLD == 0.6  # /root/reference/demo_configs.py:62-63
    # H(0) = 0 on both thresholds: 0.4 -> 0, 0.6 stays
    np.testing.assert_allclose(viz.sharpen(x).numpy(), [0.0, 0.0, 0.0, 0.41, 0.6, 1.0, 1.0])


def test_tensor_batches_shards_are_disjoint_and_cover_one_permutation():
    imgs = torch.arange(103, dtype=torch.float32).reshape(103, 1, 1, 1)
    labels = torch.zeros(103, dtype=torch.int64)
    one = data.TensorBatches(imgs, labels, 5, seed=9)
    ranks = [data.TensorBatches(imgs, labels, 5, seed=9, rank=r, world_size=4) for r in range(4)]
    assert len(one) == 20 and all(len(r) == 5 for r in ranks)  # (103 // 4) // 5
    for _epoch in range(2):  # the permutation generator advances identically on every rank
        whole = torch.cat([b for b, _ in one]).flatten()
        seen = [torch.cat([b for b, _ in r]).flatten() for r in ranks]
        allv = torch.cat(seen)
        assert len(set(allv.tolist())) == allv.numel() == 100
        # rank r holds entries r, r + 4, ... of the same permutation the single-rank loader walks
        perm = torch.cat([whole, torch.tensor(sorted(set(range(103)) - set(whole.tolist())), dtype=torch.float32)])
        for r in range(4):
            assert set(seen[r].tolist()) <= set(perm.tolist())
    a = [b.flatten().tolist() for b, _ in data.TensorBatches(imgs, labels, 5, seed=9, rank=1, world_size=4)]
    b = [b.flatten().tolist() for b, _ in data.TensorBatches(imgs, labels, 5, seed=9, rank=1, world_size=4)]
    assert a == b


def test_reference_entry_points_exist_with_the_reference_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(ModelWrapper.generate_output) == ["self", "latent_qpu_file", "sharpen", "save_to_file"]
    assert sig(ModelWrapper.generate_reconstucted_samples) == ["self", "sharpen", "save_to_file"]
    assert sig(ModelWrapper.generate_loss_plot) == ["self", "save_to_file_mse", "save_to_file_total", "old_loss_data"]
    for name in ("setup", "train_init", "step", "save", "load", "_load_dataset"):
        assert callable(getattr(ModelWrapper, name))


def test_generate_loss_plot_figures_and_side_files(tmp_path, golden_dir):
    pytest.importorskip("plotly")
    m = ModelWrapper("Advantage_system4", n_latents=64, training_parameter_file=os.path.join(golden_dir, "step_params.yaml"))
    m.losses = {"mse_losses": [0.3, torch.tensor(0.2)], "dvae_losses": [0.5, torch.tensor(0.4)]}
    old = {"mse_losses": [0.9], "dvae_losses": [1.1]}
    f_mse, f_tot = m.generate_loss_plot(str(tmp_path / "mse.json"), str(tmp_path / "tot.json"), old_loss_data=old)
    np.testing.assert_allclose(list(f_mse.data[0].y), [0.9, 0.3, 0.2], rtol=1e-6)
    np.testing.assert_allclose(list(f_tot.data[0].y), [1.1, 0.5, 0.4], rtol=1e-6)
    assert list(f_tot.data[0].x) == [0, 1, 2] and f_mse.layout.xaxis.title.text == "Batch" and f_mse.layout.yaxis.title.text == "Loss"
    d = json.load(open(tmp_path / "tot.json"))
    assert d["data"][0]["type"] == "scatter" and d["layout"]["margin"] == {"t": 0, "l": 0, "b": 0, "r": 0}


def test_dataset_size_is_the_references_random_split_subset():
    """/root/reference/src/model_wrapper.py:96-100: ``random_split(dataset, [k, n - k])[0]`` -- a random subset drawn from
    torch's global generator, not the first k images; data-parallel ranks (seeded form) agree among themselves."""
    torch.manual_seed(5)
    want = torch.utils.data.random_split(range(1000), [100, 900])[0].indices
    torch.manual_seed(5)
    got = data.random_subset_indices(1000, 100)
    assert got.tolist() == want and sorted(want) != list(range(100)) and len(set(want)) == 100
    a, b = data.random_subset_indices(1000, 100, seed=3), data.random_subset_indices(1000, 100, seed=3)
    assert torch.equal(a, b) and not torch.equal(a, got)
    with pytest.raises(ValueError):
        data.random_subset_indices(10, 11)
    torch.manual_seed(5)
    dl = data.get_dataloader(32, 10, dataset_size=100, seed=1, device="cpu")
    assert len(dl) == 10 and dl.images.shape == (100, 1, 32, 32)


def test_schedule_decisions_of_the_wrapper_need_no_gpu():
    """Round 4's host-side schedule decisions: the decoder's weight-only prologue is forked only from
    ``PREPARE_DECODER_ROWS`` decoder rows up (a fork costs a captured step more than the prologue takes below that) unless
    ``prepare_decoder`` forces it; on a CPU device both the preparation and the device-hold of the join measurement are
    no-ops; the MMD-join decision takes the LARGEST measured lag (a host-bound sample reads ~0)."""
    from image_generation_amd.modules import Decoder

    m = ModelWrapper.__new__(ModelWrapper)
    m.prepare_decoder, m._prep_stream, m._device, m.N_REPLICAS = None, None, torch.device("cpu"), 8
    assert ModelWrapper.PREPARE_DECODER_ROWS == 32768
    m._prepare_decoder(torch.zeros(4096, 1, 32, 32), None)   # 32768 rows, but no GPU: nothing happens
    assert m._prep_stream is None
    m.n_latents = 1024                                        # (round 6: ... and from 512 latent spins up, rows x spins >= 2^20)
    m._prepare_decoder(torch.zeros(256, 1, 32, 32), None)
    assert m._prep_stream is None
    m.overlap_sampler = m.overlap_mmd = True
    m.sampler = None
    m._hold_device_while_measuring(4096 * 8)                  # (returns before touching torch.cuda)
    dec = Decoder(32)
    dec.prepare(64, None)                                     # CPU parameters: a no-op, nothing pending
    assert dec._prepared is None
    # the decision rule itself
    m.DEFER_SAMPLES, m.DEFER_LAG_MS = 2, 0.05
    rec = {"decision": None, "events": [], "lags": [0.004, 0.9]}
    m.__dict__["_defer_state"] = {((16, 32), (4, 32), 0): rec}

    class _Ev:  # two already-synchronised "event pairs" whose lags are 0.004 and 0.9 ms
        def __init__(self, v): self.v = v
        def synchronize(self): pass
        def elapsed_time(self, other): return other.v - self.v
    rec["lags"], rec["events"] = [], [(_Ev(0.0), _Ev(0.004)), (_Ev(0.0), _Ev(0.9))]
    m.__dict__["_defer_rec"] = rec
    assert m._defer_undecided() is True                       # (a shape still being measured is not captured into a graph)
    assert m._defer_mmd_join(torch.empty(16, 32), torch.empty(4, 32)) is True and rec["lags"] == [0.004, 0.9]
    assert m._defer_undecided() is False and m.__dict__["_defer_by_rows"][16] is rec


# Which kernel form every MFMA convolution layer takes (forward, data gradient, weight gradient) at the benchmark
# configurations under the default options.  Transcribed from the arrays the planners carried BEFORE the forms became one
# enum per pass (fold / wino / wino4 flags, resolved by the priority of the launch code: F(4x4) over F(2x2) over composed /
# dense / folded over direct), not from the code under test: a threshold edit that moves a configuration to another
# form has to change this table knowingly.
_D, _F, _W2, _W4 = "direct", "fold", "wino2", "wino4"
_DIRECT3, _FOLD3 = (_D, _D, _D), (_F, _F, _F)
_ENC_ALL_DIRECT = [None, _DIRECT3, _DIRECT3, _DIRECT3]
_DEC_SMALL = [("d22",) * 3, _FOLD3, _FOLD3, None]
_DEC_SMALL_LC0 = [("lc0",) * 3, _FOLD3, _FOLD3, None]
_PLANS = {  # (config, bf16-input mode): encoder in training mode, encoder in evaluation mode, decoder, the decoder's lc0
    ("c1", 0): (_ENC_ALL_DIRECT, _ENC_ALL_DIRECT, _DEC_SMALL, False),
    ("c1", 1): (_ENC_ALL_DIRECT, _ENC_ALL_DIRECT, _DEC_SMALL, False),
    ("c2", 0): (_ENC_ALL_DIRECT, [None, (_W2, _D, _D), _DIRECT3, _DIRECT3], _DEC_SMALL, False),
    ("c2", 1): (_ENC_ALL_DIRECT, _ENC_ALL_DIRECT, _DEC_SMALL, False),
    ("c3", 0): ([None, (_W2, _W4, _W2), (_W2, _W4, _W2), (_W4, _W4, _W4)],
                [None, (_W2, _D, _D), (_W2, _D, _D), (_W4, _D, _D)],
                [("lc0",) * 3, (_W2, _W2, _W2), (_W4, _W2, _W2), None], True),
    ("c3", 1): ([None, (_D, _D, _W2), (_D, _D, _W2), (_D, _D, _W4)], _ENC_ALL_DIRECT,
                [("lc0",) * 3, (_F, _F, _W2), (_F, _F, _W2), None], True),
    ("c5", 0): (_ENC_ALL_DIRECT, [None, (_W2, _D, _D), _DIRECT3, (_W2, _D, _D)], _DEC_SMALL_LC0, True),
    ("c5", 1): (_ENC_ALL_DIRECT, _ENC_ALL_DIRECT, _DEC_SMALL_LC0, True),
}
_SHAPES = {"c1": (64, 8, 64), "c2": (256, 8, 128), "c3": (4096, 8, 512), "c5": (256, 8, 1024)}  # batch, replicas, n_latents


@pytest.mark.parametrize("config,bf16", sorted(_PLANS))
def test_benchmark_configurations_take_the_pinned_kernel_forms(config, bf16):
    from image_generation_amd import _lib, dev
    L = _lib.lib()
    B, R, n = _SHAPES[config]
    enc_train, enc_eval, dec, lc0 = _PLANS[(config, bf16)]
    _lib.check(L.dvg_reset_options(), "dvg_reset_options")
    before = L.dvg_get_conv_precision()
    assert L.dvg_set_conv_precision(bf16) == 0
    try:
        assert dev.plan_forms("encoder", B, n, training=True) == (enc_train, dict(d22=False, lc0=False, tail=False))
        assert dev.plan_forms("encoder", B, n, training=False) == (enc_eval, dict(d22=False, lc0=False, tail=False))
        for training in (True, False):  # (the decoder's plan does not depend on the mode)
            assert dev.plan_forms("decoder", B * R, n, training=training) == (dec, dict(d22=True, lc0=lc0, tail=True))
    finally:
        assert L.dvg_set_conv_precision(before) == 0


# Which kernels one MMD call launches at the benchmark configurations' shapes (x rows, y rows, latent width).  Transcribed
# from the behaviour of the commit BEFORE the call got its plan (csrc/mmd_plan.h), not from the code under test: forms,
# template arguments and grids (in workgroups) from that commit's kernel-trace rows (profiles/r08_mmd_trace_parent.txt),
# workspace bytes and priced work from its dvg_mmd_workspace_bytes / dvg_mmd_spin_flops.  A threshold edit that moves a
# configuration to another form has to change this table knowingly.
_MMD_SHAPES = {"c1": (512, 256, 64), "c2": (2048, 256, 128), "c3": (32768, 256, 512), "c5": (2048, 2048, 1024)}
_MMD_PLANS = {  # (config, options): pair kernel, its template arguments and grid; gated float32 launch (NFB, grid) or None;
    # distance-sum kernel, its argument and grid; Gram pipe; final kernel's grid; workspace bytes; int8 FLOPs, bf16 FLOPs, terms
    ("c1", ()): ("sliced", dict(NFB=2), (24, 6, 1), None, "spin", 4, (3, 7), "int8", 128,
                 943616, 58720256.0, 150994944.0, 3),
    ("c2", ()): ("fq", dict(NFBW=1), (72, 4, 1), None, "spin", 4, (9, 19), "int8", 1024,
                 5101568, 1224736768.0, 3623878656.0, 3),
    ("c3", ()): ("w128", dict(NST=16, NFT=16, ONE=False), (258, 1, 1), (8, 512), "spin256", 16, (64, 8), "fp4", 1,
                 59357184, 1108168671232.0, 2216203124736.0, 2),
    ("c5", ()): ("w128", dict(NST=32, NFT=8, ONE=True), (32, 4, 4), (8, 512), "spin", 32, (16, 32), "int8", 2048,
                 46203648, 77309411328.0, 34359738368.0, 2),
    ("c3", (("mmd_gram_fp4", 0),)): ("w128", dict(NST=16, NFT=16, ONE=False), (258, 1, 1), (8, 512), "spin256", 16, (64, 8), "int8", 1,
                                     59357184, 1108168671232.0, 2216203124736.0, 2),
    ("c2", (("mmd_w128", 1), ("mmd_d256", 1))): ("w128", dict(NST=4, NFT=4, ONE=False), (18, 4, 1), (4, 288), "spin256", 4, (64, 8), "int8", 1024,
                                                  5104128, 1224736768.0, 2415919104.0, 2),
}


def _align256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("config,options", sorted(_MMD_PLANS))
def test_benchmark_mmd_shapes_take_the_pinned_kernel_forms(config, options):
    import ctypes

    from image_generation_amd import _lib, dev
    L = _lib.lib()
    nx, ny, d = _MMD_SHAPES[config]
    pair, params, pair_grid, gated, dist, dist_ns, dist_grid, gram, final_grid, ws, i8, b16, terms = _MMD_PLANS[(config, options)]
    _lib.check(L.dvg_reset_options(), "dvg_reset_options")
    with _lib.option_scope(**dict(options)):
        p = dev.mmd_plan(nx, ny, d)
        assert (p["pair"], p["pair_params"], p["pair_grid"]) == (pair, params, pair_grid)
        assert (p["gated_f32"], p["gated_nfb"], p["gated_grid"]) == ((True,) + gated if gated else (False, 0, 0))
        assert (p["dist"], p["dist_ns"], p["dist_grid"]) == (dist, dist_ns, dist_grid)
        assert p["gram"] == gram and p["final_grid"] == final_grid
        assert (p["splits"], p["slices"]) == pair_grid[1:] and p["dist_splits"] == dist_grid[1]
        # the priced work comes out of the same plan
        f8, f16, t = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _lib.check(L.dvg_mmd_spin_flops(nx, ny, d, ctypes.byref(f8), ctypes.byref(f16), ctypes.byref(t)), "dvg_mmd_spin_flops")
        assert (f8.value, f16.value, t.value) == (i8, b16, terms)
        assert (p["gram_passes"], p["bf16_terms"]) == (pair_grid[2] if pair == "w128" else 1, terms)
        # ... and so does the workspace: the total is dvg_mmd_workspace_bytes, and the layout rebuilt from the plan's counts
        # (loss partials among them; at these shapes the gradient slabs are the pair form's splits) gives the same total
        assert p["workspace_bytes"] == ws == L.dvg_mmd_workspace_bytes(nx, ny, d)
        rows32 = -(-nx // 128) * 4 + -(-ny // 128) * 4  # 32-row blocks of the transposed copy: whole 128-row tiles
        segments = [4 * (nx + ny), 4 * 16, 8 * dist_grid[0] * dist_grid[1], 8 * 3 * p["loss_parts"],
                    4 * p["splits"] * nx * d if p["splits"] > 1 else 0, 4, (nx + ny) * d, rows32 * d * 32 * 2, 2 * (d + 1) * 16,
                    (nx + ny) * d // 2 if d in (256, 512) else 0]
        assert sum(_align256(s) for s in segments) == ws


def test_launch_form_hooks_report_the_launchers_rules():
    """dev.conv_igemm_form / dev.conv_wgrad_form / dev.conv_wino_shape (no device): the launchers' own decisions, which the
    under-load tests assert their instantiations through.  The expected values follow from the rules written in the
    launchers: the block tile from the block counts (csrc/conv_igemm.hip: 128x128 from 512 such blocks at Cout % 128 == 0,
    128x64 from 512, 64x64 from 96, else 32x64; 128x32 at Cout % 64 != 0), split K below 192 blocks (at most a third of the
    K iterations), the operand form from the operand mode and the spin promise; the weight gradient's channel tile from
    the channel counts and its 1-tap 128 x 128 kernel from 256 blocks of 256 rows."""
    from image_generation_amd import _lib, dev
    _lib.check(_lib.lib().dvg_reset_options(), "dvg_reset_options")
    form = dev.conv_igemm_form
    assert form(262144, 64, 128, 3) == dict(tile=(128, 128), pm=3, ksplit=1, posmajor=True)       # 2048 blocks of 128 x 128
    assert form(65536, 32, 64, 3) == dict(tile=(128, 64), pm=3, ksplit=1, posmajor=True)          # 512 blocks of 128 x 64
    assert form(65408, 32, 64, 3)["tile"] == (64, 64)                                             # 511
    assert form(16384, 64, 64, 3) == dict(tile=(64, 64), pm=3, ksplit=1, posmajor=True)           # 256 blocks: unsplit
    # 32 blocks of 64 x 64 -> 64 of 32 x 64; 36 K iterations of two 32-channel taps: ceil(512 / 64) = 8 <= 36 / 3
    assert form(2048, 256, 64, 2) == dict(tile=(32, 64), pm=3, ksplit=8, posmajor=False)
    assert form(16384, 64, 96, 3)["tile"] == (128, 32)
    assert not form(16384, 64, 64, 3, ups=1)["posmajor"] and not form(16384, 64, 64, 3, poolsum=1)["posmajor"]
    assert form(16384, 512, 512, 0, ntaps=1) == dict(tile=(128, 128), pm=3, ksplit=1, posmajor=False)  # 512 blocks exactly
    assert form(16384 - 128, 512, 512, 0, ntaps=1)["tile"] == (128, 64)                               # 508: 1016 of 128 x 64
    with _lib.option_scope(igemm_posmajor=0):
        assert not form(16384, 64, 64, 3)["posmajor"]
    with _lib.option_scope(igemm_dma=0):
        assert form(16384, 64, 64, 3)["pm"] == 0
    try:
        for mode, pm, pm_spin in (("f32", 3, 6), ("f32x3", 4, 6), ("bf16", 5, 5)):
            _lib.set_conv_precision(mode)
            assert form(16384, 64, 128, 3)["pm"] == pm
            with _lib.option_scope(dev_spin_operand=1):
                assert form(16384, 64, 128, 3)["pm"] == pm_spin
                with _lib.option_scope(dec_spin_gemm=0):
                    assert form(16384, 64, 128, 3)["pm"] == pm
                if mode == "bf16":
                    assert not dev.conv_wgrad_form(16384, 256, 256, ntaps=1)["spin"]
    finally:
        _lib.set_conv_precision("f32")
    with pytest.raises(_lib.DvgError):
        form(16384, 16, 64, 3)
    wform = dev.conv_wgrad_form
    for Cin, Cout in ((128, 96), (96, 128), (96, 96), (128, 128)):
        tile = (64 if Cin % 64 == 0 else 32, 64 if Cout % 64 == 0 else 32)
        assert wform(16384, Cin, Cout) == wform(16384, Cin, Cout, ups=1) == dict(tile=tile, dma=True, tap1_dma=False, spin=False)
        with _lib.option_scope(wgrad_dma=0):
            assert not wform(16384, Cin, Cout)["dma"]
    assert wform(16384, 256, 256, ntaps=1) == dict(tile=(128, 128), dma=True, tap1_dma=True, spin=False)  # 4 x 64 blocks
    assert wform(16384 - 256, 256, 256, ntaps=1) == dict(tile=(64, 64), dma=False, tap1_dma=False, spin=False)  # 4 x 63
    assert wform(65536, 128, 384, ntaps=1)["tile"] == (128, 128) and not wform(65536, 128, 192, ntaps=1)["tap1_dma"]
    with _lib.option_scope(dev_spin_operand=1):
        assert wform(16384, 256, 256, ntaps=1)["spin"] and not wform(16384, 128, 96)["spin"]
        with _lib.option_scope(dec_spin_gemm=2):
            assert not wform(16384, 256, 256, ntaps=1)["spin"]
    with _lib.option_scope(wgrad_dma=0):
        assert not wform(16384, 256, 256, ntaps=1)["tap1_dma"]
    # the F(2x2) shape query does not look at option enc_wino: whole tile blocks (256 rows at Cout % 64 == 0, else 512)
    with _lib.option_scope(enc_wino=0):
        assert not dev.conv_wino_ok(256, 16, 64, 2)
        assert dev.conv_wino_shape(256, 16, 64, 2) and not dev.conv_wino_shape(128, 16, 64, 2)
        assert dev.conv_wino_shape(512, 8, 32, 3) and not dev.conv_wino_shape(256, 8, 32, 3) and not dev.conv_wino_shape(256, 8, 64, 2)
