"""The six checkpoints shipped with the reference (models/*/{dvae,grbm}.pth) load UNCHANGED into the
MI355X-native modules (strict state_dict match: SURVEY.md App. B).  The checkpoints are 25 MB of third-party data; what
these tests read of them is committed under tests/golden/ (make_golden.py ``ref_checkpoints``): every state_dict key in
order with its shape, the GRBM states, the small DVAE tensors, and all of one checkpoint's DVAE weights
(ckpt_adv2_40.npz).  The other checkpoints' large weights are seeded stand-ins of their shapes."""
import os

import numpy as np
import pytest
import torch

import gen
from image_generation_amd.model_wrapper import ModelWrapper
from image_generation_amd.modules import Decoder, Encoder
from image_generation_amd.plugin import DiscreteVariationalAutoencoder, GraphRestrictedBoltzmannMachine
from oracle import nets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FX = gen.load_npz_parts(os.path.join(GOLDEN, "ref_checkpoints.npz"))
MODELS = sorted({k.split("/")[0] for k in FX})
FULL = "Advantage2_system1_40_epochs"  # (its DVAE weights are committed whole: ckpt_adv2_40.npz)


def _checkpoint(name):
    """(dvae state_dict, grbm state_dict) of the shipped checkpoint ``name``, keys in the file's order."""
    full = {k[3:]: v for k, v in gen.load_npz_parts(os.path.join(GOLDEN, "ckpt_adv2_40.npz")).items()
            if k.startswith("sd/")} if name == FULL else {}
    rng = np.random.default_rng(sum(map(ord, name)))
    dvae = {}
    for k in FX[f"{name}/dvae_keys"].tolist():
        if f"{name}/dvae/{k}" in FX:
            dvae[k] = torch.from_numpy(np.array(FX[f"{name}/dvae/{k}"]))
        elif k in full:
            dvae[k] = torch.from_numpy(np.array(full[k]))
        else:
            shape = tuple(FX[f"{name}/dvae_shape/{k}"].tolist())
            fan_in = int(np.prod(shape[1:])) or 1
            dvae[k] = torch.from_numpy((rng.standard_normal(shape) / np.sqrt(fan_in)).astype(np.float32))
    grbm = {k: torch.from_numpy(np.array(FX[f"{name}/grbm/{k}"])) for k in FX[f"{name}/grbm_keys"].tolist()}
    return dvae, grbm


def test_fixture_holds_the_six_shipped_checkpoints():
    assert len(MODELS) == 6 and FULL in MODELS


@pytest.mark.parametrize("name", MODELS)
def test_reference_checkpoint_loads_strictly(name):
    dvae_sd, grbm_sd = _checkpoint(name)
    n = dvae_sd["_encoder.projection.weight"].numel() and dvae_sd["_decoder.increase_latent_dim.weight"].shape[1]
    dvae = DiscreteVariationalAutoencoder(Encoder(n), Decoder(n))
    missing, unexpected = dvae.load_state_dict(dvae_sd, strict=True)
    assert not missing and not unexpected
    assert list(dvae.state_dict().keys()) == list(dvae_sd.keys())
    ei, ej = grbm_sd["_edge_idx_i"].tolist(), grbm_sd["_edge_idx_j"].tolist()
    grbm = GraphRestrictedBoltzmannMachine(range(n), zip(ei, ej))
    grbm.load_state_dict(grbm_sd, strict=True)
    assert list(grbm.state_dict().keys()) == list(grbm_sd.keys())
    # the real-QPU sub-graph is a valid sampler graph: proper colouring, CSR consistent with the edge list
    plan = grbm.plan
    assert plan.n == n and plan.n_edges == len(ei) and plan.n_colours <= 6
    # and the loaded weights mean the same network: oracle forward (stock torch ops) == the stock sub-modules
    x = (torch.rand(3, 1, 32, 32) < 0.13).float()
    dvae.eval()
    enc_sd = {k[len("_encoder."):]: v for k, v in dvae_sd.items() if k.startswith("_encoder.")}
    with torch.no_grad():
        want = dvae.encoder.projection(dvae.encoder.flatten_last_two_dims(dvae.encoder.conv(x))).flatten(1)
        got = nets.encoder_forward({k: v.clone() for k, v in enc_sd.items()}, x, training=False)
    assert torch.allclose(got, want, atol=1e-5)


def test_model_wrapper_load_rebuilds_sampler_on_checkpoint_graph(tmp_path):
    """ModelWrapper.load accepts a checkpoint trained on another (real-QPU) sub-graph: the GRBM and the local
    sampler are rebuilt on the checkpoint's own edge list (the reference needs the same live QPU for that)."""
    src = tmp_path / "Advantage2_system1_10_epochs"
    src.mkdir()
    dvae_sd, grbm_sd = _checkpoint(src.name)
    torch.save(dvae_sd, src / "dvae.pth")
    torch.save(grbm_sd, src / "grbm.pth")
    golden = os.path.join(GOLDEN, "step_params.yaml")
    m = ModelWrapper("Advantage2_system1", n_latents=256, training_parameter_file=golden)
    m.set_dataloader([(torch.zeros(8, 1, 32, 32), torch.zeros(8))])
    m.load(src)
    want = torch.load(os.path.join(src, "grbm.pth"), weights_only=True)
    assert torch.equal(m._grbm._quadratic.detach().cpu(), want["_quadratic"])
    assert m.sampler.plan.n_edges == want["_quadratic"].numel()
    assert torch.equal(m._dvae.state_dict()["_decoder.convtrans.20.weight"].cpu(),
                       torch.load(os.path.join(src, "dvae.pth"), weights_only=True)["_decoder.convtrans.20.weight"])
