"""MI355X-native ``ModelWrapper``: same entry points as /root/reference/src/model_wrapper.py
(``setup``, ``train_init``, ``step``, ``save``, ``load``, the YAML-backed attributes), with
every piece of arithmetic in libdvg.so and the QPU replaced by the on-GPU block-Gibbs sampler.

Reference quirks that are reproduced on purpose: the learning-rate
schedule is applied *after* the step (:347-351), the GRBM trains only for ``epoch < 6`` on
every 10th step (:59-67) with a second, independent sampler draw (:332-342), and the
checkpoint holds only the two ``state_dict``s (:148-162).
"""
from __future__ import annotations

import os
import time
from pathlib import Path
from typing import Callable, Optional

import numpy as np
import torch
import yaml

from . import functional as F
from .losses import nll_loss
from .modules import Decoder, Encoder, writes_grads_direct
from .optim import FlatAdam
from .persistent_sampler import PersistentQPUSampleHelper
from .plugin import (DiscreteVariationalAutoencoder, GaussianKernel, GraphRestrictedBoltzmannMachine,
                     maximum_mean_discrepancy_loss, maximum_mean_discrepancy_loss_and_grad)
from .sampler import beta_schedule, get_sampler_and_sampler_kwargs
from .viz import LOWER_THRESHOLD, UPPER_THRESHOLD  # /root/reference/demo_configs.py:62-63

_DEFAULT_YAML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "training_parameters.yaml")


def train_dvae(opt_step: int, epoch: int) -> bool:
    return True  # /root/reference/src/model_wrapper.py:48-56


def train_grbm(opt_step: int, epoch: int) -> bool:
    return epoch < 6 and opt_step % 10 == 0  # /root/reference/src/model_wrapper.py:59-67


def get_latent_to_discrete(mode):
    """/root/reference/src/utils/common.py:143-175."""
    if mode is None:
        return None
    if mode != "heaviside":
        raise ValueError("Invalid Mode: Mode is not heaviside.")
    return F.heaviside_latent_to_discrete


class TrainingError(Exception):
    """Error when training the model."""


class ModelWrapper:
    """Container for the discrete VAE with a GRBM prior.

    Args:
        qpu: solver name; selects the topology of the local sampler (graphs.LOCAL_SOLVERS).
        n_latents: number of latent spins (= GRBM nodes); a multiple of 32.
        training_parameter_file: YAML with the reference's keys (+ the GIBBS_* keys).
        dist: optional ``parallel.DataParallel`` context (one process per GPU).
    """

    # executable instances of the captured step, replayed round-robin (see _capture); 2 measured no faster than 1
    # on MI355X / ROCm 7.2 (1.265 vs 1.220 ms per c2 step: the host already runs ahead of the device)
    N_GRAPHS = 1

    def __init__(self, qpu: str, n_latents: Optional[int] = None, training_parameter_file: Optional[str] = None,
                 dist=None) -> None:
        self.qpu = qpu
        self.n_latents = n_latents
        self._dvae = None
        self._grbm = None
        self._device = None
        self.sampler = None
        self.sampler_kwargs = None
        self._dvae_optimizer = None
        self._grbm_optimizer = None
        self._dataloader = None
        self.losses = {"mse_losses": [], "dvae_losses": []}
        self.dist = dist
        self.noise_hook: Optional[Callable[[int], dict]] = None  # parity tests inject Gumbel noise / dropout masks
        self.sync_losses = True   # False: keep loss tensors on device (no .item() host syncs in the step)
        self.overlap_sampler = True  # run the step's sampler draw on a side stream under the forward pass
        self.overlap_mmd = True      # ... and the MMD behind it, under the decoder forward
        self._side_stream = None
        # use_graph: replay the autoencoder half of the step from a captured hipGraph (needs sync_losses = False);
        # ~120 kernel launches become one graph launch.  Off by default; bench.py turns it on.
        self.use_graph = False
        # prepare_decoder: enqueue the decoder's weight-only prologue at the start of the step, beside the encoder
        # (None: from PREPARE_DECODER_ROWS decoder rows up; True / False force it)
        self.prepare_decoder = None
        # defer_mmd_join: join the MMD stream behind the decoder's backward (None: measured per shape, _defer_mmd_join)
        self.defer_mmd_join = None
        # fuse_decoder_mse: Decoder.forward_mse in the training step (the reconstruction is never written) -- None: from
        # FUSE_DECODER_MSE_ROWS decoder rows (B * R) up; True / False: always / never (A/B runs, tests)
        self.fuse_decoder_mse = None
        self._prep_stream = None
        # Replayed steps write their losses into the graph's static output tensors.  keep_step_losses = True (default)
        # appends a COPY per step to self.losses (two tiny device copies, ~0.5 % of a c2 step), as the reference's lists
        # hold one value per step; False appends nothing (throughput runs: self.last still holds the latest values).
        self.keep_step_losses = True
        self._graph = None
        # (executable graph, its static input, its static outputs, Adam tail graph or None, the device addresses the
        # capture baked in: see _graph_addresses)
        self._graphs = []
        self._capturing_split = False
        self._pending = []        # data-parallel: optimizers whose packed gradients await the step's ONE all-reduce
        self._pending_tail = None
        self._joint_grad = None   # [dvae gradients | GRBM gradients]: the buffer of that all-reduce
        self._replays = 0
        self._replay_host_s = 0.0
        self._graph_failed = False
        self._static_images = None
        self._dyn = None
        self._eager_steps = 0
        self.last = {}            # device scalars of the last step: mse, mmd, nll
        with open(training_parameter_file or _DEFAULT_YAML, "r") as f:
            self._params = yaml.safe_load(f)

    def __getattr__(self, name: str):
        params = self.__dict__.get("_params")
        if params is not None and name in params:
            return params[name]
        raise AttributeError(name)

    # ------------------------------------------------------------------ checkpoints
    def save(self, file_path) -> None:
        """Two ``state_dict`` files, as /root/reference/src/model_wrapper.py:148-162.

        Rank-local (no collective): ``if rank == 0: model.save(...)`` is safe.  In a data-parallel run the BatchNorm
        running statistics differ per rank until :meth:`sync_buffers` -- a collective every rank must reach; the epoch
        driver (training.execute_training) calls it at the end of every epoch -- has made them rank 0's."""
        file_path = Path(file_path)
        file_path.mkdir(exist_ok=True, parents=True)
        torch.save({k: v.detach().cpu().clone() for k, v in self._dvae.state_dict().items()}, file_path / "dvae.pth")
        torch.save({k: v.detach().cpu().clone() for k, v in self._grbm.state_dict().items()}, file_path / "grbm.pth")

    def load(self, file_path) -> None:
        """/root/reference/src/model_wrapper.py:164-175 (``setup``, the dataset, the two ``state_dict``s)."""
        file_path = Path(file_path)
        self.setup()
        if self._dataloader is None:
            self._load_dataset(batch_size=self.BATCH_SIZE, dataset_size=self.DATASET_SIZE)
        grbm_sd = torch.load(file_path / "grbm.pth", weights_only=True)
        if grbm_sd["_edge_idx_i"].numel() != self._grbm._edge_idx_i.numel() or not (
            torch.equal(grbm_sd["_edge_idx_i"].cpu(), self._grbm._edge_idx_i.cpu())
            and torch.equal(grbm_sd["_edge_idx_j"].cpu(), self._grbm._edge_idx_j.cpu())
        ):
            # the checkpoint was trained on another (real-QPU) sub-graph: rebuild GRBM + sampler on ITS edges
            self._rebuild_on_edges(grbm_sd["_edge_idx_i"].cpu().numpy(), grbm_sd["_edge_idx_j"].cpu().numpy())
        self._dvae.load_state_dict(torch.load(file_path / "dvae.pth", weights_only=True))
        self._grbm.load_state_dict(grbm_sd)
        self._invalidate_graphs()

    def _invalidate_graphs(self) -> None:
        """Drops every captured step.  A captured hipGraph holds raw device addresses (parameter views and Adam
        moments in the optimizers' flat buffers, the GRBM parameters, the persistent chains, the step-state block):
        whatever replaces one of those tensors calls this, and the next eligible step captures afresh."""
        self._graph = None
        self._graphs = []
        self._static_images = None
        self._eager_steps = 0
        self._replays = 0
        self._graph_failed = False
        self._pending = []
        self._pending_tail = None

    def _graph_addresses(self):
        """Device addresses a captured step reads or writes outside its own static tensors; compared before every
        replay (a mismatch -- e.g. the sampler re-allocated its chains for another ``num_reads`` -- re-captures)."""
        s = self.sampler
        return (self._dvae_optimizer.flat.data_ptr(), self._dvae_optimizer.flat_grad.data_ptr(),
                self._dvae_optimizer.exp_avg.data_ptr(), self._dvae_optimizer.exp_avg_sq.data_ptr(),
                self._grbm._linear.data_ptr(), self._grbm._quadratic.data_ptr(),
                0 if (s._state is None or not s.persistent) else s._state.data_ptr(),  # (restarted chains: a fresh tensor per draw)
                0 if self._dyn is None else self._dyn.ptr,
                # (a changed beta schedule: another number of sweeps per draw -- baked in -- or a new table)
                int(s.sweeps), 0 if getattr(s, "_betas", None) is None else s._betas.data_ptr())

    # -- exact resume: an EXTRA file next to the reference-schema checkpoint, never read by the UI
    def save_training_state(self, file_path) -> None:
        """``train_state.pth``: everything beyond the two state_dicts that the next step depends on -- Adam moments
        and step counts, the persistent Gibbs chains and every counter that positions a device random stream -- so
        that ``load`` + ``load_training_state`` continues the run bit for bit."""
        file_path = Path(file_path)
        file_path.mkdir(exist_ok=True, parents=True)
        s = self.sampler
        helper = self._tpar.get("persistent_qpu_sample_helper")
        state = {
            "opt_step": int(self._tpar["opt_step"]),
            "dvae_optimizer": {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in self._dvae_optimizer.state_dict().items()},
            "grbm_optimizer": {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in self._grbm_optimizer.state_dict().items()},
            "sampler": {"state": None if s._state is None else s._state.cpu(), "sweep_count": s.sweep_count, "calls": s.calls},
            "gumbel_calls": self._dvae._gumbel_calls, "gumbel_seed": self._dvae.gumbel_seed,
            "dropout_calls": self._dvae.decoder._dropout_calls, "dropout_seed": self._dvae.decoder.dropout_seed,
            "helper_iterations": None if helper is None else int(helper.iterations_since_last_resampling),
            "losses": {k: [float(v) for v in vals] for k, vals in self.losses.items()},
        }
        torch.save(state, file_path / "train_state.pth")

    def load_training_state(self, file_path) -> None:
        """Counterpart of :meth:`save_training_state`; call after ``load`` and ``train_init``."""
        state = torch.load(Path(file_path) / "train_state.pth", weights_only=False)
        self._tpar["opt_step"] = state["opt_step"]
        for opt, key in ((self._dvae_optimizer, "dvae_optimizer"), (self._grbm_optimizer, "grbm_optimizer")):
            sd = state[key]
            opt.load_state_dict({k: (v.to(self._device) if torch.is_tensor(v) else v) for k, v in sd.items()})
        s = self.sampler
        s._state = None if state["sampler"]["state"] is None else state["sampler"]["state"].to(self._device)
        s.sweep_count, s.calls = state["sampler"]["sweep_count"], state["sampler"]["calls"]
        self._dvae._gumbel_calls, self._dvae.gumbel_seed = state["gumbel_calls"], state["gumbel_seed"]
        self._dvae.decoder._dropout_calls, self._dvae.decoder.dropout_seed = state["dropout_calls"], state["dropout_seed"]
        helper = self._tpar.get("persistent_qpu_sample_helper")
        if helper is not None and state["helper_iterations"] is not None:
            helper.iterations_since_last_resampling = state["helper_iterations"]
        self.losses = {k: list(v) for k, v in state["losses"].items()}
        self._invalidate_graphs()  # the chains (and possibly the moments) live in new tensors
        # the learning rates in force are the ones the schedule set after the last completed step
        if state["opt_step"] > 0:
            self._dvae_optimizer.param_groups[0]["lr"] = self._tpar["dvae_lr_schedule"][state["opt_step"] - 1]
            self._grbm_optimizer.param_groups[0]["lr"] = self._tpar["grbm_lr_schedule"][state["opt_step"] - 1]

    def _rebuild_on_edges(self, ei, ej):
        from .graphs import build_plan
        from .sampler import GibbsSampler

        n = self.n_latents
        plan = build_plan(n, ei, ej)
        old = self.sampler
        betas = getattr(old, "_betas", None)  # (with a schedule set, old.sweeps is the schedule's length)
        self.sampler = GibbsSampler(plan, list(range(n)), beta=old.beta, sweeps=old.sweeps if betas is None else old._fixed_sweeps, seed=old.seed,
                                    persistent=old.persistent, device=self._device, chain_offset=old.chain_offset,
                                    h_range=tuple(old.properties["h_range"]), j_range=tuple(old.properties["j_range"]))
        if betas is not None:
            self.sampler.set_beta_schedule(betas)
        grbm = GraphRestrictedBoltzmannMachine(list(range(n)), list(zip(ei.tolist(), ej.tolist())))
        self._grbm = grbm.to(self._device)
        self._make_optimizers()

    # ------------------------------------------------------------------ construction
    def setup(self) -> None:
        """Build DVAE, sampler, GRBM and the two optimizers (/root/reference/src/model_wrapper.py:177-217)."""
        self._device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if self.LATENT_TO_DISCRETE in ["heaviside"] and self.N_REPLICAS != 1:
            raise ValueError("heaviside latent-to-discrete can only be used with n_replicas=1")
        precision = self._params.get("CONV_PRECISION")  # absent (the reference's YAML): the library's mode stands
        if precision is not None and self._device.type == "cuda":
            from . import _lib

            _lib.set_conv_precision(str(precision))
        dvae = DiscreteVariationalAutoencoder(
            encoder=Encoder(n_latents=self.n_latents),
            decoder=Decoder(n_latents=self.n_latents),
            latent_to_discrete=get_latent_to_discrete(self.LATENT_TO_DISCRETE),
        )
        self._dvae = dvae.to(self._device)
        rank = self.dist.rank if self.dist is not None else 0
        num_reads = self.local_num_reads()
        self.sampler, self.sampler_kwargs, graph, self.linear_range, self.quadratic_range = get_sampler_and_sampler_kwargs(
            num_reads=num_reads,
            annealing_time=self.ANNEALING_TIME,
            n_latents=self.n_latents,
            random_seed=self.RANDOM_SEED,
            qpu=self.qpu,
            sweeps=int(self._params.get("GIBBS_SWEEPS", 50)),
            beta=self._params.get("GIBBS_BETA"),
            prefactor=self.PREFACTOR,
            persistent=bool(self._params.get("GIBBS_PERSISTENT", True)),
            device=self._device,
            chain_offset=rank * num_reads,  # chains are globally numbered: G GPUs sample G*num_reads distinct chains
        )
        # GIBBS_BETA_START (optional): every draw anneals from that beta to the sampler's own over its GIBBS_SWEEPS sweeps,
        # spaced as GIBBS_BETA_SCHEDULE says ("geometric", the default, or "linear")
        beta_start = self._params.get("GIBBS_BETA_START")
        if beta_start is not None:
            kind = str(self._params.get("GIBBS_BETA_SCHEDULE", "geometric"))
            self.sampler.set_beta_schedule(beta_schedule(float(beta_start), self.sampler.beta, self.sampler.sweeps, kind))
        grbm = GraphRestrictedBoltzmannMachine(graph.nodes, graph.edges)
        self._grbm = grbm.to(self._device)
        self._dvae.gumbel_seed = int(self.RANDOM_SEED) + 7919 * rank
        self._dvae.decoder.dropout_seed = int(self.RANDOM_SEED) + 104729 * rank
        self._make_optimizers()
        self.sync_replicas()

    # ------------------------------------------------------------------ data-parallel replica consistency
    def _bn_buffers(self):
        return [b for _, b in self._dvae.named_buffers()]

    def sync_replicas(self) -> None:
        """Every rank starts from rank 0's model: one broadcast per flat parameter buffer plus the BatchNorm buffers.
        (``setup`` may run before or after the seeding of ``train_init`` -- reference quirk 7 -- so identical seeding
        is not relied upon.)  No-op without a process group."""
        if not self._dist_active() or self._device.type != "cuda":
            return
        self.dist.broadcast_(self._dvae_optimizer.flat)
        self.dist.broadcast_(self._grbm_optimizer.flat)
        self.sync_buffers()

    def sync_buffers(self) -> None:
        """BatchNorm running statistics are rank 0's (they are read only in eval mode; each rank's training-mode
        batch statistics stay local, DDP semantics).  A COLLECTIVE: every rank must call it (the epoch driver does, at
        the end of each epoch); ``save`` / ``generate_*`` / ``reconstruct_images`` are rank-local and never call it."""
        if not self._dist_active():
            return
        bufs = self._bn_buffers()
        if not bufs:
            return
        # ONE broadcast: float32 statistics and the int64 batch counters travel as float64 (exact for both)
        flat = torch.cat([b.detach().reshape(-1).to(torch.float64) for b in bufs])
        self.dist.broadcast_(flat)
        off = 0
        with torch.no_grad():
            for b in bufs:
                b.copy_(flat[off: off + b.numel()].view(b.shape).to(b.dtype))
                off += b.numel()

    def is_main_rank(self) -> bool:
        """True on the rank that writes checkpoints / figures / side files (rank 0; always without a process group)."""
        return self.dist is None or self.dist.rank == 0

    def local_num_reads(self) -> int:
        """Chains per rank.  Data parallelism is weak-scaled: every rank keeps the full per-GPU
        workload (its own mini-batch AND its own NUM_READS chains, globally numbered by rank)."""
        return int(self.NUM_READS)

    def _make_optimizers(self):
        self._invalidate_graphs()
        if self._device.type != "cuda":
            self._dvae_optimizer = _DeferredAdam(self._dvae.parameters(), lr=self.AUTOENCODER_INITIAL_LR,
                                                 weight_decay=self.AUTOENCODER_WEIGHT_DECAY)
            self._grbm_optimizer = _DeferredAdam(self._grbm.parameters(), lr=self.BM_INITIAL_LR,
                                                 weight_decay=self.BM_WEIGHT_DECAY)
            return
        # Both optimizers pack their gradients into ONE buffer, [encoder + decoder | GRBM h, J], so that a
        # data-parallel step -- also one that trains the GRBM -- is a single all-reduce.
        nd = sum(p.numel() for p in self._dvae.parameters())
        ng = sum(p.numel() for p in self._grbm.parameters())
        self._joint_grad = torch.zeros(nd + ng, dtype=torch.float32, device=self._device)
        self._dvae_optimizer = FlatAdam(self._dvae.parameters(), lr=self.AUTOENCODER_INITIAL_LR,
                                        weight_decay=self.AUTOENCODER_WEIGHT_DECAY, grad_buffer=self._joint_grad[:nd])
        self._grbm_optimizer = FlatAdam(self._grbm.parameters(), lr=self.BM_INITIAL_LR, weight_decay=self.BM_WEIGHT_DECAY,
                                        grad_buffer=self._joint_grad[nd:])
        # the networks' backward kernels write their parameter gradients straight into the joint buffer
        for net in (self._dvae.encoder, self._dvae.decoder):
            net._grad_sink = [self._dvae_optimizer.grad_view(p) for p in net._trainable()]

    def set_dataloader(self, dataloader) -> None:
        """Any iterable of ``(images (B,1,32,32) in {0,1}, labels)`` with ``len()``."""
        self._dataloader = dataloader

    def _load_dataset(self, batch_size: int, dataset_size: Optional[int] = None) -> None:
        from .data import get_dataloader

        rank, world = (self.dist.rank, self.dist.world_size) if self.dist is not None else (0, 1)
        self._dataloader = get_dataloader(self.IMAGE_SIZE, batch_size, dataset_size, seed=self.RANDOM_SEED, rank=rank,
                                          world_size=world)  # disjoint shards of one permutation per epoch

    def train_init(self, n_epochs: int) -> None:
        """/root/reference/src/model_wrapper.py:229-277."""
        self.losses["mse_losses"].clear()
        self.losses["dvae_losses"].clear()
        torch.manual_seed(self.RANDOM_SEED)
        self._tpar = {}
        self._tpar["persistent_qpu_sample_helper"] = PersistentQPUSampleHelper(
            max_deque_size=self.MAX_DEQUE_SIZE, iterations_before_resampling=self.ITERATIONS_BEFORE_RESAMPLING
        )
        if self._dvae is None or self._grbm is None:
            self.setup()
        if self._dataloader is None:
            self._load_dataset(batch_size=self.BATCH_SIZE, dataset_size=self.DATASET_SIZE)
        total_opt_steps = n_epochs * len(self._dataloader)
        self._tpar["dvae_lr_schedule"] = np.geomspace(self.AUTOENCODER_INITIAL_LR, self.AUTOENCODER_FINAL_LR,
                                                      total_opt_steps + 1)
        self._tpar["grbm_lr_schedule"] = np.geomspace(self.BM_INITIAL_LR, self.BM_FINAL_LR, total_opt_steps + 1)
        self._tpar["opt_step"] = 0
        self._tpar["kernel"] = GaussianKernel(n_kernels=7).to(self._device)
        self._tpar["sample_set"] = None
        self._tpar["init_done"] = True

    # ------------------------------------------------------------------ the hot path
    def step(self, batch, epoch: int) -> torch.Tensor:
        """One training step; same order of operations as /root/reference/src/model_wrapper.py:279-353."""
        if not self._tpar.get("init_done", True):
            raise TrainingError("Initialization required before training.")
        images, _ = batch
        images = images.to(self._device)
        self._dvae.train()
        self._grbm.train()
        opt_step = self._tpar["opt_step"]
        if self.noise_hook is not None:
            noise = self.noise_hook(opt_step)
            if noise.get("gumbels") is not None:
                self._dvae.inject_gumbels(noise["gumbels"].to(self._device))
            if noise.get("dropout_masks") is not None:
                self._dvae.decoder.inject_dropout_masks([m.to(self._device) for m in noise["dropout_masks"]])

        if self._graph_eligible(opt_step, epoch, images):
            mse_loss, spins = self._step_graphed(images)
        else:
            mse_loss, dvae_loss, _mmd_loss, spins = self._dvae_half(images)
            self._log("mse_losses", mse_loss)
            self._log("dvae_losses", dvae_loss)
            self.last.update(mse=mse_loss.detach(), mmd=_mmd_loss.detach())
            self._eager_steps += 1

        if train_grbm(opt_step, epoch):
            self._grbm_optimizer.zero_grad()
            grbm_loss, self._tpar["sample_set"] = nll_loss(
                spins=spins.detach(),
                grbm=self._grbm,
                sampler=self.sampler,
                sampler_kwargs=self.sampler_kwargs,
                linear_range=self.linear_range,
                quadratic_range=self.quadratic_range,
                prefactor=self.PREFACTOR,
                persistent_qpu_sample_helper=self._tpar["persistent_qpu_sample_helper"],
                sample_set=self._tpar["sample_set"],
            )
            grbm_loss.backward()
            self._reduce_and_step(self._grbm_optimizer)
            self.last.update(nll=grbm_loss.detach())
        # Data-parallel: everything this step produced -- the encoder/decoder gradients and, on a GRBM step, the
        # sufficient-statistic differences behind them in the same buffer -- goes through ONE all-reduce, then the
        # Adam launches.  (The autoencoder's Adam thus runs after the GRBM's backward on such a step; neither reads what
        # the other writes -- the GRBM branch works on ``spins.detach()`` and its own parameters -- so the result is the
        # reference's order bit for bit.)
        self._flush_dist()

        for param_group in self._dvae_optimizer.param_groups:
            param_group["lr"] = self._tpar["dvae_lr_schedule"][opt_step]
        for param_group in self._grbm_optimizer.param_groups:
            param_group["lr"] = self._tpar["grbm_lr_schedule"][opt_step]
        self._tpar["opt_step"] += 1
        return mse_loss

    def _dvae_half(self, images):
        """Forward, MSE + MMD, backward and Adam for the autoencoder (/root/reference/src/model_wrapper.py:297-327)."""
        try:
            return self._dvae_half_impl(images)
        except BaseException:
            # the decoder's backward may have returned with the library's side stream still forked (deferred join): close
            # the fork, release what it pinned and clear the flag, so that neither a later standalone decoder backward nor
            # the end of a failed hipGraph capture sees a half-open step
            try:
                self._join_deferred()
            except Exception:
                pass
            raise

    def _join_deferred(self):
        """Joins the library's side stream into the current stream (the decoder's deferred weight-gradient chain), then
        drops the tensors the decoder's backward pinned for that chain and clears the deferral flag."""
        dec = self._dvae.decoder
        try:
            if self._device is not None and self._device.type == "cuda":
                from . import _lib
                _lib.check(_lib.lib().dvg_stream_join_side(_lib.stream_ptr(self._device)), "dvg_stream_join_side")
        finally:
            dec._defer_join = False  # (only this step's own backward runs deferred)
            dec._deferred_keep = None

    def _dvae_half_impl(self, images):
        # The sampler draw of this step needs nothing but the current GRBM parameters, so it is enqueued FIRST, on a
        # side HIP stream, and runs under the encoder/decoder forward (it occupies a few dozen CUs for hundreds of
        # microseconds).  Same draw, same position in the sampler's random stream as in the reference's order.
        self._hold_device_while_measuring(int(images.shape[0]) * int(self.N_REPLICAS))
        samples = self._draw_overlapped() if self.overlap_sampler else None
        self._dvae.decoder._defer_join = True  # (this step always runs the encoder's backward behind the decoder's)
        if samples is not None and self.overlap_mmd:
            # The MMD needs only the spins and the draw, so it follows the draw on the side stream and runs under
            # the decoder forward and the MSE; the streams join before the two losses are added.
            main, side = torch.cuda.current_stream(self._device), self._side_stream
            # (enqueued BEHIND the draw: a replayed graph submits its nodes in capture order, and the draw is the long pole)
            self._prepare_decoder(images, main)
            latents = self._dvae.encoder(images)
            # The default (Gumbel) latent_to_discrete runs outside autograd: its backward is fed the SUM of the two spin
            # gradients (through the decoder and from the MMD) by ONE kernel -- dvg_gumbel_bwd2 -- instead of an add pass
            # over (B, R, n) followed by the single-gradient kernel.  A custom latent_to_discrete (heaviside) stays an
            # autograd node and gets the two terms added by the engine.
            raw = self._dvae.default_l2d_raw(latents, self.N_REPLICAS)
            spins, dspin = raw if raw is not None else (self._dvae.latent_to_discrete(latents, self.N_REPLICAS), None)
            spins_ready = torch.cuda.Event()
            spins_ready.record(main)
            # Order of enqueueing matters under hipGraph capture: the first kernel node captured after a fork keeps
            # the parent's hardware queue (so an anchor node goes first on the main stream and the decoder chain, the
            # critical path, stays on its queue), and a replay submits nodes in capture order (so the MMD is captured
            # BEFORE the ~50 decoder-forward nodes, not behind them).
            self._dvae_optimizer.zero_grad()
            from . import _lib
            _lib.check(_lib.lib().dvg_stream_anchor(main.cuda_stream), "dvg_stream_anchor")
            side.wait_event(spins_ready)
            # Both loss kernels produce their gradient with the value, so the backward pass is seeded with those two
            # tensors directly (d(mse + mmd) = 1 * each): no ones_like, no per-term multiply, and the sum of the two
            # scalars (logging only) is off the critical path.
            flat = spins.reshape(-1, spins.shape[-1])
            with torch.cuda.stream(side):
                _mmd_loss, g_spins = maximum_mean_discrepancy_loss_and_grad(x=flat, y=samples, kernel=self._tpar["kernel"])
            # The autograd graph is cut at the spins: the decoder's backward needs only the MSE gradient, so the join with
            # the MMD stream can sit IN FRONT of the decoder's backward (small problems: the MMD ends well inside the
            # decoder forward, and a mid-backward join costs 45 us there) or BEHIND it (large pair counts -- c3: the pair
            # kernel runs 1.4 ms past the decoder forward, which the main stream used to sit out; 23.65 -> 22.93 ms).
            defer = self._defer_mmd_join(flat, samples)
            spins_cut = spins.detach().requires_grad_(True)
            dec = self._dvae.decoder
            # fuse_decoder_mse: the reconstruction loss behind the decoder in one pair of library calls -- the reconstruction
            # and its gradient are never written (Decoder.forward_mse; same loss to rounding, same gradients bit for bit)
            n_rows = int(spins.shape[0]) * int(spins.shape[1])
            want = self.fuse_decoder_mse if self.fuse_decoder_mse is not None else n_rows >= self.FUSE_DECODER_MSE_ROWS
            fused = bool(want) and _lib.get_option("dec_tail_fused") != 0
            # (the spins of the library's own Gumbel kernel are exactly +-1, and the decoder is told so: Decoder.forward)
            pm1 = raw is not None
            if fused:
                mse_loss = dec.forward_mse(spins_cut, images, spins_pm1=pm1)
                seed_t, seed_g = [mse_loss], None
            else:
                reconstructed_images = dec(spins_cut, spins_pm1=pm1)
                mse_loss, g_recon = F.replicated_mse_loss_and_grad(reconstructed_images, images)
                seed_t, seed_g = [reconstructed_images], [g_recon]
            if not defer:
                self._defer_measure(main, side)
                main.wait_stream(side)
            # torch.autograd.grad hands the decoder's spin gradient back as the tensor the backward kernel wrote; .backward()
            # would route it through AccumulateGrad of the leaf, which CLONES it (67 MB at c3: an 86 us copy on the critical
            # chain).  The decoder's parameter gradients do not travel through autograd at all here: its backward writes
            # them into the optimizer's flat buffer and sets .grad itself (modules._grad_targets).
            if writes_grads_direct(dec):
                (g_dec,) = torch.autograd.grad(seed_t, [spins_cut], seed_g)
                assert all(p.grad is not None for p in dec._trainable()), "decoder backward did not take the direct path"
            else:
                torch.autograd.backward(seed_t, seed_g)
                g_dec = spins_cut.grad
            mse_loss = mse_loss.detach()
            if defer:
                main.wait_stream(side)
            g_spins.record_stream(main)
            if dspin is not None:
                gl = F.gumbel_backward(dspin, g_dec, g_spins)  # (the same two terms the autograd engine would add)
                torch.autograd.backward([latents], [gl])
            else:
                torch.autograd.backward([spins], [g_dec.add_(g_spins.view_as(g_dec))])
            _mmd_loss.record_stream(main)
            dvae_loss = F.scalar_add(mse_loss, _mmd_loss)
            self._reduce_and_step(self._dvae_optimizer)
            return mse_loss, dvae_loss, _mmd_loss, flat.detach()
        _, spins, reconstructed_images = self._dvae(images, self.N_REPLICAS)
        self._dvae_optimizer.zero_grad()
        mse_loss = F.replicated_mse_loss(reconstructed_images, images)
        if samples is None:
            with torch.no_grad():
                samples = self._grbm.sample(
                    sampler=self.sampler,
                    prefactor=self.PREFACTOR,
                    linear_range=self.linear_range,
                    quadratic_range=self.quadratic_range,
                    device=spins.device,
                    sample_params=self.sampler_kwargs,
                )
        else:
            torch.cuda.current_stream(self._device).wait_stream(self._side_stream)
        spins = spins.reshape(-1, spins.shape[-1])
        _mmd_loss = maximum_mean_discrepancy_loss(x=spins, y=samples, kernel=self._tpar["kernel"])
        dvae_loss = mse_loss + _mmd_loss
        dvae_loss.backward()
        self._reduce_and_step(self._dvae_optimizer)
        return mse_loss, dvae_loss, _mmd_loss, spins

    # Decision: join the MMD stream BEHIND the decoder's backward instead of in front of it?  It pays exactly when the
    # side chain (draw -> MMD) is still running when the main stream reaches the join -- then a join in front of the
    # backward stalls the main stream for the remainder, while the decoder's backward needs only the MSE gradient -- and
    # costs a mid-backward dependency (~45 us at c2's size) when it is not.  Which of the two holds depends on the whole
    # shape (sweeps and chains of the draw, n, B, R: tools/defer_crossover.py, profiles/r04_defer_mmd_join_crossover.txt:
    # behind / first = 1.05 at c2, 0.85 at n = 512 with B = 128, 0.83 at the c5 slice, 1.00 at c3), so it is MEASURED
    # instead of guessed from a work count (round 3 switched on (nx + ny) d >= 4e6, tuned on c3): the first eager steps
    # of a shape join in front and time, with two HIP events, how long after the main stream reached the join the side
    # stream finished; from then on the join is deferred iff that lag exceeds DEFER_LAG_MS.  The order of the join does
    # not change any number (tests/test_gpu_step.py::test_deferred_mmd_join_is_bit_identical).
    DEFER_LAG_MS = 0.05
    DEFER_SAMPLES = 2

    def _defer_mmd_join(self, flat, samples) -> bool:
        """``defer_mmd_join`` = True / False forces it; otherwise the measured decision for this shape, False while the
        measurement is still running."""
        forced = getattr(self, "defer_mmd_join", None)
        if forced is not None:
            return bool(forced)
        key = (tuple(flat.shape), tuple(samples.shape), int(getattr(self.sampler, "sweeps", 0)))
        state = self.__dict__.setdefault("_defer_state", {})
        rec = state.get(key)
        if rec is None:
            rec = state[key] = {"decision": None, "events": [], "lags": []}
        self._defer_rec = rec
        self.__dict__.setdefault("_defer_by_rows", {})[int(flat.shape[0])] = rec
        if self._device is not None and self._device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            # never wait for an event inside a stream capture (it would fail the capture and force eager steps for the
            # rest of the process): the graph bakes in whatever is decided so far -- _graph_eligible keeps an undecided
            # shape eager until its measurement is in
            return bool(rec["decision"])
        if rec["decision"] is None and len(rec["events"]) >= self.DEFER_SAMPLES:
            for ev_main, ev_side in rec["events"]:
                ev_main.synchronize()  # (warm-up steps only: one host wait per shape)
                ev_side.synchronize()
                rec["lags"].append(ev_main.elapsed_time(ev_side))  # > 0: the side stream finished that much LATER
            rec["events"] = []
            # (the LARGEST of the samples: a sample taken while the host was the slower side reads ~0)
            rec["decision"] = bool(max(rec["lags"]) > self.DEFER_LAG_MS)
        return bool(rec["decision"])

    def _defer_undecided(self, rows=None) -> bool:
        """True while the shape of the step about to run (``rows`` = B x replicas; None: the last step's shape) is still
        being measured (its graph must not be captured yet).  Keyed on the step's OWN shape: a ragged last
        batch, which appears once per epoch and never reaches a decision, no longer sends the next epoch's first
        full-shape step down the eager path although that shape's decision and graph exist."""
        if getattr(self, "defer_mmd_join", None) is not None or not (self.overlap_sampler and self.overlap_mmd):
            return False
        rec = self.__dict__.get("_defer_by_rows", {}).get(int(rows)) if rows is not None else getattr(self, "_defer_rec", None)
        if rows is not None and rec is None:
            return True  # (a shape never seen: it measures first)
        return rec is not None and rec["decision"] is None

    def _hold_device_while_measuring(self, rows: int) -> None:
        """The lag behind ``_defer_mmd_join`` must be the DEVICE's: an eager step whose launches the host issues more
        slowly than the GPU runs them (the first steps of a process: module loads, allocator growth) finds both streams
        idle at the join and measures ~0 whatever the shape.  So a step that is going to measure starts with a spin kernel
        on the main stream, in front of the fork of the side stream: the host enqueues the whole step behind it and the
        two chains then run at the device's pace.  ~20 ms on each of the DEFER_SAMPLES measuring steps of a shape and on the
        step that reads the events (``rows`` = rows of the flattened spins of the step about to run: B x replicas)."""
        if (self._device is None or self._device.type != "cuda" or not (self.overlap_sampler and self.overlap_mmd)
                or getattr(self, "defer_mmd_join", None) is not None or torch.cuda.is_current_stream_capturing()):
            return
        # (keyed on the shape of the step that is about to run: the record of the PREVIOUS step's shape says nothing
        # about a new one; a shape never seen before has no record yet and measures)
        rec = self.__dict__.get("_defer_by_rows", {}).get(int(rows))
        spin = getattr(torch.cuda, "_sleep", None)
        if spin is not None and (rec is None or rec["decision"] is None):
            spin(2_000_000)  # (~20 ms: the counter behind it runs at 100 MHz)

    def _defer_measure(self, main, side) -> None:
        """Called at the join-in-front point of a step that is still measuring: marks "main stream reached the join" and
        "side stream done" (never inside a stream capture)."""
        rec = getattr(self, "_defer_rec", None)
        if rec is None or rec["decision"] is not None or getattr(self, "defer_mmd_join", None) is not None:
            return
        if torch.cuda.is_current_stream_capturing():
            return
        ev_main, ev_side = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev_main.record(main)
        ev_side.record(side)
        rec["events"].append((ev_main, ev_side))

    # ------------------------------------------------------------------ hipGraph replay of the autoencoder half
    def _graph_eligible(self, opt_step, epoch, images) -> bool:
        """The captured graph covers the autoencoder half of every step (on a GRBM step the quasi-NLL update runs
        eagerly behind the replay, on the replay's static spins); noise-injected (parity) steps take the eager path.
        With several GPUs the step is two graphs with the (eager) all-reduce between them."""
        return (self.use_graph and self._device.type == "cuda" and self.noise_hook is None and not self._graph_failed
                and self._eager_steps >= 3 and not self.sync_losses
                and not self._defer_undecided(int(images.shape[0]) * int(self.N_REPLICAS))
                and (self._static_images is None or images.shape == self._static_images.shape))

    def _host_counters(self):
        d, s = self._dvae, self.sampler
        return (s.sweep_count, s.calls, d._gumbel_calls, d.decoder._dropout_calls, self._dvae_optimizer.step_count)

    def _set_host_counters(self, c):
        d, s = self._dvae, self.sampler
        s.sweep_count, s.calls, d._gumbel_calls, d.decoder._dropout_calls, self._dvae_optimizer.step_count = c

    def _write_dyn(self):
        """Per-step scalars of the NEXT autoencoder half, as the kernels would receive them by value."""
        c = self._host_counters()
        step_size, bc2 = self._dvae_optimizer.hyper(c[4] + 1)
        self._dyn.write(sweep0=c[0], gumbel_offset=c[2], dropout_offset=c[3], step_size=(step_size, 0.0), bc2_sqrt=(bc2, 1.0))

    def _capture(self, images):
        """Capture one more instance of the autoencoder half.  ``N_GRAPHS`` instances can be replayed round-robin
        (each with its own static input / outputs); the idea -- a second executable so that step k+1 is submitted
        while step k still runs -- measured no gain (the host is already ~0.25 ms per step ahead of the device), so
        one instance is the default."""
        from . import _lib

        if self._dyn is None:
            self._dyn = _lib.StepState(self._device)
        static_images = torch.empty_like(images)
        static_images.copy_(images)
        self._static_images = static_images
        saved = self._host_counters()
        self._write_dyn()
        torch.cuda.synchronize(self._device)
        graph = torch.cuda.CUDAGraph()
        tail = None
        dot = os.environ.get("DVG_GRAPH_DOT")  # diagnostics: write the captured graph (nodes and edges) to this path
        if dot:
            graph.enable_debug_mode()
        _lib.DYN = self._dyn.ptr
        try:
            # Data-parallel runs: graph 1 ends with the gradients packed into the optimizer's flat buffer; the ONE
            # all-reduce of the step runs eagerly on RCCL's stream; graph 2 is the Adam launch (the 1/world_size of
            # the mean is its grad_scale argument).  Three host calls per step instead of ~120.
            self._capturing_split = self._dist_active()
            # (thread_local: RCCL's watchdog thread may touch the runtime while this thread captures)
            mode = dict(capture_error_mode="thread_local") if self._capturing_split else {}
            with torch.cuda.graph(graph, **mode):
                mse, dvae, mmd, spins = self._dvae_half(static_images)
            if self._capturing_split:
                tail = torch.cuda.CUDAGraph()
                with torch.cuda.graph(tail, **mode):
                    self._dvae_optimizer.step(grad_scale=1.0 / self.dist.world_size, gathered=True)
        finally:
            self._capturing_split = False
            _lib.DYN = None
            self._set_host_counters(saved)  # the capture pass launched nothing: roll the host counters back
        if dot:
            graph.debug_dump(dot)
        self._graphs.append((graph, static_images, (mse, dvae, mmd, spins.detach()), tail, self._graph_addresses()))
        self._graph = graph

    def _step_graphed(self, images):
        slot = self._replays % self.N_GRAPHS
        if len(self._graphs) <= slot:
            try:
                self._capture(images)
            except Exception as exc:  # capture is an optimisation: fall back to eager, loudly, once
                import warnings

                self._graph_failed = True
                warnings.warn(f"hipGraph capture of the training step failed ({exc!r}); continuing eagerly")
                mse_loss, dvae_loss, _mmd_loss, spins = self._dvae_half(images)
                self._log("mse_losses", mse_loss)
                self._log("dvae_losses", dvae_loss)
                self.last.update(mse=mse_loss.detach(), mmd=_mmd_loss.detach())
                return mse_loss, spins
        if self._graphs[slot][4] != self._graph_addresses():
            # a tensor the capture baked in was replaced behind our back (e.g. the sampler re-allocated its chains):
            # drop the captures and run this step eagerly; the next eligible one captures afresh
            self._invalidate_graphs()
            mse_loss, dvae_loss, _mmd_loss, spins = self._dvae_half(images)
            self._log("mse_losses", mse_loss)
            self._log("dvae_losses", dvae_loss)
            self.last.update(mse=mse_loss.detach(), mmd=_mmd_loss.detach())
            self._eager_steps += 1
            return mse_loss, spins
        graph, static_images, outs, tail, _addr = self._graphs[slot]
        self._replays += 1
        static_images.copy_(images)
        self._write_dyn()
        t_host = time.perf_counter()
        graph.replay()
        self._replay_host_s += time.perf_counter() - t_host  # (host time of the launch call alone: bench.py reports it)
        if tail is not None:  # data-parallel: the collective and the captured Adam launch follow in _flush_dist
            self._pending.append(self._dvae_optimizer)
            self._pending_tail = tail
        c = self._host_counters()
        self._set_host_counters((c[0] + self.sampler.sweeps, c[1] + 1, c[2] + 1, c[3] + 1, c[4] + 1))
        mse, dvae, mmd, spins = outs
        if self.keep_step_losses:  # the outputs are static tensors, overwritten by the next replay: log copies
            self.losses["mse_losses"].append(mse.clone())
            self.losses["dvae_losses"].append(dvae.clone())
        self.last.update(mse=mse, mmd=mmd)
        return mse, spins

    # Below this many decoder rows (B * R) the prologue is left at the head of the decoder's forward: the extra fork / join
    # of the captured step costs 40-70 us (measured at B R = 2048 ... 16384), more than the 20-60 us the prologue takes
    # there; at 32768 rows it takes 190 us (the composed Linear o ConvTranspose weights) and the step gains 0.10-0.15 ms.
    PREPARE_DECODER_ROWS = 32768

    # Below this many decoder rows the three separate calls are kept: the fused tail's kernels redo the final layer's forward
    # in three passes and pay a per-block set-up per image at one image per block (measured: c3, 32768 rows, 8.12 -> 8.05 ms;
    # c2, 2048 rows, 0.880 -> 0.888 ms)
    FUSE_DECODER_MSE_ROWS = 8192

    def _prepare_decoder(self, images, main) -> None:
        """The decoder's weight-only prologue (packs, composed weights, dropout masks: ``Decoder.prepare``) on a stream
        forked off the main stream where the step starts: it runs beside the encoder instead of between the spins and
        the decoder's first GEMM, and the decoder's forward joins it.  ``prepare_decoder`` = True / False forces it."""
        N = int(images.shape[0]) * self.N_REPLICAS
        # (... or where the prologue is long whatever the rows: from 512 latent spins up the composed Linear o ConvTranspose
        # weights of csrc/decoder.cpp -- two n x 4n x 4C GEMMs and an 8 n^2-entry pack -- are 0.29 ms at c5's n = 1024)
        n_lat = int(getattr(self, "n_latents", 0) or 0)
        big_prologue = n_lat >= 512 and N * n_lat >= (1 << 20)
        want = self.prepare_decoder if self.prepare_decoder is not None else (N >= self.PREPARE_DECODER_ROWS or big_prologue)
        if not want or self._device.type != "cuda":
            return
        if self._prep_stream is None:
            self._prep_stream = torch.cuda.Stream(device=self._device)
        self._prep_stream.wait_stream(main)  # (the previous step's Adam has landed)
        self._dvae.decoder.prepare(N, self._prep_stream)

    def _draw_overlapped(self):
        if self._device.type != "cuda":
            return None
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=self._device)
        main = torch.cuda.current_stream(self._device)
        self._side_stream.wait_stream(main)  # the previous step's GRBM update must have landed
        with torch.cuda.stream(self._side_stream), torch.no_grad():
            samples = self._grbm.sample(sampler=self.sampler, prefactor=self.PREFACTOR, linear_range=self.linear_range,
                                        quadratic_range=self.quadratic_range, device=self._device,
                                        sample_params=self.sampler_kwargs)
        samples.record_stream(main)
        return samples

    def _log(self, key: str, value: torch.Tensor):
        self.losses[key].append(value.item() if self.sync_losses else value.detach())

    def _dist_active(self) -> bool:
        return self.dist is not None and (self.dist.world_size > 1 or getattr(self.dist, "force", False))

    def _reduce_and_step(self, opt):
        if opt is self._dvae_optimizer and self._device.type == "cuda":
            # the decoder's backward ran with its weight-gradient join deferred (see _dvae_half): the encoder's backward
            # behind it joined the shared side stream already; this makes the ordering explicit whatever ran in between,
            # and only now are the decoder's workspace / gradient tensors handed back to the allocator
            self._join_deferred()
        if self._dist_active():
            opt.gather_grads()  # packed into this optimizer's part of the joint buffer; see _flush_dist
            if not self._capturing_split:  # (under capture the replay re-registers it: _step_graphed)
                self._pending.append(opt)
        else:
            opt.step()

    def _flush_dist(self):
        """The step's ONE collective (RCCL all-reduce, sum) and the Adam launches behind it; the 1/world_size of the
        mean is the Adam kernel's ``grad_scale``."""
        if not self._pending:
            return
        both = len(self._pending) == 2
        buf = self._joint_grad if both else self._pending[0].flat_grad
        self.dist.all_reduce_sum(buf)
        scale = 1.0 / self.dist.world_size
        for opt in self._pending:
            if opt is self._dvae_optimizer and self._pending_tail is not None:
                self._pending_tail.replay()  # the captured Adam launch (same grad_scale)
            else:
                opt.step(grad_scale=scale, gathered=True)
        self._pending = []
        self._pending_tail = None

    # ------------------------------------------------------------------ generation (tensor-returning core)
    @torch.no_grad()
    def generate_images(self, sharpen: bool = False, lower: float = LOWER_THRESHOLD, upper: float = UPPER_THRESHOLD,
                        betas=None, tempered=None) -> torch.Tensor:
        """Sampler -> decoder -> clip, the compute of /root/reference/src/model_wrapper.py:355-385
        (plotting left to the caller).  Returns (NUM_READS, 1, 32, 32) on the device.  ``betas``: a (S,) or
        (NUM_READS, S) schedule -- generate from FRESH annealed chains (``GibbsSampler.sample_annealed``) instead of the
        sampler's own draw.  ``tempered``: a mapping of :meth:`GibbsSampler.sample_tempered` keywords (``betas``: the
        ladder; ``num_sweeps``, ``swap_every``, ...) -- generate from the target rung of NUM_READS fresh parallel-tempering
        ladders instead.  One of the two at most."""
        images, _samples = self._generate(sharpen, lower, upper, betas, tempered)
        return images

    @torch.no_grad()
    def _generate(self, sharpen: bool, lower: float, upper: float, betas=None, tempered=None):
        if betas is not None and tempered is not None:
            raise ValueError("give betas (annealed chains) or tempered (parallel-tempering ladders), not both")
        if tempered is not None and ("betas" not in tempered or "num_ladders" in tempered):
            raise ValueError("tempered: a mapping of sample_tempered keywords with the ladder as 'betas' (num_ladders is NUM_READS)")
        # (rank-local, like save(): data-parallel callers run sync_buffers() on every rank first)
        self._dvae.eval()
        self._grbm.eval()
        if tempered is not None:
            kw = dict(tempered)
            samples = self._grbm.sample_tempered(self.sampler, kw.pop("betas"), prefactor=self.PREFACTOR,
                                                 linear_range=self.linear_range, quadratic_range=self.quadratic_range,
                                                 num_ladders=int(self.sampler_kwargs.get("num_reads", 1)), **kw).target
        elif betas is None:
            samples = self._grbm.sample(self.sampler, prefactor=self.PREFACTOR, device=self._device,
                                        linear_range=self.linear_range, quadratic_range=self.quadratic_range,
                                        sample_params=self.sampler_kwargs)
        else:
            samples = self.sampler.sample_annealed(self._grbm._linear, self._grbm._quadratic, self.PREFACTOR,
                                                   self.linear_range, self.quadratic_range, betas,
                                                   num_reads=int(self.sampler_kwargs.get("num_reads", 1)))
        images = self._dvae.decoder(samples.unsqueeze(1)).squeeze(1).clip(0.0, 1.0)
        if sharpen:
            over = (images > upper).to(images.dtype)   # heaviside(x, 0): strict
            under = (images > lower).to(images.dtype)
            images = (over + (1 - over) * images) * under
        return images, samples

    @torch.no_grad()
    def generate_variations(self, images: torch.Tensor, n_variations: int = 8, keep: float = 0.5,
                            sweeps: Optional[int] = None, sharpen: bool = False, lower: float = LOWER_THRESHOLD,
                            upper: float = UPPER_THRESHOLD, mask_seed: int = 0, return_latents: bool = False):
        """Variations of given images: encode -> hard spins (heaviside, H(0) = 0) -> hold ``round(keep n)`` of each
        image's spins and let the prior redraw the others (a conditional block-Gibbs draw, ``n_variations`` chains per
        image, free spins started from the INIT stream) -> decoder -> clip [-> sharpen as ``generate_images`` does].

        The held set of an image is drawn with a ``torch.Generator`` seeded by ``mask_seed`` and is the same for all of
        its variations.  Returns (B, n_variations, 1, 32, 32) on the device; with ``return_latents`` also the
        (B n_variations, n) spins and the (B, n) bool mask.  Rank-local, like ``generate_images``."""
        self._dvae.eval()
        self._grbm.eval()
        images = images.to(self._device)
        B, V = int(images.shape[0]), int(n_variations)
        if V < 1 or not 0.0 <= keep <= 1.0:
            raise ValueError(f"n_variations={n_variations} keep={keep}")
        spins = F.heaviside_latent_to_discrete(self._dvae.encoder(images)).squeeze(1)  # (B, n) +-1
        n = int(spins.shape[1])
        gen = torch.Generator().manual_seed(int(mask_seed))
        held = torch.zeros((B, n), dtype=torch.bool)
        n_held = int(round(keep * n))
        for b in range(B):
            held[b, torch.randperm(n, generator=gen)[:n_held]] = True
        held = held.to(self._device)
        start = spins.repeat_interleave(V, dim=0)
        samples = self._grbm.sample_conditional(self.sampler, start, held.repeat_interleave(V, dim=0),
                                                prefactor=self.PREFACTOR, linear_range=self.linear_range,
                                                quadratic_range=self.quadratic_range, sweeps=sweeps)
        out = self._dvae.decoder(samples.unsqueeze(1)).squeeze(1).clip(0.0, 1.0)
        if sharpen:
            over = (out > upper).to(out.dtype)
            under = (out > lower).to(out.dtype)
            out = (over + (1 - over) * out) * under
        out = out.reshape(B, V, *out.shape[1:])
        return (out, samples, held) if return_latents else out

    @torch.no_grad()
    def prior_log_likelihood(self, images: torch.Tensor, *, num_sweeps: int = 1000, num_reads: int = 1024, method: str = "ais",
                             num_populations: int = 8):
        """How well the prior fits given images' latent codes: encode -> hard spins (heaviside, H(0) = 0, as
        ``generate_variations`` does) -> ``log p(spins)`` under the distribution the sampler draws from
        (``GraphRestrictedBoltzmannMachine.log_likelihood``), with ``log Z`` from one AIS run of ``num_reads`` chains
        over ``num_sweeps`` sweeps.  Returns the (B,) float64 log-likelihoods on the device and the ``LogPartition``
        result (its ``std_err`` is the estimate's).  ``method="population"``: ``log Z`` from a population-annealing draw of
        ``num_reads`` chains in ``num_populations`` populations over the same sweeps instead, the result a
        ``sampler.Population``.  Rank-local and eval-mode, like ``generate_images``."""
        self._dvae.eval()
        self._grbm.eval()
        images = images.to(self._device)
        spins = F.heaviside_latent_to_discrete(self._dvae.encoder(images)).squeeze(1)  # (B, n) +-1
        ranges = dict(prefactor=self.PREFACTOR, linear_range=self.linear_range, quadratic_range=self.quadratic_range)
        extra = dict(method=method, num_populations=num_populations) if method != "ais" else {}
        result = self._grbm.log_partition(self.sampler, num_sweeps=num_sweeps, num_reads=num_reads, **extra, **ranges)
        return self._grbm.log_likelihood(spins, self.sampler, log_z=result.log_z, **ranges), result

    @torch.no_grad()
    def prior_log_evidence(self, images: torch.Tensor, chains_per_image: int = 64, num_sweeps: int = 100, **kw):
        """How much prior mass agrees with what the encoder believes about each image: ``log sum_z p(z) q(z | x)``, ``p`` the
        distribution the sampler draws from and ``q`` the encoder's factorial posterior with logits ``l`` -- encode -> logits
        -> ``GraphRestrictedBoltzmannMachine.log_evidence`` (``chains_per_image`` chains per image started from draws of the
        prior, the image's evidence turned on over ``num_sweeps`` sweeps and every step weighed inside the kernel; ``burn_in``
        and ``start`` are passed on) -> ``log_ratio - sum_i log(2 cosh(l_i / 2))``, since ``q(z | x) = prod_i exp(l_i z_i / 2) /
        (2 cosh(l_i / 2))``.  No estimate of ``log Z`` is needed, and no code is hardened as ``prior_log_likelihood`` does.  This
        is ``log sum_z p(z) q(z | x)`` exactly (in expectation of the weights) where no ``linear_range`` clamps the sum of the
        prior's linear terms and the evidence; a range that does caps the evidence with it.  Returns the (B,) float64 values
        on the device and the ``sampler.LogEvidence`` (its ``std_err`` is the estimate's, per image).  Rank-local and
        eval-mode, like ``prior_log_likelihood``; of the sampler's counters only ``field_sweep_count`` and
        ``field_ais_sweep_count`` move."""
        self._dvae.eval()
        self._grbm.eval()
        images = images.to(self._device)
        logits = self._dvae.encoder(images).to(torch.float32)  # (B, n)
        ranges = dict(prefactor=self.PREFACTOR, linear_range=self.linear_range, quadratic_range=self.quadratic_range)
        result = self._grbm.log_evidence(self.sampler, logits, chains_per_row=chains_per_image, num_sweeps=num_sweeps, **kw, **ranges)
        half = 0.5 * logits.to(torch.float64).abs()
        log_norm = (half + torch.log1p(torch.exp(-2.0 * half))).sum(dim=1)  # sum_i log(2 cosh(l_i / 2)), without overflow
        return result.log_ratio - log_norm, result

    @torch.no_grad()
    def prior_pseudo_likelihood(self, images: torch.Tensor, **kw) -> dict:
        """How well the prior fits given images' latent codes WITHOUT an estimate of ``log Z``: encode ``images`` -> hard spins
        (heaviside, H(0) = 0, as ``prior_log_likelihood`` does) -> their :class:`~.sampler.PseudoLikelihood` under the prior
        at the sampler's beta (``GraphRestrictedBoltzmannMachine.pseudo_likelihood``), beside that of the records of one
        traced draw from the prior itself (``num_reads``, ``num_sweeps``, ``burn_in``, ``thin``, ``start`` are passed on,
        ``num_reads`` defaults to NUM_READS).  Returns a dict: ``data`` / ``prior``, the two; ``gap`` = ``data.per_spin -
        prior.per_spin`` -- at or above 0 the codes look like the prior's own draws spin by spin, far below they do not;
        ``local_minimum_share_prior``: the share of the draw's records that sit in a local minimum of the energy.  Rank-local
        and eval-mode, like ``prior_overlap``; of the sampler's counters only ``trace_sweep_count`` moves."""
        self._dvae.eval()
        self._grbm.eval()
        images = images.to(self._device)
        spins = F.heaviside_latent_to_discrete(self._dvae.encoder(images)).squeeze(1)  # (B, n) +-1
        ranges = dict(prefactor=self.PREFACTOR, linear_range=self.linear_range, quadratic_range=self.quadratic_range)
        beta = float(self.sampler.beta)
        if "num_reads" not in kw and "start" not in kw:
            kw["num_reads"] = int(self.sampler_kwargs.get("num_reads", 1))
        data = self._grbm.pseudo_likelihood(spins, beta=beta, **ranges)
        trace = self._grbm.sample_trace(self.sampler, **ranges, **kw)
        prior = self._grbm.pseudo_likelihood(trace.bits, beta=beta, **ranges)
        return dict(data=data, prior=prior, gap=data.per_spin - prior.per_spin, local_minimum_share_prior=prior.local_minimum_share)

    @torch.no_grad()
    def prior_minima(self, images: torch.Tensor = None, max_sweeps: int = 1000, **kw) -> dict:
        """The local minima of the prior's energy that its own draws sit above, and whether given images' latent codes drain
        into the same ones: the records of one traced draw from the prior (``num_reads``, ``num_sweeps``, ``burn_in``,
        ``thin``, ``start`` are passed on, ``num_reads`` defaults to NUM_READS) taken by zero-temperature descent to their
        :class:`~.sampler.Minima` (``GraphRestrictedBoltzmannMachine.descend``).  Returns a dict: ``prior``, those; with
        ``images`` also ``data``, the ``Minima`` of their hard spins (heaviside, H(0) = 0, as ``prior_log_likelihood`` does),
        and ``shared``, the share of the data's distinct minima that are also among the prior's (the packed rows compared
        exactly).  Rank-local and eval-mode, like ``prior_overlap``; of the sampler's counters only ``trace_sweep_count``
        moves."""
        self._dvae.eval()
        self._grbm.eval()
        ranges = dict(prefactor=self.PREFACTOR, linear_range=self.linear_range, quadratic_range=self.quadratic_range)
        if "num_reads" not in kw and "start" not in kw:
            kw["num_reads"] = int(self.sampler_kwargs.get("num_reads", 1))
        trace = self._grbm.sample_trace(self.sampler, **ranges, **kw)
        out = dict(prior=self._grbm.descend(trace.bits, max_sweeps=max_sweeps, **ranges))
        if images is not None:
            spins = F.heaviside_latent_to_discrete(self._dvae.encoder(images.to(self._device))).squeeze(1)  # (B, n) +-1
            out["data"] = data = self._grbm.descend(spins, max_sweeps=max_sweeps, **ranges)
            mine, theirs = data.unique()[0], out["prior"].unique()[0]
            _rows, counts = torch.unique(torch.cat([mine, theirs]), dim=0, return_counts=True)  # (each side's rows are distinct)
            out["shared"] = (counts == 2).sum().to(torch.float64) / float(mine.shape[0])
        return out

    @torch.no_grad()
    def prior_moments(self, **kw):
        """The prior's moments ``<s_i>``, ``<s_i s_j>`` under the distribution the sampler draws from, over every record of
        one traced draw (``GraphRestrictedBoltzmannMachine.model_moments``; ``num_reads``, ``num_sweeps``, ``burn_in``,
        ``thin``, ``start`` are passed on, ``num_reads`` defaults to NUM_READS).  Returns ``(mean_spin, mean_pair)`` float64
        on the device, shaped like the GRBM's ``linear`` / ``quadratic``.  Rank-local and eval-mode, like ``generate_images``."""
        self._dvae.eval()
        self._grbm.eval()
        if "num_reads" not in kw and "start" not in kw:
            kw["num_reads"] = int(self.sampler_kwargs.get("num_reads", 1))
        return self._grbm.model_moments(self.sampler, prefactor=self.PREFACTOR, linear_range=self.linear_range,
                                        quadratic_range=self.quadratic_range, **kw)

    @torch.no_grad()
    def prior_correlations(self, **kw):
        """The prior's correlations between EVERY pair of latent spins under the distribution the sampler draws from: the
        :class:`~.sampler.Correlations` over every record of one traced draw
        (``GraphRestrictedBoltzmannMachine.model_correlations``; ``num_reads``, ``num_sweeps``, ``burn_in``, ``thin``, ``start``
        are passed on, ``num_reads`` defaults to NUM_READS) -- ``chi_sg``, and through ``off_edge_share(graph)`` how much of
        the prior's correlation sits on pairs the graph has no coupling for.  Rank-local and eval-mode, like ``prior_overlap``;
        of the sampler's counters only ``trace_sweep_count`` moves."""
        self._dvae.eval()
        self._grbm.eval()
        if "num_reads" not in kw and "start" not in kw:
            kw["num_reads"] = int(self.sampler_kwargs.get("num_reads", 1))
        return self._grbm.model_correlations(self.sampler, prefactor=self.PREFACTOR, linear_range=self.linear_range,
                                             quadratic_range=self.quadratic_range, **kw)

    @torch.no_grad()
    def latent_correlation_gap(self, images: torch.Tensor, k: int = 16, **kw) -> dict:
        """Is the graph rich enough for the encoder's latent code?  Encode ``images`` -> hard spins (heaviside, H(0) = 0, as
        ``latent_novelty`` does) -> packed rows (``sampler.pack_spins``) -> their full :class:`~.sampler.Correlations`
        (``dvg_packed_correlation``), set against the prior's from one traced draw (:meth:`prior_correlations`, ``**kw``
        passed on).  Returns a dict: ``data`` / ``prior``, the two :class:`~.sampler.Correlations`; ``spin_rms``,
        ``pair_rms``, ``edge_rms``, ``off_edge_rms`` of ``data.gap(prior, graph)`` -- the quasi-NLL gradient matches the
        edges only, so ``off_edge_rms`` beside ``edge_rms`` is what training cannot close; ``off_edge_share_data``, the share
        of the data's squared connected correlation on pairs that are not edges; ``top_pairs``, ``(i, j, value)`` of the
        ``k`` non-edges of largest |C_ij| in the data: the couplings the graph lacks most.  Rank-local and eval-mode, like
        ``prior_overlap``."""
        from .sampler import Correlations, pack_spins

        self._dvae.eval()
        self._grbm.eval()
        images = images.to(self._device)
        spins = F.heaviside_latent_to_discrete(self._dvae.encoder(images)).squeeze(1)  # (B, n) +-1
        n = int(spins.shape[1])
        spin_sum, pair_sum = F.packed_correlation(pack_spins(spins), n=n)
        data = Correlations.from_sums(spin_sum, pair_sum, int(spins.shape[0]))
        prior = self.prior_correlations(**kw)
        plan = self._grbm.plan
        return dict(data=data, prior=prior, **data.gap(prior, plan), off_edge_share_data=data.off_edge_share(plan),
                    top_pairs=data.top_pairs(k, plan))

    @torch.no_grad()
    def prior_mixing(self, max_lag=None, **kw):
        """How the sampler's chains mix on the prior: the :class:`~.sampler.Autocorrelation` of one traced draw
        (``GraphRestrictedBoltzmannMachine.mixing``; ``num_reads``, ``num_sweeps``, ``burn_in``, ``thin``, ``start`` are
        passed on, ``num_reads`` defaults to NUM_READS) over lags 0 .. ``max_lag`` records -- ``tau_int_sweeps`` is the
        number of sweeps between two independent samples.  Rank-local and eval-mode, like ``prior_moments``."""
        self._dvae.eval()
        self._grbm.eval()
        if "num_reads" not in kw and "start" not in kw:
            kw["num_reads"] = int(self.sampler_kwargs.get("num_reads", 1))
        return self._grbm.mixing(self.sampler, prefactor=self.PREFACTOR, linear_range=self.linear_range,
                                 quadratic_range=self.quadratic_range, max_lag=max_lag, **kw)

    @torch.no_grad()
    def prior_energy_mixing(self, max_lag=None, **kw):
        """How the sampler's chains mix in energy on the prior: the :class:`~.sampler.EnergySeries` of one traced draw
        (``GraphRestrictedBoltzmannMachine.energy_mixing``; ``num_reads``, ``num_sweeps``, ``burn_in``, ``thin``, ``start`` are
        passed on, ``num_reads`` defaults to NUM_READS) over lags 0 .. ``max_lag`` records -- the energy's ``tau_int_sweeps``
        bounds how slowly the chains mix, its ``r_hat`` says whether they found the same basin.  Rank-local and eval-mode,
        like ``prior_mixing``; of the sampler's counters only ``trace_sweep_count`` moves."""
        self._dvae.eval()
        self._grbm.eval()
        if "num_reads" not in kw and "start" not in kw:
            kw["num_reads"] = int(self.sampler_kwargs.get("num_reads", 1))
        return self._grbm.energy_mixing(self.sampler, prefactor=self.PREFACTOR, linear_range=self.linear_range,
                                        quadratic_range=self.quadratic_range, max_lag=max_lag, **kw)

    @torch.no_grad()
    def prior_tempered_mixing(self, betas, max_lag=None, **kw):
        """Does tempering help under the trained prior?  One traced exchange draw over the ladder ``betas`` and one plain traced
        draw of the same sweeps, chains, ``burn_in`` and ``thin`` at ``betas[-1]``
        (``GraphRestrictedBoltzmannMachine.tempered_mixing``; ``num_ladders``, ``num_sweeps``, ``swap_every``, ``burn_in``,
        ``thin`` are passed on, ``num_ladders`` defaults to NUM_READS), over lags 0 .. ``max_lag`` records.  Returns a dict:
        ``tempered_autocorrelation`` / ``tempered_energy`` of the target rung, ``plain_autocorrelation`` / ``plain_energy`` of
        the plain draw, and the ladder's ``acceptance_rate``, ``round_trips`` and ``flow``.  Rank-local and eval-mode, like
        ``prior_energy_mixing``; of the sampler's counters only ``pt_sweep_count`` and ``trace_sweep_count`` move."""
        self._dvae.eval()
        self._grbm.eval()
        if "num_ladders" not in kw:
            kw["num_ladders"] = int(self.sampler_kwargs.get("num_reads", 1))
        return self._grbm.tempered_mixing(self.sampler, betas, prefactor=self.PREFACTOR, linear_range=self.linear_range,
                                          quadratic_range=self.quadratic_range, max_lag=max_lag, **kw)

    @torch.no_grad()
    def prior_overlap(self, **kw):
        """Which modes the sampler's chains populate on the prior: the :class:`~.sampler.Overlap` between distinct chains at
        equal times of one traced draw (``GraphRestrictedBoltzmannMachine.replica_overlap``; ``num_reads``, ``num_sweeps``,
        ``burn_in``, ``thin``, ``start`` are passed on, ``num_reads`` defaults to NUM_READS) -- ``q2``, ``binder`` and
        ``mass`` tell one mode from two mirror modes from many.  Rank-local and eval-mode, like ``prior_mixing``."""
        self._dvae.eval()
        self._grbm.eval()
        if "num_reads" not in kw and "start" not in kw:
            kw["num_reads"] = int(self.sampler_kwargs.get("num_reads", 1))
        return self._grbm.replica_overlap(self.sampler, prefactor=self.PREFACTOR, linear_range=self.linear_range,
                                          quadratic_range=self.quadratic_range, **kw)

    @torch.no_grad()
    def prior_link_overlap(self, **kw):
        """Whether the sampler's chains differ by compact domains or everywhere on the prior: the
        :class:`~.sampler.LinkOverlap` between distinct chains at equal times of one traced draw
        (``GraphRestrictedBoltzmannMachine.link_overlap``; ``num_reads``, ``num_sweeps``, ``burn_in``, ``thin``, ``start`` are
        passed on, ``num_reads`` defaults to NUM_READS) -- ``link_given_q`` against ``q``, ``corr_q2_link`` and ``fit()``.
        Rank-local and eval-mode, like ``prior_overlap``."""
        self._dvae.eval()
        self._grbm.eval()
        if "num_reads" not in kw and "start" not in kw:
            kw["num_reads"] = int(self.sampler_kwargs.get("num_reads", 1))
        return self._grbm.link_overlap(self.sampler, prefactor=self.PREFACTOR, linear_range=self.linear_range,
                                       quadratic_range=self.quadratic_range, **kw)

    @torch.no_grad()
    def latent_novelty(self, images: torch.Tensor, samples: Optional[torch.Tensor] = None) -> dict:
        """How far generated latents lie from the data's: encode ``images`` -> hard spins (heaviside, H(0) = 0, as
        ``generate_variations`` does) -> packed rows (``sampler.pack_spins``); ``samples`` (rows, n) +-1 spins, or None for
        one draw of the sampler as ``generate_images`` takes it.  Returns a dict: ``nearest_dist`` / ``nearest_row`` (rows,)
        int32, each generated latent's Hamming distance to its nearest data latent and that latent's index in ``images``;
        ``overlap``, the :class:`~.sampler.Overlap` of all (generated, data) pairs; ``data_nearest_dist`` (B,) int32, every
        data latent's distance to its nearest OTHER data latent (-1 for a single image) -- the baseline to read the first
        against: generated codes far closer than that are copies, far further are codes the encoder never emits.
        Rank-local and eval-mode, like ``generate_images``."""
        from .sampler import Overlap, pack_spins

        self._dvae.eval()
        self._grbm.eval()
        images = images.to(self._device)
        spins = F.heaviside_latent_to_discrete(self._dvae.encoder(images)).squeeze(1)  # (B, n) +-1
        n = int(spins.shape[1])
        if samples is None:
            samples = self._grbm.sample(self.sampler, prefactor=self.PREFACTOR, device=self._device,
                                        linear_range=self.linear_range, quadratic_range=self.quadratic_range,
                                        sample_params=self.sampler_kwargs)
        samples = samples.to(self._device)
        if samples.dim() != 2 or int(samples.shape[1]) != n:
            raise ValueError(f"samples must be (rows, {n}) spins, got {tuple(samples.shape)}")
        data, drawn = pack_spins(spins), pack_spins(samples)
        hist, (dist, row) = F.packed_overlap(drawn, data, n=n, nearest=True)
        _hist, (data_dist, _row) = F.packed_overlap(data, n=n, nearest=True)
        return dict(nearest_dist=dist, nearest_row=row, overlap=Overlap.from_hist(hist, n), data_nearest_dist=data_dist)

    @torch.no_grad()
    def prior_distinct(self, **kw):
        """How many distinct states one draw of the sampler holds on the prior: the :class:`~.sampler.Distinct` of the draw
        ``generate_images`` takes (``kw`` go on top of the sampler's keyword arguments, ``num_reads`` for instance) --
        ``distinct``, ``entropy``, ``collision_share``, ``unseen_mass``.  Rank-local and eval-mode, like ``generate_images``."""
        from .sampler import distinct, pack_spins

        self._dvae.eval()
        self._grbm.eval()
        samples = self._grbm.sample(self.sampler, prefactor=self.PREFACTOR, device=self._device, linear_range=self.linear_range,
                                    quadratic_range=self.quadratic_range, sample_params=dict(self.sampler_kwargs, **kw))
        return distinct(pack_spins(samples.to(self._device)), n=int(samples.shape[1]))

    @torch.no_grad()
    def latent_usage(self, images: torch.Tensor, samples: Optional[torch.Tensor] = None) -> dict:
        """Exact copies between generated and data latents, and how many codes the encoder uses: ``images`` and ``samples``
        are encoded, packed and drawn as ``latent_novelty`` does.  Returns a dict: ``data``, the :class:`~.sampler.Distinct` of
        the data latents (few classes: the encoder collapses onto a few codes); ``drawn``, the :class:`~.sampler.Distinct` of
        the generated latents with the data latents looked up among them; ``copied_share``, the share of generated rows that
        are exactly a data code (``latent_novelty``'s ``nearest_dist == 0``); ``data_found_share``, the share of data rows
        whose code the draw contains -- float64 scalars on the device.  Rank-local and eval-mode, like ``generate_images``."""
        from .sampler import distinct, pack_spins

        self._dvae.eval()
        self._grbm.eval()
        images = images.to(self._device)
        spins = F.heaviside_latent_to_discrete(self._dvae.encoder(images)).squeeze(1)  # (B, n) +-1
        n = int(spins.shape[1])
        if samples is None:
            samples = self._grbm.sample(self.sampler, prefactor=self.PREFACTOR, device=self._device,
                                        linear_range=self.linear_range, quadratic_range=self.quadratic_range,
                                        sample_params=self.sampler_kwargs)
        samples = samples.to(self._device)
        if samples.dim() != 2 or int(samples.shape[1]) != n:
            raise ValueError(f"samples must be (rows, {n}) spins, got {tuple(samples.shape)}")
        data, drawn = pack_spins(spins), pack_spins(samples)
        of_data, of_drawn = distinct(data, n=n), distinct(drawn, data, n=n)
        copied = (of_drawn.other_hits > 0)[of_drawn.index.to(torch.int64)].to(torch.float64).mean()
        return dict(data=of_data, drawn=of_drawn, copied_share=copied, data_found_share=of_drawn.coverage[0])

    @torch.no_grad()
    def reconstruct_images(self, batch: Optional[torch.Tensor] = None, sharpen: bool = False,
                           lower: float = LOWER_THRESHOLD, upper: float = UPPER_THRESHOLD) -> torch.Tensor:
        """Eval-mode encode -> discretise -> decode of one batch of training images, interleaved with the originals:
        the compute of /root/reference/src/model_wrapper.py:447-481 (plotting left to the caller).  Returns
        (2 B, 1, 32, 32) on the device in the reference's ``(b i)`` order: original 0, reconstruction 0, original 1, ...;
        the reconstruction's last pixel column is set to 1 (the reference's separator line, :465)."""
        if batch is None:
            if self._dataloader is None:
                self._load_dataset(batch_size=self.BATCH_SIZE, dataset_size=self.DATASET_SIZE)
            from .data import preview_batch

            batch = preview_batch(self._dataloader)[0]  # never advances the training permutation stream
        batch = batch.to(self._device)
        self._dvae.eval()
        self._grbm.eval()
        _, _, reconstructed = self._dvae(batch)
        reconstructed = reconstructed.clone()
        reconstructed[:, :, :, :, -1] = 1.0
        rec = reconstructed.clip(0.0, 1.0).squeeze(1)
        images = torch.stack((batch, rec), dim=1).reshape(-1, *batch.shape[1:])
        if sharpen:
            over = (images > upper).to(images.dtype)
            under = (images > lower).to(images.dtype)
            images = (over + (1 - over) * images) * under
        return images


    # ------------------------------------------------------------------ the reference's figure-returning entry points
    # (called by /root/reference/src/utils/callback_helpers.py:206-215 and /root/reference/demo_callbacks.py:781-785:
    # same names, arguments, side files and return types; the compute is generate_images / reconstruct_images above)
    @staticmethod
    def _image_figure(grid: torch.Tensor, save_to_file: str = ""):
        import plotly.express as px

        fig = px.imshow(grid.permute(1, 2, 0).cpu().numpy())
        fig.update_xaxes(showticklabels=False)
        fig.update_yaxes(showticklabels=False)
        fig.update_layout(margin={"t": 0, "l": 0, "b": 0, "r": 0})
        if save_to_file:
            with open(save_to_file, "w") as f:
                f.write(fig.to_json())
        return fig

    def generate_output(self, latent_qpu_file: str, sharpen: bool = False, save_to_file: str = ""):
        """/root/reference/src/model_wrapper.py:355-399: one sampler draw -> decoder (eval) -> clip [-> sharpen] -> a
        16-per-row grid as a plotly figure; the first sample's spins go to ``latent_qpu_file`` (JSON list)."""
        import json

        from . import viz

        images, samples = self._generate(sharpen, viz.LOWER_THRESHOLD, viz.UPPER_THRESHOLD)
        with open(latent_qpu_file, "w") as f:
            json.dump(samples[0].tolist(), f)
        return self._image_figure(viz.make_grid(images.cpu(), nrow=16), save_to_file)

    def generate_reconstucted_samples(self, sharpen: bool = False, save_to_file: str = ""):
        """/root/reference/src/model_wrapper.py:447-491 (the reference's spelling): first batch of the dataloader,
        eval-mode reconstruction, originals and reconstructions interleaved in a 16-per-row grid without padding;
        the sharpening, when asked for, is applied to the grid as the reference does."""
        from . import viz

        images = self.reconstruct_images(None, sharpen=False)
        grid = viz.make_grid(images.cpu(), nrow=16, padding=0)
        if sharpen:
            grid = viz.sharpen(grid)
        return self._image_figure(grid, save_to_file)

    def generate_loss_plot(self, save_to_file_mse: str = "", save_to_file_total: str = "", old_loss_data=None):
        """/root/reference/src/model_wrapper.py:401-445: the MSE and MSE + MMD curves as two plotly figures."""
        import plotly.graph_objects as go

        mse_losses = [float(v) for v in self.losses["mse_losses"]]
        dvae_losses = [float(v) for v in self.losses["dvae_losses"]]
        if old_loss_data:
            mse_losses = list(old_loss_data["mse_losses"]) + mse_losses
            dvae_losses = list(old_loss_data["dvae_losses"]) + dvae_losses
        figs = []
        for ys, path in ((mse_losses, save_to_file_mse), (dvae_losses, save_to_file_total)):
            fig = go.Figure()
            fig.add_trace(go.Scatter(x=list(range(len(mse_losses))), y=ys))
            fig.update_xaxes(title_text="Batch")
            fig.update_yaxes(title_text="Loss")
            fig.update_layout(margin={"t": 0, "l": 0, "b": 0, "r": 0})
            if path:
                with open(path, "w") as f:
                    f.write(fig.to_json())
            figs.append(fig)
        return figs[0], figs[1]


class _DeferredAdam:
    """Placeholder used when no GPU is present (CPU-side construction / checkpoint tests): it keeps
    the optimizer surface (``param_groups``, ``zero_grad``) and refuses to step: no CPU fallback."""

    def __init__(self, params, lr, weight_decay=0.0):
        self.params = list(params)
        self.param_groups = [dict(params=self.params, lr=lr, weight_decay=weight_decay)]

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def step(self, *a, **k):
        from ._lib import DvgError

        raise DvgError("optimizer step needs the HIP library and a GPU; there is no CPU fallback")

    def gather_grads(self):
        return self.step()
