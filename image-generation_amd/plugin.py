"""MI355X-native counterparts of the ``dwave.plugins.torch`` classes the reference uses
(/root/reference/src/model_wrapper.py:25-30): same names, constructor arguments,
attributes, ``state_dict`` keys and call signatures, with the arithmetic behind them
running in libdvg.so.

``dwave-pytorch-plugin`` is absent from the reference tree (requirements.txt:4); the
semantics follow the published API as restated (and documented, switch by switch) in
oracle/plugin.py and DESIGN.md.
"""
from __future__ import annotations

from typing import Callable, Iterable, Optional

import numpy as np
import torch

from . import _lib, functional as F
from .graphs import GibbsPlan, build_plan
from .sampler import GibbsSampler, GraphHandle, SampleSet, logit_fields


class DiscreteVariationalAutoencoder(torch.nn.Module):
    """``(latents, discretes, reconstructed) = dvae(x, n_samples)``
    (/root/reference/src/model_wrapper.py:184-188, :297)."""

    def __init__(self, encoder: torch.nn.Module, decoder: torch.nn.Module,
                 latent_to_discrete: Optional[Callable[[torch.Tensor, int], torch.Tensor]] = None):
        super().__init__()
        self._encoder = encoder
        self._decoder = decoder
        self._custom_l2d = latent_to_discrete
        self.gumbel_seed = 0          # device-RNG stream of the default latent_to_discrete
        self._gumbel_calls = 0
        self._injected_gumbels: Optional[torch.Tensor] = None

    @property
    def encoder(self):
        return self._encoder

    @property
    def decoder(self):
        return self._decoder

    def inject_gumbels(self, gumbels: Optional[torch.Tensor]):
        """Parity hook: Gumbel(0,1) noise (B,R,n,2) for the next default latent_to_discrete call."""
        self._injected_gumbels = gumbels

    def _default_l2d(self, logits: torch.Tensor, n_samples: int) -> torch.Tensor:
        g, self._injected_gumbels = self._injected_gumbels, None
        offset = self._gumbel_calls
        self._gumbel_calls += 1
        return F.gumbel_latent_to_discrete(logits, n_samples, gumbels=g, seed=self.gumbel_seed, offset=offset)

    def default_l2d_raw(self, logits: torch.Tensor, n_samples: int):
        """The default latent_to_discrete outside autograd: ``(spins, dspin)`` (same noise stream / injected noise as
        :meth:`_default_l2d`); ``None`` when a custom latent_to_discrete is installed."""
        if self._custom_l2d is not None:
            return None
        g, self._injected_gumbels = self._injected_gumbels, None
        offset = self._gumbel_calls
        self._gumbel_calls += 1
        return F.gumbel_forward_raw(logits, n_samples, gumbels=g, seed=self.gumbel_seed, offset=offset)

    @property
    def latent_to_discrete(self):
        return self._custom_l2d if self._custom_l2d is not None else self._default_l2d

    def forward(self, x: torch.Tensor, n_samples: int = 1):
        latents = self._encoder(x)
        discretes = self.latent_to_discrete(latents, n_samples)
        # the default latent_to_discrete is the library's Gumbel kernel, whose spins are exactly +-1: the package's own
        # decoder is told so (Decoder.forward: spins_pm1); a custom latent_to_discrete never makes that promise
        from .modules import Decoder
        if self._custom_l2d is None and isinstance(self._decoder, Decoder):
            return latents, discretes, self._decoder(discretes, spins_pm1=True)
        return latents, discretes, self._decoder(discretes)


class GraphRestrictedBoltzmannMachine(torch.nn.Module):
    """Fully-visible GRBM: parameters ``_linear`` (n), ``_quadratic`` (|E|) and the index
    buffers of the shipped checkpoints.  ``grbm(x)`` is the energy."""

    def __init__(self, nodes: Iterable, edges: Iterable):
        super().__init__()
        self._nodes = list(nodes)
        idx = {v: k for k, v in enumerate(self._nodes)}
        ei, ej = [], []
        for a, b in edges:
            ia, ib = idx[a], idx[b]
            ei.append(min(ia, ib))
            ej.append(max(ia, ib))
        n, ne = len(self._nodes), len(ei)
        self._linear = torch.nn.Parameter(0.05 * (2 * torch.rand(n) - 1))
        self._quadratic = torch.nn.Parameter(5.0 * (2 * torch.rand(ne) - 1))
        self.register_buffer("_edge_idx_i", torch.tensor(ei, dtype=torch.int64))
        self.register_buffer("_edge_idx_j", torch.tensor(ej, dtype=torch.int64))
        self.register_buffer("_visible_idx", torch.arange(n, dtype=torch.int64))
        for name in ("_hidden_idx", "_flat_adj", "_flat_j_idx", "_bin_idx"):
            self.register_buffer(name, torch.zeros(0, dtype=torch.int64))
        self._plan: Optional[GibbsPlan] = None
        self._handles = {}

    # -- graph plumbing --------------------------------------------------------------------
    @property
    def n_nodes(self) -> int:
        return len(self._nodes)

    @property
    def nodes(self):
        return list(self._nodes)

    @property
    def plan(self) -> GibbsPlan:
        if self._plan is None or self._plan.n_edges != self._edge_idx_i.numel():
            self._plan = build_plan(self.n_nodes, self._edge_idx_i.cpu().numpy(), self._edge_idx_j.cpu().numpy())
        return self._plan

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._plan = None  # the checkpoint's edge list is authoritative
        self._handles = {}

    def graph_handle(self, device) -> GraphHandle:
        key = str(torch.device(device))
        if key not in self._handles:
            self._handles[key] = GraphHandle(self.plan, device)
        return self._handles[key]

    # -- energy ---------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return F.grbm_energy(x, self._linear, self._quadratic, self.graph_handle(x.device))

    # -- sampling -------------------------------------------------------------------------
    def to_ising(self, prefactor: float, linear_range=None, quadratic_range=None):
        """(h, J) dicts handed to a generic sampler: prefactor-scaled, clamped to the solver ranges."""
        h = prefactor * self._linear.detach()
        J = prefactor * self._quadratic.detach()
        if linear_range is not None:
            h = h.clamp(*linear_range)
        if quadratic_range is not None:
            J = J.clamp(*quadratic_range)
        hd = dict(zip(self._nodes, h.tolist()))
        Jd = {(self._nodes[i], self._nodes[j]): v
              for i, j, v in zip(self._edge_idx_i.tolist(), self._edge_idx_j.tolist(), J.tolist())}
        return hd, Jd

    def sampleset_to_tensor(self, sample_set, device=None) -> torch.Tensor:
        dt = getattr(sample_set, "device_tensor", None)
        if dt is not None and list(sample_set.variables) == self._nodes:
            return dt if device is None else dt.to(device)
        col = {v: k for k, v in enumerate(sample_set.variables)}
        perm = [col[v] for v in self._nodes]
        t = torch.from_numpy(np.asarray(sample_set.record.sample)[:, perm].astype(np.float32))
        return t if device is None else t.to(device)

    def sample(self, sampler, *, prefactor: float, linear_range=None, quadratic_range=None, device=None,
               sample_params: Optional[dict] = None, as_tensor: bool = True):
        """Draw spin strings from the model (/root/reference/src/model_wrapper.py:309-316).

        With the local :class:`GibbsSampler` the GRBM parameters go to the kernel as device
        tensors (scaling and clamping happen in its prologue): no host round trip.  Any other
        ``sample_ising``-style sampler gets the (h, J) dicts like the plugin would send."""
        sample_params = dict(sample_params or {})
        if isinstance(sampler, GibbsSampler) and list(sampler.nodes) == self._nodes:
            num_reads = int(sample_params.get("num_reads", 1))
            t = sampler.sample_native(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, num_reads)
            if as_tensor:
                return t if device is None else t.to(device)
            return SampleSet(None, self._nodes, device_tensor=t)
        h, J = self.to_ising(prefactor, linear_range, quadratic_range)
        ss = sampler.sample_ising(h, J, **sample_params)
        return self.sampleset_to_tensor(ss, device) if as_tensor else ss

    def sample_conditional(self, sampler, start: torch.Tensor, clamp: torch.Tensor, *, prefactor: float,
                           linear_range=None, quadratic_range=None, sweeps: Optional[int] = None) -> torch.Tensor:
        """Draw from the model with the spins flagged in ``clamp`` held at their value in ``start`` (one chain per row
        of ``start``; :meth:`GibbsSampler.sample_conditional`, free spins started from the INIT stream).  The local
        :class:`GibbsSampler` only: a ``sample_ising``-style sampler has no conditional form."""
        if not (isinstance(sampler, GibbsSampler) and list(sampler.nodes) == self._nodes):
            raise TypeError("sample_conditional needs the local GibbsSampler built on this model's nodes, got "
                            f"{type(sampler).__name__}")
        return sampler.sample_conditional(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, start,
                                          clamp, sweeps=sweeps, init_free=True)


    def _need_local_sampler(self, sampler, what: str) -> None:
        if not (isinstance(sampler, GibbsSampler) and list(sampler.nodes) == self._nodes):
            raise TypeError(f"{what} needs the local GibbsSampler built on this model's nodes, got {type(sampler).__name__}")

    def log_partition(self, sampler, *, prefactor: float, linear_range=None, quadratic_range=None, method: str = "ais", **kw):
        """The AIS estimate of ``log Z`` of the distribution ``sampler`` draws from -- ``exp(-beta E_s)`` with ``E_s`` the
        energy under the prefactor-scaled, clamped ``(h, J)`` and ``beta = sampler.beta`` unless ``beta=`` says otherwise
        (:meth:`GibbsSampler.log_partition`; ``num_sweeps``, ``num_reads``, ``schedule`` are passed on).  The local
        :class:`GibbsSampler` only.

        ``method="population"``: population annealing instead (:meth:`sample_population`): ``betas = linspace(0, beta,
        num_sweeps + 1)[1:]`` at one sweep per beta, ``num_reads`` (default 1024) chains in ``num_populations`` (default 8)
        populations.  Returns the :class:`~.sampler.Population`, which has ``.log_z`` and ``.std_err`` like the
        :class:`~.sampler.LogPartition` of the default method."""
        self._need_local_sampler(sampler, "log_partition")
        if method not in ("ais", "population"):
            raise ValueError(f"method must be 'ais' or 'population', got {method!r}")
        if method == "ais":
            return sampler.log_partition(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, **kw)
        beta, num_sweeps = kw.pop("beta", None), kw.pop("num_sweeps", 1000)
        if isinstance(num_sweeps, bool) or int(num_sweeps) != num_sweeps or int(num_sweeps) < 1:
            raise ValueError(f"num_sweeps must be an integer >= 1, got {num_sweeps!r}")
        b = float(sampler.beta if beta is None else beta)
        if not np.isfinite(b) or b <= 0.0:
            raise ValueError(f"beta={beta!r} must be finite and > 0")
        betas = np.linspace(0.0, b, int(num_sweeps) + 1)[1:].astype(np.float32)
        return self.sample_population(sampler, betas, prefactor=prefactor, linear_range=linear_range, quadratic_range=quadratic_range,
                                      num_reads=kw.pop("num_reads", 1024), num_populations=kw.pop("num_populations", 8), **kw)

    def sample_fields(self, sampler, fields: torch.Tensor, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """Draw from the model with a linear field of its own per chain, ``(linear + fields[c], quadratic)`` -- soft evidence
        (:meth:`GibbsSampler.sample_fields`; ``start``, ``sweeps``, ``num_reads`` are passed on; ``sampler.logit_fields`` makes
        the fields of factorial logits).  Returns (C, n) float32 +-1 on the device.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "sample_fields")
        return sampler.sample_fields(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, fields, **kw)

    def log_evidence(self, sampler, logits: torch.Tensor, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """Per row of ``logits`` (rows, n), the log odds of ``z_i = +1`` under factorial evidence: the estimate of ``log sum_z
        p(z) prod_i exp(logits[r, i] z_i / 2)``, ``p`` the distribution ``sampler`` draws from under the prefactor-scaled,
        clamped ``(h, J)`` -- ``sampler.logit_fields`` followed by :meth:`GibbsSampler.log_evidence` (``chains_per_row``,
        ``num_sweeps``, ``burn_in``, ``start`` are passed on).  Exact in expectation where no ``linear_range`` clamps the sum
        of the linear terms and the fields.  Returns its :class:`~.sampler.LogEvidence`.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "log_evidence")
        fields = logit_fields(logits.to(self._linear.device), sampler.beta, prefactor)
        return sampler.log_evidence(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, fields, **kw)

    def sample_population(self, sampler, betas, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """A population-annealing draw from the model under the prefactor-scaled, clamped ``(h, J)``: chains annealed through
        ``betas`` and resampled in proportion to their weights after every step, on the device
        (:meth:`GibbsSampler.sample_population`; ``num_reads``, ``num_populations``, ``sweeps_per_beta``, ``history`` are
        passed on).  Returns its :class:`~.sampler.Population`: equally weighted samples at ``betas[-1]``, ``log_z``,
        ``std_err`` and the surviving families.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "sample_population")
        return sampler.sample_population(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, betas, **kw)

    def sample_tempered(self, sampler, betas, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """A parallel-tempering draw from the model under the prefactor-scaled, clamped ``(h, J)``: ladders of ``len(betas)``
        chains that exchange rungs inside the kernel (:meth:`GibbsSampler.sample_tempered`; ``num_ladders``, ``num_sweeps``,
        ``swap_every``, ``start``, ``rungs`` are passed on).  Returns its :class:`~.sampler.Tempered`; ``.target`` holds the
        samples at ``betas[-1]``.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "sample_tempered")
        return sampler.sample_tempered(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, betas, **kw)

    def sample_tempered_cluster(self, sampler, betas, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """A parallel-tempering draw of twin ladders with isoenergetic cluster moves between the twins' equal rungs, from
        the model under the prefactor-scaled, clamped ``(h, J)`` (:meth:`GibbsSampler.sample_tempered_cluster`;
        ``num_ladders``, ``num_sweeps``, ``swap_every``, ``cluster_every``, ``rung_from``, ``start``, ``rungs`` are passed
        on).  Returns its :class:`~.sampler.TemperedCluster`; ``.tempered.target`` holds the samples at ``betas[-1]``.  The
        local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "sample_tempered_cluster")
        return sampler.sample_tempered_cluster(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, betas, **kw)

    def sample_quantum(self, sampler, beta_slice, kappa, *, slices: int, prefactor: float, linear_range=None,
                       quadratic_range=None, **kw):
        """A simulated-quantum-annealing draw from the model under the prefactor-scaled, clamped ``(h, J)``: chains of
        ``slices`` Trotter slices under the per-sweep tables ``beta_slice`` and ``kappa`` -- ``sampler.transverse_schedule``
        makes them from a transverse-field schedule (:meth:`GibbsSampler.sample_quantum`; ``num_reads``, ``start`` are passed
        on).  Returns its :class:`~.sampler.Sliced`; ``.samples`` holds slice 0 of every chain.  The local
        :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "sample_quantum")
        return sampler.sample_quantum(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, beta_slice, kappa,
                                      slices=slices, **kw)

    def sample_trace(self, sampler, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """A traced draw from the model under the prefactor-scaled, clamped ``(h, J)``: the chains' states after every
        ``thin``-th sweep behind ``burn_in``, bit-packed inside the kernel (:meth:`GibbsSampler.sample_trace`; ``num_reads``,
        ``start``, ``num_sweeps``, ``burn_in``, ``thin`` are passed on).  Returns its :class:`~.sampler.Trace`.  The local
        :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "sample_trace")
        return sampler.sample_trace(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, **kw)

    @torch.no_grad()
    def model_moments(self, sampler, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """The model's moments ``<s_i>`` and ``<s_i s_j>`` estimated over every record of one traced draw
        (:meth:`sample_trace`, ``**kw`` passed on; the sums are exact integers, ``dvg_grbm_moments_packed``).  Returns
        ``(mean_spin, mean_pair)`` float64 on the device, shaped like ``linear`` / ``quadratic``.  The local
        :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "model_moments")
        trace = self.sample_trace(sampler, prefactor=prefactor, linear_range=linear_range, quadratic_range=quadratic_range, **kw)
        m = trace.moments(self.graph_handle(trace.bits.device))
        return m.mean_spin.reshape(self._linear.shape), m.mean_pair.reshape(self._quadratic.shape)

    @torch.no_grad()
    def model_correlations(self, sampler, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """The model's correlations between EVERY pair of spins, estimated over every record of one traced draw
        (:meth:`sample_trace`, ``**kw`` passed on; the sums are exact integers, ``dvg_packed_correlation``).  Returns the
        :class:`~.sampler.Correlations` (:meth:`Trace.correlations`): ``connected``, ``pearson``, ``chi_sg``,
        ``off_edge_share(graph)`` -- what :meth:`model_moments` cannot show, the pairs that are not edges.  The local
        :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "model_correlations")
        trace = self.sample_trace(sampler, prefactor=prefactor, linear_range=linear_range, quadratic_range=quadratic_range, **kw)
        return trace.correlations()

    @torch.no_grad()
    def mixing(self, sampler, *, prefactor: float, linear_range=None, quadratic_range=None, max_lag=None, **kw):
        """How the sampler's chains mix on this model: one traced draw (:meth:`sample_trace`, ``**kw`` passed on) and its
        :class:`~.sampler.Autocorrelation` over lags 0 .. ``max_lag`` records (:meth:`Trace.autocorrelation`): ``rho``,
        ``tau_int``, ``ess``, ``r_hat``.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "mixing")
        trace = self.sample_trace(sampler, prefactor=prefactor, linear_range=linear_range, quadratic_range=quadratic_range, **kw)
        return trace.autocorrelation(max_lag)

    @torch.no_grad()
    def energy_packed(self, bits: torch.Tensor, *, prefactor: float, linear_range=None, quadratic_range=None) -> torch.Tensor:
        """The float64 energies of bit-packed rows ((rows, W) or (C, M, W) int32 on the device: ``sampler.pack_spins``,
        ``Trace.bits``) under the prefactor-scaled, clamped ``(h, J)`` the samplers draw from (``dvg_grbm_energy_packed``:
        the rows stay packed); ``prefactor=1`` without ranges is ``grbm(x)`` of the unpacked rows, in float64."""
        if not torch.is_tensor(bits) or not bits.is_cuda:
            raise _lib.DvgError(f"bits must be a tensor on the GPU (got {bits.device if torch.is_tensor(bits) else type(bits).__name__}); "
                                "the HIP path has no CPU fallback")
        return F.grbm_energy_packed(bits, self.graph_handle(bits.device), self._linear, self._quadratic, prefactor=prefactor,
                                    linear_range=linear_range, quadratic_range=quadratic_range)

    @torch.no_grad()
    def energy_mixing(self, sampler, *, prefactor: float, linear_range=None, quadratic_range=None, max_lag=None, **kw):
        """How the sampler's chains mix in ENERGY on this model: one traced draw (:meth:`sample_trace`, ``**kw`` passed on)
        and the :class:`~.sampler.EnergySeries` of its records' energies under the same scaled, clamped ``(h, J)``
        (:meth:`Trace.energy_series`) over lags 0 .. ``max_lag`` records: ``tau_int``, ``ess``, ``r_hat``,
        ``heat_capacity``.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "energy_mixing")
        if max_lag is not None and (isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or max_lag < 0):
            raise ValueError(f"max_lag must be None or an integer >= 0, got {max_lag!r}")
        trace = self.sample_trace(sampler, prefactor=prefactor, linear_range=linear_range, quadratic_range=quadratic_range, **kw)
        return trace.energy_series(self.graph_handle(trace.bits.device), self._linear, self._quadratic, prefactor, linear_range,
                                   quadratic_range, max_lag=max_lag)

    def sample_tempered_trace(self, sampler, betas, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """A traced parallel-tempering draw from the model under the prefactor-scaled, clamped ``(h, J)``: :meth:`sample_tempered`
        with the ladders' history -- per rung the packed states and energies, per chain the rung walk -- written inside the
        kernel (:meth:`GibbsSampler.sample_tempered_trace`; ``num_ladders``, ``num_sweeps``, ``swap_every``, ``burn_in``,
        ``thin``, ``start``, ``rungs``, ``energies``, ``rung_walk`` are passed on).  Returns its
        :class:`~.sampler.TemperedTrace`.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "sample_tempered_trace")
        return sampler.sample_tempered_trace(self._linear, self._quadratic, prefactor, linear_range, quadratic_range, betas, **kw)

    @torch.no_grad()
    def tempered_mixing(self, sampler, betas, *, prefactor: float, linear_range=None, quadratic_range=None, max_lag=None, **kw):
        """Does tempering help on this model?  One traced exchange draw over the ladder ``betas`` (:meth:`sample_tempered_trace`;
        ``num_ladders``, ``num_sweeps``, ``swap_every``, ``burn_in``, ``thin`` are passed on) and one plain traced draw
        (:meth:`sample_trace`) of the same sweeps, ``burn_in``, ``thin`` and as many chains (``num_ladders``) at ``betas[-1]``
        -- the sampler's ``beta`` is set to it for that draw and put back.  Returns a dict: ``tempered_autocorrelation`` /
        ``tempered_energy`` (the target rung's :class:`~.sampler.Autocorrelation` and :class:`~.sampler.EnergySeries`, from the
        carried energies), ``plain_autocorrelation`` / ``plain_energy`` (the plain draw's, its energies exact:
        :meth:`Trace.energy_series`), ``acceptance_rate`` (R - 1,), ``round_trips`` (Q, R) and ``flow`` (R,) of the ladder.
        Compare the two ``tau_int_sweeps``: an exchange draw spends R chains per target sample.  The local
        :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "tempered_mixing")
        if max_lag is not None and (isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or max_lag < 0):
            raise ValueError(f"max_lag must be None or an integer >= 0, got {max_lag!r}")
        for name in ("start", "rungs", "energies", "rung_walk"):
            if name in kw:
                raise ValueError(f"tempered_mixing draws fresh ladders with every record: {name} is not an argument of it")
        ranges = dict(prefactor=prefactor, linear_range=linear_range, quadratic_range=quadratic_range)
        tt = self.sample_tempered_trace(sampler, betas, **ranges, **kw)
        plain_kw = {k: kw[k] for k in ("num_sweeps", "burn_in", "thin") if k in kw}
        beta = sampler.beta
        try:
            sampler.beta = float(tt.betas[-1])
            plain = self.sample_trace(sampler, num_reads=int(tt.bits.shape[0]), **ranges, **plain_kw)
        finally:
            sampler.beta = beta
        target = tt.target
        return dict(
            tempered_autocorrelation=target.autocorrelation(max_lag), tempered_energy=tt.energy_series(-1, max_lag),
            plain_autocorrelation=plain.autocorrelation(max_lag),
            plain_energy=plain.energy_series(self.graph_handle(plain.bits.device), self._linear, self._quadratic, prefactor,
                                             linear_range, quadratic_range, max_lag=max_lag),
            acceptance_rate=tt.final.acceptance_rate, round_trips=tt.round_trips(), flow=tt.flow())

    def _packed_bits(self, x_or_bits):
        """``x_or_bits`` on the GPU as bit-packed rows: int32 is taken as packed already, any other dtype as +-1 rows (..., n)."""
        from .sampler import pack_spins

        if not torch.is_tensor(x_or_bits) or not x_or_bits.is_cuda:
            raise _lib.DvgError("x_or_bits must be a tensor on the GPU (got "
                                f"{x_or_bits.device if torch.is_tensor(x_or_bits) else type(x_or_bits).__name__}); the HIP path has "
                                "no CPU fallback")
        bits = x_or_bits
        if bits.dtype != torch.int32:
            if bits.dim() < 2 or bits.shape[-1] != len(self._nodes):
                raise _lib.DvgError(f"x_or_bits: +-1 rows must be (..., {len(self._nodes)}), got {tuple(bits.shape)}")
            bits = pack_spins(bits.detach().reshape(-1, bits.shape[-1]) if bits.dim() > 3 else bits.detach())
        return bits

    @torch.no_grad()
    def pseudo_likelihood(self, x_or_bits: torch.Tensor, *, beta: float, prefactor: float, linear_range=None, quadratic_range=None):
        """The :class:`~.sampler.PseudoLikelihood` of spin rows under the prefactor-scaled, clamped ``(h, J)`` at ``beta``:
        ``sum_i log P(s_i | rest)`` per row -- the likelihood-type score that needs no ``log Z`` -- the rows' unstable spins,
        and the Rao-Blackwellised moments (``dvg_grbm_fields_packed``).  ``x_or_bits``: bit-packed rows ((rows, W) or (C, M, W)
        int32: ``Trace.bits``) or +-1 rows ((..., n), any other dtype; packed with ``sampler.pack_spins``), on the GPU."""
        from .sampler import pseudo_likelihood

        bits = self._packed_bits(x_or_bits)
        return pseudo_likelihood(bits, self.graph_handle(bits.device), self._linear, self._quadratic, beta=beta, prefactor=prefactor,
                                 linear_range=linear_range, quadratic_range=quadratic_range)

    @torch.no_grad()
    def pseudo_likelihood_grad(self, x_or_bits: torch.Tensor, *, beta: float, prefactor: float, linear_range=None,
                               quadratic_range=None):
        """``(mean log PL, grad_linear, grad_quadratic)``: the mean pseudo-log-likelihood of the rows
        (:meth:`pseudo_likelihood`) and its gradient with respect to this model's ``linear`` and ``quadratic``, float64 on the
        device and shaped like them -- ascend it and ``(h, J)`` are trained with no negative-phase sampler at all."""
        pl = self.pseudo_likelihood(x_or_bits, beta=beta, prefactor=prefactor, linear_range=linear_range,
                                    quadratic_range=quadratic_range)
        gl, gq = pl.grad(prefactor, self._linear, self._quadratic, linear_range, quadratic_range)
        return pl.mean, gl, gq

    @torch.no_grad()
    def descend(self, x_or_bits: torch.Tensor, *, prefactor: float, linear_range=None, quadratic_range=None, max_sweeps: int = 1000):
        """The :class:`~.sampler.Minima` of spin rows under the prefactor-scaled, clamped ``(h, J)``: every row taken by
        zero-temperature descent -- colour class by colour class every unstable spin flips -- to a local minimum of the
        energy, or through ``max_sweeps`` sweeps (``dvg_grbm_descend_packed``), with the energies before and after.
        ``x_or_bits``: bit-packed rows ((rows, W) or (C, M, W) int32: ``Trace.bits``) or +-1 rows ((..., n), any other dtype;
        packed with ``sampler.pack_spins``), on the GPU; it is left as it is."""
        from .sampler import descend

        bits = self._packed_bits(x_or_bits)
        return descend(bits, self.graph_handle(bits.device), self._linear, self._quadratic, prefactor=prefactor,
                       linear_range=linear_range, quadratic_range=quadratic_range, max_sweeps=max_sweeps)

    @torch.no_grad()
    def replica_overlap(self, sampler, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """Which modes the sampler's chains populate on this model: one traced draw (:meth:`sample_trace`, ``**kw`` passed
        on) and the :class:`~.sampler.Overlap` between its distinct chains at equal times (:meth:`Trace.overlap`): ``q2``,
        ``binder``, ``mass``.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "replica_overlap")
        trace = self.sample_trace(sampler, prefactor=prefactor, linear_range=linear_range, quadratic_range=quadratic_range, **kw)
        return trace.overlap()

    @torch.no_grad()
    def bonds(self, x_or_bits: torch.Tensor, satisfied: bool = False) -> torch.Tensor:
        """The bond rows of spin rows, bit-packed ((rows, WE) or (C, M, WE) int32, ``dvg_packed_bonds``): bit e set iff s_i s_j
        = +1 on edge e, or with ``satisfied=True`` iff the bond is satisfied under this model's couplings -- the popcount of
        such a row is its number of satisfied couplings.  ``x_or_bits``: bit-packed rows ((rows, W) or (C, M, W) int32:
        ``Trace.bits``) or +-1 rows ((..., n), any other dtype; packed with ``sampler.pack_spins``), on the GPU."""
        from .sampler import bonds

        bits = self._packed_bits(x_or_bits)
        return bonds(bits, self.graph_handle(bits.device), self._quadratic.detach() if satisfied else None)

    @torch.no_grad()
    def link_overlap(self, sampler, *, prefactor: float, linear_range=None, quadratic_range=None, **kw):
        """Do the sampler's chains differ by compact domains or everywhere?  One traced draw (:meth:`sample_trace`, ``**kw``
        passed on) and the :class:`~.sampler.LinkOverlap` between its distinct chains at equal times
        (:meth:`Trace.link_overlap`): ``link_given_q``, ``corr_q2_link``, ``fit()``.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "link_overlap")
        trace = self.sample_trace(sampler, prefactor=prefactor, linear_range=linear_range, quadratic_range=quadratic_range, **kw)
        return trace.link_overlap(self.graph_handle(trace.bits.device))

    @torch.no_grad()
    def log_likelihood(self, x: torch.Tensor, sampler, *, prefactor: float, linear_range=None, quadratic_range=None,
                       log_z=None, **kw) -> torch.Tensor:
        """``log p(x) = -beta E_s(x) - log Z`` per row of ``x`` ((B, n) +-1 on the device) under the distribution
        ``sampler`` draws from: ``E_s`` the energy under the scaled, clamped ``(h, J)`` (``dvg_grbm_energy``), ``beta =
        sampler.beta``.  ``log_z``: a value from :meth:`log_partition` (at that beta); None: estimated here, ``**kw``
        passed on.  With ``beta = 1 / prefactor`` and inactive clamps this is the GRBM's own ``log p(x)``.  Returns (B,)
        float64 on the device.  The local :class:`GibbsSampler` only."""
        self._need_local_sampler(sampler, "log_likelihood")
        if log_z is None:
            log_z = self.log_partition(sampler, prefactor=prefactor, linear_range=linear_range,
                                       quadratic_range=quadratic_range, **kw).log_z
        h = prefactor * self._linear.detach()
        J = prefactor * self._quadratic.detach()
        if linear_range is not None:
            h = h.clamp(*linear_range)
        if quadratic_range is not None:
            J = J.clamp(*quadratic_range)
        energy = F.grbm_energy(x, h, J, self.graph_handle(x.device))
        return -float(sampler.beta) * energy.double() - log_z


class GaussianKernel(torch.nn.Module):
    """Multi-bandwidth RBF kernel configuration (/root/reference/src/model_wrapper.py:273).

    The hot path never builds the kernel matrix: ``maximum_mean_discrepancy_loss`` hands this
    module's settings to the fused ``dvg_mmd_fwd_bwd``.  ``forward(x, y)`` (the explicit matrix)
    is kept for API compatibility as plain tensor algebra on the inputs' device."""

    def __init__(self, n_kernels: int, factor: float = 2.0, bandwidth: Optional[float] = None,
                 squared: bool = False, reduce: str = "sum"):
        super().__init__()
        self.register_buffer("factors", factor ** (torch.arange(n_kernels) - n_kernels // 2).to(torch.float32))
        self.n_kernels, self.factor, self.bandwidth = int(n_kernels), float(factor), bandwidth
        self.squared, self.reduce = bool(squared), reduce

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        d2 = ((x * x).sum(-1, keepdim=True) + (y * y).sum(-1, keepdim=True).T - 2.0 * (x @ y.T)).clamp_min(0.0)
        D = d2 if self.squared else torch.where(d2 > 0, torch.where(d2 > 0, d2, torch.ones_like(d2)).sqrt(), d2)
        N = D.shape[0]
        bw = D.detach().sum() / (N * N - N) if self.bandwidth is None else torch.as_tensor(self.bandwidth, device=D.device)
        K = torch.exp(-D.unsqueeze(0) / (bw * self.factors.to(D.device)).reshape(-1, 1, 1))
        return K.sum(0) if self.reduce == "sum" else K.mean(0)


def maximum_mean_discrepancy_loss(x: torch.Tensor, y: torch.Tensor, kernel: GaussianKernel, biased: bool = False):
    """MMD^2(x, y) under ``kernel`` with gradient wrt x (/root/reference/src/model_wrapper.py:320)."""
    return F.mmd_loss(x, y, n_kernels=kernel.n_kernels, factor=kernel.factor, bandwidth=kernel.bandwidth,
                      squared=kernel.squared, reduce_mean=(kernel.reduce == "mean"), biased=biased)


def maximum_mean_discrepancy_loss_and_grad(x: torch.Tensor, y: torch.Tensor, kernel: GaussianKernel, biased: bool = False):
    """Same value as :func:`maximum_mean_discrepancy_loss` plus its gradient wrt ``x``, both detached (the fused
    kernel computes them together anyway)."""
    return F.mmd_loss_and_grad(x, y, n_kernels=kernel.n_kernels, factor=kernel.factor, bandwidth=kernel.bandwidth,
                               squared=kernel.squared, reduce_mean=(kernel.reduce == "mean"), biased=biased)
