"""Local sampler: the on-GPU block-Gibbs stand-in for the QPU.

Mirrors the sampler side of the reference:
``get_sampler_and_sampler_kwargs`` (/root/reference/src/utils/common.py:103-140)
returns ``(sampler, sampler_kwargs, graph, linear_range, quadratic_range)`` where
``sampler.sample_ising(h, J, **sampler_kwargs)`` is a blocking QPU call.  Here
``sampler`` is a :class:`GibbsSampler` whose draw is ``dvg_gibbs_sample``
(include/dvg.h): many persistent chains, graph-coloured block-Gibbs sweeps.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Dict, Optional, Sequence, Tuple

import networkx as nx
import numpy as np
import torch

from . import _lib
from .graphs import LOCAL_SOLVERS, GibbsPlan, build_plan, edges_of, get_graph_mapping, greedy_get_subgraph


class GraphHandle:
    """Owns a ``dvg_graph_t`` (device copy of the plan) for one device."""

    def __init__(self, plan: GibbsPlan, device: torch.device):
        self.plan = plan
        self.device = torch.device(device)
        self._h = ctypes.c_void_p()
        L = _lib.lib()
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        arrs = [i32(plan.edge_i), i32(plan.edge_j), i32(plan.order), i32(plan.class_ptr), i32(plan.adj_ptr),
                i32(plan.adj_idx), i32(plan.adj_eid)]
        p = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) for a in arrs]
        with torch.cuda.device(self.device):
            _lib.check(
                L.dvg_graph_create(plan.n, plan.n_edges, p[0], p[1], p[2], p[3], plan.n_colours, p[4], p[5], p[6],
                                   ctypes.byref(self._h)),
                "dvg_graph_create",
            )

    @property
    def ptr(self):
        return self._h

    def __del__(self):
        try:
            if self._h:
                _lib.lib().dvg_graph_destroy(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass


def beta_schedule(beta_start: float, beta_end: float, num_sweeps: int, kind: str = "geometric") -> np.ndarray:
    """The inverse temperature of each sweep of an annealed draw, ``num_sweeps`` float32 values from ``beta_start`` (hot)
    to ``beta_end`` (the target), as ``neal.SimulatedAnnealingSampler`` spaces them: ``kind`` "geometric" (both ends > 0)
    or "linear".  The points are computed in float64 (``np.geomspace`` / ``np.linspace``) and rounded to float32; the
    first entry is ``float32(beta_start)``, the last ``float32(beta_end)``; ``num_sweeps == 1`` gives ``[beta_end]``."""
    if kind not in ("geometric", "linear"):
        raise ValueError(f"beta schedule kind must be 'geometric' or 'linear', got {kind!r}")
    if isinstance(num_sweeps, bool) or int(num_sweeps) != num_sweeps or int(num_sweeps) < 1:
        raise ValueError(f"num_sweeps must be an integer >= 1, got {num_sweeps!r}")
    num_sweeps = int(num_sweeps)
    b0, b1 = float(beta_start), float(beta_end)
    if not (np.isfinite(b0) and np.isfinite(b1)) or b0 < 0.0 or b1 < 0.0:
        raise ValueError(f"beta_start={beta_start!r}, beta_end={beta_end!r}: both must be finite and >= 0")
    if kind == "geometric" and not (b0 > 0.0 and b1 > 0.0):
        raise ValueError(f"a geometric schedule needs both ends > 0, got beta_start={b0}, beta_end={b1}")
    if num_sweeps == 1:
        return np.array([b1], dtype=np.float32)
    pts = np.geomspace(b0, b1, num_sweeps) if kind == "geometric" else np.linspace(b0, b1, num_sweeps)
    out = pts.astype(np.float32)
    out[0], out[-1] = np.float32(b0), np.float32(b1)
    return out


_make_beta_schedule = beta_schedule  # (sample_ising has a keyword of that name)


def logit_fields(logits, beta: float, prefactor: float):
    """The ``fields`` of :meth:`GibbsSampler.sample_fields` that multiply the prior by factorial evidence: with
    ``fields = -logits / (2 * beta * prefactor)`` chain c draws from

        ``p(z) * prod_i sigmoid(logits[c, i])^[z_i = +1] * sigmoid(-logits[c, i])^[z_i = -1]``,  normalised,

    ``p`` being the sampler's distribution without fields -- e.g. a GRBM prior times an encoder's logits for one image per
    chain (``logits`` = the log odds of ``z_i = +1``).  Derivation: the draw samples ``exp(-beta (hs_c . z + z Js z))`` with
    ``hs_c = prefactor * (linear + fields[c])`` where no range clamps, i.e. ``p(z) * exp(-beta * prefactor * fields[c] . z)``.
    The evidence of spin i is ``sigmoid(l z_i)`` with ``l = logits[c, i]``, and ``sigmoid(l) / sigmoid(-l) = e^l`` makes it
    ``exp(l z_i / 2)`` up to a factor that does not depend on ``z_i``.  Matching exponents, ``-beta * prefactor * field =
    l / 2``.  A ``linear_range`` that clamps ``prefactor * (linear + fields)`` caps the evidence with it.

    ``logits``: a tensor (any device; the result stays there, float32) or an array (the result is a float32 array);
    ``beta`` and ``prefactor`` must be finite and nonzero."""
    scale = 2.0 * float(beta) * float(prefactor)
    if not np.isfinite(scale) or scale == 0.0:
        raise ValueError(f"beta={beta!r}, prefactor={prefactor!r}: both must be finite and nonzero")
    if torch.is_tensor(logits):
        return (-logits.detach().to(torch.float32) / scale).contiguous()
    return (-np.asarray(logits, dtype=np.float32) / np.float32(scale)).astype(np.float32)


def _slice_count(slices) -> int:
    """``slices`` as an int, if it is a power of two in 2 .. 64 (the Trotter slices of a :meth:`GibbsSampler.sample_quantum` chain)."""
    if isinstance(slices, bool) or not isinstance(slices, (int, np.integer)) or not 2 <= slices <= 64 or slices & (slices - 1):
        raise ValueError(f"slices must be a power of two in 2 .. 64, got {slices!r}")
    return int(slices)


def transverse_schedule(beta: float, gamma_start: float, gamma_end: float, num_sweeps: int, slices: int,
                        kind: str = "linear") -> Tuple[np.ndarray, np.ndarray]:
    """The two tables of a simulated-quantum-annealing draw (:meth:`GibbsSampler.sample_quantum`, "DVG SQA v1") at inverse
    temperature ``beta`` with ``slices`` = P Trotter slices, the transverse field going from ``gamma_start`` to ``gamma_end``
    over ``num_sweeps`` sweeps, ``kind`` "linear" or "geometric" (``np.linspace`` / ``np.geomspace`` in float64; ``num_sweeps
    == 1`` gives ``gamma_end`` alone).  Returns ``(beta_slice, kappa)``, two (num_sweeps,) float32 arrays: ``beta_slice = beta /
    P`` throughout, ``kappa[k] = -1/2 ln tanh(beta Gamma_k / P)`` computed in float64 and rounded once -- it falls as Gamma
    grows: a strong field decouples the slices, a vanishing one locks them together.  Both fields must be finite and > 0
    and ``beta`` finite and > 0; a field so small that ``kappa`` overflows float32 is an error."""
    if kind not in ("geometric", "linear"):
        raise ValueError(f"transverse schedule kind must be 'geometric' or 'linear', got {kind!r}")
    num_sweeps, P = _whole("num_sweeps", num_sweeps), _slice_count(slices)
    try:
        b, g0, g1 = float(beta), float(gamma_start), float(gamma_end)
    except (TypeError, ValueError):
        raise ValueError(f"beta={beta!r}, gamma_start={gamma_start!r}, gamma_end={gamma_end!r} must be numbers") from None
    if not (np.isfinite(b) and b > 0.0):
        raise ValueError(f"beta={beta!r} must be finite and > 0")
    for name, g in (("gamma_start", g0), ("gamma_end", g1)):
        if not (np.isfinite(g) and g > 0.0):
            raise ValueError(f"{name}={g!r} must be finite and > 0 (kappa = -1/2 ln tanh(beta Gamma / P))")
    gammas = np.array([g1]) if num_sweeps == 1 else (np.geomspace if kind == "geometric" else np.linspace)(g0, g1, num_sweeps)
    if num_sweeps > 1:
        gammas[0], gammas[-1] = g0, g1
    with np.errstate(divide="ignore", over="ignore"):
        kappa = (-0.5 * np.log(np.tanh(b * gammas / P)) + 0.0).astype(np.float32)
        beta_slice = np.full(num_sweeps, b / P, dtype=np.float64).astype(np.float32)
    if not np.isfinite(kappa).all():
        k = int(np.flatnonzero(~np.isfinite(kappa))[0])
        raise ValueError(f"kappa overflows float32 at sweep {k} (Gamma = {gammas[k]!r}): gamma_start={g0!r} / gamma_end={g1!r} "
                         f"is too small for beta / slices = {b / P!r}")
    if not np.isfinite(beta_slice).all():
        raise ValueError(f"beta={beta!r} / slices overflows float32")
    return beta_slice, kappa


def _check_beta_table(betas, what: str, rows: Optional[int] = None, signed: bool = False):
    """The host-side checks of a table of betas, no device work: shape (S,) or (rows, S) with S >= 1; a CUDA tensor must
    be float32 (its values are the caller's business: looking would be a host sync); host values -- a sequence, an
    array, a CPU tensor -- must be finite and >= 0 once rounded to float32 (``signed``, a table of field strengths: finite).
    Returns the float32 host array, or None for a CUDA tensor."""
    on_device = torch.is_tensor(betas) and betas.is_cuda
    if on_device:
        if betas.dtype != torch.float32:
            raise _lib.DvgError(f"{what}: a device table must be float32, got {betas.dtype}")
        host, shape = None, tuple(betas.shape)
    else:
        try:
            host = np.asarray(betas.detach().numpy() if torch.is_tensor(betas) else betas, dtype=np.float64)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"{what}: not a numeric table ({exc})") from None
        with np.errstate(over="ignore"):
            host = host.astype(np.float32)
        shape = host.shape  # (before ascontiguousarray: it makes a scalar one-dimensional)
        host = np.ascontiguousarray(host)
    want = "(sweeps,)" if rows is None else f"(sweeps,) or ({rows}, sweeps)"
    if len(shape) not in (1, 2) or int(np.prod(shape)) == 0 or (len(shape) == 2 and (rows is None or int(shape[0]) != rows)):
        raise _lib.DvgError(f"{what} must be {want} with at least one sweep, got {tuple(shape)}")
    if host is not None and signed and not np.isfinite(host).all():
        raise ValueError(f"{what}: every entry must be finite")
    if host is not None and not signed and not (np.isfinite(host).all() and (host >= 0).all()):
        raise ValueError(f"{what}: every beta must be finite and >= 0")
    return host


_UNCHECKED = object()


def _beta_table(betas, device, what: str, rows: Optional[int] = None, own: bool = False, host=_UNCHECKED) -> torch.Tensor:
    """``betas``, checked (:func:`_check_beta_table`), as a contiguous float32 tensor on ``device``: host values are
    uploaded, a CUDA tensor is used as it is (``own``: copied).  ``host``: what :func:`_check_beta_table` returned, where the
    caller has run it already."""
    if host is _UNCHECKED:
        host = _check_beta_table(betas, what, rows)
    device = torch.device(device)
    if host is None:
        if device.type == "cuda" and device.index is not None and betas.device != device:
            raise _lib.DvgError(f"{what} is on {betas.device}, expected {device}")
        table = betas.detach().contiguous()
        return table.clone() if own and table.data_ptr() == betas.data_ptr() else table
    if device.type != "cuda":
        raise _lib.DvgError(f"{what}: the sampler's device is {device}; the HIP path has no CPU fallback")
    return torch.from_numpy(host).to(device)


class _Record:
    def __init__(self, sample, energy, num_occurrences=None):
        self.sample = sample
        self.energy = energy
        self.num_occurrences = num_occurrences


class SampleSet:
    """The slice of ``dimod.SampleSet`` the hot path touches
    (/root/reference/src/losses.py:59, /root/reference/src/utils/persistent_qpu_sampler.py:90-95):
    ``.record.sample`` (reads x variables, int8), ``.record.energy``, ``.variables``, ``.vartype``.
    ``device_tensor`` keeps the float32 samples on the GPU so ``sampleset_to_tensor``
    needs no host round trip.  ``.record.num_occurrences`` (reads,) int64: all ones for a raw set, the multiplicities of the
    distinct reads for an aggregated one (:meth:`aggregate`)."""

    def __init__(self, samples: np.ndarray, variables: Sequence, energy=None, vartype="SPIN", device_tensor=None,
                 device_energy=None, num_occurrences=None, device_occurrences=None):
        self._samples = samples
        self._energy = energy
        self.variables = list(variables)
        self.vartype = vartype
        self.device_tensor = device_tensor
        self.device_energy = device_energy  # (reads,) float32 on the GPU: the per-read energy, not yet on the host
        self._occurrences = num_occurrences
        self.device_occurrences = device_occurrences  # (reads,) int64 on the GPU, or None

    @property
    def record(self):
        if self._samples is None:  # lazily materialise on the host
            self._samples = self.device_tensor.to(torch.int8).cpu().numpy()
        if self._energy is None and self.device_energy is not None:
            self._energy = self.device_energy.cpu().numpy()
        if self._occurrences is None:
            self._occurrences = self.device_occurrences.cpu().numpy() if self.device_occurrences is not None else \
                np.ones(len(self), dtype=np.int64)
        return _Record(self._samples, self._energy, self._occurrences)

    def __len__(self):
        return int(self.device_tensor.shape[0]) if self.device_tensor is not None else len(self._samples)

    def aggregate(self) -> "SampleSet":
        """``dimod.SampleSet.aggregate()``: a new set of the distinct reads in the order of their first occurrence, each once,
        ``record.num_occurrences`` the sum of the occurrences of its copies and ``record.energy`` the first copy's.  Two reads
        are equal when the same variables are > 0.  A device-held set stays on the device (``pack_spins`` and
        ``dvg_packed_distinct``: one host read, the number of distinct reads); a host-only set takes the same definition in
        numpy."""
        if self.device_tensor is not None:
            from . import functional as F  # (functional imports this module)

            t = self.device_tensor
            d = F.packed_distinct(pack_spins(t), n=int(t.shape[1]))
            rep = d.rep.to(torch.int64)
            occ = d.count
            if self.device_occurrences is not None or self._occurrences is not None:
                had = self.device_occurrences if self.device_occurrences is not None else torch.from_numpy(np.asarray(self._occurrences))
                occ = torch.zeros_like(d.count).index_add_(0, d.id.to(torch.int64), had.to(device=t.device, dtype=torch.int64))
            energy = self.device_energy[rep] if self.device_energy is not None else None
            host_energy = np.asarray(self._energy)[rep.cpu().numpy()] if energy is None and self._energy is not None else None
            return SampleSet(None, self.variables, energy=host_energy, vartype=self.vartype, device_tensor=t[rep],
                             device_energy=energy, device_occurrences=occ)
        rec = self.record
        samples = np.asarray(rec.sample)
        keys = np.packbits(samples > 0, axis=1)
        seen, rep, ident = {}, [], np.empty(len(samples), dtype=np.int64)
        for t in range(len(samples)):
            k = keys[t].tobytes()
            if k not in seen:
                seen[k] = len(rep)
                rep.append(t)
            ident[t] = seen[k]
        occ = np.bincount(ident, weights=None if rec.num_occurrences is None else np.asarray(rec.num_occurrences),
                          minlength=len(rep)).astype(np.int64)
        energy = np.asarray(rec.energy)[rep] if rec.energy is not None else None
        return SampleSet(samples[rep], self.variables, energy=energy, vartype=self.vartype, num_occurrences=occ)

    def _sorted_by_energy(self) -> "SampleSet":
        """The same reads by rising energy, ties in their present order (a stable sort, on the device for a device-held set)."""
        if self.device_tensor is not None and self.device_energy is not None:
            order = torch.sort(self.device_energy, stable=True).indices
            occ = self.device_occurrences[order] if self.device_occurrences is not None else None
            return SampleSet(None, self.variables, vartype=self.vartype, device_tensor=self.device_tensor[order],
                             device_energy=self.device_energy[order], device_occurrences=occ)
        rec = self.record
        order = np.argsort(np.asarray(rec.energy), kind="stable")
        return SampleSet(np.asarray(rec.sample)[order], self.variables, energy=np.asarray(rec.energy)[order], vartype=self.vartype,
                         num_occurrences=np.asarray(rec.num_occurrences)[order])


class LogPartition:
    """What :meth:`GibbsSampler.log_partition` returns.  ``log_z``: float64 device scalar, ``n log 2 + logsumexp(log_weights)
    - log C``; ``ess``: the effective sample size ``(sum w)^2 / sum w^2`` of the C weights; ``std_err``: the standard
    error of ``log_z`` to first order, ``sqrt(1 / ess - 1 / C)`` (the relative standard error of the mean weight);
    ``log_weights`` (C,) float64 and ``samples`` (C, n) float32: the chains."""

    def __init__(self, log_z, ess, std_err, log_weights, samples):
        self.log_z, self.ess, self.std_err, self.log_weights, self.samples = log_z, ess, std_err, log_weights, samples

    @classmethod
    def from_weights(cls, n: int, log_weights: torch.Tensor, samples=None, log_z_from: float = None) -> "LogPartition":
        C = int(log_weights.shape[0])
        lse = torch.logsumexp(log_weights, 0)
        base = n * float(np.log(2.0)) if log_z_from is None else float(log_z_from)
        ess = torch.exp(2.0 * lse - torch.logsumexp(2.0 * log_weights, 0))
        std_err = torch.sqrt(torch.clamp(1.0 / ess - 1.0 / C, min=0.0))
        return cls(lse + (base - float(np.log(C))), ess, std_err, log_weights, samples)

    def __repr__(self):
        return f"LogPartition(log_z={float(self.log_z):.6f}, ess={float(self.ess):.1f}, std_err={float(self.std_err):.4f})"


class LogEvidence:
    """What :meth:`GibbsSampler.log_evidence` returns, per row of ``fields``.  ``log_ratio`` (rows,) float64 on the device:
    ``logsumexp(log_weights[r]) - log chains_per_row``, the estimate of ``log(Z_r / Z)``, ``Z_r`` the normaliser of the model
    with row r added to its linear terms; ``ess``, ``std_err`` (rows,): the effective sample size ``(sum w)^2 / sum w^2`` of a
    row's weights and the standard error of its ``log_ratio`` to first order, ``sqrt(1 / ess - 1 / chains_per_row)``, as
    :class:`LogPartition` has them; ``log_weights`` (rows, chains_per_row) float64; ``samples`` (rows * chains_per_row, n)
    float32: the chains, annealed draws of each row's posterior (row r: chains ``r * chains_per_row ...``)."""

    def __init__(self, log_ratio, ess, std_err, log_weights, samples):
        self.log_ratio, self.ess, self.std_err, self.log_weights, self.samples = log_ratio, ess, std_err, log_weights, samples

    @classmethod
    def from_weights(cls, log_weights: torch.Tensor, samples=None) -> "LogEvidence":
        """``log_weights``: (rows, chains_per_row) float64."""
        K = int(log_weights.shape[1])
        lse = torch.logsumexp(log_weights, 1)
        ess = torch.exp(2.0 * lse - torch.logsumexp(2.0 * log_weights, 1))
        std_err = torch.sqrt(torch.clamp(1.0 / ess - 1.0 / K, min=0.0))
        return cls(lse - float(np.log(K)), ess, std_err, log_weights, samples)

    def __repr__(self):
        return (f"LogEvidence(rows={int(self.log_ratio.shape[0])}, chains_per_row={int(self.log_weights.shape[1])}, "
                f"mean log_ratio={float(self.log_ratio.mean()):.6f}, min ess={float(self.ess.min()):.1f})")


class Tempered:
    """What :meth:`GibbsSampler.sample_tempered` returns, for Q ladders of R rungs; device tensors unless said otherwise.
    ``samples`` (Q, R, n) float32 +-1 and ``energies`` (Q, R) float64, BY RUNG: ``[q, r]`` is the chain of ladder q that ended
    the draw on rung r -- a sample at ``betas[r]``; ``target`` = ``samples[:, -1]``, the last rung's.  ``accepted`` (Q, R - 1)
    int64: the accepted exchanges of each pair of neighbouring rungs; ``attempts`` (R - 1,) host int64: the exchanges of the
    draw that had the pair (computed from the sweep range); ``acceptance_rate`` (R - 1,) float64: accepted over all ladders /
    (Q attempts), NaN for a pair the draw never tried.  ``state`` (Q R, n) int8 and ``rungs`` (Q R,) int32, BY CHAIN: hand them
    back as ``start`` / ``rungs`` to continue the draw."""

    def __init__(self, samples, energies, accepted, attempts, state, rungs):
        self.samples, self.energies, self.accepted, self.attempts, self.state, self.rungs = (samples, energies, accepted,
                                                                                             attempts, state, rungs)

    @classmethod
    def from_draw(cls, n: int, R: int, out, energy, accept, sweep0: int, n_sweeps: int, swap_every: int, state, rungs) -> "Tempered":
        Q = int(out.shape[0]) // R
        x = np.arange(sweep0 + 1, sweep0 + n_sweeps + 1, dtype=np.int64)
        x = x[x % swap_every == 0] // swap_every  # the numbers of the draw's exchanges; number x has the pairs r = x & 1, ...
        attempts = np.array([int(((x & 1) == (r & 1)).sum()) for r in range(R - 1)], dtype=np.int64)
        return cls(out.view(Q, R, n), energy.view(Q, R), accept.view(Q, R)[:, :R - 1].to(torch.int64), attempts, state, rungs)

    @property
    def target(self):
        return self.samples[:, -1]

    @property
    def acceptance_rate(self):
        tried = torch.from_numpy(self.attempts.astype(np.float64)).to(self.accepted.device) * int(self.accepted.shape[0])
        return self.accepted.sum(0).to(torch.float64) / tried

    def __repr__(self):
        Q, R, n = self.samples.shape
        return f"Tempered({Q} ladders x {R} rungs, n={n}, attempts={self.attempts.tolist()})"


class ClusterMoves:
    """What :meth:`GibbsSampler.cluster_move` returns, for P twin pairs of R rungs ("DVG ICM v1"); device tensors.  ``sizes``
    (P, R) int64: the spins each pair exchanged at each rung, 0 where nothing moved (rungs below ``rung_from``, identical
    twins); ``differ`` (P, R) int64: the sites where the pair's two holders of the rung disagreed.  ``moved_share`` (R,)
    float64: exchanged sites over disagreeing sites, summed over the pairs -- 1 where every cluster is the whole of D, the move
    then only renames the twins; ``mean_size`` (R,) float64: the mean cluster over the pairs that disagreed anywhere.  Both
    NaN for a rung without a disagreeing pair."""

    def __init__(self, sizes, differ):
        self.sizes, self.differ = sizes, differ

    @classmethod
    def from_outputs(cls, sizes: torch.Tensor, differ: torch.Tensor, R: int) -> "ClusterMoves":
        return cls(sizes.view(-1, R).to(torch.int64), differ.view(-1, R).to(torch.int64))

    @property
    def moved_share(self):
        return self.sizes.sum(0).to(torch.float64) / self.differ.sum(0).to(torch.float64)

    @property
    def mean_size(self):
        return self.sizes.sum(0).to(torch.float64) / (self.differ > 0).sum(0).to(torch.float64)

    def __repr__(self):
        P, R = self.sizes.shape
        return f"ClusterMoves({P} twin pairs x {R} rungs)"


def cluster_schedule(sweep0: int, num_sweeps: int, cluster_every: int, fresh: bool):
    """The segments of a :meth:`GibbsSampler.sample_tempered_cluster` call of ``num_sweeps`` sweeps from global sweep
    ``sweep0``: a list of ``(move, first_sweep, sweeps)`` -- ``move``: the index t / cluster_every of the cluster move in front
    of the segment's first sweep t (t % cluster_every == 0), or None for a first segment without one: ``sweep0`` is no
    multiple of ``cluster_every``, or the chains are ``fresh``.  Every segment is one exchange draw of ``sweeps`` >= 1."""
    cuts = [t for t in range(sweep0, sweep0 + num_sweeps) if t % cluster_every == 0 and not (fresh and t == sweep0)]
    firsts = ([] if cuts and cuts[0] == sweep0 else [sweep0]) + cuts
    ends = firsts[1:] + [sweep0 + num_sweeps]
    return [(t // cluster_every if t in cuts else None, t, e - t) for t, e in zip(firsts, ends)]


class TemperedCluster:
    """What :meth:`GibbsSampler.sample_tempered_cluster` returns.  ``tempered``: the :class:`Tempered` of the call's last
    sweeps (samples, energies, state and rungs after them; ``accepted`` and ``attempts`` summed over the call); ``sizes`` and
    ``differ`` (moves, pairs, R) int64 device tensors: per cluster move of the call what :class:`ClusterMoves` holds;
    ``moves`` (moves,) host int64: their indices t / cluster_every."""

    def __init__(self, tempered, sizes, differ, moves):
        self.tempered, self.sizes, self.differ, self.moves = tempered, sizes, differ, moves

    def __repr__(self):
        return f"TemperedCluster({self.tempered!r}, moves={self.moves.tolist()})"


class Population:
    """What :meth:`GibbsSampler.sample_population` returns, for P populations of R chains annealed over T temperature steps;
    tensors live where the draw's do.  ``samples`` (C, n) float32 +-1 and ``state`` (C, n) int8: the final population,
    equally weighted samples at the last beta.  ``log_z_populations`` (P,) float64: each population's estimate, ``n log 2 +
    sum_t (logsumexp_c log_weights[t] - log R)``; ``log_z``: ``logsumexp_p - log P``, the estimate of the mean of the
    ``Z_p``; ``std_err``: the relative standard error of that mean, ``std(Z_p, ddof=1) / mean(Z_p) / sqrt(P)``, NaN for P = 1.
    ``families`` (C,) int32: the index of the founder -- the chain at the start -- each final chain descends from;
    ``survivors`` (P,) int64: the distinct families of each population; ``rho_t`` (P,) float64: ``R sum_f (n_f / R)^2`` over
    its families' sizes n_f -- ``R / rho_t`` independent samples remain.  ``ess`` (T, P) float64: the effective sample size
    ``(sum w)^2 / sum w^2`` of each step's weights, which says where the schedule is too coarse.  ``log_weights`` (T, C)
    float64 and ``parents`` (T, C) int32: each step's weights and resampling, kept with ``history=True``, else None."""

    def __init__(self, samples, state, log_z_populations, log_z, std_err, families, survivors, rho_t, ess, log_weights=None,
                 parents=None):
        self.samples, self.state, self.log_z_populations, self.log_z, self.std_err = samples, state, log_z_populations, log_z, std_err
        self.families, self.survivors, self.rho_t, self.ess, self.log_weights, self.parents = (families, survivors, rho_t, ess,
                                                                                              log_weights, parents)

    @staticmethod
    def step_estimates(log_weights: torch.Tensor, P: int):
        """(log mean weight, ess) per step and population, both (T, P), from (T, C) float64 log weights: plain torch ops."""
        lw = log_weights.view(log_weights.shape[0], P, -1)
        lse = torch.logsumexp(lw, 2)
        return lse - float(np.log(lw.shape[2])), torch.exp(2.0 * lse - torch.logsumexp(2.0 * lw, 2))

    @classmethod
    def from_estimates(cls, log_z_populations, families, ess, samples=None, state=None, log_weights=None, parents=None) -> "Population":
        P = int(log_z_populations.shape[0])
        R = int(families.shape[0]) // P
        log_z = torch.logsumexp(log_z_populations, 0) - float(np.log(P))
        z = torch.exp(log_z_populations - log_z_populations.max())
        std_err = z.std(unbiased=True) / z.mean() / float(np.sqrt(P)) if P > 1 else torch.full_like(log_z, float("nan"))
        # a family's founder lies in its own population, p R .. p R + R - 1: its index there is the remainder
        local = torch.remainder(families.view(P, R).to(torch.int64), R)
        sizes = torch.zeros((P, R), dtype=torch.int64, device=families.device).scatter_add_(1, local, torch.ones_like(local))
        survivors = (sizes > 0).sum(1)
        rho_t = (sizes * sizes).sum(1).to(torch.float64) / float(R)
        return cls(samples, state, log_z_populations, log_z, std_err, families, survivors, rho_t, ess, log_weights, parents)

    @classmethod
    def from_history(cls, n: int, log_weights: torch.Tensor, families: torch.Tensor, populations: int = 1, samples=None,
                     state=None, parents=None) -> "Population":
        """The estimates from plain tensors (CPU ones too): ``log_weights`` (T, C) float64, every step's; ``families`` (C,)
        integer founder indices of the final chains; ``populations`` P dividing C."""
        if log_weights.dim() != 2 or log_weights.dtype != torch.float64 or min(log_weights.shape) < 1:
            raise ValueError(f"log_weights must be (steps >= 1, chains >= 1) float64, got {tuple(log_weights.shape)} {log_weights.dtype}")
        T, C = (int(v) for v in log_weights.shape)
        P = int(populations)
        if P < 1 or C % P or tuple(families.shape) != (C,):
            raise ValueError(f"populations={populations!r} must divide the {C} chains, and families be ({C},), got {tuple(families.shape)}")
        inc, ess = cls.step_estimates(log_weights, P)
        return cls.from_estimates(n * float(np.log(2.0)) + inc.sum(0), families, ess, samples, state, log_weights, parents)

    def __repr__(self):
        return (f"Population({int(self.log_z_populations.shape[0])} x {int(self.families.shape[0]) // int(self.log_z_populations.shape[0])} "
                f"chains, {int(self.ess.shape[0])} steps, log_z={float(self.log_z):.6f}, std_err={float(self.std_err):.4f})")


def pack_spins(x: torch.Tensor) -> torch.Tensor:
    """(..., n) spins (+1 where the entry is > 0) -> (..., W = ceil(n / 32)) int32 in the layout of "DVG trace v1"
    (include/dvg.h): bit b of word w is 1 iff spin 32 w + b is +1, bits of spins >= n are 0.  Plain torch operations, on
    the tensor's device (CPU tensors too)."""
    n = int(x.shape[-1])
    W = (n + 31) // 32
    up = (x > 0).to(torch.int64)
    up = torch.nn.functional.pad(up, (0, 32 * W - n)).reshape(*x.shape[:-1], W, 32)
    words = (up << torch.arange(32, dtype=torch.int64, device=x.device)).sum(-1)  # 0 .. 2^32 - 1
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def unpack_spins(bits: torch.Tensor, n: int) -> torch.Tensor:
    """The inverse of :func:`pack_spins`: (..., W) int32 -> (..., n) float32 +-1.  Bits of spins >= n are ignored."""
    W = int(bits.shape[-1])
    if W != (int(n) + 31) // 32:
        raise ValueError(f"{W} words per row do not hold {n} spins")
    b = (bits.to(torch.int64).unsqueeze(-1) >> torch.arange(32, dtype=torch.int64, device=bits.device)) & 1
    return (2 * b.reshape(*bits.shape[:-1], 32 * W)[..., :int(n)] - 1).to(torch.float32)


class Moments:
    """Exact first and second moments of +-1 rows: ``spin_sum`` (n,) int64 = sum over rows of s_i, ``pair_sum`` (E,) int64 =
    sum over rows of s_i s_j per edge of the graph, ``count`` the number of rows; ``mean_spin`` / ``mean_pair``: the sums
    over ``count``, float64.  What :meth:`Trace.moments` returns (``dvg_grbm_moments_packed``)."""

    def __init__(self, spin_sum, pair_sum, count):
        self.spin_sum, self.pair_sum, self.count = spin_sum, pair_sum, int(count)

    @classmethod
    def from_sums(cls, spin_sum: torch.Tensor, pair_sum: torch.Tensor, count: int) -> "Moments":
        if isinstance(count, bool) or int(count) != count or int(count) < 1:
            raise ValueError(f"count must be an integer >= 1, got {count!r}")
        for name, t in (("spin_sum", spin_sum), ("pair_sum", pair_sum)):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1:
                raise ValueError(f"{name} must be a one-dimensional int64 tensor")
        return cls(spin_sum, pair_sum, count)

    @property
    def mean_spin(self):
        return self.spin_sum.to(torch.float64) / self.count

    @property
    def mean_pair(self):
        return self.pair_sum.to(torch.float64) / self.count

    def __repr__(self):
        return f"Moments(n={int(self.spin_sum.shape[0])}, edges={int(self.pair_sum.shape[0])}, count={self.count})"


class Autocorrelation:
    """Autocorrelation estimates from the exact sums of a trace of C chains x M records (``dvg_trace_autocorr``, "DVG acf v1"):
    ``lag_sum`` (L + 1, n) int64 = sum over chains and over the M - t pairs of lag t of s_i(m) s_i(m + t), ``spin_sum`` (n,)
    int64 = sum over chains and records of s_i, ``chain_sum`` (C, n) int32 = the same per chain, or None; ``thin`` the sweeps
    between two records.  Every property is float64 torch on the sums' device (CPU tensors too), no host sync:

    ``counts`` (L + 1,) host int64: C (M - t) pairs;  ``mean_spin`` (n,): the pooled mean mu;
    ``rho`` (L + 1, n): (lag_sum / counts - mu^2) / (1 - mu^2) -- around the POOLED mean, so chains stuck in different modes
    show as slow; NaN for a spin with mu^2 = 1;
    ``tau_int`` (n,), in records: 1 + 2 sum_{t = 1}^{T} rho[t], T the number of leading lags 1, 2, .. with rho > 0 (the initial
    positive sequence), at most L; ``truncated`` (n,) bool: rho > 0 at every lag 1 .. L (L >= 1) -- the window hit max_lag
    and tau_int is a lower bound; ``tau_int_sweeps`` = tau_int * thin; ``ess`` = C M / tau_int;
    ``overlap`` (L + 1,): lag_sum.sum(1) / (n counts), the spin-overlap autocorrelation q(t);
    ``r_hat`` (n,): Gelman-Rubin over the chains' means (needs ``chain_sum``, C >= 2, M >= 2)."""

    def __init__(self, lag_sum, spin_sum, chain_sum, chains, records, thin=1):
        self.lag_sum, self.spin_sum, self.chain_sum = lag_sum, spin_sum, chain_sum
        self.chains, self.records, self.thin = int(chains), int(records), int(thin)

    @classmethod
    def from_sums(cls, lag_sum: torch.Tensor, spin_sum: torch.Tensor, chain_sum: Optional[torch.Tensor], chains: int,
                  records: int, thin: int = 1) -> "Autocorrelation":
        for name, v in (("chains", chains), ("records", records), ("thin", thin)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        if not torch.is_tensor(lag_sum) or lag_sum.dtype != torch.int64 or lag_sum.dim() != 2 or lag_sum.shape[0] < 1:
            raise ValueError("lag_sum must be a (max_lag + 1, n) int64 tensor")
        n = int(lag_sum.shape[1])
        if int(lag_sum.shape[0]) > int(records):
            raise ValueError(f"lag_sum holds lags 0 .. {int(lag_sum.shape[0]) - 1}, but {int(records)} records have lags below {int(records)}")
        if not torch.is_tensor(spin_sum) or spin_sum.dtype != torch.int64 or tuple(spin_sum.shape) != (n,):
            raise ValueError(f"spin_sum must be a ({n},) int64 tensor")
        if chain_sum is not None and (not torch.is_tensor(chain_sum) or chain_sum.dtype != torch.int32 or
                                      tuple(chain_sum.shape) != (int(chains), n)):
            raise ValueError(f"chain_sum must be a ({int(chains)}, {n}) int32 tensor or None")
        return cls(lag_sum, spin_sum, chain_sum, chains, records, thin)

    @property
    def max_lag(self) -> int:
        return int(self.lag_sum.shape[0]) - 1

    @property
    def counts(self) -> np.ndarray:
        return self.chains * (self.records - np.arange(self.max_lag + 1, dtype=np.int64))

    def _counts(self):
        return torch.from_numpy(self.counts).to(device=self.lag_sum.device, dtype=torch.float64)

    @property
    def mean_spin(self):
        return self.spin_sum.to(torch.float64) / (self.chains * self.records)

    @property
    def rho(self):
        mu2 = self.mean_spin ** 2
        return (self.lag_sum.to(torch.float64) / self._counts()[:, None] - mu2) / (1.0 - mu2)

    @property
    def tau_int(self):
        rho = self.rho
        window = torch.cumprod((rho[1:] > 0).to(torch.float64), dim=0)  # 1 over the initial positive sequence, 0 behind it
        tau = 1.0 + 2.0 * torch.where(window > 0, rho[1:], torch.zeros_like(rho[1:])).sum(0)
        return torch.where(torch.isnan(rho[0]), rho[0], tau)  # (a frozen spin: rho is NaN at every lag, lag 0 included)

    @property
    def truncated(self):
        rho = self.rho[1:]
        if rho.shape[0] == 0:
            return torch.zeros(rho.shape[1], dtype=torch.bool, device=rho.device)
        return (rho > 0).all(0)

    @property
    def tau_int_sweeps(self):
        return self.tau_int * self.thin

    @property
    def ess(self):
        return (self.chains * self.records) / self.tau_int

    @property
    def overlap(self):
        return self.lag_sum.sum(1).to(torch.float64) / (self.lag_sum.shape[1] * self._counts())

    @property
    def r_hat(self):
        C, M = self.chains, self.records
        if self.chain_sum is None or C < 2 or M < 2:
            raise ValueError(f"r_hat needs the chains' sums, at least 2 chains and at least 2 records (chain_sum "
                             f"{'missing' if self.chain_sum is None else 'given'}, {C} chains, {M} records)")
        m_c = self.chain_sum.to(torch.float64) / M
        Wv = (1.0 - m_c ** 2).mean(0) * (M / (M - 1.0))
        Bm = m_c.var(0, unbiased=True)
        return torch.sqrt(((M - 1.0) / M * Wv + Bm) / Wv)

    def __repr__(self):
        return (f"Autocorrelation({self.chains} chains x {self.records} records, n={int(self.lag_sum.shape[1])}, "
                f"max_lag={self.max_lag}, thin={self.thin})")


class EnergySeries:
    """Mixing statistics of the energies of C chains x M records (``dvg_grbm_energy_packed``, "DVG energy v1"; :meth:`Trace.energy`):
    ``energies`` (C, M) float64, ``thin`` the sweeps between two records, ``max_lag`` = L.  Every property is float64 torch on
    the energies' device (CPU tensors too), no host sync; d(c, m) = E(c, m) - mean:

    ``mean``: the pooled mean;  ``var``: the pooled variance, dividing by C M;  ``chain_mean`` (C,);
    ``rho`` (L + 1,): rho[t] = [sum_c sum_{m < M - t} d(c, m) d(c, m + t) / (C (M - t))] / var -- around the POOLED mean, so chains
    stuck in different basins show as slow; NaN when var = 0;
    ``tau_int``, in records: 1 + 2 sum_{t = 1}^{T} rho[t], T the number of leading lags 1, 2, .. with rho > 0 (the initial
    positive sequence), at most L; ``truncated``: rho > 0 at every lag 1 .. L (L >= 1) -- the window hit max_lag and tau_int
    is a lower bound; ``tau_int_sweeps`` = tau_int * thin; ``ess`` = C M / tau_int;
    ``r_hat``: Gelman-Rubin, sqrt(((M - 1) / M W + B) / W) with W the mean within-chain variance (ddof = 1) and B the variance
    of the chain means (ddof = 1) -- :attr:`Autocorrelation.r_hat`'s formula; needs C >= 2 and M >= 2;
    ``heat_capacity(beta)`` = beta^2 var;  ``std_err``: the between-chain standard deviation of ``chain_mean`` over sqrt(C), the
    standard error of ``mean`` whatever the autocorrelation within a chain; NaN at C = 1."""

    def __init__(self, energies, thin, max_lag):
        self.energies, self.thin, self.max_lag = energies, int(thin), int(max_lag)
        self.chains, self.records = int(energies.shape[0]), int(energies.shape[1])

    @classmethod
    def from_energies(cls, energies: torch.Tensor, thin: int = 1, max_lag: Optional[int] = None) -> "EnergySeries":
        if not torch.is_tensor(energies) or energies.dtype != torch.float64 or energies.dim() != 2 or min(energies.shape) < 1:
            raise ValueError(f"energies must be a (chains >= 1, records >= 1) float64 tensor, got "
                             f"{(tuple(energies.shape), energies.dtype) if torch.is_tensor(energies) else type(energies).__name__}")
        if isinstance(thin, bool) or not isinstance(thin, (int, np.integer)) or thin < 1:
            raise ValueError(f"thin must be an integer >= 1, got {thin!r}")
        M = int(energies.shape[1])
        if max_lag is None:
            max_lag = min(M - 1, 512)
        if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 0 <= max_lag < M:
            raise ValueError(f"max_lag must be an integer in 0 .. {M - 1} (records - 1), got {max_lag!r}")
        return cls(energies, thin, max_lag)

    @property
    def mean(self):
        return self.energies.mean()

    def _d(self):
        return self.energies - self.mean

    @property
    def var(self):
        return (self._d() ** 2).mean()

    @property
    def chain_mean(self):
        return self.energies.mean(1)

    @property
    def rho(self):
        d, C, M = self._d(), self.chains, self.records
        cov = torch.stack([(d[:, :M - t] * d[:, t:]).sum() / (C * (M - t)) for t in range(self.max_lag + 1)])
        return cov / self.var  # (var = 0: 0 / 0 = NaN at every lag)

    @property
    def tau_int(self):
        rho = self.rho
        window = torch.cumprod((rho[1:] > 0).to(torch.float64), dim=0)  # 1 over the initial positive sequence, 0 behind it
        tau = 1.0 + 2.0 * torch.where(window > 0, rho[1:], torch.zeros_like(rho[1:])).sum()
        return torch.where(torch.isnan(rho[0]), rho[0], tau)

    @property
    def truncated(self):
        rho = self.rho[1:]
        if rho.shape[0] == 0:
            return torch.zeros((), dtype=torch.bool, device=rho.device)
        return (rho > 0).all()

    @property
    def tau_int_sweeps(self):
        return self.tau_int * self.thin

    @property
    def ess(self):
        return (self.chains * self.records) / self.tau_int

    @property
    def r_hat(self):
        C, M = self.chains, self.records
        if C < 2 or M < 2:
            raise ValueError(f"r_hat needs at least 2 chains and at least 2 records ({C} chains, {M} records)")
        Wv = self.energies.var(1, unbiased=True).mean()
        Bm = self.chain_mean.var(0, unbiased=True)
        return torch.sqrt(((M - 1.0) / M * Wv + Bm) / Wv)

    def heat_capacity(self, beta: float):
        return float(beta) ** 2 * self.var

    @property
    def std_err(self):
        if self.chains < 2:
            return torch.full_like(self.mean, float("nan"))
        return self.chain_mean.std(0, unbiased=True) / float(np.sqrt(self.chains))

    def __repr__(self):
        return f"EnergySeries({self.chains} chains x {self.records} records, max_lag={self.max_lag}, thin={self.thin})"


class Overlap:
    """The distribution of the spin overlap q = (1 / n) sum_i s_i^a s_i^b = 1 - 2 d / n over pairs of +-1 rows, from the exact
    histogram of their Hamming distances d (``dvg_packed_overlap``, "DVG overlap v1"): ``hist`` (n + 1,) int64, ``hist[d]``
    pairs at distance d.  Every property is float64 torch on the histogram's device (CPU tensors too), no host sync:

    ``pairs`` (): the number of pairs;  ``q`` (n + 1,): the grid 1 - 2 d / n;  ``density`` (n + 1,): hist / pairs, P(q);
    ``mean_q``, ``mean_abs_q``, ``q2``, ``q4``: the means of q, |q|, q^2, q^4;  ``binder`` = (3 - q4 / q2^2) / 2: 1 for a
    distribution on +-q0 (one mode and its mirror), 0 for a Gaussian round 0;  ``hamming_mean``: the mean of d;
    ``mass(lo, hi)``: the share of pairs with lo <= |q| <= hi.  No pairs at all give NaN, as IEEE division does."""

    def __init__(self, hist, n):
        self.hist, self.n = hist, int(n)

    @classmethod
    def from_hist(cls, hist: torch.Tensor, n: int) -> "Overlap":
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"n must be an integer >= 1, got {n!r}")
        if not torch.is_tensor(hist) or hist.dtype != torch.int64 or tuple(hist.shape) != (int(n) + 1,):
            raise ValueError(f"hist must be a ({int(n) + 1},) int64 tensor")
        return cls(hist, n)

    def _h(self):
        return self.hist.to(torch.float64)

    def _mean(self, f):
        return (self._h() * f).sum() / self.pairs

    @property
    def pairs(self):
        return self._h().sum()

    @property
    def q(self):
        return 1.0 - 2.0 * torch.arange(self.n + 1, dtype=torch.float64, device=self.hist.device) / self.n

    @property
    def density(self):
        return self._h() / self.pairs

    @property
    def mean_q(self):
        return self._mean(self.q)

    @property
    def mean_abs_q(self):
        return self._mean(self.q.abs())

    @property
    def q2(self):
        return self._mean(self.q ** 2)

    @property
    def q4(self):
        return self._mean(self.q ** 4)

    @property
    def binder(self):
        return (3.0 - self.q4 / self.q2 ** 2) / 2.0

    @property
    def hamming_mean(self):
        return self._mean(torch.arange(self.n + 1, dtype=torch.float64, device=self.hist.device))

    def mass(self, lo: float, hi: float):
        aq = self.q.abs()
        return self._mean(((aq >= lo) & (aq <= hi)).to(torch.float64))

    def __repr__(self):
        return f"Overlap(n={self.n})"


class LinkOverlap:
    """The link overlap q_l = (1 / E) sum_e t_e^a t_e^b = 1 - 2 l / E of pairs of +-1 rows -- t_e = s_i s_j the bonds on the
    graph's E edges -- beside their spin overlap q = 1 - 2 d / n, from the exact sums of ``dvg_packed_overlap_link`` ("DVG link
    overlap v1"): ``hist`` (n + 1,), pairs per spin distance d; ``link_hist`` (E + 1,), pairs per bond distance l; ``link_sum``
    and ``link_sq`` (n + 1,), per d the sums of l and l^2; all int64.  Flipping a compact domain moves q a lot and q_l little
    (only the domain's surface changes bonds), so q_l against q^2 tells droplets from rows that differ everywhere.  Every
    property is float64 torch on the sums' device (CPU tensors too), no host sync:

    ``pairs`` ();  ``spin``: the :class:`Overlap` of ``hist``;  ``link``: the :class:`Overlap` of ``link_hist`` over E -- P(q_l),
    ``mean_q``, ``q2``, ``binder`` of the link overlap;  ``q`` (n + 1,): the grid 1 - 2 d / n;
    ``link_given_q`` (n + 1,): the mean of q_l over the pairs at each d, ``1 - 2 link_sum / (E hist)``, NaN in empty bins;
    ``link_var_given_q`` (n + 1,): the variance of q_l over the pairs at each d, NaN in empty bins;
    ``mean_link``: the mean of q_l over all pairs;  ``corr_q2_link``: the Pearson correlation of q^2 and q_l over the pairs;
    ``fit()``: ``(a, b)`` of the least-squares line q_l = a + b q^2 over the pairs (the ``hist``-weighted fit of
    ``link_given_q``).  No pairs at all give NaN, as IEEE division does."""

    def __init__(self, hist, link_hist, link_sum, link_sq, n, n_edges):
        self.hist, self.link_hist, self.link_sum, self.link_sq = hist, link_hist, link_sum, link_sq
        self.n, self.n_edges = int(n), int(n_edges)

    @classmethod
    def from_sums(cls, hist, link_hist, link_sum, link_sq, n: int, n_edges: int) -> "LinkOverlap":
        for name, v in (("n", n), ("n_edges", n_edges)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        for name, t, k in (("hist", hist, n), ("link_hist", link_hist, n_edges), ("link_sum", link_sum, n), ("link_sq", link_sq, n)):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != (int(k) + 1,):
                raise ValueError(f"{name} must be a ({int(k) + 1},) int64 tensor")
            if t.device != hist.device:
                raise ValueError(f"{name} must be on the device of hist ({hist.device}), got {t.device}")
        return cls(hist, link_hist, link_sum, link_sq, n, n_edges)

    @property
    def spin(self) -> Overlap:
        return Overlap(self.hist, self.n)

    @property
    def link(self) -> Overlap:
        return Overlap(self.link_hist, self.n_edges)

    @property
    def pairs(self):
        return self.hist.to(torch.float64).sum()

    @property
    def q(self):
        return self.spin.q

    def _per_bin(self):
        """(hist, sum of q_l, sum of q_l^2) over the pairs at each d, float64."""
        h, s, sq, E = self.hist.to(torch.float64), self.link_sum.to(torch.float64), self.link_sq.to(torch.float64), float(self.n_edges)
        return h, h - 2.0 * s / E, h - 4.0 * s / E + 4.0 * sq / (E * E)

    @property
    def link_given_q(self):
        return 1.0 - 2.0 * self.link_sum.to(torch.float64) / (float(self.n_edges) * self.hist.to(torch.float64))

    @property
    def link_var_given_q(self):
        h, s1, s2 = self._per_bin()
        return s2 / h - (s1 / h) ** 2

    @property
    def mean_link(self):
        return 1.0 - 2.0 * self.link_sum.to(torch.float64).sum() / (float(self.n_edges) * self.pairs)

    def _moments(self):
        """(mean of q^2, mean of q_l, var of q^2, var of q_l, their covariance) over the pairs, each sum centred."""
        h, s1, _s2 = self._per_bin()
        P, x = self.pairs, self.q ** 2
        mx, my = (h * x).sum() / P, self.mean_link
        link = self.link
        var_x = (h * (x - mx) ** 2).sum() / P
        var_y = (link._h() * (link.q - my) ** 2).sum() / P
        cov = ((x - mx) * (s1 - my * h)).sum() / P
        return mx, my, var_x, var_y, cov

    @property
    def corr_q2_link(self):
        _mx, _my, var_x, var_y, cov = self._moments()
        return cov / torch.sqrt(var_x * var_y)

    def fit(self):
        mx, my, var_x, _var_y, cov = self._moments()
        b = cov / var_x
        return my - b * mx, b

    def __repr__(self):
        return f"LinkOverlap(n={self.n}, n_edges={self.n_edges})"


def bonds(bits, graph, quadratic=None) -> torch.Tensor:
    """The bond rows of bit-packed rows ((rows, W) or (C, M, W) int32 on the device, views welcome): bit e set iff s_i s_j = +1
    on edge e of ``graph`` (a :class:`GraphHandle`), or with the model's ``quadratic`` iff the bond is satisfied
    (``dvg_packed_bonds``, "DVG bonds v1").  The result is packed rows of E "spins": :func:`distinct` on it counts states
    modulo a global flip, ``functional.packed_correlation`` gives edge-edge correlations."""
    from . import functional as F  # (functional imports this module)

    return F.packed_bonds(bits, graph, quadratic)


def link_overlap(bits, graph, other=None) -> LinkOverlap:
    """The :class:`LinkOverlap` of bit-packed rows ((rows, W), or (C, M, W): M groups of C rows) with themselves (the pairs r
    < r' of each group) or with ``other`` (rows as ``functional.packed_overlap``'s ``b``): product-mode bonds of both sides
    (``dvg_packed_bonds``), then one call of ``dvg_packed_overlap_link``; the rows stay packed."""
    from . import functional as F  # (functional imports this module)

    n, E = int(graph.plan.n), int(graph.plan.n_edges)
    a_bonds = F.packed_bonds(bits, graph)
    b_bonds = F.packed_bonds(other, graph) if other is not None else None
    return LinkOverlap.from_sums(*F.packed_link_overlap(bits, a_bonds, other, b_bonds, n=n, n_edges=E), n, E)


class Correlations:
    """Full pair correlations of +-1 rows from their exact sums (``dvg_packed_correlation``, "DVG corr v1"): ``spin_sum`` (n,)
    int64 = sum over rows of s_i, ``pair_sum`` (n, n) int64 = sum over rows of s_i s_j for EVERY pair of spins, ``count`` = T
    the number of rows.  Every member is float64 torch on the sums' device (CPU tensors too), no host sync.  With m =
    spin_sum / T and P = pair_sum / T:

    ``mean_spin`` (n,): m;  ``mean_pair`` (n, n): P;  ``connected`` (n, n): C = P - m m^T;
    ``pearson`` (n, n): C_ij / sqrt(C_ii C_jj), NaN where a spin is frozen (C_ii = 0);
    ``chi_sg`` (): (1 / n) sum_ij C_ij^2, the diagonal included -- the spin-glass susceptibility;
    ``on_edges(graph)`` (E,): C at the plan's (edge_i, edge_j), shaped like ``quadratic``;
    ``off_edge_share(graph)`` (): sum of C_ij^2 over the pairs i < j that are NOT edges / the same over all i < j -- the share
    of the correlation the graph has no coupling for; NaN if the denominator is 0;
    ``top_pairs(k, graph=None)``: ``(i, j, value)``, the k pairs i < j of largest |C_ij| (fewer if there are fewer), edges
    excluded when a graph is given, ``value`` = C_ij; ties go to the smaller flat index i n + j;
    ``gap(other, graph=None)``: a dict against another :class:`Correlations` -- ``spin_rms`` the root mean square of m - m',
    ``pair_rms`` that of P - P' over i < j, and with a graph ``edge_rms`` / ``off_edge_rms`` the same over the edges / over
    the pairs i < j that are not edges (NaN over no pairs).
    ``graph``: a :class:`GraphHandle`, or its plan."""

    def __init__(self, spin_sum, pair_sum, count):
        self.spin_sum, self.pair_sum, self.count = spin_sum, pair_sum, int(count)

    @classmethod
    def from_sums(cls, spin_sum: torch.Tensor, pair_sum: torch.Tensor, count: int) -> "Correlations":
        if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or int(count) < 1:
            raise ValueError(f"count must be an integer >= 1, got {count!r}")
        if not torch.is_tensor(spin_sum) or spin_sum.dtype != torch.int64 or spin_sum.dim() != 1 or spin_sum.shape[0] < 1:
            raise ValueError("spin_sum must be a one-dimensional int64 tensor")
        n = int(spin_sum.shape[0])
        if not torch.is_tensor(pair_sum) or pair_sum.dtype != torch.int64 or tuple(pair_sum.shape) != (n, n):
            raise ValueError(f"pair_sum must be a ({n}, {n}) int64 tensor")
        if pair_sum.device != spin_sum.device:
            raise ValueError(f"pair_sum must be on the device of spin_sum ({spin_sum.device}), got {pair_sum.device}")
        return cls(spin_sum, pair_sum, count)

    @property
    def n(self) -> int:
        return int(self.spin_sum.shape[0])

    @property
    def mean_spin(self):
        return self.spin_sum.to(torch.float64) / self.count

    @property
    def mean_pair(self):
        return self.pair_sum.to(torch.float64) / self.count

    @property
    def connected(self):
        m = self.mean_spin
        return self.mean_pair - m[:, None] * m[None, :]

    @property
    def pearson(self):
        c = self.connected
        d = torch.diagonal(c)
        return c / torch.sqrt(d[:, None] * d[None, :])

    @property
    def chi_sg(self):
        return (self.connected ** 2).sum() / self.n

    def _edges(self, graph):
        """The plan's edge list as device index tensors, the (n, n) bool mask of the pairs i < j that are edges, and (host
        integers) the number of distinct edges and of pairs i < j."""
        plan = getattr(graph, "plan", graph)
        n = self.n
        if int(plan.n) != n:
            raise ValueError(f"the graph has {int(plan.n)} spins, the sums {n}")
        ei, ej = np.asarray(plan.edge_i, dtype=np.int64), np.asarray(plan.edge_j, dtype=np.int64)
        lo, hi = np.minimum(ei, ej), np.maximum(ei, ej)
        mask = np.zeros((n, n), dtype=bool)
        mask[lo, hi] = True
        dev = self.pair_sum.device
        return (torch.from_numpy(ei).to(dev), torch.from_numpy(ej).to(dev), torch.from_numpy(mask).to(dev), int(mask.sum()),
                n * (n - 1) // 2)

    def _upper(self):
        return torch.triu(torch.ones((self.n, self.n), dtype=torch.bool, device=self.pair_sum.device), diagonal=1)

    def on_edges(self, graph):
        ei, ej, _mask, _e, _p = self._edges(graph)
        return self.connected[ei, ej]

    def off_edge_share(self, graph):
        _ei, _ej, mask, _e, _p = self._edges(graph)
        c2 = self.connected ** 2
        upper = self._upper()
        return (c2 * (upper & ~mask)).sum() / (c2 * upper).sum()

    def top_pairs(self, k: int, graph=None):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError(f"k must be an integer >= 0, got {k!r}")
        n, c = self.n, self.connected
        iu = torch.triu_indices(n, n, 1, device=c.device)  # the pairs i < j in the order of their flat index i n + j
        key, pairs = c[iu[0], iu[1]].abs(), n * (n - 1) // 2
        if graph is not None:
            _ei, _ej, mask, edges, _p = self._edges(graph)
            key = torch.where(mask[iu[0], iu[1]], torch.full_like(key, -1.0), key)  # (behind every pair that is not an edge)
            pairs -= edges
        order = torch.sort(key, descending=True, stable=True).indices[:min(int(k), pairs)]
        i, j = iu[0][order], iu[1][order]
        return i, j, c[i, j]

    def gap(self, other: "Correlations", graph=None) -> dict:
        if not isinstance(other, Correlations) or other.n != self.n:
            raise ValueError(f"other must be Correlations of the same {self.n} spins")
        dm = self.mean_spin - other.mean_spin.to(self.spin_sum.device)
        d2 = (self.mean_pair - other.mean_pair.to(self.pair_sum.device)) ** 2
        upper = self._upper()
        rms = lambda s, cnt: torch.sqrt(s / cnt) if cnt else torch.full_like(s, float("nan"))  # noqa: E731
        res = dict(spin_rms=torch.sqrt((dm ** 2).mean()), pair_rms=rms((d2 * upper).sum(), self.n * (self.n - 1) // 2))
        if graph is not None:
            ei, ej, mask, edges, pairs = self._edges(graph)
            res["edge_rms"] = rms(d2[ei, ej].sum(), int(ei.numel()))
            res["off_edge_rms"] = rms((d2 * (upper & ~mask)).sum(), pairs - edges)
        return res

    def __repr__(self):
        return f"Correlations(n={self.n}, count={self.count})"


class PseudoLikelihood:
    """The pseudo-likelihood of T +-1 rows under a model and what comes with it (``dvg_grbm_fields_packed``, "DVG fields v1";
    :meth:`Trace.pseudo_likelihood`): ``log_pl`` (T,) or (C, M) float64, ``sum_i log P(s_i | rest)`` of every row at ``beta``;
    ``unstable`` int32 of the same shape, the row's spins whose flip would lower the energy; ``cond_sum`` (n,) and ``cond_pair``
    (E,) float64, the pooled sums of ``m_ri = E[s_i | rest of row r]`` and of ``m_ri s_rj + m_rj s_ri`` per edge; ``spin_sum``
    (n,) and ``pair_sum`` (E,) int64, the exact sums of ``s_i`` and ``s_i s_j`` over the same rows (``dvg_grbm_moments_packed``).
    Every member is float64 torch on the data's device (CPU tensors too), no host sync:

    ``count``: T (a host integer);  ``mean``: the mean of ``log_pl``;  ``per_spin``: mean / n;
    ``std_err``: the standard error of ``mean`` -- for (C, M) the between-chain standard deviation of the chain means over
    sqrt(C), whatever the autocorrelation within a chain; for flat rows their standard deviation (ddof = 1) over sqrt(T); NaN
    with fewer than 2 chains or rows;
    ``local_minimum_share``: the share of rows without an unstable spin;
    ``mean_spin`` = cond_sum / T and ``mean_pair`` = cond_pair / (2 T): the Rao-Blackwellised ``<s_i>`` and ``<s_i s_j>``;
    ``residual_linear`` = spin_sum - cond_sum and ``residual_quadratic`` = 2 pair_sum - cond_pair: the pseudo-likelihood's
    residual sums, of zero mean under the model;
    ``grad(prefactor, linear, quadratic, linear_range, quadratic_range)``: the gradient of ``mean`` with respect to the raw
    ``linear`` and ``quadratic`` the rows were scored under, shaped like them: ``-beta residual / T`` per scaled field, times
    ``prefactor``, times 1 where ``lo <= rn(prefactor h) <= hi`` in float32 and 0 where the clamp is active."""

    def __init__(self, log_pl, unstable, cond_sum, cond_pair, spin_sum, pair_sum, beta):
        self.log_pl, self.unstable, self.cond_sum, self.cond_pair = log_pl, unstable, cond_sum, cond_pair
        self.spin_sum, self.pair_sum, self.beta = spin_sum, pair_sum, float(beta)

    @classmethod
    def from_outputs(cls, log_pl, unstable, cond_sum, cond_pair, spin_sum, pair_sum, beta) -> "PseudoLikelihood":
        if not torch.is_tensor(log_pl) or log_pl.dtype != torch.float64 or log_pl.dim() not in (1, 2) or log_pl.numel() < 1:
            raise ValueError("log_pl must be a float64 tensor of shape (rows >= 1,) or (chains >= 1, records >= 1)")
        if not torch.is_tensor(unstable) or unstable.dtype != torch.int32 or unstable.shape != log_pl.shape:
            raise ValueError(f"unstable must be an int32 tensor of log_pl's shape {tuple(log_pl.shape)}")
        for name, t, dt in (("cond_sum", cond_sum, torch.float64), ("cond_pair", cond_pair, torch.float64),
                            ("spin_sum", spin_sum, torch.int64), ("pair_sum", pair_sum, torch.int64)):
            if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 1:
                raise ValueError(f"{name} must be a one-dimensional {str(dt).replace('torch.', '')} tensor")
        if cond_sum.shape[0] < 1 or spin_sum.shape != cond_sum.shape or pair_sum.shape != cond_pair.shape:
            raise ValueError(f"spin_sum {tuple(spin_sum.shape)} / pair_sum {tuple(pair_sum.shape)} must have the shapes of cond_sum "
                             f"{tuple(cond_sum.shape)} / cond_pair {tuple(cond_pair.shape)}, at least one spin")
        if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)) or not 0 <= beta < float("inf"):
            raise ValueError(f"beta must be a finite number >= 0, got {beta!r}")
        return cls(log_pl, unstable, cond_sum, cond_pair, spin_sum, pair_sum, beta)

    @property
    def n(self) -> int:
        return int(self.cond_sum.shape[0])

    @property
    def count(self) -> int:
        return int(self.log_pl.numel())

    @property
    def mean(self):
        return self.log_pl.mean()

    @property
    def per_spin(self):
        return self.mean / self.n

    @property
    def std_err(self):
        x = self.log_pl.mean(1) if self.log_pl.dim() == 2 else self.log_pl
        k = int(x.shape[0])
        if k < 2:
            return torch.full_like(self.mean, float("nan"))
        return x.std(0, unbiased=True) / float(np.sqrt(k))

    @property
    def local_minimum_share(self):
        return (self.unstable == 0).to(torch.float64).mean()

    @property
    def mean_spin(self):
        return self.cond_sum / self.count

    @property
    def mean_pair(self):
        return self.cond_pair / (2.0 * self.count)

    @property
    def residual_linear(self):
        return self.spin_sum.to(torch.float64) - self.cond_sum

    @property
    def residual_quadratic(self):
        return 2.0 * self.pair_sum.to(torch.float64) - self.cond_pair

    def grad(self, prefactor, linear, quadratic, linear_range=None, quadratic_range=None):
        if isinstance(prefactor, bool) or not isinstance(prefactor, (int, float, np.integer, np.floating)) or \
                not float("-inf") < prefactor < float("inf"):
            raise ValueError(f"prefactor must be a finite number, got {prefactor!r}")
        out = []
        for name, raw, res, rng in (("linear", linear, self.residual_linear, linear_range),
                                    ("quadratic", quadratic, self.residual_quadratic, quadratic_range)):
            if not torch.is_tensor(raw) or raw.dtype != torch.float32 or raw.numel() != res.numel():
                raise ValueError(f"{name} must be a float32 tensor of {res.numel()} values")
            g = (-self.beta * float(prefactor) / self.count) * res
            if rng is not None:
                lo, hi = rng
                scaled = raw.detach().reshape(-1).to(res.device) * torch.tensor(float(prefactor), dtype=torch.float32, device=res.device)
                g = g * ((scaled >= float(lo)) & (scaled <= float(hi))).to(torch.float64)
            out.append(g.reshape(raw.shape))
        return out[0], out[1]

    def __repr__(self):
        return f"PseudoLikelihood(n={self.n}, count={self.count}, beta={self.beta:g})"


def pseudo_likelihood(bits, graph, linear, quadratic, *, beta, prefactor=1.0, linear_range=None, quadratic_range=None) -> PseudoLikelihood:
    """The :class:`PseudoLikelihood` of bit-packed rows ((rows, W) or (C, M, W) int32 on the device, views welcome) under the
    prefactor-scaled, clamped ``(linear, quadratic)`` at ``beta``: one pass of ``dvg_grbm_fields_packed`` over the rows and
    the exact sums of ``dvg_grbm_moments_packed``; the rows stay packed.  ``graph``: the :class:`GraphHandle` whose edge list
    ``quadratic`` follows."""
    from . import functional as F  # (functional imports this module)

    f = F.grbm_fields_packed(bits, graph, linear, quadratic, beta=beta, prefactor=prefactor, linear_range=linear_range,
                             quadratic_range=quadratic_range, log_pl=True, unstable=True, conditional=True, fields=False)
    spin_sum, pair_sum = F.grbm_moments_packed(bits.detach().reshape(-1, bits.shape[-1]).contiguous(), graph)
    return PseudoLikelihood.from_outputs(f.log_pl, f.unstable, f.cond_sum, f.cond_pair, spin_sum, pair_sum, beta)


def _popcount32(words):
    """The set bits of every int32 word, int64 (the words read as unsigned)."""
    x = words.to(torch.int64) & 0xFFFFFFFF
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return ((x * 0x01010101) >> 24) & 0xFF


class Distinct:
    """Which of T bit-packed +-1 rows are the same state, and how often each state occurs (``dvg_packed_distinct``, "DVG
    distinct v1"; :func:`distinct`, :meth:`Trace.distinct`, :meth:`Minima.distinct`): the D classes of the rows under equality
    on the spins < n, numbered in the order of their first occurrence.  ``rows`` (D, W) int32: the classes' first rows, pad
    bits cleared; ``counts`` (D,) int64: their sizes; ``index`` and ``first``, int32 of the input's leading shape: every
    row's class and the smallest flattened index with the row's content; ``other_id`` (rows_other,) int32 and ``other_hits``
    (D,) int64 where a second set was looked up (else None): the class equal to each of its rows, -1 for none, and how many of
    its rows each class equals; ``n`` the number of spins.  Every member is torch on the data's device (CPU tensors too); no
    host sync except ``count`` and ``distinct``, which read shapes:

    ``count``: T;  ``distinct``: D;  ``singletons``: the classes of size 1, int64;
    ``entropy``: the plug-in entropy ``-sum p log p`` of p = counts / T, float64 (nats);
    ``collision_share``: ``sum c (c - 1) / (T (T - 1))``, the share of ordered pairs of rows that are equal (NaN for T = 1);
    ``unseen_mass``: the Good-Turing estimate ``singletons / T`` of the probability of states not seen;
    ``top(k)``: ``(rows, counts, classes)`` of the ``k`` largest classes (all if fewer), by falling size, ties by first
    occurrence;
    ``coverage``: ``(found, hit)`` float64 -- the share of ``other``'s rows that equal a class and the share of classes that
    equal a row of ``other`` -- or None without ``other``."""

    def __init__(self, rows, counts, index, first, n, other_id=None, other_hits=None):
        self.rows, self.counts, self.index, self.first, self.n = rows, counts, index, first, int(n)
        self.other_id, self.other_hits = other_id, other_hits

    @classmethod
    def from_outputs(cls, bits, first, id, rep, count, n, other_id=None, other_hits=None) -> "Distinct":
        """From the rows ``bits`` ((T, W) or (C, M, W) int32) and ``functional.packed_distinct``'s outputs for them."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"n must be an integer >= 1, got {n!r}")
        W = (int(n) + 31) // 32
        if not torch.is_tensor(bits) or bits.dtype != torch.int32 or bits.dim() not in (2, 3) or bits.shape[-1] != W or bits.numel() < 1:
            raise ValueError(f"bits must be an int32 tensor of shape (rows >= 1, {W}) or (chains >= 1, records >= 1, {W})")
        lead = bits.shape[:-1]
        T = int(np.prod(lead))
        for name, t in (("first", first), ("id", id)):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.numel() != T:
                raise ValueError(f"{name} must be an int32 tensor of the {T} rows")
        if not torch.is_tensor(rep) or rep.dtype != torch.int32 or rep.dim() != 1 or not 1 <= rep.numel() <= T:
            raise ValueError(f"rep must be a (D,) int32 tensor, 1 <= D <= {T}")
        if not torch.is_tensor(count) or count.dtype != torch.int64 or count.shape != rep.shape:
            raise ValueError(f"count must be a ({rep.numel()},) int64 tensor")
        if (other_id is None) != (other_hits is None):
            raise ValueError("other_id and other_hits go together")
        if other_hits is not None and (not torch.is_tensor(other_hits) or other_hits.dtype != torch.int64 or other_hits.shape != rep.shape):
            raise ValueError(f"other_hits must be a ({rep.numel()},) int64 tensor")
        r = rep.to(torch.int64)
        rows = bits[r] if bits.dim() == 2 else bits[r // int(lead[1]), r % int(lead[1])]
        if int(n) % 32:
            mask = torch.full((W,), -1, dtype=torch.int32, device=rows.device)
            mask[-1] = (1 << (int(n) % 32)) - 1
            rows = rows & mask
        return cls(rows, count, id.view(lead), first.view(lead), n, other_id, other_hits)

    @property
    def count(self) -> int:
        return int(self.index.numel())

    @property
    def distinct(self) -> int:
        return int(self.counts.numel())

    @property
    def singletons(self):
        return (self.counts == 1).sum()

    @property
    def entropy(self):
        p = self.counts.to(torch.float64) / float(self.count)
        return -(p * torch.log(p)).sum()

    @property
    def collision_share(self):
        T = self.count
        return (self.counts * (self.counts - 1)).sum().to(torch.float64) / float(T * (T - 1))

    @property
    def unseen_mass(self):
        return self.singletons.to(torch.float64) / float(self.count)

    def top(self, k: int):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"k must be an integer >= 1, got {k!r}")
        pick = torch.sort(self.counts, descending=True, stable=True).indices[:int(k)]
        return self.rows[pick], self.counts[pick], pick

    @property
    def coverage(self):
        if self.other_id is None:
            return None
        return (self.other_id >= 0).to(torch.float64).mean(), (self.other_hits > 0).to(torch.float64).mean()

    def __repr__(self):
        return f"Distinct(n={self.n}, count={self.count}, distinct={self.distinct})"


def distinct(bits, other=None, *, n) -> Distinct:
    """The :class:`Distinct` of bit-packed rows ((rows, W) or (C, M, W) int32 on the device, views welcome; a 3-D set is pooled):
    one call of ``dvg_packed_distinct`` -- the rows stay packed and ``bits`` is left as it is.  ``other``: a flat (rows, W) set
    to look up among the classes (``other_id``, ``other_hits``, ``coverage``), never inserted."""
    from . import functional as F  # (functional imports this module)

    d = F.packed_distinct(bits, other, n=n)
    return Distinct.from_outputs(bits.detach(), d.first, d.id, d.rep, d.count, int(n), d.other_id, d.other_hits)


class Minima:
    """What a zero-temperature descent of T +-1 rows arrived at (``dvg_grbm_descend_packed``, "DVG descent v1";
    :func:`descend`, :meth:`Trace.descend`): ``start_bits`` and ``bits`` (T, W) or (C, M, W) int32, the rows before and after
    (the pad bits of ``bits`` are 0); ``sweeps``, ``flips``, ``unstable`` int32 of the leading shape -- the sweeps in which
    the row moved, its flips in all, the unstable spins left (0 = a local minimum); ``energy_start`` and ``energy`` float64 of
    the same shape (``dvg_grbm_energy_packed`` before and after); ``n`` the number of spins.  Every member is torch on the
    data's device (CPU tensors too), no host sync except ``count``:

    ``count``: T (a host integer);  ``converged``: bool per row, ``unstable == 0``;  ``converged_share``: its mean;
    ``energy_drop`` = energy_start - energy;
    ``distance``: the Hamming distance from a row to where it ended, int32 (pad bits of the start masked);
    ``mean_flips``, ``mean_sweeps``: float64 means;
    ``unique()``: ``(rows, counts, index)`` -- the distinct final rows (U, W) int32, their multiplicities (U,) int64 and every
    row's index into them (leading shape, int64); ordered by falling multiplicity, ties in the order of
    ``torch.unique(dim=0)`` on the words;
    ``distinct()``: the same partition as a :class:`Distinct` (``dvg_packed_distinct``), the classes by first occurrence;
    ``basin_entropy``: ``-sum p log p`` of the multiplicities over T;
    ``lowest(k)``: ``(rows, energy, counts)`` of the ``k`` distinct final rows of lowest energy (all of them if fewer), by
    rising energy, ties in ``unique()``'s order."""

    def __init__(self, start_bits, bits, sweeps, flips, unstable, energy_start, energy, n):
        self.start_bits, self.bits, self.sweeps, self.flips, self.unstable = start_bits, bits, sweeps, flips, unstable
        self.energy_start, self.energy, self.n = energy_start, energy, int(n)

    @classmethod
    def from_outputs(cls, start_bits, bits, sweeps, flips, unstable, energy_start, energy, n) -> "Minima":
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"n must be an integer >= 1, got {n!r}")
        W = (int(n) + 31) // 32
        if not torch.is_tensor(bits) or bits.dtype != torch.int32 or bits.dim() not in (2, 3) or bits.shape[-1] != W or bits.numel() < 1:
            raise ValueError(f"bits must be an int32 tensor of shape (rows >= 1, {W}) or (chains >= 1, records >= 1, {W})")
        if not torch.is_tensor(start_bits) or start_bits.dtype != torch.int32 or start_bits.shape != bits.shape:
            raise ValueError(f"start_bits must be an int32 tensor of bits' shape {tuple(bits.shape)}")
        lead = bits.shape[:-1]
        for name, t in (("sweeps", sweeps), ("flips", flips), ("unstable", unstable)):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.shape != lead:
                raise ValueError(f"{name} must be an int32 tensor of shape {tuple(lead)}")
        for name, t in (("energy_start", energy_start), ("energy", energy)):
            if not torch.is_tensor(t) or t.dtype != torch.float64 or t.shape != lead:
                raise ValueError(f"{name} must be a float64 tensor of shape {tuple(lead)}")
        return cls(start_bits, bits, sweeps, flips, unstable, energy_start, energy, n)

    @property
    def count(self) -> int:
        return int(self.unstable.numel())

    @property
    def converged(self):
        return self.unstable == 0

    @property
    def converged_share(self):
        return self.converged.to(torch.float64).mean()

    @property
    def energy_drop(self):
        return self.energy_start - self.energy

    @property
    def distance(self):
        x = self.start_bits ^ self.bits
        if self.n % 32:
            mask = torch.full((x.shape[-1],), -1, dtype=torch.int32, device=x.device)
            mask[-1] = (1 << (self.n % 32)) - 1
            x = x & mask
        return _popcount32(x).sum(-1).to(torch.int32)

    @property
    def mean_flips(self):
        return self.flips.to(torch.float64).mean()

    @property
    def mean_sweeps(self):
        return self.sweeps.to(torch.float64).mean()

    def unique(self):
        rows, inverse, counts = torch.unique(self.bits.reshape(-1, self.bits.shape[-1]), dim=0, return_inverse=True, return_counts=True)
        perm = torch.sort(counts, descending=True, stable=True).indices
        rank = torch.empty_like(perm)
        rank[perm] = torch.arange(perm.numel(), dtype=perm.dtype, device=perm.device)
        return rows[perm], counts[perm], rank[inverse.reshape(-1)].view(self.bits.shape[:-1])

    def distinct(self) -> Distinct:
        """The distinct final rows as a :class:`Distinct` (``dvg_packed_distinct``: the rows stay packed, on the device): the
        partition of :meth:`unique`, the classes in the order of their first occurrence."""
        return distinct(self.bits, n=self.n)

    @property
    def basin_entropy(self):
        _rows, counts, _index = self.unique()
        p = counts.to(torch.float64) / float(self.count)
        return -(p * torch.log(p)).sum()

    def lowest(self, k: int):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"k must be an integer >= 1, got {k!r}")
        rows, counts, index = self.unique()
        e = torch.empty((rows.shape[0],), dtype=torch.float64, device=rows.device)
        e[index.reshape(-1)] = self.energy.reshape(-1)  # (equal rows have equal energies: whichever is written last)
        pick = torch.sort(e, stable=True).indices[:int(k)]
        return rows[pick], e[pick], counts[pick]

    def __repr__(self):
        return f"Minima(n={self.n}, count={self.count})"


def descend(bits, graph, linear, quadratic, *, prefactor=1.0, linear_range=None, quadratic_range=None, max_sweeps=1000) -> Minima:
    """The :class:`Minima` of bit-packed rows ((rows, W) or (C, M, W) int32 on the device, views welcome) under the
    prefactor-scaled, clamped ``(linear, quadratic)``: one call of ``dvg_grbm_descend_packed`` -- every row taken to a row
    without an unstable spin, or through ``max_sweeps`` sweeps -- and two of ``dvg_grbm_energy_packed``, before and after; the
    rows stay packed and ``bits`` is left as it is.  ``graph``: the :class:`GraphHandle` whose edge list ``quadratic``
    follows."""
    from . import functional as F  # (functional imports this module)

    kw = dict(prefactor=prefactor, linear_range=linear_range, quadratic_range=quadratic_range)
    d = F.grbm_descend_packed(bits, graph, linear, quadratic, max_sweeps=max_sweeps, **kw)
    return Minima.from_outputs(bits.detach(), d.bits, d.sweeps, d.flips, d.unstable, F.grbm_energy_packed(bits, graph, linear, quadratic, **kw),
                               F.grbm_energy_packed(d.bits, graph, linear, quadratic, **kw), int(graph.plan.n))


class Sliced:
    """What :meth:`GibbsSampler.sample_quantum` returns, for C chains of P Trotter slices ("DVG SQA v1").  ``bits`` (C, P, W) int32
    on the device: the slices one bit per spin ("DVG trace v1": bit b of word w = spin 32 w + b is +1, pad bits 0) -- hand it
    back as ``start`` to continue, or to any packed-row function as ``groups = C``, ``rows = P``; ``samples`` (C, n) float32 +-1:
    slice 0 of every chain; ``slices`` = P; ``n`` the spin count."""

    def __init__(self, bits, samples, n):
        self.bits, self.samples, self.n = bits, samples, int(n)

    @property
    def slices(self) -> int:
        return int(self.bits.shape[1])

    def energy(self, graph, linear, quadratic, prefactor: float = 1.0, linear_range=None, quadratic_range=None) -> torch.Tensor:
        """The (C, P) float64 classical energies of the slices under the prefactor-scaled, clamped ``(linear, quadratic)`` --
        hand in what the draw was given (``dvg_grbm_energy_packed``: the slices stay packed).  ``graph``: the
        :class:`GraphHandle` whose edge list ``quadratic`` follows."""
        from . import functional as F  # (functional imports this module)

        return F.grbm_energy_packed(self.bits, graph, linear, quadratic, prefactor=prefactor, linear_range=linear_range,
                                    quadratic_range=quadratic_range)

    def best(self, graph=None, linear=None, quadratic=None, prefactor: float = 1.0, linear_range=None, quadratic_range=None, *,
             energies: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(C, n) float32 +-1: of each chain the slice of lowest classical energy, ties to the lowest slice index.  The
        energies are :meth:`energy`'s of the same arguments, or ``energies`` (C, P) given (then plain torch, CPU tensors too)."""
        C, P, _W = self.bits.shape
        e = self.energy(graph, linear, quadratic, prefactor, linear_range, quadratic_range) if energies is None else energies
        if not torch.is_tensor(e) or tuple(e.shape) != (C, P):
            raise ValueError(f"energies must be a ({C}, {P}) tensor, got {tuple(e.shape) if torch.is_tensor(e) else type(e).__name__}")
        first = torch.argmax((e == e.min(1, keepdim=True).values).to(torch.int8), 1)  # (the first of the minima)
        rows = self.bits[torch.arange(C, device=self.bits.device), first.to(self.bits.device)]
        return unpack_spins(rows, self.n)

    def slice_overlap(self) -> torch.Tensor:
        """The mean over chains and over the P pairs of neighbouring slices (k, k + 1 mod P) of ``(1 / n) sum_i s[k][i]
        s[k+1][i]``, a float64 scalar on ``bits``' device (plain torch, CPU tensors too): 1 when the slices of every chain
        agree, about 0 when kappa = 0 leaves them independent.  Pad bits are ignored."""
        n, W = self.n, int(self.bits.shape[-1])
        words = self.bits.to(torch.int64) & 0xFFFFFFFF
        diff = words ^ torch.roll(words, -1, 1)
        if n % 32:
            mask = torch.full((W,), 0xFFFFFFFF, dtype=torch.int64, device=self.bits.device)
            mask[-1] = (1 << (n % 32)) - 1
            diff = diff & mask
        d = _popcount32(diff).sum(-1).to(torch.float64)  # Hamming distance of every neighbouring pair
        return (1.0 - 2.0 * d / n).mean()

    def __repr__(self):
        C, P, _W = self.bits.shape
        return f"Sliced({C} chains x {P} slices, n={self.n})"


def trace_sweeps(num_sweeps: int, burn_in: int, thin: int) -> np.ndarray:
    """The recorded sweeps of a traced draw as the numbers k + 1 (k the 0-based sweep of the call), host int64: sweep k is
    recorded iff ``k + 1 > burn_in`` and ``(k + 1 - burn_in) % thin == 0`` -- M = (num_sweeps - burn_in) // thin of them."""
    return burn_in + thin * np.arange(1, max(0, (num_sweeps - burn_in) // thin) + 1, dtype=np.int64)


class Trace:
    """What :meth:`GibbsSampler.sample_trace` returns, for C chains and M records.  ``bits`` (C, M, W) int32 on the device:
    the chains' states after the recorded sweeps, one bit per spin ("DVG trace v1": bit b of word w = spin 32 w + b is +1);
    ``samples`` (C, n) float32 +-1: the final states; ``state`` (C, n) int8: the same, to hand back as ``start``;
    ``sweeps`` (M,) host int64: the recorded sweeps, as k + 1 counted from the call's first sweep; ``n`` the spin count."""

    def __init__(self, bits, samples, state, sweeps, n):
        self.bits, self.samples, self.state, self.sweeps, self.n = bits, samples, state, sweeps, int(n)

    def unpack(self) -> torch.Tensor:
        """(C, M, n) float32 +-1, by plain torch bit operations on ``bits``' device (CPU tensors too)."""
        return unpack_spins(self.bits, self.n)

    def moments(self, graph) -> Moments:
        """Exact moments over all C M records (``dvg_grbm_moments_packed``: the rows stay packed).  ``graph``: the
        :class:`GraphHandle` whose edge list the pair sums follow."""
        from . import functional as F  # (functional imports this module)

        rows = self.bits.reshape(-1, self.bits.shape[-1])
        spin_sum, pair_sum = F.grbm_moments_packed(rows, graph)
        return Moments.from_sums(spin_sum, pair_sum, int(rows.shape[0]))

    @property
    def thin(self) -> int:
        """The sweeps between two records (1 for a single record)."""
        return int(self.sweeps[1] - self.sweeps[0]) if len(self.sweeps) > 1 else 1

    def autocorrelation(self, max_lag: Optional[int] = None, chain_sums: bool = True) -> Autocorrelation:
        """Exact autocorrelation sums of every spin over lags 0 .. ``max_lag`` records (``dvg_trace_autocorr``: the records
        stay packed), as an :class:`Autocorrelation` carrying the trace's ``thin``.  ``max_lag``: an integer in 0 .. M - 1,
        default min(M - 1, 512); ``chain_sums=False`` leaves the per-chain sums (``r_hat``) out."""
        from . import functional as F  # (functional imports this module)

        C, M, _W = self.bits.shape
        if max_lag is None:
            max_lag = min(int(M) - 1, 512)
        if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 0 <= max_lag < M:
            raise ValueError(f"max_lag must be an integer in 0 .. {int(M) - 1} (records - 1), got {max_lag!r}")
        lag_sum, spin_sum, chain_sum = F.trace_autocorr(self.bits, self.n, int(max_lag), chain_sums=bool(chain_sums))
        return Autocorrelation.from_sums(lag_sum, spin_sum, chain_sum, int(C), int(M), self.thin)

    def energy(self, graph, linear, quadratic, prefactor: float = 1.0, linear_range=None, quadratic_range=None) -> torch.Tensor:
        """The (C, M) float64 energies of the records under the prefactor-scaled, clamped ``(linear, quadratic)`` -- hand in
        what the draw was given and these are the energies its chains moved in (``dvg_grbm_energy_packed``: the records stay
        packed).  ``graph``: the :class:`GraphHandle` whose edge list ``quadratic`` follows."""
        from . import functional as F  # (functional imports this module)

        return F.grbm_energy_packed(self.bits, graph, linear, quadratic, prefactor=prefactor, linear_range=linear_range,
                                    quadratic_range=quadratic_range)

    def energy_series(self, graph, linear, quadratic, prefactor: float = 1.0, linear_range=None, quadratic_range=None,
                      max_lag: Optional[int] = None) -> EnergySeries:
        """:meth:`energy` as an :class:`EnergySeries` carrying the trace's ``thin``, over lags 0 .. ``max_lag`` records
        (default min(M - 1, 512))."""
        M = int(self.bits.shape[1]) if torch.is_tensor(self.bits) and self.bits.dim() == 3 else 0
        if max_lag is not None and (isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 0 <= max_lag < M):
            raise ValueError(f"max_lag must be an integer in 0 .. {M - 1} (records - 1), got {max_lag!r}")
        e = self.energy(graph, linear, quadratic, prefactor, linear_range, quadratic_range)
        return EnergySeries.from_energies(e, self.thin, max_lag)

    def overlap(self, other=None, nearest: bool = False):
        """The equal-time replica overlap (``dvg_packed_overlap``: the records stay packed) as an :class:`Overlap`: over every
        record the pairs of distinct chains of this trace, or with ``other`` -- a :class:`Trace` with as many records, its
        ``bits``, or a flat (rows, W) set shared by every record -- the pairs (chain, row of ``other``).  ``nearest=True``
        returns ``(Overlap, (dist, row))`` with the (M, C) int32 nearest partners of ``functional.packed_overlap``."""
        from . import functional as F  # (functional imports this module)

        b = other.bits if isinstance(other, Trace) else other
        hist, near = F.packed_overlap(self.bits, b, n=self.n, nearest=bool(nearest))
        o = Overlap.from_hist(hist, self.n)
        return (o, near) if nearest else o

    def bonds(self, graph, quadratic=None) -> torch.Tensor:
        """The records' bond rows, (C, M, WE) int32 (:func:`bonds`, ``dvg_packed_bonds``: the records stay packed): bit e set
        iff s_i s_j = +1 on edge e of ``graph``, or with ``quadratic`` iff the bond is satisfied."""
        return bonds(self.bits, graph, quadratic)

    def link_overlap(self, graph, other=None) -> LinkOverlap:
        """The equal-time :class:`LinkOverlap` (``dvg_packed_overlap_link``: the records stay packed): over every record the
        pairs of distinct chains of this trace, or with ``other`` -- a :class:`Trace` with as many records, its ``bits``, or
        a flat (rows, W) set shared by every record -- the pairs (chain, row of ``other``), as :meth:`overlap` takes them."""
        return link_overlap(self.bits, graph, other.bits if isinstance(other, Trace) else other)

    def satisfied(self, graph, quadratic) -> torch.Tensor:
        """The number of satisfied couplings of every record under ``quadratic``, int64 (C, M): the popcount of the
        satisfied-mode bond rows (:meth:`bonds`); ``E`` minus it is the record's frustrated bonds."""
        if quadratic is None:
            raise ValueError("satisfied needs the model's quadratic: without it the bonds are products, not satisfied couplings")
        return _popcount32(self.bonds(graph, quadratic)).sum(-1)

    def pseudo_likelihood(self, graph, linear, quadratic, *, beta, prefactor: float = 1.0, linear_range=None,
                          quadratic_range=None) -> PseudoLikelihood:
        """The :class:`PseudoLikelihood` of the C x M records under the prefactor-scaled, clamped ``(linear, quadratic)`` at
        ``beta`` -- hand in what the draw was given and its ``local_minimum_share`` says how many records sit in a local
        minimum, its ``mean_spin`` / ``mean_pair`` are the Rao-Blackwellised moments of :meth:`moments`' rows
        (``dvg_grbm_fields_packed``: the records stay packed)."""
        return pseudo_likelihood(self.bits, graph, linear, quadratic, beta=beta, prefactor=prefactor, linear_range=linear_range,
                                 quadratic_range=quadratic_range)

    def descend(self, graph, linear, quadratic, *, prefactor: float = 1.0, linear_range=None, quadratic_range=None,
                max_sweeps: int = 1000) -> Minima:
        """The :class:`Minima` of the C x M records under the prefactor-scaled, clamped ``(linear, quadratic)``: every record
        quenched to the local minimum below it -- hand in what the draw was given and ``unique()`` counts the distinct minima
        the chains sat above (``dvg_grbm_descend_packed``: the records stay packed and are left as they are)."""
        return descend(self.bits, graph, linear, quadratic, prefactor=prefactor, linear_range=linear_range,
                       quadratic_range=quadratic_range, max_sweeps=max_sweeps)

    def distinct(self, pooled: bool = True):
        """Which states the chains visited (``dvg_packed_distinct``: the records stay packed).  ``pooled=True``: the
        :class:`Distinct` of all C M records under the flattened index c M + m -- ``distinct`` states in all, the plug-in
        ``entropy`` of their visit counts, the Good-Turing ``unseen_mass``.  ``pooled=False``: a (C,) int64 tensor on the
        device, the number of distinct states every chain visited on its own (one call per chain on its slice of ``bits``,
        no copy and no host sync)."""
        if pooled:
            return distinct(self.bits, n=self.n)
        from . import functional as F  # (functional imports this module)

        return F.packed_distinct_counts(self.bits, n=self.n)

    def correlations(self) -> Correlations:
        """The full pair correlations over all C M records, pooled (``dvg_packed_correlation``: the records stay packed), as
        a :class:`Correlations` -- every pair of spins, where :meth:`moments` has the graph's edges only."""
        from . import functional as F  # (functional imports this module)

        C, M, _W = self.bits.shape
        spin_sum, pair_sum = F.packed_correlation(self.bits, n=self.n)
        return Correlations.from_sums(spin_sum, pair_sum, int(C) * int(M))

    def __repr__(self):
        C, M, _W = self.bits.shape
        return f"Trace({C} chains x {M} records, n={self.n})"


class TemperedTrace:
    """What :meth:`GibbsSampler.sample_tempered_trace` returns, for Q ladders of R rungs and M records ("DVG PT trace v1");
    device tensors unless said otherwise.  BY RUNG: ``bits`` (Q, R, M, W) int32, ``[q, r, m]`` the packed state ("DVG trace
    v1") at record m of the chain of ladder q that holds rung r then -- a sample at ``betas[r]``; ``energies`` (Q, R, M)
    float64, that chain's carried energy, or None.  BY CHAIN: ``walk`` (Q, R, M) uint8, ``[q, j, m]`` the rung chain j of
    ladder q holds at record m, or None.  A record is taken behind the exchange that follows its sweep.  ``sweeps`` (M,) host
    int64: the recorded sweeps as k + 1 (``trace_sweeps``); ``final``: the :class:`Tempered` of the draw (hand its ``state`` /
    ``rungs`` back to continue); ``betas`` (R,) host float32; ``n`` the spin count.

    The ladder diagnostics ``occupancy``, ``round_trips`` and ``flow`` are exact integer counts over ``walk``, in vectorised
    torch on its device (CPU tensors too), no host sync.  Their LABEL RULE: at a record a chain is "up" if the last extreme
    rung it held (0 or R - 1, this record included) was rung 0, "down" if it was rung R - 1, and unlabelled before it first
    holds either."""

    def __init__(self, bits, energies, walk, sweeps, final, betas, n):
        self.bits, self.energies, self.walk, self.sweeps, self.final = bits, energies, walk, sweeps, final
        self.betas, self.n = np.asarray(betas, dtype=np.float32), int(n)

    @property
    def thin(self) -> int:
        """The sweeps between two records (1 for a single record)."""
        return int(self.sweeps[1] - self.sweeps[0]) if len(self.sweeps) > 1 else 1

    def rung(self, r: int) -> Trace:
        """The Q chains-at-rung-r as a :class:`Trace` of contiguous (Q, M, W) ``bits``: ``autocorrelation``, ``energy``,
        ``overlap`` and ``moments`` work on it unchanged.  Its ``samples`` are the final states at rung r; it has no ``state``
        (a draw is continued from ``final``).  ``r``: -R .. R - 1."""
        R = int(self.bits.shape[1])
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not -R <= r < R:
            raise ValueError(f"r must be an integer in {-R} .. {R - 1}, got {r!r}")
        samples = self.final.samples[:, r] if self.final is not None and self.final.samples is not None else None
        return Trace(self.bits[:, r].contiguous(), samples, None, self.sweeps, self.n)

    @property
    def target(self) -> Trace:
        """``rung(R - 1)``: the history at ``betas[-1]``."""
        return self.rung(int(self.bits.shape[1]) - 1)

    def energy_series(self, r: int = -1, max_lag: Optional[int] = None) -> EnergySeries:
        """The carried energies of the chains at rung ``r`` (default: the target) as an :class:`EnergySeries` of Q chains x M
        records with the trace's ``thin``, over lags 0 .. ``max_lag`` records (default min(M - 1, 512))."""
        if self.energies is None:
            raise ValueError("this trace was drawn with energies=False")
        R = int(self.energies.shape[1])
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not -R <= r < R:
            raise ValueError(f"r must be an integer in {-R} .. {R - 1}, got {r!r}")
        return EnergySeries.from_energies(self.energies[:, r].contiguous(), self.thin, max_lag)

    def _walk(self, what: str) -> torch.Tensor:
        if self.walk is None:
            raise ValueError(f"{what} needs the rung walk: this trace was drawn with rung_walk=False")
        return self.walk.to(torch.int64)

    def _labels(self, what: str):
        """(walk int64, label int64): +1 up, -1 down, 0 unlabelled -- running maxima of "last record at rung 0" and "last
        record at rung R - 1" (records counted from 1; 0: never)."""
        w = self._walk(what)
        R, M = int(w.shape[1]), int(w.shape[2])
        idx = torch.arange(1, M + 1, dtype=torch.int64, device=w.device)
        zero = torch.zeros((), dtype=torch.int64, device=w.device)
        last_bottom = torch.cummax(torch.where(w == 0, idx, zero), dim=2).values
        last_top = torch.cummax(torch.where(w == R - 1, idx, zero), dim=2).values
        return w, (last_bottom > last_top).to(torch.int64) - (last_top > last_bottom).to(torch.int64)

    def occupancy(self) -> torch.Tensor:
        """(Q, R, R) int64: ``[q, j, r]`` = the records chain j of ladder q spent on rung r (each row sums to M)."""
        w = self._walk("occupancy")
        Q, R, _M = w.shape
        return torch.zeros((Q, R, R), dtype=torch.int64, device=w.device).scatter_add_(2, w, torch.ones_like(w))

    def round_trips(self) -> torch.Tensor:
        """(Q, R) int64 per chain: floor(label changes / 2) under the class's label rule -- a change is a record whose label
        differs from the record before it, both labelled.  A chain that went rung 0 -> R - 1 -> 0 (or R - 1 -> 0 -> R - 1)
        made one round trip."""
        _w, lab = self._labels("round_trips")
        changes = ((lab[:, :, 1:] != lab[:, :, :-1]) & (lab[:, :, :-1] != 0)).sum(2)
        return torch.div(changes, 2, rounding_mode="floor")

    def flow(self) -> torch.Tensor:
        """(R,) float64: f(r) = up(r) / (up(r) + down(r)), up(r) / down(r) the records over all ladders and chains at which a
        chain labelled up / down (the class's label rule) held rung r; unlabelled records are not counted, and a rung no
        labelled chain has visited gives NaN.  f(0) = 1 and f(R - 1) = 0 wherever defined; a ladder with evenly spent effort
        falls linearly in between."""
        w, lab = self._labels("flow")
        R = int(w.shape[1])
        up = torch.zeros(R, dtype=torch.int64, device=w.device).scatter_add_(0, w.reshape(-1), (lab == 1).to(torch.int64).reshape(-1))
        down = torch.zeros(R, dtype=torch.int64, device=w.device).scatter_add_(0, w.reshape(-1), (lab == -1).to(torch.int64).reshape(-1))
        return up.to(torch.float64) / (up + down).to(torch.float64)

    def __repr__(self):
        Q, R, M, _W = self.bits.shape
        return f"TemperedTrace({Q} ladders x {R} rungs x {M} records, n={self.n})"


def _whole(name: str, v, low: int = 1) -> int:
    """``v`` as an int, if it is a whole number of at least ``low`` (a bool is none, nor is anything that is not a number)."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or int(v) < low:
        raise ValueError(f"{name} must be an integer >= {low}, got {v!r}")
    return int(v)


def _ranges(linear_range, quadratic_range) -> Tuple[float, float, float, float]:
    """``(h_lo, h_hi, j_lo, j_hi)`` as the library takes them; None: no clamp."""
    inf = float("inf")
    hl, hh = linear_range if linear_range is not None else (-inf, inf)
    jl, jh = quadratic_range if quadratic_range is not None else (-inf, inf)
    return float(hl), float(hh), float(jl), float(jh)


def _on_gpu(name: str, t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise _lib.DvgError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")


class GibbsSampler:
    """``sample_ising``-compatible local solver running on the MI355X.

    Args:
        plan: graph plan (colour classes + CSR) of the relabelled sub-graph.
        nodes: variable labels in GRBM order (0..n-1 after get_graph_mapping).
        beta: inverse temperature applied to the (h, J) it is handed.  The
            reference sends ``prefactor * (h, J)`` to the QPU
            (/root/reference/src/model_wrapper.py:311); ``beta = 1/prefactor`` makes the
            stationary distribution the GRBM's own ``exp(-E)``.
        sweeps: Gibbs sweeps per draw.   persistent: keep chains between draws (PCD).
        chain_offset: global id of this sampler's first chain (rank sharding).
    """

    PA_BLOCK_BYTES = 1 << 26  # sample_population without `history`: the log weights of this many bytes of steps are kept at a time

    def __init__(self, plan: GibbsPlan, nodes: Sequence, *, beta: float, sweeps: int, seed: int,
                 persistent: bool = True, device="cuda", chain_offset: int = 0,
                 h_range: Tuple[float, float] = (-4.0, 4.0), j_range: Tuple[float, float] = (-1.0, 1.0)):
        self.plan = plan
        self.nodes = list(nodes)
        self.beta = float(beta)
        self.sweeps = int(sweeps)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.persistent = persistent
        self.device = torch.device(device)
        self.chain_offset = int(chain_offset)
        self.properties = {"h_range": list(h_range), "j_range": list(j_range)}
        self._graph: Optional[GraphHandle] = None
        self._state: Optional[torch.Tensor] = None
        self.sweep_count = 0
        self.calls = 0
        # conditional draws (sample_conditional) run under a key and a sweep counter of their own: they never share a
        # random word with the training draws, and interleaving them leaves the training stream as it was
        self.cond_seed = self.seed ^ 0x636F6E64
        self.cond_sweep_count = 0
        # ... and so do the one-off annealed draws (sample_annealed)
        self.anneal_seed = self.seed ^ 0x616E6E6C
        self.anneal_sweep_count = 0
        # ... and the weighed annealed draws (sample_ais, log_partition)
        self.ais_seed = self.seed ^ 0x61697331
        self.ais_sweep_count = 0
        # ... and the exchange draws (sample_tempered)
        self.pt_seed = self.seed ^ 0x70743031
        self.pt_sweep_count = 0
        # ... and the traced draws (sample_trace)
        self.trace_seed = self.seed ^ 0x74726163
        self.trace_sweep_count = 0
        # ... and the population-annealing draws (sample_population), whose counter also numbers the resamplings
        self.pa_seed = self.seed ^ 0x70613031
        self.pa_sweep_count = 0
        # ... and the simulated-quantum-annealing draws (sample_quantum)
        self.sqa_seed = self.seed ^ 0x73716131
        self.sqa_sweep_count = 0
        # ... and the draws with a field per chain (sample_fields)
        self.field_seed = self.seed ^ 0x666C6431
        self.field_sweep_count = 0
        # ... and their weighed, annealed form (sample_fields_ais, log_evidence)
        self.field_ais_seed = self.seed ^ 0x66616931
        self.field_ais_sweep_count = 0
        # set_beta_schedule: the (sweeps,) float32 device table the training draws anneal along; None: fixed beta
        self._betas: Optional[torch.Tensor] = None
        self._fixed_sweeps = self.sweeps

    # -- native fast path ------------------------------------------------------------------
    @property
    def graph(self) -> GraphHandle:
        if self._graph is None:
            self._graph = GraphHandle(self.plan, self.device)
        return self._graph

    def reset(self):
        self._state = None
        self.sweep_count = 0
        self.cond_sweep_count = 0
        self.anneal_sweep_count = 0
        self.ais_sweep_count = 0
        self.pt_sweep_count = 0
        self.trace_sweep_count = 0
        self.pa_sweep_count = 0
        self.sqa_sweep_count = 0
        self.field_sweep_count = 0
        self.field_ais_sweep_count = 0

    def set_beta_schedule(self, betas) -> None:
        """Make every draw of :meth:`sample_native` an annealed one: sweep k of a draw runs at ``betas[k]``, the same
        (S,) schedule for every chain and every draw (``dvg_gibbs_sample_annealed``, shared row).  Sets ``sweeps = S``;
        the key, ``sweep_count``, ``init`` and persistence are those of the fixed-beta draw.  ``betas``: a host sequence,
        array or CPU tensor (checked: finite, >= 0) or a CUDA float32 tensor; it is copied into a device tensor of the
        sampler's own (a new one per call: a captured training step notices and is captured again).  ``None`` restores
        the fixed-beta draw (``dvg_gibbs_sample`` at ``beta``) and the sweeps per draw it had."""
        if betas is None:
            if self._betas is not None:
                self._betas, self.sweeps = None, self._fixed_sweeps
            return
        table = _beta_table(betas, self.device, "betas", own=True)
        if self._betas is None:
            self._fixed_sweeps = self.sweeps
        self._betas, self.sweeps = table, int(table.shape[0])

    def launch_info(self, num_reads: int) -> dict:
        """Launch geometry of one draw of ``num_reads`` chains (``dvg_gibbs_launch_info``: nothing is launched):
        ``workgroups``, ``threads`` per workgroup, ``lds_bytes`` per workgroup."""
        import ctypes

        wg, th, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        _lib.check(_lib.lib().dvg_gibbs_launch_info(self.graph.ptr, int(num_reads), ctypes.byref(wg), ctypes.byref(th),
                                                    ctypes.byref(lds)), "dvg_gibbs_launch_info")
        return {"workgroups": wg.value, "threads": th.value, "lds_bytes": lds.value}

    # -- what the draws share: a draw checks its arguments, allocates its outputs, makes one library call, advances one counter
    def _check_start(self, start, *, count=None, count_name: str = "num_reads", per: int = 1, rungs=None) -> int:
        """The host-side checks of a draw's ``start``, in the one order every draw has: a tensor, its dtype, its shape, the
        chain count the caller named (``count`` groups of ``per`` chains), on the GPU.  The exchange draws' ``rungs`` go
        beside it.  That it lives where the parameters do is :meth:`_parameters`' to check.  Returns the chains."""
        n, named = self.plan.n, (("start", start),) + ((("rungs", rungs),) if per > 1 else ())
        for name, t in named:
            if not torch.is_tensor(t):
                raise _lib.DvgError(f"{name} must be a tensor, got {type(t).__name__}")
        if start.dtype not in (torch.float32, torch.int8):
            raise _lib.DvgError(f"start must be float32 or int8 (+-1), got {start.dtype}")
        if start.dim() != 2 or start.shape[1] != n or start.shape[0] < 1 or start.shape[0] % per:
            raise _lib.DvgError(f"start must be ({'chains' if per == 1 else f'ladders x {per}'}, {n}), got {tuple(start.shape)}")
        C = int(start.shape[0])
        if per > 1 and (rungs.dtype not in (torch.int32, torch.int64) or tuple(rungs.shape) != (C,)):
            raise _lib.DvgError(f"rungs must be ({C},) int32 or int64, got {tuple(rungs.shape)} {rungs.dtype}")
        if count is not None and count != C // per:
            raise _lib.DvgError(f"{count_name}={count!r} but start has {C} chains" + (f" ({per} per ladder)" if per > 1 else ""))
        for name, t in named:
            _on_gpu(name, t)
        return C

    def _parameters(self, linear, quadratic, **beside):
        """``(lin, quad)``: the detached parameters, on the GPU, contiguous and of the graph's sizes.  ``beside``: the draw's
        other tensors by name (None and host values pass); one on another GPU than the parameters' is an error."""
        lin = _lib.require_cuda(linear.detach(), "linear")
        quad = _lib.require_cuda(quadratic.detach(), "quadratic")
        if lin.numel() != self.plan.n or quad.numel() != self.plan.n_edges:
            raise _lib.DvgError("linear/quadratic do not match the sampler's graph")
        for name, t in beside.items():
            if torch.is_tensor(t) and t.is_cuda and t.device != lin.device:
                raise _lib.DvgError(f"{name} is on {t.device}, the model parameters on {lin.device}")
        return lin, quad

    def _own_chains(self, start, C: int, device):
        """``(state, init)`` of a one-off draw, never the persistent chains: an empty buffer the INIT stream fills, or the
        call's own contiguous int8 copy of ``start``."""
        if start is None:
            return torch.empty((C, self.plan.n), dtype=torch.int8, device=device), 1
        return start.detach().to(torch.int8, copy=True).contiguous(), 0

    def _call(self, name: str, lin, quad, prefactor, linear_range, quadratic_range, *rest) -> None:
        """One library call on the parameters' device and current stream: the graph and the model arguments every draw's entry
        point begins with, then ``rest`` (which ends with ``dyn`` where the entry point has one), then the stream."""
        head = (lin.data_ptr(), quad.data_ptr(), float(prefactor)) + _ranges(linear_range, quadratic_range)
        with torch.cuda.device(lin.device):
            _lib.check(getattr(_lib.lib(), name)(self.graph.ptr, *head, *rest, _lib.stream_ptr(lin.device)), name)

    def sample_native(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float,
                      linear_range=None, quadratic_range=None, num_reads: int = 256) -> torch.Tensor:
        """Device tensors in, (num_reads, n) float32 +-1 device tensor out; no host sync."""
        lin, quad = self._parameters(linear, quadratic)
        n = self.plan.n
        init = 0
        if self._state is None or not self.persistent or self._state.shape[0] != num_reads:
            self._state = torch.empty((num_reads, n), dtype=torch.int8, device=lin.device)
            init = 1
            if not self.persistent:
                pass  # fresh chains every call; the sweep counter keeps the random stream moving
        out = torch.empty((num_reads, n), dtype=torch.float32, device=lin.device)
        betas = self._betas
        if betas is not None and (betas.device != lin.device or int(betas.shape[0]) != self.sweeps):
            raise _lib.DvgError(f"the beta schedule ({tuple(betas.shape)} on {betas.device}) does not match the draw "
                                f"({self.sweeps} sweeps on {lin.device}); set it again with set_beta_schedule")
        tail = (self._state.data_ptr(), num_reads, self.chain_offset & 0xFFFFFFFF, self.seed, self.sweep_count & 0xFFFFFFFF,
                self.sweeps, init, out.data_ptr(), _lib.DYN)
        if betas is None:
            self._call("dvg_gibbs_sample", lin, quad, prefactor, linear_range, quadratic_range, self.beta, *tail)
        else:
            self._call("dvg_gibbs_sample_annealed", lin, quad, prefactor, linear_range, quadratic_range, betas.data_ptr(), 0, *tail)
        self.sweep_count += self.sweeps
        self.calls += 1
        return out

    def sample_conditional(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float,
                           linear_range, quadratic_range, start: torch.Tensor, clamp: torch.Tensor, *,
                           sweeps: Optional[int] = None, init_free: bool = True) -> torch.Tensor:
        """A conditional draw (``dvg_gibbs_sample_clamped``): the spins flagged in ``clamp`` are held at their value in
        ``start``, the others are redrawn from their conditionals under the same ``(h, J)``.

        ``start``: (C, n) float32 or int8; its values must be +-1 (not checked: that would be a host sync).  ``clamp``: (C, n), or (n,) for one held set shared by all chains, bool or
        uint8.  ``init_free``: the free spins start from the INIT stream (else from ``start``).  Returns (C, n) float32
        +-1 on the device; no host sync.

        Apart from the graph handle it shares nothing with the training draws: it leaves the persistent chains,
        ``sweep_count`` and ``calls`` alone, counts its sweeps in ``cond_sweep_count`` and draws its random words under
        its own key ``cond_seed``; chain ids are ``chain_offset + arange(C)``."""
        n = self.plan.n
        C = self._check_start(start)
        if tuple(clamp.shape) not in ((C, n), (n,)):
            raise _lib.DvgError(f"clamp must be ({C}, {n}) or ({n},), got {tuple(clamp.shape)}")
        if clamp.dtype not in (torch.bool, torch.uint8):
            raise _lib.DvgError(f"clamp must be bool or uint8, got {clamp.dtype}")
        _on_gpu("clamp", clamp)
        lin, quad = self._parameters(linear, quadratic, start=start, clamp=clamp)
        state, _init = self._own_chains(start, C, lin.device)
        flags = clamp.detach().to(torch.uint8).contiguous()
        stride = n if flags.dim() == 2 else 0
        n_sweeps = self.sweeps if sweeps is None else int(sweeps)
        out = torch.empty((C, n), dtype=torch.float32, device=lin.device)
        self._call("dvg_gibbs_sample_clamped", lin, quad, prefactor, linear_range, quadratic_range, self.beta, state.data_ptr(), C,
                   self.chain_offset & 0xFFFFFFFF, self.cond_seed, self.cond_sweep_count & 0xFFFFFFFF, n_sweeps,
                   int(bool(init_free)), flags.data_ptr(), stride, out.data_ptr(), None)
        self.cond_sweep_count += n_sweeps
        return out

    def sample_fields(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range, quadratic_range,
                      fields: torch.Tensor, *, start: Optional[torch.Tensor] = None, sweeps: Optional[int] = None,
                      num_reads: Optional[int] = None) -> torch.Tensor:
        """A draw with a linear field of its own per chain (``dvg_gibbs_sample_fields``, "DVG field v1" in include/dvg.h):
        chain c samples the model ``(linear + fields[c], quadratic)`` -- soft evidence, where :meth:`sample_conditional`
        holds spins outright.  :func:`logit_fields` makes the fields of factorial logits (posterior refinement: a prior times
        an encoder's logits, one image per chain); a batch of Ising problems that share their couplings is ``fields =
        h_batch - linear``.

        ``fields``: float32, on the parameters' GPU, in the raw units of ``linear`` (``prefactor`` and ``linear_range`` apply
        to the sum); (C, n), a row per chain, or (n,), one row for all chains, with ``start`` or ``num_reads`` naming C.  Its
        values must be finite (not checked: that would be a host sync).  ``start``: (C, n) float32 or int8 +-1 to start the
        chains from; None: the INIT stream.  ``sweeps``: default the sampler's.  Returns (C, n) float32 +-1 on the device;
        no host sync.

        Like :meth:`sample_conditional` it leaves the persistent chains, ``sweep_count`` and ``calls`` alone; it counts its
        sweeps in ``field_sweep_count`` and draws its random words under its own key ``field_seed``; chain ids are
        ``chain_offset + arange(C)``."""
        n = self.plan.n
        if not torch.is_tensor(fields):
            raise _lib.DvgError(f"fields must be a tensor, got {type(fields).__name__}")
        if fields.dtype != torch.float32:
            raise _lib.DvgError(f"fields must be float32, got {fields.dtype}")
        if fields.dim() not in (1, 2) or fields.shape[-1] != n or fields.shape[0] < 1:
            raise _lib.DvgError(f"fields must be (chains, {n}) or ({n},), got {tuple(fields.shape)}")
        rows = int(fields.shape[0]) if fields.dim() == 2 else None
        if num_reads is not None:
            num_reads = _whole("num_reads", num_reads)
        if start is not None:
            C = self._check_start(start, count=num_reads)
        elif num_reads is not None:
            C = num_reads
        elif rows is not None:
            C = rows
        else:
            raise ValueError(f"fields of shape ({n},) need start or num_reads to know how many chains to draw")
        if rows is not None and rows != C:
            raise _lib.DvgError(f"fields has {rows} rows but the draw has {C} chains")
        n_sweeps = self.sweeps if sweeps is None else _whole("sweeps", sweeps, low=0)
        _on_gpu("fields", fields)
        lin, quad = self._parameters(linear, quadratic, start=start, fields=fields)
        state, init = self._own_chains(start, C, lin.device)
        rows_dev = fields.detach().contiguous()
        out = torch.empty((C, n), dtype=torch.float32, device=lin.device)
        self._call("dvg_gibbs_sample_fields", lin, quad, prefactor, linear_range, quadratic_range, self.beta, state.data_ptr(), C,
                   self.chain_offset & 0xFFFFFFFF, self.field_seed, self.field_sweep_count & 0xFFFFFFFF, n_sweeps, init,
                   rows_dev.data_ptr(), n if rows is not None else 0, out.data_ptr(), None)
        self.field_sweep_count += n_sweeps
        return out

    def sample_fields_ais(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range, quadratic_range,
                          fields: torch.Tensor, betas=None, scales=None, *, chains_per_row: int = 1,
                          start: Optional[torch.Tensor] = None, num_reads: Optional[int] = None, beta_from: float = 0.0,
                          scale_from: float = 1.0):
        """The per-chain-field draw along a path in (beta, field strength), weighed (``dvg_gibbs_sample_fields_ais``, "DVG field
        AIS v1" in include/dvg.h): sweep k of chain c runs at ``betas[k]`` (or ``betas[c, k]``) on the model ``(linear +
        scales[k] * fields[row of c], quadratic)``, and the kernel carries the chain's energy and the log importance weight of
        annealed importance sampling along that path.  Over the chains of one row, ``logsumexp(log_weights) - log(count)``
        estimates ``log Z(betas[-1], scales[-1]) - log Z(beta_from, scale_from)`` of that row's model (:meth:`log_evidence`).

        ``fields``: as for :meth:`sample_fields`; (rows, n) makes ``rows * chains_per_row`` chains, chain c reading row ``c //
        chains_per_row`` (the rows are not replicated in memory); (n,): one row for all chains, ``start`` or ``num_reads``
        naming them.  ``betas``, ``scales``: (S,) or (C, S) tables under the rules of :meth:`sample_annealed` -- host values
        are checked (finite; betas >= 0) and uploaded, a CUDA float32 tensor is used as it is.  ``betas=None``: the sampler's
        own beta on every sweep; ``scales=None``: strength 1 throughout; one of the two must be given, and both must name the
        same S.  ``beta_from``, ``scale_from``: the point of the path ``start`` is a sample at; fresh chains (``start=None``)
        are uniform and need ``beta_from == 0``.  Returns ``(samples, log_weights, energies)``: (C, n) float32 +-1, (C,)
        float64, (C,) float64 on the device; no host sync.

        Its own key ``field_ais_seed`` and counter ``field_ais_sweep_count``: every other stream, the persistent chains,
        ``sweep_count`` and ``calls`` are left alone; chain ids are ``chain_offset + arange(C)``."""
        n = self.plan.n
        if not torch.is_tensor(fields):
            raise _lib.DvgError(f"fields must be a tensor, got {type(fields).__name__}")
        if fields.dtype != torch.float32:
            raise _lib.DvgError(f"fields must be float32, got {fields.dtype}")
        if fields.dim() not in (1, 2) or fields.shape[-1] != n or fields.shape[0] < 1:
            raise _lib.DvgError(f"fields must be (rows, {n}) or ({n},), got {tuple(fields.shape)}")
        R = _whole("chains_per_row", chains_per_row)
        rows = int(fields.shape[0]) if fields.dim() == 2 else None
        if betas is None and scales is None:
            raise ValueError("sample_fields_ais needs betas, scales or both: they name the sweeps")
        bf, sf = float(beta_from), float(scale_from)
        with np.errstate(over="ignore"):
            if not np.isfinite(np.float32(bf)) or bf < 0.0:
                raise ValueError(f"beta_from={beta_from!r} must be finite and >= 0")
            if not np.isfinite(np.float32(sf)):
                raise ValueError(f"scale_from={scale_from!r} must be finite")
        if start is None and np.float32(bf) != 0.0:
            raise ValueError(f"beta_from={beta_from!r} with fresh chains: they are uniform, a sample at beta 0 and at no other; "
                             "give the chains' states as `start`")
        if num_reads is not None:
            num_reads = _whole("num_reads", num_reads)
        if start is not None:
            C = self._check_start(start, count=num_reads)
        elif num_reads is not None:
            C = num_reads
        elif rows is not None:
            C = rows * R
        else:
            raise ValueError(f"fields of shape ({n},) need start or num_reads to know how many chains to draw")
        if rows is not None and rows * R != C:
            raise _lib.DvgError(f"fields has {rows} rows of {R} chains each but the draw has {C} chains")
        host_b = None if betas is None else _check_beta_table(betas, "betas", rows=C)
        host_s = None if scales is None else _check_beta_table(scales, "scales", rows=C, signed=True)
        shapes = [tuple(t.shape) if hasattr(t, "shape") else np.shape(t) for t in (betas, scales) if t is not None]
        S = int(shapes[0][-1])
        if any(int(sh[-1]) != S for sh in shapes):
            raise _lib.DvgError(f"betas names {int(shapes[0][-1])} sweeps, scales {int(shapes[1][-1])}")
        _on_gpu("fields", fields)
        lin, quad = self._parameters(linear, quadratic, start=start, fields=fields, betas=betas, scales=scales)
        if betas is None:
            b_table = torch.full((S,), self.beta, dtype=torch.float32, device=lin.device)
        else:
            b_table = _beta_table(betas, lin.device, "betas", rows=C, host=host_b)
        s_table = None if scales is None else _beta_table(scales, lin.device, "scales", rows=C, host=host_s)
        state, init = self._own_chains(start, C, lin.device)
        rows_dev = fields.detach().contiguous()
        out = torch.empty((C, n), dtype=torch.float32, device=lin.device)
        log_w = torch.empty((C,), dtype=torch.float64, device=lin.device)
        energy = torch.empty((C,), dtype=torch.float64, device=lin.device)
        self._call("dvg_gibbs_sample_fields_ais", lin, quad, prefactor, linear_range, quadratic_range,
                   b_table.data_ptr(), S if b_table.dim() == 2 else 0, bf,
                   None if s_table is None else s_table.data_ptr(), S if s_table is not None and s_table.dim() == 2 else 0, sf,
                   state.data_ptr(), C, self.chain_offset & 0xFFFFFFFF, self.field_ais_seed,
                   self.field_ais_sweep_count & 0xFFFFFFFF, S, init, rows_dev.data_ptr(), n if rows is not None else 0, R,
                   out.data_ptr(), log_w.data_ptr(), energy.data_ptr(), None)
        self.field_ais_sweep_count += S
        return out, log_w, energy

    def log_evidence(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range, quadratic_range,
                     fields: torch.Tensor, *, chains_per_row: int = 64, num_sweeps: int = 100, burn_in: Optional[int] = None,
                     start: Optional[torch.Tensor] = None) -> "LogEvidence":
        """Per row of ``fields`` (rows, n), the estimate of ``log(Z_r / Z)``: ``Z`` the normaliser of the distribution the
        sampler draws from, ``Z_r`` that of the same model with row r added to its linear terms.  With ``fields =
        logit_fields(logits, ...)`` this is the log of the prior mass that agrees with the evidence, ``log sum_z p(z) prod_i
        exp(l_i z_i / 2)``, without an estimate of ``log Z``.

        ``chains_per_row`` chains per row start as draws of the prior -- ``start`` (rows * chains_per_row, n) if given, else
        one :meth:`sample_fields` call with a shared all-zero row and ``burn_in`` sweeps (default: the sampler's ``sweeps``) from
        fresh chains -- and one :meth:`sample_fields_ais` call at the sampler's beta turns the rows on linearly over
        ``num_sweeps`` sweeps, ``scales = linspace(0, 1, num_sweeps + 1)[1:]``, weighing each step.  Returns a
        :class:`LogEvidence`; its reductions are torch ops on the device, no host sync.

        The estimate is unbiased in ``Z_r / Z`` only if the start states are draws of the prior: chains that are not yet at
        equilibrium after ``burn_in`` sweeps bias it, and the standard error does not show that."""
        n = self.plan.n
        if not torch.is_tensor(fields) or fields.dim() != 2 or fields.shape[-1] != n or fields.shape[0] < 1:
            raise _lib.DvgError(f"fields must be a (rows, {n}) tensor, got "
                                f"{tuple(fields.shape) if torch.is_tensor(fields) else type(fields).__name__}")
        R, S = _whole("chains_per_row", chains_per_row), _whole("num_sweeps", num_sweeps)
        rows = int(fields.shape[0])
        burn = self.sweeps if burn_in is None else _whole("burn_in", burn_in, low=0)
        if start is None:
            zero = torch.zeros((n,), dtype=torch.float32, device=fields.device)
            start = self.sample_fields(linear, quadratic, prefactor, linear_range, quadratic_range, zero, sweeps=burn,
                                       num_reads=rows * R)
        scales = np.linspace(0.0, 1.0, S + 1)[1:].astype(np.float32)
        samples, log_w, _energy = self.sample_fields_ais(linear, quadratic, prefactor, linear_range, quadratic_range, fields, None,
                                                         scales, chains_per_row=R, start=start, beta_from=self.beta, scale_from=0.0)
        return LogEvidence.from_weights(log_w.view(rows, R), samples)

    def _annealed_arguments(self, linear, quadratic, betas, num_reads, start, beta_from=None):
        """The argument checks and buffers :meth:`sample_annealed` and :meth:`sample_ais` share; every check comes before
        the first library call (the table's upload included).  Returns them by name: ``lin``, ``quad``, the device ``table``
        of ``S`` sweeps and its chain ``stride``, the ``C`` chains' ``state`` and ``init``, and ``out``."""
        if beta_from is not None:  # (sample_ais)
            bf = float(beta_from)
            with np.errstate(over="ignore"):
                finite = bool(np.isfinite(np.float32(bf)))
            if not finite or bf < 0.0:
                raise ValueError(f"beta_from={beta_from!r} must be finite and >= 0")
            if start is None and np.float32(bf) != 0.0:
                raise ValueError(f"beta_from={beta_from!r} with fresh chains: they are uniform, a sample at beta 0 and at no "
                                 "other; give the chains' states as `start`")
        if start is not None:
            C = self._check_start(start, count=num_reads)
        elif num_reads is not None:
            C = _whole("num_reads", num_reads)
        else:
            try:
                shape = tuple(betas.shape) if hasattr(betas, "shape") else np.shape(betas)
            except ValueError:
                shape = ()
            if len(shape) != 2 or int(shape[0]) < 1:
                raise ValueError("an annealed draw needs num_reads, start or a (chains, sweeps) table to know how many chains to draw")
            C = int(shape[0])
        _check_beta_table(betas, "betas", rows=C)
        lin, quad = self._parameters(linear, quadratic, start=start, betas=betas)
        table = _beta_table(betas, lin.device, "betas", rows=C)
        S = int(table.shape[-1])
        state, init = self._own_chains(start, C, lin.device)
        out = torch.empty((C, self.plan.n), dtype=torch.float32, device=lin.device)
        return SimpleNamespace(lin=lin, quad=quad, table=table, S=S, stride=S if table.dim() == 2 else 0, C=C, state=state,
                               init=init, out=out)

    def sample_annealed(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range,
                        quadratic_range, betas, *, num_reads: Optional[int] = None,
                        start: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A one-off annealed draw (``dvg_gibbs_sample_annealed``): sweep k runs at ``betas[k]`` -- ``betas`` of shape
        (S,), one schedule for all chains -- or at ``betas[c, k]`` on chain c -- shape (C, S), a temperature ladder.
        ``betas``: a host sequence, array or CPU tensor (checked here: finite, >= 0; then uploaded) or a CUDA float32
        tensor, used as it is.  ``start=None``: ``num_reads`` fresh chains from the INIT stream (with a (C, S) table
        ``num_reads`` defaults to C); ``start`` (C, n) int8 or float32 +-1 on the device: the chains begin there.
        Returns (C, n) float32 +-1 on the device; no host sync.

        Apart from the graph handle it shares nothing with the training draws: it leaves the persistent chains,
        ``sweep_count``, ``calls`` and any schedule set with :meth:`set_beta_schedule` alone, counts its sweeps in
        ``anneal_sweep_count`` and draws its random words under its own key ``anneal_seed``; chain ids are
        ``chain_offset + arange(C)``."""
        a = self._annealed_arguments(linear, quadratic, betas, num_reads, start)
        self._call("dvg_gibbs_sample_annealed", a.lin, a.quad, prefactor, linear_range, quadratic_range, a.table.data_ptr(), a.stride,
                   a.state.data_ptr(), a.C, self.chain_offset & 0xFFFFFFFF, self.anneal_seed, self.anneal_sweep_count & 0xFFFFFFFF,
                   a.S, a.init, a.out.data_ptr(), None)
        self.anneal_sweep_count += a.S
        return a.out

    def sample_ais(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range, quadratic_range,
                   betas, *, num_reads: Optional[int] = None, start: Optional[torch.Tensor] = None, beta_from: float = 0.0):
        """An annealed draw, weighed (``dvg_gibbs_sample_ais``, "DVG AIS v1" in include/dvg.h): the chains of
        :meth:`sample_annealed` with the same arguments plus, per chain, the log importance weight of annealed
        importance sampling, ``-sum_k (betas[k] - betas[k-1]) E(state before sweep k)`` with ``betas[-1] = beta_from``, and
        the energy of the returned state under the scaled, clamped ``(h, J)`` -- both accumulated inside the kernel.
        ``log Z(betas[-1]) ~= log Z(beta_from) + logsumexp(log_weights) - log C`` (:meth:`log_partition`).

        The argument rules are :meth:`sample_annealed`'s.  ``beta_from``: the inverse temperature ``start`` is a sample
        of; fresh chains (``start=None``) are uniform, so they need ``beta_from == 0``.  Returns ``(samples, log_weights,
        energies)``: (C, n) float32 +-1, (C,) float64, (C,) float64, on the device; no host sync.

        Its own key ``ais_seed`` and counter ``ais_sweep_count``: the training, conditional and annealed streams are
        left alone."""
        a = self._annealed_arguments(linear, quadratic, betas, num_reads, start, beta_from=beta_from)
        log_w = torch.empty((a.C,), dtype=torch.float64, device=a.lin.device)
        energy = torch.empty((a.C,), dtype=torch.float64, device=a.lin.device)
        self._call("dvg_gibbs_sample_ais", a.lin, a.quad, prefactor, linear_range, quadratic_range, a.table.data_ptr(), a.stride,
                   float(beta_from), a.state.data_ptr(), a.C, self.chain_offset & 0xFFFFFFFF, self.ais_seed,
                   self.ais_sweep_count & 0xFFFFFFFF, a.S, a.init, a.out.data_ptr(), log_w.data_ptr(), energy.data_ptr(), None)
        self.ais_sweep_count += a.S
        return a.out, log_w, energy

    def log_partition(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range, quadratic_range,
                      *, beta: Optional[float] = None, num_sweeps: int = 1000, num_reads: int = 1024,
                      schedule: str = "linear") -> "LogPartition":
        """The AIS estimate of ``log Z(beta)`` of the scaled, clamped model (``beta=None``: the sampler's own):
        ``num_reads`` fresh chains annealed from beta 0 -- where ``log Z = n log 2`` -- to ``beta`` over ``num_sweeps``
        sweeps through :meth:`sample_ais`.  ``schedule`` "linear": ``linspace(0, beta, num_sweeps)``; "geometric": 0, then
        ``geomspace(beta / num_sweeps, beta, num_sweeps - 1)``.  Returns a :class:`LogPartition`; its reductions are
        plain torch ops on the device, no host sync."""
        if schedule not in ("linear", "geometric"):
            raise ValueError(f"schedule must be 'linear' or 'geometric', got {schedule!r}")
        num_sweeps = _whole("num_sweeps", num_sweeps, 2)
        b = float(self.beta if beta is None else beta)
        if not np.isfinite(b) or b <= 0.0:
            raise ValueError(f"beta={beta!r} must be finite and > 0")
        if schedule == "linear":
            betas = beta_schedule(0.0, b, num_sweeps, "linear")
        else:
            betas = np.concatenate([np.zeros(1, np.float32), beta_schedule(b / num_sweeps, b, num_sweeps - 1, "geometric")])
        samples, log_w, _energy = self.sample_ais(linear, quadratic, prefactor, linear_range, quadratic_range, betas,
                                                  num_reads=num_reads)
        return LogPartition.from_weights(self.plan.n, log_w, samples)

    def sample_population(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range, quadratic_range,
                          betas, *, num_reads: int, num_populations: int = 1, sweeps_per_beta: int = 1,
                          history: bool = False) -> "Population":
        """A population-annealing draw (sequential Monte Carlo; "DVG PA v1" in include/dvg.h): ``num_reads`` fresh chains in
        ``num_populations`` independent populations of consecutive chains are annealed through ``betas`` (T,) -- a host
        sequence, array or CPU tensor, finite and >= 0, with ``betas[-1] = 0`` before it -- and after every temperature step
        each population is resampled in proportion to its chains' weights: heavy chains are copied, light ones dropped, so
        every chain keeps working and the samples are equally weighted at every temperature.  Step t: (1)
        ``dvg_gibbs_sample_ais`` on the chains in place, ``sweeps_per_beta`` sweeps at ``betas[t]`` weighed from
        ``betas[t - 1]``; (2) each population's ``logsumexp(log_weights) - log R`` is added to its log Z (plain torch ops, a
        block of steps at a time); (3) ``dvg_population_resample`` with ``step`` the global index of the sweep after the step's last.  The last step is
        resampled too.  (The weight depends on the state before the sweeps only and the sweeps leave the new distribution
        invariant: move-then-resample is properly weighted.)  Returns a :class:`Population`; ``history=True`` keeps every
        step's ``log_weights`` and ``parents``.  The table is uploaded once; no host sync.

        Its own key ``pa_seed`` and counter ``pa_sweep_count``: every other stream and counter is left alone.  Chain ids are
        ``chain_offset + arange(num_reads)``."""
        n = self.plan.n
        # every argument check comes before the first library call (the table's upload included)
        if torch.is_tensor(betas) and betas.is_cuda:
            raise _lib.DvgError("betas: the schedule is a host sequence, array or CPU tensor (it is checked, then uploaded)")
        sched = _check_beta_table(betas, "betas")
        if sched.ndim != 1:
            raise _lib.DvgError(f"betas must be (steps,), got {tuple(sched.shape)}")
        C, P = _whole("num_reads", num_reads), _whole("num_populations", num_populations)
        theta, T = _whole("sweeps_per_beta", sweeps_per_beta), int(sched.size)
        if C % P:
            raise ValueError(f"num_populations={num_populations!r} does not divide num_reads={num_reads!r}")
        if C // P > 2 ** 20:
            raise ValueError(f"num_reads={num_reads!r} / num_populations={num_populations!r}: more than 2^20 chains per population")
        lin, quad = self._parameters(linear, quadratic)
        dev = lin.device
        L = _lib.lib()
        table = torch.from_numpy(np.repeat(sched, theta)).to(dev)  # (T theta,) float32: each call points into it
        state, other = (torch.empty((C, n), dtype=torch.int8, device=dev) for _ in range(2))
        families, other_families = None, torch.empty((C,), dtype=torch.int32, device=dev)
        # the steps' log weights are kept in rows (all T with `history`, else a ring of at most PA_BLOCK_BYTES) and the
        # estimates are taken a block of rows at a time: a handful of torch launches per block instead of per step
        rows = T if history else min(T, max(1, self.PA_BLOCK_BYTES // (8 * C)))
        log_w = torch.empty((rows, C), dtype=torch.float64, device=dev)
        parents = torch.empty((T if history else 1, C), dtype=torch.int32, device=dev)
        log_z = torch.full((P,), n * float(np.log(2.0)), dtype=torch.float64, device=dev)
        ess = torch.empty((T, P), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            ws = torch.empty((int(L.dvg_population_resample_workspace_bytes(C)),), dtype=torch.uint8, device=dev)
            stream = _lib.stream_ptr(dev)
            for t in range(T):
                lw = log_w.data_ptr() + 8 * C * (t % rows)
                par = parents.data_ptr() + (4 * C * t if history else 0)
                sweep0 = self.pa_sweep_count + t * theta
                self._call("dvg_gibbs_sample_ais", lin, quad, prefactor, linear_range, quadratic_range, table.data_ptr() + 4 * t * theta,
                           0, float(sched[t - 1]) if t else 0.0, state.data_ptr(), C, self.chain_offset & 0xFFFFFFFF, self.pa_seed,
                           sweep0 & 0xFFFFFFFF, theta, int(t == 0), None, lw, None, None)
                _lib.check(
                    L.dvg_population_resample(lw, C, P, self.chain_offset & 0xFFFFFFFF, self.pa_seed,
                                              (sweep0 + theta) & 0xFFFFFFFF, state.data_ptr(), other.data_ptr(), n,
                                              _lib.ptr(families), other_families.data_ptr(), par, None, ws.data_ptr(), ws.numel(),
                                              stream),
                    "dvg_population_resample",
                )
                state, other = other, state
                families, other_families = other_families, (families if families is not None else torch.empty_like(other_families))
                if (t + 1) % rows == 0 or t == T - 1:  # the block of steps whose weights the rows hold
                    first = t - t % rows
                    inc, ess[first:t + 1] = Population.step_estimates(log_w[:t + 1 - first], P)
                    log_z = log_z + inc.sum(0)
        self.pa_sweep_count += T * theta
        return Population.from_estimates(log_z, families, ess, state.to(torch.float32), state, log_w if history else None,
                                         parents if history else None)

    def sample_tempered(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range, quadratic_range,
                        betas, *, num_ladders: int, num_sweeps: Optional[int] = None, swap_every: int = 1,
                        start: Optional[torch.Tensor] = None, rungs: Optional[torch.Tensor] = None) -> "Tempered":
        """A parallel-tempering (replica-exchange) draw (``dvg_gibbs_sample_tempered``, "DVG PT v1" in include/dvg.h):
        ``num_ladders`` ladders of R = ``len(betas)`` chains each.  A chain sweeps at the beta of the rung it holds; after
        every ``swap_every`` sweeps the chains on neighbouring rungs of a ladder exchange their rungs on a Metropolis coin,
        inside the kernel, so that the chain at the last rung -- the target -- is fed states that crossed between modes
        where it is hot.

        ``betas``: (R,), R in 2..16, rung 0 first (hot) and the target last; a host sequence, array or CPU tensor (checked:
        finite, >= 0).  ``beta_schedule(b_hot, b_target, R)`` builds a geometric or linear ladder.  ``num_sweeps``: default
        the sampler's ``sweeps``.  ``start=None``: fresh chains from the INIT stream, chain c on rung c % R; to continue a
        draw give the ``state`` and ``rungs`` of its :class:`Tempered` as ``start`` ((Q R, n) int8 or float32 +-1) and
        ``rungs`` ((Q R,) integer), both on the device, both or neither.  Returns a :class:`Tempered`; no host sync.

        Its own key ``pt_seed`` and counter ``pt_sweep_count`` (which also numbers the exchanges): the training,
        conditional, annealed and AIS streams are left alone.  Chain ids are ``chain_offset + arange(Q R)``."""
        a = self._tempered_arguments(linear, quadratic, betas, num_ladders, num_sweeps, swap_every, start, rungs)
        return self._tempered_draw(a, prefactor, linear_range, quadratic_range)[0]

    def _tempered_arguments(self, linear, quadratic, betas, num_ladders, num_sweeps, swap_every, start, rungs, traced=False,
                            burn_in=0, thin=1):
        """The argument checks of the exchange draws, every one before the first library call (the ladder's upload included).
        ``traced``: ``burn_in`` and ``thin`` count, checked as :meth:`sample_trace` does.  Returns by name the ``ladder`` (host
        float32), ``R``, ``Q``, the sweeps ``S``, ``swap_every``, ``burn_in``, ``thin``, the records ``M`` (None unless
        ``traced``), ``start``, ``rungs`` and the parameters ``lin``, ``quad``."""
        if torch.is_tensor(betas) and betas.is_cuda:
            raise _lib.DvgError("betas: the ladder is a host sequence, array or CPU tensor (it is checked, then uploaded)")
        ladder = _check_beta_table(betas, "betas")
        if ladder.ndim != 1 or not 2 <= ladder.size <= 16:
            raise _lib.DvgError(f"betas must be (replicas,) with 2 to 16 replicas, got {tuple(ladder.shape)}")
        R, Q, swap_every = int(ladder.size), _whole("num_ladders", num_ladders), _whole("swap_every", swap_every)
        S, M = _whole("num_sweeps", self.sweeps if num_sweeps is None else num_sweeps), None
        if traced:
            burn_in, thin = _whole("burn_in", burn_in, 0), _whole("thin", thin)
            M = (S - burn_in) // thin
            if M < 1:
                raise ValueError(f"num_sweeps={S}, burn_in={burn_in}, thin={thin} record nothing (a draw without a trace is "
                                 "sample_tempered)")
        if (start is None) != (rungs is None):
            raise ValueError("start and rungs go together: give both (to continue a draw) or neither (fresh chains)")
        if start is not None:
            self._check_start(start, count=num_ladders, count_name="num_ladders", per=R, rungs=rungs)
        lin, quad = self._parameters(linear, quadratic, start=start, rungs=rungs)
        return SimpleNamespace(ladder=ladder, R=R, Q=Q, S=S, swap_every=swap_every, burn_in=burn_in, thin=thin, M=M, start=start,
                               rungs=rungs, lin=lin, quad=quad)

    def _tempered_draw(self, a, prefactor, linear_range, quadratic_range, energies=False, rung_walk=False):
        """The exchange draw on checked arguments (:meth:`_tempered_arguments`' ``a``); with records (``a.M``) the traced entry
        point, which takes the same arguments and five more.  Returns ``(Tempered, bits, energies, walk)``: the last three
        are the trace's buffers, None where there is none."""
        n, R, C, dev = self.plan.n, a.R, a.Q * a.R, a.lin.device
        table = torch.from_numpy(a.ladder).to(dev)
        state, init = self._own_chains(a.start, C, dev)
        if a.rungs is None:
            rung = torch.empty((C,), dtype=torch.int32, device=dev)
        else:
            rung = a.rungs.detach().to(torch.int32, copy=True).contiguous()
        out = torch.empty((C, n), dtype=torch.float32, device=dev)
        energy = torch.empty((C,), dtype=torch.float64, device=dev)
        accept = torch.empty((C,), dtype=torch.int32, device=dev)  # (uint32 counts; a draw has fewer than 2^31 exchanges)
        sweep0 = self.pt_sweep_count & 0xFFFFFFFF
        name, bits, e_trace, walk = "dvg_gibbs_sample_tempered", None, None, None
        args = [table.data_ptr(), R, a.swap_every, state.data_ptr(), rung.data_ptr(), C, self.chain_offset & 0xFFFFFFFF, self.pt_seed,
                sweep0, a.S, init, out.data_ptr(), energy.data_ptr(), accept.data_ptr()]
        if a.M is not None:
            name = "dvg_gibbs_sample_tempered_traced"
            bits = torch.empty((a.Q, R, a.M, (n + 31) // 32), dtype=torch.int32, device=dev)
            e_trace = torch.empty((a.Q, R, a.M), dtype=torch.float64, device=dev) if energies else None
            walk = torch.empty((a.Q, R, a.M), dtype=torch.uint8, device=dev) if rung_walk else None
            args += [bits.data_ptr(), _lib.ptr(e_trace), _lib.ptr(walk), a.burn_in, a.thin]
        self._call(name, a.lin, a.quad, prefactor, linear_range, quadratic_range, *args, None)
        self.pt_sweep_count += a.S
        return Tempered.from_draw(n, R, out, energy, accept, sweep0, a.S, a.swap_every, state, rung), bits, e_trace, walk

    def _cluster_arguments(self, state, rungs, replicas, rung_from, move):
        """The argument checks of :meth:`cluster_move`, every one before the first library call.  Returns ``(R, rung_from, move,
        rung)``, ``rung`` the (C,) int32 contiguous table or None."""
        n = self.plan.n
        R = _whole("replicas", replicas)
        if R > 16:
            raise ValueError(f"replicas must be an integer in 1 .. 16, got {replicas!r}")
        rung_from, move = _whole("rung_from", rung_from, 0), _whole("move", move, 0)
        if rung_from >= R:
            raise ValueError(f"rung_from must be an integer in 0 .. {R - 1}, got {rung_from!r}")
        if move >= 2 ** 32:
            raise ValueError(f"move must stay below 2^32, got {move!r}")
        if rungs is None and R > 1:
            raise ValueError(f"replicas={R} ladders need their rungs (only single chains, replicas=1, go without)")
        for name, t in (("state", state),) + ((("rungs", rungs),) if rungs is not None else ()):
            if not torch.is_tensor(t):
                raise _lib.DvgError(f"{name} must be a tensor, got {type(t).__name__}")
        if state.dtype != torch.int8 or not state.is_contiguous():
            raise _lib.DvgError(f"state must be a contiguous int8 tensor (it is changed in place), got {state.dtype}")
        if state.dim() != 2 or state.shape[1] != n or state.shape[0] < 2 or state.shape[0] % (2 * R):
            raise _lib.DvgError(f"state must be (twin pairs x {2 * R}, {n}), got {tuple(state.shape)}")
        C = int(state.shape[0])
        if rungs is not None and (rungs.dtype not in (torch.int32, torch.int64) or tuple(rungs.shape) != (C,)):
            raise _lib.DvgError(f"rungs must be ({C},) int32 or int64, got {tuple(rungs.shape)} {rungs.dtype}")
        _on_gpu("state", state)
        if rungs is not None:
            _on_gpu("rungs", rungs)
            if rungs.device != state.device:
                raise _lib.DvgError(f"rungs is on {rungs.device}, state on {state.device}")
        return R, rung_from, move, None if rungs is None else rungs.detach().to(torch.int32).contiguous()

    def cluster_move(self, state: torch.Tensor, rungs: Optional[torch.Tensor] = None, *, replicas: int = 1, rung_from: int = 0,
                     move: int) -> "ClusterMoves":
        """One isoenergetic cluster move (``dvg_gibbs_cluster_move``, "DVG ICM v1" in include/dvg.h) on ``state`` (C, n) int8
        +-1 on the device, IN PLACE: ladders of R = ``replicas`` consecutive chains, the ladders 2p and 2p + 1 twins; for
        every rung r >= ``rung_from`` the twins' holders of r exchange their spins on one connected cluster of the sites
        where they disagree, rooted at a random such site.  The pair's total energy does not change: no acceptance test.
        ``rungs`` (C,) integer on the device, the rung each chain holds (a :class:`Tempered`'s ``state`` and ``rungs`` fit);
        None with ``replicas=1``: chains 2p and 2p + 1 are twins.  ``move``: the number of the move, the third word of its
        Philox counter -- the same number again undoes the move.  Returns a :class:`ClusterMoves`; no host sync.

        Its key is the exchange draw's ``pt_seed``; no counter advances and no stream of sweeps is touched.  Chain ids are
        ``chain_offset + arange(C)``."""
        R, rung_from, move, rung = self._cluster_arguments(state, rungs, replicas, rung_from, move)
        jobs = int(state.shape[0]) // 2
        sizes = torch.empty((jobs,), dtype=torch.int32, device=state.device)  # (uint32 counts of at most n spins)
        differ = torch.empty((jobs,), dtype=torch.int32, device=state.device)
        with torch.cuda.device(state.device):
            _lib.check(_lib.lib().dvg_gibbs_cluster_move(self.graph.ptr, state.data_ptr(), _lib.ptr(rung), int(state.shape[0]), R,
                                                         rung_from, self.chain_offset & 0xFFFFFFFF, self.pt_seed, move,
                                                         sizes.data_ptr(), differ.data_ptr(), _lib.stream_ptr(state.device)),
                       "dvg_gibbs_cluster_move")
        return ClusterMoves.from_outputs(sizes, differ, R)

    def sample_tempered_cluster(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range,
                                quadratic_range, betas, *, num_ladders: int, num_sweeps: Optional[int] = None, swap_every: int = 1,
                                cluster_every: int, rung_from: int = 0, start: Optional[torch.Tensor] = None,
                                rungs: Optional[torch.Tensor] = None) -> "TemperedCluster":
        """A parallel-tempering draw of TWIN ladders with isoenergetic cluster moves between them: BY DEFINITION a composition
        of :meth:`sample_tempered` calls ("DVG PT v1") and :meth:`cluster_move` calls ("DVG ICM v1") on the exchange draw's key
        ``pt_seed`` and counter ``pt_sweep_count``.  ``num_ladders`` is even: the ladders 2p and 2p + 1 are twins.  In front of
        every sweep of global index t with ``t % cluster_every == 0`` -- the call's first sweep included when ``start`` is
        given, never in front of the first sweep of fresh chains -- move number ``t // cluster_every`` takes place at the rungs
        ``rung_from`` .. R - 1; the sweeps between two moves are one exchange draw that is handed ``state`` and ``rungs``
        (:func:`cluster_schedule` lists the segments).  A call ends on sweeps: the energies are the kernel's own.  One call of
        S sweeps and two calls of S1 + S2 sweeps that hand ``state`` and ``rungs`` on are the same draw, as for
        :meth:`sample_tempered`, whose other arguments and checks these are; every check comes before the first library
        call.  Returns a :class:`TemperedCluster`; no host sync.

        ``pt_sweep_count`` advances by ``num_sweeps``; every other stream and counter is left alone."""
        import copy

        if isinstance(num_ladders, bool) or not isinstance(num_ladders, (int, np.integer)) or num_ladders < 2 or num_ladders % 2:
            raise ValueError(f"num_ladders must be an even integer >= 2 (twin ladders), got {num_ladders!r}")
        every = _whole("cluster_every", cluster_every)
        rung_from = _whole("rung_from", rung_from, 0)
        rungs_of_ladder = int(betas.numel()) if torch.is_tensor(betas) else int(np.size(betas))
        if 2 <= rungs_of_ladder <= rung_from:  # (a ladder of another size is _tempered_arguments' to reject)
            raise ValueError(f"rung_from must be an integer in 0 .. {rungs_of_ladder - 1}, got {rung_from!r}")
        a = self._tempered_arguments(linear, quadratic, betas, num_ladders, num_sweeps, swap_every, start, rungs)
        P = a.Q // 2
        parts, sizes, differ, moves = [], [], [], []
        for move, _first, sweeps in cluster_schedule(self.pt_sweep_count, a.S, every, a.start is None):
            seg = copy.copy(a)
            seg.S = sweeps
            if parts:
                seg.start, seg.rungs = parts[-1].state, parts[-1].rungs
            if move is not None:
                if not parts:
                    seg.start = seg.start.detach().to(torch.int8, copy=True).contiguous()  # (the caller's start stays as it was)
                m = self.cluster_move(seg.start, seg.rungs, replicas=a.R, rung_from=rung_from, move=move & 0xFFFFFFFF)
                sizes.append(m.sizes)
                differ.append(m.differ)
                moves.append(move)
            parts.append(self._tempered_draw(seg, prefactor, linear_range, quadratic_range)[0])
        last, dev = parts[-1], a.lin.device
        total = Tempered(last.samples, last.energies, sum(p.accepted for p in parts[1:]) + parts[0].accepted,
                         sum(p.attempts for p in parts[1:]) + parts[0].attempts, last.state, last.rungs)
        empty = torch.zeros((0, P, a.R), dtype=torch.int64, device=dev)
        return TemperedCluster(total, torch.stack(sizes) if sizes else empty, torch.stack(differ) if differ else empty.clone(),
                               np.asarray(moves, dtype=np.int64))

    def sample_tempered_trace(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range,
                              quadratic_range, betas, *, num_ladders: int, num_sweeps: Optional[int] = None, swap_every: int = 1,
                              burn_in: int = 0, thin: int = 1, start: Optional[torch.Tensor] = None,
                              rungs: Optional[torch.Tensor] = None, energies: bool = True, rung_walk: bool = True) -> "TemperedTrace":
        """A traced parallel-tempering draw (``dvg_gibbs_sample_tempered_traced``, "DVG PT trace v1" in include/dvg.h):
        :meth:`sample_tempered` -- the same draw, bit for bit -- with a history of the ladders written from inside the
        kernel: after every ``thin``-th sweep behind the first ``burn_in`` (sweep k iff ``k + 1 > burn_in`` and
        ``(k + 1 - burn_in) % thin == 0``, M = ``(num_sweeps - burn_in) // thin`` records), and after the exchange that
        follows such a sweep, per rung the packed state and (``energies``) the carried energy of the chain that holds it,
        and (``rung_walk``) per chain the rung it holds.

        The arguments and their checks are :meth:`sample_tempered`'s and :meth:`sample_trace`'s, all before the first
        library call.  Returns a :class:`TemperedTrace`; no host sync.

        The stream is :meth:`sample_tempered`'s: the key ``pt_seed``, and ``pt_sweep_count`` advances by ``num_sweeps``;
        every other stream and counter is left alone."""
        a = self._tempered_arguments(linear, quadratic, betas, num_ladders, num_sweeps, swap_every, start, rungs, traced=True,
                                     burn_in=burn_in, thin=thin)
        final, bits, e_trace, walk = self._tempered_draw(a, prefactor, linear_range, quadratic_range, bool(energies), bool(rung_walk))
        return TemperedTrace(bits, e_trace, walk, trace_sweeps(a.S, a.burn_in, a.thin), final, a.ladder, self.plan.n)

    def sample_trace(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range, quadratic_range, *,
                     num_reads: Optional[int] = None, start: Optional[torch.Tensor] = None, num_sweeps: Optional[int] = None,
                     burn_in: int = 0, thin: int = 1) -> "Trace":
        """A traced draw (``dvg_gibbs_sample_traced``, "DVG trace v1" in include/dvg.h): ``num_sweeps`` (default: the
        sampler's ``sweeps``) sweeps at the sampler's ``beta``, with the chains' states written out from inside the kernel
        after every ``thin``-th sweep behind the first ``burn_in`` -- sweep k (0-based) iff ``k + 1 > burn_in`` and
        ``(k + 1 - burn_in) % thin == 0``, M = ``(num_sweeps - burn_in) // thin`` records of n / 8 bytes per chain.

        ``start=None``: ``num_reads`` fresh chains from the INIT stream; ``start`` (C, n) int8 or float32 +-1 on the device:
        the chains begin at the call's own copy of it.  Returns a :class:`Trace`; no host sync.

        Its own key ``trace_seed`` and counter ``trace_sweep_count``: the training, conditional, annealed, AIS and exchange
        streams, the persistent chains, ``sweep_count`` and ``calls`` are left alone.  Chain ids are ``chain_offset +
        arange(C)``."""
        n = self.plan.n
        # every argument check comes before the first library call
        S = _whole("num_sweeps", self.sweeps if num_sweeps is None else num_sweeps)
        burn_in, thin = _whole("burn_in", burn_in, 0), _whole("thin", thin)
        M = (S - burn_in) // thin
        if M < 1:
            raise ValueError(f"num_sweeps={S}, burn_in={burn_in}, thin={thin} record nothing (a draw without a trace is sample_native)")
        if start is not None:
            C = self._check_start(start, count=num_reads)
        elif num_reads is not None:
            C = _whole("num_reads", num_reads)
        else:
            raise ValueError("a traced draw needs num_reads (fresh chains) or start to know how many chains to draw")
        lin, quad = self._parameters(linear, quadratic, start=start)
        state, init = self._own_chains(start, C, lin.device)
        out = torch.empty((C, n), dtype=torch.float32, device=lin.device)
        bits = torch.empty((C, M, (n + 31) // 32), dtype=torch.int32, device=lin.device)
        self._call("dvg_gibbs_sample_traced", lin, quad, prefactor, linear_range, quadratic_range, self.beta, state.data_ptr(), C,
                   self.chain_offset & 0xFFFFFFFF, self.trace_seed, self.trace_sweep_count & 0xFFFFFFFF, S, init, out.data_ptr(),
                   bits.data_ptr(), burn_in, thin, None)
        self.trace_sweep_count += S
        return Trace(bits, out, state, trace_sweeps(S, burn_in, thin), n)

    def sample_quantum(self, linear: torch.Tensor, quadratic: torch.Tensor, prefactor: float, linear_range, quadratic_range,
                       beta_slice, kappa, *, slices: int, num_reads: Optional[int] = None,
                       start: Optional[torch.Tensor] = None) -> "Sliced":
        """A simulated-quantum-annealing draw (``dvg_gibbs_sample_quantum``, "DVG SQA v1" in include/dvg.h): chains of
        ``slices`` = P Trotter slices of the n spins (P a power of two in 2 .. 64), Gibbs-sampled for S sweeps under
        ``p(s) ~ exp(-beta_slice[k] sum_slices E + kappa[k] sum s[slice][i] s[slice + 1][i])`` in sweep k -- path-integral
        Monte Carlo of the transverse-field Ising model; :func:`transverse_schedule` makes the two tables from a field
        schedule.  ``beta_slice``, ``kappa``: (S,) each, host sequences, arrays or CPU tensors (checked here: finite, >= 0,
        equal length; then uploaded) or CUDA float32 tensors, used as they are.  ``start=None``: ``num_reads`` fresh chains
        from the INIT stream; ``start`` (C, P, W) int32 on the device (a :class:`Sliced`'s ``bits``): the chains continue
        from the call's own copy of it.  Returns a :class:`Sliced`; no host sync.

        Its own key ``sqa_seed`` and counter ``sqa_sweep_count``: every other stream, the persistent chains, ``sweep_count``
        and ``calls`` are left alone.  Chain ids are ``chain_offset + arange(C)``."""
        n = self.plan.n
        W = (n + 31) // 32
        # every argument check comes before the first library call (the tables' upload included)
        P = _slice_count(slices)
        if start is not None:
            if not torch.is_tensor(start):
                raise _lib.DvgError(f"start must be a tensor, got {type(start).__name__}")
            if start.dtype != torch.int32:
                raise _lib.DvgError(f"start must be int32 packed slices, got {start.dtype}")
            if start.dim() != 3 or start.shape[0] < 1 or tuple(start.shape[1:]) != (P, W):
                raise _lib.DvgError(f"start must be (chains, {P}, {W}), got {tuple(start.shape)}")
            C = int(start.shape[0])
            if num_reads is not None and num_reads != C:
                raise _lib.DvgError(f"num_reads={num_reads!r} but start has {C} chains")
            _on_gpu("start", start)
        elif num_reads is not None:
            C = _whole("num_reads", num_reads)
        else:
            raise ValueError("a quantum draw needs num_reads (fresh chains) or start to know how many chains to draw")
        if C * P >= 2 ** 31:
            raise ValueError(f"num_reads={C} x slices={P} must stay below 2^31")
        hosts = [_check_beta_table(t, name) for name, t in (("beta_slice", beta_slice), ("kappa", kappa))]
        lengths = [int(np.shape(t)[-1]) if h is None else int(h.shape[-1]) for t, h in zip((beta_slice, kappa), hosts)]
        if lengths[0] != lengths[1]:
            raise ValueError(f"beta_slice has {lengths[0]} sweeps, kappa {lengths[1]}: an entry of each per sweep")
        lin, quad = self._parameters(linear, quadratic, start=start, beta_slice=beta_slice, kappa=kappa)
        tb = _beta_table(beta_slice, lin.device, "beta_slice")
        tk = _beta_table(kappa, lin.device, "kappa")
        S = lengths[0]
        if start is None:
            bits, init = torch.empty((C, P, W), dtype=torch.int32, device=lin.device), 1
        else:
            bits, init = start.detach().clone(memory_format=torch.contiguous_format), 0
        out = torch.empty((C, n), dtype=torch.float32, device=lin.device)
        self._call("dvg_gibbs_sample_quantum", lin, quad, prefactor, linear_range, quadratic_range, tb.data_ptr(), tk.data_ptr(),
                   bits.data_ptr(), C, P, self.chain_offset & 0xFFFFFFFF, self.sqa_seed, self.sqa_sweep_count & 0xFFFFFFFF, S, init,
                   out.data_ptr())
        self.sqa_sweep_count += S
        return Sliced(bits, out, n)

    # -- dimod-style entry point -----------------------------------------------------------
    def sample_ising(self, h: Dict, J: Dict, num_reads: int = 1, answer_mode: str = "raw", auto_scale: bool = False,
                     annealing_time: float = 1.0, label: str = "", beta_schedule=None, beta_range=None,
                     num_sweeps: Optional[int] = None, beta_schedule_type: str = "geometric", transverse_field_range=None,
                     num_slices: Optional[int] = None, **_unused) -> SampleSet:
        """Same call the reference makes on its QPU sampler (kwargs built at
        /root/reference/src/utils/common.py:130-138).  ``h``/``J`` are already
        scaled by the prefactor and clamped by the caller (plugin ``to_ising``).

        Annealed reads, under ``neal.SimulatedAnnealingSampler``'s names: ``beta_range=(hot, target)`` with
        ``num_sweeps`` (default: the sampler's ``sweeps``) and ``beta_schedule_type`` "geometric" / "linear", or an
        explicit ``beta_schedule`` ((S,) or (num_reads, S); ``beta_schedule_type`` may then be "custom").  Either one
        draws ``num_reads`` FRESH chains through :meth:`sample_annealed` (its key and counter; the persistent chains
        are left alone).  ``annealing_time`` is accepted, as the reference passes it, and unused: nothing maps a QPU's
        microseconds to a schedule.

        Simulated-quantum-annealing reads: ``transverse_field_range=(Gamma_start, Gamma_end)`` with ``num_slices`` Trotter
        slices and ``num_sweeps`` (default: the sampler's ``sweeps``) build the linear :func:`transverse_schedule` at the
        sampler's ``beta`` and return slice 0 of ``num_reads`` FRESH chains of :meth:`sample_quantum` (its key and counter);
        they do not go together with ``beta_range`` / ``beta_schedule``.

        The returned set carries the per-read Ising energy ``h.s + sum J s_i s_j`` of the ``(h, J)`` given, computed on
        the device (``dvg_grbm_energy``) and brought to the host when ``.record`` is read.

        ``answer_mode="histogram"`` (a D-Wave sampler's own default) returns every distinct read once, with
        ``record.num_occurrences``, by rising energy and ties by first occurrence (:meth:`SampleSet.aggregate` of the raw
        reads; the energy is that of the first copy).  ``"raw"``, which the reference passes, and every other value return
        the reads as drawn."""
        if auto_scale:
            raise ValueError("auto_scale=True is not supported: the sampler draws from the distribution it is given")
        betas = tables = None
        if transverse_field_range is not None or num_slices is not None:
            if beta_schedule is not None or beta_range is not None:
                raise ValueError("transverse_field_range / num_slices (a quantum draw) do not go with beta_range / beta_schedule "
                                 "(an annealed one)")
            if transverse_field_range is None or num_slices is None:
                raise ValueError("a quantum draw needs both transverse_field_range and num_slices")
            try:
                g0, g1 = transverse_field_range
            except (TypeError, ValueError):
                raise ValueError(f"transverse_field_range must be (gamma_start, gamma_end), got {transverse_field_range!r}") from None
            _whole("num_reads", num_reads)
            tables = transverse_schedule(self.beta, g0, g1, self.sweeps if num_sweeps is None else num_sweeps, num_slices)
        elif beta_schedule is not None:
            if beta_range is not None:
                raise ValueError("give beta_schedule or beta_range, not both")
            if beta_schedule_type not in ("custom", "geometric", "linear"):
                raise ValueError(f"beta_schedule_type must be 'geometric', 'linear' or 'custom', got {beta_schedule_type!r}")
            betas = beta_schedule
        elif beta_range is not None:
            if beta_schedule_type not in ("geometric", "linear"):
                raise ValueError(f"beta_schedule_type must be 'geometric' or 'linear' with beta_range, got {beta_schedule_type!r}")
            try:
                b0, b1 = beta_range
            except (TypeError, ValueError):
                raise ValueError(f"beta_range must be (beta_start, beta_end), got {beta_range!r}") from None
            betas = _make_beta_schedule(b0, b1, self.sweeps if num_sweeps is None else num_sweeps, beta_schedule_type)
        elif num_sweeps is not None:
            raise ValueError("num_sweeps needs beta_range (or a beta_schedule): a fixed-beta draw runs the sampler's own sweeps")
        if betas is not None:
            _check_beta_table(betas, "beta_schedule", rows=_whole("num_reads", num_reads))  # (before anything is built or uploaded)
            if num_sweeps is not None and beta_schedule is not None and int(num_sweeps) != int(np.shape(betas)[-1]):
                raise ValueError(f"num_sweeps={num_sweeps} does not match the beta_schedule given ({np.shape(betas)[-1]} sweeps)")
        idx = {v: k for k, v in enumerate(self.nodes)}
        lin = torch.zeros(self.plan.n, dtype=torch.float32)
        for v, val in h.items():
            lin[idx[v]] = float(val)
        edge_pos = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(self.plan.edge_i, self.plan.edge_j))}
        quad = torch.zeros(self.plan.n_edges, dtype=torch.float32)
        for (a, b), val in J.items():
            ia, ib = idx[a], idx[b]
            key = (min(ia, ib), max(ia, ib))
            if key not in edge_pos:
                raise ValueError(f"coupler {(a, b)} is not an edge of the sampler's graph")
            quad[edge_pos[key]] = float(val)
        dev = self.device
        lin, quad = lin.to(dev), quad.to(dev)
        if tables is not None:
            t = self.sample_quantum(lin, quad, 1.0, None, None, *tables, slices=num_slices, num_reads=num_reads).samples
        elif betas is None:
            t = self.sample_native(lin, quad, 1.0, None, None, num_reads)
        else:
            t = self.sample_annealed(lin, quad, 1.0, None, None, betas, num_reads=num_reads)
        from . import functional as F  # (functional imports this module)

        with torch.no_grad():
            energy = F.grbm_energy(t, lin, quad, self.graph)
        raw = SampleSet(None, self.nodes, energy=None, device_tensor=t, device_energy=energy)
        if isinstance(answer_mode, str) and answer_mode == "histogram":
            return raw.aggregate()._sorted_by_energy()
        return raw


def get_sampler_and_sampler_kwargs(num_reads: int, annealing_time: float, n_latents: int, random_seed: int, qpu: str,
                                   *, sweeps: int = 50, beta: Optional[float] = None, prefactor: float = 0.05,
                                   persistent: bool = True, device="cuda", chain_offset: int = 0,
                                   graph: Optional[nx.Graph] = None):
    """Local-solver counterpart of /root/reference/src/utils/common.py:103-140.

    Returns the same 5-tuple ``(sampler, sampler_kwargs, mapped_graph, linear_range, quadratic_range)``.
    ``qpu`` names a topology in ``graphs.LOCAL_SOLVERS`` (the three QPU names of the shipped
    checkpoints are accepted and map to the ideal Pegasus P16 / Zephyr Z12 graph).
    """
    if qpu not in LOCAL_SOLVERS:
        raise ValueError(f"unknown local solver {qpu!r}; known: {sorted(LOCAL_SOLVERS)}")
    make, h_range, j_range = LOCAL_SOLVERS[qpu]
    full = graph if graph is not None else make()
    sub = greedy_get_subgraph(n_nodes=n_latents, random_seed=random_seed, graph=full)
    mapped, _mapping = get_graph_mapping(sub)
    nodes, ei, ej = edges_of(mapped)
    plan = build_plan(len(nodes), ei, ej)
    sampler = GibbsSampler(plan, nodes, beta=(1.0 / prefactor) if beta is None else beta, sweeps=sweeps,
                           seed=random_seed, persistent=persistent, device=device, chain_offset=chain_offset,
                           h_range=h_range, j_range=j_range)
    sampler_kwargs = dict(num_reads=num_reads, answer_mode="raw", auto_scale=False, annealing_time=annealing_time,
                          label="Examples - ML MNIST Image Gen")
    return sampler, sampler_kwargs, mapped, tuple(h_range), tuple(j_range)
