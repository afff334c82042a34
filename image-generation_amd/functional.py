"""torch.autograd glue over the C ABI: each Function calls one fused HIP entry
point for forward (+ saved quantities) and one for backward.  torch only owns
the memory and the stream.  No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import collections
import ctypes
import numbers
from typing import Optional

import torch

from . import _lib
from ._lib import MmdCfg, check, lib, require_cuda, stream_ptr

GUMBEL_TAU = 1.0 / 7.0


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ----------------------------------------------------------------------------- MMD


class _MMD(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, n_kernels, factor, bandwidth, squared, reduce_mean, biased):
        L = lib()
        xd = require_cuda(x.detach().float().contiguous(), "x")
        yd = require_cuda(y.detach().float().contiguous(), "y")
        if xd.dim() != 2 or yd.dim() != 2 or xd.shape[1] != yd.shape[1]:
            raise ValueError("maximum_mean_discrepancy_loss expects x (nx, d) and y (ny, d)")
        nx, d = xd.shape
        ny = yd.shape[0]
        cfg = MmdCfg(int(n_kernels), float(factor), float(bandwidth if bandwidth is not None else -1.0),
                     int(bool(squared)), int(bool(reduce_mean)), int(bool(biased)))
        need_grad = x.requires_grad
        loss = torch.empty((), dtype=torch.float32, device=xd.device)
        grad = torch.empty_like(xd) if need_grad else None
        nbytes = L.dvg_mmd_workspace_bytes(nx, ny, d)
        if nbytes == 0:
            raise _lib.DvgError(f"MMD: unsupported shape nx={nx} ny={ny} d={d} (d must be a multiple of 32)")
        ws = _ws(nbytes, xd.device)
        with torch.cuda.device(xd.device):
            check(L.dvg_mmd_fwd_bwd(xd.data_ptr(), nx, yd.data_ptr(), ny, d, ctypes.byref(cfg), loss.data_ptr(),
                                    _lib.ptr(grad), ws.data_ptr(), ws.numel(), stream_ptr(xd.device)), "dvg_mmd_fwd_bwd")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None, None, None, None, None, None, None, None)


def mmd_loss(x, y, n_kernels=7, factor=2.0, bandwidth=None, squared=False, reduce_mean=False, biased=False):
    return _MMD.apply(x, y, n_kernels, factor, bandwidth, squared, reduce_mean, biased)


def mmd_loss_and_grad(x, y, n_kernels=7, factor=2.0, bandwidth=None, squared=False, reduce_mean=False, biased=False):
    """(loss, d loss / d x) from the one fused call, outside autograd: for callers that seed the backward pass
    themselves (``torch.autograd.backward(x, grad)``) instead of paying a ones_like + multiply per loss term."""
    L = lib()
    xd = require_cuda(x.detach().float().contiguous(), "x")
    yd = require_cuda(y.detach().float().contiguous(), "y")
    if xd.dim() != 2 or yd.dim() != 2 or xd.shape[1] != yd.shape[1]:
        raise ValueError("maximum_mean_discrepancy_loss expects x (nx, d) and y (ny, d)")
    nx, d = xd.shape
    ny = yd.shape[0]
    cfg = MmdCfg(int(n_kernels), float(factor), float(bandwidth if bandwidth is not None else -1.0),
                 int(bool(squared)), int(bool(reduce_mean)), int(bool(biased)))
    loss = torch.empty((), dtype=torch.float32, device=xd.device)
    grad = torch.empty_like(xd)
    nbytes = L.dvg_mmd_workspace_bytes(nx, ny, d)
    if nbytes == 0:
        raise _lib.DvgError(f"MMD: unsupported shape nx={nx} ny={ny} d={d} (d must be a multiple of 32)")
    ws = _ws(nbytes, xd.device)
    with torch.cuda.device(xd.device):
        check(L.dvg_mmd_fwd_bwd(xd.data_ptr(), nx, yd.data_ptr(), ny, d, ctypes.byref(cfg), loss.data_ptr(),
                                grad.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(xd.device)), "dvg_mmd_fwd_bwd")
    return loss, grad


# ----------------------------------------------------------------------------- latent -> discrete


class _Gumbel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, n_samples, tau, gumbels, seed, offset):
        L = lib()
        lg = require_cuda(logits.detach().float().contiguous(), "logits")
        B, n = lg.shape
        R = int(n_samples)
        spins = torch.empty((B, R, n), dtype=torch.float32, device=lg.device)
        dspin = torch.empty_like(spins)
        gb = None
        if gumbels is not None:
            gb = require_cuda(gumbels.detach().float().contiguous(), "gumbels")
            if tuple(gb.shape) != (B, R, n, 2):
                raise ValueError(f"gumbels must have shape {(B, R, n, 2)}, got {tuple(gb.shape)}")
        with torch.cuda.device(lg.device):
            check(L.dvg_gumbel_fwd(lg.data_ptr(), B, n, R, float(tau), _lib.ptr(gb), int(seed) & (2**64 - 1),
                                   int(offset) & (2**64 - 1), spins.data_ptr(), dspin.data_ptr(), _lib.DYN,
                                   stream_ptr(lg.device)),
                  "dvg_gumbel_fwd")
        ctx.save_for_backward(dspin)
        ctx.shape = (B, n, R)
        return spins

    @staticmethod
    def backward(ctx, gs):
        (dspin,) = ctx.saved_tensors
        B, n, R = ctx.shape
        gs = gs.contiguous()
        gl = torch.empty((B, n), dtype=torch.float32, device=gs.device)
        with torch.cuda.device(gs.device):
            check(lib().dvg_gumbel_bwd(gs.data_ptr(), dspin.data_ptr(), B, n, R, gl.data_ptr(), stream_ptr(gs.device)),
                  "dvg_gumbel_bwd")
        return gl, None, None, None, None, None


def gumbel_latent_to_discrete(logits, n_samples, gumbels=None, tau=GUMBEL_TAU, seed=0, offset=0):
    return _Gumbel.apply(logits, n_samples, tau, gumbels, seed, offset)


def gumbel_forward_raw(logits, n_samples, gumbels=None, tau=GUMBEL_TAU, seed=0, offset=0):
    """``(spins (B,R,n), dspin (B,R,n))`` outside autograd, for callers that run the backward themselves
    (:func:`gumbel_backward`): the training step feeds it the SUM of two spin gradients in one kernel."""
    L = lib()
    lg = require_cuda(logits.detach().float().contiguous(), "logits")
    B, n = lg.shape
    R = int(n_samples)
    spins = torch.empty((B, R, n), dtype=torch.float32, device=lg.device)
    dspin = torch.empty_like(spins)
    gb = None
    if gumbels is not None:
        gb = require_cuda(gumbels.detach().float().contiguous(), "gumbels")
        if tuple(gb.shape) != (B, R, n, 2):
            raise ValueError(f"gumbels must have shape {(B, R, n, 2)}, got {tuple(gb.shape)}")
    with torch.cuda.device(lg.device):
        check(L.dvg_gumbel_fwd(lg.data_ptr(), B, n, R, float(tau), _lib.ptr(gb), int(seed) & (2**64 - 1),
                               int(offset) & (2**64 - 1), spins.data_ptr(), dspin.data_ptr(), _lib.DYN,
                               stream_ptr(lg.device)), "dvg_gumbel_fwd")
    return spins, dspin


def gumbel_backward(dspin, grad_spins, grad_spins2=None):
    """``d loss / d logits (B,n) = sum_r (grad_spins + grad_spins2) * dspin``: one kernel, no separate add pass."""
    B, R, n = dspin.shape
    g1 = require_cuda(grad_spins.detach().float().contiguous(), "grad_spins")
    g2 = None if grad_spins2 is None else require_cuda(grad_spins2.detach().float().contiguous(), "grad_spins2")
    if g1.numel() != dspin.numel() or (g2 is not None and g2.numel() != dspin.numel()):
        raise ValueError("gumbel_backward: gradients must have the spins' shape")
    gl = torch.empty((B, n), dtype=torch.float32, device=dspin.device)
    with torch.cuda.device(dspin.device):
        check(lib().dvg_gumbel_bwd2(g1.data_ptr(), _lib.ptr(g2), dspin.data_ptr(), B, n, R, gl.data_ptr(),
                                    stream_ptr(dspin.device)), "dvg_gumbel_bwd2")
    return gl


def scalar_add(a, b):
    """``a + b`` of two device scalars by the library (the step's ``mse + mmd``)."""
    a = require_cuda(a.detach().float().reshape(()), "a")
    b = require_cuda(b.detach().float().reshape(()), "b")
    out = torch.empty((), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().dvg_scalar_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), stream_ptr(a.device)), "dvg_scalar_add")
    return out


class _Heaviside(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        lg = require_cuda(logits.detach().float().contiguous(), "logits")
        out = torch.empty_like(lg)
        with torch.cuda.device(lg.device):
            check(lib().dvg_heaviside_fwd(lg.data_ptr(), lg.numel(), out.data_ptr(), stream_ptr(lg.device)),
                  "dvg_heaviside_fwd")
        return out.unsqueeze(1)

    @staticmethod
    def backward(ctx, g):
        return g.squeeze(1)  # straight-through identity (/root/reference/src/utils/common.py:173)


def heaviside_latent_to_discrete(logits, n_samples=1):
    return _Heaviside.apply(logits)


# ----------------------------------------------------------------------------- GRBM energy


class _Energy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, linear, quadratic, graph):
        L = lib()
        xd = require_cuda(x.detach().float().contiguous(), "x")
        lin = require_cuda(linear.detach(), "linear")
        quad = require_cuda(quadratic.detach(), "quadratic")
        n = xd.shape[-1]
        rows = xd.numel() // n
        out = torch.empty(xd.shape[:-1], dtype=torch.float32, device=xd.device)
        with torch.cuda.device(xd.device):
            check(L.dvg_grbm_energy(graph.ptr, xd.data_ptr(), rows, lin.data_ptr(), quad.data_ptr(), out.data_ptr(),
                                    stream_ptr(xd.device)), "dvg_grbm_energy")
        ctx.graph = graph
        ctx.save_for_backward(xd)
        ctx.needs = (x.requires_grad, linear.requires_grad or quadratic.requires_grad)
        ctx.meta = (linear.shape, quadratic.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        (xd,) = ctx.saved_tensors
        if ctx.needs[0]:
            raise NotImplementedError("gradient of the GRBM energy wrt its input spins is not on the hot path "
                                      "(the reference detaches them: /root/reference/src/model_wrapper.py:333)")
        L = lib()
        n = xd.shape[-1]
        rows = xd.numel() // n
        gw = g.contiguous().float().reshape(-1)
        gl = torch.empty(ctx.meta[0], dtype=torch.float32, device=xd.device)
        gq = torch.empty(ctx.meta[1], dtype=torch.float32, device=xd.device)
        ws = _ws(L.dvg_grbm_suffstats_workspace_bytes(ctx.graph.ptr), xd.device)
        with torch.cuda.device(xd.device):
            check(L.dvg_grbm_suffstats(ctx.graph.ptr, xd.data_ptr(), rows, gw.data_ptr(), 1.0, gl.data_ptr(),
                                       gq.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream_ptr(xd.device)),
                  "dvg_grbm_suffstats")
        return None, gl, gq, None


def grbm_energy(x, linear, quadratic, graph):
    return _Energy.apply(x, linear, quadratic, graph)


def grbm_moments_packed(bits, graph, out=None):
    """Exact integer moments of bit-packed +-1 rows (``dvg_grbm_moments_packed``): ``bits`` (rows, W) int32 on the device in
    the layout of a traced draw (``sampler.Trace.bits``, ``sampler.pack_spins``; bits of spins >= n are ignored), ``graph``
    a ``GraphHandle``.  Returns ``(spin_sum (n,), pair_sum (E,))`` int64: the sums over the rows of s_i and, per edge, of
    s_i s_j.  ``out``: such a pair to add onto instead.  No host sync."""
    n, E = int(graph.plan.n), int(graph.plan.n_edges)
    if not torch.is_tensor(bits) or bits.dtype != torch.int32 or bits.dim() != 2 or bits.shape[1] != (n + 31) // 32 or bits.shape[0] < 1:
        raise _lib.DvgError(f"bits must be (rows >= 1, {(n + 31) // 32}) int32, got "
                            f"{tuple(bits.shape) if torch.is_tensor(bits) else type(bits).__name__}")
    bd = require_cuda(bits.detach(), "bits")
    if out is None:
        spin_sum = torch.empty((n,), dtype=torch.int64, device=bd.device)
        pair_sum = torch.empty((E,), dtype=torch.int64, device=bd.device)
    else:
        spin_sum, pair_sum = out
        for name, t, k in (("spin_sum", spin_sum, n), ("pair_sum", pair_sum, E)):
            if t.dtype != torch.int64 or tuple(t.shape) != (k,) or not t.is_contiguous() or t.device != bd.device:
                raise _lib.DvgError(f"out: {name} must be a contiguous ({k},) int64 tensor on {bd.device}")
    with torch.cuda.device(bd.device):
        check(lib().dvg_grbm_moments_packed(graph.ptr, bd.data_ptr(), int(bd.shape[0]), spin_sum.data_ptr(),
                                            pair_sum.data_ptr() if E else spin_sum.data_ptr(), int(out is not None),
                                            stream_ptr(bd.device)), "dvg_grbm_moments_packed")
    return spin_sum, pair_sum


def trace_autocorr(bits, n, max_lag, *, chain_sums=True, out=None):
    """Exact autocorrelation sums of a bit-packed trace (``dvg_trace_autocorr``, "DVG acf v1"): ``bits`` (C, M, W) int32 on
    the device in the layout of a traced draw (``sampler.Trace.bits``; bits of spins >= n are ignored), ``n`` the spin count,
    ``max_lag`` = L in 0 .. M - 1.  Returns ``(lag_sum (L + 1, n) int64, spin_sum (n,) int64, chain_sum (C, n) int32)``: per
    spin the sums over chains of s(m) s(m + t) over the M - t pairs of lag t, of s(m), and per chain of s(m);
    ``chain_sums=False`` leaves the last out (None).  ``out``: a pair ``(lag_sum, spin_sum)`` to add onto instead (pooling
    traces; ``chain_sum`` is always this trace's own).  ``sampler.Autocorrelation.from_sums`` turns them into estimates.  No
    host sync."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError(f"n must be an integer >= 1, got {n!r}")
    n = int(n)
    W = (n + 31) // 32
    if not torch.is_tensor(bits) or bits.dtype != torch.int32 or bits.dim() != 3 or bits.shape[2] != W or bits.shape[0] < 1 or \
            bits.shape[1] < 1:
        raise _lib.DvgError(f"bits must be (chains >= 1, records >= 1, {W}) int32, got "
                            f"{(tuple(bits.shape), bits.dtype) if torch.is_tensor(bits) else type(bits).__name__}")
    C, M = int(bits.shape[0]), int(bits.shape[1])
    if isinstance(max_lag, bool) or not isinstance(max_lag, numbers.Integral) or not 0 <= max_lag < M:
        raise ValueError(f"max_lag must be an integer in 0 .. {M - 1} (records - 1), got {max_lag!r}")
    max_lag = int(max_lag)
    bd = require_cuda(bits.detach(), "bits")
    if out is None:
        lag_sum = torch.empty((max_lag + 1, n), dtype=torch.int64, device=bd.device)
        spin_sum = torch.empty((n,), dtype=torch.int64, device=bd.device)
    else:
        lag_sum, spin_sum = out
        for name, t, shape in (("lag_sum", lag_sum, (max_lag + 1, n)), ("spin_sum", spin_sum, (n,))):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or \
                    t.device != bd.device:
                raise _lib.DvgError(f"out: {name} must be a contiguous {shape} int64 tensor on {bd.device}")
    chain_sum = torch.empty((C, n), dtype=torch.int32, device=bd.device) if chain_sums else None
    with torch.cuda.device(bd.device):
        check(_lib.lib().dvg_trace_autocorr(bd.data_ptr(), C, M, n, max_lag, lag_sum.data_ptr(), spin_sum.data_ptr(),
                                            chain_sum.data_ptr() if chain_sums else None, int(out is not None),
                                            stream_ptr(bd.device)), "dvg_trace_autocorr")
    return lag_sum, spin_sum, chain_sum


def _packed_rows(t, name, W, groups_first=True):
    """``(rows, row_stride, groups, group_stride)`` of a 2-D (rows, W) or 3-D (C, M, W) int32 tensor of packed rows, in words.
    A 3-D tensor is C groups of M rows -- a trace's chains, pooled -- or with ``groups_first=False`` M groups of C rows:
    :func:`packed_overlap`'s chains at equal times."""
    if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() not in (2, 3) or t.shape[-1] != W or min(t.shape) < 1:
        raise _lib.DvgError(f"{name} must be (rows >= 1, {W}) or (chains >= 1, records >= 1, {W}) int32, got "
                            f"{(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__}")
    if W > 1 and t.stride(-1) != 1:
        raise _lib.DvgError(f"{name}: the last dimension must have stride 1, got strides {tuple(t.stride())}")
    rd, gd = (t.dim() - 2, 0) if groups_first else (0, 1)
    rows = int(t.shape[rd])
    rs = int(t.stride(rd)) if rows > 1 else W
    groups = int(t.shape[gd]) if t.dim() == 3 else 1
    gs = int(t.stride(gd)) if groups > 1 else 0
    if rs < W or gs < 0:
        raise _lib.DvgError(f"{name}: a row stride of {rs} words is less than the {W} words of a row (strides {tuple(t.stride())})")
    return rows, rs, groups, gs


def _model_arguments(graph, linear, quadratic, prefactor, linear_range, quadratic_range):
    """The early checks of a model's ``linear`` (n) and ``quadratic`` (E) float32 tensors and ``prefactor``;
    ``(h_lo, h_hi, j_lo, j_hi)`` of the two ranges."""
    for name, t, k in (("linear", linear, int(graph.plan.n)), ("quadratic", quadratic, int(graph.plan.n_edges))):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != k:
            raise _lib.DvgError(f"{name} must be a float32 tensor of the graph's {k} values, got "
                                f"{(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__}")
    if isinstance(prefactor, bool) or not isinstance(prefactor, numbers.Real) or not float("-inf") < prefactor < float("inf"):
        raise ValueError(f"prefactor must be a finite number, got {prefactor!r}")
    return _clamp_range(linear_range, "linear_range") + _clamp_range(quadratic_range, "quadratic_range")


def _on_the_device(bits, linear, quadratic):
    """The late checks, behind every other argument error: ``bits`` on the GPU, the model on its device.  Returns the three
    detached, the model's two contiguous."""
    if not bits.is_cuda:
        raise _lib.DvgError(f"bits must live on the GPU (got {bits.device}); the HIP path has no CPU fallback")
    for name, t in (("linear", linear), ("quadratic", quadratic)):
        if t.device != bits.device:
            raise _lib.DvgError(f"{name} must be on the device of bits ({bits.device}), got {t.device}")
    return bits.detach(), linear.detach().contiguous(), quadratic.detach().contiguous()


def packed_overlap(a, b=None, *, n, nearest=False, out=None):
    """Exact Hamming-distance histogram and nearest rows of bit-packed +-1 rows (``dvg_packed_overlap``, "DVG overlap v1").
    ``a``: (rows, W) or (C, M, W) int32 on the device (``sampler.pack_spins``, ``sampler.Trace.bits``; bits of spins >= n are
    ignored); the 3-D form is M groups of C rows -- a trace's chains at equal times.  ``b``: None -- self mode, the unordered
    pairs r < r' of ``a`` within each group -- or 2-D (with a 3-D ``a``: shared by every group) or 3-D with the same M: all
    pairs (row of a, row of b).  The last dimension must have stride 1; row and group strides are taken from the tensors, so
    slices need no copy.  Returns ``(hist (n + 1,) int64, nearest)``: ``hist[d]`` pairs at distance d over all groups (the
    overlap is q = 1 - 2 d / n: ``sampler.Overlap.from_hist``); ``nearest`` None, or with ``nearest=True`` a pair ``(dist,
    row)`` of int32 tensors shaped (rows,) or (M, C): every row's smallest distance to a row of ``b`` (self mode: to another
    row of ``a``) and the smallest row index that attains it, -1 where there is no partner.  ``out``: a histogram to add
    onto.  No host sync."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError(f"n must be an integer >= 1, got {n!r}")
    n = int(n)
    W = (n + 31) // 32
    rows_a, a_rs, groups, a_gs = _packed_rows(a, "a", W, groups_first=False)
    rows_b, b_rs, b_gs = 0, 0, 0
    if b is not None:
        rows_b, b_rs, groups_b, b_gs = _packed_rows(b, "b", W, groups_first=False)
        if b.dim() == 3 and (a.dim() != 3 or groups_b != groups):
            raise _lib.DvgError(f"b: a 3-D b needs a 3-D a with the same number of records, got a {tuple(a.shape)} and b {tuple(b.shape)}")
        if b.dim() == 2:
            b_gs = 0
        if b.device != a.device:
            raise _lib.DvgError(f"b must be on the device of a ({a.device}), got {b.device}")
    if not a.is_cuda:
        raise _lib.DvgError(f"a must live on the GPU (got {a.device}); the HIP path has no CPU fallback")
    ad, bd = a.detach(), b.detach() if b is not None else None
    if out is None:
        hist = torch.empty((n + 1,), dtype=torch.int64, device=ad.device)
    else:
        hist = out
        if not torch.is_tensor(hist) or hist.dtype != torch.int64 or tuple(hist.shape) != (n + 1,) or not hist.is_contiguous() or \
                hist.device != ad.device:
            raise _lib.DvgError(f"out: hist must be a contiguous ({n + 1},) int64 tensor on {ad.device}")
    near = torch.empty((groups * rows_a,), dtype=torch.int64, device=ad.device) if nearest else None
    with torch.cuda.device(ad.device):
        check(lib().dvg_packed_overlap(ad.data_ptr(), rows_a, a_rs, a_gs, bd.data_ptr() if bd is not None else None, rows_b, b_rs,
                                       b_gs, groups, n, hist.data_ptr(), near.data_ptr() if nearest else None,
                                       int(out is not None), stream_ptr(ad.device)), "dvg_packed_overlap")
    if not nearest:
        return hist, None
    none = near < 0
    dist = torch.where(none, near, near >> 32).to(torch.int32)
    row = torch.where(none, near, near & 0x7FFFFFFF).to(torch.int32)
    if a.dim() == 3:
        dist, row = dist.view(groups, rows_a), row.view(groups, rows_a)
    return hist, (dist, row)


def packed_bonds(bits, graph, quadratic=None):
    """The bonds t_e = s_i s_j of bit-packed +-1 rows as bit-packed rows (``dvg_packed_bonds``, "DVG bonds v1").  ``bits``:
    (rows, W) or (C, M, W) int32 on the device (``sampler.pack_spins``, ``sampler.Trace.bits``; bits of spins >= n are
    ignored); the last dimension must have stride 1, the other strides are taken from the tensor, so slices need no copy.
    ``graph`` a ``GraphHandle`` with at least one edge.  ``quadratic``: None -- product mode, bit e of a bond row is set iff
    s_i s_j = +1 on edge e -- or the model's (E,) float32 couplings on the same device -- satisfied mode, the bit is set iff
    the bond is satisfied (J_e > 0: the spins differ; J_e < 0: they agree; +-0 or NaN: always).  Returns (rows, WE) or (C, M,
    WE) int32, WE = (E + 31) // 32, dense, bits >= E cleared: packed rows of E "spins" that every function on packed rows
    takes with ``n=E``.  Pure bit operations; no host sync."""
    n, E = int(graph.plan.n), int(graph.plan.n_edges)
    rows, rs, groups, gs = _packed_rows(bits, "bits", (n + 31) // 32)
    if E < 1:
        raise _lib.DvgError("graph: the graph has no edge, so there are no bonds")
    if quadratic is not None and (not torch.is_tensor(quadratic) or quadratic.dtype != torch.float32 or quadratic.numel() != E):
        raise _lib.DvgError(f"quadratic must be None or a float32 tensor of the graph's {E} values, got "
                            f"{(tuple(quadratic.shape), quadratic.dtype) if torch.is_tensor(quadratic) else type(quadratic).__name__}")
    if not bits.is_cuda:
        raise _lib.DvgError(f"bits must live on the GPU (got {bits.device}); the HIP path has no CPU fallback")
    if quadratic is not None and quadratic.device != bits.device:
        raise _lib.DvgError(f"quadratic must be on the device of bits ({bits.device}), got {quadratic.device}")
    bd = bits.detach()
    quad = quadratic.detach().contiguous() if quadratic is not None else None
    WE = (E + 31) // 32
    out = torch.empty((groups * rows, WE), dtype=torch.int32, device=bd.device)
    with torch.cuda.device(bd.device):
        check(lib().dvg_packed_bonds(graph.ptr, _lib.ptr(quad), bd.data_ptr(), rows, rs, groups, gs, out.data_ptr(),
                                     stream_ptr(bd.device)), "dvg_packed_bonds")
    return out.view(groups, rows, WE) if bits.dim() == 3 else out


def packed_link_overlap(a, a_bonds, b=None, b_bonds=None, *, n, n_edges, out=None):
    """Spin and bond distances of all pairs of bit-packed +-1 rows, together and exactly (``dvg_packed_overlap_link``, "DVG link
    overlap v1").  ``a`` / ``b``: spin rows as :func:`packed_overlap` takes them -- (rows, W) or (C, M, W) int32 on the device,
    the 3-D form M groups of C rows; ``b`` None (self mode: the pairs r < r' of ``a`` in each group), 2-D (with a 3-D ``a``:
    shared by every group) or 3-D with the same M.  ``a_bonds`` / ``b_bonds``: the sides' bond rows (:func:`packed_bonds`, or
    views of them), int32 with the leading shape of their spin rows and WE = (n_edges + 31) // 32 words; ``b_bonds`` goes with
    ``b``.  Row and group strides are taken from each tensor.  Returns ``(hist (n + 1,), link_hist (n_edges + 1,), link_sum
    (n + 1,), link_sq (n + 1,))`` int64: pairs per spin distance d (``packed_overlap``'s histogram), pairs per bond distance
    l, and per d the sums of l and of l^2 -- ``sampler.LinkOverlap.from_sums`` turns them into estimates.  ``out``: such a
    quadruple to add onto.  No host sync."""
    for name, v in (("n", n), ("n_edges", n_edges)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    n, E = int(n), int(n_edges)
    W, WE = (n + 31) // 32, (E + 31) // 32
    rows_a, a_rs, groups, a_gs = _packed_rows(a, "a", W, groups_first=False)
    _rows, ab_rs, _groups, ab_gs = _packed_rows(a_bonds, "a_bonds", WE, groups_first=False)
    if tuple(a_bonds.shape[:-1]) != tuple(a.shape[:-1]):
        raise _lib.DvgError(f"a_bonds must have the leading shape of a, got a {tuple(a.shape)} and a_bonds {tuple(a_bonds.shape)}")
    if a_bonds.device != a.device:
        raise _lib.DvgError(f"a_bonds must be on the device of a ({a.device}), got {a_bonds.device}")
    rows_b = b_rs = b_gs = bb_rs = bb_gs = 0
    if (b is None) != (b_bonds is None):
        raise _lib.DvgError("b and b_bonds go together: both None (self mode) or both given")
    if b is not None:
        rows_b, b_rs, groups_b, b_gs = _packed_rows(b, "b", W, groups_first=False)
        if b.dim() == 3 and (a.dim() != 3 or groups_b != groups):
            raise _lib.DvgError(f"b: a 3-D b needs a 3-D a with the same number of records, got a {tuple(a.shape)} and b {tuple(b.shape)}")
        _rows, bb_rs, _groups, bb_gs = _packed_rows(b_bonds, "b_bonds", WE, groups_first=False)
        if tuple(b_bonds.shape[:-1]) != tuple(b.shape[:-1]):
            raise _lib.DvgError(f"b_bonds must have the leading shape of b, got b {tuple(b.shape)} and b_bonds {tuple(b_bonds.shape)}")
        if b.dim() == 2:
            b_gs = bb_gs = 0
        for name, t in (("b", b), ("b_bonds", b_bonds)):
            if t.device != a.device:
                raise _lib.DvgError(f"{name} must be on the device of a ({a.device}), got {t.device}")
    shapes = ((n + 1,), (E + 1,), (n + 1,), (n + 1,))
    names = ("hist", "link_hist", "link_sum", "link_sq")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise _lib.DvgError("out must be a quadruple (hist, link_hist, link_sum, link_sq)")
        for name, t, shape in zip(names, out, shapes):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or \
                    t.device != a.device:
                raise _lib.DvgError(f"out: {name} must be a contiguous {shape} int64 tensor on {a.device}")
    if not a.is_cuda:
        raise _lib.DvgError(f"a must live on the GPU (got {a.device}); the HIP path has no CPU fallback")
    ad, abd = a.detach(), a_bonds.detach()
    bd, bbd = (b.detach(), b_bonds.detach()) if b is not None else (None, None)
    sums = tuple(out) if out is not None else tuple(torch.empty(s, dtype=torch.int64, device=ad.device) for s in shapes)
    with torch.cuda.device(ad.device):
        check(lib().dvg_packed_overlap_link(ad.data_ptr(), abd.data_ptr(), rows_a, a_rs, a_gs, ab_rs, ab_gs, _lib.ptr(bd), _lib.ptr(bbd),
                                            rows_b, b_rs, b_gs, bb_rs, bb_gs, groups, n, E, *(t.data_ptr() for t in sums),
                                            int(out is not None), stream_ptr(ad.device)), "dvg_packed_overlap_link")
    return sums


def _clamp_range(r, name):
    """``(lo, hi)`` floats of a solver range, None meaning no clamp."""
    if r is None:
        return -float("inf"), float("inf")
    try:
        lo, hi = r
        ok = all(isinstance(v, numbers.Real) and not isinstance(v, bool) and v == v for v in (lo, hi))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} must be None or a pair (lo, hi) of numbers, got {r!r}")
    return float(lo), float(hi)


def grbm_energy_packed(bits, graph, linear, quadratic, *, prefactor=1.0, linear_range=None, quadratic_range=None):
    """Float64 energies of bit-packed +-1 rows (``dvg_grbm_energy_packed``, "DVG energy v1") under the fields every draw uses,
    ``hs = clamp(prefactor linear, *linear_range)`` and ``Js`` likewise in float32 (a range of None does not clamp; the
    defaults give the raw GRBM energy).  ``bits``: (rows, W) or (C, M, W) int32 on the device (``sampler.pack_spins``,
    ``sampler.Trace.bits``; bits of spins >= n are ignored); the last dimension must have stride 1, the other strides are
    taken from the tensor, so slices need no copy.  ``graph`` a ``GraphHandle``; ``linear`` (n) and ``quadratic`` (E) float32
    on the same device.  Returns ``sum_i hs_i s_i + sum_e Js_e s_i s_j`` per row, float64 (rows,) or (C, M): every addend
    exact, the order of the additions fixed -- the same bits on every call.  No host sync."""
    n, E = int(graph.plan.n), int(graph.plan.n_edges)
    rows, rs, groups, gs = _packed_rows(bits, "bits", (n + 31) // 32)
    hl, hh, jl, jh = _model_arguments(graph, linear, quadratic, prefactor, linear_range, quadratic_range)
    bd, lin, quad = _on_the_device(bits, linear, quadratic)
    out = torch.empty((groups * rows,), dtype=torch.float64, device=bd.device)
    with torch.cuda.device(bd.device):
        check(lib().dvg_grbm_energy_packed(graph.ptr, lin.data_ptr(), quad.data_ptr() if E else lin.data_ptr(), float(prefactor), hl,
                                           hh, jl, jh, bd.data_ptr(), rows, rs, groups, gs, out.data_ptr(),
                                           stream_ptr(bd.device)), "dvg_grbm_energy_packed")
    return out.view(groups, rows) if bits.dim() == 3 else out


# rows of one slab of dvg_packed_correlation's product kernel (CR_SLAB_ROWS, csrc/correlation.hip): the most a 32-bit count sees
PACKED_CORRELATION_SLAB_ROWS = 1 << 18


def packed_correlation(bits, *, n, spin_sums=True, out=None):
    """Exact full pair-correlation sums of bit-packed +-1 rows (``dvg_packed_correlation``, "DVG corr v1"): every pair of spins,
    not the graph's edges only.  ``bits``: (rows, W) or (C, M, W) int32 on the device (``sampler.pack_spins``,
    ``sampler.Trace.bits``; bits of spins >= n are ignored); all rows are pooled.  The last dimension must have stride 1, the
    other strides are taken from the tensor, so slices need no copy.  Returns ``(spin_sum (n,) | None, pair_sum (n, n))``
    int64: the sums over the rows of s_i (``spin_sums=False``: None) and of s_i s_j -- symmetric, the diagonal the number of
    rows.  ``out``: such a pair to add onto (pooling calls).  ``sampler.Correlations.from_sums`` turns them into estimates.
    It allocates its workspace, the size of the input; no host sync."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError(f"n must be an integer >= 1, got {n!r}")
    n = int(n)
    rows, rs, groups, gs = _packed_rows(bits, "bits", (n + 31) // 32)
    spin_sum = pair_sum = None
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise _lib.DvgError("out must be a pair (spin_sum | None, pair_sum)")
        spin_sum, pair_sum = out
        if (spin_sum is not None) != bool(spin_sums):
            raise _lib.DvgError(f"out: spin_sum must be {'a tensor' if spin_sums else 'None'} with spin_sums={bool(spin_sums)}")
        for name, t, shape in (("spin_sum", spin_sum, (n,)), ("pair_sum", pair_sum, (n, n))):
            if name == "spin_sum" and t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or \
                    t.device != bits.device:
                raise _lib.DvgError(f"out: {name} must be a contiguous {shape} int64 tensor on {bits.device}")
    if not bits.is_cuda:
        raise _lib.DvgError(f"bits must live on the GPU (got {bits.device}); the HIP path has no CPU fallback")
    bd = bits.detach()
    if out is None:
        spin_sum = torch.empty((n,), dtype=torch.int64, device=bd.device) if spin_sums else None
        pair_sum = torch.empty((n, n), dtype=torch.int64, device=bd.device)
    with torch.cuda.device(bd.device):
        ws = _ws(lib().dvg_packed_correlation_workspace_bytes(rows, groups, n), bd.device)
        check(lib().dvg_packed_correlation(bd.data_ptr(), rows, rs, groups, gs, n, _lib.ptr(spin_sum), pair_sum.data_ptr(),
                                           int(out is not None), ws.data_ptr(), ws.numel(), stream_ptr(bd.device)),
              "dvg_packed_correlation")
    return spin_sum, pair_sum


DistinctRows = collections.namedtuple("DistinctRows", "first id rep count other_id other_hits")


def packed_distinct(bits, other=None, *, n):
    """Which bit-packed +-1 rows are the same state and how often each state occurs, exactly (``dvg_packed_distinct``, "DVG
    distinct v1").  ``bits``: (rows, W) or (C, M, W) int32 on the device (``sampler.pack_spins``, ``sampler.Trace.bits``; bits
    of spins >= n are ignored and never distinguish rows); the T rows are pooled under the flattened index t = c M + m.  The
    last dimension must have stride 1, the other strides are taken from the tensor, so slices need no copy.  ``other``: None or
    a (rows, W) int32 set on the same device whose rows are looked up among the classes, never inserted.  Returns the
    namedtuple ``DistinctRows``: ``first`` (T,) int32, the smallest index with row t's content; ``id`` (T,) int32, row t's
    class, the classes numbered by first occurrence; ``rep`` (D,) int32, the classes' first rows; ``count`` (D,) int64, their
    sizes; with ``other`` ``other_id`` (rows_other,) int32, the class equal to each row of ``other`` or -1, and
    ``other_hits`` (D,) int64, how many rows of ``other`` each class equals -- else None.  It allocates its workspace (about
    32 bytes a row) and reads the number of classes D back: one host sync."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError(f"n must be an integer >= 1, got {n!r}")
    n = int(n)
    W = (n + 31) // 32
    rows, rs, groups, gs = _packed_rows(bits, "bits", W)
    rows_o = o_rs = 0
    if other is not None:
        if torch.is_tensor(other) and other.dim() == 3:
            raise _lib.DvgError(f"other must be a flat (rows >= 1, {W}) int32 set, got {tuple(other.shape)}")
        rows_o, o_rs, _groups, _gs = _packed_rows(other, "other", W)
        if other.device != bits.device:
            raise _lib.DvgError(f"other must be on the device of bits ({bits.device}), got {other.device}")
    T = rows * groups
    if T >= 2 ** 31 or rows_o >= 2 ** 31:
        raise _lib.DvgError(f"packed_distinct indexes rows by int32: {T} rows and {rows_o} rows of other must stay below 2^31")
    if not bits.is_cuda:
        raise _lib.DvgError(f"bits must live on the GPU (got {bits.device}); the HIP path has no CPU fallback")
    bd, od = bits.detach(), other.detach() if other is not None else None
    dev = bd.device
    first, ident, rep = (torch.empty((T,), dtype=torch.int32, device=dev) for _ in range(3))
    count = torch.empty((T,), dtype=torch.int64, device=dev)
    n_distinct = torch.empty((1,), dtype=torch.int64, device=dev)
    other_id = torch.empty((rows_o,), dtype=torch.int32, device=dev) if od is not None else None
    other_hits = torch.empty((T,), dtype=torch.int64, device=dev) if od is not None else None
    with torch.cuda.device(dev):
        ws = _ws(lib().dvg_packed_distinct_workspace_bytes(rows, groups, n), dev)
        check(lib().dvg_packed_distinct(bd.data_ptr(), rows, rs, groups, gs, n, _lib.ptr(od), rows_o, o_rs, first.data_ptr(),
                                        ident.data_ptr(), rep.data_ptr(), count.data_ptr(), n_distinct.data_ptr(), _lib.ptr(other_id),
                                        _lib.ptr(other_hits), ws.data_ptr(), ws.numel(), stream_ptr(dev)), "dvg_packed_distinct")
    D = int(n_distinct.item())  # the one host read
    if D < 1:
        raise _lib.DvgError(f"dvg_packed_distinct: the table of {T} rows overflowed (n_distinct = {D})")
    return DistinctRows(first, ident, rep[:D], count[:D], other_id, other_hits[:D] if other_hits is not None else None)


def packed_distinct_counts(bits, *, n):
    """The number of distinct rows of every group of a (C, M, W) int32 set of bit-packed rows, each group on its own: (C,)
    int64 on the device.  One call of ``dvg_packed_distinct`` per group on its slice of ``bits`` -- only ``n_distinct`` is
    asked for, element c of the result -- through one workspace; no copy and no host sync."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError(f"n must be an integer >= 1, got {n!r}")
    n = int(n)
    if not torch.is_tensor(bits) or bits.dim() != 3:
        raise _lib.DvgError(f"bits must be (chains >= 1, records >= 1, {(n + 31) // 32}) int32, got "
                            f"{(tuple(bits.shape), bits.dtype) if torch.is_tensor(bits) else type(bits).__name__}")
    rows, rs, groups, gs = _packed_rows(bits, "bits", (n + 31) // 32)
    if not bits.is_cuda:
        raise _lib.DvgError(f"bits must live on the GPU (got {bits.device}); the HIP path has no CPU fallback")
    bd = bits.detach()
    out = torch.empty((groups,), dtype=torch.int64, device=bd.device)
    with torch.cuda.device(bd.device):
        ws = _ws(lib().dvg_packed_distinct_workspace_bytes(rows, 1, n), bd.device)
        for c in range(groups):
            check(lib().dvg_packed_distinct(bd.data_ptr() + 4 * c * gs, rows, rs, 1, 0, n, None, 0, 0, None, None, None, None,
                                            out.data_ptr() + 8 * c, None, None, ws.data_ptr(), ws.numel(), stream_ptr(bd.device)),
                  "dvg_packed_distinct")
    return out


Fields = collections.namedtuple("Fields", "log_pl unstable cond_sum cond_pair fields")


def grbm_fields_packed(bits, graph, linear, quadratic, *, beta, prefactor=1.0, linear_range=None, quadratic_range=None,
                       log_pl=True, unstable=True, conditional=True, fields=False, out=None):
    """Per-spin statistics of bit-packed +-1 rows through the model's local fields (``dvg_grbm_fields_packed``, "DVG fields
    v1"): with ``hs`` / ``Js`` the scaled, clamped float32 fields every draw uses (:func:`grbm_energy_packed`), ``f_i`` the
    sampler's float32 local field and ``z = clamp(2 beta f, -87, 87)`` its logit, per row and in float64
    ``log_pl = sum_i log P(s_i | rest)``, the count of ``unstable`` spins (``s_i f_i > 0``: the flip lowers the energy), and
    pooled over the rows ``cond_sum[i] = sum_r E[s_i | rest of row r]``, ``cond_pair[e] = sum_r (m_ri s_rj + m_rj s_ri)`` -- the
    Rao-Blackwellised moment sums.  ``bits``: (rows, W) or (C, M, W) int32 on the device, the strides taken from the tensor as
    in :func:`grbm_energy_packed`; ``graph`` a ``GraphHandle``; ``linear`` (n) and ``quadratic`` (E) float32 on the same
    device; ``beta`` a finite number >= 0.  ``log_pl`` / ``unstable`` / ``conditional`` / ``fields`` choose the outputs (at
    least one).  Returns ``Fields(log_pl, unstable, cond_sum, cond_pair, fields)``: float64 and int32 (rows,) or (C, M),
    float64 (n,) and (E,), float32 (rows, n) or (C, M, n); None for what was not asked for.  ``out``: a pair ``(cond_sum,
    cond_pair)`` to add this call's pooled sums onto (needs ``conditional``).  The order of every addition is fixed by the
    shapes alone: the same bits on every call.  It allocates its workspace; no host sync."""
    n, E = int(graph.plan.n), int(graph.plan.n_edges)
    rows, rs, groups, gs = _packed_rows(bits, "bits", (n + 31) // 32)
    hl, hh, jl, jh = _model_arguments(graph, linear, quadratic, prefactor, linear_range, quadratic_range)
    if isinstance(beta, bool) or not isinstance(beta, numbers.Real) or not 0 <= beta < float("inf"):
        raise ValueError(f"beta must be a finite number >= 0, got {beta!r}")
    for name, v in (("log_pl", log_pl), ("unstable", unstable), ("conditional", conditional), ("fields", fields)):
        if not isinstance(v, bool):
            raise ValueError(f"{name} must be True or False, got {v!r}")
    if not (log_pl or unstable or conditional or fields):
        raise ValueError("no output requested: at least one of log_pl, unstable, conditional, fields must be True")
    cond_sum = cond_pair = None
    if out is not None:
        if not conditional:
            raise _lib.DvgError("out: pooled sums to add onto need conditional=True")
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise _lib.DvgError("out must be a pair (cond_sum, cond_pair)")
        cond_sum, cond_pair = out
        for name, t, k in (("cond_sum", cond_sum, n), ("cond_pair", cond_pair, E)):
            if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != (k,) or not t.is_contiguous() or \
                    t.device != bits.device:
                raise _lib.DvgError(f"out: {name} must be a contiguous ({k},) float64 tensor on {bits.device}")
    bd, lin, quad = _on_the_device(bits, linear, quadratic)
    T, dev = groups * rows, bd.device
    shape = (groups, rows) if bits.dim() == 3 else (rows,)
    lp = torch.empty((T,), dtype=torch.float64, device=dev) if log_pl else None
    un = torch.empty((T,), dtype=torch.int32, device=dev) if unstable else None
    fo = torch.empty((T, n), dtype=torch.float32, device=dev) if fields else None
    if conditional and out is None:
        cond_sum = torch.empty((n,), dtype=torch.float64, device=dev)
        cond_pair = torch.empty((E,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = _ws(lib().dvg_grbm_fields_packed_workspace_bytes(graph.ptr, rows, groups), dev) if conditional else None
        check(lib().dvg_grbm_fields_packed(graph.ptr, lin.data_ptr(), quad.data_ptr() if E else lin.data_ptr(), float(prefactor), hl,
                                           hh, jl, jh, float(beta), bd.data_ptr(), rows, rs, groups, gs, _lib.ptr(lp), _lib.ptr(un),
                                           _lib.ptr(cond_sum), (cond_pair.data_ptr() if E else cond_sum.data_ptr()) if conditional else None,
                                           _lib.ptr(fo), int(out is not None), _lib.ptr(ws), ws.numel() if conditional else 0,
                                           stream_ptr(dev)), "dvg_grbm_fields_packed")
    return Fields(lp.view(shape) if log_pl else None, un.view(shape) if unstable else None, cond_sum, cond_pair,
                  fo.view(*shape, n) if fields else None)


Descent = collections.namedtuple("Descent", "bits sweeps flips unstable")
DESCEND_MAX_SWEEPS = 65536  # (DS_MAX_SWEEPS, csrc/descent.hip: with n <= 8192 a row's flip count then fits an int32)


def grbm_descend_packed(bits, graph, linear, quadratic, *, prefactor=1.0, linear_range=None, quadratic_range=None,
                        max_sweeps=1000, out=None):
    """Zero-temperature descent of bit-packed +-1 rows to local minima of the energy (``dvg_grbm_descend_packed``, "DVG descent
    v1"): with ``hs`` / ``Js`` the scaled, clamped float32 fields every draw uses (:func:`grbm_energy_packed`) and ``f_i`` the
    sampler's float32 local field, a sweep goes through the graph's colour classes in order and flips every unstable spin
    (``s_i f_i > 0``; ``f_i = 0`` is stable) of the class; a row stops after its first sweep without a flip -- a fixed point --
    or after ``max_sweeps`` (1 .. 65536) sweeps.  ``bits``: (rows, W) or (C, M, W) int32 on the device, the strides taken from
    the tensor as in :func:`grbm_fields_packed`; ``graph`` a ``GraphHandle``; ``linear`` (n) and ``quadratic`` (E) float32 on
    the same device.  ``out``: a contiguous int32 tensor of the input's shape for the final rows -- ``bits`` itself when
    ``bits`` is contiguous (in place); any other sharing of memory with ``bits`` is refused.  Returns ``Descent(bits, sweeps,
    flips, unstable)``: the final rows (pad bits 0), and int32 shaped like the leading dimensions the sweeps in which the row
    flipped something, its flips in all, and the unstable spins left (0 = converged; non-zero only where ``sweeps ==
    max_sweeps``).  No randomness and no sum across rows: a row's result depends on that row alone, the same bits on every
    call.  The energy falls strictly with every flip when the float32 field sums are exact; in general ``max_sweeps`` is the
    only promise of termination.  No workspace, no host sync."""
    n, E = int(graph.plan.n), int(graph.plan.n_edges)
    W = (n + 31) // 32
    rows, rs, groups, gs = _packed_rows(bits, "bits", W)
    hl, hh, jl, jh = _model_arguments(graph, linear, quadratic, prefactor, linear_range, quadratic_range)
    if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, numbers.Integral) or not 1 <= max_sweeps <= DESCEND_MAX_SWEEPS:
        raise ValueError(f"max_sweeps must be an integer in 1 .. {DESCEND_MAX_SWEEPS}, got {max_sweeps!r}")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.int32 or out.shape != bits.shape or not out.is_contiguous() or \
                out.device != bits.device:
            raise _lib.DvgError(f"out must be a contiguous int32 tensor of shape {tuple(bits.shape)} on {bits.device}, got "
                                f"{(tuple(out.shape), out.dtype, out.device) if torch.is_tensor(out) else type(out).__name__}")
        a0, b0 = bits.data_ptr(), out.data_ptr()
        a1 = a0 + 4 * ((groups - 1) * gs + (rows - 1) * rs + W)
        if a0 < b0 + 4 * out.numel() and b0 < a1 and not (a0 == b0 and bits.is_contiguous()):
            raise _lib.DvgError("out shares memory with bits: in place needs out to be bits itself and bits contiguous "
                                f"(strides {tuple(bits.stride())})")
    bd, lin, quad = _on_the_device(bits, linear, quadratic)
    T, dev = groups * rows, bd.device
    shape = (groups, rows) if bits.dim() == 3 else (rows,)
    res = torch.empty(tuple(bits.shape), dtype=torch.int32, device=dev) if out is None else out.detach()
    sw, fl, un = (torch.empty((T,), dtype=torch.int32, device=dev) for _ in range(3))
    with torch.cuda.device(dev):
        check(lib().dvg_grbm_descend_packed(graph.ptr, lin.data_ptr(), quad.data_ptr() if E else lin.data_ptr(), float(prefactor), hl,
                                            hh, jl, jh, bd.data_ptr(), rows, rs, groups, gs, int(max_sweeps), res.data_ptr(),
                                            sw.data_ptr(), fl.data_ptr(), un.data_ptr(), stream_ptr(dev)), "dvg_grbm_descend_packed")
    return Descent(res if out is None else out, sw.view(shape), fl.view(shape), un.view(shape))


Resampled = collections.namedtuple("Resampled", "parents state family weights")


def _population_arguments(log_weight, populations, chain_id0, seed, step, state, family):
    """The argument checks of :func:`population_resample`, none of which touches the library.  Returns (C, n)."""
    if not torch.is_tensor(log_weight) or log_weight.dtype != torch.float64 or log_weight.dim() != 1 or log_weight.numel() < 1:
        raise _lib.DvgError(f"log_weight must be a (chains >= 1,) float64 tensor, got "
                            f"{(tuple(log_weight.shape), log_weight.dtype) if torch.is_tensor(log_weight) else type(log_weight).__name__}")
    C = int(log_weight.shape[0])
    for name, v, top in (("populations", populations, 2 ** 31), ("chain_id0", chain_id0, 2 ** 32), ("seed", seed, 2 ** 64),
                         ("step", step, 2 ** 32)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not (name == "populations") <= v < top:
            raise ValueError(f"{name} must be an integer in {int(name == 'populations')} .. {top - 1}, got {v!r}")
    if C % int(populations):
        raise ValueError(f"populations={populations!r} does not divide the {C} chains of log_weight")
    if C // int(populations) > 2 ** 20:
        raise ValueError(f"populations={populations!r}: {C // int(populations)} chains per population are more than 2^20")
    n = 0
    if state is not None:
        if not torch.is_tensor(state) or state.dtype != torch.int8 or state.dim() != 2 or int(state.shape[0]) != C or state.shape[1] < 1:
            raise _lib.DvgError(f"state must be a ({C}, n >= 1) int8 tensor, got "
                                f"{(tuple(state.shape), state.dtype) if torch.is_tensor(state) else type(state).__name__}")
        n = int(state.shape[1])
    if family is not None and (not torch.is_tensor(family) or family.dtype != torch.int32 or tuple(family.shape) != (C,)):
        raise _lib.DvgError(f"family must be a ({C},) int32 tensor, got "
                            f"{(tuple(family.shape), family.dtype) if torch.is_tensor(family) else type(family).__name__}")
    if not log_weight.is_cuda:
        raise _lib.DvgError(f"log_weight must live on the GPU (got {log_weight.device}); the HIP path has no CPU fallback")
    for name, t in (("state", state), ("family", family)):
        if t is not None and t.device != log_weight.device:
            raise _lib.DvgError(f"{name} must be on the device of log_weight ({log_weight.device}), got {t.device}")
    return C, n


def population_resample(log_weight, *, populations=1, chain_id0=0, seed, step, state=None, family=None, weights=False):
    """Population annealing's resampling step (``dvg_population_resample``, "DVG PA v1" in include/dvg.h): systematic
    resampling of weighed chains in exact integer arithmetic.  ``log_weight``: (C,) float64 on the device, ``populations``
    independent populations of C / populations consecutive chains (at most 2^20 each); ``chain_id0``, ``seed``, ``step``: the
    Philox counter and key of the populations' offsets.  ``state`` (C, n) int8: the chains' rows, gathered out of place;
    ``family`` (C,) int32: the founders' indices to hand down (None: a child gets its parent's index).  Returns the namedtuple
    ``(parents, state, family, weights)`` of device tensors: ``parents`` (C,) int32, child j's parent; ``state`` the
    gathered rows or None; ``family`` (C,) int32; ``weights`` None, or with ``weights=True`` the (C,) int64 integer weights
    k_c in 0 .. 2^32.  It owns its workspace; no host sync."""
    C, n = _population_arguments(log_weight, populations, chain_id0, seed, step, state, family)
    lw = log_weight.detach().contiguous()
    dev = lw.device
    st = state.detach().contiguous() if state is not None else None
    fam = family.detach().contiguous() if family is not None else None
    parents = torch.empty((C,), dtype=torch.int32, device=dev)
    state_out = torch.empty_like(st) if st is not None else None
    family_out = torch.empty((C,), dtype=torch.int32, device=dev)
    k = torch.empty((C,), dtype=torch.int64, device=dev) if weights else None
    with torch.cuda.device(dev):
        ws = torch.empty((int(lib().dvg_population_resample_workspace_bytes(C)),), dtype=torch.uint8, device=dev)
        check(lib().dvg_population_resample(lw.data_ptr(), C, int(populations), int(chain_id0), int(seed), int(step),
                                            _lib.ptr(st), _lib.ptr(state_out), n, _lib.ptr(fam), family_out.data_ptr(),
                                            parents.data_ptr(), _lib.ptr(k), ws.data_ptr(), ws.numel(), stream_ptr(dev)),
              "dvg_population_resample")
    return Resampled(parents, state_out, family_out, k)


# ----------------------------------------------------------------------------- MSE


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, recon, images):
        L = lib()
        rd = require_cuda(recon.detach().float().contiguous(), "reconstructed")
        im = require_cuda(images.detach().float().contiguous(), "images")
        B, R = rd.shape[0], rd.shape[1]
        if rd.numel() != B * R * 1024 or im.numel() != B * 1024:
            raise ValueError("mse_loss expects reconstructed (B,R,1,32,32) and images (B,1,32,32)")
        loss = torch.empty((), dtype=torch.float32, device=rd.device)
        grad = torch.empty_like(rd) if recon.requires_grad else None
        ws = _ws(L.dvg_mse_workspace_bytes(), rd.device)
        with torch.cuda.device(rd.device):
            check(L.dvg_mse_fwd_bwd(rd.data_ptr(), im.data_ptr(), B, R, 1.0, loss.data_ptr(), _lib.ptr(grad),
                                    ws.data_ptr(), ws.numel(), stream_ptr(rd.device)), "dvg_mse_fwd_bwd")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None), None


def replicated_mse_loss(reconstructed, images):
    """mse_loss(reconstructed, images.unsqueeze(1).repeat(1, R, 1, 1, 1)) without building the repeat
    (/root/reference/src/model_wrapper.py:302-305)."""
    return _MSE.apply(reconstructed, images)


def replicated_mse_loss_and_grad(reconstructed, images):
    """(loss, d loss / d reconstructed) outside autograd (see :func:`mmd_loss_and_grad`)."""
    L = lib()
    rd = require_cuda(reconstructed.detach().float().contiguous(), "reconstructed")
    im = require_cuda(images.detach().float().contiguous(), "images")
    B, R = rd.shape[0], rd.shape[1]
    if rd.numel() != B * R * 1024 or im.numel() != B * 1024:
        raise ValueError("mse_loss expects reconstructed (B,R,1,32,32) and images (B,1,32,32)")
    loss = torch.empty((), dtype=torch.float32, device=rd.device)
    grad = torch.empty_like(rd)
    ws = _ws(L.dvg_mse_workspace_bytes(), rd.device)
    with torch.cuda.device(rd.device):
        check(L.dvg_mse_fwd_bwd(rd.data_ptr(), im.data_ptr(), B, R, 1.0, loss.data_ptr(), grad.data_ptr(),
                                ws.data_ptr(), ws.numel(), stream_ptr(rd.device)), "dvg_mse_fwd_bwd")
    return loss, grad
