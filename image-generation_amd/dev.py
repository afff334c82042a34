"""Development access to the two MFMA GEMM kernels (include/dvg_dev.h) + layout helpers.
Used by kernel-level tests and micro-benchmarks; not part of the product surface."""
import ctypes

import numpy as np
import torch

from . import _abi, _lib

# every function of include/dvg_dev.h but the option accessors, which _lib binds with the library
_SIGS = {k: v for k, v in _abi.signatures("dvg_dev.h").items() if k not in _lib.DEV_OPTION_SIGNATURES}
_bound = False


def lib():
    global _bound
    L = _lib.lib()
    if not _bound:
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _bound = True
    return L


def morton_perm(side: int) -> torch.Tensor:
    """perm[m] = row-major index (y*side + x) of the pixel stored at Morton position m."""
    def compact(v):
        v &= 0x55555555
        v = (v | (v >> 1)) & 0x33333333
        v = (v | (v >> 2)) & 0x0F0F0F0F
        v = (v | (v >> 4)) & 0x00FF00FF
        return v
    m = np.arange(side * side)
    return torch.from_numpy((compact(m >> 1) * side + compact(m)).astype(np.int64))


def nchw_to_morton(x: torch.Tensor) -> torch.Tensor:
    """(N,C,H,W) -> (N*H*W, C) NHWC with Morton-ordered pixels."""
    N, C, H, W = x.shape
    perm = morton_perm(H).to(x.device)
    return x.permute(0, 2, 3, 1).reshape(N, H * W, C)[:, perm, :].reshape(N * H * W, C).contiguous()


def morton_to_nchw(t: torch.Tensor, N: int, C: int, side: int) -> torch.Tensor:
    perm = morton_perm(side).to(t.device)
    out = torch.empty((N, side * side, C), dtype=t.dtype, device=t.device)
    out[:, perm, :] = t.reshape(N, side * side, C)
    return out.reshape(N, side, side, C).permute(0, 3, 1, 2).contiguous()


def conv_igemm(x_m, w, mode, M, Cin, Cout, L, ntaps=9, ups=0, poolsum=0, bias=None, stats=False, wp=None, repack=True,
               splitk=True):
    Lb = lib()
    dev = x_m.device
    wp = wp if wp is not None else torch.empty((ntaps * Cin * Cout * 3 + 1) // 2, device=dev)  # (up to three bf16 planes)
    out = torch.empty(((M // 4) if poolsum else M, Cout), device=dev)
    st = torch.empty((Lb.dvg_dev_conv_stats_blocks(M, Cout), Cout, 2), device=dev) if stats else None
    nsk = Lb.dvg_dev_conv_splitk_floats(M, Cin, Cout, ntaps, poolsum) if splitk else 0
    sk = torch.empty(nsk, device=dev) if nsk else None
    _lib.check(Lb.dvg_dev_conv_igemm(x_m.data_ptr(), w.data_ptr(), mode, wp.data_ptr(), _lib.ptr(bias), out.data_ptr(),
                                     _lib.ptr(st), M, Cin, Cout, L, ntaps, ups, poolsum, int(repack), _lib.ptr(sk),
                                     _lib.stream_ptr(dev)))
    return (out, st) if stats else out


def conv_igemm_form(M, Cin, Cout, L, ntaps=9, ups=0, poolsum=0):
    """The form ``conv_igemm`` of these arguments takes under the current options and operand mode (the launcher's own
    decision; no device needed): ``tile`` = (BM, BN), ``pm`` = the operand form (0 float32 through registers, 3 float32 by
    LDS-DMA, 4 f32x3, 5 bf16 inputs, 6 spin A), ``ksplit`` = the split-K count (1: unsplit), ``posmajor``."""
    o = (ctypes.c_int * 5)()
    _lib.check(lib().dvg_dev_conv_igemm_form(M, Cin, Cout, L, ntaps, ups, poolsum, o), "dvg_dev_conv_igemm_form")
    return dict(tile=(o[0], o[1]), pm=o[2], ksplit=o[3], posmajor=bool(o[4]))


def conv_wgrad_form(M, Cin, Cout, ntaps=9, ups=0):
    """The kernel ``conv_wgrad`` of these arguments takes under the current options and operand mode (no device needed):
    ``tile`` = the channel tile (Cin x Cout), ``dma`` = an LDS-DMA kernel (``conv_wgrad9_dma_kernel<tile[0] / 32, tile[1] / 32, ..>``
    or the 1-tap ``conv_wgrad1_dma_kernel``) instead of a register-staged one, ``tap1_dma``, ``spin`` = its spin form."""
    o = (ctypes.c_int * 5)()
    _lib.check(lib().dvg_dev_conv_wgrad_form(M, Cin, Cout, ntaps, ups, o), "dvg_dev_conv_wgrad_form")
    return dict(tile=(o[0], o[1]), dma=bool(o[2]), tap1_dma=bool(o[3]), spin=bool(o[4]))


def conv_wino_ok(M, Cin, Cout, L):
    return bool(lib().dvg_dev_conv_wino_ok(M, Cin, Cout, L))


def conv_wino_shape(M, Cin, Cout, L):
    """Whether the F(2x2,3x3) form can run the shape (whatever option enc_wino says)."""
    return bool(lib().dvg_dev_conv_wino_shape(M, Cin, Cout, L))


FORMS = ("direct", "fold", "d22", "lc0", "wino2", "wino4")  # csrc/conv_plan.h: ConvForm


def plan_forms(network, rows, n_latents, training=True):
    """The kernel forms a network call would take under the current options and operand mode (no device needed):
    ``(layers, flags)`` with ``layers[l] = (forward, data gradient, weight gradient)`` as names of ``FORMS`` (``None`` for
    the VALU layers) and ``flags = dict(d22, lc0, tail)``.  ``network``: ``"encoder"`` (rows = batch) or ``"decoder"``
    (rows = batch x replicas)."""
    out = (ctypes.c_int * 15)()
    _lib.check(lib().dvg_dev_plan_forms({"encoder": 0, "decoder": 1}[network], rows, n_latents, int(training), out),
               "dvg_dev_plan_forms")
    layers = [tuple(FORMS[out[3 * l + k]] for k in range(3)) if out[3 * l] >= 0 else None for l in range(4)]
    return layers, dict(d22=bool(out[12]), lc0=bool(out[13]), tail=bool(out[14]))


MMD_PAIR_FORMS = ("f32", "sliced", "fq", "w128")  # csrc/mmd_plan.h: MmdPairForm
MMD_DIST_FORMS = ("f32", "spin", "spin256")        # MmdDistForm
MMD_GRAM_PIPES = ("int8", "fp4")                   # MmdGram


def mmd_plan(nx, ny, d):
    """The kernel forms ``F.mmd_loss_and_grad`` takes for x of (nx, d) and y of (ny, d) under the current options (no device
    needed).  ``pair`` / ``pair_params``: the pair kernel and its template parameters; ``dist`` / ``dist_ns``: the
    distance-sum kernel (launched when no bandwidth is given) and its parameter; ``gram``: the matrix pipe of the exact
    spin Gram; ``gated_f32``: a float32 launch (``mmd_main_kernel<gated_nfb>``) follows the pair kernel."""
    o = (ctypes.c_int64 * 24)()
    _lib.check(lib().dvg_dev_mmd_plan(nx, ny, d, o), "dvg_dev_mmd_plan")
    pair = MMD_PAIR_FORMS[o[0]]
    params = {"f32": dict(NFB=o[1]), "sliced": dict(NFB=o[1]), "fq": dict(NFBW=o[2]),
              "w128": dict(NST=o[3], NFT=o[4], ONE=bool(o[5]))}[pair]
    return dict(pair=pair, pair_params=params, dist=MMD_DIST_FORMS[o[6]], dist_ns=o[7], gram=MMD_GRAM_PIPES[o[8]],
                splits=o[9], slices=o[10], gated_f32=o[11] != 0, gated_nfb=o[11], loss_parts=o[12], workspace_bytes=o[13],
                dist_splits=o[14], gram_passes=o[15], bf16_terms=o[16], pair_grid=(o[17], o[18], o[19]),
                dist_grid=(o[20], o[21]), gated_grid=o[22], final_grid=o[23])


GIBBS_FORMS = ("rolled", "lane", "slots")            # csrc/gibbs_plan.h: GibbsForm
GIBBS_KINDS = ("plain", "held", "table", "weigh")    # GibbsDrawKind
# ... by name: "trace" (dvg_gibbs_sample_traced) is GK_TRACE = 5, behind GK_EXCHANGE, which dvg_dev_gibbs_exchange_plan plans;
# "field" (dvg_gibbs_sample_fields) is GK_FIELD = 6
GIBBS_KIND_IDS = dict({k: i for i, k in enumerate(GIBBS_KINDS)}, trace=5, field=6)
# the weighed forms of the kinds above that plan as their unweighed one does: "field_weigh" (dvg_gibbs_sample_fields_ais) is
# GK_FIELD_WEIGH = 7
GIBBS_WEIGHED_KIND_IDS = dict(field_weigh=7)


def gibbs_draw_plan(plan, n_chains, kind="plain"):
    """The kernel form a Gibbs draw of ``n_chains`` chains takes on the graph of ``plan`` (a ``graphs.GibbsPlan``) under
    the current option ``gibbs_generic`` (no device needed).  ``kind``: ``"plain"`` (``dvg_gibbs_sample``), ``"held"``
    (``_clamped``), ``"table"`` (``_annealed``), ``"weigh"`` (``_ais``), ``"trace"`` (``_traced``: the table kind's plan), ``"field"`` (``_fields``: rolled on every graph,
    ``lds_bytes`` with the chains' rows of hs) or ``"field_weigh"`` (``_fields_ais``: the field kind's plan).  ``form``: ``"rolled"`` (``gibbs_kernel``),
    ``"lane"`` (``gibbs_fast_kernel``) or ``"slots"`` (``gibbs_slot_kernel``), ``params`` its template parameters;
    ``workgroups``, ``threads``, ``lds_bytes``: the launch, what ``dvg_gibbs_launch_info`` reports for the plain kind;
    ``lane_image``: the shape of the graph's lane-major image (csrc/graph.h), ``None`` for a graph that gets none."""
    class_ptr = np.ascontiguousarray(plan.class_ptr, dtype=np.int32)
    adj_ptr = np.ascontiguousarray(plan.adj_ptr, dtype=np.int32)
    o = (ctypes.c_int64 * 19)()
    kind_id = GIBBS_WEIGHED_KIND_IDS[kind] if kind in GIBBS_WEIGHED_KIND_IDS else GIBBS_KIND_IDS[kind]
    _lib.check(lib().dvg_dev_gibbs_draw_plan(int(plan.n), int(plan.n_colours), class_ptr.ctypes.data, adj_ptr.ctypes.data,
                                             int(n_chains), kind_id, o), "dvg_dev_gibbs_draw_plan")
    return _gibbs_plan_dict(o)


def _gibbs_plan_dict(o):
    form = GIBBS_FORMS[o[0]]
    params = {"rolled": dict(LPC=o[1], WAVES=o[2]), "lane": dict(LPC=o[1], WAVES=o[2], MB=o[3], NR=o[4], MAXS=o[5]),
              "slots": dict(MAXS=o[5], CH=o[6], FIX=bool(o[7]))}[form]
    return dict(form=form, params=params, slots=o[8], chains_per_workgroup=o[9], workgroups=o[10], threads=o[11],
                lds_bytes=o[12], lane_image=dict(LPC=o[14], MB=o[15], NR=o[16], rows=o[17]) if o[13] else None, n_batches=o[18])


def gibbs_exchange_plan(plan, n_ladders, n_replicas):
    """The kernel form an exchange draw (``dvg_gibbs_sample_tempered``) of ``n_ladders`` ladders of ``n_replicas`` chains takes
    on the graph of ``plan`` under the current option ``gibbs_generic`` (no device needed).  The entries of
    :func:`gibbs_draw_plan` -- ``chains_per_workgroup`` counts chain slots, ``lds_bytes`` includes the exchange's mailboxes --
    plus ``ladders_per_workgroup``: the whole ladders a workgroup holds (its other slots idle)."""
    class_ptr = np.ascontiguousarray(plan.class_ptr, dtype=np.int32)
    adj_ptr = np.ascontiguousarray(plan.adj_ptr, dtype=np.int32)
    o = (ctypes.c_int64 * 20)()
    _lib.check(lib().dvg_dev_gibbs_exchange_plan(int(plan.n), int(plan.n_colours), class_ptr.ctypes.data, adj_ptr.ctypes.data,
                                                 int(n_ladders), int(n_replicas), o), "dvg_dev_gibbs_exchange_plan")
    return dict(_gibbs_plan_dict(o), ladders_per_workgroup=o[19])


def conv_wino(x_m, w, mode, M, Cin, Cout, L, bias=None, stats=False, cus=0, um=0):
    """The stride-1 3x3 layer of conv_igemm (modes 0 / 1) in the Winograd F(2x2,3x3) form (csrc/conv_wino.hip).  ``um`` as in
    :func:`conv_wino4`: 1 = the Upsample(x2) + 3x3 forward (``x_m`` = the source map, M / L of the output grid; 9 of the 16
    positions), 2 = its data gradient (``x_m`` = the fine-grid gradient, the result = the source map's gradient, M / 4 rows).
    ``cus``: CUs the persistent grid is sized for (0 = 256)."""
    Lb = lib()
    dev = x_m.device
    u = torch.empty(16 * Cin * Cout, device=dev)
    out = torch.empty((M // 4 if um == 2 else M, Cout), device=dev)
    st = torch.empty((Lb.dvg_dev_conv_wino_stats_blocks(M, Cout), Cout, 2), device=dev) if stats else None
    _lib.check(Lb.dvg_dev_conv_wino(x_m.data_ptr(), w.data_ptr(), mode, u.data_ptr(), _lib.ptr(bias), out.data_ptr(),
                                    _lib.ptr(st), M, Cin, Cout, L, int(cus), int(um), _lib.stream_ptr(dev)))
    return (out, st) if stats else out


def conv_wino4_shape(M, Cin, Cout, L):
    return bool(lib().dvg_dev_conv_wino4_shape(M, Cin, Cout, L))


def conv_wino4(x_m, w, mode, M, Cin, Cout, L, bias=None, stats=False, cus=0, um=0):
    """The same layer in the Winograd F(4x4,3x3) form (csrc/conv_wino4.hip).  ``um`` = 1: the Upsample(x2) + 3x3 forward
    (``x_m`` = the source map, M / L of the output grid; 25 of the 36 positions); ``um`` = 2: its data gradient (``x_m`` = the
    fine-grid gradient, the result = the source map's gradient, M / 4 rows)."""
    Lb = lib()
    dev = x_m.device
    u = torch.empty(36 * Cin * Cout, device=dev)
    out = torch.empty((M // 4 if um == 2 else M, Cout), device=dev)
    st = torch.empty((M // 1024, Cout, 2), device=dev) if stats else None
    _lib.check(Lb.dvg_dev_conv_wino4(x_m.data_ptr(), w.data_ptr(), mode, u.data_ptr(), _lib.ptr(bias), out.data_ptr(),
                                     _lib.ptr(st), M, Cin, Cout, L, int(cus), int(um), _lib.stream_ptr(dev)))
    return (out, st) if stats else out


def conv_wgrad(x_m, dy, mode, w_shape, M, Cin, Cout, L, ntaps=9, ups=0):
    Lb = lib()
    dev = x_m.device
    slabs = torch.empty(Lb.dvg_dev_wgrad_slab_floats(M, Cin, Cout, ntaps), device=dev)
    gw = torch.empty(w_shape, device=dev)
    _lib.check(Lb.dvg_dev_conv_wgrad(x_m.data_ptr(), dy.data_ptr(), slabs.data_ptr(), gw.data_ptr(), mode, M, Cin, Cout, L,
                                     ntaps, ups, _lib.stream_ptr(dev)))
    return gw


def conv_wino_wgrad(x_m, dy, mode, w_shape, M, Cin, Cout, L, ups=0, cus=0):
    """The 3x3 weight gradient in the Winograd form (csrc/conv_wino_wgrad.hip), or None when the shape does not qualify.
    ``cus``: CUs the persistent grid is sized for (0: the budget the training step gives the launch)."""
    Lb = lib()
    dev = x_m.device
    nf = Lb.dvg_dev_wino_wgrad_slab_floats(M, Cin, Cout, L)
    if nf == 0:
        return None
    slabs = torch.empty(nf, device=dev)
    gw = torch.empty(w_shape, device=dev)
    _lib.check(Lb.dvg_dev_conv_wino_wgrad(x_m.data_ptr(), dy.data_ptr(), slabs.data_ptr(), gw.data_ptr(), mode, M, Cin, Cout, L,
                                          int(ups), int(cus), _lib.stream_ptr(dev)))
    return gw


def encoder_saved(ws: torch.Tensor, B: int, n: int):
    """Views into an encoder workspace after a forward call: per layer the pre-BatchNorm convolution output as NCHW, the
    batch mean and the batch inverse standard deviation (diagnostics).  The offsets are the TRAINING plan's (an evaluation-
    mode forward may plan its packs differently: do not use this after one).  Layer 0's ``Y`` is ``None`` under the
    default ``enc_l0_fused`` != 0: that output is recomputed by every pass that needs it and never written."""
    off = (ctypes.c_size_t * 16)()
    _lib.check(lib().dvg_dev_encoder_layout(B, n, off), "dvg_dev_encoder_layout")
    f = ws.view(torch.float32)
    ch = [32, 64, 128, n]
    out = []
    for l in range(4):
        side, C = 32 >> l, ch[l]
        y = f[off[l]: off[l] + B * side * side * C]
        stored = l > 0 or _lib.get_option("enc_l0_fused") == 0
        out.append(dict(Y=morton_to_nchw(y, B, C, side) if stored else None, mean=f[off[8 + l]: off[8 + l] + C], invstd=f[off[12 + l]: off[12 + l] + C]))
    return out


def conv_wino4_wgrad(x_m, dy, mode, w_shape, M, Cin, Cout, L, cus=0):
    """The 3x3 weight gradient in the Winograd F(4x4,3x3) form (csrc/conv_wino4_wgrad.hip), or None when the shape does not
    qualify.  ``cus``: CUs the grid is sized for (0: the budget the training step gives the launch)."""
    Lb = lib()
    dev = x_m.device
    nf = Lb.dvg_dev_wino4_wgrad_slab_floats(M, Cin, Cout, L)
    if nf == 0:
        return None
    slabs = torch.empty(nf, device=dev)
    gw = torch.empty(w_shape, device=dev)
    _lib.check(Lb.dvg_dev_conv_wino4_wgrad(x_m.data_ptr(), dy.data_ptr(), slabs.data_ptr(), gw.data_ptr(), mode, M, Cin, Cout, L,
                                           int(cus), _lib.stream_ptr(dev)))
    return gw
