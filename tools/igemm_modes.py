"""The implicit-GEMM kernel alone in its three operand modes (float32 / f32x3 / bf16 inputs, dvg_set_conv_precision) on
c3-sized layer shapes: `python tools/igemm_modes.py` on an MI355X.  Times one launch (HIP events over 20 repeats), prices
it in 9-tap float32 FLOPs and checks the result against a float64 convolution of the same operands."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_generation_amd import _lib, dev


def run(M, Cin, Cout, L, x, w, reps=20):
    wp = torch.empty(9 * Cin * Cout * 2, device="cuda")
    out = dev.conv_igemm(x, w, 2, M, Cin, Cout, L, 9, 0, 0, wp=wp)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dev.conv_igemm(x, w, 2, M, Cin, Cout, L, 9, 0, 0, wp=wp, repack=False)
    e1.record(); torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / reps * 1e3


for arg in [a for a in sys.argv[1:] if "=" in a]:
    name, value = arg.split("=")
    _lib.set_option(name, int(value))
    sys.argv.remove(arg)
shapes = [(128, 128, 2, 32768), (128, 128, 3, 8192), (64, 128, 3, 32768), (128, 64, 3, 32768), (64, 32, 4, 32768), (512, 128, 1, 32768)]
if len(sys.argv) > 1:
    shapes = shapes[: int(sys.argv[1])]
for Cin, Cout, L, imgs in shapes:
    M = imgs << (2 * L)
    if M * max(Cin, Cout) * 4 >= 2**32: continue
    torch.manual_seed(0)
    x = torch.randn(M, Cin, device="cuda"); w = torch.randn((Cin, Cout, 3, 3), device="cuda") / (3 * Cin**0.5)
    fl = 2.0 * M * Cin * Cout * 9
    # float64 truth on a slice of images (ConvTranspose2d fwd, mode 2)
    ni = 8
    xi = dev.morton_to_nchw(x[: ni << (2 * L)], ni, Cin, 1 << L).double()
    want = torch.nn.functional.conv_transpose2d(xi, w.double(), padding=1)
    line = f"Cin={Cin:3d} Cout={Cout:3d} L={L} M={M:8d} "
    for mode in ("f32", "f32x3", "bf16"):
        _lib.set_conv_precision(mode)
        o, t = run(M, Cin, Cout, L, x, w)
        got = dev.morton_to_nchw(o[: ni << (2 * L)], ni, Cout, 1 << L).double()
        err = float((got - want).abs().max() / want.abs().max())
        line += f" | {mode} {t:7.1f} us {fl/t/1e6:6.1f} TF/s err {err:.1e}"
    _lib.set_conv_precision("f32")
    print(line, flush=True)

# The decoder head's own launches at c3 (the composed Linear o ConvTranspose map: rows x n x 4 C = 32768 x 512 x 512, one tap,
# +-1 rows): the forward GEMM in the three operand modes and in the spin-operand form (dev option dev_spin_operand makes
# the +-1 promise for the hook's input), and its weight-gradient GEMM dW = S^T dY in the float32 and the spin form.
if len(sys.argv) <= 1:
    M, Cin, Cout = 32768, 512, 512
    torch.manual_seed(0)
    x = (torch.randint(0, 2, (M, Cin), device="cuda").float() * 2 - 1).contiguous()
    w9 = torch.zeros((Cout, Cin, 3, 3), device="cuda"); w9[:, :, 0, 0] = torch.randn((Cout, Cin), device="cuda") / Cin**0.5
    dy = torch.randn(M, Cout, device="cuda")
    want = x[:256].double() @ w9[:, :, 0, 0].double().T
    fl = 2.0 * M * Cin * Cout

    def head(reps=20):
        wp = torch.empty(Cin * Cout * 2, device="cuda")
        out = dev.conv_igemm(x, w9, 0, M, Cin, Cout, 0, 1, 0, 0, wp=wp)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            dev.conv_igemm(x, w9, 0, M, Cin, Cout, 0, 1, 0, 0, wp=wp, repack=False)
        e1.record(); torch.cuda.synchronize()
        return float((out[:256].double() - want).abs().max() / want.abs().max()), e0.elapsed_time(e1) / reps * 1e3

    line = f"head fwd   M={M} Cin={Cin} Cout={Cout} 1 tap, +-1 rows "
    for mode, spin in (("f32", 0), ("f32x3", 0), ("bf16", 0), ("f32", 1), ("f32x3", 1)):
        _lib.set_conv_precision(mode)
        _lib.set_option("dev_spin_operand", spin)
        err, t = head()
        line += f" | {mode}{' spin' if spin else ''} {t:7.1f} us {fl/t/1e6:6.1f} TF/s err {err:.1e}"
    _lib.set_conv_precision("f32")
    print(line, flush=True)
    want_g = dy.double().T[:64] @ x.double()
    line = f"head wgrad M={M} Cin={Cin} Cout={Cout} 1 tap, +-1 rows "
    for spin in (0, 1):
        _lib.set_option("dev_spin_operand", spin)
        g = dev.conv_wgrad(x, dy, 0, (Cout, Cin, 3, 3), M, Cin, Cout, 0, ntaps=1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            dev.conv_wgrad(x, dy, 0, (Cout, Cin, 3, 3), M, Cin, Cout, 0, ntaps=1)
        e1.record(); torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / 20 * 1e3
        err = float((g[:64, :, 0, 0].double() - want_g).abs().max() / want_g.abs().max())
        line += f" | {'spin' if spin else 'f32 '} {t:7.1f} us (with its slab reduce) err {err:.1e}"
    _lib.set_option("dev_spin_operand", 0)
    print(line, flush=True)
