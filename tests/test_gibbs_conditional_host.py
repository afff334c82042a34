"""CPU-side checks of the conditional block-Gibbs entry point (``dvg_gibbs_sample_clamped``, include/dvg.h): the symbol is
declared and exported, and its argument checks answer before any device work."""
import ctypes

import support
from image_generation_amd import _lib

NAME = "dvg_gibbs_sample_clamped"


def test_symbol_is_declared_bound_and_exported():
    support.assert_declared_bound_exported(NAME)


def _call(g, lin, quad, state, clamp, stride, n_chains=4):
    L = _lib.lib()
    rc = L.dvg_gibbs_sample_clamped(g, lin, quad, 1.0, -1, 1, -1, 1, 1.0, state, n_chains, 0, 0, 0, 1, 1, clamp, stride,
                                    None, None, None)
    return rc, L.dvg_last_error()


def test_argument_validation_without_gpu():
    """Null pointers, a null ``clamp`` and a chain stride that is neither 0 nor n are DVG_E_INVALID (-1) with a message,
    before any HIP call (safe on a CPU-only box)."""
    rc, msg = _call(None, None, None, None, None, 0)
    assert rc == -1 and b"null" in msg
    # The remaining checks need non-null pointers that are never handed to the device: the graph handle is host memory
    # whose first field is its spin count (csrc/graph.h), here 64; the others are never dereferenced on the host.
    n = 64
    graph = ctypes.create_string_buffer(4096)
    ctypes.c_int32.from_buffer(graph).value = n
    g = ctypes.cast(graph, ctypes.c_void_p)
    dummy = ctypes.create_string_buffer(16)
    p = ctypes.cast(dummy, ctypes.c_void_p)
    rc, msg = _call(g, p, p, p, None, n)
    assert rc == -1 and b"clamp" in msg
    for stride in (1, n - 1, n + 1, 2 * n, -n):
        rc, msg = _call(g, p, p, p, p, stride)
        assert rc == -1 and b"clamp_chain_stride" in msg, (stride, rc, msg)
    rc, msg = _call(g, p, p, p, p, n, n_chains=0)
    assert rc == -1 and b"n_chains" in msg
