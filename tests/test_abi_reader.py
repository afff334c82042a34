"""CPU-side checks of the header reader (image-generation_amd/_abi.py) and of the binding built from it: what the reader must
refuse, the hard declarators, every bound function's type list against the reader's, the library's exports against the
prototypes, and the struct layouts -- ``StepState.FORMAT`` among them -- against the typedefs."""
import ctypes
import struct
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import pytest

from image_generation_amd import _abi, _lib, dev


@pytest.mark.parametrize("text,offenders", [
    ("int dvg_f(int a, long x);", ("dvg_f", "'x'", "'long'")),
    ("int dvg_f(struct foo *p);", ("dvg_f", "parameter 1", "struct foo *p")),
    ("int dvg_f(int a, void (*cb)(int));", ("dvg_f", "parameter 2", "(*cb)")),
    ("int dvg_f(unsigned int a);", ("dvg_f", "parameter 1", "unsigned int a")),
    ("int dvg_f(int);", ("dvg_f", "parameter 1")),
    ("int dvg_f(float a[2][3]);", ("dvg_f", "parameter 1")),
    ("int dvg_f(char ***names);", ("dvg_f", "'names'")),
    ("dvg_missing_t *dvg_f(void);", ("dvg_f", "return type", "'dvg_missing_t'")),
    ("typedef struct { long n; } dvg_s_t;", ("dvg_s_t.n", "'long'")),
    ("typedef struct { int a; } dvg_s_t; int dvg_f(dvg_s_t by_value);", ("dvg_f", "'by_value'")),
    ("typedef int dvg_int_t;", ("typedef int dvg_int_t",)),
    ("static inline int dvg_f(void) { return 0; }", ("static inline int dvg_f",)),
    ("#define DVG_TWO_LINES 1 \\\n  + 1\nint dvg_f(void);", ("line continuation",)),
    ("int dvg_f(void)", ("unterminated",)),
], ids=["long", "struct-tag", "function-pointer", "two-word-type", "unnamed", "2d-array", "triple-pointer", "unknown-return",
        "long-field", "struct-by-value", "scalar-typedef", "function-body", "line-continuation", "no-semicolon"])
def test_reader_refuses_what_it_does_not_know_and_names_it(text, offenders):
    with pytest.raises(_lib.DvgError) as err:
        _abi.parse(text, "include/bad.h")
    for word in ("bad.h",) + offenders:
        assert word in str(err.value), (word, str(err.value))


def test_reader_names_a_missing_header():
    with pytest.raises(_lib.DvgError, match=r"no_such\.h.*include.no_such\.h"):
        _abi.read("no_such.h")


def test_reader_on_the_hard_declarators():
    hdr = _abi.parse("""
        /* a comment with int dvg_not_this(void); in it */
        typedef void *dvg_stream_t; // hipStream_t
        typedef struct dvg_graph dvg_graph_t;
        typedef struct {
          const float *conv_w[4], *conv_b[4]; /* pointers */
          float *lin_w, *lin_b, *bn_g[5];
          int64_t *nbt[2];
          uint32_t sweep0; float step[2];
        } dvg_p_t;
        typedef struct { uint64_t offset; } dvg_dev_t;
        int dvg_version(void);
        const char *dvg_name(int index);
        size_t dvg_hard(const dvg_graph_t *g, dvg_graph_t **out, const float *const keep[4], int32_t *rung /* in/out */,
                        const dvg_p_t *p, const dvg_dev_t *dyn, const char *name, int64_t out64[24], void *ws, size_t bytes,
                        double *e, uint8_t *flags, int8_t *state, uint64_t seed, float beta, dvg_stream_t stream);
    """, "include/hard.h", by_address=("dvg_dev_t",))
    P = hdr.structures["dvg_p_t"]
    assert hdr.protos == {
        "dvg_version": (c_int, []),
        "dvg_name": (c_char_p, [("index", c_int)]),
        "dvg_hard": (c_size_t, [
            ("g", c_void_p), ("out", POINTER(c_void_p)), ("keep", POINTER(c_void_p)), ("rung", c_void_p), ("p", POINTER(P)),
            ("dyn", c_void_p), ("name", c_char_p), ("out64", c_void_p), ("ws", c_void_p), ("bytes", c_size_t), ("e", c_void_p),
            ("flags", c_void_p), ("state", c_void_p), ("seed", c_uint64), ("beta", c_float), ("stream", c_void_p)]),
    }
    assert hdr.layouts["dvg_p_t"] == [("conv_w", c_void_p, 4), ("conv_b", c_void_p, 4), ("lin_w", c_void_p, 0), ("lin_b", c_void_p, 0),
                                      ("bn_g", c_void_p, 5), ("nbt", c_void_p, 2), ("sweep0", c_uint32, 0), ("step", c_float, 2)]
    assert P._fields_ == [("conv_w", c_void_p * 4), ("conv_b", c_void_p * 4), ("lin_w", c_void_p), ("lin_b", c_void_p),
                          ("bn_g", c_void_p * 5), ("nbt", c_void_p * 2), ("sweep0", c_uint32), ("step", c_float * 2)]
    assert hdr.layouts["dvg_dev_t"] == [("offset", c_uint64, 0)]


# ------------------------------------------------------------------------------------------------ the binding
def _exported_functions(path):
    """The defined function symbols of an ELF64 shared object's dynamic symbol table."""
    with open(path, "rb") as f:
        elf = f.read()
    assert elf[:6] == b"\x7fELF\x02\x01"  # 64-bit, little-endian
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + k * shentsize) for k in range(shnum)]
    names = set()
    for _name, kind, _flags, _addr, offset, size, link, _info, _align, entsize in sections:
        if kind != 11:  # SHT_DYNSYM
            continue
        strings = sections[link][4]
        for at in range(offset, offset + size, entsize):
            st_name, st_info, _other, st_shndx = struct.unpack_from("<IBBH", elf, at)
            if st_shndx != 0 and st_info & 0xF == 2:  # defined, STT_FUNC
                names.add(elf[strings + st_name: elf.index(b"\0", strings + st_name)].decode())
    return names


def test_every_function_is_bound_as_its_prototype_says():
    _lib.build()
    L = dev.lib()
    protos = {**_abi.read("dvg.h").protos, **_abi.read("dvg_dev.h").protos}
    assert len(_abi.read("dvg.h").protos) >= 75 and len(_abi.read("dvg_dev.h").protos) >= 27
    assert set(protos) == set(_lib.SIGNATURES) | set(_lib.DEV_OPTION_SIGNATURES) | set(dev._SIGS)
    for name, (restype, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == [t for _name, t in params], name
    exported = {s for s in _exported_functions(_lib.LIB_PATH) if s.startswith("dvg_")}
    assert exported == set(protos), (sorted(exported - set(protos)), sorted(set(protos) - exported))


# ------------------------------------------------------------------------------------------------ the struct layouts
def _c_size(layout):
    """sizeof of a C struct of these members on this ABI: every member aligned to its own size, the struct to its widest."""
    at = widest = 0
    for _field, ctype, n in layout:
        size = ctypes.sizeof(ctype)
        at = (at + size - 1) // size * size + size * max(n, 1)
        widest = max(widest, size)
    return (at + widest - 1) // widest * widest


STRUCTURES = {"dvg_mmd_cfg_t": _lib.MmdCfg, "dvg_encoder_params_t": _lib.EncoderParams, "dvg_encoder_grads_t": _lib.EncoderGrads,
              "dvg_decoder_params_t": _lib.DecoderParams, "dvg_decoder_grads_t": _lib.DecoderGrads}


def test_structures_are_the_typedefs():
    hdr = _abi.read("dvg.h")
    assert set(hdr.layouts) == set(STRUCTURES) | {"dvg_step_state_t"}
    for name, cls in STRUCTURES.items():
        assert cls is hdr.structures[name]
        assert [f for f, _t in cls._fields_] == [f for f, _t, _n in hdr.layouts[name]], name
        assert ctypes.sizeof(cls) == _c_size(hdr.layouts[name]), name
    # literal rows: the callers' field names and the sizes the C side was compiled with
    assert _lib.MmdCfg._fields_ == [("n_kernels", c_int32), ("factor", c_float), ("bandwidth", c_float), ("squared", c_int32),
                                    ("reduce_mean", c_int32), ("biased", c_int32)]
    assert [(f, getattr(t, "_length_", 0)) for f, t in _lib.DecoderParams._fields_] == [
        ("lin_w", 0), ("lin_b", 0), ("conv_w", 5), ("conv_b", 5), ("bn_g", 4), ("bn_b", 4), ("bn_rm", 4), ("bn_rv", 4), ("bn_nbt", 4)]
    assert [ctypes.sizeof(c) for c in STRUCTURES.values()] == [24, 240, 144, 256, 160]


def test_step_state_format_is_the_typedef():
    """``StepState.write`` packs by position: field order, widths, array lengths and the total size are the header's."""
    hdr = _abi.read("dvg.h")
    layout = hdr.layouts["dvg_step_state_t"]
    assert [f for f, _t, _n in layout] == ["sweep0", "reserved", "gumbel_offset", "dropout_offset", "adam_step_size", "adam_bc2_sqrt"]
    codes = {c_uint32: "I", c_uint64: "Q", c_float: "f"}
    assert _lib.StepState.FORMAT == "<" + "".join((str(n) if n else "") + codes[t] for _f, t, n in layout)
    size = struct.calcsize(_lib.StepState.FORMAT)  # "<": no padding -- and the C layout has none either
    assert size == _c_size(layout) == ctypes.sizeof(hdr.structures["dvg_step_state_t"]) == 40
    # a pointer to it crosses the boundary as a device address
    assert dict(hdr.protos["dvg_gibbs_sample"][1])["dyn"] is c_void_p


def test_option_names_are_read_once_per_loaded_library():
    _lib.build()
    L = _lib.lib()
    assert _lib._dev_names() is _lib._dev_names() and _lib._dev_names() == set(_lib.dev_options())
    calls = []
    real = L.dvg_dev_option_count
    try:
        L.dvg_dev_option_count = lambda: calls.append(1) or real()
        for _ in range(3):
            assert _lib.get_option("dec_tail_fused") in (0, 1) and _lib.get_option("dec_lc0") == -1
    finally:
        L.dvg_dev_option_count = real
    assert calls == []
    with pytest.raises(_lib.DvgError, match="unknown option"):  # an unknown name still reaches the library
        _lib.get_option("no_such_option")
