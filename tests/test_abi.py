"""CPU-side checks of the C ABI: the library loads and exports every symbol include/dvg.h declares."""
import os
import re
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import pytest

from image_generation_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "dvg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dvg_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
    _lib.build()
    handle = _lib.lib()
    declared = _declared_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/dvg.h but not exported"
    # and the binding table, which is read from the header, covers exactly the header ...
    assert sorted(_lib.SIGNATURES) == declared
    # ... and reads it right: a few rows written out by hand as the types ctypes is given
    P, DP = POINTER(c_void_p), POINTER(_lib.DecoderParams)
    assert _lib.SIGNATURES["dvg_gibbs_sample"] == (c_int, [
        c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_float, c_float, c_void_p, c_int, c_uint32, c_uint64,
        c_uint32, c_int, c_int, c_void_p, c_void_p, c_void_p])
    assert _lib.SIGNATURES["dvg_mmd_fwd_bwd"] == (c_int, [
        c_void_p, c_int64, c_void_p, c_int64, c_int, POINTER(_lib.MmdCfg), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p])
    assert _lib.SIGNATURES["dvg_decoder_fwd_mse_ex"] == (c_int, [
        DP, c_int, c_void_p, c_int64, P, c_uint64, c_uint64, c_void_p, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p,
        c_int, c_void_p])
    assert _lib.SIGNATURES["dvg_packed_distinct"] == (c_int, [
        c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
        c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p])
    assert _lib.SIGNATURES["dvg_packed_distinct_workspace_bytes"] == (c_size_t, [c_int64, c_int64, c_int])
    assert _lib.SIGNATURES["dvg_source_hash"] == (c_char_p, [])


def test_version_and_error_string():
    L = _lib.lib()
    assert L.dvg_version() >= 100
    assert isinstance(L.dvg_last_error(), bytes)
    assert L.dvg_prof_num_kernels() > 10
    names = {L.dvg_prof_kernel_name(i).decode() for i in range(L.dvg_prof_num_kernels())}
    assert "gibbs_sweeps" in names and "conv_igemm_kernel<64,64,2,2,1>" in names


def test_argument_validation_without_gpu():
    """Bad arguments are rejected before any device work (safe on a CPU-only box)."""
    L = _lib.lib()
    rc = L.dvg_adam_step(None, None, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None, 0, None)
    assert rc == -1 and b"null" in L.dvg_last_error()
    rc = L.dvg_gibbs_sample(None, None, None, 1.0, -1, 1, -1, 1, 1.0, None, 4, 0, 0, 0, 1, 1, None, None, None)
    assert rc == -1


def test_missing_library_is_loud(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.DvgError, match="no CPU fallback"):
        _lib.lib()


def test_kernel_form_options_live_in_the_abi_not_in_the_environment():
    """dvg_set_option / dvg_get_option / dvg_reset_options (include/dvg.h): every option has a name, a documented meaning
    and a default; unknown names are errors; and no source file of the library reads the environment any more."""
    opts, dev = _lib.options(), _lib.dev_options()
    assert {"igemm_posmajor", "dec_d22", "dec_lc0", "side_stream", "enc_wino", "enc_wino4"} <= set(opts)
    assert {"igemm_dma", "wgrad_dma", "mmd_w128", "enc_l0_fused", "dec_tail_fused", "wino_dynamic"} <= set(dev)
    assert not set(opts) & set(dev)
    assert all(doc for _v, doc in opts.values()) and all(doc for _v, doc in dev.values())
    assert opts["dec_lc0"][0] == -1 and dev["igemm_dma"][0] == 1
    with _lib.option_scope(dec_lc0=0, igemm_posmajor=0, igemm_dma=0):
        assert _lib.get_option("dec_lc0") == 0 and _lib.get_option("igemm_posmajor") == 0 and _lib.get_option("igemm_dma") == 0
    assert _lib.get_option("dec_lc0") == -1 and _lib.get_option("igemm_posmajor") == 1 and _lib.get_option("igemm_dma") == 1
    with pytest.raises(_lib.DvgError, match="unknown option"):
        _lib.set_option("no_such_option", 1)
    # the two name spaces are apart at the C boundary: a dev knob is not reachable through dvg_set_option
    assert _lib.lib().dvg_set_option(b"igemm_dma", 0) != 0 and _lib.lib().dvg_dev_set_option(b"dec_lc0", 0) != 0
    _lib.set_option("igemm_thr128", 128)
    _lib.check(_lib.lib().dvg_reset_options())
    assert _lib.get_option("igemm_thr128") == 512
    # round 6: the boundary (include/dvg.h) carries at most 8 switches; the A/B references a default replaced and the test
    # knobs (round 5: 16 switches in one list) sit behind include/dvg_dev.h
    assert len(opts) <= 8, sorted(opts)
    src = os.path.join(ROOT, "image-generation_amd", "csrc")
    offenders = [f for f in os.listdir(src) if os.path.isfile(os.path.join(src, f))
                 and "getenv(" in open(os.path.join(src, f)).read().replace("getenv() sites", "")]
    assert offenders == [], offenders
