"""CPU-side checks of G.711 in the PCM gateway (include/nutls.h, "PCM gateway", G.711): the two format constants and the two host-only
helpers are declared, exported, bound and listed; ``nutls_pcm_g711_expand`` / ``nutls_pcm_g711_compress`` equal the numpy statement of the
header's rule (tests/g711_reference.py) for all 256 codes and all 65 536 int16 values of both laws, and CPython's ``audioop`` where it can be
imported; the algebra the header documents holds; refusals name the entry and write nothing; the Python wrappers refuse a codec that does not
go with the samples before they touch the library.  No reference counterpart: the reference takes float samples at 16 kHz only
(dnn_model/interpreter_proposed.py:384-385)."""
import ctypes
import os
import re

import numpy as np
import pytest

import g711_reference as G
from nunet_amd import runner
from nunet_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = {"ulaw": 2, "alaw": 3}
ALL_S16 = np.arange(-32768, 32768).astype(np.int16)
SIGNATURES = {
    "nutls_pcm_g711_expand": "int sample_format, short* table, int n",
    "nutls_pcm_g711_compress": "int sample_format, const short* in, unsigned char* out, size_t n",
}


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def sp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_short))


def bp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))


def test_the_constants_and_helpers_are_declared_exported_bound_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    assert re.search(r"^#define NUTLS_PCM_ULAW 2\b", hdr, re.M) and re.search(r"^#define NUTLS_PCM_ALAW 3\b", hdr, re.M)
    assert re.search(r"^#define NUTLS_PCM_F32 0\b", hdr, re.M) and re.search(r"^#define NUTLS_PCM_S16 1\b", hdr, re.M)      # (as they were)
    declared = dict(re.findall(r"^int (nutls_[a-z_0-9]+)\(([^)]*)\);", hdr, re.M))
    for name, params in SIGNATURES.items():
        assert " ".join(declared.get(name, "").split()) == params, name
        # listed -- beside ABI_SYMBOLS: test_abi.py finds the header's names by a pattern without digits, and compares that tuple with them
        assert name in runner.ABI_SYMBOLS_G711 and name not in runner.ABI_SYMBOLS, name
        fn = getattr(lib, name)      # AttributeError: not exported
        assert fn.argtypes is not None and len(fn.argtypes) == params.count(",") + 1 and fn.restype is ctypes.c_int, name
    assert runner._PcmFormat._PCM_FORMATS == {"float32": 0, "int16": 1, "ulaw": 2, "alaw": 3}
    assert runner.G711_CODECS == FMT and runner.G711_SILENCE == G.SILENCE
    # the header spells the rule out, and says silence where it says zeros
    flat = " ".join(hdr.replace("\n * ", " ").split())
    for text in ("u = ~c & 0xFF; t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4); s = (u & 0x80) ? 0x84 - t : t - 0x84",
                 "a = c ^ 0x55; t = (a & 15) << 4; g = (a & 0x70) >> 4; t = g == 0 ? t + 8 : (t + 0x108) << (g - 1); s = (a & 0x80) ? t : -t",
                 "v = min(v, 8159) + 33", "(seg >= 8 ? 0x7F : (seg << 4) | ((v >> (seg + 1)) & 15)) ^ mask",
                 "(seg >= 8 ? 0x7F : (seg << 4) | ((seg < 2 ? v >> 1 : v >> seg) & 15)) ^ mask", "0xFF (mu-law) or 0xD5 (A-law)"):
        assert text in flat, text
    assert flat.count("silence code") >= 5


@pytest.mark.parametrize("codec", G.CODECS)
def test_expand_and_compress_equal_the_rule_for_every_code_and_every_int16(lib, codec):
    table = np.full(256, 77, np.int16)
    assert lib.nutls_pcm_g711_expand(FMT[codec], sp(table), 256) == 0
    assert np.array_equal(table, G.expand(codec))
    assert int(np.abs(table.astype(np.int32)).max()) == G.PEAK[codec]
    codes = np.zeros(65536, np.uint8)
    assert lib.nutls_pcm_g711_compress(FMT[codec], sp(ALL_S16), bp(codes), 65536) == 0
    assert np.array_equal(codes, G.compress(codec, ALL_S16))
    # the Python wrappers are the same two calls
    assert np.array_equal(runner.g711_expand(codec), table) and runner.g711_expand(codec).dtype == np.int16
    got = runner.g711_compress(codec, ALL_S16.reshape(256, 256))
    assert got.dtype == np.uint8 and got.shape == (256, 256) and np.array_equal(got.ravel(), codes)


@pytest.mark.parametrize("codec", G.CODECS)
def test_expand_and_compress_equal_audioop(codec):
    audioop = pytest.importorskip("audioop")
    to_lin, from_lin = (audioop.ulaw2lin, audioop.lin2ulaw) if codec == "ulaw" else (audioop.alaw2lin, audioop.lin2alaw)
    assert np.array_equal(np.frombuffer(to_lin(bytes(range(256)), 2), np.int16), runner.g711_expand(codec))
    assert np.array_equal(np.frombuffer(from_lin(ALL_S16.tobytes(), 2), np.uint8), runner.g711_compress(codec, ALL_S16))


@pytest.mark.parametrize("codec", G.CODECS)
def test_the_algebra_the_header_documents(codec):
    table = runner.g711_expand(codec)
    codes = runner.g711_compress(codec, ALL_S16)
    every = np.arange(256, dtype=np.uint8)
    # expand o compress is the identity on expand's range
    assert np.array_equal(table[runner.g711_compress(codec, table)], table)
    # compress o expand is the identity on the codes, but for mu-law's negative zero
    want = every.copy()
    if codec == "ulaw":
        want[0x7F] = 0xFF
        assert 0x7F not in set(codes.tolist()) and len(set(codes.tolist())) == 255
    else:
        assert len(set(codes.tolist())) == 256
    assert np.array_equal(runner.g711_compress(codec, table), want)
    # silence: what 0 compresses to, and what that expands to
    zero = runner.g711_compress(codec, np.zeros(1, np.int16))[0]
    assert zero == G.SILENCE[codec] == runner.G711_SILENCE[codec]
    assert int(table[zero]) == (0 if codec == "ulaw" else 8)
    assert int(table[0]) == (-32124 if codec == "ulaw" else -5504)      # a zero BYTE is not silence
    # monotone in s, measured on the expanded value
    back = table[codes].astype(np.int32)
    assert np.all(np.diff(back) >= 0)
    assert back[0] == -G.PEAK[codec] and back[-1] == G.PEAK[codec]


def test_refusals_name_the_entry_and_write_nothing(lib):
    table, codes, s = np.full(300, 77, np.int16), np.full(16, 77, np.uint8), np.arange(16, dtype=np.int16)
    for call in (lambda: lib.nutls_pcm_g711_expand(0, sp(table), 256), lambda: lib.nutls_pcm_g711_expand(1, sp(table), 256),
                 lambda: lib.nutls_pcm_g711_expand(4, sp(table), 256), lambda: lib.nutls_pcm_g711_expand(-1, sp(table), 256),
                 lambda: lib.nutls_pcm_g711_expand(2, None, 256), lambda: lib.nutls_pcm_g711_expand(2, sp(table), 255),
                 lambda: lib.nutls_pcm_g711_expand(3, sp(table), 257), lambda: lib.nutls_pcm_g711_expand(3, sp(table), 0)):
        assert call() == runner.NUTLS_ERR_ARG
        assert b"nutls_pcm_g711_expand" in lib.nutls_last_error(), lib.nutls_last_error()
    for call in (lambda: lib.nutls_pcm_g711_compress(0, sp(s), bp(codes), 16), lambda: lib.nutls_pcm_g711_compress(1, sp(s), bp(codes), 16),
                 lambda: lib.nutls_pcm_g711_compress(4, sp(s), bp(codes), 16), lambda: lib.nutls_pcm_g711_compress(2, None, bp(codes), 16),
                 lambda: lib.nutls_pcm_g711_compress(3, sp(s), None, 16)):
        assert call() == runner.NUTLS_ERR_ARG
        assert b"nutls_pcm_g711_compress" in lib.nutls_last_error(), lib.nutls_last_error()
    assert np.all(table == 77) and np.all(codes == 77), "a refused call wrote"
    # a null handle is an argument error of nutls_set_pcm_format whatever the format
    for fmt in (2, 3):
        assert lib.nutls_set_pcm_format(None, 8000, fmt) == runner.NUTLS_ERR_ARG
        assert b"nutls_set_pcm_format" in lib.nutls_last_error()
    for bad in (lambda: runner.g711_expand("pcmu"), lambda: runner.g711_expand(2), lambda: runner.g711_compress("int16", s),
                lambda: runner.g711_compress("ulaw", s.astype(np.int32)), lambda: runner.g711_compress("alaw", s.astype(np.float32))):
        with pytest.raises(ValueError):
            bad()


def test_python_refuses_a_codec_that_does_not_go_with_the_samples_before_the_library():
    off = runner.NutlsOffline.__new__(runner.NutlsOffline)      # no handle, no library: whatever reaches for either fails with AttributeError
    off.utterances, off.max_frames = 1, 8
    f, s, b = np.zeros(300, np.float32), np.zeros(300, np.int16), np.full(300, 0xFF, np.uint8)
    for wave, rate, codec in ((f, 8000, "ulaw"), (s, 8000, "alaw"),          # a codec with samples that are no codes
                              (b, 8000, None),                                # codes without a codec
                              (b, 16000, "ulaw"), (b, 48000, "alaw"), (b, 8000.0, "ulaw"),      # G.711 is 8 kHz
                              (b, 8000, "pcmu"), (b, 8000, 2), (b, 8000, "")):                  # no such codec
        with pytest.raises(ValueError):
            off.enhance_wave(wave, rate, codec=codec)
    with pytest.raises(ValueError):
        off.enhance_many([b, b], rate=8000)                # enhance_many keeps its signature: codes go through enhance_many_codec
    for waves, codec, rate in (([f], "ulaw", 8000), ([b, s], "alaw", 8000), ([b], "ulaw", 16000), ([b], "g711", 8000), ([b], None, 8000),
                               ([], "ulaw", 32000), ([np.zeros((2, 300), np.uint8)], "ulaw", 8000)):
        with pytest.raises(ValueError):
            off.enhance_many_codec(waves, codec, rate=rate)
    with pytest.raises(ValueError):
        off.enhance_many_codec([b], "ulaw", dc_mode="middle")
    with pytest.raises(ValueError):
        off.enhance_many_codec([b, b], "ulaw", atten_lim_db=[6.0])
    import inspect
    wave = inspect.signature(runner.NutlsOffline.enhance_wave).parameters
    assert wave["codec"].default is None and list(wave)[:4] == ["self", "wave", "rate", "dc_mode"]
    many = inspect.signature(runner.NutlsOffline.enhance_many_codec).parameters
    assert list(many) == ["self", "waves", "codec", "dc_mode", "rate", "atten_lim_db"] and many["rate"].default == 8000
    off._h = None      # (nothing for __del__ to close)
