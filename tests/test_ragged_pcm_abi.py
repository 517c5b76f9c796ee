"""CPU-side checks of the ragged blocks in the callers' format (include/nutls.h, "PCM gateway", the ``_pcm_ragged`` entries): the four
entries are declared with the documented signatures, exported and bound, they refuse a null handle before touching a device, the header
no longer puts them out of scope, and ``NutlsOffline.enhance_many(rate=...)`` refuses mixed dtypes and unsupported rates before it touches
the library.  No reference counterpart: the reference enhances one float recording at 16 kHz at a time
(dnn_model/interpreter_proposed.py:203-370, 384-385)."""
import ctypes
import os
import re

import numpy as np
import pytest

from nunet_amd import runner
from nunet_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "nutls_enhance_block_pcm_ragged": "nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream",
    "nutls_enhance_block_pcm_ragged_host": "nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, const int* hops, int dc_mode",
    "nutls_pcm_decode_block_ragged": "nutls_handle* h, const void* pcm_in, float* wave_out, int n_hops, const int* hops, void* stream",
    "nutls_pcm_encode_block_ragged": "nutls_handle* h, const float* wave_in, void* pcm_out, int n_hops, const int* hops, void* stream",
}


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def test_the_four_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    declared = dict(re.findall(r"^int (nutls_[a-z_0-9]+)\(([^)]*)\);", hdr, re.M))
    for name, params in SIGNATURES.items():
        assert " ".join(declared.get(name, "").split()) == params, name
        assert name in runner.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == params.count(",") + 1 and fn.restype is ctypes.c_int, name
    import inspect
    for method in ("enhance_block_pcm_device", "pcm_decode_block_device", "pcm_encode_block_device"):
        assert inspect.signature(getattr(runner.NutlsOffline, method)).parameters["hops"].default is None, method
    many = inspect.signature(runner.NutlsOffline.enhance_many).parameters
    assert list(many)[1:] == ["waves", "dc_mode", "rate"] and many["rate"].default is None and many["dc_mode"].default == "edge"
    assert "no ragged" not in " ".join(hdr.split()), "the header still lists ragged blocks in the callers' format as unsupported"
    assert "ero-copy reads of pinned PCM stay out of scope" in " ".join(hdr.replace("\n * ", " ").split())


def test_a_null_handle_is_an_argument_error_with_a_message(lib):
    x = np.zeros(768, np.float32)
    cnt = np.zeros(1, np.int32)
    a, c, ip = x.ctypes.data, cnt.ctypes.data, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    calls = {
        "nutls_enhance_block_pcm_ragged": lambda f: f(None, a, a, 1, c, 0, None),
        "nutls_enhance_block_pcm_ragged_host": lambda f: f(None, a, a, 1, ip, 0),
        "nutls_pcm_decode_block_ragged": lambda f: f(None, a, a, 1, c, None),
        "nutls_pcm_encode_block_ragged": lambda f: f(None, a, a, 1, c, None),
    }
    assert set(calls) == set(SIGNATURES)
    for name, call in calls.items():
        assert call(getattr(lib, name)) == runner.NUTLS_ERR_ARG, name
        msg = lib.nutls_last_error()
        assert name.encode() in msg and b"null" in msg, (name, msg)


def test_enhance_many_refuses_mixed_dtypes_and_unsupported_rates_before_the_library():
    off = runner.NutlsOffline.__new__(runner.NutlsOffline)      # no handle, no library: whatever reaches for either fails with AttributeError
    off.utterances, off.max_frames = 3, 8
    f, s = np.zeros(300, np.float32), np.zeros(300, np.int16)
    for waves, rate in (([f, s], 8000), ([s, f, s], 48000),           # mixed
                        ([f.astype(np.float64)], 8000), ([s.astype(np.int32)], 8000),      # neither int16 nor float32
                        ([s, s], 44100), ([f], 0), ([f], 16000.5), ([s], "8000"),          # no supported rate
                        ([np.zeros((2, 300), np.int16)], 8000)):                           # not one-dimensional
        with pytest.raises(ValueError):
            off.enhance_many(waves, rate=rate)
    with pytest.raises(ValueError):
        off.enhance_many([s], dc_mode="middle", rate=8000)
    off._h = None      # (nothing for __del__ to close)
