"""CPU-side checks of the PCM gateway (include/nutls.h, "PCM gateway"): the prototype filters the conversion kernels use meet the
contract's conditions (checked from ``nutls_pcm_filter`` alone with a float64 ``freqz``), the entries are declared, exported, bound and
listed, the two new translation units are sources of the library, and every entry refuses a null handle -- with its own name in the
message -- before touching a device.  No reference counterpart: the reference refuses anything but float samples at 16 kHz
(dnn_model/interpreter_proposed.py:384-385)."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import signal

from nunet_amd import runner
from nunet_amd.build import SOURCES, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 24
HANDLE_ENTRIES = (
    "nutls_set_pcm_format", "nutls_pcm_hop_samples", "nutls_pcm_delay_samples",
    "nutls_enhance_hop_pcm", "nutls_enhance_hop_pcm_active", "nutls_enhance_hop_pcm_host", "nutls_enhance_hop_pcm_host_active",
    "nutls_pcm_decode_hop", "nutls_pcm_encode_hop",
    "nutls_enhance_block_pcm", "nutls_enhance_block_pcm_host", "nutls_pcm_decode_block", "nutls_pcm_encode_block",
)
HOST_ONLY = ("nutls_pcm_filter_taps", "nutls_pcm_filter")


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def ratio(rate):
    return max(rate, 16000) // min(rate, 16000)


@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_the_prototype_filter_meets_the_contract(lib, rate):
    q = ratio(rate)
    assert lib.nutls_pcm_filter_taps(rate) == 2 * K * q + 1
    p = runner.pcm_filter(rate)
    assert p.dtype == np.float32 and p.shape == (2 * K * q + 1,)
    assert np.array_equal(p.view(np.uint32), p[::-1].view(np.uint32)), "the taps are not symmetric to the bit"
    p64 = p.astype(np.float64)

    def gain_db(f):      # f in units of the lower rate's Nyquist frequency; the filter runs at q times that rate
        _, h = signal.freqz(p64, worN=np.pi * np.asarray(f, np.float64) / q)
        return 20 * np.log10(np.maximum(np.abs(h), 1e-300))

    passband = gain_db(np.linspace(0.0, 0.85, 4001))
    stopband = gain_db(np.linspace(1.15, q, 8001))
    edge = float(gain_db([1.0])[0])
    print("rate %d: passband deviation %.5f dB, stopband %.2f dB, at the band edge %.3f dB" % (rate, np.abs(passband).max(), stopband.max(), edge))
    assert np.abs(passband).max() <= 0.01
    assert stopband.max() <= -80.0
    assert abs(edge - 20 * np.log10(0.5)) <= 0.1


def test_sixteen_kilohertz_is_the_single_tap_one_and_other_rates_are_refused(lib):
    assert lib.nutls_pcm_filter_taps(16000) == 1
    assert np.array_equal(runner.pcm_filter(16000), np.ones(1, np.float32))
    assert lib.nutls_pcm_filter_taps(44100) == -1
    buf = np.zeros(256, np.float32)
    assert lib.nutls_pcm_filter(44100, runner._fptr(buf), 97) == runner.NUTLS_ERR_ARG
    assert lib.nutls_pcm_filter(48000, runner._fptr(buf), 97) == runner.NUTLS_ERR_ARG      # 48 kHz has 145 taps
    assert b"nutls_pcm_filter" in lib.nutls_last_error()
    assert lib.nutls_pcm_filter(8000, runner._fptr(buf), 96) == runner.NUTLS_ERR_ARG
    assert lib.nutls_pcm_filter(8000, None, 97) == runner.NUTLS_ERR_ARG
    assert not buf.any(), "a refused call wrote taps"
    with pytest.raises(ValueError):
        runner.pcm_filter(44100)


def test_the_symbols_are_declared_exported_bound_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    declared = dict(re.findall(r"^int (nutls_[a-z_]+)\(([^)]*)\);", hdr, re.M))
    for name in HANDLE_ENTRIES + HOST_ONLY:
        assert name in declared, name
        assert name in runner.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == declared[name].count(",") + 1 and fn.restype is ctypes.c_int, name
    assert re.search(r"^#define NUTLS_PCM_F32 0\b", hdr, re.M) and re.search(r"^#define NUTLS_PCM_S16 1\b", hdr, re.M)
    assert "pcm.hip" in SOURCES and "api_pcm.cpp" in SOURCES
    for method in ("set_pcm_format", "enhance_hop_pcm", "pcm_decode_hop", "pcm_encode_hop"):
        assert callable(getattr(runner.NutlsEngine, method)), method
    for method in ("set_pcm_format", "enhance_block_pcm_device", "pcm_decode_block_device", "pcm_encode_block_device", "enhance_wave"):
        assert callable(getattr(runner.NutlsOffline, method)), method
    for cls in (runner.NutlsEngine, runner.NutlsOffline):
        assert isinstance(cls.pcm_hop_samples, property) and isinstance(cls.pcm_delay_samples, property)


def test_a_null_handle_is_an_argument_error_that_names_the_entry(lib):
    x = np.zeros(768, np.float32)
    a, m = x.ctypes.data, np.ones(4, np.uint8).ctypes.data
    calls = {
        "nutls_set_pcm_format": lambda f: f(None, 48000, 1),
        "nutls_pcm_hop_samples": lambda f: f(None),
        "nutls_pcm_delay_samples": lambda f: f(None),
        "nutls_enhance_hop_pcm": lambda f: f(None, a, a, 0, None),
        "nutls_enhance_hop_pcm_active": lambda f: f(None, a, a, m, 0, None),
        "nutls_enhance_hop_pcm_host": lambda f: f(None, a, a, 0),
        "nutls_enhance_hop_pcm_host_active": lambda f: f(None, a, a, m, 0),
        "nutls_pcm_decode_hop": lambda f: f(None, a, a, None, None),
        "nutls_pcm_encode_hop": lambda f: f(None, a, a, None, None),
        "nutls_enhance_block_pcm": lambda f: f(None, a, a, 1, 0, None),
        "nutls_enhance_block_pcm_host": lambda f: f(None, a, a, 1, 0),
        "nutls_pcm_decode_block": lambda f: f(None, a, a, 1, None),
        "nutls_pcm_encode_block": lambda f: f(None, a, a, 1, None),
    }
    assert set(calls) == set(HANDLE_ENTRIES)
    for name, call in calls.items():
        assert call(getattr(lib, name)) == runner.NUTLS_ERR_ARG, name
        assert name.encode() in lib.nutls_last_error(), (name, lib.nutls_last_error())
    # the masked entries name themselves with a null mask too (where they would otherwise be the unmasked entry)
    assert lib.nutls_enhance_hop_pcm_active(None, a, a, None, 0, None) == runner.NUTLS_ERR_ARG
    assert b"nutls_enhance_hop_pcm_active" in lib.nutls_last_error()
    assert lib.nutls_enhance_hop_pcm_host_active(None, a, a, None, 0) == runner.NUTLS_ERR_ARG
    assert b"nutls_enhance_hop_pcm_host_active" in lib.nutls_last_error()
