"""CPU checks of the PCM gateway's upper band (include/nutls.h, "Upper band"): the two entries exist at every layer, refuse a null handle by
name, the crossover 1 - H^2 of the library's own prototype is what the header says, and the float64 helper the GPU tests trust
(tests/pcm_upper_reference.py) has its delays right."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
from scipy import signal

from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner
from nunet_amd.build import build

import pcm_upper_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def test_the_entries_exist_at_every_layer(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    assert re.search(r"\bint\s+nutls_set_pcm_upper_band\s*\(\s*nutls_handle\s*\*\s*h\s*,\s*float\s+gain\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+nutls_pcm_upper_band\s*\(\s*nutls_handle\s*\*\s*h\s*,\s*float\s*\*\s*gain\s*\)\s*;", hdr)
    for name, argtypes in (("nutls_set_pcm_upper_band", [ctypes.c_void_p, ctypes.c_float]),
                           ("nutls_pcm_upper_band", [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)])):
        assert name in runner.ABI_SYMBOLS
        fn = getattr(lib, name)      # AttributeError: not exported
        assert list(fn.argtypes) == argtypes and fn.restype is ctypes.c_int
    for cls in (NutlsEngine, NutlsOffline):
        assert list(inspect.signature(cls.set_pcm_upper_band).parameters) == ["self", "gain"]
        assert isinstance(inspect.getattr_static(cls, "pcm_upper_band"), property)
    assert inspect.signature(NutlsOffline.enhance_wave).parameters["upper_gain"].default == 0.0


def test_a_null_handle_is_refused_by_name(lib):
    g = ctypes.c_float(7.0)
    for call, name in ((lambda: lib.nutls_set_pcm_upper_band(None, 0.5), b"nutls_set_pcm_upper_band"),
                       (lambda: lib.nutls_pcm_upper_band(None, ctypes.byref(g)), b"nutls_pcm_upper_band")):
        assert lib.nutls_batch(None) == runner.NUTLS_ERR_ARG and name not in lib.nutls_last_error()      # (another text in the one error slot)
        assert call() == runner.NUTLS_ERR_ARG
        assert name in lib.nutls_last_error()
    assert g.value == 7.0


@pytest.mark.parametrize("rate", [32000, 48000])
def test_the_crossover_is_the_prototypes_own(rate):
    """|1 - |H|^2| from the library's taps alone, float64 freqz; frequencies in units of 8 kHz."""
    q = rate // 16000
    p = runner.pcm_filter(rate).astype(np.float64)
    assert len(p) == 2 * R.K * q + 1
    f = np.linspace(0.0, q, 8 * 4096 + 1)      # 0 .. the caller's Nyquist frequency
    # D filters with p and keeps every q-th sample, E zero-stuffs and filters with q p: the alias-free part of E(D(x)) is (1 / q) H (q H) = H^2,
    # H the response of p (sum 1, linear phase: H^2 = |H|^2 once the delay 2 K q is taken out, which u's delayed input does)
    _, h = signal.freqz(p, worN=f * np.pi / q)
    cross_db = 20 * np.log10(np.maximum(np.abs(1.0 - np.abs(h) ** 2), 1e-300))
    low = cross_db[f <= 0.85].max()
    print("q = %d: |1 - |H|^2| <= %.2f dB on [0, 0.85]; %.2f dB at 0.95, %.2f dB at 1.0; [%.4f, %.4f] dB on [1.15, q]" % (
        q, low, cross_db[np.argmin(np.abs(f - 0.95))], cross_db[np.argmin(np.abs(f - 1.0))], cross_db[f >= 1.15].min(), cross_db[f >= 1.15].max()))
    assert low <= -70.0
    assert np.all(np.abs(cross_db[f >= 1.15]) <= 0.1)


@pytest.mark.parametrize("rate", [32000, 48000])
def test_the_references_identity(rate):
    """With M the identity and g = 1 the output is the delayed input, whatever the filter: algebra, to float64 rounding."""
    q, S = rate // 16000, 256 * rate // 16000
    rng = np.random.default_rng(rate)
    x = rng.standard_normal((2, 7 * S))
    p = runner.pcm_filter(rate).astype(np.float64)
    d = R.decode64(p, x, q)
    tol = 1e-12 * np.abs(x).max()
    out, bound = R.encode_with_upper(d, x, rate, 1.0, hop_lag=0)
    assert out.shape == x.shape == bound.shape and np.all(bound >= 0) and np.all(bound[:, 4 * R.K * q:] > 0)
    assert np.abs(out - R.delayed(x, 2 * R.K * q)).max() <= tol
    # the model's one-hop lag: the encode half is handed D(x) one hop late and adds the upper band of the hop in front
    out1, _ = R.encode_with_upper(R.delayed(d, 256), x, rate, 1.0)
    assert np.abs(out1 - R.delayed(x, 2 * R.K * q + S)).max() <= tol
    # and the helper's u is what it says: with g = 0 nothing is added, with y = 0 the output is g u
    out0, _ = R.encode_with_upper(d, x, rate, 0.0)
    assert np.array_equal(out0, R.encode64(p, d, q))
    outu, _ = R.encode_with_upper(np.zeros_like(d), x, rate, 0.5, hop_lag=0)
    assert np.abs(outu - 0.5 * R.upper_band(x, rate)).max() <= tol
    assert R.roundings(rate) == 2 * 24 * q + 2 * 24 + 4
