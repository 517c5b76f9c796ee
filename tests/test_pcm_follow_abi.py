"""CPU checks of the PCM gateway's following upper-band gain (include/nutls.h, "Upper band", follow): the three entries exist at every layer and
refuse a null handle by name, the float64 restatement the GPU tests trust (tests/pcm_follow_reference.py) has its windows, its clamp and its
ramp right, and the designed inputs of the GPU tests exercise what they are meant to."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner
from nunet_amd.build import build

import pcm_follow_reference as F
import pcm_upper_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def test_the_entries_exist_at_every_layer(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    assert re.search(r"#define\s+NUTLS_PCM_FOLLOW_HOPS\s+4\b", hdr) and F.W == 4
    assert re.search(r"\bint\s+nutls_set_pcm_upper_follow\s*\(\s*nutls_handle\s*\*\s*h\s*,\s*int\s+enable\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+nutls_pcm_upper_follow\s*\(\s*nutls_handle\s*\*\s*h\s*,\s*int\s*\*\s*enable\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+nutls_pcm_follow_gain\s*\(\s*nutls_handle\s*\*\s*h\s*,\s*float\s*\*\s*gains\s*,\s*int\s+n\s*\)\s*;", hdr)
    assert "Zero-copy reads of pinned PCM stay out of scope" in hdr
    assert not re.search(r"Out of scope: a gain that follows", hdr)
    for name, argtypes in (("nutls_set_pcm_upper_follow", [ctypes.c_void_p, ctypes.c_int]),
                           ("nutls_pcm_upper_follow", [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
                           ("nutls_pcm_follow_gain", [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int])):
        assert name in runner.ABI_SYMBOLS
        fn = getattr(lib, name)      # AttributeError: not exported
        assert list(fn.argtypes) == argtypes and fn.restype is ctypes.c_int
    for cls in (NutlsEngine, NutlsOffline):
        assert list(inspect.signature(cls.set_pcm_upper_follow).parameters) == ["self", "enable"]
        assert isinstance(inspect.getattr_static(cls, "pcm_upper_follow"), property)
        assert list(inspect.signature(cls.pcm_follow_gain).parameters) == ["self"]
        assert list(inspect.signature(cls.set_pcm_upper_band).parameters) == ["self", "gain"]      # (as it was)
    wave = inspect.signature(NutlsOffline.enhance_wave).parameters
    assert list(wave)[-1] == "upper_follow" and wave["upper_follow"].default is False
    assert list(inspect.signature(NutlsOffline.enhance_many).parameters) == ["self", "waves", "dc_mode", "rate"]      # (as it was)
    assert "set_pcm_upper_follow" in NutlsOffline.enhance_many.__doc__


def test_a_null_handle_is_refused_by_name(lib):
    on, g = ctypes.c_int(7), (ctypes.c_float * 3)(7.0, 7.0, 7.0)
    for call, name in ((lambda: lib.nutls_set_pcm_upper_follow(None, 1), b"nutls_set_pcm_upper_follow"),
                       (lambda: lib.nutls_pcm_upper_follow(None, ctypes.byref(on)), b"nutls_pcm_upper_follow"),
                       (lambda: lib.nutls_pcm_follow_gain(None, g, 3), b"nutls_pcm_follow_gain")):
        assert lib.nutls_batch(None) == runner.NUTLS_ERR_ARG and name not in lib.nutls_last_error()      # (another text in the one error slot)
        assert call() == runner.NUTLS_ERR_ARG
        assert name in lib.nutls_last_error()
    assert on.value == 7 and list(g) == [7.0, 7.0, 7.0]


@pytest.mark.parametrize("rate", [32000, 48000])
def test_the_references_identities(rate):
    """y = c * (d one hop late): the windows of a and b hold the same energies, so r = c from hop 1 on -- g = gain * min(c, 1)."""
    q, S, gain = rate // 16000, F.hop_len(rate), 0.75
    rng = np.random.default_rng(rate)
    x = rng.standard_normal((2, 7 * S))
    d = R.decode64(R.taps_of(rate), x, q)
    for c, want in ((1.0, gain), (0.25, 0.25 * gain), (2.0, gain)):
        g, gamma, out, bound = F.follow(d, c * R.delayed(d, 256), x, rate, gain)
        assert g.shape == (2, 7) and gamma.shape == out.shape == bound.shape == x.shape and np.all(bound >= 0)
        assert np.all(g[:, 0] == 0.0)                                  # nothing decoded, nothing handed over: B = 0
        assert np.abs(g[:, 1:] - want).max() <= 1e-12                  # hop 1: A = a_0, B = c^2 a_0
        assert np.abs(gamma[:, 2 * S:] - want).max() <= 1e-12          # from hop 2 on the ramp stands still
        fixed, _ = R.encode_with_upper(c * R.delayed(d, 256), x, rate, want)
        assert np.abs(out[:, 2 * S:] - fixed[:, 2 * S:]).max() <= 1e-12 * np.abs(x).max()
    # the windows: W hops, b's ending at the hop, a's one hop earlier (the model's lag)
    a, b = F.energies(d), F.energies(0.5 * d)
    A, B, _ = F.windows(d, 0.5 * d)
    t = 5
    assert np.allclose(A[:, t + 1], a[:, t - 4:t].sum(axis=1), rtol=1e-14) and np.allclose(B[:, t + 1], b[:, t - 3:t + 1].sum(axis=1), rtol=1e-14)
    assert np.all(A[:, 0] == 0) and np.all(B[:, 0] == 0) and np.all(A[:, 1] == 0) and np.allclose(B[:, 1], b[:, 0])


@pytest.mark.parametrize("rate", [32000, 48000])
def test_gamma_is_continuous_at_hop_edges(rate):
    S = F.hop_len(rate)
    w = F.ramp(S)
    assert w[-1] == 1.0 and np.all(np.diff(w) > 0) and np.abs(w - np.arange(1, S + 1) / S).max() <= 2.0 ** -23
    x = F.designed_x(rate).astype(np.float64)
    d = R.decode64(R.taps_of(rate), x, rate // 16000).astype(np.float32)
    g, gamma, _, _ = F.follow(d, F.designed_y(d), x, rate, 1.0)
    gm = gamma.reshape(F.ROWS, F.HOPS, S)
    assert np.abs(gm[:, :, -1] - g).max() <= 1e-12                     # a hop's ramp ends at its own gain ...
    delta = np.diff(np.concatenate([np.zeros((F.ROWS, 1)), g], axis=1), axis=1)
    start = gm[:, :, 0] - delta * w[0]                                 # ... and the next one starts there: no step at a hop edge
    assert np.abs(start[:, 1:] - gm[:, :-1, -1]).max() <= 1e-12 and np.abs(start[:, 0]).max() <= 1e-12
    assert np.abs(np.diff(gamma, axis=1)).max() <= np.abs(delta).max() * max(np.diff(w).max(), w[0]) + 1e-12


@pytest.mark.parametrize("rate", [32000, 48000])
def test_the_designed_inputs_do_what_they_are_for(rate):
    """What tests/test_gpu_pcm_follow.py feeds: no window near the floor, the clamp reached, a deep suppression reached."""
    x = F.designed_x(rate).astype(np.float64)
    d = R.decode64(R.taps_of(rate), x, rate // 16000).astype(np.float32)
    y = F.designed_y(d)
    assert y.dtype == np.float32 and y.shape == d.shape == (F.ROWS, F.HOPS * 256)
    A, B, r = F.windows(d, y)
    A, r = A[:, 1:], r[:, 1:]      # column t = hop t
    print("%d Hz: r per hop, row 0: %s; smallest A from hop 1 on %.3g" % (rate, np.array2string(r[0], precision=3), A[:, 1:].min()))
    assert np.all(A[:, 1:] >= 2.0 ** -40)
    assert np.all((r > 1.0).sum(axis=1) >= 1) and np.all((r < 0.5).sum(axis=1) >= 3)
    assert np.all(r[:, 1:4] > 1.0) and np.all(np.abs(r[:, -1] - 0.05) < 0.01)      # across 1 and down to about 0.05
    assert np.all(np.abs(r[:, 1:] - 1.0) > 1e-3)                       # no hop sits on the clamp's edge
