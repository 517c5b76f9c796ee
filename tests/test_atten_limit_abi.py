"""CPU checks of the attenuation limit (include/nutls.h, "Attenuation limit"): the three entries exist at every layer and refuse a null
handle by name, the dB helper and the CPU statement of the formula (``stream_enhance.mix_magnitudes``) have their exact ends, the reference's
host loop takes the limit, and the float64 reference of tests/test_gpu_atten_limit.py is sharp enough on the limits and inputs it uses."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import atten_limit_reference as A
import transform_signals as TS
from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner
from nunet_amd import stream_enhance as SE
from nunet_amd import topology as T
from nunet_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = TS.HOP


@pytest.fixture(scope="module")
def lib():
    build()
    return runner.load_library()


def test_the_entries_exist_at_every_layer(lib):
    hdr = open(os.path.join(ROOT, "include", "nutls.h")).read()
    assert re.search(r"\bint\s+nutls_set_atten_limit\s*\(\s*nutls_handle\s*\*\s*h\s*,\s*const\s+float\s*\*\s*limit\s*,\s*int\s+n\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+nutls_atten_limit\s*\(\s*nutls_handle\s*\*\s*h\s*,\s*float\s*\*\s*limit\s*,\s*int\s+n\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+nutls_istft_block_mix\s*\(\s*nutls_handle\s*\*\s*h\s*,\s*const\s+float\s*\*\s*est\s*,\s*const\s+float\s*\*\s*noisy\s*,"
                     r"\s*float\s*\*\s*pcm_out\s*,\s*int\s+n_hops\s*,\s*const\s+int\s*\*\s*hops\s*,\s*int\s+dc_mode\s*,\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    assert "Attenuation limit" in hdr
    fp, vp = ctypes.POINTER(ctypes.c_float), ctypes.c_void_p
    for name, argtypes in (("nutls_set_atten_limit", [vp, fp, ctypes.c_int]),
                           ("nutls_atten_limit", [vp, fp, ctypes.c_int]),
                           ("nutls_istft_block_mix", [vp, vp, vp, vp, ctypes.c_int, vp, ctypes.c_int, vp])):
        assert name in runner.ABI_SYMBOLS
        fn = getattr(lib, name)      # AttributeError: not exported
        assert list(fn.argtypes) == argtypes and fn.restype is ctypes.c_int
    for cls in (NutlsEngine, NutlsOffline):
        assert list(inspect.signature(cls.set_atten_limit).parameters) == ["self", "limit", "db"]
        assert isinstance(inspect.getattr_static(cls, "atten_limit"), property)
    assert inspect.signature(NutlsOffline.istft_block_device).parameters["noisy"].default is None
    for method in ("enhance", "enhance_ragged"):
        assert inspect.signature(getattr(NutlsOffline, method)).parameters["atten_lim_db"].default is None
    assert list(inspect.signature(NutlsOffline.enhance_many_atten).parameters) == ["self", "waves", "atten_lim_db", "dc_mode", "rate"]
    assert inspect.signature(SE.real_time_speech_enhancer).parameters["atten_limit"].default == 0.0


def test_a_null_handle_is_refused_by_name(lib):
    a = (ctypes.c_float * 3)(7.0, 7.0, 7.0)
    x = np.zeros(256, np.float32).ctypes.data
    for call, name in ((lambda: lib.nutls_set_atten_limit(None, a, 3), b"nutls_set_atten_limit"),
                       (lambda: lib.nutls_atten_limit(None, a, 3), b"nutls_atten_limit"),
                       (lambda: lib.nutls_istft_block_mix(None, x, x, x, 1, None, 0, None), b"nutls_istft_block_mix")):
        assert lib.nutls_batch(None) == runner.NUTLS_ERR_ARG and name not in lib.nutls_last_error()      # (another text in the one error slot)
        assert call() == runner.NUTLS_ERR_ARG
        assert name in lib.nutls_last_error()
    assert list(a) == [7.0, 7.0, 7.0]


def test_the_db_helper():
    f = runner.atten_limit_from_db
    assert f(0) == 1.0 and f(None) == 0.0 and f(20) == np.float32(0.1)
    assert all(isinstance(f(d), np.float32) for d in (0, None, 20, 6.5))
    assert 0.0 < f(6) < 1.0 and f(12) < f(6)
    for bad in (-1, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            f(bad)


def test_mix_magnitudes_is_exact_at_both_ends():
    rng = np.random.default_rng(5)
    x = np.float32([0.0, 1e-45, 1e-40, 1.17549435e-38, 1e-30, 1.0, 3.0, 1e30] * 4)
    e = rng.permutation(x)
    assert (x == 0).any() and ((x > 0) & (x < 1.1754944e-38)).any() and (x == np.float32(1e30)).any()
    got0, got1 = SE.mix_magnitudes(x, e, 0.0), SE.mix_magnitudes(x, e, 1.0)
    assert got0.dtype == np.float32 and got0.tobytes() == e.tobytes() and got1.tobytes() == x.tobytes()
    rows = SE.mix_magnitudes(np.stack([x, x]), np.stack([e, e]), np.float32([[1.0], [0.0]]))          # one limit per row
    assert rows[0].tobytes() == x.tobytes() and rows[1].tobytes() == e.tobytes()
    # in between: the float32 l, c = float32(1 - l) formed in double, one rounding of the double sum
    l = np.float32(0.1)
    want = (np.float64(l) * x.astype(np.float64) + np.float64(np.float32(1.0 - np.float64(l))) * e.astype(np.float64)).astype(np.float32)
    assert SE.mix_magnitudes(x, e, 0.1).tobytes() == want.tobytes()
    assert A.companion(np.float32(1.0 - 2.0 ** -24)) == np.float32(2.0 ** -24)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            SE.mix_magnitudes(x, e, bad)


class _Stub:
    """A runner for ``real_time_speech_enhancer`` whose 'model' halves its input and adds the rows of ``est`` in turn (states: zeros, echoed)."""

    def __init__(self, est):
        self.est, self.i, self.out = est, 0, SE.zero_state()

    def __call__(self, **feeds):
        x = feeds["input"]
        assert x.shape == (1, 1, T.N_BINS, 1)
        self.out["model_out"] = (0.5 * x.reshape(-1) + self.est[self.i]).astype(np.float32).reshape(1, 1, T.N_BINS, 1)
        self.i += 1
        return self.out


@pytest.mark.parametrize("dc", ["edge", "zero"])
def test_the_host_loop_mixes_linearly(dc):
    """``real_time_speech_enhancer(atten_limit=l)`` = (1 - l) x the loop at 0 + l x the loop at 1 to 1e-6 relative RMS: mix and synthesis are
    linear, the float32 roundings of the mix and of the loop's blocks are what is left."""
    noise = TS.NAMES.index("noise")
    x, est = TS.signals()[noise], 0.05 * TS.estimates()[noise]
    run = lambda l: SE.real_time_speech_enhancer(x, _Stub(est), dc_mode=dc, atten_limit=l)[0]
    out0, out1 = run(0.0), run(1.0)
    assert np.array_equal(out0, SE.real_time_speech_enhancer(x, _Stub(est), dc_mode=dc)[0])          # 0 is the loop as it was
    for l in (np.float32(0.3), np.float32(0.1)):
        got, want = run(float(l)), (1.0 - np.float64(l)) * out0 + np.float64(l) * out1
        assert TS.rel_rms(got, want) <= 1e-6, (l, TS.rel_rms(got, want))
    assert TS.rel_rms(out1, out0) > 0.1          # (the two ends differ: the comparison above is not empty)


@pytest.mark.parametrize("dc", ["edge", "zero"])
def test_conditioning_of_the_gpu_tests_reference(dc):
    """The limits ``L``, one per row, on the float32 magnitudes of the analysis reference and ``estimates()``: a float32 CPU synthesis of the
    ``mix_magnitudes`` rows lies within CAP of SYNTH x the block normaliser of the float64-mixed rows, on EVERY output hop that has a
    normaliser -- so the float64 reference of tests/test_gpu_atten_limit.py measures the kernels, not itself.  The worst ratio is printed."""
    X = TS.analysis_reference()
    noisy = np.abs(X)[..., 1:].astype(np.float32)
    rot = TS.unit_phasors(X)
    est = TS.estimates()
    mixed32 = SE.mix_magnitudes(noisy, est, A.L[:, None, None])
    mixed64 = A.mix64(noisy, est, A.L)
    assert mixed32.dtype == np.float32 and mixed32[0].tobytes() == est[0].tobytes() and mixed32[1].tobytes() == noisy[1].tobytes()
    assert np.abs(mixed32 - mixed64).max() <= 2.0 ** -23 * np.abs(mixed64).max()
    got = TS.synthesis_float32(mixed32, rot, dc)
    want, norm = TS.synthesis_reference(mixed64, rot, dc)
    full = TS.block_normaliser(mixed64, rot, dc)
    S, n = full.shape
    err = np.sqrt(np.mean((got.astype(np.float64) - want).reshape(S, n, HOP) ** 2, axis=-1))
    live = full > 0
    ratio = err[live] / (TS.SYNTH * full[live])
    print("float32 CPU synthesis of the mixed rows, dc %s: worst error / (SYNTH x block normaliser) %.3g over %d output hops" % (dc, ratio.max(), ratio.size))
    own = err[norm > 0] / (TS.SYNTH * norm[norm > 0])
    print("the same over the hop's own normaliser: worst %.3g (a frame with a silent half synthesises to a hop that is a cancellation)" % own.max())
    assert ratio.size == live.sum() and np.all(live[norm > 0])                                    # every hop with a normaliser is tested ...
    assert np.all(ratio <= TS.CAP), ratio.max()
    assert not got.reshape(S, n, HOP)[~live].any()                                                # ... and the others are exactly zero
    assert live.sum() > S * n // 2 and all(live[s].any() for s in range(S))
