"""``-m gpu``: ragged waveform blocks (``nutls_enhance_block_ragged`` and the two halves, include/nutls.h "Ragged blocks") and the corpus
scheduler on top of them (``NutlsOffline.enhance_many``), on the golden clip's waveform with ``NutlsOffline(max_frames=8, utterances=3)``.
The halves are compared bit for bit with the uniform halves (precedent: tests/test_gpu_enhance_block.py::test_block_split_does_not_change_a_bit);
the whole pipeline against one-utterance handles at the bound of ``test_batch_independence_and_reset`` there (relative RMS < 1e-5)."""
import ctypes
import os

import numpy as np
import pytest
import torch      # (before the first handle: torch must bring up the HIP runtime it ships with itself)

from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd.runner import NUTLS_ERR_ARG, _fptr

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

HOP, U, W = 256, 3, 8


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


@pytest.fixture(scope="module")
def audio():
    clip = np.load(os.path.join(GOLDEN, "clip_4s.npz"))
    return (clip["noisy_i16"].astype(np.float64) / 32768.0).astype(np.float32)


@pytest.fixture(scope="module")
def off():
    h = NutlsOffline(max_frames=W, utterances=U)
    yield h
    h.close()


@pytest.fixture(scope="module")
def solo():
    h = NutlsOffline(max_frames=W)
    yield h
    h.close()


def enhance_alone(solo, wave):
    solo.reset()
    return solo.enhance(wave)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_ragged_halves_are_the_uniform_halves_bit_for_bit(off, audio):
    c1, c2 = [8, 3, 0], [2, 8, 5]
    pcm = np.stack([audio[s:s + 11 * HOP] for s in (0, 20 * HOP + 37, 55 * HOP)])          # [U, 11 hops]
    rng = np.random.default_rng(5)
    est = rng.uniform(0.0, 0.05, size=(U, 11, 256)).astype(np.float32)                     # the 'model output' of every (utterance, hop)
    # uniform halves: widths 8 and 3, every utterance alike
    off.reset()
    want_m, want_p, want_x = [], [], []
    for a, n in ((0, 8), (8, 3)):
        want_m.append(off.stft_block_device(cuda(pcm[:, a * HOP:(a + n) * HOP])).cpu().numpy())
        want_p.append(off.debug_get("phasor_block", (n, 257, 2)))
        want_x.append(off.istft_block_device(cuda(est[:, a:a + n])).cpu().numpy())
    want_m, want_p, want_x = np.concatenate(want_m, axis=1), np.concatenate(want_p, axis=1), np.concatenate(want_x, axis=1)
    assert np.abs(want_x).max() > 1e-3
    # ragged halves: NaN in every input row behind a count
    off.reset()
    got_x = [[] for _ in range(U)]
    first = [0] * U
    for counts in (c1, c2):
        x = np.full((U, W * HOP), np.nan, np.float32)
        e = np.full((U, W, 256), np.nan, np.float32)
        for u, k in enumerate(counts):
            x[u, :k * HOP] = pcm[u, first[u] * HOP:(first[u] + k) * HOP]
            e[u, :k] = est[u, first[u]:first[u] + k]
        mag = off.stft_block_device(cuda(x), hops=counts).cpu().numpy()
        ph = off.debug_get("phasor_block", (W, 257, 2))
        out = off.istft_block_device(cuda(e), hops=np.array(counts)).cpu().numpy()
        for u, k in enumerate(counts):
            np.testing.assert_array_equal(mag[u, :k], want_m[u, first[u]:first[u] + k])
            np.testing.assert_array_equal(ph[u, :k], want_p[u, first[u]:first[u] + k])
            np.testing.assert_array_equal(mag[u, k:], 0.0)
            np.testing.assert_array_equal(out[u, k * HOP:], 0.0)
            got_x[u].append(out[u, :k * HOP])
            first[u] += k
    assert first == [10, 11, 5]
    for u in range(U):
        np.testing.assert_array_equal(np.concatenate(got_x[u]), want_x[u, :first[u] * HOP])


def test_enhance_ragged_equals_each_recording_alone(off, solo, audio):
    waves = [audio[:20 * HOP + 100], audio[3000:3300], audio[40 * HOP:53 * HOP]]          # not a multiple of 256; shorter than two hops; 13 hops
    off.reset()
    got = off.enhance_ragged(waves)
    assert [g.shape for g in got] == [w.shape for w in waves]
    for u, w in enumerate(waves):
        want = enhance_alone(solo, w)
        if len(w) < 3 * HOP:          # fewer than two hops: the only output hop, if any, is the dropped leading one -- all zeros
            assert not want.any() and not got[u].any()
            continue
        e = rel_rms(got[u], want)
        print("recording %d (%d samples): relative rms %.3e (bound 1e-5)" % (u, len(w), e))
        assert e < 1e-5, u
    with pytest.raises(ValueError):
        off.enhance_ragged(waves[:2])


def test_enhance_many_schedules_a_corpus_through_the_slots(off, solo, audio):
    cuts = [(0, 9 * HOP), (5 * HOP, 30 * HOP + 77), (100, 400), (60 * HOP, 62 * HOP), (17, 17 + 12 * HOP + 1), (90 * HOP, 107 * HOP), (33 * HOP, 38 * HOP + 200)]
    waves = [audio[a:b] for a, b in cuts]
    assert len(waves) == 7
    got = off.enhance_many(waves)
    assert [g.shape for g in got] == [w.shape for w in waves]          # input order
    for i, w in enumerate(waves):
        want = enhance_alone(solo, w)
        if len(w) < 3 * HOP:          # fewer than two hops: the only output hop, if any, is the dropped leading one -- all zeros
            assert not want.any() and not got[i].any()
            continue
        e = rel_rms(got[i], want)
        print("recording %d (%d samples): relative rms %.3e (bound 1e-5)" % (i, len(w), e))
        assert e < 1e-5, i
    again = off.enhance_many(waves)          # slots are reset between recordings: nothing of the first run is left
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)


def test_streaming_handles_and_bad_host_counts_are_refused(off, audio):
    eng = NutlsEngine(batch=2)
    lib = eng._lib
    d = torch.zeros(2, 256, device="cuda")
    dc = torch.ones(2, dtype=torch.int32, device="cuda")
    hbuf = np.zeros((2, 256), np.float32)
    hc = np.ones(2, np.int32)
    ip = hc.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    p, c = d.data_ptr(), dc.data_ptr()
    calls = {
        "nutls_process_block_ragged": lambda: lib.nutls_process_block_ragged(eng._h, p, p, 1, c, None),
        "nutls_process_block_ragged_host": lambda: lib.nutls_process_block_ragged_host(eng._h, _fptr(hbuf), _fptr(hbuf), 1, ip),
        "nutls_enhance_block_ragged": lambda: lib.nutls_enhance_block_ragged(eng._h, p, p, 1, c, 0, None),
        "nutls_enhance_block_ragged_host": lambda: lib.nutls_enhance_block_ragged_host(eng._h, _fptr(hbuf), _fptr(hbuf), 1, ip, 0),
        "nutls_stft_block_ragged": lambda: lib.nutls_stft_block_ragged(eng._h, p, p, 1, c, None),
        "nutls_istft_block_ragged": lambda: lib.nutls_istft_block_ragged(eng._h, p, p, 1, c, 0, None),
    }
    for name, call in calls.items():
        assert call() == NUTLS_ERR_ARG, name
        assert b"offline handle" in lib.nutls_last_error(), name
    eng.close()
    # host counts outside 0 .. n_hops: refused, and the handle goes on as if nothing had happened
    waves = [audio[:9 * HOP], audio[HOP:4 * HOP], audio[2 * HOP:7 * HOP]]
    off.reset()
    want = off.enhance_ragged(waves)
    off.reset()
    blk = np.zeros((U, W * HOP), np.float32)
    out = np.empty_like(blk)
    for bad in ([W + 1, 0, 0], [1, -1, 1]):
        cnt = np.array(bad, np.int32)
        rc = off._lib.nutls_enhance_block_ragged_host(off._h, _fptr(blk), _fptr(out), W, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 0)
        assert rc == NUTLS_ERR_ARG and b"outside" in off._lib.nutls_last_error()
        with pytest.raises(ValueError):
            off.enhance_block_device(cuda(blk), hops=bad)
    for a, b in zip(off.enhance_ragged(waves), want):
        np.testing.assert_array_equal(a, b)
