"""``-m gpu``: waveform block mode of the offline handles -- block STFT / inverse STFT + overlap-add on the device
(``csrc/stft_block.hip``) around ``nutls_process_block`` -- against the numpy restatement of the reference's host
loop (``nunet_amd.stream_enhance`` <- ``dnn_model/interpreter_proposed.py:15-370``), the committed golden clip and
the streaming path.  The bounds are those ``tests/test_gpu_frontend.py`` / ``tests/test_gpu_offline.py`` apply to the
same comparisons of the per-hop kernels and of the block model."""
import ctypes
import os

import numpy as np
import pytest
import torch      # (before the first handle: torch must bring up the HIP runtime it ships with itself)

from nunet_amd import NutlsEngine, NutlsOffline, host_alloc, stream_enhance as SE

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

HOP = SE.FRAME_STEP
RAGGED = [1, 9, 15, 16, 17, 23, 8, 31, 33, 40, 2, 14]


@pytest.fixture(scope="module")
def clip():
    return np.load(os.path.join(GOLDEN, "clip_4s.npz"))


def audio_of(clip):
    return (clip["noisy_i16"].astype(np.float64) / 32768.0).astype(np.float32)


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def analyse(off, pcm, sizes):
    """``pcm [U, hops*256]`` through ``stft_block_device`` in blocks of ``sizes`` hops -> (mags [U,n,256], phasors [U,n,257,2])."""
    mags, phs, t = [], [], 0
    for n in sizes:
        x = torch.from_numpy(np.ascontiguousarray(pcm[:, t * HOP:(t + n) * HOP])).cuda()
        mags.append(off.stft_block_device(x).cpu().numpy())
        phs.append(off.debug_get("phasor_block", (n, 257, 2)))
        t += n
    return np.concatenate(mags, axis=1), np.concatenate(phs, axis=1)


def synthesise(off, pcm, est, sizes, dc_mode="edge"):
    """Analysis of ``pcm`` and synthesis of ``est [U,n,256]`` with its phase, block by block -> PCM ``[U, n*256]``."""
    out, t = [], 0
    for n in sizes:
        x = torch.from_numpy(np.ascontiguousarray(pcm[:, t * HOP:(t + n) * HOP])).cuda()
        off.stft_block_device(x)
        m = torch.from_numpy(np.ascontiguousarray(est[:, t:t + n])).cuda()
        out.append(off.istft_block_device(m, dc_mode=dc_mode).cpu().numpy())
        t += n
    return np.concatenate(out, axis=1)


def blocks_of(total, size):
    return [min(size, total - a) for a in range(0, total, size)]


def test_block_analysis_matches_host_loop_and_golden_magnitudes(clip):
    audio = audio_of(clip)
    mags, phases = SE.frame_magnitudes(audio)
    n = mags.shape[0]
    assert n == 249
    off = NutlsOffline(max_frames=256)
    got, ph = analyse(off, audio[None, :n * HOP], [n])
    off.close()
    scale = float(np.abs(mags).max())
    err_host = np.abs(got[0] - mags[:, 1:]).max()
    err_gold = np.abs(got[0] - clip["mags_in"]).max()
    ref = np.exp(1j * phases)
    strong = mags > 1e-3 * scale          # the phase of a numerically empty bin is noise on both sides
    err_ph = np.abs((ph[0, :, :, 0] + 1j * ph[0, :, :, 1]) - ref)[strong].max()
    print("block analysis: |mag - host| %.3e, |mag - golden| %.3e (bound %.3e), phasor %.3e (bound 2e-4)" % (err_host, err_gold, 2e-6 * scale, err_ph))
    assert err_host < 2e-6 * scale
    assert err_gold < 2e-6 * scale
    assert err_ph < 2e-4
    np.testing.assert_array_equal(ph[0, :, 0, 1], 0.0)          # angle(real) is 0 or pi
    assert np.all(np.abs(ph[0, :, 0, 0]) == 1.0)


def test_block_split_does_not_change_a_bit(clip):
    audio = audio_of(clip)[None]
    n = 249
    off = NutlsOffline(max_frames=256)
    whole_m, whole_p = analyse(off, audio, [n])
    off.reset()
    m64, p64 = analyse(off, audio, blocks_of(n, 64))
    off.reset()
    mr, pr = analyse(off, audio, RAGGED)
    t = sum(RAGGED)
    assert t == 209
    np.testing.assert_array_equal(m64, whole_m)
    np.testing.assert_array_equal(p64, whole_p)
    np.testing.assert_array_equal(mr, whole_m[:, :t])
    np.testing.assert_array_equal(pr, whole_p[:, :t])
    est = clip["mags_out"][None]
    off.reset()
    whole = synthesise(off, audio, est, [n])
    off.reset()
    s64 = synthesise(off, audio, est, blocks_of(n, 64))
    off.reset()
    sr = synthesise(off, audio, est, RAGGED)
    off.close()
    assert np.abs(whole).max() > 0.01
    np.testing.assert_array_equal(s64, whole)
    np.testing.assert_array_equal(sr, whole[:, :t * HOP])


def test_identity_model_reconstructs_the_input_one_hop_late():
    """window * inverse window overlap-adds to one: stft_block -> istft_block on the same magnitudes returns the input delayed
    by one hop (the signal of test_gpu_frontend.py's identity test: bin-centred sinusoids far from DC, dc_mode zero)."""
    rng = np.random.default_rng(7)
    B, n_hops = 5, 12
    n = np.arange(HOP * n_hops)
    x = np.zeros((B, n.size))
    for b in range(B):
        for k in rng.choice(np.arange(16, 201), size=24, replace=False):
            x[b] += rng.uniform(0.2, 1.0) * np.cos(2 * np.pi * k * n / SE.FRAME_LEN + rng.uniform(0, 2 * np.pi))
    x = x.astype(np.float32)
    off = NutlsOffline(max_frames=n_hops, utterances=B)
    mag = off.stft_block_device(torch.from_numpy(x).cuda())
    got = off.istft_block_device(mag, dc_mode="zero").cpu().numpy()
    off.close()
    ref = x[:, HOP:-HOP]
    err = got[:, 2 * HOP:] - ref
    rel = np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(ref ** 2))
    print("identity model: relative rms error %.3e (bound 2e-5)" % rel)
    assert rel < 2e-5


@pytest.mark.parametrize("max_frames", [256, 64, 7])
def test_whole_pipeline_matches_the_goldens(clip, max_frames):
    audio = audio_of(clip)
    off = NutlsOffline(max_frames=max_frames)
    dev = off.enhance(audio)
    off.close()
    assert dev.shape == audio.shape
    gold = clip["enhanced"].astype(np.float64)
    n = min(len(dev), len(gold))
    scale = np.sqrt(np.mean(gold[:n] ** 2))
    diff = np.sqrt(np.mean((dev[:n] - gold[:n]) ** 2))
    clean = clip["clean_i16"].astype(np.float64) / 32768.0
    n = 248 * 256                      # the samples the 249 frames fully cover (make_golden.py)
    snr, sisnr = SE.snr_db(clean[:n], dev[:n]), SE.si_snr_db(clean[:n], dev[:n])
    print("pipeline max_frames=%d: rms vs golden %.3e x rms (bound 1e-4), snr %.4f (golden %.4f), si-snr %.4f (golden %.4f)" % (
        max_frames, diff / scale, snr, float(clip["snr_after"]), sisnr, float(clip["sisnr_after"])))
    assert diff < 1e-4 * scale
    assert abs(snr - float(clip["snr_after"])) < 0.05
    assert abs(sisnr - float(clip["sisnr_after"])) < 0.05


def test_block_mode_equals_the_streaming_path(clip):
    audio = audio_of(clip)
    eng = NutlsEngine(batch=1)
    stream = SE.enhance_batch_on_device(audio[None], eng)[0]
    eng.close()
    off = NutlsOffline(max_frames=256)
    block = off.enhance(audio)
    off.close()
    rel = rel_rms(block, stream)
    print("block vs streaming: relative rms %.3e (bound 1e-5)" % rel)
    assert rel < 1e-5


def test_batch_independence_and_reset(clip):
    audio = audio_of(clip)[:HOP * 20]
    batch = np.stack([audio, 0.5 * audio, audio[::-1].copy()])
    off = NutlsOffline(max_frames=8, utterances=3)
    ref = off.enhance(batch)
    off.reset()
    again = off.enhance(batch)
    np.testing.assert_array_equal(ref, again)                 # reset restores the all-zero start exactly
    solo = NutlsOffline(max_frames=8)
    one = solo.enhance(batch[2])
    solo.close()
    assert rel_rms(ref[2], one) < 1e-5
    # a new recording starts in slot 1 in the middle of the run: only utterance 1's later output changes
    off.reset()
    half = HOP * 8
    first = off.enhance_block_host(np.ascontiguousarray(batch[:, :half]))
    off.reset_utterance(1)
    second = off.enhance_block_host(np.ascontiguousarray(batch[:, half:2 * half]))
    off.close()
    full = np.concatenate([first, second], axis=1)[:, HOP:]          # (enhance() drops the first output hop)
    np.testing.assert_array_equal(full[0], ref[0, :full.shape[1]])
    np.testing.assert_array_equal(full[2], ref[2, :full.shape[1]])
    np.testing.assert_array_equal(full[1, :half - HOP], ref[1, :half - HOP])
    assert np.abs(full[1, half - HOP:] - ref[1, half - HOP:full.shape[1]]).max() > 0


def test_chunked_pipeline_with_two_utterances(clip):
    """800 hops of two utterances in ONE call (three chunk streams fork from and join the caller's stream between analysis and
    synthesis) equal the same audio in blocks of 100 (one chunk)."""
    audio = audio_of(clip)
    hops = 800
    long = np.tile(audio, 4)[:(hops + 1) * HOP]
    late = np.concatenate([np.zeros(3 * HOP, np.float32), long[:-3 * HOP]])
    batch = np.stack([long, late])
    big = NutlsOffline(max_frames=hops, utterances=2)
    got = big.enhance(batch)
    big.close()
    small = NutlsOffline(max_frames=100, utterances=2)
    want = small.enhance(batch)
    small.close()
    assert got.shape == batch.shape
    for u in range(2):
        rel = rel_rms(got[u], want[u])
        print("chunked pipeline, utterance %d: relative rms %.3e (bound 1e-5)" % (u, rel))
        assert rel < 1e-5
    assert rel_rms(got[1], got[0]) > 1e-2          # (the two utterances differ)


def test_host_buffers_pageable_and_page_locked(clip):
    audio = audio_of(clip)
    n = 32
    x = np.ascontiguousarray(np.stack([audio[:n * HOP], audio[HOP:(n + 1) * HOP]]))
    off = NutlsOffline(max_frames=n, utterances=2)
    pageable = off.enhance_block_host(x)
    off.reset()
    pin_in, pin_out = host_alloc(x.shape), host_alloc(x.shape)
    pin_in[...] = x
    locked = off.enhance_block_host(pin_in, pin_out)
    off.close()
    assert locked is pin_out
    assert np.abs(pageable).max() > 1e-4          # (32 hops of the clip's quiet lead-in: small, not zero)
    np.testing.assert_array_equal(pageable, np.array(locked))


def test_bad_arguments_leave_the_handle_usable(clip):
    audio = audio_of(clip)
    off = NutlsOffline(max_frames=8)
    lib, h = off._lib, off._h
    buf = np.zeros(9 * HOP, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for n_hops, dc in ((0, 0), (9, 0), (8, 5)):
        assert lib.nutls_enhance_block_host(h, fp, fp, n_hops, dc) == -1, (n_hops, dc)
        assert lib.nutls_last_error()
    dev = torch.zeros(9 * HOP, device="cuda")
    assert lib.nutls_enhance_block(h, dev.data_ptr(), dev.data_ptr(), 0, 0, None) == -1
    assert lib.nutls_enhance_block(h, dev.data_ptr(), dev.data_ptr(), 9, 0, None) == -1
    assert lib.nutls_enhance_block(h, dev.data_ptr(), dev.data_ptr(), 8, 5, None) == -1
    assert lib.nutls_stft_block(h, dev.data_ptr(), dev.data_ptr(), 9, None) == -1
    assert lib.nutls_istft_block(h, dev.data_ptr(), dev.data_ptr(), 8, 5, None) == -1
    with pytest.raises(ValueError):
        off.enhance_block_device(torch.zeros(9 * HOP, device="cuda"))
    with pytest.raises(ValueError):
        off.enhance_block_device(torch.zeros(100, device="cuda"))
    with pytest.raises(ValueError):
        off.enhance_block_device(torch.zeros(8 * HOP, device="cuda"), dc_mode="mirror")
    with pytest.raises(ValueError):
        off.enhance(audio, "mirror")
    eng = NutlsEngine(batch=1)
    assert lib.nutls_enhance_block(eng._h, dev.data_ptr(), dev.data_ptr(), 1, 0, None) == -1
    assert b"nutls_enhance_hop" in lib.nutls_last_error()
    assert lib.nutls_enhance_block_host(eng._h, fp, fp, 1, 0) == -1
    assert lib.nutls_stft_block(eng._h, dev.data_ptr(), dev.data_ptr(), 1, None) == -1
    eng.close()
    # the handle still works, from its untouched zero start
    got = off.enhance(audio[:HOP * 17])
    off.close()
    fresh = NutlsOffline(max_frames=8)
    want = fresh.enhance(audio[:HOP * 17])
    fresh.close()
    assert np.abs(want).max() > 1e-4
    np.testing.assert_array_equal(got, want)


def test_quality_harness_with_the_block_engine(clip, tmp_path):
    from scipy.io import wavfile
    from nunet_amd.evaluate import evaluate_directory
    wavfile.write(str(tmp_path / "40hc020i_0.wav"), 16000, clip["noisy_i16"])
    wavfile.write(str(tmp_path / "40hc020i.wav"), 16000, clip["clean_i16"])
    wavfile.write(str(tmp_path / "short_0.wav"), 16000, clip["noisy_i16"][:20000])
    wavfile.write(str(tmp_path / "short.wav"), 16000, clip["clean_i16"][:20000])
    rows = {r["name"]: r for r in evaluate_directory(str(tmp_path), out_dir=str(tmp_path / "out"), engine="block")}
    full = rows["40hc020i"]
    assert abs(full["snr_before"] - float(clip["snr_before"])) < 0.05 and abs(full["snr_after"] - float(clip["snr_after"])) < 0.05
    assert abs(full["sisnr_after"] - float(clip["sisnr_after"])) < 0.05
    assert rows["short"]["snr_after"] > rows["short"]["snr_before"] + 5.0
    assert (tmp_path / "out" / "short_enhanced.wav").exists()
