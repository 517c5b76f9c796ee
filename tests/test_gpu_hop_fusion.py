"""``-m gpu``: hop fusion (include/nutls.h nutls_set_hop_fusion; csrc/fused_step.hip hop_prologue / hop_epilogue) -- the streaming hop as
ONE launch of a hop build of the fused step kernel instead of analysis, step and synthesis in a launch each.

References, all of them code that existed before the feature:
  * to the last place or two: the waveform block mode's transform (``nutls_stft_block`` / ``nutls_istft_block`` of an offline handle, csrc/stft_block.hip,
    whose wave-level code the hop builds share through csrc/stft_wave.hpp) around ``nutls_step`` of a plain fused handle;
  * to rounding: the three-launch path (csrc/stft.hip, a radix-2 transform) and, behind it, the numpy restatement of the reference's host
    loop (``nunet_amd.stream_enhance`` <- dnn_model/interpreter_proposed.py:15-370) and the golden clip.  Tolerances are those of
    tests/test_gpu_frontend.py: 2e-6 x scale on magnitudes, 2e-4 on the phasors of strong bins, 1e-4 relative RMS against the golden
    waveform, 1e-5 relative RMS between two device paths.
Inputs: the first 12 hops of the golden clip (stream 0) and seeded white noise at speech level (the other streams)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from nunet_amd import NutlsEngine, NutlsOffline, host_alloc, stream_enhance as SE
from nunet_amd import weights as W

pytestmark = pytest.mark.gpu

HOP = SE.FRAME_STEP
N_HOPS = 12
PLANS = [(3, 1), (4, 2)]      # (streams, streams per workgroup): the one-stream plan with an odd batch, the two-stream plan with two pairs


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


@pytest.fixture(scope="module")
def clip():
    return np.load(os.path.join(GOLDEN, "clip_4s.npz"))


@pytest.fixture(scope="module")
def audio(clip):
    """[4, 12 * 256]: stream 0 = the clip's first 12 hops, streams 1..3 = white noise at speech level."""
    x = np.empty((4, N_HOPS * HOP), np.float32)
    x[0] = (clip["noisy_i16"][:N_HOPS * HOP].astype(np.float64) / 32768.0).astype(np.float32)
    x[1:] = (0.05 * np.random.default_rng(20240612).standard_normal((3, N_HOPS * HOP))).astype(np.float32)
    return x


def hop_of(audio, B, i):
    return np.ascontiguousarray(audio[:B, i * HOP:(i + 1) * HOP])


def run_hops(eng, audio, B, hops, dc="edge"):
    """enhance_hop on pageable numpy hops -> [B, len(hops) * 256]"""
    return np.concatenate([eng.enhance_hop(hop_of(audio, B, i), dc) for i in hops], axis=1)


@pytest.fixture(scope="module")
def three_launch(audio):
    """The parent's path, computed once per plan: 12 three-launch hops (dc edge) of a handle that never heard of fusion."""
    out = {}
    for B, G in PLANS:
        eng = NutlsEngine(batch=B, streams_per_workgroup=G)
        assert eng.launches_per_hop == 3
        out[(B, G)] = run_hops(eng, audio, B, range(N_HOPS))
        eng.close()
    return out


@pytest.fixture(scope="module")
def block_reference(audio):
    """Per plan: block analysis of all 12 hops -> nutls_step frame by frame on a plain fused handle -> block synthesis in both DC modes.
    -> {(B, G): (mags [B,12,256], {dc: pcm [B, 12 * 256]}, states [B][...])}"""
    import torch
    ref = {}
    for B, G in PLANS:
        off = NutlsOffline(max_frames=N_HOPS, utterances=B)
        mags = off.stft_block_device(torch.from_numpy(audio[:B].copy()).cuda())
        eng = NutlsEngine(batch=B, streams_per_workgroup=G)
        est = torch.empty_like(mags)
        for i in range(N_HOPS):
            est[:, i] = eng.step(mags[:, i].contiguous())
        states = [eng.state_get_all(b) for b in range(B)]
        eng.close()
        pcm = {}
        for dc in ("edge", "zero"):      # (the phasors of the analysis stay inside the handle; the overlap tail starts from zero again)
            off.reset()
            off.stft_block_device(torch.from_numpy(audio[:B].copy()).cuda())
            pcm[dc] = off.istft_block_device(est, dc_mode=dc).cpu().numpy()
        off.close()
        ref[(B, G)] = (mags.cpu().numpy(), pcm, states)
    return ref


@pytest.mark.parametrize("B,G", PLANS)
def test_fused_hop_equals_block_transform_around_the_step(audio, block_reference, B, G):
    """pcm_out of all 12 hops in both DC modes, the library's mag_in row after every hop and all 130 states at the end, against block
    analysis -> nutls_step -> block synthesis.

    The two kernels inline the same source (csrc/stft_wave.hpp), but they are not bit-identical: hop 0 (previous hop all zero) agrees in
    every bit, from hop 1 on single magnitudes differ in the last place (measured on an MI355X over the 12 hops: magnitudes 2.98e-7 at a scale of 1.8-2.0, pcm
    1.45e-7 absolute and 2.2e-6 relative RMS, states 6.6e-7 relative RMS) --
    the compiler contracts the window multiplies into the first butterfly's adds differently in the two surroundings.  The block kernels'
    arithmetic is not rewritten to force equality; the comparison falls back to the tolerances tests/test_gpu_frontend.py uses between
    device paths: 2e-6 x scale on magnitudes, 1e-5 relative RMS on waveforms -- and the same 1e-5 relative RMS on a stream's concatenated
    states, which are activations of the same network fed those magnitudes.  The largest differences are printed."""
    import torch
    mags, pcm, states = block_reference[(B, G)]
    scale = float(np.abs(mags).max())
    for dc in ("edge", "zero"):
        eng = NutlsEngine(batch=B, streams_per_workgroup=G, hop_fusion=True)
        assert eng.launches_per_hop == 1 and eng.streams_per_workgroup == G
        outs, worst_mag = [], 0.0
        for i in range(N_HOPS):
            outs.append(eng.enhance_hop(torch.from_numpy(hop_of(audio, B, i)).cuda(), dc).cpu().numpy())
            worst_mag = max(worst_mag, float(np.abs(eng.debug_get("mag_in", (256,)) - mags[:, i]).max()))
        got = np.concatenate(outs, axis=1)
        err_pcm = max(rel_rms(got[b], pcm[dc][b]) for b in range(B))
        err_state = max(rel_rms(eng.state_get_all(b), states[b]) for b in range(B))
        eng.close()
        print("plan %d dc %s: max |mag diff| %.3g (scale %.3g), max |pcm diff| %.3g, pcm relative RMS %.3g, states relative RMS %.3g" % (
            G, dc, worst_mag, scale, float(np.abs(got - pcm[dc]).max()), err_pcm, err_state))
        assert worst_mag < 2e-6 * scale, dc
        assert err_pcm < 1e-5, dc
        assert err_state < 1e-5, dc


def test_fused_hop_matches_host_loop_and_goldens(clip, audio):
    """The assertions of test_gpu_frontend.py's analysis and waveform tests, on a fused handle over the clip's first 12 hops."""
    import torch
    full = (clip["noisy_i16"].astype(np.float64) / 32768.0).astype(np.float32)
    mags, phases = SE.frame_magnitudes(full)
    scale = float(np.abs(mags).max())
    eng = NutlsEngine(batch=1, hop_fusion=True)
    outs = []
    for i in range(N_HOPS):
        outs.append(eng.enhance_hop(torch.from_numpy(hop_of(audio, 1, i)).cuda()).cpu().numpy()[0])
        got = eng.debug_get("mag_in", (256,))[0]
        assert np.abs(got - mags[i, 1:]).max() < 2e-6 * scale, i
        assert np.abs(got - clip["mags_in"][i]).max() < 2e-6 * scale, i
        ph = eng.debug_get("phasor", (257, 2))[0]
        ref = np.exp(1j * phases[i])
        strong = mags[i] > 1e-3 * scale          # the phase of a numerically empty bin is noise on both sides
        assert np.abs((ph[:, 0] + 1j * ph[:, 1]) - ref)[strong].max() < 2e-4, i
    eng.close()
    dev = np.concatenate(outs)[HOP:]             # (the loop drops the leading half window: interpreter_proposed.py:368)
    gold = clip["enhanced"].astype(np.float64)[:len(dev)]
    err = np.sqrt(np.mean((dev - gold) ** 2)) / np.sqrt(np.mean(gold ** 2))
    print("fused hops vs golden waveform prefix: relative RMS %.3g" % err)
    assert err < 1e-4


@pytest.mark.parametrize("B,G", PLANS)
def test_masks_streams_on_their_own_clocks(audio, B, G):
    """Stream 1 takes its hops 0, 1, 2 at ticks 0, 3, 4, the others one per tick (on the two-stream plan pair (0, 1) is half held, pair
    (2, 3) never): every stream's active hops equal the lock-step fused handle's bit for bit, held rows are exactly zero though the held
    input row is NaN."""
    ticks = 5
    ref = NutlsEngine(batch=B, streams_per_workgroup=G, hop_fusion=True)
    want = [ref.enhance_hop(hop_of(audio, B, k)) for k in range(ticks)]
    ref.close()
    eng = NutlsEngine(batch=B, streams_per_workgroup=G, hop_fusion=True)
    cnt = [0] * B
    for t in range(ticks):
        mask = np.ones(B, np.uint8)
        mask[1] = t in (0, 3, 4)
        x = np.full((B, HOP), np.nan, np.float32)
        for b in range(B):
            if mask[b]:
                x[b] = audio[b, cnt[b] * HOP:(cnt[b] + 1) * HOP]
        out = eng.enhance_hop(x, active=mask)
        for b in range(B):
            if mask[b]:
                assert np.array_equal(out[b], want[cnt[b]][b]), (t, b)
                cnt[b] += 1
            else:
                assert out[b].tobytes() == bytes(4 * HOP), (t, b)
    assert cnt[1] == 3 and all(cnt[b] == ticks for b in range(B) if b != 1)
    assert eng.launches_per_hop == 1
    eng.close()


def test_switching_between_fused_and_three_launch_hops_and_reset(audio, three_launch):
    B, G = PLANS[0]
    want = three_launch[(B, G)]
    for first in (True, False):
        eng = NutlsEngine(batch=B, streams_per_workgroup=G, hop_fusion=first)
        a = run_hops(eng, audio, B, range(6))
        eng.set_hop_fusion(not first)
        assert eng.launches_per_hop == (3 if first else 1)
        b = run_hops(eng, audio, B, range(6, N_HOPS))
        eng.close()
        err = rel_rms(np.concatenate([a, b], axis=1), want)
        print("fusion %s for hops 0..5, %s for 6..11, against 12 three-launch hops: relative RMS %.3g" % (first, not first, err))
        assert err < 1e-5
    eng = NutlsEngine(batch=B, streams_per_workgroup=G, hop_fusion=True)
    once = run_hops(eng, audio, B, range(N_HOPS))
    eng.reset()
    again = run_hops(eng, audio, B, range(N_HOPS))
    eng.close()
    assert np.array_equal(once, again)                      # reset restores the all-zero start exactly
    assert rel_rms(once, want) < 1e-5


def test_pinned_host_buffers_give_the_bits_of_pageable_ones(audio):
    B, G = PLANS[0]
    eng = NutlsEngine(batch=B, streams_per_workgroup=G, hop_fusion=True)
    pageable = run_hops(eng, audio, B, range(N_HOPS))
    eng.reset()
    pin_in, pin_out = host_alloc((B, HOP)), host_alloc((B, HOP))
    pinned = []
    for i in range(N_HOPS):
        pin_in[...] = hop_of(audio, B, i)
        assert eng.enhance_hop(pin_in, out=pin_out) is pin_out
        pinned.append(pin_out.copy())
    eng.close()
    assert np.array_equal(np.concatenate(pinned, axis=1), pageable)


def test_launch_counts_and_what_is_refused_while_fusion_is_on(audio, three_launch):
    B, G = PLANS[0]
    eng = NutlsEngine(batch=B, streams_per_workgroup=G)
    assert eng.launches_per_hop == 3
    eng.set_hop_fusion(True)
    assert eng.launches_per_hop == 1
    for call in (lambda: eng.debug_trace(True), lambda: eng.set_mode("launches"), lambda: eng.set_mode("graph"), eng.profile_fused,
                 eng.profile_step, eng.profile_production):
        with pytest.raises(ValueError, match="hop fusion"):
            call()
        assert eng.launches_per_hop == 1
    eng.set_hop_fusion(False)
    assert eng.launches_per_hop == 3
    assert np.array_equal(run_hops(eng, audio, B, range(N_HOPS)), three_launch[(B, G)])      # (nothing of the refused calls stuck)
    eng.close()


def _refused(make, prepare=None):
    """A handle on which nutls_set_hop_fusion(h, 1) must fail, and an identical one that is never asked: -> (the asked handle, the other)"""
    asked, twin = make(), make()
    for e in (asked, twin):
        if prepare:
            prepare(e)
    rc = asked._lib.nutls_set_hop_fusion(asked._h, 1)
    assert rc == -1                                                       # NUTLS_ERR_ARG
    assert len(asked._lib.nutls_last_error()) > 0
    assert asked._lib.nutls_launches_per_hop(asked._h) == 3
    return asked, twin


@pytest.mark.parametrize("case", ["baseline", "four_stream_plan", "mode_launches", "mode_graph", "debug_trace"])
def test_refusals_on_streaming_handles_leave_the_three_launch_bits(audio, case):
    B = 4
    if case == "baseline":
        blob = W.write_blob(W.synthetic_weights("baseline"), int8_convs=True)
        asked, twin = _refused(lambda: NutlsEngine(blob, batch=B, variant="baseline"))
    elif case == "four_stream_plan":
        asked, twin = _refused(lambda: NutlsEngine(batch=B, streams_per_workgroup=4))
    elif case == "mode_launches":
        asked, twin = _refused(lambda: NutlsEngine(batch=B, mode="launches"))
    elif case == "mode_graph":
        asked, twin = _refused(lambda: NutlsEngine(batch=B, mode="graph"))
    else:
        asked, twin = _refused(lambda: NutlsEngine(batch=B, streams_per_workgroup=1), lambda e: e.debug_trace(True))
    got, want = run_hops(asked, audio, B, range(3)), run_hops(twin, audio, B, range(3))
    asked.close()
    twin.close()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(got, want)


def test_refusal_on_an_offline_handle(audio):
    import torch
    asked, twin = _refused(lambda: NutlsOffline(max_frames=4, utterances=2))
    x = torch.from_numpy(audio[:2, :4 * HOP].copy()).cuda()
    got, want = asked.enhance_block_device(x).cpu().numpy(), twin.enhance_block_device(x).cpu().numpy()
    asked.close()
    twin.close()
    assert np.array_equal(got, want)


def test_environment_switch_reaches_handles_built_through_the_engine_class(monkeypatch):
    monkeypatch.setenv("NUTLS_HOP_FUSION", "1")
    on = NutlsEngine(batch=2)
    quiet = NutlsEngine(batch=4, streams_per_workgroup=4)      # (no hop build for this plan: the switch is quietly off)
    assert on.launches_per_hop == 1 and quiet.launches_per_hop == 3
    on.set_hop_fusion(False)
    assert on.launches_per_hop == 3
    on.close()
    quiet.close()
