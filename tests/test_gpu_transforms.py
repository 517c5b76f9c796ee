"""``-m gpu``: the three implementations of the 512-point analysis and synthesis -- the per-hop kernels (csrc/stft.hip: radix-2 in LDS), the
block kernels, uniform and ragged (csrc/stft_block.hip on csrc/stft_wave.hpp: radix-4 in registers) and the hop builds of the fused step
(csrc/fused_step.hip, FZ_HOP: the same header, their own loads, stores and LDS placement) -- against ``np.fft`` in double on the designed
signals and estimates of tests/transform_signals.py, PER FRAME and PER OUTPUT HOP: MAG x the frame's own scale on magnitudes, PHASOR on the
bins that are strong in their own frame, SYNTH x the output hop's own normaliser, and the exact conditions (an empty frame gives 0 and (1, 0),
the DC phasor is (+-1, 0) with the sign of X_0, an output hop of two empty blocks is 0).  Synthesis is referenced on the device's own
phasors, read back, so that analysis error is not charged twice.

Measured on an MI355X (worst ratio to the bound over all signals, frames and bins; profiles/transform_parity.json):
                      magnitudes / MAG   phasors / PHASOR   synthesis / SYNTH   (edge - zero) / SYNTH
  per-hop kernels     0.118 (impulse)    0.028 (noise)      0.126 (impulse)     0.052 (nyquist)
  block kernels       0.118 (impulse)    0.024 (gaps)       0.125 (impulse)     0.071 (dc_neg)
  hop builds, G = 1   0.118 (impulse)    0.018 (gaps)       0.124 / 0.081 (edge / zero, on the model's outputs, block normaliser)
  hop builds, G = 2   0.118 (impulse)    0.018 (gaps)       0.131 / 0.090
  float32 CPU (scipy) 0.121 (impulse)    0.023 (sine)       0.132 (nyquist)     -- tests/test_transform_signals.py
All three implementations sit where pocketfft in single precision sits; the exact conditions hold everywhere.  Between device paths
(DEVICE_REL): block against per-hop kernels 0.012 on magnitudes, 0.053 on waveforms (sine); hop builds against three launches 0.90
(nyquist; the step's answer to two analyses that differ in the last place).

Mutation check (scratch builds of the library, not committed): the DC phasor's sign negated in ``analyse_frame`` and ``e0.y`` for ``e0.x`` in
the edge DC of ``synthesise_frame`` fail test_block_kernels_against_float64 (DC phasor of impulse frame 0; every live output hop, first
impulse hop 0 at 1.4e5 x SYNTH); ``tw[(j << (8 - s)) + 1]`` in stage 3 of ``fft512`` fails test_per_hop_kernels_against_float64 (dc_neg frame 0
at 1.4e3 x MAG).  Keeping the imaginary part of bin 256 in ``istft_hop_kernel`` cannot fail anything: that kernel runs a full complex
inverse FFT and keeps the real part, and i c (-1)^n is imaginary (and its own analysis leaves that imaginary part exactly zero).
"""
import ctypes

import numpy as np
import pytest
import torch      # (before the first handle: torch must bring up the HIP runtime it ships with itself)

import transform_signals as TS
from nunet_amd import NutlsEngine, NutlsOffline

pytestmark = pytest.mark.gpu

HOP, N = TS.HOP, TS.N_HOPS
DCS = ("edge", "zero")
ODD = (0, 1, 6)                              # the streams of the three-stream handle: impulse, dc_neg, gaps
CUT = (1, 3, 4, 5, 16, 17, 2)                # the 48 hops again, cut across the 4-frame runs and the 16-frame tiles
COUNTS = (48, 1, 17, 0, 16, 5, 33, 4)        # ragged: per-utterance hop counts
FUSED_HOPS = 16


def cuda(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()          # (a copy: the helper module's arrays are read-only)


def hop_of(x, i):
    return np.ascontiguousarray(x[:, i * HOP:(i + 1) * HOP])


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64.so not loadable through ctypes")


def per_hop_run(streams, est=None):
    """The per-hop kernels on ``streams`` of the designed signals: 48 x (stft_hop, read mag_in and phasor, estimates -> the model-output
    buffer, istft_hop), once per DC mode from a reset -> (mag [B,48,256], ph [B,48,257,2], {dc: pcm [B, 48 * 256]})."""
    x, est = TS.signals()[list(streams)], (TS.estimates() if est is None else est)[list(streams)]
    B = len(streams)
    eng = NutlsEngine(batch=B)
    assert eng.launches_per_hop == 3
    hip = _hip()
    est_dev = cuda(est.transpose(1, 0, 2))          # [48, B, 256]: row i is what the 'model' leaves for hop i
    y = torch.empty(B, HOP, device="cuda")
    pcm = {}
    for dc in DCS:
        eng.reset()
        mags, phs, outs = [], [], []
        for i in range(N):
            eng.stft_hop(cuda(hop_of(x, i)))
            mags.append(eng.debug_get("mag_in", (256,)))
            phs.append(eng.debug_get("phasor", (257, 2)))
            torch.cuda.synchronize()
            # hipMemcpyDeviceToDevice = 3
            assert hip.hipMemcpy(ctypes.c_void_p(eng.io_out_ptr), ctypes.c_void_p(est_dev[i].data_ptr()), ctypes.c_size_t(B * 256 * 4), 3) == 0
            eng.istft_hop(y, dc)
            outs.append(y.cpu().numpy().copy())
        pcm[dc] = np.concatenate(outs, axis=1)
        mag, ph = np.stack(mags, axis=1), np.stack(phs, axis=1)
        if dc != DCS[0]:
            assert np.array_equal(mag, first[0]) and np.array_equal(ph, first[1])          # reset restores the all-zero previous hop
        first = (mag, ph)
    eng.close()
    return mag, ph, pcm


@pytest.fixture(scope="module")
def per_hop():
    return per_hop_run(range(8))


def block_run(off, sizes, est=None, counts=None, dcs=DCS):
    """The block kernels on the designed signals in calls of ``sizes`` hops (``counts``: the ragged kernels, one call) from a reset, once
    per DC mode -> (mag [8,n,256], ph [8,n,257,2], {dc: pcm [8, n * 256]})."""
    x = TS.signals()
    est = TS.estimates() if est is None else est
    pcm = {}
    for dc in dcs:
        off.reset()
        mags, phs, outs, t = [], [], [], 0
        for n in sizes:
            px, pe = x[:, t * HOP:(t + n) * HOP], est[:, t:t + n]
            if counts is not None:          # NaN in every input row behind a count: never read
                px, pe = px.copy().reshape(8, n, HOP), pe.copy()
                for u, k in enumerate(counts):
                    px[u, k:], pe[u, k:] = np.nan, np.nan
                px = px.reshape(8, n * HOP)
            mags.append(off.stft_block_device(cuda(px), hops=counts).cpu().numpy())
            phs.append(off.debug_get("phasor_block", (n, 257, 2)))
            outs.append(off.istft_block_device(cuda(pe), dc_mode=dc, hops=None if counts is None else np.array(counts)).cpu().numpy())
            t += n
        pcm[dc] = np.concatenate(outs, axis=1)
        mag, ph = np.concatenate(mags, axis=1), np.concatenate(phs, axis=1)
    return mag, ph, pcm


@pytest.fixture(scope="module")
def offline():
    h = NutlsOffline(max_frames=N, utterances=8)
    yield h
    h.close()


@pytest.fixture(scope="module")
def block(offline):
    return block_run(offline, [N])


def check_against_float64(what, mag, ph, pcm, streams=None, n=N):
    """MAG, PHASOR, SYNTH (both DC modes, and the difference between them) and the exact conditions -> the ledger's worst ratios"""
    sel = list(range(8)) if streams is None else list(streams)
    led = TS.Ledger(what, streams)
    led.analysis(mag, ph, TS.analysis_reference()[sel, :n])
    want = {}
    for dc in DCS:
        want[dc], norm = TS.synthesis_reference(TS.estimates()[sel, :n], ph, dc)
        led.synthesis(pcm[dc], want[dc], norm)
    # edge - zero is the DC term alone: est[0] x Re phasor[0] / 512 x the inverse window, against the reference's difference
    led.synthesis(pcm["edge"].astype(np.float64) - pcm["zero"], want["edge"] - want["zero"], norm, kind="(edge - zero) / SYNTH")
    assert np.abs(want["edge"] - want["zero"]).max() > 0.1
    return led.close()


# ---- a, b. per-hop kernels -------------------------------------------------------------------------------------------------------------
def test_per_hop_kernels_against_float64(per_hop):
    """stft_hop_kernel / istft_hop_kernel<false>, 8 streams x 48 hops: analysis per frame, synthesis of ``estimates()`` per output hop in both DC
    modes on the phasors read back, and edge - zero against the reference's difference (the DC term: est[0] x Re phasor[0] / 512 x the
    inverse window -- a flipped DC sign doubles it)."""
    mag, ph, pcm = per_hop
    check_against_float64("per-hop kernels", mag, ph, pcm)


def test_per_hop_kernels_with_an_odd_batch_give_the_same_bits(per_hop):
    mag, ph, pcm = per_hop
    m3, p3, x3 = per_hop_run(ODD)
    sel = list(ODD)
    assert np.array_equal(m3, mag[sel]) and np.array_equal(p3, ph[sel])
    for dc in DCS:
        assert np.array_equal(x3[dc], pcm[dc][sel]), dc


# ---- c. block kernels ------------------------------------------------------------------------------------------------------------------
def test_block_kernels_against_float64(block):
    """stft_block_kernel<false> / istft_block_kernel<false, false>, one call of 48 hops of 8 utterances (three tiles of four runs each)."""
    mag, ph, pcm = block
    check_against_float64("block kernels", mag, ph, pcm)


def test_block_kernels_cut_across_runs_and_tiles_give_the_same_bits(offline, block):
    assert sum(CUT) == N
    mag, ph, pcm = block
    m, p, x = block_run(offline, CUT)
    assert np.array_equal(m, mag) and np.array_equal(p, ph)
    for dc in DCS:
        assert np.array_equal(x[dc], pcm[dc]), dc


def test_block_kernels_agree_with_the_per_hop_kernels(offline, block, per_hop):
    """Relative RMS per stream at DEVICE_REL: magnitudes (every stream by its own RMS), and the waveforms of both DC modes synthesised from
    the estimates on the strong bins (``strong_estimates``) by both families, each on its own phasors."""
    led = TS.Ledger("block against per-hop kernels")
    led.device("magnitudes", block[0], per_hop[0])
    est = TS.strong_estimates()
    _, _, xb = block_run(offline, [N], est=est)
    _, _, xh = per_hop_run(range(8), est=est)
    for dc in DCS:
        assert np.abs(xh[dc]).max(axis=1).min() > 0
        led.device("waveform, dc %s" % dc, xb[dc], xh[dc])
    # for the record: the same on all of estimates(), noise bins included (not asserted: see strong_estimates)
    for dc in DCS:
        print("block against per-hop kernels, all of estimates(), dc %s: relative RMS per stream %s" % (
            dc, " ".join("%s %.3g" % (TS.NAMES[b], TS.rel_rms(block[2][dc][b], per_hop[2][dc][b])) for b in range(8))))
    led.close()


# ---- d. ragged block kernels -----------------------------------------------------------------------------------------------------------
def test_ragged_block_kernels_are_the_uniform_ones_in_front_of_each_count(offline, block):
    """stft_block_kernel<true> / istft_block_kernel<true, false> with counts 48, 1, 17, 0, 16, 5, 33, 4 (NaN behind every count): the rows in
    front of a count carry the bits of the uniform call, the rows behind it are zeros.  Then a second ragged call that holds every other
    utterance (count 0: on a previous hop and an overlap tail that are not zero any more, except the one that never started) and gives
    the rest 8 more hops, and a uniform call of 8 hops: every utterance goes on with the bits of the uniform 48-hop call from where its
    own counts have brought it -- a count of 0 has left its carried hop and overlap untouched."""
    mag, ph, pcm = block
    m, p, x = block_run(offline, [N], counts=COUNTS, dcs=("zero", "edge"))          # (leaves the handle behind the ragged call in dc mode edge)
    for u, k in enumerate(COUNTS):
        assert np.array_equal(m[u, :k], mag[u, :k]) and np.array_equal(p[u, :k], ph[u, :k]), u
        assert not m[u, k:].any(), u
        for dc in DCS:
            assert np.array_equal(x[dc][u, :k * HOP], pcm[dc][u, :k * HOP]), (u, dc)
            assert not x[dc][u, k * HOP:].any(), (u, dc)
    sig, est = TS.signals(), TS.estimates()
    pos = list(COUNTS)
    for counts in ((0, 0, 8, 0, 8, 0, 8, 0), None):
        take = [min(8, N - pos[u]) if counts is None else counts[u] for u in range(8)]
        px, pe = np.full((8, 8, HOP), np.nan, np.float32), np.full((8, 8, 256), np.nan, np.float32)
        for u, n in enumerate(take):
            px[u, :n], pe[u, :n] = sig[u, pos[u] * HOP:(pos[u] + n) * HOP].reshape(n, HOP), est[u, pos[u]:pos[u] + n]
        if counts is None:          # (a uniform call reads every row: zeros behind the end of the audio)
            px, pe = np.nan_to_num(px), np.nan_to_num(pe)
        m2 = offline.stft_block_device(cuda(px.reshape(8, 8 * HOP)), hops=counts).cpu().numpy()
        p2 = offline.debug_get("phasor_block", (8, 257, 2))
        x2 = offline.istft_block_device(cuda(pe), dc_mode="edge", hops=None if counts is None else np.array(counts)).cpu().numpy()
        for u, n in enumerate(take):
            assert np.array_equal(m2[u, :n], mag[u, pos[u]:pos[u] + n]) and np.array_equal(p2[u, :n], ph[u, pos[u]:pos[u] + n]), (counts, u)
            assert np.array_equal(x2[u, :n * HOP], pcm["edge"][u, pos[u] * HOP:(pos[u] + n) * HOP]), (counts, u)
            if counts is not None:
                assert not m2[u, n:].any() and not x2[u, n * HOP:].any(), u
            pos[u] += n
    assert pos == [48, 9, 33, 8, 32, 13, 48, 12]


# ---- e. hop builds ---------------------------------------------------------------------------------------------------------------------
def hop_run(G, fusion, dc):
    """16 x ``enhance_hop`` of the designed signals on a fresh handle -> (mag_in [8,16,256], phasor [8,16,257,2], mag_out [8,16,256] -- each
    read after its hop --, pcm [8, 16 * 256])"""
    x = TS.signals()
    eng = NutlsEngine(batch=8, streams_per_workgroup=G, hop_fusion=fusion)
    assert eng.launches_per_hop == (1 if fusion else 3) and eng.streams_per_workgroup == G
    mags, phs, ests, outs = [], [], [], []
    for i in range(FUSED_HOPS):
        outs.append(eng.enhance_hop(cuda(hop_of(x, i)), dc).cpu().numpy())
        mags.append(eng.debug_get("mag_in", (256,)))
        phs.append(eng.debug_get("phasor", (257, 2)))
        ests.append(eng.debug_get("mag_out", (256,)))
    eng.close()
    return np.stack(mags, axis=1), np.stack(phs, axis=1), np.stack(ests, axis=1), np.concatenate(outs, axis=1)


@pytest.fixture(scope="module")
def three_launch():
    """{(G, dc): hop_run of the three-launch path (the per-hop kernels around the step)}"""
    return {(G, dc): hop_run(G, False, dc) for G in (1, 2) for dc in DCS}


@pytest.mark.parametrize("G", [1, 2])
def test_hop_builds_against_float64_and_the_three_launch_path(three_launch, G):
    """hop_prologue / hop_epilogue of the one- and two-stream hop builds, 8 streams x 16 hops with the model in between, both DC modes.
      * After every ``enhance_hop``: ``mag_in`` and ``phasor`` (the hop build fills the buffers of the three-launch path) against the
        analysis reference at MAG / PHASOR, and the exact conditions.
      * Every output hop against the float64 synthesis of what the model left (``mag_out``) on those phasors, at SYNTH x
        ``block_normaliser``: the model answers an impulse with a block whose energy sits in one half, and the hop that gets the other
        half is then at the level of the rounding of the whole block (over the hop's own normaliser: hop build 4.5 x SYNTH, the float32
        CPU transform on the same inputs 3.7 x; over the block normaliser 0.12 both; all four are printed).  This is the hop build's synthesis against double, DC sign on dc_neg included.
      * The waveform against a three-launch handle on the same hops at DEVICE_REL per stream -- on the bins whose phase is defined.  The
        two analyses give the bins that hold rounding noise alone unrelated phasors (dc_neg, nyquist, sine: nearly all bins; measured
        1.2e-4, 3.3e-4 and 3.0e-4 relative RMS on the raw waveforms, which are printed; the other five streams 1e-7 .. 2e-6), and
        whatever the model leaves on them is turned differently.  Synthesis is linear in the spectrum: each path's float64 synthesis of its own not-strong bins (its own
        ``mag_out``, its own phasors) is taken off its waveform, and what remains is compared."""
    keep = TS.strong_bins(TS.analysis_reference()[:, :FUSED_HOPS])
    led = TS.Ledger("hop build, %d stream%s per workgroup" % (G, "s" if G > 1 else ""))
    for dc in DCS:
        mag, ph, est, got = hop_run(G, True, dc)
        assert np.isfinite(est).all()
        led.analysis(mag, ph, TS.analysis_reference()[:, :FUSED_HOPS])
        want, norm = TS.synthesis_reference(est, ph, dc)
        full = TS.block_normaliser(est, ph, dc)
        led.synthesis(got, want, full, kind="synthesis of mag_out, dc %s / SYNTH (block normaliser)" % dc)
        cpu = TS.synthesis_float32(est, ph, dc)
        for name, arr in (("hop build", got), ("float32 CPU transform", cpu)):
            err = np.sqrt(np.mean((arr.astype(np.float64) - want).reshape(8, FUSED_HOPS, HOP) ** 2, axis=-1))
            print("%s on the model's outputs, dc %s: worst error / SYNTH over the hop's normaliser %.3g, over the block normaliser %.3g" % (
                name, dc, np.max(err[norm > 0] / norm[norm > 0]) / TS.SYNTH, np.max(err[full > 0] / full[full > 0]) / TS.SYNTH))
        defined = []
        for m_, p_, e_, pcm in ((mag, ph, est, got), three_launch[(G, dc)]):
            defined.append(pcm - (TS.synthesis_reference(e_, p_, dc)[0] - TS.synthesis_reference(e_, p_, dc, keep)[0]))
        assert min(np.sqrt(np.mean(d ** 2, axis=1)).min() for d in defined) > 0
        led.device("waveform on the defined bins against three launches, dc %s" % dc, defined[0], defined[1])
        raw = three_launch[(G, dc)][3]
        print("raw waveform against three launches, dc %s: relative RMS per stream %s" % (
            dc, " ".join("%s %.3g" % (TS.NAMES[b], TS.rel_rms(got[b], raw[b])) for b in range(8))))
    led.close()
