"""``-m gpu``: the attenuation limit (include/nutls.h, "Attenuation limit") -- ``istft_hop_kernel<true>`` (csrc/stft.hip) and
``istft_block_kernel<RAGGED, true>``, uniform and ragged (csrc/stft_block.hip on ``synthesise_frame_mix`` of csrc/stft_wave.hpp) against the float64
synthesis of the rows mixed in double, on the designed signals and estimates of tests/transform_signals.py with the limits ``L`` of
tests/atten_limit_reference.py; the exact ends inside one launch; the same bits however the audio is cut; and, with the model in between,
limit 0 as the path it was, linearity in the limit, masks, settings, refusals and the corpus scheduler.

The shape is that of tests/test_gpu_transforms.py: analysis, magnitudes and phasors read back, ``estimates()`` where the model's output
goes, synthesis; the reference uses the phasors read back and the ``l`` the getter returns, ``c = float32(1 - l)``.

Measured on an MI355X (worst ratio to the bound): synthesis of the mixed rows / SYNTH x block normaliser, per-hop mix kernel 0.100 (edge) /
0.088 (zero), block mix kernel 0.113 / 0.118 -- the float32 CPU transform on the same rows 0.110 / 0.109 (tests/test_atten_limit_abi.py);
block against per-hop mix kernel 0.050 / 0.054 of DEVICE_REL (sine); linearity with the model in between at most 0.02 of DEVICE_REL
(enhance_hop 0.011, ragged blocks 0.006, enhance_hop_pcm 0.018 at 48 kHz and 0.019 at 8 kHz, baseline 0.011).
"""
import ctypes

import numpy as np
import pytest
import torch      # (before the first handle: torch must bring up the HIP runtime it ships with itself)

import atten_limit_reference as A
import transform_signals as TS
from nunet_amd import NutlsEngine, NutlsOffline

pytestmark = pytest.mark.gpu

HOP, N = TS.HOP, TS.N_HOPS
DCS = ("edge", "zero")
ODD = (0, 1, 6)
CUT = (1, 3, 4, 5, 16, 17, 2)
COUNTS = (48, 1, 17, 0, 16, 5, 33, 4)
MODEL = (TS.NAMES.index("noise"), TS.NAMES.index("sine"), TS.NAMES.index("gaps"))      # the streams of the runs with the model
MIXED = np.float32([0.5, 0.1, 0.999])


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


def per_hop_run(streams, limits, est=None, echo=()):
    """The per-hop kernels on ``streams`` of the designed signals with ``limits``: 48 x (stft_hop, read mag_in and phasor, estimates -> the
    model-output buffer, istft_hop), once per DC mode from a reset.  ``echo``: rows whose estimates are the magnitudes just read back.
    -> (mag [B,48,256], ph [B,48,257,2], {dc: pcm [B, 48 * 256]}, the limits the getter returns)"""
    x, est = TS.signals()[list(streams)], (TS.estimates() if est is None else est)[list(streams)]
    B = len(streams)
    eng = NutlsEngine(batch=B)
    eng.set_atten_limit(limits)
    got_limits = eng.atten_limit
    assert eng.launches_per_hop == 3 and got_limits.dtype == np.float32 and np.array_equal(got_limits, np.float32(limits))
    hip = _hip()
    y = torch.empty(B, HOP, device="cuda")
    pcm = {}
    for dc in DCS:
        eng.reset()
        assert np.array_equal(eng.atten_limit, got_limits)          # a setting, not stream state
        mags, phs, outs = [], [], []
        for i in range(N):
            eng.stft_hop(cuda(hop_of(x, i)))
            mags.append(eng.debug_get("mag_in", (256,)))
            phs.append(eng.debug_get("phasor", (257, 2)))
            rows = est[:, i].copy()
            for b in echo:
                rows[b] = mags[-1][b]
            rows = cuda(rows)
            torch.cuda.synchronize()
            # hipMemcpyDeviceToDevice = 3
            assert hip.hipMemcpy(ctypes.c_void_p(eng.io_out_ptr), ctypes.c_void_p(rows.data_ptr()), ctypes.c_size_t(B * 256 * 4), 3) == 0
            eng.istft_hop(y, dc)
            outs.append(y.cpu().numpy().copy())
        pcm[dc] = np.concatenate(outs, axis=1)
        mag, ph = np.stack(mags, axis=1), np.stack(phs, axis=1)
    eng.close()
    return mag, ph, pcm, got_limits


def block_run(off, sizes, limits, est=None, counts=None, dcs=DCS, echo=(), streams=range(8)):
    """The block kernels on the designed signals in calls of ``sizes`` hops (``counts``: the ragged kernel, one call, NaN in every estimate,
    noisy and PCM row behind a count) from a reset, once per DC mode, through ``istft_block_device(est, noisy=mag)``.
    -> (mag [U,n,256], ph [U,n,257,2], {dc: pcm [U, n * 256]}, the limits the getter returns)"""
    sel = list(streams)
    U = len(sel)
    x = TS.signals()[sel]
    est = (TS.estimates() if est is None else est)[sel]
    off.set_atten_limit(limits)
    got_limits = off.atten_limit
    assert np.array_equal(got_limits, np.float32(limits))
    pcm = {}
    for dc in dcs:
        off.reset()
        assert np.array_equal(off.atten_limit, got_limits)
        mags, phs, outs, t = [], [], [], 0
        for n in sizes:
            px, pe = x[:, t * HOP:(t + n) * HOP], est[:, t:t + n].copy()
            if counts is not None:
                px = px.copy().reshape(U, n, HOP)
                for u, k in enumerate(counts):
                    px[u, k:], pe[u, k:] = np.nan, np.nan
                px = px.reshape(U, n * HOP)
            mag = off.stft_block_device(cuda(px), hops=counts)
            mags.append(mag.cpu().numpy())
            phs.append(off.debug_get("phasor_block", (n, 257, 2)))
            for u in echo:
                pe[u] = mags[-1][u]
            if counts is not None:          # the analysis wrote zeros behind the counts: poison the noisy rows there too
                mag = mag.clone()
                for u, k in enumerate(counts):
                    mag[u, k:] = float("nan")
            outs.append(off.istft_block_device(cuda(pe), dc_mode=dc, hops=None if counts is None else np.array(counts), noisy=mag).cpu().numpy())
            t += n
        pcm[dc] = np.concatenate(outs, axis=1)
        mag_all, ph_all = np.concatenate(mags, axis=1), np.concatenate(phs, axis=1)
    return mag_all, ph_all, pcm, got_limits


@pytest.fixture(scope="module")
def per_hop():
    return per_hop_run(range(8), A.L)


@pytest.fixture(scope="module")
def offline():
    h = NutlsOffline(max_frames=N, utterances=8)
    yield h
    h.close()


@pytest.fixture(scope="module")
def block(offline):
    return block_run(offline, [N], A.L)


def check_against_float64(what, run, streams=None):
    """SYNTH x the output hop's ``block_normaliser``, both DC modes, against ``synthesis_reference`` of the rows mixed in double -> worst ratios.
    The normaliser is the one tests/test_atten_limit_abi.py conditions this reference with, and the one tests/test_gpu_transforms.py holds
    the hop builds to on the model's outputs, for the same reason: the share ``l x`` of a mixed row synthesises the windowed input frame back,
    and where that frame has a silent half (the first frame of a stream, the frame behind the end of ``gaps``) the block's energy sits in the
    other output hop while the rounding of a float32 transform is spread over the whole block.  Over the hop's own normaliser the float32
    CPU transform misses SYNTH on the same inputs too (printed there and here; measured on an MI355X: per-hop kernel 49.7 x SYNTH, block
    kernel 52.8 x, both at output hop 0 of ``signs``)."""
    mag, ph, pcm, limits = run
    sel = list(range(8)) if streams is None else list(streams)
    mixed = A.mix64(mag, TS.estimates()[sel], limits)
    led = TS.Ledger(what, streams)
    for dc in DCS:
        want, norm = TS.synthesis_reference(mixed, ph, dc)
        full = TS.block_normaliser(mixed, ph, dc)
        assert np.all(full[norm > 0] > 0)          # (no output hop with a normaliser of its own is left out)
        led.synthesis(pcm[dc], want, full, kind="synthesis of the mixed rows, dc %s / SYNTH (block normaliser)" % dc)
        err = np.sqrt(np.mean((pcm[dc].astype(np.float64) - want).reshape(len(sel), -1, HOP) ** 2, axis=-1))
        print("%s, dc %s: worst error / SYNTH over the hop's own normaliser %.3g" % (what, dc, np.max(err[norm > 0] / norm[norm > 0]) / TS.SYNTH))
    return led.close()


# ---- 1, 2. against float64 -------------------------------------------------------------------------------------------------------------
def test_per_hop_mix_kernel_against_float64(per_hop):
    """istft_hop_kernel<true>, 8 streams with the limits L x 48 hops, both DC modes.  The mix adds two roundings, at most
    2^-23 (l |x| + c |e|) per bin: under 6 % of the bound."""
    check_against_float64("per-hop mix kernel", per_hop)


def test_block_mix_kernel_against_float64(block):
    """istft_block_kernel<false, true>, one call of 48 hops of 8 utterances (three tiles of four runs each)."""
    check_against_float64("block mix kernel", block)


# ---- 3. exactness inside one launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signal", ["sine", "noise"])
def test_limit_one_and_limit_zero_meet_bit_for_bit_in_one_launch(signal):
    """Row A: l = 1 and the designed estimates -> m' = x.  Row B: l = 0 and the magnitudes read back as its estimates -> m' = e = x.  Same
    signal, same phasors: the rows leave the per-hop and the block kernel bit-identical in both DC modes.  (``fma(l, x - e, e)`` fails here:
    at l = 1 it returns (x - e) + e, which is not x.)"""
    s = TS.NAMES.index(signal)
    mag, ph, pcm, _ = per_hop_run((s, s), (1.0, 0.0), echo=(1,))
    assert np.array_equal(mag[0], mag[1]) and np.array_equal(ph[0], ph[1])
    off = NutlsOffline(max_frames=N, utterances=2)
    try:
        _, _, blk, _ = block_run(off, [N], (1.0, 0.0), echo=(1,), streams=(s, s))
    finally:
        off.close()
    for dc in DCS:
        assert np.abs(pcm[dc][0]).max() > 0 and np.abs(blk[dc][0]).max() > 0
        assert pcm[dc][0].tobytes() == pcm[dc][1].tobytes(), ("per-hop", dc)
        assert blk[dc][0].tobytes() == blk[dc][1].tobytes(), ("block", dc)


# ---- 4. same bits however the audio is cut ---------------------------------------------------------------------------------------------
def test_per_hop_mix_kernel_with_an_odd_batch_gives_the_same_bits(per_hop):
    sel = list(ODD)
    m3, p3, x3, _ = per_hop_run(ODD, A.L[sel])
    assert np.array_equal(m3, per_hop[0][sel]) and np.array_equal(p3, per_hop[1][sel])
    for dc in DCS:
        assert np.array_equal(x3[dc], per_hop[2][dc][sel]), dc


def test_block_mix_kernel_cut_across_runs_and_tiles_gives_the_same_bits(offline, block):
    assert sum(CUT) == N
    m, p, x, _ = block_run(offline, CUT, A.L)
    assert np.array_equal(m, block[0]) and np.array_equal(p, block[1])
    for dc in DCS:
        assert np.array_equal(x[dc], block[2][dc]), dc


def test_ragged_mix_kernel_is_the_uniform_one_in_front_of_each_count(offline, block):
    """istft_block_kernel<true, true> with counts 48, 1, 17, 0, 16, 5, 33, 4 and NaN in every estimate, noisy and PCM row behind a count: the
    uniform call's bits in front of each count, zeros behind it.  Utterance 3 (count 0) keeps its overlap tail: a uniform call of 8 hops
    afterwards gives it the first 8 hops of the uniform run, as if the ragged block had not been there."""
    _, _, pcm = block[:3]
    _, _, x, _ = block_run(offline, [N], A.L, counts=COUNTS, dcs=("zero", "edge"))          # (leaves the handle behind the ragged call in dc mode edge)
    for u, k in enumerate(COUNTS):
        for dc in DCS:
            assert np.array_equal(x[dc][u, :k * HOP], pcm[dc][u, :k * HOP]), (u, dc)
            assert not x[dc][u, k * HOP:].any(), (u, dc)
    u = COUNTS.index(0)
    mag = offline.stft_block_device(cuda(TS.signals()[:, :8 * HOP]))
    y = offline.istft_block_device(cuda(TS.estimates()[:, :8]), dc_mode="edge", noisy=mag).cpu().numpy()
    assert np.array_equal(y[u], pcm["edge"][u, :8 * HOP])
    assert np.abs(pcm["edge"][u, :8 * HOP]).max() > 0


# ---- 5. per-hop against block ----------------------------------------------------------------------------------------------------------
def test_block_mix_kernel_agrees_with_the_per_hop_mix_kernel(offline):
    est = TS.strong_estimates()          # (the two families give the bins that hold rounding noise alone unrelated phasors)
    _, _, xb, _ = block_run(offline, [N], A.L, est=est)
    _, _, xh, _ = per_hop_run(range(8), A.L, est=est)
    led = TS.Ledger("block against per-hop mix kernel")
    for dc in DCS:
        assert np.abs(xh[dc]).max(axis=1).min() > 0
        led.device("waveform, dc %s" % dc, xb[dc], xh[dc])
    led.close()


# ---- 6. limit 0 is today's path --------------------------------------------------------------------------------------------------------
def test_limit_zero_is_the_path_it_was():
    """A handle that never had a limit, one set to limits and back to NULL, one set to zeros from the start: identical bits through
    ``enhance_hop`` (B = 3, 6 hops, the real model) and through ``enhance_block_device`` (2 utterances x 20 hops, cut at 7)."""
    x = TS.signals()[list(MODEL)]
    outs = []
    for prepare in (lambda h: None, lambda h: (h.set_atten_limit(MIXED), h.set_atten_limit()), lambda h: h.set_atten_limit(0.0)):
        eng = NutlsEngine(batch=3)
        prepare(eng)
        assert not eng.atten_limit.any()
        outs.append(np.concatenate([eng.enhance_hop(cuda(hop_of(x, i))).cpu().numpy() for i in range(6)], axis=1))
        eng.close()
    assert np.abs(outs[0]).max() > 0 and outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()
    outs = []
    for prepare in (lambda h: None, lambda h: (h.set_atten_limit(MIXED[:2]), h.set_atten_limit()), lambda h: h.set_atten_limit([0.0, 0.0])):
        off = NutlsOffline(max_frames=20, utterances=2)
        prepare(off)
        assert not off.atten_limit.any()
        outs.append(np.concatenate([off.enhance_block_device(cuda(x[:2, a * HOP:b * HOP])).cpu().numpy() for a, b in ((0, 7), (7, 20))], axis=1))
        off.close()
    assert np.abs(outs[0]).max() > 0 and outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


# ---- 7. end to end with the model: linearity -------------------------------------------------------------------------------------------
def check_linear(what, run, limits=MIXED):
    """``run(limits or None) -> [3, samples]``: out_l against (1 - l) out_0 + l out_1 per stream, relative RMS at DEVICE_REL against the
    larger RMS of out_0 and out_1 (mix and synthesis are linear: what is left is rounding)."""
    out0, out1, outl = (np.asarray(run(l), np.float64) for l in (None, np.ones(3, np.float32), limits))
    rms = lambda a: np.sqrt(np.mean(a ** 2, axis=-1))
    scale = np.maximum(rms(out0), rms(out1))
    l = np.float32(limits).astype(np.float64)[:, None]
    err = rms(outl - ((1.0 - l) * out0 + l * out1))
    live = scale > 0
    ratio = err[live] / scale[live] / TS.DEVICE_REL
    print("%s: linearity, relative RMS per stream / DEVICE_REL: %s" % (what, " ".join("%.3g" % r for r in ratio)))
    assert np.isfinite(outl).all() and not outl[~live].any()
    assert np.all(rms(out1 - out0)[live] > 0.05 * scale[live])          # (the two ends differ: the comparison is not empty)
    assert np.all(ratio <= 1.0), ratio
    return live


def hop_runner(make, pcm_hops, call="enhance_hop"):
    def run(limits):
        eng = make()
        try:
            if limits is not None:
                eng.set_atten_limit(limits)
            return np.concatenate([getattr(eng, call)(p).cpu().numpy() for p in pcm_hops], axis=1)
        finally:
            eng.close()
    return run


def test_enhance_hop_is_linear_in_the_limit():
    x = TS.signals()[list(MODEL)]
    live = check_linear("enhance_hop", hop_runner(lambda: NutlsEngine(batch=3), [cuda(hop_of(x, i)) for i in range(12)]))
    assert live.all()


def test_ragged_blocks_and_the_pcm_gateway_are_linear_in_the_limit():
    x = TS.signals()[list(MODEL)]
    counts = np.array((12, 5, 0), np.int32)

    def ragged(limits):
        off = NutlsOffline(max_frames=12, utterances=3)
        try:
            if limits is not None:
                off.set_atten_limit(limits)
            return off.enhance_block_device(cuda(x[:, :12 * HOP]), hops=counts).cpu().numpy()
        finally:
            off.close()
    live = check_linear("enhance_block_device, ragged", ragged)
    assert list(live) == [True, True, False]
    rng = np.random.default_rng(TS.SEED + 2)
    for rate in (48000, 8000):
        def make(rate=rate):
            eng = NutlsEngine(batch=3)
            eng.set_pcm_format(rate, "float32")
            assert eng.pcm_upper_band == 0.0
            return eng
        S = 256 * rate // 16000
        hops = [cuda(0.1 * rng.standard_normal((3, S))) for _ in range(12)]
        assert check_linear("enhance_hop_pcm at %d Hz" % rate, hop_runner(make, hops, "enhance_hop_pcm")).all()


def test_enhance_hop_of_the_baseline_variant_is_linear_in_the_limit():
    from nunet_amd.weights import synthetic_weights, write_blob
    blob = write_blob(synthetic_weights("baseline", seed=4321, bias_std=0.1, affine_jitter=0.1), int8_convs=True)
    x = TS.signals()[list(MODEL)]
    live = check_linear("enhance_hop, baseline", hop_runner(lambda: NutlsEngine(blob, batch=3, variant="baseline"), [cuda(hop_of(x, i)) for i in range(12)]))
    assert live.all()


# ---- 8. masks and settings -------------------------------------------------------------------------------------------------------------
def test_masks_and_settings():
    x = TS.signals()[list(MODEL)]
    hops = [cuda(hop_of(x, i)) for i in range(6)]

    def run(active=None, change=None):
        eng = NutlsEngine(batch=3)
        eng.set_atten_limit(MIXED)
        outs = []
        for i, p in enumerate(hops):
            if change is not None and i == 3:
                eng.set_atten_limit(change)
            outs.append(eng.enhance_hop(p, active=active).cpu().numpy())
        eng.close()
        return np.concatenate(outs, axis=1)
    plain = run()
    masked = run(active=torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda"))
    assert np.array_equal(masked[[0, 2]], plain[[0, 2]]) and not masked[1].any() and np.abs(plain[1]).max() > 0
    changed = run(change=np.float32([0.5, 0.7, 0.999]))
    assert np.array_equal(changed[[0, 2]], plain[[0, 2]])
    assert np.array_equal(changed[1, :3 * HOP], plain[1, :3 * HOP]) and not np.array_equal(changed[1, 3 * HOP:], plain[1, 3 * HOP:])
    eng = NutlsEngine(batch=3)
    eng.set_atten_limit(db=[6.0, None, 20.0])
    want = eng.atten_limit
    assert want[1] == 0 and want[2] == np.float32(0.1) and 0.5 < want[0] < 0.51
    eng.enhance_hop(hops[0])
    eng.reset()
    assert np.array_equal(eng.atten_limit, want)
    eng.set_pcm_format(48000, "int16")
    assert np.array_equal(eng.atten_limit, want)
    eng.reset(1)
    eng.set_mode("launches")
    eng.set_mode("fused")
    assert np.array_equal(eng.atten_limit, want)
    eng.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    eng = NutlsEngine(batch=3, hop_fusion=True)
    with pytest.raises(ValueError, match="nutls_set_atten_limit"):
        eng.set_atten_limit(MIXED)
    assert not eng.atten_limit.any() and eng.launches_per_hop == 1
    eng.set_atten_limit(0.0)
    eng.set_atten_limit()
    eng.set_hop_fusion(False)
    eng.set_atten_limit(MIXED)
    with pytest.raises(ValueError, match="nutls_set_hop_fusion"):
        eng.set_hop_fusion(True)
    assert eng.launches_per_hop == 3 and np.array_equal(eng.atten_limit, MIXED)
    for bad in ([0.5, 1.5, 0.0], [0.5, float("nan"), 0.0], [-0.25, 0.0, 0.0], [0.5, 0.5], [0.5] * 4):
        with pytest.raises(ValueError, match="nutls_set_atten_limit"):
            eng.set_atten_limit(bad)
        assert np.array_equal(eng.atten_limit, MIXED)
    with pytest.raises(ValueError):
        eng.set_atten_limit(db=-3.0)
    assert np.array_equal(eng.atten_limit, MIXED)
    eng.set_atten_limit()
    eng.set_hop_fusion(True)
    assert eng.launches_per_hop == 1
    eng.close()


# ---- 10. the corpus scheduler ----------------------------------------------------------------------------------------------------------
def test_enhance_many_sets_each_recordings_limit():
    """5 recordings of 3 .. 20 hops through 2 slots, one cap per recording: each result is that recording alone through
    ``enhance(wave, atten_lim_db=...)`` of a one-utterance handle, to DEVICE_REL."""
    rng = np.random.default_rng(TS.SEED + 3)
    lengths = (3, 20, 7, 12, 5)
    dbs = [6.0, None, 20.0, 0.0, 40.0]
    noise = TS.signals()[TS.NAMES.index("noise")]
    waves = [np.ascontiguousarray(noise[i * 700:i * 700 + (n + 1) * HOP + 17 * i]) + np.float32(0.01) * rng.standard_normal((n + 1) * HOP + 17 * i).astype(np.float32)
             for i, n in enumerate(lengths)]
    off = NutlsOffline(max_frames=8, utterances=2)
    got = off.enhance_many_atten(waves, dbs)
    off.close()
    one = NutlsOffline(max_frames=8, utterances=1)
    for i, (w, d) in enumerate(zip(waves, dbs)):
        one.reset()
        one.set_atten_limit()
        want = one.enhance(w, atten_lim_db=d)
        assert got[i].shape == want.shape and np.abs(want).max() > 0
        assert TS.rel_rms(got[i], want) <= TS.DEVICE_REL, (i, TS.rel_rms(got[i], want))
    one.close()
