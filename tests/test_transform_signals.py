"""The designed signals and the float64 reference transforms of tests/transform_signals.py, checked on the CPU: the reference is the
restatement of the reference project's loop (``nunet_amd.stream_enhance``), a float32 CPU transform stays well inside every bound on every
signal (the conditioning cap: the bounds of tests/test_gpu_transforms.py measure the kernels, not the reference), and the signals reach the
special paths they were designed for."""
import numpy as np
import scipy.fft

import transform_signals as TS
from nunet_amd import stream_enhance as SE
from nunet_amd import topology as T

HOP = TS.HOP
NOISE = TS.NAMES.index("noise")


def test_signals_and_estimates_are_cached_and_read_only():
    x, est, X = TS.signals(), TS.estimates(), TS.analysis_reference()
    assert x.shape == (8, TS.N_HOPS * HOP) and x.dtype == np.float32 and not x.flags.writeable and TS.signals() is x
    assert est.shape == (8, TS.N_HOPS, 256) and est.dtype == np.float32 and not est.flags.writeable and TS.estimates() is est
    assert X.shape == (8, TS.N_HOPS, 257) and X.dtype == np.complex128 and not X.flags.writeable and TS.analysis_reference() is X
    assert TS.PHASOR == TS.MAG / TS.STRONG


def test_analysis_reference_is_the_host_loop_on_the_noise_stream():
    """``frame_magnitudes`` keeps (len - 256) // 256 = 47 frames of the 48 hops: the same float32 buffers, ``np.fft.rfft`` -- which keeps
    single precision on float32 input from numpy 2.0 on, so the two agree as a float32 CPU transform must: within CAP of MAG and PHASOR."""
    mags, phases = SE.frame_magnitudes(TS.signals()[NOISE])
    X = TS.analysis_reference()[NOISE]
    n = mags.shape[0]
    assert n == TS.N_HOPS - 1
    absX, scale = np.abs(X[:n]), TS.frame_scales(X[:n])
    assert np.all(np.abs(mags - absX).max(axis=-1) <= TS.CAP * TS.MAG * scale)
    strong = absX > TS.STRONG * scale[:, None]
    assert np.all(np.abs(np.exp(1j * phases) - TS.unit_phasors(X[:n]))[strong] <= TS.CAP * TS.PHASOR)
    # and for a handed-in block of PCM
    np.testing.assert_array_equal(TS.analysis_reference(TS.signals()[NOISE:NOISE + 1, :5 * HOP])[0], X[:5])


class _Replay:
    """A runner for ``real_time_speech_enhancer`` whose 'model' returns the rows of ``est`` in turn (states: zeros, echoed)."""

    def __init__(self, est):
        self.est, self.i, self.out = est, 0, SE.zero_state()

    def __call__(self, **feeds):
        assert feeds["input"].shape == (1, 1, T.N_BINS, 1)
        self.out["model_out"] = self.est[self.i].reshape(1, 1, T.N_BINS, 1)
        self.i += 1
        return self.out


def test_synthesis_reference_is_the_host_loop_on_the_noise_stream():
    """``real_time_speech_enhancer`` (np.fft.irfft of est x e^{j angle}, float32 blocks x the inverse window, float32 overlap-add) around a
    replay of ``estimates()``, against ``synthesis_reference`` on the same phasors.  The loop rounds a block to float32, multiplies by the
    window in float32 and adds two blocks in float32: at most 3 x 2^-24 (|a| + |b|) per sample, so 3 x 2^-24 x sqrt(2) = 2.6e-7 x the hop's
    normaliser in RMS."""
    x = TS.signals()[NOISE]
    est = TS.estimates()[NOISE]
    X = TS.analysis_reference()[NOISE]
    n = TS.N_HOPS - 1
    rotors = np.exp(1j * np.angle(X[:n]))          # (what the loop multiplies with)
    for dc in ("edge", "zero"):
        runner = _Replay(est)
        wave, _ = SE.real_time_speech_enhancer(x, runner, dc_mode=dc)
        assert runner.i == n and wave.shape == x.shape
        want, norm = TS.synthesis_reference(est[None, :n], rotors[None], dc)
        got = np.concatenate([np.zeros(HOP), wave])[:n * HOP].reshape(n, HOP)          # (the loop drops the first output hop)
        err = np.sqrt(np.mean((got[1:] - want[0].reshape(n, HOP)[1:]) ** 2, axis=-1))
        assert (norm[0, 1:] > 0).sum() > 30
        assert np.all(err <= 3 * 2.0 ** -24 * np.sqrt(2.0) * norm[0, 1:]), dc
        assert np.all(got[1:][norm[0, 1:] == 0] == 0)
    edge, zero = (TS.synthesis_reference(est[None], TS.unit_phasors(X)[None], dc)[0] for dc in ("edge", "zero"))
    assert np.abs(edge - zero).max() > 0.1          # (the DC bin matters on these estimates: 150 / 512 per sample where a frame's level is 30)


def _float32_transform():
    """Analysis and synthesis of the designed signals with scipy.fft in single precision -> (mag [8,48,256], ph [8,48,257,2], {dc: pcm})."""
    frames = TS.windowed_frames(TS.signals())
    spec = scipy.fft.rfft(frames, axis=-1)
    assert frames.dtype == np.float32 and spec.dtype == np.complex64
    mag = np.abs(spec)
    assert mag.dtype == np.float32
    safe = np.where(mag > 0, mag, np.float32(1))          # (re / |X|, im / |X| as the kernels divide: a complex division is not exact on a real bin)
    ph = np.stack([np.where(mag > 0, spec.real / safe, np.float32(1)), np.where(mag > 0, spec.imag / safe, np.float32(0))], axis=-1)
    assert ph.dtype == np.float32
    rot = TS.unit_phasors(TS.analysis_reference())          # the float64 phasors (rounded to complex64 on the way in)
    pcm = {dc: TS.synthesis_float32(TS.estimates(), rot, dc) for dc in ("edge", "zero")}
    return mag[..., 1:], ph, pcm


def test_conditioning_cap_a_float32_cpu_transform_uses_a_quarter_of_every_bound_at_most():
    """pocketfft in single precision against the float64 reference, per frame and per output hop on every signal.  Measured: 0.12 of MAG
    (impulse), 0.023 of PHASOR (sine), 0.13 of SYNTH (nyquist); the worst ratios are printed."""
    mag, ph, pcm = _float32_transform()
    led = TS.Ledger("float32 CPU transform")
    led.analysis(mag, ph, TS.analysis_reference())
    for dc in ("edge", "zero"):
        want, norm = TS.synthesis_reference(TS.estimates(), TS.unit_phasors(TS.analysis_reference()), dc)
        led.synthesis(pcm[dc], want, norm)
    worst = led.close()          # (the exact conditions hold for the CPU transform too)
    for kind in ("magnitudes / MAG", "phasors / PHASOR", "synthesis / SYNTH"):
        assert worst[kind] <= TS.CAP, (kind, worst[kind])


def test_the_signals_reach_what_they_were_designed_for():
    X = TS.analysis_reference()
    absX, scale = np.abs(X), TS.frame_scales(X)
    s = {name: i for i, name in enumerate(TS.NAMES)}
    x = TS.signals()
    # impulse: a single sample per frame, and frames whose whole spectrum lies at 1e-7
    frames = TS.windowed_frames(x[s["impulse"]][None])[0]
    assert np.array_equal((x[s["impulse"]].reshape(TS.N_HOPS, HOP) != 0).sum(axis=1), 1 - np.arange(TS.N_HOPS) % 2)
    assert np.all((frames != 0).sum(axis=1) == 1)
    quiet = scale[s["impulse"]] < 1e-6
    assert quiet.sum() >= 2 and np.all(scale[s["impulse"]] > 0)
    assert np.all(absX[s["impulse"]][quiet].min(axis=-1) > 0.99 * scale[s["impulse"]][quiet])          # flat: every bin carries the sample
    # dc_neg: bin 0 negative and the strongest bin of every frame
    assert np.all(X[s["dc_neg"], :, 0].real < 0) and np.all(absX[s["dc_neg"], :, 0] == scale[s["dc_neg"]])
    # sine: a positive, strong bin 0 beside the tone (the other sign)
    assert np.all(X[s["sine"], :, 0].real > 0) and np.all(absX[s["sine"], :, 0] > TS.STRONG * scale[s["sine"]])
    # nyquist: bin 256 is the maximum
    assert np.all(absX[s["nyquist"]].argmax(axis=-1) == 256)
    # signs: full scale
    assert np.abs(x[s["signs"]]).min() == 1.0 and scale[s["signs"]].min() > 10.0
    # tiny
    assert 1e-6 < scale[s["tiny"]].max() < 1e-4
    # gaps: all-zero frames, frames with one silent half
    assert (scale[s["gaps"]] == 0).sum() >= 2
    g = x[s["gaps"]].reshape(TS.N_HOPS, HOP)
    silent = ~g.any(axis=1)
    assert (silent[:-1] & ~silent[1:]).any() and (~silent[:-1] & silent[1:]).any()
    # together: every bin 0..256 strong in some frame, both DC signs strong, every frame compared
    strong = (scale[..., None] > 0) & (absX > TS.STRONG * scale[..., None])
    assert strong.any(axis=(0, 1)).all()
    dc = X[..., 0].real
    assert (strong[..., 0] & (dc < 0)).any() and (strong[..., 0] & (dc > 0)).any()
    live = scale > 0
    assert np.all(strong.any(axis=-1) == live)          # a live frame has strong bins: its magnitudes AND phasors are compared
    assert live.sum() + (~live).sum() == 8 * TS.N_HOPS and (~live).sum() >= 2          # an empty one is held to the exact conditions
    # the span of frame scales the per-frame bounds cover
    assert scale[live].max() / scale[live].min() > 1e8


def test_the_estimates_reach_what_they_were_designed_for():
    est = TS.estimates()
    level = est.max(axis=-1)
    for s in range(8):
        zero = level[s] == 0
        assert (zero[:-1] & zero[1:]).any(), s                                            # two all-zero frames in a row
        _, norm = TS.synthesis_reference(est[s:s + 1], TS.unit_phasors(TS.analysis_reference()[s:s + 1]), "edge")
        assert (norm == 0).any() and (norm > 0).sum() > 30, s
    jumps = level[:, 1:] / np.maximum(level[:, :-1], 1e-30)
    assert ((jumps > 1e4) & (level[:, :-1] > 0)).any() and ((jumps < 1e-4) & (level[:, 1:] > 0)).any()      # 1e-3 <-> 30 between neighbours
    big = est[:, ::4]
    assert np.all(big[..., 0] == big[..., 255]) and np.all(big[..., 0] >= big.max(axis=-1) * 0.99) and big[..., 0].max() == 150.0
    # the ledger reports a miss, with its place
    led = TS.Ledger("self-test")
    X = TS.analysis_reference()
    mag = np.abs(X[..., 1:]).astype(np.float32)
    u = TS.unit_phasors(X)
    ph = np.stack([u.real, u.imag], axis=-1).astype(np.float32)
    ph[1, 5, 0, 0] = 1.0                                                                 # dc_neg: a flipped DC sign
    mag[0, 2, 17] *= 1.0 + 1e-5                                                          # impulse: 1e-5 of one bin of one frame
    led.analysis(mag, ph, X)
    assert len(led.misses) == 3 and "stream impulse frame 2" in led.misses[0] and "stream dc_neg frame 5 bin 0" in led.misses[1]
    assert "DC phasor of stream dc_neg frame 5" in led.misses[2]
