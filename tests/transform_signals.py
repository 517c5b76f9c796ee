"""Designed signals, designed model outputs and float64 reference transforms for the three implementations of the 512-point analysis
and synthesis (csrc/stft.hip, csrc/stft_block.hip on csrc/stft_wave.hpp, the hop builds of csrc/fused_step.hip) -- a plain helper
module: the CPU tests of tests/test_transform_signals.py and the GPU tests of tests/test_gpu_transforms.py share it, and its caches.

The reference is ``np.fft`` in double on exactly what the kernels multiply: the float32 hops times the float32 window taps
(``stream_enhance.hop_frames x analysis_window()``), and the float32 ``inverse_window()`` taps behind the inverse transform.  Every bound
is applied per frame (analysis) or per output hop (synthesis), so that a frame at 1e-7 is held to the same relative error as one at 100."""
import functools

import numpy as np

from nunet_amd import stream_enhance as SE

SEED = 23
HOP = SE.FRAME_STEP
N_HOPS = 48
NAMES = ("impulse", "dc_neg", "nyquist", "signs", "sine", "tiny", "gaps", "noise")
IMPULSE_POSITIONS = (0, 1, 127, 128, 254, 255)

MAG = 2e-6
"""max_k |got - |X_f,k|| < MAG x scale_f, scale_f = max_k |X_f,k| of the SAME frame: the project's own number (tests/test_gpu_frontend.py,
tests/test_gpu_enhance_block.py: 2e-6 x max |X| over the whole clip), applied per frame instead of per clip."""
STRONG = 1e-2
"""A bin is strong where |X_f,k| > STRONG x scale_f; phasors are compared on strong bins, on every frame that has a scale at all."""
PHASOR = MAG / STRONG
"""|got - X/|X|| < PHASOR = 2e-4 on strong bins: an error of MAG x scale_f on a bin of at least STRONG x scale_f turns its phasor by at most
MAG / STRONG -- what the magnitude bound implies (and the figure tests/test_gpu_frontend.py uses for its strong bins)."""
SYNTH = 2e-6
"""RMS of (got - want) over an output hop < SYNTH x that hop's normaliser (the root mean square of the two half blocks that are added,
taken before the sum so that a cancellation cannot shrink it).  A float32 CPU transform (pocketfft) lies at 2.6e-7 of the normaliser on
these inputs; the bound leaves the device transforms a factor of about 8 over it (measured on an MI355X: 2.5e-7, all three of them)."""
DEVICE_REL = 1e-5
"""Relative RMS per stream between two device paths, as in tests/test_gpu_hop_fusion.py and tests/test_gpu_enhance_block.py."""
CAP = 1.0 / 4.0
"""The share of MAG, PHASOR and SYNTH that a float32 CPU transform may use on these signals: the reference is then sharp enough."""

LEVELS = np.float32([0.0, 1e-3, 1.0, 30.0])


@functools.lru_cache(maxsize=None)
def signals():
    """[8, N_HOPS * 256] float32, read-only; the streams in the order of NAMES:
    impulse  one sample of +-1 in every second hop, at 0, 1, 127, 128, 254, 255 in turn: every frame holds a single sample; position 0 as the
             old hop and position 255 as the new hop meet the analysis window's 1e-7 end taps (a full flat spectrum at 1e-7)
    dc_neg   -0.75 everywhere: the DC phasor is -1, every other bin leakage
    nyquist  0.9 (-1)^n
    signs    +-1 at random: full scale
    sine     0.5 cos(2 pi 37.5 n / 512 + 0.3) + 0.1: between two bins, positive DC
    tiny     1e-6 x white noise
    gaps     zeros in hops 0..2, 0.3 x white noise in hops 3..40, zeros behind: all-zero frames and frames with one silent half
    noise    0.05 x white noise"""
    rng = np.random.default_rng(SEED)
    total = N_HOPS * HOP
    n = np.arange(total)
    x = np.zeros((len(NAMES), total), np.float64)
    for j, hop in enumerate(range(0, N_HOPS, 2)):
        x[0, hop * HOP + IMPULSE_POSITIONS[j % 6]] = rng.choice([-1.0, 1.0])
    x[1] = -0.75
    x[2] = 0.9 * (1.0 - 2.0 * (n & 1))
    x[3] = rng.choice([-1.0, 1.0], size=total)
    x[4] = 0.5 * np.cos(2.0 * np.pi * 37.5 * n / SE.FRAME_LEN + 0.3) + 0.1
    x[5] = 1e-6 * rng.standard_normal(total)
    x[6, 3 * HOP:41 * HOP] = 0.3 * rng.standard_normal(38 * HOP)
    x[7] = 0.05 * rng.standard_normal(total)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def windowed_frames(pcm):
    """``pcm [S, n * 256]`` -> the float32 windowed analysis buffers ``[S, n, 512]`` (frame i = hop i - 1, zeros for the first, and hop i)."""
    pcm = np.asarray(pcm, np.float32)
    win = SE.analysis_window()
    pad = np.zeros(SE.FRAME_LEN - HOP, np.float32)          # (hop_frames keeps (len - 256) // 256 frames)
    out = np.stack([SE.hop_frames(np.concatenate([row, pad])) * win for row in pcm])
    assert out.dtype == np.float32 and out.shape[1] * HOP == pcm.shape[1]
    return out


def analysis_reference(pcm=None):
    """float64 ``X [S, n, 257]``: ``np.fft.rfft`` of the float32 windowed frames, promoted.  ``pcm``: ``[S, n * 256]``; None: ``signals()``
    (computed once, read-only)."""
    if pcm is None:
        return _signals_reference()
    return np.fft.rfft(windowed_frames(pcm).astype(np.float64), axis=-1)


@functools.lru_cache(maxsize=None)
def _signals_reference():
    X = analysis_reference(signals())
    X.setflags(write=False)
    return X


def frame_scales(X):
    """scale_f = max_k |X_f,k| -> [S, n]"""
    return np.abs(X).max(axis=-1)


def unit_phasors(X):
    """X / |X|, (1, 0) where X is 0 -> complex [S, n, 257]"""
    a = np.abs(X)
    return np.where(a > 0, X / np.where(a > 0, a, 1.0), 1.0 + 0.0j)


@functools.lru_cache(maxsize=None)
def estimates():
    """[8, N_HOPS, 256] float32, read-only: 'model outputs' whose level jumps from frame to frame -- |N(0,1)| x a per-frame level drawn
    from LEVELS; every fourth frame has est[0] (bin 1, the one dc_mode edge copies to bin 0) and est[255] (bin 256) at 5 x the frame's
    level; frames 3 + 2 s and 4 + 2 s of stream s are all zero (stream 0: across a run seam of the block kernels, stream 6: across a tile
    seam), so every stream has an output hop that is exactly zero."""
    rng = np.random.default_rng(SEED + 1)
    S = len(NAMES)
    level = LEVELS[rng.integers(0, len(LEVELS), size=(S, N_HOPS))]
    for s in range(S):
        level[s, 3 + 2 * s:5 + 2 * s] = 0.0
    est = np.abs(rng.standard_normal((S, N_HOPS, 256))) * level[:, :, None]
    est[:, ::4, 0] = 5.0 * level[:, ::4]
    est[:, ::4, 255] = 5.0 * level[:, ::4]
    est = est.astype(np.float32)
    est.setflags(write=False)
    return est


def as_complex(phasors):
    """``[..., 257, 2]`` float32 as read back from the device (or a complex array) -> complex128 ``[..., 257]``"""
    p = np.asarray(phasors)
    if np.iscomplexobj(p):
        return p.astype(np.complex128)
    return p[..., 0].astype(np.float64) + 1j * p[..., 1].astype(np.float64)


def synthesis_blocks(est, phasors, dc_mode, keep=None):
    """The inverse-windowed synthesis blocks in double, ``[S, n, 512]``: bins 1..256 = est x phasor, bin 0 = est[0] x Re phasor[0] (edge) or
    0 (zero), the imaginary parts of bins 0 and 256 dropped, ``np.fft.irfft``, x the float32 ``inverse_window()`` taps.  ``keep
    [S, n, 257]`` (bool): only these bins of the spectrum, the others zero."""
    if dc_mode not in ("edge", "zero"):
        raise ValueError("dc_mode must be 'edge' or 'zero'")
    est = np.asarray(est, np.float64)
    ph = as_complex(phasors)
    Y = np.zeros(est.shape[:-1] + (257,), np.complex128)
    Y[..., 1:] = est * ph[..., 1:]
    if dc_mode == "edge":
        Y[..., 0] = est[..., 0] * ph[..., 0].real
    Y[..., 256] = Y[..., 256].real
    if keep is not None:
        Y = Y * keep
    return np.fft.irfft(Y, n=SE.FRAME_LEN, axis=-1) * SE.inverse_window().astype(np.float64)


def synthesis_reference(est, phasors, dc_mode, keep=None):
    """``est [S, n, 256]``, ``phasors [S, n, 257, 2]`` (the DEVICE's own, read back: analysis error is not charged twice), from an all-zero
    overlap tail -> (``y [S, n * 256]`` float64: output hop i = first half of block i + second half of block i - 1,
    ``norm [S, n]``: sqrt(mean(block_i[:256]^2 + block_{i-1}[256:]^2)) per output hop)."""
    b = synthesis_blocks(est, phasors, dc_mode, keep)
    first, second = b[..., :HOP], np.zeros_like(b[..., HOP:])
    second[:, 1:] = b[:, :-1, HOP:]
    y = first + second
    norm = np.sqrt(np.mean(first ** 2 + second ** 2, axis=-1))
    return y.reshape(y.shape[0], -1), norm


def block_normaliser(est, phasors, dc_mode):
    """``[S, n]``: sqrt(mean(block_i^2) + mean(block_{i-1}^2)), each mean over all 512 samples of the block.  The rounding error of a
    float32 transform is spread over the whole block it transforms, whichever half the block's energy sits in; where the energy is spread
    evenly this is the normaliser of ``synthesis_reference``, where a block keeps its energy in the half that belongs to the other output
    hop (the model's answer to an impulse) it is the larger of the two, and the one an error can be held against."""
    b = synthesis_blocks(est, phasors, dc_mode)
    e = np.mean(b ** 2, axis=-1)
    prev = np.zeros_like(e)
    prev[:, 1:] = e[:, :-1]
    return np.sqrt(e + prev)


def synthesis_float32(est, phasors, dc_mode):
    """The synthesis in single precision on the CPU (scipy.fft on complex64, float32 window and overlap-add) -> ``[S, n * 256]`` float32:
    what a float32 transform that is not under test makes of the same inputs (the conditioning cap)."""
    import scipy.fft
    est = np.asarray(est, np.float32)
    rot = as_complex(phasors).astype(np.complex64)
    Y = np.zeros(est.shape[:-1] + (257,), np.complex64)
    Y[..., 1:] = est * rot[..., 1:]
    if dc_mode == "edge":
        Y[..., 0] = est[..., 0] * rot[..., 0].real
    Y[..., 256] = Y[..., 256].real
    blocks = scipy.fft.irfft(Y, n=SE.FRAME_LEN, axis=-1)
    assert blocks.dtype == np.float32
    blocks = blocks * SE.inverse_window()
    y = blocks[..., :HOP].copy()
    y[:, 1:] += blocks[:, :-1, HOP:]
    assert y.dtype == np.float32
    return y.reshape(y.shape[0], -1)


def strong_bins(X):
    """bool ``[S, n, 257]``: the bins whose phase a transform defines, |X_f,k| > STRONG x scale_f.  The others hold rounding noise alone on
    some of the signals (dc_neg, nyquist, sine: most bins of most frames), and two implementations give them unrelated phasors."""
    return np.abs(X) > STRONG * frame_scales(X)[..., None]


def strong_estimates():
    """``estimates()`` with the bins zeroed whose phasor no transform defines: |X_f,k| <= STRONG x scale_f in the float64 reference.  (On
    dc_neg, nyquist and sine most bins of most frames hold rounding noise alone; two device paths give them unrelated phasors, and a
    waveform synthesised from estimates on those bins differs by its own size whatever the kernels do.  A comparison with float64 does not
    need this: there each path is referenced on its own phasors.)"""
    return np.ascontiguousarray(estimates() * strong_bins(analysis_reference())[..., 1:])


def rel_rms(got, want):
    """Relative RMS of one stream (DEVICE_REL): RMS of the difference over the RMS of ``want``."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2)) / np.sqrt(np.mean(want ** 2)))


class Ledger:
    """Worst ratio to each bound and the first miss of each kind (stream, frame, bin), by kernel family; ``close()`` prints and fails."""

    def __init__(self, what, streams=None):
        """``streams[b]``: the index into NAMES of row b of what is compared (default: row b is stream b)"""
        self.what, self.streams, self.worst, self.misses = what, streams, {}, []

    def name(self, b):
        return NAMES[self.streams[b] if self.streams is not None else b]

    def note(self, kind, ratio, where):
        ratio = float(ratio) if np.isfinite(ratio) else float("inf")
        if ratio >= self.worst.get(kind, (-1.0, ""))[0]:
            self.worst[kind] = (ratio, where)

    def miss(self, text):
        self.misses.append(text)

    def _ratios(self, kind, ratio, fmt):
        """``ratio``: an array of ratios to a bound, every entry taking part; records the worst and the first entry that is not < 1"""
        ratio = np.where(np.isfinite(ratio), ratio, np.inf)
        idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        self.note(kind, ratio[idx], fmt(idx))
        bad = np.argwhere(~(ratio < 1.0))
        if len(bad):
            first = tuple(bad[0])
            self.miss("%s: %d miss the bound, first %s at %.3g x the bound" % (kind, len(bad), fmt(first), ratio[first]))

    def analysis(self, mag, ph, X, frame0=0):
        """``mag [S, n, 256]`` (bins 1..256) and ``ph [S, n, 257, 2]`` of a device against ``X [S, n, 257]``: MAG and PHASOR per frame, and
        the exact conditions.  Every frame takes part: one with scale_f = 0 in the exact conditions, every other in both bounds."""
        mag, ph = np.asarray(mag), np.asarray(ph)
        assert mag.shape == X.shape[:2] + (256,) and ph.shape == X.shape + (2,), (mag.shape, ph.shape, X.shape)
        if not (np.isfinite(mag).all() and np.isfinite(ph).all()):
            self.miss("analysis: not finite")
            return
        absX, scale = np.abs(X), frame_scales(X)
        live = scale > 0
        safe = np.where(live, scale, 1.0)
        at = lambda i: "stream %s frame %d" % (self.name(i[0]), frame0 + i[1])
        at_bin = lambda i: "%s bin %d" % (at(i), i[2])
        # magnitudes, bins 1..256
        err = np.abs(mag.astype(np.float64) - absX[..., 1:]).max(axis=-1)
        self._ratios("magnitudes / MAG", np.where(live, err / (MAG * safe), 0.0), at)
        # phasors of strong bins, bins 0..256
        strong = live[..., None] & (absX > STRONG * scale[..., None])
        assert strong.any(axis=-1)[live].all()          # (the maximum itself is strong: every live frame is compared)
        perr = np.abs(as_complex(ph) - unit_phasors(X))
        self._ratios("phasors / PHASOR", np.where(strong, perr / PHASOR, 0.0), lambda i: at_bin((i[0], i[1], i[2])))
        # exact: an empty frame gives magnitudes 0 and phasors (1, 0)
        dead_bad = ~live & ((mag != 0).any(axis=-1) | (ph[..., 0] != 1).any(axis=-1) | (ph[..., 1] != 0).any(axis=-1))
        for i in np.argwhere(dead_bad)[:1]:
            self.miss("exact: %s is all zero but its magnitudes are not 0 or its phasors not (1, 0)" % at(i))
        # exact: the DC phasor is (+-1, 0), with the sign of X_f,0 where bin 0 is strong
        dc = ph[..., 0, :]
        dc_bad = (np.abs(dc[..., 0]) != 1) | (dc[..., 1] != 0) | (strong[..., 0] & (dc[..., 0] != np.sign(X[..., 0].real)))
        for i in np.argwhere(dc_bad)[:1]:
            self.miss("exact: DC phasor of %s is (%r, %r), X_0 = %.6g at scale %.6g" % (at(i), float(dc[tuple(i)][0]), float(dc[tuple(i)][1]),
                                                                                      X[tuple(i)][0].real, scale[tuple(i)]))
        self.note("frames compared", float(live.sum()), "%d live, %d empty, %d with a strong bin 0" % (live.sum(), (~live).sum(), strong[..., 0].sum()))

    def synthesis(self, got, want, norm, kind="synthesis / SYNTH"):
        """``got [S, n * 256]`` of a device against ``want`` and ``norm [S, n]`` of ``synthesis_reference``: SYNTH per output hop, and hops
        whose normaliser is 0 are exactly 0."""
        got = np.asarray(got)
        assert got.shape == want.shape
        if not np.isfinite(got).all():
            self.miss("%s: not finite" % kind)
            return
        S, n = norm.shape
        g = got.reshape(S, n, HOP)
        err = np.sqrt(np.mean((g.astype(np.float64) - want.reshape(S, n, HOP)) ** 2, axis=-1))
        live = norm > 0
        at = lambda i: "stream %s output hop %d" % (self.name(i[0]), i[1])
        self._ratios(kind, np.where(live, err / (SYNTH * np.where(live, norm, 1.0)), 0.0), at)
        for i in np.argwhere(~live & (g != 0).any(axis=-1))[:1]:
            self.miss("exact: %s has normaliser 0 but is not all zero" % at(i))
        self.note("output hops compared", float(live.sum()), "%d live, %d exactly zero" % (live.sum(), (~live).sum()))

    def device(self, label, got, want):
        """two device paths, ``[S, ...]``: relative RMS per stream (each stream by its own RMS) against DEVICE_REL"""
        got, want = np.asarray(got), np.asarray(want)
        if not np.isfinite(got).all():
            self.miss("%s: not finite" % label)
            return
        r = np.array([rel_rms(got[b], want[b]) for b in range(got.shape[0])])
        self._ratios("%s / DEVICE_REL" % label, r / DEVICE_REL, lambda i: "stream %s" % self.name(i[0]))

    def report(self):
        """{kind: worst ratio}; printed one line per kind"""
        for kind, (ratio, where) in self.worst.items():
            print("%s: %s: worst %.4g (%s)" % (self.what, kind, ratio, where))
        return {kind: ratio for kind, (ratio, _) in self.worst.items()}

    def close(self):
        res = self.report()
        if self.misses:
            raise AssertionError("%s: %s" % (self.what, "; ".join(self.misses)))
        return res
