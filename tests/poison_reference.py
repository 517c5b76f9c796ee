"""Non-finite input on a live row (include/nutls.h, "Non-finite input") -- a plain helper module with no GPU in it: the poisons, the clean
twin of a poisoned input and the support windows of the stateless halves.  tests/test_poison_reference.py holds every window against the
float64 references (``scipy.signal.upfirdn`` with the taps of ``nutls_pcm_filter``, tests/transform_signals.py,
tests/pcm_upper_reference.py, tests/pcm_follow_reference.py); tests/test_gpu_poison.py then holds the kernels to the same windows.

The contract in one line: whatever a live row is fed, every OTHER row is bit-identical to the run in which that row was fed zeros, and
``nutls_reset`` of the row makes it bit-identical to the same row of a fresh handle.

The windows, all from the header's formulas (nothing here was read off a kernel's output).  With T = ``nutls_pcm_filter_taps(rate)``,
L = T - 1 = 2 K q, q = max(rate, 16000) / min(rate, 16000), S = 256 rate / 16000, W = ``NUTLS_PCM_FOLLOW_HOPS``:

  rate reduction by q      input sample n          -> output samples ceil(n / q) .. floor((n + L) / q)
  rate increase by q       input sample m          -> output samples q m .. q m + L
  analysis (512 / 256)     input sample n          -> magnitude frames floor(n / 256) and floor(n / 256) + 1
  synthesis                frame f (bin or phasor) -> output samples 256 f .. 256 (f + 2) - 1
  upper band               caller's sample n       -> u[q ceil(n / q) .. q floor(n / q) + 2 L], added one hop (S samples) later
  follow                   a non-finite energy a_s -> the whole hops s + 1 .. s + W + 1;  b_s -> the whole hops s .. s + W

A rate above 16 kHz is reduced on the way in (decode) and increased on the way out (encode); 8 kHz the other way round.  Every window is
closed (both ends included) and is returned as a sorted int64 array of output indices; indices beyond the end of a run are the caller's to
cut (``clip``)."""
import numpy as np

HOP = 256
FRAME = 512
FOLLOW_HOPS = 4          # NUTLS_PCM_FOLLOW_HOPS
BIG = np.float32(3.0e38)
KINDS = ("nan", "inf", "big")
EDGES = ("first", "last")


# ---- the poisons ---------------------------------------------------------------------------------------------------------------------------
def poison(row, kind, edge="first"):
    """A poisoned copy of ``row`` (one float32 vector: a magnitude row of 256 bins, a hop or a packet of samples):
      "nan"  NaN over the whole row;
      "inf"  +Inf in ONE edge element -- ``edge`` "first" (bin 0, the first sample) or "last" (bin 255, the last sample) --, the others as
             they were, finite: the frequency halos and the hop seams sit at the edges;
      "big"  3.0e38 over the whole row: finite on the way in, overflows inside."""
    out = np.array(row, dtype=np.float32)
    if not np.isfinite(out).all():
        raise ValueError("the row to poison must be finite")
    if kind == "nan":
        out[...] = np.nan
    elif kind == "inf":
        if edge not in EDGES:
            raise ValueError("edge must be one of %s" % (EDGES,))
        out[..., 0 if edge == "first" else -1] = np.inf
    elif kind == "big":
        out[...] = BIG
    else:
        raise ValueError("kind must be one of %s" % (KINDS,))
    return out


def poisoned(x, row, frames, kind):
    """``x [frames, rows, n]`` with row ``row`` poisoned at the frames ``frames``: the first of them through the "first" edge, the second
    through the "last" one, and so on in turn (the whole-row poisons have no edge)."""
    out = np.array(x, dtype=np.float32)
    for i, f in enumerate(frames):
        out[f, row] = poison(out[f, row], kind, EDGES[i % 2])
    return out


def clean_twin(x, row, frames):
    """The expectation of every other row: the same input with the poisoned part -- row ``row`` at the frames ``frames`` -- fed zeros."""
    out = np.array(x, dtype=np.float32)
    for f in frames:
        out[f, row] = 0.0
    return out


# ---- support windows -----------------------------------------------------------------------------------------------------------------------
def ratio(rate):
    if rate not in (8000, 16000, 32000, 48000):
        raise ValueError("rate must be 8000, 16000, 32000 or 48000")
    return max(rate, 16000) // min(rate, 16000)


def hop_samples(rate):
    return HOP * rate // 16000


def filter_span(rate, taps):
    """L = taps - 1 = 2 K q, from ``nutls_pcm_filter_taps(rate)``; 0 at 16000 (the single tap 1.0)."""
    q = ratio(rate)
    if taps < 1 or (taps - 1) % (2 * q) or (rate == 16000) != (taps == 1):
        raise ValueError("%d taps are not 2 K q + 1 at %d Hz" % (taps, rate))
    return taps - 1


def _span(lo, hi):
    return np.arange(lo, hi + 1, dtype=np.int64)


def reduce_support(n, q, span):
    """y[m] = sum_j p[j] x[q m - j], j = 0 .. span: x[n] is under tap j = q m - n."""
    return _span(-(-n // q), (n + span) // q)


def increase_support(m, q, span):
    """zero-stuff by q, then filter: x[m] sits at q m and is under tap j = k - q m."""
    return _span(q * m, q * m + span)


def _over(indices, fn):
    return np.unique(np.concatenate([fn(int(i)) for i in indices]))


def decode_support(n, rate, taps):
    """Caller's sample n -> the 16 kHz samples of the decode half (``nutls_pcm_decode_hop`` / ``_block``) that may differ."""
    q, span = ratio(rate), filter_span(rate, taps)
    if rate == 16000:
        return _span(n, n)
    return reduce_support(n, q, span) if rate > 16000 else increase_support(n, q, span)


def encode_support(m, rate, taps):
    """16 kHz sample m -> the caller's samples of the encode half (``nutls_pcm_encode_hop`` / ``_block``) that may differ."""
    q, span = ratio(rate), filter_span(rate, taps)
    if rate == 16000:
        return _span(m, m)
    return increase_support(m, q, span) if rate > 16000 else reduce_support(m, q, span)


def roundtrip_support(n, rate, taps):
    """Caller's sample n through decode and encode (the model the identity, no lag): n' .. n'' + 2 ``nutls_pcm_delay_samples`` with n', n''
    = n rounded up, down to a multiple of q above 16 kHz, n itself at 8 kHz."""
    return _over(decode_support(n, rate, taps), lambda m: encode_support(m, rate, taps))


def stft_support(n):
    """Input sample n -> the magnitude frames (and phasor rows) that may differ: frame f is hops f - 1 and f."""
    return _span(n // HOP, n // HOP + 1)


def istft_support(f):
    """Frame f of the magnitudes (or of the phasors) -> output samples: output hop f is the first half of block f plus the second half of
    block f - 1, so block f reaches hops f and f + 1."""
    return _span(HOP * f, HOP * (f + 2) - 1)


def stft_istft_support(n):
    """Input sample n through analysis and synthesis (the model the identity): the three output hops floor(n / 256) .. + 2."""
    return _over(stft_support(n), istft_support)


def upper_support(n, rate, taps, hop_lag=1):
    """Caller's sample n (32 / 48 kHz) -> the samples of the encode half's output that the upper band u[. - hop_lag S] may change:
    u[k] = x[k - L] - E(D(x))[k], so u differs where the round trip does (k = n + L lies inside that window), ``hop_lag`` hops later."""
    if rate not in (32000, 48000):
        raise ValueError("the upper band exists above 16 kHz only")
    w = roundtrip_support(n, rate, taps)
    assert w[0] <= n + filter_span(rate, taps) <= w[-1]
    return w + hop_lag * hop_samples(rate)


def follow_support_a(s, rate):
    """A non-finite decode energy a_s: A_t sums a_{t-1} .. a_{t-W}, and gamma_t is a ramp from g_{t-1} to g_t, so the hops t = s + 1 ..
    s + W + 1 of the encode half's output may differ, whole."""
    S = hop_samples(rate)
    return _span(S * (s + 1), S * (s + FOLLOW_HOPS + 2) - 1)


def follow_support_b(s, rate):
    """A non-finite encode energy b_s: B_t sums b_t .. b_{t-W+1}; with the ramp the hops t = s .. s + W may differ, whole."""
    S = hop_samples(rate)
    return _span(S * s, S * (s + FOLLOW_HOPS + 1) - 1)


def hops_of(indices):
    """The 16 kHz hops that hold the samples ``indices``."""
    return np.unique(np.asarray(indices) // HOP)


def upper_chain_support(n, rate, taps, follow):
    """Caller's sample n through ``decode`` and ``encode(decode(x))`` with the upper band on (and follow): the union of the round trip, the
    upper band one hop later and, with follow, the whole hops that the energies of the decoded hops it reaches touch (a of the decode
    half, b of what the encode half is handed -- here the same hops)."""
    parts = [roundtrip_support(n, rate, taps), upper_support(n, rate, taps)]
    if follow:
        for s in hops_of(decode_support(n, rate, taps)):
            parts += [follow_support_a(int(s), rate), follow_support_b(int(s), rate)]
    return np.unique(np.concatenate(parts))


def clip(indices, length):
    indices = np.asarray(indices)
    return indices[(indices >= 0) & (indices < length)]


def changed(a, b):
    """The flat indices along the last axis at which two arrays differ in any bit (NaN against NaN of the same bits is no difference)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype.kind == "c":
        a, b = a.view(a.real.dtype).reshape(a.shape + (2,)), b.view(b.real.dtype).reshape(b.shape + (2,))
        diff = (a.view("u%d" % a.itemsize) != b.view("u%d" % b.itemsize)).any(axis=-1)
    else:
        diff = a.view("u%d" % a.itemsize) != b.view("u%d" % b.itemsize)
    return np.flatnonzero(diff.reshape(-1, diff.shape[-1]).any(axis=0)) if diff.ndim > 1 else np.flatnonzero(diff)
