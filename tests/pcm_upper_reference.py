"""float64 restatement of the PCM gateway's upper band (include/nutls.h, "Upper band"), for the tests: ``scipy.signal.upfirdn`` with the taps of
``runner.pcm_filter``.  Per stream, with D the decode half, E the encode half, q = rate / 16000, S = 256 q, K = 24:

    u[n]   = x[n - 2 K q] - E(D(x))[n]
    out[n] = E(y)[n] + g * u[n - hop_lag * S]

``y`` is what the encode half is handed (the model's output in the ``_pcm`` entries); the library adds the upper band of the hop in front
(``hop_lag = 1``, the model's one-hop lag); ``hop_lag = 0`` is the same sum without that wait.  Samples before the first are zeros.

The bound: the header documents the operation order -- d: 2 K q + 1 FMAs; c over d: at most 2 K + 1 FMAs; u = fma(-q, c, x): one; z = the
encode sum over y (at most 2 K + 1 FMAs) and its product by q; out = fma(g, u, z): one.  The longest path of an output sample (d, c, u, out)
has ``N = 2 K q + 2 K + 4`` roundings of relative size 2**-24, each on a partial result that never exceeds the sum of absolute products

    A[n] = q sum |p| |y|  +  g ( |x[n - 2 K q - lag S]| + q sum |p| (sum |p| |x|) [n - lag S] )

so the error is at most ``N 2**-24 A`` to first order; ``(N + 3) 2**-24 A`` leaves room for the second-order terms (about N 2**-24 of the first)."""
import numpy as np
from scipy import signal

K = 24
U2 = 2.0 ** -24


def ratio(rate):
    assert rate in (32000, 48000), "the upper band exists above 16 kHz only"
    return rate // 16000


def taps_of(rate):
    from nunet_amd import runner
    return runner.pcm_filter(rate).astype(np.float64)


def roundings(rate):
    """N of the header: fp32 roundings on the longest path of an output sample."""
    return 2 * K * ratio(rate) + 2 * K + 4


def decode64(p, x, q):
    """D: rate reduction by q of the rows of x [rows, n] -> [rows, n // q]."""
    return np.stack([signal.upfirdn(p, r, 1, q)[:x.shape[1] // q] for r in np.asarray(x, np.float64)])


def encode64(p, y, q):
    """E: rate increase by q of the rows of y [rows, m] -> [rows, m * q]."""
    return np.stack([signal.upfirdn(q * p, r, q, 1)[:y.shape[1] * q] for r in np.asarray(y, np.float64)])


def delayed(a, d):
    """a[n - d] along the last axis, zeros in front."""
    if d == 0:
        return a.copy()
    out = np.zeros_like(a)
    out[..., d:] = a[..., :-d]
    return out


def upper_band(x, rate, p=None, with_mag=False):
    """u [rows, n] in float64 for the rows of x [rows, n] at ``rate`` (n a multiple of q); with_mag: also |x[n - 2 K q]| + q sum|p| sum|p||x|."""
    q = ratio(rate)
    p = taps_of(rate) if p is None else np.asarray(p, np.float64)
    x = np.asarray(x, np.float64)
    u = delayed(x, 2 * K * q) - encode64(p, decode64(p, x, q), q)
    if not with_mag:
        return u
    mag = delayed(np.abs(x), 2 * K * q) + encode64(np.abs(p), decode64(np.abs(p), np.abs(x), q), q)
    return u, mag


def encode_with_upper(y, x, rate, g, hop_lag=1, p=None):
    """(out, bound): out = E(y) + g * u delayed by hop_lag hops, in float64, and the per-sample bound of the fp32 result (module docstring).
    y: [rows, hops * 256] at 16 kHz; x: [rows, hops * S] at ``rate``."""
    q = ratio(rate)
    p = taps_of(rate) if p is None else np.asarray(p, np.float64)
    y = np.asarray(y, np.float64)
    assert y.shape[1] * q == np.shape(x)[1]
    u, umag = upper_band(x, rate, p, with_mag=True)
    lag = hop_lag * 256 * q
    out = encode64(p, y, q) + g * delayed(u, lag)
    mag = encode64(np.abs(p), np.abs(y), q) + abs(g) * delayed(umag, lag)
    return out, (roundings(rate) + 3) * U2 * mag
