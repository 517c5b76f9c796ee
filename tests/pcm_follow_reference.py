"""float64 restatement of the PCM gateway's following upper-band gain (include/nutls.h, "Upper band", follow), for the tests, on top of
``pcm_upper_reference``.  Per row, t counting the row's real hops, d_t the 256 decoded 16 kHz samples of hop t, y_t the 256 samples the
encode half is handed for hop t (energies of hops before the first are 0), W = 4:

    a_t = sum d_t^2                      b_t = sum y_t^2
    A_t = a_{t-1} + ... + a_{t-4}        B_t = b_t + ... + b_{t-3}
    g_t = gain * min(sqrt(B_t / max(A_t, 2^-100)), 1)
    gamma_t[n] = g_{t-1} + (g_t - g_{t-1}) * w[n],   w[n] = float32(n + 1) * float32(1 / S) (the library's table, rounded as it rounds it)
    out[n]     = E(y)[n] + gamma_t[n] * u[n - S]

``follow`` takes the fp32 ``d`` and ``y`` the library saw and returns everything in float64 with a per-sample bound of the fp32 result.

The bounds, with e = 2^-24 the relative size of one fp32 rounding, to first order:
  - a_t: every square is rounded once and passes through the 8 levels of the pairwise tree, 9 roundings; all terms are non-negative, so no
    cancellation: the relative error of a_t is at most 9 e.  The window adds 4 of them with 3 more additions: A_t and B_t carry 12
    roundings each, relative error at most 12 e (the max with 2^-100 is exact).
  - g_t: the quotient (12 + 12 + 1) e = 25 e; the square root halves that and rounds once, 13.5 e; the minimum with 1 is exact and only
    lowers an error; the product by the gain rounds once: 14.5 e, "15 e".  ``G_ROUNDINGS = 20``: |g32 - g| <= 20 e g leaves a third of
    room for the second-order terms and for a ratio within 25 e of the clamp (where fp32 and float64 may sit on different sides of it:
    the difference is then still at most the 13.5 e of the unclamped value).
  - gamma_t[n] = (1 - w) g_{t-1} + w g_t: the two gains contribute at most 15 e max(g_{t-1}, g_t) <= 15 e gain; delta = g_t - g_{t-1} rounds
    once (e |delta|), w[n] is two roundings off (n + 1) / S -- but this restatement uses the library's rounded table, so that is no error
    here --, and the FMA rounds once (e gamma).  With |delta| <= gain and gamma <= gain: 15 + 1 + 1 = 17 e gain against this restatement,
    19 e gain against the exact ramp.  ``GAMMA_ROUNDINGS = 24``: |gamma32 - gamma| <= 24 e gain.
  - out[n]: the fp32 result is fma(gamma32, u32, z32).  Replace gamma32 by gamma: what remains is ``encode_with_upper``'s sum with a gain
    gamma <= ``gain``, whose bound grows with the gain, so that function's bound AT ``gain`` covers it; the replacement itself moves the
    result by at most |gamma32 - gamma| |u32| <= 24 e gain umag[n - S], umag the sum of absolute products behind u (>= |u32| to first
    order).  bound = encode_with_upper(..., gain)'s + 24 e gain umag[n - S]."""
import numpy as np

import pcm_upper_reference as R

W = 4                       # NUTLS_PCM_FOLLOW_HOPS
A_FLOOR = 2.0 ** -100
G_ROUNDINGS = 20
GAMMA_ROUNDINGS = 24
U2 = R.U2


def hop_len(rate):
    return 256 * rate // 16000


def energies(v):
    """[rows, hops * 256] -> [rows, hops] float64 sums of squares."""
    v = np.asarray(v, np.float64)
    return (v.reshape(v.shape[0], -1, 256) ** 2).sum(axis=2)


def ramp(S):
    """w[n] as the library rounds it: float32(n + 1) * float32(1 / S), in float64.  w[S - 1] == 1.0 for S = 512 and 768."""
    w = (np.arange(1, S + 1, dtype=np.float32) * np.float32(1.0 / S)).astype(np.float32)
    return w.astype(np.float64)


def windows(d, y):
    """(A, B, r) [rows, hops + 1]: column t + 1 belongs to hop t, column 0 to the hop in front of the first (all energies 0)."""
    a, b = energies(d), energies(y)
    rows, hops = a.shape
    assert b.shape == a.shape
    ap = np.concatenate([np.zeros((rows, W + 1)), a], axis=1)      # ap[:, W + 1 + t] = a_t
    bp = np.concatenate([np.zeros((rows, W)), b], axis=1)          # bp[:, W + t] = b_t
    A = np.zeros((rows, hops + 1))
    B = np.zeros((rows, hops + 1))
    for t in range(-1, hops):
        A[:, t + 1] = ap[:, t + 1:t + 1 + W].sum(axis=1)           # a_{t-4} .. a_{t-1}
        B[:, t + 1] = bp[:, t + 1:t + 1 + W].sum(axis=1)           # b_{t-3} .. b_t
    return A, B, np.sqrt(B / np.maximum(A, A_FLOOR))


def gains(d, y, gain):
    """g [rows, hops + 1] in float64, column t + 1 = g_t, column 0 = g_{-1} = 0."""
    _, _, r = windows(d, y)
    return gain * np.minimum(r, 1.0)


def follow(d, y, x, rate, gain, p=None):
    """(g [rows, hops], gamma [rows, hops * S], out [rows, hops * S], bound [rows, hops * S]) in float64.  d, y: [rows, hops * 256] fp32 as the
    library saw them; x: [rows, hops * S] the callers' samples as float (int16 / 32768)."""
    S = hop_len(rate)
    g = gains(d, y, gain)
    w = ramp(S)
    gamma = (g[:, :-1, None] + (g[:, 1:, None] - g[:, :-1, None]) * w[None, None, :]).reshape(g.shape[0], -1)
    fixed, bound = R.encode_with_upper(y, x, rate, gain, p=p)      # (its bound: the fixed gain `gain`, the ceiling)
    u, umag = R.upper_band(x, rate, p, with_mag=True)
    out = R.encode64(R.taps_of(rate) if p is None else np.asarray(p, np.float64), y, R.ratio(rate)) + gamma * R.delayed(u, S)
    return g[:, 1:], gamma, out, bound + GAMMA_ROUNDINGS * U2 * gain * R.delayed(umag, S)


# ---- the designed inputs of the tests -----------------------------------------------------------------------------------------------------
ROWS, HOPS = 3, 9
# the model's "suppression" per hop: r = sqrt(B / A) starts above 1 (the clamp), crosses 1 between hops 4 and 5 and ends at about 0.05
ENVELOPE = np.array([2.0, 1.6, 1.2, 0.5, 0.05, 0.05, 0.05, 0.05, 0.05])


def designed_x(rate, rows=ROWS, hops=HOPS, seed=300):
    """[rows, hops * S] float32: a tone at 0.3 of 8 kHz, one at 1.4 of 8 kHz and seeded noise, at half scale."""
    rng = np.random.default_rng(seed + rate // 16000)
    t = np.arange(hops * hop_len(rate), dtype=np.float64)
    x = 0.35 * np.sin(2 * np.pi * 0.3 * 8000.0 / rate * t[None, :] + rng.uniform(0, 6.28, (rows, 1)))
    x = x + 0.3 * np.sin(2 * np.pi * 1.4 * 8000.0 / rate * t[None, :] + rng.uniform(0, 6.28, (rows, 1)))
    x = x + 0.1 * rng.standard_normal((rows, t.size))
    return (0.5 * x).astype(np.float32)


def designed_y_hop(d_before, t, seed=310):
    """y_t [rows, 256] float32 from d_{t-1} (None: zeros, the hop in front of the first): the envelope times the decoded hop in front plus a
    little noise of its own, so that y is no exact multiple of d."""
    rows = ROWS if d_before is None else d_before.shape[0]
    noise = np.random.default_rng(seed + t).standard_normal((rows, 256))
    base = np.zeros((rows, 256)) if d_before is None else np.asarray(d_before, np.float64)
    return (ENVELOPE[t] * (base + 0.01 * noise)).astype(np.float32)


def designed_y(d, seed=310):
    """[rows, hops * 256] float32: designed_y_hop over the hops of d [rows, hops * 256]."""
    hops = d.shape[1] // 256
    return np.concatenate([designed_y_hop(None if t == 0 else d[:, (t - 1) * 256:t * 256], t, seed) for t in range(hops)], axis=1)
