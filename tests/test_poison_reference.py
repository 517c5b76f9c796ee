"""The support windows of tests/poison_reference.py (include/nutls.h, "Non-finite input", point 3) against brute force on the float64
references -- no GPU: ``scipy.signal.upfirdn`` with the taps of ``nutls_pcm_filter`` (as tests/test_gpu_pcm_format.py uses it), the float64
transforms of tests/transform_signals.py, tests/pcm_upper_reference.py and tests/pcm_follow_reference.py.  One input sample is perturbed --
by a finite amount and by NaN --, the outputs that change are recorded, and

  - the changed set is a subset of the calculator's window, and
  - both ends of every window are attained (the windows are not wider than the operation).

Every second tap of the prototypes is exactly 0, the two end taps among them (a sinc at its zero crossings), so a finite perturbation never
reaches the ends of a rate increase's window; NaN does -- 0 x NaN is NaN, which is the point of the whole exercise.  ``upfirdn`` cannot
take NaN for this (it pads the taps of a rate increase with zeros to a multiple of q and multiplies them too: one sample that no tap
reaches), so the NaN runs go through the header's two sums written out (``reduce64``, ``increase64``), which equal ``upfirdn`` on finite
data.

tests/test_gpu_poison.py holds the kernels to these windows; here they are shown to be right from the references alone.  Last, oracle B
(``oracle.nutls_ref.NutlsRef``) at batch 4 has the containment and the healing property -- trivially, but it pins that the clean twin is
the right expectation."""
import numpy as np
import pytest
import torch

import pcm_follow_reference as F
import pcm_upper_reference as R
import poison_reference as P
import transform_signals as TS
from nunet_amd import runner
from nunet_amd import topology as T
from oracle.nutls_ref import NutlsRef

HOPS = 8
RATES = (8000, 32000, 48000)
DELTA = 1.0e30          # finite, and large enough for a tap of 1e-19 (the prototype's end taps, a sinc at its zero crossing) to show


def taps(rate):
    return runner.pcm_filter(rate).astype(np.float64)


def positions(rate, unit=None):
    """The first and the last sample of hop 3, and the samples next to them (every residue modulo q = 2, 3)."""
    S = P.hop_samples(rate) if unit is None else unit
    return (3 * S, 3 * S + 1, 4 * S - 2, 4 * S - 1)


def decode64(x, rate):
    p, q = taps(rate), P.ratio(rate)
    return R.decode64(p, x, q) if rate > 16000 else R.encode64(p, x, q)


def encode64(y, rate):
    p, q = taps(rate), P.ratio(rate)
    return R.encode64(p, y, q) if rate > 16000 else R.decode64(p, y, q)


def reduce64(p, x, q):
    """y[m] = sum_j p[j] x[q m - j], samples before the first are zeros: the header's sum, every tap multiplied."""
    x = np.asarray(x, np.float64)
    span, m = len(p) - 1, x.shape[-1] // q
    xp = np.concatenate([np.zeros(x.shape[:-1] + (span,)), x], axis=-1)
    y = np.zeros(x.shape[:-1] + (m,))
    for j in range(span + 1):
        y += p[j] * xp[..., span - j + q * np.arange(m)]
    return y


def increase64(p, x, q):
    """zero-stuff by q, then filter with q p."""
    x = np.asarray(x, np.float64)
    xs = np.zeros(x.shape[:-1] + (x.shape[-1] * q,))
    xs[..., ::q] = x
    return reduce64(q * p, xs, 1)


def decode_sum(x, rate):
    p, q = taps(rate), P.ratio(rate)
    return reduce64(p, x, q) if rate > 16000 else increase64(p, x, q)


def encode_sum(y, rate):
    p, q = taps(rate), P.ratio(rate)
    return increase64(p, y, q) if rate > 16000 else reduce64(p, y, q)


def upper_sum(x, rate):
    """u[n] = x[n - L] - E(D(x))[n] with the plain sums."""
    return R.delayed(np.asarray(x, np.float64), len(taps(rate)) - 1) - encode_sum(decode_sum(x, rate), rate)


def perturbed(x, n, value):
    out = np.array(x, dtype=np.float64)
    out[..., n] = value if np.isnan(value) else out[..., n] + value
    return out


class Ends:
    """Which ends of a calculator's windows were attained, over everything a test tried."""

    def __init__(self, what):
        self.what, self.lo, self.hi = what, False, False

    def check(self, got, window, length, where):
        window = P.clip(window, length)
        assert len(got), "%s, %s: nothing changed" % (self.what, where)
        assert np.isin(got, window).all(), "%s, %s: outputs %s changed outside the window %d .. %d" % (
            self.what, where, got[~np.isin(got, window)][:8], window[0], window[-1])
        self.lo |= bool(got[0] == window[0])
        self.hi |= bool(got[-1] == window[-1])

    def close(self):
        assert self.lo and self.hi, "%s: the window is wider than the operation (low end attained: %s, high end: %s)" % (self.what, self.lo, self.hi)


# ---- the poisons -----------------------------------------------------------------------------------------------------------------------
def test_the_three_poisons_and_the_clean_twin():
    row = np.linspace(0.1, 1.0, 256, dtype=np.float32)
    nan, big = P.poison(row, "nan"), P.poison(row, "big")
    assert np.isnan(nan).all() and np.all(big == np.float32(3.0e38)) and np.isfinite(big).all()
    with np.errstate(over="ignore"):
        assert not np.isfinite(big * np.float32(2.0)).any()          # finite on the way in, overflows inside
    for edge, at in (("first", 0), ("last", 255)):
        inf = P.poison(row, "inf", edge)
        assert inf[at] == np.inf and np.array_equal(np.delete(inf, at), np.delete(row, at))
    with pytest.raises(ValueError):
        P.poison(nan, "nan")
    x = np.random.default_rng(1).random((10, 4, 256), dtype=np.float32)
    for kind in P.KINDS:
        xp = P.poisoned(x, 2, (3, 4), kind)
        keep = np.ones(x.shape, bool)
        keep[3:5, 2] = False
        assert np.array_equal(xp[keep], x[keep]) and not np.array_equal(xp[3, 2], x[3, 2]) and not np.array_equal(xp[4, 2], x[4, 2])
        if kind == "inf":
            assert xp[3, 2, 0] == np.inf and xp[4, 2, 255] == np.inf and np.isfinite(xp[3, 2, 1:]).all() and np.isfinite(xp[4, 2, :255]).all()
        twin = P.clean_twin(xp, 2, (3, 4))
        assert np.array_equal(twin[keep], x[keep]) and not twin[3:5, 2].any() and np.isfinite(twin).all()


# ---- the resamplers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", ["decode", "encode", "roundtrip"])
def test_resampler_windows_hold_for_upfirdn(half):
    ends = Ends(half)
    for rate in RATES:
        n_taps, S = len(taps(rate)), P.hop_samples(rate)
        assert n_taps == 2 * R.K * P.ratio(rate) + 1
        unit = 256 if half == "encode" else S
        x = np.random.default_rng(rate).standard_normal((1, HOPS * unit))
        run = {"decode": lambda v: decode64(v, rate), "encode": lambda v: encode64(v, rate),
               "roundtrip": lambda v: encode64(decode64(v, rate), rate)}[half]
        plain = {"decode": lambda v: decode_sum(v, rate), "encode": lambda v: encode_sum(v, rate),
                 "roundtrip": lambda v: encode_sum(decode_sum(v, rate), rate)}[half]
        support = {"decode": P.decode_support, "encode": P.encode_support, "roundtrip": P.roundtrip_support}[half]
        base, base_sum = run(x), plain(x)
        assert base.shape[1] == HOPS * (S if half != "decode" else 256)
        assert base_sum.shape == base.shape and np.abs(base_sum - base).max() < 1e-12          # the plain sums are upfirdn
        for n in positions(rate, unit):
            window = P.clip(support(n, rate, n_taps), base.shape[1])
            got = P.changed(base, run(perturbed(x, n, DELTA)))
            assert len(got) and np.isin(got, window).all(), (rate, n, got[~np.isin(got, window)][:8])
            ends.check(P.changed(base_sum, plain(perturbed(x, n, np.nan))), window, base.shape[1], "%d Hz sample %d = NaN" % (rate, n))
    ends.close()


def test_the_round_trip_window_is_twice_the_documented_delay():
    """``nutls_pcm_delay_samples`` = 2 K max(1, rate / 16000): the round trip of sample n ends 2 x that behind n (rounded to q)."""
    for rate in RATES:
        q, n_taps = P.ratio(rate), len(taps(rate))
        delay = 2 * R.K * max(1, rate // 16000)
        for n in positions(rate):
            w = P.roundtrip_support(n, rate, n_taps)
            lo, hi = (-(-n // q) * q, n // q * q) if rate > 16000 else (n, n)
            assert (w[0], w[-1]) == (lo, hi + 2 * delay) and len(w) == w[-1] - w[0] + 1
    assert P.decode_support(77, 16000, 1).tolist() == [77] and P.encode_support(77, 16000, 1).tolist() == [77]
    with pytest.raises(ValueError):
        P.filter_span(48000, 100)


# ---- the transforms --------------------------------------------------------------------------------------------------------------------
def _identity_synthesis(pcm):
    X = TS.analysis_reference(pcm)
    return TS.synthesis_reference(np.abs(X)[..., 1:], TS.unit_phasors(X), "edge")[0]


def test_transform_windows_hold_for_the_float64_transforms():
    pcm = (0.1 * np.random.default_rng(5).standard_normal((1, HOPS * 256))).astype(np.float32)
    X = TS.analysis_reference(pcm)
    y = _identity_synthesis(pcm)
    a_ends, c_ends = Ends("analysis"), Ends("analysis and synthesis")
    for n in positions(16000):
        for value in (np.float32(0.5), np.float32(np.nan)):
            bad = pcm.copy()
            bad[0, n] = value if np.isnan(value) else bad[0, n] + value
            Xb = TS.analysis_reference(bad)
            frames = np.flatnonzero([not np.array_equal(X[0, f], Xb[0, f], equal_nan=True) for f in range(HOPS)])
            a_ends.check(frames, P.stft_support(n), HOPS, "sample %d" % n)
            if not np.isnan(value):          # (NaN phasors: unit_phasors of the reference maps them to (1, 0); the finite run covers the chain)
                got = P.changed(y, _identity_synthesis(bad))
                assert np.isin(got, P.stft_istft_support(n)).all()
                c_ends.check(np.unique(got // 256), np.unique(P.stft_istft_support(n) // 256), HOPS, "sample %d" % n)
    a_ends.close()
    c_ends.close()
    # synthesis alone: one bin of one frame of the estimate, at the two edge bins, and one phasor
    est, ph = np.abs(X)[..., 1:].copy(), TS.unit_phasors(X)
    base = TS.synthesis_reference(est, ph, "edge")[0]
    s_ends = Ends("synthesis")
    for f in (0, 3, HOPS - 1):
        for b in (0, 255):
            for value in (1.0, np.nan):
                e2 = est.copy()
                e2[0, f, b] = value if np.isnan(value) else e2[0, f, b] + value
                got = P.changed(base, TS.synthesis_reference(e2, ph, "edge")[0])
                s_ends.check(np.unique(got // 256), np.unique(P.istft_support(f) // 256), HOPS, "frame %d bin %d" % (f, b + 1))
                assert np.isin(got, P.istft_support(f)).all()
        p2 = ph.copy()
        p2[0, f, 7] = np.nan
        assert np.isin(P.changed(base, TS.synthesis_reference(est, p2, "edge")[0]), P.istft_support(f)).all()
    s_ends.close()


# ---- the upper band and follow ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [32000, 48000])
def test_upper_band_windows_hold_for_the_float64_restatement(rate):
    n_taps, S, q = len(taps(rate)), P.hop_samples(rate), P.ratio(rate)
    x = F.designed_x(rate, rows=1, hops=HOPS).astype(np.float64)
    y = 0.2 * np.random.default_rng(9).standard_normal((1, HOPS * 256))
    u_ends, o_ends, c_ends = Ends("u"), Ends("encode with the upper band"), Ends("decode, encode with the upper band")
    for n in positions(rate):
        bad, where = perturbed(x, n, DELTA), "%d Hz sample %d" % (rate, n)
        inside = lambda got, window: len(got) and np.isin(got, P.clip(window, x.shape[1])).all()
        assert inside(P.changed(R.upper_band(x, rate), R.upper_band(bad, rate)), P.upper_support(n, rate, n_taps, hop_lag=0)), where
        assert inside(P.changed(R.encode_with_upper(y, x, rate, 1.0)[0], R.encode_with_upper(y, bad, rate, 1.0)[0]), P.upper_support(n, rate, n_taps)), where
        chain = lambda v: R.encode_with_upper(R.decode64(taps(rate), v, q), v, rate, 1.0)[0]
        assert inside(P.changed(chain(x), chain(bad)), P.upper_chain_support(n, rate, n_taps, follow=False)), where
        # NaN through the plain sums: the ends
        nan = perturbed(x, n, np.nan)
        u_ends.check(P.changed(upper_sum(x, rate), upper_sum(nan, rate)), P.upper_support(n, rate, n_taps, hop_lag=0), x.shape[1], where)
        out = lambda v: encode_sum(y, rate) + R.delayed(upper_sum(v, rate), S)
        o_ends.check(P.changed(out(x), out(nan)), P.upper_support(n, rate, n_taps), x.shape[1], where)
        both = lambda v: encode_sum(decode_sum(v, rate), rate) + R.delayed(upper_sum(v, rate), S)
        c_ends.check(P.changed(both(x), both(nan)), P.upper_chain_support(n, rate, n_taps, follow=False), x.shape[1], where)
    assert np.abs(upper_sum(x, rate) - R.upper_band(x, rate)).max() < 1e-12
    for e in (u_ends, o_ends, c_ends):
        e.close()


def test_follow_forgets_a_hop_after_the_documented_number_of_hops():
    rate, gain = 48000, 1.0
    S, q, n_taps = P.hop_samples(rate), P.ratio(rate), len(taps(rate))
    hops = 12
    x = F.designed_x(rate, rows=1, hops=hops)
    d = R.decode64(taps(rate), x, q).astype(np.float32)
    y = (0.3 * d).astype(np.float32)          # (r = 0.3: off the clamp, so a change of an energy shows in g)
    g0, gamma0, out0, _ = F.follow(d, y, x, rate, gain)
    assert 0.0 < g0[0, 5] < gain
    a_ends, b_ends = Ends("follow, a"), Ends("follow, b")
    for s in (2, 3):
        for value in (np.float32(3.0), np.float32(np.nan)):
            d2 = d.copy()
            d2[0, s * 256 + 17] = value
            g, gamma, out, _ = F.follow(d2, y, x, rate, gain)
            assert np.isin(P.changed(g0, g), np.arange(s + 1, s + 1 + P.FOLLOW_HOPS)).all()
            a_ends.check(P.changed(gamma0, gamma), P.follow_support_a(s, rate), gamma0.shape[1], "a_%d" % s)
            assert np.isin(P.changed(out0, out), P.follow_support_a(s, rate)).all()
            y2 = y.copy()
            y2[0, s * 256 + 17] = value
            g, gamma, out, _ = F.follow(d, y2, x, rate, gain)
            assert np.isin(P.changed(g0, g), np.arange(s, s + P.FOLLOW_HOPS)).all()
            b_ends.check(P.changed(gamma0, gamma), P.follow_support_b(s, rate), gamma0.shape[1], "b_%d" % s)
    a_ends.close()
    b_ends.close()
    # the whole chain from one caller's sample: decode, follow on the decoded hops, encode(decode(x))
    def chain(v):
        dd = R.decode64(taps(rate), v, q)
        return F.follow(dd, dd, v, rate, gain)[2]
    base = chain(x.astype(np.float64))
    for n in positions(rate):
        for value in (1.0,):
            got = P.changed(base, chain(perturbed(x, n, value)))
            window = P.clip(P.upper_chain_support(n, rate, n_taps, follow=True), base.shape[1])
            assert len(got) and np.isin(got, window).all(), (n, value, got[~np.isin(got, window)][:8])
            assert window[-1] < base.shape[1] - S, "the run is long enough for the row to be clean again behind the window"


# ---- oracle B has the two properties ---------------------------------------------------------------------------------------------------
def test_the_oracle_contains_and_heals():
    """Batch 4, six frames, row 1 fed +Inf in bin 0, then 3e38, then NaN, its state zeroed in front of the last frame: the neighbours equal
    the clean twin's bit for bit, and the zeroed row equals the same row of an oracle that starts from nothing."""
    rng = np.random.default_rng(3)
    x = (0.25 * np.abs(rng.standard_normal((6, 4, 256)))).astype(np.float32)
    row, others, bad, heal = 1, [0, 2, 3], (2, 3, 4), 5

    def run(frames, first):
        ref = NutlsRef(batch=4, ctfa_mode="causal32")
        outs = []
        for f in range(first, frames.shape[0]):
            if first == 0 and f == heal:
                for v in list(ref.state.values()) + list(ref.ta_hist.values()):
                    v[row] = 0.0
            outs.append(ref.step(frames[f]).numpy().copy())
        return np.stack(outs), {k: v.numpy().copy() for k, v in ref.state.items()}

    xp = x.copy()
    for f, kind in zip(bad, ("inf", "big", "nan")):
        xp[f, row] = P.poison(x[f, row], kind)
    clean, clean_state = run(P.clean_twin(xp, row, bad), 0)
    fresh, fresh_state = run(x, heal)
    out, state = run(xp, 0)
    assert len(state) == len(T.state_specs("lstm")) == 130 and clean[:, others].any(axis=-1).all()
    assert not np.isfinite(out[2:5, row]).all(axis=-1).any()
    assert np.array_equal(out[:, others], clean[:, others])
    assert np.array_equal(out[heal:, row], fresh[:, row]) and np.isfinite(out[heal:]).all()
    for k in state:
        assert np.array_equal(state[k][others], clean_state[k][others]) and np.array_equal(state[k][row], fresh_state[k][row]), k
