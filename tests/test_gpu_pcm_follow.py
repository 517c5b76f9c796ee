"""GPU checks of the PCM gateway's following upper-band gain (include/nutls.h, "Upper band", follow; csrc/pcm.hip): the gain of the band
above 8 kHz follows the suppression the model applied below it -- g_t = gain * min(sqrt(B_t / A_t), 1) over windows of 4 hops, ramped across
the hop.  The references are
  - tests/pcm_follow_reference.py: the float64 restatement, at the bounds derived there (g: 20 * 2**-24 * g; an output sample:
    ``encode_with_upper``'s bound at the ceiling plus 24 * 2**-24 * gain * umag); an int16 result gets half a step (2**-16) on top;
  - the library itself for everything the contract promises bit for bit: the fixed-gain kernels where the followed gain stands still, the
    hop entry against its halves, every cut of a recording, masks, reset, switches, follow off against a handle never told, int16 against
    float32.
Shapes: 3 rows x 9 hops (offline handles of 9 frames with 3 utterances), 32 and 48 kHz, LSTM variant with the shipped weights."""
import ctypes

import numpy as np
import pytest
import torch      # (before the first handle: torch must bring up the HIP runtime it ships with itself)

from nunet_amd import NutlsEngine, NutlsOffline

import pcm_follow_reference as F
import pcm_upper_reference as R

pytestmark = pytest.mark.gpu
B, HOPS = F.ROWS, F.HOPS
E = 2.0 ** -24


def as_s16(x):
    return np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hops_of(x, unit):
    return [np.ascontiguousarray(x[:, k * unit:(k + 1) * unit]) for k in range(x.shape[1] // unit)]


def engine(rate, dtype, gain, follow=True, **kw):
    e = NutlsEngine(batch=B, **kw)
    e.set_pcm_format(rate, dtype)
    if gain is not None:
        e.set_pcm_upper_band(gain)
    if follow:
        e.set_pcm_upper_follow(True)
    assert e.pcm_upper_follow == bool(follow)
    return e


def offline(rate, dtype, gain, follow=True):
    o = NutlsOffline(max_frames=HOPS, utterances=B)
    o.set_pcm_format(rate, dtype)
    o.set_pcm_upper_band(gain)
    o.set_pcm_upper_follow(follow)
    assert o.pcm_upper_follow == bool(follow)
    return o


def feed_of(rate, dtype, seed=300):
    """(what the handle is fed, the same samples as float32)"""
    x = F.designed_x(rate, seed=seed)
    if dtype == "int16":
        s = as_s16(x)
        return s, s.astype(np.float32) / np.float32(32768.0)      # exact: what the kernel converts to
    return x, x


# ---- 1. exact identities through the halves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1.0, 0.25, 2.0])
@pytest.mark.parametrize("rate,dtype", [(32000, "float32"), (48000, "int16")])
def test_a_scaled_copy_of_the_input_gives_the_fixed_gain_bit_for_bit(rate, dtype, c):
    """y_t = c d_{t-1}, c a power of two: b_t is a_{t-1} times c^2 to the bit if and only if the two kernels' energy code is the same
    arithmetic, B / A = c^2 and the square root are exact, and at delta = 0 the ramp is its left end exactly."""
    gain, S = 0.75, F.hop_len(rate)
    want_g = np.float32(gain * min(c, 1.0))
    feed, _ = feed_of(rate, dtype)
    fol, fix = engine(rate, dtype, gain), engine(rate, dtype, float(want_g), follow=False)
    before = torch.zeros(B, 256, device="cuda")
    ramped = False
    for t, h in enumerate(hops_of(feed, S)):
        d = fol.pcm_decode_hop(dev(h))
        assert torch.equal(d, fix.pcm_decode_hop(dev(h))), t
        y = (c * before).contiguous()      # exact
        got, want = fol.pcm_encode_hop(y), fix.pcm_encode_hop(y)
        g = fol.pcm_follow_gain()
        assert g.dtype == np.float32 and g.shape == (B,)
        if t == 0:
            assert np.all(g == 0.0)        # nothing decoded in front, nothing handed over
        else:
            assert np.all(g == want_g), (t, g)
        if t >= 2:
            assert torch.equal(got, want), t
        elif t == 1:
            ramped = not torch.equal(got, want)
        before = d
    assert ramped, "hop 1 ramps from 0 to g: it cannot be the fixed gain's"
    assert want.cpu().numpy().any()
    fol.close(); fix.close()


# ---- 2. against float64 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("rate", [32000, 48000])
def test_against_float64(rate, dtype):
    gain, S = 0.875, F.hop_len(rate)
    feed, x = feed_of(rate, dtype)
    eng = engine(rate, dtype, gain)
    ds, ys, outs, gs = [], [], [], []
    for t, h in enumerate(hops_of(feed, S)):
        ds.append(eng.pcm_decode_hop(dev(h)).cpu().numpy())
        ys.append(F.designed_y_hop(ds[t - 1] if t else None, t))
        outs.append(eng.pcm_encode_hop(dev(ys[t])).cpu().numpy())
        gs.append(eng.pcm_follow_gain())
    eng.close()
    d, y, got, got_g = np.concatenate(ds, axis=1), np.concatenate(ys, axis=1), np.concatenate(outs, axis=1), np.stack(gs, axis=1)
    g, gamma, want, bound = F.follow(d, y, x, rate, gain)
    _, _, r = F.windows(d, y)
    assert np.all(r[:, 2:5] > 1.0) and np.all(r[:, -1] < 0.1) and np.all((r[:, 1:] < 0.5).sum(axis=1) >= 3)      # across 1 and down to about 0.05
    gerr = np.abs(got_g.astype(np.float64) - g)
    print("%d Hz %s: g of row 0 %s; worst |g32 - g| / (2^-24 g) = %.2f (bound %d)" % (
        rate, dtype, np.array2string(got_g[0], precision=4), (gerr / np.maximum(E * g, 1e-300)).max(), F.G_ROUNDINGS))
    assert np.all(gerr <= F.G_ROUNDINGS * E * g)
    assert got.shape == x.shape and got.dtype == np.dtype(dtype)
    if dtype == "int16":
        got = got.astype(np.float64) / 32768.0
        want = np.clip(want, -1.0, 32767.0 / 32768.0)      # saturation moves a value towards the range, never away from the float's
        bound = bound + 2.0 ** -16
    err = np.abs(got.astype(np.float64) - want)
    print("%d Hz %s: worst error %.3g, worst error / bound %.3f" % (rate, dtype, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), float((err - bound).max())
    # the followed gain is in there: against the fixed gain the result is off by (gain - gamma) u, far beyond the bound
    fixed, _ = R.encode_with_upper(y, x, rate, gain)
    assert np.abs(fixed - F.follow(d, y, x, rate, gain)[2])[:, 5 * S:].max() > 1000 * bound[:, 5 * S:].max()


# ---- 3. the hop entry is its halves -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", [False, True])
@pytest.mark.parametrize("rate", [48000, 32000])
def test_the_pcm_hop_is_decode_enhance_encode(rate, fusion):
    feed, _ = feed_of(rate, "int16", seed=330)
    one, twin, fixed = (engine(rate, "int16", 1.0, follow=f, hop_fusion=fusion) for f in (True, True, False))
    assert one.launches_per_hop == (1 if fusion else 3)
    differs = False
    for k, h in enumerate(hops_of(feed, F.hop_len(rate))[:6]):
        got = one.enhance_hop_pcm(dev(h))
        want = twin.pcm_encode_hop(twin.enhance_hop(twin.pcm_decode_hop(dev(h))))
        assert got.dtype == torch.int16 and torch.equal(got, want), k
        assert np.array_equal(one.pcm_follow_gain(), twin.pcm_follow_gain()), k
        differs = differs or not torch.equal(got, fixed.enhance_hop_pcm(dev(h)))
    assert differs, "follow returns what the fixed gain returns: it is not there"
    for e in (one, twin, fixed):
        e.close()


# ---- 4. cuts ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,dtype", [(48000, "int16"), (32000, "float32")])
def test_every_cut_of_a_recording_gives_the_same_bits(rate, dtype):
    S = F.hop_len(rate)
    feed, _ = feed_of(rate, dtype, seed=340)
    junk = np.full((B, HOPS * S), np.nan, np.float32) if dtype == "float32" else np.full((B, HOPS * S), 0x7FFF, np.int16)
    off = offline(rate, dtype, 1.0)
    whole = off.enhance_block_pcm_device(dev(feed))
    whole_g = off.pcm_follow_gain()
    assert whole.cpu().numpy().any() and np.all(whole_g > 0) and np.all(whole_g <= 1)
    for cut in ((4, 5), (1,) * HOPS):
        off.reset()
        assert np.all(off.pcm_follow_gain() == 0.0)
        at, parts = 0, []
        for n in cut:
            parts.append(off.enhance_block_pcm_device(dev(feed[:, at * S:(at + n) * S])))
            at += n
        assert torch.equal(torch.cat(parts, dim=1), whole), cut
        assert np.array_equal(off.pcm_follow_gain(), whole_g), cut
    # ragged counts, a held utterance (k = 0) in the middle of utterance 1 and at the end of the others
    off.reset()
    at = [0] * B
    for counts in ([5, 3, 4], [4, 0, 5], [0, 6, 0]):
        n = max(counts)
        blk = junk[:, :n * S].copy()
        for u, k in enumerate(counts):
            blk[u, :k * S] = feed[u, at[u] * S:(at[u] + k) * S]
        before = off.pcm_follow_gain()
        got = off.enhance_block_pcm_device(dev(blk), hops=counts)
        after = off.pcm_follow_gain()
        for u, k in enumerate(counts):
            assert torch.equal(got[u, :k * S], whole[u, at[u] * S:(at[u] + k) * S]), (counts, u)
            assert not got[u, k * S:].cpu().numpy().view(np.uint8).any(), (counts, u)
            if k == 0:
                assert after[u] == before[u] and (at[u] == 0 or after[u] > 0), (counts, u)      # held: its gain stays where it was
            at[u] += k
    assert at == [HOPS] * B and np.array_equal(off.pcm_follow_gain(), whole_g)
    # the halves of the offline handle against the hop halves of a streaming handle fed the same rows
    y = (0.1 * np.random.default_rng(341).standard_normal((B, HOPS * 256))).astype(np.float32)
    y[:, 4 * 256:] *= 0.1
    off.reset()
    blk_dec = off.pcm_decode_block_device(dev(feed))
    blk_enc = off.pcm_encode_block_device(dev(y))
    blk_g = off.pcm_follow_gain()
    off.close()
    stream = engine(rate, dtype, 1.0)
    hop_dec, hop_enc = [], []
    for xh, yh in zip(hops_of(feed, S), hops_of(y, 256)):
        hop_dec.append(stream.pcm_decode_hop(dev(xh)))
        hop_enc.append(stream.pcm_encode_hop(dev(yh)))
    assert torch.equal(torch.cat(hop_dec, dim=1), blk_dec) and torch.equal(torch.cat(hop_enc, dim=1), blk_enc)
    assert np.array_equal(stream.pcm_follow_gain(), blk_g) and np.all(blk_g < 0.5) and np.all(blk_g > 0)
    stream.close()


def test_a_held_stream_keeps_its_follow_state():
    rate, ticks = 48000, 6
    feed, _ = feed_of(rate, "float32", seed=350)
    hops = hops_of(feed, F.hop_len(rate))[:ticks]
    masks = np.ones((ticks, B), np.uint8)
    masks[1, 1] = masks[2, 1] = 0      # stream 1 takes its hops at ticks 0, 3, 4, 5
    ref = engine(rate, "float32", 1.0)
    want, want_g = [], []
    for h in hops:                     # lockstep: every stream takes its k-th hop at step k
        want.append(ref.enhance_hop_pcm(dev(h)).cpu().numpy())
        want_g.append(ref.pcm_follow_gain())
    ref.close()
    assert want_g[0][1] > 0
    for host in (False, True):
        eng = engine(rate, "float32", 1.0)
        taken = 0
        for t in range(ticks):
            feed_t = hops[t].copy()
            feed_t[1] = hops[taken][1] if masks[t, 1] else np.nan      # a held row may hold anything
            if host:
                out = eng.enhance_hop_pcm(feed_t, active=masks[t])
            else:
                out = eng.enhance_hop_pcm(dev(feed_t), active=dev(masks[t])).cpu().numpy()
            g = eng.pcm_follow_gain()
            assert np.array_equal(out[0], want[t][0]) and np.array_equal(out[2], want[t][2]), (host, t)
            assert g[0] == want_g[t][0] and g[2] == want_g[t][2], (host, t)
            if masks[t, 1]:
                assert np.array_equal(out[1], want[taken][1]), (host, t, taken)
                taken += 1
            else:
                assert not out[1].any(), (host, t)
            assert g[1] == want_g[taken - 1][1], (host, t)      # held: the gain of its last real hop
        assert taken == 4
        eng.close()


# ---- 5. restarts --------------------------------------------------------------------------------------------------------------------------------
def test_reset_and_switches_restart_follow():
    rate, S = 32000, F.hop_len(32000)
    feed, _ = feed_of(rate, "float32", seed=360)
    hops = hops_of(feed, S)
    y = hops_of((0.05 * np.random.default_rng(361).standard_normal((B, HOPS * 256))).astype(np.float32), 256)
    a, whole, fresh = (engine(rate, "float32", 1.0) for _ in range(3))
    for k in range(3):
        assert torch.equal(a.enhance_hop_pcm(dev(hops[k])), whole.enhance_hop_pcm(dev(hops[k]))), k
    g = a.pcm_follow_gain()
    a.reset(1)
    g1 = a.pcm_follow_gain()
    assert g1[1] == 0.0 and g[1] > 0 and g1[0] == g[0] and g1[2] == g[2]      # row 1's alone
    for k in range(3, 6):
        got = a.enhance_hop_pcm(dev(hops[k])).cpu().numpy()
        cont = whole.enhance_hop_pcm(dev(hops[k])).cpu().numpy()
        new = fresh.enhance_hop_pcm(dev(hops[k])).cpu().numpy()
        assert np.array_equal(got[0], cont[0]) and np.array_equal(got[2], cont[2]), k
        assert np.array_equal(got[1], new[1]), k
        assert not np.array_equal(got[1], cont[1]), k
        ga, gw, gf = a.pcm_follow_gain(), whole.pcm_follow_gain(), fresh.pcm_follow_gain()
        assert ga[0] == gw[0] and ga[2] == gw[2] and ga[1] == gf[1], k

    def run(e, ks):      # (the halves: the model's own state is not theirs)
        out = []
        for k in ks:
            out.append(e.pcm_decode_hop(dev(hops[k])))
            out.append(e.pcm_encode_hop(dev(y[k])))
        return out

    def same(p, q):
        return all(torch.equal(u, v) for u, v in zip(p, q))

    # toggling follow restarts everyone: off is the fixed gain from zero histories, on again is follow from zero state
    b, fixed, c = engine(rate, "float32", 1.0), engine(rate, "float32", 1.0, follow=False), engine(rate, "float32", 1.0)
    run(b, range(3))
    b.set_pcm_upper_follow(False)
    assert not b.pcm_upper_follow and b.pcm_upper_band == 1.0
    assert same(run(b, range(3, 6)), run(fixed, range(3, 6)))
    b.set_pcm_upper_follow(True)
    assert np.all(b.pcm_follow_gain() == 0.0)
    assert same(run(b, range(2, 6)), run(c, range(2, 6))) and np.array_equal(b.pcm_follow_gain(), c.pcm_follow_gain())
    # a new gain keeps follow and restarts everyone
    d = engine(rate, "float32", 0.5)
    b.set_pcm_upper_band(0.5)
    assert b.pcm_upper_follow and np.all(b.pcm_follow_gain() == 0.0)
    assert same(run(b, range(1, 5)), run(d, range(1, 5))) and np.array_equal(b.pcm_follow_gain(), d.pcm_follow_gain())
    # ... the values in force do not (no-ops): b goes on where a handle that was not told again goes on
    b.set_pcm_upper_band(0.5)
    b.set_pcm_upper_follow(True)
    assert same(run(b, [5, 6]), run(d, [5, 6])) and np.array_equal(b.pcm_follow_gain(), d.pcm_follow_gain())
    # gain 0 turns follow off, and a later gain does not bring it back
    b.set_pcm_upper_band(0.0)
    assert not b.pcm_upper_follow
    b.set_pcm_upper_band(1.0)
    fixed.set_pcm_upper_band(0.0)
    fixed.set_pcm_upper_band(1.0)
    assert not b.pcm_upper_follow and same(run(b, range(4)), run(fixed, range(4)))
    # a new format turns follow and the upper band off
    assert d.pcm_upper_follow
    d.set_pcm_format(rate, "float32")
    assert not d.pcm_upper_follow and d.pcm_upper_band == 0.0
    plain = engine(rate, "float32", None, follow=False)
    assert same(run(d, range(3)), run(plain, range(3)))
    for e in (a, whole, fresh, b, fixed, c, d, plain):
        e.close()


# ---- 6. follow off is the gateway without it ------------------------------------------------------------------------------------------------------
def test_follow_off_is_the_gateway_that_never_had_it():
    rate = 48000
    feed, _ = feed_of(rate, "int16", seed=370)
    hops = hops_of(feed, F.hop_len(rate))
    back, never = engine(rate, "int16", 1.0), engine(rate, "int16", 1.0, follow=False)
    for h in hops[:3]:
        back.enhance_hop_pcm(dev(h))
    back.set_pcm_upper_follow(False)
    back.reset()
    for k, h in enumerate(hops[3:]):
        want = never.enhance_hop_pcm(dev(h))
        assert torch.equal(back.enhance_hop_pcm(dev(h)), want), k
    assert want.cpu().numpy().any()
    back.close(); never.close()


# ---- 7. int16 ---------------------------------------------------------------------------------------------------------------------------------
def test_int16_is_the_float_result_quantised_and_saturates():
    rate, hops, S = 48000, 6, F.hop_len(48000)
    t = np.arange(hops * S, dtype=np.float64)
    # a low-band tone (1 kHz) and an upper-band tone (12 kHz) of amplitude 0.7 each, both cosines: their peaks coincide every millisecond;
    # the encode half is handed the low-band tone as it is (r about 1: the gain stays near its ceiling) and, from hop 4 on, a tenth of it
    tone = 0.7 * np.cos(2 * np.pi * 1000.0 / rate * t) + 0.7 * np.cos(2 * np.pi * 12000.0 / rate * t)
    s = as_s16(np.stack([tone, -tone, 0.5 * tone]))
    f = s.astype(np.float32) / np.float32(32768.0)
    low = np.stack([0.7 * np.cos(2 * np.pi * 1000.0 / 16000.0 * np.arange(hops * 256))] * B) * np.array([[1], [-1], [0.5]])
    low[:, 4 * 256:] *= 0.1
    y = hops_of(low.astype(np.float32), 256)
    res, gains = {}, {}
    for dtype, x in (("float32", f), ("int16", s)):
        eng = engine(rate, dtype, 1.0)
        out = []
        for xh, yh in zip(hops_of(x, S), y):
            eng.pcm_decode_hop(dev(xh))
            out.append(eng.pcm_encode_hop(dev(yh)))
        res[dtype], gains[dtype] = torch.cat(out, dim=1).cpu().numpy(), eng.pcm_follow_gain()
        eng.close()
    assert res["int16"].dtype == np.int16
    assert np.array_equal(res["int16"], as_s16(res["float32"])) and np.array_equal(gains["int16"], gains["float32"])
    assert np.abs(res["float32"]).max() > 1.2, "the float result does not leave +-1: nothing saturates"
    assert res["int16"].max() == 32767 and res["int16"].min() == -32768
    assert np.all(gains["float32"] < 0.9) and np.all(gains["float32"] > 0.05)      # and the gain has come down behind hop 4


# ---- 8. refusals change nothing -----------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    for rate in (16000, 8000, 48000):      # gain 0: at 8 and 16 kHz it cannot be anything else
        S = F.hop_len(rate)
        x = hops_of(as_s16(0.3 * np.random.default_rng(380).standard_normal((B, 3 * S))), S)
        eng, twin = engine(rate, "int16", None, follow=False), engine(rate, "int16", None, follow=False)
        assert torch.equal(eng.enhance_hop_pcm(dev(x[0])), twin.enhance_hop_pcm(dev(x[0])))
        with pytest.raises(ValueError, match="nutls_set_pcm_upper_follow"):
            eng.set_pcm_upper_follow(True)
        assert not eng.pcm_upper_follow and eng.pcm_upper_band == 0.0
        eng.set_pcm_upper_follow(False)      # (what the handle has: allowed everywhere)
        with pytest.raises(ValueError, match="nutls_pcm_follow_gain"):
            eng.pcm_follow_gain()
        for k in (1, 2):
            assert torch.equal(eng.enhance_hop_pcm(dev(x[k])), twin.enhance_hop_pcm(dev(x[k]))), (rate, k)
        eng.close(); twin.close()
    rate = 48000
    feed, _ = feed_of(rate, "int16", seed=381)
    x = hops_of(feed, F.hop_len(rate))
    off_eng, off_twin = engine(rate, "int16", 0.5, follow=False), engine(rate, "int16", 0.5, follow=False)
    on_eng, on_twin = engine(rate, "int16", 0.5), engine(rate, "int16", 0.5)
    buf = (ctypes.c_float * (B + 1))(*([7.0] * (B + 1)))
    for k in range(4):
        for eng, twin in ((off_eng, off_twin), (on_eng, on_twin)):
            assert torch.equal(eng.enhance_hop_pcm(dev(x[k])), twin.enhance_hop_pcm(dev(x[k]))), k
        with pytest.raises(ValueError, match="nutls_pcm_follow_gain"):
            off_eng.pcm_follow_gain()      # follow off
        for n in (B + 1, B - 1, 0):          # a wrong n
            assert on_eng._lib.nutls_pcm_follow_gain(on_eng._h, buf, n) == -1
            assert b"nutls_pcm_follow_gain" in on_eng._lib.nutls_last_error() and list(buf) == [7.0] * (B + 1)
        assert on_eng._lib.nutls_pcm_follow_gain(on_eng._h, None, B) == -1
        assert np.array_equal(on_eng.pcm_follow_gain(), on_twin.pcm_follow_gain())
    for e in (off_eng, off_twin, on_eng, on_twin):
        e.close()
