"""GPU checks of the PCM gateway's upper band (include/nutls.h, "Upper band"; csrc/pcm.hip): the band above 8 kHz of a 32 / 48 kHz caller,
passed around the model inside the two conversion launches and added back at a gain.  The reference refuses anything but float samples at
16 kHz (dnn_model/interpreter_proposed.py:384-385), so the references here are
  - tests/pcm_upper_reference.py: float64 ``upfirdn`` with the taps of ``nutls_pcm_filter``, per sample, at the bound computed from the
    operation order the header documents: ``(N + 3) * 2**-24 * (sum of absolute products)``, N = 2 K q + 2 K + 4.  An int16 result is that
    float quantised, so it gets half a step (2**-16) on top, against the float64 value saturated to the int16 range;
  - the library itself for everything the contract promises bit for bit (torch.equal / np.array_equal): gain 0 against a handle never told,
    the hop entry against its halves, masks, reset, gain and format switches, cuts of a block, ragged counts, int16 against float32.
    Between a streaming and an offline handle the halves are compared bit for bit; the whole entries are compared at the bound
    tests/test_gpu_enhance_block.py has between block mode and the streaming path (relative RMS 1e-5): the model kernels of the two differ.
Shapes: 3 streams, at most 12 hops, offline handles of 8 frames with 3 utterances, LSTM variant with the shipped weights."""
import numpy as np
import pytest
import torch      # (before the first handle: torch must bring up the HIP runtime it ships with itself)
from scipy import signal

from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner

import pcm_upper_reference as R

pytestmark = pytest.mark.gpu
B = 3
K = 24


def hop_len(rate):
    return 256 * rate // 16000


def designed(rate, rows, hops, seed, out_of_band=True):
    """[rows, hops * S] float32: a tone at 0.3 of the lower rate's Nyquist frequency, one at 1.4 (rates above 16 kHz) and seeded noise."""
    rng = np.random.default_rng(seed)
    n = hops * hop_len(rate)
    t = np.arange(n, dtype=np.float64)
    nyq = min(rate, 16000) / 2.0
    x = 0.35 * np.sin(2 * np.pi * 0.3 * nyq / rate * t[None, :] + rng.uniform(0, 6.28, (rows, 1)))
    if rate > 16000 and out_of_band:
        x = x + 0.3 * np.sin(2 * np.pi * 1.4 * nyq / rate * t[None, :] + rng.uniform(0, 6.28, (rows, 1)))
    x = x + 0.1 * rng.standard_normal((rows, n))
    return x.astype(np.float32)


def as_s16(x):
    return np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hops_of(x, unit):
    return [np.ascontiguousarray(x[:, k * unit:(k + 1) * unit]) for k in range(x.shape[1] // unit)]


def engine(rate, dtype, gain, **kw):
    e = NutlsEngine(batch=B, **kw)
    e.set_pcm_format(rate, dtype)
    if gain is not None:
        e.set_pcm_upper_band(gain)
    return e


def offline(rate, dtype, gain):
    o = NutlsOffline(max_frames=8, utterances=B)
    o.set_pcm_format(rate, dtype)
    o.set_pcm_upper_band(gain)
    return o


# ---- 1. the halves against float64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("rate", [32000, 48000])
def test_halves_against_float64(rate, dtype):
    hops, S = 8, hop_len(rate)
    x = 0.5 * designed(rate, B, hops, seed=200 + rate // 16000)
    if dtype == "int16":
        feed = as_s16(x)
        x = feed.astype(np.float32) / np.float32(32768.0)      # exact: what the kernel converts to
    else:
        feed = x
    y = (0.2 * np.random.default_rng(210).standard_normal((B, hops * 256))).astype(np.float32)
    eng = engine(rate, dtype, None)
    for g in (0.5, 1.0):
        eng.set_pcm_upper_band(g)      # (restarts every history and the upper band)
        assert eng.pcm_upper_band == g
        out = []
        for xh, yh in zip(hops_of(feed, S), hops_of(y, 256)):
            eng.pcm_decode_hop(dev(xh))
            out.append(eng.pcm_encode_hop(dev(yh)))
        got = torch.cat(out, dim=1).cpu().numpy()
        want, bound = R.encode_with_upper(y, x, rate, g)
        assert got.shape == x.shape and got.dtype == np.dtype(dtype)
        if dtype == "int16":
            got = got.astype(np.float64) / 32768.0
            want = np.clip(want, -1.0, 32767.0 / 32768.0)      # saturation moves a value towards the range, never away from the float's
            bound = bound + 2.0 ** -16
        err = np.abs(got.astype(np.float64) - want)
        rel = err / np.maximum(bound, 1e-300)
        print("%d Hz %s g = %.1f: worst error %.3g, worst error / bound %.3f (first two hops: %.3f)" % (
            rate, dtype, g, err.max(), rel.max(), rel[:, :2 * S].max()))
        assert np.all(err <= bound), float((err - bound).max())
        # the upper band is in there: without it the result is off by g u, far beyond the bound
        u = R.upper_band(x, rate)
        assert np.sqrt(np.mean(u[:, S:] ** 2)) > 0.05
    eng.close()


# ---- 2. gain 0 is today ---------------------------------------------------------------------------------------------------------------------
def test_gain_zero_is_the_gateway_without_the_upper_band():
    rate = 48000
    x = as_s16(0.5 * designed(rate, B, 6, seed=220))
    told, never, back = engine(rate, "int16", 0.0), engine(rate, "int16", None), engine(rate, "int16", 1.0)
    back.reset()
    back.set_pcm_upper_band(0.0)
    assert told.pcm_upper_band == never.pcm_upper_band == back.pcm_upper_band == 0.0
    for k, h in enumerate(hops_of(x, hop_len(rate))):
        want = never.enhance_hop_pcm(dev(h))
        assert torch.equal(told.enhance_hop_pcm(dev(h)), want), k
        assert torch.equal(back.enhance_hop_pcm(dev(h)), want), k
    assert want.cpu().numpy().any()
    for e in (told, never, back):
        e.close()


# ---- 3. the hop entry is its halves -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", [False, True])
@pytest.mark.parametrize("rate", [48000, 32000])
def test_the_pcm_hop_is_decode_enhance_encode(rate, fusion):
    x = as_s16(0.5 * designed(rate, B, 4, seed=230))
    one, twin, off = (engine(rate, "int16", g, hop_fusion=fusion) for g in (1.0, 1.0, 0.0))
    assert one.launches_per_hop == (1 if fusion else 3)
    differs = False
    for k, h in enumerate(hops_of(x, hop_len(rate))):
        got = one.enhance_hop_pcm(dev(h))
        want = twin.pcm_encode_hop(twin.enhance_hop(twin.pcm_decode_hop(dev(h))))
        assert got.dtype == torch.int16 and torch.equal(got, want), k
        differs = differs or not torch.equal(got, off.enhance_hop_pcm(dev(h)))
    assert differs, "gain 1 returns what gain 0 returns: the upper band is not there"
    for e in (one, twin, off):
        e.close()


# ---- 4. the band comes back, aligned ----------------------------------------------------------------------------------------------------------
def test_the_band_comes_back_aligned():
    rate = 48000
    x = (0.5 * designed(rate, 1, 12, seed=240)[0]).astype(np.float32)
    res = {}
    for g in (1.0, 0.0):
        off = NutlsOffline(max_frames=8)
        res[g] = off.enhance_wave(x, rate, upper_gain=g).astype(np.float64)
        assert off.pcm_upper_band == g and res[g].shape == x.shape
        off.close()
    # one float64 linear-phase high-pass for all three: stopband up to 9.2 kHz (Kaiser, beta 12: 120 dB), passband from 10.4 kHz
    taps = signal.firwin(401, 9800.0, window=("kaiser", 12.0), pass_zero=False, fs=rate)
    w, h = signal.freqz(taps, worN=4096, fs=rate)
    assert 20 * np.log10(np.abs(h[w <= 9200.0]).max()) <= -110.0 and np.abs(20 * np.log10(np.abs(h[w >= 10400.0]))).max() <= 0.01

    def hp(a):
        return np.convolve(a, taps, mode="same")[len(taps):-len(taps)]      # the same index for all; the filter's edge transients dropped

    rms = lambda a: float(np.sqrt(np.mean(a ** 2)))      # noqa: E731
    limit = 3 * 10 ** (-80 / 20) * rms(res[0.0])
    diff, dull, band = rms(hp(res[1.0]) - hp(x.astype(np.float64))), rms(hp(res[0.0])), rms(hp(x.astype(np.float64)))
    print("rms: gain-0 output %.4g, limit %.4g; input above 9.2 kHz %.4g; gain 1 minus input above 9.2 kHz %.4g; gain 0 above 9.2 kHz %.4g" % (
        rms(res[0.0]), limit, band, diff, dull))
    assert band > 100 * limit, "the input has nothing up there: the checks below would show nothing"
    assert diff <= limit
    assert dull <= limit


# ---- 5. held streams --------------------------------------------------------------------------------------------------------------------------
def test_a_held_stream_keeps_its_upper_band():
    rate, ticks = 48000, 6
    x = 0.5 * designed(rate, B, ticks, seed=250)
    hops = hops_of(x, hop_len(rate))
    masks = np.ones((ticks, B), np.uint8)
    masks[1, 1] = masks[2, 1] = 0      # stream 1 takes its hops at ticks 0, 3, 4, 5
    ref = engine(rate, "float32", 1.0)
    want = [ref.enhance_hop_pcm(dev(h)).cpu().numpy() for h in hops]      # lockstep: every stream takes its k-th hop at step k
    ref.close()
    for host in (False, True):
        eng = engine(rate, "float32", 1.0)
        taken = 0
        for t in range(ticks):
            feed = hops[t].copy()
            feed[1] = hops[taken][1] if masks[t, 1] else np.nan      # a held row may hold anything
            if host:
                out = eng.enhance_hop_pcm(feed, active=masks[t])
            else:
                out = eng.enhance_hop_pcm(dev(feed), active=dev(masks[t])).cpu().numpy()
            assert np.array_equal(out[0], want[t][0]) and np.array_equal(out[2], want[t][2]), (host, t)
            if masks[t, 1]:
                assert np.array_equal(out[1], want[taken][1]), (host, t, taken)
                taken += 1
            else:
                assert not out[1].any(), (host, t)
        assert taken == 4
        eng.close()


# ---- 6. reset and switches --------------------------------------------------------------------------------------------------------------------
def test_reset_gain_and_format_switches_restart_the_upper_band():
    rate, S = 32000, hop_len(32000)
    x = 0.5 * designed(rate, B, 6, seed=260)
    hops = hops_of(x, S)
    y = hops_of((0.2 * np.random.default_rng(261).standard_normal((B, 6 * 256))).astype(np.float32), 256)
    a, whole, fresh = (engine(rate, "float32", 1.0) for _ in range(3))
    for k in range(3):
        assert torch.equal(a.enhance_hop_pcm(dev(hops[k])), whole.enhance_hop_pcm(dev(hops[k]))), k
    a.reset(1)
    for k in range(3, 6):
        got = a.enhance_hop_pcm(dev(hops[k])).cpu().numpy()
        cont = whole.enhance_hop_pcm(dev(hops[k])).cpu().numpy()
        new = fresh.enhance_hop_pcm(dev(hops[k])).cpu().numpy()
        assert np.array_equal(got[0], cont[0]) and np.array_equal(got[2], cont[2]), k
        assert np.array_equal(got[1], new[1]), k
        assert not np.array_equal(got[1], cont[1]), k
    # a new gain starts the resamplers and the upper band anew (the halves: the model's own state is not theirs)
    b, c = engine(rate, "float32", 1.0), engine(rate, "float32", 0.5)
    for k in range(3):
        b.pcm_decode_hop(dev(hops[k]))
        b.pcm_encode_hop(dev(y[k]))
    b.set_pcm_upper_band(0.5)
    for k in range(3, 6):
        assert torch.equal(b.pcm_decode_hop(dev(hops[k])), c.pcm_decode_hop(dev(hops[k]))), k
        assert torch.equal(b.pcm_encode_hop(dev(y[k])), c.pcm_encode_hop(dev(y[k]))), k
    # ... the gain in force does not (a no-op): b goes on where a handle that was not told again goes on
    b.set_pcm_upper_band(0.5)
    assert torch.equal(b.pcm_decode_hop(dev(hops[0])), c.pcm_decode_hop(dev(hops[0])))
    assert torch.equal(b.pcm_encode_hop(dev(y[0])), c.pcm_encode_hop(dev(y[0])))
    # a new format turns the upper band off
    assert b.pcm_upper_band == 0.5
    b.set_pcm_format(rate, "float32")
    assert b.pcm_upper_band == 0.0
    plain = engine(rate, "float32", None)
    assert torch.equal(b.pcm_decode_hop(dev(hops[1])), plain.pcm_decode_hop(dev(hops[1])))
    assert torch.equal(b.pcm_encode_hop(dev(y[1])), plain.pcm_encode_hop(dev(y[1])))
    for e in (a, whole, fresh, b, c, plain):
        e.close()


# ---- 7. blocks, cuts, ragged ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,dtype", [(48000, "int16"), (32000, "float32")])
def test_blocks_cuts_and_ragged_counts(rate, dtype):
    hops, S = 8, hop_len(rate)
    x = 0.5 * designed(rate, B, 2 * hops, seed=270)
    x = as_s16(x) if dtype == "int16" else x
    first, second = x[:, :hops * S], x[:, hops * S:]
    junk = np.full((B, hops * S), np.nan, np.float32) if dtype == "float32" else np.full((B, hops * S), 0x7FFF, np.int16)
    off = offline(rate, dtype, 1.0)
    whole = off.enhance_block_pcm_device(dev(first))
    whole2 = off.enhance_block_pcm_device(dev(second))      # (the carried state: the second block of the uniform run)
    assert whole.cpu().numpy().any()
    for cut in ((3, 5), (1, 7)):
        off.reset()
        at, parts = 0, []
        for n in cut:
            parts.append(off.enhance_block_pcm_device(dev(first[:, at * S:(at + n) * S])))
            at += n
        assert torch.equal(torch.cat(parts, dim=1), whole), cut
    # the halves of an offline handle against those of a streaming handle fed the same rows, bit for bit; the whole entries at the bound
    # block mode has against the streaming path
    y = (0.2 * np.random.default_rng(271).standard_normal((B, hops * 256))).astype(np.float32)
    off.reset()
    blk_dec = off.pcm_decode_block_device(dev(first))
    blk_enc = off.pcm_encode_block_device(dev(y))
    stream = engine(rate, dtype, 1.0)
    hop_dec, hop_enc = [], []
    for xh, yh in zip(hops_of(first, S), hops_of(y, 256)):
        hop_dec.append(stream.pcm_decode_hop(dev(xh)))
        hop_enc.append(stream.pcm_encode_hop(dev(yh)))
    assert torch.equal(torch.cat(hop_dec, dim=1), blk_dec) and torch.equal(torch.cat(hop_enc, dim=1), blk_enc)
    stream.reset()
    got = torch.cat([stream.enhance_hop_pcm(dev(h)) for h in hops_of(first, S)], dim=1).cpu().numpy().astype(np.float64)
    ref = whole.cpu().numpy().astype(np.float64)
    rel = np.sqrt(np.mean((got - ref) ** 2) / np.mean(ref ** 2))
    print("hop entries vs block entry at %d Hz %s: relative rms %.3e (bound %s)" % (rate, dtype, rel, "1e-5" if dtype == "float32" else "1e-5 + half a step"))
    assert rel <= 1e-5 + (2.0 ** -16 / np.sqrt(np.mean((ref / 32768.0) ** 2)) if dtype == "int16" else 0.0)
    stream.close()
    # ragged counts [8, 3, 0]
    off.reset()
    counts = [8, 3, 0]
    blk = junk.copy()
    for u, k in enumerate(counts):
        blk[u, :k * S] = first[u, :k * S]
    got = off.enhance_block_pcm_device(dev(blk), hops=counts)
    for u, k in enumerate(counts):
        assert torch.equal(got[u, :k * S], whole[u, :k * S]), u      # in front of the count: the uniform call's bits
        assert not got[u, k * S:].cpu().numpy().view(np.uint8).any(), u      # behind it: zeros, whatever the input held
    # the next block continues each utterance from its own last real hop: utterance 0 with its second block, utterance 1 with hops 3 .. 7 of
    # its first, the held utterance 2 with its first block from the start
    nxt = junk.copy()
    nxt[0] = second[0]
    nxt[1, :5 * S] = first[1, 3 * S:]
    nxt[2] = first[2]
    got = off.enhance_block_pcm_device(dev(nxt), hops=[8, 5, 8])
    assert torch.equal(got[0], whole2[0])
    assert torch.equal(got[1, :5 * S], whole[1, 3 * S:]) and not got[1, 5 * S:].cpu().numpy().view(np.uint8).any()
    assert torch.equal(got[2], whole[2])
    off.close()


# ---- 8. int16 and saturation ------------------------------------------------------------------------------------------------------------------
def test_int16_is_the_float_result_quantised_and_saturates():
    rate, hops, S = 48000, 5, hop_len(48000)
    t = np.arange(hops * S, dtype=np.float64)
    # a low-band tone (1 kHz) and an upper-band tone (12 kHz) of amplitude 0.7 each, both cosines: their peaks coincide every millisecond
    tone = 0.7 * np.cos(2 * np.pi * 1000.0 / rate * t) + 0.7 * np.cos(2 * np.pi * 12000.0 / rate * t)
    s = as_s16(np.stack([tone, -tone, 0.5 * tone]))
    f = s.astype(np.float32) / np.float32(32768.0)
    y = hops_of(np.stack([0.7 * np.cos(2 * np.pi * 1000.0 / 16000.0 * np.arange(hops * 256))] * B).astype(np.float32) * np.array([[1], [-1], [0.5]], np.float32), 256)
    res = {}
    for dtype, x in (("float32", f), ("int16", s)):
        eng = engine(rate, dtype, 1.0)
        out = []
        for xh, yh in zip(hops_of(x, S), y):      # the halves: what is quantised does not depend on what a model makes of the tones
            eng.pcm_decode_hop(dev(xh))
            out.append(eng.pcm_encode_hop(dev(yh)))
        res[dtype] = torch.cat(out, dim=1).cpu().numpy()
        whole = np.concatenate([eng.enhance_hop_pcm(dev(xh)).cpu().numpy() for xh in hops_of(x, S)], axis=1)      # and the entry itself
        res[dtype + " entry"] = whole
        eng.close()
    for tail in ("", " entry"):
        assert res["int16" + tail].dtype == np.int16
        assert np.array_equal(res["int16" + tail], as_s16(res["float32" + tail])), tail
    assert np.abs(res["float32"]).max() > 1.2, "the float result does not leave +-1: nothing saturates"
    assert res["int16"].max() == 32767 and res["int16"].min() == -32768


# ---- 9. refusals change nothing ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from nunet_amd.weights import synthetic_weights, write_blob
    for rate in (16000, 8000):
        x = hops_of(as_s16(0.5 * designed(rate, B, 3, seed=290)), hop_len(rate))
        eng, twin = engine(rate, "int16", None), engine(rate, "int16", None)
        assert torch.equal(eng.enhance_hop_pcm(dev(x[0])), twin.enhance_hop_pcm(dev(x[0])))
        with pytest.raises(ValueError, match="nutls_set_pcm_upper_band"):
            eng.set_pcm_upper_band(0.5)
        assert eng.pcm_upper_band == 0.0
        eng.set_pcm_upper_band(0.0)      # (0 is what the handle has: allowed at every rate)
        for k in (1, 2):
            assert torch.equal(eng.enhance_hop_pcm(dev(x[k])), twin.enhance_hop_pcm(dev(x[k]))), (rate, k)
        eng.close(); twin.close()
    rate = 48000
    x = hops_of(as_s16(0.5 * designed(rate, B, 5, seed=291)), hop_len(rate))
    eng, twin = engine(rate, "int16", 0.5), engine(rate, "int16", 0.5)
    assert torch.equal(eng.enhance_hop_pcm(dev(x[0])), twin.enhance_hop_pcm(dev(x[0])))
    for k, bad in enumerate((-0.1, 1.5, float("nan")), start=1):
        with pytest.raises(ValueError, match="nutls_set_pcm_upper_band"):
            eng.set_pcm_upper_band(bad)
        assert eng.pcm_upper_band == 0.5
        assert torch.equal(eng.enhance_hop_pcm(dev(x[k])), twin.enhance_hop_pcm(dev(x[k]))), bad
    eng.close(); twin.close()
    # a masked call on a handle that refuses masks (baseline variant), with the gain on: refused before the decode
    blob = write_blob(synthetic_weights("baseline", seed=4321, bias_std=0.1, affine_jitter=0.1), int8_convs=True)
    base, twin = (NutlsEngine(blob, batch=B, variant="baseline") for _ in range(2))
    for e in (base, twin):
        e.set_pcm_format(rate, "int16")
        e.set_pcm_upper_band(1.0)
    assert torch.equal(base.enhance_hop_pcm(dev(x[0])), twin.enhance_hop_pcm(dev(x[0])))
    with pytest.raises(ValueError, match="baseline"):
        base.enhance_hop_pcm(dev(x[1]), active=dev(np.array([1, 0, 1], np.uint8)))
    for k in (1, 2):
        assert torch.equal(base.enhance_hop_pcm(dev(x[k])), twin.enhance_hop_pcm(dev(x[k]))), k
    base.close(); twin.close()
