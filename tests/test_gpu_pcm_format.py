"""GPU checks of the PCM gateway (include/nutls.h, "PCM gateway"; csrc/pcm.hip): int16 and 8 / 32 / 48 kHz audio in and out of the
waveform entries, converted on the device.  The reference refuses anything but float samples at 16 kHz
(dnn_model/interpreter_proposed.py:384-385), so the references here are
  - ``scipy.signal.upfirdn`` in float64 with the taps of ``nutls_pcm_filter`` for the two conversion halves.  Per-sample bound:
    ``(n_taps + 3) * 2**-24 * upfirdn(|p|, |x|)`` -- an output sample is one chain of at most n_taps fp32 FMAs (one rounding of relative
    size 2**-24 each, on a partial sum that never exceeds sum |p||x|), plus the final scaling and the float32 conversion of the result;
  - the library itself for everything the contract promises bit for bit (np.array_equal / torch.equal): pass-through at 16 kHz float32,
    int16 against float32, composition of the halves around ``enhance_hop``, masks, reset, cuts of a block, hop entries against block entries.
Shapes: 3 streams, at most 12 hops, offline handles of 8 frames with 2 utterances."""
import numpy as np
import pytest
import torch
from scipy import signal

from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner

pytestmark = pytest.mark.gpu
B = 3
K = 24
U2 = 2.0 ** -24


def ratio(rate):
    return max(rate, 16000) // min(rate, 16000)


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


def hops_of(x, rate):
    S = hop_len(rate)
    return [np.ascontiguousarray(x[:, k * S:(k + 1) * S]) for k in range(x.shape[1] // S)]


def reference_halves(p, x, rate, decode):
    """float64 result and per-sample bound of one conversion half on the concatenated rows of x."""
    q = ratio(rate)
    p64 = p.astype(np.float64)
    reduce = (rate > 16000) == decode
    up, down = (1, q) if reduce else (q, 1)
    n_out = x.shape[1] // q if reduce else x.shape[1] * q
    want = np.stack([signal.upfirdn(p64 if reduce else q * p64, r.astype(np.float64), up, down)[:n_out] for r in x])
    mag = np.stack([signal.upfirdn(np.abs(p64), np.abs(r.astype(np.float64)), up, down)[:n_out] for r in x])
    return want, (len(p) + 3) * U2 * mag


# ---- 5. pass-through ----------------------------------------------------------------------------------------------------------------------
def test_at_16k_float32_the_pcm_entry_is_the_plain_entry():
    x = designed(16000, B, 6, seed=5)
    a, b = NutlsEngine(batch=B), NutlsEngine(batch=B)
    before = a.launches_per_hop
    a.set_pcm_format(16000, "float32")
    assert a.pcm_hop_samples == 256 and a.pcm_delay_samples == 0 and a.launches_per_hop == before == b.launches_per_hop
    for k, h in enumerate(hops_of(x, 16000)):
        if k % 2:      # the host entry
            assert np.array_equal(a.enhance_hop_pcm(h), b.enhance_hop(h)), k
        else:
            assert torch.equal(a.enhance_hop_pcm(dev(h)), b.enhance_hop(dev(h))), k
    assert a.launches_per_hop == before
    a.close(); b.close()


# ---- 6. the halves against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_halves_against_float64(rate):
    hops, q = 10, ratio(rate)
    x = designed(rate, B, hops, seed=60 + q)
    if rate > 16000:      # row 1: the out-of-band tone alone
        t = np.arange(x.shape[1], dtype=np.float64)
        x[1] = (0.5 * np.sin(2 * np.pi * 1.4 * 8000.0 / rate * t)).astype(np.float32)
    p = runner.pcm_filter(rate)
    eng = NutlsEngine(batch=B)
    eng.set_pcm_format(rate, "float32")
    assert eng.pcm_hop_samples == hop_len(rate) and eng.pcm_delay_samples == 2 * K * max(1, rate // 16000)
    dec = [eng.pcm_decode_hop(dev(h)) for h in hops_of(x, rate)]
    enc = [eng.pcm_encode_hop(d) for d in dec]
    got_dec = torch.cat(dec, dim=1).cpu().numpy()
    got_enc = torch.cat(enc, dim=1).cpu().numpy()
    eng.close()
    assert got_dec.shape == (B, hops * 256) and got_enc.shape == x.shape and got_enc.dtype == np.float32
    for name, got, (want, bound) in (("decode", got_dec, reference_halves(p, x, rate, True)),
                                     ("encode", got_enc, reference_halves(p, got_dec, rate, False))):
        err = np.abs(got.astype(np.float64) - want)
        print("%s at %d Hz: worst error %.3g, worst error / bound %.3f" % (name, rate, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (name, float((err - bound).max()))
    if rate > 16000:
        settled = got_dec[1, 2 * K + 8:].astype(np.float64)
        down_db = 20 * np.log10(np.sqrt(np.mean(settled ** 2)) / (0.5 / np.sqrt(2)))
        print("out-of-band tone at %d Hz: %.1f dB" % (rate, down_db))
        assert down_db <= -80.0


# ---- 7. int16 is exact ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 16000, 32000, 48000])
def test_int16_is_exact(rate):
    hops = 5
    s = as_s16(designed(rate, B, hops, seed=70))
    f = (s.astype(np.float32) / np.float32(32768.0))
    loud = (2.0 * designed(16000, B, hops, seed=71, out_of_band=False)).astype(np.float32)      # 16 kHz floats for the encode half
    loud[0], loud[1] = 1.5, -1.5
    eng = NutlsEngine(batch=B)
    res = {}
    for dtype, x in (("float32", f), ("int16", s)):
        eng.set_pcm_format(rate, dtype)      # (restarts every history)
        dec = torch.cat([eng.pcm_decode_hop(dev(h)) for h in hops_of(x, rate)], dim=1).cpu().numpy()
        enc = torch.cat([eng.pcm_encode_hop(dev(h)) for h in hops_of(loud, 16000)], dim=1).cpu().numpy()
        res[dtype] = (dec, enc)
    eng.close()
    assert np.array_equal(res["int16"][0], res["float32"][0]), "decoded floats differ between int16 and float32 input"
    enc_f, enc_s = res["float32"][1], res["int16"][1]
    assert enc_s.dtype == np.int16 and enc_s.shape == enc_f.shape == (B, hops * hop_len(rate))
    assert np.abs(enc_f).max() > 1.4, "the float result does not leave +-1: nothing saturates"
    assert np.array_equal(enc_s, np.clip(np.rint(enc_f * np.float32(32768.0)), -32768, 32767).astype(np.int16))
    assert enc_s[0].max() == 32767 and enc_s[1].min() == -32768
    assert np.all(enc_s[0, -hop_len(rate):] == 32767) and np.all(enc_s[1, -hop_len(rate):] == -32768)


# ---- 8. composition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", [False, True])
@pytest.mark.parametrize("rate", [48000, 8000])
def test_the_pcm_hop_is_decode_enhance_encode(rate, fusion):
    x = as_s16(0.5 * designed(rate, B, 4, seed=80))
    one, twin = NutlsEngine(batch=B, hop_fusion=fusion), NutlsEngine(batch=B, hop_fusion=fusion)
    assert one.launches_per_hop == (1 if fusion else 3)
    for e in (one, twin):
        e.set_pcm_format(rate, "int16")
    for k, h in enumerate(hops_of(x, rate)):
        got = one.enhance_hop_pcm(dev(h))
        want = twin.pcm_encode_hop(twin.enhance_hop(twin.pcm_decode_hop(dev(h))))
        assert got.dtype == torch.int16 and torch.equal(got, want), k
        assert got.cpu().numpy().any() or k == 0
    assert one.launches_per_hop == (1 if fusion else 3)
    one.close(); twin.close()


# ---- 9. masks ---------------------------------------------------------------------------------------------------------------------------------
def test_a_held_stream_keeps_its_resampler_state():
    rate, ticks = 48000, 5
    x = 0.5 * designed(rate, B, ticks, seed=90)
    hops = hops_of(x, rate)
    masks = np.ones((ticks, B), np.uint8)
    masks[1, 1] = masks[2, 1] = 0
    ref = NutlsEngine(batch=B)
    ref.set_pcm_format(rate, "float32")
    want = [ref.enhance_hop_pcm(dev(h)).cpu().numpy() for h in hops]      # lockstep: every stream takes its k-th hop at step k
    ref.close()
    for host in (False, True):
        eng = NutlsEngine(batch=B)
        eng.set_pcm_format(rate, "float32")
        taken = 0
        for t in range(ticks):
            feed = hops[t].copy()
            if masks[t, 1]:
                feed[1] = hops[taken][1]
            else:
                feed[1] = np.nan      # a held row may hold anything
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
        assert taken == 3
        eng.close()


# ---- 10. reset and format switch --------------------------------------------------------------------------------------------------------------
def test_reset_and_format_switch_restart_the_conversion():
    rate = 32000
    x = 0.5 * designed(rate, B, 6, seed=100)
    hops = hops_of(x, rate)
    a, whole, fresh = NutlsEngine(batch=B), NutlsEngine(batch=B), NutlsEngine(batch=B)
    for e in (a, whole, fresh):
        e.set_pcm_format(rate, "float32")
    first_dec = a.pcm_decode_hop(dev(hops[0]))      # from a zero history
    first_enc = a.pcm_encode_hop(first_dec)
    assert not torch.equal(a.pcm_decode_hop(dev(hops[0])), first_dec), "the history has no effect: the checks below would show nothing"
    a.set_pcm_format(rate, "float32")
    assert torch.equal(a.pcm_decode_hop(dev(hops[0])), first_dec) and torch.equal(a.pcm_encode_hop(first_dec), first_enc)
    a.set_pcm_format(rate, "float32")
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
    with pytest.raises(ValueError):
        a.set_pcm_format(44100, "float32")
    assert a.pcm_hop_samples == 512
    for e in (a, whole, fresh):
        e.close()


# ---- 11. block mode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 8000])
def test_blocks_do_not_depend_on_the_cut_and_equal_the_hops(rate):
    U, hops, S = 2, 8, hop_len(rate)
    x = as_s16(0.5 * designed(rate, U, hops, seed=110))
    off, twin = NutlsOffline(max_frames=8, utterances=U), NutlsOffline(max_frames=8, utterances=U)
    for o in (off, twin):
        o.set_pcm_format(rate, "int16")
    whole_dec = off.pcm_decode_block_device(dev(x))
    whole_enc = off.pcm_encode_block_device(whole_dec)
    assert whole_dec.shape == (U, hops * 256) and whole_enc.shape == (U, hops * S) and whole_enc.dtype == torch.int16
    off.reset()
    dec, enc, at = [], [], 0
    for n in (1, 5, 2):
        dec.append(off.pcm_decode_block_device(dev(x[:, at * S:(at + n) * S])))
        enc.append(off.pcm_encode_block_device(whole_dec[:, at * 256:(at + n) * 256].contiguous()))
        at += n
    assert torch.equal(torch.cat(dec, dim=1), whole_dec) and torch.equal(torch.cat(enc, dim=1), whole_enc)
    stream = NutlsEngine(batch=U)
    stream.set_pcm_format(rate, "int16")
    hop_dec = [stream.pcm_decode_hop(dev(h)) for h in hops_of(x, rate)]
    hop_enc = [stream.pcm_encode_hop(d) for d in hop_dec]
    assert torch.equal(torch.cat(hop_dec, dim=1), whole_dec) and torch.equal(torch.cat(hop_enc, dim=1), whole_enc)
    with pytest.raises(ValueError):
        runner._check(stream._lib, stream._lib.nutls_enhance_block_pcm(stream._h, dev(x).data_ptr(), dev(x).data_ptr(), 1, 0, None))
    stream.close()
    # the whole entry against its three parts on a twin handle, then the host entry against the device entry
    off.reset()
    got = off.enhance_block_pcm_device(dev(x))
    want = twin.pcm_encode_block_device(twin.enhance_block_device(twin.pcm_decode_block_device(dev(x))))
    assert torch.equal(got, want) and got.cpu().numpy().any()
    off.reset()
    assert np.array_equal(off.enhance_block_pcm_host(x), got.cpu().numpy())
    with pytest.raises(ValueError):
        runner._check(off._lib, off._lib.nutls_enhance_hop_pcm(off._h, dev(x).data_ptr(), dev(x).data_ptr(), 0, None))
    off.close(); twin.close()


# ---- 12. enhance_wave -------------------------------------------------------------------------------------------------------------------------
def test_enhance_wave_lines_up_with_its_input():
    rate, U = 48000, 2
    n = 6 * 768 + 333      # not a multiple of a hop
    amp = 12000.0
    t = np.arange(n, dtype=np.float64)
    x = np.stack([np.rint(amp * np.sin(2 * np.pi * 1000.0 / rate * t + ph)) for ph in (0.0, 1.0)]).astype(np.int16)
    off = NutlsOffline(max_frames=8, utterances=U)
    off.set_pcm_format(rate, "int16")
    # the alignment logic of enhance_wave with the model replaced by decode -> encode: the lag is then the resamplers' alone
    out = off._wave_through_blocks(x, off.pcm_delay_samples, lambda blk: off.pcm_encode_block_device(off.pcm_decode_block_device(dev(blk))).cpu().numpy())
    assert out.shape == x.shape and out.dtype == np.int16
    basis = np.stack([np.sin(2 * np.pi * 1000.0 / rate * t), np.cos(2 * np.pi * 1000.0 / rate * t)], axis=1)[480:-480]
    for u in range(U):
        xc = np.correlate(out[u].astype(np.float64), x[u].astype(np.float64), mode="full")
        assert int(np.argmax(xc)) - (n - 1) == 0, "row %d is off by %d samples" % (u, int(np.argmax(xc)) - (n - 1))
        a_in = np.hypot(*np.linalg.lstsq(basis, x[u, 480:-480].astype(np.float64), rcond=None)[0])
        a_out = np.hypot(*np.linalg.lstsq(basis, out[u, 480:-480].astype(np.float64), rcond=None)[0])
        print("row %d: amplitude in %.2f, out %.2f" % (u, a_in, a_out))
        assert abs(a_out - a_in) <= a_in * (10 ** (0.01 / 20) - 1) + 1.0
    # the public method: same shape, dtype and length, whatever the model makes of a tone
    y = off.enhance_wave(x, rate)
    assert y.shape == x.shape and y.dtype == np.int16
    y1 = NutlsOffline(max_frames=8).enhance_wave(x[0].astype(np.float32) / np.float32(32768.0), rate)
    assert y1.shape == (n,) and y1.dtype == np.float32 and np.isfinite(y1).all()
    off.close()
