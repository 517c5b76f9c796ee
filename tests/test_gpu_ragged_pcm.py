"""``-m gpu``: ragged blocks in the callers' format (include/nutls.h, "PCM gateway", the ``_pcm_ragged`` entries; csrc/pcm.hip) and the
corpus scheduler on top of them (``NutlsOffline.enhance_many(waves, rate=...)``), with ``NutlsOffline(max_frames=8, utterances=3)``.
The reference refuses anything but float samples at 16 kHz and enhances one recording at a time
(dnn_model/interpreter_proposed.py:203-370, 384-385), so the references here are
  - the library's own uniform entries for everything the contract promises bit for bit (torch.equal / np.array_equal): hops in front of a
    count, cuts of a stream, the entry against its three parts, the host entry against the device entry, int16 against float32;
  - ``scipy.signal.upfirdn`` in float64 with the taps of ``nutls_pcm_filter`` for the decode half, at the bound of
    tests/test_gpu_pcm_format.py: ``(n_taps + 3) * 2**-24 * upfirdn(|p|, |x|)`` per sample (one chain of at most n_taps fp32 FMAs, each one
    rounding of relative size 2**-24 on a partial sum that never exceeds sum |p||x|, plus the final scaling and the float32 result);
  - ``enhance_wave`` of a one-utterance handle for ``enhance_many``, at the bound tests/test_gpu_ragged_enhance.py uses between handle
    shapes (relative RMS < 1e-5).
Signals as in tests/test_gpu_pcm_format.py (``designed`` / ``as_s16``)."""
import ctypes

import numpy as np
import pytest
import torch      # (before the first handle: torch must bring up the HIP runtime it ships with itself)
from scipy import signal

from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner

pytestmark = pytest.mark.gpu

U, W = 3, 8
U2 = 2.0 ** -24
# per-utterance counts of consecutive calls: k = 0, 1 and n_hops; utterance 1 is held in two (then three) consecutive calls, utterance 2 in the
# first, utterance 0 in the last; every utterance has taken 8 hops at the end
SCHEDULE = ((3, 8, 0), (1, 0, 5), (4, 0, 1), (0, 0, 2))
FORMATS = [(rate, dtype) for rate in (8000, 32000, 48000) for dtype in ("int16", "float32")]


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


def reference_decode(p, x, rate):
    """float64 result and per-sample bound of the decode half on the rows of x."""
    q = ratio(rate)
    p64 = p.astype(np.float64)
    reduce = rate > 16000
    up, down = (1, q) if reduce else (q, 1)
    n_out = x.shape[1] // q if reduce else x.shape[1] * q
    want = np.stack([signal.upfirdn(p64 if reduce else q * p64, r.astype(np.float64), up, down)[:n_out] for r in x])
    mag = np.stack([signal.upfirdn(np.abs(p64), np.abs(r.astype(np.float64)), up, down)[:n_out] for r in x])
    return want, (len(p) + 3) * U2 * mag


def signal_in(rate, dtype, hops, seed):
    x = designed(rate, U, hops, seed)
    return as_s16(x) if dtype == "int16" else x


def behind(dtype, shape):
    """What the rows behind a count hold: NaN, or the int16 0x7FFF."""
    return np.full(shape, np.nan, np.float32) if np.dtype(dtype) == np.float32 else np.full(shape, 0x7FFF, np.int16)


def block_of(x, first, counts, unit):
    """[U, W * unit]: counts[u] hops of row u of x from hop first[u], the rest `behind`."""
    blk = behind(x.dtype, (U, W * unit))
    for u, k in enumerate(counts):
        blk[u, :k * unit] = x[u, first[u] * unit:(first[u] + k) * unit]
    return blk


def counts_as(i, counts):
    """The three kinds of ``hops=`` in turn: a list, an int64 array, an int32 CUDA tensor."""
    return (list(counts), np.array(counts), torch.tensor(counts, dtype=torch.int32, device="cuda"))[i % 3]


def same_bits(a, b):
    word = torch.int32 if a.dtype == torch.float32 else a.dtype
    return a.dtype == b.dtype and torch.equal(a.view(word), b.view(word))


def all_zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint8).any()


@pytest.fixture(scope="module")
def off():
    h = NutlsOffline(max_frames=W, utterances=U)
    yield h
    h.close()


@pytest.fixture(scope="module")
def twin():
    h = NutlsOffline(max_frames=W, utterances=U)
    yield h
    h.close()


@pytest.fixture(scope="module")
def solo():
    h = NutlsOffline(max_frames=W)
    yield h
    h.close()


def fresh(rate, dtype, *handles):
    for h in handles:
        h.reset()
        h.set_pcm_format(rate, dtype)      # (restarts every resampler history)


def ragged_halves(off, x, w, rate, schedule, clamp=None):
    """Decode x [U, hops * S] and encode w [U, hops * 256] through ragged calls of `schedule`; checks the rows behind the counts and the
    input tensors on the way.  clamp: the counts the device is GIVEN in place of the last call's (they must clamp to the schedule's).
    Returns per utterance the concatenated real hops of both halves."""
    S = hop_len(rate)
    first = [0] * U
    dec, enc = [[] for _ in range(U)], [[] for _ in range(U)]
    for i, counts in enumerate(schedule):
        dx, dw = dev(block_of(x, first, counts, S)), dev(block_of(w, first, counts, 256))
        keep_x, keep_w = dx.clone(), dw.clone()
        given = counts_as(i, counts)
        if clamp is not None and i == len(schedule) - 1:
            given = torch.tensor(clamp, dtype=torch.int32, device="cuda")
        d = off.pcm_decode_block_device(dx, hops=given)
        e = off.pcm_encode_block_device(dw, hops=given)
        assert d.shape == (U, W * 256) and d.dtype == torch.float32 and e.shape == (U, W * S) and e.dtype == dx.dtype
        assert same_bits(dx, keep_x) and same_bits(dw, keep_w), "call %d wrote its input" % i
        d, e = d.cpu().numpy(), e.cpu().numpy()
        for u, k in enumerate(counts):
            assert all_zero_bits(d[u, k * 256:]) and all_zero_bits(e[u, k * S:]), (i, u)
            dec[u].append(d[u, :k * 256])
            enc[u].append(e[u, :k * S])
            first[u] += k
    return [np.concatenate(r) for r in dec], [np.concatenate(r) for r in enc], first


# ---- 1. the halves are the uniform halves, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,dtype", FORMATS)
def test_ragged_halves_are_the_uniform_halves_bit_for_bit(off, twin, rate, dtype):
    S = hop_len(rate)
    x = signal_in(rate, dtype, 2 * W, seed=rate // 1000)
    w = designed(16000, U, 2 * W, seed=7, out_of_band=False)
    fresh(rate, dtype, off, twin)
    want_dec = torch.cat([twin.pcm_decode_block_device(dev(x[:, a * S:(a + W) * S])) for a in (0, W)], dim=1).cpu().numpy()
    want_enc = torch.cat([twin.pcm_encode_block_device(dev(w[:, a * 256:(a + W) * 256])) for a in (0, W)], dim=1).cpu().numpy()
    assert np.abs(want_dec).max() > 0.1 and np.abs(want_enc.astype(np.float64)).max() > (0.1 if dtype == "float32" else 3000)
    # the schedule, then device counts of -3 and 99: they behave as 0 and n_hops
    schedule = SCHEDULE + ((0, W, 2),)
    dec, enc, taken = ragged_halves(off, x, w, rate, schedule, clamp=(-3, 99, 2))
    assert taken == [8, 16, 10]
    for u in range(U):
        assert np.array_equal(dec[u].view(np.uint32), want_dec[u, :taken[u] * 256].view(np.uint32)), u
        assert np.array_equal(enc[u], want_enc[u, :taken[u] * S]) and enc[u].dtype == want_enc.dtype, u


# ---- 2. against float64 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 48000])
def test_ragged_decode_against_float64(off, rate):
    S = hop_len(rate)
    x = designed(rate, U, W, seed=20 + ratio(rate))
    w = np.zeros((U, W * 256), np.float32)
    fresh(rate, "float32", off)
    dec, _, taken = ragged_halves(off, x, w, rate, SCHEDULE)
    assert taken == [W] * U
    want, bound = reference_decode(runner.pcm_filter(rate), x, rate)
    err = np.abs(np.stack(dec).astype(np.float64) - want)
    print("ragged decode at %d Hz: worst error %.3g, worst error / bound %.3f" % (rate, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), float((err - bound).max())


# ---- 3. 16 kHz --------------------------------------------------------------------------------------------------------------------------------
def test_at_16k_int16_the_rows_behind_a_count_are_zeros(off, twin):
    counts = (3, W, 0)
    x = as_s16(designed(16000, U, W, seed=30))
    w = designed(16000, U, W, seed=31)
    fresh(16000, "int16", off, twin)
    want_dec = twin.pcm_decode_block_device(dev(x)).cpu().numpy()
    want_enc = twin.pcm_encode_block_device(dev(w)).cpu().numpy()
    dec, enc, _ = ragged_halves(off, x, w, 16000, (counts,))
    for u, k in enumerate(counts):
        assert np.array_equal(dec[u], want_dec[u, :k * 256]) and np.array_equal(enc[u], want_enc[u, :k * 256]), u
    assert np.array_equal(want_dec, x.astype(np.float32) / np.float32(32768.0)) and want_enc.dtype == np.int16 and want_enc.any()


def test_at_16k_float32_the_entry_is_the_ragged_float_entry(off, twin):
    x = 0.5 * designed(16000, U, 2 * W, seed=32)
    fresh(16000, "float32", off, twin)
    first = [0] * U
    for i, counts in enumerate(SCHEDULE):
        blk = dev(block_of(x, first, counts, 256))
        got = off.enhance_block_pcm_device(blk, hops=counts_as(i, counts))
        want = twin.enhance_block_device(blk.clone(), hops=list(counts))
        assert same_bits(got, want), i
        first = [a + k for a, k in zip(first, counts)]
    assert got.cpu().numpy().any()


# ---- 4. the whole entry is its three parts ----------------------------------------------------------------------------------------------------
def host_entry(off, blk, counts, dc=0):
    out = np.empty_like(blk)
    cnt = np.asarray(counts, np.int32)
    n = blk.shape[1] // off.pcm_hop_samples
    runner._check(off._lib, off._lib.nutls_enhance_block_pcm_ragged_host(off._h, blk.ctypes.data, out.ctypes.data, n,
                                                                         cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), dc))
    return out


@pytest.mark.parametrize("rate,dtype", [(8000, "int16"), (48000, "float32")])
def test_the_ragged_pcm_entry_is_decode_enhance_encode(off, twin, rate, dtype):
    S = hop_len(rate)
    x = signal_in(rate, dtype, 2 * W, seed=40)
    if dtype == "float32":
        x = 0.5 * x
    fresh(rate, dtype, off, twin)
    first, blocks, results = [0] * U, [], []
    for i, counts in enumerate(SCHEDULE):
        blk = block_of(x, first, counts, S)
        c = counts_as(i, counts)
        got = off.enhance_block_pcm_device(dev(blk), hops=c)
        want = twin.pcm_encode_block_device(twin.enhance_block_device(twin.pcm_decode_block_device(dev(blk), hops=c), hops=c), hops=c)
        assert got.dtype == getattr(torch, dtype) and same_bits(got, want), i
        for u, k in enumerate(counts):
            assert all_zero_bits(got[u, k * S:].cpu().numpy()), (i, u)
        blocks.append(blk)
        results.append(got.cpu().numpy())
        first = [a + k for a, k in zip(first, counts)]
    assert results[0].any() and results[-1].any()
    # the host entry, from reset, against the device entry
    fresh(rate, dtype, off)
    for i, counts in enumerate(SCHEDULE):
        assert np.array_equal(host_entry(off, blocks[i], counts).view(np.uint8), results[i].view(np.uint8)), i
    # null counts: the uniform entry
    fresh(rate, dtype, off, twin)
    full = dev(x[:, :W * S])
    out = torch.empty_like(full)
    stream = torch.cuda.current_stream().cuda_stream
    runner._check(off._lib, off._lib.nutls_enhance_block_pcm_ragged(off._h, full.data_ptr(), out.data_ptr(), W, None, 0, stream))
    assert same_bits(out, twin.enhance_block_pcm_device(full))
    assert same_bits(off.enhance_block_pcm_device(dev(x[:, W * S:]), hops=None), twin.enhance_block_pcm_device(dev(x[:, W * S:])))
    assert np.array_equal(host_entry_null(off, x[:, :W * S]), host_entry_null(twin, x[:, :W * S], uniform=True))


def host_entry_null(off, blk, uniform=False):
    blk = np.ascontiguousarray(blk)
    if uniform:
        return off.enhance_block_pcm_host(blk)
    out = np.empty_like(blk)
    runner._check(off._lib, off._lib.nutls_enhance_block_pcm_ragged_host(off._h, blk.ctypes.data, out.ctypes.data, W, None, 0))
    return out


# ---- 5. a cut does not matter, with the model in ----------------------------------------------------------------------------------------------
def test_the_cut_of_a_recording_into_ragged_calls_does_not_matter(off, twin):
    rate, dtype, hops = 48000, "int16", 10
    S = hop_len(rate)
    x = as_s16(0.5 * designed(rate, U, hops, seed=50))
    cuts = (((8, 3, 0), (2, 7, 8), (0, 0, 2)), ((1, 8, 5), (8, 0, 5), (1, 2, 0)))
    fresh(rate, dtype, off, twin)
    whole = []
    for h, schedule in zip((off, twin), cuts):
        first, rows = [0] * U, [[] for _ in range(U)]
        for counts in schedule:
            got = h.enhance_block_pcm_device(dev(block_of(x, first, counts, S)), hops=list(counts)).cpu().numpy()
            for u, k in enumerate(counts):
                rows[u].append(got[u, :k * S])
                first[u] += k
        assert first == [hops] * U
        whole.append(np.stack([np.concatenate(r) for r in rows]))
    assert whole[0].dtype == np.int16 and whole[0][:, 2 * S:].any(axis=1).all()
    assert np.array_equal(whole[0], whole[1])


# ---- 6. enhance_many(rate=...) ----------------------------------------------------------------------------------------------------------------
def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


@pytest.mark.parametrize("rate", [8000, 48000])
def test_enhance_many_in_the_callers_format(off, solo, rate):
    S = hop_len(rate)
    lengths = [S // 2 + 3, 20 * S + 11, 3 * S + 1, 9 * S - 5, 13 * S + S // 3, S + 7, 6 * S + 101]      # less than a hop .. about 20 hops
    source = as_s16(0.5 * designed(rate, 1, 21 * len(lengths), seed=60 + ratio(rate)))[0]
    xs = [source[21 * S * i:21 * S * i + n].copy() for i, n in enumerate(lengths)]
    xf = [x.astype(np.float32) / np.float32(32768.0) for x in xs]
    assert len(xs) == 7 and all(n % S for n in lengths)
    yf = off.enhance_many(xf, rate=rate)
    assert off.pcm_rate == rate and off.pcm_dtype == "float32"
    for i, (x, y) in enumerate(zip(xf, yf)):
        assert y.shape == x.shape and y.dtype == np.float32, i
        solo.reset()
        want = solo.enhance_wave(x, rate)
        if not want.any():
            assert not y.any(), i
            continue
        e = rel_rms(y, want)
        print("%d Hz, recording %d (%d samples): relative rms vs a one-utterance handle %.3e (bound 1e-5)" % (rate, i, len(x), e))
        assert e < 1e-5, i
    ys = off.enhance_many(xs, rate=rate)
    assert off.pcm_dtype == "int16"
    for i, (x, y, f) in enumerate(zip(xs, ys, yf)):
        assert y.shape == x.shape and y.dtype == np.int16, i
        assert np.array_equal(y, np.clip(np.rint(f * np.float32(32768.0)), -32768, 32767).astype(np.int16)), i
    assert any(y.any() for y in ys)
    for a, b in zip(ys, off.enhance_many(xs, rate=rate)):
        assert np.array_equal(a, b)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_streaming_handles_and_bad_host_counts_are_refused(off, twin):
    eng = NutlsEngine(batch=2)
    lib = eng._lib
    d = torch.zeros(2, 768, device="cuda")
    dc = torch.ones(2, dtype=torch.int32, device="cuda")
    hbuf = np.zeros((2, 768), np.float32)
    ip = np.ones(2, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    p, c = d.data_ptr(), dc.data_ptr()
    calls = {
        "nutls_enhance_block_pcm_ragged": lambda: lib.nutls_enhance_block_pcm_ragged(eng._h, p, p, 1, c, 0, None),
        "nutls_enhance_block_pcm_ragged_host": lambda: lib.nutls_enhance_block_pcm_ragged_host(eng._h, hbuf.ctypes.data, hbuf.ctypes.data, 1, ip, 0),
        "nutls_pcm_decode_block_ragged": lambda: lib.nutls_pcm_decode_block_ragged(eng._h, p, p, 1, c, None),
        "nutls_pcm_encode_block_ragged": lambda: lib.nutls_pcm_encode_block_ragged(eng._h, p, p, 1, c, None),
    }
    for fmt in ((16000, "float32"), (8000, "int16")):
        eng.set_pcm_format(*fmt)
        for name, call in calls.items():
            with pytest.raises(ValueError, match="offline handle"):
                runner._check(lib, call())
    eng.close()
    # host counts outside 0 .. n_hops (and a bad dc_mode): refused, and the handle goes on as if nothing had happened
    rate, dtype = 8000, "int16"
    S = hop_len(rate)
    x = signal_in(rate, dtype, 2 * W, seed=70)
    fresh(rate, dtype, off, twin)
    counts = (5, W, 2)
    blk = block_of(x, [0] * U, counts, S)
    assert np.array_equal(host_entry(off, blk, counts), host_entry(twin, blk, counts))      # (histories and state are no longer zeros)
    for bad in ((-1, 1, 1), (1, W + 1, 0)):
        with pytest.raises(ValueError, match="outside"):
            host_entry(off, blk, bad)
        with pytest.raises(ValueError):
            off.enhance_block_pcm_device(dev(blk), hops=list(bad))
    with pytest.raises(ValueError, match="dc_mode"):
        host_entry(off, blk, counts, dc=7)
    nxt = block_of(x, list(counts), (3, 0, W), S)
    got, want = host_entry(off, nxt, (3, 0, W)), host_entry(twin, nxt, (3, 0, W))
    assert np.array_equal(got, want) and got.any()
