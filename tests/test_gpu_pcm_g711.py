"""GPU checks of G.711 in the PCM gateway (include/nutls.h, "PCM gateway", G.711; csrc/pcm.hip): mu-law and A-law bytes at 8 kHz in and out
of every ``_pcm`` entry.  The companding is an exact bit rule, so everything here is bit equality (``np.array_equal`` / ``torch.equal``):
  - decode: a companded handle fed codes ``c`` against an int16 handle fed ``expand(c)``;
  - encode: the codes of a companded handle against ``compress`` of what an int16 handle returns for the same floats;
with ``expand`` / ``compress`` the numpy statement of the header's rule (tests/g711_reference.py), which test_pcm_g711_abi.py holds against
the library's host helpers and ``audioop``.  No reference counterpart: the reference takes float samples at 16 kHz only
(dnn_model/interpreter_proposed.py:384-385).
Shapes: streaming handles of 4 streams, offline handles of 2 utterances x 8 hops; the encode test alone takes 8 utterances x 64 hops (it
runs the halves only, no model), so that a ramp through the whole int16 range fits.
Two readings of the checks' wording, where it cannot be met as written:
  - the decode test feeds 8 hops, not 6: 256 codes at 16 byte positions are 4096 bytes, 4 streams x 6 hops x 128 bytes are 3072;
  - "blocks equal the streaming hops" is asserted for the two conversion halves, which the contract promises bit for bit between hop and
    block entries; the model path of an offline handle equals the streaming one to rounding only (test_gpu_enhance_block.py), for every
    format, so the whole block entry is held against the int16 block entry instead."""
import ctypes

import numpy as np
import pytest
import torch

import g711_reference as G
from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner

pytestmark = pytest.mark.gpu
B = 4
S = 128      # samples (bytes) of a hop at 8 kHz
CODECS = G.CODECS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def speech_like(rows, hops, seed):
    """[rows, hops * 128] int16: a tone, seeded noise and a slow envelope -- every segment of the laws is visited."""
    rng = np.random.default_rng(seed)
    n = hops * S
    t = np.arange(n, dtype=np.float64)
    x = 0.45 * np.sin(2 * np.pi * 440.0 / 8000.0 * t[None, :] + rng.uniform(0, 6.28, (rows, 1))) * (0.02 + np.abs(np.sin(2 * np.pi * t[None, :] / 700.0)))
    x = x + 0.05 * rng.standard_normal((rows, n))
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


def codes_like(codec, rows, hops, seed):
    return G.compress(codec, speech_like(rows, hops, seed))


def hops_of(x):
    return [np.ascontiguousarray(x[:, k * S:(k + 1) * S]) for k in range(x.shape[1] // S)]


def engine(fmt, batch=B, **kw):
    e = NutlsEngine(batch=batch, **kw)
    e.set_pcm_format(8000, fmt)
    assert e.pcm_hop_samples == S and e.pcm_delay_samples == 48
    assert e.pcm_dtype == ("int16" if fmt == "int16" else "uint8") and e.pcm_codec == (None if fmt == "int16" else fmt)
    return e


def offline(fmt, utterances=2, max_frames=8):
    o = NutlsOffline(max_frames=max_frames, utterances=utterances)
    o.set_pcm_format(8000, fmt)
    assert o.pcm_hop_samples == S and o.pcm_delay_samples == 48
    return o


# ---- 1. decode ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
def test_decode_is_the_int16_decode_of_the_expanded_codes(codec):
    hops = 8
    perm = np.random.default_rng(1).permutation(256)
    i = np.arange(hops * B * S)                      # byte i of the feed, hop-major: lane load i // 16, position i % 16 in its 16 bytes
    feed = perm[(i // 16 + 37 * (i % 16)) % 256].astype(np.uint8).reshape(hops, B, S)
    for pos in range(16):                            # every code at every byte position of a lane's load
        assert len(set(feed.reshape(-1, 16)[:, pos].tolist())) == 256, pos
    table = G.expand(codec)
    comp, lin = engine(codec), engine("int16")
    for k in range(hops):
        got = comp.pcm_decode_hop(dev(feed[k]))
        want = lin.pcm_decode_hop(dev(table[feed[k]]))
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, 256) and torch.equal(got, want), k
        assert got.abs().max().item() > 0.1
    comp.close(); lin.close()


# ---- 2. encode ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded():
    """The encode half of ONE offline handle (8 utterances x 64 hops) in int16, mu-law and A-law on the same two blocks of 16 kHz floats:
    (a) a linear ramp from -1.1 to +1.1 across the concatenated rows; (b) row 0: NaN hops, then single +inf / -inf samples among zeros;
    row 1: a plateau of one hop at every int16 value next to a segment end of either law (the ramp of (a) advances 1.1 int16 steps per
    sample and so skips one value in eleven: in float64 it misses 124, -888, -32632 of mu-law's edges and 256, -8192 of A-law's); row 2:
    +-3.0; the other rows zeros."""
    U, H = 8, 64
    ramp = np.linspace(-1.1, 1.1, U * H * 256).astype(np.float32).reshape(U, H * 256)
    extra = np.zeros((U, H * 256), np.float32)
    extra[0, :4 * 256] = np.nan
    extra[0, 8 * 256 + 100], extra[0, 12 * 256 + 101] = np.inf, -np.inf
    edges = sorted(set(G.segment_edges("ulaw") + G.segment_edges("alaw")))
    assert len(edges) <= H
    for k, v in enumerate(edges):
        extra[1, k * 256:(k + 1) * 256] = np.float32(v / 32768.0)
    extra[2, :16 * 256], extra[2, 16 * 256:32 * 256] = 3.0, -3.0
    off = NutlsOffline(max_frames=H, utterances=U)
    res = {}
    for fmt in ("int16",) + CODECS:
        off.set_pcm_format(8000, fmt)      # (restarts every history)
        a = off.pcm_encode_block_device(dev(ramp)).cpu().numpy()
        off.reset()
        b = off.pcm_encode_block_device(dev(extra)).cpu().numpy()
        res[fmt] = np.concatenate([a, b], axis=0)
    off.close()
    return res, edges


@pytest.mark.parametrize("codec", CODECS)
def test_encode_is_the_compression_of_the_int16_encode(encoded, codec):
    res, edges = encoded
    lin, got = res["int16"], res[codec]
    assert lin.dtype == np.int16 and got.dtype == np.uint8 and got.shape == lin.shape == (16, 64 * S)
    # the condition on the input, on the int16 handle's output
    values = set(lin.ravel().tolist())
    produced = set(G.compress(codec, lin).ravel().tolist())
    print("%s: %d distinct int16 values, %d codes" % (codec, len(values), len(produced)))
    assert len(produced) == (255 if codec == "ulaw" else 256)
    missing = [v for v in G.segment_edges(codec) if v not in values]
    assert not missing, missing
    assert -32768 in values and 32767 in values
    # the check
    assert np.array_equal(got, G.compress(codec, lin))
    assert np.array_equal(got, runner.g711_compress(codec, lin))      # ... and the library's own statement of the rule
    # NaN -> 0 -> the silence code (row 0 of the second block, its first four hops less the filter's reach into the zeros behind them)
    assert np.all(lin[8, :4 * S - 48] == 0) and np.all(got[8, :4 * S - 48] == G.SILENCE[codec])
    assert np.all(got[8 + 3] == G.SILENCE[codec])                      # a zero row


# ---- 3. the whole hop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion,limit", [(False, None), (True, None), (False, 0.5)])
@pytest.mark.parametrize("codec", CODECS)
def test_the_whole_hop_is_the_int16_hop_between_expand_and_compress(codec, fusion, limit):
    x = codes_like(codec, B, 6, seed=30)
    table = G.expand(codec)
    comp, lin = engine(codec, hop_fusion=fusion), engine("int16", hop_fusion=fusion)
    assert comp.launches_per_hop == (1 if fusion else 3)
    if limit is not None:
        for e in (comp, lin):
            e.set_atten_limit(limit=[0.0, limit, 0.0, 0.0])
    outs = []
    for k, h in enumerate(hops_of(x)):
        buf = dev(h)
        got = comp.enhance_hop_pcm(buf, out=buf if k % 2 else None)      # odd hops in place: pcm_in == pcm_out
        want = lin.enhance_hop_pcm(dev(table[h])).cpu().numpy()
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), G.compress(codec, want)), k
        outs.append(got.cpu().numpy())
    assert np.any(np.concatenate(outs, axis=1) != G.SILENCE[codec])
    assert comp.launches_per_hop == (1 if fusion else 3)
    comp.close(); lin.close()


# ---- 4. masks -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
def test_masks_hold_a_stream_and_write_silence(codec):
    ticks = 5
    x = codes_like(codec, B, ticks + 2, seed=40)
    hops = hops_of(x)
    masks = np.ones((ticks, B), np.uint8)
    masks[1, 1] = masks[2, 1] = 0
    ref = engine(codec)
    want = [ref.enhance_hop_pcm(dev(h)).cpu().numpy() for h in hops[:ticks]]      # lockstep: every stream takes its k-th hop at step k
    runs = []
    for filler in (0x00, 0x55):      # what a held row's input holds has no effect
        eng = engine(codec)
        taken, outs = 0, []
        for t in range(ticks):
            feed = hops[t].copy()
            feed[1] = hops[taken][1] if masks[t, 1] else filler
            out = eng.enhance_hop_pcm(dev(feed), active=dev(masks[t])).cpu().numpy()
            assert np.array_equal(out[[0, 2, 3]], want[t][[0, 2, 3]]), (filler, t)
            if masks[t, 1]:      # ticks 0, 3, 4 return the bits of ticks 0, 1, 2
                assert np.array_equal(out[1], want[taken][1]), (filler, t, taken)
                taken += 1
            else:                # a held row: the silence code, not zero bytes
                assert np.all(out[1] == G.SILENCE[codec]), (filler, t)
            outs.append(out)
        assert taken == 3
        runs.append((eng, np.stack(outs)))
    assert np.array_equal(runs[0][1], runs[1][1])
    runs[1][0].close()
    # reset(1) restarts row 1 alone
    eng, fresh = runs[0][0], engine(codec)
    eng.reset(1)
    for k in (ticks, ticks + 1):
        got = eng.enhance_hop_pcm(dev(hops[k])).cpu().numpy()
        cont = ref.enhance_hop_pcm(dev(hops[k])).cpu().numpy()
        new = fresh.enhance_hop_pcm(dev(hops[k])).cpu().numpy()
        assert np.array_equal(got[[0, 2, 3]], cont[[0, 2, 3]]), k
        assert np.array_equal(got[1], new[1]) and not np.array_equal(got[1], cont[1]), k
    for e in (eng, fresh, ref):
        e.close()


# ---- 5. host entries ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
def test_the_host_entries_give_the_device_entrys_bytes(codec):
    x = codes_like(codec, B, 4, seed=50)
    masks = [None, np.array([1, 0, 1, 1], np.uint8), None, np.array([0, 1, 1, 1], np.uint8)]
    on_dev, pageable, pinned = engine(codec), engine(codec), engine(codec)
    pin_in = runner.host_alloc((B, S // 4)).view(np.uint8)
    pin_out = runner.host_alloc((B, S // 4)).view(np.uint8)
    assert pin_in.shape == (B, S) and pin_in.flags.c_contiguous
    for k, (h, m) in enumerate(zip(hops_of(x), masks)):
        want = on_dev.enhance_hop_pcm(dev(h), active=None if m is None else dev(m)).cpu().numpy()
        got = pageable.enhance_hop_pcm(h, active=m)
        assert got.dtype == np.uint8 and np.array_equal(got, want), k
        pin_in[...] = h
        pin_out[...] = 0x11
        assert pinned.enhance_hop_pcm(pin_in, out=pin_out, active=m) is pin_out
        assert np.array_equal(pin_out, want), k
        if m is not None:
            assert np.all(want[m == 0] == G.SILENCE[codec])
    for e in (on_dev, pageable, pinned):
        e.close()


# ---- 6. blocks ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
def test_blocks_do_not_depend_on_the_cut_and_the_halves_equal_the_hops(codec):
    U, hops = 2, 8
    x = codes_like(codec, U, hops, seed=60)
    table = G.expand(codec)
    off = offline(codec)
    whole = off.enhance_block_pcm_device(dev(x))
    assert whole.dtype == torch.uint8 and tuple(whole.shape) == (U, hops * S)
    for cut in ((3, 5), (1, 7)):
        off.reset()
        parts, at = [], 0
        for n in cut:
            parts.append(off.enhance_block_pcm_device(dev(x[:, at * S:(at + n) * S])))
            at += n
        assert torch.equal(torch.cat(parts, dim=1), whole), cut
    # the whole entry between expand and compress of the int16 one, device and host, in place too
    lin = offline("int16")
    want = G.compress(codec, lin.enhance_block_pcm_device(dev(table[x])).cpu().numpy())
    assert np.array_equal(whole.cpu().numpy(), want) and np.any(want != G.SILENCE[codec])
    off.reset()
    assert np.array_equal(off.enhance_block_pcm_host(x), want)
    off.reset()
    buf = dev(x)
    assert off.enhance_block_pcm_device(buf, out=buf) is buf and np.array_equal(buf.cpu().numpy(), want)
    lin.close()
    # the two halves: block entries against the hop entries of a streaming handle, bit for bit
    off.reset()
    dec = off.pcm_decode_block_device(dev(x))
    enc = off.pcm_encode_block_device(dec)
    stream = engine(codec, batch=U)
    hop_dec = [stream.pcm_decode_hop(dev(h)) for h in hops_of(x)]
    hop_enc = [stream.pcm_encode_hop(d) for d in hop_dec]
    assert torch.equal(torch.cat(hop_dec, dim=1), dec) and torch.equal(torch.cat(hop_enc, dim=1), enc)
    off.reset()
    parts = [off.pcm_decode_block_device(dev(x[:, a * S:b * S])) for a, b in ((0, 1), (1, 6), (6, 8))]      # (later hops of a block take their context from the row)
    assert torch.equal(torch.cat(parts, dim=1), dec)
    stream.close(); off.close()


@pytest.mark.parametrize("codec", CODECS)
def test_ragged_blocks_write_silence_behind_a_count(codec):
    U, n = 2, 8
    x = codes_like(codec, U, n, seed=61)
    sil = G.SILENCE[codec]
    ref = offline(codec)
    want = ref.enhance_block_pcm_device(dev(x)).cpu().numpy()      # both utterances, 8 hops each, uniform
    ref.close()
    runs = []
    for junk in (0x00, 0x2A):      # what lies behind a count has no effect
        off = offline(codec)
        first = np.full((U, n * S), junk, np.uint8)
        first[0, :5 * S] = x[0, :5 * S]
        got1 = off.enhance_block_pcm_device(dev(first), hops=[5, 0]).cpu().numpy()
        assert np.array_equal(got1[0, :5 * S], want[0, :5 * S]), junk
        assert np.all(got1[0, 5 * S:] == sil) and np.all(got1[1] == sil), junk      # behind the count, and a held row: the silence code
        # a count outside 0 .. n_hops is refused by the _host entry before anything is converted: nothing is touched
        out = np.full((U, n * S), 0x11, np.uint8)
        bad = np.array([9, 0], np.int32)
        rc = off._lib.nutls_enhance_block_pcm_ragged_host(off._h, first.ctypes.data, out.ctypes.data, n, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 0)
        assert rc == runner.NUTLS_ERR_ARG and b"nutls_enhance_block_pcm_ragged_host" in off._lib.nutls_last_error()
        assert np.all(out == 0x11)
        second = np.full((U, n * S), junk, np.uint8)
        second[0, :3 * S] = x[0, 5 * S:]
        second[1] = x[1]
        got2 = off.enhance_block_pcm_device(dev(second), hops=[3, 8]).cpu().numpy()
        assert np.array_equal(got2[0, :3 * S], want[0, 5 * S:]) and np.all(got2[0, 3 * S:] == sil), junk      # row 0 carried on from its hop 4
        assert np.array_equal(got2[1], want[1]), junk                                                           # row 1 was held: it starts here
        runs.append(np.concatenate([got1, got2], axis=1))
        off.close()
    assert np.array_equal(runs[0], runs[1])


# ---- 7. switches and refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
def test_switches_restart_the_conversion_and_other_rates_are_refused(codec):
    x = codes_like(codec, B, 2, seed=70)
    h0 = hops_of(x)[0]
    table = G.expand(codec)
    loud = dev((0.6 * np.sin(np.arange(B * 256, dtype=np.float32) * 0.07)).reshape(B, 256))
    eng = engine("int16")
    first_dec = eng.pcm_decode_hop(dev(table[h0]))      # from a zero history
    first_enc = eng.pcm_encode_hop(loud).cpu().numpy()
    assert not torch.equal(eng.pcm_decode_hop(dev(table[h0])), first_dec), "the history has no effect: the checks below would show nothing"
    eng.set_pcm_format(8000, codec)
    assert eng.pcm_dtype == "uint8" and eng.pcm_codec == codec and eng.pcm_hop_samples == S
    assert torch.equal(eng.pcm_decode_hop(dev(h0)), first_dec)
    assert np.array_equal(eng.pcm_encode_hop(loud).cpu().numpy(), G.compress(codec, first_enc))
    eng.pcm_decode_hop(dev(h0))
    eng.set_pcm_format(8000, "int16")
    assert eng.pcm_dtype == "int16" and eng.pcm_codec is None
    assert torch.equal(eng.pcm_decode_hop(dev(table[h0])), first_dec)
    assert np.array_equal(eng.pcm_encode_hop(loud).cpu().numpy(), first_enc)
    # G.711 is 8 kHz: any other rate is refused, the handle keeps its format, its hop length and its histories
    eng.set_pcm_format(8000, codec)
    twin = engine(codec)
    assert torch.equal(eng.pcm_decode_hop(dev(h0)), twin.pcm_decode_hop(dev(h0)))
    for rate in (16000, 32000, 48000):
        for fmt in CODECS:
            with pytest.raises(ValueError, match="nutls_set_pcm_format.*8 kHz"):
                eng.set_pcm_format(rate, fmt)
            assert eng.pcm_hop_samples == S and eng.pcm_delay_samples == 48 and eng.pcm_codec == codec and eng.pcm_rate == 8000
    assert torch.equal(eng.pcm_decode_hop(dev(h0)), twin.pcm_decode_hop(dev(h0)))
    with pytest.raises(ValueError):
        eng.set_pcm_format(44100, codec)
    eng.set_pcm_format(48000, "int16")
    with pytest.raises(ValueError):
        eng.set_pcm_format(48000, codec)
    assert eng.pcm_hop_samples == 768 and eng.pcm_dtype == "int16"
    # the upper band: refused as on every 8 kHz handle
    eng.set_pcm_format(8000, codec)
    with pytest.raises(ValueError, match="nutls_set_pcm_upper_band"):
        eng.set_pcm_upper_band(1.0)
    assert eng.pcm_upper_band == 0.0
    with pytest.raises(ValueError):
        eng.set_pcm_upper_follow(True)
    eng.close(); twin.close()


# ---- 8. enhance_wave and enhance_many_codec -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
def test_enhance_wave_pads_with_silence_and_lines_up_like_int16(codec):
    n = 11 * S + 77      # not a multiple of a hop, more than one block of 8 hops
    x = codes_like(codec, 1, 12, seed=80)[0, :n]
    table, sil = G.expand(codec), G.SILENCE[codec]
    off = offline(codec, utterances=1)
    lag = off.pcm_hop_samples + off.pcm_delay_samples
    seen = []
    off._wave_through_blocks(x[None], lag, lambda blk: (seen.append(blk.copy()), blk)[1])
    fed = np.concatenate(seen, axis=1)
    assert fed.shape[1] % S == 0 and fed.shape[1] >= n + lag and np.array_equal(fed[0, :n], x) and np.all(fed[0, n:] == sil)
    y = off.enhance_wave(x, 8000, codec=codec)
    assert y.shape == (n,) and y.dtype == np.uint8 and off.pcm_codec == codec
    off.close()
    # the int16 result for expand(wave) -- of the wave as it was padded, so that A-law's silence (+8) is what the int16 handle sees too
    lin = NutlsOffline(max_frames=8)
    want = lin.enhance_wave(table[fed[0]], 8000)
    lin.close()
    assert want.dtype == np.int16 and np.array_equal(y, G.compress(codec, want[:n]))
    assert np.any(y != sil)


@pytest.mark.parametrize("codec", CODECS)
def test_enhance_many_codec_equals_the_recordings_run_alone(codec):
    lengths = (700, 11 * S + 77, 300)
    waves = [codes_like(codec, 1, 12, seed=90 + i)[0, :n] for i, n in enumerate(lengths)]
    off = NutlsOffline(max_frames=8, utterances=2)
    got = off.enhance_many_codec(waves, codec)
    assert off.pcm_codec == codec and off.pcm_rate == 8000
    again = off.enhance_many_codec(waves, codec, atten_lim_db=None)
    off.close()
    for w, g, a in zip(waves, got, again):
        solo = NutlsOffline(max_frames=8)
        want = solo.enhance_wave(w, 8000, codec=codec)
        solo.close()
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, want) and np.array_equal(a, want)
