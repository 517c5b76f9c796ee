"""GPU checks of the channels of the PCM gateway (include/nutls.h, "Channels"; csrc/channels.hip, csrc/api_pcm.cpp): interleaved 2- and
4-channel frames in and out of every ``_pcm`` entry, one stream per channel.

The yardstick is the rule of the header, ``E_C(x) == interleave(E_1(deinterleave(x)))``: a second handle of the same batch and settings with
1 channel is fed the de-interleaved buffers (tests/channels_reference.py: a reshape and a transpose), and everything is compared with ``==``
on the bytes -- no tolerance anywhere, except where the issue of this feature names one (``enhance_many_channels`` against another handle
shape, the bound of tests/test_gpu_ragged_pcm.py).  Held samples and hops behind a count are fed poison.  No reference counterpart: the
reference takes one float row per call (dnn_model/interpreter_proposed.py:384-385).

Shapes: at most 8 streams, the shipped weights.  The kernels' edges: a row of fewer quads than a wavefront (8 kHz G.711 hop: 8 quads), a row
of more than one lane pass (48 kHz float32 hop: 192 quads), a block row of more than one workgroup chunk with a partly filled last chunk
(5 hops at 48 kHz float32: 960 quads)."""
import ctypes

import numpy as np
import pytest
import torch

import channels_reference as CH
from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner
from stream_gate import Seq, assert_same, same_bits

pytestmark = pytest.mark.gpu
DTYPE = {"float32": np.float32, "int16": np.int16, "ulaw": np.uint8, "alaw": np.uint8}
SILENCE = {"float32": 0.0, "int16": 0, "ulaw": 0xFF, "alaw": 0xD5}
POISON = {"float32": np.nan, "int16": -32768, "ulaw": 0x00, "alaw": 0x00}      # (a zero byte is full-scale negative in mu-law)
FORMATS = [("ulaw", 8000), ("alaw", 8000), ("int16", 8000), ("float32", 16000), ("int16", 16000), ("int16", 32000), ("float32", 48000)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def audio(fmt, rate, rows, n, seed):
    """[rows, n] in the format: a tone per row under a slow envelope, and seeded noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.4 * np.sin(2 * np.pi * 440.0 / rate * t[None, :] + rng.uniform(0, 6.28, (rows, 1))) * (0.05 + np.abs(np.sin(2 * np.pi * t[None, :] / (0.09 * rate))))
    x = x + 0.05 * rng.standard_normal((rows, n))
    if fmt == "float32":
        return x.astype(np.float32)
    s = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
    return s if fmt == "int16" else runner.g711_compress(fmt, s)


def engines(fmt, rate, B, C, setup=None, **kw):
    """The handle under test with C channels and the yardstick with 1, same batch and settings."""
    pair = []
    for channels in (C, 1):
        e = NutlsEngine(None, batch=B, **kw)
        e.set_pcm_format(rate, fmt)
        if setup:
            setup(e)
        e.set_pcm_channels(channels)
        assert e.pcm_channels == channels
        pair.append(e)
    return pair


def offlines(fmt, rate, U, C, T=8):
    pair = []
    for channels in (C, 1):
        o = NutlsOffline(None, max_frames=T, utterances=U)
        o.set_pcm_format(rate, fmt)
        o.set_pcm_channels(channels)
        pair.append(o)
    return pair


def poisoned(rows, fmt, held):
    """rows [B, n] with the rows of ``held`` (bool [B]) replaced by poison"""
    fed = rows.copy()
    fed[np.asarray(held, bool)] = POISON[fmt]
    return fed


def same(got, want, what):
    assert same_bits(got, want), "%s: %d of %d bytes differ" % (what, int((np.ascontiguousarray(got).view(np.uint8).reshape(-1) !=
                                                                           np.ascontiguousarray(want).view(np.uint8).reshape(-1)).sum())
                                                                if np.shape(got) == np.shape(want) else -1, np.asarray(want).nbytes)


def hop_both(eng, yard, C, rows, mask, on_device, fmt):
    """One hop of per-stream ``rows`` [B, S] through both handles; returns the handle's result split into stream rows, and the yardstick's."""
    fed = np.ascontiguousarray(rows) if mask is None else poisoned(rows, fmt, ~np.asarray(mask, bool))
    frames = CH.join_rows(fed, C)
    if on_device:
        got = eng.enhance_hop_pcm(dev(frames), active=None if mask is None else dev(np.asarray(mask, np.uint8))).cpu().numpy()
        want = yard.enhance_hop_pcm(dev(fed), active=None if mask is None else dev(np.asarray(mask, np.uint8))).cpu().numpy()
    else:
        got = eng.enhance_hop_pcm(frames, active=mask)
        want = yard.enhance_hop_pcm(fed, active=mask)
    assert got.shape == frames.shape and got.dtype == frames.dtype
    return got, want


# ---- 1. the hop entry, every format, 2 and 4 channels, device tensors and host arrays ---------------------------------------------------------
@pytest.mark.parametrize("fmt,rate", FORMATS)
@pytest.mark.parametrize("B,C", [(4, 2), (8, 4)])
def test_hop_entry_equals_the_one_channel_entry_on_the_transposed_buffers(fmt, rate, B, C):
    S = 256 * rate // 16000
    eng, yard = engines(fmt, rate, B, C)
    x = audio(fmt, rate, B, 6 * S, 11 * B + C)
    for on_device in (True, False):
        eng.reset()
        yard.reset()
        loud = False
        for k in range(6):
            got, want = hop_both(eng, yard, C, x[:, k * S:(k + 1) * S], None, on_device, fmt)
            same(got, CH.join_rows(want, C), "%s hop %d" % ("device" if on_device else "host", k))
            loud = loud or np.abs(want.astype(np.float64) - SILENCE[fmt]).max() > 0
        assert loud, "the yardstick returned silence only"
    # the three-dimensional view of the same memory is taken and returned as it is
    frames3 = CH.join_rows(x[:, :S], C).reshape(B // C, S, C)
    out3 = eng.enhance_hop_pcm(frames3)
    assert out3.shape == frames3.shape
    same(out3.reshape(B // C, S * C), CH.join_rows(yard.enhance_hop_pcm(np.ascontiguousarray(x[:, :S])), C), "[B / C, S, C]")
    eng.close()
    yard.close()


# ---- 2. masks: one channel of a frame row held while its partner steps ----------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rate", [("ulaw", 8000), ("float32", 48000)])
@pytest.mark.parametrize("on_device", [True, False])
def test_a_held_channel_is_silence_and_its_partner_is_unaffected(fmt, rate, on_device):
    B, C, S = 4, 2, 256 * rate // 16000
    eng, yard = engines(fmt, rate, B, C)
    free = NutlsEngine(None, batch=B)      # no holds at all: what a partner returns when nobody is ever held
    free.set_pcm_format(rate, fmt)
    masks = [[1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 1, 0], [1, 0, 0, 1], [1, 1, 0, 1], [0, 1, 1, 1], [1, 1, 1, 1]]
    x = audio(fmt, rate, B, len(masks) * S, 5)
    fed_at = [0] * B      # per stream: how many of its own hops it has been fed -- a held stream resumes as if no tick had passed
    outs = [[] for _ in range(B)]
    for m in masks:
        m = np.asarray(m, bool)
        rows = np.stack([x[b, fed_at[b] * S:(fed_at[b] + 1) * S] for b in range(B)])
        got, want = hop_both(eng, yard, C, rows, m, on_device, fmt)
        same(got, CH.join_rows(want, C), "mask %s" % m.astype(int))
        split = CH.split_rows(got, C)
        assert same_bits(split[~m], np.full(split[~m].shape, SILENCE[fmt], DTYPE[fmt])), "held positions are the silence word"
        for b in np.flatnonzero(m):
            outs[b].append(split[b])
            fed_at[b] += 1
    for k in range(max(fed_at)):      # every stream's own hops, never held: the same bits
        w = free.enhance_hop_pcm(np.ascontiguousarray(x[:, k * S:(k + 1) * S]))
        for b in range(B):
            if k < fed_at[b]:
                same(outs[b][k], w[b], "stream %d, its hop %d, against a run without holds" % (b, k))
    for e in (eng, yard, free):
        e.close()


# ---- 3. settings that ride along, different between the two channels of a row ------------------------------------------------------------------
def test_the_attenuation_limit_is_per_stream():
    fmt, rate, B, C, S = "int16", 32000, 4, 2, 512
    eng, yard = engines(fmt, rate, B, C, setup=lambda e: e.set_atten_limit(limit=[0.0, 0.5, 1.0, 0.125]))
    x = audio(fmt, rate, B, 4 * S, 3)
    for k in range(4):
        got, want = hop_both(eng, yard, C, x[:, k * S:(k + 1) * S], None, k % 2 == 0, fmt)
        same(got, CH.join_rows(want, C), "hop %d" % k)
    assert not same_bits(want[0], want[1])
    eng.close()
    yard.close()


def test_hop_fusion_rides_along():
    fmt, rate, B, C, S = "alaw", 8000, 4, 2, 128
    eng, yard = engines(fmt, rate, B, C, hop_fusion=True, streams_per_workgroup=1)
    x = audio(fmt, rate, B, 4 * S, 4)
    masks = [None, [1, 0, 1, 1], [0, 1, 1, 1], None]
    for k, m in enumerate(masks):
        got, want = hop_both(eng, yard, C, x[:, k * S:(k + 1) * S], m, True, fmt)
        same(got, CH.join_rows(want, C), "hop %d" % k)
    eng.close()
    yard.close()


def test_upper_band_and_follow_are_per_stream():
    fmt, rate, B, C, S = "float32", 48000, 4, 2, 768

    def setup(e):
        e.set_pcm_upper_band(0.75)
        e.set_pcm_upper_follow(True)

    eng, yard = engines(fmt, rate, B, C, setup=setup)
    x = audio(fmt, rate, B, 5 * S, 6)
    x[1] *= 0.01      # the two channels of row 0 differ in level: their followed gains differ
    masks = [None, None, [1, 0, 1, 1], None, [1, 1, 0, 1]]
    for k, m in enumerate(masks):
        got, want = hop_both(eng, yard, C, x[:, k * S:(k + 1) * S], m, True, fmt)
        same(got, CH.join_rows(want, C), "hop %d" % k)
        same(eng.pcm_follow_gain(), yard.pcm_follow_gain(), "follow gain after hop %d" % k)
    g = eng.pcm_follow_gain()
    assert g.shape == (B,) and len(set(g.tolist())) > 1
    eng.close()
    yard.close()


# ---- 4. the halves ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rate", [("ulaw", 8000), ("float32", 48000), ("float32", 16000)])
def test_the_hop_halves(fmt, rate):
    B, C, S = 4, 2, 256 * rate // 16000
    eng, yard = engines(fmt, rate, B, C)
    x = audio(fmt, rate, B, 3 * S, 8)
    for k, m in enumerate([None, [1, 0, 1, 1], None]):
        rows = x[:, k * S:(k + 1) * S]
        fed = rows if m is None else poisoned(rows, fmt, ~np.asarray(m, bool))
        a = None if m is None else dev(np.asarray(m, np.uint8))
        f_got, f_want = eng.pcm_decode_hop(dev(CH.join_rows(fed, C)), active=a), yard.pcm_decode_hop(dev(fed), active=a)
        assert tuple(f_got.shape) == (B, 256)      # the 16 kHz float side stays one row per stream
        same(f_got.cpu().numpy(), f_want.cpu().numpy(), "decode %d" % k)
        p_got, p_want = eng.pcm_encode_hop(f_want, active=a), yard.pcm_encode_hop(f_want, active=a)
        assert tuple(p_got.shape) == (B // C, S * C)
        same(p_got.cpu().numpy(), CH.join_rows(p_want.cpu().numpy(), C), "encode %d" % k)
    eng.close()
    yard.close()


@pytest.mark.parametrize("fmt,rate", [("alaw", 8000), ("float32", 48000)])
def test_the_block_halves_with_and_without_counts(fmt, rate):
    U, C, S = 4, 2, 256 * rate // 16000
    off, yard = offlines(fmt, rate, U, C)
    x = audio(fmt, rate, U, 5 * S, 9)
    for counts in (None, [5, 0, 3, 5], [2, 4, 0, 1]):
        fed = x.copy()
        if counts is not None:
            for u, k in enumerate(counts):
                fed[u, k * S:] = POISON[fmt]
        f_got, f_want = off.pcm_decode_block_device(dev(CH.join_rows(fed, C)), hops=counts), yard.pcm_decode_block_device(dev(fed), hops=counts)
        assert tuple(f_got.shape) == (U, 5 * 256)
        same(f_got.cpu().numpy(), f_want.cpu().numpy(), "decode %s" % (counts,))
        p_got, p_want = off.pcm_encode_block_device(f_want, hops=counts), yard.pcm_encode_block_device(f_want, hops=counts)
        assert tuple(p_got.shape) == (U // C, 5 * S * C)
        same(p_got.cpu().numpy(), CH.join_rows(p_want.cpu().numpy(), C), "encode %s" % (counts,))
    off.close()
    yard.close()


# ---- 5. offline blocks: uniform with a carry, ragged with counts that differ within a row ---------------------------------------------------------
def ragged_host(off, blk, n, counts):
    out = np.empty_like(blk)
    c = np.asarray(counts, np.int32)
    rc = off._lib.nutls_enhance_block_pcm_ragged_host(off._h, blk.ctypes.data, out.ctypes.data, n, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 0)
    assert rc == 0, off._lib.nutls_last_error()
    return out


@pytest.mark.parametrize("fmt,rate", [("alaw", 8000), ("float32", 48000)])
@pytest.mark.parametrize("on_device", [True, False])
def test_offline_blocks_uniform_and_ragged(fmt, rate, on_device):
    U, C, S = 4, 2, 256 * rate // 16000
    off, yard = offlines(fmt, rate, U, C)
    x = audio(fmt, rate, U, 17 * S, 10)
    at = 0
    for n, counts in ((5, None), (3, None), (5, [5, 0, 3, 5]), (4, [2, 4, 0, 1])):
        fed = np.ascontiguousarray(x[:, at * S:(at + n) * S])
        at += n
        if counts is not None:
            for u, k in enumerate(counts):
                fed[u, k * S:] = POISON[fmt]
        frames = CH.join_rows(fed, C)
        if on_device:
            got = off.enhance_block_pcm_device(dev(frames), hops=counts).cpu().numpy()
            want = yard.enhance_block_pcm_device(dev(fed), hops=counts).cpu().numpy()
        elif counts is None:
            got, want = off.enhance_block_pcm_host(frames), yard.enhance_block_pcm_host(fed)
        else:
            got, want = ragged_host(off, frames, n, counts), ragged_host(yard, fed, n, counts)
        assert got.shape == frames.shape
        same(got, CH.join_rows(want, C), "block of %d hops, counts %s" % (n, counts))
        if counts is not None:      # behind a count: what the 1-channel entry writes there
            split = CH.split_rows(got, C)
            for u, k in enumerate(counts):
                assert same_bits(split[u, k * S:], np.full((n - k) * S, SILENCE[fmt], DTYPE[fmt])), (u, k)
    off.close()
    yard.close()


# ---- 6. packet mode ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rate,P", [("ulaw", 8000, 160), ("int16", 48000, 480)])
@pytest.mark.parametrize("masking", ["none", "host", "device"])
def test_packet_mode(fmt, rate, P, masking):
    B, C = 4, 2
    eng, yard = engines(fmt, rate, B, C, setup=lambda e: e.set_pcm_packet(P))
    x = audio(fmt, rate, B, 12 * P, 12)
    rng = np.random.default_rng(2)
    for t in range(12):
        m = None if masking == "none" else (rng.random(B) < 0.7)
        if m is not None and t == 0:
            m[:] = [True, False, True, True]
        rows = np.ascontiguousarray(x[:, t * P:(t + 1) * P])
        fed = rows if m is None else poisoned(rows, fmt, ~m)
        if t == 5:      # one channel of a row starts anew in mid-cycle
            eng.reset(1)
            yard.reset(1)
        if masking == "device":
            got = eng.enhance_packet_pcm(dev(CH.join_rows(fed, C)), active=dev(m.astype(np.uint8))).cpu().numpy()
            want = yard.enhance_packet_pcm(dev(fed), active=dev(m.astype(np.uint8))).cpu().numpy()
        elif t % 2 and masking == "none":
            got = eng.enhance_packet_pcm(dev(CH.join_rows(fed, C))).cpu().numpy()
            want = yard.enhance_packet_pcm(dev(fed)).cpu().numpy()
        else:
            got, want = eng.enhance_packet_pcm(CH.join_rows(fed, C), active=m), yard.enhance_packet_pcm(fed, active=m)
        assert got.shape == (B // C, P * C)
        same(got, CH.join_rows(want, C), "tick %d" % t)
        assert eng.pcm_packet_last_rounds == yard.pcm_packet_last_rounds, t
        assert np.array_equal(eng.pcm_packet_fill(), yard.pcm_packet_fill()), t
    eng.close()
    yard.close()


# ---- 7. the layout is a setting: it may change in mid-stream and survives a format switch ---------------------------------------------------------
def test_layout_switch_in_mid_stream():
    fmt, rate, B, S = "int16", 16000, 4, 256
    eng, yard = engines(fmt, rate, B, 2)
    x = audio(fmt, rate, B, 8 * S, 13)
    layout = [2, 2, 2, 1, 1, 4]
    got, want = [], []
    for k, C in enumerate(layout):
        eng.set_pcm_channels(C)
        rows = np.ascontiguousarray(x[:, k * S:(k + 1) * S])
        out = eng.enhance_hop_pcm(dev(CH.join_rows(rows, C)) if C > 1 else dev(rows)).cpu().numpy()
        assert out.shape == (B // C, S * C)
        got.append(CH.split_rows(out, C) if C > 1 else out)
        want.append(yard.enhance_hop_pcm(dev(rows)).cpu().numpy())
    same(np.concatenate(got, axis=1), np.concatenate(want, axis=1), "every stream's concatenated output")
    for e in (eng, yard):      # the same format again: histories restart on both alike, the layout stays
        e.set_pcm_format(8000, "int16")
        e.set_pcm_format(rate, fmt)
    assert eng.pcm_channels == 4 and yard.pcm_channels == 1
    eng.reset(2)
    yard.reset(2)
    assert eng.pcm_channels == 4
    for k in (6, 7):
        rows = np.ascontiguousarray(x[:, k * S:(k + 1) * S])
        same(eng.enhance_hop_pcm(CH.join_rows(rows, 4)), CH.join_rows(yard.enhance_hop_pcm(rows), 4), "hop %d behind the format switch" % k)
    eng.close()
    yard.close()


# ---- 8. in place -----------------------------------------------------------------------------------------------------------------------------------
def test_in_place_hop_and_block():
    fmt, rate, C, S = "float32", 48000, 2, 768
    eng, yard = engines(fmt, rate, 4, C)
    x = audio(fmt, rate, 4, 5 * S, 14)
    for k in range(3):
        rows = np.ascontiguousarray(x[:, k * S:(k + 1) * S])
        buf = dev(CH.join_rows(rows, C))
        assert eng.enhance_hop_pcm(buf, out=buf) is buf
        same(buf.cpu().numpy(), CH.join_rows(yard.enhance_hop_pcm(dev(rows)).cpu().numpy(), C), "hop %d in place" % k)
    eng.close()
    yard.close()
    off, yard = offlines(fmt, rate, 4, C)
    for n in (5, 3):
        buf = dev(CH.join_rows(x[:, :n * S], C))
        off.enhance_block_pcm_device(buf, out=buf)
        same(buf.cpu().numpy(), CH.join_rows(yard.enhance_block_pcm_device(dev(x[:, :n * S])).cpu().numpy(), C), "block of %d hops in place" % n)
    off.close()
    yard.close()


# ---- 9. stream order: a busy non-blocking side stream, no synchronisation between the calls -----------------------------------------------------
def test_on_a_busy_side_stream_behind_the_gate():
    fmt, rate, B, C, S = "int16", 48000, 4, 2, 768
    x = audio(fmt, rate, B, 4 * S, 15)
    masks = [None, [1, 0, 1, 1], None]
    results = {}
    for gated in (False, True):
        eng = engines(fmt, rate, B, C)[0]
        eng.enhance_hop_pcm(CH.join_rows(x[:, 3 * S:], C))      # (every lazily allocated buffer exists before the gate)
        eng.reset()
        q = Seq(gated, "channels")
        ins = [q.input(CH.join_rows(x[:, k * S:(k + 1) * S], C)) for k in range(3)]
        acts = [None if m is None else q.input(np.asarray(m, np.uint8)) for m in masks]
        outs = [q.output((B // C, S * C), fmt) for _ in range(3)]
        q.open()
        with q:
            for k in range(3):
                q.call(eng.enhance_hop_pcm, ins[k], out=outs[k], active=acts[k])
        q.close()
        results[gated] = {"hop %d" % k: o.cpu().numpy() for k, o in enumerate(outs)}
        eng.close()
    assert_same(results[False], results[True], "enhance_hop_pcm with 2 channels")


# ---- 10. refusals on a live handle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,bad,keeps", [(3, 2, 1), (4, 3, 2), (6, 4, 2)])
def test_refusals_change_nothing(B, bad, keeps):
    fmt, rate, S = "ulaw", 8000, 128
    eng, yard = engines(fmt, rate, B, keeps)
    x = audio(fmt, rate, B, 2 * S, 16)
    join = (lambda r: CH.join_rows(r, keeps)) if keeps > 1 else (lambda r: r)
    same(eng.enhance_hop_pcm(join(np.ascontiguousarray(x[:, :S]))), join(yard.enhance_hop_pcm(np.ascontiguousarray(x[:, :S]))), "hop 0")
    rc = eng._lib.nutls_set_pcm_channels(eng._h, bad)
    assert rc == runner.NUTLS_ERR_ARG
    err = eng._lib.nutls_last_error().decode()
    assert err.startswith("nutls_set_pcm_channels: ") and ("multiple" in err if bad in (2, 4) else "1 (off), 2 or 4" in err), err
    with pytest.raises(ValueError):
        eng.set_pcm_channels(bad)
    assert eng.pcm_channels == keeps
    same(eng.enhance_hop_pcm(join(np.ascontiguousarray(x[:, S:]))), join(yard.enhance_hop_pcm(np.ascontiguousarray(x[:, S:]))), "the next hop")
    eng.close()
    yard.close()


# ---- 11. / 12. whole recordings of interleaved frames --------------------------------------------------------------------------------------------
def test_enhance_wave_channels_is_enhance_wave_of_the_transposed_recording():
    N = 5 * 128 + 37      # not a multiple of the hop
    x = np.ascontiguousarray(audio("ulaw", 8000, 2, N, 17).T)      # [N, 2], the wave-file layout
    off, yard = NutlsOffline(None, max_frames=4, utterances=2), NutlsOffline(None, max_frames=4, utterances=2)
    got = off.enhance_wave_channels(x, 8000, 2, codec="ulaw")
    want = yard.enhance_wave(np.ascontiguousarray(x.T), 8000, codec="ulaw")
    assert got.shape == x.shape and got.dtype == x.dtype and off.pcm_channels == 2 and yard.pcm_channels == 1
    same(got, np.ascontiguousarray(want.T), "enhance_wave_channels")
    assert np.abs(want.astype(np.int32) - 0xFF).max() > 0
    with pytest.raises(ValueError):
        off.enhance_wave_channels(x[:, :1], 8000, 2, codec="ulaw")
    with pytest.raises(ValueError):
        off.enhance_wave_channels(x, 8000, 3, codec="ulaw")
    off.close()
    yard.close()


def test_enhance_many_channels():
    rate, C, S = 48000, 2, 768
    lengths = [7 * S + 100, 2 * S + 5, 4 * S]
    ints = [np.ascontiguousarray(audio("int16", rate, C, n, 20 + i).T) for i, n in enumerate(lengths)]      # [N_i, 2]
    waves = [x.astype(np.float32) / np.float32(32768.0) for x in ints]      # the same recordings as float32, exactly
    off = NutlsOffline(None, max_frames=4, utterances=4)
    got = off.enhance_many_channels(waves, rate, C)
    one = NutlsOffline(None, max_frames=4, utterances=1)
    for i, (g, w) in enumerate(zip(got, waves)):
        assert g.shape == w.shape and g.dtype == w.dtype
        for c in range(C):
            one.reset()
            want = one.enhance_wave(np.ascontiguousarray(w[:, c]), rate).astype(np.float64)
            rel = np.sqrt(np.mean((g[:, c] - want) ** 2)) / np.sqrt(np.mean(want ** 2))
            print("recording %d channel %d: relative RMS %.3g against a one-utterance handle" % (i, c, rel))
            assert rel < 1e-5, (i, c, rel)      # the bound between handle shapes of tests/test_gpu_ragged_pcm.py
    again = off.enhance_many_channels(waves, rate, C)
    for g, a in zip(got, again):
        same(a, g, "a second call")
    for i, (x, q, f) in enumerate(zip(ints, off.enhance_many_channels(ints, rate, C), got)):      # int16: the quantised float32 result
        assert q.dtype == np.int16 and q.shape == x.shape, i
        assert np.array_equal(q, np.clip(np.rint(f * np.float32(32768.0)), -32768, 32767).astype(np.int16)), i
    assert any(g.any() for g in got)
    off.close()
    one.close()
