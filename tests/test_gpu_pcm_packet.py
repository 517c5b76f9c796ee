"""GPU checks of packet mode in the PCM gateway (include/nutls.h, "Packet mode"; csrc/packet.hip, csrc/api_pcm.cpp): the callers' packets
of P samples in and out, re-framed into the model's hops of S samples on the device.

The yardstick is the existing hop entry, whose streams the header guarantees to be bitwise independent: a second handle of the same batch
and settings is fed each stream's concatenated input, cut into hops, through ``enhance_hop_pcm`` -- in lockstep by hop index, so with masks
of its own, not the packet handle's (tests/packet_reference.py ``lockstep``).  The FIFO arithmetic between the two is the numpy model of
tests/packet_reference.py.  Everything is compared with ``==`` on the bytes: no tolerance anywhere.  No reference counterpart: the reference
takes float samples at 16 kHz in hops only (dnn_model/interpreter_proposed.py:384-385).

Shapes: at most 5 streams and 24 ticks, the shipped weights; every run covers at least two cycles of S / g ticks."""
import ctypes

import numpy as np
import pytest
import torch

import packet_reference as PK
import weight_families as WF
from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner
from stream_gate import Seq, assert_same, same_bits

pytestmark = pytest.mark.gpu
ERR_ARG = runner.NUTLS_ERR_ARG
DTYPE = {"float32": np.float32, "int16": np.int16, "ulaw": np.uint8, "alaw": np.uint8}
SILENCE = {"float32": 0.0, "int16": 0, "ulaw": 0xFF, "alaw": 0xD5}
POISON = {"float32": np.nan, "int16": -32768, "ulaw": 0x00, "alaw": 0x00}      # (a zero byte is full-scale negative in mu-law)


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


def engine(fmt, rate, B, setup=None, weights=None, **kw):
    e = NutlsEngine(weights, batch=B, **kw)
    e.set_pcm_format(rate, fmt)
    if setup:
        setup(e)
    return e


class Run:
    """A packet handle, the numpy model of its FIFOs and, at the end, the lockstep reference handle."""

    def __init__(self, fmt, rate, P, B, setup=None, seed=0, **kw):
        self.fmt, self.rate, self.B, self.S, self.kw, self.setup = fmt, rate, B, 256 * rate // 16000, kw, setup
        self.eng = engine(fmt, rate, B, setup, **kw)
        assert self.eng.pcm_hop_samples == self.S and self.eng.pcm_packet_samples == 0
        self.model = PK.FifoModel(B, P, self.S, SILENCE[fmt], DTYPE[fmt])
        self.set_packet(P, model=False)
        self.x, self.pos = audio(fmt, rate, B, 24 * max(P, 2 * self.S), seed), 0
        self.got, self.rounds, self.fills, self.masks = [], [], [], []

    def set_packet(self, P, model=True):
        self.eng.set_pcm_packet(P)
        if model:
            self.model.set_packet(P)
        self.P, self.plan = P, PK.plan(P, self.S)
        assert self.eng.pcm_packet_samples == P and self.eng.pcm_packet_delay_samples == self.plan["delay"]
        assert runner.pcm_packet_plan(self.rate, self.fmt, P) == self.plan

    def reset(self, b=-1):
        self.eng.reset(b)
        self.model.reset(b)

    def tick(self, mask=None, entry="host", fill=True):
        """One tick through the ``_host`` entry (numpy, host mask) or the device entry (tensors, device mask); held rows are fed poison."""
        pk = np.ascontiguousarray(self.x[:, self.pos:self.pos + self.P])
        self.pos += self.P
        assert pk.shape[1] == self.P
        fed = pk.copy()
        if mask is not None:
            mask = np.asarray(mask, bool)
            fed[~mask] = POISON[self.fmt]
        if entry == "host":
            out = self.eng.enhance_packet_pcm(fed, active=mask)
        else:
            out = self.eng.enhance_packet_pcm(dev(fed), active=None if mask is None else dev(mask)).cpu().numpy()
        self.model.tick(mask, pk)
        self.got.append(out)
        self.masks.append(mask)
        self.rounds.append(self.eng.pcm_packet_last_rounds)
        if fill:
            self.fills.append(self.eng.pcm_packet_fill())
        return out

    def reference(self):
        """hop_outs[b]: what the hop entry of a fresh handle with the same settings returns for the stream's hops"""
        ref = engine(self.fmt, self.rate, self.B, self.setup, **self.kw)
        outs = PK.lockstep(self.model.items, lambda x, a: ref.enhance_hop_pcm(x, active=a), ref.reset, self.B, self.S, DTYPE[self.fmt], POISON[self.fmt])
        ref.close()
        return outs

    def check(self, rounds=True):
        hop_outs = self.reference()
        want = self.model.expected(hop_outs)
        assert len(want) == len(self.got)
        for t, (g, w) in enumerate(zip(self.got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape, t
            for b in range(self.B):
                assert same_bits(g[b], w[b]), "tick %d, stream %d: %d of %d samples differ" % (t, b, int((g[b] != w[b]).sum()), g.shape[1])
            if self.masks[t] is not None:      # held rows are the silence word
                held = g[~self.masks[t]]
                assert same_bits(held, np.full(held.shape, SILENCE[self.fmt], DTYPE[self.fmt])), t
        for t, f in enumerate(self.fills):
            assert f.dtype == np.int32 and np.array_equal(f, self.model.fills[t]), (t, f, self.model.fills[t])
        if rounds:
            assert self.rounds == self.model.rounds, (self.rounds, self.model.rounds)
        assert any(np.abs(np.asarray(h, np.float64) - SILENCE[self.fmt]).max() > 0 for outs in hop_outs for h in outs[2:]), "the reference returned silence only"
        return hop_outs

    def close(self):
        self.eng.close()


# ---- 1. the concatenation property, NULL masks, every shape -----------------------------------------------------------------------------
SHAPES = [      # fmt, rate, P, ticks, entry
    ("ulaw", 8000, 160, 8, "device"),          # g 32, D 96, R 2: rounds 1, 1, 1, 2 repeating
    ("alaw", 8000, 80, 16, "host"),            # g 16, D 112, R 1: ticks with ZERO rounds
    ("int16", 48000, 480, 16, "device"),       # g 96, D 672, R 1
    ("float32", 48000, 960, 8, "host"),        # g 192, D 576, R 2
    ("int16", 32000, 320, 16, "device"),       # g 64, D 448, R 1
    ("float32", 16000, 160, 16, "host"),       # g 32, D 224, R 1: the plain-format path
    ("int16", 16000, 1024, 4, "device"),       # g 256, D 0, R 4: four rounds every tick
    ("float32", 32000, 512, 4, "device"),      # P = S: D 0, R 1: equals the hop entry tick for tick
]


@pytest.mark.parametrize("fmt,rate,P,ticks,entry", SHAPES, ids=["%s-%d-%d" % s[:3] for s in SHAPES])
def test_packets_are_the_delayed_hops(fmt, rate, P, ticks, entry):
    r = Run(fmt, rate, P, 3, seed=P)
    S, D, R = r.S, r.plan["delay"], r.plan["rounds"]
    assert ticks >= 2 * S // np.gcd(P, S)
    for _ in range(ticks):
        r.tick(entry=entry)
    hop_outs = r.check()
    # the property itself, without the model: D samples of silence, then the hop entry's output for the concatenated input cut into hops
    for b in range(3):
        got = np.concatenate([g[b] for g in r.got])
        x = r.x[b, :ticks * P]
        n = len(x) // S
        assert len(hop_outs[b]) == n and all(np.array_equal(it[1], x[k * S:(k + 1) * S]) for k, it in enumerate(r.model.items[b]))
        want = np.concatenate([np.full(D, SILENCE[fmt], DTYPE[fmt])] + hop_outs[b])[:len(got)]
        assert len(want) == len(got) and same_bits(got, want), b
    assert max(r.rounds) == R
    if (fmt, P) == ("ulaw", 160):
        assert r.rounds == [1, 1, 1, 2] * 2
    if (fmt, P) == ("alaw", 80):
        assert r.rounds.count(0) == 6 and set(r.rounds) == {0, 1}
    if P == 1024:
        assert r.rounds == [4] * ticks
    if P == S:
        assert r.rounds == [1] * ticks and all(same_bits(r.got[t][b], hop_outs[b][t]) for t in range(ticks) for b in range(3))
    r.close()


# ---- 2. joins and holes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rate,P", [("ulaw", 8000, 160), ("int16", 48000, 480)])
def test_joins_and_holes(fmt, rate, P):
    """Five streams join (reset(b), then active) at ticks 0, 1, 2, 3 and 5 -- every phase of the packet against the hop occurs -- and each
    is held at random ticks; held input rows are poison.  Host masks: the library sees them, so every tick issues exactly the model's rounds."""
    B, ticks, join = 5, 24, [0, 1, 2, 3, 5]
    rng = np.random.default_rng(7)
    r = Run(fmt, rate, P, B, seed=11)
    for t in range(ticks):
        mask = np.array([t >= join[b] and (t == join[b] or rng.random() > 0.25) for b in range(B)])
        for b in range(B):
            if t == join[b]:
                r.reset(b)
        r.tick(mask)
    assert len(r.fills) == ticks and len({tuple(f) for f in r.fills}) > 4
    assert any(not m.all() for m in r.masks[6:])
    r.check()
    r.close()


# ---- 3. device masks ------------------------------------------------------------------------------------------------------------------------
def test_device_masks_equal_host_masks_and_cost_every_round_until_reset():
    B, ticks = 4, 12
    rng = np.random.default_rng(3)
    masks = [np.ones(B, bool)] + [rng.random(B) > 0.3 for _ in range(ticks - 1)]
    host, devc = Run("ulaw", 8000, 160, B, seed=5), Run("ulaw", 8000, 160, B, seed=5)
    for m in masks:
        a, b = host.tick(m, "host"), devc.tick(m, "device")
        assert same_bits(a, b)
    assert not all(m.all() for m in masks)
    host.check()
    assert devc.rounds == [2] * ticks      # R on every tick: the library has not seen the masks
    devc.tick(None, "device")
    assert devc.rounds[-1] == 2            # ... and does not know the counters until they start anew
    devc.reset(-1)
    for _ in range(8):
        devc.tick(None, "device")
    assert devc.rounds[-8:] == [1, 1, 1, 2] * 2
    devc.check(rounds=False)
    host.close(); devc.close()


# ---- 4. reset(b) in mid-stream --------------------------------------------------------------------------------------------------------------
def test_reset_of_one_stream_in_mid_stream():
    r = Run("int16", 8000, 160, 3, seed=9)
    for _ in range(5):
        r.tick(entry="device")
    assert r.fills[-1].tolist() == [32, 32, 32]
    r.reset(1)      # stream 1 restarts with D samples of silence and a fresh reference; no bit of streams 0 and 2 changes
    for _ in range(9):
        r.tick(entry="device")
    assert r.fills[5].tolist() == [64, 32, 64]
    first = r.got[5][1]
    assert same_bits(first[:96], np.zeros(96, np.int16))
    r.check()
    r.close()


# ---- 5. another packet length in mid-stream ---------------------------------------------------------------------------------------------------
def test_another_packet_length_in_mid_stream():
    """set_pcm_packet re-primes the FIFOs and keeps model state and resampler histories: the reference is the hop entry fed the same hops
    without a break (the samples that waited in the input FIFOs are gone with it)."""
    r = Run("int16", 8000, 160, 3, seed=13)
    for _ in range(6):
        r.tick()
    assert r.fills[-1].tolist() == [64] * 3
    r.eng.set_pcm_packet(160)      # the value in force: nothing happens (the model is not told)
    assert r.eng.pcm_packet_fill().tolist() == [64] * 3
    r.tick()
    assert r.fills[-1].tolist() == [96] * 3
    r.set_packet(80)
    assert r.eng.pcm_packet_fill().tolist() == [0] * 3 and r.eng.pcm_packet_delay_samples == 112
    for _ in range(16):
        r.tick(entry="device")
    r.set_packet(256)
    for _ in range(2):
        r.tick()
    assert r.rounds[-2:] == [2, 2]
    r.check()
    r.close()


# ---- 6. what comes with the hop entry -----------------------------------------------------------------------------------------------------------
def _upper_follow(e):
    e.set_pcm_upper_band(1.0)
    e.set_pcm_upper_follow(True)


@pytest.mark.parametrize("case", ["upper_follow", "atten", "fusion"])
def test_settings_of_the_hop_entry_apply(case):
    if case == "upper_follow":
        r = Run("int16", 48000, 480, 3, setup=_upper_follow, seed=17)
    elif case == "atten":
        r = Run("ulaw", 8000, 160, 3, setup=lambda e: e.set_atten_limit([0.25, 0.0, 0.25]), seed=17)
    else:
        r = Run("ulaw", 8000, 160, 3, seed=17, hop_fusion=True)
        assert r.eng.launches_per_hop == 1
    rng = np.random.default_rng(19)
    for t in range(16):
        r.tick(None if t < 8 else rng.random(3) > 0.3)
    r.check()
    if case == "upper_follow":
        assert r.eng.pcm_upper_follow and r.eng.pcm_upper_band == 1.0 and r.eng.pcm_follow_gain().max() > 0
    r.close()


# ---- 7. stream order ------------------------------------------------------------------------------------------------------------------------------
def packets_case(q, masked):
    B, P, ticks = 4, 160, 8
    eng = engine("ulaw", 8000, B)
    eng.set_pcm_packet(P)
    x = audio("ulaw", 8000, B, ticks * P, 23).reshape(B, ticks, P).transpose(1, 0, 2).copy()
    m = None
    if masked:
        m = (np.random.default_rng(29).random((ticks, B)) > 0.3).astype(np.uint8)
        m[0] = 1
        x[m == 0] = POISON["ulaw"]
    X, O = q.input(x), q.output(x.shape, "uint8")
    M = None if m is None else q.input(m)
    q.open()
    with q:
        for t in range(ticks):
            q.call(eng.enhance_packet_pcm, X[t], out=O[t], active=None if M is None else M[t])
    q.close()
    res = {"packet %d" % t: O[t].cpu().numpy() for t in range(ticks)}
    res["fill"] = eng.pcm_packet_fill()
    res["rounds"] = np.array([eng.pcm_packet_last_rounds])
    eng.close()
    return res


@pytest.mark.parametrize("masked", [False, True])
def test_stream_order_on_a_busy_side_stream(masked):
    """The device entry on a non-blocking side stream behind a gate (tests/stream_gate.py), inputs and masks poison until the gate opens,
    no synchronisation between ticks: equals the synchronous run bit for bit."""
    what = "packet ticks, %s" % ("device masks" if masked else "NULL masks")
    s = packets_case(Seq(False, what), masked)
    g = packets_case(Seq(True, what), masked)
    assert_same(s, g, what)
    assert any((s["packet %d" % t] != 0xFF).any() for t in range(3, 8))


# ---- 8. refusals change nothing --------------------------------------------------------------------------------------------------------------------
def _host_call(e, x, o, dc=0, active=None):
    return e._lib.nutls_enhance_packet_pcm_host(e._h, None if x is None else x.ctypes.data, None if o is None else o.ctypes.data, active, dc)


def last_error(e):
    return e._lib.nutls_last_error().decode()


def test_refusals_change_nothing():
    r = Run("ulaw", 8000, 160, 3, seed=31)
    for _ in range(3):
        r.tick()
    x, o = np.full((3, 160), 0x00, np.uint8), np.full((3, 160), 0x5A, np.uint8)
    before = r.eng.pcm_packet_fill()
    assert before.tolist() == [96] * 3
    lib, h = r.eng._lib, r.eng._h
    for call, word in ((lambda: _host_call(r.eng, x, o, dc=7), "dc_mode"), (lambda: _host_call(r.eng, None, o), "null"),
                       (lambda: _host_call(r.eng, x, None), "null"), (lambda: lib.nutls_enhance_packet_pcm(h, None, None, None, 0, None), "null"),
                       (lambda: lib.nutls_set_pcm_packet(h, 100), "multiple of 16"), (lambda: lib.nutls_set_pcm_packet(h, 528), "1 .. 512")):
        rc = call()
        assert rc == ERR_ARG and word in last_error(r.eng), (rc, word, last_error(r.eng))
        assert np.array_equal(r.eng.pcm_packet_fill(), before) and r.eng.pcm_packet_samples == 160
    assert (o == 0x5A).all()
    for _ in range(5):      # ... and the stream goes on as if nothing had been asked
        r.tick()
    r.check()
    # set_pcm_format turns the mode off; a packet call with the mode off is refused
    r.eng.set_pcm_format(8000, "ulaw")
    assert r.eng.pcm_packet_samples == 0 and r.eng.pcm_packet_delay_samples == 0
    assert _host_call(r.eng, x, o) == ERR_ARG and "packet mode is off" in last_error(r.eng)
    with pytest.raises(ValueError, match="packet mode is off"):
        r.eng.pcm_packet_fill()
    with pytest.raises(ValueError, match="packet mode is off"):
        r.eng.enhance_packet_pcm(x)
    r.eng.set_pcm_packet(ms=20)
    assert r.eng.pcm_packet_samples == 160 and r.eng.pcm_packet_fill().tolist() == [0] * 3
    with pytest.raises(ValueError):
        r.eng.set_pcm_packet(ms=0.3)
    r.close()


def test_offline_handles_are_refused():
    off = NutlsOffline(max_frames=8, utterances=2)
    off.set_pcm_format(8000, "ulaw")
    x = np.zeros((2, 160), np.uint8)
    assert off._lib.nutls_set_pcm_packet(off._h, 160) == ERR_ARG and "offline handle" in off._lib.nutls_last_error().decode()
    assert off._lib.nutls_pcm_packet_samples(off._h) == 0
    assert off._lib.nutls_enhance_packet_pcm_host(off._h, x.ctypes.data, x.ctypes.data, None, 0) == ERR_ARG
    assert "offline handle" in off._lib.nutls_last_error().decode()
    off.close()


def test_where_masks_are_refused_so_are_packets_that_need_them():
    """Baseline variant, causal32 CTFA and the per-layer modes: P = 160 needs masked hops and is refused with check_active's reason, at the
    set and -- the mode can change in between -- again at the call; P a multiple of S without a mask works wherever the hop entry does."""
    x = audio("ulaw", 8000, 2, 4 * 256, 37)
    # causal32: set while packet mode is on
    e = engine("ulaw", 8000, 2)
    e.set_pcm_packet(160)
    e.enhance_packet_pcm(np.ascontiguousarray(x[:, :160]))
    before = e.pcm_packet_fill()
    e.set_ctfa_mode("causal32")
    o = np.full((2, 160), 0x5A, np.uint8)
    assert _host_call(e, np.ascontiguousarray(x[:, 160:320]), o) == ERR_ARG and "NUTLS_CTFA_CAUSAL32" in last_error(e)
    assert np.array_equal(e.pcm_packet_fill(), before) and (o == 0x5A).all()
    assert e._lib.nutls_set_pcm_packet(e._h, 80) == ERR_ARG and "NUTLS_CTFA_CAUSAL32" in last_error(e) and e.pcm_packet_samples == 160
    e.close()
    e, ref = engine("ulaw", 8000, 2), engine("ulaw", 8000, 2)
    e.set_ctfa_mode("causal32"), ref.set_ctfa_mode("causal32")
    e.set_pcm_packet(256)      # whole hops, no mask: works, and equals the hop entry
    got = e.enhance_packet_pcm(np.ascontiguousarray(x[:, :256]))
    want = np.concatenate([ref.enhance_hop_pcm(np.ascontiguousarray(x[:, k * 128:(k + 1) * 128])) for k in range(2)], axis=1)
    assert same_bits(got, want) and e.pcm_packet_last_rounds == 2
    m = np.array([True, False])
    assert _host_call(e, np.ascontiguousarray(x[:, :256]), o, active=m.ctypes.data) == ERR_ARG and "NUTLS_CTFA_CAUSAL32" in last_error(e)
    e.close(); ref.close()
    # the baseline variant
    w = WF.container("plain", variant="baseline")
    e, ref = engine("ulaw", 8000, 2, weights=w, variant="baseline"), engine("ulaw", 8000, 2, weights=w, variant="baseline")
    assert e._lib.nutls_set_pcm_packet(e._h, 160) == ERR_ARG and "baseline variant" in last_error(e) and e.pcm_packet_samples == 0
    e.set_pcm_packet(128)
    for k in range(3):
        hop = np.ascontiguousarray(x[:, k * 128:(k + 1) * 128])
        assert same_bits(e.enhance_packet_pcm(hop), ref.enhance_hop_pcm(hop)), k
    assert _host_call(e, hop, o[:, :128].copy(), active=m.ctypes.data) == ERR_ARG and "baseline variant" in last_error(e)
    e.close(); ref.close()
    # a per-layer mode
    e = engine("ulaw", 8000, 2, mode="launches")
    assert e._lib.nutls_set_pcm_packet(e._h, 160) == ERR_ARG and "mode 3" in last_error(e)
    e.close()
