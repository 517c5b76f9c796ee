"""Stream ordering of every device entry (include/nutls.h: "asynchronous on `stream`"; "calls on one handle take effect in the order
they are made, whichever streams they name"), on a busy non-default stream.

Every case runs its call sequence twice on fresh handles (tests/stream_gate.py):
  S  on the legacy default stream with a synchronisation after every call -- what the rest of the suite does;
  G  on a non-blocking side stream behind a gate: the inputs, masks and counts hold poison until a bounded sleep on that stream
     has run, the calls are made with no synchronisation between them, the host synchronises at the end.
G must equal S bit for bit: outputs, all states of every stream at the end, the followed gain where there is one, and the overlap tails
through one more zero hop.  Work that the library queued on another stream runs during the sleep, on NaN or on stale state, and the
comparison sees it.  Where the float64 oracle covers the path, S also meets the suite's bounds against it (WF.OUT_BOUND / WF.STATE_BOUND).

A gated run counts only if the gate was still closed when the last non-blocking call had returned ("gate held" in the output); a gate
that opened early fails the test as inconclusive.

What the cases see (measured on an MI355X): without the cross-stream event of engine.cpp order_after_last, all eight cases of g fail --
the step on another side stream or on NULL with NaN everywhere, the _host entries with bit-different results.  With `e->stream` in place
of the caller's stream in istft_hop_impl's launch, four of the eight hop cases of c fail with bit-different hops (the cases that reach
that launch: three launches, the halves, both PCM formats).  Dropping the chunk streams' wait for the fork event in process_block_impl
is NOT seen by e: every chunk's first launch of every group also waits for the previous chunk's event of that group, which is recorded
behind the gate, so the chunk streams stay ordered behind the caller's stream without the fork."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import weight_families as WF
from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd import runner
from stream_gate import Seq, assert_same, calibrate, same_bits, side_streams
from test_gpu_step_active import schedule

pytestmark = pytest.mark.gpu

ATTEN = [0.0, 0.1, 1.0, 0.5]          # the attenuation limits of the hop cases (B = 4)


# ---- premises, once per session ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def premises():
    """torch side streams do not block on the legacy default stream here (a tiny copy on the default stream completes while a gated side
    stream is busy), and the synchronous one-stream step sequence is deterministic (two runs are bit-identical)."""
    calibrate()
    q = Seq(True, "premise")
    q.open()
    a, b = torch.zeros(16, device="cuda"), torch.ones(16, device="cuda")      # (the fills run on the default stream too)
    a.copy_(b)
    done = torch.cuda.Event()
    done.record()
    done.synchronize()
    busy = not q.marker.query()
    q.close()
    assert busy, "a copy on the default stream waited for the gated side stream: torch side streams block on the default stream here"
    assert bool((a == 1).all())
    first, second = (steps_case(Seq(False), WF.container("plain"), 3, 1, WF.inputs(3)) for _ in range(2))
    assert_same(first, second, "two synchronous runs of the one-stream step sequence")


def both(case, *args, **kwargs):
    """The sequence synchronously (S) and gated (G) on fresh handles; G must equal S bit for bit.  Returns S."""
    what = kwargs.pop("what", case.__name__)
    s = case(Seq(False, what), *args, **kwargs)
    g = case(Seq(True, what), *args, **kwargs)
    for key, v in s.items():
        if np.asarray(v).dtype.kind == "f":
            assert np.isfinite(v).all(), "%s: '%s' of the synchronous run is not finite" % (what, key)
    assert_same(s, g, what)
    return s


def state_layout(h):
    """[(name, floats per row)] of a handle's state tensors (streaming or offline) in the order of nutls_state_get_all"""
    lib, res = h._lib, []
    for i in range(lib.nutls_state_count(h._h)):
        name, d0, d1 = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
        runner._check(lib, lib.nutls_state_info(h._h, i, ctypes.byref(name), ctypes.byref(d0), ctypes.byref(d1)))
        res.append((name.value.decode(), d0.value * d1.value))
    return res


def all_states(h, rows):
    """nutls_state_get_all of every row (stream / utterance): [rows, total]"""
    total = sum(n for _, n in state_layout(h))
    out = np.empty((rows, total), np.float32)
    for r in range(rows):
        runner._check(h._lib, h._lib.nutls_state_get_all(h._h, r, runner._fptr(out[r]), total))
    return out


def check_oracle(s, ref_out, ref_state=None, streams=None, names=None):
    """S against the float64 oracle with the suite's bounds: outputs per frame, and (``ref_state``) every state tensor of every stream."""
    for f in range(s["out"].shape[0]):
        r = WF.scaled_rms(s["out"][f], ref_out[f]) / WF.OUT_BOUND
        assert r < 1.0, "output of frame %d is at %.3g x the bound against the float64 oracle" % (f, r)
    if ref_state is None:
        return
    o = 0
    for name, size in names:
        for b, src in enumerate(streams):
            r = WF.scaled_rms(s["states"][b, o:o + size], np.asarray(ref_state[name][src]).reshape(-1)) / WF.STATE_BOUND
            assert r < 1.0, "state %s of stream %d is at %.3g x the bound against the float64 oracle" % (name, b, r)
        o += size


@functools.lru_cache(maxsize=None)
def lstm_sizes():
    eng = NutlsEngine(WF.container("plain"), batch=1)
    sizes = tuple(state_layout(eng))
    eng.close()
    return sizes


def noise(shape, seed, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def noise16(shape, seed):
    return np.clip(np.round(noise(shape, seed, 0.2) * 32768.0), -32768, 32767).astype(np.int16)


# ---- a. the model step ---------------------------------------------------------------------------------------------------------------
def steps_case(q, blob, B, G, x, variant="lstm", mode=None, ctfa=None, masks=None, edit_after=None, host_call=None, host_at=()):
    """x [F, B, 256] through ``step``; masks [F, B] uint8 (device masks written behind the gate); ``edit_after``: after that many frames
    a state tensor is read, changed and written back (host-blocking); ``host_call(eng, k)``: the k-th host call, made in front of the
    frames of ``host_at``."""
    eng = NutlsEngine(blob, batch=B, streams_per_workgroup=G, variant=variant, mode=mode)
    if ctfa:
        eng.set_ctfa_mode(ctfa)
    X, O = q.input(x), q.output(x.shape)
    M = None if masks is None else q.input(masks)
    q.open()
    with q:
        k = 0
        for f in range(x.shape[0]):
            if edit_after == f:
                q.check_held()
                name = eng.state_specs()[0][0]
                v = eng.state_get(name)
                eng.state_set(name, 0.5 * v + 0.25)
            if f in host_at:
                q.check_held()
                host_call(eng, k)
                k += 1
            q.call(eng.step, X[f], out=O[f], active=None if M is None else M[f])
    q.close()
    res = {"out": O.cpu().numpy(), "states": all_states(eng, B)}
    eng.close()
    return res


@pytest.mark.parametrize("G,B", [(1, 3), (2, 4), (4, 8)])
def test_stream_order_step_fused_plans(G, B):
    ref = WF.reference("plain")
    s = both(steps_case, WF.container("plain"), B, G, WF.inputs(B), what="step, %d-stream plan" % G)
    idx = np.arange(B) % 4
    check_oracle(s, ref.out[:, idx], ref.state, idx, lstm_sizes())


@pytest.mark.parametrize("mode", ["launches", "graph"])
def test_stream_order_step_per_layer_modes(mode):
    """Mode 0, and mode 1: the graphs are captured on the handle's private stream and replayed on a stream they were not captured on."""
    ref = WF.reference("plain")
    s = both(steps_case, WF.container("plain"), 2, None, WF.inputs(2), mode=mode, what="step, mode " + mode)
    check_oracle(s, ref.out[:, :2], ref.state, [0, 1], lstm_sizes())


BASE_CUT = 12          # frames of the baseline case: the dilated rings (d = 1, 2, 4, 8) wrap


@functools.lru_cache(maxsize=None)
def baseline_cut_reference():
    return WF._oracle(WF.container("plain", variant="baseline"), WF.inputs(3, "baseline")[:BASE_CUT], torch.float64, trace=False, variant="baseline")


def test_stream_order_step_baseline_fused():
    s = both(steps_case, WF.container("plain", variant="baseline"), 3, None, WF.inputs(3, "baseline")[:BASE_CUT], variant="baseline",
             what="step, baseline fused")
    check_oracle(s, baseline_cut_reference().out)      # (the states: tests/test_gpu_baseline_families.py has the rings' own comparison)


CAUSAL_CUT = 34        # the history ring's slot wraps at 32, launch_ta_sum runs in front of every step


@functools.lru_cache(maxsize=None)
def causal_cut_reference():
    return WF._oracle(WF.container("plain"), np.ascontiguousarray(WF.causal_streams()[:CAUSAL_CUT, :2]), torch.float64, trace=False,
                      ctfa_mode="causal32")


def test_stream_order_step_causal32():
    x = np.ascontiguousarray(WF.causal_streams()[:CAUSAL_CUT, :2])
    s = both(steps_case, WF.container("plain"), 2, 1, x, ctfa="causal32", what="step, causal32 CTFA")
    ref = causal_cut_reference()
    check_oracle(s, ref.out, ref.state, [0, 1], lstm_sizes())


# ---- b. masks -------------------------------------------------------------------------------------------------------------------------
TICKS = 12


@pytest.mark.parametrize("edit", [False, True])
@pytest.mark.parametrize("G", [1, 2, 4])
def test_stream_order_masked_steps(G, edit):
    """Device masks written behind the gate (tests/test_gpu_step_active.py's schedule); ``edit``: three unmasked steps, a state edit, then
    the masked steps -- the launches that write every state until all streams have stepped (lazy_edited, states_materialize(e, s))."""
    B = 8
    masks = schedule(B, TICKS, G, seed=100 + G)
    x = np.ascontiguousarray(np.tile(WF.inputs(B), (TICKS // WF.FRAMES + 1, 1, 1))[:TICKS + 3])
    if edit:
        masks = np.concatenate([np.ones((3, B), np.uint8), masks])
        both(steps_case, WF.container("plain"), B, G, x, masks=masks, edit_after=3, what="state_set, then masked steps, %d-stream plan" % G)
    else:
        both(steps_case, WF.container("plain"), B, G, x[:TICKS], masks=masks, what="masked steps, %d-stream plan" % G)


# ---- c. the hop entries ----------------------------------------------------------------------------------------------------------------
def hops_case(q, kind, B=4, hops=6, G=1, fusion=False, atten=None, fmt=None, upper=0.0, follow=False, masked=False, host_call=None, host_at=(),
              lazy_format=False, first_blocks=False):
    """``kind``: "enhance" (enhance_hop / enhance_hop_pcm when ``fmt`` is given), "halves" (stft_hop, step on the library buffers,
    istft_hop) or "codec" (pcm_decode_hop, pcm_encode_hop).  ``lazy_format``: the format, the upper band and follow are set INSIDE the
    gated sequence, as the handle's very first calls; ``first_blocks``: the first call of the sequence allocates and zeroes the gateway's
    buffers and synchronises the device while it does (pcm_init): the gate is checked in front of it."""
    eng = NutlsEngine(WF.container("plain"), batch=B, streams_per_workgroup=G, hop_fusion=True if fusion else None)
    if atten is not None:
        eng.set_atten_limit(atten)

    def set_format():
        eng.set_pcm_format(*fmt)
        if upper:
            eng.set_pcm_upper_band(upper)
        if follow:
            eng.set_pcm_upper_follow(True)
    if fmt and not lazy_format:
        set_format()
    rate, dtype = fmt or (16000, "float32")
    S = 256 * rate // 16000
    x = noise16((hops, B, S), 7) if dtype == "int16" else noise((hops, B, S), 7)
    X, O = q.input(x), q.output(x.shape, dtype)
    D = q.output((hops, B, 256)) if kind == "codec" else None
    M = None
    if masked:
        m = (np.random.default_rng(5).random((hops, B)) < 0.6).astype(np.uint8)
        m[0], m[2, :] = 1, 0
        m[3, 1] = 0
        M = q.input(m)
    q.open()
    with q:
        if lazy_format or first_blocks:
            q.check_held()
        if fmt and lazy_format:
            set_format()
        k = 0
        for f in range(hops):
            if f in host_at:
                q.check_held()
                if host_call(eng, k) == "reformat":      # (the rest of the hops in the new format: inputs the host call made are real already)
                    x2 = noise((hops, B, eng.pcm_hop_samples), 8)
                    X, O2 = torch.from_numpy(x2).cuda(), q.output(x2.shape)
                    O = [O[i] if i < f else O2[i] for i in range(hops)]
                k += 1
            a = None if M is None else M[f]
            if kind == "enhance" and fmt:
                q.call(eng.enhance_hop_pcm, X[f], out=O[f], active=a)
            elif kind == "enhance":
                q.call(eng.enhance_hop, X[f], out=O[f], active=a)
            elif kind == "halves":
                q.call(eng.stft_hop, X[f])
                q.call(eng.step_resident, torch.cuda.current_stream().cuda_stream)
                q.call(eng.istft_hop, O[f])
            else:
                q.call(eng.pcm_decode_hop, X[f], out=D[f], active=a)
                q.call(eng.pcm_encode_hop, D[f], out=O[f], active=a)
    q.close()
    res = {"hop %d" % i: o.cpu().numpy() for i, o in enumerate(O)}
    if kind != "codec":
        res["states"] = all_states(eng, B)
    if D is not None:
        res["decoded"] = D.cpu().numpy()
    if eng.pcm_upper_follow:
        res["follow gain"] = eng.pcm_follow_gain()
    # the overlap tails, previous hops and resampler histories: one more hop of zeros, synchronously
    if kind == "codec":
        z = torch.zeros((B, eng.pcm_hop_samples), dtype=getattr(torch, eng.pcm_dtype), device="cuda")
        res["tail"] = eng.pcm_encode_hop(eng.pcm_decode_hop(z)).cpu().numpy()
    elif kind == "halves":
        eng.stft_hop(torch.zeros((B, 256), device="cuda"))
        res["tail"] = eng.istft_hop(torch.empty((B, 256), device="cuda")).cpu().numpy()
    else:
        z = torch.zeros((B, eng.pcm_hop_samples), dtype=getattr(torch, eng.pcm_dtype), device="cuda")
        res["tail"] = eng.enhance_hop_pcm(z).cpu().numpy()
    torch.cuda.synchronize()
    eng.close()
    return res


HOP_CASES = {
    "three launches": dict(kind="enhance"),
    "hop fusion, one-stream plan": dict(kind="enhance", fusion=True, G=1),
    "hop fusion, two-stream plan": dict(kind="enhance", fusion=True, G=2),
    "attenuation limit": dict(kind="enhance", atten=ATTEN),
    "stft_hop / istft_hop": dict(kind="halves"),
    "int16 48 kHz, upper band, follow, masks": dict(kind="enhance", fmt=(48000, "int16"), upper=1.0, follow=True, masked=True, hops=8),
    "float32 8 kHz, masks": dict(kind="enhance", fmt=(8000, "float32"), masked=True, hops=8),
    "pcm_decode_hop / pcm_encode_hop": dict(kind="codec", fmt=(48000, "int16")),
}


@pytest.mark.parametrize("name", sorted(HOP_CASES))
def test_stream_order_hop_entries(name):
    both(hops_case, what="hops: " + name, **HOP_CASES[name])


# ---- d. the handle's very first call is the gated one ---------------------------------------------------------------------------------
# The front end (frontend_init), the block front end (frontend_block_init) and the chunk streams are allocated by the first call of every
# case of c and e: each runs on a fresh handle.  The PCM state, the upper band and follow are allocated by host-blocking calls.
@pytest.mark.parametrize("name", ["pcm state", "upper band and follow"])
def test_stream_order_first_call_allocates(name):
    if name == "pcm state":      # at 16000 / float32 the halves are the first to need the gateway's buffers
        both(hops_case, kind="codec", first_blocks=True, what="first call: " + name)
    else:
        both(hops_case, kind="enhance", fmt=(48000, "int16"), upper=1.0, follow=True, lazy_format=True, what="first call: " + name)


# ---- e. offline -----------------------------------------------------------------------------------------------------------------------
BLOCKS = WF.BLOCK_SETS[2]["blocks"]
RAGGED = WF.BLOCK_SETS[2]["ragged"]


def block_counts(i):
    return np.asarray(RAGGED.get(i, (BLOCKS[i],) * 2), np.int32)


def blocks_case(q, entry, chunks, ctfa="frame", then_host=False):
    """The two utterances of the block set, blocks of 17 / 1 / 9 frames.  ``entry``: "process", "enhance", their "_ragged" twins (device
    counts written behind the gate), "mix" (stft_block, process_block, istft_block_mix) or "pcm" (int16 / 32 kHz).  ``then_host``: the
    last block goes through the _host entry, with no synchronisation in front of it."""
    U, maxf = 2, max(BLOCKS)
    off = NutlsOffline(WF.container("plain"), max_frames=maxf, utterances=U, ctfa_mode=ctfa, pipeline=chunks)
    ragged = entry.endswith("_ragged")
    base = entry.split("_")[0]
    if base == "mix":
        off.set_atten_limit([0.1, 0.5])
    if base == "pcm":
        off.set_pcm_format(32000, "int16")
    total = sum(BLOCKS)
    if base == "process":
        whole = np.asarray(WF.block_inputs())
        cut = lambda a, n: np.ascontiguousarray(whole[:, a:a + n])
    else:
        unit = 512 if base == "pcm" else 256
        whole = noise16((U, total * unit), 9) if base == "pcm" else noise((U, total * unit), 9)
        cut = lambda a, n: np.ascontiguousarray(whole[:, a * unit:(a + n) * unit])
    starts = WF.block_starts(2)
    host_last = [cut(starts[-1], BLOCKS[-1])] if then_host else []
    dev = list(zip(starts, BLOCKS))[:-1 if then_host else None]
    X = [q.input(cut(a, n)) for a, n in dev]
    O = [q.output(x.shape, "int16" if base == "pcm" else "float32") for x in X]
    C = [q.input(block_counts(i)) if ragged else None for i in range(len(dev))]
    MAG = [q.output((U, n, 256)) for _, n in dev] if base == "mix" else None
    EST = [q.output((U, n, 256)) for _, n in dev] if base == "mix" else None
    q.open()
    res = {}
    with q:
        for i in range(len(dev)):
            if base == "process":
                q.call(off.process_block_device, X[i], out=O[i], frames=C[i])
            elif base == "enhance":
                q.call(off.enhance_block_device, X[i], out=O[i], hops=C[i])
            elif base == "pcm":
                q.call(off.enhance_block_pcm_device, X[i], out=O[i], hops=C[i])
            else:
                q.call(off.stft_block_device, X[i], out=MAG[i])
                q.call(off.process_block_device, MAG[i], out=EST[i])
                q.call(off.istft_block_device, EST[i], out=O[i], noisy=MAG[i])
        if then_host:
            q.check_held()
            if base == "process":
                res["host block"] = off.process(host_last[0])
            elif base == "enhance":
                res["host block"] = off.enhance_block_host(host_last[0])
            else:
                res["host block"] = off.enhance_block_pcm_host(host_last[0])
    q.close()
    for i, o in enumerate(O):
        res["block %d" % i] = o.cpu().numpy()
    res["states"] = all_states(off, U)
    if base != "process":      # previous hops, overlap tails and resampler histories: one more hop of zeros, synchronously
        if base == "pcm":
            res["tail"] = off.enhance_block_pcm_device(torch.zeros((U, 512), dtype=torch.int16, device="cuda")).cpu().numpy()
        else:
            res["tail"] = off.enhance_block_device(torch.zeros((U, 256), device="cuda")).cpu().numpy()
        torch.cuda.synchronize()
    off.close()
    return res


@pytest.mark.parametrize("chunks", [1, 2, 3])
@pytest.mark.parametrize("entry", ["process", "process_causal32", "process_ragged", "enhance", "enhance_ragged", "mix", "pcm", "pcm_ragged"])
def test_stream_order_offline_blocks(entry, chunks):
    ctfa = "frame"
    if entry == "process_causal32":
        entry, ctfa = "process", "causal32"
    s = both(blocks_case, entry, chunks, ctfa=ctfa, what="blocks: %s, %s CTFA, %d chunk%s" % (entry, ctfa, chunks, "s" * (chunks > 1)))
    if entry == "process" and ctfa == "frame":
        ref = WF.block_reference("plain")
        for i, (a, n) in enumerate(zip(WF.block_starts(2), BLOCKS)):
            for u in range(2):
                r = WF.scaled_rms(s["block %d" % i][u], ref.out[a:a + n, u]) / WF.OUT_BOUND
                assert r < 1.0, "block %d, utterance %d is at %.3g x the bound against the float64 oracle" % (i, u, r)
        o = 0
        for name, size in lstm_sizes():
            for u in range(2):
                r = WF.scaled_rms(s["states"][u, o:o + size], ref.state[name][u].reshape(-1)) / WF.STATE_BOUND
                assert r < 1.0, "state %s of utterance %d is at %.3g x the bound against the float64 oracle" % (name, u, r)
            o += size


# ---- f. host calls in the middle of queued work ---------------------------------------------------------------------------------------
def _set_modes(eng, k):
    eng.set_mode(("launches", "fused")[k])


STEP_HOST_CALLS = {
    "reset(b)": dict(host_call=lambda eng, k: eng.reset(1), host_at=(3,)),
    "state_get / state_set": dict(edit_after=3),
    "set_mode 3 -> 0 -> 3": dict(host_call=_set_modes, host_at=(2, 4)),
    "set_ctfa_mode": dict(host_call=lambda eng, k: eng.set_ctfa_mode("causal32"), host_at=(3,)),
}


def _reformat(eng, k):
    eng.set_pcm_format(8000, "float32")
    return "reformat"


def _fusion(eng, k):
    eng.set_hop_fusion(k == 0)


HOP_HOST_CALLS = {
    "set_pcm_format": dict(kind="enhance", fmt=(48000, "int16"), host_call=_reformat, host_at=(3,)),
    "set_atten_limit": dict(kind="enhance", host_call=lambda eng, k: eng.set_atten_limit(ATTEN), host_at=(3,)),
    "set_hop_fusion": dict(kind="enhance", host_call=_fusion, host_at=(2, 4)),
}


@pytest.mark.parametrize("name", sorted(STEP_HOST_CALLS) + sorted(HOP_HOST_CALLS))
def test_stream_order_host_call_amid_queued_work(name):
    """The host call is made while the gated stream is still busy with the calls in front of it."""
    if name in STEP_HOST_CALLS:
        both(steps_case, WF.container("plain"), 4, 1, WF.inputs(4), what="host call: " + name, **STEP_HOST_CALLS[name])
    else:
        both(hops_case, what="host call: " + name, **HOP_HOST_CALLS[name])


# ---- g. the stream changes between two calls on one handle, with no synchronisation between them ------------------------------------------
def change_case(q, second):
    """Three steps on the run's stream (gated in G), then three steps ``second``: "host" (the _host entry on numpy frames, which runs on the
    handle's private stream), "side" (another, idle side stream) or "null" (stream = NULL)."""
    B = 4
    x = WF.inputs(B)
    eng = NutlsEngine(WF.container("plain"), batch=B, streams_per_workgroup=1)
    X, O = q.input(x), q.output(x.shape)
    other = {"side": side_streams()[1] if q.gated else torch.cuda.default_stream(), "null": torch.cuda.default_stream()}.get(second)
    host_out = []
    q.open()
    with q:
        for f in range(3):
            q.call(eng.step, X[f], out=O[f])
    q.check_held()
    if second == "host":
        for f in range(3, WF.FRAMES):
            host_out.append(eng.step(x[f]).copy())
    else:
        with torch.cuda.stream(other):
            for f in range(3, WF.FRAMES):
                q.call(eng.step, X[f], out=O[f])
    q.close()
    res = {"out": O.cpu().numpy()[:3 if second == "host" else None], "states": all_states(eng, B)}
    if host_out:
        res["host out"] = np.stack(host_out)
    eng.close()
    return res


@pytest.mark.parametrize("second", ["host", "side", "null"])
def test_stream_order_stream_changes_between_steps(second):
    ref = WF.reference("plain")
    s = both(change_case, second, what="step on the gated stream, then " + second)
    out = s["out"] if second != "host" else np.concatenate([s["out"], s["host out"]])
    check_oracle({"out": out, "states": s["states"]}, ref.out, ref.state, range(4), lstm_sizes())


def hop_then_host_case(q, fmt):
    """Three hops on the run's stream, then three through the _host entry (numpy), no synchronisation in front of them."""
    B = 4
    eng = NutlsEngine(WF.container("plain"), batch=B, streams_per_workgroup=1)
    if fmt:
        eng.set_pcm_format(*fmt)
    S = eng.pcm_hop_samples
    x = noise16((6, B, S), 7) if fmt else noise((6, B, S), 7)
    X, O = q.input(x[:3]), q.output(x[:3].shape, eng.pcm_dtype)
    q.open()
    with q:
        for f in range(3):
            q.call(eng.enhance_hop_pcm, X[f], out=O[f])
    q.check_held()
    host = [eng.enhance_hop_pcm(np.ascontiguousarray(x[f])).copy() for f in range(3, 6)]
    q.close()
    res = {"out": O.cpu().numpy(), "host out": np.stack(host), "states": all_states(eng, B)}
    res["tail"] = eng.enhance_hop_pcm(np.zeros((B, S), x.dtype))
    eng.close()
    return res


@pytest.mark.parametrize("fmt", [None, (48000, "int16")], ids=["enhance_hop", "enhance_hop_pcm"])
def test_stream_order_hop_then_host_entry(fmt):
    both(hop_then_host_case, fmt, what="hops on the gated stream, then the _host entry")


@pytest.mark.parametrize("entry", ["process", "enhance", "pcm"])
def test_stream_order_block_then_host_entry(entry):
    both(blocks_case, entry, 2, then_host=True, what="blocks on the gated stream, then the _host entry: " + entry)


# ---- h. two handles on two gated side streams, interleaved call by call -------------------------------------------------------------------
def two_handles(gated, kinds):
    """-> the results of the two handles.  ``kinds[i]``: (G, fusion) of handle i; both take enhance_hop, call by call in turn."""
    B, hops = 4, 6
    qs = [Seq(gated, "two handles, handle %d" % i, slot=i) for i in range(2)]
    engs = [NutlsEngine(WF.container("plain"), batch=B, streams_per_workgroup=G, hop_fusion=True if fusion else None) for G, fusion in kinds]
    xs = [noise((hops, B, 256), 20 + i) for i in range(2)]
    X = [q.input(x) for q, x in zip(qs, xs)]
    O = [q.output(x.shape) for q, x in zip(qs, xs)]
    torch.cuda.synchronize()
    for q in qs:
        q.open(sync=False)
    for f in range(hops):
        for i, q in enumerate(qs):
            with q:
                q.call(engs[i].enhance_hop, X[i][f], out=O[i][f])
    for q in qs:
        q.check_held()
    for q in qs:
        q.close()
    res = []
    for i, eng in enumerate(engs):
        res.append({"out": O[i].cpu().numpy(), "states": all_states(eng, B)})
        eng.close()
    return res


@pytest.mark.parametrize("kinds", [((1, False), (2, False)), ((1, True), (2, True)), ((1, True), (1, False))],
                         ids=["plans 1 and 2", "hop builds 1 and 2", "hop build and three launches"])
def test_stream_order_two_handles_two_streams(kinds):
    """Shared statics (the kernels' attributes, the page-locked map): each handle equals its own synchronous run."""
    s, g = two_handles(False, kinds), two_handles(True, kinds)
    for i in range(2):
        assert np.isfinite(s[i]["out"]).all()
        assert_same(s[i], g[i], "two handles, handle %d" % i)
    assert not same_bits(s[0]["out"], s[1]["out"])
