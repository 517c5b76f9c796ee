"""``-m gpu``: the channel-time-frequency attention on designed gate weights (the `gatesat`, `gatedead` and `gatehist` families of
tests/weight_families.py) and in the causal 32-frame mode, against oracle B in float64 (``NutlsRef(ctfa_mode="causal32",
dtype=torch.float64)``).  The three gate families run in frame mode through the parametrised tests of
tests/test_gpu_synthetic_weights.py; this file runs the causal mode, which until now had only seen the trained weights and the float32
oracle (tests/test_gpu_ctfa_modes.py): the streaming ring in the one-, two- and four-stream step kernels, the profiling build and both hop
builds, a history that starts at a non-zero ring slot (after `reset()`, after a mode switch in mid-run), and the offline handle's
history roll with blocks shorter than, equal to and longer than the 31 rows of history, uniform and ragged.

70 frames of `causal_streams`: the ring wraps at 32 and at 64.  Bounds: those of tests/test_gpu_synthetic_weights.py, per frame, against
the float64 oracle; tests/test_ctfa_families.py shows that the float32 oracle uses at most 1/20 of each, and that an attention window of
31 or 33 frames or the frame-mode formula misses the output bound at least ten times over.  Every test prints its worst ratio to the
bound; a failure names the first offending tensor in the order of the fused plan."""
import numpy as np
import pytest
import torch

import weight_families as WF
from nunet_amd import NutlsEngine, NutlsOffline
from test_gpu_synthetic_weights import DEVICE_REL, DEVICE_RMS, LAST_OP, PACKED, Ledger

pytestmark = pytest.mark.gpu

N = WF.CAUSAL_FRAMES


def _engine(blob, B, G, ctfa_mode="causal32", **kw):
    eng = NutlsEngine(blob, batch=B, streams_per_workgroup=G, **kw)
    assert eng.mode == "fused" and eng.streams_per_workgroup == G
    if ctfa_mode != "frame":
        eng.set_ctfa_mode(ctfa_mode)
    return eng


# ---- a. streaming causal32, one-stream plan: profiling build with the trace, then the production kernel -----------------------------------
@pytest.mark.parametrize("family", WF.CAUSAL_FAMILIES)
def test_streaming_causal32_one_stream_plan(family):
    """B = 3 (odd).  Profiling build (`debug_trace`): the outputs of all 70 frames, the 18 traced tensors (12 of them the CTFA outputs) on
    the frames of CAUSAL_TRACE_FRAMES and the 130 states after frame 70 against the float64 oracle; then a fresh handle on the
    production kernel: outputs within 1e-6 RMS of the profiling build's and within the bound of the oracle's, all states again."""
    B = 3
    blob, ref, x = WF.container(family), WF.reference(family, ctfa_mode="causal32"), WF.causal_streams()
    eng = _engine(blob, B, 1)
    led = Ledger("%s, causal32, one-stream plan, profiling build" % family, eng.fused_plan())
    eng.debug_trace(True)
    traced_out = []
    for f in range(N):
        out = eng.step(np.ascontiguousarray(x[f, :B]))
        traced_out.append(out.copy())
        led.outputs(out, ref.out[f, :B], f)
        if f in WF.CAUSAL_TRACE_FRAMES:
            for name in WF.traced_names():
                got = eng.debug_get(name, WF.traced_shape(name))
                led.add("traced %s, frame %d" % (name, f), WF.traced_op(name), WF.rel_rms(got, ref.trace[name][f][:B]) / WF.TRACE_BOUND)
    led.states(eng, ref.state, range(B))
    plan = led.plan
    eng.close()
    assert len(led.ratio) == N + len(WF.CAUSAL_TRACE_FRAMES) * 18 + 130 * B
    led.close()
    eng = _engine(blob, B, 1)
    eng.debug_trace(False)
    led = Ledger("%s, causal32, one-stream plan, production kernel" % family, plan)
    for f in range(N):
        out = eng.step(np.ascontiguousarray(x[f, :B]))
        led.outputs(out, ref.out[f, :B], f)
        led.add("output against the profiling build, frame %d" % f, LAST_OP, WF.rms(out, traced_out[f]) / DEVICE_RMS, device=True)
    led.states(eng, ref.state, range(B))
    eng.close()
    led.close()


# ---- b. packed plans; a history that starts at ring slot 6 and at ring slot 12 -----------------------------------------------------------
@pytest.mark.parametrize("family", WF.CAUSAL_FAMILIES)
@pytest.mark.parametrize("G", [2, 4])
def test_packed_plans_causal32_and_a_history_from_a_later_ring_slot(family, G):
    """Two workgroups of the two-stream (B = 4) and of the four-stream plan (B = 8) in causal32.  First pass: the outputs of every frame and
    all 130 states of every slot against the float64 oracle.  Then `reset()` on the same handle: the handle-wide frame counter stands
    at 70 (140 after the third pass of G = 2) and is not rewound, so the new history starts at ring slot 6 (12), and the base streams
    run in other slots and workgroups (the PACKED permutations).  The outputs of every pass meet the oracle's bound; within a pass every
    copy of a base stream, in whatever slot, next to whatever partners, is bit-identical to the first one.

    Between passes the copies are compared within 1e-6 RMS (device path against device path), not bit for bit: the 31 history rows are
    summed in the order of the ring, which is rotated by 6 rows from pass to pass, and float32 addition in another order rounds
    differently.  The largest difference between passes is printed."""
    B, passes = PACKED[G]
    blob, ref, base = WF.container(family), WF.reference(family, ctfa_mode="causal32"), WF.causal_streams()
    eng = _engine(blob, B, G)
    led = Ledger("%s, causal32, %d-stream plan" % (family, G), eng.fused_plan())
    first_pass, across = {}, 0.0
    for p, idx in enumerate(passes):
        if p:
            eng.reset()
        for f in range(N):
            out = eng.step(np.ascontiguousarray(base[f][idx]))
            led.outputs(out, ref.out[f][idx], f, prefix="pass %d (history from ring slot %d): " % (p, (N * p) % 32))
            seen = {}
            for b, s in enumerate(idx):
                first = seen.setdefault(s, out[b])
                assert np.array_equal(out[b], first), "pass %d, frame %d: base stream %d in slot %d differs from its first copy in this pass" % (p, f, s, b)
                if p == 0:
                    first_pass.setdefault((f, s), out[b].copy())
                else:
                    d = WF.rms(out[b], first_pass[(f, s)])
                    across = max(across, d)
                    led.add("pass %d against pass 0, frame %d" % (p, f), LAST_OP, d / DEVICE_RMS, device=True)
        led.states(eng, ref.state, idx, prefix="pass %d: " % p)
    eng.close()
    print("%s, %d-stream plan: largest RMS difference of a stream's output frame between passes %.3g" % (family, G, across))
    assert len([k for k in led.ratio if k not in led.device]) == len(passes) * (N + 130 * B)
    led.close()


# ---- c. restart in mid-run ---------------------------------------------------------------------------------------------------------------
def test_causal32_stream_reset_in_mid_run():
    """One-stream plan, B = 2, `gatehist`: `reset(1)` after frame 40 (ring slot 8).  Stream 1 then follows the float64 oracle of a fresh
    start on the frames it is fed from there on, stream 0 the uninterrupted one; outputs of every frame, all states at the end."""
    family, B, cut = "gatehist", 2, WF.CAUSAL_RESTART
    blob, ref, fresh, x = WF.container(family), WF.reference(family, ctfa_mode="causal32"), WF.causal_restart_reference(family), WF.causal_streams()
    eng = _engine(blob, B, 1)
    led = Ledger("%s, causal32, reset(1) after frame %d" % (family, cut), eng.fused_plan())
    for f in range(N):
        if f == cut:
            eng.reset(1)
        out = eng.step(np.ascontiguousarray(x[f, :B]))
        led.outputs(out[0], ref.out[f, 0], f, prefix="stream 0: ")
        led.outputs(out[1], ref.out[f, 1] if f < cut else fresh.out[f - cut, 0], f, prefix="stream 1: ")
    led.states(eng, ref.state, (0, 1), only=(0,))
    led.states(eng, fresh.state, (0, 0), only=(1,))
    eng.close()
    assert len(led.ratio) == 2 * N + 130 * B
    led.close()


def test_causal32_mode_switch_in_mid_run():
    """One-stream plan, B = 2, `gatehist`: 10 frames in frame mode, `set_ctfa_mode("causal32")`, 45 more (the new history starts at ring
    slot 10 and wraps at frame 32 of the handle) against a float64 oracle that switches at the same frame: its states carry over, its
    history starts empty."""
    family, B = "gatehist", 2
    n0, n1 = WF.CAUSAL_SWITCH
    blob, ref, x = WF.container(family), WF.causal_switch_reference(family), WF.causal_streams()
    eng = _engine(blob, B, 1, ctfa_mode="frame")
    led = Ledger("%s, frame mode for %d frames, then causal32" % (family, n0), eng.fused_plan())
    for f in range(n0 + n1):
        if f == n0:
            eng.set_ctfa_mode("causal32")
        led.outputs(eng.step(np.ascontiguousarray(x[f, :B])), ref.out[f], f)
    led.states(eng, ref.state, range(B))
    eng.close()
    assert len(led.ratio) == n0 + n1 + 130 * B
    led.close()


# ---- d. hop builds in causal32 --------------------------------------------------------------------------------------------------------------
HOPS = 40
_HOP_ORACLE = {}


def _hop_oracle(family, mags):
    """mags [HOPS, B, 256] (the device's own analysis magnitudes) through the float64 causal32 oracle; kept per stream by content, so that
    a stream that two plans analyse to the same bits runs once."""
    keys = [(family, mags[:, b].tobytes()) for b in range(mags.shape[1])]
    todo = [b for b in range(mags.shape[1]) if keys[b] not in _HOP_ORACLE and keys[b] not in keys[:b]]
    if todo:
        run = WF._oracle(WF.container(family), np.ascontiguousarray(mags[:, todo]), torch.float64, trace=False, ctfa_mode="causal32")
        for i, b in enumerate(todo):
            _HOP_ORACLE[keys[b]] = run.out[:, i]
    return np.stack([_HOP_ORACLE[k] for k in keys], axis=1)


@pytest.mark.parametrize("family", ["plain", "gatehist"])
@pytest.mark.parametrize("B,G", [(3, 1), (4, 2)])
def test_hop_builds_causal32_against_the_three_launch_path(family, B, G):
    """`hop_fusion=True` (the hop builds of the step kernel are compilations of their own of the CTFA op) against analysis, step and
    synthesis in a launch each, both in causal32, 40 hops of seeded noise at 0.05 (the ring wraps once): waveforms and each stream's
    states within 1e-5 relative RMS; the three-launch path's magnitudes of every hop within the output bound of the float64 oracle fed
    the same path's analysis magnitudes."""
    blob = WF.container(family)
    pcm = (0.05 * np.random.default_rng(WF.SEED + 8).standard_normal((HOPS, 4, 256))).astype(np.float32)[:, :B]
    three, one = _engine(blob, B, G), _engine(blob, B, G, hop_fusion=True)
    assert (three.launches_per_hop, one.launches_per_hop) == (3, 1) and one.ctfa_mode == three.ctfa_mode == "causal32"
    want, got, mag_in, mag_out = [], [], [], []
    for i in range(HOPS):
        want.append(three.enhance_hop(np.ascontiguousarray(pcm[i])))
        mag_in.append(three.debug_get("mag_in", (256,)))
        mag_out.append(three.debug_get("mag_out", (256,)))
        got.append(one.enhance_hop(np.ascontiguousarray(pcm[i])))
    want, got = np.concatenate(want, axis=1), np.concatenate(got, axis=1)
    led = Ledger("%s, causal32, hop build of the %d-stream plan" % (family, G), three.fused_plan())
    assert np.isfinite(got).all() and float(np.abs(want).max()) > 1e-3
    for b in range(B):
        led.add("waveform, stream %d" % b, LAST_OP, WF.rel_rms(got[b], want[b]) / DEVICE_REL, device=True)
        led.add("states, stream %d" % b, LAST_OP, WF.rel_rms(one.state_get_all(b), three.state_get_all(b)) / DEVICE_REL, device=True)
    three.close()
    one.close()
    ref = _hop_oracle(family, np.stack(mag_in))
    for i in range(HOPS):
        led.outputs(mag_out[i], ref[i], i, prefix="three-launch path: ")
    led.close()


# ---- e. offline causal32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", WF.CAUSAL_FAMILIES)
@pytest.mark.parametrize("U", [2, 1])
def test_offline_causal32_blocks(family, U):
    """`NutlsOffline(..., ctfa_mode="causal32")` against the float64 oracle run frame by frame.  Two utterances (base streams 0 and 1) in
    blocks of 17, 1, 31, 2 and 19: the history is rolled from a partly filled one, by one frame, by exactly its 31 rows.  One utterance
    (base stream 3) in blocks of 33, 32 and 5: blocks longer than the history.  Outputs of every frame, all 130 states of every
    utterance after every block."""
    streams, blocks = WF.CAUSAL_BLOCKS[U]
    blob, ref = WF.container(family), WF.reference(family, ctfa_mode="causal32")
    x = np.ascontiguousarray(WF.causal_streams()[:, list(streams)].transpose(1, 0, 2))          # [U, frames, 256]
    assert sum(blocks) == N
    off = NutlsOffline(blob, max_frames=max(blocks), utterances=U, ctfa_mode="causal32")
    led = Ledger("%s, offline causal32, %d utterance(s), blocks %s" % (family, U, blocks))
    a = 0
    for i, n in enumerate(blocks):
        out = off.process(x[:, a:a + n])
        assert out.shape == (U, n, 256)
        for f in range(a, a + n):
            led.outputs(out[:, f - a], ref.out[f][list(streams)], f)
        a += n
        led.states(off, ref.states_at[a - 1], streams, prefix="after block %d (%d frames): " % (i, n))
    off.close()
    assert len(led.ratio) == N + len(blocks) * 130 * U
    led.close()


@pytest.mark.parametrize("family", ["plain", "gatehist"])
def test_offline_causal32_ragged_blocks(family):
    """Two utterances, ragged: a block of 17 with counts (17, 0), then a block of 20 with counts (9, 20).  Utterance 1 is held through
    the first call -- its output rows are zero and every state is bit for bit what it was -- and both utterances follow the float64
    oracle at their own frame counts, outputs and all states (a history roll with a count of 0 that moved anything would show in
    utterance 1's second call)."""
    blob, ref = WF.container(family), WF.reference(family, ctfa_mode="causal32")
    x = np.ascontiguousarray(WF.causal_streams()[:, :2].transpose(1, 0, 2))
    off = NutlsOffline(blob, max_frames=max(n for n, _ in WF.CAUSAL_RAGGED), utterances=2, ctfa_mode="causal32")
    led = Ledger("%s, offline causal32, ragged blocks" % family)
    before = {name: off.state_get(name) for name in WF.state_names()}
    done = [0, 0]
    for call, (n, counts) in enumerate(WF.CAUSAL_RAGGED):
        blk = np.stack([x[u, done[u]:done[u] + n] for u in range(2)])
        out = off.process_block_device(torch.from_numpy(blk).cuda(), frames=list(counts)).cpu().numpy()
        for u, c in enumerate(counts):
            assert not out[u, c:].any(), "call %d: utterance %d has non-zero output rows behind its count" % (call, u)
            for f in range(c):
                led.outputs(out[u, f], ref.out[done[u] + f, u], done[u] + f, prefix="utterance %d: " % u)
            done[u] += c
            if c == 0:
                for name in WF.state_names():
                    assert np.array_equal(off.state_get(name)[u], before[name][u]), "call %d: state %s of the held utterance %d moved" % (call, name, u)
            else:
                led.states(off, ref.states_at[done[u] - 1], (0, 1), prefix="after call %d: " % call, only=(u,))
    off.close()
    assert done == [26, 20] and len(led.ratio) == 26 + 20 + 3 * 130
    led.close()
