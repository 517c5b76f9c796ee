"""``-m gpu``: every kernel family of the LSTM variant on synthetic and edge-case weights (tests/weight_families.py) against oracle B in
float64 -- the one-, two- and four-stream fused step kernels, the profiling build, both hop builds, the per-layer kernels and the block
mode in both conv flavours plus its LSTM scan.  Until this file the only weights those kernels ever saw were the trained ones.

Bounds: the project's own (tests/test_gpu_packed.py, tests/test_gpu_trace.py, tests/test_gpu_hop_fusion.py), now against the float64
oracle -- outputs RMS < 2e-5 x max(1, max|want|), traced tensors 2e-5 relative RMS, each of the 130 states of every stream
RMS < 1e-4 x max(1, max|want|), device path against device path 1e-6 RMS / 1e-5 relative RMS.  tests/test_weight_families.py shows that
the float32 oracle itself uses at most 1/20 of each on every family.  Every test prints its worst ratio to the bound; a failure names the
first offending tensor in the order of the fused plan, so that it points at an op.

Reference semantics: one step of the signature, /root/reference/dnn_model/converter_proposed.py:188-867."""
import ctypes

import numpy as np
import pytest

import weight_families as WF
from nunet_amd import NutlsEngine, NutlsOffline
from nunet_amd.runner import load_library
from nunet_amd.weights import quantize_like_export, write_blob

pytestmark = pytest.mark.gpu

DEVICE_RMS = 1e-6          # device path against device path, outputs (tests/test_gpu_packed.py, tests/test_gpu_parity.py)
DEVICE_REL = 1e-5          # device path against device path, waveforms (tests/test_gpu_hop_fusion.py)
LAST_OP = "msfe6_de_ctfa"  # the op that also holds the output conv


class Ledger:
    """Ratios to the bound, by tensor label, with the op each tensor belongs to."""

    def __init__(self, what, plan=()):
        self.what, self.plan, self.ratio, self.op, self.device = what, list(plan), {}, {}, set()

    def add(self, label, op, ratio, device=False):
        """``device``: a comparison of two device paths (printed apart from the comparisons with the oracle)"""
        ratio = float(ratio) if np.isfinite(ratio) else float("inf")
        if ratio >= self.ratio.get(label, -1.0):
            self.ratio[label], self.op[label] = ratio, op
        if device:
            self.device.add(label)

    def outputs(self, got, want, frame, prefix=""):
        assert np.isfinite(got).all(), "%s: %soutput of frame %d is not finite" % (self.what, prefix, frame)
        self.add("%soutput, frame %d" % (prefix, frame), LAST_OP, WF.scaled_rms(got, want) / WF.OUT_BOUND)

    def states(self, eng, want, streams, prefix="", only=None):
        """all 130 states of every stream of ``eng``; ``streams[b]``: the base stream that stream b of the handle carries; ``only``: the
        streams of the handle to look at (all otherwise)"""
        for name in WF.state_names():
            got = eng.state_get(name)
            for b, s in enumerate(streams):
                if only is None or b in only:
                    self.add("%sstate %s, stream %d" % (prefix, name, b), WF.state_consumer(name),
                             WF.scaled_rms(got[b].reshape(-1), want[name][s].reshape(-1)) / WF.STATE_BOUND)

    def close(self):
        for kind, labels in (("against the float64 oracle", [k for k in self.ratio if k not in self.device]), ("between device paths", sorted(self.device))):
            if labels:
                worst = max(labels, key=self.ratio.get)
                print("%s: %d quantities %s, worst ratio to the bound %.3f (%s)" % (self.what, len(labels), kind, self.ratio[worst], worst))
        bad = {k: self.op[k] for k, r in self.ratio.items() if not r < 1.0}
        if bad:
            first = WF.first_in_plan_order(self.plan, bad) if self.plan else sorted(bad)[0]
            pytest.fail("%s: %d of %d quantities miss their bound; first in plan order: %s (op %s) at %.3g x the bound"
                        % (self.what, len(bad), len(self.ratio), first, bad[first], self.ratio[first]))


# ---- a. one-stream plan: profiling build with the trace, then the production kernel ----------------------------------------------------
@pytest.mark.parametrize("family", WF.FAMILIES)
def test_one_stream_plan_trace_states_and_production_kernel(family):
    """B = 3 (odd).  Profiling build (`debug_trace`): outputs, the 18 traced tensors of every frame and the 130 states after frame 6 against
    the float64 oracle; then a fresh handle on the production kernel: the same outputs within 1e-6 RMS, the oracle's within the bounds,
    all 130 states again."""
    B = 3
    blob, ref, x = WF.container(family), WF.reference(family), WF.inputs(B)
    eng = NutlsEngine(blob, batch=B, streams_per_workgroup=1)
    assert eng.mode == "fused" and eng.streams_per_workgroup == 1
    led = Ledger("%s, one-stream plan, profiling build" % family, eng.fused_plan())
    eng.debug_trace(True)
    traced_out = []
    for f in range(WF.FRAMES):
        out = eng.step(x[f])
        traced_out.append(out.copy())
        led.outputs(out, ref.out[f, :B], f)
        for name in WF.traced_names():
            got = eng.debug_get(name, WF.traced_shape(name))
            led.add("traced %s, frame %d" % (name, f), WF.traced_op(name), WF.rel_rms(got, ref.trace[name][f, :B]) / WF.TRACE_BOUND)
    led.states(eng, ref.state, range(B))
    plan = led.plan
    eng.close()
    assert len(led.ratio) == WF.FRAMES * (1 + 18) + 130 * B
    led.close()
    eng = NutlsEngine(blob, batch=B, streams_per_workgroup=1)
    eng.debug_trace(False)
    led = Ledger("%s, one-stream plan, production kernel" % family, plan)
    for f in range(WF.FRAMES):
        out = eng.step(x[f])
        led.outputs(out, ref.out[f, :B], f)
        led.add("output against the profiling build, frame %d" % f, LAST_OP, WF.rms(out, traced_out[f]) / DEVICE_RMS, device=True)
    led.states(eng, ref.state, range(B))
    eng.close()
    led.close()


# ---- b. packed plans ---------------------------------------------------------------------------------------------------------------------
PACKED = {2: (4, [[0, 1, 2, 3], [1, 0, 0, 1], [3, 2, 2, 3]]),
          4: (8, [[0, 1, 2, 3, 0, 1, 2, 3], [1, 0, 3, 2, 2, 3, 0, 1]])}


@pytest.mark.parametrize("family", WF.FAMILIES)
@pytest.mark.parametrize("G", [2, 4])
def test_packed_plans_outputs_states_and_slot_independence(family, G):
    """Two workgroups of the two-stream (B = 4) and of the four-stream plan (B = 8): outputs of every frame and all 130 states of every
    slot against the float64 oracle.  Then the same handle, reset, with the base streams in other slots and workgroups: every copy of a
    base stream, in whatever slot, next to whatever partners, in whichever pass, gives bit-identical outputs."""
    B, passes = PACKED[G]
    blob, ref, base = WF.container(family), WF.reference(family), WF.base_streams()
    eng = NutlsEngine(blob, batch=B, streams_per_workgroup=G)
    assert eng.mode == "fused" and eng.streams_per_workgroup == G
    led = Ledger("%s, %d-stream plan" % (family, G), eng.fused_plan())
    seen = {}
    for p, idx in enumerate(passes):
        if p:
            eng.reset()
        for f in range(WF.FRAMES):
            out = eng.step(np.ascontiguousarray(base[f][idx]))
            if p == 0:
                led.outputs(out, ref.out[f][idx], f)
            for b, s in enumerate(idx):
                first = seen.setdefault((f, s), out[b].copy())
                assert np.array_equal(out[b], first), "pass %d, frame %d: base stream %d in slot %d differs from its first copy" % (p, f, s, b)
        if p == 0:
            led.states(eng, ref.state, idx)
    eng.close()
    assert len(led.ratio) == WF.FRAMES + 130 * B
    led.close()


# ---- c. per-layer kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["plain", "satbias", "const", "gatesat", "gatedead", "gatehist"])
def test_per_layer_kernels(family):
    """hipGraph replay and plain launches of the per-layer kernels on the shipped-form container: outputs and all 130 states of the four
    base streams against the float64 oracle, the two modes bit-identical to each other (as test_execution_modes_agree asserts)."""
    B = 4
    blob, ref, x = WF.container(family), WF.reference(family), WF.inputs(B)
    a, b = NutlsEngine(blob, batch=B, mode="graph"), NutlsEngine(blob, batch=B, mode="launches")
    led = Ledger("%s, per-layer kernels" % family)
    for f in range(WF.FRAMES):
        oa, ob = a.step(x[f]), b.step(x[f])
        assert np.array_equal(oa, ob), f
        led.outputs(oa, ref.out[f], f)
    led.states(a, ref.state, range(B))
    for name in WF.state_names():
        assert np.array_equal(a.state_get(name), b.state_get(name)), name
    a.close()
    b.close()
    led.close()


def test_per_layer_kernels_float_container():
    """The float container of `plain` (no quantisation on either side): the library's own choice for it is the hipGraph replay."""
    B = 4
    blob, ref, x = WF.container("plain", "float"), WF.reference("plain", form="float"), WF.inputs(B)
    eng = NutlsEngine(blob, batch=B)
    assert eng.mode == "graph"
    led = Ledger("plain (float container), per-layer kernels")
    for f in range(WF.FRAMES):
        led.outputs(eng.step(x[f]), ref.out[f], f)
    led.states(eng, ref.state, range(B))
    eng.close()
    led.close()


# ---- d. carried partial sums rebuilt on synthetic weights ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["scales", "forms_single_scale_convs"])
@pytest.mark.parametrize("B,G", [(3, 1), (4, 2)])
def test_carried_sums_rebuilt_after_state_write_back(family, B, G):
    """After frame 3 every state is written back (`state_set(name, state_get(name))`): the library rebuilds the carried partial sums from
    the packed weights and their per-channel (or single) scales.  Frames 4-6 still meet the oracle bounds and stay within 1e-6 RMS of a
    handle that never was interrupted; so do the final states."""
    blob, ref, x = WF.container(family), WF.reference(family), WF.inputs(B)
    a, b = (NutlsEngine(blob, batch=B, streams_per_workgroup=G) for _ in range(2))
    assert b.mode == "fused" and b.streams_per_workgroup == G
    led = Ledger("%s, %d-stream plan, states written back after frame 3" % (family, G), b.fused_plan())
    for f in range(WF.FRAMES):
        if f == 3:
            for name in WF.state_names():
                b.state_set(name, b.state_get(name))
        oa, ob = a.step(x[f]), b.step(x[f])
        led.outputs(ob, ref.out[f][np.arange(B) % 4], f)
        led.add("output against the uninterrupted handle, frame %d" % f, LAST_OP, WF.rms(oa, ob) / DEVICE_RMS, device=True)
    led.states(b, ref.state, np.arange(B) % 4)
    a.close()
    b.close()
    led.close()


# ---- e. hop builds -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["plain", "satbias"])
@pytest.mark.parametrize("B,G", [(3, 1), (4, 2)])
def test_hop_builds_against_the_three_launch_path(family, B, G):
    """`hop_fusion=True` (STFT and inverse STFT inside the hop build of the step kernel) against analysis, step and synthesis in a launch
    each, same container, 4 hops of seeded noise at 0.05: 1e-5 relative RMS on the waveform (tests/test_gpu_hop_fusion.py)."""
    blob = WF.container(family)
    pcm = (0.05 * np.random.default_rng(WF.SEED + 4).standard_normal((4, B, 256))).astype(np.float32)
    three, one = NutlsEngine(blob, batch=B, streams_per_workgroup=G), NutlsEngine(blob, batch=B, streams_per_workgroup=G, hop_fusion=True)
    assert (three.launches_per_hop, one.launches_per_hop) == (3, 1) and one.streams_per_workgroup == G
    want = np.concatenate([three.enhance_hop(pcm[i]) for i in range(4)], axis=1)
    got = np.concatenate([one.enhance_hop(pcm[i]) for i in range(4)], axis=1)
    three.close()
    one.close()
    assert np.isfinite(got).all() and float(np.abs(want).max()) > 1e-3
    led = Ledger("%s, hop build of the %d-stream plan" % (family, G))
    for b in range(B):
        led.add("waveform, stream %d" % b, LAST_OP, WF.rel_rms(got[b], want[b]) / DEVICE_REL, device=True)
    led.close()


# ---- f. block mode -------------------------------------------------------------------------------------------------------------------------
def _run_blocks(blob):
    off = NutlsOffline(blob, max_frames=17, utterances=2)
    x = WF.block_inputs()
    outs, a = [], 0
    for n in (17, 1, 9):          # a full 16-frame scan round plus a guarded step; a one-frame block; one group plus one frame
        outs.append(off.process(x[:, a:a + n]))
        a += n
    states = {name: off.state_get(name) for name in ("msfe4_en_h", "state_c", "msfe6_ee_prev1")}
    off.close()
    return np.concatenate(outs, axis=1), states


@pytest.mark.parametrize("family", WF.BLOCK_FAMILIES)
def test_block_mode_both_conv_flavours(family, monkeypatch):
    """Two utterances, 27 frames in blocks of 17, 1 and 9: the bf16-pipe convs (the default for int8 containers) and the fp32-MFMA convs
    (NUTLS_OFFLINE_FP32=1), each with the LSTM scan, against the float64 oracle run frame by frame; within 1e-6 RMS of each other; three
    carried states after the last block."""
    blob, ref = WF.container(family), WF.block_reference(family)
    monkeypatch.delenv("NUTLS_OFFLINE_FP32", raising=False)
    got = {"bf16 pipe": _run_blocks(blob)}
    monkeypatch.setenv("NUTLS_OFFLINE_FP32", "1")
    got["fp32"] = _run_blocks(blob)
    led = Ledger("%s, block mode" % family)
    for flavour, (out, states) in got.items():
        assert out.shape == (2, WF.BLOCK_FRAMES, 256)
        for f in range(WF.BLOCK_FRAMES):
            led.outputs(out[:, f], ref.out[f], f, prefix=flavour + ": ")
        for name, st in states.items():
            for u in range(2):
                led.add("%s: state %s, utterance %d" % (flavour, name, u), WF.state_consumer(name),
                        WF.scaled_rms(st[u].reshape(-1), ref.state[name][u].reshape(-1)) / WF.STATE_BOUND)
    led.add("bf16 pipe against fp32, all frames", LAST_OP, WF.rms(got["bf16 pipe"][0], got["fp32"][0]) / DEVICE_RMS, device=True)
    led.close()


# ---- g. refusals stay refusals ---------------------------------------------------------------------------------------------------------------
def _create(lib, blob, spw):
    """nutls_create (spw None) / nutls_create_plan on the raw ABI -> (return code, message, handle)"""
    h = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(blob, len(blob))
    if spw is None:
        rc = lib.nutls_create(buf, len(blob), 0, 2, 0, ctypes.byref(h))
    else:
        rc = lib.nutls_create_plan(buf, len(blob), 0, 2, 0, spw, ctypes.byref(h))
    return rc, lib.nutls_last_error().decode("utf-8", "replace"), h


def _partly_int8():
    q = quantize_like_export(WF.family_tensors("plain"), "shipped")
    q["msfe4_en_conv2.w"] = WF.family_tensors("plain")["msfe4_en_conv2.w"]          # one conv kernel left float
    return write_blob(q), "msfe4_en_conv2.w"


def _per_row_wx():
    w = WF.family_tensors("plain")
    q = quantize_like_export(w, "shipped")
    a = w["msfe5_de_lstm.wx"]
    amax = np.abs(a).max(axis=1)
    sc = (amax / 127.0).astype(np.float32)
    q["msfe5_de_lstm.wx"] = (np.clip(np.rint(a / sc[:, None]), -127, 127).astype(np.int8), sc)          # 84 scales, one per row
    return write_blob(q), "msfe5_de_lstm.wx"


@pytest.mark.parametrize("make", [_partly_int8, _per_row_wx])
def test_containers_the_packer_refuses(make):
    """Only some conv kernels int8, or an LSTM kernel with per-row scales: `nutls_create` runs such a container on the per-layer kernels
    (checked against the float64 oracle on its de-quantised tensors), an explicit plan request is NUTLS_ERR_WEIGHTS with a message that
    names the tensor.  Neither crashes."""
    import torch
    blob, tensor = make()
    lib = load_library()
    for spw in (1, 2):
        rc, msg, h = _create(lib, blob, spw)
        assert rc == -2 and not h.value, (rc, msg)
        assert tensor in msg, msg
    rc, msg, h = _create(lib, blob, None)
    assert rc == 0 and h.value, (rc, msg)
    lib.nutls_destroy(h)
    eng = NutlsEngine(blob, batch=4)
    assert eng.mode == "graph"
    with pytest.raises(ValueError):
        eng.set_mode("fused")
    x = WF.inputs(4)
    ref = WF._oracle(blob, x[:2], torch.float64, trace=False)
    led = Ledger("refused container (%s), per-layer kernels" % tensor)
    for f in range(2):
        led.outputs(eng.step(x[f]), ref.out[f], f)
    eng.close()
    led.close()
