"""``-m gpu``: the dilated-dense baseline's kernels on synthetic and edge-case weights (the baseline half of tests/weight_families.py)
against oracle B in float64 over 37 frames -- the fused plan (`fused_base.hip` and its profiling build: csrc/ddb_fused.hpp), the
per-layer kernels as a hipGraph and as plain launches (csrc/ddb_device.hpp), the history rings at a wrapped phase under `state_set`,
`state_get` and `state_get_all` (csrc/api_state.cpp), and mode switches with wrapped rings.

Bounds: the project's own, as tests/test_gpu_synthetic_weights.py applies them to the LSTM variant -- outputs RMS < 2e-5 x max(1,
max|want|), traced tensors 2e-5 relative RMS, each of the 208 states of every stream RMS < 1e-4 x max(1, max|want|), device path against
device path 1e-6 RMS.  tests/test_baseline_families.py shows that the float32 oracle itself uses at most 1/20 of each on every family.
Every test prints its worst ratio to the bound; a failure names the first offending tensor in the order of the fused plan, and inside a
dilated-dense block the first block output o_0 .. o_6 that is off (the newest frame of ``X_ddb_prevK`` is ``[o_{K-1}, ..., o_0]``).

Reference semantics: the streaming wiring of the block, converter_nunet_tls.py:374-411 of the reference (restated in oracle/nutls_ref.py)."""
import numpy as np
import pytest

import weight_families as WF
from nunet_amd import NutlsEngine
from nunet_amd import topology as T
from test_gpu_synthetic_weights import DEVICE_RMS, LAST_OP, Ledger

pytestmark = pytest.mark.gpu

V = "baseline"
N = WF.BASE_FRAMES


class BaselineLedger(Ledger):
    def states(self, eng, want, streams, prefix=""):
        """all 208 states of every stream of ``eng`` and, apart from them, the outputs o_0 .. o_6 of every dilated-dense block's last
        step; ``streams[b]``: the base stream that stream b of the handle carries"""
        got = {name: eng.state_get(name) for name in WF.state_names(V)}
        for name in WF.state_names(V):
            for b, s in enumerate(streams):
                self.add(prefix + WF.state_label(name, b), WF.state_consumer(name),
                         WF.scaled_rms(got[name][b].reshape(-1), want[name][s].reshape(-1)) / WF.STATE_BOUND)
        for p, f, c in T.bottlenecks():
            tag, g = (p + "_ddb") if p else "ddb", c // 2
            for k in range(T.DDB_BLOCKS + 1):
                ring = "%s_prev%d" % (tag, k + 1) if k < T.DDB_BLOCKS else tag + "_prev_out"
                d = want[ring].shape[1]
                a, w = got[ring].reshape(len(streams), d, f, -1)[:, -1, :, :g], want[ring][:, -1, :, :g]
                for b, s in enumerate(streams):
                    self.add("%s%s o_%d (block %d output, newest frame of %s), stream %d" % (prefix, tag, k, k, ring, b), tag,
                             WF.scaled_rms(a[b], w[s]) / WF.STATE_BOUND)


PER_HANDLE = 208 + 13 * 7          # ledger entries `states` adds per stream


def _family_run(family, B):
    return WF.container(family, variant=V), WF.reference(family, variant=V), WF.inputs(B, V)


# ---- a. the fused plan: profiling build with the trace, then the production kernel -----------------------------------------------------
@pytest.mark.parametrize("family", WF.BASELINE_FAMILIES)
def test_fused_plan_trace_states_and_production_kernel(family):
    """B = 3 (odd).  Profiling build (`debug_trace`): outputs and the 18 traced tensors of every one of the 37 frames and the 208 states
    after the last against the float64 oracle, every block output o_0 .. o_6 of every dilated-dense block on its own; then a fresh handle
    on the production kernel: the same outputs within 1e-6 RMS, the oracle's within the bounds, all states again."""
    B = 3
    blob, ref, x = _family_run(family, B)
    eng = NutlsEngine(blob, batch=B, variant=V)
    assert eng.mode == "fused" and eng.streams_per_workgroup == 1
    plan = eng.fused_plan()
    led = BaselineLedger("baseline %s, fused plan, profiling build" % family, plan)
    eng.debug_trace(True)
    traced_out = []
    for f in range(N):
        out = eng.step(x[f])
        traced_out.append(out.copy())
        led.outputs(out, ref.out[f, :B], f)
        for name in WF.traced_names():
            got = eng.debug_get(name, WF.traced_shape(name))
            led.add("traced %s, frame %d" % (name, f), WF.traced_op(name), WF.rel_rms(got, ref.trace[name][f, :B]) / WF.TRACE_BOUND)
    led.states(eng, ref.state, range(B))
    eng.close()
    assert len(led.ratio) == N * (1 + 18) + PER_HANDLE * B
    led.close()
    eng = NutlsEngine(blob, batch=B, variant=V)
    eng.debug_trace(False)
    led = BaselineLedger("baseline %s, fused plan, production kernel" % family, plan)
    for f in range(N):
        out = eng.step(x[f])
        led.outputs(out, ref.out[f, :B], f)
        led.add("output against the profiling build, frame %d" % f, LAST_OP, WF.rms(out, traced_out[f]) / DEVICE_RMS, device=True)
    led.states(eng, ref.state, range(B))
    eng.close()
    led.close()


# ---- b. per-layer kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["plain", "const", "tinyvar", "alpha"])
def test_per_layer_kernels(family):
    """hipGraph replay and plain launches of the per-layer kernels (the dilated-dense block of csrc/ddb_device.hpp): outputs of the 37
    frames and all 208 states of the four base streams against the float64 oracle, the two modes bit-identical to each other."""
    B = 4
    blob, ref, x = _family_run(family, B)
    a, b = NutlsEngine(blob, batch=B, variant=V, mode="graph"), NutlsEngine(blob, batch=B, variant=V, mode="launches")
    assert (a.mode, b.mode) == ("graph", "launches")
    led = BaselineLedger("baseline %s, per-layer kernels" % family)
    for f in range(N):
        oa, ob = a.step(x[f]), b.step(x[f])
        assert np.array_equal(oa, ob), f
        led.outputs(oa, ref.out[f], f)
    led.states(a, ref.state, range(B))
    for name in WF.state_names(V):
        assert np.array_equal(a.state_get(name), b.state_get(name)), name
    a.close()
    b.close()
    led.close()


def test_per_layer_kernels_float_container():
    """The float container of `plain` (no quantisation on either side): the library's own choice for it is the hipGraph replay."""
    B = 4
    blob, ref, x = WF.container("plain", "float", V), WF.reference("plain", form="float", variant=V), WF.inputs(B, V)
    eng = NutlsEngine(blob, batch=B, variant=V)
    assert eng.mode == "graph"
    led = BaselineLedger("baseline plain (float container), per-layer kernels")
    for f in range(N):
        led.outputs(eng.step(x[f]), ref.out[f], f)
    led.states(eng, ref.state, range(B))
    eng.close()
    led.close()


# ---- c. the history rings at a wrapped phase ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["plain", "scales"])
def test_rings_written_back_and_transplanted_at_a_wrapped_phase(family):
    """After frame 33 (ring phases 1, 1, 1, 1, 1 for depths 2 .. 32: the 32-deep ring has wrapped once) every state is written back
    (`state_set(name, state_get(name))`): frames 34 .. 37 stay within 1e-6 RMS of a handle that never was interrupted and within the bounds
    of the oracle.  Then the states read after frame 37 are set on a FRESH handle, whose rings stand at phase 0, not 5: both take 8 more
    frames and agree within 1e-6 RMS on every one, and the fresh handle's states are the oracle's after frame 45."""
    B = 3
    blob, ref, x = _family_run(family, B)
    tail, cont = WF.inputs(B, V, tail=True), WF.baseline_continuation(family)
    a, b = (NutlsEngine(blob, batch=B, variant=V) for _ in range(2))
    assert a.mode == b.mode == "fused"
    led = BaselineLedger("baseline %s, states written back after frame 33, transplanted after frame 37" % family, b.fused_plan())
    for f in range(N):
        if f == 33:
            for name in WF.state_names(V):
                b.state_set(name, b.state_get(name))
        oa, ob = a.step(x[f]), b.step(x[f])
        led.outputs(ob, ref.out[f, :B], f)
        led.add("output against the uninterrupted handle, frame %d" % f, LAST_OP, WF.rms(oa, ob) / DEVICE_RMS, device=True)
    led.states(b, ref.state, range(B))
    a.close()
    c = NutlsEngine(blob, batch=B, variant=V)
    for name in WF.state_names(V):
        c.state_set(name, b.state_get(name))
    for name in WF.state_names(V):          # what was set is what is read, at the other phase
        assert np.array_equal(c.state_get(name), b.state_get(name)), name
    for f in range(WF.BASE_TAIL):
        ob, oc = b.step(tail[f]), c.step(tail[f])
        led.outputs(oc, cont.out[f, :B], N + f, prefix="fresh handle: ")
        led.add("fresh handle against the one that ran from frame 0, frame %d" % (N + f), LAST_OP, WF.rms(ob, oc) / DEVICE_RMS, device=True)
    led.states(c, cont.state, range(B), prefix="fresh handle after frame %d: " % (N + WF.BASE_TAIL))
    b.close()
    c.close()
    led.close()


# ---- d. state_get_all ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "graph"])
def test_state_get_all_unrotates_like_state_get(mode):
    """`state_get_all(b)` has its own un-rotation of the history rings: after frames 5, 33 and 37 (phases 1 1 5 5 5, all 1, 1 1 5 5 5 with
    the 32-deep ring wrapped) it equals the concatenation of `state_get(name)[b]` in `state_specs()` order bit for bit, for every stream;
    the states themselves are the oracle's after frame 37."""
    B = 3
    blob, ref, x = _family_run("plain", B)
    eng = NutlsEngine(blob, batch=B, variant=V, mode=mode)
    specs = eng.state_specs()
    assert [n for n, _ in specs] == WF.state_names(V)
    checked = 0
    for f in range(N):
        eng.step(x[f])
        if f + 1 in (5, 33, 37):
            each = {n: eng.state_get(n) for n, _ in specs}
            for b in range(B):
                whole, o = eng.state_get_all(b), 0
                for n, (d0, d1) in specs:
                    assert np.array_equal(whole[o:o + d0 * d1], each[n][b].reshape(-1)), "after frame %d, stream %d: %s" % (f + 1, b, n)
                    o += d0 * d1
                assert o == whole.size == T.state_floats_per_stream(V)
                checked += 1
    led = BaselineLedger("baseline plain, %s mode, states behind state_get_all" % mode)
    led.states(eng, ref.state, range(B))
    eng.close()
    assert checked == 3 * B
    led.close()


# ---- e. mode switches with wrapped rings ------------------------------------------------------------------------------------------------------
def test_mode_switches_with_wrapped_rings():
    """`alpha`, 37 frames on ONE handle alternating fused, graph and launches in runs that cross frames 16 and 32 (where the two deepest rings
    wrap): every output against the float64 oracle at the output bound, and the final states."""
    B = 4
    blob, ref, x = _family_run("alpha", B)
    order = ["fused"] * 5 + ["graph"] * 6 + ["launches"] * 3 + ["fused"] * 5 + ["graph"] * 6 + ["launches"] * 9 + ["fused"] * 3
    assert len(order) == N and order[15] == order[16] == "fused" and order[31] == order[32] == "launches"
    eng = NutlsEngine(blob, batch=B, variant=V, mode="fused")
    led = BaselineLedger("baseline alpha, mode switches", eng.fused_plan())
    for f, mode in enumerate(order):
        eng.set_mode(mode)
        led.outputs(eng.step(x[f]), ref.out[f], f, prefix=mode + ": ")
    led.states(eng, ref.state, range(B))
    eng.close()
    assert len(led.ratio) == N + PER_HANDLE * B
    led.close()
