"""``-m gpu``: streaming and offline handles whose arena offsets pass 2^31 and 2^32, of bytes and of floats, against the float64 oracle.

Every kernel family addresses a stream's (a frame's) slice as ``arena + row * sstride``; at the shapes the rest of the suite runs, that
product stays below 2^31 bytes.  Here the developer knob ``NUTLS_STRIDE_ALIGN`` (floats; ``arena_commit`` reads it when a handle is created)
forces every slice to 2^26 bytes: row 32 starts at 2^31 bytes, row 64 at 2^32 bytes, row 128 at 2^31 floats, row 256 at 2^32 floats, and
handles of 264 and 300 rows cross all four in a few frames.  The stride is addressing alone: the arithmetic, the bounds (those of
tests/test_gpu_synthetic_weights.py) and the references (tests/weight_families.py) are the small handles'.  The rows carry the four base
streams by an index map under which a row whose offset was cut to 31 or 32 bits lands on a row with other data
(``WF.large_index_map``; tests/test_large_offsets.py checks the map, the thresholds and the conditioning of the new references).

Further: the documented offline shape (8 utterances x 1024 frames, 8200 rows of about 2.6 MB at the natural stride) against one-utterance
handles, and the page-locked host path at 1024 streams and on views inside and across the end of a pinned allocation.

Handles are created one after the other, each closed before the next (the largest takes 18.75 GiB of device memory)."""
import ctypes
import os

import numpy as np
import pytest

import weight_families as WF
from conftest import GOLDEN
from test_gpu_synthetic_weights import DEVICE_RMS, LAST_OP, Ledger
from nunet_amd import NutlsEngine, NutlsOffline, host_alloc
from nunet_amd.runner import load_library
from oracle.nutls_ref import NutlsRef

pytestmark = pytest.mark.gpu

KNOB = "NUTLS_STRIDE_ALIGN"
TIGHT_RMS = 2e-5          # tests/test_gpu_parity.py


def _create(monkeypatch, make, rows, env=()):
    """``make()`` with the stride knob (and ``env``) set; the environment is cleared again (the handle has read it).  The device memory
    the handle took shows that its stride is the forced one: at least half of rows x 2^26 bytes (the natural strides are 25 times
    smaller; half, because the figure is the device's, not the process's)."""
    import torch
    monkeypatch.setenv(KNOB, str(WF.STRIDE_ALIGN))
    for var, val in env:
        monkeypatch.setenv(var, val)
    free = torch.cuda.mem_get_info()[0]
    try:
        h = make()
    finally:
        for var in (KNOB,) + tuple(v for v, _ in env):
            monkeypatch.delenv(var, raising=False)
    taken = free - torch.cuda.mem_get_info()[0]
    if taken < rows * WF.ROW_BYTES // 2:
        h.close()
        pytest.fail("the handle took %.2f GiB of device memory, %d rows of 2^26 bytes are %.2f GiB: the stride is not the forced one"
                    % (taken / 2.0 ** 30, rows, rows * WF.ROW_BYTES / 2.0 ** 30))
    return h


def _op(name):
    try:
        return WF.state_consumer(name)
    except ValueError:
        return name


def _rows_ratio(got, want):
    """worst row of ``got [R, 256]`` against ``want``: RMS over max(1, max|want|), as a share of OUT_BOUND"""
    want = np.asarray(want, np.float64)
    d = np.sqrt(np.mean((got.astype(np.float64) - want) ** 2, axis=1)) / np.maximum(1.0, np.abs(want).max(axis=1))
    return float(d.max()) / WF.OUT_BOUND


def _assert_replicas(a, idx, what, skip=()):
    """rows of ``a`` that carry the same base stream are bit-identical (``skip``: rows that no longer are replicas)"""
    for s in range(4):
        rows = [r for r in np.flatnonzero(idx == s) if r not in skip]
        same = a[rows]
        assert np.array_equal(same, np.broadcast_to(same[0], same.shape)), "%s: the rows of base stream %d differ (rows %s)" % (
            what, s, [r for r, v in zip(rows, same) if not np.array_equal(v, same[0])][:8])


def _split(flat, specs):
    res, o = {}, 0
    for name, (d0, d1) in specs:
        res[name] = flat[o:o + d0 * d1]
        o += d0 * d1
    assert o == flat.size
    return res


def _add_states(led, flat, specs, want, row, label):
    """every tensor of one row's `state_get_all` against ``want[name][row]``"""
    for name, got in _split(flat, specs).items():
        led.add("%s, state %s" % (label, name), _op(name), WF.scaled_rms(got, want[name][row].reshape(-1)) / WF.STATE_BOUND)


# ---- A. streaming handles -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,spw,B,plan", WF.LARGE_HANDLES, ids=["%s-B%d-plan%d" % (v, B, p) for v, _, B, p in WF.LARGE_HANDLES])
def test_streaming_handle_on_a_forced_stride(variant, spw, B, plan, monkeypatch):
    """Family `plain`, fused mode.  Every frame of the base run: the outputs of all B rows within OUT_BOUND of the oracle's stream idx[r],
    rows with the same idx bit-identical.  After it: `state_get_all` of the rows on both sides of every threshold (and of every row of base
    stream 3) within STATE_BOUND per tensor, replicas bit-identical; `state_get` of two whole [B, ...] tensors (B rows at a pitch of 2^26
    bytes) against the oracle and against `state_get_all`.  Then, on the last row: `state_set` of a changed row and a step against the
    oracle started from that state; `reset(B - 1)` and a step: the row's output and states are bit for bit those of its first frame; a
    masked step that holds rows 255, 256 and B - 1: their states stay bit-identical, their outputs are zero, the others go on (the
    baseline has no masked step: it says so and steps all rows).  One-stream LSTM handle only: two frames each on the per-layer kernels,
    hipGraph replay and plain launches, bit-identical to each other and within 1e-6 RMS of the fused kernel
    (tests/test_gpu_parity.py::test_execution_modes_agree)."""
    idx = WF.large_index_map(B)
    assert WF.large_map_ok(idx)
    blob, ref, cont = WF.container("plain", variant=variant), WF.reference("plain", variant=variant), WF.large_continuation(variant)
    base = WF.baseline_streams() if variant == "baseline" else WF.base_streams()
    frames = WF.BASE_FRAMES if variant == "baseline" else WF.FRAMES
    last = B - 1
    eng = _create(monkeypatch, lambda: NutlsEngine(blob, batch=B, variant=variant, streams_per_workgroup=spw), B)
    try:
        assert eng.mode == "fused" and eng.streams_per_workgroup == plan
        specs = eng.state_specs()
        assert [n for n, _ in specs] == WF.state_names(variant)
        led = Ledger("%s, B = %d, %d-stream plan, slices of 2^26 bytes" % (variant, B, plan), eng.fused_plan())
        fused_out = []
        for f in range(frames):
            out = eng.step(np.ascontiguousarray(base[f][idx]))
            assert out.shape == (B, 256) and np.isfinite(out).all(), f
            led.add("output, frame %d (worst row)" % f, LAST_OP, _rows_ratio(out, ref.out[f][idx]))
            _assert_replicas(out, idx, "output of frame %d" % f)
            if f < 2:
                fused_out.append(out.copy())
            if f == 0:
                first_state = eng.state_get_all(last)
        # -- all states of the sampled rows, and two whole tensors
        sampled = sorted(set(WF.large_sample_rows(B)) | set(WF.LARGE_FOURTH))
        flats = {r: eng.state_get_all(r) for r in sampled}
        for r in sampled:
            _add_states(led, flats[r], specs, ref.state, idx[r], "row %d" % r)
            twin = min(q for q in sampled if idx[q] == idx[r])
            assert np.array_equal(flats[r], flats[twin]), "states of row %d differ from those of row %d (both base stream %d)" % (r, twin, idx[r])
        whole = {}
        for name in WF.LARGE_EDITED[variant]:
            got = whole[name] = eng.state_get(name)
            assert got.shape[0] == B
            want = ref.state[name][idx].reshape(B, -1)
            d = np.sqrt(np.mean((got.reshape(B, -1) - want) ** 2, axis=1)) / np.maximum(1.0, np.abs(want).max(axis=1))
            led.add("state_get(%s), all rows (worst row)" % name, _op(name), float(d.max()) / WF.STATE_BOUND)
            _assert_replicas(got.reshape(B, -1), idx, "state_get(%s)" % name)
            for r in sampled:
                assert np.array_equal(got[r].reshape(-1), _split(flats[r], specs)[name]), (name, r)
        # -- a changed last row
        wmap = idx.copy()
        wmap[last] = 4
        for name, v in cont.edits.items():
            t = whole[name].copy()
            t[last] = v.reshape(t[last].shape)
            eng.state_set(name, t)
        out = eng.step(np.ascontiguousarray(base[cont.extra[0]][idx]))
        led.add("output behind state_set (worst row)", LAST_OP, _rows_ratio(out, cont.steps[0].out[0][wmap]))
        _assert_replicas(out, idx, "output behind state_set", skip=(last,))
        _add_states(led, eng.state_get_all(last), specs, cont.steps[0].state, 4, "behind state_set, row %d" % last)
        _add_states(led, eng.state_get_all(256), specs, cont.steps[0].state, idx[256], "behind state_set, row 256")
        # -- the last row started anew
        eng.reset(last)
        x = np.ascontiguousarray(base[cont.extra[1]][idx])
        x[last] = base[0][3]
        out = eng.step(x)
        led.add("output behind reset(%d) (worst row)" % last, LAST_OP, _rows_ratio(out, cont.steps[1].out[0][wmap]))
        _assert_replicas(out, idx, "output behind reset", skip=(last,))
        assert np.array_equal(out[last], fused_out[0][last]), "reset(%d) and a step: not the output of the row's first frame" % last
        flat = eng.state_get_all(last)
        _add_states(led, flat, specs, cont.steps[1].state, 4, "behind reset, row %d" % last)
        assert np.array_equal(flat, first_state), "reset(%d) and a step: not the states behind the row's first frame" % last
        # -- a masked step that holds rows on both sides of 2^32 floats
        held = WF.large_held_rows(B)
        mask = np.ones(B, bool)
        mask[list(held)] = False
        x = np.ascontiguousarray(base[cont.extra[2]][idx])
        if variant == "baseline":
            with pytest.raises(ValueError):
                eng.step(x, active=mask)
            out = eng.step(x)
            led.add("output of the last step (worst row)", LAST_OP, _rows_ratio(out, cont.steps[2].out[0][wmap]))
            _assert_replicas(out, idx, "output of the last step", skip=(last,))
            moved = sampled
        else:
            before = {r: eng.state_get_all(r) for r in held}
            out = eng.step(x, active=mask)
            assert not out[list(held)].any(), "held rows have output"
            for r in held:
                assert np.array_equal(eng.state_get_all(r), before[r]), "the masked step changed the states of held row %d" % r
            led.add("output of the masked step, active rows (worst row)", LAST_OP, _rows_ratio(out[mask], cont.steps[2].out[0][idx[mask]]))
            _assert_replicas(out, idx, "output of the masked step", skip=held)
            moved = [r for r in sampled if r not in held]
        for r in moved:
            _add_states(led, eng.state_get_all(r), specs, cont.steps[2].state, wmap[r], "at the end, row %d" % r)
        # -- the per-layer kernels' slot_of(b) * sstride
        if variant == "lstm" and plan == 1:
            per_layer = {}
            for mode in ("graph", "launches"):
                eng.reset()
                eng.set_mode(mode)
                per_layer[mode] = [eng.step(np.ascontiguousarray(base[f][idx])).copy() for f in range(2)]
            for f in range(2):
                g, l = per_layer["graph"][f], per_layer["launches"][f]
                assert np.array_equal(g, l), "frame %d: hipGraph replay and plain launches differ" % f
                led.add("per-layer kernels, output, frame %d (worst row)" % f, LAST_OP, _rows_ratio(g, ref.out[f][idx]))
                led.add("per-layer kernels against the fused kernel, frame %d" % f, LAST_OP, WF.rms(g, fused_out[f]) / DEVICE_RMS, device=True)
                _assert_replicas(g, idx, "per-layer kernels, output of frame %d" % f)
    finally:
        eng.close()
    led.close()


# ---- B. offline handles -------------------------------------------------------------------------------------------------------------------------
OFFLINE = {"frame, one chunk": ("frame", 1, ()), "frame, three chunks": ("frame", 3, ()), "causal32, one chunk": ("causal32", 1, ()),
           "frame, fp32 convs": ("frame", 0, (("NUTLS_OFFLINE_FP32", "1"),))}


@pytest.mark.parametrize("config", list(OFFLINE))
def test_offline_handle_on_a_forced_stride(config, monkeypatch):
    """Eight utterances x 32 frames, 264 rows of 2^26 bytes (utterance 7's frames 25 .. 32 start beyond 2^32 floats, its carried slot is row
    231): a uniform block of 32 (the strided carry copy reads row 263 and writes row 231), a ragged block of width 32 with counts
    (32, 0, 1, 17, 32, 5, 31, 32), a uniform block of 7, then `reset_utterance(7)` and a block of 5.  Every output row of every call within
    OUT_BOUND and all 130 carried states of every utterance after every call within STATE_BOUND of the float64 oracle fed frame by frame;
    behind the reset utterance 7 is an oracle that starts from nothing.  Three chunks: the chunk pipeline (frame offsets U * t0 into the
    LSTM's input products); causal32: the history roll with the utterance stride; fp32 convs: ``conv_mfma_kernel``."""
    ctfa_mode, pipeline, env = OFFLINE[config]
    x, ref = WF.block_set_inputs(8), WF.block_reference("plain", utterances=8, ctfa_mode=ctfa_mode)
    off = _create(monkeypatch, lambda: NutlsOffline(WF.container("plain"), max_frames=WF.BLOCK8_MAX, utterances=8, ctfa_mode=ctfa_mode, pipeline=pipeline),
                  8 * (WF.BLOCK8_MAX + 1), env)
    led = Ledger("plain, 8 utterances x 32 frames, %s, slices of 2^26 bytes" % config)
    try:
        pos = [0] * 8
        for k, counts in enumerate(WF.block8_calls()):
            if k == 3:
                off.reset_utterance(WF.BLOCK8_RESET)
            if len(set(counts)) == 1:
                got = list(off.process(np.stack([x[u, pos[u]:pos[u] + counts[u]] for u in range(8)])))
            else:
                got = off.process_ragged([x[u, pos[u]:pos[u] + counts[u]] for u in range(8)])
            for u, c in enumerate(counts):
                assert got[u].shape == (c, 256) and np.isfinite(got[u]).all(), (k, u)
                for f in range(c):
                    led.add("call %d, utterance %d, frame %d: output" % (k, u, f), LAST_OP, WF.scaled_rms(got[u][f], ref.out(k, u)[f]) / WF.OUT_BOUND)
                pos[u] += c
            for name in WF.state_names():
                st = off.state_get(name)
                for u in range(8):
                    led.add("behind call %d, utterance %d: state %s" % (k, u, name), WF.state_consumer(name),
                            WF.scaled_rms(st[u].reshape(-1), ref.state(k, u)[name].reshape(-1)) / WF.STATE_BOUND)
    finally:
        off.close()
    assert len(led.ratio) == sum(sum(c) for c in WF.block8_calls()) + 4 * 8 * 130
    led.close()


# ---- C. the documented shape at its natural stride ----------------------------------------------------------------------------------------------
DOC_COUNTS = (1024, 0, 1, 513, 256, 1000, 77, 1023)


def test_documented_offline_shape_against_one_utterance_handles():
    """`NutlsOffline(max_frames=1024, utterances=8)` on the shipped weights, automatic chunk count: 8200 arena rows of about 2.6 MB, about
    22 GB -- byte and element offsets pass 2^31 and 2^32, and the carry copy behind a uniform block runs with a pitch above 2^31 bytes.
    Two uniform blocks of 1024 and a ragged block (counts 1024, 0, 1, 513, 256, 1000, 77, 1023) of the golden clip's magnitudes, repeated,
    each utterance from another frame, against eight one-utterance handles of max_frames = 256 (257 rows; four calls per block; pinned to
    the goldens by tests/test_gpu_offline.py): every call of every utterance within 1e-6 RMS and 5e-5 maximum (the bounds between handles
    that differ in tiling alone, tests/test_gpu_offline.py), `msfe6_ee_prev1` and `msfe4_en_h` of every utterance after every call within
    rtol 1e-4 / atol 3e-5 (test_offline_handle_state_get_set_addresses_the_carried_state), utterance 0's first 249 frames within 2e-5 RMS
    of the golden outputs.  (Measured on an MI355X: worst RMS 2.0e-7, worst maximum 2.3e-5 over the 23 calls.)"""
    clip = np.load(os.path.join(GOLDEN, "clip_4s.npz"))
    mags, U, M = clip["mags_in"], 8, 1024
    calls = ((M,) * U, (M,) * U, DOC_COUNTS)
    x = np.stack([mags[(31 * u + np.arange(3 * M)) % len(mags)] for u in range(U)]).astype(np.float32)
    names = ("msfe6_ee_prev1", "msfe4_en_h")
    big = NutlsOffline(max_frames=M, utterances=U)
    try:
        got, got_states, pos = [], [], [0] * U
        for counts in calls:
            if len(set(counts)) == 1:
                got.append(list(big.process(np.stack([x[u, pos[u]:pos[u] + M] for u in range(U)]))))
            else:
                got.append(big.process_ragged([x[u, pos[u]:pos[u] + c] for u, c in enumerate(counts)]))
            got_states.append({n: big.state_get(n) for n in names})
            pos = [p + c for p, c in zip(pos, counts)]
    finally:
        big.close()
    worst_rms = worst_max = 0.0
    for u in range(U):
        one = NutlsOffline(max_frames=256)
        try:
            a = 0
            for k, counts in enumerate(calls):
                c = counts[u]
                assert got[k][u].shape == (c, 256)
                if c:
                    want = one.process(x[u, a:a + c])
                    r, m = WF.rms(got[k][u], want), float(np.abs(got[k][u] - want).max())
                    print("documented shape | call %d, utterance %d, %4d frames | RMS %.3e, max %.3e" % (k, u, c, r, m))
                    worst_rms, worst_max = max(worst_rms, r), max(worst_max, m)
                    assert np.isfinite(got[k][u]).all() and float(np.abs(want).max()) > 1e-3
                    assert r < 1e-6 and m < 5e-5, (k, u, r, m)
                    if u == 0 and k == 0:
                        assert WF.rms(got[0][0][:249], clip["mags_out"]) < TIGHT_RMS
                for n in names:
                    np.testing.assert_allclose(got_states[k][n][u], one.state_get(n)[0], rtol=1e-4, atol=3e-5, err_msg="%s behind call %d, utterance %d" % (n, k, u))
                a += c
        finally:
            one.close()
    print("documented shape | worst RMS %.3e (bound 1e-6), worst max %.3e (bound 5e-5)" % (worst_rms, worst_max))


# ---- D. the page-locked path --------------------------------------------------------------------------------------------------------------------
def test_pinned_host_buffers_at_1024_streams():
    """`nutls_step_host` on `host_alloc` buffers at B = 1024 (the fused kernel reads and writes them over the link): four steps bit-identical
    to pageable arrays on a twin handle; copies of an input stream give bit-identical rows wherever they sit, and the first eight rows meet
    the oracle (the scheme of tests/test_gpu_parity.py::test_config_size_streams_properties)."""
    B, steps = 1024, 4
    rng = np.random.default_rng(5)
    base = (0.25 * np.abs(rng.standard_normal((steps, 8, 256)))).astype(np.float32)
    idx = rng.integers(0, 8, size=B)
    idx[:8] = np.arange(8)
    a, ref = NutlsEngine(batch=B), NutlsRef(batch=8)
    assert a.mode == "fused"
    want = []
    for s in range(steps):
        want.append(a.step(np.ascontiguousarray(base[s][idx])).copy())
        assert WF.rms(want[s][:8], ref.step(base[s]).numpy()) < TIGHT_RMS
    a.close()
    b = NutlsEngine(batch=B)
    pin_in, pin_out = host_alloc((B, 256)), host_alloc((B, 256))
    try:
        for s in range(steps):
            pin_in[...] = base[s][idx]
            got = b.step(pin_in, out=pin_out)
            assert got is pin_out
            assert np.array_equal(got, want[s]), s
            for j in range(8):
                same = got[idx == j]
                assert np.array_equal(same, np.broadcast_to(same[0], same.shape)), (s, j)
    finally:
        b.close()
    del pin_in, pin_out, got


@pytest.mark.parametrize("mode", ["fused", "graph"])
def test_pinned_views_inside_and_across_the_end_of_an_allocation(mode):
    """What tests/test_gpu_parity.py::test_step_on_pinned_host_buffers_equals_pageable_ones describes and does not run.  "inside": a view at
    an offset inside a pinned allocation -- the direct path.  "across": a buffer that starts inside a pinned allocation and runs past its
    end -- the library must not hand it to the kernel as pinned; it takes the staged copies.  Such a buffer is made from an allocation
    of one page and a quarter: the runtime maps whole pages, so the view at the second page's start is addressable for its 3072 bytes,
    of which the allocation owns 1024.  All four pairings of the two kinds for input and output, bit-identical to pageable arrays."""
    B, n = 3, 3 * 256
    clip = np.load(os.path.join(GOLDEN, "clip_4s.npz"))
    x = np.stack([np.roll(clip["mags_in"][:8], s, axis=0) for s in range(B)], axis=1).astype(np.float32)      # [8, B, 256]
    a = NutlsEngine(batch=B, mode=mode)
    want = [a.step(x[i]).copy() for i in range(8)]
    a.close()
    lib, page = load_library(), os.sysconf("SC_PAGESIZE")
    assert page >= 4 * n
    big = host_alloc((4 * n,))
    inside = {"in": big[64:64 + n].reshape(B, 256), "out": big[2 * n + 128:3 * n + 128].reshape(B, 256)}
    raw, across, kinds, got = [], {}, None, None
    b = NutlsEngine(batch=B, mode=mode)
    try:
        for side in ("in", "out"):
            p = lib.nutls_host_alloc(page + 1024)
            assert p and p % page == 0, lib.nutls_last_error()
            raw.append(p)
            pages = np.frombuffer((ctypes.c_float * (2 * page // 4)).from_address(p), dtype=np.float32)
            across[side] = pages[page // 4:page // 4 + n].reshape(B, 256)
        kinds = {"inside": inside, "across": across}
        for i, (ki, ko) in enumerate([("inside", "inside"), ("across", "across"), ("across", "inside"), ("inside", "across")] * 2):
            kinds[ki]["in"][...] = x[i]
            got = b.step(kinds[ki]["in"], out=kinds[ko]["out"])
            assert got is kinds[ko]["out"]
            assert np.array_equal(got, want[i]), (i, ki, ko)
    finally:
        b.close()
        del across, kinds, got
        for p in raw:
            lib.nutls_host_free(p)
    del inside, big
