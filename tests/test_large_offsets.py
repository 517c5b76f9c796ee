"""CPU half of tests/test_gpu_large_offsets.py (no GPU): the index map of the large streaming handles never puts a replica where a truncated
offset would land, the shapes cross the four thresholds they are said to cross, and the float32 oracle stays within 1/20 of every bound on
the inputs that are new there (the eight-utterance call sequence in both CTFA modes, the steps behind the state edits)."""
import os

import numpy as np
import pytest
import torch

import weight_families as WF
from nunet_amd.build import CSRC


def test_index_maps_never_alias_a_replica():
    """For every large streaming handle: idx[r] != idx[r - T] for T = 32, 64, 128, 256 rows and every r >= T; all four base streams ride on
    several rows, base stream 3 on row B - 1, and the sampled and the held rows lie on both sides of every threshold.  The plain map
    r % 4 fails the same condition: the check is not empty."""
    assert sorted(WF.THRESHOLD_ROWS.values()) == [32, 64, 128, 256]
    for variant, _, B, _ in WF.LARGE_HANDLES:
        idx = WF.large_index_map(B)
        assert idx.shape == (B,) and WF.large_map_ok(idx), (variant, B)
        for T in WF.THRESHOLD_ROWS.values():
            assert all(idx[r] != idx[r - T] for r in range(T, B)), (B, T)
        assert idx[B - 1] == 3 and all(idx[r] == 3 for r in WF.LARGE_FOURTH)
        assert all(int((idx == s).sum()) >= 4 for s in range(4))
        rows = WF.large_sample_rows(B)
        assert rows == [0, 31, 32, 63, 64, 127, 128, 255, 256, B - 1]
        assert set(WF.large_held_rows(B)) <= set(rows) and {int(idx[r]) for r in WF.large_held_rows(B)} == {1, 2, 3}
        for T in WF.THRESHOLD_ROWS.values():          # replicas of base stream 3 on both sides of every threshold: "bit-identical" spans it
            assert any(idx[:T] == 3) and any(idx[T:] == 3), (B, T)
        assert not WF.large_map_ok(np.arange(B) % 4)
    bad = WF.large_index_map(264)
    bad[200 - 128] = 3          # row 200 carries stream 3: one replica 2^31 floats below it is enough to fail
    assert not WF.large_map_ok(bad)


def test_shapes_cross_the_four_thresholds():
    """Rows x 2^26 bytes: the last row of every shape starts beyond 2^32 floats, so each shape has rows on both sides of 2^31 and 2^32, of
    bytes and of floats.  The offline shape: utterance 7's carried slot is row 231, its frames 25 .. 32 rows 256 .. 263, and the uniform
    block of 32 carries row 263 over to row 231.  The knob that makes the stride is still read where the arena is laid out."""
    assert WF.ROW_BYTES == 1 << 26 and WF.STRIDE_ALIGN * 4 == WF.ROW_BYTES
    assert WF.THRESHOLD_ROWS == {"2^31 bytes": 32, "2^32 bytes": 64, "2^31 floats": 128, "2^32 floats": 256}
    offline_rows = 8 * (WF.BLOCK8_MAX + 1)
    for rows in [B for _, _, B, _ in WF.LARGE_HANDLES] + [offline_rows]:
        last = (rows - 1) * WF.ROW_BYTES
        assert last >= 1 << 31 and last >= 1 << 32 and last // 4 >= 1 << 31 and last // 4 >= 1 << 32, rows
        for what, row in WF.THRESHOLD_ROWS.items():
            limit = (1 << int(what[2:4])) * (4 if what.endswith("floats") else 1)
            assert row * WF.ROW_BYTES >= limit > (row - 1) * WF.ROW_BYTES and row < rows, (rows, what)
        assert rows * WF.ROW_BYTES <= 19 * (1 << 30) + (1 << 29)          # the largest handle: 300 rows, 18.75 GiB
    assert offline_rows == 264
    slot = lambda u, t: u * (WF.BLOCK8_MAX + 1) + t          # t = 0: the carried slot, t >= 1: frame t of the block
    assert slot(7, 0) == 231 and [slot(7, t) for t in range(25, 33)] == list(range(256, 264))
    assert slot(7, 25) * WF.ROW_BYTES // 4 >= 1 << 32 > slot(7, 24) * WF.ROW_BYTES // 4
    assert slot(7, WF.BLOCK8_CALLS[0][7]) == 263
    with open(os.path.join(CSRC, "engine.cpp")) as f:
        assert 'getenv("NUTLS_STRIDE_ALIGN")' in f.read()


def test_block8_call_sequence():
    """The counts of the eight-utterance sequence: what the issue of the large-offset tests sets, and that every utterance's frames fit."""
    assert WF.BLOCK8_CALLS == ((32,) * 8, (32, 0, 1, 17, 32, 5, 31, 32), (7,) * 8) and (WF.BLOCK8_RESET, WF.BLOCK8_TAIL) == (7, 5)
    starts = WF.block8_starts()
    assert starts[1] == [32] * 8 and starts[2] == [64, 32, 33, 49, 64, 37, 63, 64] and starts[4][7] == WF.BLOCK8_FRAMES == 76
    x = WF.block_set_inputs(8)
    assert x.shape == (8, WF.BLOCK8_FRAMES, 256) and x.dtype == np.float32 and not x.flags.writeable
    assert len({x[u].tobytes() for u in range(8)}) == 8          # eight distinct streams


@pytest.mark.parametrize("ctfa_mode", WF.BLOCK8_MODES)
def test_conditioning_cap_of_the_block8_set(ctfa_mode):
    """Every output row of every call and all 130 states of every utterance after every call: the float32 oracle within 1/20 of the bound
    the GPU test applies against the float64 oracle, in both CTFA modes."""
    r64, r32 = WF.block_reference("plain", utterances=8, ctfa_mode=ctfa_mode), WF.block_reference("plain", torch.float32, 8, ctfa_mode)
    out, st = (0.0,), (0.0,)
    for k, counts in enumerate(WF.block8_calls()):
        for u, c in enumerate(counts):
            want = r64.out(k, u)
            assert want.shape == (c, 256) and np.isfinite(want).all()
            out = max([out] + [(WF.scaled_rms(r32.out(k, u)[f], want[f]), k, u, f) for f in range(c)])
            st = max([st] + [(WF.scaled_rms(r32.state(k, u)[n], r64.state(k, u)[n]), n, k, u) for n in WF.state_names()])
    print("block8, %s: float32 oracle vs float64 oracle: outputs %.2e x scale (share of the bound %.4f; call, utterance, frame %s), states %.2e x scale "
          "(share %.4f; %s)" % (ctfa_mode, out[0], out[0] / WF.OUT_BOUND, out[1:], st[0], st[0] / WF.STATE_BOUND, st[1:]))
    assert out[0] <= WF.CAP * WF.OUT_BOUND, out
    assert st[0] <= WF.CAP * WF.STATE_BOUND, st
    # a held utterance keeps its state, the reset one starts from nothing, and the two modes are different functions
    for n in WF.state_names():
        assert np.array_equal(r64.state(0, 1)[n], r64.state(1, 1)[n]), n
    fresh = WF._oracle(WF.container("plain"), np.ascontiguousarray(WF.block8_inputs()[7:8, 71:72].transpose(1, 0, 2)), torch.float64, trace=False,
                       ctfa_mode=ctfa_mode)
    assert np.array_equal(r64.out(3, 7)[0], fresh.out[0, 0])
    if ctfa_mode == "causal32":
        frame = WF.block_reference("plain", utterances=8)
        assert WF.scaled_rms(r64.out(2, 0), frame.out(2, 0)) > 10 * WF.OUT_BOUND


@pytest.mark.parametrize("variant", ["lstm", "baseline"])
def test_conditioning_cap_of_the_continuation(variant):
    """The three steps behind the base run (an edited row, a row started anew, the step the handle masks): the float32 oracle from the same
    start within 1/20 of the output and the state bound, per row.  The edits change the row (its output leaves stream 3's by far more than
    the bound), and the row started anew gives frame 0 of the reference."""
    cont, ref = WF.large_continuation(variant), WF.reference("plain", variant=variant)
    names = WF.state_names(variant)
    assert set(cont.edits) == set(WF.LARGE_EDITED[variant]) and all(v.dtype == np.float32 for v in cont.edits.values())
    x = WF.baseline_streams() if variant == "baseline" else WF.base_streams()
    state = {n: np.concatenate([ref.state[n], ref.state[n][3:4]]) for n in names}
    for n, v in cont.edits.items():
        assert WF.scaled_rms(v, ref.state[n][3]) > 100 * WF.STATE_BOUND, n
        state[n][4] = v
    worst_out = worst_st = 0.0
    for i, f in enumerate(cont.extra):
        if i == 1:
            for n in names:
                state[n][4] = 0.0
        frame = np.concatenate([x[f], x[0 if i == 1 else f][3:4]])[None]
        r32 = WF._oracle(WF.container("plain", variant=variant), frame, torch.float32, trace=False, variant=variant, state=state)
        r64 = cont.steps[i]
        for b in range(5):
            worst_out = max(worst_out, WF.scaled_rms(r32.out[0, b], r64.out[0, b]))
            worst_st = max([worst_st] + [WF.scaled_rms(r32.state[n][b], r64.state[n][b]) for n in names])
        state = {n: np.array(r64.state[n]) for n in names}
    print("continuation, %s: float32 oracle vs float64 oracle: outputs %.2e x scale (share %.4f), states %.2e x scale (share %.4f)"
          % (variant, worst_out, worst_out / WF.OUT_BOUND, worst_st, worst_st / WF.STATE_BOUND))
    assert worst_out <= WF.CAP * WF.OUT_BOUND and worst_st <= WF.CAP * WF.STATE_BOUND
    assert WF.scaled_rms(cont.steps[0].out[0, 4], cont.steps[0].out[0, 3]) > 10 * WF.OUT_BOUND
    assert WF.rms(cont.steps[1].out[0, 4], ref.out[0, 3]) < 1e-12          # (float64 on both sides; the batch sizes differ)
