"""GPU: the fused step computes what it computed when tests/golden/fused_bitexact.npz was recorded, BIT FOR BIT.

The parity tests bound the step's error against the oracle; a change that only re-arranges the kernel's instruction stream (addressing, register
hand-over, scheduling) must not move a single bit, and a tolerance would not notice if it did.  The fixture (tools/make_fused_bitexact_golden.py)
holds, for 2 streams on the one-stream plan and the 6 frames of bench.synthetic_pool(2, 6, 1234) from the zero state with every launch writing
every state: the 6 output rows of both streams and the SHA-256 of both streams' full state after frame 6.  Held to it: the production kernel and
its stop twin run to the end (NUTLS_FUSED_STOP_TWIN=1: the production instruction stream plus one scalar compare per op)."""
import os

import numpy as np
import pytest

from tools.make_fused_bitexact_golden import FRAMES, STREAMS, run_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "fused_bitexact.npz"))
    out, sha = z["out"], str(z["state_sha256"])
    assert out.dtype == np.float32 and out.shape == (FRAMES, STREAMS, 256) and len(sha) == 64
    return out, sha


def _check(got, golden):
    out, sha = got
    want_out, want_sha = golden
    # (bit patterns, not values: +0 and -0 compare equal as floats)
    diff = np.flatnonzero(out.view(np.uint32) != want_out.view(np.uint32))
    assert diff.size == 0, "%d of %d output words differ, first at flat index %d: got %r, recorded %r" % (
        diff.size, out.size, diff[0], out.ravel()[diff[0]], want_out.ravel()[diff[0]])
    assert sha == want_sha, "outputs equal, but the streams' states after frame %d differ from the recorded ones" % FRAMES


def test_one_stream_plan_is_bit_identical_to_the_recorded_step(golden):
    _check(run_frames(), golden)


def test_stop_twin_run_to_the_end_is_bit_identical_to_the_recorded_step(golden, monkeypatch):
    monkeypatch.setenv("NUTLS_FUSED_STOP_TWIN", "1")          # (read when the handle is created)
    _check(run_frames(), golden)
