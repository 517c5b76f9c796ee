"""GPU: the one-stream builds of csrc/fused_step.hip that tests/test_gpu_fused_bitexact.py does not run compute what they computed when
tests/golden/fused_bitexact_modes.npz was recorded, BIT FOR BIT.

That test holds the production kernel and its stop twin with every launch writing every state.  Held here (tools/make_fused_bitexact_modes_golden.py,
2 streams, the 6 frames of bench.synthetic_pool(2, 6, 1234) from the zero state): the production kernel WITHOUT NUTLS_EAGER_STATES -- the path
bench.py runs -- whose outputs are fused_bitexact.npz's, with the state hash recorded for that path (the states read back are the eager
run's: the library completes the lazily written ones when they are read); the profiling twin; the hop build; the
baseline variant's build on synthetic weights of seed 4321.  A change that re-arranges the instruction stream of the source they share must not
move a bit in any of them."""
import os

import numpy as np
import pytest

from tools.make_fused_bitexact_modes_golden import FRAMES, STREAMS, run_mode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "fused_bitexact_modes.npz"))
    rec = {k: z[k] for k in z.files}
    rec["out_lazy"] = np.load(os.path.join(golden_dir, "fused_bitexact.npz"))["out"]
    return rec


@pytest.mark.parametrize("mode", ["lazy", "prof", "hop", "base"])
def test_build_is_bit_identical_to_the_recorded_step(golden, mode):
    want_out, want_sha = golden["out_" + mode], str(golden["state_sha256_" + mode])
    assert want_out.dtype == np.float32 and want_out.shape == (FRAMES, STREAMS, 256) and len(want_sha) == 64
    out, sha = run_mode(mode)
    # (bit patterns, not values: +0 and -0 compare equal as floats)
    diff = np.flatnonzero(out.view(np.uint32) != want_out.view(np.uint32))
    assert diff.size == 0, "%s: %d of %d output words differ, first at flat index %d: got %r, recorded %r" % (
        mode, diff.size, out.size, diff[0], out.ravel()[diff[0]], want_out.ravel()[diff[0]])
    assert sha == want_sha, "%s: outputs equal, but the streams' states after frame %d differ from the recorded ones" % (mode, FRAMES)
