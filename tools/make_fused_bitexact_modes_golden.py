#!/usr/bin/env python3
"""GPU box: record, bit for bit, what the OTHER one-stream builds of csrc/fused_step.hip compute (tests/golden/fused_bitexact_modes.npz;
tests/test_gpu_fused_bitexact_modes.py).

    python tools/make_fused_bitexact_modes_golden.py [out.npz]

tools/make_fused_bitexact_golden.py records the production kernel with every launch writing every state (NUTLS_EAGER_STATES=1).  This one
records the paths that fixture does not run, each for 2 streams on the one-stream plan and the 6 frames of bench.synthetic_pool(2, 6, 1234)
from the zero state:

    lazy   the production kernel WITHOUT NUTLS_EAGER_STATES -- what bench.py runs (its outputs are fused_bitexact.npz's; only the hash is kept)
    prof   the profiling twin (debug_trace: every step on fused_step_prof.hip's kernel), eager states
    hop    the hop build (enhance_hop with hop fusion on: fused_step_hop.hip), eager states; the frames are 6 PCM hops of a seeded generator
    base   the baseline variant's build (fused_base.hip) on synthetic weights of seed 4321, eager states

and for each the output rows and the SHA-256 of both streams' full state after frame 6.  Re-run it only when a change is MEANT to alter the
step's results, with the library of the commit BEFORE that change."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STREAMS, FRAMES, SEED, BASE_SEED = 2, 6, 1234, 4321
MODES = ("lazy", "prof", "hop", "base")


def _engine(eager, *args, **kw):
    """A fresh fused-mode engine on the one-stream plan, created with NUTLS_EAGER_STATES set (eager) or absent (read when the handle is created)."""
    import nunet_amd
    old = os.environ.pop("NUTLS_EAGER_STATES", None)
    if eager:
        os.environ["NUTLS_EAGER_STATES"] = "1"
    try:
        return nunet_amd.NutlsEngine(*args, batch=STREAMS, device=0, mode="fused", streams_per_workgroup=1, **kw)
    finally:
        os.environ.pop("NUTLS_EAGER_STATES", None)
        if old is not None:
            os.environ["NUTLS_EAGER_STATES"] = old


def hop_frames():
    """The 6 PCM hops [FRAMES, STREAMS, 256] of the hop build's run."""
    return (0.1 * np.random.default_rng(SEED).standard_normal((FRAMES, STREAMS, 256))).astype(np.float32)


def run_mode(mode):
    """(out [FRAMES, STREAMS, 256] float32, hex SHA-256 of the streams' states after the last frame) of a fresh engine in `mode`."""
    import bench
    pool = bench.synthetic_pool(STREAMS, FRAMES, SEED)
    if mode == "lazy":
        eng = _engine(False)
        call = eng.step
    elif mode == "prof":
        eng = _engine(True)
        eng.debug_trace(True)
        call = eng.step
    elif mode == "hop":
        eng = _engine(True, hop_fusion=True)
        assert eng.launches_per_hop == 1
        pool, call = hop_frames(), eng.enhance_hop
    elif mode == "base":
        from nunet_amd.weights import synthetic_weights, write_blob
        eng = _engine(True, write_blob(synthetic_weights("baseline", seed=BASE_SEED, bias_std=0.1, affine_jitter=0.1), int8_convs=True), variant="baseline")
        call = eng.step
    else:
        raise ValueError(mode)
    out = np.stack([call(pool[i]).copy() for i in range(FRAMES)])
    h = hashlib.sha256()
    for s in range(STREAMS):
        h.update(np.ascontiguousarray(eng.state_get_all(s), dtype=np.float32).tobytes())
    eng.close()
    return out, h.hexdigest()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fused_bitexact_modes.npz")
    rec = {}
    for mode in MODES:
        out, sha = run_mode(mode)
        if mode != "lazy":
            rec["out_" + mode] = out
        rec["state_sha256_" + mode] = np.array(sha)
        print("%-5s out %s, state sha256 %s" % (mode, out.shape, sha), flush=True)
    np.savez(path, **rec)
    print("wrote %s" % path)
