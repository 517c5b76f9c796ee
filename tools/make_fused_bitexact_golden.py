#!/usr/bin/env python3
"""GPU box: record what the fused step computes, bit for bit (tests/golden/fused_bitexact.npz; tests/test_gpu_fused_bitexact.py).

    python tools/make_fused_bitexact_golden.py [out.npz]

2 streams, one-stream plan, the 6 frames of bench.synthetic_pool(2, 6, 1234) from the zero state, every launch writing every state
(NUTLS_EAGER_STATES=1): the 6 output rows of both streams and the SHA-256 of both streams' full state after frame 6.  Re-run it only when a
change is MEANT to alter the step's results."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STREAMS, FRAMES, SEED = 2, 6, 1234


def run_frames(**engine_kw):
    """(out [FRAMES, STREAMS, 256] float32, hex SHA-256 of the streams' states after the last frame) of a fresh engine."""
    import bench
    import nunet_amd
    old = os.environ.get("NUTLS_EAGER_STATES")
    os.environ["NUTLS_EAGER_STATES"] = "1"          # (read when the handle is created)
    try:
        eng = nunet_amd.NutlsEngine(batch=STREAMS, device=0, mode="fused", streams_per_workgroup=1, **engine_kw)
    finally:
        if old is None:
            del os.environ["NUTLS_EAGER_STATES"]
        else:
            os.environ["NUTLS_EAGER_STATES"] = old
    pool = bench.synthetic_pool(STREAMS, FRAMES, SEED)
    out = np.stack([eng.step(pool[i]).copy() for i in range(FRAMES)])
    h = hashlib.sha256()
    for s in range(STREAMS):
        h.update(np.ascontiguousarray(eng.state_get_all(s), dtype=np.float32).tobytes())
    eng.close()
    return out, h.hexdigest()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fused_bitexact.npz")
    out, sha = run_frames()
    np.savez(path, out=out, state_sha256=np.array(sha))
    print("wrote %s: out %s, state sha256 %s" % (path, out.shape, sha))
