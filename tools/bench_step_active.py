"""What the per-stream active mask (nutls_step_active) costs -- and what the headline pays for its existence.

    python tools/bench_step_active.py [--parent-lib PATH/libnutls_hip.so] [--out profiles/step_active_bench.json]

ms per call of the model step on device buffers, one child process per library and round (a fresh HIP context each):

  (a) B = 256, plain nutls_step: this tree's library, and -- with --parent-lib, a build of the parent commit's library -- the parent's,
      interleaved parent / branch / parent / branch in the same job on the same device.  The two parent rounds give the run-to-run spread
      of the box; the branch must lie within it (the mask support may cost the headline nothing).
  (b) B = 256 (one stream per workgroup) with 0, 128 and 255 streams held.
  (c) B = 1024 on the two-stream plan: unmasked, every other stream held (every workgroup mixed: the step runs, then one slot is copied
      back) and every other PAIR held (whole workgroups held: they never start the step).

Like bench.py, every measurement is taken at steady clocks: untimed calls of the same step for --condition-ms first (an idle GPU runs
its first ~50 ms of launches below its steady clocks), a warm-up, then `windows` windows of `calls` back-to-back calls between two HIP
events; minimum and median over the windows.  Input: synthetic magnitudes 0.25 |N(0,1)| as in bench.py.  One JSON line (and --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, calls, windows, condition_ms, warmup=5):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < condition_ms:
        for _ in range(16):
            fn()
        torch.cuda.synchronize()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return {"min_ms": round(min(ms), 5), "median_ms": round(statistics.median(ms), 5), "max_ms": round(max(ms), 5)}


def child(args):
    """One library, one process: the cases named in --cases, one JSON line."""
    import numpy as np
    import torch
    from nunet_amd import NutlsEngine

    def run(B, plan, mask):
        eng = NutlsEngine(batch=B, streams_per_workgroup=plan)
        assert eng.mode == "fused" and eng.streams_per_workgroup == plan
        gen = torch.Generator().manual_seed(1234)
        pool = (0.25 * torch.randn(8, B, 256, generator=gen).abs()).cuda()
        out = torch.empty(B, 256, device="cuda")
        m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).cuda()
        k = [0]

        def fn():
            k[0] += 1
            if m is None:
                eng.step(pool[k[0] & 7], out)
            else:
                eng.step(pool[k[0] & 7], out, active=m)

        r = timed(torch, fn, args.calls, args.windows, args.condition_ms)
        torch.cuda.synchronize()
        live = out if m is None else out[m.bool()]
        assert bool(torch.isfinite(live).all()) and (m is None or not bool(out[~m.bool()].any()))
        eng.close()
        return r

    def held(B, idx):
        m = np.ones(B, np.uint8)
        m[idx] = 0
        return m

    res = {}
    for case in args.cases.split(","):
        if case == "plain256":
            res[case] = run(256, 1, None)
        elif case == "mask256_held0":
            res[case] = run(256, 1, held(256, []))
        elif case == "mask256_held128":
            res[case] = run(256, 1, held(256, np.arange(0, 256, 2)))
        elif case == "mask256_held255":
            res[case] = run(256, 1, held(256, np.arange(1, 256)))
        elif case == "plain1024_g2":
            res[case] = run(1024, 2, None)
        elif case == "mask1024_g2_every_other_stream":
            res[case] = run(1024, 2, held(1024, np.arange(0, 1024, 2)))
        elif case == "mask1024_g2_every_other_pair":
            res[case] = run(1024, 2, held(1024, np.flatnonzero((np.arange(1024) // 2) % 2 == 0)))
        else:
            raise SystemExit("unknown case " + case)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "cases": res}))


ALL_CASES = "plain256,mask256_held0,mask256_held128,mask256_held255,plain1024_g2,mask1024_g2_every_other_stream,mask1024_g2_every_other_pair"


def spawn(args, lib, cases):
    env = dict(os.environ)
    if lib:
        env["NUTLS_DEV"], env["NUTLS_LIB"] = "1", os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--cases", cases, "--calls", str(args.calls), "--windows", str(args.windows),
           "--condition-ms", str(args.condition_ms)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("child failed with status %d (%s): nothing more is started" % (r.returncode, lib or "this tree's library"))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libnutls_hip.so built from the parent commit (case (a); without it only this tree's library is timed)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--condition-ms", type=float, default=200.0)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--cases", default=ALL_CASES)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rec = {"what": "nutls_step / nutls_step_active on device buffers, ms per call: min / median / max over %d windows of %d back-to-back calls "
                   "(HIP events) after %.0f ms of clock conditioning; one process per library and round" % (args.windows, args.calls, args.condition_ms)}
    a = {}
    if args.parent_lib:      # parent, branch, parent, branch: the parent's two rounds are the box's own spread
        a["parent_round1"] = spawn(args, args.parent_lib, "plain256")["cases"]["plain256"]
        a["branch_round1"] = spawn(args, None, "plain256")["cases"]["plain256"]
        a["parent_round2"] = spawn(args, args.parent_lib, "plain256")["cases"]["plain256"]
        a["branch_round2"] = spawn(args, None, "plain256")["cases"]["plain256"]
        p = [a["parent_round1"]["median_ms"], a["parent_round2"]["median_ms"]]
        b = [a["branch_round1"]["median_ms"], a["branch_round2"]["median_ms"]]
        a["parent_spread_ms"] = round(abs(p[0] - p[1]), 5)
        a["branch_minus_parent_ms"] = round(statistics.mean(b) - statistics.mean(p), 5)
        a["branch_within_parent_spread"] = bool(a["branch_minus_parent_ms"] <= a["parent_spread_ms"])
    rec["a_plain_step_256_streams"] = a
    got = spawn(args, None, args.cases)
    rec["device"], rest = got["device"], got["cases"]
    rec["b_256_streams_one_stream_plan"] = {k: v for k, v in rest.items() if "256" in k}
    rec["c_1024_streams_two_stream_plan"] = {k: v for k, v in rest.items() if "1024" in k}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
