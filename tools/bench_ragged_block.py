"""What per-utterance frame counts (nutls_process_block_ragged) cost -- and what the uniform block pays for their existence.

    python tools/bench_ragged_block.py [--parent-lib PATH/libnutls_hip.so] [--out profiles/ragged_block_bench.json]

8 utterances x 1024 frames (the offline batch workload), one child process per library and round (a fresh HIP context each):

  (a) the UNIFORM call, nutls_process_block on device buffers: this tree's library, and -- with --parent-lib, a build of the parent commit's
      library -- the parent's, interleaved parent / branch / parent / branch in the same job on the same device.  The two parent rounds give
      the run-to-run spread of the box; the branch must lie within it (the ragged entries may cost the uniform call nothing).
  (b) the RAGGED call with all counts full against the uniform call of the same handle, two rounds: the price of stage-in and commit
      (masked copies in and out and the per-utterance state gather, in place of two plain copies and one strided copy).
  (c) NutlsOffline.enhance_many on a fixed synthetic corpus (LENGTHS_IN_HOPS below: seeded once, committed here) through 8 slots of 1024
      hops, against the same recordings one after the other on a one-utterance handle of 1024 hops: useful frames per second of wall
      time (host clock around the whole call, PCM in host memory both ways), two rounds each, interleaved.

(a) and (b) are timed as in tools/bench_step_active.py: untimed calls for --condition-ms first (an idle GPU runs its first launches below
its steady clocks), a warm-up, then `windows` windows of `calls` back-to-back calls between two HIP events; minimum and median over the
windows.  Input: synthetic magnitudes 0.25 |N(0,1)| as in bench.py, white noise at 0.1 for (c).  One JSON line (and --out).
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

U, FRAMES = 8, 1024
# 40 recordings, 0.5 .. 60 s at 62.5 hops per second: numpy.random.default_rng(2024).lognormal(6.3, 0.9, 40), clipped to 30 .. 3750, as int
LENGTHS_IN_HOPS = [
    1374, 2386, 1528, 226, 155, 578, 1182, 861, 2777, 1070, 968, 281, 200, 2071, 569, 1130, 157, 367, 170, 270,
    1227, 143, 336, 631, 298, 433, 446, 793, 369, 695, 573, 798, 666, 2420, 299, 1602, 379, 229, 1619, 366,
]


def timed(torch, fn, calls, windows, condition_ms, warmup=3):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < condition_ms:
        for _ in range(4):
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
    med = statistics.median(ms)
    return {"min_ms": round(min(ms), 4), "median_ms": round(med, 4), "max_ms": round(max(ms), 4), "frames_per_s": round(U * FRAMES / med * 1e3)}


def child(args):
    """One library, one process: the cases named in --cases, one JSON line."""
    import numpy as np
    import torch
    from nunet_amd import NutlsOffline

    res = {}
    cases = args.cases.split(",")
    if "uniform" in cases or "ragged_full" in cases:
        off = NutlsOffline(max_frames=FRAMES, utterances=U)
        gen = torch.Generator().manual_seed(1234)
        x = (0.25 * torch.randn(U, FRAMES, 256, generator=gen).abs()).cuda()
        out = torch.empty_like(x)
        full = torch.full((U,), FRAMES, dtype=torch.int32, device="cuda")
        for case in cases:      # (in the order given: "uniform,ragged_full,uniform,ragged_full" interleaves two rounds on one handle)
            if case not in ("uniform", "ragged_full"):
                continue
            fn = (lambda: off.process_block_device(x, out)) if case == "uniform" else (lambda: off.process_block_device(x, out, frames=full))
            key = case + "_round%d" % (1 + sum(k.startswith(case) for k in res))
            res[key] = timed(torch, fn, args.calls, args.windows, args.condition_ms)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all())
        off.close()
    if "corpus" in cases:
        rng = np.random.default_rng(99)
        waves = [(0.1 * rng.standard_normal((n + 1) * 256)).astype(np.float32) for n in LENGTHS_IN_HOPS]
        useful = sum(LENGTHS_IN_HOPS)
        many = NutlsOffline(max_frames=FRAMES, utterances=U)
        one = NutlsOffline(max_frames=FRAMES)

        def alone():
            outs = []
            for w in waves:
                one.reset()
                outs.append(one.enhance(w))
            return outs

        many.enhance_many(waves[:U])          # warm-up of both handles: code objects, staging buffers
        alone_out = alone()
        reps = 3          # (passes over the corpus per timed round: a round is a second or so of work)
        for rnd in (1, 2):
            t0 = time.perf_counter()
            for _ in range(reps):
                got = many.enhance_many(waves)
            t1 = time.perf_counter()
            for _ in range(reps):
                alone()
            t2 = time.perf_counter()
            res["enhance_many_round%d" % rnd] = {"seconds_per_pass": round((t1 - t0) / reps, 4), "useful_frames_per_s": round(useful * reps / (t1 - t0))}
            res["one_utterance_handles_round%d" % rnd] = {"seconds_per_pass": round((t2 - t1) / reps, 4), "useful_frames_per_s": round(useful * reps / (t2 - t1))}
        worst = max(float(np.sqrt(np.mean((g - r) ** 2)) / np.sqrt(np.mean(r ** 2))) for g, r in zip(got, alone_out))
        from nunet_amd import plan_ragged_blocks
        blocks = plan_ragged_blocks(LENGTHS_IN_HOPS, U, FRAMES)
        res["corpus"] = {"recordings": len(waves), "useful_frames": useful, "blocks": len(blocks),
                         "computed_frames": sum(U * max(e[3] for e in b) for b in blocks),
                         "worst_relative_rms_vs_one_utterance_handles": worst}
        assert worst < 1e-5
        many.close(); one.close()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "cases": res}))


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
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--condition-ms", type=float, default=300.0)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--cases", default="uniform")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rec = {"what": "offline batch handle, %d utterances x %d frames on device buffers, ms per call: min / median / max over %d windows of %d "
                   "back-to-back calls (HIP events) after %.0f ms of clock conditioning; one process per library and round"
                   % (U, FRAMES, args.windows, args.calls, args.condition_ms)}
    a = {}
    if args.parent_lib:      # parent, branch, parent, branch: the parent's two rounds are the box's own spread
        a["parent_round1"] = spawn(args, args.parent_lib, "uniform")["cases"]["uniform_round1"]
        a["branch_round1"] = spawn(args, None, "uniform")["cases"]["uniform_round1"]
        a["parent_round2"] = spawn(args, args.parent_lib, "uniform")["cases"]["uniform_round1"]
        a["branch_round2"] = spawn(args, None, "uniform")["cases"]["uniform_round1"]
        p = [a["parent_round1"]["median_ms"], a["parent_round2"]["median_ms"]]
        b = [a["branch_round1"]["median_ms"], a["branch_round2"]["median_ms"]]
        a["parent_spread_ms"] = round(abs(p[0] - p[1]), 4)
        a["branch_minus_parent_ms"] = round(statistics.mean(b) - statistics.mean(p), 4)
        a["branch_within_parent_spread"] = bool(a["branch_minus_parent_ms"] <= a["parent_spread_ms"])
    rec["a_uniform_call_parent_vs_branch"] = a
    got = spawn(args, None, "uniform,ragged_full,uniform,ragged_full")
    rec["device"] = got["device"]
    b = got["cases"]
    b["ragged_minus_uniform_ms"] = round(statistics.mean([b["ragged_full_round1"]["median_ms"], b["ragged_full_round2"]["median_ms"]])
                                         - statistics.mean([b["uniform_round1"]["median_ms"], b["uniform_round2"]["median_ms"]]), 4)
    rec["b_ragged_call_all_counts_full_vs_uniform_same_handle"] = b
    rec["c_enhance_many_synthetic_corpus"] = spawn(args, None, "corpus")["cases"]
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
