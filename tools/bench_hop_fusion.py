"""What hop fusion (nutls_set_hop_fusion) buys: ms per streaming hop -- PCM hop in, enhanced PCM hop out -- as three launches (STFT
analysis, fused step, inverse STFT / overlap-add: the default) and as one launch of the hop build of the step kernel.

    python tools/bench_hop_fusion.py [--out profiles/hop_fusion_bench.json]

Shapes: B = 1, 8, 256 (one stream per workgroup) and 1024 (the library's choice there: the two-stream plan), each
  * on device buffers (nutls_enhance_hop, asynchronous: `calls` back-to-back calls between two HIP events), and
  * on page-locked host buffers from nutls_host_alloc (nutls_enhance_hop_host, synchronous: wall clock around `calls` calls).  With fusion
    off the hop is staged through two copy commands; with fusion on the kernel reads and writes the pinned buffers over the link itself.
One child process per setting and round (a fresh HIP context each), in the order off, on, off, on in the same job on the same device:
the two rounds of a setting give the run-to-run spread of the box, and `fused_over_three_launch` is the ratio of the settings' mean medians.

Like bench.py, every measurement is taken at steady clocks: untimed calls of the same hop for --condition-ms first, a warm-up, then
`windows` windows of `calls` calls; minimum, median and maximum over the windows.  Input: white noise at speech level (0.05 N(0,1)) as
in bench.py --frontend.  One JSON line (and --out).
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

SHAPES = (1, 8, 256, 1024)


def timed(torch, fn, calls, windows, condition_ms, wall, warmup=5):
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
        if wall:      # (synchronous calls: each returns with its result in the caller's buffer)
            t = time.perf_counter()
            for _ in range(calls):
                fn()
            ms.append((time.perf_counter() - t) * 1e3 / calls)
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / calls)
    return {"min_ms": round(min(ms), 5), "median_ms": round(statistics.median(ms), 5), "max_ms": round(max(ms), 5)}


def child(args):
    """One setting, one process: every shape on device and on pinned host buffers, one JSON line."""
    import numpy as np
    import torch
    from nunet_amd import NutlsEngine, host_alloc

    fusion = bool(args.fusion)
    res = {}
    for B in SHAPES:
        eng = NutlsEngine(batch=B, hop_fusion=fusion)
        assert eng.mode == "fused" and eng.launches_per_hop == (1 if fusion else 3)
        gen = torch.Generator().manual_seed(1234)
        pool = 0.05 * torch.randn(8, B, 256, generator=gen)
        dev_pool, dev_out = pool.cuda(), torch.empty(B, 256, device="cuda")
        k = [0]

        def on_device():
            k[0] += 1
            eng.enhance_hop(dev_pool[k[0] & 7], "edge", dev_out)

        r = {"streams_per_workgroup": eng.streams_per_workgroup,
             "device_buffers": timed(torch, on_device, args.calls, args.windows, args.condition_ms, wall=False)}
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dev_out).all())
        pins = [host_alloc((B, 256)) for _ in range(8)]
        for i in range(8):
            pins[i][...] = pool[i].numpy()
        pin_out = host_alloc((B, 256))

        def on_pinned():
            k[0] += 1
            eng.enhance_hop(pins[k[0] & 7], "edge", pin_out)

        r["pinned_host_buffers"] = timed(torch, on_pinned, args.calls, args.windows, args.condition_ms, wall=True)
        assert bool(np.isfinite(pin_out).all())
        eng.close()
        res["B%d" % B] = r
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hop_fusion": fusion, "shapes": res}))


def spawn(args, fusion):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--fusion", str(int(fusion)), "--calls", str(args.calls),
           "--windows", str(args.windows), "--condition-ms", str(args.condition_ms)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("child failed with status %d (hop fusion %s): nothing more is started" % (r.returncode, "on" if fusion else "off"))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--condition-ms", type=float, default=200.0)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--fusion", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rec = {"what": "one streaming hop (nutls_enhance_hop on device buffers, HIP events; nutls_enhance_hop_host on buffers from nutls_host_alloc, wall "
                   "clock), ms per hop: min / median / max over %d windows of %d calls after %.0f ms of clock conditioning; one process per setting "
                   "and round, order three_launch, fused, three_launch, fused" % (args.windows, args.calls, args.condition_ms)}
    rounds = []
    for rnd in (1, 2):
        for fusion in (False, True):
            got = spawn(args, fusion)
            rec["device"] = got["device"]
            rounds.append((fusion, got["shapes"]))
            rec["%s_round%d" % ("fused" if fusion else "three_launch", rnd)] = got["shapes"]
    ratio = {}
    for shape in rounds[0][1]:
        ratio[shape] = {}
        for buf in ("device_buffers", "pinned_host_buffers"):
            off = statistics.mean(s[shape][buf]["median_ms"] for f, s in rounds if not f)
            on = statistics.mean(s[shape][buf]["median_ms"] for f, s in rounds if f)
            ratio[shape][buf] = {"three_launch_ms": round(off, 5), "fused_ms": round(on, 5), "fused_over_three_launch": round(on / off, 4)}
    rec["summary"] = ratio
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
