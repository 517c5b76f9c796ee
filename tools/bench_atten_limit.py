"""What the attenuation limit (nutls_set_atten_limit) costs: nutls_enhance_hop at B = 256 in ms per hop and nutls_enhance_block at 8 utterances
x 1 024 hops in ms per block, with every limit 0 (the kernels every entry always launched), with every limit 0.1 (the synthesis runs its MIX
instantiation, csrc/stft.hip / csrc/stft_block.hip: one more magnitude row read per stream and hop) and with the PARENT commit's library.

    python tools/bench_atten_limit.py [--parent-lib PATH] [--out profiles/atten_limit_bench.json]

--parent-lib: a libnutls_hip.so built from the parent commit (a checkout of it, `python -m nunet_amd.build`).  One child process per library
and round (a fresh HIP context each), in the order parent, this, parent, this, all in one job on one device; a figure is the mean of its two
rounds' medians, and the margin for "limit 0 costs what the parent costs" is the spread between the two rounds of the parent itself.

Like bench.py and tools/bench_pcm_upper.py every measurement is taken at steady clocks: untimed calls for --condition-ms first, a warm-up,
then `windows` windows of `calls` back-to-back calls on device buffers between two HIP events; minimum, median and maximum over the windows.
Input: white noise at speech level (0.05 N(0,1)).  One JSON line (and --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_hop_fusion import timed  # noqa: E402

B = 256
UTTERANCES, HOPS = 8, 1024
LIMIT = 0.1


def child(args):
    """One library, one process: one JSON line."""
    import numpy as np
    import torch
    from nunet_amd import NutlsEngine, NutlsOffline

    limits = (0.0,) if args.parent else (0.0, LIMIT)
    gen = torch.Generator().manual_seed(1234)
    res = {}
    eng = NutlsEngine(batch=B)
    assert eng.mode == "fused" and eng.launches_per_hop == 3
    off = NutlsOffline(max_frames=HOPS, utterances=UTTERANCES)
    xs, out = (0.05 * torch.randn(8, B, 256, generator=gen)).cuda(), torch.empty(B, 256, device="cuda")
    blk = (0.05 * torch.randn(UTTERANCES, HOPS * 256, generator=gen)).cuda()
    blk_out = torch.empty_like(blk)
    k = [0]
    for l in limits:
        if not args.parent:      # (the parent's library has no such entry; its path is the one limit 0 must equal)
            eng.set_atten_limit(l)
            off.set_atten_limit(l)

        def hop():
            k[0] += 1
            eng.enhance_hop(xs[k[0] & 7], "edge", out)

        def block():
            off.enhance_block_device(blk, blk_out)

        tag = "limit%s" % ("0" if l == 0 else "%g" % l)
        res["enhance_hop_" + tag] = timed(torch, hop, args.calls, args.windows, args.condition_ms, wall=False)
        res["enhance_block_" + tag] = timed(torch, block, args.block_calls, args.windows, args.condition_ms, wall=False, warmup=1)
        torch.cuda.synchronize()
        assert bool(np.isfinite(out.cpu().numpy()).all()) and bool(np.isfinite(blk_out.cpu().numpy()).all())
    eng.close()
    off.close()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "ms": res}))


def spawn(args, parent):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--block-calls", str(args.block_calls),
           "--windows", str(args.windows), "--condition-ms", str(args.condition_ms)]
    env = dict(os.environ)
    if parent:      # (runner.py: another build of the same library is honoured only together with NUTLS_DEV=1)
        cmd.append("--parent")
        env.update(NUTLS_DEV="1", NUTLS_LIB=os.path.abspath(args.parent_lib))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("child failed with status %d (%s library): nothing more is started" % (r.returncode, "parent" if parent else "this"))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libnutls_hip.so built from the parent commit")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--block-calls", type=int, default=4)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--condition-ms", type=float, default=200.0)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rec = {"what": "nutls_enhance_hop at B = %d, ms per hop, and nutls_enhance_block at %d utterances x %d hops, ms per block: min / median / max "
                   "over %d windows of %d (hop) / %d (block) calls after %.0f ms of clock conditioning, device buffers between HIP events; one "
                   "process per library and round, order parent, this, parent, this" % (
                       B, UTTERANCES, HOPS, args.windows, args.calls, args.block_calls, args.condition_ms)}
    rounds = {"parent": [], "this": []}
    for rnd in (1, 2):
        for which in ("parent", "this"):
            if which == "parent" and not args.parent_lib:
                continue
            got = spawn(args, which == "parent")
            rec["device"] = got["device"]
            rec["%s_round%d" % (which, rnd)] = got["ms"]
            rounds[which].append(got["ms"])
    summary = {}
    for key0 in sorted(k for k in rounds["this"][0] if k.endswith("_limit0")):
        stem = key0[:-len("_limit0")]
        key1 = "%s_limit%g" % (stem, LIMIT)
        this0 = [r[key0]["median_ms"] for r in rounds["this"]]
        this1 = [r[key1]["median_ms"] for r in rounds["this"]]
        row = {"limit0_ms": round(statistics.mean(this0), 5), "limit%g_ms" % LIMIT: round(statistics.mean(this1), 5),
               "limit%g_minus_limit0_us" % LIMIT: round((statistics.mean(this1) - statistics.mean(this0)) * 1e3, 2),
               "this_round_spread_us": round(abs(this0[0] - this0[1]) * 1e3, 2)}
        if rounds["parent"]:
            p = [r[key0]["median_ms"] for r in rounds["parent"]]
            delta, spread = statistics.mean(this0) - statistics.mean(p), abs(p[0] - p[1])
            row.update(parent_ms=round(statistics.mean(p), 5), limit0_minus_parent_us=round(delta * 1e3, 2),
                       parent_round_spread_us=round(spread * 1e3, 2), limit0_within_parent_spread=bool(abs(delta) <= spread))
        summary[stem] = row
    rec["summary"] = summary
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
