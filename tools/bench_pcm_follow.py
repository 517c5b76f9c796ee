"""What the PCM gateway's following upper-band gain (nutls_set_pcm_upper_follow) costs: nutls_enhance_hop_pcm at B = 256 in ms per hop and
nutls_enhance_block_pcm at 8 utterances x 1 024 hops in ms per block, int16 at 48 kHz and float32 at 32 kHz, all at gain 1: with follow off
(the upper band's kernels, as before), with follow on (the two kernels whose gain follows the model, csrc/pcm.hip) and with the PARENT
commit's library (which has the upper band and no follow).

    python tools/bench_pcm_follow.py [--parent-lib PATH] [--out profiles/pcm_follow_bench.json]

--parent-lib: a libnutls_hip.so built from the parent commit (a checkout of it, `python -m nunet_amd.build`).  One child process per library
and round (a fresh HIP context each), in the order parent, this, parent, this, all in one job on one device; a figure is the mean of its two
rounds' medians, and the margin for "follow off costs what the parent costs" is the spread between the two rounds of the parent itself.

Like bench.py and tools/bench_pcm_upper.py every measurement is taken at steady clocks: untimed calls for --condition-ms first, a warm-up,
then `windows` windows of `calls` back-to-back calls on device buffers between two HIP events; minimum, median and maximum over the windows.
Input: white noise at speech level (0.05 N(0,1)) -- at 32 / 48 kHz it has as much energy above 8 kHz as a signal can.  One JSON line (and --out).
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
FORMATS = (("int16", 48000), ("float32", 32000))


def child(args):
    """One library, one process: one JSON line."""
    import numpy as np
    import torch
    from nunet_amd import NutlsEngine, NutlsOffline

    modes = (0,) if args.parent else (0, 1)
    gen = torch.Generator().manual_seed(1234)

    def samples(shape, dtype):
        noise = 0.05 * torch.randn(*shape, generator=gen)
        return ((noise * 32768.0).round().clamp(-32768, 32767).to(torch.int16) if dtype == "int16" else noise).cuda()

    res = {}
    eng = NutlsEngine(batch=B)
    assert eng.mode == "fused" and eng.launches_per_hop == 3
    off = NutlsOffline(max_frames=HOPS, utterances=UTTERANCES)
    k = [0]
    for dtype, rate in FORMATS:
        for handle in (eng, off):
            handle.set_pcm_format(rate, dtype)
            handle.set_pcm_upper_band(1.0)
        S = eng.pcm_hop_samples
        xs, out = samples((8, B, S), dtype), torch.empty(B, S, dtype=getattr(torch, dtype), device="cuda")
        blk = samples((UTTERANCES, HOPS * S), dtype)
        blk_out = torch.empty_like(blk)
        for follow in modes:
            if not args.parent:      # (the parent's library has no such entry; its gateway is the one follow off must equal)
                eng.set_pcm_upper_follow(bool(follow))
                off.set_pcm_upper_follow(bool(follow))

            def pcm_hop():
                k[0] += 1
                eng.enhance_hop_pcm(xs[k[0] & 7], "edge", out)

            def pcm_block():
                off.enhance_block_pcm_device(blk, blk_out)

            tag = "%s_%dk_follow%d" % (dtype, rate // 1000, follow)
            res["enhance_hop_pcm_" + tag] = timed(torch, pcm_hop, args.calls, args.windows, args.condition_ms, wall=False)
            res["enhance_block_pcm_" + tag] = timed(torch, pcm_block, args.block_calls, args.windows, args.condition_ms, wall=False, warmup=1)
            torch.cuda.synchronize()
            assert bool(np.isfinite(np.asarray(out.cpu(), np.float64)).all()) and bool(np.isfinite(np.asarray(blk_out.cpu(), np.float64)).all())
            if follow:
                g = np.concatenate([eng.pcm_follow_gain(), off.pcm_follow_gain()])
                assert bool(np.all((g >= 0.0) & (g <= 1.0)))
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
    rec = {"what": "nutls_enhance_hop_pcm at B = %d, ms per hop, and nutls_enhance_block_pcm at %d utterances x %d hops, ms per block, upper-band "
                   "gain 1: min / median / max over %d windows of %d (hop) / %d (block) calls after %.0f ms of clock conditioning, device buffers "
                   "between HIP events; one process per library and round, order parent, this, parent, this" % (
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
    for key0 in sorted(k for k in rounds["this"][0] if k.endswith("_follow0")):
        stem, key1 = key0[:-len("_follow0")], key0[:-1] + "1"
        this0 = [r[key0]["median_ms"] for r in rounds["this"]]
        this1 = [r[key1]["median_ms"] for r in rounds["this"]]
        row = {"follow0_ms": round(statistics.mean(this0), 5), "follow1_ms": round(statistics.mean(this1), 5),
               "follow1_minus_follow0_us": round((statistics.mean(this1) - statistics.mean(this0)) * 1e3, 2)}
        if rounds["parent"]:
            p = [r[key0]["median_ms"] for r in rounds["parent"]]
            delta, spread = statistics.mean(this0) - statistics.mean(p), abs(p[0] - p[1])
            row.update(parent_ms=round(statistics.mean(p), 5), follow0_minus_parent_us=round(delta * 1e3, 2),
                       parent_round_spread_us=round(spread * 1e3, 2), follow0_within_parent_spread=bool(abs(delta) <= spread))
        summary[stem] = row
    rec["summary"] = summary
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
