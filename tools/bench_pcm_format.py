"""What the PCM gateway (nutls_set_pcm_format, the _pcm entries) costs: ms per streaming hop at B = 256 for nutls_enhance_hop and for
nutls_enhance_hop_pcm in the callers' formats -- the plain hop plus the two conversion launches (csrc/pcm.hip).

    python tools/bench_pcm_format.py [--parent-lib PATH] [--out profiles/pcm_format_bench.json]

Measured, per process:
  * device buffers (asynchronous: `calls` back-to-back calls between two HIP events): nutls_enhance_hop, and nutls_enhance_hop_pcm at
    int16 / 16 kHz, int16 / 8 kHz, int16 / 48 kHz and float32 / 48 kHz;
  * pageable host buffers (synchronous, wall clock): nutls_enhance_hop_host on float32 against nutls_enhance_hop_pcm_host on int16 at 16 kHz
    (half the bytes over the link), and int16 at 8 and 48 kHz.
--parent-lib: a libnutls_hip.so built from the PARENT commit (a checkout of it, `python -m nunet_amd.build`).  With it, nutls_enhance_hop
of that library is measured in the same job on the same device: the gateway must not change what the plain hop costs.  One child process
per library and round (a fresh HIP context each), in the order parent, this, parent, this; the margin for "unchanged" is the spread
between the two rounds of the parent itself.  Both figures are in the record (`enhance_hop_vs_parent`).

Like bench.py and tools/bench_hop_fusion.py every measurement is taken at steady clocks: untimed calls for --condition-ms first, a warm-up,
then `windows` windows of `calls` calls; minimum, median and maximum over the windows.  Input: white noise at speech level (0.05 N(0,1)).
One JSON line (and --out).
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
DEVICE_FORMATS = (("int16", 16000), ("int16", 8000), ("int16", 48000), ("float32", 48000))
HOST_FORMATS = (("int16", 16000), ("int16", 8000), ("int16", 48000))


def child(args):
    """One library, one process: one JSON line."""
    import numpy as np
    import torch
    from nunet_amd import NutlsEngine

    def t(fn, wall):
        return timed(torch, fn, args.calls, args.windows, args.condition_ms, wall=wall)

    res = {}
    eng = NutlsEngine(batch=B)
    assert eng.mode == "fused" and eng.launches_per_hop == 3
    gen = torch.Generator().manual_seed(1234)
    pool = 0.05 * torch.randn(8, B, 256, generator=gen)
    dev_pool, dev_out = pool.cuda(), torch.empty(B, 256, device="cuda")
    host_pool, host_out = [np.ascontiguousarray(p.numpy()) for p in pool], np.empty((B, 256), np.float32)
    k = [0]

    def plain_device():
        k[0] += 1
        eng.enhance_hop(dev_pool[k[0] & 7], "edge", dev_out)

    def plain_host():
        k[0] += 1
        eng.enhance_hop(host_pool[k[0] & 7], "edge", host_out)

    res["enhance_hop"] = t(plain_device, False)
    res["enhance_hop_host_float32"] = t(plain_host, True)
    if not args.parent:
        for dtype, rate in DEVICE_FORMATS + tuple(("host", f) for f in HOST_FORMATS):
            host = dtype == "host"
            if host:
                dtype, rate = rate
            eng.set_pcm_format(rate, dtype)
            S = eng.pcm_hop_samples
            noise = 0.05 * torch.randn(8, B, S, generator=gen)
            x = (noise * 32768.0).round().clamp(-32768, 32767).to(torch.int16) if dtype == "int16" else noise
            if host:
                xs, out = [np.ascontiguousarray(v.numpy()) for v in x], np.empty((B, S), dtype)
            else:
                xs, out = x.cuda(), torch.empty(B, S, dtype=getattr(torch, dtype), device="cuda")

            def pcm_hop():
                k[0] += 1
                eng.enhance_hop_pcm(xs[k[0] & 7], "edge", out)

            res["enhance_hop_pcm%s_%s_%dk" % ("_host" if host else "", dtype, rate // 1000)] = t(pcm_hop, host)
            torch.cuda.synchronize()
            assert bool(np.isfinite(np.asarray(out if host else out.cpu(), np.float64)).all())
    eng.close()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "ms_per_hop": res}))


def spawn(args, parent):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--windows", str(args.windows),
           "--condition-ms", str(args.condition_ms)]
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
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--condition-ms", type=float, default=200.0)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rec = {"what": "one streaming hop at B = %d, ms per hop: min / median / max over %d windows of %d calls after %.0f ms of clock conditioning; "
                   "device buffers between HIP events, pageable host buffers by wall clock; one process per library and round, order "
                   "parent, this, parent, this" % (B, args.windows, args.calls, args.condition_ms)}
    rounds = {"parent": [], "this": []}
    for rnd in (1, 2):
        for which in ("parent", "this"):
            if which == "parent" and not args.parent_lib:
                continue
            got = spawn(args, which == "parent")
            rec["device"] = got["device"]
            rec["%s_round%d" % (which, rnd)] = got["ms_per_hop"]
            rounds[which].append(got["ms_per_hop"])

    def mean(which, key):
        return statistics.mean(r[key]["median_ms"] for r in rounds[which])

    plain = mean("this", "enhance_hop")
    summary = {"enhance_hop_ms": round(plain, 5)}
    for key in rounds["this"][0]:
        if key.startswith("enhance_hop_pcm_") and "_host_" not in key:
            summary[key + "_ms"] = round(mean("this", key), 5)
            summary[key + "_extra_us"] = round((mean("this", key) - plain) * 1e3, 2)
    host = mean("this", "enhance_hop_host_float32")
    summary["enhance_hop_host_float32_ms"] = round(host, 5)
    for key in rounds["this"][0]:
        if key.startswith("enhance_hop_pcm_host_"):
            summary[key + "_ms"] = round(mean("this", key), 5)
    rec["summary"] = summary
    if rounds["parent"]:
        p = [r["enhance_hop"]["median_ms"] for r in rounds["parent"]]
        spread = abs(p[0] - p[1])
        delta = plain - statistics.mean(p)
        rec["enhance_hop_vs_parent"] = {"parent_ms": round(statistics.mean(p), 5), "this_ms": round(plain, 5), "this_minus_parent_ms": round(delta, 5),
                                        "parent_round_spread_ms": round(spread, 5), "within_parent_spread": bool(delta <= spread)}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
