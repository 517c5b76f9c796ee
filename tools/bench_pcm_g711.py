"""What G.711 in the PCM gateway (NUTLS_PCM_ULAW / NUTLS_PCM_ALAW, 8 kHz) costs: ms per streaming hop at B = 256 for nutls_enhance_hop_pcm at
8 kHz in int16, mu-law and A-law on this library, against int16 on the parent commit's library.

    python tools/bench_pcm_g711.py --parent-lib PATH [--out profiles/pcm_g711_bench.json]

Measured, per process:
  * device buffers (asynchronous: `calls` back-to-back calls between two HIP events): nutls_enhance_hop_pcm at 8000 Hz in each format;
  * pageable host arrays (synchronous, wall clock): nutls_enhance_hop_pcm_host in each format -- 64 KiB each way per hop in int16, 32 KiB in
    G.711: where the quartered bytes should show.
--parent-lib: a libnutls_hip.so built from the PARENT commit (a checkout of it, `python -m nunet_amd.build`); it has int16 only.  One child
process per library and round (a fresh HIP context each), in the order parent, this, parent, this, in one job on one box; every figure of
the summary is the mean of the two rounds' medians.  There is no threshold for the new formats; the int16 figure of this library is held
against the parent's, and the margin for "where the parent's lies" is the spread between the two rounds of the parent itself
(`int16_vs_parent`).

Measured like tools/bench_pcm_format.py: untimed calls for --condition-ms first, a warm-up, then `windows` windows of `calls` calls; minimum,
median and maximum over the windows.  Input: white noise at speech level (0.05 N(0,1)), quantised, and for G.711 compressed with the
library's own nutls_pcm_g711_compress.  One JSON line (and --out).
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
RATE = 8000
FORMATS = ("int16", "ulaw", "alaw")


def child(args):
    """One library, one process: one JSON line."""
    import numpy as np
    import torch
    from nunet_amd import NutlsEngine, runner

    res = {}
    eng = NutlsEngine(batch=B)
    assert eng.mode == "fused" and eng.launches_per_hop == 3
    gen = torch.Generator().manual_seed(1234)
    k = [0]
    for fmt in FORMATS[:1] if args.parent else FORMATS:
        eng.set_pcm_format(RATE, fmt)
        S = eng.pcm_hop_samples
        s16 = (0.05 * torch.randn(8, B, S, generator=gen) * 32768.0).round().clamp(-32768, 32767).to(torch.int16).numpy()
        x = s16 if fmt == "int16" else runner.g711_compress(fmt, s16)
        for host in (False, True):
            if host:
                xs, out = [np.ascontiguousarray(v) for v in x], np.empty((B, S), x.dtype)
            else:
                xs, out = torch.from_numpy(x).cuda(), torch.empty(B, S, dtype=getattr(torch, eng.pcm_dtype), device="cuda")

            def pcm_hop():
                k[0] += 1
                eng.enhance_hop_pcm(xs[k[0] & 7], "edge", out)

            res["enhance_hop_pcm%s_%s" % ("_host" if host else "", fmt)] = timed(torch, pcm_hop, args.calls, args.windows, args.condition_ms, wall=host)
            torch.cuda.synchronize()
            got = out if host else out.cpu().numpy()
            assert got.dtype == x.dtype and len(set(got.ravel().tolist())) > 16      # (audio came back, not one code)
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
    rec = {"what": "one streaming hop at B = %d and %d Hz, ms per hop: min / median / max over %d windows of %d calls after %.0f ms of clock "
                   "conditioning; device buffers between HIP events, pageable host arrays by wall clock; one process per library and round, "
                   "order parent, this, parent, this; summary: mean of the two rounds' medians" % (B, RATE, args.windows, args.calls, args.condition_ms)}
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

    rec["summary"] = {key + "_ms": round(mean("this", key), 5) for key in rounds["this"][0]}
    for where in ("", "_host"):
        base = mean("this", "enhance_hop_pcm%s_int16" % where)
        for fmt in FORMATS[1:]:
            rec["summary"]["enhance_hop_pcm%s_%s_minus_int16_us" % (where, fmt)] = round((mean("this", "enhance_hop_pcm%s_%s" % (where, fmt)) - base) * 1e3, 2)
    if rounds["parent"]:
        rec["int16_vs_parent"] = {}
        for key in ("enhance_hop_pcm_int16", "enhance_hop_pcm_host_int16"):
            p = [r[key]["median_ms"] for r in rounds["parent"]]
            spread = abs(p[0] - p[1])
            delta = mean("this", key) - statistics.mean(p)
            rec["int16_vs_parent"][key] = {"parent_ms": round(statistics.mean(p), 5), "this_ms": round(mean("this", key), 5),
                                           "this_minus_parent_ms": round(delta, 5), "parent_round_spread_ms": round(spread, 5),
                                           "within_parent_spread": bool(abs(delta) <= spread)}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
