"""What per-utterance hop counts in the callers' format (nutls_enhance_block_pcm_ragged) cost -- and what the uniform PCM block pays for
their existence.

    python tools/bench_ragged_pcm.py [--parent-lib PATH/libnutls_hip.so] [--out profiles/ragged_pcm_bench.json]

8 utterances x 1024 hops of int16 at 8 kHz and at 48 kHz, one child process per library and round (a fresh HIP context each):

  (a) the UNIFORM call, nutls_enhance_block_pcm on device buffers: this tree's library, and -- with --parent-lib, a build of the parent
      commit's library -- the parent's, interleaved parent / branch / parent / branch in the same job on the same device.  The two parent
      rounds give the run-to-run spread of the box; the branch must lie within it (the counts may cost the uniform call nothing).
  (b) the RAGGED call with all counts full against the uniform call of the same handle, two interleaved rounds.
  (c) NutlsOffline.enhance_many(rate=8000) on int16, the synthetic corpus of tools/bench_ragged_block.py (40 recordings) through 8 slots
      of 1024 hops, against the same recordings one after the other through enhance_wave on a one-utterance handle of 1024 hops: useful
      hops per second of wall time (host clock around the whole call, PCM in host memory both ways), two rounds each, interleaved.

(a) and (b) are timed as in tools/bench_ragged_block.py (`timed`: clock conditioning, warm-up, windows of back-to-back calls between two
HIP events; minimum and median over the windows).  Input: white noise at 0.1 of full scale.  One JSON line (and --out).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ragged_block import FRAMES, LENGTHS_IN_HOPS, U, timed      # noqa: E402

RATES = (8000, 48000)


def child(args):
    """One library, one process: the cases named in --cases ("uniform@8000", "ragged_full@48000", "corpus"), one JSON line."""
    import numpy as np
    import torch
    from nunet_amd import NutlsOffline

    res = {}
    cases = args.cases.split(",")
    block_cases = [c for c in cases if c != "corpus"]
    if block_cases:
        off = NutlsOffline(max_frames=FRAMES, utterances=U)
        full = torch.full((U,), FRAMES, dtype=torch.int32, device="cuda")
        rate_now = None
        for case in block_cases:      # (in the order given: "uniform@8000,ragged_full@8000,uniform@8000,ragged_full@8000" interleaves two rounds on one handle)
            kind, rate = case.split("@")
            if rate != rate_now:
                off.reset()
                off.set_pcm_format(int(rate), "int16")
                gen = torch.Generator().manual_seed(1234)
                x = (0.1 * 32768.0 * torch.randn(U, FRAMES * off.pcm_hop_samples, generator=gen)).clamp(-32768, 32767).to(torch.int16).cuda()
                out = torch.empty_like(x)
                rate_now = rate
            fn = (lambda: off.enhance_block_pcm_device(x, out)) if kind == "uniform" else (lambda: off.enhance_block_pcm_device(x, out, hops=full))
            key = "%s_%s_round%d" % (kind, rate, 1 + sum(k.startswith("%s_%s_" % (kind, rate)) for k in res))
            res[key] = timed(torch, fn, args.calls, args.windows, args.condition_ms)
            torch.cuda.synchronize()
            assert bool(out.any())
        off.close()
    if "corpus" in cases:
        rate = 8000
        rng = np.random.default_rng(99)
        waves = [np.rint(0.1 * 32768.0 * rng.standard_normal(n * 128)).clip(-32768, 32767).astype(np.int16) for n in LENGTHS_IN_HOPS]
        useful = sum(LENGTHS_IN_HOPS)
        many = NutlsOffline(max_frames=FRAMES, utterances=U)
        one = NutlsOffline(max_frames=FRAMES)

        def alone():
            outs = []
            for w in waves:
                one.reset()
                outs.append(one.enhance_wave(w, rate))
            return outs

        many.enhance_many(waves[:U], rate=rate)          # warm-up of both handles: code objects, staging buffers
        alone_out = alone()
        reps = 3          # (passes over the corpus per timed round)
        for rnd in (1, 2):
            t0 = time.perf_counter()
            for _ in range(reps):
                got = many.enhance_many(waves, rate=rate)
            t1 = time.perf_counter()
            for _ in range(reps):
                alone()
            t2 = time.perf_counter()
            res["enhance_many_round%d" % rnd] = {"seconds_per_pass": round((t1 - t0) / reps, 4), "useful_hops_per_s": round(useful * reps / (t1 - t0))}
            res["one_utterance_enhance_wave_round%d" % rnd] = {"seconds_per_pass": round((t2 - t1) / reps, 4), "useful_hops_per_s": round(useful * reps / (t2 - t1))}
        assert all(g.shape == w.shape and g.dtype == np.int16 for g, w in zip(got, waves))
        worst = max(int(np.abs(g.astype(np.int32) - r.astype(np.int32)).max()) for g, r in zip(got, alone_out))
        res["corpus"] = {"recordings": len(waves), "rate": rate, "dtype": "int16", "useful_hops": useful,
                         "worst_int16_difference_vs_one_utterance_handles": worst}
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
    ap.add_argument("--cases", default="uniform@8000")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rec = {"what": "offline batch handle, %d utterances x %d hops of int16 on device buffers, ms per call: min / median / max over %d windows of %d "
                   "back-to-back calls (HIP events) after %.0f ms of clock conditioning; one process per library and round"
                   % (U, FRAMES, args.windows, args.calls, args.condition_ms)}
    uniform = ",".join("uniform@%d" % r for r in RATES)
    a = {}
    if args.parent_lib:      # parent, branch, parent, branch: the parent's two rounds are the box's own spread
        runs = {}
        for who, lib in (("parent_round1", args.parent_lib), ("branch_round1", None), ("parent_round2", args.parent_lib), ("branch_round2", None)):
            runs[who] = spawn(args, lib, uniform)["cases"]
        for r in RATES:
            key = "uniform_%d_round1" % r
            at = {who: got[key] for who, got in runs.items()}
            p = [at["parent_round1"]["median_ms"], at["parent_round2"]["median_ms"]]
            b = [at["branch_round1"]["median_ms"], at["branch_round2"]["median_ms"]]
            at["parent_spread_ms"] = round(abs(p[0] - p[1]), 4)
            at["branch_minus_parent_ms"] = round(statistics.mean(b) - statistics.mean(p), 4)
            at["branch_within_parent_spread"] = bool(at["branch_minus_parent_ms"] <= at["parent_spread_ms"])
            a["int16_%d" % r] = at
    rec["a_uniform_call_parent_vs_branch"] = a
    got = spawn(args, None, ",".join("uniform@%d,ragged_full@%d,uniform@%d,ragged_full@%d" % (r, r, r, r) for r in RATES))
    rec["device"] = got["device"]
    b = got["cases"]
    for r in RATES:
        b["ragged_minus_uniform_ms_%d" % r] = round(
            statistics.mean([b["ragged_full_%d_round1" % r]["median_ms"], b["ragged_full_%d_round2" % r]["median_ms"]])
            - statistics.mean([b["uniform_%d_round1" % r]["median_ms"], b["uniform_%d_round2" % r]["median_ms"]]), 4)
    rec["b_ragged_call_all_counts_full_vs_uniform_same_handle"] = b
    rec["c_enhance_many_synthetic_corpus"] = spawn(args, None, "corpus")["cases"]
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
