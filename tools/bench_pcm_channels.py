"""What the channels of the PCM gateway (nutls_set_pcm_channels) cost: the split and the join launches around the 1-channel entry, on this
library, with the same entries of the parent commit's library beside them.

    python tools/bench_pcm_channels.py --parent-lib PATH [--out profiles/pcm_channels_bench.json]

Measured, per process, device buffers between HIP events:
  (a) nutls_enhance_hop_pcm at B = 256 streams, 8 kHz mu-law: channels 1 and 2;
  (b) nutls_enhance_hop_pcm at B = 256 streams, 48 kHz int16: channels 1 and 2;
  (c) nutls_enhance_block_pcm, 8 utterances x 1 024 hops, 48 kHz int16: channels 1 and 2.
--parent-lib: a libnutls_hip.so built from the PARENT commit (a checkout of it, `python -m nunet_amd.build`); it has channels 1 only.  One
child process per library and round (a fresh HIP context each), in the order parent, this, parent, this, in one job on one box; every figure
of the summary is the mean of the two rounds' medians.  No figure is fixed in advance: channels 1 of this library runs the parent's
instructions and is held against the parent's own spread between its two rounds (`channels_1_vs_parent`); the price of channels 2 is
reported as measured (`channels_2_minus_1_ms`).

Measured like tools/bench_pcm_packet.py: untimed calls for --condition-ms first, a warm-up, then `windows` windows of `calls` calls (the block:
--block-calls); minimum, median and maximum over the windows.  Input: white noise at speech level (0.05 N(0,1)), quantised, and compressed
with the library's own nutls_pcm_g711_compress.  One JSON line (and --out).
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
HOP_CASES = (("hop_8k_ulaw", 8000, "ulaw"), ("hop_48k_int16", 48000, "int16"))
BLOCK_CASE = ("block_8x1024_48k_int16", 48000, "int16")


def child(args):
    """One library, one process: one JSON line."""
    import torch
    from nunet_amd import NutlsEngine, NutlsOffline, runner

    layouts = (1,) if args.parent else (1, 2)
    res = {}
    gen = torch.Generator().manual_seed(1234)

    def noise(rows, n, fmt):
        s16 = (0.05 * torch.randn(rows, n, generator=gen) * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        return torch.from_numpy(runner.g711_compress(fmt, s16.numpy())) if fmt in runner.G711_CODECS else s16

    for name, rate, fmt in HOP_CASES:
        eng = NutlsEngine(batch=B)
        assert eng.mode == "fused" and eng.launches_per_hop == 3
        eng.set_pcm_format(rate, fmt)
        S = eng.pcm_hop_samples
        for ch in layouts:
            if ch > 1:
                eng.set_pcm_channels(ch)
            xs = [noise(B // ch, S * ch, fmt).cuda() for _ in range(8)]      # (noise: any layout of it is noise)
            out, k = torch.empty_like(xs[0]), [0]

            def hop():
                k[0] += 1
                eng.enhance_hop_pcm(xs[k[0] & 7], "edge", out)

            eng.reset()
            res["%s_channels_%d" % (name, ch)] = timed(torch, hop, args.calls, args.windows, args.condition_ms, wall=False)
            torch.cuda.synchronize()
            assert len(set(out.cpu().numpy().ravel().tolist())) > 16      # (audio came back, not one code)
        eng.close()

    name, rate, fmt = BLOCK_CASE
    off = NutlsOffline(max_frames=HOPS, utterances=UTTERANCES)
    off.set_pcm_format(rate, fmt)
    S = off.pcm_hop_samples
    for ch in layouts:
        if ch > 1:
            off.set_pcm_channels(ch)
        x = noise(UTTERANCES // ch, HOPS * S * ch, fmt).cuda()
        out = torch.empty_like(x)
        off.reset()
        res["%s_channels_%d" % (name, ch)] = timed(torch, lambda: off.enhance_block_pcm_device(x, out), args.block_calls, args.windows, 0.0, wall=False, warmup=1)
        torch.cuda.synchronize()
        assert len(set(out[0, :4096].cpu().numpy().ravel().tolist())) > 16
    off.close()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "ms_per_call": res}))


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
    ap.add_argument("--block-calls", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--condition-ms", type=float, default=200.0)
    ap.add_argument("--child-timeout", type=float, default=280.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rec = {"what": "ms per call, min / median / max over %d windows of %d calls (the block: %d) after %.0f ms of clock conditioning (the block: one "
                   "warm-up call); device buffers between HIP events; hop entries at B = %d streams, the block entry at %d utterances x %d hops; one "
                   "process per library and round, order parent, this, parent, this; summary: mean of the two rounds' medians"
                   % (args.windows, args.calls, args.block_calls, args.condition_ms, B, UTTERANCES, HOPS)}
    rounds = {"parent": [], "this": []}
    for rnd in (1, 2):
        for which in ("parent", "this"):
            if which == "parent" and not args.parent_lib:
                continue
            got = spawn(args, which == "parent")
            rec["device"] = got["device"]
            rec["%s_round%d" % (which, rnd)] = got["ms_per_call"]
            rounds[which].append(got["ms_per_call"])

    def medians(which, key):
        return [r[key]["median_ms"] for r in rounds[which]]

    rec["summary"] = {key + "_ms": round(statistics.mean(medians("this", key)), 5) for key in rounds["this"][0]}
    rec["channels_2_minus_1_ms"], rec["channels_1_vs_parent"] = {}, {}
    for name in [c[0] for c in HOP_CASES] + [BLOCK_CASE[0]]:
        one, two = medians("this", name + "_channels_1"), medians("this", name + "_channels_2")
        rec["channels_2_minus_1_ms"][name] = {"mean": round(statistics.mean(two) - statistics.mean(one), 5),
                                              "per_round": [round(b - a, 5) for a, b in zip(one, two)]}
        if rounds["parent"]:
            p = medians("parent", name + "_channels_1")
            spread, delta = abs(p[0] - p[1]), statistics.mean(one) - statistics.mean(p)
            rec["channels_1_vs_parent"][name] = {"parent_ms": round(statistics.mean(p), 5), "this_ms": round(statistics.mean(one), 5),
                                                 "this_minus_parent_ms": round(delta, 5), "parent_round_spread_ms": round(spread, 5),
                                                 "within_parent_spread": bool(abs(delta) <= spread)}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
