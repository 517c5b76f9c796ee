"""What packet mode of the PCM gateway (nutls_set_pcm_packet, nutls_enhance_packet_pcm) costs: B = 256 streams of 8 kHz mu-law, 20 ms packets
(P = 160 samples) against the 16 ms hop (S = 128), on this library, with the hop entry of the parent commit's library beside it.

    python tools/bench_pcm_packet.py --parent-lib PATH [--out profiles/pcm_packet_bench.json]

Measured, per process:
  (a) nutls_enhance_hop_pcm, device buffers, ms per hop -- this library and the parent's: the hop entries are claimed unchanged;
  (b) packet mode, all streams in phase, NULL mask: nutls_enhance_packet_pcm on device buffers and nutls_enhance_packet_pcm_host on pageable
      arrays, ms per tick (1.25 hops per tick: rounds 1, 1, 1, 2) and per 16 ms of audio (x 128 / 160);
  (c) packet mode with 64 streams at each of the four phases (they join one tick apart) and HOST masks, nutls_enhance_packet_pcm_host: every
      tick then runs a full round and a round in which 64 streams step and 192 are held -- the held-state copies show.
--parent-lib: a libnutls_hip.so built from the PARENT commit (a checkout of it, `python -m nunet_amd.build`); it has (a) only.  One child
process per library and round (a fresh HIP context each), in the order parent, this, parent, this, in one job on one box; every figure of the
summary is the mean of the two rounds' medians.  There is no threshold for (b) and (c); (a) of this library is held against the parent's,
and the margin is the spread between the two rounds of the parent itself (`hop_vs_parent`).

Measured like tools/bench_pcm_g711.py: untimed calls for --condition-ms first, a warm-up, then `windows` windows of `calls` calls (a multiple
of 4 ticks: whole cycles); minimum, median and maximum over the windows.  Device buffers between HIP events, host arrays by wall clock.
Input: white noise at speech level (0.05 N(0,1)), quantised and compressed with the library's own nutls_pcm_g711_compress.  One JSON line
(and --out).
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
FMT = "ulaw"
P = 160


def child(args):
    """One library, one process: one JSON line."""
    import numpy as np
    import torch
    from nunet_amd import NutlsEngine, runner

    res, info = {}, {}
    eng = NutlsEngine(batch=B)
    assert eng.mode == "fused" and eng.launches_per_hop == 3
    eng.set_pcm_format(RATE, FMT)
    S = eng.pcm_hop_samples
    gen = torch.Generator().manual_seed(1234)
    s16 = (0.05 * torch.randn(8, B, max(P, S), generator=gen) * 32768.0).round().clamp(-32768, 32767).to(torch.int16).numpy()
    codes = runner.g711_compress(FMT, s16)
    k = [0]

    # (a) the hop entry
    xs, out = torch.from_numpy(np.ascontiguousarray(codes[:, :, :S])).cuda(), torch.empty(B, S, dtype=torch.uint8, device="cuda")

    def hop():
        k[0] += 1
        eng.enhance_hop_pcm(xs[k[0] & 7], "edge", out)

    res["enhance_hop_pcm"] = timed(torch, hop, args.calls, args.windows, args.condition_ms, wall=False)
    torch.cuda.synchronize()
    assert len(set(out.cpu().numpy().ravel().tolist())) > 16      # (audio came back, not one code)
    if not args.parent:
        pk = np.ascontiguousarray(codes[:, :, :P])
        # (b) in phase, NULL mask
        eng.reset()
        eng.set_pcm_packet(P)
        assert eng.pcm_packet_delay_samples == 96
        xd, od = torch.from_numpy(pk).cuda(), torch.empty(B, P, dtype=torch.uint8, device="cuda")
        rounds = []

        def tick():
            k[0] += 1
            eng.enhance_packet_pcm(xd[k[0] & 7], "edge", od)

        for _ in range(8):
            tick()
            rounds.append(eng.pcm_packet_last_rounds)
        assert rounds == [1, 1, 1, 2] * 2, rounds
        res["packet_in_phase"] = timed(torch, tick, args.calls, args.windows, args.condition_ms, wall=False)
        torch.cuda.synchronize()
        assert len(set(od.cpu().numpy().ravel().tolist())) > 16
        xh, oh = [np.ascontiguousarray(v) for v in pk], np.empty((B, P), np.uint8)

        def tick_host(mask=None):
            k[0] += 1
            eng.enhance_packet_pcm(xh[k[0] & 7], "edge", oh, active=mask)

        eng.reset()
        res["packet_in_phase_host"] = timed(torch, tick_host, args.calls, args.windows, args.condition_ms, wall=True)
        # (c) four phases, host masks
        eng.reset()
        group = np.arange(B) // (B // 4)
        for t in range(4):      # 64 streams join at each of four consecutive ticks
            tick_host(group <= t)
        fills = eng.pcm_packet_fill()
        assert sorted(set(fills.tolist())) == [0, 32, 64, 96] and all(int((fills == f).sum()) == B // 4 for f in (0, 32, 64, 96)), fills
        everyone = np.ones(B, bool)
        rounds = []
        for _ in range(4):
            tick_host(everyone)
            rounds.append(eng.pcm_packet_last_rounds)
        assert rounds == [2] * 4, rounds
        res["packet_four_phases_host_masks"] = timed(torch, lambda: tick_host(everyone), args.calls, args.windows, args.condition_ms, wall=True)
        assert len(set(oh.ravel().tolist())) > 16
        info = {"hops_per_tick_in_phase": 1.25, "rounds_per_tick_four_phases": 2, "held_streams_in_second_round": B - B // 4}
    eng.close()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "ms_per_call": res, "info": info}))


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
    if args.calls % 4:
        raise SystemExit("--calls must be a multiple of 4: a cycle of 20 ms packets against 16 ms hops is 4 ticks")
    if args.child:
        return child(args)
    rec = {"what": "B = %d streams of %d Hz mu-law, packets of %d samples: ms per call, min / median / max over %d windows of %d calls after %.0f ms "
                   "of clock conditioning; device buffers between HIP events, pageable host arrays by wall clock; one process per library and "
                   "round, order parent, this, parent, this; summary: mean of the two rounds' medians" % (B, RATE, P, args.windows, args.calls, args.condition_ms)}
    rounds = {"parent": [], "this": []}
    for rnd in (1, 2):
        for which in ("parent", "this"):
            if which == "parent" and not args.parent_lib:
                continue
            got = spawn(args, which == "parent")
            rec["device"] = got["device"]
            rec["%s_round%d" % (which, rnd)] = got["ms_per_call"]
            if got["info"]:
                rec["info"] = got["info"]
            rounds[which].append(got["ms_per_call"])

    def mean(which, key):
        return statistics.mean(r[key]["median_ms"] for r in rounds[which])

    hop = mean("this", "enhance_hop_pcm")
    rec["summary"] = {key + "_ms": round(mean("this", key), 5) for key in rounds["this"][0]}
    for key in rounds["this"][0]:
        if key.startswith("packet"):
            rec["summary"][key + "_per_16ms_of_audio_ms"] = round(mean("this", key) * 128.0 / P, 5)
            rec["summary"][key + "_in_hops"] = round(mean("this", key) / hop, 3)
    if rounds["parent"]:
        p = [r["enhance_hop_pcm"]["median_ms"] for r in rounds["parent"]]
        spread, delta = abs(p[0] - p[1]), hop - statistics.mean(p)
        rec["hop_vs_parent"] = {"parent_ms": round(statistics.mean(p), 5), "this_ms": round(hop, 5), "this_minus_parent_ms": round(delta, 5),
                                "parent_round_spread_ms": round(spread, 5), "within_parent_spread": bool(abs(delta) <= spread)}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
