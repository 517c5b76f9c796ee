"""Waveform block mode: what the block front end / back end (csrc/stft_block.hip) costs beside the model.

    python tools/bench_enhance_block.py [--out profiles/enhance_block_bench.json]

For 1 x 1024 and 8 x 1024 frames, on device buffers, one handle per shape, all in this process: nutls_process_block alone,
nutls_enhance_block (analysis + model + synthesis), nutls_stft_block + nutls_istft_block alone and each of the two on its
own; for comparison 1024 x nutls_enhance_hop on a batch-8 streaming handle.  HIP events around windows of back-to-back
calls on one stream after a warm-up; every figure is reported as the minimum and the median over the windows.  The
bytes of the two kernels (PCM, magnitudes, phasors: what they must move) over their times are set against the HBM peak.
One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

HBM_PEAK_TBS = 8.0
FRAMES = 1024


def timed(torch, fn, calls: int, windows: int, warmup: int = 3):
    """ms per call: [min, median] over `windows` windows of `calls` back-to-back calls."""
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
    return {"min_ms": round(min(ms), 5), "median_ms": round(statistics.median(ms), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    import torch
    from nunet_amd import NutlsEngine, NutlsOffline

    rng = np.random.default_rng(0)
    rec = {"what": "waveform block mode, device buffers, HIP events, ms per call (min / median over %d windows)" % args.windows,
           "device": torch.cuda.get_device_name(0), "frames": FRAMES, "hbm_peak_TBs": HBM_PEAK_TBS, "shapes": {}}
    for utts in (1, 8):
        off = NutlsOffline(max_frames=FRAMES, utterances=utts)
        pcm = torch.from_numpy((0.1 * rng.standard_normal((utts, FRAMES * 256))).astype(np.float32)).cuda()
        out = torch.empty_like(pcm)
        mag = off.stft_block_device(pcm)
        est = torch.empty_like(mag)
        r = {}
        r["process_block"] = timed(torch, lambda: off.process_block_device(mag, est), 4, args.windows)
        r["enhance_block"] = timed(torch, lambda: off.enhance_block_device(pcm, out), 4, args.windows)

        def both():
            off.stft_block_device(pcm, mag)
            off.istft_block_device(mag, out)
        r["stft_plus_istft"] = timed(torch, both, 50, args.windows)
        r["stft_block"] = timed(torch, lambda: off.stft_block_device(pcm, mag), 50, args.windows)
        r["istft_block"] = timed(torch, lambda: off.istft_block_device(mag, out), 50, args.windows)
        n = utts * FRAMES
        by = {"stft_block": n * (256 * 4 + 256 * 4 + 257 * 8), "istft_block": n * (256 * 4 + 257 * 8 + 256 * 4)}
        for k, b in by.items():
            r[k]["bytes"] = b
            r[k]["TBs_at_min"] = round(b / (r[k]["min_ms"] * 1e-3) / 1e12, 3)
            r[k]["share_of_hbm_peak"] = round(r[k]["TBs_at_min"] / HBM_PEAK_TBS, 4)
        r["front_and_back_share_of_enhance_block"] = round(1.0 - r["process_block"]["median_ms"] / r["enhance_block"]["median_ms"], 4)
        r["stft_plus_istft_over_process_block"] = round(r["stft_plus_istft"]["median_ms"] / r["process_block"]["median_ms"], 4)
        r["frames_per_s_enhance_block"] = round(n / (r["enhance_block"]["median_ms"] * 1e-3))
        rec["shapes"]["%dx%d" % (utts, FRAMES)] = r
        off.close()
    eng = NutlsEngine(batch=8)
    hop = torch.from_numpy((0.1 * rng.standard_normal((8, 256))).astype(np.float32)).cuda()
    o = torch.empty_like(hop)
    s = timed(torch, lambda: eng.enhance_hop(hop, out=o), FRAMES, 3, warmup=20)
    eng.close()
    rec["streaming_batch8_1024_enhance_hop"] = {"min_ms": round(s["min_ms"] * FRAMES, 3), "median_ms": round(s["median_ms"] * FRAMES, 3),
                                                "per_hop_us_median": round(s["median_ms"] * 1e3, 2)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
