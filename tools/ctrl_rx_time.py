#!/usr/bin/env python3
"""Timing of the batched UE control decoding: oai4g_pdcch_rx_batch (k_cc_decode fed through the soft-bit
gather table + k_pdcch_resolve) at 25 and 100 PRB over 4096 subframes with the full tmode-1 plan (common
L = 2, 3 and UE-specific L = 0..3, each at two DCI sizes), and oai4g_pbch_decode_batch at 65536 decodes.
HIP events around each launch after a warm-up, the median of --reps runs, one JSON line.  Run it in
several processes to see the process-to-process spread; the decode has no data-dependent path except the
length of the repetition sums, so the inputs are moderate noise.

    python tools/ctrl_rx_time.py [--subframes 4096] [--pbch 65536] [--reps 15] [--only pdcch25|pdcch100|pbch]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def tm1_plan(size_1a, size_1c, size_0, size_1):
    """dci_decoding_procedure's tmode-1 calls (dci.c:2990-3356)"""
    by = lambda b: 4 if b <= 32 else 8
    p = []
    for L in (2, 3):
        p += [(1, L, size_1a, by(size_1a), 2, 2, 0, 0), (1, L, size_1c, by(size_1c), 4, 4, 4, 0)]
    p += [(0, L, size_0, by(size_0), 2, 2, 0, 0) for L in (3, 2, 1, 0)]
    p += [(0, L, size_1, by(size_1), 2, 2, 1, 1) for L in (0, 1, 2, 3)]
    return p


def timed(fn, torch, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in evs)
    return statistics.median(t), t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=4096)
    ap.add_argument("--pbch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import openair4g_amd as oai
    oai.init()
    sid = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    out = {"subframes": args.subframes, "pbch": args.pbch, "reps": args.reps}
    for N_RB, sizes in ((25, (27, 13, 27, 31)), (100, (31, 15, 31, 39))):
        if args.only and args.only != f"pdcch{N_RB}":
            continue
        fp = oai.frame_parms(N_RB, 137)
        b = oai.PdcchRxBatch(fp, 3, 0x1234, 0xFFFF, 0x0002, tm1_plan(*sizes), args.subframes)
        one = rng.integers(-40, 41, size=(16, b.comp_words * 2)).astype(np.int16).view(np.int32)
        b.upload(np.ascontiguousarray(np.tile(one, (args.subframes // 16 + 1, 1))[:args.subframes]))
        n_dec = sum(len(b.candidates(s % 10)) for s in range(args.subframes))
        med, lo, hi = timed(lambda: b.launch(0, stream=sid), torch, args.warmup, args.reps)
        out[f"pdcch{N_RB}"] = {"decodes": n_dec, "us_median": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                               "decodes_per_s": round(n_dec / med * 1e6)}
        b.close()
    if not args.only or args.only == "pbch":
        fp = oai.frame_parms(25, 137)
        b = oai.PbchDecodeBatch(fp, args.pbch)
        one = rng.integers(-20, 21, size=(64, b.E)).astype(np.int8)
        b.upload(np.ascontiguousarray(np.tile(one, (args.pbch // 64 + 1, 1))[:args.pbch]), np.arange(args.pbch) & 3)
        med, lo, hi = timed(lambda: b.launch(stream=sid), torch, args.warmup, args.reps)
        out["pbch"] = {"decodes": args.pbch, "us_median": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                       "decodes_per_s": round(args.pbch / med * 1e6)}
        b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
