#!/usr/bin/env python3
"""Timing of the UE's initial cell search on the device: oai4g_sync_time_batch (k_sync_time: the PSS time-domain
correlation, one workgroup of 4 waves per 64 positions of both half frames, then k_sync_peak) and oai4g_sss_batch
(the offsets, four slot_fep symbols per antenna and k_sss, one workgroup per frame) at 6 / 25 / 100 PRB with 1 and 2
receive antennas.  HIP events around each launch after a warm-up, the median of --reps launches, one JSON line.

A term is one complex product of one replica tap with one received sample: per frame
2 halves x (length - N) / 4 positions x 3 sequences x N taps x nb_rx.  Beside the time per frame and the terms per
second the tool prints the fraction of the VALU-issue bound: the inner loop of k_sync_time spends, per wave and per
4 taps of its 64 positions and 3 sequences (768 terms), 24 v_dot2_i32_i16, 24 v_ashrrev_i32 and 12 v_add3_u32 (the
listing of oai4g_sync_rx.hip; loads, address arithmetic and the per-pass reduction are not counted), which at the
issue rates measured on this machine with 8 waves per SIMD (profiles/valu_rate_r04.txt: 4.44, 2.44 and 4.25 cycles)
is 216 cycles, on 256 CUs x 4 SIMDs at 2.4 GHz.

    python tools/sync_rx_time.py [--reps 15] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from pdcch_front_time import timed  # noqa: E402  (tools/ is the script's directory)

STEP_OPS = {"v_dot2_i32_i16": (24, 4.44), "v_ashrrev_i32": (24, 2.44), "v_add3_u32": (12, 4.25)}
STEP_TERMS = 4 * 64 * 3
SIMDS, CLOCK = 256 * 4, 2.4e9
FRAMES = {6: 64, 25: 16, 100: 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_rx_timing.txt"))
    args = ap.parse_args()
    import torch
    import openair4g_amd as oai
    oai.init()
    sid = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(21)
    cycles = sum(n * c for n, c in STEP_OPS.values())
    bound = SIMDS * CLOCK / (cycles / STEP_TERMS)
    out = {"reps": args.reps, "step_cycles": round(cycles, 1), "bound_terms_per_s": round(bound)}
    for N_RB, n in FRAMES.items():
        for nb_rx in (1, 2):
            fp = oai.frame_parms(N_RB)
            N, length = fp.ofdm_symbol_size, 5 * fp.samples_per_tti
            with oai.sync_batch(fp, n, nb_rx) as sb:
                sb.upload(rng.integers(-2000, 2001, size=(n, nb_rx, 4 * length)).astype(np.int16).view(np.int32))
                med, lo, hi = timed(lambda: sb.launch(stream=sid), torch, args.warmup, args.reps)
                smed, slo, shi = timed(lambda: sb.launch_sss(stream=sid), torch, args.warmup, args.reps)
            terms = n * 2 * ((length - N) // 4) * 3 * N * nb_rx
            out[f"sync{N_RB}_{nb_rx}rx"] = {
                "frames": n, "us_median": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
                "us_per_frame": round(med / n, 2), "terms": terms, "terms_per_s": round(terms / med * 1e6),
                "fraction_of_valu_bound": round(terms / med * 1e6 / bound, 3),
                "sss_us_median": round(smed, 1), "sss_us_min": round(slo, 1), "sss_us_max": round(shi, 1),
                "sss_us_per_frame": round(smed / n, 2)}
    print(json.dumps(out))
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "sync_time_ref.json")))["seconds"]
    lines = [
        "UE initial cell search on one MI355X (gfx950), tools/sync_rx_time.py on " + oai.device_name() + ":",
        "HIP events around each launch, %d warm-up launches, median (min .. max) of %d launches." % (args.warmup, args.reps),
        "",
        "oai4g_sync_time_batch (k_sync_time + k_sync_peak).  A term is one complex product of a replica tap with a received",
        "sample: per frame 2 halves x (length - N) / 4 positions x 3 sequences x N taps x antennas.  The VALU-issue bound",
        "counts the inner loop alone: per wave and 4 taps of 64 positions and 3 sequences (768 terms) 24 v_dot2_i32_i16,",
        "24 v_ashrrev_i32 and 12 v_add3_u32, %.0f cycles at the rates of profiles/valu_rate_r04.txt (8 waves per SIMD)," % cycles,
        "on 1024 SIMDs at 2.4 GHz: %.2e terms/s.  No target was set for this kernel; this is its first measurement." % bound,
        "",
        "case          frames   launch us (min..max)      us/frame   terms/s     of VALU bound   oai4g_sss_batch us (min..max)   us/frame",
    ]
    for N_RB, n in FRAMES.items():
        for nb_rx in (1, 2):
            r = out[f"sync{N_RB}_{nb_rx}rx"]
            lines.append("%3d PRB %d RX  %6d   %8.1f (%8.1f..%8.1f)  %8.2f   %.3e   %5.3f           %8.1f (%8.1f..%8.1f)          %8.2f" % (
                N_RB, nb_rx, n, r["us_median"], r["us_min"], r["us_max"], r["us_per_frame"], r["terms_per_s"],
                r["fraction_of_valu_bound"], r["sss_us_median"], r["sss_us_min"], r["sss_us_max"], r["sss_us_per_frame"]))
    lines += ["",
              "For context, the reference's lte_sync_time on one CPU core of the machine that generated",
              "tests/golden/sync_time_ref.json (seconds per frame, the fastest of its runs): "
              + ", ".join("%s PRB x %s RX %.4f" % tuple(k.split("x") + [v]) for k, v in sorted(ref.items(), key=lambda kv: (int(kv[0].split("x")[0]), kv[0]))) + "."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
