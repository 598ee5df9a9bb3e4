#!/usr/bin/env python3
"""Timing of the SC-FDMA layer on the device: oai4g_pusch_mod_batch (k_pusch_mod: scrambling, QAM, transform
precoding and RE mapping of a subframe's 12 PUSCH symbols, one launch) and oai4g_pusch_idft_batch (k_pusch_idft:
lte_idft in place on the 12 data symbols of a compensated grid) at --subframes subframes of a 6, 25, 50 and 100 PRB
allocation in a 100 PRB carrier, 16-QAM.  HIP events around each launch after a warm-up, the median of --reps
launches, one JSON line, and profiles/pusch_timing.txt.

Each time stands beside two figures: the time a streaming kernel needs for the bytes the kernel must move (k_pusch_mod
reads G bytes of h and writes 12 Msc words per subframe; k_pusch_idft reads and writes 12 Msc words) at --stream-tbs,
the rate a streaming kernel sustains on this machine, and the reference's ulsch_modulation on one
CPU core, from tests/golden/pusch_ref.json.

    python tools/pusch_time.py [--subframes 4096] [--reps 15] [--stream-tbs 6.3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from pdcch_front_time import timed  # noqa: E402  (tools/ is the script's directory)

ALLOCATIONS = (6, 25, 50, 100)
QM = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subframes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pusch_timing.txt"))
    args = ap.parse_args()
    import torch
    import openair4g_amd as oai
    oai.init()
    sid = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(33)
    n_sf = args.subframes
    fp = oai.frame_parms(100, 11)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "pusch_ref.json")))["seconds"]
    out = {"subframes": n_sf, "reps": args.reps, "stream_tbs": args.stream_tbs, "Qm": QM}
    for nb_rb in ALLOCATIONS:
        with oai.PuschBatch(fp, n_sf, 0, nb_rb, QM, 0, 0x1234, 0, 1) as b:
            b.upload_h(rng.integers(0, 2, (n_sf, b.G), dtype=np.uint8))
            b.d_txdataF = b._dev(n_sf * b.nsymb * b.N * 4, zero=True)
            one = rng.integers(-2000, 2001, (1, b.nsymb, 12 * fp.N_RB_DL, 2)).astype(np.int16)
            b.upload_comp(np.tile(one, (n_sf, 1, 1, 1)))
            mod = timed(lambda: b.launch_mod(512, stream=sid), torch, args.warmup, args.reps)
            idft = timed(lambda: b.launch_idft(stream=sid), torch, args.warmup, args.reps)
            words = 12 * b.Msc
            for name, (med, lo, hi), nbytes in (("mod", mod, n_sf * (b.G + 4 * words)), ("idft", idft, n_sf * 8 * words)):
                out[f"{name}_{nb_rb}"] = {
                    "us_median": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1), "bytes": nbytes,
                    "ns_per_subframe": round(med / n_sf * 1e3, 1), "stream_us": round(nbytes / args.stream_tbs / 1e6, 1),
                    "fraction_of_stream": round(nbytes / med / 1e6 / args.stream_tbs, 3),
                    "symbols_per_s": round(12 * n_sf / med * 1e6)}
            out[f"mod_{nb_rb}"]["cpu_core_us_per_subframe"] = round(ref[str(nb_rb)] * 1e6, 1)
            out[f"mod_{nb_rb}"]["cpu_core_over_gpu"] = round(ref[str(nb_rb)] * 1e6 / (mod[0] / n_sf), 0)
    print(json.dumps(out))
    lines = [
        "SC-FDMA layer on one MI355X (gfx950), tools/pusch_time.py on " + oai.device_name() + ":",
        "%d subframes of one allocation in a 100 PRB carrier, %d-QAM, normal prefix, 12 PUSCH symbols per subframe." % (n_sf, 1 << QM),
        "HIP events around each launch, %d warm-up launches, median (min .. max) of %d launches." % (args.warmup, args.reps),
        "stream us: the time for the bytes the kernel must move (k_pusch_mod: G bytes of h in, 12 Msc words out;",
        "k_pusch_idft: 12 Msc words in and out) at %.1f TB/s.  CPU core: the reference's ulsch_modulation, one call," % args.stream_tbs,
        "tests/golden/pusch_ref.json.  No target was set for these kernels; this is their first measurement.",
        "",
        "kernel        PRB   launch us (min..max)        ns/subframe   stream us   of stream   symbols/s    CPU core us/subframe   CPU core / GPU",
    ]
    for name in ("mod", "idft"):
        for nb_rb in ALLOCATIONS:
            r = out[f"{name}_{nb_rb}"]
            cpu = "%10.1f             %8.0f" % (r["cpu_core_us_per_subframe"], r["cpu_core_over_gpu"]) if name == "mod" else ""
            lines.append("k_pusch_%-4s  %3d   %8.1f (%8.1f..%8.1f)  %10.1f   %8.1f    %5.3f      %.3e   %s" % (
                name, nb_rb, r["us_median"], r["us_min"], r["us_max"], r["ns_per_subframe"], r["stream_us"],
                r["fraction_of_stream"], r["symbols_per_s"], cpu))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
