#!/usr/bin/env python3
"""Timing of the batched PDCCH / PCFICH receive front end: oai4g_pdcch_front_batch (k_pdcch_front, one
workgroup per subframe) over 4096 subframes at 25 and 100 PRB, 1 TX x 1 RX (SISO) and 2 TX x 2 RX (ALAMOUTI),
high_speed_flag = 1.  HIP events around each launch after a warm-up, the median of --reps launches, one JSON
line.  Beside the time it prints the bytes a launch must move: per subframe the (8 + 12 + 12) N_RB_DL extracted
samples of every antenna and estimates of every (port, antenna) plane read once (the level's second read of the
symbol-1 estimates is not counted), plane 0 written once and the two result bytes; and that count over the time
as a fraction of --stream-tbs, the rate a streaming kernel sustains on this machine.

    python tools/pdcch_front_time.py [--subframes 4096] [--reps 15] [--stream-tbs 6.3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    args = ap.parse_args()
    import torch
    import openair4g_amd as oai
    oai.init()
    sid = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(11)
    n_sf = args.subframes
    out = {"subframes": n_sf, "reps": args.reps, "stream_tbs": args.stream_tbs}
    for N_RB in (25, 100):
        for nb_tx, nb_rx in ((1, 1), (2, 2)):
            kw = dict(nb_antennas_tx=2, mode1_flag=0) if nb_tx == 2 else {}
            fp = oai.frame_parms(N_RB, 137, **kw)
            grid = fp.symbols_per_tti * fp.ofdm_symbol_size
            fb = oai.PdcchFrontBatch(fp, n_sf, nb_rx, 1 if nb_tx == 2 else 0, 1, 0, 1)
            # 16 distinct subframes tiled over the batch: every subframe still reads its own memory
            one = rng.integers(-2000, 2001, size=(16, nb_rx * grid * 2)).astype(np.int16).view(np.int32)
            rx = np.ascontiguousarray(np.tile(one, (n_sf // 16 + 1, 1))[:n_sf])
            d_rx = oai.lib().oai4g_dev_alloc(rx.nbytes)
            assert d_rx and oai.lib().oai4g_memcpy_h2d(d_rx, oai._ptr(rx), rx.nbytes) == 0
            h = rng.integers(-300, 301, size=(16, grid * 2)).astype(np.int16).view(np.int32)
            plane = np.ascontiguousarray(np.tile(h, (n_sf // 16 + 1, 1))[:n_sf])
            fb.upload_estimates({(p, a): plane for p in range(nb_tx) for a in range(nb_rx)})
            med, lo, hi = timed(lambda: fb.launch(d_rx, stream=sid), torch, args.warmup, args.reps)
            words_in = (8 + 12 + 12) * N_RB * (nb_rx + nb_tx * nb_rx)
            nbytes = n_sf * 4 * (words_in + 36 * N_RB) + 2 * n_sf
            out[f"front{N_RB}_{nb_tx}x{nb_rx}"] = {
                "us_median": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1), "bytes": nbytes,
                "subframes_per_s": round(n_sf / med * 1e6), "tb_per_s": round(nbytes / med / 1e6, 3),
                "fraction_of_stream": round(nbytes / med / 1e6 / args.stream_tbs, 3)}
            fb.close()
            oai.lib().oai4g_dev_free(d_rx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
