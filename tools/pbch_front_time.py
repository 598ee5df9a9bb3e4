#!/usr/bin/env python3
"""Timing of the batched PBCH receive front end and the detection behind it: oai4g_pbch_front_batch
(k_pbch_front, one workgroup per subframe, one wave per PBCH symbol) and oai4g_pbch_detect_batch (eight decodes
per subframe and the resolve) over 4096 subframes at 6 and 100 PRB, 1 port x 1 RX and 2 ports x 2 RX,
high_speed_flag = 1.  The work does not depend on the bandwidth (72 subcarriers of four symbols); only the
strides between what is read do.  HIP events around each launch after a warm-up, the median of --reps launches,
one JSON line.  Beside the time it prints the bytes a front launch must move: per subframe the 48 + 48 + 72 + 72
extracted samples of every antenna and estimates of every (port, antenna) plane read once, the 2 x 480 soft bits
and the four shifts written once; and that count over the time as a fraction of --stream-tbs, the rate a
streaming kernel sustains on this machine.

    python tools/pbch_front_time.py [--subframes 4096] [--reps 15] [--stream-tbs 6.3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pdcch_front_time import timed  # noqa: E402  (tools/ is the script's directory)


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
    rng = np.random.default_rng(12)
    n = args.subframes
    out = {"subframes": n, "reps": args.reps, "stream_tbs": args.stream_tbs}
    for N_RB in (6, 100):
        for nb_tx, nb_rx in ((1, 1), (2, 2)):
            kw = dict(nb_antennas_tx=2, mode1_flag=0) if nb_tx == 2 else {}
            fp = oai.frame_parms(N_RB, 137, **kw)
            grid = fp.symbols_per_tti * fp.ofdm_symbol_size
            fb = oai.PbchFrontBatch(fp, n, nb_rx, nb_tx, 1)
            # 16 distinct subframes tiled over the batch: every subframe still reads its own memory
            one = rng.integers(-2000, 2001, size=(16, nb_rx * grid * 2)).astype(np.int16).view(np.int32)
            rx = np.ascontiguousarray(np.tile(one, (n // 16 + 1, 1))[:n])
            d_rx = oai.lib().oai4g_dev_alloc(rx.nbytes)
            assert d_rx and oai.lib().oai4g_memcpy_h2d(d_rx, oai._ptr(rx), rx.nbytes) == 0
            del rx
            h = rng.integers(-300, 301, size=(16, grid * 2)).astype(np.int16).view(np.int32)
            plane = np.ascontiguousarray(np.tile(h, (n // 16 + 1, 1))[:n])
            fb.upload_estimates({(p, a): plane for p in range(nb_tx) for a in range(nb_rx)})
            del plane
            med, lo, hi = timed(lambda: fb.launch(d_rx, stream=sid), torch, args.warmup, args.reps)
            nbytes = n * (4 * 240 * (nb_rx + nb_tx * nb_rx) + 2 * 480 + 4)
            dmed, dlo, dhi = timed(lambda: fb.detect(stream=sid), torch, args.warmup, args.reps)
            out[f"front{N_RB}_{nb_tx}x{nb_rx}"] = {
                "us_median": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1), "bytes": nbytes,
                "subframes_per_s": round(n / med * 1e6), "tb_per_s": round(nbytes / med / 1e6, 3),
                "fraction_of_stream": round(nbytes / med / 1e6 / args.stream_tbs, 3),
                "detect_us_median": round(dmed, 1), "detect_us_min": round(dlo, 1), "detect_us_max": round(dhi, 1)}
            fb.close()
            oai.lib().oai4g_dev_free(d_rx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
