#!/usr/bin/env python3
"""A/B timing of the TM4-6 demodulator against the TM3 one at the UE3 bench shape (100 PRB, 2 RX
antennas, 64-QAM, estimate planes): RxBatchTM56.launch (k_rx_level_dual<false, true> +
k_rx_llr_prec<6, false, RX_TM56>) and RxBatchTM3.launch (k_rx_level_tm3 + k_rx_llr_prec<6, false, RX_TM3>)
alternate inside one process on the same FEP output and the same estimate planes, HIP events around each
launch, medians printed as one JSON line.  Both kernels load the same words per RE (two estimate planes per RX antenna and one
received word).  Run it in several processes to see the process-to-process spread; OAI4G_LIB selects the
library build, so the same runs compare two builds.

    python tools/rx_tm56_ab.py [--batch 2048] [--reps 200]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    import openair4g_amd as oai
    oai.init()
    L = oai.lib()
    fp = oai.frame_parms(100, nb_antennas_tx=2, mode1_flag=0)
    n_sf, nb_rx, N, nsymb = args.batch, 2, fp.ofdm_symbol_size, fp.symbols_per_tti
    ra = [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xF]
    rng = np.random.default_rng(56)
    # moderate random words (one subframe's worth, repeated): the kernels have no data-dependent path
    def words(n_rows):
        one = rng.integers(-3000, 3000, (nsymb * N, 2)).astype(np.int16).view(np.int32).reshape(-1)
        return np.ascontiguousarray(np.tile(one, n_rows))
    rxF = words(n_sf * nb_rx)
    d_rxF = L.oai4g_dev_alloc(rxF.nbytes)
    assert d_rxF and L.oai4g_memcpy_h2d(d_rxF, rxF.ctypes.data, rxF.nbytes) == 0
    tm3 = oai.RxBatchTM3(fp, ra, 6, 6, 19, 1, 0x1234, n_sf, nb_rx=nb_rx, first_subframe=0)
    tm56 = oai.RxBatchTM56(fp, ra, 6, oai.PUSCH_PRECODING0, 0xE4B1, 1, 0x1234, n_sf, nb_rx=nb_rx, first_subframe=0,
                           pmi_rule=oai.RX_PMI_TX)
    est = words(4 * n_sf)
    for rb in (tm3, tm56):
        assert L.oai4g_memcpy_h2d(rb.d_est, est.ctypes.data, est.nbytes) == 0
    sid = torch.cuda.current_stream().cuda_stream
    runs = {"tm3": lambda: tm3.launch(d_rxF, 1, stream=sid), "tm56": lambda: tm56.launch(d_rxF, 1, stream=sid)}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {"batch": n_sf, "reps": args.reps}
    for k, pairs in evs.items():
        t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs)
        out[k + "_us_median"] = round(statistics.median(t), 2)
        out[k + "_us_p10"] = round(t[len(t) // 10], 2)
        out[k + "_us_p90"] = round(t[(9 * len(t)) // 10], 2)
    out["tm56_over_tm3"] = round(out["tm56_us_median"] / out["tm3_us_median"], 4)
    tm3.close()
    tm56.close()
    L.oai4g_dev_free(ctypes.c_void_p(d_rxF))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
