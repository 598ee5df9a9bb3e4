#!/usr/bin/env python3
"""Timing of the fading channel on the device: oai4g_multipath_batch (k_multipath: the convolution of two subframes
with the vectors' taps plus dlsim's noise) and oai4g_channel_random_batch (k_channel_taps) at 25 PRB for EPA / EVA /
ETU (5 / 27 / 52 taps at BW 5) and at 100 PRB for ETU (202 taps at BW 20), 1x1 and 2x2, per 4096 trials.  HIP events
around each launch after a warm-up, the median of --reps launches, one JSON line.  The 100 PRB cases run 256 trials
(a 2x2 batch of 4096 would be 3 GB of samples and most of a minute per launch) and are scaled to 4096.

Two bounds stand beside the time of k_multipath:
  bytes    what it must move, the int16 input once and the output once (the shared tail and the taps stay in cache),
           over the 6.29 TB/s a copy reaches on this chip;
  f64      its inner loop's double-precision operations, 4 v_mul_f64 and 4 v_add_f64 per tap, transmit antenna,
           receive antenna and output sample, at the issue rate tools/ubench/f64_rate measures in the same run (a
           dependent-free loop of each, 8 waves per SIMD), on the CUs' SIMDs at 2.4 GHz.
Then the BLER step of MCS 9 at 25 PRB (DlsimBler.step, 4096 trials, no host synchronisation): the link stage alone
and the whole step, through oai4g_awgn_batch (channel_model None), through the general kernel with model AWGN, and
under Rayleigh1 and ETU.

    python tools/channel_time.py [--reps 9] [--warmup 2] [--resources profiles/channel_kernel_resources.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from pdcch_front_time import timed  # noqa: E402  (tools/ is the script's directory)

UBENCH = os.path.join(ROOT, "tools", "ubench", "f64_rate")
HBM = 6.29e12
CLOCK = 2.4e9
CASES = [(25, "EPA", 5.0, 4096), (25, "EVA", 5.0, 4096), (25, "ETU", 5.0, 4096), (100, "ETU", 20.0, 256)]


def f64_rate():
    """cycles per wave instruction of v_mul_f64 / v_add_f64 at 1, 2, 4, 8 waves per SIMD, in a process of its own"""
    if not os.path.exists(UBENCH):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", UBENCH + ".hip", "-o", UBENCH],
                       check=True)
    return json.loads(subprocess.run([UBENCH], capture_output=True, text=True, check=True, timeout=120).stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_timing.txt"))
    ap.add_argument("--resources", default=os.path.join(ROOT, "profiles", "channel_kernel_resources.txt"))
    args = ap.parse_args()
    rate = f64_rate()
    import torch
    import openair4g_amd as oai
    from openair4g_amd.dlsim import DlsimBler
    L = oai.init()
    sid = torch.cuda.current_stream().cuda_stream
    simds = rate["cus"] * 4
    cyc = (rate["v_mul_f64"]["8"] + rate["v_add_f64"]["8"]) / 2          # per wave instruction, half of them each
    out = {"reps": args.reps, "f64_rate_cycles": rate, "simds": simds}
    rng = np.random.default_rng(31)
    for N_RB, model, bw, n in CASES:
        fp = oai.frame_parms(N_RB)
        spt = fp.samples_per_tti
        for nt, nr in ((1, 1), (2, 2)):
            with oai.ChannelBatch(nt, nr, getattr(oai, model), bw, n) as ch:
                x = rng.integers(-3000, 3001, size=(2, nt, spt, 2)).astype(np.int16).view(np.int32)[..., 0]
                d_tx = ch._dev(n * nt * spt * 4)
                for v in range(n):                             # two different subframes, alternating
                    ch._put(d_tx + v * nt * spt * 4, np.ascontiguousarray(x[v & 1]))
                d_tail = ch._dev(nt * spt * 4)
                ch._put(d_tail, np.ascontiguousarray(x[0]))
                d_rx = ch._dev(n * 2 * nr * spt * 4)
                d_lev = ch._dev(n * nt * 4)
                assert L.oai4g_signal_energy_batch(d_tx, n * nt, spt, spt, d_lev, None) == 0
                assert L.oai4g_sync() == 0
                step = [0]

                def draw():
                    ch.draw(seed=1, step=step[0], stream=sid)
                    step[0] += 1
                tmed, tlo, thi = timed(draw, torch, args.warmup, args.reps)
                med, lo, hi = timed(lambda: ch.run(d_tx, nt * spt, spt, spt, d_tail, spt, d_rx, 2 * nr * spt, spt, spt, nr * spt,
                                                   d_lev, 3.0, 5, stream=sid), torch, args.warmup, args.reps)
                taps = ch.channel_length
            k = 4096 / n
            length = 2 * spt
            nbytes = 4096 * (nt * spt + nr * length) * 4
            ops = 4096 * length * nr * nt * taps * 8            # lane operations: 4 multiplies and 4 adds per term
            t_bytes, t_f64 = nbytes / HBM * 1e6, ops / 64 * cyc / (simds * CLOCK) * 1e6
            out[f"{model}{N_RB}_{nt}x{nr}"] = {
                "trials_run": n, "taps": taps, "multipath_us_per_4096": round(med * k, 1), "us_min": round(lo * k, 1),
                "us_max": round(hi * k, 1), "bytes_bound_us": round(t_bytes, 1), "f64_bound_us": round(t_f64, 1),
                "of_bytes_bound": round(t_bytes / (med * k), 3), "of_f64_bound": round(t_f64 / (med * k), 3),
                "taps_us_per_4096": round(tmed * k, 1), "taps_us_min": round(tlo * k, 1), "taps_us_max": round(thi * k, 1)}
    bler = {}
    for label, model in (("awgn_batch", None), ("model_AWGN", oai.AWGN), ("Rayleigh1", oai.Rayleigh1), ("ETU", oai.ETU)):
        with DlsimBler(9, N_RB_DL=25, batch=4096, num_rounds=2, channel_model=model) as sim:
            sim.reset_rounds(3)
            sim.step(3.5)
            link = timed(lambda: sim._channel(3.5, 3, 0, 0), torch, args.warmup, args.reps)
            whole = timed(lambda: sim.step(3.5), torch, args.warmup, args.reps)
        bler[label] = {"link_us": [round(v, 1) for v in link], "step_us": [round(v, 1) for v in whole]}
    out["bler_step_mcs9_25prb_4096"] = bler
    print(json.dumps(out))
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "channel_ref.json")))["seconds"]
    lines = [
        "Fading channel on one MI355X (gfx950), tools/channel_time.py on " + oai.device_name() + ":",
        "HIP events around each launch, %d warm-up launches, median (min .. max) of %d launches, microseconds per 4096" % (args.warmup, args.reps),
        "trials of two subframes each (the 100 PRB rows ran 256 trials and are scaled by 16).",
        "",
        "Issue rate of the inner loop's operations, tools/ubench/f64_rate in the same run: cycles per wave instruction per",
        "SIMD in a dependent-free loop, at 1 / 2 / 4 / 8 waves per SIMD:",
    ] + ["  %-10s %s" % (k, "  ".join("%.2f" % rate[k][w] for w in ("1", "2", "4", "8"))) for k in ("v_mul_f64", "v_add_f64", "v_fma_f64")] + [
        "",
        "bytes bound: int16 input once + output once over 6.29 TB/s.  f64 bound: 4 v_mul_f64 + 4 v_add_f64 per tap, antenna",
        "pair and output sample at the 8-wave rates above (%.2f cycles on average) on %d SIMDs at 2.4 GHz.  No target was" % (cyc, simds),
        "set: this is the kernels' first measurement.",
        "",
        "case            taps   k_multipath us (min..max)        bytes bound  share   f64 bound  share   k_channel_taps us (min..max)",
    ]
    for N_RB, model, bw, n in CASES:
        for nt, nr in ((1, 1), (2, 2)):
            r = out[f"{model}{N_RB}_{nt}x{nr}"]
            lines.append("%3d PRB %-3s %dx%d  %4d   %10.1f (%10.1f..%10.1f)   %9.1f   %5.3f   %9.1f  %5.3f   %8.1f (%8.1f..%8.1f)" % (
                N_RB, model, nt, nr, r["taps"], r["multipath_us_per_4096"], r["us_min"], r["us_max"], r["bytes_bound_us"],
                r["of_bytes_bound"], r["f64_bound_us"], r["of_f64_bound"], r["taps_us_per_4096"], r["taps_us_min"], r["taps_us_max"]))
    lines += ["", "BLER step, MCS 9, 25 PRB, 4096 trials (DlsimBler.step, num_rounds 2): the link stage alone (tx_lev + channel + noise)",
              "and the whole step, median (min .. max) us:"]
    for label, r in bler.items():
        lines.append("  %-11s link %9.1f (%9.1f..%9.1f)   step %9.1f (%9.1f..%9.1f)" % ((label,) + tuple(r["link_us"]) + tuple(r["step_us"])))
    lines += ["", "For context, the reference's multipath_channel on one CPU core of the machine that generated",
              "tests/golden/channel_ref.json, seconds per call (one trial): " + ", ".join("%s %.4f" % kv for kv in sorted(ref.items())) + "."]
    if os.path.exists(args.resources):
        lines += ["", "Compiler's figures of the kernels (tools/kernel_resources.py, " + os.path.relpath(args.resources, ROOT) + "):"]
        lines += ["  " + ln.rstrip() for ln in open(args.resources) if "k_multipath" in ln or "k_channel_taps" in ln]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
