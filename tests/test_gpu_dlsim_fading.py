"""GPU suite: dlsim's BLER loop under a fading channel (DlsimBler(channel_model=...), G7).

With a flat tap h_t, trial t sees the AWGN link at SNR + 10 log10 |h_t|^2.  The reference's AWGN table for the MCS
(tests/golden/bler_awgn_tx1_nrx1.json) gives s_hi, the lowest row with BLER <= 0.01 plus 1 dB, and s_lo, the highest
row with BLER >= 0.99 minus 1 dB; the 1 dB covers the 0.3 dB between the reference's two curve sets and the 0.1 dB the
GPU chain is known to keep.  At mean SNR s_hi + 3 dB, trials with instantaneous SNR >= s_hi must decode and trials
<= s_lo must fail, at most 1 % of each class doing otherwise, each class holding at least 200 of the 4096 trials
(P(|h|^2 > 0.5) is 0.61 there, the low class about 0.2)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MCS = 9


def thresholds(mcs):
    rows = json.load(open(os.path.join(HERE, "golden", "bler_awgn_tx1_nrx1.json")))["curves"][str(mcs)]["rows"]
    s_hi = min(r[0] for r in rows if r[1] / r[2] <= 0.01) + 1.0
    s_lo = max(r[0] for r in rows if r[1] / r[2] >= 0.99) - 1.0
    assert s_lo < s_hi
    return s_hi, s_lo


def test_g7_rayleigh_trials_follow_their_instantaneous_snr(gpu):
    from openair4g_amd.dlsim import DlsimBler
    s_hi, s_lo = thresholds(MCS)
    snr = s_hi + 3.0
    with DlsimBler(mcs=MCS, N_RB_DL=25, batch=4096, channel_model=gpu.Rayleigh1) as sim:
        err, gain = sim.run_batch(snr, seed=20261022, want_gain=True)
        a, ch = sim.chan.taps()
    assert np.array_equal(gain, np.abs(ch[:, 0, 0]) ** 2) and np.array_equal(a[:, 0, 0], ch[:, 0, 0])
    inst = snr + 10 * np.log10(gain)
    hi, lo = inst >= s_hi, inst <= s_lo
    bad_hi, bad_lo = int(err[hi].sum()), int((~err[lo]).sum())
    print(f"s_hi {s_hi} s_lo {s_lo} mean gain {gain.mean():.4f}: high class {hi.sum()} trials, {bad_hi} failed; "
          f"low class {lo.sum()} trials, {bad_lo} decoded; in between {(~hi & ~lo).sum()}, BLER {err.mean():.4f}")
    assert hi.sum() >= 200 and lo.sum() >= 200
    assert bad_hi <= 0.01 * hi.sum() and bad_lo <= 0.01 * lo.sum()


def test_g7_awgn_model_equals_the_awgn_path(gpu):
    """channel_model = None runs oai4g_awgn_batch as before; model AWGN runs the general kernel: the same error flags
    for the same seed, in a batch and along the round loop's counters"""
    from openair4g_amd.dlsim import DlsimBler
    with DlsimBler(mcs=MCS, N_RB_DL=25, batch=512) as old, \
            DlsimBler(mcs=MCS, N_RB_DL=25, batch=512, channel_model=gpu.AWGN) as new:
        assert old.chan is None and new.chan is not None
        e0, e1 = old.run_batch(3.4, seed=7, first_trial=512), new.run_batch(3.4, seed=7, first_trial=512)
        assert 0 < e0.sum() < 512 and np.array_equal(e0, e1)
        assert np.all(new.channel_gain() == 1.0)
    with DlsimBler(mcs=MCS, N_RB_DL=25, batch=256, num_rounds=2) as old, \
            DlsimBler(mcs=MCS, N_RB_DL=25, batch=256, num_rounds=2, channel_model=gpu.AWGN) as new:
        r0, r1 = old.run_steps(2.4, 3, seed=5), new.run_steps(2.4, 3, seed=5)
        assert r0 == r1 and r0["round_trials"][1] > 0
