"""The random part of the channel stage (k_awgn, k_multipath's noise, k_channel_taps' Philox draws) pinned sample by
sample to tests/noise_model.py, the numpy restatement that test_noise_model_cpu.py holds to Random123's known answers
and to mpmath.  Every int16 comparison is np.array_equal over all samples: tests/noise_cases.py states the guard
condition under which that is sound and test_noise_model_cpu.py asserts it for cases A and B; D asserts it here, on the
transmit samples the device made.  Taps are compared within 1e-12, the bound of test_gpu_channel.py.

  A  oai4g_awgn_batch: tile edges, the tail, the seed's two words, sigma below 1 and the (short) wrap, pad words, and the
     same vectors in two launches;
  B  oai4g_multipath_batch with the noise on: 1x1 .. 2x2, a stream per receive antenna, sigma from the summed levels,
     both store paths;
  C  oai4g_channel_random_batch from the seed: a and ch of two successive calls against the model fed tap_draws, and
     the same draws supplied, so that a failure names Philox or the ordering; the drop-in's three steps;
  D  the BLER loop hands (seed, step B, step) to the taps and the noise: what FepBatch receives equals the model."""
import numpy as np
import pytest

import channel_cases as CC
import channel_model as M
import noise_cases as NC
import noise_model as NM
from test_gpu_channel import TOL, Mem

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A


@pytest.mark.parametrize("case", NC.A_CASES, ids=NC.a_id)
def test_a_awgn_batch_equals_the_model(gpu, case):
    tx_len, tail_len, seed, off = case
    L, n, ln = gpu.lib(), NC.A_N, tx_len + tail_len
    stride = ln + NC.A_PAD
    x, tail = NC.a_input(case)
    want = np.full((n, stride), FILL, np.int32)
    want[:, :ln] = NC.words(NC.a_model(case)[0])
    m = Mem(gpu)
    try:
        d_x, d_l = m.put(NC.words(x)), m.put(NC.A_LEV)
        d_t = m.put(NC.words(tail)) if tail_len else None
        for launches in (((0, n),), NC.A_SPLIT):
            d_r = m.put(np.full((n, stride), FILL, np.int32))
            for first, count in launches:
                assert L.oai4g_awgn_batch(d_x + 4 * first * tx_len, tx_len, tx_len, d_t, tail_len, d_r + 4 * first * stride,
                                          stride, count, d_l + 4 * first, off, seed, NC.A_FIRST + first, None) == 0
            got = m.get(d_r, (n, stride), np.int32)
            bad = np.argwhere(got != want)
            assert not len(bad), (launches, len(bad), bad[:4].tolist())
    finally:
        m.close()


@pytest.mark.parametrize("case", NC.B_CASES, ids="-".join)
def test_b_multipath_batch_noise_equals_the_model(gpu, case):
    model, nt, nr, bw, off = NC.B_CONFIGS[case[0]]
    tx_len, tail_len, nseg = NC.B_LAYOUTS[case[1]]
    length, seg, seg_stride, ant_stride, rx_stride = NC.b_geometry(case)
    (taps, x, tail, lev), (w16, _) = NC.b_expected(case)
    want = np.full((NC.B_N, rx_stride), FILL, np.int32)
    i = np.arange(length)
    for a in range(nr):
        want[:, a * ant_stride + (i // seg) * seg_stride + i % seg] = NC.words(w16[:, a])
    m = Mem(gpu)
    try:
        with gpu.ChannelBatch(nt, nr, CC.MODELS[model], bw, NC.B_N, channel_offset=off) as ch:
            assert ch.channel_length == taps.shape[2]
            ch.set_taps(ch=taps)
            d_x, d_t, d_l = m.put(NC.words(x)), m.put(NC.words(tail)), m.put(lev)
            d_r = m.put(np.full((NC.B_N, rx_stride), FILL, np.int32))
            assert d_r % 16 == 0
            ch.run(d_x, nt * tx_len, tx_len, tx_len, d_t, tail_len, d_r, rx_stride, ant_stride, seg, seg_stride, d_l,
                   NC.B_OFFSET_DB, NC.SEED_BOTH, first_vector=NC.B_FIRST)
            got = m.get(d_r, (NC.B_N, rx_stride), np.int32)
    finally:
        m.close()
    bad = np.argwhere(got != want)
    assert not len(bad), (len(bad), bad[:4].tolist())


def _close(got, want):
    return float(np.abs(got - want).max())


@pytest.mark.parametrize("case", NC.C_CASES, ids=lambda c: "%s-%dx%d-ff%g" % c)
def test_c_random_batch_from_the_seed(gpu, case):
    model, nt, nr, ff = case
    desc = M.describe(model, nt, nr, NC.C_BW)
    want = [NC.c_model(desc, NC.SEED_BOTH, NC.C_FIRST + v, 2, ff) for v in range(NC.C_N)]
    with gpu.ChannelBatch(nt, nr, CC.MODELS[model], NC.C_BW, NC.C_N, forgetting_factor=ff) as ch, \
            gpu.ChannelBatch(nt, nr, CC.MODELS[model], NC.C_BW, NC.C_N, forgetting_factor=ff) as sup:
        assert ch.draws_per_vector == len(want[0][0][0])
        for step in (0, 1):
            # the model's draws supplied: the ordering and the arithmetic behind the draws
            sup.draw(draws=np.stack([want[v][step][0] for v in range(NC.C_N)]))
            a, taps = sup.taps()
            for v in range(NC.C_N):
                ea, ec = _close(a[v], want[v][step][1]), _close(taps[v], want[v][step][2])
                assert ea <= TOL and ec <= TOL, ("supplied draws", step, v, ea, ec)
            # the device's own Philox draws
            ch.draw(seed=NC.SEED_BOTH, first_vector=NC.C_FIRST, step=step)
            a, taps = ch.taps()
            for v in range(NC.C_N):
                ea, ec = _close(a[v], want[v][step][1]), _close(taps[v], want[v][step][2])
                assert ea <= TOL and ec <= TOL, ("Philox draws", step, v, ea, ec)


def test_c_random_channel_drop_in_steps(gpu):
    model, nt, nr, ff = NC.C_DROP_IN
    want = NC.c_model(M.describe(model, nt, nr, NC.C_BW), 0, 0, 3, ff)
    with gpu.ChannelBatch(nt, nr, CC.MODELS[model], NC.C_BW, 1, forgetting_factor=ff) as ch:
        for step in range(3):
            gpu.random_channel(ch)
            a, taps = ch.taps()
            ea, ec = _close(a[0], want[step][1]), _close(taps[0], want[step][2])
            assert ea <= TOL and ec <= TOL, (step, ea, ec)


@pytest.mark.parametrize("fading", [False, True], ids=["awgn", "rayleigh1"])
def test_d_loop_hands_each_step_its_own_streams(gpu, fading):
    """two steps of the round loop: the samples FepBatch receives equal the model built from the transmit samples, the
    common tail, tx_lev and (under fading) the taps read back, with (seed, first_vector = step B, step); the guard
    condition of noise_cases.py is asserted on these samples, none left out"""
    from openair4g_amd.dlsim import CHANNEL_BW, DlsimBler
    B, seed = NC.D_BATCH, NC.D_SEED
    sim = DlsimBler(mcs=NC.D_MCS, N_RB_DL=NC.D_N_RB, batch=B, num_rounds=NC.D_ROUNDS,
                    channel_model=gpu.Rayleigh1 if fading else None)
    m = Mem(gpu)
    try:
        spt, off = sim.spt, sim.sigma_offset(NC.D_SNR)
        desc = M.describe("Rayleigh1", 1, 1, CHANNEL_BW[NC.D_N_RB])
        tail = NC.unwords(sim.tail)
        a_prev, residual = [None] * B, []
        sim.reset_rounds(seed)
        for step in range(NC.D_STEPS):
            sim.step(NC.D_SNR)
            rounds = sim.round_state()[0]                   # synchronises
            if step == 0:
                assert rounds.any(), "no slot retransmits in step 1"
            iq, lev = NC.unwords(sim.tx.iq()[:, 0]), sim.tx_lev()
            got = NC.unwords(m.get(sim.fep.d_rx, (B, 2 * spt), np.int32))
            ch = sim.chan.taps()[1] if fading else None
            res = []
            for v in range(B):
                vec, sig = step * B + v, np.concatenate([iq[v], tail])
                if fading:
                    a_prev[v], want_ch = M.random_channel(desc, a_prev[v], NM.tap_draws(desc, seed, vec, step), 0.0, step == 0)
                    assert _close(ch[v], want_ch) <= TOL, (step, v)
                    sig = M.multipath(ch[v], sig.astype(np.float64)[None], 1)[0]
                want, dist = NM.awgn_d(sig, lev[v], off, seed, vec)
                print("step %d vector %d: sigma %.1f, closest approach to an integer %.3g" %
                      (step, v, float(NM.sigma(lev[v], off)), dist.min()))
                assert dist.min() > NC.GUARD, (step, v, np.argwhere(dist <= NC.GUARD).tolist())
                bad = np.argwhere(got[v] != want)
                assert not len(bad), (step, v, len(bad), bad[:4].tolist())
                res.append(got[v].astype(np.int64) - np.rint(sig).astype(np.int64))
            residual.append(res)
        for v in range(B):                                    # step 1 saw noise of its own, not step 0's again
            assert np.mean(np.any(residual[0][v] != residual[1][v], axis=-1)) > 0.99, v
    finally:
        m.close()
        sim.close()
