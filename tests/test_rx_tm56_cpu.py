"""Validation of tests/rx_tm56_model.py, the numpy restatement of rx_pdsch for the single-layer
precoding modes (TM4-6, MIMO modes 3..7, dual_stream_flag = 0) that the GPU tests compare against.
dlsch_demodulation.c cannot be compiled stand-alone (PHY_VARS_UE), so the model is checked piecewise:
hand-derived precoder vectors, the C oracle's TM2 chain for the extraction length and the channel
level, the C oracle's LLR stage, a noiseless float construction for the precoder orientation, and the
two subband rules."""
import numpy as np
import pytest

import oracle_lib as O
import rx_tm56_model as M
from test_rx_cpu import alloc, dual_alloc


# (h0, h1, p) -> h' = mulhi(sat(h0 + w_p h1), 23170) << 1, derived by hand:
#   mulhi2(g) = ((g * 23170) >> 16) << 1, >> an arithmetic shift (floor)
PREC_VECTORS = [
    # plain values, all four precoders: g = (1300, -1600), (700, -2400), h0 - t = (600, -1700), h0 + t = (1400, -2300)
    # with t = (h1.im, -h1.re) = (400, -300)
    ((1000, -2000), (300, 400), 0, (918, -1132)),       # 30121000 >> 16 = 459; -37072000 >> 16 = -566
    ((1000, -2000), (300, 400), 1, (494, -1698)),       # 16219000 >> 16 = 247; -55608000 >> 16 = -849
    ((1000, -2000), (300, 400), 2, (424, -1204)),       # 13902000 >> 16 = 212; -39389000 >> 16 = -602
    ((1000, -2000), (300, 400), 3, (988, -1628)),       # 32438000 >> 16 = 494; -53291000 >> 16 = -814
    # adds_epi16 saturates up (re) and down (im): g = (32767, -32768) -> 759211390 >> 16 = 11584; -759234560 >> 16 = -11585
    ((30000, -30000), (10000, -10000), 0, (23168, -23170)),
    # subs_epi16 saturates in both directions
    ((30000, -30000), (-10000, 10000), 1, (23168, -23170)),
    # h1.re = -32768: sign_epi16 leaves it -32768, so t = (5, -32768); h0 - t = (95, sat(200 + 32768) = 32767)
    ((100, 200), (-32768, 5), 2, (66, 23168)),          # 2201150 >> 16 = 33; a true negation would give 200 - 32768
    ((100, 200), (-32768, 5), 3, (74, -23030)),         # h0 + t = (105, -32568): 2432850 >> 16 = 37; -754600560 >> 16 = -11515
    # mulhi then << 1 is not (g * 23170) >> 15: g = 5 -> (115850 >> 16) << 1 = 2, not 3; g = 2 -> 0, not 1
    ((3, 1), (2, 1), 0, (2, 0)),
]


@pytest.mark.parametrize("h0,h1,p,want", PREC_VECTORS)
def test_precoder_vectors(h0, h1, p, want):
    r, i = M.prec_tm56(np.array([h0[0]]), np.array([h0[1]]), np.array([h1[0]]), np.array([h1[1]]), np.array([p]))
    assert (int(r[0]), int(i[0])) == want


def _random(fo, nb_rx, seed, scale):
    n = fo.symbols_per_tti * fo.ofdm_symbol_size
    rng = np.random.default_rng(seed)
    rx = [rng.integers(-scale, scale, n, dtype=np.int64).astype(np.int32) for _ in range(nb_rx)]
    est = {(p, a): rng.integers(-scale, scale, n, dtype=np.int64).astype(np.int32) for p in (0, 1) for a in range(nb_rx)}
    return rx, est


# (N_RB, subframe, RX antennas, PDCCH symbols, allocation): odd N_RB_DL in subframes 0 / 5 takes one RB
# away from the PBCH / sync RBs (the dual extraction stays defined for one full RB, test_rx_cpu.dual_alloc)
LEVEL = [(6, 0, 1, 3, None), (6, 5, 2, 2, None), (6, 7, 2, 3, None), (15, 0, 2, 1, [1 << 1, 0, 0, 0]),
         (15, 5, 1, 2, [1 << 13, 0, 0, 0]), (15, 7, 2, 1, None), (25, 0, 1, 2, [1 << 2, 0, 0, 0]),
         (25, 5, 2, 1, [1 << 22, 0, 0, 0]), (25, 7, 1, 3, None)]


@pytest.mark.parametrize("N_RB,sf,nb_rx,npd,ra", LEVEL)
def test_level_and_count_equal_the_tm2_oracle(N_RB, sf, nb_rx, npd, ra):
    """dlsch_extract_rbs_dual and dlsch_channel_level are TM2's: same LLR count, same log2_maxh with
    dl_power_off = 0, one more with dl_power_off = 1"""
    ra = ra or dual_alloc(N_RB)
    fo = O.frame(N_RB, Nid_cell=N_RB + sf, nb_antennas_tx=2, mode1_flag=0)
    for k, scale in enumerate((2 ** 31 - 1, 3000)):
        rx, est = _random(fo, nb_rx, 1000 * N_RB + 10 * sf + k, scale)
        for Qm in (2, 6):
            lo, so = O.rx_pdsch_tm2(fo, rx, est, ra, Qm, npd, sf)
            l0, s0 = M.rx_pdsch_tm56(fo, rx, est, ra, Qm, 7, 0xE4B1, 0, npd, sf)
            l1, s1 = M.rx_pdsch_tm56(fo, rx, est, ra, Qm, 3, 0xE4B1, 1, npd, sf)
            assert len(l0) == len(lo) == len(l1)
            assert s0 == so and s1 == so + 1


@pytest.mark.parametrize("Qm", [2, 4, 6])
def test_llr_stage_equals_oracle(Qm):
    N_RB, sf, npd = 25, 7, 1
    fo = O.frame(N_RB, Nid_cell=3, nb_antennas_tx=2, mode1_flag=0)
    for scale in (2 ** 31 - 1, 3000):
        rx, est = _random(fo, 2, Qm + (scale & 7), scale)
        parts = []
        llr, _ = M.rx_pdsch_tm56(fo, rx, est, dual_alloc(N_RB), Qm, 5, 0x1B4E, 1, npd, sf, parts=parts)
        cr, ci, mag, magb = (np.concatenate([p[i] for p in parts]) for i in range(4))
        comp = np.stack([cr, ci], axis=1).astype(np.int16).reshape(-1)
        want = O.orc_llr_qam(Qm, comp, mag.astype(np.int16), magb.astype(np.int16), len(cr))
        assert np.array_equal(llr, want)


LEVELS = {2: np.array([1.0]) / np.sqrt(2), 4: np.array([1.0, 3.0]) / np.sqrt(10),
          6: np.array([3.0, 1.0, 5.0, 7.0]) / np.sqrt(42)}       # index b2 (16-QAM), 2 b2 + b4 (64-QAM)


def _axis(bits):
    """one axis of the constellation point from its bits (b0[, b2[, b4]]): bit 1 = negative / outer"""
    idx = 0
    for b in bits[1:]:
        idx = 2 * idx + b
    return (1 - 2 * bits[0]) * LEVELS[2 * len(bits)][idx]


W = [1, -1, 1j, -1j]


@pytest.mark.parametrize("Qm,nb_rx", [(2, 1), (4, 2), (6, 1)])
def test_precoder_orientation(Qm, nb_rx):
    """y = round((h0 + w_p h1) x / sqrt 2) with known bits: hard decisions equal the bits under
    precoder p, and under every other precoder at least one differs."""
    N_RB, sf, npd = 6, 7, 3
    fo = O.frame(N_RB, Nid_cell=1, nb_antennas_tx=2, mode1_flag=0)
    N, nsymb = fo.ofdm_symbol_size, fo.symbols_per_tti
    ra = alloc(N_RB)
    for p in range(4):
        rng = np.random.default_rng(100 * Qm + p)
        rx = [np.zeros(nsymb * N, np.int32) for _ in range(nb_rx)]
        est = {(q, a): np.zeros(nsymb * N, np.int32) for q in (0, 1) for a in range(nb_rx)}
        bits_all = []
        for l in range(npd, nsymb):
            bins, cols, _, _, n, _ = M.extract_dual(fo, ra, sf, l)
            assert n == len(bins)
            bits = rng.integers(0, 2, (n, Qm))
            bits_all.append(bits)
            x = np.array([_axis(list(b[0::2])) + 1j * _axis(list(b[1::2])) for b in bits])
            for a in range(nb_rx):
                h = np.zeros((2, n, 2), np.int64)
                bad = np.ones(n, bool)
                while bad.any():                                   # moderate channels, no deep fade of h0 + w h1
                    h[:, bad] = rng.integers(300, 2000, (2, bad.sum(), 2)) * rng.choice([-1, 1], (2, bad.sum(), 2))
                    h0, h1 = h[0, :, 0] + 1j * h[0, :, 1], h[1, :, 0] + 1j * h[1, :, 1]
                    bad = np.abs(h0 + W[p] * h1) <= 800
                y = (h0 + W[p] * h1) * x / np.sqrt(2)
                pack = lambda re, im: ((np.asarray(re, np.int64) & 0xFFFF) | ((np.asarray(im, np.int64) & 0xFFFF) << 16)) \
                    .astype(np.uint32).view(np.int32)
                rx[a][l * N + bins] = pack(np.round(y.real), np.round(y.imag))
                est[(0, a)][l * N + 5 + cols] = pack(h[0, :, 0], h[0, :, 1])
                est[(1, a)][l * N + 5 + cols] = pack(h[1, :, 0], h[1, :, 1])
        want = np.concatenate(bits_all).reshape(-1)
        for q in range(4):
            llr, _ = M.rx_pdsch_tm56(fo, rx, est, ra, Qm, 7, q * 0x5555, 1, npd, sf)
            assert len(llr) == len(want) and (q != p or np.all(llr != 0))
            errs = int(np.sum((llr < 0).astype(np.int64) != want))
            assert (errs == 0) if q == p else (errs >= 1), (p, q, errs)


def test_subband_rules():
    """the UE's 4-RB subbands against the transmitter's get_pmi (1 / 4 / 6 / 8 RBs): equal at 25 PRB only"""
    w = 0xE4B1
    for n_rb, equal in ((6, False), (25, True), (50, False), (100, False)):
        ue = [M.pmi_of(n_rb, 7, w, prb, M.RULE_UE) for prb in range(min(n_rb, 64))]
        tx = [M.pmi_of(n_rb, 7, w, prb, M.RULE_TX) for prb in range(min(n_rb, 64))]
        assert (ue == tx) == equal, n_rb
    assert [M.pmi_of(25, 7, w, prb, M.RULE_UE) for prb in range(0, 25, 4)] == [1, 0, 3, 2, 0, 1, 2]
    # a word whose subbands are all equal reads the same under both rules
    assert all(M.pmi_of(100, 7, 0xAAAA, prb, M.RULE_UE) == M.pmi_of(100, 7, 0xAAAA, prb, M.RULE_TX) == 2
               for prb in range(32))


def test_ue_rule_shift_counts():
    """pmi is an unsigned short promoted to int: counts 16..31 (PRB 32..63) read 0; counts >= 32 are
    undefined in C and refused, except for pmi_alloc 0"""
    assert [M.pmi_of(100, 7, 0xFFFF, prb, M.RULE_UE) for prb in range(28, 36)] == [3, 3, 3, 3, 0, 0, 0, 0]
    assert all(M.pmi_of(100, 7, 0xFFFF, prb, M.RULE_UE) == 0 for prb in range(32, 64))
    assert all(M.pmi_of(50, 7, 0xFFFF, prb, M.RULE_UE) == 0 for prb in range(32, 50))
    for prb in (64, 99):
        with pytest.raises(M.Refused):
            M.pmi_of(100, 7, 0x0001, prb, M.RULE_UE)
        assert M.pmi_of(100, 7, 0, prb, M.RULE_UE) == 0


def test_mode_8_is_refused():
    fo = O.frame(6, nb_antennas_tx=2, mode1_flag=0)
    rx, est = _random(fo, 1, 1, 3000)
    with pytest.raises(M.Refused):
        M.rx_pdsch_tm56(fo, rx, est, alloc(6), 2, 8, 0, 1, 3, 7)
