"""Seeded inputs of the PSS timing fixture (tests/golden/sync_time_ref.json, written by
tests/golden/gen_sync_time_ref.py from the reference's own lte_sync_time.c) — shared by the generator, the CPU model
test and the GPU tests, so all of them correlate the same samples.

A case is (name, N_RB_DL, rx int32 [frames][nb_rx][10 samples_per_tti], info).  The transmitted frames are the
oracle's: ten subframes of CRS, PSS + SSS in subframes 0 and 5, PBCH in subframe 0, through its IDFT and prefix."""
import ctypes
import hashlib

import numpy as np

import oracle_lib as O

SEED = 20261021
AMP = 1024
PDU = (0xA4, 0x3C, 0x10)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def tx_frame(N_RB, Nid, nb_tx=1, frame_mod4=0, amp=AMP, pdu=PDU):
    """int32 [nb_tx][10 samples_per_tti]: the oracle's time-domain frame of cell Nid"""
    fp = O.frame(N_RB, Nid, 0, nb_tx, 1 if nb_tx == 1 else 0)
    N, nsymb = fp.ofdm_symbol_size, fp.symbols_per_tti
    crs = O.generate_pilots(fp, amp, 10)
    grids = [np.zeros(10 * nsymb * N + N, dtype=np.int32) for _ in range(nb_tx)]
    for a in range(nb_tx):
        grids[a][:10 * nsymb * N] = crs[a]
    nsl = nsymb // 2
    for sf in (0, 5):
        assert O.generate_pss(grids, amp, fp, nsl - 1, 2 * sf) == 0
        assert O.generate_sss(grids, amp, fp, nsl - 2, 2 * sf) == 0
    state = O.OrcPbch()
    scratch = [np.zeros_like(g) for g in grids]
    assert O.generate_pbch(state, scratch, amp, fp, np.array(pdu, np.uint8), 0) == 0       # frame_mod4 0 encodes
    assert O.generate_pbch(state, grids, amp, fp, np.array(pdu, np.uint8), frame_mod4) == 0
    out = np.zeros((nb_tx, 10 * fp.samples_per_tti), dtype=np.int32)
    for a in range(nb_tx):
        for sf in range(10):
            sub = np.ascontiguousarray(grids[a][sf * nsymb * N:(sf + 1) * nsymb * N])
            txd = np.zeros(fp.samples_per_tti, dtype=np.int32)
            O.orc().orc_normal_prefix_mod(O.P(sub), O.P(txd), nsymb, ctypes.byref(fp))
            out[a, sf * fp.samples_per_tti:(sf + 1) * fp.samples_per_tti] = txd
    return out


def _c16(v):
    """int64 [..., 2] -> packed int32"""
    return np.ascontiguousarray(np.clip(v, -32768, 32767).astype(np.int16)).view(np.int32)[..., 0]


def received(tx, delay, nb_rx, sigma, rng):
    """the frame circularly delayed by `delay` samples on nb_rx antennas: one port through gains 1 and -1/2, two
    ports through H = [1 1] / [1 -1]; Gaussian noise of deviation sigma per component.  int32 [nb_rx][frame]"""
    t = np.roll(tx.view(np.int16).reshape(len(tx), -1, 2).astype(np.int64), delay, axis=1)
    out = []
    for a in range(nb_rx):
        if len(tx) == 2:
            s = t[0] + (t[1] if a == 0 else -t[1])
        else:
            s = t[0] if a == 0 else -(t[0] >> 1)
        out.append(_c16(s + np.rint(rng.normal(0.0, sigma, s.shape)).astype(np.int64)))
    return np.stack(out)


def pss_position(N_RB, delay):
    """where the delayed frame's first PSS body starts (the last symbol of slot 0), modulo the half frame"""
    fp = O.frame(N_RB, 0)
    return (delay + fp.samples_per_tti // 2 - fp.ofdm_symbol_size) % (5 * fp.samples_per_tti)


def _burst(N_RB, Nid2):
    """the PSS body alone: N samples int16 [N][2]"""
    fp = O.frame(N_RB, Nid2)
    p = fp.samples_per_tti // 2 - fp.ofdm_symbol_size
    grid = [np.zeros(10 * fp.symbols_per_tti * fp.ofdm_symbol_size + fp.ofdm_symbol_size, dtype=np.int32)]
    assert O.generate_pss(grid, 4 * AMP, fp, fp.symbols_per_tti // 2 - 1, 0) == 0
    sub = np.ascontiguousarray(grid[0][:fp.symbols_per_tti * fp.ofdm_symbol_size])
    txd = np.zeros(fp.samples_per_tti, dtype=np.int32)
    O.orc().orc_normal_prefix_mod(O.P(sub), O.P(txd), fp.symbols_per_tti, ctypes.byref(fp))
    return txd[p:p + fp.ofdm_symbol_size].view(np.int16).reshape(-1, 2).copy()


# the planted positions of the deterministic 6 PRB cases (length = 9600, N = 128)
TWICE = (1000, 5000)
LATE = 9600 - 128 + 32
FULL = {"neg": 2000, "pos": 4000, "min": 7000}


def full_scale_frame(rep0):
    """Two antennas of zeros with three planted patterns against replica 0 (int16 [128][2]):
      at FULL["neg"], antenna 0 holds g x0 (-1 - j) at full scale, antenna 1 nothing: conj(x0) y sums far below
        -2^15 in both components, so the dot product saturates to (-32768, -32768), the antenna sum keeps it and
        abs32 is 2^31;
      at FULL["pos"], both antennas hold g x0 (1 + j): each saturates to (32767, 32767) and the int16 sum wraps to -2;
      at FULL["min"], antenna 0 holds the sample (-32768, 0), whose real part's int16 negation stays -32768, and a
        second sample behind it, without which the sign of that one term would not show in re^2 + im^2."""
    x = rep0.astype(np.int64)
    z = np.stack([x[:, 0] - x[:, 1], x[:, 0] + x[:, 1]], axis=1)          # x0 (1 + j)
    g = 32767.0 / np.abs(z).max()
    pat = np.floor(z * g).astype(np.int64)
    rx = np.zeros((2, 19200, 2), dtype=np.int64)
    rx[0, FULL["neg"]:FULL["neg"] + 128] = -pat
    rx[0, FULL["pos"]:FULL["pos"] + 128] = pat
    rx[1, FULL["pos"]:FULL["pos"] + 128] = pat
    rx[0, FULL["min"]] = (-32768, 0)
    rx[0, FULL["min"] + 1] = (20000, 20000)
    return _c16(rx)


TX6 = [(150, 1236), (301, 10400), (5, 18001)]              # (Nid_cell, delay) for Nid2 = 0, 1, 2
BATCH6 = [(27, 0), (442, 7777), (91, 12344)]
TX25 = (214, 40004)
TX100 = (77, 123456)
NAMES = ["noise6", "tx6_0", "tx6_1", "tx6_2", "zero6", "twice6", "late6", "full6", "batch6", "tx25", "tx100"]


def _planted(positions):
    b = _burst(6, 1).astype(np.int64)
    rx = np.zeros((1, 19200, 2), dtype=np.int64)
    for p in positions:
        rx[0, p:p + 128] = b
    return _c16(rx)[None]


def case(name):
    """(N_RB_DL, rx int32 [frames][nb_rx][frame]) of one case; each has its own seed"""
    import sync_rx_model as M
    rng = np.random.default_rng([SEED, NAMES.index(name)])
    if name == "noise6":
        return 6, received(np.zeros((1, 19200), np.int32), 0, 1, 300.0, rng)[None]
    if name.startswith("tx6_"):
        nid, delay = TX6[int(name[-1])]
        assert nid % 3 == int(name[-1])
        return 6, received(tx_frame(6, nid), delay, 2, 60.0, rng)[None]
    if name == "zero6":
        return 6, np.zeros((1, 1, 19200), np.int32)
    if name == "twice6":
        return 6, _planted(TWICE)
    if name == "late6":
        return 6, _planted([LATE])
    if name == "full6":
        return 6, full_scale_frame(M.replicas(6)[0])[None]
    if name == "batch6":
        return 6, np.stack([received(tx_frame(6, nid, 2, fm4), d, 2, 40.0, rng) for fm4, (nid, d) in enumerate(BATCH6)])
    if name == "tx25":
        return 25, received(tx_frame(25, TX25[0], 2, 3), TX25[1], 2, 50.0, rng)[None]
    if name == "tx100":
        return 100, received(tx_frame(100, TX100[0]), TX100[1], 1, 50.0, rng)[None]
    raise KeyError(name)
