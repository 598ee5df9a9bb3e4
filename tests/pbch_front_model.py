"""numpy restatement of the PBCH receive front end: rx_pbch up to the quantised soft bits
(PHY/LTE_TRANSPORT/pbch.c:434-758, 816-973, normal prefix), rx_pbch whole, and pbch_detection's order
(initial_sync.c:135-161).

  1. symbols l = 7..10 of subframe 0 (symbol_mod 0..3), each on its own, with its own level and shift;
  2. pbch_extract: 72 subcarriers; receive words N - 36 + k (k < 36) and 1 + k - 36 (DC skipped), estimate
     words 5 + 6 N_RB - 36 + k, contiguous (no DC skip), from row l when high_speed_flag == 1, else row 0;
     symbol_mod 0 / 1 drop nushift % 3 + {0, 3, 6, 9} of every 12 and pack 8 per RB (also with one port): 48
     words at symbol_mod * 72, words 48..71 never written: 0, as the reference's cleared buffers;
  3. pbch_channel_level: per plane (aatx << 1) + aarx, aatx 0..3 always (planes never estimated are 0), the
     32-bit wrapping sum of |h|^2 over the region's 72 words, divided as a signed int by 72, the maximum from
     0 on; log2_maxh = 3 + log2_approx(max) / 2;
  4. pbch_channel_compensation, pbch_detection_mrc: as the PDCCH front's;
  5. pbch_alamouti on planes 0 and 2 over all 72 words (int16 sums that wrap); SISO is the identity; ALAMOUTI
     with one estimated port is not refused: plane 2 is 0 and the result equals SISO;
  6. pbch_quantize: clamp to [-8, 7], re before im; 96 + 96 + 144 + 144 soft bits at llr[frame_mod4 * 480] of a
     1920-byte buffer that is 0 elsewhere;
  7. pbch_detection: frame_mod4 0..3, for each SISO then ALAMOUTI; the first result in 1..2 wins.
"""
import numpy as np

import ctrl_rx_model as M
from pdcch_front_model import ALAMOUTI, SISO, _c16, _wrap32, alamouti, compensate, log2_approx, mrc

SOFT = (96, 96, 144, 144)


def extract_map(N_RB, N, nushift, symbol_mod):
    """(receive word within row 7 + symbol_mod, estimate word within its row) of every extracted RE, in the order of
    rxdataF_ext: 48 entries on symbol_mod 0 / 1, else 72"""
    k = np.arange(72)
    if symbol_mod < 2:
        k = k[(k % 12) % 3 != nushift % 3]
    return np.where(k < 36, N - 36 + k, 1 + k - 36), 5 + 6 * N_RB - 36 + k


def channel_level(h72):
    """the signed average pbch_channel_level forms of one plane's region (zeros where nothing was written)"""
    h = _c16(h72)
    total = int(_wrap32(int((h[:, 0] ** 2 + h[:, 1] ** 2).sum()) % 2 ** 32))
    q = abs(total) // 72                                 # C division truncates toward zero
    return q if total >= 0 else -q


def rx_pbch_front(fp, rxdataF, est, nb_ports, mimo_mode, high_speed_flag=1):
    """fp: anything with N_RB_DL, ofdm_symbol_size, nushift.  rxdataF[a], est[(p, a)] (p < nb_ports): int32 rows
    [nsymb * N] of subframe 0.  Returns a dict: comp (plane 0, 288 words), log2_maxh [4], llr (480 int8), planes
    ((p, a) -> compensated plane before MRC), defined (bool per word), avg [4] ((p, a) -> level), unwrapped
    (the largest |exact Alamouti sum|, 0 under SISO)."""
    N_RB, N, nb_rx = fp.N_RB_DL, fp.ofdm_symbol_size, len(rxdataF)
    defined = np.ones(288, dtype=bool)
    planes = {(p, a): np.zeros(288, dtype=np.int32) for p in range(nb_ports) for a in range(nb_rx)}
    shifts, avgs = [], []
    for sm in range(4):
        l = 7 + sm
        rxw, chw = extract_map(N_RB, N, fp.nushift, sm)
        n = len(rxw)
        defined[sm * 72 + n:(sm + 1) * 72] = False
        row = l if high_speed_flag == 1 else 0
        ext_h = {}
        for pa in planes:
            h = np.zeros(72, dtype=np.int32)
            h[:n] = np.asarray(est[pa], np.int32)[row * N + chw]
            ext_h[pa] = h
        avg = {pa: channel_level(h) for pa, h in ext_h.items()}
        shift = 3 + log2_approx(max([0] + list(avg.values()))) // 2
        shifts.append(shift)
        avgs.append(avg)
        for (p, a) in planes:
            y = np.asarray(rxdataF[a], np.int32)[l * N + rxw]
            planes[(p, a)][sm * 72:sm * 72 + n] = compensate(ext_h[(p, a)][:n], y, shift)
    zero = np.zeros(288, dtype=np.int32)
    comb = []
    for p in range(2):
        if p >= nb_ports:
            comb.append(zero)
        elif nb_rx > 1:
            comb.append(mrc(planes[(p, 0)], planes[(p, 1)]))
        else:
            comb.append(planes[(p, 0)].copy())
    unwrapped = 0
    if mimo_mode == ALAMOUTI:
        comp = alamouti(comb[0], comb[1])
        a, b = _c16(comb[0]).reshape(-1, 2, 2), _c16(comb[1]).reshape(-1, 2, 2)
        unwrapped = int(max(np.abs(a[:, 0, 0] + b[:, 1, 0]).max(), np.abs(a[:, 0, 1] - b[:, 1, 1]).max(),
                            np.abs(a[:, 1, 0] - b[:, 0, 0]).max(), np.abs(a[:, 1, 1] + b[:, 0, 1]).max()))
    else:
        comp = comb[0].copy()
    assert not comp[~defined].any()
    c16 = comp.view(np.int16)
    llr = np.concatenate([np.clip(c16[sm * 144:sm * 144 + SOFT[sm]], -8, 7) for sm in range(4)]).astype(np.int8)
    return dict(comp=comp, log2_maxh=shifts, llr=llr, planes=planes, defined=defined, avg=avgs, comb=comb,
                unwrapped=unwrapped)


def llr_buffer(llr480, frame_mod4):
    buf = np.zeros(1920, dtype=np.int8)
    buf[frame_mod4 * 480:(frame_mod4 + 1) * 480] = llr480
    return buf


def rx_pbch(fp, rxdataF, est, nb_ports, mimo_mode, frame_mod4, high_speed_flag=1):
    """(1 / 2 / 4 or -1, the three MIB bytes)"""
    f = rx_pbch_front(fp, rxdataF, est, nb_ports, mimo_mode, high_speed_flag)
    return M.pbch_decode(llr_buffer(f["llr"], frame_mod4), fp.Nid_cell, frame_mod4)


def detect_rows(rows, Nid_cell):
    """pbch_detection's order over the soft bits of both modes, rows[mode] = 480 int8: (tx_ant, frame_mod4,
    mimo_mode, MIB) of the first hit in 1..2, or None"""
    for q in range(4):
        for mode in (SISO, ALAMOUTI):
            n, mib = M.pbch_decode(llr_buffer(rows[mode], q), Nid_cell, q)
            if n in (1, 2):
                return n, q, mode, mib
    return None


def pbch_detection(fp, rxdataF, est, nb_ports, high_speed_flag=1):
    rows = [rx_pbch_front(fp, rxdataF, est, nb_ports, mode, high_speed_flag)["llr"] for mode in (SISO, ALAMOUTI)]
    return detect_rows(rows, fp.Nid_cell)


def decode_480(llr480, Nid_cell, frame_mod4):
    """the decode over the quarter's 480 soft bits alone, with the Gold words 15 frame_mod4 .. of the cell"""
    g = M.gold_words(Nid_cell, 60)[15 * frame_mod4:15 * frame_mod4 + 15]
    e = np.asarray(llr480, dtype=np.int8).astype(np.int16)
    bits = np.array([(g[i >> 5] >> (i & 31)) & 1 for i in range(480)])
    e = np.where(bits == 0, -e, e).astype(np.int8)                  # -(-128) stays -128
    d = M.cc_rx_d(40, 480, e)
    a, _, _ = M.viterbi(d, 40)
    crc = M.crc16(a, 24) ^ ((int(a[3]) << 8) + int(a[4]))
    return {0x0000: 1, 0xFFFF: 2, 0x5555: 4}.get(crc, -1), bytes(int(x) for x in a[2::-1])
