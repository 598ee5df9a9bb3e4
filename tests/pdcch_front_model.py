"""numpy restatement of the PDCCH / PCFICH receive front end: rx_pdcch up to the compensated symbols
(PHY/LTE_TRANSPORT/dci.c:1689-1830, is_secondary_ue = 0, MU_RECEIVER off) and rx_pcfich (pcfich.c:231).

  1. three control symbols always (dci.c:1704); rx_pcfich runs afterwards on the result;
  2. symbol 0 is packed: the four REs nushift % 3 + {0, 3, 6, 9} of every RB are dropped (also with one TX port)
     and 8 REs per RB stand at the symbol's start; symbols 1 / 2 hold 12 per RB at 12 N_RB_DL; words
     8 N_RB_DL .. 12 N_RB_DL - 1 of symbol 0 are never defined: 0 here, compared nowhere;
  3. odd N_RB_DL: the middle RB takes six REs from the top of the spectrum and six from word 1 on; even sizes
     restart at word 1 with the second half.  pdcch_extract_rbs_dual reads the second six of the middle RB of
     symbols 1 / 2 from word 7 on (dci.c:1275, `rxF[(1 + i)]` where the single twin has `rxF[(1 + i - 6)]`),
     and goes on from word 7 as well: words 7..12 serve twice.  Kept;
  4. high_speed_flag 1 reads the estimate row of each symbol, 0 row 0 for all; estimates at word 5 + 12 rb + i;
  5. the level is the 32-bit wrapping sum of |h|^2 over symbol 1 (the four epi32 lanes and their sum commute
     under wrap), divided by 12 N_RB_DL as a signed integer;
  6. avg[(aatx << 1) + aarx] is written, avgP[(aarx << 1) + aatx] read, never-written entries 0;
     log2_maxh = log2_approx(avgs) / 2 + 6 + nb_antennas_rx - 1;
  7. compensation: conj(h) y from 32-bit products, >> log2_maxh arithmetically, packs_epi32;
  8. MRC: adds_epi16(x0 >> 1, x1 >> 1) -- the two halves lie in [-16384, 16383], so this adds never
     saturates: its extremes are -32768 and 32766;
  9. pdcch_alamouti on planes 0 and 2, pairs of packed words, int16 sums that wrap; pdcch_siso is the identity;
 10. rx_pcfich: 16 REs of plane 0 at pcfich_reg * 4, re before im, unscrambled, three correlations, the
     first strictly larger metric from -16384 on, 3 when none exceeds it.
"""
import numpy as np

import ctrl_rx_model as M

SISO, ALAMOUTI = 0, 1
PCFICH_B = np.array([[0 if j % 3 == i else 1 for j in range(32)] for i in range(3)])


def log2_approx(x):
    """PHY/TOOLS/log2_approx.c: the highest set bit among bits 0..30, plus one"""
    x &= 0x7FFFFFFF
    return x.bit_length()


def extract_map(N_RB, N, fco, nushift, symbol, dual):
    """(rx word within the symbol, estimate word within the row) of every extracted RE of `symbol`, in the
    order of rxdataF_ext: 8 N_RB entries for symbol 0, 12 N_RB otherwise.  Closed form."""
    NRE = 12 * N_RB
    k = np.arange(NRE)
    if symbol == 0:
        k = k[(k % 12) % 3 != nushift % 3]
    rx = np.where(k < NRE // 2, fco + k, 1 + k - NRE // 2)
    if dual and (N_RB & 1) and symbol > 0:
        mid = (k >= NRE // 2) & (k < NRE // 2 + 6)
        rx = np.where(mid, rx + 6, rx)
    return rx, 5 + k


def pcfich_regs(N_RB, Nid_cell):
    """generate_pcfich_reg_mapping (pcfich.c:48-79), units of 6 REs"""
    kbar = 6 * (Nid_cell % (2 * N_RB))
    return [kbar // 6] + [((kbar + s * 6) % (N_RB * 12)) // 6 for s in (N_RB >> 1, N_RB, (3 * N_RB) >> 1)]


def _c16(v):
    return np.asarray(v, dtype=np.int32).reshape(-1).view(np.int16).astype(np.int64).reshape(-1, 2)


def _pack(re, im):
    out = np.empty((len(re), 2), dtype=np.int16)
    out[:, 0], out[:, 1] = re, im
    return out.reshape(-1).view(np.int32).copy()


def _wrap32(v):
    return ((np.asarray(v, dtype=np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _wrap16(v):
    return ((np.asarray(v, dtype=np.int64) + 2 ** 15) % 2 ** 16) - 2 ** 15


def channel_level(h_sym1, N_RB):
    """pdcch_channel_level of one plane: h_sym1 = the 12 N_RB extracted estimates of symbol 1"""
    h = _c16(h_sym1)
    total = int(_wrap32(int((h[:, 0] ** 2 + h[:, 1] ** 2).sum()) % 2 ** 32))
    q = abs(total) // (12 * N_RB)                        # C division truncates toward zero
    return q if total >= 0 else -q


def avgs_of(avg, nb_tx, nb_rx):
    """rx_pdcch's maximum (dci.c:1751-1755): avg is keyed (port, antenna); the read is transposed"""
    written = {(p << 1) + a: v for (p, a), v in avg.items()}
    avgs = 0
    for aatx in range(nb_tx):
        for aarx in range(nb_rx):
            avgs = max(avgs, written.get((aarx << 1) + aatx, 0))
    return avgs


def compensate(h, y, shift):
    """pdcch_channel_compensation on words: packs((conj(h) y) >> shift)"""
    h, y = _c16(h), _c16(y)
    nhi = _wrap16(-h[:, 1])                              # sign_epi16: -(-32768) stays -32768
    re = _wrap32(h[:, 0] * y[:, 0] + h[:, 1] * y[:, 1]) >> shift
    im = _wrap32(nhi * y[:, 0] + h[:, 0] * y[:, 1]) >> shift
    return _pack(np.clip(re, -32768, 32767), np.clip(im, -32768, 32767))


def mrc(x0, x1):
    a, b = _c16(x0), _c16(x1)
    s = np.clip((a >> 1) + (b >> 1), -32768, 32767)
    return _pack(s[:, 0], s[:, 1])


def alamouti(p0, p2):
    """pdcch_alamouti over pairs of words of planes 0 and 2 -> plane 0 (int16 wrap)"""
    a, b = _c16(p0).reshape(-1, 2, 2), _c16(p2).reshape(-1, 2, 2)
    out = np.empty_like(a)
    out[:, 0, 0] = a[:, 0, 0] + b[:, 1, 0]
    out[:, 0, 1] = a[:, 0, 1] - b[:, 1, 1]
    out[:, 1, 0] = a[:, 1, 0] - b[:, 0, 0]
    out[:, 1, 1] = a[:, 1, 1] + b[:, 0, 1]
    out = _wrap16(out).reshape(-1, 2)
    return _pack(out[:, 0], out[:, 1])


def pcfich_metrics(comp, N_RB, Nid_cell, subframe):
    """the three correlations of rx_pcfich on plane 0"""
    words = np.concatenate([np.asarray(comp, dtype=np.int32)[4 * r:4 * r + 4] for r in pcfich_regs(N_RB, Nid_cell)])
    d = words.view(np.int16).astype(np.int64)
    s = M.gold_words((((2 * Nid_cell + 1) * (1 + subframe)) << 9) + Nid_cell, 1)[0]
    bits = np.array([(s >> j) & 1 for j in range(32)])
    d = np.where(bits == 1, _wrap16(-d), d)
    return [int(np.where(PCFICH_B[i] == 0, d, -d).sum()) for i in range(3)]


def pcfich_plane_below(N_RB, Nid_cell, subframe, amp=20000):
    """a plane 0 that rx_pcfich sees, after its unscrambling, as the constant +amp: every codeword has more ones
    than zeros, so all three metrics are negative multiples of amp (a constant plane as it stands does the same
    wherever the subframe's Gold word happens to leave it so)"""
    comp = np.zeros(36 * N_RB, dtype=np.int32)
    s = M.gold_words((((2 * Nid_cell + 1) * (1 + subframe)) << 9) + Nid_cell, 1)[0]
    c16 = comp.view(np.int16)
    c16[:] = amp
    for q, r in enumerate(pcfich_regs(N_RB, Nid_cell)):
        for i in range(8):
            if (s >> (8 * q + i)) & 1:
                c16[8 * r + i] = -amp
    return comp


def pcfich_plane_of(d, N_RB, Nid_cell, subframe, fill=0):
    """a plane 0 whose 32 PCFICH components are d[0..31] after rx_pcfich's unscrambling (no component -32768)"""
    comp = np.zeros(36 * N_RB, dtype=np.int32)
    s = M.gold_words((((2 * Nid_cell + 1) * (1 + subframe)) << 9) + Nid_cell, 1)[0]
    c16 = comp.view(np.int16)
    c16[:] = fill
    for q, r in enumerate(pcfich_regs(N_RB, Nid_cell)):
        for i in range(8):
            j = 8 * q + i
            c16[8 * r + i] = -d[j] if (s >> j) & 1 else d[j]
    return comp


PCFICH_SEED = 20240611


def pcfich_cases():
    """(name, N_RB, Nid_cell, subframe, plane 0) of tests/golden/pcfich_rx_ref.json: random planes whose metrics
    fall on both sides of the start value -16384, the all-below plane, ties between the largest metrics (the
    strictly-greater rule keeps the first), a metric of exactly -16384 and of -16383, and components of -32768
    (their int16 negation stays -32768)."""
    rng = np.random.default_rng(PCFICH_SEED)
    out = []
    for N_RB, Nid in ((6, 0), (15, 37), (25, 137), (50, 301), (100, 503)):
        for sf in (0, 3, 9):
            for amp in (700, 3000, 32767):
                for k in range(3):
                    pl = rng.integers(-amp, amp + 1, 72 * N_RB).astype(np.int16).view(np.int32)
                    out.append((f"rand_{N_RB}_{Nid}_{sf}_{amp}_{k}", N_RB, Nid, sf, pl))
            out.append((f"below_{N_RB}_{Nid}_{sf}", N_RB, Nid, sf, pcfich_plane_below(N_RB, Nid, sf)))
            z = lambda: [0] * 32
            d = z()
            for j in range(2, 32, 3):
                d[j] = -1000                                     # metrics +S, +S, -S: the first of the two wins
            out.append((f"tie01_{N_RB}_{Nid}_{sf}", N_RB, Nid, sf, pcfich_plane_of(d, N_RB, Nid, sf, 77)))
            d = z()
            for j in range(0, 32, 3):
                d[j] = -1000                                     # metrics -S, +S, +S
            out.append((f"tie12_{N_RB}_{Nid}_{sf}", N_RB, Nid, sf, pcfich_plane_of(d, N_RB, Nid, sf, -5)))
            for top in (-16384, -16383):                         # every metric equal to `top`: 3, or 1
                d = z()
                d[0] = d[1] = d[2] = -top                        # metric i = d[i] - d[i'] - d[i''] = top
                out.append((f"edge{-top}_{N_RB}_{Nid}_{sf}", N_RB, Nid, sf, pcfich_plane_of(d, N_RB, Nid, sf)))
            pl = np.zeros(36 * N_RB, dtype=np.int32)
            pl.view(np.int16)[:] = -32768
            out.append((f"min_{N_RB}_{Nid}_{sf}", N_RB, Nid, sf, pl))
    return out


def rx_pcfich(comp, N_RB, Nid_cell, subframe):
    n, old = 3, -16384
    for i, m in enumerate(pcfich_metrics(comp, N_RB, Nid_cell, subframe)):
        if m > old:
            n, old = 1 + i, m
    return n


def rx_pdcch_front(fp, rxdataF, est, subframe, mimo_mode, high_speed_flag=1):
    """fp: anything with N_RB_DL, ofdm_symbol_size, first_carrier_offset, nushift, Nid_cell, nb_antennas_tx_eNB.
    rxdataF[a], est[(p, a)]: int32 rows [nsymb * N].  Returns a dict: comp (plane 0, 36 N_RB words), log2_maxh,
    cfi, planes ((p, a) -> compensated plane before MRC), defined (bool per word of comp), avg."""
    N_RB, N, nb_tx, nb_rx = fp.N_RB_DL, fp.ofdm_symbol_size, fp.nb_antennas_tx_eNB, len(rxdataF)
    NRE = 12 * N_RB
    dual = nb_tx > 1
    maps = [extract_map(N_RB, N, fp.first_carrier_offset, fp.nushift, s, dual) for s in range(3)]
    row = (lambda s: s) if high_speed_flag == 1 else (lambda s: 0)
    ext_y = {a: [np.asarray(rxdataF[a], np.int32)[s * N + maps[s][0]] for s in range(3)] for a in range(nb_rx)}
    ext_h = {(p, a): [np.asarray(est[(p, a)], np.int32)[row(s) * N + maps[s][1]] for s in range(3)]
             for p in range(nb_tx) for a in range(nb_rx)}
    avg = {pa: channel_level(ext_h[pa][1], N_RB) for pa in ext_h}
    shift = log2_approx(avgs_of(avg, nb_tx, nb_rx)) // 2 + 6 + nb_rx - 1
    defined = np.ones(3 * NRE, dtype=bool)
    defined[8 * N_RB:NRE] = False
    planes = {}
    for pa in ext_h:
        pl = np.zeros(3 * NRE, dtype=np.int32)
        for s in range(3):
            c = compensate(ext_h[pa][s], ext_y[pa[1]][s], shift)
            pl[s * NRE:s * NRE + len(c)] = c
        planes[pa] = pl
    comb = {p: (mrc(planes[(p, 0)], planes[(p, 1)]) if nb_rx > 1 else planes[(p, 0)]) for p in range(nb_tx)}
    comp = alamouti(comb[0], comb[1]) if mimo_mode == ALAMOUTI else comb[0].copy()
    comp[~defined] = 0
    return dict(comp=comp, log2_maxh=shift, cfi=rx_pcfich(comp, N_RB, fp.Nid_cell, subframe), planes=planes,
                defined=defined, avg=avg)
