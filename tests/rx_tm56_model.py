"""numpy restatement of rx_pdsch for the single-layer precoding modes (MIMO_mode_t 3..7, TM4-6) as
dlsim's UE runs it (dual_stream_flag = 0), PHY/LTE_TRANSPORT/dlsch_demodulation.c:
  dlsch_extract_rbs_dual           :3683-4049 (the loop restated below, pointer steps as written) with
                                   pmi_ext = (pmi >> ((prb >> 2) << 1)) & 3 per allocated PRB (:3812, :3907)
  dlsch_channel_level              :2777-2838 over every (port, RX antenna), un-precoded estimates;
                                   log2_maxh = log2_approx(max avg) / 2, + 1 when dl_power_off == 1 (:285-292)
  prec2A_TM56_128                  :1273-1315, dlsch_channel_compensation_TM56 :1466-1669 (pmi_ext[rb]
                                   per 12 extracted REs, 8 in pilot symbols)
  dlsch_detection_mrc              :2583-2621
  dlsch_qpsk / 16qam / 64qam_llr   dlsch_llr_computation.c:636-930
Integer arithmetic lane for lane (SSE: adds / subs / sign / mulhi / slli_epi16, madd_epi16 with int32
wrap, srai_epi32 + packs_epi32).  dlsch_demodulation.c needs PHY_VARS_UE and cannot be compiled
stand-alone, so this model is the pin; tests/test_rx_tm56_cpu.py cross-checks it against the C oracle
where they overlap and by decoding.

precoded_cqi_dB and the in-place overwrite of dl_ch_estimates_ext are not restated (no LLR depends on
them)."""
import numpy as np

RULE_UE, RULE_TX = 0, 1
QAM16_n1, QAM64_n1, QAM64_n2 = 20724, 20225, 10112          # PHY/impl_defs_top.h:215-224
ONE_OVER_SQRT2_Q15 = 23170


class Refused(Exception):
    """the reference's behaviour is undefined (or it reads ext slots it did not write) for this input"""


def alloc_bit(rb_alloc, rb):
    return (rb_alloc[rb >> 5] >> (rb & 31)) & 1 if rb < 100 else 0


def get_pmi_tx(n_rb, mode, pmi_alloc, rb):
    """the transmitter's get_pmi (dlsch_modulation.c:1136-1178) for the two-bit modes (<= 8)"""
    sb = rb if n_rb == 6 else rb // 6 if n_rb == 50 else rb >> 3 if n_rb == 100 else rb >> 2
    return ((pmi_alloc & 0xFFFF) >> (2 * sb)) & 3 if 2 * sb < 32 else 0


def pmi_of(n_rb, mode, pmi_alloc, prb, rule):
    """pmi_ext of allocated PRB prb.  RULE_UE: the unsigned short pmi is promoted to int, so a shift
    count of 16..31 reads 0; a count >= 32 is undefined in C (Refused unless pmi_alloc == 0)."""
    if rule == RULE_TX:
        return get_pmi_tx(n_rb, mode, pmi_alloc, prb)
    cnt = (prb >> 2) << 1
    if cnt >= 32:
        if pmi_alloc & 0xFFFF:
            raise Refused(f"PRB {prb}: shift count {cnt}")
        return 0
    return ((pmi_alloc & 0xFFFF) >> cnt) & 3


def adjust_G2(fp, rb_alloc, subframe, symbol):
    """lte_mcs.c:157-245"""
    nsymb = 14 if fp.Ncp == 0 else 12
    if subframe not in (0, 5, 6):
        return 0
    if symbol < (nsymb >> 1) and fp.frame_type == 1 and subframe != 6:
        return 0
    if fp.frame_type == 1:
        if symbol > (nsymb >> 1) + 3 and symbol != nsymb - 1:
            return 0
        if subframe == 5 and symbol != nsymb - 1:
            return 0
        if subframe == 6 and symbol != 2:
            return 0
    else:
        if symbol > (nsymb >> 1) + 3 or symbol < (nsymb >> 1) - 2:
            return 0
        if subframe == 5 and symbol not in ((nsymb >> 1) - 1, (nsymb >> 1) - 2):
            return 0
        if subframe == 6:
            return 0
    half, re = fp.N_RB_DL >> 1, 0
    if fp.N_RB_DL & 1:
        for rb in range(half - 3, half + 4):
            if alloc_bit(rb_alloc, rb):
                re += 6 if rb in (half - 3, half + 3) else 12
    else:
        for rb in range(half - 3, half + 3):
            if alloc_bit(rb_alloc, rb):
                re += 12
    return re


def extract_dual(fp, rb_alloc, subframe, l):
    """dlsch_extract_rbs_dual of one symbol, one antenna's pass (every antenna and both ports share the
    slots).  Returns (bins, cols, prbs, nb_rb, n): FFT bin and estimate column (without the 5-word
    offset) of each ext slot, the allocated PRBs in the order pmi_loc advances, and n = the prefix of
    slots that the call wrote with the received RE and both ports' estimates from the same column (the
    odd-N_RB_DL full-RB branch moves dl_ch0_ext by 144 per RB, :3932-3934, and the skip_half = 2 pilot
    branch advances its pointers inside the RE loop, :3955-3967)."""
    Ncp, ns = fp.Ncp, fp.nushift
    smod = l - (7 - Ncp) if l >= 7 - Ncp else l
    pil = smod == 0 or smod == 4 - Ncp
    nsymb, half, fco = (14 if Ncp == 0 else 12), fp.N_RB_DL >> 1, fp.first_carrier_offset
    sss = nsymb - 1 if fp.frame_type == 1 else (nsymb >> 1) - 2
    pss = 2 if fp.frame_type == 1 else (nsymb >> 1) - 1
    X = 12 * 110 + 256
    bins, cols, col0s = np.zeros(X, np.int64), np.full(X, -1, np.int64), np.full(X, -2, np.int64)
    st = dict(p=0, drift=0, hw=0)

    def put(pos, b, c):
        bins[pos], cols[pos] = b, c
        if pos + st["drift"] < X:
            col0s[pos + st["drift"]] = c
        st["hw"] = max(st["hw"], pos + 1)

    def data4(i):
        return i != ns and i != ns + 3 and i != ns + 6 and i != (ns + 9) % 12

    prbs = []
    pbch_l = (nsymb >> 1) <= l < (nsymb >> 1) + 4
    for prb in range(fp.N_RB_DL):
        ind = alloc_bit(rb_alloc, prb)
        centre = half - 3 < prb < half + 3
        if subframe == 0 and centre and pbch_l:
            ind = 0
        if subframe in (0, 5) and centre and l == sss:
            ind = 0
        if fp.frame_type == 0 and subframe in (0, 5) and centre and l == pss:
            ind = 0
        if fp.frame_type == 1 and subframe == 6 and half - 3 <= prb <= half + 3 and l == pss:
            ind = 0
        if not ind:
            continue
        prbs.append(prb)
        p, c0 = st["p"], 12 * prb
        if fp.N_RB_DL & 1 == 0:
            b0 = fco + 12 * prb if prb < half else 1 + 12 * (prb - half)
            j = 0
            for i in range(12):
                if not pil or data4(i):
                    put(p + j, b0 + i, c0 + i)
                    j += 1
            st["p"] += 8 if pil else 12
            continue
        skip = 0
        if subframe == 0 and prb == half - 3 and pbch_l:
            skip = 1
        elif subframe == 0 and prb == half + 3 and pbch_l:
            skip = 2
        if subframe in (0, 5) and prb == half - 3 and l == sss:
            skip = 1
        elif subframe in (0, 5) and prb == half + 3 and l == sss:
            skip = 2
        if (fp.frame_type == 0 and subframe in (0, 5)) or (fp.frame_type == 1 and subframe in (2, 6)):
            if prb == half - 3 and l == pss:
                skip = 1
            elif subframe in (0, 5) and prb == half + 3 and l == pss:
                skip = 2
        b0 = fco + 12 * prb if prb <= half else 7 + 12 * (prb - half - 1)
        if prb != half:
            if not pil:
                o, cnt = (6 if skip == 2 else 0), (6 if skip else 12)
                for i in range(cnt):
                    put(p + i, b0 + o + i, c0 + o + i)
                st["p"] += cnt
                if not skip:
                    st["drift"] += 132                    # `for (i=0;i<12;i++) dl_ch0_ext+=12;`
            elif skip == 1:
                j = 0
                for i in range(6):
                    if i != ns and i != (ns + 3) % 6:
                        put(p + j, b0 + i, c0 + i)
                        j += 1
                st["p"] += 4
            elif skip == 2:
                j = 0
                for i in range(6):
                    if i != ns and i != (ns + 3) % 6:
                        put(st["p"] + j, b0 + i + 6, c0 + i + 6)
                        j += 1
                    st["p"] += 4                          # inside the loop, as written
            else:
                j = 0
                for i in range(12):
                    if data4(i):
                        put(p + j, b0 + i, c0 + i)
                        j += 1
                st["p"] += 8
        else:                                             # the RB around DC
            if not pil:
                for i in range(6):
                    put(p + i, b0 + i, c0 + i)
                for i in range(6):
                    put(p + 6 + i, i, c0 + 6 + i)         # bins 0..5 (:4002-4006)
                st["p"] += 12
            else:
                j = 0
                for i in range(6):
                    if i != ns and i != (ns + 3) % 6:
                        put(p + j, b0 + i, c0 + i)
                        j += 1
                for i in range(6, 12):
                    if i != (ns + 6) % 12 and i != (ns + 9) % 12:
                        put(p + j, 1 + i - 6, c0 + i)
                        j += 1
                st["p"] += 8
    n = 0
    while n < st["hw"] and cols[n] >= 0 and cols[n] == col0s[n]:
        n += 1
    return bins[:st["hw"]], cols[:st["hw"]], prbs, len(prbs), n, pil


# ---- int16 lane arithmetic -------------------------------------------------------------------------
def s16(v):
    """wrap to int16 (kept as int64 values)"""
    return ((np.asarray(v, np.int64) + 32768) & 0xFFFF) - 32768


def s32(v):
    return ((np.asarray(v, np.int64) + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31


def sat16(v):
    return np.clip(np.asarray(v, np.int64), -32768, 32767)


def mulhi2(a, b):
    """mulhi_epi16 then slli_epi16 1"""
    return s16(((np.asarray(a, np.int64) * b) >> 16) << 1)


def split(w):
    """(re, im) int16 components of int32 words, as int64"""
    w = np.asarray(w).astype(np.int32)
    return s16(w.astype(np.int64) & 0xFFFF), s16((w.astype(np.int64) >> 16) & 0xFFFF)


def prec_tm56(h0r, h0i, h1r, h1i, p):
    """prec2A_TM56_128 on (re, im) components: sat(h0 + w_p h1) then mulhi(., 23170) << 1"""
    p = np.asarray(p)
    tr, ti = h1i, s16(-np.asarray(h1r, np.int64))                 # sign_epi16 by conjugate[], then swap
    gr = np.where(p == 0, sat16(h0r + h1r), np.where(p == 1, sat16(h0r - h1r),
                  np.where(p == 2, sat16(h0r - tr), sat16(h0r + tr))))
    gi = np.where(p == 0, sat16(h0i + h1i), np.where(p == 1, sat16(h0i - h1i),
                  np.where(p == 2, sat16(h0i - ti), sat16(h0i + ti))))
    return mulhi2(gr, ONE_OVER_SQRT2_Q15), mulhi2(gi, ONE_OVER_SQRT2_Q15)


def madd(a0, b0, a1, b1):
    return s32(np.asarray(a0, np.int64) * b0 + np.asarray(a1, np.int64) * b1)


def compensate(hr, hi, yr, yi, sh, Qm):
    """conj(h') y >> sh and the scaled magnitudes of one antenna"""
    cr = sat16(madd(hr, yr, hi, yi) >> sh)
    ci = sat16(madd(s16(-hi), yr, hr, yi) >> sh)
    a1 = QAM16_n1 if Qm == 4 else QAM64_n1 if Qm == 6 else 0
    a2 = QAM64_n2 if Qm == 6 else 0
    m = sat16(madd(hr, hr, hi, hi) >> sh)
    return cr, ci, mulhi2(m, a1), mulhi2(m, a2)


def mrc(x0, x1):
    return sat16((x0 >> 1) + (x1 >> 1))


def abs16(v):
    return s16(np.abs(np.asarray(v, np.int64)))                   # abs_epi16: -32768 stays


def llr_stage(Qm, cr, ci, mag, magb):
    """dlsch_qpsk / 16qam / 64qam_llr: [n, Qm] int16"""
    out = [cr, ci]
    if Qm > 2:
        out += [sat16(mag - abs16(cr)), sat16(mag - abs16(ci))]
    if Qm > 4:
        out += [sat16(magb - abs16(out[2])), sat16(magb - abs16(out[3]))]
    return np.stack(out, axis=1).astype(np.int16)


def log2_approx(x):
    x = int(x) & 0x7FFFFFFF
    return x.bit_length()


def channel_level(est_cols, div):
    """dlsch_channel_level of one (port, antenna): int32 wrap sum of |h|^2 over the level REs / div
    (C division)"""
    r, i = split(est_cols)
    tot = int(s32(np.sum(r * r + i * i)))
    return int(abs(tot) // div) * (1 if tot >= 0 else -1)


def rx_pdsch_tm56(fp, rxF, est, rb_alloc, Qm, mode, pmi_alloc, dl_power_off, num_pdcch, subframe, rule=RULE_UE,
                  parts=None):
    """rxF = [nb_rx][nsymb*N] int32, est[(p, a)] = [nsymb*N] int32.  Returns (LLRs int16, log2_maxh).
    parts, a list, receives per symbol (cr, ci, mag, magb) of the demodulated REs after the MRC."""
    if not 3 <= mode <= 7:
        raise Refused("Unknown MIMO mode")                        # :595-597 (mode 8)
    nb_rx, N = len(rxF), fp.ofdm_symbol_size
    nsymb = 14 if fp.Ncp == 0 else 12
    out, log2_maxh = [], 0
    for l in range(num_pdcch, nsymb):
        bins, cols, prbs, nb_rb, n, pil = extract_dual(fp, rb_alloc, subframe, l)
        if nb_rb == 0:
            raise Refused("nb_rb = 0")
        smod = l - (7 - fp.Ncp) if l >= 7 - fp.Ncp else l
        nre = 8 if pil else 12
        pm = np.array([pmi_of(fp.N_RB_DL, mode, pmi_alloc, prb, rule) for prb in prbs], np.int64)
        if l == num_pdcch:
            lvl = (8 if smod == 0 else 12) * nb_rb
            if lvl > n:
                raise Refused("the level reads unwritten ext slots")
            avgs = 0
            for a in range(nb_rx):
                for p in (0, 1):
                    avgs = max(avgs, channel_level(np.asarray(est[(p, a)])[l * N + 5 + cols[:lvl]], lvl))
            log2_maxh = log2_approx(avgs) // 2 + (1 if dl_power_off == 1 else 0)
        adj = 0 if Qm == 2 else adjust_G2(fp, rb_alloc, subframe, l)
        ln = nb_rb * 8 - 2 * adj // 3 if pil else nb_rb * 12 - adj
        ln = max(ln, 0)
        if ln > n:
            raise Refused("the LLRs read unwritten ext slots")
        b, c = bins[:ln], cols[:ln]
        pe = pm[np.arange(ln) // nre]                             # pmi_ext[rb] per nre extracted REs
        acc = None
        for a in range(nb_rx):
            yr, yi = split(np.asarray(rxF[a])[l * N + b])
            h0r, h0i = split(np.asarray(est[(0, a)])[l * N + 5 + c])
            h1r, h1i = split(np.asarray(est[(1, a)])[l * N + 5 + c])
            hr, hi = prec_tm56(h0r, h0i, h1r, h1i, pe)
            cur = compensate(hr, hi, yr, yi, log2_maxh, Qm)
            acc = cur if acc is None else tuple(mrc(x0, x1) for x0, x1 in zip(acc, cur))
        if parts is not None:
            parts.append(acc)
        out.append(llr_stage(Qm, *acc).reshape(-1))
    return np.concatenate(out), log2_maxh
