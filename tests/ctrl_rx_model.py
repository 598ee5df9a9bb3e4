"""Numpy model of the UE control decoding chain, restated from the reference's text:

  viterbi        phy_viterbi_lte_sse2       PHY/CODING/viterbi_lte.c:140-416
  cc_rx_plan     generate_dummy_w_cc + lte_rate_matching_cc_rx + sub_block_deinterleaving_cc
                                            PHY/CODING/lte_rate_matching.c:384, :834-906, :245-291
  dci_decoding   dci_decoding               PHY/LTE_TRANSPORT/dci.c:2426-2489
  dci_crc        crc16 ^ extract_crc        dci.c:122-163, :2660
  pbch_decode    rx_pbch from the quantised soft bits on   PHY/LTE_TRANSPORT/pbch.c:975-1043
  pdcch_table    pdcch_llr / _demapping / _deinterleaving / _unscrambling   dci.c:342-549, 603-638, 1932-1961
  procedure0     dci_decoding_procedure0 and the stops between its calls     dci.c:2547-2786, 3032, 3266

TEST INFRASTRUCTURE ONLY.  Everything is literal: 8-bit saturating add, min-subtract after every
step, ties to the predecessor k + 32, first strictly largest final metric.
"""
import numpy as np

GLTE = (0o133, 0o171, 0o165)
GLTE_REV = (0o155, 0o117, 0o127)
BITREV_CC = np.array([1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31,
                      0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30])


def _parity(x):
    return bin(x).count("1") & 1


# ccodelte_table_rev (ccoding_byte_lte.c:270-289): input in the LSB, the state in the 6 MSBs
REV = np.array([sum(_parity(i & GLTE_REV[j]) << j for j in range(3)) for i in range(128)])
_SIGN = np.array([[1 if (c >> i) & 1 else -1 for i in range(3)] for c in range(8)])   # w[c] = 24 + sum sign * in


def tbcc_encode(c):
    """d[3 i + s] = parity(g_s & (c_i .. c_{i-6} mod D)): the tail-biting encoder (36.212 5.1.3.1)"""
    c = np.asarray(c, dtype=np.int64)
    D = len(c)
    d = np.zeros(3 * D, dtype=np.uint8)
    for s, g in enumerate(GLTE):
        for t in range(7):
            if (g >> (6 - t)) & 1:
                d[s::3] ^= np.roll(c, t).astype(np.uint8)
    return d


def viterbi_batch(y):
    """y: (B, n, 3) integers in [-8, 7].  Returns dict of decoded bytes (B, ceil(n/8)), start state (B,),
    final metrics (B, 64), the largest pre-renormalisation metric (B,) and the saturation flag (B,)."""
    y = np.asarray(y, dtype=np.int64)
    assert y.min() >= -8 and y.max() <= 7
    B, n, _ = y.shape
    k = np.arange(32)
    m = np.zeros((B, 64), dtype=np.int64)
    dec = np.zeros((n, B, 64), dtype=np.uint8)
    peak = np.zeros(B, dtype=np.int64)
    sat = np.zeros(B, dtype=bool)
    for it in range(2):
        for p in range(n):
            w = 24 + y[:, p, :] @ _SIGN.T                          # (B, 8)
            nm = np.zeros_like(m)
            for b in range(2):
                lo = m[:, k] + w[:, REV[2 * k + b]]
                hi = m[:, k + 32] + w[:, REV[2 * (k + 32) + b]]
                sat |= (lo > 255).any(axis=1) | (hi > 255).any(axis=1)
                lo, hi = np.minimum(lo, 255), np.minimum(hi, 255)
                mx = np.maximum(lo, hi)
                nm[:, 2 * k + b] = mx
                dec[p][:, 2 * k + b] = mx == hi                   # a tie selects k + 32
            peak = np.maximum(peak, nm.max(axis=1))
            m = nm - nm.min(axis=1, keepdims=True)
    start = np.argmax(m, axis=1)                                  # first of the largest; all equal -> 0
    out = np.zeros((B, (n + 7) >> 3), dtype=np.uint8)
    s = start.copy()
    rows = np.arange(B)
    for p in range(n - 1, -1, -1):
        out[:, p >> 3] += ((s & 1) << (7 - (p & 7))).astype(np.uint8)
        s = (s >> 1) + 32 * dec[p][rows, s]
    return {"bytes": out, "start": start, "metrics": m, "peak": peak, "sat": sat, "end": s}


def viterbi(y, n):
    y = np.asarray(y, dtype=np.int64)[:3 * n].reshape(1, n, 3)
    r = viterbi_batch(y)
    return r["bytes"][0], int(r["start"][0]), r["metrics"][0].astype(np.uint8)


def clamp(y):
    return np.clip(np.asarray(y, dtype=np.int64), -8, 7)


def cc_rx_plan(D):
    """plan[3 i + s] = the first e index that lte_rate_matching_cc_rx sums into d^(s)_i; the others
    follow every 3 D.  The k-th non-<NULL> entry of dummy_w (stream, then column, then row) is
    d position (32 row + bitrev[col] - ND, stream)."""
    R = (D + 31) >> 5
    ND = 32 * R - D
    plan = np.zeros(3 * D, dtype=np.uint16)
    for s in range(3):
        j = 0
        for col in range(32):
            for row in range(R):
                i = 32 * row + int(BITREV_CC[col]) - ND
                if i < 0:
                    continue
                plan[3 * i + s] = s * D + j
                j += 1
        assert j == D
    return plan


def cc_rx_d(D, E, e):
    """the Viterbi's input of dci_decoding / rx_pbch: summed, clamped, deinterleaved"""
    e = np.asarray(e, dtype=np.int64)[:E]
    plan = cc_rx_plan(D).astype(np.int64)
    d = np.zeros(3 * D, dtype=np.int64)
    for q in range(3 * D):
        d[q] = e[plan[q]::3 * D].sum()
    return np.clip(d, -8, 7)


def crc16(data, bitlen):
    """crc16 (crc_byte.c:155-171) >> 16: MSB first, polynomial 0x1021, zero start"""
    reg = 0
    for i in range(bitlen):
        bit = (int(data[i >> 3]) >> (7 - (i & 7))) & 1
        fb = ((reg >> 15) ^ bit) & 1
        reg = (reg << 1) & 0xFFFF
        if fb:
            reg ^= 0x1021
    return reg


def extract_crc(data, bitlen):
    """the 16 bits that follow bit `bitlen` (dci.c:122-163)"""
    v = 0
    for i in range(bitlen, bitlen + 16):
        v = (v << 1) | ((int(data[i >> 3]) >> (7 - (i & 7))) & 1)
    return v


def dci_decoding(dci_length, L, e):
    """Returns (decoded_output with 2 + (D >> 3) bytes, crc16 ^ extract_crc)"""
    D, E = dci_length + 16, 72 << L
    d = cc_rx_d(D, E, e)
    b, _, _ = viterbi(d, D)
    out = np.zeros(2 + (D >> 3) + 1, dtype=np.uint8)
    out[:len(b)] = b
    return out[:2 + (D >> 3)], crc16(out, dci_length) ^ extract_crc(out, dci_length)


def gold_words(c_init, n):
    """lte_gold_generic (lte_gold.c:151-177): n successive 32-bit words"""
    M = 0xFFFFFFFF
    x1 = 1 + (1 << 31)
    x2 = c_init
    x2 = (x2 ^ ((x2 ^ (x2 >> 1) ^ (x2 >> 2) ^ (x2 >> 3)) << 31)) & M

    def step(x1, x2):
        x1 = (x1 >> 1) ^ (x1 >> 4)
        x1 = (x1 ^ (x1 << 31) ^ (x1 << 28)) & M
        x2 = (x2 >> 1) ^ (x2 >> 2) ^ (x2 >> 3) ^ (x2 >> 4)
        x2 = (x2 ^ (x2 << 31) ^ (x2 << 30) ^ (x2 << 29) ^ (x2 << 28)) & M
        return x1, x2
    for _ in range(49):
        x1, x2 = step(x1, x2)
    out = []
    for _ in range(n):
        x1, x2 = step(x1, x2)
        out.append(x1 ^ x2)
    return out


def pbch_unscramble(llr, Nid_cell, frame_mod4):
    """pbch_unscrambling (pbch.c:785-814): int8 negation of the quarter where the Gold bit is 0"""
    llr = np.asarray(llr, dtype=np.int8).copy()
    E = len(llr)
    g = gold_words(Nid_cell, (E + 31) // 32)
    bits = np.array([(g[i >> 5] >> (i & 31)) & 1 for i in range(E)])
    q = E >> 2
    sel = np.zeros(E, dtype=bool)
    sel[frame_mod4 * q:(frame_mod4 + 1) * q] = True
    flip = sel & (bits == 0)
    with np.errstate(over="ignore"):
        llr[flip] = (-llr[flip].astype(np.int16)).astype(np.int8)   # -(-128) stays -128 as in the reference
    return llr


def pbch_decode(llr, Nid_cell, frame_mod4):
    """Returns (antenna count 1 / 2 / 4 or -1, the three MIB bytes)"""
    e = pbch_unscramble(llr, Nid_cell, frame_mod4)
    d = cc_rx_d(40, len(e), e)
    a, _, _ = viterbi(d, 40)
    crc = crc16(a, 24) ^ ((int(a[3]) << 8) + int(a[4]))
    n = {0x0000: 1, 0xFFFF: 2, 0x5555: 4}.get(crc, -1)
    return n, bytes(int(x) for x in a[2::-1])


# ---- rx_pdcch after compensation (dci.c:1852-1897) as a gather, and the DCI search ----
MSYMB = ((2 * 33 + 22) * 72) // 2
NONE = 0xFFFFFFFF


def pdcch_gather(N_RB, npd, Nid, mi, pcfich_reg, phich_regs, Mquad):
    """The comp RE index behind every QPSK symbol of e_rx (-1: none): pdcch_demapping (dci.c:342-446, with
    its two RE counters and the break that leaves the inner loop only) and pdcch_deinterleaving
    (:449-549), normal prefix.  phich_regs: the Ngroup triples check_phich_reg scans (:62-121)."""
    NRE = 12 * N_RB
    Msymb2 = {100: MSYMB, 50: MSYMB >> 1, 6: MSYMB * 6 // 100}.get(N_RB, MSYMB >> 2)

    def taken(kp, lp):
        if lp > 0:
            return False
        m = kp // 6
        if m in pcfich_reg:
            return True
        return mi > 0 and any(m in t for t in phich_regs)

    wbar = {}
    mprime = re_offset = re_offset0 = 0
    for kp in range(NRE):
        for lp in range(npd):
            so = NRE * lp
            if taken(kp, lp):
                if lp == 0 and kp % 6 == 0:
                    re_offset0 += 4
            elif lp == 0:
                if kp % 12 in (0, 6):
                    for _ in range(4):
                        wbar[mprime] = so + re_offset0
                        mprime += 1
                        re_offset0 += 1
            elif kp % 12 in (0, 4, 8):
                for i in range(4):
                    wbar[mprime] = so + re_offset + i
                    mprime += 1
            if mprime >= Msymb2:
                break
        re_offset += 1
    wtemp = [-1] * (4 * Mquad)
    for i in range(Mquad):
        for j in range(4):
            wtemp[4 * ((i + Nid) % Mquad) + j] = wbar.get(4 * i + j, -1)
    RCC = (Mquad + 31) >> 5
    ND = 32 * RCC - Mquad
    z = [-1] * (4 * Mquad)
    k = 0
    for col in range(32):
        index = int(BITREV_CC[col])
        for _ in range(RCC):
            if index >= ND:
                z[4 * (index - ND):4 * (index - ND) + 4] = wtemp[4 * k:4 * k + 4]
                k += 1
            index += 32
    return z


def pdcch_table(N_RB, npd, Nid, subframe, mi, pcfich_reg, phich_regs, Mquad):
    """per soft bit of e_rx: int16 index into comp | negate << 31 (pdcch_unscrambling, :1932-1961: over
    72 nCCE soft bits, negated where the Gold bit is 0), NONE where nothing is mapped"""
    z = pdcch_gather(N_RB, npd, Nid, mi, pcfich_reg, phich_regs, Mquad)
    n, nuns = 8 * Mquad, 72 * (Mquad // 9)
    g = gold_words((subframe << 9) + Nid, (n + 31) // 32)
    tab = np.full(n, NONE, dtype=np.uint32)
    for i in range(n):
        re = z[i >> 1]
        if re < 0:
            continue
        neg = 1 if (i < nuns and ((g[i >> 5] >> (i & 31)) & 1) == 0) else 0
        tab[i] = (2 * re + (i & 1)) | (neg << 31)
    return tab


def pdcch_soft_bits(comp, tab):
    """pdcch_llr (:603-638): clip to [-32, 31]; then the gather and the sign"""
    c16 = np.clip(np.ascontiguousarray(comp, dtype=np.int32).view(np.int16).astype(np.int64), -32, 31)
    tab = np.asarray(tab, dtype=np.int64)
    e = np.zeros(len(tab), dtype=np.int8)
    ok = tab != NONE
    v = c16[tab[ok] & 0x7FFFFFFF]
    e[ok] = np.where(tab[ok] >> 31, -v, v)
    return e


def candidates(nCCE, nCCE_max, do_common, L, crnti, subframe):
    """CCEind of every candidate of one dci_decoding_procedure0 call (dci.c:2576-2624)"""
    L2 = 1 << L
    if nCCE > nCCE_max or nCCE < L2:
        return []
    if do_common == 1:
        Yk, nb = 0, (4 if L2 == 4 else 2)
    else:
        Yk = crnti
        for _ in range(subframe + 1):
            Yk = (Yk * 39827) % 65537
        Yk %= nCCE // L2
        nb = 6 if L2 <= 2 else 2
    if nb * L2 > nCCE:
        nb = nCCE // L2
    return [((Yk + m) % (nCCE // L2)) * L2 for m in range(nb)]


def new_state():
    return {"maps": [0, 0, 0], "cnt": 0, "f0": 0, "fc": 0, "nCCE": -1, "ovf": 0, "alloc": {}}


def procedure0(st, e_rx, nCCE, nCCE_max, crnti, si_rnti, ra_rnti, subframe, entry, cap=255):
    """dci_decoding_procedure0 (dci.c:2547-2786); entry = (do_common, L, sizeof_bits, sizeof_bytes,
    format_si, format_ra, format_c, stop_if_found).  alloc[slot] = (dci_length, L, nCCE, rnti, format,
    pdu bytes); the slot at cnt is filled before acceptance is known (format None until accepted)."""
    do_common, L, bits, nbytes, f_si, f_ra, f_c, _ = entry
    for cce in candidates(nCCE, nCCE_max, do_common, L, crnti, subframe):
        mask = ((1 << (1 << L)) - 1) << (cce & 31)
        if st["maps"][cce >> 5] & mask:
            continue
        out, crc = dci_decoding(bits, L, e_rx[72 * cce:72 * cce + (72 << L)])
        out = np.concatenate([out, np.zeros(8, np.uint8)])
        if not ((L > 1 and crc in (si_rnti, ra_rnti)) or crc == crnti):
            continue
        if st["cnt"] >= cap:                                 # the library's bounded result: the match only marks its CCEs
            st["ovf"] = 1
            st["maps"][cce >> 5] |= mask
            continue
        nb = 4 if nbytes <= 4 else 8
        pdu = bytes(int(out[nb - 1 - i]) for i in range(nb)) + bytes(8 - nb)
        fmt = None
        if crc == si_rnti:
            fmt = f_si
        elif crc == ra_rnti:
            fmt = f_ra
            st["nCCE"] = cce
        elif crc == crnti:
            if f_c == 0 and (out[0] & 0x80) == 0:
                if st["f0"] == 0:
                    fmt, st["f0"], st["nCCE"] = 0, 1, cce
            elif f_c == 0:
                fmt, st["nCCE"] = 2, cce
            elif st["fc"] == 0:
                fmt, st["fc"], st["nCCE"] = f_c, 1, cce
        st["alloc"][st["cnt"]] = (bits, L, cce, crc, fmt, pdu)
        if fmt is not None:
            st["cnt"] += 1
        st["maps"][cce >> 5] |= mask                         # also when the counter did not advance
    return st


def dci_search(e_rx, nCCE, nCCE_max, crnti, si_rnti, ra_rnti, subframe, plan, cap=8):
    """the plan's calls in order with dci_decoding_procedure's stops between them; cap: the result's DCI slots"""
    st = new_state()
    for i, entry in enumerate(plan):
        if i > 0 and (st["maps"][0] == 0xFFFF or (st["f0"] and st["fc"])):
            break
        old = st["cnt"]
        procedure0(st, e_rx, nCCE, nCCE_max, crnti, si_rnti, ra_rnti, subframe, entry, cap)
        if entry[7] and st["cnt"] > old:
            break
    return st


def pbch_encode(mib_reversed, amask, Nid_cell, E):
    """The scrambled coded bits pbch_e of generate_pbch (pbch.c:161-420) for the CRC mask `amask`
    (0, 0xffff, 0x5555 = 1, 2, 4 eNB antennas): a = the MIB bytes as rx_pbch returns them, reversed."""
    a = bytes(mib_reversed[::-1])
    crc = crc16(a, 24) ^ amask
    c = np.concatenate([np.unpackbits(np.frombuffer(a, np.uint8)), np.array([(crc >> (15 - i)) & 1 for i in range(16)], np.uint8)])
    d = tbcc_encode(c)
    inv = np.zeros(120, dtype=np.int64)
    inv[cc_rx_plan(40).astype(np.int64)] = np.arange(120)
    e = d[inv[np.arange(E) % 120]]
    g = gold_words(Nid_cell, (E + 31) // 32)
    return e ^ np.array([(g[i >> 5] >> (i & 31)) & 1 for i in range(E)], dtype=np.uint8)
