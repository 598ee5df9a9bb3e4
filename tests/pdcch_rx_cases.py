"""Shared helpers of the PDCCH receive tests: the transmit grid of generate_dci_top as the compensated
control symbols rx_pdcch works on, and the model's geometry inputs from the oracle."""
import ctypes
import itertools

import numpy as np

import ctrl_rx_model as M
import oracle_lib as O


def grid_to_comp(grid, fp, subframe, npd):
    """rxdataF_comp plane 0 of a unit channel: symbol s at s * 12 * N_RB_DL int32, the 12 N_RB_DL
    subcarriers in order (DC skipped); symbol 0 holds its 8 non-pilot REs per RB packed
    (pdcch_extract_rbs_single, dci.c:931-1100)."""
    N, NRE = fp.ofdm_symbol_size, 12 * fp.N_RB_DL
    comp = np.zeros(npd * NRE, dtype=np.int32)
    base = subframe * fp.symbols_per_tti * N
    k = np.arange(NRE)
    sc = np.where(k < NRE // 2, fp.first_carrier_offset + k, 1 + k - NRE // 2)
    for s in range(npd):
        row = np.asarray(grid[base + s * N:base + (s + 1) * N])[sc]
        if s == 0:
            row = row[(k % 3) != (fp.nushift % 3)]
        comp[s * NRE:s * NRE + len(row)] = row
    return comp


def geometry(fo, subframe, npd):
    """(mi, pcfich regs, phich reg triples, Mquad, nCCE, nCCE of 3 symbols with mi = 1) from the oracle"""
    mi = 1 if fo.frame_type == 0 else None
    assert mi is not None, "FDD only"
    pcf, _ = O.pcfich_reg_mapping(fo)
    return mi, pcf, O.phich_reg_mapping(fo), O.get_nquad(npd, fo, mi), O.get_nCCE(npd, fo, mi), O.get_nCCE(3, fo, 1)


def model_table(fo, subframe, npd):
    mi, pcf, ph, Mquad, _, _ = geometry(fo, subframe, npd)
    return M.pdcch_table(fo.N_RB_DL, npd, fo.Nid_cell, subframe, mi, pcf, ph, Mquad)


def dci_code_bits(length, L, rnti, pdu):
    """the rate-matched code bits of one DCI, by the oracle: orc_ccodelte_encode (CRC16 ^ RNTI, TBCC),
    orc_sub_block_interleaving_cc and orc_lte_rate_matching_cc"""
    data = bytes(reversed(bytes(pdu[:4]))) if length <= 32 else bytes(reversed(bytes(pdu[:8])))
    D = length + 16
    d = np.full(96 + 3 * D + 16, 2, dtype=np.uint8)
    d[96:96 + 3 * D] = O.ccode_encode(np.frombuffer(data, np.uint8), length, 2, rnti)
    w = np.zeros(3 * 32 * ((D + 31) >> 5) + 16, dtype=np.uint8)
    e = np.zeros((72 << L) + 16, dtype=np.uint8)
    L_ = O.orc()
    L_.orc_sub_block_interleaving_cc.restype = ctypes.c_uint32
    rcc = L_.orc_sub_block_interleaving_cc(ctypes.c_uint32(D), ctypes.c_void_p(d.ctypes.data + 96), ctypes.c_void_p(w.ctypes.data))
    L_.orc_lte_rate_matching_cc(ctypes.c_uint32(rcc), ctypes.c_uint16(72 << L), ctypes.c_void_p(w.ctypes.data),
                                ctypes.c_void_p(e.ctypes.data))
    return e[:72 << L].copy()


# the tmode-1 plan of dci_decoding_procedure (dci.c:2990-3356) at two DCI sizes per pass: common L = 2, 3
# (1A / 1C sizes), UE-specific L = 3..0 with format 0 / 1A, then format 1 with the early return
def tm1_plan(size_1a, size_1c, size_0, size_1):
    by = lambda b: 4 if b <= 32 else 8
    p = []
    for L in (2, 3):
        p.append((1, L, size_1a, by(size_1a), 2, 2, 0, 0))
        p.append((1, L, size_1c, by(size_1c), 4, 4, 4, 0))
    for L in (3, 2, 1, 0):
        p.append((0, L, size_0, by(size_0), 2, 2, 0, 0))
    for L in (0, 1, 2, 3):
        p.append((0, L, size_1, by(size_1), 2, 2, 1, 1))
    return p


def tx_items(fo, sf, size, rng, crnti, si_rnti):
    """The DCIs of the loop tests, placed as an eNB would (first free candidate of each search space):
    one common DCI (SI-RNTI, L = 2) and two UE DCIs (L = 0 and L = 3) where the control region holds
    their 13 CCEs; at 6 PRB it holds 4 CCEs at most, so there the two UE DCIs are L = 0 and L = 1 and
    no common DCI is sent.  Returns (items for generate_dci_top, n_common, num_pdcch_symbols)."""
    want = [(1, 2, si_rnti), (0, 3, crnti), (0, 0, crnti)] if O.get_nCCE(3, fo, 1) >= 13 else [(0, 1, crnti), (0, 0, crnti)]
    total = sum(1 << L for _, L, _ in want)
    npd = next(n for n in (1, 2, 3) if O.get_nCCE(n, fo, 1) >= total)
    nCCE, items = O.get_nCCE(npd, fo, 1), None
    for order in itertools.permutations(want):             # an eNB scheduler's search for a placement
        taken, placed = set(), []
        for common, L, rnti in order:
            cce = next((c for c in M.candidates(nCCE, O.get_nCCE(3, fo, 1), common, L, crnti, sf)
                        if not taken & set(range(c, c + (1 << L)))), None)
            if cce is None:
                break
            taken |= set(range(cce, cce + (1 << L)))
            placed.append((L, cce, rnti))
        if len(placed) == len(want):
            items = [(size, L, cce, rnti, bytes(rng.integers(0, 256, 8, dtype=np.uint8))) for L, cce, rnti in sorted(placed)]
            break
    assert items is not None, "no placement of the test DCIs in this control region"
    # the UE DCIs share one size: the first is a format 0 (leading payload bit 0), the second a format 1A
    # (bit 1), as dci_decoding_procedure0 tells them apart (dci.c:2730); two format 0s would count once
    ue = [i for i, it in enumerate(items) if it[3] == crnti]
    for n, i in enumerate(ue):
        pdu = bytearray(items[i][4])
        pdu[3] = (pdu[3] & 0x7F) | (0x80 if n & 1 else 0)
        items[i] = items[i][:4] + (bytes(pdu),)
    items.sort(key=lambda it: it[3] != si_rnti)            # common DCIs first, as generate_dci_top takes them
    return items, sum(1 for it in items if it[3] == si_rnti), npd


def pdu_bits(pdu, length):
    """the `length` payload bits of a DCI_ALLOC_t pdu (its bytes reversed, MSB first: dci.c:233-251)"""
    flip = bytes(reversed(bytes(pdu[:4]))) if length <= 32 else bytes(reversed(bytes(pdu[:8])))
    return np.unpackbits(np.frombuffer(flip, np.uint8))[:length].tolist()


def sent_came_back(items, found):
    """every transmitted PDU is among the found DCIs (cce, rnti, length, pdu) at its first CCE with its
    RNTI; the aggregation level a DCI is found at may be lower than the one it was sent at (its first
    CCEs alone decode: the search tries the plan's levels in the plan's order)"""
    for length, L, cce, rnti, pdu in items:
        if not any(c == cce and r == rnti and ln == length and pdu_bits(p, ln) == pdu_bits(pdu, length)
                   for c, r, ln, p in found):
            return False
    return True
