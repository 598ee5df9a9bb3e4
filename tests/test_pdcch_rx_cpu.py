"""CPU suite of the PDCCH receive tables (no GPU):

  - the exported soft-bit gather table (oai4g_pdcch_soft_bit_table) equals the model's literal
    pdcch_llr / pdcch_demapping / pdcch_deinterleaving / pdcch_unscrambling for 6 / 25 / 50 / 100 PRB,
    Nid_cell 0 / 1 / 137, subframes 0 and 7, 1..3 control symbols and two PHICH resources (mi > 0);
  - the exported candidate lists (oai4g_pdcch_candidates) equal the model's for both search spaces;
  - the soft-bit chain against the oracle transmitter: the oracle's generate_dci_top grid taken as
    rxdataF_comp (SISO) and gathered through the exported table carries, on each DCI's CCEs, the
    signs of its rate-matched code bits (orc_ccodelte_encode + orc_lte_rate_matching_cc), and 0 on
    every <NIL> position; the model's DCI search then finds exactly the transmitted DCIs;
  - refusals: 4 TX ports, the geometries generate_dci_top refuses, L > 3, DCI_LENGTH > 45, and the
    error value of every device entry point without a device.
"""
import ctypes

import numpy as np
import pytest

import ctrl_rx_model as M
import openair4g_amd as oai
import oracle_lib as O
import pdcch_rx_cases as PC

CRNTI, SI, RA = 0x1234, 0xFFFF, 0x0002


def _frames(N_RB, Nid, phich_resource=1):
    fo, fg = O.frame(N_RB, Nid), oai.frame_parms(N_RB, Nid)
    fo.phich_resource = fg.phich_resource = phich_resource
    return fo, fg


@pytest.mark.parametrize("N_RB", [6, 25, 50, 100])
@pytest.mark.parametrize("Nid", [0, 1, 137])
def test_soft_bit_table_equals_model(N_RB, Nid):
    for res in (1, 6):
        fo, fg = _frames(N_RB, Nid, res)
        assert len(O.phich_reg_mapping(fo)) > 0
        for sf in (0, 7):
            for npd in (1, 2, 3):
                tab = oai.pdcch_soft_bit_table(fg, sf, npd)
                ref = PC.model_table(fo, sf, npd)
                assert len(tab) == 8 * O.get_nquad(npd, fo, 1)
                assert np.array_equal(tab, ref), (N_RB, Nid, res, sf, npd)
                src = tab[tab != M.NONE] & 0x7FFFFFFF
                assert len(np.unique(src)) == len(src) and src.max() < 2 * npd * 12 * N_RB


@pytest.mark.parametrize("N_RB", [6, 25, 50, 100])
@pytest.mark.parametrize("Nid", [0, 1, 137])
def test_candidates_equal_model(N_RB, Nid):
    """the same grid as the table: nCCE, which sets the candidate cut and the Yk modulus, moves with all of it"""
    seen = set()
    for res in (1, 6):
        fo, fg = _frames(N_RB, Nid, res)
        for sf in (0, 7):
            for npd in (1, 2, 3):
                _, _, _, _, nCCE, nmax = PC.geometry(fo, sf, npd)
                seen.add(nCCE)
                for crnti in (CRNTI, 1, 0xFFF3):
                    for common in (0, 1):
                        for L in range(4):
                            got = oai.pdcch_candidates(fg, npd, sf, crnti, common, L)
                            assert got == M.candidates(nCCE, nmax, common, L, crnti, sf), (res, sf, npd, crnti, common, L)
                            assert all(c % (1 << L) == 0 and c + (1 << L) <= nCCE for c in got)
                            assert (len(got) == 0) == (nCCE < (1 << L))
    assert len(seen) >= 3                                  # the symbol count and the PHICH resource move nCCE


CHAIN = [(25, 137, 0), (25, 137, 7), (6, 137, 7), (50, 1, 0), (100, 0, 7)]


@pytest.mark.parametrize("N_RB,Nid,sf", CHAIN)
def test_soft_bit_chain_against_the_oracle_transmitter(N_RB, Nid, sf):
    fo, fg = _frames(N_RB, Nid, 6)
    rng = np.random.default_rng(N_RB + Nid + sf)
    size = 27 if N_RB > 6 else 21
    items, n_common, npd_want = PC.tx_items(fo, sf, size, rng, CRNTI, SI)
    grid = np.zeros(10 * fo.symbols_per_tti * fo.ofdm_symbol_size, dtype=np.int32)
    npd = O.generate_dci_top(items, n_common, 512, fo, [grid], sf)
    assert npd == npd_want
    nCCE_tx = O.get_nCCE(npd, fo, 1)
    comp = PC.grid_to_comp(grid, fo, sf, npd)
    e = M.pdcch_soft_bits(comp, oai.pdcch_soft_bit_table(fg, sf, npd))
    assert np.array_equal(e, M.pdcch_soft_bits(comp, PC.model_table(fo, sf, npd)))
    used = np.zeros(len(e), dtype=bool)
    for length, L, cce, rnti, pdu in items:
        assert cce + (1 << L) <= nCCE_tx
        bits = PC.dci_code_bits(length, L, rnti, pdu)
        seg = e[72 * cce:72 * cce + (72 << L)]
        assert np.array_equal(seg > 0, bits == 1) and np.all(seg != 0), (L, cce)      # unscrambled: bit 1 positive
        used[72 * cce:72 * cce + (72 << L)] = True
    assert not e[~used].any()                                                         # <NIL>: amplitude 0
    # the model's search over those soft bits returns what was sent
    st = M.dci_search(e, nCCE_tx, O.get_nCCE(3, fo, 1), CRNTI, SI, RA, sf, PC.tm1_plan(size, 13, size, 31))
    found = [(v[2], v[3], v[0], v[5]) for k, v in sorted(st["alloc"].items()) if k < st["cnt"]]
    assert PC.sent_came_back(items, found) and st["cnt"] == len(items), found
    for _, L, cce, _, _ in items:                          # every transmitted DCI's first CCE is marked taken
        assert (st["maps"][cce >> 5] >> (cce & 31)) & 1


def test_refusals_and_error_values():
    lib = oai.load_library()
    have_gpu = lib.oai4g_init() == 0
    fp = oai.frame_parms(25, 137)
    tab = np.zeros(8 * 800, dtype=np.uint32)
    buf = np.zeros(8 * 800, dtype=np.int8)
    comp = np.zeros(3 * 300, dtype=np.int32)
    plan = (oai.PdcchPlan * 1)(oai.PdcchPlan(0, 0, 27, 4, 2, 2, 0, 0))

    def refused(call, word):
        r = call()
        assert r in (-1, None), word
        assert word in lib.oai4g_last_error(), (word, lib.oai4g_last_error())

    fp4 = oai.frame_parms(25, 137, nb_antennas_tx=2, mode1_flag=0)
    fp4.nb_antennas_tx_eNB = 4
    fp15 = oai.frame_parms(15, 137)
    fpx = oai.frame_parms(25, 137, Ncp=1)
    for f, word in ((fp4, b"4 TX ports"), (fp15, b"no PDCCH geometry"), (fpx, b"normal cyclic prefix")):
        refused(lambda: lib.oai4g_pdcch_soft_bit_table(ctypes.byref(f), 0, 1, oai._ptr(tab), len(tab)), word)
        refused(lambda: lib.oai4g_pdcch_soft_bits(oai._ptr(comp), ctypes.byref(f), 0, 1, oai._ptr(buf)), word)
        refused(lambda: lib.oai4g_pdcch_rx_config_create(ctypes.byref(f), 1, 1, 2, 3, plan, 1), word)
    refused(lambda: lib.oai4g_pdcch_soft_bit_table(ctypes.byref(fp), 0, 4, oai._ptr(tab), len(tab)), b"num_pdcch_symbols 4")
    refused(lambda: lib.oai4g_pdcch_soft_bit_table(ctypes.byref(fp), 10, 1, oai._ptr(tab), len(tab)), b"subframe 10")
    refused(lambda: lib.oai4g_pdcch_candidates(ctypes.byref(fp), 1, 0, 1, 0, 4, None, 0), b"L 4")
    bad_L = (oai.PdcchPlan * 1)(oai.PdcchPlan(0, 4, 27, 4, 2, 2, 0, 0))
    bad_len = (oai.PdcchPlan * 1)(oai.PdcchPlan(0, 0, 46, 8, 2, 2, 0, 0))
    refused(lambda: lib.oai4g_pdcch_rx_config_create(ctypes.byref(fp), 1, 1, 2, 3, bad_L, 1), b"L 4")
    refused(lambda: lib.oai4g_pdcch_rx_config_create(ctypes.byref(fp), 1, 1, 2, 3, bad_len, 1), b"DCI_LENGTH 46")
    st = oai.DciSearchState()
    args = lambda L, bits: (oai._ptr(buf), 1, CRNTI, ctypes.addressof(st.nCCE), 0, 0, ctypes.addressof(st.alloc),
                            ctypes.byref(fp), 1, SI, RA, L, 2, 2, 0, bits, 4, ctypes.addressof(st.cnt),
                            ctypes.addressof(st.f0), ctypes.addressof(st.fc), ctypes.addressof(st.maps[0]),
                            ctypes.addressof(st.maps[1]), ctypes.addressof(st.maps[2]))
    refused(lambda: lib.oai4g_dci_decoding_procedure0(*args(4, 27)), b"L 4")
    refused(lambda: lib.oai4g_dci_decoding_procedure0(*args(0, 46)), b"DCI_LENGTH 46")
    refused(lambda: lib.oai4g_pdcch_rx_batch(None, None, 1, 0, None, None), b"pdcch_rx_batch")
    if not have_gpu:
        assert lib.oai4g_pdcch_soft_bits(oai._ptr(comp), ctypes.byref(fp), 0, 1, oai._ptr(buf)) == -1
        assert lib.oai4g_dci_decoding_procedure0(*args(0, 27)) == -1
        assert not lib.oai4g_pdcch_rx_config_create(ctypes.byref(fp), 1, 1, 2, 3, plan, 1)
        assert st.cnt.value == 0 and not buf.any()
