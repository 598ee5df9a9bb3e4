"""CPU suite of PHICH reception's model (tests/phich_rx_model.py) and of the new entry points without a device:

  - the oracle transmitter's PHICH, every sequence, two groups, HI 0 and 1, one port, N_RB 6 / 25, through the flat
    channel and the model's PDCCH front, is detected as sent (HI 1 = ACK, HI 0 = NACK);
  - with two ports the reference's pdcch_alamouti + rx_phich recover the HI in the groups of both parities: with
    the normal prefix the reference's transmit mapping (phich.c:696-760) is the same Alamouti pair order in every
    group (its only `ngroup_PHICH & 1` switch, :773, is the extended prefix's), which is the order pdcch_alamouti
    undoes;
  - the new entry points exist and, without a device, return -1 / null with a message.
"""
import ctypes

import numpy as np
import pytest

import openair4g_amd as oai
import oracle_lib as O
import pdcch_front_model as F
import phich_rx_model as P
from test_gpu_pdcch_front import _through


def _frame(N_RB, Nid, nb_tx):
    kw = dict(nb_antennas_tx=2, mode1_flag=0) if nb_tx == 2 else {}
    fo = O.frame(N_RB, Nid, **kw)
    if N_RB == 6:
        fo.phich_resource = 12                           # Ng = 2: two groups at 6 PRB
    return fo


def _received(fo, nb_tx, sf, g, q, hi, nb_rx=1):
    grids = [np.zeros(10 * fo.symbols_per_tti * fo.ofdm_symbol_size, dtype=np.int32) for _ in range(nb_tx)]
    assert O.generate_phich(fo, 512, q, g, hi, sf, grids) == 0
    rx, est = _through(grids, sf, fo, nb_rx)
    return F.rx_pdcch_front(fo, rx, est, sf, F.ALAMOUTI if nb_tx == 2 else F.SISO)["comp"]


@pytest.mark.parametrize("N_RB", [6, 25])
def test_phich_detected_as_sent(N_RB):
    fo = _frame(N_RB, 1, 1)
    regs = O.phich_reg_mapping(fo)
    assert len(regs) >= 2
    for sf in (0, 7):
        for g in (0, len(regs) - 1):
            for q in range(8):
                for hi in (0, 1):
                    comp = _received(fo, 1, sf, g, q, hi)
                    nack, hi16, exact = P.rx_phich(comp, regs, g, q, fo.Nid_cell, sf)
                    assert hi16 == exact and abs(hi16) >= 24            # at least one unit in each of the 24 terms
                    assert nack == 1 - hi, (sf, g, q, hi, hi16)
                    other = P.rx_phich(comp, regs, g, q ^ 1, fo.Nid_cell, sf)     # an orthogonal sequence sees nothing
                    assert abs(other[1]) < abs(hi16) // 8


def test_phich_two_ports_every_group_parity():
    fo = _frame(25, 2, 2)
    regs = O.phich_reg_mapping(fo)
    assert len(regs) == 4
    for g in range(4):
        got = []
        for q in range(8):
            for hi in (0, 1):
                comp = _received(fo, 2, 3, g, q, hi, nb_rx=2)
                got.append(P.rx_phich(comp, regs, g, q, fo.Nid_cell, 3)[0] == 1 - hi)
        assert all(got), (g, got)


def test_new_entry_points_without_a_device():
    L = oai.load_library()
    names = ["oai4g_rx_phich", "oai4g_phich_rx_config_create", "oai4g_phich_rx_config_destroy", "oai4g_phich_rx_batch"]
    assert all(hasattr(L, n) for n in names) and set(names) <= set(oai.exported_symbols())
    assert ctypes.sizeof(oai.PhichRxItem) == 8 and ctypes.sizeof(oai.PhichRxOut) == 4
    if L.oai4g_init() == 0:
        return                                           # a device is present: tests/test_gpu_phich_rx.py runs them
    fp = oai.frame_parms(25, 1)
    with pytest.raises(oai.OAI4GError):
        oai.rx_phich(fp, 0, np.zeros(8 * 25, dtype=np.int32), 0, 0)
    assert L.oai4g_last_error()
    assert not L.oai4g_phich_rx_config_create(ctypes.byref(fp), 0, 1)
    assert L.oai4g_phich_rx_batch(None, None, 1, None, 1, None, None) == -1
