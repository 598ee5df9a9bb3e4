"""CPU suite of the PBCH receive front end's model (tests/pbch_front_model.py) and of the new entry points
without a device:

  - the oracle transmitter's PBCH through a flat channel (exact integers) comes back from the model's rx_pbch as
    the MIB and antenna count sent, for every frame_mod4, one and two ports, N_RB 6 / 15 / 25 / 100, the three
    pilot shifts, one and two receive antennas; the model's pbch_detection returns the frame_mod4 sent and the
    first mode that decodes;
  - the decode over a quarter's 480 soft bits alone, with the Gold words 15 frame_mod4 .., equals the reference's
    decode over the 1920-byte buffer that is 0 elsewhere (what oai4g_pbch_detect_batch relies on);
  - the new entry points exist and, without a device, return -1 / null with a message.
"""
import ctypes

import numpy as np
import pytest

import ctrl_rx_model as M
import openair4g_amd as oai
import oracle_lib as O
import pbch_front_model as B
from test_gpu_pdcch_front import _through

PDU = bytes([0xA4, 0x3C, 0x59])


def _sent(N_RB, Nid, nb_tx, q):
    kw = dict(nb_antennas_tx=2, mode1_flag=0) if nb_tx == 2 else {}
    fo = O.frame(N_RB, Nid, **kw)
    n = 10 * fo.symbols_per_tti * fo.ofdm_symbol_size
    st = O.OrcPbch()
    pdu = np.frombuffer(PDU, np.uint8)
    if q:                                                # frame_mod4 0 encodes, the others map
        assert O.generate_pbch(st, [np.zeros(n, dtype=np.int32) for _ in range(nb_tx)], 512, fo, pdu, 0) == 0
    grids = [np.zeros(n, dtype=np.int32) for _ in range(nb_tx)]
    assert O.generate_pbch(st, grids, 512, fo, pdu, q) == 0
    return fo, grids


@pytest.mark.parametrize("N_RB", [6, 15, 25, 100])
@pytest.mark.parametrize("Nid", [0, 1, 2])
@pytest.mark.parametrize("nb_tx,nb_rx", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_pbch_through_a_flat_channel(N_RB, Nid, nb_tx, nb_rx):
    mode = B.ALAMOUTI if nb_tx == 2 else B.SISO
    for q in range(4):
        fo, grids = _sent(N_RB, Nid, nb_tx, q)
        assert fo.nushift % 3 == Nid
        rx, est = _through(grids, 0, fo, nb_rx)
        f = B.rx_pbch_front(fo, rx, est, nb_tx, mode)
        assert f["defined"].sum() == 48 + 48 + 72 + 72 and np.abs(f["llr"]).min() > 0
        assert B.rx_pbch(fo, rx, est, nb_tx, mode, q) == (nb_tx, PDU)
        assert B.rx_pbch(fo, rx, est, nb_tx, mode, (q + 1) % 4)[0] == -1
        first = next(m for m in (B.SISO, B.ALAMOUTI) if B.rx_pbch(fo, rx, est, nb_tx, m, q)[0] in (1, 2))
        assert B.pbch_detection(fo, rx, est, nb_tx) == (nb_tx, q, first, PDU)
        if nb_tx == 1:                                   # ALAMOUTI with one estimated port equals SISO
            assert first == B.SISO
            assert np.array_equal(B.rx_pbch_front(fo, rx, est, 1, B.ALAMOUTI)["comp"], f["comp"])


def test_a_quarter_alone_decodes_as_the_whole_buffer():
    rng = np.random.default_rng(480)
    hits = 0
    for i in range(24):
        Nid, q = int(rng.integers(0, 504)), i % 4
        if i < 12:
            llr = rng.integers(-8, 8, 480).astype(np.int8)
        else:                                            # an encoded quarter under noise: the CRC path
            amask = (0, 0xFFFF, 0x5555)[i % 3]
            e = M.pbch_encode(PDU, amask, Nid, 1920)[q * 480:(q + 1) * 480].astype(np.int64)
            llr = np.clip(3 * (1 - 2 * e) + rng.integers(-3, 4, 480), -8, 7).astype(np.int8)
        want = M.pbch_decode(B.llr_buffer(llr, q), Nid, q)
        assert B.decode_480(llr, Nid, q) == want
        hits += want[0] > 0
    assert hits == 12


def test_new_entry_points_without_a_device():
    L = oai.load_library()
    names = ["oai4g_rx_pbch_front", "oai4g_rx_pbch", "oai4g_pbch_front_config_create", "oai4g_pbch_front_config_destroy",
             "oai4g_pbch_front_batch", "oai4g_pbch_detect_batch"]
    assert all(hasattr(L, n) for n in names) and set(names) <= set(oai.exported_symbols())
    assert ctypes.sizeof(oai.PbchDetect) == 8
    if L.oai4g_init() == 0:
        return                                           # a device is present: tests/test_gpu_pbch_front.py runs them
    fp = oai.frame_parms(6, 0)
    n = fp.symbols_per_tti * fp.ofdm_symbol_size
    rx, est = [np.zeros(n, dtype=np.int32)], {(0, 0): np.zeros(n, dtype=np.int32)}
    with pytest.raises(oai.OAI4GError):
        oai.rx_pbch_front(fp, rx, est, 1, 0)
    with pytest.raises(oai.OAI4GError):
        oai.rx_pbch(fp, rx, est, 1, 0, 0)
    assert L.oai4g_last_error()
    assert not L.oai4g_pbch_front_config_create(ctypes.byref(fp), 1, 1, 1)
    assert L.oai4g_pbch_front_batch(None, 1, None, None, None, None, None) == -1
    assert L.oai4g_pbch_detect_batch(None, 1, None, None, None) == -1
