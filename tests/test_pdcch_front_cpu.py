"""CPU suite of the PDCCH / PCFICH receive front end's model (tests/pdcch_front_model.py) and ABI (no GPU):

  - log2_approx against the reference's own (oracle/_ref/libref_tools.so);
  - the PCFICH REGs and the scrambling against pcfich.c compiled unmodified (oracle/_ref/libref_mod.so): the
    reference's generate_pcfich grid, read as the compensated plane of a unit channel, gives under the model's
    rx_pcfich the count that was sent, with the full correlation 32 * gain on its codeword;
  - the extraction index maps against a direct transcription of the loops of pdcch_extract_rbs_single / _dual
    (dci.c:903-1368, pointer walk by pointer walk) for N_RB 6 / 15 / 25 / 50, the three pilot shifts, symbols 0
    and 1;
  - compensation, MRC and Alamouti on hand-derived vectors, one RE (pair) each, with one saturating and one
    wrapping case (dci.c's front functions have no reference execution: DESIGN section 4);
  - the avgP index mismatch: which planes raise log2_maxh for 1x1, 2x1, 1x2, 2x2;
  - rx_pcfich against the reference's own execution (tests/golden/pcfich_rx_ref.json, made by
    tests/golden/gen_pcfich_ref.py from pcfich.c compiled unmodified): seeded planes with metrics on both sides of
    -16384, the all-below plane, ties, metrics of exactly -16384 and -16383, components of -32768;
  - a plane whose three PCFICH metrics are all below -16384: the answer is 3;
  - the ABI is exported and refuses 4 TX ports, the extended prefix and more than 2 receive antennas.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import openair4g_amd as oai
import pdcch_front_model as F
import pdcch_rx_cases as PC


def test_log2_approx_is_the_reference_one():
    L = O.ref_tools()
    if L is None or not hasattr(L, "log2_approx"):
        pytest.skip("the reference tree was not there when the oracle was built")
    xs = [0, 1, 2, 3, 4, 255, 256, 2 ** 29 - 1, 2 ** 29, 2 ** 30, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 5, 2 ** 32 - 1]
    xs += np.random.default_rng(1).integers(0, 2 ** 32, 200).tolist()
    for x in xs:
        assert F.log2_approx(x) == L.log2_approx(x), x


@pytest.mark.parametrize("N_RB", [6, 15, 25, 50, 100])
@pytest.mark.parametrize("Nid", [0, 1, 2, 137, 503])
def test_pcfich_regs_and_scrambling_against_the_reference(N_RB, Nid):
    if O.ref_mod() is None:
        pytest.skip("the reference tree was not there when the oracle was built")
    fo = O.frame(N_RB, Nid)
    amp = 1024
    gain = (amp * 23170) >> 15
    for sf in (0, 4, 9):
        for cfi in (1, 2, 3):
            grids, reg, _ = O.ref_pcfich(cfi, amp, fo, sf)
            assert reg == F.pcfich_regs(N_RB, Nid)
            comp = PC.grid_to_comp(grids[0], fo, sf, 1)
            m = F.pcfich_metrics(comp, N_RB, Nid, sf)
            assert m[cfi - 1] == 32 * gain and max(m) == m[cfi - 1] and sorted(m)[1] < m[cfi - 1]
            assert F.rx_pcfich(comp, N_RB, Nid, sf) == cfi


def _loops(N_RB, N, fco, nushift, symbol, dual):
    """pdcch_extract_rbs_single (dci.c:926-1116) / _dual (:1138-1366) for one antenna, as written: rxF and dl_ch0
    are running positions (words within the symbol / the estimate row); returns what lands in rxF_ext and
    dl_ch0_ext, in order."""
    n3 = nushift % 3
    rx_ext, ch_ext = [], []
    dl_ch0, rxF = 5, fco

    def whole(rxF, dl_ch0):
        for i in range(12):
            if symbol > 0 or i not in (n3, n3 + 3, n3 + 6, n3 + 9):
                rx_ext.append(rxF + i)
                ch_ext.append(dl_ch0 + i)

    if N_RB & 1 == 0:
        for rb in range(N_RB):
            if rb == N_RB >> 1:
                rxF = 1
            whole(rxF, dl_ch0)
            dl_ch0 += 12
            rxF += 12
    else:
        rb = 0
        while rb < N_RB >> 1:
            whole(rxF, dl_ch0)
            dl_ch0 += 12
            rxF += 12
            rb += 1
        # the middle RB (around DC)
        for i in range(6):
            if symbol > 0 or i not in (n3, n3 + 3):
                ch_ext.append(dl_ch0 + i)
                rx_ext.append(rxF + i)
        rxF = 0
        for i in range(6, 12):
            if symbol > 0 or i not in (n3 + 6, n3 + 9):
                ch_ext.append(dl_ch0 + i)
                # single: rxF[(1 + i - 6)] on every symbol; dual: rxF[(1 + i)] on symbols > 0 (dci.c:1275)
                rx_ext.append(rxF + (1 + i if dual and symbol > 0 else 1 + i - 6))
        dl_ch0 += 12
        rxF += 7
        rb += 1
        while rb < N_RB:
            whole(rxF, dl_ch0)
            dl_ch0 += 12
            rxF += 12
            rb += 1
    return np.array(rx_ext), np.array(ch_ext)


@pytest.mark.parametrize("N_RB", [6, 15, 25, 50])
@pytest.mark.parametrize("Nid", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("dual", [False, True])
def test_extraction_map_equals_the_loops(N_RB, Nid, dual):
    fo = O.frame(N_RB, Nid)
    assert fo.nushift == Nid % 6
    for symbol in (0, 1):
        rx, ch = F.extract_map(N_RB, fo.ofdm_symbol_size, fo.first_carrier_offset, fo.nushift, symbol, dual)
        lrx, lch = _loops(N_RB, fo.ofdm_symbol_size, fo.first_carrier_offset, fo.nushift, symbol, dual)
        assert len(rx) == (8 if symbol == 0 else 12) * N_RB
        assert np.array_equal(rx, lrx) and np.array_equal(ch, lch), (symbol,)
        assert rx.max() < fo.ofdm_symbol_size and ch.max() < fo.ofdm_symbol_size
    # the dual twin's second half of the middle RB differs from the single one exactly at odd sizes, symbols > 0
    a, _ = F.extract_map(N_RB, fo.ofdm_symbol_size, fo.first_carrier_offset, fo.nushift, 1, False)
    b, _ = F.extract_map(N_RB, fo.ofdm_symbol_size, fo.first_carrier_offset, fo.nushift, 1, True)
    assert np.array_equal(a, b) == (N_RB % 2 == 0)


def _w(re, im):
    return np.array([re, im], dtype=np.int16).view(np.int32)


def _ri(word):
    return tuple(int(x) for x in np.asarray(word, dtype=np.int32).reshape(-1).view(np.int16))


def test_compensation_by_hand():
    # h = 3 + 4j, y = 100 - 50j: conj(h) y = (300 - 200) + j(-150 - 400) = 100 - 550j; >> 2 = 25, -138 (floor)
    assert _ri(F.compensate(_w(3, 4), _w(100, -50), 2)) == (25, -138)
    # saturating: h = y = 30000 + 30000j, conj(h) y = 1.8e9 + 0j; >> 6 = 28125000 -> packs gives 32767
    assert _ri(F.compensate(_w(30000, 30000), _w(30000, 30000), 6)) == (32767, 0)
    # and downwards: y = -30000 - 30000j
    assert _ri(F.compensate(_w(30000, 30000), _w(-30000, -30000), 6)) == (-32768, 0)
    # h.im = -32768: sign_epi16 leaves it, so the imaginary part is (-32768) y.re + h.re y.im, not (+32768) y.re
    assert _ri(F.compensate(_w(0, -32768), _w(1, 0), 0)) == (0, -32768)
    # 32-bit wrap of madd: all four factors -32768 give 2^31 -> -2^31; >> 16 = -32768
    assert _ri(F.compensate(_w(-32768, -32768), _w(-32768, -32768), 16))[0] == -32768


def test_mrc_by_hand():
    assert _ri(F.mrc(_w(101, -7), _w(50, -8))) == (75, -8)              # 50 + 25, -4 + -4 (arithmetic shifts)
    # the halves lie in [-16384, 16383]: the saturating add reaches its extremes without clipping anything
    assert _ri(F.mrc(_w(32767, -32768), _w(32767, -32768))) == (32766, -32768)


def test_alamouti_by_hand():
    p0 = np.concatenate([_w(10, 20), _w(30, 40)])
    p2 = np.concatenate([_w(1, 2), _w(3, 4)])
    assert _ri(F.alamouti(p0, p2)) == (10 + 3, 20 - 4, 30 - 1, 40 + 2)
    # wrapping, not saturating: 32767 + 1 = -32768, -32768 - 1 = 32767
    p0 = np.concatenate([_w(32767, -32768), _w(-32768, 32767)])
    p2 = np.concatenate([_w(1, 1), _w(1, 1)])
    assert _ri(F.alamouti(p0, p2)) == (-32768, 32767, 32767, -32768)


class _Fp:
    def __init__(self, fo, nb_tx):
        self.N_RB_DL, self.ofdm_symbol_size, self.first_carrier_offset = fo.N_RB_DL, fo.ofdm_symbol_size, fo.first_carrier_offset
        self.nushift, self.Nid_cell, self.nb_antennas_tx_eNB = fo.nushift, fo.Nid_cell, nb_tx


def _flat(fo, gain):
    """an estimate grid that is `gain` (real) everywhere"""
    g = np.zeros((fo.symbols_per_tti * fo.ofdm_symbol_size, 2), dtype=np.int16)
    g[:, 0] = gain
    return g.reshape(-1).view(np.int32).copy()


@pytest.mark.parametrize("nb_tx,nb_rx,strong,raises", [
    (1, 1, (0, 0), True),
    (2, 1, (0, 0), True), (2, 1, (1, 0), False),      # 2 TX x 1 RX looks at port 0 only
    (1, 2, (0, 0), True), (1, 2, (0, 1), False),      # 1 TX x 2 RX looks at antenna 0 only
    (2, 2, (0, 0), True), (2, 2, (0, 1), True), (2, 2, (1, 0), True), (2, 2, (1, 1), True)])
def test_avgp_index_mismatch(nb_tx, nb_rx, strong, raises):
    fo = O.frame(6, 1)
    fp = _Fp(fo, nb_tx)
    rng = np.random.default_rng(5)
    rx = [rng.integers(-2000, 2000, fo.symbols_per_tti * fo.ofdm_symbol_size * 2).astype(np.int16).view(np.int32)
          for _ in range(nb_rx)]
    est = {(p, a): _flat(fo, 64) for p in range(nb_tx) for a in range(nb_rx)}
    base = F.rx_pdcch_front(fp, rx, est, 0, F.SISO)
    assert base["log2_maxh"] == F.log2_approx(64 * 64) // 2 + 6 + nb_rx - 1
    est[strong] = _flat(fo, 4096)
    got = F.rx_pdcch_front(fp, rx, est, 0, F.SISO)
    assert got["avg"][strong] == 4096 * 4096
    assert (got["log2_maxh"] > base["log2_maxh"]) == raises
    if raises:
        assert got["log2_maxh"] == F.log2_approx(4096 * 4096) // 2 + 6 + nb_rx - 1
    # the level as the reference sums it: four epi32 lanes (RE mod 4) that wrap, added, divided
    h = rng.integers(-32768, 32768, 2 * 72).astype(np.int16)
    lanes = np.zeros(4, dtype=np.uint32)
    sq = (h.astype(np.int64).reshape(-1, 2) ** 2).sum(axis=1)
    for i, v in enumerate(sq):
        lanes[i % 4] = (int(lanes[i % 4]) + int(v)) % 2 ** 32
    tot = int(lanes.astype(np.uint64).sum() % 2 ** 32)
    tot = tot - 2 ** 32 if tot >= 2 ** 31 else tot
    assert F.channel_level(h.view(np.int32), 6) == int(tot / 72)


@pytest.mark.parametrize("N_RB,Nid", [(6, 0), (25, 137)])
def test_pcfich_all_metrics_below_the_start_gives_3(N_RB, Nid):
    for sf in (0, 3, 9):
        comp = F.pcfich_plane_below(N_RB, Nid, sf)
        m = F.pcfich_metrics(comp, N_RB, Nid, sf)
        assert all(x < -16384 for x in m), m
        assert F.rx_pcfich(comp, N_RB, Nid, sf) == 3
    # and the ordinary rule: the first of equal largest metrics wins
    assert F.rx_pcfich(np.zeros(36 * N_RB, np.int32), N_RB, Nid, 0) == 1


def test_rx_pcfich_equals_the_reference_execution():
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcfich_rx_ref.json")))
    assert ref["seed"] == F.PCFICH_SEED
    cases = F.pcfich_cases()
    assert sorted(c[0] for c in cases) == sorted(ref["cases"])
    seen = set()
    for name, N_RB, Nid, sf, plane in cases:
        dig, n = ref["cases"][name]
        assert hashlib.sha256(np.ascontiguousarray(plane, dtype=np.int32).tobytes()).hexdigest()[:16] == dig, name
        assert F.rx_pcfich(plane, N_RB, Nid, sf) == n, (name, F.pcfich_metrics(plane, N_RB, Nid, sf))
        seen.add((name.split("_")[0], n))
    # what the fixture pins: the start value and its strictness, the first of equal maxima, the int16 negation
    assert {("edge16384", 3), ("edge16383", 1), ("tie01", 1), ("tie12", 2), ("below", 3), ("min", 3)} <= seen
    assert {("rand", 1), ("rand", 2), ("rand", 3)} <= seen
    lo = [m for name, N_RB, Nid, sf, pl in cases if name.startswith("rand") for m in F.pcfich_metrics(pl, N_RB, Nid, sf)]
    assert min(lo) < -16384 < max(lo)


NEW = ["oai4g_rx_pdcch_front", "oai4g_rx_pcfich", "oai4g_rx_pdcch", "oai4g_pdcch_front_config_create",
       "oai4g_pdcch_front_config_destroy", "oai4g_pdcch_front_batch", "oai4g_pdcch_rx_batch_detected"]


def test_abi_presence_and_refusals():
    lib = oai.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in oai.exported_symbols()
    header = open(oai.__file__.replace("openair4g_amd/__init__.py", "include/oai4g.h")).read()
    for name in NEW:
        assert name + "(" in header
    fp = oai.frame_parms(25, 137, nb_antennas_tx=2, mode1_flag=0)
    fp4 = oai.frame_parms(25, 137, nb_antennas_tx=2, mode1_flag=0)
    fp4.nb_antennas_tx_eNB = 4
    fpx = oai.frame_parms(25, 137, Ncp=1)
    fp1 = oai.frame_parms(25, 137)
    n = 14 * fp.ofdm_symbol_size
    planes = [np.zeros(n, np.int32) for _ in range(4)]
    rx = (ctypes.c_void_p * 2)(planes[0].ctypes.data, planes[1].ctypes.data)
    ep = (ctypes.c_void_p * 4)(*[p.ctypes.data for p in planes])
    comp = np.zeros(36 * 25, np.int32)
    e = np.zeros(8 * 800, np.int8)

    def refused(call, word):
        r = call()
        assert r in (-1, None), word
        assert word in lib.oai4g_last_error(), (word, lib.oai4g_last_error())

    for f, nrx, mode, word in ((fp4, 1, 1, b"4 TX ports"), (fpx, 1, 0, b"normal cyclic prefix"), (fp, 3, 1, b"3 receive antennas"),
                               (fp, 1, 2, b"mimo_mode 2"), (fp1, 1, 1, b"ALAMOUTI combining needs 2 TX ports")):
        refused(lambda: lib.oai4g_rx_pdcch_front(rx, ep, ctypes.byref(f), nrx, 0, mode, 1, oai._ptr(comp), None, None, None), word)
        refused(lambda: lib.oai4g_pdcch_front_config_create(ctypes.byref(f), nrx, mode, 1, 0, 1), word)
    for f, word in ((fp4, b"4 TX ports"), (fpx, b"normal cyclic prefix")):
        refused(lambda: lib.oai4g_rx_pcfich(ctypes.byref(f), 0, oai._ptr(comp), 0), word)
        refused(lambda: lib.oai4g_rx_pdcch(rx, ep, ctypes.byref(f), 1, 0, 0, 1, oai._ptr(e), None), word)
    refused(lambda: lib.oai4g_rx_pdcch(rx, ep, ctypes.byref(fp), 3, 0, 1, 1, oai._ptr(e), None), b"3 receive antennas")
    refused(lambda: lib.oai4g_rx_pdcch_front(rx, ep, ctypes.byref(fp), 1, 10, 1, 1, oai._ptr(comp), None, None, None), b"bad arguments")
    refused(lambda: lib.oai4g_pdcch_front_batch(None, 1, None, None, None, None, None, None), b"pdcch_front_batch")
    refused(lambda: lib.oai4g_pdcch_rx_batch_detected(None, None, None, 1, 0, 1, None, None), b"pdcch_rx_batch_detected")
    if lib.oai4g_init() != 0:                                             # no device: the error value, nothing written
        assert lib.oai4g_rx_pdcch_front(rx, ep, ctypes.byref(fp), 1, 0, 1, 1, oai._ptr(comp), None, None, None) == -1
        assert lib.oai4g_rx_pcfich(ctypes.byref(fp), 0, oai._ptr(comp), 0) == -1
        assert not comp.any()
