"""CPU suite of the UE control decoding path (no GPU):

  - the numpy model (tests/ctrl_rx_model.py) equals the reference's own phy_viterbi_lte_sse2 on every
    case of tests/golden/viterbi_ref.json (tests/golden/gen_viterbi_ref.py), and decodes the payload
    exactly where the fixture records that the reference did;
  - the model's rate-matching receive + deinterleaver equal the reference's own, live, through
    oracle/_ref/libref_rm.so (generate_dummy_w_cc, lte_rate_matching_cc_rx, sub_block_deinterleaving_cc),
    where that library was built;
  - the model's bitwise CRC16 equals the oracle's bytewise one at every DCI length;
  - the exported host plan oai4g_cc_rx_plan equals the model for D = 24..61, and summing through it
    equals a literal restatement of the reference's loops for L = 0..3;
  - every new entry point refuses bad arguments with a message and returns its error value without
    a device.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import ctrl_rx_model as M
import openair4g_amd as oai
import oracle_lib as O
import viterbi_cases as VC

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "viterbi_ref.json")))["cases"]


def test_fixture_covers_every_case():
    names = [c[0] for c in VC.cases()]
    assert sorted(names) == sorted(FIX) and len(names) == len(VC.NS) * len(VC.KINDS)


@pytest.mark.parametrize("n", VC.NS)
def test_model_equals_reference_fixture(n):
    for name, nn, kind, y in VC.cases():
        if nn != n:
            continue
        row = FIX[name]
        assert VC.digest(y) == row["y"], name
        out, start, met = M.viterbi(y, n)
        assert out.tobytes().hex() == row["out"], name
        if "ok" in row:
            assert bool(np.array_equal(out, VC.payload(n)[1])) == row["ok"], name
        if row.get("ok"):
            assert M.crc16(out, n - 16) == M.extract_crc(np.append(out, 0), n - 16), name
        if kind == "zero":     # every step ties: predecessor k + 32 from start state 0, so 0 -> 32 -> ... -> 63 -> 63
            assert start == 0 and not met.any(), name
            assert np.array_equal(out, np.packbits(np.array([1] * (n - 6) + [0] * 6, dtype=np.uint8))), name


def test_clean_and_light_noise_decode():
    """what the reference decodes, by the fixture: every clean codeword and every sigma = 2 one"""
    assert all(FIX[f"{n}_{k}"]["ok"] for n in VC.NS for k in ("clean", "noisy2"))


def _cc_rx_literal(D, E, e):
    """generate_dummy_w_cc + lte_rate_matching_cc_rx + sub_block_deinterleaving_cc, loop by loop"""
    R = (D + 31) >> 5
    Kpi, ND = 32 * R, 32 * R - D
    null = np.zeros(3 * Kpi, dtype=bool)
    k = 0
    for col in range(32):
        if M.BITREV_CC[col] < ND:
            null[[k, Kpi + k, 2 * Kpi + k]] = True
        k += R
    w16 = np.zeros(3 * Kpi, dtype=np.int64)
    ind = 0
    for kk in range(E):
        while null[ind]:
            ind = (ind + 1) % (3 * Kpi)
        w16[ind] += int(e[kk])
        ind = (ind + 1) % (3 * Kpi)
    w = np.clip(w16, -8, 7)
    d = np.zeros(96 + 3 * D, dtype=np.int64)
    k = 0
    for col in range(32):
        index3 = 3 * int(M.BITREV_CC[col])
        for _ in range(R):
            for s in range(3):
                d[96 + index3 - 3 * ND + s] = w[s * Kpi + k]
            index3 += 96
            k += 1
    return d[96:]


@pytest.mark.parametrize("L", range(4))
def test_cc_rx_plan_export_and_sum(L):
    rng = np.random.default_rng(L)
    for D in range(24, 62):
        plan = oai.cc_rx_plan(D)
        assert np.array_equal(plan, M.cc_rx_plan(D)), D
        assert sorted(plan.tolist()) == list(range(3 * D)), D
        e = rng.integers(-128, 128, size=72 << L).astype(np.int8)
        assert np.array_equal(M.cc_rx_d(D, 72 << L, e), _cc_rx_literal(D, 72 << L, e)), (D, L)


@pytest.mark.skipif(O.ref_rm() is None, reason="oracle/_ref/libref_rm.so not built (no reference tree)")
@pytest.mark.parametrize("D,E", [(24, 72), (43, 144), (61, 72), (61, 576), (40, 1920), (40, 1728), (33, 288)])
def test_model_cc_rx_equals_reference_live(D, E):
    L = O.ref_rm()
    rng = np.random.default_rng(D * 4096 + E)
    e = rng.integers(-128, 128, size=E).astype(np.int8)
    R = (D + 31) >> 5
    dummy = np.zeros(3 * 32 * R + 64, dtype=np.uint8)
    L.generate_dummy_w_cc.restype = ctypes.c_uint32
    assert L.generate_dummy_w_cc(ctypes.c_uint32(D), ctypes.c_void_p(dummy.ctypes.data)) == R
    w = np.zeros(3 * 32 * R + 64, dtype=np.int8)
    L.lte_rate_matching_cc_rx(ctypes.c_uint32(R), ctypes.c_uint16(E), ctypes.c_void_p(w.ctypes.data),
                              ctypes.c_void_p(dummy.ctypes.data), ctypes.c_void_p(e.ctypes.data))
    d = np.zeros(96 + 3 * D + 64, dtype=np.int8)
    L.sub_block_deinterleaving_cc(ctypes.c_uint32(D), ctypes.c_void_p(d.ctypes.data + 96), ctypes.c_void_p(w.ctypes.data))
    assert np.array_equal(d[96:96 + 3 * D], M.cc_rx_d(D, E, e))


def test_model_crc16_equals_oracle():
    rng = np.random.default_rng(16)
    for bits in range(8, 46):
        data = rng.integers(0, 256, size=8, dtype=np.uint8)
        assert M.crc16(data, bits) == (O.crc16(data, bits) >> 16), bits


def test_model_pbch_roundtrip():
    """the model decodes what the oracle transmitter's pbch_e carries, for the quarter it was told"""
    fp = O.frame(25, 137, nb_antennas_tx=1)
    st = O.OrcPbch()
    grids = [np.zeros(140 * fp.ofdm_symbol_size, dtype=np.int32)]
    pdu = bytes([0xA4, 0x5C, 0x31])
    O.generate_pbch(st, grids, 512, fp, np.frombuffer(pdu, np.uint8), 0)
    e = np.frombuffer(bytes(st.pbch_e), dtype=np.uint8)[:1920]
    for q in range(4):
        llr = np.zeros(1920, dtype=np.int8)
        llr[q * 480:(q + 1) * 480] = 4 * (1 - 2 * e[q * 480:(q + 1) * 480].astype(np.int8))   # QPSK: bit 1 is -gain
        assert M.pbch_decode(llr, 137, q) == (1, pdu)
        assert M.pbch_decode(llr, 137, (q + 1) & 3)[0] == -1


# ---- the C ABI without a device ----
NEW = {"oai4g_phy_viterbi_lte": 3, "oai4g_diag_viterbi_lte": 5, "oai4g_cc_rx_plan": 2, "oai4g_dci_decoding": 4,
       "oai4g_dci_decoding_crc": 5, "oai4g_pbch_decode": 4, "oai4g_pbch_decode_batch": 6,
       "oai4g_pdcch_soft_bit_table": 5, "oai4g_pdcch_soft_bits": 5, "oai4g_pdcch_candidates": 8,
       "oai4g_dci_decoding_procedure0": 23, "oai4g_pdcch_rx_config_create": 7, "oai4g_pdcch_rx_config_destroy": 1,
       "oai4g_pdcch_rx_candidates": 5, "oai4g_pdcch_rx_batch": 6}
RESTYPE = {"oai4g_pdcch_rx_config_create": ctypes.c_void_p, "oai4g_pdcch_rx_config_destroy": None}


def _declared_args(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(HERE), "include", "oai4g.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name + " is not declared in include/oai4g.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_symbols_are_exported_declared_and_bound():
    lib = oai.load_library()
    for name, nargs in NEW.items():
        assert hasattr(lib, name) and name in oai.exported_symbols(), name
        assert _declared_args(name) == nargs, name
        assert len(getattr(lib, name).argtypes) == nargs, name
        assert getattr(lib, name).restype is RESTYPE.get(name, ctypes.c_int), name


def test_bad_arguments_are_refused_with_a_message():
    lib = oai.load_library()
    y = np.zeros(3 * 600, dtype=np.int8)
    out = np.zeros(128, dtype=np.uint8)
    fp = oai.frame_parms(25, 137)
    for call, word in [
            (lambda: lib.oai4g_phy_viterbi_lte(oai._ptr(y), oai._ptr(out), 0), b"n 0"),
            (lambda: lib.oai4g_phy_viterbi_lte(oai._ptr(y), oai._ptr(out), 513), b"n 513"),
            (lambda: lib.oai4g_dci_decoding(27, 4, oai._ptr(y), oai._ptr(out)), b"aggregation_level 4"),
            (lambda: lib.oai4g_dci_decoding(46, 0, oai._ptr(y), oai._ptr(out)), b"DCI_LENGTH 46"),
            (lambda: lib.oai4g_cc_rx_plan(0, oai._ptr(out)), b"cc_rx_plan"),
            (lambda: lib.oai4g_cc_rx_plan(513, oai._ptr(out)), b"cc_rx_plan"),
            (lambda: lib.oai4g_pbch_decode(oai._ptr(y), ctypes.byref(fp), 4, oai._ptr(out)), b"frame_mod4 4"),
            (lambda: lib.oai4g_pbch_decode_batch(None, 2, ctypes.byref(fp), None, None, None), b"pbch_decode_batch")]:
        assert call() == -1
        assert word in lib.oai4g_last_error(), (word, lib.oai4g_last_error())
    assert not out.any()


def test_entries_return_their_error_value_without_a_device():
    """Checks nothing where a device is present (it returns at once): there the decodes themselves run, in
    tests/test_gpu_ctrl_rx.py.  The PDCCH entry points' error values are in tests/test_pdcch_rx_cpu.py."""
    lib = oai.load_library()
    if lib.oai4g_init() == 0:
        return                                   # a device is present: the decodes themselves are tests/test_gpu_ctrl_rx.py
    y = np.zeros(1920, dtype=np.int8)
    out = np.zeros(64, dtype=np.uint8)
    met = np.zeros(64, dtype=np.uint8)
    st = ctypes.c_uint8()
    fp = oai.frame_parms(25, 137)
    crc = ctypes.c_uint16()
    assert lib.oai4g_phy_viterbi_lte(oai._ptr(y), oai._ptr(out), 40) == -1
    assert lib.oai4g_diag_viterbi_lte(oai._ptr(y), 40, oai._ptr(out), oai._ptr(met), ctypes.byref(st)) == -1
    assert lib.oai4g_dci_decoding(27, 2, oai._ptr(y), oai._ptr(out)) == -1
    assert lib.oai4g_dci_decoding_crc(27, 2, oai._ptr(y), oai._ptr(out), ctypes.byref(crc)) == -1
    assert lib.oai4g_pbch_decode(oai._ptr(y), ctypes.byref(fp), 0, oai._ptr(out)) == -1
    assert lib.oai4g_last_error()                                    # the refusal, not the reference's -1
    assert lib.oai4g_pbch_decode_batch(oai._ptr(y), 1, ctypes.byref(fp), oai._ptr(y), oai._ptr(out), None) == -1
    assert not out.any()
