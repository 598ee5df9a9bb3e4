"""GPU parity of the UE control decoding kernel (oai4g_ctrl_rx.hip: k_cc_decode) through its drop-ins:

  - oai4g_phy_viterbi_lte equals the reference fixture (tests/golden/viterbi_ref.json) and the numpy
    model (tests/ctrl_rx_model.py) on every case: decoded bytes, the 64 final path metrics and the
    traceback's start state; it adds into the caller's buffer; an out-of-range input returns 1 and
    decodes as the model does on the clamped input; n = 512 runs the large-trellis kernel;
  - oai4g_dci_decoding equals the model for D = 24, 43, 61 x L = 0..3 (puncturing at L = 0, up to
    eightfold repetition at L = 3) on noisy codewords and on full-range noise, CRC word included;
  - oai4g_pbch_decode / oai4g_pbch_decode_batch: the transmitter's pbch_e as +-4 soft bits in quarter
    frame_mod4, zeros elsewhere -> MIB and antenna count, 1 and 2 antennas, 1920 and 1728 soft bits;
    the wrong quarter gives -1; one batch mixes 1-, 2- and 4-antenna MIBs, right and wrong quarters, noise.
Where noise is added the assertion is equality with the model; decoding success is asserted exactly
where the fixture records that the reference succeeded.
"""
import json
import os

import numpy as np
import pytest

import ctrl_rx_model as M
import viterbi_cases as VC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "viterbi_ref.json")))["cases"]


@pytest.mark.parametrize("n", VC.NS)
def test_gpu_viterbi_equals_fixture_and_model(gpu, n):
    seen = 0
    for name, nn, kind, y in VC.cases():
        if nn != n:
            continue
        seen += 1
        clamped, out, met, start = gpu.viterbi_lte_state(y, n)
        mo, ms, mm = M.viterbi(y, n)
        assert clamped == 0, name
        assert out.tobytes().hex() == FIX[name]["out"], name
        assert np.array_equal(out, mo) and start == ms and np.array_equal(met, mm), name
        if FIX[name].get("ok"):
            assert np.array_equal(out, VC.payload(n)[1]), name
        acc = np.full((n + 7) >> 3, 0x11, dtype=np.uint8)          # the drop-in adds, as the reference does
        r, acc = gpu.viterbi_lte(y, n, acc)
        assert r == 0 and np.array_equal(acc, (mo.astype(np.int32) + 0x11).astype(np.uint8)), name
    assert seen == len(VC.KINDS)


def test_gpu_viterbi_clamps_out_of_range_input(gpu):
    rng = np.random.default_rng(5)
    for n in (24, 61):
        y = rng.integers(-128, 128, size=3 * n).astype(np.int8)
        assert y.min() < -8 and y.max() > 7
        clamped, out, met, start = gpu.viterbi_lte_state(y, n)
        mo, ms, mm = M.viterbi(M.clamp(y), n)
        assert clamped == 1
        assert np.array_equal(out, mo) and start == ms and np.array_equal(met, mm)
        assert gpu.viterbi_lte(y, n)[0] == 1 and gpu.viterbi_lte(M.clamp(y).astype(np.int8), n)[0] == 0


@pytest.mark.parametrize("n", [65, 200, 512])
def test_gpu_viterbi_large_trellis(gpu, n):
    """n > 64 takes the 512-step instance of the kernel"""
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 2, size=n, dtype=np.uint8)
    y = np.clip(np.rint(7.0 * (2.0 * M.tbcc_encode(bits) - 1.0) + rng.normal(0, 4.0, 3 * n)), -8, 7).astype(np.int8)
    for yy in (y, rng.integers(-8, 8, size=3 * n).astype(np.int8)):
        clamped, out, met, start = gpu.viterbi_lte_state(yy, n)
        mo, ms, mm = M.viterbi(yy, n)
        assert clamped == 0 and np.array_equal(out, mo) and start == ms and np.array_equal(met, mm)


def _dci_e(D, L, rng, sigma):
    """the rate-matched soft bits of a seeded DCI of D - 16 bits at aggregation level L, as they reach
    dci_decoding: unscrambled, bit 1 positive"""
    bits, _ = VC.payload(D)
    d = M.tbcc_encode(bits)
    plan = M.cc_rx_plan(D).astype(np.int64)
    inv = np.zeros(3 * D, dtype=np.int64)
    inv[plan] = np.arange(3 * D)                     # e index (mod 3 D) -> d position
    E = 72 << L
    e = 2.0 * d[inv[np.arange(E) % (3 * D)]] - 1.0
    return np.clip(np.rint(20.0 * e + rng.normal(0, sigma, E)), -128, 127).astype(np.int8)


@pytest.mark.parametrize("D", [24, 43, 61])
@pytest.mark.parametrize("L", range(4))
def test_gpu_dci_decoding_equals_model(gpu, D, L):
    rng = np.random.default_rng(D * 8 + L)
    cases = [_dci_e(D, L, rng, 0.0), _dci_e(D, L, rng, 12.0), _dci_e(D, L, rng, 40.0),
             rng.integers(-128, 128, size=72 << L).astype(np.int8), rng.integers(-3, 4, size=72 << L).astype(np.int8)]
    for i, e in enumerate(cases):
        out, crc = gpu.dci_decoding(D - 16, L, e)
        mo, mc = M.dci_decoding(D - 16, L, e)
        assert len(out) == 2 + (D >> 3)
        assert np.array_equal(out, mo) and crc == mc, (D, L, i)
    if 72 << L >= 3 * D:                             # nothing punctured: the clean codeword comes back, CRC ^ RNTI 0 = 0
        out, crc = gpu.dci_decoding(D - 16, L, cases[0])
        assert np.array_equal(out[:(D + 7) >> 3], VC.payload(D)[1]) and crc == 0 and not out[(D + 7) >> 3:].any()


def _pbch_llr(gpu, n_ant, Ncp, Nid, pdu, q):
    """oai4g_generate_pbch's pbch_e as +-4 soft bits (bit 1 is -gain) in quarter q, zeros elsewhere"""
    fp = gpu.frame_parms(25, Nid, Ncp=Ncp, nb_antennas_tx=n_ant, mode1_flag=1 if n_ant == 1 else 0)
    fp.nb_antennas_tx_eNB = n_ant
    st = gpu.Pbch()
    grids = [np.zeros(10 * fp.symbols_per_tti * fp.ofdm_symbol_size, dtype=np.int32) for _ in range(n_ant)]
    gpu.generate_pbch(st, grids, 512, fp, np.frombuffer(pdu, np.uint8), 0)
    E = 1920 if Ncp == 0 else 1728
    e = np.frombuffer(bytes(st.pbch_e), dtype=np.uint8)[:E].astype(np.int8)
    llr = np.zeros(E, dtype=np.int8)
    llr[q * (E >> 2):(q + 1) * (E >> 2)] = 4 * (1 - 2 * e[q * (E >> 2):(q + 1) * (E >> 2)])
    return fp, llr


PBCH = [(1, 0, 137, bytes([0xA4, 0x5C, 0x31])), (2, 0, 137, bytes([0x00, 0xFF, 0x80])),
        (1, 1, 22, bytes([0x12, 0x34, 0x56])), (2, 1, 503, bytes([0xE1, 0x00, 0x07]))]


@pytest.mark.parametrize("n_ant,Ncp,Nid,pdu", PBCH)
def test_gpu_pbch_decode(gpu, n_ant, Ncp, Nid, pdu):
    rng = np.random.default_rng(Nid)
    for q in range(4):
        fp, llr = _pbch_llr(gpu, n_ant, Ncp, Nid, pdu, q)
        assert gpu.pbch_decode(llr, fp, q) == (n_ant, pdu) == M.pbch_decode(llr, Nid, q)
        wrong = gpu.pbch_decode(llr, fp, (q + 1) & 3)
        assert wrong[0] == -1 and wrong == M.pbch_decode(llr, Nid, (q + 1) & 3)
        noisy = np.clip(llr.astype(np.int32) + rng.integers(-128, 128, size=len(llr)), -128, 127).astype(np.int8)
        assert gpu.pbch_decode(noisy, fp, q) == M.pbch_decode(noisy, Nid, q)     # every soft bit is read


@pytest.mark.parametrize("Ncp", [0, 1])
def test_gpu_pbch_decode_batch(gpu, Ncp):
    """8 decodes of one cell in one launch.  The antenna count is in the data (the CRC mask), so 1-, 2- and
    4-antenna MIBs share the batch: right and wrong quarters, clean, noisy and pure noise.  The 1- and
    2-antenna items are oai4g_generate_pbch's pbch_e; the transmitter has no 4-antenna PBCH, so that item's
    pbch_e is the model encoder's with the 0x5555 mask (checked against the transmitter's for 1 and 2)."""
    Nid = 137 + Ncp
    E = 1920 if Ncp == 0 else 1728
    pdus = {1: bytes([0x5A, 0xC3, 0x0F]), 2: bytes([0x81, 0x7E, 0xA0]), 4: bytes([0x33, 0x0C, 0xF1])}
    rng = np.random.default_rng(Nid)
    for n_ant, mask in ((1, 0), (2, 0xFFFF)):                    # the model encoder is the transmitter's
        _, llr = _pbch_llr(gpu, n_ant, Ncp, Nid, pdus[n_ant], 0)
        e = M.pbch_encode(pdus[n_ant], mask, Nid, E)
        assert np.array_equal(llr[:E >> 2], 4 * (1 - 2 * e[:E >> 2].astype(np.int8)))

    def item(n_ant, q):
        if n_ant < 4:
            return _pbch_llr(gpu, n_ant, Ncp, Nid, pdus[n_ant], q)[1]
        e = M.pbch_encode(pdus[4], 0x5555, Nid, E).astype(np.int8)
        llr = np.zeros(E, dtype=np.int8)
        llr[q * (E >> 2):(q + 1) * (E >> 2)] = 4 * (1 - 2 * e[q * (E >> 2):(q + 1) * (E >> 2)])
        return llr

    def noisy(llr):
        return np.clip(llr.astype(np.int32) + rng.integers(-128, 128, size=E), -128, 127).astype(np.int8)
    # (antennas, quarter sent, quarter told, noise)
    spec = [(1, 0, 0, False), (2, 1, 1, False), (2, 2, 3, False), (1, 3, 3, False),
            (4, 0, 0, False), (2, 1, 1, True), (1, 2, 3, True), (4, 3, 3, False)]
    llrs = [noisy(item(a, q)) if nz else item(a, q) for a, q, _, nz in spec]
    qs = [t for _, _, t, _ in spec]
    llrs.append(rng.integers(-128, 128, size=E).astype(np.int8))          # a ninth decode: pure noise
    qs.append(2)
    fp = gpu.frame_parms(25, Nid, Ncp=Ncp)
    b = gpu.PbchDecodeBatch(fp, len(llrs))
    b.upload(np.stack(llrs), qs)
    b.launch()
    cnt, mib = b.results()
    b.close()
    for i in range(len(llrs)):
        assert (int(cnt[i]), bytes(mib[i])) == M.pbch_decode(llrs[i], Nid, qs[i]), i
        assert (int(cnt[i]), bytes(mib[i])) == gpu.pbch_decode(llrs[i], fp, qs[i]), i
    for i, (a, q, t, nz) in enumerate(spec):
        if not nz:
            assert int(cnt[i]) == (a if q == t else -1), i
            assert q != t or bytes(mib[i]) == pdus[a], i
