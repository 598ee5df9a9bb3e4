"""GPU tests of the PBCH receive front end (k_pbch_front) and the detection behind it
(oai4g_pbch_detect_batch), against tests/pbch_front_model.py:

  - the drop-in oai4g_rx_pbch_front bit-exact on every defined word (plane 0, the four planes before MRC,
    log2_maxh[4], the 480 soft bits; the undefined words are 0): N_RB 6 / 15 / 25 with the three pilot shifts,
    (ports, RX) in 1x1, 2x1, 1x2, 2x2, both high_speed_flag values, both modes (ALAMOUTI also with one port), a
    different gain per plane: a strong port 1 raises log2_maxh (all planes are looked at), and log2_maxh differs
    between a pilot symbol and a data symbol (the / 72 over 48 words);
  - saturation and wrap at 6 PRB, 1x2 SISO and 2x2 ALAMOUTI: small estimates keep the level low while a few REs
    carry full-scale estimates whose |h|^2 sum to a multiple of 2^32 and so leave the level alone; packs_epi32
    saturates, the MRC reaches 32766 / -32768, the Alamouti sums wrap, h = y = -32768 - 32768j and h = -32768j are
    there, and on one symbol one plane's sum wraps negative and is ignored by the maximum.  Each is asserted from
    the model before the comparison;
  - batch = drop-in over 8 subframes, 25 PRB, 2x2, with log2_maxh differing across the batch;
  - the closed loop from IQ: batch transmitter with PBCH and CRS -> oai4g_fep_batch -> oai4g_chest_batch ->
    oai4g_pbch_front_batch -> oai4g_pbch_detect_batch returns the MIB, the antenna count and frame_mod4 0..3 in
    one batch, the mode the model finds on the same estimates, and none for a subframe without PBCH;
  - the detection's order on built soft bits: the earlier of two passing hypotheses, and a hit naming 4 antennas
    does not stop the search;
  - refusals return -1 with a message.
"""
import ctypes

import numpy as np
import pytest

import ctrl_rx_model as M
import oracle_lib as O
import pbch_front_model as B
from test_gpu_pdcch_front import GAIN, RB_ALLOC, _c16, _frames, _upload

pytestmark = pytest.mark.gpu

LO = int(np.array([-32768, -32768], dtype=np.int16).view(np.int32)[0])
MJ = int(np.array([0, -32768], dtype=np.int16).view(np.int32)[0])


def _same(got, want):
    comp, l2, llr, planes = got
    d = want["defined"]
    assert l2.tolist() == want["log2_maxh"]
    assert np.array_equal(comp, want["comp"]) and not comp[~d].any()
    for (p, a), pl in want["planes"].items():
        assert np.array_equal(planes[2 * p + a], pl), (p, a)
    absent = [i for i in range(4) if (i >> 1, i & 1) not in want["planes"]]
    assert not planes[absent].any()
    assert np.array_equal(llr, want["llr"])


@pytest.mark.parametrize("N_RB,Nid", [(6, 0), (15, 1), (25, 2)])
@pytest.mark.parametrize("nb_tx,nb_rx", [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("hs", [0, 1])
def test_gpu_pbch_front_drop_in_equals_model(gpu, N_RB, Nid, nb_tx, nb_rx, hs):
    fo, fg = _frames(gpu, N_RB, Nid, nb_tx)
    assert fo.nushift % 3 == Nid
    n = fo.symbols_per_tti * fo.ofdm_symbol_size
    rng = np.random.default_rng(N_RB * 64 + nb_tx * 8 + nb_rx * 2 + hs)
    rx = [_c16(rng, n, 3000) for _ in range(nb_rx)]
    est = {(p, a): _c16(rng, n, GAIN[(p, a)]) for p in range(nb_tx) for a in range(nb_rx)}
    for mode in (B.SISO, B.ALAMOUTI):
        want = B.rx_pbch_front(fo, rx, est, nb_tx, mode, hs)
        assert all(0 < 72 * v < 2 ** 29 for avg in want["avg"] for v in avg.values())   # the level's sum stays defined
        if nb_tx == 2:
            for sm in range(4):                            # the strong port 1 is looked at
                assert want["log2_maxh"][sm] > 3 + B.log2_approx(want["avg"][sm][(0, 0)]) // 2
            if hs == 0:                                    # one estimate row for all four symbols: 48 words over 72
                assert want["log2_maxh"][0] == want["log2_maxh"][1] < want["log2_maxh"][2] == want["log2_maxh"][3]
        assert {-8, 7} <= set(want["llr"].tolist()) and ((want["llr"] > -8) & (want["llr"] < 7)).any()
        _same(gpu.rx_pbch_front(fg, rx, est, nb_tx, mode, hs, diag=True), want)


@pytest.mark.parametrize("nb_tx,nb_rx,mode", [(1, 2, B.SISO), (2, 2, B.ALAMOUTI)])
def test_gpu_pbch_front_saturation_and_wrap(gpu, nb_tx, nb_rx, mode):
    N_RB, Nid = 6, 4
    fo, fg = _frames(gpu, N_RB, Nid, nb_tx)
    N, n = fo.ofdm_symbol_size, fo.symbols_per_tti * fo.ofdm_symbol_size
    rng = np.random.default_rng(91 + nb_tx)
    rx = [_c16(rng, n, 32767) for _ in range(nb_rx)]
    est = {(p, a): _c16(rng, n, 16) for p in range(nb_tx) for a in range(nb_rx)}
    # symbol 9 (symbol_mod 2), on every plane: words 10, 11 h = y = -32768 - 32768j (both dot products are 2^31 and
    # wrap to -2^31); words 20, 21 h = -32768 - 32768j, y = -20000 - 10000j (a large positive real part); words
    # 30..33 h = -32768j, y = 1 (the int16 negation of h.im stays -32768).  Four |h|^2 of 2^31 and four of 2^30 add a
    # multiple of 2^32 to the level's sum: the level is that of the small estimates
    rxw, chw = B.extract_map(N_RB, N, fo.nushift, 2)
    yp = int(np.array([-20000, -10000], dtype=np.int16).view(np.int32)[0])
    for a in range(nb_rx):
        for w, y in ((10, LO), (11, LO), (20, yp), (21, yp), (30, 1), (31, 1), (32, 1), (33, 1)):
            rx[a][9 * N + rxw[w]] = y
            for p in range(nb_tx):
                est[(p, a)][9 * N + chw[w]] = MJ if w >= 30 else LO
    # symbol 10: one 2^31 on the last plane alone: its sum is negative and the maximum passes it by
    last = (nb_tx - 1, 1)
    est[last][10 * N + B.extract_map(N_RB, N, fo.nushift, 3)[1][5]] = LO
    want = B.rx_pbch_front(fo, rx, est, nb_tx, mode, 1)
    avg, l2 = want["avg"], want["log2_maxh"]
    assert all(0 < v < 16 * 16 * 2 for v in avg[2].values()) and l2[2] <= 7
    assert avg[3][last] < 0 and l2[3] == 3 + B.log2_approx(max(v for k, v in avg[3].items() if k != last)) // 2
    for v in want["planes"].values():
        c = v[2 * 72:3 * 72].view(np.int16).reshape(-1, 2)
        assert c[10].tolist() == [-32768, -32768] and c[20].tolist()[0] == 32767      # packs_epi32 saturates both ways
        assert c[30].tolist() == [0, -32768 >> l2[2]]
    comb = [want["comb"][p][2 * 72:3 * 72].view(np.int16) for p in range(nb_tx)]
    assert all((v == 32766).any() and (v == -32768).any() for v in comb)         # all the MRC's adds can reach
    assert (want["unwrapped"] > 32768) == (mode == B.ALAMOUTI)                     # the Alamouti sums wrap
    _same(gpu.rx_pbch_front(fg, rx, est, nb_tx, mode, 1, diag=True), want)


def test_gpu_pbch_front_batch_equals_drop_in(gpu):
    N_RB, Nid, n_sf = 25, 137, 8
    fo, fg = _frames(gpu, N_RB, Nid, 2)
    n = fo.symbols_per_tti * fo.ofdm_symbol_size
    rng = np.random.default_rng(18)
    rx = np.stack([[_c16(rng, n, 3000) for _ in range(2)] for _ in range(n_sf)])          # [n_sf][2][n]
    est = {(p, a): np.stack([_c16(rng, n, GAIN[(p, a)] * (1 + i % 3)) for i in range(n_sf)]) for p in (0, 1) for a in (0, 1)}
    fb = gpu.PbchFrontBatch(fg, n_sf, 2, 2)
    d_rx = _upload(gpu, rx)
    try:
        fb.upload_estimates(est)
        fb.launch(d_rx)
        llr, l2 = fb.results()
    finally:
        fb.close()
        gpu.lib().oai4g_dev_free(ctypes.c_void_p(d_rx))
    for i in range(n_sf):
        e = {k: v[i] for k, v in est.items()}
        for mode in (B.SISO, B.ALAMOUTI):
            _, l1, b1 = gpu.rx_pbch_front(fg, list(rx[i]), e, 2, mode)
            assert np.array_equal(llr[i, mode], b1) and l2[i].tolist() == l1.tolist(), (i, mode)
            want = B.rx_pbch_front(fo, list(rx[i]), e, 2, mode)
            assert np.array_equal(llr[i, mode], want["llr"]) and l2[i].tolist() == want["log2_maxh"]
    assert len({tuple(r) for r in l2.tolist()}) > 1


@pytest.mark.parametrize("N_RB,tm2,nb_rx", [(6, False, 1), (6, True, 1), (25, False, 2), (25, True, 2)])
def test_gpu_pbch_closed_loop_from_iq(gpu, N_RB, tm2, nb_rx):
    Nid, n_sf = 137, 5
    nb_tx = 2 if tm2 else 1
    fo, fg = _frames(gpu, N_RB, Nid, nb_tx)
    rng = np.random.default_rng(N_RB + nb_tx)
    pdu = rng.integers(0, 256, 3, dtype=np.uint8)
    iq = np.zeros((n_sf + 1, nb_rx, fg.samples_per_tti), dtype=np.int32)
    for i in range(n_sf):                                  # frame_mod4 0..3, and a subframe 0 without PBCH
        p = gpu.make_params("TM2S" if tm2 else "C1", subframe=0, subframe_step=0, Nid_cell=Nid, with_crs=1, N_RB_DL=N_RB,
                            rb_alloc=RB_ALLOC[N_RB], nb_rb=N_RB)
        pipe = gpu.TxPipeline(p, 1)
        if i < 4:
            pipe.set_common(pbch_pdu=pdu, frame_mod4=i)
        pipe.upload_payload(rng.integers(0, 256, size=(1, 1, p.payload_stride), dtype=np.uint8))
        pipe.run()
        pipe.sync()
        t16 = pipe.iq()[0].view(np.int16).astype(np.int64)                 # [nb_tx][2 spt]
        pipe.close()
        for a in range(nb_rx):                                             # H = [1 1] / [1 -1] over the ports
            s = t16[0] + (t16[1] if a == 0 else -t16[1]) if tm2 else t16[0]
            iq[i, a] = np.clip(s, -32768, 32767).astype(np.int16).view(np.int32)
    fep = gpu.FepBatch(fg, n_sf + 1, nb_rx)
    fb = gpu.PbchFrontBatch(fg, n_sf, nb_rx, nb_tx, 1, first_subframe=0, subframe_step=0)
    try:
        fep.upload(iq)
        fep.run()
        fb.estimate(fep.d_rxF)
        fb.launch(fep.d_rxF)
        fb.detect()
        det = fb.detected()
        rxF = fep.result().reshape(n_sf + 1, nb_rx, -1)
        est = fb.estimates()
        llr, _ = fb.results()
    finally:
        fb.close()
        fep.close()
    for i in range(n_sf):
        d = det[i]
        e = {k: v[i] for k, v in est.items()}
        rows = [B.rx_pbch_front(fo, list(rxF[i]), e, nb_tx, mode)["llr"] for mode in (B.SISO, B.ALAMOUTI)]
        assert np.array_equal(llr[i, 0], rows[0]) and np.array_equal(llr[i, 1], rows[1])
        want = B.detect_rows(rows, Nid)
        if i == 4:
            assert want is None and d.tx_ant == 0xFF
            continue
        assert want is not None and want[:2] == (nb_tx, i) and want[3] == bytes(pdu)
        assert (d.tx_ant, d.frame_mod4, d.mimo_mode, bytes(d.mib)) == want, i


def test_gpu_pbch_detection_order(gpu):
    Nid = 77
    _, fg = _frames(gpu, 25, Nid, 1)
    mib = bytes([0x5A, 0xC3, 0x0F])

    def quarter(q, amask):
        e = M.pbch_encode(mib, amask, Nid, 1920)[q * 480:(q + 1) * 480].astype(np.int64)
        return (4 * (1 - 2 * e)).astype(np.int8)

    rng = np.random.default_rng(5)
    rows = np.stack([
        [quarter(2, 0), quarter(1, 0xFFFF)],               # (1, ALAMOUTI) comes before (2, SISO)
        [quarter(3, 0x5555), quarter(3, 0xFFFF)],          # (3, SISO) names 4 antennas: the search goes on
        [quarter(0, 0xFFFF), quarter(0, 0)],               # the same quarter in both rows: SISO first
        rng.integers(-8, 8, (2, 480)).astype(np.int8)])
    want = [B.detect_rows(r, Nid) for r in rows]
    assert want == [(2, 1, B.ALAMOUTI, mib), (2, 3, B.ALAMOUTI, mib), (2, 0, B.SISO, mib), None]
    assert B.decode_480(rows[1, 0], Nid, 3)[0] == 4 and B.decode_480(rows[0, 0], Nid, 2)[0] == 1
    fb = gpu.PbchFrontBatch(fg, len(rows), 1, 1)
    try:
        fb.upload_llr(rows)
        fb.detect()
        det = fb.detected()
    finally:
        fb.close()
    for d, w in zip(det, want):
        if w is None:
            assert d.tx_ant == 0xFF
        else:
            assert (d.tx_ant, d.frame_mod4, d.mimo_mode, bytes(d.mib)) == w


def test_gpu_pbch_front_refusals(gpu):
    fg = gpu.frame_parms(25, 1)
    n = fg.symbols_per_tti * fg.ofdm_symbol_size
    z = np.zeros(n, dtype=np.int32)
    est = {(p, a): z for p in range(2) for a in range(2)}

    def refused(call, *words):
        with pytest.raises(gpu.OAI4GError) as ei:
            call()
        assert all(w in str(ei.value) for w in words), str(ei.value)

    ext = gpu.frame_parms(25, 1, Ncp=1)
    refused(lambda: gpu.rx_pbch_front(ext, [z], est, 1, B.SISO), "prefix")
    refused(lambda: gpu.rx_pbch_front(fg, [z], est, 4, B.SISO), "4", "ports")
    refused(lambda: gpu.rx_pbch_front(fg, [z, z, z], est, 1, B.SISO), "3 receive antennas")
    refused(lambda: gpu.rx_pbch_front(fg, [z], est, 1, 2), "mimo_mode 2")
    refused(lambda: gpu.rx_pbch(fg, [z], est, 1, B.SISO, 4), "frame_mod4 4")
    assert not gpu.lib().oai4g_pbch_front_config_create(ctypes.byref(ext), 1, 1, 1)
    assert gpu.lib().oai4g_last_error()
    # and an accepted call, ALAMOUTI with one estimated port, on zeros: what the model decodes from zeros
    assert gpu.rx_pbch(fg, [z], est, 1, B.ALAMOUTI, 0) == M.pbch_decode(np.zeros(1920, dtype=np.int8), 1, 0)
