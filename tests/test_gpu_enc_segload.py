"""k_encode loads the payload straight into the systematic streams, runs both CRCs on the stream
words and splices the CRC bytes in afterwards (phases 0-1).  The sizes below are
the smallest that reach each branch of that: the byte-exact path of block 0's filler and of every
block's last payload word, the single-word tail, every lanes-per-block setting of the CRC pass and
both block sizes of a mixed segmentation.  C3's shape (two codewords, G = 86 400 bits each, 83 952
at subframe index 0) with TBS overridden; every payload row is 0xFF past TBS/8, so that a missing
mask shows in the e bits, which are compared bit for bit with the oracle chain.

Kmimo = 2 halves the soft buffer, so from C = 7 on the reference's rate matcher refuses the block
(C Kw > Nir, lte_rate_matching.c:518-521).  Those launches run with rm_limited_buffer = 1 against the
oracle's 36.212 5.1.4.1.2 rate matcher, as tests/test_gpu_rm_limited.py does; phases 0-1 are the same."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import enc_sweep_cases as S

pytestmark = pytest.mark.gpu

N_SF = 4
# (C, TBS): geometry from include/oai4g_qpp.c and lte_segmentation.c
CASES = [
    (1, 16),       # K = 40: 32 does not divide K, A mod 4 = 2
    (1, 40),       # K = 64: single-word tail
    (1, 1008),     # F = 24: filler
    (1, 6096),     # K = 6144, F = 24: filler in the largest block
    (1, 6120),     # F = 0, A mod 4 = 1
    (2, 6128),     # 3072 + 3136, F = 8: the smallest multi-block TB, mixed sizes
    (3, 12232),    # F = 24, A mod 4 = 1
    (3, 12960),    # F = 0, A mod 4 = 0
    (4, 18360),    # 3 x 4608 + 4672, F = 16: last C with 64 lanes per block
    (5, 24504),    # F = 56: 32 lanes per block
    (5, 25456),    # 5 x 5120, F = 0: 32-fold QPP behind it
    (8, 48936),    # 8 x 6144: last C with 32 lanes per block
    (9, 49000),    # 4 x 5440 + 5 x 5504, F = 40: 16 lanes per block, mixed sizes
    (13, 73728),   # 12 x 5696 + 5760, F = 48, A mod 4 = 0
    (13, 75376),   # 13 x 5824: the largest TB
]
# codeword 1 takes the list backwards: 14 of the 15 launches have two different sizes, and the row
# stride comes from the larger
PAIRS = [(CASES[i][1], CASES[len(CASES) - 1 - i][1]) for i in range(len(CASES))]


def test_case_geometry():
    for C, tbs in CASES:
        assert S.seg_params(tbs + 24)[0] == C, tbs


def _limited(tbs):
    """a codeword whose blocks do not fit the halved soft buffer (the reference emits E = 0)"""
    segs = [S.seg_params(t + 24) for t in tbs]
    return any(C * S.Ncb(Kp) > S.NIR_KMIMO2 for C, _, Kp, _, _ in segs)


def _params(gpu, tbs):
    p = gpu.make_params("C3", subframe=0, subframe_step=1, TBS=tbs)
    p.rm_limited_buffer = 1 if _limited(tbs) else 0
    return p


def _payload(p, tbs, seed):
    pay = np.random.default_rng(seed).integers(0, 256, size=(N_SF, p.n_cw, p.payload_stride), dtype=np.uint8)
    for cw in range(p.n_cw):
        pay[:, cw, tbs[cw] // 8:] = 0xFF
    return pay


def _check_ebits(gpu, p, pipe, pay, eb, tag):
    O.set_rm_limited(bool(p.rm_limited_buffer))
    try:
        for i in range(N_SF):
            cfg = O.tx_cfg_from_params(p, i)
            _, _, e_o = O.tx_subframe(cfg, [pay[i, cw] for cw in range(p.n_cw)], want_e=True)
            for cw in range(p.n_cw):
                G = pipe.G(cw, i)
                assert np.array_equal(gpu.unpack_bits(eb[i, cw], G), e_o[cw][:G]), (tag, i, cw)
    finally:
        O.set_rm_limited(False)


@pytest.mark.parametrize("tbs", PAIRS, ids=lambda t: "tbs%d_%d" % t)
def test_pipeline_segload(gpu, tbs):
    p = _params(gpu, tbs)
    pipe = gpu.TxPipeline(p, N_SF)
    assert all(pipe.G(cw, i) >= tbs[cw] for cw in range(2) for i in range(N_SF))
    pay = _payload(p, tbs, tbs[0])
    pipe.upload_payload(pay)
    pipe.run()
    pipe.sync()
    _check_ebits(gpu, p, pipe, pay, pipe.ebits(), tbs)
    pipe.close()


@pytest.mark.parametrize("tbs", [24504])
def test_debug_instantiation_b_c_e(gpu, tbs):
    """dlsch_encoding (k_encode_debug): b = TB || CRC-24A and every c[r] keep the reference's layout"""
    sf = 7
    p = gpu.make_params("C2", subframe=sf, TBS=(tbs, 0))
    cfg = O.tx_cfg_from_params(p, sf)
    fp = gpu.frame_parms(p.N_RB_DL, p.Nid_cell, 0, p.nb_antennas_tx, p.mode1_flag, 0)
    A = tbs // 8
    pay = np.random.default_rng(tbs).integers(0, 256, size=A + 8, dtype=np.uint8)
    pay[A:] = 0xFF
    _, _, e_o = O.tx_subframe(cfg, [pay.copy()], want_e=True)
    blocks = S.oracle_blocks(pay, tbs)
    crc = O.crc24a(np.concatenate([pay[:A], np.zeros(8, np.uint8)]), tbs) >> 8
    dl = gpu.DlschHandle(Kmimo=p.Kmimo, Mdlharq=8, N_RB_DL=p.N_RB_DL)
    h = dl.h
    h.TBS, h.mcs, h.rvidx, h.round, h.mimo_mode, h.Nl = tbs, p.mcs[0], 0, 0, p.mimo_mode, 1
    for i in range(4):
        h.rb_alloc[i] = p.rb_alloc[i]
    h.nb_rb = p.nb_rb
    dl.d.rnti = p.rnti
    assert gpu.dlsch_encoding(pay.copy(), fp, p.num_pdcch_symbols, dl, sf) == 0
    b = dl.view("b", A + 3)
    assert np.array_equal(b[:A], pay[:A])
    assert list(b[A:]) == [(crc >> 16) & 255, (crc >> 8) & 255, crc & 255]
    assert h.C == len(blocks) == 5
    for r, blk in enumerate(blocks):
        assert np.array_equal(dl.view("c", blk["K"] // 8, r), blk["c"]), r
    G = O.get_G(p.N_RB_DL, 0, p.mode1_flag, 0, p.nb_rb, list(p.rb_alloc), gpu.lib().oai4g_get_Qm(p.mcs[0]), 1,
                p.num_pdcch_symbols, sf)
    gpu.dlsch_scrambling(fp, dl, G, 0, 2 * sf)
    assert np.array_equal(dl.view("e", G), e_o[0][:G])
    dl.close()


@pytest.mark.parametrize("tbs", [(12232, 6096), (75376, 75376)])
def test_rows_end_at_the_allocation(gpu, tbs):
    """The payload rows are followed in the same allocation by one canary row only: the e bits are
    the oracle's and do not change with the canary (nothing at or past a row's end is read into them)"""
    p = _params(gpu, tbs)
    pipe = gpu.TxPipeline(p, N_SF)
    pay = _payload(p, tbs, 3 * tbs[0] + 1)
    L = gpu.lib()
    own = pipe.d_payload
    buf = L.oai4g_dev_alloc(pay.nbytes + p.payload_stride)
    assert buf
    got = []
    try:
        pipe.d_payload = buf
        for canary in (0xFF, 0x00):
            host = np.concatenate([pay.reshape(-1), np.full(p.payload_stride, canary, np.uint8)])
            assert L.oai4g_memcpy_h2d(buf, host.ctypes.data_as(ctypes.c_void_p), host.nbytes) == 0
            pipe.run()
            pipe.sync()
            got.append(pipe.ebits().copy())
    finally:
        pipe.d_payload = own
        L.oai4g_dev_free(buf)
    assert np.array_equal(got[0], got[1])
    _check_ebits(gpu, p, pipe, pay, got[0], tbs)
    pipe.close()
