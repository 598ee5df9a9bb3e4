"""dlsch_encoding for retransmission rounds through the reference-side boundary.

integration/liboai4g_shim.so is driven with the reference's own LTE_eNB_DLSCH_t / LTE_DL_eNB_HARQ_t, as
tests/test_gpu_shim_ref.py does.  A transport block is encoded at round 0 / rv 0; then, for (round,
rv) in (1, 1), (2, 2), (3, 3) and (1, 0), `a` and `e` are overwritten with 0xA5 and dlsch_encoding runs
again.  The reference's branch (dlsch_coding.c:286, 383-406) skips CRC, segmentation, coding and
interleaving and rate-matches the stored harq->w[r] again, so:

  - it returns 0 and e[0..G) is the concatenation, over r < C, of the reference's own
    lte_rate_matching_turbo (O.ref_rate_match) on w_flat[r 18432 : r 18432 + 3 Kpi] with the round's rv;
  - e past G, `a`, c, d, w and the segmentation fields are unchanged.

harq->w is uint8_t w[16][3 * 6144], but a K = 6144 block has 3 Kpi = 18528 entries: its last 96 lie on
the next row, where the next block's first 96 entries have replaced them.  The reference reads the
rows as they lie, and so does the drop-in.  A block reads the circular buffer from k0 for E entries:
  - C3 (E = 14400 or so per block): rv 0 starts at k0 = 386 and stays below entry 18432; rv 1, 2 and 3
    (k0 = 5018, 9650, 14282) read across entry 18431;
  - C2 / TM2 (E = 11000 or so): rv 2 and rv 3 read across it, rv 0 and rv 1 do not;
  - C1 has one small block and no overlap.
For those cases the expected e differs from the rate-matched intact w of every block (the test
asserts that at least one does), so the test shows that the overlap is honoured."""
import numpy as np
import pytest

import oracle_lib as O
import seg_ofdm_ref_cases as SC
from test_gpu_shim_ref import LIVE, _view, shim  # noqa: F401  (shim is the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not LIVE, reason="integration/liboai4g_shim.so or oracle/_ref "
                                                                   "not built (needs the reference tree)")]

W = 3 * 6144
MAX_E = 14 * 1200 * 6
ROUNDS = [(1, 1), (2, 2), (3, 3), (1, 0)]
CASES = [("C1", 7), ("C2", 7), ("C3", 7), ("TM2", 7), ("C3", 0)]
# (configuration, rv) whose blocks read across entry 18431 of their row
CROSSING = {("C3", 1), ("C3", 2), ("C3", 3), ("C2", 2), ("C2", 3), ("TM2", 2), ("TM2", 3)}


def _ref_frame(gpu, G, p):
    """(the library's frame parameters, the reference's LTE_DL_FRAME_PARMS laid out by the glue)"""
    ofp = gpu.frame_parms(p.N_RB_DL, p.Nid_cell, p.Ncp, p.nb_antennas_tx, p.mode1_flag, 0)
    f = np.array([ofp.N_RB_DL, ofp.Nid_cell, ofp.Ncp, ofp.nushift, ofp.mode1_flag, ofp.nb_antennas_tx,
                  ofp.nb_antennas_tx_eNB or ofp.nb_antennas_tx, ofp.frame_type, ofp.tdd_config, ofp.symbols_per_tti,
                  ofp.log2_symbol_size, ofp.ofdm_symbol_size, ofp.first_carrier_offset, ofp.nb_prefix_samples,
                  ofp.nb_prefix_samples0, ofp.samples_per_tti, ofp.phich_resource, ofp.phich_duration,
                  ofp.Nid_cell_mbsfn, 1], np.int32)
    return ofp, G.ref_shim_frame(f.ctypes.data)


def _set(G, dl, p, cw, rv, rnd):
    v = np.array([p.rnti, p.TBS[cw], p.mcs[cw], rv, rnd, p.mimo_mode, 1, p.nb_rb, *[p.rb_alloc[i] for i in range(4)],
                  p.sqrt_rho_a, p.sqrt_rho_b, 1, 0], np.int64).astype(np.uint32).view(np.int32)
    G.ref_shim_set(dl, v.ctypes.data)


@pytest.mark.parametrize("name,subframe", CASES)
def test_retransmission_rounds_rate_match_the_stored_rows(gpu, shim, name, subframe):
    S, G = shim
    p = gpu.make_params(name, subframe=subframe)
    ofp, rfp = _ref_frame(gpu, G, p)
    pay = SC.bench_payload(0x4A51 + subframe, 1, p.n_cw, p.payload_stride)[0]
    dls, differs = [], set()
    try:
        for cw in range(p.n_cw):
            dl = G.ref_shim_new_dlsch(p.Kmimo, 8, p.N_RB_DL)
            dls.append(dl)
            TBS, mcs = p.TBS[cw], p.mcs[cw]
            Qm = 2 if mcs < 10 else 4 if mcs < 17 else 6

            def setv(rv, rnd):
                _set(G, dl, p, cw, rv, rnd)

            setv(0, 0)
            a = np.zeros(TBS // 8 + 16, np.uint8)
            a[:TBS // 8] = pay[cw][:TBS // 8]
            assert S.dlsch_encoding(a.ctypes.data, rfp, p.num_pdcch_symbols, dl, 0, subframe, None, None, None) == 0
            out0 = np.zeros(23, np.uint32)
            G.ref_shim_get(dl, out0.ctypes.data)
            C, Cminus, Kplus, Kminus = int(out0[1]), int(out0[3]), int(out0[4]), int(out0[5])
            Ks = [Kminus if r < Cminus else Kplus for r in range(C)]
            RTC = [int(out0[7 + r]) for r in range(C)]
            Gbits = gpu.get_G(ofp, p.nb_rb, [p.rb_alloc[i] for i in range(4)], Qm, 1, p.num_pdcch_symbols, subframe)
            w_flat = _view(G, dl, 3, 16 * W).copy()
            snap_c = [_view(G, dl, 1, Ks[r] // 8, r).copy() for r in range(C)]
            snap_d = [_view(G, dl, 2, 96 + 3 * (Ks[r] + 4), r).copy() for r in range(C)]
            snap_b = _view(G, dl, 0, TBS // 8 + 3).copy()
            # every block's intact w, from the stored d[r]
            w_intact = [O.ref_subblock(snap_d[r][96:].copy(), Ks[r] + 4)[1] for r in range(C)]
            for rnd, rv in ROUNDS:
                setv(rv, rnd)
                a2 = np.full(TBS // 8 + 16, 0xA5, np.uint8)
                _view(G, dl, 4, MAX_E)[:] = 0xA5
                assert S.dlsch_encoding(a2.ctypes.data, rfp, p.num_pdcch_symbols, dl, 0, subframe, None, None,
                                        None) == 0, (name, cw, rnd, rv)
                want = np.concatenate([O.ref_rate_match(RTC[r], Gbits, w_flat[r * W:r * W + 3 * 32 * RTC[r]].copy(), C, r,
                                                        Qm, rvidx=rv, Nl=1, Kmimo=p.Kmimo) for r in range(C)])
                assert len(want) == Gbits
                e = _view(G, dl, 4, MAX_E).copy()
                assert np.array_equal(e[:Gbits], want), (name, cw, rnd, rv)
                assert np.all(e[Gbits:] == 0xA5), (name, cw, rnd, rv)
                assert np.all(a2 == 0xA5), (name, cw, rnd, rv)
                out = np.zeros(23, np.uint32)
                G.ref_shim_get(dl, out.ctypes.data)
                assert np.array_equal(out, out0), (name, cw, rnd, rv)
                assert np.array_equal(_view(G, dl, 3, 16 * W), w_flat), (name, cw, rnd, rv)
                assert np.array_equal(_view(G, dl, 0, TBS // 8 + 3), snap_b), (name, cw, rnd, rv)
                for r in range(C):
                    assert np.array_equal(_view(G, dl, 1, Ks[r] // 8, r), snap_c[r]), (name, cw, rnd, rv, r)
                    assert np.array_equal(_view(G, dl, 2, 96 + 3 * (Ks[r] + 4), r), snap_d[r]), (name, cw, rnd, rv, r)
                intact = np.concatenate([O.ref_rate_match(RTC[r], Gbits, w_intact[r].copy(), C, r, Qm, rvidx=rv, Nl=1,
                                                          Kmimo=p.Kmimo) for r in range(C)])
                if not np.array_equal(intact, want):
                    differs.add((name, rv))
        # the overlap shows where, and only where, the reads cross a row's end
        assert differs <= CROSSING, differs
        if any(n == name for n, _ in CROSSING):
            assert differs, "no case of %s differs from the intact-w result" % name
    finally:
        for dl in dls:
            G.ref_shim_free_dlsch(dl)
        G.ref_shim_free(rfp)


def test_a_row_of_nulls_is_refused(gpu, shim):
    """A stored row without a single non-NULL entry has nothing to rate-match (no first round leaves one):
    the call returns -1 and e stays as it was."""
    S, G = shim
    p = gpu.make_params("C1", subframe=7)
    _, rfp = _ref_frame(gpu, G, p)
    dl = G.ref_shim_new_dlsch(p.Kmimo, 8, p.N_RB_DL)
    try:
        _set(G, dl, p, 0, 0, 0)
        a = np.zeros(p.TBS[0] // 8 + 16, np.uint8)
        assert S.dlsch_encoding(a.ctypes.data, rfp, p.num_pdcch_symbols, dl, 0, 7, None, None, None) == 0
        out = np.zeros(23, np.uint32)
        G.ref_shim_get(dl, out.ctypes.data)
        assert out[1] == 1
        _view(G, dl, 3, 3 * 32 * int(out[7]))[:] = 2          # LTE_NULL over the whole of w[0]
        _view(G, dl, 4, MAX_E)[:] = 0xA5
        _set(G, dl, p, 0, 1, 1)
        assert S.dlsch_encoding(a.ctypes.data, rfp, p.num_pdcch_symbols, dl, 0, 7, None, None, None) == -1
        assert b"non-NULL" in gpu.lib().oai4g_last_error()
        assert np.all(_view(G, dl, 4, MAX_E) == 0xA5)
    finally:
        G.ref_shim_free_dlsch(dl)
        G.ref_shim_free(rfp)
