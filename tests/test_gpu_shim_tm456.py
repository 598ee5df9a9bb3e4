"""dlsch_modulation for the single-layer precoding modes through the reference-side boundary
(integration/liboai4g_shim.so, called with the reference's own LTE_DL_FRAME_PARMS / LTE_eNB_DLSCH_t),
compared live with the reference's dlsch_modulation.c.  The harness is tests/test_gpu_shim_ref.py's.

Limit: oracle/ref_glue_shim.c lays the reference structs out but has no field for pmi_alloc, which
new_eNB_dlsch leaves 0, so this covers precoder 0 only (antenna 1 = antenna 0, QPSK floors included);
the other precoders are covered through the C ABI in tests/test_gpu_mod_tm456.py."""
import numpy as np
import pytest

import oracle_lib as O
from mod_ref_cases import FULL, e_bits
from test_gpu_shim_ref import LIVE, _ptrs, _view, shim  # noqa: F401  (shim: the module's fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not LIVE, reason="integration/liboai4g_shim.so or oracle/_ref "
                                                                   "not built (needs the reference tree)")]


@pytest.mark.parametrize("mode,n_rb,mcs,subframe", [(3, 25, 5, 0), (8, 100, 22, 7)])
def test_shim_dlsch_modulation_precoding_modes(gpu, shim, mode, n_rb, mcs, subframe):  # noqa: F811
    S, G = shim
    npdcch, nid = 2, 11
    ofp = gpu.frame_parms(n_rb, nid, 0, 2, 0, 0)
    f = np.array([ofp.N_RB_DL, ofp.Nid_cell, ofp.Ncp, ofp.nushift, ofp.mode1_flag, ofp.nb_antennas_tx,
                  ofp.nb_antennas_tx_eNB or ofp.nb_antennas_tx, ofp.frame_type, ofp.tdd_config, ofp.symbols_per_tti,
                  ofp.log2_symbol_size, ofp.ofdm_symbol_size, ofp.first_carrier_offset, ofp.nb_prefix_samples,
                  ofp.nb_prefix_samples0, ofp.samples_per_tti, ofp.phich_resource, ofp.phich_duration,
                  ofp.Nid_cell_mbsfn, 1], np.int32)
    rfp = G.ref_shim_frame(f.ctypes.data)
    dl = G.ref_shim_new_dlsch(1, 8, n_rb)
    try:
        v = np.array([0x1234, 1024, mcs, 0, 0, mode, 1, n_rb, *FULL[n_rb], 8192, 8192, 1, 0],
                     np.int64).astype(np.uint32).view(np.int32)
        G.ref_shim_set(dl, v.ctypes.data)
        bits = e_bits(0x4565000 + mode)
        _view(G, dl, 4, bits.size)[:] = bits
        grids = [np.zeros(10 * 14 * ofp.ofdm_symbol_size, np.int32) for _ in range(2)]
        ret = S.dlsch_modulation(_ptrs(grids), 512, subframe, rfp, npdcch, dl, None)
        ret_ref, grids_ref = O.ref_modulation(O.frame(n_rb, nid, 0, 2, 0, 0), 512, subframe, npdcch,
                                              [dict(e=bits, mcs=mcs, mimo_mode=mode, rb_alloc=list(FULL[n_rb]))])
        assert ret == ret_ref and ret > 0
        for a in range(2):
            assert np.array_equal(grids[a], grids_ref[a]), a
        assert np.array_equal(grids[0], grids[1]) and grids[0].any()
    finally:
        G.ref_shim_free_dlsch(dl)
        G.ref_shim_free(rfp)
