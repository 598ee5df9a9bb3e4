"""Configurations that free, grow or rebuild their device memory while in use, at 6 PRB:

  - the drop-in receiver's per-thread cache evicts and destroys its oldest configuration; the same key then
    builds a new one that gives the first call's LLRs and log2_maxh;
  - one oai4g_rx_config runs batches of 1, 4 and 1 subframes (its shift buffer grows once and is kept);
  - one oai4g_pdcch_rx_config runs batches of 1 and 8 subframes (its record buffer grows).

Every run equals that of a configuration created for just that batch.
"""
import ctypes

import numpy as np
import pytest

import pdcch_rx_cases as PC
from test_gpu_pdcch_rx import CRNTI, RA, SI, _comp_of, _frames
from test_rx_cpu import alloc

pytestmark = pytest.mark.gpu

N_RB = 6
RX_SLOTS = 32            # entries of the drop-in receiver's cache


def _grids(gpu, fg, n_sf, seed):
    n = fg.symbols_per_tti * fg.ofdm_symbol_size
    rng = np.random.default_rng(seed)
    return (rng.integers(-3000, 3000, (n_sf, n), dtype=np.int64).astype(np.int32),
            rng.integers(-1500, 1500, (n_sf, n), dtype=np.int64).astype(np.int32))


def test_dropin_receiver_cache_eviction(gpu):
    # a cell identity no other test uses: none of the keys is in this thread's cache yet.  Subframe indices 0
    # and 5 are left out: at 6 PRB the PBCH / PSS / SSS take every RB of some symbols there
    fg = gpu.frame_parms(N_RB, Nid_cell=311)
    y, h = _grids(gpu, fg, 1, 41)
    keys = [(sf, Qm, npd) for sf in (1, 2, 3, 4, 6, 7, 8, 9) for Qm in (2, 4, 6) for npd in (1, 2)][:40]
    assert len(set(keys)) == 40 > RX_SLOTS
    run = lambda k: gpu.rx_pdsch_siso(fg, y[0], h[0], alloc(N_RB), k[1], k[2], k[0])
    llr0, shift0 = run(keys[0])
    llr0 = llr0.copy()
    assert len(llr0) > 0
    for k in keys[1:]:
        run(k)
    llr, shift = run(keys[0])
    assert shift == shift0 and llr.tobytes() == llr0.tobytes()


def test_rx_batch_grows_and_shrinks_on_one_configuration(gpu):
    Qm, npd, rnti, first = 4, 2, 0x1234, 1          # subframe indices 1..4
    fg = gpu.frame_parms(N_RB, Nid_cell=17)
    y, h = _grids(gpu, fg, 4, 43)
    L = gpu.lib()

    def fresh(n):
        rx = gpu.RxBatch(fg, alloc(N_RB), Qm, npd, rnti, n, first_subframe=first, subframe_step=1)
        try:
            return rx.run(y[:n], h[:n], unscramble=1)
        finally:
            rx.close()

    want = {n: fresh(n) for n in (1, 4)}
    rx = gpu.RxBatch(fg, alloc(N_RB), Qm, npd, rnti, 4, first_subframe=first, subframe_step=1)
    try:
        assert L.oai4g_memcpy_h2d(rx.d_y, y.ctypes.data, y.nbytes) == 0
        assert L.oai4g_memcpy_h2d(rx.d_h, h.ctypes.data, h.nbytes) == 0
        for n in (1, 4, 1):
            assert L.oai4g_memset_d(rx.d_llr, 0, 4 * rx.stride * 2) == 0
            assert L.oai4g_rx_batch(rx.cfg, n, rx.d_y, rx.d_h, rx.d_llr, 1, None) == 0
            got = rx.llrs()
            for i in range(n):
                cnt = rx.llr_count((first + i) % 10)
                assert cnt > 0 and got[i, :cnt].tobytes() == want[n][i, :cnt].tobytes(), (n, i)
    finally:
        rx.close()


def test_pdcch_batch_record_growth(gpu):
    fo, fg = _frames(gpu, N_RB)
    size, first, n_big = 21, 6, 8
    plan = [(0, 0, size, 4, 2, 2, 0, 0), (0, 1, size, 4, 2, 2, 0, 0)]     # the two UE-specific passes 4 CCEs can hold
    rng = np.random.default_rng(47)
    comps, npd = [], None
    for i in range(n_big):
        sf = (first + i) % 10
        items, n_common, want = PC.tx_items(fo, sf, size, rng, CRNTI, SI)
        n, comp = _comp_of(gpu, fg, fo, items, n_common, sf)
        assert n == want and npd in (None, n)
        npd = n
        comps.append(comp)
    comps = np.stack(comps)
    L = gpu.lib()

    def results(b, n):
        assert L.oai4g_pdcch_rx_batch(b.cfg, b.d_comp, n, first, b.d_out, None) == 0
        assert L.oai4g_sync() == 0
        out = (gpu.PdcchRxResult * n)()
        assert L.oai4g_memcpy_d2h(ctypes.addressof(out), b.d_out, ctypes.sizeof(out)) == 0
        return bytes(out), [r.dci_cnt for r in out]

    want = {}
    for n in (1, n_big):
        b = gpu.PdcchRxBatch(fg, npd, CRNTI, SI, RA, plan, n)
        try:
            b.upload(comps[:n])
            want[n] = results(b, n)
        finally:
            b.close()
    assert all(c > 0 for c in want[n_big][1])           # every subframe's DCIs are found: the records are in use
    b = gpu.PdcchRxBatch(fg, npd, CRNTI, SI, RA, plan, n_big)
    try:
        b.upload(comps)
        for n in (1, n_big):
            assert results(b, n) == want[n], n
    finally:
        b.close()
