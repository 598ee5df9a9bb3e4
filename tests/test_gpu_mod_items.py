"""k_modofdm's dense item space on the GPU: many rounds per workgroup, ragged last rounds, fill duties.

The suite's other transmit tests run small batches, where every workgroup of the persistent grid takes
one item (one round).  oai4g_set_modofdm_grid_cap caps the grid so that a few workgroups walk the whole
item space: the item -> (subframe, symbol, pair) map over many rounds, the prefetch chain across the
items that also zero-fill the skipped leading symbols, and inactive units in the last round.

Reference: the same pipeline with the default grid (the path the rest of the suite pins to the
oracle), itself compared with the oracle on the first, a middle and the last subframe.  Requirement:
the whole IQ equal.  Before every run the IQ buffer is set to a non-zero byte pattern, so the leading
symbols and their prefixes, which no transform writes, must really be rewritten as zeros."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

POISON = 0x5A


def _run(gpu, pipe, cap):
    assert gpu.lib().oai4g_memset_d(pipe.d_iq, POISON, pipe.iq_samples * 4) == 0
    gpu.lib().oai4g_set_modofdm_grid_cap(cap)
    pipe.run()
    pipe.sync()
    return pipe.iq()


def _sfi(p, i):
    return (p.first_subframe + i * p.subframe_step) % 10


def _check(gpu, p, n_sf, cap, lz, dci=None, n_common=0, setup=None):
    pipe = gpu.TxPipeline(p, n_sf)
    try:
        if setup:
            setup(pipe)
        assert pipe.mod_lz == lz
        pay = np.random.default_rng(n_sf * 131 + cap).integers(0, 256, size=(n_sf, p.n_cw, p.payload_stride),
                                                                dtype=np.uint8)
        pipe.upload_payload(pay)
        ref = _run(gpu, pipe, 0)
        for i in sorted({0, n_sf // 2, n_sf - 1}):
            txd, _, _ = O.tx_subframe(O.tx_cfg_from_params(p, _sfi(p, i)), [pay[i, cw] for cw in range(p.n_cw)],
                                      dci=dci, n_common=n_common)
            assert np.array_equal(ref[i], txd), ("default grid against the oracle", i)
        got = _run(gpu, pipe, cap)
        assert np.array_equal(got, ref)
    finally:
        gpu.lib().oai4g_set_modofdm_grid_cap(0)
        pipe.close()


# name, n_sf, cap, lz: rounds per workgroup and what the case covers
@pytest.mark.parametrize("name,n_sf,cap,lz", [
    ("C3", 37, 16, 1),    # 481 items: 30 rounds + 1 leftover item
    ("C3", 3, 1, 1),      # one workgroup runs everything: the prefetch chain across fill items
    ("C4", 5, 8, 1),      # two items per symbol, each fills its antenna pair
    ("C2", 5, 8, 1),      # one transform stored to every antenna
    ("C1", 9, 2, 3),      # 128 points, 16 units per workgroup, 99 items: inactive units in the last round
])
def test_capped_grid_equals_default_grid(gpu, name, n_sf, cap, lz):
    _check(gpu, gpu.make_params(name, subframe=7), n_sf, cap, lz)


@pytest.mark.parametrize("npd", [2, 3])
def test_two_and_three_control_symbols(gpu, npd):
    """per = 12 and 11 at 2048 points"""
    p = gpu.make_params("C3", subframe=7)
    p.num_pdcch_symbols = npd
    _check(gpu, p, 7, 4, npd)


def test_full_grid_keeps_the_map(gpu):
    """CRS on symbol 0: lz = 0, every symbol an item, all ten subframe indices"""
    _check(gpu, gpu.make_params("C3", subframe=0, subframe_step=1, with_crs=1), 10, 16, 0)


def test_chunked_pipeline(gpu, monkeypatch):
    """OAI4G_PIPE_CHUNK: three modulator launches, the later ones with sf0 = 8 and 16"""
    monkeypatch.setenv("OAI4G_PIPE_CHUNK", "8")
    _check(gpu, gpu.make_params("C3", subframe=3, subframe_step=1), 24, 16, 1)


def test_set_control_drops_the_skipped_symbols(gpu):
    """a PCFICH + PDCCH in symbol 0 of a grid without CRS: lz falls from 1 to 0 and symbol 0 is an item again"""
    p = gpu.make_params("C3", subframe=0, subframe_step=1, Nid_cell=77)
    fp = O.frame(p.N_RB_DL, p.Nid_cell, p.Ncp, p.nb_antennas_tx, p.mode1_flag)
    nCCE = O.get_nCCE(p.num_pdcch_symbols, fp)
    table = np.zeros(800, np.int32)
    items = [(48, 1, O.get_nCCE_offset(table, 2, nCCE, 0, p.rnti, 7), p.rnti,      # dlsim's format 2A DCI, L = 1
              np.random.default_rng(9).integers(0, 256, 8, dtype=np.uint8))]

    def setup(pipe):
        assert pipe.mod_lz == 1
        pipe.set_control(items, 0)

    _check(gpu, p, 10, 4, 0, dci=items, setup=setup)
