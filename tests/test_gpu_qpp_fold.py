"""k_encode phase 3a's 32-fold QPP path (block sizes with 1024 | K) on the GPU, bit for bit against
the oracle chain: e bits and IQ of the batch pipeline, and the drop-in dlsch_encoding (k_encode's
debug instantiation shares the code).

The one-antenna 20 MHz configuration with TBS overridden so that segmentation (lte_segmentation.c)
yields exactly the block sizes under test:
  TBS = K - 24          one block of K (B = K, no CRC-24B)
  TBS = 2K - 72         two blocks of K (B' = 2K, no filler)
  TBS = 12152           K- = 6080 (quarter fold) and K+ = 6144 (32-fold) in one codeword, no filler
and the flagship shape itself (C3: 6 blocks of 6144 on both codewords).

The exhaustive form (all 188 block sizes, every K- / K+ pair) is tests/test_gpu_enc_sweep.py."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import _pipeline_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [1024, 2048, 3072, 4096, 5120, 6144])
def test_one_block_of_each_eligible_size(gpu, K):
    _pipeline_check(gpu, "C2", 2, 7, 1, seed=K, TBS=(K - 24, 0))


@pytest.mark.parametrize("K", [4096, 5120, 6144])
def test_two_equal_blocks(gpu, K):
    _pipeline_check(gpu, "C2", 2, 7, 1, seed=K + 1, TBS=(2 * K - 72, 0))


def test_mixed_pair_fallback_and_fast_in_one_codeword(gpu):
    _pipeline_check(gpu, "C2", 3, 7, 1, seed=12152, TBS=(12152, 0))


def test_flagship_shape(gpu):
    _pipeline_check(gpu, "C3", 2, 7, 0, seed=19)


@pytest.mark.parametrize("tbs", [6120, 12216])
def test_drop_in_dlsch_encoding(gpu, tbs):
    p = gpu.make_params("C2", subframe=7, TBS=(tbs, 0))
    cfg = O.tx_cfg_from_params(p, 7)
    fp = gpu.frame_parms(p.N_RB_DL, p.Nid_cell, 0, p.nb_antennas_tx, p.mode1_flag, 0)
    pay = np.random.default_rng(tbs).integers(0, 256, size=tbs // 8 + 8, dtype=np.uint8)
    _, _, e_o = O.tx_subframe(cfg, [pay.copy()], want_e=True)
    dl = gpu.DlschHandle(Kmimo=p.Kmimo, Mdlharq=8, N_RB_DL=p.N_RB_DL)
    h = dl.h
    h.TBS, h.mcs, h.rvidx, h.round, h.mimo_mode, h.Nl = tbs, p.mcs[0], 0, 0, p.mimo_mode, 1
    for i in range(4):
        h.rb_alloc[i] = p.rb_alloc[i]
    h.nb_rb = p.nb_rb
    dl.d.rnti = p.rnti
    assert gpu.dlsch_encoding(pay.copy(), fp, p.num_pdcch_symbols, dl, 7) == 0
    G = O.get_G(p.N_RB_DL, 0, p.mode1_flag, 0, p.nb_rb, list(p.rb_alloc), gpu.lib().oai4g_get_Qm(p.mcs[0]), 1,
                p.num_pdcch_symbols, 7)
    gpu.dlsch_scrambling(fp, dl, G, 0, 14)
    assert np.array_equal(dl.view("e", G), e_o[0][:G])
