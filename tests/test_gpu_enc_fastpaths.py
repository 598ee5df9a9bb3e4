"""k_encode's per-geometry fast paths on the GPU, bit for bit against the oracle chain (e bits and IQ).

Phase 3b (turbo encoding) runs a lane-exact segment encoder for block sizes with 32 | K
(turbo_segment32<Q>, Q = ceil(K / 32 / 64) chunks per lane) and the generic one for every other size.
Phase 4 (sub-block interleaving + rate matching) walks the tile pairs of each half of the codeword's
blocks, on the `once` path (no repetition) or the general one.

The one-antenna 20 MHz configuration (C2) with TBS overridden so that segmentation
(lte_segmentation.c) yields the block sizes under test:
  TBS = K - 24          one block of K (B = K, no CRC-24B)
  TBS = 2K - 72         two blocks of K
  TBS = 3K - 96         three blocks of K (halves of 2 + 1 blocks)
  TBS = 12152           K- = 6080 and K+ = 6144 in one codeword, no filler
  TBS = 6208            K- = 3136 and K+ = 3200 with F = 56 filler bits
  TBS = 75376           13 blocks of 5824
and the flagship shape itself (C3: 6 blocks of 6144 on both codewords).

The exhaustive form (all 188 block sizes, every K- / K+ pair) is tests/test_gpu_enc_sweep.py."""
import pytest

import numpy as np

import oracle_lib as O
from test_gpu_parity import _pipeline_check
from test_gpu_rm_paths import _run

pytestmark = pytest.mark.gpu

# K: what the segment encoder does with it
SEGMENT_K = [40,      # generic path, partial chunk
             528,     # generic path, partial chunk
             1024,    # Q = 1, half the lanes
             2048,    # Q = 1, all 64 lanes
             2112,    # first Q = 2
             4096,    # Q = 2 exact
             4160,    # first Q = 3
             5120,    # Q = 3 with a part-filled last lane
             6080,    # Q = 3, 190 chunks
             6144]    # Q = 3 exact


@pytest.mark.parametrize("K", SEGMENT_K)
def test_segment_encoder_one_block(gpu, K):
    _pipeline_check(gpu, "C2", 2, 7, 1, seed=K, TBS=(K - 24, 0))


# codeword shapes of the phase-4 pair walk
SHAPES = [("C2", dict(TBS=(6120, 0))),        # C = 1: the second half is empty
          ("C2", dict(TBS=(12216, 0))),       # C = 2
          ("C2", dict(TBS=(18336, 0))),       # C = 3: halves of 2 + 1
          ("C2", dict(TBS=(12152, 0))),       # 6080 + 6144 in one codeword
          ("C2", dict(TBS=(6208, 0))),        # 3136 + 3200, F = 56
          ("C2", dict(TBS=(75376, 0))),       # C = 13
          ("C3", {})]                         # the flagship shape
REPEAT = ("C2", dict(TBS=(1000, 0)))          # one block of 1024 on 100 PRB: E > Nnn, the buffer repeats


@pytest.mark.parametrize("name,over", SHAPES)
def test_pair_walk_pipeline(gpu, name, over):
    _pipeline_check(gpu, name, 3, 7, 1, seed=len(name) + over.get("TBS", (0,))[0], **over)


@pytest.mark.parametrize("name,over", SHAPES + [REPEAT])
@pytest.mark.parametrize("rv", [0, 1, 2, 3])
def test_pair_walk_placement_paths(gpu, name, over, rv):
    """the `once` placement (where the plan allows it) and the forced general one, every redundancy
    version, subframes 0..9"""
    runs = [_run(gpu, name, over, rv, general) for general in (False, True)]
    p, pay, _, Gs = runs[0]
    for sf in range(10):
        cfg = O.tx_cfg_from_params(p, sf)
        _, _, e_o = O.tx_subframe(cfg, [pay[sf, cw] for cw in range(p.n_cw)], want_e=True)
        for cw in range(p.n_cw):
            G = Gs[sf][cw]
            for k, (_, _, eb, _) in enumerate(runs):
                assert np.array_equal(gpu.unpack_bits(eb[sf, cw], G), e_o[cw][:G]), (name, over, rv, sf, cw,
                                                                                      "general" if k else "once")
