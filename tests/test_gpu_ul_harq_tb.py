"""oai4g_ul_decode_batch_harq_tb: one batch whose transport blocks sit at different HARQ rounds.

Four transport blocks run four rounds; in every round each holds another (rv, clear) pair, and block
1 restarts (clear = 1, rv 0) in round 2 while its neighbours keep combining.  Per round the soft
buffers up to Ncb, the iteration counts and the decoded blocks are bit-exact against the oracle
chain (O.ulsch_decode_harq, lte_rate_matching_turbo_rx pinned to the reference's own in
tests/test_ref_pin_rm_cpu.py) called with each block's own rv and clear.

The int16 sums wrap: rounds 2 and 3 carry soft values of magnitude 20000, and from round 2 to round 3
every block moves to the next rv without a clear.  Consecutive rvs start a quarter of the circular
buffer apart and a round covers 0.44 of it or more at these shapes (E / Nnn), so the two rounds meet on
a stretch of every buffer, where the same coded bit arrives twice: +-40000.  The test keeps every
buffer's sum in 64 bits beside the oracle's and asserts, per code block, that the two differ
somewhere after round 3, so the case cannot vanish unnoticed."""
import numpy as np
import pytest

import oracle_lib as O
from test_ul_chain_cpu import UL, ul_e

pytestmark = pytest.mark.gpu

# SCHED[round][tb] = (rv, clear)
SCHED = [[(0, 1), (1, 1), (2, 1), (3, 1)],
         [(3, 0), (2, 0), (0, 0), (1, 0)],
         [(1, 0), (0, 1), (2, 0), (3, 0)],
         [(2, 0), (1, 0), (3, 0), (0, 0)]]
AMP = [20, 20, 20000, 20000]


def test_schedule_covers_the_cases():
    for rnd in SCHED:
        assert len(set(rnd)) == len(rnd)                       # different pairs within a round
    assert SCHED[2][1] == (0, 1) and all(c == 0 for t, (_, c) in enumerate(SCHED[2]) if t != 1)
    assert {rv for rnd in SCHED for rv, _ in rnd} == {0, 1, 2, 3}
    # the two large rounds: consecutive rvs, combined
    assert all(SCHED[3][t] == ((SCHED[2][t][0] + 1) & 3, 0) for t in range(4)) and AMP[2] + AMP[3] > 32767


def _wide_round(e, blocks, F, G, Qm, rv):
    """this round's contribution to every soft buffer of a transport block in 64 bits: the soft values in
    two halves, so that no int16 sum inside lte_rate_matching_turbo_rx wraps"""
    C, out, off = len(blocks), [], 0
    lo = (e.astype(np.int32) // 2).astype(np.int16)
    hi = (e.astype(np.int32) - lo).astype(np.int16)
    top = int(max(np.abs(lo.astype(np.int32)).max(), np.abs(hi.astype(np.int32)).max()))
    for r, blk in enumerate(blocks):
        K = len(blk)
        dw = O.dummy_w_F(K + 4, F if r == 0 else 0)
        a, E = O.rate_match_rx(lo[off:], K, G, C, r, Qm, rvidx=rv, dw=dw)
        b, _ = O.rate_match_rx(hi[off:], K, G, C, r, Qm, rvidx=rv, dw=dw)
        off += E
        assert top * -(-E // (3 * K)) < 32768        # a position takes at most ceil(E / Nnn) values, Nnn >= 3 K
        out.append(a.astype(np.int64) + b.astype(np.int64))
    return out


@pytest.mark.parametrize("tbs,G,Qm", UL)
def test_gpu_ul_harq_per_tb_rounds_match_oracle(gpu, tbs, G, Qm):
    import spec_model as S
    n_tb, rng = 4, np.random.default_rng(tbs + 1)
    pays = [rng.integers(0, 256, tbs // 8 + 8, dtype=np.uint8) for _ in range(n_tb)]
    blocks, F = S.segment([0] * (tbs + 24))
    wide = [[np.zeros(3 * 32 * ((len(b) + 4 + 31) // 32) + 64, np.int64) for b in blocks] for _ in range(n_tb)]
    w_o = [[np.zeros(3 * 32 * ((len(b) + 4 + 31) // 32) + 64, np.int16) for b in blocks] for _ in range(n_tb)]
    coded = {}

    def bits(t, rv):
        if (t, rv) not in coded:
            coded[t, rv] = 2 * np.array(ul_e(pays[t], tbs, G, Qm, rv=rv), np.float64) - 1
        return coded[t, rv]

    ub = gpu.UlDecodeBatch(tbs + 24, G, Qm, n_tb, max_iterations=4)
    try:
        for rnd, sched in enumerate(SCHED):
            amp = AMP[rnd]
            e = np.stack([np.clip(np.round(bits(t, sched[t][0]) * amp + rng.normal(0, 30, G)), -32768, 32767)
                          .astype(np.int16) for t in range(n_tb)])
            ub.upload(e)
            ub.launch_harq_tb([rv for rv, _ in sched], [c for _, c in sched])
            its, c = ub.results()
            wg = ub.soft_buffers()
            for t, (rv, clear) in enumerate(sched):
                ref = O.ulsch_decode_harq(e[t], tbs + 24, G, Qm, rv, clear, w_o[t], max_it=4)
                for r, contrib in enumerate(_wide_round(e[t], blocks, F, G, Qm, rv)):
                    wide[t][r] = contrib if clear else wide[t][r] + contrib
                for r, (it, d) in enumerate(ref):
                    Ncb = 3 * 32 * ((len(blocks[r]) + 4 + 31) // 32)
                    assert np.array_equal(wg[t, r, :Ncb], w_o[t][r][:Ncb]), (rnd, t, r)
                    assert its[t, r] == it, (rnd, t, r, its[t, r], it)
                    assert np.array_equal(c[t, r, :len(d)], d), (rnd, t, r)
                    # the buffer is the 64-bit sum reduced mod 2^16 ...
                    assert np.array_equal(wide[t][r][:Ncb].astype(np.int16), w_o[t][r][:Ncb]), (rnd, t, r)
                if rnd == 3:      # ... and in the last round that reduction is no identity: the sums wrapped
                    assert all(np.any(wide[t][r] != w_o[t][r]) for r in range(len(blocks))), (t, "no int16 sum wrapped")
    finally:
        ub.close()


def test_gpu_ul_harq_tb_masks_rv_and_takes_any_nonzero_clear(gpu):
    """rv is used masked with 3 and clear as zero / non-zero: (rv 6, clear 7) is (rv 2, clear 1)."""
    tbs, G, Qm = UL[1]
    rng = np.random.default_rng(5)
    e = rng.integers(-200, 200, size=(2, G)).astype(np.int16)
    out = []
    for rv, clear in (([2, 2], [1, 1]), ([6, 0xFE], [7, 0x80])):
        ub = gpu.UlDecodeBatch(tbs + 24, G, Qm, 2, max_iterations=2)
        try:
            ub.upload(e)
            ub.launch_harq_tb([1, 1], [1, 1])     # something to clear
            ub.launch_harq_tb(rv, clear)
            its, c = ub.results()
            out.append((its.copy(), c.copy(), ub.soft_buffers()))
        finally:
            ub.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
