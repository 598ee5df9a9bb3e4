"""Both turbo decoders over every block size, bit for bit against the oracle: k_td16 (and its 3-wave
build k_td16_w3) over all 188 table sizes, k_td8 over the 129 sizes it takes (K >= 512, 16 | K).

The earlier decoder files run every K <= 320 and eight larger sizes through the 16-bit decoder and
nine sizes through the 8-bit one; both kernels take their chunking, checkpoint segments, state layout
period, prefetch parity, hard-decision rounds and CRC lane split from K (tests/dec_sweep_cases.py
names the classes, tests/test_dec_sweep_cases_cpu.py counts what the earlier sizes reached).  Here
every size runs a main batch (14 blocks, CRC24_B, blocks of one wave stopping at different
iterations, a partial tail wave) and a filler batch (CRC24_A from byte F / 8 on, the filler bytes
non-zero so that the offset matters), through the batched API and the drop-ins.  The rows are
uploaded with their padding set to 0x7fff and the output buffer poisoned, so a read of the padding
or a missing store shows.  The UL chain runs with the 8-bit decoder against the oracle chain."""
import numpy as np
import pytest

import dec_sweep_cases as D
import oracle_lib as O
from test_gpu_ul_chain import _batch as ul_batch
from test_ul_chain_cpu import UL

pytestmark = pytest.mark.gpu

POISON = 0xA5


def _cls(gpu, bits):
    return gpu.TurboDecoderBatch if bits == 16 else gpu.TurboDecoder8Batch


def _run(gpu, bits, b, max_it=None):
    """one launch over the rows of Batch b, uploaded with 0x7fff padding into a poisoned d_out"""
    n = len(b.y)
    dec = _cls(gpu, bits)(b.K, n)
    try:
        buf = b.padded(dec.llr_stride)
        assert buf.shape == (dec.n_cb, dec.llr_stride)
        poison = np.full(n * (b.K // 8), POISON, dtype=np.uint8)
        gpu._check(dec.L.oai4g_memcpy_h2d(dec.d_llr, gpu._ptr(buf), buf.nbytes) == 0)
        gpu._check(dec.L.oai4g_memcpy_h2d(dec.d_out, gpu._ptr(poison), poison.nbytes) == 0)
        dec.run(max_iterations=b.max_it if max_it is None else max_it, crc_type=b.crc_type, F=b.F)
        return dec.results()
    finally:
        dec.close()


def _diff(tag, got, want):
    """[] or one entry naming the rows whose iteration count or bytes differ: (batch, rows, got, oracle)"""
    its, out = got
    o_its, o_out = want
    rows = sorted(set(np.flatnonzero(its != o_its).tolist()) | set(np.flatnonzero((out != o_out).any(axis=1)).tolist()))
    return [(tag, rows, its[rows].tolist(), o_its[rows].tolist())] if rows else []


# One size per test: a size's 19 blocks on the oracle are most of a test's time, so a test cannot be
# cut smaller, and a failing run names its sizes in the test ids.
def _sweep(gpu, bits, K):
    bad = _diff("main", _run(gpu, bits, D.main_batch(K)), D.oracle_main(bits, K))
    bad += _diff("filler F=%d" % D.filler_F(K), _run(gpu, bits, D.filler_batch(K)), D.oracle_filler(bits, K))
    assert not bad, (K, bad)


@pytest.mark.parametrize("K", D.K16)
def test_batch16(gpu, K):
    _sweep(gpu, 16, K)


@pytest.mark.parametrize("K", D.K8)
def test_batch8(gpu, K):
    _sweep(gpu, 8, K)


@pytest.mark.parametrize("bits,K", [(16, 40), (16, 1056), (16, 6144), (8, 512), (8, 1056), (8, 6144)])
def test_one_iteration_leaves_the_output_untouched(gpu, bits, K):
    """max_iterations = 1 makes no hard decision (the reference leaves decoded_bytes as they were)"""
    b = D.main_batch(K)
    its, out = _run(gpu, bits, b, max_it=1)
    o_its, _ = D.oracle_rows(bits, K, b.y, 1, b.crc_type, b.F)
    assert np.array_equal(its, o_its) and np.all(its == 2)
    assert np.all(out == POISON)


# ---- the drop-ins: the 1.0 rung and the unstructured block of the main batch, and the clean block of
# the filler batch (the one whose stop depends on the CRC's start offset at every size with F > 0) ----
def _drop_in(gpu, bits, K):
    fn = gpu.turbo_decoder16 if bits == 16 else gpu.turbo_decoder8
    bad = []
    for b, want, rows in ((D.main_batch(K), D.oracle_main(bits, K), (D.MAIN_RUNG1, D.MAIN_UNSTRUCTURED)),
                          (D.filler_batch(K), D.oracle_filler(bits, K), (D.FILL_CLEAN,))):
        for i in rows:
            it, out = fn(b.y[i], K, max_iterations=b.max_it, crc_type=b.crc_type, F=b.F)
            if it != want[0][i] or not np.array_equal(out, want[1][i]):
                bad.append(("crc%d F=%d" % (b.crc_type, b.F), i, it, int(want[0][i])))
    assert not bad, (K, bad)


@pytest.mark.parametrize("K", D.K16)
def test_drop_in16(gpu, K):
    _drop_in(gpu, 16, K)


@pytest.mark.parametrize("K", D.K8)
def test_drop_in8(gpu, K):
    _drop_in(gpu, 8, K)


def test_decoder8_rejects_every_other_size(gpu):
    """the 59 table sizes outside K >= 512, 16 | K: the batch returns -1, the drop-in 255"""
    L = gpu.init()
    others = [K for K in D.K16 if K not in D.K8]
    assert len(others) == 59
    d = L.oai4g_dev_alloc(4096)
    gpu._check(bool(d))
    try:
        for K in others:
            assert L.oai4g_td8_batch(1, K, d, 3 * K + 16, d, K // 8, d, 8, 1, 0, d, None) == -1, K
            y = np.zeros(3 * K + 16, dtype=np.int16)
            out = np.zeros(K // 8, dtype=np.uint8)
            assert L.oai4g_phy_threegpplte_turbo_decoder8(gpu._ptr(y), gpu._ptr(out), K, 0, 0, 8, 1, 0) == 255, K
    finally:
        L.oai4g_dev_free(d)


# ---- k_td16_w3 ----
W3_MIN_CB = 98304               # TD16_W3_MIN_CB (oai4g_decode.hip): launches from here on run the 3-wave build


@pytest.mark.parametrize("K,n_cb", [(40, W3_MIN_CB - 1)] + [(K, W3_MIN_CB) for K in (40, 48, 88, 96, 200, 320, 512)])
def test_w3_build_small_sizes(gpu, K, n_cb):
    """K1 = 5 (the re-run reaches step K1), 6 and 11 (no full segment), 12, 25, 40 and 64 (one and
    several pipelined segments, both prefetch parities) through k_td16_w3, and K = 40 one block
    below the threshold through k_td16: every row against the oracle result of its period"""
    y = D.w3_rows(K)
    want = D.oracle_rows(16, K, y, 8, 1, 0)
    dec = gpu.TurboDecoderBatch(K, n_cb)
    try:
        dec.upload_tiled(y)
        dec.run(max_iterations=8, crc_type=1, F=0)
        its, out = dec.results()
    finally:
        dec.close()
    idx = np.arange(n_cb) % len(y)
    bad_it = np.flatnonzero(its != want[0][idx])
    assert bad_it.size == 0, (K, bad_it[:8], its[bad_it[:8]], want[0][idx[bad_it[:8]]])
    bad = np.flatnonzero((out != want[1][idx]).any(axis=1))
    assert bad.size == 0, (K, bad[:8])
    assert len(set(want[0].tolist())) > 2


# ---- the UL chain with the 8-bit decoder ----
def _check_ul(ub, refs, tag):
    ub.launch()
    its, c = ub.results()
    for t, ref in enumerate(refs):
        assert len(ref) == ub.C
        for r, (it, d) in enumerate(ref):
            assert its[t, r] == it, (tag, t, r, its[t, r], it)
            assert np.array_equal(c[t, r, :len(d)], d), (tag, t, r)


@pytest.mark.parametrize("tbs,G,Qm", UL[:2])
@pytest.mark.parametrize("amp,sigma,max_it", [(40, 45, 6), (30, 60, 8)])
def test_ul_chain_decoder8_matches_oracle(gpu, tbs, G, Qm, amp, sigma, max_it):
    """8 x 5504 and one block of 1056 with F = 24: 16 -> 8 -> 16 on one config, the scratch
    reallocated between the launches, each launch against the oracle chain of its decoder"""
    n_tb = 6
    e = ul_batch(tbs, G, Qm, n_tb, tbs + amp, amp, sigma, n_unique=2)
    ref16, ref8 = ([O.ulsch_decode(e[t], tbs + 24, G, Qm, max_it=max_it, decoder=dec) for t in range(n_tb)]
                   for dec in (O.turbo_decode, O.turbo_decode8))
    # the two decoders disagree on some iteration count or block (at these SNRs blocks run to the
    # last iteration and end on different hard decisions), so a launch that left the previous
    # launch's results in place would be seen
    assert any(i16 != i8 or not np.array_equal(d16, d8)
               for a, b in zip(ref16, ref8) for (i16, d16), (i8, d8) in zip(a, b))
    ub = gpu.UlDecodeBatch(tbs + 24, G, Qm, n_tb, max_iterations=max_it)
    try:
        ub.upload(e)
        _check_ul(ub, ref16, "16")
        ub.set_decoder(8)
        _check_ul(ub, ref8, "8")
        ub.set_decoder(16)
        _check_ul(ub, ref16, "16 again")
    finally:
        ub.close()


def test_ul_chain_decoder8_refuses_mixed_sizes(gpu):
    tbs, G, Qm = UL[2]
    ub = gpu.UlDecodeBatch(tbs + 24, G, Qm, 1)
    try:
        assert ub.L.oai4g_ul_config_set_decoder(ub.cfg, 8) == -1
        with pytest.raises(gpu.OAI4GError):
            ub.set_decoder(8)
        assert ub.L.oai4g_ul_config_set_decoder(ub.cfg, 12) == -1
        ub.set_decoder(16)
    finally:
        ub.close()
