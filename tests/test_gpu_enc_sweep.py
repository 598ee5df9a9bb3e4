"""The fused encoder (k_encode) over all 188 block sizes and every (K-, K+) pair segmentation can
produce, bit for bit against the oracle chain (turbo_encode, subblock, rate_match, scramble).

The drop-in 188-K sweeps (test_gpu_td_ref.py, the rm_ref digests) run k_turbo_bytes,
k_subblock_bytes and k_rm_bytes, which share no code with the fused kernel's per-size paths; the
fused kernel itself was pinned at some fifteen sizes (test_gpu_enc_fastpaths.py, test_gpu_qpp_fold.py).
Here the production kernel runs every case of tests/enc_sweep_cases.py: per case a `repeat`
geometry (every non-NULL position of the circular buffer appears in e), a `once` geometry at
rv 0..3 (together the whole buffer, the wrap tile moving across the block) and the same geometry
once more down the forced general placement, each on subframes 0 and 7 in one launch; fifteen pairs
also two at a time as the codewords of the LARGE_CDD shape.  k_encode's debug instantiation
(dlsch_encoding) is compared stage by stage (c, d, w, e), so that a production failure can be placed
at the phase where the stages first differ.

Consecutive sizes are grouped so that every production test makes about as many launches (a size
above 512 has two cases, with and without filler); a group's failures are collected and reported
together, block sizes first."""
import os

import numpy as np
import pytest

import enc_sweep_cases as S

pytestmark = pytest.mark.gpu

LAUNCHES = 24                   # pipeline launches per single-block production test: 4 sizes up to 512, 2 above
DEBUG_GROUP = 16                # block sizes per debug-instantiation test
PAIR_GROUP = 3                  # pairs per test
CDD_GROUP = 5


def _groups(items, n):
    return [items[i:i + n] for i in range(0, len(items), n)]


def _gid(group):
    def name(c):
        return "%d+%d" % (c.Km, c.Kp) if isinstance(c, S.Case) else str(c)
    return "%s..%s" % (name(group[0]), name(group[-1]))


def _cases_by_size():
    out = {}
    for c in S.single_cases():
        out.setdefault(c.Kp, []).append(c)
    return out


def _size_groups(launches):
    """consecutive block sizes, closed as soon as their cases make `launches` pipeline launches"""
    by_size, out, n = _cases_by_size(), [[]], 0
    for K in S.sizes():
        out[-1].append(K)
        n += sum(len(c.runs()) for c in by_size[K])
        if n >= launches:
            out.append([])
            n = 0
    return [g for g in out if g]


def _pipeline_ebits(gpu, name, g, tbs, rv, general, pay):
    """one launch over SUBFRAMES; returns per batch element and codeword the unpacked e bits"""
    n_cw = len(tbs)
    p = gpu.make_params(name, subframe=S.SUBFRAMES[0], subframe_step=S.SUBFRAMES[1] - S.SUBFRAMES[0], rnti=S.RNTI,
                        N_RB_DL=g.N_RB, rb_alloc=S.rb_alloc(g), nb_rb=g.nb_rb, num_pdcch_symbols=g.npdcch,
                        mcs=(S.MCS_OF_QM[g.Qm],) * 2, TBS=tuple(tbs) + (0,) * (2 - n_cw))
    for cw in range(n_cw):
        p.rvidx[cw] = rv
    if general:
        os.environ["OAI4G_ENC_GENERAL_RM"] = "1"
    try:
        pipe = gpu.TxPipeline(p, len(S.SUBFRAMES))
    finally:
        os.environ.pop("OAI4G_ENC_GENERAL_RM", None)
    assert pay.shape == (len(S.SUBFRAMES), n_cw, p.payload_stride)
    pipe.upload_payload(pay)
    pipe.run()
    pipe.sync()
    eb = pipe.ebits()
    out = []
    for i, sf in enumerate(S.SUBFRAMES):
        G = S.G_of(g, sf, p.mode1_flag)
        assert [pipe.G(cw, sf) for cw in range(n_cw)] == [G] * n_cw, (g, sf)
        out.append([gpu.unpack_bits(eb[i, cw], G) for cw in range(n_cw)])
    pipe.close()
    return out


def _stride(tbs):
    return (max(tbs) // 8 + 3 + 15) & ~15


def _production_failures(gpu, c):
    """every run of one single-codeword case; returns the runs whose e bits differ"""
    pay = np.random.default_rng(c.Kp).integers(0, 256, size=(len(S.SUBFRAMES), 1, _stride([c.tbs])), dtype=np.uint8)
    blocks = [S.oracle_blocks(pay[i, 0], c.tbs) for i in range(len(S.SUBFRAMES))]
    bad = []
    for label, g, rv, general in c.runs():
        got = _pipeline_ebits(gpu, "C2", g, (c.tbs,), rv, general, pay)
        for i, sf in enumerate(S.SUBFRAMES):
            want = S.oracle_e(blocks[i], S.G_of(g, sf), g.Qm, rv, sf)
            if not np.array_equal(got[i][0], want):
                bad.append((c.Kp, c.tbs, label, rv, sf, int(np.flatnonzero(got[i][0] != want)[0])))
    return bad


def _report(bad):
    """block sizes first, then (K, TBS, run, rv, subframe, first differing e index) of the first few"""
    return "sizes %s: %s" % (sorted({b[0] for b in bad}), bad[:8])


@pytest.mark.parametrize("group", _size_groups(LAUNCHES), ids=_gid)
def test_production_single_blocks(gpu, group):
    by_size = _cases_by_size()
    bad = [b for K in group for c in by_size[K] for b in _production_failures(gpu, c)]
    assert not bad, _report(bad)


@pytest.mark.parametrize("group", _groups(S.pair_cases(), PAIR_GROUP), ids=_gid)
def test_production_mixed_pairs(gpu, group):
    bad = [b for c in group for b in _production_failures(gpu, c)]
    assert not bad, _report(bad)


@pytest.mark.parametrize("group", _groups(S.cdd_cases(), CDD_GROUP), ids=lambda g: "tbs%d..%d" % (g[0][0], g[-1][0]))
def test_production_pairs_as_two_codewords(gpu, group):
    """C3's shape (LARGE_CDD, Kmimo = 2) with a different pair on each codeword: two per-codeword
    tables in one launch"""
    g = S.CDD_GEOM
    bad = []
    for tbs in group:
        pay = np.random.default_rng(tbs[0]).integers(0, 256, size=(len(S.SUBFRAMES), 2, _stride(tbs)), dtype=np.uint8)
        got = _pipeline_ebits(gpu, "C3", g, tbs, 0, False, pay)
        for i, sf in enumerate(S.SUBFRAMES):
            for cw in range(2):
                want = S.oracle_e(S.oracle_blocks(pay[i, cw], tbs[cw]), S.G_of(g, sf, 0), g.Qm, 0, sf, Kmimo=2)
                if not np.array_equal(got[i][cw], want):
                    bad.append((S.seg_params(tbs[cw] + 24)[2], tbs, "cw%d" % cw, 0, sf,
                                int(np.flatnonzero(got[i][cw] != want)[0])))
    assert not bad, _report(bad)


# ---- the debug instantiation, stage by stage ----
DEBUG_GEOM = S.Geom(100, 100, 4, 1)
DEBUG_SF = 7


def _debug_stages(gpu, c):
    g = DEBUG_GEOM
    fp = gpu.frame_parms(g.N_RB, 0, 0, 1, 1, 0)
    pay = np.random.default_rng(c.Kp).integers(0, 256, size=c.tbs // 8 + 8, dtype=np.uint8)
    blocks = S.oracle_blocks(pay, c.tbs)
    dl = gpu.DlschHandle(Kmimo=1, Mdlharq=8, N_RB_DL=g.N_RB)
    h = dl.h
    h.TBS, h.mcs, h.rvidx, h.round, h.mimo_mode, h.Nl = c.tbs, S.MCS_OF_QM[g.Qm], 0, 0, gpu.SISO, 1
    for i, w in enumerate(S.rb_alloc(g)):
        h.rb_alloc[i] = w
    h.nb_rb = g.nb_rb
    dl.d.rnti = S.RNTI
    assert gpu.dlsch_encoding(pay.copy(), fp, g.npdcch, dl, DEBUG_SF) == 0
    assert (h.C, h.Cminus, h.Kplus, h.Kminus, h.F) == (c.C, c.n0, c.Kp, c.Km if c.n0 else h.Kminus, c.F), c
    for r, b in enumerate(blocks):
        K, D = b["K"], b["K"] + 4
        assert np.array_equal(dl.view("c", K // 8, r), b["c"]), (K, r, "c", c.tbs)
        d = dl.view("d", 96 + 3 * D + 3, r)
        assert np.array_equal(d[:96], b["d"][:96]), (K, r, "d: NULL prefix", c.tbs)
        assert np.array_equal(d[96:96 + 3 * K], b["d"][96:96 + 3 * K]), (K, r, "d: the 3 K stream entries, filler included", c.tbs)
        assert np.array_equal(d[96 + 3 * K:96 + 3 * D], b["d"][96 + 3 * K:96 + 3 * D]), (K, r, "d: the 12 tail entries", c.tbs)
        assert d[96 + 3 * D + 2] == b["d"][96 + 3 * D + 2], (K, r, "d: the interleaver's d[3 D + 2] side effect", c.tbs)
        assert h.RTC[r] == b["R"], (K, r, "RTC", c.tbs)
        assert np.array_equal(dl.view("w", 3 * 32 * b["R"], r), b["w"]), (K, r, "w", c.tbs)
    G = S.G_of(g, DEBUG_SF)
    gpu.dlsch_scrambling(fp, dl, G, 0, 2 * DEBUG_SF)
    assert np.array_equal(dl.view("e", G), S.oracle_e(blocks, G, g.Qm, 0, DEBUG_SF)), (c.Kp, "e", c.tbs)
    dl.close()


@pytest.mark.parametrize("group", _groups(S.sizes(), DEBUG_GROUP), ids=_gid)
def test_debug_stages_single_blocks(gpu, group):
    by_size = _cases_by_size()
    for K in group:
        for c in by_size[K]:
            _debug_stages(gpu, c)


@pytest.mark.parametrize("group", _groups(S.pair_cases(), 2 * PAIR_GROUP), ids=_gid)
def test_debug_stages_mixed_pairs(gpu, group):
    for c in group:
        _debug_stages(gpu, c)
