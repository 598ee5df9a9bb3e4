"""Conditions on the fused encoder sweep's case list (tests/enc_sweep_cases.py), on the CPU: the
list covers what it claims, its geometries satisfy their inequalities with E taken from the
oracle's rate matcher, and the oracle chain the GPU sweep compares against equals the spec model
on one small case of every path class."""
import collections
import ctypes

import numpy as np
import pytest

import enc_sweep_cases as S
import oracle_lib as O
import spec_model as M

import openair4g_amd as oai


def test_every_size_has_a_single_block_case_that_repeats():
    singles = [c for c in S.single_cases() if c.F == 0]
    assert [c.Kp for c in singles] == S.sizes() and len(singles) == 188
    for c in singles:
        assert (c.C, c.tbs) == (1, c.Kp - 24)
        assert c.repeat is not None, c


def test_every_size_above_512_has_a_filler_case():
    ks = S.sizes()
    fill = {c.Kp: c for c in S.single_cases() if c.F > 0}
    assert sorted(fill) == [K for K in ks if K > 512]
    for K, c in fill.items():
        step = K - ks[ks.index(K) - 1]
        assert c.C == 1 and c.F == step - 8 and c.F in (8, 24, 56)
        assert S.seg_params(c.tbs + 24 - 8)[2] < K        # one more filler byte segments to the size below


def test_segmentation_restatement_equals_the_spec_model():
    for c in S.single_cases() + S.pair_cases():
        blocks, F = M.segment([0] * (c.tbs + 24))
        assert ([len(b) for b in blocks], F) == (c.Ks, c.F), c


def test_all_pairs_block_counts_and_splits_are_present():
    cand = S.pair_candidates()
    from_6144 = {(S.seg_params(t + 24)[3], S.seg_params(t + 24)[2]) for t in range(6144, 75376 + 8, 8)
                 if S.seg_params(t + 24)[1]}
    assert len(from_6144) == 47 and all(3200 <= kp <= 6144 for _, kp in from_6144)
    # TBS 6128 and 6136 (below that range, C = 2 already) add 3072 + 3136
    assert set(cand) == from_6144 | {(3072, 3136)}
    cases = S.pair_cases()
    assert [(c.Km, c.Kp) for c in cases] == sorted(cand)
    assert {c.C for c in cases} == set(range(2, 14))
    kinds = collections.Counter(k for c in cases for k in S.n0_kind(c.C, c.n0))
    assert all(kinds[k] >= 3 for k in ("one", "last", "middle")), kinds
    assert any(c.n0 == c.C - 1 and c.C > 2 for c in cases) and any(c.n0 == 1 and c.C > 2 for c in cases)
    assert 2 * sum(c.F > 0 for c in cases) >= len(cases)
    for c in cases:
        assert c.once is not None, c
        assert 0 < c.n0 < c.C and c.Kp * (c.C - c.n0) + c.Km * c.n0 - c.F == c.tbs + 24 + 24 * c.C


def test_cdd_shape_cases():
    cdd = S.cdd_cases()
    assert len(cdd) == 15
    kps = [S.seg_params(a + 24)[2] for a, _ in cdd]
    assert kps == sorted(set(kps)) and kps[0] == 3200 and kps[-1] == 6144
    assert max(b - a for a, b in zip(kps, kps[1:])) <= 256               # spread over K+
    for a, b in cdd:
        assert a != b
        for t in (a, b):
            C, Cm, Kp, Km, F = S.seg_params(t + 24)
            assert Cm > 0 and C * S.Ncb(Kp) <= S.NIR_KMIMO2               # no limited-buffer refusal
    assert sum(S.seg_params(a + 24)[4] > 0 for a, _ in cdd) >= 7


def test_once_unreachable_is_exactly_what_the_menu_cannot_reach():
    smallest = min(S.G_of(g, S.COND_SF) for g in S.MENU)
    want = {K: smallest for K in S.sizes()
            if not any(O.get_G(g.N_RB, 0, 1, 0, g.nb_rb, list(S.rb_alloc(g)), g.Qm, 1, g.npdcch, S.COND_SF) <= S.Nnn(K)
                       for g in S.MENU)}
    assert S.ONCE_UNREACHABLE == want
    assert 40 in want
    for c in S.single_cases():
        assert (c.once is None) == (c.Kp in S.ONCE_UNREACHABLE), c
        assert (c.small is not None) == (c.once is None)
    # the issue's own count: with full allocations alone every K >= 504 has Ncb / 2 <= E <= Nnn
    full = [g for g in S.MENU if g.nb_rb == g.N_RB]
    for K in S.sizes():
        if K >= 504:
            assert any(S.lands_once(g, [K]) and S.reads_half(g, [K]) for g in full), K
    assert sum(K >= 504 for K in S.sizes()) == 130


def _rate_matched_sizes(c, g, sf, rv):
    """E of every block from the oracle's rate matcher (w's content does not matter)"""
    G = S.G_of(g, sf)
    out = []
    for r, K in enumerate(c.Ks):
        R = (K + 4 + 31) // 32
        out.append(O.rate_match(R, G, np.zeros(3 * 32 * R, np.uint8), c.C, r, g.Qm, rvidx=rv).size)
    assert sum(out) == G
    return out


def test_inequalities_hold_for_every_chosen_geometry():
    checked = 0
    for c in S.single_cases() + S.pair_cases():
        nnn, ncb = [S.Nnn(K) for K in c.Ks], [S.Ncb(K) for K in c.Ks]
        if c.repeat:
            E = _rate_matched_sizes(c, c.repeat, S.COND_SF, 0)
            assert all(e >= n for e, n in zip(E, nnn)), c
            assert E == S.block_E(S.G_of(c.repeat, S.COND_SF), c.repeat.Qm, c.C)
        if c.once:
            for sf in S.SUBFRAMES:                                     # the once placement in both subframes
                E = _rate_matched_sizes(c, c.once, sf, c.general_rv)
                assert all(e <= n for e, n in zip(E, nnn)), (c, sf)
            if c.once_full:
                assert all(2 * e >= n for e, n in zip(E, ncb)), c     # E of COND_SF, the last of SUBFRAMES
            else:                                                      # nothing in the menu reads half the buffer
                assert not any(S.lands_once(g, c.Ks) and S.reads_half(g, c.Ks) for g in S.MENU), c
        if c.small:
            assert S.G_of(c.small, S.COND_SF) == S.ONCE_UNREACHABLE[c.Kp]
        checked += 1
    assert checked == 188 + 128 + 48
    # single blocks always find an entry that reads half the buffer, so rv 0..3 cover all of it
    assert all(c.once_full for c in S.single_cases() if c.once)
    # a pair without a repeat entry has none in the menu: even the largest allocation ends before the buffer
    gmax = max(S.MENU, key=lambda g: S.G_of(g, S.COND_SF))
    for c in S.pair_cases():
        assert (c.repeat is None) == (min(_rate_matched_sizes(c, gmax, S.COND_SF, 0)) < max(S.Nnn(K) for K in c.Ks)), c


def test_every_path_class_has_at_least_8_sizes():
    count = collections.Counter(k for K in S.sizes() for k in S.classes(K))
    assert set(count) == set(S.CLASSES)
    # fold32 admits six sizes in all (1024, 2048, .., 6144): each is in the sweep, there is no eighth
    assert count.pop("fold32") == 6 and [K for K in S.sizes() if S.fold32(K)] == [1024 * i for i in range(1, 7)]
    assert all(n >= 8 for n in count.values()), count
    assert (count["generic"], count["Q1"], count["Q2"], count["Q3"]) == (61, 63, 32, 32)
    assert (count["quarter-aligned"], count["quarter-or_bits"]) == (121, 61)
    assert (count["s1"], count["s3"]) == (86, 96)
    assert sum(S.plane_swap(K) for K in S.sizes()) == 102                 # 96 + the six 32-fold sizes
    assert sum(count["ND%d" % n] for n in (4, 12, 20, 28)) == 188
    print(sorted(count.items()))


def test_fold32_restatement_equals_the_library_predicate():
    for K in S.sizes():
        s, tab = ctypes.c_uint32(), (ctypes.c_uint16 * 256)()
        assert (oai.lib().oai4g_qpp_fold32(K, ctypes.byref(s), tab) == 1) == S.fold32(K), K


def _class_cases():
    """the smallest size of every class, plus the smallest filler case and the smallest pair"""
    ks = {min(K for K in S.sizes() if k in S.classes(K)) for k in S.CLASSES}
    return [c for c in S.single_cases() if c.F == 0 and c.Kp in ks] + \
        [min((c for c in S.single_cases() if c.F), key=lambda c: c.Kp), S.pair_cases()[0]]


@pytest.mark.parametrize("c", _class_cases(), ids=lambda c: "tbs%d" % c.tbs)
def test_oracle_chain_equals_the_spec_model(c):
    pay = np.random.default_rng(c.Kp).integers(0, 256, c.tbs // 8, dtype=np.uint8)
    blocks = S.oracle_blocks(pay, c.tbs)
    assert [b["K"] for b in blocks] == c.Ks
    for label, g, rv, _ in c.runs()[:2] + c.runs()[-1:]:
        G = S.G_of(g, S.COND_SF)
        c_init = (S.RNTI << 14) + (S.COND_SF << 9)
        want = M.dlsch_e(pay, c.tbs, G, g.Qm, rv=rv, c_init=c_init)
        assert np.array_equal(S.oracle_e(blocks, G, g.Qm, rv, S.COND_SF), want), (c, label)
