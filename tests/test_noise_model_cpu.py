"""tests/noise_model.py against published and high-precision references, and the cases of tests/noise_cases.py against
the guard condition stated there (no device):

  - Philox-4x32-10 reproduces Random123's known-answer vectors (kat_vectors, "philox4x32 10");
  - u53's two edges;
  - normals and sigma agree with mpmath at 100 bits to 2^-60 relative;
  - no component of any committed case's model lies within GUARD of an integer, so tests/test_gpu_noise.py compares
    every sample;
  - the cases do what they are for: the wrap cases wrap, the small-sigma cases truncate on both sides of zero, the
    antennas' streams differ, and no two draws of a run share a Philox counter."""
import mpmath
import numpy as np
import pytest

import channel_model as M
import noise_cases as NC
import noise_model as NM

KAT = (
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
REL = 2.0 ** -60


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in NM.philox4x32_10(*ctr, *key)) == want
    # the vectorised form is the scalar one, element by element
    c = np.array([k[0] for k in KAT], dtype=np.uint64).T
    k = np.array([k[1] for k in KAT], dtype=np.uint64).T
    got = np.stack(NM.philox4x32_10(*c, *k), axis=-1)
    assert got.tolist() == [list(k[2]) for k in KAT]


def test_key_is_the_seeds_two_words():
    assert NM.key(99) == (99, 0) and NM.key(1 << 32) == (0, 1)
    assert NM.key(0x9E3779B97F4A7C15) == (0x7F4A7C15, 0x9E3779B9)


def test_u53_edges():
    assert NM.u53(0, 0) == 2.0 ** -53
    assert NM.u53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0
    assert NM.u53(0, 0x7FF) == 2.0 ** -53 and NM.u53(0, 0x800) == 2.0 ** -52      # the low 11 bits are dropped
    assert NM.u53(0x80000000, 0) == 0.5 + 2.0 ** -53


def _mp(x):
    """a long double as an mpf, exactly"""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - NM.LD(hi)))


def _rel(got, want):
    return abs((_mp(got) - want) / want)


def test_precision_against_mpmath():
    n = 256
    q = NM.philox4x32_10(np.arange(n, dtype=np.uint64), 1, 2, 3, 4, 5)
    # the edges of the reduction and of the logarithm ride along: u2 at the quadrant boundaries and next to them,
    # u1 = 1 - 2^-53 (the smallest radius) and 2^-53 (the largest)
    q = [w.copy() for w in q]
    for i, (hi, lo) in enumerate(((0x1FFFFFFF, 0xFFFFF800), (0x3FFFFFFF, 0xFFFFF800), (0x20000000, 0), (0x7FFFFFFF, 0xFFFFF000),
                                  (0xBFFFFFFF, 0xFFFFF800), (0xFFFFFFFF, 0xFFFFF800), (0, 0))):
        q[2][i], q[3][i] = hi, lo
    q[0][7], q[1][7] = 0xFFFFFFFF, 0xFFFFF000
    q[0][8], q[1][8] = 0, 0
    g_re, g_im = NM.normals(q)
    worst = 0.0
    with mpmath.workprec(100):
        for i in range(n):
            u1 = mpmath.mpf(((int(q[0][i]) << 32 | int(q[1][i])) >> 11) + 1) / 2 ** 53
            u2 = mpmath.mpf(((int(q[2][i]) << 32 | int(q[3][i])) >> 11) + 1) / 2 ** 53
            assert u1 == NM.u53(q[0][i], q[1][i]) and u2 == NM.u53(q[2][i], q[3][i])
            rad = mpmath.sqrt(-2 * mpmath.log(u1))
            for got, want in ((g_re[i], rad * mpmath.cospi(2 * u2)), (g_im[i], rad * mpmath.sinpi(2 * u2))):
                if want == 0:
                    assert got == 0, i
                    continue
                worst = max(worst, float(_rel(got, want)))
        print("normals: worst relative error 2^%.1f" % np.log2(worst))
        assert worst <= REL
        rng = np.random.default_rng(7)
        levs = list(NC.A_LEV) + [1, 2, 2 ** 31 - 1] + rng.integers(1, 2 ** 31, 256 - 3 - len(NC.A_LEV)).tolist()
        offs = rng.uniform(-40.0, 10.0, len(levs))
        offs[:len(NC.A_LEV)] = -3.0
        worst = 0.0
        for lev, off in zip(levs, offs):
            want = mpmath.sqrt(mpmath.power(10, (10 * mpmath.log10(int(lev)) + mpmath.mpf(float(off))) / 10) / 2)
            worst = max(worst, float(_rel(NM.sigma(np.int32(lev), off), want)))
        print("sigma: worst relative error 2^%.1f" % np.log2(worst))
        assert worst <= REL


def _report(name, dist):
    print("%-28s closest approach to an integer %.3g" % (name, dist.min()))


@pytest.mark.parametrize("case", NC.A_CASES, ids=NC.a_id)
def test_guard_awgn_cases(case):
    """zero samples excluded: every component of the model is further than GUARD from an integer"""
    _, dist = NC.a_model(case)
    _report(NC.a_id(case), dist)
    assert dist.min() > NC.GUARD, np.argwhere(dist <= NC.GUARD).tolist()


@pytest.mark.parametrize("case", NC.B_CASES, ids="-".join)
def test_guard_multipath_cases(case):
    """the same for convolution plus noise; sigma lies in 10 .. 100 as the cases intend"""
    (taps, x, tail, lev), (_, dist) = NC.b_expected(case)
    _report("-".join(case), dist)
    assert dist.min() > NC.GUARD, np.argwhere(dist <= NC.GUARD).tolist()
    s = [float(NM.sigma(np.int32(l.sum()), NC.B_OFFSET_DB)) for l in lev]
    assert 10.0 <= min(s) and max(s) <= 100.0
    assert len(set(lev.ravel().tolist())) == lev.size


@pytest.mark.parametrize("case", NC.A_CASES, ids=NC.a_id)
def test_awgn_cases_wrap_and_truncate(case):
    tx_len, tail_len, seed, off = case
    x, tail = NC.a_input(case)
    got, _ = NC.a_model(case)
    sig = np.concatenate([x, np.broadcast_to(tail, (NC.A_N,) + tail.shape)], axis=1).astype(np.int64)
    # the untruncated value, to the integer: signal + truncated noise; a wrap shows as a jump of 2^16
    jump = got.astype(np.int64) - sig
    assert np.any(np.abs(jump) > 60000), "no sample wraps"
    for v in range(NC.A_N):
        s = float(NM.sigma(NC.A_LEV[v], off))
        if s * 8.6 < 1.0:
            # |noise| < 1: (short) gives the signal itself, or one nearer to zero where the noise points there
            d = got[v].astype(np.int64) - sig[v]
            pos, neg = sig[v] > 0, sig[v] < 0
            assert set(np.unique(d[pos])) == {-1, 0} and set(np.unique(d[neg])) == {0, 1}, (v, s)
            assert np.all(d[sig[v] == 0] == 0)
    small = [v for v in range(NC.A_N) if float(NM.sigma(NC.A_LEV[v], off)) * 8.6 < 1.0]
    assert small if off == -30.0 else not small


def test_multipath_layouts_reach_both_store_paths():
    """the host's condition for the 16-byte store, restated: every "vec4" case meets it, no "odd" case does"""
    for case in NC.B_CASES:
        length, seg, seg_stride, ant_stride, rx_stride = NC.b_geometry(case)
        vec4 = all(v % 4 == 0 for v in (length, seg, seg_stride, ant_stride, rx_stride))
        assert vec4 == (case[1] == "vec4"), case
        assert length > 1024 and length % 1024                       # more than one tile, the last one partial


def test_antenna_streams_differ():
    n = 4096
    for seed in NC.SEEDS:
        g0, g1 = NM.noise(n, seed, NC.B_FIRST, 0), NM.noise(n, seed, NC.B_FIRST, 1)
        assert np.mean(np.all(g0 != g1, axis=-1)) > 0.99
        w0, _ = NM.awgn(np.zeros((n, 2), np.int16), 5000, NC.B_OFFSET_DB, seed, NC.B_FIRST, 0)
        w1, _ = NM.awgn(np.zeros((n, 2), np.int16), 5000, NC.B_OFFSET_DB, seed, NC.B_FIRST, 1)
        assert np.mean(np.any(w0 != w1, axis=-1)) > 0.99


def _rows(w0, w1, w2, w3):
    return np.stack([a.ravel() for a in np.broadcast_arrays(*[np.asarray(w, dtype=np.uint64) for w in (w0, w1, w2, w3)])], axis=-1)


def _distinct(rows):
    rows = np.concatenate(rows)
    return len(np.unique(rows, axis=0)) == len(rows)


def test_counters_are_pairwise_distinct():
    """all blocks drawn under one key, over the sizes of the cases: the noise of every vector and antenna, the taps and
    the angles of every vector and step"""
    # A and B: noise streams of the vectors and antennas
    rows = [_rows(*NM.noise_counters(3845, NC.A_FIRST + v)) for v in range(NC.A_N)]
    rows += [_rows(*NM.noise_counters(2056, NC.B_FIRST + v, a)) for v in range(NC.B_N) for a in range(2)]
    assert _distinct(rows)
    # C: normals and angles of every model, vector and step, beside a noise stream of the same vectors
    for model, nt, nr in NC.C_MODELS:
        d = M.describe(model, nt, nr, NC.C_BW)
        rows = []
        for v in range(NC.C_N):
            for step in range(3):
                w0, a0 = NM.tap_counters(d, NC.C_FIRST + v, step)
                rows += [_rows(w0, NC.C_FIRST + v, step, NM.TAP_WORD3), _rows(a0, NC.C_FIRST + v, step, NM.TAP_WORD3)]
            rows.append(_rows(*NM.noise_counters(512, NC.C_FIRST + v)))
        assert _distinct(rows), model
    # D: the loop hands step s the vectors [s B, (s + 1) B) and the step s, to the taps and to the noise
    d = M.describe("Rayleigh1", 1, 1, 5.0)
    rows = []
    for step in range(NC.D_STEPS):
        for v in range(NC.D_BATCH):
            vec = step * NC.D_BATCH + v
            w0, a0 = NM.tap_counters(d, vec, step)
            rows += [_rows(w0, vec, step, NM.TAP_WORD3), _rows(*NM.noise_counters(2 * 7680, vec))]
    assert _distinct(rows)


def test_tap_draws_order():
    """tap_draws hands channel_model.random_channel what it consumes: the count, and each value at the place the loop
    (tap, aarx, aatx: x, y, then the angle's uniform on tap 0) reads it"""
    import channel_cases as CC
    for model, nt, nr in NC.C_MODELS:
        d = M.describe(model, nt, nr, NC.C_BW)
        seq = NM.tap_draws(d, NC.SEED_BOTH, NC.C_FIRST, 1)
        assert len(seq) == CC.n_draws(d.nb_taps, nt, nr, d.ricean_factor, d.random_aoa)
        it = iter(seq)
        for t in range(d.nb_taps):
            for aarx in range(nr):
                for aatx in range(nt):
                    p = aarx + aatx * nr
                    q = NM.philox4x32_10(4 * t + p, NC.C_FIRST, 1, 0xC4A7, *NM.key(NC.SEED_BOTH))
                    gx, gy = NM.normals(q)
                    assert next(it) == float(gx) and next(it) == float(gy)
                    if t == 0 and NM.angles_drawn(d):
                        r = NM.philox4x32_10(0x100 + p, NC.C_FIRST, 1, 0xC4A7, *NM.key(NC.SEED_BOTH))
                        assert next(it) == NM.u53(r[0], r[1])
        assert next(it, None) is None
