"""The case list of the fused encoder sweep (tests/test_gpu_enc_sweep.py): plain Python, no GPU.

k_encode (openair4g_amd/csrc/oai4g_encode.hip) takes a different code path per block size K: the QPP
interleave by 32-fold coset transpose or by the quarter fold (byte-aligned stores or or_bits, with
or without the plane swap), the generic turbo segment encoder or turbo_segment32<1|2|3>, and a
host-built rate-matching plan whose shape follows R = ceil((K + 4) / 32), ND = 32 R - (K + 4), the
redundancy version and E.  This module lists what the sweep runs so that every one of the 188 block
sizes, and every (K-, K+) pair that segmentation can produce, goes through the production kernel:

  single-block cases   TBS = K - 24 (C = 1, F = 0) for every K, and for every K > 512 the TBS with the
                       largest byte-aligned filler that still segments to K (F = K - K_prev - 8)
  mixed-pair cases     one TBS per (K-, K+) pair, C rotated over 2..13, n0 = C- rotated over 1, C - 1
                       and a middle split, F > 0 in at least half of them
  geometries           per case a `repeat` entry (E >= Nnn for every block: every non-NULL position of
                       the circular buffer appears in e at rv 0) and a `once` entry (Ncb / 2 <= E <= Nnn:
                       rv 0..3 start a quarter buffer apart and together read the whole buffer, the
                       wrap tile moving across the block), both from MENU by the oracle's get_G

Nothing here comes from the library under test: segmentation is restated from lte_segmentation.c
(spec_model.segment restates it too; the CPU test compares the two), G is the oracle's get_G, E the
reference's split of G over the blocks (dlsch_coding.c / lte_rate_matching.c:506-512).

The reference encodes filler bits as zeros and never marks them NULL (3gpplte_sse.c:380-476, the
oracle and the library follow it), so Nnn = 3 K + 12 whatever F is.

The conditions on E are taken at subframe 7 (COND_SF).  Every run also covers subframe 0, whose G
is smaller through the PBCH and synchronisation exclusions: there a `repeat` entry may stop short
of the whole buffer, and a `once` entry stays on the once placement (E only shrinks)."""
import collections
import functools
import re
from pathlib import Path

import numpy as np

import oracle_lib as O

SUBFRAMES = (0, 7)          # first_subframe 0, subframe_step 7: batch elements 0 and 1
COND_SF = 7
RNTI = 0x1234
MCS_OF_QM = {2: 9, 4: 16, 6: 19}
NSOFT = 1827072


@functools.lru_cache(None)
def qpp():
    text = (Path(__file__).resolve().parent.parent / "include" / "oai4g_qpp.c").read_text()
    rows = [tuple(int(v) for v in m) for m in re.findall(r"\{\s*(\d+),\s*(\d+),\s*(\d+)\}", text)]
    assert len(rows) == 188 and [r[0] for r in rows] == sorted(r[0] for r in rows)
    return {K: (f1, f2) for K, f1, f2 in rows}


def sizes():
    return sorted(qpp())


def seg_params(B):
    """lte_segmentation.c:39-133 for B = TBS + 24 bits: (C, Cminus, Kplus, Kminus, F)"""
    if B <= 6144:
        L, C, Bp = 0, 1, B
    else:
        L = 24
        C = (B + (6144 - L) - 1) // (6144 - L)
        Bp = B + C * L
    per = Bp // C
    if per <= 40:
        Kp, Km = 40, 0
    elif per <= 512:
        Kp, Km = (per >> 3) << 3, per - 8
    elif per <= 1024:
        Kp = ((per + 15) >> 4) << 4
        Km = Kp - 16
    elif per <= 2048:
        Kp = ((per + 31) >> 5) << 5
        Km = Kp - 32
    else:
        Kp = ((per + 63) >> 6) << 6
        Km = Kp - 64
    if C == 1:
        Cm, Km = 0, 0
    else:
        Cm = (C * Kp - Bp) // (Kp - Km)
    F = (C - Cm) * Kp + Cm * Km - Bp
    return C, Cm, Kp, Km, F


# ---------------------------------------------------------------- path classes of a block size
def fold32(K):
    """phase 3a's 32-fold predicate (oai4g_qpp_fold32 restated): 1024 | K and Pi(k + K/32) - Pi(k)
    an odd multiple of K/32 for every k"""
    if K % 1024:
        return False
    f1, f2 = qpp()[K]
    Q = K // 32

    def pi(k):
        return (f1 * k + f2 * k * k) % K
    d = (pi(Q) - pi(0)) % K
    if d % Q or not (d // Q) & 1:
        return False
    return all((pi(k + Q) - pi(k)) % K == d for k in range(K))


def plane_swap(K):
    """the quarter fold's `s3`: output quarter q reads plane (q c4 / Q) mod 4 with c4 / Q = 3
    (c4 = Pi(K / 4) - Pi(0) = f1 K / 4 mod K, f2 (K / 4)^2 being a multiple of K)"""
    f1, _ = qpp()[K]
    c4 = (f1 * (K // 4)) % K
    assert c4 % (K // 4) == 0 and c4 // (K // 4) in (1, 3)
    return c4 // (K // 4) == 3


def classes(K):
    """labels of the k_encode paths block size K takes"""
    R = (K + 4 + 31) // 32
    out = {"ND%d" % (32 * R - (K + 4))}
    out.add("generic" if K & 31 else "Q%d" % (1 if K // 32 <= 64 else 2 if K // 32 <= 128 else 3))
    if fold32(K):
        out.add("fold32")
    else:
        out.add("quarter-or_bits" if K & 31 else "quarter-aligned")
        out.add("s3" if plane_swap(K) else "s1")
    return out


CLASSES = ("generic", "Q1", "Q2", "Q3", "fold32", "quarter-aligned", "quarter-or_bits", "s1", "s3",
           "ND4", "ND12", "ND20", "ND28")


# ---------------------------------------------------------------- the geometry menu
Geom = collections.namedtuple("Geom", "N_RB nb_rb Qm npdcch")     # the nb_rb lowest PRBs of N_RB, one antenna

# full allocations at 1.4 / 3 / 5 / 10 / 20 MHz, and 1..5 of the 6 PRBs at 1.4 MHz for the small sizes
MENU = tuple(Geom(n, n, qm, pd) for n in (6, 15, 25, 50, 100) for qm in (2, 4, 6) for pd in (1, 3)) + \
    tuple(Geom(6, n, qm, pd) for n in (1, 2, 3, 4, 5) for qm in (2, 4, 6) for pd in (1, 3))


def rb_alloc(g):
    m = (1 << g.nb_rb) - 1
    return tuple((m >> (32 * i)) & 0xffffffff for i in range(4))


@functools.lru_cache(None)
def G_of(g, sf, mode1_flag=1):
    """G of one codeword (one layer); mode1_flag 0 leaves out the second port's reference signals too"""
    return O.get_G(g.N_RB, 0, mode1_flag, 0, g.nb_rb, list(rb_alloc(g)), g.Qm, 1, g.npdcch, sf)


def block_E(G, Qm, C, Nl=1):
    """E of each block (lte_rate_matching.c:506-512)"""
    Gp = G // (Nl * Qm)
    return [Nl * Qm * (Gp // C) if r < C - Gp % C else Nl * Qm * -(-Gp // C) for r in range(C)]


def Nnn(K):
    return 3 * K + 12


def Ncb(K):
    return 3 * 32 * ((K + 4 + 31) // 32)


class Case:
    """one transport block size: its segmentation and the geometries it runs at"""

    def __init__(self, kind, tbs):
        self.kind, self.tbs = kind, tbs
        self.C, self.n0, self.Kp, self.Km, self.F = seg_params(tbs + 24)
        self.Ks = [self.Km] * self.n0 + [self.Kp] * (self.C - self.n0)
        self.repeat, self.once, self.once_full = pick_geometries(self.Ks)
        # sizes no menu entry reaches without repetition still run the smallest entry at every rv: at
        # subframe 0 its G is small enough for the once placement down to K = 40
        self.small = None if self.once else min(MENU, key=lambda g: G_of(g, COND_SF))

    @property
    def general_rv(self):
        return sizes().index(self.Kp) % 4

    def runs(self):
        """(label, geometry, rv, forced general placement)"""
        out = []
        if self.repeat:
            out.append(("repeat", self.repeat, 0, False))
        g = self.once or self.small
        out += [("once" if self.once else "small", g, rv, False) for rv in range(4)]
        out.append(("general", g, self.general_rv, True))
        return out

    def __repr__(self):
        return "Case(%s TBS=%d C=%d n0=%d K-=%d K+=%d F=%d)" % (self.kind, self.tbs, self.C, self.n0, self.Km,
                                                                self.Kp, self.F)


def repeats(g, Ks, sf=COND_SF):
    return min(block_E(G_of(g, sf), g.Qm, len(Ks))) >= max(Nnn(K) for K in Ks)


def lands_once(g, Ks, sf=COND_SF):
    return max(block_E(G_of(g, sf), g.Qm, len(Ks))) <= min(Nnn(K) for K in Ks)


def reads_half(g, Ks, sf=COND_SF):
    return 2 * min(block_E(G_of(g, sf), g.Qm, len(Ks))) >= max(Ncb(K) for K in Ks)


def pick_geometries(Ks):
    """(repeat, once, once_full): the smallest entry that repeats, and the smallest entry with
    Ncb / 2 <= E <= Nnn, or failing that lower bound (once_full False) the largest with E <= Nnn"""
    menu = sorted(MENU, key=lambda g: (G_of(g, COND_SF), g))
    rep = next((g for g in menu if repeats(g, Ks)), None)
    fits = [g for g in menu if lands_once(g, Ks)]
    full = [g for g in fits if reads_half(g, Ks)]
    return rep, (full[0] if full else fits[-1] if fits else None), bool(full)


# sizes for which no menu entry has E <= Nnn at subframe 7, with the menu's smallest G there:
# Nnn = 3 K + 12 is below one PRB of QPSK behind three control symbols (252 bits)
ONCE_UNREACHABLE = {40: 252, 48: 252, 56: 252, 64: 252, 72: 252}


# ---------------------------------------------------------------- the cases
@functools.lru_cache(None)
def single_cases():
    ks = sizes()
    out = []
    for i, K in enumerate(ks):
        out.append(Case("single", K - 24))
        if K > 512:
            out.append(Case("single", K - 24 - (K - ks[i - 1] - 8)))
    return out


@functools.lru_cache(None)
def pair_candidates():
    """every (K-, K+) a byte-aligned transport block can segment to, with its (TBS, C, C-, F) list"""
    pairs = collections.defaultdict(list)
    for tbs in range(6128, 75376 + 8, 8):        # C > 1 from TBS 6128 on; 75376 is the largest table TBS
        C, Cm, Kp, Km, F = seg_params(tbs + 24)
        if Cm:
            pairs[(Km, Kp)].append((tbs, C, Cm, F))
    return dict(sorted(pairs.items()))


def n0_kind(C, Cm):
    """which of the three splits (C = 2 has only the first two, in one)"""
    return {k for k, on in (("one", Cm == 1), ("last", Cm == C - 1), ("middle", 1 < Cm < C - 1)) if on}


@functools.lru_cache(None)
def pair_cases():
    """One TBS per pair.  Going up the pairs, C is the feasible block count used least so far (the
    larger of equals), so that the few pairs that reach C = 13 spend themselves on the rare counts;
    the split kind and F > 0 / F = 0 rotate with the pair's index (two in three carry filler)."""
    used = collections.Counter()
    out = []
    for i, (pair, cands) in enumerate(pair_candidates().items()):
        C = min({c[1] for c in cands}, key=lambda v: (used[v], -v))
        used[C] += 1
        cands = [c for c in cands if c[1] == C]
        kind = ("one", "last", "middle")[i % 3]
        cands = [c for c in cands if kind in n0_kind(C, c[2])] or cands
        tbs = max(cands, key=lambda c: (c[3], -c[0]))[0] if i % 3 else min(cands, key=lambda c: (c[3], c[0]))[0]
        out.append(Case("pair", tbs))
        assert (out[-1].Km, out[-1].Kp) == pair
    return out


NIR_KMIMO2 = NSOFT // 2 // 8


@functools.lru_cache(None)
def cdd_cases():
    """Fifteen pairs spread over K+ for the two-codeword LARGE_CDD shape: codeword 0 carries pair i,
    codeword 1 the next chosen pair, so two different per-codeword tables share one launch.  Kmimo = 2
    halves the soft buffer: the TBS of a pair is the one with the most blocks that the reference still
    rate-matches (C Kw <= Nir, lte_rate_matching.c:518-521), with filler on every other one."""
    items = list(pair_candidates().items())
    items = [it for it in items if it[0][1] >= 3200]
    chosen = [items[round(k * (len(items) - 1) / 14)] for k in range(15)]
    tbs = []
    for k, (pair, cands) in enumerate(chosen):
        ok = [c for c in cands if c[1] * Ncb(pair[1]) <= NIR_KMIMO2]
        C = max(c[1] for c in ok)
        ok = [c for c in ok if c[1] == C]
        tbs.append(max(ok, key=lambda c: (c[3], c[0]))[0] if k % 2 else min(ok, key=lambda c: (c[3], c[0]))[0])
    return [(tbs[k], tbs[(k + 1) % 15]) for k in range(15)]


CDD_GEOM = Geom(100, 100, 6, 1)          # C3's own allocation


# ---------------------------------------------------------------- the expected side: the oracle chain
_seg = None


def _segmentation(a, B):
    global _seg
    import ctypes
    if _seg is None:
        _seg = O.orc().orc_segmentation
        _seg.restype = ctypes.c_int
        _seg.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32] + \
            [ctypes.POINTER(ctypes.c_uint32)] * 6
    bufs = [np.zeros(8 + 3 + 768, np.uint8) for _ in range(16)]
    ptrs = (ctypes.c_void_p * 16)(*[b.ctypes.data for b in bufs])
    vals = [ctypes.c_uint32(0) for _ in range(6)]
    assert _seg(O.P(a), ptrs, B, *[ctypes.byref(v) for v in vals]) == 0
    C, Cp, Cm, Kp, Km, F = (v.value for v in vals)
    return [bufs[r][:(Km if r < Cm else Kp) // 8] for r in range(C)], F


def oracle_blocks(payload, tbs):
    """CRC-24A, segmentation, turbo coding and sub-block interleaving of one transport block with
    the oracle: per block a dict of K, c (bytes), d (the harq buffer: 96 NULLs, 3 K + 12 entries and
    the d[3 D + 2] side effect of the interleaver), R and w."""
    A = tbs // 8
    a = np.zeros(A + 8, np.uint8)
    a[:A] = np.asarray(payload, np.uint8)[:A]
    crc = O.crc24a(a, tbs) >> 8
    a[A:A + 3] = [(crc >> 16) & 255, (crc >> 8) & 255, crc & 255]
    cs, _ = _segmentation(a, tbs + 24)
    out = []
    for c in cs:
        K = 8 * len(c)
        d = O.turbo_encode(c, *qpp()[K])
        R, w, dbuf = O.subblock(d, K + 4)
        out.append(dict(K=K, c=c, d=dbuf[:96 + 3 * (K + 4) + 3], R=R, w=w))
    return out


def oracle_e(blocks, G, Qm, rv, subframe, Kmimo=1, rnti=RNTI, scrambled=True):
    """rate matching of every block and dlsch_scrambling (q = 0, Nid_cell = 0): the G bits of e"""
    C = len(blocks)
    e = np.concatenate([O.rate_match(b["R"], G, b["w"], C, r, Qm, rvidx=rv, Kmimo=Kmimo) for r, b in enumerate(blocks)])
    assert e.size == G
    return O.scramble(e, G, (rnti << 14) + (subframe << 9))[:G] if scrambled else e
