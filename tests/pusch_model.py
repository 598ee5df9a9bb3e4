"""numpy restatement of the reference's SC-FDMA layer: the 33 mixed-radix "PUSCH DFTs" of PHY/TOOLS/lte_dfts.c
(:3510-16087), dft_lte and ulsch_modulation (PHY/LTE_TRANSPORT/ulsch_modulation.c) and lte_idft
(ulsch_demodulation.c:58-465).  Every operation is the SSE one it restates, on int64 arrays holding int16 / int32
values, vectorised over the leading axis (one row per transform; the reference's four interleaved transforms per
call are four rows here).  Pinned against the reference's own output in tests/test_pusch_cpu.py.
"""
import numpy as np

SIZES = (12, 24, 36, 48, 60, 72, 96, 108, 120, 144, 180, 192, 216, 240, 288, 300, 324, 360, 384, 432, 480, 540, 576,
         600, 648, 720, 864, 900, 960, 972, 1080, 1152, 1200)
# the factor each dftN splits off (N = r * N/r, r sub-transforms of N/r), read from the code, not from factorisation rules
RADIX = {24: 2, 36: 3, 48: 4, 60: 5, 72: 2, 96: 2, 108: 3, 120: 2, 144: 3, 180: 3, 192: 4, 216: 3, 240: 4, 288: 3, 300: 5,
         324: 3, 360: 3, 384: 4, 432: 4, 480: 4, 540: 3, 576: 3, 600: 2, 648: 3, 720: 4, 864: 3, 900: 3, 960: 4, 972: 3,
         1080: 3, 1152: 4, 1200: 4}
# the constant of the size's final mulhi_int16: dft_norm_table[0..15] for 12..300 (12's is applied by dft_lte / lte_idft,
# not by dft12), entry 14 (18918), 16384 or ONE_OVER_SQRT2_Q15 above
_TABLE = (9459, 6689, 5461, 4729, 4230, 23170, 3344, 3153, 2991, 18918, 18918, 16384, 18918, 16384, 18918, 14654)
NORM = {N: _TABLE[i] for i, N in enumerate(SIZES[:16])}
NORM.update({N: 18918 for N in (324, 360, 540, 576, 648, 864, 900, 972, 1080)})
NORM.update({N: 16384 for N in (384, 432, 480, 720, 960, 1152, 1200)})
NORM[600] = 23170
# dft96, dft108 and dft120 call their sub-transforms (dft48, dft36, dft60) with scale_flag 0; every other size passes 1
SUB_UNSCALED = (96, 108, 120)
AMP = 512                   # impl_defs_top.h:253, dlsim's and ulsim's amplitude
QAM16 = (10362, 31086, -10362, -31086)                                # qam16_table: offset 2 b0 + b2
QAM64 = (15169, 5057, 25281, 35393, -15169, -5057, -25281, -35393)    # qam64_table: offset 4 b0 + 2 b2 + b4
PUSCH_x, PUSCH_y = 2, 3


def chain(N):
    """the radix chain from the outermost level down to the 12-point leaf"""
    out = []
    while N != 12:
        out.append(RADIX[N])
        N //= RADIX[N]
    return out


def twiddles(N):
    """int64 [r - 1][N / r - 1][2]: tw<q>[k - 1] = 32767 (cos, -sin)(2 pi q k / N), q = 1..r-1, k = 1..N/r-1;
    truncated toward zero in the tables of sizes up to 300, floor() from 324 on (the generator scripts quoted in
    lte_dfts.c use floor; the older tables were not made with them)"""
    r, M = RADIX[N], N // RADIX[N]
    th = 2 * np.pi * np.arange(1, r)[:, None] * np.arange(1, M)[None, :] / N
    v = np.stack([32767 * np.cos(th), -32767 * np.sin(th)], axis=-1)
    return (np.trunc(v) if N <= 300 else np.floor(v)).astype(np.int64)


def _s16(v):
    return np.clip(v, -32768, 32767)


def _w16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _w32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _adds(a, b):
    return _s16(a[0] + b[0]), _s16(a[1] + b[1])


def _subs(a, b):
    return _s16(a[0] - b[0]), _s16(a[1] - b[1])


def _cmult(a, b):
    """cmult (lte_dfts.c:109-121): two _mm_madd_epi16, b's imaginary part negated by a wrapping _mm_sign_epi16"""
    return _w32(a[0] * b[0] + a[1] * _w16(-b[1])), _w32(a[0] * b[1] + a[1] * b[0])


def _cpack(re, im):
    return _s16(re >> 15), _s16(im >> 15)


def _pcmult(a, b):
    return _cpack(*_cmult(a, b))


def _const(c):
    return np.int64(c[0]), np.int64(c[1])


W0 = _const((32767, 0))
W13, W23 = _const((-16384, -28378)), _const((-16384, 28378))
W15, W25, W35, W45 = _const((10126, -31163)), _const((-26509, -19260)), _const((-26510, 19260)), _const((10126, 31163))
W1_12, W2_12, W3_12, W4_12, W6_12 = (_const(c) for c in ((28377, -16383), (16383, -28377), (0, -32767), (-16383, -28377),
                                                         (-32767, 0)))


def _mac(terms):
    """cmult then cmac ...: 32-bit sums that wrap"""
    re = im = 0
    for a, b in terms:
        r, i = _cmult(a, b)
        re, im = _w32(re + r), _w32(im + i)
    return re, im


def bfly2(x0, x1, tw):
    a, b = _cmult(x0, W0), _cmult(x1, tw)
    return ((_s16(_w32(a[0] + b[0]) >> 15), _s16(_w32(a[1] + b[1]) >> 15)),
            (_s16(_w32(a[0] - b[0]) >> 15), _s16(_w32(a[1] - b[1]) >> 15)))


def bfly2_tw1(x0, x1):
    return _adds(x0, x1), _subs(x0, x1)


def _b3(x0, x1, x2):
    y0 = _adds(x0, _adds(x1, x2))
    y1 = _adds(x0, _cpack(*_mac([(x1, W13), (x2, W23)])))
    y2 = _adds(x0, _cpack(*_mac([(x1, W23), (x2, W13)])))
    return y0, y1, y2


def bfly3_tw1(x0, x1, x2):
    return _b3(x0, x1, x2)


def bfly3(x0, x1, x2, t1, t2):
    return _b3(x0, _pcmult(x1, t1), _pcmult(x2, t2))


def _flip(a):
    """_mm_sign_epi16(x, {-1, 1}) then the pair swap: (im, -re), the negation wrapping"""
    return a[1], _w16(-a[0])


def bfly4_tw1(x0, x1, x2, x3):
    s02, s13 = _adds(x0, x2), _adds(x1, x3)
    d02, d13 = _subs(x0, x2), _subs(_flip(x1), _flip(x3))
    return _adds(s02, s13), _adds(d02, d13), _subs(s02, s13), _subs(d02, d13)


def bfly4(x0, x1, x2, x3, t1, t2, t3):
    (ar, ai), (br, bi), (cr, ci) = _cmult(x1, t1), _cmult(x2, t2), _cmult(x3, t3)

    def out(re, im):
        p = _cpack(_w32(re), _w32(im))
        return _w16(x0[0] + p[0]), _w16(x0[1] + p[1])        # _mm_add_epi16 wraps

    return (out(ar + _w32(br + cr), ai + _w32(bi + ci)), out(ai - _w32(br + ci), _w32(cr - bi) - ar),
            out(_w32(br - cr) - ar, _w32(bi - ci) - ai), out(_w32(ci - br) - ai, ar - _w32(bi + cr)))


def _b5(x0, x1, x2, x3, x4):
    y0 = _adds(x0, _adds(x1, _adds(x2, _adds(x3, x4))))
    rows = ((W15, W25, W35, W45), (W25, W45, W15, W35), (W35, W15, W45, W25), (W45, W35, W25, W15))
    return (y0,) + tuple(_adds(x0, _cpack(*_mac(list(zip((x1, x2, x3, x4), w))))) for w in rows)


def bfly5_tw1(x0, x1, x2, x3, x4):
    return _b5(x0, x1, x2, x3, x4)


def bfly5(x0, x1, x2, x3, x4, t1, t2, t3, t4):
    return _b5(x0, _pcmult(x1, t1), _pcmult(x2, t2), _pcmult(x3, t3), _pcmult(x4, t4))


_TW1 = {2: bfly2_tw1, 3: bfly3_tw1, 4: bfly4_tw1, 5: bfly5_tw1}
_TW = {2: bfly2, 3: bfly3, 4: bfly4, 5: bfly5}


def mulhi(v, c):
    """mulhi_int16: _mm_slli_epi16(_mm_mulhi_epi16(a, b), 1), the low bit always clear"""
    return _w16(((v * c) >> 16) << 1)


def _dft12f(re, im):
    """[B][12] -> [B][12], unscaled (lte_dfts.c:3553-3657)"""
    x = [(re[:, i], im[:, i]) for i in range(12)]
    t = [None] * 12
    for j in range(3):
        t[j], t[3 + j], t[6 + j], t[9 + j] = bfly4_tw1(x[j], x[3 + j], x[6 + j], x[9 + j])
    y = [None] * 12
    y[0], y[4], y[8] = bfly3_tw1(t[0], t[1], t[2])
    y[1], y[5], y[9] = bfly3(t[3], t[4], t[5], W1_12, W2_12)
    y[2], y[6], y[10] = bfly3(t[6], t[7], t[8], W2_12, W4_12)
    y[3], y[7], y[11] = bfly3(t[9], t[10], t[11], W3_12, W6_12)
    return np.stack([v[0] for v in y], 1), np.stack([v[1] for v in y], 1)


def _dft(N, re, im, scale):
    if N == 12:
        return _dft12f(re, im)
    r, M = RADIX[N], N // RADIX[N]
    sub = [_dft(M, re[:, j::r], im[:, j::r], N not in SUB_UNSCALED) for j in range(r)]
    tw = twiddles(N)
    yr, yi = np.empty_like(re), np.empty_like(im)
    o0 = _TW1[r](*[(s[0][:, 0], s[1][:, 0]) for s in sub])
    ok = _TW[r](*[(s[0][:, 1:], s[1][:, 1:]) for s in sub], *[(tw[q, :, 0], tw[q, :, 1]) for q in range(r - 1)])
    for m in range(r):
        yr[:, m * M], yi[:, m * M] = o0[m]
        yr[:, m * M + 1:(m + 1) * M], yi[:, m * M + 1:(m + 1) * M] = ok[m]
    if scale:
        yr, yi = mulhi(yr, NORM[N]), mulhi(yi, NORM[N])
    return yr, yi


def dft(N, x, scale_flag=1):
    """dftN(x, y, scale_flag) on plain samples: x int16 [..., N, 2] -> int16 of the same shape.  dft12 ignores the
    flag (it has none)."""
    if N not in SIZES:
        raise ValueError(f"no dft{N} in the reference")
    x = np.asarray(x)
    v = x.reshape(-1, N, 2).astype(np.int64)
    yr, yi = _dft(N, v[:, :, 0], v[:, :, 1], bool(scale_flag))
    return np.stack([yr, yi], -1).astype(np.int16).reshape(x.shape)


def dft_lte_sym(N, x):
    """one column as dft_lte and lte_idft transform it: dftN with scale_flag 1, and for 12 the 9459 product behind dft12"""
    y = dft(N, x, 1)
    return mulhi(y.astype(np.int64), 9459).astype(np.int16) if N == 12 else y


def dft_lte(d, Msc, Nsymb):
    """d int16 [>= Nsymb * Msc][2] -> z [Nsymb * Msc][2] (the reference also transforms columns Nsymb..11, which hold
    stale data and are never mapped)"""
    d = np.asarray(d, dtype=np.int16).reshape(-1, 2)[:Nsymb * Msc]
    return dft_lte_sym(Msc, d.reshape(Nsymb, Msc, 2)).reshape(-1, 2)


def gold_words(c_init, n):
    """lte_gold_generic's 32-bit words (36.211 7.2, Nc = 1600)"""
    x1 = [1] + [0] * 30
    x2 = [(c_init >> i) & 1 for i in range(31)]
    L = 1600 + 32 * n
    for i in range(L - 31):
        x1.append(x1[i + 3] ^ x1[i])
        x2.append(x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i])
    c = np.array(x1[1600:L], dtype=np.uint8) ^ np.array(x2[1600:L], dtype=np.uint8)
    return (c.reshape(n, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def pusch_symbols(Ncp, srs_active):
    """the symbols ulsch_modulation maps, in order"""
    nsymb = 12 if Ncp else 14
    pilots = (2, 8) if Ncp else (3, 10)
    return [l for l in range(nsymb - srs_active) if l not in pilots]


def scramble(h, G, rnti, subframe, Nid_cell):
    """b_tilde[0, G) (ulsch_modulation.c:446-470)"""
    c = gold_words((rnti << 14) + (subframe << 9) + Nid_cell, 1 + (G >> 5))
    cb = ((c[:, None] >> np.arange(32, dtype=np.uint32)) & 1).ravel()[:G].astype(np.uint8)
    h = np.asarray(h, dtype=np.uint8)[:G]
    b = (h + cb) & 1
    for k in np.nonzero(h >= PUSCH_x)[0]:   # in order: PUSCH_y copies the scrambled bit before it
        b[k] = 1 if h[k] == PUSCH_x else (b[k - 1] if k else 0)
    return b


def modulate(b, Qm, amp):
    """d int16 [G / Qm][2] (ulsch_modulation.c:619-687, cooperation_flag != 2)"""
    b = np.asarray(b, dtype=np.int64).reshape(-1, Qm)
    if Qm == 2:
        g = (amp * 23170) >> 15
        return np.where(b == 1, -g, g).astype(np.int16)
    tab = np.array(QAM16 if Qm == 4 else QAM64, dtype=np.int64)
    out = np.empty((len(b), 2), dtype=np.int16)
    for c in range(2):
        idx = sum(b[:, c + 2 * i] << (Qm // 2 - 1 - i) for i in range(Qm // 2))
        out[:, c] = (amp * tab[idx]) >> 15
    return out


def ulsch_modulation(grid, amp, subframe, N_RB_DL, N, Ncp, Nid_cell, rnti, first_rb, nb_rb, Qm, srs_active, h):
    """writes the subframe's allocated REs into grid int16 [nsymb][N][2] (one subframe of txdataF[0]) and returns z.
    The reference's refusals return None with the grid untouched."""
    if nb_rb == 0 or first_rb > 25:
        return None
    syms = pusch_symbols(Ncp, srs_active)
    Msc = 12 * nb_rb
    G = Msc * Qm * len(syms)
    z = dft_lte(modulate(scramble(h, G, rnti, subframe, Nid_cell), Qm, amp), Msc, len(syms))
    off = N - 6 * N_RB_DL + 12 * first_rb
    if off > N:                             # '>': at off == N the reference runs on into the next symbol
        off -= N
    assert off != N, "the reference writes past the symbol here; the library refuses this allocation"
    re = (off + np.arange(Msc)) % N
    for j, l in enumerate(syms):
        grid[l, re] = z[j * Msc:(j + 1) * Msc]
    return z


def idft_symbols(Ncp):
    return (0, 1, 3, 4, 5, 6, 7, 9, 10, 11) if Ncp else (0, 1, 2, 4, 5, 6, 7, 8, 9, 11, 12, 13)


def _conj(v):
    """_mm_sign_epi16 by {1, -1}: an imaginary part of -32768 stays -32768"""
    out = v.copy()
    out[..., 1] = _w16(-v[..., 1].astype(np.int64)).astype(np.int16)
    return out


def lte_idft(comp, N_RB_DL, Ncp, Msc):
    """in place on comp int16 [nsymb][12 N_RB_DL][2] (rxdataF_comp[0] of one subframe): conjugate, forward transform,
    conjugate, on subcarriers < Msc of the data symbols; the pilot symbols and the rest are not touched"""
    if Msc not in SIZES:
        raise ValueError(f"no dft{Msc} in the reference")
    for l in idft_symbols(Ncp):
        comp[l, :Msc] = _conj(dft_lte_sym(Msc, _conj(comp[l, :Msc])))
    return comp


def hard_bits(y, Qm, amp, gain):
    """hard decisions of received symbols y int16 [n][2]: per component the nearest of `modulate`'s levels times `gain`
    (the real gain of the transform pair, which the receiver knows as its channel magnitude)"""
    y = np.asarray(y, dtype=np.float64)
    lv = modulate(np.array([[(i >> (Qm // 2 - 1 - k)) & 1 for k in range(Qm // 2) for _ in range(2)]
                            for i in range(1 << (Qm // 2))]).ravel(), Qm, amp)[:, 0].astype(np.float64) * gain
    out = np.empty((len(y), Qm), dtype=np.uint8)
    for c in range(2):
        idx = np.abs(y[:, c, None] - lv[None, :]).argmin(1)
        for k in range(Qm // 2):
            out[:, c + 2 * k] = (idx >> (Qm // 2 - 1 - k)) & 1
    return out.ravel()
