"""numpy restatement of the random part of the channel stage (openair4g_amd/csrc/oai4g_channel.hip), built from its
definitions, with no device: the Philox-4x32-10 block (Salmon et al., SC'11; checked against Random123's known-answer
vectors in test_noise_model_cpu.py), u53, the Box-Muller pair, sigma from tx_lev and the offset, the noise streams of
k_awgn / k_multipath (counter (sample, vector, 0x5EED + (antenna << 16), 0xA3C5)) and the tap draws of k_channel_taps
(counter (4 tap + pair, vector, step, 0xC4A7), the angle's uniform from (0x100 + pair, vector, step, 0xC4A7)); the key
is the seed's two words everywhere.

The transcendental part runs in np.longdouble with a 64-bit mantissa and sin / cos of pi (2u) after reducing 2u to a
quadrant (the device calls sincospi, which has no argument-reduction error), so a value here is the exact one to about
2^-60 relative (test_noise_model_cpu.py measures it against mpmath).  The device rounds its library calls to a few ulp
of a double; where a device sample may therefore differ is stated once, in noise_cases.py."""
import numpy as np

import channel_model as M

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the model needs a long double with a 64-bit mantissa"

MASK = np.uint64(0xFFFFFFFF)
MUL0, MUL2 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
KEY0, KEY1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
NOISE_WORD2, NOISE_WORD3, TAP_WORD3, ANGLE_BASE = 0x5EED, 0xA3C5, 0xC4A7, 0x100
PI = LD("3.14159265358979323846264338327950288")
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """one block per element: uint64 arrays holding 32-bit words in, the four output words out (kernel order)"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0, p1 = MUL0 * c0, MUL2 * c2                       # 32 x 32 bits: the product fits the 64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + KEY0) & MASK, (k1 + KEY1) & MASK
    return c0, c1, c2, c3


def key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def u53(hi, lo):
    """(0, 1] with 53 bits, exact in float64"""
    w = (np.asarray(hi, dtype=np.uint64) << S32) | np.asarray(lo, dtype=np.uint64)
    return ((w >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def sincospi(t):
    """(sin, cos) of pi t for float64 t in [0, 2]: t = k / 2 + r with |r| <= 1 / 4 exactly, the quadrant by rotation"""
    t = np.asarray(t, dtype=np.float64)
    k = np.rint(2.0 * t)
    r = (t - 0.5 * k).astype(LD)                             # exact: k / 2 and t share their exponent range
    s, c = np.sin(PI * r), np.cos(PI * r)
    q = k.astype(np.int64) & 3
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def normals(q):
    """the Box-Muller pair (g_re, g_im) of a block's four words, long double"""
    rad = np.sqrt(LD(-2) * np.log(u53(q[0], q[1]).astype(LD)))
    sn, cs = sincospi(2.0 * u53(q[2], q[3]))
    return rad * cs, rad * sn


def sigma(lev, offset_db):
    """dlsim.c:2852-2853: sqrt(10^((10 log10(tx_lev) + offset_db) / 10) / 2), long double.  Evaluated as the same real
    number sqrt(tx_lev 10^(offset_db / 10) / 2): taken literally, the exponent of up to 8 multiplies its own rounding by
    8 ln 10 in the power, which leaves 2^-59 relative at the largest levels; this form keeps 2^-61."""
    lev = np.asarray(lev)
    assert np.all(lev > 0)
    return np.sqrt(lev.astype(LD) * np.power(LD(10), LD(float(offset_db)) / LD(10)) / LD(2))


def noise_counters(n, vector, antenna=0):
    """the counter words of samples [0, n) of one vector and receive antenna"""
    return np.arange(n, dtype=np.uint64), vector, NOISE_WORD2 + (antenna << 16), NOISE_WORD3


def noise(n, seed, vector, antenna=0):
    """the unit normals of samples [0, n): long double [n][2] (I, Q)"""
    g = normals(philox4x32_10(*noise_counters(n, vector, antenna), *key(seed)))
    return np.stack(g, axis=-1)


def awgn_d(signal, lev, offset_db, seed, vector, antenna=0):
    """signal [n][2] (I, Q) of one vector, any real dtype -> (int16 [n][2]: C's (short) of signal + sigma g, the distance
    [n][2] of the untruncated value from the nearest integer)"""
    v = np.asarray(signal).astype(LD) + sigma(lev, offset_db) * noise(len(signal), seed, vector, antenna)
    return M.to_short(v), np.abs(v - np.rint(v)).astype(np.float64)


def awgn(words, lev, offset_db, seed, vector, antenna=0):
    """awgn_d on int16 IQ words [n][2]"""
    assert np.asarray(words).dtype == np.int16
    return awgn_d(words, lev, offset_db, seed, vector, antenna)


def angles_drawn(desc):
    return desc.ricean_factor != 1.0 and desc.random_aoa == 1


def tap_counters(desc, vector, step):
    """(word 0 of the normals' counters [nb_taps][nb_rx][nb_tx] in the reference's loop order, word 0 of the angles'
    counters [nb_rx][nb_tx]), words 1..3 being (vector, step, 0xC4A7)"""
    t, aarx, aatx = np.meshgrid(np.arange(desc.nb_taps), np.arange(desc.nb_rx), np.arange(desc.nb_tx), indexing="ij")
    p = aarx + aatx * desc.nb_rx
    return (4 * t + p).astype(np.uint64), (ANGLE_BASE + p[0]).astype(np.uint64)


def tap_draws(desc, seed, vector, step):
    """the float64 draws of one random_channel call in the reference's order, as channel_model.random_channel takes
    them: per tap, aarx, aatx the two normals, and on tap 0 of a model that draws its angle the uniform behind them"""
    w0, a0 = tap_counters(desc, vector, step)
    x, y = normals(philox4x32_10(w0, vector, step, TAP_WORD3, *key(seed)))
    x, y = x.astype(np.float64), y.astype(np.float64)
    if not angles_drawn(desc):
        return np.stack([x, y], axis=-1).ravel()
    r = philox4x32_10(a0, vector, step, TAP_WORD3, *key(seed))
    first = np.stack([x[0], y[0], u53(r[0], r[1])], axis=-1).ravel()
    return np.concatenate([first, np.stack([x[1:], y[1:]], axis=-1).ravel()])
