"""Cases of the noise and tap-draw pins (tests/test_gpu_noise.py on the device, tests/test_noise_model_cpu.py on their
model side), shared so that both see the same inputs, and the one statement of where a device sample may differ from
tests/noise_model.py.

The guard.  A noisy sample is (short)(s + sigma g).  The model computes s + sigma g to about 2^-60 relative; the device
rounds log, pow, log10 and sincospi to a few ulp of a double each and may contract the last multiply-add.  (short)
truncates, so the two can differ legitimately only where the exact value lies within the device's error of an integer.
Assuming at most 4 ulp per library call (not measured for this ROCm), with |g| <= 8.6 (u53 >= 2^-53) and sigma <=
2.4e4 the device's error stays below 4e-10.  GUARD is 1e-8, about 25 times that, and the number of samples a GPU test
may leave out is zero: test_noise_model_cpu.py asserts for every case below that no component of the model lies
within GUARD of an integer, so every comparison on the device is np.array_equal over all samples.  (The chance of a
uniformly placed value falling inside is 2e-8 per component; the inputs' seeds below are ones for which none does.)
The loop cases (D) take their transmit samples from the device, so their guard assertion stands in the GPU test."""
import functools
import hashlib

import numpy as np

import channel_model as M
import noise_model as NM

GUARD = 1e-8
SEEDS = (99, 1 << 32, 0x9E3779B97F4A7C15)               # small, low word zero, both words set
SEED_BOTH = SEEDS[2]


def _rng(kind, name):
    return np.random.default_rng([20261021, kind, int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)])


def words(x16):
    """int16 [..., 2] -> packed int32 [...]"""
    return np.ascontiguousarray(x16.astype(np.int16)).view(np.int32)[..., 0]


def unwords(w):
    """packed int32 [...] -> int16 [..., 2]"""
    return np.ascontiguousarray(w, dtype=np.int32).view(np.int16).reshape(w.shape + (2,))


# ---- A: oai4g_awgn_batch ------------------------------------------------------------------------------------------
# a workgroup covers 1024 samples: one exact tile, a tile plus 1, partial last tiles, with and without the tail
A_SHAPES = ((1919, 5), (1024, 0), (1025, 0), (2047, 2), (3845, 0))
A_OFFSETS = (-3.0, -30.0)                                # at -30 dB the small levels give sigma < 1
A_N, A_FIRST, A_PAD = 8, 5, 3
A_SPLIT = ((0, 3), (3, 5))                               # the same vectors as two launches: (first, count)
# tx_lev per vector; the even vectors carry full-range samples, the odd ones +-500.  134209536 is the order of the
# largest value signal_energy returns (full-scale samples: 2 * 32767^2 >> 4)
A_LEV = np.array([1, 7, 134209536, 1000, 900, 123456, 250000, 40000], np.int32)
A_CASES = [(tx, tl, seed, off) for tx, tl in A_SHAPES for seed in SEEDS for off in A_OFFSETS]


def a_id(case):
    tx, tl, seed, off = case
    return f"{tx}+{tl}-seed{SEEDS.index(seed)}-{off:g}dB"


def a_input(case):
    """(tx int16 [8][tx_len][2], tail int16 [tail_len][2]); the full-range vectors open with the two extreme values,
    where positive / negative noise of any size wraps"""
    tx_len, tail_len, _, _ = case
    rng = _rng(1, a_id(case))
    x = rng.integers(-500, 501, (A_N, tx_len, 2)).astype(np.int16)
    x[0::2] = rng.integers(-32768, 32768, (A_N // 2, tx_len, 2)).astype(np.int16)
    x[0::2, 0:8] = 32767
    x[0::2, 8:16] = -32768
    return x, rng.integers(-500, 501, (tail_len, 2)).astype(np.int16)


@functools.lru_cache(maxsize=None)
def a_model(case):
    """(int16 [8][length][2], distance to the nearest integer [8][length][2]); computed once, not to be written to"""
    _, _, seed, off = case
    x, tail = a_input(case)
    out = [NM.awgn(np.concatenate([x[v], tail]), A_LEV[v], off, seed, A_FIRST + v) for v in range(A_N)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- B: oai4g_multipath_batch with the noise on ----------------------------------------------------------------------
B_N, B_FIRST, B_OFFSET_DB = 3, 40, -3.0
# name: (model, nb_tx, nb_rx, BW, channel_offset): channel lengths 52, 5, 27 and 14
B_CONFIGS = {"1x1": ("ETU", 1, 1, 5.0, 0), "1x2": ("EPA", 1, 2, 5.0, 0), "2x1": ("EVA", 2, 1, 5.0, 0),
             "2x2": ("ETU", 2, 2, 1.25, 3)}
# layout: (tx_len, tail_len, n_seg): "vec4" has length, seg_len and strides multiples of 4 in two segments (four samples
# leave in one 16-byte store), "odd" has an odd length and odd strides (sample by sample); both pass the 1024 tile
# The host takes the 16-byte store only when length, seg_len, rx_stride, rx_ant_stride and seg_stride are all multiples
# of 4 and d_rx is 16-byte aligned (oai4g_multipath_batch, "a.vec4 ="): b_geometry keeps "vec4" inside that condition
# and "odd" outside it, and test_noise_model_cpu.py asserts both
B_LAYOUTS = {"vec4": (1956, 100, 2), "odd": (2001, 50, 1)}
B_CASES = [(c, l) for c in B_CONFIGS for l in B_LAYOUTS]


def b_geometry(case):
    """(length, seg_len, seg_stride, rx_ant_stride, rx_stride) in samples: [vector][segment][antenna][seg_len] + pad"""
    cfg, layout = case
    nr = B_CONFIGS[cfg][2]
    tx_len, tail_len, nseg = B_LAYOUTS[layout]
    length = tx_len + tail_len
    seg = length // nseg
    ant = seg if layout == "vec4" else seg + 2
    pad = 4 if layout == "vec4" else (2 if nr == 1 else 3)      # the odd layout's vector stride is odd too
    return length, seg, nr * ant, ant, nseg * nr * ant + pad


def b_input(case, channel_length):
    """(taps complex [3][npair][channel_length], tx int16 [3][nb_tx][tx_len][2], tail int16 [nb_tx][tail_len][2],
    tx_lev int32 [3][nb_tx], different per transmit antenna)"""
    cfg, layout = case
    _, nt, nr, _, _ = B_CONFIGS[cfg]
    tx_len, tail_len, _ = B_LAYOUTS[layout]
    rng = _rng(2, cfg + layout)
    shape = (B_N, nt * nr, channel_length)
    taps = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / 2.0
    x = rng.integers(-3000, 3001, (B_N, nt, tx_len, 2)).astype(np.int16)
    tail = rng.integers(-3000, 3001, (nt, tail_len, 2)).astype(np.int16)
    lev = (2000 + 1500 * np.arange(nt)[None, :] + 700 * np.arange(B_N)[:, None]).astype(np.int32)
    return taps, x, tail, lev


def b_model(case, taps, x, tail, lev):
    """(int16 [3][nb_rx][length][2], distance [3][nb_rx][length][2]): noise_model on channel_model.multipath's doubles
    with the unwritten head as 0, stream a for receive antenna a"""
    _, nt, nr, _, off = B_CONFIGS[case[0]]
    got, dist = [], []
    for v in range(B_N):
        sig = np.concatenate([x[v], tail], axis=1).astype(np.float64)
        rx = np.nan_to_num(M.multipath(taps[v], sig, nr, off), nan=0.0)
        out = [NM.awgn_d(rx[a], np.int32(lev[v].sum()), B_OFFSET_DB, SEED_BOTH, B_FIRST + v, a) for a in range(nr)]
        got.append(np.stack([o[0] for o in out]))
        dist.append(np.stack([o[1] for o in out]))
    return np.stack(got), np.stack(dist)


@functools.lru_cache(maxsize=None)
def b_expected(case):
    """(inputs, model) of a case at its model's own channel length; computed once, not to be written to"""
    model, nt, nr, bw, _ = B_CONFIGS[case[0]]
    inp = b_input(case, M.describe(model, nt, nr, bw).channel_length)
    return inp, b_model(case, *inp)


# ---- C: oai4g_channel_random_batch from the seed ----------------------------------------------------------------------
C_N, C_FIRST, C_BW = 5, 1000, 5.0
C_MODELS = (("Rayleigh8", 1, 1), ("EPA", 2, 2), ("ETU", 1, 2), ("Rice8", 2, 2), ("Rice1_corr", 2, 1),
            ("Rayleigh1_anticorr", 2, 2))
C_FFS = (0.0, 0.5)
C_CASES = [(m, nt, nr, ff) for m, nt, nr in C_MODELS for ff in C_FFS]
C_DROP_IN = ("Rice8", 2, 2, 0.5)                         # oai4g_random_channel: seed 0, vector 0, steps 0, 1, 2


def c_model(desc, seed, vector, steps, ff):
    """[(draws, a, ch)] of the successive calls of one vector"""
    out, a = [], None
    for step in range(steps):
        d = NM.tap_draws(desc, seed, vector, step)
        a, ch = M.random_channel(desc, a, d, ff, step == 0)
        out.append((d, a, ch))
    return out


# ---- D: the BLER loop's wiring ------------------------------------------------------------------------------------------
D_MCS, D_N_RB, D_BATCH, D_ROUNDS, D_STEPS, D_SEED = 9, 25, 4, 2, 2, SEED_BOTH
D_SNR = 0.0                                              # 3.4 dB below MCS 9's AWGN waterfall: round 0 fails
