"""Seeded inputs of the SC-FDMA fixture (tests/golden/pusch_ref.json and pusch_ref_vectors.npz, written by
tests/golden/gen_pusch_ref.py from the reference's own lte_dfts.c and ulsch_modulation.c) — shared by the generator,
the CPU model test and the GPU tests, so all of them transform the same samples.
"""
import hashlib

import numpy as np

import pusch_model as M

SEED = 20261021
SIZES = M.SIZES
AMP = M.AMP
N_SF, N_SYM = 3, 12                       # the transform batch: 3 subframes of 12 symbols
ROWS = N_SF * N_SYM
# the input class of each of the 36 rows of a size's batch.  The reference transforms four rows per call (rows 4i..4i+3
# interleaved), so every call below mixes different columns, and the two extreme rows share theirs with ordinary ones.
CLASSES = ["full"] * 12 + ["qpsk", "qam16", "qam64", "full"] * 3 + ["impulse"] * 4 + ["max", "min", "alt", "full"] + ["qam64"] * 4
VECTOR_SIZES = (12, 24, 36, 48, 60, 72)   # full vectors are stored for these
assert len(CLASSES) == ROWS


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _qam(rng, n, Qm):
    return M.modulate(rng.integers(0, 2, n * Qm), Qm, AMP)


def dft_input(N):
    """int16 [36][N][2]: the batch of size N"""
    rng = np.random.default_rng([SEED, 1, N])
    x = np.zeros((ROWS, N, 2), dtype=np.int16)
    for i, c in enumerate(CLASSES):
        if c == "full":                   # full scale, so that the saturating and the wrapping paths differ
            x[i] = rng.integers(-32768, 32768, (N, 2))
        elif c in ("qpsk", "qam16", "qam64"):
            x[i] = _qam(rng, N, {"qpsk": 2, "qam16": 4, "qam64": 6}[c])
        elif c == "impulse":
            x[i, int(rng.integers(0, N))] = ((32767, 0), (0, -32768), (-32768, 32767), (12345, -23456))[i % 4]
        elif c == "max":
            x[i] = 32767
        elif c == "min":
            x[i] = -32768
        else:
            x[i, :, 0], x[i, :, 1] = 32767, -32768
    return x


# ulsch_modulation: (N_RB_DL, Ncp, first_rb, nb_rb, Qm, srs_active).  N_RB_DL 6 / 25 / 100, every nb_rb of the list, first_rb
# 0, an allocation that straddles the wrap at ofdm_symbol_size (first_rb < N_RB_DL / 2 < first_rb + nb_rb), and the
# largest first_rb the reference accepts (25, or what the band leaves), both prefixes, all Qm, srs on and off
MOD_CASES = [
    (6, 0, 0, 1, 2, 0), (6, 0, 2, 2, 4, 1), (6, 1, 1, 3, 6, 0), (6, 0, 5, 1, 6, 1), (6, 1, 0, 5, 2, 1), (6, 0, 2, 3, 2, 0),
    (25, 0, 0, 25, 2, 0), (25, 1, 0, 25, 4, 1), (25, 0, 11, 3, 6, 0), (25, 0, 10, 5, 4, 0), (25, 1, 12, 1, 2, 0),
    (25, 0, 24, 1, 4, 1), (25, 1, 20, 5, 6, 1), (25, 0, 23, 2, 6, 0),
    (100, 0, 0, 100, 2, 0), (100, 1, 0, 100, 6, 1), (100, 0, 0, 50, 4, 0), (100, 0, 25, 50, 6, 1), (100, 1, 25, 27, 4, 0),
    (100, 0, 24, 27, 2, 1), (100, 0, 25, 75, 6, 0), (100, 0, 20, 5, 6, 0), (100, 1, 25, 2, 2, 1), (100, 0, 25, 25, 4, 0),
    (100, 0, 3, 1, 6, 0), (100, 1, 25, 3, 4, 1),
]
# (N_RB_DL, first_rb, nb_rb) the reference runs but the library refuses: first_carrier_offset + 12 first_rb equals
# ofdm_symbol_size, where '>' does not wrap and the reference writes past the symbol (and past the frame in the last one)
MOD_PAST_SYMBOL = [(6, 3, 1), (50, 25, 2)]


def fft_size(N_RB_DL):
    return {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}[N_RB_DL]


def mod_case(i):
    """the i-th case as a dict with its seeded h (placeholders included), rnti, subframe, cell and pre-fill pattern"""
    N_RB_DL, Ncp, first_rb, nb_rb, Qm, srs = MOD_CASES[i]
    rng = np.random.default_rng([SEED, 2, i])
    nsym = len(M.pusch_symbols(Ncp, srs))
    G = 12 * nb_rb * Qm * nsym
    h = rng.integers(0, 2, G + 64).astype(np.uint8)
    # PUSCH_x / PUSCH_y runs as ulsch_encoding leaves them for 1-bit ACK / RI: [b, y, x, x...]; the second run's y is
    # bit 32, the first of a Gold word, and copies the bit scrambled with the word before; the third crosses bit 64
    for p, nx in ((Qm * int(rng.integers(12, max(13, G // Qm - 2))), Qm - 2), (31, 2), (61, 3)):
        if p + 2 + nx <= G:
            h[p + 1] = M.PUSCH_y
            h[p + 2:p + 2 + nx] = M.PUSCH_x
    return dict(N_RB_DL=N_RB_DL, N=fft_size(N_RB_DL), Ncp=Ncp, first_rb=first_rb, nb_rb=nb_rb, Qm=Qm, srs_active=srs,
                rnti=int(rng.integers(1, 65536)), subframe=int(rng.integers(0, 10)), Nid_cell=int(rng.integers(0, 504)),
                amp=AMP, h=h, G=G, nsymb=12 if Ncp else 14)


def grid_pattern(shape, salt=0):
    """the pre-fill of a grid whose untouched REs a test checks: int16 [..., 2], no two neighbours alike"""
    n = int(np.prod(shape))
    v = (np.arange(n, dtype=np.int64) * 2654435761 + 12345 + salt) & 0xFFFFFFFF
    return v.astype(np.uint32).view(np.int16).reshape(tuple(shape) + (2,)).copy()
