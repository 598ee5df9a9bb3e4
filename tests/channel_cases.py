"""Cases of the fading-channel fixture (tests/golden/channel_ref.json and .npz, written by tests/golden/gen_channel_ref.py from
the reference's own random_channel.c and multipath_channel.c) -- shared by the generator, the CPU model test and the
GPU tests, so all of them see the same scripted draws, taps and samples.

A descriptor case is (model, nb_tx, nb_rx, BW, forgetting_factor): the descriptor's tables and scalars, then `a` and
`ch` after a first and a second random_channel call fed from draws(name).  EPA / EVA / ETU at 1x2 and 2x1 are left
out: the reference leaves their correlation matrix's off-diagonals uninitialised (the project uses identity there).

A convolution case is (model, nb_tx, nb_rx, BW, channel_offset, length): multipath_channel with keep_channel = 1 on
given taps (conv_taps) and two inputs (conv_input): full-range random int16 samples, and impulses at samples 0,
channel_length - 1 and length - 1."""
import hashlib
import json
import os

import numpy as np

SEED = 20261022

# SCM_t (SIMULATION/TOOLS/defs.h:158-178): dlsim's -g letters map to these
MODELS = {"custom": 0, "SCM_A": 1, "SCM_B": 2, "SCM_C": 3, "SCM_D": 4, "EPA": 5, "EVA": 6, "ETU": 7, "MBSFN": 8,
          "Rayleigh8": 9, "Rayleigh1": 10, "Rayleigh1_800": 11, "Rayleigh1_corr": 12, "Rayleigh1_anticorr": 13,
          "Rice8": 14, "Rice1": 15, "Rice1_corr": 16, "Rice1_anticorr": 17, "AWGN": 18}
TAPPED = ("EPA", "EVA", "ETU")
EIGHT = ("Rayleigh8", "Rice8")
ONE = ("Rayleigh1", "Rayleigh1_800", "Rayleigh1_corr", "Rayleigh1_anticorr", "Rice1", "Rice1_corr", "Rice1_anticorr",
       "AWGN")
SUPPORTED = TAPPED + EIGHT + ONE
SIZES = ((1, 1), (1, 2), (2, 1), (2, 2))
BWS = (1.25, 5.0, 20.0)
FFS = (0.0, 0.5)


def _desc_cases():
    out = {}
    for m in TAPPED + EIGHT:
        for si, (nt, nr) in enumerate(SIZES):
            if m in TAPPED and nt * nr == 2:
                continue
            for bi, bw in enumerate(BWS):
                out[f"{m}_{nt}x{nr}_bw{bw:g}"] = (m, nt, nr, bw, FFS[(si + bi) & 1])
    for mi, m in enumerate(ONE):
        for si, (nt, nr) in enumerate(SIZES):
            out[f"{m}_{nt}x{nr}"] = (m, nt, nr, BWS[(mi + si) % 3], FFS[(mi + si) & 1])
    return out


DESC = _desc_cases()

# name: (model, nb_tx, nb_rx, BW, channel_offset, length)
CONV = {
    "etu6_2x2": ("ETU", 2, 2, 1.25, 0, 3840),
    "etu6_2x2_off3": ("ETU", 2, 2, 1.25, 3, 3840),
    "etu6_2x2_odd": ("ETU", 2, 2, 1.25, 0, 3839),
    "eva25_2x1": ("EVA", 2, 1, 5.0, 0, 15360),
    "etu100_1x1": ("ETU", 1, 1, 20.0, 0, 61440),
    "ray1_2x2": ("Rayleigh1", 2, 2, 5.0, 0, 3840),
}
CONV_INPUTS = ("rand", "imp")


def load_ref():
    """the fixture: channel_ref.json, with each descriptor case's "a0", "ch0", "a1", "ch1" from channel_ref.npz"""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ref = json.load(open(os.path.join(golden, "channel_ref.json")))
    with np.load(os.path.join(golden, "channel_ref.npz")) as z:
        for key in z.files:
            name, what = key.split("/")
            ref["desc"][name][what] = z[key]
    return ref


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _rng(kind, name):
    return np.random.default_rng([SEED, kind, int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)])


def n_draws(nb_taps, nb_tx, nb_rx, ricean_factor, random_aoa):
    """values one random_channel call takes: two normals per tap and antenna pair, and on tap 0 an angle per pair
    where the model draws one"""
    return nb_taps * nb_tx * nb_rx * 2 + (nb_tx * nb_rx if ricean_factor != 1.0 and random_aoa else 0)


def draws(name, call, count, n_angle_pairs=0):
    """the scripted sequence of call 0 / 1 of a descriptor case, in the reference's draw order: per tap, aarx, aatx the
    two normals x, y, and on tap 0 of a model with a random angle of arrival a uniform in [0, 1) behind them
    (n_angle_pairs = nb_tx nb_rx there, else 0)"""
    rng = _rng(1 + call, name)
    d = rng.standard_normal(count)
    for p in range(n_angle_pairs):
        d[3 * p + 2] = rng.random()
    return d


def conv_taps(name, channel_length):
    """complex128 [nb_tx nb_rx][channel_length], pair index aarx + aatx nb_rx as in the descriptor's ch"""
    _, nt, nr, _, _, _ = CONV[name]
    rng = _rng(8, name)
    return (rng.standard_normal((nt * nr, channel_length)) + 1j * rng.standard_normal((nt * nr, channel_length))) / 2.0


def conv_input(name, kind, channel_length):
    """int16 [nb_tx][length][2]"""
    _, nt, _, _, _, length = CONV[name]
    if kind == "rand":
        return _rng(9, name).integers(-32768, 32768, (nt, length, 2), dtype=np.int64).astype(np.int16)
    x = np.zeros((nt, length, 2), np.int16)
    for j in range(nt):
        x[j, 0] = (32767, -32768)
        x[j, channel_length - 1] = (-12345 + j, 321)
        x[j, length - 1] = (-32768, 32767 - j)
    return x
