"""numpy restatement of the reference's fading channel: new_channel_desc_scm / fill_channel_desc
(SIMULATION/TOOLS/random_channel.c:195-860, :42-147), random_channel (:866-1015) and the non-SSE multipath_channel
(multipath_channel.c:152-219).  Checked against tests/golden/channel_ref.json (test_channel_cpu.py); the GPU tests
take their expected doubles from here."""
import math

import numpy as np

from channel_cases import MODELS

OFFSET = 4                                              # NB_SAMPLES_CHANNEL_OFFSET

# tap delays (us) and powers (dB): 3GPP TS 36.101 B.2.1 as the reference states them (:156-165)
TAPS = {
    "EPA": (0.410, (0, .03, .07, .09, .11, .19, .41), (0.0, -1.0, -2.0, -3.0, -8.0, -17.2, -20.8)),
    "EVA": (2.51, (0, .03, .15, .31, .37, .71, 1.09, 1.73, 2.51), (0.0, -1.5, -1.4, -3.6, -0.6, -9.1, -7.0, -12.0, -16.9)),
    "ETU": (5.0, (0, .05, .12, .2, .23, .5, 1.6, 2.3, 5.0), (-1.0, -1.0, -1.0, 0.0, 0.0, 0.0, -3.0, -5.0, -7.0)),
}
AMPS8 = (0.3868472, 0.3094778, 0.1547389, 0.0773694, 0.0386847, 0.0193424, 0.0096712, 0.0038685)

# scm_corrmat.h R22_sqrt: six 4x4 complex matrices, (re, im) pairs row by row
R22 = (
    (0.921700, -0.000000, 0.010380, -0.027448, -0.250153, 0.294754, 0.005961, 0.010769, 0.010380, 0.027448, 0.921700, 0.000000, -0.011595, -0.004130, -0.250153, 0.294754, -0.250153, -0.294754, -0.011595, 0.004130, 0.921700, 0.000000, 0.010380, -0.027448, 0.005961, -0.010769, -0.250153, -0.294754, 0.010380, 0.027448, 0.921700, 0.000000),
    (0.923810, 0.000000, 0.004069, 0.027832, 0.151730, 0.350180, -0.009882, 0.006114, 0.004069, -0.027832, 0.923810, 0.000000, 0.011218, -0.003029, 0.151730, 0.350180, 0.151730, -0.350180, 0.011218, 0.003029, 0.923810, -0.000000, 0.004069, 0.027832, -0.009882, -0.006114, 0.151730, -0.350180, 0.004069, -0.027832, 0.923810, 0.000000),
    (0.927613, 0.000000, 0.014253, 0.025767, -0.061171, -0.367133, 0.009258, -0.007340, 0.014253, -0.025767, 0.927613, -0.000000, -0.011138, -0.003942, -0.061171, -0.367133, -0.061171, 0.367133, -0.011138, 0.003942, 0.927613, 0.000000, 0.014253, 0.025767, 0.009258, 0.007340, -0.061171, 0.367133, 0.014253, -0.025767, 0.927613, 0.000000),
    (0.869794, -0.000000, -0.010613, -0.001218, 0.399115, 0.289852, -0.004464, -0.004096, -0.010613, 0.001218, 0.869794, -0.000000, -0.005276, -0.002978, 0.399115, 0.289852, 0.399115, -0.289852, -0.005276, 0.002978, 0.869794, -0.000000, -0.010613, -0.001218, -0.004464, 0.004096, 0.399115, -0.289852, -0.010613, 0.001218, 0.869794, 0.000000),
    (0.919726, -0.000000, 0.038700, -0.111146, 0.217804, 0.300925, 0.045531, -0.013659, 0.038700, 0.111146, 0.919726, 0.000000, -0.027201, 0.038983, 0.217804, 0.300925, 0.217804, -0.300925, -0.027201, -0.038983, 0.919726, 0.000000, 0.038700, -0.111146, 0.045531, 0.013659, 0.217804, -0.300925, 0.038700, 0.111146, 0.919726, 0.000000),
    (0.867608, -0.000000, 0.194097, -0.112414, -0.418811, 0.095938, -0.081264, 0.075727, 0.194097, 0.112414, 0.867608, -0.000000, -0.106125, -0.032801, -0.418811, 0.095938, -0.418811, -0.095938, -0.106125, 0.032801, 0.867608, 0.000000, 0.194097, -0.112414, -0.081264, -0.075727, -0.418811, -0.095938, 0.194097, 0.112414, 0.867608, 0.000000),
)
C = 0.70711
CORR = {   # (sign of the cross terms): the fully (anti-)correlated transmit pair, 2x1 and 2x2 (:169-190)
    (2, 1): lambda s: np.array([[C, s * C], [s * C, C]], dtype=complex),
    (2, 2): lambda s: np.array([[C, 0, s * C, 0], [0, C, 0, s * C], [s * C, 0, C, 0], [0, s * C, 0, C]], dtype=complex),
}


class Desc:
    pass


def describe(model, nb_tx, nb_rx, BW):
    """the descriptor of a supported model; raises ValueError where the project refuses"""
    if not (1 <= nb_tx <= 2 and 1 <= nb_rx <= 2):
        raise ValueError("antennas")
    d = Desc()
    d.model, d.nb_tx, d.nb_rx, d.BW = model, nb_tx, nb_rx, BW
    n = nb_tx * nb_rx
    eye = np.eye(n, dtype=complex)
    d.aoa, d.random_aoa, d.ricean_factor = 0.03, 0, 1.0
    if model in TAPS:
        Td, delays, dB = TAPS[model]
        amps = [math.pow(10, .1 * v) for v in dB]
        s = 0.0
        for v in amps:
            s += v
        d.amps = np.array([v / s for v in amps])
        d.delays = np.array(delays, dtype=float)
        d.channel_length = int(2 * BW * Td + 1 + 2 / (math.pi * math.pi) * math.log(4 * math.pi * BW * Td))
        d.aoa = 0.0
        # 2x2: R22_sqrt[i / 3] for tap i; any other size: identity (the reference's 1x2 / 2x1 matrices have
        # uninitialised off-diagonals and its log line says identity)
        d.R_sqrt = [np.array(r).reshape(4, 4, 2) @ np.array([1, 1j]) for r in R22] if n == 4 else [eye] * 6
    elif model in ("Rayleigh8", "Rice8"):
        Td = 0.8
        d.amps = np.array(AMPS8)
        d.delays = np.array([i * (Td / 8) for i in range(8)])
        d.channel_length = int(11 + 2 * BW * Td)
        d.R_sqrt = [eye] * 8
        if model == "Rice8":
            d.ricean_factor, d.random_aoa = 0.1, 1
    elif model in MODELS and MODELS[model] >= 10:
        d.amps, d.delays, d.channel_length = np.array([1.0]), np.array([0.0]), 1
        d.R_sqrt = [eye]
        if model.startswith("Rice1"):
            d.ricean_factor = 0.1
        if model in ("Rice1_corr", "Rice1_anticorr"):
            d.random_aoa = 1
        if model == "AWGN":
            d.ricean_factor, d.aoa = 0.0, 0.0
        if model.endswith("corr") and (nb_tx, nb_rx) in CORR:
            d.R_sqrt = [CORR[(nb_tx, nb_rx)](-1.0 if model.endswith("anticorr") else 1.0)]
    else:
        raise ValueError("model")
    d.nb_taps = len(d.amps)
    return d


def random_channel(d, a, draws, ff, first_run):
    """one call: `a` complex [nb_taps][nb_tx nb_rx] is the state (ignored on the first run); draws in the reference's
    order.  Returns (a, ch)."""
    n, it = d.nb_tx * d.nb_rx, iter(draws)
    aoa = d.aoa
    out = np.zeros((d.nb_taps, n), dtype=complex)
    for i in range(d.nb_taps):
        anew = np.zeros(n, dtype=complex)
        for aarx in range(d.nb_rx):
            for aatx in range(d.nb_tx):
                sc = math.sqrt(d.ricean_factor * d.amps[i] / 2)
                x = sc * next(it)
                y = sc * next(it)
                if i == 0 and d.ricean_factor != 1.0:
                    if d.random_aoa == 1:
                        aoa = next(it) * 2 * math.pi
                    ph = math.pi * ((aarx - aatx) * math.sin(aoa))
                    x += math.cos(ph) * math.sqrt(1.0 - d.ricean_factor)
                    y += math.sin(ph) * math.sqrt(1.0 - d.ricean_factor)
                anew[aarx + aatx * d.nb_rx] = complex(x, y)
        acorr = d.R_sqrt[i // 3] @ anew
        out[i] = acorr if first_run else math.sqrt(ff) * a[i] + math.sqrt(1 - ff) * acorr
    return out, interpolate(d, out)


def interpolate(d, a):
    """ch [nb_tx nb_rx][channel_length] from the taps' state"""
    n = d.nb_tx * d.nb_rx
    if d.channel_length == 1:
        return a[0].reshape(n, 1).copy()
    ch = np.zeros((n, d.channel_length), dtype=complex)
    for k in range(d.channel_length):
        for l in range(d.nb_taps):
            t = k - d.delays[l] * d.BW - OFFSET
            s = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
            ch[:, k] += s * a[l]
    return ch


def multipath(ch, tx, nb_rx, channel_offset=0, path_loss_dB=0.0):
    """tx float64 [nb_tx][length][2] -> float64 [nb_rx][length][2] with the reference's operation order (separate
    multiplies and adds, j outer, l inner); samples [0, |channel_offset|) are not written (NaN here)"""
    nb_tx, length, _ = tx.shape
    dd = abs(channel_offset)
    L = ch.shape[1]
    path_loss = math.pow(10, path_loss_dB / 20)
    rx = np.full((nb_rx, length, 2), np.nan)
    m = length - dd
    if m <= 0:
        return rx
    pad = np.zeros((nb_tx, L - 1 + m, 2))
    pad[:, L - 1:] = tx[:, :m]
    for ii in range(nb_rx):
        ax, ay = np.zeros(m), np.zeros(m)
        for j in range(nb_tx):
            for l in range(L):
                c = ch[ii + j * nb_rx][l]
                tx_x, tx_y = pad[j, L - 1 - l:L - 1 - l + m, 0], pad[j, L - 1 - l:L - 1 - l + m, 1]
                ax = ax + ((tx_x * c.real) - (tx_y * c.imag))
                ay = ay + ((tx_y * c.real) + (tx_x * c.imag))
        rx[ii, dd:, 0] = ax * path_loss
        rx[ii, dd:, 1] = ay * path_loss
    return rx


def to_short(v):
    """C's (short) of a double on x86: truncation toward zero through int, 16-bit wrap"""
    return np.trunc(v).astype(np.int64).astype(np.int16)
