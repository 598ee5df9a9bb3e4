"""Seeded inputs of the tail-biting Viterbi reference fixture (tests/golden/viterbi_ref.json, written
by tests/golden/gen_viterbi_ref.py from the reference's own viterbi_lte.c) — shared by the generator,
the CPU model test and the GPU test, so all of them decode the same soft bits."""
import hashlib

import numpy as np

import ctrl_rx_model as M

NS = (24, 27, 31, 40, 43, 47, 56, 61)
KINDS = ("clean", "noisy2", "noisy5", "random", "zero", "plus7", "minus8")
SIGMA = {"noisy2": 2.0, "noisy5": 5.0}     # noise on the +-7 codeword, before rounding and the clamp
SEED = 20261020


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def payload(n):
    """n - 16 seeded bits followed by their CRC16, as a DCI or the MIB is coded (ccodelte_encode with
    add_crc = 2 and RNTI 0), and the same packed MSB first as the decoder returns them"""
    rng = np.random.default_rng([SEED, n])
    a = rng.integers(0, 2, size=n - 16, dtype=np.uint8)
    crc = M.crc16(np.packbits(a), n - 16)
    bits = np.concatenate([a, np.array([(crc >> (15 - i)) & 1 for i in range(16)], dtype=np.uint8)])
    return bits, np.packbits(bits)


def soft(n, kind):
    """int8[3 n] in [-8, 7]; bit 1 is positive (viterbi_lte.c:458)"""
    rng = np.random.default_rng([SEED, n, KINDS.index(kind)])
    if kind in ("clean", "noisy2", "noisy5"):
        y = 7.0 * (2.0 * M.tbcc_encode(payload(n)[0]) - 1.0)
        if kind != "clean":
            y = y + rng.normal(0.0, SIGMA[kind], size=3 * n)
        return np.clip(np.rint(y), -8, 7).astype(np.int8)
    if kind == "random":
        return rng.integers(-8, 8, size=3 * n).astype(np.int8)
    return np.full(3 * n, {"zero": 0, "plus7": 7, "minus8": -8}[kind], dtype=np.int8)


def cases():
    for n in NS:
        for kind in KINDS:
            yield f"{n}_{kind}", n, kind, soft(n, kind)
