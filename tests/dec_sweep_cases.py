"""The inputs of the turbo decoder sweep (tests/test_gpu_dec_sweep.py, conditions on them in
tests/test_dec_sweep_cases_cpu.py): plain Python and the oracle, no GPU.

Both decoders pick their loop structure from the block size.  k_td16 (oai4g_decode.hip) derives from
K1 = K / 8 the forward chunks of TD_FS = 12 steps, the alpha checkpoints every TD_SEG = 6 steps, the
period-3 state layout, the number `nfast` of software-pipelined backward segments and its parity
(two-bundle prefetch), the K1 = 5 re-run, the hard-decision rounds of 32 bytes and the CRC split over
8 lanes; k_td8 (oai4g_decode8.hip) derives from K1 = K / 16 chunks of 16 and segments of 4, demux
rounds of 8, exchange rounds of 16, two hard-decision branches (K mod 128) and a CRC split over 16
lanes.  classes16 / classes8 name those, EARLIER16 / EARLIER8 are the sizes the older decoder files
run, and the batches below go to every size.

Everything is seeded by K alone, so the CPU and the GPU file build identical inputs.  The oracle
results are computed once per (decoder, K) and shared (lru_cache); callers do not modify them."""
import functools

import numpy as np

import oracle_lib as O
from ref_cases import QPP, crc_block, llrs

K16 = sorted(QPP)                                              # all 188 table sizes
K8 = [K for K in K16 if K >= 512 and K % 16 == 0]              # the 129 sizes the 8-bit decoder takes
assert len(K16) == 188 and len(K8) == 129

# sizes the earlier decoder files run, by file
EARLIER16_BY_FILE = {
    "test_gpu_decoder.py": sorted({K for K in K16 if K <= 320} | {40, 48, 512, 1024, 2048, 5504, 6144}),
    "test_gpu_decoder_cases.py": [40, 104, 512, 1024, 1056, 2048, 5504, 6144],      # ref_cases.decoder_cases
    "test_gpu_ul_chain.py": [40, 1056, 3520, 3584, 5504],      # UL[0..2] (8 x 5504; 1056; K- / K+) and TBS 16
}
EARLIER8_BY_FILE = {
    "test_gpu_decoder8.py": [512, 528, 1024, 1056, 2048, 2112, 4160, 5504, 6144],
}
EARLIER16 = sorted(set().union(*EARLIER16_BY_FILE.values()))
EARLIER8 = sorted(set().union(*EARLIER8_BY_FILE.values()))

TD_FS, TD_SEG = 12, 6


def filler_F(K):
    """the largest filler segmentation produces for a single block of size K: K - K_prev - 8"""
    i = K16.index(K)
    return K - K16[i - 1] - 8 if i else 0


def classes16(K, F=0):
    """schedule classes of k_td16 at block size K (CRC over (K - 24 - F) / 8 bytes)"""
    K1 = K // 8
    kr = K1 - 6
    nfast = kr // TD_SEG if kr > 0 else 0
    return {
        "K1 mod 12": K1 % TD_FS,
        "K1 mod 6": K1 % TD_SEG,
        "K1 mod 3": K1 % 3,
        "nfast": min(nfast, 3),
        "nfast parity": nfast & 1,
        "K1 == 5": K1 == 5,
        "K1 <= 11": K1 <= 11,
        "K/8 mod 32": (K // 8) % 32,
        "crc mod 8": ((K - 24 - F) // 8) % 8,
    }


def classes8(K, F=0):
    """schedule classes of k_td8 at block size K"""
    K1 = K // 16
    return {
        "K1 mod 16": K1 % 16,
        "K1 mod 8": K1 % 8,
        "K1 mod 4": K1 % 4,
        "K mod 128 == 0": K % 128 == 0,
        "crc mod 16": ((K - 24 - F) // 8) % 16,
    }


def class_values(fn, sizes):
    """{class name: set of values} over `sizes`"""
    out = {}
    for K in sizes:
        for name, v in fn(K).items():
            out.setdefault(name, set()).add(v)
    return out


# ---------------------------------------------------------------- the batches
AMPS = (8, 20, 40, 100, 300)            # the 8-bit decoder's input scaling shifts 0..4 (mean |y| against 16, 32, 64, 128)
LADDER = (0, 0.7, 0.85, 0.95, 1.0, 1.05, 1.1, 1.15, 1.2, 1.25, 1.3, 1.4)        # sigma / amplitude
MAIN_MAX_IT, MAIN_CRC = 8, 1
FILL_MAX_IT, FILL_CRC = 5, 0
FILL_LADDER = (0, 0.95, 1.05, 1.15)
FILL_AMP = 32
MAIN_CLEAN, MAIN_RUNG1, MAIN_UNSTRUCTURED = 0, 4, 12           # rows of the main batch (13: saturating)
FILL_CLEAN = 0                                                 # row of the filler batch (1..3 noisy, 4 unstructured)
PAD = 0x7fff


class Batch:
    """y: [n][3 K + 12] int16 rows; c: the code blocks of the codeword rows (row i < len(c))"""

    def __init__(self, K, y, c, max_it, crc_type, F):
        self.K, self.y, self.c, self.max_it, self.crc_type, self.F = K, y, c, max_it, crc_type, F
        self.y.setflags(write=False)

    def padded(self, stride):
        """the rows at `stride` entries each, the padding [3 K + 12, stride) filled with 0x7fff"""
        buf = np.full((len(self.y), stride), PAD, dtype=np.int16)
        buf[:, :self.y.shape[1]] = self.y
        return buf


@functools.lru_cache(None)
def main_batch(K):
    """14 blocks, CRC24_B, F = 0, max_iterations 8: 12 noisy codewords down the ladder with the
    amplitudes cycling, one unstructured block in +-40, one of saturating values"""
    rng = np.random.default_rng(K)
    ys, cs = [], []
    for i, rel in enumerate(LADDER):
        amp = AMPS[i % len(AMPS)]
        c = crc_block(rng, K, MAIN_CRC)
        cs.append(c)
        ys.append(llrs(O.turbo_encode(c, *QPP[K]), amp, rel * amp, rng))
    ys.append(rng.integers(-40, 41, 3 * K + 12).astype(np.int16))
    ys.append(rng.integers(-32768, 32768, 3 * K + 12).astype(np.int16))
    return Batch(K, np.stack(ys), cs, MAIN_MAX_IT, MAIN_CRC, 0)


@functools.lru_cache(None)
def filler_batch(K):
    """5 blocks, CRC24_A over the bytes from F / 8 on, F = filler_F(K), max_iterations 5: the F / 8
    filler bytes are random NON-ZERO bytes (zero ones would leave a zero CRC register unchanged and
    hide a decoder that ignores F); one clean block, three noisy, one unstructured"""
    rng = np.random.default_rng(100000 + K)
    F = filler_F(K)
    ys, cs = [], []
    for rel in FILL_LADDER:
        c = crc_block(rng, K, FILL_CRC, F).copy()
        c[:F // 8] = rng.integers(1, 256, F // 8, dtype=np.uint8)
        cs.append(c)
        ys.append(llrs(O.turbo_encode(c, *QPP[K]), FILL_AMP, rel * FILL_AMP, rng))
    ys.append(rng.integers(-40, 41, 3 * K + 12).astype(np.int16))
    return Batch(K, np.stack(ys), cs, FILL_MAX_IT, FILL_CRC, F)


W3_ROWS = 64


@functools.lru_cache(None)
def w3_rows(K):
    """64 different rows for the tiled 98 304-block launches: the main batch, the filler batch and
    further codewords down the ladder (all decoded as CRC24_B, F = 0, so the filler batch's
    codewords, coded with CRC24_A, run to the last iteration)"""
    rng = np.random.default_rng(200000 + K)
    ys = [main_batch(K).y, filler_batch(K).y]
    i = 0
    while sum(len(y) for y in ys) < W3_ROWS:
        amp = AMPS[i % len(AMPS)]
        c = crc_block(rng, K, MAIN_CRC)
        ys.append(llrs(O.turbo_encode(c, *QPP[K]), amp, LADDER[i % len(LADDER)] * amp, rng)[None])
        i += 1
    y = np.concatenate(ys)
    assert y.shape == (W3_ROWS, 3 * K + 12) and len({r.tobytes() for r in y}) == W3_ROWS
    y.setflags(write=False)
    return y


# ---------------------------------------------------------------- the expected side
DECODERS = {16: O.turbo_decode, 8: O.turbo_decode8}


def oracle_rows(bits, K, y, max_it, crc_type, F):
    """(iterations [n] uint8, bytes [n][K / 8]) of the oracle over the rows of y"""
    res = [DECODERS[bits](row, K, max_it=max_it, crc_type=crc_type, F=F) for row in y]
    its = np.array([r[0] for r in res], dtype=np.uint8)
    out = np.stack([r[1] for r in res])
    its.setflags(write=False)
    out.setflags(write=False)
    return its, out


@functools.lru_cache(None)
def oracle_main(bits, K):
    b = main_batch(K)
    return oracle_rows(bits, K, b.y, b.max_it, b.crc_type, b.F)


@functools.lru_cache(None)
def oracle_filler(bits, K):
    b = filler_batch(K)
    return oracle_rows(bits, K, b.y, b.max_it, b.crc_type, b.F)
