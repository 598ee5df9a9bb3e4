"""Host model of oai4g_harq_advance (k_harq_advance) and of the device payload generator it refills
rows with (k_fill: 8-byte word w of the stream of `seed` is splitmix64's output for seed + gamma (w + 1))."""
import numpy as np

GAMMA = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def fill_words(seed, w0, n):
    """words w0 .. w0 + n - 1 of the oai4g_fill_payload stream of `seed`, as bytes (little-endian)"""
    out = np.empty(n, np.uint64)
    for k in range(n):
        z = (seed + GAMMA * (w0 + k + 1)) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        out[k] = z ^ (z >> 31)
    return out.view(np.uint8)


def payload_row(seed, trial, slot, n_slots, row_bytes):
    """the row of transport block `trial` of `slot`: row trial n_slots + slot of the stream"""
    rw = row_bytes // 8
    return fill_words(seed, (trial * n_slots + slot) * rw, rw)


class HarqState:
    """round, trial, rv, clear, done per slot, counters = round_trials[4] | errs[4], payload rows"""

    def __init__(self, n_slots, n_cw, row_bytes, seed):
        self.n, self.n_cw, self.row_bytes, self.seed = n_slots, n_cw, row_bytes, seed
        self.round = np.zeros(n_slots, np.uint8)
        self.trial = np.zeros(n_slots, np.uint32)
        self.rv = np.zeros((n_slots, n_cw), np.uint8)
        self.clear = np.ones(n_slots, np.uint8)
        self.done = np.zeros(n_slots, np.uint8)
        self.counters = np.zeros(8, np.uint32)
        self.payload = np.stack([payload_row(seed, 0, i, n_slots, row_bytes) for i in range(n_slots)])

    def advance(self, iters, max_it, num_rounds):
        """iters [n_slots][C]; returns the slots whose rows were refilled"""
        refilled = []
        for i in range(self.n):
            fail = bool(np.any(np.asarray(iters[i]) > max_it))
            rnd = int(self.round[i])
            self.counters[rnd] += 1
            if fail:
                self.counters[4 + rnd] += 1
            if fail and rnd + 1 < num_rounds:
                self.round[i] = rnd + 1
                self.done[i] = 0
            else:
                self.round[i] = 0
                self.done[i] = 2 if fail else 1
                self.trial[i] += 1
                self.payload[i] = payload_row(self.seed, int(self.trial[i]), i, self.n, self.row_bytes)
                refilled.append(i)
            self.rv[i, :] = self.round[i] & 3
            self.clear[i] = 1 if self.round[i] == 0 else 0
        return refilled
