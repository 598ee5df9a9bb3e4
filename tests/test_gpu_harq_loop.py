"""The HARQ round state on the device (oai4g_harq_advance) and dlsim's four-round loop on it
(DlsimBler(..., num_rounds=4).step / run_steps).

(a) oai4g_harq_advance against the host model (tests/harq_model.py) on hand-made iteration arrays;
(b) three steps of a 6-slot loop at the waterfall point of test_gpu_trial_equals_oracle_trial: per
    step and slot the transmitted e bits against the oracle's for the slot's rv, the soft buffers and
    iteration counts against O.ulsch_decode_harq on the GPU's own LLRs with the slot's (rv, clear), and
    the state against the model;
(c) the loop's statistics as conditions: 1 dB below the reference curve's waterfall first
    transmissions fail and retransmissions, soft-combined, decode; at 30 dB nothing is sent twice."""
import numpy as np
import pytest

import dlsim_oracle as D
import oracle_lib as O
from harq_model import HarqState, payload_row

pytestmark = pytest.mark.gpu


class DevState:
    """the device arrays of oai4g_harq_advance for n slots, mirrored from a HarqState"""

    def __init__(self, gpu, m, C):
        self.gpu, self.L, self.m, self.C = gpu, gpu.lib(), m, C
        n = m.n
        self.sizes = dict(iters=n * C, round=n, trial=4 * n, rv=n * m.n_cw, clear=n, done=n, counters=32,
                          payload=n * m.row_bytes)
        self.d = {k: self.L.oai4g_dev_alloc(v) for k, v in self.sizes.items()}
        assert all(self.d.values())
        for k, a in (("round", m.round), ("trial", m.trial), ("rv", m.rv), ("clear", m.clear), ("done", m.done),
                     ("counters", m.counters), ("payload", m.payload)):
            a = np.ascontiguousarray(a)
            assert self.L.oai4g_memcpy_h2d(self.d[k], gpu._ptr(a), a.nbytes) == 0

    def advance(self, iters, max_it, num_rounds):
        it = np.ascontiguousarray(iters, np.uint8)
        d, m = self.d, self.m
        assert self.L.oai4g_memcpy_h2d(d["iters"], self.gpu._ptr(it), it.nbytes) == 0
        assert self.L.oai4g_harq_advance(m.n, self.C, max_it, num_rounds, m.n_cw, d["iters"], d["round"], d["trial"],
                                         d["rv"], d["clear"], d["done"], d["counters"], d["payload"], m.row_bytes,
                                         m.seed, None) == 0
        assert self.L.oai4g_sync() == 0

    def get(self, k, dtype=np.uint8):
        out = np.empty(self.sizes[k], np.uint8)
        assert self.L.oai4g_memcpy_d2h(self.gpu._ptr(out), self.d[k], out.nbytes) == 0
        return out.view(dtype)

    def close(self):
        for p in self.d.values():
            self.L.oai4g_dev_free(p)


def _same(dev, m):
    assert np.array_equal(dev.get("round"), m.round)
    assert np.array_equal(dev.get("trial", np.uint32), m.trial)
    assert np.array_equal(dev.get("rv").reshape(m.n, m.n_cw), m.rv)
    assert np.array_equal(dev.get("clear"), m.clear)
    assert np.array_equal(dev.get("done"), m.done)
    assert np.array_equal(dev.get("counters", np.uint32), m.counters)
    assert np.array_equal(dev.get("payload").reshape(m.n, m.row_bytes), m.payload)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("num_rounds", [1, 2, 4])
def test_harq_advance_equals_the_model(gpu, C, num_rounds):
    n, max_it, seed, row_bytes, n_cw = 16, 4, 0xC0FFEE + C, 2 * 48, 2
    m = HarqState(n, n_cw, row_bytes, seed)
    dev = DevState(gpu, m, C)
    try:
        # the initial rows are oai4g_fill_payload over the whole buffer
        assert gpu.lib().oai4g_fill_payload(dev.d["payload"], n * row_bytes, seed, None) == 0
        assert gpu.lib().oai4g_sync() == 0
        _same(dev, m)
        rng = np.random.default_rng(num_rounds * 10 + C)
        for call in range(3):
            iters = rng.integers(1, max_it + 1, size=(n, C)).astype(np.uint8)         # every block decodes ...
            bad = rng.random((n, C)) < 0.4
            iters[bad] = max_it + 1                                                   # ... but these
            iters[3, :] = max_it + 1                                                  # slot 3 fails every round
            iters[5, :] = 1                                                           # slot 5 never fails
            iters[7, :] = 1
            iters[7, C - 1] = max_it + 1                                              # only the last block fails
            kept = m.payload.copy()
            refilled = m.advance(iters, max_it, num_rounds)
            dev.advance(iters, max_it, num_rounds)
            _same(dev, m)
            for i in range(n):
                if i in refilled:
                    assert np.array_equal(m.payload[i], payload_row(seed, int(m.trial[i]), i, n, row_bytes))
                    assert not np.array_equal(m.payload[i], kept[i])
                else:
                    assert np.array_equal(m.payload[i], kept[i])
            if num_rounds == 1:
                assert len(refilled) == n and not m.round.any()
        if num_rounds == 4:
            assert m.round[3] == 3 and m.trial[3] == 0 and m.done[3] == 0            # three failures, the fourth round next
        assert m.trial[5] == 3
    finally:
        dev.close()


def _blocks(TBS):
    import spec_model as S
    blocks, F = S.segment([0] * (TBS + 24))
    return [len(b) for b in blocks], F


def test_three_steps_of_the_loop_equal_the_oracle(gpu):
    from openair4g_amd.dlsim import DlsimBler
    B, mcs, snr, seed = 6, 9, 3.4, 7
    sim = DlsimBler(mcs, batch=B, num_rounds=4)
    L = gpu.lib()
    try:
        Ks, _ = _blocks(sim.TBS)
        Ncb = [3 * 32 * ((K + 4 + 31) // 32) for K in Ks]
        w_o = [[np.zeros(n + 64, np.int16) for n in Ncb] for _ in range(B)]
        m = HarqState(B, 1, sim.p.payload_stride, seed)
        sim.reset_rounds(seed)
        seen = set()
        for step in range(3):
            pay = sim.tx.download_payload()
            assert np.array_equal(pay[:, 0], m.payload), step
            rv, clear = m.rv[:, 0].copy(), m.clear.copy()
            seen |= {(int(a), int(b)) for a, b in zip(rv, clear)}
            sim.step(snr)
            state = sim.round_state()                 # synchronises: for the test only
            eb = sim.tx.ebits()
            llr = np.empty((B, sim.rx.stride), np.int16)
            assert L.oai4g_memcpy_d2h(gpu._ptr(llr), sim.rx.d_llr, llr.nbytes) == 0
            it, _ = sim.dec.results()
            wg = sim.dec.soft_buffers()
            for i in range(B):
                sim.p.rvidx[0] = int(rv[i])
                try:
                    _, _, e_o = O.tx_subframe(O.tx_cfg_from_params(sim.p, sim.sf), [pay[i, 0]], want_e=True)
                finally:
                    sim.p.rvidx[0] = 0
                assert np.array_equal(gpu.unpack_bits(eb[i, 0], sim.G), e_o[0][:sim.G]), (step, i, int(rv[i]))
                ref = O.ulsch_decode_harq(llr[i, :sim.G], sim.TBS + 24, sim.G, sim.Qm, int(rv[i]), int(clear[i]), w_o[i],
                                          max_it=4)
                for r, (n_it, _) in enumerate(ref):
                    assert np.array_equal(wg[i, r, :Ncb[r]], w_o[i][r][:Ncb[r]]), (step, i, r)
                    assert it[i, r] == n_it, (step, i, r)
            m.advance(it, 4, 4)
            for got, want in zip(state, (m.round, m.rv[:, 0], m.clear, m.done, m.trial, m.counters)):
                assert np.array_equal(got, want), step
        assert len(seen) > 1, "the waterfall point gave no retransmission in three steps"
    finally:
        sim.close()


def _snr_below_waterfall(mcs):
    rows = [r for r in D.load_curves("perf_curves_abs")[mcs] if r[1] / r[2] < 0.995]
    return min(r[0] for r in rows) - 1.0


def test_loop_statistics_below_the_waterfall(gpu):
    """MCS 9, 25 PRB, 64 slots, 8 steps, 1 dB below the lowest row of the reference's Perf_Curves_Abs
    curve with BLER < 0.995: by that curve round 0 fails almost always there, and two combined
    transmissions gain 3 dB or more against the 1 dB deficit and a waterfall under 1 dB wide."""
    from openair4g_amd.dlsim import DlsimBler, tb_bytes_from_blocks
    B, mcs, steps, seed = 64, 9, 8, 11
    snr = _snr_below_waterfall(mcs)
    sim = DlsimBler(mcs, batch=B, num_rounds=4)
    try:
        Ks, F = _blocks(sim.TBS)
        sim.reset_rounds(seed)
        rnd = np.zeros(B, np.uint8)
        later_ok = later_all = 0
        for step in range(steps):
            pay = sim.tx.download_payload()
            sim.step(snr)
            state = sim.round_state()
            _, c = sim.dec.results()
            done = state[3]
            for i in np.nonzero(done == 1)[0]:
                tb = tb_bytes_from_blocks(c[i], sim.TBS, sim.C, Ks, F)
                assert np.array_equal(tb, pay[i, 0, :sim.TBS // 8]), (step, i)
            later_ok += int(np.sum((done == 1) & (rnd >= 1)))
            later_all += int(np.sum((done != 0) & (rnd >= 1)))
            rnd = state[0]
        cnt = state[5]
        rt, errs = cnt[:4].astype(int), cnt[4:].astype(int)
        print(f"SNR {snr:.2f} dB: round_trials {rt.tolist()} errs {errs.tolist()}, decoded in a later round "
              f"{later_ok}/{later_all}")
        assert rt[0] + rt[1] + rt[2] + rt[3] == B * steps
        for k in range(3):      # a block that failed round k ran round k + 1, or still waits for it
            assert rt[k + 1] == errs[k] - int(np.sum(rnd == k + 1)), (k, rt, errs)
        assert errs[0] >= 0.9 * rt[0], (rt, errs)
        assert later_all > 0 and later_ok >= 0.5 * later_all, (later_ok, later_all)
    finally:
        sim.close()


def test_loop_at_high_snr_and_single_round(gpu):
    from openair4g_amd.dlsim import DlsimBler
    B, mcs = 64, 9
    sim = DlsimBler(mcs, batch=B, num_rounds=4)
    try:
        res = sim.run_steps(30.0, 4, seed=3)
        assert res["round_trials"] == [4 * B, 0, 0, 0] and res["errs"] == [0, 0, 0, 0], res
        assert res["effective_rate"] == 1.0 and abs(res["throughput"] - sim.TBS / sim.G) < 1e-12
    finally:
        sim.close()
    snr = _snr_below_waterfall(mcs) + 1.3         # inside the waterfall: both outcomes occur
    flags = []
    for kw in ({}, {"num_rounds": 1}):
        sim = DlsimBler(mcs, batch=B, **kw)
        try:
            flags.append(sim.run_batch(snr, seed=5))
            if kw:
                with pytest.raises(gpu.OAI4GError):
                    sim.reset_rounds(1)
        finally:
            sim.close()
    assert np.array_equal(flags[0], flags[1])
