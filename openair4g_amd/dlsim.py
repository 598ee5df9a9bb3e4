"""dlsim's BLER loop on the GPU (openair1/SIMULATION/LTE_PHY/dlsim.c:2065-3545), batched over trials.

One trial of the reference, TM1 / SISO / one receive antenna / AWGN (`-gN`: channel_model = AWGN, value
18 of SCM_t in SIMULATION/TOOLS/defs.h:158-178, applied through multipath_channel, a single unit tap at
Ricean factor 0 -- `-gL` would be Rice8 = 14), the configuration the reference's
AWGN_results/bler_tx1_chan18_nrx1_mcs*.csv name in their file names (the reference also holds a second
set for it, AWGN/Perf_Curves_Abs/awgn_bler_tx1_mcs*.csv, 0.05-0.3 dB apart; the GPU chain follows that
one, tests/test_gpu_dlsim.py):
  - transmit (:2553-2704): generate_dci_top's PCFICH + PDCCH for one format-1 DCI (L = 1, RNTI
    0x1234; dlsim.c:1154-1157), dlsch_encoding / dlsch_scrambling / dlsch_modulation of a random
    transport block, generate_pilots, do_OFDM_mod_l of the subframe's two slots, and of the next
    subframe's first slot (which carries only its CRS, the grid being cleared each trial :2161);
  - tx_lev = signal_energy of the subframe (:2714-2719);
  - AWGN over the two subframes with sigma2_dB = 10 log10(tx_lev) + 10 log10(N / (12 NB_RB)) - SNR
    - pa_dB (:2852-2866), pa = 0 dB;
  - the UE (:2907-3260): slot_fep of both slots plus symbol 0 of the next, lte_dl_channel_estimation
    (perfect_ce = 0, high_speed_flag = 1), rx_pdsch, dlsch_unscrambling, dlsch_decoding with the
    16-bit decoder (dlsim's default, llr8_flag = 0 at dlsim.c:339; `-L` selects the 8-bit one, llr8
    here) and MAX_TURBO_ITERATIONS = 4 (PHY/CODING/defs.h:51);
  - a trial errs when dlsch_decoding returns more than max_turbo_iterations (:3330-3350).  run_batch /
    run_point run one round (the CSVs hold no retransmission counts);
  - with num_rounds = 2..4, run_steps runs dlsim's round loop (:2141, rvidx = round & 3 at :2331): a
    failed transport block is sent again with the next redundancy version and combined into the kept
    soft buffers (dlsch_decoding.c:348-383, clear = (round == 0)).  Every batch slot is a HARQ process
    with its own round, so one step carries first transmissions and retransmissions side by side.
On the GPU: TxPipeline (k_encode + k_modofdm with CRS + control) -> k_signal_energy -> k_awgn ->
k_fep over [trial][2 subframes] -> k_rx_chest (estimation + demodulation + unscrambling, elements two
subframes apart) -> k_ul_rm_deint + k_td16.  The round loop: k_encode_rv (a redundancy version per
slot) ... k_ul_rm_harq_tb (rv and clear per slot) + k_td16 -> k_harq_advance, which keeps the rounds,
dlsim's round_trials / errs counters and the payload refills on the device: a step needs no host
synchronisation.  Nothing here runs on the CPU but bookkeeping.

With channel_model (a value of SCM_t: dlsim's -g option, dlsim.c:465-525) the link is a fading channel in place of
the unit tap: ChannelBatch.draw (random_channel, a new channel every round as dlsim's hold_channel = 0 at :2150-2156
has it, unless hold_channel is asked for) and oai4g_multipath_batch (multipath_channel + the same noise) on the same
buffers, 1x1, with BW from dlsim's table (:684-703).  The default, None, runs oai4g_awgn_batch as before."""
import ctypes
import math

import numpy as np

from . import (FULL_ALLOC_25, ChannelBatch, ChestBatch, FepBatch, OAI4GError, RxBatch, TxPipeline, _check, _DeviceOwner, frame_parms,
               init, lib, make_params, normal_prefix_mod, generate_pilots, UlDecodeBatch)

DCI1_LEN = {6: 23, 15: 25, 25: 27, 50: 27, 100: 39}      # sizeof_DCI1_xMHz_FDD_t (PHY/LTE_TRANSPORT/dci.h)
FULL_ALLOC = {6: (0x3F, 0, 0, 0), 15: (0x7FFF, 0, 0, 0), 25: FULL_ALLOC_25, 50: (0xFFFFFFFF, 0x3FFFF, 0, 0),
              100: (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xF)}
CHANNEL_BW = {6: 1.25, 25: 5.0, 50: 10.0, 100: 20.0}      # dlsim.c:684-703: the BW new_channel_desc_scm is given


def qm_of(mcs):
    """get_Qm (lte_mcs.c:31)"""
    return 2 if mcs < 10 else (4 if mcs < 17 else 6)


class DlsimBler(_DeviceOwner):
    """Batched BLER trials of one (N_RB_DL, MCS) configuration; see the module docstring."""

    def __init__(self, mcs, N_RB_DL=25, batch=4096, subframe=7, num_pdcch_symbols=1, Nid_cell=0, rnti=0x1234,
                 max_iterations=4, with_dci=True, llr8=False, num_rounds=1, channel_model=None, hold_channel=False,
                 forgetting_factor=0.0):
        self.L = init()
        self.mcs, self.N_RB, self.B, self.sf = mcs, N_RB_DL, batch, subframe
        self.max_it = max_iterations
        self.Qm = qm_of(mcs)
        self.p = make_params("C2", subframe=subframe, subframe_step=0, rnti=rnti, Nid_cell=Nid_cell, with_crs=1,
                             N_RB_DL=N_RB_DL, nb_rb=N_RB_DL, rb_alloc=FULL_ALLOC[N_RB_DL], mcs=[mcs], TBS=None,
                             num_pdcch_symbols=num_pdcch_symbols)
        self.fp = frame_parms(N_RB_DL, Nid_cell=Nid_cell)
        self.spt, self.N = self.fp.samples_per_tti, self.fp.ofdm_symbol_size
        self.tx = self._own(TxPipeline(self.p, batch))
        if with_dci:
            self.L.oai4g_init_nCCE_table()
            nCCE = self.L.oai4g_get_nCCE(num_pdcch_symbols, ctypes.byref(self.fp), 1)
            ncce = self.L.oai4g_get_nCCE_offset(2, nCCE, 0, rnti, subframe)
            pdu = np.zeros(8, np.uint8)       # DCI1 content (rah 0, rballoc, mcs, ndi 1, rv 0): bits only move QPSK signs
            self.tx.set_control([(DCI1_LEN[N_RB_DL], 1, ncce, rnti, pdu)])
        # the next subframe's first slot: its CRS only (generate_pilots over the cleared grid), the
        # second slot never modulated (zeros)
        nsymb = self.fp.symbols_per_tti
        grid = np.zeros(10 * nsymb * self.N, np.int32)
        generate_pilots([grid], 512, self.fp)
        nxt = (subframe + 1) % 10
        tail = np.zeros(self.spt, np.int32)
        normal_prefix_mod(grid[nxt * nsymb * self.N:], self.fp, nsymb // 2, tail)
        self.tail = tail
        L = self.L
        self.d_tail = self._dev(tail.nbytes)
        self.d_lev = self._dev(4 * batch)
        self.fep = self._own(FepBatch(self.fp, 2 * batch, 1))
        self._put(self.d_tail, tail)
        self.ce = self._own(ChestBatch(self.fp, batch, first_subframe=subframe, subframe_step=0))
        _check(L.oai4g_chest_config_set_stride(self.ce.cfg, 2, 1) == 0)
        self.rx = self._own(RxBatch(self.fp, list(FULL_ALLOC[N_RB_DL]), self.Qm, num_pdcch_symbols, rnti, batch,
                                    first_subframe=subframe, subframe_step=0))
        self.G = self.rx.llr_count(subframe)
        self.TBS = self.p.TBS[0]
        self.dec = self._own(UlDecodeBatch(self.TBS + 24, self.G, self.Qm, batch, max_iterations=max_iterations))
        if llr8:                              # dlsim -L: dlsch_decoding with the 8-bit decoder
            _check(self.L.oai4g_ul_config_set_decoder(self.dec.cfg, 8) == 0)
        self.C = self.dec.C
        self.offset_fac = 10 * math.log10(self.N / (12.0 * N_RB_DL))
        self.chan, self.hold_channel, self._drawn = None, hold_channel, False
        if channel_model is not None:
            if N_RB_DL not in CHANNEL_BW:
                raise ValueError("dlsim gives no channel bandwidth for N_RB_DL = %d" % N_RB_DL)
            self.chan = self._own(ChannelBatch(1, 1, channel_model, CHANNEL_BW[N_RB_DL], batch,
                                               forgetting_factor=forgetting_factor))
        if not 1 <= num_rounds <= 4:
            raise ValueError("num_rounds must be 1..4 (dlsim's round loop)")
        self.num_rounds = num_rounds
        self.d_state = None
        if num_rounds > 1:
            # per-slot round state (oai4g_harq_advance): round | rv | clear | done [B] bytes each, then the
            # running trial index [B] and round_trials[4] | errs[4] as uint32
            self.tx.enable_tb_rv()
            self.dec._alloc_w()
            nb = (4 * batch + 7) & ~7
            self.d_state = self._dev(nb + 4 * batch + 32)
            self.d_round, self.d_rv = self.d_state, self.d_state + batch
            self.d_clear, self.d_done = self.d_state + 2 * batch, self.d_state + 3 * batch
            self.d_trial, self.d_counters = self.d_state + nb, self.d_state + nb + 4 * batch
            self._state_bytes = nb + 4 * batch + 32

    def sigma_offset(self, snr_db, pa_db=0.0):
        return self.offset_fac - snr_db - pa_db

    def _channel(self, snr_db, seed, first_vector, step):
        """the link of one subframe of every trial: tx_lev, then the unit tap or the fading channel, plus noise"""
        L, B, d_iq = self.L, self.B, self.tx.d_iq
        _check(L.oai4g_signal_energy_batch(d_iq, B, self.spt, self.spt, self.d_lev, None) == 0)
        if self.chan is None:
            _check(L.oai4g_awgn_batch(d_iq, self.spt, self.spt, self.d_tail, self.spt, self.fep.d_rx, 2 * self.spt, B,
                                      self.d_lev, self.sigma_offset(snr_db), seed, first_vector, None) == 0)
            return
        if not (self.hold_channel and self._drawn):       # dlsim.c:2150-2156: a new channel every round
            self.chan.draw(seed, first_vector, step)
            self._drawn = True
        self.chan.run(d_iq, self.spt, 0, self.spt, self.d_tail, self.spt, self.fep.d_rx, 2 * self.spt, 0, 2 * self.spt, 0,
                      self.d_lev, self.sigma_offset(snr_db), seed, first_vector)

    def channel_gain(self):
        """each trial's sum_k |ch[k]|^2 of the channel it last went through"""
        if self.chan is None:
            return np.ones(self.B)
        return (np.abs(self.chan.taps()[1]) ** 2).sum(axis=(1, 2))

    def run_batch(self, snr_db, seed, first_trial=0, want_bits=False, want_gain=False):
        """One batch of trials; returns the per-trial error flags (and decoded / sent bytes; with want_gain each
        trial's channel gain behind them)."""
        L, B = self.L, self.B
        self.tx.fill_payload(seed)
        self.tx.run()
        self._channel(snr_db, seed, first_trial, 0)
        self.fep.run()
        self.rx.launch_estimated(self.ce, self.fep.d_rxF, 1)
        _check(L.oai4g_ul_decode_batch(self.dec.cfg, B, self.rx.d_llr, self.rx.stride, self.dec.d_c,
                                       self.dec.c_stride, self.dec.d_it, None) == 0)
        it, c = self.dec.results()
        err = np.any(it > self.max_it, axis=1)
        out = (err, c, self.tx.download_payload()) if want_bits else (err,)
        if want_gain:
            out += (self.channel_gain(),)
        return out if len(out) > 1 else err

    def reset_rounds(self, seed):
        """Every slot at round 0 of its transport block 0: payloads oai4g_fill_payload(seed), counters 0."""
        if self.d_state is None:
            raise OAI4GError("DlsimBler was created with num_rounds = 1")
        B = self.B
        st = np.zeros(self._state_bytes, np.uint8)
        st[2 * B:3 * B] = 1                                   # clear
        self._put(self.d_state, st)
        self.tx.fill_payload(seed)
        self._seed, self._step, self._drawn = seed, 0, False

    def step(self, snr_db):
        """One subframe of every slot, enqueued without a host synchronisation: transmit with the slot's
        rv, fresh noise, receive, combine and decode with the slot's (rv, clear), advance the rounds."""
        L, B = self.L, self.B
        _check(L.oai4g_tx_batch_rv(self.tx.cfg, B, self.tx.d_payload, self.d_rv, self.tx.d_work, self.tx.d_iq,
                                   None) == 0)
        self._channel(snr_db, self._seed, self._step * B, self._step)
        self.fep.run()
        self.rx.launch_estimated(self.ce, self.fep.d_rxF, 1)
        _check(L.oai4g_ul_decode_batch_harq_tb(self.dec.cfg, B, self.rx.d_llr, self.rx.stride, self.dec.d_w,
                                               self.dec.w_stride, self.d_rv, self.d_clear, self.dec.d_c,
                                               self.dec.c_stride, self.dec.d_it, None) == 0)
        _check(L.oai4g_harq_advance(B, self.C, self.max_it, self.num_rounds, 1, self.dec.d_it, self.d_round,
                                    self.d_trial, self.d_rv, self.d_clear, self.d_done, self.d_counters,
                                    self.tx.d_payload, self.p.payload_stride, self._seed, None) == 0)
        self._step += 1

    def round_state(self):
        """(round, rv, clear, done, trial, counters) after the steps enqueued so far (synchronises)."""
        B = self.B
        st = self._get(self.d_state, self._state_bytes, np.uint8)
        nb = (4 * B + 7) & ~7
        u32 = st[nb:].view(np.uint32)
        return st[:B].copy(), st[B:2 * B].copy(), st[2 * B:3 * B].copy(), st[3 * B:4 * B].copy(), u32[:B].copy(), \
            u32[B:B + 8].copy()

    def run_steps(self, snr_db, n_steps, seed=1):
        """n_steps subframes of dlsim's round loop over the batch, from a reset state, with no host
        synchronisation between steps.  Returns dlsim's counters and figures (dlsim.c:3685-3713):
        round_trials[4], errs[4], effective_rate = round_trials[0] / sum(round_trials) and throughput =
        rate effective_rate with rate = TBS / G."""
        self.reset_rounds(seed)
        for _ in range(n_steps):
            self.step(snr_db)
        cnt = self.round_state()[5]
        rt, errs = [int(v) for v in cnt[:4]], [int(v) for v in cnt[4:]]
        eff = rt[0] / max(1, sum(rt))
        return dict(round_trials=rt, errs=errs, effective_rate=eff, rate=self.TBS / self.G,
                    throughput=self.TBS / self.G * eff)

    def tx_lev(self):
        return self._get(self.d_lev, self.B, np.int32)

    def run_point(self, snr_db, n_trials, seed=1):
        """(errors, trials) at one SNR over ceil(n_trials / batch) batches."""
        errs = trials = 0
        b = 0
        while trials < n_trials:
            e = self.run_batch(snr_db, seed * 1000003 + b, first_trial=b * self.B)
            take = min(self.B, n_trials - trials)
            errs += int(e[:take].sum())
            trials += take
            b += 1
        return errs, trials


def tb_bytes_from_blocks(c, TBS, C, K_list, F):
    """Reassemble a TB from the decoded code blocks c[r] (dlsch_decoding.c:455-490)."""
    out = []
    for r in range(C):
        kb = K_list[r] // 8
        start = (F >> 3) if r == 0 else 0
        out.append(c[r, start:kb - (3 if C > 1 else 0)])
    return np.concatenate(out)[:TBS // 8]


def wilson(k, n, z=1.96):
    """95 % binomial (Wilson) interval of k errors in n trials."""
    if n == 0:
        return 0.0, 1.0
    ph = k / n
    d = 1 + z * z / n
    c = (ph + z * z / (2 * n)) / d
    h = z * math.sqrt(ph * (1 - ph) / n + z * z / (4 * n * n)) / d
    return max(0.0, c - h), min(1.0, c + h)


__all__ = ["DlsimBler", "CHANNEL_BW", "qm_of", "wilson", "OAI4GError", "lib"]
