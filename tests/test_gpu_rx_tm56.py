"""GPU parity of the TM4-6 (single-layer precoding, MIMO modes 3..7) receive chain — the dual
extraction with pmi_ext, dlsch_channel_level (+ 1 with dl_power_off), prec2A_TM56_128 inside
dlsch_channel_compensation_TM56, dlsch_detection_mrc, the LLRs (k_rx_level_dual / k_rx_llr_prec) —
against the numpy restatement tests/rx_tm56_model.py (validated by tests/test_rx_tm56_cpu.py): the drop-in
on full-range random grids and estimates, its refusals, the batch (estimate planes and pilot rows)
against the drop-in, and receive loops on the GPU: TM4-6 TxPipeline with both ports' CRS -> channel ->
FepBatch -> 4 channel-estimation batches -> RxBatchTM56 -> RM-rx / deinterleaving / turbo decoding."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import rx_tm56_model as M
from test_rx_cpu import alloc, decode_tb, dual_alloc, n_alloc
from test_rx_tm2_cpu import qm_of

pytestmark = pytest.mark.gpu

# N_RB, Qm, PDCCH symbols, subframe, RX antennas, mode, pmi_alloc, dl_power_off, allocation
RAND = [(50, 6, 1, 0, 2, 7, 0xE4B1, 1, None),             # PBCH / SSS / PSS rows, PRB >= 32 read precoder 0
        (50, 4, 2, 5, 1, 5, 0x1B4E, 0, None),
        (25, 6, 1, 7, 2, 7, 0xE4B1, 1, None),             # odd N_RB_DL: the DC split
        (15, 2, 3, 3, 1, 3, 0x1B4E, 1, None),
        (6, 4, 3, 8, 2, 4, 0xE4B1, 0, None),
        (6, 2, 2, 5, 2, 6, 0x1B4E, 1, None),
        (50, 2, 3, 2, 2, 6, 0xE4B1, 0, [0xF0F0F0F6, 0x0002FF0F, 0, 0]),   # partial: subbands change mid-RB-run
        (25, 4, 2, 6, 1, 7, 0x1B4E, 1, None)]


def _frames(gpu, N_RB, sf):
    return (O.frame(N_RB, Nid_cell=N_RB + sf, nb_antennas_tx=2, mode1_flag=0),
            gpu.frame_parms(N_RB, Nid_cell=N_RB + sf, nb_antennas_tx=2, mode1_flag=0))


def _random(fo, nb_rx, rng, scale):
    n = fo.symbols_per_tti * fo.ofdm_symbol_size
    rx = [rng.integers(-scale, scale, n, dtype=np.int64).astype(np.int32) for _ in range(nb_rx)]
    est = {(p, a): rng.integers(-scale, scale, n, dtype=np.int64).astype(np.int32) for p in (0, 1) for a in range(nb_rx)}
    return rx, est


@pytest.mark.parametrize("N_RB,Qm,npd,sf,nb_rx,mode,pmi,poff,ra", RAND)
def test_gpu_tm56_random_inputs(gpu, N_RB, Qm, npd, sf, nb_rx, mode, pmi, poff, ra):
    ra = ra or dual_alloc(N_RB)
    fo, fg = _frames(gpu, N_RB, sf)
    rng = np.random.default_rng(N_RB * 7 + Qm + sf)
    for scale in (2 ** 31 - 1, 3000):
        rx, est = _random(fo, nb_rx, rng, scale)
        lo, so = M.rx_pdsch_tm56(fo, rx, est, ra, Qm, mode, pmi, poff, npd, sf)
        lg, sg = gpu.rx_pdsch_tm56(fg, rx, est, ra, Qm, mode, pmi, poff, npd, sf)
        assert sg == so and np.array_equal(lg, lo), (scale, so, sg)


def test_gpu_tm56_dropin_refusals(gpu):
    fo, fg = _frames(gpu, 100, 7)
    rng = np.random.default_rng(56)
    rx, est = _random(fo, 2, rng, 2 ** 31 - 1)
    low = [0xFFFFFFFF, 0xFFFFFFFF, 0, 0]                   # PRB 0..63
    lg, sg = gpu.rx_pdsch_tm56(fg, rx, est, low, 4, 7, 0xE4B1, 1, 1, 7)
    lo, so = M.rx_pdsch_tm56(fo, rx, est, low, 4, 7, 0xE4B1, 1, 1, 7)
    assert sg == so and np.array_equal(lg, lo)
    # mode 8: rx_pdsch's "Unknown MIMO mode"
    with pytest.raises(gpu.OAI4GError, match="mimo_mode 8"):
        gpu.rx_pdsch_tm56(fg, rx, est, low, 4, 8, 0xE4B1, 1, 1, 7)
    # an allocated PRB >= 64 shifts the 16-bit word by >= 32: undefined in the reference
    with pytest.raises(gpu.OAI4GError, match="undefined"):
        gpu.rx_pdsch_tm56(fg, rx, est, alloc(100), 4, 7, 0xE4B1, 1, 1, 7)
    with pytest.raises(M.Refused):
        M.rx_pdsch_tm56(fo, rx, est, alloc(100), 4, 7, 0xE4B1, 1, 1, 7)
    # ... except for pmi_alloc 0, where every reading gives precoder 0
    lg, sg = gpu.rx_pdsch_tm56(fg, rx, est, alloc(100), 4, 7, 0, 1, 1, 7)
    lo, so = M.rx_pdsch_tm56(fo, rx, est, alloc(100), 4, 7, 0, 1, 1, 7)
    assert sg == so and np.array_equal(lg, lo)


@pytest.mark.parametrize("N_RB,Qm,npd,sf,nb_rx,pmi,poff", [(50, 6, 1, 4, 2, 0xE4B1, 1), (6, 4, 3, 9, 1, 0x1B4E, 0),
                                                         (25, 2, 2, 6, 2, 0xE4B1, 1)])
def test_gpu_tm56_batch_equals_dropin(gpu, N_RB, Qm, npd, sf, nb_rx, pmi, poff):
    """n_sf = 3 consecutive subframe indices: the four ChestBatch planes + RxBatchTM56.launch equal the
    drop-in per subframe on the same planes; the pilot-row form is bit-identical."""
    fg = gpu.frame_parms(N_RB, Nid_cell=N_RB + sf, nb_antennas_tx=2, mode1_flag=0)
    n_sf, N, nsymb = 3, fg.ofdm_symbol_size, fg.symbols_per_tti
    rng = np.random.default_rng(N_RB + Qm)
    rxF = rng.integers(-2 ** 31 + 1, 2 ** 31 - 1, (n_sf + 1) * nb_rx * nsymb * N, dtype=np.int64).astype(np.int32)
    L = gpu.lib()
    d = L.oai4g_dev_alloc(rxF.nbytes)
    assert d and L.oai4g_memcpy_h2d(d, rxF.ctypes.data, rxF.nbytes) == 0
    ra = dual_alloc(N_RB)
    rx = gpu.RxBatchTM56(fg, ra, Qm, 7, pmi, npd, 0x1234, n_sf, nb_rx=nb_rx, first_subframe=sf, dl_power_off=poff)
    rx.estimate(d, first_subframe=sf)
    rx.launch(d, unscramble=0)
    a = rx.llrs()
    est = rx.estimates()                                 # [p * 2 + a][n_sf][nsymb * N]
    rx.estimate_pilots(d, first_subframe=sf)
    rx.launch_pilots(d, unscramble=0)
    b = rx.llrs()
    counts = [rx.llr_count((sf + i) % 10) for i in range(n_sf)]
    rx.close()
    L.oai4g_dev_free(ctypes.c_void_p(d))
    g = rxF.reshape(n_sf + 1, nb_rx, nsymb * N)
    for i in range(n_sf):
        e = {(p, a_): est[2 * p + a_, i] for p in (0, 1) for a_ in range(nb_rx)}
        ld, _ = gpu.rx_pdsch_tm56(fg, [g[i, a_] for a_ in range(nb_rx)], e, ra, Qm, 7, pmi, poff, npd, (sf + i) % 10)
        assert len(ld) == counts[i] and np.array_equal(a[i, :counts[i]], ld), i
    assert np.array_equal(a, b)


def _loop_alloc(N_RB):
    """the receive loops' allocation: dual_alloc without the DC RB; at 100 PRB the PRBs below 64, the
    ones for which the reference UE's shift of its 16-bit pmi_alloc is defined (so both rules run)"""
    return [0xFFFFFFFF, 0xFFFFFFFF, 0, 0] if N_RB == 100 else dual_alloc(N_RB, dc=False)


def _tm56_params(gpu, N_RB, mcs, npd, sf, mode, pmi):
    ra = _loop_alloc(N_RB)
    p = gpu.make_params("TM6", subframe=sf, N_RB_DL=N_RB, nb_rb=n_alloc(ra), rb_alloc=ra, mcs=[mcs, 0], TBS=None,
                        num_pdcch_symbols=npd, with_crs=1, mimo_mode=mode, pmi_alloc=pmi)
    p.subframe_step = 1
    return p


# N_RB, mcs, PDCCH symbols, subframe, RX antennas, rules that decode
LOOPS = [(25, 20, 1, 7, 2, (M.RULE_UE, M.RULE_TX)),      # (a) RX antenna a takes TX antenna a; the rules agree at 25 PRB
         (25, 16, 2, 3, 1, (M.RULE_UE,)),                # (b) y = sat(x0 + (x1 >> 1)): 1 + w / 2 never vanishes
         (100, 22, 1, 8, 2, (M.RULE_TX,))]               # (c) the transmitter's 8-RB subbands (PRB 0..63)


@pytest.mark.parametrize("N_RB,mcs,npd,sf,nb_rx,rules", LOOPS)
def test_gpu_tm56_receive_loop(gpu, N_RB, mcs, npd, sf, nb_rx, rules):
    n_tx, n_sf, mode, pmi = 3, 2, 7, 0xE4B1
    p = _tm56_params(gpu, N_RB, mcs, npd, sf, mode, pmi)
    pipe = gpu.TxPipeline(p, n_tx)
    rng = np.random.default_rng(mcs + N_RB)
    pay = rng.integers(0, 256, size=(n_tx, 1, p.payload_stride), dtype=np.uint8)
    pipe.upload_payload(pay)
    pipe.run()
    pipe.sync()
    iq = pipe.iq()                                      # [n_tx][2 antennas][spt]
    pipe.close()
    if nb_rx == 1:                                      # H = [1 1/2] (a plain sum cancels under precoder 1)
        t16 = iq.view(np.int16).astype(np.int64)
        s = np.clip(t16[:, 0] + (t16[:, 1] >> 1), -32768, 32767).astype(np.int16)
        iq = np.ascontiguousarray(s.view(np.int32)[:, None, :])
    fg = gpu.frame_parms(N_RB, nb_antennas_tx=2, mode1_flag=0)
    fo = O.frame(N_RB, nb_antennas_tx=2, mode1_flag=0)
    fep = gpu.FepBatch(fg, n_tx, nb_rx)
    fep.upload(iq)
    fep.run()
    rxF = fep.result()                                   # [n_tx][nb_rx][nsymb][N]
    Qm, ra = qm_of(mcs), _loop_alloc(N_RB)
    got = {}
    for rule in (M.RULE_UE, M.RULE_TX):
        rx = gpu.RxBatchTM56(fg, ra, Qm, mode, pmi, npd, p.rnti, n_sf, nb_rx=nb_rx, first_subframe=sf, pmi_rule=rule)
        rx.estimate(fep.d_rxF, first_subframe=sf)
        rx.launch(fep.d_rxF, unscramble=1)
        got[rule] = (rx.llrs(), [rx.llr_count((sf + i) % 10) for i in range(n_sf)])
        rx.close()
    fep.close()
    for i in range(n_sf):
        s_ = (sf + i) % 10
        est = {(pp, a): O.chest_subframe(fo, rxF[i, a].ravel(), rxF[i + 1, a, 0], s_, p=pp) for pp in (0, 1)
               for a in range(nb_rx)}
        for rule in rules:
            llr, G = got[rule][0][i], got[rule][1][i]
            lo, _ = M.rx_pdsch_tm56(fo, [rxF[i, a].ravel() for a in range(nb_rx)], est, ra, Qm, mode, pmi, 1, npd, s_, rule)
            u = np.zeros(32 * (1 + G // 32), np.int16)
            u[:G] = lo
            O.dlsch_unscrambling(u, G, (p.rnti << 14) + (s_ << 9) + fo.Nid_cell)
            assert len(lo) == G and np.array_equal(llr[:G], u[:G]), (s_, rule)
            res, tb = decode_tb(llr[:G], G, p.TBS[0], Qm)
            assert all(it <= 4 for it, _ in res), (s_, rule, [it for it, _ in res])
            assert np.array_equal(tb, pay[i, 0, :p.TBS[0] // 8]), (s_, rule)
        if len(rules) == 1 and N_RB == 100:
            # the reference UE's 4-RB subbands against a transmitter that used 8-RB ones: other LLRs
            G = got[M.RULE_UE][1][i]
            assert not np.array_equal(got[M.RULE_UE][0][i][:G], got[M.RULE_TX][0][i][:G])
