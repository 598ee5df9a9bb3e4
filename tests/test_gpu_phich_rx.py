"""GPU tests of PHICH reception (k_phich_rx) against tests/phich_rx_model.py:

  - the drop-in oai4g_rx_phich equals the model on random full-scale planes: every sequence, every group of 6 and
    25 PRB, subframes 0 / 5 / 9; the exact sum often exceeds +-32768, so the int16 wrap decides the answer (at
    least one decision differs from the unwrapped sum's sign); refusals return -1 with a message;
  - batch = drop-in: 16 items over 4 subframes whose indices cross 9 -> 0, several items per subframe, one subframe
    with none, and two items outside the batch / the mapping, which come back as refused;
  - the closed loop: batch transmitter with PHICHs (ACKs and NACKs, two groups, sequences from both halves) and
    control -> oai4g_fep_batch -> oai4g_chest_batch -> oai4g_pdcch_front_batch -> oai4g_phich_rx_batch gives every
    HI as sent with one port and the model's answers on the same compensated symbols with two.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import pdcch_front_model as F
import pdcch_rx_cases as PC
import phich_rx_model as P
from test_gpu_pdcch_front import CRNTI, RB_ALLOC, SI, _c16, _frames, _plan, _upload

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N_RB,Nid", [(6, 1), (25, 2)])
def test_gpu_rx_phich_equals_model(gpu, N_RB, Nid):
    fo, fg = _frames(gpu, N_RB, Nid, 1)
    assert fo.phich_resource == fg.phich_resource
    regs = O.phich_reg_mapping(fo)
    rng = np.random.default_rng(N_RB)
    flipped = 0
    for sf in (0, 5, 9):
        comp = _c16(rng, 36 * N_RB, 32767)
        for g in range(len(regs)):
            for q in range(8):
                nack, hi16, exact = P.rx_phich(comp, regs, g, q, Nid, sf)
                flipped += (exact > 0) != (hi16 > 0)
                assert gpu.rx_phich(fg, sf, comp, g, q) == (nack, hi16), (sf, g, q)
    assert flipped > 0
    comp = np.zeros(36 * N_RB, dtype=np.int32)
    for bad, args in ((fg, (10, comp, 0, 0)), (fg, (0, comp, len(regs), 0)), (fg, (0, comp, 0, 8)),
                      (gpu.frame_parms(N_RB, 3), (0, comp, 0, 0)), (gpu.frame_parms(N_RB, Nid, Ncp=1), (0, comp, 0, 0))):
        with pytest.raises(gpu.OAI4GError) as ei:
            gpu.rx_phich(bad, *args)
        assert str(ei.value)


def test_gpu_phich_rx_batch_equals_drop_in(gpu):
    N_RB, Nid, n_sf, first = 25, 2, 4, 8
    fo, fg = _frames(gpu, N_RB, Nid, 1)
    regs = O.phich_reg_mapping(fo)
    rng = np.random.default_rng(16)
    comp = np.stack([_c16(rng, 36 * N_RB, 32767) for _ in range(n_sf)])
    slots = [0] * 5 + [1] * 4 + [3] * 7                    # slot 2 (subframe index 0) has none
    items = [(s, int(rng.integers(0, len(regs))), int(rng.integers(0, 8))) for s in slots]
    assert len(items) == 16 and [(first + s) % 10 for s in sorted(set(slots))] == [8, 9, 1]
    bad = [(n_sf, 0, 0), (1, len(regs), 0)]
    b = gpu.PhichRxBatch(fg, items + bad, first_subframe=first, subframe_step=1)
    d_comp = _upload(gpu, comp)
    try:
        b.launch(d_comp, n_sf)
        got = b.results()
    finally:
        b.close()
        gpu.lib().oai4g_dev_free(ctypes.c_void_p(d_comp))
    for (s, g, q), (hi16, nack) in zip(items, got):
        sf = (first + s) % 10
        assert (nack, hi16) == gpu.rx_phich(fg, sf, comp[s], g, q) == P.rx_phich(comp[s], regs, g, q, Nid, sf)[:2], (s, g, q)
    assert got[16:] == [(0, 0xFF), (0, 0xFF)]


@pytest.mark.parametrize("tm2,nb_rx", [(False, 1), (True, 2)])
def test_gpu_phich_closed_loop_from_iq(gpu, tm2, nb_rx):
    N_RB, Nid, n_sf, first = 25, 2, 3, 9
    nb_tx = 2 if tm2 else 1
    fo, fg = _frames(gpu, N_RB, Nid, nb_tx)
    regs = O.phich_reg_mapping(fo)
    assert len(regs) == 4
    size, _ = _plan(N_RB)
    rng = np.random.default_rng(40 + nb_tx)
    sfs = [(first + i) % 10 for i in range(n_sf)]
    sent = [[(sf, 0, 1, 1), (sf, 0, 6, 0), (sf, 3, 4, i & 1), (sf, 3, 2, 1 - (i & 1))] for i, sf in enumerate(sfs)]
    iq = np.zeros((n_sf + 1, nb_rx, fg.samples_per_tti), dtype=np.int32)
    for i, sf in enumerate(sfs):
        items, n_common, _ = PC.tx_items(fo, sf, size, rng, CRNTI, SI)
        probe = [np.zeros(10 * fg.symbols_per_tti * fg.ofdm_symbol_size, dtype=np.int32) for _ in range(nb_tx)]
        npd = gpu.generate_dci_top(items, n_common, 512, fg, probe, sf)
        p = gpu.make_params("TM2S" if tm2 else "C1", subframe=sf, subframe_step=0, Nid_cell=Nid, with_crs=1, N_RB_DL=N_RB,
                            rb_alloc=RB_ALLOC[N_RB], nb_rb=N_RB, num_pdcch_symbols=npd)
        pipe = gpu.TxPipeline(p, 1)
        pipe.set_common(phich=sent[i])
        pipe.set_control(items, n_common)
        pipe.upload_payload(rng.integers(0, 256, size=(1, 1, p.payload_stride), dtype=np.uint8))
        pipe.run()
        pipe.sync()
        t16 = pipe.iq()[0].view(np.int16).astype(np.int64)                 # [nb_tx][2 spt]
        pipe.close()
        for a in range(nb_rx):                                             # H = [1 1] / [1 -1] over the ports
            s = t16[0] + (t16[1] if a == 0 else -t16[1]) if tm2 else t16[0]
            iq[i, a] = np.clip(s, -32768, 32767).astype(np.int16).view(np.int32)
    fep = gpu.FepBatch(fg, n_sf + 1, nb_rx)
    fb = gpu.PdcchFrontBatch(fg, n_sf, nb_rx, F.ALAMOUTI if tm2 else F.SISO, 1, first_subframe=first, subframe_step=1)
    flat = [(i, g, q) for i in range(n_sf) for (_, g, q, _) in sent[i]]
    rxb = gpu.PhichRxBatch(fg, flat, first_subframe=first, subframe_step=1)
    try:
        fep.upload(iq)
        fep.run()
        fb.estimate(fep.d_rxF)
        fb.launch(fep.d_rxF)
        rxb.launch(fb.d_comp, n_sf)
        got = rxb.results()
        comp, _, _ = fb.results()
    finally:
        rxb.close()
        fb.close()
        fep.close()
    his = [hi for i in range(n_sf) for (_, _, _, hi) in sent[i]]
    assert 0 in his and 1 in his
    for (i, g, q), hi, (hi16, nack) in zip(flat, his, got):
        assert (nack, hi16) == P.rx_phich(comp[i], regs, g, q, Nid, sfs[i])[:2], (i, g, q)
        if not tm2:
            assert nack == 1 - hi, (i, g, q, hi16)
