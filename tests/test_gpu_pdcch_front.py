"""GPU tests of the PDCCH / PCFICH receive front end (k_pdcch_front) and the DCI search behind it
(oai4g_pdcch_rx_batch_detected), against tests/pdcch_front_model.py:

  - the drop-in oai4g_rx_pdcch_front bit-exact on every defined word (plane 0, the four planes before MRC,
    log2_maxh, the detected count; the undefined tail of symbol 0 is 0): N_RB 6 / 15 / 25 with the three pilot
    shifts, (TX, RX) in 1x1, 2x1, 1x2, 2x2, both high_speed_flag values, a different gain per port and antenna
    (a strong port 1 with 2x1 does not raise log2_maxh);
  - saturation and wrap: a small symbol-1 estimate row keeps log2_maxh low while rows 0 / 2 and the samples are
    large, so packs_epi32 saturates in the compensation; the MRC's adds_epi16(a >> 1, b >> 1) cannot saturate
    (both halves lie in [-16384, 16383]), so the test asserts what it can reach, its extremes 32766 and -32768,
    from two saturated antennas; with two ports the Alamouti sums then wrap; two deterministic REs carry the
    32-bit wrap of the dot product (h = y = -32768 - 32768j) and the int16 negation of h.im = -32768.  Each is
    asserted from the model before the comparison;
  - batch = drop-in over 8 subframes whose indices cross 9 -> 0, N_RB 25, 2x2;
  - PCFICH: the oracle transmitter's grid through a flat channel with a complex gain per port and antenna is
    detected as sent, N_RB 6 / 25, counts 1..3, one and two ports; the all-below plane gives 3;
  - the closed loop from IQ: batch transmitter with control -> oai4g_fep_batch -> oai4g_chest_batch per port and
    antenna -> oai4g_pdcch_front_batch -> oai4g_pdcch_rx_batch_detected returns the DCIs that were sent (payload,
    RNTI, first CCE, format, and the level of the common DCI; the level of the UE DCIs, which an earlier and
    narrower pass of the plan may decode from their first CCEs, and everything else as the model's search on the
    same symbols), with the count varying inside the batch;
  - oai4g_pdcch_rx_batch_detected equals oai4g_pdcch_rx_batch when every subframe carries the same count.
"""
import ctypes

import numpy as np
import pytest

import ctrl_rx_model as M
import oracle_lib as O
import pdcch_front_model as F
import pdcch_rx_cases as PC

pytestmark = pytest.mark.gpu

CRNTI, SI, RA = 0x1234, 0xFFFF, 0x0002
RB_ALLOC = {6: [0x3F, 0, 0, 0], 25: [0x1FFFFFF, 0, 0, 0]}


def _frames(gpu, N_RB, Nid, nb_tx):
    kw = dict(nb_antennas_tx=2, mode1_flag=0) if nb_tx == 2 else {}
    fo, fg = O.frame(N_RB, Nid, **kw), gpu.frame_parms(N_RB, Nid, **kw)
    assert fg.nb_antennas_tx_eNB == nb_tx == fo.nb_antennas_tx_eNB
    return fo, fg


def _c16(rng, n, amp):
    return rng.integers(-amp, amp + 1, 2 * n).astype(np.int16).view(np.int32)


def _same_front(got, want, planes=True):
    comp, l2, cfi = got[:3]
    d = want["defined"]
    assert l2 == want["log2_maxh"]
    assert np.array_equal(comp[d], want["comp"][d])
    assert not comp[~d].any()
    assert cfi == want["cfi"]
    if planes:
        for (p, a), pl in want["planes"].items():
            assert np.array_equal(got[3][2 * p + a][d], pl[d]), (p, a)


GAIN = {(0, 0): 100, (1, 0): 900, (0, 1): 300, (1, 1): 500}


@pytest.mark.parametrize("N_RB,Nid", [(6, 0), (15, 1), (25, 2)])
@pytest.mark.parametrize("nb_tx,nb_rx", [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("hs", [0, 1])
def test_gpu_front_drop_in_equals_model(gpu, N_RB, Nid, nb_tx, nb_rx, hs):
    fo, fg = _frames(gpu, N_RB, Nid, nb_tx)
    assert fo.nushift % 3 == Nid
    n = fo.symbols_per_tti * fo.ofdm_symbol_size
    rng = np.random.default_rng(N_RB * 64 + nb_tx * 8 + nb_rx * 2 + hs)
    rx = [_c16(rng, n, 3000) for _ in range(nb_rx)]
    est = {(p, a): _c16(rng, n, GAIN[(p, a)]) for p in range(nb_tx) for a in range(nb_rx)}
    sf = (N_RB + hs) % 10
    for mode in ([F.SISO, F.ALAMOUTI] if nb_tx == 2 else [F.SISO]):
        want = F.rx_pdcch_front(fo, rx, est, sf, mode, hs)
        assert all(12 * N_RB * v < 2 ** 29 for v in want["avg"].values())       # the level's sum stays defined
        if (nb_tx, nb_rx) == (2, 1):                                            # the strong port 1 is not looked at
            assert want["avg"][(1, 0)] > 16 * want["avg"][(0, 0)]
            assert want["log2_maxh"] == F.log2_approx(want["avg"][(0, 0)]) // 2 + 6
            assert F.log2_approx(want["avg"][(1, 0)]) // 2 > F.log2_approx(want["avg"][(0, 0)]) // 2
        _same_front(gpu.rx_pdcch_front(fg, rx, est, sf, mode, hs, diag=True), want)
        if N_RB != 15 and hs == 1:                       # rx_pdcch whole: the soft bits of the detected count (15 PRB: no PDCCH geometry)
            e, n = gpu.rx_pdcch(fg, rx, est, sf, mode, hs)
            assert n == want["cfi"]
            assert np.array_equal(e, M.pdcch_soft_bits(want["comp"][:n * 12 * N_RB], PC.model_table(fo, sf, n)))


@pytest.mark.parametrize("nb_tx,nb_rx,mode", [(1, 2, F.SISO), (2, 2, F.ALAMOUTI)])
def test_gpu_front_saturation_and_wrap(gpu, nb_tx, nb_rx, mode):
    N_RB, Nid, sf = 6, 4, 3
    fo, fg = _frames(gpu, N_RB, Nid, nb_tx)
    N, n = fo.ofdm_symbol_size, fo.symbols_per_tti * fo.ofdm_symbol_size
    rng = np.random.default_rng(77 + nb_tx)
    rx = [_c16(rng, n, 32767) for _ in range(nb_rx)]
    est = {}
    for p in range(nb_tx):
        for a in range(nb_rx):
            e = _c16(rng, n, 32767)
            e[N:2 * N] = _c16(rng, N, 16)                                       # the row the level is taken from
            est[(p, a)] = e
    # two deterministic REs of symbol 2 on every plane: h = y = -32768 - 32768j, where both dot products are 2^31 and
    # wrap to -2^31 (a clamping dot product would give 2^31 - 1), and h = -32768j, y = 1, where the int16 negation
    # of h.im stays -32768 (a wider one would give +32768)
    rxw, chw = F.extract_map(N_RB, N, fo.first_carrier_offset, fo.nushift, 2, nb_tx > 1)
    e0, e1 = 17, 40
    lo = np.array([-32768, -32768], dtype=np.int16).view(np.int32)[0]
    for a in range(nb_rx):
        rx[a][2 * N + rxw[e0]] = lo
        rx[a][2 * N + rxw[e1]] = 1
        for p in range(nb_tx):
            est[(p, a)][2 * N + chw[e0]] = lo
            est[(p, a)][2 * N + chw[e1]] = np.array([0, -32768], dtype=np.int16).view(np.int32)[0]
    want = F.rx_pdcch_front(fo, rx, est, sf, mode, 1)
    d = want["defined"]
    assert want["log2_maxh"] <= 11
    for v in want["planes"].values():
        w0, w1 = v[24 * N_RB + e0:24 * N_RB + e0 + 1].view(np.int16), v[24 * N_RB + e1:24 * N_RB + e1 + 1].view(np.int16)
        assert w0.tolist() == [-32768, -32768]                                  # (-2^31) >> shift, saturated downwards
        assert w1.tolist() == [0, -32768 >> want["log2_maxh"]] and w1[1] < 0
    pl = {k: v[d].view(np.int16) for k, v in want["planes"].items()}
    assert all((v == 32767).any() and (v == -32768).any() for v in pl.values())   # packs_epi32 saturates
    comb = {p: F.mrc(want["planes"][(p, 0)], want["planes"][(p, 1)])[d].view(np.int16) for p in range(nb_tx)}
    assert all((v == 32766).any() and (v == -32768).any() for v in comb.values())  # all the MRC's adds can reach
    if mode == F.ALAMOUTI:
        a, b = comb[0].astype(np.int64).reshape(-1, 2, 2), comb[1].astype(np.int64).reshape(-1, 2, 2)
        assert (np.abs(a[:, 0, 0] + b[:, 1, 0]) > 32768).any() and (np.abs(a[:, 1, 0] - b[:, 0, 0]) > 32768).any()
    _same_front(gpu.rx_pdcch_front(fg, rx, est, sf, mode, 1, diag=True), want)


def _upload(gpu, a):
    a = np.ascontiguousarray(a)
    d = gpu.lib().oai4g_dev_alloc(a.nbytes)
    assert d and gpu.lib().oai4g_memcpy_h2d(d, a.ctypes.data, a.nbytes) == 0
    return d


def test_gpu_front_batch_equals_drop_in(gpu):
    N_RB, Nid, n_sf, first = 25, 137, 8, 6
    fo, fg = _frames(gpu, N_RB, Nid, 2)
    n = fo.symbols_per_tti * fo.ofdm_symbol_size
    rng = np.random.default_rng(8)
    rx = np.stack([[_c16(rng, n, 3000) for _ in range(2)] for _ in range(n_sf)])          # [n_sf][2][n]
    est = {(p, a): np.stack([_c16(rng, n, GAIN[(p, a)] * (1 + i % 3)) for i in range(n_sf)]) for p in (0, 1) for a in (0, 1)}
    fb = gpu.PdcchFrontBatch(fg, n_sf, 2, F.ALAMOUTI, 1, first_subframe=first, subframe_step=1)
    d_rx = _upload(gpu, rx)
    try:
        fb.upload_estimates(est)
        fb.launch(d_rx)
        comp, cfi, l2 = fb.results()
    finally:
        fb.close()
        gpu.lib().oai4g_dev_free(ctypes.c_void_p(d_rx))
    sfs = [(first + i) % 10 for i in range(n_sf)]
    assert 9 in sfs and 0 in sfs
    for i, sf in enumerate(sfs):
        e = {k: v[i] for k, v in est.items()}
        c1, l1, n1 = gpu.rx_pdcch_front(fg, list(rx[i]), e, sf, F.ALAMOUTI, 1)
        assert np.array_equal(comp[i], c1) and (cfi[i], l2[i]) == (n1, l1), sf
        _same_front((comp[i], int(l2[i]), int(cfi[i])), F.rx_pdcch_front(fo, list(rx[i]), e, sf, F.ALAMOUTI, 1), planes=False)
    assert len(set(l2.tolist())) > 1


H = {(0, 0): 300 + 200j, (1, 0): -150 + 260j, (0, 1): 90 - 310j, (1, 1): -280 - 120j}


def _through(grids, sf, fo, nb_rx):
    """subframe `sf` of the transmit grids through the flat channel H: y_a = sum_p (H[p, a] x_p) >> 8, exact
    integers; the estimates are H itself on every RE"""
    n = fo.symbols_per_tti * fo.ofdm_symbol_size
    rx, est = [], {}
    for a in range(nb_rx):
        acc = np.zeros((n, 2), dtype=np.int64)
        for p, g in enumerate(grids):
            x = np.asarray(g[sf * n:(sf + 1) * n], dtype=np.int32).view(np.int16).astype(np.int64).reshape(-1, 2)
            hr, hi = int(H[(p, a)].real), int(H[(p, a)].imag)
            acc[:, 0] += hr * x[:, 0] - hi * x[:, 1]
            acc[:, 1] += hr * x[:, 1] + hi * x[:, 0]
            e = np.empty((n, 2), dtype=np.int16)
            e[:, 0], e[:, 1] = hr, hi
            est[(p, a)] = e.reshape(-1).view(np.int32).copy()
        rx.append((acc >> 8).astype(np.int16).reshape(-1).view(np.int32).copy())
    return rx, est


@pytest.mark.parametrize("N_RB", [6, 25])
@pytest.mark.parametrize("nb_tx,nb_rx", [(1, 1), (2, 2)])
def test_gpu_pcfich_detected_as_sent(gpu, N_RB, nb_tx, nb_rx):
    Nid = 137
    fo, fg = _frames(gpu, N_RB, Nid, nb_tx)
    mode = F.ALAMOUTI if nb_tx == 2 else F.SISO
    for cfi in (1, 2, 3):
        for sf in (0, 7):
            grids = [np.zeros(10 * fo.symbols_per_tti * fo.ofdm_symbol_size, dtype=np.int32) for _ in range(nb_tx)]
            O.generate_pcfich(cfi, 1024, fo, grids, sf)
            rx, est = _through(grids, sf, fo, nb_rx)
            want = F.rx_pdcch_front(fo, rx, est, sf, mode, 1)
            assert want["cfi"] == cfi
            comp, _, n = gpu.rx_pdcch_front(fg, rx, est, sf, mode, 1)
            assert n == cfi and gpu.rx_pcfich(fg, sf, comp, mode) == cfi
    below = F.pcfich_plane_below(N_RB, Nid, 4)
    assert all(m < -16384 for m in F.pcfich_metrics(below, N_RB, Nid, 4))
    assert gpu.rx_pcfich(fg, 4, below, mode) == 3


def _same(res, st):
    assert (res.dci_cnt, res.format0_found, res.format_c_found, res.nCCE, res.overflow) == \
        (st["cnt"], st["f0"], st["fc"], st["nCCE"], st["ovf"])
    assert list(res.CCEmap) == st["maps"]
    for i in range(st["cnt"]):
        ln, L, cce, rnti, fmt, pdu = st["alloc"][i]
        d = res.dci[i]
        assert (d.dci_length, d.L, d.nCCE, d.rnti, d.format, bytes(d.dci_pdu)[:len(pdu)]) == (ln, L, cce, rnti, fmt, pdu), i


def _plan(N_RB):
    size = 27 if N_RB > 6 else 21
    return size, (PC.tm1_plan(size, 13, size, 31) if N_RB > 6 else [(0, 0, size, 4, 2, 2, 0, 0), (0, 1, size, 4, 2, 2, 0, 0)])


def _reduced(fo, sf, items, keep):
    """the DCIs of `items` whose aggregation level is in `keep`, placed anew in the smallest control region that
    holds them (first free candidate of each search space)"""
    sel = [it for it in items if it[1] in keep]
    total = sum(1 << it[1] for it in sel)
    for npd in (1, 2, 3):
        nCCE = O.get_nCCE(npd, fo, 1)
        if nCCE < total:
            continue
        taken, out = set(), []
        for size, L, _, rnti, pdu in sel:
            cce = next((c for c in M.candidates(nCCE, O.get_nCCE(3, fo, 1), int(rnti == SI), L, CRNTI, sf)
                        if not taken & set(range(c, c + (1 << L)))), None)
            if cce is None:
                break
            taken |= set(range(cce, cce + (1 << L)))
            out.append((size, L, cce, rnti, pdu))
        else:
            return out, sum(1 for it in out if it[3] == SI), npd
    raise AssertionError("no placement")


@pytest.mark.parametrize("N_RB,tm2,nb_rx", [(6, False, 1), (6, True, 1), (25, False, 1), (25, True, 2)])
def test_gpu_closed_loop_from_iq(gpu, N_RB, tm2, nb_rx):
    Nid, n_sf, first = 137, 4, 8
    nb_tx = 2 if tm2 else 1
    fo, fg = _frames(gpu, N_RB, Nid, nb_tx)
    assert fo.phich_resource == fg.phich_resource
    size, plan = _plan(N_RB)
    rng = np.random.default_rng(N_RB + nb_tx)
    sfs = [(first + i) % 10 for i in range(n_sf)]
    spt = fg.samples_per_tti
    iq = np.zeros((n_sf + 1, nb_rx, spt), dtype=np.int32)
    sent, npds = [], []
    for i, sf in enumerate(sfs):
        items, n_common, placed_for = PC.tx_items(fo, sf, size, rng, CRNTI, SI)
        if i & 1:                                                          # a smaller set: fewer control symbols
            items, n_common, placed_for = _reduced(fo, sf, items, {0} if N_RB == 6 else {0, 2})
        probe = [np.zeros(10 * fg.symbols_per_tti * fg.ofdm_symbol_size, dtype=np.int32) for _ in range(nb_tx)]
        npd = gpu.generate_dci_top(items, n_common, 512, fg, probe, sf)
        assert npd == placed_for
        p = gpu.make_params("TM2S" if tm2 else "C1", subframe=sf, subframe_step=0, Nid_cell=Nid, with_crs=1, N_RB_DL=N_RB,
                            rb_alloc=RB_ALLOC[N_RB], nb_rb=N_RB, num_pdcch_symbols=npd)
        pipe = gpu.TxPipeline(p, 1)
        pipe.set_control(items, n_common)
        pipe.upload_payload(rng.integers(0, 256, size=(1, 1, p.payload_stride), dtype=np.uint8))
        pipe.run()
        pipe.sync()
        t16 = pipe.iq()[0].view(np.int16).astype(np.int64)                 # [nb_tx][2 spt]
        pipe.close()
        for a in range(nb_rx):                                             # H = [1 1] / [1 -1] over the ports
            s = t16[0] + (t16[1] if a == 0 else -t16[1]) if tm2 else t16[0]
            iq[i, a] = np.clip(s, -32768, 32767).astype(np.int16).view(np.int32)
        sent.append(items)
        npds.append(npd)
    assert len(set(npds)) > 1, npds
    fep = gpu.FepBatch(fg, n_sf + 1, nb_rx)
    fb = gpu.PdcchFrontBatch(fg, n_sf, nb_rx, F.ALAMOUTI if tm2 else F.SISO, 1, first_subframe=first, subframe_step=1)
    srch = gpu.PdcchRxBatchDetected(fg, CRNTI, SI, RA, plan, n_sf)
    try:
        fep.upload(iq)
        fep.run()
        fb.estimate(fep.d_rxF)
        fb.launch(fep.d_rxF)
        srch.launch(fb.d_comp, fb.d_cfi, first_subframe=first, subframe_step=1)
        res = srch.results()
        comp, cfi, _ = fb.results()
    finally:
        srch.close()
        fb.close()
        fep.close()
    assert cfi.tolist() == npds
    for i, sf in enumerate(sfs):
        r = res[i]
        found = [(d.nCCE, d.rnti, d.dci_length, bytes(d.dci_pdu)) for d in r.dci[:r.dci_cnt]]
        assert r.dci_cnt == len(sent[i]) and PC.sent_came_back(sent[i], found), (sf, found)
        for d in r.dci[:r.dci_cnt]:
            length, L, cce, rnti, pdu = next(it for it in sent[i] if it[2] == d.nCCE)
            # the level a DCI is found at is the first of the plan's that decodes: an L = 0 DCI beside empty CCEs
            # also decodes as a wider candidate from the same first CCE, so L is pinned by the model below
            assert d.rnti == rnti
            if rnti == SI:                                 # the plan's first entry is its own: the level sent.  A UE
                assert d.L == L                            # DCI at L = 3 inside the common space decodes, from its first
                                                           # four CCEs, in the common L = 2 pass of the same size first
            assert d.format == (2 if rnti == SI or pdu[3] & 0x80 else 0)
        # and what the model finds on the same compensated symbols
        e = M.pdcch_soft_bits(comp[i][:npds[i] * 12 * N_RB], PC.model_table(fo, sf, npds[i]))
        _same(r, M.dci_search(e, O.get_nCCE(npds[i], fo, 1), O.get_nCCE(3, fo, 1), CRNTI, SI, RA, sf, plan))


def test_gpu_detected_search_equals_the_fixed_count_search(gpu):
    N_RB, Nid, first, n_sf = 25, 137, 8, 3
    fo, fg = _frames(gpu, N_RB, Nid, 1)
    size, plan = _plan(N_RB)
    rng = np.random.default_rng(31)
    comps, npd = [], None
    for i in range(n_sf):
        sf = (first + i) % 10
        items, n_common, want = PC.tx_items(fo, sf, size, rng, CRNTI, SI)
        grid = np.zeros(10 * fg.symbols_per_tti * fg.ofdm_symbol_size, dtype=np.int32)
        n = gpu.generate_dci_top(items, n_common, 512, fg, [grid], sf)
        assert n == want and npd in (None, n)
        npd = n
        comps.append(PC.grid_to_comp(grid, fo, sf, npd))
    words = npd * 12 * N_RB
    wide = np.zeros((n_sf, 36 * N_RB), dtype=np.int32)
    wide[:, :words] = np.stack(comps)
    wide[:, words:] = rng.integers(-2 ** 31, 2 ** 31 - 1, (n_sf, 36 * N_RB - words))   # beyond the count: not read
    b = gpu.PdcchRxBatch(fg, npd, CRNTI, SI, RA, plan, n_sf)
    srch = gpu.PdcchRxBatchDetected(fg, CRNTI, SI, RA, plan, n_sf)
    d_wide = _upload(gpu, wide)
    d_cfi = _upload(gpu, np.full(8, npd, dtype=np.uint8))
    try:
        b.upload(np.stack(comps))
        b.launch(first_subframe=first)
        ref = b.results()
        srch.launch(d_wide, d_cfi, first_subframe=first, subframe_step=1)
        got = srch.results()
    finally:
        b.close()
        srch.close()
        gpu.lib().oai4g_dev_free(ctypes.c_void_p(d_wide))
        gpu.lib().oai4g_dev_free(ctypes.c_void_p(d_cfi))
    assert sum(r.dci_cnt for r in ref) >= n_sf
    assert bytes(got) == bytes(ref)
