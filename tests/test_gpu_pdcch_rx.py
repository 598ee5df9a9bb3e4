"""GPU tests of the PDCCH receive path: oai4g_pdcch_soft_bits, oai4g_dci_decoding_procedure0 and the
batched search oai4g_pdcch_rx_batch (k_cc_decode fed through the gather table + k_pdcch_resolve).

  - loop: 25 PRB and 6 PRB, Nid_cell 137, batches of 3 subframes that contain subframe indices 7 and 0
    (mi > 0): oai4g_generate_dci_top (one common SI-RNTI DCI at L = 2 and two UE DCIs at L = 0 and
    L = 3; at 6 PRB, whose control region holds 4 CCEs at most, two UE DCIs at L = 0 and L = 1) -> the
    grid as rxdataF_comp -> oai4g_pdcch_rx_batch.  Found DCIs, CCE maps, flags, nCCE and dci_cnt equal
    the model on the same soft bits, clean and with noise; the transmitted PDUs come back at their CCEs
    with their RNTIs (clean); the batch equals the per-call drop-ins run in plan order.  The plan is the
    whole tmode-1 plan at 25 PRB and the two UE-specific passes L = 0, 1 at 6 PRB;
  - resolution rules on crafted grids: a format 0 / 1A pair of equal size told apart by the 0x80 bit, a
    second format 0 that is not counted yet marks its CCEs, an L = 0 candidate masked by an accepted
    L = 3, and stop_if_found;
  - 6 PRB under the full tmode-1 plan with the one DCI its 4 CCEs can hold beside nothing else: the common
    SI-RNTI DCI at L = 2;
  - a ninth match in one subframe: the result keeps 8 DCIs, sets `overflow`, and the ninth still marks its CCEs.
"""
import numpy as np
import pytest

import ctrl_rx_model as M
import oracle_lib as O
import pdcch_rx_cases as PC

pytestmark = pytest.mark.gpu

CRNTI, SI, RA = 0x1234, 0xFFFF, 0x0002


def _frames(gpu, N_RB, Nid=137):
    fo, fg = O.frame(N_RB, Nid), gpu.frame_parms(N_RB, Nid)
    assert fo.phich_resource == fg.phich_resource and len(O.phich_reg_mapping(fo)) > 0
    return fo, fg


def _comp_of(gpu, fg, fo, items, n_common, sf):
    grid = np.zeros(10 * fg.symbols_per_tti * fg.ofdm_symbol_size, dtype=np.int32)
    npd = gpu.generate_dci_top(items, n_common, 512, fg, [grid], sf)
    return npd, PC.grid_to_comp(grid, fo, sf, npd)


def _model(fo, comp, sf, npd, plan, crnti=CRNTI):
    e = M.pdcch_soft_bits(comp, PC.model_table(fo, sf, npd))
    return e, M.dci_search(e, O.get_nCCE(npd, fo, 1), O.get_nCCE(3, fo, 1), crnti, SI, RA, sf, plan)


def _same(res, st):
    """a batch result against the model's state: counters, flags, maps, nCCE and every found DCI"""
    assert (res.dci_cnt, res.format0_found, res.format_c_found, res.nCCE, res.overflow) == \
        (st["cnt"], st["f0"], st["fc"], st["nCCE"], st["ovf"])
    assert list(res.CCEmap) == st["maps"]
    for i in range(st["cnt"]):
        ln, L, cce, rnti, fmt, pdu = st["alloc"][i]
        d = res.dci[i]
        assert (d.dci_length, d.L, d.nCCE, d.rnti, d.format, bytes(d.dci_pdu)[:len(pdu)]) == (ln, L, cce, rnti, fmt, pdu), i


def _drop_in_search(gpu, fg, e, npd, sf, plan, crnti=CRNTI):
    """dci_decoding_procedure's loop over the per-call drop-in"""
    st = gpu.DciSearchState()
    for i, p in enumerate(plan):
        if i > 0 and (st.maps[0].value == 0xFFFF or (st.f0.value and st.fc.value)):
            break
        old = st.cnt.value
        gpu.dci_decoding_procedure0(st, e, npd, crnti, p[0], sf, fg, 1, SI, RA, p[1], p[4], p[5], p[6], p[2], p[3])
        if p[7] and st.cnt.value > old:
            break
    return st


@pytest.mark.parametrize("N_RB,first", [(25, 6), (25, 9), (6, 6), (6, 9)])
def test_gpu_pdcch_loop(gpu, N_RB, first):
    fo, fg = _frames(gpu, N_RB)
    size = 27 if N_RB > 6 else 21
    # 25 PRB: the whole tmode-1 plan.  6 PRB: its 4 CCEs are one L = 2 candidate, which would swallow both
    # DCIs in the common pass, so the plan there is the two UE-specific passes that can hold them
    plan = PC.tm1_plan(size, 13, size, 31) if N_RB > 6 else [(0, 0, size, 4, 2, 2, 0, 0), (0, 1, size, 4, 2, 2, 0, 0)]
    rng = np.random.default_rng(N_RB * 16 + first)
    sfs = [(first + i) % 10 for i in range(3)]
    assert 7 in sfs or 0 in sfs
    sent, comps, npd = [], [], None
    for sf in sfs:
        items, n_common, want = PC.tx_items(fo, sf, size, rng, CRNTI, SI)
        n, comp = _comp_of(gpu, fg, fo, items, n_common, sf)
        assert n == want and npd in (None, n)
        npd = n
        sent.append(items)
        comps.append(comp)
    noise = [np.zeros_like(c) for c in comps]
    for c in noise:
        c.view(np.int16)[:] = rng.integers(-300, 301, size=2 * len(c))
    b = gpu.PdcchRxBatch(fg, npd, CRNTI, SI, RA, plan, 3)
    for i, sf in enumerate(sfs):                                   # the configuration's candidates, in plan order
        want = [(c, k) for k, p in enumerate(plan)
                for c in M.candidates(O.get_nCCE(npd, fo, 1), O.get_nCCE(3, fo, 1), p[0], p[1], CRNTI, sf)]
        assert b.candidates(sf) == want
    for noisy in (False, True):
        batch = [(c.view(np.int16).astype(np.int32) + (n.view(np.int16) if noisy else 0)).clip(-32768, 32767)
                 .astype(np.int16).view(np.int32) for c, n in zip(comps, noise)]
        b.upload(np.stack(batch))
        b.launch(first_subframe=first)
        res = b.results()
        for i, sf in enumerate(sfs):
            e, st = _model(fo, batch[i], sf, npd, plan)
            assert np.array_equal(gpu.pdcch_soft_bits(batch[i], fg, sf, npd), e)
            _same(res[i], st)
            di = _drop_in_search(gpu, fg, e, npd, sf, plan)            # the batch equals the per-call drop-ins
            assert di.cnt.value == res[i].dci_cnt and [m.value for m in di.maps] == list(res[i].CCEmap)
            assert di.found() == [(d.dci_length, d.L, d.nCCE, d.rnti, d.format, bytes(d.dci_pdu))
                                  for d in res[i].dci[:res[i].dci_cnt]]
            if not noisy:
                found = [(d.nCCE, d.rnti, d.dci_length, bytes(d.dci_pdu)) for d in res[i].dci[:res[i].dci_cnt]]
                assert res[i].dci_cnt == len(sent[i]) and PC.sent_came_back(sent[i], found), (sf, found)
    b.close()


def _run(gpu, fg, fo, items, sf, plan, crnti=CRNTI):
    npd, comp = _comp_of(gpu, fg, fo, items, 0, sf)
    b = gpu.PdcchRxBatch(fg, npd, crnti, SI, RA, plan, 1)
    b.upload(comp)
    b.launch(first_subframe=sf)
    res = b.results()[0]
    b.close()
    _same(res, _model(fo, comp, sf, npd, plan, crnti)[1])
    return res, npd


def _pdu(rng, top):
    p = bytearray(rng.integers(0, 256, 8, dtype=np.uint8).tobytes())
    p[3] = (p[3] & 0x7F) | (0x80 if top else 0)
    return bytes(p)


def test_gpu_format0_1a_pair_and_uncounted_second_format0(gpu):
    fo, fg = _frames(gpu, 25)
    rng = np.random.default_rng(1)
    sf, size = 3, 27
    plan = [(0, 1, size, 4, 2, 2, 0, 0)]                              # one UE-specific call at L = 1, format 0 size
    nCCE = O.get_nCCE(2, fo, 1)
    c = M.candidates(nCCE, O.get_nCCE(3, fo, 1), 0, 1, CRNTI, sf)
    pad = (size, 3, 0, 0x4444, _pdu(rng, 0))                          # someone else's DCI keeps 2 control symbols
    free = [x for x in c if x >= 8][:2]
    assert len(free) == 2
    # a format 0 and a format 1A of equal size: both counted, told apart by the leading payload bit
    res, npd = _run(gpu, fg, fo, [pad, (size, 1, free[0], CRNTI, _pdu(rng, 0)), (size, 1, free[1], CRNTI, _pdu(rng, 1))], sf, plan)
    assert npd == 2 and res.dci_cnt == 2 and sorted(d.format for d in res.dci[:2]) == [0, 2] and res.format0_found == 1
    # two format 0s: the second is not counted, yet its CCEs are marked
    res, _ = _run(gpu, fg, fo, [pad, (size, 1, free[0], CRNTI, _pdu(rng, 0)), (size, 1, free[1], CRNTI, _pdu(rng, 0))], sf, plan)
    assert res.dci_cnt == 1 and res.dci[0].format == 0
    for x in free:
        assert (res.CCEmap[x >> 5] >> (x & 31)) & 3 == 3


def test_gpu_l0_candidate_masked_by_accepted_l3(gpu):
    fo, fg = _frames(gpu, 25)
    rng = np.random.default_rng(2)
    size, npd = 27, 3
    nCCE, nmax = O.get_nCCE(npd, fo, 1), O.get_nCCE(3, fo, 1)
    # a C-RNTI and subframe whose first L = 3 candidate is also an L = 0 candidate: the DCI's first CCE alone decodes
    crnti, sf, c3 = next((r, s, M.candidates(nCCE, nmax, 0, 3, r, s)[0]) for r in range(0x100, 0x400) for s in range(10)
                         if M.candidates(nCCE, nmax, 0, 3, r, s)[0] in M.candidates(nCCE, nmax, 0, 0, r, s))
    other = 8 if c3 == 0 else 0
    items = [(size, 3, c3, crnti, _pdu(rng, 1)), (size, 3, other, 0x4444, _pdu(rng, 0))]   # 16 CCEs: 3 control symbols
    e3, e0 = (0, 3, size, 4, 2, 2, 0, 0), (0, 0, size, 4, 2, 2, 0, 0)
    res, n = _run(gpu, fg, fo, items, sf, [e3, e0], crnti)
    assert n == npd and res.dci_cnt == 1 and (res.dci[0].L, res.dci[0].nCCE) == (3, c3)
    res, _ = _run(gpu, fg, fo, items, sf, [e0], crnti)                # without the L = 3 pass the L = 0 candidate matches
    assert res.dci_cnt == 1 and (res.dci[0].L, res.dci[0].nCCE) == (0, c3)


def test_gpu_stop_if_found(gpu):
    fo, fg = _frames(gpu, 25)
    rng = np.random.default_rng(3)
    sf, s1, s0 = 4, 31, 27
    nCCE, nmax = O.get_nCCE(2, fo, 1), O.get_nCCE(3, fo, 1)
    c0 = [x for x in M.candidates(nCCE, nmax, 0, 0, CRNTI, sf) if x >= 8]
    c1 = [x for x in M.candidates(nCCE, nmax, 0, 1, CRNTI, sf) if x >= 8 and x != (c0[0] & ~1)]
    items = [(s0, 3, 0, 0x4444, _pdu(rng, 0)), (s1, 0, c0[0], CRNTI, _pdu(rng, 0)), (s0, 1, c1[0], CRNTI, _pdu(rng, 1))]
    for stop, cnt in ((1, 1), (0, 2)):
        plan = [(0, 0, s1, 4, 2, 2, 1, stop), (0, 1, s0, 4, 2, 2, 0, 0)]
        res, npd = _run(gpu, fg, fo, items, sf, plan)
        assert npd == 2 and res.dci_cnt == cnt and res.dci[0].format == 1 and res.dci[0].nCCE == c0[0]
        if cnt == 2:
            assert (res.dci[1].format, res.dci[1].nCCE, res.dci[1].L) == (2, c1[0], 1)


def test_gpu_6prb_common_dci_under_the_full_plan(gpu):
    fo, fg = _frames(gpu, 6)
    rng = np.random.default_rng(6)
    size = 21
    plan = PC.tm1_plan(size, 13, size, 19)
    for sf in (0, 7):
        items = [(size, 2, 0, SI, _pdu(rng, 1))]
        npd, comp = _comp_of(gpu, fg, fo, items, 1, sf)
        assert npd == 3 and O.get_nCCE(npd, fo, 1) == 4
        b = gpu.PdcchRxBatch(fg, npd, CRNTI, SI, RA, plan, 1)
        b.upload(comp)
        b.launch(first_subframe=sf)
        res = b.results()[0]
        b.close()
        _same(res, _model(fo, comp, sf, npd, plan)[1])
        d = res.dci[0]
        assert res.dci_cnt == 1 and (d.L, d.nCCE, d.rnti, d.format) == (2, 0, SI, 2) and res.CCEmap[0] == 0xF
        assert PC.sent_came_back(items, [(d.nCCE, d.rnti, d.dci_length, bytes(d.dci_pdu))])


def test_gpu_ninth_match_sets_overflow(gpu):
    fo, fg = _frames(gpu, 100)
    rng = np.random.default_rng(9)
    size, npd = 31, 1
    nCCE, nmax = O.get_nCCE(npd, fo, 1), O.get_nCCE(3, fo, 1)

    def disjoint(r, s):
        c0 = M.candidates(nCCE, nmax, 0, 0, r, s)
        return c0, [c for c in M.candidates(nCCE, nmax, 0, 1, r, s) if not {c, c + 1} & set(c0)]
    crnti, sf = next((r, s) for r in range(0x100, 0x200) for s in range(10)
                     if len(disjoint(r, s)[0]) == 6 and len(disjoint(r, s)[1]) >= 3)
    c0, c1 = disjoint(crnti, sf)
    items = [(size, 0, c, crnti, _pdu(rng, 1)) for c in c0] + [(size, 1, c, crnti, _pdu(rng, 1)) for c in c1[:3]]
    plan = [(0, 0, size, 4, 2, 2, 0, 0), (0, 1, size, 4, 2, 2, 0, 0)]        # format 1As: every match is counted
    res, n = _run(gpu, fg, fo, items, sf, plan, crnti)
    assert n == npd and res.dci_cnt == 8 and res.overflow == 1
    assert [d.nCCE for d in res.dci[:8]] == c0 + c1[:2]
    assert (res.CCEmap[c1[2] >> 5] >> (c1[2] & 31)) & 3 == 3                 # the dropped ninth still marks its CCEs
    res, _ = _run(gpu, fg, fo, items[:8], sf, plan, crnti)
    assert res.dci_cnt == 8 and res.overflow == 0
