"""The PDSCH receiver's one batch path across its four configuration kinds (TM1, TM2, TM3, TM4-6), at the
smallest shape: 6 PRB (N = 128), one subframe, subframe index 1 (no PBCH / sync half RB).

Refusals: every batch entry point takes its own kind of configuration and refuses the three others and a
null one before anything is launched.  Arithmetic: each kind's batch from the estimate planes, and from the
pilot rows where the kind has that form, equals the oracle restatement on full-range random grids, for one
and two receive antennas and every modulation order (the other files pin these kinds at larger shapes and
through the drop-ins)."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import rx_tm56_model as M
from test_rx_cpu import alloc

pytestmark = pytest.mark.gpu

N_RB, SF, NPD, RNTI, MCS0, MODE, PMI = 6, 1, 2, 0x1234, 9, 7, 0x1B4E
RA = alloc(N_RB)


def _frames(gpu, two_ports):
    kw = dict(nb_antennas_tx=2, mode1_flag=0) if two_ports else {}
    return O.frame(N_RB, Nid_cell=3, **kw), gpu.frame_parms(N_RB, Nid_cell=3, **kw)


@pytest.fixture(scope="module")
def grids():
    """FEP output [n_sf + 1 = 2][2 antennas][nsymb * N], full range; shared, never written"""
    g = np.random.default_rng(61).integers(-2 ** 31 + 1, 2 ** 31 - 1, (2, 2, 14 * 128), dtype=np.int64).astype(np.int32)
    g.setflags(write=False)
    return g


def _upload(gpu, a):
    a = np.ascontiguousarray(a)
    d = gpu.lib().oai4g_dev_alloc(a.nbytes)
    assert d and gpu.lib().oai4g_memcpy_h2d(d, a.ctypes.data, a.nbytes) == 0
    return d


# ------------------------------------------------------------------------------------------ refusals
KINDS = ("siso", "tm2", "tm3", "tm56")
# entry point -> (the kind it takes, takes a second LLR buffer)
ENTRIES = {"oai4g_rx_batch": ("siso", False), "oai4g_rx_batch_estimated": ("siso", False),
           "oai4g_rx_batch_tm2": ("tm2", False),
           "oai4g_rx_batch_tm3": ("tm3", False), "oai4g_rx_batch_tm3_pilots": ("tm3", False),
           "oai4g_rx_batch_tm3_2cw": ("tm3", True), "oai4g_rx_batch_tm3_2cw_pilots": ("tm3", True),
           "oai4g_rx_batch_tm56": ("tm56", False), "oai4g_rx_batch_tm56_pilots": ("tm56", False)}


def test_gpu_rx_batch_refusal_matrix(gpu, grids):
    L = gpu.lib()
    _, f1 = _frames(gpu, False)
    _, f2 = _frames(gpu, True)
    ra = (ctypes.c_uint32 * 4)(*RA)
    cfgs = {"siso": L.oai4g_rx_config_create(ctypes.byref(f1), ra, 2, NPD, RNTI, SF, 1),
            "tm2": L.oai4g_rx_config_create_tm2(ctypes.byref(f2), ra, 2, NPD, RNTI, SF, 1, 2),
            "tm3": L.oai4g_rx_config_create_tm3(ctypes.byref(f2), ra, 2, 2, MCS0, NPD, RNTI, SF, 1, 2),   # both QPSK
            "tm56": L.oai4g_rx_config_create_tm56(ctypes.byref(f2), ra, 2, MODE, PMI, gpu.RX_PMI_UE, 1, NPD, RNTI, SF, 1, 2)}
    assert all(cfgs.values()), L.oai4g_last_error()
    # a port-0 estimation configuration of the same frame and subframes for either frame description, so that
    # oai4g_rx_batch_estimated's own comparison of the two configurations passes and the kind decides
    ces = {k: L.oai4g_chest_config_create(ctypes.byref(f1 if k == "siso" else f2), 0, SF, 1) for k in KINDS}
    assert all(ces.values())
    # buffers every entry point could run on whole: no call here is able to touch memory it does not own
    d_rx = _upload(gpu, grids)
    d_est = _upload(gpu, np.zeros((4, 2, 14 * 128), np.int32))           # planes, or 4 x 8 pilot rows
    d_llr = _upload(gpu, np.zeros((2, 14 * 72 * 6 + 64), np.int16))

    def call(name, cfg, kind):
        second = ENTRIES[name][1]
        d1 = ctypes.c_void_p(d_llr + (14 * 72 * 6 + 64) * 2)
        if name == "oai4g_rx_batch_estimated":
            return L.oai4g_rx_batch_estimated(cfg, ces[kind], 1, d_rx, d_llr, 0, None)
        args = (cfg, 1, d_rx, d_est, d_llr) + ((d1,) if second else ()) + (0, None)
        return getattr(L, name)(*args)

    try:
        for name, (takes, _) in ENTRIES.items():
            for kind in KINDS:
                rc = call(name, cfgs[kind], kind)
                if kind == takes:
                    assert rc == 0, (name, kind, L.oai4g_last_error())
                else:
                    assert rc == -1 and L.oai4g_last_error(), (name, kind)
            assert call(name, None, takes) == -1 and L.oai4g_last_error(), name
        assert L.oai4g_sync() == 0
    finally:
        L.oai4g_sync()
        for d in (d_rx, d_est, d_llr):
            L.oai4g_dev_free(ctypes.c_void_p(d))
        for k in KINDS:
            L.oai4g_rx_config_destroy(cfgs[k])
            L.oai4g_chest_config_destroy(ces[k])


# ---------------------------------------------------------------------------------------- arithmetic
@pytest.mark.parametrize("Qm", [2, 4, 6])
def test_gpu_rx_modes_siso(gpu, grids, Qm):
    """oai4g_rx_batch on a random estimate grid, and oai4g_rx_batch_estimated on its own estimates"""
    fo, fg = _frames(gpu, False)
    y, nxt = grids[0, 0], grids[1, 0, :128]
    h = grids[1, 1]
    rb = gpu.RxBatch(fg, RA, Qm, NPD, RNTI, 1, first_subframe=SF)
    a = rb.run(y[None], h[None], unscramble=0)[0]
    cb = gpu.ChestBatch(fg, 1, first_subframe=SF)
    yin = np.concatenate([y, nxt])
    assert gpu.lib().oai4g_memcpy_h2d(cb.d_rx, gpu._ptr(yin), yin.nbytes) == 0
    rb.launch_estimated(cb, cb.d_rx, 0)
    b = rb.llrs()[0]
    G = rb.llr_count(SF)
    rb.close()
    cb.close()
    lo, _ = O.rx_pdsch_siso(fo, y, h, RA, Qm, NPD, SF)
    assert len(lo) == G and np.array_equal(a[:G], lo)
    lo, _ = O.rx_pdsch_siso(fo, y, O.chest_subframe(fo, y, nxt, SF), RA, Qm, NPD, SF)
    assert np.array_equal(b[:G], lo)


def _dual_case(gpu, grids, rx, nb_rx, oracle, two_cw=False):
    """estimate -> launch (planes) and estimate_pilots -> launch_pilots (when the kind has it) of `rx` on the
    shared grids against oracle(rx list, est dict) -> tuple of LLR streams"""
    g = np.ascontiguousarray(grids[:, :nb_rx])                            # [2][nb_rx][nsymb * N]
    d = _upload(gpu, g)
    try:
        rx.estimate(d, first_subframe=SF)
        (rx.launch_2cw if two_cw else rx.launch)(d, unscramble=0)
        got = [rx.llrs()[0]] + ([rx.llrs1()[0]] if two_cw else [])
        est = rx.estimates()
        G = rx.llr_count(SF)
        if rx._pilots:
            rx.estimate_pilots(d, first_subframe=SF)
            (rx.launch_2cw_pilots if two_cw else rx.launch_pilots)(d, unscramble=0)
            pil = [rx.llrs()[0]] + ([rx.llrs1()[0]] if two_cw else [])
    finally:
        rx.close()
        gpu.lib().oai4g_dev_free(ctypes.c_void_p(d))
    want = oracle([g[0, a] for a in range(nb_rx)], {(p, a): est[2 * p + a, 0] for p in (0, 1) for a in range(nb_rx)})
    for i, lo in enumerate(want):
        assert len(lo) == G and np.array_equal(got[i][:G], lo), i
        if rx._pilots:
            assert np.array_equal(pil[i][:G], lo), i


@pytest.mark.parametrize("nb_rx", [1, 2])
@pytest.mark.parametrize("Qm", [2, 4, 6])
def test_gpu_rx_modes_tm2(gpu, grids, Qm, nb_rx):
    fo, fg = _frames(gpu, True)
    rx = gpu.RxBatchTM2(fg, RA, Qm, NPD, RNTI, 1, nb_rx=nb_rx, first_subframe=SF)
    _dual_case(gpu, grids, rx, nb_rx, lambda y, e: O.rx_pdsch_tm2(fo, y, e, RA, Qm, NPD, SF)[:1])


@pytest.mark.parametrize("nb_rx", [1, 2])
@pytest.mark.parametrize("Qm0,Qm1", [(2, 2), (2, 4), (2, 6), (4, 4), (6, 6), (4, 6)])
def test_gpu_rx_modes_tm3(gpu, grids, Qm0, Qm1, nb_rx):
    fo, fg = _frames(gpu, True)
    rx = gpu.RxBatchTM3(fg, RA, Qm0, Qm1, MCS0, NPD, RNTI, 1, nb_rx=nb_rx, first_subframe=SF)
    if Qm0 == Qm1 == 2:                                                   # both codewords
        _dual_case(gpu, grids, rx, nb_rx, lambda y, e: O.rx_pdsch_tm3_qq(fo, y, e, RA, MCS0, NPD, SF)[:2], two_cw=True)
    else:
        _dual_case(gpu, grids, rx, nb_rx, lambda y, e: O.rx_pdsch_tm3(fo, y, e, RA, Qm0, Qm1, MCS0, NPD, SF)[:1])


@pytest.mark.parametrize("nb_rx", [1, 2])
@pytest.mark.parametrize("Qm,poff", [(2, 0), (4, 1), (6, 1)])
def test_gpu_rx_modes_tm56(gpu, grids, Qm, poff, nb_rx):
    fo, fg = _frames(gpu, True)
    rx = gpu.RxBatchTM56(fg, RA, Qm, MODE, PMI, NPD, RNTI, 1, nb_rx=nb_rx, first_subframe=SF, dl_power_off=poff)
    _dual_case(gpu, grids, rx, nb_rx, lambda y, e: M.rx_pdsch_tm56(fo, y, e, RA, Qm, MODE, PMI, poff, NPD, SF)[:1])
