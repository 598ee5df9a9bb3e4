"""The lifetime rule of the device-resident classes on the device: every class once in a `with` block at the
smallest size its own test uses (6 PRB, two subframes, eight code blocks of the smallest K, one transport block),
one launch and one result fetch inside; afterwards the library reports no error and the configuration and device
pointers are None.  The failing constructors and the second close() are tests/test_batch_lifetime_cpu.py's."""
import numpy as np
import pytest

from openair4g_amd.dlsim import DlsimBler

pytestmark = pytest.mark.gpu

N_RB, N_SF, SF, NPD, RNTI, SI, RA_RNTI = 6, 2, 1, 2, 0x1234, 0xFFFF, 0x0002
RA = [0x3F, 0, 0, 0]
PLAN = [(0, 0, 21, 4, 2, 2, 0, 0), (0, 1, 21, 4, 2, 2, 0, 0)]
GRID = 14 * 128


@pytest.fixture
def after(gpu):
    """after(*objs): the library's error text is what it was when the test began (it is empty in a fresh process and
    is never cleared, so a refusal test that ran earlier in the same process leaves its text behind: no new one may
    have been set), and every configuration and device pointer of the closed objects is None"""
    before = gpu.lib().oai4g_last_error()

    def check(*objs):
        assert gpu.lib().oai4g_last_error() == before
        for o in objs:
            attrs = {k: v for k, v in vars(o).items() if k in ("cfg", "ptr") or k.startswith("d_")}
            assert attrs and all(v is None for v in attrs.values()), (type(o).__name__, attrs)
    return check


@pytest.fixture(scope="module")
def fps(gpu):
    return gpu.frame_parms(N_RB, Nid_cell=2), gpu.frame_parms(N_RB, Nid_cell=2, nb_antennas_tx=2, mode1_flag=0)


@pytest.fixture(scope="module")
def iq():
    """received samples [n_sf + 1][2 antennas][samples_per_tti] as int16 pairs; shared, never written"""
    a = np.random.default_rng(90).integers(-2000, 2000, ((N_SF + 1) * 2 * 1920 * 2), dtype=np.int16).view(np.int32)
    a.setflags(write=False)
    return a


def test_fep_chest_rx(gpu, after, fps, iq):
    f1, _ = fps
    with gpu.FepBatch(f1, N_SF + 1, 1) as fep, gpu.ChestBatch(f1, N_SF, first_subframe=SF) as cb, \
            gpu.RxBatch(f1, RA, 2, NPD, RNTI, N_SF, first_subframe=SF) as rx:
        fep.upload(iq[:fep.n_in])
        fep.run()
        assert fep.result().shape == (N_SF + 1, 1, 14, 128)
        cb.launch(fep.d_rxF)
        rx.launch(fep.d_rxF, cb.d_est, 1)
        assert rx.llrs().shape == (N_SF, rx.stride)
        rx.launch_estimated(cb, fep.d_rxF, 1)
        est = cb.run(None, None, d_rxdataF=fep.d_rxF)
        assert est.shape == (N_SF, GRID) and cb.time_estimates().shape == (N_SF, 128)
        assert rx.run(np.zeros((N_SF, GRID), np.int32), est).shape == (N_SF, rx.stride)
    after(fep, cb, rx)


@pytest.mark.parametrize("kind", ["tm2", "tm3", "tm56"])
def test_two_port_receivers(gpu, after, fps, iq, kind):
    _, f2 = fps
    make = {"tm2": lambda: gpu.RxBatchTM2(f2, RA, 2, NPD, RNTI, N_SF, nb_rx=2, first_subframe=SF),
            "tm3": lambda: gpu.RxBatchTM3(f2, RA, 2, 2, 9, NPD, RNTI, N_SF, nb_rx=2, first_subframe=SF),
            "tm56": lambda: gpu.RxBatchTM56(f2, RA, 2, 7, 0x1B4E, NPD, RNTI, N_SF, nb_rx=2, first_subframe=SF)}[kind]
    with gpu.FepBatch(f2, N_SF + 1, 2) as fep, make() as rx:
        fep.upload(iq)
        fep.run()
        rx.estimate(fep.d_rxF, first_subframe=SF)
        rx.estimate(fep.d_rxF, first_subframe=SF)
        rx.launch(fep.d_rxF)
        assert rx.llrs().shape == (N_SF, rx.stride) and rx.estimates().shape == (4, N_SF, GRID)
        if kind == "tm3":                                   # the lazily allocated pilot rows and second stream
            rx.estimate_pilots(fep.d_rxF, first_subframe=SF)
            rx.launch_2cw_pilots(fep.d_rxF)
            assert rx.llrs1().shape == (N_SF, rx.stride) and rx.d_pil and rx.d_llr1
    after(fep, rx)


def test_control_front_ends(gpu, after, fps, iq):
    _, f2 = fps
    with gpu.FepBatch(f2, N_SF + 1, 2) as fep, \
            gpu.PdcchFrontBatch(f2, N_SF, 2, gpu.ALAMOUTI, 1, first_subframe=SF, subframe_step=1) as fb, \
            gpu.PdcchRxBatchDetected(f2, RNTI, SI, RA_RNTI, PLAN, N_SF) as srch, \
            gpu.PhichRxBatch(f2, [(0, 0, 0), (1, 0, 1)], first_subframe=SF, subframe_step=1) as ph, \
            gpu.PbchFrontBatch(f2, N_SF, 2, 2) as pb:
        fep.upload(iq)
        fep.run()
        fb.estimate(fep.d_rxF)
        fb.launch(fep.d_rxF)
        comp, cfi, _ = fb.results()
        assert comp.shape == (N_SF, 36 * N_RB) and set(cfi.tolist()) <= {1, 2, 3}
        srch.launch(fb.d_comp, fb.d_cfi, first_subframe=SF, subframe_step=1)
        assert len(srch.results()) == N_SF
        ph.launch(fb.d_comp, N_SF)
        assert len(ph.results()) == 2
        pb.estimate(fep.d_rxF)
        pb.launch(fep.d_rxF)
        pb.detect()
        assert pb.results()[0].shape == (N_SF, 2, 480) and len(pb.detected()) == N_SF
        assert sorted(pb.estimates()) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    after(fep, fb, srch, ph, pb, *srch.by_count)


def test_control_decoders(gpu, after, fps):
    f1, _ = fps
    with gpu.PdcchRxBatch(f1, NPD, RNTI, SI, RA_RNTI, PLAN, N_SF) as b, gpu.PbchDecodeBatch(f1, N_SF) as pd:
        b.upload(np.zeros((N_SF, NPD * 12 * N_RB), np.int32))
        b.launch(first_subframe=SF)
        assert len(b.results()) == N_SF
        pd.upload(np.zeros((N_SF, 1920), np.int8), [0, 1])
        pd.launch()
        cnt, mib = pd.results()
        assert cnt.shape == (N_SF,) and mib.shape == (N_SF, 3)
    after(b, pd)


@pytest.mark.parametrize("cls,K", [("TurboDecoderBatch", 40), ("TurboDecoder8Batch", 512)])
def test_turbo_decoders(gpu, after, cls, K):
    with getattr(gpu, cls)(K, 8) as dec:
        dec.upload(np.zeros((8, 3 * K + 12), np.int16))
        dec.run(max_iterations=1 if K == 40 else 2)
        it, out = dec.results()
        assert it.shape == (8,) and out.shape == (8, K // 8)
        if K == 40:                                         # no hard decision at one iteration: the zero fill
            assert not out.any()
    after(dec)


def test_ul_decode(gpu, after):
    with gpu.UlDecodeBatch(16 + 24, 288, 2, 1, max_iterations=2) as ub:
        ub.upload(np.zeros((1, 288), np.int16))
        ub.launch()
        it, c = ub.results()
        assert it.shape == (1, ub.C)
        ub.launch_harq_tb([0], [1])
        assert not ub.soft_buffers().any() and ub.d_w and ub.d_rc
    after(ub)


def test_transmit(gpu, after):
    p = gpu.make_params("C1", subframe=7)
    fp = gpu.frame_parms(p.N_RB_DL, p.Nid_cell, 0, p.nb_antennas_tx, p.mode1_flag, 0)
    with gpu.TxPipeline(p, N_SF) as tx, gpu.DlschHandle(Kmimo=p.Kmimo, Mdlharq=8, N_RB_DL=p.N_RB_DL) as dl:
        tx.fill_payload(3)
        tx.run()
        assert tx.iq().shape == (N_SF, 1, tx.spt)
        tx.enable_tb_rv()
        tx.run_rv([[1], [2]])
        tx.sync()
        h = dl.h
        h.TBS, h.mcs, h.rvidx, h.round, h.mimo_mode, h.Nl = p.TBS[0], p.mcs[0], 0, 0, p.mimo_mode, 1
        for i in range(4):
            h.rb_alloc[i] = p.rb_alloc[i]
        h.nb_rb = p.nb_rb
        dl.d.rnti = p.rnti
        pay = np.arange(p.TBS[0] // 8 + 8, dtype=np.uint8)
        assert gpu.dlsch_encoding(pay, fp, p.num_pdcch_symbols, dl, 7) == 0
        assert dl.view("e", tx.G(0, 7)).max() <= 1
    after(tx, dl)


@pytest.mark.parametrize("num_rounds", [1, 2])
def test_dlsim(gpu, after, num_rounds):
    with DlsimBler(9, batch=6, num_rounds=num_rounds) as sim:
        if num_rounds == 1:
            assert sim.run_batch(30.0, 5).shape == (6,)
        else:
            assert sum(sim.run_steps(30.0, 1)["round_trials"]) == 6   # one round of every slot
    after(sim, sim.tx, sim.fep, sim.ce, sim.rx, sim.dec)
