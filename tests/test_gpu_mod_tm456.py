"""Single-layer precoding, MIMO_mode_t 3..8 (transmission modes 4-6), on the GPU:
  - the drop-in oai4g_dlsch_modulation against the fixture the reference's own dlsch_modulation.c
    produced (tests/golden/mod_tm456_ref.json): return value and per-antenna grid digests;
  - accumulation into a non-zero grid (+=, int16 wrap per lane);
  - the fused modulator (k_modofdm, oai4g_tx_modulate) on random packed e bits against the drop-in
    chain oai4g_dlsch_modulation -> oai4g_do_OFDM_mod on the same bits (with CRS: generate_pilots
    first; with the control region and the common signals: their drop-ins too), at 6, 15, 25, 50 and
    100 PRB over subframe indices 0..9 twice, and against the stored digests of the reference's
    do_OFDM_mod at all four transform sizes;
  - the whole chain oai4g_tx_batch = oai4g_tx_encode + that modulator;
  - the no-saturation kernels (2048 points) against the saturating ones run in a fresh process with
    OAI4G_MOD_SAT, on all-corner 64-QAM bits under a constant precoder 0..3;
  - oai4g_dlsch_encoding treats the modes as coding-only."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import seg_ofdm_ref_cases as SC
from mod_ref_cases import FULL, NBITS, e_bits, grid_digests
from rm_ref_cases import digest
from test_gpu_mod_nosat import _corners, _words

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "mod_tm456_ref.json")))


def _dlsch(gpu, c, bits=None):
    dl = gpu.DlschHandle(Kmimo=1, Mdlharq=8, N_RB_DL=c["N_RB_DL"])
    h = dl.h
    h.mcs = c["mcs"][0]
    h.mimo_mode = c["mimo_mode"]
    h.pmi_alloc = c["pmi_alloc"]
    for i in range(4):
        h.rb_alloc[i] = c["rb_alloc"][i]
    h.nb_rb = sum(bin(int(w)).count("1") for w in c["rb_alloc"])
    h.Nl = 1
    h.Nlayers = 1
    h.TBS = 1024         # the drop-in derives a coding geometry it does not use for the grid
    dl.d.sqrt_rho_a, dl.d.sqrt_rho_b = c["rho"]
    e = dl.view("e", NBITS)
    if bits is None:
        e[:] = e_bits(c["seed"][0])
    else:
        e[:] = 0
        e[:bits.size] = bits
    return dl


def _dropin(gpu, c, grids=None, bits=None):
    fp = gpu.frame_parms(c["N_RB_DL"], c["Nid_cell"], c["Ncp"], c["n_ant"], c["mode1_flag"], 0)
    nsymb = 12 if c["Ncp"] else 14
    if grids is None:
        grids = [np.zeros(10 * nsymb * fp.ofdm_symbol_size, dtype=np.int32) for _ in range(c["n_ant"])]
    dl = _dlsch(gpu, c, bits)
    ret = gpu.dlsch_modulation(grids, c["amp"], c["subframe"], fp, c["num_pdcch"], dl)
    dl.close()
    return ret, grids, fp


@pytest.mark.parametrize("i", range(len(FIX["modulation"])))
def test_dlsch_modulation_equals_reference(gpu, i):
    m = FIX["modulation"][i]
    ret, grids, fp = _dropin(gpu, m["case"])
    assert ret == m["ret"]
    assert grid_digests(grids, m["case"], fp.ofdm_symbol_size) == m["digests"]


def test_dlsch_modulation_accumulates(gpu):
    c = next(m["case"] for m in FIX["modulation"] if m["case"]["N_RB_DL"] == 25 and m["case"]["mcs"] == [22])
    _, zero, fp = _dropin(gpu, c)
    rng = np.random.default_rng(0x456ACC)
    pre = [rng.integers(-2 ** 31, 2 ** 31, zero[0].size, dtype=np.int64).astype(np.int32) for _ in range(2)]
    _, got, _ = _dropin(gpu, c, [g.copy() for g in pre])
    for a in range(2):
        want = (pre[a].view(np.int16).astype(np.int32) + zero[a].view(np.int16).astype(np.int32)).astype(np.int16)
        assert np.array_equal(got[a].view(np.int16), want), a
        assert np.any(zero[a])


def test_two_codewords_are_refused(gpu):
    c = FIX["modulation"][0]["case"]
    fp = gpu.frame_parms(c["N_RB_DL"], c["Nid_cell"], c["Ncp"], 2, 0, 0)
    grids = [np.zeros(10 * 14 * fp.ofdm_symbol_size, dtype=np.int32) for _ in range(2)]
    d0, d1 = _dlsch(gpu, c), _dlsch(gpu, c)
    assert gpu.dlsch_modulation(grids, 512, c["subframe"], fp, c["num_pdcch"], d0, d1) == -1
    assert not grids[0].any() and not grids[1].any()


# ------------------------------------------------------------------------------------------------
# the fused path
# ------------------------------------------------------------------------------------------------
def _params(gpu, n_rb, mcs, mode, pmi, with_crs=0, Ncp=0, subframe=0, step=1, Nid_cell=0, num_pdcch=None, rho=None):
    p = gpu.make_params("TM6", subframe=subframe, subframe_step=step, with_crs=with_crs, Nid_cell=Nid_cell,
                        N_RB_DL=n_rb, rb_alloc=FULL[n_rb], nb_rb=n_rb, mcs=(mcs, 0), mimo_mode=mode, pmi_alloc=pmi, Ncp=Ncp,
                        num_pdcch_symbols=num_pdcch or (1 if n_rb > 10 else 3))
    if rho:
        p.sqrt_rho_a, p.sqrt_rho_b = rho
    return p


def _case_of(p, sfi):
    return dict(N_RB_DL=p.N_RB_DL, Nid_cell=p.Nid_cell, Ncp=p.Ncp, n_ant=2, mode1_flag=0, mimo_mode=p.mimo_mode,
                mcs=[p.mcs[0]], pmi_alloc=p.pmi_alloc, rb_alloc=[p.rb_alloc[i] for i in range(4)], amp=p.amp,
                rho=(p.sqrt_rho_a, p.sqrt_rho_b), subframe=sfi, num_pdcch=p.num_pdcch_symbols)


def _chain_iq(gpu, p, sfi, bits, static=None):
    """drop-in chain for one subframe: [static REs ->] dlsch_modulation -> do_OFDM_mod of both slots"""
    c = _case_of(p, sfi)
    fp = gpu.frame_parms(p.N_RB_DL, p.Nid_cell, p.Ncp, 2, 0, 0)
    nsymb, N, spt = fp.symbols_per_tti, fp.ofdm_symbol_size, fp.samples_per_tti
    grids = [np.zeros(10 * nsymb * N + N, dtype=np.int32) for _ in range(2)]
    if p.with_crs:
        gpu.generate_pilots(grids, p.amp, fp)
    if static:
        static(grids, fp, sfi)
    ret, grids, _ = _dropin(gpu, c, grids, bits)
    assert ret > 0
    outs = [np.zeros(10 * spt + 64, np.int32) for _ in range(2)]
    do_ofdm = SC.gpu_impl(gpu)["do_ofdm"]
    for slot in (2 * sfi, 2 * sfi + 1):
        outs = list(do_ofdm(grids, outs, 0, slot, fp).reshape(2, -1))
    return np.stack([o[sfi * spt:(sfi + 1) * spt] for o in outs])


def _fused(gpu, p, n_sf, seed, setup=None, words=None):
    pipe = gpu.TxPipeline(p, n_sf)
    if setup:
        setup(pipe)
    if words is None:
        words = np.random.default_rng(seed).integers(0, 1 << 32, size=(n_sf, 1, pipe.ebits_words), dtype=np.uint64)
        words = words.astype(np.uint32)
    G = [pipe.G(0, (p.first_subframe + i * p.subframe_step) % 10) for i in range(n_sf)]
    nosat = pipe.mod_nosat
    pipe.upload_ebits(words)
    pipe.modulate_only()
    pipe.sync()
    iq = pipe.iq()
    pipe.close()
    return words, G, iq, nosat


FUSED = [  # n_rb, mcs, mode, pmi, with_crs, Ncp, grid cap
    (6, 5, 3, 0x0E4B, 0, 0, 0), (6, 12, 8, 0x01B4, 1, 0, 0),
    (15, 12, 4, 0x0E4B, 0, 0, 0), (15, 22, 7, 0x01B4, 1, 0, 0), (15, 5, 6, 0x0B1E, 1, 1, 0),   # 256 points: own guard band
    (25, 12, 5, 0x1B4E, 0, 0, 0), (25, 22, 6, 0xE4B1, 1, 0, 4), (25, 5, 4, 0xE4B1, 0, 1, 0), (25, 22, 7, 0x1B4E, 1, 1, 0),
    (50, 22, 8, 0xE4B1, 0, 0, 0), (50, 5, 3, 0x1B4E, 1, 0, 0),
    (100, 5, 5, 0xE4B1, 0, 0, 0), (100, 12, 3, 0x1B4E, 1, 0, 0), (100, 22, 8, 0xE4B1, 0, 0, 4), (100, 22, 4, 0x1B4E, 1, 0, 0),
]


@pytest.mark.parametrize("n_rb,mcs,mode,pmi,crs,ncp,cap", FUSED)
def test_fused_modulator_equals_dropin_chain(gpu, n_rb, mcs, mode, pmi, crs, ncp, cap):
    p = _params(gpu, n_rb, mcs, mode, pmi, with_crs=crs, Ncp=ncp, Nid_cell=(n_rb + 7 * mcs) % 504)
    gpu.lib().oai4g_set_modofdm_grid_cap(cap)
    try:
        words, G, iq, _ = _fused(gpu, p, 20, 0x456F + n_rb + mcs)
    finally:
        gpu.lib().oai4g_set_modofdm_grid_cap(0)
    for i in range(20):
        want = _chain_iq(gpu, p, i % 10, gpu.unpack_bits(words[i, 0], G[i]))
        assert np.array_equal(iq[i], want), (n_rb, i)
        assert iq[i, 1].any()


def test_fused_modulator_with_control_and_common_signals(gpu):
    """100 PRB with CRS, PCFICH + PDCCH (set_control) and PSS / SSS / PBCH / PHICH (set_common)"""
    import bench
    from openair4g_amd import Pbch
    p = _params(gpu, 100, 22, 5, 0xE4B1, with_crs=1)
    items, phich = bench.full_grid_items(p, "C2")      # the name selects the DCI length alone (C2: format 1, 39 bits)
    pdu = bench.FULL_GRID_PBCH_PDU
    words, G, iq, _ = _fused(gpu, p, 10, 0x456FC, setup=lambda pipe: bench.full_grid_setup(pipe, p, "C2"))

    def static(grids, fp, sf):
        nsl = fp.symbols_per_tti // 2
        assert gpu.generate_dci_top(items, 0, p.amp, fp, grids, sf) >= 0
        if sf in (0, 5):
            assert gpu.generate_pss(grids, p.amp, fp, nsl - 1, 2 * sf) == 0
            assert gpu.generate_sss(grids, p.amp, fp, nsl - 2, 2 * sf) == 0
        if sf == 0:
            assert gpu.generate_pbch(Pbch(), grids, p.amp, fp, pdu, 0) == 0
        for (psf, g, q, h) in phich:
            if psf == sf:
                assert gpu.generate_phich(fp, p.amp, q, g, h, sf, grids) == 0

    for i in range(10):
        want = _chain_iq(gpu, p, i, gpu.unpack_bits(words[i, 0], G[i]), static)
        assert np.array_equal(iq[i], want), i


@pytest.mark.parametrize("m", [m for m in FIX["modulation"] if "ofdm_digests" in m],
                         ids=lambda m: "prb%d" % m["case"]["N_RB_DL"])
def test_fused_modulator_equals_reference_do_ofdm_digests(gpu, m):
    c = m["case"]
    p = _params(gpu, c["N_RB_DL"], c["mcs"][0], c["mimo_mode"], c["pmi_alloc"], subframe=c["subframe"], step=0,
                Nid_cell=c["Nid_cell"], num_pdcch=c["num_pdcch"], rho=c["rho"])
    probe = gpu.TxPipeline(p, 1, alloc=False)
    G, ew = probe.G(0, c["subframe"]), probe.ebits_words
    probe.close()
    buf = np.zeros(ew * 4, np.uint8)
    packed = np.packbits(e_bits(c["seed"][0])[:G], bitorder="little")
    buf[:packed.size] = packed
    _, _, iq, _ = _fused(gpu, p, 1, 0, words=buf.view(np.uint32).reshape(1, 1, ew))
    assert [digest(iq[0, a]) for a in range(2)] == m["ofdm_digests"]


def test_tx_batch_equals_encode_then_modulate(gpu):
    """payload -> k_encode -> the new mode's k_modofdm in one call, at 100 PRB 64-QAM"""
    p = _params(gpu, 100, 22, 7, 0xE4B1, subframe=3)
    n_sf = 4
    pipe = gpu.TxPipeline(p, n_sf)
    pay = np.random.default_rng(0x456B).integers(0, 256, size=(n_sf, 1, p.payload_stride), dtype=np.uint8)
    pipe.upload_payload(pay)
    pipe.run()
    pipe.sync()
    iq = pipe.iq()
    pipe.encode_only()
    pipe.sync()
    words = pipe.ebits()
    G = [pipe.G(0, (3 + i) % 10) for i in range(n_sf)]
    pipe.close()
    for i in range(n_sf):
        want = _chain_iq(gpu, p, (3 + i) % 10, gpu.unpack_bits(words[i, 0], G[i]))
        assert np.array_equal(iq[i], want), i


# ------------------------------------------------------------------------------------------------
# the no-saturation kernels
# ------------------------------------------------------------------------------------------------
NS_PMI = (0x0000, 0x5555, 0xAAAA, 0xFFFF)       # a constant precoder 0..3 (RBs 64.. read 0 at 100 PRB)
NS_SF = 4


def _ns_words(gpu, p):
    probe = gpu.TxPipeline(p, NS_SF, alloc=False)
    G, ew = probe.G(0, 7), probe.ebits_words
    probe.close()
    n_re = G // 6
    idx = np.arange(n_re)
    rot = _corners(6)
    rng = np.random.default_rng(0x456A5)
    pats = [np.full(n_re, rot[0]), np.where((idx >> 1) & 1, rot[2], rot[0]), rot[idx & 3], rot[rng.integers(0, 4, n_re)]]
    words = np.zeros((NS_SF, 1, ew), np.uint32)
    for i, s in enumerate(pats):
        words[i, 0], _ = _words(s, 6, G, ew)
    return words


def _ns_iq(gpu):
    out = {}
    for pmi in NS_PMI:
        p = _params(gpu, 100, 22, 5, pmi, subframe=7, step=0)
        _, _, iq, nosat = _fused(gpu, p, NS_SF, 0, words=_ns_words(gpu, p))
        out["iq%04x" % pmi] = iq
        out["ns%04x" % pmi] = np.array(nosat)
    return out


def _sat_child(path):
    """entry of the fresh process: OAI4G_MOD_SAT is in its environment from the start"""
    import openair4g_amd as gpu
    gpu.init()
    np.savez(path, **_ns_iq(gpu))


def test_range_check(gpu):
    pipe = gpu.TxPipeline(_params(gpu, 100, 22, 5, 0xE4B1), 1, alloc=False)
    assert pipe.mod_nosat                         # V = 391 < C3's 553 at amp 512
    pipe.close()
    pipe = gpu.TxPipeline(_params(gpu, 6, 22, 5, 0xE4B1), 1, alloc=False)
    assert not pipe.mod_nosat                     # 128 points: no fused levels
    pipe.close()


def test_fused_levels_equal_saturating_levels(gpu, tmp_path):
    ns = _ns_iq(gpu)
    path = str(tmp_path / "sat.npz")
    env = dict(os.environ, OAI4G_MOD_SAT="1",
               PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_mod_tm456 as T; T._sat_child(%r)" % path], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    sat = np.load(path)
    for pmi in NS_PMI:
        k = "%04x" % pmi
        assert ns["ns" + k] and not sat["ns" + k]
        assert np.array_equal(ns["iq" + k], sat["iq" + k]), k
        pk = np.abs(ns["iq" + k].view(np.int16).reshape(NS_SF, -1).astype(np.int32)).max(axis=1)
        print("pmi %s peak |sample| per pattern: %s" % (k, pk.tolist()))
        assert pk.max() > 8000, pk                # the bound is exercised
    assert not np.array_equal(ns["iq0000"][:, 1], ns["iq5555"][:, 1])


def test_dlsch_encoding_is_coding_only(gpu):
    p = gpu.make_params("C2", subframe=7, TBS=(24504, 0))
    fp = gpu.frame_parms(p.N_RB_DL, p.Nid_cell, 0, 2, 0, 0)
    pay = np.random.default_rng(5).integers(0, 256, size=24504 // 8 + 8, dtype=np.uint8)
    G = gpu.get_G(fp, p.nb_rb, [p.rb_alloc[i] for i in range(4)], 4, 1, 1, 7)
    es = []
    for mode in (0, 5):
        dl = gpu.DlschHandle(Kmimo=1, Mdlharq=8, N_RB_DL=100)
        h = dl.h
        h.TBS, h.mcs, h.rvidx, h.round, h.mimo_mode, h.Nl, h.pmi_alloc = 24504, p.mcs[0], 0, 0, mode, 1, 0xE4B1
        for i in range(4):
            h.rb_alloc[i] = p.rb_alloc[i]
        h.nb_rb = p.nb_rb
        assert gpu.dlsch_encoding(pay.copy(), fp, 1, dl, 7) == 0
        es.append(dl.view("e", G).copy())
        dl.close()
    assert es[0].any() and np.array_equal(es[0], es[1])
