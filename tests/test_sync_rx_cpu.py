"""CPU suite of the UE's initial cell search, without a device:

  - the numpy model (tests/sync_rx_model.py) equals the reference's own lte_sync_time.c on every case of
    tests/sync_time_cases.py up to 25 PRB (tests/golden/sync_time_ref.json: replicas, peak position, source, the
    winning metric and every defined entry of the three correlation buffers), after each case's property has been
    asserted from the model itself: all-zero input gives (0, 0); of two equal bursts the earlier wins; a burst at
    n >= length - N is not counted; the full-scale frame saturates a dot product both ways, wraps the int16 sum of
    the antennas, reaches abs32 = 2^31 and depends on the int16 negation of a received real part of -32768;
  - the library's host-only replicas equal the golden ones at 6 / 25 / 50 / 100 PRB, and what is out of scope is
    refused with a message;
  - the entry points are exported and bound;
  - the device-resident batch object obeys the lifetime rule of openair4g_amd._DeviceOwner.
"""
import ctypes
import functools
import gc
import json
import os
import re

import numpy as np
import pytest

import openair4g_amd as oai
import sync_rx_model as M
import sync_time_cases as SC
from test_batch_lifetime_cpu import FakeLib, _check_closed, fake  # noqa: F401  (fake is a fixture)

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sync_time_ref.json")))
MODEL_CASES = [n for n in SC.NAMES if n != "tx100"]


@functools.lru_cache(maxsize=None)
def case(name):
    N_RB, rx = SC.case(name)
    rx.setflags(write=False)
    return N_RB, rx


@functools.lru_cache(maxsize=None)
def model(name):
    N_RB, rx = case(name)
    return [M.sync_time(list(f), N_RB) for f in rx]


def same_as_golden(name, f, peak_pos, source, peak_val, corr):
    """one frame's defined outputs against the reference's"""
    g = GOLDEN["cases"][name][f]
    assert (peak_pos, source, peak_val) == (g["peak_pos"], g["source"], g["peak_val"]), (name, f)
    assert [SC.digest(c[::4]) for c in corr] == g["corr"], (name, f)


def test_golden_is_of_these_cases():
    assert GOLDEN["seed"] == SC.SEED and sorted(GOLDEN["cases"]) == sorted(SC.NAMES)
    for name in MODEL_CASES:
        assert [r["rx"] for r in GOLDEN["cases"][name]] == [SC.digest(f) for f in case(name)[1]], name


@pytest.mark.parametrize("N_RB", [6, 25, 50, 100])
def test_replicas_model_and_library_equal_reference(N_RB):
    want = GOLDEN["replicas"][str(N_RB)] if str(N_RB) in GOLDEN["replicas"] else None
    rep = M.replicas(N_RB)
    lib = oai.lte_sync_time_replicas(oai.frame_parms(N_RB))
    assert np.array_equal(lib, rep)
    assert rep.any(axis=(1, 2)).all()
    if want is not None:                                   # 50 PRB has no case: model and library only
        assert [SC.digest(r) for r in rep] == want
    else:
        assert N_RB == 50


def test_zero_input_gives_position_0_source_0():
    m = model("zero6")[0]
    assert (m["peak_pos"], m["source"], m["peak_val"]) == (0, 0, 0) and not m["corr"].any()


def test_noise_only():
    m = model("noise6")[0]
    assert 0 < m["peak_val"] < GOLDEN["cases"]["twice6"][0]["peak_val"] // 16


@pytest.mark.parametrize("name,cells", [("tx6_0", SC.TX6[:1]), ("tx6_1", SC.TX6[1:2]), ("tx6_2", SC.TX6[2:]),
                                        ("batch6", SC.BATCH6), ("tx25", [SC.TX25])])
def test_transmitted_frames_are_found(name, cells):
    N_RB = case(name)[0]
    for m, (nid, delay) in zip(model(name), cells):
        want = SC.pss_position(N_RB, delay)
        assert m["source"] == nid % 3 and abs(m["peak_pos"] - want) < 4, (name, m["peak_pos"], want)


def test_of_two_equal_bursts_the_earlier_wins():
    m = model("twice6")[0]
    p0, p1 = SC.TWICE
    c = m["corr"][1]
    assert c[p0] == c[p1] == c.max() and c[p0] > 0
    assert (m["peak_pos"], m["source"]) == (p0, 1)


def test_a_burst_behind_the_last_counted_position_is_not_seen():
    m, full = model("late6")[0], model("twice6")[0]["peak_val"]
    length = 9600
    assert length - 128 <= SC.LATE < length - 128 + 4 * 16 and SC.LATE % 4 == 0
    assert not m["corr"][:, length - 128:length].any()       # :420, the positions contribute 0
    assert m["peak_pos"] < length - 128 and 4 * m["peak_val"] < full


def test_full_scale_frame_reaches_every_corner():
    N_RB, rx = case("full6")
    m = model("full6")[0]
    i_neg, i_pos, i_min = (SC.FULL[k] // 4 for k in ("neg", "pos", "min"))
    (re0, im0), (re1, im1) = m["parts"][(0, 0, 0)], m["parts"][(0, 0, 1)]
    assert (re0[i_neg], im0[i_neg]) == (-32768, -32768) and (re1[i_neg], im1[i_neg]) == (0, 0)
    assert m["corr"][0, SC.FULL["neg"]] == -2 ** 31                           # abs32 = 2^31 wraps negative
    assert (re0[i_pos], im0[i_pos]) == (32767, 32767) == (re1[i_pos], im1[i_pos])
    assert m["corr"][0, SC.FULL["pos"]] == 8                                  # (-2)^2 + (-2)^2: the int16 sum wrapped
    assert m["peak_val"] == 0xC0000000                                        # and wins as an unsigned number
    y = rx[0, 0].view(np.int16).reshape(-1, 2)
    assert y[SC.FULL["min"]].tolist() == [-32768, 0]
    wide = M.sync_time(list(rx[0]), N_RB, wide_neg=True)
    near = slice(SC.FULL["min"] - 124, SC.FULL["min"] + 4)
    assert not np.array_equal(wide["corr"][:, near], m["corr"][:, near])     # the int16 negation is visible


@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_equals_reference(name):
    for f, m in enumerate(model(name)):
        same_as_golden(name, f, m["peak_pos"], m["source"], m["peak_val"], m["corr"])


REF_SSS = "/root/reference/openair1/PHY/LTE_TRANSPORT/sss.c"


@pytest.mark.skipif(not os.path.exists(REF_SSS), reason="reference tree absent")
def test_phase_tables_equal_reference():
    src = open(REF_SSS).read()
    for name, want in (("phase_re", M.PHASE_RE), ("phase_im", M.PHASE_IM)):
        body = src[src.index(name + "[7]"):]
        assert tuple(int(x) for x in re.findall(r"-?\d+", body[body.index("{"):body.index("}")])) == want


@pytest.mark.parametrize("nid,nb_tx,nb_rx,delay", [(0, 1, 1, 1236), (502, 1, 2, 10400), (503, 2, 2, 333)])
def test_model_finds_the_transmitted_cell(nid, nb_tx, nb_rx, delay):
    """6 PRB, the PSS and SSS stages together: Nid1 0 and 167, every Nid2, and a delay past the half frame, where the
    subframe-5 signals come first (flip = 1) and the reported offset has the half frame added"""
    rng = np.random.default_rng([SC.SEED, nid])
    rx = SC.received(SC.tx_frame(6, nid, nb_tx), delay, nb_rx, 40.0, rng)
    cell = M.cell_search(list(rx), 6)
    assert cell[0] == nid and cell[3] == (1 if delay >= 9600 else 0) and cell[5] == 0
    assert 0 <= delay - cell[1] < 4
    assert M.fep_window(6, 0, 0, cell[1]) == (cell[1] + 10) // 4 * 4 % 19200


def test_offset_arithmetic_and_the_sss_error_condition():
    """initial_sync.c:310-354 at 6 PRB: sync_pos_slot = 960 - 128 - 9"""
    assert M.offsets(832, 6) == (0, True) and M.offsets(4, 6) == (19200 - 832 + 4, False)
    assert M.offsets(100, 6) == (19200 - 732, False)
    assert M.offsets(9596, 6) == (9596 - 832, True)
    assert M.cell_search([np.zeros(19200, np.int32)], 6) == [-1, 19200 - 832, 0, 0, 0, M.SSS_ERROR]


def test_entry_points_are_exported_and_bound():
    L = oai.load_library()
    names = ["oai4g_lte_sync_time_replicas", "oai4g_sync_config_create", "oai4g_sync_config_destroy", "oai4g_sync_time_batch",
             "oai4g_lte_sync_time", "oai4g_fep_offset_batch", "oai4g_sss_batch", "oai4g_sss_rows_batch", "oai4g_rx_sss",
             "oai4g_initial_sync"]
    assert all(hasattr(L, n) for n in names) and set(names) <= set(oai.exported_symbols())
    for n in ("lte_sync_time_replicas", "lte_sync_time", "rx_sss", "initial_sync", "sync_batch"):
        assert callable(getattr(oai, n))
    assert issubclass(oai._SyncBatch, oai._DeviceOwner)
    assert ctypes.sizeof(oai.Cell) == 24 and ctypes.sizeof(oai.InitialSync) == 16


def test_refusals_need_no_device():
    L = oai.load_library()

    def refused(fp, nb_rx, *words):
        assert not L.oai4g_sync_config_create(ctypes.byref(fp), nb_rx)
        msg = L.oai4g_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(oai.frame_parms(25, frame_type=1), 1, "TDD")
    refused(oai.frame_parms(25, Ncp=1), 1, "extended prefix")
    refused(oai.frame_parms(25), 3, "3 receive antennas")
    refused(oai.frame_parms(15), 1, "N_RB_DL 15", "256")
    fp75 = oai.frame_parms(100)                            # oai4g_init_frame_parms itself knows no 1536-point size
    fp75.N_RB_DL = 75
    refused(fp75, 1, "N_RB_DL 75")
    with pytest.raises(oai.OAI4GError, match="N_RB_DL 15"):
        oai.lte_sync_time_replicas(oai.frame_parms(15))
    assert L.oai4g_sync_time_batch(None, 1, None, None, None, None) == -1


# ---- the lifetime rule (tests/test_batch_lifetime_cpu.py) for the batch object handed out by sync_batch ----
def _make():
    return oai.sync_batch(oai.frame_parms(6), 2, 2)


def test_sync_batch_close_releases_in_order_and_once(fake):
    o = _make()
    assert type(o).__name__.startswith("_") and isinstance(o, oai._DeviceOwner)
    acquired = list(fake.live.items())
    assert [k for _, k in acquired] == ["cfg", "buf", "buf", "buf"] and o.d_corr is None
    fake.log.clear()
    o.close()
    _check_closed(fake, o, acquired)
    with _make() as o:
        acquired = list(fake.live.items())
        fake.log.clear()
    _check_closed(fake, o, acquired)


def test_sync_batch_failing_constructor_releases_what_it_acquired(fake):
    _make().close()
    n = fake.n_acq
    assert n == 4
    for k in range(1, n + 1):
        fake.n_acq, fake.fail_at = 0, k
        with pytest.raises(oai.OAI4GError):
            _make()
        gc.collect()
        assert not fake.live and fake.n_acq == k
    assert not fake.errors


def test_sync_batch_lazy_buffer_is_released(fake):
    o = _make()
    before = len(fake.live)
    o.launch()
    assert len(fake.live) == before and o.d_corr is None
    o.launch(want_corr=True)
    o.launch(want_corr=True)
    assert len(fake.live) == before + 1 and type(o.d_corr) is int
    acquired = list(fake.live.items())
    fake.log.clear()
    o.close()
    _check_closed(fake, o, acquired)
    o = _make()
    fake.fail_at = fake.n_acq + 1                          # the lazy buffer itself cannot be had: nothing else is lost
    with pytest.raises(oai.OAI4GError):
        o.launch(want_corr=True)
    assert o.d_corr is None and len(fake.live) == before
    o.close()
    assert not fake.live
