"""CPU suite of the SC-FDMA layer, no device:

  - tests/pusch_model.py (numpy) equals the reference fixture tests/golden/pusch_ref.json (written by
    tests/golden/gen_pusch_ref.py from the reference's own lte_dfts.c and ulsch_modulation.c) for all 33 transforms and
    every input class, for dft_lte and for the ulsch_modulation cases;
  - oai4g_pusch_dft_plan's radix chain, scale constants and twiddles equal the model's for all 33 sizes, and 768 and
    other sizes without a dft<N> are refused;
  - the model's round trip ulsch_modulation -> allocated REs -> lte_idft recovers every transmitted bit by hard
    decision for each size and Qm at dlsim's AMP: a condition on the reference arithmetic.

lte_idft has no fixture of its own (ulsch_demodulation.c does not compile outside PHY_VARS_eNB): it is pinned through
the pinned transforms and the model's restatement of its gather, conjugation and 12-point scaling.
"""
import json
import os

import numpy as np
import pytest

import openair4g_amd as oai
import pusch_cases as PC
import pusch_model as M
from test_batch_lifetime_cpu import _check_closed, fake  # noqa: F401  (the stand-in library behind the lifetime rule)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ref():
    return json.load(open(os.path.join(HERE, "golden", "pusch_ref.json")))


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(HERE, "golden", "pusch_ref_vectors.npz"))


def test_fixture_is_of_these_cases(ref):
    assert ref["seed"] == PC.SEED
    assert sorted(int(k) for k in ref["dft"]) == sorted(PC.SIZES) and len(PC.SIZES) == 33
    assert len(ref["mod"]) == len(PC.MOD_CASES)
    assert {"full", "qpsk", "qam16", "qam64", "impulse", "max", "min", "alt"} == set(PC.CLASSES)


@pytest.mark.parametrize("N", PC.SIZES)
def test_model_transform_equals_reference(ref, vectors, N):
    x = PC.dft_input(N)
    y = M.dft(N, x, 1)
    if N in PC.VECTOR_SIZES:
        np.testing.assert_array_equal(y, vectors[f"dft{N}"])
    got = [PC.digest(r) for r in y]
    bad = [(i, PC.CLASSES[i]) for i in range(PC.ROWS) if got[i] != ref["dft"][str(N)][i]]
    assert not bad, bad
    assert PC.digest(M.dft_lte(x[:12].reshape(-1, 2), N, 12)) == ref["dft_lte"][str(N)]


def test_transforms_of_one_call_do_not_mix(ref):
    """rows 4i..4i+3 went through one reference call; the same rows alone through the model give the same"""
    x = PC.dft_input(60)
    for i in (12, 28, 32):
        assert [PC.digest(M.dft(60, x[r], 1)) for r in range(i, i + 4)] == ref["dft"]["60"][i:i + 4]


@pytest.mark.parametrize("i", range(len(PC.MOD_CASES)))
def test_model_ulsch_modulation_equals_reference(ref, vectors, i):
    c = PC.mod_case(i)
    grid = PC.grid_pattern((c["nsymb"], c["N"]))
    z = M.ulsch_modulation(grid, c["amp"], c["subframe"], c["N_RB_DL"], c["N"], c["Ncp"], c["Nid_cell"], c["rnti"],
                           c["first_rb"], c["nb_rb"], c["Qm"], c["srs_active"], c["h"])
    if f"mod{i}_grid" in vectors.files:
        np.testing.assert_array_equal(grid.reshape(-1, 2), vectors[f"mod{i}_grid"])
    assert PC.digest(z) == ref["mod"][i]["z"]
    assert PC.digest(grid.reshape(-1, 2)) == ref["mod"][i]["grid"]
    assert (c["h"][:c["G"]] >= M.PUSCH_x).sum() >= 1 and c["h"][32] == M.PUSCH_y


def test_reference_refusals_and_overrun(ref):
    """what the fixture records of the reference: its three refusals write nothing; where first_carrier_offset + 12
    first_rb == ofdm_symbol_size every word it writes lies at or past RE N of its symbol, the last symbol's past the
    subframe (the library refuses these allocations)"""
    assert ref["refused"] == {"first_rb_26": 1, "nb_rb_0": 1, "harq_pid_8": 1}
    for (N_RB_DL, first_rb, nb_rb), p in zip(PC.MOD_PAST_SYMBOL, ref["past"]):
        assert PC.fft_size(N_RB_DL) - 6 * N_RB_DL + 12 * first_rb == PC.fft_size(N_RB_DL)
        assert p["changed"] == p["past_symbol"] == 12 * 12 * nb_rb and p["in_tail"] == 12 * nb_rb


@pytest.mark.parametrize("N", PC.SIZES)
def test_plan_equals_model(N):
    plan, tw = oai.pusch_dft_plan(N)
    ch = M.chain(N)
    assert plan.size == N and plan.n_levels == len(ch) <= 4
    assert list(plan.radix[:len(ch)]) == ch
    assert plan.leaf_norm == (9459 if N == 12 else 0)
    size, scaled, off = N, True, 0
    for l, r in enumerate(ch):
        assert plan.sub_size[l] == size // r
        assert plan.norm[l] == (M.NORM[size] if scaled else 0), (N, l)
        want = M.twiddles(size).reshape(-1, 2)
        assert plan.tw_offset[l] == off
        np.testing.assert_array_equal(tw[off:off + len(want)], want)
        off += len(want)
        scaled = size not in M.SUB_UNSCALED
        size //= r
    assert size == 12 and plan.n_twiddles == off == len(tw)


def test_twiddle_entries_the_issue_names():
    """truncated toward zero up to 300 (23169, 16383, 31650, 28377, 32753 / -953), floor from 324 on (32753 / -954)"""
    _, tw24 = oai.pusch_dft_plan(24)
    assert tw24[0].tolist() == [31650, -8480] and tw24[1].tolist() == [28377, -16383] and tw24[2].tolist() == [23169, -23169]
    _, tw216 = oai.pusch_dft_plan(216)
    assert tw216[0].tolist() == [32753, -953]
    _, tw432 = oai.pusch_dft_plan(432)
    assert tw432[107].tolist() == [32753, -954]       # twb432[0]: the same angle, floored


@pytest.mark.parametrize("N", [768, 84, 132, 1188, 0, 13, 1212, 2400, -12])
def test_sizes_without_a_transform_are_refused(N):
    plan = oai.PuschPlan()
    assert oai.lib().oai4g_pusch_dft_plan(N, oai.ctypes.byref(plan), None, 0) == -1
    err = oai.lib().oai4g_last_error().decode()
    assert str(N) in err and ("no dft768" in err if N == 768 else "not one of" in err)
    with pytest.raises(ValueError):
        M.dft(N, np.zeros((max(N, 1), 2), np.int16))


def test_plan_refuses_a_short_twiddle_buffer():
    plan = oai.PuschPlan()
    tw = np.zeros((11, 2), np.int16)
    assert oai.lib().oai4g_pusch_dft_plan(24, oai.ctypes.byref(plan), oai._ptr(tw), 10) == -1
    assert oai.lib().oai4g_pusch_dft_plan(24, oai.ctypes.byref(plan), oai._ptr(tw), 11) == 0 and plan.n_twiddles == 11


def round_trip(N, Qm, amp, Ncp=0, seed=0):
    """(transmitted bits, hard decisions) of the model alone at N_RB_DL 100: ulsch_modulation, the allocated REs into
    rxdataF_comp's layout, lte_idft.  The decision scales the constellation by the pair's real gain (least squares
    against the transmitted symbols: what a receiver has as its channel magnitude)."""
    rng = np.random.default_rng([PC.SEED, 3, N, Qm])
    nb_rb, nsymb = N // 12, 12 if Ncp else 14
    syms = M.pusch_symbols(Ncp, 0)
    G = N * Qm * len(syms)
    h = rng.integers(0, 2, G).astype(np.uint8)
    grid = np.zeros((nsymb, 2048, 2), np.int16)
    M.ulsch_modulation(grid, amp, 3, 100, 2048, Ncp, 17, 0x4321 + seed, 0, nb_rb, Qm, 0, h)
    comp = np.zeros((nsymb, 1200, 2), np.int16)
    comp[:, :600], comp[:, 600:] = grid[:, 2048 - 600:], grid[:, :600]       # first_carrier_offset on: subcarrier order
    M.lte_idft(comp, 100, Ncp, N)
    y = comp[list(M.idft_symbols(Ncp)), :N].reshape(-1, 2)
    b = M.scramble(h, G, 0x4321 + seed, 3, 17)
    d = M.modulate(b, Qm, amp).astype(np.float64)
    gain = (y * d).sum() / (d * d).sum()
    return b, M.hard_bits(y, Qm, amp, gain), gain


# The reference arithmetic itself misses the condition at dlsim's AMP = 512 in two of the 99 cases, 64-QAM at Msc 648 (2
# of 46656 bits) and at Msc 1080 (5 of 77760): the levels are then (512 * 5057) >> 15 = 79 apart from the decision
# boundary, and the rounding of the two transform passes, about 6 LSB rms at these sizes, has outliers of up to 78 LSB
# (measured on the model, which is the reference bit for bit).  These two run at 1024, where all 99 cases hold; at 2048
# the unscaled twelve-point level begins to saturate and most sizes fail.
ROUND_TRIP_AMP = {(648, 6): 1024, (1080, 6): 1024}


@pytest.mark.parametrize("N", PC.SIZES)
def test_model_round_trip_recovers_every_bit(N):
    for Qm in (2, 4, 6):
        b, got, gain = round_trip(N, Qm, ROUND_TRIP_AMP.get((N, Qm), PC.AMP))
        assert gain > 0.9
        assert np.array_equal(b, got), (N, Qm, int((b != got).sum()), len(b), gain)


def test_model_round_trip_holds_everywhere_at_1024():
    for N in (12, 300, 648, 1080, 1200):
        for Qm in (2, 4, 6):
            b, got, _ = round_trip(N, Qm, 1024, Ncp=1, seed=1)
            assert np.array_equal(b, got), (N, Qm)


def _lazy_pusch(b):
    b.upload_h(np.zeros((b.n_sf, b.G), np.uint8))
    b.upload_grid(np.zeros((b.n_sf, b.nsymb, b.N, 2), np.int16))
    b.upload_d(np.zeros((b.n_sf, b.Nsymb_pusch, b.Msc, 2), np.int16))
    b.upload_comp(np.zeros((b.n_sf, b.nsymb, 12 * b.fp.N_RB_DL, 2), np.int16))
    for _ in range(2):                     # a second upload takes no second buffer
        b.upload_h(np.zeros((b.n_sf, b.G), np.uint8))
    b.launch_mod(512), b.launch_dft(), b.launch_idft()


def test_pusch_batch_lifetime(fake):
    """PuschBatch under the rule of every device-resident class: close() synchronises once, destroys the configuration,
    frees its five lazily acquired buffers newest first, leaves cfg and every d_* None; a second close() makes no call;
    a constructor or an upload whose acquisition fails leaves nothing live"""
    make = lambda: oai.PuschBatch(oai.frame_parms(6), 2, 0, 2, 4)
    assert issubclass(oai.PuschBatch, oai._DeviceOwner)
    o = make()
    assert len(fake.live) == 1 and o.d_h is None
    _lazy_pusch(o)
    acquired = list(fake.live.items())
    assert len(acquired) == 6
    fake.log.clear()
    o.close()
    _check_closed(fake, o, acquired)
    with make() as o:
        _lazy_pusch(o)
        acquired = list(fake.live.items())
        fake.log.clear()
    _check_closed(fake, o, acquired)
    for k in range(1, 7):
        fake.n_acq, fake.fail_at = 0, k
        with pytest.raises(oai.OAI4GError):
            with make() as o:
                _lazy_pusch(o)
        assert not fake.live, (k, fake.live)
    assert not fake.errors
