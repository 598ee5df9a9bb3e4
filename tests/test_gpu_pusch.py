"""GPU tests of the SC-FDMA layer (oai4g_pusch.hip) against the reference's own lte_dfts.c and ulsch_modulation.c
(tests/golden/pusch_ref.json) and the numpy model (tests/pusch_model.py, which tests/test_pusch_cpu.py pins to the
same fixture), on the cases of tests/pusch_cases.py.  Everything is bit-exact; there is no tolerance anywhere.

  - all 33 sizes through oai4g_pusch_dft_batch: every input class, 3 subframes x 12 symbols, run twice on one
    configuration (stale LDS or plan state would show), and 3 x 11 symbols (srs_active), an odd count, so that the
    last workgroup is partial at every number of symbols per workgroup;
  - oai4g_pusch_mod_batch on every case of pusch_cases.MOD_CASES (nb_rb 1, 2, 3, 5, 25, 27, 50, 100, Qm 2 / 4 / 6,
    srs on and off, both prefixes, first_rb 0 / across the wrap at ofdm_symbol_size / the largest accepted, N_RB_DL 6,
    25, 100, h with PUSCH_x / PUSCH_y runs, one at a Gold word boundary): subframe 0 of the batch against the
    fixture, all three against the model, on a grid pre-filled with a pattern that every RE the reference does not
    write must keep;
  - oai4g_pusch_idft_batch on pre-filled grids with imaginary parts of -32768 among the inputs: the pilot symbols
    and the subcarriers >= Msc keep their pattern;
  - the device round trip equals the model's;
  - the drop-ins equal the batch results, and the refusals write nothing and set oai4g_last_error.
"""
import json
import os

import numpy as np
import pytest

import pusch_cases as PC
import pusch_model as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ref():
    return json.load(open(os.path.join(HERE, "golden", "pusch_ref.json")))


def _err(gpu):
    return gpu.lib().oai4g_last_error().decode()


@pytest.mark.parametrize("N", PC.SIZES)
def test_gpu_dft_batch_all_sizes(gpu, ref, N):
    x = PC.dft_input(N)
    fp = gpu.frame_parms(100)
    with gpu.PuschBatch(fp, PC.N_SF, 0, N // 12, 2) as b:
        assert b.Nsymb_pusch == PC.N_SYM
        for run in range(2):
            b.upload_d(x)
            b.launch_dft()
            z = b.z().reshape(PC.ROWS, N, 2)
            bad = [(run, i, PC.CLASSES[i]) for i in range(PC.ROWS) if PC.digest(z[i]) != ref["dft"][str(N)][i]] if N != 12 else []
            assert not bad, bad
            if N == 12:                  # the fixture holds dft12 alone; dft_lte puts 9459 behind it
                np.testing.assert_array_equal(z, M.dft_lte_sym(12, x))
                assert PC.digest(z[:12].reshape(-1, 2)) == ref["dft_lte"]["12"]
    with gpu.PuschBatch(fp, PC.N_SF, 0, N // 12, 2, srs_active=1) as b:
        b.upload_d(x[:33])
        b.launch_dft()
        np.testing.assert_array_equal(b.z().reshape(33, N, 2), M.dft_lte_sym(N, x[:33]))


def _h_rows(c, n_sf):
    rng = np.random.default_rng([PC.SEED, 4, c["G"]])
    h = rng.integers(0, 2, (n_sf, c["G"])).astype(np.uint8)
    h[0] = c["h"][:c["G"]]
    h[1:, 5], h[1:, 6:8] = M.PUSCH_y, M.PUSCH_x
    return h


@pytest.mark.parametrize("i", range(len(PC.MOD_CASES)))
def test_gpu_mod_batch(gpu, ref, i):
    c = PC.mod_case(i)
    n_sf = 3
    fp = gpu.frame_parms(c["N_RB_DL"], c["Nid_cell"], c["Ncp"])
    assert fp.symbols_per_tti == c["nsymb"] and fp.ofdm_symbol_size == c["N"]
    h = _h_rows(c, n_sf)
    pat = np.stack([PC.grid_pattern((c["nsymb"], c["N"]), salt=s) for s in (0, 7, 9)])
    want = pat.copy()
    for s in range(n_sf):
        M.ulsch_modulation(want[s], c["amp"], (c["subframe"] + s) % 10, c["N_RB_DL"], c["N"], c["Ncp"], c["Nid_cell"], c["rnti"],
                           c["first_rb"], c["nb_rb"], c["Qm"], c["srs_active"], h[s])
    with gpu.PuschBatch(fp, n_sf, c["first_rb"], c["nb_rb"], c["Qm"], c["srs_active"], c["rnti"], c["subframe"], 1) as b:
        assert b.G == c["G"]
        b.upload_h(h)
        b.upload_grid(pat)
        b.launch_mod(c["amp"])
        got = b.grid()
    assert PC.digest(got[0].reshape(-1, 2)) == ref["mod"][i]["grid"]
    np.testing.assert_array_equal(got, want)
    untouched = (want == pat).all(-1)
    assert untouched.any() and (got[untouched] == pat[untouched]).all()


IDFT_CASES = [(6, 0, 1), (6, 1, 5), (25, 0, 3), (25, 1, 25), (100, 0, 27), (100, 1, 100), (100, 0, 50)]


def _comp(N_RB_DL, nsymb, n_sf, seed):
    rng = np.random.default_rng([PC.SEED, 5, seed])
    comp = rng.integers(-32768, 32768, (n_sf, nsymb, 12 * N_RB_DL, 2)).astype(np.int16)
    comp[:, :, ::5, 1] = -32768           # an imaginary part of -32768 stays -32768 through _mm_sign_epi16
    comp[0, 0, :12] = (-32768, -32768)
    return comp


@pytest.mark.parametrize("N_RB_DL,Ncp,nb_rb", IDFT_CASES)
def test_gpu_idft_batch(gpu, N_RB_DL, Ncp, nb_rb):
    fp = gpu.frame_parms(N_RB_DL, 0, Ncp)
    n_sf, Msc = 3, 12 * nb_rb
    comp = _comp(N_RB_DL, fp.symbols_per_tti, n_sf, nb_rb)
    want = comp.copy()
    for s in range(n_sf):
        M.lte_idft(want[s], N_RB_DL, Ncp, Msc)
    with gpu.PuschBatch(fp, n_sf, 0, nb_rb, 4, srs_active=1) as b:        # lte_idft covers the last symbol whatever srs_active is
        b.upload_comp(comp)
        b.launch_idft()
        got = b.comp()
    np.testing.assert_array_equal(got, want)
    pilots = [2, 8] if Ncp else [3, 10]
    np.testing.assert_array_equal(got[:, pilots], comp[:, pilots])
    np.testing.assert_array_equal(got[:, :, Msc:], comp[:, :, Msc:])
    assert (got[:, -1, :Msc] != comp[:, -1, :Msc]).any()
    # the drop-in on one subframe
    one = comp[1].copy()
    gpu.lte_idft(fp, one, Msc)
    np.testing.assert_array_equal(one, want[1])


@pytest.mark.parametrize("N_RB_DL,Ncp,first_rb,nb_rb,Qm", [(25, 0, 11, 3, 6), (100, 1, 25, 27, 4), (6, 0, 0, 5, 2)])
def test_gpu_round_trip_equals_model(gpu, N_RB_DL, Ncp, first_rb, nb_rb, Qm):
    fp = gpu.frame_parms(N_RB_DL, 5, Ncp)
    N, nsymb, Msc, n_sf = fp.ofdm_symbol_size, fp.symbols_per_tti, 12 * nb_rb, 2
    rng = np.random.default_rng([PC.SEED, 6, Msc])
    with gpu.PuschBatch(fp, n_sf, first_rb, nb_rb, Qm, 0, 0x2222, 4, 3) as b:
        h = rng.integers(0, 2, (n_sf, b.G)).astype(np.uint8)
        b.upload_h(h)
        b.upload_grid(np.zeros((n_sf, nsymb, N, 2), np.int16))
        b.launch_mod(PC.AMP)
        grid = b.grid()
        want_grid = np.zeros_like(grid)
        for s in range(n_sf):
            M.ulsch_modulation(want_grid[s], PC.AMP, (4 + 3 * s) % 10, N_RB_DL, N, Ncp, 5, 0x2222, first_rb, nb_rb, Qm, 0, h[s])
        np.testing.assert_array_equal(grid, want_grid)
        re = (N - 6 * N_RB_DL + 12 * first_rb + np.arange(Msc)) % N
        comp = np.zeros((n_sf, nsymb, 12 * N_RB_DL, 2), np.int16)
        comp[:, :, :Msc] = grid[:, :, re]
        want = comp.copy()
        b.upload_comp(comp)
        b.launch_idft()
        got = b.comp()
    for s in range(n_sf):
        M.lte_idft(want[s], N_RB_DL, Ncp, Msc)
    np.testing.assert_array_equal(got, want)
    for s in range(n_sf):                   # and the bits come back
        y = got[s][list(M.idft_symbols(Ncp)), :Msc].reshape(-1, 2)
        bits = M.scramble(h[s], b.G, 0x2222, (4 + 3 * s) % 10, 5)
        d = M.modulate(bits, Qm, PC.AMP).astype(np.float64)
        assert np.array_equal(M.hard_bits(y, Qm, PC.AMP, (y * d).sum() / (d * d).sum()), bits)


@pytest.mark.parametrize("N", [12, 60, 96, 324, 1200])
def test_gpu_transform_drop_ins(gpu, ref, N):
    x = PC.dft_input(N)
    z = np.full((12 * N + 7, 2), 77, np.int16)
    assert gpu.dft_lte(x[:12], N, 11, z=z) is z
    np.testing.assert_array_equal(z[:11 * N], M.dft_lte(x[:12].reshape(-1, 2), N, 11))
    assert (z[11 * N:] == 77).all()       # z beyond Nsymb columns is untouched
    assert PC.digest(gpu.dft_lte(x[:12], N, 12)) == ref["dft_lte"][str(N)]
    for row in (0, 13, 32, 33):
        assert PC.digest(gpu.pusch_dft(N, x[row], 1)) == ref["dft"][str(N)][row]
        np.testing.assert_array_equal(gpu.pusch_dft(N, x[row], 0), M.dft(N, x[row], 0))


def _frame(fp, salt=3):
    return PC.grid_pattern((10 * fp.symbols_per_tti, fp.ofdm_symbol_size), salt=salt)


@pytest.mark.parametrize("i", [2, 9, 18, 19])
def test_gpu_ulsch_modulation_drop_in(gpu, ref, i):
    c = PC.mod_case(i)
    fp = gpu.frame_parms(c["N_RB_DL"], c["Nid_cell"], c["Ncp"])
    frame = _frame(fp)
    want = frame.copy()
    sf, nsymb = c["subframe"], c["nsymb"]
    M.ulsch_modulation(want[sf * nsymb:(sf + 1) * nsymb], c["amp"], sf, c["N_RB_DL"], c["N"], c["Ncp"], c["Nid_cell"], c["rnti"],
                       c["first_rb"], c["nb_rb"], c["Qm"], c["srs_active"], c["h"])
    mcs = {2: 5, 4: 15, 6: 25}[c["Qm"]]
    assert gpu.ulsch_modulation(frame, c["amp"], sf, fp, c["first_rb"], c["nb_rb"], mcs, c["h"], c["rnti"], c["srs_active"], harq_pid=7) == 0
    np.testing.assert_array_equal(frame, want)
    sub = PC.grid_pattern((nsymb, c["N"]))
    sub_frame = _frame(fp)
    sub_frame[sf * nsymb:(sf + 1) * nsymb] = sub
    gpu.ulsch_modulation(sub_frame, c["amp"], sf, fp, c["first_rb"], c["nb_rb"], mcs, c["h"], c["rnti"], c["srs_active"])
    assert PC.digest(sub_frame[sf * nsymb:(sf + 1) * nsymb].reshape(-1, 2)) == ref["mod"][i]["grid"]


def test_gpu_refusals_write_nothing(gpu):
    c = PC.mod_case(8)
    fp = gpu.frame_parms(25, c["Nid_cell"], 0)
    frame = _frame(fp)
    keep = frame.copy()
    for kw, word in ((dict(first_rb=26), "first_rb 26"), (dict(nb_rb=0), "nb_rb 0"), (dict(harq_pid=8), "harq_pid 8")):
        a = dict(first_rb=c["first_rb"], nb_rb=c["nb_rb"], harq_pid=0)
        a.update(kw)
        assert gpu.ulsch_modulation(frame, c["amp"], 2, fp, a["first_rb"], a["nb_rb"], 25, c["h"], c["rnti"], harq_pid=a["harq_pid"]) == 1
        assert "Illegal " + word in _err(gpu)
        np.testing.assert_array_equal(frame, keep)
    with pytest.raises(gpu.OAI4GError, match="cooperation_flag 2"):
        gpu.ulsch_modulation(frame, c["amp"], 2, fp, c["first_rb"], c["nb_rb"], 25, c["h"], c["rnti"], cooperation_flag=2)
    with pytest.raises(gpu.OAI4GError, match="Nsymb_pusch"):
        gpu.ulsch_modulation(frame, c["amp"], 2, fp, c["first_rb"], c["nb_rb"], 25, c["h"], c["rnti"], Nsymb_pusch=9)
    fp100 = gpu.frame_parms(100)
    frame100 = _frame(fp100)
    keep100 = frame100.copy()
    with pytest.raises(gpu.OAI4GError, match="no dft768"):
        gpu.ulsch_modulation(frame100, c["amp"], 2, fp100, 0, 64, 5, np.zeros(64 * 12 * 2 * 12, np.uint8), 1)
    np.testing.assert_array_equal(frame, keep)
    np.testing.assert_array_equal(frame100, keep100)
    z = np.full((12 * 768, 2), 5, np.int16)
    with pytest.raises(gpu.OAI4GError, match="no dft768"):
        gpu.dft_lte(z.copy(), 768, 12, z=z)
    with pytest.raises(gpu.OAI4GError, match="not one of"):
        gpu.pusch_dft(84, np.zeros((84, 2), np.int16))
    comp = np.full((14, 1200, 2), 5, np.int16)
    with pytest.raises(gpu.OAI4GError, match="no dft768"):
        gpu.lte_idft(fp100, comp, 768)
    assert (z == 5).all() and (comp == 5).all()
    for args, word in (((fp100, 1, 0, 64, 2), "no dft768"), ((fp100, 1, 0, 7, 2), "not one of"), ((fp100, 1, 26, 1, 2), "Illegal first_rb"),
                       ((fp100, 1, 0, 0, 2), "Illegal nb_rb"), ((fp, 1, 20, 6, 2), "leaves the band"), ((fp100, 1, 0, 1, 3), "Qm 3"),
                       ((gpu.frame_parms(6), 1, 3, 1, 2), "past the symbol"), ((gpu.frame_parms(50), 1, 25, 2, 2), "past the symbol")):
        with pytest.raises(gpu.OAI4GError, match=word):
            gpu.PuschBatch(*args)
