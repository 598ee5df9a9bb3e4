"""Single-layer precoding (MIMO_mode_t 3..8, transmission modes 4-6), the parts that need no GPU:
  - oai4g_get_pmi (host function of the HIP library) against a restatement of get_pmi
    (dlsch_modulation.c:1136-1178), every bandwidth, modes 3..11, every RB;
  - a numpy model of the branch (mod_tm456_cases.antenna_words over the spec's RE order,
    spec_model.pdsch_res) against the reference's own dlsch_modulation.c where oracle/_ref is built,
    and against the fixture's digests everywhere: this validates the fixture and the model;
  - the two ABI structs that gained pmi_alloc keep their size;
  - without a device oai4g_tx_config_create refuses mode 3 with an error."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import openair4g_amd as oai
import spec_model as S
from mod_ref_cases import e_bits, frame_of, grid_digests
from mod_tm456_cases import antenna_words, get_pmi, modulation_cases
from rm_ref_cases import digest

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "mod_tm456_ref.json")))
QM = {5: 2, 12: 4, 22: 6}


def _lib():
    return oai.lib()       # raises when the library is not built: a failure, not a skip


@pytest.mark.parametrize("n_rb", [6, 15, 25, 50, 100])
def test_get_pmi_equals_restatement(n_rb):
    L = _lib()
    rng = np.random.default_rng(0x456 + n_rb)
    words = [0, 0x5555, 0xAAAA, 0xFFFF, 0xE4B1, 0x1B4E] + [int(w) for w in rng.integers(0, 1 << 16, 300)]
    for mode in range(3, 12):
        for w in words:
            got = [L.oai4g_get_pmi(n_rb, mode, w, rb) for rb in range(n_rb)]
            assert got == [get_pmi(n_rb, mode, w, rb) for rb in range(n_rb)], (mode, hex(w))


def test_get_pmi_100prb_rb64_and_up_reads_precoder_0():
    """pmi_alloc is a uint16_t widened to uint32_t: subbands 8..12 at 100 PRB shift by 16 or more"""
    L = _lib()
    for mode in (3, 5, 8):
        assert [L.oai4g_get_pmi(100, mode, 0xFFFF, rb) for rb in range(64, 100)] == [0] * 36
        assert L.oai4g_get_pmi(100, mode, 0xFFFF, 63) == 3
    assert L.oai4g_get_pmi(50, 5, 0xFFFF, 47) == 3 and L.oai4g_get_pmi(50, 5, 0xFFFF, 48) == 0


def model_grids(c):
    """the frame grids of case c from the numpy model: (re_allocated, [grid per antenna])"""
    fp = frame_of(O, c)
    N, nsymb, n_ant = fp.ofdm_symbol_size, fp.symbols_per_tti, c["n_ant"]
    Qm = QM[c["mcs"][0]]
    res = S.pdsch_res(c["N_RB_DL"], N, fp.first_carrier_offset, fp.nushift, c["num_pdcch"], c["subframe"],
                      1 if c["mode1_flag"] else 2, c["Ncp"], c["rb_alloc"])
    n = len(res)
    bits = e_bits(c["seed"][0])[:n * Qm].reshape(n, Qm)
    l = np.array([r[0] for r in res])
    pos = l * N + np.array([r[1] for r in res])
    prec = np.array([get_pmi(c["N_RB_DL"], c["mimo_mode"], c["pmi_alloc"], r[2]) for r in res])
    pil = np.array([S.crs_symbol(int(x), c["Ncp"]) for x in l])
    grids = [np.zeros((10 * nsymb * N, 2), np.int16) for _ in range(n_ant)]
    for sel, rho in ((~pil, c["rho"][0]), (pil, c["rho"][1])):
        a0, a1 = antenna_words(bits[sel], Qm, c["amp"], rho, prec[sel], n_ant == 2)
        grids[0][c["subframe"] * nsymb * N + pos[sel]] = a0
        if n_ant == 2:
            grids[1][c["subframe"] * nsymb * N + pos[sel]] = a1
    return n, [g.view(np.int32).ravel() for g in grids]


def test_fixture_is_current():
    assert [m["case"] for m in FIX["modulation"]] == json.loads(json.dumps(modulation_cases()))
    sizes = {m["case"]["N_RB_DL"] for m in FIX["modulation"] if "ofdm_digests" in m}
    assert sizes == {6, 25, 50, 100}
    assert os.path.getsize(os.path.join(HERE, "golden", "mod_tm456_ref.json")) < 60 * 1024


@pytest.mark.parametrize("i", range(len(FIX["modulation"])))
def test_model_equals_reference_and_fixture(i):
    m = FIX["modulation"][i]
    c = m["case"]
    fp = frame_of(O, c)
    ret, grids = model_grids(c)
    assert ret == m["ret"]
    assert grid_digests(grids, c, fp.ofdm_symbol_size) == m["digests"]
    if O.ref_mod() is not None:                      # live, where the reference objects are built
        sys.path.insert(0, os.path.join(HERE, "golden"))
        from gen_mod_tm456_ref import ref_do_ofdm, ref_modulation_pmi
        rret, rgrids = ref_modulation_pmi(fp, c)
        assert rret == ret
        for a in range(c["n_ant"]):
            assert np.array_equal(rgrids[a], grids[a]), a
        if "ofdm_digests" in m and O.ref_ofdm() is not None:
            assert [digest(x) for x in ref_do_ofdm(fp, rgrids, c["subframe"])] == m["ofdm_digests"]


def test_all_six_modes_give_one_grid():
    sweep = [m for m in FIX["modulation"] if m["case"]["seed"] == [0x456A000]]
    assert sorted(m["case"]["mimo_mode"] for m in sweep) == [3, 4, 5, 6, 7, 8]
    assert len({tuple(m["digests"]) for m in sweep}) == 1


def test_qpsk_negative_level_is_the_floor():
    """amp 512, rho 8192: g = 362, levels 255 and -256; antenna 1 minus the arithmetically rotated
    antenna 0 is in {-1, 0} (the scaling comes after the rotation)"""
    bits = np.array([[0, 0], [0, 1], [1, 0], [1, 1]] * 4)
    prec = np.repeat(np.arange(4), 4)
    a0, a1 = antenna_words(bits, 2, 512, 8192, prec)
    assert sorted(set(a0.ravel().tolist())) == [-256, 255]
    a0 = a0.astype(np.int64)
    rot = np.where(prec[:, None] == 0, a0, np.where(prec[:, None] == 1, -a0, np.where(
        prec[:, None] == 2, np.stack([-a0[:, 1], a0[:, 0]], 1), np.stack([a0[:, 1], -a0[:, 0]], 1))))
    d = a1.astype(np.int64) - rot
    assert set(d.ravel().tolist()) == {-1, 0}
    # QAM levels at amp 512: the negative ones are floors, antenna 1 the exact rotation
    b16 = np.array([[(v >> j) & 1 for j in range(4)] for v in range(16)])
    q0, q1 = antenna_words(b16, 4, 512, 8192, np.full(16, 1))
    assert sorted(set(np.abs(q0).ravel().tolist())) == [114, 115, 343, 344]
    assert np.array_equal(q1, -q0)
    b64 = np.array([[(v >> j) & 1 for j in range(6)] for v in range(64)])
    q0, _ = antenna_words(b64, 6, 512, 8192, np.zeros(64, int))
    assert sorted(set(np.abs(q0).ravel().tolist())) == [55, 56, 167, 168, 279, 280, 390, 391]


def _csize(struct):
    src = '#include <stdio.h>\n#include "oai4g.h"\nint main(void){printf("%zu\\n", sizeof(' + struct + '));return 0;}\n'
    exe = os.path.join(os.environ.get("TMPDIR", "/tmp"), "oai4g_sz_%d_%s" % (os.getpid(), struct))
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(os.path.dirname(HERE), "include"), "-o", exe],
                   input=src.encode(), check=True)
    try:
        return int(subprocess.run([exe], capture_output=True, check=True).stdout)
    finally:
        os.remove(exe)


def test_struct_sizes_unchanged():
    """pmi_alloc sits in what was padding of oai4g_dl_harq_t and in reserved[0] of oai4g_tx_params_t:
    the sizes are those of the layouts without it"""
    class HarqBefore(ctypes.Structure):
        _fields_ = oai.DlHarq._fields_[:-1]
    assert oai.DlHarq._fields_[-1][0] == "pmi_alloc" and oai.DlHarq._fields_[-2][0] == "first_layer"
    assert ctypes.sizeof(oai.DlHarq) == ctypes.sizeof(HarqBefore) == _csize("oai4g_dl_harq_t")
    assert oai.DlHarq.pmi_alloc.offset == oai.DlHarq.first_layer.offset + 2   # 16-bit aligned, in the padding

    class ParamsBefore(ctypes.Structure):
        _fields_ = [f for f in oai.TxParams._fields_ if f[0] not in ("pmi_alloc", "reserved")] + \
            [("reserved", ctypes.c_uint32 * 7)]
    assert ctypes.sizeof(oai.TxParams) == ctypes.sizeof(ParamsBefore) == _csize("oai4g_tx_params_t")
    assert oai.TxParams.pmi_alloc.offset == ParamsBefore.reserved.offset


def test_config_create_refuses_cleanly():
    """oai4g_tx_config_create with mode 3 in a fresh process: without a device it returns NULL with an
    error and does not crash; with one, the valid configuration is accepted and two codewords, one
    antenna or pmi_alloc bits above 16 are refused with an error"""
    _lib()
    code = ("import ctypes, openair4g_amd as oai\n"
            "L = oai.lib()\n"
            "dev = L.oai4g_init() == 0\n"
            "def create(**kw):\n"
            "    p = oai.make_params('TM6')\n"
            "    p.mimo_mode = oai.UNIFORM_PRECODING11\n"
            "    for k, v in kw.items(): setattr(p, k, v)\n"
            "    cfg = L.oai4g_tx_config_create(ctypes.byref(p))\n"
            "    ok = bool(cfg)\n"
            "    if cfg: L.oai4g_tx_config_destroy(cfg)\n"
            "    return ok, bool(L.oai4g_last_error())\n"
            "print(dev, create(), create(n_cw=2), create(nb_antennas_tx=1, mode1_flag=1), create(pmi_alloc=0x10000))\n")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    bad = "(False, True)"
    if r.stdout.startswith("True"):
        assert r.stdout.strip() == " ".join(["True", "(True, True)"] + [bad] * 3) or \
            r.stdout.strip() == " ".join(["True", "(True, False)"] + [bad] * 3), r.stdout
    else:
        assert r.stdout.strip() == " ".join(["False"] + [bad] * 4), r.stdout
