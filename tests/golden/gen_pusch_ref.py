"""Generates tests/golden/pusch_ref.json and pusch_ref_vectors.npz from the reference's own SC-FDMA code.

PHY/TOOLS/lte_dfts.c, PHY/LTE_TRANSPORT/ulsch_modulation.c and PHY/LTE_REFSIG/lte_gold.c are compiled unmodified into a temporary directory outside the repository, with a few lines of glue of ours (a switch
over the dftN entry points, the QAM tables by generate_16qam_table / generate_64qam_table's formula, get_Qm_ul's three
ranges (lte_mcs.c:57-67 does not compile alone), subframe2harq_pid, the VCD / log / assert stubs, and an LTE_UE_ULSCH_t filled from the case), run on the seeded inputs of
tests/pusch_cases.py, and removed; nothing compiled from the reference is kept.  Run from the repo root, with the
reference tree at $REF:

    python tests/golden/gen_pusch_ref.py

pusch_ref.json:
  dft        per size the digests of the 36 output rows of dftN(x, y, 1) on pusch_cases.dft_input(N), four rows per
             call interleaved as dft_lte interleaves them (dft12 has no scale flag and does not scale)
  dft_lte    per size the digest of z after dft_lte(z, d, Msc, 12) with d = rows 0..11
  mod        per case of pusch_cases.MOD_CASES the digest of the subframe's grid [nsymb][N] of txdataF[0], pre-filled
             with pusch_cases.grid_pattern, after ulsch_modulation, and the digest of ulsch->z
  past       per entry of pusch_cases.MOD_PAST_SYMBOL how many words the reference wrote at or beyond RE N of a symbol
  refused    the reference's own refusals (first_rb 26, nb_rb 0, harq_pid 8): 1 when the grid kept its pattern
  seconds    the reference's single-core time of one ulsch_modulation call per nb_rb (N_RB_DL 100, 16-QAM), best of 50
pusch_ref_vectors.npz: the full output rows, int16 [36][N][2], of the sizes in pusch_cases.VECTOR_SIZES
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pusch_cases as PC  # noqa: E402
from gen_sync_time_ref import DFTS, FLAGS, PHY, SYNC  # noqa: E402

GLUE = """
#include "PHY/LTE_TRANSPORT/defs.h"
int qam64_table[8], qam16_table[4];
void logRecord(const char *file, const char *func, int line, int comp, int level, const char *format, ...) {}
void vcd_signal_dumper_dump_function_by_name(int name, int in) {}
void DevAssert(const void *p) { if (!p) abort(); }   /* assertions.h is not among the includes: the call is implicit */
unsigned char get_Qm_ul(unsigned char I_MCS) { return I_MCS < 11 ? 2 : I_MCS < 21 ? 4 : 6; }
static int glue_pid;
uint8_t subframe2harq_pid(LTE_DL_FRAME_PARMS *fp, uint32_t frame, uint8_t subframe) { return glue_pid; }
void dft_lte(mod_sym_t *z, mod_sym_t *d, int32_t Msc_PUSCH, uint8_t Nsymb);
void ulsch_modulation(mod_sym_t **txdataF, short amp, uint32_t frame, uint32_t subframe, LTE_DL_FRAME_PARMS *fp, LTE_UE_ULSCH_t *ulsch);
#define D(n) void dft##n(int16_t *, int16_t *, unsigned char);
D(24) D(36) D(48) D(60) D(72) D(96) D(108) D(120) D(144) D(180) D(192) D(216) D(240) D(288) D(300) D(324) D(360) D(384)
D(432) D(480) D(540) D(576) D(600) D(648) D(720) D(864) D(900) D(960) D(972) D(1080) D(1152) D(1200)
#undef D
void dft12(int16_t *, int16_t *);
int glue_dft(int n, int16_t *x, int16_t *y)
{
  switch (n) {
  case 12: dft12(x, y); return 0;
#define C(n) case n: dft##n(x, y, 1); return 0;
  C(24) C(36) C(48) C(60) C(72) C(96) C(108) C(120) C(144) C(180) C(192) C(216) C(240) C(288) C(300) C(324) C(360) C(384)
  C(432) C(480) C(540) C(576) C(600) C(648) C(720) C(864) C(900) C(960) C(972) C(1080) C(1152) C(1200)
  }
  return -1;
}
void glue_dft_lte(int32_t *z, int32_t *d, int Msc, int Nsymb) { dft_lte((mod_sym_t *)z, (mod_sym_t *)d, Msc, Nsymb); }
static LTE_UE_ULSCH_t ulsch;
static LTE_UL_UE_HARQ_t harq;
static LTE_DL_FRAME_PARMS fp;
void glue_tables(void)
{
  for (int a = -1; a <= 1; a += 2)
    for (int b = -1; b <= 1; b += 2) {
      qam16_table[(1 + a) + (1 + b) / 2] = -a * (QAM16_n1 + b * QAM16_n2);
      for (int c = -1; c <= 1; c += 2) qam64_table[(1 + a) * 2 + (1 + b) + (1 + c) / 2] = -a * (QAM64_n1 + b * (QAM64_n2 + c * QAM64_n3));
    }
}
int32_t *glue_z(void) { return (int32_t *)ulsch.z; }
void glue_mod(int32_t *txdataF0, int amp, int subframe, int N_RB_DL, int N, int Ncp, int Nid_cell, int rnti, int first_rb,
              int nb_rb, int Qm, int srs_active, const uint8_t *h, int nh, int pid)
{
  mod_sym_t *tx[1] = {(mod_sym_t *)txdataF0};
  memset(&fp, 0, sizeof(fp));
  fp.N_RB_DL = N_RB_DL; fp.N_RB_UL = N_RB_DL; fp.ofdm_symbol_size = N; fp.first_carrier_offset = N - 6 * N_RB_DL;
  fp.Ncp = Ncp; fp.Nid_cell = Nid_cell;
  memset(&harq, 0, sizeof(harq));
  harq.first_rb = first_rb; harq.nb_rb = nb_rb; harq.mcs = Qm == 2 ? 5 : Qm == 4 ? 15 : 25;
  for (int i = 0; i < 8; i++) ulsch.harq_processes[i] = &harq;
  ulsch.rnti = rnti; ulsch.srs_active = srs_active; ulsch.cooperation_flag = 0;
  ulsch.Nsymb_pusch = (Ncp ? 10 : 12) - srs_active;
  memcpy(ulsch.h, h, nh);
  glue_pid = pid;
  ulsch_modulation(tx, amp, 0, subframe, &fp, &ulsch);
}
"""


def build(tmp):
    glue = os.path.join(tmp, "pusch_glue.c")
    open(glue, "w").write(GLUE)
    T = PHY + "/LTE_TRANSPORT/"
    plain = FLAGS + SYNC[:-2]             # without primary_synch.h, which defines its tables
    units = [(T + "ulsch_modulation.c", FLAGS + SYNC), (PHY + "/LTE_REFSIG/lte_gold.c", plain + ["-D__LTE_REFSIG_DEFS__H__"]),
             (PHY + "/TOOLS/lte_dfts.c", DFTS), (glue, plain)]
    objs = []
    for src, flags in units:
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        subprocess.run(["gcc"] + flags + ["-c", src, "-o", obj], check=True)
        objs.append(obj)
    so = os.path.join(tmp, "libref_pusch.so")
    subprocess.run(["gcc", "-shared", "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-o", so] + objs + ["-lm"], check=True)
    L = ctypes.CDLL(so)
    L.glue_z.restype = ctypes.POINTER(ctypes.c_int32)
    L.glue_tables()
    return L


def _aligned(n_words, fill=None):
    """int32 [n_words] at a 32-byte boundary (the reference loads and stores 16 bytes at a time)"""
    raw = np.zeros(n_words + 16, dtype=np.int32)
    off = (-raw.ctypes.data % 32) // 4
    out = raw[off:off + n_words]
    if fill is not None:
        out[:] = fill
    return out


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


def ref_dft(L, N, x):
    """int16 [36][N][2] -> the same, four rows per reference call"""
    y = np.zeros_like(x)
    for i in range(0, len(x), 4):
        xin = _aligned(4 * N, np.ascontiguousarray(x[i:i + 4].transpose(1, 0, 2)).view(np.int32).ravel())
        yout = _aligned(4 * N)
        assert L.glue_dft(N, P(xin), P(yout)) == 0
        y[i:i + 4] = yout.view(np.int16).reshape(N, 4, 2).transpose(1, 0, 2)
    return y


def ref_mod(L, c, first_rb=None, nb_rb=None, pid=0, tail=0):
    """the case through ulsch_modulation: (grid int16 [nsymb][N][2] (+ tail words), z int16 [G / Qm][2])"""
    first_rb = c["first_rb"] if first_rb is None else first_rb
    nb_rb = c["nb_rb"] if nb_rb is None else nb_rb
    nsymb, N = c["nsymb"], c["N"]
    pat = PC.grid_pattern((nsymb * N + tail,))
    frame = _aligned(10 * nsymb * N + tail)
    sf = c["subframe"]
    frame[sf * nsymb * N:sf * nsymb * N + nsymb * N + tail] = pat.view(np.int32).ravel()
    h = np.ascontiguousarray(c["h"])
    t0 = time.perf_counter()
    L.glue_mod(P(frame), c["amp"], sf, c["N_RB_DL"], N, c["Ncp"], c["Nid_cell"], c["rnti"], first_rb, nb_rb, c["Qm"],
               c["srs_active"], P(h), h.size, pid)
    ref_mod.seconds = time.perf_counter() - t0
    assert not frame[:sf * nsymb * N].any()
    grid = frame[sf * nsymb * N:sf * nsymb * N + nsymb * N + tail].view(np.int16).reshape(-1, 2).copy()
    z = np.ctypeslib.as_array(L.glue_z(), (c["G"] // c["Qm"],)).view(np.int16).reshape(-1, 2).copy()
    return grid, z, pat


def main():
    out = {"seed": PC.SEED, "dft": {}, "dft_lte": {}, "mod": [], "past": [], "refused": {}, "seconds": {}}
    vec = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for N in PC.SIZES:
            x = PC.dft_input(N)
            y = ref_dft(L, N, x)
            out["dft"][str(N)] = [PC.digest(r) for r in y]
            if N in PC.VECTOR_SIZES:
                vec[f"dft{N}"] = y
            d = _aligned(12 * N, x[:12].view(np.int32).ravel())
            z = _aligned(12 * N)
            L.glue_dft_lte(P(z), P(d), N, 12)
            out["dft_lte"][str(N)] = PC.digest(z)
        for i in range(len(PC.MOD_CASES)):
            c = PC.mod_case(i)
            grid, z, _ = ref_mod(L, c)
            out["mod"].append({"grid": PC.digest(grid), "z": PC.digest(z)})
            if i in (0, 2):
                vec[f"mod{i}_grid"] = grid
        for N_RB_DL, first_rb, nb_rb in PC.MOD_PAST_SYMBOL:
            c = dict(PC.mod_case(0), N_RB_DL=N_RB_DL, N=PC.fft_size(N_RB_DL), Ncp=0, nsymb=14, srs_active=0, Qm=2, G=12 * nb_rb * 24,
                     h=np.zeros(12 * nb_rb * 24 + 64, np.uint8))
            grid, _, pat = ref_mod(L, c, first_rb, nb_rb, tail=12 * nb_rb)
            changed = (grid != pat).any(1).reshape(-1)
            k = np.nonzero(changed)[0]
            # every changed word lies in [l N + N, l N + N + Msc) of a data symbol l: RE >= N of its own symbol
            past = sum(1 for v in k if (v % c["N"]) < 12 * nb_rb and v >= c["N"])
            out["past"].append({"changed": int(changed.sum()), "past_symbol": int(past), "in_tail": int(changed[14 * c["N"]:].sum())})
        c = PC.mod_case(8)
        for name, kw in (("first_rb_26", dict(first_rb=26)), ("nb_rb_0", dict(nb_rb=0)), ("harq_pid_8", dict(pid=8))):
            grid, _, pat = ref_mod(L, c, **kw)
            out["refused"][name] = int((grid == pat).all())
        for nb_rb in (6, 25, 50, 100):
            c = dict(PC.mod_case(0), N_RB_DL=100, N=2048, Ncp=0, nsymb=14, srs_active=0, Qm=4, first_rb=0, nb_rb=nb_rb,
                     G=12 * nb_rb * 48, h=np.random.default_rng(nb_rb).integers(0, 2, 12 * nb_rb * 48 + 64).astype(np.uint8))
            best = 1.0
            for _ in range(50):
                ref_mod(L, c)
                best = min(best, ref_mod.seconds)
            out["seconds"][str(nb_rb)] = round(best, 7)
        del L
    with open(os.path.join(HERE, "pusch_ref.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "pusch_ref_vectors.npz"), **vec)


if __name__ == "__main__":
    main()
