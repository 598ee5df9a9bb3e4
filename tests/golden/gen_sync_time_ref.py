"""Generates tests/golden/sync_time_ref.json from the reference's own PSS time-domain correlation.

PHY/LTE_ESTIMATION/lte_sync_time.c, PHY/TOOLS/cdot_prod.c and PHY/TOOLS/lte_dfts.c are compiled unmodified into a
temporary directory outside the repository, with a few lines of glue of ours (malloc16, logRecord, and a frame
parameter block filled from N_RB_DL; the file-scope syncF_tmp, which lte_sync_time_init never clears, is zeroed
before each size as a process that starts at that size finds it), run on the seeded inputs of tests/sync_time_cases.py, and removed; nothing
compiled from the reference is kept.  Run from the repo root, with the reference tree at $REF (default: where
oracle/Makefile looks for it) and the oracle built (the cases' transmitted frames are the oracle's):

    python tests/golden/gen_sync_time_ref.py

sync_time_ref.json:
  replicas   per N_RB_DL the digests of primary_synch0..2_time after lte_sync_time_init (N int16 pairs each)
  cases      per case a list with one row per frame:
               rx        digest of the frame's input, int32 [nb_rx][10 samples_per_tti]
               peak_pos  lte_sync_time's return value
               source    *eNB_id
               peak_val  (sync_corr[peak_pos] >> 1) + (sync_corr[peak_pos + length] >> 1) of the source's buffer
               corr      digests of every fourth entry of sync_corr_ue0..2 (the entries the function defines)
  seconds    per N_RB_DL and antenna count the reference's single-core run time per frame on the generating machine
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
import sync_time_cases as SC  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
R1 = os.path.join(REF, "openair1")
PHY = os.path.join(R1, "PHY")
# REFMOD_FLAGS of oracle/Makefile, and what lte_sync_time.c needs beyond them
FLAGS = ["-O2", "-fPIC", "-fcommon", "-std=gnu99", "-w", "-msse4.1", "-mssse3", "-DUSER_MODE", "-DNO_OPENAIR1", "-Dmsg=printf",
         "-D__PHY_DEFS__H__", "-D__PHY_EXTERN_H__", "-D__LIST_H__", "-D__MAC_INTERFACE_EXTERN_H__", "-DNB_ANTENNAS_RX=2",
         "-DNB_ANTENNAS_TX=2", "-DNB_ANTENNAS_TXRX=2",
         "-I", R1, "-I", REF + "/openair2", "-I", PHY + "/CODING", "-I", PHY + "/TOOLS", "-I", REF + "/openair2/COMMON",
         "-I", REF + "/openair2/UTIL", "-I", REF + "/openair2/UTIL/LOG", "-I", REF + "/common/utils",
         "-I", REF + "/common/utils/itti"]
for h in ("stdint.h", "stddef.h", "stdio.h", "stdlib.h", "string.h", PHY + "/impl_defs_top.h", PHY + "/impl_defs_lte.h",
          PHY + "/TOOLS/defs.h", REF + "/openair2/COMMON/platform_types.h", REF + "/openair2/UTIL/LOG/log.h",
          PHY + "/LTE_TRANSPORT/extern.h"):
    FLAGS += ["-include", h]
SYNC = ["-D__LTE_ESTIMATION_DEFS__H__", "-D__MAC_INTERFACE_DEFS_H__", "-D__SCHED_EXTERN_H__", "-include", "math.h",
        "-include", PHY + "/LTE_REFSIG/primary_synch.h"]
DFTS = ["-O2", "-fPIC", "-fcommon", "-std=gnu99", "-w", "-msse4.1", "-mssse3", "-DUSER_MODE", "-D__PHY_DEFS__H__",
        "-D__PHY_EXTERN_H__", "-DNB_ANTENNAS_RX=2", "-DNB_ANTENNAS_TX=2", "-DNB_ANTENNAS_TXRX=2", "-I", R1, "-I", PHY + "/TOOLS",
        "-include", "stdint.h", "-include", "stdio.h", "-include", "stdlib.h", "-include", "string.h", "-include", "math.h",
        "-include", PHY + "/impl_defs_top.h"]
TOOLS = ["-O2", "-fPIC", "-std=gnu99", "-w", "-msse4.1", "-mssse3", "-DUSER_MODE", "-I", R1, "-I", PHY + "/TOOLS"]

DECLS = """int16_t *primary_synch0_time, *primary_synch1_time, *primary_synch2_time;
void *malloc16(size_t);
"""
GLUE = """
void *malloc16(size_t n) { void *p = 0; return posix_memalign(&p, 32, n) ? 0 : p; }
void logRecord(const char *file, const char *func, int line, int comp, int level, const char *format, ...) {}
extern int16_t *primary_synch0_time, *primary_synch1_time, *primary_synch2_time;
extern int *sync_corr_ue0, *sync_corr_ue1, *sync_corr_ue2;
extern short syncF_tmp[];
int lte_sync_time_init(LTE_DL_FRAME_PARMS *);
int lte_sync_time(int **, LTE_DL_FRAME_PARMS *, int *);
void lte_sync_time_free(void);
static LTE_DL_FRAME_PARMS fp;
int glue_init(int N_RB_DL, int N, int log2N, int nb_rx)
{
  memset(&fp, 0, sizeof(fp));
  memset(syncF_tmp, 0, sizeof(short) * 2048 * 2);   /* as a process that starts at this N_RB_DL finds it */
  fp.N_RB_DL = N_RB_DL;
  fp.ofdm_symbol_size = N;
  fp.log2_symbol_size = log2N;
  fp.samples_per_tti = 15 * N;
  fp.nb_prefix_samples = 9 * N / 128;
  fp.nb_prefix_samples0 = 10 * N / 128;
  fp.nb_antennas_rx = nb_rx;
  return lte_sync_time_init(&fp);
}
int glue_sync(int **rxdata, int *source) { return lte_sync_time(rxdata, &fp, source); }
int16_t *glue_replica(int s) { return s == 0 ? primary_synch0_time : s == 1 ? primary_synch1_time : primary_synch2_time; }
int *glue_corr(int s) { return s == 0 ? sync_corr_ue0 : s == 1 ? sync_corr_ue1 : sync_corr_ue2; }
void glue_free(void) { lte_sync_time_free(); }
"""


def build(tmp):
    decl = os.path.join(tmp, "sync_decls.h")
    glue = os.path.join(tmp, "sync_glue.c")
    open(decl, "w").write(DECLS)
    open(glue, "w").write(GLUE)
    units = [(PHY + "/LTE_ESTIMATION/lte_sync_time.c", FLAGS + SYNC + ["-include", decl]), (PHY + "/TOOLS/cdot_prod.c", TOOLS),
             (PHY + "/TOOLS/lte_dfts.c", DFTS), (glue, FLAGS)]
    objs = []
    for src, flags in units:
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        subprocess.run(["gcc"] + flags + ["-c", src, "-o", obj], check=True)
        objs.append(obj)
    so = os.path.join(tmp, "libref_sync_time.so")
    subprocess.run(["gcc", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm"], check=True)
    L = ctypes.CDLL(so)
    L.glue_replica.restype = ctypes.POINTER(ctypes.c_int16)
    L.glue_corr.restype = ctypes.POINTER(ctypes.c_int32)
    L.glue_sync.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int)]
    return L


def _aligned(a):
    """a copy of the frame at a 32-byte boundary with room behind it (the reference loads 16 bytes at a time)"""
    raw = np.zeros(a.size + 64, dtype=np.int32)
    off = (-raw.ctypes.data % 32) // 4
    out = raw[off:off + a.size]
    out[:] = a
    return out


def main():
    out = {"seed": SC.SEED, "replicas": {}, "cases": {}, "seconds": {}}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for name in SC.NAMES:
            N_RB, rx = SC.case(name)
            N = rx.shape[2] // 150
            nb_rx, fl = rx.shape[1], rx.shape[2]
            assert L.glue_init(N_RB, N, N.bit_length() - 1, nb_rx) == 1
            reps = [np.ctypeslib.as_array(L.glue_replica(s), (2 * N,)).copy() for s in range(3)]
            out["replicas"].setdefault(str(N_RB), [SC.digest(r) for r in reps])
            assert out["replicas"][str(N_RB)] == [SC.digest(r) for r in reps]
            rows = []
            for f in range(len(rx)):
                keep = [_aligned(rx[f, a]) for a in range(nb_rx)]
                ptrs = (ctypes.c_void_p * nb_rx)(*[k.ctypes.data for k in keep])
                src = ctypes.c_int(-1)
                t0 = time.perf_counter()
                pos = L.glue_sync(ptrs, ctypes.byref(src))
                dt = time.perf_counter() - t0
                corr = [np.ctypeslib.as_array(L.glue_corr(s), (fl,)).copy() for s in range(3)]
                c = corr[src.value]
                val = ((int(c[pos]) >> 1) + (int(c[pos + fl // 2]) >> 1)) & 0xFFFFFFFF
                rows.append({"rx": SC.digest(rx[f]), "peak_pos": pos, "source": src.value, "peak_val": val,
                             "corr": [SC.digest(x[::4]) for x in corr]})
                key = f"{N_RB}x{nb_rx}"
                out["seconds"][key] = round(min(dt, out["seconds"].get(key, dt)), 4)
            out["cases"][name] = rows
            L.glue_free()
        del L
    with open(os.path.join(HERE, "sync_time_ref.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
