"""Generates tests/golden/pcfich_rx_ref.json from the reference's own rx_pcfich.

PHY/LTE_TRANSPORT/pcfich.c and PHY/LTE_REFSIG/lte_gold.c are compiled unmodified into a temporary directory
outside the repository with the flags oracle/Makefile uses for them (PHY/defs.h, PHY/extern.h and
MAC_INTERFACE/extern.h skipped through their own include guards, the types from the pre-included
impl_defs_lte.h), beside a few lines of glue written there that fill the LTE_DL_FRAME_PARMS
(generate_pcfich_reg_mapping on N_RB_DL and Nid_cell) and the LTE_UE_PDCCH (rxdataF_comp[0]) rx_pcfich reads.
It is run on the seeded planes of tests/pdcch_front_model.py pcfich_cases() and removed; nothing compiled from
the reference is kept.  Run from the repo root, with the reference tree at $REF:

    python tests/golden/gen_pcfich_ref.py

pcfich_rx_ref.json -- one row per case name: [digest of the int32 plane, the count rx_pcfich returned].
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pdcch_front_model as F  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
R1 = os.path.join(REF, "openair1")
R2 = os.path.join(REF, "openair2")
FLAGS = ["-O2", "-fPIC", "-fcommon", "-std=gnu99", "-w", "-msse4.1", "-mssse3", "-DUSER_MODE", "-DNO_OPENAIR1", "-Dmsg=printf",
         "-D__PHY_DEFS__H__", "-D__PHY_EXTERN_H__", "-D__LIST_H__", "-D__MAC_INTERFACE_EXTERN_H__", "-D__LTE_REFSIG_DEFS__H__",
         "-DNB_ANTENNAS_RX=2", "-DNB_ANTENNAS_TX=2", "-DNB_ANTENNAS_TXRX=2",
         "-I", R1, "-I", R2, "-I", os.path.join(R1, "PHY/CODING"), "-I", os.path.join(R1, "PHY/TOOLS"),
         "-I", os.path.join(R2, "COMMON"), "-I", os.path.join(R2, "UTIL"), "-I", os.path.join(R2, "UTIL/LOG"),
         "-I", os.path.join(REF, "common/utils"), "-I", os.path.join(REF, "common/utils/itti")]
for h in ("stdint.h", "stddef.h", "stdio.h", "stdlib.h", "string.h", os.path.join(R1, "PHY/impl_defs_top.h"),
          os.path.join(R1, "PHY/impl_defs_lte.h"), os.path.join(R1, "PHY/TOOLS/defs.h"),
          os.path.join(R2, "COMMON/platform_types.h"), os.path.join(R2, "UTIL/LOG/log.h"),
          os.path.join(R1, "PHY/LTE_TRANSPORT/extern.h")):
    FLAGS += ["-include", h]

GLUE = r"""
void generate_pcfich_reg_mapping(LTE_DL_FRAME_PARMS *frame_parms);
uint8_t rx_pcfich(LTE_DL_FRAME_PARMS *frame_parms, uint8_t subframe, LTE_UE_PDCCH *lte_ue_pdcch_vars, MIMO_mode_t mimo_mode);
int gen_rx_pcfich(int N_RB_DL, int Nid_cell, int subframe, int32_t *plane0)
{
  LTE_DL_FRAME_PARMS fp;
  LTE_UE_PDCCH vars;
  int32_t *comp[8];
  memset(&fp, 0, sizeof(fp));
  memset(&vars, 0, sizeof(vars));
  memset(comp, 0, sizeof(comp));
  fp.N_RB_DL = (uint8_t)N_RB_DL;
  fp.Nid_cell = (uint16_t)Nid_cell;
  generate_pcfich_reg_mapping(&fp);
  comp[0] = plane0;
  vars.rxdataF_comp = comp;
  return rx_pcfich(&fp, (uint8_t)subframe, &vars, SISO);
}
"""


def digest(plane):
    return hashlib.sha256(np.ascontiguousarray(plane, dtype=np.int32).tobytes()).hexdigest()[:16]


def build(tmp):
    glue = os.path.join(tmp, "gen_glue.c")
    with open(glue, "w") as f:
        f.write(GLUE)
    objs = []
    for src in (os.path.join(R1, "PHY/LTE_TRANSPORT/pcfich.c"), os.path.join(R1, "PHY/LTE_REFSIG/lte_gold.c"), glue):
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        subprocess.run(["gcc"] + FLAGS + ["-c", src, "-o", obj], check=True)
        objs.append(obj)
    so = os.path.join(tmp, "libref_pcfich.so")
    subprocess.run(["gcc", "-shared", "-o", so] + objs, check=True)
    L = ctypes.CDLL(so, mode=os.RTLD_LAZY | os.RTLD_LOCAL)
    L.gen_rx_pcfich.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return L


def main():
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for name, N_RB, Nid, sf, plane in F.pcfich_cases():
            buf = np.ascontiguousarray(plane, dtype=np.int32).copy()
            n = L.gen_rx_pcfich(N_RB, Nid, sf, buf.ctypes.data)
            assert np.array_equal(buf, plane), name            # rx_pcfich does not write its input
            rows[name] = [digest(plane), int(n)]
        del L
    with open(os.path.join(HERE, "pcfich_rx_ref.json"), "w") as f:
        json.dump({"seed": F.PCFICH_SEED, "cases": rows}, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
