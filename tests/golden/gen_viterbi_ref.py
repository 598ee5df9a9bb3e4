"""Generates tests/golden/viterbi_ref.json from the reference's own tail-biting Viterbi decoder.

PHY/CODING/viterbi_lte.c, ccoding_byte_lte.c, crc_byte.c and PHY/TOOLS/time_meas.c are compiled
unmodified into a temporary directory outside the repository, run on the seeded inputs of
tests/viterbi_cases.py, and removed; nothing compiled from the reference is kept.  Run from the repo
root, with the reference tree at $REF (default: where oracle/Makefile looks for it):

    python tests/golden/gen_viterbi_ref.py

viterbi_ref.json — one row per case "<n>_<kind>":
  y    digest of the int8[3 n] soft input (viterbi_cases.soft)
  out  the ceil(n / 8) bytes phy_viterbi_lte_sse2 added into a zeroed buffer, hex
  ok   (codeword kinds only) whether they are the transmitted payload
The clean codewords are the reference coder's (ccodelte_encode of the n - 16 payload bits with
add_crc = 2, RNTI 0) and are checked against the cases' own encoder here.
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import viterbi_cases as VC  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
PHY = os.path.join(REF, "openair1", "PHY")
COD = ["-DUSER_MODE", "-DNO_OPENAIR1", "-include", "stdint.h", "-include", os.path.join(PHY, "impl_defs_lte.h")]
VIT = ["-DUSER_MODE", "-DTEST_DEBUG", "-Dmain=ref_viterbi_main", "-include", "stdint.h", "-include", "unistd.h",
       "-msse4.1", "-mssse3"]
UNITS = [("CODING/crc_byte.c", COD), ("CODING/ccoding_byte_lte.c", COD + ["-Dmain=ref_ccoding_main"]),
         ("TOOLS/time_meas.c", COD), ("CODING/viterbi_lte.c", VIT)]


def build(tmp):
    objs = []
    for rel, flags in UNITS:
        obj = os.path.join(tmp, os.path.basename(rel) + ".o")
        subprocess.run(["gcc", "-O2", "-fPIC", "-fcommon", "-std=gnu99", "-w", "-I", os.path.join(REF, "openair1"),
                        "-I", os.path.join(PHY, "CODING"), "-I", os.path.join(PHY, "TOOLS")] + flags +
                       ["-c", os.path.join(PHY, rel), "-o", obj], check=True)
        objs.append(obj)
    so = os.path.join(tmp, "libref_viterbi.so")
    subprocess.run(["gcc", "-shared", "-o", so] + objs + ["-lm"], check=True)
    L = ctypes.CDLL(so)
    L.crcTableInit()
    L.ccodelte_init()
    L.ccodelte_init_inv()
    L.phy_generate_viterbi_tables_lte()
    L.ccodelte_encode.argtypes = [ctypes.c_int32, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint16]
    L.phy_viterbi_lte_sse2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint16]
    return L


def main():
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for name, n, kind, y in VC.cases():
            bits, packed = VC.payload(n)
            if kind == "clean":
                src = np.zeros(len(packed) + 8, np.uint8)
                src[:len(packed)] = packed
                cw = np.zeros(3 * n + 64, np.uint8)
                L.ccodelte_encode(n - 16, 2, src.ctypes.data, cw.ctypes.data, 0)
                assert np.array_equal(7 * (2 * cw[:3 * n].astype(np.int8) - 1), y), name
            ya = np.zeros(3 * n + 64, np.int8)
            ya[:3 * n] = y
            out = np.zeros(((n + 7) >> 3) + 16, np.uint8)
            L.phy_viterbi_lte_sse2(ya.ctypes.data, out.ctypes.data, n)
            assert not out[(n + 7) >> 3:].any()
            got = out[:(n + 7) >> 3]
            row = {"y": VC.digest(y), "out": got.tobytes().hex()}
            if kind in VC.SIGMA or kind == "clean":
                row["ok"] = bool(np.array_equal(got, packed))
            rows[name] = row
        del L
    with open(os.path.join(HERE, "viterbi_ref.json"), "w") as f:
        json.dump({"seed": VC.SEED, "cases": rows}, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
