"""Generate tests/golden/mod_tm456_ref.json from the reference's dlsch_modulation.c (and, for the
"ofdm" cases, ofdm_mod.c) compiled unmodified here (oracle/_ref/libref_mod.so, libref_ofdm.so;
`make -C oracle ref`).  Inputs come from tests/mod_tm456_cases.py and mod_ref_cases.e_bits, so only
the case list, return values and digests are stored.

    python tests/golden/gen_mod_tm456_ref.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import oracle_lib as O  # noqa: E402
from mod_ref_cases import e_bits, frame_of, grid_digests  # noqa: E402
from mod_tm456_cases import modulation_cases  # noqa: E402
from rm_ref_cases import digest  # noqa: E402


def ref_modulation_pmi(fp, c):
    """The reference's dlsch_modulation over frame grids with the harq process's pmi_alloc set
    (oracle_lib.ref_modulation always passes 0): (return value, [grid per TX antenna])."""
    n = 10 * fp.symbols_per_tti * fp.ofdm_symbol_size
    grids = [np.zeros(n, dtype=np.int32) for _ in range(fp.nb_antennas_tx)]
    ptrs = (O.VP * 2)(*([g.ctypes.data for g in grids] + [None] * (2 - len(grids))))
    e = np.ascontiguousarray(e_bits(c["seed"][0])[:14 * 1200 * 6], dtype=np.uint8)
    ra = c["rb_alloc"]
    cw = O.RefCw(e=e.ctypes.data, G=len(e), mcs=c["mcs"][0], mimo_mode=c["mimo_mode"], Nlayers=1, first_layer=0,
                 nb_rb=sum(bin(int(w)).count("1") for w in ra), pmi_alloc=c["pmi_alloc"])
    for i in range(4):
        cw.rb_alloc[i] = int(ra[i])
    f = O.mod_frame_words(fp)
    ret = O.ref_mod().ref_glue_dlsch_modulation(ptrs, c["amp"], c["subframe"], f.ctypes.data, c["num_pdcch"],
                                                ctypes.byref(cw), None, c["rho"][0], c["rho"][1])
    return ret, grids


def ref_do_ofdm(fp, grids, subframe):
    """The reference's do_OFDM_mod for both slots of `subframe`: the subframe's samples per antenna."""
    spt, na = fp.samples_per_tti, fp.nb_antennas_tx
    outs = [np.zeros(10 * spt + 64, np.int32) for _ in range(na)]
    gp = (ctypes.c_void_p * na)(*[g.ctypes.data for g in grids])
    op = (ctypes.c_void_p * na)(*[o.ctypes.data for o in outs])
    for slot in (2 * subframe, 2 * subframe + 1):
        O.ref_ofdm().ref_glue_do_OFDM_mod(gp, op, 0, slot, O.P(O.frame_geometry(fp)))
    return [o[subframe * spt:(subframe + 1) * spt] for o in outs]


def main():
    assert O.ref_mod() is not None and O.ref_ofdm() is not None, "build the reference objects first: make -C oracle ref"
    out = {"source": "PHY/LTE_TRANSPORT/dlsch_modulation.c (modes 3..8), PHY/MODULATION/ofdm_mod.c (compiled "
                     "unmodified, oracle/_ref/libref_mod.so, libref_ofdm.so)", "modulation": []}
    for c in modulation_cases():
        fp = frame_of(O, c)
        ret, grids = ref_modulation_pmi(fp, c)
        row = dict(case=c, ret=int(ret), digests=grid_digests(grids, c, fp.ofdm_symbol_size))
        if c.get("ofdm"):
            row["ofdm_digests"] = [digest(x) for x in ref_do_ofdm(fp, grids, c["subframe"])]
        out["modulation"].append(row)
    path = os.path.join(HERE, "mod_tm456_ref.json")
    with open(path, "w") as f:
        f.write("{\n \"source\": " + json.dumps(out["source"]) + ",\n \"modulation\": [\n")
        f.write(",\n".join("  " + json.dumps(r) for r in out["modulation"]))
        f.write("\n ]\n}\n")
    print(path, len(out["modulation"]), "modulation cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
