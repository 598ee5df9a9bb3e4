"""CPU suite: the rate-matching geometry header (openair4g_amd/csrc/oai4g_rm_geom.h), the one statement of
Ncb, k0, E and the compaction over the NULLs that the host layer's transmit and receive sides share.

One stand-alone C++17 program, built with the address and undefined-behaviour sanitizers, includes the header
alone and answers the cases it reads on stdin: rm_ref_cases.rm_geometries(K) x Kmimo 1/2 x rv 0-3 for all 188
block sizes.  E is checked against what the reference's own lte_rate_matching_turbo returned
(tests/golden/rm_ref.json; 0 where it takes the "RM condition" exit), Ncb and k0 against the expressions of
spec_model.rate_match (36.212 5.1.4.1.2), Nnn and k0c against counts over the oracle's generate_dummy_w masks,
from both NULL representations (the position list and the mask).
"""
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as O
import rm_ref_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openair4g_amd", "csrc")
NSOFT, MDLHARQ = 1827072, 8

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "oai4g_rm_geom.h"

int main()
{
  static char mask[32768];
  char tag[4];
  while (scanf("%3s", tag) == 1) {
    if (tag[0] == 'g') {   /* g Nsoft Kmimo Mdlharq C RTC G Nl Qm r rv -> Ncb shorter k0 E (0 on the RM-condition exit) */
      unsigned Nsoft, Kmimo, Mdlharq, C, RTC, G, Nl, Qm, r, rv;
      if (scanf("%u %u %u %u %u %u %u %u %u %u", &Nsoft, &Kmimo, &Mdlharq, &C, &RTC, &G, &Nl, &Qm, &r, &rv) != 10) return 2;
      const rm_ncb_t g = rm_ncb(Nsoft, Kmimo, Mdlharq, C, RTC);
      if (g.Kw != 96 * RTC || g.shorter != (g.Ncb < g.Kw)) return 3;
      printf("%u %d %u %u\n", g.Ncb, g.shorter ? 1 : 0, rm_k0(RTC, g.Ncb, rv), g.shorter ? 0u : rm_E(G, Nl, Qm, C, r));
    } else {               /* m mask('0' / '1' per w entry) n x1 .. xn -> per x: non-NULL below x by list and by mask */
      unsigned n;
      if (scanf("%32767s %u", mask, &n) != 2) return 2;
      const size_t len = strlen(mask);
      std::vector<uint8_t> w(len);      /* exactly len entries: a read past x is the sanitizer's to catch */
      std::vector<uint16_t> pos;
      for (size_t q = 0; q < len; q++) {
        w[q] = mask[q] == '1' ? 2 : 0;
        if (w[q]) pos.push_back((uint16_t)q);
      }
      for (unsigned i = 0; i < n; i++) {
        unsigned x;
        if (scanf("%u", &x) != 1 || x > len) return 2;
        printf("%u %u\n", rm_compact(x, rm_null_list{pos.data(), (uint32_t)pos.size()}),
               rm_compact(x, rm_null_mask{w.data(), 2}));
      }
    }
  }
  return 0;
}
"""


def _cases():
    """(stdin text, expected output lines)"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "rm_ref.json")))["rm"]
    lines, want = [], []
    assert len(RC.KS) == 188
    for K in RC.KS:
        D = K + 4
        R = (D + 31) >> 5
        Kw = 3 * 32 * R
        Es = gold[str(K)][0]
        xs = set()
        i = 0
        for (G, C, r, Qm, Nl) in RC.rm_geometries(K):
            for Kmimo in (1, 2):
                for rv in range(4):
                    # spec_model.rate_match: Nir, Ncb and k0 = R (2 ceil(Ncb / 8R) rv + 2)
                    Nir = NSOFT // (Kmimo * min(MDLHARQ, 8))
                    Ncb = min(Nir // C, Kw)
                    k0 = R * (2 * (-(-Ncb // (8 * R))) * rv + 2)
                    lines.append(f"g {NSOFT} {Kmimo} {MDLHARQ} {C} {R} {G} {Nl} {Qm} {r} {rv}")
                    want.append(f"{Ncb} {int(Ncb < Kw)} {k0} {Es[i]}")
                    assert (Es[i] == 0) == (Ncb < Kw), (K, i)        # the fixture holds the RM-condition exits as E = 0
                    xs.update(x for x in (Ncb, k0) if x <= Kw)
                    i += 1
        assert i == len(Es)
        for F in RC.DUMMY_F:
            if F >= K:
                continue
            null = O.dummy_w_F(D, F)[:Kw] == 2
            below = np.concatenate(([0], np.cumsum(~null)))          # non-NULL entries of w[0..x)
            q = sorted(xs | {0, 1, Kw})
            lines.append("m " + "".join("1" if v else "0" for v in null) + f" {len(q)} " + " ".join(map(str, q)))
            want += [f"{below[x]} {below[x]}" for x in q]
    return "\n".join(lines) + "\n", want


def test_rm_geometry_header_under_sanitizers():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    text, want = _cases()
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "rm_geom_test.cpp"), os.path.join(d, "rm_geom_test")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe], check=True)
        run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-500:] + run.stderr
    got = run.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:5]
    assert any(w.split()[1] == "1" for w in want)                    # RM-condition exits are among the cases
