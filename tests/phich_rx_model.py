"""numpy restatement of rx_phich's numeric core (PHY/LTE_TRANSPORT/phich.c:1112-1346, normal prefix, normal
duration):

  1. cs[i] = 1 - 2 bit_i of the first Gold word of c_init = ((subframe + 1)(Nid_cell + 1) << 9) + Nid_cell, i < 12;
  2. the 24 signs d of nseq_PHICH 0..7 (the switch at :1131-1222): symbol i = 4 quad + j carries the orthogonal
     sign w[nseq & 3][j] cs[i] on re and im; sequences 4..7 put -cs on re and +cs on im;
  3. HI16 += x d over the 8 int16 at word phich_reg[ngroup][quad] * 4 of plane 0 of the PDCCH front's rxdataF_comp
     (symbol 0, packed 8 per RB), accumulated in int16_t: it wraps after every term;
  4. NACK iff HI16 > 0.
"""
import numpy as np

import ctrl_rx_model as M
from pdcch_front_model import _wrap16

W = ((1, 1, 1, 1), (1, -1, 1, -1), (1, 1, -1, -1), (1, -1, -1, 1))


def signs(Nid_cell, subframe, nseq):
    s = M.gold_words((((subframe + 1) * (Nid_cell + 1)) << 9) + Nid_cell, 1)[0]
    cs = [1 - 2 * ((s >> i) & 1) for i in range(12)]
    d = np.zeros(24, dtype=np.int64)
    for i in range(12):
        w = W[nseq & 3][i & 3] * cs[i]
        d[2 * i] = w if nseq < 4 else -w
        d[2 * i + 1] = w
    return d


def rx_phich(comp, regs, ngroup, nseq, Nid_cell, subframe):
    """comp: plane 0 (int32 words), regs: the PHICH REG mapping [(r0, r1, r2)].  Returns (nack, HI16, the sum
    without the int16 wrap)."""
    comp = np.asarray(comp, dtype=np.int32)
    x = np.concatenate([comp[4 * r:4 * r + 4] for r in regs[ngroup]]).view(np.int16).astype(np.int64)
    d = signs(Nid_cell, subframe, nseq)
    hi = 0
    for v, s in zip(x, d):
        hi = int(_wrap16(hi + int(v) * int(s)))
    return int(hi > 0), hi, int((x * d).sum())
