"""Cases of the single-layer precoding fixture (tests/golden/mod_tm456_ref.json, made by
tests/golden/gen_mod_tm456_ref.py with the reference's own dlsch_modulation.c compiled here,
oracle/_ref/libref_mod.so): MIMO_mode_t 3..8 (transmission modes 4, 5 and 6), one codeword on two
ports, the precoder of each RB taken from the 16-bit pmi_alloc by get_pmi.

Inputs are generated, not stored (e bits from mod_ref_cases.e_bits).  Each case: a frame, the mode,
pmi_alloc, MCS, subframe index, PDCCH symbols, an RB bitmap, amp and rho_A / rho_B; expected:
dlsch_modulation's return value and the digest of each antenna's subframe of the frame grid.  Cases
with "ofdm" also store the per-antenna digests of the reference's do_OFDM_mod (both slots) over that
grid, one per transform size 128, 512, 1024 and 2048.

Also here: a numpy model of the branch (dlsch_modulation.c:750-866 with layer1prec2A :108-137 and
get_pmi :1136-1178), used by the CPU tests to validate the fixture and by the GPU tests as the
description of what the kernels compute."""
import numpy as np

from mod_ref_cases import FULL, alloc_bits

PMI_WORDS = (0x0000, 0x5555, 0xAAAA, 0xFFFF, 0xE4B1, 0x1B4E)
RHOS = ((8192, 8192), (5793, 8192), (8192, 11585))
MCS = (5, 12, 22)                      # QPSK, 16-QAM, 64-QAM


def _case(k, n_rb, mode, sf, **over):
    c = dict(N_RB_DL=n_rb, Ncp=1 if k % 4 == 0 else 0, n_ant=2, mode1_flag=0, Nid_cell=(41 * k + 3) % 504,
             mimo_mode=mode, n_cw=1, mcs=[MCS[(k + k // 3) % 3]], subframe=sf,
             num_pdcch=(1, 2, 3)[k % 3] if n_rb > 10 else (2, 3, 4)[k % 3],
             rb_alloc=list(alloc_bits(k, n_rb) if k % 3 == 1 else FULL[n_rb]), amp=512,
             rho=list(RHOS[(k // 2) % 3]), pmi_alloc=PMI_WORDS[(k + k // 6) % 6], seed=[0x4560000 + k])
    c.update(over)
    return c


def modulation_cases():
    cases = []
    k = 0
    for n_rb in (6, 15, 25, 50, 100):
        for mode in (3, 5, 8):
            for sf in (0, 5, 7):
                k += 1
                cases.append(_case(k, n_rb, mode, sf))
    # all six modes at one shape: one branch, one grid
    for mode in range(3, 9):
        cases.append(_case(100, 25, mode, 7, pmi_alloc=0xE4B1, mcs=[12], seed=[0x456A000]))
    # every pmi word with each modulation at 100 PRB (13 subbands: 8..12 shift by 16 or more and read 0)
    for i, pmi in enumerate(PMI_WORDS):
        cases.append(_case(110 + i, 100, (3, 5, 8)[i % 3], (7, 0, 5)[i % 3], pmi_alloc=pmi, mcs=[MCS[i % 3]], Ncp=0,
                           rb_alloc=list(FULL[100])))
    # one TX antenna: the branch writes antenna 0 alone, at the same scaling
    cases.append(_case(120, 25, 5, 7, n_ant=1, mode1_flag=1, Ncp=0, num_pdcch=3, rb_alloc=list(FULL[25]), mcs=[12],
                       pmi_alloc=0x1B4E))
    # the C3 shape: 100 PRB, subframe 7, one PDCCH symbol, amp 512
    cases.append(dict(N_RB_DL=100, Ncp=0, n_ant=2, mode1_flag=0, Nid_cell=0, mimo_mode=7, n_cw=1, mcs=[22], subframe=7,
                      num_pdcch=1, rb_alloc=list(FULL[100]), amp=512, rho=[8192, 8192], pmi_alloc=0xE4B1,
                      seed=[0x456C300]))
    # do_OFDM_mod digests: one two-antenna case per transform size (normal prefix)
    for n_rb, mode, mcs, pmi in ((6, 3, 5, 0x0E4B), (25, 5, 12, 0x1B4E), (50, 8, 22, 0xE4B1), (100, 4, 22, 0x1B4E)):
        cases.append(_case(130 + n_rb, n_rb, mode, 5, Ncp=0, mcs=[mcs], pmi_alloc=pmi, rb_alloc=list(FULL[n_rb]),
                           ofdm=1))
    return cases


# ------------------------------------------------------------------------------------------------
# the branch restated
# ------------------------------------------------------------------------------------------------
def get_pmi(n_rb, mode, pmi_alloc, rb):
    """get_pmi (dlsch_modulation.c:1136-1178): pmi_alloc is a uint16_t widened to 32 bits"""
    sb = rb if n_rb == 6 else rb // 6 if n_rb == 50 else rb >> 3 if n_rb == 100 else rb >> 2
    w = pmi_alloc & 0xFFFF
    if mode <= 8:
        return ((w >> (2 * sb)) & 3) if 2 * sb < 32 else 0
    return ((w >> sb) & 1) if sb < 32 else 0


QAM16 = np.array([10362, 31086, -10362, -31086], np.int64)                # qam16_table: offset = 2 b0 + b2
QAM64 = np.array([15169, 5057, 25281, 35393, -15169, -5057, -25281, -35393], np.int64)   # 4 b0 + 2 b2 + b4


def amp_rho(amp, rho):
    return np.int16((int(amp) * int(rho)) >> 13)


def antenna_words(bits, Qm, amp, rho, prec, two_antennas=True):
    """(antenna 0, antenna 1) int16 (re, im) arrays [n, 2] of n REs from their e bits [n, Qm] under the
    per-RE precoder indices `prec`, at amp_rho = amp * rho >> 13 (:1223-1246)."""
    bits = np.asarray(bits, np.int64)
    a = int(amp_rho(amp, rho))
    g = (a * 23170) >> 15                                       # gain_lin_QPSK, and amp' of :753
    if Qm == 2:
        raw = np.stack([np.where(bits[:, 0] == 1, -g, g), np.where(bits[:, 1] == 1, -g, g)], axis=1)
    elif Qm == 4:
        raw = np.stack([(g * QAM16[2 * bits[:, 0] + bits[:, 2]]) >> 15, (g * QAM16[2 * bits[:, 1] + bits[:, 3]]) >> 15], axis=1)
    else:
        raw = np.stack([(g * QAM64[4 * bits[:, 0] + 2 * bits[:, 2] + bits[:, 4]]) >> 15,
                        (g * QAM64[4 * bits[:, 1] + 2 * bits[:, 3] + bits[:, 5]]) >> 15], axis=1)
    raw = raw.astype(np.int16).astype(np.int64)
    prec = np.asarray(prec)[:, None]
    re, im = raw[:, :1], raw[:, 1:]
    rot = np.where(prec == 0, np.hstack([re, im]), np.where(prec == 1, np.hstack([-re, -im]),
                   np.where(prec == 2, np.hstack([-im, re]), np.hstack([im, -re]))))
    rot = rot.astype(np.int16).astype(np.int64)                 # layer1prec2A writes int16
    if Qm == 2:                                                 # scaled after the rotation: (+-g 23170) >> 15
        raw, rot = (raw * 23170) >> 15, (rot * 23170) >> 15
    return raw.astype(np.int16), (rot.astype(np.int16) if two_antennas else None)
