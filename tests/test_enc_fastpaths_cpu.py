"""Host-side pieces of k_encode's per-geometry fast paths, on the CPU.

The lane-exact segment encoder (turbo_segment32<Q>, block sizes with 32 | K) scans the chunk exit
states over lanes with packed propagation rows: row d is the constituent encoder's zero-input state
map over 32 Q 2^d steps, the image of state s in bits 4s..4s+2.  oai4g_rsc_scan_rows returns the rows
the kernel is compiled with; this file steps the trellis (3gpplte_sse.c:96-102) one bit at a time.

Phase 4 (sub-block interleaving + rate matching) takes its tile pairs from a host-built schedule,
oai4g_rm_pair_schedule; the arithmetic the kernel used to step through the same pairs is restated
here, and the schedule is compared with it for all 188 block sizes."""
import ctypes
import re
from pathlib import Path

import pytest

import openair4g_amd as oai


def _step0(s):
    """one zero-input step: state bits (s2 s1 s0), s' = ((s1 ^ s0) << 2) | (s2 << 1) | s1"""
    s2, s1, s0 = (s >> 2) & 1, (s >> 1) & 1, s & 1
    return ((s1 ^ s0) << 2) | (s2 << 1) | s1


def _rows(q):
    rows = (ctypes.c_uint32 * 6)(*([0xdeadbeef] * 6))
    return oai.lib().oai4g_rsc_scan_rows(q, rows), list(rows)


@pytest.mark.parametrize("q", [1, 2, 3])
def test_scan_rows_are_single_steps_repeated(q):
    rc, rows = _rows(q)
    assert rc == 0
    for d in range(6):
        for s in range(8):
            st = s
            for _ in range(32 * q << d):
                st = _step0(st)
            assert (rows[d] >> (4 * s)) & 0xf == st, (q, d, s)


def test_state_zero_stays_zero():
    """what lets a lane below 2^d look up entry 0 instead of being masked off"""
    for q in (1, 2, 3):
        assert all(r & 0xf == 0 for r in _rows(q)[1])


@pytest.mark.parametrize("q", [0, 4, 64])
def test_other_chunk_counts_are_refused(q):
    rc, rows = _rows(q)
    assert rc == -1
    assert rows == [0xdeadbeef] * 6   # outputs untouched


# ---- phase 4: the tile-pair schedule (oai4g_rm_pair_schedule) against the walk it replaces ----

RM_TILES = 20
NWAVES = 4
U32 = 0xffffffff


def _sizes():
    text = (Path(__file__).resolve().parent.parent / "include" / "oai4g_qpp.c").read_text()
    ks = [int(m[0]) for m in re.findall(r"\{\s*(\d+),\s*(\d+),\s*(\d+)\}", text)]
    assert len(ks) == 188 and ks == sorted(ks)
    return ks


def _tiles(K):
    """plan tiles of a block: v0 tiles of 32 rows, then interlaced tiles of 16 row pairs"""
    R = (K + 4 + 31) // 32
    return (R + 31) // 32 + (R + 15) // 16


def _schedule(C, n0, nt, wrapt):
    pairs = (ctypes.c_uint32 * (10 * 16 + 1))(*([0xdeadbeef] * (10 * 16 + 1)))
    pair0 = (ctypes.c_uint32 * 18)(*([0xdeadbeef] * 18))
    rc = oai.lib().oai4g_rm_pair_schedule(C, n0, (ctypes.c_uint32 * 2)(*nt), (ctypes.c_uint32 * 2)(*wrapt), pairs, pair0)
    return rc, list(pairs), list(pair0)


def _stepped_walk(C, n0, nt, wrapt, rb0, rb1, wave):
    """The pairs wave `wave` visits in blocks [rb0, rb1), with each pair's scalars, by the arithmetic
    the kernel stepped with before the schedule: decode the first pair by a magic-number division,
    then step 2 NWAVES tiles on, carrying over block ends."""
    pp = [(nt[0] + 1) >> 1, (nt[1] + 1) >> 1]
    psplit = n0 * pp[0]
    pm = [((1 << 20) + p - 1) // p if p else 0 for p in pp]

    def pair0(r):
        return r * pp[0] if r < n0 else psplit + (r - n0) * pp[1]

    pb, pe = pair0(rb0), pair0(rb1)
    P = pb + wave
    if P >= pe:
        return []
    ki = 1 if P >= psplit else 0
    PP = P - psplit if ki else P
    rr = (PP * pm[ki]) >> 20
    r, t0 = (n0 + rr if ki else rr), 2 * (PP - rr * pp[ki])
    out = []
    while P < pe:
        row = ki * ((RM_TILES + 1) * 32) + t0 * 32                 # plan-row word offset
        wrap = 1 if ((wrapt[ki] - t0) & U32) < 2 else 0           # t0 or t0 + 1 is the wrap tile
        out.append((P, ki, r, row, wrap))
        t0 += 2 * NWAVES
        tpb = 2 * pp[ki]
        if t0 >= tpb:
            while True:
                t0 -= tpb
                r += 1
                ki = 1 if r >= n0 else 0
                tpb = 2 * pp[ki]
                if t0 < tpb:
                    break
        P += NWAVES
    return out


def test_pair_schedule_equals_the_stepped_walk():
    ks = _sizes()
    checked = 0
    for i, K in enumerate(ks):
        Km = ks[i - 1] if i else K                                  # K- of a two-size codeword
        nt = (_tiles(Km), _tiles(K))
        assert 2 <= nt[0] <= nt[1] <= RM_TILES
        for C in range(1, 14):
            splits = sorted({0, C, 1 if C > 1 else 0, C // 2})
            # no wrap tile, the general-path mark, and wrap tiles that move with (K, C): first, odd last, mid
            wraps = [(U32, U32), (U32 - 1, U32 - 1), ((K + C) % nt[0], (K // 8 + C) % nt[1]), (nt[0] - 1, 0)]
            for n0 in splits:
                for wrapt in wraps[(K // 8 + C + n0) % 2::2]:      # two of the four per shape
                    rc, pairs, pair0 = _schedule(C, n0, nt, wrapt)
                    pp = [(nt[0] + 1) // 2, (nt[1] + 1) // 2]
                    total = n0 * pp[0] + (C - n0) * pp[1]
                    assert rc == total and pair0[C] == total
                    assert pairs[total] == 0xdeadbeef and pair0[C + 1] == 0xdeadbeef
                    hb = (C + 1) // 2
                    for rb0, rb1 in ((0, hb), (hb, C)):
                        pb, pe = pair0[rb0], pair0[rb1]
                        seen = 0
                        for wave in range(NWAVES):
                            want = _stepped_walk(C, n0, nt, wrapt, rb0, rb1, wave)
                            got = []
                            for P in range(pb + wave, pe, NWAVES):
                                d = pairs[P]
                                assert d & 0xe000ffc0 == 0 and (d >> 16) % 4 == 0
                                got.append((P, (d >> 1) & 1, (d >> 2) & 15, (d >> 16) // 4, d & 1))
                            assert got == want, (K, C, n0, wrapt, rb0, rb1, wave)
                            seen += len(got)
                        assert seen == pe - pb
                    checked += 1
    assert checked >= 188 * 13 * 2 * 2


def test_pair_schedule_refuses_out_of_range():
    assert _schedule(0, 0, (20, 20), (U32, U32))[0] < 0
    assert _schedule(17, 0, (20, 20), (U32, U32))[0] < 0
    assert _schedule(3, 4, (20, 20), (U32, U32))[0] < 0
    assert _schedule(3, 1, (20, 21), (U32, U32))[0] < 0
    assert _schedule(3, 1, (0, 20), (U32, U32))[0] < 0
    assert _schedule(3, 0, (0, 20), (U32, U32))[0] == 30      # the unused size's tiles are not looked at
