"""The 32-fold of the QPP interleaver (k_encode phase 3a's fast path), on the CPU.

With Q = K/32, a size whose QPP satisfies Pi(k + Q) = Pi(k) + s Q (mod K) for every k interleaves as
a column gather plus a per-column rotate of the block held as a 32 x Q bit matrix:
T[x] (bit j = c[x + Q (s j mod 32)]) -> word k (bit j = c'[k + Q j]) = T[Pi(k) mod Q] rotated right by
s^-1 (Pi(k) div Q) mod 32.  oai4g_qpp_fold32 is the library's predicate and table builder (what
derive_cfg uploads); this file recomputes Pi from its definition for all 188 sizes and runs the table
through a numpy model of exactly that layout."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import openair4g_amd as oai

ROOT = Path(__file__).resolve().parent.parent
ELIGIBLE = {1024, 2048, 3072, 4096, 5120, 6144}


def _rows():
    text = (ROOT / "include" / "oai4g_qpp.c").read_text()
    rows = [tuple(int(v) for v in m) for m in re.findall(r"\{\s*(\d+),\s*(\d+),\s*(\d+)\}", text)]
    assert len(rows) == 188
    return rows


ROWS = _rows()


def _pi(K, f1, f2):
    k = np.arange(K, dtype=np.int64)
    return (f1 * k + f2 * k * k) % K


def _fold32(K):
    s = ctypes.c_uint32(0xdead)
    tab = np.full(192, 0xffff, dtype=np.uint16)
    rc = oai.lib().oai4g_qpp_fold32(K, ctypes.byref(s), tab.ctypes.data_as(ctypes.c_void_p))
    return rc, s.value, tab


def test_eligible_set_is_exact():
    got = {K for K, _, _ in ROWS if _fold32(K)[0] == 1}
    assert got == ELIGIBLE


def test_illegal_size_is_an_error():
    assert _fold32(1000)[0] < 0
    assert _fold32(0)[0] < 0


@pytest.mark.parametrize("K", [5504, 6080, 40, 1056, 6016])
def test_ineligible_reports_fallback(K):
    rc, s, tab = _fold32(K)
    assert rc == 0
    assert s == 0xdead and np.all(tab == 0xffff)   # outputs untouched


@pytest.mark.parametrize("K", sorted(ELIGIBLE))
def test_multiplier_and_fold_identity(K):
    f1, f2 = next((a, b) for k, a, b in ROWS if k == K)
    rc, s, _ = _fold32(K)
    assert rc == 1
    Q = K // 32
    assert s == (f1 + f2 * Q) % 32 and s % 2 == 1
    pi = _pi(K, f1, f2)
    assert np.array_equal(np.roll(pi, -Q), (pi + s * Q) % K)   # Pi(k + Q) = Pi(k) + s Q for every k


@pytest.mark.parametrize("K", sorted(ELIGIBLE))
def test_table_interleaves_in_the_transposed_layout(K):
    f1, f2 = next((a, b) for k, a, b in ROWS if k == K)
    rc, s, tab = _fold32(K)
    assert rc == 1
    Q = K // 32
    pi = _pi(K, f1, f2)
    rng = np.random.default_rng(K)
    c = rng.integers(0, 2, size=K, dtype=np.uint64)
    j = np.arange(32)
    # forward transpose: T[x] bit j = c[x + Q (s j mod 32)]
    T = np.zeros(Q, dtype=np.uint64)
    for x in range(Q):
        T[x] = np.sum(c[x + Q * ((s * j) % 32)] << j.astype(np.uint64))
    # gather + rotate from the 16-bit entries: rotate in bits 0-4, word index in bits 7-14
    e = tab[:Q].astype(np.uint64)
    assert np.all(e & np.uint64(0x8060) == 0)
    rot, xw = e & np.uint64(31), e >> np.uint64(7)
    assert np.all(xw < Q)
    t = T[xw.astype(np.int64)]
    W = ((t >> rot) | (t << (np.uint64(32) - rot))) & np.uint64(0xffffffff)
    # back transpose: c'[k + Q j] = bit j of W[k]
    out = np.zeros(K, dtype=np.uint64)
    for jj in range(32):
        out[jj * Q:(jj + 1) * Q] = (W >> np.uint64(jj)) & np.uint64(1)
    assert np.array_equal(out, c[pi])
    assert np.all(tab[Q:] == 0xffff)   # K/32 entries written, no more
