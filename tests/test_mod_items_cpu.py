"""k_modofdm's dense item space, on the CPU, through the exported item map (oai4g_mod_item_map).

An item is a (subframe, symbol >= lz[, antenna pair]); the lz leading symbols that carry nothing at any
subframe index are no items, and the item of symbol lz zero-fills them.  Workgroup b of a grid of g
takes items b, b + g, b + 2g, ... (one transform per workgroup, 2048 points; u consecutive items per
round with u transforms per workgroup).  Checked here: every (subframe, symbol >= lz, pair) is one
item exactly, no symbol < lz ever is, every (subframe, pair) has one fill duty, and the deal is
balanced: at the three bench shapes every workgroup gets the same items and the same fills."""
import ctypes
from collections import Counter

import pytest

import openair4g_amd as oai

NSYMB = 14
# (n_sf, grid, per, ips)
BENCH = {(8192, 2048, 13, 1): (52, 4), (2048, 2048, 13, 1): (13, 1), (1024, 2048, 13, 2): (13, 1)}
SHAPES = list(BENCH) + [(37, 16, 13, 1), (5, 8, 13, 2), (9, 2, 11, 1), (10, 16, 14, 1), (3, 1, 13, 1),
                        (7, 4, 12, 1), (7, 4, 11, 1), (5, 8, 12, 2)]


def _map(item, ips, lz, per):
    sf, l, pair = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = oai.lib().oai4g_mod_item_map(item, ips, lz, per, ctypes.byref(sf), ctypes.byref(l), ctypes.byref(pair))
    assert rc in (0, 1), rc
    return sf.value, l.value, pair.value, rc


def _deal(n_sf, grid, per, ips, units=1):
    """per workgroup: the (sf, l, pair, fill) of its items, in the kernel's loop order"""
    lz, n_items = NSYMB - per, n_sf * per * ips
    out = [[] for _ in range(grid)]
    for b in range(grid):
        for base in range(b * units, n_items, grid * units):
            for item in range(base, min(base + units, n_items)):
                out[b].append(_map(item, ips, lz, per))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_dense_map_covers_and_balances(shape):
    n_sf, grid, per, ips = shape
    lz = NSYMB - per
    wg = _deal(*shape)
    seen = Counter((sf, l, pair) for items in wg for sf, l, pair, _ in items)
    assert set(seen) == {(sf, l, pair) for sf in range(n_sf) for l in range(lz, NSYMB) for pair in range(ips)}
    assert set(seen.values()) == {1}
    fills = Counter((sf, pair) for items in wg for sf, l, pair, f in items if f)
    if lz:
        assert fills == Counter({(sf, pair): 1 for sf in range(n_sf) for pair in range(ips)})
    else:
        assert not fills
    for items in wg:
        for sf, l, pair, f in items:
            assert f == (1 if lz and l == lz else 0)
    n = [len(items) for items in wg]
    nf = [sum(f for *_, f in items) for items in wg]
    if shape in BENCH:
        assert (set(n), set(nf)) == ({BENCH[shape][0]}, {BENCH[shape][1]})
    else:
        assert max(n) - min(n) <= 1


def test_small_transforms_deal_rounds_of_units():
    """128 points: 16 transforms per workgroup, a workgroup's round is 16 consecutive items"""
    n_sf, grid, per, ips, units = 9, 2, 11, 1, 16
    wg = _deal(n_sf, grid, per, ips, units)
    seen = Counter((sf, l) for items in wg for sf, l, _, _ in items)
    assert set(seen) == {(sf, l) for sf in range(n_sf) for l in range(3, NSYMB)} and set(seen.values()) == {1}
    assert sum(f for items in wg for *_, f in items) == n_sf
    assert [len(items) for items in wg] == [51, 48]     # 99 items: rounds 16 | 16 | 16 | 16 | 16 | 16 | 3


def test_multiply_high_split_is_exact_at_the_launch_bound():
    """the launch admits n_sf per^2 <= 2^30: the last items of the largest batch still split exactly"""
    for per in (10, 11, 12, 13, 14):
        lz, n_it = NSYMB - per if per >= 10 else 0, (1 << 30) // (per * per) * per
        for it in (n_it - 1, n_it - per, n_it - per - 1, n_it // 2, per, per - 1, 0):
            for ips in (1, 2):
                for pair in range(ips):
                    assert _map(it * ips + pair, ips, lz, per)[:3] == (it // per, lz + it % per, pair)


def test_arguments_out_of_range_are_refused():
    out = [ctypes.c_uint32(7) for _ in range(3)]
    refs = [ctypes.byref(o) for o in out]
    for ips, lz, per in ((0, 1, 13), (3, 1, 13), (1, 5, 9), (1, 0, 0)):
        assert oai.lib().oai4g_mod_item_map(0, ips, lz, per, *refs) < 0
    assert [o.value for o in out] == [7, 7, 7]
