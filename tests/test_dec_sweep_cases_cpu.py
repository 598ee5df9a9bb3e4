"""Conditions on the inputs of the decoder sweep (tests/dec_sweep_cases.py), on the oracle alone, so
that tests/test_gpu_dec_sweep.py cannot pass by testing nothing: the batches make blocks of one wave
stop at different iterations at every size, the filler offset of the CRC is observable, and the
sweep reaches every schedule class of both kernels that the table holds."""
import numpy as np
import pytest

import dec_sweep_cases as D

SIZES = {16: D.K16, 8: D.K8}


@pytest.mark.parametrize("bits", [16, 8])
def test_iteration_spread(bits):
    """At every size the main batch holds a block that stops at iteration 2 and one that returns
    max_iterations + 1; at 90 % of the sizes at least, also one that stops at 3..8.  With the ladder
    and the seeds of dec_sweep_cases the oracle gives 182 of 188 sizes for the 16-bit decoder (none
    at K = 88, 128, 312, 384, 504, 1760) and all 129 for the 8-bit one."""
    mid = 0
    for K in SIZES[bits]:
        its, _ = D.oracle_main(bits, K)
        assert its[D.MAIN_CLEAN] == 2, K
        assert D.MAIN_MAX_IT + 1 in its, K
        assert its.max() <= D.MAIN_MAX_IT + 1, K
        mid += any(3 <= i <= D.MAIN_MAX_IT for i in its)
    print("decoder%d: %d of %d sizes hold a block stopping at 3..8" % (bits, mid, len(SIZES[bits])))
    assert mid >= 0.9 * len(SIZES[bits])


@pytest.mark.parametrize("bits", [16, 8])
def test_filler_offset_is_observable(bits):
    """The clean block of every filler batch with F > 0 stops at iteration 2 with its F and runs to
    max_iterations + 1 with F = 0: a decoder that started the CRC at byte 0 would be seen."""
    assert [D.filler_F(K) for K in (40, 512, 528, 1024, 1056, 2048, 2112, 6144)] == [0, 0, 8, 8, 24, 24, 56, 56]
    n = 0
    for K in SIZES[bits]:
        b = D.filler_batch(K)
        its, _ = D.oracle_filler(bits, K)
        assert its[D.FILL_CLEAN] == 2, K
        if b.F:
            n += 1
            assert np.all(b.c[D.FILL_CLEAN][:b.F // 8] != 0), K
            it0, _ = D.DECODERS[bits](b.y[D.FILL_CLEAN], K, max_it=b.max_it, crc_type=b.crc_type, F=0)
            assert it0 == b.max_it + 1, K
    assert n == 128


@pytest.mark.parametrize("bits", [16, 8])
def test_clean_blocks_decode(bits):
    for K in SIZES[bits]:
        assert np.array_equal(D.oracle_main(bits, K)[1][D.MAIN_CLEAN], D.main_batch(K).c[D.MAIN_CLEAN]), K
        assert np.array_equal(D.oracle_filler(bits, K)[1][D.FILL_CLEAN], D.filler_batch(K).c[D.FILL_CLEAN]), K


def test_batches_are_seeded_and_padded():
    for K in (40, 1056, 6144):
        b = D.main_batch(K)
        assert b.y.shape == (14, 3 * K + 12) and b.y.dtype == np.int16
        assert D.filler_batch(K).y.shape == (5, 3 * K + 12)
        p = b.padded(3 * K + 16)
        assert np.array_equal(p[:, :3 * K + 12], b.y) and np.all(p[:, 3 * K + 12:] == 0x7fff)
        D.main_batch.cache_clear()
        assert np.array_equal(D.main_batch(K).y, b.y)                # the same inputs wherever they are built
    # the amplitudes put every input-scaling shift of the 8-bit decoder into one batch
    K = 1056
    mean = [int(np.abs(r[:3 * K].astype(np.int64)).mean()) for r in D.main_batch(K).y[:5]]
    assert [sum(m >= t for t in (16, 32, 64, 128)) for m in mean] == [0, 1, 2, 3, 4], mean
    assert D.w3_rows(40).shape == (64, 132)


def _table(fn, sizes, earlier, restrict=None):
    """per class: values in the table, reached by the earlier sizes, added by the sweep"""
    pick = [K for K in sizes if restrict is None or restrict(K)]
    all_v = D.class_values(fn, pick)
    old_v = D.class_values(fn, [K for K in earlier if K in pick])
    rows = {}
    for name, vals in all_v.items():
        old = old_v.get(name, set())
        rows[name] = (len(vals), len(old), len(vals - old))
    return rows, all_v, old_v


def _print(title, rows):
    print(title)
    print("  %-16s %8s %8s %8s" % ("class", "values", "earlier", "added"))
    for name, (n, o, a) in rows.items():
        print("  %-16s %8d %8d %8d" % (name, n, o, a))


def test_class_coverage():
    """Every class value of the table occurs in the sweep (it runs every size, so this pins the size
    lists), and the counts that motivated the sweep stay true of the earlier files."""
    assert set(D.EARLIER16) <= set(D.K16) and set(D.EARLIER8) <= set(D.K8)
    assert D.class_values(D.classes16, D.K16) == D.class_values(D.classes16, sorted(D.QPP))
    assert D.class_values(D.classes8, D.K8) == D.class_values(D.classes8, [K for K in D.QPP if K >= 512 and K % 16 == 0])

    rows, _, _ = _table(D.classes16, D.K16, D.EARLIER16)
    _print("k_td16, all 188 sizes", rows)
    big = lambda K: K > 320                                          # noqa: E731
    rows, all_v, old_v = _table(D.classes16, D.K16, D.EARLIER16, big)
    _print("k_td16, the 152 sizes above 320", rows)
    assert len([K for K in D.K16 if big(K)]) == 152
    assert sorted(K for K in D.EARLIER16 if big(K)) == [512, 1024, 1056, 2048, 3520, 3584, 5504, 6144]
    assert rows["K1 mod 12"] == (12, 3, 9)
    assert rows["crc mod 8"] == (8, 2, 6)
    assert rows["K/8 mod 32"] == (28, 4, 24)

    rows, all_v, old_v = _table(D.classes8, D.K8, D.EARLIER8)
    _print("k_td8, the 129 legal sizes", rows)
    assert len(D.EARLIER8) == 9
    assert 3 in all_v["K1 mod 4"] and 3 not in old_v["K1 mod 4"]
    assert sum(D.classes8(K)["K1 mod 4"] == 3 for K in D.K8) == 8
    assert rows["K1 mod 16"] == (16, 5, 11)
    assert rows["crc mod 16"] == (8, 4, 4)
    assert rows["K1 mod 8"] == (8, 4, 4)

    # the filler batches move the CRC class: with F = 8, 24, 56 the chunk class shifts by 1, 3, 7
    fill16 = {D.classes16(K, D.filler_F(K))["crc mod 8"] for K in D.K16}
    fill8 = {D.classes8(K, D.filler_F(K))["crc mod 16"] for K in D.K8}
    print("crc classes of the filler batches: k_td16 %s, k_td8 %s" % (sorted(fill16), sorted(fill8)))
    assert fill16 == set(range(8))
