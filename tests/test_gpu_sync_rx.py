"""GPU tests of the UE's initial cell search (oai4g_sync_rx.hip) against the reference's own lte_sync_time.c
(tests/golden/sync_time_ref.json) and the numpy model (tests/sync_rx_model.py), on the cases of
tests/sync_time_cases.py, whose properties tests/test_sync_rx_cpu.py asserts from the model:

  - the drop-in oai4g_lte_sync_time and the batch oai4g_sync_time_batch give the reference's peak position, source
    and winning metric and every defined entry of the three correlation buffers, on every case: noise, transmitted
    frames of the three Nid2 on two antennas, all-zero input, two equal bursts, a burst behind the last counted
    position, the full-scale frame (a dot product saturated both ways, the int16 wrap of the antenna sum,
    abs32 = 2^31, a received real part of -32768), a batch of three frames with different delays and cells, 25 PRB on
    two antennas, and 100 PRB on one antenna (golden only);
  - the batch without the correlation buffers gives the same peaks;
  - oai4g_fep_offset_batch equals oai4g_slot_fep at the offsets 0, a multiple of 4, one that is not, one whose slot-10
    windows run past the frame's end, and one past the half frame, for slots 0, 1 and 10, with the offsets read at a
    stride from device memory;
  - oai4g_rx_sss and oai4g_sss_batch equal the model at 6 and 25 PRB: 1 and 2 antennas, one and two ports, all three
    Nid2, Nid1 0 and 167, a delay of more than half a frame (flip = 1, the reported offset has the half frame
    added), a neighbouring Nid2, a peak position that gives the SSS error condition; full-scale symbols, where the
    (int16_t) casts of pss_ch_est wrap, go in as rows (oai4g_sss_rows_batch);
  - the closed loop at 6 and 25 PRB, one and two ports: delayed frames of two cells -> sync_batch (PSS, SSS) -> the
    caller's grouping by cell -> oai4g_fep_offset_batch -> estimation -> PBCH front -> detection returns the
    transmitted Nid_cell, MIB, antenna count and frame_mod4 and the delay within the 4-sample grid, after the
    model found the same records on the same samples; oai4g_initial_sync gives the same on one frame, and -1
    on noise and on the SSS error condition;
  - what is out of scope is refused with a message.
"""
import ctypes

import numpy as np
import pytest

import sync_rx_model as M
import sync_time_cases as SC
from test_sync_rx_cpu import GOLDEN, MODEL_CASES, case, model, same_as_golden

pytestmark = pytest.mark.gpu


def _u32(v):
    return int(v) & 0xFFFFFFFF


@pytest.mark.parametrize("name", SC.NAMES)
def test_gpu_lte_sync_time_drop_in(gpu, name):
    N_RB, rx = case(name)
    fg = gpu.frame_parms(N_RB)
    for f in range(len(rx)):
        pos, src, val, corr = gpu.lte_sync_time(list(rx[f]), fg, want_corr=True)
        same_as_golden(name, f, pos, src, val, corr)
        assert gpu.lte_sync_time(list(rx[f]), fg) == (pos, src, val)
        if name in MODEL_CASES:
            m = model(name)[f]
            assert np.array_equal(corr[:, ::4], m["corr"][:, ::4])


@pytest.mark.parametrize("name", SC.NAMES)
def test_gpu_sync_time_batch(gpu, name):
    N_RB, rx = case(name)
    with gpu.sync_batch(gpu.frame_parms(N_RB), len(rx), rx.shape[1]) as sb:
        sb.upload(rx)
        sb.launch()
        bare = sb.peaks()
        sb.launch(want_corr=True)
        peaks, corr = sb.peaks(), sb.corr()
    assert np.array_equal(bare, peaks)
    for f in range(len(rx)):
        same_as_golden(name, f, int(peaks[f, 0]), int(peaks[f, 2]), _u32(peaks[f, 1]), corr[f])
    assert len(GOLDEN["cases"][name]) == len(rx)


def _crossing_offset(fp):
    """the sample offset at which symbol 6 of slot 10 starts half a symbol before the frame's end"""
    N, spt = fp.ofdm_symbol_size, fp.samples_per_tti
    return 10 * spt - N // 2 - 5 * spt - fp.nb_prefix_samples0 - 6 * (N + fp.nb_prefix_samples)


@pytest.mark.parametrize("N_RB,nb_rx", [(6, 2), (25, 1)])
def test_gpu_fep_offset_batch_equals_slot_fep(gpu, N_RB, nb_rx):
    fg = gpu.frame_parms(N_RB)
    N, nsymb, fl = fg.ofdm_symbol_size, fg.symbols_per_tti, 10 * fg.samples_per_tti
    offs = np.array([0, 4 * 531, 4 * 77 + 3, _crossing_offset(fg) + 2, fl // 2 + 4 * 25 + 1], dtype=np.int32)
    start6 = int(gpu.lib().oai4g_slot_fep_offset(ctypes.byref(fg), 6, 10, int(offs[3]), 0))
    assert start6 % fl < fl < start6 % fl + N       # that window does run past the end
    n = len(offs)
    rng = np.random.default_rng(N_RB)
    rx = rng.integers(-3000, 3001, (n, nb_rx, 2 * fl)).astype(np.int16).view(np.int32)
    grid = nsymb * N
    with gpu._Scratch(gpu.lib()) as t:
        d_rx, d_off, d_out = t._dev(rx.nbytes), t._dev(4 * n * 3), t._dev(n * nb_rx * grid * 4, zero=True)
        t._put(d_rx, rx)
        t._put(d_off, np.stack([offs, offs, offs], axis=1).copy())              # the offsets at a stride of 3 words
        got = {}
        for first_slot in (0, 10):
            for k, run in ((14, slice(0, 14)), (7, slice(0, 7))) if first_slot == 0 else ((7, slice(0, 7)),):
                gpu._check(t.L.oai4g_fep_offset_batch(ctypes.byref(fg), n, nb_rx, d_rx, d_off + 4, 3, first_slot, k, d_out, 0, None) == 0)
                got[(first_slot, k)] = t._get(d_out, (n, nb_rx, nsymb, N), np.int32)[:, :, run]
    for f in range(n):
        ext = [np.concatenate([rx[f, a], np.zeros(N, np.int32)]) for a in range(nb_rx)]
        for Ns in (0, 1, 10):
            want = [np.zeros(grid, np.int32) for _ in range(nb_rx)]
            for l in range(7):
                assert gpu.slot_fep(ext, want, fg, l, Ns, int(offs[f])) == 0
            for a in range(nb_rx):
                rows = want[a].reshape(nsymb, N)[7 * (Ns & 1):7 * (Ns & 1) + 7]
                if Ns == 10:
                    assert np.array_equal(got[(10, 7)][f, a], rows), (f, a)
                else:
                    assert np.array_equal(got[(0, 14)][f, a, 7 * Ns:7 * Ns + 7], rows), (f, a, Ns)
                    if Ns == 0:
                        assert np.array_equal(got[(0, 7)][f, a], rows)


def _rx_frame(N_RB, nid, nb_tx, nb_rx, delay, frame_mod4=0, sigma=40.0):
    rng = np.random.default_rng([SC.SEED, N_RB, nid, delay])
    return SC.received(SC.tx_frame(N_RB, nid, nb_tx, frame_mod4), delay, nb_rx, sigma, rng)


SSS = [(6, 0, 1, 1, 1236), (6, 502, 1, 2, 10400), (6, 503, 2, 2, 333), (25, 232, 1, 2, 40004), (25, 17, 2, 1, 4000),
       (25, 501, 1, 1, 77)]


@pytest.mark.parametrize("N_RB,nid,nb_tx,nb_rx,delay", SSS)
def test_gpu_rx_sss_equals_model(gpu, N_RB, nid, nb_tx, nb_rx, delay):
    fg = gpu.frame_parms(N_RB)
    fl = 10 * fg.samples_per_tti
    rx = _rx_frame(N_RB, nid, nb_tx, nb_rx, delay)
    peak = (SC.pss_position(N_RB, delay) & ~3, nid % 3)
    rx_offset, ok = M.offsets(peak[0], N_RB)
    (m_nid, m_metric, m_flip, m_phase), _ = M.rx_sss(list(rx), N_RB, peak[1], rx_offset)
    assert ok and m_nid == nid and m_flip == (1 if delay >= fl // 2 else 0) and m_metric > 0
    want = M.cell_search(list(rx), N_RB, peak)
    assert want[0] == nid and want[5] == 0 and 0 <= delay - want[1] < 4      # the half frame is added where flip = 1
    assert gpu.rx_sss(list(rx), fg, peak[1], rx_offset) == (m_nid, m_metric, m_flip, m_phase)
    other = (peak[0], (nid + 1) % 3)                       # the neighbouring sequence: another frame of the batch
    error = (100, nid % 3)                                 # a peak in front of the first slot's PSS position
    assert M.offsets(error[0], N_RB) == (fl + 100 - (fg.samples_per_tti // 2 - fg.ofdm_symbol_size), False)
    with gpu.sync_batch(fg, 3, nb_rx) as sb:
        sb.upload(np.stack([rx, rx, rx]))
        sb.upload_peaks([[peak[0], 0, peak[1]], [other[0], 0, other[1]], [error[0], 0, error[1]]])
        sb.launch_sss()
        cells = sb.cells()
    got = [[getattr(c, k) for k, _ in gpu.Cell._fields_] for c in cells]
    assert got[0] == want
    assert got[1] == M.cell_search(list(rx), N_RB, other) and got[1][0] % 3 == other[1]
    assert got[2] == M.cell_search(list(rx), N_RB, error) == [-1, M.offsets(100, N_RB)[0], 0, 0, 0, M.SSS_ERROR]


@pytest.mark.parametrize("N_RB,nb_rx", [(6, 1), (6, 2), (25, 2)])
def test_gpu_sss_full_scale_casts_wrap(gpu, N_RB, nb_rx):
    """Full-scale frequency-domain symbols, given to the SSS stage as rows: the forward DFT's last level scales by
    1/sqrt(2) or 1/2, which keeps slot_fep's output at or below 23170 per component (a full-scale frame through
    oai4g_rx_sss is compared as well, and the model confirms that nothing wraps there), so the wraps of pss_ch_est's
    casts are reached with rows only."""
    fg = gpu.frame_parms(N_RB)
    N, fl = fg.ofdm_symbol_size, 10 * fg.samples_per_tti
    rng = np.random.default_rng(N_RB + nb_rx)
    rx = rng.integers(-32768, 32768, (nb_rx, 2 * fl)).astype(np.int16).view(np.int32)
    want, wrapped = M.rx_sss(list(rx), N_RB, 1, 1001)
    assert not wrapped and gpu.rx_sss(list(rx), fg, 1, 1001) == want
    n = 3
    rows = rng.integers(-32768, 32768, (n, nb_rx, 4, 2 * N)).astype(np.int16).view(np.int32)
    peak0 = fg.samples_per_tti // 2 - N                     # rx_offset 0
    peaks = [[peak0 + 4 * i, 0, i] for i in range(n)]
    wants = []
    for i in range(n):
        comp = [M.pss_sss_comp(list(rows[i, :, 2 * h]), list(rows[i, :, 2 * h + 1]), i) for h in range(2)]
        assert comp[0][1] and comp[1][1]                    # casts wrapped in both halves
        nid, metric, flip, ph = M.sss_search(comp[0][0], comp[1][0], i)
        wants.append([nid, 4 * i + (fl // 2 if flip else 0), metric, flip, ph, 0])
    with gpu.sync_batch(fg, n, nb_rx) as sb, gpu._Scratch(sb.L) as t:
        d_rows = t._dev(rows.nbytes)
        t._put(d_rows, rows)
        sb.upload_peaks(peaks)
        sb.launch_sss_rows(d_rows)
        got = [[getattr(c, k) for k, _ in gpu.Cell._fields_] for c in sb.cells()]
    assert got == wants


def _closed_loop_frames(N_RB, nb_tx, nb_rx):
    cells = [(301, 18001 if N_RB == 6 else 101, 2), (77, 4444, 1), (301, 12 if N_RB == 6 else 60000, 3)]
    if N_RB == 25:
        cells = cells[:2]                                  # two model runs at 25 PRB
    return cells, np.stack([_rx_frame(N_RB, nid, nb_tx, nb_rx, d, fm4) for nid, d, fm4 in cells])


@pytest.mark.parametrize("N_RB,nb_tx,nb_rx", [(6, 1, 1), (6, 2, 2), (25, 1, 2), (25, 2, 1)])
def test_gpu_cell_search_closed_loop(gpu, N_RB, nb_tx, nb_rx):
    cells, rx = _closed_loop_frames(N_RB, nb_tx, nb_rx)
    n = len(cells)
    want = [M.cell_search(list(f), N_RB) for f in rx]       # the model finds them first, on the same samples
    for w, (nid, delay, _) in zip(want, cells):
        assert w[0] == nid and w[5] == 0 and 0 <= delay - w[1] < 4
    fg = gpu.frame_parms(N_RB)
    grid = fg.symbols_per_tti * fg.ofdm_symbol_size
    found = {}
    with gpu.sync_batch(fg, n, nb_rx) as sb:
        sb.upload(rx)
        sb.launch()
        sb.launch_sss()
        got = [[getattr(c, k) for k, _ in gpu.Cell._fields_] for c in sb.cells()]
        assert got == want
        groups = {}
        for f, c in enumerate(got):                         # the caller groups the frames by cell
            groups.setdefault(c[0], []).append(f)
        assert len(groups) == len({c[0] for c in cells})
        for nid, frames in groups.items():
            kw = dict(nb_antennas_tx=2, mode1_flag=0) if nb_tx == 2 else {}
            fc = gpu.frame_parms(N_RB, nid, **kw)
            k = 2 * len(frames)                            # a frame's rows, then the element whose row 0 closes them
            with gpu._Scratch(sb.L) as t, gpu.PbchFrontBatch(fc, k, nb_rx, nb_tx, 1, 0, 0) as fb:
                d_rxF = t._dev((k + 1) * nb_rx * grid * 4, zero=True)
                sb.fep(d_rxF, 0, 14, frames, 2 * nb_rx * grid)
                sb.fep(d_rxF + nb_rx * grid * 4, 2, 1, frames, 2 * nb_rx * grid)
                fb.estimate(d_rxF)
                fb.launch(d_rxF)
                fb.detect()
                for f, d in zip(frames, fb.detected()[::2]):
                    found[f] = (nid, d.tx_ant, d.frame_mod4, bytes(d.mib), d.mimo_mode)
    for f, (nid, _, fm4) in enumerate(cells):
        assert found[f][:4] == (nid, nb_tx, fm4, bytes(SC.PDU)), f
    # the drop-in on one frame gives the same, the first hypothesis that decoded included (with two ports through this
    # channel SISO combining may decode before ALAMOUTI is tried, initial_sync.c:135-161)
    r, out = gpu.initial_sync(list(rx[1]), fg, nb_ports=nb_tx)
    assert r == 0 and (out.Nid_cell, out.rx_offset) == tuple(want[1][:2])
    assert (out.Nid_cell, out.tx_ant, out.frame_mod4, bytes(out.mib), out.mimo_mode) == found[1]
    if nb_tx == 1:
        assert out.mimo_mode == 0


def test_gpu_initial_sync_without_a_cell(gpu):
    fg = gpu.frame_parms(6)
    rng = np.random.default_rng(3)
    noise = SC.received(np.zeros((1, 19200), np.int32), 0, 1, 200.0, rng)
    want = M.cell_search(list(noise), 6)
    r, out = gpu.initial_sync(list(noise), fg, nb_ports=1)
    assert r == -1 and out.tx_ant == 0xFF and [out.Nid_cell, out.rx_offset] == want[:2]
    r, out = gpu.initial_sync([np.zeros(19200, np.int32)], fg)           # all zero: peak 0, the SSS error condition
    assert M.offsets(0, 6)[1] is False
    assert r == -1 and out.Nid_cell == -1 and out.rx_offset == M.offsets(0, 6)[0]


def test_gpu_sync_time_refusals(gpu):
    z = np.zeros(10 * 7680, dtype=np.int32)

    def refused(call, *words):
        with pytest.raises(gpu.OAI4GError) as ei:
            call()
        assert all(w in str(ei.value) for w in words), str(ei.value)

    refused(lambda: gpu.lte_sync_time([z], gpu.frame_parms(25, frame_type=1)), "TDD")
    refused(lambda: gpu.lte_sync_time([z], gpu.frame_parms(25, Ncp=1)), "extended prefix")
    refused(lambda: gpu.lte_sync_time([z, z, z], gpu.frame_parms(25)), "3 receive antennas")
    refused(lambda: gpu.lte_sync_time([np.zeros(10 * 3840, np.int32)], gpu.frame_parms(15)), "N_RB_DL 15")
    refused(lambda: gpu.sync_batch(gpu.frame_parms(25, Ncp=1), 1, 1), "extended prefix")
