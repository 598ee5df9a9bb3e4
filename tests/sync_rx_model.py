"""numpy restatement of the UE's initial cell search — TEST INFRASTRUCTURE ONLY.

  replicas      lte_sync_time_init (PHY/LTE_ESTIMATION/lte_sync_time.c:143-292): the three time-domain PSS replicas,
                from the oracle's pinned primary_synch tables and its pinned fixed-point inverse DFT;
  sync_time     lte_sync_time (:357-517) with dot_product (PHY/TOOLS/cdot_prod.c:40-118) stated per tap:
                (xr yr + xi yi) >> 15 and (xr yi + xi (int16)(-yr)) >> 15, the pair sums and the running sums
                wrapping in 32 bits, one saturation to int16 at the end; the antennas added in int16; abs32 in int;
                the metric compared as unsigned, strictly greater, n ascending then s.

  offsets       initial_sync's offset arithmetic (PHY/LTE_TRANSPORT/initial_sync.c:310-354, FDD, normal prefix);
  slot_fep      slot_fep's window at a sample offset (PHY/MODULATION/slot_fep.c:105-150) through the oracle's pinned
                forward DFT, read on from the frame's start where it runs past the end;
  rx_sss        pss_sss_extract, pss_ch_est and the hypothesis search (PHY/LTE_TRANSPORT/sss.c:93-391) with every
                >> 15, >> 19 and (int16_t) cast where the reference has them;
  cell_search   the record oai4g_sss_batch reports per frame.

tests/golden/sync_time_ref.json (the reference's own lte_sync_time.c, see tests/golden/gen_sync_time_ref.py) pins
replicas and sync_time.  rx_sss takes PHY_VARS_UE and cannot be compiled alone: its tables and DFT are pinned
elsewhere (tests/test_sync_cpu.py, the DFT pins), its phase constants in tests/test_sync_rx_cpu.py, and the whole in
the closed loop.  Kept at <= 25 PRB in the tests: a 100 PRB frame is 4.7e8 complex products per antenna.
"""
import numpy as np

import oracle_lib as O

SIZE = {6: 128, 25: 512, 50: 1024, 100: 2048}


def replicas(N_RB):
    """int16 [3][N][2]"""
    N = SIZE[N_RB]
    out = np.zeros((3, N, 2), dtype=np.int16)
    for s in range(3):
        ps = O.primary_synch(s).reshape(72, 2)
        F = np.zeros((N, 2), dtype=np.int16)
        k = N - 36
        for i in range(72):
            F[k] = ps[i] >> 2
            k += 1
            if k >= N:
                k = k + 1 - N                              # "skip DC carrier" (:151-154)
        out[s] = O.idft(F.ravel(), 1).reshape(N, 2)
    return out


PHASE_RE = (16383, 25101, 30791, 32767, 30791, 25101, 16383)          # sss.c:218-219
PHASE_IM = (-28378, -21063, -11208, 0, 11207, 21062, 28377)
SSS_ERROR = 1


def offsets(peak_pos, N_RB):
    """initial_sync.c:310-354 (FDD, normal prefix): (rx_offset, whether rx_sss runs)"""
    N = SIZE[N_RB]
    spt, cp = 15 * N, 9 * N // 128
    frame = 10 * spt
    sync_pos2 = peak_pos - cp if peak_pos >= cp else peak_pos + frame - cp
    d = sync_pos2 - (spt // 2 - N - cp)
    return (d if d >= 0 else frame + d), 0 <= d < frame - spt // 2


def fep_window(N_RB, Ns, l, sample_offset):
    """where slot_fep's DFT window of symbol l of slot Ns starts (slot_fep.c:105-150), modulo the frame"""
    N = SIZE[N_RB]
    spt, cp, cp0 = 15 * N, 9 * N // 128, 10 * N // 128
    off = (sample_offset + (spt // 2) * (Ns % 2) + cp0 + spt * (Ns // 2)) & 0xFFFFFFFF
    off -= off % 4
    return (off + (N + cp) * l) % (10 * spt)


def slot_fep(rx, N_RB, Ns, l, sample_offset):
    """the oracle's pinned forward DFT of that window, read on from the frame's start: int32 [N] per antenna"""
    N = SIZE[N_RB]
    st = fep_window(N_RB, Ns, l, sample_offset)
    out = []
    for a in rx:
        a = np.ascontiguousarray(a, dtype=np.int32)
        w = np.concatenate([a, a[:N]])[st:st + N]
        out.append(O.dft(w.view(np.int16), 1).view(np.int32))
    return out


def _c(v):
    return np.asarray(v, dtype=np.int64)


def _i16(v):
    return v.astype(np.int16).astype(np.int64)


def pss_sss_comp(rxF_sss, rxF_pss, Nid2):
    """pss_sss_extract (sss.c:157-215) and pss_ch_est (:93-154) of one slot's two symbols, per antenna int32 [N]:
    the 62 compensated words int16 [62][2], and whether any (int16_t) cast wrapped"""
    N = len(rxF_sss[0])
    bins = np.array([N - 36 + j if j < 36 else j - 35 for j in range(5, 67)])
    p = _c(O.primary_synch(Nid2).reshape(72, 2)[5:67])
    acc = np.zeros((62, 2), dtype=np.int64)
    wrapped = False
    for ys, yp in zip(rxF_sss, rxF_pss):
        e = _c(np.ascontiguousarray(yp, np.int32)[bins].view(np.int16).reshape(-1, 2))
        y = _c(np.ascontiguousarray(ys, np.int32)[bins].view(np.int16).reshape(-1, 2))
        wide = [((e[:, 0] * p[:, 0]) >> 15) + ((e[:, 1] * p[:, 1]) >> 15), ((e[:, 0] * p[:, 1]) >> 15) - ((e[:, 1] * p[:, 0]) >> 15)]
        tr, ti = _i16(wide[0]), _i16(wide[1])
        wide += [((tr * y[:, 0]) >> 15) - ((ti * y[:, 1]) >> 15), ((tr * y[:, 1]) >> 15) + ((ti * y[:, 0]) >> 15)]
        r2, i2 = _i16(wide[2]), _i16(wide[3])
        wide += [acc[:, 0] + r2, acc[:, 1] + i2]
        wrapped = wrapped or any((w != _i16(w)).any() for w in wide)
        acc = np.stack([_i16(wide[4]), _i16(wide[5])], axis=1)
    return acc, wrapped


def sss_search(sss0, sss5, Nid2):
    """the hypothesis search of rx_sss (sss.c:350-388): (Nid_cell, metric, flip, phase)"""
    d0 = np.stack([_c(O.sss_seq(Nid2 + 3 * n1, 0)) for n1 in range(168)])     # [168][62]
    d5 = np.stack([_c(O.sss_seq(Nid2 + 3 * n1, 1)) for n1 in range(168)])
    best = (-99999999, None)
    for flip in range(2):
        t0, t5 = (d0, d5) if flip == 0 else (d5, d0)
        for ph in range(7):
            A0 = ((PHASE_RE[ph] * sss0[:, 0]) >> 19) - ((PHASE_IM[ph] * sss0[:, 1]) >> 19)
            A5 = ((PHASE_RE[ph] * sss5[:, 0]) >> 19) - ((PHASE_IM[ph] * sss5[:, 1]) >> 19)
            metric = _i16(t0 * A0 + t5 * A5).sum(axis=1)
            n1 = int(np.argmax(metric))                    # the first of the largest
            if metric[n1] > best[0]:
                best = (int(metric[n1]), (Nid2 + 3 * n1, int(metric[n1]), flip, ph))
    return best[1]


def rx_sss(rx, N_RB, Nid2, rx_offset):
    """rx_sss on one frame: (Nid_cell, metric, flip, phase), and whether a cast of the compensation wrapped"""
    comp, wrapped = [], False
    for Ns in (0, 10):
        c, w = pss_sss_comp(slot_fep(rx, N_RB, Ns, 5, rx_offset), slot_fep(rx, N_RB, Ns, 6, rx_offset), Nid2)
        comp.append(c)
        wrapped = wrapped or w
    return sss_search(comp[0], comp[1], Nid2), wrapped


def cell_search(rx, N_RB, peak=None):
    """the PSS and SSS stages as oai4g_sss_batch reports them: the cell record
    [Nid_cell, rx_offset, metric, flip, phase, status]; peak = (peak_pos, Nid2) skips the PSS stage"""
    if peak is None:
        m = sync_time(rx, N_RB)
        peak = (m["peak_pos"], m["source"])
    rx_offset, ok = offsets(peak[0], N_RB)
    if not ok:
        return [-1, rx_offset, 0, 0, 0, SSS_ERROR]
    (nid, metric, flip, ph), _ = rx_sss(rx, N_RB, peak[1], rx_offset)
    return [nid, rx_offset + (5 * 15 * SIZE[N_RB] if flip else 0), metric, flip, ph, 0]


def _wrap32(v):
    """int64 -> int32, modulo 2^32"""
    return (v.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _sat16(v):
    return np.clip(v, -32768, 32767).astype(np.int16)


def dot_products(x, y, positions, wide_neg=False, chunk=1024):
    """dot_product(x, y + n, N, 15) for every n of positions: x int16 [N][2], y int16 [L][2] -> (re, im) int16.
    wide_neg negates the received real part in a wider type (what the reference does not do)."""
    N = len(x)
    xr, xi = x[:, 0].astype(np.int64), x[:, 1].astype(np.int64)
    wr = np.lib.stride_tricks.sliding_window_view(y[:, 0], N)
    wi = np.lib.stride_tricks.sliding_window_view(y[:, 1], N)
    positions = np.asarray(positions)
    re = np.zeros(len(positions), dtype=np.int16)
    im = np.zeros(len(positions), dtype=np.int16)
    for c in range(0, len(positions), chunk):
        p = positions[c:c + chunk]
        yr, yi = wr[p].astype(np.int64), wi[p].astype(np.int64)
        nyr = -yr if wide_neg else (-yr).astype(np.int16).astype(np.int64)
        tr = _wrap32(xr * yr + xi * yi).astype(np.int64) >> 15
        ti = _wrap32(xr * yi + xi * nyr).astype(np.int64) >> 15
        re[c:c + chunk] = _sat16(_wrap32(tr.sum(axis=1)))
        im[c:c + chunk] = _sat16(_wrap32(ti.sum(axis=1)))
    return re, im


def abs32(re, im):
    return _wrap32(re.astype(np.int64) ** 2 + im.astype(np.int64) ** 2)


def sync_time(rx, N_RB, wide_neg=False):
    """rx: [nb_rx] int32 frames of 10 samples_per_tti.  Returns peak_pos, source, peak_val (unsigned), corr int32
    [3][frame] (sync_corr_ue0..2: every fourth entry defined, the rest 0 here) and parts[(s, h, a)] = (re, im)."""
    N = SIZE[N_RB]
    rep = replicas(N_RB)
    ys = [np.ascontiguousarray(a, dtype=np.int32).view(np.int16).reshape(-1, 2) for a in rx]
    fl = len(ys[0])
    length = fl // 2
    pos = np.arange(0, length - N, 4)
    corr = np.zeros((3, fl), dtype=np.int32)
    metric = np.zeros((length // 4, 3), dtype=np.uint32)
    parts = {}
    for s in range(3):
        ab = []
        for h in range(2):
            sr = np.zeros(len(pos), dtype=np.int16)
            si = np.zeros(len(pos), dtype=np.int16)
            for a, y in enumerate(ys):
                re, im = dot_products(rep[s], y, pos + h * length, wide_neg)
                parts[(s, h, a)] = (re, im)
                sr = (sr.astype(np.int32) + re).astype(np.int16)          # the int16 += of :428-435 wraps
                si = (si.astype(np.int32) + im).astype(np.int16)
            ab.append(abs32(sr, si))
            corr[s, pos + h * length] = ab[h]
        metric[:len(pos), s] = ((ab[0].astype(np.int64) >> 1) + (ab[1].astype(np.int64) >> 1)).astype(np.int32).view(np.uint32)
    best = int(np.argmax(metric.ravel()))                  # the first maximum in the order n, then s
    return {"peak_pos": 4 * (best // 3), "source": best % 3, "peak_val": int(metric.ravel()[best]), "corr": corr,
            "parts": parts, "positions": pos}
