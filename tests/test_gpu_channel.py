"""GPU suite of the fading channel (oai4g_channel_random_batch / oai4g_multipath_batch, k_channel_taps / k_multipath)
against the reference's own execution (tests/golden/channel_ref.json and .npz through tests/channel_model.py, which
test_channel_cpu.py pins to it) and against oai4g_awgn_batch:

  G1  model AWGN 1x1 equals oai4g_awgn_batch bit for bit;
  G2  supplied draws: a and ch equal the fixture within 1e-12 (the bound test_channel_cpu.py derives), first and second
      call, every descriptor case; set_taps -> get_taps is the identity;
  G3  the convolution's doubles equal the reference's bit for bit (drop-in, keep_channel = 1), and the batch form at
      offset_db = -400 (noise under 2^-60) is (short) of them, in segments;
  G4  the Philox draws: tap powers, independence of the launch split, steps, the (anti-)correlated pairs, the Rice mean;
  G5  refusals;
  G6  the TM2 receive loop with the antenna mix on the device."""

import numpy as np
import pytest

import channel_cases as CC
import channel_model as M

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope="module")
def ref():
    return CC.load_ref()


def _c(v):
    v = np.asarray(v, dtype=float)
    return v[..., 0] + 1j * v[..., 1]


def _words(x16):
    """int16 [..., 2] -> packed int32 [...]"""
    return np.ascontiguousarray(x16.astype(np.int16)).view(np.int32)[..., 0]


class Mem:
    """device buffers of one test, freed together"""

    def __init__(self, gpu):
        self.gpu, self.L, self.p = gpu, gpu.lib(), []

    def put(self, a):
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes)
        assert self.L.oai4g_memcpy_h2d(d, self.gpu._ptr(a), a.nbytes) == 0
        return d

    def alloc(self, nbytes):
        d = self.L.oai4g_dev_alloc(nbytes)
        assert d
        self.p.append(d)
        return d

    def get(self, d, shape, dtype):
        out = np.empty(shape, dtype)
        assert self.L.oai4g_sync() == 0
        assert self.L.oai4g_memcpy_d2h(self.gpu._ptr(out), d, out.nbytes) == 0
        return out

    def close(self):
        self.L.oai4g_sync()
        for d in self.p:
            self.L.oai4g_dev_free(d)


@pytest.mark.parametrize("tx_len,tail_len", [(1920, 1920), (1920, 0), (1919, 5)])
def test_g1_awgn_model_equals_awgn_batch(gpu, tx_len, tail_len):
    """6 PRB, 8 vectors; the last shape is odd, so the kernel stores sample by sample"""
    L, n, ln = gpu.lib(), 8, tx_len + tail_len
    rng = np.random.default_rng(11)
    m = Mem(gpu)
    d_x = m.put(_words(rng.integers(-500, 500, (n, tx_len, 2))))
    d_t = m.put(_words(rng.integers(-500, 500, (max(tail_len, 1), 2))))
    d_l = m.put(np.array([1000, 40000, 250000, 7, 1, 123456, 900, 5000], np.int32))
    d_r, d_q = m.alloc(n * ln * 4), m.alloc(n * ln * 4)
    assert L.oai4g_awgn_batch(d_x, tx_len, tx_len, d_t, tail_len, d_r, ln, n, d_l, -3.0, 99, 5, None) == 0
    with gpu.ChannelBatch(1, 1, gpu.AWGN, 1.25, n) as ch:
        ch.draw(seed=3)
        a, taps = ch.taps()
        assert np.all(a == 1.0) and np.all(taps == 1.0)
        ch.run(d_x, tx_len, 0, tx_len, d_t, tail_len, d_q, ln, 0, ln, 0, d_l, -3.0, 99, first_vector=5)
        want, got = m.get(d_r, (n, ln), np.int32), m.get(d_q, (n, ln), np.int32)
    m.close()
    assert np.array_equal(got, want)
    assert len(np.unique(got[1])) > ln // 2                  # noise was added, not a constant written


def _desc_cases(model):
    return [k for k, v in CC.DESC.items() if v[0] == model]


@pytest.mark.parametrize("model", CC.SUPPORTED)
def test_g2_supplied_draws_match_the_reference(gpu, ref, model):
    for name in _desc_cases(model):
        _, nt, nr, bw, ff = CC.DESC[name]
        r = ref["desc"][name]
        with gpu.ChannelBatch(nt, nr, CC.MODELS[model], bw, 3, forgetting_factor=ff) as ch:
            assert (ch.nb_taps, ch.channel_length) == (r["nb_taps"], r["channel_length"])
            assert ch.draws_per_vector == CC.n_draws(ch.nb_taps, nt, nr, ch.info.ricean_factor, ch.info.random_aoa)
            angles = nt * nr if ch.draws_per_vector > 2 * ch.nb_taps * nt * nr else 0
            for call in (0, 1):
                seq = CC.draws(name, call, ch.draws_per_vector, angles)
                ch.draw(n=2, draws=np.stack([seq, seq]))
                a, taps = ch.taps()
                for v in (0, 1):
                    ea, ec = np.abs(a[v] - _c(r[f"a{call}"])).max(), np.abs(taps[v] - _c(r[f"ch{call}"])).max()
                    assert ea <= TOL and ec <= TOL, (name, call, v, ea, ec)
                assert not a[2].any() and not taps[2].any()              # vector 2 was not drawn
            rng = np.random.default_rng(5)
            sa = rng.standard_normal(a.shape) + 1j * rng.standard_normal(a.shape)
            sc = rng.standard_normal(taps.shape) + 1j * rng.standard_normal(taps.shape)
            ch.set_taps(ch=sc[1:], a=sa[1:], first_vector=1)
            ga, gc = ch.taps()
            assert np.array_equal(ga[1:], sa[1:]) and np.array_equal(gc[1:], sc[1:])
            assert np.array_equal(ga[0], a[0]) and np.array_equal(gc[0], taps[0])


@pytest.fixture(scope="module")
def conv_expected():
    """per convolution case and input the model's doubles [nb_rx][length][2] (NaN where the reference does not write),
    computed once"""
    out = {}

    def get(name, kind):
        if (name, kind) not in out:
            model, nt, nr, bw, off, length = CC.CONV[name]
            clen = M.describe(model, nt, nr, bw).channel_length
            out[(name, kind)] = M.multipath(CC.conv_taps(name, clen), CC.conv_input(name, kind, clen).astype(np.float64), nr,
                                            off)
        return out[(name, kind)]
    return get


@pytest.mark.parametrize("name", list(CC.CONV))
def test_g3_convolution_doubles_equal_the_reference(gpu, ref, conv_expected, name):
    model, nt, nr, bw, off, length = CC.CONV[name]
    r, dd = ref["conv"][name], abs(off)
    with gpu.ChannelBatch(nt, nr, CC.MODELS[model], bw, 1, channel_offset=off) as ch:
        assert ch.channel_length == r["channel_length"]
        ch.set_taps(ch=CC.conv_taps(name, ch.channel_length)[None])
        for kind in CC.CONV_INPUTS:
            x = CC.conv_input(name, kind, ch.channel_length).astype(np.float64)
            keep = -7.5
            rr, ri = np.full((nr, length), keep), np.full((nr, length), keep)
            re, im = gpu.multipath_channel(ch, x[:, :, 0], x[:, :, 1], length, 1, rx_re=list(rr), rx_im=list(ri))
            assert np.all(re[:, :dd] == keep) and np.all(im[:, :dd] == keep)         # left untouched
            got = [[CC.digest(re[a, dd:]), CC.digest(im[a, dd:])] for a in range(nr)]
            assert got == r[kind], (name, kind)
            want = conv_expected(name, kind)
            assert np.array_equal(re[:, dd:], want[:, dd:, 0]) and np.array_equal(im[:, dd:], want[:, dd:, 1])


@pytest.mark.parametrize("name", list(CC.CONV))
def test_g3_batch_form_is_short_of_the_doubles_in_segments(gpu, conv_expected, name):
    """two vectors (the random and the impulse input) through the int16 form at offset_db = -400, written in
    FepBatch's [2 vector + segment][nb_rx][seg_len] layout where the length is even"""
    model, nt, nr, bw, off, length = CC.CONV[name]
    dd = abs(off)
    seg = length // 2 if length % 2 == 0 else length
    nseg = length // seg
    m = Mem(gpu)
    with gpu.ChannelBatch(nt, nr, CC.MODELS[model], bw, 2, channel_offset=off) as ch:
        taps = CC.conv_taps(name, ch.channel_length)
        ch.set_taps(ch=np.stack([taps, taps]))
        x = np.stack([CC.conv_input(name, k, ch.channel_length) for k in CC.CONV_INPUTS])     # [2][nt][length][2]
        head = length - 1000
        d_x, d_tail = m.put(_words(x[:, :, :head])), m.put(_words(x[1, :, head:]))
        x[0, :, head:] = x[1, :, head:]                      # the tail is common to the vectors
        d_l = m.put(np.full((2, nt), 1000, np.int32))
        d_r = m.alloc(2 * nseg * nr * seg * 4)
        assert m.L.oai4g_memset_d(d_r, 0x5A, 2 * nseg * nr * seg * 4) == 0
        ch.run(d_x, nt * head, head, head, d_tail, 1000, d_r, nseg * nr * seg, seg, seg, nr * seg, d_l, -400.0, 1)
        got = m.get(d_r, (2, nseg, nr, seg), np.int32)
    m.close()
    clen = taps.shape[1]
    for v in range(2):
        want = conv_expected(name, CC.CONV_INPUTS[v]) if v == 1 else \
            M.multipath(taps, x[0].astype(np.float64), nr, off)
        w16 = M.to_short(np.nan_to_num(want, nan=0.0))       # the unwritten head is 0 here
        assert not w16[:, :dd].any()
        g = got[v].transpose(1, 0, 2).reshape(nr, length)
        assert np.array_equal(g, _words(w16)), (name, v, clen)


def test_g4_philox_draws(gpu):
    n = 4096
    with gpu.ChannelBatch(1, 1, gpu.Rayleigh8, 5.0, n) as ch, gpu.ChannelBatch(1, 1, gpu.Rayleigh8, 5.0, n) as part:
        ch.draw(seed=77, first_vector=0, step=0)
        a, taps = ch.taps()
        amps = np.array(list(ch.info.amps)[:8])
        p = (np.abs(a[:, :, 0]) ** 2).mean(axis=0)
        print("tap powers / amps:", (p / amps).round(4).tolist())
        assert np.all(np.abs(p / amps - 1) <= 5 / np.sqrt(n))
        # ch is the interpolation of a
        d = M.describe("Rayleigh8", 1, 1, 5.0)
        assert np.abs(taps[17] - M.interpolate(d, a[17])).max() <= TOL
        part.draw(seed=77, first_vector=1024, step=0, n=1024)
        assert np.array_equal(part.taps(0, 1024)[0], a[1024:2048])
        part.draw(seed=77, first_vector=1024, step=1, n=1024)          # a second call of those vectors: ff = 0
        b = part.taps(0, 1024)[0]
        assert not np.any(b == a[1024:2048])
    for model, sign in ((gpu.Rayleigh1_corr, 1.0), (gpu.Rayleigh1_anticorr, -1.0)):
        with gpu.ChannelBatch(2, 1, model, 5.0, n) as ch:
            ch.draw(seed=5)
            a = ch.taps()[0]
            assert np.array_equal(a[:, 0, 1], sign * a[:, 0, 0]) and np.abs(a[:, 0, 0]).min() > 0
    with gpu.ChannelBatch(1, 1, gpu.Rice1, 5.0, n) as ch:
        ch.draw(seed=6)
        a = ch.taps()[0][:, 0, 0]
        sigma = np.sqrt(0.1 / 2) / np.sqrt(n)
        print("Rice1 mean:", a.mean(), "expected", np.sqrt(0.9))
        assert abs(a.real.mean() - np.sqrt(0.9)) <= 5 * sigma and abs(a.imag.mean()) <= 5 * sigma


def test_g5_refusals(gpu):
    L = gpu.lib()
    for model, nt, nr in ((1, 1, 1), (2, 1, 1), (3, 2, 2), (4, 1, 1), (gpu.EPA, 3, 1), (gpu.EPA, 1, 3)):
        assert not L.oai4g_channel_config_create(nt, nr, model, 5.0, 0.0, 0, 0.0, 4)
        assert b"channel" in L.oai4g_last_error()
    with gpu.ChannelBatch(1, 1, gpu.Rayleigh1, 5.0, 4) as ch:
        ch.set_taps(ch=np.full((4, 1, 1), 2.0), a=np.full((4, 1, 1), 2.0))
        m = Mem(gpu)
        d_x, d_l, d_r = m.put(np.zeros((5, 64), np.int32)), m.put(np.ones(5, np.int32)), m.alloc(5 * 64 * 4)
        assert L.oai4g_channel_random_batch(ch.cfg, 5, 1, 0, 0, None, None) == -1
        assert b"5 vectors" in L.oai4g_last_error()
        assert L.oai4g_multipath_batch(ch.cfg, 5, d_x, 64, 0, 64, None, 0, d_r, 64, 0, 64, 0, d_l, 0.0, 1, 0, None) == -1
        assert b"5 vectors" in L.oai4g_last_error()
        assert L.oai4g_channel_set_taps(ch.cfg, 2, 3, None, None) == -1
        a, taps = ch.taps()
        assert np.all(a == 2.0) and np.all(taps == 2.0)       # nothing ran
        m.close()


def test_g6_tm2_receive_loop_on_the_device(gpu):
    """test_gpu_tm2_receive_loop's chain at 25 PRB, 2x2, with the antenna mix on the device: a fixed single-tap H per
    subframe through ChannelBatch at offset_db = -400, the IQ never leaving the device"""
    import oracle_lib as O
    from test_rx_cpu import decode_tb, dual_alloc
    from test_rx_tm2_cpu import qm_of, tm2_params
    N_RB, mcs, npd, sf, nb_rx = 25, 12, 1, 7, 2       # test_rx_tm2_cpu.py's 25 PRB case
    ra = dual_alloc(N_RB, dc=False)                       # odd N_RB_DL: the allocation the dual extraction defines
    n_tx, n_sf = 3, 2
    p = tm2_params(N_RB, mcs, npd, sf)
    p.subframe_step = 1
    pipe = gpu.TxPipeline(p, n_tx)
    rng = np.random.default_rng(mcs + N_RB)
    pay = rng.integers(0, 256, size=(n_tx, 1, p.payload_stride), dtype=np.uint8)
    pipe.upload_payload(pay)
    pipe.run()
    fg = gpu.frame_parms(N_RB, nb_antennas_tx=2, mode1_flag=0)
    spt = fg.samples_per_tti
    fep = gpu.FepBatch(fg, n_tx, nb_rx)
    m = Mem(gpu)
    d_lev = m.alloc(n_tx * 2 * 4)
    assert m.L.oai4g_signal_energy_batch(pipe.d_iq, n_tx * 2, spt, spt, d_lev, None) == 0
    H = np.array([[0.6, 0.3j], [-0.3, 0.5 + 0.2j]])          # [rx][tx]
    with gpu.ChannelBatch(2, 2, gpu.Rayleigh1, 5.0, n_tx) as ch:
        taps = np.array([H[a, t] for t in range(2) for a in range(2)]).reshape(1, 4, 1)       # pair aarx + 2 aatx
        ch.set_taps(ch=np.repeat(taps, n_tx, axis=0))
        ch.run(pipe.d_iq, 2 * spt, spt, spt, None, 0, fep.d_rx, 2 * spt, spt, spt, 0, d_lev, -400.0, 1)
        fep.run()
        rx_iq = m.get(fep.d_rx, (n_tx, nb_rx, spt), np.int32)
    m.close()
    t16 = pipe.iq().view(np.int16).reshape(n_tx, 2, spt, 2).astype(np.float64)
    tc = t16[..., 0] + 1j * t16[..., 1]
    mix = np.einsum("at,ntk->nak", H, tc)
    got = rx_iq.view(np.int16).reshape(n_tx, nb_rx, spt, 2)
    assert np.abs(got[..., 0] - mix.real).max() < 1.0 + 1e-9 and np.abs(got[..., 1] - mix.imag).max() < 1.0 + 1e-9
    Qm = qm_of(mcs)
    rx = gpu.RxBatchTM2(fg, ra, Qm, npd, p.rnti, n_sf, nb_rx=nb_rx, first_subframe=sf)
    rx.estimate(fep.d_rxF, first_subframe=sf)
    rx.launch(fep.d_rxF, unscramble=1)
    llr = rx.llrs()
    rxF = fep.result()
    fo = O.frame(N_RB, nb_antennas_tx=2, mode1_flag=0)
    for i in range(n_sf):
        s_ = (sf + i) % 10
        est = {(pp, a): O.chest_subframe(fo, rxF[i, a].ravel(), rxF[i + 1, a, 0], s_, p=pp) for pp in (0, 1)
               for a in range(nb_rx)}
        lo, _ = O.rx_pdsch_tm2(fo, [rxF[i, a].ravel() for a in range(nb_rx)], est, ra, Qm, npd, s_)
        G = rx.llr_count(s_)
        u = np.zeros(32 * (1 + G // 32), np.int16)
        u[:G] = lo
        O.dlsch_unscrambling(u, G, (p.rnti << 14) + (s_ << 9) + fo.Nid_cell)
        assert len(lo) == G and np.array_equal(llr[i, :G], u[:G]), s_
        res, tb = decode_tb(llr[i, :G], G, p.TBS[0], Qm)
        assert all(it <= 4 for it, _ in res), (s_, [it for it, _ in res])
        assert np.array_equal(tb, pay[i, 0, :p.TBS[0] // 8]), s_
    rx.close()
    fep.close()
    pipe.close()
