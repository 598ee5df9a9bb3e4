"""CPU suite: the fading channel's tables and the numpy restatement (tests/channel_model.py) against the fixture the
reference's own random_channel.c / multipath_channel.c wrote (tests/golden/channel_ref.json and .npz).

  - every supported model at 1x1, 1x2, 2x1 and 2x2, BW 1.25 / 5 / 20, forgetting factor 0 and 0.5: the descriptor's
    scalars and tables are equal, in the model and in the library's own host-side constructor
    (oai4g_channel_model_describe, which needs no device);
  - a and ch after a first and a second call on the scripted draws are within 1e-12 absolute.  The values are O(1),
    each a sum of at most 18 terms that carry a few ulp (2^-52) from sin / cos / sqrt, which differ between libms;
    three decades of margin still sit six decades under the smallest effect of a wrong tap, delay or index (1e-6);
  - EPA / EVA / ETU at 1x2 and 2x1, which the fixture leaves out (the reference's matrix is uninitialised off the
    diagonal there), use identity;
  - the model's convolution equals the reference's doubles bit for bit (digests)."""
import ctypes

import numpy as np
import pytest

import channel_cases as CC
import channel_model as M
import openair4g_amd as oai

TOL = 1e-12


@pytest.fixture(scope="module")
def ref():
    return CC.load_ref()


def _c(v):
    v = np.asarray(v, dtype=float)
    return v[..., 0] + 1j * v[..., 1]


def test_cases_cover_every_model_size_bandwidth_and_factor():
    seen = {(m, nt, nr) for m, nt, nr, _, _ in CC.DESC.values()}
    for m in CC.SUPPORTED:
        for nt, nr in CC.SIZES:
            assert ((m, nt, nr) in seen) != (m in CC.TAPPED and nt * nr == 2)
    for m in CC.SUPPORTED:
        assert {ff for mm, _, _, _, ff in CC.DESC.values() if mm == m} == set(CC.FFS)
    for m in CC.TAPPED + CC.EIGHT:
        assert {bw for mm, _, _, bw, _ in CC.DESC.values() if mm == m} == set(CC.BWS)
    assert {bw for _, _, _, bw, _ in CC.DESC.values()} == set(CC.BWS)


@pytest.mark.parametrize("name", list(CC.DESC))
def test_descriptor_tables_equal_the_reference(ref, name):
    model, nt, nr, bw, _ = CC.DESC[name]
    r, d = ref["desc"][name], M.describe(model, nt, nr, bw)
    assert (d.nb_taps, d.channel_length, d.ricean_factor, d.aoa, d.random_aoa) == \
        (r["nb_taps"], r["channel_length"], r["ricean_factor"], r["aoa"], r["random_aoa"])
    assert d.amps.tolist() == r["amps"] and d.delays.tolist() == r["delays"]
    for i, m in enumerate(r["R_sqrt"]):
        assert np.array_equal(d.R_sqrt[i], _c(m)), (name, i)
    info, rs = oai.channel_model_describe(CC.MODELS[model], nt, nr, bw)
    assert (info.nb_taps, info.channel_length, info.ricean_factor, info.aoa, info.random_aoa) == \
        (r["nb_taps"], r["channel_length"], r["ricean_factor"], r["aoa"], r["random_aoa"])
    assert list(info.amps)[:info.nb_taps] == r["amps"] and list(info.delays)[:info.nb_taps] == r["delays"]
    assert info.n_matrices >= len(r["R_sqrt"])
    for i, m in enumerate(r["R_sqrt"]):
        assert np.array_equal(rs[i], _c(m)), (name, i)


@pytest.mark.parametrize("name", list(CC.DESC))
def test_model_taps_match_the_reference(ref, name):
    model, nt, nr, bw, ff = CC.DESC[name]
    r, d = ref["desc"][name], M.describe(model, nt, nr, bw)
    count = CC.n_draws(d.nb_taps, nt, nr, d.ricean_factor, d.random_aoa)
    a = None
    for call in (0, 1):
        seq = CC.draws(name, call, count, nt * nr if count > 2 * d.nb_taps * nt * nr else 0)
        a, ch = M.random_channel(d, a, seq, ff, call == 0)
        ea, ech = np.abs(a - _c(r[f"a{call}"])).max(), np.abs(ch - _c(r[f"ch{call}"])).max()
        assert ea <= TOL and ech <= TOL, (name, call, ea, ech)


@pytest.mark.parametrize("model", CC.TAPPED)
@pytest.mark.parametrize("size", [(1, 2), (2, 1)])
def test_identity_where_the_reference_matrix_is_undefined(model, size):
    d = M.describe(model, size[0], size[1], 5.0)
    assert all(np.array_equal(m, np.eye(2)) for m in d.R_sqrt)
    info, rs = oai.channel_model_describe(CC.MODELS[model], size[0], size[1], 5.0)
    assert all(np.array_equal(rs[i], np.eye(2)) for i in range(info.n_matrices))


@pytest.mark.parametrize("model,nt,nr", [("SCM_A", 1, 1), ("SCM_B", 1, 1), ("SCM_C", 2, 2), ("SCM_D", 1, 1), ("custom", 1, 1),
                                         ("MBSFN", 1, 1), ("EPA", 3, 1), ("EPA", 1, 3), ("EPA", 0, 1)])
def test_refused_models_and_antennas(model, nt, nr):
    with pytest.raises(oai.OAI4GError) as e:
        oai.channel_model_describe(CC.MODELS[model], nt, nr, 5.0)
    assert "channel" in str(e.value)


def test_channel_length_beyond_the_descriptor_field_is_refused():
    with pytest.raises(oai.OAI4GError):
        oai.channel_model_describe(CC.MODELS["ETU"], 1, 1, 30.72)     # 308 taps: the reference's uint8_t would wrap


@pytest.mark.parametrize("name", list(CC.CONV))
def test_model_convolution_equals_the_reference_bit_for_bit(ref, name):
    model, nt, nr, bw, off, length = CC.CONV[name]
    r = ref["conv"][name]
    clen = M.describe(model, nt, nr, bw).channel_length
    assert clen == r["channel_length"]
    ch, dd = CC.conv_taps(name, clen), abs(off)
    for kind in CC.CONV_INPUTS:
        rx = M.multipath(ch, CC.conv_input(name, kind, clen).astype(np.float64), nr, off)
        assert np.isnan(rx[:, :dd]).all()
        got = [[CC.digest(rx[a, dd:, 0]), CC.digest(rx[a, dd:, 1])] for a in range(nr)]
        assert got == r[kind], (name, kind)


def test_channel_symbols_are_bound():
    for s in ("oai4g_channel_config_create", "oai4g_channel_random_batch", "oai4g_multipath_batch",
              "oai4g_random_channel", "oai4g_multipath_channel", "oai4g_channel_set_taps", "oai4g_channel_get_taps"):
        assert s in oai.exported_symbols()
    assert ctypes.sizeof(oai.ChannelInfo) == 32 + 16 * oai.CHANNEL_MAX_TAPS
