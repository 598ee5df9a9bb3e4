"""oai4g_tx_batch_rv / k_encode_rv: a redundancy version per transport block of a batch.

The configurations are those of tests/test_gpu_rm_paths.py that reach each placement path of
k_encode's phase 4 at the smallest size (one small block; E > Nnn, where the buffer repeats; K = 6144
with C > 1, both block halves and two codewords at Kmimo 2; 25 PRB), and one whose transport block
segments into K- and K+ blocks (Cminus > 0, checked with oai4g_lte_segmentation).  Ten consecutive
subframes carry rv[sf][cw] = (sf + 3 cw) & 3: every rv occurs, and the two codewords of a subframe
differ.

  - every transport block's e bits equal the oracle's for that block's rv, on the `once` path and,
    with OAI4G_ENC_GENERAL_RM set when the tables are derived, on the general path of every rv;
  - an all-equal rv array gives, for each rv, the e-bit words and the IQ of oai4g_tx_batch on a
    configuration created with that rvidx, byte for byte;
  - the mixed array's IQ equals, subframe by subframe, the IQ of the four configurations created
    with rvidx = (a, (a + 3) & 3);
  - without oai4g_tx_config_enable_tb_rv the calls return -1."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

N_SF = 10
MIX_TBS = 6208          # B = 6232 > 6144: C = 2, one block of K- = 3136 and one of K+ = 3200
CASES = {"C1": ("C1", {}),
         "C1-repeat": ("C1", dict(mcs=(0, 0))),                     # 6 PRB, MCS 0: E > Nnn
         "C3": ("C3", {}),
         "C2-25": ("C2", dict(N_RB_DL=25, rb_alloc=None, nb_rb=25, mcs=(4, 0))),
         "mixed-K": ("C2", dict(N_RB_DL=25, rb_alloc=None, nb_rb=25, mcs=(12, 0), TBS=(MIX_TBS, 0)))}


def _rv_mixed(n_cw):
    return np.array([[(sf + 3 * cw) & 3 for cw in range(n_cw)] for sf in range(N_SF)], np.uint8)


def _params(gpu, key, rv=(0, 0)):
    name, over = CASES[key]
    over = dict(over)
    if over.get("rb_alloc", 1) is None:
        over["rb_alloc"] = {25: gpu.FULL_ALLOC_25, 50: gpu.FULL_ALLOC_50}[over["N_RB_DL"]]
    if "mcs" in over and "TBS" not in over:
        over["TBS"] = tuple(gpu.tbs_bits(m, over.get("nb_rb", 6 if name == "C1" else 100)) for m in over["mcs"])
    p = gpu.make_params(name, subframe=0, subframe_step=1, **over)
    for cw in range(p.n_cw):
        p.rvidx[cw] = rv[cw]
    return p


def _payload(p, key):
    return np.random.default_rng(len(key) + 7).integers(0, 256, size=(N_SF, p.n_cw, p.payload_stride), dtype=np.uint8)


def _fixed(gpu, key, rv):
    """oai4g_tx_batch of the configuration created with rvidx = rv: (e-bit words, IQ)"""
    p = _params(gpu, key, rv)
    pipe = gpu.TxPipeline(p, N_SF)
    try:
        pipe.upload_payload(_payload(p, key))
        pipe.run()
        pipe.sync()
        return pipe.ebits(), pipe.iq()
    finally:
        pipe.close()


def _per_tb(gpu, key, rv, general=False):
    """oai4g_tx_batch_rv with the array rv: (e-bit words, IQ, G[sf][cw])"""
    p = _params(gpu, key)
    pipe = gpu.TxPipeline(p, N_SF)
    try:
        if general:
            os.environ["OAI4G_ENC_GENERAL_RM"] = "1"
        try:
            pipe.enable_tb_rv()
        finally:
            os.environ.pop("OAI4G_ENC_GENERAL_RM", None)
        pipe.upload_payload(_payload(p, key))
        pipe.run_rv(rv)
        pipe.sync()
        return pipe.ebits(), pipe.iq(), [[pipe.G(cw, sf) for cw in range(p.n_cw)] for sf in range(N_SF)]
    finally:
        pipe.close()


def test_mixed_case_has_both_block_sizes(gpu):
    vals = [ctypes.c_uint32(0) for _ in range(6)]
    assert gpu.lib().oai4g_lte_segmentation(None, None, MIX_TBS + 24, *[ctypes.byref(v) for v in vals]) == 0
    C, Cplus, Cminus, Kplus, Kminus, _ = (v.value for v in vals)
    assert C > 1 and Cminus > 0 and Cplus > 0 and Kminus < Kplus, (C, Cplus, Cminus, Kplus, Kminus)
    assert _params(gpu, "mixed-K").TBS[0] == MIX_TBS


@pytest.mark.parametrize("key", list(CASES))
def test_mixed_rv_ebits_equal_oracle_on_both_paths(gpu, key):
    p = _params(gpu, key)
    rv = _rv_mixed(p.n_cw)
    assert {int(v) for v in rv.ravel()} == {0, 1, 2, 3}
    if p.n_cw == 2:
        assert np.all(rv[:, 0] != rv[:, 1])
    pay = _payload(p, key)
    runs = [_per_tb(gpu, key, rv, general) for general in (False, True)]
    for sf in range(N_SF):
        po = _params(gpu, key, [int(v) for v in rv[sf]] + [0] * (2 - p.n_cw))
        _, _, e_o = O.tx_subframe(O.tx_cfg_from_params(po, sf), [pay[sf, cw] for cw in range(p.n_cw)], want_e=True)
        for cw in range(p.n_cw):
            for k, (eb, _, Gs) in enumerate(runs):
                G = Gs[sf][cw]
                assert np.array_equal(gpu.unpack_bits(eb[sf, cw], G), e_o[cw][:G]), (key, sf, cw, int(rv[sf, cw]),
                                                                                     "general" if k else "once")


@pytest.mark.parametrize("key", list(CASES))
def test_uniform_rv_equals_the_configuration_of_that_rvidx(gpu, key):
    n_cw = _params(gpu, key).n_cw
    for rv in range(4):
        eb_f, iq_f = _fixed(gpu, key, (rv, rv))
        eb, iq, Gs = _per_tb(gpu, key, np.full((N_SF, n_cw), rv, np.uint8))
        for sf in range(N_SF):
            for cw in range(n_cw):
                nw = (Gs[sf][cw] + 31) // 32     # the words the encoder writes (the last one masked to G)
                assert eb[sf, cw, :nw].tobytes() == eb_f[sf, cw, :nw].tobytes(), (key, rv, sf, cw)
        assert iq.tobytes() == iq_f.tobytes(), (key, rv)


def test_mixed_rv_iq_of_c3_equals_the_four_configurations(gpu):
    rv = _rv_mixed(2)
    _, iq, _ = _per_tb(gpu, "C3", rv)
    fixed = {a: _fixed(gpu, "C3", (a, (a + 3) & 3))[1] for a in range(4)}
    for sf in range(N_SF):
        a = int(rv[sf, 0])
        assert int(rv[sf, 1]) == (a + 3) & 3
        assert np.array_equal(iq[sf], fixed[a][sf]), sf


def test_rv_values_are_masked(gpu):
    """rv is used masked with 3: no value indexes outside the four tables"""
    rv = _rv_mixed(1)
    _, iq, _ = _per_tb(gpu, "C1", rv)
    _, iq_hi, _ = _per_tb(gpu, "C1", rv | 0xFC)
    assert iq.tobytes() == iq_hi.tobytes()


def test_enable_twice_returns_0_and_keeps_the_output(gpu):
    """the second oai4g_tx_config_enable_tb_rv finds the tables in place: 0 again, the same e bits and IQ"""
    p = _params(gpu, "C1")
    rv = _rv_mixed(1)
    pipe = gpu.TxPipeline(p, N_SF)
    try:
        pipe.upload_payload(_payload(p, "C1"))
        L = gpu.lib()
        out = []
        for _ in range(2):
            assert L.oai4g_tx_config_enable_tb_rv(pipe.cfg) == 0
            pipe.run_rv(rv)
            pipe.sync()
            out.append((pipe.ebits(), pipe.iq()))
        assert out[0][0].tobytes() == out[1][0].tobytes()
        assert out[0][1].tobytes() == out[1][1].tobytes()
    finally:
        pipe.close()
    assert _per_tb(gpu, "C1", rv)[1].tobytes() == out[1][1].tobytes()     # and that of a pipeline enabled once


def test_batch_rv_needs_enable(gpu):
    p = _params(gpu, "C1")
    pipe = gpu.TxPipeline(p, N_SF)
    try:
        pipe.upload_payload(_payload(p, "C1"))
        pipe.upload_rv(_rv_mixed(1))
        L = gpu.lib()
        assert L.oai4g_tx_batch_rv(pipe.cfg, N_SF, pipe.d_payload, pipe.d_rv, pipe.d_work, pipe.d_iq, None) == -1
        assert b"enable_tb_rv" in L.oai4g_last_error()
        assert L.oai4g_tx_encode_rv(pipe.cfg, N_SF, pipe.d_payload, pipe.d_rv, pipe.d_work, None) == -1
        pipe.enable_tb_rv()
        pipe.enable_tb_rv()          # idempotent
        assert L.oai4g_tx_batch_rv(pipe.cfg, N_SF, pipe.d_payload, pipe.d_rv, pipe.d_work, pipe.d_iq, None) == 0
        pipe.sync()
    finally:
        pipe.close()
