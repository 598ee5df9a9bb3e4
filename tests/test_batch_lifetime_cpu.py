"""CPU suite: the lifetime rule of the device-resident classes (openair4g_amd._DeviceOwner).

A pure-Python stand-in takes the place of the library behind openair4g_amd.init / openair4g_amd.lib.  It hands
out fake device addresses and configuration handles, keeps the set of live ones and the order of the calls, can
be told to fail the k-th acquisition (an allocation or a *_create), and makes the free or destroy of something
that is not live a test failure.  Host-only entry points (frame parameters, TBS tables, CCE counts) fall through
to the real library; every launch answers 0 and every size getter a small number.  The failure paths can only
be exercised here: a real allocation is never made to fail on a device, and a second close() is never made there.
"""
import ctypes
import gc

import numpy as np
import pytest

import openair4g_amd as oai
from openair4g_amd import dlsim

HOST_ONLY = {"oai4g_init_frame_parms", "oai4g_get_TBS_DL", "oai4g_get_Qm", "oai4g_init_nCCE_table", "oai4g_get_nCCE",
             "oai4g_get_nCCE_offset"}
GETTERS = {"oai4g_rx_llr_stride", "oai4g_rx_llr_count", "oai4g_td_scratch_bytes", "oai4g_td8_scratch_bytes",
           "oai4g_ul_config_C", "oai4g_ul_config_E", "oai4g_ul_config_G_offset", "oai4g_ul_config_w_entries",
           "oai4g_tx_G", "oai4g_tx_ebits_words", "oai4g_tx_iq_samples", "oai4g_tx_workspace_bytes"}
CREATE = {n for n in oai.exported_symbols() if "_config_create" in n} | {"oai4g_new_dlsch"}
DESTROY = {n for n in oai.exported_symbols() if n.endswith("_config_destroy")} | {"oai4g_free_dlsch"}


def _key(h):
    return h if isinstance(h, int) else ctypes.addressof(h.contents)


class FakeLib:
    def __init__(self, real):
        self.real = real
        self.live = {}                  # address or handle -> "buf" / "cfg"
        self.log = []                   # (call name, its first argument's key or None), device-side calls only
        self.errors = []                # frees and destroys of something not live
        self.n_acq, self.fail_at = 0, 0  # acquisitions so far; the one to fail (0: none)
        self.fail_calls = set()         # launches that answer -1
        self._next = 0x7F0000000000
        self._keep = []

    def _acquire(self, kind, name):
        self.n_acq += 1
        if self.n_acq == self.fail_at:
            return None
        self._next += 1 << 32
        h = self._next
        if name == "oai4g_new_dlsch":   # DlschHandle reads the structure: a real one on the host
            harq, d = oai.DlHarq(), oai.Dlsch()
            d.harq_processes[0] = ctypes.pointer(harq)
            self._keep.append((harq, d))
            h = ctypes.pointer(d)
        self.live[_key(h)] = kind
        return h

    def _release(self, kind, name, h):
        if self.live.pop(_key(h), None) != kind:
            self.errors.append(f"{name} of {h!r}, which is not a live {kind}")

    def __getattr__(self, name):
        if name in HOST_ONLY:
            return getattr(self.real, name)
        if name not in oai._SIGS:
            raise AttributeError(name)

        def call(*args):
            self.log.append((name, _key(args[0]) if args and isinstance(args[0], (int, ctypes._Pointer)) else None))
            if name == "oai4g_dev_alloc":
                return self._acquire("buf", name)
            if name in CREATE:
                return self._acquire("cfg", name)
            if name == "oai4g_dev_free":
                return self._release("buf", name, args[0])
            if name in DESTROY:
                return self._release("cfg", name, args[0])
            if name == "oai4g_last_error":
                return b"stand-in failure"
            if name in GETTERS:
                return 64
            return -1 if name in self.fail_calls else 0
        return call


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib(oai.load_library())
    for mod in (oai, dlsim):
        monkeypatch.setattr(mod, "init", lambda: f)
        monkeypatch.setattr(mod, "lib", lambda: f)
    yield f
    gc.collect()
    assert not f.errors, f.errors


PLAN = [(1, 2, 27, 4, 1, 1, 1, 0)]
RA6 = [0x3F, 0, 0, 0]


def _fp(ntx=1):
    return oai.frame_parms(6, nb_antennas_tx=ntx, mode1_flag=1 if ntx == 1 else 0)


def _lazy_dual(o):
    o._pil()
    o._llr1()
    for _ in range(2):
        o.estimate(0x1000)
        o.estimate_pilots(0x1000)
    o.estimate(0x1000, first_subframe=5)


def _lazy_ul(o):
    o._alloc_w()
    o.launch_harq(0, 1)
    for _ in range(2):
        o.launch_harq_tb([0, 1], [1, 0])


def _lazy_est(o):
    for _ in range(3):
        o.estimate(0x1000)


# name -> (constructor, what runs the lazy paths or None)
CASES = {
    "RxBatchTM3": (lambda: oai.RxBatchTM3(_fp(2), RA6, 2, 2, 4, 1, 0x1234, 2), _lazy_dual),
    "RxBatchTM2": (lambda: oai.RxBatchTM2(_fp(2), RA6, 2, 1, 0x1234, 2), _lazy_dual),
    "RxBatchTM56": (lambda: oai.RxBatchTM56(_fp(2), RA6, 2, 5, 0, 1, 0x1234, 2), _lazy_dual),
    "ChestBatch": (lambda: oai.ChestBatch(_fp(), 2), lambda o: (o.time_estimates(), o.freq_offset_omegas(0))),
    "RxBatch": (lambda: oai.RxBatch(_fp(), RA6, 2, 1, 0x1234, 2), None),
    "FepBatch": (lambda: oai.FepBatch(_fp(), 2, 1), None),
    "PbchDecodeBatch": (lambda: oai.PbchDecodeBatch(_fp(), 2), None),
    "PdcchRxBatch": (lambda: oai.PdcchRxBatch(_fp(), 1, 0x1234, 0xFFFF, 2, PLAN, 2), None),
    "PdcchFrontBatch": (lambda: oai.PdcchFrontBatch(_fp(2), 2, 2, oai.ALAMOUTI), _lazy_est),
    "PdcchRxBatchDetected": (lambda: oai.PdcchRxBatchDetected(_fp(), 0x1234, 0xFFFF, 2, PLAN, 2), None),
    "PbchFrontBatch": (lambda: oai.PbchFrontBatch(_fp(2), 2, 2, 2), _lazy_est),
    "PhichRxBatch": (lambda: oai.PhichRxBatch(_fp(), [(0, 0, 0), (1, 0, 1)]), None),
    "TurboDecoder8Batch": (lambda: oai.TurboDecoder8Batch(512, 8), None),
    "TurboDecoderBatch": (lambda: oai.TurboDecoderBatch(40, 8), None),
    "UlDecodeBatch": (lambda: oai.UlDecodeBatch(1024, 2048, 2, 2), _lazy_ul),
    "DlschHandle": (lambda: oai.DlschHandle(N_RB_DL=6), None),
    "TxPipeline": (lambda: oai.TxPipeline(oai.make_params("C1"), 2), lambda o: o.upload_rv([[0], [1]])),
    "TxPipeline(alloc=False)": (lambda: oai.TxPipeline(oai.make_params("C1"), 2, alloc=False), None),
    "DlsimBler": (lambda: dlsim.DlsimBler(4, N_RB_DL=6, batch=2), None),
    "DlsimBler(num_rounds=2)": (lambda: dlsim.DlsimBler(4, N_RB_DL=6, batch=2, num_rounds=2), None),
}


def test_every_device_resident_class_has_a_case():
    """none left out: every subclass of the owner in the two modules, but its private helpers"""
    def subclasses(c):
        return {s for d in c.__subclasses__() for s in {d} | subclasses(d)}
    public = {c.__name__ for c in subclasses(oai._DeviceOwner) if not c.__name__.startswith("_")}
    assert public == {n.split("(")[0] for n in CASES}
    for mod in (oai, dlsim):
        for name, c in vars(mod).items():
            if isinstance(c, type) and c is not oai._DeviceOwner:
                assert "__del__" not in vars(c), name
                assert "close" not in vars(c) or name == "DlschHandle", name


def _owned_attrs(o):
    kids = [v for v in vars(o).values() if isinstance(v, oai._DeviceOwner)]
    kids += [b for b in getattr(o, "by_count", [])]
    return [(k, v) for x in [o] + kids for k, v in vars(x).items() if k in ("cfg", "ptr") or k.startswith("d_")]


def _check_closed(fake, o, acquired):
    """after the first close(): nothing live, one synchronisation first, handles before buffers, each newest first"""
    assert not fake.live
    names = [n for n, _ in fake.log]
    assert names.count("oai4g_sync") == 1 and names[0] == "oai4g_sync"
    assert not (set(names[1:]) - DESTROY - {"oai4g_dev_free"})
    kinds = ["cfg" if n in DESTROY else "buf" for n in names[1:]]
    assert kinds == sorted(kinds, reverse=True)             # every configuration before the first buffer
    for kind in ("cfg", "buf"):
        assert [h for (n, h), k in zip(fake.log[1:], kinds) if k == kind] == \
            [h for h, k in reversed(acquired) if k == kind]
    attrs = _owned_attrs(o)
    assert attrs and all(v is None for _, v in attrs), attrs
    fake.log.clear()
    o.close()                                               # the second close makes no call at all
    assert fake.log == [] and not fake.errors


@pytest.mark.parametrize("name", list(CASES))
def test_close_releases_in_order_and_once(fake, name):
    make = CASES[name][0]
    o = make()
    acquired = list(fake.live.items())                      # in order of acquisition
    assert acquired and any(v is not None for _, v in _owned_attrs(o))
    fake.log.clear()
    o.close()
    _check_closed(fake, o, acquired)

    with make() as o:                                       # the with form leaves the same state
        acquired = list(fake.live.items())
        fake.log.clear()
    _check_closed(fake, o, acquired)


@pytest.mark.parametrize("name", list(CASES))
def test_a_failing_constructor_releases_what_it_acquired(fake, name):
    make = CASES[name][0]
    make().close()
    n = fake.n_acq
    assert n >= 1
    for k in range(1, n + 1):
        fake.n_acq, fake.fail_at = 0, k
        with pytest.raises(oai.OAI4GError):
            make()
        gc.collect()
        assert not fake.live, (k, fake.live)
        assert fake.n_acq == k                              # it stopped at the failure
    assert not fake.errors


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[1]])
def test_lazily_acquired_buffers_and_configurations_are_released(fake, name):
    make, lazy = CASES[name]
    o = make()
    before = len(fake.live)
    lazy(o)
    if name != "ChestBatch":                                # its temporaries are gone when the call returns
        assert len(fake.live) > before
    else:
        assert len(fake.live) == before
    fake.log.clear()
    o.close()
    assert not fake.live and not fake.errors
    names = [n for n, _ in fake.log]
    assert names.count("oai4g_sync") == 1 and names[0] == "oai4g_sync"
    kinds = ["cfg" if n in DESTROY else "buf" for n in names[1:]]
    assert kinds == sorted(kinds, reverse=True)
    assert all(v is None for _, v in _owned_attrs(o))
    fake.log.clear()
    o.close()
    assert fake.log == []


def test_dlsim_round_loop_buffers_are_released(fake):
    """num_rounds = 2 allocates the round state and, in its decoder child, the soft buffers"""
    one = dlsim.DlsimBler(4, N_RB_DL=6, batch=2)
    n_one = len(fake.live)
    assert one.d_state is None and one.dec.d_w is None
    one.close()
    with dlsim.DlsimBler(4, N_RB_DL=6, batch=2, num_rounds=2) as sim:
        assert len(fake.live) == n_one + 2 and sim.d_state and sim.dec.d_w
        sim.reset_rounds(1)
        assert sim.d_rv == sim.d_state + 2 and type(sim.d_state) is int
    assert not fake.live
    assert sim.d_state is None and sim.d_rv is None and sim.dec.d_w is None and sim.tx.cfg is None


@pytest.mark.parametrize("name,ports,keys", [("RxBatchTM2", 2, 2), ("PdcchFrontBatch", 2, 1), ("PbchFrontBatch", 2, 1)])
def test_estimate_planes_create_each_chest_configuration_once(fake, name, ports, keys):
    make, lazy = CASES[name]
    o = make()
    fake.log.clear()
    lazy(o)                                                 # repeated estimate() calls (two subframe keys: _lazy_dual)
    created = [n for n, _ in fake.log].count("oai4g_chest_config_create")
    assert created == ports * keys
    batches = [n for n, _ in fake.log if n.startswith("oai4g_chest_batch")]
    assert len(batches) % (ports * o.nb_rx) == 0 and batches
    fake.log.clear()
    o.close()
    destroyed = [h for n, h in fake.log if n == "oai4g_chest_config_destroy"]
    assert len(destroyed) == created and len(set(destroyed)) == created


def test_estimate_planes_are_one_implementation():
    for c in (oai._RxBatchDual, oai.PdcchFrontBatch, oai.PbchFrontBatch):
        assert issubclass(c, oai._EstPlanes)
        for m in ("est_plane", "upload_estimates", "_chest_cfgs", "_estimate"):
            assert m not in vars(c), (c.__name__, m)
    assert oai.TurboDecoder8Batch.run is oai.TurboDecoderBatch.run
    assert oai.TurboDecoder8Batch.__init__ is oai.TurboDecoderBatch.__init__


@pytest.mark.parametrize("method,entry", [("time_estimates", "oai4g_chest_time_batch"),
                                          ("freq_offset_omegas", "oai4g_freq_offset_omega_batch")])
def test_chest_temporaries_are_freed_when_the_call_raises(fake, method, entry):
    cb = oai.ChestBatch(_fp(), 2)
    before = dict(fake.live)
    fake.fail_calls.add(entry)
    with pytest.raises(oai.OAI4GError):
        getattr(cb, method)(*([0] if method == "freq_offset_omegas" else []))
    assert fake.live == before
    fake.fail_at = fake.n_acq + 1                           # and when the temporary itself cannot be had
    with pytest.raises(oai.OAI4GError):
        getattr(cb, method)(*([0] if method == "freq_offset_omegas" else []))
    assert fake.live == before
    cb.close()
    assert not fake.live


def test_device_pointers_stay_plain_integers(fake):
    with oai.TurboDecoderBatch(40, 8) as dec, oai.UlDecodeBatch(1024, 2048, 2, 2) as ub:
        ub._alloc_w()
        for p in (dec.d_llr, dec.d_out, dec.d_it, dec.d_scr, ub.d_e, ub.d_w):
            assert type(p) is int
        assert dec.d_llr + 2 * dec.llr_stride > dec.d_llr
        # the zero fills go through oai4g_memset_d: d_out of the 16-bit decoder and the soft buffers
        assert sorted(h for n, h in fake.log if n == "oai4g_memset_d") == sorted([dec.d_out, ub.d_w])
    with oai.TurboDecoder8Batch(512, 8):
        pass
    assert [n for n, _ in fake.log].count("oai4g_memset_d") == 2


def test_results_of_structures_are_ctypes_arrays(fake):
    with oai.PdcchRxBatch(_fp(), 1, 0x1234, 0xFFFF, 2, PLAN, 3) as b:
        out = b.results()
        assert len(out) == 3 and isinstance(out[0], oai.PdcchRxResult)
        assert ctypes.sizeof(out) == 3 * ctypes.sizeof(oai.PdcchRxResult)
        out[2].dci[7].rnti = 0x4321
        assert out[2].dci[7].rnti == 0x4321
    with oai.PhichRxBatch(_fp(), [(0, 0, 0), (1, 0, 1)]) as b:
        assert len(b.results()) == 2
    with oai.PhichRxBatch(_fp(), []) as b:
        assert b.results() == []


def test_rx_batch_run_ends_in_llrs(fake, monkeypatch):
    with oai.RxBatch(_fp(), RA6, 2, 1, 0x1234, 2) as rx:
        marker = np.zeros(3, np.int16)
        monkeypatch.setattr(rx, "llrs", lambda: marker)
        n = 2 * 14 * 128
        assert rx.run(np.zeros(n, np.int32), np.zeros(n, np.int32)) is marker
