"""CPU suite: the lifetime rule (openair4g_amd._DeviceOwner) for the fading channel's classes, on the stand-in
library of test_batch_lifetime_cpu.py: ChannelBatch with its lazily acquired draws buffer, and DlsimBler with a
channel model, which owns a ChannelBatch as a child."""
import gc

import numpy as np
import pytest

import openair4g_amd as oai
from openair4g_amd import dlsim
from test_batch_lifetime_cpu import FakeLib, _check_closed, fake  # noqa: F401

CASES = {
    "ChannelBatch": lambda: oai.ChannelBatch(2, 2, oai.ETU, 5.0, 4),
    "DlsimBler(channel_model)": lambda: dlsim.DlsimBler(4, N_RB_DL=6, batch=2, channel_model=oai.Rayleigh1),
}


def test_channel_batch_is_a_device_owner():
    assert issubclass(oai.ChannelBatch, oai._DeviceOwner)
    assert "close" not in vars(oai.ChannelBatch) and "__del__" not in vars(oai.ChannelBatch)


@pytest.mark.parametrize("name", list(CASES))
def test_close_releases_in_order_and_once(fake, name):  # noqa: F811
    o = CASES[name]()
    acquired = list(fake.live.items())
    assert acquired
    fake.log.clear()
    o.close()
    _check_closed(fake, o, acquired)


@pytest.mark.parametrize("name", list(CASES))
def test_a_failing_constructor_releases_what_it_acquired(fake, name):  # noqa: F811
    CASES[name]().close()
    n = fake.n_acq
    for k in range(1, n + 1):
        fake.n_acq, fake.fail_at = 0, k
        with pytest.raises(oai.OAI4GError):
            CASES[name]()
        gc.collect()
        assert not fake.live, (k, fake.live)
    assert not fake.errors


def test_the_draws_buffer_is_acquired_once_and_released(fake):  # noqa: F811
    o = oai.ChannelBatch(1, 1, oai.Rayleigh1, 5.0, 3)
    o.draws_per_vector = 2                                   # the stand-in's query fills nothing in
    before = len(fake.live)
    for _ in range(2):
        o.draw(draws=np.zeros((3, 2)))
    assert len(fake.live) == before + 1
    o.close()
    assert not fake.live and o.d_draws is None and o.cfg is None


def test_dlsim_without_a_model_creates_no_channel(fake):  # noqa: F811
    with dlsim.DlsimBler(4, N_RB_DL=6, batch=2) as sim:
        assert sim.chan is None
        assert "oai4g_channel_config_create" not in [n for n, _ in fake.log]
    with pytest.raises(ValueError):
        dlsim.DlsimBler(4, N_RB_DL=15, batch=2, channel_model=oai.Rayleigh1)
    gc.collect()
    assert not fake.live
