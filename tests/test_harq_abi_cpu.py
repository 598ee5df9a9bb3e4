"""CPU suite: the C ABI of the per-transport-block HARQ entry points, without a GPU.

  - oai4g_tx_config_enable_tb_rv, oai4g_tx_batch_rv, oai4g_tx_encode_rv,
    oai4g_ul_decode_batch_harq_tb and oai4g_harq_advance are exported, declared in include/oai4g.h,
    and bound by the Python mirror with the header's argument counts;
  - each returns its error value (-1) when it cannot run: without a device, and with a null
    configuration on any host;
  - oai4g_tx_params_t, which is broadcast as bytes, keeps its size and the offset of rvidx."""
import ctypes
import os
import re

import openair4g_amd as oai

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "oai4g.h")
NEW = {"oai4g_tx_config_enable_tb_rv": 1, "oai4g_tx_batch_rv": 7, "oai4g_tx_encode_rv": 6,
       "oai4g_ul_decode_batch_harq_tb": 12, "oai4g_harq_advance": 16}


def _declared_args(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name + " is not declared in include/oai4g.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_symbols_are_exported_declared_and_bound():
    lib = oai.load_library()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert name in oai.exported_symbols()
        assert _declared_args(name) == nargs, name
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs, name
        assert fn.restype is ctypes.c_int, name


def test_new_entries_return_their_error_value_when_they_cannot_run():
    lib = oai.load_library()
    have_gpu = lib.oai4g_init() == 0
    assert lib.oai4g_tx_config_enable_tb_rv(None) == -1
    assert lib.oai4g_last_error()
    assert lib.oai4g_tx_batch_rv(None, 1, None, None, None, None, None) == -1
    assert lib.oai4g_tx_encode_rv(None, 1, None, None, None, None) == -1
    assert lib.oai4g_ul_decode_batch_harq_tb(None, 1, None, 0, None, 0, None, None, None, 0, None, None) == -1
    assert lib.oai4g_harq_advance(1, 1, 4, 4, 1, None, None, None, None, None, None, None, None, 8, 0, None) == -1
    if not have_gpu:
        assert b"enable_tb_rv" not in lib.oai4g_last_error()      # refused for want of a device, before any argument


def test_tx_params_block_is_unchanged():
    assert ctypes.sizeof(oai.TxParams) == 92
    assert oai.TxParams.rvidx.offset == 44 and oai.TxParams.rvidx.size == 2
