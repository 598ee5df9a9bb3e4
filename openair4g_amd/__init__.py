"""openair4g_amd — MI355X-native LTE PDSCH transmit path (host side).

This module is the Python mirror of the C ABI in ``include/oai4g.h``: ctypes bindings for
the drop-in entry points (``dlsch_encoding``, ``dlsch_scrambling``, ``dlsch_modulation``,
``PHY_ofdm_mod`` and their callees, named as in openair1/PHY) and for the batched,
device-resident transmit path (``TxPipeline``).  All arithmetic runs in the gfx950 kernels
of ``lib/libopenair4g_amd.so``; if that library or a gfx950 device is missing every compute
entry point raises ``OAI4GError`` — there is no CPU fallback.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libopenair4g_amd.so")

LTE_NULL = 2
NSOFT = 1827072
MAX_SEGMENTS = 16
MAX_CHANNEL_BITS = 14 * 1200 * 6
D_BYTES = 96 + 12 + 3 + 3 * 6144
W_BYTES = 3 * 6144 + 96
SISO, ALAMOUTI, LARGE_CDD = 0, 1, 2
# single-layer closed-loop precoding (TM4-6): the precoder of an RB comes from pmi_alloc (get_pmi)
(UNIFORM_PRECODING11, UNIFORM_PRECODING1m1, UNIFORM_PRECODING1j, UNIFORM_PRECODING1mj, PUSCH_PRECODING0,
 PUSCH_PRECODING1) = 3, 4, 5, 6, 7, 8
CYCLIC_PREFIX = 0


class OAI4GError(RuntimeError):
    pass


u8p = ctypes.POINTER(ctypes.c_uint8)


class FrameParms(ctypes.Structure):
    """oai4g_frame_parms_t — LTE_DL_FRAME_PARMS subset (PHY/impl_defs_lte.h:470-572)."""
    _fields_ = [("N_RB_DL", ctypes.c_uint16), ("Nid_cell", ctypes.c_uint16), ("Ncp", ctypes.c_uint8),
                ("nushift", ctypes.c_uint8), ("mode1_flag", ctypes.c_uint8), ("nb_antennas_tx", ctypes.c_uint8),
                ("frame_type", ctypes.c_uint8), ("symbols_per_tti", ctypes.c_uint8),
                ("log2_symbol_size", ctypes.c_uint8), ("Nid_cell_mbsfn", ctypes.c_uint8),
                ("ofdm_symbol_size", ctypes.c_uint16), ("first_carrier_offset", ctypes.c_uint16),
                ("nb_prefix_samples", ctypes.c_uint16), ("nb_prefix_samples0", ctypes.c_uint16),
                ("samples_per_tti", ctypes.c_uint32), ("phich_resource", ctypes.c_uint8),
                ("phich_duration", ctypes.c_uint8), ("tdd_config", ctypes.c_uint8),
                ("nb_antennas_tx_eNB", ctypes.c_uint8)]


class DciAlloc(ctypes.Structure):
    """oai4g_dci_alloc_t — DCI_ALLOC_t (PHY/LTE_TRANSPORT/defs.h:734-749)."""
    _fields_ = [("dci_length", ctypes.c_uint8), ("L", ctypes.c_uint8), ("nCCE", ctypes.c_int32),
                ("ra_flag", ctypes.c_uint8), ("rnti", ctypes.c_uint16), ("format", ctypes.c_uint32),
                ("dci_pdu", ctypes.c_uint8 * 8)]


class DlHarq(ctypes.Structure):
    """oai4g_dl_harq_t — LTE_DL_eNB_HARQ_t subset (PHY/LTE_TRANSPORT/defs.h:104-169)."""
    _fields_ = [("TBS", ctypes.c_uint32), ("B", ctypes.c_uint32), ("b", u8p), ("c", u8p * MAX_SEGMENTS),
                ("RTC", ctypes.c_uint32 * MAX_SEGMENTS), ("round", ctypes.c_uint8), ("mcs", ctypes.c_uint8),
                ("rvidx", ctypes.c_uint8), ("mimo_mode", ctypes.c_uint8), ("rb_alloc", ctypes.c_uint32 * 4),
                ("nb_rb", ctypes.c_uint16), ("e", u8p), ("d", u8p * MAX_SEGMENTS), ("w", u8p * MAX_SEGMENTS),
                ("C", ctypes.c_uint32), ("Cminus", ctypes.c_uint32), ("Cplus", ctypes.c_uint32),
                ("Kminus", ctypes.c_uint32), ("Kplus", ctypes.c_uint32), ("F", ctypes.c_uint32),
                ("Nl", ctypes.c_uint8), ("Nlayers", ctypes.c_uint8), ("first_layer", ctypes.c_uint8),
                ("pmi_alloc", ctypes.c_uint16)]


class Dlsch(ctypes.Structure):
    """oai4g_dlsch_t — LTE_eNB_DLSCH_t subset (PHY/LTE_TRANSPORT/defs.h:240-274)."""
    _fields_ = [("rnti", ctypes.c_uint16), ("current_harq_pid", ctypes.c_uint8), ("Mdlharq", ctypes.c_uint8),
                ("Kmimo", ctypes.c_uint8), ("sqrt_rho_a", ctypes.c_int16), ("sqrt_rho_b", ctypes.c_int16),
                ("harq_processes", ctypes.POINTER(DlHarq) * 8)]


class TxParams(ctypes.Structure):
    """oai4g_tx_params_t — the POD parameter block rank 0 broadcasts to the other ranks."""
    _fields_ = [("N_RB_DL", ctypes.c_uint16), ("Nid_cell", ctypes.c_uint16), ("Ncp", ctypes.c_uint8),
                ("nb_antennas_tx", ctypes.c_uint8), ("mode1_flag", ctypes.c_uint8), ("frame_type", ctypes.c_uint8),
                ("n_cw", ctypes.c_uint8), ("mimo_mode", ctypes.c_uint8), ("num_pdcch_symbols", ctypes.c_uint8),
                ("Kmimo", ctypes.c_uint8), ("Mdlharq", ctypes.c_uint8), ("first_subframe", ctypes.c_uint8),
                ("subframe_step", ctypes.c_uint8), ("with_crs", ctypes.c_uint8), ("rnti", ctypes.c_uint16),
                ("amp", ctypes.c_int16), ("sqrt_rho_a", ctypes.c_int16), ("sqrt_rho_b", ctypes.c_int16),
                ("rb_alloc", ctypes.c_uint32 * 4), ("nb_rb", ctypes.c_uint16), ("mcs", ctypes.c_uint8 * 2),
                ("rvidx", ctypes.c_uint8 * 2), ("q", ctypes.c_uint8 * 2), ("TBS", ctypes.c_uint32 * 2),
                ("payload_stride", ctypes.c_uint32), ("rm_limited_buffer", ctypes.c_uint32),
                ("pmi_alloc", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 6)]

    def to_bytes(self):
        return bytes(ctypes.string_at(ctypes.addressof(self), ctypes.sizeof(self)))

    @classmethod
    def from_bytes(cls, b):
        p = cls()
        ctypes.memmove(ctypes.addressof(p), bytes(b), ctypes.sizeof(cls))
        return p


_lib = None

_SIGS = {
    "oai4g_init": (ctypes.c_int, []),
    "oai4g_last_error": (ctypes.c_char_p, []),
    "oai4g_device_name": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "oai4g_init_frame_parms": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_uint16, ctypes.c_uint16,
                                              ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_get_Qm": (ctypes.c_uint8, [ctypes.c_uint8]),
    "oai4g_get_Qm_ul": (ctypes.c_uint8, [ctypes.c_uint8]),
    "oai4g_get_I_TBS": (ctypes.c_uint8, [ctypes.c_uint8]),
    "oai4g_get_I_TBS_UL": (ctypes.c_uint8, [ctypes.c_uint8]),
    "oai4g_tbs_bits": (ctypes.c_uint32, [ctypes.c_uint8, ctypes.c_uint16]),
    "oai4g_get_TBS_DL": (ctypes.c_uint32, [ctypes.c_uint8, ctypes.c_uint16]),
    "oai4g_get_TBS_UL": (ctypes.c_uint32, [ctypes.c_uint8, ctypes.c_uint16]),
    "oai4g_get_G": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_uint16, ctypes.POINTER(ctypes.c_uint32),
                                   ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_int, ctypes.c_uint8]),
    "oai4g_new_dlsch": (ctypes.POINTER(Dlsch), [ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_free_dlsch": (None, [ctypes.POINTER(Dlsch)]),
    "oai4g_lte_gold_generic": (ctypes.c_uint32, [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                                 ctypes.c_uint8]),
    "oai4g_crc24a": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_crc24b": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_lte_segmentation": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(u8p), ctypes.c_uint32]
                               + [ctypes.POINTER(ctypes.c_uint32)] * 6),
    "oai4g_threegpplte_turbo_encoder": (None, [ctypes.c_void_p, ctypes.c_uint16, ctypes.c_void_p, ctypes.c_uint8,
                                               ctypes.c_uint16, ctypes.c_uint16]),
    "oai4g_sub_block_interleaving_turbo": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_lte_rate_matching_turbo": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                                        ctypes.c_void_p] + [ctypes.c_uint8] + [ctypes.c_uint32]
                                      + [ctypes.c_uint8] * 8),
    "oai4g_dlsch_encoding": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(FrameParms), ctypes.c_uint8,
                                            ctypes.POINTER(Dlsch), ctypes.c_int, ctypes.c_uint8]),
    "oai4g_dlsch_scrambling": (None, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.POINTER(Dlsch), ctypes.c_int,
                                      ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_dlsch_modulation": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int16, ctypes.c_uint32,
                                              ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.POINTER(Dlsch),
                                              ctypes.POINTER(Dlsch)]),
    "oai4g_PHY_ofdm_mod": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint16,
                                  ctypes.c_int]),
    "oai4g_normal_prefix_mod": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint8, ctypes.POINTER(FrameParms)]),
    "oai4g_do_OFDM_mod": (None, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32,
                                 ctypes.c_uint16, ctypes.POINTER(FrameParms)]),
    "oai4g_generate_pilots": (None, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int16, ctypes.POINTER(FrameParms),
                                     ctypes.c_uint16]),
    "oai4g_lte_dl_cell_spec": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int16, ctypes.POINTER(FrameParms),
                                              ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_phy_threegpplte_turbo_decoder16": (ctypes.c_uint8, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint16,
                                                               ctypes.c_uint16, ctypes.c_uint16, ctypes.c_uint8,
                                                               ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_lte_rate_matching_turbo_rx": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint8,
                                                        ctypes.c_uint32] + [ctypes.c_uint8] * 7 +
                                         [ctypes.POINTER(ctypes.c_uint32)]),
    "oai4g_sub_block_deinterleaving_turbo": (None, [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_td_scratch_bytes": (ctypes.c_size_t, [ctypes.c_uint16, ctypes.c_int]),
    "oai4g_td_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint16, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                      ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8,
                                      ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_idft": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_idft2048": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_idft1024": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_idft512": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_idft256": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_idft128": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_idft64": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_generate_pcfich_reg_mapping": (None, [ctypes.POINTER(FrameParms), ctypes.POINTER(ctypes.c_uint16),
                                                  ctypes.POINTER(ctypes.c_uint8)]),
    "oai4g_get_mi": (ctypes.c_uint8, [ctypes.POINTER(FrameParms), ctypes.c_uint8]),
    "oai4g_get_nquad": (ctypes.c_uint16, [ctypes.c_uint8, ctypes.POINTER(FrameParms), ctypes.c_uint8]),
    "oai4g_get_nCCE": (ctypes.c_uint16, [ctypes.c_uint8, ctypes.POINTER(FrameParms), ctypes.c_uint8]),
    "oai4g_get_num_pdcch_symbols": (ctypes.c_uint8, [ctypes.c_uint8, ctypes.POINTER(DciAlloc),
                                                     ctypes.POINTER(FrameParms), ctypes.c_uint8]),
    "oai4g_generate_phich_reg_mapping": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.POINTER(ctypes.c_uint16)]),
    "oai4g_init_nCCE_table": (None, []),
    "oai4g_get_nCCE_offset": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_int, ctypes.c_int, ctypes.c_uint16,
                                             ctypes.c_uint8]),
    "oai4g_generate_dci_top": (ctypes.c_uint8, [ctypes.c_uint8, ctypes.c_uint8, ctypes.POINTER(DciAlloc),
                                                ctypes.c_uint32, ctypes.c_int16, ctypes.POINTER(FrameParms),
                                                ctypes.c_void_p, ctypes.c_uint32]),
    "oai4g_tx_config_set_control": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8,
                                                    ctypes.POINTER(DciAlloc)]),
    "oai4g_generate_pcfich": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_int16, ctypes.POINTER(FrameParms),
                                             ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint8]),
    "oai4g_generate_pss": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int16, ctypes.POINTER(FrameParms),
                                          ctypes.c_uint16, ctypes.c_uint16]),
    "oai4g_generate_sss": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int16, ctypes.POINTER(FrameParms),
                                          ctypes.c_uint16, ctypes.c_uint16]),
    "oai4g_generate_pbch": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                                           ctypes.POINTER(FrameParms), ctypes.c_void_p, ctypes.c_uint8]),
    "oai4g_generate_phich": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int16, ctypes.c_uint8, ctypes.c_uint8,
                                            ctypes.c_uint8, ctypes.c_uint8, ctypes.POINTER(ctypes.c_void_p)]),
    "oai4g_phich_group_seq": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_uint16, ctypes.c_uint8,
                                             ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8)]),
    "oai4g_tx_config_set_common": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_rx_pdsch_siso": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint8, ctypes.c_uint8,
                                           ctypes.c_uint8, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8)]),
    "oai4g_dlsch_unscrambling": (None, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_uint16, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_rx_config_create": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.POINTER(ctypes.c_uint32),
                                                 ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint8,
                                                 ctypes.c_uint8]),
    "oai4g_rx_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_rx_llr_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_rx_llr_stride": (ctypes.c_size_t, [ctypes.c_void_p]),
    "oai4g_rx_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int, ctypes.c_void_p]),
    "oai4g_lte_dl_channel_estimation": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_chest_filters": (None, [ctypes.c_uint8, ctypes.c_void_p]),
    "oai4g_chest_dc_filters": (None, [ctypes.c_uint8, ctypes.c_void_p]),
    "oai4g_ul_config_set_decoder": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_set_device": (ctypes.c_int, [ctypes.c_int]),
    "oai4g_dist_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "oai4g_dist_init": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "oai4g_dist_broadcast_params": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_dist_allreduce_sum_u64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_dist_allreduce_max_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_dist_barrier": (ctypes.c_int, []),
    "oai4g_dist_rank": (ctypes.c_int, []),
    "oai4g_dist_world": (ctypes.c_int, []),
    "oai4g_dist_finalize": (ctypes.c_int, []),
    "oai4g_shard_range": (None, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                 ctypes.POINTER(ctypes.c_int)]),
    "oai4g_payload_seed": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]),
    "oai4g_chest_config_set_stride": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]),
    "oai4g_rx_pdsch_tm3": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                                          ctypes.c_uint8, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_rx_config_create_tm3": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_void_p, ctypes.c_uint8,
                                                     ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint16,
                                                     ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_rx_batch_tm3": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oai4g_rx_pdsch_tm3_2cw": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8,
                                              ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_rx_batch_tm3_2cw": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oai4g_rx_pdsch_tm2": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_rx_config_create_tm2": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_void_p, ctypes.c_uint8,
                                                     ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint8, ctypes.c_uint8,
                                                     ctypes.c_uint8]),
    "oai4g_rx_batch_tm2": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oai4g_rx_pdsch_tm56": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint16,
                                           ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "oai4g_rx_config_create_tm56": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_void_p, ctypes.c_uint8,
                                                      ctypes.c_uint8, ctypes.c_uint16, ctypes.c_int, ctypes.c_uint8,
                                                      ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint8, ctypes.c_uint8,
                                                      ctypes.c_uint8]),
    "oai4g_rx_batch_tm56": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oai4g_rx_batch_tm56_pilots": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oai4g_dl_ch_estimates_time": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_void_p]),
    "oai4g_chest_time_batch": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "oai4g_lte_est_freq_offset": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(FrameParms), ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "oai4g_freq_offset_omega_batch": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_void_p,
                                                     ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_freq_offset_update": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int32,
                                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "oai4g_signal_energy": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32]),
    "oai4g_signal_energy_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_awgn_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_double, ctypes.c_uint64, ctypes.c_uint32,
                                        ctypes.c_void_p]),
    "oai4g_chest_config_create": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8,
                                                    ctypes.c_uint8]),
    "oai4g_chest_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_rx_batch_estimated": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oai4g_chest_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "oai4g_chest_batch_pilots": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "oai4g_rx_batch_tm3_pilots": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oai4g_rx_batch_tm3_2cw_pilots": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oai4g_phy_threegpplte_turbo_decoder8": (ctypes.c_uint8, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint16,
                                                              ctypes.c_uint16, ctypes.c_uint16, ctypes.c_uint8,
                                                              ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_td8_scratch_bytes": (ctypes.c_size_t, [ctypes.c_uint16, ctypes.c_int]),
    "oai4g_td8_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint16, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                       ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_generate_dummy_w": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint8]),
    "oai4g_ul_config_create": (ctypes.c_void_p, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint8,
                                                 ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint8]),
    "oai4g_ul_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_ul_config_C": (ctypes.c_int, [ctypes.c_void_p]),
    "oai4g_ul_config_E": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_ul_config_G_offset": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_ul_decode_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_ul_config_w_entries": (ctypes.c_size_t, [ctypes.c_void_p]),
    "oai4g_ul_decode_batch_harq": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                                  ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint8, ctypes.c_uint8,
                                                  ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_dft": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_dft2048": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_dft1024": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_dft512": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_dft256": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_dft128": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_dft64": (None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_slot_fep_offset": (ctypes.c_int64, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8,
                                               ctypes.c_int, ctypes.c_int]),
    "oai4g_slot_fep": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                                      ctypes.c_int, ctypes.c_int]),
    "oai4g_fep_batch": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_tx_config_create": (ctypes.c_void_p, [ctypes.POINTER(TxParams)]),
    "oai4g_tx_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_tx_G": (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "oai4g_tx_ebits_words": (ctypes.c_uint32, [ctypes.c_void_p]),
    "oai4g_tx_iq_samples": (ctypes.c_uint32, [ctypes.c_void_p]),
    "oai4g_tx_workspace_bytes": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int]),
    "oai4g_tx_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_tx_batch_timed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "oai4g_tx_encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "oai4g_tx_modulate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "oai4g_tx_mod_nosat": (ctypes.c_int, [ctypes.c_void_p]),
    "oai4g_diag_encode_phase_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "oai4g_diag_encode_occupancy": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                                   ctypes.POINTER(ctypes.c_size_t)]),
    "oai4g_diag_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                         ctypes.c_void_p]),
    "oai4g_dev_alloc": (ctypes.c_void_p, [ctypes.c_size_t]),
    "oai4g_dev_free": (None, [ctypes.c_void_p]),
    "oai4g_memcpy_h2d": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "oai4g_memcpy_d2h": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "oai4g_memset_d": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]),
    "oai4g_sync": (ctypes.c_int, []),
    "oai4g_fill_payload": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p]),
    "oai4g_qpp_fold32": (ctypes.c_int, [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]),
    "oai4g_rsc_scan_rows": (ctypes.c_int, [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "oai4g_rm_pair_schedule": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.POINTER(ctypes.c_uint32)]),
    "oai4g_mod_item_map": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(ctypes.c_uint32)]),
    "oai4g_get_pmi": (ctypes.c_uint8, [ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint16]),
    "oai4g_set_modofdm_grid_cap": (None, [ctypes.c_int]),
    "oai4g_tx_mod_lz": (ctypes.c_int, [ctypes.c_void_p]),
    "oai4g_harq_advance": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_uint8, ctypes.c_int, ctypes.c_int]
                           + [ctypes.c_void_p] * 8 + [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p]),
    "oai4g_tx_config_enable_tb_rv": (ctypes.c_int, [ctypes.c_void_p]),
    "oai4g_tx_batch_rv": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_tx_encode_rv": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_ul_decode_batch_harq_tb": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                                     ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_phy_viterbi_lte": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint16]),
    "oai4g_diag_viterbi_lte": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint16, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    "oai4g_cc_rx_plan": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_void_p]),
    "oai4g_dci_decoding": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_dci_decoding_crc": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.POINTER(ctypes.c_uint16)]),
    "oai4g_pbch_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_void_p]),
    "oai4g_pbch_decode_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(FrameParms),
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_pdcch_soft_bit_table": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8,
                                                  ctypes.c_void_p, ctypes.c_uint32]),
    "oai4g_pdcch_soft_bits": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8,
                                             ctypes.c_void_p]),
    "oai4g_dci_decoding_procedure0": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint16, ctypes.c_void_p,
                                                     ctypes.c_int, ctypes.c_uint8, ctypes.c_void_p,
                                                     ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint16,
                                                     ctypes.c_uint16] + [ctypes.c_uint8] * 6 + [ctypes.c_void_p] * 6),
    "oai4g_pdcch_candidates": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint16,
                                              ctypes.c_int, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_pdcch_rx_config_create": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint16,
                                                       ctypes.c_uint16, ctypes.c_uint16, ctypes.c_void_p, ctypes.c_int]),
    "oai4g_pdcch_rx_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_pdcch_rx_candidates": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_int]),
    "oai4g_pdcch_rx_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_void_p]),
    "oai4g_pdcch_rx_batch_detected": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                     ctypes.c_void_p]),
    "oai4g_rx_pdcch_front": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                                            ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8),
                                            ctypes.POINTER(ctypes.c_uint8), ctypes.c_void_p]),
    "oai4g_rx_pcfich": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint8]),
    "oai4g_rx_pdcch": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                                      ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8)]),
    "oai4g_pdcch_front_config_create": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8,
                                                          ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_pdcch_front_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_pdcch_front_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_rx_pbch_front": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                           ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                                           ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "oai4g_rx_pbch": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                     ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                                     ctypes.c_uint32, ctypes.c_uint8, ctypes.c_void_p]),
    "oai4g_pbch_front_config_create": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8,
                                                         ctypes.c_uint32]),
    "oai4g_pbch_front_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_pbch_front_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    "oai4g_pbch_detect_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "oai4g_lte_sync_time_replicas": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_void_p]),
    "oai4g_sync_config_create": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_uint8]),
    "oai4g_sync_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_sync_time_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_lte_sync_time": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(FrameParms), ctypes.c_uint8,
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.c_void_p]),
    "oai4g_fep_offset_batch": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint8, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "oai4g_sss_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "oai4g_sss_rows_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_rx_sss": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(FrameParms), ctypes.c_uint8,
                                    ctypes.c_uint8, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                                    ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8)]),
    "oai4g_initial_sync": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(FrameParms), ctypes.c_uint8,
                                          ctypes.c_uint8, ctypes.c_uint32, ctypes.c_void_p]),
    "oai4g_rx_phich": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint8,
                                      ctypes.c_uint8, ctypes.POINTER(ctypes.c_int16)]),
    "oai4g_phich_rx_config_create": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_phich_rx_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_phich_rx_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_channel_config_create": (ctypes.c_void_p, [ctypes.c_uint8, ctypes.c_uint8, ctypes.c_int, ctypes.c_double,
                                                      ctypes.c_double, ctypes.c_int32, ctypes.c_double, ctypes.c_int]),
    "oai4g_channel_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_channel_config_query": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_channel_model_describe": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_double,
                                                    ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_channel_random_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32,
                                                  ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_channel_set_taps": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_channel_get_taps": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_multipath_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                             ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_size_t,
                                             ctypes.c_void_p, ctypes.c_double, ctypes.c_uint64, ctypes.c_uint32,
                                             ctypes.c_void_p]),
    "oai4g_random_channel": (ctypes.c_int, [ctypes.c_void_p]),
    "oai4g_multipath_channel": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_void_p)] * 4
                                + [ctypes.c_uint32, ctypes.c_uint8]),
    "oai4g_pusch_dft_plan": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "oai4g_pusch_config_create": (ctypes.c_void_p, [ctypes.POINTER(FrameParms), ctypes.c_uint16, ctypes.c_uint16, ctypes.c_uint8,
                                                    ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint8, ctypes.c_uint8]),
    "oai4g_pusch_config_destroy": (None, [ctypes.c_void_p]),
    "oai4g_pusch_mod_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int16,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_pusch_dft_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_pusch_idft_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "oai4g_dft_lte": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint8]),
    "oai4g_pusch_dft": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint8]),
    "oai4g_lte_idft": (ctypes.c_int, [ctypes.POINTER(FrameParms), ctypes.c_void_p, ctypes.c_uint16]),
    "oai4g_ulsch_modulation": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int16, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.POINTER(FrameParms), ctypes.c_void_p]),
}


def load_library(path=None):
    """Load the HIP library (raises OAI4GError if it is not built).  OAI4G_LIB selects an
    alternative in-tree build (kernel variants for A/B measurements)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("OAI4G_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise OAI4GError(f"HIP library not built: {path} (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return sorted(_SIGS)


def lib():
    return load_library()


def init():
    """Initialise the device (raises if no gfx950 GPU: no CPU fallback)."""
    L = lib()
    if L.oai4g_init() != 0:
        raise OAI4GError(L.oai4g_last_error().decode())
    return L


def _check(ok):
    if not ok:
        raise OAI4GError(lib().oai4g_last_error().decode())


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class _DeviceOwner:
    """Base of every device-resident class, the one owner of its buffers, handles and child batches.  close()
    synchronises once, destroys the handles newest first, then frees the buffers newest first, and leaves `cfg`
    and every `d_*` None; a second close() makes no call, and a half-built object (a constructor raised) closes."""
    _owned = ()                         # (0 handle / 1 buffer, release, its argument) in order of acquisition

    def _dev(self, nbytes, zero=False):
        """a device buffer (zero-filled on request) that close() frees: its address, a plain int"""
        p = self.L.oai4g_dev_alloc(nbytes)
        _check(bool(p))
        self._owned += ((1, self.L.oai4g_dev_free, p),)
        if zero:                        # the fill is complete on return, whichever stream uses the buffer first
            _check(self.L.oai4g_memset_d(p, 0, nbytes) == 0 and self.L.oai4g_sync() == 0)
        return p

    def _own(self, handle, destroy=None):
        """take over a handle with its destroy function, or a child batch: its handles go with ours, then its buffers"""
        _check(bool(handle))
        kid = destroy is None
        self._owned += ((0, handle._release, 0), (1, handle._release, 1)) if kid else ((0, destroy, handle),)
        return handle

    def _release(self, rank):
        for r, release, arg in reversed(self._owned):
            if r == rank:
                release(arg)
        if rank:
            self._owned = ()
            vars(self).update({k: None for k in vars(self) if k == "cfg" or k.startswith("d_")})

    def close(self):
        if self._owned:
            self.L.oai4g_sync()
            self._release(0)
            self._release(1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _put(self, d_ptr, a):
        """a contiguous host array to a device pointer"""
        _check(self.L.oai4g_memcpy_h2d(d_ptr, _ptr(a), a.nbytes) == 0)

    def _get(self, d_ptr, shape, dtype):
        """synchronise, then a device pointer's contents as a new array (a ctypes array for a Structure dtype)"""
        _check(self.L.oai4g_sync() == 0)
        struct = isinstance(dtype, type(ctypes.Structure))
        out = np.empty(shape * ctypes.sizeof(dtype), np.uint8) if struct else np.empty(shape, dtype)
        _check(self.L.oai4g_memcpy_d2h(_ptr(out), d_ptr, out.nbytes) == 0)
        return (dtype * shape).from_buffer(out) if struct else out


def device_name():
    L = init()
    buf = ctypes.create_string_buffer(256)
    _check(L.oai4g_device_name(buf, 256) == 0)
    return buf.value.decode()


# ------------------------------------------------------------------------------------------
# drop-in entry points (host numpy buffers in/out, GPU compute)
# ------------------------------------------------------------------------------------------
def frame_parms(N_RB_DL, Nid_cell=0, Ncp=0, nb_antennas_tx=1, mode1_flag=1, frame_type=0):
    fp = FrameParms()
    _check(lib().oai4g_init_frame_parms(ctypes.byref(fp), N_RB_DL, Nid_cell, Ncp, nb_antennas_tx, mode1_flag,
                                        frame_type) == 0)
    return fp


def get_G(fp, nb_rb, rb_alloc, Qm, Nl, num_pdcch, subframe):
    ra = (ctypes.c_uint32 * 4)(*rb_alloc)
    return lib().oai4g_get_G(ctypes.byref(fp), nb_rb, ra, Qm, Nl, num_pdcch, 0, subframe)


def crc24a(data, bitlen):
    init()
    a = np.ascontiguousarray(data, dtype=np.uint8)
    return int(lib().oai4g_crc24a(_ptr(a), bitlen))


def crc24b(data, bitlen):
    init()
    a = np.ascontiguousarray(data, dtype=np.uint8)
    return int(lib().oai4g_crc24b(_ptr(a), bitlen))


def turbo_encode(c, f1, f2):
    """threegpplte_turbo_encoder: c (K/8 bytes) -> d (3K+12 bytes)."""
    init()
    c = np.ascontiguousarray(c, dtype=np.uint8)
    K = 8 * len(c)
    d = np.zeros(3 * K + 12, dtype=np.uint8)
    lib().oai4g_threegpplte_turbo_encoder(_ptr(c), len(c), _ptr(d), 0, f1, f2)
    _check(True)
    return d


def subblock_interleave(d_full, D):
    """sub_block_interleaving_turbo: d_full = 96-byte NULL prefix + d.  Returns (R, w)."""
    init()
    d_full = np.ascontiguousarray(d_full, dtype=np.uint8)
    R = (D + 31) >> 5
    w = np.zeros(3 * 32 * R, dtype=np.uint8)
    dptr = ctypes.c_void_p(d_full.ctypes.data + 96)
    rtc = lib().oai4g_sub_block_interleaving_turbo(D, dptr, _ptr(w))
    if rtc == 0:
        _check(False)
    return rtc, w


def rate_match(RTC, G, w, C, r, Qm, rvidx=0, Nl=1, Kmimo=1, Mdlharq=8, Nsoft=NSOFT):
    init()
    w = np.ascontiguousarray(w, dtype=np.uint8)
    e = np.zeros(G + 64, dtype=np.uint8)
    E = lib().oai4g_lte_rate_matching_turbo(RTC, G, _ptr(w), _ptr(e), C, Nsoft, Mdlharq, Kmimo, rvidx, Qm, Nl, r,
                                            0, 0)
    return e[:E]


def idft(x, scale=1):
    """x: complex int16 pairs as int16 array of length 2N."""
    init()
    x = np.ascontiguousarray(x, dtype=np.int16)
    n = len(x) // 2
    y = np.zeros_like(x)
    _check(lib().oai4g_idft(int(n).bit_length() - 1, _ptr(x), _ptr(y), scale) == 0)
    return y


def generate_pcfich(cfi, amp, fp, grids, subframe):
    """generate_pcfich drop-in on a list of frame grids (int32 arrays, modified in place)."""
    init()
    n = len(grids)
    gp = (ctypes.c_void_p * n)(*[g.ctypes.data for g in grids])
    return lib().oai4g_generate_pcfich(cfi, amp, ctypes.byref(fp), gp, subframe)


def _grid_ptrs(grids):
    return (ctypes.c_void_p * len(grids))(*[g.ctypes.data for g in grids])


def generate_pss(grids, amp, fp, symbol, slot_offset):
    """generate_pss drop-in (pss.c:50) on frame grids (int32 arrays, modified in place)."""
    init()
    return lib().oai4g_generate_pss(_grid_ptrs(grids), amp, ctypes.byref(fp), symbol, slot_offset)


def generate_sss(grids, amp, fp, symbol, slot_offset):
    """generate_sss drop-in (sss.c:47)."""
    init()
    return lib().oai4g_generate_sss(_grid_ptrs(grids), amp, ctypes.byref(fp), symbol, slot_offset)


class PhichItem(ctypes.Structure):
    _fields_ = [("subframe", ctypes.c_uint8), ("ngroup", ctypes.c_uint8), ("nseq", ctypes.c_uint8), ("hi", ctypes.c_uint8)]


class CommonSig(ctypes.Structure):
    """oai4g_common_sig_t"""
    _fields_ = [("pss_sss", ctypes.c_uint8), ("pbch", ctypes.c_uint8), ("pbch_pdu", ctypes.c_uint8 * 3),
                ("frame_mod4", ctypes.c_uint8), ("n_phich", ctypes.c_uint8), ("phich", PhichItem * 64)]


class Pbch(ctypes.Structure):
    """oai4g_pbch_t (LTE_eNB_PBCH): the scrambled coded bits kept across frame_mod4."""
    _fields_ = [("pbch_e", ctypes.c_uint8 * 1920)]


def generate_pbch(state, grids, amp, fp, pdu, frame_mod4):
    """generate_pbch drop-in (pbch.c:161) on the subframe-0 grids."""
    init()
    pdu = np.ascontiguousarray(pdu, dtype=np.uint8)
    return lib().oai4g_generate_pbch(ctypes.byref(state), _grid_ptrs(grids), amp, ctypes.byref(fp), _ptr(pdu), frame_mod4)


def generate_phich(fp, amp, nseq, ngroup, hi, subframe, grids):
    """generate_phich drop-in (phich.c:401) on frame grids."""
    init()
    return lib().oai4g_generate_phich(ctypes.byref(fp), amp, nseq, ngroup, hi, subframe, _grid_ptrs(grids))


def phich_group_seq(fp, first_rb, n_dmrs):
    g, q = ctypes.c_uint8(), ctypes.c_uint8()
    _check(lib().oai4g_phich_group_seq(ctypes.byref(fp), first_rb, n_dmrs, ctypes.byref(g), ctypes.byref(q)) == 0)
    return g.value, q.value


def dft(x, scale=1):
    """Forward DFT (lte_dfts.c dft64..dft2048): complex int16 pairs, int16 array of length 2N."""
    init()
    x = np.ascontiguousarray(x, dtype=np.int16)
    n = len(x) // 2
    y = np.zeros_like(x)
    _check(lib().oai4g_dft(int(n).bit_length() - 1, _ptr(x), _ptr(y), scale) == 0)
    return y


def slot_fep(rxdata, rxdataF, fp, l, Ns, sample_offset=0, no_prefix=0):
    """slot_fep drop-in: rxdata / rxdataF are lists (one per RX antenna) of int32 arrays, modified
    in place (rxdata: 10 subframes + N words of wrap extension).  Returns the entry point's code."""
    init()
    n = len(rxdata)
    rp = (ctypes.c_void_p * n)(*[a.ctypes.data for a in rxdata])
    fpp = (ctypes.c_void_p * n)(*[a.ctypes.data for a in rxdataF])
    return lib().oai4g_slot_fep(rp, fpp, ctypes.byref(fp), n, l, Ns, sample_offset, no_prefix)


def rx_pdsch_siso(fp, rxdataF, dl_ch, rb_alloc, Qm, num_pdcch, subframe):
    """rx_pdsch over one subframe's PDSCH symbols (TM1, one RX antenna): rxdataF / dl_ch are
    int32 [nsymb*N].  Returns (LLR stream int16, log2_maxh)."""
    init()
    rxdataF = np.ascontiguousarray(rxdataF, dtype=np.int32)
    dl_ch = np.ascontiguousarray(dl_ch, dtype=np.int32)
    out = np.zeros(14 * 1200 * 6 + 64, dtype=np.int16)
    sh = ctypes.c_uint8()
    ra = (ctypes.c_uint32 * 4)(*rb_alloc)
    n = lib().oai4g_rx_pdsch_siso(ctypes.byref(fp), _ptr(rxdataF), _ptr(dl_ch), ra, Qm, num_pdcch, subframe,
                                  _ptr(out), ctypes.byref(sh))
    _check(n >= 0)
    return out[:n], sh.value


def _rx_dual_args(rxF, est):
    """(nb_rx, antenna pointers, plane pointers [p * 2 + a], the arrays they point into) of a two-port
    drop-in: rxF = [nb_rx][nsymb*N], est[(p, a)] = [nsymb*N]"""
    nb_rx = len(rxF)
    rx = [np.ascontiguousarray(r, dtype=np.int32) for r in rxF]
    keep = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in est.items()}
    ep = (ctypes.c_void_p * 4)()
    for (p_, a), arr in keep.items():
        if a < nb_rx:
            ep[2 * p_ + a] = arr.ctypes.data
    rp = (ctypes.c_void_p * 2)(*[r.ctypes.data for r in rx] + [None] * (2 - nb_rx))
    return nb_rx, rp, ep, (rx, keep)


def _rx_dual(entry, fp, rxF, est, rb_alloc, args, n_out=1):
    """one two-port drop-in: `args` go between rb_alloc and the n_out LLR outputs; returns the outputs
    cut to the stream length, then log2_maxh"""
    init()
    nb_rx, rp, ep, _keep = _rx_dual_args(rxF, est)
    outs = [np.zeros(14 * 1200 * 6 + 64, dtype=np.int16) for _ in range(n_out)]
    sh = ctypes.c_uint8()
    ra = (ctypes.c_uint32 * 4)(*rb_alloc)
    n = getattr(lib(), entry)(ctypes.byref(fp), nb_rx, rp, ep, ra, *args, *[_ptr(o) for o in outs], ctypes.byref(sh))
    _check(n >= 0)
    return (*[o[:n] for o in outs], sh.value)


def rx_pdsch_tm3(fp, rxF, est, rb_alloc, Qm0, Qm1, mcs0, num_pdcch, subframe):
    """rx_pdsch for TM3 (dual_stream_flag = 0): rxF = [nb_rx][nsymb*N], est[(p, a)] = [nsymb*N].
    Returns (codeword-0 LLRs, log2_maxh)."""
    return _rx_dual("oai4g_rx_pdsch_tm3", fp, rxF, est, rb_alloc, (Qm0, Qm1, mcs0, num_pdcch, subframe))


def rx_pdsch_tm3_2cw(fp, rxF, est, rb_alloc, mcs0, num_pdcch, subframe):
    """rx_pdsch for TM3 with both codewords QPSK: rxF = [nb_rx][nsymb*N], est[(p, a)] = [nsymb*N].
    Returns (codeword-0 LLRs, codeword-1 LLRs, log2_maxh)."""
    return _rx_dual("oai4g_rx_pdsch_tm3_2cw", fp, rxF, est, rb_alloc, (mcs0, num_pdcch, subframe), n_out=2)


def rx_pdsch_tm2(fp, rxF, est, rb_alloc, Qm, num_pdcch, subframe):
    """rx_pdsch for TM2 (ALAMOUTI): rxF = [nb_rx][nsymb*N], est[(p, a)] = [nsymb*N].
    Returns (LLRs, log2_maxh)."""
    return _rx_dual("oai4g_rx_pdsch_tm2", fp, rxF, est, rb_alloc, (Qm, num_pdcch, subframe))


# the subband of a PRB in the TM4-6 receiver: the reference UE's 4-RB rule / the transmitter's get_pmi
RX_PMI_UE, RX_PMI_TX = 0, 1


def rx_pdsch_tm56(fp, rxF, est, rb_alloc, Qm, mimo_mode, pmi_alloc, dl_power_off, num_pdcch, subframe):
    """rx_pdsch for the single-layer precoding modes 3..7 (TM4-6, dual_stream_flag = 0, the reference UE's
    subband rule): rxF = [nb_rx][nsymb*N], est[(p, a)] = [nsymb*N].  Returns (LLRs, log2_maxh)."""
    return _rx_dual("oai4g_rx_pdsch_tm56", fp, rxF, est, rb_alloc,
                    (Qm, mimo_mode, pmi_alloc, dl_power_off, num_pdcch, subframe))


class _EstPlanes(_DeviceOwner):
    """The estimate planes of a two-port receiver and their channel estimation, shared by _RxBatchDual,
    PdcchFrontBatch and PbchFrontBatch: d_est holds four planes [2 p + a][n][nsymb * N] (port p at receive
    antenna a) of n subframes; the user sets L, fp and nb_rx before _est_setup."""

    def _est_setup(self, n, n_ports):
        self._n_est, self._n_ports, self._chest = n, n_ports, {}
        self.plane = n * self.fp.symbols_per_tti * self.fp.ofdm_symbol_size
        self.d_est = self._dev(4 * self.plane * 4)

    def est_plane(self, p, a):
        """device pointer of the estimate plane of port p at receive antenna a"""
        return ctypes.c_void_p(self.d_est + (2 * p + a) * self.plane * 4)

    def upload_estimates(self, est):
        """est[(p, a)] = int32 [n][nsymb * N]"""
        for (p, a), v in est.items():
            v = np.ascontiguousarray(v, dtype=np.int32)
            assert v.size == self.plane
            self._put(self.est_plane(p, a), v)

    def estimates(self):
        """the four planes as they stand on the device: int32 [2 p + a][n][nsymb * N]"""
        return self._get(self.d_est, (4, self._n_est, self.plane // self._n_est), np.int32)

    def _chest_cfgs(self, first_subframe, subframe_step):
        """the ports' estimation configurations (element stride nb_rx subframes), created once and owned"""
        key = (first_subframe, subframe_step)
        if key not in self._chest:
            cfgs = []
            for p in range(self._n_ports):
                cfgs.append(self._own(self.L.oai4g_chest_config_create(ctypes.byref(self.fp), p, *key),
                                      self.L.oai4g_chest_config_destroy))
                _check(self.L.oai4g_chest_config_set_stride(cfgs[p], self.nb_rx, self.nb_rx) == 0)
            self._chest[key] = cfgs
        return self._chest[key]

    def _estimate(self, batch, d_rxF, d_planes, plane, first_subframe, subframe_step, stream):
        """batch (oai4g_chest_batch or _pilots) per (port, antenna) over the FEP output [n + 1][nb_rx][nsymb][N]
        (the extra element's symbol 0 closes the last subframe's rows 12 / 13) into d_planes [2 p + a][plane]"""
        grid = self.fp.symbols_per_tti * self.fp.ofdm_symbol_size
        for p, cfg in enumerate(self._chest_cfgs(first_subframe, subframe_step)):
            for a in range(self.nb_rx):
                _check(batch(cfg, self._n_est, ctypes.c_void_p(d_rxF + a * grid * 4),
                             ctypes.c_void_p(d_planes + (2 * p + a) * plane * 4), stream) == 0)


class _RxBatchDual(_EstPlanes):
    """Device-resident batched demodulation of a two-port mode: the FEP output of nb_rx antennas and the
    four estimate planes (ports 0 / 1 per antenna, the shared code of _EstPlanes), or the pilot rows, to LLRs.
    A subclass creates its configuration and names its batch entry points (_pilots None: estimate planes only)."""
    _batch = _pilots = None

    def _setup(self, create, fp, rb_alloc, args, n_sf, nb_rx):
        """create(fp, rb_alloc, *args) is the configuration; then the device buffers of n_sf subframes"""
        self.L = init()
        self.cfg = self._own(getattr(self.L, create)(ctypes.byref(fp), (ctypes.c_uint32 * 4)(*rb_alloc), *args),
                             self.L.oai4g_rx_config_destroy)
        self.fp, self.n_sf, self.nb_rx = fp, n_sf, nb_rx
        self.stride = self.L.oai4g_rx_llr_stride(self.cfg)
        self._est_setup(n_sf, 2)
        self.d_llr = self._dev(n_sf * self.stride * 2)
        self.d_llr1 = self.d_pil = None

    def llr_count(self, sfi):
        return self.L.oai4g_rx_llr_count(self.cfg, sfi)

    def estimate(self, d_rxF, first_subframe=0, subframe_step=1, stream=None):
        """The four channel-estimation batches over the FEP output [n_sf + 1][nb_rx][nsymb][N]."""
        self._estimate(self.L.oai4g_chest_batch, d_rxF, self.d_est, self.plane, first_subframe, subframe_step, stream)

    def launch(self, d_rxF, unscramble=1, stream=None):
        _check(getattr(self.L, self._batch)(self.cfg, self.n_sf, d_rxF, self.d_est, self.d_llr, unscramble, stream) == 0)

    def _pil(self):
        if not self.d_pil:
            self.pil_plane = self.n_sf * 4 * self.fp.ofdm_symbol_size * 2
            self.d_pil = self._dev(4 * self.pil_plane * 4)
        return self.d_pil

    def _llr1(self):
        if not self.d_llr1:
            self.d_llr1 = self._dev(self.n_sf * self.stride * 2)
        return self.d_llr1

    def estimate_pilots(self, d_rxF, first_subframe=0, subframe_step=1, stream=None):
        """The four pilot-row estimations (oai4g_chest_batch_pilots): 5 rows per subframe instead of 14."""
        self._estimate(self.L.oai4g_chest_batch_pilots, d_rxF, self._pil(), self.pil_plane, first_subframe,
                       subframe_step, stream)

    def launch_pilots(self, d_rxF, unscramble=1, stream=None):
        """the demodulation from the pilot rows (estimate_pilots)"""
        if not self._pilots:
            raise RuntimeError(f"{type(self).__name__} demodulates from the estimate planes only")
        _check(getattr(self.L, self._pilots)(self.cfg, self.n_sf, d_rxF, self._pil(), self.d_llr, unscramble, stream) == 0)

    def llrs(self):
        return self._get(self.d_llr, (self.n_sf, self.stride), np.int16)


class RxBatchTM3(_RxBatchDual):
    """Device-resident batched TM3 demodulation (oai4g_rx_batch_tm3): codeword 0's LLRs; with both
    codewords QPSK launch_2cw / launch_2cw_pilots add codeword 1's (llrs1())."""
    _batch, _pilots = "oai4g_rx_batch_tm3", "oai4g_rx_batch_tm3_pilots"

    def __init__(self, fp, rb_alloc, Qm0, Qm1, mcs0, num_pdcch, rnti, n_sf, nb_rx=2, first_subframe=0,
                 subframe_step=1):
        self._setup("oai4g_rx_config_create_tm3", fp, rb_alloc,
                    (Qm0, Qm1, mcs0, num_pdcch, rnti, first_subframe, subframe_step, nb_rx), n_sf, nb_rx)

    def launch_2cw_pilots(self, d_rxF, unscramble=1, stream=None):
        _check(self.L.oai4g_rx_batch_tm3_2cw_pilots(self.cfg, self.n_sf, d_rxF, self._pil(), self.d_llr, self._llr1(),
                                                    unscramble, stream) == 0)

    def launch_2cw(self, d_rxF, unscramble=1, stream=None):
        """both codewords QPSK: codeword 0 into d_llr, codeword 1 into d_llr1 (llrs1())"""
        _check(self.L.oai4g_rx_batch_tm3_2cw(self.cfg, self.n_sf, d_rxF, self.d_est, self.d_llr, self._llr1(),
                                             unscramble, stream) == 0)

    def llrs1(self):
        return self._get(self.d_llr1, (self.n_sf, self.stride), np.int16)


class RxBatchTM2(_RxBatchDual):
    """Device-resident batched TM2 demodulation (oai4g_rx_batch_tm2): the ALAMOUTI-combined stream's LLRs."""
    _batch = "oai4g_rx_batch_tm2"

    def __init__(self, fp, rb_alloc, Qm, num_pdcch, rnti, n_sf, nb_rx=2, first_subframe=0, subframe_step=1):
        self._setup("oai4g_rx_config_create_tm2", fp, rb_alloc,
                    (Qm, num_pdcch, rnti, first_subframe, subframe_step, nb_rx), n_sf, nb_rx)


class RxBatchTM56(_RxBatchDual):
    """Device-resident batched TM4-6 demodulation (oai4g_rx_batch_tm56 / _tm56_pilots): the single-layer
    precoded codeword's LLRs."""
    _batch, _pilots = "oai4g_rx_batch_tm56", "oai4g_rx_batch_tm56_pilots"

    def __init__(self, fp, rb_alloc, Qm, mimo_mode, pmi_alloc, num_pdcch, rnti, n_sf, nb_rx=2, first_subframe=0,
                 subframe_step=1, pmi_rule=RX_PMI_UE, dl_power_off=1):
        self._setup("oai4g_rx_config_create_tm56", fp, rb_alloc, (Qm, mimo_mode, pmi_alloc, pmi_rule, dl_power_off,
                                                                  num_pdcch, rnti, first_subframe, subframe_step, nb_rx),
                    n_sf, nb_rx)


def dlsch_unscrambling(fp, rnti, G, llr, q, Ns, mbsfn_flag=0):
    """dlsch_unscrambling drop-in (in place on an int16 array of >= 32 (1 + G/32) entries)."""
    init()
    lib().oai4g_dlsch_unscrambling(ctypes.byref(fp), mbsfn_flag, rnti, G, _ptr(llr), q, Ns)
    return llr


def lte_dl_channel_estimation(fp, rxdataF, est, Ns, p, l, symbol):
    """lte_dl_channel_estimation drop-in (high_speed_flag 1): rxdataF / est int32 [nsymb*N]; est in place."""
    init()
    rxdataF = np.ascontiguousarray(rxdataF, dtype=np.int32)
    assert est.dtype == np.int32 and est.flags.c_contiguous
    _check(lib().oai4g_lte_dl_channel_estimation(ctypes.byref(fp), _ptr(rxdataF), _ptr(est), Ns, p, l, symbol) == 0)
    return est


def _plane_ptrs(planes):
    arr = (ctypes.c_void_p * 8)()
    for i, a in enumerate(planes):
        if a is not None:
            assert a.dtype == np.int32 and a.flags.c_contiguous
            arr[i] = a.ctypes.data
    return arr


def dl_ch_estimates_time(fp, nb_antennas_rx, planes, out_planes):
    """lte_dl_channel_estimation's idft tail (:704-738): out_planes[(p << 1) + aarx] = idft_N of the
    estimate plane from word 8 (scale 1), for every non-None plane; lists of 8 int32 arrays / None."""
    init()
    _check(lib().oai4g_dl_ch_estimates_time(ctypes.byref(fp), nb_antennas_rx, _plane_ptrs(planes),
                                             _plane_ptrs(out_planes)) == 0)
    return out_planes


def lte_est_freq_offset(planes, fp, l, freq_offset, reset=0):
    """lte_est_freq_offset drop-in: planes[0] = antenna 0's estimate plane (int32 [nsymb*N]);
    freq_offset = a ctypes.c_int updated in place (process-wide first_run, as the reference's static)."""
    init()
    _check(lib().oai4g_lte_est_freq_offset(_plane_ptrs(planes), ctypes.byref(fp), l, ctypes.byref(freq_offset),
                                            reset) == 0)
    return freq_offset.value


def freq_offset_update(fp, omega, freq_offset, first_run):
    """The scalar tail of one lte_est_freq_offset call (ctypes.c_int state in place)."""
    _check(lib().oai4g_freq_offset_update(ctypes.byref(fp), int(np.int32(omega)), ctypes.byref(freq_offset),
                                           ctypes.byref(first_run)) == 0)
    return freq_offset.value


def chest_dc_filters(k):
    """The 25-PRB DC-pair filters (filt24_k_dcr, filt24_(k+2)_dcl) of pilot offset k."""
    out = np.zeros((2, 24), dtype=np.int16)
    lib().oai4g_chest_dc_filters(k, _ptr(out))
    return out


def chest_filters(k):
    """The six filt96_32.h filters (fl, f2l2, f, f2, fr, f2r2) of pilot offset k, as the library builds them."""
    out = np.zeros((6, 24), dtype=np.int16)
    lib().oai4g_chest_filters(k, _ptr(out))
    return out


class _Scratch(_DeviceOwner):
    """a short-lived owner of one call's temporaries: `with _Scratch(L) as t` frees them when the call raises too"""

    def __init__(self, L):
        self.L = L


class ChestBatch(_DeviceOwner):
    """Device-resident batched channel estimation (oai4g_chest_batch) of n_sf consecutive subframes."""

    def __init__(self, fp, n_sf, p=0, first_subframe=0, subframe_step=1):
        self.L = init()
        self.cfg = self._own(self.L.oai4g_chest_config_create(ctypes.byref(fp), p, first_subframe, subframe_step),
                             self.L.oai4g_chest_config_destroy)
        self.fp, self.n_sf = fp, n_sf
        self.n_grid = n_sf * fp.symbols_per_tti * fp.ofdm_symbol_size
        self.d_rx = self._dev((self.n_grid + fp.ofdm_symbol_size) * 4)
        self.d_est = self._dev(self.n_grid * 4)

    def run(self, rxdataF, next_symbol0, d_rxdataF=None):
        """rxdataF [n_sf][nsymb*N] and the N words of the following subframe's symbol 0."""
        if d_rxdataF is None:
            y = np.concatenate([np.ascontiguousarray(rxdataF, dtype=np.int32).ravel(),
                                np.ascontiguousarray(next_symbol0, dtype=np.int32).ravel()])
            assert y.size == self.n_grid + self.fp.ofdm_symbol_size
            self._put(self.d_rx, y)
        self.launch(d_rxdataF or self.d_rx)
        return self._get(self.d_est, (self.n_sf, self.n_grid // self.n_sf), np.int32)

    def launch(self, d_rxdataF, stream=None):
        """Device-only: estimates of d_rxdataF (n_sf grids + the next symbol 0) into self.d_est."""
        _check(self.L.oai4g_chest_batch(self.cfg, self.n_sf, d_rxdataF, self.d_est, stream) == 0)

    def time_estimates(self, stream=None):
        """dl_ch_estimates_time of every subframe's estimate plane in self.d_est: [n_sf][N] int32."""
        N, stride = self.fp.ofdm_symbol_size, self.n_grid // self.n_sf
        with _Scratch(self.L) as t:
            d_t = t._dev(self.n_sf * N * 4)
            _check(self.L.oai4g_chest_time_batch(ctypes.byref(self.fp), self.n_sf, self.d_est, stride, d_t, N,
                                                 stream) == 0)
            return t._get(d_t, (self.n_sf, N), np.int32)

    def freq_offset_omegas(self, l, stream=None):
        """lte_est_freq_offset's integer part (omega, re | im << 16) of every subframe's plane."""
        with _Scratch(self.L) as t:
            d_o = t._dev(max(4, self.n_sf * 4))
            _check(self.L.oai4g_freq_offset_omega_batch(ctypes.byref(self.fp), self.n_sf, self.d_est,
                                                        self.n_grid // self.n_sf, l, d_o, stream) == 0)
            return t._get(d_o, self.n_sf, np.int32)


class RxBatch(_DeviceOwner):
    """Device-resident batched PDSCH demodulation (oai4g_rx_batch)."""

    def __init__(self, fp, rb_alloc, Qm, num_pdcch, rnti, n_sf, first_subframe=0, subframe_step=1):
        self.L = init()
        ra = (ctypes.c_uint32 * 4)(*rb_alloc)
        self.cfg = self._own(self.L.oai4g_rx_config_create(ctypes.byref(fp), ra, Qm, num_pdcch, rnti, first_subframe,
                                                           subframe_step), self.L.oai4g_rx_config_destroy)
        self.fp, self.n_sf = fp, n_sf
        self.stride = self.L.oai4g_rx_llr_stride(self.cfg)
        n_in = n_sf * fp.symbols_per_tti * fp.ofdm_symbol_size
        self.d_y = self._dev(n_in * 4)
        self.d_h = self._dev(n_in * 4)
        self.d_llr = self._dev(n_sf * self.stride * 2)

    def llr_count(self, sfi):
        return self.L.oai4g_rx_llr_count(self.cfg, sfi)

    def run(self, rxdataF, dl_ch, unscramble=1, d_rxdataF=None):
        if d_rxdataF is None:
            self._put(self.d_y, np.ascontiguousarray(rxdataF, dtype=np.int32))
        self._put(self.d_h, np.ascontiguousarray(dl_ch, dtype=np.int32))
        self.launch(d_rxdataF or self.d_y, self.d_h, unscramble)
        return self.llrs()

    def launch_estimated(self, chest, d_rxdataF, unscramble=1, stream=None):
        """Device-only, fused with the channel estimation of `chest` (a ChestBatch of the same
        subframes): LLRs of d_rxdataF into self.d_llr, no estimate buffer."""
        _check(self.L.oai4g_rx_batch_estimated(self.cfg, chest.cfg, self.n_sf, d_rxdataF, self.d_llr, unscramble,
                                               stream) == 0)

    def llrs(self):
        return self._get(self.d_llr, (self.n_sf, self.stride), np.int16)

    def launch(self, d_rxdataF, d_est, unscramble=1, stream=None):
        """Device-only: LLRs of d_rxdataF / d_est into self.d_llr."""
        _check(self.L.oai4g_rx_batch(self.cfg, self.n_sf, d_rxdataF, d_est, self.d_llr, unscramble, stream) == 0)


class FepBatch(_DeviceOwner):
    """Device-resident batched FEP (oai4g_fep_batch): n_sf subframes x n_ant antennas."""

    def __init__(self, fp, n_sf, n_ant):
        self.L = init()
        self.fp, self.n_sf, self.n_ant = fp, n_sf, n_ant
        self.n_in = n_sf * n_ant * fp.samples_per_tti
        self.n_out = n_sf * n_ant * fp.symbols_per_tti * fp.ofdm_symbol_size
        self.d_rx = self._dev(self.n_in * 4)
        self.d_rxF = self._dev(self.n_out * 4)

    def upload(self, rx):
        rx = np.ascontiguousarray(rx, dtype=np.int32)
        assert rx.size == self.n_in
        self._put(self.d_rx, rx)

    def run(self, stream=None):
        _check(self.L.oai4g_fep_batch(ctypes.byref(self.fp), self.n_sf, self.n_ant, self.d_rx, self.d_rxF,
                                      stream) == 0)

    def result(self):
        return self._get(self.d_rxF, (self.n_sf, self.n_ant, self.fp.symbols_per_tti, self.fp.ofdm_symbol_size), np.int32)


def ofdm_mod(grid, log2n, nb_symbols, cp):
    """PHY_ofdm_mod (CYCLIC_PREFIX): grid int32[nb_symbols*N] -> int32[nb_symbols*(N+cp)]."""
    init()
    grid = np.ascontiguousarray(grid, dtype=np.int32)
    N = 1 << log2n
    out = np.zeros(nb_symbols * (N + cp), dtype=np.int32)
    lib().oai4g_PHY_ofdm_mod(_ptr(grid), _ptr(out), log2n, nb_symbols, cp, CYCLIC_PREFIX)
    return out


def generate_pilots(grids, amp, fp, ntti=10):
    """generate_pilots (pilots.c:43): CRS into the frame grids (list of int32 arrays, in place)."""
    init()
    ptrs = (ctypes.c_void_p * 2)(*[g.ctypes.data for g in grids] + [None] * (2 - len(grids)))
    lib().oai4g_generate_pilots(ptrs, amp, ctypes.byref(fp), ntti)
    return grids


def lte_dl_cell_spec(symbol, amp, fp, Ns, l, p):
    """lte_dl_cell_spec (lte_dl_cell_spec.c:123): CRS into one OFDM symbol (int32 array, in place)."""
    init()
    _check(lib().oai4g_lte_dl_cell_spec(_ptr(symbol), amp, ctypes.byref(fp), Ns, l, p) == 0)
    return symbol


def turbo_decoder16(y, n, max_iterations=8, crc_type=0, F=0):
    """phy_threegpplte_turbo_decoder16: y = 3n+12 int16 LLRs.  Returns (iterations, decoded bytes)."""
    init()
    y = np.ascontiguousarray(y, dtype=np.int16)
    out = np.zeros(n // 8, dtype=np.uint8)
    it = lib().oai4g_phy_threegpplte_turbo_decoder16(_ptr(y), _ptr(out), n, 0, 0, max_iterations, crc_type, F)
    _check(it != 255)
    return it, out


def rate_matching_turbo_rx(RTC, G, w, dummy_w, soft, C, r, Qm, rvidx=0, clear=1, Nl=1, Kmimo=1, Mdlharq=8,
                           Nsoft=1827072):
    """lte_rate_matching_turbo_rx (in place on w int16).  Returns E."""
    init()
    E = ctypes.c_uint32()
    soft = np.ascontiguousarray(soft, dtype=np.int16)
    _check(lib().oai4g_lte_rate_matching_turbo_rx(RTC, G, _ptr(w), _ptr(dummy_w), _ptr(soft), C, Nsoft, Mdlharq,
                                                  Kmimo, rvidx, clear, Qm, Nl, r, ctypes.byref(E)) == 0)
    return E.value


def sub_block_deinterleaving_turbo(D, w):
    """sub_block_deinterleaving_turbo: returns the d buffer (96 + 3D + 8 int16, d = buf[96:])."""
    init()
    buf = np.zeros(96 + 3 * D + 8, dtype=np.int16)
    lib().oai4g_sub_block_deinterleaving_turbo(D, ctypes.c_void_p(buf.ctypes.data + 2 * 96),
                                               _ptr(np.ascontiguousarray(w, dtype=np.int16)))
    return buf


def turbo_decoder8(y, n, max_iterations=8, crc_type=0, F=0):
    """phy_threegpplte_turbo_decoder8 drop-in: y = 3n+12 int16 LLRs.  Returns (iterations, bytes)."""
    init()
    y = np.ascontiguousarray(y, dtype=np.int16)
    out = np.zeros(n // 8, dtype=np.uint8)
    it = lib().oai4g_phy_threegpplte_turbo_decoder8(_ptr(y), _ptr(out), n, 0, 0, max_iterations, crc_type, F)
    _check(it != 255)
    return it, out


def viterbi_lte(y, n, decoded=None):
    """phy_viterbi_lte_sse2 drop-in: y = 3n int8 soft bits, the decoded bits are added into `decoded`
    (zeros when not given).  Returns (1 if an input had to be clamped to [-8, 7] else 0, decoded bytes)."""
    y = np.ascontiguousarray(y, dtype=np.int8)
    out = np.zeros((n + 7) >> 3, dtype=np.uint8) if decoded is None else decoded
    r = lib().oai4g_phy_viterbi_lte(_ptr(y), _ptr(out), n)
    _check(r >= 0)
    return r, out


def viterbi_lte_state(y, n):
    """The same decode with its final state: (clamped, decoded bytes, 64 final metrics, start state)."""
    y = np.ascontiguousarray(y, dtype=np.int8)
    out = np.zeros((n + 7) >> 3, dtype=np.uint8)
    met = np.zeros(64, dtype=np.uint8)
    st = ctypes.c_uint8()
    r = lib().oai4g_diag_viterbi_lte(_ptr(y), n, _ptr(out), _ptr(met), ctypes.byref(st))
    _check(r >= 0)
    return r, out, met, st.value


def cc_rx_plan(D):
    """oai4g_cc_rx_plan: uint16[3 D], the first e index summed into every Viterbi input."""
    plan = np.zeros(3 * D, dtype=np.uint16)
    _check(lib().oai4g_cc_rx_plan(D, _ptr(plan)) == 3 * D)
    return plan


def dci_decoding(dci_length, L, e):
    """dci_decoding drop-in: e = 72 << L int8 soft bits.  Returns (the 2 + ((16 + dci_length) >> 3)
    decoded bytes, crc16 ^ the received CRC: the RNTI of a match)."""
    e = np.ascontiguousarray(e, dtype=np.int8)
    out = np.full(2 + ((16 + dci_length) >> 3), 0xA5, dtype=np.uint8)
    crc = ctypes.c_uint16()
    _check(lib().oai4g_dci_decoding_crc(dci_length, L, _ptr(e), _ptr(out), ctypes.byref(crc)) == 0)
    return out, crc.value


def pbch_decode(llr, fp, frame_mod4):
    """rx_pbch from the quantised soft bits on: llr = pbch_E int8.  Returns (1 / 2 / 4 eNB antennas or -1
    when the CRC matches none, the three MIB bytes); a refused call raises."""
    llr = np.ascontiguousarray(llr, dtype=np.int8)
    out = np.zeros(3, dtype=np.uint8)
    r = lib().oai4g_pbch_decode(_ptr(llr), ctypes.byref(fp), frame_mod4, _ptr(out))
    _check(r >= 0 or not lib().oai4g_last_error())
    return r, bytes(out)


class PbchDecodeBatch(_DeviceOwner):
    """Device-resident batch of n PBCH decodes (oai4g_pbch_decode_batch)."""

    def __init__(self, fp, n):
        self.L, self.fp, self.n = init(), fp, n
        self.E = 1920 if fp.Ncp == 0 else 1728
        self.d_llr = self._dev(n * self.E)
        self.d_q = self._dev(n)
        self.d_out = self._dev(4 * n)

    def upload(self, llr, frame_mod4):
        self._put(self.d_llr, np.ascontiguousarray(llr, dtype=np.int8).reshape(self.n, self.E))
        self._put(self.d_q, np.ascontiguousarray(frame_mod4, dtype=np.uint8).reshape(self.n))

    def launch(self, stream=None):
        _check(self.L.oai4g_pbch_decode_batch(self.d_llr, self.n, ctypes.byref(self.fp), self.d_q, self.d_out,
                                              stream) == 0)

    def results(self):
        """(antenna counts int16[n] with -1 for none, MIB bytes uint8[n][3])"""
        out = self._get(self.d_out, (self.n, 4), np.uint8)
        cnt = out[:, 3].astype(np.int16)
        cnt[cnt == 0xFF] = -1
        return cnt, out[:, :3].copy()


def pdcch_soft_bit_table(fp, subframe, num_pdcch):
    """oai4g_pdcch_soft_bit_table: uint32 per soft bit of e_rx (int16 index into comp | negate << 31,
    0xFFFFFFFF: nothing mapped)."""
    tab = np.zeros(8 * 800, dtype=np.uint32)
    n = lib().oai4g_pdcch_soft_bit_table(ctypes.byref(fp), subframe, num_pdcch, _ptr(tab), len(tab))
    _check(n >= 0)
    return tab[:n].copy()


def pdcch_soft_bits(comp, fp, subframe, num_pdcch):
    """rx_pdcch after compensation: comp = int32[num_pdcch * 12 * N_RB_DL] -> e_rx int8[8 * Mquad]."""
    comp = np.ascontiguousarray(comp, dtype=np.int32)
    e = np.zeros(8 * 800, dtype=np.int8)
    n = lib().oai4g_pdcch_soft_bits(_ptr(comp), ctypes.byref(fp), subframe, num_pdcch, _ptr(e))
    _check(n >= 0)
    return e[:n].copy()


def pdcch_candidates(fp, num_pdcch, subframe, crnti, do_common, L):
    """CCEind of the candidates of one dci_decoding_procedure0 call, in its order."""
    cce = np.zeros(16, dtype=np.uint16)
    n = lib().oai4g_pdcch_candidates(ctypes.byref(fp), num_pdcch, subframe, crnti, do_common, L, _ptr(cce), 16)
    _check(n >= 0)
    return cce[:n].tolist()


class PdcchPlan(ctypes.Structure):
    """oai4g_pdcch_plan_t: one dci_decoding_procedure0 call"""
    _fields_ = [(n, ctypes.c_uint8) for n in ("do_common", "L", "sizeof_bits", "sizeof_bytes", "format_si", "format_ra",
                                              "format_c", "stop_if_found")]


class PdcchRxResult(ctypes.Structure):
    _fields_ = [("dci_cnt", ctypes.c_uint8), ("format0_found", ctypes.c_uint8), ("format_c_found", ctypes.c_uint8),
                ("overflow", ctypes.c_uint8), ("nCCE", ctypes.c_int32), ("CCEmap", ctypes.c_uint32 * 3),
                ("dci", DciAlloc * 8)]


class DciSearchState:
    """the caller state of dci_decoding_procedure0: CCE maps, found flags, dci_cnt, nCCE[subframe]"""

    def __init__(self, n_alloc=16):
        self.alloc = (DciAlloc * n_alloc)()
        self.cnt, self.f0, self.fc, self.nCCE = ctypes.c_uint8(), ctypes.c_uint8(), ctypes.c_uint8(), ctypes.c_uint8(255)
        self.maps = [ctypes.c_uint32() for _ in range(3)]

    def found(self):
        return [(a.dci_length, a.L, a.nCCE, a.rnti, a.format, bytes(a.dci_pdu)) for a in self.alloc[:self.cnt.value]]


def dci_decoding_procedure0(state, e_rx, num_pdcch, crnti, do_common, subframe, fp, mi, si_rnti, ra_rnti, L, format_si,
                            format_ra, format_c, sizeof_bits, sizeof_bytes):
    """dci_decoding_procedure0 drop-in on a DciSearchState (updated in place)."""
    e_rx = np.ascontiguousarray(e_rx, dtype=np.int8)
    st = state
    _check(lib().oai4g_dci_decoding_procedure0(
        _ptr(e_rx), num_pdcch, crnti, ctypes.addressof(st.nCCE), do_common, subframe, ctypes.addressof(st.alloc),
        ctypes.byref(fp), mi, si_rnti, ra_rnti, L, format_si, format_ra, format_c, sizeof_bits, sizeof_bytes,
        ctypes.addressof(st.cnt), ctypes.addressof(st.f0), ctypes.addressof(st.fc), ctypes.addressof(st.maps[0]),
        ctypes.addressof(st.maps[1]), ctypes.addressof(st.maps[2])) == 0)


class PdcchRxBatch(_DeviceOwner):
    """Device-resident DCI search over n_sf subframes (oai4g_pdcch_rx_config_create / oai4g_pdcch_rx_batch).
    plan: a list of (do_common, L, sizeof_bits, sizeof_bytes, format_si, format_ra, format_c, stop_if_found)."""

    def __init__(self, fp, num_pdcch, crnti, si_rnti, ra_rnti, plan, n_sf):
        self.L, self.fp, self.n_sf, self.num_pdcch = init(), fp, n_sf, num_pdcch
        arr = (PdcchPlan * len(plan))(*[PdcchPlan(*p) for p in plan])
        self.cfg = self._own(self.L.oai4g_pdcch_rx_config_create(ctypes.byref(fp), num_pdcch, crnti, si_rnti, ra_rnti,
                                                                 arr, len(plan)), self.L.oai4g_pdcch_rx_config_destroy)
        self.comp_words = num_pdcch * 12 * fp.N_RB_DL
        self.d_comp = self._dev(n_sf * self.comp_words * 4)
        self.d_out = self._dev(n_sf * ctypes.sizeof(PdcchRxResult))

    def candidates(self, subframe):
        """[(CCEind, plan entry)] of a subframe index, in plan order"""
        cce = np.zeros(1024, dtype=np.uint16)
        pe = np.zeros(1024, dtype=np.uint8)
        n = self.L.oai4g_pdcch_rx_candidates(self.cfg, subframe, _ptr(cce), _ptr(pe), 1024)
        _check(n >= 0)
        return list(zip(cce[:n].tolist(), pe[:n].tolist()))

    def upload(self, comp):
        self._put(self.d_comp, np.ascontiguousarray(comp, dtype=np.int32).reshape(self.n_sf, self.comp_words))

    def launch(self, first_subframe=0, stream=None):
        _check(self.L.oai4g_pdcch_rx_batch(self.cfg, self.d_comp, self.n_sf, first_subframe, self.d_out, stream) == 0)

    def results(self):
        return self._get(self.d_out, self.n_sf, PdcchRxResult)


def _front_planes(fp, nb_rx, rxdataF, est):
    """the plane pointer arrays of the front-end drop-ins: rxdataF[a], est[(p, a)] -> (keep-alive, rx, est)"""
    keep = [np.ascontiguousarray(rxdataF[a], dtype=np.int32).ravel() for a in range(nb_rx)]
    rx = (ctypes.c_void_p * 2)(*[k.ctypes.data for k in keep])
    ep = (ctypes.c_void_p * 4)()
    for p in range(fp.nb_antennas_tx_eNB):
        for a in range(nb_rx):
            keep.append(np.ascontiguousarray(est[(p, a)], dtype=np.int32).ravel())
            ep[2 * p + a] = keep[-1].ctypes.data
    return keep, rx, ep


def rx_pdcch_front(fp, rxdataF, est, subframe, mimo_mode, high_speed_flag=1, diag=False):
    """oai4g_rx_pdcch_front: rxdataF[a] and est[(p, a)] (rows [nsymb][N]) -> (plane 0 of rxdataF_comp
    int32[36 N_RB_DL], log2_maxh, num_pdcch_symbols), and with diag the four planes before MRC [4][36 N_RB_DL]."""
    nb_rx = len(rxdataF)
    comp = np.zeros(36 * fp.N_RB_DL, dtype=np.int32)
    planes = np.zeros((4, 36 * fp.N_RB_DL), dtype=np.int32) if diag else None
    l2, n = ctypes.c_uint8(), ctypes.c_uint8()
    keep, rx, ep = _front_planes(fp, min(nb_rx, 2), rxdataF, est)
    _check(lib().oai4g_rx_pdcch_front(rx, ep, ctypes.byref(fp), nb_rx, subframe, mimo_mode, high_speed_flag, _ptr(comp),
                                      ctypes.byref(l2), ctypes.byref(n), _ptr(planes) if diag else None) == 0)
    return (comp, l2.value, n.value) + ((planes,) if diag else ())


def rx_pcfich(fp, subframe, comp, mimo_mode=0):
    """oai4g_rx_pcfich on plane 0 of rxdataF_comp: num_pdcch_symbols 1..3 (mimo_mode, as in the reference, does
    not enter the result)"""
    comp = np.ascontiguousarray(comp, dtype=np.int32)
    assert comp.size >= 8 * fp.N_RB_DL
    n = lib().oai4g_rx_pcfich(ctypes.byref(fp), subframe, _ptr(comp), mimo_mode)
    _check(n >= 0)
    return n


def rx_pdcch(fp, rxdataF, est, subframe, mimo_mode, high_speed_flag=1):
    """oai4g_rx_pdcch: (e_rx int8[8 Mquad], num_pdcch_symbols)"""
    nb_rx = len(rxdataF)
    e = np.zeros(8 * 800, dtype=np.int8)
    n = ctypes.c_uint8()
    keep, rx, ep = _front_planes(fp, min(nb_rx, 2), rxdataF, est)
    cnt = lib().oai4g_rx_pdcch(rx, ep, ctypes.byref(fp), nb_rx, subframe, mimo_mode, high_speed_flag, _ptr(e), ctypes.byref(n))
    _check(cnt >= 0)
    return e[:cnt].copy(), n.value


class PdcchFrontBatch(_EstPlanes):
    """Device-resident control front end of n_sf subframes (oai4g_pdcch_front_batch): the FEP output
    [n_sf (+ 1)][nb_rx][nsymb][N] and the estimate planes of ports x antennas -> d_comp [n_sf][36 N_RB_DL],
    d_cfi [n_sf], d_log2_maxh [n_sf].  estimate() runs the oai4g_chest_batch of every plane into the object's
    own buffers; launch() takes them or the caller's.  The planes and their estimation are _EstPlanes'."""

    def __init__(self, fp, n_sf, nb_rx, mimo_mode, high_speed_flag=1, first_subframe=0, subframe_step=1):
        self.L, self.fp, self.n_sf, self.nb_rx = init(), fp, n_sf, nb_rx
        self.first, self.step = first_subframe, subframe_step
        self.cfg = self._own(self.L.oai4g_pdcch_front_config_create(ctypes.byref(fp), nb_rx, mimo_mode, high_speed_flag,
                                                                    first_subframe, subframe_step),
                             self.L.oai4g_pdcch_front_config_destroy)
        self.words = 36 * fp.N_RB_DL
        self._est_setup(n_sf, fp.nb_antennas_tx_eNB)
        self.d_comp = self._dev(n_sf * self.words * 4)
        self.d_cfi = self._dev(max(4, n_sf))
        self.d_log2 = self._dev(max(4, n_sf))

    def estimate(self, d_rxF, stream=None):
        """oai4g_chest_batch per (port, antenna) over the FEP output [n_sf + 1][nb_rx][nsymb][N]"""
        self._estimate(self.L.oai4g_chest_batch, d_rxF, self.d_est, self.plane, self.first, self.step, stream)

    def launch(self, d_rxF, stream=None):
        ep = (ctypes.c_void_p * 4)(*[self.est_plane(i >> 1, i & 1).value for i in range(4)])
        _check(self.L.oai4g_pdcch_front_batch(self.cfg, self.n_sf, d_rxF, ep, self.d_comp, self.d_cfi, self.d_log2,
                                              stream) == 0)

    def results(self):
        """(comp int32 [n_sf][36 N_RB_DL], cfi uint8 [n_sf], log2_maxh uint8 [n_sf])"""
        return (self._get(self.d_comp, (self.n_sf, self.words), np.int32), self._get(self.d_cfi, self.n_sf, np.uint8),
                self._get(self.d_log2, self.n_sf, np.uint8))


class PdcchRxBatchDetected(_DeviceOwner):
    """The DCI search behind PdcchFrontBatch (oai4g_pdcch_rx_batch_detected): the three configurations of 1, 2
    and 3 control symbols; every subframe is searched under the one its device-resident count selects."""

    def __init__(self, fp, crnti, si_rnti, ra_rnti, plan, n_sf):
        self.L, self.fp, self.n_sf = init(), fp, n_sf
        self.by_count = [self._own(PdcchRxBatch(fp, n, crnti, si_rnti, ra_rnti, plan, 1)) for n in (1, 2, 3)]
        self.d_out = self._dev(n_sf * ctypes.sizeof(PdcchRxResult))

    def launch(self, d_comp, d_cfi, first_subframe=0, subframe_step=1, stream=None):
        cfgs = (ctypes.c_void_p * 3)(*[b.cfg for b in self.by_count])
        _check(self.L.oai4g_pdcch_rx_batch_detected(cfgs, d_comp, d_cfi, self.n_sf, first_subframe, subframe_step,
                                                    self.d_out, stream) == 0)

    def results(self):
        return self._get(self.d_out, self.n_sf, PdcchRxResult)


def _pbch_planes(nb_ports, nb_rx, rxdataF, est):
    keep = [np.ascontiguousarray(rxdataF[a], dtype=np.int32).ravel() for a in range(min(nb_rx, 2))]
    rx = (ctypes.c_void_p * 2)(*[k.ctypes.data for k in keep])
    ep = (ctypes.c_void_p * 4)()
    for p in range(min(nb_ports, 2)):
        for a in range(min(nb_rx, 2)):
            keep.append(np.ascontiguousarray(est[(p, a)], dtype=np.int32).ravel())
            ep[2 * p + a] = keep[-1].ctypes.data
    return keep, rx, ep


def rx_pbch_front(fp, rxdataF, est, nb_ports, mimo_mode, high_speed_flag=1, diag=False):
    """oai4g_rx_pbch_front: rxdataF[a] and est[(p, a)] (rows [nsymb][N] of subframe 0) -> (plane 0 of rxdataF_comp
    int32[288], log2_maxh uint8[4], the 480 soft bits int8), and with diag the four planes before MRC [4][288]."""
    nb_rx = len(rxdataF)
    comp = np.zeros(288, dtype=np.int32)
    l2 = np.zeros(4, dtype=np.uint8)
    llr = np.zeros(480, dtype=np.int8)
    planes = np.zeros((4, 288), dtype=np.int32) if diag else None
    keep, rx, ep = _pbch_planes(nb_ports, nb_rx, rxdataF, est)
    _check(lib().oai4g_rx_pbch_front(rx, ep, ctypes.byref(fp), nb_rx, nb_ports, mimo_mode, high_speed_flag, _ptr(comp),
                                     _ptr(l2), _ptr(llr), _ptr(planes) if diag else None) == 0)
    return (comp, l2, llr) + ((planes,) if diag else ())


def rx_pbch(fp, rxdataF, est, nb_ports, mimo_mode, frame_mod4, high_speed_flag=1):
    """oai4g_rx_pbch: (1 / 2 / 4 eNB antennas or -1 when the CRC matches none, the three MIB bytes); a refused
    call raises."""
    nb_rx = len(rxdataF)
    out = np.zeros(3, dtype=np.uint8)
    keep, rx, ep = _pbch_planes(nb_ports, nb_rx, rxdataF, est)
    r = lib().oai4g_rx_pbch(rx, ep, ctypes.byref(fp), nb_rx, nb_ports, mimo_mode, high_speed_flag, frame_mod4, _ptr(out))
    _check(r >= 0 or not lib().oai4g_last_error())
    return r, bytes(out)


class PbchDetect(ctypes.Structure):
    _fields_ = [("tx_ant", ctypes.c_uint8), ("frame_mod4", ctypes.c_uint8), ("mimo_mode", ctypes.c_uint8),
                ("mib", ctypes.c_uint8 * 3), ("pad", ctypes.c_uint8 * 2)]


class PbchFrontBatch(_EstPlanes):
    """Device-resident PBCH front end and detection of n subframes 0 (oai4g_pbch_front_batch,
    oai4g_pbch_detect_batch): the FEP output [n (+ 1)][nb_rx][nsymb][N] and the estimate planes of ports x antennas
    -> d_llr [n][2][480], d_log2 [n][4], d_out [n] PbchDetect.  The planes and their estimation are _EstPlanes'."""

    def __init__(self, fp, n, nb_rx, nb_ports, high_speed_flag=1, first_subframe=0, subframe_step=0):
        self.L, self.fp, self.n, self.nb_rx, self.nb_ports = init(), fp, n, nb_rx, nb_ports
        self.first, self.step = first_subframe, subframe_step
        self.cfg = self._own(self.L.oai4g_pbch_front_config_create(ctypes.byref(fp), nb_rx, nb_ports, high_speed_flag),
                             self.L.oai4g_pbch_front_config_destroy)
        self._est_setup(n, nb_ports)
        self.d_llr = self._dev(n * 960)
        self.d_log2 = self._dev(n * 4)
        self.d_out = self._dev(n * ctypes.sizeof(PbchDetect))

    def upload_llr(self, llr):
        """the soft bits themselves, int8 [n][2][480] (the detection alone)"""
        llr = np.ascontiguousarray(llr, dtype=np.int8)
        assert llr.size == self.n * 960
        self._put(self.d_llr, llr)

    def estimate(self, d_rxF, stream=None):
        """oai4g_chest_batch per (port, antenna) over the FEP output [n + 1][nb_rx][nsymb][N]"""
        self._estimate(self.L.oai4g_chest_batch, d_rxF, self.d_est, self.plane, self.first, self.step, stream)

    def launch(self, d_rxF, stream=None):
        ep = (ctypes.c_void_p * 4)(*[self.est_plane(i >> 1, i & 1).value for i in range(4)])
        _check(self.L.oai4g_pbch_front_batch(self.cfg, self.n, d_rxF, ep, self.d_llr, self.d_log2, stream) == 0)

    def detect(self, stream=None):
        _check(self.L.oai4g_pbch_detect_batch(self.cfg, self.n, self.d_llr, self.d_out, stream) == 0)

    def results(self):
        """(llr int8 [n][2][480], log2_maxh uint8 [n][4])"""
        return self._get(self.d_llr, (self.n, 2, 480), np.int8), self._get(self.d_log2, (self.n, 4), np.uint8)

    def estimates(self):
        """est[(p, a)] = int32 [n][nsymb * N] as they stand on the device"""
        planes = super().estimates()
        return {(p, a): planes[2 * p + a] for p in range(self.nb_ports) for a in range(self.nb_rx)}

    def detected(self):
        return self._get(self.d_out, self.n, PbchDetect)


def lte_sync_time_replicas(fp):
    """oai4g_lte_sync_time_replicas: lte_sync_time_init's three time-domain PSS replicas, int16 [3][N][2].  Host only."""
    out = np.zeros((3, fp.ofdm_symbol_size, 2), dtype=np.int16)
    _check(lib().oai4g_lte_sync_time_replicas(ctypes.byref(fp), _ptr(out)) == 0)
    return out


def lte_sync_time(rxdata, fp, want_corr=False):
    """oai4g_lte_sync_time on one frame: rxdata[a] int32 [10 samples_per_tti] -> (peak_pos, Nid2, peak_val), and
    with want_corr the three correlation buffers int32 [3][10 samples_per_tti] (every fourth entry is defined)."""
    init()
    fl = 10 * fp.samples_per_tti
    keep = [np.ascontiguousarray(a, dtype=np.int32).ravel() for a in rxdata]
    assert all(a.size == fl for a in keep)
    rx = (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    corr = np.zeros((3, fl), dtype=np.int32) if want_corr else None
    src, val = ctypes.c_int(-1), ctypes.c_uint32(0)
    pos = lib().oai4g_lte_sync_time(rx, ctypes.byref(fp), len(keep), ctypes.byref(src), ctypes.byref(val),
                                    _ptr(corr) if want_corr else None)
    _check(pos >= 0)
    return (pos, src.value, val.value) + ((corr,) if want_corr else ())


def rx_sss(rxdata, fp, Nid2, rx_offset):
    """oai4g_rx_sss on one frame: rxdata[a] int32 [10 samples_per_tti] -> (Nid_cell, tot_metric, flip_max, phase_max)"""
    init()
    keep = [np.ascontiguousarray(a, dtype=np.int32).ravel() for a in rxdata]
    assert all(a.size == 10 * fp.samples_per_tti for a in keep)
    rx = (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    metric, flip, phase = ctypes.c_int32(0), ctypes.c_uint8(0), ctypes.c_uint8(0)
    nid = lib().oai4g_rx_sss(rx, ctypes.byref(fp), len(keep), Nid2, rx_offset, ctypes.byref(metric), ctypes.byref(flip),
                             ctypes.byref(phase))
    _check(nid >= 0)
    return nid, metric.value, flip.value, phase.value


class InitialSync(ctypes.Structure):
    """oai4g_initial_sync_t"""
    _fields_ = [("Nid_cell", ctypes.c_int32), ("rx_offset", ctypes.c_int32), ("tx_ant", ctypes.c_uint8),
                ("frame_mod4", ctypes.c_uint8), ("mimo_mode", ctypes.c_uint8), ("mib", ctypes.c_uint8 * 3),
                ("pad", ctypes.c_uint8 * 2)]


def initial_sync(rxdata, fp, nb_ports=2, high_speed_flag=1):
    """oai4g_initial_sync on one frame: (0 or -1 when no PBCH was found, the InitialSync record); a refused call
    raises."""
    init()
    keep = [np.ascontiguousarray(a, dtype=np.int32).ravel() for a in rxdata]
    assert all(a.size == 10 * fp.samples_per_tti for a in keep)
    rx = (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    out = InitialSync()
    r = lib().oai4g_initial_sync(rx, ctypes.byref(fp), len(keep), nb_ports, high_speed_flag, ctypes.byref(out))
    err = lib().oai4g_last_error()
    _check(r == 0 or not err or b"SSS error condition" in err)
    return r, out


# ------------------------------------------------------------------------------------------
# fading channels (SIMULATION/TOOLS/random_channel.c, multipath_channel.c)
# ------------------------------------------------------------------------------------------
CHANNEL_MAX_TAPS = 9
# SCM_t (SIMULATION/TOOLS/defs.h:158-178), the supported ones; dlsim's -g letters map to these
(EPA, EVA, ETU, Rayleigh8, Rayleigh1, Rayleigh1_800, Rayleigh1_corr, Rayleigh1_anticorr, Rice8, Rice1, Rice1_corr,
 Rice1_anticorr, AWGN) = 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18


class ChannelInfo(ctypes.Structure):
    """oai4g_channel_info_t"""
    _fields_ = [("nb_taps", ctypes.c_uint32), ("channel_length", ctypes.c_uint32), ("random_aoa", ctypes.c_uint32),
                ("n_matrices", ctypes.c_uint32), ("ricean_factor", ctypes.c_double), ("aoa", ctypes.c_double),
                ("amps", ctypes.c_double * CHANNEL_MAX_TAPS), ("delays", ctypes.c_double * CHANNEL_MAX_TAPS)]


def _r_sqrt(raw, info, n):
    return (raw[:info.n_matrices * n * n * 2].reshape(info.n_matrices, n, n, 2) @ np.array([1, 1j])).copy()


def channel_model_describe(model, nb_tx, nb_rx, BW):
    """oai4g_channel_model_describe: (ChannelInfo, R_sqrt complex [n_matrices][npair][npair]) of a model.  Host only."""
    info, raw = ChannelInfo(), np.zeros(6 * 16 * 2)
    _check(lib().oai4g_channel_model_describe(model, nb_tx, nb_rx, BW, ctypes.byref(info), _ptr(raw)) == 0)
    return info, _r_sqrt(raw, info, nb_tx * nb_rx)


class _ChannelBatch(_DeviceOwner):
    """Fading channel of n_vectors trials on the device (oai4g_channel_config_create): every vector has its own
    descriptor state.  Public as ChannelBatch.  draw() is random_channel of the vectors, run() multipath_channel on their taps plus dlsim's
    noise; taps() / set_taps() move a and ch between host and device as complex arrays a [n][nb_taps][npair] and
    ch [n][npair][channel_length], pair index aarx + aatx nb_rx."""

    def __init__(self, nb_tx, nb_rx, model, BW, n_vectors, forgetting_factor=0.0, channel_offset=0, path_loss_dB=0.0):
        self.L = init()
        self.nb_tx, self.nb_rx, self.n, self.npair = nb_tx, nb_rx, n_vectors, nb_tx * nb_rx
        self.cfg = self._own(self.L.oai4g_channel_config_create(nb_tx, nb_rx, model, BW, forgetting_factor, channel_offset,
                                                                path_loss_dB, n_vectors),
                             self.L.oai4g_channel_config_destroy)
        self.info, raw = ChannelInfo(), np.zeros(6 * 16 * 2)
        _check(self.L.oai4g_channel_config_query(self.cfg, ctypes.byref(self.info), _ptr(raw)) == 0)
        self.R_sqrt = _r_sqrt(raw, self.info, self.npair)
        self.nb_taps, self.channel_length = self.info.nb_taps, self.info.channel_length
        angles = self.info.ricean_factor != 1.0 and self.info.random_aoa == 1
        self.draws_per_vector = self.nb_taps * self.npair * 2 + (self.npair if angles else 0)
        self.d_draws = None

    def draw(self, seed=0, first_vector=0, step=0, n=None, draws=None, stream=None):
        """a new channel for vectors [0, n): Philox draws keyed by (seed, first_vector + vector, step), or the given
        float64 [n][draws_per_vector] in the reference's draw order"""
        n = self.n if n is None else n
        d = None
        if draws is not None:
            draws = np.ascontiguousarray(draws, dtype=np.float64)
            assert draws.size == n * self.draws_per_vector
            if self.d_draws is None:
                self.d_draws = self._dev(self.n * self.draws_per_vector * 8)
            self._put(self.d_draws, draws)
            d = self.d_draws
        _check(self.L.oai4g_channel_random_batch(self.cfg, n, seed, first_vector, step, d, stream) == 0)

    def run(self, d_tx, tx_stride, tx_ant_stride, tx_len, d_tail, tail_len, d_rx, rx_stride, rx_ant_stride, seg_len,
            seg_stride, d_tx_lev, offset_db, seed, first_vector=0, n=None, stream=None):
        """oai4g_multipath_batch on the vectors' current taps"""
        _check(self.L.oai4g_multipath_batch(self.cfg, self.n if n is None else n, d_tx, tx_stride, tx_ant_stride, tx_len,
                                            d_tail, tail_len, d_rx, rx_stride, rx_ant_stride, seg_len, seg_stride, d_tx_lev,
                                            offset_db, seed, first_vector, stream) == 0)

    def taps(self, first_vector=0, n=None):
        """(a, ch) of vectors [first_vector, +n) (synchronises)"""
        n = self.n - first_vector if n is None else n
        a = np.zeros((n, self.nb_taps, self.npair, 2))
        ch = np.zeros((n, self.npair, self.channel_length, 2))
        _check(self.L.oai4g_channel_get_taps(self.cfg, first_vector, n, _ptr(ch), _ptr(a)) == 0)
        return a[..., 0] + 1j * a[..., 1], ch[..., 0] + 1j * ch[..., 1]

    def set_taps(self, ch=None, a=None, first_vector=0):
        """complex ch [n][npair][channel_length] and / or a [n][nb_taps][npair] into vectors [first_vector, +n)"""
        def pairs(v, shape):
            v = np.asarray(v, dtype=np.complex128).reshape((-1,) + shape)
            return np.ascontiguousarray(np.stack([v.real, v.imag], axis=-1))
        hc = None if ch is None else pairs(ch, (self.npair, self.channel_length))
        ha = None if a is None else pairs(a, (self.nb_taps, self.npair))
        n = len(hc if hc is not None else ha)
        assert ha is None or hc is None or len(ha) == len(hc)
        _check(self.L.oai4g_channel_set_taps(self.cfg, first_vector, n, None if hc is None else _ptr(hc),
                                             None if ha is None else _ptr(ha)) == 0)


ChannelBatch = _ChannelBatch


def random_channel(chan):
    """oai4g_random_channel: the drop-in on vector 0 of a ChannelBatch"""
    _check(chan.L.oai4g_random_channel(chan.cfg) == 0)


def multipath_channel(chan, tx_re, tx_im, length=None, keep_channel=1, rx_re=None, rx_im=None):
    """oai4g_multipath_channel on vector 0 of a ChannelBatch: tx_re / tx_im float64 [nb_tx][length] -> (rx_re, rx_im)
    float64 [nb_rx][length]; samples [0, |channel_offset|) keep what rx_re / rx_im held (NaN when not given)"""
    tx = [np.ascontiguousarray(v, dtype=np.float64) for v in list(tx_re) + list(tx_im)]
    length = tx[0].size if length is None else length
    assert len(tx) == 2 * chan.nb_tx and all(v.size >= length for v in tx)
    rx = [np.full(length, np.nan) if v is None else v for v in
          ([None] * (2 * chan.nb_rx) if rx_re is None else list(rx_re) + list(rx_im))]
    pp = [(ctypes.c_void_p * len(v))(*[a.ctypes.data for a in v])
          for v in (tx[:chan.nb_tx], tx[chan.nb_tx:], rx[:chan.nb_rx], rx[chan.nb_rx:])]
    _check(chan.L.oai4g_multipath_channel(chan.cfg, *pp, length, keep_channel) == 0)
    return np.stack(rx[:chan.nb_rx]), np.stack(rx[chan.nb_rx:])


class Cell(ctypes.Structure):
    """oai4g_cell_t"""
    _fields_ = [(k, ctypes.c_int32) for k in ("Nid_cell", "rx_offset", "metric", "flip", "phase", "status")]


class _SyncBatch(_DeviceOwner):
    """Device-resident cell search of n frames: d_rx [n][nb_rx][10 samples_per_tti] -> d_peak [n] {peak_pos,
    peak_val, Nid2} (oai4g_sync_time_batch) -> d_cell [n] Cell (oai4g_sss_batch); d_corr [n][3][10 samples_per_tti]
    exists once a launch asked for it.  fep() is oai4g_fep_offset_batch of these frames at the offsets in d_cell.
    Handed out by sync_batch()."""

    def __init__(self, fp, n, nb_rx):
        self.L, self.fp, self.n, self.nb_rx = init(), fp, n, nb_rx
        self.frame = 10 * fp.samples_per_tti
        self.cfg = self._own(self.L.oai4g_sync_config_create(ctypes.byref(fp), nb_rx), self.L.oai4g_sync_config_destroy)
        self.d_rx = self._dev(n * nb_rx * self.frame * 4)
        self.d_peak = self._dev(n * 12)
        self.d_cell = self._dev(n * ctypes.sizeof(Cell))
        self.d_corr = None

    def upload_peaks(self, peaks):
        """int32 [n][3] in place of the PSS stage's result"""
        peaks = np.ascontiguousarray(peaks, dtype=np.int32)
        assert peaks.size == 3 * self.n
        self._put(self.d_peak, peaks)

    def launch_sss(self, stream=None):
        _check(self.L.oai4g_sss_batch(self.cfg, self.n, self.d_rx, self.d_peak, self.d_cell, stream) == 0)

    def launch_sss_rows(self, d_rows, stream=None):
        """the SSS stage on given rows [n][nb_rx][4][N] in place of its own FEP (oai4g_sss_rows_batch)"""
        _check(self.L.oai4g_sss_rows_batch(self.cfg, self.n, d_rows, self.d_peak, self.d_cell, stream) == 0)

    def cells(self):
        return self._get(self.d_cell, self.n, Cell)

    def fep(self, d_rxF, first_slot, nsym, frames=None, frame_stride=0, stream=None):
        """the frames (all, or the listed ones in that order) at their rx_offset: rows of d_rxF + i * frame_stride"""
        runs = [(0, self.n)] if frames is None else [(f, 1) for f in frames]
        step = (frame_stride or self.nb_rx * self.fp.symbols_per_tti * self.fp.ofdm_symbol_size) * 4
        for i, (f, k) in enumerate(runs):
            _check(self.L.oai4g_fep_offset_batch(ctypes.byref(self.fp), k, self.nb_rx, self.d_rx + f * self.nb_rx * self.frame * 4,
                                                 self.d_cell + f * ctypes.sizeof(Cell) + 4, 6, first_slot, nsym,
                                                 d_rxF + i * step, frame_stride, stream) == 0)

    def upload(self, rx):
        """int32 [n][nb_rx][10 samples_per_tti]"""
        rx = np.ascontiguousarray(rx, dtype=np.int32)
        assert rx.size == self.n * self.nb_rx * self.frame
        self._put(self.d_rx, rx)

    def launch(self, want_corr=False, stream=None):
        if want_corr and self.d_corr is None:
            self.d_corr = self._dev(self.n * 3 * self.frame * 4)
        _check(self.L.oai4g_sync_time_batch(self.cfg, self.n, self.d_rx, self.d_peak,
                                            self.d_corr if want_corr else None, stream) == 0)

    def peaks(self):
        """int32 [n][3]: peak_pos, peak_val (the unsigned metric's bits), Nid2"""
        return self._get(self.d_peak, (self.n, 3), np.int32)

    def corr(self):
        return self._get(self.d_corr, (self.n, 3, self.frame), np.int32)


def sync_batch(fp, n, nb_rx):
    """the device-resident cell search of n frames of nb_rx antennas"""
    return _SyncBatch(fp, n, nb_rx)


def rx_phich(fp, subframe, comp, ngroup, nseq):
    """oai4g_rx_phich on plane 0 of the PDCCH front's rxdataF_comp: (1 NACK / 0 ACK, HI16)"""
    comp = np.ascontiguousarray(comp, dtype=np.int32)
    assert comp.size >= 8 * fp.N_RB_DL
    hi = ctypes.c_int16()
    r = lib().oai4g_rx_phich(ctypes.byref(fp), subframe, _ptr(comp), ngroup, nseq, ctypes.byref(hi))
    _check(r >= 0)
    return r, hi.value


class PhichRxItem(ctypes.Structure):
    _fields_ = [("slot", ctypes.c_uint32), ("ngroup", ctypes.c_uint8), ("nseq", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 2)]


class PhichRxOut(ctypes.Structure):
    _fields_ = [("HI16", ctypes.c_int16), ("nack", ctypes.c_uint8), ("pad", ctypes.c_uint8)]


class PhichRxBatch(_DeviceOwner):
    """oai4g_phich_rx_batch behind PdcchFrontBatch: items = [(slot, ngroup, nseq)] -> [(HI16, nack)]"""

    def __init__(self, fp, items, first_subframe=0, subframe_step=1):
        self.L, self.n_items = init(), len(items)
        self.cfg = self._own(self.L.oai4g_phich_rx_config_create(ctypes.byref(fp), first_subframe, subframe_step),
                             self.L.oai4g_phich_rx_config_destroy)
        arr = (PhichRxItem * max(1, len(items)))()
        for i, (slot, g, q) in enumerate(items):
            arr[i].slot, arr[i].ngroup, arr[i].nseq = slot, g, q
        self.d_items = self._dev(ctypes.sizeof(arr))
        self.d_out = self._dev(max(1, len(items)) * ctypes.sizeof(PhichRxOut))
        self._put(self.d_items, np.frombuffer(arr, dtype=np.uint8))

    def launch(self, d_comp, n_sf, stream=None):
        _check(self.L.oai4g_phich_rx_batch(self.cfg, d_comp, n_sf, self.d_items, self.n_items, self.d_out, stream) == 0)

    def results(self):
        out = self._get(self.d_out, max(1, self.n_items), PhichRxOut)
        return [(o.HI16, o.nack) for o in out[:self.n_items]]


def _upload_tiled(dec, base, chunk_bytes=64 << 20):
    """Block i of a decoder batch gets base[i % len(base)], without a host copy of the whole batch
    (the C5 bench's 393 216-block batch would be 13 GB): one host chunk of whole base periods,
    copied over the device LLR buffer piece by piece."""
    base = np.asarray(base, dtype=np.int16)
    nb = len(base)
    per = max(1, chunk_bytes // (nb * dec.llr_stride * 2)) * nb       # rows per chunk, a multiple of nb
    per = min(per, ((dec.n_cb + nb - 1) // nb) * nb)
    buf = np.zeros((per, dec.llr_stride), dtype=np.int16)
    buf[:, :base.shape[1]] = np.tile(base, (per // nb, 1))
    for r0 in range(0, dec.n_cb, per):
        dec._put(dec.d_llr + r0 * dec.llr_stride * 2, buf[:min(per, dec.n_cb - r0)])


class TurboDecoderBatch(_DeviceOwner):
    """Device-resident batch of n_cb code blocks of size K (oai4g_td_batch)."""
    # the entry point, its scratch-size function, the least size of d_it, and d_out zeroed at the start: the decoder
    # writes d_out only once a hard decision is made (iteration >= 2), as the reference leaves decoded_bytes
    # untouched at max_iterations = 1
    _entry, _scratch_bytes, _min_it, _zero_out = "oai4g_td_batch", "oai4g_td_scratch_bytes", 256, True

    def __init__(self, K, n_cb):
        self.L = init()
        self.K, self.n_cb = K, n_cb
        self.llr_stride = 3 * K + 16
        self._batch = getattr(self.L, self._entry)
        self.d_llr = self._dev(n_cb * self.llr_stride * 2)
        self.d_out = self._dev(n_cb * (K // 8), zero=self._zero_out)
        self.d_it = self._dev(max(self._min_it, n_cb))
        self.d_scr = self._dev(getattr(self.L, self._scratch_bytes)(K, n_cb))

    def upload(self, llr):
        buf = np.zeros((self.n_cb, self.llr_stride), dtype=np.int16)
        llr = np.asarray(llr, dtype=np.int16)
        buf[:, :llr.shape[-1]] = llr
        self._put(self.d_llr, buf)

    def upload_tiled(self, base):
        _upload_tiled(self, base)

    def run(self, max_iterations=8, crc_type=0, F=0, stream=None):
        _check(self._batch(self.n_cb, self.K, self.d_llr, self.llr_stride, self.d_out, self.K // 8,
                           self.d_it, max_iterations, crc_type, F, self.d_scr, stream) == 0)

    def results(self):
        out = self._get(self.d_out, (self.n_cb, self.K // 8), np.uint8)
        return self._get(self.d_it, self.n_cb, np.uint8), out


class TurboDecoder8Batch(TurboDecoderBatch):
    """Device-resident batch of n_cb blocks of size K through the 8-bit decoder (oai4g_td8_batch)."""
    _entry, _scratch_bytes, _min_it, _zero_out = "oai4g_td8_batch", "oai4g_td8_scratch_bytes", 0, False


def generate_dummy_w(D, F=0):
    """generate_dummy_w: the uint8 NULL-mark buffer (3 Kpi) of a block of D = K + 4 with F fillers."""
    R = (D + 31) >> 5
    w = np.zeros(3 * 32 * R + 64, dtype=np.uint8)
    lib().oai4g_generate_dummy_w(D, _ptr(w), F)
    return w


class UlDecodeBatch(_DeviceOwner):
    """Batched ulsch_decoding chain (oai4g_ul_decode_batch): n_tb transport blocks of B = TBS + 24
    bits, G soft bits each -> RM-rx + deinterleaving + 16-bit turbo decoding per code block."""

    def __init__(self, B, G, Qm, n_tb, rvidx=0, max_iterations=8, Mdlharq=8, Nsoft=1827072):
        self.L = init()
        self.cfg = self._own(self.L.oai4g_ul_config_create(B, G, Qm, rvidx, Mdlharq, Nsoft, max_iterations),
                             self.L.oai4g_ul_config_destroy)
        self.C = self.L.oai4g_ul_config_C(self.cfg)
        self.n_tb, self.G = n_tb, G
        self.e_stride = (G + 63) & ~63
        self.c_stride = 6144 // 8 + 8
        self.d_e = self._dev(n_tb * self.e_stride * 2)
        self.d_c = self._dev(n_tb * self.C * self.c_stride)
        self.d_it = self._dev(n_tb * self.C)
        self.d_w = self.d_rc = None

    def set_decoder(self, bits):
        """16: phy_threegpplte_turbo_decoder16 (the default); 8: the 8-bit decoder, for one block size
        K % 16 == 0, K >= 512 (raises otherwise).  The scratch is reallocated on the next launch."""
        _check(self.L.oai4g_ul_config_set_decoder(self.cfg, bits) == 0)

    def E(self, r):
        return self.L.oai4g_ul_config_E(self.cfg, r)

    def offset(self, r):
        return self.L.oai4g_ul_config_G_offset(self.cfg, r)

    def upload(self, e):
        buf = np.zeros((self.n_tb, self.e_stride), dtype=np.int16)
        buf[:, :self.G] = np.asarray(e, dtype=np.int16).reshape(self.n_tb, -1)[:, :self.G]
        self._put(self.d_e, buf)

    def launch(self, stream=None):
        _check(self.L.oai4g_ul_decode_batch(self.cfg, self.n_tb, self.d_e, self.e_stride, self.d_c, self.c_stride,
                                            self.d_it, stream) == 0)

    def launch_harq(self, rvidx, clear, stream=None):
        """One HARQ round (oai4g_ul_decode_batch_harq) on the uploaded soft bits: the per-block soft
        buffers (allocated zeroed on first use) combine this round's rvidx; clear = 1 on round 0."""
        self._alloc_w()
        _check(self.L.oai4g_ul_decode_batch_harq(self.cfg, self.n_tb, self.d_e, self.e_stride, self.d_w, self.w_stride,
                                                 rvidx, clear, self.d_c, self.c_stride, self.d_it, stream) == 0)

    def launch_harq_tb(self, rv, clear, stream=None):
        """One HARQ round with a redundancy version and a clear flag per transport block
        (oai4g_ul_decode_batch_harq_tb): rv, clear are [n_tb] arrays, uploaded here."""
        self._alloc_w()
        rc = np.ascontiguousarray(np.stack([np.asarray(rv, np.uint8).reshape(self.n_tb),
                                            np.asarray(clear, np.uint8).reshape(self.n_tb)]))
        if self.d_rc is None:
            self.d_rc = self._dev(rc.nbytes)
        self._put(self.d_rc, rc)
        _check(self.L.oai4g_ul_decode_batch_harq_tb(self.cfg, self.n_tb, self.d_e, self.e_stride, self.d_w,
                                                    self.w_stride, self.d_rc, self.d_rc + self.n_tb, self.d_c,
                                                    self.c_stride, self.d_it, stream) == 0)

    def _alloc_w(self):
        if self.d_w is None:
            self.w_stride = (self.L.oai4g_ul_config_w_entries(self.cfg) + 63) & ~63
            self.d_w = self._dev(self.n_tb * self.C * self.w_stride * 2, zero=True)

    def soft_buffers(self):
        """[n_tb][C][w_stride] int16 HARQ soft buffers (after launch_harq)."""
        return self._get(self.d_w, (self.n_tb, self.C, self.w_stride), np.int16)

    def results(self):
        c = self._get(self.d_c, (self.n_tb, self.C, self.c_stride), np.uint8)
        return self._get(self.d_it, (self.n_tb, self.C), np.uint8), c


def dci_allocs(items):
    """items: (dci_length, L, nCCE, rnti, pdu bytes) -> ctypes array of DciAlloc"""
    arr = (DciAlloc * max(1, len(items)))()
    for a, (ln, L, ncce, rnti, pdu) in zip(arr, items):
        a.dci_length, a.L, a.nCCE, a.rnti = ln, L, ncce, rnti
        for i, b in enumerate(list(pdu)[:8]):
            a.dci_pdu[i] = int(b)
    return arr


def generate_dci_top(items, n_common, amp, fp, txdataF, subframe):
    """generate_dci_top on frame grids (int32 arrays, modified in place): num_pdcch_symbols"""
    init()
    arr = dci_allocs(items)
    gp = (ctypes.c_void_p * len(txdataF))(*[g.ctypes.data for g in txdataF])
    return lib().oai4g_generate_dci_top(len(items) - n_common, n_common, arr, 0, amp, ctypes.byref(fp), gp, subframe)


def normal_prefix_mod(txdataF, fp, nsymb=7, out=None):
    init()
    txdataF = np.ascontiguousarray(txdataF, dtype=np.int32)
    if out is None:
        out = np.zeros(fp.samples_per_tti, dtype=np.int32)
    lib().oai4g_normal_prefix_mod(_ptr(txdataF), _ptr(out), nsymb, ctypes.byref(fp))
    return out


class DlschHandle(_DeviceOwner):
    """Owns an oai4g_dlsch_t (new_eNB_dlsch) and exposes its HARQ-0 buffers as numpy views."""

    def __init__(self, Kmimo=1, Mdlharq=8, N_RB_DL=100):
        self.L = init()
        self.ptr = self._own(self.L.oai4g_new_dlsch(Kmimo, Mdlharq, N_RB_DL), self.L.oai4g_free_dlsch)
        self.d = self.ptr.contents
        self.h = self.d.harq_processes[0].contents

    def close(self):
        """the views die with the structure: d, h and ptr are dropped with it"""
        super().close()
        self.ptr = self.d = self.h = None

    def view(self, field, n, r=None):
        p = getattr(self.h, field) if r is None else getattr(self.h, field)[r]
        return np.ctypeslib.as_array(p, shape=(n,))


def dlsch_encoding(a, fp, num_pdcch, dl, subframe):
    return lib().oai4g_dlsch_encoding(_ptr(a), ctypes.byref(fp), num_pdcch, dl.ptr, 0, subframe)


def dlsch_scrambling(fp, dl, G, q, Ns, mbsfn_flag=0):
    lib().oai4g_dlsch_scrambling(ctypes.byref(fp), mbsfn_flag, dl.ptr, G, q, Ns)


def dlsch_modulation(txdataF, amp, subframe, fp, num_pdcch, dl0, dl1=None):
    """txdataF: list of int32 arrays (one per antenna), modified in place."""
    arr = (ctypes.c_void_p * len(txdataF))(*[a.ctypes.data for a in txdataF])
    return lib().oai4g_dlsch_modulation(arr, amp, subframe, ctypes.byref(fp), num_pdcch, dl0.ptr,
                                        dl1.ptr if dl1 is not None else None)


# ------------------------------------------------------------------------------------------
# configurations (BASELINE.json configs) and the batched pipeline
# ------------------------------------------------------------------------------------------
FULL_ALLOC_100 = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xF)
FULL_ALLOC_6 = (0x3F, 0, 0, 0)
FULL_ALLOC_15 = (0x7FFF, 0, 0, 0)
FULL_ALLOC_50 = (0xFFFFFFFF, 0x3FFFF, 0, 0)
FULL_ALLOC_25 = (0x1FFFFFF, 0, 0, 0)

def get_pmi(N_RB_DL, mimo_mode, pmi_alloc, rb):
    """get_pmi (dlsch_modulation.c:1136): the precoder index of resource block rb (host-side)."""
    return lib().oai4g_get_pmi(N_RB_DL, mimo_mode, pmi_alloc, rb)


def get_TBS_DL(mcs, nb_rb):
    """get_TBS_DL (lte_mcs.c:118): transport block size in BYTES, from the library's TBStable."""
    return lib().oai4g_get_TBS_DL(mcs, nb_rb)


def tbs_bits(mcs, nb_rb):
    """TBS in bits for (mcs, nb_rb) as dlsim uses it (get_TBS_DL << 3; dci_tools.c)."""
    return get_TBS_DL(mcs, nb_rb) << 3

CONFIGS = {
    # C1: dlsim 1.4 MHz SISO QPSK (MCS 9), 3 PDCCH symbols
    "C1": dict(N_RB_DL=6, nb_antennas_tx=1, mode1_flag=1, n_cw=1, mimo_mode=SISO, num_pdcch_symbols=3,
               mcs=(9, 0), rb_alloc=FULL_ALLOC_6, nb_rb=6, Kmimo=1),
    # C2: dlsim 20 MHz SISO 16-QAM (MCS 16)
    "C2": dict(N_RB_DL=100, nb_antennas_tx=1, mode1_flag=1, n_cw=1, mimo_mode=SISO, num_pdcch_symbols=1,
               mcs=(16, 0), rb_alloc=FULL_ALLOC_100, nb_rb=100, Kmimo=1),
    # C3: dlsim 20 MHz 2x2 TM3 (LARGE_CDD) 64-QAM, MCS 19 on both codewords (highest the reference encodes)
    "C3": dict(N_RB_DL=100, nb_antennas_tx=2, mode1_flag=0, n_cw=2, mimo_mode=LARGE_CDD, num_pdcch_symbols=1,
               mcs=(19, 19), rb_alloc=FULL_ALLOC_100, nb_rb=100, Kmimo=2),
    # C4: C3 on 4 TX antennas (build-defined extension: 4-port CRS exclusions, 36.211 6.3.4.2.2
    # large-delay CDD precoding over the rank-2 codebook entries 12-15)
    "C4": dict(N_RB_DL=100, nb_antennas_tx=4, mode1_flag=0, n_cw=2, mimo_mode=LARGE_CDD, num_pdcch_symbols=1,
               mcs=(19, 19), rb_alloc=FULL_ALLOC_100, nb_rb=100, Kmimo=2),
    # TM2: dlsim 20 MHz 2 TX transmit diversity (ALAMOUTI, DCI format 1: one codeword, Nl = 1), 16-QAM
    "TM2": dict(N_RB_DL=100, nb_antennas_tx=2, mode1_flag=0, n_cw=1, mimo_mode=ALAMOUTI, num_pdcch_symbols=1,
                mcs=(16, 0), rb_alloc=FULL_ALLOC_100, nb_rb=100, Kmimo=1),
    # TM2 at 1.4 MHz, QPSK (MCS 9), 3 PDCCH symbols
    "TM2S": dict(N_RB_DL=6, nb_antennas_tx=2, mode1_flag=0, n_cw=1, mimo_mode=ALAMOUTI, num_pdcch_symbols=3,
                 mcs=(9, 0), rb_alloc=FULL_ALLOC_6, nb_rb=6, Kmimo=1),
    # TM6: dlsim -x 6 at 20 MHz: one layer on two ports, closed-loop precoder per subband from pmi_alloc
    # (every mode 3..8 takes the same branch), 64-QAM (MCS 22)
    "TM6": dict(N_RB_DL=100, nb_antennas_tx=2, mode1_flag=0, n_cw=1, mimo_mode=PUSCH_PRECODING0, num_pdcch_symbols=1,
                mcs=(22, 0), rb_alloc=FULL_ALLOC_100, nb_rb=100, Kmimo=1, pmi_alloc=0xE4B1),
}


def make_params(name="C3", subframe=7, subframe_step=0, rnti=0x1234, Nid_cell=0, with_crs=0, **over):
    c = dict(CONFIGS[name])
    c.update(over)
    p = TxParams()
    p.N_RB_DL = c["N_RB_DL"]
    p.Nid_cell = Nid_cell
    p.Ncp = c.get("Ncp", 0)
    p.nb_antennas_tx = c["nb_antennas_tx"]
    p.mode1_flag = c["mode1_flag"]
    p.frame_type = 0
    p.n_cw = c["n_cw"]
    p.mimo_mode = c["mimo_mode"]
    p.num_pdcch_symbols = c["num_pdcch_symbols"]
    p.Kmimo = c["Kmimo"]
    p.Mdlharq = 8
    p.first_subframe = subframe
    p.subframe_step = subframe_step
    p.with_crs = with_crs
    p.rnti = rnti
    p.amp = 512
    p.sqrt_rho_a = 8192
    p.sqrt_rho_b = 8192
    for i in range(4):
        p.rb_alloc[i] = c["rb_alloc"][i]
    p.nb_rb = c["nb_rb"]
    p.pmi_alloc = c.get("pmi_alloc", 0)
    tbs = c.get("TBS")
    for cw in range(p.n_cw):
        p.mcs[cw] = c["mcs"][cw]
        p.rvidx[cw] = 0
        p.q[cw] = 0
        p.TBS[cw] = tbs[cw] if tbs else tbs_bits(c["mcs"][cw], c["nb_rb"])
    maxA = max(p.TBS[cw] // 8 for cw in range(p.n_cw))
    p.payload_stride = (maxA + 3 + 15) & ~15
    return p


class TxPipeline(_DeviceOwner):
    """Batched device-resident transmit path for one configuration (oai4g_tx_*)."""

    def __init__(self, params, n_sf, alloc=True):
        self.L = init()
        self.params = params
        self.n_sf = n_sf
        self.cfg = self._own(self.L.oai4g_tx_config_create(ctypes.byref(params)), self.L.oai4g_tx_config_destroy)
        self.n_cw = params.n_cw
        self.n_ant = params.nb_antennas_tx
        self.spt = self.L.oai4g_tx_iq_samples(self.cfg)
        self.ebits_words = self.L.oai4g_tx_ebits_words(self.cfg)
        self.payload_bytes = n_sf * self.n_cw * params.payload_stride
        self.work_bytes = self.L.oai4g_tx_workspace_bytes(self.cfg, n_sf)
        self.iq_samples = n_sf * self.n_ant * self.spt
        self.d_payload = self.d_work = self.d_iq = self.d_rv = None
        if alloc:
            self.d_payload = self._dev(self.payload_bytes)
            self.d_work = self._dev(self.work_bytes)
            self.d_iq = self._dev(self.iq_samples * 4)

    def G(self, cw, subframe):
        return self.L.oai4g_tx_G(self.cfg, cw, subframe)

    def set_control(self, items, n_common=0):
        """oai4g_tx_config_set_control: generate_dci_top's PCFICH + PDCCH for these DCIs in every
        batch element (items as for generate_dci_top; [] switches it off)."""
        arr = dci_allocs(items)
        _check(self.L.oai4g_tx_config_set_control(self.cfg, len(items) - n_common, n_common, arr) == 0)

    def set_common(self, pss_sss=False, pbch_pdu=None, frame_mod4=0, phich=()):
        """oai4g_tx_config_set_common: PSS + SSS (subframe indices 0 / 5), the PBCH quarter
        frame_mod4 of pbch_pdu (subframe index 0) and PHICHs (subframe, ngroup, nseq, hi);
        with no argument it switches them off."""
        c = CommonSig()
        c.pss_sss = 1 if pss_sss else 0
        if pbch_pdu is not None:
            c.pbch = 1
            for i in range(3):
                c.pbch_pdu[i] = int(pbch_pdu[i])
        c.frame_mod4 = frame_mod4
        c.n_phich = len(phich)
        for i, (sf, g, q, h) in enumerate(phich):
            c.phich[i].subframe, c.phich[i].ngroup, c.phich[i].nseq, c.phich[i].hi = sf, g, q, h
        on = c.pss_sss or c.pbch or c.n_phich
        _check(self.L.oai4g_tx_config_set_common(self.cfg, ctypes.byref(c) if on else None) == 0)

    def fill_payload(self, seed):
        _check(self.L.oai4g_fill_payload(self.d_payload, self.payload_bytes, seed, None) == 0)

    def upload_payload(self, payload):
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        assert payload.nbytes == self.payload_bytes
        self._put(self.d_payload, payload)

    def download_payload(self):
        return self._get(self.d_payload, (self.n_sf, self.n_cw, self.params.payload_stride), np.uint8)

    def run(self, stream=None):
        _check(self.L.oai4g_tx_batch(self.cfg, self.n_sf, self.d_payload, self.d_work, self.d_iq, stream) == 0)

    def enable_tb_rv(self):
        """oai4g_tx_config_enable_tb_rv: derive and upload the per-rv plan tables for run_rv."""
        _check(self.L.oai4g_tx_config_enable_tb_rv(self.cfg) == 0)

    def upload_rv(self, rv):
        """[n_sf][n_cw] redundancy versions (0..3) for run_rv / encode_only_rv."""
        rv = np.ascontiguousarray(np.asarray(rv, dtype=np.uint8).reshape(self.n_sf, self.n_cw))
        if self.d_rv is None:
            self.d_rv = self._dev(rv.nbytes)
        self._put(self.d_rv, rv)

    def run_rv(self, rv=None, stream=None):
        """oai4g_tx_batch_rv: the batch with a redundancy version per transport block (rv: [n_sf][n_cw],
        or None for the array uploaded last)."""
        if rv is not None:
            self.upload_rv(rv)
        _check(self.L.oai4g_tx_batch_rv(self.cfg, self.n_sf, self.d_payload, self.d_rv, self.d_work, self.d_iq,
                                        stream) == 0)

    def encode_only_rv(self, rv=None, stream=None):
        if rv is not None:
            self.upload_rv(rv)
        _check(self.L.oai4g_tx_encode_rv(self.cfg, self.n_sf, self.d_payload, self.d_rv, self.d_work, stream) == 0)

    def run_timed(self, stream=None):
        ms = (ctypes.c_float * 2)()
        _check(self.L.oai4g_tx_batch_timed(self.cfg, self.n_sf, self.d_payload, self.d_work, self.d_iq, stream,
                                           ms) == 0)
        return ms[0], ms[1]

    def encode_only(self, stream=None):
        _check(self.L.oai4g_tx_encode(self.cfg, self.n_sf, self.d_payload, self.d_work, stream) == 0)

    def diag_encode_phase_ms(self, stop_phase, reps=5):
        ms = ctypes.c_float()
        _check(self.L.oai4g_diag_encode_phase_ms(self.cfg, self.n_sf, self.d_payload, self.d_work, stop_phase, reps,
                                                 ctypes.byref(ms)) == 0)
        return ms.value

    def modulate_only(self, stream=None):
        """oai4g_tx_modulate: the modulator kernel alone, from the e-bit words in the workspace."""
        _check(self.L.oai4g_tx_modulate(self.cfg, self.n_sf, self.d_work, self.d_iq, stream) == 0)

    def upload_ebits(self, words):
        """Packed scrambled e-bit words [n_sf][n_cw][ebits_words] into the workspace."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        assert words.nbytes <= self.work_bytes
        self._put(self.d_work, words)

    @property
    def mod_nosat(self):
        return bool(self.L.oai4g_tx_mod_nosat(self.cfg))

    @property
    def mod_lz(self):
        """Leading symbols the modulator's item space skips (oai4g_mod_item_map)."""
        return self.L.oai4g_tx_mod_lz(self.cfg)

    def sync(self):
        _check(self.L.oai4g_sync() == 0)

    def ebits(self):
        return self._get(self.d_work, self.work_bytes // 4, np.uint32).reshape(self.n_sf, self.n_cw, self.ebits_words)

    def iq(self):
        return self._get(self.d_iq, (self.n_sf, self.n_ant, self.spt), np.int32)


def unpack_bits(words, nbits):
    """Packed LSB-first uint32 words -> uint8 bit array."""
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return b[:nbits]


# ------------------------------------------------------------------------------------------
# SC-FDMA: the PUSCH DFT sizes, ulsch_modulation, lte_idft
# ------------------------------------------------------------------------------------------
class PuschPlan(ctypes.Structure):
    """oai4g_pusch_plan_t"""
    _fields_ = [("size", ctypes.c_uint16), ("n_levels", ctypes.c_uint16), ("radix", ctypes.c_uint8 * 4),
                ("sub_size", ctypes.c_uint16 * 4), ("norm", ctypes.c_int16 * 4), ("leaf_norm", ctypes.c_int16),
                ("pad", ctypes.c_uint16), ("tw_offset", ctypes.c_uint32 * 4), ("n_twiddles", ctypes.c_uint32)]


class UlHarq(ctypes.Structure):
    """oai4g_ul_harq_t"""
    _fields_ = [("first_rb", ctypes.c_uint16), ("nb_rb", ctypes.c_uint16), ("mcs", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3)]


class UeUlsch(ctypes.Structure):
    """oai4g_ue_ulsch_t"""
    _fields_ = [("harq_processes", ctypes.POINTER(UlHarq) * 8), ("h", ctypes.c_void_p), ("rnti", ctypes.c_uint16),
                ("harq_pid", ctypes.c_uint8), ("Nsymb_pusch", ctypes.c_uint8), ("srs_active", ctypes.c_uint8),
                ("cooperation_flag", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 2)]


def pusch_dft_plan(Msc):
    """oai4g_pusch_dft_plan: (PuschPlan, twiddles int16 [n_twiddles][2]).  Host only; raises for a size the reference
    has no transform for."""
    plan = PuschPlan()
    tw = np.zeros((2048, 2), dtype=np.int16)
    _check(lib().oai4g_pusch_dft_plan(Msc, ctypes.byref(plan), _ptr(tw), len(tw)) == 0)
    return plan, tw[:plan.n_twiddles].copy()


def pusch_dft(Msc, x, scale_flag=1):
    """oai4g_pusch_dft: dft<Msc>(x, y, scale_flag) of one transform on plain samples, int16 [Msc][2] -> the same"""
    x = np.ascontiguousarray(x, dtype=np.int16)
    assert x.size == 2 * Msc
    y = np.zeros((Msc, 2), dtype=np.int16)
    _check(lib().oai4g_pusch_dft(Msc, _ptr(x), _ptr(y), scale_flag) == 0)
    return y


def dft_lte(d, Msc, Nsymb, z=None):
    """oai4g_dft_lte: d int16 [>= Nsymb Msc][2] -> z (the given array, whose words past Nsymb Msc stay as they are)"""
    d = np.ascontiguousarray(d, dtype=np.int16).reshape(-1, 2)
    assert len(d) >= Nsymb * Msc
    z = np.zeros((Nsymb * Msc, 2), dtype=np.int16) if z is None else z
    assert z.flags.c_contiguous and z.dtype == np.int16 and z.size >= 2 * Nsymb * Msc
    _check(lib().oai4g_dft_lte(_ptr(z), _ptr(d), Msc, Nsymb) == 0)
    return z


def lte_idft(fp, comp, Msc):
    """oai4g_lte_idft in place on comp int16 [symbols_per_tti][12 N_RB_DL][2]"""
    assert comp.flags.c_contiguous and comp.dtype == np.int16 and comp.size == 2 * fp.symbols_per_tti * 12 * fp.N_RB_DL
    _check(lib().oai4g_lte_idft(ctypes.byref(fp), _ptr(comp), Msc) == 0)
    return comp


def ulsch_modulation(txdataF0, amp, subframe, fp, first_rb, nb_rb, mcs, h, rnti, srs_active=0, harq_pid=0, cooperation_flag=0,
                     Nsymb_pusch=None):
    """oai4g_ulsch_modulation into txdataF0 int16 [10 symbols_per_tti][ofdm_symbol_size][2], one frame of antenna 0.
    Returns 0, or 1 for the reference's own refusals (nothing written); a refusal of the library raises."""
    assert txdataF0.flags.c_contiguous and txdataF0.dtype == np.int16
    assert txdataF0.size == 2 * 10 * fp.symbols_per_tti * fp.ofdm_symbol_size
    h = np.ascontiguousarray(h, dtype=np.uint8)
    harq = UlHarq(first_rb, nb_rb, mcs)
    u = UeUlsch()
    for i in range(8):
        u.harq_processes[i] = ctypes.pointer(harq)
    u.h, u.rnti, u.harq_pid, u.srs_active, u.cooperation_flag = h.ctypes.data, rnti, harq_pid, srs_active, cooperation_flag
    u.Nsymb_pusch = fp.symbols_per_tti - 2 - srs_active if Nsymb_pusch is None else Nsymb_pusch
    tx = (ctypes.c_void_p * 1)(txdataF0.ctypes.data)
    r = lib().oai4g_ulsch_modulation(tx, amp, 0, subframe, ctypes.byref(fp), ctypes.byref(u))
    _check(r >= 0)
    return r


class _PuschBatch(_DeviceOwner):
    """Device-resident PUSCH transmit / transform precoding of n_sf subframes of one allocation:
    d_h [n_sf][G] -> d_txdataF [n_sf][symbols_per_tti][ofdm_symbol_size] (launch_mod, oai4g_pusch_mod_batch);
    d_d -> d_z [n_sf][Nsymb_pusch][Msc] (launch_dft, oai4g_pusch_dft_batch);
    d_comp [n_sf][symbols_per_tti][12 N_RB_DL] in place (launch_idft, oai4g_pusch_idft_batch).
    Each buffer exists once its upload asked for it.  Public as PuschBatch."""

    def __init__(self, fp, n_sf, first_rb, nb_rb, Qm, srs_active=0, rnti=0x1234, first_subframe=0, subframe_step=1):
        self.L, self.fp, self.n_sf = init(), fp, n_sf
        self.Msc, self.Qm = 12 * nb_rb, Qm
        self.nsymb, self.N = fp.symbols_per_tti, fp.ofdm_symbol_size
        self.Nsymb_pusch = self.nsymb - 2 - srs_active
        self.G = self.Msc * Qm * self.Nsymb_pusch
        self.cfg = self._own(self.L.oai4g_pusch_config_create(ctypes.byref(fp), first_rb, nb_rb, Qm, srs_active, rnti,
                                                              first_subframe, subframe_step), self.L.oai4g_pusch_config_destroy)
        self.d_h = self.d_txdataF = self.d_d = self.d_z = self.d_comp = None

    def _up(self, name, a, dtype, size):
        a = np.ascontiguousarray(a, dtype=dtype)
        assert a.size == size, (name, a.size, size)
        if getattr(self, name) is None:
            setattr(self, name, self._dev(a.nbytes))
        self._put(getattr(self, name), a)

    def upload_h(self, h):
        """uint8 [n_sf][G]"""
        self._up("d_h", h, np.uint8, self.n_sf * self.G)

    def upload_grid(self, grid):
        """int16 [n_sf][symbols_per_tti][ofdm_symbol_size][2]: what the REs the modulator does not write keep"""
        self._up("d_txdataF", grid, np.int16, 2 * self.n_sf * self.nsymb * self.N)

    def launch_mod(self, amp, stream=None):
        _check(self.L.oai4g_pusch_mod_batch(self.cfg, self.n_sf, self.d_h, self.G, amp, self.d_txdataF, stream) == 0)

    def grid(self):
        return self._get(self.d_txdataF, (self.n_sf, self.nsymb, self.N, 2), np.int16)

    def upload_d(self, d):
        """int16 [n_sf][Nsymb_pusch][Msc][2]"""
        self._up("d_d", d, np.int16, 2 * self.n_sf * self.Nsymb_pusch * self.Msc)
        if self.d_z is None:
            self.d_z = self._dev(4 * self.n_sf * self.Nsymb_pusch * self.Msc)

    def launch_dft(self, stream=None):
        _check(self.L.oai4g_pusch_dft_batch(self.cfg, self.n_sf, self.d_d, self.d_z, stream) == 0)

    def z(self):
        return self._get(self.d_z, (self.n_sf, self.Nsymb_pusch, self.Msc, 2), np.int16)

    def upload_comp(self, comp):
        """int16 [n_sf][symbols_per_tti][12 N_RB_DL][2]"""
        self._up("d_comp", comp, np.int16, 2 * self.n_sf * self.nsymb * 12 * self.fp.N_RB_DL)

    def launch_idft(self, stream=None):
        _check(self.L.oai4g_pusch_idft_batch(self.cfg, self.n_sf, self.d_comp, stream) == 0)

    def comp(self):
        return self._get(self.d_comp, (self.n_sf, self.nsymb, 12 * self.fp.N_RB_DL, 2), np.int16)


PuschBatch = _PuschBatch    # private by name like _SyncBatch: its lifetime cases are in tests/test_pusch_cpu.py
