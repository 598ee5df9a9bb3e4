/*
 * openair4g_amd — MI355X-native LTE PDSCH transmit path, C ABI.
 *
 * Two surfaces:
 *
 *  1. Drop-in entry points mirroring the reference call surface of the DLSCH transmit path
 *     (erlgo/openair4G openair1/PHY).  Same argument meaning, same in-place side effects on
 *     caller-owned buffers, same return conventions; host buffers in, host buffers out, the
 *     arithmetic runs on the GPU.  The reference passes its own LTE_DL_FRAME_PARMS /
 *     LTE_eNB_DLSCH_t; here the fields the path touches are mirrored in oai4g_frame_parms_t /
 *     oai4g_dlsch_t (the reference-side shim that fills them is in INTEGRATION.md).
 *
 *  2. A batched, device-resident API (oai4g_tx_*) that runs whole subframes
 *     (encode -> rate-match -> scramble -> modulate/map -> IDFT + CP) for many subframes per
 *     launch, with payloads already in HBM.  This is the throughput path.
 *
 * Every entry point that computes returns/records an error if the HIP runtime or a gfx950
 * device is unavailable: there is no CPU fallback.  oai4g_last_error() gives the message.
 */
#ifndef OAI4G_H
#define OAI4G_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OAI4G_LTE_NULL 2                    /* PHY/CODING/defs.h:53 */
#define OAI4G_NSOFT 1827072                 /* PHY/LTE_TRANSPORT/defs.h:62 */
#define OAI4G_MAX_SEGMENTS 16               /* PHY/LTE_TRANSPORT/defs.h:67 */
#define OAI4G_MAX_CHANNEL_BITS (14 * 1200 * 6)
#define OAI4G_D_BYTES (96 + 12 + 3 + 3 * 6144)
#define OAI4G_W_BYTES (3 * 6144 + 96)

/* MIMO_mode_t subset (PHY/impl_defs_lte.h) */
enum {
  OAI4G_SISO = 0,
  OAI4G_ALAMOUTI = 1,
  OAI4G_LARGE_CDD = 2,
  /* transmission modes 4-6, one layer on two ports (dlsch_modulation.c:750-866).  All six take one
   * branch: the precoder of an RB comes from pmi_alloc (oai4g_get_pmi), never from the mode's name */
  OAI4G_UNIFORM_PRECODING11 = 3,
  OAI4G_UNIFORM_PRECODING1m1 = 4,
  OAI4G_UNIFORM_PRECODING1j = 5,
  OAI4G_UNIFORM_PRECODING1mj = 6,
  OAI4G_PUSCH_PRECODING0 = 7,
  OAI4G_PUSCH_PRECODING1 = 8
};
/* Extension_t (PHY/MODULATION/defs.h) */
enum { OAI4G_CYCLIC_PREFIX = 0, OAI4G_CYCLIC_SUFFIX = 1, OAI4G_ZEROS = 2, OAI4G_NONE = 3 };

/* Fields of LTE_DL_FRAME_PARMS (PHY/impl_defs_lte.h:470-572) used on this path. */
typedef struct {
  uint16_t N_RB_DL;
  uint16_t Nid_cell;
  uint8_t Ncp;              /* 0 = normal CP, 1 = extended */
  uint8_t nushift;          /* Nid_cell % 6 */
  uint8_t mode1_flag;       /* 1 = single-port CRS (TM1) */
  uint8_t nb_antennas_tx;
  uint8_t frame_type;       /* 0 = FDD, 1 = TDD */
  uint8_t symbols_per_tti;
  uint8_t log2_symbol_size;
  uint8_t Nid_cell_mbsfn;   /* MBSFN area id (impl_defs_lte.h:482; 36.211 N_ID^MBSFN is 0..255) */
  uint16_t ofdm_symbol_size;
  uint16_t first_carrier_offset;
  uint16_t nb_prefix_samples;
  uint16_t nb_prefix_samples0;
  uint32_t samples_per_tti;
  /* control region (phich_config_common, tdd_config, nb_antennas_tx_eNB of LTE_DL_FRAME_PARMS) */
  uint8_t phich_resource;   /* PHICH_RESOURCE_t (impl_defs_lte.h:80-85): 1, 3, 6, 12 = Ng 1/6, 1/2, 1, 2 */
  uint8_t phich_duration;   /* 0 normal (extended is not supported by the PDCCH path) */
  uint8_t tdd_config;
  uint8_t nb_antennas_tx_eNB;
} oai4g_frame_parms_t;

/* DCI_ALLOC_t (PHY/LTE_TRANSPORT/defs.h:734-749) */
typedef struct {
  uint8_t dci_length;       /* bits */
  uint8_t L;                /* log2 aggregation level 0..3 */
  int32_t nCCE;             /* first CCE; < 0: not transmitted */
  uint8_t ra_flag;
  uint16_t rnti;
  uint32_t format;          /* DCI_format_t (not used by the encoder) */
  uint8_t dci_pdu[8];
} oai4g_dci_alloc_t;

/* LTE_DL_eNB_HARQ_t (PHY/LTE_TRANSPORT/defs.h:104-169), path fields only. */
typedef struct {
  uint32_t TBS;
  uint32_t B;
  uint8_t *b;
  uint8_t *c[OAI4G_MAX_SEGMENTS];
  uint32_t RTC[OAI4G_MAX_SEGMENTS];
  uint8_t round;
  uint8_t mcs;
  uint8_t rvidx;
  uint8_t mimo_mode;
  uint32_t rb_alloc[4];
  uint16_t nb_rb;
  uint8_t *e;                              /* OAI4G_MAX_CHANNEL_BITS bytes */
  uint8_t *d[OAI4G_MAX_SEGMENTS];          /* OAI4G_D_BYTES; first 96 = LTE_NULL */
  uint8_t *w[OAI4G_MAX_SEGMENTS];          /* OAI4G_W_BYTES */
  uint32_t C, Cminus, Cplus, Kminus, Kplus, F;
  uint8_t Nl;
  uint8_t Nlayers;
  uint8_t first_layer;
  uint16_t pmi_alloc;                      /* modes 3..8: two precoder bits per subband (oai4g_get_pmi); in
                                              what was padding, 0 from oai4g_new_dlsch */
} oai4g_dl_harq_t;

/* LTE_eNB_DLSCH_t (PHY/LTE_TRANSPORT/defs.h:240-274), path fields only. */
typedef struct {
  uint16_t rnti;
  uint8_t current_harq_pid;
  uint8_t Mdlharq;
  uint8_t Kmimo;
  int16_t sqrt_rho_a;
  int16_t sqrt_rho_b;
  oai4g_dl_harq_t *harq_processes[8];
} oai4g_dlsch_t;

/* ---------------- library / device ----------------
 * The library runs on one device (oai4g_set_device before oai4g_init, else the current one).  Every
 * compute call makes that device the calling thread's current HIP device and leaves it so. */
int oai4g_init(void);                       /* idempotent; 0 on success, <0 if no usable GPU */
const char *oai4g_last_error(void);
int oai4g_device_name(char *buf, int len);

/* ---------------- parameter helpers (host-side, scalar) ---------------- */
/* init_frame_parms (PHY/INIT/lte_parms.c:31), osf = 1 */
int oai4g_init_frame_parms(oai4g_frame_parms_t *fp, uint16_t N_RB_DL, uint16_t Nid_cell, uint8_t Ncp,
                           uint8_t nb_antennas_tx, uint8_t mode1_flag, uint8_t frame_type);
/* get_Qm (lte_mcs.c:45), get_G (lte_mcs.c:336) */
uint8_t oai4g_get_Qm(uint8_t mcs);
int oai4g_get_G(const oai4g_frame_parms_t *fp, uint16_t nb_rb, const uint32_t *rb_alloc, uint8_t mod_order,
                uint8_t Nl, uint8_t num_pdcch_symbols, int frame, uint8_t subframe);
/* get_Qm_ul (lte_mcs.c:57), get_I_TBS (:69), get_I_TBS_UL (:84) */
uint8_t oai4g_get_Qm_ul(uint8_t mcs);
uint8_t oai4g_get_I_TBS(uint8_t mcs);
uint8_t oai4g_get_I_TBS_UL(uint8_t mcs);
/* TBStable[I_TBS][nb_rb-1] (LTE_TRANSPORT/dlsch_tbs_full.h:34, 36.213 Table 7.1.7.2.1-1) in bits,
 * 0 outside 0..26 x 1..110.  The reference's entry for I_TBS 6, 1 PRB is 328 (the spec's is 88);
 * the table keeps the reference's value. */
uint32_t oai4g_tbs_bits(uint8_t I_TBS, uint16_t nb_rb);
/* get_TBS_DL (lte_mcs.c:118) / get_TBS_UL (:137): TBS in BYTES, as the reference returns it;
 * 0 when nb_rb == 0 or mcs >= 29 */
uint32_t oai4g_get_TBS_DL(uint8_t mcs, uint16_t nb_rb);
uint32_t oai4g_get_TBS_UL(uint8_t mcs, uint16_t nb_rb);
/* new_eNB_dlsch / free_eNB_dlsch (dlsch_coding.c:120 / :85) */
oai4g_dlsch_t *oai4g_new_dlsch(uint8_t Kmimo, uint8_t Mdlharq, uint8_t N_RB_DL);
void oai4g_free_dlsch(oai4g_dlsch_t *dlsch);
/* lte_gold_generic (PHY/LTE_REFSIG/lte_gold.c:151): scalar 32-bit LFSR helper, host-side */
uint32_t oai4g_lte_gold_generic(uint32_t *x1, uint32_t *x2, uint8_t reset);
/* The encoder's 32-fold of the QPP interleaver, host-side.  With Q = K/32, a code-block size K takes
 * it when 1024 | K and Pi(k + Q) = Pi(k) + s Q (mod K) with s odd holds for every k < K (verified
 * step by step, not from a closed form).  Returns 1 and writes s and the K/32 entries
 * tab[k] = (Pi(k) mod Q) << 7 | (s^-1 (Pi(k) div Q) mod 32); 0 (outputs untouched) for a size that
 * keeps the quarter fold; < 0 when K is not a turbo block size. */
int oai4g_qpp_fold32(uint32_t K, uint32_t *s, uint16_t *tab);
/* The lane scan of the encoder's turbo phase for block sizes with 32 | K, host-side: with q = 1, 2 or
 * 3 chunks of 32 bits per lane, rows[d] is the constituent encoder's zero-input state propagation over
 * 32 q 2^d steps (d = 0..5), the image of state s in bits 4s..4s+2.  Returns 0, or -1 for another q. */
int oai4g_rsc_scan_rows(uint32_t q, uint32_t rows[6]);
/* The tile-pair schedule of the encoder's rate-matching phase, host-side.  A codeword of C blocks, the
 * first n0 of block size index 0 and the rest of index 1, with nt[i] plan tiles per block of size i
 * (1..20; ceil(R/32) + ceil(R/16)) and wrapt[i] the tile whose run straddles the circular buffer's end
 * (or ~0 / ~1: none / the general placement path).  A block of size i runs ceil(nt[i] / 2) pairs of
 * tiles (2p, 2p + 1).  Writes pair0[r] = index of block r's first pair (pair0[C] = all pairs, also the
 * return value) and one descriptor per pair in block order: bit 0 = the pair holds the wrap tile,
 * bit 1 = i, bits 2-5 = r, bits 16-28 = byte offset of the pair's first row in the plan tables
 * (4 (21 * 32 i + 32 * 2p)).  pairs holds up to 10 C entries, pair0 C + 1.  Returns < 0 for arguments
 * out of range. */
int oai4g_rm_pair_schedule(uint32_t C, uint32_t n0, const uint32_t nt[2], const uint32_t wrapt[2],
                           uint32_t *pairs, uint32_t *pair0);
/* The fused modulator's item map, host-side.  Its persistent workgroups walk a flat item space that is
 * dense over the symbols lz .. lz + per - 1 of every subframe (the lz leading symbols that carry nothing
 * at any subframe index are no items), ips items per symbol (2 with four antennas: one per antenna
 * pair): item -> sf = item / ips / per, l = lz + item / ips % per, pair = item % ips.  Workgroup b of a
 * grid of g takes items (b + k g) u .. + u - 1 for k = 0, 1, ... (u = 2048 / N transforms per
 * workgroup).  Returns 1 when the item also zero-fills symbols 0 .. lz - 1 of its subframe (l == lz > 0),
 * else 0; < 0 for arguments out of range (ips 1 or 2, lz <= 4, per >= 1). */
int oai4g_mod_item_map(uint32_t item, uint32_t ips, uint32_t lz, uint32_t per, uint32_t *sf, uint32_t *l,
                       uint32_t *pair);
/* get_pmi (dlsch_modulation.c:1136): the precoder index of resource block rb.  Modes up to
 * OAI4G_PUSCH_PRECODING1 read two bits per subband, (pmi_alloc >> 2 (rb / S)) & 3, the later modes one,
 * (pmi_alloc >> (rb / S)) & 1; a subband is S = 1 RB at 6 PRB, 6 at 50, 8 at 100 and 4 at every other
 * bandwidth.  pmi_alloc is the reference's 16-bit field widened to 32 bits before the shift, so a
 * subband whose shift reaches 16 (subband 8 at 50 PRB, 8..12 at 100 PRB) reads precoder 0. */
uint8_t oai4g_get_pmi(uint8_t N_RB_DL, uint8_t mimo_mode, uint16_t pmi_alloc, uint16_t rb);
/* Test hook: at most n_workgroups in the fused modulator's grid, so that small batches run many rounds
 * per workgroup and a ragged last round; 0 restores the default (workgroups per CU x CUs). */
void oai4g_set_modofdm_grid_cap(int n_workgroups);

/* ---------------- drop-in entry points (GPU compute on host buffers) ---------------- */
/* crc24a / crc24b (PHY/CODING/crc_byte.c:117 / :135): returns crc << 8 */
uint32_t oai4g_crc24a(const uint8_t *in, int bitlen);
uint32_t oai4g_crc24b(const uint8_t *in, int bitlen);
/* lte_segmentation (PHY/CODING/lte_segmentation.c:39) */
int oai4g_lte_segmentation(const uint8_t *input_buffer, uint8_t **output_buffers, uint32_t B, uint32_t *C,
                           uint32_t *Cplus, uint32_t *Cminus, uint32_t *Kplus, uint32_t *Kminus, uint32_t *F);
/* threegpplte_turbo_encoder (PHY/CODING/3gpplte_sse.c:380, decl CODING/defs.h:315) */
void oai4g_threegpplte_turbo_encoder(const uint8_t *input, uint16_t input_length_bytes, uint8_t *output,
                                     uint8_t F, uint16_t interleaver_f1, uint16_t interleaver_f2);
/* sub_block_interleaving_turbo (lte_rate_matching.c:51, decl CODING/defs.h:112).
 * d points at &d[96] of a buffer whose 96 preceding bytes are readable (LTE_NULL). */
uint32_t oai4g_sub_block_interleaving_turbo(uint32_t D, uint8_t *d, uint8_t *w);
/* lte_rate_matching_turbo (lte_rate_matching.c:464, decl CODING/defs.h:191) */
uint32_t oai4g_lte_rate_matching_turbo(uint32_t RTC, uint32_t G, const uint8_t *w, uint8_t *e, uint8_t C,
                                       uint32_t Nsoft, uint8_t Mdlharq, uint8_t Kmimo, uint8_t rvidx,
                                       uint8_t Qm, uint8_t Nl, uint8_t r, uint8_t nb_rb, uint8_t m);
/* dlsch_encoding (PHY/LTE_TRANSPORT/dlsch_coding.c:254, decl proto.h:110) */
int oai4g_dlsch_encoding(uint8_t *a, const oai4g_frame_parms_t *frame_parms, uint8_t num_pdcch_symbols,
                         oai4g_dlsch_t *dlsch, int frame, uint8_t subframe);
/* dlsch_scrambling (PHY/LTE_TRANSPORT/dlsch_scrambling.c:51, decl proto.h:1600) */
void oai4g_dlsch_scrambling(const oai4g_frame_parms_t *frame_parms, int mbsfn_flag, oai4g_dlsch_t *dlsch, int G,
                            uint8_t q, uint8_t Ns);
/* dlsch_modulation (PHY/LTE_TRANSPORT/dlsch_modulation.c:1181, decl proto.h:197).
 * txdataF[aa] is the caller's whole-frame grid as in the reference (indexed by
 * ofdm_symbol_size*(l + subframe_offset*nsymb)).  Returns REs allocated, or -1. */
int oai4g_dlsch_modulation(int32_t **txdataF, int16_t amp, uint32_t subframe_offset,
                           const oai4g_frame_parms_t *frame_parms, uint8_t num_pdcch_symbols,
                           oai4g_dlsch_t *dlsch0, oai4g_dlsch_t *dlsch1);
/* PHY_ofdm_mod (PHY/MODULATION/ofdm_mod.c:85, decl MODULATION/defs.h:48); CYCLIC_PREFIX only */
void oai4g_PHY_ofdm_mod(const int32_t *input, int32_t *output, uint8_t log2fftsize, uint8_t nb_symbols,
                        uint16_t nb_prefix_samples, int etype);
/* normal_prefix_mod (ofdm_mod.c:47, decl MODULATION/defs.h:88) */
void oai4g_normal_prefix_mod(const int32_t *txdataF, int32_t *txdata, uint8_t nsymb,
                             const oai4g_frame_parms_t *frame_parms);
/* do_OFDM_mod (ofdm_mod.c:233, decl MODULATION/defs.h:90); PMCH subframes not supported */
void oai4g_do_OFDM_mod(int32_t **txdataF, int32_t **txdata, uint32_t frame, uint16_t next_slot,
                       const oai4g_frame_parms_t *frame_parms);
/* generate_pilots (PHY/LTE_TRANSPORT/pilots.c:43, decl proto.h): CRS into txdataF[ant] for
 * Ntti subframes (the reference's frame grid; overwrites the pilot REs).  The reference passes
 * PHY_VARS_eNB for its frame parameters and Gold table; here the table is derived from fp. */
void oai4g_generate_pilots(int32_t **txdataF, int16_t amp, const oai4g_frame_parms_t *frame_parms, uint16_t Ntti);
/* lte_dl_cell_spec (PHY/LTE_REFSIG/lte_dl_cell_spec.c:123): CRS of port p, pilot l (0/1) of slot
 * Ns into one OFDM symbol `output` (ofdm_symbol_size REs).  Returns 0, or -1 for a bad port. */
int oai4g_lte_dl_cell_spec(int32_t *output, int16_t amp, const oai4g_frame_parms_t *frame_parms, uint8_t Ns,
                           uint8_t l, uint8_t p);
/* idft64..idft2048 (PHY/TOOLS/lte_dfts.c:1856-2866 incl. idft512 :2479, decl TOOLS/defs.h:555): y = IDFT(x) */
int oai4g_idft(int log2n, const int16_t *x, int16_t *y, int scale);
void oai4g_idft2048(const int16_t *x, int16_t *y, int scale);
void oai4g_idft1024(const int16_t *x, int16_t *y, int scale);
void oai4g_idft512(const int16_t *x, int16_t *y, int scale);   /* lte_dfts.c:2479 */
void oai4g_idft256(const int16_t *x, int16_t *y, int scale);
void oai4g_idft128(const int16_t *x, int16_t *y, int scale);
void oai4g_idft64(const int16_t *x, int16_t *y, int scale);

/* ---------------- control region of the transmit grid ---------------- */
/* generate_pcfich_reg_mapping (PHY/LTE_TRANSPORT/pcfich.c:48): REG indices (units of 6 REs) and
 * the index of the lowest; prints them as the reference does. */
void oai4g_generate_pcfich_reg_mapping(const oai4g_frame_parms_t *frame_parms, uint16_t pcfich_reg[4],
                                       uint8_t *pcfich_first_reg_idx);
/* generate_pcfich (pcfich.c:144, decl LTE_TRANSPORT/proto.h:1432): CFI codeword, scrambling, QPSK
 * (SISO / ALAMOUTI) and REG mapping into symbol 0 of `subframe` of the frame grids txdataF[ant]
 * (overwrites 16 REs per antenna).  Returns 0, or -1 (num_pdcch_symbols outside 1..3). */
int oai4g_generate_pcfich(uint8_t num_pdcch_symbols, int16_t amp, const oai4g_frame_parms_t *frame_parms,
                          int32_t **txdataF, uint8_t subframe);

/* PDCCH geometry (host-side scalar helpers): get_mi (phich.c:59), get_nquad / get_nCCE
 * (dci.c:2494-2538), get_num_pdcch_symbols (dci.c:1964), generate_phich_reg_mapping
 * (phich.c:280; normal duration: returns the number of groups written into phich_reg[56][3]),
 * get_nCCE_offset (SCHED/phy_procedures_lte_eNb.c:308, over the library's CCE table, cleared by
 * oai4g_init_nCCE_table as init_nCCE_table :302 does; not thread-safe, like the reference) */
uint8_t oai4g_get_mi(const oai4g_frame_parms_t *frame_parms, uint8_t subframe);
uint16_t oai4g_get_nquad(uint8_t num_pdcch_symbols, const oai4g_frame_parms_t *frame_parms, uint8_t mi);
uint16_t oai4g_get_nCCE(uint8_t num_pdcch_symbols, const oai4g_frame_parms_t *frame_parms, uint8_t mi);
uint8_t oai4g_get_num_pdcch_symbols(uint8_t num_dci, const oai4g_dci_alloc_t *dci_alloc,
                                    const oai4g_frame_parms_t *frame_parms, uint8_t subframe);
int oai4g_generate_phich_reg_mapping(const oai4g_frame_parms_t *frame_parms, uint16_t phich_reg[56][3]);
void oai4g_init_nCCE_table(void);
int oai4g_get_nCCE_offset(uint8_t L, int nCCE, int common_dci, uint16_t rnti, uint8_t subframe);
/* generate_dci_top (PHY/LTE_TRANSPORT/dci.c:2024, decl LTE_TRANSPORT/proto.h): PCFICH + every
 * DCI (CRC16 with the RNTI mask, tail-biting convolutional code, rate matching to 72 * 2^L bits
 * at CCE nCCE), <NIL> filling, scrambling, QPSK (SISO / ALAMOUTI), quadruplet interleaving with
 * the cell-id cyclic shift and the REG mapping around the PCFICH / PHICH REGs, into the control
 * symbols of `subframe` of the frame grids txdataF[0..1] (overwrites).  Returns
 * num_pdcch_symbols; when that is outside 1..3 (too many CCEs, or an N_RB_DL without a PDCCH
 * geometry in get_nquad: 15 / 75) nothing is written (the reference maps an undefined CFI
 * codeword there) and oai4g_last_error() says why. */
uint8_t oai4g_generate_dci_top(uint8_t num_ue_spec_dci, uint8_t num_common_dci, const oai4g_dci_alloc_t *dci_alloc,
                               uint32_t n_rnti, int16_t amp, const oai4g_frame_parms_t *frame_parms,
                               int32_t **txdataF, uint32_t subframe);

/* ---------------- UE control decoding: tail-biting Viterbi, DCI, PBCH ---------------- */
/* phy_viterbi_lte_sse2 (PHY/CODING/viterbi_lte.c:140): n triples of soft bits y (bit 1 positive), two
 * passes over them with 8-bit saturating metrics, ties to the predecessor k + 32, traceback from the
 * first state with the largest metric; the decoded bits are ADDED into decoded_bytes (MSB first),
 * so the caller zeroes it, as the reference's callers do.  The reference is defined for soft bits
 * in [-8, 7] only (outside it reads past its tables); here every input is clamped to that range
 * first.  Returns 0, 1 when an input had to be clamped, or -1 (n = 0, n > 512, no device). */
int oai4g_phy_viterbi_lte(const int8_t *y, uint8_t *decoded_bytes, uint16_t n);
/* the same decode with its final state exposed (tests): the 64 path metrics after the second pass
 * and the state the traceback starts from; decoded (ceil(n / 8) bytes) is overwritten */
int oai4g_diag_viterbi_lte(const int8_t *y, uint16_t n, uint8_t *decoded, uint8_t metrics[64], uint8_t *start_state);
/* The receive plan of the convolutional code's rate matching for D trellis steps (D = payload + 16):
 * plan[3 i + s] is the first index of e that lte_rate_matching_cc_rx (lte_rate_matching.c:834) sums
 * into d^(s)_i after sub_block_deinterleaving_cc (:245); the repetitions follow every 3 D, below E.
 * Derived from generate_dummy_w_cc's <NULL> set (:384).  Returns 3 D, or -1 (D = 0 or D > 512). */
int oai4g_cc_rx_plan(uint32_t D, uint16_t *plan);
/* dci_decoding (PHY/LTE_TRANSPORT/dci.c:2426): e holds the 72 << aggregation_level soft bits of the
 * candidate's CCEs; rate-matching receive (sum of the repetitions, clamp to [-8, 7]), deinterleaving
 * and the Viterbi over DCI_LENGTH + 16 steps into decoded_output, of which
 * 2 + ((16 + DCI_LENGTH) >> 3) bytes are zeroed first.  Returns 0, or -1 for what the reference's
 * buffers do not hold (aggregation_level > 3, DCI_LENGTH > 45) and without a device; crc, when not
 * null, receives crc16(decoded, DCI_LENGTH) ^ the 16 bits that follow (the RNTI of a match). */
int oai4g_dci_decoding(uint8_t DCI_LENGTH, uint8_t aggregation_level, const int8_t *e, uint8_t *decoded_output);
int oai4g_dci_decoding_crc(uint8_t DCI_LENGTH, uint8_t aggregation_level, const int8_t *e, uint8_t *decoded_output,
                           uint16_t *crc);
/* rx_pbch from the quantised soft bits on (PHY/LTE_TRANSPORT/pbch.c:975-1043): llr holds pbch_E =
 * 1920 (1728 with the extended prefix) soft bits, all of them read; quarter frame_mod4 is
 * unscrambled (pbch_unscrambling :785, c_init = Nid_cell), then the rate-matching receive,
 * deinterleaving, the Viterbi over 40 steps and the CRC16.  decoded_output receives the three MIB
 * bytes, reversed as the reference returns them.  Returns the number of eNB antennas 1 / 2 / 4 the
 * CRC mask names, or -1: the reference's -1 when the CRC matches none of them (oai4g_last_error()
 * is then empty), and a refused call (frame_mod4 > 3, no device; oai4g_last_error() says which). */
int oai4g_pbch_decode(const int8_t *llr, const oai4g_frame_parms_t *frame_parms, uint8_t frame_mod4,
                      uint8_t decoded_output[3]);
/* n PBCH decodes in one launch, device pointers: d_llr [n][pbch_E], d_frame_mod4 [n], d_out [n][4] =
 * the three MIB bytes as above and the antenna count (1 / 2 / 4, 0xFF when the CRC matches none).
 * Asynchronous on `stream`.  Returns 0 or -1. */
int oai4g_pbch_decode_batch(const int8_t *d_llr, int n, const oai4g_frame_parms_t *frame_parms,
                            const uint8_t *d_frame_mod4, uint8_t *d_out, void *stream);

/* The soft bits of rx_pdcch after channel compensation (dci.c:1852-1897) as one fixed gather with a
 * sign per (frame parameters, subframe, num_pdcch_symbols): pdcch_llr (:603, clip to [-32, 31], re
 * before im), pdcch_demapping (:342, the REG walk around the PCFICH / PHICH REGs with its two RE
 * counters), pdcch_deinterleaving (:449, the cell-id cyclic shift and the 32-column permutation on
 * quadruplets) and pdcch_unscrambling (:1932, c_init = (subframe << 9) + Nid_cell, negation where the
 * Gold bit is 0, over 72 nCCE soft bits).  table[i] for soft bit i of e_rx: the int16 index into
 * rxdataF_comp (plane 0, symbol * 12 * N_RB_DL int32 per symbol; symbol 0 holds its 8 non-pilot REs
 * per RB packed) | negate << 31, or 0xFFFFFFFF where nothing is mapped (the soft bit is 0).  Returns
 * the number of soft bits 8 * Mquad (cap must hold them), or -1: 4 TX ports (the reference's demapping
 * leaves them "LATER") and every geometry oai4g_generate_dci_top refuses. */
int oai4g_pdcch_soft_bit_table(const oai4g_frame_parms_t *frame_parms, uint8_t subframe, uint8_t num_pdcch_symbols,
                               uint32_t *table, uint32_t cap);
/* the gather itself on host buffers: e_rx receives 8 * Mquad soft bits.  Returns their number or -1. */
int oai4g_pdcch_soft_bits(const int32_t *rxdataF_comp, const oai4g_frame_parms_t *frame_parms, uint8_t subframe,
                          uint8_t num_pdcch_symbols, int8_t *e_rx);
/* CCEind of every candidate of one dci_decoding_procedure0 call (dci.c:2576-2624), in its order: the
 * common space from CCE 0, the UE-specific space from Yk of the C-RNTI and subframe; returns their
 * number (0 when nCCE < 2^L), or -1. */
int oai4g_pdcch_candidates(const oai4g_frame_parms_t *frame_parms, uint8_t num_pdcch_symbols, uint8_t subframe,
                           uint16_t crnti, int do_common, uint8_t L, uint16_t *cce, int cap);
/* dci_decoding_procedure0 (dci.c:2547) with the reference's argument list; lte_ue_pdcch_vars is
 * spelled out as e_rx, num_pdcch_symbols, crnti and nCCE (the nCCE[subframe] slot).  Every candidate
 * of the call is decoded in one launch; the skip / match / acceptance rules then run in candidate
 * order, so the result is the reference's (a skipped candidate's decode is ignored; the decode has no
 * side effects).  dci_alloc must have room for *dci_cnt + 1 entries.  Returns 0, or -1. */
int oai4g_dci_decoding_procedure0(const int8_t *e_rx, uint8_t num_pdcch_symbols, uint16_t crnti, uint8_t *nCCE,
                                  int do_common, uint8_t subframe, oai4g_dci_alloc_t *dci_alloc,
                                  const oai4g_frame_parms_t *frame_parms, uint8_t mi, uint16_t si_rnti, uint16_t ra_rnti,
                                  uint8_t L, uint8_t format_si, uint8_t format_ra, uint8_t format_c, uint8_t sizeof_bits,
                                  uint8_t sizeof_bytes, uint8_t *dci_cnt, uint8_t *format0_found, uint8_t *format_c_found,
                                  uint32_t *CCEmap0, uint32_t *CCEmap1, uint32_t *CCEmap2);

/* Batched, device-resident DCI search.  A plan entry is one dci_decoding_procedure0 call of
 * dci_decoding_procedure (dci.c:2788); between entries the search ends when CCEmap0 == 0xffff or both
 * found flags are set, and after an entry with stop_if_found when it advanced dci_cnt (:3266). */
typedef struct {
  uint8_t do_common, L, sizeof_bits, sizeof_bytes, format_si, format_ra, format_c, stop_if_found;
} oai4g_pdcch_plan_t;
#define OAI4G_PDCCH_MAX_DCI 8
typedef struct {
  uint8_t dci_cnt, format0_found, format_c_found;
  uint8_t overflow;                          /* 1: more than OAI4G_PDCCH_MAX_DCI matches; the further ones only marked their CCEs */
  int32_t nCCE;                              /* nCCE[subframe] where an accepted DCI stored it, else -1 */
  uint32_t CCEmap[3];
  oai4g_dci_alloc_t dci[OAI4G_PDCCH_MAX_DCI];   /* the first dci_cnt are the found DCIs */
} oai4g_pdcch_rx_result_t;
typedef struct oai4g_pdcch_rx_config oai4g_pdcch_rx_config_t;
/* derives, per subframe index 0..9, the soft-bit gather table and the candidate list in plan order */
oai4g_pdcch_rx_config_t *oai4g_pdcch_rx_config_create(const oai4g_frame_parms_t *frame_parms, uint8_t num_pdcch_symbols,
                                                      uint16_t crnti, uint16_t si_rnti, uint16_t ra_rnti,
                                                      const oai4g_pdcch_plan_t *plan, int n_plan);
void oai4g_pdcch_rx_config_destroy(oai4g_pdcch_rx_config_t *cfg);
/* the candidates of subframe index `subframe` in plan order (tests): cce[i], plan_entry[i]; returns their
 * number (cap entries are written at most) */
int oai4g_pdcch_rx_candidates(const oai4g_pdcch_rx_config_t *cfg, uint8_t subframe, uint16_t *cce, uint8_t *plan_entry,
                              int cap);
/* d_comp [n_sf][num_pdcch_symbols * 12 * N_RB_DL] int32 (device), subframe i of the batch has subframe
 * index (first_subframe + i) mod 10; one launch decodes every candidate of every subframe, a second
 * stage (one lane per subframe) walks them in plan order; d_out [n_sf] (device).  Asynchronous on
 * `stream`.  Returns 0 or -1. */
int oai4g_pdcch_rx_batch(oai4g_pdcch_rx_config_t *cfg, const int32_t *d_comp, int n_sf, int first_subframe,
                         oai4g_pdcch_rx_result_t *d_out, void *stream);
/* The same search behind oai4g_pdcch_front_batch: d_comp [n_sf][3 * 12 * N_RB_DL], d_cfi [n_sf] the count
 * rx_pcfich found for each subframe (device; it never visits the host).  cfg[n - 1] is the configuration of
 * n symbols (same frame, RNTIs and plan); subframe i, of index (first_subframe + i * subframe_step) mod 10,
 * gets what oai4g_pdcch_rx_batch gives with cfg[d_cfi[i] - 1] on its first d_cfi[i] * 12 * N_RB_DL words (a
 * count outside 1..3 finds nothing).  The records live in cfg[2].  Asynchronous on `stream`.  Returns 0 or -1. */
int oai4g_pdcch_rx_batch_detected(oai4g_pdcch_rx_config_t *const cfg[3], const int32_t *d_comp, const uint8_t *d_cfi,
                                  int n_sf, int first_subframe, int subframe_step, oai4g_pdcch_rx_result_t *d_out,
                                  void *stream);

/* ---------------- UE control receive front end: IQ and estimates to the compensated symbols ---------------- */
/* rx_pdcch up to pdcch_llr (PHY/LTE_TRANSPORT/dci.c:1689-1830, is_secondary_ue = 0, MU_RECEIVER off) and
 * rx_pcfich (pcfich.c:231) for one subframe, always over three control symbols (dci.c:1704):
 * pdcch_extract_rbs_single / _dual (:903, 1120), pdcch_channel_level (:643), the log2_maxh rule (:1751-1757,
 * with its transposed read of avgP: 2 TX x 1 RX looks at port 0 only, 1 TX x 2 RX at antenna 0 only),
 * pdcch_channel_compensation (:1371), pdcch_detection_mrc (:1591), pdcch_siso / pdcch_alamouti (:1632, 1654).
 * rxdataF[a]: the FEP rows [nsymb][N] of receive antenna a; dl_ch_estimates[(p << 1) + a]: the estimate rows
 * [nsymb][N] of port p at antenna a (rows 0..2 are read, row 0 alone unless high_speed_flag == 1).  Outputs:
 * rxdataF_comp, plane 0, 3 * 12 * N_RB_DL words in the layout oai4g_pdcch_soft_bit_table documents (words
 * 8 N_RB_DL .. 12 N_RB_DL - 1, which the reference never defines, are 0); log2_maxh; num_pdcch_symbols as
 * rx_pcfich finds it (1..3).  diag_planes, when not null, receives the four compensated planes
 * [(p << 1) + a][3 * 12 * N_RB_DL] before MRC (planes of absent ports / antennas are 0).  rho is not
 * computed.  Returns 0, or -1: 4 TX ports, the extended prefix, more than 2 receive antennas, a mimo_mode
 * other than SISO / ALAMOUTI, ALAMOUTI with one port. */
int oai4g_rx_pdcch_front(int32_t *const *rxdataF, int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *frame_parms,
                         uint8_t nb_antennas_rx, uint8_t subframe, uint8_t mimo_mode, uint32_t high_speed_flag,
                         int32_t *rxdataF_comp, uint8_t *log2_maxh, uint8_t *num_pdcch_symbols, int32_t *diag_planes);
/* rx_pcfich (pcfich.c:231) on plane 0 of rxdataF_comp (the packed symbol 0, 8 * N_RB_DL words are read): the
 * 16 REs at pcfich_reg * 4, pcfich_unscrambling, the three correlations; the first strictly larger metric
 * from -16384 on wins, 3 when none exceeds it.  mimo_mode is the reference's argument and, as there (its
 * ALAMOUTI branch is commented out, pcfich.c:270-295), has no effect on the result: plane 0 is already combined.
 * Returns 1..3, or -1 (refused as above). */
int oai4g_rx_pcfich(const oai4g_frame_parms_t *frame_parms, uint8_t subframe, const int32_t *rxdataF_comp, uint8_t mimo_mode);
/* rx_pdcch whole (dci.c:1689): the front end, then oai4g_pdcch_soft_bits with the detected count.  e_rx
 * receives the soft bits, *num_pdcch_symbols the count.  Returns the number of soft bits, or -1. */
int oai4g_rx_pdcch(int32_t *const *rxdataF, int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *frame_parms,
                   uint8_t nb_antennas_rx, uint8_t subframe, uint8_t mimo_mode, uint32_t high_speed_flag, int8_t *e_rx,
                   uint8_t *num_pdcch_symbols);
/* The batched front end, device pointers, one launch: d_rxdataF [n_sf][nb_antennas_rx][nsymb][N] as
 * oai4g_fep_batch writes it, d_est[(p << 1) + a] [n_sf][nsymb][N] as oai4g_chest_batch writes the plane of
 * port p at antenna a, subframe i of index (first_subframe + i * subframe_step) mod 10 -> d_comp
 * [n_sf][3 * 12 * N_RB_DL], d_cfi [n_sf], d_log2_maxh [n_sf].  Asynchronous on `stream`.  Returns 0 or -1. */
typedef struct oai4g_pdcch_front_config oai4g_pdcch_front_config_t;
oai4g_pdcch_front_config_t *oai4g_pdcch_front_config_create(const oai4g_frame_parms_t *frame_parms, uint8_t nb_antennas_rx,
                                                            uint8_t mimo_mode, uint32_t high_speed_flag,
                                                            uint8_t first_subframe, uint8_t subframe_step);
void oai4g_pdcch_front_config_destroy(oai4g_pdcch_front_config_t *cfg);
int oai4g_pdcch_front_batch(const oai4g_pdcch_front_config_t *cfg, int n_sf, const int32_t *d_rxdataF,
                            const int32_t *const d_est[4], int32_t *d_comp, uint8_t *d_cfi, uint8_t *d_log2_maxh,
                            void *stream);

/* ---------------- UE PBCH receive front end: IQ and estimates to the MIB ---------------- */
/* rx_pbch up to the quantised soft bits (PHY/LTE_TRANSPORT/pbch.c:876-973, normal prefix) on subframe 0:
 * symbols 7..10, each with its own level and shift.  pbch_extract (:434: the 72 centre subcarriers, DC skipped
 * on the receive side only; on symbols 7 and 8 the REs at nushift % 3 + {0, 3, 6, 9} of every 12 are dropped
 * and 8 per RB packed, with one port too), pbch_channel_level (:537: all four ports' planes are looked at, the
 * sum over a region's 72 words divided by 72 also where only 48 are defined), log2_maxh = 3 + log2_approx / 2,
 * pbch_channel_compensation (:610), pbch_detection_mrc (:719), pbch_alamouti (:816) and pbch_quantize (:854).
 * Argument conventions of oai4g_rx_pdcch_front: rxdataF[a] rows [nsymb][N] (rows 7..10 are read),
 * dl_ch_estimates[(p << 1) + a] for the nb_ports (1 or 2) estimated ports (rows 7..10 when high_speed_flag == 1,
 * else row 0).  nb_ports is the caller's, not frame_parms': the UE does not know the eNB's count before the
 * MIB.  ALAMOUTI with one estimated port is accepted, as in the reference: port 1's plane is 0 and the result
 * equals SISO.  Outputs, each may be null: rxdataF_comp, plane 0 after combining, 4 * 72 words (words 48..71
 * of the first two regions, which the reference never writes, are 0); log2_maxh[4]; llr, the 480 soft bits
 * (96 + 96 + 144 + 144); diag_planes, the four compensated planes [(p << 1) + a][288] before MRC.  Returns 0,
 * or -1: the extended prefix (the reference's own quantise lengths overrun pbch_E there), more than 2
 * estimated ports, more than 2 receive antennas, a mimo_mode other than SISO / ALAMOUTI. */
int oai4g_rx_pbch_front(int32_t *const *rxdataF, int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *frame_parms,
                        uint8_t nb_antennas_rx, uint8_t nb_ports, uint8_t mimo_mode, uint32_t high_speed_flag,
                        int32_t *rxdataF_comp, uint8_t log2_maxh[4], int8_t *llr, int32_t *diag_planes);
/* rx_pbch whole (pbch.c:876): the front end, its 480 soft bits at llr[frame_mod4 * 480] of a cleared
 * 1920-byte buffer, then oai4g_pbch_decode.  Returns as oai4g_pbch_decode does (1 / 2 / 4, or -1 with
 * oai4g_last_error() empty when the CRC matches none); also -1 for frame_mod4 > 3 and what the front refuses. */
int oai4g_rx_pbch(int32_t *const *rxdataF, int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *frame_parms,
                  uint8_t nb_antennas_rx, uint8_t nb_ports, uint8_t mimo_mode, uint32_t high_speed_flag,
                  uint8_t frame_mod4, uint8_t decoded_output[3]);
/* The batched front end, device pointers, one launch for n subframes 0: d_rxdataF [n][nb_antennas_rx][nsymb][N]
 * as oai4g_fep_batch writes it, d_est[(p << 1) + a] [n][nsymb][N] as oai4g_chest_batch writes it -> d_llr
 * [n][2][480], the soft bits under SISO and under ALAMOUTI (the combining is their only difference), and
 * d_log2_maxh [n][4].  Asynchronous on `stream`.  Returns 0 or -1. */
typedef struct oai4g_pbch_front_config oai4g_pbch_front_config_t;
oai4g_pbch_front_config_t *oai4g_pbch_front_config_create(const oai4g_frame_parms_t *frame_parms, uint8_t nb_antennas_rx,
                                                          uint8_t nb_ports, uint32_t high_speed_flag);
void oai4g_pbch_front_config_destroy(oai4g_pbch_front_config_t *cfg);
int oai4g_pbch_front_batch(const oai4g_pbch_front_config_t *cfg, int n, const int32_t *d_rxdataF,
                           const int32_t *const d_est[4], int8_t *d_llr, uint8_t *d_log2_maxh, void *stream);
/* pbch_detection's search (PHY/LTE_TRANSPORT/initial_sync.c:135-161) over d_llr as above: frame_mod4 0..3,
 * for each SISO then ALAMOUTI; the first hypothesis whose CRC names 1 or 2 antennas wins (one naming 4 does
 * not stop the search).  The eight decodes of every subframe run in one launch (a quarter's 480 soft bits
 * alone: the rest of the reference's buffer is 0), a second, one lane per subframe, picks.  d_out [n]
 * (device).  The configuration keeps the constants of its cell and the decode records; one launch at a time
 * per configuration.  Asynchronous on `stream`, no host visit.  Returns 0 or -1. */
typedef struct {
  uint8_t tx_ant;            /* 1 / 2, or 0xFF: no hypothesis decoded */
  uint8_t frame_mod4, mimo_mode;
  uint8_t mib[3];            /* as oai4g_pbch_decode returns them */
  uint8_t pad[2];
} oai4g_pbch_detect_t;
int oai4g_pbch_detect_batch(oai4g_pbch_front_config_t *cfg, int n, const int8_t *d_llr, oai4g_pbch_detect_t *d_out,
                            void *stream);

/* ---------------- UE initial cell search: PSS timing ---------------- */
/* FDD with the normal prefix, the hypothesis initial_sync tries first (PHY/LTE_TRANSPORT/initial_sync.c:274-372)
 * and the only one the PBCH front accepts.  Refused (-1 / null, oai4g_last_error says which): TDD, the extended
 * prefix, more than 2 receive antennas, N_RB_DL 15 (lte_sync_time_init's switch, lte_sync_time.c:157-186, has no
 * 256-point case and leaves all-zero replicas), N_RB_DL 75 (idft1536) and every size the switch does not name.
 *
 * lte_sync_time_init's time-domain replicas (PHY/LTE_ESTIMATION/lte_sync_time.c:143-292): for Nid2 = 0, 1, 2 the 72
 * entries of primary_synch<Nid2> (PHY/LTE_REFSIG/primary_synch.h), each component >> 2, from bin N - 36 on, DC
 * skipped at the wrap (:151-154), inverse DFT of N = ofdm_symbol_size points with scale 1.  out [3][N] packed int16
 * pairs.  Host only: no device is needed. */
int oai4g_lte_sync_time_replicas(const oai4g_frame_parms_t *frame_parms, int32_t *out);
/* lte_sync_time (lte_sync_time.c:357-517), bit-exact.  length = 5 samples_per_tti; for n = 0, 4, ... < length, every
 * sequence s and antenna: dot_product(replica_s, rxdata + n, N, 15) (PHY/TOOLS/cdot_prod.c:40-118: per tap
 * (xr yr + xi yi) >> 15 and (xr yi + xi (int16)(-yr)) >> 15 into two wrapping 32-bit sums, saturated to int16 at
 * the end) and the same at n + length, the antennas added in int16 with wrap (:428-435); n >= length - N adds
 * nothing (:420).  abs32 = re^2 + im^2 in int (:348-351), metric (abs32 >> 1) + (abs32 of the second half >> 1)
 * compared as unsigned with peak_val from 0, strictly greater, n ascending then s (:477-489): all-zero input
 * gives position 0, source 0.
 *
 * The batched form: d_rx [n][nb_antennas_rx][10 samples_per_tti] frames, d_peak [n] {peak_pos, peak_val, Nid2},
 * d_corr null or [n][3][2 length], where only every fourth entry is written: sync_corr_ue0..2 after their abs32
 * (:470-475).  Asynchronous on `stream`, no host visit.  Returns 0 or -1. */
typedef struct oai4g_sync_config oai4g_sync_config_t;
oai4g_sync_config_t *oai4g_sync_config_create(const oai4g_frame_parms_t *frame_parms, uint8_t nb_antennas_rx);
void oai4g_sync_config_destroy(oai4g_sync_config_t *cfg);
int oai4g_sync_time_batch(oai4g_sync_config_t *cfg, int n, const int32_t *d_rx, int32_t *d_peak, int32_t *d_corr,
                          void *stream);
/* The drop-in on one frame in host memory: rxdata[aa] holds 10 samples_per_tti words; returns peak_pos (or -1), the
 * sequence in *eNB_id, the winning metric in *peak_val; sync_corr, when not null, receives [3][10 samples_per_tti]. */
int oai4g_lte_sync_time(int32_t *const *rxdata, const oai4g_frame_parms_t *frame_parms, uint8_t nb_antennas_rx, int *eNB_id,
                        uint32_t *peak_val, int32_t *sync_corr);

/* ---------------- UE initial cell search: FEP at an offset, SSS cell id ---------------- */
/* slot_fep (PHY/MODULATION/slot_fep.c:40-156) of `nsym` symbols from symbol 0 of slot `first_slot` on, with
 * sample_offset = d_offset[f * offset_stride] of frame f, a device value: the windows are those of
 * oai4g_slot_fep_offset, its - rx_offset % 4 alignment included (:118), taken modulo the frame length; a window that
 * runs past the frame's end reads on from its start, where the reference's wrap extension holds that copy
 * (:123-126).  d_rx [n][nb_antennas_rx][10 samples_per_tti]; symbol k of the run lands in row k of
 * d_rxF + f * frame_stride + antenna * symbols_per_tti * N, the layout oai4g_fep_batch writes when frame_stride is
 * 0 (= nb_antennas_rx * symbols_per_tti * N words).  1 <= nsym <= symbols_per_tti: the PBCH stage's fifteenth symbol
 * (symbol 0 of slot 2, initial_sync.c:87-92) is a second call, into the row the estimation reads it from.
 * Scope and refusals as above.  Asynchronous on `stream`.  Returns 0 or -1. */
int oai4g_fep_offset_batch(const oai4g_frame_parms_t *frame_parms, int n, int nb_antennas_rx, const int32_t *d_rx,
                           const int32_t *d_offset, uint32_t offset_stride, uint8_t first_slot, int nsym, int32_t *d_rxF,
                           size_t frame_stride, void *stream);
/* What the search knows of a frame's cell.  status 0: found; 1: "SSS error condition" (initial_sync.c:373-376), the
 * frame has no cell (Nid_cell -1). */
typedef struct {
  int32_t Nid_cell, rx_offset, metric, flip, phase, status;
} oai4g_cell_t;
/* initial_sync's offset arithmetic and rx_sss per frame, from d_peak on the device (initial_sync.c:310-362, FDD,
 * normal prefix): sync_pos2 = peak_pos - nb_prefix_samples (plus the frame length when negative), sync_pos_slot =
 * samples_per_tti / 2 - N - nb_prefix_samples, rx_offset = sync_pos2 - sync_pos_slot (plus the frame length when
 * negative); rx_sss runs only when 0 <= sync_pos2 - sync_pos_slot < frame - samples_per_tti / 2 (:353-354).
 * rx_sss (PHY/LTE_TRANSPORT/sss.c:222-391): slot_fep of symbols 5 and 6 of slot 0, then of slot 10, at rx_offset;
 * pss_sss_extract (:157-215: 72 words per symbol, rxF[N - 36 ..] for three RBs, then rxF[1 ..]); pss_ch_est
 * (:93-154) over the 62 words from word 5 against &primary_synch<Nid2>[10], every >> 15 and (int16_t) cast where
 * the reference has them (:132-137), antenna 0 in place and antenna 1 added in int16; the search (:356-388) over
 * flip 0..1, phase 0..6 (phase_re / phase_im, :218-219) and Nid1 0..167 of the sum of the 62 terms
 * (int16_t)(d0[i] A0 + d5[i] A5), A = ((phase_re re) >> 19) - ((phase_im im) >> 19), flip 1 swapping the tables; the
 * first strictly greater metric from -99999999 wins.  With flip = 1 the reported rx_offset has the half frame added
 * (initial_sync.c:361-362).  d_cell [n].  Asynchronous on `stream`, no host visit.  Returns 0 or -1. */
int oai4g_sss_batch(oai4g_sync_config_t *cfg, int n, const int32_t *d_rx, const int32_t *d_peak, oai4g_cell_t *d_cell,
                    void *stream);
/* The same without the slot_fep calls, on the caller's rows d_rows [n][nb_antennas_rx][4][N]: symbols 5 and 6 of slot
 * 0, then of slot 10.  The forward DFT's last level scales by 1/sqrt(2) or 1/2, which keeps slot_fep's output at or
 * below 23170 per component, so the wraps of pss_ch_est's (int16_t) casts can only be reached with rows given
 * directly. */
int oai4g_sss_rows_batch(oai4g_sync_config_t *cfg, int n, const int32_t *d_rows, const int32_t *d_peak, oai4g_cell_t *d_cell,
                         void *stream);
/* The drop-in for rx_sss on one frame in host memory, rxdata[aa] of 10 samples_per_tti words: Nid2 is
 * lte_ue_common_vars.eNb_id, rx_offset is phy_vars_ue->rx_offset.  Returns the Nid_cell rx_sss leaves in the frame
 * parameters (or -1), and *tot_metric, *flip_max, *phase_max. */
int oai4g_rx_sss(int32_t *const *rxdata, const oai4g_frame_parms_t *frame_parms, uint8_t nb_antennas_rx, uint8_t Nid2,
                 int rx_offset, int32_t *tot_metric, uint8_t *flip_max, uint8_t *phase_max);
/* initial_sync's first hypothesis (PHY/LTE_TRANSPORT/initial_sync.c:290-372: FDD, normal prefix) on one frame in host
 * memory: oai4g_lte_sync_time (:305), the offset arithmetic (:310-354), oai4g_rx_sss (:358), the frame parameters
 * of the found cell (:359-365), pbch_detection (:57-161): slot_fep of slots 0 and 1 and of symbol 0 of slot 2 at
 * rx_offset (:69-92), the channel estimation of nb_ports (1 or 2) ports, oai4g_rx_pbch_front and the
 * eight-hypothesis search.  frame_parms gives N_RB_DL; phy_adjust_gain and the rx_power / lte_ue_measurements
 * bookkeeping (:320-341, :94-109) are not part of it.  Returns 0 with *out filled, or -1: no PBCH found
 * (oai4g_last_error() empty; Nid_cell and rx_offset are still reported), the SSS error condition (Nid_cell -1), or a
 * refused call.
 * A batch of frames of unknown cells ends on the device at oai4g_sss_batch's d_cell: the estimation and PBCH
 * configurations are per cell, so the caller reads those few bytes, groups the frames by cell, and runs
 * oai4g_fep_offset_batch -> oai4g_chest_batch -> oai4g_pbch_front_batch / oai4g_pbch_detect_batch per group. */
typedef struct {
  int32_t Nid_cell, rx_offset;
  uint8_t tx_ant;            /* 1 / 2, or 0xFF: no PBCH found */
  uint8_t frame_mod4, mimo_mode;
  uint8_t mib[3];
  uint8_t pad[2];
} oai4g_initial_sync_t;
int oai4g_initial_sync(int32_t *const *rxdata, const oai4g_frame_parms_t *frame_parms, uint8_t nb_antennas_rx, uint8_t nb_ports,
                       uint32_t high_speed_flag, oai4g_initial_sync_t *out);

/* ---------------- UE PHICH reception ---------------- */
/* rx_phich's numeric core (PHY/LTE_TRANSPORT/phich.c:1112-1346, normal prefix, normal duration): the 12
 * scrambling signs of c_init = ((subframe + 1)(Nid_cell + 1) << 9) + Nid_cell, the 24 signs d of nseq_PHICH
 * (:1131-1222), and HI16 += x d over the 8 int16 at word phich_reg[ngroup_PHICH][quad] * 4 of plane 0 of the
 * PDCCH front's rxdataF_comp (the packed symbol 0, 8 * N_RB_DL words are read), accumulated in int16_t as the
 * reference does: it wraps after every term.  *HI16, when not null, receives the sum.  Group and sequence come
 * from oai4g_phich_group_seq; the HARQ bookkeeping behind the decision is the caller's.  Returns 1 (NACK:
 * HI16 > 0), 0 (ACK), or -1: what oai4g_generate_phich refuses, a group outside
 * oai4g_generate_phich_reg_mapping's, nseq_PHICH > 7. */
int oai4g_rx_phich(const oai4g_frame_parms_t *frame_parms, uint8_t subframe, const int32_t *rxdataF_comp,
                   uint8_t ngroup_PHICH, uint8_t nseq_PHICH, int16_t *HI16);
/* The batched form behind oai4g_pdcch_front_batch: d_comp [n_sf][3 * 12 * N_RB_DL] as it writes it, subframe
 * slot i of index (first_subframe + i * subframe_step) mod 10; d_items [n_items] (device) name a slot, a group
 * and a sequence each; d_out [n_items] in one launch.  An item outside the batch, the mapping or nseq > 7
 * gives {0, 0xFF}.  The signs and word offsets of every (subframe index, group, sequence) are a table of the
 * configuration.  Asynchronous on `stream`.  Returns 0 or -1. */
typedef struct {
  uint32_t slot;
  uint8_t ngroup, nseq, pad[2];
} oai4g_phich_rx_item_t;
typedef struct {
  int16_t HI16;
  uint8_t nack;              /* 1 NACK, 0 ACK, 0xFF: refused item */
  uint8_t pad;
} oai4g_phich_rx_out_t;
typedef struct oai4g_phich_rx_config oai4g_phich_rx_config_t;
oai4g_phich_rx_config_t *oai4g_phich_rx_config_create(const oai4g_frame_parms_t *frame_parms, uint8_t first_subframe,
                                                      uint8_t subframe_step);
void oai4g_phich_rx_config_destroy(oai4g_phich_rx_config_t *cfg);
int oai4g_phich_rx_batch(const oai4g_phich_rx_config_t *cfg, const int32_t *d_comp, int n_sf,
                         const oai4g_phich_rx_item_t *d_items, int n_items, oai4g_phich_rx_out_t *d_out, void *stream);

/* ---------------- UE PDSCH demodulation (second half) ---------------- */
/* rx_pdsch (PHY/LTE_TRANSPORT/dlsch_demodulation.c:82) over the PDSCH symbols of one subframe as
 * dlsim runs it (dlsim.c:3188-3260): dlsch_extract_rbs_single (:3167), dlsch_channel_level (:2777)
 * -> log2_maxh, dlsch_channel_compensation (:801) and dlsch_qpsk / 16qam / 64qam_llr
 * (dlsch_llr_computation.c:636, 688, 810).  Transmission mode 1 (one TX port), one receive
 * antenna, every N_RB_DL (the odd 15 / 25 PRB extraction around the DC carrier included; a
 * subframe whose extraction would read slots the reference leaves unwritten returns -1), the
 * first PDSCH symbol without pilots.  rxdataF and dl_ch_estimates are one subframe, [nsymb][N]
 * each (estimate of subcarrier 12 rb + i at entry 5 + 12 rb + i of its symbol, the layout of the
 * reference's estimator and of dlsim's perfect-CE mode, dlsim.c:2935-2966).  Writes the LLR
 * stream (not unscrambled) and log2_maxh; returns its length or -1. */
int oai4g_rx_pdsch_siso(const oai4g_frame_parms_t *frame_parms, const int32_t *rxdataF, const int32_t *dl_ch_estimates,
                        const uint32_t rb_alloc[4], uint8_t Qm, uint8_t num_pdcch_symbols, uint8_t subframe,
                        int16_t *llr, uint8_t *log2_maxh);
/* dlsch_unscrambling (dlsch_scrambling.c:99, decl LTE_TRANSPORT/proto.h): llr[k] *= 2 c(k) - 1
 * for k < 32 (1 + G / 32) with c_init = rnti 2^14 + q 2^13 + (Ns / 2) 2^9 + Nid_cell, or with
 * mbsfn_flag != 0 (PMCH) c_init = (Ns / 2) 2^9 + Nid_cell_mbsfn (:115-118).  The reference reads
 * rnti from its LTE_UE_DLSCH_t. */
void oai4g_dlsch_unscrambling(const oai4g_frame_parms_t *frame_parms, int mbsfn_flag, uint16_t rnti, int G,
                              int16_t *llr, uint8_t q, uint8_t Ns);
/* Batched demodulation: n_sf subframes (subframe index first_subframe + i * subframe_step mod 10)
 * of rxdataF and per-symbol channel estimates ([n_sf][nsymb][N] int32 each, device) -> LLR
 * streams [n_sf][oai4g_rx_llr_stride] int16 (device), unscrambled (q = 0, Ns = 2 subframe) when
 * unscramble != 0.  The demodulator is elementwise per RE after the per-subframe channel level. */
typedef struct oai4g_rx_config oai4g_rx_config_t;
oai4g_rx_config_t *oai4g_rx_config_create(const oai4g_frame_parms_t *frame_parms, const uint32_t rb_alloc[4], uint8_t Qm,
                                          uint8_t num_pdcch_symbols, uint16_t rnti, uint8_t first_subframe,
                                          uint8_t subframe_step);
void oai4g_rx_config_destroy(oai4g_rx_config_t *cfg);
int oai4g_rx_llr_count(const oai4g_rx_config_t *cfg, int subframe_index);
size_t oai4g_rx_llr_stride(const oai4g_rx_config_t *cfg);
int oai4g_rx_batch(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_dl_ch_estimates,
                   int16_t *d_llr, int unscramble, void *stream);

/* TM3 (LARGE_CDD, two TX ports) with dlsim's UE (rx_pdsch with dual_stream_flag = 0,
 * dlsch_demodulation.c:82-800): dlsch_extract_rbs_dual, dlsch_channel_level_TM3 + log2_maxh,
 * dlsch_channel_compensation_TM3 (prec2A_TM3), dlsch_detection_mrc over nb_rx (1-2) receive
 * antennas, then codeword 0's LLRs: the single-stream 16 / 64-QAM LLRs for Qm0 4 / 6 (the reference
 * computes no codeword-1 LLRs there); for Qm0 = 2 the interference-aware dlsch_qpsk_qpsk_llr /
 * dlsch_qpsk_16qam_llr / dlsch_qpsk_64qam_llr against codeword 1 of modulation order Qm1
 * (dlsch_demodulation.c:643-690, dlsch_llr_computation.c:983, :1232, :1516).  Drop-in on host
 * buffers: rxdataF[a] = [nsymb][N] per receive
 * antenna, dl_ch_estimates[p * 2 + a] = [nsymb][N] (the reference's dl_ch_estimates[(p << 1) + a]).
 * Returns the LLR count (not unscrambled) or -1. */
int oai4g_rx_pdsch_tm3(const oai4g_frame_parms_t *frame_parms, int nb_rx, const int32_t *const *rxdataF,
                       const int32_t *const *dl_ch_estimates, const uint32_t rb_alloc[4], uint8_t Qm0, uint8_t Qm1,
                       uint8_t mcs0, uint8_t num_pdcch_symbols, uint8_t subframe, int16_t *llr, uint8_t *log2_maxh);
/* Batched TM3 demodulation: d_rxdataF = [n_sf][nb_rx][nsymb][N] (the FEP batch output),
 * d_est = four planes [p * 2 + a][n_sf][nsymb][N] (channel estimation batches of ports 0 / 1 per
 * receive antenna) -> codeword 0's LLR streams [n_sf][oai4g_rx_llr_stride] (unscrambled when asked). */
oai4g_rx_config_t *oai4g_rx_config_create_tm3(const oai4g_frame_parms_t *frame_parms, const uint32_t rb_alloc[4],
                                              uint8_t Qm0, uint8_t Qm1, uint8_t mcs0, uint8_t num_pdcch_symbols,
                                              uint16_t rnti, uint8_t first_subframe, uint8_t subframe_step, uint8_t nb_rx);
int oai4g_rx_batch_tm3(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_est, int16_t *d_llr,
                       int unscramble, void *stream);

/* TM3 with both codewords QPSK (rx_pdsch, dlsch_demodulation.c:643-669): both precoded streams'
 * matched filters, dlsch_dual_stream_correlation (rho, rho2), the MRC of stream 0 and rho, and the
 * interference-aware dlsch_qpsk_qpsk_llr of each stream: codeword 0's LLRs in llr0, codeword 1's in
 * llr1 (same length, returned; -1 on error). */
int oai4g_rx_pdsch_tm3_2cw(const oai4g_frame_parms_t *frame_parms, int nb_rx, const int32_t *const *rxdataF,
                           const int32_t *const *dl_ch_estimates, const uint32_t rb_alloc[4], uint8_t mcs0,
                           uint8_t num_pdcch_symbols, uint8_t subframe, int16_t *llr0, int16_t *llr1,
                           uint8_t *log2_maxh);
/* batch of the same (configuration from oai4g_rx_config_create_tm3 with Qm0 = Qm1 = 2) */
int oai4g_rx_batch_tm3_2cw(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_est,
                           int16_t *d_llr0, int16_t *d_llr1, int unscramble, void *stream);
/* The same two TM3 batches from the pilot rows only: d_pil = four planes [p * 2 + a][n_sf][4][N][2]
 * written by oai4g_chest_batch_pilots (plane p * 2 + a from a port-p configuration over receive
 * antenna a). Every other estimate row is formed in the demodulator with
 * lte_dl_channel_estimation's temporal interpolation (lte_dl_channel_estimation.c:639-698), so the
 * 14-row estimate planes never reach memory. The LLRs are bit-identical. */
int oai4g_rx_batch_tm3_pilots(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_pil,
                              int16_t *d_llr, int unscramble, void *stream);
int oai4g_rx_batch_tm3_2cw_pilots(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_pil,
                                  int16_t *d_llr0, int16_t *d_llr1, int unscramble, void *stream);

/* TM2 (ALAMOUTI, two TX ports, mode1_flag 0) with dlsim's UE (rx_pdsch, dlsch_demodulation.c:82-800):
 * dlsch_extract_rbs_dual, dlsch_channel_level over both ports (log2_maxh = log2_approx(max avg) / 2),
 * dlsch_channel_compensation per (port, RX antenna), dlsch_detection_mrc over nb_rx (1-2),
 * dlsch_alamouti over pairs of extracted REs, dlsch_qpsk / 16qam / 64qam_llr.  Same buffers as the
 * TM3 entry points (estimate planes [p * 2 + a]).  Returns the LLR count (not unscrambled) or -1. */
int oai4g_rx_pdsch_tm2(const oai4g_frame_parms_t *frame_parms, int nb_rx, const int32_t *const *rxdataF,
                       const int32_t *const *dl_ch_estimates, const uint32_t rb_alloc[4], uint8_t Qm,
                       uint8_t num_pdcch_symbols, uint8_t subframe, int16_t *llr, uint8_t *log2_maxh);
oai4g_rx_config_t *oai4g_rx_config_create_tm2(const oai4g_frame_parms_t *frame_parms, const uint32_t rb_alloc[4],
                                              uint8_t Qm, uint8_t num_pdcch_symbols, uint16_t rnti,
                                              uint8_t first_subframe, uint8_t subframe_step, uint8_t nb_rx);
int oai4g_rx_batch_tm2(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_est, int16_t *d_llr,
                       int unscramble, void *stream);

/* TM4-6 single-layer precoding (mimo_mode OAI4G_UNIFORM_PRECODING11 .. OAI4G_PUSCH_PRECODING0: one
 * codeword on two ports) with dlsim's UE (rx_pdsch with dual_stream_flag = 0, dlsch_demodulation.c:518-533):
 * dlsch_extract_rbs_dual with pmi_ext, dlsch_channel_level over both ports (log2_maxh = log2_approx(max
 * avg) / 2, + 1 when dl_power_off == 1), dlsch_channel_compensation_TM56 (prec2A_TM56_128: h0 + w h1,
 * w = 1, -1, j, -j by the PRB's precoder), dlsch_detection_mrc over nb_rx (1-2), dlsch_qpsk / 16qam /
 * 64qam_llr.  Buffers as for oai4g_rx_pdsch_tm2.  OAI4G_PUSCH_PRECODING1 is refused as rx_pdsch refuses
 * it (:595-597); the precoder never comes from the mode's name.  precoded_cqi_dB is not computed and the
 * estimates are not overwritten.
 *
 * The subband of a PRB (pmi_rule):
 *   OAI4G_RX_PMI_UE  the reference UE's: (pmi_alloc >> ((prb >> 2) << 1)) & 3, 4-RB subbands at every
 *                    bandwidth (:3812).  It equals the transmitter's get_pmi only at 15 / 25 PRB or for a
 *                    pmi_alloc whose subbands are all equal.  pmi_alloc is an unsigned short promoted to
 *                    int there: counts of 16..31 (PRB 32..63) read 0; a count >= 32 (an allocated PRB
 *                    >= 64) is undefined in C and refused unless pmi_alloc == 0.  The drop-in uses it.
 *   OAI4G_RX_PMI_TX  oai4g_get_pmi's subbands (1 / 4 / 6 / 8 RBs): decodes this library's transmitter at
 *                    every bandwidth. */
enum { OAI4G_RX_PMI_UE = 0, OAI4G_RX_PMI_TX = 1 };
int oai4g_rx_pdsch_tm56(const oai4g_frame_parms_t *frame_parms, int nb_rx, const int32_t *const *rxdataF,
                        const int32_t *const *dl_ch_estimates, const uint32_t rb_alloc[4], uint8_t Qm,
                        uint8_t mimo_mode, uint16_t pmi_alloc, uint8_t dl_power_off, uint8_t num_pdcch_symbols,
                        uint8_t subframe, int16_t *llr, uint8_t *log2_maxh);
oai4g_rx_config_t *oai4g_rx_config_create_tm56(const oai4g_frame_parms_t *frame_parms, const uint32_t rb_alloc[4],
                                               uint8_t Qm, uint8_t mimo_mode, uint16_t pmi_alloc, int pmi_rule,
                                               uint8_t dl_power_off, uint8_t num_pdcch_symbols, uint16_t rnti,
                                               uint8_t first_subframe, uint8_t subframe_step, uint8_t nb_rx);
int oai4g_rx_batch_tm56(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_est, int16_t *d_llr,
                        int unscramble, void *stream);
/* from the pilot rows of oai4g_chest_batch_pilots (d_pil as for oai4g_rx_batch_tm3_pilots); bit-identical */
int oai4g_rx_batch_tm56_pilots(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_pil,
                               int16_t *d_llr, int unscramble, void *stream);

/* lte_dl_channel_estimation (PHY/LTE_ESTIMATION/lte_dl_channel_estimation.c:37, decl
 * LTE_ESTIMATION/defs.h; called by slot_fep.c:188 for the pilot symbols of every slot) with the
 * reference's defaults high_speed_flag = 1 (dlsim.c:2057), eNB_offset 0, one RX antenna: the
 * frequency interpolation of the conjugate-pilot products of port p (filt96_32.h filters) into row
 * `symbol` of dl_ch_estimates (subcarrier i of RB rb at 5 + 12 rb + i), then the temporal
 * interpolation of the rows between this pilot symbol and the previous one (symbol 0 closes rows
 * 12 / 13 of the previous subframe's pilot 11).  rxdataF / dl_ch_estimates = [nsymb][N] host
 * buffers of the subframe; N_RB_DL 6 / 15 / 25 / 50 / 100 (other sizes: the reference's "not
 * implemented" row of zeros; 15 PRB with its second-half start 1 + nushift + 3 p, :582).  The idft of the estimate into
 * dl_ch_estimates_time (:704-738) is the separate entry oai4g_dl_ch_estimates_time below, which the
 * shim calls after this one.  Returns 0 / -1. */
int oai4g_lte_dl_channel_estimation(const oai4g_frame_parms_t *frame_parms, const int32_t *rxdataF,
                                    int32_t *dl_ch_estimates, uint8_t Ns, uint8_t p, uint8_t l, uint8_t symbol);
/* The tail of lte_dl_channel_estimation (lte_dl_channel_estimation.c:704-738): for every RX antenna
 * aarx < nb_antennas_rx and port p < nb_antennas_tx_eNB (nb_antennas_tx when 0) whose plane
 * dl_ch_estimates[(p << 1) + aarx] is not NULL, dl_ch_estimates_time[(p << 1) + aarx] =
 * idft_N(plane from word 8, scale 1): words 8 .. N + 7 (row 0 then the first 8 words of row 1),
 * N = ofdm_symbol_size (log2_symbol_size outside 7..11: idft512, the switch's default).  The
 * input of the UE timing tracker (lte_adjust_sync.c:60-70).  Returns 0 / -1. */
int oai4g_dl_ch_estimates_time(const oai4g_frame_parms_t *frame_parms, int nb_antennas_rx,
                               const int32_t *const *dl_ch_estimates, int32_t *const *dl_ch_estimates_time);
/* Batched form: job j transforms d_est[j * est_stride + 8 ...] into d_time[j * time_stride ...]
 * (est_stride >= N + 8, time_stride >= N words); device pointers, async on `stream`. */
int oai4g_chest_time_batch(const oai4g_frame_parms_t *frame_parms, int n_jobs, const int32_t *d_est,
                           size_t est_stride, int32_t *d_time, size_t time_stride, void *stream);

/* lte_est_freq_offset (PHY/LTE_ESTIMATION/lte_est_freq_offset.c:104-193, called by slot_fep.c:211-217
 * at l = 4 - Ncp): antenna 0's plane dl_ch_estimates[0]; dl_ch_shift = 6 + log2_approx(
 * dl_channel_level(row l from RE 12)) / 2; omega as the reference computes it: its dot_product
 * (cdot_prod.c:40) of row l against the other pilot row (row 4 - Ncp when l = 0, else row 0) over
 * (N_RB_DL / 2 - 1) * 12 REs from RE (N_RB_DL / 2 + 1) * 12, doubled (int16 wrap per component) — the
 * lower-half product from RE 12 is overwritten through the omega_cpx alias (:150-166) and never
 * counts; freq_offset_est = (int)(atan2(omega) / 2 pi / 285.8 us
 * (normal CP) or 250 us); the first call (or one with reset != 0) stores it, later calls filter
 * (est * 2^10 + f * (32767 - 2^10)) >> 15.  The filter state is process-wide, as the reference's
 * static first_run.  The dot products run on the GPU; atan2 and the filter are the host's scalar
 * tail, as in the reference.  Returns 0, or -1 for l other than 0 / 4 - Ncp (freq_offset untouched). */
int oai4g_lte_est_freq_offset(int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *frame_parms, int l,
                              int *freq_offset, int reset);
/* Batched integer part: omega (re | im << 16) of n_jobs estimate planes d_est[j * est_stride ...]
 * (rows 0 .. 4 - Ncp present) into d_omega[j]; then oai4g_freq_offset_update applies the scalar
 * tail of one call per omega with a caller-held first_run (1 = the reference's first run). */
int oai4g_freq_offset_omega_batch(const oai4g_frame_parms_t *frame_parms, int n_jobs, const int32_t *d_est,
                                  size_t est_stride, int l, int32_t *d_omega, void *stream);
int oai4g_freq_offset_update(const oai4g_frame_parms_t *frame_parms, int32_t omega, int *freq_offset, int *first_run);
/* The six interpolation filters of pilot offset k = (nu + nushift) % 6 as the estimator uses them
 * (lte_dl_channel_estimation.c:105-180): fl, f2l2, f, f2, fr, f2r2 (filt96_32.h by formula). */
void oai4g_chest_filters(uint8_t k, int16_t out[6][24]);
/* The 25-PRB branch's DC pair (lte_dl_channel_estimation.c:116-173): filt24_k_dcr, filt24_(k+2)_dcl
 * (filt96_32.h table data). */
void oai4g_chest_dc_filters(uint8_t k, int16_t out[2][24]);
/* Batched estimation of every symbol of n_sf consecutive subframes (subframe index first_subframe
 * + i * subframe_step mod 10) in dlsim's order (dlsim.c:2907-2931): d_rxdataF = [n_sf][nsymb][N]
 * followed by the symbol 0 of the subframe after the batch (N more words), d_est = [n_sf][nsymb][N]
 * -- the rows rx_pdsch reads for each subframe (row 0 that subframe's own estimate). */
typedef struct oai4g_chest_config oai4g_chest_config_t;
oai4g_chest_config_t *oai4g_chest_config_create(const oai4g_frame_parms_t *frame_parms, uint8_t p,
                                                uint8_t first_subframe, uint8_t subframe_step);
void oai4g_chest_config_destroy(oai4g_chest_config_t *cfg);
/* Batch elements `subframes_per_element` subframes apart in d_rxdataF, the symbol 0 that closes rows
 * 12 / 13 `next_subframes` subframes after each element's start (default 1 / 1).  dlsim's BLER loop:
 * 2 / 1 (each trial's subframe followed by the next one); a receive antenna of an n-antenna FEP
 * batch: n / n (pass d_rxdataF + a nsymb N). */
int oai4g_chest_config_set_stride(oai4g_chest_config_t *cfg, uint32_t subframes_per_element, uint32_t next_subframes);
int oai4g_chest_batch(oai4g_chest_config_t *cfg, int n_sf, const int32_t *d_rxdataF, int32_t *d_est, void *stream);
/* The pilot rows only: per subframe the 5 frequency-interpolated rows P0..P4 of symbols 0, p1, p2,
 * p3 and the next subframe's symbol 0, stored as the pairs of consecutive rows: d_pil =
 * [n_sf][4][N][2] words, pair k at column j = (P_k[j], P_k+1[j]); columns below 12 N_RB + 16 (the
 * others are not written). They feed oai4g_rx_batch_tm3_pilots. */
int oai4g_chest_batch_pilots(oai4g_chest_config_t *cfg, int n_sf, const int32_t *d_rxdataF, int32_t *d_pil,
                             void *stream);
/* The batch chain without the estimate buffer: oai4g_chest_batch followed by oai4g_rx_batch, fused
 * (the estimate of each PDSCH RE is formed in LDS from the pilot rows), same LLRs; d_rxdataF as
 * for oai4g_chest_batch (n_sf subframes + the next symbol 0).  rx and ce describe the same frame
 * and subframe sequence (port 0). */
int oai4g_rx_batch_estimated(oai4g_rx_config_t *rx, oai4g_chest_config_t *ce, int n_sf, const int32_t *d_rxdataF,
                             int16_t *d_llr, int unscramble, void *stream);

/* ---------------- synchronisation, broadcast and HARQ-indicator channels ---------------- */
/* generate_pss (PHY/LTE_TRANSPORT/pss.c:50, decl LTE_TRANSPORT/proto.h): the Zadoff-Chu sequence
 * of root 25 / 29 / 34 (Nid_cell % 3, the Q15 table of PHY/LTE_REFSIG/primary_synch.h, here
 * generated as floor(32767 x)) scaled (a v) >> 15, a = amp or (amp 23170) >> 15 with two antennas,
 * on the 62 subcarriers around DC of symbol `symbol` of slot `slot_offset` of every frame grid
 * txdataF[ant] (overwrites).  Returns 0. */
int oai4g_generate_pss(int32_t **txdataF, int16_t amp, const oai4g_frame_parms_t *frame_parms, uint16_t symbol,
                       uint16_t slot_offset);
/* generate_sss (sss.c:47): d0_sss / d5_sss (PHY/LTE_TRANSPORT/sss.h, 36.211 6.11.2.1 m-sequences,
 * slot_offset < 3 selects d0) as (a d, 0) on the same 62 subcarriers.  Returns 0. */
int oai4g_generate_sss(int32_t **txdataF, int16_t amp, const oai4g_frame_parms_t *frame_parms, uint16_t symbol,
                       uint16_t slot_offset);
/* LTE_eNB_PBCH (LTE_TRANSPORT/defs.h): the scrambled coded bits, one byte per bit, computed when
 * frame_mod4 == 0 and mapped a quarter per frame */
typedef struct {
  uint8_t pbch_e[1920];
} oai4g_pbch_t;
/* generate_pbch (pbch.c:161): MIB (pbch_pdu[0..2]), CRC16 with the antenna mask, tail-biting
 * convolutional code, rate matching to 1920 (1728) bits and scrambling (frame_mod4 == 0), then
 * quarter frame_mod4 in QPSK (SISO / ALAMOUTI) on slot 1 symbols 0..3 of the subframe-0 grids
 * txdataF[ant] ('+='), around the RS positions.  Returns 0. */
int oai4g_generate_pbch(oai4g_pbch_t *eNB_pbch, int32_t **txdataF, int amp, const oai4g_frame_parms_t *frame_parms,
                        const uint8_t *pbch_pdu, uint8_t frame_mod4);
/* generate_phich (phich.c:401, normal cyclic prefix): HI -> BPSK x3, orthogonal sequence nseq,
 * scrambling, SISO / ALAMOUTI, onto the three REGs of group ngroup in symbol 0 of `subframe` of the
 * frame grids y[ant] ('+=').  The reference returns void; here 0, or -1 for what it does not
 * define (extended CP, extended PHICH duration, nushift >= 3 where phich.c:563-569 reads past its
 * 8-entry arrays, ngroup / nseq out of range). */
int oai4g_generate_phich(const oai4g_frame_parms_t *frame_parms, int16_t amp, uint8_t nseq_PHICH, uint8_t ngroup_PHICH,
                         uint8_t HI, uint8_t subframe, int32_t **y);
/* generate_phich_top's group / sequence of an uplink allocation (phich.c:1449-1465, FDD):
 * ngroup = (first_rb + n_DMRS) mod Ngroup, nseq = (first_rb / Ngroup + n_DMRS) mod 2 NSF. */
int oai4g_phich_group_seq(const oai4g_frame_parms_t *frame_parms, uint16_t first_rb, uint8_t n_DMRS, uint8_t *ngroup_PHICH,
                          uint8_t *nseq_PHICH);

/* ---------------- UE receive front end ---------------- */
/* dft64..dft2048 (PHY/TOOLS/lte_dfts.c:1766, 1957, 2172, 2359, 2574, 2689; decl TOOLS/defs.h):
 * y = DFT(x), bit-exact fixed point.  oai4g_dft returns 0 or -1. */
int oai4g_dft(int log2n, const int16_t *x, int16_t *y, int scale);
void oai4g_dft2048(const int16_t *x, int16_t *y, int scale);
void oai4g_dft1024(const int16_t *x, int16_t *y, int scale);
void oai4g_dft512(const int16_t *x, int16_t *y, int scale);
void oai4g_dft256(const int16_t *x, int16_t *y, int scale);
void oai4g_dft128(const int16_t *x, int16_t *y, int scale);
void oai4g_dft64(const int16_t *x, int16_t *y, int scale);
/* slot_fep's DFT window start (slot_fep.c:55-150) before the % frame_length; -1 for bad l / Ns */
int64_t oai4g_slot_fep_offset(const oai4g_frame_parms_t *frame_parms, uint8_t l, uint8_t Ns, int sample_offset,
                              int no_prefix);
/* slot_fep (PHY/MODULATION/slot_fep.c:40, decl MODULATION/defs.h): the reference passes
 * PHY_VARS_UE; here its rxdata / rxdataF / frame parameters / antenna count are explicit.
 * rxdata[aa]: 10 * samples_per_tti + ofdm_symbol_size words (wrap extension, written as the
 * reference does); rxdataF[aa]: symbols_per_tti * ofdm_symbol_size words.  Returns 0 or -1.
 * Channel estimation (perfect_ce == 0 branch, :179-222) is not included. */
int oai4g_slot_fep(int32_t *const *rxdata, int32_t *const *rxdataF, const oai4g_frame_parms_t *frame_parms,
                   uint8_t nb_antennas_rx, uint8_t l, uint8_t Ns, int sample_offset, int no_prefix);
/* Batched FEP, device pointers: d_rx [n_sf][n_ant][samples_per_tti] -> d_rxF
 * [n_sf][n_ant][symbols_per_tti][ofdm_symbol_size] (every symbol of both slots, sample_offset 0).
 * Asynchronous on `stream` (a hipStream_t, NULL = default). */
int oai4g_fep_batch(const oai4g_frame_parms_t *frame_parms, int n_sf, int n_ant, const int32_t *d_rx,
                    int32_t *d_rxF, void *stream);

/* ---------------- dlsim's channel stage (SIMULATION/LTE_PHY/dlsim.c:2714-2866) ---------------- */
/* signal_energy (PHY/TOOLS/signal_energy.c:66, decl TOOLS/defs.h): mean of (re^2 + im^2) >> 4 over
 * `length` complex int16 samples minus the squared DC, with the SSE code's integer wraps; >= 1. */
int32_t oai4g_signal_energy(const int32_t *input, uint32_t length);
/* Batched, device pointers: d_energy[i] = signal_energy(d_x + i * stride, length) — dlsim's tx_lev
 * of one transmit antenna (:2714-2719).  Asynchronous on `stream`. */
int oai4g_signal_energy_batch(const int32_t *d_x, int n, size_t stride, uint32_t length, int32_t *d_energy,
                              void *stream);
/* dlsim's AWGN (:2852-2866), device pointers, n <= 65535 vectors: vector i is the tx_len samples at
 * d_tx + i * tx_stride followed by the tail_len samples of the common d_tail (dlsim adds the noise
 * over two subframes, the second carrying only the next subframe's CRS); d_rx + i * rx_stride gets
 * (short)(s + sqrt(sigma2_i / 2) g) per I / Q component with sigma2_i in dB = 10 log10(d_tx_lev[i])
 * + offset_db (offset_db = 10 log10(N / (12 NB_RB)) - SNR - pa_dB) and g ~ N(0, 1) from a counter-
 * based stream keyed by (seed, first_vector + i, sample).  Asynchronous on `stream`. */
int oai4g_awgn_batch(const int32_t *d_tx, size_t tx_stride, uint32_t tx_len, const int32_t *d_tail, uint32_t tail_len,
                     int32_t *d_rx, size_t rx_stride, int n, const int32_t *d_tx_lev, double offset_db, uint64_t seed,
                     uint32_t first_vector, void *stream);

/* ---------------- fading channels (SIMULATION/TOOLS/random_channel.c, multipath_channel.c) ---------------- */
/* new_channel_desc_scm / fill_channel_desc (random_channel.c:195-860, :42-147) for n_vectors trials, each with its
 * own descriptor state on the device: a [n_vectors][nb_taps][nb_tx nb_rx], ch [n_vectors][nb_tx nb_rx]
 * [channel_length] as complex doubles (pair index aarx + aatx nb_rx) and a first_run flag.  `model` takes the
 * numeric values of SCM_t (SIMULATION/TOOLS/defs.h:158-178; dlsim's -g letters): EPA 5, EVA 6, ETU 7, Rayleigh8 9,
 * Rayleigh1 10, Rayleigh1_800 11, Rayleigh1_corr 12, Rayleigh1_anticorr 13, Rice8 14, Rice1 15, Rice1_corr 16,
 * Rice1_anticorr 17, AWGN 18.  BW is the caller's number (dlsim passes 1.25 / 5 / 10 / 20 for 6 / 25 / 50 / 100
 * PRB, not the sampling rate).  Refused with oai4g_last_error naming it: SCM_A .. SCM_D, custom, MBSFN, nb_tx or
 * nb_rx outside 1..2, and a channel_length beyond 255 (the reference's field is a uint8_t).  EPA / EVA / ETU at
 * 1x2 and 2x1 use identity correlation (the reference leaves that matrix's off-diagonals uninitialised). */
#define OAI4G_CHANNEL_MAX_TAPS 9
typedef struct {
  uint32_t nb_taps, channel_length, random_aoa;
  uint32_t n_matrices;                    /* correlation matrices held: tap i uses matrix i / 3 */
  double ricean_factor, aoa;
  double amps[OAI4G_CHANNEL_MAX_TAPS], delays[OAI4G_CHANNEL_MAX_TAPS];
} oai4g_channel_info_t;
typedef struct oai4g_channel_config oai4g_channel_config_t;
oai4g_channel_config_t *oai4g_channel_config_create(uint8_t nb_tx, uint8_t nb_rx, int model, double BW,
                                                    double forgetting_factor, int32_t channel_offset, double path_loss_dB,
                                                    int n_vectors);
void oai4g_channel_config_destroy(oai4g_channel_config_t *cfg);
/* the descriptor's tables; r_sqrt, when not null, receives [n_matrices][nb_tx nb_rx][nb_tx nb_rx][re, im] (at most
 * 6 x 4 x 4 x 2 doubles).  _model_describe is the constructor's host side alone and needs no device. */
int oai4g_channel_config_query(const oai4g_channel_config_t *cfg, oai4g_channel_info_t *info, double *r_sqrt);
int oai4g_channel_model_describe(int model, uint8_t nb_tx, uint8_t nb_rx, double BW, oai4g_channel_info_t *info,
                                 double *r_sqrt);
/* random_channel (:866-1015) of vectors [0, n): new state a (a copy on a vector's first run, else sqrt(ff) a +
 * sqrt(1 - ff) acorr) and interpolated taps ch.  The normals and uniforms are Philox-4x32 / Box-Muller keyed by
 * (seed, first_vector + vector, step, tap, pair), or, with d_draws not null, read from d_draws [n][per vector] in
 * the reference's draw order: tap, aarx, aatx: x, y, and on tap 0 of a model that draws its angle of arrival the
 * uniform behind them.  In the reference all trials share one descriptor, so a forgetting factor correlates trial t
 * with trial t - 1; in the batch the correlation runs along the successive calls of one vector.  Asynchronous on
 * `stream`; n > n_vectors is refused. */
int oai4g_channel_random_batch(oai4g_channel_config_t *cfg, int n, uint64_t seed, uint32_t first_vector, uint32_t step,
                               const double *d_draws, void *stream);
/* host <-> device state of vectors [first_vector, first_vector + n): ch [n][nb_tx nb_rx][channel_length][re, im] and
 * a [n][nb_taps][nb_tx nb_rx][re, im]; a null array is skipped.  Setting `a` ends the vectors' first run.  Both
 * synchronise. */
int oai4g_channel_set_taps(oai4g_channel_config_t *cfg, int first_vector, int n, const double *ch, const double *a);
int oai4g_channel_get_taps(oai4g_channel_config_t *cfg, int first_vector, int n, double *ch, double *a);
/* multipath_channel (multipath_channel.c:152-219, the non-SSE form) with keep_channel = 1 on the vectors' ch, and
 * dlsim's noise (dlsim.c:2852-2864), n <= n_vectors and <= 65535.  Input of vector v and transmit antenna j: the
 * tx_len int16 IQ samples at d_tx + v tx_stride + j tx_ant_stride followed by the tail_len samples at d_tail + j
 * tail_len; length = tx_len + tail_len.  Per output sample and receive antenna the reference's loop (j outer, l
 * inner, separate double multiplies and adds, zero input in front of sample 0), times 10^(path_loss_dB / 20),
 * delayed by |channel_offset| samples; samples [0, |channel_offset|), which the reference leaves unwritten, are 0
 * here.  Then (short)(r + sqrt(sigma2 / 2) g) per component with sigma2 in dB = 10 log10(sum_j d_tx_lev[v nb_tx +
 * j]) + offset_db; g is oai4g_awgn_batch's stream for receive antenna 0 (so model AWGN 1x1 equals oai4g_awgn_batch
 * bit for bit) and a stream of its own per further antenna.  Sample i of receive antenna a goes to d_rx + v
 * rx_stride + (i / seg_len) seg_stride + a rx_ant_stride + i % seg_len.  Strides in samples.  Asynchronous. */
int oai4g_multipath_batch(oai4g_channel_config_t *cfg, int n, const int32_t *d_tx, size_t tx_stride, size_t tx_ant_stride,
                          uint32_t tx_len, const int32_t *d_tail, uint32_t tail_len, int32_t *d_rx, size_t rx_stride,
                          size_t rx_ant_stride, uint32_t seg_len, size_t seg_stride, const int32_t *d_tx_lev,
                          double offset_db, uint64_t seed, uint32_t first_vector, void *stream);
/* The drop-ins, the reference's signatures with the configuration in place of channel_desc_t *, on vector 0.
 * random_channel draws from the Philox stream of the configuration's seed 0, one step per call.  multipath_channel
 * works on host doubles, draws a new channel first unless keep_channel, and leaves rx[.][0 .. |channel_offset|)
 * untouched as the reference does. */
int oai4g_random_channel(oai4g_channel_config_t *cfg);
int oai4g_multipath_channel(oai4g_channel_config_t *cfg, double **tx_sig_re, double **tx_sig_im, double **rx_sig_re,
                            double **rx_sig_im, uint32_t length, uint8_t keep_channel);

/* ---------------- uplink turbo decoding ---------------- */
enum { OAI4G_CRC24_A = 0, OAI4G_CRC24_B = 1 };
/* phy_threegpplte_turbo_decoder16 (PHY/CODING/3gpplte_turbo_decoder_sse_16bit.c:945, decl
 * CODING/defs.h): y = 3n+12 int16 LLRs (&d[96]), positive = bit 1.  Returns the iteration count,
 * max_iterations+1 when no CRC check passes, 255 on bad arguments (CRC16 / CRC8 unsupported). */
uint8_t oai4g_phy_threegpplte_turbo_decoder16(const int16_t *y, uint8_t *decoded_bytes, uint16_t n, uint16_t f1,
                                              uint16_t f2, uint8_t max_iterations, uint8_t crc_type, uint8_t F);
/* lte_rate_matching_turbo_rx (PHY/CODING/lte_rate_matching.c:688, decl CODING/defs.h) */
int oai4g_lte_rate_matching_turbo_rx(uint32_t RTC, uint32_t G, int16_t *w, const uint8_t *dummy_w,
                                     const int16_t *soft_input, uint8_t C, uint32_t Nsoft, uint8_t Mdlharq,
                                     uint8_t Kmimo, uint8_t rvidx, uint8_t clear, uint8_t Qm, uint8_t Nl, uint8_t r,
                                     uint32_t *E_out);
/* sub_block_deinterleaving_turbo (lte_rate_matching.c:193): d points at &d[96] (96 writable
 * entries before it), w holds 3*Kpi entries */
void oai4g_sub_block_deinterleaving_turbo(uint32_t D, int16_t *d, const int16_t *w);
/* Batched decoder, device pointers: n_cb blocks of size K, llr [n_cb][llr_stride] int16
 * (3K+12 each), out [n_cb][out_stride] bytes (K/8 each), iters [n_cb]; scratch of
 * oai4g_td_scratch_bytes(K, n_cb) bytes.  Asynchronous on `stream`.  As the reference's
 * decoded_bytes, a block's out row is written only by hard decisions (iteration >= 2): with
 * max_iterations = 1 it keeps the caller's previous contents. */
size_t oai4g_td_scratch_bytes(uint16_t K, int n_cb);
int oai4g_td_batch(int n_cb, uint16_t K, const int16_t *d_llr, size_t llr_stride, uint8_t *d_out, size_t out_stride,
                   uint8_t *d_iters, uint8_t max_iterations, uint8_t crc_type, uint8_t F, void *d_scratch,
                   void *stream);

/* phy_threegpplte_turbo_decoder8 (PHY/CODING/3gpplte_turbo_decoder_sse_8bit.c:894, decl CODING/defs.h):
 * the 8-bit decoder (16 windows of int8 lanes, inputs scaled by their |LLR| mean).  Restated for
 * n % 16 == 0 and n >= 512 (other sizes: the reference reads past its interleaver tables) and
 * CRC24_A / CRC24_B; returns 255 outside that scope.  f1 / f2 are implied by n. */
uint8_t oai4g_phy_threegpplte_turbo_decoder8(const int16_t *y, uint8_t *decoded_bytes, uint16_t n, uint16_t f1,
                                             uint16_t f2, uint8_t max_iterations, uint8_t crc_type, uint8_t F);
/* Batched 8-bit decoder, device pointers as oai4g_td_batch; llr rows of >= 3K + 16 int16 (the
 * last 4 are read by the input scaling only); scratch of oai4g_td8_scratch_bytes(K, n_cb). */
size_t oai4g_td8_scratch_bytes(uint16_t K, int n_cb);
int oai4g_td8_batch(int n_cb, uint16_t K, const int16_t *d_llr, size_t llr_stride, uint8_t *d_out, size_t out_stride,
                    uint8_t *d_iters, uint8_t max_iterations, uint8_t crc_type, uint8_t F, void *d_scratch,
                    void *stream);

/* generate_dummy_w (PHY/CODING/lte_rate_matching.c:293, decl CODING/defs.h): marks LTE_NULL in w at
 * the NULL / filler positions of the 3 Kpi circular buffer of a block of D = K + 4 bits with F
 * filler bits (other entries untouched, as the reference); returns R = ceil(D / 32). */
uint32_t oai4g_generate_dummy_w(uint32_t D, uint8_t *w, uint8_t F);

/* Batched UL receive chain of ulsch_decoding (PHY/LTE_TRANSPORT/ulsch_decoding.c:1208-1350) for
 * n_tb transport blocks of one configuration (B = TBS + 24 bits, G soft bits, Qm, rvidx, first
 * round: clear = 1, Nl = 1, Kmimo = 1; later rounds: oai4g_ul_decode_batch_harq below): per code block r, lte_rate_matching_turbo_rx of the
 * E_r soft bits at offset r_offset(r) of the TB's e stream, sub_block_deinterleaving_turbo and
 * phy_threegpplte_turbo_decoder16 (CRC24_B when C > 1, else CRC24_A with the filler F).  Device
 * pointers: d_e [n_tb][e_stride] int16, d_c [n_tb][C][c_stride] bytes (the reference's c[r],
 * K_r / 8 each), d_iters [n_tb][C] (iterations, or max_iterations + 1 on a CRC failure). */
typedef struct oai4g_ul_config oai4g_ul_config_t;
oai4g_ul_config_t *oai4g_ul_config_create(uint32_t B, uint32_t G, uint8_t Qm, uint8_t rvidx, uint8_t Mdlharq,
                                          uint32_t Nsoft, uint8_t max_iterations);
void oai4g_ul_config_destroy(oai4g_ul_config_t *cfg);
int oai4g_ul_config_C(const oai4g_ul_config_t *cfg);
/* Decoder of the chain: 16 (default, phy_threegpplte_turbo_decoder16) or 8 (the 8-bit decoder, as
 * dlsch_decoding with llr8_flag = 1, dlsim -L; one block size K % 16 == 0, K >= 512).  0 / -1. */
int oai4g_ul_config_set_decoder(oai4g_ul_config_t *cfg, int bits);
uint32_t oai4g_ul_config_E(const oai4g_ul_config_t *cfg, int r);
uint32_t oai4g_ul_config_G_offset(const oai4g_ul_config_t *cfg, int r);
int oai4g_ul_decode_batch(oai4g_ul_config_t *cfg, int n_tb, const int16_t *d_e, size_t e_stride, uint8_t *d_c,
                          size_t c_stride, uint8_t *d_iters, void *stream);
/* The same chain with HARQ soft combining across rounds, as dlsch_decoding / ulsch_decoding run it
 * (dlsch_decoding.c:348-383: lte_rate_matching_turbo_rx with clear = (round == 0), the round's
 * rvidx; dlsim's round loop, dlsim.c:2141): d_w [n_tb][C][w_stride] int16 device soft buffers, the
 * reference's harq->w[r], updated in place (w_stride >= oai4g_ul_config_w_entries(cfg)).  clear = 1
 * writes every entry below Ncb (NULL positions 0, as the reference's memset); entries at or past
 * Ncb are never read, so no initialisation of d_w is needed.  rvidx 0..3 overrides the
 * configuration's.  The configuration's soft-buffer split is Kmimo = 1 (the uplink; dlsch_decoding
 * with one codeword per TB, TM1 / TM2): a DL TM3 transport block (Kmimo = 2) has another Ncb and k0
 * and is outside this API. */
size_t oai4g_ul_config_w_entries(const oai4g_ul_config_t *cfg);
int oai4g_ul_decode_batch_harq(oai4g_ul_config_t *cfg, int n_tb, const int16_t *d_e, size_t e_stride, int16_t *d_w,
                               size_t w_stride, uint8_t rvidx, uint8_t clear, uint8_t *d_c, size_t c_stride,
                               uint8_t *d_iters, void *stream);
/* The same round with a redundancy version and a clear flag per transport block, so that one batch
 * holds HARQ processes at different rounds: d_rv, d_clear are device arrays [n_tb] (rv is used
 * masked to 0..3, clear as zero / non-zero).  Transport block i is bit-exact with
 * oai4g_ul_decode_batch_harq(rvidx = d_rv[i], clear = d_clear[i]). */
int oai4g_ul_decode_batch_harq_tb(oai4g_ul_config_t *cfg, int n_tb, const int16_t *d_e, size_t e_stride, int16_t *d_w,
                                  size_t w_stride, const uint8_t *d_rv, const uint8_t *d_clear, uint8_t *d_c,
                                  size_t c_stride, uint8_t *d_iters, void *stream);

/* ---------------- batched device-resident transmit path ---------------- */
/* Plain-old-data parameter block: what rank 0 broadcasts (RCCL) to the other ranks. */
typedef struct {
  uint16_t N_RB_DL;
  uint16_t Nid_cell;
  uint8_t Ncp;
  uint8_t nb_antennas_tx;
  uint8_t mode1_flag;
  uint8_t frame_type;
  uint8_t n_cw;               /* 1 (TM1) or 2 (TM3) */
  uint8_t mimo_mode;          /* OAI4G_SISO, _ALAMOUTI, _LARGE_CDD, or a single-layer precoding mode
                                 OAI4G_UNIFORM_PRECODING11 .. OAI4G_PUSCH_PRECODING1 (one codeword, two
                                 antennas, mode1_flag 0) */
  uint8_t num_pdcch_symbols;
  uint8_t Kmimo;
  uint8_t Mdlharq;
  uint8_t first_subframe;     /* subframe index of batch element 0 */
  uint8_t subframe_step;      /* 0: every element uses first_subframe; 1: consecutive subframes */
  uint8_t with_crs;           /* 1: cell-specific reference signals in the grid (pilots.c:43) */
  uint16_t rnti;
  int16_t amp;
  int16_t sqrt_rho_a;
  int16_t sqrt_rho_b;
  uint32_t rb_alloc[4];
  uint16_t nb_rb;
  uint8_t mcs[2];
  uint8_t rvidx[2];
  uint8_t q[2];               /* scrambling codeword index q (dlsim passes 0) */
  uint32_t TBS[2];
  uint32_t payload_stride;    /* bytes between consecutive transport blocks in the payload buffer */
  uint32_t rm_limited_buffer; /* opt-in extension: 36.212 5.1.4.1.2 limited-buffer
                                 rate matching when Ncb < Kw, where the reference prints "RM condition"
                                 and emits E = 0 (lte_rate_matching.c:518-521); unlocks TM3 MCS >= 20.
                                 0 (default) keeps the reference's behaviour (config_create fails). */
  uint32_t pmi_alloc;         /* modes 3..8: the harq process's pmi_alloc for every subframe of the batch
                                 (oai4g_get_pmi); only the low 16 bits may be set */
  uint32_t reserved[6];
} oai4g_tx_params_t;

typedef struct oai4g_tx_config oai4g_tx_config_t;

/* Derive every per-configuration table (segmentation, rate-matching geometry, RE maps,
 * QAM/twiddle/Gold tables) and upload it to the current device.  NULL on error. */
oai4g_tx_config_t *oai4g_tx_config_create(const oai4g_tx_params_t *p);
void oai4g_tx_config_destroy(oai4g_tx_config_t *cfg);
/* Derived sizes */
uint32_t oai4g_tx_G(const oai4g_tx_config_t *cfg, int cw, int subframe);
uint32_t oai4g_tx_ebits_words(const oai4g_tx_config_t *cfg);        /* per codeword per subframe */
uint32_t oai4g_tx_iq_samples(const oai4g_tx_config_t *cfg);         /* per antenna per subframe */
size_t oai4g_tx_workspace_bytes(const oai4g_tx_config_t *cfg, int n_sf);

/* Run n_sf subframes.  All pointers are device pointers:
 *   d_payload : [n_sf][n_cw][payload_stride] bytes, TBS/8 valid bytes each (not modified)
 *   d_work    : oai4g_tx_workspace_bytes() bytes (packed scrambled e bits)
 *   d_iq      : [n_sf][nb_antennas_tx][samples_per_tti] int32 (int16 I, int16 Q)
 *               (8-byte aligned: sample pairs leave as 8-byte stores; -1 otherwise)
 * stream is a hipStream_t (NULL = default stream).  Asynchronous. */
int oai4g_tx_batch(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, void *d_work,
                   int32_t *d_iq, void *stream);
/* Same, but records HIP events around each kernel on `stream`, synchronizes, and returns the
 * two kernel durations in ms (kernel_ms[0] = encode/RM/scramble, [1] = modulate/IDFT/CP). */
int oai4g_tx_batch_timed(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, void *d_work,
                         int32_t *d_iq, void *stream, float *kernel_ms);
/* Control region in the batched grid: every batch element of subframe index
 * sf also carries generate_dci_top's PCFICH + PDCCH for this DCI set (the same DCIs in every
 * subframe, as dlsim transmits them), merged by the modulator; n_dci = 0 switches it off.
 * The control values are computed on the GPU once here, per subframe index.  Returns 0 / -1. */
int oai4g_tx_config_set_control(oai4g_tx_config_t *cfg, uint8_t num_ue_spec_dci, uint8_t num_common_dci,
                                const oai4g_dci_alloc_t *dci_alloc);
/* Common signals in the batched grid (the eNB's common signal procedures,
 * phy_procedures_lte_eNb.c:1529-1760, and generate_phich_top :2585): PSS + SSS in subframe
 * indices 0 and 5, the PBCH quarter frame_mod4 of pbch_pdu in subframe index 0, and the listed
 * PHICHs; merged with the PCFICH / PDCCH of oai4g_tx_config_set_control, so with with_crs = 1 the
 * GPU grid is the eNB's complete txdataF.  NULL switches them off.  Returns 0 / -1. */
#define OAI4G_MAX_PHICH_ITEMS 64
typedef struct {
  uint8_t subframe, ngroup, nseq, hi;
} oai4g_phich_item_t;
typedef struct {
  uint8_t pss_sss;
  uint8_t pbch;
  uint8_t pbch_pdu[3];
  uint8_t frame_mod4;
  uint8_t n_phich;
  oai4g_phich_item_t phich[OAI4G_MAX_PHICH_ITEMS];
} oai4g_common_sig_t;
int oai4g_tx_config_set_common(oai4g_tx_config_t *cfg, const oai4g_common_sig_t *common);
/* Stage entry for parity tests: run only the encoder kernel (payload -> packed e bits). */
int oai4g_tx_encode(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, void *d_work, void *stream);
/* HARQ retransmissions in a batch: a redundancy version per transport block.  oai4g_tx_params_t's
 * rvidx[2] holds for every subframe of oai4g_tx_batch; oai4g_tx_config_enable_tb_rv derives, once,
 * what of the rate-matching plan depends on rv (the circular buffer's start k0, hence where every run
 * of the buffer lands in e and which run straddles its end) for each of rv 0..3 and uploads it beside
 * the configuration; everything else (segmentation, E, G, scrambling) is shared.  oai4g_tx_batch_rv
 * is then oai4g_tx_batch with d_rv, a device array [n_sf][n_cw] of values 0..3 (used masked with 3):
 * transport block (sf, cw) is bit-exact with a configuration created with rvidx[cw] = d_rv[sf][cw].
 * Every rv is rate-matched from the transport block's own intact circular buffer w (36.212
 * 5.1.4.1.2), re-encoded from the payload in the same kernel: what a combining receiver expects.
 * (The drop-in oai4g_dlsch_encoding keeps the reference's stored, overlapped w instead.)
 * enable: 0 / -1 (idempotent); batch_rv / encode_rv: -1 when enable was not called.
 * oai4g_tx_encode_rv is the stage entry (payload -> packed e bits), as oai4g_tx_encode. */
int oai4g_tx_config_enable_tb_rv(oai4g_tx_config_t *cfg);
int oai4g_tx_batch_rv(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, const uint8_t *d_rv,
                      void *d_work, int32_t *d_iq, void *stream);
int oai4g_tx_encode_rv(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, const uint8_t *d_rv,
                       void *d_work, void *stream);
/* Stage entry: run only the modulator kernel (packed scrambled e bits in d_work, as oai4g_tx_encode
 * leaves them -> QAM / RE map / precoding / IDFT / CP -> d_iq). */
int oai4g_tx_modulate(const oai4g_tx_config_t *cfg, int n_sf, const void *d_work, int32_t *d_iq, void *stream);
/* 1 when the configuration's range check admits the modulator's no-saturation IDFT forms, 0
 * otherwise.  It can pass for every 2048-point normal-prefix transmit mode (TM1, ALAMOUTI, two- and
 * four-antenna LARGE_CDD): it does when the largest level among the QAM / QPSK tables, the CRS and
 * the static REs of oai4g_tx_config_set_control / _set_common keeps every value of the leaf, 64-,
 * 256-, 1024- and 2048-levels inside int16 with a margin; those calls re-check it. */
int oai4g_tx_mod_nosat(const oai4g_tx_config_t *cfg);
/* The configuration's lz of oai4g_mod_item_map: its leading symbols without data REs, CRS or static REs at
 * every subframe index (0 with CRS or a control region; set_control / set_common re-derive it). */
int oai4g_tx_mod_lz(const oai4g_tx_config_t *cfg);

/* Diagnostics: average ms of the encoder kernel stopped after phase `stop_phase`
 * (0 load+Gold, 1 CRC, 2 segmentation, 3 turbo, 4 w build, 99 = complete).  Outputs invalid. */
int oai4g_diag_encode_phase_ms(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, void *d_work,
                               int stop_phase, int reps, float *ms);
/* Diagnostics: resident k_encode workgroups per CU and the dynamic LDS bytes per workgroup. */
int oai4g_diag_encode_occupancy(const oai4g_tx_config_t *cfg, int *blocks_per_cu, size_t *lds_bytes);
/* PMC calibration: stream `bytes` through HBM at 4 B per lane (mode 0 read, 1 write) */
int oai4g_diag_stream(const void *d_src, void *d_dst, size_t bytes, int mode, void *stream);

/* ---------------- multi-GPU: one process per GPU, RCCL over xGMI ---------------- */
/* The device this process drives (its local rank); call before any other oai4g_ call.  0 / -1. */
int oai4g_set_device(int device);
#define OAI4G_DIST_ID_BYTES 128
/* rank 0: a fresh RCCL unique id (ncclGetUniqueId) for every rank, passed out of band.  0 / -1. */
int oai4g_dist_unique_id(uint8_t id[OAI4G_DIST_ID_BYTES]);
/* join the RCCL communicator as `rank` of `world` (ncclCommInitRank, on the oai4g_set_device
 * device).  0 / -1. */
int oai4g_dist_init(int rank, int world, const uint8_t id[OAI4G_DIST_ID_BYTES]);
/* the parameter block of rank `root` into *p on every rank (ncclBroadcast of its bytes): the one
 * collective the transmit path needs.  0 / -1. */
int oai4g_dist_broadcast_params(oai4g_tx_params_t *p, int root);
/* in-place sum of n counters / checksums, max of n doubles (timings) over the ranks.  0 / -1. */
int oai4g_dist_allreduce_sum_u64(uint64_t *v, int n);
int oai4g_dist_allreduce_max_f64(double *v, int n);
int oai4g_dist_barrier(void);
int oai4g_dist_rank(void);             /* -1 before oai4g_dist_init */
int oai4g_dist_world(void);            /* 0 before oai4g_dist_init */
int oai4g_dist_finalize(void);
/* the contiguous shard [*first, *first + *count) of n_total units owned by rank of world (sizes
 * differ by at most one) */
void oai4g_shard_range(int n_total, int rank, int world, int *first, int *count);
/* the oai4g_fill_payload seed that makes a rank's buffer of global subframes [first_subframe, ...)
 * equal to that slice of the global payload stream of `seed` (payloads derive from (seed, global
 * subframe index), whatever the world size) */
uint64_t oai4g_payload_seed(uint64_t seed, uint64_t first_subframe, uint32_t n_cw, uint32_t payload_stride);

/* ---------------- device memory helpers (for hosts without another allocator) ---------------- */
void *oai4g_dev_alloc(size_t bytes);
void oai4g_dev_free(void *p);
int oai4g_memcpy_h2d(void *dst, const void *src, size_t bytes);
int oai4g_memcpy_d2h(void *dst, const void *src, size_t bytes);
int oai4g_memset_d(void *dst, int value, size_t bytes);
int oai4g_sync(void);
/* Deterministic device-side payload generator: 8-byte word w = splitmix64 output for the counter
 * seed + 0x9e3779b97f4a7c15 (w + 1) (little-endian bytes). */
int oai4g_fill_payload(uint8_t *d_payload, size_t bytes, uint64_t seed, void *stream);
/* HARQ round state of a batch of n_slots HARQ processes, advanced on the device after a decode
 * (dlsim's round loop, dlsim.c:2141: up to num_rounds <= 4 transmissions of a transport block, rvidx =
 * round & 3), so that a loop of oai4g_tx_batch_rv -> channel -> receiver ->
 * oai4g_ul_decode_batch_harq_tb -> oai4g_harq_advance needs no host synchronisation.  All arrays are
 * device arrays.  Per slot i, from d_iters [n_slots][C] (a block failed when iters > max_iterations):
 *   - d_counters [8] = dlsim's round_trials[4] then errs[4] (dlsim.c:2143, 3438), accumulated:
 *     round_trials[d_round[i]]++, and errs[d_round[i]]++ when the slot failed (zero them to start);
 *   - failed with a round left (d_round[i] + 1 < num_rounds): d_round[i]++, the payload row is kept,
 *     d_done[i] = 0;
 *   - else the transport block is finished: d_done[i] = 1 (decoded) or 2 (not decoded), d_round[i] =
 *     0, d_trial[i]++ (the slot's running transport-block index; start from 0) and the slot's payload
 *     row, row_bytes at d_payload + i row_bytes (n_cw payload_stride of a tx batch; a multiple of 8,
 *     8-byte aligned), is refilled with row d_trial[i] n_slots + i of the oai4g_fill_payload stream of
 *     `seed`: the bytes oai4g_fill_payload(seed) writes at byte offset (d_trial[i] n_slots + i)
 *     row_bytes of a long enough buffer.  Trial 0 is oai4g_fill_payload over the whole buffer;
 *   - d_rv[i][cw] = d_round[i] & 3 for cw < n_cw and d_clear[i] = (d_round[i] == 0), for the next
 *     oai4g_tx_batch_rv / oai4g_ul_decode_batch_harq_tb.
 * Start with d_round, d_rv zeroed and d_clear set to 1.  0 / -1. */
int oai4g_harq_advance(int n_slots, int C, uint8_t max_iterations, int num_rounds, int n_cw, const uint8_t *d_iters,
                       uint8_t *d_round, uint32_t *d_trial, uint8_t *d_rv, uint8_t *d_clear, uint8_t *d_done,
                       uint32_t *d_counters, uint8_t *d_payload, size_t row_bytes, uint64_t seed, void *stream);

/* ---------------- SC-FDMA: the PUSCH DFT sizes, ulsch_modulation and lte_idft ---------------- */
/* The 33 mixed-radix "PUSCH DFTs" of PHY/TOOLS/lte_dfts.c (:3510-16087), bit-exact: 12, 24, 36, 48, 60, 72, 96, 108,
 * 120, 144, 180, 192, 216, 240, 288, 300, 324, 360, 384, 432, 480, 540, 576, 600, 648, 720, 864, 900, 960, 972, 1080,
 * 1152, 1200.  Every other size is refused, 768 (64 PRB) included: the reference has no dft768 (its lte_idft logs
 * "Unsupported" and returns with the input conjugated; its dft_lte copies out an unwritten buffer).
 *
 * The plan of one size as the engine runs it, outermost level first: dft<size> splits off radix[0] and runs radix[0]
 * sub-transforms of sub_size[0], and so on down to the twelve-point leaf.  norm[l] is the constant of the
 * mulhi_int16 that follows level l when the size is called with scale_flag 1 (0: that level is not scaled; dft96,
 * dft108 and dft120 call their sub-transforms with scale_flag 0); leaf_norm is 9459 for size 12 (applied by dft_lte
 * and lte_idft behind dft12) and 0 otherwise.  Level l's twiddles are entries tw_offset[l] .. of the table: for q = 1
 * .. radix - 1 and k = 1 .. sub_size - 1, entry (q - 1)(sub_size - 1) + k - 1 = 32767 (cos, -sin)(2 pi q k / (radix
 * sub_size)), truncated toward zero where radix sub_size <= 300 and floor() above, as the reference's tables are. */
#define OAI4G_PUSCH_MAX_LEVELS 4
typedef struct {
  uint16_t size, n_levels;
  uint8_t radix[OAI4G_PUSCH_MAX_LEVELS];
  uint16_t sub_size[OAI4G_PUSCH_MAX_LEVELS];
  int16_t norm[OAI4G_PUSCH_MAX_LEVELS];
  int16_t leaf_norm;
  uint16_t pad;
  uint32_t tw_offset[OAI4G_PUSCH_MAX_LEVELS];
  uint32_t n_twiddles;
} oai4g_pusch_plan_t;
/* Host only, no device: the plan of Msc, and its twiddles into `twiddles` ([capacity][2] int16, null to skip).
 * -1 (oai4g_last_error says why) for 768, every other size not listed, or capacity < n_twiddles. */
int oai4g_pusch_dft_plan(int32_t Msc, oai4g_pusch_plan_t *plan, int16_t *twiddles, uint32_t capacity);

/* One PUSCH allocation of one UE over a run of subframes: first_rb / nb_rb (Msc = 12 nb_rb), Qm 2 / 4 / 6, srs_active
 * 0 / 1 (the last symbol is left out of the mapping), the scrambling identity (rnti, frame_parms->Nid_cell) and the
 * subframe number of batch element i, (first_subframe + i subframe_step) % 10.  The plan and twiddles of Msc and the
 * Gold words of the ten subframe numbers are built here and uploaded once.  Refused (null, oai4g_last_error set):
 * what ulsch_modulation refuses (nb_rb 0, first_rb > 25), a size with no dft<Msc>, an allocation that leaves the
 * band (first_rb + nb_rb > N_RB_DL), and first_carrier_offset + 12 first_rb == ofdm_symbol_size (N_RB_DL 6 with
 * first_rb 3, N_RB_DL 50 with first_rb 25), where the reference's wrap test ('>') lets it write REs N .. N + Msc - 1
 * of every symbol, past the symbol and in the last one past the subframe. */
typedef struct oai4g_pusch_config oai4g_pusch_config_t;
oai4g_pusch_config_t *oai4g_pusch_config_create(const oai4g_frame_parms_t *frame_parms, uint16_t first_rb, uint16_t nb_rb,
                                                uint8_t Qm, uint8_t srs_active, uint16_t rnti, uint8_t first_subframe,
                                                uint8_t subframe_step);
void oai4g_pusch_config_destroy(oai4g_pusch_config_t *cfg);
/* ulsch_modulation (PHY/LTE_TRANSPORT/ulsch_modulation.c:376-783, cooperation_flag != 2) of n_sf subframes in one
 * launch: d_h [n_sf] rows of h_stride >= G bytes (ulsch->h: 0 / 1, PUSCH_x = 2, PUSCH_y = 3; G = 12 nb_rb Qm
 * Nsymb_pusch), d_txdataF [n_sf][symbols_per_tti][ofdm_symbol_size] (one subframe of txdataF[0] per element).  Only
 * the REs the reference writes are written: subcarriers (first_carrier_offset + 12 first_rb + i) mod
 * ofdm_symbol_size, i < Msc, of the symbols other than 3 / 10 (normal prefix) or 2 / 8 (extended), the last symbol
 * left out when srs_active.  Asynchronous on `stream`.  Returns 0 or -1. */
int oai4g_pusch_mod_batch(oai4g_pusch_config_t *cfg, int n_sf, const uint8_t *d_h, size_t h_stride, int16_t amp,
                          int32_t *d_txdataF, void *stream);
/* dft_lte's contract (ulsch_modulation.c:53-373) on d_d / d_z [n_sf][Nsymb_pusch][Msc] (they may be the same array):
 * each column through dft<Msc> with scale_flag 1 (12: dft12, then 9459).  Asynchronous on `stream`.  0 or -1. */
int oai4g_pusch_dft_batch(oai4g_pusch_config_t *cfg, int n_sf, const int32_t *d_d, int32_t *d_z, void *stream);
/* lte_idft (PHY/LTE_TRANSPORT/ulsch_demodulation.c:58-465) in place on d_comp [n_sf][symbols_per_tti][12 N_RB_DL]
 * (rxdataF_comp[0]): subcarriers < Msc of symbols 0, 1, 2, 4 .. 9, 11, 12, 13 (normal prefix) or 0, 1, 3 .. 7, 9, 10,
 * 11 (extended), whatever srs_active is: conjugate (an imaginary part of -32768 stays), forward transform,
 * conjugate.  The pilot symbols and the subcarriers >= Msc are not touched.  Asynchronous on `stream`.  0 or -1. */
int oai4g_pusch_idft_batch(oai4g_pusch_config_t *cfg, int n_sf, int32_t *d_comp, void *stream);
/* Drop-ins on host buffers behind the reference's call shapes.
 * oai4g_dft_lte: the reference always transforms 12 columns of d (stride Msc), whatever Nsymb is; the columns past
 * Nsymb hold stale data there and their outputs are never mapped.  This one transforms Nsymb (<= 12) columns and
 * leaves z beyond them untouched.
 * oai4g_pusch_dft: one transform in the reference's dft<Msc>(x, y, scale_flag) contract, on plain samples (one
 * transform, not the reference's four interleaved ones); dft12 has no flag and never scales.
 * oai4g_lte_idft: z is one subframe of rxdataF_comp[0], symbols_per_tti rows of 12 N_RB_DL words. */
int oai4g_dft_lte(int32_t *z, const int32_t *d, int32_t Msc_PUSCH, uint8_t Nsymb);
int oai4g_pusch_dft(int32_t Msc, const int16_t *x, int16_t *y, uint8_t scale_flag);
int oai4g_lte_idft(const oai4g_frame_parms_t *frame_parms, int32_t *z, uint16_t Msc_PUSCH);
/* The fields of LTE_UE_ULSCH_t (PHY/LTE_TRANSPORT/defs.h:258-348) and LTE_UL_UE_HARQ_t that ulsch_modulation reads;
 * harq_pid stands for subframe2harq_pid(frame_parms, frame, subframe), which the caller evaluates. */
typedef struct {
  uint16_t first_rb, nb_rb;
  uint8_t mcs;
  uint8_t pad[3];
} oai4g_ul_harq_t;
typedef struct {
  const oai4g_ul_harq_t *harq_processes[8];
  const uint8_t *h;
  uint16_t rnti;
  uint8_t harq_pid, Nsymb_pusch, srs_active, cooperation_flag;
  uint8_t pad[2];
} oai4g_ue_ulsch_t;
/* ulsch_modulation: writes the allocation into txdataF[0] at symbol_offset = ofdm_symbol_size (l + subframe
 * symbols_per_tti), a frame of ten subframes.  0: done.  1: the reference's own refusal (harq_pid > 7, nb_rb 0,
 * first_rb > 25), nothing written, as there.  -1: refused here, nothing written: cooperation_flag 2 (distributed
 * Alamouti), Nsymb_pusch other than the symbols the mapping takes, and what oai4g_pusch_config_create refuses.
 * oai4g_last_error says which in both cases. */
int oai4g_ulsch_modulation(int32_t *const *txdataF, int16_t amp, uint32_t frame, uint32_t subframe,
                           const oai4g_frame_parms_t *frame_parms, const oai4g_ue_ulsch_t *ulsch);

#ifdef __cplusplus
}
#endif
#endif
