/*
 * Internal definitions shared by the host layer (oai4g_host.cpp) and the gfx950 kernels.
 *
 * Device-resident configuration ("cfg_dev_t") holds everything that depends only on the
 * cell / DLSCH parameters and the subframe index: code-block geometry, rate-matching
 * geometry, per-symbol RE maps, QAM tables, Gold jump tables and IDFT twiddles.  It is built
 * once per configuration on the host (the same derivations the reference re-does on every
 * call) and read by every workgroup through scalar loads.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oai4g.h"

#define OAI4G_MAX_CB 16
#define OAI4G_MAX_NULLS 104
#define OAI4G_MAX_CHUNKS 192                /* 6144 / 32 */
#define OAI4G_MAX_TASKS (OAI4G_MAX_CB * 20)  /* ceil(R/32) + ceil(R/16) tiles per block, R <= 193 */
#define OAI4G_RM_TILES 20                     /* ceil(R/32) + ceil(R/16) for R <= 193 */
#define OAI4G_RM_SRC_LAST (1u << 20)
#define OAI4G_RM_DST_WRAP (1u << 27)
#define OAI4G_PIPE_MAX_CHUNKS 16
#define OAI4G_CRS_CODE 0xE000u               /* remap codes >= this (and != 0xFFFF) are CRS REs:
                                                CRS_CODE | pilot entry i << 9 | port & 1 << 8 | m */
#define OAI4G_CTL_CODE 0xC000u               /* remap code of a control-region RE (generate_dci_top) */
/* k_modofdm's staged layout, one definition for the kernel and for upload_remap, which writes the RE
 * codes the kernel reads.  Per symbol the kernel stages one LDS entry per data RE, entry idx at byte
 * idx << shift, below a zero sentinel entry at index 3N/4 that every non-data RE addresses; the
 * thread-major RE code of data RE idx is that byte offset.  Entries are 2-byte QAM-table addresses
 * (shift 1; bit 15 of the code carries the CDD parity), except in the 2048-point kernels that stage
 * looked-up values: 4-byte QAM words for TM1 (shift 2) and 8-byte precoded (y0, d) pairs, sign
 * included, for two-antenna LARGE_CDD (shift 3; 8 * 3N/4 < 2^15). */
static constexpr uint32_t oai4g_mod_entry_shift(uint32_t mimo_mode, uint32_t n_ant, uint32_t log2N)
{
  return log2N != 11 ? 1u : mimo_mode == OAI4G_LARGE_CDD && n_ant == 2 ? 3u : mimo_mode == OAI4G_SISO ? 2u : 1u;
}
/* the bits of an RE code that address its entry */
static constexpr uint32_t oai4g_mod_addr_mask(uint32_t shift) { return 0x7FFFu & ~((1u << shift) - 1u); }
static constexpr uint32_t oai4g_mod_sentinel(uint32_t N) { return (3u * N) / 4u; }
/* Single-layer precoding (modes 3..8, dlsch_modulation.c:750-866): a data RE's code carries its RB's
 * precoder index (oai4g_get_pmi) in bits 12-13 and no parity, in the natural map (data index below:
 * at most 1200 per symbol) and in the thread-major one (2-byte entries: the sentinel's offset
 * 2 * 3N/4 = 3072 at 2048 points stays below bit 12).  Every other RE's code has precoder 0. */
static constexpr bool oai4g_mode_prec1(uint32_t mimo_mode)
{
  return mimo_mode >= OAI4G_UNIFORM_PRECODING11 && mimo_mode <= OAI4G_PUSCH_PRECODING1;
}
#define OAI4G_MOD_PMI_SHIFT 12u
static constexpr uint32_t oai4g_mod_pmi_bits = 3u << OAI4G_MOD_PMI_SHIFT;
static constexpr uint32_t oai4g_mod_pmi_idx_mask = (1u << OAI4G_MOD_PMI_SHIFT) - 1u;
static_assert(2u * (oai4g_mod_sentinel(2048) + 4u) <= (1u << OAI4G_MOD_PMI_SHIFT), "staged offsets must stay below the precoder bits");
/* a symbol's data REs are staged in quads: the last quad must end below the sentinel */
static constexpr bool oai4g_mod_nre_fits(uint32_t nre, uint32_t N) { return nre + 3u <= oai4g_mod_sentinel(N); }
/* k_modofdm's item space is dense over the symbols that can carry anything: the lz leading symbols that
 * are empty at every subframe index (the control region of a grid without CRS or control signals) are
 * no items.  Item -> (subframe, symbol, antenna pair): ips items per symbol (2 in the 4-port kernel),
 * per = nsymb - lz symbols per subframe, permag = ceil(2^32 / per) (oai4g_mod_permag): the quotient is
 * exact while n_sf per^2 <= 2^32 (launch-checked).  The item with l == lz also zero-fills symbols
 * 0 .. lz - 1 of its subframe (its antenna pair's planes with ips = 2, else every antenna's). */
struct oai4g_mod_item_t {
  uint32_t sf, l, pair;
};
static constexpr uint32_t oai4g_mod_permag(uint32_t per) { return (uint32_t)(((1ull << 32) + per - 1) / per); }
static inline __host__ __device__ oai4g_mod_item_t oai4g_mod_item(uint32_t item, uint32_t ips, uint32_t lz, uint32_t per,
                                                                  uint32_t permag)
{
  const uint32_t it = item / ips;
  const uint32_t sf = (uint32_t)(((uint64_t)it * permag) >> 32);
  return {sf, lz + it - sf * per, item - it * ips};
}
/* leading symbols that may be skipped at most: the fill region [0, body of symbol lz - CP) of an antenna
 * plane stays inside slot 0 for either prefix type */
#define OAI4G_MOD_LZ_MAX 4u
#define OAI4G_ENC_CRC_TABLE_WORDS (256 + 256) /* byte tables A/B (the combine multipliers stay in global memory;
                                                  slice-by-4 tables, 2048 words, cost one workgroup per CU: slower) */
#define OAI4G_GOLD_LANES 256
#define OAI4G_GOLD_STRIDE 17   /* odd: lanes 17l + k hit distinct LDS banks */
#define OAI4G_MAX_GOLD_WORDS (OAI4G_GOLD_LANES * OAI4G_GOLD_STRIDE) /* >= (14*1200*6)/32 */
#define OAI4G_TW_TOTAL (16 + 64 + 128 + 256 + 512 + 1024 + 2048)

/* 4 bytes from any byte address of global memory (unaligned dword load) */
typedef uint32_t __attribute__((aligned(1))) u32_a1_t;
static __device__ __forceinline__ uint32_t ld_u32_any(const uint8_t *p)
{
  return *(const __attribute__((address_space(1))) u32_a1_t *)p;
}

/* the device payload generator (k_fill; the refills of k_harq_advance): 8-byte word w of the stream of
 * `seed` is splitmix64's output for the counter seed + gamma (w + 1) */
static inline __host__ __device__ uint64_t oai4g_payload_word(uint64_t seed, uint64_t w)
{
  uint64_t z = seed + 0x9e3779b97f4a7c15ull * (w + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

/* twiddle table offsets (packed int16 pairs), indexed by log2 of the level size */
static inline __host__ __device__ uint32_t oai4g_tw_offset(int log2s)
{
  /* 16:0, 64:16, 128:80, 256:208, 512:464, 1024:976, 2048:2000 */
  switch (log2s) {
  case 4: return 0;
  case 6: return 16;
  case 7: return 80;
  case 8: return 208;
  case 9: return 464;
  case 10: return 976;
  case 11: return 2000;
  default: return 0;
  }
}

struct cw_dev_t {
  uint32_t TBS;            /* bits */
  uint32_t A_bytes;        /* TBS/8 */
  uint32_t C, Cminus, Kplus, Kminus, F, L;
  uint32_t Qm;
  uint32_t q;              /* scrambling codeword index */
  /* per code block (segmentation, lte_segmentation.c:39-170) */
  uint32_t K[OAI4G_MAX_CB];
  uint32_t f1[OAI4G_MAX_CB], f2[OAI4G_MAX_CB];
  uint32_t src[OAI4G_MAX_CB];   /* byte offset in b (= TB||CRC24A) of the first copied byte */
  uint32_t fill[OAI4G_MAX_CB];  /* zero filler bytes at the start of the block */
  uint32_t ncopy[OAI4G_MAX_CB]; /* bytes copied from b */
  uint32_t crc_off[OAI4G_MAX_CB]; /* word offset of the block's streams in LDS */
  /* per code block rate-matching geometry (lte_rate_matching.c:51-130, 464-566) */
  uint32_t R[OAI4G_MAX_CB], Kpi[OAI4G_MAX_CB], ND[OAI4G_MAX_CB], Ncb[OAI4G_MAX_CB];
  uint32_t Nnn[OAI4G_MAX_CB];   /* non-NULL entries of w[0..Ncb) */
  uint32_t k0c[OAI4G_MAX_CB];   /* non-NULL entries of w[0..k0): compacted start */
  uint32_t kidx[OAI4G_MAX_CB];  /* which null list (0: Kminus, 1: Kplus) */
  uint32_t wpk_off[OAI4G_MAX_CB + 1]; /* LDS word offset of block r's packed w (3R words + 2 pad) */
  uint32_t ntask;                     /* sub-block interleaver tiles of all blocks */
  uint16_t tasks[OAI4G_MAX_TASKS];    /* block | kind << 4 (0: v0 rows, 1: v1/v2 rows) | tile << 5 */
  uint32_t ilv_off[OAI4G_MAX_CB + 1]; /* LDS word offset of block r's QPP-interleaved input words */
  /* QPP interleaver walk per 8-step unit j of the quarter fold (kidx list): Pi(8j) | (Pi(8j+1) -
   * Pi(8j) mod K) << 16, j < K/32 (3gpplte.c:50-74 restated incrementally) */
  uint32_t qpp0[2][OAI4G_MAX_CHUNKS];
  /* the quarter fold's walk as a table: entry k < K/4 (two uint16 per word) = word index of
   * x' = Pi(k) mod K/4 in the byte-interleaved planes (x' >> 3) | shift (8 (Pi(k) div K/4) +
   * (x' & 7)) << 11 */
  alignas(16) uint32_t qpp_tab[2][OAI4G_MAX_CHUNKS * 4];
  /* 32-fold (oai4g_qpp_fold32; sizes with 1024 | K): with Q = K/32, Pi(k + Q) = Pi(k) + s Q mod K.
   * qpp_f32 = 0 for a size that keeps the quarter fold, else s (odd, bits 0-4) | ceil(2^20 / (Q/32))
   * << 5 (tile index -> block), and then qpp_tab holds, as uint16 entries k < Q, the word index
   * x' = Pi(k) mod Q (bits 7-14) and the rotate s^-1 (Pi(k) div Q) mod 32 (bits 0-4) */
  uint32_t qpp_f32[2];
  /* quarter folding: Pi(k + K/4) = Pi(k) + c4 mod K with c4 = f1 K/4 mod K in {K/4, 3K/4}
   * (f2 even, 8 | K); qpp_s3 = (c4 == 3K/4) */
  uint32_t qpp_s3[2];
  /* closed-form unit -> (block, word) map of the ilv word space: n0 blocks of size kk[0] first
   * (u0 = n0 kw[0] words), then blocks of kk[1]; kmag[i] = ceil(2^20 / kw[i]) */
  uint32_t n0, u0, kk[2], kw[2], kmag[2];
  /* per block size (index as kk): sub-block interleaver / rate-matching geometry, so the encoder
   * derives block metadata from wave-uniform scalars instead of per-lane table loads */
  uint32_t Rk[2], NDk[2], Ncbk[2], Nnnk[2], k0ck[2];
  uint32_t ntk[2], t0k[2], ntmag[2];   /* tiles per block, v0 tiles per block, ceil(2^20 / ntk) */
  uint32_t rm_wrapt[2];                /* the tile whose run straddles the circular buffer's end (RM_DST_WRAP), or ~0 */
  /* NULL columns of w per block size: bit w' of [0] = row 0 of v0 / v1 column w' is NULL
   * (bitrev5(w') < ND), of [1] = row 0 of v2 column w' is NULL (bitrev5(w') + 1 < ND) */
  uint32_t nullcol[2][2];
  /* per subframe index: blocks r < esplit have E = E[sf][0], the rest E[sf][C-1]; ew = words of
   * each, emag = ceil(2^32 / ew) */
  uint32_t esplit[10], ew[10][2], emag[10][2];
  uint32_t nnull[2];
  uint16_t nullpos[2][OAI4G_MAX_NULLS]; /* sorted NULL positions of w for K = Kminus / Kplus */
  /* per subframe index */
  uint32_t G[10];
  uint32_t E[10][OAI4G_MAX_CB];
  uint32_t roff[10][OAI4G_MAX_CB + 1];
  int16_t qam_a[8], qam_b[8];   /* amp_rho-scaled QAM levels (dlsch_modulation.c:1223-1246) */
  int16_t qpsk_a, qpsk_b;
  /* ALAMOUTI (dlsch_modulation.c:362-546) and single-layer precoding (:750-866): qam_a/qam_b hold the
   * 1/sqrt2-scaled levels (amp/sqrt2 * table >> 15) and the QPSK symbol is scaled after its sign
   * (and after its rotation): [pilot][+g, -g] */
  int16_t alm_qpsk[2][2];
  uint32_t stream_words;        /* LDS words per stream per block (padded) */
  /* CRC tree combine (x^(8*per*2^d) mod P as 6 nibble tables of 16 entries per level) */
  uint32_t crc_per_tb;          /* bytes per lane, 256 lanes, CRC-24A over the TB (C == 1) */
  uint32_t crc_per_cb;          /* C > 1: bytes per lane, crc_lpb lanes per block, CRC-24A and -24B together */
  uint32_t crc_lpb;             /* lanes per block (16, 32 or 64) */
  uint32_t crcmul_tb[8][6][16];
  /* C > 1: block r's CRC-24A contribution to the TB's, x^(8 (A_bytes - end_r)) mod P_A (end_r = the
   * block's last TB byte + 1), as 6 nibble tables */
  uint32_t crcmul_blk[OAI4G_MAX_CB][96];
  /* two-level in-wave combine: lane l's chunk CRC times x^(8 per (7 - l mod 8)) ([0][j] = power
   * j), XOR over the 8 lanes of its group, times x^(64 per (g - 1 - l / 8)) ([1][j], g groups of 8),
   * XOR over the g groups */
  uint32_t crc2_tb[2][8][96];
  uint32_t crc2_cb[2][2][8][96];   /* [P_A, P_B] at crc_per_cb */
  /* sub-block interleaver + rate matcher plan per block size (k_encode phase 4), tile t of a
   * block (v0 tiles of 32 rows, then interlaced tiles of 16 y1 / y2 row pairs), half-wave lane L:
   *   rm_src: before the 32x32 transpose, the stream bits lane L loads: bit shift (0..4) and LDS
   *           word (5..19) relative to the block's streams minus one word (s sw + (pos >> 5) + 1),
   *           RM_SRC_LAST (stream-2 row R-1: bit 31 is y2_0, not a stream bit);
   *   rm_dst: after it, the run of column lane L: circular offset o = (compact index - k0c) mod
   *           Nnn, leading NULLs z << 16, run length m << 21 (0: nothing), RM_DST_WRAP when
   *           o + m > Nnn. */
  uint32_t rm_src[2][OAI4G_RM_TILES + 1][32];   /* + one idle tile: a pair's second tile may be past nt */
  uint32_t rm_dst[2][OAI4G_RM_TILES + 1][32];
  /* the tile pairs of every block in order (oai4g_rm_pair_schedule): a wave of phase 4 takes pairs
   * i = first + wave, + nwaves, ... of a half of the blocks, [rm_pair0[first block], rm_pair0[end block]),
   * and reads one descriptor per pair with a scalar load: bit 0 = the pair holds the block size's wrap
   * tile, bit 1 = block size index, bits 2-5 = block, bits 16-28 = byte offset of the pair's rows in
   * rm_src / rm_dst.  E and the e-bit offset of the block come from E[sfi] / roff[sfi]. */
  uint32_t rm_pair0[OAI4G_MAX_CB + 1];
  uint32_t rm_pairs[OAI4G_MAX_CB * ((OAI4G_RM_TILES + 1) / 2)];
};

struct cfg_dev_t {
  uint32_t N_RB_DL, N, log2N, cp0, cp, spt, nsymb, n_ant, first_carrier;
  uint32_t n_cw, mimo_mode, num_pdcch, rnti, Nid_cell, first_sf, sf_step;
  uint32_t payload_stride;
  uint32_t ebits_words;         /* per codeword per subframe */
  uint32_t lds_tb_words;        /* words of TB || CRC (k_encode no longer stages it) */
  uint32_t lds_stream_words;    /* LDS words for all block streams of one codeword */
  uint32_t lds_gold_words;      /* = e-bit staging words (Gold-prefilled) */
  uint32_t lds_w_words;         /* packed sub-block interleaver output of every block */
  uint32_t lds_a_words;         /* region A: CRC tables (0-1) | interleaved words (3) | half of the e words (4) */
  uint32_t lds_b_words;         /* region B: constituent streams, from phase 0 on */
  uint32_t mod_nosat;            /* 1: k_modofdm may take the fused IDFT levels (oai4g_host.cpp mod_nosat_ok) */
  /* k_modofdm's dense item space (oai4g_mod_item): leading symbols that are no items, nsymb - mod_lz,
   * ceil(2^32 / mod_per); set by oai4g_host.cpp mod_items_setup wherever the static REs change */
  uint32_t mod_lz, mod_per, mod_permag;
  uint32_t crctab[2][256];     /* CRC byte tables (crc_byte.c:98-105): [0] CRC-24A, [1] CRC-24B */
  cw_dev_t cw[2];
  uint32_t symbase[10][14];     /* data REs before symbol l */
  uint32_t symnre[10][14];      /* data REs in symbol l (32-bit: the modulator reads it with a scalar load) */
  uint32_t n_cu;                /* compute units of the device (persistent grids) */
  const uint16_t *remap;        /* [10][14][N] data-RE index | parity<<15; OAI4G_CRS_CODE | pilot
                                   symbol<<9 | port<<8 | m for a CRS RE; OAI4G_CTL_CODE for a static RE of
                                   set_control / set_common; 0xFFFF = none (k_modulate_bytes reads it) */
  const uint16_t *remap_tm;     /* k_modofdm's copy, thread-major: per (sf, l), [t][n] is the RE at t + (N/16) n,
                                   so each thread fetches its 16 codes with two 16-B loads.  A data RE's code
                                   is the byte offset of its staged entry (oai4g_mod_entry_shift; | parity<<15
                                   with 2-byte entries), every other RE's the zero sentinel's */
  uint32_t with_crs;            /* the grid carries CRS */
  uint32_t pilmask;             /* bit l: symbol l carries CRS (QAM levels scaled by rho_B) */
  uint32_t ctlmask[10];         /* bit l: symbol l of subframe index sf carries static REs of set_control /
                                   set_common (PCFICH, PDCCH, PHICH, PSS, SSS, PBCH) */
  uint32_t ctl_on;              /* any of them */
  const uint32_t *gold_tab;     /* [10][n_cw][ebits_words] scrambling words (dlsch_scrambling.c:51-97) per
                                   subframe index and codeword: c_init depends on nothing else */
  const uint32_t *gold_x1;      /* [256]     x1 state after 50+16l word steps */
  const uint32_t *gold_x2j;     /* [256][32] columns of M2^(50+16l) */
  const uint32_t *tw;           /* 2 x OAI4G_TW_TOTAL packed twiddles t, then (-t.im, t.re) */
  const uint32_t *stat_tm;      /* [10][14][stat_planes][N] thread-major like remap_tm: the packed IQ each
                                   kernel antenna takes at a CRS or static RE, 0 elsewhere (null without
                                   either; k_modofdm ORs it over the data path, which reads the zero
                                   sentinel there; built by build_stat_tm) */
  uint32_t stat_planes;         /* 1 (TM1: one transform) or the TX antennas */
  uint32_t pad2;
};

/* What of a codeword's rate-matching plan depends on the redundancy version, for k_encode_rv
 * (oai4g_tx_config_enable_tb_rv): the k0c-relative run offsets and wrap marks of rm_dst, the wrap
 * tiles and the pair schedule's wrap bits.  One table per (rv, codeword), [4][n_cw], outside
 * cfg_dev_t; rm_dst, rm_pairs and rm_pair0 have cw_dev_t's layouts, so a pair descriptor's byte
 * offset addresses cw.rm_src and this rm_dst alike. */
struct enc_rv_tab_t {
  uint32_t rm_dst[2][OAI4G_RM_TILES + 1][32];
  uint32_t rm_pair0[OAI4G_MAX_CB + 1];
  uint32_t rm_pairs[OAI4G_MAX_CB * ((OAI4G_RM_TILES + 1) / 2)];
  uint32_t rm_wrapt[2];
  uint32_t k0ck[2];            /* the rv's compacted start per block size (host-side record) */
  uint32_t pad[3];
};
static_assert(sizeof(enc_rv_tab_t) % 16 == 0, "tables are laid out back to back");

/* ---------------- launch helpers implemented in the .hip files ---------------- */
/* encoder path */
/* k_encode_rv: transport block (sf, cw) takes its redundancy version d_rv[sf n_cw + cw] & 3 and that
 * rv's table d_tabs[rv n_cw + cw] */
hipError_t oai4g_launch_encode_rv(const cfg_dev_t *d_cfg, const cfg_dev_t *h_cfg, int n_sf, const uint8_t *d_payload,
                                  const uint8_t *d_rv, const enc_rv_tab_t *d_tabs, uint32_t *d_ebits, hipStream_t s);
hipError_t oai4g_launch_encode(const cfg_dev_t *d_cfg, const cfg_dev_t *h_cfg, int sf0, int n_sf,
                               const uint8_t *d_payload, uint32_t *d_ebits, hipStream_t s);
hipError_t oai4g_encode_occupancy(const cfg_dev_t *h_cfg, int *blocks_per_cu, size_t *lds_bytes);
hipError_t oai4g_launch_encode_phase(const cfg_dev_t *d_cfg, const cfg_dev_t *h_cfg, int n_sf,
                                     const uint8_t *d_payload, uint32_t *d_ebits, int stop_phase, hipStream_t s);
struct enc_debug_t {
  uint8_t *c;      /* [C][8+3+768]                         */
  uint8_t *d;      /* [C][OAI4G_D_BYTES] (offset 96 = d[r][96]) */
  uint8_t *w;      /* [C][OAI4G_W_BYTES]                   */
  uint8_t *e;      /* [G] pre-scrambling rate-matcher output */
  uint8_t *b;      /* [A/8+4] TB with CRC appended          */
};
hipError_t oai4g_launch_encode_debug(const cfg_dev_t *d_cfg, const cfg_dev_t *h_cfg, int cw, int sf,
                                     const uint8_t *d_payload, enc_debug_t dbg, hipStream_t s);
hipError_t oai4g_launch_crc24(const uint8_t *d_in, int bitlen, uint32_t poly_top, uint32_t *d_out, hipStream_t s);
hipError_t oai4g_launch_turbo_bytes(const uint8_t *d_c, int nbytes, uint8_t *d_out, uint32_t f1, uint32_t f2,
                                    hipStream_t s);
hipError_t oai4g_launch_subblock_bytes(uint32_t D, const uint8_t *d_dfull, uint8_t *d_w, hipStream_t s);
hipError_t oai4g_launch_rm_bytes(const uint8_t *d_w, uint32_t Ncb, uint32_t k0, uint32_t E, uint8_t *d_e,
                                 uint32_t *d_status, hipStream_t s);
/* k_rm_bytes for the C blocks of a transport block in one launch: per block the byte offset of its
 * w in d_w, Ncb, k0, E and the offset of its e bytes in d_e */
struct rm_blk_t {
  uint32_t woff, Ncb, k0, E, eoff, pad[3];
};
hipError_t oai4g_launch_rm_bytes_blocks(const uint8_t *d_w, const rm_blk_t *d_blk, int C, uint32_t max_Ncb, uint8_t *d_e,
                                        uint32_t *d_status, hipStream_t s);
hipError_t oai4g_launch_scramble_bytes(uint8_t *d_e, int n_entries, uint32_t c_init, const uint32_t *d_gold_x1,
                                       const uint32_t *d_gold_x2j, hipStream_t s);
hipError_t oai4g_launch_fill(uint8_t *d, size_t bytes, uint64_t seed, hipStream_t s);
/* CRS into nsym_grids OFDM-symbol grids: job j writes grid `out + jobs[j].off` (N REs) with port
 * jobs[j].p, pilot l of slot Ns from gold[Ns][l][14] */
struct crs_job_t {
  uint32_t off;
  uint8_t Ns, l, p, pad;
};
hipError_t oai4g_launch_crs(int32_t *d_out, const crs_job_t *jobs, int n_jobs, const uint32_t *d_gold, int16_t amp,
                            uint32_t N, uint32_t N_RB, uint32_t nushift, uint32_t first_carrier, hipStream_t s);
hipError_t oai4g_launch_diag_stream(const void *src, void *dst, size_t bytes, int mode, hipStream_t s);

/* uplink turbo decoding (oai4g_decode.hip) */
size_t oai4g_td_block_bytes(uint32_t K);
hipError_t oai4g_launch_td16(int n_cb, uint32_t K, const int16_t *d_llr, size_t llr_stride, uint8_t *d_out,
                             size_t out_stride, uint8_t *d_iters, uint32_t max_it, uint32_t crc_type, uint32_t F,
                             const uint16_t *d_pi /* pi4 | pi5 | pi6, K each */, uint8_t *d_scratch, hipStream_t s,
                             uint32_t cg = 1, uint32_t c_per = 1, uint32_t r0 = 0);
/* 8-bit turbo decoder (oai4g_decode8.hip) */
size_t oai4g_td8_wave_bytes(uint32_t K);
hipError_t oai4g_launch_td8(int n_cb, uint32_t K, const int16_t *d_llr, size_t llr_stride, uint8_t *d_out,
                            size_t out_stride, uint8_t *d_iters, uint32_t max_it, uint32_t crc_type, uint32_t F,
                            const uint16_t *d_pi, uint8_t *d_scratch, hipStream_t s);
/* batched UL receive chain (ulsch_decoding.c:1208-1350): per code-block pattern (block size,
 * filler) the NULL map and compact indices of the rate-matching circular buffer */
#define OAI4G_UL_MAX_C 16
struct ul_pat_t {
  uint32_t D, R, Ncb, Nnn, k0c;
  uint32_t k0cr[4];                /* k0c of rvidx 0..3 (the HARQ rounds) */
  const uint8_t *dummy;            /* [3 R 32] LTE_NULL marks */
  const uint32_t *cidx;            /* [Ncb] compact index */
};
struct ul_dev_t {
  uint32_t C, Rmax;
  uint32_t E[OAI4G_UL_MAX_C], off[OAI4G_UL_MAX_C], pat_of[OAI4G_UL_MAX_C];
  ul_pat_t pat[3];
};
hipError_t oai4g_launch_ul_rm_deint(const ul_dev_t *d_cfg, const ul_dev_t *h_cfg, int n_tb, const int16_t *d_e,
                                    size_t e_stride, int16_t *d_dfull, size_t d_stride, hipStream_t s);
/* HARQ form: w [rows][w_stride] int16 circular soft buffers kept across rounds; the round's rv and
 * clear (round 0) select k0 and the reset; then w -> the decoder's d buffers */
hipError_t oai4g_launch_ul_rm_harq(const ul_dev_t *d_cfg, const ul_dev_t *h_cfg, int n_tb, const int16_t *d_e,
                                   size_t e_stride, int16_t *d_w, size_t w_stride, uint32_t rv, int clear,
                                   int16_t *d_dfull, size_t d_stride, hipStream_t s);
/* the same with rv (0..3) and clear (0 / 1) per transport block: device arrays [n_tb] */
hipError_t oai4g_launch_ul_rm_harq_tb(const ul_dev_t *d_cfg, const ul_dev_t *h_cfg, int n_tb, const int16_t *d_e,
                                      size_t e_stride, int16_t *d_w, size_t w_stride, const uint8_t *d_rv,
                                      const uint8_t *d_clear, int16_t *d_dfull, size_t d_stride, hipStream_t s);
hipError_t oai4g_launch_rm_rx(const int16_t *d_soft, uint32_t E, int16_t *d_w, const uint8_t *d_dummy,
                              const uint32_t *d_cidx, uint32_t Ncb, uint32_t Nnn, uint32_t k0c, int clear, hipStream_t s);
hipError_t oai4g_launch_subblock_deint(uint32_t D, int16_t *d_dfull, const int16_t *d_w, hipStream_t s);

/* OFDM path */
extern int g_modofdm_grid_cap;   /* oai4g_set_modofdm_grid_cap (oai4g_host.cpp): > 0 caps k_modofdm's grid */
hipError_t oai4g_launch_modofdm(const cfg_dev_t *d_cfg, const cfg_dev_t *h_cfg, int sf0, int n_sf,
                                const uint32_t *d_ebits, int32_t *d_iq, hipStream_t s);
struct ofdm_sym_t {
  uint32_t in_off;   /* int32 index of the symbol's frequency-domain input */
  uint32_t out_off;  /* int32 index of the symbol's time-domain body (after the CP) */
  uint32_t cp;       /* cyclic-prefix length written in front of the body */
};
hipError_t oai4g_launch_ofdm(const int32_t *d_in, int32_t *d_out, int log2n, int nsym, const ofdm_sym_t *syms,
                             int scale, const uint32_t *d_tw, hipStream_t s);
hipError_t oai4g_launch_idft_strided(const int32_t *d_in, int32_t *d_out, int log2n, int n_jobs, size_t in_stride,
                                     uint32_t in_off, size_t out_stride, int scale, const uint32_t *d_tw, hipStream_t s);
/* lte_est_freq_offset's integer part (oai4g_chest.hip) */
hipError_t oai4g_launch_freq_offset(const int32_t *d_est, size_t est_stride, int n_jobs, int N_RB, uint32_t row_off,
                                    uint32_t prev_off, int32_t *d_omega, hipStream_t s);
/* control region (oai4g_ctrl.hip): PCFICH */
struct pcfich_args_t {
  uint32_t c_init;      /* pcfich_scrambling x2 (pcfich.c:97) */
  uint32_t cfi;         /* num_pdcch_symbols, 1..3 */
  int16_t gain;         /* QPSK amplitude (pcfich.c:168-171) */
  uint8_t mode1;        /* 1 = SISO mapping, 0 = ALAMOUTI */
  uint8_t nushift3;     /* nushift % 3 */
  uint32_t reg_off[4];  /* first RE of each REG in the symbol, DC-skip applied (pcfich.c:210-213) */
  uint32_t n_ant;
};
hipError_t oai4g_launch_pcfich(int32_t *d_g0, int32_t *d_g1, const pcfich_args_t &a, hipStream_t s);

/* PDCCH (generate_dci_top, dci.c:2024-2346) */
#define OAI4G_MAX_DCI 32
struct dci_dev_t {
  uint8_t flip[8];      /* the pdu bytes in generate_dci0's order (dci.c:233-251) */
  uint32_t A;           /* DCI bits */
  uint32_t L;           /* log2 aggregation level */
  int32_t nCCE;
  uint32_t rnti;
};
struct dci_args_t {
  uint32_t n_dci;
  dci_dev_t dci[OAI4G_MAX_DCI];
  uint32_t nbits;       /* scrambled PDCCH bits, 8 * nquad (pdcch_scrambling length) */
  uint32_t c_init;      /* (subframe << 9) + Nid_cell */
  uint32_t n_re;        /* REs mapped */
  int16_t gain;         /* QPSK amplitude (dci.c:2170-2174) */
  uint8_t mode1;        /* 1: SISO (<NIL> -> 0), 0: ALAMOUTI (<NIL> -> +gain) */
  uint8_t n_ant;        /* antennas written (nb_antennas_tx_eNB > 1 ? 2 : 1) */
};
/* map[r] = grid offset of mapped RE r (symbol * N + subcarrier), src[r] = its QPSK symbol index
 * after quadruplet interleaving and the cyclic shift.  One workgroup. */
hipError_t oai4g_launch_dci(const dci_args_t &a, const uint32_t *d_map, const uint16_t *d_src, int32_t *d_g0,
                            int32_t *d_g1, uint32_t g1_stride, hipStream_t s);

/* synchronisation / broadcast / HARQ-indicator channels (oai4g_ctrl.hip) */
struct sync_args_t {    /* generate_pss (pss.c:50-103) / generate_sss (sss.c:47-92) */
  int16_t val[62][2];   /* PSS: the Zadoff-Chu table entries (primary_synch.h); SSS: (d(n), 0), d = +-1 */
  int16_t a;            /* amp or (amp ONE_OVER_SQRT2_Q15) >> 15 */
  uint8_t pss;          /* 1: (a v) >> 15 per component; 0: (int16)(a v), imaginary 0 */
  uint8_t n_ant;
  uint32_t N;           /* ofdm_symbol_size: k starts at N - 31 and skips DC */
};
hipError_t oai4g_launch_sync(int32_t *const *d_sym /* per antenna: the symbol's N REs */, const sync_args_t &a,
                             hipStream_t s);
struct pbch_args_t {    /* generate_pbch (pbch.c:161-420) */
  uint8_t a[3];         /* pbch_a: the pdu bytes reversed (pbch.c:214-215) */
  uint8_t encode;       /* frame_mod4 == 0: encode and scramble into e; else map the stored e */
  uint16_t amask;       /* CRC16 antenna mask (pbch.c:223-238) */
  uint16_t E;           /* 1920 (normal CP) / 1728 */
  uint32_t Nid;         /* scrambling c_init (pbch.c:770) */
  uint32_t quarter;     /* frame_mod4 */
  uint32_t N;           /* ofdm_symbol_size */
  uint32_t pil_mask;    /* bit l (0..3): symbol nsymb/2 + l is a pilot symbol for the PBCH (pbch.c:345-362) */
  uint32_t nushift3;
  int16_t gain;         /* (amp ONE_OVER_SQRT2_Q15) >> 15 */
  uint8_t mode1;
  uint8_t n_ant;
};
/* d_g[a]: 4 consecutive symbols (nsymb/2 .. +3) of antenna a; d_e: the 1920-bit state (bytes) */
hipError_t oai4g_launch_pbch(int32_t *const *d_g, uint8_t *d_e, const pbch_args_t &a, hipStream_t s);
#define OAI4G_MAX_PHICH 64
struct phich_item_t {
  uint32_t c_init;      /* ((subframe + 1)(Nid + 1)) << 9 + Nid (phich.c:440) */
  uint32_t reg_off[3];  /* first RE of each REG relative to the subframe's symbol 0 (phich.c:556-561) */
  uint8_t nseq, hi;
};
struct phich_args_t {   /* generate_phich (phich.c:401-780), normal CP */
  uint32_t n;
  phich_item_t it[OAI4G_MAX_PHICH];
  int16_t gain;         /* SISO (amp 23170) >> 15, ALAMOUTI amp / 2 */
  uint8_t mode1;
  uint8_t n_ant;
  uint32_t nushift;     /* < 3 */
  uint32_t win;         /* REs of the window the offsets index (2 symbols) */
};
/* d_g[a]: window of symbols 0..1 of the subframe, antenna a; d_acc: 4 * win int32 scratch */
hipError_t oai4g_launch_phich(int32_t *const *d_g, int32_t *d_acc, const phich_args_t &a, hipStream_t s);

/* UE receive front end (oai4g_fep.hip): per-symbol CP removal + forward DFT */
#define OAI4G_FEP_MAX_SYM 14
struct fep_args_t {
  int n_units;        /* items x nsym */
  int nsym;           /* symbols per item */
  uint32_t in_stride, in_len, out_stride;   /* int32 samples */
  uint32_t in_off[OAI4G_FEP_MAX_SYM];       /* DFT window start of each symbol (< in_len) */
  uint32_t out_off[OAI4G_FEP_MAX_SYM];      /* output offset of each symbol */
  int scale;
};
hipError_t oai4g_launch_fep(const int32_t *d_in, int32_t *d_out, int log2n, const fep_args_t &a,
                            const uint32_t *d_twf, int n_cu, hipStream_t s);
hipError_t oai4g_launch_modulate_bytes(const cfg_dev_t *d_cfg, const cfg_dev_t *h_cfg, int sf,
                                       const uint8_t *d_e0, const uint8_t *d_e1, int32_t *d_grid, hipStream_t s);

/* UE PDSCH demodulation (oai4g_rx.hip): TM1, one receive antenna, even N_RB_DL */
/* downlink channel estimation (lte_dl_channel_estimation, high_speed_flag = 1, one RX antenna) */
struct chest_dev_t {
  uint32_t N, N_RB, nsymb, Ncp, fco, p;
  uint32_t first_sf, sf_step;
  uint32_t branch;                /* 1: the 6 / 15 / 25 / 50 / 100 PRB interpolators; 0: "not implemented" (rows of 0) */
  uint32_t k[2];                  /* pilot offset (nu + nushift) % 6 for pilot symbols l = 0 / l > 0 */
  uint32_t off2[2];               /* first bin of the pilots above DC: 1 + k, or 1 + nushift + 3 p at 15 PRB */
  uint32_t elem_syms;             /* symbols between batch elements in rxdataF (nsymb; 2 nsymb in dlsim's BLER
                                     loop, where each trial's subframe is followed by the next one) */
  uint32_t next_syms;             /* symbols from an element's start to the symbol 0 closing its rows 12 / 13 */
  int16_t filt[2][8][24];         /* fl, f2l2, f, f2, fr, f2r2, f_dc, f2_dc (filt96_32.h) for k[0] / k[1] */
  uint32_t gold[20][2][14];       /* lte_gold_table */
};
/* UE control decoding (oai4g_ctrl_rx.hip: k_cc_decode), one wave per tail-biting decode.  A launch
 * decodes n_items x n_jobs: batch item i (a subframe, a PBCH) has its soft bits at e + i e_stride, job j
 * (a DCI candidate) starts e_off into them. */
struct cc_job_t {
  uint32_t e_off;
  uint16_t E;           /* soft bits summed: 72 << L, pbch_E (unused in raw mode) */
  uint16_t D;           /* trellis steps */
  uint16_t plan_off;    /* plan[plan_off + 3 i + s]: first e index of d^(s)_i (oai4g_cc_rx_plan) */
  uint16_t crc_bits;    /* payload bits in front of the CRC16; 0: no CRC */
};
struct cc_args_t {
  const int8_t *e;
  size_t e_stride;
  const cc_job_t *jobs;
  uint32_t n_jobs, n_items;
  const uint16_t *plan;
  const uint32_t *gold;     /* PBCH: Gold words of c_init = Nid_cell, else null */
  const uint8_t *quarter;   /* PBCH: frame_mod4 of every item */
  uint8_t *out;             /* per decode out_stride bytes: the decoded bytes, and in the last four
                               crc16 ^ received CRC (little endian), the clamp flag, the start state */
  uint32_t out_stride;
  uint8_t *metrics;         /* null, or 64 final path metrics per decode */
  uint32_t raw;             /* 1: e holds the 3 D Viterbi inputs themselves (phy_viterbi_lte) */
  uint32_t pbch_out;        /* 1: the record is 4 bytes, the reversed MIB and the antenna count (0xFF: none) */
  /* PDCCH batch: the soft bits come straight from the compensated symbols through the gather table of
   * the item's subframe index (first_row + item) mod 10, and the jobs are that row's candidates */
  const uint32_t *tab;      /* null, or [10][tab_stride]: per soft bit the int16 index into the item's comp | negate << 31 */
  uint32_t tab_stride;
  const int16_t *comp;      /* [n_items][comp_stride] */
  size_t comp_stride;
  uint32_t first_row;
};
#define OAI4G_PDCCH_NONE 0xFFFFFFFFu
/* pdcch_llr (dci.c:603) + pdcch_unscrambling (:1932) of one soft bit: clip to [-32, 31], negate where the Gold bit is 0 */
static inline __host__ __device__ int8_t oai4g_pdcch_soft(const int16_t *comp, uint32_t t)
{
  if (t == OAI4G_PDCCH_NONE) return 0;
  const int v = comp[t & 0x7FFFFFFFu];
  const int c = v > 31 ? 31 : (v < -32 ? -32 : v);
  return (int8_t)((t >> 31) ? -c : c);
}
hipError_t oai4g_launch_pdcch_soft(const int16_t *d_comp, const uint32_t *d_tab, uint32_t n, int8_t *d_e, hipStream_t s);

/* dci_decoding_procedure0's rules (dci.c:2661-2784) on one decoded candidate, shared by the host drop-in
 * and the batch's second stage */
typedef oai4g_pdcch_plan_t pdcch_plan_t;   /* one dci_decoding_procedure0 call */
struct pdcch_cand_t {
  uint16_t cce;           /* CCEind */
  uint8_t plan;           /* its plan entry */
  uint8_t first;          /* 1: the first candidate of its plan entry */
};
struct pdcch_state_t {
  uint32_t map[3];        /* CCEmap0..2 */
  uint8_t dci_cnt, format0_found, format_c_found;
  uint8_t overflow;       /* 1: a match found no room in dci_alloc and was dropped */
  int32_t nCCE;           /* lte_ue_pdcch_vars->nCCE[subframe]; untouched when nothing stores it */
};
#define OAI4G_PDCCH_REC 16u   /* batch record: 8 decoded bytes, 4 spare, the 4-byte trailer */
static inline __host__ __device__ void oai4g_pdcch_resolve(pdcch_state_t &st, const pdcch_plan_t &pl, uint32_t cce,
                                                           const uint8_t *out, uint32_t crc, uint32_t crnti, uint32_t si_rnti,
                                                           uint32_t ra_rnti, oai4g_dci_alloc_t *alloc, uint32_t cap)
{
  const uint32_t mask = ((1u << (1u << pl.L)) - 1u) << (cce & 31u);
  uint32_t &m = st.map[cce >> 5];
  if (m & mask) return;                                                /* a CCE is taken: skipped (:2665) */
  if (!((pl.L > 1 && (crc == si_rnti || crc == ra_rnti)) || crc == crnti)) return;
  if (st.dci_cnt >= cap) {                                             /* no room left: the match only marks its CCEs */
    st.overflow = 1;
    m |= mask;
    return;
  }
  oai4g_dci_alloc_t &d = alloc[st.dci_cnt];                            /* filled before acceptance is known */
  d.dci_length = pl.sizeof_bits;
  d.rnti = (uint16_t)crc;
  d.L = pl.L;
  d.nCCE = (int32_t)cce;
  const int nb = pl.sizeof_bytes <= 4 ? 4 : 8;
  for (int i = 0; i < nb; i++) d.dci_pdu[nb - 1 - i] = out[i];
  if (crc == si_rnti) {
    d.format = pl.format_si;
    st.dci_cnt++;
  } else if (crc == ra_rnti) {
    d.format = pl.format_ra;
    st.nCCE = (int32_t)cce;
    st.dci_cnt++;
  } else if (crc == crnti) {
    if (pl.format_c == 0 && (out[0] & 0x80) == 0) {                    /* format 0 or 1A by the first bit (:2730) */
      if (st.format0_found == 0) {
        d.format = 0;
        st.format0_found = 1;
        st.dci_cnt++;
        st.nCCE = (int32_t)cce;
      }
    } else if (pl.format_c == 0) {
      d.format = 2;                                                    /* format1A */
      st.dci_cnt++;
      st.nCCE = (int32_t)cce;
    } else if (st.format_c_found == 0) {
      d.format = pl.format_c;
      st.dci_cnt++;
      st.format_c_found = 1;
      st.nCCE = (int32_t)cce;
    }
  }
  m |= mask;                                                           /* also when the counter did not advance */
}
struct pdcch_resolve_args_t {
  const uint8_t *rec;          /* [n_sf][n_jobs][OAI4G_PDCCH_REC] */
  const pdcch_cand_t *cands;   /* [10][n_jobs] */
  const uint32_t *n_cand;      /* [10] */
  const pdcch_plan_t *plans;
  uint32_t n_jobs, n_sf, first_row;
  uint32_t crnti, si_rnti, ra_rnti;
  oai4g_pdcch_rx_result_t *out;
};
hipError_t oai4g_launch_pdcch_resolve(const pdcch_resolve_args_t &a, hipStream_t s);
#define OAI4G_CC_NMAX 512
hipError_t oai4g_launch_cc_decode(const cc_args_t &a, uint32_t nmax, hipStream_t s);

/* The DCI search over subframes whose num_pdcch_symbols was detected on the device (k_pdcch_front): subframe
 * i takes the jobs, gather table and candidates of the configuration built for cfi[i] (1..3, anything else
 * decodes nothing), at subframe index (first_row + i sf_step) mod 10.  The records of a subframe lie n_jobs
 * (the largest of the three) apart. */
struct pdcch_det_set_t {
  const cc_job_t *jobs;        /* [10][n_jobs] */
  const uint32_t *tab;         /* [10][tab_stride] */
  const pdcch_cand_t *cands;   /* [10][n_jobs] */
  const uint32_t *n_cand;      /* [10] */
  const uint16_t *plan;        /* the receive plans of the convolutional code */
  uint32_t n_jobs, tab_stride;
};
struct cc_det_args_t : cc_args_t {
  pdcch_det_set_t set[3];
  const uint8_t *cfi;          /* [n_items] */
  uint32_t sf_step;
};
struct pdcch_resolve_det_args_t : pdcch_resolve_args_t {
  pdcch_det_set_t set[3];
  const uint8_t *cfi;
  uint32_t sf_step;
};
hipError_t oai4g_launch_cc_decode_detected(const cc_det_args_t &a, hipStream_t s);
hipError_t oai4g_launch_pdcch_resolve_detected(const pdcch_resolve_det_args_t &a, hipStream_t s);

/* The PDCCH / PCFICH receive front end (oai4g_pdcch_front.hip: k_pdcch_front), one workgroup per subframe */
struct pdcch_front_args_t {
  const int32_t *rxF;          /* [n_sf][nb_rx][nsymb][N] */
  size_t rx_sf_stride, rx_ant_stride;   /* words */
  const int32_t *est[4];       /* plane (p << 1) + a: [n_sf][nsymb][N] */
  size_t est_sf_stride;        /* words */
  uint32_t N, N_RB, fco, nushift3;
  uint32_t nb_tx, nb_rx, alamouti, high_speed;
  uint32_t first_sf, sf_step, n_sf;
  uint32_t pcf_word[4];        /* pcfich_reg * 4: the REGs' first words in the packed symbol 0 */
  uint32_t pcf_gold[10];       /* the PCFICH scrambling word of every subframe index */
  int32_t *comp;               /* [n_sf][36 N_RB]: plane 0 of rxdataF_comp */
  int32_t *planes;             /* null, or [n_sf][4][36 N_RB]: the compensated planes before MRC */
  uint8_t *cfi, *log2_maxh;    /* [n_sf] */
};
hipError_t oai4g_launch_pdcch_front(const pdcch_front_args_t &a, hipStream_t s);
/* rx_pcfich alone on a plane 0 in device memory: pcf_word as above, gold the subframe's scrambling word */
hipError_t oai4g_launch_rx_pcfich(const int32_t *d_comp, const uint32_t pcf_word[4], uint32_t gold, uint8_t *d_out, hipStream_t s);

/* The PBCH receive front end (oai4g_pbch_front.hip: k_pbch_front), one workgroup per subframe, one wave per
 * PBCH symbol.  Every output pointer may be null. */
#define OAI4G_PBCH_WORDS 288u    /* rxdataF_comp of the PBCH: four regions of 72 words */
#define OAI4G_PBCH_SOFT 480u     /* 96 + 96 + 144 + 144 soft bits of one subframe 0 */
struct pbch_front_args_t {
  const int32_t *rxF;          /* [n_sf][nb_rx][nsymb][N] */
  size_t rx_sf_stride, rx_ant_stride;   /* words */
  const int32_t *est[4];       /* plane (p << 1) + a: [n_sf][nsymb][N]; null where the port was not estimated */
  size_t est_sf_stride;        /* words */
  uint32_t N, N_RB, nushift3;
  uint32_t nb_tx, nb_rx, alamouti, high_speed;
  uint32_t n_sf;
  int32_t *comp;               /* [n_sf][288]: plane 0 after combining under `alamouti` */
  int32_t *planes;             /* [n_sf][4][288]: the compensated planes before MRC */
  int8_t *llr;                 /* [n_sf][2][480]: the soft bits under SISO and under ALAMOUTI */
  uint8_t *log2_maxh;          /* [n_sf][4] */
};
hipError_t oai4g_launch_pbch_front(const pbch_front_args_t &a, hipStream_t s);
/* pbch_detection's hypotheses through k_cc_decode: item i holds the two soft-bit rows of subframe i
 * (e_stride = 2 * 480), job j = 2 frame_mod4 + mimo_mode decodes row j & 1 (its e_off) over E = 480 alone, with
 * the Gold words of quarter j >> 1 (gold + 15 (j >> 1)); the rest of the reference's 1920-byte buffer is 0 and
 * adds nothing to the rate-matching sums.  The records are those of pbch_out. */
struct cc_hyp_args_t : cc_args_t {};
hipError_t oai4g_launch_cc_decode_hyp(const cc_hyp_args_t &a, hipStream_t s);
/* the first of the eight records of a subframe whose antenna count is 1 or 2 (initial_sync.c:135-161) */
hipError_t oai4g_launch_pbch_resolve(const uint8_t *d_rec, uint32_t n_sf, oai4g_pbch_detect_t *d_out, hipStream_t s);

/* rx_phich's correlation (oai4g_pbch_front.hip: k_phich_rx), one lane per item */
struct phich_rx_ent_t {        /* one (subframe index, group, sequence) */
  uint32_t neg;                /* bit i: d[i] == -1 (phich.c:1131-1222 on the subframe's scrambling word) */
  uint16_t word[3];            /* phich_reg[ngroup][quad] * 4 */
  uint16_t pad;
};
struct phich_rx_args_t {
  const int32_t *comp;         /* [n_sf][comp_stride]: plane 0 as k_pdcch_front writes it */
  size_t comp_stride;          /* words */
  const phich_rx_ent_t *tab;   /* [10][ngroup][8] */
  uint32_t ngroup, n_sf, first_sf, sf_step;
  const oai4g_phich_rx_item_t *items;
  uint32_t n_items;
  oai4g_phich_rx_out_t *out;   /* [n_items] */
};
hipError_t oai4g_launch_phich_rx(const phich_rx_args_t &a, hipStream_t s);

/* The PSS time-domain correlation of initial cell search (oai4g_sync_rx.hip: k_sync_time, k_sync_peak) */
struct sync_time_args_t {
  const uint32_t *rx;          /* [n][nb_rx][2 length] received frames, packed int16 pairs */
  const uint32_t *rep;         /* [3][N] the time-domain replicas of lte_sync_time_init, 16-byte aligned */
  uint32_t N, length, nb_rx, n;   /* ofdm_symbol_size, 5 samples_per_tti, receive antennas (1 or 2), frames */
  unsigned long long *keys;    /* [n] scratch: metric << 32 | ~(n + s), the largest wins */
  int32_t *peak;               /* [n] {peak_pos, peak_val, Nid2} */
  int32_t *corr;               /* null, or [n][3][2 length]: sync_corr_ue0..2 after abs32, every fourth entry */
};
hipError_t oai4g_launch_sync_time(const sync_time_args_t &a, hipStream_t s);
/* slot_fep at a per-frame device offset (oai4g_fep.hip: k_fep_offset): items are (frame, antenna) pairs of
 * frame_len input words; symbol sym of the run starts at ((offset + pre[sym]) & ~3) + post[sym] modulo frame_len
 * (slot_fep.c:105-150) and lands at out + frame * out_frame_stride + antenna * out_ant_stride + sym * N */
#define OAI4G_FEP_OFFSET_MAX_SYM 16
struct fep_offset_args_t {
  int n_units;                 /* frames x antennas x nsym */
  int nsym;
  uint32_t n_ant, frame_len;
  uint32_t out_frame_stride, out_ant_stride;   /* words */
  const int32_t *offset;       /* frame f's sample offset at offset[f * offset_stride] */
  uint32_t offset_stride;
  uint32_t pre[OAI4G_FEP_OFFSET_MAX_SYM];    /* slot_offset + nb_prefix_samples0 + subframe_offset of the symbol's slot */
  uint32_t post[OAI4G_FEP_OFFSET_MAX_SYM];   /* (N + nb_prefix_samples) l */
  int scale;
};
hipError_t oai4g_launch_fep_offset(const int32_t *d_in, int32_t *d_out, int log2n, const fep_offset_args_t &a,
                                   const uint32_t *d_twf, int n_cu, hipStream_t s);
/* SSS detection behind the PSS stage (oai4g_sync_rx.hip: k_sss_offsets, k_sss).  A cell record is six int32:
 * {Nid_cell, rx_offset, metric, flip, phase, status} */
#define OAI4G_CELL_WORDS 6u
#define OAI4G_SSS_ERROR 1      /* status: "SSS error condition" (initial_sync.c:373-376), the frame has no cell */
struct sss_args_t {
  const int32_t *peak;         /* [n] {peak_pos, peak_val, Nid2} */
  int32_t *cell;               /* [n] records */
  const int32_t *rxF;          /* [n][nb_rx][4][N]: symbols 5 and 6 of slot 0, then of slot 10, at the record's rx_offset */
  const uint32_t *pss;         /* [3][62] primary_synch<Nid2>[10..133] as packed int16 pairs */
  const unsigned long long *d;   /* [504][2] bit i: d0_sss / d5_sss [Nid_cell][i] is -1 */
  uint32_t n, nb_rx, N, cp, spt;
  uint32_t add_half;           /* 1: flip = 1 adds the half frame to the reported rx_offset (initial_sync.c:361-362) */
  int16_t phase_re[8], phase_im[8];   /* sss.c:218-219: floor(32767 cos / sin) of -60, -40, ... 60 degrees */
};
hipError_t oai4g_launch_sss_offsets(const sss_args_t &a, hipStream_t s);
hipError_t oai4g_launch_sss(const sss_args_t &a, hipStream_t s);
/* SC-FDMA transform precoding (oai4g_pusch.hip).  The plan of one size as the kernels read it, by value: level 0 is the
 * outermost; rcp_r / rcp_m1 are ceil(2^32 / radix) and ceil(2^32 / (M - 1)) for the index divisions */
#define OAI4G_PUSCH_LEVELS 4
struct pusch_plan_t {
  uint32_t N, n_lvl;
  uint32_t spw;                /* symbols per workgroup of 256 threads: 1, 2, 4, 8 or 16 */
  uint32_t lds_sym;            /* LDS words per symbol: N (natural order) + N + N / 12 (blocks, padded) */
  uint32_t leaf_norm;          /* 9459 behind dft12 in dft_lte / lte_idft, else 0 */
  uint32_t radix[OAI4G_PUSCH_LEVELS], M[OAI4G_PUSCH_LEVELS], norm[OAI4G_PUSCH_LEVELS], tw_off[OAI4G_PUSCH_LEVELS];
  uint32_t rcp_r[OAI4G_PUSCH_LEVELS], rcp_m1[OAI4G_PUSCH_LEVELS];
};
struct pusch_grid_t {          /* the data symbols of a subframe's grid */
  uint32_t n_data, nsymb, row; /* data symbols per subframe, symbols per subframe, words per symbol row */
  uint32_t sym[12];
};
struct pusch_mod_t {
  uint32_t Qm, h_stride, first_sf, sf_step, gold_words;
  uint32_t re_offset;          /* first RE of the allocation, < ofdm_symbol_size */
  int amp, gain_qpsk;
};
/* d_tw: per twiddle (t.re, -t.im) and (t.im, t.re) as packed int16 pairs */
hipError_t oai4g_launch_pusch_dft(const pusch_plan_t &p, const uint2 *d_tw, const uint32_t *d_in, uint32_t *d_out, uint32_t n_sym,
                                  hipStream_t s);
hipError_t oai4g_launch_pusch_idft(const pusch_plan_t &p, const uint2 *d_tw, const pusch_grid_t &g, uint32_t *d_comp, uint32_t n_sf,
                                   hipStream_t s);
hipError_t oai4g_launch_pusch_mod(const pusch_plan_t &p, const uint2 *d_tw, const pusch_grid_t &g, const pusch_mod_t &m,
                                  const uint8_t *d_h, const uint32_t *d_gold, uint32_t *d_txF, uint32_t n_sf, hipStream_t s);
void oai4g_set_error(const char *fmt, ...);
/* binds the calling thread to the device the library was initialised on (hipSetDevice is per thread) */
int oai4g_bind_thread(void);
hipError_t oai4g_launch_signal_energy(const int32_t *d_x, int n, size_t stride, uint32_t length, int32_t *d_out,
                                      hipStream_t s);
hipError_t oai4g_launch_awgn(const int32_t *d_tx, size_t tx_stride, uint32_t tx_len, const int32_t *d_tail,
                             uint32_t tail_len, int32_t *d_rx, size_t rx_stride, int n, const int32_t *d_tx_lev,
                             double offset_db, uint64_t seed, uint32_t vec0, hipStream_t s);
/* a fading-channel configuration as k_channel_taps reads it (oai4g_channel.hip); by value */
#define OAI4G_CHAN_TAPS 9               /* OAI4G_CHANNEL_MAX_TAPS */
#define OAI4G_CHAN_MAX_LENGTH 255       /* the reference's channel_length is a uint8_t */
struct chan_dev_t {
  uint32_t nb_tx, nb_rx, nb_taps, channel_length, random_aoa;
  double ricean_factor, aoa, BW, sqrt_ff, sqrt_1mff;
  double amps[OAI4G_CHAN_TAPS], delays[OAI4G_CHAN_TAPS];
  const double *R;       /* [ceil(nb_taps / 3)][npair][npair][re, im], npair = nb_tx nb_rx */
  double *a;             /* [n_vectors][nb_taps][npair][re, im] */
  double *ch;            /* [n_vectors][npair][channel_length][re, im] */
  uint8_t *first_run;    /* [n_vectors] */
};
hipError_t oai4g_launch_channel_taps(const chan_dev_t &c, int n, uint64_t seed, uint32_t vec0, uint32_t step,
                                     const double *d_draws, hipStream_t s);
/* k_multipath's arguments: element strides (int32 IQ words, or [re, im] double pairs in the double form) */
struct multipath_args_t {
  uint32_t nb_tx, nb_rx, channel_length, dd, tx_len, tail_len, seg_len, vec4;
  size_t tx_stride, tx_ant_stride, rx_stride, rx_ant_stride, seg_stride;
  const void *tx, *tail;
  void *rx;
  const double *ch;      /* vector 0's taps: [npair][channel_length][re, im], a vector apart npair channel_length */
  double path_loss, offset_db;
  const int32_t *tx_lev; /* [n][nb_tx] */
  uint32_t seed_lo, seed_hi, vec0;
};
hipError_t oai4g_launch_multipath(const multipath_args_t &a, int n, bool double_form, hipStream_t s);
/* device arrays of oai4g_harq_advance (oai4g_channel.hip: k_harq_advance) */
struct harq_state_t {
  uint8_t *round;        /* [n_slots] 0 .. num_rounds - 1 */
  uint32_t *trial;       /* [n_slots] running transport-block index of the slot */
  uint8_t *rv;           /* [n_slots][n_cw] */
  uint8_t *clear;        /* [n_slots] */
  uint8_t *done;         /* [n_slots] 0: retransmission follows; 1: finished, decoded; 2: finished, not decoded */
  uint32_t *counters;    /* [8] round_trials[4] | errs[4] */
  uint8_t *payload;      /* [n_slots][8 row_words] bytes, 8-byte aligned */
};
hipError_t oai4g_launch_harq_advance(const harq_state_t &st, uint32_t n_slots, uint32_t C, uint32_t max_it,
                                     uint32_t num_rounds, uint32_t n_cw, uint32_t row_words, uint64_t seed,
                                     const uint8_t *d_iters, hipStream_t s);
hipError_t oai4g_launch_unscramble(int16_t *d_llr, const uint32_t *d_c, int n, hipStream_t s);
hipError_t oai4g_launch_chest(const chest_dev_t *d_cfg, const chest_dev_t *h_cfg, int n_sf, const int32_t *d_rxF,
                              int32_t *d_est, hipStream_t s);
/* the 5 pilot rows per subframe only ([n_sf][5][N], columns < 12 N_RB + 16) */
hipError_t oai4g_launch_chest_pilots(const chest_dev_t *d_cfg, const chest_dev_t *h_cfg, int n_sf, const int32_t *d_rxF,
                                     int32_t *d_pil, hipStream_t s);
hipError_t oai4g_launch_chest_symbol(const chest_dev_t *d_cfg, const chest_dev_t *h_cfg, const int32_t *d_rxF_sym,
                                     int32_t *d_est, int Ns, int l, int symbol, hipStream_t s);

/* what a PDSCH receive configuration demodulates: TM1, TM2 (ALAMOUTI), TM3 (LARGE_CDD) or the
 * single-layer precoding of TM4-6; all but the first use the dual extraction and nb_rx antennas */
enum rx_mode_t { RX_SISO, RX_TM2, RX_TM3, RX_TM56 };

struct rx_dev_t {
  uint32_t N, nsymb, Qm, npdcch;
  uint32_t llr_stride;            /* LLRs per batch element */
  uint32_t n_sym;                 /* PDSCH symbols per subframe (nsymb - npdcch) */
  /* per subframe index and PDSCH symbol: extraction map offset, demodulated REs, LLR offset; level
   * REs and divisor for the first symbol */
  uint32_t map_off[10][14], len[10][14], llr_off[10][14];
  uint32_t lvl_n[10], lvl_div[10];
  uint32_t gold_words;            /* scrambling words per subframe index */
  uint32_t first_sf, sf_step;
  int16_t a1, a2;                 /* QAM_n1 / QAM_n2 of the channel magnitude (0 for QPSK) */
  /* extracted RE j: FFT bin (< 2^11) | (estimate index within the symbol, < 2^11) << 16; a TM4-6
   * configuration's own copy carries the RE's precoder in bits 30-31 */
  const uint32_t *map;
  const uint32_t *gold;           /* [10][gold_words] */
  uint32_t nb_rx;                 /* receive antennas (1 for TM1) */
  int32_t mu_off;                 /* TM3: offset_mumimo_llr_drange */
  uint32_t qm1;                   /* TM3: codeword 1's modulation order (Qm = 2 picks qpsk_qpsk / _qam16 / _qam64) */
  uint32_t lvl_inc;               /* TM4-6: 1 when dl_power_off == 1 (log2_maxh++, dlsch_demodulation.c:289-292) */
  /* estimate row l from the 5 pilot rows (lte_dl_channel_estimation.c:639-698): pilot row ea[l]
   * when ewa[l] == 0, else mulhi(P[ea], ewa) << 1 +sat mulhi(P[ea + 1], ewb) << 1 */
  uint8_t ea[14];
  int16_t ewa[14], ewb[14];
};
hipError_t oai4g_launch_rx_chest(const chest_dev_t *d_ce, const rx_dev_t *d_rx, const rx_dev_t *h_rx, int n_sf,
                                 const int32_t *d_rxF, int16_t *d_llr, uint8_t *d_shift, int unscramble, hipStream_t s);
/* level + LLR kernels of one mode.  d_est: TM1's estimate grid [n_sf][nsymb][N], else the planes
 * [p * 2 + a] of `plane` words, or (pil; TM3 and TM4-6) the pilot-row pairs.  d_llr1: codeword 1 of a
 * TM3 configuration with both codewords QPSK, or null. */
hipError_t oai4g_launch_rx(rx_mode_t mode, const rx_dev_t *d_cfg, const rx_dev_t *h_cfg, int n_sf, const int32_t *d_rxF,
                           const int32_t *d_est, size_t plane, int16_t *d_llr, int16_t *d_llr1, uint8_t *d_shift,
                           int unscramble, hipStream_t s, int pil);
