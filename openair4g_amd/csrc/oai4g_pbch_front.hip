/*
 * gfx950 kernels of the UE's PBCH receive front end and of PHICH reception.
 *
 * k_pbch_front: rx_pbch up to the quantised soft bits (PHY/LTE_TRANSPORT/pbch.c:876-973, normal prefix):
 *   pbch_extract (:434) as a closed-form index map, never materialised; pbch_channel_level (:537) per symbol
 *   over all four ports' planes -> log2_maxh = 3 + log2_approx / 2; pbch_channel_compensation (:610) per
 *   (port, antenna); pbch_detection_mrc (:719); pbch_alamouti (:816) or nothing; pbch_quantize (:854).
 *
 *   One workgroup of 256 lanes per subframe 0, one wave per PBCH symbol (the four symbols have a level and a
 *   shift each and share nothing), lane j < 36 of a wave owns the word pair 2 j, 2 j + 1 of the symbol's
 *   72-word region:
 *     1. the lane gathers y and h of its two words through the index map: the 72 centre subcarriers (DC
 *        skipped on the receive side only), and on the two pilot symbols the 8 of every 12 that are not at
 *        nushift % 3 + {0, 3, 6, 9}, packed, which leaves words 48..71 of those regions undefined: 0 here, as
 *        the reference's cleared buffers have them;
 *     2. the level: |h|^2 of the lane's words summed with 32-bit wrap over the wave by shuffles (the
 *        reference's four epi32 lanes and their sum, in any order), per plane, no LDS and no barrier; every
 *        lane divides by 72, takes the maximum from 0 on and forms the symbol's shift;
 *     3. conj(h) y >> shift saturated, MRC, both in the lane; the Alamouti sums need the pair's two words of
 *        ports 0 and 1, which the lane holds.  The soft bits of both combining modes leave as one dword per
 *        lane and mode (four int8: re, im, re, im), plane 0 as two dwords.
 *
 * k_pbch_resolve: pbch_detection's order (initial_sync.c:135-161) over the eight decoded hypotheses of a
 *   subframe, one lane per subframe.
 *
 * k_phich_rx: rx_phich's correlation (phich.c:1312-1346), one lane per item: 12 words of plane 0 of the PDCCH
 *   front's rxdataF_comp against the 24 signs of the item's (subframe index, group, sequence), accumulated in
 *   int16 with a wrap after every term.
 */
#include "oai4g_internal.h"
#include "oai4g_front_prims.h"

/* the int16 sums of pbch_alamouti, which wrap */
static __device__ __forceinline__ uint32_t pb_pack_wrap(int32_t re, int32_t im)
{
  return (uint32_t)(uint16_t)re | ((uint32_t)(uint16_t)im << 16);
}

/* pbch_quantize of one word pair: clamp to [-8, 7], re before im */
static __device__ __forceinline__ uint32_t pb_quant(uint32_t w0, uint32_t w1)
{
  auto q = [](uint32_t h) {
    const int32_t v = (int16_t)h;
    return (uint32_t)(uint8_t)(int8_t)(v > 7 ? 7 : (v < -8 ? -8 : v));
  };
  return q(w0) | (q(w0 >> 16) << 8) | (q(w1) << 16) | (q(w1 >> 16) << 24);
}

__global__ void __launch_bounds__(256) k_pbch_front(pbch_front_args_t a)
{
  const uint32_t sf = blockIdx.x, sm = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const bool pilot = sm < 2u;
  const bool in = lane < 36u, defined = lane < (pilot ? 24u : 36u);
  const uint32_t l = 7u + sm;                                   /* the symbol's row of the subframe */
  const uint32_t erow = a.high_speed ? l : 0u;

  /* 1. the index map of the lane's two words: k = subcarrier 0..71 of the six centre RBs */
  uint32_t bin[2], hw[2];
#pragma unroll
  for (uint32_t i = 0; i < 2; i++) {
    const uint32_t w = 2u * (defined ? lane : 0u) + i;
    uint32_t k = w;
    if (pilot) {                                                /* the 8 non-pilot REs of every RB, packed */
      const uint32_t rb = w >> 3, jj = w & 7u;
      k = 12u * rb + jj + (a.nushift3 == 0 ? (jj >> 1) + 1u : a.nushift3 == 1 ? (jj + 1u) >> 1 : jj >> 1);
    }
    bin[i] = k < 36u ? a.N - 36u + k : 1u + k - 36u;
    hw[i] = 5u + 6u * a.N_RB - 36u + k;
  }

  /* 2. the level of every plane, and the estimates kept for the compensation */
  uint32_t h[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
  int32_t maxh = 0;
#pragma unroll
  for (uint32_t pl = 0; pl < 4; pl++) {
    if ((pl >> 1) >= a.nb_tx || (pl & 1u) >= a.nb_rx) continue;   /* a plane never estimated is 0 and adds nothing */
    const int32_t *__restrict__ e = a.est[pl] + (size_t)sf * a.est_sf_stride + (size_t)erow * a.N;
    uint32_t part = 0;
    if (defined) {
      h[pl][0] = (uint32_t)e[hw[0]];
      h[pl][1] = (uint32_t)e[hw[1]];
      part = (uint32_t)pf_madd(h[pl][0], h[pl][0]) + (uint32_t)pf_madd(h[pl][1], h[pl][1]);
    }
    for (int o = 32; o > 0; o >>= 1) part += (uint32_t)__shfl_xor((int)part, o);
    const int32_t avg = (int32_t)part / 72;                     /* nb_rb * 12, on the 48-word symbols too */
    maxh = avg > maxh ? avg : maxh;
  }
  const uint32_t l2 = maxh ? 32u - (uint32_t)__clz((int)((uint32_t)maxh & 0x7FFFFFFFu)) : 0u;   /* log2_approx: bits 0..30 */
  const uint32_t shift = 3u + l2 / 2u;

  /* 3. compensation, MRC, the two combinings and the quantiser */
  uint32_t c[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
  if (defined) {
    const int32_t *__restrict__ rx_row = a.rxF + (size_t)sf * a.rx_sf_stride + (size_t)l * a.N;
#pragma unroll
    for (uint32_t rx = 0; rx < 2; rx++) {
      if (rx >= a.nb_rx) continue;
      const uint32_t y0 = (uint32_t)rx_row[(size_t)rx * a.rx_ant_stride + bin[0]];
      const uint32_t y1 = (uint32_t)rx_row[(size_t)rx * a.rx_ant_stride + bin[1]];
#pragma unroll
      for (uint32_t tx = 0; tx < 2; tx++)
        if (tx < a.nb_tx) {
          c[(tx << 1) + rx][0] = pf_comp(h[(tx << 1) + rx][0], y0, shift);
          c[(tx << 1) + rx][1] = pf_comp(h[(tx << 1) + rx][1], y1, shift);
        }
    }
  }
  const uint32_t w0 = sm * 72u + 2u * lane;                     /* the pair's first word in the 288 */
  if (a.planes && in) {
    int32_t *__restrict__ pl = a.planes + (size_t)sf * 4u * OAI4G_PBCH_WORDS + w0;
#pragma unroll
    for (uint32_t p = 0; p < 4; p++) {
      pl[(size_t)p * OAI4G_PBCH_WORDS] = (int32_t)c[p][0];
      pl[(size_t)p * OAI4G_PBCH_WORDS + 1u] = (int32_t)c[p][1];
    }
  }
  uint32_t s0 = c[0][0], s1 = c[0][1], p0 = c[2][0], p1 = c[2][1];
  if (a.nb_rx > 1) {
    s0 = pf_mrc(c[0][0], c[1][0]);
    s1 = pf_mrc(c[0][1], c[1][1]);
    p0 = pf_mrc(c[2][0], c[3][0]);
    p1 = pf_mrc(c[2][1], c[3][1]);
  }
  /* rxF0[0] + rxF1[2], rxF0[1] - rxF1[3], rxF0[2] - rxF1[0], rxF0[3] + rxF1[1] (pbch.c:840-844) */
  const uint32_t a0 = pb_pack_wrap((int16_t)s0 + (int16_t)p1, (int16_t)(s0 >> 16) - (int16_t)(p1 >> 16));
  const uint32_t a1 = pb_pack_wrap((int16_t)s1 - (int16_t)p0, (int16_t)(s1 >> 16) + (int16_t)(p0 >> 16));
  if (a.comp && in) {
    int32_t *__restrict__ o = a.comp + (size_t)sf * OAI4G_PBCH_WORDS + w0;
    o[0] = (int32_t)(a.alamouti ? a0 : s0);
    o[1] = (int32_t)(a.alamouti ? a1 : s1);
  }
  if (a.llr && defined) {
    const uint32_t off = (pilot ? sm * 96u : 192u + (sm - 2u) * 144u) + 4u * lane;   /* a multiple of 4 */
    uint32_t *__restrict__ o = (uint32_t *)(a.llr + (size_t)sf * 2u * OAI4G_PBCH_SOFT + off);
    o[0] = pb_quant(s0, s1);
    o[OAI4G_PBCH_SOFT / 4u] = pb_quant(a0, a1);
  }
  if (a.log2_maxh && lane == 0) a.log2_maxh[(size_t)sf * 4u + sm] = (uint8_t)shift;
}

hipError_t oai4g_launch_pbch_front(const pbch_front_args_t &a, hipStream_t s)
{
  if (a.n_sf == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pbch_front, dim3(a.n_sf), dim3(256), 0, s, a);
  return hipGetLastError();
}

/* rec: [n_sf][8][4], hypothesis j = 2 frame_mod4 + mimo_mode, each the reversed MIB and the antenna count.  A
 * count of 4 (or none) does not end the search */
__global__ void __launch_bounds__(64) k_pbch_resolve(const uint8_t *__restrict__ rec, uint32_t n_sf,
                                                     oai4g_pbch_detect_t *__restrict__ out)
{
  const uint32_t sf = blockIdx.x * 64u + threadIdx.x;
  if (sf >= n_sf) return;
  oai4g_pbch_detect_t r = {};
  r.tx_ant = 0xFF;
  const uint32_t *__restrict__ w = (const uint32_t *)rec + (size_t)sf * 8u;
  for (uint32_t j = 0; j < 8; j++) {
    const uint32_t v = w[j], n = v >> 24;
    if (n == 1u || n == 2u) {
      r.tx_ant = (uint8_t)n;
      r.frame_mod4 = (uint8_t)(j >> 1);
      r.mimo_mode = (uint8_t)(j & 1u);
      r.mib[0] = (uint8_t)v;
      r.mib[1] = (uint8_t)(v >> 8);
      r.mib[2] = (uint8_t)(v >> 16);
      break;
    }
  }
  out[sf] = r;
}

hipError_t oai4g_launch_pbch_resolve(const uint8_t *d_rec, uint32_t n_sf, oai4g_pbch_detect_t *d_out, hipStream_t s)
{
  if (n_sf == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pbch_resolve, dim3((n_sf + 63) / 64), dim3(64), 0, s, d_rec, n_sf, d_out);
  return hipGetLastError();
}

/* An item outside the batch or the table gives {0, 0xFF} */
__global__ void __launch_bounds__(64) k_phich_rx(phich_rx_args_t a)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= a.n_items) return;
  const oai4g_phich_rx_item_t it = a.items[i];
  oai4g_phich_rx_out_t o = {};
  o.nack = 0xFF;
  if (it.slot < a.n_sf && it.ngroup < a.ngroup && it.nseq < 8u) {
    const uint32_t sfi = (a.first_sf + it.slot * a.sf_step) % 10u;
    const phich_rx_ent_t e = a.tab[((size_t)sfi * a.ngroup + it.ngroup) * 8u + it.nseq];
    const int32_t *__restrict__ comp = a.comp + (size_t)it.slot * a.comp_stride;
    int16_t hi = 0;
#pragma unroll
    for (uint32_t q = 0; q < 3; q++)
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) {
        const uint32_t v = (uint32_t)comp[(uint32_t)e.word[q] + k], b = 8u * q + 2u * k;
        const int32_t re = (int16_t)v, im = (int16_t)(v >> 16);
        hi = (int16_t)(hi + (((e.neg >> b) & 1u) ? -re : re));              /* HI16 += x * d, in int16_t */
        hi = (int16_t)(hi + (((e.neg >> (b + 1u)) & 1u) ? -im : im));
      }
    o.HI16 = hi;
    o.nack = hi > 0 ? 1 : 0;
  }
  a.out[i] = o;
}

hipError_t oai4g_launch_phich_rx(const phich_rx_args_t &a, hipStream_t s)
{
  if (a.n_items == 0) return hipSuccess;
  hipLaunchKernelGGL(k_phich_rx, dim3((a.n_items + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}
