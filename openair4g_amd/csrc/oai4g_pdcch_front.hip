/*
 * gfx950 kernel of the UE control channel's receive front end: rx_pdcch up to the compensated symbols
 * (PHY/LTE_TRANSPORT/dci.c:1689-1830, is_secondary_ue = 0, MU_RECEIVER off) and rx_pcfich
 * (PHY/LTE_TRANSPORT/pcfich.c:231-330) on them, always over three control symbols (dci.c:1704):
 *   pdcch_extract_rbs_single / _dual (dci.c:903, 1120) as a closed-form index map, never materialised;
 *   pdcch_channel_level (:643) over symbol 1, the avgP read of rx_pdcch (:1753-1757) -> log2_maxh;
 *   pdcch_channel_compensation (:1371) per (port, antenna), pdcch_detection_mrc (:1591),
 *   pdcch_siso (:1632, the identity) / pdcch_alamouti (:1654); rx_pcfich with pcfich_unscrambling.
 *
 * One workgroup of 256 lanes per subframe:
 *   1. the level: lane-strided over the 12 N_RB estimates of symbol 1 of every (port, antenna) plane, |h|^2
 *      summed with 32-bit wrap (the reference's four epi32 lanes and their sum, in any order), a wave
 *      reduction and one LDS atomic per wave and plane; lane 0 divides, takes the maximum over the planes
 *      rx_pdcch reads (it indexes avgP transposed) and forms log2_maxh;
 *   2. one lane per word of the 36 N_RB output words: gather y and h through the index map, conj(h) y by two
 *      16-bit dot products, >> log2_maxh, saturate; MRC in the lane; Alamouti with the neighbouring lane's
 *      port-1 value (a pair of words is a pair of lanes of one wave); plane 0 leaves as one coalesced
 *      dword store per lane.  Words 8 N_RB .. 12 N_RB - 1 of symbol 0, which the reference leaves undefined,
 *      are written as 0;
 *   3. the 16 PCFICH words were kept in LDS on their way out; 32 lanes unscramble their component and the
 *      three correlations are wave reductions.  Lane 0 stores the two per-subframe bytes.
 */
#include "oai4g_internal.h"
#include "oai4g_front_prims.h"

/* rx_pcfich's detection in one wave (pcfich.c:298-320): lane j < 32 holds word j / 2 of pcfich_d and takes its
 * component j, negated in int16 where the Gold bit is 1 (pcfich_unscrambling); codeword i has its zeros where
 * j % 3 == i (pcfich_b, :138), so metric i adds the component there and subtracts it elsewhere.  The running
 * maximum starts from -16384 and the answer from 3.  The same value in every lane. */
static __device__ __forceinline__ uint32_t pf_pcfich(uint32_t word, uint32_t gold, uint32_t lane)
{
  int32_t d = 0;
  if (lane < 32) {
    d = (lane & 1u) ? (int16_t)(word >> 16) : (int16_t)word;
    if ((gold >> lane) & 1u) d = (int16_t)(-d);
  }
  int32_t old = -16384;
  uint32_t n = 3;
#pragma unroll
  for (uint32_t i = 0; i < 3; i++) {
    int32_t m = (lane % 3u == i) ? d : -d;
    for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o);
    if (m > old) {
      n = 1u + i;
      old = m;
    }
  }
  return n;
}

__global__ void __launch_bounds__(256) k_pdcch_front(pdcch_front_args_t a)
{
  __shared__ uint32_t s_sum[4];
  __shared__ uint32_t s_shift;
  __shared__ uint32_t s_pcf[16];
  const uint32_t tid = threadIdx.x, sf = blockIdx.x;
  const uint32_t NRE = 12u * a.N_RB, half = 6u * a.N_RB, total = 3u * NRE;
  const uint32_t row1 = a.high_speed ? 1u : 0u;
  if (tid < 4) s_sum[tid] = 0;
  __syncthreads();

  /* 1. pdcch_channel_level: symbol 1 of dl_ch_estimates_ext is the estimate row at words 5 .. 5 + 12 N_RB */
#pragma unroll
  for (uint32_t pl = 0; pl < 4; pl++) {
    if ((pl >> 1) >= a.nb_tx || (pl & 1u) >= a.nb_rx) continue;
    const int32_t *__restrict__ h = a.est[pl] + (size_t)sf * a.est_sf_stride + (size_t)row1 * a.N + 5;
    uint32_t part = 0;
    for (uint32_t k = tid; k < NRE; k += 256) {
      const uint32_t v = (uint32_t)h[k];
      part += (uint32_t)pf_madd(v, v);
    }
    for (int o = 32; o > 0; o >>= 1) part += (uint32_t)__shfl_xor((int)part, o);
    if ((tid & 63u) == 0) atomicAdd(&s_sum[pl], part);
  }
  __syncthreads();
  if (tid == 0) {
    /* avg[(aatx << 1) + aarx] is written, avgP[(aarx << 1) + aatx] is read: entry r counts when it was written */
    int32_t avgs = 0;
    for (uint32_t tx = 0; tx < a.nb_tx; tx++)
      for (uint32_t rx = 0; rx < a.nb_rx; rx++) {
        const uint32_t r = (rx << 1) + tx;
        const int32_t avg = ((r >> 1) < a.nb_tx && (r & 1u) < a.nb_rx) ? (int32_t)s_sum[r] / (int32_t)NRE : 0;
        avgs = avg > avgs ? avg : avgs;
      }
    const uint32_t l2 = avgs ? 32u - (uint32_t)__clz((int)((uint32_t)avgs & 0x7FFFFFFFu)) : 0u;   /* log2_approx: bits 0..30 */
    s_shift = l2 / 2 + 6 + a.nb_rx - 1;
  }
  __syncthreads();
  const uint32_t shift = s_shift;

  /* 2. extraction, compensation, MRC and the combining, one lane per output word */
  const bool quirk = a.nb_tx > 1 && (a.N_RB & 1u);   /* pdcch_extract_rbs_dual, odd N_RB, symbols 1 / 2 (dci.c:1275) */
  const int32_t *__restrict__ rx_sf = a.rxF + (size_t)sf * a.rx_sf_stride;
  int32_t *__restrict__ out = a.comp + (size_t)sf * total;
  for (uint32_t base = 0; base < total; base += 256) {
    const uint32_t w = base + tid;
    const bool in = w < total;
    const uint32_t s = in ? w / NRE : 0u, j = in ? w - s * NRE : 0u;
    const bool defined = in && (s > 0 || j < 8u * a.N_RB);
    uint32_t k = j;
    if (s == 0) {                                       /* the 8 non-pilot REs of every RB, packed */
      const uint32_t rb = j >> 3, jj = j & 7u;
      k = 12u * rb + jj + (a.nushift3 == 0 ? (jj >> 1) + 1u : a.nushift3 == 1 ? (jj + 1u) >> 1 : jj >> 1);
    }
    uint32_t bin = k < half ? a.fco + k : 1u + k - half;
    if (quirk && s > 0 && k >= half && k < half + 6u) bin += 6u;
    uint32_t c[4] = {0, 0, 0, 0};
    if (defined) {
      const size_t hoff = (size_t)sf * a.est_sf_stride + (size_t)(a.high_speed ? s : 0u) * a.N + 5u + k;
#pragma unroll
      for (uint32_t rx = 0; rx < 2; rx++) {
        if (rx >= a.nb_rx) continue;
        const uint32_t y = (uint32_t)rx_sf[(size_t)rx * a.rx_ant_stride + (size_t)s * a.N + bin];
#pragma unroll
        for (uint32_t tx = 0; tx < 2; tx++)
          if (tx < a.nb_tx) c[(tx << 1) + rx] = pf_comp((uint32_t)a.est[(tx << 1) + rx][hoff], y, shift);
      }
    }
    if (a.planes && in) {
      int32_t *__restrict__ pl = a.planes + (size_t)sf * 4u * total + w;
#pragma unroll
      for (uint32_t p = 0; p < 4; p++) pl[(size_t)p * total] = (int32_t)c[p];
    }
    uint32_t x0 = c[0], x1 = c[2];
    if (a.nb_rx > 1) {
      x0 = pf_mrc(c[0], c[1]);
      x1 = pf_mrc(c[2], c[3]);
    }
    const uint32_t other = (uint32_t)__shfl_xor((int)x1, 1);   /* the pair's other port-1 value */
    if (a.alamouti) {                                   /* int16 sums that wrap (dci.c:1673-1677) */
      const int32_t orr = (int16_t)other, oi = (int16_t)(other >> 16);
      const int32_t re = (int16_t)x0, im = (int16_t)(x0 >> 16);
      const bool odd = (w & 1u) != 0;
      x0 = (uint32_t)(uint16_t)(odd ? re - orr : re + orr) | ((uint32_t)(uint16_t)(odd ? im + oi : im - oi) << 16);
    }
    if (in) out[w] = (int32_t)x0;
    if (in && s == 0) {
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t d = w - a.pcf_word[q];
        if (d < 4u) s_pcf[4u * q + d] = x0;
      }
    }
  }
  __syncthreads();

  /* 3. rx_pcfich on the 16 words kept in LDS */
  if (tid < 64) {
    const uint32_t sfi = (a.first_sf + sf * a.sf_step) % 10u;
    uint32_t gold = 0;
#pragma unroll
    for (uint32_t i = 0; i < 10; i++) gold = sfi == i ? a.pcf_gold[i] : gold;
    const uint32_t n = pf_pcfich(tid < 32 ? s_pcf[tid >> 1] : 0u, gold, tid);
    if (tid == 0) {
      a.cfi[sf] = (uint8_t)n;
      a.log2_maxh[sf] = (uint8_t)shift;
    }
  }
}

hipError_t oai4g_launch_pdcch_front(const pdcch_front_args_t &a, hipStream_t s)
{
  if (a.n_sf == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pdcch_front, dim3(a.n_sf), dim3(256), 0, s, a);
  return hipGetLastError();
}

/* rx_pcfich alone on a given plane 0 (the drop-in oai4g_rx_pcfich): one wave, step 3 of k_pdcch_front */
__global__ void __launch_bounds__(64) k_rx_pcfich(const int32_t *__restrict__ comp, uint32_t w0, uint32_t w1, uint32_t w2,
                                                  uint32_t w3, uint32_t gold, uint8_t *__restrict__ out)
{
  const uint32_t tid = threadIdx.x, q = (tid >> 3) & 3u;
  const uint32_t base = q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : w3;
  const uint32_t n = pf_pcfich(tid < 32 ? (uint32_t)comp[base + ((tid >> 1) & 3u)] : 0u, gold, tid);
  if (tid == 0) out[0] = (uint8_t)n;
}

hipError_t oai4g_launch_rx_pcfich(const int32_t *d_comp, const uint32_t pcf_word[4], uint32_t gold, uint8_t *d_out, hipStream_t s)
{
  hipLaunchKernelGGL(k_rx_pcfich, dim3(1), dim3(64), 0, s, d_comp, pcf_word[0], pcf_word[1], pcf_word[2], pcf_word[3], gold,
                     d_out);
  return hipGetLastError();
}
