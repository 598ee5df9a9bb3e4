/*
 * gfx950 kernels of the UE's initial cell search: the PSS time-domain correlation (k_sync_time, k_sync_peak) and,
 * behind it, initial_sync's offset arithmetic and the SSS detection (k_sss_offsets, k_sss: described where they
 * stand).  The slot_fep between them is k_fep_offset (oai4g_fep.hip).
 *
 * k_sync_time: lte_sync_time (PHY/LTE_ESTIMATION/lte_sync_time.c:357-517) of one frame per blockIdx.y.
 *   For every position n = 0, 4, ... of a half frame, every sequence s and every antenna the reference forms
 *   dot_product(replica_s, rx + n, N, 15) (PHY/TOOLS/cdot_prod.c:40-118): per tap
 *       re += (xr yr + xi yi) >> 15,   im += (xr yi + xi (int16)(-yr)) >> 15
 *   in two 32-bit sums that wrap, saturated to int16 once at the end.  The shift in front of the sum rules out
 *   an FFT or a matrix unit; the wrap allows any split of the taps.
 *
 *   One workgroup of 4 waves owns 64 positions (256 samples) of both halves.  Lane l of every wave owns
 *   position n0 + 4 l; wave w owns the taps [w N/4, (w + 1) N/4).  Per (half, antenna):
 *     1. the window rx[n0, n0 + 256 + N) is staged into LDS twice: y as it stands and y' = (yi, (int16)(-yr)),
 *        the negation in int16 so that -32768 stays -32768.  Samples behind the half's end are staged as 0;
 *        only positions that contribute 0 anyway would read them;
 *     2. a lane reads four consecutive words of y and of y' at word 4 l + k with one 16-byte LDS read each
 *        (lanes 16 bytes apart: no bank conflict), the wave reads the same four taps of the three replicas
 *        through scalar loads, and 24 v_dot2_i32_i16, shifts and adds update the lane's six partial sums;
 *     3. the four waves' partial sums meet in LDS; wave 0 adds them (32-bit wrap), saturates, and adds the
 *        antenna's result to the position's int16 sums, which wrap.
 *   Then wave 0 forms abs32 = re^2 + im^2 (32-bit wrap: (-32768, -32768) gives 2^31), the metric
 *   (abs32(first half) >> 1) + (abs32(second half) >> 1), and the key metric << 32 | ~(n + s): the largest key
 *   is the reference's first strictly greater metric in the order n ascending, s = 0, 1, 2 (n is a multiple
 *   of 4, so n + s orders both).  The wave's largest key goes to the frame's slot with one 64-bit atomic
 *   maximum, which does not depend on the order in which workgroups finish.  No floating point.
 *
 * k_sync_peak: a frame's key -> {peak_pos, peak_val, Nid2}.
 */
#include "oai4g_internal.h"
#include "oai4g_dft_prims.h"

#define SYNC_POS 64u                       /* positions per workgroup */
#define SYNC_SPAN (4u * SYNC_POS)          /* samples they cover */
#define SYNC_MAX_N 2048u

__global__ void __launch_bounds__(256) k_sync_time(sync_time_args_t a)
{
  __shared__ __attribute__((aligned(16))) uint32_t s_y[SYNC_SPAN + SYNC_MAX_N], s_yn[SYNC_SPAN + SYNC_MAX_N];
  __shared__ int32_t s_part[4][6][64];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
  const uint32_t N = a.N, length = a.length, f = blockIdx.y;
  const uint32_t n0 = blockIdx.x * SYNC_SPAN, n = n0 + 4u * lane;
  const uint32_t win = SYNC_SPAN + N;
  const uint32_t *rx_f = a.rx + (size_t)f * a.nb_rx * 2u * length;
  const uint32_t q0 = w * (N >> 4), q1 = q0 + (N >> 4);
  const uint32_t *__restrict__ rep = a.rep;

  uint32_t sum[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};   /* per half and sequence: the antennas' int16 pair, wrapping */
  for (uint32_t h = 0; h < 2u; h++)
    for (uint32_t ar = 0; ar < a.nb_rx; ar++) {
      const uint32_t *src = rx_f + (size_t)ar * 2u * length + h * length;
      __syncthreads();                                  /* the previous pass has read its window */
      for (uint32_t i = t; i < win; i += 256u) {
        const uint32_t y = n0 + i < length ? src[n0 + i] : 0u;
        s_y[i] = y;
        s_yn[i] = c2u(cflip(u2c(y)));
      }
      __syncthreads();
      int32_t acc[3][2] = {{0, 0}, {0, 0}, {0, 0}};
      for (uint32_t q = q0; q < q1; q++) {                           /* taps 4 q .. 4 q + 3 */
        const u32x4_t y4 = *(const u32x4_t *)&s_y[4u * (lane + q)];
        const u32x4_t yn4 = *(const u32x4_t *)&s_yn[4u * (lane + q)];
#pragma unroll
        for (uint32_t s = 0; s < 3u; s++) {
          const u32x4_t x4 = *(const u32x4_t *)&rep[s * N + 4u * q];   /* wave-uniform address: a scalar load */
#pragma unroll
          for (uint32_t j = 0; j < 4u; j++) {
            acc[s][0] = wadd(acc[s][0], dot2s(u2c(y4[j]), u2c(x4[j])) >> 15);
            acc[s][1] = wadd(acc[s][1], dot2s(u2c(yn4[j]), u2c(x4[j])) >> 15);
          }
        }
      }
#pragma unroll
      for (uint32_t s = 0; s < 3u; s++) {
        s_part[w][2u * s][lane] = acc[s][0];
        s_part[w][2u * s + 1u][lane] = acc[s][1];
      }
      __syncthreads();
      if (w == 0u) {
#pragma unroll
        for (uint32_t s = 0; s < 3u; s++) {
          int32_t re = 0, im = 0;
#pragma unroll
          for (uint32_t q = 0; q < 4u; q++) {
            re = wadd(re, s_part[q][2u * s][lane]);
            im = wadd(im, s_part[q][2u * s + 1u][lane]);
          }
          sum[h][s] = c2u(caddw(u2c(sum[h][s]), __builtin_bit_cast(s16x2, __builtin_amdgcn_cvt_pk_i16(re, im))));
        }
      }
    }
  if (w != 0u) return;

  unsigned long long key = 0ull;
  const bool inside = n < length, counted = n + N < length;   /* lte_sync_time.c:420 */
#pragma unroll
  for (uint32_t s = 0; s < 3u; s++) {
    uint32_t ab[2];
#pragma unroll
    for (uint32_t h = 0; h < 2u; h++) {
      const int32_t re = (int16_t)sum[h][s], im = (int16_t)(sum[h][s] >> 16);
      ab[h] = counted ? (uint32_t)re * (uint32_t)re + (uint32_t)im * (uint32_t)im : 0u;
      if (a.corr && inside) a.corr[((size_t)f * 3u + s) * 2u * length + h * length + n] = (int32_t)ab[h];
    }
    const uint32_t metric = (uint32_t)(((int32_t)ab[0] >> 1) + ((int32_t)ab[1] >> 1));
    const unsigned long long ks = ((unsigned long long)metric << 32) | (0xFFFFFFFFu - (n + s));
    if (inside && ks > key) key = ks;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const unsigned long long other = __shfl_xor(key, 32 >> i, 64);
    if (other > key) key = other;
  }
  if (lane == 0u) atomicMax(&a.keys[f], key);
}

__global__ void k_sync_peak(const unsigned long long *keys, uint32_t n, int32_t *peak)
{
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n) return;
  const unsigned long long key = keys[f];
  const uint32_t idx = 0xFFFFFFFFu - (uint32_t)key;
  peak[3u * f] = (int32_t)(idx & ~3u);
  peak[3u * f + 1u] = (int32_t)(uint32_t)(key >> 32);
  peak[3u * f + 2u] = (int32_t)(idx & 3u);
}

/* initial_sync's offset arithmetic (initial_sync.c:310-354, FDD, normal prefix), one lane per frame */
__global__ void k_sss_offsets(sss_args_t a)
{
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.n) return;
  const int32_t frame = 10 * (int32_t)a.spt, cp = (int32_t)a.cp, sync_pos = a.peak[3u * f];
  const int32_t sync_pos2 = sync_pos >= cp ? sync_pos - cp : sync_pos + frame - cp;
  const int32_t sync_pos_slot = (int32_t)(a.spt >> 1) - (int32_t)a.N - cp, d = sync_pos2 - sync_pos_slot;
  int32_t *c = a.cell + OAI4G_CELL_WORDS * f;
  c[0] = -1;
  c[1] = d >= 0 ? d : frame + d;
  c[2] = c[3] = c[4] = 0;
  c[5] = (d >= 0 && d < frame - (int32_t)(a.spt >> 1)) ? 0 : OAI4G_SSS_ERROR;
}

/* rx_sss behind its four slot_fep calls (sss.c:284-390), one workgroup per frame:
 *   1. lanes i < 62, for the symbols of slot 0 and of slot 10: pss_sss_extract's word i + 5 of the 72 (bins
 *      N - 36 .. N - 1, then 1 .. 36) of the PSS and SSS rows, pss_ch_est (:129-149) with every >> 15 and int16
 *      cast where the reference has them, antenna 0 written, antenna 1 added in int16;
 *   2. A0 / A5 [phase][i] = ((phase_re re) >> 19) - ((phase_im im) >> 19) (:371-372), which depend on nothing else;
 *   3. the 2 x 7 x 168 hypotheses over the lanes: 62 terms (int16)(d0[i] A0 + d5[i] A5), d as sign bits, flip 1
 *      swapping the two tables; the first strictly greater metric in the order flip, phase, Nid1 is the largest
 *      key (metric, ~hypothesis). */
__global__ void __launch_bounds__(256) k_sss(sss_args_t a)
{
  __shared__ int32_t s_A[2][7][62];
  __shared__ uint32_t s_sss[2][62];
  __shared__ unsigned long long s_key[4];
  const uint32_t f = blockIdx.x, t = threadIdx.x, N = a.N;
  int32_t *cell = a.cell + OAI4G_CELL_WORDS * f;
  if (cell[5] != 0) return;                              /* no SSS detection for this frame: the record stands */
  const uint32_t nid2 = (uint32_t)a.peak[3u * f + 2u] % 3u;
  if (t < 124u) {
    const uint32_t half = t / 62u, i = t - half * 62u, j = i + 5u;
    const uint32_t bin = j < 36u ? N - 36u + j : j - 35u;
    const uint32_t p = a.pss[nid2 * 62u + i];
    const int32_t pr = (int16_t)p, pi = (int16_t)(p >> 16);
    int32_t sr = 0, si = 0;
    for (uint32_t ar = 0; ar < a.nb_rx; ar++) {
      const int32_t *rows = a.rxF + (((size_t)f * a.nb_rx + ar) * 4u + 2u * half) * N;
      const uint32_t ws = (uint32_t)rows[bin], wp = (uint32_t)rows[N + bin];
      const int32_t er = (int16_t)wp, ei = (int16_t)(wp >> 16), yr = (int16_t)ws, yi = (int16_t)(ws >> 16);
      const int32_t tr = (int16_t)(((er * pr) >> 15) + ((ei * pi) >> 15));
      const int32_t ti = (int16_t)(((er * pi) >> 15) - ((ei * pr) >> 15));
      const int32_t r2 = (int16_t)(((tr * yr) >> 15) - ((ti * yi) >> 15));
      const int32_t i2 = (int16_t)(((tr * yi) >> 15) + ((ti * yr) >> 15));
      sr = (int16_t)(sr + r2);
      si = (int16_t)(si + i2);
    }
    s_sss[half][i] = (uint32_t)(uint16_t)sr | ((uint32_t)(uint16_t)si << 16);
  }
  __syncthreads();
  for (uint32_t e = t; e < 2u * 7u * 62u; e += 256u) {
    const uint32_t half = e / 434u, ph = (e - half * 434u) / 62u, i = e - half * 434u - ph * 62u;
    const uint32_t w = s_sss[half][i];
    s_A[half][ph][i] = (((int32_t)a.phase_re[ph] * (int16_t)w) >> 19) - (((int32_t)a.phase_im[ph] * (int16_t)(w >> 16)) >> 19);
  }
  __syncthreads();
  unsigned long long key = 0ull;
  for (uint32_t h = t; h < 2u * 7u * 168u; h += 256u) {
    const uint32_t flip = h / 1176u, ph = (h - flip * 1176u) / 168u, nid1 = h - flip * 1176u - ph * 168u;
    const unsigned long long *d = a.d + 2u * (nid2 + 3u * nid1);
    const unsigned long long b0 = d[flip], b5 = d[flip ^ 1u];
    int32_t metric = 0;
    for (uint32_t i = 0; i < 62u; i++) {
      const int32_t a0 = s_A[0][ph][i], a5 = s_A[1][ph][i];
      metric += (int16_t)(((b0 >> i) & 1ull ? -a0 : a0) + ((b5 >> i) & 1ull ? -a5 : a5));
    }
    const unsigned long long k = ((unsigned long long)((uint32_t)metric ^ 0x80000000u) << 32) | (0xFFFFFFFFu - h);
    if (k > key) key = k;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const unsigned long long other = __shfl_xor(key, 32 >> i, 64);
    if (other > key) key = other;
  }
  if ((t & 63u) == 0u) s_key[t >> 6] = key;
  __syncthreads();
  if (t == 0u) {
    for (uint32_t q = 1; q < 4u; q++)
      if (s_key[q] > key) key = s_key[q];
    const uint32_t h = 0xFFFFFFFFu - (uint32_t)key, flip = h / 1176u, ph = (h - flip * 1176u) / 168u;
    const int32_t metric = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
    if (metric > -99999999) {                           /* :350, :376 (always: |metric| <= 62 * 32768) */
      cell[0] = (int32_t)(nid2 + 3u * (h - flip * 1176u - ph * 168u));
      if (a.add_half && flip) cell[1] += 5 * (int32_t)a.spt;
      cell[2] = metric;
      cell[3] = (int32_t)flip;
      cell[4] = (int32_t)ph;
    }
  }
}

hipError_t oai4g_launch_sss_offsets(const sss_args_t &a, hipStream_t s)
{
  if (a.n == 0u) return hipSuccess;
  hipLaunchKernelGGL(k_sss_offsets, dim3((a.n + 63u) / 64u), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t oai4g_launch_sss(const sss_args_t &a, hipStream_t s)
{
  if (a.n == 0u) return hipSuccess;
  if (a.nb_rx < 1u || a.nb_rx > 2u || a.N < 128u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sss, dim3(a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t oai4g_launch_sync_time(const sync_time_args_t &a, hipStream_t s)
{
  if (a.n == 0u) return hipSuccess;
  if (a.N > SYNC_MAX_N || a.N < 128u || (a.N & 15u) || (a.length & 3u) || a.nb_rx < 1u || a.nb_rx > 2u) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.keys, 0, (size_t)a.n * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  const dim3 grid((a.length + SYNC_SPAN - 1u) / SYNC_SPAN, a.n);
  hipLaunchKernelGGL(k_sync_time, grid, dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_sync_peak, dim3((a.n + 63u) / 64u), dim3(64), 0, s, a.keys, a.n, a.peak);
  return hipGetLastError();
}
