/*
 * SC-FDMA transform precoding: the mixed-radix "PUSCH DFTs" of PHY/TOOLS/lte_dfts.c (:3510-16087, sizes 12 N_RB with
 * N_RB = 2^a 3^b 5^c, 33 of them), bit-exact, and the three kernels on it:
 *   k_pusch_dft   dft_lte's contract on [n][Msc] arrays (ulsch_modulation.c:53-373)
 *   k_pusch_mod   ulsch_modulation (ulsch_modulation.c:376-783): scrambling with the PUSCH_x / PUSCH_y placeholders,
 *                 QAM, transform precoding and RE mapping in one launch; b_tilde, d and z never reach memory
 *   k_pusch_idft  lte_idft (ulsch_demodulation.c:58-465) in place on compensated grids
 *
 * One transform.  dftN is decimation in time over one factor r per level: r sub-transforms of N / r on x[j], x[j + r],
 * ..., then bfly<r>_tw1 at k = 0 and bfly<r> with twiddles at k >= 1, down to dft12f.  Unrolled, the recursion is
 *   leaf     N / 12 twelve-point transforms; the one whose level digits are (j1 .. jL) reads x[o + (N / 12) m], m < 12,
 *            o = j1 + r1 j2 + r1 r2 j3 ..., and writes block j1 M1 + j2 M2 + ... (Ml the sub-size at level l): where
 *            the reference's ytmp arrays hold it
 *   level l  (innermost first) in every block of M(l-1) words, butterfly k reads and writes words j Ml + k, j < rl:
 *            in place
 * and the outermost level leaves y in natural order.  A symbol lives in LDS from its load to its store: region A holds
 * the input in natural order, region B the blocks.  Nothing goes to HBM or scratch in between.
 *
 * Lane map.  A symbol has tps = 256 / spw threads (spw symbols per workgroup, from the host: more for the small sizes).
 * In the leaf a thread owns one twelve-point transform, consecutive threads consecutive offsets o (region A is read at
 * stride 1 across lanes); in a level a thread owns one butterfly, consecutive threads consecutive k (stride 1 again).
 * The leaf's twelve stores go to blocks 12 words apart, which by themselves would meet 8 of the 32 write banks (4-way);
 * region B is therefore padded by one word per twelve (bphys), stride 13.
 * The k = 0 butterflies of a level round differently (the _tw1 forms) and run as a loop of their own, so that no wave
 * executes both forms for the same element.
 */
#include <hip/hip_runtime.h>

#include "oai4g_dft_prims.h"

#define PUSCH_THREADS 256u

/* cmult (lte_dfts.c:109-121): x * t with t stored as a = (t.re, -t.im), b = (t.im, t.re): one dot2 per component */
struct ptw_t {
  s16x2 a, b;
};
#define PTW(re, im) ptw_t{s16x2{(short)(re), (short)(-(im))}, s16x2{(short)(im), (short)(re)}}

static __device__ __forceinline__ void pmul32(s16x2 x, const ptw_t &t, int &re, int &im)
{
  re = dot2(x, t.a);
  im = dot2(x, t.b);
}
static __device__ __forceinline__ s16x2 pmul16(s16x2 x, const ptw_t &t)      /* packed_cmult */
{
  return cpack32(dot2(x, t.a), dot2(x, t.b));
}
/* mulhi_int16(a, c) = slli(mulhi_epi16(a, c), 1): the low bit always clear */
static __device__ __forceinline__ s16x2 pnorm(s16x2 a, int c)
{
  return s16x2{(short)((((int)a.x * c) >> 16) << 1), (short)((((int)a.y * c) >> 16) << 1)};
}
static __device__ __forceinline__ uint32_t bphys(uint32_t pos) { return pos + __umulhi(pos, 0x15555556u); }   /* pos + pos / 12 */

/* bfly2 (:396-418): x0 goes through the same madd by W0 = 32767; 32-bit sums >> 15, then packs */
static __device__ __forceinline__ void pb2(s16x2 x0, s16x2 x1, const ptw_t &t, s16x2 &y0, s16x2 &y1)
{
  const int a0r = dot2(x0, s16x2{32767, 0}), a0i = dot2(x0, s16x2{0, 32767});
  int a1r, a1i;
  pmul32(x1, t, a1r, a1i);
  y0 = cpack32(wadd(a0r, a1r), wadd(a0i, a1i));
  y1 = cpack32(wsub(a0r, a1r), wsub(a0i, a1i));
}
static __device__ __forceinline__ void pb2_tw1(s16x2 x0, s16x2 x1, s16x2 &y0, s16x2 &y1)
{
  y0 = cadds(x0, x1);
  y1 = csubs(x0, x1);
}
/* bfly3_tw1 (:664-679); bfly3 (:560-578) is the same behind two packed_cmult */
static __device__ __forceinline__ void pb3_tw1(s16x2 x0, s16x2 x1, s16x2 x2, s16x2 &y0, s16x2 &y1, s16x2 &y2)
{
  const ptw_t W13 = PTW(-16384, -28378), W23 = PTW(-16384, 28378);
  int ar, ai, br, bi;
  y0 = cadds(x0, cadds(x1, x2));
  pmul32(x1, W13, ar, ai);
  pmul32(x2, W23, br, bi);
  y1 = cadds(x0, cpack32(wadd(ar, br), wadd(ai, bi)));
  pmul32(x1, W23, ar, ai);
  pmul32(x2, W13, br, bi);
  y2 = cadds(x0, cpack32(wadd(ar, br), wadd(ai, bi)));
}
static __device__ __forceinline__ void pb3(s16x2 x0, s16x2 x1, s16x2 x2, const ptw_t &t1, const ptw_t &t2, s16x2 &y0,
                                           s16x2 &y1, s16x2 &y2)
{
  pb3_tw1(x0, pmul16(x1, t1), pmul16(x2, t2), y0, y1, y2);
}
/* bfly4_tw1 (:860-889): saturating throughout, -j x by a wrapping negate */
static __device__ __forceinline__ void pb4_tw1(s16x2 x0, s16x2 x1, s16x2 x2, s16x2 x3, s16x2 &y0, s16x2 &y1, s16x2 &y2,
                                               s16x2 &y3)
{
  const s16x2 s02 = cadds(x0, x2), s13 = cadds(x1, x3), d02 = csubs(x0, x2), d13 = csubs(cflip(x1), cflip(x3));
  y0 = cadds(s02, s13);
  y2 = csubs(s02, s13);
  y1 = cadds(d02, d13);
  y3 = csubs(d02, d13);
}
/* bfly4 (:709-744): 32-bit products, one cpack per output, x0 added with a wrapping _mm_add_epi16 */
static __device__ __forceinline__ void pb4(s16x2 x0, s16x2 x1, s16x2 x2, s16x2 x3, const ptw_t &t1, const ptw_t &t2,
                                           const ptw_t &t3, s16x2 &y0, s16x2 &y1, s16x2 &y2, s16x2 &y3)
{
  int a1r, a1i, a2r, a2i, a3r, a3i;
  pmul32(x1, t1, a1r, a1i);
  pmul32(x2, t2, a2r, a2i);
  pmul32(x3, t3, a3r, a3i);
  y0 = caddw(x0, cpack32(wadd(a1r, wadd(a2r, a3r)), wadd(a1i, wadd(a2i, a3i))));
  y1 = caddw(x0, cpack32(wsub(a1i, wadd(a2r, a3i)), wsub(wsub(a3r, a2i), a1r)));
  y2 = caddw(x0, cpack32(wsub(wsub(a2r, a3r), a1r), wsub(wsub(a2i, a3i), a1i)));
  y3 = caddw(x0, cpack32(wsub(wsub(a3i, a2r), a1i), wsub(a1r, wadd(a2i, a3r))));
}
/* bfly5_tw1 (:1235-1266); bfly5 (:1130-1174) is the same behind four packed_cmult */
static __device__ __forceinline__ void pb5_tw1(s16x2 x0, s16x2 x1, s16x2 x2, s16x2 x3, s16x2 x4, s16x2 &y0, s16x2 &y1,
                                               s16x2 &y2, s16x2 &y3, s16x2 &y4)
{
  const ptw_t W[4] = {PTW(10126, -31163), PTW(-26509, -19260), PTW(-26510, 19260), PTW(10126, 31163)};   /* W15 .. W45 */
  const s16x2 x[4] = {x1, x2, x3, x4};
  s16x2 *const y[4] = {&y1, &y2, &y3, &y4};
  y0 = cadds(x0, cadds(x1, cadds(x2, cadds(x3, x4))));
#pragma unroll
  for (int m = 1; m <= 4; m++) {          /* output m: x_j by W^(m j mod 5) */
    int re = 0, im = 0;
#pragma unroll
    for (int j = 1; j <= 4; j++) {
      int r, i;
      pmul32(x[j - 1], W[(m * j) % 5 - 1], r, i);
      re = wadd(re, r);
      im = wadd(im, i);
    }
    *y[m - 1] = cadds(x0, cpack32(re, im));
  }
}
static __device__ __forceinline__ void pb5(s16x2 x0, s16x2 x1, s16x2 x2, s16x2 x3, s16x2 x4, const ptw_t *t, s16x2 &y0,
                                           s16x2 &y1, s16x2 &y2, s16x2 &y3, s16x2 &y4)
{
  pb5_tw1(x0, pmul16(x1, t[0]), pmul16(x2, t[1]), pmul16(x3, t[2]), pmul16(x4, t[3]), y0, y1, y2, y3, y4);
}

/* dft12f (:3553-3657) in registers: three bfly4_tw1, then bfly3_tw1 and three bfly3 by the W*_12 constants */
static __device__ __forceinline__ void dft12f(const s16x2 *x, s16x2 *y)
{
  s16x2 t[12];
#pragma unroll
  for (int j = 0; j < 3; j++) pb4_tw1(x[j], x[3 + j], x[6 + j], x[9 + j], t[j], t[3 + j], t[6 + j], t[9 + j]);
  pb3_tw1(t[0], t[1], t[2], y[0], y[4], y[8]);
  pb3(t[3], t[4], t[5], PTW(28377, -16383), PTW(16383, -28377), y[1], y[5], y[9]);
  pb3(t[6], t[7], t[8], PTW(16383, -28377), PTW(-16383, -28377), y[2], y[6], y[10]);
  pb3(t[9], t[10], t[11], PTW(0, -32767), PTW(-32767, 0), y[3], y[7], y[11]);
}

static __device__ __forceinline__ ptw_t ldtw(const uint2 *tw, uint32_t i)
{
  const uint2 v = tw[i];
  return ptw_t{u2c(v.x), u2c(v.y)};
}

/* one level of one symbol: every block of R M words, butterflies k = 1 .. M - 1 with the level's twiddles
 * tw[q (M - 1) + k - 1] (q = 0 .. R - 2), then the k = 0 butterflies in their _tw1 form; norm != 0: mulhi_int16 on the
 * way out */
template <int R>
static __device__ __forceinline__ void level(uint32_t *B, uint32_t N, uint32_t M, uint32_t rcpM1, const uint2 *tw, int norm,
                                             uint32_t tid, uint32_t tps)
{
  const uint32_t blocks = N / (R * M), per = M - 1;
  for (uint32_t b = tid; b < blocks * M; b += tps) {
    uint32_t g, k;
    if (b < blocks * per) {
      g = __umulhi(b, rcpM1);             /* b / (M - 1) */
      k = b - g * per + 1;
    } else {
      g = b - blocks * per;
      k = 0;
    }
    const uint32_t base = g * R * M + k;
    s16x2 x[R], y[R];
#pragma unroll
    for (int j = 0; j < R; j++) x[j] = u2c(B[bphys(base + j * M)]);
    if (k != 0) {
      ptw_t t[R - 1];
#pragma unroll
      for (int q = 0; q < R - 1; q++) t[q] = ldtw(tw, q * per + k - 1);
      if constexpr (R == 2) pb2(x[0], x[1], t[0], y[0], y[1]);
      if constexpr (R == 3) pb3(x[0], x[1], x[2], t[0], t[1], y[0], y[1], y[2]);
      if constexpr (R == 4) pb4(x[0], x[1], x[2], x[3], t[0], t[1], t[2], y[0], y[1], y[2], y[3]);
      if constexpr (R == 5) pb5(x[0], x[1], x[2], x[3], x[4], t, y[0], y[1], y[2], y[3], y[4]);
    } else {
      if constexpr (R == 2) pb2_tw1(x[0], x[1], y[0], y[1]);
      if constexpr (R == 3) pb3_tw1(x[0], x[1], x[2], y[0], y[1], y[2]);
      if constexpr (R == 4) pb4_tw1(x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]);
      if constexpr (R == 5) pb5_tw1(x[0], x[1], x[2], x[3], x[4], y[0], y[1], y[2], y[3], y[4]);
    }
#pragma unroll
    for (int j = 0; j < R; j++) B[bphys(base + j * M)] = c2u(norm ? pnorm(y[j], norm) : y[j]);
  }
}

/* The transform of the workgroup's symbols: region A (natural order, N words per symbol) -> region B (bphys).  Every
 * thread of the workgroup calls it (the barriers); tid / tps are the thread's place within its symbol, live = false for
 * the threads of a symbol past the batch's end.  Ends with a barrier: B is complete. */
static __device__ __forceinline__ void pusch_transform(const pusch_plan_t &p, const uint2 *tw, const uint32_t *A, uint32_t *B,
                                                       uint32_t tid, uint32_t tps, bool live)
{
  __syncthreads();                        /* A is complete */
  if (live) {
    const uint32_t P = p.N / 12;
    for (uint32_t s = tid; s < P; s += tps) {
      uint32_t o = s, base = 0;
      for (uint32_t l = 0; l < p.n_lvl; l++) {
        const uint32_t q = __umulhi(o, p.rcp_r[l]);      /* o / radix[l] */
        base += (o - q * p.radix[l]) * p.M[l];
        o = q;
      }
      s16x2 x[12], y[12];
#pragma unroll
      for (int m = 0; m < 12; m++) x[m] = u2c(A[s + P * m]);
      dft12f(x, y);
#pragma unroll
      for (int m = 0; m < 12; m++) B[bphys(base + m)] = c2u(p.leaf_norm ? pnorm(y[m], (int)p.leaf_norm) : y[m]);
    }
  }
  for (int l = (int)p.n_lvl - 1; l >= 0; l--) {
    __syncthreads();
    if (!live) continue;
    const uint2 *t = tw + p.tw_off[l];
    switch (p.radix[l]) {                                /* uniform over the launch: one radix's code per level */
    case 2: level<2>(B, p.N, p.M[l], p.rcp_m1[l], t, (int)p.norm[l], tid, tps); break;
    case 3: level<3>(B, p.N, p.M[l], p.rcp_m1[l], t, (int)p.norm[l], tid, tps); break;
    case 4: level<4>(B, p.N, p.M[l], p.rcp_m1[l], t, (int)p.norm[l], tid, tps); break;
    default: level<5>(B, p.N, p.M[l], p.rcp_m1[l], t, (int)p.norm[l], tid, tps); break;
    }
  }
  __syncthreads();
}

/* _mm_sign_epi16 by {1, -1}: an imaginary part of -32768 stays -32768 */
static __device__ __forceinline__ uint32_t pconj(uint32_t v)
{
  const s16x2 c = u2c(v);
  return c2u(s16x2{c.x, (short)(-(int)c.y)});
}

extern "C" __global__ void __launch_bounds__(PUSCH_THREADS) k_pusch_dft(pusch_plan_t p, const uint2 *tw, const uint32_t *in,
                                                                        uint32_t *out, uint32_t n_sym)
{
  extern __shared__ uint32_t lds[];
  const uint32_t tps = PUSCH_THREADS / p.spw, ls = threadIdx.x / tps, tid = threadIdx.x - ls * tps;
  const uint32_t sym = blockIdx.x * p.spw + ls;
  const bool live = sym < n_sym;
  uint32_t *A = lds + ls * p.lds_sym, *B = A + p.N;
  if (live)
    for (uint32_t i = tid; i < p.N; i += tps) A[i] = in[(size_t)sym * p.N + i];
  pusch_transform(p, tw, A, B, tid, tps, live);
  if (live)
    for (uint32_t i = tid; i < p.N; i += tps) out[(size_t)sym * p.N + i] = B[bphys(i)];
}

extern "C" __global__ void __launch_bounds__(PUSCH_THREADS) k_pusch_idft(pusch_plan_t p, const uint2 *tw, pusch_grid_t g,
                                                                         uint32_t *comp, uint32_t n_sym)
{
  extern __shared__ uint32_t lds[];
  const uint32_t tps = PUSCH_THREADS / p.spw, ls = threadIdx.x / tps, tid = threadIdx.x - ls * tps;
  const uint32_t sym = blockIdx.x * p.spw + ls;
  const bool live = sym < n_sym;
  const uint32_t sf = sym / g.n_data, l = g.sym[sym - sf * g.n_data];
  uint32_t *row = comp + ((size_t)sf * g.nsymb + l) * g.row;
  uint32_t *A = lds + ls * p.lds_sym, *B = A + p.N;
  if (live)
    for (uint32_t i = tid; i < p.N; i += tps) A[i] = pconj(row[i]);
  pusch_transform(p, tw, A, B, tid, tps, live);
  if (live)
    for (uint32_t i = tid; i < p.N; i += tps) row[i] = pconj(B[bphys(i)]);
}

/* b_tilde[k] (ulsch_modulation.c:452-470): PUSCH_x -> 1; PUSCH_y -> the scrambled bit before it (through a run of
 * PUSCH_y, and 1 behind a PUSCH_x); else h + c */
static __device__ __forceinline__ uint32_t pusch_bit(const uint8_t *h, const uint32_t *gold, uint32_t k)
{
  while (k > 0 && h[k] == 3) k--;
  const uint32_t v = h[k];
  if (v == 2) return 1u;
  if (v == 3) return 0u;                  /* a PUSCH_y at bit 0: the reference reads b_tilde[-1] */
  return (v + ((gold[k >> 5] >> (k & 31)) & 1u)) & 1u;
}

extern "C" __global__ void __launch_bounds__(PUSCH_THREADS) k_pusch_mod(pusch_plan_t p, const uint2 *tw, pusch_grid_t g,
                                                                        pusch_mod_t m, const uint8_t *h, const uint32_t *gold,
                                                                        uint32_t *txF, uint32_t n_sym)
{
  extern __shared__ uint32_t lds[];
  const uint32_t tps = PUSCH_THREADS / p.spw, ls = threadIdx.x / tps, tid = threadIdx.x - ls * tps;
  const uint32_t sym = blockIdx.x * p.spw + ls;
  const bool live = sym < n_sym;
  const uint32_t sf = sym / g.n_data, j = sym - sf * g.n_data, l = g.sym[j];
  uint32_t *A = lds + ls * p.lds_sym, *B = A + p.N;
  if (live) {
    const uint8_t *hs = h + (size_t)sf * m.h_stride;
    const uint32_t *gs = gold + ((m.first_sf + sf * m.sf_step) % 10u) * m.gold_words;
    /* qam16_table / qam64_table's magnitudes by offset (2 b0 + b2; 4 b0 + 2 b2 + b4: the top bit is the sign) */
    const int lv16[2] = {10362, 31086}, lv64[4] = {15169, 5057, 25281, 35393};
    for (uint32_t i = tid; i < p.N; i += tps) {
      const uint32_t k = (j * p.N + i) * m.Qm;
      int c[2];
#pragma unroll
      for (uint32_t q = 0; q < 2; q++) {
        const uint32_t b0 = pusch_bit(hs, gs, k + q);
        if (m.Qm == 2) {
          c[q] = b0 ? -m.gain_qpsk : m.gain_qpsk;
        } else {
          /* (int16_t)((amp * table[offset]) >> 15): the table's second half is the negated first, and the shift floors */
          const int t = m.Qm == 4 ? lv16[pusch_bit(hs, gs, k + 2 + q)]
                                  : lv64[2 * pusch_bit(hs, gs, k + 2 + q) + pusch_bit(hs, gs, k + 4 + q)];
          c[q] = (m.amp * (b0 ? -t : t)) >> 15;
        }
      }
      A[i] = c2u(s16x2{(short)c[0], (short)c[1]});
    }
  }
  pusch_transform(p, tw, A, B, tid, tps, live);
  if (live) {
    uint32_t *row = txF + ((size_t)sf * g.nsymb + l) * g.row;
    for (uint32_t i = tid; i < p.N; i += tps) {
      uint32_t re = m.re_offset + i;
      if (re >= g.row) re -= g.row;
      row[re] = B[bphys(i)];
    }
  }
}

static size_t pusch_lds(const pusch_plan_t &p) { return (size_t)p.spw * p.lds_sym * 4; }

hipError_t oai4g_launch_pusch_dft(const pusch_plan_t &p, const uint2 *d_tw, const uint32_t *d_in, uint32_t *d_out, uint32_t n_sym,
                                  hipStream_t s)
{
  if (n_sym == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pusch_dft, dim3((n_sym + p.spw - 1) / p.spw), dim3(PUSCH_THREADS), pusch_lds(p), s, p, d_tw, d_in, d_out, n_sym);
  return hipGetLastError();
}

hipError_t oai4g_launch_pusch_idft(const pusch_plan_t &p, const uint2 *d_tw, const pusch_grid_t &g, uint32_t *d_comp, uint32_t n_sf,
                                   hipStream_t s)
{
  const uint32_t n_sym = n_sf * g.n_data;
  if (n_sym == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pusch_idft, dim3((n_sym + p.spw - 1) / p.spw), dim3(PUSCH_THREADS), pusch_lds(p), s, p, d_tw, g, d_comp, n_sym);
  return hipGetLastError();
}

hipError_t oai4g_launch_pusch_mod(const pusch_plan_t &p, const uint2 *d_tw, const pusch_grid_t &g, const pusch_mod_t &m,
                                  const uint8_t *d_h, const uint32_t *d_gold, uint32_t *d_txF, uint32_t n_sf, hipStream_t s)
{
  const uint32_t n_sym = n_sf * g.n_data;
  if (n_sym == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pusch_mod, dim3((n_sym + p.spw - 1) / p.spw), dim3(PUSCH_THREADS), pusch_lds(p), s, p, d_tw, g, m, d_h, d_gold,
                     d_txF, n_sym);
  return hipGetLastError();
}
