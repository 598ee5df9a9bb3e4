/*
 * gfx950 kernels of dlsim's AWGN channel stage (openair1/SIMULATION/LTE_PHY/dlsim.c:2714-2866), the
 * link between the transmit batch and the UE receive batch in a BLER run:
 *   signal_energy   PHY/TOOLS/signal_energy.c:66-110: mean of (re^2 + im^2) >> 4 over the vector,
 *                   minus the squared DC (16-bit lane sums), with the SSE code's wraps and its
 *                   int / uint32_t divisions — dlsim's tx_lev per transmit antenna (:2714-2719)
 *   AWGN            dlsim.c:2852-2866: sigma2_dB = 10 log10(tx_lev) + 10 log10(N / (12 NB_RB)) - SNR
 *                   - pa_dB; r = (short)(s + sqrt(sigma2 / 2) g) per I / Q component, g ~ N(0, 1)
 *                   (the reference draws g from gaussdouble, SIMULATION/TOOLS/rangen_double.c:97, a
 *                   polar Box-Muller over a shuffled 32-bit LCG; here a counter-based Philox-4x32
 *                   stream with the Box-Muller transform in double precision, so a run is
 *                   reproducible from (seed, vector, sample) whatever the launch shape)
 * Both are HBM-streaming (one read + one write of the int16 IQ per sample), one workgroup per
 * vector chunk, coalesced 4-byte lanes.
 * Behind them the fading channels that take the unit tap's place (k_channel_taps, k_multipath; their
 * own header below), and the HARQ round state of the BLER loop.
 */
#include "oai4g_internal.h"

namespace {

constexpr uint32_t SE_WG = 256;
constexpr uint32_t AW_WG = 256;
constexpr uint32_t AW_PER = 4;          /* samples per thread: 1024 per workgroup */

/* Philox-4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) */
__device__ __forceinline__ uint4 philox(uint4 c, uint2 k)
{
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
    c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k.x, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k.y, (uint32_t)p0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}

/* (0, 1] with 53 bits */
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo)
{
  return ((double)((((uint64_t)hi << 32) | lo) >> 11) + 1.0) * (1.0 / 9007199254740992.0);
}

/* C's (short) of a double: truncation toward zero through int, 16-bit wrap as on x86 */
__device__ __forceinline__ uint32_t to_short(double v) { return (uint32_t)(uint16_t)(int16_t)(int32_t)v; }

}  // namespace

/* energy of vector blockIdx.x: length complex samples at x + blockIdx.x * stride */
__global__ void __launch_bounds__(SE_WG) k_signal_energy(const int32_t *__restrict__ x, size_t stride, uint32_t length,
                                                         int32_t *__restrict__ out)
{
  __shared__ uint32_t s_pw[SE_WG / 64], s_dc[SE_WG / 64];
  const int32_t *v = x + (size_t)blockIdx.x * stride;
  const uint32_t n = length & ~1u;                  /* the SSE loop runs length >> 1 sample pairs */
  uint32_t pw = 0, dre = 0, dim = 0;
  for (uint32_t i = threadIdx.x; i < n; i += SE_WG) {
    const uint32_t w = (uint32_t)v[i];
    const int32_t re = (int16_t)w, im = (int16_t)(w >> 16);
    /* pmaddwd (int32 wrap), psrad 4, paddd (wrap) */
    const int32_t p = (int32_t)((uint32_t)(re * re) + (uint32_t)(im * im));
    pw += (uint32_t)(p >> 4);
    dre += (uint32_t)re;                            /* paddw: only the low 16 bits matter */
    dim += (uint32_t)im;
  }
  const uint32_t dc = (dre & 0xFFFFu) | (dim << 16);
  uint32_t a = pw, lo = dc & 0xFFFFu, hi = dc >> 16;
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    lo += __shfl_xor(lo, o);
    hi += __shfl_xor(hi, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_pw[threadIdx.x >> 6] = a;
    s_dc[threadIdx.x >> 6] = (lo & 0xFFFFu) | (hi << 16);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sp = 0, sr = 0, si = 0;
    for (uint32_t w = 0; w < SE_WG / 64; w++) {
      sp += s_pw[w];
      sr += s_dc[w] & 0xFFFFu;
      si += s_dc[w] >> 16;
    }
    /* temp /= length with length unsigned (the int32 sum is converted), then <<= 4 */
    int32_t temp = (int32_t)(sp / length);
    temp = (int32_t)((uint32_t)temp << 4);
    /* the DC term: pmaddwd of the two 16-bit lane sums, / (length * length) as unsigned */
    const int32_t r16 = (int16_t)sr, i16 = (int16_t)si;
    const int32_t t2 = (int32_t)((uint32_t)(r16 * r16) + (uint32_t)(i16 * i16));
    const int32_t temp2 = (int32_t)((uint32_t)t2 / (length * length));
    temp -= temp2;
    out[blockIdx.x] = temp > 0 ? temp : 1;
  }
}

/* vector blockIdx.y, samples [blockIdx.x * 1024, +1024): the transmit samples (tx_len from tx, then
 * tail_len from the common tail) plus noise of standard deviation sqrt(sigma2 / 2) per component */
__global__ void __launch_bounds__(AW_WG) k_awgn(const int32_t *__restrict__ tx, size_t tx_stride, uint32_t tx_len,
                                                const int32_t *__restrict__ tail, uint32_t tail_len,
                                                int32_t *__restrict__ rx, size_t rx_stride,
                                                const int32_t *__restrict__ tx_lev, double offset_db, uint32_t seed_lo,
                                                uint32_t seed_hi, uint32_t vec0)
{
  __shared__ double s_sigma;
  const uint32_t vec = blockIdx.y;
  if (threadIdx.x == 0) {
    /* dlsim.c:2852-2853 */
    const double sigma2_dB = 10.0 * log10((double)tx_lev[vec]) + offset_db;
    s_sigma = sqrt(pow(10.0, sigma2_dB / 10.0) / 2.0);
  }
  __syncthreads();
  const double sigma = s_sigma;
  const uint32_t len = tx_len + tail_len;
  const int32_t *t = tx + (size_t)vec * tx_stride;
  int32_t *r = rx + (size_t)vec * rx_stride;
#pragma unroll
  for (uint32_t u = 0; u < AW_PER; u++) {
    const uint32_t i = blockIdx.x * (AW_WG * AW_PER) + u * AW_WG + threadIdx.x;
    if (i >= len) break;
    const uint32_t w = (uint32_t)(i < tx_len ? t[i] : tail[i - tx_len]);
    const uint4 q = philox(make_uint4(i, vec0 + vec, 0x5EEDu, 0xA3C5u), make_uint2(seed_lo, seed_hi));
    const double u1 = u53(q.x, q.y), u2 = u53(q.z, q.w);
    const double rad = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    const double re = (double)(int16_t)w + sigma * rad * cs, im = (double)(int16_t)(w >> 16) + sigma * rad * sn;
    r[i] = (int32_t)(to_short(re) | (to_short(im) << 16));
  }
}

hipError_t oai4g_launch_signal_energy(const int32_t *d_x, int n, size_t stride, uint32_t length, int32_t *d_out,
                                      hipStream_t s)
{
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_signal_energy, dim3(n), dim3(SE_WG), 0, s, d_x, stride, length, d_out);
  return hipGetLastError();
}

hipError_t oai4g_launch_awgn(const int32_t *d_tx, size_t tx_stride, uint32_t tx_len, const int32_t *d_tail,
                             uint32_t tail_len, int32_t *d_rx, size_t rx_stride, int n, const int32_t *d_tx_lev,
                             double offset_db, uint64_t seed, uint32_t vec0, hipStream_t s)
{
  if (n <= 0) return hipSuccess;
  const uint32_t len = tx_len + tail_len, per = AW_WG * AW_PER;
  hipLaunchKernelGGL(k_awgn, dim3((len + per - 1) / per, n), dim3(AW_WG), 0, s, d_tx, tx_stride, tx_len, d_tail,
                     tail_len, d_rx, rx_stride, d_tx_lev, offset_db, (uint32_t)seed, (uint32_t)(seed >> 32), vec0);
  return hipGetLastError();
}

/* ---------------------------------------------------------------------------------------
 * Fading channels (SIMULATION/TOOLS/random_channel.c:866-1015, multipath_channel.c:152-219), batched
 * over trials: every vector has its own descriptor state (a, ch, first_run).
 *
 * k_channel_taps, one wave per vector, what random_channel does in three phases:
 *   draws   per tap and antenna pair two normals scaled by sqrt(ricean_factor amps[i] / 2); on tap 0
 *           of a model with ricean_factor != 1 the line-of-sight term, its angle redrawn per pair where
 *           the model says so.  From the supplied sequence (the reference's order: tap, aarx, aatx: x,
 *           y, then the angle's uniform), or from Philox keyed by (seed, vector, step, tap, pair): the
 *           counter's last word is 0xC4A7, the noise streams' is 0xA3C5, so no counter is shared;
 *   state   acorr = R_sqrt[i / 3] anew; a = acorr on the first run, else sqrt(ff) a + sqrt(1 - ff) acorr;
 *   taps    ch[k] = sum_l sinc(k - delays[l] BW - 4) a[l] with the exact-zero test, or the copy for
 *           channel_length 1.
 * In the reference all trials share one descriptor, so with a forgetting factor trial t correlates
 * with trial t - 1; here the correlation runs along the successive calls of one vector.
 *
 * k_multipath, the hot path: a workgroup computes 1024 consecutive output samples of one vector for
 * all receive antennas.  The input tile plus a halo of channel_length - 1 samples per transmit antenna
 * is staged in LDS once (zeros in front of sample 0, as the reference's i - l < 0 test supplies); the
 * taps are wave-uniform loads; a thread keeps four consecutive samples' accumulators in registers
 * and slides a four-sample window over the taps, j outer and l inner as the reference's loop, with
 * separate double multiplies and adds (contraction off), so the doubles are the reference's built
 * without FMA.  The int16 form adds dlsim's noise (dlsim.c:2852-2864, k_awgn's counters for receive
 * antenna 0, word 2 plus a << 16 for antenna a) and writes (short); the double form writes the
 * doubles.  Output samples [0, |channel_offset|), which the reference never writes, are 0 (plus
 * noise) in the int16 form and left alone in the double form.
 * ------------------------------------------------------------------------------------- */
namespace {

constexpr uint32_t CT_WG = 64;
constexpr uint32_t MP_WG = 256;
constexpr uint32_t MP_PER = 4;
constexpr uint32_t MP_TILE = MP_WG * MP_PER;
constexpr double PI = 3.14159265358979323846;

struct cplx {
  double x, y;
};

/* the (j, l) sum of four consecutive samples: win slides over s (the thread's first sample at tap 0 is
 * s[3 .. 0] behind base), acc[ii][u] as rx_tmp of receive antenna ii and sample u */
template <int NRX, class LOAD>
__device__ __forceinline__ void mp_accumulate(cplx (&acc)[NRX][MP_PER], uint32_t nb_tx, uint32_t L, uint32_t span,
                                              uint32_t base, const double *__restrict__ ch, double path_loss,
                                              LOAD load)
{
#pragma clang fp contract(off)
  for (uint32_t j = 0; j < nb_tx; j++) {
    const uint32_t row = j * span + base + (L - 1);
    cplx w[MP_PER];
#pragma unroll
    for (uint32_t u = 0; u + 1 < MP_PER; u++) w[u] = load(row + u + 1);   /* w[u] of tap l is entry row + u - l; tap 0 shifts first */
    const double *c = ch + (size_t)j * NRX * L * 2;
#pragma unroll 4
    for (uint32_t l = 0; l < L; l++) {
#pragma unroll
      for (uint32_t u = MP_PER - 1; u > 0; u--) w[u] = w[u - 1];
      w[0] = load(row - l);
#pragma unroll
      for (int ii = 0; ii < NRX; ii++) {
        const double cx = c[((size_t)ii * L + l) * 2], cy = c[((size_t)ii * L + l) * 2 + 1];
#pragma unroll
        for (uint32_t u = 0; u < MP_PER; u++) {
          acc[ii][u].x = acc[ii][u].x + ((w[u].x * cx) - (w[u].y * cy));
          acc[ii][u].y = acc[ii][u].y + ((w[u].y * cx) + (w[u].x * cy));
        }
      }
    }
  }
  /* rx_tmp path_loss, kept out of the noise's contraction */
#pragma unroll
  for (int ii = 0; ii < NRX; ii++)
#pragma unroll
    for (uint32_t u = 0; u < MP_PER; u++) {
      acc[ii][u].x = acc[ii][u].x * path_loss;
      acc[ii][u].y = acc[ii][u].y * path_loss;
    }
}

}  // namespace

__global__ void __launch_bounds__(CT_WG) k_channel_taps(chan_dev_t c, uint32_t seed_lo, uint32_t seed_hi, uint32_t vec0,
                                                        uint32_t step, const double *__restrict__ draws,
                                                        uint32_t draws_per)
{
#pragma clang fp contract(off)
  __shared__ cplx s_new[OAI4G_CHAN_TAPS * 4], s_a[OAI4G_CHAN_TAPS * 4];
  const uint32_t v = blockIdx.x, npair = c.nb_tx * c.nb_rx, L = c.channel_length;
  const bool los = c.ricean_factor != 1.0, angles = los && c.random_aoa == 1;
  const bool first = c.first_run[v] != 0;
  for (uint32_t t = threadIdx.x; t < c.nb_taps * npair; t += CT_WG) {
    const uint32_t tap = t / npair, seq = t % npair, aarx = seq / c.nb_tx, aatx = seq % c.nb_tx;
    const uint32_t p = aarx + aatx * c.nb_rx;
    double gx, gy, un = 0.0;
    if (draws) {
      /* the reference's order: on tap 0 of a model with drawn angles three values per pair, else two */
      const double *d = draws + (size_t)v * draws_per;
      const uint32_t at = angles ? (tap == 0 ? 3 * seq : npair + 2 * t) : 2 * t;
      gx = d[at];
      gy = d[at + 1];
      if (angles && tap == 0) un = d[at + 2];
    } else {
      const uint2 key = make_uint2(seed_lo, seed_hi);
      const uint4 q = philox(make_uint4(tap * 4u + p, vec0 + v, step, 0xC4A7u), key);
      const double rad = sqrt(-2.0 * log(u53(q.x, q.y)));
      double sn, cs;
      sincospi(2.0 * u53(q.z, q.w), &sn, &cs);
      gx = rad * cs;
      gy = rad * sn;
      if (angles && tap == 0) {
        const uint4 r = philox(make_uint4(0x100u + p, vec0 + v, step, 0xC4A7u), key);
        un = u53(r.x, r.y);
      }
    }
    const double sc = sqrt(c.ricean_factor * c.amps[tap] / 2);
    double x = sc * gx, y = sc * gy;
    if (tap == 0 && los) {
      const double aoa = angles ? un * 2 * PI : c.aoa;
      const double ph = PI * (((double)aarx - (double)aatx) * sin(aoa));
      x += cos(ph) * sqrt(1.0 - c.ricean_factor);
      y += sin(ph) * sqrt(1.0 - c.ricean_factor);
    }
    s_new[tap * 4 + p] = {x, y};
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < c.nb_taps * npair; t += CT_WG) {
    const uint32_t tap = t / npair, r = t % npair;
    const double *R = c.R + ((size_t)(tap / 3) * npair + r) * npair * 2;
    cplx s = {0.0, 0.0};
    for (uint32_t k = 0; k < npair; k++) {
      const cplx b = s_new[tap * 4 + k];
      s.x += R[2 * k] * b.x - R[2 * k + 1] * b.y;
      s.y += R[2 * k] * b.y + R[2 * k + 1] * b.x;
    }
    double *a = c.a + (((size_t)v * c.nb_taps + tap) * npair + r) * 2;
    if (!first) {
      s.x = c.sqrt_ff * a[0] + c.sqrt_1mff * s.x;
      s.y = c.sqrt_ff * a[1] + c.sqrt_1mff * s.y;
    }
    a[0] = s.x;
    a[1] = s.y;
    s_a[tap * 4 + r] = s;
  }
  __syncthreads();
  double *ch = c.ch + (size_t)v * npair * L * 2;
  for (uint32_t t = threadIdx.x; t < npair * L; t += CT_WG) {
    const uint32_t p = t / L, k = t % L;
    cplx s = {0.0, 0.0};
    if (L == 1) {
      s = s_a[p];
    } else {
      for (uint32_t l = 0; l < c.nb_taps; l++) {
        const double d = (double)k - (c.delays[l] * c.BW) - 4.0;        /* NB_SAMPLES_CHANNEL_OFFSET */
        const double w = d == 0.0 ? 1.0 : sin(PI * d) / (PI * d);
        s.x += w * s_a[l * 4 + p].x;
        s.y += w * s_a[l * 4 + p].y;
      }
    }
    ch[2 * t] = s.x;
    ch[2 * t + 1] = s.y;
  }
  if (threadIdx.x == 0 && first) c.first_run[v] = 0;
}

/* DBL: [re, im] double pairs in and out, no noise; else int16 IQ words in, (short) plus noise out */
template <bool DBL, int NRX>
__global__ void __launch_bounds__(MP_WG) k_multipath(multipath_args_t a)
{
  extern __shared__ double s_mp[];                     /* [nb_tx][MP_TILE + L - 1] words or double pairs */
  __shared__ double s_sigma;
  const uint32_t vec = blockIdx.y, L = a.channel_length, span = MP_TILE + L - 1;
  const uint32_t length = a.tx_len + a.tail_len, o0 = blockIdx.x * MP_TILE;
  /* LDS entry e of antenna j is input sample o0 - dd - (L - 1) + e; outside [0, length) it is zero */
  const int64_t first = (int64_t)o0 - a.dd - (L - 1);
  for (uint32_t e = threadIdx.x; e < a.nb_tx * span; e += MP_WG) {
    const uint32_t j = e / span;
    const int64_t i = first + (e - j * span);
    const bool in = i >= 0 && i < (int64_t)length;
    if (DBL) {
      const cplx *t = (const cplx *)a.tx + (size_t)vec * a.tx_stride + (size_t)j * a.tx_ant_stride;
      double x = 0.0, y = 0.0;
      if (in) {
        const cplx *src = i < a.tx_len ? t + i : (const cplx *)a.tail + ((size_t)j * a.tail_len + (i - a.tx_len));
        x = src->x;
        y = src->y;
      }
      ((cplx *)s_mp)[e] = {x, y};
    } else {
      const uint32_t *t = (const uint32_t *)a.tx + (size_t)vec * a.tx_stride + (size_t)j * a.tx_ant_stride;
      ((uint32_t *)s_mp)[e] = !in ? 0u : (i < a.tx_len ? t[i] : ((const uint32_t *)a.tail)[(size_t)j * a.tail_len + (i - a.tx_len)]);
    }
  }
  if (!DBL && threadIdx.x == 0) {
    /* dlsim.c:2716-2720, :2852-2853: the antennas' energies summed as integers */
    int32_t lev = 0;
    for (uint32_t j = 0; j < a.nb_tx; j++) lev += a.tx_lev[(size_t)vec * a.nb_tx + j];
    const double sigma2_dB = 10.0 * log10((double)lev) + a.offset_db;
    s_sigma = sqrt(pow(10.0, sigma2_dB / 10.0) / 2.0);
  }
  __syncthreads();
  cplx acc[NRX][MP_PER];
#pragma unroll
  for (int ii = 0; ii < NRX; ii++)
#pragma unroll
    for (uint32_t u = 0; u < MP_PER; u++) acc[ii][u] = {0.0, 0.0};
  const double *ch = a.ch + (size_t)vec * a.nb_tx * NRX * L * 2;
  const uint32_t base = threadIdx.x * MP_PER;
  if (DBL)
    mp_accumulate<NRX>(acc, a.nb_tx, L, span, base, ch, a.path_loss, [&](uint32_t e) { return ((const cplx *)s_mp)[e]; });
  else
    mp_accumulate<NRX>(acc, a.nb_tx, L, span, base, ch, a.path_loss, [&](uint32_t e) {
      const uint32_t w = ((const uint32_t *)s_mp)[e];
      return cplx{(double)(int16_t)w, (double)(int16_t)(w >> 16)};
    });
  const uint32_t o = o0 + base;
  if (o >= length) return;
#pragma unroll
  for (int ii = 0; ii < NRX; ii++) {
    uint32_t out[MP_PER];
#pragma unroll
    for (uint32_t u = 0; u < MP_PER; u++) {
      const uint32_t i = o + u;
      const double rx = acc[ii][u].x, ry = acc[ii][u].y;
      const size_t at = (size_t)vec * a.rx_stride + (size_t)(i / a.seg_len) * a.seg_stride + (size_t)ii * a.rx_ant_stride +
                        i % a.seg_len;
      if (DBL) {
        if (i < length && i >= a.dd) ((cplx *)a.rx)[at] = {rx, ry};
        continue;
      }
      const double sigma = s_sigma;
      const uint4 q = philox(make_uint4(i, a.vec0 + vec, 0x5EEDu + ((uint32_t)ii << 16), 0xA3C5u), make_uint2(a.seed_lo, a.seed_hi));
      const double u1 = u53(q.x, q.y), u2 = u53(q.z, q.w);
      const double rad = sqrt(-2.0 * log(u1));
      double sn, cs;
      sincospi(2.0 * u2, &sn, &cs);
      const double re = rx + sigma * rad * cs, im = ry + sigma * rad * sn;
      out[u] = to_short(re) | (to_short(im) << 16);
      if (!a.vec4 && i < length) ((uint32_t *)a.rx)[at] = out[u];
    }
    if (!DBL && a.vec4) {
      /* seg_len, the strides and length are multiples of 4 and rx is 16-byte aligned: one 16-byte store */
      const size_t at = (size_t)vec * a.rx_stride + (size_t)(o / a.seg_len) * a.seg_stride + (size_t)ii * a.rx_ant_stride +
                        o % a.seg_len;
      *(uint4 *)((uint32_t *)a.rx + at) = make_uint4(out[0], out[1], out[2], out[3]);
    }
  }
}

hipError_t oai4g_launch_channel_taps(const chan_dev_t &c, int n, uint64_t seed, uint32_t vec0, uint32_t step,
                                     const double *d_draws, hipStream_t s)
{
  if (n <= 0) return hipSuccess;
  const uint32_t npair = c.nb_tx * c.nb_rx;
  const uint32_t per = c.nb_taps * npair * 2 + (c.ricean_factor != 1.0 && c.random_aoa == 1 ? npair : 0);
  hipLaunchKernelGGL(k_channel_taps, dim3(n), dim3(CT_WG), 0, s, c, (uint32_t)seed, (uint32_t)(seed >> 32), vec0, step,
                     d_draws, per);
  return hipGetLastError();
}

hipError_t oai4g_launch_multipath(const multipath_args_t &a, int n, bool double_form, hipStream_t s)
{
  if (n <= 0) return hipSuccess;
  const uint32_t length = a.tx_len + a.tail_len;
  const dim3 grid((length + MP_TILE - 1) / MP_TILE, n);
  const size_t lds = (size_t)a.nb_tx * (MP_TILE + a.channel_length - 1) * (double_form ? 16 : 4);
  if (double_form) {
    if (a.nb_rx == 1) hipLaunchKernelGGL((k_multipath<true, 1>), grid, dim3(MP_WG), lds, s, a);
    else hipLaunchKernelGGL((k_multipath<true, 2>), grid, dim3(MP_WG), lds, s, a);
  } else {
    if (a.nb_rx == 1) hipLaunchKernelGGL((k_multipath<false, 1>), grid, dim3(MP_WG), lds, s, a);
    else hipLaunchKernelGGL((k_multipath<false, 2>), grid, dim3(MP_WG), lds, s, a);
  }
  return hipGetLastError();
}

/* ---------------------------------------------------------------------------------------
 * HARQ round state of a batch of slots (dlsim's round loop, dlsim.c:2141-3460, one slot per HARQ
 * process), advanced on the device after a decode.  One wave per slot:
 *   fail = any of the slot's C blocks has iters > max_it;
 *   round_trials[round]++, and errs[round]++ on a failure (dlsim.c:2143, 3438);
 *   failed with a round left: round++, the payload row is kept, done = 0;
 *   else: done = 1 (decoded) or 2 (not decoded after the last round), round = 0, the slot's running
 *   trial index advances and its payload row is refilled: row (trial, slot) of the k_fill stream of
 *   `seed`, i.e. 8-byte word w of the row is word (trial n_slots + slot) row_words + w of that stream
 *   (trial 0 is oai4g_fill_payload over the whole buffer);
 *   rv[slot][cw] = round & 3, clear[slot] = (round == 0) for the next step.
 * ------------------------------------------------------------------------------------- */
__global__ void __launch_bounds__(64) k_harq_advance(harq_state_t st, uint32_t n_slots, uint32_t C, uint32_t max_it,
                                                     uint32_t num_rounds, uint32_t n_cw, uint32_t row_words, uint64_t seed,
                                                     const uint8_t *__restrict__ iters)
{
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= n_slots) return;
  /* every lane derives the slot's (wave-uniform) state from the same loads */
  bool fail = false;
  for (uint32_t r = 0; r < C; r++) fail = fail || iters[(size_t)i * C + r] > max_it;
  const uint32_t round = st.round[i] & 3u;
  const bool again = fail && round + 1 < num_rounds;
  const uint32_t next = again ? round + 1 : 0u;
  const uint32_t trial = st.trial[i] + (again ? 0u : 1u);
  if (!again) {
    uint64_t *row = (uint64_t *)st.payload + (size_t)i * row_words;
    const uint64_t w0 = ((uint64_t)trial * n_slots + i) * row_words;
    for (uint32_t w = lane; w < row_words; w += 64) row[w] = oai4g_payload_word(seed, w0 + w);
  }
  if (lane == 0) {
    atomicAdd(&st.counters[round], 1u);
    if (fail) atomicAdd(&st.counters[4 + round], 1u);
    st.round[i] = (uint8_t)next;
    st.trial[i] = trial;
    st.clear[i] = next == 0 ? 1 : 0;
    st.done[i] = again ? 0 : (fail ? 2 : 1);
    for (uint32_t cw = 0; cw < n_cw; cw++) st.rv[(size_t)i * n_cw + cw] = (uint8_t)(next & 3u);
  }
}

hipError_t oai4g_launch_harq_advance(const harq_state_t &st, uint32_t n_slots, uint32_t C, uint32_t max_it,
                                     uint32_t num_rounds, uint32_t n_cw, uint32_t row_words, uint64_t seed,
                                     const uint8_t *d_iters, hipStream_t s)
{
  if (n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(k_harq_advance, dim3(n_slots), dim3(64), 0, s, st, n_slots, C, max_it, num_rounds, n_cw, row_words,
                     seed, d_iters);
  return hipGetLastError();
}
