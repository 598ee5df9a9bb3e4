/*
 * gfx950 kernel of the UE control decoding path: one tail-biting convolutional decode, whole.
 *   dci_decoding (PHY/LTE_TRANSPORT/dci.c:2426-2489) and rx_pbch from the quantised soft bits on
 *   (PHY/LTE_TRANSPORT/pbch.c:975-1043): pbch_unscrambling (:785-814), lte_rate_matching_cc_rx
 *   (PHY/CODING/lte_rate_matching.c:834-906), sub_block_deinterleaving_cc (:245-291),
 *   phy_viterbi_lte_sse2 (PHY/CODING/viterbi_lte.c:140-416) and the CRC16 against the 16 bits that
 *   follow the payload (crc_byte.c:155-171, extract_crc dci.c:122-163).
 *
 * One 64-lane wave per decode, lane = NEW trellis state t = 2k + b:
 *   1. lane-parallel gather of the 3 D Viterbi inputs into LDS: entry q sums e[plan[q] + 3 D r] for
 *      every repetition r below E (the host plan folds the <NULL> set of generate_dummy_w_cc, the
 *      circular buffer and the deinterleaver into one index), clamped to [-8, 7];
 *   2. 2 D add-compare-select steps.  The three soft inputs of a step are wave-uniform LDS reads;
 *      lane t forms the branch metrics w[rev[t]] and w[rev[t + 64]] from its own three signs, fetches
 *      the metrics of its predecessors k and k + 32 with two ds_bpermute, adds with saturation at 255,
 *      takes the maximum (a tie selects k + 32, as cmpeq(max, b) does) and subtracts the wave minimum
 *      (a DPP reduction).  All literal: no deferred offset.  The 64 decisions are one ballot, kept as
 *      8 bytes per step in LDS (second pass only: the reference resets TB_ptr per pass);
 *   3. the first lane holding the largest final metric starts the traceback (all metrics equal: 0);
 *   4. CRC16 of the payload XOR the 16 bits after it; vector stores of the bytes and a 4-byte trailer.
 * Nothing between the steps touches HBM.  NMAX = 64 serves every DCI and the PBCH (D <= 61),
 * NMAX = 512 the phy_viterbi_lte drop-in.
 */
#include <type_traits>

#include "oai4g_internal.h"

static __device__ __forceinline__ uint32_t dpp_min(uint32_t v, uint32_t t) { return t < v ? t : v; }

/* minimum over the wave, in every lane.  Within a row of 16: xor 1, xor 2 (quad_perm), the mirrored
 * half row and the mirrored row; min is idempotent, so after these four every lane of a row holds the
 * row's minimum.  Then row_bcast:15 and row_bcast:31 accumulate the rows into row 3 (lanes without a
 * source keep `old`), and lane 63 is read back as a scalar. */
static __device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
  v = dpp_min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));    /* quad_perm [1,0,3,2] */
  v = dpp_min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));    /* quad_perm [2,3,0,1] */
  v = dpp_min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));   /* row_half_mirror */
  v = dpp_min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));   /* row_mirror */
  v = dpp_min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x142, 0xF, 0xF, false));   /* row_bcast:15 */
  v = dpp_min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x143, 0xF, 0xF, false));   /* row_bcast:31 */
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

/* ccodelte_table_rev[i] (ccoding_byte_lte.c:270-289): bit j = parity(i & glte_rev[j]) */
static __device__ __forceinline__ uint32_t cc_rev(uint32_t i)
{
  return (__popc(i & 0155u) & 1u) | ((__popc(i & 0117u) & 1u) << 1) | ((__popc(i & 0127u) & 1u) << 2);
}

/* ARGS = cc_det_args_t: the PDCCH batch whose subframes carry a detected num_pdcch_symbols each; the jobs, the
 * gather table and the receive plans are then those of the subframe's own count.
 * ARGS = cc_hyp_args_t: pbch_detection's eight hypotheses of a subframe as its jobs; job j unscrambles all of its
 * 480 soft bits with the Gold words of quarter j >> 1 */
template <int NMAX, typename ARGS = cc_args_t>
__global__ void __launch_bounds__(64) k_cc_decode(ARGS a)
{
  constexpr bool DET = std::is_same<ARGS, cc_det_args_t>::value;
  constexpr bool HYP = std::is_same<ARGS, cc_hyp_args_t>::value;
  __shared__ int8_t s_d[3 * NMAX];
  __shared__ uint64_t s_tb[NMAX];
  __shared__ uint8_t s_out[NMAX / 8 + 8];
  const uint32_t lane = threadIdx.x, dec = blockIdx.x, item = dec / a.n_jobs;
  uint32_t row = a.tab ? (a.first_row + item) % 10u : 0u;              /* PDCCH batch: the subframe index */
  uint32_t jrow = row * a.n_jobs + (dec - item * a.n_jobs);
  if constexpr (DET) {
    const uint32_t n = (uint32_t)a.cfi[item] - 1u, j = dec - item * a.n_jobs;
    if (n > 2u) return;
    pdcch_det_set_t st = a.set[0];
    if (n == 1u) st = a.set[1];
    if (n == 2u) st = a.set[2];
    if (j >= st.n_jobs) return;
    row = (a.first_row + item * a.sf_step) % 10u;
    jrow = row * st.n_jobs + j;
    a.jobs = st.jobs;
    a.tab = st.tab;
    a.tab_stride = st.tab_stride;
    a.plan = st.plan;
  }
  const cc_job_t job = a.jobs[jrow];
  const uint32_t D = job.D, D3 = 3u * D, E = job.E;
  if (D == 0 || D > (uint32_t)NMAX) return;
  const int8_t *__restrict__ e = a.e + (size_t)item * a.e_stride + job.e_off;
  const uint32_t *__restrict__ tab = a.tab ? a.tab + (size_t)row * a.tab_stride + job.e_off : nullptr;
  const int16_t *__restrict__ comp = a.comp + (size_t)item * a.comp_stride;
  if constexpr (HYP) a.gold += 15u * ((dec - item * a.n_jobs) >> 1);
  const uint32_t qlo = !HYP && a.gold ? (uint32_t)a.quarter[item] * (E >> 2) : 0u, qhi = HYP ? E : a.gold ? qlo + (E >> 2) : 0u;
  bool clamped = false;
  for (uint32_t q = lane; q < D3; q += 64) {
    int v = 0;
    if (a.raw) {
      v = e[q];
    } else {
      for (uint32_t k = a.plan[job.plan_off + q]; k < E; k += D3) {
        int8_t x = tab ? oai4g_pdcch_soft(comp, tab[k]) : e[k];
        if (k >= qlo && k < qhi && ((a.gold[k >> 5] >> (k & 31)) & 1u) == 0) x = (int8_t)-x;   /* pbch_unscrambling */
        v += x;
      }
    }
    const int c = v > 7 ? 7 : (v < -8 ? -8 : v);
    clamped |= c != v;
    s_d[q] = (int8_t)c;
  }
  for (uint32_t i = lane; i < (uint32_t)(NMAX / 8 + 8); i += 64) s_out[i] = 0;
  __syncthreads();

  /* branch-metric signs of this lane's two predecessors: w[c] = 24 + sum_i (bit i of c ? +in_i : -in_i) */
  const uint32_t c_lo = cc_rev(lane), c_hi = cc_rev(lane + 64);
  const int l0 = (c_lo & 1) ? 1 : -1, l1 = (c_lo & 2) ? 1 : -1, l2 = (c_lo & 4) ? 1 : -1;
  const int h0 = (c_hi & 1) ? 1 : -1, h1 = (c_hi & 2) ? 1 : -1, h2 = (c_hi & 4) ? 1 : -1;
  const int src_lo = (int)((lane >> 1) << 2), src_hi = (int)(((lane >> 1) + 32) << 2);   /* ds_bpermute byte addresses */
  uint32_t m = 0;
  for (int iter = 0; iter < 2; iter++) {
    for (uint32_t p = 0; p < D; p++) {
      const int i0 = s_d[3 * p], i1 = s_d[3 * p + 1], i2 = s_d[3 * p + 2];
      const uint32_t w_lo = (uint32_t)(24 + l0 * i0 + l1 * i1 + l2 * i2);
      const uint32_t w_hi = (uint32_t)(24 + h0 * i0 + h1 * i1 + h2 * i2);
      uint32_t a_lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lo, (int)m) + w_lo;
      uint32_t a_hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src_hi, (int)m) + w_hi;
      a_lo = a_lo > 255u ? 255u : a_lo;                            /* adds_epu8 */
      a_hi = a_hi > 255u ? 255u : a_hi;
      const uint32_t nm = a_lo > a_hi ? a_lo : a_hi;
      const unsigned long long tb = __ballot(nm == a_hi);          /* cmpeq(max, b): a tie selects k + 32 */
      if (iter == 1 && lane == 0) s_tb[p] = tb;
      m = nm - wave_min_u32(nm);                                   /* subs_epu8 of the minimum */
    }
  }
  __syncthreads();

  /* first state with the largest metric (viterbi_lte.c:341-367) */
  uint32_t mx = m;
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)mx, o);
    mx = t > mx ? t : mx;
  }
  const uint32_t start = (uint32_t)__ffsll((long long)__ballot(m == mx)) - 1u;

  /* traceback, the same in every lane; lane 0 keeps the bytes */
  uint32_t s = start, cur = 0;
  for (int p = (int)D - 1; p >= 0; p--) {
    cur |= (s & 1u) << (7 - (p & 7));
    s = (s >> 1) + 32u * (uint32_t)((s_tb[p] >> s) & 1ull);
    if ((p & 7) == 0) {
      if (lane == 0) s_out[p >> 3] = (uint8_t)cur;
      cur = 0;
    }
  }
  __syncthreads();

  uint32_t crc = 0;
  const uint32_t A = job.crc_bits;
  if (A) {   /* crc16 MSB first, polynomial 0x1021, then XOR the 16 bits that follow bit A */
    uint32_t reg = 0, rx = 0;
    for (uint32_t i = 0; i < A; i++) {
      const uint32_t fb = ((reg >> 15) ^ ((uint32_t)s_out[i >> 3] >> (7 - (i & 7)))) & 1u;
      reg = (reg << 1) & 0xFFFFu;
      if (fb) reg ^= 0x1021u;
    }
    for (uint32_t i = A; i < A + 16; i++) rx = (rx << 1) | (((uint32_t)s_out[i >> 3] >> (7 - (i & 7))) & 1u);
    crc = reg ^ rx;
  }
  const bool any_clamped = __ballot(clamped) != 0ull;
  uint8_t *__restrict__ rec = a.out + (size_t)dec * a.out_stride;
  if (a.pbch_out) {   /* the MIB reversed (pbch.c:1017) and the antenna count of the CRC mask (:1036-1043) */
    if (lane < 3) rec[lane] = s_out[2 - lane];
    if (lane == 3) rec[3] = crc == 0 ? 1 : (crc == 0xFFFFu ? 2 : (crc == 0x5555u ? 4 : 0xFF));
  } else {
    if (lane + 4 < a.out_stride && lane < (uint32_t)(NMAX / 8 + 8)) rec[lane] = s_out[lane];   /* zeros after the last decoded byte */
    if (lane < 4) {
      const uint32_t tr = lane == 0 ? (crc & 0xFFu) : lane == 1 ? (crc >> 8) : lane == 2 ? (any_clamped ? 1u : 0u) : start;
      rec[a.out_stride - 4 + lane] = (uint8_t)tr;
    }
  }
  if (a.metrics) a.metrics[(size_t)dec * 64 + lane] = (uint8_t)m;
}

/* the soft-bit drop-in: pdcch_llr + demapping + deinterleaving + unscrambling as one gather */
__global__ void __launch_bounds__(256) k_pdcch_soft(const int16_t *__restrict__ comp, const uint32_t *__restrict__ tab,
                                                    uint32_t n, int8_t *__restrict__ e)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) e[i] = oai4g_pdcch_soft(comp, tab[i]);
}

hipError_t oai4g_launch_pdcch_soft(const int16_t *d_comp, const uint32_t *d_tab, uint32_t n, int8_t *d_e, hipStream_t s)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pdcch_soft, dim3((n + 255) / 256), dim3(256), 0, s, d_comp, d_tab, n, d_e);
  return hipGetLastError();
}

/* second stage of the batched DCI search: one lane per subframe walks its decoded candidates in plan
 * order under dci_decoding_procedure0's rules and dci_decoding_procedure's stops between calls */
/* ARGS = pdcch_resolve_det_args_t: the candidates are those of the subframe's detected count; the records stay
 * a.n_jobs apart */
template <typename ARGS = pdcch_resolve_args_t>
__global__ void __launch_bounds__(64) k_pdcch_resolve(ARGS a)
{
  constexpr bool DET = !std::is_same<ARGS, pdcch_resolve_args_t>::value;
  const uint32_t sf = blockIdx.x * 64u + threadIdx.x;
  if (sf >= a.n_sf) return;
  uint32_t row = (a.first_row + sf) % 10u, cstride = a.n_jobs;
  if constexpr (DET) {
    const uint32_t n = (uint32_t)a.cfi[sf] - 1u;
    pdcch_det_set_t s = a.set[0];
    if (n == 1u) s = a.set[1];
    if (n == 2u) s = a.set[2];
    row = (a.first_row + sf * a.sf_step) % 10u;
    a.cands = s.cands;
    a.n_cand = s.n_cand;
    cstride = s.n_jobs;
    if (n > 2u) cstride = 0u;                                           /* no count, no candidates */
  }
  const uint32_t nc = DET && cstride == 0u ? 0u : a.n_cand[row];
  oai4g_pdcch_rx_result_t &o = a.out[sf];
  pdcch_state_t st = {};
  st.nCCE = -1;
  uint32_t old_cnt = 0, prev_plan = 0;
  for (uint32_t c = 0; c < nc; c++) {
    const pdcch_cand_t cd = a.cands[row * cstride + c];
    if (cd.first) {
      if (c > 0) {
        if (st.map[0] == 0xFFFFu || (st.format0_found && st.format_c_found)) break;
        if (a.plans[prev_plan].stop_if_found && st.dci_cnt > old_cnt) break;
      }
      old_cnt = st.dci_cnt;
      prev_plan = cd.plan;
    }
    const uint8_t *rec = a.rec + ((size_t)sf * a.n_jobs + c) * OAI4G_PDCCH_REC;
    const uint32_t crc = rec[OAI4G_PDCCH_REC - 4] | ((uint32_t)rec[OAI4G_PDCCH_REC - 3] << 8);
    oai4g_pdcch_resolve(st, a.plans[cd.plan], cd.cce, rec, crc, a.crnti, a.si_rnti, a.ra_rnti, o.dci, OAI4G_PDCCH_MAX_DCI);
  }
  o.dci_cnt = st.dci_cnt;
  o.format0_found = st.format0_found;
  o.format_c_found = st.format_c_found;
  o.overflow = st.overflow;
  o.nCCE = st.nCCE;
  for (int i = 0; i < 3; i++) o.CCEmap[i] = st.map[i];
}

hipError_t oai4g_launch_pdcch_resolve(const pdcch_resolve_args_t &a, hipStream_t s)
{
  if (a.n_sf == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pdcch_resolve<>, dim3((a.n_sf + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t oai4g_launch_pdcch_resolve_detected(const pdcch_resolve_det_args_t &a, hipStream_t s)
{
  if (a.n_sf == 0) return hipSuccess;
  hipLaunchKernelGGL((k_pdcch_resolve<pdcch_resolve_det_args_t>), dim3((a.n_sf + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t oai4g_launch_cc_decode(const cc_args_t &a, uint32_t nmax, hipStream_t s)
{
  const uint32_t n = a.n_items * a.n_jobs;
  if (n == 0) return hipSuccess;
  if (nmax <= 64)
    hipLaunchKernelGGL(k_cc_decode<64>, dim3(n), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL(k_cc_decode<512>, dim3(n), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t oai4g_launch_cc_decode_hyp(const cc_hyp_args_t &a, hipStream_t s)
{
  const uint32_t n = a.n_items * a.n_jobs;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_cc_decode<64, cc_hyp_args_t>), dim3(n), dim3(64), 0, s, a);
  return hipGetLastError();
}

/* every DCI fits 64 trellis steps; a.n_jobs is the largest job count of the three sets */
hipError_t oai4g_launch_cc_decode_detected(const cc_det_args_t &a, hipStream_t s)
{
  const uint32_t n = a.n_items * a.n_jobs;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_cc_decode<64, cc_det_args_t>), dim3(n), dim3(64), 0, s, a);
  return hipGetLastError();
}
