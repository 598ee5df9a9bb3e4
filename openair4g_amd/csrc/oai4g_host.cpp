/*
 * Host side of openair4g_amd: C ABI (include/oai4g.h), configuration derivation, drop-in
 * entry points and the batched transmit path.  All arithmetic on samples / bits runs in the
 * gfx950 kernels; this file only derives parameters (what the reference recomputes on every
 * call: segmentation, rate-matching geometry, RE maps), moves buffers and launches.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/oai4g.h"
#include "../../include/oai4g_qpp.h"
#include "../../include/oai4g_tbs.h"
#include "oai4g_internal.h"
#include "oai4g_dev_buf.h"
#include "oai4g_rm_geom.h"

/* ------------------------------------------------------------------------------------------
 * errors
 * ---------------------------------------------------------------------------------------- */
static thread_local char g_err[512] = "";

static void set_err(const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char *oai4g_last_error(void) { return g_err; }

/* the error slot for the library's other translation units (oai4g_dist.cpp) */
void oai4g_set_error(const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define HCK(call, ret)                                                                          \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) {                                                                     \
      set_err("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);       \
      fprintf(stderr, "[openair4g_amd] %s\n", g_err);                                           \
      return ret;                                                                               \
    }                                                                                           \
  } while (0)

/* ------------------------------------------------------------------------------------------
 * global device tables: twiddles, Gold jump-ahead
 * ---------------------------------------------------------------------------------------- */
static pthread_once_t g_once = PTHREAD_ONCE_INIT;
static int g_init_status = -1;
static char g_init_err[512] = "";
static uint32_t *g_tw = nullptr, *g_twf = nullptr, *g_gx1 = nullptr, *g_gx2j = nullptr;
static int g_n_cu = 256;
static uint32_t h_gx1[OAI4G_GOLD_LANES], h_gx2j[OAI4G_GOLD_LANES * 32];

static void twiddle_host(int N, int m, int16_t *re, int16_t *im)
{
  /* W_N^m in Q15: (floor(32767 cos), floor(-32767 sin)) — reproduces lte_dfts.c tw* tables */
  double a = 2.0 * M_PI * (double)m / (double)N;
  *re = (int16_t)floor(32767.0 * cos(a));
  *im = (int16_t)floor(-32767.0 * sin(a));
}

/* forward DFT operand pair (a, b) with x * W = (dot2(x, a), dot2(x, b)): a = (Wr, -Wi), b = (Wi, Wr)
 * for cmult (tw1024, tw2048) and the packed_cmult2 tables tw16a/b … tw512a/b; tw256a alone holds
 * floor(32767 sin) as its second entry (lte_dfts.c:2162 vs :2167) */
static void dft_twiddle_ab_host(int N, int m, int16_t a[2], int16_t b[2])
{
  int16_t wr, wi;
  twiddle_host(N, m, &wr, &wi);
  a[0] = wr;
  a[1] = (N == 256) ? (int16_t)floor(32767.0 * sin(2.0 * M_PI * (double)m / (double)N)) : (int16_t)-wi;
  b[0] = wi;
  b[1] = wr;
}

static void gold_step_h(uint32_t *x1, uint32_t *x2)
{
  *x1 = (*x1 >> 1) ^ (*x1 >> 4);
  *x1 = *x1 ^ (*x1 << 31) ^ (*x1 << 28);
  *x2 = (*x2 >> 1) ^ (*x2 >> 2) ^ (*x2 >> 3) ^ (*x2 >> 4);
  *x2 = *x2 ^ (*x2 << 31) ^ (*x2 << 30) ^ (*x2 << 29) ^ (*x2 << 28);
}

/* lte_gold_generic's reset (lte_gold.c:151-177): x1 = 1 + 2^31, bit 31 of x2 from c_init, and the
 * 49 discarded word steps */
static void gold_start_h(uint32_t c_init, uint32_t *x1, uint32_t *x2)
{
  *x1 = 1u + (1u << 31);
  *x2 = c_init ^ ((c_init ^ (c_init >> 1) ^ (c_init >> 2) ^ (c_init >> 3)) << 31);
  for (int n = 1; n < 50; n++) gold_step_h(x1, x2);
}

/* the first n Gold words of c_init */
static void gold_seq_h(uint32_t c_init, uint32_t *w, size_t n)
{
  uint32_t x1, x2;
  gold_start_h(c_init, &x1, &x2);
  for (size_t i = 0; i < n; i++) {
    gold_step_h(&x1, &x2);
    w[i] = x1 ^ x2;
  }
}

/* the column permutation of the convolutional code's sub-block interleaver (36.212 Table 5.1.4-2) */
static const uint8_t bitrev_cc[32] = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31,
                                      0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};

/* lte_gold (LTE_REFSIG/lte_gold.c:52-93): CRS Gold words [ns][pilot l][14] */
/* 14 CRS Gold words of slot ns, symbol lsym of the slot: c_init = 2^10 (7(ns+1) + lsym + 1)
 * (2 Nid + 1) + 2 Nid + N_CP (lte_gold.c:52-93; lsym = 1 for the port-2/3 extension) */
static void gold_words_h(const oai4g_frame_parms_t *fp, uint32_t ns, uint32_t lsym, uint32_t w[14])
{
  const uint32_t Ncp = 1 - fp->Ncp, Nid = fp->Nid_cell;
  gold_seq_h(Ncp + (Nid << 1) + (((1 + (Nid << 1)) * (1 + lsym + 7 * (1 + ns))) << 10), w, 14);
}

static void lte_gold_table_h(const oai4g_frame_parms_t *fp, uint32_t t[20][2][14])
{
  for (uint32_t ns = 0; ns < 20; ns++)
    for (uint32_t l = 0; l < 2; l++) gold_words_h(fp, ns, (fp->Ncp == 0 ? 4 : 3) * l, t[ns][l]);
}

/* CRS pilot RE of port p, pilot l (0: symbol 0 of the slot, 1: symbol 4 / 3), index m
 * (lte_dl_cell_spec.c:147-200): subcarrier bin and QPSK index into qpsk[] */
static uint32_t crs_bin(const oai4g_frame_parms_t *fp, uint32_t p, uint32_t l, uint32_t m)
{
  const uint32_t nu = (p == 0) ? (l == 0 ? 0 : 3) : (l == 0 ? 3 : 0);
  uint32_t k = nu + fp->nushift;
  if (k > 5) k -= 6;
  k += fp->first_carrier_offset + 6 * m;
  if (k >= fp->ofdm_symbol_size) k = k + 1 - fp->ofdm_symbol_size;     /* DC skip */
  return k;
}
/* CRS RE of port 2/3 (4-TX extension, 36.211 6.10.1.2): symbol 1 of slot ns, nu = 3 (ns mod 2)
 * for p = 2, 3 + 3 (ns mod 2) for p = 3 */
static uint32_t crs_bin_p23(const oai4g_frame_parms_t *fp, uint32_t p, uint32_t ns, uint32_t m)
{
  uint32_t k = ((p == 2 ? 0u : 3u) + 3u * (ns & 1u) + fp->nushift) % 6u + fp->first_carrier_offset + 6 * m;
  if (k >= fp->ofdm_symbol_size) k = k + 1 - fp->ofdm_symbol_size;
  return k;
}
static uint32_t crs_qpsk(int16_t amp, uint32_t idx)
{
  const int16_t a = (int16_t)((amp * 23170) >> 15);                  /* ONE_OVER_SQRT2_Q15 */
  const int16_t re = (idx & 1) ? (int16_t)-a : a, im = (idx & 2) ? (int16_t)-a : a;
  return (uint16_t)re | ((uint32_t)(uint16_t)im << 16);
}

static bool g_init_done = false;
static int g_device = 0;                           /* the device the tables live on (do_init) */
static void do_init(void)
{
  g_init_done = true;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    snprintf(g_init_err, sizeof(g_init_err), "no HIP device available (%s)",
             e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    g_init_status = -1;
    return;
  }
  int dev = 0;
  hipGetDevice(&dev);
  g_device = dev;                                  /* every later thread binds to this device */
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    snprintf(g_init_err, sizeof(g_init_err), "device %d is not gfx950 (%s)", dev, prop.gcnArchName);
    g_init_status = -2;
    return;
  }
  g_n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  /* twiddles */
  std::vector<uint32_t> tw(2 * OAI4G_TW_TOTAL);   /* t, then the rotated companions (-t.im, t.re) */
  const int sizes[] = {4, 6, 7, 8, 9, 10, 11};
  for (int log2s : sizes) {
    int N = 1 << log2s;
    uint32_t off = oai4g_tw_offset(log2s);
    for (int m = 0; m < N; m++) {
      int16_t re, im;
      twiddle_host(N, m, &re, &im);
      tw[off + m] = (uint16_t)re | ((uint32_t)(uint16_t)im << 16);
      tw[OAI4G_TW_TOTAL + off + m] = (uint16_t)(int16_t)(-im) | ((uint32_t)(uint16_t)re << 16);
    }
  }
  std::vector<uint32_t> twf(2 * OAI4G_TW_TOTAL);  /* forward: a, then b */
  for (int log2s : sizes) {
    int N = 1 << log2s;
    uint32_t off = oai4g_tw_offset(log2s);
    for (int m = 0; m < N; m++) {
      int16_t a[2], b[2];
      dft_twiddle_ab_host(N, m, a, b);
      twf[off + m] = (uint16_t)a[0] | ((uint32_t)(uint16_t)a[1] << 16);
      twf[OAI4G_TW_TOTAL + off + m] = (uint16_t)b[0] | ((uint32_t)(uint16_t)b[1] << 16);
    }
  }
  /* Gold: x1 after 50+S l word steps; x2 step-matrix powers M2^(50+S l) (columns), S = OAI4G_GOLD_STRIDE */
  uint32_t x1 = 1u + (1u << 31), cols[32];
  for (int b = 0; b < 32; b++) cols[b] = 1u << b;
  int steps_done = 0;
  for (int l = 0; l < OAI4G_GOLD_LANES; l++) {
    int target = 50 + OAI4G_GOLD_STRIDE * l;
    while (steps_done < target) {
      uint32_t dummy = 0;
      gold_step_h(&x1, &dummy);
      for (int b = 0; b < 32; b++) {
        uint32_t z = 0;
        gold_step_h(&z, &cols[b]);
      }
      steps_done++;
    }
    h_gx1[l] = x1;
    for (int b = 0; b < 32; b++) h_gx2j[OAI4G_GOLD_LANES * b + l] = cols[b];   /* [b][lane]: coalesced */
  }
  dev_buf<uint32_t> d_tw, d_twf, d_gx1, d_gx2j;
  if (d_tw.upload(tw) != hipSuccess || d_twf.upload(twf) != hipSuccess ||
      d_gx1.upload(h_gx1, OAI4G_GOLD_LANES) != hipSuccess ||
      d_gx2j.upload(h_gx2j, OAI4G_GOLD_LANES * 32) != hipSuccess) {
    snprintf(g_init_err, sizeof(g_init_err), "device table upload failed");
    g_init_status = -3;
    return;
  }
  /* process lifetime: released, never freed (the HIP runtime may be gone when statics are destroyed) */
  g_tw = d_tw.release();
  g_twf = d_twf.release();
  g_gx1 = d_gx1.release();
  g_gx2j = d_gx2j.release();
  g_init_status = 0;
}

extern "C" int oai4g_set_device(int device)
{
  /* before the first oai4g_init: the process's rank drives `device` (one process per GPU) */
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
    set_err("set_device: device %d of %d", device, n);
    return -1;
  }
  if (g_init_done && g_device != device) {
    set_err("set_device: the library is already initialised on device %d", g_device);
    return -1;
  }
  HCK(hipSetDevice(device), -1);
  return 0;
}

/* hipSetDevice is per thread: every library call binds the calling thread to the library's device
 * before it creates streams, buffers or launches (the device tables live there).  Checked on every
 * call, not cached: the application may switch the thread's device in between (hipSetDevice,
 * torch.cuda.set_device).  The binding stays in effect after the call (include/oai4g.h).  Called by
 * NEED_INIT. */
static int bind_thread_device(void)
{
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) return -1;
  if (cur != g_device && hipSetDevice(g_device) != hipSuccess) {
    set_err("thread bind: hipSetDevice(%d) failed", g_device);
    return -1;
  }
  return 0;
}
int oai4g_bind_thread(void) { return bind_thread_device(); }

extern "C" int oai4g_init(void)
{
  pthread_once(&g_once, do_init);
  if (g_init_status != 0) {
    set_err("openair4g_amd: %s", g_init_err);
    fprintf(stderr, "[openair4g_amd] %s\n", g_err);
  }
  return g_init_status;
}

extern "C" int oai4g_device_name(char *buf, int len)
{
  if (oai4g_init() != 0) return -1;
  int dev = 0;
  hipGetDevice(&dev);
  hipDeviceProp_t prop;
  HCK(hipGetDeviceProperties(&prop, dev), -1);
  snprintf(buf, len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * per-thread scratch (drop-in path): one stream + one growable device buffer
 * ---------------------------------------------------------------------------------------- */
struct scratch_t {
  hipStream_t s = nullptr;
  uint8_t *buf = nullptr;
  size_t cap = 0;
};
static thread_local scratch_t g_scr;

static uint8_t *scratch(size_t bytes)
{
  if (!g_scr.s && hipStreamCreateWithFlags(&g_scr.s, hipStreamNonBlocking) != hipSuccess) return nullptr;
  if (bytes > g_scr.cap) {
    if (g_scr.buf) hipFree(g_scr.buf);
    size_t cap = bytes < (64u << 20) ? (64u << 20) : bytes;
    if (hipMalloc(&g_scr.buf, cap) != hipSuccess) {
      g_scr.buf = nullptr;
      g_scr.cap = 0;
      return nullptr;
    }
    g_scr.cap = cap;
  }
  return g_scr.buf;
}

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

/* The staging of one drop-in call.  Regions of the thread's scratch buffer are declared in order: add(bytes,
 * slack), where slack is what a kernel may touch past the payload (a comment names the access; where there is
 * none, the slack is what the earlier hand-written layout left there and no reader is known).  Every region
 * starts 256-byte aligned.  open() asks the thread scratch once for the total the declarations add up to, and
 * every transfer is checked against the declared sizes before it is issued; it may run on from region r into
 * the regions behind it, up to the end of region `last`.  Everything runs on g_scr.s. */
namespace {
struct stage_t {
  enum { MAX_REGIONS = 12 };
  const char *who;
  size_t off[MAX_REGIONS + 1] = {0}, len[MAX_REGIONS] = {0};
  int n = 0;
  bool full = false;
  uint8_t *buf = nullptr;

  explicit stage_t(const char *w) : who(w) {}
  int add(size_t bytes, size_t slack = 0)
  {
    if (n == MAX_REGIONS) { full = true; return 0; }        /* open() refuses */
    len[n] = bytes + slack;
    off[n + 1] = off[n] + up256(len[n]);
    return n++;
  }
  bool open()
  {
    buf = full ? nullptr : scratch(off[n]);
    if (!buf) set_err("%s: scratch allocation failed", who);
    return buf != nullptr;
  }
  template <class T = uint8_t> T *ptr(int r, size_t at = 0) const { return (T *)(buf + off[r] + at); }
  uint8_t *span(int r, size_t at, size_t bytes, int last) const      /* null (and the error set) outside the regions */
  {
    if (last < r) last = r;
    const size_t room = r >= 0 && last < n ? off[last] + len[last] - off[r] : 0;
    if (buf && at <= room && bytes <= room - at) return ptr(r, at);
    set_err("%s: transfer of %zu bytes at %zu leaves staging region %d..%d (%zu bytes)", who, bytes, at, r, last, room);
    fprintf(stderr, "[openair4g_amd] %s\n", g_err);
    return nullptr;
  }
  hipError_t up(int r, const void *src, size_t bytes, size_t at = 0, int last = -1) const
  {
    uint8_t *d = span(r, at, bytes, last);
    return d ? hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, g_scr.s) : hipErrorInvalidValue;
  }
  hipError_t down(void *dst, int r, size_t bytes, size_t at = 0, int last = -1) const
  {
    const uint8_t *d = span(r, at, bytes, last);
    return d ? hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, g_scr.s) : hipErrorInvalidValue;
  }
  hipError_t zero(int r, size_t bytes, int last) const
  {
    uint8_t *d = span(r, 0, bytes, last);
    return d ? hipMemsetAsync(d, 0, bytes, g_scr.s) : hipErrorInvalidValue;
  }
  hipError_t sync() const { return hipStreamSynchronize(g_scr.s); }
};
}  // namespace

#define NEED_INIT(ret)                                          \
  do {                                                          \
    if (oai4g_init() != 0 || bind_thread_device() != 0) return ret; \
  } while (0)

/* ------------------------------------------------------------------------------------------
 * parameter helpers (lte_parms.c, lte_mcs.c)
 * ---------------------------------------------------------------------------------------- */
extern "C" int oai4g_init_frame_parms(oai4g_frame_parms_t *fp, uint16_t N_RB_DL, uint16_t Nid_cell, uint8_t Ncp,
                                      uint8_t nb_antennas_tx, uint8_t mode1_flag, uint8_t frame_type)
{
  memset(fp, 0, sizeof(*fp));
  fp->N_RB_DL = N_RB_DL;
  fp->Nid_cell = Nid_cell;
  fp->Ncp = Ncp;
  fp->nushift = (uint8_t)(Nid_cell % 6);
  fp->nb_antennas_tx = nb_antennas_tx;
  fp->mode1_flag = mode1_flag;
  fp->frame_type = frame_type;
  uint16_t cp0 = Ncp ? 512 : 160, cp = Ncp ? 512 : 144;
  fp->symbols_per_tti = Ncp ? 12 : 14;
  int sh;
  switch (N_RB_DL) {
  case 100: fp->ofdm_symbol_size = 2048; fp->log2_symbol_size = 11; sh = 0; break;
  case 50: fp->ofdm_symbol_size = 1024; fp->log2_symbol_size = 10; sh = 1; break;
  case 25: fp->ofdm_symbol_size = 512; fp->log2_symbol_size = 9; sh = 2; break;
  case 15: fp->ofdm_symbol_size = 256; fp->log2_symbol_size = 8; sh = 3; break;
  case 6: fp->ofdm_symbol_size = 128; fp->log2_symbol_size = 7; sh = 4; break;
  default: set_err("init_frame_parms: unsupported N_RB_DL %u", N_RB_DL); return -1;
  }
  fp->samples_per_tti = 30720u >> sh;
  fp->first_carrier_offset = (uint16_t)(fp->ofdm_symbol_size - 6 * N_RB_DL);
  fp->nb_prefix_samples = (uint16_t)(cp >> sh);
  fp->nb_prefix_samples0 = (uint16_t)(cp0 >> sh);
  fp->phich_resource = 6;                 /* Ng = one (dlsim.c:138) */
  fp->phich_duration = 0;
  fp->tdd_config = 3;
  fp->nb_antennas_tx_eNB = nb_antennas_tx; /* dlsim.c:137 */
  return 0;
}

extern "C" uint8_t oai4g_get_Qm(uint8_t mcs) { return mcs < 10 ? 2 : (mcs < 17 ? 4 : 6); }

/* get_Qm_ul (lte_mcs.c:57) */
extern "C" uint8_t oai4g_get_Qm_ul(uint8_t mcs) { return mcs < 11 ? 2 : (mcs < 21 ? 4 : 6); }

/* get_I_TBS (lte_mcs.c:69-82): 36.213 Table 7.1.7.1-1 */
extern "C" uint8_t oai4g_get_I_TBS(uint8_t mcs)
{
  if (mcs < 10) return mcs;
  if (mcs == 10) return 9;
  if (mcs < 17) return (uint8_t)(mcs - 1);
  if (mcs == 17) return 15;
  return (uint8_t)(mcs - 2);
}

/* get_I_TBS_UL (lte_mcs.c:84-95): its `I_MCS == 10` branch is unreachable after `<= 10`, kept as is */
extern "C" uint8_t oai4g_get_I_TBS_UL(uint8_t mcs)
{
  if (mcs <= 10) return mcs;
  if (mcs < 21) return (uint8_t)(mcs - 1);
  return (uint8_t)(mcs - 2);
}

/* TBStable[I_TBS][N_PRB-1] (dlsch_tbs_full.h:34) in bits; 0 outside the table */
extern "C" uint32_t oai4g_tbs_bits(uint8_t I_TBS, uint16_t nb_rb)
{
  if (I_TBS > 26 || nb_rb < 1 || nb_rb > 110) return 0;
  return oai4g_tbs_by_prb[nb_rb - 1][I_TBS];
}

/* get_TBS_DL (lte_mcs.c:118-137): transport block size in BYTES (TBStable >> 3), 0 for nb_rb = 0
 * or mcs >= 29 — the reference's unit, which its callers multiply back by 8 */
extern "C" uint32_t oai4g_get_TBS_DL(uint8_t mcs, uint16_t nb_rb)
{
  if (nb_rb == 0 || mcs >= 29) return 0;
  return oai4g_tbs_bits(oai4g_get_I_TBS(mcs), nb_rb) >> 3;
}

/* get_TBS_UL (lte_mcs.c:137-155), same unit */
extern "C" uint32_t oai4g_get_TBS_UL(uint8_t mcs, uint16_t nb_rb)
{
  if (nb_rb == 0 || mcs >= 29) return 0;
  return oai4g_tbs_bits(oai4g_get_I_TBS_UL(mcs), nb_rb) >> 3;
}

static int rb_bit(const uint32_t *rb_alloc, int rb)
{
  if (rb < 32) return (rb_alloc[0] >> rb) & 1;
  if (rb < 64) return (rb_alloc[1] >> (rb - 32)) & 1;
  if (rb < 96) return (rb_alloc[2] >> (rb - 64)) & 1;
  if (rb < 100) return (rb_alloc[3] >> (rb - 96)) & 1;
  return 0;
}

/* adjust_G (lte_mcs.c:249-334) */
static int adjust_G(const oai4g_frame_parms_t *fp, const uint32_t *rb_alloc, int Qm, int subframe)
{
  if (subframe != 0 && subframe != 5 && subframe != 6) return 0;
  int re = 0, half = fp->N_RB_DL >> 1;
  if (fp->N_RB_DL & 1) {
    for (int rb = half - 3; rb <= half + 3; rb++)
      if (rb_bit(rb_alloc, rb)) re += (rb == half - 3 || rb == half + 3) ? 6 : 12;
  } else {
    for (int rb = half - 3; rb < half + 3; rb++)
      if (rb_bit(rb_alloc, rb)) re += 12;
  }
  int Ncp = fp->Ncp;
  if (subframe == 0) {
    if (fp->frame_type == 1)
      return fp->mode1_flag == 0 ? (-Ncp + 14) * re * Qm / 3 : (-Ncp + 29) * re * Qm / 6;
    return fp->mode1_flag == 0 ? (-Ncp + 17) * re * Qm / 3 : (-Ncp + 35) * re * Qm / 6;
  }
  if (subframe == 5) return (fp->frame_type == 0 ? 2 : 1) * re * Qm;
  if (subframe == 6 && fp->frame_type == 1) return re * Qm;
  return 0;
}

/* get_G (lte_mcs.c:336-368); PMCH subframes are not part of this path */
extern "C" int oai4g_get_G(const oai4g_frame_parms_t *fp, uint16_t nb_rb, const uint32_t *rb_alloc,
                           uint8_t mod_order, uint8_t Nl, uint8_t num_pdcch_symbols, int frame, uint8_t subframe)
{
  (void)frame;
  int adj = adjust_G(fp, rb_alloc, mod_order, subframe);
  int nd = fp->Ncp == 0 ? 11 : 9;
  if (fp->mode1_flag == 0) return (((int)nb_rb * mod_order * ((nd - num_pdcch_symbols) * 12 + 3 * 8)) - adj) * Nl;
  return ((int)nb_rb * mod_order * ((nd - num_pdcch_symbols) * 12 + 3 * 10)) - adj;
}

/* lte_segmentation parameter math (lte_segmentation.c:39-126) */
static int seg_params(uint32_t B, uint32_t *C, uint32_t *Cplus, uint32_t *Cminus, uint32_t *Kplus, uint32_t *Kminus,
                      uint32_t *F, uint32_t *L)
{
  uint32_t Bp;
  if (B <= 6144) { *L = 0; *C = 1; Bp = B; }
  else { *L = 24; *C = (B + (6144 - 24) - 1) / (6144 - 24); Bp = B + *C * 24; }
  if (*C > OAI4G_MAX_SEGMENTS) {
    printf("lte_segmentation.c: too many segments %u\n", *C);
    return -1;
  }
  uint32_t per = Bp / *C;
  if (per <= 40) { *Kplus = 40; *Kminus = 0; }
  else if (per <= 512) { *Kplus = (per >> 3) << 3; *Kminus = per - 8; }
  else if (per <= 1024) { *Kplus = ((per + 15) >> 4) << 4; *Kminus = *Kplus - 16; }
  else if (per <= 2048) { *Kplus = ((per + 31) >> 5) << 5; *Kminus = *Kplus - 32; }
  else if (per <= 6144) { *Kplus = ((per + 63) >> 6) << 6; *Kminus = *Kplus - 64; }
  else {
    printf("lte_segmentation.c: Illegal codeword size !!!\n");
    return -1;
  }
  if (*C == 1) { *Cplus = 1; *Kminus = 0; *Cminus = 0; }
  else { *Cminus = (*C * *Kplus - Bp) / (*Kplus - *Kminus); *Cplus = *C - *Cminus; }
  *F = *Cplus * *Kplus + *Cminus * *Kminus - Bp;
  return 0;
}

/* NULL positions of the sub-block interleaver output for block size K (by simulating
 * sub_block_interleaving_turbo on a marker input: lte_rate_matching.c:51-130) */
static const uint8_t k_colperm[32] = {0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30,
                                      1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31};
static int null_positions(uint32_t K, uint16_t *out, uint32_t maxn)
{
  uint32_t D = K + 4, R = (D + 31) >> 5, Kpi = R << 5, ND = Kpi - D;
  std::vector<uint8_t> d(96 + 3 * D + 16, 0);
  memset(d.data(), OAI4G_LTE_NULL, 96);
  uint8_t *dd = d.data() + 96;
  dd[3 * D + 2] = dd[2];
  const uint8_t *base = dd - 3 * ND;
  std::vector<uint8_t> w(3 * Kpi);
  uint32_t k = 0;
  for (uint32_t col = 0; col < 32; col++)
    for (uint32_t row = 0; row < R; row++, k++) {
      uint32_t j = k_colperm[col] + 32 * row;
      w[k] = base[3 * j];
      w[Kpi + 2 * k] = base[3 * j + 1];
      w[Kpi + 2 * k + 1] = base[3 * j + 5];
    }
  if (ND > 0) w[3 * Kpi - 1] = OAI4G_LTE_NULL;
  uint32_t n = 0;
  for (uint32_t p = 0; p < 3 * Kpi; p++)
    if (w[p] == OAI4G_LTE_NULL) {
      if (n >= maxn) return -1;
      out[n++] = (uint16_t)p;
    }
  return (int)n;
}

/* GF(2)[x] products modulo a CRC-24 polynomial (24-bit register, x^24 implicit) */
static uint32_t crc_mulmod_h(uint32_t a, uint32_t b, uint32_t poly)
{
  uint32_t r = 0;
  for (int i = 23; i >= 0; i--) {
    r <<= 1;
    if (r & 0x1000000u) r ^= 0x1000000u | poly;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}

static uint32_t crc_xpow8_h(uint64_t n, uint32_t poly)   /* x^(8n) mod P */
{
  uint32_t result = 1, base = 0x100;
  while (n) {
    if (n & 1u) result = crc_mulmod_h(result, base, poly);
    base = crc_mulmod_h(base, base, poly);
    n >>= 1;
  }
  return result;
}

/* tab[d][k][v] = (v * x^(4k)) * x^(8*per*2^d) mod P, so a*m_d = xor_k tab[d][k][nibble_k(a)] */
/* nibble tables of the two-level combine: [0][j] = x^(8 per j), [1][j] = x^(64 per j) mod P */
static void crc_mul_tables2(uint32_t per, uint32_t poly, uint32_t (*tab)[8][96])
{
  for (int lv = 0; lv < 2; lv++)
    for (uint32_t j = 0; j < 8; j++) {
      const uint32_t m = crc_xpow8_h((uint64_t)per * j * (lv ? 8u : 1u), poly);
      for (int k = 0; k < 6; k++)
        for (uint32_t v = 0; v < 16; v++) tab[lv][j][16 * k + v] = crc_mulmod_h((v << (4 * k)) & 0xffffffu, m, poly);
    }
}

static void crc_mul_tables(uint32_t per, int levels, uint32_t poly, uint32_t (*tab)[6][16])
{
  for (int d = 0; d < levels; d++) {
    uint32_t m = crc_xpow8_h((uint64_t)per << d, poly);
    for (int k = 0; k < 6; k++)
      for (uint32_t v = 0; v < 16; v++) tab[d][k][v] = crc_mulmod_h((v << (4 * k)) & 0xffffffu, m, poly);
  }
}

/* QAM tables (dlsch_modulation.c:79-103, 1223-1246).  The raw tables are int (LTE_TRANSPORT/
 * vars.h:72): the outer 64-QAM level 35393 exceeds int16 and is only narrowed after the scaling. */
/* `alamouti` also serves the single-layer precoding modes 3..8 (:753, :758-770, :801-802, :851-852), whose
 * arithmetic is the same: amp' = (amp_rho 23170) >> 15, a QAM level (amp' raw table) >> 15 on antenna 0
 * and its exact rotation on antenna 1; a QPSK component +-g rotated first and scaled after,
 * (+-g 23170) >> 15, so its two levels are kept apart (the negative one is the floor, not the negation) */
static void qam_tables_scaled(int Qm, int16_t amp, int16_t srho_a, int16_t srho_b, bool alamouti, cw_dev_t &c)
{
  int32_t q16[4], q64[8];
  for (int a = -1; a <= 1; a += 2)
    for (int b = -1; b <= 1; b += 2) {
      q16[(1 + a) + (1 + b) / 2] = -a * (20724 + b * 10362);
      for (int cc = -1; cc <= 1; cc += 2)
        q64[(1 + a) * 2 + (1 + b) + (1 + cc) / 2] = -a * (20225 + b * (10112 + cc * 5056));
    }
  int16_t amp_a = (int16_t)(((int32_t)amp * srho_a) >> 13), amp_b = (int16_t)(((int32_t)amp * srho_b) >> 13);
  c.qpsk_a = (int16_t)((amp_a * 23170) >> 15);
  c.qpsk_b = (int16_t)((amp_b * 23170) >> 15);
  /* ALAMOUTI normalises for two antennas: amp/sqrt2 times the raw table (:364, :398-399) */
  const int16_t sa = alamouti ? (int16_t)(((int32_t)amp_a * 23170) >> 15) : amp_a;
  const int16_t sb = alamouti ? (int16_t)(((int32_t)amp_b * 23170) >> 15) : amp_b;
  for (int i = 0; i < 8; i++) {
    const int32_t v = Qm == 4 ? q16[i & 3] : q64[i];
    c.qam_a[i] = (int16_t)((v * sa) >> 15);
    c.qam_b[i] = (int16_t)((v * sb) >> 15);
  }
  /* ALAMOUTI QPSK (:371-386): +-gain, then * ONE_OVER_SQRT2_Q15 >> 15 */
  const int16_t g[2] = {c.qpsk_a, c.qpsk_b};
  for (int pil = 0; pil < 2; pil++) {
    c.alm_qpsk[pil][0] = (int16_t)(((int32_t)g[pil] * 23170) >> 15);
    c.alm_qpsk[pil][1] = (int16_t)(((int32_t)(int16_t)-g[pil] * 23170) >> 15);
  }
}

/* ------------------------------------------------------------------------------------------
 * Range check for k_modofdm's no-saturation IDFT forms (ibfly4_shr1_ns and r4inv<NS>,
 * oai4g_dft_prims.h).  The 2048-point transform is DIT: a 64-level value (before its >> 3) is part
 * of a 64-point DFT over the subcarriers of one residue class mod 32, a 256-level value one of a
 * 256-point DFT over a class mod 8 scaled by 1/8 (the 64-level's shift), a 1024-level value one over
 * a class mod 2 scaled by 1/16, a 2048-level sum (before mulhi) one over every subcarrier scaled by
 * 1/32; the leaf's are parts of 16-point DFTs, inside the 64-level's classes.
 * Every twiddle has modulus < 1 (Q15, |t| <= 32767.7), so a value's modulus is at most (occupied
 * subcarriers of its class) x (largest input modulus) x scale, plus the truncations of the levels
 * below (< 64 in modulus).  Every transform input is a QAM word (TM1), a sign-flipped / swapped one
 * (ALAMOUTI), a QAM word and its rotation by 1, -1, j or -j (single-layer precoding: one word per RE
 * and antenna from the same tables, so V and the bounds are ALAMOUTI's), a CDD pair (floor((x0 + x1) / 2), +-floor((x0 - x1) / 2)) of two (LARGE_CDD) or a halved
 * one (4-port CDD): components <= the largest level V of the configuration's QAM / QPSK tables,
 * modulus <= sqrt(2) V, and only 12 N_RB_DL subcarriers carry anything.  When the four bounds stay inside
 * int16 with a margin of 128, no add of those levels saturates or wraps, packs_epi32 never clamps
 * and no operand is -32768, whatever the bits: the no-saturation forms are then the reference's
 * arithmetic.  (C3: V = 553, R = 782.1; 39 R + 128 = 30629, 151 R / 8 + 128 = 14890, 601 R / 16 +
 * 128 = 29505, 1201 R / 32 + 128 = 29480.)  With CRS or static REs (PCFICH, PDCCH, PHICH, PSS, SSS,
 * PBCH) in the grid, V also covers their components (v_static: the largest over the CRS table and the
 * static-RE table, re-checked whenever oai4g_tx_config_set_control / _set_common rebuild it).
 * OAI4G_MOD_SAT (test hook) keeps the saturating forms.
 * ---------------------------------------------------------------------------------------- */
static uint32_t mod_nosat_ok(const cfg_dev_t &h, int v_static)
{
  if (h.log2N != 11 || h.nsymb != 14 || getenv("OAI4G_MOD_SAT")) return 0;
  int v = v_static;
  for (uint32_t cw = 0; cw < h.n_cw; cw++) {
    const cw_dev_t &c = h.cw[cw];
    for (int i = 0; i < 8; i++) v = std::max(v, std::max(std::abs((int)c.qam_a[i]), std::abs((int)c.qam_b[i])));
    v = std::max(v, std::max(std::abs((int)c.qpsk_a), std::abs((int)c.qpsk_b)));
    for (int i = 0; i < 2; i++)
      v = std::max(v, std::max(std::abs((int)c.alm_qpsk[i][0]), std::abs((int)c.alm_qpsk[i][1])));
  }
  const double R = std::sqrt(2.0) * v, band = 12.0 * h.N_RB_DL;
  const double c32 = std::ceil(band / 32) + 1, c8 = std::ceil(band / 8) + 1, c2 = std::ceil(band / 2) + 1;
  return (c32 * R + 128 <= 32767 && c8 * R / 8 + 128 <= 32767 && c2 * R / 16 + 128 <= 32767 &&
          (band + 1) * R / 32 + 128 <= 32767) ? 1u : 0u;
}

static int packed_iq_max(const std::vector<uint32_t> &t)
{
  int v = 0;
  for (uint32_t w : t) v = std::max(v, std::max(std::abs((int)(int16_t)(w & 0xFFFFu)), std::abs((int)(int16_t)(w >> 16))));
  return v;
}

/* k_modofdm's dense item space (oai4g_internal.h oai4g_mod_item): mod_lz = the leading symbols that are
 * empty at every subframe index: no data REs, in a grid without static REs.  With CRS (symbol 0 carries
 * it) or the static REs of set_control / set_common (a PCFICH sits in symbol 0) it is 0, and the kernels
 * for such grids are compiled for that; re-run wherever those change. */
static void mod_items_setup(cfg_dev_t &h)
{
  uint32_t lz = 0;
  if (!h.with_crs && !h.ctl_on)
    for (; lz < OAI4G_MOD_LZ_MAX && lz + 1 < h.nsymb / 2; lz++) {
      bool empty = true;
      for (int sf = 0; sf < 10 && empty; sf++) empty = h.symnre[sf][lz] == 0;
      if (!empty) break;
    }
  h.mod_lz = lz;
  h.mod_per = h.nsymb - lz;
  h.mod_permag = oai4g_mod_permag(h.mod_per);
}

/* the item map as k_modofdm and its launch use it (include/oai4g.h).  Plain host arithmetic, no device. */
extern "C" int oai4g_mod_item_map(uint32_t item, uint32_t ips, uint32_t lz, uint32_t per, uint32_t *sf, uint32_t *l,
                                  uint32_t *pair)
{
  if (ips < 1 || ips > 2 || per < 1 || lz > OAI4G_MOD_LZ_MAX) return -1;
  const oai4g_mod_item_t m = oai4g_mod_item(item, ips, lz, per, oai4g_mod_permag(per));
  *sf = m.sf;
  *l = m.l;
  *pair = m.pair;
  return m.l == lz && lz > 0 ? 1 : 0;
}

/* test hook: at most n workgroups in k_modofdm's persistent grid (0: the occupancy default) */
int g_modofdm_grid_cap = 0;
extern "C" void oai4g_set_modofdm_grid_cap(int n_workgroups) { g_modofdm_grid_cap = n_workgroups > 0 ? n_workgroups : 0; }

/* get_pmi (dlsch_modulation.c:1136-1178).  The reference widens its uint16_t pmi_alloc to uint32_t and
 * shifts: a shift of 16 or more (subband 8 at 50 PRB, 8..12 at 100 PRB) reads 0. */
extern "C" uint8_t oai4g_get_pmi(uint8_t N_RB_DL, uint8_t mimo_mode, uint16_t pmi_alloc, uint16_t rb)
{
  const uint32_t sb = N_RB_DL == 6 ? rb : N_RB_DL == 50 ? rb / 6u : N_RB_DL == 100 ? rb >> 3 : rb >> 2;
  const uint32_t two = mimo_mode <= OAI4G_PUSCH_PRECODING1, sh = two ? sb << 1 : sb;
  return sh >= 32 ? 0 : (uint8_t)(((uint32_t)pmi_alloc >> sh) & (two ? 3u : 1u));
}

/* ------------------------------------------------------------------------------------------
 * RE map: restatement of dlsch_modulation's control flow (dlsch_modulation.c:1258-1493 and
 * allocate_REs_in_RB :139-249, 745-748) producing, per symbol, the data-RE order.
 * Returns REs allocated, or -1 for an unsupported mode.
 * ---------------------------------------------------------------------------------------- */
static int not_pilot(int pilots, int re, int nushift, int use2nd)
{
  int off = (pilots == 2) ? 3 : 0, v = nushift % 3;
  if (pilots == 0) return 1;
  if (use2nd) return (re != nushift + off) && (re != ((nushift + 6 + off) % 12));
  return (re != v) && (re != v + 6) && (re != v + 3) && (re != v + 9);
}

static int build_remap(const oai4g_frame_parms_t *fp, const uint32_t *rb_alloc, int num_pdcch, int subframe,
                       int mimo_mode, uint16_t pmi_alloc, uint16_t *remap /* [14][N] */, uint32_t *symbase /* [14] */,
                       int *re_alloc /* the reference's re_allocated */)
{
  const bool alm = mimo_mode == OAI4G_ALAMOUTI, prec1 = oai4g_mode_prec1((uint32_t)mimo_mode);
  int ralloc = 0;
  int N = fp->ofdm_symbol_size, nsymb = fp->Ncp == 0 ? 14 : 12, half = fp->N_RB_DL >> 1;
  int use2nd = fp->mode1_flag == 1;
  for (int i = 0; i < 14 * N; i++) remap[i] = 0xFFFF;
  uint32_t total = 0;
  for (int l = 0; l < 14; l++) symbase[l] = 0;
  for (int l = num_pdcch; l < nsymb; l++) {
    symbase[l] = total;
    uint32_t idx = 0;
    int pilots;
    if (fp->Ncp == 0) pilots = (l == 4 || l == 11) ? 2 : (l == 7 ? 1 : 0);
    else pilots = (l == 3 || l == 9) ? 2 : (l == 6 ? 1 : 0);
    if (fp->nb_antennas_tx == 4 && l % (nsymb >> 1) == 1) pilots = 3;   /* port-2/3 CRS (4-TX extension) */
    int re_offset = fp->first_carrier_offset;
    for (int rb = 0; rb < fp->N_RB_DL; rb++) {
      int alloc = rb_bit(rb_alloc, rb), skip_half = 0, skip_dc = 0;
      if (fp->N_RB_DL & 1) {
        skip_dc = (rb == half);
        if (subframe == 0 && rb > half - 3 && rb < half + 3 && l >= (nsymb >> 1) && l < (nsymb >> 1) + 4) alloc = 0;
        if (subframe == 0 && rb == half - 3 && l >= (nsymb >> 1) && l < (nsymb >> 1) + 4) skip_half = 1;
        else if (subframe == 0 && rb == half + 3 && l >= (nsymb >> 1) && l < (nsymb >> 1) + 4) skip_half = 2;
        if (fp->frame_type == 1) {
          if ((subframe == 0 || subframe == 5) && rb > half - 3 && rb < half + 3 && l == nsymb - 1) alloc = 0;
          if ((subframe == 0 || subframe == 5) && rb == half - 3 && l == nsymb - 1) skip_half = 1;
          else if ((subframe == 0 || subframe == 5) && rb == half + 3 && l == nsymb - 1) skip_half = 2;
          if ((subframe == 1 || subframe == 6) && rb > half - 3 && rb < half + 3 && l == 2) alloc = 0;
          if ((subframe == 1 || subframe == 6) && rb == half - 3 && l == 2) skip_half = 1;
          else if ((subframe == 1 || subframe == 6) && rb == half + 3 && l == 2) skip_half = 2;
        } else {
          int ls = (nsymb >> 1) - 1, lp = (nsymb >> 1) - 2;
          if ((subframe == 0 || subframe == 5) && rb > half - 3 && rb < half + 3 && l == ls) alloc = 0;
          if ((subframe == 0 || subframe == 5) && rb == half - 3 && l == ls) skip_half = 1;
          else if ((subframe == 0 || subframe == 5) && rb == half + 3 && l == ls) skip_half = 2;
          if ((subframe == 0 || subframe == 5) && rb > half - 3 && rb < half + 3 && l == lp) alloc = 0;
          if ((subframe == 0 || subframe == 5) && rb == half - 3 && l == lp) skip_half = 1;
          else if ((subframe == 0 || subframe == 5) && rb == half + 3 && l == lp) skip_half = 2;
        }
      } else {
        if (subframe == 0 && rb >= half - 3 && rb < half + 3 && l >= (nsymb >> 1) && l < (nsymb >> 1) + 4) alloc = 0;
        if (fp->frame_type == 1) {
          if ((subframe == 0 || subframe == 5) && rb >= half - 3 && rb < half + 3 && l == nsymb - 1) alloc = 0;
          if ((subframe == 1 || subframe == 6) && rb >= half - 3 && rb < half + 3 && l == 2) alloc = 0;
        } else {
          if ((subframe == 0 || subframe == 5) && rb >= half - 3 && rb < half + 3 && l == (nsymb >> 1) - 2) alloc = 0;
          if ((subframe == 0 || subframe == 5) && rb >= half - 3 && rb < half + 3 && l == (nsymb >> 1) - 1) alloc = 0;
        }
      }
      if (alloc) {
        int first = 0, last = 12, re_off = re_offset, par = 0;
        if (skip_half == 1) last = 6;
        else if (skip_half == 2) first = 6;
        for (int re = first; re < last; re++) {
          if (skip_dc && re == 6) re_off = re_off - N + 1;
          if (!not_pilot(pilots, re, fp->nushift, use2nd)) continue;
          int k = re_off + re;
          if (k < 0 || k >= N) return -1;
          if (alm) {
            /* ALAMOUTI pair (:362-546, :868-876): symbols 2i, 2i+1 at RE n and its partner, the
             * next carrier or the one after when that is a pilot (linear grid index); code =
             * 2i | role.  A partner outside this symbol's row or on an RE that is written twice
             * would need accumulation: not produced by any supported grid, rejected here. */
            int k2 = k + (not_pilot(pilots, re + 1, fp->nushift, use2nd) ? 1 : 2);
            if (k2 >= N || remap[l * N + k] != 0xFFFF || remap[l * N + k2] != 0xFFFF) return -1;
            remap[l * N + k] = (uint16_t)idx;
            remap[l * N + k2] = (uint16_t)(idx | 1u);
            idx += 2;
            ralloc += 2;
            re++;
            if (!not_pilot(pilots, re, fp->nushift, use2nd)) {
              re++;
              ralloc++;          /* the reference also counts the pilot it steps over */
            }
            continue;
          }
          /* single-layer precoding: the RB's precoder (:1461) instead of the CDD parity */
          if (prec1)
            remap[l * N + k] = (uint16_t)(idx | ((uint32_t)oai4g_get_pmi(fp->N_RB_DL, (uint8_t)mimo_mode, pmi_alloc, (uint16_t)rb)
                                                 << OAI4G_MOD_PMI_SHIFT));
          else
            remap[l * N + k] = (uint16_t)(idx | (par << 15));
          idx++;
          ralloc++;
          par ^= 1;
        }
      }
      re_offset += 12;
      if (re_offset >= N) re_offset = skip_dc == 0 ? 1 : 7;
    }
    total += idx;
  }
  if (re_alloc) *re_alloc = ralloc;
  return (int)total;
}

/* ------------------------------------------------------------------------------------------
 * configuration
 * ---------------------------------------------------------------------------------------- */
struct oai4g_tx_config {
  oai4g_tx_params_t p;
  oai4g_frame_parms_t fp;
  cfg_dev_t h;                      /* host mirror */
  dev_buf<cfg_dev_t> d;             /* device copy */
  dev_buf<uint16_t> d_remap;
  std::vector<uint16_t> h_remap;
  dev_buf<uint32_t> d_gold;             /* [10][n_cw][ebits_words] scrambling words */
  dev_buf<enc_rv_tab_t> d_rvtab;        /* [4][n_cw] per-rv plan tables (oai4g_tx_config_enable_tb_rv), else empty */
  /* build_stat_tm's inputs (host only) */
  std::vector<uint32_t> h_crs;          /* [10][6][200] packed CRS IQ of pilot entry i, index m (empty without CRS) */
  std::vector<uint32_t> h_ctl;          /* [10][14][ctl_planes][N] packed IQ of the static REs of set_control /
                                           set_common per antenna (empty without them) */
  uint32_t ctl_planes = 2;              /* 2, or the TX antennas when there are more */
  dev_buf<uint32_t> d_stat;             /* cfg_dev_t::stat_tm */
  int ctl_vmax = 0;                     /* largest I / Q magnitude in the static-RE table (mod_nosat_ok) */
  std::vector<oai4g_dci_alloc_t> dci;   /* oai4g_tx_config_set_control's DCI set */
  uint8_t n_ue_dci = 0, n_common_dci = 0;
  bool common_on = false;
  oai4g_common_sig_t common;            /* oai4g_tx_config_set_common's signals */
  int re_count[10];
  int re_alloc[10];                 /* dlsch_modulation's return value (ALAMOUTI counts skipped pilots) */
  /* optional pipelined batches (OAI4G_PIPE_CHUNK=n): the encoder runs on the caller's stream, the
   * modulator/IDFT on s_mod, chunk by chunk.  Off by default: measured slower on MI355X than the
   * serial pair (the persistent modulator grid already fills every CU). */
  hipStream_t s_mod = nullptr;
  hipEvent_t ev_enc[OAI4G_PIPE_MAX_CHUNKS] = {};
  hipEvent_t ev_done = nullptr;
  int pipe_chunk = 0;
  ~oai4g_tx_config()
  {
    for (auto &e : ev_enc)
      if (e) hipEventDestroy(e);
    if (ev_done) hipEventDestroy(ev_done);
    if (s_mod) hipStreamDestroy(s_mod);
  }
};

/* The sub-block interleaver + rate matcher plan of block size ki (k_encode phase 4;
 * lte_rate_matching.c:51-130, 464-566).  Tile t: v0 tiles cover 32 rows of y0, interlaced tiles 16
 * rows of y1 / y2 alternating per lane (lane 2i: y1 row, 2i + 1: y2 row, shifted by one for the
 * (pi(k) + 1) mod Kpi rule).  After the half-wave's 32x32 transpose lane c holds matrix column c =
 * w column bitrev5(c), rows of the tile: its NULLs (row 0 of the column) lead the run, and the
 * run's place in the NULL-free circular buffer is closed-form. */
static void rm_plan(cw_dev_t &c, int ki)
{
  const uint32_t R = c.Rk[ki], ND = c.NDk[ki], Ncb = c.Ncbk[ki], Nnn = c.Nnnk[ki], k0c = c.k0ck[ki];
  const uint32_t tz = c.t0k[ki], nt = c.ntk[ki], sw = c.stream_words;
  memset(c.rm_dst[ki], 0, sizeof(c.rm_dst[ki]));
  c.rm_wrapt[ki] = ~0u;
  for (uint32_t t = 0; t <= OAI4G_RM_TILES; t++)
    for (uint32_t L = 0; L < 32; L++) c.rm_src[ki][t][L] = 1u << 5;   /* idle: word 0 of stream 0 */
  for (uint32_t t = 0; t < nt; t++) {
    const bool il = t >= tz;
    const uint32_t rb = il ? t - tz : t;
    for (uint32_t L = 0; L < 32; L++) {
      /* source: row of the tile this lane loads */
      const uint32_t row = il ? 16 * rb + (L >> 1) : 32 * rb + L, s = il ? 1 + (L & 1) : 0;
      if (row < R) {
        const int pos = (int)(32 * row) - (int)ND + (s == 2 ? 1 : 0);     /* >= -32 */
        const uint32_t wrel = (uint32_t)((int)(s * sw) + (pos >> 5) + 1);
        c.rm_src[ki][t][L] = ((uint32_t)pos & 31u) | (wrel << 5) | (s == 2 && row == R - 1 ? OAI4G_RM_SRC_LAST : 0u);
      }   /* past the last row: the idle word (any bits, beyond the run) */
      /* destination: the run of matrix column L = w column wc */
      uint32_t wc = 0;
      for (int b = 0; b < 5; b++) wc |= ((L >> b) & 1u) << (4 - b);
      uint32_t b0 = 0, b1 = 0;           /* NULL-headed w columns before wc in v0 / v1, v2 */
      for (uint32_t w2 = 0; w2 < wc; w2++) {
        uint32_t p2 = 0;
        for (int b = 0; b < 5; b++) p2 |= ((w2 >> b) & 1u) << (4 - b);
        b0 += p2 < ND ? 1u : 0u;
        b1 += p2 + 1 < ND ? 1u : 0u;
      }
      const uint32_t z0 = L < ND ? 1u : 0u, z1 = z0 + (L + 1 < ND ? 1u : 0u);
      const uint32_t zc = il ? z1 : z0;
      const uint32_t cs = il ? 32 * R - ND + 2 * wc * R - b0 - b1 : wc * R - b0;   /* compact index of the column's first entry */
      const uint32_t pc = il ? 32 * R + 2 * wc * R : wc * R;                       /* w position of the column start */
      const int left = il ? 2 * ((int)R - 16 * (int)rb) : (int)R - 32 * (int)rb;
      int n = left < 32 ? left : 32;
      if (il && L == 31 && ND > 0 && left <= 32 && n) n--;                         /* w[3Kpi-1] is NULL */
      const uint32_t z = rb ? 0u : zc, ci0 = rb ? cs + 32 * rb - zc : cs, p0 = pc + 32 * rb;
      const int m = p0 + (uint32_t)n > Ncb ? (int)Ncb - (int)(p0 + z) : n - (int)z;   /* limited buffer */
      if (m <= 0) continue;
      uint32_t o = ci0 + Nnn - k0c;
      o = o >= Nnn ? o - Nnn : o;
      c.rm_dst[ki][t][L] = o | (z << 16) | ((uint32_t)m << 21) | (o + (uint32_t)m > Nnn ? OAI4G_RM_DST_WRAP : 0u);
      /* runs are disjoint intervals of the circular buffer, so at most one straddles its end; ~1
       * (never expected) sends the encoder down its general placement path */
      if (o + (uint32_t)m > Nnn) c.rm_wrapt[ki] = c.rm_wrapt[ki] == ~0u || c.rm_wrapt[ki] == t ? t : ~1u;
    }
  }
  /* test hook: OAI4G_ENC_GENERAL_RM set sends every block size down the encoder's general placement
   * path (the ~1 plan), which no LTE geometry reaches by itself (tests/test_gpu_rm_paths.py) */
  if (getenv("OAI4G_ENC_GENERAL_RM")) c.rm_wrapt[ki] = ~1u;
}

/* k_encode phase 4's tile-pair schedule (include/oai4g.h).  Plain host arithmetic, no device. */
extern "C" int oai4g_rm_pair_schedule(uint32_t C, uint32_t n0, const uint32_t nt[2], const uint32_t wrapt[2],
                                      uint32_t *pairs, uint32_t *pair0)
{
  if (C < 1 || C > OAI4G_MAX_CB || n0 > C) return -1;
  for (uint32_t ki = 0; ki < 2; ki++)
    if ((ki ? n0 < C : n0 > 0) && (nt[ki] < 1 || nt[ki] > OAI4G_RM_TILES)) return -1;
  uint32_t n = 0;
  for (uint32_t r = 0; r < C; r++) {
    const uint32_t ki = r >= n0 ? 1u : 0u, pp = (nt[ki] + 1) / 2;
    pair0[r] = n;
    for (uint32_t p = 0; p < pp; p++) {
      const uint32_t t0 = 2 * p, row = ki * ((OAI4G_RM_TILES + 1) * 32) + t0 * 32;   /* plan-row word offset */
      const uint32_t wrap = wrapt[ki] - t0 < 2u ? 1u : 0u;                           /* t0 or t0 + 1 (not ~0, ~1) */
      pairs[n++] = wrap | (ki << 1) | (r << 2) | ((4 * row) << 16);
    }
  }
  pair0[C] = n;
  return (int)n;
}

/* k_encode phase 3a's 32-fold: predicate and table for block size K (include/oai4g.h).  Plain host
 * arithmetic, no device. */
extern "C" int oai4g_qpp_fold32(uint32_t K, uint32_t *s_out, uint16_t *tab)
{
  const int qi = oai4g_qpp_index(K);
  if (qi < 0 || oai4g_qpp_table[qi].K != K) return -1;
  if (K & 1023u) return 0;                 /* rows of a 32 x 32 tile must be aligned words: 32 | Q */
  const uint64_t f1 = oai4g_qpp_table[qi].f1, f2 = oai4g_qpp_table[qi].f2;
  const uint32_t Q = K >> 5;
  auto pi = [&](uint64_t k) { return (uint32_t)((f1 * k + f2 * k * k) % K); };
  const uint32_t d = (pi(Q) + K - pi(0)) % K;
  if (d % Q) return 0;
  const uint32_t s = d / Q;
  if (!(s & 1u)) return 0;
  for (uint32_t k = 0; k < K; k++)
    if ((pi(k + Q) + K - pi(k)) % K != d) return 0;
  uint32_t si = 1;                          /* s^-1 mod 32 */
  while (((si * s) & 31u) != 1u) si += 2;
  *s_out = s;
  for (uint32_t k = 0; k < Q; k++) {
    const uint32_t x = pi(k);
    tab[k] = (uint16_t)(((x % Q) << 7) | ((si * (x / Q)) & 31u));
  }
  return 1;
}

/* what the reference prints where Ncb < Kw before its rate matcher returns 0 (lte_rate_matching.c:518-521) */
static void rm_condition_exit(const rm_ncb_t &g, uint32_t Nsoft)
{
  printf("Exiting, RM condition (Nir %u, Nsoft %u, Kw %u\n", g.Nir, Nsoft, g.Kw);
}

/* Compacted start of the circular buffer w[0..Ncb) of a block with R rows and the NULL list of size
 * index ki, for redundancy version rv (lte_rate_matching.c:523-524): k0 less the NULLs below it */
static uint32_t rm_k0c_of_rv(const cw_dev_t &c, uint32_t ki, uint32_t R, uint32_t Ncb, uint32_t rv)
{
  return rm_compact(rm_k0(R, Ncb, rv), rm_null_list{c.nullpos[ki], c.nnull[ki]});
}

static int derive_cfg(oai4g_tx_config *cfg, const oai4g_tx_params_t *p, const uint8_t Nl[2], bool need_remap,
                      int only_sf)
{
  memset(&cfg->h, 0, sizeof(cfg->h));
  cfg->p = *p;
  oai4g_frame_parms_t &fp = cfg->fp;
  if (oai4g_init_frame_parms(&fp, p->N_RB_DL, p->Nid_cell, p->Ncp, p->nb_antennas_tx, p->mode1_flag,
                             p->frame_type) != 0)
    return -1;
  cfg_dev_t &h = cfg->h;
  if (p->n_cw < 1 || p->n_cw > 2) { set_err("n_cw must be 1 or 2"); return -1; }
  const bool prec1 = oai4g_mode_prec1(p->mimo_mode);
  if (p->mimo_mode != OAI4G_SISO && p->mimo_mode != OAI4G_LARGE_CDD && p->mimo_mode != OAI4G_ALAMOUTI && !prec1) {
    set_err("mimo_mode %u not supported (SISO, ALAMOUTI, LARGE_CDD and the single-layer precoding modes 3..8)", p->mimo_mode);
    return -1;
  }
  if (prec1 && (p->n_cw != 1 || p->nb_antennas_tx > 2)) {
    set_err("single-layer precoding (mimo_mode %u) takes one codeword and at most 2 TX antennas (dlsch_modulation.c:750)",
            p->mimo_mode);
    return -1;
  }
  if (p->pmi_alloc > 0xFFFFu) { set_err("pmi_alloc %#x: only the low 16 bits may be set", p->pmi_alloc); return -1; }
  if (p->mimo_mode == OAI4G_ALAMOUTI && (p->nb_antennas_tx != 2 || p->n_cw != 1)) {
    set_err("ALAMOUTI requires 2 TX antennas and one codeword (dlsch_modulation.c:362)");
    return -1;
  }
  if (p->mimo_mode == OAI4G_LARGE_CDD && ((p->nb_antennas_tx != 2 && p->nb_antennas_tx != 4) || p->n_cw != 2)) {
    set_err("LARGE_CDD requires 2 (dlsch_modulation.c:551) or 4 (C4 extension) TX antennas and 2 codewords");
    return -1;
  }
  if (p->nb_antennas_tx == 4 && p->mimo_mode != OAI4G_LARGE_CDD) {
    set_err("4 TX antennas: LARGE_CDD only (C4 extension)");
    return -1;
  }
  if (p->payload_stride % 4) { set_err("payload_stride must be a multiple of 4"); return -1; }
  h.N_RB_DL = fp.N_RB_DL;
  h.N = fp.ofdm_symbol_size;
  h.log2N = fp.log2_symbol_size;
  h.cp0 = fp.nb_prefix_samples0;
  h.cp = fp.nb_prefix_samples;
  h.spt = fp.samples_per_tti;
  h.nsymb = fp.symbols_per_tti;
  h.n_ant = fp.nb_antennas_tx;
  h.first_carrier = fp.first_carrier_offset;
  h.n_cw = p->n_cw;
  h.mimo_mode = p->mimo_mode;
  h.num_pdcch = p->num_pdcch_symbols;
  h.rnti = p->rnti;
  h.Nid_cell = p->Nid_cell;
  h.first_sf = p->first_subframe % 10;
  h.sf_step = p->subframe_step;
  h.payload_stride = p->payload_stride;
  for (uint32_t v = 0; v < 256; v++) {            /* crc_byte.c:98-105 */
    uint32_t ra = v << 16, rb = v << 16;
    for (int i = 0; i < 8; i++) {
      ra = (ra & 0x800000u) ? ((ra << 1) ^ 0x864cfbu) & 0xffffffu : (ra << 1) & 0xffffffu;
      rb = (rb & 0x800000u) ? ((rb << 1) ^ 0x800063u) & 0xffffffu : (rb << 1) & 0xffffffu;
    }
    h.crctab[0][v] = ra;
    h.crctab[1][v] = rb;
  }
  uint32_t max_tb_words = 0, max_stream_words = 0, max_gw = 0, max_bits = 0, max_w = 0, max_inw = 0;
  bool rm_fail = false;
  for (int cw = 0; cw < p->n_cw; cw++) {
    cw_dev_t &c = h.cw[cw];
    c.TBS = p->TBS[cw];
    if (c.TBS == 0 || (c.TBS & 7)) { set_err("TBS[%d]=%u must be a positive multiple of 8", cw, c.TBS); return -1; }
    c.A_bytes = c.TBS >> 3;
    if (p->payload_stride < ((c.A_bytes + 3) & ~3u)) {
      set_err("payload_stride %u < TBS/8 rounded to 4 (%u)", p->payload_stride, (c.A_bytes + 3) & ~3u);
      return -1;
    }
    c.Qm = oai4g_get_Qm(p->mcs[cw]);
    c.q = p->q[cw];
    uint32_t C, Cp, Cm, Kp, Km, F, L;
    if (seg_params(c.TBS + 24, &C, &Cp, &Cm, &Kp, &Km, &F, &L) < 0) { set_err("segmentation failed"); return -1; }
    c.C = C; c.Cminus = Cm; c.Kplus = Kp; c.Kminus = Km; c.F = F; c.L = L;
    uint32_t src = 0, maxK = 0;
    for (uint32_t r = 0; r < C; r++) {
      uint32_t K = r < Cm ? Km : Kp;
      int qi = oai4g_qpp_index(K);
      if (qi < 0) { set_err("illegal code block size %u", K); return -1; }
      c.K[r] = K;
      c.f1[r] = oai4g_qpp_table[qi].f1;
      c.f2[r] = oai4g_qpp_table[qi].f2;
      c.fill[r] = r == 0 ? F / 8 : 0;
      c.ncopy[r] = (K - L) / 8 - c.fill[r];
      c.src[r] = src;
      src += c.ncopy[r];
      maxK = K > maxK ? K : maxK;
      /* rate matching geometry */
      uint32_t D = K + 4, R = (D + 31) >> 5, Kpi = R << 5;
      c.R[r] = R; c.Kpi[r] = Kpi; c.ND[r] = Kpi - D;
      const rm_ncb_t g = rm_ncb(OAI4G_NSOFT, p->Kmimo, p->Mdlharq, C, R);
      c.Ncb[r] = g.Ncb;
      if (g.shorter && !p->rm_limited_buffer) {
        rm_condition_exit(g, OAI4G_NSOFT);
        set_err("RM condition: Ncb %u < Kw %u (the reference emits E=0, lte_rate_matching.c:518-521)", g.Ncb, g.Kw);
        rm_fail = true;
        c.Ncb[r] = g.Kw;
      }   /* else (opt-in): the circular buffer is w[0..Ncb), 36.212 5.1.4.1.2 */
      c.kidx[r] = (C > 1 && r < Cm) ? 0 : 1;
    }
    if (src != (c.TBS + 24) / 8) { set_err("segmentation byte accounting mismatch"); return -1; }
    /* QPP walk tables per block size (Kminus list 0, Kplus list 1) and interleaved-word offsets */
    for (int ki = 0; ki < 2; ki++) {
      uint32_t K = ki == 0 ? Km : Kp;
      if (K == 0 || (ki == 0 && !(C > 1 && Cm > 0))) continue;
      int qi = oai4g_qpp_index(K);
      uint64_t f1 = oai4g_qpp_table[qi].f1, f2 = oai4g_qpp_table[qi].f2;
      for (uint32_t j = 0; j < (K + 31) / 32; j++) {   /* k = 8j < K/4: walk starts of the quarter fold */
        uint64_t k = 8 * j;
        uint32_t pi = (uint32_t)((f1 * k + f2 * k * k) % K), pi1 = (uint32_t)((f1 * (k + 1) + f2 * (k + 1) * (k + 1)) % K);
        c.qpp0[ki][j] = pi | (((pi1 + K - pi) % K) << 16);
      }
      memset(c.qpp_tab[ki], 0, sizeof(c.qpp_tab[ki]));
      /* entry k: plane word xp/8 (bits 7-14) and the rotate (bits 0-4) that lands bit (8u + xp%8) of
       * it at bit k%8 of each byte (the walk's step index is folded into the rotate, so the kernel
       * needs no shift) */
      for (uint64_t k = 0; k < K / 4; k++) {
        const uint32_t x = (uint32_t)((f1 * k + f2 * k * k) % K), Q = K / 4, xp = x % Q, u = x / Q;
        const uint32_t rot = (8 * u + (xp & 7) + 32 - (uint32_t)(k & 7)) & 31u;
        c.qpp_tab[ki][k >> 1] |= (((xp >> 3) << 7) | rot) << (16 * (k & 1));
      }
      c.qpp_s3[ki] = (uint32_t)((f1 * (K / 4)) % K) == K / 4 ? 0u : 1u;
      /* the 32-fold where the size admits it: its K/32 uint16 entries replace the quarter fold's in
       * qpp_tab (the kernel takes one path or the other per block size) */
      static_assert(sizeof(c.qpp_tab[0]) >= OAI4G_MAX_CHUNKS * sizeof(uint16_t), "32-fold entries fit qpp_tab");
      uint32_t s32 = 0;
      uint16_t t32[OAI4G_MAX_CHUNKS];
      if (oai4g_qpp_fold32(K, &s32, t32) == 1) {
        memset(c.qpp_tab[ki], 0, sizeof(c.qpp_tab[ki]));
        memcpy(c.qpp_tab[ki], t32, (K / 32) * sizeof(uint16_t));
        c.qpp_f32[ki] = s32 | ((((1u << 20) + K / 1024 - 1) / (K / 1024)) << 5);
      }
    }
    {
      uint32_t o = 0;
      for (uint32_t r = 0; r < C; r++) {
        c.ilv_off[r] = o;
        o += (c.K[r] + 31) / 32;
      }
      c.ilv_off[C] = o;
      c.n0 = (C > 1) ? Cm : 0;
      c.kk[0] = c.n0 ? Km : Kp;
      c.kk[1] = Kp;
      for (int ki = 0; ki < 2; ki++) {
        c.kw[ki] = (c.kk[ki] + 31) / 32;
        c.kmag[ki] = ((1u << 20) + c.kw[ki] - 1) / c.kw[ki];
      }
      c.u0 = c.n0 * c.kw[0];
    }
    c.crc_per_tb = (((c.A_bytes + 255) / 256) + 3) & ~3u;   /* bytes per lane, a multiple of 4 */
    crc_mul_tables(c.crc_per_tb, 8, 0x864cfbu, c.crcmul_tb);
    crc_mul_tables2(c.crc_per_tb, 0x864cfbu, c.crc2_tb);
    uint32_t ncb_max = 0;
    for (uint32_t r = 0; r < C; r++) {
      uint32_t n = c.ncopy[r];
      if (c.src[r] + n > c.A_bytes) n = c.A_bytes > c.src[r] ? c.A_bytes - c.src[r] : 0;
      ncb_max = n > ncb_max ? n : ncb_max;
    }
    /* C > 1: the CRC-24A and every CRC-24B in one pass, crc_lpb lanes per block (k_encode phase 1) */
    c.crc_lpb = C <= 4 ? 64u : (C <= 8 ? 32u : 16u);
    c.crc_per_cb = (((ncb_max + c.crc_lpb - 1) / c.crc_lpb) + 3) & ~3u;
    crc_mul_tables2(c.crc_per_cb ? c.crc_per_cb : 1, 0x864cfbu, c.crc2_cb[0]);
    crc_mul_tables2(c.crc_per_cb ? c.crc_per_cb : 1, 0x800063u, c.crc2_cb[1]);
    for (uint32_t r = 0; r < C; r++) {
      uint32_t end = c.src[r] + c.ncopy[r];
      if (end > c.A_bytes) end = c.A_bytes;
      const uint32_t m = crc_xpow8_h(c.A_bytes - (end > c.src[r] ? end : c.src[r]), 0x864cfbu);
      for (int k = 0; k < 6; k++)
        for (uint32_t v = 0; v < 16; v++) c.crcmul_blk[r][16 * k + v] = crc_mulmod_h((v << (4 * k)) & 0xffffffu, m, 0x864cfbu);
    }
    for (int ki = 0; ki < 2; ki++) {
      uint32_t K = ki == 0 ? (Km ? Km : Kp) : Kp;
      int n = null_positions(K, c.nullpos[ki], OAI4G_MAX_NULLS);
      if (n < 0) { set_err("too many NULL positions"); return -1; }
      c.nnull[ki] = (uint32_t)n;
    }
    for (uint32_t r = 0; r < C; r++) {
      /* k0 >= Ncb (limited buffer only) keeps k0 less the NULLs below it: enable_tb_rv refuses such a start */
      c.k0c[r] = rm_k0c_of_rv(c, c.kidx[r], c.R[r], c.Ncb[r], p->rvidx[cw]);
      c.Nnn[r] = rm_compact(c.Ncb[r], rm_null_list{c.nullpos[c.kidx[r]], c.nnull[c.kidx[r]]});   /* the (possibly limited) buffer */
    }
    uint32_t nw = (maxK + 31) >> 5;
    c.stream_words = nw + 3;   /* + tail word + read-ahead words */
    uint32_t inw = 0;
    for (uint32_t r = 0; r < C; r++) inw += (c.K[r] + 31) >> 5;
    max_inw = inw > max_inw ? inw : max_inw;
    /* packed w of every block (3 Kpi bits = 3R words, + 2 read-ahead words each) and the
     * 32x32 transpose tiles of the sub-block interleaver (3 streams x ceil(R/32) per block) */
    uint32_t wwords = 0, ntask = 0;
    for (uint32_t r = 0; r < C; r++) {
      c.wpk_off[r] = wwords;
      wwords += 3 * c.R[r] + 2;
      for (uint32_t rb = 0; rb < (c.R[r] + 31) / 32; rb++) c.tasks[ntask++] = (uint16_t)(r | (rb << 5));
      for (uint32_t rb = 0; rb < (c.R[r] + 15) / 16; rb++) c.tasks[ntask++] = (uint16_t)(r | (1u << 4) | (rb << 5));
    }
    c.wpk_off[C] = wwords;
    c.ntask = ntask;
    for (uint32_t r = 0; r < C; r++) {   /* every block of one size shares its geometry */
      const uint32_t ki = r < c.n0 ? 0 : 1;
      if (c.K[r] != c.kk[ki]) { set_err("block size order"); return -1; }
      c.Rk[ki] = c.R[r]; c.NDk[ki] = c.ND[r]; c.Ncbk[ki] = c.Ncb[r]; c.Nnnk[ki] = c.Nnn[r]; c.k0ck[ki] = c.k0c[r];
    }
    for (uint32_t r = 0; r < C; r++) {
      const uint32_t ki = r < c.n0 ? 0 : 1;
      if (c.R[r] != c.Rk[ki] || c.ND[r] != c.NDk[ki] || c.Ncb[r] != c.Ncbk[ki] || c.Nnn[r] != c.Nnnk[ki] ||
          c.k0c[r] != c.k0ck[ki] || c.kidx[r] != ki) {
        set_err("per-size block geometry differs");
        return -1;
      }
    }
    if (c.n0 == 0) { c.Rk[0] = c.Rk[1]; c.NDk[0] = c.NDk[1]; c.Ncbk[0] = c.Ncbk[1]; c.Nnnk[0] = c.Nnnk[1]; c.k0ck[0] = c.k0ck[1]; }
    for (int ki = 0; ki < 2; ki++) {
      c.nullcol[ki][0] = c.nullcol[ki][1] = 0;
      for (uint32_t wc = 0; wc < 32; wc++) {
        uint32_t pc = 0;
        for (int b = 0; b < 5; b++) pc |= ((wc >> b) & 1u) << (4 - b);   /* bitrev5 column permutation */
        if (pc < c.NDk[ki]) c.nullcol[ki][0] |= 1u << wc;
        if (pc + 1 < c.NDk[ki]) c.nullcol[ki][1] |= 1u << wc;
      }
      c.t0k[ki] = (c.Rk[ki] + 31) / 32;
      c.ntk[ki] = c.t0k[ki] + (c.Rk[ki] + 15) / 16;
      c.ntmag[ki] = ((1u << 20) + c.ntk[ki] - 1) / c.ntk[ki];
      if (c.ntk[ki] > OAI4G_RM_TILES) { set_err("rate-matching plan: %u tiles", c.ntk[ki]); return -1; }
      rm_plan(c, ki);
    }
    if (oai4g_rm_pair_schedule(C, c.n0, c.ntk, c.rm_wrapt, c.rm_pairs, c.rm_pair0) < 0) {
      set_err("rate-matching pair schedule");
      return -1;
    }
    max_w = wwords > max_w ? wwords : max_w;
    uint32_t tbw = (c.A_bytes + 3 + 3) / 4 + 1;
    max_tb_words = tbw > max_tb_words ? tbw : max_tb_words;
    uint32_t strw = C * 3 * c.stream_words;
    max_stream_words = strw > max_stream_words ? strw : max_stream_words;
    for (int sf = 0; sf < 10; sf++) {
      int G;
      if (fp.nb_antennas_tx == 4) {
        /* 4-TX extension: the reference's get_G formula knows no port-2/3 CRS; G = the RE map's
         * PDSCH RE count x Qm (one layer per codeword) */
        std::vector<uint16_t> tmp((size_t)14 * fp.ofdm_symbol_size);
        uint32_t sb[14];
        int n = build_remap(&fp, p->rb_alloc, p->num_pdcch_symbols, sf, p->mimo_mode, (uint16_t)p->pmi_alloc, tmp.data(), sb,
                            nullptr);
        G = n < 0 ? -1 : n * (int)c.Qm;
      } else {
        G = oai4g_get_G(&fp, p->nb_rb, p->rb_alloc, (uint8_t)c.Qm, Nl[cw], p->num_pdcch_symbols, 0, (uint8_t)sf);
      }
      if (G <= 0 || G > OAI4G_MAX_CHANNEL_BITS) { set_err("G=%d out of range", G); return -1; }
      c.G[sf] = (uint32_t)G;
      uint32_t off = 0;
      for (uint32_t r = 0; r < C; r++) {
        c.E[sf][r] = rm_E((uint32_t)G, Nl[cw], c.Qm, C, r);
        c.roff[sf][r] = off;
        off += c.E[sf][r];
      }
      c.roff[sf][C] = off;
      c.esplit[sf] = rm_esplit((uint32_t)G, Nl[cw], c.Qm, C);
      for (int h = 0; h < 2; h++) {
        const uint32_t E = c.E[sf][h ? C - 1 : 0], w = (E + 31) / 32;
        c.ew[sf][h] = w;
        c.emag[sf][h] = w ? (uint32_t)(((1ull << 32) + w - 1) / w) : 0u;
      }
      uint32_t gw = (off + 31) / 32;
      max_gw = gw > max_gw ? gw : max_gw;
      max_bits = (uint32_t)G > max_bits ? (uint32_t)G : max_bits;
    }
    qam_tables_scaled((int)c.Qm, p->amp, p->sqrt_rho_a, p->sqrt_rho_b, p->mimo_mode == OAI4G_ALAMOUTI || prec1, c);
  }
  if (max_gw > OAI4G_MAX_GOLD_WORDS) { set_err("G too large"); return -1; }
  h.lds_tb_words = max_tb_words;
  h.lds_stream_words = max_stream_words;
  h.lds_gold_words = max_gw + 1;
  h.lds_w_words = max_w;
  (void)max_inw;
  /* encoder LDS regions with phase-disjoint lifetimes (see oai4g_encode.hip) */
  h.lds_a_words = OAI4G_ENC_CRC_TABLE_WORDS;   /* the CRC tables, phases 0-1 (the TB is never staged) */
  for (int cw = 0; cw < p->n_cw; cw++) {
    const cw_dev_t &c = h.cw[cw];
    /* region A also holds the interleaved words in phase 3 (the planes sit in the parity slots) */
    if (c.ilv_off[c.C] > h.lds_a_words) h.lds_a_words = c.ilv_off[c.C];
    /* and, in phase 4, the e words of one half of the blocks at a time (k_encode): blocks [0, hb)
     * then [hb, C), each half from the word holding its first bit, + 1 word for or_bits */
    const uint32_t hb = (c.C + 1) / 2;
    for (int sf = 0; sf < 10; sf++) {
      const uint32_t G = c.G[sf], eb = hb < c.C ? c.roff[sf][hb] : G;
      const uint32_t w1 = (eb + 31) / 32 + 1, w2 = (G + 31) / 32 - eb / 32 + 1;
      if (w1 > h.lds_a_words) h.lds_a_words = w1;
      if (w2 > h.lds_a_words) h.lds_a_words = w2;
    }
  }
  h.lds_b_words = max_stream_words;

  /* RE maps */
  if (need_remap) {
    uint32_t N = h.N;
    cfg->h_remap.assign((size_t)10 * 14 * N, 0xFFFF);
    for (int sf = 0; sf < 10; sf++) {
      if (only_sf >= 0 && sf != only_sf) continue;
      int n = build_remap(&fp, p->rb_alloc, p->num_pdcch_symbols, sf, p->mimo_mode, (uint16_t)p->pmi_alloc,
                          cfg->h_remap.data() + (size_t)sf * 14 * N, h.symbase[sf], &cfg->re_alloc[sf]);
      if (n < 0) { set_err("RE map construction failed"); return -1; }
      cfg->re_count[sf] = n;
      if (p->with_crs) {
        /* pilots.c:43-168: port 0 on antenna 0; antenna 1 port 0 (mode1) or port 1 */
        uint32_t gt[20][2][14];
        lte_gold_table_h(&fp, gt);
        const uint32_t sps = fp.Ncp == 0 ? 7 : 6, psym[4] = {0, sps - 3, sps, 2 * sps - 3};   /* l' = 0, 4 (3) per slot */
        const int nports = (fp.nb_antennas_tx > 1 && !fp.mode1_flag) ? 2 : 1;
        cfg->h_crs.resize((size_t)10 * 6 * 200);
        for (uint32_t i = 0; i < 4; i++) {
          const uint32_t Ns = 2 * sf + (i >> 1), l = i & 1;
          for (uint32_t m = 0; m < 2u * fp.N_RB_DL; m++) {
            const uint32_t mp = 110 - fp.N_RB_DL + m;
            cfg->h_crs[((size_t)sf * 6 + i) * 200 + m] = crs_qpsk(p->amp, (gt[Ns][l][mp >> 4] >> (2 * (mp & 15))) & 3);
            for (int port = 0; port < nports; port++) {
              uint16_t &code = cfg->h_remap[((size_t)sf * 14 + psym[i]) * N + crs_bin(&fp, port, l, m)];
              if (code != 0xFFFF) { set_err("CRS RE collides with a PDSCH RE"); return -1; }
              code = (uint16_t)(OAI4G_CRS_CODE | (i << 9) | ((uint32_t)port << 8) | m);
            }
          }
        }
        if (fp.nb_antennas_tx == 4)   /* ports 2/3: pilot entries 4, 5 = symbol 1 of each slot */
          for (uint32_t s = 0; s < 2; s++) {
            const uint32_t Ns = 2 * sf + s;
            uint32_t gw[14];
            gold_words_h(&fp, Ns, 1, gw);
            for (uint32_t m = 0; m < 2u * fp.N_RB_DL; m++) {
              const uint32_t mp = 110 - fp.N_RB_DL + m;
              cfg->h_crs[((size_t)sf * 6 + 4 + s) * 200 + m] = crs_qpsk(p->amp, (gw[mp >> 4] >> (2 * (mp & 15))) & 3);
              for (uint32_t port = 2; port < 4; port++) {
                uint16_t &code = cfg->h_remap[((size_t)sf * 14 + s * sps + 1) * N + crs_bin_p23(&fp, port, Ns, m)];
                if (code != 0xFFFF) { set_err("CRS RE collides with a PDSCH RE"); return -1; }
                code = (uint16_t)(OAI4G_CRS_CODE | ((4 + s) << 9) | ((port & 1u) << 8) | m);
              }
            }
          }
      }
      /* symbols whose QAM levels use rho_B (CRS-bearing: dlsch_modulation.c:1223-1246) */
      h.pilmask = 0;
      for (uint32_t l = 0, hs = h.nsymb >> 1; l < h.nsymb; l++) {
        const uint32_t ls = l % hs;
        if (ls == 0 || ls == hs - 3 || (fp.nb_antennas_tx == 4 && ls == 1)) h.pilmask |= 1u << l;
      }
      for (int l = 0; l < 14; l++) {
        uint32_t next = l + 1 < (int)h.nsymb ? h.symbase[sf][l + 1] : (uint32_t)n;
        h.symnre[sf][l] = (uint32_t)(l < p->num_pdcch_symbols || l >= (int)h.nsymb ? 0 : next - h.symbase[sf][l]);
      }
      for (int cw = 0; cw < p->n_cw; cw++) {
        uint32_t bits = (uint32_t)n * h.cw[cw].Qm;
        max_bits = bits > max_bits ? bits : max_bits;
      }
    }
  }
  h.ebits_words = (max_bits + 31) / 32 + 2;
  return rm_fail ? -2 : 0;
}

/* cfg_dev_t::stat_tm from the RE map, the CRS values (h_crs) and the static-RE table (h_ctl): the
 * packed IQ that kernel antenna `ant` (TM1: the one transform) carries at every RE that is not a
 * data RE, in remap_tm's thread-major order.  A CRS RE holds port p's pilot on antenna p and 0 on
 * the others, every port's in the single TM1 transform (pilots.c:43-168); a static RE holds the
 * table's value for that antenna (generate_dci_top, the PBCH and the PHICH write antennas 0 / 1, the
 * PSS and SSS every antenna).  k_modofdm ORs the plane over its data path. */
static int build_stat_tm(oai4g_tx_config *cfg)
{
  if (cfg->h_remap.empty() || (cfg->h_crs.empty() && cfg->h_ctl.empty())) {
    cfg->d_stat.reset();
    cfg->h.stat_tm = nullptr;
    cfg->h.stat_planes = 0;
    return 0;
  }
  const size_t N = cfg->h.N, T = N >> 4, nsl = cfg->h_remap.size() / N;
  const uint32_t planes = cfg->h.mimo_mode == OAI4G_SISO ? 1u : cfg->h.n_ant;
  std::vector<uint32_t> st(nsl * planes * N, 0u);
  for (size_t sl = 0; sl < nsl; sl++) {
    const size_t sf = sl / 14;
    for (size_t pos = 0; pos < N; pos++) {
      const uint32_t cd = cfg->h_remap[sl * N + pos];
      const size_t t = pos % T, k = pos / T;
      for (uint32_t ant = 0; ant < planes; ant++) {
        uint32_t v = 0;
        if (cd != 0xFFFFu && (cd & 0xE000u) == OAI4G_CRS_CODE) {
          const uint32_t ci = (cd >> 9) & 7u, m = cd & 0xFFu, port = ((cd >> 8) & 1u) | (ci >= 4 ? 2u : 0u);
          if (!cfg->h_crs.empty() && (planes == 1 || ant == port)) v = cfg->h_crs[(sf * 6 + ci) * 200 + m];
        } else if ((cd & 0xE000u) == OAI4G_CTL_CODE) {
          if (!cfg->h_ctl.empty() && ant < cfg->ctl_planes) v = cfg->h_ctl[(sl * cfg->ctl_planes + ant) * N + pos];
        }
        st[(sl * planes + ant) * N + t * 16 + k] = v;
      }
    }
  }
  HCK(cfg->d_stat.upload(st), -1);
  cfg->h.stat_tm = cfg->d_stat.get();
  cfg->h.stat_planes = planes;
  return 0;
}

static int upload_remap(oai4g_tx_config *cfg)
{
  const size_t n = cfg->h_remap.size();
  if (n) {
    /* the natural layout k_modulate_bytes reads, then k_modofdm's thread-major copy */
    const size_t N = cfg->h.N, T = N >> 4;
    for (int sf = 0; sf < 10; sf++)
      for (int l = 0; l < 14; l++)
        if (!oai4g_mod_nre_fits(cfg->h.symnre[sf][l], (uint32_t)N)) { set_err("too many data REs per symbol for the modulator"); return -1; }
    std::vector<uint16_t> both(2 * n);
    std::copy(cfg->h_remap.begin(), cfg->h_remap.end(), both.begin());
    /* k_modofdm's staged entries (oai4g_internal.h): 2-byte QAM-table addresses, or in the 2048-point
     * kernels 8-byte (y0, d) pairs of two-antenna LARGE_CDD / 4-byte QAM words of TM1 */
    const uint32_t esh = oai4g_mod_entry_shift(cfg->h.mimo_mode, cfg->h.n_ant, cfg->h.log2N);
    const bool pre = esh == 3, pre1 = esh == 2;
    const uint16_t sentinel = (uint16_t)(oai4g_mod_sentinel((uint32_t)N) << esh);
    for (size_t sl = 0; sl < n / N; sl++)
      for (size_t t = 0; t < T; t++)
        for (size_t k = 0; k < 16; k++) {
          uint16_t code = cfg->h_remap[sl * N + t + T * k];
          /* data RE (idx | parity << 15, idx below the sentinel): the byte offset of its staged entry */
          if (code < OAI4G_CTL_CODE) {
            /* the precoded pairs carry the CDD sign already: the staging step stores -d for an odd
             * data index.  The reference alternates the sign per RE within each RB
             * (dlsch_modulation.c:733-749) and every RB of a two-port grid holds an even number of
             * data REs (12, 8 beside the 4 CRS REs, 6 / 4 in a half RB), so the parity is the index's;
             * checked here for every RE */
            const bool prec1 = oai4g_mode_prec1(cfg->h.mimo_mode);   /* precoder bits instead of a parity */
            const uint32_t idx = code & (prec1 ? oai4g_mod_pmi_idx_mask : 0x3FFFu), par = code >> 15;
            if (pre && par != (idx & 1u)) { set_err("LARGE_CDD: CDD parity differs from the RE index parity"); return -1; }
            code = (uint16_t)(((pre || pre1 ? 0u : par) << 15) | (prec1 ? code & oai4g_mod_pmi_bits : 0u) | (idx << esh));
          }
          both[n + sl * N + t * 16 + k] = code < OAI4G_CTL_CODE ? code : sentinel;
        }
    HCK(cfg->d_remap.upload(both), -1);
  } else {
    cfg->d_remap.reset();
  }
  cfg->h.remap = cfg->d_remap.get();
  cfg->h.remap_tm = n ? cfg->d_remap.get() + n : nullptr;
  return build_stat_tm(cfg);
}

/* the scrambling words of every (subframe index, codeword): lte_gold_generic (lte_gold.c:151-177)
 * with c_init = rnti 2^14 + q 2^13 + subframe 2^9 + Nid_cell (dlsch_scrambling.c:74-76) */
static int upload_gold(oai4g_tx_config *cfg)
{
  const cfg_dev_t &h = cfg->h;
  const size_t stride = h.ebits_words;
  std::vector<uint32_t> g((size_t)10 * h.n_cw * stride, 0u);
  for (uint32_t sf = 0; sf < 10; sf++)
    for (uint32_t cw = 0; cw < h.n_cw; cw++) {
      const uint32_t c_init = (h.rnti << 14) + (h.cw[cw].q << 13) + (sf << 9) + h.Nid_cell;
      const size_t nw = std::min(stride, (size_t)(h.cw[cw].G[sf] + 31) / 32);
      gold_seq_h(c_init, g.data() + ((size_t)sf * h.n_cw + cw) * stride, nw);
    }
  HCK(cfg->d_gold.upload(g), -1);
  cfg->h.gold_tab = cfg->d_gold.get();
  return 0;
}

static int upload_cfg(oai4g_tx_config *cfg)
{
  if (upload_remap(cfg) != 0) return -1;
  if (upload_gold(cfg) != 0) return -1;
  cfg->h.with_crs = !cfg->h_crs.empty();
  cfg->h.mod_nosat = mod_nosat_ok(cfg->h, std::max(packed_iq_max(cfg->h_crs), cfg->ctl_vmax));
  mod_items_setup(cfg->h);
  cfg->h.n_cu = (uint32_t)g_n_cu;
  cfg->h.gold_x1 = g_gx1;
  cfg->h.gold_x2j = g_gx2j;
  cfg->h.tw = g_tw;
  HCK(cfg->d.upload(&cfg->h, 1), -1);
  return 0;
}

/* declared after a drop-in's stack configuration, so that it goes first on every path out: unless the
 * caller has already synchronised (done), it waits for the scratch stream before the configuration's
 * device memory is freed: a launched kernel may still read it. */
namespace {
struct cfg_scope_t {
  bool done = false;
  ~cfg_scope_t() { if (!done && g_scr.s) hipStreamSynchronize(g_scr.s); }
};
}  // namespace

extern "C" oai4g_tx_config_t *oai4g_tx_config_create(const oai4g_tx_params_t *p)
{
  NEED_INIT(nullptr);
  if (p->N_RB_DL != 6 && p->N_RB_DL != 15 && p->N_RB_DL != 25 && p->N_RB_DL != 50 && p->N_RB_DL != 100) {
    set_err("batched path supports N_RB_DL 6, 15, 25, 50, 100 (IDFT 128/256/512/1024/2048)");
    return nullptr;
  }
  if (oai4g_mode_prec1(p->mimo_mode) && (p->n_cw != 1 || p->nb_antennas_tx != 2 || p->mode1_flag != 0)) {
    set_err("single-layer precoding (mimo_mode %u) requires one codeword, 2 TX antennas and mode1_flag 0", p->mimo_mode);
    return nullptr;
  }
  std::unique_ptr<oai4g_tx_config> cfg(new oai4g_tx_config());
  uint8_t Nl[2] = {1, 1};
  /* RM condition (-2) is an error here */
  if (derive_cfg(cfg.get(), p, Nl, true, -1) != 0 || upload_cfg(cfg.get()) != 0) return nullptr;
  bool ok = hipStreamCreateWithFlags(&cfg->s_mod, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&cfg->ev_done, hipEventDisableTiming) == hipSuccess;
  for (auto &e : cfg->ev_enc) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    set_err("stream/event creation failed");
    return nullptr;
  }
  if (const char *pc = getenv("OAI4G_PIPE_CHUNK")) cfg->pipe_chunk = atoi(pc);
  return cfg.release();
}

extern "C" void oai4g_tx_config_destroy(oai4g_tx_config_t *cfg)
{
  if (cfg) delete cfg;
}

extern "C" uint32_t oai4g_tx_G(const oai4g_tx_config_t *cfg, int cw, int subframe)
{
  return cfg->h.cw[cw].G[subframe % 10];
}
extern "C" uint32_t oai4g_tx_ebits_words(const oai4g_tx_config_t *cfg) { return cfg->h.ebits_words; }
extern "C" uint32_t oai4g_tx_iq_samples(const oai4g_tx_config_t *cfg) { return cfg->h.spt; }
extern "C" size_t oai4g_tx_workspace_bytes(const oai4g_tx_config_t *cfg, int n_sf)
{
  return (size_t)n_sf * cfg->h.n_cw * cfg->h.ebits_words * 4;
}

extern "C" int oai4g_tx_encode(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, void *d_work,
                               void *stream)
{
  NEED_INIT(-1);
  HCK(oai4g_launch_encode(cfg->d.get(), &cfg->h, 0, n_sf, d_payload, (uint32_t *)d_work, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_tx_config_enable_tb_rv(oai4g_tx_config_t *cfg)
{
  NEED_INIT(-1);
  if (!cfg) { set_err("tx_config_enable_tb_rv: null configuration"); return -1; }
  if (cfg->d_rvtab) return 0;
  const uint32_t n_cw = cfg->h.n_cw;
  std::vector<enc_rv_tab_t> tabs(4 * (size_t)n_cw);
  for (uint32_t rv = 0; rv < 4; rv++)
    for (uint32_t cw = 0; cw < n_cw; cw++) {
      /* the configuration's own plan builder on a copy of the codeword with this rv's k0c: the
       * limited-buffer extension and the general-path test hook apply per rv as they do there.  The
       * "RM condition" exit (Ncb < Kw without the extension) depends on no rv: a configuration that
       * takes it was refused at creation. */
      std::unique_ptr<cw_dev_t> c(new cw_dev_t(cfg->h.cw[cw]));
      enc_rv_tab_t &t = tabs[rv * n_cw + cw];
      memset(&t, 0, sizeof(t));
      /* with one block size (n0 = 0) index 0 mirrors index 1, whose NULL list is the size's */
      c->k0ck[1] = rm_k0c_of_rv(*c, 1, c->Rk[1], c->Ncbk[1], rv);
      c->k0ck[0] = c->n0 ? rm_k0c_of_rv(*c, 0, c->Rk[0], c->Ncbk[0], rv) : c->k0ck[1];
      for (int ki = 0; ki < 2; ki++) {
        if (c->k0ck[ki] >= c->Nnnk[ki]) {
          set_err("tx_config_enable_tb_rv: rv %u starts at %u of %u circular-buffer entries", rv, c->k0ck[ki], c->Nnnk[ki]);
          return -1;
        }
        rm_plan(*c, ki);
      }
      if (oai4g_rm_pair_schedule(c->C, c->n0, c->ntk, c->rm_wrapt, c->rm_pairs, c->rm_pair0) < 0) {
        set_err("tx_config_enable_tb_rv: rate-matching pair schedule");
        return -1;
      }
      if (memcmp(c->rm_src, cfg->h.cw[cw].rm_src, sizeof(c->rm_src)) != 0) {
        set_err("tx_config_enable_tb_rv: the source plan depends on rv");
        return -1;
      }
      memcpy(t.rm_dst, c->rm_dst, sizeof(t.rm_dst));
      memcpy(t.rm_pair0, c->rm_pair0, sizeof(t.rm_pair0));
      memcpy(t.rm_pairs, c->rm_pairs, sizeof(t.rm_pairs));
      memcpy(t.rm_wrapt, c->rm_wrapt, sizeof(t.rm_wrapt));
      memcpy(t.k0ck, c->k0ck, sizeof(t.k0ck));
    }
  if (cfg->d_rvtab.upload(tabs) != hipSuccess) {
    set_err("tx_config_enable_tb_rv: upload failed");
    return -1;
  }
  return 0;
}

static int iq_aligned(const int32_t *d_iq);

static int tb_rv_ready(const oai4g_tx_config_t *cfg, const uint8_t *d_rv, const char *who)
{
  if (!cfg || !cfg->d_rvtab) { set_err("%s: oai4g_tx_config_enable_tb_rv was not called", who); return 0; }
  if (!d_rv) { set_err("%s: null rv array", who); return 0; }
  return 1;
}

extern "C" int oai4g_tx_encode_rv(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, const uint8_t *d_rv,
                                  void *d_work, void *stream)
{
  NEED_INIT(-1);
  if (!tb_rv_ready(cfg, d_rv, "tx_encode_rv")) return -1;
  HCK(oai4g_launch_encode_rv(cfg->d.get(), &cfg->h, n_sf, d_payload, d_rv, cfg->d_rvtab.get(), (uint32_t *)d_work,
                             (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_tx_batch_rv(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, const uint8_t *d_rv,
                                 void *d_work, int32_t *d_iq, void *stream)
{
  NEED_INIT(-1);
  if (!tb_rv_ready(cfg, d_rv, "tx_batch_rv")) return -1;
  if (n_sf <= 0) return 0;
  if (!iq_aligned(d_iq)) return -1;
  hipStream_t s = (hipStream_t)stream;
  HCK(oai4g_launch_encode_rv(cfg->d.get(), &cfg->h, n_sf, d_payload, d_rv, cfg->d_rvtab.get(), (uint32_t *)d_work, s), -1);
  HCK(oai4g_launch_modofdm(cfg->d.get(), &cfg->h, 0, n_sf, (const uint32_t *)d_work, d_iq, s), -1);
  return 0;
}

/* the 2048-point modulator stores sample pairs as 8-byte words */
static int iq_aligned(const int32_t *d_iq)
{
  if ((uintptr_t)d_iq & 7u) {
    set_err("iq buffer must be 8-byte aligned");
    return 0;
  }
  return 1;
}

extern "C" int oai4g_tx_batch(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, void *d_work,
                              int32_t *d_iq, void *stream)
{
  NEED_INIT(-1);
  if (n_sf <= 0) return 0;
  if (!iq_aligned(d_iq)) return -1;
  hipStream_t s = (hipStream_t)stream;
  uint32_t *ew = (uint32_t *)d_work;
  int chunk = cfg->pipe_chunk;
  if (chunk <= 0 || n_sf < 2 * chunk) {
    HCK(oai4g_launch_encode(cfg->d.get(), &cfg->h, 0, n_sf, d_payload, ew, s), -1);
    HCK(oai4g_launch_modofdm(cfg->d.get(), &cfg->h, 0, n_sf, ew, d_iq, s), -1);
    return 0;
  }
  int nch = (n_sf + chunk - 1) / chunk;
  if (nch > OAI4G_PIPE_MAX_CHUNKS) {
    nch = OAI4G_PIPE_MAX_CHUNKS;
    chunk = (n_sf + nch - 1) / nch;
  }
  /* the modulator stream must not start before work already queued on the caller's stream */
  HCK(hipEventRecord(cfg->ev_done, s), -1);
  HCK(hipStreamWaitEvent(cfg->s_mod, cfg->ev_done, 0), -1);
  for (int i = 0; i < nch; i++) {
    const int sf0 = i * chunk, n = n_sf - sf0 < chunk ? n_sf - sf0 : chunk;
    HCK(oai4g_launch_encode(cfg->d.get(), &cfg->h, sf0, n, d_payload, ew, s), -1);
    HCK(hipEventRecord(cfg->ev_enc[i], s), -1);
    HCK(hipStreamWaitEvent(cfg->s_mod, cfg->ev_enc[i], 0), -1);
    HCK(oai4g_launch_modofdm(cfg->d.get(), &cfg->h, sf0, n, ew, d_iq, cfg->s_mod), -1);
  }
  HCK(hipEventRecord(cfg->ev_done, cfg->s_mod), -1);
  HCK(hipStreamWaitEvent(s, cfg->ev_done, 0), -1);
  return 0;
}

extern "C" int oai4g_tx_batch_timed(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload, void *d_work,
                                    int32_t *d_iq, void *stream, float *kernel_ms)
{
  NEED_INIT(-1);
  if (!iq_aligned(d_iq)) return -1;
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t ev[3];
  for (int i = 0; i < 3; i++) HCK(hipEventCreate(&ev[i]), -1);
  HCK(hipEventRecord(ev[0], s), -1);
  HCK(oai4g_launch_encode(cfg->d.get(), &cfg->h, 0, n_sf, d_payload, (uint32_t *)d_work, s), -1);
  HCK(hipEventRecord(ev[1], s), -1);
  HCK(oai4g_launch_modofdm(cfg->d.get(), &cfg->h, 0, n_sf, (const uint32_t *)d_work, d_iq, s), -1);
  HCK(hipEventRecord(ev[2], s), -1);
  HCK(hipEventSynchronize(ev[2]), -1);
  HCK(hipEventElapsedTime(&kernel_ms[0], ev[0], ev[1]), -1);
  HCK(hipEventElapsedTime(&kernel_ms[1], ev[1], ev[2]), -1);
  for (int i = 0; i < 3; i++) hipEventDestroy(ev[i]);
  return 0;
}

extern "C" int oai4g_tx_modulate(const oai4g_tx_config_t *cfg, int n_sf, const void *d_work, int32_t *d_iq,
                                 void *stream)
{
  NEED_INIT(-1);
  if (!cfg || !iq_aligned(d_iq)) return -1;
  HCK(oai4g_launch_modofdm(cfg->d.get(), &cfg->h, 0, n_sf, (const uint32_t *)d_work, d_iq, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_tx_mod_nosat(const oai4g_tx_config_t *cfg) { return cfg ? (int)cfg->h.mod_nosat : 0; }
extern "C" int oai4g_tx_mod_lz(const oai4g_tx_config_t *cfg) { return cfg ? (int)cfg->h.mod_lz : -1; }

/* Diagnostics: time the encoder with an early exit after phase `stop_phase`
 * (0 load/Gold, 1 CRC, 2 segmentation, 3 turbo, 4 w build, 99 full). Outputs are invalid. */
extern "C" int oai4g_diag_encode_phase_ms(const oai4g_tx_config_t *cfg, int n_sf, const uint8_t *d_payload,
                                          void *d_work, int stop_phase, int reps, float *ms)
{
  NEED_INIT(-1);
  hipEvent_t a, b;
  HCK(hipEventCreate(&a), -1);
  HCK(hipEventCreate(&b), -1);
  HCK(oai4g_launch_encode_phase(cfg->d.get(), &cfg->h, n_sf, d_payload, (uint32_t *)d_work, stop_phase, nullptr), -1);
  HCK(hipEventRecord(a, nullptr), -1);
  for (int i = 0; i < reps; i++)
    HCK(oai4g_launch_encode_phase(cfg->d.get(), &cfg->h, n_sf, d_payload, (uint32_t *)d_work, stop_phase, nullptr), -1);
  HCK(hipEventRecord(b, nullptr), -1);
  HCK(hipEventSynchronize(b), -1);
  HCK(hipEventElapsedTime(ms, a, b), -1);
  *ms /= reps;
  hipEventDestroy(a);
  hipEventDestroy(b);
  return 0;
}

/* Diagnostics: resident encoder workgroups per CU and the dynamic LDS bytes of one workgroup */
extern "C" int oai4g_diag_encode_occupancy(const oai4g_tx_config_t *cfg, int *blocks_per_cu, size_t *lds_bytes)
{
  NEED_INIT(-1);
  if (!cfg || !blocks_per_cu || !lds_bytes) { set_err("diag_encode_occupancy: bad arguments"); return -1; }
  HCK(oai4g_encode_occupancy(&cfg->h, blocks_per_cu, lds_bytes), -1);
  return 0;
}

/* PMC calibration: stream `bytes` at 4 B per lane (mode 0 read from src, 1 write to dst) */
extern "C" int oai4g_diag_stream(const void *d_src, void *d_dst, size_t bytes, int mode, void *stream)
{
  NEED_INIT(-1);
  HCK(oai4g_launch_diag_stream(d_src, d_dst, bytes, mode, (hipStream_t)stream), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * device memory helpers
 * ---------------------------------------------------------------------------------------- */
extern "C" void *oai4g_dev_alloc(size_t bytes)
{
  NEED_INIT(nullptr);
  void *p = nullptr;
  HCK(hipMalloc(&p, bytes), nullptr);
  return p;
}
extern "C" void oai4g_dev_free(void *p)
{
  if (p) hipFree(p);
}
extern "C" int oai4g_memcpy_h2d(void *dst, const void *src, size_t bytes)
{
  NEED_INIT(-1);
  HCK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), -1);
  return 0;
}
extern "C" int oai4g_memcpy_d2h(void *dst, const void *src, size_t bytes)
{
  NEED_INIT(-1);
  HCK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), -1);
  return 0;
}
extern "C" int oai4g_memset_d(void *dst, int value, size_t bytes)
{
  NEED_INIT(-1);
  HCK(hipMemset(dst, value, bytes), -1);
  return 0;
}
extern "C" int oai4g_sync(void)
{
  NEED_INIT(-1);
  HCK(hipDeviceSynchronize(), -1);
  return 0;
}
/* ------------------------------------------------------------------------------------------
 * dlsim's channel stage (dlsim.c:2714-2866): tx_lev and AWGN, device batches and the host drop-in
 * ---------------------------------------------------------------------------------------- */
extern "C" int oai4g_signal_energy_batch(const int32_t *d_x, int n, size_t stride, uint32_t length, int32_t *d_energy,
                                         void *stream)
{
  NEED_INIT(-1);
  if (n < 0 || length < 2 || (n > 0 && (!d_x || !d_energy))) { set_err("signal_energy_batch: bad arguments"); return -1; }
  HCK(oai4g_launch_signal_energy(d_x, n, stride, length, d_energy, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int32_t oai4g_signal_energy(const int32_t *input, uint32_t length)
{
  NEED_INIT(-1);
  if (!input || length < 2) { set_err("signal_energy: bad arguments"); return -1; }
  int32_t e = -1;
  stage_t st("signal_energy");
  const int r_x = st.add((size_t)length * 4), r_e = st.add(4, 252);
  if (!st.open()) return -1;
  HCK(st.up(r_x, input, (size_t)length * 4), -1);
  HCK(oai4g_launch_signal_energy(st.ptr<int32_t>(r_x), 1, 0, length, st.ptr<int32_t>(r_e), g_scr.s), -1);
  HCK(st.down(&e, r_e, 4), -1);
  HCK(st.sync(), -1);
  return e;
}

extern "C" int oai4g_awgn_batch(const int32_t *d_tx, size_t tx_stride, uint32_t tx_len, const int32_t *d_tail,
                                uint32_t tail_len, int32_t *d_rx, size_t rx_stride, int n, const int32_t *d_tx_lev,
                                double offset_db, uint64_t seed, uint32_t first_vector, void *stream)
{
  NEED_INIT(-1);
  if (n < 0 || (n > 0 && (!d_tx || !d_rx || !d_tx_lev || (tail_len && !d_tail))) || n > 65535 ||
      tx_len + tail_len == 0) {
    set_err("awgn_batch: bad arguments");
    return -1;
  }
  HCK(oai4g_launch_awgn(d_tx, tx_stride, tx_len, d_tail, tail_len, d_rx, rx_stride, n, d_tx_lev, offset_db, seed,
                        first_vector, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_fill_payload(uint8_t *d_payload, size_t bytes, uint64_t seed, void *stream)
{
  NEED_INIT(-1);
  HCK(oai4g_launch_fill(d_payload, bytes, seed, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_harq_advance(int n_slots, int C, uint8_t max_iterations, int num_rounds, int n_cw,
                                  const uint8_t *d_iters, uint8_t *d_round, uint32_t *d_trial, uint8_t *d_rv,
                                  uint8_t *d_clear, uint8_t *d_done, uint32_t *d_counters, uint8_t *d_payload,
                                  size_t row_bytes, uint64_t seed, void *stream)
{
  NEED_INIT(-1);
  if (n_slots <= 0) return 0;
  if (C < 1 || C > OAI4G_MAX_SEGMENTS || num_rounds < 1 || num_rounds > 4 || n_cw < 1 || n_cw > 2) {
    set_err("harq_advance: C %d (1..16), num_rounds %d (1..4), n_cw %d (1..2)", C, num_rounds, n_cw);
    return -1;
  }
  if (!d_iters || !d_round || !d_trial || !d_rv || !d_clear || !d_done || !d_counters || !d_payload) {
    set_err("harq_advance: null array");
    return -1;
  }
  if (row_bytes == 0 || (row_bytes & 7) || ((uintptr_t)d_payload & 7) || row_bytes / 8 > 0xFFFFFFFFu) {
    set_err("harq_advance: payload rows must be 8-byte aligned multiples of 8 bytes (row_bytes %zu)", row_bytes);
    return -1;
  }
  harq_state_t st = {d_round, d_trial, d_rv, d_clear, d_done, d_counters, d_payload};
  HCK(oai4g_launch_harq_advance(st, (uint32_t)n_slots, (uint32_t)C, max_iterations, (uint32_t)num_rounds, (uint32_t)n_cw,
                                (uint32_t)(row_bytes / 8), seed, d_iters, (hipStream_t)stream), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * dlsch containers (new_eNB_dlsch / free_eNB_dlsch, dlsch_coding.c:85-220)
 * ---------------------------------------------------------------------------------------- */
extern "C" oai4g_dlsch_t *oai4g_new_dlsch(uint8_t Kmimo, uint8_t Mdlharq, uint8_t N_RB_DL)
{
  int bw_scaling = N_RB_DL == 6 ? 16 : (N_RB_DL == 25 ? 4 : (N_RB_DL == 50 ? 2 : 1));
  oai4g_dlsch_t *d = (oai4g_dlsch_t *)calloc(1, sizeof(oai4g_dlsch_t));
  if (!d) return nullptr;
  d->Kmimo = Kmimo;
  d->Mdlharq = Mdlharq;
  d->sqrt_rho_a = 8192;
  d->sqrt_rho_b = 8192;
  for (int i = 0; i < Mdlharq && i < 8; i++) {
    oai4g_dl_harq_t *h = (oai4g_dl_harq_t *)calloc(1, sizeof(oai4g_dl_harq_t));
    d->harq_processes[i] = h;
    h->b = (uint8_t *)calloc(OAI4G_MAX_SEGMENTS * 768 / bw_scaling + 8, 1);
    h->e = (uint8_t *)calloc(OAI4G_MAX_CHANNEL_BITS + 64, 1);
    h->Nl = 1;
    for (int r = 0; r < OAI4G_MAX_SEGMENTS; r++) {
      h->c[r] = (uint8_t *)calloc(8 + 3 + 768, 1);
      h->d[r] = (uint8_t *)calloc(OAI4G_D_BYTES + 16, 1);
      h->w[r] = (uint8_t *)calloc(OAI4G_W_BYTES, 1);
      memset(h->d[r], OAI4G_LTE_NULL, 96);
    }
  }
  return d;
}

extern "C" void oai4g_free_dlsch(oai4g_dlsch_t *d)
{
  if (!d) return;
  for (int i = 0; i < 8; i++) {
    oai4g_dl_harq_t *h = d->harq_processes[i];
    if (!h) continue;
    for (int r = 0; r < OAI4G_MAX_SEGMENTS; r++) { free(h->c[r]); free(h->d[r]); free(h->w[r]); }
    free(h->b);
    free(h->e);
    free(h);
  }
  free(d);
}

/* lte_gold_generic (lte_gold.c:151-177): host-side scalar helper */
extern "C" uint32_t oai4g_lte_gold_generic(uint32_t *x1, uint32_t *x2, uint8_t reset)
{
  if (reset) gold_start_h(*x2, x1, x2);
  gold_step_h(x1, x2);
  return *x1 ^ *x2;
}

/* ------------------------------------------------------------------------------------------
 * drop-in coding entry points
 * ---------------------------------------------------------------------------------------- */
static uint32_t crc_dropin(const uint8_t *in, int bitlen, uint32_t poly_top)
{
  NEED_INIT(0);
  uint32_t nbytes = (uint32_t)(bitlen + 7) / 8;
  stage_t st("crc24");
  const int r_in = st.add(nbytes), r_out = st.add(4, 60);
  if (!st.open()) return 0;
  uint32_t out = 0;
  HCK(st.up(r_in, in, nbytes), 0);
  HCK(oai4g_launch_crc24(st.ptr(r_in), bitlen, poly_top, st.ptr<uint32_t>(r_out), g_scr.s), 0);
  HCK(st.down(&out, r_out, 4), 0);
  HCK(st.sync(), 0);
  return out;
}

extern "C" uint32_t oai4g_crc24a(const uint8_t *in, int bitlen) { return crc_dropin(in, bitlen, 0x864cfb00u); }
extern "C" uint32_t oai4g_crc24b(const uint8_t *in, int bitlen) { return crc_dropin(in, bitlen, 0x80006300u); }

extern "C" int oai4g_lte_segmentation(const uint8_t *input_buffer, uint8_t **output_buffers, uint32_t B, uint32_t *C,
                                      uint32_t *Cplus, uint32_t *Cminus, uint32_t *Kplus, uint32_t *Kminus,
                                      uint32_t *F)
{
  uint32_t L;
  if (seg_params(B, C, Cplus, Cminus, Kplus, Kminus, F, &L) < 0) return -1;
  if (input_buffer && output_buffers) {
    uint32_t k = 0, s = 0;
    for (; k < (*F >> 3); k++) output_buffers[0][k] = 0;
    for (uint32_t r = 0; r < *C; r++) {
      uint32_t Kr = r < *Cminus ? *Kminus : *Kplus;
      for (; k < ((Kr - L) >> 3); k++) output_buffers[r][k] = input_buffer[s++];
      if (*C > 1) {
        uint32_t crc = oai4g_crc24b(output_buffers[r], (int)(Kr - 24)) >> 8;
        output_buffers[r][(Kr - 24) >> 3] = (uint8_t)(crc >> 16);
        output_buffers[r][1 + ((Kr - 24) >> 3)] = (uint8_t)(crc >> 8);
        output_buffers[r][2 + ((Kr - 24) >> 3)] = (uint8_t)crc;
      }
      k = 0;
    }
  }
  return 0;
}

extern "C" void oai4g_threegpplte_turbo_encoder(const uint8_t *input, uint16_t input_length_bytes, uint8_t *output,
                                                uint8_t F, uint16_t f1, uint16_t f2)
{
  (void)F; /* the reference's SSE encoder ignores F (3gpplte_sse.c:380-476) */
  NEED_INIT();
  uint32_t K = (uint32_t)input_length_bytes * 8;
  if (oai4g_qpp_index(K) < 0) {
    printf("Illegal frame length!\n");
    return;
  }
  stage_t st("threegpplte_turbo_encoder");
  const int r_in = st.add(6144 / 8, 256), r_out = st.add(3 * 6144 + 12, 52);   /* the largest block */
  if (!st.open()) return;
  HCK(st.up(r_in, input, input_length_bytes), );
  HCK(oai4g_launch_turbo_bytes(st.ptr(r_in), input_length_bytes, st.ptr(r_out), f1, f2, g_scr.s), );
  HCK(st.down(output, r_out, 3 * K + 12), );
  HCK(st.sync(), );
}

extern "C" uint32_t oai4g_sub_block_interleaving_turbo(uint32_t D, uint8_t *d, uint8_t *w)
{
  NEED_INIT(0);
  uint32_t R = (D + 31) >> 5, Kpi = R << 5;
  size_t dbytes = 96 + 3 * (size_t)D + 3;
  stage_t st("sub_block_interleaving_turbo");
  const int r_d = st.add(dbytes), r_w = st.add(3 * (size_t)Kpi, 64);
  if (!st.open()) return 0;
  HCK(st.up(r_d, d - 96, dbytes), 0);
  HCK(oai4g_launch_subblock_bytes(D, st.ptr(r_d), st.ptr(r_w), g_scr.s), 0);
  HCK(st.down(w, r_w, 3 * (size_t)Kpi), 0);
  HCK(st.sync(), 0);
  d[3 * D + 2] = d[2]; /* side effect kept (lte_rate_matching.c:75) */
  return R;
}

extern "C" uint32_t oai4g_lte_rate_matching_turbo(uint32_t RTC, uint32_t G, const uint8_t *w, uint8_t *e, uint8_t C,
                                                  uint32_t Nsoft, uint8_t Mdlharq, uint8_t Kmimo, uint8_t rvidx,
                                                  uint8_t Qm, uint8_t Nl, uint8_t r, uint8_t nb_rb, uint8_t m)
{
  (void)nb_rb;
  (void)m;
  NEED_INIT(0);
  const rm_ncb_t g = rm_ncb(Nsoft, Kmimo, Mdlharq, C, RTC);
  if (g.shorter) {
    rm_condition_exit(g, Nsoft);
    return 0;
  }
  const uint32_t Ncb = g.Ncb, E = rm_E(G, Nl, Qm, C, r), k0 = rm_k0(RTC, Ncb, rvidx);
  stage_t st("lte_rate_matching_turbo");
  const int r_w = st.add(Ncb), r_e = st.add(E), r_s = st.add(4, 60);   /* s: the status word */
  if (!st.open()) return 0;
  HCK(st.up(r_w, w, Ncb), 0);
  HCK(oai4g_launch_rm_bytes(st.ptr(r_w), Ncb, k0, E, st.ptr(r_e), st.ptr<uint32_t>(r_s), g_scr.s), 0);
  HCK(st.down(e, r_e, E), 0);
  HCK(st.sync(), 0);
  return E;
}

/* parameter block for a single-DLSCH drop-in call */
static void params_from_dlsch(const oai4g_frame_parms_t *fp, uint8_t num_pdcch, const oai4g_dlsch_t *d0,
                              const oai4g_dlsch_t *d1, uint8_t subframe, oai4g_tx_params_t *p, uint8_t Nl[2])
{
  memset(p, 0, sizeof(*p));
  const oai4g_dl_harq_t *h0 = d0->harq_processes[d0->current_harq_pid];
  p->N_RB_DL = fp->N_RB_DL;
  p->Nid_cell = fp->Nid_cell;
  p->Ncp = fp->Ncp;
  p->nb_antennas_tx = fp->nb_antennas_tx;
  p->mode1_flag = fp->mode1_flag;
  p->frame_type = fp->frame_type;
  p->n_cw = d1 ? 2 : 1;
  p->mimo_mode = h0->mimo_mode;
  p->num_pdcch_symbols = num_pdcch;
  p->Kmimo = d0->Kmimo;
  p->Mdlharq = d0->Mdlharq;
  p->first_subframe = subframe;
  p->subframe_step = 0;
  p->rnti = d0->rnti;
  p->amp = 512;
  p->sqrt_rho_a = d0->sqrt_rho_a;
  p->sqrt_rho_b = d0->sqrt_rho_b;
  memcpy(p->rb_alloc, h0->rb_alloc, sizeof(p->rb_alloc));
  p->nb_rb = h0->nb_rb;
  p->pmi_alloc = h0->pmi_alloc;
  p->mcs[0] = h0->mcs;
  p->rvidx[0] = h0->rvidx;
  p->TBS[0] = h0->TBS;
  Nl[0] = h0->Nl ? h0->Nl : 1;
  Nl[1] = 1;
  if (d1) {
    const oai4g_dl_harq_t *h1 = d1->harq_processes[d0->current_harq_pid];
    p->mcs[1] = h1->mcs;
    p->rvidx[1] = h1->rvidx;
    p->TBS[1] = h1->TBS;
    Nl[1] = h1->Nl ? h1->Nl : 1;
  }
  uint32_t maxA = p->TBS[0] / 8;
  if (d1 && p->TBS[1] / 8 > maxA) maxA = p->TBS[1] / 8;
  p->payload_stride = (maxA + 3 + 15) & ~15u;
}

/* dlsch_encoding for round != 0 (dlsch_coding.c:286, 383-406): no CRC, segmentation, coding or
 * interleaving; every block's stored w is rate-matched again with the round's rvidx.  The caller's
 * w[r] bytes are taken as they lie, Ncb <= 3 Kpi of them from the row's start: in the reference's
 * w[MAX_NUM_DLSCH_SEGMENTS][3 * 6144] a K = 6144 row (3 Kpi = 18528) runs into the next one, which
 * the first round's interleaver has overwritten, and that is what the reference reads.  One upload,
 * one launch (a workgroup per block), one download; only e[0..G) is written. */
static int dlsch_encoding_retx(const oai4g_frame_parms_t *fp, uint8_t num_pdcch_symbols, const oai4g_dlsch_t *dlsch,
                               oai4g_dl_harq_t *h, int frame, uint8_t subframe)
{
  const uint32_t C = h->C, Qm = oai4g_get_Qm(h->mcs), Nl = h->Nl ? h->Nl : 1;   /* Nl as the first round takes it */
  if (C < 1 || C > OAI4G_MAX_SEGMENTS || dlsch->Kmimo == 0 || dlsch->Mdlharq == 0) {
    set_err("dlsch_encoding: round %u with C %u, Nl %u, Kmimo %u, Mdlharq %u", h->round, C, Nl, dlsch->Kmimo, dlsch->Mdlharq);
    return -1;
  }
  const int Gi = oai4g_get_G(fp, h->nb_rb, h->rb_alloc, (uint8_t)Qm, (uint8_t)Nl, num_pdcch_symbols, frame, subframe);
  if (Gi <= 0 || Gi > OAI4G_MAX_CHANNEL_BITS) { set_err("dlsch_encoding: G=%d out of range", Gi); return -1; }
  const uint32_t G = (uint32_t)Gi;
  /* device layout: w rows | block descriptors | status words (uploaded as 0) | e: the upload ends
   * behind the status words and the download starts at them */
  rm_blk_t blk[OAI4G_MAX_SEGMENTS];
  memset(blk, 0, sizeof(blk));
  const size_t st_bytes = 4 * OAI4G_MAX_SEGMENTS;
  size_t wtot = 0;
  uint32_t etot = 0, max_Ncb = 0;
  for (uint32_t r = 0; r < C; r++) {
    const uint32_t RTC = h->RTC[r];
    const rm_ncb_t g = rm_ncb(OAI4G_NSOFT, dlsch->Kmimo, dlsch->Mdlharq, C, RTC);
    if (RTC == 0 || g.Kw > OAI4G_W_BYTES) { set_err("dlsch_encoding: RTC[%u] = %u", r, RTC); return -1; }
    if (g.shorter) {   /* lte_rate_matching_turbo returns 0: e untouched, r_offset stays (lte_rate_matching.c:518-521) */
      rm_condition_exit(g, OAI4G_NSOFT);
      continue;
    }
    const uint32_t Ncb = g.Ncb;
    blk[r].woff = (uint32_t)wtot;
    blk[r].Ncb = Ncb;
    blk[r].k0 = rm_k0(RTC, Ncb, h->rvidx);
    blk[r].E = rm_E(G, Nl, Qm, C, r);
    blk[r].eoff = etot;
    etot += blk[r].E;
    wtot += up256(Ncb);
    max_Ncb = Ncb > max_Ncb ? Ncb : max_Ncb;
  }
  if (etot == 0) return 0;
  if (etot > OAI4G_MAX_CHANNEL_BITS) { set_err("dlsch_encoding: %u e bits", etot); return -1; }
  stage_t st("dlsch_encoding");
  const int r_w = st.add(wtot), r_blk = st.add(sizeof(blk)), r_s = st.add(st_bytes), r_e = st.add(etot, 64);
  const size_t up_bytes = st.off[r_s] + st_bytes, e_at = st.off[r_e] - st.off[r_s];   /* host images follow the regions */
  std::vector<uint8_t> up(up_bytes, 0);
  for (uint32_t r = 0; r < C; r++)
    if (blk[r].E) memcpy(up.data() + blk[r].woff, h->w[r], blk[r].Ncb);
  memcpy(up.data() + st.off[r_blk], blk, sizeof(blk));
  if (!st.open()) return -1;
  HCK(st.up(r_w, up.data(), up_bytes, 0, r_s), -1);
  HCK(oai4g_launch_rm_bytes_blocks(st.ptr(r_w), st.ptr<const rm_blk_t>(r_blk), (int)C, max_Ncb, st.ptr(r_e),
                                   st.ptr<uint32_t>(r_s), g_scr.s), -1);
  std::vector<uint8_t> down(e_at + etot);
  HCK(st.down(down.data(), r_s, down.size(), 0, r_e), -1);
  HCK(st.sync(), -1);
  /* a row without a single non-NULL byte has nothing to repeat (the block's status word is 1, its e
   * bytes were not written): no stored w of a first round looks like that, so e stays as it was */
  uint32_t status[OAI4G_MAX_SEGMENTS];
  memcpy(status, down.data(), st_bytes);
  for (uint32_t r = 0; r < C; r++)
    if (status[r]) {
      set_err("dlsch_encoding: round %u, w[%u] holds no non-NULL entry below Ncb %u", h->round, r, blk[r].Ncb);
      return -1;
    }
  memcpy(h->e, down.data() + e_at, etot);
  return 0;
}

extern "C" int oai4g_dlsch_encoding(uint8_t *a, const oai4g_frame_parms_t *frame_parms, uint8_t num_pdcch_symbols,
                                    oai4g_dlsch_t *dlsch, int frame, uint8_t subframe)
{
  NEED_INIT(-1);
  oai4g_dl_harq_t *h = dlsch->harq_processes[dlsch->current_harq_pid];
  if (h->round != 0) return dlsch_encoding_retx(frame_parms, num_pdcch_symbols, dlsch, h, frame, subframe);
  oai4g_tx_params_t p;
  uint8_t Nl[2];
  params_from_dlsch(frame_parms, num_pdcch_symbols, dlsch, nullptr, subframe, &p, Nl);
  if (p.mimo_mode == OAI4G_ALAMOUTI || p.mimo_mode == OAI4G_LARGE_CDD || oai4g_mode_prec1(p.mimo_mode))
    p.mimo_mode = OAI4G_SISO; /* coding only */
  if (p.N_RB_DL != 6 && p.N_RB_DL != 15 && p.N_RB_DL != 25 && p.N_RB_DL != 50 && p.N_RB_DL != 100) return -1;
  oai4g_tx_config cfg;
  int rc = derive_cfg(&cfg, &p, Nl, false, -1);
  bool rm_fail = rc == -2; /* reference: every block's rate matcher returns E = 0, e untouched */
  if (rc != 0 && !rm_fail) return -1;
  cfg_scope_t scope;
  if (upload_cfg(&cfg) != 0) return -1;
  cw_dev_t &c = cfg.h.cw[0];
  uint32_t G = c.G[subframe % 10];
  /* payload | b | c | d | w | e, downloaded in one copy: the host image hb follows the regions */
  const size_t n_seg = OAI4G_MAX_SEGMENTS;                  /* 768 bytes a block */
  stage_t st("dlsch_encoding");
  const int r_pay = st.add(n_seg * 768, 4096), r_b = st.add(n_seg * 768, 4096), r_c = st.add(n_seg * (8 + 3 + 768));
  const int r_d = st.add(n_seg * OAI4G_D_BYTES), r_w = st.add(n_seg * OAI4G_W_BYTES), r_e = st.add(OAI4G_MAX_CHANNEL_BITS, 64);
  const size_t off_b = st.off[r_b], off_c = st.off[r_c], off_d = st.off[r_d], off_w = st.off[r_w], off_e = st.off[r_e];
  if (!st.open()) return -1;
  HCK(st.up(r_pay, a, c.A_bytes), -1);
  enc_debug_t dbg = {st.ptr(r_c), st.ptr(r_d), st.ptr(r_w), rm_fail ? nullptr : st.ptr(r_e), st.ptr(r_b)};
  HCK(oai4g_launch_encode_debug(cfg.d.get(), &cfg.h, 0, subframe % 10, st.ptr(r_pay), dbg, g_scr.s), -1);
  std::vector<uint8_t> hb(off_e + G);
  HCK(st.down(hb.data(), r_pay, off_e + G, 0, r_e), -1);
  HCK(st.sync(), -1);
  scope.done = true;
  /* CRC appended into the caller's buffer and copied to b (dlsch_coding.c:296-305) */
  memcpy(a + c.A_bytes, hb.data() + off_b + c.A_bytes, 3);
  h->B = c.TBS + 24;
  memcpy(h->b, a, c.A_bytes + 4); /* memcpy(b, a, A/8 + 4) (dlsch_coding.c:305) */
  h->C = c.C; h->Cplus = c.C - c.Cminus; h->Cminus = c.Cminus; h->Kplus = c.Kplus; h->Kminus = c.Kminus; h->F = c.F;
  for (uint32_t r = 0; r < c.C; r++) {
    uint32_t K = c.K[r];
    memcpy(h->c[r], hb.data() + off_c + r * (8 + 3 + 768), K / 8);
    memcpy(h->d[r], hb.data() + off_d + r * (size_t)OAI4G_D_BYTES, 96 + 3 * (K + 4) + 3);
    memcpy(h->w[r], hb.data() + off_w + r * (size_t)OAI4G_W_BYTES, 3 * c.Kpi[r]);
    h->RTC[r] = c.R[r];
  }
  if (!rm_fail) memcpy(h->e, hb.data() + off_e, G);
  return 0;
}

extern "C" void oai4g_dlsch_scrambling(const oai4g_frame_parms_t *frame_parms, int mbsfn_flag, oai4g_dlsch_t *dlsch,
                                       int G, uint8_t q, uint8_t Ns)
{
  NEED_INIT();
  uint8_t *e = dlsch->harq_processes[dlsch->current_harq_pid]->e;
  uint32_t x2 = mbsfn_flag == 0 ? ((uint32_t)dlsch->rnti << 14) + ((uint32_t)q << 13) + ((uint32_t)(Ns >> 1) << 9) +
                                      frame_parms->Nid_cell
                                : ((uint32_t)(Ns >> 1) << 9) + frame_parms->Nid_cell_mbsfn;   /* :70-72 */
  int n = (1 + (G >> 5)) * 32; /* the reference writes past G (dlsch_scrambling.c:83-92) */
  stage_t st("dlsch_scrambling");
  const int r_e = st.add((size_t)n, 64);      /* n covers the write past G */
  if (!st.open()) return;
  HCK(st.up(r_e, e, n), );
  HCK(oai4g_launch_scramble_bytes(st.ptr(r_e), n, x2, g_gx1, g_gx2j, g_scr.s), );
  HCK(st.down(e, r_e, n), );
  HCK(st.sync(), );
}

extern "C" int oai4g_dlsch_modulation(int32_t **txdataF, int16_t amp, uint32_t subframe_offset,
                                      const oai4g_frame_parms_t *frame_parms, uint8_t num_pdcch_symbols,
                                      oai4g_dlsch_t *dlsch0, oai4g_dlsch_t *dlsch1)
{
  NEED_INIT(-1);
  oai4g_tx_params_t p;
  uint8_t Nl[2];
  params_from_dlsch(frame_parms, num_pdcch_symbols, dlsch0, dlsch1, (uint8_t)(subframe_offset % 10), &p, Nl);
  const oai4g_dl_harq_t *h0 = dlsch0->harq_processes[dlsch0->current_harq_pid];
  if (h0->Nlayers > 1) return -1;
  p.amp = amp;
  if (p.mimo_mode == OAI4G_LARGE_CDD && !dlsch1) p.n_cw = 1;
  if (p.mimo_mode == OAI4G_ALAMOUTI) p.n_cw = 1;       /* both symbols of a pair come from dlsch0 */
  const bool prec1 = oai4g_mode_prec1(p.mimo_mode);
  if (p.mimo_mode != OAI4G_SISO && p.mimo_mode != OAI4G_LARGE_CDD && p.mimo_mode != OAI4G_ALAMOUTI && !prec1) {
    set_err("dlsch_modulation: mimo_mode %u not supported", p.mimo_mode);
    return -1;
  }
  if (prec1 && dlsch1) {
    set_err("dlsch_modulation: single-layer precoding (mimo_mode %u) takes one codeword", p.mimo_mode);
    return -1;
  }
  /* coding geometry is irrelevant here; use the grid-only derivation */
  oai4g_tx_config cfg;
  if (p.mimo_mode == OAI4G_LARGE_CDD && p.n_cw == 1) {
    set_err("LARGE_CDD with one codeword is not supported");
    return -1;
  }
  int rc = derive_cfg(&cfg, &p, Nl, true, (int)(subframe_offset % 10));
  if (rc != 0 && rc != -2) return -1;
  cfg_scope_t scope;
  if (upload_cfg(&cfg) != 0) return -1;
  int sf = (int)(subframe_offset % 10);
  uint32_t N = cfg.h.N, nsymb = cfg.h.nsymb, nant = cfg.h.n_ant;
  const size_t ant_bytes = (size_t)nsymb * N * 4;
  uint32_t n_re = (uint32_t)cfg.re_count[sf];
  const size_t e0_bytes = (size_t)n_re * cfg.h.cw[0].Qm, e1_bytes = p.n_cw > 1 ? (size_t)n_re * cfg.h.cw[1].Qm : 0;
  stage_t st("dlsch_modulation");
  const int r_grid = st.add(nant * ant_bytes);
  /* k_modulate_bytes loads 4 unaligned bytes past n_re Qm: 64 each; the last 64 have no known reader */
  const int r_e0 = st.add(e0_bytes, 64), r_e1 = st.add(e1_bytes, 64 + 64);
  if (!st.open()) return -1;
  size_t sym_off = (size_t)N * subframe_offset * nsymb;
  for (uint32_t aa = 0; aa < nant; aa++) HCK(st.up(r_grid, txdataF[aa] + sym_off, ant_bytes, aa * ant_bytes), -1);
  HCK(st.up(r_e0, h0->e, e0_bytes), -1);
  if (p.n_cw > 1) HCK(st.up(r_e1, dlsch1->harq_processes[dlsch0->current_harq_pid]->e, e1_bytes), -1);
  HCK(oai4g_launch_modulate_bytes(cfg.d.get(), &cfg.h, sf, st.ptr(r_e0), p.n_cw > 1 ? st.ptr(r_e1) : nullptr,
                                  st.ptr<int32_t>(r_grid), g_scr.s), -1);
  for (uint32_t aa = 0; aa < nant; aa++) HCK(st.down(txdataF[aa] + sym_off, r_grid, ant_bytes, aa * ant_bytes), -1);
  HCK(st.sync(), -1);
  scope.done = true;
  return cfg.re_alloc[sf];
}

/* ------------------------------------------------------------------------------------------
 * drop-in OFDM entry points
 * ---------------------------------------------------------------------------------------- */
static int run_ofdm(const int32_t *input, size_t in_n, int32_t *output, size_t out_lo, size_t out_n, int log2n,
                    int nsym, const ofdm_sym_t *syms, int scale)
{
  NEED_INIT(-1);
  stage_t st("ofdm");
  const int r_in = st.add(in_n * 4), r_out = st.add(out_n * 4, 64);
  if (!st.open()) return -1;
  HCK(st.up(r_in, input, in_n * 4), -1);
  /* the output window is read-modify-write: samples outside the written symbols stay intact */
  HCK(st.up(r_out, output + out_lo, out_n * 4), -1);
  HCK(oai4g_launch_ofdm(st.ptr<int32_t>(r_in), st.ptr<int32_t>(r_out), log2n, nsym, syms, scale, g_tw, g_scr.s), -1);
  HCK(st.down(output + out_lo, r_out, out_n * 4), -1);
  HCK(st.sync(), -1);
  return 0;
}

static bool log2n_ok(int l) { return l >= 6 && l <= 11; }
/* PHY_ofdm_mod's switch (ofdm_mod.c:103-127) names idft128..idft2048; any other size falls to its
 * default (idft512 over a 2^log2 stride, overlapping symbols), which the drop-in refuses instead */
static bool ofdm_log2_ok(int l) { return l >= 7 && l <= 11; }

extern "C" void oai4g_PHY_ofdm_mod(const int32_t *input, int32_t *output, uint8_t log2fftsize, uint8_t nb_symbols,
                                   uint16_t nb_prefix_samples, int etype)
{
  if (etype != OAI4G_CYCLIC_PREFIX) {
    set_err("PHY_ofdm_mod: only CYCLIC_PREFIX is supported");
    return;
  }
  if (!ofdm_log2_ok(log2fftsize) || nb_symbols == 0 || nb_symbols > 28) {
    set_err("PHY_ofdm_mod: unsupported size 2^%u or symbol count %u", log2fftsize, nb_symbols);
    return;
  }
  ofdm_sym_t syms[28];
  uint32_t N = 1u << log2fftsize;
  if (nb_prefix_samples > N) { /* the CP loop (ofdm_mod.c:167-171) would read in front of the symbol */
    set_err("PHY_ofdm_mod: prefix %u longer than the symbol", nb_prefix_samples);
    return;
  }
  for (int i = 0; i < nb_symbols; i++) {
    syms[i].in_off = (uint32_t)i * N;
    syms[i].out_off = (uint32_t)i * N + (uint32_t)(1 + i) * nb_prefix_samples;
    syms[i].cp = nb_prefix_samples;
  }
  size_t out_n = (size_t)nb_symbols * (N + nb_prefix_samples);
  run_ofdm(input, (size_t)nb_symbols * N, output, 0, out_n, log2fftsize, nb_symbols, syms, 1);
}

/* one slot = symbol 0 with CP0, then symbols 1..nsymb-1 with CP, in a single launch */
static void slot_syms(const oai4g_frame_parms_t *fp, uint32_t in_base, uint32_t out_base, int nsym_slot,
                      ofdm_sym_t *syms)
{
  uint32_t N = fp->ofdm_symbol_size;
  syms[0].in_off = in_base;
  syms[0].out_off = out_base + fp->nb_prefix_samples0;
  syms[0].cp = fp->nb_prefix_samples0;
  for (int i = 1; i < nsym_slot; i++) {
    syms[i].in_off = in_base + (uint32_t)i * N;
    syms[i].out_off = out_base + N + fp->nb_prefix_samples0 + (uint32_t)(i - 1) * N + (uint32_t)i * fp->nb_prefix_samples;
    syms[i].cp = fp->nb_prefix_samples;
  }
}

extern "C" void oai4g_normal_prefix_mod(const int32_t *txdataF, int32_t *txdata, uint8_t nsymb,
                                        const oai4g_frame_parms_t *fp)
{
  if (!ofdm_log2_ok(fp->log2_symbol_size)) { set_err("normal_prefix_mod: unsupported FFT size"); return; }
  uint32_t N = fp->ofdm_symbol_size;
  int short_offset = (2 * nsymb) < fp->symbols_per_tti;
  int nslots = short_offset + 2 * nsymb / fp->symbols_per_tti;
  ofdm_sym_t syms[28];
  int ns = 0;
  for (int i = 0; i < nslots; i++) {
    int per = short_offset ? 2 : (fp->symbols_per_tti >> 1);
    slot_syms(fp, (uint32_t)((i * N * fp->symbols_per_tti) >> 1), (uint32_t)((i * fp->samples_per_tti) >> 1), per,
              syms + ns);
    ns += per;
  }
  uint32_t in_n = 0, out_hi = 0;
  for (int i = 0; i < ns; i++) {
    in_n = syms[i].in_off + N > in_n ? syms[i].in_off + N : in_n;
    out_hi = syms[i].out_off + N > out_hi ? syms[i].out_off + N : out_hi;
  }
  run_ofdm(txdataF, in_n, txdata, 0, out_hi, fp->log2_symbol_size, ns, syms, 1);
}

extern "C" void oai4g_do_OFDM_mod(int32_t **txdataF, int32_t **txdata, uint32_t frame, uint16_t next_slot,
                                  const oai4g_frame_parms_t *fp)
{
  (void)frame;
  uint32_t slot_offset_F = (uint32_t)next_slot * fp->ofdm_symbol_size * (fp->Ncp == 1 ? 6 : 7);
  uint32_t slot_offset = (uint32_t)next_slot * (fp->samples_per_tti >> 1);
  for (int aa = 0; aa < fp->nb_antennas_tx; aa++) {
    if (fp->Ncp == 1)
      oai4g_PHY_ofdm_mod(txdataF[aa] + slot_offset_F, txdata[aa] + slot_offset, fp->log2_symbol_size, 6,
                         fp->nb_prefix_samples, OAI4G_CYCLIC_PREFIX);
    else
      oai4g_normal_prefix_mod(txdataF[aa] + slot_offset_F, txdata[aa] + slot_offset, 7, fp);
  }
}

/* ------------------------------------------------------------------------------------------
 * Cell-specific reference signals (pilots.c:43-168, lte_dl_cell_spec.c:123-203)
 * ---------------------------------------------------------------------------------------- */
static int run_crs(int32_t *const *grids, int n_grids, size_t grid_res, const crs_job_t *jobs, int n_jobs, int16_t amp,
                   const oai4g_frame_parms_t *fp)
{
  uint32_t gt[20][2][14];
  lte_gold_table_h(fp, gt);
  const size_t gbytes = sizeof(gt), jbytes = (size_t)n_jobs * sizeof(crs_job_t), dbytes = (size_t)n_grids * grid_res * 4;
  stage_t st("crs");
  const int r_gold = st.add(gbytes), r_jobs = st.add(jbytes), r_grid = st.add(dbytes, 256);
  if (!st.open()) return -1;
  HCK(st.up(r_gold, gt, gbytes), -1);
  HCK(st.up(r_jobs, jobs, jbytes), -1);
  for (int g = 0; g < n_grids; g++) HCK(st.up(r_grid, grids[g], grid_res * 4, g * grid_res * 4), -1);
  HCK(oai4g_launch_crs(st.ptr<int32_t>(r_grid), st.ptr<crs_job_t>(r_jobs), n_jobs, st.ptr<uint32_t>(r_gold), amp,
                       fp->ofdm_symbol_size, fp->N_RB_DL, fp->nushift, fp->first_carrier_offset, g_scr.s), -1);
  for (int g = 0; g < n_grids; g++) HCK(st.down(grids[g], r_grid, grid_res * 4, g * grid_res * 4), -1);
  HCK(st.sync(), -1);
  return 0;
}

extern "C" void oai4g_generate_pilots(int32_t **txdataF, int16_t amp, const oai4g_frame_parms_t *fp, uint16_t Ntti)
{
  NEED_INIT();
  const uint32_t N = fp->ofdm_symbol_size, Nsymb = fp->Ncp == 0 ? 14 : 12, second = fp->Ncp == 0 ? 4 : 3;
  const int n_ant = fp->nb_antennas_tx > 1 ? 2 : 1;
  std::vector<crs_job_t> jobs;
  for (uint32_t tti = 0; tti < Ntti; tti++) {
    const uint32_t base = tti * N * Nsymb, slot = (tti * 2) % 20;
    const uint32_t sym[4] = {0, second, Nsymb >> 1, (Nsymb >> 1) + second};
    for (int i = 0; i < 4; i++)
      for (int a = 0; a < n_ant; a++) {
        const size_t grid_res = (size_t)Ntti * N * Nsymb;
        crs_job_t j;
        j.off = (uint32_t)(a * grid_res + base + sym[i] * N);
        j.Ns = (uint8_t)(slot + (i >> 1));
        j.l = (uint8_t)(i & 1);
        j.p = (uint8_t)(a == 0 || fp->mode1_flag ? 0 : 1);
        j.pad = 0;
        jobs.push_back(j);
      }
  }
  run_crs(txdataF, n_ant, (size_t)Ntti * N * Nsymb, jobs.data(), (int)jobs.size(), amp, fp);
}

extern "C" int oai4g_lte_dl_cell_spec(int32_t *output, int16_t amp, const oai4g_frame_parms_t *fp, uint8_t Ns,
                                      uint8_t l, uint8_t p)
{
  NEED_INIT(-1);
  if (p > 1 || l > 1 || Ns >= 20) {
    set_err("lte_dl_cell_spec: p %d, l %d -> ERROR", p, l);
    return -1;
  }
  crs_job_t j = {0, Ns, l, p, 0};
  return run_crs(&output, 1, fp->ofdm_symbol_size, &j, 1, amp, fp);
}

/* ------------------------------------------------------------------------------------------
 * Uplink turbo decoding (3gpplte_turbo_decoder_sse_16bit.c, lte_rate_matching.c)
 * ---------------------------------------------------------------------------------------- */
/* init_td16 (:898-943; 8 windows) and init_td8 (3gpplte_turbo_decoder_sse_8bit.c:846-892; 16 windows,
 * K % 16 == 0) for block size K: pi4 | pi5 | pi6 as uint16.  Window w holds the K / windows positions
 * w, w + windows, …; uploaded once per (K, windows) and kept as long as the process. */
static const uint16_t *td_tables(uint32_t K, uint32_t windows = 8)
{
  static std::mutex mu;
  static std::map<std::pair<uint32_t, uint32_t>, uint16_t *> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({K, windows});
  if (it != cache.end()) return it->second;
  const int qi = oai4g_qpp_index(K);
  if (qi < 0 || K % windows) return nullptr;
  const uint64_t f1 = oai4g_qpp_table[qi].f1, f2 = oai4g_qpp_table[qi].f2;
  std::vector<uint32_t> pi2(K);
  for (uint32_t i = 0, j = 0; i < K; i++, j += windows) {
    if (j >= K) j -= (K - 1);
    pi2[i] = j;
  }
  std::vector<uint16_t> t(3 * (size_t)K);
  for (uint32_t i = 0; i < K; i++) {
    const uint32_t pi = (uint32_t)((f1 * i + f2 * (uint64_t)i * i) % K), pi3 = pi2[pi];
    t[pi2[i]] = (uint16_t)pi3;          /* pi4 */
    t[K + pi3] = (uint16_t)pi2[i];      /* pi5 */
    t[2 * K + pi] = (uint16_t)pi2[i];   /* pi6 */
  }
  dev_buf<uint16_t> d;
  if (d.upload(t) != hipSuccess) {
    set_err("decoder table upload failed");
    return nullptr;
  }
  return cache[{K, windows}] = d.release();
}
static const uint16_t *td8_tables(uint32_t K) { return td_tables(K, 16); }

extern "C" size_t oai4g_td8_scratch_bytes(uint16_t K, int n_cb) { return (size_t)((n_cb + 3) / 4) * oai4g_td8_wave_bytes(K); }

extern "C" int oai4g_td8_batch(int n_cb, uint16_t K, const int16_t *d_llr, size_t llr_stride, uint8_t *d_out,
                               size_t out_stride, uint8_t *d_iters, uint8_t max_iterations, uint8_t crc_type, uint8_t F,
                               void *d_scratch, void *stream)
{
  NEED_INIT(-1);
  if (crc_type > OAI4G_CRC24_B) { set_err("turbo decoder8: only CRC24_A / CRC24_B are on the path"); return -1; }
  if ((K & 15) || K < 512 || oai4g_qpp_index(K) < 0) {
    set_err("turbo decoder8: K %u outside n %% 16 == 0, n >= 512 (the reference reads past its tables there)", K);
    return -1;
  }
  if ((F & 7) || F + 24 > K) { set_err("turbo decoder8: filler F=%u unsupported", F); return -1; }
  if (llr_stride < 3 * (size_t)K + 16) { set_err("turbo decoder8: llr_stride < 3K + 16"); return -1; }
  const uint16_t *pi = td8_tables(K);
  if (!pi) return -1;
  HCK(oai4g_launch_td8(n_cb, K, d_llr, llr_stride, d_out, out_stride, d_iters, max_iterations, crc_type, F, pi,
                       (uint8_t *)d_scratch, (hipStream_t)stream), -1);
  return 0;
}

/* phy_threegpplte_turbo_decoder8 drop-in: y = 3n + 12 int16 (the reference's conversion reads 4 more
 * entries; they only reach its unused tail and are taken as 0 here); decoded_bytes n/8 bytes. */
extern "C" uint8_t oai4g_phy_threegpplte_turbo_decoder8(const int16_t *y, uint8_t *decoded_bytes, uint16_t n,
                                                       uint16_t f1, uint16_t f2, uint8_t max_iterations,
                                                       uint8_t crc_type, uint8_t F)
{
  (void)f1;
  (void)f2;
  if (oai4g_init() != 0) return 255;
  if ((n & 15) || n < 512 || oai4g_qpp_index(n) < 0 || crc_type > OAI4G_CRC24_B) {
    set_err("turbo decoder8: n %u / crc %u outside the restated scope", n, crc_type);
    return 255;
  }
  const size_t ly = 3 * (size_t)n + 16;
  stage_t st("turbo decoder8");
  const int r_y = st.add(ly * 2), r_out = st.add((size_t)n / 8, 256), r_it = st.add(1, 255);
  const int r_scr = st.add(oai4g_td8_scratch_bytes(n, 1));
  if (!st.open()) return 255;
  std::vector<int16_t> h(ly, 0);
  memcpy(h.data(), y, (3 * (size_t)n + 12) * 2);
  uint8_t itc = 255;
  HCK(st.up(r_y, h.data(), ly * 2), 255);
  HCK(st.up(r_out, decoded_bytes, n / 8), 255);
  if (oai4g_td8_batch(1, n, st.ptr<int16_t>(r_y), ly, st.ptr(r_out), n / 8, st.ptr(r_it), max_iterations, crc_type, F,
                      st.ptr(r_scr), g_scr.s) != 0)
    return 255;
  HCK(st.down(decoded_bytes, r_out, n / 8), 255);
  HCK(st.down(&itc, r_it, 1), 255);
  HCK(st.sync(), 255);
  return itc;
}

/* per wave of 8 blocks (the decoder interleaves a wave's blocks in its scratch) */
extern "C" size_t oai4g_td_scratch_bytes(uint16_t K, int n_cb) { return (size_t)((n_cb + 7) & ~7) * oai4g_td_block_bytes(K); }

extern "C" int oai4g_td_batch(int n_cb, uint16_t K, const int16_t *d_llr, size_t llr_stride, uint8_t *d_out,
                              size_t out_stride, uint8_t *d_iters, uint8_t max_iterations, uint8_t crc_type, uint8_t F,
                              void *d_scratch, void *stream)
{
  NEED_INIT(-1);
  if (crc_type > OAI4G_CRC24_B) { set_err("turbo decoder: only CRC24_A / CRC24_B are on the path"); return -1; }
  if ((F & 7) || F + 24 > K) { set_err("turbo decoder: filler F=%u unsupported", F); return -1; }
  const uint16_t *pi = td_tables(K);
  if (!pi) { set_err("Illegal frame length %u", K); return -1; }
  HCK(oai4g_launch_td16(n_cb, K, d_llr, llr_stride, d_out, out_stride, d_iters, max_iterations, crc_type, F, pi,
                        (uint8_t *)d_scratch, (hipStream_t)stream), -1);
  return 0;
}

/* generate_dummy_w (lte_rate_matching.c:293-382): LTE_NULL marks of the 3 Kpi circular buffer of a
 * block of D = K + 4 bits with F filler bits; returns R (RTC) */
static uint32_t dummy_w_h(uint32_t D, uint32_t F, std::vector<uint8_t> &w)
{
  const uint32_t R = (D >> 5) + ((D & 31) ? 1 : 0), Kpi = R << 5, ND = Kpi - D;
  w.assign(3 * (size_t)Kpi, 0);
  for (uint32_t col = 0, k = 0; col < 32; col++, k += R) {
    const uint32_t index = __builtin_bitreverse32(col) >> 27;
    if (index < ND + F) { w[k] = OAI4G_LTE_NULL; w[Kpi + 2 * k] = OAI4G_LTE_NULL; }
    if (index + 32 < ND + F) { w[k + 1] = OAI4G_LTE_NULL; w[Kpi + 2 + 2 * k] = OAI4G_LTE_NULL; }
    if (index + 64 < ND + F) { w[k + 2] = OAI4G_LTE_NULL; w[Kpi + 4 + 2 * k] = OAI4G_LTE_NULL; }
    if (index + 1 < ND) w[Kpi + 1 + 2 * k] = OAI4G_LTE_NULL;
  }
  if (ND > 0) w[3 * Kpi - 1] = OAI4G_LTE_NULL;
  return R;
}

extern "C" uint32_t oai4g_generate_dummy_w(uint32_t D, uint8_t *w, uint8_t F)
{
  std::vector<uint8_t> v;
  const uint32_t R = dummy_w_h(D, F, v);
  for (size_t i = 0; i < v.size(); i++)
    if (v[i] == OAI4G_LTE_NULL) w[i] = OAI4G_LTE_NULL;   /* the reference only writes the NULL marks */
  return R;
}

/* compact (non-NULL) index of every position of w[0..Ncb) under generate_dummy_w's mask: the kernels' cidx table */
static std::vector<uint32_t> rm_compact_index(const uint8_t *dw, uint32_t Ncb)
{
  std::vector<uint32_t> cidx(Ncb);
  for (uint32_t q = 0, nn = 0; q < Ncb; q++) {
    cidx[q] = nn;
    nn += dw[q] != OAI4G_LTE_NULL ? 1u : 0u;
  }
  return cidx;
}

/* the receive side's compacted start of redundancy version rv (lte_rate_matching.c:743-745); with k0 >= Ncb the
 * reference's first pass is empty and the selection starts at 0 */
static uint32_t rm_rx_k0c(const uint8_t *dw, uint32_t R, uint32_t Ncb, uint32_t rv)
{
  const uint32_t k0 = rm_k0(R, Ncb, rv);
  return k0 >= Ncb ? 0 : rm_compact(k0, rm_null_mask{dw, OAI4G_LTE_NULL});
}

/* ------------------------------------------------------------------------------------------
 * Batched UL receive chain (ulsch_decoding.c:1208-1350): n_tb transport blocks of one
 * configuration, e soft bits -> RM-rx + sub-block deinterleaving (k_ul_rm_deint) -> 16-bit turbo
 * decoding (k_td16, one launch per block size) with CRC24B / CRC24A early stop.
 * ---------------------------------------------------------------------------------------- */
struct oai4g_ul_config {
  ul_dev_t h;
  dev_buf<ul_dev_t> d;
  uint32_t B, G, C, Cminus, Kminus, Kplus, F, max_it;
  dev_buf<uint8_t> d_dummy[3];    /* ul_pat_t::dummy / cidx of each pattern */
  dev_buf<uint32_t> d_cidx[3];
  size_t d_stride = 0;
  dev_buf<int16_t> d_dfull;       /* the work buffers, sized by the largest batch so far (ul_reserve) */
  dev_buf<uint8_t> d_td;
  int bits = 16;                  /* 16: phy_threegpplte_turbo_decoder16; 8: the 8-bit decoder (llr8_flag) */
};

extern "C" void oai4g_ul_config_destroy(oai4g_ul_config_t *cfg)
{
  if (cfg) delete cfg;
}

extern "C" oai4g_ul_config_t *oai4g_ul_config_create(uint32_t B, uint32_t G, uint8_t Qm, uint8_t rvidx, uint8_t Mdlharq,
                                                     uint32_t Nsoft, uint8_t max_iterations)
{
  NEED_INIT(nullptr);
  std::unique_ptr<oai4g_ul_config> cfg(new oai4g_ul_config());
  uint32_t Cplus, L;
  if (Qm == 0 || Mdlharq == 0 || rvidx > 3 ||
      seg_params(B, &cfg->C, &Cplus, &cfg->Cminus, &cfg->Kplus, &cfg->Kminus, &cfg->F, &L) < 0 ||
      cfg->C > OAI4G_UL_MAX_C || (cfg->F & 7) || cfg->F + 24 > cfg->Kplus) {
    set_err("ul_config: unsupported (B %u, Qm %u, rv %u, Mdlharq %u)", B, Qm, rvidx, Mdlharq);
    return nullptr;
  }
  cfg->B = B;
  cfg->G = G;
  cfg->max_it = max_iterations;
  ul_dev_t &h = cfg->h;
  memset(&h, 0, sizeof(h));
  h.C = cfg->C;
  const uint32_t C = cfg->C;
  uint32_t off = 0, npat = 0, keyK[3] = {0, 0, 0}, keyF[3] = {0, 0, 0};
  for (uint32_t r = 0; r < C; r++) {
    h.E[r] = rm_E(G, 1, Qm, C, r);   /* Nl = 1 */
    h.off[r] = off;
    off += h.E[r];
    const uint32_t K = r < cfg->Cminus ? cfg->Kminus : cfg->Kplus, Fr = r == 0 ? cfg->F : 0;
    uint32_t pi = 0;
    while (pi < npat && !(keyK[pi] == K && keyF[pi] == Fr)) pi++;
    if (pi == npat) {
      keyK[npat] = K;
      keyF[npat] = Fr;
      dev_buf<uint8_t> &dd = cfg->d_dummy[npat];
      dev_buf<uint32_t> &dc = cfg->d_cidx[npat];
      ul_pat_t &P = h.pat[npat++];
      std::vector<uint8_t> dw;
      P.D = K + 4;
      P.R = dummy_w_h(P.D, Fr, dw);
      P.Ncb = rm_ncb(Nsoft, 1, Mdlharq, C, P.R).Ncb;   /* Kmimo = 1 */
      const std::vector<uint32_t> cidx = rm_compact_index(dw.data(), P.Ncb);
      P.Nnn = rm_compact(P.Ncb, rm_null_mask{dw.data(), OAI4G_LTE_NULL});
      for (uint32_t rv = 0; rv < 4; rv++)          /* every round's k0 (lte_rate_matching.c:743-745) */
        P.k0cr[rv] = rm_rx_k0c(dw.data(), P.R, P.Ncb, rv);
      P.k0c = P.k0cr[rvidx];
      if (P.R > h.Rmax) h.Rmax = P.R;
      if (dd.upload(dw) != hipSuccess || dc.upload(cidx) != hipSuccess) {
        set_err("ul_config: device allocation failed");
        return nullptr;
      }
      P.dummy = dd.get();
      P.cidx = dc.get();
    }
    h.pat_of[r] = pi;
  }
  if (!td_tables(cfg->Kplus) || (cfg->Cminus && !td_tables(cfg->Kminus))) return nullptr;
  cfg->d_stride = (96 + 3 * (size_t)cfg->Kplus + 12 + 15) & ~(size_t)15;
  if (cfg->d.upload(&h, 1) != hipSuccess) {
    set_err("ul_config: upload failed");
    return nullptr;
  }
  return cfg.release();
}

extern "C" int oai4g_ul_config_set_decoder(oai4g_ul_config_t *cfg, int bits)
{
  if (!cfg || (bits != 8 && bits != 16)) { set_err("ul_config_set_decoder: bits must be 8 or 16"); return -1; }
  if (bits == 8 && (cfg->Cminus || (cfg->Kplus & 15) || cfg->Kplus < 512 || (cfg->C == 1 && (cfg->F & 7)))) {
    set_err("ul_config_set_decoder: the 8-bit decoder needs one block size K %% 16 == 0, K >= 512 (K %u, C- %u)",
            cfg->Kplus, cfg->Cminus);
    return -1;
  }
  if (bits != cfg->bits) {          /* the scratch size differs: reallocate on the next batch */
    cfg->d_dfull.reset();
    cfg->d_td.reset();
  }
  cfg->bits = bits;
  return 0;
}

extern "C" int oai4g_ul_config_C(const oai4g_ul_config_t *cfg) { return (int)cfg->C; }
extern "C" uint32_t oai4g_ul_config_G_offset(const oai4g_ul_config_t *cfg, int r) { return cfg->h.off[r]; }
extern "C" uint32_t oai4g_ul_config_E(const oai4g_ul_config_t *cfg, int r) { return cfg->h.E[r]; }

static int ul_reserve(oai4g_ul_config_t *cfg, int n_tb)
{
  const size_t nb = (size_t)n_tb * cfg->C;
  const size_t td = cfg->bits == 8 ? oai4g_td8_scratch_bytes((uint16_t)cfg->Kplus, (int)nb)
                                   : oai4g_td_scratch_bytes((uint16_t)cfg->Kplus, (int)nb);
  /* the two grow together: free both before either is allocated anew */
  if (nb * cfg->d_stride > cfg->d_dfull.count()) cfg->d_td.reset();
  if (cfg->d_dfull.reserve(nb * cfg->d_stride) != hipSuccess || cfg->d_td.reserve(td) != hipSuccess) {
    set_err("ul_decode_batch: device allocation failed");
    return -1;
  }
  return 0;
}

/* the decoders over the deinterleaved rows (one launch per block size) */
static int ul_decode_rows(oai4g_ul_config_t *cfg, int n_tb, uint8_t *d_c, size_t c_stride, uint8_t *d_iters,
                          hipStream_t s)
{
  const uint32_t crc = cfg->C == 1 ? OAI4G_CRC24_A : OAI4G_CRC24_B, F = cfg->C == 1 ? cfg->F : 0;
  const int16_t *y = cfg->d_dfull.get() + 96;
  if (cfg->bits == 8) {
    /* every block of one size (set_decoder checked), rows (tb, r) in the d_c / d_iters order */
    const uint16_t *pi = td8_tables(cfg->Kplus);
    if (!pi) return -1;
    HCK(oai4g_launch_td8(n_tb * (int)cfg->C, cfg->Kplus, y, cfg->d_stride, d_c, c_stride, d_iters, cfg->max_it, crc, F,
                         pi, cfg->d_td.get(), s), -1);
    return 0;
  }
  if (cfg->Cminus)
    HCK(oai4g_launch_td16(n_tb * (int)cfg->Cminus, cfg->Kminus, y, cfg->d_stride, d_c, c_stride, d_iters, cfg->max_it,
                          crc, F, td_tables(cfg->Kminus), cfg->d_td.get(), s, cfg->Cminus, cfg->C, 0), -1);
  HCK(oai4g_launch_td16(n_tb * (int)(cfg->C - cfg->Cminus), cfg->Kplus, y, cfg->d_stride, d_c, c_stride, d_iters,
                        cfg->max_it, crc, F, td_tables(cfg->Kplus), cfg->d_td.get(), s, cfg->C - cfg->Cminus, cfg->C,
                        cfg->Cminus), -1);
  return 0;
}

/* what the three batch entry points share: the stride checks (the caller words the error), and after the caller's own
 * checks the work buffers, its rate-matching launch into cfg->d_dfull (0 or -1 with the error set) and the decoders */
static bool ul_strides_ok(const oai4g_ul_config_t *cfg, size_t c_stride, size_t e_stride)
{
  return c_stride >= cfg->Kplus / 8 && e_stride >= cfg->G;
}

template <typename LaunchRm>
static int ul_batch(oai4g_ul_config_t *cfg, int n_tb, uint8_t *d_c, size_t c_stride, uint8_t *d_iters, void *stream,
                    LaunchRm launch_rm)
{
  if (ul_reserve(cfg, n_tb) != 0) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (launch_rm(s) != 0) return -1;
  return ul_decode_rows(cfg, n_tb, d_c, c_stride, d_iters, s);
}

extern "C" int oai4g_ul_decode_batch(oai4g_ul_config_t *cfg, int n_tb, const int16_t *d_e, size_t e_stride,
                                     uint8_t *d_c, size_t c_stride, uint8_t *d_iters, void *stream)
{
  NEED_INIT(-1);
  if (n_tb <= 0) return 0;
  if (!ul_strides_ok(cfg, c_stride, e_stride)) { set_err("ul_decode_batch: strides too small"); return -1; }
  return ul_batch(cfg, n_tb, d_c, c_stride, d_iters, stream, [&](hipStream_t s) {
    HCK(oai4g_launch_ul_rm_deint(cfg->d.get(), &cfg->h, n_tb, d_e, e_stride, cfg->d_dfull.get(), cfg->d_stride, s), -1);
    return 0;
  });
}

extern "C" size_t oai4g_ul_config_w_entries(const oai4g_ul_config_t *cfg) { return 3 * ((size_t)cfg->h.Rmax << 5); }

/* the batch with HARQ soft combining: the decoders' input comes from the caller's per-block soft
 * buffers d_w, updated in place by this round (dlsch_decoding.c:348-383, ulsch_decoding.c:1262-1294) */
extern "C" int oai4g_ul_decode_batch_harq(oai4g_ul_config_t *cfg, int n_tb, const int16_t *d_e, size_t e_stride,
                                          int16_t *d_w, size_t w_stride, uint8_t rvidx, uint8_t clear, uint8_t *d_c,
                                          size_t c_stride, uint8_t *d_iters, void *stream)
{
  NEED_INIT(-1);
  if (n_tb <= 0) return 0;
  if (rvidx > 3 || clear > 1) { set_err("ul_decode_batch_harq: rvidx 0..3, clear 0 / 1"); return -1; }
  if (!ul_strides_ok(cfg, c_stride, e_stride) || w_stride < oai4g_ul_config_w_entries(cfg)) {
    set_err("ul_decode_batch_harq: strides too small");
    return -1;
  }
  return ul_batch(cfg, n_tb, d_c, c_stride, d_iters, stream, [&](hipStream_t s) {
    HCK(oai4g_launch_ul_rm_harq(cfg->d.get(), &cfg->h, n_tb, d_e, e_stride, d_w, w_stride, rvidx, clear,
                                cfg->d_dfull.get(), cfg->d_stride, s), -1);
    return 0;
  });
}

/* the same round with rv and clear per transport block (device arrays [n_tb]) */
extern "C" int oai4g_ul_decode_batch_harq_tb(oai4g_ul_config_t *cfg, int n_tb, const int16_t *d_e, size_t e_stride,
                                             int16_t *d_w, size_t w_stride, const uint8_t *d_rv, const uint8_t *d_clear,
                                             uint8_t *d_c, size_t c_stride, uint8_t *d_iters, void *stream)
{
  NEED_INIT(-1);
  if (n_tb <= 0) return 0;
  if (!cfg || !d_rv || !d_clear) { set_err("ul_decode_batch_harq_tb: null configuration, rv or clear array"); return -1; }
  if (!ul_strides_ok(cfg, c_stride, e_stride) || w_stride < oai4g_ul_config_w_entries(cfg)) {
    set_err("ul_decode_batch_harq_tb: strides too small");
    return -1;
  }
  return ul_batch(cfg, n_tb, d_c, c_stride, d_iters, stream, [&](hipStream_t s) {
    HCK(oai4g_launch_ul_rm_harq_tb(cfg->d.get(), &cfg->h, n_tb, d_e, e_stride, d_w, w_stride, d_rv, d_clear,
                                   cfg->d_dfull.get(), cfg->d_stride, s), -1);
    return 0;
  });
}

extern "C" uint8_t oai4g_phy_threegpplte_turbo_decoder16(const int16_t *y, uint8_t *decoded_bytes, uint16_t n,
                                                         uint16_t f1, uint16_t f2, uint8_t max_iterations,
                                                         uint8_t crc_type, uint8_t F)
{
  NEED_INIT(255);
  (void)f1; (void)f2;   /* the reference also selects its tables by n (:986) */
  if (crc_type > 3) { set_err("Illegal crc length!"); return 255; }
  if (oai4g_qpp_index(n) < 0) { set_err("Illegal frame length!"); return 255; }
  if (crc_type > OAI4G_CRC24_B) { set_err("turbo decoder: CRC16 / CRC8 are not on the path"); return 255; }
  const size_t ybytes = (3 * (size_t)n + 12) * 2, sbytes = oai4g_td_scratch_bytes(n, 1);
  stage_t st("turbo decoder");
  const int r_y = st.add(ybytes), r_it = st.add(1, 255), r_out = st.add((size_t)n / 8), r_scr = st.add(sbytes, 768);
  if (!st.open()) return 255;
  HCK(st.up(r_y, y, ybytes), 255);
  HCK(st.up(r_out, decoded_bytes, n / 8), 255);            /* untouched if never decided */
  if (oai4g_td_batch(1, n, st.ptr<int16_t>(r_y), 3 * (size_t)n + 12, st.ptr(r_out), n / 8, st.ptr(r_it), max_iterations,
                     crc_type, F, st.ptr(r_scr), g_scr.s))
    return 255;
  uint8_t it = 0;
  HCK(st.down(decoded_bytes, r_out, n / 8), 255);
  HCK(st.down(&it, r_it, 1), 255);
  HCK(st.sync(), 255);
  return it;
}

extern "C" int oai4g_lte_rate_matching_turbo_rx(uint32_t RTC, uint32_t G, int16_t *w, const uint8_t *dummy_w,
                                                const int16_t *soft_input, uint8_t C, uint32_t Nsoft, uint8_t Mdlharq,
                                                uint8_t Kmimo, uint8_t rvidx, uint8_t clear, uint8_t Qm, uint8_t Nl,
                                                uint8_t r, uint32_t *E_out)
{
  NEED_INIT(-1);
  if (Kmimo == 0 || Mdlharq == 0 || C == 0 || Qm == 0 || Nl == 0) return -1;
  const uint32_t Ncb = rm_ncb(Nsoft, Kmimo, Mdlharq, C, RTC).Ncb, E = rm_E(G, Nl, Qm, C, r);
  const std::vector<uint32_t> cidx = rm_compact_index(dummy_w, Ncb);
  const uint32_t nn = rm_compact(Ncb, rm_null_mask{dummy_w, OAI4G_LTE_NULL}), k0c = rm_rx_k0c(dummy_w, RTC, Ncb, rvidx);
  if (nn == 0 && E > 0) { set_err("rate_matching_rx: no non-NULL entries"); return -1; }
  const size_t b_soft = (size_t)E * 2, b_w = (size_t)Ncb * 2, b_c = (size_t)Ncb * 4;
  stage_t st("rate_matching_rx");
  const int r_soft = st.add(b_soft), r_w = st.add(b_w), r_c = st.add(b_c), r_dummy = st.add(Ncb, 1024);
  if (!st.open()) return -1;
  HCK(st.up(r_soft, soft_input, b_soft), -1);
  HCK(st.up(r_w, w, b_w), -1);
  HCK(st.up(r_c, cidx.data(), b_c), -1);
  HCK(st.up(r_dummy, dummy_w, Ncb), -1);
  HCK(oai4g_launch_rm_rx(st.ptr<int16_t>(r_soft), E, st.ptr<int16_t>(r_w), st.ptr(r_dummy), st.ptr<uint32_t>(r_c), Ncb, nn,
                         k0c, clear == 1, g_scr.s), -1);
  HCK(st.down(w, r_w, b_w), -1);
  HCK(st.sync(), -1);
  *E_out = E;
  return 0;
}

extern "C" void oai4g_sub_block_deinterleaving_turbo(uint32_t D, int16_t *d, const int16_t *w)
{
  NEED_INIT();
  const uint32_t R = (D + 31) >> 5, Kpi = R << 5;
  const size_t nd = 96 + 3 * (size_t)D + 8, b_d = nd * 2, b_w = 3 * (size_t)Kpi * 2;
  stage_t st("sub_block_deinterleaving_turbo");
  const int r_d = st.add(b_d), r_w = st.add(b_w, 512);
  if (!st.open()) return;
  HCK(st.up(r_d, d - 96, b_d), );
  HCK(st.up(r_w, w, b_w), );
  HCK(oai4g_launch_subblock_deint(D, st.ptr<int16_t>(r_d), st.ptr<int16_t>(r_w), g_scr.s), );
  HCK(st.down(d - 96, r_d, b_d), );
  HCK(st.sync(), );
}

extern "C" int oai4g_idft(int log2n, const int16_t *x, int16_t *y, int scale)
{
  if (!log2n_ok(log2n)) { set_err("idft: size 2^%d not supported", log2n); return -1; }
  ofdm_sym_t s = {0, 0, 0};
  return run_ofdm((const int32_t *)x, (size_t)1 << log2n, (int32_t *)y, 0, (size_t)1 << log2n, log2n, 1, &s, scale);
}

extern "C" void oai4g_idft2048(const int16_t *x, int16_t *y, int scale) { oai4g_idft(11, x, y, scale); }
extern "C" void oai4g_idft1024(const int16_t *x, int16_t *y, int scale) { oai4g_idft(10, x, y, scale); }
extern "C" void oai4g_idft512(const int16_t *x, int16_t *y, int scale) { oai4g_idft(9, x, y, scale); }
extern "C" void oai4g_idft256(const int16_t *x, int16_t *y, int scale) { oai4g_idft(8, x, y, scale); }
extern "C" void oai4g_idft128(const int16_t *x, int16_t *y, int scale) { oai4g_idft(7, x, y, scale); }
extern "C" void oai4g_idft64(const int16_t *x, int16_t *y, int scale) { oai4g_idft(6, x, y, scale); }

/* ------------------------------------------------------------------------------------------
 * UE receive front end: forward DFT drop-ins, slot_fep, batched FEP
 * ---------------------------------------------------------------------------------------- */
static int run_fep_window(const int32_t *h_in, int32_t *h_out, int log2n, int scale)
{
  NEED_INIT(-1);
  const size_t N = (size_t)1 << log2n;
  stage_t st("dft");
  const int r_in = st.add(N * 4), r_out = st.add(N * 4, 256);
  if (!st.open()) return -1;
  fep_args_t a;
  memset(&a, 0, sizeof(a));
  a.n_units = 1;
  a.nsym = 1;
  a.in_stride = a.in_len = (uint32_t)N;
  a.out_stride = (uint32_t)N;
  a.scale = scale;
  HCK(st.up(r_in, h_in, N * 4), -1);
  HCK(oai4g_launch_fep(st.ptr<int32_t>(r_in), st.ptr<int32_t>(r_out), log2n, a, g_twf, g_n_cu, g_scr.s), -1);
  HCK(st.down(h_out, r_out, N * 4), -1);
  HCK(st.sync(), -1);
  return 0;
}

extern "C" int oai4g_dft(int log2n, const int16_t *x, int16_t *y, int scale)
{
  if (!log2n_ok(log2n)) { set_err("dft: size 2^%d not supported", log2n); return -1; }
  return run_fep_window((const int32_t *)x, (int32_t *)y, log2n, scale);
}
extern "C" void oai4g_dft2048(const int16_t *x, int16_t *y, int scale) { oai4g_dft(11, x, y, scale); }
extern "C" void oai4g_dft1024(const int16_t *x, int16_t *y, int scale) { oai4g_dft(10, x, y, scale); }
extern "C" void oai4g_dft512(const int16_t *x, int16_t *y, int scale) { oai4g_dft(9, x, y, scale); }
extern "C" void oai4g_dft256(const int16_t *x, int16_t *y, int scale) { oai4g_dft(8, x, y, scale); }
extern "C" void oai4g_dft128(const int16_t *x, int16_t *y, int scale) { oai4g_dft(7, x, y, scale); }
extern "C" void oai4g_dft64(const int16_t *x, int16_t *y, int scale) { oai4g_dft(6, x, y, scale); }

/* slot_fep's DFT window (slot_fep.c:55-150), unsigned arithmetic as in the reference: returns
 * rx_offset (before the % frame_length of the read), -1 for a bad l / Ns */
extern "C" int64_t oai4g_slot_fep_offset(const oai4g_frame_parms_t *fp, uint8_t l, uint8_t Ns, int sample_offset,
                                         int no_prefix)
{
  if (l >= 7 - fp->Ncp) {
    fprintf(stderr, "slot_fep: l must be between 0 and %d\n", 7 - fp->Ncp);
    set_err("slot_fep: l must be between 0 and %d", 7 - fp->Ncp);
    return -1;
  }
  if (Ns >= 20) {
    fprintf(stderr, "slot_fep: Ns must be between 0 and 19\n");
    set_err("slot_fep: Ns must be between 0 and 19");
    return -1;
  }
  const uint32_t N = fp->ofdm_symbol_size;
  const uint32_t cp = no_prefix ? 0u : fp->nb_prefix_samples, cp0 = no_prefix ? 0u : fp->nb_prefix_samples0;
  uint32_t subframe_offset, slot_offset;
  if (no_prefix) {
    subframe_offset = N * fp->symbols_per_tti * (Ns >> 1);
    slot_offset = N * (fp->symbols_per_tti >> 1) * (Ns % 2);
  } else {
    subframe_offset = fp->samples_per_tti * (Ns >> 1);
    slot_offset = (fp->samples_per_tti >> 1) * (Ns % 2);
  }
  uint32_t rx_offset = (uint32_t)sample_offset + slot_offset + cp0 + subframe_offset;
  rx_offset = rx_offset - rx_offset % 4;                     /* "Align with 128 bit" (:118) */
  if (l > 0) rx_offset += (N + cp) + (N + cp) * (uint32_t)(l - 1);
  return (int64_t)rx_offset;
}

/* slot_fep (PHY/MODULATION/slot_fep.c:40, decl MODULATION/defs.h): CP removal + DFT of symbol l of
 * slot Ns for every receive antenna.  rxdata[aa] holds the frame (10 samples_per_tti) plus
 * ofdm_symbol_size words of wrap extension, rxdataF[aa] the frequency-domain subframe.  The
 * channel / frequency-offset estimation that follows in the reference (perfect_ce == 0) is not
 * part of this entry point. */
extern "C" int oai4g_slot_fep(int32_t *const *rxdata, int32_t *const *rxdataF, const oai4g_frame_parms_t *fp,
                              uint8_t nb_antennas_rx, uint8_t l, uint8_t Ns, int sample_offset, int no_prefix)
{
  NEED_INIT(-1);
  const int64_t off = oai4g_slot_fep_offset(fp, l, Ns, sample_offset, no_prefix);
  if (off < 0) return -1;
  const uint32_t N = fp->ofdm_symbol_size, fl = fp->samples_per_tti * 10, rx_offset = (uint32_t)off;
  const uint32_t symbol = l + (7 - fp->Ncp) * (Ns & 1);
  std::vector<int32_t> win(N);
  for (int aa = 0; aa < nb_antennas_rx; aa++) {
    if (rx_offset > fl - N) memcpy(&rxdata[aa][fl], &rxdata[aa][0], N * sizeof(int32_t));   /* :123-126, :153-156 */
    const uint32_t st = rx_offset % fl;
    memcpy(win.data(), &rxdata[aa][st], N * sizeof(int32_t));   /* the window the reference's dft reads */
    if (run_fep_window(win.data(), &rxdataF[aa][N * symbol], fp->log2_symbol_size, 1) != 0) return -1;
  }
  return 0;
}

/* Batched FEP: every symbol of n_sf subframes x n_ant antennas, device pointers
 *   d_rx  [n_sf][n_ant][samples_per_tti] int32, d_rxF [n_sf][n_ant][symbols_per_tti][N] int32;
 * each subframe is slot_fep'd (slots 0 and 1, sample_offset 0, with prefix) on its own samples. */
extern "C" int oai4g_fep_batch(const oai4g_frame_parms_t *fp, int n_sf, int n_ant, const int32_t *d_rx, int32_t *d_rxF,
                               void *stream)
{
  NEED_INIT(-1);
  if (n_sf < 0 || n_ant <= 0 || !log2n_ok(fp->log2_symbol_size) || fp->symbols_per_tti > OAI4G_FEP_MAX_SYM) {
    set_err("fep_batch: bad arguments");
    return -1;
  }
  const uint32_t N = fp->ofdm_symbol_size, spt = fp->samples_per_tti, nslot = fp->symbols_per_tti / 2;
  fep_args_t a;
  memset(&a, 0, sizeof(a));
  a.nsym = fp->symbols_per_tti;
  a.n_units = n_sf * n_ant * a.nsym;
  a.in_stride = a.in_len = spt;
  a.out_stride = N * a.nsym;
  a.scale = 1;
  for (int sym = 0; sym < a.nsym; sym++) {
    const int64_t off = oai4g_slot_fep_offset(fp, (uint8_t)(sym % nslot), (uint8_t)(sym / nslot), 0, 0);
    if (off < 0 || (uint64_t)off + N > spt) { set_err("fep_batch: symbol %d window outside its subframe", sym); return -1; }
    a.in_off[sym] = (uint32_t)off;
    a.out_off[sym] = N * (uint32_t)sym;
  }
  HCK(oai4g_launch_fep(d_rx, d_rxF, fp->log2_symbol_size, a, g_twf, g_n_cu, (hipStream_t)stream), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * Control region: PCFICH (pcfich.c:48-228)
 * ---------------------------------------------------------------------------------------- */
/* generate_pcfich_reg_mapping (pcfich.c:48-84): the four REGs (units of 6 REs from the first
 * carrier) and the index of the lowest.  The silent helper serves generate_pcfich; the exported
 * drop-in prints them as the reference does (once, at init, in the reference's callers). */
static void pcfich_regs(const oai4g_frame_parms_t *fp, uint16_t pcfich_reg[4], uint8_t *pcfich_first_reg_idx)
{
  const uint32_t NRB = fp->N_RB_DL, kbar = 6 * (fp->Nid_cell % (2 * NRB));
  uint16_t first;
  pcfich_reg[0] = (uint16_t)(kbar / 6);
  first = pcfich_reg[0];
  *pcfich_first_reg_idx = 0;
  const uint32_t steps[3] = {(NRB >> 1) * 6, NRB * 6, ((3 * NRB) >> 1) * 6};
  for (int i = 1; i < 4; i++) {
    pcfich_reg[i] = (uint16_t)(((kbar + steps[i - 1]) % (NRB * 12)) / 6);
    if (pcfich_reg[i] < first) {
      *pcfich_first_reg_idx = (uint8_t)i;
      first = pcfich_reg[i];
    }
  }
}

extern "C" void oai4g_generate_pcfich_reg_mapping(const oai4g_frame_parms_t *fp, uint16_t pcfich_reg[4],
                                                  uint8_t *pcfich_first_reg_idx)
{
  pcfich_regs(fp, pcfich_reg, pcfich_first_reg_idx);
  printf("pcfich_reg : %d,%d,%d,%d\n", pcfich_reg[0], pcfich_reg[1], pcfich_reg[2], pcfich_reg[3]);
}

/* the PCFICH kernel's arguments: scrambling c_init (pcfich.c:96), the first RE of each REG in
 * symbol 0 (wrapped over DC), and the caller's gain / antenna choice */
static void pcfich_args_h(const oai4g_frame_parms_t *fp, uint32_t subframe, uint8_t cfi, int16_t gain, uint8_t mode1,
                          uint32_t n_ant, pcfich_args_t *a)
{
  uint16_t reg[4];
  uint8_t first_idx;
  pcfich_regs(fp, reg, &first_idx);
  memset(a, 0, sizeof(*a));
  a->c_init = ((((2u * fp->Nid_cell) + 1u) * (1u + subframe)) << 9) + fp->Nid_cell;
  a->cfi = cfi;
  a->gain = gain;
  a->mode1 = mode1;
  a->nushift3 = (uint8_t)(fp->nushift % 3);
  for (int q = 0; q < 4; q++) {
    uint32_t ro = fp->first_carrier_offset + (uint32_t)reg[q] * 6;
    if (ro >= fp->ofdm_symbol_size) ro = 1 + ro - fp->ofdm_symbol_size;
    a->reg_off[q] = ro;
  }
  a->n_ant = n_ant;
}

/* generate_pcfich (pcfich.c:144, decl proto.h:1432): overwrites the 16 PCFICH REs of symbol 0 of
 * `subframe` in the frame grids txdataF[0] (and txdataF[1] with two antennas).  The reference
 * reads frame_parms->pcfich_reg (set at init by generate_pcfich_reg_mapping); here they are
 * derived from fp.  num_pdcch_symbols outside 1..3 is rejected (-1): the reference would map an
 * uninitialised codeword (pcfich.c:164-165). */
extern "C" int oai4g_generate_pcfich(uint8_t num_pdcch_symbols, int16_t amp, const oai4g_frame_parms_t *fp,
                                     int32_t **txdataF, uint8_t subframe)
{
  NEED_INIT(-1);
  if (num_pdcch_symbols < 1 || num_pdcch_symbols > 3 || subframe > 9) {
    set_err("generate_pcfich: num_pdcch_symbols %u / subframe %u out of range", num_pdcch_symbols, subframe);
    return -1;
  }
  const uint32_t N = fp->ofdm_symbol_size, nsymb = fp->Ncp == 0 ? 14 : 12;
  const size_t symbol_offset = (size_t)N * subframe * nsymb;
  pcfich_args_t a;
  pcfich_args_h(fp, subframe, num_pdcch_symbols,
                fp->mode1_flag == 1 ? (int16_t)((amp * 23170) >> 15) : (int16_t)(amp / 2), fp->mode1_flag ? 1 : 0,
                fp->nb_antennas_tx > 1 ? 2 : 1, &a);
  stage_t st("generate_pcfich");
  const int r_g[2] = {st.add((size_t)N * 4), st.add((size_t)N * 4, 256)};
  if (!st.open()) return -1;
  for (uint32_t aa = 0; aa < a.n_ant; aa++) HCK(st.up(r_g[aa], txdataF[aa] + symbol_offset, (size_t)N * 4), -1);
  HCK(oai4g_launch_pcfich(st.ptr<int32_t>(r_g[0]), st.ptr<int32_t>(r_g[1]), a, g_scr.s), -1);
  for (uint32_t aa = 0; aa < a.n_ant; aa++) HCK(st.down(txdataF[aa] + symbol_offset, r_g[aa], (size_t)N * 4), -1);
  HCK(st.sync(), -1);
  return 0;
}

/* ----------------------------------------------------------------------------------------
 * Control region: PDCCH / DCI (generate_dci_top, dci.c:2024-2346) — host-side geometry
 * (the reference's init-time / scalar helpers) + the k_dci kernel for the per-subframe data.
 * ---------------------------------------------------------------------------------------- */
extern "C" uint8_t oai4g_get_mi(const oai4g_frame_parms_t *fp, uint8_t sf)
{
  if (fp->frame_type == 0) return 1;                                  /* phich.c:59-118 */
  switch (fp->tdd_config) {
  case 0: return (sf == 0 || sf == 5) ? 2 : 1;
  case 1: return (sf == 0 || sf == 5) ? 0 : 1;
  case 2: return (sf == 3 || sf == 8) ? 1 : 0;
  case 3: return (sf == 0 || sf == 8 || sf == 9) ? 1 : 0;
  case 4: return (sf == 8 || sf == 9) ? 1 : 0;
  case 5: return sf == 8 ? 1 : 0;
  case 6: return 1;
  default: return 0;
  }
}

static uint32_t phich_ngroup(const oai4g_frame_parms_t *fp)   /* Ngroup_PHICH (phich.c:292-303) */
{
  uint32_t ng = (fp->phich_resource * fp->N_RB_DL) / 48;
  if ((fp->phich_resource * fp->N_RB_DL) % 48) ng++;
  if (fp->Ncp == 1) ng <<= 1;
  return ng;
}

extern "C" uint16_t oai4g_get_nquad(uint8_t npdcch, const oai4g_frame_parms_t *fp, uint8_t mi)
{
  uint32_t Nreg = 0;                                                  /* dci.c:2499-2538 */
  uint8_t ng = (uint8_t)((fp->phich_resource * fp->N_RB_DL) / 48);    /* uint8_t, as :2502 */
  if ((fp->phich_resource * fp->N_RB_DL) % 48) ng++;
  if (fp->Ncp == 1) ng = (uint8_t)(ng << 1);
  ng = (uint8_t)(ng * mi);
  if (npdcch > 0 && npdcch < 4) {
    switch (fp->N_RB_DL) {
    case 6: Nreg = 12 + (npdcch - 1) * 18; break;
    case 25: Nreg = 50 + (npdcch - 1) * 75; break;
    case 50: Nreg = 100 + (npdcch - 1) * 150; break;
    case 100: Nreg = 200 + (npdcch - 1) * 300; break;
    default: return 0;
    }
  }
  return (uint16_t)(Nreg - 4 - 3 * ng);
}

extern "C" uint16_t oai4g_get_nCCE(uint8_t npdcch, const oai4g_frame_parms_t *fp, uint8_t mi)
{
  return (uint16_t)(oai4g_get_nquad(npdcch, fp, mi) / 9);
}

extern "C" uint8_t oai4g_get_num_pdcch_symbols(uint8_t num_dci, const oai4g_dci_alloc_t *dci,
                                               const oai4g_frame_parms_t *fp, uint8_t sf)
{
  uint16_t numCCE = 0;                                                /* dci.c:1964-2022 */
  uint8_t nmin = 0;
  if (fp->Ncp == 1)
    nmin = (fp->frame_type == 1 && (fp->tdd_config < 3 || fp->tdd_config == 6) && (sf == 1 || sf == 6)) ? 2 : 3;
  for (int i = 0; i < num_dci; i++) numCCE = (uint16_t)(numCCE + (1 << dci[i].L));
  const uint8_t mi = oai4g_get_mi(fp, sf);
  for (uint8_t n = 1; n <= 3; n++)
    if (numCCE <= oai4g_get_nCCE(n, fp, mi)) return nmin > n ? nmin : n;
  if (fp->N_RB_DL <= 10 && 9u * numCCE <= fp->N_RB_DL * (fp->nb_antennas_tx_eNB == 4 ? (fp->Ncp ? 9u : 10u)
                                                                                  : (fp->Ncp ? 10u : 11u)))
    return 4;
  return 0;
}

extern "C" int oai4g_generate_phich_reg_mapping(const oai4g_frame_parms_t *fp, uint16_t phich_reg[56][3])
{
  uint16_t pcf[4];                                                    /* phich.c:280-386 */
  uint8_t fi;
  pcfich_regs(fp, pcf, &fi);
  const uint32_t n0 = fp->N_RB_DL * 2u - 4u, ng = phich_ngroup(fp), nloop = fp->Ncp == 0 ? ng : ng >> 1;
  for (uint32_t m = 0; m < nloop && m < 56; m++) {
    const uint32_t base[3] = {(fp->Nid_cell + m) % n0, (fp->Nid_cell + m + n0 / 3) % n0,
                              (fp->Nid_cell + m + 2 * n0 / 3) % n0};
    for (int j = 0; j < 3; j++) {
      uint32_t r = base[j];
      for (int q = 0; q < 4; q++)
        if (r >= pcf[(fi + q) & 3]) r++;
      phich_reg[m][j] = (uint16_t)r;
    }
  }
  return (int)nloop;
}

static int g_cce_table[800];
extern "C" void oai4g_init_nCCE_table(void) { memset(g_cce_table, 0, sizeof(g_cce_table)); }

extern "C" int oai4g_get_nCCE_offset(uint8_t L, int nCCE, int common_dci, uint16_t rnti, uint8_t subframe)
{
  int *T = g_cce_table;                                               /* phy_procedures_lte_eNb.c:308-391 */
  if (L == 0 || nCCE / L <= 0) return -1;
  if (common_dci == 1) {
    int nb = L == 4 ? 4 : 2;
    if (nCCE / L < nb) nb = nCCE / L;
    for (int m = nb - 1; m >= 0; m--) {
      int fr = 1;
      for (int l = 0; l < L; l++) fr &= T[m * L + l] != 1;
      if (fr) {
        for (int l = 0; l < L; l++) T[m * L + l] = 1;
        return m * L;
      }
    }
    return -1;
  }
  uint32_t Yk = rnti;
  for (int i = 0; i <= subframe; i++) Yk = (Yk * 39827u) % 65537u;
  Yk %= (uint32_t)(nCCE / L);
  const int nb = (L == 1 || L == 2) ? 6 : 2;
  for (int m = 0; m < nb; m++) {
    const int s0 = (int)(((Yk + m) % (uint32_t)(nCCE / L)) * L);
    int fr = 1;
    for (int l = 0; l < L; l++) fr &= T[s0 + l] != 1;
    if (fr) {
      for (int l = 0; l < L; l++) T[s0 + l] = 1;
      return s0;
    }
  }
  return -1;
}

/* The static part of generate_dci_top for (fp, npdcch, subframe): the QPSK symbol interleaving
 * (pdcch_interleaving, dci.c:277-341: 32-column sub-block interleaver on quadruplets with the
 * <NULL>s dropped, then the cyclic shift by Nid_cell) composed with the REG allocation
 * (:2234-2340: k' outer, l' inner, PCFICH / PHICH REGs skipped (check_phich_reg :62-121), six-RE
 * REGs around the RS in symbol 0, four-RE REGs with the DC split elsewhere), cut at Msymb2
 * mapped REs.  map[r] = l * N + subcarrier, src[r] = QPSK symbol index.  Returns the RE count. */
static uint32_t pdcch_map(const oai4g_frame_parms_t *fp, uint8_t npdcch, uint8_t mi, std::vector<uint32_t> &map,
                          std::vector<uint16_t> &src)
{
  const uint32_t N = fp->ofdm_symbol_size, Mquad = oai4g_get_nquad(npdcch, fp, mi);
  const int Msymb = ((2 * 33 + 22) * 72) / 2;
  int Msymb2;
  switch (fp->N_RB_DL) {
  case 100: Msymb2 = Msymb; break;
  case 75: Msymb2 = 3 * Msymb / 4; break;
  case 50: Msymb2 = Msymb >> 1; break;
  case 25: Msymb2 = Msymb >> 2; break;
  case 15: Msymb2 = Msymb * 15 / 100; break;
  case 6: Msymb2 = Msymb * 6 / 100; break;
  default: Msymb2 = Msymb >> 2; break;
  }
  /* quadruplet k of wtemp <- quadruplet perm[k] of y; wbar[i] = wtemp[(i + Nid) mod Mquad] */
  std::vector<uint32_t> perm;
  const uint32_t RCC = (Mquad + 31) >> 5, ND = (RCC << 5) - Mquad;
  for (uint32_t col = 0; col < 32; col++)
    for (uint32_t row = 0, idx = bitrev_cc[col]; row < RCC; row++, idx += 32)
      if (idx >= ND) perm.push_back(idx - ND);
  uint16_t pcf[4], phr[56][3];
  uint8_t fi;
  memset(phr, 0, sizeof(phr));            /* groups the mapping never writes read as REG 0 (calloc'd frame_parms) */
  pcfich_regs(fp, pcf, &fi);
  oai4g_generate_phich_reg_mapping(fp, phr);
  const uint32_t ng = phich_ngroup(fp), ns3 = fp->nushift % 3;
  const bool tx4 = fp->nb_antennas_tx_eNB == 4;
  auto phich_or_pcfich = [&](uint32_t kp, uint32_t lp) {
    if (lp > 0 && fp->Ncp == 0) return false;
    const uint32_t m = (lp == 0 || (lp == 1 && tx4)) ? kp / 6 : kp >> 2;
    if (lp == 0 && (m == pcf[0] || m == pcf[1] || m == pcf[2] || m == pcf[3])) return true;
    if (mi > 0)
      for (uint32_t i = 0; i < ng && i < 56; i++)
        if (m == phr[i][0] || m == phr[i][1] || m == phr[i][2]) return true;
    return false;
  };
  map.clear();
  src.clear();
  uint32_t mprime = 0;
  int re_offset = fp->first_carrier_offset;
  auto put = [&](uint32_t off) {
    const uint32_t q = mprime >> 2;       /* wbar quadruplet -> y symbol */
    map.push_back(off);
    src.push_back((uint16_t)(4 * perm[(q + fp->Nid_cell) % Mquad] + (mprime & 3)));
    mprime++;
  };
  for (uint32_t kp = 0; kp < (uint32_t)fp->N_RB_DL * 12; kp++) {
    for (uint32_t lp = 0; lp < npdcch; lp++) {
      const uint32_t tti = N * lp + (uint32_t)re_offset;
      if (!phich_or_pcfich(kp, lp)) {
        const uint32_t km = kp % 12;
        if (lp == 0 || (lp == 1 && tx4)) {
          if (km == 0 || km == 6)
            for (uint32_t i = 0; i < 6; i++)
              if (i != ns3 && i != ns3 + 3) put(tti + i);
        } else if (km == 0 || km == 4 || km == 8) {
          if (re_offset != (int)N - 2) {
            for (uint32_t i = 0; i < 4; i++) put(tti + i);
          } else {                        /* the REG straddles DC */
            put(tti);
            put(tti + 1);
            put(tti - N + 3);
            put(tti - N + 4);
          }
        }
        if (mprime >= (uint32_t)Msymb2) return (uint32_t)map.size();
      }
    }
    re_offset++;
    if (re_offset == (int)N) re_offset = 1;
  }
  return (uint32_t)map.size();
}

/* Fills the kernel arguments and the map of one subframe; returns npdcch (0 on error). */
static uint8_t dci_prepare(uint8_t n_ue, uint8_t n_common, const oai4g_dci_alloc_t *dci, int16_t amp,
                           const oai4g_frame_parms_t *fp, uint32_t subframe, dci_args_t &a, std::vector<uint32_t> &map,
                           std::vector<uint16_t> &src)
{
  const uint32_t n = (uint32_t)n_ue + n_common;
  if (n > OAI4G_MAX_DCI) { set_err("generate_dci_top: %u DCIs (at most %d)", n, OAI4G_MAX_DCI); return 0; }
  if (fp->phich_duration != 0 || fp->Ncp != 0) {
    set_err("generate_dci_top: only the normal cyclic prefix with normal PHICH duration is supported");
    return 0;
  }
  const uint8_t npd = oai4g_get_num_pdcch_symbols((uint8_t)n, dci, fp, (uint8_t)subframe);
  if (npd < 1 || npd > 3) {
    set_err("generate_dci_top: num_pdcch_symbols %u (too many CCEs, or no PDCCH geometry for N_RB_DL %u)", npd,
            fp->N_RB_DL);
    return npd;
  }
  const uint8_t mi = oai4g_get_mi(fp, (uint8_t)subframe);
  memset(&a, 0, sizeof(a));
  /* generate_dci_top's order: aggregation level 3 .. 0, common DCIs first within a level; the
   * encoded blocks land at their own CCEs, so only later writers over overlapping CCEs matter */
  uint32_t k = 0;
  for (int L = 3; L >= 0; L--)
    for (uint32_t i = 0; i < n; i++)
      if (dci[i].L == L && dci[i].nCCE >= 0) {
        dci_dev_t &d = a.dci[k++];
        const uint8_t *p = dci[i].dci_pdu;
        for (int b = 0; b < 8; b++) d.flip[b] = 0;
        if (dci[i].dci_length <= 32) for (int b = 0; b < 4; b++) d.flip[b] = p[3 - b];
        else for (int b = 0; b < 8; b++) d.flip[b] = p[7 - b];
        d.A = dci[i].dci_length;
        d.L = dci[i].L;
        d.nCCE = dci[i].nCCE;
        d.rnti = dci[i].rnti;
        if (d.A > 64 || d.A < 8 || d.L > 3 || 72u * (uint32_t)(d.nCCE + (1 << d.L)) > (2 * 33 + 22 + 8) * 72u) {
          set_err("generate_dci_top: DCI %u: length %u / L %u / nCCE %d out of range", i, d.A, d.L, d.nCCE);
          return 0;
        }
      }
  a.n_dci = k;
  a.nbits = 8u * oai4g_get_nquad(npd, fp, mi);
  a.c_init = (subframe << 9) + fp->Nid_cell;
  a.gain = fp->mode1_flag == 1 ? (int16_t)((amp * 23170) >> 15) : (int16_t)(amp / 2);
  a.mode1 = fp->mode1_flag ? 1 : 0;
  a.n_ant = fp->nb_antennas_tx_eNB > 1 ? 2 : 1;
  a.n_re = pdcch_map(fp, npd, mi, map, src);
  return npd;
}

extern "C" uint8_t oai4g_generate_dci_top(uint8_t num_ue_spec_dci, uint8_t num_common_dci,
                                          const oai4g_dci_alloc_t *dci_alloc, uint32_t n_rnti, int16_t amp,
                                          const oai4g_frame_parms_t *fp, int32_t **txdataF, uint32_t subframe)
{
  (void)n_rnti;
  NEED_INIT(0);
  if (subframe > 9) { set_err("generate_dci_top: subframe %u", subframe); return 0; }
  dci_args_t a;
  std::vector<uint32_t> map;
  std::vector<uint16_t> src;
  const uint8_t npd = dci_prepare(num_ue_spec_dci, num_common_dci, dci_alloc, amp, fp, subframe, a, map, src);
  if (npd < 1 || npd > 3) return npd;
  const uint32_t N = fp->ofdm_symbol_size, nsymb = 14;
  const size_t sym_off = (size_t)N * subframe * nsymb, gbytes = (size_t)npd * N * 4;
  stage_t st("generate_dci_top");
  const int r_g[2] = {st.add(gbytes), st.add(gbytes)};
  const int r_map = st.add((size_t)a.n_re * 4), r_src = st.add((size_t)a.n_re * 2, 256);
  if (!st.open()) return 0;
  int32_t *d0 = st.ptr<int32_t>(r_g[0]), *d1 = st.ptr<int32_t>(r_g[1]);
  const uint32_t n_ant = a.n_ant;
  for (uint32_t aa = 0; aa < n_ant; aa++) HCK(st.up(r_g[aa], txdataF[aa] + sym_off, gbytes), 0);
  HCK(st.up(r_map, map.data(), (size_t)a.n_re * 4), 0);
  HCK(st.up(r_src, src.data(), (size_t)a.n_re * 2), 0);
  /* PCFICH first (generate_dci_top :2084-2088), then the PDCCH REs */
  pcfich_args_t pa;
  pcfich_args_h(fp, subframe, npd, a.gain, a.mode1, n_ant, &pa);
  HCK(oai4g_launch_pcfich(d0, d1, pa, g_scr.s), 0);
  HCK(oai4g_launch_dci(a, st.ptr<uint32_t>(r_map), st.ptr<uint16_t>(r_src), d0, d1, 0, g_scr.s), 0);
  for (uint32_t aa = 0; aa < n_ant; aa++) HCK(st.down(txdataF[aa] + sym_off, r_g[aa], gbytes), 0);
  HCK(st.sync(), 0);
  return npd;
}

/* Batched static REs: generate_dci_top's PCFICH + PDCCH (set_control) and the PSS / SSS, PBCH and
 * PHICH of the common signal procedures (set_common, phy_procedures_lte_eNb.c:1529-1760, 2585)
 * for every subframe index, computed on the GPU by the drop-in kernels into one subframe grid per
 * subframe index, gathered into the host table h_ctl, marked in the RE map with OAI4G_CTL_CODE and
 * folded into cfg_dev_t::stat_tm (upload_remap -> build_stat_tm), which the modulator merges. */
static void sync_args(const oai4g_frame_parms_t *fp, int16_t amp, bool pss, uint16_t slot_offset, sync_args_t &a);
static void pbch_args(const oai4g_frame_parms_t *fp, int amp, const uint8_t *pdu, uint8_t frame_mod4, pbch_args_t &a);
static int phich_item(const oai4g_frame_parms_t *fp, uint8_t nseq, uint8_t ngroup, uint8_t HI, uint8_t subframe,
                      phich_item_t &it);
static void phich_common(const oai4g_frame_parms_t *fp, int16_t amp, phich_args_t &a);

static int rebuild_static(oai4g_tx_config_t *cfg)
{
  const uint32_t N = cfg->h.N, nsymb = cfg->h.nsymb, n_ant = cfg->p.nb_antennas_tx;
  for (auto &c : cfg->h_remap)
    if ((c & 0xE000u) == OAI4G_CTL_CODE) c = 0xFFFF;
  memset(cfg->h.ctlmask, 0, sizeof(cfg->h.ctlmask));
  cfg->h.ctl_on = 0;
  cfg->h_ctl.clear();
  cfg->ctl_vmax = 0;
  const bool dci_on = (uint32_t)cfg->n_ue_dci + cfg->n_common_dci > 0;
  if (dci_on || cfg->common_on) {
    if (cfg->h_remap.empty()) { set_err("static REs: configuration has no RE map"); return -1; }
    const oai4g_frame_parms_t &fp = cfg->fp;
    const uint32_t n_tab = cfg->ctl_planes = n_ant > 2 ? n_ant : 2;
    std::vector<uint32_t> tab((size_t)10 * 14 * n_tab * N, 0);
    const size_t gbytes = (size_t)14 * N * 4;
    const size_t mcap = (size_t)4 * 1024;    /* >= 4 nquad REs for every geometry */
    const size_t accb = (size_t)4 * 4 * N * 4;   /* PHICH accumulators / PBCH encode grid (4 antennas x 4 symbols) */
    /* the regions serve all ten subframe indices in turn */
    stage_t st("static REs");
    const int r_g[4] = {st.add(gbytes), st.add(gbytes), st.add(gbytes), st.add(gbytes)};   /* cleared as one span */
    const int r_map = st.add(mcap * 4), r_src = st.add(mcap * 2), r_acc = st.add(accb);
    const int r_pe = st.add(1920, 128 + 256);    /* the PBCH's E <= 1920 bytes */
    if (!st.open()) return -1;
    int32_t *dg[4] = {st.ptr<int32_t>(r_g[0]), st.ptr<int32_t>(r_g[1]), st.ptr<int32_t>(r_g[2]), st.ptr<int32_t>(r_g[3])};
    uint32_t *dmap = st.ptr<uint32_t>(r_map);
    uint16_t *dsrc = st.ptr<uint16_t>(r_src);
    int32_t *dacc = st.ptr<int32_t>(r_acc);
    uint8_t *dpe = st.ptr(r_pe);
    std::vector<uint32_t> g((size_t)14 * N);
    for (uint32_t sf = 0; sf < 10; sf++) {
      HCK(st.zero(r_g[0], st.off[r_g[3]] - st.off[r_g[0]] + gbytes, r_g[3]), -1);
      uint32_t n_out = n_ant > 2 ? 2 : n_ant;          /* antennas that can carry a static RE */
      if (dci_on) {
        dci_args_t a;
        std::vector<uint32_t> map;
        std::vector<uint16_t> src;
        const uint8_t npd = dci_prepare(cfg->n_ue_dci, cfg->n_common_dci, cfg->dci.data(), cfg->p.amp, &cfg->fp, sf, a,
                                        map, src);
        if (npd < 1 || npd > 3) return -1;
        if (npd > cfg->p.num_pdcch_symbols) {
          set_err("set_control: the DCIs need %u control symbols but the PDSCH starts at symbol %u (dlsim.c:2562-2565)",
                  npd, cfg->p.num_pdcch_symbols);
          return -1;
        }
        if (map.size() > mcap) { set_err("set_control: PDCCH map too large"); return -1; }
        HCK(st.up(r_map, map.data(), map.size() * 4), -1);
        HCK(st.up(r_src, src.data(), src.size() * 2), -1);
        pcfich_args_t pa;
        pcfich_args_h(&fp, sf, npd, a.gain, a.mode1, a.n_ant, &pa);
        HCK(oai4g_launch_pcfich(dg[0], dg[1], pa, g_scr.s), -1);
        HCK(oai4g_launch_dci(a, dmap, dsrc, dg[0], dg[1], 0, g_scr.s), -1);
      }
      if (cfg->common_on) {
        const oai4g_common_sig_t &cm = cfg->common;
        const uint32_t nsl = nsymb / 2;
        if (cm.pss_sss && (sf == 0 || sf == 5)) {
          sync_args_t sa;
          int32_t *sp[4];
          sync_args(&fp, cfg->p.amp, true, (uint16_t)(2 * sf), sa);
          for (uint32_t aa = 0; aa < 4; aa++) sp[aa] = dg[aa] + (size_t)(nsl - 1) * N;
          HCK(oai4g_launch_sync(sp, sa, g_scr.s), -1);
          sync_args(&fp, cfg->p.amp, false, (uint16_t)(2 * sf), sa);
          for (uint32_t aa = 0; aa < 4; aa++) sp[aa] = dg[aa] + (size_t)(nsl - 2) * N;
          HCK(oai4g_launch_sync(sp, sa, g_scr.s), -1);
        }
        if (cm.pbch && sf == 0) {
          pbch_args_t pa;
          pbch_args(&fp, cfg->p.amp, cm.pbch_pdu, 0, pa);
          int32_t *pp[4];
          for (uint32_t aa = 0; aa < 4; aa++) pp[aa] = dg[aa] + (size_t)nsl * N;
          if (cm.frame_mod4) {                          /* encode (quarter 0) into a scratch grid, then map */
            int32_t *sp[4];
            for (uint32_t aa = 0; aa < 4; aa++) sp[aa] = dacc + (size_t)aa * 4 * N;
            HCK(oai4g_launch_pbch(sp, dpe, pa, g_scr.s), -1);
            pbch_args(&fp, cfg->p.amp, cm.pbch_pdu, cm.frame_mod4, pa);
          }
          HCK(oai4g_launch_pbch(pp, dpe, pa, g_scr.s), -1);
        }
        static thread_local phich_args_t ph;
        memset(&ph, 0, sizeof(ph));
        phich_common(&fp, cfg->p.amp, ph);
        for (uint32_t i = 0; i < cm.n_phich; i++) {
          const oai4g_phich_item_t &it = cm.phich[i];
          if (it.subframe != sf) continue;
          if (phich_item(&fp, it.nseq, it.ngroup, it.hi, (uint8_t)sf, ph.it[ph.n]) != 0) return -1;
          ph.n++;
        }
        if (ph.n) {
          if (ph.n_ant > 1 && n_ant < 2) { set_err("set_common: ALAMOUTI PHICH needs two antennas"); return -1; }
          HCK(oai4g_launch_phich(dg, dacc, ph, g_scr.s), -1);
        }
        if (cm.pbch || cm.pss_sss) n_out = n_ant;
      }
      for (uint32_t ant = 0; ant < n_out; ant++) {
        HCK(st.down(g.data(), r_g[ant], gbytes), -1);
        HCK(st.sync(), -1);
        for (uint32_t l = 0; l < nsymb; l++)
          for (uint32_t k = 0; k < N; k++) {
            const uint32_t v = g[(size_t)l * N + k];
            if (!v) continue;
            tab[(((size_t)sf * 14 + l) * n_tab + ant) * N + k] = v;
            uint16_t &code = cfg->h_remap[((size_t)sf * 14 + l) * N + k];
            if (code != 0xFFFF && code != OAI4G_CTL_CODE) {
              set_err("static REs: subframe %u symbol %u RE %u collides with a PDSCH / CRS RE", sf, l, k);
              return -1;
            }
            code = (uint16_t)OAI4G_CTL_CODE;
            cfg->h.ctlmask[sf] |= 1u << l;
          }
      }
    }
    cfg->h.ctl_on = 1;
    cfg->ctl_vmax = packed_iq_max(tab);
    cfg->h_ctl = std::move(tab);
  }
  cfg->h.mod_nosat = mod_nosat_ok(cfg->h, std::max(packed_iq_max(cfg->h_crs), cfg->ctl_vmax));
  mod_items_setup(cfg->h);
  if (upload_remap(cfg) != 0) return -1;
  HCK(hipMemcpy(cfg->d.get(), &cfg->h, sizeof(cfg_dev_t), hipMemcpyHostToDevice), -1);
  return 0;
}

extern "C" int oai4g_tx_config_set_control(oai4g_tx_config_t *cfg, uint8_t n_ue, uint8_t n_common,
                                           const oai4g_dci_alloc_t *dci)
{
  NEED_INIT(-1);
  cfg->dci.assign(dci, dci + ((uint32_t)n_ue + n_common));
  cfg->n_ue_dci = n_ue;
  cfg->n_common_dci = n_common;
  return rebuild_static(cfg);
}

extern "C" int oai4g_tx_config_set_common(oai4g_tx_config_t *cfg, const oai4g_common_sig_t *c)
{
  NEED_INIT(-1);
  if (c && c->n_phich > OAI4G_MAX_PHICH_ITEMS) { set_err("set_common: %u PHICHs", c->n_phich); return -1; }
  if (c && c->n_phich && cfg->p.mode1_flag == 1 && cfg->p.nb_antennas_tx > 1) {
    set_err("set_common: a SISO PHICH on antenna 0 only is not representable in the one-transform TM1 grid");
    return -1;
  }
  cfg->common_on = c != nullptr && (c->pss_sss || c->pbch || c->n_phich);
  if (c) cfg->common = *c;
  return rebuild_static(cfg);
}

/* ----------------------------------------------------------------------------------------
 * Synchronisation, broadcast and HARQ-indicator channels: host geometry and
 * tables of pss.c / sss.c / pbch.c / phich.c, the per-call data on the GPU (oai4g_ctrl.hip).
 * -------------------------------------------------------------------------------------- */
/* primary_synch0/1/2 (PHY/LTE_REFSIG/primary_synch.h): entries 10..133 of the reference table are
 * floor(32767 x) of the Zadoff-Chu sequence d_u(n), u = 25 / 29 / 34 (checked entry by entry
 * against the header in tests/test_sync_cpu.py) */
static void pss_table(uint32_t Nid2, int16_t v[62][2])
{
  static const int u[3] = {25, 29, 34};
  for (int n = 0; n < 62; n++) {
    const int m = n < 31 ? n : n + 1;
    const double ang = -M_PI * u[Nid2 % 3] * m * (m + 1) / 63.0;
    v[n][0] = (int16_t)floor(32767.0 * cos(ang));
    v[n][1] = (int16_t)floor(32767.0 * sin(ang));
  }
}

/* d0_sss / d5_sss (PHY/LTE_TRANSPORT/sss.h) restated from 36.211 6.11.2.1 */
static void sss_table(uint32_t Nid_cell, bool sf5, int16_t d[62])
{
  auto mseq = [](const int *taps, int nt, int8_t *out) {
    int x[31] = {0, 0, 0, 0, 1};
    for (int i = 0; i < 26; i++) {
      int v = 0;
      for (int t = 0; t < nt; t++) v += x[i + taps[t]];
      x[i + 5] = v & 1;
    }
    for (int i = 0; i < 31; i++) out[i] = (int8_t)(1 - 2 * x[i]);
  };
  static const int ts[2] = {2, 0}, tc[2] = {3, 0}, tz[4] = {4, 2, 1, 0};
  int8_t st[31], ct[31], zt[31];
  mseq(ts, 2, st);
  mseq(tc, 2, ct);
  mseq(tz, 4, zt);
  const int n1 = (int)Nid_cell / 3, n2 = (int)Nid_cell % 3;
  const int qp = n1 / 30, q = (n1 + qp * (qp + 1) / 2) / 30, mp = n1 + q * (q + 1) / 2;
  const int m0 = mp % 31, m1 = (m0 + mp / 31 + 1) % 31;
  for (int n = 0; n < 31; n++) {
    const int s0 = st[(n + m0) % 31], s1 = st[(n + m1) % 31], c0 = ct[(n + n2) % 31], c1 = ct[(n + n2 + 3) % 31];
    const int z0 = zt[(n + m0 % 8) % 31], z1 = zt[(n + m1 % 8) % 31];
    d[2 * n] = (int16_t)(sf5 ? s1 * c0 : s0 * c0);
    d[2 * n + 1] = (int16_t)(sf5 ? s0 * c1 * z1 : s1 * c1 * z0);
  }
}

static void sync_args(const oai4g_frame_parms_t *fp, int16_t amp, bool pss, uint16_t slot_offset, sync_args_t &a)
{
  memset(&a, 0, sizeof(a));
  if (pss) {
    pss_table(fp->Nid_cell % 3, a.val);
  } else {
    int16_t d[62];
    sss_table(fp->Nid_cell, slot_offset >= 3, d);
    for (int i = 0; i < 62; i++) a.val[i][0] = d[i];
  }
  a.a = fp->nb_antennas_tx == 1 ? amp : (int16_t)((amp * 23170) >> 15);
  a.pss = pss ? 1 : 0;
  a.n_ant = fp->nb_antennas_tx;
  a.N = fp->ofdm_symbol_size;
}

/* one symbol of every antenna: upload, kernel, download */
static int sync_dropin(int32_t **txdataF, int16_t amp, const oai4g_frame_parms_t *fp, uint16_t symbol,
                       uint16_t slot_offset, bool pss)
{
  NEED_INIT(-1);
  const uint32_t N = fp->ofdm_symbol_size, Nsymb = fp->Ncp == 0 ? 14 : 12, n_ant = fp->nb_antennas_tx;
  if (n_ant < 1 || n_ant > 4) { set_err("generate_%s: nb_antennas_tx %u", pss ? "pss" : "sss", n_ant); return -1; }
  const size_t off = (size_t)slot_offset * Nsymb / 2 * N + (size_t)symbol * N, sb = (size_t)N * 4;
  sync_args_t a;
  sync_args(fp, amp, pss, slot_offset, a);
  stage_t st(pss ? "generate_pss" : "generate_sss");
  const int r_g[4] = {st.add(sb), st.add(sb), st.add(sb), st.add(sb)};
  if (!st.open()) return -1;
  int32_t *d[4];
  for (uint32_t aa = 0; aa < n_ant; aa++) {
    d[aa] = st.ptr<int32_t>(r_g[aa]);
    HCK(st.up(r_g[aa], txdataF[aa] + off, sb), -1);
  }
  HCK(oai4g_launch_sync(d, a, g_scr.s), -1);
  for (uint32_t aa = 0; aa < n_ant; aa++) HCK(st.down(txdataF[aa] + off, r_g[aa], sb), -1);
  HCK(st.sync(), -1);
  return 0;
}

extern "C" int oai4g_generate_pss(int32_t **txdataF, int16_t amp, const oai4g_frame_parms_t *fp, uint16_t symbol,
                                  uint16_t slot_offset)
{
  return sync_dropin(txdataF, amp, fp, symbol, slot_offset, true);
}

extern "C" int oai4g_generate_sss(int32_t **txdataF, int16_t amp, const oai4g_frame_parms_t *fp, uint16_t symbol,
                                  uint16_t slot_offset)
{
  return sync_dropin(txdataF, amp, fp, symbol, slot_offset, false);
}

static void pbch_args(const oai4g_frame_parms_t *fp, int amp, const uint8_t *pdu, uint8_t frame_mod4, pbch_args_t &a)
{
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < 3; i++) a.a[3 - i - 1] = pdu[i];       /* pbch.c:214-215 */
  a.encode = frame_mod4 == 0 ? 1 : 0;
  a.amask = fp->mode1_flag == 1 ? 0 : (fp->nb_antennas_tx_eNB == 2 ? 0xffff : (fp->nb_antennas_tx_eNB == 4 ? 0x5555 : 0));
  a.E = fp->Ncp == 0 ? 1920 : 1728;
  a.Nid = fp->Nid_cell;
  a.quarter = frame_mod4 & 3u;
  a.N = fp->ofdm_symbol_size;
  const uint32_t nsymb = fp->Ncp == 0 ? 14 : 12, second = fp->Ncp == 0 ? 4 : 3;
  for (uint32_t i = 0; i < 4; i++) {                          /* pbch.c:345-362 */
    const uint32_t l = (nsymb >> 1) + i;
    if (l == 0 || l == (nsymb >> 1) || l == 1 || l == (nsymb >> 1) + 1 || l == second || l == second + (nsymb >> 1))
      a.pil_mask |= 1u << i;
  }
  a.nushift3 = fp->nushift % 3;
  a.gain = (int16_t)((amp * 23170) >> 15);
  a.mode1 = fp->mode1_flag == 1 ? 1 : 0;
  a.n_ant = fp->nb_antennas_tx;
}

extern "C" int oai4g_generate_pbch(oai4g_pbch_t *st, int32_t **txdataF, int amp, const oai4g_frame_parms_t *fp,
                                   const uint8_t *pbch_pdu, uint8_t frame_mod4)
{
  NEED_INIT(-1);
  const uint32_t N = fp->ofdm_symbol_size, nsymb = fp->Ncp == 0 ? 14 : 12, n_ant = fp->nb_antennas_tx;
  if (n_ant < 1 || n_ant > 4 || (fp->mode1_flag != 1 && n_ant != 2) || frame_mod4 > 3) {
    set_err("generate_pbch: %u antennas (mode1 %u), frame_mod4 %u", n_ant, fp->mode1_flag, frame_mod4);
    return -1;
  }
  pbch_args_t a;
  pbch_args(fp, amp, pbch_pdu, frame_mod4, a);
  const size_t gb = (size_t)4 * N * 4, off = (size_t)(nsymb >> 1) * N;
  stage_t sg("generate_pbch");
  const int r_g[4] = {sg.add(gb), sg.add(gb), sg.add(gb), sg.add(gb)};
  const int r_e = sg.add(1920, 128);          /* E <= 1920 bytes */
  if (!sg.open()) return -1;
  int32_t *d[4];
  for (uint32_t aa = 0; aa < n_ant; aa++) {
    d[aa] = sg.ptr<int32_t>(r_g[aa]);
    HCK(sg.up(r_g[aa], txdataF[aa] + off, gb), -1);
  }
  if (!a.encode) HCK(sg.up(r_e, st->pbch_e, a.E), -1);
  HCK(oai4g_launch_pbch(d, sg.ptr(r_e), a, g_scr.s), -1);
  if (a.encode) HCK(sg.down(st->pbch_e, r_e, a.E), -1);
  for (uint32_t aa = 0; aa < n_ant; aa++) HCK(sg.down(txdataF[aa] + off, r_g[aa], gb), -1);
  HCK(sg.sync(), -1);
  return 0;
}

static uint32_t ngroup_phich_h(const oai4g_frame_parms_t *fp)
{
  uint32_t n = ((uint32_t)fp->phich_resource * fp->N_RB_DL) / 48;
  if (((uint32_t)fp->phich_resource * fp->N_RB_DL) % 48) n++;
  return n;
}

/* phich_item_t of one generate_phich call; offsets relative to symbol 0 of the subframe */
static int phich_item(const oai4g_frame_parms_t *fp, uint8_t nseq, uint8_t ngroup, uint8_t HI, uint8_t subframe,
                      phich_item_t &it)
{
  if (fp->Ncp != 0 || fp->phich_duration != 0 || fp->nushift >= 3) {
    set_err("generate_phich: only normal CP, normal duration and nushift < 3 are defined (phich.c:540-580)");
    return -1;
  }
  uint16_t reg[56][3];
  const int ng = oai4g_generate_phich_reg_mapping(fp, reg);
  if (ngroup >= ng || nseq > 7 || subframe > 9) { set_err("generate_phich: group %u / seq %u", ngroup, nseq); return -1; }
  it.c_init = ((((uint32_t)subframe + 1u) * (fp->Nid_cell + 1u)) << 9) + fp->Nid_cell;
  const uint32_t N = fp->ofdm_symbol_size;
  for (int q = 0; q < 3; q++) {
    uint32_t ro = fp->first_carrier_offset + (uint32_t)reg[ngroup][q] * 6;
    if (ro > N) ro -= N - 1;                                   /* '>' as phich.c:560 */
    it.reg_off[q] = ro;
  }
  it.nseq = nseq;
  it.hi = HI ? 1 : 0;
  return 0;
}

static void phich_common(const oai4g_frame_parms_t *fp, int16_t amp, phich_args_t &a)
{
  a.gain = fp->mode1_flag == 1 ? (int16_t)(((int32_t)amp * 23170) >> 15) : (int16_t)(amp / 2);
  a.mode1 = fp->mode1_flag == 1 ? 1 : 0;
  a.n_ant = fp->mode1_flag == 1 ? 1 : 2;                      /* SISO writes y[0] only (phich.c:696-760) */
  a.nushift = fp->nushift;
  a.win = 2u * fp->ofdm_symbol_size;
}

extern "C" int oai4g_generate_phich(const oai4g_frame_parms_t *fp, int16_t amp, uint8_t nseq_PHICH, uint8_t ngroup_PHICH,
                                    uint8_t HI, uint8_t subframe, int32_t **y)
{
  NEED_INIT(-1);
  static thread_local phich_args_t a;
  memset(&a, 0, sizeof(a));
  if (phich_item(fp, nseq_PHICH, ngroup_PHICH, HI, subframe, a.it[0]) != 0) return -1;
  a.n = 1;
  phich_common(fp, amp, a);
  if (a.n_ant > 1 && fp->nb_antennas_tx < 2) { set_err("generate_phich: ALAMOUTI needs two grids"); return -1; }
  const uint32_t N = fp->ofdm_symbol_size;
  const size_t wb = (size_t)a.win * 4, off = (size_t)14 * N * subframe;
  stage_t st("generate_phich");
  const int r_y[2] = {st.add(wb), st.add(wb)};
  const int r_acc = st.add(4 * up256(wb));    /* the accumulators of four windows */
  if (!st.open()) return -1;
  int32_t *d[2] = {st.ptr<int32_t>(r_y[0]), st.ptr<int32_t>(r_y[1])};
  for (uint32_t aa = 0; aa < a.n_ant; aa++) HCK(st.up(r_y[aa], y[aa] + off, wb), -1);
  HCK(oai4g_launch_phich(d, st.ptr<int32_t>(r_acc), a, g_scr.s), -1);
  for (uint32_t aa = 0; aa < a.n_ant; aa++) HCK(st.down(y[aa] + off, r_y[aa], wb), -1);
  HCK(st.sync(), -1);
  return 0;
}

extern "C" int oai4g_phich_group_seq(const oai4g_frame_parms_t *fp, uint16_t first_rb, uint8_t n_DMRS, uint8_t *ngroup,
                                     uint8_t *nseq)
{
  const uint32_t Ng = ngroup_phich_h(fp), NSF = fp->Ncp == 1 ? 2 : 4;
  if (!Ng) { set_err("phich_group_seq: no PHICH groups"); return -1; }
  *ngroup = (uint8_t)((first_rb + n_DMRS) % Ng);
  *nseq = (uint8_t)((first_rb / Ng + n_DMRS) % (2 * NSF));
  return 0;
}

/* ----------------------------------------------------------------------------------------
 * UE PDSCH demodulation (second half): host geometry of rx_pdsch's
 * extraction / LLR lengths (dlsch_demodulation.c:3167-3300, dlsch_llr_computation.c:636-930,
 * adjust_G2 lte_mcs.c:157-245) and the scrambling words; the per-RE work on the GPU
 * (oai4g_rx.hip).  TM1, one receive antenna, even N_RB_DL.
 * -------------------------------------------------------------------------------------- */
struct oai4g_rx_config {
  oai4g_frame_parms_t fp;
  rx_mode_t mode;
  rx_dev_t h;
  dev_buf<rx_dev_t> d;
  dev_buf<uint32_t> d_map, d_gold;
  dev_buf<uint8_t> d_shift;       /* one entry per subframe of the largest batch so far (rx_prepare) */
  uint32_t llr_count[10];
  bool bad[10];                   /* subframe index whose LLR stream would read unwritten ext slots */
};

static int rx_alloc_bit(const uint32_t rb_alloc[4], int rb)
{
  if (rb < 32) return (rb_alloc[0] >> rb) & 1;
  if (rb < 64) return (rb_alloc[1] >> (rb - 32)) & 1;
  if (rb < 96) return (rb_alloc[2] >> (rb - 64)) & 1;
  if (rb < 100) return (rb_alloc[3] >> (rb - 96)) & 1;
  return 0;
}

/* adjust_G2 (lte_mcs.c:157-245) */
static int rx_adjust_G2(const oai4g_frame_parms_t *fp, const uint32_t rb_alloc[4], uint32_t subframe, uint32_t symbol)
{
  const uint32_t nsymb = fp->Ncp == 0 ? 14 : 12;
  int re = 0;
  if (subframe != 0 && subframe != 5 && subframe != 6) return 0;
  if (symbol < (nsymb >> 1) && fp->frame_type == 1 && subframe != 6) return 0;
  if (fp->frame_type == 1) {
    if (symbol > (nsymb >> 1) + 3 && symbol != nsymb - 1) return 0;
    if (subframe == 5 && symbol != nsymb - 1) return 0;
    if (subframe == 6 && symbol != 2) return 0;
  } else {
    if (symbol > (nsymb >> 1) + 3 || symbol < (nsymb >> 1) - 2) return 0;
    if (subframe == 5 && symbol != (nsymb >> 1) - 1 && symbol != (nsymb >> 1) - 2) return 0;
    if (subframe == 6) return 0;
  }
  const int half = fp->N_RB_DL >> 1;
  if (fp->N_RB_DL & 1) {
    for (int rb = half - 3; rb <= half + 3; rb++)
      if (rx_alloc_bit(rb_alloc, rb)) re += (rb == half - 3 || rb == half + 3) ? 6 : 12;
  } else {
    for (int rb = half - 3; rb < half + 3; rb++)
      if (rx_alloc_bit(rb_alloc, rb)) re += 12;
  }
  return re;
}

/* dlsch_extract_rbs_single (dlsch_demodulation.c:3167-3681) of one symbol as an extraction map:
 * the ext slots the call leaves written, each FFT bin | (estimate column 5 + 12 rb + i) << 16, with
 * the reference's pointer steps (the odd-N_RB RB around DC can write one slot past the step it then
 * takes; the next RB overwrites it).  n = slots written; nb_rb as the reference counts it. */
static void rx_extract_map(const oai4g_frame_parms_t *fp, const uint32_t rb_alloc[4], uint32_t subframe, uint32_t l,
                           std::vector<uint32_t> &map, uint32_t &nb_rb, uint32_t &n)
{
  const uint32_t smod = l >= 7u - fp->Ncp ? l - (7u - fp->Ncp) : l;
  const bool pil = smod == 0 || smod == 4u - fp->Ncp;
  const uint32_t poff = smod == 4u - fp->Ncp ? 3 : 0, ns = fp->nushift;
  const int nsymb = fp->Ncp == 0 ? 14 : 12, half = fp->N_RB_DL >> 1;
  uint32_t slot[12 * 110 + 12];
  uint32_t ptr = 0, hw = 0;
  nb_rb = 0;
  auto put = [&](uint32_t pos, uint32_t bin, uint32_t col) {
    slot[pos] = bin | (col << 16);
    hw = pos + 1 > hw ? pos + 1 : hw;
  };
  if ((fp->N_RB_DL & 1) == 0) {
    uint32_t bin = fp->first_carrier_offset;
    for (int rb = 0; rb < fp->N_RB_DL; rb++) {
      if (rb == half) bin = 1;
      if (rx_alloc_bit(rb_alloc, rb)) {
        for (uint32_t i = 0; i < 12; i++)
          if (!pil || (i != ns + poff && i != (ns + poff + 6) % 12)) put(ptr++, bin + i, 5 + 12 * rb + i);
        nb_rb++;
      }
      bin += 12;
    }
  } else {
    const int sss_symb = fp->frame_type == 1 ? nsymb - 1 : (nsymb >> 1) - 2;
    const int pss_symb = fp->frame_type == 1 ? 2 : (nsymb >> 1) - 1;
    const int li = (int)l;
    const bool pbch = subframe == 0 && li >= (nsymb >> 1) && li < (nsymb >> 1) + 4;
    const bool sss = (subframe == 0 || subframe == 5) && li == sss_symb;
    const bool pss = (fp->frame_type == 0 && (subframe == 0 || subframe == 5) && li == pss_symb) ||
                     (fp->frame_type == 1 && subframe == 6 && li == pss_symb);
    const bool excl = pbch || sss || pss;
    uint32_t bin = fp->first_carrier_offset;
    for (int rb = 0; rb < fp->N_RB_DL; rb++) {
      int ind = rx_alloc_bit(rb_alloc, rb);
      const uint32_t col = 5 + 12 * rb;
      if (rb == half) {                                       /* :3434-3525, split at bin 0 */
        if (excl) ind = 0;
        if (ind) {
          uint32_t j = 0;
          for (uint32_t i = 0; i < 12; i++) {
            const uint32_t b = i < 6 ? bin + i : 1 + i - 6;
            if (!pil) put(ptr + i, b, col + i);
            else if (i < 6 ? i != (ns + poff) % 6 : i != (ns + 6 + poff) % 12) put(ptr + j++, b, col + i);
          }
          ptr += pil ? 10 : 12;
          nb_rb++;
        }
        bin = 7;
        continue;
      }
      int skip_half = 0;
      if (excl && rb > half - 3 && rb < half + 3) ind = 0;
      if (excl) skip_half = rb == half - 3 ? 1 : (rb == half + 3 ? 2 : 0);
      if (ind) {
        uint32_t j = 0;
        if (skip_half) {
          const uint32_t o = skip_half == 2 ? 6 : 0;
          for (uint32_t i = 0; i < 6; i++)
            if (!pil || i != (ns + poff) % 6) put(ptr + j++, bin + i + o, col + i + o);
          ptr += pil ? 5 : 6;
        } else {
          for (uint32_t i = 0; i < 12; i++)
            if (!pil || (i != ns + poff && i != (ns + poff + 6) % 12)) put(ptr + j++, bin + i, col + i);
          ptr += pil ? 10 : 12;
        }
        nb_rb++;
      }
      bin += 12;
    }
  }
  n = hw;
  map.insert(map.end(), slot, slot + hw);
}

/* dlsch_extract_rbs_dual (dlsch_demodulation.c:3683-4056) of one symbol as an extraction map of
 * the slots one receive antenna's call leaves written (every antenna and both ports share it): the
 * PBCH / PSS / SSS RBs are dropped; 8 REs per RB in pilot symbols; odd N_RB_DL as written there —
 * the RB around DC reads bins 0..5 for its upper half in non-pilot symbols, the skip_half = 2
 * pilot branch advances the pointers inside its RE loop, and the full-RB non-pilot branch
 * (:3932-3936) is `for (i=0;i<12;i++) dl_ch0_ext+=12;` (its loop body was a printf, now commented
 * out), so the port-0 estimate pointer moves 144 slots per RB while rxF_ext / dl_ch1_ext move 12.
 * The port-0 writes are tracked with that drift; n = the prefix of slots where the received RE and
 * both estimates come from the same column (past it the reference reads stale or unwritten port-0
 * slots, and its writes run past dl_ch_estimates_ext: a stream reaching there is refused).
 * prbs, when given, receives the PRBs in the order the extraction fills pmi_ext for them. */
static void rx_extract_map_dual(const oai4g_frame_parms_t *fp, const uint32_t rb_alloc[4], uint32_t subframe, uint32_t l,
                                std::vector<uint32_t> &map, uint32_t &nb_rb, uint32_t &n,
                                std::vector<uint16_t> *prbs = nullptr)
{
  const uint32_t smod = l >= 7u - fp->Ncp ? l - (7u - fp->Ncp) : l;
  const bool pil = smod == 0 || smod == 4u - fp->Ncp;
  const int nsymb = fp->Ncp == 0 ? 14 : 12, half = fp->N_RB_DL >> 1, li = (int)l;
  const uint32_t ns = fp->nushift;
  const int sss_symb = fp->frame_type == 1 ? nsymb - 1 : (nsymb >> 1) - 2;
  const int pss_symb = fp->frame_type == 1 ? 2 : (nsymb >> 1) - 1;
  std::vector<uint32_t> slot(12 * 110 + 256, 0);
  std::vector<uint8_t> wr(12 * 110 + 256, 0);
  std::vector<int32_t> col_rx(12 * 110 + 256, -1), col_c0(12 * 110 + 256, -1);
  uint32_t p = 0, hw = 0, drift = 0;                         /* drift = dl_ch0_ext - rxF_ext (slots) */
  nb_rb = 0;
  auto put = [&](uint32_t pos, uint32_t bin, uint32_t col) {
    slot[pos] = bin | ((5 + col) << 16);
    wr[pos] = 1;
    col_rx[pos] = (int32_t)col;
    if (pos + drift < col_c0.size()) col_c0[pos + drift] = (int32_t)col;
    hw = pos + 1 > hw ? pos + 1 : hw;
  };
  auto data_re = [&](uint32_t i) { return i != ns && i != ns + 3 && i != ns + 6 && i != (ns + 9) % 12; };
  for (int prb = 0; prb < fp->N_RB_DL; prb++) {
    int ind = rx_alloc_bit(rb_alloc, prb), skip_half = 0;
    if (subframe == 0 && prb > half - 3 && prb < half + 3 && li >= (nsymb >> 1) && li < (nsymb >> 1) + 4) ind = 0;
    if ((subframe == 0 || subframe == 5) && prb > half - 3 && prb < half + 3 && li == sss_symb) ind = 0;
    if (fp->frame_type == 0 && (subframe == 0 || subframe == 5) && prb > half - 3 && prb < half + 3 && li == pss_symb) ind = 0;
    if (fp->frame_type == 1 && subframe == 6 && prb >= half - 3 && prb <= half + 3 && li == pss_symb) ind = 0;
    if (!ind) continue;
    if (prbs) prbs->push_back((uint16_t)prb);                  /* the PRBs pmi_ext gets an entry for, in order */
    const uint32_t col0 = 12 * prb;
    if ((fp->N_RB_DL & 1) == 0) {
      const uint32_t b0 = prb < half ? fp->first_carrier_offset + 12 * prb : 1 + 12 * (prb - half);
      uint32_t j = 0;
      for (uint32_t i = 0; i < 12; i++)
        if (!pil || data_re(i)) put(p + j++, b0 + i, col0 + i);
      p += pil ? 8 : 12;
      nb_rb++;
      continue;
    }
    if (subframe == 0 && prb == half - 3 && li >= (nsymb >> 1) && li < (nsymb >> 1) + 4) skip_half = 1;
    else if (subframe == 0 && prb == half + 3 && li >= (nsymb >> 1) && li < (nsymb >> 1) + 4) skip_half = 2;
    if ((subframe == 0 || subframe == 5) && prb == half - 3 && li == sss_symb) skip_half = 1;
    else if ((subframe == 0 || subframe == 5) && prb == half + 3 && li == sss_symb) skip_half = 2;
    if ((fp->frame_type == 0 && (subframe == 0 || subframe == 5)) || (fp->frame_type == 1 && (subframe == 2 || subframe == 6))) {
      if (prb == half - 3 && li == pss_symb) skip_half = 1;
      else if ((subframe == 0 || subframe == 5) && prb == half + 3 && li == pss_symb) skip_half = 2;
    }
    const uint32_t b0 = prb <= half ? fp->first_carrier_offset + 12 * prb : 7 + 12 * (prb - half - 1);
    if (prb != half) {
      if (!pil) {
        const uint32_t o = skip_half == 2 ? 6 : 0, cnt = skip_half ? 6 : 12;
        for (uint32_t i = 0; i < cnt; i++) put(p + i, b0 + o + i, col0 + o + i);
        p += cnt;
        if (!skip_half) drift += 132;                        /* dl_ch0_ext += 144 (:3932-3934) */
      } else if (skip_half == 1) {
        uint32_t j = 0;
        for (uint32_t i = 0; i < 6; i++)
          if (i != ns && i != (ns + 3) % 6) put(p + j++, b0 + i, col0 + i);
        p += 4;
      } else if (skip_half == 2) {
        uint32_t j = 0;
        for (uint32_t i = 0; i < 6; i++) {
          if (i != ns && i != (ns + 3) % 6) put(p + j++, b0 + i + 6, col0 + i + 6);
          p += 4;                                            /* inside the loop, as written */
        }
      } else {
        uint32_t j = 0;
        for (uint32_t i = 0; i < 12; i++)
          if (data_re(i)) put(p + j++, b0 + i, col0 + i);
        p += 8;
      }
    } else {                                                 /* the RB around DC */
      if (!pil) {
        for (uint32_t i = 0; i < 6; i++) put(p + i, b0 + i, col0 + i);
        for (uint32_t i = 0; i < 6; i++) put(p + 6 + i, i, col0 + 6 + i);
        p += 12;
      } else {
        uint32_t j = 0, i = 0;
        for (; i < 6; i++)
          if (i != ns && i != (ns + 3) % 6) put(p + j++, b0 + i, col0 + i);
        for (; i < 12; i++)
          if (i != (ns + 6) % 12 && i != (ns + 9) % 12) put(p + j++, 1 + i - 6, col0 + i);
        p += 8;
      }
    }
    nb_rb++;
  }
  /* n = the written prefix: the skip_half = 2 pilot branch leaves holes, which the reference would
   * fill from earlier symbols' ext data (a stream reaching one is refused) */
  n = 0;
  while (n < hw && wr[n] && col_c0[n] == col_rx[n]) n++;
  map.insert(map.end(), slot.begin(), slot.begin() + hw);
}

/* offset_mumimo_llr_drange (dlsch_demodulation.c:76, the active table) [MCS][Qm1 / 2 - 1] */
static const uint8_t k_mumimo_off[29][3] = {{0, 6, 5}, {0, 4, 5}, {0, 4, 5}, {0, 5, 4}, {0, 5, 6}, {0, 5, 3}, {0, 4, 4},
                                            {0, 4, 4}, {0, 3, 3}, {0, 1, 2}, {1, 1, 0}, {1, 3, 2}, {3, 4, 1}, {2, 0, 0},
                                            {2, 2, 2}, {1, 1, 1}, {2, 1, 0}, {2, 1, 1}, {1, 0, 1}, {1, 0, 1}, {0, 0, 0},
                                            {1, 0, 0}, {0, 0, 0}, {0, 1, 0}, {1, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0},
                                            {0, 0, 0}};

/* what a mode takes beyond the common arguments (no padding: the drop-ins' cache compares it bytewise).
 * TM3: codeword 1's modulation and codeword 0's MCS; TM4-6: the precoder word, the subband rule and
 * dl_power_off of oai4g_rx_config_create_tm56 */
struct rx_parms_t {
  int pmi_rule;
  uint16_t pmi_alloc;
  uint8_t nb_rx, Qm1, mcs0, mimo_mode, dl_power_off, pad;
};

/* pmi_ext of one allocated PRB.  OAI4G_RX_PMI_UE: dlsch_extract_rbs_dual's (pmi >> ((prb >> 2) << 1)) & 3
 * (:3812, :3907) — 4-RB subbands at every bandwidth; pmi is an unsigned short promoted to int, so a count
 * of 16..31 reads 0 (counts >= 32 are refused by the caller).  OAI4G_RX_PMI_TX: the transmitter's get_pmi. */
static uint32_t rx_pmi_of(const oai4g_frame_parms_t *fp, const rx_parms_t &t, uint32_t prb)
{
  if (t.pmi_rule == OAI4G_RX_PMI_TX) return oai4g_get_pmi(fp->N_RB_DL, t.mimo_mode, t.pmi_alloc, (uint16_t)prb);
  const uint32_t cnt = (prb >> 2) << 1;
  return cnt >= 32 ? 0u : ((uint32_t)t.pmi_alloc >> cnt) & 3u;
}

static oai4g_rx_config_t *rx_config_build(const oai4g_frame_parms_t *fp, const uint32_t rb_alloc[4], uint8_t Qm,
                                          uint8_t num_pdcch_symbols, uint16_t rnti, uint8_t first_subframe,
                                          uint8_t subframe_step, rx_mode_t mode, const rx_parms_t &mp)
{
  NEED_INIT(nullptr);
  const bool tm2 = mode == RX_TM2, tm3 = mode == RX_TM3, tm56 = mode == RX_TM56, dual = mode != RX_SISO;
  const uint8_t nb_rx = mp.nb_rx, Qm1 = mp.Qm1, mcs0 = mp.mcs0;
  if (tm56) {
    if (fp->nb_antennas_tx != 2 || fp->mode1_flag != 0 || (Qm != 2 && Qm != 4 && Qm != 6) || nb_rx < 1 || nb_rx > 2 ||
        num_pdcch_symbols < 1 || num_pdcch_symbols > 3 ||
        (mp.pmi_rule != OAI4G_RX_PMI_UE && mp.pmi_rule != OAI4G_RX_PMI_TX)) {
      set_err("rx_config_tm56: two TX ports (mode1_flag 0), Qm 2/4/6, 1-2 RX antennas, 1..3 PDCCH symbols, "
              "pmi_rule OAI4G_RX_PMI_UE / _TX");
      return nullptr;
    }
    if (mp.mimo_mode < OAI4G_UNIFORM_PRECODING11 || mp.mimo_mode > OAI4G_PUSCH_PRECODING0) {
      set_err("rx_config_tm56: mimo_mode %u: rx_pdsch demodulates the single-layer modes 3..7 (mode 8 ends in "
              "\"Unknown MIMO mode\", dlsch_demodulation.c:595-597)", mp.mimo_mode);
      return nullptr;
    }
    if (mp.pmi_rule == OAI4G_RX_PMI_UE && mp.pmi_alloc != 0)
      for (int prb = 64; prb < fp->N_RB_DL; prb++)
        if (rx_alloc_bit(rb_alloc, prb)) {
          set_err("rx_config_tm56: PRB %d is allocated: the reference UE shifts its 16-bit pmi_alloc by %d there "
                  "(dlsch_demodulation.c:3812), which is undefined; only pmi_alloc 0 reads the same either way",
                  prb, (prb >> 2) << 1);
          return nullptr;
        }
  }
  if (tm2 && (fp->nb_antennas_tx != 2 || fp->mode1_flag != 0 || (Qm != 2 && Qm != 4 && Qm != 6) || nb_rx < 1 ||
              nb_rx > 2 || num_pdcch_symbols < 1 || num_pdcch_symbols > 3)) {
    set_err("rx_config_tm2: two TX ports (mode1_flag 0), Qm 2/4/6, 1-2 RX antennas, 1..3 PDCCH symbols");
    return nullptr;
  }
  if (!dual && (fp->nb_antennas_tx != 1 || fp->mode1_flag != 1 || (Qm != 2 && Qm != 4 && Qm != 6) ||
               num_pdcch_symbols < 1 || num_pdcch_symbols > 3)) {
    set_err("rx_config: TM1 (one TX port), Qm 2/4/6, 1..3 PDCCH symbols only");
    return nullptr;
  }
  if (tm3 && (fp->nb_antennas_tx != 2 || fp->mode1_flag != 0 || (Qm != 2 && Qm != 4 && Qm != 6) ||
              (Qm1 != 2 && Qm1 != 4 && Qm1 != 6) || mcs0 > 28 || nb_rx < 1 || nb_rx > 2 || num_pdcch_symbols < 1 ||
              num_pdcch_symbols > 3)) {
    set_err("rx_config_tm3: two TX ports, Qm0 and Qm1 2/4/6, 1-2 RX antennas, 1..3 PDCCH symbols");
    return nullptr;
  }
  const uint32_t nsymb = fp->Ncp == 0 ? 14 : 12, N = fp->ofdm_symbol_size;
  const uint32_t first_mod = num_pdcch_symbols >= 7u - fp->Ncp ? num_pdcch_symbols - (7u - fp->Ncp) : num_pdcch_symbols;
  if (first_mod == 0 || first_mod == 4u - fp->Ncp) {
    set_err("rx_config: the first PDSCH symbol carries pilots (dlsch_channel_level would read past the extracted REs)");
    return nullptr;
  }
  std::unique_ptr<oai4g_rx_config> cfg(new oai4g_rx_config());
  cfg->fp = *fp;
  cfg->mode = mode;
  rx_dev_t &h = cfg->h;
  memset(&h, 0, sizeof(h));
  h.N = N;
  h.nsymb = nsymb;
  h.Qm = Qm;
  h.npdcch = num_pdcch_symbols;
  h.n_sym = nsymb - num_pdcch_symbols;
  h.first_sf = first_subframe % 10;
  h.sf_step = subframe_step;
  h.a1 = Qm == 4 ? 20724 : (Qm == 6 ? 20225 : 0);          /* QAM16_n1 / QAM64_n1 (impl_defs_top.h:215-224) */
  h.a2 = Qm == 6 ? 10112 : 0;                               /* QAM64_n2 */
  h.nb_rx = dual ? nb_rx : 1u;
  h.mu_off = tm3 ? k_mumimo_off[mcs0][(Qm1 >> 1) - 1] : 0;
  h.qm1 = tm3 ? Qm1 : 0u;
  h.lvl_inc = tm56 && mp.dl_power_off == 1 ? 1u : 0u;
  /* estimate rows from the 5 pilot rows (P0 .. P3 = symbols 0, p1, p2, p3; P4 = the next subframe's
   * symbol 0): lte_dl_channel_estimation.c:639-698 as k_chest's ce_interp applies it; row l is P[a] alone
   * (wa 0) or P[a] wa + P[a + 1] wb */
  {
    const uint32_t p1 = fp->Ncp ? 3 : 4, p2 = fp->Ncp ? 6 : 7, p3 = fp->Ncp ? 9 : 11;
    auto row = [&](uint32_t l, uint8_t a, int16_t wa, int16_t wb) { h.ea[l] = a; h.ewa[l] = wa; h.ewb[l] = wb; };
    row(0, 0, 0, 0); row(p1, 1, 0, 0); row(p2, 2, 0, 0); row(p3, 3, 0, 0);
    row(p3 + 1, 3, 21845, 10923); row(p3 + 2, 3, 10923, 21845);
    row(p1 + 1, 1, 21845, 10923); row(p1 + 2, 1, 10923, 21845);
    if (fp->Ncp == 0) {
      row(1, 0, 24576, 8192); row(2, 0, 16384, 16384); row(3, 0, 8192, 24576);
      row(p2 + 1, 2, 24576, 8192); row(p2 + 2, 2, 16384, 16384); row(p2 + 3, 2, 8192, 24576);
    } else {                                                 /* the reference's 1/3, 2/3 order, as written */
      row(1, 0, 10923, 21845); row(2, 0, 21845, 10923);
      row(p2 + 1, 2, 10923, 21845); row(p2 + 2, 2, 21845, 10923);
    }
  }
  std::vector<uint32_t> map;
  uint32_t max_llr = 0;
  for (uint32_t sf = 0; sf < 10; sf++) {
    uint32_t off = 0;
    for (uint32_t k = 0; k < h.n_sym; k++) {
      const uint32_t l = num_pdcch_symbols + k;
      const uint32_t smod = l >= 7u - fp->Ncp ? l - (7u - fp->Ncp) : l;
      const bool pil = smod == 0 || smod == 4u - fp->Ncp;
      h.map_off[sf][k] = (uint32_t)map.size();
      uint32_t nb_rb = 0, n = 0;
      if (tm56) {
        /* this configuration's own copy of the dual map: slot j belongs to pmi_ext[j / 12] (j / 8 in
         * pilot symbols, dlsch_channel_compensation_TM56 :1518-1528, :1641-1654), whose precoder goes
         * into bits 30-31 (bin and 5 + column stay below 2^11) */
        std::vector<uint16_t> prbs;
        rx_extract_map_dual(fp, rb_alloc, sf, l, map, nb_rb, n, &prbs);
        const uint32_t nre = pil ? 8 : 12;
        for (size_t j = h.map_off[sf][k]; j < map.size(); j++) {
          const size_t rb = (j - h.map_off[sf][k]) / nre;
          if (rb < prbs.size()) map[j] |= rx_pmi_of(fp, mp, prbs[rb]) << 30;
        }
      } else if (dual)
        rx_extract_map_dual(fp, rb_alloc, sf, l, map, nb_rb, n);
      else
        rx_extract_map(fp, rb_alloc, sf, l, map, nb_rb, n);
      const int adj = Qm == 2 ? 0 : rx_adjust_G2(fp, rb_alloc, sf, l);
      /* dlsch_*_llr: pilot symbols carry 10 (one port) or 8 (two ports, mode1_flag 0) REs per RB */
      const int len = pil ? (dual ? (int)nb_rb * 8 - 2 * adj / 3 : (int)nb_rb * 10 - 5 * adj / 6) : (int)nb_rb * 12 - adj;
      h.len[sf][k] = (uint32_t)(len > 0 ? len : 0);
      /* channel_level_TM3 takes 8 REs per RB only where symbol_mod == 0 (its 4-Ncp test reads
       * Ncp-1, :2917-2922); the SISO level reads 12 per RB */
      const uint32_t lvl_nre = dual && smod == 0 ? 8u : 12u;
      /* TM2 combines RE pairs: the partner of an odd last RE must have been extracted too */
      const uint32_t need = tm2 ? (h.len[sf][k] + 1) & ~1u : h.len[sf][k];
      if (need > n || (k == 0 && lvl_nre * nb_rb > n)) {
        /* the reference would read ext slots this symbol did not write (odd N_RB_DL with a
         * PBCH / sync half RB and the unadjusted QPSK length, :3354-3427): a batch that runs
         * this subframe index is refused */
        cfg->bad[sf] = true;
        h.len[sf][k] = h.len[sf][k] < n ? h.len[sf][k] : n;
      }
      if (h.len[sf][k] > 1280) { set_err("rx_config: > 1280 REs in a symbol (k_rx_llr covers 256 x 5)"); return nullptr; }
      h.llr_off[sf][k] = off;
      off += h.len[sf][k] * Qm;
      if (k == 0) {
        h.lvl_n[sf] = lvl_nre * nb_rb;
        h.lvl_div[sf] = dual ? lvl_nre * nb_rb : (pil ? 10 : 12) * nb_rb;
      }
      if (nb_rb == 0) cfg->bad[sf] = true;                   /* empty allocation in this symbol */
    }
    cfg->llr_count[sf] = off;
    max_llr = off > max_llr ? off : max_llr;
  }
  h.llr_stride = (max_llr + 63) & ~63u;
  /* scrambling words per subframe index: c_init = rnti 2^14 + q 2^13 + (Ns/2) 2^9 + Nid, q = 0,
   * Ns = 2 subframe (dlsch_scrambling.c:116), word w = lte_gold_generic output 50 + w */
  h.gold_words = (max_llr + 31) / 32 + 1;
  std::vector<uint32_t> gold((size_t)10 * h.gold_words);
  for (uint32_t sf = 0; sf < 10; sf++)
    gold_seq_h(((uint32_t)rnti << 14) + (sf << 9) + fp->Nid_cell, gold.data() + (size_t)sf * h.gold_words, h.gold_words);
  if (cfg->d_map.upload(map) != hipSuccess || cfg->d_gold.upload(gold) != hipSuccess) {
    set_err("rx_config: table upload failed");
    return nullptr;
  }
  h.map = cfg->d_map.get();
  h.gold = cfg->d_gold.get();
  if (cfg->d.upload(&h, 1) != hipSuccess) {
    set_err("rx_config: upload failed");
    return nullptr;
  }
  return cfg.release();
}

extern "C" oai4g_rx_config_t *oai4g_rx_config_create(const oai4g_frame_parms_t *fp, const uint32_t rb_alloc[4], uint8_t Qm,
                                                     uint8_t num_pdcch_symbols, uint16_t rnti, uint8_t first_subframe,
                                                     uint8_t subframe_step)
{
  rx_parms_t mp = {};
  mp.nb_rx = 1;
  return rx_config_build(fp, rb_alloc, Qm, num_pdcch_symbols, rnti, first_subframe, subframe_step, RX_SISO, mp);
}

extern "C" oai4g_rx_config_t *oai4g_rx_config_create_tm3(const oai4g_frame_parms_t *fp, const uint32_t rb_alloc[4],
                                                         uint8_t Qm0, uint8_t Qm1, uint8_t mcs0,
                                                         uint8_t num_pdcch_symbols, uint16_t rnti,
                                                         uint8_t first_subframe, uint8_t subframe_step, uint8_t nb_rx)
{
  rx_parms_t mp = {};
  mp.nb_rx = nb_rx; mp.Qm1 = Qm1; mp.mcs0 = mcs0;
  return rx_config_build(fp, rb_alloc, Qm0, num_pdcch_symbols, rnti, first_subframe, subframe_step, RX_TM3, mp);
}

extern "C" oai4g_rx_config_t *oai4g_rx_config_create_tm2(const oai4g_frame_parms_t *fp, const uint32_t rb_alloc[4],
                                                         uint8_t Qm, uint8_t num_pdcch_symbols, uint16_t rnti,
                                                         uint8_t first_subframe, uint8_t subframe_step, uint8_t nb_rx)
{
  rx_parms_t mp = {};
  mp.nb_rx = nb_rx;
  return rx_config_build(fp, rb_alloc, Qm, num_pdcch_symbols, rnti, first_subframe, subframe_step, RX_TM2, mp);
}

extern "C" oai4g_rx_config_t *oai4g_rx_config_create_tm56(const oai4g_frame_parms_t *fp, const uint32_t rb_alloc[4],
                                                          uint8_t Qm, uint8_t mimo_mode, uint16_t pmi_alloc,
                                                          int pmi_rule, uint8_t dl_power_off,
                                                          uint8_t num_pdcch_symbols, uint16_t rnti,
                                                          uint8_t first_subframe, uint8_t subframe_step, uint8_t nb_rx)
{
  rx_parms_t mp = {};
  mp.nb_rx = nb_rx; mp.mimo_mode = mimo_mode; mp.pmi_alloc = pmi_alloc; mp.pmi_rule = pmi_rule; mp.dl_power_off = dl_power_off;
  return rx_config_build(fp, rb_alloc, Qm, num_pdcch_symbols, rnti, first_subframe, subframe_step, RX_TM56, mp);
}

extern "C" void oai4g_rx_config_destroy(oai4g_rx_config_t *cfg)
{
  if (cfg) delete cfg;
}

extern "C" int oai4g_rx_llr_count(const oai4g_rx_config_t *cfg, int subframe_index)
{
  return (subframe_index < 0 || subframe_index > 9) ? -1 : (int)cfg->llr_count[subframe_index];
}

extern "C" size_t oai4g_rx_llr_stride(const oai4g_rx_config_t *cfg) { return cfg->h.llr_stride; }

/* a batch of n_sf elements must not run a subframe index whose stream the reference would build
 * from ext slots it did not write (rx_config's bad[]) */
static int rx_check_batch(const oai4g_rx_config_t *cfg, int n_sf)
{
  for (int i = 0; i < n_sf && i < 10; i++) {
    const uint32_t sfi = (cfg->h.first_sf + (uint32_t)i * cfg->h.sf_step) % 10;
    if (cfg->bad[sfi]) {
      set_err("rx_batch: subframe index %u reads extracted REs the reference does not write (odd N_RB_DL with "
              "PBCH / sync half RBs, or an empty symbol)", sfi);
      return -1;
    }
  }
  return 0;
}

/* The opening of every batch entry point: the library is up, cfg is a configuration of `mode` (else
 * `refusal` is the error; `not_2cw`, when given, likewise unless both codewords are QPSK), the batch runs
 * no bad subframe index, d_shift holds n_sf entries.  -1 refused, 0 nothing to do, 1 launch. */
static int rx_prepare(oai4g_rx_config_t *cfg, int n_sf, rx_mode_t mode, const char *refusal, const char *not_2cw = nullptr)
{
  NEED_INIT(-1);
  if (!cfg || cfg->mode != mode) { set_err("%s", refusal); return -1; }
  if (not_2cw && (cfg->h.Qm != 2 || cfg->h.qm1 != 2)) { set_err("%s", not_2cw); return -1; }
  if (n_sf <= 0) return 0;
  if (rx_check_batch(cfg, n_sf) != 0) return -1;
  HCK(cfg->d_shift.reserve((size_t)n_sf), -1);
  return 1;
}

/* words per (port, antenna) plane of d_est: [n_sf][nsymb][N] estimates, or (pil) the 4 pilot-row pairs
 * per subframe that oai4g_chest_batch_pilots wrote */
static size_t rx_plane(const oai4g_rx_config_t *cfg, int n_sf, int pil)
{
  return pil ? (size_t)n_sf * 4 * cfg->h.N * 2 : (size_t)n_sf * cfg->h.nsymb * cfg->h.N;
}

/* d_est: TM1's estimate grid, else the planes [p * 2 + a][n_sf][nsymb][N], or (pil; TM3 and TM4-6) the
 * pilot rows [p * 2 + a][n_sf][5][N]: the demodulator forms every other row with the estimator's temporal
 * interpolation, so the 14-row planes never reach HBM and the LLRs are bit-identical */
static int rx_batch(oai4g_rx_config_t *cfg, int n_sf, rx_mode_t mode, const char *refusal, const char *not_2cw,
                    const int32_t *d_rxdataF, const int32_t *d_est, int pil, int16_t *d_llr0, int16_t *d_llr1,
                    int unscramble, void *stream)
{
  const int go = rx_prepare(cfg, n_sf, mode, refusal, not_2cw);
  if (go <= 0) return go;
  HCK(oai4g_launch_rx(mode, cfg->d.get(), &cfg->h, n_sf, d_rxdataF, d_est, rx_plane(cfg, n_sf, pil), d_llr0, d_llr1,
                      cfg->d_shift.get(), unscramble, (hipStream_t)stream, pil), -1);
  return 0;
}

extern "C" int oai4g_rx_batch(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_ch,
                              int16_t *d_llr, int unscramble, void *stream)
{
  return rx_batch(cfg, n_sf, RX_SISO, "rx_batch: not a TM1 configuration (oai4g_rx_config_create)", nullptr, d_rxdataF, d_ch,
                  0, d_llr, nullptr, unscramble, stream);
}

/* codeword 0 QPSK takes the interference-aware qpsk_qpsk / qpsk_16qam / qpsk_64qam LLRs */
extern "C" int oai4g_rx_batch_tm3(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_est,
                                  int16_t *d_llr, int unscramble, void *stream)
{
  return rx_batch(cfg, n_sf, RX_TM3, "rx_batch_tm3: not a TM3 configuration (oai4g_rx_config_create_tm3)", nullptr,
                  d_rxdataF, d_est, 0, d_llr, nullptr, unscramble, stream);
}

extern "C" int oai4g_rx_batch_tm3_pilots(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_pil,
                                         int16_t *d_llr, int unscramble, void *stream)
{
  return rx_batch(cfg, n_sf, RX_TM3, "rx_batch_tm3_pilots: not a TM3 configuration", nullptr, d_rxdataF, d_pil, 1, d_llr,
                  nullptr, unscramble, stream);
}

extern "C" int oai4g_rx_batch_tm3_2cw_pilots(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF,
                                             const int32_t *d_pil, int16_t *d_llr0, int16_t *d_llr1, int unscramble,
                                             void *stream)
{
  return rx_batch(cfg, n_sf, RX_TM3, "rx_batch_tm3_pilots: not a TM3 configuration",
                  "rx_batch_tm3_2cw_pilots: not a TM3 configuration with both codewords QPSK", d_rxdataF, d_pil, 1, d_llr0,
                  d_llr1, unscramble, stream);
}

extern "C" int oai4g_rx_batch_tm3_2cw(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_est,
                                      int16_t *d_llr0, int16_t *d_llr1, int unscramble, void *stream)
{
  const char *refusal = "rx_batch_tm3_2cw: not a TM3 configuration with both codewords QPSK";
  return rx_batch(cfg, n_sf, RX_TM3, refusal, refusal, d_rxdataF, d_est, 0, d_llr0, d_llr1, unscramble, stream);
}

extern "C" int oai4g_rx_batch_tm2(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_est,
                                  int16_t *d_llr, int unscramble, void *stream)
{
  return rx_batch(cfg, n_sf, RX_TM2, "rx_batch_tm2: not a TM2 configuration (oai4g_rx_config_create_tm2)", nullptr,
                  d_rxdataF, d_est, 0, d_llr, nullptr, unscramble, stream);
}

static const char k_not_tm56[] = "rx_batch_tm56: not a TM4-6 configuration (oai4g_rx_config_create_tm56)";
extern "C" int oai4g_rx_batch_tm56(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF, const int32_t *d_est,
                                   int16_t *d_llr, int unscramble, void *stream)
{
  return rx_batch(cfg, n_sf, RX_TM56, k_not_tm56, nullptr, d_rxdataF, d_est, 0, d_llr, nullptr, unscramble, stream);
}
extern "C" int oai4g_rx_batch_tm56_pilots(oai4g_rx_config_t *cfg, int n_sf, const int32_t *d_rxdataF,
                                          const int32_t *d_pil, int16_t *d_llr, int unscramble, void *stream)
{
  return rx_batch(cfg, n_sf, RX_TM56, k_not_tm56, nullptr, d_rxdataF, d_pil, 1, d_llr, nullptr, unscramble, stream);
}

/* The rx_pdsch drop-ins' configurations, cached per calling thread (the UE calls rx_pdsch once per
 * subframe with a handful of distinct (frame, allocation, modulation, subframe) keys; building one
 * costs Gold generation, allocations and copies).  Round-robin over 32 entries; an evicted entry
 * is destroyed.  Entries of an exiting thread are not reclaimed (the UE's threads live as long as
 * the process, and tearing down device memory in thread-exit handlers can run after the HIP
 * runtime is gone). */
namespace {
struct rx_key_t {
  oai4g_frame_parms_t fp;
  uint32_t rb_alloc[4];
  rx_parms_t mp;
  uint8_t Qm, npdcch, subframe, mode;
};
struct rx_cache_t {
  rx_key_t key[32];
  oai4g_rx_config_t *cfg[32] = {};
  int next = 0;
};
thread_local rx_cache_t t_rx_cache;

oai4g_rx_config_t *rx_cached(const oai4g_frame_parms_t *fp, const uint32_t rb_alloc[4], uint8_t Qm, uint8_t npdcch,
                             uint8_t subframe, rx_mode_t mode, int nb_rx, uint8_t Qm1 = 0, uint8_t mcs0 = 0,
                             uint8_t mimo_mode = 0, uint16_t pmi_alloc = 0, uint8_t dl_power_off = 0)
{
  rx_key_t k;
  memset(&k, 0, sizeof(k));
  k.fp = *fp;
  memcpy(k.rb_alloc, rb_alloc, sizeof(k.rb_alloc));
  k.Qm = Qm; k.npdcch = npdcch; k.subframe = subframe; k.mode = (uint8_t)mode;
  k.mp.nb_rx = (uint8_t)nb_rx; k.mp.Qm1 = Qm1; k.mp.mcs0 = mcs0;
  k.mp.pmi_rule = OAI4G_RX_PMI_UE; k.mp.pmi_alloc = pmi_alloc; k.mp.mimo_mode = mimo_mode; k.mp.dl_power_off = dl_power_off;
  rx_cache_t &c = t_rx_cache;
  for (int i = 0; i < 32; i++)
    if (c.cfg[i] && memcmp(&c.key[i], &k, sizeof(k)) == 0) return c.cfg[i];
  oai4g_rx_config_t *cfg = rx_config_build(fp, rb_alloc, Qm, npdcch, 0, subframe, 1, mode, k.mp);
  if (!cfg) return nullptr;
  const int slot = c.next;
  c.next = (c.next + 1) % 32;
  if (c.cfg[slot]) {
    hipStreamSynchronize(g_scr.s);
    oai4g_rx_config_destroy(c.cfg[slot]);
  }
  c.cfg[slot] = cfg;
  c.key[slot] = k;
  return cfg;
}

/* rx_pdsch over the PDSCH symbols of one subframe (dlsim.c:3188-3260) on host buffers, the body of every
 * drop-in: rxdataF[a] and est[p * 2 + a] = [nsymb][N] of the subframe (n_planes 1: TM1's one estimate, 4:
 * ports 0 / 1 per antenna) go up, batch(dy, de, dl0, dl1) runs on g_scr.s, the n_out LLR streams (not
 * unscrambled) and log2_maxh come back; returns the stream length or -1 */
template <class Batch>
int rx_pdsch_run(oai4g_rx_config_t *cfg, const char *who, uint8_t subframe, int nb_rx, const int32_t *const *rxdataF,
                 int n_planes, const int32_t *const *est, int n_out, int16_t *const *llr, uint8_t *log2_maxh, Batch batch)
{
  if (!cfg) return -1;
  if (rx_check_batch(cfg, 1) != 0) return -1;
  const size_t gb = (size_t)cfg->h.nsymb * cfg->h.N * 4, ny = n_planes == 1 ? 1 : 2, lb = (size_t)cfg->h.llr_stride * 2;
  const int n = (int)cfg->llr_count[subframe % 10];
  stage_t st(who);
  const int r_y = st.add(ny * up256(gb)), r_e = st.add(n_planes * up256(gb));   /* [nb_rx][grid], planes [p * 2 + a] */
  const int r_l = st.add(lb * n_out, 256);
  if (!st.open()) return -1;
  for (int a = 0; a < nb_rx; a++) HCK(st.up(r_y, rxdataF[a], gb, a * gb), -1);
  for (int pa = 0; pa < n_planes; pa++)
    if ((pa & 1) < nb_rx) HCK(st.up(r_e, est[pa], gb, pa * gb), -1);
  int16_t *dl = st.ptr<int16_t>(r_l);
  if (batch(st.ptr<const int32_t>(r_y), st.ptr<const int32_t>(r_e), dl, dl + cfg->h.llr_stride) != 0) return -1;
  for (int i = 0; i < n_out; i++) HCK(st.down(llr[i], r_l, (size_t)n * 2, i * lb), -1);
  /* the shift lives in the configuration, not in the staging buffer */
  if (log2_maxh) HCK(hipMemcpyAsync(log2_maxh, cfg->d_shift.get(), 1, hipMemcpyDeviceToHost, g_scr.s), -1);
  HCK(st.sync(), -1);
  return n;
}
}  // namespace

extern "C" int oai4g_rx_pdsch_tm3(const oai4g_frame_parms_t *fp, int nb_rx, const int32_t *const *rxdataF,
                                  const int32_t *const *dl_ch_estimates, const uint32_t rb_alloc[4], uint8_t Qm0,
                                  uint8_t Qm1, uint8_t mcs0, uint8_t num_pdcch_symbols, uint8_t subframe, int16_t *llr,
                                  uint8_t *log2_maxh)
{
  NEED_INIT(-1);
  oai4g_rx_config_t *cfg = rx_cached(fp, rb_alloc, Qm0, num_pdcch_symbols, subframe, RX_TM3, nb_rx, Qm1, mcs0);
  return rx_pdsch_run(cfg, "rx_pdsch_tm3", subframe, nb_rx, rxdataF, 4, dl_ch_estimates, 1, &llr, log2_maxh,
                      [&](const int32_t *dy, const int32_t *de, int16_t *dl, int16_t *) {
                        return oai4g_rx_batch_tm3(cfg, 1, dy, de, dl, 0, g_scr.s);
                      });
}

extern "C" int oai4g_rx_pdsch_tm3_2cw(const oai4g_frame_parms_t *fp, int nb_rx, const int32_t *const *rxdataF,
                                      const int32_t *const *dl_ch_estimates, const uint32_t rb_alloc[4], uint8_t mcs0,
                                      uint8_t num_pdcch_symbols, uint8_t subframe, int16_t *llr0, int16_t *llr1,
                                      uint8_t *log2_maxh)
{
  NEED_INIT(-1);
  oai4g_rx_config_t *cfg = rx_cached(fp, rb_alloc, 2, num_pdcch_symbols, subframe, RX_TM3, nb_rx, 2, mcs0);
  int16_t *const llr[2] = {llr0, llr1};
  return rx_pdsch_run(cfg, "rx_pdsch_tm3_2cw", subframe, nb_rx, rxdataF, 4, dl_ch_estimates, 2, llr, log2_maxh,
                      [&](const int32_t *dy, const int32_t *de, int16_t *dl, int16_t *dl1) {
                        return oai4g_rx_batch_tm3_2cw(cfg, 1, dy, de, dl, dl1, 0, g_scr.s);
                      });
}

extern "C" int oai4g_rx_pdsch_tm2(const oai4g_frame_parms_t *fp, int nb_rx, const int32_t *const *rxdataF,
                                  const int32_t *const *dl_ch_estimates, const uint32_t rb_alloc[4], uint8_t Qm,
                                  uint8_t num_pdcch_symbols, uint8_t subframe, int16_t *llr, uint8_t *log2_maxh)
{
  NEED_INIT(-1);
  oai4g_rx_config_t *cfg = rx_cached(fp, rb_alloc, Qm, num_pdcch_symbols, subframe, RX_TM2, nb_rx);
  return rx_pdsch_run(cfg, "rx_pdsch_tm2", subframe, nb_rx, rxdataF, 4, dl_ch_estimates, 1, &llr, log2_maxh,
                      [&](const int32_t *dy, const int32_t *de, int16_t *dl, int16_t *) {
                        return oai4g_rx_batch_tm2(cfg, 1, dy, de, dl, 0, g_scr.s);
                      });
}

/* rx_pdsch for the single-layer precoding modes 3..7 (dual_stream_flag 0), the reference UE's subband
 * rule (OAI4G_RX_PMI_UE); buffers as for oai4g_rx_pdsch_tm2 */
extern "C" int oai4g_rx_pdsch_tm56(const oai4g_frame_parms_t *fp, int nb_rx, const int32_t *const *rxdataF,
                                   const int32_t *const *dl_ch_estimates, const uint32_t rb_alloc[4], uint8_t Qm,
                                   uint8_t mimo_mode, uint16_t pmi_alloc, uint8_t dl_power_off,
                                   uint8_t num_pdcch_symbols, uint8_t subframe, int16_t *llr, uint8_t *log2_maxh)
{
  NEED_INIT(-1);
  oai4g_rx_config_t *cfg = rx_cached(fp, rb_alloc, Qm, num_pdcch_symbols, subframe, RX_TM56, nb_rx, 0, 0, mimo_mode,
                                     pmi_alloc, dl_power_off);
  return rx_pdsch_run(cfg, "rx_pdsch_tm56", subframe, nb_rx, rxdataF, 4, dl_ch_estimates, 1, &llr, log2_maxh,
                      [&](const int32_t *dy, const int32_t *de, int16_t *dl, int16_t *) {
                        return oai4g_rx_batch_tm56(cfg, 1, dy, de, dl, 0, g_scr.s);
                      });
}

extern "C" int oai4g_rx_pdsch_siso(const oai4g_frame_parms_t *fp, const int32_t *rxdataF, const int32_t *dl_ch_estimates,
                                   const uint32_t rb_alloc[4], uint8_t Qm, uint8_t num_pdcch_symbols, uint8_t subframe,
                                   int16_t *llr, uint8_t *log2_maxh)
{
  NEED_INIT(-1);
  oai4g_rx_config_t *cfg = rx_cached(fp, rb_alloc, Qm, num_pdcch_symbols, subframe, RX_SISO, 1);
  return rx_pdsch_run(cfg, "rx_pdsch_siso", subframe, 1, &rxdataF, 1, &dl_ch_estimates, 1, &llr, log2_maxh,
                      [&](const int32_t *dy, const int32_t *dh, int16_t *dl, int16_t *) {
                        return oai4g_rx_batch(cfg, 1, dy, dh, dl, 0, g_scr.s);
                      });
}

/* dlsch_unscrambling (dlsch_scrambling.c:99-137): llr[k] *= 2 c(k) - 1 for k < 32 (1 + G / 32),
 * c_init = rnti 2^14 + q 2^13 + (Ns / 2) 2^9 + Nid_cell (mbsfn_flag = 0), on a host buffer: the
 * sequence words are set up here, the sign flips run on the GPU (k_rx_unscramble) */
extern "C" void oai4g_dlsch_unscrambling(const oai4g_frame_parms_t *fp, int mbsfn_flag, uint16_t rnti, int G,
                                         int16_t *llr, uint8_t q, uint8_t Ns)
{
  NEED_INIT();
  if (G < 0) return;
  /* dlsch_scrambling.c:115-118: the PMCH (mbsfn_flag) sequence depends on the MBSFN area only */
  const uint32_t c_init = mbsfn_flag ? ((uint32_t)(Ns >> 1) << 9) + fp->Nid_cell_mbsfn
                                     : ((uint32_t)rnti << 14) + ((uint32_t)q << 13) + ((uint32_t)(Ns >> 1) << 9) + fp->Nid_cell;
  const int words = 1 + (G >> 5);
  std::vector<uint32_t> c(words);
  gold_seq_h(c_init, c.data(), c.size());
  const size_t lb = (size_t)words * 64;
  stage_t st("dlsch_unscrambling");
  const int r_l = st.add(lb), r_c = st.add((size_t)words * 4);
  if (!st.open()) return;
  HCK(st.up(r_l, llr, lb), );
  HCK(st.up(r_c, c.data(), (size_t)words * 4), );
  HCK(oai4g_launch_unscramble(st.ptr<int16_t>(r_l), st.ptr<uint32_t>(r_c), words * 32, g_scr.s), );
  HCK(st.down(llr, r_l, lb), );
  HCK(st.sync(), );
}

/* ------------------------------------------------------------------------------------------
 * Downlink channel estimation (lte_dl_channel_estimation.c:37-701 with high_speed_flag = 1;
 * one RX antenna; the 6 / 50 / 100, 25 and 15 PRB interpolators).
 * ---------------------------------------------------------------------------------------- */
/* filt96_32.h by formula: ramp levels floor(16384 v / 6); the six filters of pilot offset k
 * (lte_dl_channel_estimation.c:105-180) as fl, f2l2, f, f2, fr, f2r2 */
extern "C" void oai4g_chest_filters(uint8_t k, int16_t out[6][24])
{
  auto lv = [](int v) { return (int16_t)((16384 * v) / 6); };
  const int s1 = k, s2 = k + 2;
  for (int t = 0; t < 24; t++) {
    const int u1 = t - s1, u2 = t - s2;
    const int16_t tri1 = (u1 >= 0 && u1 <= 10) ? lv(6 - std::abs(u1 - 5)) : 0;
    const int16_t tri2 = (u2 >= 0 && u2 <= 10) ? lv(6 - std::abs(u2 - 5)) : 0;
    out[2][t] = tri1;                                                           /* filt24_k */
    out[3][t] = tri2;                                                           /* filt24_(k+2) */
    out[4][t] = (u1 >= 11 && u1 <= 16) ? (int16_t)-lv(u1 - 11) : tri1;          /* filt24_kr2 */
    out[5][t] = (u2 >= 0 && u2 <= 10) ? lv(u2 + 1) : 0;                         /* filt24_(k+2)r */
    if (k == 0) {                                                               /* filt24_0, filt24_2 */
      out[0][t] = tri1;
      out[1][t] = tri2;
    } else {
      out[0][t] = (u1 >= 0 && u1 <= 10 && !(k == 3 && (t == 3 || t == 4))) ? lv(11 - u1) : 0;   /* filt24_kl */
      out[1][t] = (u2 >= -6 && u2 <= -1) ? (int16_t)(k == 3 && t == 0 ? 0 : -lv(-u2 - 1)) : tri2; /* _(k+2)l2 */
    }
  }
}

/* The DC-pair filters of the 25-PRB interpolator, filt24_k_dcr (last pilot below DC) and
 * filt24_(k+2)_dcl (first pilot above it), k = 0..5 (filt96_32.h:35-113; used at
 * lte_dl_channel_estimation.c:431-454).  Their slopes round irregularly, so they are table data. */
static const int16_t chest_dcr[6][24] = {
    {2730, 5461, 8192, 10922, 13653, 16384, 14043, 11703, 9362, 7022, 4681},
    {0, 2730, 5461, 8192, 10922, 13653, 16384, 14043, 11703, 9362, 7022, 4681},
    {0, 0, 2730, 5461, 8192, 10922, 13653, 16384, 14043, 11703, 9362, 4681, 2341},
    {0, 0, 0, 2730, 5461, 8192, 10922, 13653, 16384, 14043, 11703, 7022, 4681, 2341},
    {0, 0, 0, 0, 2730, 5461, 8192, 10922, 13653, 16384, 14043, 11703, 7022, 4681, 2341},
    {0, 0, 0, 0, 0, 2730, 5461, 8192, 10922, 13653, 16384, 11703, 9362, 7022, 4681, 2730}};
static const int16_t chest_dcl[6][24] = {
    {0, 0, 2341, 4681, 7022, 9362, 11703, 16384, 13653, 10922, 8192, 5461, 2730},
    {0, 0, 0, 2341, 4681, 7022, 9362, 14043, 16384, 13653, 10922, 8192, 5461, 2730},
    {0, 0, 0, 0, 2341, 7022, 9362, 11703, 14043, 16384, 13653, 10922, 8192, 5461, 2730},
    {0, 0, 0, 0, 0, 2341, 4681, 9362, 11703, 14043, 16384, 13653, 10922, 8192, 5461, 2730},
    {0, 0, 0, 0, 0, 0, 4681, 7022, 9362, 11703, 14043, 16384, 13653, 10922, 8192, 5461, 2730},
    {0, 0, 0, 0, 0, 0, 0, 4681, 7022, 9362, 11703, 14043, 16384, 13653, 10922, 8192, 5461, 2730}};

extern "C" void oai4g_chest_dc_filters(uint8_t k, int16_t out[2][24])
{
  memcpy(out[0], chest_dcr[k % 6], sizeof(out[0]));
  memcpy(out[1], chest_dcl[k % 6], sizeof(out[1]));
}

struct oai4g_chest_config {
  chest_dev_t h;
  dev_buf<chest_dev_t> d;
};

static int chest_fill(const oai4g_frame_parms_t *fp, uint8_t p, chest_dev_t &h)
{
  const uint32_t N_RB = fp->N_RB_DL;
  if (p > 1) { set_err("lte_dl_channel_estimation: p %d (ports 0 / 1 only)", p); return -1; }
  memset(&h, 0, sizeof(h));
  h.N = fp->ofdm_symbol_size;
  h.N_RB = N_RB;
  h.nsymb = fp->Ncp == 0 ? 14 : 12;
  h.elem_syms = h.nsymb;
  h.next_syms = h.nsymb;
  h.Ncp = fp->Ncp;
  h.fco = fp->first_carrier_offset;
  h.p = p;
  h.branch = (N_RB == 6 || N_RB == 15 || N_RB == 25 || N_RB == 50 || N_RB == 100) ? 1 : 0;   /* others: "not implemented" */
  for (int l01 = 0; l01 < 2; l01++) {
    const uint32_t nu = p == 0 ? (l01 ? 3 : 0) : (l01 ? 0 : 3);
    h.k[l01] = (nu + fp->nushift) % 6;
    /* the pilots above DC start at bin 1 + k; the 15-PRB branch uses 1 + nushift + 3 p whatever
     * nu is (lte_dl_channel_estimation.c:582) */
    h.off2[l01] = N_RB == 15 ? 1 + fp->nushift + 3 * p : 1 + h.k[l01];
    oai4g_chest_filters((uint8_t)h.k[l01], h.filt[l01]);
    memcpy(h.filt[l01][6], chest_dcr[h.k[l01]], sizeof(h.filt[l01][6]));
    memcpy(h.filt[l01][7], chest_dcl[h.k[l01]], sizeof(h.filt[l01][7]));
  }
  lte_gold_table_h(fp, h.gold);
  return 0;
}

extern "C" oai4g_chest_config_t *oai4g_chest_config_create(const oai4g_frame_parms_t *fp, uint8_t p,
                                                           uint8_t first_subframe, uint8_t subframe_step)
{
  NEED_INIT(nullptr);
  std::unique_ptr<oai4g_chest_config> cfg(new oai4g_chest_config());
  if (chest_fill(fp, p, cfg->h) != 0) return nullptr;
  cfg->h.first_sf = first_subframe % 10;
  cfg->h.sf_step = subframe_step;
  if (cfg->d.upload(&cfg->h, 1) != hipSuccess) {
    set_err("chest_config: device allocation / upload failed");
    return nullptr;
  }
  return cfg.release();
}

extern "C" int oai4g_chest_config_set_stride(oai4g_chest_config_t *cfg, uint32_t subframes_per_element,
                                             uint32_t next_subframes)
{
  NEED_INIT(-1);
  if (!cfg || subframes_per_element < 1 || next_subframes < 1) { set_err("chest_config_set_stride: bad arguments"); return -1; }
  cfg->h.elem_syms = cfg->h.nsymb * subframes_per_element;
  cfg->h.next_syms = cfg->h.nsymb * next_subframes;
  if (hipMemcpy(cfg->d.get(), &cfg->h, sizeof(chest_dev_t), hipMemcpyHostToDevice) != hipSuccess) {
    set_err("chest_config_set_stride: upload failed");
    return -1;
  }
  return 0;
}

extern "C" void oai4g_chest_config_destroy(oai4g_chest_config_t *cfg)
{
  if (cfg) delete cfg;
}

extern "C" int oai4g_chest_batch(oai4g_chest_config_t *cfg, int n_sf, const int32_t *d_rxdataF, int32_t *d_est,
                                 void *stream)
{
  NEED_INIT(-1);
  if (!cfg || n_sf < 0) { set_err("chest_batch: bad arguments"); return -1; }
  HCK(oai4g_launch_chest(cfg->d.get(), &cfg->h, n_sf, d_rxdataF, d_est, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_chest_batch_pilots(oai4g_chest_config_t *cfg, int n_sf, const int32_t *d_rxdataF, int32_t *d_pil,
                                        void *stream)
{
  NEED_INIT(-1);
  if (!cfg || n_sf < 0) { set_err("chest_batch_pilots: bad arguments"); return -1; }
  HCK(oai4g_launch_chest_pilots(cfg->d.get(), &cfg->h, n_sf, d_rxdataF, d_pil, (hipStream_t)stream), -1);
  return 0;
}

/* Fused batch: estimation + demodulation without the estimate buffer (k_rx_chest); the two
 * configurations must describe the same frame and subframe sequence. */
extern "C" int oai4g_rx_batch_estimated(oai4g_rx_config_t *rx, oai4g_chest_config_t *ce, int n_sf,
                                        const int32_t *d_rxdataF, int16_t *d_llr, int unscramble, void *stream)
{
  NEED_INIT(-1);
  if (!rx || !ce || n_sf < 0) { set_err("rx_batch_estimated: bad arguments"); return -1; }
  if (rx->h.N != ce->h.N || rx->h.nsymb != ce->h.nsymb || rx->h.first_sf != ce->h.first_sf ||
      rx->h.sf_step != ce->h.sf_step || ce->h.p != 0 || ce->h.N_RB > 100) {
    set_err("rx_batch_estimated: the demodulation and estimation configurations differ (frame, subframes, port 0)");
    return -1;
  }
  const int go = rx_prepare(rx, n_sf, RX_SISO, "rx_batch_estimated: not a TM1 configuration (oai4g_rx_config_create)");
  if (go <= 0) return go;
  HCK(oai4g_launch_rx_chest(ce->d.get(), rx->d.get(), &rx->h, n_sf, d_rxdataF, d_llr, rx->d_shift.get(), unscramble,
                            (hipStream_t)stream), -1);
  return 0;
}

/* lte_dl_channel_estimation drop-in on host buffers: rxdataF / dl_ch_estimates = [nsymb][N] of the
 * subframe (the UE's rxdataF and dl_ch_estimates[eNB_offset 0][(p << 1) + 0]); Ns, p, l, symbol as
 * slot_fep passes them (slot_fep.c:188-192) */
extern "C" int oai4g_lte_dl_channel_estimation(const oai4g_frame_parms_t *fp, const int32_t *rxdataF,
                                               int32_t *dl_ch_estimates, uint8_t Ns, uint8_t p, uint8_t l,
                                               uint8_t symbol)
{
  NEED_INIT(-1);
  const uint32_t nsymb = fp->Ncp == 0 ? 14 : 12, p1 = fp->Ncp ? 3 : 4, p2 = fp->Ncp ? 6 : 7, p3 = fp->Ncp ? 9 : 11;
  if (Ns >= 20 || (symbol != 0 && symbol != p1 && symbol != p2 && symbol != p3)) {
    set_err("lte_dl_channel_estimation: Ns %d / symbol %d is not a pilot symbol", Ns, symbol);
    return -1;
  }
  chest_dev_t h;
  if (chest_fill(fp, p, h) != 0) return -1;
  const size_t N = fp->ofdm_symbol_size, rb = N * 4;
  stage_t st("lte_dl_channel_estimation");
  const int r_c = st.add(sizeof(chest_dev_t)), r_e = st.add(nsymb * rb), r_r = st.add(rb);
  if (!st.open()) return -1;
  /* the call reads the previous pilot row and writes its own row plus the rows between the two
   * (k_chest_symbol / ce_interp): only those rows cross PCIe */
  const uint32_t prev_row = symbol == 0 ? p3 : symbol == p1 ? 0 : symbol == p2 ? p1 : p2;
  auto rows_d2h = [&](uint32_t r0, uint32_t n) { return st.down(dl_ch_estimates + (size_t)r0 * N, r_e, n * rb, r0 * rb); };
  HCK(st.up(r_c, &h, sizeof(h)), -1);
  HCK(st.up(r_e, dl_ch_estimates + (size_t)prev_row * N, rb, prev_row * rb), -1);
  HCK(st.up(r_r, rxdataF + (size_t)symbol * N, rb), -1);
  HCK(oai4g_launch_chest_symbol(st.ptr<chest_dev_t>(r_c), &h, st.ptr<int32_t>(r_r), st.ptr<int32_t>(r_e), Ns, l, symbol,
                                g_scr.s), -1);
  if (symbol == 0) {
    HCK(rows_d2h(p3 + 1, nsymb - 1 - p3), -1);
    HCK(rows_d2h(0, 1), -1);
  } else
    HCK(rows_d2h(prev_row + 1, symbol - prev_row), -1);
  HCK(st.sync(), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * lte_est_freq_offset (PHY/LTE_ESTIMATION/lte_est_freq_offset.c:104-193) and dl_ch_estimates_time
 * (lte_dl_channel_estimation.c:704-738)
 * ---------------------------------------------------------------------------------------- */
static int fo_rows(const oai4g_frame_parms_t *fp, int l, uint32_t *row_off, uint32_t *prev_off)
{
  const int lp = 4 - fp->Ncp;
  if (l != 0 && l != lp) {
    set_err("lte_est_freq_offset: l (%d) must be 0 or %d", l, lp);   /* :127-130 */
    return -1;
  }
  if (fp->N_RB_DL < 4 || (size_t)fp->N_RB_DL * 12 + 12 > fp->ofdm_symbol_size) {
    set_err("lte_est_freq_offset: N_RB_DL %d not supported", fp->N_RB_DL);
    return -1;
  }
  *row_off = (uint32_t)l * fp->ofdm_symbol_size;
  *prev_off = (uint32_t)(l == 0 ? lp : 0) * fp->ofdm_symbol_size;
  return 0;
}

extern "C" int oai4g_freq_offset_omega_batch(const oai4g_frame_parms_t *fp, int n_jobs, const int32_t *d_est,
                                             size_t est_stride, int l, int32_t *d_omega, void *stream)
{
  NEED_INIT(-1);
  uint32_t ro, po;
  if (fo_rows(fp, l, &ro, &po) != 0) return -1;
  if (n_jobs < 0 || (n_jobs > 0 && (!d_est || !d_omega))) { set_err("freq_offset_omega_batch: bad arguments"); return -1; }
  HCK(oai4g_launch_freq_offset(d_est, est_stride, n_jobs, fp->N_RB_DL, ro, po, d_omega, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_freq_offset_update(const oai4g_frame_parms_t *fp, int32_t omega, int *freq_offset, int *first_run)
{
  if (!fp || !freq_offset || !first_run) { set_err("freq_offset_update: bad arguments"); return -1; }
  const double phase = atan2((double)(int16_t)((uint32_t)omega >> 16), (double)(int16_t)omega);   /* :168 */
  const int est = (int)(phase / (2 * M_PI) / (fp->Ncp == 0 ? 285.8e-6 : 2.5e-4));              /* :174 */
  if (*first_run == 1) {                                                                          /* :178-182 */
    *freq_offset = est;
    *first_run = 0;
  } else
    *freq_offset = (est * (1 << 10) + *freq_offset * (32767 - (1 << 10))) >> 15;
  return 0;
}

/* the reference's function-static first_run (:117), shared by every caller as there */
static int g_fo_first_run = 1;
static std::mutex g_fo_mu;

extern "C" int oai4g_lte_est_freq_offset(int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *fp, int l,
                                         int *freq_offset, int reset)
{
  NEED_INIT(-1);
  if (!dl_ch_estimates || !dl_ch_estimates[0] || !fp || !freq_offset) { set_err("lte_est_freq_offset: bad arguments"); return -1; }
  std::lock_guard<std::mutex> lk(g_fo_mu);
  if (reset != 0) g_fo_first_run = 1;                                                             /* :122-123 */
  uint32_t ro, po;
  if (fo_rows(fp, l, &ro, &po) != 0) return -1;
  const size_t words = (size_t)(4 - fp->Ncp + 1) * fp->ofdm_symbol_size;   /* rows 0 .. 4 - Ncp */
  stage_t st("lte_est_freq_offset");
  const int r_est = st.add(words * 4), r_om = st.add(4, 252);
  if (!st.open()) return -1;
  int32_t om = 0;
  HCK(st.up(r_est, dl_ch_estimates[0], words * 4), -1);
  HCK(oai4g_launch_freq_offset(st.ptr<int32_t>(r_est), 0, 1, fp->N_RB_DL, ro, po, st.ptr<int32_t>(r_om), g_scr.s), -1);
  HCK(st.down(&om, r_om, 4), -1);
  HCK(st.sync(), -1);
  return oai4g_freq_offset_update(fp, om, freq_offset, &g_fo_first_run);
}

static int chest_time_log2n(const oai4g_frame_parms_t *fp)
{
  const int l2 = fp->log2_symbol_size;
  return (l2 >= 7 && l2 <= 11) ? l2 : 9;   /* the switch's default: idft512 (:713-735) */
}

extern "C" int oai4g_chest_time_batch(const oai4g_frame_parms_t *fp, int n_jobs, const int32_t *d_est,
                                      size_t est_stride, int32_t *d_time, size_t time_stride, void *stream)
{
  NEED_INIT(-1);
  const int l2 = chest_time_log2n(fp);
  if (!fp || n_jobs < 0 || (n_jobs > 0 && (!d_est || !d_time)) || est_stride < ((size_t)1 << l2) + 8 ||
      time_stride < ((size_t)1 << l2)) {
    set_err("chest_time_batch: bad arguments (an estimate plane must hold N + 8 words)");
    return -1;
  }
  HCK(oai4g_launch_idft_strided(d_est, d_time, l2, n_jobs, est_stride, 8, time_stride, 1, g_tw, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_dl_ch_estimates_time(const oai4g_frame_parms_t *fp, int nb_antennas_rx,
                                          const int32_t *const *dl_ch_estimates, int32_t *const *dl_ch_estimates_time)
{
  NEED_INIT(-1);
  if (!fp || !dl_ch_estimates || !dl_ch_estimates_time || nb_antennas_rx < 1 || nb_antennas_rx > 2) {
    set_err("dl_ch_estimates_time: bad arguments");
    return -1;
  }
  const int l2 = chest_time_log2n(fp);
  const size_t n = (size_t)1 << l2, in_w = n + 8;
  const int ntx = fp->nb_antennas_tx_eNB ? fp->nb_antennas_tx_eNB : fp->nb_antennas_tx;
  int planes[8], np = 0;
  for (int aarx = 0; aarx < nb_antennas_rx; aarx++)        /* :731-737, NULL planes skipped */
    for (int p = 0; p < ntx && p < 4; p++)
      if (dl_ch_estimates[(p << 1) + aarx]) planes[np++] = (p << 1) + aarx;
  if (np == 0) return 0;
  const size_t ib = (size_t)np * in_w * 4, ob = (size_t)np * n * 4;
  stage_t st("dl_ch_estimates_time");
  const int r_in = st.add(ib), r_out = st.add(ob, 256);
  if (!st.open()) return -1;
  for (int i = 0; i < np; i++) HCK(st.up(r_in, dl_ch_estimates[planes[i]], in_w * 4, i * in_w * 4), -1);
  HCK(oai4g_launch_idft_strided(st.ptr<int32_t>(r_in), st.ptr<int32_t>(r_out), l2, np, in_w, 8, n, 1, g_tw, g_scr.s),
      -1);                                    /* words 8 .. N + 7 */
  for (int i = 0; i < np; i++) HCK(st.down(dl_ch_estimates_time[planes[i]], r_out, n * 4, i * n * 4), -1);
  HCK(st.sync(), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * UE control decoding (oai4g_ctrl_rx.hip): the tail-biting Viterbi, dci_decoding (dci.c:2426-2489)
 * and rx_pbch from the quantised soft bits on (pbch.c:975-1043).
 * ---------------------------------------------------------------------------------------- */
/* plan[3 i + s]: the k-th non-<NULL> entry of generate_dummy_w_cc's w (lte_rate_matching.c:384: stream s,
 * then column, then row; <NULL> where bitrev_cc[col] < ND in row 0) is where lte_rate_matching_cc_rx
 * (:834) accumulates e[k], e[k + 3 D], ..., and sub_block_deinterleaving_cc (:245) moves that entry to
 * d[3 (32 row + bitrev_cc[col] - ND) + s] */
static void cc_rx_plan_h(uint32_t D, uint16_t *plan)
{
  const uint32_t R = (D + 31) >> 5, ND = 32 * R - D;
  for (uint32_t s = 0; s < 3; s++) {
    uint32_t j = 0;
    for (uint32_t col = 0; col < 32; col++)
      for (uint32_t row = 0; row < R; row++) {
        const uint32_t idx = 32 * row + bitrev_cc[col];
        if (idx < ND) continue;
        plan[3 * (idx - ND) + s] = (uint16_t)(s * D + j++);
      }
  }
}

extern "C" int oai4g_cc_rx_plan(uint32_t D, uint16_t *plan)
{
  if (D == 0 || D > OAI4G_CC_NMAX || !plan) { set_err("cc_rx_plan: D %u (1..%d)", D, OAI4G_CC_NMAX); return -1; }
  cc_rx_plan_h(D, plan);
  return (int)(3 * D);
}

#define CC_REC 68u   /* drop-in record: 64 decoded bytes + the 4-byte trailer */
/* one decode through the scratch buffer: e (e_bytes), the job, its plan, the PBCH Gold words */
static int cc_decode_one(const char *who, const int8_t *e, size_t e_bytes, cc_job_t job, const uint16_t *plan,
                         uint32_t n_plan, const uint32_t *gold, uint32_t n_gold, uint8_t quarter, bool raw,
                         uint8_t rec[CC_REC], uint8_t *metrics)
{
  stage_t st(who);
  const int r_e = st.add(e_bytes), r_job = st.add(sizeof(cc_job_t), 244);
  const int r_plan = st.add(3 * 61 * 2, 1682), r_gold = st.add(60 * 4, 272);   /* the largest plan (D = 45 + 16), the PBCH's words */
  const int r_q = st.add(1, 255), r_rec = st.add(CC_REC, 188), r_met = st.add(64, 192 + 256);
  if (!st.open()) return -1;
  job.e_off = 0;
  job.plan_off = 0;
  HCK(st.up(r_e, e, e_bytes), -1);
  HCK(st.up(r_job, &job, sizeof(job)), -1);
  if (n_plan) HCK(st.up(r_plan, plan, (size_t)n_plan * 2), -1);
  if (n_gold) HCK(st.up(r_gold, gold, (size_t)n_gold * 4), -1);
  HCK(st.up(r_q, &quarter, 1), -1);
  cc_args_t a;
  memset(&a, 0, sizeof(a));
  a.e = st.ptr<const int8_t>(r_e);
  a.e_stride = 0;
  a.jobs = st.ptr<const cc_job_t>(r_job);
  a.n_jobs = a.n_items = 1;
  a.plan = st.ptr<const uint16_t>(r_plan);
  a.gold = n_gold ? st.ptr<const uint32_t>(r_gold) : nullptr;
  a.quarter = st.ptr(r_q);
  a.out = st.ptr(r_rec);
  a.out_stride = CC_REC;
  a.metrics = metrics ? st.ptr(r_met) : nullptr;
  a.raw = raw ? 1 : 0;
  HCK(oai4g_launch_cc_decode(a, job.D, g_scr.s), -1);
  HCK(st.down(rec, r_rec, CC_REC), -1);
  if (metrics) HCK(st.down(metrics, r_met, 64), -1);
  HCK(st.sync(), -1);
  return 0;
}

static int viterbi_one(const char *who, const int8_t *y, uint16_t n, uint8_t rec[CC_REC], uint8_t *metrics)
{
  if (!y || n == 0 || n > OAI4G_CC_NMAX) { set_err("%s: n %u (1..%d)", who, n, OAI4G_CC_NMAX); return -1; }
  NEED_INIT(-1);
  cc_job_t job = {};
  job.D = n;
  return cc_decode_one(who, y, 3 * (size_t)n, job, nullptr, 0, nullptr, 0, 0, true, rec, metrics);
}

extern "C" int oai4g_phy_viterbi_lte(const int8_t *y, uint8_t *decoded_bytes, uint16_t n)
{
  uint8_t rec[CC_REC];
  if (!decoded_bytes) { set_err("phy_viterbi_lte: null output"); return -1; }
  if (viterbi_one("phy_viterbi_lte", y, n, rec, nullptr) != 0) return -1;
  for (uint32_t i = 0; i < ((uint32_t)n + 7) >> 3; i++) decoded_bytes[i] = (uint8_t)(decoded_bytes[i] + rec[i]);   /* '+=' (:400) */
  return rec[CC_REC - 2];
}

extern "C" int oai4g_diag_viterbi_lte(const int8_t *y, uint16_t n, uint8_t *decoded, uint8_t metrics[64],
                                      uint8_t *start_state)
{
  uint8_t rec[CC_REC];
  if (!decoded || !metrics || !start_state) { set_err("diag_viterbi_lte: null output"); return -1; }
  if (viterbi_one("diag_viterbi_lte", y, n, rec, metrics) != 0) return -1;
  memcpy(decoded, rec, ((size_t)n + 7) >> 3);
  *start_state = rec[CC_REC - 1];
  return rec[CC_REC - 2];
}

extern "C" int oai4g_dci_decoding_crc(uint8_t DCI_LENGTH, uint8_t aggregation_level, const int8_t *e,
                                      uint8_t *decoded_output, uint16_t *crc)
{
  if (aggregation_level > 3) { set_err("dci_decoding: illegal aggregation_level %u", aggregation_level); return -1; }
  if (DCI_LENGTH == 0 || DCI_LENGTH > 45) {   /* MAX_DCI_SIZE_BITS (dci.h:2979) sizes the reference's buffers */
    set_err("dci_decoding: DCI_LENGTH %u (1..45)", DCI_LENGTH);
    return -1;
  }
  if (!e || !decoded_output) { set_err("dci_decoding: null buffer"); return -1; }
  NEED_INIT(-1);
  const uint32_t D = (uint32_t)DCI_LENGTH + 16;
  uint16_t plan[3 * 61];
  cc_rx_plan_h(D, plan);
  cc_job_t job = {};
  job.E = (uint16_t)(72u << aggregation_level);
  job.D = (uint16_t)D;
  job.crc_bits = DCI_LENGTH;
  uint8_t rec[CC_REC];
  if (cc_decode_one("dci_decoding", e, job.E, job, plan, 3 * D, nullptr, 0, 0, false, rec, nullptr) != 0) return -1;
  memset(decoded_output, 0, 2 + (D >> 3));                            /* :2477 */
  for (uint32_t i = 0; i < (D + 7) >> 3; i++) decoded_output[i] = rec[i];
  if (crc) *crc = (uint16_t)(rec[CC_REC - 4] | (rec[CC_REC - 3] << 8));
  return 0;
}

extern "C" int oai4g_dci_decoding(uint8_t DCI_LENGTH, uint8_t aggregation_level, const int8_t *e, uint8_t *decoded_output)
{
  return oai4g_dci_decoding_crc(DCI_LENGTH, aggregation_level, e, decoded_output, nullptr);
}

/* lte_gold_generic words of c_init = Nid_cell over the PBCH's E soft bits (pbch_unscrambling, pbch.c:785) */
static uint32_t pbch_gold_h(uint32_t Nid, uint32_t E, uint32_t w[60])
{
  const uint32_t nw = (E + 31) / 32;
  gold_seq_h(Nid, w, nw);
  return nw;
}

extern "C" int oai4g_pbch_decode(const int8_t *llr, const oai4g_frame_parms_t *fp, uint8_t frame_mod4,
                                 uint8_t decoded_output[3])
{
  if (!llr || !fp || !decoded_output || frame_mod4 > 3) { set_err("pbch_decode: frame_mod4 %u or a null argument", frame_mod4); return -1; }
  NEED_INIT(-1);
  const uint32_t E = fp->Ncp == 0 ? 1920 : 1728;
  uint16_t plan[120];
  uint32_t gold[60];
  cc_rx_plan_h(40, plan);
  const uint32_t nw = pbch_gold_h(fp->Nid_cell, E, gold);
  cc_job_t job = {};
  job.E = (uint16_t)E;
  job.D = 40;
  job.crc_bits = 24;
  uint8_t rec[CC_REC];
  if (cc_decode_one("pbch_decode", llr, E, job, plan, 120, gold, nw, frame_mod4, false, rec, nullptr) != 0) return -1;
  for (int i = 0; i < 3; i++) decoded_output[2 - i] = rec[i];         /* pbch.c:1017 */
  const uint32_t crc = rec[CC_REC - 4] | ((uint32_t)rec[CC_REC - 3] << 8);
  set_err("");
  return crc == 0 ? 1 : (crc == 0xFFFFu ? 2 : (crc == 0x5555u ? 4 : -1));
}

/* device constants of the batched PBCH decode, kept for the last (Nid_cell, E) */
static std::mutex g_pbch_rx_mu;
static uint8_t *g_pbch_rx_dev = nullptr;
static uint32_t g_pbch_rx_key = 0xFFFFFFFFu;

extern "C" int oai4g_pbch_decode_batch(const int8_t *d_llr, int n, const oai4g_frame_parms_t *fp,
                                       const uint8_t *d_frame_mod4, uint8_t *d_out, void *stream)
{
  if (n < 0 || !fp || (n > 0 && (!d_llr || !d_frame_mod4 || !d_out))) { set_err("pbch_decode_batch: bad arguments"); return -1; }
  NEED_INIT(-1);
  if (n == 0) return 0;
  const uint32_t E = fp->Ncp == 0 ? 1920 : 1728, key = ((uint32_t)fp->Nid_cell << 16) | E;
  /* held until the launch is enqueued: another thread's cell may replace the constants only after a device
   * synchronisation that then covers this launch */
  std::lock_guard<std::mutex> lk(g_pbch_rx_mu);
  {
    if (!g_pbch_rx_dev) {             /* allocated once and kept as long as the process */
      dev_buf<uint8_t> b;
      HCK(b.reserve(1024), -1);
      g_pbch_rx_dev = b.release();
    }
    if (g_pbch_rx_key != key) {
      uint8_t h[1024] = {};
      cc_job_t job = {};
      job.E = (uint16_t)E;
      job.D = 40;
      job.crc_bits = 24;
      memcpy(h, &job, sizeof(job));
      cc_rx_plan_h(40, (uint16_t *)(h + 256));
      pbch_gold_h(fp->Nid_cell, E, (uint32_t *)(h + 512));
      HCK(hipDeviceSynchronize(), -1);                                /* earlier launches may still read the old constants */
      HCK(hipMemcpy(g_pbch_rx_dev, h, sizeof(h), hipMemcpyHostToDevice), -1);
      g_pbch_rx_key = key;
    }
  }
  cc_args_t a;
  memset(&a, 0, sizeof(a));
  a.e = d_llr;
  a.e_stride = E;
  a.jobs = (const cc_job_t *)g_pbch_rx_dev;
  a.n_jobs = 1;
  a.n_items = (uint32_t)n;
  a.plan = (const uint16_t *)(g_pbch_rx_dev + 256);
  a.gold = (const uint32_t *)(g_pbch_rx_dev + 512);
  a.quarter = d_frame_mod4;
  a.out = d_out;
  a.out_stride = 4;
  a.pbch_out = 1;
  HCK(oai4g_launch_cc_decode(a, 40, (hipStream_t)stream), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * PDCCH receive: the soft-bit gather of rx_pdcch after compensation (dci.c:1852-1897), the DCI
 * search of dci_decoding_procedure0 (:2547-2786) and its batched form.
 * ---------------------------------------------------------------------------------------- */
static int pdcch_rx_geometry_ok(const char *who, const oai4g_frame_parms_t *fp, uint32_t subframe, uint8_t npd)
{
  if (!fp) { set_err("%s: null frame parameters", who); return 0; }
  if (fp->nb_antennas_tx_eNB == 4) { set_err("%s: 4 TX ports are not defined by the reference's demapping (dci.c:420)", who); return 0; }
  if (fp->phich_duration != 0 || fp->Ncp != 0) {
    set_err("%s: only the normal cyclic prefix with normal PHICH duration is supported", who);
    return 0;
  }
  if (subframe > 9 || npd < 1 || npd > 3 || oai4g_get_nquad(npd, fp, 1) == 0) {
    set_err("%s: subframe %u / num_pdcch_symbols %u / no PDCCH geometry for N_RB_DL %u", who, subframe, npd, fp->N_RB_DL);
    return 0;
  }
  return 1;
}

/* tab[i], soft bit i of e_rx: int16 index into rxdataF_comp | negate << 31, or OAI4G_PDCCH_NONE */
static int pdcch_soft_table_h(const oai4g_frame_parms_t *fp, uint8_t subframe, uint8_t npd, std::vector<uint32_t> &tab)
{
  const uint8_t mi = oai4g_get_mi(fp, subframe);
  const uint32_t Mquad = oai4g_get_nquad(npd, fp, mi), NRE = (uint32_t)fp->N_RB_DL * 12;
  const int Msymb = ((2 * 33 + 22) * 72) / 2;
  int Msymb2;
  switch (fp->N_RB_DL) {
  case 100: Msymb2 = Msymb; break;
  case 50: Msymb2 = Msymb >> 1; break;
  case 6: Msymb2 = Msymb * 6 / 100; break;
  default: Msymb2 = Msymb >> 2; break;
  }
  uint16_t pcf[4], phr[56][3];
  uint8_t fi;
  memset(phr, 0, sizeof(phr));
  pcfich_regs(fp, pcf, &fi);
  oai4g_generate_phich_reg_mapping(fp, phr);
  const uint32_t ng = phich_ngroup(fp);
  auto taken = [&](uint32_t kp, uint32_t lp) {           /* check_phich_reg (:62-121), normal prefix */
    if (lp > 0) return false;
    const uint32_t m = kp / 6;
    if (m == pcf[0] || m == pcf[1] || m == pcf[2] || m == pcf[3]) return true;
    if (mi > 0)
      for (uint32_t i = 0; i < ng && i < 56; i++)
        if (m == phr[i][0] || m == phr[i][1] || m == phr[i][2]) return true;
    return false;
  };
  /* pdcch_demapping (:342-446): wbar[mprime] <- llr RE index; its break leaves the inner loop only */
  std::vector<uint32_t> wbar;
  uint32_t re_offset = 0, re_offset0 = 0;
  for (uint32_t kp = 0; kp < NRE; kp++) {
    for (uint32_t lp = 0; lp < npd; lp++) {
      const uint32_t so = NRE * lp;
      if (taken(kp, lp)) {
        if (lp == 0 && kp % 6 == 0) re_offset0 += 4;
      } else if (lp == 0) {
        if (kp % 12 == 0 || kp % 12 == 6)
          for (uint32_t i = 0; i < 4; i++) wbar.push_back(so + re_offset0++);
      } else if (kp % 12 == 0 || kp % 12 == 4 || kp % 12 == 8) {
        for (uint32_t i = 0; i < 4; i++) wbar.push_back(so + re_offset + i);
      }
      if (wbar.size() >= (size_t)Msymb2) break;
    }
    re_offset++;
  }
  /* pdcch_deinterleaving (:449-549): wtemp[(i + Nid) % Mquad] = wbar[i]; z[perm[k]] = wtemp[k] */
  std::vector<uint32_t> z((size_t)4 * Mquad, OAI4G_PDCCH_NONE);
  const uint32_t RCC = (Mquad + 31) >> 5, ND = (RCC << 5) - Mquad;
  uint32_t k = 0;
  for (uint32_t col = 0; col < 32; col++)
    for (uint32_t row = 0, idx = bitrev_cc[col]; row < RCC; row++, idx += 32)
      if (idx >= ND) {
        const uint32_t i = (k + Mquad - fp->Nid_cell % Mquad) % Mquad;   /* the wbar quadruplet behind wtemp[k] */
        for (uint32_t j = 0; j < 4; j++)
          if ((size_t)4 * i + j < wbar.size()) z[(size_t)4 * (idx - ND) + j] = wbar[(size_t)4 * i + j];
        k++;
      }
  /* pdcch_unscrambling (:1932-1961) over 72 nCCE soft bits */
  const uint32_t n = 8 * Mquad, nuns = 72u * (Mquad / 9);
  std::vector<uint32_t> sw((n + 31) / 32);
  gold_seq_h(((uint32_t)subframe << 9) + fp->Nid_cell, sw.data(), sw.size());
  tab.assign(n, OAI4G_PDCCH_NONE);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t re = z[i >> 1];
    if (re == OAI4G_PDCCH_NONE) continue;
    const uint32_t neg = (i < nuns && ((sw[i >> 5] >> (i & 31)) & 1u) == 0) ? 1u : 0u;
    tab[i] = (2 * re + (i & 1)) | (neg << 31);
  }
  return (int)n;
}

extern "C" int oai4g_pdcch_soft_bit_table(const oai4g_frame_parms_t *fp, uint8_t subframe, uint8_t npd, uint32_t *table,
                                          uint32_t cap)
{
  if (!pdcch_rx_geometry_ok("pdcch_soft_bit_table", fp, subframe, npd)) return -1;
  std::vector<uint32_t> tab;
  const int n = pdcch_soft_table_h(fp, subframe, npd, tab);
  if (!table || (uint32_t)n > cap) { set_err("pdcch_soft_bit_table: room for %u of %d entries", cap, n); return -1; }
  memcpy(table, tab.data(), (size_t)n * 4);
  return n;
}

extern "C" int oai4g_pdcch_soft_bits(const int32_t *rxdataF_comp, const oai4g_frame_parms_t *fp, uint8_t subframe,
                                     uint8_t npd, int8_t *e_rx)
{
  if (!pdcch_rx_geometry_ok("pdcch_soft_bits", fp, subframe, npd)) return -1;
  if (!rxdataF_comp || !e_rx) { set_err("pdcch_soft_bits: null buffer"); return -1; }
  NEED_INIT(-1);
  std::vector<uint32_t> tab;
  const int n = pdcch_soft_table_h(fp, subframe, npd, tab);
  const size_t cb = (size_t)npd * fp->N_RB_DL * 12 * 4;
  stage_t st("pdcch_soft_bits");
  const int r_comp = st.add(cb), r_tab = st.add((size_t)n * 4), r_e = st.add((size_t)n, 256);
  if (!st.open()) return -1;
  HCK(st.up(r_comp, rxdataF_comp, cb), -1);
  HCK(st.up(r_tab, tab.data(), (size_t)n * 4), -1);
  HCK(oai4g_launch_pdcch_soft(st.ptr<const int16_t>(r_comp), st.ptr<const uint32_t>(r_tab), (uint32_t)n,
                              st.ptr<int8_t>(r_e), g_scr.s), -1);
  HCK(st.down(e_rx, r_e, (size_t)n), -1);
  HCK(st.sync(), -1);
  return n;
}

/* the candidates of one dci_decoding_procedure0 call (:2576-2624) */
static void pdcch_candidates_h(const oai4g_frame_parms_t *fp, uint8_t npd, uint8_t mi, uint8_t subframe, uint16_t crnti,
                               int do_common, uint8_t L, std::vector<uint16_t> &cce)
{
  const uint32_t nCCE = oai4g_get_nCCE(npd, fp, mi), L2 = 1u << L;
  if (nCCE > oai4g_get_nCCE(3, fp, 1) || nCCE < L2) return;
  uint32_t Yk = 0, nb;
  if (do_common == 1) {
    nb = L2 == 4 ? 4 : 2;
  } else {
    Yk = crnti;
    for (uint32_t i = 0; i <= subframe; i++) Yk = (Yk * 39827u) % 65537u;
    Yk %= nCCE / L2;
    nb = L2 <= 2 ? 6 : 2;
  }
  if (nb * L2 > nCCE) nb = nCCE / L2;
  for (uint32_t m = 0; m < nb; m++) cce.push_back((uint16_t)(((Yk + m) % (nCCE / L2)) * L2));
}

extern "C" int oai4g_pdcch_candidates(const oai4g_frame_parms_t *fp, uint8_t npd, uint8_t subframe, uint16_t crnti,
                                      int do_common, uint8_t L, uint16_t *cce, int cap)
{
  if (!pdcch_rx_geometry_ok("pdcch_candidates", fp, subframe, npd)) return -1;
  if (L > 3) { set_err("pdcch_candidates: illegal aggregation level L %u", L); return -1; }
  std::vector<uint16_t> v;
  pdcch_candidates_h(fp, npd, oai4g_get_mi(fp, subframe), subframe, crnti, do_common, L, v);
  for (int i = 0; i < cap && i < (int)v.size() && cce; i++) cce[i] = v[i];
  return (int)v.size();
}

static int pdcch_plan_ok(const char *who, uint8_t L, uint8_t sizeof_bits, uint8_t sizeof_bytes)
{
  if (L > 3) { set_err("%s: illegal aggregation level L %u", who, L); return 0; }
  if (sizeof_bits == 0 || sizeof_bits > 45 || sizeof_bytes == 0 || sizeof_bytes > 8) {
    set_err("%s: DCI_LENGTH %u (1..45), %u bytes (1..8)", who, sizeof_bits, sizeof_bytes);
    return 0;
  }
  return 1;
}

extern "C" int oai4g_dci_decoding_procedure0(const int8_t *e_rx, uint8_t npd, uint16_t crnti, uint8_t *nCCE, int do_common,
                                             uint8_t subframe, oai4g_dci_alloc_t *dci_alloc, const oai4g_frame_parms_t *fp,
                                             uint8_t mi, uint16_t si_rnti, uint16_t ra_rnti, uint8_t L, uint8_t format_si,
                                             uint8_t format_ra, uint8_t format_c, uint8_t sizeof_bits, uint8_t sizeof_bytes,
                                             uint8_t *dci_cnt, uint8_t *format0_found, uint8_t *format_c_found,
                                             uint32_t *CCEmap0, uint32_t *CCEmap1, uint32_t *CCEmap2)
{
  if (!pdcch_plan_ok("dci_decoding_procedure0", L, sizeof_bits, sizeof_bytes)) return -1;
  if (!pdcch_rx_geometry_ok("dci_decoding_procedure0", fp, subframe, npd)) return -1;
  if (!e_rx || !dci_alloc || !dci_cnt || !format0_found || !format_c_found || !CCEmap0 || !CCEmap1 || !CCEmap2) {
    set_err("dci_decoding_procedure0: null argument");
    return -1;
  }
  NEED_INIT(-1);
  std::vector<uint16_t> cce;
  pdcch_candidates_h(fp, npd, mi, subframe, crnti, do_common, L, cce);
  const uint32_t nc = (uint32_t)cce.size(), D = (uint32_t)sizeof_bits + 16;
  if (nc == 0) return 0;
  const size_t eb = (size_t)72 * oai4g_get_nCCE(npd, fp, mi);
  std::vector<cc_job_t> jobs(nc);
  for (uint32_t c = 0; c < nc; c++) {
    jobs[c] = cc_job_t{};
    jobs[c].e_off = 72u * cce[c];
    jobs[c].E = (uint16_t)(72u << L);
    jobs[c].D = (uint16_t)D;
    jobs[c].crc_bits = sizeof_bits;
  }
  uint16_t plan[3 * 61];
  cc_rx_plan_h(D, plan);
  uint8_t rec[16 * OAI4G_PDCCH_REC];
  stage_t sg("dci_decoding_procedure0");   /* room for the 16 candidates of rec and the largest plan, D = 45 + 16 */
  const int r_e = sg.add(eb), r_job = sg.add(sizeof(cc_job_t) * 16, 832);
  const int r_plan = sg.add(3 * 61 * 2, 146), r_rec = sg.add(sizeof(rec), 768);
  if (!sg.open()) return -1;
  HCK(sg.up(r_e, e_rx, eb), -1);
  HCK(sg.up(r_job, jobs.data(), nc * sizeof(cc_job_t)), -1);
  HCK(sg.up(r_plan, plan, (size_t)3 * D * 2), -1);
  cc_args_t a;
  memset(&a, 0, sizeof(a));
  a.e = sg.ptr<const int8_t>(r_e);
  a.jobs = sg.ptr<const cc_job_t>(r_job);
  a.n_jobs = nc;
  a.n_items = 1;
  a.plan = sg.ptr<const uint16_t>(r_plan);
  a.out = sg.ptr(r_rec);
  a.out_stride = OAI4G_PDCCH_REC;
  HCK(oai4g_launch_cc_decode(a, D, g_scr.s), -1);
  HCK(sg.down(rec, r_rec, (size_t)nc * OAI4G_PDCCH_REC), -1);
  HCK(sg.sync(), -1);
  pdcch_state_t st = {};
  st.map[0] = *CCEmap0;
  st.map[1] = *CCEmap1;
  st.map[2] = *CCEmap2;
  st.dci_cnt = *dci_cnt;
  st.format0_found = *format0_found;
  st.format_c_found = *format_c_found;
  st.nCCE = -1;
  const oai4g_pdcch_plan_t pl = {(uint8_t)do_common, L, sizeof_bits, sizeof_bytes, format_si, format_ra, format_c, 0};
  for (uint32_t c = 0; c < nc; c++) {
    const uint8_t *r = rec + (size_t)c * OAI4G_PDCCH_REC;
    oai4g_pdcch_resolve(st, pl, cce[c], r, r[OAI4G_PDCCH_REC - 4] | ((uint32_t)r[OAI4G_PDCCH_REC - 3] << 8), crnti, si_rnti,
                        ra_rnti, dci_alloc, 255);
  }
  *CCEmap0 = st.map[0];
  *CCEmap1 = st.map[1];
  *CCEmap2 = st.map[2];
  *dci_cnt = st.dci_cnt;
  *format0_found = st.format0_found;
  *format_c_found = st.format_c_found;
  if (st.nCCE >= 0 && nCCE) *nCCE = (uint8_t)st.nCCE;
  return 0;
}

struct oai4g_pdcch_rx_config {
  oai4g_frame_parms_t fp;
  uint8_t npd;
  uint16_t crnti, si_rnti, ra_rnti;
  std::vector<oai4g_pdcch_plan_t> plan;
  std::vector<pdcch_cand_t> cands[10];
  uint32_t n_jobs = 0, tab_stride = 0;
  dev_buf<uint8_t> dev;              /* tables, jobs, candidates, counts, plans, receive plans */
  size_t o_jobs = 0, o_cands = 0, o_ncand = 0, o_plans = 0, o_ccplan = 0;
  dev_buf<uint8_t> d_rec;            /* the records of the largest batch so far (pdcch_batch_clear) */
};

extern "C" void oai4g_pdcch_rx_config_destroy(oai4g_pdcch_rx_config_t *cfg)
{
  if (cfg) delete cfg;
}

extern "C" oai4g_pdcch_rx_config_t *oai4g_pdcch_rx_config_create(const oai4g_frame_parms_t *fp, uint8_t npd, uint16_t crnti,
                                                                 uint16_t si_rnti, uint16_t ra_rnti,
                                                                 const oai4g_pdcch_plan_t *plan, int n_plan)
{
  if (!pdcch_rx_geometry_ok("pdcch_rx_config_create", fp, 0, npd)) return nullptr;
  if (!plan || n_plan < 1 || n_plan > 64) { set_err("pdcch_rx_config_create: %d plan entries (1..64)", n_plan); return nullptr; }
  for (int i = 0; i < n_plan; i++)
    if (!pdcch_plan_ok("pdcch_rx_config_create", plan[i].L, plan[i].sizeof_bits, plan[i].sizeof_bytes)) return nullptr;
  NEED_INIT(nullptr);
  std::unique_ptr<oai4g_pdcch_rx_config_t> cfg(new oai4g_pdcch_rx_config_t);
  cfg->fp = *fp;
  cfg->npd = npd;
  cfg->crnti = crnti;
  cfg->si_rnti = si_rnti;
  cfg->ra_rnti = ra_rnti;
  cfg->plan.assign(plan, plan + n_plan);
  /* one receive plan per distinct D, in order of first use */
  std::vector<uint32_t> Ds;
  std::vector<uint16_t> ccplan;
  std::vector<uint32_t> ccoff(n_plan);
  for (int i = 0; i < n_plan; i++) {
    const uint32_t D = (uint32_t)plan[i].sizeof_bits + 16;
    size_t j = 0, off = 0;
    for (; j < Ds.size() && Ds[j] != D; j++) off += 3 * Ds[j];
    if (j == Ds.size()) {
      Ds.push_back(D);
      ccplan.resize(off + 3 * D);
      cc_rx_plan_h(D, ccplan.data() + off);
    }
    ccoff[i] = (uint32_t)off;
  }
  if (ccplan.size() > 0xFFFF) { set_err("pdcch_rx_config_create: too many distinct DCI sizes"); return nullptr; }
  std::vector<uint32_t> tabs[10];
  for (uint8_t sf = 0; sf < 10; sf++) {
    pdcch_soft_table_h(fp, sf, npd, tabs[sf]);
    if (tabs[sf].size() > cfg->tab_stride) cfg->tab_stride = (uint32_t)tabs[sf].size();
    const uint8_t mi = oai4g_get_mi(fp, sf);
    for (int i = 0; i < n_plan; i++) {
      std::vector<uint16_t> cce;
      pdcch_candidates_h(fp, npd, mi, sf, crnti, plan[i].do_common, plan[i].L, cce);
      for (size_t c = 0; c < cce.size(); c++) cfg->cands[sf].push_back(pdcch_cand_t{cce[c], (uint8_t)i, (uint8_t)(c == 0)});
    }
    if (cfg->cands[sf].size() > cfg->n_jobs) cfg->n_jobs = (uint32_t)cfg->cands[sf].size();
  }
  if (cfg->n_jobs == 0) cfg->n_jobs = 1;
  const uint32_t nj = cfg->n_jobs;
  cfg->o_jobs = up256((size_t)10 * cfg->tab_stride * 4);
  cfg->o_cands = cfg->o_jobs + up256((size_t)10 * nj * sizeof(cc_job_t));
  cfg->o_ncand = cfg->o_cands + up256((size_t)10 * nj * sizeof(pdcch_cand_t));
  cfg->o_plans = cfg->o_ncand + up256(10 * 4);
  cfg->o_ccplan = cfg->o_plans + up256((size_t)n_plan * sizeof(oai4g_pdcch_plan_t));
  const size_t total = cfg->o_ccplan + up256(ccplan.size() * 2);
  std::vector<uint8_t> h(total, 0);
  for (uint32_t sf = 0; sf < 10; sf++) {
    uint32_t *t = (uint32_t *)h.data() + (size_t)sf * cfg->tab_stride;
    for (uint32_t i = 0; i < cfg->tab_stride; i++) t[i] = i < tabs[sf].size() ? tabs[sf][i] : OAI4G_PDCCH_NONE;
    cc_job_t *jobs = (cc_job_t *)(h.data() + cfg->o_jobs) + (size_t)sf * nj;
    pdcch_cand_t *cd = (pdcch_cand_t *)(h.data() + cfg->o_cands) + (size_t)sf * nj;
    for (uint32_t c = 0; c < cfg->cands[sf].size(); c++) {
      const pdcch_cand_t &k = cfg->cands[sf][c];
      const oai4g_pdcch_plan_t &pl = plan[k.plan];
      if (72u * (k.cce + (1u << pl.L)) > tabs[sf].size()) { set_err("pdcch_rx_config_create: candidate outside the soft bits"); return nullptr; }
      jobs[c].e_off = 72u * k.cce;
      jobs[c].E = (uint16_t)(72u << pl.L);
      jobs[c].D = (uint16_t)(pl.sizeof_bits + 16);
      jobs[c].plan_off = (uint16_t)ccoff[k.plan];
      jobs[c].crc_bits = pl.sizeof_bits;
      cd[c] = k;
    }
    ((uint32_t *)(h.data() + cfg->o_ncand))[sf] = (uint32_t)cfg->cands[sf].size();   /* the other jobs have D = 0: no decode */
  }
  memcpy(h.data() + cfg->o_plans, plan, (size_t)n_plan * sizeof(oai4g_pdcch_plan_t));
  memcpy(h.data() + cfg->o_ccplan, ccplan.data(), ccplan.size() * 2);
  HCK(cfg->dev.upload(h), nullptr);
  return cfg.release();
}

extern "C" int oai4g_pdcch_rx_candidates(const oai4g_pdcch_rx_config_t *cfg, uint8_t subframe, uint16_t *cce,
                                         uint8_t *plan_entry, int cap)
{
  if (!cfg || subframe > 9) { set_err("pdcch_rx_candidates: bad arguments"); return -1; }
  const auto &v = cfg->cands[subframe];
  for (int i = 0; i < cap && i < (int)v.size(); i++) {
    if (cce) cce[i] = v[i].cce;
    if (plan_entry) plan_entry[i] = v[i].plan;
  }
  return (int)v.size();
}

/* the record buffer of a PDCCH batch, kept in `own`: grown when `need` bytes do not fit, then cleared together
 * with the results (unwritten fields and slots read as 0) */
static int pdcch_batch_clear(oai4g_pdcch_rx_config_t *own, size_t need, oai4g_pdcch_rx_result_t *d_out, int n_sf, hipStream_t s)
{
  if (need > own->d_rec.count()) {
    HCK(hipDeviceSynchronize(), -1);
    HCK(own->d_rec.reserve(need), -1);
  }
  HCK(hipMemsetAsync(own->d_rec.get(), 0, need, s), -1);
  HCK(hipMemsetAsync(d_out, 0, (size_t)n_sf * sizeof(oai4g_pdcch_rx_result_t), s), -1);
  return 0;
}

/* what the decode and the resolve stage of both batches take from a configuration: its tables, jobs, candidates
 * and plans, nj records per subframe, npd control symbols per compensated subframe */
static void pdcch_batch_args(const oai4g_pdcch_rx_config_t *c, uint32_t nj, uint32_t npd, const int32_t *d_comp, int n_sf,
                             int first_subframe, oai4g_pdcch_rx_result_t *d_out, cc_args_t &a, pdcch_resolve_args_t &r)
{
  a.jobs = (const cc_job_t *)(c->dev.get() + c->o_jobs);
  a.n_jobs = nj;
  a.n_items = (uint32_t)n_sf;
  a.plan = (const uint16_t *)(c->dev.get() + c->o_ccplan);
  a.out = c->d_rec.get();
  a.out_stride = OAI4G_PDCCH_REC;
  a.tab = (const uint32_t *)c->dev.get();
  a.tab_stride = c->tab_stride;
  a.comp = (const int16_t *)d_comp;
  a.comp_stride = (size_t)npd * c->fp.N_RB_DL * 12 * 2;
  a.first_row = (uint32_t)first_subframe;
  r.rec = c->d_rec.get();
  r.cands = (const pdcch_cand_t *)(c->dev.get() + c->o_cands);
  r.n_cand = (const uint32_t *)(c->dev.get() + c->o_ncand);
  r.plans = (const oai4g_pdcch_plan_t *)(c->dev.get() + c->o_plans);
  r.n_jobs = nj;
  r.n_sf = (uint32_t)n_sf;
  r.first_row = (uint32_t)first_subframe;
  r.crnti = c->crnti, r.si_rnti = c->si_rnti, r.ra_rnti = c->ra_rnti;
  r.out = d_out;
}

extern "C" int oai4g_pdcch_rx_batch(oai4g_pdcch_rx_config_t *cfg, const int32_t *d_comp, int n_sf, int first_subframe,
                                    oai4g_pdcch_rx_result_t *d_out, void *stream)
{
  if (!cfg || n_sf < 0 || first_subframe < 0 || first_subframe > 9 || (n_sf > 0 && (!d_comp || !d_out))) {
    set_err("pdcch_rx_batch: bad arguments");
    return -1;
  }
  NEED_INIT(-1);
  if (n_sf == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (pdcch_batch_clear(cfg, (size_t)n_sf * cfg->n_jobs * OAI4G_PDCCH_REC, d_out, n_sf, s) != 0) return -1;
  cc_args_t a;
  pdcch_resolve_args_t r;
  memset(&a, 0, sizeof(a));
  memset(&r, 0, sizeof(r));
  pdcch_batch_args(cfg, cfg->n_jobs, cfg->npd, d_comp, n_sf, first_subframe, d_out, a, r);
  HCK(oai4g_launch_cc_decode(a, 61, s), -1);
  HCK(oai4g_launch_pdcch_resolve(r, s), -1);
  return 0;
}

/* The search over subframes whose count was detected on the device: one launch decodes, per subframe, the
 * candidates of its own count's configuration; the count stays in d_cfi. */
extern "C" int oai4g_pdcch_rx_batch_detected(oai4g_pdcch_rx_config_t *const cfg[3], const int32_t *d_comp, const uint8_t *d_cfi,
                                             int n_sf, int first_subframe, int subframe_step, oai4g_pdcch_rx_result_t *d_out,
                                             void *stream)
{
  if (!cfg || !cfg[0] || !cfg[1] || !cfg[2] || n_sf < 0 || first_subframe < 0 || first_subframe > 9 || subframe_step < 0 ||
      subframe_step > 9 || (n_sf > 0 && (!d_comp || !d_cfi || !d_out))) {
    set_err("pdcch_rx_batch_detected: bad arguments");
    return -1;
  }
  for (int i = 0; i < 3; i++) {
    const oai4g_pdcch_rx_config_t *c = cfg[i], *c0 = cfg[0];
    if (c->npd != i + 1 || memcmp(&c->fp, &c0->fp, sizeof(c->fp)) != 0 || c->crnti != c0->crnti || c->si_rnti != c0->si_rnti ||
        c->ra_rnti != c0->ra_rnti || c->plan.size() != c0->plan.size() ||
        memcmp(c->plan.data(), c0->plan.data(), c->plan.size() * sizeof(oai4g_pdcch_plan_t)) != 0) {
      set_err("pdcch_rx_batch_detected: configuration %d must be the one of %d symbols for the same frame, RNTIs and plan", i, i + 1);
      return -1;
    }
  }
  NEED_INIT(-1);
  if (n_sf == 0) return 0;
  uint32_t nj = 0;
  for (int i = 0; i < 3; i++) nj = std::max(nj, cfg[i]->n_jobs);
  oai4g_pdcch_rx_config_t *own = cfg[2];   /* holds the records; its tables are the base arguments' */
  hipStream_t s = (hipStream_t)stream;
  if (pdcch_batch_clear(own, (size_t)n_sf * nj * OAI4G_PDCCH_REC, d_out, n_sf, s) != 0) return -1;
  cc_det_args_t a;
  pdcch_resolve_det_args_t r;
  memset(&a, 0, sizeof(a));
  memset(&r, 0, sizeof(r));
  pdcch_batch_args(own, nj, 3, d_comp, n_sf, first_subframe, d_out, a, r);
  for (int i = 0; i < 3; i++) {
    const oai4g_pdcch_rx_config_t *c = cfg[i];
    pdcch_det_set_t &t = a.set[i];
    t.jobs = (const cc_job_t *)(c->dev.get() + c->o_jobs);
    t.tab = (const uint32_t *)c->dev.get();
    t.cands = (const pdcch_cand_t *)(c->dev.get() + c->o_cands);
    t.n_cand = (const uint32_t *)(c->dev.get() + c->o_ncand);
    t.plan = (const uint16_t *)(c->dev.get() + c->o_ccplan);
    t.n_jobs = c->n_jobs;
    t.tab_stride = c->tab_stride;
    r.set[i] = t;
  }
  a.cfi = r.cfi = d_cfi;
  a.sf_step = r.sf_step = (uint32_t)subframe_step;
  HCK(oai4g_launch_cc_decode_detected(a, s), -1);
  HCK(oai4g_launch_pdcch_resolve_detected(r, s), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * PDCCH / PCFICH receive front end: rx_pdcch up to the compensated symbols (dci.c:1689-1830) and
 * rx_pcfich (pcfich.c:231), k_pdcch_front.
 * ---------------------------------------------------------------------------------------- */
static int pdcch_front_ok(const char *who, const oai4g_frame_parms_t *fp, int nb_rx, uint8_t mimo_mode)
{
  if (!fp) { set_err("%s: null frame parameters", who); return 0; }
  if (fp->nb_antennas_tx_eNB == 4) { set_err("%s: 4 TX ports are not defined by the reference's demapping (dci.c:420)", who); return 0; }
  if (fp->Ncp != 0) { set_err("%s: only the normal cyclic prefix is supported", who); return 0; }
  if (nb_rx < 1 || nb_rx > 2) { set_err("%s: %d receive antennas (1 or 2)", who, nb_rx); return 0; }
  if (fp->nb_antennas_tx_eNB < 1 || fp->nb_antennas_tx_eNB > 2) { set_err("%s: %u TX ports (1 or 2)", who, fp->nb_antennas_tx_eNB); return 0; }
  if (mimo_mode != OAI4G_SISO && mimo_mode != OAI4G_ALAMOUTI) { set_err("%s: mimo_mode %u (SISO or ALAMOUTI)", who, mimo_mode); return 0; }
  if (mimo_mode == OAI4G_ALAMOUTI && fp->nb_antennas_tx_eNB != 2) { set_err("%s: ALAMOUTI combining needs 2 TX ports", who); return 0; }
  const uint32_t N = fp->ofdm_symbol_size, NRE = 12u * fp->N_RB_DL;
  if (fp->N_RB_DL == 0 || 5u + NRE > N || fp->first_carrier_offset + NRE / 2 > N || 13u + NRE / 2 > N) {
    set_err("%s: N_RB_DL %u does not fit the symbol size %u", who, fp->N_RB_DL, N);
    return 0;
  }
  return 1;
}

/* the first Gold word of pcfich_unscrambling (pcfich.c:122) */
static uint32_t pcfich_gold_h(const oai4g_frame_parms_t *fp, uint32_t subframe)
{
  uint32_t w;
  gold_seq_h(((((2u * fp->Nid_cell) + 1u) * (1u + subframe)) << 9) + fp->Nid_cell, &w, 1);
  return w;
}

/* the four PCFICH REGs as word offsets into the packed symbol 0 (four words a REG) */
static void pcfich_words_h(const oai4g_frame_parms_t *fp, uint32_t w[4])
{
  uint16_t reg[4];
  uint8_t fi;
  pcfich_regs(fp, reg, &fi);
  for (int q = 0; q < 4; q++) w[q] = (uint32_t)reg[q] * 4u;
}

static void pdcch_front_fill(pdcch_front_args_t &a, const oai4g_frame_parms_t *fp, int nb_rx, uint8_t mimo_mode,
                             uint32_t high_speed_flag, uint32_t first_sf, uint32_t sf_step)
{
  memset(&a, 0, sizeof(a));
  a.N = fp->ofdm_symbol_size;
  a.N_RB = fp->N_RB_DL;
  a.fco = fp->first_carrier_offset;
  a.nushift3 = fp->nushift % 3u;
  a.nb_tx = fp->nb_antennas_tx_eNB;
  a.nb_rx = (uint32_t)nb_rx;
  a.alamouti = mimo_mode == OAI4G_ALAMOUTI;
  a.high_speed = high_speed_flag == 1;
  a.first_sf = first_sf;
  a.sf_step = sf_step;
  pcfich_words_h(fp, a.pcf_word);
  for (uint32_t sf = 0; sf < 10; sf++) a.pcf_gold[sf] = pcfich_gold_h(fp, sf);
}

extern "C" int oai4g_rx_pdcch_front(int32_t *const *rxdataF, int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *fp,
                                    uint8_t nb_antennas_rx, uint8_t subframe, uint8_t mimo_mode, uint32_t high_speed_flag,
                                    int32_t *rxdataF_comp, uint8_t *log2_maxh, uint8_t *num_pdcch_symbols, int32_t *diag_planes)
{
  if (!pdcch_front_ok("rx_pdcch_front", fp, nb_antennas_rx, mimo_mode)) return -1;
  if (subframe > 9 || !rxdataF || !dl_ch_estimates || !rxdataF_comp) { set_err("rx_pdcch_front: bad arguments"); return -1; }
  const int nb_tx = fp->nb_antennas_tx_eNB;
  for (int a = 0; a < nb_antennas_rx; a++)
    for (int p = 0; p < nb_tx; p++)
      if (!rxdataF[a] || !dl_ch_estimates[(p << 1) + a]) { set_err("rx_pdcch_front: null plane"); return -1; }
  NEED_INIT(-1);
  const size_t rows = (size_t)3 * fp->ofdm_symbol_size * 4, out_b = (size_t)36 * fp->N_RB_DL * 4;
  const size_t row_s = up256(rows);           /* an antenna's / a plane's three rows, a stride apart */
  stage_t st("rx_pdcch_front");
  const int r_rx = st.add(2 * row_s), r_est = st.add(4 * row_s), r_comp = st.add(out_b);
  const int r_pl = st.add(4 * up256(out_b)), r_b = st.add(2, 254);   /* four diagnostic planes, out_b apart; cfi, log2_maxh */
  if (!st.open()) return -1;
  pdcch_front_args_t a;
  pdcch_front_fill(a, fp, nb_antennas_rx, mimo_mode, high_speed_flag, subframe, 0);
  a.n_sf = 1;
  a.rxF = st.ptr<const int32_t>(r_rx);
  a.rx_ant_stride = row_s / 4;
  for (int rx = 0; rx < nb_antennas_rx; rx++) {
    HCK(st.up(r_rx, rxdataF[rx], rows, rx * row_s), -1);
    for (int p = 0; p < nb_tx; p++) {
      const int pl = (p << 1) + rx;
      HCK(st.up(r_est, dl_ch_estimates[pl], rows, pl * row_s), -1);
      a.est[pl] = st.ptr<const int32_t>(r_est, pl * row_s);
    }
  }
  a.comp = st.ptr<int32_t>(r_comp);
  a.planes = diag_planes ? st.ptr<int32_t>(r_pl) : nullptr;
  a.cfi = st.ptr(r_b);
  a.log2_maxh = st.ptr(r_b, 1);
  HCK(oai4g_launch_pdcch_front(a, g_scr.s), -1);
  uint8_t two[2] = {0, 0};
  HCK(st.down(rxdataF_comp, r_comp, out_b), -1);
  if (diag_planes) HCK(st.down(diag_planes, r_pl, 4 * out_b), -1);
  HCK(st.down(two, r_b, 2), -1);
  HCK(st.sync(), -1);
  if (num_pdcch_symbols) *num_pdcch_symbols = two[0];
  if (log2_maxh) *log2_maxh = two[1];
  return 0;
}

extern "C" int oai4g_rx_pcfich(const oai4g_frame_parms_t *fp, uint8_t subframe, const int32_t *rxdataF_comp, uint8_t mimo_mode)
{
  if (!pdcch_front_ok("rx_pcfich", fp, 1, fp && fp->nb_antennas_tx_eNB == 2 ? mimo_mode : (uint8_t)OAI4G_SISO)) return -1;
  if (subframe > 9 || !rxdataF_comp) { set_err("rx_pcfich: bad arguments"); return -1; }
  NEED_INIT(-1);
  const size_t cb = (size_t)8 * fp->N_RB_DL * 4;              /* the packed symbol 0 */
  stage_t st("rx_pcfich");
  const int r_comp = st.add(cb), r_n = st.add(1, 511);
  if (!st.open()) return -1;
  uint8_t n = 0;
  uint32_t w[4];
  pcfich_words_h(fp, w);
  HCK(st.up(r_comp, rxdataF_comp, cb), -1);
  HCK(oai4g_launch_rx_pcfich(st.ptr<const int32_t>(r_comp), w, pcfich_gold_h(fp, subframe), st.ptr(r_n), g_scr.s), -1);
  HCK(st.down(&n, r_n, 1), -1);
  HCK(st.sync(), -1);
  return n;
}

extern "C" int oai4g_rx_pdcch(int32_t *const *rxdataF, int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *fp,
                              uint8_t nb_antennas_rx, uint8_t subframe, uint8_t mimo_mode, uint32_t high_speed_flag,
                              int8_t *e_rx, uint8_t *num_pdcch_symbols)
{
  if (!pdcch_rx_geometry_ok("rx_pdcch", fp, subframe, 3)) return -1;
  if (!e_rx) { set_err("rx_pdcch: null e_rx"); return -1; }
  std::vector<int32_t> comp((size_t)36 * fp->N_RB_DL);
  uint8_t n = 0;
  if (oai4g_rx_pdcch_front(rxdataF, dl_ch_estimates, fp, nb_antennas_rx, subframe, mimo_mode, high_speed_flag, comp.data(),
                           nullptr, &n, nullptr) != 0)
    return -1;
  if (num_pdcch_symbols) *num_pdcch_symbols = n;
  return oai4g_pdcch_soft_bits(comp.data(), fp, subframe, n, e_rx);
}

struct oai4g_pdcch_front_config {
  oai4g_frame_parms_t fp;
  pdcch_front_args_t a;
};

extern "C" oai4g_pdcch_front_config_t *oai4g_pdcch_front_config_create(const oai4g_frame_parms_t *fp, uint8_t nb_antennas_rx,
                                                                       uint8_t mimo_mode, uint32_t high_speed_flag,
                                                                       uint8_t first_subframe, uint8_t subframe_step)
{
  if (!pdcch_front_ok("pdcch_front_config_create", fp, nb_antennas_rx, mimo_mode)) return nullptr;
  if (first_subframe > 9 || subframe_step > 9) { set_err("pdcch_front_config_create: subframe %u / step %u", first_subframe, subframe_step); return nullptr; }
  oai4g_pdcch_front_config_t *cfg = new oai4g_pdcch_front_config_t;
  cfg->fp = *fp;
  pdcch_front_fill(cfg->a, fp, nb_antennas_rx, mimo_mode, high_speed_flag, first_subframe, subframe_step);
  return cfg;
}

extern "C" void oai4g_pdcch_front_config_destroy(oai4g_pdcch_front_config_t *cfg) { delete cfg; }

extern "C" int oai4g_pdcch_front_batch(const oai4g_pdcch_front_config_t *cfg, int n_sf, const int32_t *d_rxdataF,
                                       const int32_t *const d_est[4], int32_t *d_comp, uint8_t *d_cfi, uint8_t *d_log2_maxh,
                                       void *stream)
{
  if (!cfg || n_sf < 0 || (n_sf > 0 && (!d_rxdataF || !d_est || !d_comp || !d_cfi || !d_log2_maxh))) {
    set_err("pdcch_front_batch: bad arguments");
    return -1;
  }
  pdcch_front_args_t a = cfg->a;
  for (uint32_t p = 0; p < a.nb_tx; p++)
    for (uint32_t rx = 0; rx < a.nb_rx; rx++) {
      if (n_sf > 0 && !d_est[(p << 1) + rx]) { set_err("pdcch_front_batch: null estimate plane %u", (p << 1) + rx); return -1; }
      a.est[(p << 1) + rx] = n_sf > 0 ? d_est[(p << 1) + rx] : nullptr;
    }
  NEED_INIT(-1);
  if (n_sf == 0) return 0;
  const size_t grid = (size_t)cfg->fp.symbols_per_tti * cfg->fp.ofdm_symbol_size;
  a.n_sf = (uint32_t)n_sf;
  a.rxF = d_rxdataF;
  a.rx_ant_stride = grid;
  a.rx_sf_stride = grid * a.nb_rx;
  a.est_sf_stride = grid;
  a.comp = d_comp;
  a.cfi = d_cfi;
  a.log2_maxh = d_log2_maxh;
  HCK(oai4g_launch_pdcch_front(a, (hipStream_t)stream), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * PBCH receive front end: rx_pbch up to the quantised soft bits (pbch.c:876-973), k_pbch_front, and
 * pbch_detection's hypothesis search (initial_sync.c:135-161) behind it.
 * ---------------------------------------------------------------------------------------- */
static int pbch_front_ok(const char *who, const oai4g_frame_parms_t *fp, int nb_rx, int nb_ports, uint8_t mimo_mode)
{
  if (!fp) { set_err("%s: null frame parameters", who); return 0; }
  if (fp->Ncp != 0) { set_err("%s: only the normal cyclic prefix is supported (the reference's quantise lengths overrun pbch_E with the extended one)", who); return 0; }
  if (nb_ports == 4) { set_err("%s: 4 estimated TX ports are not supported", who); return 0; }
  if (nb_ports < 1 || nb_ports > 2) { set_err("%s: %d estimated TX ports (1 or 2)", who, nb_ports); return 0; }
  if (nb_rx < 1 || nb_rx > 2) { set_err("%s: %d receive antennas (1 or 2)", who, nb_rx); return 0; }
  if (mimo_mode != OAI4G_SISO && mimo_mode != OAI4G_ALAMOUTI) { set_err("%s: mimo_mode %u (SISO or ALAMOUTI)", who, mimo_mode); return 0; }
  const uint32_t N = fp->ofdm_symbol_size;
  if (fp->N_RB_DL < 6 || 6u * fp->N_RB_DL + 41u > N || fp->symbols_per_tti != 14) {   /* estimate words 6 N_RB - 31 .. 6 N_RB + 40 */
    set_err("%s: N_RB_DL %u does not fit the symbol size %u", who, fp->N_RB_DL, N);
    return 0;
  }
  return 1;
}

static void pbch_front_fill(pbch_front_args_t &a, const oai4g_frame_parms_t *fp, int nb_rx, int nb_ports, uint8_t mimo_mode,
                            uint32_t high_speed_flag)
{
  memset(&a, 0, sizeof(a));
  a.N = fp->ofdm_symbol_size;
  a.N_RB = fp->N_RB_DL;
  a.nushift3 = fp->nushift % 3u;
  a.nb_tx = (uint32_t)nb_ports;
  a.nb_rx = (uint32_t)nb_rx;
  a.alamouti = mimo_mode == OAI4G_ALAMOUTI;
  a.high_speed = high_speed_flag == 1;
}

extern "C" int oai4g_rx_pbch_front(int32_t *const *rxdataF, int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *fp,
                                   uint8_t nb_antennas_rx, uint8_t nb_ports, uint8_t mimo_mode, uint32_t high_speed_flag,
                                   int32_t *rxdataF_comp, uint8_t log2_maxh[4], int8_t *llr, int32_t *diag_planes)
{
  if (!pbch_front_ok("rx_pbch_front", fp, nb_antennas_rx, nb_ports, mimo_mode)) return -1;
  if (!rxdataF || !dl_ch_estimates) { set_err("rx_pbch_front: bad arguments"); return -1; }
  for (int a = 0; a < nb_antennas_rx; a++)
    for (int p = 0; p < nb_ports; p++)
      if (!rxdataF[a] || !dl_ch_estimates[(p << 1) + a]) { set_err("rx_pbch_front: null plane"); return -1; }
  NEED_INIT(-1);
  const size_t N = fp->ofdm_symbol_size, grid = 14 * N * 4, grid_s = up256(grid);
  const size_t cb = OAI4G_PBCH_WORDS * 4, lb = 2 * OAI4G_PBCH_SOFT;
  stage_t st("rx_pbch_front");
  const int r_rx = st.add(2 * grid_s), r_est = st.add(4 * grid_s), r_comp = st.add(cb);
  const int r_pl = st.add(4 * cb), r_llr = st.add(lb), r_l2 = st.add(4);
  if (!st.open()) return -1;
  pbch_front_args_t a;
  pbch_front_fill(a, fp, nb_antennas_rx, nb_ports, mimo_mode, high_speed_flag);
  a.n_sf = 1;
  a.rxF = st.ptr<const int32_t>(r_rx);
  a.rx_ant_stride = grid_s / 4;
  const size_t e0 = high_speed_flag == 1 ? 7 * N * 4 : 0, eb = high_speed_flag == 1 ? 4 * N * 4 : N * 4;   /* the rows read */
  for (int rx = 0; rx < nb_antennas_rx; rx++) {
    HCK(st.up(r_rx, (const uint8_t *)rxdataF[rx] + 7 * N * 4, 4 * N * 4, rx * grid_s + 7 * N * 4), -1);
    for (int p = 0; p < nb_ports; p++) {
      const int pl = (p << 1) + rx;
      HCK(st.up(r_est, (const uint8_t *)dl_ch_estimates[pl] + e0, eb, pl * grid_s + e0), -1);
      a.est[pl] = st.ptr<const int32_t>(r_est, pl * grid_s);
    }
  }
  a.comp = st.ptr<int32_t>(r_comp);
  a.planes = diag_planes ? st.ptr<int32_t>(r_pl) : nullptr;
  a.llr = st.ptr<int8_t>(r_llr);
  a.log2_maxh = st.ptr(r_l2);
  HCK(oai4g_launch_pbch_front(a, g_scr.s), -1);
  if (rxdataF_comp) HCK(st.down(rxdataF_comp, r_comp, cb), -1);
  if (diag_planes) HCK(st.down(diag_planes, r_pl, 4 * cb), -1);
  if (llr) HCK(st.down(llr, r_llr, OAI4G_PBCH_SOFT, a.alamouti ? OAI4G_PBCH_SOFT : 0), -1);
  if (log2_maxh) HCK(st.down(log2_maxh, r_l2, 4), -1);
  HCK(st.sync(), -1);
  return 0;
}

extern "C" int oai4g_rx_pbch(int32_t *const *rxdataF, int32_t *const *dl_ch_estimates, const oai4g_frame_parms_t *fp,
                             uint8_t nb_antennas_rx, uint8_t nb_ports, uint8_t mimo_mode, uint32_t high_speed_flag,
                             uint8_t frame_mod4, uint8_t decoded_output[3])
{
  if (frame_mod4 > 3 || !decoded_output) { set_err("rx_pbch: frame_mod4 %u or a null argument", frame_mod4); return -1; }
  int8_t llr[1920];
  memset(llr, 0, sizeof(llr));                                         /* pbch.c:908 */
  if (oai4g_rx_pbch_front(rxdataF, dl_ch_estimates, fp, nb_antennas_rx, nb_ports, mimo_mode, high_speed_flag, nullptr, nullptr,
                          llr + frame_mod4 * OAI4G_PBCH_SOFT, nullptr) != 0)
    return -1;
  return oai4g_pbch_decode(llr, fp, frame_mod4, decoded_output);
}

struct oai4g_pbch_front_config {
  oai4g_frame_parms_t fp;
  pbch_front_args_t a;
  dev_buf<uint8_t> consts;   /* the detection's eight jobs | the receive plan at 256 | the cell's 60 Gold words at 512 */
  dev_buf<uint8_t> rec;      /* [n][8][4] decode records of the last detection */
};

extern "C" oai4g_pbch_front_config_t *oai4g_pbch_front_config_create(const oai4g_frame_parms_t *fp, uint8_t nb_antennas_rx,
                                                                     uint8_t nb_ports, uint32_t high_speed_flag)
{
  if (!pbch_front_ok("pbch_front_config_create", fp, nb_antennas_rx, nb_ports, OAI4G_SISO)) return nullptr;
  NEED_INIT(nullptr);
  std::unique_ptr<oai4g_pbch_front_config_t> cfg(new oai4g_pbch_front_config_t);
  cfg->fp = *fp;
  pbch_front_fill(cfg->a, fp, nb_antennas_rx, nb_ports, OAI4G_SISO, high_speed_flag);
  std::vector<uint8_t> h(1024, 0);
  for (uint32_t j = 0; j < 8; j++) {
    cc_job_t job = {};
    job.e_off = (j & 1u) * OAI4G_PBCH_SOFT;
    job.E = OAI4G_PBCH_SOFT;
    job.D = 40;
    job.crc_bits = 24;
    memcpy(h.data() + j * sizeof(job), &job, sizeof(job));
  }
  static_assert(8 * sizeof(cc_job_t) <= 256, "the jobs end before the plan");
  cc_rx_plan_h(40, (uint16_t *)(h.data() + 256));
  pbch_gold_h(fp->Nid_cell, 1920, (uint32_t *)(h.data() + 512));
  HCK(cfg->consts.upload(h), nullptr);
  return cfg.release();
}

extern "C" void oai4g_pbch_front_config_destroy(oai4g_pbch_front_config_t *cfg) { delete cfg; }

extern "C" int oai4g_pbch_front_batch(const oai4g_pbch_front_config_t *cfg, int n, const int32_t *d_rxdataF,
                                      const int32_t *const d_est[4], int8_t *d_llr, uint8_t *d_log2_maxh, void *stream)
{
  if (!cfg || n < 0 || (n > 0 && (!d_rxdataF || !d_est || !d_llr || !d_log2_maxh))) {
    set_err("pbch_front_batch: bad arguments");
    return -1;
  }
  pbch_front_args_t a = cfg->a;
  for (uint32_t p = 0; p < a.nb_tx; p++)
    for (uint32_t rx = 0; rx < a.nb_rx; rx++) {
      if (n > 0 && !d_est[(p << 1) + rx]) { set_err("pbch_front_batch: null estimate plane %u", (p << 1) + rx); return -1; }
      a.est[(p << 1) + rx] = n > 0 ? d_est[(p << 1) + rx] : nullptr;
    }
  NEED_INIT(-1);
  if (n == 0) return 0;
  const size_t grid = (size_t)cfg->fp.symbols_per_tti * cfg->fp.ofdm_symbol_size;
  a.n_sf = (uint32_t)n;
  a.rxF = d_rxdataF;
  a.rx_ant_stride = grid;
  a.rx_sf_stride = grid * a.nb_rx;
  a.est_sf_stride = grid;
  a.llr = d_llr;
  a.log2_maxh = d_log2_maxh;
  HCK(oai4g_launch_pbch_front(a, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_pbch_detect_batch(oai4g_pbch_front_config_t *cfg, int n, const int8_t *d_llr, oai4g_pbch_detect_t *d_out,
                                       void *stream)
{
  if (!cfg || n < 0 || (n > 0 && (!d_llr || !d_out))) { set_err("pbch_detect_batch: bad arguments"); return -1; }
  NEED_INIT(-1);
  if (n == 0) return 0;
  if (cfg->rec.count() < (size_t)n * 32) {
    HCK(hipDeviceSynchronize(), -1);                                   /* an earlier detection may still write the old records */
    HCK(cfg->rec.reserve((size_t)n * 32), -1);
  }
  cc_hyp_args_t a;
  memset(&a, 0, sizeof(a));
  a.e = d_llr;
  a.e_stride = 2 * OAI4G_PBCH_SOFT;
  a.jobs = (const cc_job_t *)cfg->consts.get();
  a.n_jobs = 8;
  a.n_items = (uint32_t)n;
  a.plan = (const uint16_t *)(cfg->consts.get() + 256);
  a.gold = (const uint32_t *)(cfg->consts.get() + 512);
  a.out = cfg->rec.get();
  a.out_stride = 4;
  a.pbch_out = 1;
  HCK(oai4g_launch_cc_decode_hyp(a, (hipStream_t)stream), -1);
  HCK(oai4g_launch_pbch_resolve(cfg->rec.get(), (uint32_t)n, d_out, (hipStream_t)stream), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * PHICH reception: rx_phich's correlation (phich.c:1112-1346), k_phich_rx.
 * ---------------------------------------------------------------------------------------- */
/* the table entries of one subframe index: [ng][8].  Returns the number of groups, or -1 */
static int phich_rx_table(const char *who, const oai4g_frame_parms_t *fp, uint32_t subframe, phich_rx_ent_t *ent)
{
  if (!fp) { set_err("%s: null frame parameters", who); return -1; }
  if (fp->Ncp != 0 || fp->phich_duration != 0 || fp->nushift >= 3) {   /* as oai4g_generate_phich */
    set_err("%s: only normal CP, normal duration and nushift < 3 are defined", who);
    return -1;
  }
  if (subframe > 9 || fp->N_RB_DL < 6 || fp->N_RB_DL > 110) { set_err("%s: subframe %u / N_RB_DL %u", who, subframe, fp->N_RB_DL); return -1; }
  uint16_t reg[56][3];
  const int ng = oai4g_generate_phich_reg_mapping(fp, reg);
  if (ng <= 0 || ng > 56) { set_err("%s: no PHICH groups", who); return -1; }
  uint32_t s;
  gold_seq_h(((((uint32_t)subframe + 1u) * (fp->Nid_cell + 1u)) << 9) + fp->Nid_cell, &s, 1);
  static const uint8_t w_neg[4] = {0x0, 0xA, 0xC, 0x6};                 /* bit j: the orthogonal sequence's element j is -1 */
  for (int g = 0; g < ng; g++)
    for (uint32_t q = 0; q < 8; q++) {
      phich_rx_ent_t &e = ent[g * 8 + q];
      memset(&e, 0, sizeof(e));
      for (uint32_t i = 0; i < 12; i++) {
        const uint32_t cs_neg = (s >> i) & 1u, neg = cs_neg ^ ((w_neg[q & 3u] >> (i & 3u)) & 1u);
        e.neg |= (q < 4 ? neg : neg ^ 1u) << (2 * i);                   /* sequences 4..7: -cs on re */
        e.neg |= neg << (2 * i + 1);
      }
      for (int k = 0; k < 3; k++) {
        if ((uint32_t)reg[g][k] * 4u + 4u > 8u * fp->N_RB_DL) { set_err("%s: PHICH REG %u outside symbol 0", who, reg[g][k]); return -1; }
        e.word[k] = (uint16_t)(reg[g][k] * 4u);
      }
    }
  return ng;
}

extern "C" int oai4g_rx_phich(const oai4g_frame_parms_t *fp, uint8_t subframe, const int32_t *rxdataF_comp,
                              uint8_t ngroup_PHICH, uint8_t nseq_PHICH, int16_t *HI16)
{
  std::vector<phich_rx_ent_t> ent(56 * 8);
  const int ng = phich_rx_table("rx_phich", fp, subframe, ent.data());
  if (ng < 0) return -1;
  if (ngroup_PHICH >= ng || nseq_PHICH > 7 || !rxdataF_comp) { set_err("rx_phich: group %u / seq %u or a null plane", ngroup_PHICH, nseq_PHICH); return -1; }
  NEED_INIT(-1);
  const size_t cb = (size_t)8 * fp->N_RB_DL * 4;                       /* the packed symbol 0 */
  stage_t st("rx_phich");
  const int r_comp = st.add(cb), r_tab = st.add((size_t)ng * 8 * sizeof(phich_rx_ent_t));
  const int r_it = st.add(sizeof(oai4g_phich_rx_item_t)), r_out = st.add(sizeof(oai4g_phich_rx_out_t));
  if (!st.open()) return -1;
  oai4g_phich_rx_item_t it = {};
  it.ngroup = ngroup_PHICH;
  it.nseq = nseq_PHICH;
  HCK(st.up(r_comp, rxdataF_comp, cb), -1);
  HCK(st.up(r_tab, ent.data(), (size_t)ng * 8 * sizeof(phich_rx_ent_t)), -1);
  HCK(st.up(r_it, &it, sizeof(it)), -1);
  phich_rx_args_t a;
  memset(&a, 0, sizeof(a));
  a.comp = st.ptr<const int32_t>(r_comp);
  a.tab = st.ptr<const phich_rx_ent_t>(r_tab);                          /* the one row of this subframe index: slot 0 of a batch from 0 */
  a.ngroup = (uint32_t)ng;
  a.n_sf = 1;
  a.items = st.ptr<const oai4g_phich_rx_item_t>(r_it);
  a.n_items = 1;
  a.out = st.ptr<oai4g_phich_rx_out_t>(r_out);
  HCK(oai4g_launch_phich_rx(a, g_scr.s), -1);
  oai4g_phich_rx_out_t o = {};
  HCK(st.down(&o, r_out, sizeof(o)), -1);
  HCK(st.sync(), -1);
  if (o.nack > 1) { set_err("rx_phich: the item was refused on the device"); return -1; }
  if (HI16) *HI16 = o.HI16;
  return o.nack;
}

struct oai4g_phich_rx_config {
  oai4g_frame_parms_t fp;
  uint32_t ngroup, first_sf, sf_step;
  dev_buf<phich_rx_ent_t> tab;   /* [10][ngroup][8] */
};

extern "C" oai4g_phich_rx_config_t *oai4g_phich_rx_config_create(const oai4g_frame_parms_t *fp, uint8_t first_subframe,
                                                                 uint8_t subframe_step)
{
  if (first_subframe > 9 || subframe_step > 9) { set_err("phich_rx_config_create: subframe %u / step %u", first_subframe, subframe_step); return nullptr; }
  std::vector<phich_rx_ent_t> one(56 * 8), all;
  int ng = 0;
  for (uint32_t sf = 0; sf < 10; sf++) {
    ng = phich_rx_table("phich_rx_config_create", fp, sf, one.data());
    if (ng < 0) return nullptr;
    all.insert(all.end(), one.begin(), one.begin() + ng * 8);
  }
  NEED_INIT(nullptr);
  std::unique_ptr<oai4g_phich_rx_config_t> cfg(new oai4g_phich_rx_config_t);
  cfg->fp = *fp;
  cfg->ngroup = (uint32_t)ng;
  cfg->first_sf = first_subframe;
  cfg->sf_step = subframe_step;
  HCK(cfg->tab.upload(all), nullptr);
  return cfg.release();
}

extern "C" void oai4g_phich_rx_config_destroy(oai4g_phich_rx_config_t *cfg) { delete cfg; }

extern "C" int oai4g_phich_rx_batch(const oai4g_phich_rx_config_t *cfg, const int32_t *d_comp, int n_sf,
                                    const oai4g_phich_rx_item_t *d_items, int n_items, oai4g_phich_rx_out_t *d_out, void *stream)
{
  if (!cfg || n_sf < 0 || n_items < 0 || (n_items > 0 && (!d_comp || !d_items || !d_out))) {
    set_err("phich_rx_batch: bad arguments");
    return -1;
  }
  NEED_INIT(-1);
  phich_rx_args_t a;
  memset(&a, 0, sizeof(a));
  a.comp = d_comp;
  a.comp_stride = (size_t)36 * cfg->fp.N_RB_DL;
  a.tab = cfg->tab.get();
  a.ngroup = cfg->ngroup;
  a.n_sf = (uint32_t)n_sf;
  a.first_sf = cfg->first_sf;
  a.sf_step = cfg->sf_step;
  a.items = d_items;
  a.n_items = (uint32_t)n_items;
  a.out = d_out;
  HCK(oai4g_launch_phich_rx(a, (hipStream_t)stream), -1);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * UE initial cell search: lte_sync_time (PHY/LTE_ESTIMATION/lte_sync_time.c), k_sync_time.
 * ---------------------------------------------------------------------------------------- */
/* The fixed-point inverse DFT of lte_dfts.c on the host, for the three replicas only (they are derived
 * once per configuration and pinned without a device): the arithmetic of oai4g_dft_prims.h word for word. */
namespace {
struct hc16 {
  int16_t r, i;
};
inline int16_t h_sat16(int32_t v) { return (int16_t)(v > 32767 ? 32767 : (v < -32768 ? -32768 : v)); }
inline int16_t h_wrap16(int32_t v) { return (int16_t)(uint16_t)(uint32_t)v; }
inline hc16 h_adds(hc16 a, hc16 b) { return {h_sat16(a.r + b.r), h_sat16(a.i + b.i)}; }
inline hc16 h_subs(hc16 a, hc16 b) { return {h_sat16(a.r - b.r), h_sat16(a.i - b.i)}; }
inline hc16 h_addw(hc16 a, hc16 b) { return {h_wrap16(a.r + b.r), h_wrap16(a.i + b.i)}; }
inline hc16 h_flip(hc16 a) { return {a.i, h_wrap16(-(int32_t)a.r)}; }
inline hc16 h_pack(uint32_t re, uint32_t im) { return {h_sat16((int32_t)re >> 15), h_sat16((int32_t)im >> 15)}; }
inline hc16 h_tw(int N, int m)
{
  hc16 t;
  twiddle_host(N, m, &t.r, &t.i);
  return t;
}
/* x conj(t) in 32 bits, as unsigned so that the sums behind it wrap */
inline void h_mulc(hc16 x, hc16 t, uint32_t &re, uint32_t &im)
{
  re = (uint32_t)((int32_t)x.r * t.r + (int32_t)x.i * t.i);
  im = (uint32_t)((int32_t)x.r * (int32_t)h_wrap16(-(int32_t)t.i) + (int32_t)x.i * t.r);
}
inline hc16 h_mulc16(hc16 x, hc16 t)
{
  uint32_t re, im;
  h_mulc(x, t, re, im);
  return h_pack(re, im);
}
inline void h_r4inv(hc16 p0, hc16 p1, hc16 p2, hc16 p3, hc16 &o0, hc16 &o1, hc16 &o2, hc16 &o3)
{
  const hc16 s02 = h_adds(p0, p2), s13 = h_adds(p1, p3), d02 = h_subs(p0, p2), d13 = h_subs(h_flip(p1), h_flip(p3));
  o0 = h_adds(s02, s13);
  o2 = h_subs(s02, s13);
  o3 = h_adds(d02, d13);
  o1 = h_subs(d02, d13);
}
/* y = IDFT(x) of 2^l2 points with the size's own scaling (idft64 >> 3, radix-4 levels >> 1, radix-2 levels x 23170 >> 15) */
void h_idft(int l2, const hc16 *x, hc16 *y)
{
  const int N = 1 << l2;
  if (l2 == 4) {
    hc16 S[4][4], B[4][4];
    for (int j = 0; j < 4; j++) h_r4inv(x[j], x[4 + j], x[8 + j], x[12 + j], S[0][j], S[1][j], S[2][j], S[3][j]);
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 4; k++) B[j][k] = j == 0 ? S[k][j] : h_mulc16(S[k][j], h_tw(16, j * k));
    for (int k = 0; k < 4; k++) h_r4inv(B[0][k], B[1][k], B[2][k], B[3][k], y[k], y[4 + k], y[8 + k], y[12 + k]);
    return;
  }
  const int R = (l2 & 1) ? 2 : 4, M = N / R;
  std::vector<hc16> blk(N), Y(N);
  for (int r = 0; r < R; r++) {
    for (int n = 0; n < M; n++) blk[r * M + n] = x[R * n + r];
    h_idft(l2 - (R == 2 ? 1 : 2), &blk[r * M], &Y[r * M]);
  }
  for (int k = 0; k < M; k++) {
    if (l2 == 6) {
      h_r4inv(Y[k], h_mulc16(Y[M + k], h_tw(64, k)), h_mulc16(Y[2 * M + k], h_tw(64, 2 * k)), h_mulc16(Y[3 * M + k], h_tw(64, 3 * k)),
              y[k], y[M + k], y[2 * M + k], y[3 * M + k]);
    } else if (R == 4) {
      uint32_t a1r, a1i, a2r, a2i, a3r, a3i;
      h_mulc(Y[M + k], h_tw(N, k), a1r, a1i);
      h_mulc(Y[2 * M + k], h_tw(N, 2 * k), a2r, a2i);
      h_mulc(Y[3 * M + k], h_tw(N, 3 * k), a3r, a3i);
      y[k] = h_addw(Y[k], h_pack(a1r + a2r + a3r, a1i + a2i + a3i));
      y[3 * M + k] = h_addw(Y[k], h_pack(a1i - (a2r + a3i), a3r - a2i - a1r));
      y[2 * M + k] = h_addw(Y[k], h_pack(a2r - a3r - a1r, a2i - a3i - a1i));
      y[M + k] = h_addw(Y[k], h_pack(a3i - a2r - a1i, a1r - (a2i + a3r)));
    } else {
      uint32_t a0r, a0i, a1r, a1i;
      h_mulc(Y[k], hc16{32767, 0}, a0r, a0i);
      h_mulc(Y[M + k], h_tw(N, k), a1r, a1i);
      y[k] = h_pack(a0r + a1r, a0i + a1i);
      y[M + k] = h_pack(a0r - a1r, a0i - a1i);
    }
  }
  for (int k = 0; k < N; k++) {
    if (l2 == 6) y[k] = {(int16_t)(y[k].r >> 3), (int16_t)(y[k].i >> 3)};
    else if (R == 4) y[k] = {(int16_t)(y[k].r >> 1), (int16_t)(y[k].i >> 1)};
    else y[k] = {h_wrap16((((int32_t)y[k].r * 23170) >> 16) << 1), h_wrap16((((int32_t)y[k].i * 23170) >> 16) << 1)};
  }
}
}  // namespace

/* what the cell search is defined for: FDD, the normal prefix, 1 or 2 receive antennas, and the sizes for which
 * lte_sync_time_init's switch (:157-186) builds replicas with an inverse DFT this library has */
static bool sync_ok(const char *who, const oai4g_frame_parms_t *fp, uint32_t nb_rx)
{
  if (!fp) { set_err("%s: null frame parameters", who); return false; }
  if (fp->frame_type != 0) { set_err("%s: TDD is not supported", who); return false; }
  if (fp->Ncp != 0) { set_err("%s: the extended prefix is not supported", who); return false; }
  if (nb_rx < 1 || nb_rx > 2) { set_err("%s: %u receive antennas (1 or 2 are supported)", who, nb_rx); return false; }
  if (fp->N_RB_DL == 15) { set_err("%s: N_RB_DL 15 has no 256-point case in lte_sync_time_init: its replicas are all zero", who); return false; }
  if (fp->N_RB_DL == 75) { set_err("%s: N_RB_DL 75 (idft1536) is not supported", who); return false; }
  const uint32_t N = fp->N_RB_DL == 6 ? 128u : fp->N_RB_DL == 25 ? 512u : fp->N_RB_DL == 50 ? 1024u : fp->N_RB_DL == 100 ? 2048u : 0u;
  if (N == 0 || fp->ofdm_symbol_size != N || fp->samples_per_tti != 15u * N) {
    set_err("%s: N_RB_DL %u with ofdm_symbol_size %u is not supported", who, fp->N_RB_DL, fp->ofdm_symbol_size);
    return false;
  }
  return true;
}

/* lte_sync_time_init (:143-292): primary_synch<Nid2>[0..71] >> 2 from bin N - 36 on, DC skipped at the wrap, inverse
 * DFT with scale 1.  Entries 5..66 of the reference's 72 are the Zadoff-Chu values, the rest are 0. */
extern "C" int oai4g_lte_sync_time_replicas(const oai4g_frame_parms_t *fp, int32_t *out)
{
  if (!sync_ok("lte_sync_time_replicas", fp, 1) || !out) { if (fp && !out) set_err("lte_sync_time_replicas: null output"); return -1; }
  const uint32_t N = fp->ofdm_symbol_size;
  std::vector<hc16> F(N), T(N);
  for (uint32_t s = 0; s < 3; s++) {
    int16_t v[62][2];
    pss_table(s, v);
    std::fill(F.begin(), F.end(), hc16{0, 0});
    uint32_t k = N - 36;
    for (uint32_t i = 0; i < 72; i++) {
      if (i >= 5 && i < 67) F[k] = {(int16_t)(v[i - 5][0] >> 2), (int16_t)(v[i - 5][1] >> 2)};
      if (++k >= N) k = k + 1 - N;
    }
    h_idft(fp->log2_symbol_size, F.data(), T.data());
    memcpy(out + (size_t)s * N, T.data(), (size_t)N * 4);
  }
  return 0;
}

struct oai4g_sync_config {
  oai4g_frame_parms_t fp;
  uint32_t nb_rx;
  dev_buf<uint32_t> rep;                  /* [3][N] */
  dev_buf<unsigned long long> keys;       /* [n] of the last batch */
  dev_buf<uint32_t> pss;                  /* [3][62], with dbits: the SSS stage's tables, built when it first runs */
  dev_buf<unsigned long long> dbits;      /* [504][2] */
  dev_buf<int32_t> sssF;                  /* [n][nb_rx][4][N]: the SSS stage's FEP rows of the last batch */
};

extern "C" oai4g_sync_config_t *oai4g_sync_config_create(const oai4g_frame_parms_t *fp, uint8_t nb_antennas_rx)
{
  if (!sync_ok("sync_config_create", fp, nb_antennas_rx)) return nullptr;
  std::vector<uint32_t> rep(3 * (size_t)fp->ofdm_symbol_size);
  if (oai4g_lte_sync_time_replicas(fp, (int32_t *)rep.data()) != 0) return nullptr;
  NEED_INIT(nullptr);
  std::unique_ptr<oai4g_sync_config_t> cfg(new oai4g_sync_config_t);
  cfg->fp = *fp;
  cfg->nb_rx = nb_antennas_rx;
  HCK(cfg->rep.upload(rep), nullptr);
  return cfg.release();
}

extern "C" void oai4g_sync_config_destroy(oai4g_sync_config_t *cfg) { delete cfg; }

extern "C" int oai4g_sync_time_batch(oai4g_sync_config_t *cfg, int n, const int32_t *d_rx, int32_t *d_peak, int32_t *d_corr,
                                     void *stream)
{
  if (!cfg || n < 0 || (n > 0 && (!d_rx || !d_peak))) { set_err("sync_time_batch: bad arguments"); return -1; }
  NEED_INIT(-1);
  if (n == 0) return 0;
  if (cfg->keys.count() < (size_t)n) {
    HCK(hipDeviceSynchronize(), -1);                                   /* an earlier batch may still use the old slots */
    HCK(cfg->keys.reserve((size_t)n), -1);
  }
  sync_time_args_t a;
  memset(&a, 0, sizeof(a));
  a.rx = (const uint32_t *)d_rx;
  a.rep = cfg->rep.get();
  a.N = cfg->fp.ofdm_symbol_size;
  a.length = 5u * cfg->fp.samples_per_tti;
  a.nb_rx = cfg->nb_rx;
  a.n = (uint32_t)n;
  a.keys = cfg->keys.get();
  a.peak = d_peak;
  a.corr = d_corr;
  HCK(oai4g_launch_sync_time(a, (hipStream_t)stream), -1);
  return 0;
}

/* lte_sync_time (:357) of one frame on the host's buffers: rxdata[aa] holds 10 samples_per_tti words.  sync_corr,
 * when not null, receives the three buffers [3][10 samples_per_tti], every fourth entry defined. */
extern "C" int oai4g_lte_sync_time(int32_t *const *rxdata, const oai4g_frame_parms_t *fp, uint8_t nb_antennas_rx, int *eNB_id,
                                   uint32_t *peak_val, int32_t *sync_corr)
{
  if (!sync_ok("lte_sync_time", fp, nb_antennas_rx)) return -1;
  if (!rxdata || !rxdata[0] || (nb_antennas_rx > 1 && !rxdata[1])) { set_err("lte_sync_time: null rxdata"); return -1; }
  NEED_INIT(-1);
  const size_t fl = (size_t)10 * fp->samples_per_tti, fb = fl * 4;
  std::unique_ptr<oai4g_sync_config_t, void (*)(oai4g_sync_config_t *)> cfg(oai4g_sync_config_create(fp, nb_antennas_rx),
                                                                            oai4g_sync_config_destroy);
  if (!cfg) return -1;
  stage_t st("lte_sync_time");
  const int r_rx = st.add(fb * nb_antennas_rx), r_peak = st.add(12), r_corr = st.add(sync_corr ? 3 * fb : 0);
  if (!st.open()) return -1;
  for (uint32_t aa = 0; aa < nb_antennas_rx; aa++) HCK(st.up(r_rx, rxdata[aa], fb, aa * fb), -1);
  if (oai4g_sync_time_batch(cfg.get(), 1, st.ptr<int32_t>(r_rx), st.ptr<int32_t>(r_peak), sync_corr ? st.ptr<int32_t>(r_corr) : nullptr,
                            g_scr.s) != 0)
    return -1;
  int32_t peak[3] = {0, 0, 0};
  HCK(st.down(peak, r_peak, 12), -1);
  if (sync_corr) HCK(st.down(sync_corr, r_corr, 3 * fb), -1);
  HCK(st.sync(), -1);                                                  /* the configuration goes after the kernels have run */
  if (eNB_id) *eNB_id = peak[2];
  if (peak_val) *peak_val = (uint32_t)peak[1];
  return peak[0];
}

/* slot_fep's window of symbol l of slot Ns without the sample offset (slot_fep.c:105-150): what is added in front of
 * the alignment and what behind it */
static void fep_offset_sym(const oai4g_frame_parms_t *fp, uint32_t Ns, uint32_t l, uint32_t &pre, uint32_t &post)
{
  pre = fp->samples_per_tti * (Ns >> 1) + (fp->samples_per_tti >> 1) * (Ns & 1u) + fp->nb_prefix_samples0;
  post = (fp->ofdm_symbol_size + fp->nb_prefix_samples) * l;
}

extern "C" int oai4g_fep_offset_batch(const oai4g_frame_parms_t *fp, int n, int nb_antennas_rx, const int32_t *d_rx,
                                      const int32_t *d_offset, uint32_t offset_stride, uint8_t first_slot, int nsym,
                                      int32_t *d_rxF, size_t frame_stride, void *stream)
{
  if (!sync_ok("fep_offset_batch", fp, nb_antennas_rx > 0 ? (uint32_t)nb_antennas_rx : 0u)) return -1;
  const uint32_t nslot = fp->symbols_per_tti / 2u, N = fp->ofdm_symbol_size;
  if (n < 0 || nsym < 1 || nsym > (int)fp->symbols_per_tti || first_slot + (nsym + nslot - 1) / nslot > 20 ||
      (n > 0 && (!d_rx || !d_offset || !d_rxF))) {
    set_err("fep_offset_batch: bad arguments (1 to %u symbols from slot %u, inside the frame)", fp->symbols_per_tti, first_slot);
    return -1;
  }
  static_assert(OAI4G_FEP_MAX_SYM <= OAI4G_FEP_OFFSET_MAX_SYM, "a subframe's rows fit the argument block");
  const size_t ant_stride = (size_t)fp->symbols_per_tti * N;
  if (frame_stride == 0) frame_stride = ant_stride * nb_antennas_rx;
  if (frame_stride < ant_stride * nb_antennas_rx || frame_stride * (size_t)n > 0xFFFFFFFFull) {
    set_err("fep_offset_batch: frame stride %zu", frame_stride);
    return -1;
  }
  NEED_INIT(-1);
  if (n == 0) return 0;
  fep_offset_args_t a;
  memset(&a, 0, sizeof(a));
  a.nsym = nsym;
  a.n_units = n * nb_antennas_rx * nsym;
  a.n_ant = (uint32_t)nb_antennas_rx;
  a.frame_len = 10u * fp->samples_per_tti;
  a.out_frame_stride = (uint32_t)frame_stride;
  a.out_ant_stride = (uint32_t)ant_stride;
  a.offset = d_offset;
  a.offset_stride = offset_stride;
  a.scale = 1;
  for (int k = 0; k < nsym; k++) fep_offset_sym(fp, first_slot + (uint32_t)k / nslot, (uint32_t)k % nslot, a.pre[k], a.post[k]);
  HCK(oai4g_launch_fep_offset(d_rx, d_rxF, fp->log2_symbol_size, a, g_twf, g_n_cu, (hipStream_t)stream), -1);
  return 0;
}

/* the tables of the SSS stage, built when it first runs: primary_synch<Nid2>[10..133] as words, and d0_sss / d5_sss as
 * sign bits */
static int sync_sss_tables(oai4g_sync_config_t *cfg)
{
  if (cfg->pss) return 0;
  std::vector<uint32_t> pss(3 * 62);
  for (uint32_t s = 0; s < 3; s++) {
    int16_t v[62][2];
    pss_table(s, v);
    for (int i = 0; i < 62; i++) pss[s * 62 + i] = (uint32_t)(uint16_t)v[i][0] | ((uint32_t)(uint16_t)v[i][1] << 16);
  }
  std::vector<unsigned long long> bits(504 * 2, 0ull);
  for (uint32_t nid = 0; nid < 504; nid++)
    for (int sf5 = 0; sf5 < 2; sf5++) {
      int16_t d[62];
      sss_table(nid, sf5 != 0, d);
      for (int i = 0; i < 62; i++)
        if (d[i] < 0) bits[2 * nid + sf5] |= 1ull << i;
    }
  HCK(cfg->dbits.upload(bits), -1);
  HCK(cfg->pss.upload(pss), -1);
  return 0;
}

static void sss_fill(const oai4g_sync_config_t *cfg, sss_args_t &a, uint32_t n)
{
  memset(&a, 0, sizeof(a));
  a.pss = cfg->pss.get();
  a.d = cfg->dbits.get();
  a.n = n;
  a.nb_rx = cfg->nb_rx;
  a.N = cfg->fp.ofdm_symbol_size;
  a.cp = cfg->fp.nb_prefix_samples;
  a.spt = cfg->fp.samples_per_tti;
  /* the seven phase hypotheses between PSS and SSS, -60 .. 60 degrees in Q15 (the values of sss.c:218-219, which no
   * single rounding rule reproduces) */
  static const int16_t phase_re[7] = {16383, 25101, 30791, 32767, 30791, 25101, 16383};
  static const int16_t phase_im[7] = {-28378, -21063, -11208, 0, 11207, 21062, 28377};
  memcpy(a.phase_re, phase_re, sizeof(phase_re));
  memcpy(a.phase_im, phase_im, sizeof(phase_im));
}

/* the four slot_fep calls of rx_sss (sss.c:247-259, :306-316) at the records' rx_offset, then the detection */
static int sss_run(oai4g_sync_config_t *cfg, sss_args_t &a, const int32_t *d_rx, hipStream_t s)
{
  const uint32_t N = a.N;
  if (cfg->sssF.count() < (size_t)a.n * a.nb_rx * 4 * N) {
    HCK(hipDeviceSynchronize(), -1);                                   /* an earlier batch may still use the old rows */
    HCK(cfg->sssF.reserve((size_t)a.n * a.nb_rx * 4 * N), -1);
  }
  fep_offset_args_t f;
  memset(&f, 0, sizeof(f));
  f.nsym = 4;
  f.n_units = (int)(a.n * a.nb_rx * 4u);
  f.n_ant = a.nb_rx;
  f.frame_len = 10u * a.spt;
  f.out_ant_stride = 4u * N;
  f.out_frame_stride = a.nb_rx * 4u * N;
  f.offset = a.cell + 1;
  f.offset_stride = OAI4G_CELL_WORDS;
  f.scale = 1;
  for (uint32_t k = 0; k < 4; k++) fep_offset_sym(&cfg->fp, k < 2 ? 0u : 10u, 5u + (k & 1u), f.pre[k], f.post[k]);
  HCK(oai4g_launch_fep_offset(d_rx, cfg->sssF.get(), cfg->fp.log2_symbol_size, f, g_twf, g_n_cu, s), -1);
  a.rxF = cfg->sssF.get();
  HCK(oai4g_launch_sss(a, s), -1);
  return 0;
}

static_assert(sizeof(oai4g_cell_t) == 4 * OAI4G_CELL_WORDS, "the kernels address a cell record as six words");

extern "C" int oai4g_sss_batch(oai4g_sync_config_t *cfg, int n, const int32_t *d_rx, const int32_t *d_peak, oai4g_cell_t *d_cell,
                               void *stream)
{
  if (!cfg || n < 0 || (n > 0 && (!d_rx || !d_peak || !d_cell))) { set_err("sss_batch: bad arguments"); return -1; }
  NEED_INIT(-1);
  if (n == 0) return 0;
  if (sync_sss_tables(cfg) != 0) return -1;
  sss_args_t a;
  sss_fill(cfg, a, (uint32_t)n);
  a.peak = d_peak;
  a.cell = (int32_t *)d_cell;
  a.add_half = 1;
  HCK(oai4g_launch_sss_offsets(a, (hipStream_t)stream), -1);
  return sss_run(cfg, a, d_rx, (hipStream_t)stream);
}

/* the same behind the four slot_fep calls, on the caller's rows [n][nb_rx][4][N] (symbols 5 and 6 of slot 0, then of
 * slot 10): values the forward DFT's own scaling never produces, such as full-scale symbols, can be put through the
 * compensation and the search */
extern "C" int oai4g_sss_rows_batch(oai4g_sync_config_t *cfg, int n, const int32_t *d_rows, const int32_t *d_peak,
                                    oai4g_cell_t *d_cell, void *stream)
{
  if (!cfg || n < 0 || (n > 0 && (!d_rows || !d_peak || !d_cell))) { set_err("sss_rows_batch: bad arguments"); return -1; }
  NEED_INIT(-1);
  if (n == 0) return 0;
  if (sync_sss_tables(cfg) != 0) return -1;
  sss_args_t a;
  sss_fill(cfg, a, (uint32_t)n);
  a.peak = d_peak;
  a.cell = (int32_t *)d_cell;
  a.add_half = 1;
  a.rxF = d_rows;
  HCK(oai4g_launch_sss_offsets(a, (hipStream_t)stream), -1);
  HCK(oai4g_launch_sss(a, (hipStream_t)stream), -1);
  return 0;
}

/* rx_sss (sss.c:222) on one frame in host memory: the sequence the PSS stage found and phy_vars_ue->rx_offset come
 * from the caller; returns the Nid_cell it leaves in the frame parameters */
extern "C" int oai4g_rx_sss(int32_t *const *rxdata, const oai4g_frame_parms_t *fp, uint8_t nb_antennas_rx, uint8_t Nid2,
                            int rx_offset, int32_t *tot_metric, uint8_t *flip_max, uint8_t *phase_max)
{
  if (!sync_ok("rx_sss", fp, nb_antennas_rx)) return -1;
  if (!rxdata || !rxdata[0] || (nb_antennas_rx > 1 && !rxdata[1]) || Nid2 > 2 || rx_offset < 0) {
    set_err("rx_sss: null rxdata, Nid2 %u or a negative rx_offset", Nid2);
    return -1;
  }
  NEED_INIT(-1);
  const size_t fb = (size_t)10 * fp->samples_per_tti * 4;
  std::unique_ptr<oai4g_sync_config_t, void (*)(oai4g_sync_config_t *)> cfg(oai4g_sync_config_create(fp, nb_antennas_rx),
                                                                            oai4g_sync_config_destroy);
  if (!cfg || sync_sss_tables(cfg.get()) != 0) return -1;
  stage_t st("rx_sss");
  const int r_rx = st.add(fb * nb_antennas_rx), r_peak = st.add(12), r_cell = st.add(4 * OAI4G_CELL_WORDS);
  if (!st.open()) return -1;
  const int32_t peak[3] = {0, 0, Nid2};
  int32_t cell[OAI4G_CELL_WORDS] = {-1, rx_offset, 0, 0, 0, 0};
  for (uint32_t aa = 0; aa < nb_antennas_rx; aa++) HCK(st.up(r_rx, rxdata[aa], fb, aa * fb), -1);
  HCK(st.up(r_peak, peak, sizeof(peak)), -1);
  HCK(st.up(r_cell, cell, sizeof(cell)), -1);
  sss_args_t a;
  sss_fill(cfg.get(), a, 1);
  a.peak = st.ptr<int32_t>(r_peak);
  a.cell = st.ptr<int32_t>(r_cell);
  if (sss_run(cfg.get(), a, st.ptr<int32_t>(r_rx), g_scr.s) != 0) return -1;
  HCK(st.down(cell, r_cell, sizeof(cell)), -1);
  HCK(st.sync(), -1);
  if (tot_metric) *tot_metric = cell[2];
  if (flip_max) *flip_max = (uint8_t)cell[3];
  if (phase_max) *phase_max = (uint8_t)cell[4];
  return cell[0];
}

/* initial_sync's first hypothesis (initial_sync.c:290-372, FDD with the normal prefix) on one frame in host memory:
 * lte_sync_time, the offset arithmetic and rx_sss, the frame parameters of the found cell, pbch_detection's slot_fep
 * calls (:69-92: slots 0 and 1 and symbol 0 of slot 2 at rx_offset), the channel estimation of nb_ports ports, the
 * PBCH front end and the eight-hypothesis search.  The cell is read back once in the middle: the estimation and PBCH
 * configurations are per cell. */
extern "C" int oai4g_initial_sync(int32_t *const *rxdata, const oai4g_frame_parms_t *fp, uint8_t nb_antennas_rx, uint8_t nb_ports,
                                  uint32_t high_speed_flag, oai4g_initial_sync_t *out)
{
  if (!sync_ok("initial_sync", fp, nb_antennas_rx)) return -1;
  if (!rxdata || !rxdata[0] || (nb_antennas_rx > 1 && !rxdata[1]) || !out || nb_ports < 1 || nb_ports > 2) {
    set_err("initial_sync: null argument or %u estimated ports (1 or 2)", nb_ports);
    return -1;
  }
  NEED_INIT(-1);
  memset(out, 0, sizeof(*out));
  out->Nid_cell = -1;
  out->tx_ant = 0xFF;
  using sync_ptr = std::unique_ptr<oai4g_sync_config_t, void (*)(oai4g_sync_config_t *)>;
  using chest_ptr = std::unique_ptr<oai4g_chest_config_t, void (*)(oai4g_chest_config_t *)>;
  using pbch_ptr = std::unique_ptr<oai4g_pbch_front_config_t, void (*)(oai4g_pbch_front_config_t *)>;
  sync_ptr cfg(oai4g_sync_config_create(fp, nb_antennas_rx), oai4g_sync_config_destroy);
  if (!cfg) return -1;
  const uint32_t N = fp->ofdm_symbol_size, nb_rx = nb_antennas_rx;
  const size_t fb = (size_t)10 * fp->samples_per_tti * 4, grid = (size_t)fp->symbols_per_tti * N;
  stage_t st("initial_sync");
  const int r_rx = st.add(fb * nb_rx), r_peak = st.add(12), r_cell = st.add(sizeof(oai4g_cell_t));
  const int r_rxF = st.add(2 * nb_rx * grid * 4), r_est = st.add(4 * grid * 4), r_llr = st.add(2 * OAI4G_PBCH_SOFT);
  const int r_l2 = st.add(4), r_det = st.add(sizeof(oai4g_pbch_detect_t));
  if (!st.open()) return -1;
  for (uint32_t aa = 0; aa < nb_rx; aa++) HCK(st.up(r_rx, rxdata[aa], fb, aa * fb), -1);
  const int32_t *d_rx = st.ptr<int32_t>(r_rx);
  oai4g_cell_t *d_cell = st.ptr<oai4g_cell_t>(r_cell);
  if (oai4g_sync_time_batch(cfg.get(), 1, d_rx, st.ptr<int32_t>(r_peak), nullptr, g_scr.s) != 0 ||
      oai4g_sss_batch(cfg.get(), 1, d_rx, st.ptr<int32_t>(r_peak), d_cell, g_scr.s) != 0)
    return -1;
  oai4g_cell_t cell;
  HCK(st.down(&cell, r_cell, sizeof(cell)), -1);
  HCK(st.sync(), -1);
  out->rx_offset = cell.rx_offset;
  if (cell.status != 0) { set_err("initial_sync: SSS error condition (rx_offset %d)", cell.rx_offset); return -1; }
  out->Nid_cell = cell.Nid_cell;
  oai4g_frame_parms_t fc;
  if (oai4g_init_frame_parms(&fc, fp->N_RB_DL, (uint16_t)cell.Nid_cell, 0, nb_ports, nb_ports == 1, 0) != 0) return -1;
  /* rows: element 0 holds slots 0 and 1 per antenna, element 1's row 0 the symbol that closes rows 12 / 13 */
  int32_t *d_rxF = st.ptr<int32_t>(r_rxF);
  const int32_t *d_off = &d_cell->rx_offset;
  if (oai4g_fep_offset_batch(&fc, 1, nb_rx, d_rx, d_off, 0, 0, fc.symbols_per_tti, d_rxF, 0, g_scr.s) != 0 ||
      oai4g_fep_offset_batch(&fc, 1, nb_rx, d_rx, d_off, 0, 2, 1, d_rxF + nb_rx * grid, 0, g_scr.s) != 0)
    return -1;
  HCK(st.zero(r_est, 4 * grid * 4, r_est), -1);
  const int32_t *ep[4] = {nullptr, nullptr, nullptr, nullptr};
  for (uint32_t p = 0; p < nb_ports; p++) {
    chest_ptr ce(oai4g_chest_config_create(&fc, (uint8_t)p, 0, 0), oai4g_chest_config_destroy);
    if (!ce || oai4g_chest_config_set_stride(ce.get(), nb_rx, nb_rx) != 0) return -1;
    for (uint32_t aa = 0; aa < nb_rx; aa++) {
      int32_t *e = st.ptr<int32_t>(r_est, ((p << 1) + aa) * grid * 4);
      if (oai4g_chest_batch(ce.get(), 1, d_rxF + aa * grid, e, g_scr.s) != 0) return -1;
      ep[(p << 1) + aa] = e;
    }
    HCK(st.sync(), -1);                                                /* the configuration goes with this scope */
  }
  pbch_ptr pb(oai4g_pbch_front_config_create(&fc, nb_antennas_rx, nb_ports, high_speed_flag), oai4g_pbch_front_config_destroy);
  if (!pb) return -1;
  oai4g_pbch_detect_t det;
  if (oai4g_pbch_front_batch(pb.get(), 1, d_rxF, ep, st.ptr<int8_t>(r_llr), st.ptr(r_l2), g_scr.s) != 0 ||
      oai4g_pbch_detect_batch(pb.get(), 1, st.ptr<int8_t>(r_llr), st.ptr<oai4g_pbch_detect_t>(r_det), g_scr.s) != 0)
    return -1;
  HCK(st.down(&det, r_det, sizeof(det)), -1);
  HCK(st.sync(), -1);
  if (det.tx_ant != 1 && det.tx_ant != 2) { set_err(""); return -1; }   /* no PBCH found: not an error of the call */
  out->tx_ant = det.tx_ant;
  out->frame_mod4 = det.frame_mod4;
  out->mimo_mode = det.mimo_mode;
  memcpy(out->mib, det.mib, 3);
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * fading channels: new_channel_desc_scm / fill_channel_desc (SIMULATION/TOOLS/random_channel.c:195-860, :42-147),
 * random_channel and multipath_channel batched over trials (oai4g_channel.hip)
 * ---------------------------------------------------------------------------------------- */
namespace {
enum { CH_EPA = 5, CH_EVA = 6, CH_ETU = 7, CH_RAYLEIGH8 = 9, CH_RAYLEIGH1 = 10, CH_RAYLEIGH1_800 = 11, CH_RAYLEIGH1_CORR = 12,
       CH_RAYLEIGH1_ANTICORR = 13, CH_RICE8 = 14, CH_RICE1 = 15, CH_RICE1_CORR = 16, CH_RICE1_ANTICORR = 17, CH_AWGN = 18 };

/* tap delays in us and powers in dB (3GPP TS 36.101 B.2.1, as random_channel.c:156-163 states them), and the 8-tap
 * models' linear powers (:165) */
const double epa_delays[] = {0, .03, .07, .09, .11, .19, .41};
const double epa_amps_dB[] = {0.0, -1.0, -2.0, -3.0, -8.0, -17.2, -20.8};
const double eva_delays[] = {0, .03, .15, .31, .37, .71, 1.09, 1.73, 2.51};
const double eva_amps_dB[] = {0.0, -1.5, -1.4, -3.6, -0.6, -9.1, -7.0, -12.0, -16.9};
const double etu_delays[] = {0, .05, .12, .2, .23, .5, 1.6, 2.3, 5.0};
const double etu_amps_dB[] = {-1.0, -1.0, -1.0, 0.0, 0.0, 0.0, -3.0, -5.0, -7.0};
const double amps8_lin[] = {0.3868472, 0.3094778, 0.1547389, 0.0773694, 0.0386847, 0.0193424, 0.0096712, 0.0038685};

/* scm_corrmat.h R22_sqrt: six 4x4 complex matrices, [re, im] row by row; pinned entry by entry by
 * tests/golden/channel_ref.json */
const double r22_sqrt[6][32] = {
  {0.921700, -0.000000, 0.010380, -0.027448, -0.250153, 0.294754, 0.005961, 0.010769, 0.010380, 0.027448, 0.921700, 0.000000, -0.011595, -0.004130, -0.250153, 0.294754, -0.250153, -0.294754, -0.011595, 0.004130, 0.921700, 0.000000, 0.010380, -0.027448, 0.005961, -0.010769, -0.250153, -0.294754, 0.010380, 0.027448, 0.921700, 0.000000},
  {0.923810, 0.000000, 0.004069, 0.027832, 0.151730, 0.350180, -0.009882, 0.006114, 0.004069, -0.027832, 0.923810, 0.000000, 0.011218, -0.003029, 0.151730, 0.350180, 0.151730, -0.350180, 0.011218, 0.003029, 0.923810, -0.000000, 0.004069, 0.027832, -0.009882, -0.006114, 0.151730, -0.350180, 0.004069, -0.027832, 0.923810, 0.000000},
  {0.927613, 0.000000, 0.014253, 0.025767, -0.061171, -0.367133, 0.009258, -0.007340, 0.014253, -0.025767, 0.927613, -0.000000, -0.011138, -0.003942, -0.061171, -0.367133, -0.061171, 0.367133, -0.011138, 0.003942, 0.927613, 0.000000, 0.014253, 0.025767, 0.009258, 0.007340, -0.061171, 0.367133, 0.014253, -0.025767, 0.927613, 0.000000},
  {0.869794, -0.000000, -0.010613, -0.001218, 0.399115, 0.289852, -0.004464, -0.004096, -0.010613, 0.001218, 0.869794, -0.000000, -0.005276, -0.002978, 0.399115, 0.289852, 0.399115, -0.289852, -0.005276, 0.002978, 0.869794, -0.000000, -0.010613, -0.001218, -0.004464, 0.004096, 0.399115, -0.289852, -0.010613, 0.001218, 0.869794, 0.000000},
  {0.919726, -0.000000, 0.038700, -0.111146, 0.217804, 0.300925, 0.045531, -0.013659, 0.038700, 0.111146, 0.919726, 0.000000, -0.027201, 0.038983, 0.217804, 0.300925, 0.217804, -0.300925, -0.027201, -0.038983, 0.919726, 0.000000, 0.038700, -0.111146, 0.045531, 0.013659, 0.217804, -0.300925, 0.038700, 0.111146, 0.919726, 0.000000},
  {0.867608, -0.000000, 0.194097, -0.112414, -0.418811, 0.095938, -0.081264, 0.075727, 0.194097, 0.112414, 0.867608, -0.000000, -0.106125, -0.032801, -0.418811, 0.095938, -0.418811, -0.095938, -0.106125, 0.032801, 0.867608, 0.000000, 0.194097, -0.112414, -0.081264, -0.075727, -0.418811, -0.095938, 0.194097, 0.112414, 0.867608, 0.000000},
};

struct chan_model_t {
  oai4g_channel_info_t info;
  std::vector<double> R;                 /* [n_matrices][npair][npair][re, im] */
};

/* the descriptor of a model, or false with the error set */
bool chan_describe(int model, uint32_t nb_tx, uint32_t nb_rx, double BW, chan_model_t &m)
{
  if (nb_tx < 1 || nb_tx > 2 || nb_rx < 1 || nb_rx > 2) {
    set_err("channel: nb_tx %u, nb_rx %u: 1 or 2 antennas a side (the reference's NB_ANTENNAS_TX / _RX)", nb_tx, nb_rx);
    return false;
  }
  if (!(BW > 0.0)) { set_err("channel: BW %g", BW); return false; }
  oai4g_channel_info_t &d = m.info;
  memset(&d, 0, sizeof(d));
  const uint32_t n = nb_tx * nb_rx;
  double corr = 0.0;                     /* the cross terms' sign of a fully (anti-)correlated transmit pair */
  const double *delays = nullptr, *dB = nullptr;
  double Td = 0.0, len = 1.0;
  d.ricean_factor = 1.0;
  d.aoa = .03;
  switch (model) {
  case CH_EPA: d.nb_taps = 7; Td = .410; delays = epa_delays; dB = epa_amps_dB; break;
  case CH_EVA: d.nb_taps = 9; Td = 2.51; delays = eva_delays; dB = eva_amps_dB; break;
  case CH_ETU: d.nb_taps = 9; Td = 5.0; delays = etu_delays; dB = etu_amps_dB; break;
  case CH_RICE8: d.ricean_factor = 0.1; d.random_aoa = 1; /* fall through */
  case CH_RAYLEIGH8: d.nb_taps = 8; Td = 0.8; break;
  case CH_RICE1_CORR: case CH_RICE1_ANTICORR: d.random_aoa = 1; /* fall through */
  case CH_RICE1: d.ricean_factor = 0.1; /* fall through */
  case CH_RAYLEIGH1: case CH_RAYLEIGH1_800: case CH_RAYLEIGH1_CORR: case CH_RAYLEIGH1_ANTICORR: d.nb_taps = 1; break;
  case CH_AWGN: d.nb_taps = 1; d.ricean_factor = 0.0; d.aoa = 0.0; break;
  case 1: case 2: set_err("channel: model %d (SCM_A / SCM_B): the reference has no such descriptor", model); return false;
  case 3: case 4: set_err("channel: model %d (SCM_C / SCM_D) is not built", model); return false;
  default: set_err("channel: model %d is not supported", model); return false;
  }
  if (model == CH_RAYLEIGH1_CORR || model == CH_RICE1_CORR) corr = 1.0;
  if (model == CH_RAYLEIGH1_ANTICORR || model == CH_RICE1_ANTICORR) corr = -1.0;
  if (dB) {
    /* amps = 10^(dB / 10) / sum_amps; channel_length from the delay spread (:352) */
    double sum_amps = 0;
    for (uint32_t i = 0; i < d.nb_taps; i++) {
      d.amps[i] = pow(10, .1 * dB[i]);
      sum_amps += d.amps[i];
    }
    for (uint32_t i = 0; i < d.nb_taps; i++) {
      d.amps[i] /= sum_amps;
      d.delays[i] = delays[i];
    }
    d.aoa = 0;
    len = 2 * BW * Td + 1 + 2 / (M_PI * M_PI) * log(4 * M_PI * BW * Td);
  } else if (d.nb_taps == 8) {
    const double delta_tau = Td / d.nb_taps;
    for (uint32_t i = 0; i < 8; i++) {
      d.amps[i] = amps8_lin[i];
      d.delays[i] = ((double)i) * delta_tau;
    }
    len = 11 + 2 * BW * Td;
  } else {
    d.amps[0] = 1;
  }
  if (!(len < OAI4G_CHAN_MAX_LENGTH + 1.0)) {
    set_err("channel: channel_length %.0f at BW %g is beyond %d (the reference's field is a uint8_t)", len, BW, OAI4G_CHAN_MAX_LENGTH);
    return false;
  }
  d.channel_length = (uint32_t)(int)len;
  /* correlation: R22_sqrt[i / 3] for the tapped models at 2x2; the 0.70711 matrices of the _corr / _anticorr models
   * at 2x1 and 2x2 (:169-190); identity everywhere else, also for the tapped models at 1x2 and 2x1, where the
   * reference sets only the diagonal of uninitialised memory */
  d.n_matrices = dB ? 6 : (d.nb_taps - 1) / 3 + 1;
  m.R.assign((size_t)d.n_matrices * n * n * 2, 0.0);
  for (uint32_t k = 0; k < d.n_matrices; k++) {
    double *R = &m.R[(size_t)k * n * n * 2];
    if (dB && n == 4) {
      memcpy(R, r22_sqrt[k], sizeof(r22_sqrt[k]));
      continue;
    }
    for (uint32_t r = 0; r < n; r++) R[(r * n + r) * 2] = 1.0;
    if (corr != 0.0 && nb_tx == 2)
      for (uint32_t r = 0; r < n; r++) {
        R[(r * n + r) * 2] = 0.70711;
        R[(r * n + (r + nb_rx) % n) * 2] = corr * 0.70711;   /* the same receive antenna's other transmit antenna */
      }
  }
  return true;
}

void chan_r_out(const chan_model_t &m, double *r_sqrt)
{
  if (r_sqrt) memcpy(r_sqrt, m.R.data(), m.R.size() * sizeof(double));
}
}  // namespace

struct oai4g_channel_config {
  chan_model_t m;
  uint32_t nb_tx, nb_rx, n_vectors, dd, calls;
  double BW, ff, path_loss;
  dev_buf<double> R, a, ch;
  dev_buf<uint8_t> first_run;
};

extern "C" int oai4g_channel_model_describe(int model, uint8_t nb_tx, uint8_t nb_rx, double BW, oai4g_channel_info_t *info,
                                            double *r_sqrt)
{
  chan_model_t m;
  if (!info) { set_err("channel_model_describe: null info"); return -1; }
  if (!chan_describe(model, nb_tx, nb_rx, BW, m)) return -1;
  *info = m.info;
  chan_r_out(m, r_sqrt);
  return 0;
}

extern "C" oai4g_channel_config_t *oai4g_channel_config_create(uint8_t nb_tx, uint8_t nb_rx, int model, double BW,
                                                               double forgetting_factor, int32_t channel_offset,
                                                               double path_loss_dB, int n_vectors)
{
  std::unique_ptr<oai4g_channel_config_t> cfg(new oai4g_channel_config_t);
  if (!chan_describe(model, nb_tx, nb_rx, BW, cfg->m)) return nullptr;
  if (n_vectors < 1 || !(forgetting_factor >= 0.0 && forgetting_factor <= 1.0) || channel_offset == INT32_MIN) {
    set_err("channel_config_create: n_vectors %d (>= 1), forgetting_factor %g (0..1)", n_vectors, forgetting_factor);
    return nullptr;
  }
  NEED_INIT(nullptr);
  cfg->nb_tx = nb_tx;
  cfg->nb_rx = nb_rx;
  cfg->n_vectors = (uint32_t)n_vectors;
  cfg->dd = (uint32_t)abs(channel_offset);
  cfg->calls = 0;
  cfg->BW = BW;
  cfg->ff = forgetting_factor;
  cfg->path_loss = pow(10, path_loss_dB / 20);
  const size_t n = (size_t)nb_tx * nb_rx;
  HCK(cfg->R.upload(cfg->m.R), nullptr);
  HCK(cfg->a.reserve((size_t)n_vectors * cfg->m.info.nb_taps * n * 2), nullptr);
  HCK(cfg->ch.reserve((size_t)n_vectors * n * cfg->m.info.channel_length * 2), nullptr);
  HCK(cfg->first_run.upload(std::vector<uint8_t>((size_t)n_vectors, 1)), nullptr);
  HCK(hipMemset(cfg->a.get(), 0, cfg->a.count() * sizeof(double)), nullptr);
  HCK(hipMemset(cfg->ch.get(), 0, cfg->ch.count() * sizeof(double)), nullptr);
  return cfg.release();
}

extern "C" void oai4g_channel_config_destroy(oai4g_channel_config_t *cfg) { delete cfg; }

extern "C" int oai4g_channel_config_query(const oai4g_channel_config_t *cfg, oai4g_channel_info_t *info, double *r_sqrt)
{
  if (!cfg || !info) { set_err("channel_config_query: null argument"); return -1; }
  *info = cfg->m.info;
  chan_r_out(cfg->m, r_sqrt);
  return 0;
}

extern "C" int oai4g_channel_random_batch(oai4g_channel_config_t *cfg, int n, uint64_t seed, uint32_t first_vector, uint32_t step,
                                          const double *d_draws, void *stream)
{
  if (!cfg || n < 0 || (uint32_t)n > cfg->n_vectors) {
    set_err("channel_random_batch: %d vectors of a configuration for %u", n, cfg ? cfg->n_vectors : 0u);
    return -1;
  }
  NEED_INIT(-1);
  const oai4g_channel_info_t &d = cfg->m.info;
  chan_dev_t c;
  memset(&c, 0, sizeof(c));
  c.nb_tx = cfg->nb_tx;
  c.nb_rx = cfg->nb_rx;
  c.nb_taps = d.nb_taps;
  c.channel_length = d.channel_length;
  c.random_aoa = d.random_aoa;
  c.ricean_factor = d.ricean_factor;
  c.aoa = d.aoa;
  c.BW = cfg->BW;
  c.sqrt_ff = sqrt(cfg->ff);
  c.sqrt_1mff = sqrt(1 - cfg->ff);
  static_assert(OAI4G_CHAN_TAPS == OAI4G_CHANNEL_MAX_TAPS, "the kernel's tap tables hold the header's count");
  memcpy(c.amps, d.amps, sizeof(c.amps));
  memcpy(c.delays, d.delays, sizeof(c.delays));
  c.R = cfg->R.get();
  c.a = cfg->a.get();
  c.ch = cfg->ch.get();
  c.first_run = cfg->first_run.get();
  HCK(oai4g_launch_channel_taps(c, n, seed, first_vector, step, d_draws, (hipStream_t)stream), -1);
  return 0;
}

static bool chan_span(const oai4g_channel_config_t *cfg, const char *who, int first_vector, int n)
{
  if (cfg && first_vector >= 0 && n >= 0 && (uint32_t)first_vector <= cfg->n_vectors && (uint32_t)n <= cfg->n_vectors - first_vector)
    return true;
  set_err("%s: vectors [%d, +%d) of a configuration for %u", who, first_vector, n, cfg ? cfg->n_vectors : 0u);
  return false;
}

extern "C" int oai4g_channel_set_taps(oai4g_channel_config_t *cfg, int first_vector, int n, const double *ch, const double *a)
{
  if (!chan_span(cfg, "channel_set_taps", first_vector, n)) return -1;
  NEED_INIT(-1);
  const size_t np = (size_t)cfg->nb_tx * cfg->nb_rx, cw = np * cfg->m.info.channel_length * 2, aw = np * cfg->m.info.nb_taps * 2;
  HCK(hipDeviceSynchronize(), -1);
  if (ch) HCK(hipMemcpy(cfg->ch.get() + first_vector * cw, ch, (size_t)n * cw * sizeof(double), hipMemcpyHostToDevice), -1);
  if (a) {
    HCK(hipMemcpy(cfg->a.get() + first_vector * aw, a, (size_t)n * aw * sizeof(double), hipMemcpyHostToDevice), -1);
    HCK(hipMemset(cfg->first_run.get() + first_vector, 0, (size_t)n), -1);
  }
  return 0;
}

extern "C" int oai4g_channel_get_taps(oai4g_channel_config_t *cfg, int first_vector, int n, double *ch, double *a)
{
  if (!chan_span(cfg, "channel_get_taps", first_vector, n)) return -1;
  NEED_INIT(-1);
  const size_t np = (size_t)cfg->nb_tx * cfg->nb_rx, cw = np * cfg->m.info.channel_length * 2, aw = np * cfg->m.info.nb_taps * 2;
  HCK(hipDeviceSynchronize(), -1);
  if (ch) HCK(hipMemcpy(ch, cfg->ch.get() + first_vector * cw, (size_t)n * cw * sizeof(double), hipMemcpyDeviceToHost), -1);
  if (a) HCK(hipMemcpy(a, cfg->a.get() + first_vector * aw, (size_t)n * aw * sizeof(double), hipMemcpyDeviceToHost), -1);
  return 0;
}

/* the layout checks both forms share: every sample a segment holds must lie inside it */
static bool mp_layout_ok(const char *who, const oai4g_channel_config_t *cfg, uint32_t length, uint32_t seg_len, size_t seg_stride)
{
  if (length == 0 || seg_len == 0 || (length > seg_len && seg_stride == 0)) {
    set_err("%s: %u samples in segments of %u, %zu apart", who, length, seg_len, seg_stride);
    return false;
  }
  (void)cfg;
  return true;
}

extern "C" int oai4g_multipath_batch(oai4g_channel_config_t *cfg, int n, const int32_t *d_tx, size_t tx_stride, size_t tx_ant_stride,
                                     uint32_t tx_len, const int32_t *d_tail, uint32_t tail_len, int32_t *d_rx, size_t rx_stride,
                                     size_t rx_ant_stride, uint32_t seg_len, size_t seg_stride, const int32_t *d_tx_lev,
                                     double offset_db, uint64_t seed, uint32_t first_vector, void *stream)
{
  if (!cfg || n < 0 || (uint32_t)n > cfg->n_vectors || n > 65535) {
    set_err("multipath_batch: %d vectors of a configuration for %u (at most 65535 a call)", n, cfg ? cfg->n_vectors : 0u);
    return -1;
  }
  if (n > 0 && (!d_tx || !d_rx || !d_tx_lev || (tail_len && !d_tail) || (uint64_t)tx_len + tail_len > 0x7FFFFFFFull)) {
    set_err("multipath_batch: null array, or more than 2^31 - 1 samples");
    return -1;
  }
  if (!mp_layout_ok("multipath_batch", cfg, tx_len + tail_len, seg_len, seg_stride)) return -1;
  NEED_INIT(-1);
  multipath_args_t a;
  memset(&a, 0, sizeof(a));
  a.nb_tx = cfg->nb_tx;
  a.nb_rx = cfg->nb_rx;
  a.channel_length = cfg->m.info.channel_length;
  a.dd = cfg->dd;
  a.tx_len = tx_len;
  a.tail_len = tail_len;
  a.seg_len = seg_len;
  a.tx_stride = tx_stride;
  a.tx_ant_stride = tx_ant_stride;
  a.rx_stride = rx_stride;
  a.rx_ant_stride = rx_ant_stride;
  a.seg_stride = seg_stride;
  /* four samples in one 16-byte store where no group of four can straddle a segment or leave the alignment */
  a.vec4 = ((tx_len + tail_len) % 4 == 0 && seg_len % 4 == 0 && rx_stride % 4 == 0 && rx_ant_stride % 4 == 0 && seg_stride % 4 == 0 &&
            (uintptr_t)d_rx % 16 == 0) ? 1u : 0u;
  a.tx = d_tx;
  a.tail = d_tail;
  a.rx = d_rx;
  a.ch = cfg->ch.get();
  a.path_loss = cfg->path_loss;
  a.offset_db = offset_db;
  a.tx_lev = d_tx_lev;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.vec0 = first_vector;
  HCK(oai4g_launch_multipath(a, n, false, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_random_channel(oai4g_channel_config_t *cfg)
{
  if (!cfg) { set_err("random_channel: null configuration"); return -1; }
  NEED_INIT(-1);
  if (oai4g_channel_random_batch(cfg, 1, 0, 0, cfg->calls, nullptr, g_scr.s) != 0) return -1;
  cfg->calls++;
  HCK(hipStreamSynchronize(g_scr.s), -1);
  return 0;
}

extern "C" int oai4g_multipath_channel(oai4g_channel_config_t *cfg, double **tx_sig_re, double **tx_sig_im, double **rx_sig_re,
                                       double **rx_sig_im, uint32_t length, uint8_t keep_channel)
{
  if (!cfg || !tx_sig_re || !tx_sig_im || !rx_sig_re || !rx_sig_im || length == 0 || length > 0x7FFFFFFFu) {
    set_err("multipath_channel: null argument or length %u", length);
    return -1;
  }
  for (uint32_t j = 0; j < cfg->nb_tx; j++)
    if (!tx_sig_re[j] || !tx_sig_im[j]) { set_err("multipath_channel: null tx_sig[%u]", j); return -1; }
  for (uint32_t i = 0; i < cfg->nb_rx; i++)
    if (!rx_sig_re[i] || !rx_sig_im[i]) { set_err("multipath_channel: null rx_sig[%u]", i); return -1; }
  NEED_INIT(-1);
  if (!keep_channel && oai4g_random_channel(cfg) != 0) return -1;
  if (length <= cfg->dd) return 0;                          /* the reference's loop does not run */
  /* [antenna][length][re, im] on both sides */
  const size_t plane = (size_t)length * 2;
  std::vector<double> h((size_t)std::max(cfg->nb_tx, cfg->nb_rx) * plane);
  for (uint32_t j = 0; j < cfg->nb_tx; j++)
    for (size_t i = 0; i < length; i++) {
      h[j * plane + 2 * i] = tx_sig_re[j][i];
      h[j * plane + 2 * i + 1] = tx_sig_im[j][i];
    }
  stage_t st("multipath_channel");
  const int r_tx = st.add(cfg->nb_tx * plane * sizeof(double)), r_rx = st.add(cfg->nb_rx * plane * sizeof(double));
  if (!st.open()) return -1;
  HCK(st.up(r_tx, h.data(), cfg->nb_tx * plane * sizeof(double)), -1);
  multipath_args_t a;
  memset(&a, 0, sizeof(a));
  a.nb_tx = cfg->nb_tx;
  a.nb_rx = cfg->nb_rx;
  a.channel_length = cfg->m.info.channel_length;
  a.dd = cfg->dd;
  a.tx_len = length;
  a.seg_len = length;
  a.tx_ant_stride = length;
  a.rx_ant_stride = length;
  a.tx = st.ptr(r_tx);
  a.rx = st.ptr(r_rx);
  a.ch = cfg->ch.get();
  a.path_loss = cfg->path_loss;
  HCK(oai4g_launch_multipath(a, 1, true, g_scr.s), -1);
  const size_t skip = (size_t)cfg->dd * 2 * sizeof(double);
  for (uint32_t i = 0; i < cfg->nb_rx; i++)
    HCK(st.down(&h[i * plane + 2 * cfg->dd], r_rx, plane * sizeof(double) - skip, i * plane * sizeof(double) + skip), -1);
  HCK(st.sync(), -1);
  for (uint32_t i = 0; i < cfg->nb_rx; i++)
    for (size_t k = cfg->dd; k < length; k++) {
      rx_sig_re[i][k] = h[i * plane + 2 * k];
      rx_sig_im[i][k] = h[i * plane + 2 * k + 1];
    }
  return 0;
}

/* ------------------------------------------------------------------------------------------
 * SC-FDMA: the PUSCH DFT sizes (PHY/TOOLS/lte_dfts.c:3510-16087), ulsch_modulation, lte_idft.
 * ---------------------------------------------------------------------------------------- */
/* dft<N>: the factor it splits off, the constant of its final mulhi_int16 and whether it calls its sub-transforms with
 * scale_flag 1, read from the code (dft192 = 4 x 48, dft324 = 3 x 108, dft600 = 2 x 300 ...), not from factorisation
 * rules.  Norms: dft_norm_table[1..15] for 24..300; entry 14, 16384 or ONE_OVER_SQRT2_Q15 above. */
namespace {
struct pusch_size_t {
  uint16_t N;
  uint8_t r, sub_scaled;
  int16_t norm;
};
const pusch_size_t k_pusch_sizes[] = {
    {24, 2, 1, 6689},    {36, 3, 1, 5461},    {48, 4, 1, 4729},    {60, 5, 1, 4230},    {72, 2, 1, 23170},   {96, 2, 0, 3344},
    {108, 3, 0, 3153},   {120, 2, 0, 2991},   {144, 3, 1, 18918},  {180, 3, 1, 18918},  {192, 4, 1, 16384},  {216, 3, 1, 18918},
    {240, 4, 1, 16384},  {288, 3, 1, 18918},  {300, 5, 1, 14654},  {324, 3, 1, 18918},  {360, 3, 1, 18918},  {384, 4, 1, 16384},
    {432, 4, 1, 16384},  {480, 4, 1, 16384},  {540, 3, 1, 18918},  {576, 3, 1, 18918},  {600, 2, 1, 23170},  {648, 3, 1, 18918},
    {720, 4, 1, 16384},  {864, 3, 1, 18918},  {900, 3, 1, 18918},  {960, 4, 1, 16384},  {972, 3, 1, 18918},  {1080, 3, 1, 18918},
    {1152, 4, 1, 16384}, {1200, 4, 1, 16384}};

const pusch_size_t *pusch_size(int32_t N)
{
  for (const pusch_size_t &e : k_pusch_sizes)
    if (e.N == N) return &e;
  return nullptr;
}

/* the plan of dft<Msc>(x, y, scale_flag) (leaf12: the 9459 product dft_lte and lte_idft put behind dft12) and its twiddles */
bool pusch_plan(const char *who, int32_t Msc, bool scale_flag, bool leaf12, oai4g_pusch_plan_t &pl, std::vector<int16_t> &tw)
{
  memset(&pl, 0, sizeof(pl));
  tw.clear();
  if (Msc == 768) { set_err("%s: Msc 768 (64 PRB): the reference has no dft768", who); return false; }
  if (Msc != 12 && !pusch_size(Msc)) { set_err("%s: Msc %d is not one of the reference's 33 PUSCH DFT sizes", who, Msc); return false; }
  pl.size = (uint16_t)Msc;
  pl.leaf_norm = (int16_t)(Msc == 12 && leaf12 ? 9459 : 0);
  bool scaled = scale_flag;
  for (int32_t N = Msc; N != 12;) {
    const pusch_size_t *e = pusch_size(N);
    const uint32_t l = pl.n_levels++, M = N / e->r;
    pl.radix[l] = e->r;
    pl.sub_size[l] = (uint16_t)M;
    pl.norm[l] = (int16_t)(scaled ? e->norm : 0);
    pl.tw_offset[l] = (uint32_t)tw.size() / 2;
    for (uint32_t q = 1; q < e->r; q++)
      for (uint32_t k = 1; k < M; k++) {
        const double th = 2.0 * M_PI * q * k / N, c = 32767.0 * cos(th), s = -32767.0 * sin(th);
        tw.push_back((int16_t)(N <= 300 ? trunc(c) : floor(c)));   /* the tables up to 300 truncate, the later ones floor */
        tw.push_back((int16_t)(N <= 300 ? trunc(s) : floor(s)));
      }
    scaled = e->sub_scaled != 0;
    N = (int32_t)M;
  }
  pl.n_twiddles = (uint32_t)tw.size() / 2;
  return true;
}

/* a plan as the kernels read it, with its twiddles on the device */
struct pusch_engine_t {
  pusch_plan_t p;
  dev_buf<uint2> tw;
};
uint32_t rcp32(uint32_t d) { return (uint32_t)((0x100000000ull + d - 1) / d); }

bool pusch_engine(const char *who, int32_t Msc, bool scale_flag, bool leaf12, pusch_engine_t &e)
{
  oai4g_pusch_plan_t pl;
  std::vector<int16_t> tw;
  if (!pusch_plan(who, Msc, scale_flag, leaf12, pl, tw)) return false;
  pusch_plan_t &p = e.p;
  memset(&p, 0, sizeof(p));
  p.N = pl.size;
  p.n_lvl = pl.n_levels;
  p.spw = p.N <= 24 ? 16 : p.N <= 48 ? 8 : p.N <= 108 ? 4 : p.N <= 240 ? 2 : 1;
  p.lds_sym = 2 * p.N + p.N / 12;
  p.leaf_norm = (uint32_t)pl.leaf_norm;
  for (uint32_t l = 0; l < p.n_lvl; l++) {
    p.radix[l] = pl.radix[l];
    p.M[l] = pl.sub_size[l];
    p.norm[l] = (uint32_t)pl.norm[l];
    p.tw_off[l] = pl.tw_offset[l];
    p.rcp_r[l] = rcp32(p.radix[l]);
    p.rcp_m1[l] = rcp32(p.M[l] - 1);
  }
  std::vector<uint2> dtw(std::max<size_t>(1, pl.n_twiddles));
  for (uint32_t i = 0; i < pl.n_twiddles; i++) {
    const uint16_t re = (uint16_t)tw[2 * i], im = (uint16_t)tw[2 * i + 1], nim = (uint16_t)(-(int32_t)tw[2 * i + 1]);
    dtw[i] = make_uint2((uint32_t)re | (uint32_t)nim << 16, (uint32_t)im | (uint32_t)re << 16);
  }
  if (e.tw.upload(dtw) != hipSuccess) { set_err("%s: twiddle upload failed", who); return false; }
  return true;
}

void pusch_data_symbols(uint32_t Ncp, bool mapping, uint32_t srs_active, uint32_t row, pusch_grid_t &g)
{
  memset(&g, 0, sizeof(g));
  g.nsymb = Ncp ? 12 : 14;
  g.row = row;
  const uint32_t p0 = Ncp ? 2 : 3, p1 = Ncp ? 8 : 10, last = g.nsymb - (mapping ? srs_active : 0);
  for (uint32_t l = 0; l < last; l++)
    if (l != p0 && l != p1) g.sym[g.n_data++] = l;
}
}  // namespace

extern "C" int oai4g_pusch_dft_plan(int32_t Msc, oai4g_pusch_plan_t *plan, int16_t *twiddles, uint32_t capacity)
{
  oai4g_pusch_plan_t pl;
  std::vector<int16_t> tw;
  if (!plan) { set_err("pusch_dft_plan: null plan"); return -1; }
  if (!pusch_plan("pusch_dft_plan", Msc, true, true, pl, tw)) return -1;
  if (twiddles && capacity < pl.n_twiddles) { set_err("pusch_dft_plan: %u twiddles do not fit %u", pl.n_twiddles, capacity); return -1; }
  *plan = pl;
  if (twiddles && !tw.empty()) memcpy(twiddles, tw.data(), tw.size() * sizeof(int16_t));
  return 0;
}

struct oai4g_pusch_config {
  oai4g_frame_parms_t fp;
  uint32_t Qm, G;
  pusch_engine_t eng;
  pusch_grid_t map_grid, idft_grid;
  pusch_mod_t mod;
  dev_buf<uint32_t> gold;                 /* [10][1 + (G >> 5)] */
};

/* what ulsch_modulation itself refuses, nothing written (ulsch_modulation.c:413-429): 1 with the error set */
static int pusch_ref_refusal(const char *who, uint32_t harq_pid, uint32_t first_rb, uint32_t nb_rb)
{
  if (harq_pid > 7) { set_err("%s: Illegal harq_pid %u", who, harq_pid); return 1; }
  if (nb_rb == 0) { set_err("%s: Illegal nb_rb 0", who); return 1; }
  if (first_rb > 25) { set_err("%s: Illegal first_rb %u", who, first_rb); return 1; }
  return 0;
}

/* everything of a configuration but the device: the checks, shared with the drop-in so that it refuses before it touches anything */
static bool pusch_config_ok(const char *who, const oai4g_frame_parms_t *fp, uint32_t first_rb, uint32_t nb_rb, uint32_t Qm,
                            uint32_t srs_active, uint32_t first_subframe, uint32_t subframe_step)
{
  if (!fp) { set_err("%s: null frame parameters", who); return false; }
  if (pusch_ref_refusal(who, 0, first_rb, nb_rb)) return false;
  oai4g_pusch_plan_t pl;
  std::vector<int16_t> tw;
  if (!pusch_plan(who, 12 * (int32_t)nb_rb, true, true, pl, tw)) return false;
  const uint32_t N = fp->ofdm_symbol_size;
  if (fp->N_RB_DL == 0 || N < 12u * fp->N_RB_DL || N > 2048 || fp->first_carrier_offset != N - 6u * fp->N_RB_DL || fp->Ncp > 1) {
    set_err("%s: frame parameters are not initialised (N_RB_DL %u, ofdm_symbol_size %u)", who, fp->N_RB_DL, N);
    return false;
  }
  if (first_rb + nb_rb > fp->N_RB_DL) { set_err("%s: first_rb %u + nb_rb %u leaves the band of %u PRB", who, first_rb, nb_rb, fp->N_RB_DL); return false; }
  if (Qm != 2 && Qm != 4 && Qm != 6) { set_err("%s: Qm %u", who, Qm); return false; }
  if (srs_active > 1) { set_err("%s: srs_active %u", who, srs_active); return false; }
  if (first_subframe > 9 || subframe_step > 9) { set_err("%s: subframe %u step %u", who, first_subframe, subframe_step); return false; }
  if (fp->first_carrier_offset + 12 * first_rb == N) {
    set_err("%s: first_carrier_offset + 12 first_rb == ofdm_symbol_size (first_rb %u): the reference's wrap test is '>' and it "
            "writes past the symbol here", who, first_rb);
    return false;
  }
  return true;
}

extern "C" oai4g_pusch_config_t *oai4g_pusch_config_create(const oai4g_frame_parms_t *fp, uint16_t first_rb, uint16_t nb_rb, uint8_t Qm,
                                                           uint8_t srs_active, uint16_t rnti, uint8_t first_subframe,
                                                           uint8_t subframe_step)
{
  const char *who = "pusch_config_create";
  if (!pusch_config_ok(who, fp, first_rb, nb_rb, Qm, srs_active, first_subframe, subframe_step)) return nullptr;
  NEED_INIT(nullptr);
  std::unique_ptr<oai4g_pusch_config_t> cfg(new oai4g_pusch_config_t);
  cfg->fp = *fp;
  cfg->Qm = Qm;
  if (!pusch_engine(who, 12 * nb_rb, true, true, cfg->eng)) return nullptr;
  const uint32_t N = fp->ofdm_symbol_size;
  pusch_data_symbols(fp->Ncp, true, srs_active, N, cfg->map_grid);
  pusch_data_symbols(fp->Ncp, false, 0, 12u * fp->N_RB_DL, cfg->idft_grid);
  cfg->G = 12u * nb_rb * Qm * cfg->map_grid.n_data;
  pusch_mod_t &m = cfg->mod;
  memset(&m, 0, sizeof(m));
  m.Qm = Qm;
  m.first_sf = first_subframe;
  m.sf_step = subframe_step;
  m.gold_words = 1 + (cfg->G >> 5);
  m.re_offset = fp->first_carrier_offset + 12u * first_rb;
  if (m.re_offset > N) m.re_offset -= N;
  std::vector<uint32_t> gold((size_t)10 * m.gold_words);
  for (uint32_t sf = 0; sf < 10; sf++) {
    uint32_t x1 = 0, x2 = ((uint32_t)rnti << 14) + (sf << 9) + fp->Nid_cell;     /* c_init, 36.211 5.3.1 */
    for (uint32_t w = 0; w < m.gold_words; w++) gold[(size_t)sf * m.gold_words + w] = oai4g_lte_gold_generic(&x1, &x2, w == 0);
  }
  HCK(cfg->gold.upload(gold), nullptr);
  return cfg.release();
}

extern "C" void oai4g_pusch_config_destroy(oai4g_pusch_config_t *cfg) { delete cfg; }

extern "C" int oai4g_pusch_mod_batch(oai4g_pusch_config_t *cfg, int n_sf, const uint8_t *d_h, size_t h_stride, int16_t amp,
                                     int32_t *d_txdataF, void *stream)
{
  if (!cfg || n_sf < 0 || (n_sf > 0 && (!d_h || !d_txdataF))) { set_err("pusch_mod_batch: bad arguments"); return -1; }
  if (h_stride < cfg->G || h_stride > 0xFFFFFFFFu) { set_err("pusch_mod_batch: h_stride %zu is less than G = %u", h_stride, cfg->G); return -1; }
  NEED_INIT(-1);
  pusch_mod_t m = cfg->mod;
  m.h_stride = (uint32_t)h_stride;
  m.amp = amp;
  m.gain_qpsk = (int16_t)((amp * 23170) >> 15);          /* gain_lin_QPSK = (amp * ONE_OVER_SQRT2_Q15) >> 15 */
  HCK(oai4g_launch_pusch_mod(cfg->eng.p, cfg->eng.tw.get(), cfg->map_grid, m, d_h, cfg->gold.get(), (uint32_t *)d_txdataF,
                             (uint32_t)n_sf, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_pusch_dft_batch(oai4g_pusch_config_t *cfg, int n_sf, const int32_t *d_d, int32_t *d_z, void *stream)
{
  if (!cfg || n_sf < 0 || (n_sf > 0 && (!d_d || !d_z))) { set_err("pusch_dft_batch: bad arguments"); return -1; }
  NEED_INIT(-1);
  HCK(oai4g_launch_pusch_dft(cfg->eng.p, cfg->eng.tw.get(), (const uint32_t *)d_d, (uint32_t *)d_z,
                             (uint32_t)n_sf * cfg->map_grid.n_data, (hipStream_t)stream), -1);
  return 0;
}

extern "C" int oai4g_pusch_idft_batch(oai4g_pusch_config_t *cfg, int n_sf, int32_t *d_comp, void *stream)
{
  if (!cfg || n_sf < 0 || (n_sf > 0 && !d_comp)) { set_err("pusch_idft_batch: bad arguments"); return -1; }
  NEED_INIT(-1);
  HCK(oai4g_launch_pusch_idft(cfg->eng.p, cfg->eng.tw.get(), cfg->idft_grid, (uint32_t *)d_comp, (uint32_t)n_sf, (hipStream_t)stream), -1);
  return 0;
}

/* n transforms of Msc on host samples through k_pusch_dft */
static int pusch_dft_host(const char *who, int32_t Msc, bool scale_flag, bool leaf12, const void *x, void *y, uint32_t n)
{
  if (!x || !y) { set_err("%s: null buffer", who); return -1; }
  oai4g_pusch_plan_t pl;
  std::vector<int16_t> tw;
  if (!pusch_plan(who, Msc, scale_flag, leaf12, pl, tw)) return -1;       /* refuse before the device is touched */
  if (n == 0) return 0;
  NEED_INIT(-1);
  pusch_engine_t eng;
  if (!pusch_engine(who, Msc, scale_flag, leaf12, eng)) return -1;
  const size_t bytes = (size_t)n * Msc * 4;
  stage_t st(who);
  const int r_in = st.add(bytes), r_out = st.add(bytes);
  if (!st.open()) return -1;
  HCK(st.up(r_in, x, bytes), -1);
  HCK(oai4g_launch_pusch_dft(eng.p, eng.tw.get(), st.ptr<uint32_t>(r_in), st.ptr<uint32_t>(r_out), n, g_scr.s), -1);
  HCK(st.down(y, r_out, bytes), -1);
  HCK(st.sync(), -1);
  return 0;
}

extern "C" int oai4g_dft_lte(int32_t *z, const int32_t *d, int32_t Msc_PUSCH, uint8_t Nsymb)
{
  if (Nsymb > 12) { set_err("dft_lte: Nsymb %u (at most 12 columns)", Nsymb); return -1; }
  return pusch_dft_host("dft_lte", Msc_PUSCH, true, true, d, z, Nsymb);
}

extern "C" int oai4g_pusch_dft(int32_t Msc, const int16_t *x, int16_t *y, uint8_t scale_flag)
{
  return pusch_dft_host("pusch_dft", Msc, scale_flag == 1, false, x, y, 1);
}

extern "C" int oai4g_lte_idft(const oai4g_frame_parms_t *fp, int32_t *z, uint16_t Msc_PUSCH)
{
  const char *who = "lte_idft";
  if (!fp || !z) { set_err("%s: null argument", who); return -1; }
  oai4g_pusch_plan_t pl;
  std::vector<int16_t> tw;
  if (!pusch_plan(who, Msc_PUSCH, true, true, pl, tw)) return -1;
  if (fp->N_RB_DL == 0 || fp->N_RB_DL > 110 || Msc_PUSCH > 12u * fp->N_RB_DL || fp->Ncp > 1) {
    set_err("%s: Msc %u does not fit N_RB_DL %u", who, Msc_PUSCH, fp->N_RB_DL);
    return -1;
  }
  NEED_INIT(-1);
  pusch_engine_t eng;
  if (!pusch_engine(who, Msc_PUSCH, true, true, eng)) return -1;
  pusch_grid_t g;
  pusch_data_symbols(fp->Ncp, false, 0, 12u * fp->N_RB_DL, g);
  const size_t bytes = (size_t)g.nsymb * g.row * 4;
  stage_t st(who);
  const int r = st.add(bytes);
  if (!st.open()) return -1;
  HCK(st.up(r, z, bytes), -1);
  HCK(oai4g_launch_pusch_idft(eng.p, eng.tw.get(), g, st.ptr<uint32_t>(r), 1, g_scr.s), -1);
  HCK(st.down(z, r, bytes), -1);
  HCK(st.sync(), -1);
  return 0;
}

extern "C" int oai4g_ulsch_modulation(int32_t *const *txdataF, int16_t amp, uint32_t frame, uint32_t subframe,
                                      const oai4g_frame_parms_t *fp, const oai4g_ue_ulsch_t *ulsch)
{
  const char *who = "ulsch_modulation";
  (void)frame;
  if (!fp || !ulsch) { set_err("%s: Null ulsch or frame parameters", who); return -1; }
  if (ulsch->harq_pid > 7) return pusch_ref_refusal(who, ulsch->harq_pid, 0, 1);
  const oai4g_ul_harq_t *hp = ulsch->harq_processes[ulsch->harq_pid];
  if (!hp) { set_err("%s: null harq process %u", who, ulsch->harq_pid); return -1; }
  if (int r = pusch_ref_refusal(who, ulsch->harq_pid, hp->first_rb, hp->nb_rb)) return r;
  if (ulsch->cooperation_flag == 2) { set_err("%s: cooperation_flag 2 (distributed Alamouti) is not supported", who); return -1; }
  if (subframe > 9) { set_err("%s: subframe %u", who, subframe); return -1; }
  const uint8_t Qm = oai4g_get_Qm_ul(hp->mcs);
  if (!pusch_config_ok(who, fp, hp->first_rb, hp->nb_rb, Qm, ulsch->srs_active, subframe, 0)) return -1;
  const uint32_t nsymb = fp->Ncp ? 12 : 14;
  if (ulsch->Nsymb_pusch != nsymb - 2 - ulsch->srs_active) {
    set_err("%s: Nsymb_pusch %u, but the mapping takes %u symbols", who, ulsch->Nsymb_pusch, nsymb - 2 - ulsch->srs_active);
    return -1;
  }
  if (!txdataF || !txdataF[0] || !ulsch->h) { set_err("%s: null txdataF or h", who); return -1; }
  std::unique_ptr<oai4g_pusch_config_t, void (*)(oai4g_pusch_config_t *)> cfg(
      oai4g_pusch_config_create(fp, hp->first_rb, hp->nb_rb, Qm, ulsch->srs_active, ulsch->rnti, (uint8_t)subframe, 0),
      oai4g_pusch_config_destroy);
  if (!cfg) return -1;
  const size_t gb = (size_t)nsymb * fp->ofdm_symbol_size * 4;
  int32_t *sub = txdataF[0] + (size_t)subframe * nsymb * fp->ofdm_symbol_size;
  stage_t st(who);
  const int r_h = st.add(cfg->G), r_g = st.add(gb);
  if (!st.open()) return -1;
  HCK(st.up(r_h, ulsch->h, cfg->G), -1);
  HCK(st.up(r_g, sub, gb), -1);
  if (oai4g_pusch_mod_batch(cfg.get(), 1, st.ptr<uint8_t>(r_h), cfg->G, amp, st.ptr<int32_t>(r_g), g_scr.s) != 0) return -1;
  HCK(st.down(sub, r_g, gb), -1);
  HCK(st.sync(), -1);
  return 0;
}
