/* Rate-matching geometry of lte_rate_matching.c (lte_rate_matching_turbo :464-566 and
 * lte_rate_matching_turbo_rx :688-745), stated once for the transmit and the receive side of the host
 * layer.  Plain C++ without a HIP include: tests/test_rm_geom_cpu.py compiles it alone. */
#ifndef OAI4G_RM_GEOM_H
#define OAI4G_RM_GEOM_H
#include <stdint.h>

/* The circular buffer of one of C code blocks with RTC interleaver rows: Kw = 3 Kpi entries of w, of
 * which the soft-buffer share Nir / C keeps the first Ncb.  `shorter` (Ncb < Kw) is the reference's
 * "RM condition": it prints, and its rate matcher returns E = 0. */
struct rm_ncb_t {
  uint32_t Nir, Kw, Ncb;
  bool shorter;
};

static inline rm_ncb_t rm_ncb(uint32_t Nsoft, uint32_t Kmimo, uint32_t Mdlharq, uint32_t C, uint32_t RTC)
{
  rm_ncb_t g;
  g.Nir = Nsoft / Kmimo / (Mdlharq < 8 ? Mdlharq : 8);
  g.Kw = 3 * (RTC << 5);
  g.Ncb = g.Nir / C < g.Kw ? g.Nir / C : g.Kw;
  g.shorter = g.Ncb < g.Kw;
  return g;
}

/* start of redundancy version rv in w: k0 = R (2 + rv ceil(Ncb / 8R) 2) */
static inline uint32_t rm_k0(uint32_t RTC, uint32_t Ncb, uint32_t rv)
{
  const uint32_t ncol8 = RTC << 3;
  return RTC * (2 + rv * ((Ncb % ncol8 ? 1 : 0) + Ncb / ncol8) * 2);
}

/* e entries of block r of C: of the G' = G / (Nl Qm) symbols, blocks 0 .. rm_esplit - 1 carry
 * floor(G' / C) each and the G' mod C blocks after them one more */
static inline uint32_t rm_esplit(uint32_t G, uint32_t Nl, uint32_t Qm, uint32_t C) { return C - G / Nl / Qm % C; }

static inline uint32_t rm_E(uint32_t G, uint32_t Nl, uint32_t Qm, uint32_t C, uint32_t r)
{
  return Nl * Qm * (G / Nl / Qm / C + (r < rm_esplit(G, Nl, Qm, C) ? 0 : 1));
}

/* The circular selection skips the <NULL> entries of w, so it runs over the compacted buffer: the
 * entries of w[0..x) that are not <NULL>.  x = Ncb gives its length Nnn, x = k0 its start k0c.
 * `nulls_below(x)` is the number of <NULL>s in w[0..x), from either representation below; what a
 * caller does with k0 >= Ncb (the limited-buffer extension only) is the caller's rule. */
template <typename NullsBelow>
static inline uint32_t rm_compact(uint32_t x, const NullsBelow &nulls_below)
{
  return x - nulls_below(x);
}

/* the <NULL> positions as a list (the transmit side's cw_dev_t::nullpos) */
struct rm_null_list {
  const uint16_t *pos;
  uint32_t n;
  uint32_t operator()(uint32_t x) const
  {
    uint32_t below = 0;
    for (uint32_t i = 0; i < n; i++) below += pos[i] < x ? 1u : 0u;
    return below;
  }
};

/* the <NULL> positions as generate_dummy_w's mask (the receive side): w[q] == mark for q < x */
struct rm_null_mask {
  const uint8_t *w;
  uint8_t mark;
  uint32_t operator()(uint32_t x) const
  {
    uint32_t below = 0;
    for (uint32_t q = 0; q < x; q++) below += w[q] == mark ? 1u : 0u;
    return below;
  }
};

#endif
