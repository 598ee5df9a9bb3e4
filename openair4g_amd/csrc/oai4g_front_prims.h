/*
 * Per-RE arithmetic shared by the UE control front ends (oai4g_pdcch_front.hip, oai4g_pbch_front.hip): the
 * reference's SSE steps of pdcch_ / pbch_channel_level, _channel_compensation and _detection_mrc on one word.
 */
#pragma once
#include <stdint.h>

typedef short pf_short2 __attribute__((ext_vector_type(2)));

/* a.x b.x + a.y b.y on the int16 halves, 32-bit wrap (_mm_madd_epi16) */
static __device__ __forceinline__ int32_t pf_madd(uint32_t a, uint32_t b)
{
#if __has_builtin(__builtin_amdgcn_sdot2)
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(pf_short2, a), __builtin_bit_cast(pf_short2, b), 0, false);
#else
  return (int32_t)((uint32_t)((int32_t)(int16_t)a * (int16_t)b) + (uint32_t)((int32_t)(int16_t)(a >> 16) * (int16_t)(b >> 16)));
#endif
}

static __device__ __forceinline__ uint32_t pf_sat16(int32_t v)
{
  return (uint32_t)(uint16_t)(int16_t)(v > 32767 ? 32767 : (v < -32768 ? -32768 : v));
}

/* pdcch_channel_compensation on one RE: (conj(h) y) >> shift, packs_epi32.  The imaginary part multiplies by
 * (-h.im, h.re), the negation in int16 (sign_epi16: -(-32768) stays -32768) */
static __device__ __forceinline__ uint32_t pf_comp(uint32_t h, uint32_t y, uint32_t shift)
{
  const uint32_t hc = (uint32_t)(uint16_t)(int16_t)(-(int32_t)(int16_t)(h >> 16)) | (h << 16);
  return pf_sat16(pf_madd(h, y) >> shift) | (pf_sat16(pf_madd(hc, y) >> shift) << 16);
}

/* pdcch_detection_mrc on one RE: adds_epi16(a >> 1, b >> 1) per component */
static __device__ __forceinline__ uint32_t pf_mrc(uint32_t a, uint32_t b)
{
  const int32_t re = ((int32_t)(int16_t)a >> 1) + ((int32_t)(int16_t)b >> 1);
  const int32_t im = ((int32_t)(int16_t)(a >> 16) >> 1) + ((int32_t)(int16_t)(b >> 16) >> 1);
  return pf_sat16(re) | (pf_sat16(im) << 16);
}
