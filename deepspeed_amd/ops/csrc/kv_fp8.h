// Device helpers shared by the fp8 (OCP e4m3fn) KV slot-pool kernels:
// ragged_rope_append_fp8 / ragged_decode_fp8 / ragged_prefill_fp8.
//
// Pool format, per layer: codes [B,Smax,Hk,D] e4m3fn plus one fp32 scale per
// (slot, position, kv head) row, [B,Smax,Hk]. A row x[0..D) of bf16 values is
// stored as
//   amax  = max |x[d]|                      (exact)
//   scale = amax > 0 ? amax / 448 : 1       (fp32, correctly rounded)
//   inv   = 1 / scale                       (fp32, correctly rounded)
//   code  = e4m3fn_rne(clamp(x[d] * inv, -448, 448))
// and reads back as float(code) * scale. ops/functional.py kv_quantize is the
// same composition in torch; the append kernel matches it bit for bit.
#pragma once

#include "common.h"

namespace kvfp8 {

using bf16x8_t = __attribute__((ext_vector_type(8))) short;

constexpr float FP8_MAX = 448.f;

// 4 floats -> 4 e4m3fn codes in one dword; clamp to +-448 first (x * inv can
// round just above 448). NaN bypasses the clamp and becomes the NaN code.
DEV_INLINE unsigned int pack4(float a, float b, float c, float d) {
  a = (a != a) ? a : fminf(fmaxf(a, -FP8_MAX), FP8_MAX);
  b = (b != b) ? b : fminf(fmaxf(b, -FP8_MAX), FP8_MAX);
  c = (c != c) ? c : fminf(fmaxf(c, -FP8_MAX), FP8_MAX);
  d = (d != d) ? d : fminf(fmaxf(d, -FP8_MAX), FP8_MAX);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  return (unsigned int)__builtin_amdgcn_cvt_pk_fp8_f32(c, d, lo, true);
}

// 4 codes (one dword) -> 4 floats, exact
DEV_INLINE void unpack4(unsigned int w, float* __restrict__ f) {
  auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}

DEV_INLINE void unpack8(uint2 c, float* __restrict__ f) {
  unpack4(c.x, f);
  unpack4(c.y, f + 4);
}

// 8 codes -> 8 bf16. Every e4m3 value (3 mantissa bits, subnormals included)
// is exactly a bf16, so the top half of its fp32 pattern is that bf16.
DEV_INLINE bf16x8_t widen8(uint2 c) {
  float f[8];
  unpack8(c, f);
  bf16x8_t r;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    r[j] = (short)(__builtin_bit_cast(unsigned int, f[j]) >> 16);
  return r;
}

}  // namespace kvfp8
