// Fused ragged RoPE + quantizing KV-append into the fp8 slot pool (gfx950).
//
// Same contract as ragged_rope_append (ragged_rope_append.hip): q_rot comes
// back in bf16, a token whose slot / position is out of range is skipped
// (no code, no scale, no lens write; q_rot row 0) and the last token of each
// sequence sets lens[slot]. The K and V rows are written as e4m3fn codes plus
// one fp32 scale per (slot, position, kv head), format in kv_fp8.h. K is
// rotated and rounded to bf16 exactly as the bf16 kernel stores it, and that
// bf16 row is what gets quantized.
//
// Work item = (token, head, 8-pair group) as in the bf16 kernel, so a lane
// holds 16 values of a row and the D/16 lanes of a row (8 at D = 128, 4 at
// D = 64) are adjacent and aligned in the wave: the row amax is a sub-wave
// __shfl_xor butterfly on the |bf16| bit patterns, no LDS. Each lane packs
// its 2 x 8 codes with v_cvt_pk_fp8_f32 and stores two 8-byte vectors.
#include <torch/extension.h>

#include <climits>

#include "kv_fp8.h"

namespace rrafp8 {

DEV_INLINE bool tok_ok(long long slot, long long pos, int B, int Smax,
                       int P) {
  return slot >= 0 && slot < B && pos >= 0 && pos < Smax && pos < P;
}

DEV_INLINE void write_len(int64_t* __restrict__ lens,
                          const int64_t* __restrict__ tok_slot, long long t,
                          int T, long long slot, long long pos) {
  if (lens == nullptr) return;
  if (t == T - 1 || tok_slot[t + 1] != slot) lens[slot] = pos + 1;
}

// the rotation of ragged_rope_append's rotate8, result kept in registers
DEV_INLINE void rotate8(bf16x8& o1, bf16x8& o2,
                        const short* __restrict__ src,
                        const float* __restrict__ crow,
                        const float* __restrict__ srow, int half) {
  bf16x8 x1 = *reinterpret_cast<const bf16x8*>(src);
  bf16x8 x2 = *reinterpret_cast<const bf16x8*>(src + half);
  f32x4 c0 = *reinterpret_cast<const f32x4*>(crow);
  f32x4 c1 = *reinterpret_cast<const f32x4*>(crow + 4);
  f32x4 s0 = *reinterpret_cast<const f32x4*>(srow);
  f32x4 s1 = *reinterpret_cast<const f32x4*>(srow + 4);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float c = (j < 4 ? c0.v[j] : c1.v[j - 4]);
    float sv = (j < 4 ? s0.v[j] : s1.v[j - 4]);
    float a = bf2f(x1.v[j]);
    float b = bf2f(x2.v[j]);
    o1.v[j] = f2bf(a * c - b * sv);
    o2.v[j] = f2bf(b * c + a * sv);
  }
}

DEV_INLINE uint2 quant8(const bf16x8& x, float inv) {
  uint2 w;
  w.x = kvfp8::pack4(bf2f(x.v[0]) * inv, bf2f(x.v[1]) * inv,
                     bf2f(x.v[2]) * inv, bf2f(x.v[3]) * inv);
  w.y = kvfp8::pack4(bf2f(x.v[4]) * inv, bf2f(x.v[5]) * inv,
                     bf2f(x.v[6]) * inv, bf2f(x.v[7]) * inv);
  return w;
}

// q [T,Hq,D], k/v [T,Hk,D], q_rot [T,Hq,D] bf16; kpool/vpool [B,Smax,Hk,D]
// e4m3fn bytes; kscale/vscale [B,Smax,Hk] fp32; cs/sn [P, D/2] fp32;
// tok_slot/tok_pos [T] i64; lens [B] i64 or null.
// total = T * (Hq + 2*Hk) * (D/16), a multiple of the D/16 lanes of a row,
// and a block's first item is too, so a row's lanes enter and leave the loop
// and every branch below together.
template <int D>
__global__ void ragged_rope_append_fp8_kernel(
    short* __restrict__ q_rot, const short* __restrict__ q,
    const short* __restrict__ k, const short* __restrict__ v,
    const float* __restrict__ cs, const float* __restrict__ sn,
    const int64_t* __restrict__ tok_slot,
    const int64_t* __restrict__ tok_pos, unsigned char* __restrict__ kpool,
    unsigned char* __restrict__ vpool, float* __restrict__ kscale,
    float* __restrict__ vscale, int64_t* __restrict__ lens, long long total,
    int T, int Hq, int Hk, int B, int Smax, int P) {
  constexpr int half = D / 2;
  constexpr int half8 = half / 8;  // lanes per row: 8 (D=128) or 4 (D=64)
  const int heads = Hq + 2 * Hk;
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < total; i += stride) {
    const int d8 = (int)(i % half8);
    const long long rem = i / half8;
    const int hh = (int)(rem % heads);
    const long long t = rem / heads;
    const long long slot = tok_slot[t];
    const long long pos = tok_pos[t];
    const bool ok = tok_ok(slot, pos, B, Smax, P);
    const int off = d8 * 8;
    if (hh < Hq) {
      const long long base = (t * Hq + hh) * D + off;
      bf16x8 o1, o2;
      if (!ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o1.v[j] = o2.v[j] = 0;
      } else {
        if (hh == 0 && d8 == 0) write_len(lens, tok_slot, t, T, slot, pos);
        rotate8(o1, o2, q + base, cs + pos * half + off,
                sn + pos * half + off, half);
      }
      *reinterpret_cast<bf16x8*>(q_rot + base) = o1;
      *reinterpret_cast<bf16x8*>(q_rot + base + half) = o2;
      continue;
    }
    if (!ok) continue;
    const bool is_k = hh < Hq + Hk;
    const int hk = is_k ? hh - Hq : hh - Hq - Hk;
    const long long src = (t * Hk + hk) * D + off;
    const long long row = (slot * Smax + pos) * Hk + hk;
    bf16x8 x1, x2;
    if (is_k) {
      rotate8(x1, x2, k + src, cs + pos * half + off, sn + pos * half + off,
              half);
    } else {
      x1 = *reinterpret_cast<const bf16x8*>(v + src);
      x2 = *reinterpret_cast<const bf16x8*>(v + src + half);
    }
    // row amax on the |bf16| bit patterns (integer order = float order)
    unsigned int m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      m = max(m, (unsigned int)(x1.v[j] & 0x7fff));
      m = max(m, (unsigned int)(x2.v[j] & 0x7fff));
    }
#pragma unroll
    for (int o = half8 / 2; o > 0; o >>= 1)
      m = max(m, (unsigned int)__shfl_xor((int)m, o, WAVE));
    const float amax = bf2f((short)m);
    const float scale = amax > 0.f ? amax / kvfp8::FP8_MAX : 1.f;
    const float inv = 1.f / scale;
    unsigned char* dst = (is_k ? kpool : vpool) + row * D + off;
    *reinterpret_cast<uint2*>(dst) = quant8(x1, inv);
    *reinterpret_cast<uint2*>(dst + half) = quant8(x2, inv);
    if (d8 == 0) (is_k ? kscale : vscale)[row] = scale;
  }
}

}  // namespace rrafp8

at::Tensor ragged_rope_append_fp8(at::Tensor q, at::Tensor k, at::Tensor v,
                                  at::Tensor cos, at::Tensor sin,
                                  at::Tensor tok_slot, at::Tensor tok_pos,
                                  at::Tensor kpool, at::Tensor vpool,
                                  at::Tensor k_scale, at::Tensor v_scale,
                                  c10::optional<at::Tensor> lens) {
  CHECK_ARG(q, at::kBFloat16);
  CHECK_ARG(k, at::kBFloat16);
  CHECK_ARG(v, at::kBFloat16);
  CHECK_ARG(cos, at::kFloat);
  CHECK_ARG(sin, at::kFloat);
  CHECK_ARG(tok_slot, at::kLong);
  CHECK_ARG(tok_pos, at::kLong);
  CHECK_ARG(kpool, at::kFloat8_e4m3fn);
  CHECK_ARG(vpool, at::kFloat8_e4m3fn);
  CHECK_ARG(k_scale, at::kFloat);
  CHECK_ARG(v_scale, at::kFloat);
  CHECK_ON(k, q);
  CHECK_ON(v, q);
  CHECK_ON(cos, q);
  CHECK_ON(sin, q);
  CHECK_ON(tok_slot, q);
  CHECK_ON(tok_pos, q);
  CHECK_ON(kpool, q);
  CHECK_ON(vpool, q);
  CHECK_ON(k_scale, q);
  CHECK_ON(v_scale, q);
  TORCH_CHECK(q.dim() == 3, "ragged_rope_append_fp8: q must be [T,Hq,D]");
  TORCH_CHECK(k.dim() == 3 && v.sizes() == k.sizes(),
              "ragged_rope_append_fp8: k and v must both be [T,Hk,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(),
              "ragged_rope_append_fp8: kpool and vpool must both be "
              "[B,Smax,Hk,D]");
  const long T = q.size(0), Hq = q.size(1), D = q.size(2);
  const long Hk = k.size(1);
  const long B = kpool.size(0), Smax = kpool.size(1);
  TORCH_CHECK(D == 64 || D == 128,
              "ragged_rope_append_fp8: head_dim must be 64 or 128, got ", D);
  TORCH_CHECK(k.size(0) == T && k.size(2) == D,
              "ragged_rope_append_fp8: k/v must have q's token count and "
              "head_dim");
  TORCH_CHECK(Hk >= 1 && Hq >= 1 && Hq % Hk == 0,
              "ragged_rope_append_fp8: Hq % Hk != 0");
  TORCH_CHECK(kpool.size(2) == Hk && kpool.size(3) == D,
              "ragged_rope_append_fp8: pool heads/head_dim != k "
              "heads/head_dim");
  TORCH_CHECK(k_scale.dim() == 3 && k_scale.size(0) == B &&
                  k_scale.size(1) == Smax && k_scale.size(2) == Hk &&
                  v_scale.sizes() == k_scale.sizes(),
              "ragged_rope_append_fp8: k_scale and v_scale must both be "
              "[B,Smax,Hk]");
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == D / 2 &&
                  sin.sizes() == cos.sizes(),
              "ragged_rope_append_fp8: cos and sin must both be [P, D/2]");
  const long P = cos.size(0);
  TORCH_CHECK(P >= Smax, "ragged_rope_append_fp8: table rows P ", P,
              " < pool Smax ", Smax);
  TORCH_CHECK(tok_slot.dim() == 1 && tok_slot.size(0) == T &&
                  tok_pos.dim() == 1 && tok_pos.size(0) == T,
              "ragged_rope_append_fp8: tok_slot and tok_pos must be [T]");
  int64_t* lens_ptr = nullptr;
  if (lens.has_value()) {
    const at::Tensor& lens_t = *lens;
    CHECK_ARG(lens_t, at::kLong);
    CHECK_ON(lens_t, q);
    TORCH_CHECK(lens_t.dim() == 1 && lens_t.size(0) == B,
                "ragged_rope_append_fp8: lens must be [B]");
    lens_ptr = lens_t.data_ptr<int64_t>();
  }
  TORCH_CHECK(T <= INT_MAX && B <= INT_MAX && Smax <= INT_MAX &&
                  P <= INT_MAX && Hq + 2 * Hk <= INT_MAX,
              "ragged_rope_append_fp8: a dimension exceeds int32");

  auto q_rot = at::empty_like(q);
  if (T == 0) return q_rot;
  TORCH_CHECK(B >= 1 && Smax >= 1, "ragged_rope_append_fp8: empty pool");
  TORCH_CHECK(ptr_aligned(q.data_ptr(), 16) && ptr_aligned(k.data_ptr(), 16) &&
                  ptr_aligned(v.data_ptr(), 16) &&
                  ptr_aligned(q_rot.data_ptr(), 16) &&
                  ptr_aligned(cos.data_ptr(), 16) &&
                  ptr_aligned(sin.data_ptr(), 16) &&
                  ptr_aligned(kpool.data_ptr(), 8) &&
                  ptr_aligned(vpool.data_ptr(), 8),
              "ragged_rope_append_fp8: q/k/v/cos/sin must be 16-byte and the "
              "pools 8-byte aligned");

  auto stream = c10::hip::getCurrentHIPStream();
  const int block = 256;
  const long long total = (long long)T * (Hq + 2 * Hk) * (D / 16);
  const int grid = grid_for(total, block);
#define LAUNCH(DD)                                                          \
  hipLaunchKernelGGL(rrafp8::ragged_rope_append_fp8_kernel<DD>, dim3(grid), \
                     dim3(block), 0, stream.stream(),                       \
                     reinterpret_cast<short*>(q_rot.data_ptr()),            \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const short*>(k.data_ptr()),          \
                     reinterpret_cast<const short*>(v.data_ptr()),          \
                     cos.data_ptr<float>(), sin.data_ptr<float>(),          \
                     tok_slot.data_ptr<int64_t>(),                          \
                     tok_pos.data_ptr<int64_t>(),                           \
                     reinterpret_cast<unsigned char*>(kpool.data_ptr()),    \
                     reinterpret_cast<unsigned char*>(vpool.data_ptr()),    \
                     k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),  \
                     lens_ptr, total, (int)T, (int)Hq, (int)Hk, (int)B,     \
                     (int)Smax, (int)P)
  if (D == 128)
    LAUNCH(128);
  else
    LAUNCH(64);
#undef LAUNCH
  HIP_CHECK_KERNEL();
  return q_rot;
}
