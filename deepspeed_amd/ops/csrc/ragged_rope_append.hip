// Fused ragged RoPE + KV-append for the serving steps on MI355X (gfx950).
//
// Role parity: reference inference/v2/kernels/ragged_ops/
// linear_blocked_kv_rotary (rotate q and k, copy k/v into the KV store, one
// launch per layer). MI355X-native: the store is the slot pool
// [B, Smax, Hk, D] that ragged_decode / ragged_prefill read, so a token's
// K/V row goes straight to kpool[tok_slot[t], tok_pos[t]] and the per-slot
// length is written by the same launch. Replaces, per layer, the eager
// per-row RoPE of q and k (a dozen elementwise launches each) and the three
// index_puts of RaggedKVCache.update.
//
// Memory-bound, so it follows rope_kernel (elementwise.hip): host-precomputed
// fp32 cos/sin table, each lane rotates 8 (d, d + D/2) pairs with two bf16x8
// loads, f32x4 table loads and 16-byte stores, grid-stride, no LDS. One work
// item is (token, head, 8-pair group) over the Hq q heads, then the Hk k
// heads, then the Hk v heads (a plain copy).
//
// Device guard: tok_slot / tok_pos are device data. A token whose slot is
// outside [0,B) or whose position is outside [0, min(Smax,P)) is skipped:
// nothing is written for it to the pools or to lens, and its q_rot row is 0.
#include <torch/extension.h>

#include <climits>

#include "common.h"

namespace rra {

DEV_INLINE bool tok_ok(long long slot, long long pos, int B, int Smax,
                       int P) {
  return slot >= 0 && slot < B && pos >= 0 && pos < Smax && pos < P;
}

// Called by exactly one lane per valid token (q head 0, first group). A
// sequence is one contiguous q range with its own slot, so its last token is
// the one followed by another slot (or by nothing).
DEV_INLINE void write_len(int64_t* __restrict__ lens,
                          const int64_t* __restrict__ tok_slot, long long t,
                          int T, long long slot, long long pos) {
  if (lens == nullptr) return;
  if (t == T - 1 || tok_slot[t + 1] != slot) lens[slot] = pos + 1;
}

DEV_INLINE void rotate8(short* __restrict__ dst,
                        const short* __restrict__ src,
                        const float* __restrict__ crow,
                        const float* __restrict__ srow, int half) {
  bf16x8 x1 = *reinterpret_cast<const bf16x8*>(src);
  bf16x8 x2 = *reinterpret_cast<const bf16x8*>(src + half);
  f32x4 c0 = *reinterpret_cast<const f32x4*>(crow);
  f32x4 c1 = *reinterpret_cast<const f32x4*>(crow + 4);
  f32x4 s0 = *reinterpret_cast<const f32x4*>(srow);
  f32x4 s1 = *reinterpret_cast<const f32x4*>(srow + 4);
  bf16x8 o1, o2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float c = (j < 4 ? c0.v[j] : c1.v[j - 4]);
    float sv = (j < 4 ? s0.v[j] : s1.v[j - 4]);
    float a = bf2f(x1.v[j]);
    float b = bf2f(x2.v[j]);
    o1.v[j] = f2bf(a * c - b * sv);
    o2.v[j] = f2bf(b * c + a * sv);
  }
  *reinterpret_cast<bf16x8*>(dst) = o1;
  *reinterpret_cast<bf16x8*>(dst + half) = o2;
}

// q [T,Hq,D], k/v [T,Hk,D], q_rot [T,Hq,D], kpool/vpool [B,Smax,Hk,D] bf16;
// cs/sn [P, D/2] fp32; tok_slot/tok_pos [T] i64; lens [B] i64 or null.
// total = T * (Hq + 2*Hk) * (D/16).
__global__ void ragged_rope_append_kernel(
    short* __restrict__ q_rot, const short* __restrict__ q,
    const short* __restrict__ k, const short* __restrict__ v,
    const float* __restrict__ cs, const float* __restrict__ sn,
    const int64_t* __restrict__ tok_slot,
    const int64_t* __restrict__ tok_pos, short* __restrict__ kpool,
    short* __restrict__ vpool, int64_t* __restrict__ lens, long long total,
    int T, int Hq, int Hk, int D, int B, int Smax, int P) {
  const int half = D / 2;
  const int half8 = half / 8;
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
      if (!ok) {
        bf16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z.v[j] = 0;
        *reinterpret_cast<bf16x8*>(q_rot + base) = z;
        *reinterpret_cast<bf16x8*>(q_rot + base + half) = z;
        continue;
      }
      if (hh == 0 && d8 == 0) write_len(lens, tok_slot, t, T, slot, pos);
      rotate8(q_rot + base, q + base, cs + pos * half + off,
              sn + pos * half + off, half);
      continue;
    }
    if (!ok) continue;
    const int hk = hh < Hq + Hk ? hh - Hq : hh - Hq - Hk;
    const long long src = (t * Hk + hk) * D + off;
    const long long dst = ((slot * Smax + pos) * Hk + hk) * D + off;
    if (hh < Hq + Hk) {
      rotate8(kpool + dst, k + src, cs + pos * half + off,
              sn + pos * half + off, half);
    } else {
      *reinterpret_cast<bf16x8*>(vpool + dst) =
          *reinterpret_cast<const bf16x8*>(v + src);
      *reinterpret_cast<bf16x8*>(vpool + dst + half) =
          *reinterpret_cast<const bf16x8*>(v + src + half);
    }
  }
}

// scalar arm: D/2 not divisible by 8, or a pointer off 16-byte alignment.
// One work item is one (d, d + D/2) pair; total = T * (Hq + 2*Hk) * (D/2).
__global__ void ragged_rope_append_kernel_scalar(
    short* __restrict__ q_rot, const short* __restrict__ q,
    const short* __restrict__ k, const short* __restrict__ v,
    const float* __restrict__ cs, const float* __restrict__ sn,
    const int64_t* __restrict__ tok_slot,
    const int64_t* __restrict__ tok_pos, short* __restrict__ kpool,
    short* __restrict__ vpool, int64_t* __restrict__ lens, long long total,
    int T, int Hq, int Hk, int D, int B, int Smax, int P) {
  const int half = D / 2;
  const int heads = Hq + 2 * Hk;
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < total; i += stride) {
    const int d = (int)(i % half);
    const long long rem = i / half;
    const int hh = (int)(rem % heads);
    const long long t = rem / heads;
    const long long slot = tok_slot[t];
    const long long pos = tok_pos[t];
    const bool ok = tok_ok(slot, pos, B, Smax, P);
    if (hh < Hq) {
      const long long base = (t * Hq + hh) * D + d;
      if (!ok) {
        q_rot[base] = 0;
        q_rot[base + half] = 0;
        continue;
      }
      if (hh == 0 && d == 0) write_len(lens, tok_slot, t, T, slot, pos);
      const float c = cs[pos * half + d];
      const float sv = sn[pos * half + d];
      const float a = bf2f(q[base]);
      const float b = bf2f(q[base + half]);
      q_rot[base] = f2bf(a * c - b * sv);
      q_rot[base + half] = f2bf(b * c + a * sv);
      continue;
    }
    if (!ok) continue;
    const int hk = hh < Hq + Hk ? hh - Hq : hh - Hq - Hk;
    const long long src = (t * Hk + hk) * D + d;
    const long long dst = ((slot * Smax + pos) * Hk + hk) * D + d;
    if (hh < Hq + Hk) {
      const float c = cs[pos * half + d];
      const float sv = sn[pos * half + d];
      const float a = bf2f(k[src]);
      const float b = bf2f(k[src + half]);
      kpool[dst] = f2bf(a * c - b * sv);
      kpool[dst + half] = f2bf(b * c + a * sv);
    } else {
      vpool[dst] = v[src];
      vpool[dst + half] = v[src + half];
    }
  }
}

}  // namespace rra

at::Tensor ragged_rope_append(at::Tensor q, at::Tensor k, at::Tensor v,
                              at::Tensor cos, at::Tensor sin,
                              at::Tensor tok_slot, at::Tensor tok_pos,
                              at::Tensor kpool, at::Tensor vpool,
                              c10::optional<at::Tensor> lens) {
  CHECK_ARG(q, at::kBFloat16);
  CHECK_ARG(k, at::kBFloat16);
  CHECK_ARG(v, at::kBFloat16);
  CHECK_ARG(cos, at::kFloat);
  CHECK_ARG(sin, at::kFloat);
  CHECK_ARG(tok_slot, at::kLong);
  CHECK_ARG(tok_pos, at::kLong);
  CHECK_ARG(kpool, at::kBFloat16);
  CHECK_ARG(vpool, at::kBFloat16);
  CHECK_ON(k, q);
  CHECK_ON(v, q);
  CHECK_ON(cos, q);
  CHECK_ON(sin, q);
  CHECK_ON(tok_slot, q);
  CHECK_ON(tok_pos, q);
  CHECK_ON(kpool, q);
  CHECK_ON(vpool, q);
  TORCH_CHECK(q.dim() == 3, "ragged_rope_append: q must be [T,Hq,D]");
  TORCH_CHECK(k.dim() == 3 && v.sizes() == k.sizes(),
              "ragged_rope_append: k and v must both be [T,Hk,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(),
              "ragged_rope_append: kpool and vpool must both be "
              "[B,Smax,Hk,D]");
  const long T = q.size(0), Hq = q.size(1), D = q.size(2);
  const long Hk = k.size(1);
  const long B = kpool.size(0), Smax = kpool.size(1);
  TORCH_CHECK(k.size(0) == T && k.size(2) == D,
              "ragged_rope_append: k/v must have q's token count and "
              "head_dim");
  TORCH_CHECK(D >= 2 && D % 2 == 0, "ragged_rope_append: D must be even");
  TORCH_CHECK(Hk >= 1 && Hq >= 1 && Hq % Hk == 0,
              "ragged_rope_append: Hq % Hk != 0");
  TORCH_CHECK(kpool.size(2) == Hk && kpool.size(3) == D,
              "ragged_rope_append: pool heads/head_dim != k heads/head_dim");
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == D / 2 &&
                  sin.sizes() == cos.sizes(),
              "ragged_rope_append: cos and sin must both be [P, D/2]");
  const long P = cos.size(0);
  TORCH_CHECK(P >= Smax, "ragged_rope_append: table rows P ", P,
              " < pool Smax ", Smax);
  TORCH_CHECK(tok_slot.dim() == 1 && tok_slot.size(0) == T &&
                  tok_pos.dim() == 1 && tok_pos.size(0) == T,
              "ragged_rope_append: tok_slot and tok_pos must be [T]");
  int64_t* lens_ptr = nullptr;
  if (lens.has_value()) {
    const at::Tensor& lens_t = *lens;
    CHECK_ARG(lens_t, at::kLong);
    CHECK_ON(lens_t, q);
    TORCH_CHECK(lens_t.dim() == 1 && lens_t.size(0) == B,
                "ragged_rope_append: lens must be [B]");
    lens_ptr = lens_t.data_ptr<int64_t>();
  }
  TORCH_CHECK(T <= INT_MAX && B <= INT_MAX && Smax <= INT_MAX &&
                  P <= INT_MAX && Hq + 2 * Hk <= INT_MAX && D <= INT_MAX,
              "ragged_rope_append: a dimension exceeds int32");

  auto q_rot = at::empty_like(q);
  if (T == 0) return q_rot;
  TORCH_CHECK(B >= 1 && Smax >= 1, "ragged_rope_append: empty pool");

  auto stream = c10::hip::getCurrentHIPStream();
  const int block = 256;
  const bool vec = (D / 2) % 8 == 0 && ptr_aligned(q.data_ptr(), 16) &&
                   ptr_aligned(k.data_ptr(), 16) &&
                   ptr_aligned(v.data_ptr(), 16) &&
                   ptr_aligned(q_rot.data_ptr(), 16) &&
                   ptr_aligned(kpool.data_ptr(), 16) &&
                   ptr_aligned(vpool.data_ptr(), 16) &&
                   ptr_aligned(cos.data_ptr(), 16) &&
                   ptr_aligned(sin.data_ptr(), 16);
  const long long total =
      (long long)T * (Hq + 2 * Hk) * (vec ? D / 16 : D / 2);
  const int grid = grid_for(total, block);
#define LAUNCH(KERNEL)                                                      \
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(block), 0, stream.stream(),   \
                     reinterpret_cast<short*>(q_rot.data_ptr()),            \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const short*>(k.data_ptr()),          \
                     reinterpret_cast<const short*>(v.data_ptr()),          \
                     cos.data_ptr<float>(), sin.data_ptr<float>(),          \
                     tok_slot.data_ptr<int64_t>(),                          \
                     tok_pos.data_ptr<int64_t>(),                           \
                     reinterpret_cast<short*>(kpool.data_ptr()),            \
                     reinterpret_cast<short*>(vpool.data_ptr()), lens_ptr,  \
                     total, (int)T, (int)Hq, (int)Hk, (int)D, (int)B,       \
                     (int)Smax, (int)P)
  if (vec)
    LAUNCH(rra::ragged_rope_append_kernel);
  else
    LAUNCH(rra::ragged_rope_append_kernel_scalar);
#undef LAUNCH
  HIP_CHECK_KERNEL();
  return q_rot;
}
