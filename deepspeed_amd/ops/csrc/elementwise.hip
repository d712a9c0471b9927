// RoPE + SwiGLU elementwise kernels for MI355X (gfx950).
//
// Role parity: reference csrc/transformer/inference/csrc/apply_rotary_pos_emb.cu
// and gelu.cu (gated activations). MI355X-native: memory-bound, host-side
// precomputed cos/sin table (guide Appendix B: on-device trig turns these
// VALU-bound), vectorized bf16 IO, grid-stride.
#include <torch/extension.h>

#include "common.h"

// q/k layout: [B, S, H, D] bf16 contiguous; cos/sin: [>= pos0 + S, D/2] fp32;
// sequence position s uses table row s + pos0.
// Llama "rotate_half" pairing: (d, d + D/2).
// vectorized: each lane rotates 8 consecutive pairs (bf16x8 loads from both
// halves, float4x2 table loads) — scalar version measured 2.5 TB/s, this
// pattern is the guide-G13 8-16 B/lane sweet spot.
// one lane's share: 8 consecutive (d, d + D/2) pairs at element offset base
DEV_INLINE void rope_vec8(short* __restrict__ dst,
                          const short* __restrict__ src, long long base,
                          int half, const float* __restrict__ crow,
                          const float* __restrict__ srow, float sgn) {
  bf16x8 x1 = *reinterpret_cast<const bf16x8*>(src + base);
  bf16x8 x2 = *reinterpret_cast<const bf16x8*>(src + base + half);
  f32x4 c0 = *reinterpret_cast<const f32x4*>(crow);
  f32x4 c1 = *reinterpret_cast<const f32x4*>(crow + 4);
  f32x4 s0 = *reinterpret_cast<const f32x4*>(srow);
  f32x4 s1 = *reinterpret_cast<const f32x4*>(srow + 4);
  bf16x8 o1, o2;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float c = (k < 4 ? c0.v[k] : c1.v[k - 4]);
    float sv = (k < 4 ? s0.v[k] : s1.v[k - 4]) * sgn;
    float a = bf2f(x1.v[k]);
    float bb = bf2f(x2.v[k]);
    // the fused multiply-adds are spelled out: left to the compiler, the
    // contraction differed between rope_kernel and rope_qk_kernel (one
    // element per lane got mul, mul, sub), and with it the rounded bits
    o1.v[k] = f2bf(__builtin_fmaf(a, c, -(bb * sv)));
    o2.v[k] = f2bf(__builtin_fmaf(bb, c, a * sv));
  }
  *reinterpret_cast<bf16x8*>(dst + base) = o1;
  *reinterpret_cast<bf16x8*>(dst + base + half) = o2;
}

__global__ void rope_kernel(short* __restrict__ dst,
                            const short* __restrict__ src,
                            const float* __restrict__ cs,  // [S, D/2] cos
                            const float* __restrict__ sn,  // [S, D/2] sin
                            long long total_vec, int S, int H, int D,
                            int pos0, int backward) {
  int half = D / 2;
  int half8 = half / 8;
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < total_vec; i += stride) {
    int d8 = (int)(i % half8);
    long long rem = i / half8;
    int h = (int)(rem % H);
    long long rem2 = rem / H;
    int s = (int)(rem2 % S);
    long long b = rem2 / S;
    long long base = ((b * S + s) * (long long)H + h) * D + d8 * 8;
    rope_vec8(dst, src, base, half,
              cs + (long long)(s + pos0) * half + d8 * 8,
              sn + (long long)(s + pos0) * half + d8 * 8,
              backward ? -1.f : 1.f);
  }
}

// q and k in one launch: the grid runs over the Hq + Hk heads of a token;
// heads below Hq are q's, the rest k's. Same per-element math as rope_kernel.
__global__ void rope_qk_kernel(short* __restrict__ qd,
                               const short* __restrict__ qs,
                               short* __restrict__ kd,
                               const short* __restrict__ ks,
                               const float* __restrict__ cs,
                               const float* __restrict__ sn,
                               long long total_vec, int S, int Hq, int Hk,
                               int D) {
  int half = D / 2;
  int half8 = half / 8;
  int HT = Hq + Hk;
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < total_vec; i += stride) {
    int d8 = (int)(i % half8);
    long long rem = i / half8;
    int h = (int)(rem % HT);
    long long tok = rem / HT;  // b * S + s
    int s = (int)(tok % S);
    const float* crow = cs + (long long)s * half + d8 * 8;
    const float* srow = sn + (long long)s * half + d8 * 8;
    if (h < Hq)
      rope_vec8(qd, qs, (tok * Hq + h) * D + d8 * 8, half, crow, srow, 1.f);
    else
      rope_vec8(kd, ks, (tok * Hk + (h - Hq)) * D + d8 * 8, half, crow, srow,
                1.f);
  }
}

// scalar fallback for D/2 not divisible by 8
__global__ void rope_kernel_scalar(short* __restrict__ dst,
                                   const short* __restrict__ src,
                                   const float* __restrict__ cs,
                                   const float* __restrict__ sn,
                                   long long total_pairs, int S, int H,
                                   int D, int pos0, int backward) {
  int half = D / 2;
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < total_pairs; i += stride) {
    int d = (int)(i % half);
    long long rem = i / half;
    int h = (int)(rem % H);
    long long rem2 = rem / H;
    int s = (int)(rem2 % S);
    long long b = rem2 / S;
    long long base = ((b * S + s) * (long long)H + h) * D;
    float c = cs[(long long)(s + pos0) * half + d];
    float sv = sn[(long long)(s + pos0) * half + d];
    if (backward) sv = -sv;
    float x1 = bf2f(src[base + d]);
    float x2 = bf2f(src[base + d + half]);
    dst[base + d] = f2bf(x1 * c - x2 * sv);
    dst[base + d + half] = f2bf(x2 * c + x1 * sv);
  }
}

void rope(at::Tensor dst, at::Tensor src, at::Tensor cos, at::Tensor sin,
          long pos0, bool backward) {
  CHECK_ARG(src, at::kBFloat16);
  CHECK_ARG(dst, at::kBFloat16);
  CHECK_LIKE(dst, src);
  TORCH_CHECK(src.dim() == 4, "rope expects [B,S,H,D]");
  int B = src.size(0), S = src.size(1), H = src.size(2), D = src.size(3);
  TORCH_CHECK(D % 2 == 0, "rope: D must be even");
  if (src.numel() == 0) return;
  // the kernel dereferences the table on the device: reject host tensors
  // and tables shorter than the sequence instead of faulting
  TORCH_CHECK(cos.device() == src.device() && sin.device() == src.device() &&
                  dst.device() == src.device(),
              "rope: cos/sin/dst must be on the same device as src");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && cos.is_contiguous() &&
                  sin.scalar_type() == at::kFloat && sin.is_contiguous(),
              "rope: cos/sin must be contiguous fp32");
  TORCH_CHECK(pos0 >= 0, "rope: pos0 must be >= 0");
  TORCH_CHECK((long long)(pos0 + S) * (D / 2) <= cos.numel() &&
                  (long long)(pos0 + S) * (D / 2) <= sin.numel(),
              "rope: cos/sin table shorter than [pos0 + S, D/2]");
  auto stream = c10::hip::getCurrentHIPStream();
  int block = 256;
  bool vec = (D / 2) % 8 == 0 && ptr_aligned(src.data_ptr(), 16) &&
             ptr_aligned(dst.data_ptr(), 16) &&
             ptr_aligned(cos.data_ptr(), 16) &&
             ptr_aligned(sin.data_ptr(), 16);
  if (vec) {
    long long total_vec = (long long)B * S * H * (D / 16);
    int grid = grid_for(total_vec, block);
    hipLaunchKernelGGL(rope_kernel, dim3(grid), dim3(block), 0,
                       stream.stream(),
                       reinterpret_cast<short*>(dst.data_ptr()),
                       reinterpret_cast<const short*>(src.data_ptr()),
                       cos.data_ptr<float>(), sin.data_ptr<float>(),
                       total_vec, S, H, D, (int)pos0, backward ? 1 : 0);
  } else {
    long long total_pairs = (long long)B * S * H * (D / 2);
    int grid = grid_for(total_pairs, block);
    hipLaunchKernelGGL(rope_kernel_scalar, dim3(grid), dim3(block), 0,
                       stream.stream(),
                       reinterpret_cast<short*>(dst.data_ptr()),
                       reinterpret_cast<const short*>(src.data_ptr()),
                       cos.data_ptr<float>(), sin.data_ptr<float>(),
                       total_pairs, S, H, D, (int)pos0, backward ? 1 : 0);
  }
  HIP_CHECK_KERNEL();
}

// Table contract shared by rope_qk and the flash backward epilogues: fp32,
// contiguous, on ref's device, at least [S, D/2], 16-byte aligned.
void check_rope_table(const at::Tensor& cos, const at::Tensor& sin,
                      const at::Tensor& ref, long long S, int D,
                      const char* who) {
  TORCH_CHECK(cos.defined() && sin.defined() &&
                  cos.device() == ref.device() && sin.device() == ref.device(),
              who, ": cos/sin must be on the same device as q");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && cos.is_contiguous() &&
                  sin.scalar_type() == at::kFloat && sin.is_contiguous(),
              who, ": cos/sin must be contiguous fp32");
  TORCH_CHECK(S * (D / 2) <= cos.numel() && S * (D / 2) <= sin.numel(),
              who, ": cos/sin table shorter than [S, D/2]");
  TORCH_CHECK(ptr_aligned(cos.data_ptr(), 16) &&
                  ptr_aligned(sin.data_ptr(), 16),
              who, ": cos/sin must be 16-byte aligned");
}

// Forward rotation of q [B,S,Hq,D] and k [B,S,Hk,D] in one launch (training
// path: positions 0..S-1, vector layout required; other callers use rope()).
std::vector<at::Tensor> rope_qk(at::Tensor q, at::Tensor k, at::Tensor cos,
                                at::Tensor sin) {
  CHECK_ARG(q, at::kBFloat16);
  CHECK_ARG(k, at::kBFloat16);
  CHECK_ON(k, q);
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && q.size(0) == k.size(0) &&
                  q.size(1) == k.size(1) && q.size(3) == k.size(3),
              "rope_qk expects q [B,S,Hq,D] and k [B,S,Hk,D]");
  int B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3);
  int Hk = k.size(2);
  TORCH_CHECK(D % 16 == 0, "rope_qk: D must be a multiple of 16");
  auto qo = at::empty_like(q);
  auto ko = at::empty_like(k);
  if (q.numel() + k.numel() == 0) return {qo, ko};
  check_rope_table(cos, sin, q, S, D, "rope_qk");
  TORCH_CHECK(ptr_aligned(q.data_ptr(), 16) && ptr_aligned(k.data_ptr(), 16) &&
                  ptr_aligned(qo.data_ptr(), 16) &&
                  ptr_aligned(ko.data_ptr(), 16),
              "rope_qk: q/k must be 16-byte aligned");
  auto stream = c10::hip::getCurrentHIPStream();
  int block = 256;
  long long total_vec = (long long)B * S * (Hq + Hk) * (D / 16);
  int grid = grid_for(total_vec, block);
  hipLaunchKernelGGL(rope_qk_kernel, dim3(grid), dim3(block), 0,
                     stream.stream(), reinterpret_cast<short*>(qo.data_ptr()),
                     reinterpret_cast<const short*>(q.data_ptr()),
                     reinterpret_cast<short*>(ko.data_ptr()),
                     reinterpret_cast<const short*>(k.data_ptr()),
                     cos.data_ptr<float>(), sin.data_ptr<float>(), total_vec,
                     S, Hq, Hk, D);
  HIP_CHECK_KERNEL();
  return {qo, ko};
}

void rope_inplace(at::Tensor t, at::Tensor cos, at::Tensor sin, long pos0,
                  bool backward) {
  rope(t, t, cos, sin, pos0, backward);
}

// -------- SwiGLU: y = silu(g) * u; packed gu = [..., 2*I] (g|u) ----------
__global__ void swiglu_fwd_kernel(const short* __restrict__ g,
                                  const short* __restrict__ u,
                                  short* __restrict__ y, long long n,
                                  int vec_ok) {
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  long long n8 = vec_ok ? n / 8 : 0;  // vec_ok: all bases 16-byte aligned
  for (long long i = i0; i < n8; i += stride) {
    bf16x8 gv = reinterpret_cast<const bf16x8*>(g)[i];
    bf16x8 uv = reinterpret_cast<const bf16x8*>(u)[i];
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float gf = bf2f(gv.v[k]);
      float s = gf / (1.f + __expf(-gf));
      o.v[k] = f2bf(s * bf2f(uv.v[k]));
    }
    reinterpret_cast<bf16x8*>(y)[i] = o;
  }
  for (long long i = n8 * 8 + i0; i < n; i += stride) {
    float gf = bf2f(g[i]);
    float s = gf / (1.f + __expf(-gf));
    y[i] = f2bf(s * bf2f(u[i]));
  }
}

__global__ void swiglu_bwd_kernel(const short* __restrict__ dy,
                                  const short* __restrict__ g,
                                  const short* __restrict__ u,
                                  short* __restrict__ dg,
                                  short* __restrict__ du, long long n,
                                  int vec_ok) {
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  long long n8 = vec_ok ? n / 8 : 0;
  for (long long i = i0; i < n8; i += stride) {
    bf16x8 dv = reinterpret_cast<const bf16x8*>(dy)[i];
    bf16x8 gv = reinterpret_cast<const bf16x8*>(g)[i];
    bf16x8 uv = reinterpret_cast<const bf16x8*>(u)[i];
    bf16x8 og, ou;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float gf = bf2f(gv.v[k]);
      float d = bf2f(dv.v[k]);
      float sig = 1.f / (1.f + __expf(-gf));
      float silu = gf * sig;
      og.v[k] = f2bf(d * bf2f(uv.v[k]) * (sig + silu * (1.f - sig)));
      ou.v[k] = f2bf(d * silu);
    }
    reinterpret_cast<bf16x8*>(dg)[i] = og;
    reinterpret_cast<bf16x8*>(du)[i] = ou;
  }
  for (long long i = n8 * 8 + i0; i < n; i += stride) {
    float gf = bf2f(g[i]);
    float d = bf2f(dy[i]);
    float sig = 1.f / (1.f + __expf(-gf));
    float silu = gf * sig;
    dg[i] = f2bf(d * bf2f(u[i]) * (sig + silu * (1.f - sig)));
    du[i] = f2bf(d * silu);
  }
}

at::Tensor swiglu_fwd(at::Tensor g, at::Tensor u) {
  CHECK_ARG(g, at::kBFloat16);
  CHECK_ARG(u, at::kBFloat16);
  CHECK_LIKE(u, g);
  auto y = at::empty_like(g);
  long long n = g.numel();
  if (n == 0) return y;
  int vec_ok = ptr_aligned(g.data_ptr(), 16) && ptr_aligned(u.data_ptr(), 16) &&
               ptr_aligned(y.data_ptr(), 16);
  auto stream = c10::hip::getCurrentHIPStream();
  int block = 256;
  int grid = grid_for(vec_ok ? n / 8 + 1 : n, block);
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3(grid), dim3(block), 0,
                     stream.stream(),
                     reinterpret_cast<const short*>(g.data_ptr()),
                     reinterpret_cast<const short*>(u.data_ptr()),
                     reinterpret_cast<short*>(y.data_ptr()), n, vec_ok);
  HIP_CHECK_KERNEL();
  return y;
}

std::vector<at::Tensor> swiglu_bwd(at::Tensor dy, at::Tensor g, at::Tensor u) {
  CHECK_ARG(g, at::kBFloat16);
  CHECK_ARG(u, at::kBFloat16);
  CHECK_ARG(dy, at::kBFloat16);
  CHECK_LIKE(u, g);
  CHECK_LIKE(dy, g);
  auto dg = at::empty_like(g);
  auto du = at::empty_like(u);
  long long n = g.numel();
  if (n == 0) return {dg, du};
  int vec_ok = ptr_aligned(dy.data_ptr(), 16) &&
               ptr_aligned(g.data_ptr(), 16) &&
               ptr_aligned(u.data_ptr(), 16) &&
               ptr_aligned(dg.data_ptr(), 16) &&
               ptr_aligned(du.data_ptr(), 16);
  auto stream = c10::hip::getCurrentHIPStream();
  int block = 256;
  int grid = grid_for(vec_ok ? n / 8 + 1 : n, block);
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(grid), dim3(block), 0,
                     stream.stream(),
                     reinterpret_cast<const short*>(dy.data_ptr()),
                     reinterpret_cast<const short*>(g.data_ptr()),
                     reinterpret_cast<const short*>(u.data_ptr()),
                     reinterpret_cast<short*>(dg.data_ptr()),
                     reinterpret_cast<short*>(du.data_ptr()), n, vec_ok);
  HIP_CHECK_KERNEL();
  return {dg, du};
}
