// Misc ZeRO-path kernels: fused grad accumulate (bf16 -> fp32 +=) and
// multi-tensor L2-norm^2 (single pass, device-side accumulation).
//
// These replace torch eager chains that cost multiple full passes over the
// 32 GB fp32 grad shards per step (profiled: .double().pow(2).sum() chain
// was ~69 ms/step on the 8B config; this is one ~5 ms read pass).
#include <torch/extension.h>

#include "common.h"

// OVERWRITE: dst = float(src) * scale and dst is never read (the first
// accumulate of a window needs no zero fill before it); else dst += ...
template <bool OVERWRITE>
__global__ void accum_bf16_f32_kernel(float* __restrict__ dst,
                                      const short* __restrict__ src,
                                      long long n, float scale,
                                      int vec_ok) {
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  // vec_ok: dst 16-byte and src 8-byte aligned (host-checked), else scalar
  long long n4 = vec_ok ? n / 4 : 0;
  for (long long i = i0; i < n4; i += stride) {
    uint2 sv = reinterpret_cast<const uint2*>(src)[i];
    const short* s = reinterpret_cast<const short*>(&sv);
    f32x4 d;
    if (OVERWRITE) {
#pragma unroll
      for (int k = 0; k < 4; ++k) d.v[k] = bf2f(s[k]) * scale;
    } else {
      d = reinterpret_cast<f32x4*>(dst)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) d.v[k] += bf2f(s[k]) * scale;
    }
    reinterpret_cast<f32x4*>(dst)[i] = d;
  }
  for (long long i = n4 * 4 + i0; i < n; i += stride) {
    if (OVERWRITE)
      dst[i] = bf2f(src[i]) * scale;
    else
      dst[i] += bf2f(src[i]) * scale;
  }
}

void accum_bf16_to_f32(at::Tensor dst, at::Tensor src, double scale,
                       bool overwrite) {
  CHECK_ARG(dst, at::kFloat);
  CHECK_ARG(src, at::kBFloat16);
  CHECK_LIKE(src, dst);
  long long n = dst.numel();
  if (n == 0) return;
  int vec_ok = ptr_aligned(dst.data_ptr(), 16) && ptr_aligned(src.data_ptr(), 8);
  auto stream = c10::hip::getCurrentHIPStream();
  int block = 256;
  int grid = grid_for(n / 4 + 1, block);
  auto kern = overwrite ? accum_bf16_f32_kernel<true>
                        : accum_bf16_f32_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, stream.stream(),
                     dst.data_ptr<float>(),
                     reinterpret_cast<const short*>(src.data_ptr()), n,
                     (float)scale, vec_ok);
  HIP_CHECK_KERNEL();
}

template <int BLOCK>
__global__ void l2norm_sq_kernel(const float* __restrict__ x, long long n,
                                 float* __restrict__ out /* accum */,
                                 int vec_ok) {
  __shared__ float lds[BLOCK / WAVE];
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  float acc = 0.f;
  long long n4 = vec_ok ? n / 4 : 0;
  for (long long i = i0; i < n4; i += stride) {
    f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += v.v[k] * v.v[k];
  }
  for (long long i = n4 * 4 + i0; i < n; i += stride) acc += x[i] * x[i];
  acc = block_reduce_sum<BLOCK>(acc, lds);
  if (threadIdx.x == 0) atomicAdd(out, acc);
}

at::Tensor l2norm_sq(std::vector<at::Tensor> tensors) {
  TORCH_CHECK(!tensors.empty());
  for (auto& t : tensors) {
    CHECK_ARG(t, at::kFloat);
    CHECK_ON(t, tensors[0]);
  }
  auto out = at::zeros({1}, tensors[0].options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStream();
  constexpr int BLOCK = 256;
  for (auto& t : tensors) {
    long long n = t.numel();
    if (n == 0) continue;
    int vec_ok = ptr_aligned(t.data_ptr(), 16);
    int grid = grid_for(n / 4 + 1, BLOCK);
    hipLaunchKernelGGL(l2norm_sq_kernel<BLOCK>, dim3(grid), dim3(BLOCK), 0,
                       stream.stream(), t.data_ptr<float>(), n,
                       out.data_ptr<float>(), vec_ok);
    HIP_CHECK_KERNEL();
  }
  return out;
}
