// Fused channel bias-add for convolutional/diffusion blocks (NHWC/NCHW).
//
// Role parity: reference csrc/spatial/opt_bias_add.cu (UNet channels).
#include <torch/extension.h>

#include "common.h"

// y = a + bias (bias broadcast over the channel dim, last-dim layout)
__global__ void bias_add_kernel(const short* __restrict__ a,
                                const short* __restrict__ bias,
                                short* __restrict__ y, long long total,
                                int C, int vec_ok) {
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  long long t8 = vec_ok ? total / 8 : 0;  // vec_ok: a and y 16-byte aligned
  for (long long i = i0; i < t8; i += stride) {
    bf16x8 av = reinterpret_cast<const bf16x8*>(a)[i];
    long long base = i * 8;
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      o.v[k] = f2bf(bf2f(av.v[k]) + bf2f(bias[(base + k) % C]));
    reinterpret_cast<bf16x8*>(y)[i] = o;
  }
  for (long long i = t8 * 8 + i0; i < total; i += stride)
    y[i] = f2bf(bf2f(a[i]) + bf2f(bias[i % C]));
}

// y = a + b + bias (fused residual variant, ref opt_bias_add_add)
__global__ void bias_add_add_kernel(const short* __restrict__ a,
                                    const short* __restrict__ b,
                                    const short* __restrict__ bias,
                                    short* __restrict__ y, long long total,
                                    int C) {
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < total; i += stride)
    y[i] = f2bf(bf2f(a[i]) + bf2f(b[i]) + bf2f(bias[i % C]));
}

at::Tensor spatial_bias_add(at::Tensor a, at::Tensor bias,
                            c10::optional<at::Tensor> other) {
  CHECK_ARG(a, at::kBFloat16);
  CHECK_ARG(bias, at::kBFloat16);
  CHECK_ON(bias, a);
  int C = bias.numel();
  TORCH_CHECK(a.dim() >= 1 && C > 0 && a.size(-1) == C,
              "bias must match the last dim");
  if (other.has_value()) {
    CHECK_ARG(*other, at::kBFloat16);
    CHECK_LIKE(*other, a);
  }
  long long total = a.numel();
  auto y = at::empty_like(a);
  if (total == 0) return y;
  int vec_ok = ptr_aligned(a.data_ptr(), 16) && ptr_aligned(y.data_ptr(), 16);
  auto stream = c10::hip::getCurrentHIPStream();
  int grid = grid_for(total / 8 + 1, 256);
  if (other.has_value()) {
    hipLaunchKernelGGL(bias_add_add_kernel, dim3(grid), dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const short*>(a.data_ptr()),
                       reinterpret_cast<const short*>(other->data_ptr()),
                       reinterpret_cast<const short*>(bias.data_ptr()),
                       reinterpret_cast<short*>(y.data_ptr()), total, C);
  } else {
    hipLaunchKernelGGL(bias_add_kernel, dim3(grid), dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const short*>(a.data_ptr()),
                       reinterpret_cast<const short*>(bias.data_ptr()),
                       reinterpret_cast<short*>(y.data_ptr()), total, C,
                       vec_ok);
  }
  HIP_CHECK_KERNEL();
  return y;
}
