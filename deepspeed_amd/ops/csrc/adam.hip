// Fused AdamW for MI355X (gfx950).
//
// Role parity: reference csrc/adam/multi_tensor_adam.cu (multi_tensor_adam_cuda).
// MI355X-native design: ZeRO masters are a handful of LARGE flat fp32 slabs,
// so instead of CUDA-style kernarg metadata packing we launch one grid-stride
// kernel per slab with float4 vector IO (memory-bound: 28 B/elem traffic),
// and optionally fuse the fp32->bf16 shard writeback (saves a full extra
// read+write pass over the parameters).
#include <torch/extension.h>

#include "common.h"

__global__ void adam_kernel_f32(float* __restrict__ p,
                                const float* __restrict__ g,
                                float* __restrict__ m, float* __restrict__ v,
                                short* __restrict__ out16,  // optional bf16 out
                                long long n, float lr, float beta1, float beta2,
                                float eps, float bc1, float bc2, int adamw,
                                float wd, float gscale, int vec_ok) {
  const float step_size = lr / bc1;
  const float bc2_sqrt = sqrtf(bc2);
  long long i0 = (long long)(blockIdx.x) * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  // vectorized main loop: 4 floats per lane; vec_ok: p/g/m/v 16-byte and
  // out16 8-byte aligned (host-checked), else everything takes the tail loop
  long long n4 = vec_ok ? n / 4 : 0;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  f32x4* p4 = reinterpret_cast<f32x4*>(p);
  f32x4* m4 = reinterpret_cast<f32x4*>(m);
  f32x4* v4 = reinterpret_cast<f32x4*>(v);
  for (long long i = i0; i < n4; i += stride) {
    f32x4 gv = g4[i], pv = p4[i], mv = m4[i], vv = v4[i];
    short o16[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gk = gv.v[k] * gscale;
      float pk = pv.v[k];
      if (adamw) {
        pk *= (1.f - lr * wd);
      } else if (wd != 0.f) {
        gk += wd * pk;
      }
      float mk = mv.v[k] * beta1 + gk * (1.f - beta1);
      float vk = vv.v[k] * beta2 + gk * gk * (1.f - beta2);
      float denom = sqrtf(vk) / bc2_sqrt + eps;
      pk -= step_size * mk / denom;
      mv.v[k] = mk;
      vv.v[k] = vk;
      pv.v[k] = pk;
      o16[k] = f2bf(pk);
    }
    p4[i] = pv;
    m4[i] = mv;
    v4[i] = vv;
    if (out16) {
      *reinterpret_cast<uint2*>(out16 + i * 4) =
          *reinterpret_cast<uint2*>(o16);
    }
  }
  // tail
  for (long long i = n4 * 4 + i0; i < n; i += stride) {
    float gk = g[i] * gscale, pk = p[i];
    if (adamw) {
      pk *= (1.f - lr * wd);
    } else if (wd != 0.f) {
      gk += wd * pk;
    }
    float mk = m[i] * beta1 + gk * (1.f - beta1);
    float vk = v[i] * beta2 + gk * gk * (1.f - beta2);
    float denom = sqrtf(vk) / bc2_sqrt + eps;
    pk -= step_size * mk / denom;
    m[i] = mk;
    v[i] = vk;
    p[i] = pk;
    if (out16) out16[i] = f2bf(pk);
  }
}

// Shared argument contract of the multi-tensor optimizers: fp32 contiguous
// state lists of equal length and matching numel, optional bf16 out16.
static void check_opt_lists(
    const std::vector<at::Tensor>& params,
    std::initializer_list<const std::vector<at::Tensor>*> states,
    const std::vector<at::Tensor>& out16) {
  for (auto* s : states)
    TORCH_CHECK(s->size() == params.size(),
                "optimizer tensor lists must have equal length");
  TORCH_CHECK(out16.empty() || out16.size() == params.size(),
              "out16 must be empty or one tensor per param");
  for (size_t t = 0; t < params.size(); ++t) {
    const at::Tensor& p = params[t];
    TORCH_CHECK(p.scalar_type() == at::kFloat, "fp32 masters expected");
    CHECK_ARG(p, at::kFloat);
    for (auto* s : states) {
      const at::Tensor& st = (*s)[t];
      CHECK_ARG(st, at::kFloat);
      CHECK_LIKE(st, p);
    }
    if (!out16.empty()) {
      const at::Tensor& o = out16[t];
      CHECK_ARG(o, at::kBFloat16);
      CHECK_LIKE(o, p);
    }
  }
}

void multi_tensor_adam(std::vector<at::Tensor> params,
                       std::vector<at::Tensor> grads,
                       std::vector<at::Tensor> exp_avgs,
                       std::vector<at::Tensor> exp_avg_sqs, double lr,
                       double beta1, double beta2, double eps, long step,
                       long adamw_mode, long bias_correction,
                       double weight_decay,
                       std::vector<at::Tensor> out16 /* may be empty */,
                       double grad_scale) {
  float bc1 = 1.f, bc2 = 1.f;
  if (bias_correction) {
    bc1 = 1.f - powf((float)beta1, (float)step);
    bc2 = 1.f - powf((float)beta2, (float)step);
  }
  check_opt_lists(params, {&grads, &exp_avgs, &exp_avg_sqs}, out16);
  auto stream = c10::hip::getCurrentHIPStream();
  for (size_t t = 0; t < params.size(); ++t) {
    auto& p = params[t];
    long long n = p.numel();
    short* o16 = nullptr;
    if (!out16.empty())
      o16 = reinterpret_cast<short*>(out16[t].data_ptr());
    int vec_ok = ptr_aligned(p.data_ptr(), 16) &&
                 ptr_aligned(grads[t].data_ptr(), 16) &&
                 ptr_aligned(exp_avgs[t].data_ptr(), 16) &&
                 ptr_aligned(exp_avg_sqs[t].data_ptr(), 16) &&
                 (o16 == nullptr || ptr_aligned(o16, 8));
    int block = 256;
    int grid = grid_for(n / 4 + 1, block);
    hipLaunchKernelGGL(adam_kernel_f32, dim3(grid), dim3(block), 0,
                       stream.stream(), p.data_ptr<float>(),
                       grads[t].data_ptr<float>(),
                       exp_avgs[t].data_ptr<float>(),
                       exp_avg_sqs[t].data_ptr<float>(), o16, n, (float)lr,
                       (float)beta1, (float)beta2, (float)eps, bc1, bc2,
                       (int)adamw_mode, (float)weight_decay,
                       (float)grad_scale, vec_ok);
    HIP_CHECK_KERNEL();
  }
}

// Lion update (ref csrc/lion/multi_tensor_lion.cu) — sign-based, fp32 master.
__global__ void lion_kernel_f32(float* __restrict__ p,
                                const float* __restrict__ g,
                                float* __restrict__ m,
                                short* __restrict__ out16, long long n,
                                float lr, float beta1, float beta2, float wd) {
  long long i0 = (long long)(blockIdx.x) * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < n; i += stride) {
    float gk = g[i], pk = p[i], mk = m[i];
    pk *= (1.f - lr * wd);
    float u = mk * beta1 + gk * (1.f - beta1);
    pk -= lr * (u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f));
    m[i] = mk * beta2 + gk * (1.f - beta2);
    p[i] = pk;
    if (out16) out16[i] = f2bf(pk);
  }
}

void multi_tensor_lion(std::vector<at::Tensor> params,
                       std::vector<at::Tensor> grads,
                       std::vector<at::Tensor> exp_avgs, double lr,
                       double beta1, double beta2, double weight_decay,
                       std::vector<at::Tensor> out16) {
  check_opt_lists(params, {&grads, &exp_avgs}, out16);
  auto stream = c10::hip::getCurrentHIPStream();
  for (size_t t = 0; t < params.size(); ++t) {
    long long n = params[t].numel();
    short* o16 = out16.empty()
                     ? nullptr
                     : reinterpret_cast<short*>(out16[t].data_ptr());
    int block = 256;
    int grid = grid_for(n, block);
    hipLaunchKernelGGL(lion_kernel_f32, dim3(grid), dim3(block), 0,
                       stream.stream(), params[t].data_ptr<float>(),
                       grads[t].data_ptr<float>(),
                       exp_avgs[t].data_ptr<float>(), o16, n, (float)lr,
                       (float)beta1, (float)beta2, (float)weight_decay);
    HIP_CHECK_KERNEL();
  }
}

// Adagrad (ref csrc/adagrad/cpu_adagrad.cpp GPU analogue): fp32 master.
__global__ void adagrad_kernel_f32(float* __restrict__ p,
                                   const float* __restrict__ g,
                                   float* __restrict__ h,
                                   short* __restrict__ out16, long long n,
                                   float lr, float eps, float wd) {
  long long i0 = (long long)(blockIdx.x) * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < n; i += stride) {
    float gk = g[i], pk = p[i];
    if (wd != 0.f) gk += wd * pk;
    float hk = h[i] + gk * gk;
    pk -= lr * gk / (sqrtf(hk) + eps);
    h[i] = hk;
    p[i] = pk;
    if (out16) out16[i] = f2bf(pk);
  }
}

void multi_tensor_adagrad(std::vector<at::Tensor> params,
                          std::vector<at::Tensor> grads,
                          std::vector<at::Tensor> sq_accums, double lr,
                          double eps, double weight_decay,
                          std::vector<at::Tensor> out16) {
  check_opt_lists(params, {&grads, &sq_accums}, out16);
  auto stream = c10::hip::getCurrentHIPStream();
  for (size_t t = 0; t < params.size(); ++t) {
    long long n = params[t].numel();
    short* o16 = out16.empty()
                     ? nullptr
                     : reinterpret_cast<short*>(out16[t].data_ptr());
    int block = 256;
    int grid = grid_for(n, block);
    hipLaunchKernelGGL(adagrad_kernel_f32, dim3(grid), dim3(block), 0,
                       stream.stream(), params[t].data_ptr<float>(),
                       grads[t].data_ptr<float>(),
                       sq_accums[t].data_ptr<float>(), o16, n, (float)lr,
                       (float)eps, (float)weight_decay);
    HIP_CHECK_KERNEL();
  }
}

// LAMB (ref csrc/lamb/fused_lamb_cuda_kernel.cu). Two passes, trust ratio
// computed DEVICE-side so there is no host sync per parameter:
//   pass 1: adam-moment update, u = mhat/(sqrt(vhat)+eps) + wd*p written
//           into the grad buffer (scratch), block-reduced ||p||^2,||u||^2
//           atomically accumulated into a 2-float workspace
//   pass 2: p -= lr * (||p||/||u||) * u
__global__ void lamb_phase1_f32(float* __restrict__ p,
                                const float* __restrict__ g,
                                float* __restrict__ u_out,
                                float* __restrict__ m, float* __restrict__ v,
                                float* __restrict__ ws, long long n,
                                float beta1, float beta2, float eps,
                                float bc1, float bc2, float wd,
                                float gscale) {
  __shared__ float red[2][4];
  long long i0 = (long long)(blockIdx.x) * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  float psq = 0.f, usq = 0.f;
  for (long long i = i0; i < n; i += stride) {
    float gk = g[i] * gscale, pk = p[i];
    float mk = m[i] * beta1 + gk * (1.f - beta1);
    float vk = v[i] * beta2 + gk * gk * (1.f - beta2);
    float u = (mk / bc1) / (sqrtf(vk / bc2) + eps) + wd * pk;
    m[i] = mk;
    v[i] = vk;
    u_out[i] = u;
    psq += pk * pk;
    usq += u * u;
  }
  psq = wave_reduce_sum(psq);
  usq = wave_reduce_sum(usq);
  int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wid] = psq;
    red[1][wid] = usq;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ps = 0.f, us = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
      ps += red[0][w];
      us += red[1][w];
    }
    atomicAdd(&ws[0], ps);
    atomicAdd(&ws[1], us);
  }
}

__global__ void lamb_phase2_f32(float* __restrict__ p,
                                const float* __restrict__ u,
                                const float* __restrict__ ws,
                                short* __restrict__ out16, long long n,
                                float lr) {
  float r1 = sqrtf(ws[0]), r2 = sqrtf(ws[1]);
  float ratio = (r1 > 0.f && r2 > 0.f) ? r1 / r2 : 1.f;
  long long i0 = (long long)(blockIdx.x) * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = i0; i < n; i += stride) {
    float pk = p[i] - lr * ratio * u[i];
    p[i] = pk;
    if (out16) out16[i] = f2bf(pk);
  }
}

void multi_tensor_lamb(std::vector<at::Tensor> params,
                       std::vector<at::Tensor> grads,
                       std::vector<at::Tensor> updates,  // scratch, grad-sized
                       std::vector<at::Tensor> exp_avgs,
                       std::vector<at::Tensor> exp_avg_sqs,
                       at::Tensor workspace,  // fp32 [2*nparams], zeroed
                       double lr, double beta1, double beta2, double eps,
                       long step, long bias_correction, double weight_decay,
                       std::vector<at::Tensor> out16, double grad_scale) {
  float bc1 = 1.f, bc2 = 1.f;
  if (bias_correction) {
    bc1 = 1.f - powf((float)beta1, (float)step);
    bc2 = 1.f - powf((float)beta2, (float)step);
  }
  check_opt_lists(params, {&grads, &updates, &exp_avgs, &exp_avg_sqs}, out16);
  CHECK_ARG(workspace, at::kFloat);
  TORCH_CHECK(workspace.numel() >= (long)(2 * params.size()));
  if (!params.empty()) CHECK_ON(workspace, params[0]);
  auto stream = c10::hip::getCurrentHIPStream();
  float* ws = workspace.data_ptr<float>();
  for (size_t t = 0; t < params.size(); ++t) {
    long long n = params[t].numel();
    int block = 256;
    int grid = grid_for(n, block);
    hipLaunchKernelGGL(lamb_phase1_f32, dim3(grid), dim3(block), 0,
                       stream.stream(), params[t].data_ptr<float>(),
                       grads[t].data_ptr<float>(),
                       updates[t].data_ptr<float>(),
                       exp_avgs[t].data_ptr<float>(),
                       exp_avg_sqs[t].data_ptr<float>(), ws + 2 * t, n,
                       (float)beta1, (float)beta2, (float)eps, bc1, bc2,
                       (float)weight_decay, (float)grad_scale);
    HIP_CHECK_KERNEL();
  }
  for (size_t t = 0; t < params.size(); ++t) {
    long long n = params[t].numel();
    short* o16 = out16.empty()
                     ? nullptr
                     : reinterpret_cast<short*>(out16[t].data_ptr());
    int block = 256;
    int grid = grid_for(n, block);
    hipLaunchKernelGGL(lamb_phase2_f32, dim3(grid), dim3(block), 0,
                       stream.stream(), params[t].data_ptr<float>(),
                       updates[t].data_ptr<float>(), ws + 2 * t, o16, n,
                       (float)lr);
    HIP_CHECK_KERNEL();
  }
}
