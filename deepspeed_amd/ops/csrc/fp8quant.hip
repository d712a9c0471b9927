// Fused fp8 (OCP e4m3fn / e5m2) quantization kernels for the fp8 Linear
// path — MI355X (gfx950).
//
// Why: torch-op quantization (inf-norm reduce + mul + clamp + cast, plus
// fp8 transposes in backward) measured ~24% of the fp8-MLP training step
// (profiles/fp8_mlp_kernel_stats) — more than the fp8 GEMMs themselves.
// These kernels do it at HBM speed-of-light:
//   amax:            1 read  (grid-stride bf16x8, DPP wave reduce,
//                             atomicMax on float bits)
//   cast:            1 read + 1/2 write (v_cvt_pk_fp8/bf8_f32 packing)
//   cast_transpose:  1 read + 1 write (both orientations via a 64x64
//                             LDS byte tile) — backward needs x^T and
//                             dy^T anyway, so the transpose is free.
// Role parity: reference csrc/fp_quantizer (fp8 stochastic quant for
// weight-only); here the training-GEMM fp8 recipe is MI355X-native.
#include <torch/extension.h>

#include "common.h"

using bf16x8_t = __attribute__((ext_vector_type(8))) short;

namespace fp8q {

// ---- amax -----------------------------------------------------------------
// max over |x| taken on the bf16 BIT patterns with the sign cleared: for
// non-negative floats the integer order is the float order, +inf sorts above
// every finite value and every NaN pattern above +inf, so a NaN anywhere in
// x comes out as NaN (fmaxf would drop it). `head` elements before the first
// 16-byte-aligned address and the tail after the last full vector are read
// one by one.
__global__ void amax_bf16_kernel(const short* __restrict__ x, long long n,
                                 long long head,
                                 unsigned int* __restrict__ out) {
  long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  long long stride = (long long)gridDim.x * blockDim.x * 8;
  const long long nv = (n - head) & ~7LL;  // elements in full vectors
  unsigned int m = 0;
  for (long long i = i0; i < nv; i += stride) {
    bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(x + head + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) m = max(m, (unsigned int)(v[j] & 0x7fff));
  }
  if (i0 == 0) {
    for (long long i = 0; i < head; ++i)
      m = max(m, (unsigned int)(x[i] & 0x7fff));
    for (long long i = head + nv; i < n; ++i)
      m = max(m, (unsigned int)(x[i] & 0x7fff));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    m = max(m, (unsigned int)__shfl_down((int)m, off, WAVE));
  if ((threadIdx.x & 63) == 0)
    atomicMax(out, m << 16);  // bf16 bits -> fp32 bits of the same value
}

// ---- packed convert helpers ----------------------------------------------
template <bool E5M2>
DEV_INLINE unsigned int cvt4(float a, float b, float c, float d, float fmax) {
  // saturate (+-inf included); fminf/fmaxf would turn NaN into -fmax, so
  // NaN bypasses the clamp and converts to the format's NaN
  a = (a != a) ? a : fminf(fmaxf(a, -fmax), fmax);
  b = (b != b) ? b : fminf(fmaxf(b, -fmax), fmax);
  c = (c != c) ? c : fminf(fmaxf(c, -fmax), fmax);
  d = (d != d) ? d : fminf(fmaxf(d, -fmax), fmax);
  int lo, w;
  if (E5M2) {
    lo = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, lo, true);
  } else {
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, lo, true);
  }
  return (unsigned int)w;
}

// ---- cast (row-major only) ------------------------------------------------
template <bool E5M2>
__global__ void fp8_cast_kernel(const short* __restrict__ x,
                                unsigned int* __restrict__ y,  // 4B = 4 fp8
                                long long n,
                                const float* __restrict__ scale,
                                float fmax) {
  const float inv = 1.f / fmaxf(*scale, 1e-12f);
  long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // 8-group
  long long n8 = n / 8;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; g < n8; g += stride) {
    bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(x + g * 8);
    unsigned int w0 = cvt4<E5M2>(bf2f(v[0]) * inv, bf2f(v[1]) * inv,
                                 bf2f(v[2]) * inv, bf2f(v[3]) * inv, fmax);
    unsigned int w1 = cvt4<E5M2>(bf2f(v[4]) * inv, bf2f(v[5]) * inv,
                                 bf2f(v[6]) * inv, bf2f(v[7]) * inv, fmax);
    y[g * 2] = w0;
    y[g * 2 + 1] = w1;
  }
}

// ---- cast + transpose -----------------------------------------------------
// x[M,K] bf16 -> y[M,K] fp8 row-major AND yt[K,M] fp8. 64x64 tiles staged
// as bytes in LDS (pad 4 per row spreads the column reads). The 16-byte
// vector accesses need every row start aligned: xvec (x rows, K % 8 == 0),
// yvec (y rows, K % 16 == 0), ytvec (yt rows, M % 16 == 0); otherwise that
// side goes element by element.
constexpr int TDIM = 64;
constexpr int TPAD = 4;

template <bool E5M2>
__launch_bounds__(256, 4)
__global__ void fp8_cast_transpose_kernel(const short* __restrict__ x,
                                          unsigned char* __restrict__ y,
                                          unsigned char* __restrict__ yt,
                                          int M, int K,
                                          const float* __restrict__ scale,
                                          float fmax, bool xvec, bool yvec,
                                          bool ytvec) {
  __shared__ unsigned char tile[TDIM][TDIM + TPAD];
  const float inv = 1.f / fmaxf(*scale, 1e-12f);
  const int tm = blockIdx.x * TDIM;  // row tile origin
  const int tk = blockIdx.y * TDIM;  // col tile origin
  // phase 1: 256 threads x 16 elems: row r = t/4, cols c0..c0+15
  {
    int r = threadIdx.x >> 2;
    int c0 = (threadIdx.x & 3) * 16;
    int gr = tm + r;
    if (gr < M) {
      const short* src = x + (long long)gr * K + tk + c0;
      unsigned int w[4];
      int avail = K - (tk + c0);  // >=16 except ragged edge
      if (xvec && avail >= 16) {
        bf16x8_t v0 = *reinterpret_cast<const bf16x8_t*>(src);
        bf16x8_t v1 = *reinterpret_cast<const bf16x8_t*>(src + 8);
        w[0] = cvt4<E5M2>(bf2f(v0[0]) * inv, bf2f(v0[1]) * inv,
                          bf2f(v0[2]) * inv, bf2f(v0[3]) * inv, fmax);
        w[1] = cvt4<E5M2>(bf2f(v0[4]) * inv, bf2f(v0[5]) * inv,
                          bf2f(v0[6]) * inv, bf2f(v0[7]) * inv, fmax);
        w[2] = cvt4<E5M2>(bf2f(v1[0]) * inv, bf2f(v1[1]) * inv,
                          bf2f(v1[2]) * inv, bf2f(v1[3]) * inv, fmax);
        w[3] = cvt4<E5M2>(bf2f(v1[4]) * inv, bf2f(v1[5]) * inv,
                          bf2f(v1[6]) * inv, bf2f(v1[7]) * inv, fmax);
      } else {
        unsigned char tmp[16];
        for (int j = 0; j < 16; ++j) {
          float f = (j < avail) ? bf2f(src[j]) * inv : 0.f;
          unsigned int p = cvt4<E5M2>(f, 0.f, 0.f, 0.f, fmax);
          tmp[j] = (unsigned char)(p & 0xff);
        }
        memcpy(w, tmp, 16);
      }
      if (yvec && tk + c0 + 16 <= K) {
        *reinterpret_cast<uint4*>(y + (long long)gr * K + tk + c0) =
            *reinterpret_cast<uint4*>(w);
      } else {
        const unsigned char* bw = reinterpret_cast<unsigned char*>(w);
        for (int j = 0; j < 16 && tk + c0 + j < K; ++j)
          y[(long long)gr * K + tk + c0 + j] = bw[j];
      }
      const unsigned char* bw = reinterpret_cast<unsigned char*>(w);
#pragma unroll
      for (int j = 0; j < 16; ++j) tile[r][c0 + j] = bw[j];
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) tile[r][c0 + j] = 0;
    }
  }
  __syncthreads();
  // phase 2: col c = t/4, rows r0..r0+15 -> yt[tk+c][tm+r0..]
  {
    int c = threadIdx.x >> 2;
    int r0 = (threadIdx.x & 3) * 16;
    int gc = tk + c;
    if (gc < K) {
      unsigned char out[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) out[j] = tile[r0 + j][c];
      if (ytvec && tm + r0 + 16 <= M) {
        *reinterpret_cast<uint4*>(yt + (long long)gc * M + tm + r0) =
            *reinterpret_cast<uint4*>(out);
      } else {
        for (int j = 0; j < 16 && tm + r0 + j < M; ++j)
          yt[(long long)gc * M + tm + r0 + j] = out[j];
      }
    }
  }
}

}  // namespace fp8q

at::Tensor fp8_amax(at::Tensor x) {
  CHECK_ARG(x, at::kBFloat16);
  auto out = at::zeros({1}, x.options().dtype(at::kFloat));
  long long n = x.numel();
  if (n == 0) return out;
  // elements before the first 16-byte boundary (bf16 is 2-byte aligned)
  long long head = (16 - reinterpret_cast<uintptr_t>(x.data_ptr()) % 16) % 16 / 2;
  head = std::min(head, n);
  auto stream = c10::hip::getCurrentHIPStream();
  int blocks = (int)std::min<long long>(4096, (n / 8 + 255) / 256);
  hipLaunchKernelGGL(fp8q::amax_bf16_kernel, dim3(std::max(blocks, 1)),
                     dim3(256), 0, stream.stream(),
                     reinterpret_cast<const short*>(x.data_ptr()), n, head,
                     reinterpret_cast<unsigned int*>(out.data_ptr()));
  HIP_CHECK_KERNEL();
  return out;
}

static void check_fp8_scale(const at::Tensor& scale, const at::Tensor& x) {
  CHECK_ARG(scale, at::kFloat);
  CHECK_ON(scale, x);
  TORCH_CHECK(scale.numel() == 1, "scale must hold one float");
}

at::Tensor fp8_cast(at::Tensor x, at::Tensor scale, bool e5m2) {
  CHECK_ARG(x, at::kBFloat16);
  check_fp8_scale(scale, x);
  TORCH_CHECK(x.numel() % 8 == 0 && ptr_aligned(x.data_ptr(), 16),
              "fp8_cast: numel must be 8-aligned and x 16-byte aligned");
  auto y = at::empty_like(x, x.options().dtype(at::kByte));
  long long n = x.numel();
  if (n == 0) return y;
  auto stream = c10::hip::getCurrentHIPStream();
  int blocks = (int)std::min<long long>(8192, (n / 8 + 255) / 256);
  float fmax = e5m2 ? 57344.f : 448.f;
  if (e5m2)
    hipLaunchKernelGGL(fp8q::fp8_cast_kernel<true>, dim3(blocks), dim3(256),
                       0, stream.stream(),
                       reinterpret_cast<const short*>(x.data_ptr()),
                       reinterpret_cast<unsigned int*>(y.data_ptr()), n,
                       scale.data_ptr<float>(), fmax);
  else
    hipLaunchKernelGGL(fp8q::fp8_cast_kernel<false>, dim3(blocks), dim3(256),
                       0, stream.stream(),
                       reinterpret_cast<const short*>(x.data_ptr()),
                       reinterpret_cast<unsigned int*>(y.data_ptr()), n,
                       scale.data_ptr<float>(), fmax);
  HIP_CHECK_KERNEL();
  return y;
}

std::vector<at::Tensor> fp8_cast_transpose(at::Tensor x, at::Tensor scale,
                                           bool e5m2) {
  CHECK_ARG(x, at::kBFloat16);
  check_fp8_scale(scale, x);
  TORCH_CHECK(x.dim() == 2 && x.numel() > 0,
              "fp8_cast_transpose: x must be a non-empty [M,K] matrix");
  int M = x.size(0), K = x.size(1);
  auto y = at::empty({M, K}, x.options().dtype(at::kByte));
  auto yt = at::empty({K, M}, x.options().dtype(at::kByte));
  const bool xvec = K % 8 == 0 && ptr_aligned(x.data_ptr(), 16);
  const bool yvec = K % 16 == 0 && ptr_aligned(y.data_ptr(), 16);
  const bool ytvec = M % 16 == 0 && ptr_aligned(yt.data_ptr(), 16);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((M + 63) / 64, (K + 63) / 64);
  float fmax = e5m2 ? 57344.f : 448.f;
  if (e5m2)
    hipLaunchKernelGGL(fp8q::fp8_cast_transpose_kernel<true>, grid,
                       dim3(256), 0, stream.stream(),
                       reinterpret_cast<const short*>(x.data_ptr()),
                       reinterpret_cast<unsigned char*>(y.data_ptr()),
                       reinterpret_cast<unsigned char*>(yt.data_ptr()),
                       M, K, scale.data_ptr<float>(), fmax, xvec, yvec,
                       ytvec);
  else
    hipLaunchKernelGGL(fp8q::fp8_cast_transpose_kernel<false>, grid,
                       dim3(256), 0, stream.stream(),
                       reinterpret_cast<const short*>(x.data_ptr()),
                       reinterpret_cast<unsigned char*>(y.data_ptr()),
                       reinterpret_cast<unsigned char*>(yt.data_ptr()),
                       M, K, scale.data_ptr<float>(), fmax, xvec, yvec,
                       ytvec);
  HIP_CHECK_KERNEL();
  return {y, yt};
}
