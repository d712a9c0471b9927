// Fused RMSNorm / LayerNorm fwd+bwd for MI355X (gfx950).
//
// Role parity: reference csrc/transformer/inference/csrc/rms_norm.cu and
// csrc/transformer/normalize_kernels.cu. MI355X-native: one workgroup per
// row, bf16x8 vector loads (guide G13), wave64 shuffle + LDS reductions,
// fp32 math throughout. RMSNorm backward reads dy and x once: a fixed grid
// writes dx and per-workgroup dgamma partial rows, a small kernel sums the
// rows in a fixed order (no atomics, bit-reproducible). LayerNorm dgamma /
// dbeta: a separate column-sum kernel with coalesced column access.
#include <torch/extension.h>

#include "common.h"

// Row kernels may take the bf16x8 path only when every row start is 16-byte
// aligned: row stride a multiple of 8 elements and aligned base pointers.
static inline int row_vec_ok(int H, std::initializer_list<const void*> ptrs) {
  if (H % 8 != 0) return 0;
  for (const void* p : ptrs)
    if (!ptr_aligned(p, 16)) return 0;
  return 1;
}

static inline void check_norm_args(const at::Tensor& x, const at::Tensor& w) {
  CHECK_ARG(x, at::kBFloat16);
  CHECK_ARG(w, at::kBFloat16);
  CHECK_ON(w, x);
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0 && w.numel() == x.size(-1),
              "weight must have x.size(-1) elements");
}

// ---------------------------------------------------------------- RMSNorm
template <int BLOCK>
__global__ void rmsnorm_fwd_kernel(const short* __restrict__ x,
                                   const short* __restrict__ w,
                                   short* __restrict__ y,
                                   float* __restrict__ rstd_out, int H,
                                   float eps, int vec) {
  __shared__ float lds[BLOCK / WAVE];
  const long long row = blockIdx.x;
  const short* xr = x + row * (long long)H;
  short* yr = y + row * (long long)H;
  // vec: H % 8 == 0 and 16-byte-aligned bases (host-checked), else scalar
  int H8 = vec ? H / 8 : 0;
  float ss = 0.f;
  for (int i = threadIdx.x; i < H8; i += BLOCK) {
    bf16x8 v = reinterpret_cast<const bf16x8*>(xr)[i];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float f = bf2f(v.v[k]);
      ss += f * f;
    }
  }
  for (int i = H8 * 8 + threadIdx.x; i < H; i += BLOCK) {
    float f = bf2f(xr[i]);
    ss += f * f;
  }
  ss = block_reduce_sum<BLOCK>(ss, lds);
  float rstd = rsqrtf(ss / H + eps);
  if (threadIdx.x == 0 && rstd_out) rstd_out[row] = rstd;
  for (int i = threadIdx.x; i < H8; i += BLOCK) {
    bf16x8 v = reinterpret_cast<const bf16x8*>(xr)[i];
    bf16x8 wv = reinterpret_cast<const bf16x8*>(w)[i];
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      o.v[k] = f2bf(bf2f(v.v[k]) * rstd * bf2f(wv.v[k]));
    reinterpret_cast<bf16x8*>(yr)[i] = o;
  }
  for (int i = H8 * 8 + threadIdx.x; i < H; i += BLOCK)
    yr[i] = f2bf(bf2f(xr[i]) * rstd * bf2f(w[i]));
}

// dx = rstd * (dy*w - xhat * mean(dy*w*xhat))   where xhat = x*rstd
template <int BLOCK>
__global__ void rmsnorm_bwd_dx_kernel(const short* __restrict__ dy,
                                      const short* __restrict__ x,
                                      const short* __restrict__ w,
                                      const float* __restrict__ rstd,
                                      short* __restrict__ dx, int H,
                                      int vec) {
  __shared__ float lds[BLOCK / WAVE];
  const long long row = blockIdx.x;
  const short* dyr = dy + row * (long long)H;
  const short* xr = x + row * (long long)H;
  short* dxr = dx + row * (long long)H;
  float rs = rstd[row];
  // vec: H % 8 == 0 and 16-byte-aligned bases (host-checked), else scalar
  int H8 = vec ? H / 8 : 0;
  float dot = 0.f;
  for (int i = threadIdx.x; i < H8; i += BLOCK) {
    bf16x8 dv = reinterpret_cast<const bf16x8*>(dyr)[i];
    bf16x8 xv = reinterpret_cast<const bf16x8*>(xr)[i];
    bf16x8 wv = reinterpret_cast<const bf16x8*>(w)[i];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      dot += bf2f(dv.v[k]) * bf2f(wv.v[k]) * bf2f(xv.v[k]);
  }
  for (int i = H8 * 8 + threadIdx.x; i < H; i += BLOCK)
    dot += bf2f(dyr[i]) * bf2f(w[i]) * bf2f(xr[i]);
  dot = block_reduce_sum<BLOCK>(dot, lds);
  float c = dot * rs * rs / H;  // mean(dy*w*x) * rstd^2
  for (int i = threadIdx.x; i < H8; i += BLOCK) {
    bf16x8 dv = reinterpret_cast<const bf16x8*>(dyr)[i];
    bf16x8 xv = reinterpret_cast<const bf16x8*>(xr)[i];
    bf16x8 wv = reinterpret_cast<const bf16x8*>(w)[i];
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      o.v[k] = f2bf(rs * (bf2f(dv.v[k]) * bf2f(wv.v[k]) -
                          bf2f(xv.v[k]) * c));
    reinterpret_cast<bf16x8*>(dxr)[i] = o;
  }
  for (int i = H8 * 8 + threadIdx.x; i < H; i += BLOCK)
    dxr[i] = f2bf(rs * (bf2f(dyr[i]) * bf2f(w[i]) - bf2f(xr[i]) * c));
}

// One-pass backward: dx as above plus the dw partials, reading dy and x once.
// A fixed grid of workgroups each walks a contiguous chunk of rows. Thread t
// owns the 16-byte vectors t, t + BLOCK, ... of a row (NV of them) and keeps
// dy*x*rstd summed over its rows in NV*8 fp32 registers; the next row's dy/x
// are loaded before the current row's reduction so loads stay in flight.
// Each workgroup ends by storing its partial row part[blockIdx.x, :].
// Register limit: NV <= kRmsBwdMaxV, i.e. H <= 8 * BLOCK * kRmsBwdMaxV = 8192
// at BLOCK 256; wider rows take the two-kernel path below.
constexpr int kRmsBwdMaxV = 4;

template <int BLOCK, int NV>
__launch_bounds__(BLOCK)
__global__ void rmsnorm_bwd_fused_kernel(const short* __restrict__ dy,
                                         const short* __restrict__ x,
                                         const short* __restrict__ w,
                                         const float* __restrict__ rstd,
                                         short* __restrict__ dx,
                                         float* __restrict__ part,
                                         long long rows, long long per,
                                         int H) {
  __shared__ float lds[BLOCK / WAVE];
  const int H8 = H / 8;
  const long long r0 = blockIdx.x * per;
  const long long r1 = r0 + per < rows ? r0 + per : rows;
  bf16x8 wv[NV], dv[NV], xv[NV];
  float acc[NV][8];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = threadIdx.x + j * BLOCK;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
    if (i < H8) {
      wv[j] = reinterpret_cast<const bf16x8*>(w)[i];
      if (r0 < r1) {
        dv[j] = reinterpret_cast<const bf16x8*>(dy + r0 * H)[i];
        xv[j] = reinterpret_cast<const bf16x8*>(x + r0 * H)[i];
      }
    }
  }
  for (long long r = r0; r < r1; ++r) {
    const float rs = rstd[r];
    bf16x8 ndv[NV], nxv[NV];
    const bool more = r + 1 < r1;
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = threadIdx.x + j * BLOCK;
      if (i < H8) {
        if (more) {
          ndv[j] = reinterpret_cast<const bf16x8*>(dy + (r + 1) * H)[i];
          nxv[j] = reinterpret_cast<const bf16x8*>(x + (r + 1) * H)[i];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
          dot += bf2f(dv[j].v[k]) * bf2f(wv[j].v[k]) * bf2f(xv[j].v[k]);
      }
    }
    dot = block_reduce_sum<BLOCK>(dot, lds);
    const float c = dot * rs * rs / H;  // mean(dy*w*x) * rstd^2
    short* dxr = dx + r * H;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = threadIdx.x + j * BLOCK;
      if (i < H8) {
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = bf2f(dv[j].v[k]);
          const float xf = bf2f(xv[j].v[k]);
          o.v[k] = f2bf(rs * (d * bf2f(wv[j].v[k]) - xf * c));
          acc[j][k] += d * xf * rs;
        }
        reinterpret_cast<bf16x8*>(dxr)[i] = o;
        if (more) {
          dv[j] = ndv[j];
          xv[j] = nxv[j];
        }
      }
    }
  }
  float* pr = part + (long long)blockIdx.x * H;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = threadIdx.x + j * BLOCK;
    if (i < H8) {
      f32x4 lo = {{acc[j][0], acc[j][1], acc[j][2], acc[j][3]}};
      f32x4 hi = {{acc[j][4], acc[j][5], acc[j][6], acc[j][7]}};
      reinterpret_cast<f32x4*>(pr)[2 * i] = lo;
      reinterpret_cast<f32x4*>(pr)[2 * i + 1] = hi;
    }
  }
}

// Two-kernel path (scalar rows, or H past the register limit above), dw half:
// part[y, c] = sum over rows r = y, y + gridDim.y, ... of dy*x*rstd;
// column-parallel, coalesced: consecutive lanes take consecutive columns.
__global__ void rmsnorm_bwd_dw_partial_kernel(const short* __restrict__ dy,
                                              const short* __restrict__ x,
                                              const float* __restrict__ rstd,
                                              float* __restrict__ part,
                                              long long rows, int H) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= H) return;
  float acc = 0.f;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    long long idx = r * H + c;
    acc += bf2f(dy[idx]) * bf2f(x[idx]) * rstd[r];
  }
  part[(long long)blockIdx.y * H + c] = acc;
}

// dw[c] = sum_p part[p, c], in a fixed order (no atomics: bit-reproducible).
// Workgroup: 32 columns x BLOCK/32 groups of partial rows, then LDS.
template <int BLOCK>
__launch_bounds__(BLOCK)
__global__ void colsum_partials_kernel(const float* __restrict__ part,
                                       int nparts, int H,
                                       float* __restrict__ dw) {
  constexpr int COLS = 32;
  constexpr int NG = BLOCK / COLS;
  __shared__ float lds[BLOCK];
  const int cx = threadIdx.x % COLS;
  const int g = threadIdx.x / COLS;
  const int c = blockIdx.x * COLS + cx;
  float acc = 0.f;
  if (c < H) {
#pragma unroll 8
    for (int p = g; p < nparts; p += NG) acc += part[(long long)p * H + c];
  }
  lds[threadIdx.x] = acc;
  __syncthreads();
  if (g == 0 && c < H) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NG; ++k) s += lds[k * COLS + cx];
    dw[c] = s;
  }
}

// Workgroups for the one-pass backward: a few per CU, independent of rows.
static int rms_bwd_max_blocks() {
  static int cached[64] = {0};
  int dev = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess, "hipGetDevice failed");
  if (dev < 0 || dev >= 64) return 1024;
  if (cached[dev] == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || cus <= 0)
      cus = 256;
    cached[dev] = 4 * cus;
  }
  return cached[dev];
}

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  check_norm_args(x, w);
  int H = x.size(-1);
  long long rows = x.numel() / H;
  auto y = at::empty_like(x);
  auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  if (rows == 0) return {y, rstd};
  auto stream = c10::hip::getCurrentHIPStream();
  constexpr int BLOCK = 256;
  int vec = row_vec_ok(H, {x.data_ptr(), w.data_ptr(), y.data_ptr()});
  hipLaunchKernelGGL(rmsnorm_fwd_kernel<BLOCK>, dim3(rows), dim3(BLOCK), 0,
                     stream.stream(),
                     reinterpret_cast<const short*>(x.data_ptr()),
                     reinterpret_cast<const short*>(w.data_ptr()),
                     reinterpret_cast<short*>(y.data_ptr()),
                     rstd.data_ptr<float>(), H, (float)eps, vec);
  HIP_CHECK_KERNEL();
  return {y, rstd};
}

std::vector<at::Tensor> rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                    at::Tensor rstd) {
  check_norm_args(x, w);
  CHECK_ARG(dy, at::kBFloat16);
  CHECK_LIKE(dy, x);
  CHECK_ARG(rstd, at::kFloat);
  CHECK_ON(rstd, x);
  int H = x.size(-1);
  long long rows = x.numel() / H;
  TORCH_CHECK(rstd.numel() == rows, "rstd must have one entry per row");
  auto dx = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  if (rows == 0) return {dx, at::zeros({H}, fopt)};
  auto dw = at::empty({H}, fopt);
  auto stream = c10::hip::getCurrentHIPStream();
  constexpr int BLOCK = 256;
  int vec = row_vec_ok(
      H, {dy.data_ptr(), x.data_ptr(), w.data_ptr(), dx.data_ptr()});
  const short* dyp = reinterpret_cast<const short*>(dy.data_ptr());
  const short* xp = reinterpret_cast<const short*>(x.data_ptr());
  const short* wp = reinterpret_cast<const short*>(w.data_ptr());
  short* dxp = reinterpret_cast<short*>(dx.data_ptr());
  const int nv = (H / 8 + BLOCK - 1) / BLOCK;
  at::Tensor part;  // [nparts, H] fp32, fully written by either path
  int nparts;
  if (vec && nv <= kRmsBwdMaxV) {
    const long long maxb = rms_bwd_max_blocks();
    const long long per = (rows + maxb - 1) / maxb;
    nparts = (int)((rows + per - 1) / per);
    part = at::empty({nparts, H}, fopt);
    auto kern = nv == 1   ? rmsnorm_bwd_fused_kernel<BLOCK, 1>
                : nv == 2 ? rmsnorm_bwd_fused_kernel<BLOCK, 2>
                          : rmsnorm_bwd_fused_kernel<BLOCK, 4>;
    hipLaunchKernelGGL(kern, dim3(nparts), dim3(BLOCK), 0, stream.stream(),
                       dyp, xp, wp, rstd.data_ptr<float>(), dxp,
                       part.data_ptr<float>(), rows, per, H);
    HIP_CHECK_KERNEL();
  } else {
    hipLaunchKernelGGL(rmsnorm_bwd_dx_kernel<BLOCK>, dim3(rows), dim3(BLOCK),
                       0, stream.stream(), dyp, xp, wp,
                       rstd.data_ptr<float>(), dxp, H, vec);
    HIP_CHECK_KERNEL();
    nparts = rows > 4096 ? 64 : (rows > 512 ? 16 : 1);
    part = at::empty({nparts, H}, fopt);
    hipLaunchKernelGGL(rmsnorm_bwd_dw_partial_kernel,
                       dim3((H + 255) / 256, nparts), dim3(256), 0,
                       stream.stream(), dyp, xp, rstd.data_ptr<float>(),
                       part.data_ptr<float>(), rows, H);
    HIP_CHECK_KERNEL();
  }
  constexpr int RB = 1024;
  hipLaunchKernelGGL(colsum_partials_kernel<RB>, dim3((H + 31) / 32),
                     dim3(RB), 0, stream.stream(), part.data_ptr<float>(),
                     nparts, H, dw.data_ptr<float>());
  HIP_CHECK_KERNEL();
  return {dx, dw};
}

// --------------------------------------------------------------- LayerNorm
template <int BLOCK>
__global__ void layernorm_fwd_kernel(const short* __restrict__ x,
                                     const short* __restrict__ w,
                                     const short* __restrict__ b,
                                     short* __restrict__ y,
                                     float* __restrict__ mean_out,
                                     float* __restrict__ rstd_out, int H,
                                     float eps) {
  __shared__ float lds[BLOCK / WAVE];
  const long long row = blockIdx.x;
  const short* xr = x + row * (long long)H;
  short* yr = y + row * (long long)H;
  float s = 0.f;
  for (int i = threadIdx.x; i < H; i += BLOCK) s += bf2f(xr[i]);
  s = block_reduce_sum<BLOCK>(s, lds);
  float mean = s / H;
  // two-pass variance: E[x^2] - mean^2 loses |mean|^2/var of the fp32
  // mantissa (rows with a large offset); the row is L2-hot on re-read
  float ss = 0.f;
  for (int i = threadIdx.x; i < H; i += BLOCK) {
    float d = bf2f(xr[i]) - mean;
    ss += d * d;
  }
  ss = block_reduce_sum<BLOCK>(ss, lds);
  float var = ss / H;
  float rstd = rsqrtf(var + eps);
  if (threadIdx.x == 0) {
    if (mean_out) mean_out[row] = mean;
    if (rstd_out) rstd_out[row] = rstd;
  }
  for (int i = threadIdx.x; i < H; i += BLOCK) {
    float xhat = (bf2f(xr[i]) - mean) * rstd;
    float o = xhat * bf2f(w[i]) + (b ? bf2f(b[i]) : 0.f);
    yr[i] = f2bf(o);
  }
}

template <int BLOCK>
__global__ void layernorm_bwd_dx_kernel(
    const short* __restrict__ dy, const short* __restrict__ x,
    const short* __restrict__ w, const float* __restrict__ mean,
    const float* __restrict__ rstd, short* __restrict__ dx, int H) {
  __shared__ float lds[BLOCK / WAVE];
  const long long row = blockIdx.x;
  const short* dyr = dy + row * (long long)H;
  const short* xr = x + row * (long long)H;
  short* dxr = dx + row * (long long)H;
  float mu = mean[row], rs = rstd[row];
  float c1 = 0.f, c2 = 0.f;
  for (int i = threadIdx.x; i < H; i += BLOCK) {
    float g = bf2f(dyr[i]) * bf2f(w[i]);
    float xhat = (bf2f(xr[i]) - mu) * rs;
    c1 += g;
    c2 += g * xhat;
  }
  c1 = block_reduce_sum<BLOCK>(c1, lds) / H;
  c2 = block_reduce_sum<BLOCK>(c2, lds) / H;
  for (int i = threadIdx.x; i < H; i += BLOCK) {
    float g = bf2f(dyr[i]) * bf2f(w[i]);
    float xhat = (bf2f(xr[i]) - mu) * rs;
    dxr[i] = f2bf((g - c1 - xhat * c2) * rs);
  }
}

__global__ void layernorm_bwd_dwdb_kernel(const short* __restrict__ dy,
                                          const short* __restrict__ x,
                                          const float* __restrict__ mean,
                                          const float* __restrict__ rstd,
                                          float* __restrict__ dw,
                                          float* __restrict__ db,
                                          long long rows, int H) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= H) return;
  float accw = 0.f, accb = 0.f;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    long long idx = r * H + c;
    float d = bf2f(dy[idx]);
    accw += d * (bf2f(x[idx]) - mean[r]) * rstd[r];
    accb += d;
  }
  if (gridDim.y == 1) {
    dw[c] = accw;
    db[c] = accb;
  } else {
    atomicAdd(dw + c, accw);
    atomicAdd(db + c, accb);
  }
}

std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor w,
                                      c10::optional<at::Tensor> b,
                                      double eps) {
  check_norm_args(x, w);
  if (b.has_value()) {
    CHECK_ARG(*b, at::kBFloat16);
    CHECK_LIKE(*b, w);
  }
  int H = x.size(-1);
  long long rows = x.numel() / H;
  auto y = at::empty_like(x);
  auto mean = at::empty({rows}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  if (rows == 0) return {y, mean, rstd};
  auto stream = c10::hip::getCurrentHIPStream();
  constexpr int BLOCK = 256;
  hipLaunchKernelGGL(
      layernorm_fwd_kernel<BLOCK>, dim3(rows), dim3(BLOCK), 0,
      stream.stream(), reinterpret_cast<const short*>(x.data_ptr()),
      reinterpret_cast<const short*>(w.data_ptr()),
      b.has_value() ? reinterpret_cast<const short*>(b->data_ptr()) : nullptr,
      reinterpret_cast<short*>(y.data_ptr()), mean.data_ptr<float>(),
      rstd.data_ptr<float>(), H, (float)eps);
  HIP_CHECK_KERNEL();
  return {y, mean, rstd};
}

std::vector<at::Tensor> layernorm_bwd(at::Tensor dy, at::Tensor x,
                                      at::Tensor w, at::Tensor mean,
                                      at::Tensor rstd) {
  check_norm_args(x, w);
  CHECK_ARG(dy, at::kBFloat16);
  CHECK_LIKE(dy, x);
  CHECK_ARG(mean, at::kFloat);
  CHECK_ARG(rstd, at::kFloat);
  CHECK_ON(mean, x);
  CHECK_ON(rstd, x);
  int H = x.size(-1);
  long long rows = x.numel() / H;
  TORCH_CHECK(mean.numel() == rows && rstd.numel() == rows,
              "mean/rstd must have one entry per row");
  auto dx = at::empty_like(x);
  auto dw = at::zeros({H}, x.options().dtype(at::kFloat));
  auto db = at::zeros({H}, x.options().dtype(at::kFloat));
  if (rows == 0) return {dx, dw, db};
  auto stream = c10::hip::getCurrentHIPStream();
  constexpr int BLOCK = 256;
  hipLaunchKernelGGL(layernorm_bwd_dx_kernel<BLOCK>, dim3(rows), dim3(BLOCK),
                     0, stream.stream(),
                     reinterpret_cast<const short*>(dy.data_ptr()),
                     reinterpret_cast<const short*>(x.data_ptr()),
                     reinterpret_cast<const short*>(w.data_ptr()),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     reinterpret_cast<short*>(dx.data_ptr()), H);
  HIP_CHECK_KERNEL();
  int gy = rows > 4096 ? 64 : (rows > 512 ? 16 : 1);
  hipLaunchKernelGGL(layernorm_bwd_dwdb_kernel, dim3((H + 255) / 256, gy),
                     dim3(256), 0, stream.stream(),
                     reinterpret_cast<const short*>(dy.data_ptr()),
                     reinterpret_cast<const short*>(x.data_ptr()),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     dw.data_ptr<float>(), db.data_ptr<float>(), rows, H);
  HIP_CHECK_KERNEL();
  return {dx, dw, db};
}
