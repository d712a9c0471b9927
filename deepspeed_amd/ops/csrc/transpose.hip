// transpose_bf16: x[M,K] -> xT[K,M] for 2-byte elements, MI355X (gfx950).
//
// Why: the weight-gradient GEMM dW = dY^T X reduces over tokens, and neither
// row-major operand is contiguous along tokens; hipBLASLt then picks a slower
// kernel class than for the forward (profiles/README.md, "Weight-gradient
// GEMMs in the fast layout"). One read + one write per element puts an
// operand in the layout the fast class wants.
//
// 64x64 tiles through LDS, 256 threads, 16-byte global accesses on both
// sides. The tile is held as dwords (two adjacent columns each), row stride
// 33 dwords. Bank = dword address mod 64:
//   fill:  one ds_write_b32 per dword k of a 16-byte vector; the 64 lanes of
//          a wave hold vectors v = 0..7 of the rows {b..b+3, b+32..b+35}
//          (b a multiple of 4), whose row starts fall on banks
//          {0,33,2,35, 32,1,34,3} + b*33: every residue mod 4 on both
//          halves, and 4v + k fills the rest: 64 distinct banks.
//   drain: lane (rg, cp) reads dword column cp of rows 8rg..8rg+7, one row
//          per instruction; a wave holds rg = 0..7 and 8 consecutive cp, so
//          bank = 8*33*rg + cp + const = 8rg + cp + const: 64 distinct banks.
// The drain splits its 8 dwords into the low and the high halves: 8
// consecutive elements of two output rows, 16 bytes each.
//
// Rows that are not 16-byte aligned take the element-by-element arm of that
// side: xvec (K % 8 == 0 and x aligned), tvec (M % 8 == 0 and xT aligned),
// the pattern of fp8_cast_transpose.
#include <torch/extension.h>

#include "common.h"

namespace tr16 {

constexpr int TILE = 64;
constexpr int STRIDE = 33;  // dwords per tile row: 32 + 1 pad

__launch_bounds__(256)
__global__ void transpose_bf16_kernel(const short* __restrict__ x,
                                      short* __restrict__ xt, long long M,
                                      long long K, long long tiles_m,
                                      bool xvec, bool tvec) {
  __shared__ unsigned int tile[TILE * STRIDE];
  const long long tm = (long long)(blockIdx.x % tiles_m) * TILE;
  const long long tk = (long long)(blockIdx.x / tiles_m) * TILE;
  const int t = threadIdx.x;
  // fill: two passes of 256 vectors (8 shorts each)
  {
    const int v = t & 7;
    const int rr = (t >> 3) & 7;
    const int w = t >> 6;
    const int r0 = 8 * w + (rr & 3) + 32 * (rr >> 2);  // pass p: row r0 + 4p
    const long long gc = tk + v * 8;
    unsigned int d[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    if (xvec && tm + TILE <= M && tk + TILE <= K) {
      // interior tile: both loads in flight before the first LDS write
      const short* src = x + (tm + r0) * K + gc;
      uint4 q0 = *reinterpret_cast<const uint4*>(src);
      uint4 q1 = *reinterpret_cast<const uint4*>(src + 4 * K);
      d[0][0] = q0.x; d[0][1] = q0.y; d[0][2] = q0.z; d[0][3] = q0.w;
      d[1][0] = q1.x; d[1][1] = q1.y; d[1][2] = q1.z; d[1][3] = q1.w;
    } else {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const long long gr = tm + r0 + 4 * p;
        if (gr >= M) continue;
        const short* src = x + gr * K + gc;
        if (xvec && gc + 8 <= K) {
          uint4 q = *reinterpret_cast<const uint4*>(src);
          d[p][0] = q.x; d[p][1] = q.y; d[p][2] = q.z; d[p][3] = q.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (gc + j < K)
              d[p][j >> 1] |= (unsigned int)(unsigned short)src[j]
                              << (16 * (j & 1));
        }
      }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        tile[(r0 + 4 * p) * STRIDE + v * 4 + k] = d[p][k];
  }
  __syncthreads();
  // drain: lane (rg, cp) -> xt rows tk+2cp, tk+2cp+1, columns tm+8rg..+7
  {
    const int rg = t & 7;
    const int cp = t >> 3;
    unsigned int d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = tile[(rg * 8 + j) * STRIDE + cp];
    const long long gm = tm + rg * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long gk = tk + 2 * cp + h;
      if (gk >= K || gm >= M) continue;
      unsigned int o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = h ? ((d[2 * k] >> 16) | (d[2 * k + 1] & 0xffff0000u))
                 : ((d[2 * k] & 0xffffu) | (d[2 * k + 1] << 16));
      short* dst = xt + gk * M + gm;
      if (tvec && gm + 8 <= M) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (gm + j < M)
            dst[j] = (short)(o[j >> 1] >> (16 * (j & 1)));
      }
    }
  }
}

}  // namespace tr16

// x: a contiguous [M, K] device matrix of a 2-byte dtype (bf16 or fp16);
// returns a new contiguous [K, M] tensor. A non-contiguous x is refused.
at::Tensor transpose_bf16(at::Tensor x) {
  TORCH_CHECK(x.defined() && x.is_cuda() && x.dim() == 2 &&
                  x.element_size() == 2 && x.is_contiguous(),
              "transpose_bf16: x must be a contiguous [M,K] device matrix "
              "of a 2-byte dtype");
  const long long M = x.size(0), K = x.size(1);
  auto xt = at::empty({K, M}, x.options());
  if (M == 0 || K == 0) return xt;
  const long long tiles_m = (M + tr16::TILE - 1) / tr16::TILE;
  const long long tiles_k = (K + tr16::TILE - 1) / tr16::TILE;
  // HIP limits grid.x * block.x to 2^32 threads
  TORCH_CHECK(tiles_m * tiles_k < (1LL << 24),
              "transpose_bf16: matrix too large for one launch");
  const bool xvec = K % 8 == 0 && ptr_aligned(x.data_ptr(), 16);
  const bool tvec = M % 8 == 0 && ptr_aligned(xt.data_ptr(), 16);
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(tr16::transpose_bf16_kernel,
                     dim3((unsigned int)(tiles_m * tiles_k)), dim3(256), 0,
                     stream.stream(),
                     reinterpret_cast<const short*>(x.data_ptr()),
                     reinterpret_cast<short*>(xt.data_ptr()), M, K, tiles_m,
                     xvec, tvec);
  HIP_CHECK_KERNEL();
  return xt;
}
