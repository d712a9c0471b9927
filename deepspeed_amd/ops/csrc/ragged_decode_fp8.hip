// Ragged-batch decode attention over the fp8 KV slot pool (gfx950).
//
// Same split-KV scheme, grid, partials, combine kernel and output layout as
// ragged_decode (ragged_decode.hip); the pools hold e4m3fn codes with one
// fp32 scale per (slot, position, kv head), format in kv_fp8.h:
//   score = (q . code_k) * k_scale[pos] * softmax_scale
//   O    += p * v_scale[pos] * code_v
//
// Lane layout. In the bf16 kernel a lane owns D/64 dims, which over a fp8 row
// would be a 1- or 2-byte load per lane. Here D/8 lanes cover a row with one
// 8-byte load each (16 lanes at D = 128, 8 at D = 64), so a wave reads 64*8/D
// rows per load and the q.k dot is a D/8-lane butterfly instead of a 64-lane
// one. Each row group keeps its own online-softmax state (m, l, acc); the
// groups of a wave are merged with a __shfl_xor butterfly before the 4 waves
// merge in LDS the way ragged_decode_kernel does.
//
// Only positions < len are ever loaded, codes and scales alike, so whatever
// sits past a slot's length (NaN codes, NaN / inf scales, another request's
// rows) cannot reach a live value.
#include <torch/extension.h>

#include "kv_fp8.h"

namespace raggedfp8 {

constexpr int MAXG = 8;  // max q-heads per kv head handled per block

// q [n, Hq, D] bf16, kpool/vpool [B, Smax, Hk, D] e4m3fn bytes,
// kscale/vscale [B, Smax, Hk] f32, rows [n] i64, lens [n] i64,
// partial_out [n, Hq, NS, D] f32, partial_ml [n, Hq, NS, 2] f32
template <int D, int G>
__launch_bounds__(256)
__global__ void ragged_decode_fp8_kernel(
    const short* __restrict__ q, const unsigned char* __restrict__ kpool,
    const unsigned char* __restrict__ vpool, const float* __restrict__ kscale,
    const float* __restrict__ vscale, const int64_t* __restrict__ rows,
    const int64_t* __restrict__ lens, float* __restrict__ partial_out,
    float* __restrict__ partial_ml, int Hq, int Hk, int Smax, int NS,
    int chunk, float scale) {
  constexpr int LPR = D / 8;    // lanes per kv row, 8 codes each
  constexpr int RPW = 64 / LPR; // kv rows per wave load
  constexpr int DL = D / 64;    // dims per lane in the wave merge
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int li = lane & (LPR - 1);  // 8-dim group inside the row
  const int rg = lane / LPR;        // row group inside the wave
  const int r = blockIdx.x;       // active-row index
  const int hk = blockIdx.y;      // kv head
  const int cidx = blockIdx.z;    // kv chunk
  const long long slot = rows[r];
  const int len = (int)lens[r];
  const int c0 = cidx * chunk;
  if (c0 >= len && cidx > 0) {
    // no work: mark partials empty
    if (threadIdx.x < G * 2) {
      int g = threadIdx.x / 2;
      int hq = hk * G + g;
      partial_ml[(((long long)r * Hq + hq) * NS + cidx) * 2 +
                 (threadIdx.x & 1)] = (threadIdx.x & 1) ? 0.f : -INFINITY;
    }
    return;
  }
  const int c1 = min(len, c0 + chunk);
  // wave's sub-range
  const int per_wave = (c1 - c0 + 3) / 4;
  const int w0 = c0 + wave * per_wave;
  const int w1 = min(c1, w0 + per_wave);

  const long long kvrs = (long long)Hk * D;  // bytes per position
  const unsigned char* kbase = kpool + (slot * Smax) * kvrs + hk * D + li * 8;
  const unsigned char* vbase = vpool + (slot * Smax) * kvrs + hk * D + li * 8;
  const float* ksb = kscale + (slot * Smax) * Hk + hk;
  const float* vsb = vscale + (slot * Smax) * Hk + hk;

  // q fragments: G heads, this lane's 8 dims, pre-scaled
  float qf[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const bf16x8 qv = *reinterpret_cast<const bf16x8*>(
        q + ((long long)r * Hq + hk * G + g) * D + li * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[g][j] = bf2f(qv.v[j]) * scale;
  }

  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
  }

  // the LPR lanes of a row group share p, so they loop and branch together
  for (int p = w0 + rg; p < w1; p += RPW) {
    const uint2 kc =
        *reinterpret_cast<const uint2*>(kbase + (long long)p * kvrs);
    const uint2 vc =
        *reinterpret_cast<const uint2*>(vbase + (long long)p * kvrs);
    const float ks = ksb[(long long)p * Hk];
    const float vs = vsb[(long long)p * Hk];
    float kf[8], vf[8];
    kvfp8::unpack8(kc, kf);
    kvfp8::unpack8(vc, vf);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d += qf[g][j] * kf[j];
#pragma unroll
      for (int off = LPR / 2; off > 0; off >>= 1)
        d += __shfl_xor(d, off, WAVE);
      const float s = d * ks;
      if (s > m[g]) {
        float c = (m[g] == -INFINITY) ? 0.f : __expf(m[g] - s);
        l[g] *= c;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] *= c;
        m[g] = s;
      }
      const float pv = __expf(s - m[g]);
      l[g] += pv;  // the row sum stays unscaled
      const float w = pv * vs;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] += w * vf[j];
    }
  }

  // merge the RPW row groups of this wave (all 64 lanes are back together)
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float m2 = __shfl_xor(m[g], off, WAVE);
      const float l2 = __shfl_xor(l[g], off, WAVE);
      const float mn = fmaxf(m[g], m2);
      const float ca = (m[g] == -INFINITY) ? 0.f : __expf(m[g] - mn);
      const float cb = (m2 == -INFINITY) ? 0.f : __expf(m2 - mn);
      l[g] = l[g] * ca + l2 * cb;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a2 = __shfl_xor(acc[g][j], off, WAVE);
        acc[g][j] = acc[g][j] * ca + a2 * cb;
      }
      m[g] = mn;
    }
  }

  // combine the 4 waves in LDS: per (g): m, l, acc[D]
  __shared__ float lm[4][MAXG], ll[4][MAXG];
  __shared__ float lacc[4][MAXG][D];
  if (rg == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (lane == 0) {
        lm[wave][g] = m[g];
        ll[wave][g] = l[g];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) lacc[wave][g][li * 8 + j] = acc[g][j];
    }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mw = fmaxf(fmaxf(lm[0][g], lm[1][g]),
                       fmaxf(lm[2][g], lm[3][g]));
      float lw = 0.f;
      float o[DL];
#pragma unroll
      for (int j = 0; j < DL; ++j) o[j] = 0.f;
      for (int wv = 0; wv < 4; ++wv) {
        float mi = lm[wv][g];
        if (mi == -INFINITY) continue;
        float c = __expf(mi - mw);
        lw += ll[wv][g] * c;
#pragma unroll
        for (int j = 0; j < DL; ++j)
          o[j] += lacc[wv][g][lane * DL + j] * c;
      }
      int hq = hk * G + g;
      long long ob = (((long long)r * Hq + hq) * NS + cidx) * D + lane * DL;
#pragma unroll
      for (int j = 0; j < DL; ++j) partial_out[ob + j] = o[j];
      if (lane == 0) {
        long long mb = (((long long)r * Hq + hq) * NS + cidx) * 2;
        partial_ml[mb] = mw;
        partial_ml[mb + 1] = lw;
      }
    }
  }
}

// merge NS chunk partials -> out [n, Hq, D] bf16; one wave per (r, hq).
// Same arithmetic as ragged_combine_kernel (ragged_decode.hip).
template <int D>
__global__ void ragged_combine_fp8_kernel(
    const float* __restrict__ partial_out,
    const float* __restrict__ partial_ml, short* __restrict__ out,
    long long nhq, int NS) {
  constexpr int DL = D / 64;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long rh = (long long)blockIdx.x * 4 + wave;  // over n*Hq
  if (rh >= nhq) return;
  float mstar = -INFINITY;
  for (int c = 0; c < NS; ++c)
    mstar = fmaxf(mstar, partial_ml[(rh * NS + c) * 2]);
  float lsum = 0.f;
  float o[DL];
#pragma unroll
  for (int j = 0; j < DL; ++j) o[j] = 0.f;
  for (int c = 0; c < NS; ++c) {
    float mi = partial_ml[(rh * NS + c) * 2];
    if (mi == -INFINITY) continue;
    float li = partial_ml[(rh * NS + c) * 2 + 1];
    float sc = __expf(mi - mstar);
    lsum += li * sc;
    const float* po = partial_out + (rh * NS + c) * D + lane * DL;
#pragma unroll
    for (int j = 0; j < DL; ++j) o[j] += po[j] * sc;
  }
  float inv = lsum > 0.f ? 1.f / lsum : 0.f;
#pragma unroll
  for (int j = 0; j < DL; ++j)
    out[rh * D + lane * DL + j] = f2bf(o[j] * inv);
}

}  // namespace raggedfp8

at::Tensor ragged_decode_fp8(at::Tensor q, at::Tensor kpool, at::Tensor vpool,
                             at::Tensor k_scale, at::Tensor v_scale,
                             at::Tensor rows, at::Tensor lens, long chunk) {
  CHECK_ARG(q, at::kBFloat16);
  CHECK_ARG(kpool, at::kFloat8_e4m3fn);
  CHECK_ARG(vpool, at::kFloat8_e4m3fn);
  CHECK_ARG(k_scale, at::kFloat);
  CHECK_ARG(v_scale, at::kFloat);
  CHECK_ARG(rows, at::kLong);
  CHECK_ARG(lens, at::kLong);
  CHECK_ON(kpool, q);
  CHECK_ON(vpool, q);
  CHECK_ON(k_scale, q);
  CHECK_ON(v_scale, q);
  CHECK_ON(rows, q);
  CHECK_ON(lens, q);
  TORCH_CHECK((q.dim() == 4 && q.size(1) == 1) || q.dim() == 3,
              "ragged_decode_fp8: q must be [n,1,Hq,D] or [n,Hq,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(),
              "ragged_decode_fp8: kpool and vpool must both be "
              "[B,Smax,Hk,D]");
  TORCH_CHECK(chunk >= 1, "ragged_decode_fp8: chunk must be >= 1");
  int n = q.size(0);
  int Hq = q.size(-2), D = q.size(-1);
  int Smax = kpool.size(1), Hk = kpool.size(2);
  TORCH_CHECK(n >= 1 && Hk >= 1 && kpool.size(3) == D,
              "ragged_decode_fp8: empty batch or pool head_dim != q "
              "head_dim");
  TORCH_CHECK(k_scale.dim() == 3 && k_scale.size(0) == kpool.size(0) &&
                  k_scale.size(1) == Smax && k_scale.size(2) == Hk &&
                  v_scale.sizes() == k_scale.sizes(),
              "ragged_decode_fp8: k_scale and v_scale must both be "
              "[B,Smax,Hk]");
  TORCH_CHECK(rows.numel() == n && lens.numel() == n,
              "ragged_decode_fp8: rows and lens must have one entry per q "
              "row");
  int G = Hq / Hk;
  TORCH_CHECK(Hq % Hk == 0 && G <= raggedfp8::MAXG,
              "ragged_decode_fp8: GQA group too large");
  TORCH_CHECK(D == 128 || D == 64,
              "ragged_decode_fp8: head_dim must be 64 or 128");
  TORCH_CHECK(ptr_aligned(q.data_ptr(), 16) &&
                  ptr_aligned(kpool.data_ptr(), 8) &&
                  ptr_aligned(vpool.data_ptr(), 8),
              "ragged_decode_fp8: q must be 16-byte and the pools 8-byte "
              "aligned");
  long maxlen = lens.max().item<long>();
  TORCH_CHECK(maxlen >= 1, "ragged_decode_fp8: every row is empty");
  TORCH_CHECK(maxlen <= Smax, "ragged_decode_fp8: lens.max() = ", maxlen,
              " exceeds the pool's Smax = ", Smax);
  int NS = (int)std::min<long>((maxlen + chunk - 1) / chunk, 64);
  int eff_chunk = (int)((maxlen + NS - 1) / NS);
  eff_chunk = (eff_chunk + 3) & ~3;
  auto opts = q.options().dtype(at::kFloat);
  auto pout = at::empty({n, Hq, NS, D}, opts);
  auto pml = at::empty({n, Hq, NS, 2}, opts);
  auto out = at::empty({n, 1, Hq, D}, q.options());
  float scale = 1.0f / std::sqrt((float)D);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid(n, Hk, NS);

#define LAUNCH(DD, GG)                                                       \
  hipLaunchKernelGGL((raggedfp8::ragged_decode_fp8_kernel<DD, GG>), grid,    \
                     dim3(256), 0, stream.stream(),                          \
                     reinterpret_cast<const short*>(q.data_ptr()),           \
                     reinterpret_cast<const unsigned char*>(                 \
                         kpool.data_ptr()),                                  \
                     reinterpret_cast<const unsigned char*>(                 \
                         vpool.data_ptr()),                                  \
                     k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),   \
                     rows.data_ptr<int64_t>(), lens.data_ptr<int64_t>(),     \
                     pout.data_ptr<float>(), pml.data_ptr<float>(), Hq, Hk,  \
                     Smax, NS, eff_chunk, scale)

  bool done = false;
  if (D == 128) {
    switch (G) {
      case 1: LAUNCH(128, 1); done = true; break;
      case 2: LAUNCH(128, 2); done = true; break;
      case 4: LAUNCH(128, 4); done = true; break;
      case 8: LAUNCH(128, 8); done = true; break;
    }
  } else {
    switch (G) {
      case 1: LAUNCH(64, 1); done = true; break;
      case 2: LAUNCH(64, 2); done = true; break;
      case 4: LAUNCH(64, 4); done = true; break;
      case 8: LAUNCH(64, 8); done = true; break;
    }
  }
#undef LAUNCH
  TORCH_CHECK(done, "ragged_decode_fp8: unsupported GQA group ", G);
  HIP_CHECK_KERNEL();

  const long long nhq = (long long)n * Hq;
  dim3 gridc((unsigned)((nhq + 3) / 4));
  if (D == 128)
    hipLaunchKernelGGL(raggedfp8::ragged_combine_fp8_kernel<128>, gridc,
                       dim3(256), 0, stream.stream(), pout.data_ptr<float>(),
                       pml.data_ptr<float>(),
                       reinterpret_cast<short*>(out.data_ptr()), nhq, NS);
  else
    hipLaunchKernelGGL(raggedfp8::ragged_combine_fp8_kernel<64>, gridc,
                       dim3(256), 0, stream.stream(), pout.data_ptr<float>(),
                       pml.data_ptr<float>(),
                       reinterpret_cast<short*>(out.data_ptr()), nhq, NS);
  HIP_CHECK_KERNEL();
  return out;
}
