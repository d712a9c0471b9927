// Ragged prefill attention over the KV slot pool for MI355X (gfx950).
//
// Role parity: reference inference/v2 blocked flash attention with
// per-sequence "atoms" (deepspeed/inference/v2/kernels/ragged_ops/).
// MI355X-native design: ONE call serves every sequence of a serving step --
// fresh prompts, prompt chunks over a cached prefix and single-token decode
// rows -- reading K/V STRAIGHT from the slot pool [B, Smax, Hk, D] that
// ragged_decode reads (the step's new rows are already written there). A
// device descriptor per sequence (slot, q_start, q_len, kv_len) replaces the
// host-built [1,1,S,total] masks and the pool slices of the per-chunk path.
//
// Local token j of a sequence lives at q[q_start + j], has position
// p = kv_len - q_len + j and attends to pool positions 0..p of its slot.
//
// Shape: grid (ceil(max_qlen/32), n, Hq), 4 waves per block. A block owns one
// 32-token q tile of one sequence and one q head; its waves split the KV
// tiles of 64 (wave w takes tiles w, w+4, ...) and merge (m, l, O) in LDS the
// way ragged_decode_kernel does. Fragment layouts and the in-register P build
// are those documented at the top of attention.hip; V is transposed by hand
// into a padded [D][64+8] image (vtswz below), as the training forward did
// before it moved to hardware-transposed reads:
//   S^T = K Q^T  (C col = q = lane&31, so the softmax row is lane-local),
//   O^T = V^T P^T with V^T staged per wave in LDS.
// K fragments are read straight from the pool (a lane's 8 k-values are 16
// contiguous bytes of one pool row).
//
// Masking is per element and by SELECT: a column > p contributes exactly 0
// (never exp(-inf) * x). No position >= the tile's last visible column is
// ever loaded -- K rows past it are clamped onto it, V rows past it are
// zeros -- so NaN (or another request's data) beyond kv_len cannot leak.
#include <torch/extension.h>

#include "common.h"

namespace rprefill {

using bf16x8_t = __attribute__((ext_vector_type(8))) short;
using f32x16_t = __attribute__((ext_vector_type(16))) float;
#define RP_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16

constexpr int QT = 32;      // q tokens per block
constexpr int KT = 64;      // kv rows per tile
constexpr int NW = 4;       // waves per block
constexpr int VT_PAD = 8;   // Vt rows padded: [D][64+8]
constexpr int OPAD = 4;     // merge rows padded: [32][D+4] floats

// Vt[d][kv] byte offset: pad-8 rows spread the d-read and the ((d>>5)&3)<<5
// XOR spreads the 4 d-groups on the transpose write (~2-way)
DEV_INLINE int vtswz(int d, int kv_byte) {
  return d * ((KT + VT_PAD) * 2) + (kv_byte ^ (((d >> 5) & 3) << 5));
}

DEV_INLINE float half_swap(float x, int hi) {
  int i = __builtin_bit_cast(int, x);
  auto r = __builtin_amdgcn_permlane32_swap(i, i, false, false);
  return __builtin_bit_cast(float, hi ? r[0] : r[1]);
}

DEV_INLINE unsigned int cvtpk2(float lo, float hi) {
  unsigned short a = __builtin_bit_cast(unsigned short, (__bf16)lo);
  unsigned short b = __builtin_bit_cast(unsigned short, (__bf16)hi);
  return (unsigned int)a | ((unsigned int)b << 16);
}

template <int D>
struct Smem {
  static constexpr int VT_BYTES = D * (KT + VT_PAD) * 2;       // per wave
  static constexpr int ACC_BYTES = NW * QT * (D + OPAD) * 4;   // merge O
  static constexpr int ML_BYTES = NW * QT * 2 * 4;             // merge m, l
  static constexpr int BYTES = NW * VT_BYTES > ACC_BYTES + ML_BYTES
                                   ? NW * VT_BYTES
                                   : ACC_BYTES + ML_BYTES;
};

// q [T,Hq,D] bf16, kpool/vpool [B,Smax,Hk,D] bf16, desc [n,4] i64
// (slot, q_start, q_len, kv_len), out [T,Hq,D] bf16.
template <int D>
__launch_bounds__(256)
__global__ void ragged_prefill_kernel(
    const short* __restrict__ q, const short* __restrict__ kpool,
    const short* __restrict__ vpool, const int64_t* __restrict__ desc,
    short* __restrict__ out, int T, int Hq, int Hk, int B, int Smax,
    int max_kvlen, float scale) {
  __shared__ __attribute__((aligned(16))) char smem[Smem<D>::BYTES];

  constexpr int NQF = D / 16;  // Q k-slices
  constexpr int NOT = D / 32;  // O^T d m-tiles

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  const int qt = blockIdx.x;
  const int seq = blockIdx.y;
  const int h = blockIdx.z;
  const int hk = h / (Hq / Hk);

  const long long slot = desc[seq * 4 + 0];
  const long long q_start = desc[seq * 4 + 1];
  const long long q_len64 = desc[seq * 4 + 2];
  const long long kv_len64 = desc[seq * 4 + 3];
  // RaggedBatch validates descriptors on the host; a row that breaks the
  // contract anyway is skipped, so no address below can leave q or the pool.
  if (slot < 0 || slot >= B || q_len64 < 1 || kv_len64 < q_len64 ||
      kv_len64 > max_kvlen || kv_len64 > Smax || q_start < 0 ||
      q_start + q_len64 > T)
    return;
  const int q_len = (int)q_len64;
  const int kv_len = (int)kv_len64;
  const int j0 = qt * QT;
  if (j0 >= q_len) return;  // tile past this sequence's tokens

  const int my_j = j0 + l31;
  const bool my_valid = my_j < q_len;
  // this lane's last visible column; -1 hides every column from a pad lane
  const int my_p = my_valid ? kv_len - q_len + my_j : -1;
  // columns visible to the tile's last token: 0 .. kv_end-1 (< kv_len)
  const int j_last = min(q_len, j0 + QT) - 1;
  const int kv_end = kv_len - q_len + j_last + 1;
  const int n_tiles = (kv_end + KT - 1) / KT;

  const long long qrs = (long long)Hq * D;
  const long long kvrs = (long long)Hk * D;
  const short* kp = kpool + (slot * Smax) * kvrs + hk * D;
  const short* vp = vpool + (slot * Smax) * kvrs + hk * D;

  // ---- Q fragments: qfrag[ks] = Q[my_j][16*ks + hi*8 .. +7] ---------------
  bf16x8_t qfrag[NQF];
  {
    const int sj = my_valid ? my_j : q_len - 1;
    const short* src = q + (q_start + sj) * qrs + h * D + hi * 8;
#pragma unroll
    for (int ks = 0; ks < NQF; ++ks)
      qfrag[ks] = *reinterpret_cast<const bf16x8_t*>(src + 16 * ks);
  }

  const float sc2 = scale * 1.44269504f;  // exp2 domain
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t ot[NOT];  // O^T accum: rows d = 32*mt + (reg&3)+8*(reg>>2)+4*hi
#pragma unroll
  for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[mt][r] = 0.f;

  char* vt = smem + wave * Smem<D>::VT_BYTES;  // this wave's V^T tile

  // every wave runs the same number of rounds so the barriers stay uniform
  const int n_rounds = (n_tiles + NW - 1) / NW;
  for (int rd = 0; rd < n_rounds; ++rd) {
    const int t = rd * NW + wave;
    const bool active = t < n_tiles;
    const int kvbase = t * KT;

    // ---- stage V^T: lane = kv row, 8 d per pass -------------------------
    if (active) {
      const int grow = kvbase + lane;
      const bool inb = grow < kv_end;
      const short* vrow = vp + (long long)(inb ? grow : kv_end - 1) * kvrs;
#pragma unroll
      for (int c = 0; c < D / 8; ++c) {
        bf16x8_t x = *reinterpret_cast<const bf16x8_t*>(vrow + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          *reinterpret_cast<short*>(vt + vtswz(c * 8 + j, lane * 2)) =
              inb ? x[j] : (short)0;
      }
    }
    __syncthreads();

    if (active) {
      // ---- S^T = K Q^T: rows kv = kvbase+32mt+(r&3)+8*(r>>2)+4hi --------
      f32x16_t st[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        f32x16_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const int grow = kvbase + 32 * mt + l31;
        const short* krow =
            kp + (long long)(grow < kv_end ? grow : kv_end - 1) * kvrs +
            hi * 8;
#pragma unroll
        for (int ks = 0; ks < NQF; ++ks) {
          bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(krow + 16 * ks);
          acc = RP_MFMA(kf, qfrag[ks], acc, 0, 0, 0);
        }
        st[mt] = acc;
      }

      // ---- online softmax, lane-local q row; masked by select -----------
      float tmax = -INFINITY;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int gkv = kvbase + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hi;
          const float sv = gkv <= my_p ? st[mt][r] * sc2 : -INFINITY;
          st[mt][r] = sv;
          tmax = fmaxf(tmax, sv);
        }
      tmax = fmaxf(tmax, half_swap(tmax, hi));
      const float m_new = fmaxf(m_run, tmax);
      if (m_new > m_run) {
        const float c = (m_run == -INFINITY)
                            ? 0.f
                            : __builtin_amdgcn_exp2f(m_run - m_new);
        l_run *= c;
#pragma unroll
        for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) ot[mt][r] *= c;
        m_run = m_new;
      }
      const float m_sub = (m_run == -INFINITY) ? 0.f : m_run;
      float psum = 0.f;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float sv = st[mt][r];
          const float p =
              sv == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sv - m_sub);
          st[mt][r] = p;
          psum += p;
        }
      psum += half_swap(psum, hi);
      l_run += psum;

      // ---- P fragments in-register (see attention.hip) ------------------
      bf16x8_t pfrag[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int mt = ks >> 1, s = ks & 1;
        unsigned int wA0 = cvtpk2(st[mt][8 * s + 0], st[mt][8 * s + 1]);
        unsigned int wA1 = cvtpk2(st[mt][8 * s + 2], st[mt][8 * s + 3]);
        unsigned int wB0 = cvtpk2(st[mt][8 * s + 4], st[mt][8 * s + 5]);
        unsigned int wB1 = cvtpk2(st[mt][8 * s + 6], st[mt][8 * s + 7]);
        auto r0 = __builtin_amdgcn_permlane32_swap((int)wA0, (int)wB0, false,
                                                   false);
        auto r1 = __builtin_amdgcn_permlane32_swap((int)wA1, (int)wB1, false,
                                                   false);
        unsigned int w[4] = {(unsigned int)r0[0], (unsigned int)r1[0],
                             (unsigned int)r0[1], (unsigned int)r1[1]};
        pfrag[ks] = *reinterpret_cast<bf16x8_t*>(w);
      }

      // ---- O^T += V^T P^T ----------------------------------------------
#pragma unroll
      for (int mt = 0; mt < NOT; ++mt) {
        const int drow = 32 * mt + l31;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(
              vt + vtswz(drow, (16 * ks + hi * 8) * 2));
          ot[mt] = RP_MFMA(vf, pfrag[ks], ot[mt], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // V^T tile is overwritten next round / by the merge
  }

  // ---- merge the 4 waves' (m, l, O) in LDS (reuses the V^T space) --------
  float* lacc = reinterpret_cast<float*>(smem);            // [NW][32][D+4]
  float* lml = reinterpret_cast<float*>(smem + Smem<D>::ACC_BYTES);
  {
    float* row = lacc + ((long long)wave * QT + l31) * (D + OPAD);
#pragma unroll
    for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = 32 * mt + 8 * g + 4 * hi;
#pragma unroll
        for (int i = 0; i < 4; ++i) row[d0 + i] = ot[mt][4 * g + i];
      }
    if (hi == 0) {
      lml[(wave * QT + l31) * 2 + 0] = m_run;
      lml[(wave * QT + l31) * 2 + 1] = l_run;
    }
  }
  __syncthreads();

  constexpr int DPT = D / 8;  // output dims per thread: 8 threads per token
  const int tq = threadIdx.x >> 3;
  const int d0 = (threadIdx.x & 7) * DPT;
  if (j0 + tq < q_len) {
    float mstar = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w)
      mstar = fmaxf(mstar, lml[(w * QT + tq) * 2]);
    float lsum = 0.f;
    float o[DPT];
#pragma unroll
    for (int i = 0; i < DPT; ++i) o[i] = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float mi = lml[(w * QT + tq) * 2];
      if (mi == -INFINITY) continue;  // wave saw no visible column
      const float c = __builtin_amdgcn_exp2f(mi - mstar);
      lsum += lml[(w * QT + tq) * 2 + 1] * c;
      const float* src = lacc + ((long long)w * QT + tq) * (D + OPAD) + d0;
#pragma unroll
      for (int i = 0; i < DPT; ++i) o[i] += src[i] * c;
    }
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    short* dst = out + (q_start + j0 + tq) * qrs + h * D + d0;
#pragma unroll
    for (int i = 0; i < DPT; i += 2)
      *reinterpret_cast<unsigned int*>(dst + i) =
          cvtpk2(o[i] * inv, o[i + 1] * inv);
  }
}

}  // namespace rprefill

at::Tensor ragged_prefill(at::Tensor q, at::Tensor kpool, at::Tensor vpool,
                          at::Tensor desc, long max_qlen, long max_kvlen) {
  CHECK_ARG(q, at::kBFloat16);
  CHECK_ARG(kpool, at::kBFloat16);
  CHECK_ARG(vpool, at::kBFloat16);
  CHECK_ARG(desc, at::kLong);
  CHECK_ON(kpool, q);
  CHECK_ON(vpool, q);
  CHECK_ON(desc, q);
  TORCH_CHECK(q.dim() == 3, "ragged_prefill: q must be [T,Hq,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(),
              "ragged_prefill: kpool and vpool must both be [B,Smax,Hk,D]");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 4,
              "ragged_prefill: desc must be [n,4] "
              "(slot, q_start, q_len, kv_len)");
  const long T = q.size(0), Hq = q.size(1), D = q.size(2);
  const long B = kpool.size(0), Smax = kpool.size(1), Hk = kpool.size(2);
  const long n = desc.size(0);
  TORCH_CHECK(n >= 1 && T >= 1, "ragged_prefill: empty batch");
  TORCH_CHECK(B >= 1 && Hk >= 1 && kpool.size(3) == D,
              "ragged_prefill: empty pool or pool head_dim != q head_dim");
  TORCH_CHECK(D == 128 || D == 64,
              "ragged_prefill: head_dim must be 64 or 128");
  TORCH_CHECK(Hq >= 1 && Hq % Hk == 0, "ragged_prefill: Hq % Hk != 0");
  const long G = Hq / Hk;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8,
              "ragged_prefill: unsupported GQA group ", G);
  TORCH_CHECK(1 <= max_qlen && max_qlen <= max_kvlen && max_kvlen <= Smax,
              "ragged_prefill: need 1 <= max_qlen <= max_kvlen <= Smax, got ",
              max_qlen, ", ", max_kvlen, ", ", Smax);
  TORCH_CHECK(n <= 65535 && Hq <= 65535,
              "ragged_prefill: more than 65535 sequences or heads");

  auto out = at::empty_like(q);
  const float scale = 1.0f / std::sqrt((float)D);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((unsigned)((max_qlen + rprefill::QT - 1) / rprefill::QT),
            (unsigned)n, (unsigned)Hq);

#define LAUNCH(DD)                                                          \
  hipLaunchKernelGGL((rprefill::ragged_prefill_kernel<DD>), grid,           \
                     dim3(256), 0, stream.stream(),                         \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const short*>(kpool.data_ptr()),      \
                     reinterpret_cast<const short*>(vpool.data_ptr()),      \
                     desc.data_ptr<int64_t>(),                              \
                     reinterpret_cast<short*>(out.data_ptr()), (int)T,      \
                     (int)Hq, (int)Hk, (int)B, (int)Smax, (int)max_kvlen,   \
                     scale)
  if (D == 128)
    LAUNCH(128);
  else
    LAUNCH(64);
#undef LAUNCH
  HIP_CHECK_KERNEL();
  return out;
}
