// MFMA split-KV decode attention over the KV slot pool for MI355X (gfx950):
// any GQA group up to 32 and an optional sliding window.
//
// Role parity: reference inference/v2 blocked flash decode
// (deepspeed/inference/v2/kernels/ragged_ops/). ragged_decode.hip is templated
// on the group G = Hq/Hk and spends a 6-step butterfly per (key, q head); here
// the G query heads that share a kv head are the COLUMNS of one 32x32x16 MFMA,
// so one build serves G = 1..32 and a K row is multiplied with all of them at
// once.
//
// Row i attends pool positions [lo_i, len_i) of slot rows[i], len_i clamped
// into [0, Smax], lo_i = max(0, len_i - window) under a window, else 0.
//
// Work split: grid (n, Hk, NS), one workgroup of 4 waves per (row, kv head,
// split). Split s covers [lo + s*per, lo + (s+1)*per) cut at len, per =
// ceil((len - lo) / NS) rounded up to whole 32-key tiles: every workgroup
// derives its range from its own row's length, so the host needs no length
// (max_len only sizes NS). A split past the row's end writes the empty
// partial (m = -inf, l = 0). Wave w takes the split's tiles w, w+4, ...
//
// Per tile (layouts as documented at the top of attention.hip):
//   S^T = K Q^T   A = K tile (32 keys as rows), B = Q^T with column c < G the
//                 query head hk*G + c (registers, loaded once), columns >= G
//                 zero. C column = lane&31 = head: the online softmax of a head
//                 is lane-local plus one permlane32_swap.
//   P             built in registers (cvt_pk + permlane32_swap), as in
//                 ragged_prefill.hip.
//   O^T += V^T P^T  V^T fragments by ds_read_b64_tr_b16 (lds_tr_read.h) from a
//                 ROW-MAJOR V image; nothing is transposed by hand.
//
// Data movement: decode is HBM-bound, so each K and V byte of a split is
// fetched once per workgroup, by full-row coalesced loads (consecutive lanes
// take consecutive 16 bytes of a pool row, 64 lanes = 4 rows at D 128), held
// in registers, and stored into the wave's own K and V image [32][D] (the
// swizzles of flash_fwd_layout.h). Tile t+4's loads are issued right after
// tile t's registers went to LDS and fly under tile t's MFMAs. The images are
// private to a wave and a wave's LDS operations complete in order, so the tile
// loop has no barrier.
//
// LDS per workgroup: 4 waves x 2 images x 32 x 2D bytes = 64 KiB at D 128,
// 32 KiB at D 64; the merge of the 4 waves' (m, l, O) reuses it (3 waves x
// (16 D/32 + 2) x 256 bytes = 49.5 KiB / 25.5 KiB, lane for lane: wave 0's
// lane reads what the same lane of waves 1..3 stored, so no layout is
// involved). Resident workgroups per CU: 2 at D 128 (160 KiB LDS; the kernel is
// held to 256 registers for it), 3 at D 64 (148 registers; LDS would allow 5).
// Each resident wave has a whole tile of K and V in flight: 32 KiB per CU at
// D 128, 24 KiB at D 64.
//
// Masking is by SELECT: a key outside [start, end) scores -inf and its P is
// exactly 0. K rows past the split's end are clamped onto its last row, V rows
// past it are staged as zeros: nothing outside [lo, len) is loaded, so NaN or
// another request's data cannot reach a live value through 0 * NaN.
//
// NS > 1: fp32 partials [n,Hq,NS,D] (unnormalised O) and [n,Hq,NS,2] (m in the
// exp2 domain, l), merged by the combine kernel below. NS == 1: the kernel
// normalises and writes bf16 itself.
#include <torch/extension.h>

#include <algorithm>

#include "common.h"
#include "flash_fwd_layout.h"
#include "lds_tr_read.h"

namespace rdgqa {

using bf16x8_t = __attribute__((ext_vector_type(8))) short;
using f32x16_t = __attribute__((ext_vector_type(16))) float;
using f32x4_t = __attribute__((ext_vector_type(4))) float;
#define RG_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16

constexpr int KT = 32;    // keys per tile
constexpr int NW = 4;     // waves per workgroup
constexpr int MAXG = 32;  // q heads per kv head: the MFMA's columns
constexpr int MAX_SPLITS = 128;

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
  static constexpr int RB = D * 2;                  // bytes per image row
  static constexpr int IMG = KT * RB;               // one image
  static constexpr int NREG = (D / 32) * 16 + 2;    // O^T regs + m + l
  static constexpr int MERGE = (NW - 1) * NREG * 64 * 4;
  static constexpr int BYTES = NW * 2 * IMG > MERGE ? NW * 2 * IMG : MERGE;
};

// the wave's share of one image: NL 16-byte pieces per lane, piece j of lane
// `lane` is bytes cb .. cb+15 of tile row `row`
template <int D>
struct Piece {
  static constexpr int PPR = D * 2 / 16;  // pieces per row
  static constexpr int NL = KT * PPR / 64;
  DEV_INLINE static int row(int j, int lane) { return (j * 64 + lane) / PPR; }
  DEV_INLINE static int cb(int j, int lane) {
    return ((j * 64 + lane) % PPR) * 16;
  }
};

// keys kb .. kb+31 of one (slot, kv head) into registers. A row at or past
// `end` repeats row end-1 (end > kb >= 0: always a row of the range).
template <int D>
DEV_INLINE void load_tile(bf16x8_t (&kr)[Piece<D>::NL],
                          bf16x8_t (&vr)[Piece<D>::NL], const short* kp,
                          const short* vp, long long kvrs, int kb, int end,
                          int lane) {
#pragma unroll
  for (int j = 0; j < Piece<D>::NL; ++j) {
    const int key = min(kb + Piece<D>::row(j, lane), end - 1);
    const long long off = (long long)key * kvrs + Piece<D>::cb(j, lane) / 2;
    kr[j] = *reinterpret_cast<const bf16x8_t*>(kp + off);
    vr[j] = *reinterpret_cast<const bf16x8_t*>(vp + off);
  }
}

// the 2 k-slices x 2 halves of V's operand for one d-tile (4 reads)
template <int D>
DEV_INLINE void issue_v_dtile(tr_frag (&f)[2], unsigned base) {
  using namespace fwd_layout;
  f[0] = issue_tr_read_off<v_tr_step<D>(0, 0), v_tr_step<D>(0, 1)>(base);
  f[1] = issue_tr_read_off<v_tr_step<D>(1, 0), v_tr_step<D>(1, 1)>(base);
}

// q [n,Hq,D] bf16, kpool/vpool [B,Smax,Hk,D] bf16, rows/lens [n] i64.
// NS > 1: partial_out [n,Hq,NS,D] f32, partial_ml [n,Hq,NS,2] f32.
// NS == 1: out [n,Hq,D] bf16.
template <int D>
__launch_bounds__(256, 2)
__global__ void ragged_decode_gqa_kernel(
    const short* __restrict__ q, const short* __restrict__ kpool,
    const short* __restrict__ vpool, const int64_t* __restrict__ rows,
    const int64_t* __restrict__ lens, float* __restrict__ partial_out,
    float* __restrict__ partial_ml, short* __restrict__ out, int Hq, int Hk,
    int G, int B, int Smax, int NS, int window, float scale) {
  __shared__ __attribute__((aligned(16))) char smem[Smem<D>::BYTES];

  constexpr int NQF = D / 16;  // Q k-slices
  constexpr int NOT = D / 32;  // O^T d m-tiles
  constexpr int NL = Piece<D>::NL;
  using namespace fwd_layout;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  const int i = blockIdx.x;   // active-row index
  const int hk = blockIdx.y;  // kv head
  const int s = blockIdx.z;   // split

  const long long slot = rows[i];
  const long long len64 = lens[i];
  // a slot outside the pool is served as an empty row
  const int len = (slot < 0 || slot >= B)
                      ? 0
                      : (int)min(max(len64, (long long)0), (long long)Smax);
  const int lo = window > 0 ? max(0, len - window) : 0;
  const int per = ((len - lo + NS - 1) / NS + KT - 1) / KT * KT;
  const int start = lo + s * per;
  const int end = min(len, start + per);
  const long long head0 = (long long)i * Hq + hk * G;  // first q head

  if (start >= end) {  // empty row, or a split past the row's end
    if (NS == 1) {
      for (int e = threadIdx.x; e < G * D; e += 256) out[head0 * D + e] = 0;
    } else if (threadIdx.x < 2 * G) {
      partial_ml[((head0 + (threadIdx.x >> 1)) * NS + s) * 2 +
                 (threadIdx.x & 1)] = (threadIdx.x & 1) ? 0.f : -INFINITY;
    }
    return;
  }
  const int n_tiles = (end - start + KT - 1) / KT;

  const long long kvrs = (long long)Hk * D;
  const short* kp = kpool + (slot * Smax) * kvrs + hk * D;
  const short* vp = vpool + (slot * Smax) * kvrs + hk * D;

  // ---- Q^T: qfrag[ks] = Q[head hk*G + l31][16*ks + hi*8 .. +7], 0 past G --
  bf16x8_t qfrag[NQF];
#pragma unroll
  for (int ks = 0; ks < NQF; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) qfrag[ks][j] = 0;
  if (l31 < G) {
    const short* src = q + (head0 + l31) * D + hi * 8;
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

  // this wave's images and its lane's read addresses
  char* kimg = smem + wave * 2 * Smem<D>::IMG;
  char* vimg = kimg + Smem<D>::IMG;
  unsigned vbase[NOT];
#pragma unroll
  for (int mt = 0; mt < NOT; ++mt)
    vbase[mt] = lds_addr(vimg + v_tr_lane_base<D>(lane, mt));

  bf16x8_t kr[NL], vr[NL];
  if (wave < n_tiles)
    load_tile<D>(kr, vr, kp, vp, kvrs, start + wave * KT, end, lane);

  for (int t = wave; t < n_tiles; t += NW) {  // wave-uniform: EXEC stays full
    const int kb = start + t * KT;

    // ---- registers -> images; V rows past the end become zeros ------------
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int row = Piece<D>::row(j, lane), cb = Piece<D>::cb(j, lane);
      bf16x8_t vz = vr[j];
      if (kb + row >= end) {
#pragma unroll
        for (int e = 0; e < 8; ++e) vz[e] = 0;
      }
      *reinterpret_cast<bf16x8_t*>(kimg + k_off<D>(row, cb)) = kr[j];
      *reinterpret_cast<bf16x8_t*>(vimg + v_off<D>(row, cb)) = vz;
    }
    // the wave's next tile flies under this one's compute
    if (t + NW < n_tiles)
      load_tile<D>(kr, vr, kp, vp, kvrs, kb + NW * KT, end, lane);

    // ---- S^T = K Q^T: rows key = kb + (r&3)+8*(r>>2)+4*hi, col = head ------
    f32x16_t st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NQF; ++ks) {
      bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(
          kimg + k_row_read_addr<D>(lane, 0, ks));
      st = RG_MFMA(kf, qfrag[ks], st, 0, 0, 0);
    }

    // V's operand for d-tile 0: the transposed reads fly under the softmax
    tr_frag vf[2][2];
    issue_v_dtile<D>(vf[0], vbase[0]);

    // ---- online softmax, lane-local head; masked by select -----------------
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kb + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const float sv = key < end ? st[r] * sc2 : -INFINITY;
      st[r] = sv;
      tmax = fmaxf(tmax, sv);
    }
    tmax = fmaxf(tmax, half_swap(tmax, hi));
    const float m_new = fmaxf(m_run, tmax);
    if (m_new > m_run) {
      const float c =
          (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
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
    for (int r = 0; r < 16; ++r) {
      const float sv = st[r];
      const float p =
          sv == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sv - m_sub);
      st[r] = p;
      psum += p;
    }
    psum += half_swap(psum, hi);
    l_run += psum;

    // ---- P fragments in-register (see attention.hip) -----------------------
    bf16x8_t pfrag[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      unsigned int wA0 = cvtpk2(st[8 * ks + 0], st[8 * ks + 1]);
      unsigned int wA1 = cvtpk2(st[8 * ks + 2], st[8 * ks + 3]);
      unsigned int wB0 = cvtpk2(st[8 * ks + 4], st[8 * ks + 5]);
      unsigned int wB1 = cvtpk2(st[8 * ks + 6], st[8 * ks + 7]);
      auto r0 =
          __builtin_amdgcn_permlane32_swap((int)wA0, (int)wB0, false, false);
      auto r1 =
          __builtin_amdgcn_permlane32_swap((int)wA1, (int)wB1, false, false);
      unsigned int w[4] = {(unsigned int)r0[0], (unsigned int)r1[0],
                           (unsigned int)r0[1], (unsigned int)r1[1]};
      pfrag[ks] = *reinterpret_cast<bf16x8_t*>(w);
    }

    // ---- O^T += V^T P^T ---------------------------------------------------
    // one d-tile (4 reads) ahead of the MFMAs that use them
#pragma unroll
    for (int mt = 0; mt < NOT; ++mt) {
      if (mt + 1 < NOT) {
        issue_v_dtile<D>(vf[(mt + 1) & 1], vbase[mt + 1]);
        tr_wait<4>(vf[mt & 1][0], vf[mt & 1][1]);
      } else {
        tr_wait<0>(vf[mt & 1][0], vf[mt & 1][1]);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        ot[mt] = RG_MFMA(tr_operand(vf[mt & 1][ks]), pfrag[ks], ot[mt], 0, 0,
                         0);
    }
  }

  // ---- merge the 4 waves' (m, l, O), lane for lane, over the images --------
  float* mg = reinterpret_cast<float*>(smem);  // [NW-1][NREG][64]
  constexpr int NREG = Smem<D>::NREG;
  __syncthreads();  // every wave is done with its images
  if (wave > 0) {
    float* dst = mg + (wave - 1) * NREG * 64 + lane;
#pragma unroll
    for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(mt * 16 + r) * 64] = ot[mt][r];
    dst[(NREG - 2) * 64] = m_run;
    dst[(NREG - 1) * 64] = l_run;
  }
  __syncthreads();
  if (wave > 0) return;

#pragma unroll 1
  for (int w = 1; w < NW; ++w) {
    const float* src = mg + (w - 1) * NREG * 64 + lane;
    const float mw = src[(NREG - 2) * 64];
    if (mw == -INFINITY) continue;  // that wave saw no key
    const float m_new = fmaxf(m_run, mw);
    const float c0 =
        (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
    const float c1 = __builtin_amdgcn_exp2f(mw - m_new);
    l_run = l_run * c0 + src[(NREG - 1) * 64] * c1;
#pragma unroll
    for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ot[mt][r] = ot[mt][r] * c0 + src[(mt * 16 + r) * 64] * c1;
    m_run = m_new;
  }

  if (l31 >= G) return;  // columns past the group hold no head
  const long long head = head0 + l31;
  if (NS == 1) {
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    short* dst = out + head * D;
#pragma unroll
    for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        unsigned int w[2];
        w[0] = cvtpk2(ot[mt][4 * g + 0] * inv, ot[mt][4 * g + 1] * inv);
        w[1] = cvtpk2(ot[mt][4 * g + 2] * inv, ot[mt][4 * g + 3] * inv);
        *reinterpret_cast<unsigned long long*>(dst + 32 * mt + 8 * g +
                                               4 * hi) =
            *reinterpret_cast<unsigned long long*>(w);
      }
  } else {
    float* dst = partial_out + (head * NS + s) * D;
#pragma unroll
    for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4_t x = {ot[mt][4 * g + 0], ot[mt][4 * g + 1], ot[mt][4 * g + 2],
                     ot[mt][4 * g + 3]};
        *reinterpret_cast<f32x4_t*>(dst + 32 * mt + 8 * g + 4 * hi) = x;
      }
    if (hi == 0) {
      partial_ml[(head * NS + s) * 2] = m_run;
      partial_ml[(head * NS + s) * 2 + 1] = l_run;
    }
  }
}

// merge the NS split partials -> out [n,Hq,D] bf16; one wave per (row, head)
template <int D>
__global__ void ragged_decode_gqa_combine_kernel(
    const float* __restrict__ partial_out,
    const float* __restrict__ partial_ml, short* __restrict__ out,
    long long nhq, int NS) {
  constexpr int DL = D / 64;
  const int lane = threadIdx.x & 63;
  const long long rh = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rh >= nhq) return;
  float mstar = -INFINITY;
  for (int c = 0; c < NS; ++c)
    mstar = fmaxf(mstar, partial_ml[(rh * NS + c) * 2]);
  float lsum = 0.f;
  float o[DL];
#pragma unroll
  for (int j = 0; j < DL; ++j) o[j] = 0.f;
  for (int c = 0; c < NS; ++c) {
    const float mi = partial_ml[(rh * NS + c) * 2];
    if (mi == -INFINITY) continue;  // empty split: its O was never written
    const float sc = __builtin_amdgcn_exp2f(mi - mstar);
    lsum += partial_ml[(rh * NS + c) * 2 + 1] * sc;
    const float* po = partial_out + (rh * NS + c) * D + lane * DL;
#pragma unroll
    for (int j = 0; j < DL; ++j) o[j] += po[j] * sc;
  }
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
#pragma unroll
  for (int j = 0; j < DL; ++j)
    out[rh * D + lane * DL + j] = f2bf(o[j] * inv);
}

static int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      cus <= 0)
    cus = 256;
  return cus;
}

}  // namespace rdgqa

at::Tensor ragged_decode_gqa(at::Tensor q, at::Tensor kpool, at::Tensor vpool,
                             at::Tensor rows, at::Tensor lens, long window,
                             long max_len, long splits) {
  CHECK_ARG(q, at::kBFloat16);
  CHECK_ARG(kpool, at::kBFloat16);
  CHECK_ARG(vpool, at::kBFloat16);
  CHECK_ARG(rows, at::kLong);
  CHECK_ARG(lens, at::kLong);
  CHECK_ON(kpool, q);
  CHECK_ON(vpool, q);
  CHECK_ON(rows, q);
  CHECK_ON(lens, q);
  TORCH_CHECK((q.dim() == 4 && q.size(1) == 1) || q.dim() == 3,
              "ragged_decode_gqa: q must be [n,1,Hq,D] or [n,Hq,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(),
              "ragged_decode_gqa: kpool and vpool must both be "
              "[B,Smax,Hk,D]");
  const long n = q.size(0), Hq = q.size(-2), D = q.size(-1);
  const long B = kpool.size(0), Smax = kpool.size(1), Hk = kpool.size(2);
  TORCH_CHECK(n >= 1 && B >= 1 && Smax >= 1 && Hk >= 1 && kpool.size(3) == D,
              "ragged_decode_gqa: empty batch or pool, or pool head_dim != "
              "q head_dim");
  TORCH_CHECK(rows.numel() == n && lens.numel() == n,
              "ragged_decode_gqa: rows and lens must have one entry per q "
              "row");
  TORCH_CHECK(D == 128 || D == 64,
              "ragged_decode_gqa: head_dim must be 64 or 128");
  TORCH_CHECK(Hq >= 1 && Hq % Hk == 0, "ragged_decode_gqa: Hq % Hk != 0");
  const long G = Hq / Hk;
  TORCH_CHECK(G <= rdgqa::MAXG, "ragged_decode_gqa: GQA group ", G,
              " exceeds ", rdgqa::MAXG);
  TORCH_CHECK(window >= 0, "ragged_decode_gqa: window must be >= 0, got ",
              window);
  TORCH_CHECK(0 <= max_len && max_len <= Smax,
              "ragged_decode_gqa: need 0 <= max_len <= Smax, got ", max_len,
              ", ", Smax);
  TORCH_CHECK(0 <= splits && splits <= rdgqa::MAX_SPLITS,
              "ragged_decode_gqa: need 0 <= splits <= ", rdgqa::MAX_SPLITS);
  TORCH_CHECK(Hk <= 65535, "ragged_decode_gqa: more than 65535 kv heads");

  if (max_len == 0) {  // the one host read; callers that know a bound skip it
    max_len = lens.max().item<long>();
    TORCH_CHECK(max_len <= Smax, "ragged_decode_gqa: lens.max() = ", max_len,
                " exceeds the pool's Smax = ", Smax);
    max_len = std::max<long>(max_len, 1);
  }
  // about two workgroups per CU, no split shorter than one tile per wave
  long NS = splits;
  if (NS == 0) {
    const long span = window > 0 ? std::min(max_len, window) : max_len;
    const long longest = std::max<long>(span / (rdgqa::KT * rdgqa::NW), 1);
    const long want = (2 * rdgqa::device_cus() + n * Hk - 1) / (n * Hk);
    NS = std::min<long>(std::min(want, longest), rdgqa::MAX_SPLITS);
  }

  auto opts = q.options().dtype(at::kFloat);
  auto out = at::empty({n, 1, Hq, D}, q.options());
  at::Tensor pout, pml;
  if (NS > 1) {
    pout = at::empty({n, Hq, NS, D}, opts);
    pml = at::empty({n, Hq, NS, 2}, opts);
  }
  const float scale = 1.0f / std::sqrt((float)D);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((unsigned)n, (unsigned)Hk, (unsigned)NS);

#define LAUNCH(DD)                                                          \
  hipLaunchKernelGGL((rdgqa::ragged_decode_gqa_kernel<DD>), grid,           \
                     dim3(256), 0, stream.stream(),                         \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const short*>(kpool.data_ptr()),      \
                     reinterpret_cast<const short*>(vpool.data_ptr()),      \
                     rows.data_ptr<int64_t>(), lens.data_ptr<int64_t>(),    \
                     NS > 1 ? pout.data_ptr<float>() : nullptr,             \
                     NS > 1 ? pml.data_ptr<float>() : nullptr,              \
                     reinterpret_cast<short*>(out.data_ptr()), (int)Hq,     \
                     (int)Hk, (int)G, (int)B, (int)Smax, (int)NS,           \
                     (int)std::min<long>(window, Smax), scale)
  if (D == 128)
    LAUNCH(128);
  else
    LAUNCH(64);
#undef LAUNCH
  HIP_CHECK_KERNEL();
  if (NS == 1) return out;

  const long long nhq = (long long)n * Hq;
  dim3 gridc((unsigned)((nhq + 3) / 4));
#define COMBINE(DD)                                                         \
  hipLaunchKernelGGL(rdgqa::ragged_decode_gqa_combine_kernel<DD>, gridc,    \
                     dim3(256), 0, stream.stream(), pout.data_ptr<float>(), \
                     pml.data_ptr<float>(),                                 \
                     reinterpret_cast<short*>(out.data_ptr()), nhq, (int)NS)
  if (D == 128)
    COMBINE(128);
  else
    COMBINE(64);
#undef COMBINE
  HIP_CHECK_KERNEL();
  return out;
}
