// The tile engine of the four MFMA ragged GQA kernels for MI355X (gfx950):
//   ragged_decode_gqa.hip       split-KV decode over the bf16 slot pool
//   ragged_decode_gqa_fp8.hip   the same over the fp8 pool (kv_fp8.h)
//   ragged_prefill_gqa.hip      the fused serving step over the bf16 pool
//   ragged_prefill_gqa_fp8.hip  the same over the fp8 pool
// Each unit keeps what is its own: which 32 columns a workgroup serves, which
// keys a column may see, how a tile gets from HBM into LDS, and where the
// result goes. Everything a tile goes through after that is here, once.
//
// A workgroup is 4 waves. Its 32 COLUMNS are the columns of one 32x32x16 bf16
// MFMA: the G query heads of one decode row, or 32 (token, head) pairs of a
// sequence; lane & 31 is the lane's column. Its keys run over [start, end) in
// tiles of KT = 32; wave w takes tiles w, w+4, ... and keeps its own K and V
// image [32][D] bf16 in LDS, row-major with the swizzles of flash_fwd_layout.h.
// The images are private to a wave and a wave's LDS operations complete in
// order, so the tile loop has no barrier.
//
// Per tile (register layouts as documented at the top of attention.hip):
//   S^T = K Q^T      A = the K image (32 keys as rows), B = Q^T held in
//                    registers (load_q; columns that hold nothing are zero).
//                    C row = key kb + (r&3) + 8*(r>>2) + 4*hi, C column = the
//                    lane's column: the online softmax of a column is
//                    lane-local plus one permlane32_swap (softmax_step).
//   P                built in registers, 4 cvt_pk + 2 permlane32_swap per
//                    k-slice (build_p).
//   O^T += V^T P^T   V^T fragments by ds_read_b64_tr_b16 (lds_tr_read.h) from
//                    the ROW-MAJOR V image, one d-tile ahead of the MFMAs that
//                    use them (pv_accumulate); nothing is transposed by hand.
// Over the fp8 pool every e4m3 code is exactly a bf16, so the MFMAs are these
// same ones run on the CODES; the scales enter in softmax_step (TileScales):
// score = S^T * k_scale[key] * softmax_scale, the row sum is of the unscaled
// p, and P = bf16(p * v_scale[key]).
//
// Masking is by SELECT: a key the column may not see scores -inf and its P is
// exactly 0, never a product with a score or a scale. The units load nothing
// outside [start, end): K rows (and scales) past the end come from row end-1,
// the staged V rows (and scales) past it are zeros. So NaN or another
// request's data cannot reach a live value through 0 * NaN. A lane may see no
// key in a whole tile or in a wave's whole share: the m == -inf guards cover
// it, in softmax_step and in merge_waves.
//
// Merge: the 4 waves' (m, l, O) meet in the image space, [NW-1][NREG][64]
// floats, lane for lane: wave 0's lane reads what the same lane of waves 1..3
// stored, so no layout is involved (3 x (16 D/32 + 2) x 256 bytes = 49.5 KiB
// at D 128, 25.5 KiB at D 64, inside the images' 64 / 32 KiB).
//
// Decode splits a row's keys over NS workgroups (plan_splits). NS > 1: fp32
// partials [n,Hq,NS,D] (unnormalised O) and [n,Hq,NS,2] (m in the exp2
// domain, l; store_partial), merged by combine_kernel. NS == 1, and prefill:
// the kernel normalises and writes bf16 itself (store_row).
//
// A header, so that each unit keeps its build flags (no packed fp32,
// ops/build.py) and its own tuned staging loop.
#pragma once

#include <torch/extension.h>

#include <algorithm>

#include "common.h"
#include "flash_fwd_layout.h"
#include "lds_tr_read.h"

namespace rgqa {

using bf16x8_t = __attribute__((ext_vector_type(8))) short;
using f32x16_t = __attribute__((ext_vector_type(16))) float;
using f32x4_t = __attribute__((ext_vector_type(4))) float;
using u32x4_t = __attribute__((ext_vector_type(4))) unsigned int;
#define RGQA_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16

constexpr int CT = 32;    // columns per workgroup: the MFMA's columns
constexpr int KT = 32;    // keys per tile
constexpr int NW = 4;     // waves per workgroup
constexpr int MAXG = 32;  // q heads per kv head
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

// LDS of a workgroup; SCALES adds a wave's staged k_scale[32], v_scale[32]
template <int D, bool SCALES = false>
struct Smem {
  static constexpr int RB = D * 2;                  // bytes per image row
  static constexpr int IMG = KT * RB;               // one image
  static constexpr int NREG = (D / 32) * 16 + 2;    // O^T regs + m + l
  static constexpr int MERGE = (NW - 1) * NREG * 64 * 4;
  static constexpr int MAIN = NW * 2 * IMG > MERGE ? NW * 2 * IMG : MERGE;
  static constexpr int SC = SCALES ? 2 * KT * 4 : 0;
  static constexpr int BYTES = MAIN + NW * SC;
};

// the wave's share of one tile of a pool with EB bytes per element: NL
// 16-byte pieces per lane, piece j of lane `lane` is pool bytes cb .. cb+15 of
// tile row `row`
template <int D, int EB>
struct Piece {
  static constexpr int PPR = D * EB / 16;  // pieces per row
  static constexpr int NL = KT * PPR / 64;
  static constexpr int RJ = 64 / PPR;  // piece j is RJ rows below piece j-1
  DEV_INLINE static int row(int j, int lane) { return (j * 64 + lane) / PPR; }
  DEV_INLINE static int cb(int j, int lane) {
    return ((j * 64 + lane) % PPR) * 16;
  }
};

// the 2 k-slices x 2 halves of V's operand for one d-tile (4 reads)
template <int D>
DEV_INLINE void issue_v_dtile(tr_frag (&f)[2], unsigned base) {
  using namespace fwd_layout;
  f[0] = issue_tr_read_off<v_tr_step<D>(0, 0), v_tr_step<D>(0, 1)>(base);
  f[1] = issue_tr_read_off<v_tr_step<D>(1, 0), v_tr_step<D>(1, 1)>(base);
}

// Q^T: qfrag[ks] = the column's q row [16*ks + hi*8 .. +7]; 0 in a column
// that holds nothing. row() is the row's address, formed for a valid column
// only (computed ahead of the branch it costs the decode kernels 2 to 3
// registers).
template <int NQF, class Row>
DEV_INLINE void load_q(bf16x8_t (&qfrag)[NQF], bool valid, int hi, Row row) {
#pragma unroll
  for (int ks = 0; ks < NQF; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) qfrag[ks][j] = 0;
  if (valid) {
    const short* src = row() + hi * 8;
#pragma unroll
    for (int ks = 0; ks < NQF; ++ks)
      qfrag[ks] = *reinterpret_cast<const bf16x8_t*>(src + 16 * ks);
  }
}

// the scales of softmax_step over the bf16 pool: none
struct NoScales {
  DEV_INLINE float k(int, float s) const { return s; }
  DEV_INLINE void load_v() {}
  DEV_INLINE float v(int, float p) const { return p; }
};

// the scales of softmax_step over the fp8 pool, from the wave's staged k[32],
// v[32] of the tile: the 16 of this lane's score rows, key = kb + (r&3) +
// 8*(r>>2) + 4*hi, as four float4 (the 32 lanes of a half read one address: a
// broadcast). The v scales are loaded once the k scales are dead.
struct TileScales {
  const float* scl;
  int hi;
  f32x4_t sc[4];
  DEV_INLINE void load(int first) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      sc[g] = *reinterpret_cast<const f32x4_t*>(scl + first + 8 * g + 4 * hi);
  }
  DEV_INLINE void load_k() { load(0); }
  DEV_INLINE void load_v() { load(KT); }
  DEV_INLINE float k(int r, float s) const { return s * sc[r >> 2][r & 3]; }
  DEV_INLINE float v(int r, float p) const { return p * sc[r >> 2][r & 3]; }
};

// One tile's online softmax of the lane's column. In: st = the 16 raw scores.
// Out: st = P (times v_scale over the fp8 pool); m_run, l_run, ot rescaled and
// updated. visible(r) is the unit's mask for score register r; sc2 is the
// softmax scale in the exp2 domain.
template <int NOT, class Visible, class Scales>
DEV_INLINE void softmax_step(f32x16_t& st, float& m_run, float& l_run,
                             f32x16_t (&ot)[NOT], int hi, float sc2,
                             Visible visible, Scales& scales) {
  float tmax = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float sv = visible(r) ? scales.k(r, st[r]) * sc2 : -INFINITY;
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
  scales.load_v();
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float sv = st[r];
    float p = 0.f, pv = 0.f;
    if (sv != -INFINITY) {
      p = __builtin_amdgcn_exp2f(sv - m_sub);
      pv = scales.v(r, p);
    }
    psum += p;   // the row sum stays unscaled
    st[r] = pv;  // P (* v_scale) goes into the PV MFMA
  }
  psum += half_swap(psum, hi);
  l_run += psum;
}

// P fragments in-register (see attention.hip)
DEV_INLINE void build_p(bf16x8_t (&pfrag)[2], const f32x16_t& st) {
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
}

// O^T += V^T P^T, one d-tile (4 reads) ahead of the MFMAs that use them. The
// caller has issued d-tile 0 into vf[0], so that it flies under the softmax;
// vbase(mt) is the lane's V^T base address of d-tile mt.
template <int D, class VBase>
DEV_INLINE void pv_accumulate(f32x16_t (&ot)[D / 32], tr_frag (&vf)[2][2],
                              const bf16x8_t (&pfrag)[2], VBase vbase) {
  constexpr int NOT = D / 32;
#pragma unroll
  for (int mt = 0; mt < NOT; ++mt) {
    if (mt + 1 < NOT) {
      issue_v_dtile<D>(vf[(mt + 1) & 1], vbase(mt + 1));
      tr_wait<4>(vf[mt & 1][0], vf[mt & 1][1]);
    } else {
      tr_wait<0>(vf[mt & 1][0], vf[mt & 1][1]);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      ot[mt] = RGQA_MFMA(tr_operand(vf[mt & 1][ks]), pfrag[ks], ot[mt], 0, 0,
                         0);
  }
}

// Merge the 4 waves' (m, l, O) into wave 0, lane for lane, over the images at
// `smem`. Every thread of the workgroup calls it; true in wave 0, which holds
// the result, false in the others, which are done. m and l are worked on as
// copies: through the references the bf16 prefill kernel takes 153 registers
// at D 64 instead of 149.
template <int NOT>
DEV_INLINE bool merge_waves(char* smem, int wave, int lane, float& m_out,
                            float& l_out, f32x16_t (&ot)[NOT]) {
  float m_run = m_out, l_run = l_out;
  float* mg = reinterpret_cast<float*>(smem);  // [NW-1][NREG][64]
  constexpr int NREG = NOT * 16 + 2;
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
  if (wave > 0) return false;

#pragma unroll 1
  for (int w = 1; w < NW; ++w) {
    const float* src = mg + (w - 1) * NREG * 64 + lane;
    const float mw = src[(NREG - 2) * 64];
    if (mw == -INFINITY) continue;  // that wave saw no key of this column
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
  m_out = m_run;
  l_out = l_run;
  return true;
}

// the lane's share of its column's row of out: O / l as bf16, 8 bytes a store
template <int NOT>
DEV_INLINE void store_row(short* dst, const f32x16_t (&ot)[NOT], float l_run,
                          int hi) {
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
#pragma unroll
  for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      unsigned int w[2];
      w[0] = cvtpk2(ot[mt][4 * g + 0] * inv, ot[mt][4 * g + 1] * inv);
      w[1] = cvtpk2(ot[mt][4 * g + 2] * inv, ot[mt][4 * g + 3] * inv);
      *reinterpret_cast<unsigned long long*>(dst + 32 * mt + 8 * g + 4 * hi) =
          *reinterpret_cast<unsigned long long*>(w);
    }
}

// the lane's share of split partial `idx` = head * NS + split
template <int NOT>
DEV_INLINE void store_partial(float* partial_out, float* partial_ml,
                              long long idx, const f32x16_t (&ot)[NOT],
                              float m_run, float l_run, int hi) {
  float* dst = partial_out + idx * (NOT * 32);
#pragma unroll
  for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4_t x = {ot[mt][4 * g + 0], ot[mt][4 * g + 1], ot[mt][4 * g + 2],
                   ot[mt][4 * g + 3]};
      *reinterpret_cast<f32x4_t*>(dst + 32 * mt + 8 * g + 4 * hi) = x;
    }
  if (hi == 0) {
    partial_ml[idx * 2] = m_run;
    partial_ml[idx * 2 + 1] = l_run;
  }
}

// merge the NS split partials -> out [n,Hq,D] bf16; one wave per (row, head)
template <int D>
__global__ void combine_kernel(const float* __restrict__ partial_out,
                               const float* __restrict__ partial_ml,
                               short* __restrict__ out, long long nhq,
                               int NS) {
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

// ---- host side -------------------------------------------------------------
// Each entry point checks its tensors' dtypes and devices itself, then calls
// the helper of its step; `name` is the entry point's, the prefix of every
// message. The fp8 entry points pass their scales, the bf16 ones nullptr.

struct Shape {
  long n, T, Hq, Hk, G, D, B, Smax;
  long col_tiles;  // prefill: the grid's tiles of CT columns
};

inline void check_fp8_scales(const char* name, const at::Tensor* k_scale,
                             const at::Tensor* v_scale, const Shape& s) {
  if (!k_scale) return;
  TORCH_CHECK(k_scale->dim() == 3 && k_scale->size(0) == s.B &&
                  k_scale->size(1) == s.Smax && k_scale->size(2) == s.Hk &&
                  v_scale->sizes() == k_scale->sizes(),
              name, ": k_scale and v_scale must both be [B,Smax,Hk]");
}

inline void check_fp8_aligned(const char* name, bool fp8, const at::Tensor& q,
                              const at::Tensor& kpool,
                              const at::Tensor& vpool) {
  if (!fp8) return;
  TORCH_CHECK(ptr_aligned(q.data_ptr(), 16) &&
                  ptr_aligned(kpool.data_ptr(), 16) &&
                  ptr_aligned(vpool.data_ptr(), 16),
              name, ": q and the code pools must be 16-byte aligned");
}

inline Shape check_decode(const char* name, const at::Tensor& q,
                          const at::Tensor& kpool, const at::Tensor& vpool,
                          const at::Tensor* k_scale, const at::Tensor* v_scale,
                          const at::Tensor& rows, const at::Tensor& lens,
                          long window, long max_len, long splits) {
  TORCH_CHECK((q.dim() == 4 && q.size(1) == 1) || q.dim() == 3, name,
              ": q must be [n,1,Hq,D] or [n,Hq,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(), name,
              ": kpool and vpool must both be [B,Smax,Hk,D]");
  Shape s{};
  s.n = s.T = q.size(0), s.Hq = q.size(-2), s.D = q.size(-1);
  s.B = kpool.size(0), s.Smax = kpool.size(1), s.Hk = kpool.size(2);
  TORCH_CHECK(s.n >= 1 && s.B >= 1 && s.Smax >= 1 && s.Hk >= 1 &&
                  kpool.size(3) == s.D,
              name,
              ": empty batch or pool, or pool head_dim != q head_dim");
  check_fp8_scales(name, k_scale, v_scale, s);
  TORCH_CHECK(rows.numel() == s.n && lens.numel() == s.n, name,
              ": rows and lens must have one entry per q row");
  TORCH_CHECK(s.D == 128 || s.D == 64, name,
              ": head_dim must be 64 or 128");
  TORCH_CHECK(s.Hq >= 1 && s.Hq % s.Hk == 0, name, ": Hq % Hk != 0");
  s.G = s.Hq / s.Hk;
  TORCH_CHECK(s.G <= MAXG, name, ": GQA group ", s.G, " exceeds ", MAXG);
  TORCH_CHECK(window >= 0, name, ": window must be >= 0, got ", window);
  TORCH_CHECK(0 <= max_len && max_len <= s.Smax, name,
              ": need 0 <= max_len <= Smax, got ", max_len, ", ", s.Smax);
  TORCH_CHECK(0 <= splits && splits <= MAX_SPLITS, name,
              ": need 0 <= splits <= ", MAX_SPLITS);
  TORCH_CHECK(s.Hk <= 65535, name, ": more than 65535 kv heads");
  check_fp8_aligned(name, k_scale != nullptr, q, kpool, vpool);
  return s;
}

inline Shape check_prefill(const char* name, const at::Tensor& q,
                           const at::Tensor& kpool, const at::Tensor& vpool,
                           const at::Tensor* k_scale,
                           const at::Tensor* v_scale, const at::Tensor& desc,
                           long max_qlen, long max_kvlen, long window) {
  TORCH_CHECK(q.dim() == 3, name, ": q must be [T,Hq,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(), name,
              ": kpool and vpool must both be [B,Smax,Hk,D]");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 4, name,
              ": desc must be [n,4] (slot, q_start, q_len, kv_len)");
  Shape s{};
  s.T = q.size(0), s.Hq = q.size(1), s.D = q.size(2);
  s.B = kpool.size(0), s.Smax = kpool.size(1), s.Hk = kpool.size(2);
  s.n = desc.size(0);
  TORCH_CHECK(s.n >= 1 && s.T >= 1, name, ": empty batch");
  TORCH_CHECK(s.B >= 1 && s.Hk >= 1 && kpool.size(3) == s.D, name,
              ": empty pool or pool head_dim != q head_dim");
  check_fp8_scales(name, k_scale, v_scale, s);
  TORCH_CHECK(s.D == 128 || s.D == 64, name,
              ": head_dim must be 64 or 128");
  TORCH_CHECK(s.Hq >= 1 && s.Hq % s.Hk == 0, name, ": Hq % Hk != 0");
  s.G = s.Hq / s.Hk;
  TORCH_CHECK(s.G <= MAXG, name, ": GQA group ", s.G, " exceeds ", MAXG);
  TORCH_CHECK(window >= 0, name, ": window must be >= 0, got ", window);
  TORCH_CHECK(1 <= max_qlen && max_qlen <= max_kvlen && max_kvlen <= s.Smax,
              name, ": need 1 <= max_qlen <= max_kvlen <= Smax, got ",
              max_qlen, ", ", max_kvlen, ", ", s.Smax);
  TORCH_CHECK(s.Smax <= 0x7fffffffL && s.T <= 0x7fffffffL, name,
              ": Smax or T exceeds 2^31 - 1");
  s.col_tiles = (max_qlen * s.G + CT - 1) / CT;
  TORCH_CHECK(s.col_tiles <= 0x7fffffffL, name,
              ": more than 2^31 - 1 column tiles");
  TORCH_CHECK(s.n <= 65535 && s.Hk <= 65535, name,
              ": more than 65535 sequences or kv heads");
  check_fp8_aligned(name, k_scale != nullptr, q, kpool, vpool);
  return s;
}

inline int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      cus <= 0)
    cus = 256;
  return cus;
}

// decode's split count NS: `splits` if given, else about two workgroups per
// CU and no split shorter than one tile per wave
inline long plan_splits(const char* name, const Shape& s,
                        const at::Tensor& lens, long window, long max_len,
                        long splits) {
  if (max_len == 0) {  // the one host read; callers that know a bound skip it
    max_len = lens.max().item<long>();
    TORCH_CHECK(max_len <= s.Smax, name, ": lens.max() = ", max_len,
                " exceeds the pool's Smax = ", s.Smax);
    max_len = std::max<long>(max_len, 1);
  }
  if (splits != 0) return splits;
  const long span = window > 0 ? std::min(max_len, window) : max_len;
  const long longest = std::max<long>(span / (KT * NW), 1);
  const long want = (2 * device_cus() + s.n * s.Hk - 1) / (s.n * s.Hk);
  return std::min<long>(std::min(want, longest), MAX_SPLITS);
}

// decode's result and, for NS > 1, its split partials
struct DecodeOut {
  at::Tensor out, pout, pml;
  float* pout_ptr() const {
    return pout.defined() ? pout.data_ptr<float>() : nullptr;
  }
  float* pml_ptr() const {
    return pml.defined() ? pml.data_ptr<float>() : nullptr;
  }
};

inline DecodeOut alloc_decode(const at::Tensor& q, const Shape& s, long NS) {
  DecodeOut o;
  o.out = at::empty({s.n, 1, s.Hq, s.D}, q.options());
  if (NS > 1) {
    auto opts = q.options().dtype(at::kFloat);
    o.pout = at::empty({s.n, s.Hq, NS, s.D}, opts);
    o.pml = at::empty({s.n, s.Hq, NS, 2}, opts);
  }
  return o;
}

// the partials of NS > 1 splits -> o.out. A template, so that only the units
// that call it carry the kernel.
template <int D>
void launch_combine(const DecodeOut& o, const Shape& s, long NS,
                    hipStream_t stream) {
  const long long nhq = (long long)s.n * s.Hq;
  dim3 grid((unsigned)((nhq + 3) / 4));
  hipLaunchKernelGGL(combine_kernel<D>, grid, dim3(256), 0, stream,
                     o.pout_ptr(), o.pml_ptr(),
                     reinterpret_cast<short*>(o.out.data_ptr()), nhq, (int)NS);
  HIP_CHECK_KERNEL();
}

}  // namespace rgqa
