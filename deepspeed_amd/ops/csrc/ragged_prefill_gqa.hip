// MFMA ragged prefill attention over the KV slot pool for MI355X (gfx950): the
// fused serving step for any GQA group up to 32 and an optional sliding
// window.
//
// Role parity: reference inference/v2 blocked flash attention with
// per-sequence "atoms" (deepspeed/inference/v2/kernels/ragged_ops/).
// ragged_prefill.hip gives a workgroup (32 tokens, one Q HEAD): every K and V
// row is fetched once per q head, a decode row fills 1 of the MFMA's 32
// columns, and V is transposed by hand. Here the design of
// ragged_decode_gqa.hip serves the whole ragged step.
//
// Contract (that of ragged_prefill): q [T,Hq,D] bf16, pools [B,Smax,Hk,D]
// bf16, desc [n,4] i64 rows (slot, q_start, q_len, kv_len), out [T,Hq,D].
// Local token j of a sequence lives at q[q_start + j], has position
// p = kv_len - q_len + j and attends pool positions [lo, p] of its slot,
// lo = max(0, p - window + 1) under a window (a token sees its last `window`
// positions, itself included), else 0.
//
// Columns are (token, head) pairs. Column c of a sequence runs over
// [0, q_len * G): token j = c / G, head g = c % G, which is q head hk*G + g.
// Grid (ceil(max_qlen * G / 32), n, Hk), one workgroup of 4 waves per tile of
// 32 consecutive columns of one (sequence, kv head). A tile may start and end
// inside a token (G = 3, 7, ...): every lane derives its own token, head, p
// and lo and its own q and out addresses. Columns at or past q_len * G are pad
// lanes: they see no key and write nothing. A decode row uses G columns and
// reads K/V once per KV head; a chunk of q_len < 32 tokens fills q_len * G
// columns.
//
// Key range of a workgroup: [start, end) with end = p(last valid token) + 1
// and start = lo(first token) under a window, else 0. Tiles of 32 keys run
// from `start` (nothing is aligned down below the band); wave w takes tiles
// w, w+4, ... These two bounds are the causal skip and the band skip. Inside
// them the mask is per element and by SELECT: lo_c <= key <= p_c, else the
// score is -inf and P is exactly 0. A lane may see no key in a whole tile or
// in a wave's whole share: the m == -inf guards cover it, in the tile loop and
// in the merge (where a wave's m may be -inf for some columns only).
//
// Per tile, as in ragged_decode_gqa.hip (layouts at the top of attention.hip):
//   loads          full-row coalesced 16-byte loads of K and V into registers,
//                  the wave's tile t+4 in flight under tile t's MFMAs, then
//                  stored into the wave's private row-major K and V images
//                  [32][D] (the swizzles of flash_fwd_layout.h)
//   S^T = K Q^T    Q^T fragments loaded once per lane into registers; C column
//                  = lane&31, so the softmax of a column is lane-local plus
//                  one permlane32_swap
//   P              built in registers (cvt_pk + permlane32_swap)
//   O^T += V^T P^T V's operand by ds_read_b64_tr_b16 one d-tile ahead;
//                  nothing is transposed by hand
// The images are private to a wave and a wave's LDS operations complete in
// order, so the tile loop has no barrier. The 4 waves' (m, l, O) are merged
// lane for lane over the image space; the epilogue normalises and writes bf16,
// 8 bytes per store, to the lane's own (token, head) row of out.
//
// Nothing outside [start, end) is loaded: K rows past `end` are clamped onto
// row end-1, V rows past it are staged as zeros, so NaN or another request's
// rows past kv_len, below the band or in other slots cannot reach a live
// value through 0 * NaN.
//
// LDS per workgroup is the decode kernel's: 64 KiB at D 128, 32 KiB at D 64.
// The kernel is held to 256 registers (two workgroups per CU at D 128).
#include <torch/extension.h>

#include <algorithm>

#include "common.h"
#include "flash_fwd_layout.h"
#include "lds_tr_read.h"

namespace rpgqa {

using bf16x8_t = __attribute__((ext_vector_type(8))) short;
using f32x16_t = __attribute__((ext_vector_type(16))) float;
#define RPG_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16

constexpr int CT = 32;    // (token, head) columns per workgroup
constexpr int KT = 32;    // keys per tile
constexpr int NW = 4;     // waves per workgroup
constexpr int MAXG = 32;  // q heads per kv head

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

template <int D>
__launch_bounds__(256, 2)
__global__ void ragged_prefill_gqa_kernel(
    const short* __restrict__ q, const short* __restrict__ kpool,
    const short* __restrict__ vpool, const int64_t* __restrict__ desc,
    short* __restrict__ out, int T, int Hq, int Hk, int G, int B, int Smax,
    int max_kvlen, int window, float scale) {
  __shared__ __attribute__((aligned(16))) char smem[Smem<D>::BYTES];

  constexpr int NQF = D / 16;  // Q k-slices
  constexpr int NOT = D / 32;  // O^T d m-tiles
  constexpr int NL = Piece<D>::NL;
  using namespace fwd_layout;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  const int seq = blockIdx.y;
  const int hk = blockIdx.z;

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
  const long long ncol = (long long)q_len * G;
  // Workgroups go to the 8 XCDs round-robin in launch order, so with a tile
  // count that is a multiple of 8 tile 0 of every sequence -- all a decode
  // row has -- would meet on one XCD. Rotating the tile index by the sequence
  // deals them to all of them.
  const unsigned tile = (blockIdx.x + (unsigned)seq) % gridDim.x;
  const long long c0 = (long long)tile * CT;
  if (c0 >= ncol) return;  // tile past this sequence's columns

  // ---- this lane's column: token, head, last and first visible key --------
  const int j_first = (int)(c0 / G);
  const int g_first = (int)(c0 - (long long)j_first * G);
  const int n_valid = (int)min((long long)CT, ncol - c0);
  const bool my_valid = l31 < n_valid;
  const int my_j = j_first + (g_first + l31) / G;
  const int my_g = (g_first + l31) % G;
  const int p0 = kv_len - q_len;  // position of local token 0
  // p = -1 with lo = 0 hides every key from a pad lane
  const int my_p = my_valid ? p0 + my_j : -1;
  const int my_lo = window > 0 ? max(0, my_p - window + 1) : 0;

  // ---- the workgroup's key range: causal skip and band skip ---------------
  const int j_last = j_first + (g_first + n_valid - 1) / G;
  const int end = p0 + j_last + 1;  // <= kv_len
  const int start = window > 0 ? max(0, p0 + j_first - window + 1) : 0;
  const int n_tiles = (end - start + KT - 1) / KT;  // start <= p(j_first) < end

  const long long kvrs = (long long)Hk * D;
  const short* kp = kpool + (slot * Smax) * kvrs + hk * D;
  const short* vp = vpool + (slot * Smax) * kvrs + hk * D;
  // this lane's row of q and out
  const long long my_row =
      ((q_start + (my_valid ? my_j : j_first)) * Hq + hk * G +
       (my_valid ? my_g : 0)) * D;

  // ---- Q^T: qfrag[ks] = Q[token, head of column l31][16*ks + hi*8 .. +7],
  // 0 in pad columns -----------------------------------------------------------
  bf16x8_t qfrag[NQF];
#pragma unroll
  for (int ks = 0; ks < NQF; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) qfrag[ks][j] = 0;
  if (my_valid) {
    const short* src = q + my_row + hi * 8;
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

    // ---- S^T = K Q^T: rows key = kb + (r&3)+8*(r>>2)+4*hi, col = column ----
    f32x16_t st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NQF; ++ks) {
      bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(
          kimg + k_row_read_addr<D>(lane, 0, ks));
      st = RPG_MFMA(kf, qfrag[ks], st, 0, 0, 0);
    }

    // V's operand for d-tile 0: the transposed reads fly under the softmax
    tr_frag vf[2][2];
    issue_v_dtile<D>(vf[0], vbase[0]);

    // ---- online softmax, lane-local column; masked by select ---------------
    // my_p < end, so a key the range clamped or zeroed is hidden as well
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kb + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const float sv =
          (key >= my_lo && key <= my_p) ? st[r] * sc2 : -INFINITY;
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
        ot[mt] = RPG_MFMA(tr_operand(vf[mt & 1][ks]), pfrag[ks], ot[mt], 0, 0,
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
    if (mw == -INFINITY) continue;  // that wave saw no key of this column
    const float m_new = fmaxf(m_run, mw);
    const float c0w =
        (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
    const float c1w = __builtin_amdgcn_exp2f(mw - m_new);
    l_run = l_run * c0w + src[(NREG - 1) * 64] * c1w;
#pragma unroll
    for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ot[mt][r] = ot[mt][r] * c0w + src[(mt * 16 + r) * 64] * c1w;
    m_run = m_new;
  }

  if (!my_valid) return;  // pad columns hold no (token, head)
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
  short* dst = out + my_row;
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

}  // namespace rpgqa

at::Tensor ragged_prefill_gqa(at::Tensor q, at::Tensor kpool,
                              at::Tensor vpool, at::Tensor desc, long max_qlen,
                              long max_kvlen, long window) {
  CHECK_ARG(q, at::kBFloat16);
  CHECK_ARG(kpool, at::kBFloat16);
  CHECK_ARG(vpool, at::kBFloat16);
  CHECK_ARG(desc, at::kLong);
  CHECK_ON(kpool, q);
  CHECK_ON(vpool, q);
  CHECK_ON(desc, q);
  TORCH_CHECK(q.dim() == 3, "ragged_prefill_gqa: q must be [T,Hq,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(),
              "ragged_prefill_gqa: kpool and vpool must both be "
              "[B,Smax,Hk,D]");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 4,
              "ragged_prefill_gqa: desc must be [n,4] "
              "(slot, q_start, q_len, kv_len)");
  const long T = q.size(0), Hq = q.size(1), D = q.size(2);
  const long B = kpool.size(0), Smax = kpool.size(1), Hk = kpool.size(2);
  const long n = desc.size(0);
  TORCH_CHECK(n >= 1 && T >= 1, "ragged_prefill_gqa: empty batch");
  TORCH_CHECK(B >= 1 && Hk >= 1 && kpool.size(3) == D,
              "ragged_prefill_gqa: empty pool or pool head_dim != q "
              "head_dim");
  TORCH_CHECK(D == 128 || D == 64,
              "ragged_prefill_gqa: head_dim must be 64 or 128");
  TORCH_CHECK(Hq >= 1 && Hq % Hk == 0, "ragged_prefill_gqa: Hq % Hk != 0");
  const long G = Hq / Hk;
  TORCH_CHECK(G <= rpgqa::MAXG, "ragged_prefill_gqa: GQA group ", G,
              " exceeds ", rpgqa::MAXG);
  TORCH_CHECK(window >= 0, "ragged_prefill_gqa: window must be >= 0, got ",
              window);
  TORCH_CHECK(1 <= max_qlen && max_qlen <= max_kvlen && max_kvlen <= Smax,
              "ragged_prefill_gqa: need 1 <= max_qlen <= max_kvlen <= Smax, "
              "got ", max_qlen, ", ", max_kvlen, ", ", Smax);
  TORCH_CHECK(Smax <= 0x7fffffffL && T <= 0x7fffffffL,
              "ragged_prefill_gqa: Smax or T exceeds 2^31 - 1");
  const long col_tiles = (max_qlen * G + rpgqa::CT - 1) / rpgqa::CT;
  TORCH_CHECK(col_tiles <= 0x7fffffffL,
              "ragged_prefill_gqa: more than 2^31 - 1 column tiles");
  TORCH_CHECK(n <= 65535 && Hk <= 65535,
              "ragged_prefill_gqa: more than 65535 sequences or kv heads");

  auto out = at::empty_like(q);
  const float scale = 1.0f / std::sqrt((float)D);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((unsigned)col_tiles, (unsigned)n, (unsigned)Hk);

#define LAUNCH(DD)                                                          \
  hipLaunchKernelGGL((rpgqa::ragged_prefill_gqa_kernel<DD>), grid,          \
                     dim3(256), 0, stream.stream(),                         \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const short*>(kpool.data_ptr()),      \
                     reinterpret_cast<const short*>(vpool.data_ptr()),      \
                     desc.data_ptr<int64_t>(),                              \
                     reinterpret_cast<short*>(out.data_ptr()), (int)T,      \
                     (int)Hq, (int)Hk, (int)G, (int)B, (int)Smax,           \
                     (int)max_kvlen, (int)std::min<long>(window, Smax),     \
                     scale)
  if (D == 128)
    LAUNCH(128);
  else
    LAUNCH(64);
#undef LAUNCH
  HIP_CHECK_KERNEL();
  return out;
}
