// MFMA ragged prefill attention over the KV slot pool for MI355X (gfx950): the
// fused serving step for any GQA group up to 32 and an optional sliding
// window. The tile engine (MFMA roles, softmax, masking rule, wave merge,
// epilogue) is ragged_gqa.h; this unit is prefill's (token, head) columns,
// their per-column band and key range, and the bf16 pool's staging, which is
// ragged_decode_gqa.hip's.
//
// Role parity: reference inference/v2 blocked flash attention with
// per-sequence "atoms" (deepspeed/inference/v2/kernels/ragged_ops/).
// ragged_prefill.hip gives a workgroup (32 tokens, one Q HEAD): every K and V
// row is fetched once per q head, a decode row fills 1 of the MFMA's 32
// columns, and V is transposed by hand.
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
// from `start` (nothing is aligned down below the band). These two bounds are
// the causal skip and the band skip. Inside them a key is visible to column c
// iff lo_c <= key <= p_c, so a lane may see no key in a whole tile or in a
// wave's whole share, and in the merge a wave's m may be -inf for some
// columns only.
//
// LDS per workgroup is the decode kernel's: 64 KiB at D 128, 32 KiB at D 64.
// The kernel is held to 256 registers (two workgroups per CU at D 128).
#include <torch/extension.h>

#include "ragged_gqa.h"

namespace rgqa::prefill {

template <int D>
using Piece = rgqa::Piece<D, 2>;  // bf16 rows

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

  // ---- Q^T, 0 in pad columns -------------------------------------------------
  bf16x8_t qfrag[NQF];
  load_q(qfrag, my_valid, hi, [&] { return q + my_row; });

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
      st = RGQA_MFMA(kf, qfrag[ks], st, 0, 0, 0);
    }

    // V's operand for d-tile 0: the transposed reads fly under the softmax
    tr_frag vf[2][2];
    issue_v_dtile<D>(vf[0], vbase[0]);

    // ---- online softmax over the lane's band -------------------------------
    // my_p < end, so a key the range clamped or zeroed is hidden as well
    NoScales none;
    softmax_step(st, m_run, l_run, ot, hi, sc2, [&](int r) {
      const int key = kb + (r & 3) + 8 * (r >> 2) + 4 * hi;
      return key >= my_lo && key <= my_p;
    }, none);

    bf16x8_t pfrag[2];
    build_p(pfrag, st);
    pv_accumulate<D>(ot, vf, pfrag, [&](int mt) { return vbase[mt]; });
  }

  if (!merge_waves(smem, wave, lane, m_run, l_run, ot)) return;

  if (!my_valid) return;  // pad columns hold no (token, head)
  store_row(out + my_row, ot, l_run, hi);
}

}  // namespace rgqa::prefill

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
  const rgqa::Shape a =
      rgqa::check_prefill("ragged_prefill_gqa", q, kpool, vpool, nullptr,
                          nullptr, desc, max_qlen, max_kvlen, window);
  auto out = at::empty_like(q);
  const float scale = 1.0f / std::sqrt((float)a.D);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((unsigned)a.col_tiles, (unsigned)a.n, (unsigned)a.Hk);

#define LAUNCH(DD)                                                          \
  hipLaunchKernelGGL((rgqa::prefill::ragged_prefill_gqa_kernel<DD>), grid,  \
                     dim3(256), 0, stream.stream(),                         \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const short*>(kpool.data_ptr()),      \
                     reinterpret_cast<const short*>(vpool.data_ptr()),      \
                     desc.data_ptr<int64_t>(),                              \
                     reinterpret_cast<short*>(out.data_ptr()), (int)a.T,    \
                     (int)a.Hq, (int)a.Hk, (int)a.G, (int)a.B, (int)a.Smax, \
                     (int)max_kvlen, (int)std::min<long>(window, a.Smax),   \
                     scale)
  if (a.D == 128)
    LAUNCH(128);
  else
    LAUNCH(64);
#undef LAUNCH
  HIP_CHECK_KERNEL();
  return out;
}
