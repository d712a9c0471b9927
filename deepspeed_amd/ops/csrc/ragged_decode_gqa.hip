// MFMA split-KV decode attention over the KV slot pool for MI355X (gfx950):
// any GQA group up to 32 and an optional sliding window. The tile engine (MFMA
// roles, softmax, masking rule, wave merge, split partials and their combine
// kernel) is ragged_gqa.h; this unit is decode's columns and key range and the
// bf16 pool's staging.
//
// Role parity: reference inference/v2 blocked flash decode
// (deepspeed/inference/v2/kernels/ragged_ops/). ragged_decode.hip is templated
// on the group G = Hq/Hk and spends a 6-step butterfly per (key, q head); here
// the G query heads that share a kv head are the COLUMNS of one 32x32x16 MFMA
// (column c < G is query head hk*G + c, columns >= G are zero), so one build
// serves G = 1..32 and a K row is multiplied with all of them at once.
//
// Row i attends pool positions [lo_i, len_i) of slot rows[i], len_i clamped
// into [0, Smax], lo_i = max(0, len_i - window) under a window, else 0.
//
// Work split: grid (n, Hk, NS), one workgroup of 4 waves per (row, kv head,
// split). Split s covers [lo + s*per, lo + (s+1)*per) cut at len, per =
// ceil((len - lo) / NS) rounded up to whole 32-key tiles: every workgroup
// derives its range from its own row's length, so the host needs no length
// (max_len only sizes NS). A split past the row's end writes the empty
// partial (m = -inf, l = 0). A key is visible iff it is in [start, end).
//
// Data movement: decode is HBM-bound, so each K and V byte of a split is
// fetched once per workgroup, by full-row coalesced loads (consecutive lanes
// take consecutive 16 bytes of a pool row, 64 lanes = 4 rows at D 128), held
// in registers, and stored into the wave's own K and V image. Tile t+4's
// loads are issued right after tile t's registers went to LDS and fly under
// tile t's MFMAs.
//
// LDS per workgroup: 4 waves x 2 images x 32 x 2D bytes = 64 KiB at D 128,
// 32 KiB at D 64. Resident workgroups per CU: 2 at D 128 (160 KiB LDS; the
// kernel is held to 256 registers for it), 3 at D 64 (148 registers; LDS would
// allow 5). Each resident wave has a whole tile of K and V in flight: 32 KiB
// per CU at D 128, 24 KiB at D 64.
#include <torch/extension.h>

#include "ragged_gqa.h"

namespace rgqa::decode {

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

  // ---- Q^T, column c < G = head hk*G + c -------------------------------------
  bf16x8_t qfrag[NQF];
  load_q(qfrag, l31 < G, hi, [&] { return q + (head0 + l31) * D; });

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
      st = RGQA_MFMA(kf, qfrag[ks], st, 0, 0, 0);
    }

    // V's operand for d-tile 0: the transposed reads fly under the softmax
    tr_frag vf[2][2];
    issue_v_dtile<D>(vf[0], vbase[0]);

    // ---- online softmax; keys at or past the split's end are masked --------
    NoScales none;
    softmax_step(st, m_run, l_run, ot, hi, sc2, [&](int r) {
      return kb + (r & 3) + 8 * (r >> 2) + 4 * hi < end;
    }, none);

    bf16x8_t pfrag[2];
    build_p(pfrag, st);
    pv_accumulate<D>(ot, vf, pfrag, [&](int mt) { return vbase[mt]; });
  }

  if (!merge_waves(smem, wave, lane, m_run, l_run, ot)) return;

  if (l31 >= G) return;  // columns past the group hold no head
  const long long head = head0 + l31;
  if (NS == 1)
    store_row(out + head * D, ot, l_run, hi);
  else
    store_partial(partial_out, partial_ml, head * NS + s, ot, m_run, l_run,
                  hi);
}

}  // namespace rgqa::decode

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
  const char* name = "ragged_decode_gqa";
  const rgqa::Shape a = rgqa::check_decode(name, q, kpool, vpool, nullptr,
                                           nullptr, rows, lens, window,
                                           max_len, splits);
  const long NS = rgqa::plan_splits(name, a, lens, window, max_len, splits);
  const rgqa::DecodeOut o = rgqa::alloc_decode(q, a, NS);
  const float scale = 1.0f / std::sqrt((float)a.D);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((unsigned)a.n, (unsigned)a.Hk, (unsigned)NS);

#define LAUNCH(DD)                                                          \
  hipLaunchKernelGGL((rgqa::decode::ragged_decode_gqa_kernel<DD>), grid,    \
                     dim3(256), 0, stream.stream(),                         \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const short*>(kpool.data_ptr()),      \
                     reinterpret_cast<const short*>(vpool.data_ptr()),      \
                     rows.data_ptr<int64_t>(), lens.data_ptr<int64_t>(),    \
                     o.pout_ptr(), o.pml_ptr(),                             \
                     reinterpret_cast<short*>(o.out.data_ptr()), (int)a.Hq, \
                     (int)a.Hk, (int)a.G, (int)a.B, (int)a.Smax, (int)NS,   \
                     (int)std::min<long>(window, a.Smax), scale)
  if (a.D == 128)
    LAUNCH(128);
  else
    LAUNCH(64);
#undef LAUNCH
  HIP_CHECK_KERNEL();
  if (NS > 1) {
    if (a.D == 128)
      rgqa::launch_combine<128>(o, a, NS, stream.stream());
    else
      rgqa::launch_combine<64>(o, a, NS, stream.stream());
  }
  return o.out;
}
