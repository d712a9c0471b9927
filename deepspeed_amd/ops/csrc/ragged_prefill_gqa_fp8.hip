// MFMA ragged prefill attention over the fp8 KV slot pool for MI355X (gfx950):
// the fused serving step for any GQA group up to 32 and an optional sliding
// window, over e4m3 codes.
//
// The join of two kernels of this directory. The contract (with code pools
// [B,Smax,Hk,D] e4m3fn and scales [B,Smax,Hk] fp32, kv_fp8.h), the grid, the
// (token, head) column tiling, the per-column band and the key range are
// ragged_prefill_gqa.hip's; the staging of codes and scales, two tiles ahead,
// is ragged_decode_gqa_fp8.hip's. The tile engine and its fp8 arithmetic are
// ragged_gqa.h. ragged_prefill_fp8.hip gives a workgroup (32 tokens, one Q
// HEAD), fetches every K and V row once per q head, transposes V by hand,
// serves G in {1, 2, 4, 8} and has no window.
//
// Nothing outside [start, end) is loaded: K rows and scales past `end` come
// from row end-1 (clamped index), the staged V rows and both scales past it
// are zeros. So NaN codes and NaN / inf scales below the band, past kv_len or
// in other slots cannot reach a live value.
//
// Per-lane column state in the tile loop is ONE register, p: the band test is
// key <= p && key > p - window (keys are >= start >= 0, so this is lo <= key),
// and key <= p alone without a window. The lane's q / out row is derived
// again in the epilogue instead of living through the loop. The images' lane
// addresses are one register each, rebased per tile (see
// ragged_decode_gqa_fp8.hip).
//
// Resources (the compiler's report for gfx950, built without packed fp32):
//   LDS per workgroup  4 waves x (2 images x 32 x 2D + 256 bytes of scales):
//                      66560 bytes at D 128, 33792 at D 64.
//   registers          250 at D 128, 165 at D 64 (ragged_decode_gqa_fp8: 238 /
//                      154); no AGPRs, ZERO scratch, two stages at both.
//   resident per CU    2 workgroups at D 128 (registers, launch bound; LDS
//                      130 of 160 KiB), 3 at D 64 (registers; LDS would
//                      allow 4).
#include <torch/extension.h>

#include "kv_fp8.h"
#include "ragged_gqa.h"

namespace rgqa::prefill_fp8 {

template <int D>
using Smem = rgqa::Smem<D, true>;  // with the waves' staged scales
template <int D>
using Piece = rgqa::Piece<D, 1>;  // code bytes

// one tile in flight: its K and V codes and this lane's scale
template <int D>
struct Stage {
  u32x4_t k[Piece<D>::NL], v[Piece<D>::NL];
  float sc;
};

// keys kb .. kb+31 of one (slot, kv head) into registers; lane l31 of half hi
// takes the k (hi 0) or v (hi 1) scale of key kb + l31. A row at or past `end`
// repeats row end-1 (end > start >= 0: always a row of the range).
template <int D>
DEV_INLINE void load_tile(Stage<D>& st, const unsigned char* kp,
                          const unsigned char* vp, const float* scp,
                          long long kvrs, int Hk, int kb, int end, int lane) {
#pragma unroll
  for (int j = 0; j < Piece<D>::NL; ++j) {
    const int key = min(kb + Piece<D>::row(j, lane), end - 1);
    const long long off = (long long)key * kvrs + Piece<D>::cb(j, lane);
    st.k[j] = *reinterpret_cast<const u32x4_t*>(kp + off);
    st.v[j] = *reinterpret_cast<const u32x4_t*>(vp + off);
  }
  st.sc = scp[(long long)min(kb + (lane & 31), end - 1) * Hk];
}

// Element offset of column c0 + l31's row in q and out: token c / G, head
// hk*G + c % G. Only called for a valid column.
DEV_INLINE long long column_row(long long q_start, int j_first, int g_first,
                                int l31, int G, int Hq, int hk, int D) {
  const int j = j_first + (g_first + l31) / G;
  const int g = (g_first + l31) % G;
  return ((q_start + j) * Hq + hk * G + g) * D;
}

template <int D>
__launch_bounds__(256, 2)
__global__ void ragged_prefill_gqa_fp8_kernel(
    const short* __restrict__ q, const unsigned char* __restrict__ kpool,
    const unsigned char* __restrict__ vpool, const float* __restrict__ kscale,
    const float* __restrict__ vscale, const int64_t* __restrict__ desc,
    short* __restrict__ out, int T, int Hq, int Hk, int G, int B, int Smax,
    int max_kvlen, int window, float scale) {
  // 1 KiB: the lane addresses below are XORed with constants in bits 4..7
  __shared__ __attribute__((aligned(1024))) char smem[Smem<D>::BYTES];

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
  // see ragged_prefill_gqa.hip: deals tile 0 of the sequences to all XCDs
  const unsigned tile_idx = (blockIdx.x + (unsigned)seq) % gridDim.x;
  const long long c0 = (long long)tile_idx * CT;
  if (c0 >= ncol) return;  // tile past this sequence's columns

  // ---- this lane's column: token and last visible key ----------------------
  const int j_first = (int)(c0 / G);
  const int g_first = (int)(c0 - (long long)j_first * G);
  const int n_valid = (int)min((long long)CT, ncol - c0);
  const int p0 = kv_len - q_len;  // position of local token 0
  // p = -1 hides every key (all >= 0) from a pad lane
  const int my_p = l31 < n_valid ? p0 + j_first + (g_first + l31) / G : -1;

  // ---- the workgroup's key range: causal skip and band skip ----------------
  const int j_last = j_first + (g_first + n_valid - 1) / G;
  const int end = p0 + j_last + 1;  // <= kv_len
  const int start = window > 0 ? max(0, p0 + j_first - window + 1) : 0;
  const int n_tiles = (end - start + KT - 1) / KT;  // start <= p(j_first) < end

  const long long kvrs = (long long)Hk * D;  // bytes per position
  const unsigned char* kp = kpool + (slot * Smax) * kvrs + hk * D;
  const unsigned char* vp = vpool + (slot * Smax) * kvrs + hk * D;
  // this lane's scale column: k_scale for the lower half, v_scale above
  const float* scp = (hi ? vscale : kscale) + (slot * Smax) * Hk + hk;

  // ---- Q^T, 0 in pad columns -------------------------------------------------
  bf16x8_t qfrag[NQF];
  load_q(qfrag, l31 < n_valid, hi, [&] {
    return q + column_row(q_start, j_first, g_first, l31, G, Hq, hk, D);
  });

  const float sc2 = scale * 1.44269504f;  // exp2 domain
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t ot[NOT];  // O^T accum: rows d = 32*mt + (reg&3)+8*(reg>>2)+4*hi
#pragma unroll
  for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[mt][r] = 0.f;

  // this wave's images, its staged scales and its lane's read addresses
  char* kimg = smem + wave * 2 * Smem<D>::IMG;
  char* vimg = kimg + Smem<D>::IMG;
  float* scl = reinterpret_cast<float*>(smem + Smem<D>::MAIN +
                                        wave * Smem<D>::SC);  // k[32], v[32]
  // Lane addresses into the images, one register each; the others differ by
  // constants (the derivation is in ragged_decode_gqa_fp8.hip):
  //   K piece (j, half h) at (kst0 ^ (16h ^ k_xor(j*RJ))) + j*RJ*RB
  //   V piece (j, half h) at vst0 + j*RJ*RB + 16h
  //   K row read of slice ks at krd0 ^ 32ks, V^T base of d-tile mt at
  //   vtr0 ^ 64mt.
  // tile() hides them from the optimiser once per tile: hoisted out of the
  // loop as loop invariants per piece, slice and d-tile they spill.
  constexpr int RB = Smem<D>::RB;
  unsigned kst0 = lds_addr(
      kimg + k_off<D>(Piece<D>::row(0, lane), 2 * Piece<D>::cb(0, lane)));
  unsigned vst0 = lds_addr(
      vimg + v_off<D>(Piece<D>::row(0, lane), 2 * Piece<D>::cb(0, lane)));
  unsigned krd0 = lds_addr(kimg + k_row_read_addr<D>(lane, 0, 0));
  unsigned vtr0 = lds_addr(vimg + v_tr_lane_base<D>(lane, 0));
  using lds_b128 = __attribute__((address_space(3))) bf16x8_t;

  // one tile: stage -> LDS, the stage's reload, S, softmax, PV
  auto tile = [&](Stage<D>& sg, int t,
                  bool reload) __attribute__((always_inline)) {
    const int kb = start + t * KT;
    asm volatile("" : "+v"(kst0), "+v"(vst0), "+v"(krd0), "+v"(vtr0));

    // ---- codes -> bf16 images; V rows and scales past the end are zeros ---
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const bool live = kb + Piece<D>::row(j, lane) < end;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint2 kc = {sg.k[j][2 * h], sg.k[j][2 * h + 1]};
        const uint2 vc = {sg.v[j][2 * h], sg.v[j][2 * h + 1]};
        bf16x8_t vz = kvfp8::widen8(vc);
        if (!live) {
#pragma unroll
          for (int e = 0; e < 8; ++e) vz[e] = 0;
        }
        constexpr int RJ = Piece<D>::RJ;
        *(lds_b128*)((kst0 ^ (16 * h ^ k_xor<D>(j * RJ))) + j * RJ * RB) =
            kvfp8::widen8(kc);
        *(lds_b128*)(vst0 + j * RJ * RB + 16 * h) = vz;
      }
    }
    scl[lane] = kb + l31 < end ? sg.sc : 0.f;
    // the tile two rounds ahead flies under this one's and the next's compute
    if (reload)
      load_tile<D>(sg, kp, vp, scp, kvrs, Hk, kb + 2 * NW * KT, end, lane);

    // ---- S^T = K Q^T: rows key = kb + (r&3)+8*(r>>2)+4*hi, col = column ----
    f32x16_t st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NQF; ++ks) {
      bf16x8_t kf = *(const lds_b128*)(krd0 ^ (32 * ks));
      st = RGQA_MFMA(kf, qfrag[ks], st, 0, 0, 0);
    }
    TileScales scales{scl, hi};
    scales.load_k();

    // V's operand for d-tile 0: the transposed reads fly under the softmax
    tr_frag vf[2][2];
    issue_v_dtile<D>(vf[0], vtr0);

    // ---- online softmax over the lane's band -------------------------------
    // band of this lane's column relative to its first score row: row offset
    // o = (r&3) + 8*(r>>2) is visible iff dlo < o <= dhi. my_p < end, so a
    // key the range clamped or zeroed is hidden as well.
    const int dhi = my_p - kb - 4 * hi;
    const int dlo = window > 0 ? dhi - window : -1;  // o >= 0
    softmax_step(st, m_run, l_run, ot, hi, sc2, [&](int r) {
      const int o = (r & 3) + 8 * (r >> 2);
      return o <= dhi && o > dlo;
    }, scales);

    bf16x8_t pfrag[2];
    build_p(pfrag, st);
    pv_accumulate<D>(ot, vf, pfrag,
                     [&](int mt) { return vtr0 ^ (64 * mt); });
  };

  // Two stages: A holds the wave's tiles 0, 2, 4, ..., B its tiles 1, 3, ...
  // Every load of the pair loop is UNCONDITIONAL, so the compiler's vmcnt
  // waits are exact (see ragged_decode_gqa_fp8.hip). A tile past the range's
  // end is load_tile's clamp: one row, end-1, again and again. A wave with no
  // tile at all (wave >= n_tiles) loads that row twice and computes nothing.
  Stage<D> sa, sb;
  load_tile<D>(sa, kp, vp, scp, kvrs, Hk, start + wave * KT, end, lane);
  load_tile<D>(sb, kp, vp, scp, kvrs, Hk, start + (wave + NW) * KT, end, lane);
  int t = wave;  // wave-uniform control flow: EXEC stays full
  for (; t + NW < n_tiles; t += 2 * NW) {
    tile(sa, t, true);
    tile(sb, t + NW, true);
  }
  if (t < n_tiles) tile(sa, t, false);  // an odd count's last tile

  if (!merge_waves(smem, wave, lane, m_run, l_run, ot)) return;

  // the lane's column again, from a copy of l31 the optimiser cannot tie to
  // the one above: the row offset then costs no registers in the tile loop
  int l31e = l31;
  asm volatile("" : "+v"(l31e));
  if (l31e >= n_valid) return;  // pad columns hold no (token, head)
  store_row(out + column_row(q_start, j_first, g_first, l31e, G, Hq, hk, D),
            ot, l_run, hi);
}

}  // namespace rgqa::prefill_fp8

at::Tensor ragged_prefill_gqa_fp8(at::Tensor q, at::Tensor kpool,
                                  at::Tensor vpool, at::Tensor k_scale,
                                  at::Tensor v_scale, at::Tensor desc,
                                  long max_qlen, long max_kvlen, long window) {
  CHECK_ARG(q, at::kBFloat16);
  CHECK_ARG(kpool, at::kFloat8_e4m3fn);
  CHECK_ARG(vpool, at::kFloat8_e4m3fn);
  CHECK_ARG(k_scale, at::kFloat);
  CHECK_ARG(v_scale, at::kFloat);
  CHECK_ARG(desc, at::kLong);
  CHECK_ON(kpool, q);
  CHECK_ON(vpool, q);
  CHECK_ON(k_scale, q);
  CHECK_ON(v_scale, q);
  CHECK_ON(desc, q);
  const rgqa::Shape a =
      rgqa::check_prefill("ragged_prefill_gqa_fp8", q, kpool, vpool, &k_scale,
                          &v_scale, desc, max_qlen, max_kvlen, window);
  auto out = at::empty_like(q);
  const float scale = 1.0f / std::sqrt((float)a.D);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((unsigned)a.col_tiles, (unsigned)a.n, (unsigned)a.Hk);

#define LAUNCH(DD)                                                          \
  hipLaunchKernelGGL((rgqa::prefill_fp8::ragged_prefill_gqa_fp8_kernel<     \
                         DD>),                                              \
                     grid, dim3(256), 0, stream.stream(),                   \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const unsigned char*>(                \
                         kpool.data_ptr()),                                 \
                     reinterpret_cast<const unsigned char*>(                \
                         vpool.data_ptr()),                                 \
                     k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),  \
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
