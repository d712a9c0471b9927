// MFMA split-KV decode attention over the fp8 KV slot pool for MI355X
// (gfx950): any GQA group up to 32 and an optional sliding window.
//
// The fp8-pool variant of ragged_decode_gqa (ragged_decode_gqa.hip), whose
// semantics, grid, work split and key range [start, end) are this kernel's;
// pool format in kv_fp8.h: codes [B,Smax,Hk,D] e4m3fn plus one fp32 scale per
// (slot, position, kv head). The tile engine, its fp8 arithmetic (MFMAs on the
// codes, k_scale on the score, v_scale on P) and the combine kernel are
// ragged_gqa.h; this unit is the staging of codes and scales.
//
// Data movement. A K or V row is D code bytes: a 32-key tile is 32*D/16
// 16-byte pieces per pool, NL = D/32 per lane (4 at D 128, 2 at D 64), half
// the bf16 kernel's. Consecutive lanes take consecutive 16 bytes of a pool row
// (8 lanes a row at D 128: 64 lanes = 8 rows). A piece stays in registers AS
// CODES until its tile's turn, then is widened (kvfp8::widen8, twice) into two
// 16-byte stores of the wave's own bf16 image: every LDS read and MFMA is the
// bf16 kernel's. Codes take half the registers of bf16 rows, so a wave keeps
// TWO tiles ahead: stage A holds tile t, stage B tile t+4; after tile t's
// registers went to LDS, stage A is reloaded with tile t+8, which flies under
// the compute of tiles t and t+4. Bytes in flight per wave: 2 tiles x 2 pools
// x 32 x D = the bf16 kernel's one tile of 2-byte rows.
//
// Scales: a tile needs 32 k_scale and 32 v_scale values, strided by Hk floats.
// One lane per value (lanes 0..31 K, 32..63 V), loaded and prefetched with the
// tile's codes (one register per stage), staged in the wave's 64-float LDS
// array and read back by rgqa::TileScales. K rows and both scales past the
// split's end are loaded from its last row (clamped index); the staged V rows
// and scales past it are zeros.
//
// Resources (the compiler's report for gfx950, built without packed fp32):
//   LDS per workgroup  4 waves x (2 images x 32 x 2D + 256 bytes of scales):
//                      66560 bytes at D 128, 33792 at D 64.
//   registers          238 at D 128, 154 at D 64; no AGPRs, ZERO scratch.
//   resident per CU    2 workgroups at D 128 (registers, launch bound; LDS
//                      130 of 160 KiB), 3 at D 64 (registers; LDS would
//                      allow 4).
//   in flight per CU   2 tiles x (2 x 32 x D + 256) bytes per wave: 33 KiB at
//                      D 128 (8 waves), 25.5 KiB at D 64 (12 waves); the bf16
//                      kernel's 32 / 24 KiB plus the scales.
// The images' lane addresses are one register each (see the kernel): as loop
// invariants per piece, slice and d-tile they cost 20 registers more and the
// D 128 build spilled.
#include <torch/extension.h>

#include "kv_fp8.h"
#include "ragged_gqa.h"

namespace rgqa::decode_fp8 {

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
// repeats row end-1 (end > kb >= 0: always a row of the range).
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

// q [n,Hq,D] bf16, kpool/vpool [B,Smax,Hk,D] e4m3fn bytes, kscale/vscale
// [B,Smax,Hk] f32, rows/lens [n] i64.
// NS > 1: partial_out [n,Hq,NS,D] f32, partial_ml [n,Hq,NS,2] f32.
// NS == 1: out [n,Hq,D] bf16.
template <int D>
__launch_bounds__(256, 2)
__global__ void ragged_decode_gqa_fp8_kernel(
    const short* __restrict__ q, const unsigned char* __restrict__ kpool,
    const unsigned char* __restrict__ vpool, const float* __restrict__ kscale,
    const float* __restrict__ vscale, const int64_t* __restrict__ rows,
    const int64_t* __restrict__ lens, float* __restrict__ partial_out,
    float* __restrict__ partial_ml, short* __restrict__ out, int Hq, int Hk,
    int G, int B, int Smax, int NS, int window, float scale) {
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

  const long long kvrs = (long long)Hk * D;  // bytes per position
  const unsigned char* kp = kpool + (slot * Smax) * kvrs + hk * D;
  const unsigned char* vp = vpool + (slot * Smax) * kvrs + hk * D;
  // this lane's scale column: k_scale for the lower half, v_scale above
  const float* scp = (hi ? vscale : kscale) + (slot * Smax) * Hk + hk;

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

  // this wave's images, its staged scales and its lane's read addresses
  char* kimg = smem + wave * 2 * Smem<D>::IMG;
  char* vimg = kimg + Smem<D>::IMG;
  float* scl = reinterpret_cast<float*>(smem + Smem<D>::MAIN +
                                        wave * Smem<D>::SC);  // k[32], v[32]
  // Lane addresses into the images, one register each; the others differ by
  // constants, because every XOR of flash_fwd_layout.h moves bits that the
  // constants below own (rows a multiple of 4 apart share v_xor, k_xor of
  // row0 + j*RJ is k_xor(row0) ^ k_xor(j*RJ)):
  //   K piece (j, half h) at (kst0 ^ (16h ^ k_xor(j*RJ))) + j*RJ*RB
  //   V piece (j, half h) at vst0 + j*RJ*RB + 16h
  //   K row read of slice ks at krd0 ^ 32ks, V^T base of d-tile mt at
  //   vtr0 ^ 64mt.
  // tile() hides them from the optimiser once per tile: hoisted out of the
  // loop as 8 + 8 + NQF + NOT loop invariants they spill.
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

    // ---- S^T = K Q^T: rows key = kb + (r&3)+8*(r>>2)+4*hi, col = head ------
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

    // ---- online softmax; keys at or past the split's end are masked --------
    softmax_step(st, m_run, l_run, ot, hi, sc2, [&](int r) {
      return kb + (r & 3) + 8 * (r >> 2) + 4 * hi < end;
    }, scales);

    bf16x8_t pfrag[2];
    build_p(pfrag, st);
    pv_accumulate<D>(ot, vf, pfrag,
                     [&](int mt) { return vtr0 ^ (64 * mt); });
  };

  // Two stages: A holds the wave's tiles 0, 2, 4, ..., B its tiles 1, 3, ...
  // Every load of the pair loop is UNCONDITIONAL: the compiler's s_waitcnt
  // vmcnt counts are then exact (A's pieces wait with all of B's loads still
  // in flight), where a load under `if (more tiles)` makes it assume the
  // fewest loads any path issued and wait for both stages. A tile past the
  // split's end is load_tile's clamp: one row, end-1, again and again.
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

  if (l31 >= G) return;  // columns past the group hold no head
  const long long head = head0 + l31;
  if (NS == 1)
    store_row(out + head * D, ot, l_run, hi);
  else
    store_partial(partial_out, partial_ml, head * NS + s, ot, m_run, l_run,
                  hi);
}

}  // namespace rgqa::decode_fp8

at::Tensor ragged_decode_gqa_fp8(at::Tensor q, at::Tensor kpool,
                                 at::Tensor vpool, at::Tensor k_scale,
                                 at::Tensor v_scale, at::Tensor rows,
                                 at::Tensor lens, long window, long max_len,
                                 long splits) {
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
  const char* name = "ragged_decode_gqa_fp8";
  const rgqa::Shape a = rgqa::check_decode(name, q, kpool, vpool, &k_scale,
                                           &v_scale, rows, lens, window,
                                           max_len, splits);
  const long NS = rgqa::plan_splits(name, a, lens, window, max_len, splits);
  const rgqa::DecodeOut o = rgqa::alloc_decode(q, a, NS);
  const float scale = 1.0f / std::sqrt((float)a.D);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((unsigned)a.n, (unsigned)a.Hk, (unsigned)NS);

#define LAUNCH(DD)                                                           \
  hipLaunchKernelGGL((rgqa::decode_fp8::ragged_decode_gqa_fp8_kernel<DD>),   \
                     grid, dim3(256), 0, stream.stream(),                    \
                     reinterpret_cast<const short*>(q.data_ptr()),           \
                     reinterpret_cast<const unsigned char*>(                 \
                         kpool.data_ptr()),                                  \
                     reinterpret_cast<const unsigned char*>(                 \
                         vpool.data_ptr()),                                  \
                     k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),   \
                     rows.data_ptr<int64_t>(), lens.data_ptr<int64_t>(),     \
                     o.pout_ptr(), o.pml_ptr(),                              \
                     reinterpret_cast<short*>(o.out.data_ptr()), (int)a.Hq,  \
                     (int)a.Hk, (int)a.G, (int)a.B, (int)a.Smax, (int)NS,    \
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
