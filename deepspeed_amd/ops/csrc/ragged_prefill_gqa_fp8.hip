// MFMA ragged prefill attention over the fp8 KV slot pool for MI355X (gfx950):
// the fused serving step for any GQA group up to 32 and an optional sliding
// window, over e4m3 codes.
//
// The join of two kernels of this directory. The semantics, the grid, the
// (token, head) column tiling, the per-column band, the wave merge and the
// epilogue are ragged_prefill_gqa.hip's; the pool format (kv_fp8.h), the
// arithmetic, the code staging and the scales are ragged_decode_gqa_fp8.hip's.
// ragged_prefill_fp8.hip gives a workgroup (32 tokens, one Q HEAD), fetches
// every K and V row once per q head, transposes V by hand, serves G in
// {1, 2, 4, 8} and has no window.
//
// Contract: q [T,Hq,D] bf16, code pools [B,Smax,Hk,D] e4m3fn, scales
// [B,Smax,Hk] fp32, desc [n,4] i64 rows (slot, q_start, q_len, kv_len), out
// [T,Hq,D] bf16. Local token j of a sequence lives at q[q_start + j], has
// position p = kv_len - q_len + j and attends pool positions [lo, p] of its
// slot, lo = max(0, p - window + 1) under a window, else 0.
//
// Work split. Column c of a sequence runs over [0, q_len * G): token c / G,
// head c % G, which is q head hk*G + c % G. Grid (ceil(max_qlen * G / 32), n,
// Hk), one workgroup of 4 waves per tile of 32 consecutive columns of one
// (sequence, kv head); the tile index is rotated by the sequence, so the one
// tile of every decode row does not meet on one XCD. Every lane derives its
// own token, head and p and its own q and out row; columns at or past
// q_len * G are pad lanes (p = -1): they see no key and write nothing.
// Workgroup key range [start, end): end = p(last valid token) + 1, start =
// lo(first token) under a window, else 0. Tiles of 32 keys run from `start`,
// unaligned; wave w takes tiles w, w+4, ...
//
// Arithmetic (the fp8 contract of ragged_prefill_fp8.hip): every e4m3 code is
// exactly a bf16, so the MFMAs are the bf16 32x32x16 ones run on the CODES.
//   S^T = K Q^T      A = the tile's K codes widened to bf16, B = Q^T (bf16,
//                    not quantised), C column = lane & 31 = the lane's column.
//   score            = S^T * k_scale[key] * softmax_scale, masked by select.
//   row sum          of p, unscaled.
//   P                = bf16(p * v_scale[key]).
//   O^T += V^T P^T   V^T fragments of the widened V codes by
//                    ds_read_b64_tr_b16 from a ROW-MAJOR image, one d-tile
//                    ahead of the MFMAs.
//
// Data movement. Codes move as 16-byte pieces, NL = D/32 per lane per pool,
// and stay in registers AS CODES, two tiles ahead at both head dims: stage A
// holds the wave's tile t, stage B tile t+4; after tile t's registers went to
// LDS (kvfp8::widen8 into the wave's bf16 K and V images, the swizzles of
// flash_fwd_layout.h) stage A is reloaded with tile t+8. One scale per lane
// per stage (lanes 0..31 k_scale, 32..63 v_scale of key kb + lane&31), staged
// in the wave's 64-float LDS array and read back as float4 broadcasts. Images
// and scales are private to a wave and a wave's LDS operations complete in
// order: the tile loop has no barrier. The 4 waves' (m, l, O) are merged lane
// for lane over the image space; the epilogue normalises and writes bf16, 8
// bytes per store, to the lane's own (token, head) row.
//
// Masking is by SELECT, scales included: lo_c <= key <= p_c, else the score is
// -inf and P is exactly 0, never a product with a scale. Nothing outside
// [start, end) is loaded: K rows and scales past `end` come from row end-1
// (clamped index), the staged V rows and both scales past it are zeros. So NaN
// codes and NaN / inf scales below the band, past kv_len or in other slots
// cannot reach a live value. A lane may see no key in a whole tile or in a
// wave's whole share (a pad lane, a column whose band another wave holds): the
// m == -inf guards cover it, in the tile loop and in the merge.
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
//                      66560 bytes at D 128, 33792 at D 64; the merge reuses
//                      the images (49.5 / 25.5 KiB).
//   registers          250 at D 128, 165 at D 64 (ragged_decode_gqa_fp8: 238 /
//                      154); no AGPRs, ZERO scratch, two stages at both.
//   resident per CU    2 workgroups at D 128 (registers, launch bound; LDS
//                      130 of 160 KiB), 3 at D 64 (registers; LDS would
//                      allow 4).
#include <torch/extension.h>

#include <algorithm>

#include "flash_fwd_layout.h"
#include "kv_fp8.h"
#include "lds_tr_read.h"

namespace rpgqa8 {

using kvfp8::bf16x8_t;
using f32x16_t = __attribute__((ext_vector_type(16))) float;
using f32x4_t = __attribute__((ext_vector_type(4))) float;
using u32x4_t = __attribute__((ext_vector_type(4))) unsigned int;
#define RP8_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16

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
  static constexpr int MAIN = NW * 2 * IMG > MERGE ? NW * 2 * IMG : MERGE;
  static constexpr int SC = 2 * KT * 4;             // a wave's staged scales
  static constexpr int BYTES = MAIN + NW * SC;
};

// the wave's share of one tile of codes: NL 16-byte pieces per lane, piece j
// of lane `lane` is code bytes cb .. cb+15 of tile row `row`
template <int D>
struct Piece {
  static constexpr int PPR = D / 16;  // pieces per row
  static constexpr int NL = KT * PPR / 64;
  static constexpr int RJ = 64 / PPR;  // piece j is RJ rows below piece j-1
  DEV_INLINE static int row(int j, int lane) { return (j * 64 + lane) / PPR; }
  DEV_INLINE static int cb(int j, int lane) {
    return ((j * 64 + lane) % PPR) * 16;
  }
};

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

// the 2 k-slices x 2 halves of V's operand for one d-tile (4 reads)
template <int D>
DEV_INLINE void issue_v_dtile(tr_frag (&f)[2], unsigned base) {
  using namespace fwd_layout;
  f[0] = issue_tr_read_off<v_tr_step<D>(0, 0), v_tr_step<D>(0, 1)>(base);
  f[1] = issue_tr_read_off<v_tr_step<D>(1, 0), v_tr_step<D>(1, 1)>(base);
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

  // ---- Q^T: qfrag[ks] = Q[token, head of column l31][16*ks + hi*8 .. +7],
  // 0 in pad columns ----------------------------------------------------------
  bf16x8_t qfrag[NQF];
#pragma unroll
  for (int ks = 0; ks < NQF; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) qfrag[ks][j] = 0;
  if (l31 < n_valid) {
    const short* src =
        q + column_row(q_start, j_first, g_first, l31, G, Hq, hk, D) + hi * 8;
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
      st = RP8_MFMA(kf, qfrag[ks], st, 0, 0, 0);
    }
    // the 16 k scales of this lane's score rows
    f32x4_t ksc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      ksc[g] = *reinterpret_cast<const f32x4_t*>(scl + 8 * g + 4 * hi);

    // V's operand for d-tile 0: the transposed reads fly under the softmax
    tr_frag vf[2][2];
    issue_v_dtile<D>(vf[0], vtr0);

    // ---- k_scale, online softmax, lane-local column; masked by select ------
    // band of this lane's column relative to its first score row: row offset
    // o = (r&3) + 8*(r>>2) is visible iff dlo < o <= dhi. my_p < end, so a
    // key the range clamped or zeroed is hidden as well.
    const int dhi = my_p - kb - 4 * hi;
    const int dlo = window > 0 ? dhi - window : -1;  // o >= 0
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = (r & 3) + 8 * (r >> 2);
      const float sv = (o <= dhi && o > dlo)
                           ? st[r] * ksc[r >> 2][r & 3] * sc2
                           : -INFINITY;
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
    // the 16 v scales, once the k scales are dead
    f32x4_t vsc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      vsc[g] = *reinterpret_cast<const f32x4_t*>(scl + KT + 8 * g + 4 * hi);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float sv = st[r];
      float p = 0.f, pv = 0.f;
      if (sv != -INFINITY) {
        p = __builtin_amdgcn_exp2f(sv - m_sub);
        pv = p * vsc[r >> 2][r & 3];
      }
      psum += p;   // the row sum stays unscaled
      st[r] = pv;  // P * v_scale goes into the PV MFMA
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
        issue_v_dtile<D>(vf[(mt + 1) & 1], vtr0 ^ (64 * (mt + 1)));
        tr_wait<4>(vf[mt & 1][0], vf[mt & 1][1]);
      } else {
        tr_wait<0>(vf[mt & 1][0], vf[mt & 1][1]);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        ot[mt] = RP8_MFMA(tr_operand(vf[mt & 1][ks]), pfrag[ks], ot[mt], 0, 0,
                          0);
    }
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

  // the lane's column again, from a copy of l31 the optimiser cannot tie to
  // the one above: the row offset then costs no registers in the tile loop
  int l31e = l31;
  asm volatile("" : "+v"(l31e));
  if (l31e >= n_valid) return;  // pad columns hold no (token, head)
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
  short* dst =
      out + column_row(q_start, j_first, g_first, l31e, G, Hq, hk, D);
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

}  // namespace rpgqa8

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
  TORCH_CHECK(q.dim() == 3, "ragged_prefill_gqa_fp8: q must be [T,Hq,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(),
              "ragged_prefill_gqa_fp8: kpool and vpool must both be "
              "[B,Smax,Hk,D]");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 4,
              "ragged_prefill_gqa_fp8: desc must be [n,4] "
              "(slot, q_start, q_len, kv_len)");
  const long T = q.size(0), Hq = q.size(1), D = q.size(2);
  const long B = kpool.size(0), Smax = kpool.size(1), Hk = kpool.size(2);
  const long n = desc.size(0);
  TORCH_CHECK(n >= 1 && T >= 1, "ragged_prefill_gqa_fp8: empty batch");
  TORCH_CHECK(B >= 1 && Hk >= 1 && kpool.size(3) == D,
              "ragged_prefill_gqa_fp8: empty pool or pool head_dim != q "
              "head_dim");
  TORCH_CHECK(k_scale.dim() == 3 && k_scale.size(0) == B &&
                  k_scale.size(1) == Smax && k_scale.size(2) == Hk &&
                  v_scale.sizes() == k_scale.sizes(),
              "ragged_prefill_gqa_fp8: k_scale and v_scale must both be "
              "[B,Smax,Hk]");
  TORCH_CHECK(D == 128 || D == 64,
              "ragged_prefill_gqa_fp8: head_dim must be 64 or 128");
  TORCH_CHECK(Hq >= 1 && Hq % Hk == 0,
              "ragged_prefill_gqa_fp8: Hq % Hk != 0");
  const long G = Hq / Hk;
  TORCH_CHECK(G <= rpgqa8::MAXG, "ragged_prefill_gqa_fp8: GQA group ", G,
              " exceeds ", rpgqa8::MAXG);
  TORCH_CHECK(window >= 0,
              "ragged_prefill_gqa_fp8: window must be >= 0, got ", window);
  TORCH_CHECK(1 <= max_qlen && max_qlen <= max_kvlen && max_kvlen <= Smax,
              "ragged_prefill_gqa_fp8: need 1 <= max_qlen <= max_kvlen <= "
              "Smax, got ", max_qlen, ", ", max_kvlen, ", ", Smax);
  TORCH_CHECK(Smax <= 0x7fffffffL && T <= 0x7fffffffL,
              "ragged_prefill_gqa_fp8: Smax or T exceeds 2^31 - 1");
  const long col_tiles = (max_qlen * G + rpgqa8::CT - 1) / rpgqa8::CT;
  TORCH_CHECK(col_tiles <= 0x7fffffffL,
              "ragged_prefill_gqa_fp8: more than 2^31 - 1 column tiles");
  TORCH_CHECK(n <= 65535 && Hk <= 65535,
              "ragged_prefill_gqa_fp8: more than 65535 sequences or kv "
              "heads");
  TORCH_CHECK(ptr_aligned(q.data_ptr(), 16) &&
                  ptr_aligned(kpool.data_ptr(), 16) &&
                  ptr_aligned(vpool.data_ptr(), 16),
              "ragged_prefill_gqa_fp8: q and the code pools must be 16-byte "
              "aligned");

  auto out = at::empty_like(q);
  const float scale = 1.0f / std::sqrt((float)D);
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((unsigned)col_tiles, (unsigned)n, (unsigned)Hk);

#define LAUNCH(DD)                                                          \
  hipLaunchKernelGGL((rpgqa8::ragged_prefill_gqa_fp8_kernel<DD>), grid,     \
                     dim3(256), 0, stream.stream(),                         \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const unsigned char*>(                \
                         kpool.data_ptr()),                                 \
                     reinterpret_cast<const unsigned char*>(                \
                         vpool.data_ptr()),                                 \
                     k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),  \
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
