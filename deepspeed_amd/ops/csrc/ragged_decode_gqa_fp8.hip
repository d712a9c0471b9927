// MFMA split-KV decode attention over the fp8 KV slot pool for MI355X
// (gfx950): any GQA group up to 32 and an optional sliding window.
//
// The fp8-pool variant of ragged_decode_gqa (ragged_decode_gqa.hip); pool
// format in kv_fp8.h: codes [B,Smax,Hk,D] e4m3fn plus one fp32 scale per
// (slot, position, kv head). Semantics, grid, work split, MFMA roles, the
// lane-local softmax, the wave merge and the split partials are that kernel's:
//
// Row i attends pool positions [lo_i, len_i) of slot rows[i], len_i clamped
// into [0, Smax], lo_i = max(0, len_i - window) under a window, else 0. Grid
// (n, Hk, NS), one workgroup of 4 waves per (row, kv head, split); split s
// covers [lo + s*per, lo + (s+1)*per) cut at len, per = ceil((len - lo) / NS)
// rounded up to whole 32-key tiles; wave w takes the split's tiles w, w+4, ...
//
// Arithmetic (the fp8 contract of ragged_prefill_fp8.hip): every e4m3 code is
// exactly a bf16, so the MFMAs are the bf16 ones run on the CODES.
//   S^T = K Q^T      A = the tile's K codes widened to bf16, B = Q^T (bf16,
//                    not quantised), column c < G the query head hk*G + c.
//   score            = S^T * k_scale[key] * softmax_scale, masked by select.
//   row sum          of p, unscaled.
//   P                = bf16(p * v_scale[key]): the one fp32 rounding on the PV
//                    side beyond the bf16 kernel's.
//   O^T += V^T P^T   V^T fragments of the widened V codes by
//                    ds_read_b64_tr_b16 from a ROW-MAJOR image.
//
// Data movement, the part that is new. A K or V row is D code bytes: a 32-key
// tile is 32*D/16 16-byte pieces per pool, NL = D/32 per lane (4 at D 128, 2
// at D 64), half the bf16 kernel's. Consecutive lanes take consecutive 16
// bytes of a pool row (8 lanes a row at D 128: 64 lanes = 8 rows). A piece
// stays in registers AS CODES until its tile's turn, then is widened
// (kvfp8::widen8, twice) into two 16-byte stores of the wave's own bf16 image
// [32][D] (the swizzles of flash_fwd_layout.h): every LDS read and MFMA is the
// bf16 kernel's. Codes take half the registers of bf16 rows, so a wave keeps
// TWO tiles ahead: stage A holds tile t, stage B tile t+4; after tile t's
// registers went to LDS, stage A is reloaded with tile t+8, which flies under
// the compute of tiles t and t+4. Bytes in flight per wave: 2 tiles x 2 pools
// x 32 x D = the bf16 kernel's one tile of 2-byte rows.
//
// Scales: a tile needs 32 k_scale and 32 v_scale values, strided by Hk floats.
// One lane per value (lanes 0..31 K, 32..63 V), loaded and prefetched with the
// tile's codes (one register per stage), staged in the wave's 64-float LDS
// array; each lane then reads the 16 + 16 its score registers need, key =
// kb + (r&3) + 8*(r>>2) + 4*hi, as four float4 each (the 32 lanes of a half
// read one address: a broadcast).
//
// The images and the scale array are private to a wave and a wave's LDS
// operations complete in order, so the tile loop has no barrier.
//
// Masking is by SELECT, scales included: a key outside [start, end) scores
// -inf and its P is exactly 0, never a product with a scale. K rows and both
// scales past the split's end are loaded from its last row (clamped index);
// the staged V rows and scales past it are zeros. Nothing outside [lo, len)
// is loaded, so NaN codes and NaN / inf scales there cannot reach the output.
//
// Resources (the compiler's report for gfx950, built without packed fp32):
//   LDS per workgroup  4 waves x (2 images x 32 x 2D + 256 bytes of scales):
//                      66560 bytes at D 128, 33792 at D 64; the merge of the
//                      4 waves' (m, l, O) reuses the images (49.5 / 25.5 KiB).
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
//
// NS > 1: fp32 partials [n,Hq,NS,D] (unnormalised O) and [n,Hq,NS,2] (m in the
// exp2 domain, l), merged by the combine kernel below (the arithmetic of
// ragged_decode_gqa's). NS == 1: the kernel normalises and writes bf16 itself.
#include <torch/extension.h>

#include <algorithm>

#include "flash_fwd_layout.h"
#include "kv_fp8.h"
#include "lds_tr_read.h"

namespace rdgqa8 {

using kvfp8::bf16x8_t;
using f32x16_t = __attribute__((ext_vector_type(16))) float;
using f32x4_t = __attribute__((ext_vector_type(4))) float;
using u32x4_t = __attribute__((ext_vector_type(4))) unsigned int;
#define RG8_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16

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

// the 2 k-slices x 2 halves of V's operand for one d-tile (4 reads)
template <int D>
DEV_INLINE void issue_v_dtile(tr_frag (&f)[2], unsigned base) {
  using namespace fwd_layout;
  f[0] = issue_tr_read_off<v_tr_step<D>(0, 0), v_tr_step<D>(0, 1)>(base);
  f[1] = issue_tr_read_off<v_tr_step<D>(1, 0), v_tr_step<D>(1, 1)>(base);
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
      st = RG8_MFMA(kf, qfrag[ks], st, 0, 0, 0);
    }
    // the 16 k scales of this lane's score rows
    f32x4_t ksc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      ksc[g] = *reinterpret_cast<const f32x4_t*>(scl + 8 * g + 4 * hi);

    // V's operand for d-tile 0: the transposed reads fly under the softmax
    tr_frag vf[2][2];
    issue_v_dtile<D>(vf[0], vtr0);

    // ---- k_scale, online softmax, lane-local head; masked by select --------
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kb + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const float sv =
          key < end ? st[r] * ksc[r >> 2][r & 3] * sc2 : -INFINITY;
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
        ot[mt] = RG8_MFMA(tr_operand(vf[mt & 1][ks]), pfrag[ks], ot[mt], 0, 0,
                          0);
    }
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

// merge the NS split partials -> out [n,Hq,D] bf16; one wave per (row, head).
// The arithmetic of ragged_decode_gqa's combine kernel.
template <int D>
__global__ void ragged_decode_gqa_fp8_combine_kernel(
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

}  // namespace rdgqa8

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
  TORCH_CHECK((q.dim() == 4 && q.size(1) == 1) || q.dim() == 3,
              "ragged_decode_gqa_fp8: q must be [n,1,Hq,D] or [n,Hq,D]");
  TORCH_CHECK(kpool.dim() == 4 && vpool.sizes() == kpool.sizes(),
              "ragged_decode_gqa_fp8: kpool and vpool must both be "
              "[B,Smax,Hk,D]");
  const long n = q.size(0), Hq = q.size(-2), D = q.size(-1);
  const long B = kpool.size(0), Smax = kpool.size(1), Hk = kpool.size(2);
  TORCH_CHECK(n >= 1 && B >= 1 && Smax >= 1 && Hk >= 1 && kpool.size(3) == D,
              "ragged_decode_gqa_fp8: empty batch or pool, or pool head_dim "
              "!= q head_dim");
  TORCH_CHECK(k_scale.dim() == 3 && k_scale.size(0) == B &&
                  k_scale.size(1) == Smax && k_scale.size(2) == Hk &&
                  v_scale.sizes() == k_scale.sizes(),
              "ragged_decode_gqa_fp8: k_scale and v_scale must both be "
              "[B,Smax,Hk]");
  TORCH_CHECK(rows.numel() == n && lens.numel() == n,
              "ragged_decode_gqa_fp8: rows and lens must have one entry per "
              "q row");
  TORCH_CHECK(D == 128 || D == 64,
              "ragged_decode_gqa_fp8: head_dim must be 64 or 128");
  TORCH_CHECK(Hq >= 1 && Hq % Hk == 0,
              "ragged_decode_gqa_fp8: Hq % Hk != 0");
  const long G = Hq / Hk;
  TORCH_CHECK(G <= rdgqa8::MAXG, "ragged_decode_gqa_fp8: GQA group ", G,
              " exceeds ", rdgqa8::MAXG);
  TORCH_CHECK(window >= 0,
              "ragged_decode_gqa_fp8: window must be >= 0, got ", window);
  TORCH_CHECK(0 <= max_len && max_len <= Smax,
              "ragged_decode_gqa_fp8: need 0 <= max_len <= Smax, got ",
              max_len, ", ", Smax);
  TORCH_CHECK(0 <= splits && splits <= rdgqa8::MAX_SPLITS,
              "ragged_decode_gqa_fp8: need 0 <= splits <= ",
              rdgqa8::MAX_SPLITS);
  TORCH_CHECK(Hk <= 65535, "ragged_decode_gqa_fp8: more than 65535 kv heads");
  TORCH_CHECK(ptr_aligned(q.data_ptr(), 16) &&
                  ptr_aligned(kpool.data_ptr(), 16) &&
                  ptr_aligned(vpool.data_ptr(), 16),
              "ragged_decode_gqa_fp8: q and the code pools must be 16-byte "
              "aligned");

  if (max_len == 0) {  // the one host read; callers that know a bound skip it
    max_len = lens.max().item<long>();
    TORCH_CHECK(max_len <= Smax, "ragged_decode_gqa_fp8: lens.max() = ",
                max_len, " exceeds the pool's Smax = ", Smax);
    max_len = std::max<long>(max_len, 1);
  }
  // about two workgroups per CU, no split shorter than one tile per wave
  long NS = splits;
  if (NS == 0) {
    const long span = window > 0 ? std::min(max_len, window) : max_len;
    const long longest = std::max<long>(span / (rdgqa8::KT * rdgqa8::NW), 1);
    const long want = (2 * rdgqa8::device_cus() + n * Hk - 1) / (n * Hk);
    NS = std::min<long>(std::min(want, longest), rdgqa8::MAX_SPLITS);
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
  hipLaunchKernelGGL((rdgqa8::ragged_decode_gqa_fp8_kernel<DD>), grid,      \
                     dim3(256), 0, stream.stream(),                         \
                     reinterpret_cast<const short*>(q.data_ptr()),          \
                     reinterpret_cast<const unsigned char*>(                \
                         kpool.data_ptr()),                                 \
                     reinterpret_cast<const unsigned char*>(                \
                         vpool.data_ptr()),                                 \
                     k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),  \
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
#define COMBINE(DD)                                                          \
  hipLaunchKernelGGL(rdgqa8::ragged_decode_gqa_fp8_combine_kernel<DD>,       \
                     gridc, dim3(256), 0, stream.stream(),                   \
                     pout.data_ptr<float>(), pml.data_ptr<float>(),          \
                     reinterpret_cast<short*>(out.data_ptr()), nhq, (int)NS)
  if (D == 128)
    COMBINE(128);
  else
    COMBINE(64);
#undef COMBINE
  HIP_CHECK_KERNEL();
  return out;
}
