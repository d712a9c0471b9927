// Flash attention BACKWARD for MI355X (gfx950) — hand-written MFMA kernels.
//
// Exact flash backward (recompute P from saved LSE), two passes:
//   pass 1 (kv-outer): dV = P^T dO ; dK = dS^T Q    — no atomics
//   pass 2 (q-outer):  dQ = dS K                     — no atomics
// with dS = P o (dP - Drow) * scale, dP = dO V^T, P = exp(S*scale - lse).
//
// Pre-pass (bwd_preprocess, once per call): Drow = rowsum(dO o O) and a
// copy of lse (with -inf -> +inf, so exp(s - lse) = 0 on rows that have no
// admissible column), both [B,Hq,Sp]. Sp is S padded to a multiple of 128 and
// the pad is written as zeros, so every read of them is in bounds. They are
// the only scratch: no transposed copy of Q, dO or K exists.
//
// Both passes have the same shape: a workgroup of 4 waves owns a block of
// its outer index (pass 1: 4 waves x 16 keys = 64 keys, three workgroups
// resident per CU at D 128; pass 2: 4 waves x 32 q rows = 128, two resident)
// and streams the other index in steps of 32. Several independent workgroups
// per CU are what hides a workgroup's load wait and barrier.
//   - the first two products put the OUTER index on the MFMA lane
//     (pass 1: S = Q K^T, dP = dO V^T with the key on the lane; pass 2:
//     S^T = K Q^T, dP^T = V dO^T with the q row on the lane). A pair of
//     16x16 accumulator tiles, rounded to bf16, is then already the B operand
//     of the second products (dV^T += dO^T P, dK^T += Q^T dS; dQ^T += K^T
//     dS^T): P and dS never cross LDS. The A operand of those products comes
//     from the SAME row-major image as the first products' (Q, dO; K), read
//     transposed in hardware with the matching k order (element j of lane
//     group l4 is row 4*l4 + j for j < 4 and 16 + 4*l4 + j - 4 above): two
//     ds_read_b64_tr_b16, issued one d-tile ahead of their MFMAs.
//   - each step's images (pass 1: Q, dO and the step's lse / Drow; pass 2:
//     K, V), one per tile, arrive by global_load_lds into a double buffer;
//     step t+1 is issued before step t's MFMAs, one barrier per step. Rows
//     past S-1 of an image repeat row S-1; the predicate zeroes their P, dS.
//     (A three-deep ring with counted vmcnt waits was measured slower in
//     pass 1: profiles/README.md.)
//   - -Drow is the initial accumulator of dP.
//   - steps with nothing to mask (all rows in range, below the causal
//     diagonal, no kv mask) skip the predicate; steps fully above the
//     diagonal skip the math.
//   - pass 2 launches the causal-heaviest q blocks first. Pass 1 is a 1-D
//     grid whose workgroup id is mapped to (key block, b * Hk + kv head) by
//     flash_bwd_wgmap.h: the key blocks of one (b, kv head), which all
//     stream the same Q / dO, get ids of one residue mod 8 and so share an
//     XCD and its L2, heaviest first; every XCD gets the same work.
// Results are written transposed from the accumulators: 4 consecutive d per
// lane, one 8-byte store.
//
// Layout conventions follow the forward kernel (attention.hip): C/D layout
// row=(lane>>4)*4+reg, col=lane&15; A-operand lane holds A[l15][l4*8+j];
// the LDS image layout (32-byte pair XOR, conflict-free for both kinds of
// read, pre-swizzled DMA sources) is in flash_bwd_layout.h.
// GQA: pass 1 accumulates over the q-head group in-kernel (K/V fragments
// stay in registers across the group), writing dK/dV at [B,S,Hk,D]
// directly — no per-q-head buffers, no wrapper reduction.
#include <torch/extension.h>

#include "common.h"
#include "flash_bwd_layout.h"
#include "flash_bwd_wgmap.h"
#include "lds_tr_read.h"

using bf16x8_t = __attribute__((ext_vector_type(8))) short;
using f32x4_t = __attribute__((ext_vector_type(4))) float;
using u32x4_t = __attribute__((ext_vector_type(4))) unsigned int;
using u32x2_t = __attribute__((ext_vector_type(2))) unsigned int;

#define MFMA_BF16_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_bf16

namespace bwd {

constexpr int BR = 128;   // q rows per workgroup, pass 2; padding of Sp
constexpr int WR = 32;    // q rows per wave, pass 2 (4 waves)
// 16-key tiles per wave, pass 1. 2 needs 128 + 64 registers for dK^T, dV^T
// and the K/V fragments alone: at D 128 it spills under a 256-register budget
// and was slower at one wave per SIMD than 1 at two.
constexpr int KTW1 = 1;
// Waves per workgroup, pass 1: 4 waves = 64 keys, so that three (D 128: 161
// registers, 33 KB of LDS each) or four (D 64) independent workgroups share a
// CU and one's load wait and barrier run under the others' MFMAs. 8 waves
// (one workgroup per CU) and 2 (178 + 64 registers at D 128: two waves per
// SIMD, not three) were measured slower: profiles/README.md.
constexpr int NW1 = 4;
constexpr int BRK1 = 16 * KTW1 * NW1;  // keys per workgroup, pass 1
static_assert(BR % BRK1 == 0, "Sp covers every pass 1 workgroup's q steps");
constexpr int TS = 32;    // streamed rows per step
static_assert(TS == bwd_layout::TS, "the image layout is for 32-row steps");
constexpr int PT = 64;    // rows per pre-pass tile

// two f32 -> one u32 of 2 bf16, RNE (v_cvt_pk_bf16_f32)
DEV_INLINE unsigned int cvtpk2(float lo, float hi) {
  unsigned short a = __builtin_bit_cast(unsigned short, (__bf16)lo);
  unsigned short b = __builtin_bit_cast(unsigned short, (__bf16)hi);
  return (unsigned int)a | ((unsigned int)b << 16);
}

// ---------------------------------------------------------------------------
// PRE-PASS. grid (Sp/64, B*Hq): Drow = rowsum(dO o O) and the copy of lse,
// both padded to Sp (Drow 0, lse 0 past S-1). 16-byte pieces, DH/8 lanes per
// row.
// ---------------------------------------------------------------------------
template <int DH>
__launch_bounds__(256)
__global__ void bwd_preprocess(
    const short* __restrict__ dout, const short* __restrict__ out,
    const float* __restrict__ lse,  // [B,Hq,S]
    float* __restrict__ drowP, float* __restrict__ lseP,  // [B,Hq,Sp]
    int B, int S, int Sp, int Hq) {
  constexpr int PPR = DH / 8;  // 16-byte pieces per row
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int h = bh % Hq;
  const int s0 = blockIdx.x * PT;

  for (int i = threadIdx.x; i < PT * PPR; i += 256) {
    const int row = i / PPR;
    const int c = i % PPR;
    const int s = s0 + row;
    const long long off = (((long long)b * S + s) * Hq + h) * DH + c * 8;
    u32x4_t x = {0u, 0u, 0u, 0u};
    u32x4_t o = {0u, 0u, 0u, 0u};
    if (s < S) {
      x = *reinterpret_cast<const u32x4_t*>(dout + off);
      o = *reinterpret_cast<const u32x4_t*>(out + off);
    }
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      acc += bf2f((short)(x[w] & 0xffff)) * bf2f((short)(o[w] & 0xffff)) +
             bf2f((short)(x[w] >> 16)) * bf2f((short)(o[w] >> 16));
#pragma unroll
    for (int m = PPR / 2; m > 0; m >>= 1) acc += __shfl_xor(acc, m, WAVE);
    if (c == 0) {
      float l = 0.f;
      if (s < S) {
        l = lse[((long long)b * Hq + h) * S + s];
        // a row with no admissible column has lse = -inf: subtracting +inf
        // instead makes its P exp(-inf) = 0, not exp(-inf - -inf) = NaN
        if (l == -INFINITY) l = INFINITY;
      }
      drowP[((long long)b * Hq + h) * Sp + s] = acc;
      lseP[((long long)b * Hq + h) * Sp + s] = l;
    }
  }
}

// ---------------------------------------------------------------------------
// LDS images of one 32-row step: row-major [32][DH] in the layout of
// flash_bwd_layout.h, which serves the 16-byte row reads and the hardware
// transposed reads alike. An image is DH/16 wave-segments of 1024 B (64 lanes
// x 16 B, LDS-linear), so the XOR is applied to the per-lane SOURCE address.
// ---------------------------------------------------------------------------
DEV_INLINE void lds_dma16(const short* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      reinterpret_cast<const unsigned int*>(src),
      reinterpret_cast<unsigned int*>(lds_wave_base), 16, 0, 0);
}

// rows r0..r0+31 of a [*, rs] row-major tensor (rows past S-1 repeat S-1)
template <int DH>
DEV_INLINE void issue_rm(const short* base, long long rs, int r0, int S,
                         char* img, int sseg, int lane) {
  const int linear = sseg * 1024 + lane * 16;
  const int src_col = bwd_layout::dma_src_byte<DH>(linear);
  const int grow = r0 + bwd_layout::dma_row<DH>(linear);
  const int srow = grow < S ? grow : S - 1;
  lds_dma16(base + (long long)srow * rs + (src_col >> 1), img + sseg * 1024);
}

// A (or B) fragment, natural k order: T[row][32*ks + 8*l4 .. +7]
template <int DH>
DEV_INLINE bf16x8_t read_rm(const char* img, int row, int ks, int l4) {
  return *reinterpret_cast<const bf16x8_t*>(
      img + bwd_layout::img_off<DH>(row, (l4 * 8 + 32 * ks) * 2));
}

// A fragment in accumulator-pair k order, taken from the ROW-MAJOR image by
// two ds_read_b64_tr_b16: T^T[16*dt + l15][4*l4 .. +3, 16+4*l4 .. +3].
// The reads, their counted waits (tr_wait<N>) and tr_operand are in
// lds_tr_read.h, with the reasons they are inline assembly. They need EXEC
// all ones: wave-uniform control flow only.
template <int DH>
DEV_INLINE tr_frag issue_tr_read(unsigned img, int dt, int lane) {
  return ::issue_tr_read(img + bwd_layout::tr_read_addr<DH>(lane, dt, 0),
                       img + bwd_layout::tr_read_addr<DH>(lane, dt, 1));
}

// two accumulator tiles (rows 0..15 and 16..31 of the summed index) -> the
// B fragment of the next product
DEV_INLINE bf16x8_t pack_pair(const f32x4_t& a, const f32x4_t& b) {
  u32x4_t w = {cvtpk2(a[0], a[1]), cvtpk2(a[2], a[3]), cvtpk2(b[0], b[1]),
               cvtpk2(b[2], b[3])};
  return __builtin_bit_cast(bf16x8_t, w);
}

DEV_INLINE void store4(short* p, const f32x4_t& a) {
  u32x2_t w = {cvtpk2(a[0], a[1]), cvtpk2(a[2], a[3])};
  *reinterpret_cast<u32x2_t*>(p) = w;
}

// Inverse RoPE (rotate-half) on one row's gradient held as NDT d-tiles of 4:
// d = 16dt + 4*l4 .. +3 pairs with d + D/2, i.e. tile dt + NDT/2 of the same
// lane. cr/sr point at the row's cos/sin table entries [p, 4*l4]. fp32, before
// the single bf16 rounding in store4.
template <int NDT, int STRIDE>
DEV_INLINE void unrotate_row(f32x4_t* acc /* [NDT] tiles, STRIDE apart */,
                             const float* __restrict__ cr,
                             const float* __restrict__ sr) {
#pragma unroll
  for (int dt = 0; dt < NDT / 2; ++dt) {
    const f32x4_t c = *reinterpret_cast<const f32x4_t*>(cr + 16 * dt);
    const f32x4_t sn = *reinterpret_cast<const f32x4_t*>(sr + 16 * dt);
    const f32x4_t d1 = acc[dt * STRIDE];
    const f32x4_t d2 = acc[(dt + NDT / 2) * STRIDE];
    acc[dt * STRIDE] = d1 * c + d2 * sn;
    acc[(dt + NDT / 2) * STRIDE] = d2 * c - d1 * sn;
  }
}

// ---------------------------------------------------------------------------
// PASS 1: kv-outer. Block: NW waves x 16 * KTW keys = BRK keys; q steps of 32
// over every q head of the group. Accumulates dK^T, dV^T (d on the register
// row, key on the lane). A key's accumulators see the same steps in the same
// order whatever NW is, so dk and dv do not depend on it.
// ---------------------------------------------------------------------------
// ROPE: q and k are the rotated tensors forward attended over; dk is returned
// with respect to the un-rotated k (rope_cos/rope_sin: fp32 [>=S, DH/2]).
template <int DH, int KTW, int NW, bool ROPE>
__launch_bounds__(64 * NW, DH == 128 ? 3 : 4)
__global__ void flash_bwd_dkv_kernel(
    const short* __restrict__ q,     // [B,S,Hq,D]
    const short* __restrict__ k,     // [B,S,Hk,D]
    const short* __restrict__ v,     // [B,S,Hk,D]
    const short* __restrict__ dout,  // [B,S,Hq,D]
    const float* __restrict__ lseP,  // [B,Hq,Sp]
    const float* __restrict__ drowP,  // [B,Hq,Sp]
    const float* __restrict__ kvmask,  // [B,S] or null
    short* __restrict__ dk,          // [B,S,Hk,D]
    short* __restrict__ dv,          // [B,S,Hk,D]
    const float* __restrict__ rope_cos,  // ROPE only, else null
    const float* __restrict__ rope_sin,
    int B, int S, int Sp, int Hq, int Hk, float scale, int causal) {
  constexpr int NKS = DH / 32;        // k-slices of the S / dP products
  constexpr int NDT = DH / 16;        // d-tiles of dK^T / dV^T
  constexpr int IMG = TS * DH * 2;    // bytes per image
  constexpr int SPI = DH / 16;        // 1 KiB segments per image
  constexpr int WRK = 16 * KTW;       // keys per wave
  constexpr int BRK = WRK * NW;       // keys per workgroup
  constexpr int LD_OFF = 2 * IMG;     // lse[32], Drow[32]
  constexpr int BUF = LD_OFF + 256;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

  const int lane = threadIdx.x & 63;
  // in a scalar register: the branches on it below (the skipped strips, the
  // counted waits) are then scalar branches and EXEC stays all ones around
  // the transposed reads
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15;
  const int l4 = lane >> 4;

  // 1-D grid of ceil(S / BRK) * B * Hk workgroups: a (b, kv head)'s key
  // blocks share an XCD, heaviest (causal: block 0) first
  const bwd_wgmap::WgIndex wg =
      bwd_wgmap::wg_index(blockIdx.x, (S + BRK - 1) / BRK, B * Hk);
  const int bh = wg.bh;                 // over B * Hk (kv heads)
  const int b = bh / Hk;
  const int hk = bh % Hk;
  const int G = Hq / Hk;
  const int kv_base = wg.kb * BRK;
  const int wk = kv_base + wave * WRK;

  const long long qrs = (long long)Hq * DH;
  const long long kvrs = (long long)Hk * DH;
  const short* kp = k + ((long long)b * S) * kvrs + hk * DH;
  const short* vp = v + ((long long)b * S) * kvrs + hk * DH;

  // K/V fragments in registers (B operands: key on the lane)
  bf16x8_t kfrag[KTW][NKS], vfrag[KTW][NKS];
  float maskv[KTW];
#pragma unroll
  for (int kt = 0; kt < KTW; ++kt) {
    const int krow = wk + 16 * kt + l15;
    const int srow = krow < S ? krow : S - 1;
    const short* ks = kp + (long long)srow * kvrs;
    const short* vs = vp + (long long)srow * kvrs;
#pragma unroll
    for (int ks_i = 0; ks_i < NKS; ++ks_i) {
      kfrag[kt][ks_i] =
          *reinterpret_cast<const bf16x8_t*>(ks + ks_i * 32 + l4 * 8);
      vfrag[kt][ks_i] =
          *reinterpret_cast<const bf16x8_t*>(vs + ks_i * 32 + l4 * 8);
    }
    maskv[kt] = (kvmask && krow < S) ? kvmask[(long long)b * S + krow] : 0.f;
  }
  // Consume them here, before the first DMA is issued: the compiler then
  // waits for these loads now, not with a vmcnt(0) at their first use inside
  // the loop, where it would also wait for the steps in flight.
#pragma unroll
  for (int kt = 0; kt < KTW; ++kt) {
#pragma unroll
    for (int ks_i = 0; ks_i < NKS; ++ks_i) {
      asm volatile("" : "+v"(kfrag[kt][ks_i]));
      asm volatile("" : "+v"(vfrag[kt][ks_i]));
    }
    asm volatile("" : "+v"(maskv[kt]));
  }

  f32x4_t dk_acc[NDT][KTW], dv_acc[NDT][KTW];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int kt = 0; kt < KTW; ++kt) {
      dk_acc[dt][kt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      dv_acc[dt][kt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }

  const int q_start = causal ? kv_base : 0;  // multiple of 32
  const int nq = (S - q_start + TS - 1) / TS;
  const int total = G * nq;

  static_assert(NW >= SPI || SPI % NW == 0,
                "the waves share an image's segments evenly");
  // one step's loads: the Q and dO images, lse/Drow. Wave w issues segments
  // w, w + NW, .. of each image.
  auto issue = [&](int g, int qb, int bufi) {
    const int h = hk * G + g;
    char* buf = smem + bufi * BUF;
    const short* qp = q + ((long long)b * S) * qrs + h * DH;
    const short* dop = dout + ((long long)b * S) * qrs + h * DH;
    const long long roff = ((long long)b * Hq + h) * Sp;
#pragma unroll
    for (int i = 0; i < (SPI + NW - 1) / NW; ++i) {
      const int sseg = wave + i * NW;
      if (sseg < SPI) {
        issue_rm<DH>(qp, qrs, qb, S, buf, sseg, lane);
        issue_rm<DH>(dop, qrs, qb, S, buf + IMG, sseg, lane);
      }
    }
    if (wave == 0) {
      const float* s = (lane < 32 ? lseP : drowP) + roff + qb + (lane & 31);
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(s),
          reinterpret_cast<unsigned int*>(buf + LD_OFF), 4, 0, 0);
    }
  };

  int g_nx = 0, qb_nx = q_start;  // the step to issue next
  issue(g_nx, qb_nx, 0);
  for (int it = 0; it < total; ++it) {
    const int qb = qb_nx;
    // this step's loads (the only ones in flight) have landed; after the
    // barrier every wave is also done reading the other buffer. The bare
    // barrier, not __syncthreads(): every LDS read of step it-1 was waited
    // for before its MFMA, and the wait above is the only fence needed.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    qb_nx += TS;
    if (qb_nx >= S) {
      qb_nx = q_start;
      ++g_nx;
    }
    if (it + 1 < total) issue(g_nx, qb_nx, (it + 1) & 1);

    // wave-uniform: nothing admissible in this 32 x 32 strip
    if (wk >= S || (causal && qb + TS - 1 < wk)) continue;
    const bool interior = !kvmask && qb + TS <= S && wk + WRK <= S &&
                          (!causal || qb >= wk + WRK - 1);
    const char* buf = smem + (it & 1) * BUF;
    const float* ld = reinterpret_cast<const float*>(buf + LD_OFF);

    // ---- S = Q K^T ; dP - Drow = dO V^T - Drow (2 q-tiles x 2 key-tiles) --
    f32x4_t s_acc[2][KTW], dp_acc[2][KTW], lrow[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      lrow[qt] = *reinterpret_cast<const f32x4_t*>(ld + 16 * qt + 4 * l4);
      f32x4_t dr = *reinterpret_cast<const f32x4_t*>(ld + 32 + 16 * qt + 4 * l4);
#pragma unroll
      for (int kt = 0; kt < KTW; ++kt) {
        s_acc[qt][kt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        dp_acc[qt][kt] = -dr;
      }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int ks_i = 0; ks_i < NKS; ++ks_i) {
        bf16x8_t aq = read_rm<DH>(buf, l15 + 16 * qt, ks_i, l4);
        bf16x8_t ad = read_rm<DH>(buf + IMG, l15 + 16 * qt, ks_i, l4);
#pragma unroll
        for (int kt = 0; kt < KTW; ++kt) {
          s_acc[qt][kt] = MFMA_BF16_16x16x32(aq, kfrag[kt][ks_i],
                                             s_acc[qt][kt], 0, 0, 0);
          dp_acc[qt][kt] = MFMA_BF16_16x16x32(ad, vfrag[kt][ks_i],
                                              dp_acc[qt][kt], 0, 0, 0);
        }
      }
    __builtin_amdgcn_s_setprio(0);

    // ---- P, dS in place: rows q = qb+16qt+4*l4+r, column key = wk+16kt+l15
    if (interior) {
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int kt = 0; kt < KTW; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float p = __expf(s_acc[qt][kt][r] * scale - lrow[qt][r]);
            s_acc[qt][kt][r] = p;
            dp_acc[qt][kt][r] = p * dp_acc[qt][kt][r] * scale;
          }
    } else {
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int kt = 0; kt < KTW; ++kt) {
          const int gkv = wk + 16 * kt + l15;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int gq = qb + 16 * qt + 4 * l4 + r;
            const bool valid = gq < S && gkv < S && (!causal || gq >= gkv);
            float sval = s_acc[qt][kt][r] * scale + maskv[kt];
            float p = valid ? __expf(sval - lrow[qt][r]) : 0.f;
            s_acc[qt][kt][r] = p;
            dp_acc[qt][kt][r] = p * dp_acc[qt][kt][r] * scale;
          }
        }
    }
    bf16x8_t pb[KTW], dsb[KTW];
#pragma unroll
    for (int kt = 0; kt < KTW; ++kt) {
      pb[kt] = pack_pair(s_acc[0][kt], s_acc[1][kt]);
      dsb[kt] = pack_pair(dp_acc[0][kt], dp_acc[1][kt]);
    }

    // ---- dV^T += dO^T P ; dK^T += Q^T dS --------------------------------
    // A operands by transposed reads of the two row-major images, one d-tile
    // ahead of the MFMAs that use them
    const unsigned qimg = lds_addr(buf);
    tr_frag fq[2], fd[2];
    fq[0] = issue_tr_read<DH>(qimg, 0, lane);
    fd[0] = issue_tr_read<DH>(qimg + IMG, 0, lane);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      if (dt + 1 < NDT) {
        fq[(dt + 1) & 1] = issue_tr_read<DH>(qimg, dt + 1, lane);
        fd[(dt + 1) & 1] = issue_tr_read<DH>(qimg + IMG, dt + 1, lane);
        tr_wait<4>(fq[dt & 1], fd[dt & 1]);
      } else {
        tr_wait<0>(fq[dt & 1], fd[dt & 1]);
      }
      const bf16x8_t aqt = tr_operand(fq[dt & 1]);
      const bf16x8_t adt = tr_operand(fd[dt & 1]);
#pragma unroll
      for (int kt = 0; kt < KTW; ++kt) {
        dv_acc[dt][kt] =
            MFMA_BF16_16x16x32(adt, pb[kt], dv_acc[dt][kt], 0, 0, 0);
        dk_acc[dt][kt] =
            MFMA_BF16_16x16x32(aqt, dsb[kt], dk_acc[dt][kt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // ---- epilogue: lane holds d = 16dt+4*l4 .. +3 of key wk+16kt+l15 -------
#pragma unroll
  for (int kt = 0; kt < KTW; ++kt) {
    const int gkv = wk + 16 * kt + l15;
    if (gkv >= S) continue;
    short* dkr = dk + ((long long)b * S + gkv) * kvrs + hk * DH + 4 * l4;
    short* dvr = dv + ((long long)b * S + gkv) * kvrs + hk * DH + 4 * l4;
    if (ROPE)
      unrotate_row<NDT, KTW>(&dk_acc[0][kt],
                             rope_cos + (long long)gkv * (DH / 2) + 4 * l4,
                             rope_sin + (long long)gkv * (DH / 2) + 4 * l4);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      store4(dkr + 16 * dt, dk_acc[dt][kt]);
      store4(dvr + 16 * dt, dv_acc[dt][kt]);
    }
  }
}

// ---------------------------------------------------------------------------
// PASS 2: q-outer. Block: 4 waves x 32 q rows = 128; kv steps of 32.
// Accumulates dQ^T (d on the register row, q on the lane).
// ---------------------------------------------------------------------------
// ROPE: as in pass 1; dq is returned with respect to the un-rotated q.
template <int DH, bool ROPE>
__launch_bounds__(256, 2)
__global__ void flash_bwd_dq_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lseP,   // [B,Hq,Sp]
    const float* __restrict__ drowP,  // [B,Hq,Sp]
    const float* __restrict__ kvmask,  // [B,S] or null
    short* __restrict__ dq,  // [B,S,Hq,D]
    const float* __restrict__ rope_cos,  // ROPE only, else null
    const float* __restrict__ rope_sin,
    int B, int S, int Sp, int Hq, int Hk, float scale, int causal) {
  constexpr int NKS = DH / 32;
  constexpr int NDT = DH / 16;
  constexpr int IMG = TS * DH * 2;
  constexpr int SPI = DH / 16;
  constexpr int IPI = SPI / 4;
  constexpr int BUF = 2 * IMG;  // K, V
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l15 = lane & 15;
  const int l4 = lane >> 4;

  // causal: the last q block has the most kv steps; launch it first
  const int qtile = gridDim.x - 1 - blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int h = bh % Hq;
  const int hk = h / (Hq / Hk);
  const int qbase = qtile * BR;
  const int wq = qbase + wave * WR;

  const long long qrs = (long long)Hq * DH;
  const long long kvrs = (long long)Hk * DH;
  const short* qp = q + ((long long)b * S) * qrs + h * DH;
  const short* dop = dout + ((long long)b * S) * qrs + h * DH;
  const short* kp = k + ((long long)b * S) * kvrs + hk * DH;
  const short* vp = v + ((long long)b * S) * kvrs + hk * DH;
  const float* mp = kvmask ? kvmask + (long long)b * S : nullptr;

  // Q and dO fragments in registers (B operands: q row on the lane), and
  // the lane's row constants (wq + 31 < Sp: the padded copies are in bounds)
  bf16x8_t qfrag[2][NKS], dofrag[2][NKS];
  float lse_l[2], dr_l[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int qrow = wq + 16 * qt + l15;
    const int srow = qrow < S ? qrow : S - 1;
    const short* qs = qp + (long long)srow * qrs;
    const short* ds = dop + (long long)srow * qrs;
#pragma unroll
    for (int ks_i = 0; ks_i < NKS; ++ks_i) {
      qfrag[qt][ks_i] =
          *reinterpret_cast<const bf16x8_t*>(qs + ks_i * 32 + l4 * 8);
      dofrag[qt][ks_i] =
          *reinterpret_cast<const bf16x8_t*>(ds + ks_i * 32 + l4 * 8);
    }
    lse_l[qt] = lseP[((long long)b * Hq + h) * Sp + qrow];
    dr_l[qt] = drowP[((long long)b * Hq + h) * Sp + qrow];
  }

  f32x4_t dq_acc[NDT][2];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) dq_acc[dt][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int kv_end = causal ? min(S, qbase + BR) : S;
  const int n_tiles = (kv_end + TS - 1) / TS;

  auto issue = [&](int kvb, int bufi) {
    char* buf = smem + bufi * BUF;
#pragma unroll
    for (int i = 0; i < IPI; ++i) {
      const int sseg = i * 4 + wave;
      issue_rm<DH>(kp, kvrs, kvb, S, buf, sseg, lane);
      issue_rm<DH>(vp, kvrs, kvb, S, buf + IMG, sseg, lane);
    }
  };

  issue(0, 0);
  for (int t = 0; t < n_tiles; ++t) {
    const int kvb = t * TS;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < n_tiles) issue(kvb + TS, (t + 1) & 1);

    // wave-uniform: nothing admissible in this 32 x 32 strip
    if (wq >= S || (causal && kvb > wq + WR - 1)) continue;
    const bool interior = !mp && kvb + TS <= S && wq + WR <= S &&
                          (!causal || kvb + TS - 1 <= wq);
    const char* buf = smem + (t & 1) * BUF;

    // ---- S^T = K Q^T ; dP^T - Drow (2 key-tiles x 2 q-tiles) -------------
    f32x4_t s_acc[2][2], dp_acc[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        s_acc[kt][qt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        dp_acc[kt][qt] =
            f32x4_t{-dr_l[qt], -dr_l[qt], -dr_l[qt], -dr_l[qt]};
      }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int ks_i = 0; ks_i < NKS; ++ks_i) {
        bf16x8_t ak = read_rm<DH>(buf, l15 + 16 * kt, ks_i, l4);
        bf16x8_t av = read_rm<DH>(buf + IMG, l15 + 16 * kt, ks_i, l4);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          s_acc[kt][qt] = MFMA_BF16_16x16x32(ak, qfrag[qt][ks_i],
                                             s_acc[kt][qt], 0, 0, 0);
          dp_acc[kt][qt] = MFMA_BF16_16x16x32(av, dofrag[qt][ks_i],
                                              dp_acc[kt][qt], 0, 0, 0);
        }
      }
    __builtin_amdgcn_s_setprio(0);

    // ---- dS^T in place: rows key = kvb+16kt+4*l4+r, column q = wq+16qt+l15
    if (interior) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float p = __expf(s_acc[kt][qt][r] * scale - lse_l[qt]);
            dp_acc[kt][qt][r] = p * dp_acc[kt][qt][r] * scale;
          }
    } else {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gkv = kvb + 16 * kt + 4 * l4 + r;
          const float mv = (mp && gkv < S) ? mp[gkv] : 0.f;
#pragma unroll
          for (int qt = 0; qt < 2; ++qt) {
            const int gq = wq + 16 * qt + l15;
            const bool valid = gq < S && gkv < S && (!causal || gkv <= gq);
            float sval = s_acc[kt][qt][r] * scale + mv;
            float p = valid ? __expf(sval - lse_l[qt]) : 0.f;
            dp_acc[kt][qt][r] = p * dp_acc[kt][qt][r] * scale;
          }
        }
    }
    bf16x8_t dsb[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
      dsb[qt] = pack_pair(dp_acc[0][qt], dp_acc[1][qt]);

    // ---- dQ^T += K^T dS^T -------------------------------------------------
    // K^T by transposed reads of the row-major K image, one d-tile ahead
    const unsigned kimg = lds_addr(buf);
    tr_frag fk[2];
    fk[0] = issue_tr_read<DH>(kimg, 0, lane);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      if (dt + 1 < NDT) {
        fk[(dt + 1) & 1] = issue_tr_read<DH>(kimg, dt + 1, lane);
        tr_wait<2>(fk[dt & 1]);
      } else {
        tr_wait<0>(fk[dt & 1]);
      }
      const bf16x8_t akt = tr_operand(fk[dt & 1]);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
        dq_acc[dt][qt] =
            MFMA_BF16_16x16x32(akt, dsb[qt], dq_acc[dt][qt], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // ---- epilogue: lane holds d = 16dt+4*l4 .. +3 of q row wq+16qt+l15 ------
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int gq = wq + 16 * qt + l15;
    if (gq >= S) continue;
    short* dqr = dq + ((long long)b * S + gq) * qrs + h * DH + 4 * l4;
    if (ROPE)
      unrotate_row<NDT, 2>(&dq_acc[0][qt],
                           rope_cos + (long long)gq * (DH / 2) + 4 * l4,
                           rope_sin + (long long)gq * (DH / 2) + 4 * l4);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) store4(dqr + 16 * dt, dq_acc[dt][qt]);
  }
}

}  // namespace bwd

template <int DH, bool ROPE>
static void launch_bwd(at::Tensor& q, at::Tensor& k, at::Tensor& v,
                       at::Tensor& dout, at::Tensor& out, at::Tensor& lse,
                       at::Tensor& dq, at::Tensor& dk, at::Tensor& dv,
                       const float* mp, const float* cosp, const float* sinp,
                       int B, int S, int Hq, int Hk, float scale,
                       int causal) {
  auto stream = c10::hip::getCurrentHIPStream();
  // row constants, fully rewritten (pad included) by the pre-pass of every
  // call: the only scratch left
  const int Sp = (S + bwd::BR - 1) / bwd::BR * bwd::BR;
  auto drow = at::empty({B, Hq, Sp}, q.options().dtype(at::kFloat));
  auto lseP = at::empty({B, Hq, Sp}, q.options().dtype(at::kFloat));
  auto sp = [](const at::Tensor& t) {
    return reinterpret_cast<const short*>(t.data_ptr());
  };
  auto spm = [](at::Tensor& t) {
    return reinterpret_cast<short*>(t.data_ptr());
  };
  dim3 grid0(Sp / bwd::PT, B * Hq);
  hipLaunchKernelGGL(bwd::bwd_preprocess<DH>, grid0, dim3(256), 0,
                     stream.stream(), sp(dout), sp(out),
                     lse.data_ptr<float>(), drow.data_ptr<float>(),
                     lseP.data_ptr<float>(), B, S, Sp, Hq);
  HIP_CHECK_KERNEL();
  // 1-D: the kernel maps the workgroup id to (key block, b * Hk + kv head)
  // with bwd_wgmap::wg_index, so the grid is exactly their product
  const int nkb1 = (S + bwd::BRK1 - 1) / bwd::BRK1;
  dim3 grid1(nkb1 * B * Hk);
  hipLaunchKernelGGL(
      (bwd::flash_bwd_dkv_kernel<DH, bwd::KTW1, bwd::NW1, ROPE>), grid1,
      dim3(64 * bwd::NW1), 0, stream.stream(), sp(q), sp(k), sp(v), sp(dout),
      lseP.data_ptr<float>(), drow.data_ptr<float>(), mp, spm(dk), spm(dv),
      cosp, sinp, B, S, Sp, Hq, Hk, scale, causal);
  HIP_CHECK_KERNEL();
  dim3 grid2(Sp / bwd::BR, B * Hq);
  hipLaunchKernelGGL((bwd::flash_bwd_dq_kernel<DH, ROPE>), grid2, dim3(256), 0,
                     stream.stream(), sp(q), sp(k), sp(v), sp(dout),
                     lseP.data_ptr<float>(), drow.data_ptr<float>(), mp,
                     spm(dq), cosp, sinp, B, S, Sp, Hq, Hk, scale, causal);
  HIP_CHECK_KERNEL();
}

void flash_check_qkv(const at::Tensor& q, const at::Tensor& k,
                     const at::Tensor& v, const char* who);
const float* flash_check_kvmask(const c10::optional<at::Tensor>& kvmask,
                                const at::Tensor& q);
void check_rope_table(const at::Tensor& cos, const at::Tensor& sin,
                      const at::Tensor& ref, long long S, int D,
                      const char* who);

std::vector<at::Tensor> flash_attn_bwd(at::Tensor q, at::Tensor k,
                                       at::Tensor v, at::Tensor dout,
                                       at::Tensor out, at::Tensor lse,
                                       bool causal, double scale,
                                       c10::optional<at::Tensor> kvmask,
                                       c10::optional<at::Tensor> cos,
                                       c10::optional<at::Tensor> sin) {
  flash_check_qkv(q, k, v, "flash_attn_bwd");
  CHECK_ARG(dout, at::kBFloat16);
  CHECK_ARG(out, at::kBFloat16);
  CHECK_ARG(lse, at::kFloat);
  CHECK_ON(dout, q);
  CHECK_ON(out, q);
  CHECK_ON(lse, q);
  TORCH_CHECK(dout.sizes() == q.sizes() && out.sizes() == q.sizes(),
              "flash_attn_bwd: dout and out must have q's shape");
  int B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3);
  int Hk = k.size(2);
  TORCH_CHECK(lse.dim() == 3 && lse.size(0) == B && lse.size(1) == Hq &&
                  lse.size(2) == S,
              "flash_attn_bwd: lse must be [B,Hq,S]");
  const float* mp = flash_check_kvmask(kvmask, q);
  // scale == 0 selects the default softmax scale 1/sqrt(D), as in forward
  const float fscale =
      scale == 0.0 ? 1.0f / std::sqrt((float)D) : (float)scale;
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  // cos/sin given: q, k are the rotated tensors and dq, dk come back with
  // respect to the un-rotated ones (inverse RoPE in the epilogues)
  TORCH_CHECK(cos.has_value() == sin.has_value(),
              "flash_attn_bwd: cos and sin must be given together");
  const bool rope = cos.has_value();
  const float* cosp = nullptr;
  const float* sinp = nullptr;
  if (rope) {
    check_rope_table(*cos, *sin, q, S, D, "flash_attn_bwd");
    cosp = cos->data_ptr<float>();
    sinp = sin->data_ptr<float>();
  }
  const int ic = causal ? 1 : 0;
#define DSAMD_LAUNCH_BWD(DH_, ROPE_)                                        \
  launch_bwd<DH_, ROPE_>(q, k, v, dout, out, lse, dq, dk, dv, mp, cosp, sinp, \
                         B, S, Hq, Hk, fscale, ic)
  if (D == 128) {
    if (rope) DSAMD_LAUNCH_BWD(128, true); else DSAMD_LAUNCH_BWD(128, false);
  } else {
    if (rope) DSAMD_LAUNCH_BWD(64, true); else DSAMD_LAUNCH_BWD(64, false);
  }
#undef DSAMD_LAUNCH_BWD
  return {dq, dk, dv};
}
