// Flash attention forward for MI355X (gfx950) — hand-written MFMA kernel.
//
// Role parity: reference uses CUTLASS/flash-attn kernels
// (deepspeed/inference/v2/kernels, csrc/transformer/inference/csrc/softmax.cu).
// MI355X-native design (guide §B "fused attention prefill"): one kernel,
// flash_fwd_v6_kernel below — 8 waves/block, 256 q-rows per block (32 per
// wave), KV tiles of 64, mfma_f32_32x32x16_bf16, online softmax in fp32
// registers, causal and additive kv-column masking, GQA via head-group
// indexing; saves per-row LSE for the backward pass.
// A q row with no admissible kv column (fully masked) yields out = 0 and
// lse = -inf.
// Correctness: elementwise against a float64 reference with derived bounds
// (tests/test_attention_edges_gpu.py, tests/test_flash_fwd_vimage_gpu.py,
// references in tests/attn_refs.py); the LDS layout is proven on the CPU
// (tests/test_flash_fwd_layout_cpu.py).
#include <torch/extension.h>

#include "common.h"
#include "flash_fwd_layout.h"
#include "lds_tr_read.h"

using bf16x8_t = __attribute__((ext_vector_type(8))) short;

// ===========================================================================
// v6: 8-wave 32x32 "swapped QK^T" forward (guide §B 8-warp ladder).
//   - each wave owns 32 q rows (block = 256 q rows), KV tiles of 64
//   - S^T = K·Q^T via mfma_f32_32x32x16_bf16: C col = q = lane&31, so the
//     softmax row (over kv) is LANE-LOCAL: in-lane reduce + one half-swap
//   - P stays in registers: cvt_pk to bf16 pairs + permlane32_swap build
//     the PV A/B fragments directly — no P LDS staging, no cross-wave sync
//   - PV computed as O^T = V^T·P^T so O's q is also lane-local and the
//     online-softmax rescale is a scalar multiply
//   - K and V each have ONE row-major [64][DH] LDS image per tile, both
//     filled by global_load_lds (pre-swizzled source column) into a double
//     buffer: tile t+1 is in flight while tile t computes, one barrier per
//     tile. K is read by rows (ds_read_b128); V's MFMA operand is read
//     TRANSPOSED in hardware (ds_read_b64_tr_b16, lds_tr_read.h), one d-tile
//     ahead of its MFMAs. No transposed copy of V is made. The layout, with
//     its bank-conflict argument (both reads degree 1), is flash_fwd_layout.h.
//   - image rows past S-1 repeat row S-1 (nothing outside q, k, v is read);
//     their score is -inf, so their P is exactly 0.
// C/D layout (32x32x16): col=lane&31, row=(reg&3)+8*(reg>>2)+4*(lane>>5).
// A/B operand: row(col)=lane&31, k=(lane>>5)*8+j.
// ===========================================================================

using f32x16_t = __attribute__((ext_vector_type(16))) float;
#define MFMA_BF16_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_bf16

constexpr int QB5 = 32;    // q rows per wave
constexpr int QT5 = 256;   // q rows per block (8 waves)
constexpr int KT5 = 64;    // kv rows per tile

// exchange a scalar with the other half-wave (VALU permlane, no LDS pipe)
DEV_INLINE float half_swap(float x, int hi) {
  int i = __builtin_bit_cast(int, x);
  auto r = __builtin_amdgcn_permlane32_swap(i, i, false, false);
  return __builtin_bit_cast(float, hi ? r[0] : r[1]);
}

// pack two f32 into a u32 of 2 bf16 (compiler emits v_cvt_pk_bf16_f32)
DEV_INLINE unsigned int cvtpk2(float lo, float hi) {
  unsigned short a = __builtin_bit_cast(unsigned short, (__bf16)lo);
  unsigned short b = __builtin_bit_cast(unsigned short, (__bf16)hi);
  return (unsigned int)a | ((unsigned int)b << 16);
}

static_assert(KT5 == fwd_layout::KT, "the image layout is for 64-key tiles");

// 16 bytes per lane, global -> LDS; the wave's 64 pieces land LDS-linear
DEV_INLINE void fwd_dma16(const short* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      reinterpret_cast<const unsigned int*>(src),
      reinterpret_cast<unsigned int*>(lds_wave_base), 16, 0, 0);
}

// the 4 k-slices x 2 halves of V's operand for one d-tile: one base register,
// the (ks, hf) constants of the layout in the offset field
template <int DH>
DEV_INLINE void issue_v_dtile(tr_frag (&f)[4], unsigned base) {
  using namespace fwd_layout;
  f[0] = issue_tr_read_off<v_tr_step<DH>(0, 0), v_tr_step<DH>(0, 1)>(base);
  f[1] = issue_tr_read_off<v_tr_step<DH>(1, 0), v_tr_step<DH>(1, 1)>(base);
  f[2] = issue_tr_read_off<v_tr_step<DH>(2, 0), v_tr_step<DH>(2, 1)>(base);
  f[3] = issue_tr_read_off<v_tr_step<DH>(3, 0), v_tr_step<DH>(3, 1)>(base);
}

// kvmask: optional [B,S] additive float mask over kv columns (padding
// masks, ALiBi-free BERT-class workloads); nullptr = none.
template <int DH>
__launch_bounds__(512, 2)
__global__ void flash_fwd_v6_kernel(
    const short* __restrict__ q,  // [B,S,Hq,D]
    const short* __restrict__ k,  // [B,S,Hk,D]
    const short* __restrict__ v,  // [B,S,Hk,D]
    short* __restrict__ out,      // [B,S,Hq,D]
    float* __restrict__ lse_out,  // [B,Hq,S]
    const float* __restrict__ kvmask,  // [B,S] or null
    int B, int S, int Hq, int Hk, float scale, int causal) {
  // K and V double-buffered, one array: [K 0][K 1][V 0][V 1], each a
  // row-major image of flash_fwd_layout.h. Tile t+1's global_load_lds issue
  // before tile t's compute.
  constexpr int IMG = KT5 * DH * 2;  // bytes per image
  __shared__ __attribute__((aligned(16))) char smem[4 * IMG];

  const int lane = threadIdx.x & 63;
  // in a scalar register: the LDS-DMA segment bases are then scalar and no
  // branch on it can leave EXEC partial around the transposed reads
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31;
  const int hi = lane >> 5;  // half-wave: 0 or 1

  constexpr int NQF = DH / 16;   // Q k-slices
  constexpr int NOT = DH / 32;   // O^T d m-tiles

  const int qtile = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int h = bh % Hq;
  const int hk = h / (Hq / Hk);
  const int qbase = qtile * QT5;
  const int wave_q = qbase + wave * QB5;
  const int my_q = wave_q + l31;  // this lane's q row (lane-local softmax)

  const long long qrs = (long long)Hq * DH;
  const long long kvrs = (long long)Hk * DH;
  const short* qp = q + ((long long)b * S) * qrs + h * DH;
  const short* kp = k + ((long long)b * S) * kvrs + hk * DH;
  const short* vp = v + ((long long)b * S) * kvrs + hk * DH;
  const float* mp = kvmask ? kvmask + (long long)b * S : nullptr;

  // ---- Q fragments: qfrag[ks] = Q[my_q][16*ks + hi*8 .. +7] -------------
  bf16x8_t qfrag[NQF];
  {
    int srow = my_q < S ? my_q : S - 1;
    const short* src = qp + (long long)srow * qrs + hi * 8;
#pragma unroll
    for (int ks = 0; ks < NQF; ++ks)
      qfrag[ks] = *reinterpret_cast<const bf16x8_t*>(src + 16 * ks);
    // Consume them here, before the first DMA is issued: the compiler then
    // waits for these loads now, not with a vmcnt(0) at their first use
    // inside the loop, where it would also wait for the tile in flight.
#pragma unroll
    for (int ks = 0; ks < NQF; ++ks) asm volatile("" : "+v"(qfrag[ks]));
  }

  // softmax runs in the exp2 domain (v_exp_f32 is natively 2^x): S values
  // are scaled by scale*log2(e) once, so every exp is a bare v_exp with no
  // hidden *log2e multiply; LSE converts back with ln2 at the epilogue.
  const float sc2 = scale * 1.44269504f;
  float m_run = -INFINITY, l_run = 0.f;
  f32x16_t ot[NOT];  // O^T accum: rows d = 32*mt + (reg&3)+8*(reg>>2)+4*hi
#pragma unroll
  for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[mt][r] = 0.f;

  const int kv_end = causal ? min(S, qbase + QT5) : S;
  const int n_tiles = (kv_end + KT5 - 1) / KT5;

  // One tile's loads: an image is IMG/1024 wave segments of 1024 bytes (64
  // lanes x 16 B, LDS-linear), so the layout's XOR is applied to the per-lane
  // SOURCE column. Rows past S-1 repeat row S-1.
  constexpr int SEGS = IMG / 1024;
  static_assert(SEGS % 8 == 0, "whole passes of the 8 waves");
  constexpr int PASSES = SEGS / 8;
  auto issue_tile = [&](int t_) {
    char* kimg_ = smem + (t_ & 1) * IMG;
    char* vimg_ = smem + (2 + (t_ & 1)) * IMG;
#pragma unroll
    for (int pass = 0; pass < PASSES; ++pass) {
      const int seg = pass * 8 + wave;
      const int linear = seg * 1024 + lane * 16;
      const int grow = t_ * KT5 + fwd_layout::dma_row<DH>(linear);
      const int srow = grow < S ? grow : S - 1;
      const long long roff = (long long)srow * kvrs;
      fwd_dma16(kp + roff + (fwd_layout::k_dma_src_byte<DH>(linear) >> 1),
                kimg_ + seg * 1024);
      fwd_dma16(vp + roff + (fwd_layout::v_dma_src_byte<DH>(linear) >> 1),
                vimg_ + seg * 1024);
    }
  };

  const unsigned smem_a = lds_addr(smem);
  issue_tile(0);

  for (int t = 0; t < n_tiles; ++t) {
    const int kvbase = t * KT5;
    // This tile's loads (the only ones in flight) have landed; after the
    // barrier every wave is also done reading the other buffers. The bare
    // barrier: every LDS read of tile t-1 was waited for before its MFMA.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 1 < n_tiles) issue_tile(t + 1);  // lands in the other buffers
    const char* kimg = smem + (t & 1) * IMG;
    const unsigned vimg = smem_a + (2 + (t & 1)) * IMG;

    // ---- S^T = K Q^T: st[mt] rows kv = kvbase+32mt+(r&3)+8*(r>>2)+4hi ---
    f32x16_t st[2];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f32x16_t acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < NQF; ++ks) {
        bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(
            kimg + fwd_layout::k_row_read_addr<DH>(lane, mt, ks));
        acc = MFMA_BF16_32x32x16(kf, qfrag[ks], acc, 0, 0, 0);
      }
      st[mt] = acc;
    }
    __builtin_amdgcn_s_setprio(0);

    // V's operand for d-tile 0: the reads fly under the softmax
    tr_frag vf[2][4];
    issue_v_dtile<DH>(vf[0], vimg + fwd_layout::v_tr_lane_base<DH>(lane, 0));

    // ---- online softmax (lane-local q row) ------------------------------
    // btile is wave-uniform: interior tiles take the cmp-free path
    const bool btile = (causal && (kvbase + KT5 > qbase)) ||
                       (kvbase + KT5 > S) || mp != nullptr;
    float tmax = -INFINITY;
    if (btile) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float sv = st[mt][r] * sc2;
          int gkv = kvbase + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (mp && gkv < S) sv += mp[gkv] * 1.44269504f;
          if ((causal && gkv > my_q) || gkv >= S) sv = -INFINITY;
          st[mt][r] = sv;
          tmax = fmaxf(tmax, sv);
        }
    } else {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float sv = st[mt][r] * sc2;
          st[mt][r] = sv;
          tmax = fmaxf(tmax, sv);
        }
    }
    tmax = fmaxf(tmax, half_swap(tmax, hi));
    // defer-max (guide T13): only rescale when the running max grew by more
    // than 8/ln2 (P is then bounded by e^8, which f32 accum tolerates; LSE
    // stays exact). Masked values rely on exp2(-inf)=0 — no per-value select.
    // (-inf - -inf = NaN fails the <= too, so a still-empty lane rescales.)
    if (!__all(tmax - m_run <= 11.5416f)) {
      float m_new = fmaxf(m_run, tmax);
      float c = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= c;
#pragma unroll
      for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[mt][r] *= c;
      m_run = m_new;
    }
    // A lane whose columns were all -inf so far (left padding, a fully
    // masked row) still has m_run = -inf, and -inf - -inf is NaN: subtract
    // 0 instead, so those P are exp2(-inf) = 0. Only boundary / masked
    // tiles can hold -inf; interior tiles keep the select-free path.
    float m_sub = m_run;
    if (btile) m_sub = (m_run == -INFINITY) ? 0.f : m_run;
    float psum = 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = __builtin_amdgcn_exp2f(st[mt][r] - m_sub);
        st[mt][r] = p;  // P overwrites S in-register
        psum += p;
      }
    psum += half_swap(psum, hi);
    l_run += psum;

    // ---- build P fragments in-register ----------------------------------
    // pfrag[ks] = P[q=l31][kv = kvbase + 16ks + hi*8 + j]; own C regs hold
    // kv (r&3)+8*(r>>2)+4hi — the other half-wave holds the 4-offset rows.
    // permlane32_swap(wA, wB): x = {lo: wA_lo, hi: wB_lo},
    //                          y = {lo: wA_hi, hi: wB_hi}
    // with wA = own rows +0..3 packed, wB = own rows +4..7 packed gives
    // each half the partner words it needs (guide T12).
    bf16x8_t pfrag[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      int mt = ks >> 1, s = ks & 1;  // kv 16s..16s+15 of m-tile mt
      // own regs 8s..8s+3 = rows 16s+4hi+0..3 ; 8s+4..8s+7 = +8
      unsigned int wA0 = cvtpk2(st[mt][8 * s + 0], st[mt][8 * s + 1]);
      unsigned int wA1 = cvtpk2(st[mt][8 * s + 2], st[mt][8 * s + 3]);
      unsigned int wB0 = cvtpk2(st[mt][8 * s + 4], st[mt][8 * s + 5]);
      unsigned int wB1 = cvtpk2(st[mt][8 * s + 6], st[mt][8 * s + 7]);
      auto r0 = __builtin_amdgcn_permlane32_swap((int)wA0, (int)wB0,
                                                 false, false);
      auto r1 = __builtin_amdgcn_permlane32_swap((int)wA1, (int)wB1,
                                                 false, false);
      unsigned int w[4] = {(unsigned int)r0[0], (unsigned int)r1[0],
                           (unsigned int)r0[1], (unsigned int)r1[1]};
      pfrag[ks] = *reinterpret_cast<bf16x8_t*>(w);
    }

    // ---- O^T += V^T P^T  (4 d m-tiles x 4 kv k-slices) ------------------
    // A operand V[16ks + 8hi + j][32mt + l31] by transposed reads of the
    // row-major image, one d-tile (8 reads) ahead of the MFMAs that use them
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mt = 0; mt < NOT; ++mt) {
      if (mt + 1 < NOT) {
        issue_v_dtile<DH>(
            vf[(mt + 1) & 1],
            vimg + fwd_layout::v_tr_lane_base<DH>(lane, mt + 1));
        tr_wait<8>(vf[mt & 1]);
      } else {
        tr_wait<0>(vf[mt & 1]);
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        ot[mt] = MFMA_BF16_32x32x16(tr_operand(vf[mt & 1][ks]), pfrag[ks],
                                    ot[mt], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // ---- epilogue: O^T lane holds d rows for its q col --------------------
  if (my_q < S) {
    float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
    short* orow = out + ((long long)b * S + my_q) * qrs + h * DH;
#pragma unroll
    for (int mt = 0; mt < NOT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        int d0 = 32 * mt + 8 * g + 4 * hi;  // 4 consecutive d
        unsigned int w[2];
        w[0] = cvtpk2(ot[mt][4 * g + 0] * inv_l, ot[mt][4 * g + 1] * inv_l);
        w[1] = cvtpk2(ot[mt][4 * g + 2] * inv_l, ot[mt][4 * g + 3] * inv_l);
        *reinterpret_cast<unsigned long long*>(orow + d0) =
            *reinterpret_cast<unsigned long long*>(w);
      }
    if (hi == 0 && lse_out)  // back to base-e: lse = ln2*(m2 + log2 l)
      lse_out[((long long)b * Hq + h) * S + my_q] =
          0.693147181f * (m_run + __log2f(fmaxf(l_run, 1e-30f)));
  }
}

// Shared host-side contract of flash_attn_fwd / flash_attn_bwd: the kernels
// index k and v with q's B and S and reinterpret every pointer as bf16.
void flash_check_qkv(const at::Tensor& q, const at::Tensor& k,
                     const at::Tensor& v, const char* who) {
  CHECK_ARG(q, at::kBFloat16);
  CHECK_ARG(k, at::kBFloat16);
  CHECK_ARG(v, at::kBFloat16);
  CHECK_ON(k, q);
  CHECK_ON(v, q);
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, who,
              ": q, k, v must be [B,S,H,D]");
  const long D = q.size(3);
  TORCH_CHECK(D == 128 || D == 64, who, ": head_dim must be 64 or 128");
  TORCH_CHECK(q.size(1) >= 1 && q.size(2) >= 1 && k.size(2) >= 1, who,
              ": empty sequence or head dimension");
  TORCH_CHECK(k.size(0) == q.size(0) && k.size(1) == q.size(1) &&
                  k.size(3) == D,
              who, ": k must be [B,S,Hk,D] with q's B, S and D");
  TORCH_CHECK(v.sizes() == k.sizes(), who, ": v must have k's shape");
  TORCH_CHECK(q.size(2) % k.size(2) == 0, who, ": GQA requires Hq % Hk == 0");
}

const float* flash_check_kvmask(const c10::optional<at::Tensor>& kvmask,
                                const at::Tensor& q) {
  if (!kvmask.has_value() || !kvmask->defined()) return nullptr;
  TORCH_CHECK(kvmask->is_cuda() && kvmask->device() == q.device() &&
                  kvmask->scalar_type() == at::kFloat &&
                  kvmask->is_contiguous() &&
                  kvmask->numel() == q.size(0) * q.size(1),
              "kvmask must be a contiguous float [B,S] tensor on q's device");
  return kvmask->data_ptr<float>();
}

std::vector<at::Tensor> flash_attn_fwd(at::Tensor q, at::Tensor k,
                                       at::Tensor v, bool causal,
                                       double scale,
                                       c10::optional<at::Tensor> kvmask) {
  flash_check_qkv(q, k, v, "flash_attn_fwd");
  int B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3);
  int Hk = k.size(2);
  const float* mp = flash_check_kvmask(kvmask, q);
  // scale == 0 selects the default softmax scale 1/sqrt(D)
  const float fscale =
      scale == 0.0 ? 1.0f / std::sqrt((float)D) : (float)scale;
  auto out = at::empty_like(q);
  auto lse = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid((S + QT5 - 1) / QT5, B * Hq);
  if (D == 128) {
    hipLaunchKernelGGL(flash_fwd_v6_kernel<128>, grid, dim3(512), 0,
                       stream.stream(),
                       reinterpret_cast<const short*>(q.data_ptr()),
                       reinterpret_cast<const short*>(k.data_ptr()),
                       reinterpret_cast<const short*>(v.data_ptr()),
                       reinterpret_cast<short*>(out.data_ptr()),
                       lse.data_ptr<float>(), mp, B, S, Hq, Hk, fscale,
                       causal ? 1 : 0);
  } else {
    hipLaunchKernelGGL(flash_fwd_v6_kernel<64>, grid, dim3(512), 0,
                       stream.stream(),
                       reinterpret_cast<const short*>(q.data_ptr()),
                       reinterpret_cast<const short*>(k.data_ptr()),
                       reinterpret_cast<const short*>(v.data_ptr()),
                       reinterpret_cast<short*>(out.data_ptr()),
                       lse.data_ptr<float>(), mp, B, S, Hq, Hk, fscale,
                       causal ? 1 : 0);
  }
  HIP_CHECK_KERNEL();
  return {out, lse};
}
