// MoE routing for MI355X (gfx950): fused top-k gate, dispatch and combine.
//
// Role parity: reference moe/sharded_moe.py top-k gating and the MOELayer
// dispatch / combine around the expert all-to-all. Replaces the eager chain
// (softmax, topk, scatter mask, cumsum over [S, E], gather, boolean indexing,
// index_select / index_copy and their autograd mirrors) by:
//
//   gate      gate_rank_kernel   a workgroup owns TB consecutive tokens; the
//                                logits tile sits in LDS, one lane per token
//                                does softmax + k-pass argmax, wave ballots
//                                rank each choice inside the block
//             gate_scan_kernel   one workgroup, one thread per expert: block
//                                counts -> exclusive offsets, counts, l_aux
//             gate_finish_kernel one thread per (token, choice): loc, keep,
//                                weights, and the slot -> choice inverse map
//             gate_bwd_kernel    row-local dlogits (softmax recomputed)
//   rows      scatter_rows       slot-owner: one wave per [E*C, M] row, every
//                                row written exactly once (copy, scaled copy
//                                or zeros)
//             gather_rows        token-owner: one wave per token, k rows
//                                FMA'd in fp32, one store
//             gather_dot         token-owner: dw[s, j] = <dout[s], row_j>
//
// Phases that depend on each other are separate launches: no workgroup ever
// waits on another. No float atomics: every sum has a fixed order, so every
// output is deterministic.
//
// Ties in the top-k go to the LOWER expert index (value descending, index
// ascending). torch.topk does not promise an order among equal values.
#include <torch/extension.h>

#include <climits>

#include "common.h"

namespace moe {

constexpr int kMaxK = 8;
constexpr int kMaxE = 256;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / WAVE;

// Tokens per workgroup of the gate kernels. The fp32 tile TB * (E | 1) stays
// near 33 KB, so four workgroups fit a CU's LDS at every E.
static inline int block_tokens(int E) {
  return E <= 32 ? 256 : E <= 64 ? 128 : E <= 128 ? 64 : 32;
}

// Odd row stride: lanes walking their own rows hit distinct LDS banks.
DEV_INLINE int row_stride(int E) { return E | 1; }

// rows [nt, E] contiguous in global <-> tile rows of stride row_stride(E).
DEV_INLINE void load_tile(float* __restrict__ tile,
                          const float* __restrict__ g, int nt, int E) {
  const int ldw = row_stride(E);
  for (int i = threadIdx.x; i < nt * E; i += kThreads)
    tile[(i / E) * ldw + (i % E)] = g[i];
}

DEV_INLINE void store_tile(float* __restrict__ g,
                           const float* __restrict__ tile, int nt, int E) {
  const int ldw = row_stride(E);
  for (int i = threadIdx.x; i < nt * E; i += kThreads)
    g[i] = tile[(i / E) * ldw + (i % E)];
}

// In place: row <- softmax(row), fp32, sum in expert order.
DEV_INLINE void softmax_row(float* __restrict__ row, int E) {
  float m = row[0];
  for (int e = 1; e < E; ++e) m = fmaxf(m, row[e]);
  float sum = 0.f;
  for (int e = 0; e < E; ++e) {
    const float ex = expf(row[e] - m);
    row[e] = ex;
    sum += ex;
  }
  for (int e = 0; e < E; ++e) row[e] = row[e] / sum;
}

// logits [S, E] -> idx / vals / rank [S, k] (rank counted inside the block),
// block_counts / block_gsum [nblk, E].
__global__ __launch_bounds__(kThreads) void gate_rank_kernel(
    const float* __restrict__ logits, int* __restrict__ idx,
    float* __restrict__ vals, int* __restrict__ rank,
    int* __restrict__ block_counts, float* __restrict__ block_gsum, int S,
    int E, int k, int TB) {
  extern __shared__ float tile[];
  __shared__ int wavecnt[kWaves][kMaxE];
  __shared__ float gpart[kThreads];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int ldw = row_stride(E);
  const long long s0 = (long long)blockIdx.x * TB;
  const int nt = (int)min((long long)TB, (long long)S - s0);
  load_tile(tile, logits + s0 * E, nt, E);
  __syncthreads();

  const bool has = tid < nt;
  float* row = tile + tid * ldw;
  int my_idx[kMaxK];
  float my_val[kMaxK];
  int my_rank[kMaxK];
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) {
    my_idx[j] = -1;
    my_val[j] = 0.f;
    my_rank[j] = 0;
  }
  if (has) {
    softmax_row(row, E);
    // pass j takes the largest gate that comes after pass j-1's pick in the
    // order (value descending, index ascending)
    float pv = INFINITY;
    int pi = -1;
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      if (j < k) {
        float bv = -1.f;
        int bi = j;
        for (int e = 0; e < E; ++e) {
          const float v = row[e];
          const bool after = v < pv || (v == pv && e > pi);
          if (after && v > bv) {
            bv = v;
            bi = e;
          }
        }
        my_idx[j] = bi;
        my_val[j] = row[bi];
        pv = bv;
        pi = bi;
      }
    }
  }

  // rank inside the wave: lanes below me that chose the same expert
  for (int e = 0; e < E; ++e) {
    bool ch = false;
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) ch |= my_idx[j] == e;
    const unsigned long long b = __ballot(ch);
    const int below = __popcll(b & ((1ull << lane) - 1ull));
#pragma unroll
    for (int j = 0; j < kMaxK; ++j)
      if (my_idx[j] == e) my_rank[j] = below;
    if (lane == 0) wavecnt[wid][e] = __popcll(b);
  }
  __syncthreads();

  if (has) {
    const long long o = (s0 + tid) * k;
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      if (j < k) {
        const int e = my_idx[j];
        int off = 0;
        for (int w = 0; w < wid; ++w) off += wavecnt[w][e];
        idx[o + j] = e;
        vals[o + j] = my_val[j];
        rank[o + j] = my_rank[j] + off;
      }
    }
  }
  if (tid < E) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += wavecnt[w][tid];
    block_counts[(long long)blockIdx.x * E + tid] = c;
  }

  // column sums of the gates: nparts threads per expert walk a chunk of rows
  // each, then one thread per expert adds the parts in order
  const int nparts = kThreads / E;
  const int chunk = (TB + nparts - 1) / nparts;
  if (tid < nparts * E) {
    const int e = tid % E;
    const int p = tid / E;
    const int r1 = min(nt, (p + 1) * chunk);
    float g = 0.f;
    for (int r = p * chunk; r < r1; ++r) g += tile[r * ldw + e];
    gpart[tid] = g;
  }
  __syncthreads();
  if (tid < E) {
    float g = 0.f;
    for (int p = 0; p < nparts; ++p) g += gpart[p * E + tid];
    block_gsum[(long long)blockIdx.x * E + tid] = g;
  }
}

// One workgroup. block_counts becomes the exclusive offset of each block in
// each expert's queue.
__global__ __launch_bounds__(kThreads) void gate_scan_kernel(
    int* __restrict__ block_counts, const float* __restrict__ block_gsum,
    int* __restrict__ counts, float* __restrict__ l_aux, int nblk, int E,
    int S, int k) {
  __shared__ float term[kMaxE];
  const int e = threadIdx.x;
  if (e < E) {
    int run = 0;
    float g = 0.f;
    for (int b = 0; b < nblk; ++b) {
      const long long i = (long long)b * E + e;
      const int c = block_counts[i];
      block_counts[i] = run;
      run += c;
      g += block_gsum[i];
    }
    counts[e] = run;
    term[e] = (g / (float)S) * ((float)run / (float)S);
  }
  __syncthreads();
  if (e == 0) {
    float sum = 0.f;
    for (int i = 0; i < E; ++i) sum += term[i];
    l_aux[0] = sum * (float)E * (float)E / (float)k;
  }
}

DEV_INLINE int choice_loc(const int* __restrict__ rank,
                          const int* __restrict__ block_off,
                          const int* __restrict__ idx, long long i,
                          long long blk, int E) {
  return rank[i] + block_off[blk * E + idx[i]];
}

// n = max(S*k, E*C) work items: item i < S*k finishes choice i, item
// i < E*C clears slot i if no kept choice lands on it.
__global__ __launch_bounds__(kThreads) void gate_finish_kernel(
    const int* __restrict__ idx, const float* __restrict__ vals,
    const int* __restrict__ rank, const int* __restrict__ block_off,
    const int* __restrict__ counts, int* __restrict__ loc,
    unsigned char* __restrict__ keep, float* __restrict__ weights,
    int* __restrict__ slot_token, long long SK, long long EC, int E, int k,
    int C, int TB, int drop) {
  const long long n = SK > EC ? SK : EC;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if (i < SK) {
      const long long s = i / k;
      const long long blk = s / TB;
      const int l = choice_loc(rank, block_off, idx, i, blk, E);
      const bool kp = !drop || l < C;
      float den = 0.f;
      for (int j = 0; j < k; ++j) {
        const long long ii = s * k + j;
        const int ll = choice_loc(rank, block_off, idx, ii, blk, E);
        den += (!drop || ll < C) ? vals[ii] : 0.f;
      }
      den = fmaxf(den, 1e-9f);
      loc[i] = l;
      keep[i] = kp ? 1 : 0;
      weights[i] = kp ? vals[i] / den : 0.f;
      if (kp && l < C) slot_token[(long long)idx[i] * C + l] = (int)i;
    }
    if (i < EC) {
      const int e = (int)(i / C);
      const int c = (int)(i % C);
      if (c >= min(counts[e], C)) slot_token[i] = -1;
    }
  }
}

// dlogits of (weights, l_aux) with the mask held constant.
__global__ __launch_bounds__(kThreads) void gate_bwd_kernel(
    const float* __restrict__ logits, const int* __restrict__ idx,
    const unsigned char* __restrict__ keep, const int* __restrict__ counts,
    const float* __restrict__ dweights, const float* __restrict__ dl_aux,
    float* __restrict__ dlogits, int S, int E, int k, int TB) {
  extern __shared__ float tile[];
  __shared__ float coef[kMaxE];
  const int tid = threadIdx.x;
  const int ldw = row_stride(E);
  const long long s0 = (long long)blockIdx.x * TB;
  const int nt = (int)min((long long)TB, (long long)S - s0);
  if (tid < E)
    coef[tid] = dl_aux[0] * ((float)E * (float)E / (float)k) *
                (float)counts[tid] / (float)S / (float)S;
  load_tile(tile, logits + s0 * E, nt, E);
  __syncthreads();
  if (tid < nt) {
    float* row = tile + tid * ldw;
    softmax_row(row, E);
    const long long o = (s0 + tid) * k;
    int ej[kMaxK];
    float v[kMaxK], dv[kMaxK];
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      ej[j] = -1;
      v[j] = 0.f;
      dv[j] = 0.f;
      if (j < k) {
        const int e = idx[o + j];
        if (e >= 0 && e < E) {
          ej[j] = e;
          v[j] = row[e];
          if (keep[o + j]) {
            dv[j] = dweights[o + j];
            den += v[j];
          } else {
            ej[j] = -1;
          }
        }
      }
    }
    // w_j = v_j / den  =>  dv_j = (dw_j - sum_i dw_i w_i) / den; under the
    // clamp den is a constant and the second term drops
    const bool clamped = den < 1e-9f;
    den = fmaxf(den, 1e-9f);
    float sdw = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxK; ++j)
      if (ej[j] >= 0) sdw += dv[j] * (v[j] / den);
    if (clamped) sdw = 0.f;
    float dot = 0.f;
    for (int e = 0; e < E; ++e) dot += row[e] * coef[e];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      if (ej[j] >= 0) {
        dv[j] = (dv[j] - sdw) / den;
        dot += v[j] * dv[j];
      }
    }
    for (int e = 0; e < E; ++e) row[e] = row[e] * (coef[e] - dot);
#pragma unroll
    for (int j = 0; j < kMaxK; ++j)
      if (ej[j] >= 0) row[ej[j]] = v[j] * (coef[ej[j]] + dv[j] - dot);
  }
  __syncthreads();
  store_tile(dlogits + s0 * E, tile, nt, E);
}

// ------------------------------------------------------------- row kernels
// A row is nvec 16-byte vectors: 8 bf16 or 4 fp32 each.
template <bool BF16>
struct Vec {
  static constexpr int N = BF16 ? 8 : 4;
  DEV_INLINE static void unpack(const f32x4& raw, float* f) {
    if constexpr (BF16) {
      const bf16x8 b = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = bf2f(b.v[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) f[i] = raw.v[i];
    }
  }
  DEV_INLINE static f32x4 pack(const float* f) {
    if constexpr (BF16) {
      bf16x8 b;
#pragma unroll
      for (int i = 0; i < 8; ++i) b.v[i] = f2bf(f[i]);
      return __builtin_bit_cast(f32x4, b);
    } else {
      f32x4 r;
#pragma unroll
      for (int i = 0; i < 4; ++i) r.v[i] = f[i];
      return r;
    }
  }
};

// out [R, M] <- x [S, M] through slot_token [R]: row r copies token
// slot_token[r] / k (times scale[slot_token[r]] in fp32), or is zero.
template <bool BF16>
__global__ __launch_bounds__(kThreads) void scatter_rows_kernel(
    f32x4* __restrict__ out, const f32x4* __restrict__ x,
    const int* __restrict__ slot_token, const float* __restrict__ scale,
    long long R, long long SK, int k, int nvec) {
  using V = Vec<BF16>;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  for (long long r = (long long)blockIdx.x * kWaves + wid; r < R;
       r += (long long)gridDim.x * kWaves) {
    const int tok = slot_token[r];
    f32x4* __restrict__ dst = out + r * nvec;
    if (tok < 0 || tok >= SK) {
      f32x4 z;
      z.v[0] = z.v[1] = z.v[2] = z.v[3] = 0.f;
      for (int v = lane; v < nvec; v += WAVE) dst[v] = z;
      continue;
    }
    const f32x4* __restrict__ src = x + (long long)(tok / k) * nvec;
    if (scale == nullptr) {
#pragma unroll 4
      for (int v = lane; v < nvec; v += WAVE) dst[v] = src[v];
    } else {
      const float sc = scale[tok];
#pragma unroll 4
      for (int v = lane; v < nvec; v += WAVE) {
        float f[V::N];
        V::unpack(src[v], f);
#pragma unroll
        for (int i = 0; i < V::N; ++i) f[i] *= sc;
        dst[v] = V::pack(f);
      }
    }
  }
}

// Vector offsets of a token's k slot rows, -1 where the choice is dropped
// (or does not name a slot of [E, C]).
DEV_INLINE void slot_rows(long long (&pos)[kMaxK], const int* __restrict__ idx,
                          const int* __restrict__ loc,
                          const unsigned char* __restrict__ keep, long long s,
                          int k, int E, int C, int nvec) {
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) {
    pos[j] = -1;
    if (j < k) {
      const long long i = s * k + j;
      const int e = idx[i];
      const int l = loc[i];
      if (keep[i] && e >= 0 && e < E && l >= 0 && l < C)
        pos[j] = ((long long)e * C + l) * nvec;
    }
  }
}

// out [S, M] <- sum_j w[s, j] * src[idx*C + loc] over the kept choices
// (w == nullptr: plain sum), accumulated in fp32, stored once.
template <bool BF16>
__global__ __launch_bounds__(kThreads) void gather_rows_kernel(
    f32x4* __restrict__ out, const f32x4* __restrict__ src,
    const int* __restrict__ idx, const int* __restrict__ loc,
    const unsigned char* __restrict__ keep, const float* __restrict__ w,
    long long S, int k, int E, int C, int nvec) {
  using V = Vec<BF16>;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  for (long long s = (long long)blockIdx.x * kWaves + wid; s < S;
       s += (long long)gridDim.x * kWaves) {
    long long pos[kMaxK];
    float wj[kMaxK];
    slot_rows(pos, idx, loc, keep, s, k, E, C, nvec);
#pragma unroll
    for (int j = 0; j < kMaxK; ++j)
      wj[j] = (w != nullptr && j < k) ? w[s * k + j] : 1.f;
#pragma unroll 2
    for (int v = lane; v < nvec; v += WAVE) {
      float acc[V::N];
#pragma unroll
      for (int i = 0; i < V::N; ++i) acc[i] = 0.f;
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) {
        if (pos[j] >= 0) {
          float f[V::N];
          V::unpack(src[pos[j] + v], f);
#pragma unroll
          for (int i = 0; i < V::N; ++i) acc[i] = fmaf(wj[j], f[i], acc[i]);
        }
      }
      out[s * nvec + v] = V::pack(acc);
    }
  }
}

// dw [S, k] <- <dout[s], src[idx*C + loc]> in fp32; 0 where dropped.
template <bool BF16>
__global__ __launch_bounds__(kThreads) void gather_dot_kernel(
    float* __restrict__ dw, const f32x4* __restrict__ dout,
    const f32x4* __restrict__ src, const int* __restrict__ idx,
    const int* __restrict__ loc, const unsigned char* __restrict__ keep,
    long long S, int k, int E, int C, int nvec) {
  using V = Vec<BF16>;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  for (long long s = (long long)blockIdx.x * kWaves + wid; s < S;
       s += (long long)gridDim.x * kWaves) {
    long long pos[kMaxK];
    float acc[kMaxK];
    slot_rows(pos, idx, loc, keep, s, k, E, C, nvec);
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) acc[j] = 0.f;
    for (int v = lane; v < nvec; v += WAVE) {
      float d[V::N];
      V::unpack(dout[s * nvec + v], d);
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) {
        if (pos[j] >= 0) {
          float f[V::N];
          V::unpack(src[pos[j] + v], f);
#pragma unroll
          for (int i = 0; i < V::N; ++i) acc[j] = fmaf(d[i], f[i], acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      if (j < k) {  // uniform over the wave
        const float a = wave_reduce_sum(acc[j]);
        if (lane == 0) dw[s * k + j] = pos[j] >= 0 ? a : 0.f;
      }
    }
  }
}

static inline size_t tile_bytes(int E, int TB) {
  return (size_t)TB * (E | 1) * sizeof(float);
}

// [R, M] activation rows: bf16 or fp32, contiguous, 16-byte aligned, a whole
// number of 16-byte vectors wide. Returns vectors per row.
static int check_rows(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.dim() == 2 && t.is_contiguous() &&
                  (t.scalar_type() == at::kBFloat16 ||
                   t.scalar_type() == at::kFloat),
              name, " must be a contiguous 2-d bf16 / fp32 device tensor");
  const long long bytes = (long long)t.size(1) * t.element_size();
  TORCH_CHECK(bytes > 0 && bytes % 16 == 0 && bytes / 16 <= INT_MAX &&
                  ptr_aligned(t.data_ptr(), 16),
              name, " rows must be 16-byte aligned and a multiple of 16 bytes");
  return (int)(bytes / 16);
}

static void check_routing(const at::Tensor& idx, const at::Tensor& loc,
                          const at::Tensor& keep, const at::Tensor& ref) {
  CHECK_ARG(idx, at::kInt);
  CHECK_ARG(loc, at::kInt);
  CHECK_ARG(keep, at::kBool);
  CHECK_ON(idx, ref);
  CHECK_ON(loc, ref);
  CHECK_ON(keep, ref);
  TORCH_CHECK(idx.dim() == 2 && idx.size(1) >= 1 && idx.size(1) <= kMaxK &&
                  loc.sizes() == idx.sizes() && keep.sizes() == idx.sizes(),
              "moe routing: idx, loc and keep must all be [S, k], k <= 8");
  TORCH_CHECK(idx.numel() <= INT_MAX, "moe routing: S * k exceeds int32");
}

static inline int row_grid(long long rows) {
  return grid_for(rows * WAVE, kThreads);
}

}  // namespace moe

long moe_gate_block_tokens(long E) { return moe::block_tokens((int)E); }

// -> {idx, vals, rank, block_counts, block_gsum}
std::vector<at::Tensor> moe_gate_rank(at::Tensor logits, long k) {
  CHECK_ARG(logits, at::kFloat);
  TORCH_CHECK(logits.dim() == 2, "moe_gate_rank: logits must be [S, E]");
  const long S = logits.size(0), E = logits.size(1);
  TORCH_CHECK(S >= 1 && S * moe::kMaxK <= INT_MAX,
              "moe_gate_rank: S out of range");
  TORCH_CHECK(k >= 1 && k <= moe::kMaxK && k <= E && E <= moe::kMaxE,
              "moe_gate_rank: needs 1 <= k <= 8 and k <= E <= 256");
  const int TB = moe::block_tokens((int)E);
  const long nblk = (S + TB - 1) / TB;
  auto io = logits.options().dtype(at::kInt);
  auto idx = at::empty({S, k}, io);
  auto vals = at::empty({S, k}, logits.options());
  auto rank = at::empty({S, k}, io);
  auto block_counts = at::empty({nblk, E}, io);
  auto block_gsum = at::empty({nblk, E}, logits.options());
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe::gate_rank_kernel, dim3((unsigned)nblk),
                     dim3(moe::kThreads), moe::tile_bytes((int)E, TB),
                     stream.stream(), logits.data_ptr<float>(),
                     idx.data_ptr<int>(), vals.data_ptr<float>(),
                     rank.data_ptr<int>(), block_counts.data_ptr<int>(),
                     block_gsum.data_ptr<float>(), (int)S, (int)E, (int)k, TB);
  HIP_CHECK_KERNEL();
  return {idx, vals, rank, block_counts, block_gsum};
}

// block_counts [nblk, E] becomes the blocks' exclusive offsets, in place.
// -> {counts [E], l_aux []}
std::vector<at::Tensor> moe_gate_scan(at::Tensor block_counts,
                                      at::Tensor block_gsum, long S, long k) {
  CHECK_ARG(block_counts, at::kInt);
  CHECK_ARG(block_gsum, at::kFloat);
  CHECK_ON(block_gsum, block_counts);
  TORCH_CHECK(block_counts.dim() == 2 &&
                  block_gsum.sizes() == block_counts.sizes(),
              "moe_gate_scan: block_counts and block_gsum must be [nblk, E]");
  const long nblk = block_counts.size(0), E = block_counts.size(1);
  TORCH_CHECK(E >= 1 && E <= moe::kMaxE && nblk >= 1 && nblk <= INT_MAX &&
                  S >= 1 && S <= INT_MAX && k >= 1 && k <= moe::kMaxK,
              "moe_gate_scan: shape out of range");
  auto counts = at::empty({E}, block_counts.options());
  auto l_aux = at::empty({}, block_gsum.options());
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe::gate_scan_kernel, dim3(1), dim3(moe::kThreads), 0,
                     stream.stream(), block_counts.data_ptr<int>(),
                     block_gsum.data_ptr<float>(), counts.data_ptr<int>(),
                     l_aux.data_ptr<float>(), (int)nblk, (int)E, (int)S,
                     (int)k);
  HIP_CHECK_KERNEL();
  return {counts, l_aux};
}

// -> {loc, keep, weights [S, k], slot_token [E * C]}
std::vector<at::Tensor> moe_gate_finish(at::Tensor idx, at::Tensor vals,
                                        at::Tensor rank, at::Tensor block_off,
                                        at::Tensor counts, long C,
                                        bool drop_tokens) {
  CHECK_ARG(idx, at::kInt);
  CHECK_ARG(vals, at::kFloat);
  CHECK_ARG(rank, at::kInt);
  CHECK_ARG(block_off, at::kInt);
  CHECK_ARG(counts, at::kInt);
  CHECK_ON(vals, idx);
  CHECK_ON(rank, idx);
  CHECK_ON(block_off, idx);
  CHECK_ON(counts, idx);
  TORCH_CHECK(idx.dim() == 2 && vals.sizes() == idx.sizes() &&
                  rank.sizes() == idx.sizes(),
              "moe_gate_finish: idx, vals and rank must all be [S, k]");
  const long S = idx.size(0), k = idx.size(1), E = counts.numel();
  TORCH_CHECK(S >= 1 && k >= 1 && k <= moe::kMaxK && E >= k &&
                  E <= moe::kMaxE && S * k <= INT_MAX,
              "moe_gate_finish: shape out of range");
  const int TB = moe::block_tokens((int)E);
  TORCH_CHECK(block_off.dim() == 2 && block_off.size(1) == E &&
                  block_off.size(0) == (S + TB - 1) / TB,
              "moe_gate_finish: block_off must be [ceil(S / TB), E]");
  TORCH_CHECK(C >= 1 && E * C <= INT_MAX,
              "moe_gate_finish: capacity out of range");
  auto loc = at::empty_like(idx);
  auto keep = at::empty({S, k}, idx.options().dtype(at::kBool));
  auto weights = at::empty_like(vals);
  auto slot_token = at::empty({E * C}, idx.options());
  const long long SK = S * k, EC = E * C;
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      moe::gate_finish_kernel, dim3(grid_for(SK > EC ? SK : EC, moe::kThreads)),
      dim3(moe::kThreads), 0, stream.stream(), idx.data_ptr<int>(),
      vals.data_ptr<float>(), rank.data_ptr<int>(), block_off.data_ptr<int>(),
      counts.data_ptr<int>(), loc.data_ptr<int>(),
      reinterpret_cast<unsigned char*>(keep.data_ptr<bool>()),
      weights.data_ptr<float>(), slot_token.data_ptr<int>(), SK, EC, (int)E,
      (int)k, (int)C, TB, drop_tokens ? 1 : 0);
  HIP_CHECK_KERNEL();
  return {loc, keep, weights, slot_token};
}

at::Tensor moe_gate_topk_bwd(at::Tensor logits, at::Tensor idx,
                             at::Tensor keep, at::Tensor counts,
                             at::Tensor dweights, at::Tensor dl_aux) {
  CHECK_ARG(logits, at::kFloat);
  CHECK_ARG(idx, at::kInt);
  CHECK_ARG(keep, at::kBool);
  CHECK_ARG(counts, at::kInt);
  CHECK_ARG(dweights, at::kFloat);
  CHECK_ARG(dl_aux, at::kFloat);
  CHECK_ON(idx, logits);
  CHECK_ON(keep, logits);
  CHECK_ON(counts, logits);
  CHECK_ON(dweights, logits);
  CHECK_ON(dl_aux, logits);
  TORCH_CHECK(logits.dim() == 2 && idx.dim() == 2,
              "moe_gate_topk_bwd: logits [S, E], idx [S, k]");
  const long S = logits.size(0), E = logits.size(1), k = idx.size(1);
  TORCH_CHECK(S >= 1 && S * moe::kMaxK <= INT_MAX && k >= 1 &&
                  k <= moe::kMaxK && k <= E && E <= moe::kMaxE,
              "moe_gate_topk_bwd: shape out of range");
  TORCH_CHECK(idx.size(0) == S && keep.sizes() == idx.sizes() &&
                  dweights.sizes() == idx.sizes() && counts.numel() == E &&
                  dl_aux.numel() == 1,
              "moe_gate_topk_bwd: idx / keep / dweights [S, k], counts [E], "
              "dl_aux scalar");
  auto dlogits = at::empty_like(logits);
  const int TB = moe::block_tokens((int)E);
  const long nblk = (S + TB - 1) / TB;
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      moe::gate_bwd_kernel, dim3((unsigned)nblk), dim3(moe::kThreads),
      moe::tile_bytes((int)E, TB), stream.stream(), logits.data_ptr<float>(),
      idx.data_ptr<int>(),
      reinterpret_cast<const unsigned char*>(keep.data_ptr<bool>()),
      counts.data_ptr<int>(), dweights.data_ptr<float>(),
      dl_aux.data_ptr<float>(), dlogits.data_ptr<float>(), (int)S, (int)E,
      (int)k, TB);
  HIP_CHECK_KERNEL();
  return dlogits;
}

// out [R, M] <- rows of x [S, M] named by slot_token [R] (choice index
// s * k + j, or -1 for a zero row), times scale [S, k] when given.
void moe_scatter_rows(at::Tensor out, at::Tensor x, at::Tensor slot_token,
                      c10::optional<at::Tensor> scale, long k) {
  const int nvec = moe::check_rows(out, "moe_scatter_rows: out");
  TORCH_CHECK(moe::check_rows(x, "moe_scatter_rows: x") == nvec &&
                  x.scalar_type() == out.scalar_type(),
              "moe_scatter_rows: x and out differ in dtype or width");
  CHECK_ARG(slot_token, at::kInt);
  CHECK_ON(x, out);
  CHECK_ON(slot_token, out);
  const long long R = out.size(0), S = x.size(0);
  TORCH_CHECK(slot_token.numel() == R,
              "moe_scatter_rows: slot_token must have one entry per out row");
  TORCH_CHECK(k >= 1 && k <= moe::kMaxK && S * k <= INT_MAX,
              "moe_scatter_rows: k or S * k out of range");
  const float* scale_ptr = nullptr;
  if (scale.has_value()) {
    const at::Tensor& scale_t = *scale;
    CHECK_ARG(scale_t, at::kFloat);
    CHECK_ON(scale_t, out);
    TORCH_CHECK(scale_t.numel() == S * k,
                "moe_scatter_rows: scale must be [S, k]");
    scale_ptr = scale_t.data_ptr<float>();
  }
  if (R == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
#define LAUNCH(BF)                                                          \
  hipLaunchKernelGGL(moe::scatter_rows_kernel<BF>, dim3(moe::row_grid(R)),  \
                     dim3(moe::kThreads), 0, stream.stream(),               \
                     reinterpret_cast<f32x4*>(out.data_ptr()),              \
                     reinterpret_cast<const f32x4*>(x.data_ptr()),          \
                     slot_token.data_ptr<int>(), scale_ptr, R, S * k,       \
                     (int)k, nvec)
  if (out.scalar_type() == at::kBFloat16)
    LAUNCH(true);
  else
    LAUNCH(false);
#undef LAUNCH
  HIP_CHECK_KERNEL();
}

// out [S, M] <- sum over the kept choices of w[s, j] * src[idx * C + loc]
// (w absent: plain sum). src is [E * C, M].
void moe_gather_rows(at::Tensor out, at::Tensor src, at::Tensor idx,
                     at::Tensor loc, at::Tensor keep,
                     c10::optional<at::Tensor> w, long C) {
  const int nvec = moe::check_rows(out, "moe_gather_rows: out");
  TORCH_CHECK(moe::check_rows(src, "moe_gather_rows: src") == nvec &&
                  src.scalar_type() == out.scalar_type(),
              "moe_gather_rows: src and out differ in dtype or width");
  CHECK_ON(src, out);
  moe::check_routing(idx, loc, keep, out);
  const long long S = out.size(0);
  const long k = idx.size(1);
  TORCH_CHECK(idx.size(0) == S, "moe_gather_rows: idx must be [S, k]");
  TORCH_CHECK(C >= 1 && C <= INT_MAX && src.size(0) % C == 0 &&
                  src.size(0) / C <= INT_MAX,
              "moe_gather_rows: src must be [E * C, M]");
  const int E = (int)(src.size(0) / C);
  const float* w_ptr = nullptr;
  if (w.has_value()) {
    const at::Tensor& w_t = *w;
    CHECK_ARG(w_t, at::kFloat);
    CHECK_ON(w_t, out);
    TORCH_CHECK(w_t.sizes() == idx.sizes(),
                "moe_gather_rows: w must be [S, k]");
    w_ptr = w_t.data_ptr<float>();
  }
  if (S == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
#define LAUNCH(BF)                                                          \
  hipLaunchKernelGGL(                                                       \
      moe::gather_rows_kernel<BF>, dim3(moe::row_grid(S)),                  \
      dim3(moe::kThreads), 0, stream.stream(),                              \
      reinterpret_cast<f32x4*>(out.data_ptr()),                             \
      reinterpret_cast<const f32x4*>(src.data_ptr()), idx.data_ptr<int>(),  \
      loc.data_ptr<int>(),                                                  \
      reinterpret_cast<const unsigned char*>(keep.data_ptr<bool>()), w_ptr, \
      S, (int)k, E, (int)C, nvec)
  if (out.scalar_type() == at::kBFloat16)
    LAUNCH(true);
  else
    LAUNCH(false);
#undef LAUNCH
  HIP_CHECK_KERNEL();
}

// dw [S, k] fp32 <- <dout[s], src[idx * C + loc]>, 0 where dropped.
at::Tensor moe_gather_dot(at::Tensor dout, at::Tensor src, at::Tensor idx,
                          at::Tensor loc, at::Tensor keep, long C) {
  const int nvec = moe::check_rows(dout, "moe_gather_dot: dout");
  TORCH_CHECK(moe::check_rows(src, "moe_gather_dot: src") == nvec &&
                  src.scalar_type() == dout.scalar_type(),
              "moe_gather_dot: src and dout differ in dtype or width");
  CHECK_ON(src, dout);
  moe::check_routing(idx, loc, keep, dout);
  const long long S = dout.size(0);
  const long k = idx.size(1);
  TORCH_CHECK(idx.size(0) == S, "moe_gather_dot: idx must be [S, k]");
  TORCH_CHECK(C >= 1 && C <= INT_MAX && src.size(0) % C == 0 &&
                  src.size(0) / C <= INT_MAX,
              "moe_gather_dot: src must be [E * C, M]");
  const int E = (int)(src.size(0) / C);
  auto dw = at::empty({(long)S, k}, dout.options().dtype(at::kFloat));
  if (S == 0) return dw;
  auto stream = c10::hip::getCurrentHIPStream();
#define LAUNCH(BF)                                                          \
  hipLaunchKernelGGL(                                                       \
      moe::gather_dot_kernel<BF>, dim3(moe::row_grid(S)),                   \
      dim3(moe::kThreads), 0, stream.stream(), dw.data_ptr<float>(),        \
      reinterpret_cast<const f32x4*>(dout.data_ptr()),                      \
      reinterpret_cast<const f32x4*>(src.data_ptr()), idx.data_ptr<int>(),  \
      loc.data_ptr<int>(),                                                  \
      reinterpret_cast<const unsigned char*>(keep.data_ptr<bool>()), S,     \
      (int)k, E, (int)C, nvec)
  if (dout.scalar_type() == at::kBFloat16)
    LAUNCH(true);
  else
    LAUNCH(false);
#undef LAUNCH
  HIP_CHECK_KERNEL();
  return dw;
}
