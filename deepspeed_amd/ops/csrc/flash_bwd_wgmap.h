// Workgroup id -> (block, bh) of the three causal flash kernels, each launched
// as a 1-D grid of (blocks per bh) * nbh workgroups:
//   wg_index  pass 1 of the backward (attention_bwd.hip, flash_bwd_dkv_kernel):
//             nkb key blocks for each of nbh = B * Hk (batch, kv head) pairs;
//   q_index   the q-outer kernels, the forward (attention.hip,
//             flash_fwd_v6_kernel) and pass 2 of the backward
//             (flash_bwd_dq_kernel): nqb q blocks for each of nbh = B * Hq
//             (batch, q head) pairs.
//
// Why a map: workgroups are dealt to the 8 XCDs round-robin by linear id, so
// ids i and i + 8 share an XCD and its L2. Two things follow for a plain
// (block, bh) grid, where id % 8 = block % 8 whenever the block count is even.
//   balance: under the causal mask a q block's work grows with its index and
//     a key block's falls, so the XCD of blocks 0, 8, .. and the XCD of
//     blocks 7, 15, .. get unequal work and the call ends with the heavier
//     (at S 4096: 21 % over the mean with 32 blocks, 41 % with the forward's
//     16). Here every XCD gets whole bh, all of equal weight.
//   locality: every block of one bh streams the same rows (pass 1: Q / dO of
//     G q heads; q-outer: K / V of the kv head). Here all blocks of a bh get
//     ids of one residue mod 8, so one L2 serves a bh and holds as few
//     distinct bh at a time as the CU count allows.
// Both are speed choices only: id % 8 labels the ids that share an XCD, not
// the XCD, and nothing depends on where a workgroup runs.
//
//   bh in complete rounds of 8 (bh < 8 * (nbh / 8)): round r owns the ids
//     [r * 8 * nkb, (r + 1) * 8 * nkb); inside it id % 8 picks the bh and
//     id / 8 the key block, ascending. A round starts at a multiple of 8, so
//     id % 8 is the same before and after subtracting its start.
//   the ragged tail (nbh % 8 bh, all of them when nbh < 8) cannot give each
//     bh an XCD of its own without leaving XCDs idle: it is dealt key block
//     major over the remaining bh, as the plain grid would.
// The heaviest block under the causal mask comes first in a bh, in both parts:
// key block 0 (it has the most q steps) for wg_index, whose key block ascends
// with the id; the LAST q block (the most key steps) for q_index, whose q
// block descends.
// Measured and not built in: walking the G q heads of one kv head on one
// residue in the q-outer kernels (profiles/README.md).
//
// Host and device: no HIP headers, so the CPU checks compile this text
// (tests/flash_bwd_wgmap_check.cpp, tests/flash_qmap_check.cpp).
#pragma once

#if defined(__HIPCC__)
#define FBW_HD __host__ __device__ __forceinline__
#else
#define FBW_HD inline
#endif

namespace bwd_wgmap {

constexpr int NXCD = 8;

struct WgIndex {
  int kb;  // key block, 0 .. nkb-1
  int bh;  // 0 .. nbh-1
};

// id in [0, nkb * nbh): a bijection onto (kb, bh) for every nkb, nbh >= 1
FBW_HD WgIndex wg_index(int id, int nkb, int nbh) {
  const int full = nbh / NXCD * NXCD;  // bh in complete rounds
  const int head = full * nkb;         // their ids
  if (id < head) {
    const int round = id / (NXCD * nkb);
    const int r = id - round * (NXCD * nkb);
    return WgIndex{r / NXCD, round * NXCD + r % NXCD};
  }
  const int rem = nbh - full;
  const int r = id - head;
  return WgIndex{r / rem, full + r % rem};
}

struct QIndex {
  int qb;  // q block, 0 .. nqb-1
  int bh;  // 0 .. nbh-1
};

// The q-outer kernels: id in [0, nqb * nbh) onto (q block, bh), the same map
// with the q block descending as the id ascends.
FBW_HD QIndex q_index(int id, int nqb, int nbh) {
  const WgIndex w = wg_index(id, nqb, nbh);
  return QIndex{nqb - 1 - w.kb, w.bh};
}

}  // namespace bwd_wgmap
