// Workgroup id -> (key block, bh) of the flash backward's pass 1
// (attention_bwd.hip, flash_bwd_dkv_kernel), launched as a 1-D grid of
// nkb * nbh workgroups: nkb key blocks for each of nbh = B * Hk (batch, kv
// head) pairs.
//
// Why a map: workgroups are dealt to the 8 XCDs round-robin by linear id, so
// ids i and i + 8 share an XCD and its L2. Every key block of one bh streams
// the same Q / dO rows (G q heads x S x D, twice). With the plain (key block,
// bh) grid those blocks are spread over all 8 L2s and each L2 sees every
// stream; here all blocks of a bh get ids of one residue mod 8, so one L2
// serves a bh and holds as few distinct bh at a time as the CU count allows.
// That is a speed choice only: id % 8 labels the ids that share an XCD, not
// the XCD, and nothing depends on where a workgroup runs.
//
//   bh in complete rounds of 8 (bh < 8 * (nbh / 8)): round r owns the ids
//     [r * 8 * nkb, (r + 1) * 8 * nkb); inside it id % 8 picks the bh and
//     id / 8 the key block, ascending. A round starts at a multiple of 8, so
//     id % 8 is the same before and after subtracting its start.
//   the ragged tail (nbh % 8 bh, all of them when nbh < 8) cannot give each
//     bh an XCD of its own without leaving XCDs idle: it is dealt key block
//     major over the remaining bh, as the plain grid would.
// Key block 0 is the heaviest under the causal mask (it has the most q steps),
// and a bh's blocks come in ascending order of id in both parts: heaviest
// first.
//
// Host and device: no HIP headers, so the CPU check compiles this text
// (tests/flash_bwd_wgmap_check.cpp).
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

}  // namespace bwd_wgmap
