// LDS image of one 32-row step of the flash backward (attention_bwd.hip):
// one row-major [32][DH] bf16 tile that serves BOTH kinds of MFMA operand
// read, so no transposed copy of the tile exists anywhere.
//
//   row read        ds_read_b128: lane (l15, l4) takes T[16*rt + l15][32*ks +
//                   8*l4 .. +7], the A operand of S = Q K^T / dP = dO V^T
//                   (pass 2: K, V) in natural k order.
//   transposed read ds_read_b64_tr_b16, twice: per 16-lane group l4 a block of
//                   4 rows x 16 columns, rows 16*hf + 4*l4 .. +3, columns
//                   16*dt .. +15. Lane 4q+p of the group addresses row q,
//                   columns 4p .. 4p+3; lane i receives column i, row q in
//                   element q. hf = 0, 1 give elements 0..3 and 4..7 of the
//                   A operand T^T[16*dt + l15][.] in the k order of a packed
//                   accumulator pair (4*l4 + j, then 16 + 4*l4 + j).
//
// Layout: plain rows of DH*2 bytes; the 32-byte pair index of a row is XORed
// with the row's 256-byte bank-row index,
//     off(row, byte) = row*RB + (byte ^ (((row / RPB) & (NP - 1)) << 5)),
// RB = DH*2 bytes per row, RPB = 256/RB rows per bank row (1 at D 128, 2 at
// D 64), NP = RB/32 pairs per row (8, 4). Bits 0..4 are untouched, so the two
// 16-byte chunks of a pair and the two 8-byte halves of a chunk keep their
// order: a transposed read's 8*p stays inside the pair it was computed for.
//
// Bank conflicts, bank = (a/4) mod 64 (counted by tests/flash_bwd_layout_check
// .cpp from these same functions):
//   transposed read, per 32-lane half: 8 rows x one 32-byte pair. The 8 rows
//     (8n .. 8n+7) fill 8 (D 128) or 4 (D 64) bank rows; within a bank row
//     position the pair index dt ^ xor(row) is distinct for every row that
//     shares it: conflict-free, degree 1.
//   row read, per ds_read_b128 16-lane group {0-3,12-15,20-27} (+4/+32): the
//     group holds every l15 once, rows {0-3,12-15} at chunk c and rows
//     {4-11} at chunk c^1. Rows r and r^8 share the XOR and differ in the
//     chunk's low bit; all others differ in the pair: conflict-free, degree 1.
//     (The ((row&7)<<4) XOR this replaces was 2-way here: rows r and r^8
//     met on one slot.)
//
// Every address is below 32*RB and a multiple of 8 (16 for row reads). The
// image is filled by global_load_lds in LDS-linear 16-byte pieces, so the
// XOR is applied to the per-lane SOURCE column: dma_src_byte().
//
// Host and device: no HIP headers, so the CPU layout proof compiles this text.
#pragma once

#if defined(__HIPCC__)
#define FBL_HD __host__ __device__ __forceinline__
#else
#define FBL_HD inline
#endif

namespace bwd_layout {

constexpr int TS = 32;  // rows per image

template <int DH>
FBL_HD int img_xor(int row) {
  constexpr int RB = DH * 2;
  constexpr int RPB = 256 / RB;
  constexpr int NP = RB / 32;
  return ((row / RPB) & (NP - 1)) << 5;
}

// byte offset of byte `byte_off` (< DH*2) of row `row` (< 32)
template <int DH>
FBL_HD int img_off(int row, int byte_off) {
  return row * (DH * 2) + (byte_off ^ img_xor<DH>(row));
}

// The 16-byte piece at LDS-linear offset `linear` of the image holds row
// linear / RB; this is the byte offset inside that row it must be loaded from.
template <int DH>
FBL_HD int dma_row(int linear) {
  return linear / (DH * 2);
}
template <int DH>
FBL_HD int dma_src_byte(int linear) {
  return (linear % (DH * 2)) ^ img_xor<DH>(dma_row<DH>(linear));
}

// 16-byte row read of lane `lane`: T[16*rt + l15][32*ks + 8*l4 .. +7]
template <int DH>
FBL_HD int row_read_addr(int lane, int rt, int ks) {
  const int l15 = lane & 15, l4 = lane >> 4;
  return img_off<DH>(16 * rt + l15, (32 * ks + 8 * l4) * 2);
}

// 8-byte address lane `lane` supplies to the transposed read of rows
// 16*hf + 4*l4 .. +3, columns 16*dt .. +15
template <int DH>
FBL_HD int tr_read_addr(int lane, int dt, int hf) {
  const int l15 = lane & 15, l4 = lane >> 4;
  const int q = l15 >> 2, p = l15 & 3;
  return img_off<DH>(16 * hf + 4 * l4 + q, 32 * dt + 8 * p);
}

}  // namespace bwd_layout
