// LDS images of one 64-key tile of the flash forward (attention.hip): K and V
// each as ONE row-major [64][DH] bf16 image, filled by global_load_lds.
//
//   K row read      ds_read_b128: lane (l31, hi) takes K[32*mt + l31][16*ks +
//                   8*hi .. +7], the A operand of S^T = K Q^T
//                   (mfma_f32_32x32x16_bf16, natural k order).
//   V transposed    ds_read_b64_tr_b16, twice: the A operand of O^T += V^T P^T
//   read            in lane (l31, hi) is V[16*ks + 8*hi + j][32*mt + l31],
//                   j = 0..7, the k order of the P fragment. The 16-lane group
//                   g = lane>>4 (hi = g>>1, dh = g&1) takes a block of 4 rows
//                   x 16 columns: rows 16*ks + 8*hi + 4*hf .. +3, columns
//                   32*mt + 16*dh .. +15. Lane 4q+p of the group addresses row
//                   q, columns 4p .. 4p+3; lane i receives column i, row q in
//                   element q. hf = 0, 1 give elements 0..3 and 4..7.
//
// Both images are plain rows of RB = DH*2 bytes with an XOR on the byte offset
// inside the row; RPB = 256/RB rows share one 256-byte bank row (1 at D 128,
// 2 at D 64).
//
//   V: the 64-byte unit index is XORed with the bank-row index,
//        v_off(row, byte) = row*RB + (byte ^ (((row/RPB) & (NU-1)) << 6)),
//      NU = RB/64 units per row (4, 2). Bits 0..5 are untouched, so the two
//      16-column blocks of a unit and the 8-byte pieces of a block keep their
//      order. A 32-lane half reads 4 rows (4n .. 4n+3) x one 64-byte unit:
//      the four rows' units land on the four distinct unit slots of the bank
//      rows they fill (D 128: unit mt^q of one bank row each; D 64: rows q, q^1
//      share a bank row at different halves, rows q, q^2 differ in the XOR).
//      Conflict-free, degree 1. The XOR term depends on the row only through
//      (row/RPB) & (NU-1), which adding a multiple of 4 rows does not change:
//      a lane's 2*4 addresses for one mt are one base (v_tr_lane_base) plus
//      the constants v_tr_step(ks, hf), which go into the offset field.
//   K: the 16-byte chunk index is XORed with the bank-row index,
//        k_off(row, byte) = row*RB + (byte ^ (((row/RPB) & (NC-1)) << 4)),
//      NC = RB/16 chunks per row (16, 8). A ds_read_b128 16-lane group, e.g.
//      {0-3,12-15,20-27}, holds 16 rows at one chunk index c; their
//      (row/RPB) & (NC-1) take every value once per position inside the bank
//      row, so the 16 chunks c ^ x fill the 64 banks once: degree 1.
//      (The ((row&7)<<4) XOR this replaces is 2-way at both head dims: rows
//      r and r^8 of a group at D 128, r and r^4 at D 64, meet on one slot.)
//
// Bank = (a/4) mod 64; tests/flash_fwd_layout_check.cpp counts the degrees
// from these same functions. Every address is below 64*RB and a multiple of 8
// (16 for row reads). The images are filled in LDS-linear 16-byte pieces, so
// the XOR is applied to the per-lane SOURCE column: *_dma_src_byte().
//
// Host and device: no HIP headers, so the CPU layout proof compiles this text.
#pragma once

#if defined(__HIPCC__)
#define FFL_HD __host__ __device__ __forceinline__
#else
#define FFL_HD inline
#endif

namespace fwd_layout {

constexpr int KT = 64;  // rows (keys) per image

template <int DH>
FFL_HD int v_xor(int row) {
  constexpr int RB = DH * 2;
  constexpr int RPB = 256 / RB;
  constexpr int NU = RB / 64;
  return ((row / RPB) & (NU - 1)) << 6;
}

template <int DH>
FFL_HD int k_xor(int row) {
  constexpr int RB = DH * 2;
  constexpr int RPB = 256 / RB;
  constexpr int NC = RB / 16;
  return ((row / RPB) & (NC - 1)) << 4;
}

// byte offset of byte `byte_off` (< DH*2) of row `row` (< 64)
template <int DH>
FFL_HD int v_off(int row, int byte_off) {
  return row * (DH * 2) + (byte_off ^ v_xor<DH>(row));
}
template <int DH>
FFL_HD int k_off(int row, int byte_off) {
  return row * (DH * 2) + (byte_off ^ k_xor<DH>(row));
}

// The 16-byte piece at LDS-linear offset `linear` of an image holds row
// linear / RB; *_dma_src_byte is the byte offset inside that row it must be
// loaded from.
template <int DH>
FFL_HD int dma_row(int linear) {
  return linear / (DH * 2);
}
template <int DH>
FFL_HD int v_dma_src_byte(int linear) {
  return (linear % (DH * 2)) ^ v_xor<DH>(dma_row<DH>(linear));
}
template <int DH>
FFL_HD int k_dma_src_byte(int linear) {
  return (linear % (DH * 2)) ^ k_xor<DH>(dma_row<DH>(linear));
}

// 16-byte row read of lane `lane`: K[32*mt + l31][16*ks + 8*hi .. +7]
template <int DH>
FFL_HD int k_row_read_addr(int lane, int mt, int ks) {
  const int l31 = lane & 31, hi = lane >> 5;
  return k_off<DH>(32 * mt + l31, (16 * ks + 8 * hi) * 2);
}

// 8-byte address lane `lane` supplies to the transposed read of rows
// 16*ks + 8*hi + 4*hf .. +3, columns 32*mt + 16*dh .. +15: a per-lane base for
// the d-tile mt plus a constant for (ks, hf).
template <int DH>
FFL_HD int v_tr_lane_base(int lane, int mt) {
  const int l15 = lane & 15, g = lane >> 4;
  const int hi = g >> 1, dh = g & 1;
  const int q = l15 >> 2, p = l15 & 3;
  return v_off<DH>(8 * hi + q, 64 * mt + 32 * dh + 8 * p);
}
template <int DH>
FFL_HD constexpr int v_tr_step(int ks, int hf) {
  return (16 * ks + 4 * hf) * (DH * 2);
}
template <int DH>
FFL_HD int v_tr_read_addr(int lane, int mt, int ks, int hf) {
  return v_tr_lane_base<DH>(lane, mt) + v_tr_step<DH>(ks, hf);
}

}  // namespace fwd_layout
