// Hardware-transposed LDS reads (ds_read_b64_tr_b16) for MFMA operands taken
// from a ROW-MAJOR image, shared by the flash forward and backward kernels.
//
// The reads are inline assembly: through the builtin the compiler takes them
// to alias the LDS-DMA writes (global_load_lds) of the tiles in flight and
// puts s_waitcnt vmcnt(0) in front, which undoes the prefetch. The compiler
// therefore does not count them either: tr_wait<N>() is the s_waitcnt
// lgkmcnt(N) before a fragment's use, and it takes the fragment so that the
// use cannot move above it.
// They need EXEC all ones: wave-uniform control flow only.
// The per-lane addresses come from the kernel's layout header
// (flash_bwd_layout.h, flash_fwd_layout.h).
#pragma once

#include "common.h"

using lds_u32x4_t = __attribute__((ext_vector_type(4))) unsigned int;
using lds_u32x2_t = __attribute__((ext_vector_type(2))) unsigned int;
using lds_bf16x8_t = __attribute__((ext_vector_type(8))) short;

DEV_INLINE unsigned lds_addr(const char* p) {
  return (unsigned)(size_t)(
      (const __attribute__((address_space(3))) char*)p);
}

// the two 8-byte halves (elements 0..3, 4..7) of one 8-element operand
struct tr_frag {
  lds_u32x2_t lo, hi;
};

// both halves at byte addresses a0, a1
DEV_INLINE tr_frag issue_tr_read(unsigned a0, unsigned a1) {
  tr_frag f;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.lo) : "v"(a0) : "memory");
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.hi) : "v"(a1) : "memory");
  return f;
}

// both halves at base + OFF0, base + OFF1: the constants go into the
// instruction's 16-bit offset field, so one address register serves them all
template <int OFF0, int OFF1>
DEV_INLINE tr_frag issue_tr_read_off(unsigned base) {
  static_assert(OFF0 >= 0 && OFF0 < 65536 && OFF1 >= 0 && OFF1 < 65536,
                "ds offset field is 16 bits");
  tr_frag f;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(f.lo) : "v"(base), "n"(OFF0) : "memory");
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(f.hi) : "v"(base), "n"(OFF1) : "memory");
  return f;
}

template <int N>
DEV_INLINE void tr_wait(tr_frag& a, tr_frag& b) {
  asm volatile("s_waitcnt lgkmcnt(%4)"
               : "+v"(a.lo), "+v"(a.hi), "+v"(b.lo), "+v"(b.hi)
               : "n"(N));
}

template <int N>
DEV_INLINE void tr_wait(tr_frag& a) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a.lo), "+v"(a.hi) : "n"(N));
}

// four fragments (one d-tile of the forward's PV product) behind one wait
template <int N>
DEV_INLINE void tr_wait(tr_frag (&f)[4]) {
  asm volatile("s_waitcnt lgkmcnt(%8)"
               : "+v"(f[0].lo), "+v"(f[0].hi), "+v"(f[1].lo), "+v"(f[1].hi),
                 "+v"(f[2].lo), "+v"(f[2].hi), "+v"(f[3].lo), "+v"(f[3].hi)
               : "n"(N));
}

DEV_INLINE lds_bf16x8_t tr_operand(const tr_frag& f) {
  lds_u32x4_t w = {f.lo[0], f.lo[1], f.hi[0], f.hi[1]};
  return __builtin_bit_cast(lds_bf16x8_t, w);
}
