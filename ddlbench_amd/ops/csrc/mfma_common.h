// Primitives shared by the MFMA conv kernels (conv_mfma.hip,
// conv_mfma2.hip, conv_wgrad.hip, conv_stem.hip): fragment vector types,
// the 16-byte global->LDS DMA, the counted vmcnt wait and the XCD block
// remap.
#pragma once

#include "common.h"

// MFMA 16x16x32 bf16 operand / accumulator fragments (bf16 carried as
// raw 16-bit lanes)
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// One 16-byte global_load_lds: every lane DMAs 16 B from src straight
// into LDS at dst (lane-linear destination, no VGPR round trip).
DEV void glds16(const void* src, void* dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// Counted wait: at most N vector-memory operations stay in flight.
// Emits exactly s_waitcnt vmcnt(N); N must fit gfx9's 6-bit vmcnt field.
template <int N> DEV void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit count on gfx950");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Bijective XCD-aware block remap: hardware deals consecutive block ids
// round-robin over the 8 XCDs; this gives each XCD a contiguous chunk of
// the logical tile order (neighbouring tiles share operands in its L2).
DEV int xcd_remap(int block, int nwg) {
  const int q = nwg / 8, rmd = nwg % 8;
  const int xcd = block % 8, idx = block / 8;
  return (xcd < rmd ? xcd * (q + 1) : rmd * (q + 1) + (xcd - rmd) * q) + idx;
}
