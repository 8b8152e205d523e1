// LDS staging helpers shared by the frame-level kernels (gfx950 only): the XOR swizzle of the 16-byte slots of a 128-byte LDS row
// and the LDS-DMA instruction in the three forms the kernels use.  New kernels use these; only the stand-alone probe programs
// (tools/*_probe.hip) keep copies of their own.
#pragma once
#include "device_utils.h"

namespace asv {

// LDS byte address of a __shared__ array: (uint32_t)(uintptr_t)(lds_byte *)array
typedef __attribute__((address_space(3))) unsigned char lds_byte;

// A 128-byte row holds eight 16-byte slots; slot s of row `row` lives at slot s ^ ((row >> 1) & 7).  The LDS-DMA writes a row group
// linearly, so the swizzle is applied to the SOURCE slot a lane fetches; every reader applies the same function.  With it the 32
// rows a matrix-fragment read touches (one slot each) spread over all banks instead of hitting the same four.
__device__ __forceinline__ int lds_swz(int row, int slot) { return slot ^ ((row >> 1) & 7); }

// One LDS-DMA instruction: every lane of the wave fetches 16 bytes from global memory, lane l's land at LDS byte M0 + 16 l (1 KiB
// per wave, no VGPR round trip).  Inline asm because the destination base travels in M0, a register the compiler reserves for
// itself and does not preserve for us: the write of M0 and the instruction that reads it have to sit in ONE statement, with
// `lds_dst` a wave-uniform LDS byte address (callers pass it through readfirstlane).  These two forms save and restore M0 around
// the instruction, so they are safe anywhere.
// What the caller waits on: the compiler does not count an asm load in its s_waitcnt bookkeeping.  The transfer counts in vmcnt;
// the bytes are in LDS once the ISSUING wave has waited for vmcnt to cover it (s_waitcnt vmcnt(n) by hand), and other waves may
// read them after the workgroup barrier behind that wait.  The "memory" clobber only orders the statement against the compiler's
// own memory accesses.
// Form 1: a 64-bit per-lane address.
__device__ __forceinline__ void glds16(const void *gsrc, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}

// Form 2: a scalar base + a 32-bit per-lane byte offset (no 64-bit VALU address arithmetic per piece).
__device__ __forceinline__ void glds16_s(const void *sbase, uint32_t voff, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

// Form 3: form 2 with M0 declared clobbered instead of saved and restored - two SALU operations less per piece.  M0 is a reserved
// register: clang honours the clobber and warns about it (-Winline-asm), so only translation units built with -Wno-inline-asm
// define ASV_GLDS_CLOBBER_M0 before including this header (the 8-phase kernels, whose loops issue a piece every few matrix
// instructions and in which nothing else the compiler emits depends on M0 across the statement).  Same waits as above.
#ifdef ASV_GLDS_CLOBBER_M0
__device__ __forceinline__ void glds16_s_m0(const void *sbase, uint32_t voff, uint32_t lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %1"
      :
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory", "m0");
}
#endif

}  // namespace asv
