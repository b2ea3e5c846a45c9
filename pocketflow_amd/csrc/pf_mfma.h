// Operand fetch for v_mfma_f32_16x16x32_bf16 where the contraction runs over the SLOW index of an operand in LDS (pixels of an NHWC
// tile, rows of a dense chunk): the one spelling of the device idioms every backward-filter family (pf_wrw.hip, pf_wrw3x3_c64.hip,
// pf_conv3x3_narrow.hip, pf_dense.hip, the stems) is built around.
//
// gfx950 reads a [4 rows][16 columns] bf16 block out of LDS transposed in one instruction, ds_read_b64_tr_b16: lane i of a 16-lane
// group supplies the address of the i-th 8-byte piece of the block (row i >> 2, column quad i & 3) and receives column i, four rows of
// it (pf_v4s).  Every lane gives its OWN address, so a row pitch, a row wrap or a tap shift costs nothing.  Two such reads, rows 0 .. 3
// and the rows sixteen further on, are joined into the eight k-values a lane feeds to the MFMA (pf_join).
//
// The read comes in two forms and a kernel keeps the one it was written with:
//   * pf_tr_read, the compiler's builtin: the compiler schedules the read and places its wait.  Right where no LDS-DMA is pending
//     when the fragments are read (the stems wait for vmcnt(0) behind their staging), and what the wave-private k_wrw_tr was written with.
//   * pf_tr_issue, inline asm: right where the NEXT stage's LDS-DMA is already in flight.  hipcc (ROCm 7.2) treats a pending
//     `buffer_load ... lds` as a store to LDS the builtin may alias and puts `s_waitcnt vmcnt(0)` in front of the first builtin read it
//     meets: in k_wrw2 that wait sat right behind the issue of the next stage's loads, every step waited for the prefetch it had just
//     started.  The asm read is invisible to that pass and carries NO wait: pf_lds_wait() is the wait, and a register is valid behind
//     PF_TIE(reg) placed after it (volatile asm statements keep their order, and the tie is a definition no use can be scheduled in
//     front of).  The caller guarantees that the stage it reads has landed (own counted vmcnt + barrier).
//
// Made under the rule that no kernel's code changes: every helper here compiles to the instructions of the text it replaced
// (profiles/mfma_header_isa.txt).
#pragma once
#include "pf_conv_common.h"

typedef short pf_v4s __attribute__((ext_vector_type(4)));
typedef short pf_v8s __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bf16x8 pf_join(const pf_v4s& lo, const pf_v4s& hi) {
  pf_v8s x;
  x[0] = lo[0]; x[1] = lo[1]; x[2] = lo[2]; x[3] = lo[3];
  x[4] = hi[0]; x[5] = hi[1]; x[6] = hi[2]; x[7] = hi[3];
  return *reinterpret_cast<const bf16x8*>(&x);
}

// `p`: this lane's 8-byte piece, a generic pointer into LDS
__device__ __forceinline__ pf_v4s pf_tr_read(const void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) pf_v4s*)p);
}
// `p`: the piece's LDS byte address (lds_addr); <OFF>: an immediate offset on top of it.  (Two statements, not a default OFF = 0: the
// kernels written with an explicit offset print `offset:0` and the others print none, and the rule above compares the text.)
__device__ __forceinline__ void pf_tr_issue(uint32_t p, pf_v4s& v) {
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=&v"(v) : "v"(p) : "memory");
}
template <int OFF>
__device__ __forceinline__ void pf_tr_issue(uint32_t p, pf_v4s& v) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=&v"(v) : "v"(p), "n"(OFF) : "memory");
}
__device__ __forceinline__ void pf_lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
#define PF_TIE(x) asm volatile("" : "+v"(x) : : "memory")
