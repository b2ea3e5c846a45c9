// Buffer descriptors, shared by every kernel that reads through one: the descriptor type, its constructor, the LDS-DMA load
// (16 bytes per lane straight into LDS) and the 16-byte register load.  A load whose byte offset lies outside the descriptor's
// size returns zeros -- no branch around it --, and PF_BUFFER_OOB is the offset that lies outside every descriptor (sizes < 2^31).
#pragma once
#include "pf_common.h"

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define PF_BUFFER_OOB 0x80000000u

// The buffer-descriptor type exists only in the device pass; the host pass (which merely emits the launch stub) still has
// to parse the kernel body -- without this the host pass silently DROPS the stubs and the library fails to load.
#if defined(__HIP_DEVICE_COMPILE__)
typedef __amdgpu_buffer_rsrc_t pf_rsrc_t;
#define PF_MAKE_RSRC(p, bytes) __builtin_amdgcn_make_buffer_rsrc((void*)(p), (short)0, (int)(bytes), 0x00020000)
#define PF_BUFFER_LOAD_LDS16(rs, lds, voff, soff) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, LDS_PTR(lds), 16, voff, soff, 0, 0)
typedef uint32_t pf_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 pf_buffer_load16(pf_rsrc_t rs, uint32_t off) {
  const pf_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}
#else
typedef int pf_rsrc_t;
#define PF_MAKE_RSRC(p, bytes) 0
#define PF_BUFFER_LOAD_LDS16(rs, lds, voff, soff) ((void)(rs), (void)(lds), (void)(voff), (void)(soff))
__device__ __forceinline__ uint4 pf_buffer_load16(pf_rsrc_t, uint32_t) { return make_uint4(0, 0, 0, 0); }
#endif
