// Shared by the two first-layer ("stem") convolutions: pf_stem.hip (ResNet: 7x7 / stride 2 / pad 3, 3 -> 64 channels) and
// pf_stem3.hip (MobileNet: 3x3 / stride 2 / 'SAME' by its front pads, 3 -> 16 | 32).  The MFMA bodies differ and stay in their files;
// here is what both families do alike: the argument blocks, the staging of one input row, and the host code of every launcher.
#pragma once
#include "pf_mfma.h"
#include "pf_buffer.h"

#define ST_THREADS 256

// ---- argument blocks ---------------------------------------------------------------------------------------------------------------
// Forward and backward-filter, each WITHOUT (7x7: the window's pad of 3 is in the kernel) and WITH the front pads ph, pw (3x3).  They
// are one record in all but those two fields, and stem_fill() below fills all four; they stay four types because a kernel's symbol
// carries its argument type's name and its code the field offsets: one block with the pads appended changes the code of the 7x7
// kernels (kernarg size, offsets of the implicit arguments), one with the pads in the middle moves every offset they read
// (profiles/stem_fold_isa.txt).
struct StemArgs {
  const bf16_t* X;   // [imgs][H][Wd][3]
  const bf16_t* W;   // [N][k][k][3]
  bf16_t* Y;         // [imgs][Ho][Wo][N]
  int imgs, H, Wd, Ho, Wo;
  int strips, n_items;
  int rsb;           // LDS bytes per staged input row = (Wd + 8) * 8
};
struct Stem3Args {
  const bf16_t* X;
  const bf16_t* W;
  bf16_t* Y;
  int imgs, H, Wd, Ho, Wo, ph, pw;
  int strips, n_items;
  int rsb;
};
struct StemWrwArgs {
  const bf16_t* dY;  // [imgs][Ho][Wo][N]
  const bf16_t* X;   // [imgs][H][Wd][3]
  float* slabs;      // [S][N][k * k * 3]
  int imgs, H, Wd, Ho, Wo;
  int strips, n_items;
  int rsb;
  int dy_bytes;
};
struct Stem3WrwArgs {
  const bf16_t* dY;
  const bf16_t* X;
  float* slabs;
  int imgs, H, Wd, Ho, Wo, ph, pw;
  int strips, n_items;
  int rsb;
  int dy_bytes;
};

// one staged input row: the Wd pixels of 3 channels at `row` -> 4 channels (8 bytes) at `dst`, the LDS pixel of the row's front pad;
// a row outside the image (`live` false, `row` any address inside it) is staged as zeros.  The halo pixels left and right of a row
// are zeroed once per workgroup.  (The caller forms `row`: each family keeps the address arithmetic its code was generated from.)
__device__ __forceinline__ void stem_stage_row(unsigned char* dst, const bf16_t* row, bool live, int pairs, int t0, int tstep) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(row);
  for (int j = t0; j < pairs; j += tstep) {         // two pixels (12 bytes) per task
    uint32_t d0 = 0u, d1 = 0u, d2 = 0u;
    if (live) { d0 = src[3 * j]; d1 = src[3 * j + 1]; d2 = src[3 * j + 2]; }
    *reinterpret_cast<uint2*>(dst + j * 16) = make_uint2(d0, d1 & 0xFFFFu);
    *reinterpret_cast<uint2*>(dst + j * 16 + 8) = make_uint2((d1 >> 16) | (d2 << 16), d2 >> 16);
  }
}
// ... with the row given by its element offset into X (the form the 3x3 kernels were generated from)
__device__ __forceinline__ void stem_stage_row(unsigned char* dst, const bf16_t* X, int64_t row_elems_off, bool live, int pairs, int t0, int tstep) {
  stem_stage_row(dst, X + (live ? row_elems_off : 0), live, pairs, t0, tstep);
}

// ---- host: what the four launchers share ----------------------------------------------------------------------------------------------
// workgroups of a persistent launch over `items` (image, strip) items: each launcher passes its own cap
static inline int stem_grid(int items, int cap) { return items < cap ? items : cap; }

static inline int stem_strips(int Ho, int orows) { return (Ho + orows - 1) / orows; }

// bytes of dY: the backward-filter kernels address it through a buffer descriptor with 31-bit offsets
static inline int64_t stem_dy_bytes(int imgs, int Ho, int Wo, int N) { return (int64_t)imgs * Ho * Wo * N * 2; }
static inline bool stem_dy_fits(int imgs, int Ho, int Wo, int N) { return stem_dy_bytes(imgs, Ho, Wo, N) < ((int64_t)1 << 31); }

// The fields every argument block has, for `orows` output rows per item (the launcher adds its other pointers and, 3x3, the pads).
// false: a pointer the kernels cannot take -- Y / dY (`y16`) moves in 16-byte vectors, the image in dwords, the kernel `W` (forward
// only) in bf16 elements.
template <class Args>
static inline bool stem_fill(Args& a, const void* X, const void* y16, const void* W, int imgs, int H, int Wd, int Ho, int Wo, int orows) {
  a.X = (const bf16_t*)X;
  a.imgs = imgs; a.H = H; a.Wd = Wd; a.Ho = Ho; a.Wo = Wo;
  a.strips = stem_strips(Ho, orows);
  a.n_items = imgs * a.strips;
  a.rsb = (Wd + 8) * 8;
  return pf_aligned16(y16) && !(reinterpret_cast<uintptr_t>(X) & 3u) && !(reinterpret_cast<uintptr_t>(W) & 1u);
}
