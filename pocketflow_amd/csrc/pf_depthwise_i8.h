// The depthwise 3x3 kernel on activation CODES of pf_depthwise_i8.hip, shared with its requantising sibling (pf_depthwise_i8_q.hip):
// the buffer loads, the operand struct, the strip loop and the epilogue up to the float32 value of every output.  What happens to
// that value -- one rounding to the output type (k_dw_i8), or the consumer's BatchNorm + activation + static quantiser (k_dw_i8_q)
// -- is the caller's `emit`.
#pragma once
#include "pf_common.h"

#define DWI_T 256
#define DWI_PW 4
#define DWI_OOB 0x80000000u

#if defined(__HIP_DEVICE_COMPILE__)
typedef __amdgpu_buffer_rsrc_t dwi_rsrc_t;
#define DWI_MAKE_RSRC(p, bytes) __builtin_amdgcn_make_buffer_rsrc((void*)(p), (short)0, (int)(bytes), 0x00020000)
typedef uint32_t dwi_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void dwi_load16(dwi_rsrc_t rs, uint32_t off, uint32_t* o) {
  const dwi_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
  o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
}
// sum of the four byte products of a and b, plus c
__device__ __forceinline__ uint32_t dwi_dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }
#else
typedef int dwi_rsrc_t;
#define DWI_MAKE_RSRC(p, bytes) 0
__device__ __forceinline__ void dwi_load16(dwi_rsrc_t, uint32_t, uint32_t* o) { o[0] = o[1] = o[2] = o[3] = 0u; }
__device__ __forceinline__ uint32_t dwi_dot4(uint32_t, uint32_t, uint32_t c) { return c; }
#endif

struct DwiArgs {
  const uint8_t* x;         // [B][H][W][C] codes
  const uint32_t* wcol;     // [C][3]: column s of channel c, d[c][0][s] | d[c][1][s] << 8 | d[c][2][s] << 16
  const float* wsb;         // (alpha_w / k_w, beta_w)
  const float* ab;          // (alpha_a, beta_a)
  void* y;                  // [B][Ho][Wo][C]
  int B, H, W, C, Ho, Wo, ph, pw;
  int C16;                  // 16-channel groups
  int cgb, spb;             // channel groups / strips per workgroup: cgb * spb <= DWI_T
  int strips_w;             // strips per output row
  int total;                // strips in the tensor (< 2^27: the output has fewer than 2^31 elements)
  uint32_t x_bytes;         // size of x (buffer descriptor; < 2^31)
  float ka;
};

// emit(off, v, cg): the sixteen float32 outputs of one pixel, channels 16 cg .. 16 cg + 15, at element offset `off` of the output
template <int ST, typename Emit>
__device__ __forceinline__ void dw_i8_body(const DwiArgs& a, Emit&& emit) {
  const int cgl = threadIdx.x % a.cgb, sl = threadIdx.x / a.cgb;
  const int cg = blockIdx.y * a.cgb + cgl;
  if (cg >= a.C16 || sl >= a.spb) return;                  // lanes left over when cgb does not divide the workgroup
  const dwi_rsrc_t rsx = DWI_MAKE_RSRC(a.x, a.x_bytes);
  uint32_t wc[3][16];
#pragma unroll
  for (int j = 0; j < 16; ++j)
#pragma unroll
    for (int s = 0; s < 3; ++s) wc[s][j] = a.wcol[(int64_t)(cg * 16 + j) * 3 + s];
  const float alpha_a = a.ab[0], beta_a = a.ab[1];
  const float sw = a.wsb[0], bw = a.wsb[1];
  const float sa = alpha_a / a.ka;
  const float f1 = sa * sw, f2 = sa * bw;
  constexpr int NV = (DWI_PW - 1) * ST + 3;
  for (int strip = blockIdx.x * a.spb + sl; strip < a.total; strip += gridDim.x * a.spb) {
    const int swi = strip % a.strips_w;
    const int t = strip / a.strips_w;
    const int ho = t % a.Ho, b = t / a.Ho;
    const int wo0 = swi * DWI_PW;
    // all 3 x NV vectors of the strip are requested before the first one is used (positions outside the image: code 0)
    uint32_t raw[3][NV][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int hi = ho * ST + r - a.ph;
      const bool rok = (unsigned)hi < (unsigned)a.H;
      const uint32_t rbase = (uint32_t)(((int64_t)(b * a.H + hi) * a.W) * a.C + cg * 16);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int wi = wo0 * ST - a.pw + i;
        const bool ok = rok && (unsigned)wi < (unsigned)a.W;
        dwi_load16(rsx, ok ? rbase + (uint32_t)(wi * a.C) : DWI_OOB, raw[r][i]);
      }
    }
    float out[DWI_PW][16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                          // four channels (one dword of every vector) at a time
      uint32_t col[NV][4];                                 // the three rows of input column i, channel 4 q + e, in bytes 0..2
#pragma unroll
      for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          col[i][e] = ((raw[0][i][q] >> (8 * e)) & 0xFFu) | (((raw[1][i][q] >> (8 * e)) & 0xFFu) << 8) |
                      (((raw[2][i][q] >> (8 * e)) & 0xFFu) << 16);
#pragma unroll
      for (int p = 0; p < DWI_PW; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          uint32_t P = 0u, Sc = 0u;
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            P = dwi_dot4(col[p * ST + s][e], wc[s][4 * q + e], P);
            Sc = dwi_dot4(col[p * ST + s][e], 0x00010101u, Sc);
          }
          out[p][4 * q + e] = f1 * (float)P + f2 * (float)Sc;
        }
    }
    if (beta_a != 0.0f) {
      // one branch per strip: Dv and V from the validity bytes of the three rows, per column of each output pixel
      uint32_t rows = 0u;
#pragma unroll
      for (int r = 0; r < 3; ++r) rows |= ((unsigned)(ho * ST + r - a.ph) < (unsigned)a.H ? 1u : 0u) << (8 * r);
#pragma unroll
      for (int p = 0; p < DWI_PW; ++p) {
        uint32_t vm[3];
        int cols = 0;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const bool ok = (unsigned)((wo0 + p) * ST + s - a.pw) < (unsigned)a.W;
          vm[s] = ok ? rows : 0u;
          cols += ok ? 1 : 0;
        }
        const float t3b = bw * (float)(cols * __popc(rows));
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          uint32_t Dv = 0u;
#pragma unroll
          for (int s = 0; s < 3; ++s) Dv = dwi_dot4(wc[s][j], vm[s], Dv);
          out[p][j] += beta_a * (sw * (float)Dv + t3b);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < DWI_PW; ++p) {
      if (wo0 + p >= a.Wo) continue;
      emit(((int64_t)(b * a.Ho + ho) * a.Wo + wo0 + p) * a.C + cg * 16, out[p], cg);
    }
  }
}

// ---- host side: checks and launch geometry shared by the entries (C % 16 == 0 and stride 1 or 2 are the caller's check) ----------
static inline int dwi_setup(DwiArgs& a, dim3& grid, const uint8_t* x, const uint32_t* w_cols, const float* w_scale_beta,
                            const float* act_alpha_beta, int act_bits, int B, int H, int W, int C, int stride, int pad_h, int pad_w,
                            int Ho, int Wo) {
  if (x == nullptr || w_cols == nullptr || w_scale_beta == nullptr || act_alpha_beta == nullptr) return (int)hipErrorInvalidValue;
  if (!pf_aligned16(x) || act_bits < 1 || act_bits > 8) return (int)hipErrorInvalidValue;
  if (B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || pad_h < 0 || pad_w < 0 || pad_h > 2 || pad_w > 2)
    return (int)hipErrorInvalidValue;
  // every output window starts inside the padded image
  if ((int64_t)(Ho - 1) * stride - pad_h >= H || (int64_t)(Wo - 1) * stride - pad_w >= W) return (int)hipErrorInvalidValue;
  const int64_t x_bytes = (int64_t)B * H * W * C;
  if (x_bytes >= ((int64_t)1 << 31) || (int64_t)B * Ho * Wo * C >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  a.x = x; a.wcol = w_cols; a.wsb = w_scale_beta; a.ab = act_alpha_beta; a.y = nullptr;
  a.B = B; a.H = H; a.W = W; a.C = C; a.Ho = Ho; a.Wo = Wo; a.ph = pad_h; a.pw = pad_w;
  a.C16 = C / 16;
  a.cgb = a.C16 < DWI_T ? a.C16 : DWI_T;
  a.spb = DWI_T / a.cgb;
  a.strips_w = (Wo + DWI_PW - 1) / DWI_PW;
  a.total = B * Ho * a.strips_w;
  a.x_bytes = (uint32_t)x_bytes;
  a.ka = uq_k_of_bits(act_bits);
  const int gy = (a.C16 + a.cgb - 1) / a.cgb;
  if (gy > 65535) return (int)hipErrorInvalidValue;
  int gx = (a.total + a.spb - 1) / a.spb;
  const int cap = 2048 / gy > 0 ? 2048 / gy : 1;        // ~8 workgroups per CU, grid-stride beyond
  if (gx > cap) gx = cap;
  grid = dim3((unsigned)gx, (unsigned)gy);
  return 0;
}
