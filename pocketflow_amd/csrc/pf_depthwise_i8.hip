// Int8 inference of MobileNet-v1's depthwise 3x3 layers on activation CODES: the sibling of pf_depthwise.hip's forward
// kernel that reads one byte per input element instead of two.
//
// The producer (pf_bn_act_quant_codes, pf_conv_i8.hip) leaves the activation as unsigned codes c in [0, k_a] with one (alpha_a, beta_a)
// on the device; an exported depthwise kernel [3][3][C][1] is unsigned codes d in [0, k_w] with ONE (alpha_w, beta_w) (a depthwise
// kernel has a single bucket in tensor and in channel mode).  The layer of the decoded operands, taps outside the image contributing
// nothing (TensorFlow 'SAME': front pads floor(total / 2), asymmetric for stride 2 on even sizes), is
//
//   y[b][ho][wo][c] = (alpha_a/k_a)(alpha_w/k_w) P + (alpha_a/k_a) beta_w Sc + beta_a ((alpha_w/k_w) Dv + beta_w V)
//   P = sum over the taps inside the image of code * d[c][r][s],  Sc = sum of those codes,  Dv = sum of those d[c][r][s],  V = their number
//
// MI355X mapping.  No GEMM: one multiply-add per loaded byte, HBM-bound like pf_depthwise.hip, whose strip structure this keeps.  A
// lane owns 16 consecutive channels of a pixel -- one 16-byte vector of codes -- and walks strips of 4 output pixels of one row;
// consecutive lanes read consecutive vectors.  The 3 x (3 + 3 * stride) vectors of a strip go through a buffer descriptor with a
// per-lane byte offset, positions outside the image get an offset outside the buffer and read as code 0: all loads of a strip are
// issued back to back and waited for once (the round-5 lesson in pf_depthwise.hip's header).
// Integer part.  P <= 9 * 255 * 255 < 2^24 is exact in int32.  The three codes of one input COLUMN (rows r = 0..2 of a channel) are
// gathered into the bytes of one dword, the weight table holds the matching column of d, and v_dot4_u32_u8 multiplies and adds a
// column per instruction: 3 instructions per output for P and 3 against 0x010101 for Sc, where the byte -> float route needs 9
// conversions' worth of FMAs and 9 adds.  A gathered column serves every output pixel of the strip that reads it.  The 3 x 16 weight
// dwords of the lane's channels live in registers for the whole launch.
// Epilogue in float32, terms in the order of the formula, one rounding to the output type.  beta_a is 0 in practice (ReLU outputs
// start at 0): the kernel branches on the scalar and only then forms Dv and V, again with dot products, against the per-tap validity
// bytes of the output position.
// Deterministic: no atomics, no workspace, no LDS, no barrier.
#include "pf_depthwise_i8.h"

template <typename TO> __device__ __forceinline__ void dwi_store16(TO* p, const float* v) {
  store8<TO>(p, v);
  store8<TO>(p + 8, v + 8);
}

template <typename TO, int ST>
__global__ __launch_bounds__(DWI_T) void k_dw_i8(const DwiArgs a) {
  TO* __restrict__ y = (TO*)a.y;
  dw_i8_body<ST>(a, [&](int64_t off, const float* v, int) { dwi_store16<TO>(y + off, v); });
}

// ---- host side ---------------------------------------------------------------------------------------------------
extern "C" int pf_dw_i8_supported(int C, int k, int stride) {
  return (C > 0 && (C % 16) == 0 && k == 3 && (stride == 1 || stride == 2)) ? 1 : 0;
}

extern "C" int pf_dw_i8_fwd(const uint8_t* x, const uint32_t* w_cols, const float* w_scale_beta, const float* act_alpha_beta,
                            int act_bits, void* y, int dtype, int B, int H, int W, int C, int stride, int pad_h, int pad_w, int Ho,
                            int Wo, void* stream) {
  if (!pf_dw_i8_supported(C, 3, stride)) return (int)hipErrorInvalidValue;
  if (y == nullptr || !pf_aligned16(y)) return (int)hipErrorInvalidValue;
  DwiArgs a;
  dim3 grid;
  const int err = dwi_setup(a, grid, x, w_cols, w_scale_beta, act_alpha_beta, act_bits, B, H, W, C, stride, pad_h, pad_w, Ho, Wo);
  if (err) return err;
  a.y = y;
  hipStream_t st = (hipStream_t)stream;
#define PF_DWI(TT)                                                                   \
  do {                                                                               \
    if (stride == 1) k_dw_i8<TT, 1><<<grid, DWI_T, 0, st>>>(a);                      \
    else k_dw_i8<TT, 2><<<grid, DWI_T, 0, st>>>(a);                                  \
  } while (0)
  if (dtype == PF_F32) PF_DWI(float);
  else if (dtype == PF_BF16) PF_DWI(bf16_t);
  else return (int)hipErrorInvalidValue;
#undef PF_DWI
  PF_LAUNCH_CHECK();
  return 0;
}
