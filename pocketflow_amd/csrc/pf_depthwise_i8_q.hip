// pf_dw_i8_fwd with a REQUANTISING epilogue: on a graph with fixed activation ranges the depthwise layer applies the
// BatchNorm + ReLU6 + quantiser behind it itself and writes what the pointwise convolution reads -- one byte per element where that
// multiplies codes (1 byte in, 1 byte out), the fake-quantised value otherwise.  No statistics pass, no apply pass.
//
// Strip loop and epilogue up to the float32 output `out[p][j]` are pf_depthwise_i8.h's, shared with k_dw_i8: `out` is exactly the value
// the float32 instantiation of that kernel stores.  Then, per element,
//   u = act(fmaf(scale[c], out, shift[c]));   level / value = the static quantiser of pf_act_static.h on (out_alpha, out_beta)
// so the result is, bit for bit, pf_bn_act_quant_static applied to the float32 output of pf_dw_i8_fwd.  The 2 x 16 per-channel
// constants of a lane are loaded where a pixel is stored (eight 16-byte loads that hit the cache), not held across the strip loop:
// the stride-2 parent already needs 218 vector registers.  Sixteen codes leave as one 16-byte store.
#include "pf_depthwise_i8.h"
#include "pf_act_static.h"

struct DwiQArgs {
  const float* ss;          // [2][C] the consumer BatchNorm folded to scale / shift
  const float* oab;         // (alpha, beta) of the OUTPUT range, on the device
  void* out;                // [B][Ho][Wo][C] codes or values
  float ko;                 // 2^out_bits - 1
};

template <typename TO, int ST, int ACT>
__global__ __launch_bounds__(DWI_T) void k_dw_i8_q(const DwiArgs a, const DwiQArgs q) {
  TO* __restrict__ o = (TO*)q.out;
  const float alpha = q.oab[0], beta = q.oab[1];
  dw_i8_body<ST>(a, [&](int64_t off, const float* v, int cg) {
    float lv[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      uqs_requant4<ACT>(q.ss + cg * 16 + 4 * i, q.ss + a.C + cg * 16 + 4 * i, v + 4 * i, lv + 4 * i, alpha, beta, q.ko);
    UqsStore<TO, 16>::run(o + off, lv, alpha, beta, q.ko);
  });
}

extern "C" int pf_dw_i8_supported(int C, int k, int stride);

extern "C" int pf_dw_i8_fwd_q(const uint8_t* x, const uint32_t* w_cols, const float* w_scale_beta, const float* act_alpha_beta,
                              int act_bits, const float* out_scale_shift, int out_act, const float* out_alpha_beta, int out_bits,
                              void* out, int out_kind, int B, int H, int W, int C, int stride, int pad_h, int pad_w, int Ho, int Wo,
                              void* stream) {
  if (!pf_dw_i8_supported(C, 3, stride)) return (int)hipErrorInvalidValue;
  if (!pf_static_out_ok(true, out_kind, out_bits, out_act, out, out_scale_shift, out_alpha_beta)) return (int)hipErrorInvalidValue;
  DwiArgs a;
  dim3 grid;
  const int err = dwi_setup(a, grid, x, w_cols, w_scale_beta, act_alpha_beta, act_bits, B, H, W, C, stride, pad_h, pad_w, Ho, Wo);
  if (err) return err;
  DwiQArgs q;
  q.ss = out_scale_shift; q.oab = out_alpha_beta; q.out = out; q.ko = uq_k_of_bits(out_bits);
  hipStream_t st = (hipStream_t)stream;
  pf_with_out_kind(out_kind, [&](auto* o) {
    using TO = std::remove_pointer_t<decltype(o)>;
    pf_with_act(out_act, [&](auto A) {
      if (stride == 1) k_dw_i8_q<TO, 1, decltype(A)::value><<<grid, DWI_T, 0, st>>>(a, q);
      else k_dw_i8_q<TO, 2, decltype(A)::value><<<grid, DWI_T, 0, st>>>(a, q);
    });
  });
  PF_LAUNCH_CHECK();
  return 0;
}
