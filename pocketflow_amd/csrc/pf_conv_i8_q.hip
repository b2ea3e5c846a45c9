// pf_conv_i8_fwd with a REQUANTISING epilogue: on a graph with fixed activation ranges the one consumer of this
// convolution's output is a quantising BatchNormAct whose range is known before the launch, so the kernel applies that layer itself
// and writes what the NEXT convolution reads -- one byte per element where it multiplies codes, the fake-quantised value otherwise.
// Neither a statistics pass nor an apply pass runs behind it.
//
// Main loop and epilogue up to the float32 output `out` are pf_conv_i8.h's, shared with k_conv_i8: `out` is exactly the value the
// float32 instantiation of that kernel stores.  Then, per element,
//   u = act(fmaf(scale[n], out, shift[n]));   level / value = the static quantiser of pf_act_static.h on (out_alpha, out_beta)
// so the result is, bit for bit, pf_bn_act_quant_static applied to the float32 output of pf_conv_i8_fwd.  A lane's four channels
// are one 4-byte store of codes, one 16-byte store of float32 or one 8-byte store of bf16.
#include "pf_conv_i8.h"
#include "pf_act_static.h"

struct I8QArgs {
  const float* ss;          // [2][N] the consumer BatchNorm folded to scale / shift
  const float* oab;         // (alpha, beta) of the OUTPUT range, on the device
  void* out;                // [imgs][Ho][Wo][N] codes or values
  float ko;                 // 2^out_bits - 1
};

template <typename TO, int ACT>
__global__ __launch_bounds__(PF_THREADS) void k_conv_i8_q(const I8Args a, const I8QArgs q) {
  TO* __restrict__ o = (TO*)q.out;
  const float alpha = q.oab[0], beta = q.oab[1];
  conv_i8_body<float>(a, [&](int64_t m, int n0, const float* v) {
    float lv[4];
    uqs_requant4<ACT>(q.ss + n0, q.ss + a.N + n0, v, lv, alpha, beta, q.ko);
    UqsStore<TO, 4>::run(o + m * a.N + n0, lv, alpha, beta, q.ko);
  });
}

extern "C" int pf_conv_i8_fwd_q(const uint8_t* x, const int8_t* w, const float* act_alpha_beta, int act_bits, const float* w_scale_beta,
                                const int32_t* w_tsum, const int32_t* w_tapsum, const void* res, const float* out_scale_shift, int out_act,
                                const float* out_alpha_beta, int out_bits, void* out, int out_kind, int imgs, int H, int W, int C, int N,
                                int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream) {
  if (res != nullptr) return (int)hipErrorInvalidValue;            // a residual sum has no single consumer to requantise for
  if (!pf_static_out_ok(true, out_kind, out_bits, out_act, out, out_scale_shift, out_alpha_beta)) return (int)hipErrorInvalidValue;
  I8Args a;
  dim3 grid;
  const int err = i8_setup(a, grid, x, w, act_alpha_beta, act_bits, w_scale_beta, w_tsum, w_tapsum, imgs, H, W, C, N, R, S, stride, pad_h,
                           pad_w, Ho, Wo);
  if (err) return err;
  I8QArgs q;
  q.ss = out_scale_shift; q.oab = out_alpha_beta; q.out = out; q.ko = uq_k_of_bits(out_bits);
  hipStream_t st = (hipStream_t)stream;
  pf_with_out_kind(out_kind, [&](auto* o) {
    using TO = std::remove_pointer_t<decltype(o)>;
    pf_with_act(out_act, [&](auto A) { k_conv_i8_q<TO, decltype(A)::value><<<grid, PF_THREADS, 0, st>>>(a, q); });
  });
  PF_LAUNCH_CHECK();
  return 0;
}
