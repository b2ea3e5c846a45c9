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
    const float4 sc = *reinterpret_cast<const float4*>(q.ss + n0);
    const float4 sh = *reinterpret_cast<const float4*>(q.ss + a.N + n0);
    float lv[4];
    lv[0] = uqs_level(apply_act<ACT>(fmaf(sc.x, v[0], sh.x)), alpha, beta, q.ko);
    lv[1] = uqs_level(apply_act<ACT>(fmaf(sc.y, v[1], sh.y)), alpha, beta, q.ko);
    lv[2] = uqs_level(apply_act<ACT>(fmaf(sc.z, v[2], sh.z)), alpha, beta, q.ko);
    lv[3] = uqs_level(apply_act<ACT>(fmaf(sc.w, v[3], sh.w)), alpha, beta, q.ko);
    UqsStore<TO, 4>::run(o + m * a.N + n0, lv, alpha, beta, q.ko);
  });
}

extern "C" int pf_conv_i8_supported(int C, int N, int R, int S, int stride);

extern "C" int pf_conv_i8_fwd_q(const uint8_t* x, const int8_t* w, const float* act_alpha_beta, int act_bits, const float* w_scale_beta,
                                const int32_t* w_tsum, const int32_t* w_tapsum, const void* res, const float* out_scale_shift, int out_act,
                                const float* out_alpha_beta, int out_bits, void* out, int out_kind, int imgs, int H, int W, int C, int N,
                                int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream) {
  if (!pf_conv_i8_supported(C, N, R, S, stride) || imgs <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || pad_h < 0 || pad_w < 0)
    return (int)hipErrorInvalidValue;
  if (res != nullptr) return (int)hipErrorInvalidValue;            // a residual sum has no single consumer to requantise for
  if (act_bits < 1 || act_bits > 8 || x == nullptr || w == nullptr || act_alpha_beta == nullptr || w_scale_beta == nullptr ||
      w_tsum == nullptr || w_tapsum == nullptr || out == nullptr || out_scale_shift == nullptr || out_alpha_beta == nullptr)
    return (int)hipErrorInvalidValue;
  if (out_kind != PF_OUT_CODES && out_kind != PF_OUT_F32 && out_kind != PF_OUT_BF16) return (int)hipErrorInvalidValue;
  if (out_bits < 1 || out_bits > 8) return (int)hipErrorInvalidValue;
  if (out_act != PF_ACT_NONE && out_act != PF_ACT_RELU && out_act != PF_ACT_RELU6) return (int)hipErrorInvalidValue;
  if ((int64_t)(Ho - 1) * stride + R - 2 * pad_h > H || (int64_t)(Wo - 1) * stride + S - 2 * pad_w > W) return (int)hipErrorInvalidValue;
  if (!pf_aligned16(x) || !pf_aligned16(w) || !pf_aligned16(out) || !pf_aligned16(out_scale_shift)) return (int)hipErrorInvalidValue;
  I8Args a;
  a.x = x; a.w = w; a.ab = act_alpha_beta; a.wtab = w_scale_beta; a.tsum = w_tsum; a.dtap = w_tapsum; a.res = nullptr; a.y = nullptr;
  a.imgs = imgs; a.H = H; a.W = W; a.C = C; a.N = N; a.R = R; a.S = S; a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w;
  a.Ho = Ho; a.Wo = Wo;
  a.K = R * S * C;
  a.Kp = (a.K + I8_BK - 1) / I8_BK * I8_BK;
  a.M = (int64_t)imgs * Ho * Wo;
  a.ka = uq_k_of_bits(act_bits);
  I8QArgs q;
  q.ss = out_scale_shift; q.oab = out_alpha_beta; q.out = out; q.ko = uq_k_of_bits(out_bits);
  const int64_t gx = (a.M + I8_BM - 1) / I8_BM;
  if (gx > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)((N + I8_BN - 1) / I8_BN));
  if (grid.y > 65535u) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  pf_with_out_kind(out_kind, [&](auto* o) {
    using TO = std::remove_pointer_t<decltype(o)>;
    pf_with_act(out_act, [&](auto A) { k_conv_i8_q<TO, decltype(A)::value><<<grid, PF_THREADS, 0, st>>>(a, q); });
  });
  PF_LAUNCH_CHECK();
  return 0;
}
