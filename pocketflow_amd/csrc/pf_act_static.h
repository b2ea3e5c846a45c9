// The STATIC activation quantiser: quantisation against a range that was calibrated once and travels with the
// artefact, instead of the per-batch range of uq_point / uq_code.  Shared by the stand-alone pass (pf_act_static.hip) and by the
// requantising epilogues of the kernels on codes (pf_conv_i8_q.hip, pf_depthwise_i8_q.hip).
//
//   t = ((u - beta) / alpha) * k;   t = min(max(t, 0), k);   level = rint(t);   value = alpha * (level / k) + beta
//
// The chain of uq_code / uq_point plus ONE clamp, in front of the rounding: a value outside the calibrated range takes the end
// level.  On a range calibrated on the tensor itself 0 <= t <= k holds already, the clamp does not act and the levels are those of
// the per-batch kernels bit for bit.  (alpha, beta) are read from a device pair, as a slot decodes: never by the host.
#pragma once
#include "pf_common.h"

#define PF_OUT_CODES 0   // uint8 level
#define PF_OUT_F32 1     // fake-quantised value, float32
#define PF_OUT_BF16 2    // fake-quantised value, bf16

__device__ __forceinline__ float uqs_level(float u, float alpha, float beta, float k) {
  float t = ((u - beta) / alpha) * k;
  t = fminf(fmaxf(t, 0.0f), k);
  return rintf(t);
}
__device__ __forceinline__ float uqs_value(float level, float alpha, float beta, float k) {
  return alpha * (level / k) + beta;           // multiply, then add: two roundings, as uq_point
}

// the requantising step of the kernels on codes, four channels at a time: lv = the levels of act(scale * v + shift); scale / shift
// point at the four channels' entries of the folded BatchNorm table (16-byte aligned)
template <int ACT>
__device__ __forceinline__ void uqs_requant4(const float* scale, const float* shift, const float* v, float* lv, float alpha, float beta,
                                             float k) {
  const float4 sc = *reinterpret_cast<const float4*>(scale);
  const float4 sh = *reinterpret_cast<const float4*>(shift);
  lv[0] = uqs_level(apply_act<ACT>(fmaf(sc.x, v[0], sh.x)), alpha, beta, k);
  lv[1] = uqs_level(apply_act<ACT>(fmaf(sc.y, v[1], sh.y)), alpha, beta, k);
  lv[2] = uqs_level(apply_act<ACT>(fmaf(sc.z, v[2], sh.z)), alpha, beta, k);
  lv[3] = uqs_level(apply_act<ACT>(fmaf(sc.w, v[3], sh.w)), alpha, beta, k);
}

// N consecutive channels of one pixel, given as levels, stored as the output kind TO: uint8_t = codes (N bytes, one vector store of
// N bytes), float / bf16_t = values.  p is aligned to the vector it takes (N bytes of codes, 16 bytes of float32, 2 N bytes of bf16).
template <typename TO, int N> struct UqsStore;
template <int N> struct UqsStore<uint8_t, N> {
  static __device__ __forceinline__ void run(uint8_t* p, const float* lv, float, float, float) {
    uint32_t w[N / 4];
#pragma unroll
    for (int i = 0; i < N / 4; ++i)
      w[i] = (uint32_t)lv[4 * i] | ((uint32_t)lv[4 * i + 1] << 8) | ((uint32_t)lv[4 * i + 2] << 16) | ((uint32_t)lv[4 * i + 3] << 24);
    if constexpr (N == 4) *reinterpret_cast<uint32_t*>(p) = w[0];
    else if constexpr (N == 8) *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    else *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <int N> struct UqsStore<float, N> {
  static __device__ __forceinline__ void run(float* p, const float* lv, float alpha, float beta, float k) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i)
      *reinterpret_cast<float4*>(p + 4 * i) = make_float4(uqs_value(lv[4 * i], alpha, beta, k), uqs_value(lv[4 * i + 1], alpha, beta, k),
                                                          uqs_value(lv[4 * i + 2], alpha, beta, k), uqs_value(lv[4 * i + 3], alpha, beta, k));
  }
};
template <int N> struct UqsStore<bf16_t, N> {
  static __device__ __forceinline__ void run(bf16_t* p, const float* lv, float alpha, float beta, float k) {
    uint32_t w[N / 2];
#pragma unroll
    for (int i = 0; i < N / 2; ++i)
      w[i] = (uint32_t)f32_to_bf16(uqs_value(lv[2 * i], alpha, beta, k)) | ((uint32_t)f32_to_bf16(uqs_value(lv[2 * i + 1], alpha, beta, k)) << 16);
    if constexpr (N == 4) *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    else {
#pragma unroll
      for (int i = 0; i < N / 8; ++i) *reinterpret_cast<uint4*>(p + 8 * i) = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
  }
};

// host: out_kind -> f(type tag); returns false for an unknown kind
template <typename F> static inline bool pf_with_out_kind(int out_kind, F&& f) {
  if (out_kind == PF_OUT_CODES) f((uint8_t*)nullptr);
  else if (out_kind == PF_OUT_F32) f((float*)nullptr);
  else if (out_kind == PF_OUT_BF16) f((bf16_t*)nullptr);
  else return false;
  return true;
}
// host: what every static entry checks of its output side.  `epilogue`: a kernel on codes, whose lanes store whole vectors (out and
// scale_shift 16-byte aligned), which has at most 8 bits for every output kind and no instantiation for an unknown activation.  The
// stand-alone pass takes up to 32 bits for a value output and any alignment (its scalar loop); an unknown activation there is none.
static inline bool pf_static_out_ok(bool epilogue, int out_kind, int out_bits, int out_act, const void* out, const float* scale_shift,
                                    const float* out_alpha_beta) {
  if (out == nullptr || scale_shift == nullptr || out_alpha_beta == nullptr) return false;
  if (out_kind != PF_OUT_CODES && out_kind != PF_OUT_F32 && out_kind != PF_OUT_BF16) return false;
  if (out_bits < 1 || out_bits > (epilogue || out_kind == PF_OUT_CODES ? 8 : 32)) return false;
  if (!epilogue) return true;
  if (out_act != PF_ACT_NONE && out_act != PF_ACT_RELU && out_act != PF_ACT_RELU6) return false;
  return pf_aligned16(out) && pf_aligned16(scale_shift);
}
static inline bool pf_out_aligned(int out_kind, const void* p, int n) {   // n consecutive channels per vector store
  const uintptr_t bytes = out_kind == PF_OUT_CODES ? (uintptr_t)n : out_kind == PF_OUT_F32 ? 16u : (uintptr_t)(2 * n > 16 ? 16 : 2 * n);
  return (((uintptr_t)p) & (bytes - 1)) == 0;
}
