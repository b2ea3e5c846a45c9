// Stand-alone BN -> activation -> STATIC quantiser pass: pf_bn_act_quant_apply / pf_bn_act_quant_codes against a range
// that was calibrated once (pf_act_static.h), with the clamp in front of the rounding and no slot: nothing is calibrated, nothing is
// written but the output.  For every quantiser of a graph with fixed ranges whose producer cannot requantise in its own epilogue: the
// stem, residual sums, a float-kernel producer, the network head.
//
// One read of x (float32 / bf16), one write: uint8 codes, or the fake-quantised value in float32 / bf16.  The thread -> (row, 8
// channels) map of k_bn_codes where C % 8 == 0 and C <= 2048 (pf_bn_vector_ok), a scalar loop otherwise.  HBM-bound; no LDS, no
// atomics, deterministic.
#include "pf_act_static.h"

static inline bool static_fast_ok(int C) { return pf_vec8_ok(C); }   // the thread -> (row, 8 channels) map of k_bn_apply / k_bn_codes

template <typename T, typename TO, int ACT, bool FAST>
__global__ __launch_bounds__(PF_THREADS) void k_bn_static(const T* __restrict__ x, TO* __restrict__ out, int64_t rows, int C,
                                                          const float* __restrict__ scale_shift,
                                                          const float* __restrict__ alpha_beta, float k) {
  const float alpha = alpha_beta[0], beta = alpha_beta[1];
  if (FAST) {
    const int G = C >> 3, RPS = PF_THREADS / G;
    const int cg = threadIdx.x % G, rsub = threadIdx.x / G;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = scale_shift[(cg << 3) + j]; sh[j] = scale_shift[C + (cg << 3) + j]; }
#pragma unroll 2
    for (int64_t r = pf_vec8_first_row(rsub, RPS, rows); r < rows; r += (int64_t)gridDim.x * RPS) {
      float v[8];
      const int64_t off = r * C + (cg << 3);
      load8<T>(x + off, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = uqs_level(apply_act<ACT>(fmaf(sc[j], v[j], sh[j])), alpha, beta, k);
      UqsStore<TO, 8>::run(out + off, v, alpha, beta, k);
    }
  } else {
    const int64_t n = rows * C;
    for (int64_t e = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * PF_THREADS) {
      const int c = (int)(e % C);
      const float lv = uqs_level(apply_act<ACT>(fmaf(scale_shift[c], load_one<T>(x + e), scale_shift[C + c])), alpha, beta, k);
      if (sizeof(TO) == 1) out[e] = (TO)lv;
      else if (sizeof(TO) == 4) out[e] = (TO)uqs_value(lv, alpha, beta, k);
      else out[e] = (TO)f32_to_bf16(uqs_value(lv, alpha, beta, k));
    }
  }
}

template <typename T>
static int launch_bn_static(const T* x, void* out, int out_kind, int64_t rows, int C, const float* ss, int act, const float* ab, float k,
                            hipStream_t st) {
  const bool fast = static_fast_ok(C) && pf_aligned16(x) && pf_out_aligned(out_kind, out, 8);
  const int grid = fast ? pf_grid_for(rows, (PF_THREADS / (C / 8)) * 2) : pf_grid_for(rows * C, PF_THREADS * 4);
  const bool known = pf_with_out_kind(out_kind, [&](auto* o) {
    using TO = std::remove_pointer_t<decltype(o)>;
    pf_with_act(act, [&](auto A) {
      pf_with_bool(fast, [&](auto F) {
        k_bn_static<T, TO, decltype(A)::value, decltype(F)::value><<<grid, PF_THREADS, 0, st>>>(x, (TO*)out, rows, C, ss, ab, k);
      });
    });
  });
  if (!known) return (int)hipErrorInvalidValue;
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_bn_act_quant_static(const void* x, void* out, int dtype, int out_kind, int64_t rows, int C, const float* scale_shift,
                                      int act, const float* out_alpha_beta, int bits, void* stream) {
  if (rows <= 0 || C <= 0 || x == nullptr || !pf_static_out_ok(false, out_kind, bits, act, out, scale_shift, out_alpha_beta))
    return (int)hipErrorInvalidValue;
  const float k = uq_k_of_bits(bits);
  if (dtype == PF_F32)
    return launch_bn_static<float>((const float*)x, out, out_kind, rows, C, scale_shift, act, out_alpha_beta, k, (hipStream_t)stream);
  if (dtype == PF_BF16)
    return launch_bn_static<bf16_t>((const bf16_t*)x, out, out_kind, rows, C, scale_shift, act, out_alpha_beta, k, (hipStream_t)stream);
  return (int)hipErrorInvalidValue;
}
