// Int8 inference of a uniformly quantised convolution on the i8 matrix cores (v_mfma_i32_16x16x64_i8).
//
// The learner's quantiser (learners/uniform_quantization/utils.py:163-245 under /root/reference) leaves every quantised operand as
// UNSIGNED codes on an affine grid: activation a = beta_a + alpha_a * c / k_a (one pair per tensor, recalibrated per batch, on the
// device), weight w[n][j] = beta_w[n] + alpha_w[n] * d[n][j] / k_w.  The convolution of the decoded operands is therefore
//
//   y[m][n] = (alpha_a/k_a)(alpha_w[n]/k_w) P + (alpha_a/k_a) beta_w[n] Sc + beta_a ((alpha_w[n]/k_w) Dv + beta_w[n] V)
//   P = sum_window c d,  Sc = sum_window c   (padding taps hold code 0),  Dv = sum over the VALID taps of d[n],  V = valid taps * C
//
// with P and Sc exact integers.  The matrix instruction takes SIGNED bytes, so the kernel multiplies s = c - 128 and t = d - 128:
//   P = sum s t + 128 sum s + 128 sum_all t[n] + 16384 K,   Sc = sum s + 128 K,   K = R S C,
// padding taps held as s = -128 and the tail of the last 64-wide K step as s = t = 0.  sum s per output pixel comes out of the same
// loop as a product with an all-ones fragment; sum_all t[n] and the per-tap sums of d are tables made when the layer is packed.
//
// pf_bn_act_quant_codes is the producer: the twin of pf_bn_act_quant_apply (pf_bn.hip) that stores the code instead of the value.
#include "pf_common.h"

// =============================================================================================
// producer: code = rint((act(scale * x + shift) - beta) / alpha * k)
// =============================================================================================
// Same arithmetic, in the same order, as k_bn_apply + uq_point up to the rounding decision rintf(xn * k); what uq_point goes on to
// compute from it, alpha * (code / k) + beta, is what the consumer's formula expands.  The clamp to [0, k] never acts on a slot
// calibrated on this tensor (0 <= xn <= 1); it keeps a foreign slot from wrapping a byte.
__device__ __forceinline__ uint32_t uq_code(float t, float alpha, float beta, float k) {
  const float xn = (t - beta) / alpha;
  return (uint32_t)fminf(fmaxf(rintf(xn * k), 0.0f), k);
}

static inline bool codes_fast_ok(int C) { return pf_vec8_ok(C); }   // the thread -> (row, 8 channels) map of k_bn_apply

template <typename T, int ACT, bool FAST>
__global__ __launch_bounds__(PF_THREADS) void k_bn_codes(const T* __restrict__ x, uint8_t* __restrict__ codes, int64_t rows, int C,
                                                         const float* __restrict__ scale_shift,
                                                         const uint32_t* __restrict__ slot, float k,
                                                         float* __restrict__ alpha_beta) {
  float alpha, beta;
  slot_alpha_beta(slot, alpha, beta);
  if (blockIdx.x == 0 && threadIdx.x == 0) { alpha_beta[0] = alpha; alpha_beta[1] = beta; }
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
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lo |= uq_code(apply_act<ACT>(fmaf(sc[j], v[j], sh[j])), alpha, beta, k) << (8 * j);
        hi |= uq_code(apply_act<ACT>(fmaf(sc[j + 4], v[j + 4], sh[j + 4])), alpha, beta, k) << (8 * j);
      }
      *reinterpret_cast<uint2*>(codes + off) = make_uint2(lo, hi);
    }
  } else {
    const int64_t n = rows * C;
    for (int64_t e = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * PF_THREADS) {
      const int c = (int)(e % C);
      const float y = apply_act<ACT>(fmaf(scale_shift[c], load_one<T>(x + e), scale_shift[C + c]));
      codes[e] = (uint8_t)uq_code(y, alpha, beta, k);
    }
  }
}

template <typename T>
static int launch_bn_codes(const T* x, uint8_t* codes, int64_t rows, int C, const float* ss, int act, const uint32_t* slot, float k,
                           float* alpha_beta, hipStream_t st) {
  const bool fast = codes_fast_ok(C) && pf_aligned16(x) && (((uintptr_t)codes) & 7) == 0;
  const int grid = fast ? pf_grid_for(rows, (PF_THREADS / (C / 8)) * 2) : pf_grid_for(rows * C, PF_THREADS * 4);
  pf_with_act(act, [&](auto A) {
    pf_with_bool(fast, [&](auto F) {
      k_bn_codes<T, decltype(A)::value, decltype(F)::value><<<grid, PF_THREADS, 0, st>>>(x, codes, rows, C, ss, slot, k, alpha_beta);
    });
  });
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_bn_act_quant_codes(const void* x, uint8_t* codes, int dtype, int64_t rows, int C, const float* scale_shift, int act,
                                     const uint32_t* slot, int bits, float* alpha_beta, void* stream) {
  if (rows <= 0 || C <= 0 || bits < 1 || bits > 8 || slot == nullptr || alpha_beta == nullptr || scale_shift == nullptr)
    return (int)hipErrorInvalidValue;
  const float k = uq_k_of_bits(bits);
  if (dtype == PF_F32)
    return launch_bn_codes<float>((const float*)x, codes, rows, C, scale_shift, act, slot, k, alpha_beta, (hipStream_t)stream);
  if (dtype == PF_BF16)
    return launch_bn_codes<bf16_t>((const bf16_t*)x, codes, rows, C, scale_shift, act, slot, k, alpha_beta, (hipStream_t)stream);
  return (int)hipErrorInvalidValue;
}

// the consumer (pf_conv_i8.h: implicit GEMM over K = R S C bytes on v_mfma_i32_16x16x64_i8): one rounding to the output type
#include "pf_conv_i8.h"

template <typename TO>
__global__ __launch_bounds__(PF_THREADS) void k_conv_i8(const I8Args a) {
  TO* __restrict__ y = (TO*)a.y;
  conv_i8_body<TO>(a, [&](int64_t m, int n0, const float* v) { i8_store4<TO>(y + m * a.N + n0, v); });
}

extern "C" int pf_conv_i8_supported(int C, int N, int R, int S, int stride) {
  if (C <= 0 || N <= 0 || R <= 0 || S <= 0 || (stride != 1 && stride != 2)) return 0;
  if (C % 16 || N % 8) return 0;
  return (int64_t)R * S * C * 16384 < ((int64_t)1 << 31) ? 1 : 0;      // the int32 accumulator holds sum s t
}

extern "C" int pf_conv_i8_fwd(const uint8_t* x, const int8_t* w, const float* act_alpha_beta, int act_bits, const float* w_scale_beta,
                              const int32_t* w_tsum, const int32_t* w_tapsum, const void* res, void* y, int out_dtype, int imgs, int H,
                              int W, int C, int N, int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream) {
  if (y == nullptr || !pf_aligned16(y) || !pf_aligned16(res)) return (int)hipErrorInvalidValue;
  I8Args a;
  dim3 grid;
  const int err = i8_setup(a, grid, x, w, act_alpha_beta, act_bits, w_scale_beta, w_tsum, w_tapsum, imgs, H, W, C, N, R, S, stride, pad_h,
                           pad_w, Ho, Wo);
  if (err) return err;
  a.res = res; a.y = y;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == PF_F32) k_conv_i8<float><<<grid, PF_THREADS, 0, st>>>(a);
  else if (out_dtype == PF_BF16) k_conv_i8<bf16_t><<<grid, PF_THREADS, 0, st>>>(a);
  else return (int)hipErrorInvalidValue;
  PF_LAUNCH_CHECK();
  return 0;
}
