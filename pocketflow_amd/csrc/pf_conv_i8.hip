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

static inline bool codes_fast_ok(int C) {     // the thread -> (row, 8 channels) map of k_bn_apply
  if (C % 8) return false;
  const int G = C / 8;
  return G <= PF_THREADS && (PF_THREADS % G) == 0;
}

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
    for (int64_t r = (int64_t)blockIdx.x * RPS + rsub; r < rows; r += (int64_t)gridDim.x * RPS) {
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

// =============================================================================================
// consumer: implicit GEMM, [N channels] x [M output pixels] over K = R S C bytes
// =============================================================================================
// A workgroup of four wavefronts owns I8_BM = 128 output pixels x I8_BN = 64 output channels; a wavefront 32 pixels x 64 channels
// (4 x 2 tiles of 16 x 16).  The WEIGHTS are the instruction's A operand and the pixels its B operand, so an accumulator lane holds
// four consecutive output channels of one pixel: one 16-byte (float32) or 8-byte (bf16) store, and everything per pixel -- the code
// sum, the valid taps -- is per lane.  A lane's 16-byte fragment is row (lane & 15), bytes 16 (lane >> 4) .. + 15 of the 64-byte K
// step for both operands; the products are summed over the whole step, so the order of k inside it is immaterial as long as both
// operands share it.
// One K step per iteration: global -> registers (next step) overlaps the MFMAs of the current one; registers -> LDS between two
// barriers.  LDS rows are 80 bytes apart (64 + 16): the 16 rows a quarter-wave reads with ds_read_b128 then fall into 16 distinct
// groups of four banks.
#define I8_BM 128
#define I8_BN 64
#define I8_BK 64
#define I8_LDS_ROW 80

typedef int i8x16_t __attribute__((ext_vector_type(4)));   // 16 signed bytes: one fragment
typedef int i32x4_t __attribute__((ext_vector_type(4)));

struct I8Args {
  const uint8_t* x;         // [imgs][H][W][C] codes
  const int8_t* w;          // [N][Kp] signed weights t = d - 128, zero beyond K
  const float* ab;          // (alpha_a, beta_a)
  const float* wtab;        // [N][2] (alpha_w / k_w, beta_w)
  const int32_t* tsum;      // [N] sum over the window of t
  const int32_t* dtap;      // [N][R*S] per-tap sums of d
  const void* res;
  void* y;
  int imgs, H, W, C, N, R, S, stride, pad_h, pad_w, Ho, Wo;
  int K, Kp;
  int64_t M;
  float ka;
};

template <typename TO> __device__ __forceinline__ void i8_load4(const TO* p, float* v);
template <> __device__ __forceinline__ void i8_load4<float>(const float* p, float* v) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <> __device__ __forceinline__ void i8_load4<bf16_t>(const bf16_t* p, float* v) {
  const uint2 t = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xFFFF0000u);
  v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xFFFF0000u);
}
template <typename TO> __device__ __forceinline__ void i8_store4(TO* p, const float* v);
template <> __device__ __forceinline__ void i8_store4<float>(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void i8_store4<bf16_t>(bf16_t* p, const float* v) {
  uint2 o;
  o.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
  o.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
  *reinterpret_cast<uint2*>(p) = o;
}

// the 16 bytes of pixel row (ih0, iw0) + tap, channels c0 .. c0 + 15, as signed s = c - 128; a tap outside the image is code 0
__device__ __forceinline__ uint4 i8_load_x(const I8Args& a, bool row_ok, int img, int ih0, int iw0, int kk) {
  if (kk >= a.K) return make_uint4(0u, 0u, 0u, 0u);               // tail of the last K step: s = 0
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (row_ok) {
    const int tap = kk / a.C, c0 = kk - tap * a.C;
    const int r = tap / a.S, s = tap - r * a.S;
    const int ih = ih0 + r, iw = iw0 + s;
    if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
      v = *reinterpret_cast<const uint4*>(a.x + (((int64_t)img * a.H + ih) * a.W + iw) * a.C + c0);
  }
  v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
  return v;
}

template <typename TO>
__global__ __launch_bounds__(PF_THREADS) void k_conv_i8(const I8Args a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_w[I8_BN * I8_LDS_ROW];
  __shared__ __attribute__((aligned(16))) uint8_t s_x[I8_BM * I8_LDS_ROW];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t m_blk = (int64_t)blockIdx.x * I8_BM;
  const int n_blk = blockIdx.y * I8_BN;

  // staging map: thread -> 16-byte chunk (tid & 3) of weight row (tid >> 2) and of pixel rows (tid >> 2), (tid >> 2) + 64
  const int st_row = tid >> 2, st_q = (tid & 3) << 4;
  const bool w_ok = n_blk + st_row < a.N;
  const int8_t* w_src = a.w + (int64_t)(n_blk + st_row) * a.Kp + st_q;
  bool x_ok[2];
  int x_img[2], x_ih0[2], x_iw0[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t m = m_blk + st_row + 64 * h;
    x_ok[h] = m < a.M;
    const int64_t mm = x_ok[h] ? m : 0;
    const int hw = a.Ho * a.Wo;
    x_img[h] = (int)(mm / hw);
    const int rem = (int)(mm - (int64_t)x_img[h] * hw);
    const int oh = rem / a.Wo;
    x_ih0[h] = oh * a.stride - a.pad_h;
    x_iw0[h] = (rem - oh * a.Wo) * a.stride - a.pad_w;
  }

  i32x4_t acc[4][2], accs[2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (i32x4_t){0, 0, 0, 0};
  accs[0] = accs[1] = (i32x4_t){0, 0, 0, 0};
  const i8x16_t ones = (i8x16_t){0x01010101, 0x01010101, 0x01010101, 0x01010101};

  uint4 gw = make_uint4(0u, 0u, 0u, 0u), gx[2];
  if (w_ok) gw = *reinterpret_cast<const uint4*>(w_src);
  gx[0] = i8_load_x(a, x_ok[0], x_img[0], x_ih0[0], x_iw0[0], st_q);
  gx[1] = i8_load_x(a, x_ok[1], x_img[1], x_ih0[1], x_iw0[1], st_q);

  const int f_off = (lane & 15) * I8_LDS_ROW + ((lane >> 4) << 4);     // this lane's fragment inside a 16-row tile
  for (int k0 = 0; k0 < a.Kp; k0 += I8_BK) {
    __syncthreads();                                                  // the previous step's fragments are read
    *reinterpret_cast<uint4*>(s_w + st_row * I8_LDS_ROW + st_q) = gw;
    *reinterpret_cast<uint4*>(s_x + st_row * I8_LDS_ROW + st_q) = gx[0];
    *reinterpret_cast<uint4*>(s_x + (st_row + 64) * I8_LDS_ROW + st_q) = gx[1];
    __syncthreads();
    const int kn = k0 + I8_BK;
    if (kn < a.Kp) {
      if (w_ok) gw = *reinterpret_cast<const uint4*>(w_src + kn);
      gx[0] = i8_load_x(a, x_ok[0], x_img[0], x_ih0[0], x_iw0[0], kn + st_q);
      gx[1] = i8_load_x(a, x_ok[1], x_img[1], x_ih0[1], x_iw0[1], kn + st_q);
    }
    i8x16_t fx[2], fw[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) fx[j] = *reinterpret_cast<const i8x16_t*>(s_x + (wave * 32 + j * 16) * I8_LDS_ROW + f_off);
#pragma unroll
    for (int i = 0; i < 4; ++i) fw[i] = *reinterpret_cast<const i8x16_t*>(s_w + (i * 16) * I8_LDS_ROW + f_off);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fw[i], fx[j], acc[i][j], 0, 0, 0);
      accs[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, fx[j], accs[j], 0, 0, 0);
    }
  }

  // ---- epilogue.  Accumulator element (i, j, e): channel n_blk + 16 i + 4 (lane >> 4) + e, pixel m_blk + 32 wave + 16 j + (lane & 15)
  const float alpha_a = a.ab[0], beta_a = a.ab[1];
  const float sa = alpha_a / a.ka;
  const int taps = a.R * a.S;
  TO* __restrict__ y = (TO*)a.y;
  const TO* __restrict__ res = (const TO*)a.res;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t m = m_blk + wave * 32 + j * 16 + (lane & 15);
    if (m >= a.M) continue;
    const int ssum = accs[j][0];                                      // sum of s over the window (every row of the ones product)
    const int sc_sum = ssum + 128 * a.K;                              // Sc
    const long long p_pix = 128ll * ssum + 16384ll * a.K;
    // valid taps of this pixel (only read when beta_a != 0)
    int ih0 = 0, iw0 = 0;
    if (beta_a != 0.0f) {
      const int hw = a.Ho * a.Wo;
      const int rem = (int)(m % hw);
      const int oh = rem / a.Wo;
      ih0 = oh * a.stride - a.pad_h;
      iw0 = (rem - oh * a.Wo) * a.stride - a.pad_w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n0 = n_blk + i * 16 + ((lane >> 4) << 2);
      if (n0 >= a.N) continue;                                        // N % 4 == 0: a lane's four channels are in or out together
      float v[4], r4[4];
      if (res != nullptr) i8_load4<TO>(res + m * a.N + n0, r4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + e;
        const float sw = a.wtab[2 * n], bw = a.wtab[2 * n + 1];
        const long long P = (long long)acc[i][j][e] + p_pix + 128ll * a.tsum[n];
        float out = (sa * sw) * (float)P + (sa * bw) * (float)sc_sum;
        if (beta_a != 0.0f) {
          long long dv = 0;
          int nvalid = 0;
          for (int t = 0; t < taps; ++t) {
            const int r = t / a.S, s = t - r * a.S;
            const int ih = ih0 + r, iw = iw0 + s;
            if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) { dv += a.dtap[(int64_t)n * taps + t]; ++nvalid; }
          }
          out += beta_a * (sw * (float)dv + bw * (float)(nvalid * a.C));
        }
        if (res != nullptr) out += r4[e];
        v[e] = out;
      }
      i8_store4<TO>(y + m * a.N + n0, v);
    }
  }
}

extern "C" int pf_conv_i8_supported(int C, int N, int R, int S, int stride) {
  if (C <= 0 || N <= 0 || R <= 0 || S <= 0 || (stride != 1 && stride != 2)) return 0;
  if (C % 16 || N % 8) return 0;
  return (int64_t)R * S * C * 16384 < ((int64_t)1 << 31) ? 1 : 0;      // the int32 accumulator holds sum s t
}

extern "C" int pf_conv_i8_fwd(const uint8_t* x, const int8_t* w, const float* act_alpha_beta, int act_bits, const float* w_scale_beta,
                              const int32_t* w_tsum, const int32_t* w_tapsum, const void* res, void* y, int out_dtype, int imgs, int H,
                              int W, int C, int N, int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream) {
  if (!pf_conv_i8_supported(C, N, R, S, stride) || imgs <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || pad_h < 0 || pad_w < 0)
    return (int)hipErrorInvalidValue;
  if (act_bits < 1 || act_bits > 8 || x == nullptr || w == nullptr || act_alpha_beta == nullptr || w_scale_beta == nullptr ||
      w_tsum == nullptr || w_tapsum == nullptr || y == nullptr)
    return (int)hipErrorInvalidValue;
  if ((int64_t)(Ho - 1) * stride + R - 2 * pad_h > H || (int64_t)(Wo - 1) * stride + S - 2 * pad_w > W) return (int)hipErrorInvalidValue;
  if (!pf_aligned16(x) || !pf_aligned16(w) || !pf_aligned16(y) || !pf_aligned16(res)) return (int)hipErrorInvalidValue;
  I8Args a;
  a.x = x; a.w = w; a.ab = act_alpha_beta; a.wtab = w_scale_beta; a.tsum = w_tsum; a.dtap = w_tapsum; a.res = res; a.y = y;
  a.imgs = imgs; a.H = H; a.W = W; a.C = C; a.N = N; a.R = R; a.S = S; a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w;
  a.Ho = Ho; a.Wo = Wo;
  a.K = R * S * C;
  a.Kp = (a.K + I8_BK - 1) / I8_BK * I8_BK;
  a.M = (int64_t)imgs * Ho * Wo;
  a.ka = uq_k_of_bits(act_bits);
  const int64_t gx = (a.M + I8_BM - 1) / I8_BM;
  if (gx > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)((N + I8_BN - 1) / I8_BN));
  if (grid.y > 65535u) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == PF_F32) k_conv_i8<float><<<grid, PF_THREADS, 0, st>>>(a);
  else if (out_dtype == PF_BF16) k_conv_i8<bf16_t><<<grid, PF_THREADS, 0, st>>>(a);
  else return (int)hipErrorInvalidValue;
  PF_LAUNCH_CHECK();
  return 0;
}
