// The kernel on activation CODES of pf_conv_i8.hip, shared with its requantising sibling (pf_conv_i8_q.hip): the operand structs, the
// main loop and the epilogue up to the float32 value of every output.  What happens to that value -- one rounding to the output type
// (k_conv_i8), or the consumer's BatchNorm + activation + static quantiser (k_conv_i8_q) -- is the caller's `emit`.
#pragma once
#include "pf_common.h"

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

// TO: the type of the residual (a.res, may be null).  emit(m, n0, v): the four float32 outputs of pixel m, channels n0 .. n0 + 3.
template <typename TO, typename Emit>
__device__ __forceinline__ void conv_i8_body(const I8Args& a, Emit&& emit) {
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
      emit(m, n0, v);
    }
  }
}

// ---- host side: checks, operands and launch geometry shared by the entries (residual and output are each entry's own) ------------
extern "C" int pf_conv_i8_supported(int C, int N, int R, int S, int stride);

static inline int i8_setup(I8Args& a, dim3& grid, const uint8_t* x, const int8_t* w, const float* act_alpha_beta, int act_bits,
                           const float* w_scale_beta, const int32_t* w_tsum, const int32_t* w_tapsum, int imgs, int H, int W, int C,
                           int N, int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo) {
  if (!pf_conv_i8_supported(C, N, R, S, stride) || imgs <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || pad_h < 0 || pad_w < 0)
    return (int)hipErrorInvalidValue;
  if (act_bits < 1 || act_bits > 8 || x == nullptr || w == nullptr || act_alpha_beta == nullptr || w_scale_beta == nullptr ||
      w_tsum == nullptr || w_tapsum == nullptr)
    return (int)hipErrorInvalidValue;
  // every output window lies inside the symmetrically padded image
  if ((int64_t)(Ho - 1) * stride + R - 2 * pad_h > H || (int64_t)(Wo - 1) * stride + S - 2 * pad_w > W) return (int)hipErrorInvalidValue;
  if (!pf_aligned16(x) || !pf_aligned16(w)) return (int)hipErrorInvalidValue;
  a.x = x; a.w = w; a.ab = act_alpha_beta; a.wtab = w_scale_beta; a.tsum = w_tsum; a.dtap = w_tapsum; a.res = nullptr; a.y = nullptr;
  a.imgs = imgs; a.H = H; a.W = W; a.C = C; a.N = N; a.R = R; a.S = S; a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w;
  a.Ho = Ho; a.Wo = Wo;
  a.K = R * S * C;
  a.Kp = (a.K + I8_BK - 1) / I8_BK * I8_BK;
  a.M = (int64_t)imgs * Ho * Wo;
  a.ka = uq_k_of_bits(act_bits);
  const int64_t gx = (a.M + I8_BM - 1) / I8_BM;
  const int gy = (N + I8_BN - 1) / I8_BN;
  if (gx > 0x7FFFFFFFll || gy > 65535) return (int)hipErrorInvalidValue;
  grid = dim3((unsigned)gx, (unsigned)gy);
  return 0;
}
