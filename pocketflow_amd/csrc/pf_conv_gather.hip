// Channel-gather convolution: the forward pass of a physically SHRUNK channel-pruned layer (the artefact of
// tools/conversion/export_chn_pruned_model.py; reference tools/conversion/export_chn_pruned_tflite_model.py:236-276 expresses it as
// tf.gather(input, nnz, axis=channel) followed by the smaller convolution).  Inference only.
//
//     Y[m][n] = sum_{tap (r, s)} sum_{j < Ck}  X[pixel(m, r, s)][gather[j]] * Wk[n][r][s][j]        (zero outside the image)
//     then, optionally and in this order:  + bias[n],  + R[m][n],  act(scale[n] * y + shift[n])
//
// X is channels-last with ALL C channels, Wk is KRSC cut along C to the Ck kept channels, gather (int32, strictly ascending, values in
// [0, C)) names them.  The reduction runs over the kept channels only; float32 accumulation; no atomics: one workgroup owns one
// output tile and sums in a fixed order, so results are bit-identical from run to run.
//
// Channel is the innermost index of X, so fetching the kept channels one by one would be a 2-byte gather from HBM.  Instead a
// k-step of BK kept channels [j0, j0 + BK) reads, for every pixel of the tile, the CONTIGUOUS source segment gather[j0] ..
// gather[j0 + BK - 1] in 16-byte vectors (eight lanes per pixel: 128 contiguous bytes per pixel and pass) and COMPACTS while writing
// to LDS: an inverse map inv[c] = j | -1 (int16, built once per workgroup in LDS) sends each loaded element to column j - j0 of
// the tile, or drops it.  A vector that holds no kept channel of the k-step is not loaded at all.  Dropped elements never enter
// LDS or a register that is multiplied: a NaN in a pruned channel cannot reach Y.  Input bytes from HBM therefore do not shrink
// (every cache line that holds one kept channel is read), weight bytes, LDS traffic and multiply work do.
// C % (16 / sizeof(T)) != 0 or an unaligned X (the 3-channel stem): scalar loads of the kept elements, as k_convg does.
//
// bf16: matrix cores.  128 pixels x (64 | 128) output channels per workgroup, 4 wavefronts, each 32 pixels x all columns;
//   __builtin_amdgcn_mfma_f32_16x16x32_bf16 with weights = operand A and pixels = operand B as in pf_conv.hip, so a lane holds 4
//   consecutive output channels of one pixel.  Each tap's Ck is padded with ZERO columns (both operands) to the MFMA depth of 32;
//   tails of pixels / output channels are zero rows that are never stored.  LDS rows are BK + 8 elements (144 bytes): the 16-byte
//   fragment reads of 16 consecutive rows then start 36 banks apart and spread over all 64 banks.
// float32: vector ALUs, 64 x 64 tile, 4 x 4 outputs per thread, one fmaf per term; taps ascending, kept channels ascending within
//   a tap (the order of k_convg over the gathered input).  Tiles are stored [k][row] with 68-float rows so that the inner product
//   reads two float4 per k.
//
// Epilogue: bias, residual and the output affine (a folded inference-mode BatchNorm + activation: act(fmaf(scale, y, shift))) are all
// applied to the float32 accumulators, and the result is rounded to the storage type ONCE.  (The dense MFMA kernels apply their
// folded affine to the value already rounded to bf16, to stay bit-identical with the separate BN pass they replace; a gathered layer
// has no such twin to match, and a second rounding would cost accuracy.)
#include "pf_conv_common.h"

#define GC_T 256
#define GC_MAX_C 8192                 // inverse map: int16[C] in LDS (16 KiB at most)

struct GcArgs {
  const void* X;                      // [imgs][H][W][C]
  const void* Wk;                     // [N][R][S][Ck]
  const int32_t* gather;              // [Ck]
  const float* bias;                  // [N] or null
  const void* Res;                    // [M][N] or null
  const float* oss;                   // scale | shift [2][N] or null
  void* Y;                            // [M][N]
  int act;
  int imgs, H, W, C, Ck, N, R, S, stride, pad_h, pad_w, Ho, Wo;
  int M;
  int xvec, wvec, yvec;               // 16-byte loads along C of X / along Ck of Wk; 4-element stores of Y (and loads of Res)
};

template <typename T> struct GcTile;
template <> struct GcTile<bf16_t> { static constexpr int BM = 128, BK = 64, XLD = 64 + 8, VE = 8; };
template <> struct GcTile<float> { static constexpr int BM = 64, BK = 32, XLD = 64 + 4, VE = 4; };

// tile element (row, k): bf16 [row][k] (MFMA fragments are 8 consecutive k of one row), float32 [k][row]
template <typename T> __device__ __forceinline__ T* gc_at(T* tile, int row, int k);
template <> __device__ __forceinline__ bf16_t* gc_at<bf16_t>(bf16_t* tile, int row, int k) { return tile + row * GcTile<bf16_t>::XLD + k; }
template <> __device__ __forceinline__ float* gc_at<float>(float* tile, int row, int k) { return tile + k * GcTile<float>::XLD + row; }

// one output quadruple: channels n .. n + 3 of pixel m (this lane's accumulators in both layouts)
template <typename T>
__device__ __forceinline__ void gc_epilogue4(const GcArgs& a, int m, int n, float v[4]) {
  if (m >= a.M || n >= a.N) return;
  T* __restrict__ Y = reinterpret_cast<T*>(a.Y);
  const T* __restrict__ Rs = reinterpret_cast<const T*>(a.Res);
  const int64_t o = (int64_t)m * a.N + n;
  const bool full = a.yvec && n + 3 < a.N;
  const int cnt = min(4, a.N - n);
  if (a.bias != nullptr) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) v[e] = v[e] + a.bias[n + e];
  }
  if (Rs != nullptr) {
    if (full) {
      float r[4];
      if (sizeof(T) == 2) {
        const uint2 u = *reinterpret_cast<const uint2*>(Rs + o);
        r[0] = __uint_as_float(u.x << 16); r[1] = __uint_as_float(u.x & 0xFFFF0000u);
        r[2] = __uint_as_float(u.y << 16); r[3] = __uint_as_float(u.y & 0xFFFF0000u);
      } else {
        const float4 u = *reinterpret_cast<const float4*>(Rs + o);
        r[0] = u.x; r[1] = u.y; r[2] = u.z; r[3] = u.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] + r[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) v[e] = v[e] + load_one<T>(Rs + o + e);
    }
  }
  if (a.oss != nullptr) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e >= cnt) break;
      float y = v[e];
      y = fmaf(a.oss[n + e], y, a.oss[a.N + n + e]);
      if (a.act != PF_ACT_NONE) y = fmaxf(y, 0.f);
      if (a.act == PF_ACT_RELU6) y = fminf(y, 6.f);
      v[e] = y;
    }
  }
  if (full) {
    if (sizeof(T) == 2) {
      *reinterpret_cast<uint2*>(Y + o) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    } else {
      *reinterpret_cast<float4*>(Y + o) = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) store_one<T>(Y + o + e, v[e]);
  }
}

// NB: 16-column blocks of the output tile (bf16: 4 | 8; float32: 4)
template <typename T, int NB>
__global__ __launch_bounds__(GC_T) void k_conv_gather(const GcArgs a) {
  typedef GcTile<T> TL;
  constexpr int BM = TL::BM, BK = TL::BK, VE = TL::VE, BN = NB * 16;
  constexpr bool MFMA = sizeof(T) == 2;
  constexpr int XS_ELEMS = MFMA ? BM * TL::XLD : BK * TL::XLD;
  constexpr int WS_ELEMS = MFMA ? BN * TL::XLD : BK * TL::XLD;
  __shared__ __attribute__((aligned(16))) T Xs[XS_ELEMS];
  __shared__ __attribute__((aligned(16))) T Ws[WS_ELEMS];
  __shared__ int p_base[BM], p_h[BM], p_w[BM];                   // pixel of tile row: image * H * W, ho * stride - pad_h, wo * stride - pad_w
  extern __shared__ __attribute__((aligned(16))) unsigned char gc_dyn[];
  int16_t* inv = reinterpret_cast<int16_t*>(gc_dyn);             // [C rounded up to 8]: kept index of a source channel, or -1

  const T* __restrict__ X = reinterpret_cast<const T*>(a.X);
  const T* __restrict__ Wk = reinterpret_cast<const T*>(a.Wk);
  const int tid = threadIdx.x;
  const int tiles_n = (a.N + BN - 1) / BN;
  const int m0 = (blockIdx.x / tiles_n) * BM, n0 = (blockIdx.x % tiles_n) * BN;
  const int RS = a.R * a.S;

  // ---- once per workgroup: inverse map and pixel coordinates ----------------------------------------------------------------
  if (a.xvec) {
    const int Cr = (a.C + 7) & ~7;
    for (int c = tid; c < Cr; c += GC_T) inv[c] = -1;
    __syncthreads();
    for (int j = tid; j < a.Ck; j += GC_T) {
      const int g = a.gather[j];
      if ((unsigned)g < (unsigned)a.C) inv[g] = (int16_t)j;
    }
  }
  for (int i = tid; i < BM; i += GC_T) {
    const int m = m0 + i;
    int base = 0, h = -(1 << 28), w = -(1 << 28);                 // rows past M: outside the image for every tap
    if (m < a.M) {
      const int hw = a.Ho * a.Wo;
      const int img = m / hw, rem = m - img * hw;
      const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
      base = img * a.H * a.W;
      h = ho * a.stride - a.pad_h;
      w = wo * a.stride - a.pad_w;
    }
    p_base[i] = base; p_h[i] = h; p_w[i] = w;
  }
  __syncthreads();

  // accumulators: bf16 -- wavefront `wave` owns pixels wave*32 .. +31, all NB column blocks; float32 -- thread (tx, ty): 4 x 4
  const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
  const int tx = tid & 15, ty = tid >> 4;
  f32x4 acc[MFMA ? NB : 4][MFMA ? 2 : 1];
#pragma unroll
  for (int i = 0; i < (MFMA ? NB : 4); ++i)
#pragma unroll
    for (int j = 0; j < (MFMA ? 2 : 1); ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int sub = tid & 7, prow = tid >> 3;                      // loaders: 8 lanes per tile row, 32 rows per pass

  for (int tap = 0; tap < RS; ++tap) {
    const int r = tap / a.S, s = tap - r * a.S;
    for (int j0 = 0; j0 < a.Ck; j0 += BK) {
      const int jn = min(BK, a.Ck - j0);                         // kept channels of this k-step
      const int jpad = MFMA ? ((jn + 31) & ~31) : jn;            // columns the multiply reads
      // ---- X tile: contiguous source segment, compacted while writing ------------------------------------------------------
      if (a.xvec) {
        const int v_lo = a.gather[j0] / VE, v_hi = a.gather[j0 + jn - 1] / VE;
        const int nvec = v_hi - v_lo + 1;
        for (int row = prow; row < BM; row += GC_T / 8) {
          const int h = p_h[row] + r, w = p_w[row] + s;
          const bool inside = (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W;
          const T* src = inside ? X + ((int64_t)p_base[row] + (int64_t)h * a.W + w) * a.C : X;
          for (int v = sub; v < nvec; v += 8) {
            const int c = (v_lo + v) * VE;                       // < C: the segment ends at a kept channel and C % VE == 0
            __attribute__((aligned(16))) int16_t jj[VE];
            if (VE == 8) *reinterpret_cast<uint4*>(jj) = *reinterpret_cast<const uint4*>(inv + c);
            else *reinterpret_cast<uint2*>(jj) = *reinterpret_cast<const uint2*>(inv + c);
            bool any = false;
#pragma unroll
            for (int e = 0; e < VE; ++e) any = any || ((unsigned)(jj[e] - j0) < (unsigned)jn);
            if (!any) continue;
            __attribute__((aligned(16))) T xv[VE];
            if (inside) {
              *reinterpret_cast<uint4*>(xv) = *reinterpret_cast<const uint4*>(src + c);
            } else {
#pragma unroll
              for (int e = 0; e < VE; ++e) xv[e] = (T)0;
            }
#pragma unroll
            for (int e = 0; e < VE; ++e) {
              const int j = jj[e] - j0;
              if ((unsigned)j < (unsigned)jn) *gc_at<T>(Xs, row, j) = xv[e];
            }
          }
          for (int j = jn + sub; j < jpad; j += 8) *gc_at<T>(Xs, row, j) = (T)0;
        }
      } else {
        for (int row = prow; row < BM; row += GC_T / 8) {
          const int h = p_h[row] + r, w = p_w[row] + s;
          const bool inside = (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W;
          const T* src = inside ? X + ((int64_t)p_base[row] + (int64_t)h * a.W + w) * a.C : X;
          for (int j = sub; j < jpad; j += 8) {
            T x = (T)0;
            if (inside && j < jn) {
              const int g = a.gather[j0 + j];
              if ((unsigned)g < (unsigned)a.C) x = src[g];
            }
            *gc_at<T>(Xs, row, j) = x;
          }
        }
      }
      // ---- W tile: Wk[n][tap][j0 .. j0 + jn), zero rows past N and zero columns past jn --------------------------------------
      for (int row = prow; row < BN; row += GC_T / 8) {
        const int n = n0 + row;
        const T* src = Wk + ((int64_t)n * RS + tap) * a.Ck + j0;
        if (a.wvec) {                                            // Ck % VE == 0: jn is a multiple of VE too
          const int j = sub * VE;
          if (j < jpad) {
            __attribute__((aligned(16))) T wv[VE];
            if (n < a.N && j < jn) {
              *reinterpret_cast<uint4*>(wv) = *reinterpret_cast<const uint4*>(src + j);
            } else {
#pragma unroll
              for (int e = 0; e < VE; ++e) wv[e] = (T)0;
            }
            if (MFMA) {
              *reinterpret_cast<uint4*>(gc_at<T>(Ws, row, j)) = *reinterpret_cast<const uint4*>(wv);
            } else {
#pragma unroll
              for (int e = 0; e < VE; ++e) *gc_at<T>(Ws, row, j + e) = wv[e];
            }
          }
        } else {
          for (int j = sub; j < jpad; j += 8) *gc_at<T>(Ws, row, j) = (n < a.N && j < jn) ? src[j] : (T)0;
        }
      }
      __syncthreads();
      // ---- multiply ---------------------------------------------------------------------------------------------------------
      if constexpr (MFMA) {
        for (int k = 0; k < jpad; k += 32) {
          bf16x8 xf[2];
#pragma unroll
          for (int jm = 0; jm < 2; ++jm)
            xf[jm] = *reinterpret_cast<const bf16x8*>(gc_at<T>(Xs, wave * 32 + jm * 16 + l15, k + q * 8));
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const bf16x8 wf = *reinterpret_cast<const bf16x8*>(gc_at<T>(Ws, i * 16 + l15, k + q * 8));
#pragma unroll
            for (int jm = 0; jm < 2; ++jm) acc[i][jm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[jm], acc[i][jm], 0, 0, 0);
          }
        }
      } else {
        for (int k = 0; k < jn; ++k) {
          const float4 xa = *reinterpret_cast<const float4*>(gc_at<T>(Xs, ty * 4, k));
          const float4 wb = *reinterpret_cast<const float4*>(gc_at<T>(Ws, tx * 4, k));
          const float xr[4] = {xa.x, xa.y, xa.z, xa.w}, wr[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][0][j] = fmaf(xr[i], wr[j], acc[i][0][j]);
        }
      }
      __syncthreads();
    }
  }

  // ---- epilogue -----------------------------------------------------------------------------------------------------------------
  if constexpr (MFMA) {
#pragma unroll
    for (int jm = 0; jm < 2; ++jm)
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        float v[4] = {acc[i][jm][0], acc[i][jm][1], acc[i][jm][2], acc[i][jm][3]};
        gc_epilogue4<T>(a, m0 + wave * 32 + jm * 16 + l15, n0 + i * 16 + q * 4, v);
      }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v[4] = {acc[i][0][0], acc[i][0][1], acc[i][0][2], acc[i][0][3]};
      gc_epilogue4<T>(a, m0 + ty * 4 + i, n0 + tx * 4, v);
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
template <typename T, int NB>
static int gc_launch(const GcArgs& a, hipStream_t st) {
  const int BM = GcTile<T>::BM, BN = NB * 16;
  const int64_t tiles = (int64_t)((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
  if (tiles >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  const size_t dyn = a.xvec ? (size_t)((a.C + 7) & ~7) * sizeof(int16_t) : 0;
  k_conv_gather<T, NB><<<dim3((unsigned)tiles), GC_T, dyn, st>>>(a);
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_conv_gather_fwd(const void* x, const void* w, const int32_t* gather, const float* bias, const void* res,
                                  const float* scale_shift, int act, void* y, int dtype, int imgs, int H, int W, int C, int Ck, int N,
                                  int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream) {
  if (imgs <= 0 || H <= 0 || W <= 0 || C <= 0 || Ck <= 0 || Ck > C || N <= 0 || R <= 0 || S <= 0 || stride <= 0 || pad_h < 0 ||
      pad_w < 0 || Ho <= 0 || Wo <= 0 || x == nullptr || w == nullptr || gather == nullptr || y == nullptr)
    return (int)hipErrorInvalidValue;
  if (act != PF_ACT_NONE && act != PF_ACT_RELU && act != PF_ACT_RELU6) return (int)hipErrorInvalidValue;
  if ((int64_t)imgs * Ho * Wo >= ((int64_t)1 << 31) || (int64_t)imgs * H * W >= ((int64_t)1 << 31) ||
      (int64_t)R * S * Ck >= ((int64_t)1 << 31) || C > GC_MAX_C)
    return (int)hipErrorInvalidValue;
  GcArgs a{};
  a.X = x; a.Wk = w; a.gather = gather; a.bias = bias; a.Res = res; a.oss = scale_shift; a.Y = y; a.act = act;
  a.imgs = imgs; a.H = H; a.W = W; a.C = C; a.Ck = Ck; a.N = N; a.R = R; a.S = S; a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w;
  a.Ho = Ho; a.Wo = Wo; a.M = imgs * Ho * Wo;
  const int ve = (dtype == PF_BF16) ? 8 : 4;
  a.xvec = (C % ve == 0) && pf_aligned16(x);
  a.wvec = (Ck % ve == 0) && pf_aligned16(w);
  const size_t esz = (dtype == PF_BF16) ? 2 : 4;
  a.yvec = (N % 4 == 0) && (((uintptr_t)y) % (4 * esz) == 0) && (res == nullptr || ((uintptr_t)res) % (4 * esz) == 0);
  if (dtype == PF_F32) return gc_launch<float, 4>(a, (hipStream_t)stream);
  if (dtype == PF_BF16) return (N <= 64) ? gc_launch<bf16_t, 4>(a, (hipStream_t)stream) : gc_launch<bf16_t, 8>(a, (hipStream_t)stream);
  return (int)hipErrorInvalidValue;
}
