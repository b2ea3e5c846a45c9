// K13 fused with K4: batch-norm (training / inference) + ReLU/ReLU6 + activation fake-quant over
// NHWC activations viewed as a [rows][C] matrix, forward and backward.
//
//   forward : pass 1 reads x once -> per-channel {sum, sumsq, min, max} (block partials)
//             finalize            -> mean/var, scale/shift, moving stats, and the EXACT whole-tensor
//                                    min/max of y = act(scale*x+shift) from per-channel min/max of x
//                                    (y is monotone in x per channel), written to the min/max slot
//             pass 2 reads x, writes q = fake_quant(y)
//   i.e. 2 reads + 1 write per element instead of the reference's ~9 separate TF elementwise /
//   reduction kernels (batch_norm, relu, reduce_max, reduce_min, sub, div, mul, round, div, mul, add).
//   backward: pass 1 reads dq, x -> per-channel {sum dy, sum dy*xhat}; pass 2 reads dq, x, writes dx.
//             The ReLU mask is recomputed from x, so neither y nor a mask tensor is ever stored.
//
// Reference semantics restated here (paths under /root/reference; BN maths is TF's fused kernel):
//   utils/external/resnet_model.py:55-62   tf.layers.batch_normalization(momentum=.997, eps=1e-5, fused)
//   utils/external/mobilenet_v1.py:428-477 slim.batch_norm(decay=.9997, epsilon=1e-3)
//   learners/uniform_quantization/utils.py:51-79  activation fake-quant after every Relu / Relu6
#include "pf_common.h"

// Fast path: C % 8 == 0, G = C/8 <= 256 (C = 8 .. 2048): a thread owns one group of 8 consecutive
// channels and walks rows; a wavefront reads 1 KiB contiguous.  Where G does not divide the
// workgroup, the left-over lanes idle (pf_common.h); for the powers of two nothing changed.
static inline bool bn_fast_ok(int C) { return pf_vec8_ok(C); }
extern "C" int pf_bn_vector_ok(int C) { return bn_fast_ok(C) ? 1 : 0; }

// The storage type of an extern "C" entry: f is called with a null T* (T = float / bf16_t) and returns the entry's status.
template <typename F> static inline int bn_with_dtype(int dtype, F&& f) {
  if (dtype == PF_F32) return f((float*)nullptr);
  if (dtype == PF_BF16) return f((bf16_t*)nullptr);
  return (int)hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// forward pass 1
// ---------------------------------------------------------------------------------------------
// 2-D decomposition: a 1024-thread workgroup (16 wavefronts) owns a SLAB of up to 64 channels
// (CG <= 8 groups of 8 channels, 16 B per lane) and one of `nsplit` interleaved row ranges;
// 1024/CG row-lanes walk the rows.  Per-workgroup partials are only 4 x 64 floats, so the partial
// buffer [nsplit][4][C] stays ~1000x smaller than the tensor and the finalize pass is a few us.
// CG is a power of two (the butterfly of bn_wave_reduce8): G = C/8 itself for 1, 2, 4, the next power of two for 3, 5, 6, 7,
// and 8 beyond, with nslab = ceil(G / CG) slabs.  The lanes of a group >= G (in the last slab only, and only where CG does not
// divide G) load nothing -- no pivot, no row -- carry the identity of every statistic through the reductions, and no thread
// writes a channel >= C.
#define BN_BIG 1024
__host__ __device__ __forceinline__ int bn_cg_of(int C) {
  const int G = C >> 3;
  return G >= 8 ? 8 : (G <= 2 ? G : (G <= 4 ? 4 : 8));
}
static inline int bn_nslab_of(int C) { return ((C >> 3) + bn_cg_of(C) - 1) / bn_cg_of(C); }

// KIND per statistic: 0 = sum, 1 = min, 2 = max
template <int KIND> __device__ __forceinline__ float bn_comb(float a, float b) {
  return KIND == 0 ? (a + b) : (KIND == 1 ? fminf(a, b) : fmaxf(a, b));
}
template <int KIND>
__device__ __forceinline__ void bn_wave_reduce8(float (&a)[8], int CG) {
  // lanes with equal (lane % CG) hold the same channel group: butterfly over the other lane bits
  for (int m = CG; m < 64; m <<= 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = bn_comb<KIND>(a[j], __shfl_xor(a[j], m, 64));
  }
}
template <int KIND>
__device__ __forceinline__ void bn_lds_put(const float (&a)[8], int st, int NS, int CG, float* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < CG) {
#pragma unroll
    for (int j = 0; j < 8; ++j) lds[(wave * NS + st) * 64 + lane * 8 + j] = a[j];
  }
}
template <int KIND>
__device__ __forceinline__ void bn_lds_finish(int st, int NS, int slabC, const float* lds, float* out) {
  // threads [st*slabC, (st+1)*slabC) combine the 16 per-wave partials of statistic `st`
  const int t = (int)threadIdx.x - st * slabC;
  if (t >= 0 && t < slabC) {
    float a = lds[st * 64 + t];
    for (int w = 1; w < BN_BIG / 64; ++w) a = bn_comb<KIND>(a, lds[(w * NS + st) * 64 + t]);
    out[t] = a;
  }
}

template <typename T>
__global__ __launch_bounds__(BN_BIG) void k_bn_stats_fast(const T* __restrict__ x, int64_t rows, int C,
                                                          float* __restrict__ partial, int nslab, int nsplit) {
  __shared__ float lds[(BN_BIG / 64) * 4 * 64];
  const int CG = bn_cg_of(C), slabC = CG * 8, RL = BN_BIG / CG;
  const int slab = blockIdx.x % nslab, split = blockIdx.x / nslab;
  const int cg = threadIdx.x % CG, rl = threadIdx.x / CG;
  const int c0 = slab * slabC + cg * 8;
  const bool live = c0 < C;                       // false: a group >= G of the guarded last slab
  float piv[8];
  float s[8], ss[8], mn[8], mx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s[j] = 0.f; ss[j] = 0.f; mn[j] = INFINITY; mx[j] = -INFINITY; }
  if (live) {
    load8<T>(x + c0, piv);                        // pivot = row 0 (shifted sums: no cancellation)
#pragma unroll 2
    for (int64_t r = (int64_t)split * RL + rl; r < rows; r += (int64_t)nsplit * RL) {
      float v[8];
      load8<T>(x + r * C + c0, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[j] - piv[j];
        s[j] += d;
        ss[j] = fmaf(d, d, ss[j]);
        mn[j] = pf_acc_min(mn[j], v[j]);
        mx[j] = pf_acc_max(mx[j], v[j]);
      }
    }
  }
  bn_wave_reduce8<0>(s, CG); bn_wave_reduce8<0>(ss, CG); bn_wave_reduce8<1>(mn, CG); bn_wave_reduce8<2>(mx, CG);
  bn_lds_put<0>(s, 0, 4, CG, lds); bn_lds_put<0>(ss, 1, 4, CG, lds);
  bn_lds_put<1>(mn, 2, 4, CG, lds); bn_lds_put<2>(mx, 3, 4, CG, lds);
  __syncthreads();
  float* out = partial + (int64_t)split * 4 * C + slab * slabC;
  const int nC = min(slabC, C - slab * slabC);    // channels of this slab that exist
  bn_lds_finish<0>(0, 4, nC, lds, out);
  bn_lds_finish<0>(1, 4, nC, lds, out + C);
  bn_lds_finish<1>(2, 4, nC, lds, out + 2 * C);
  bn_lds_finish<2>(3, 4, nC, lds, out + 3 * C);
}

template <typename T>
__global__ __launch_bounds__(PF_THREADS) void k_bn_stats_generic(const T* __restrict__ x, int64_t rows, int C,
                                                                 float* __restrict__ partial) {
  // thread = channel (grid.x over channel tiles), grid.y = row split
  const int c = blockIdx.x * PF_THREADS + threadIdx.x;
  if (c >= C) return;
  const float piv = load_one<T>(x + c);
  float s = 0.f, ss = 0.f, mn = INFINITY, mx = -INFINITY;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const float v = load_one<T>(x + r * C + c);
    const float d = v - piv;
    s += d; ss = fmaf(d, d, ss);
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  float* out = partial + (int64_t)blockIdx.y * 4 * C;
  out[c] = s; out[C + c] = ss; out[2 * C + c] = mn; out[3 * C + c] = mx;
}

extern "C" int pf_bn_stats(const void* x, int dtype, int64_t rows, int C, float* partial,
                           int n_blocks, void* stream) {
  if (rows <= 0 || C <= 0 || n_blocks <= 0) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  return bn_with_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    if (bn_fast_ok(C) && pf_aligned16(x)) {
      const int nslab = bn_nslab_of(C);
      k_bn_stats_fast<T><<<nslab * n_blocks, BN_BIG, 0, st>>>((const T*)x, rows, C, partial, nslab, n_blocks);
    } else {
      dim3 grid((C + PF_THREADS - 1) / PF_THREADS, n_blocks);
      k_bn_stats_generic<T><<<grid, PF_THREADS, 0, st>>>((const T*)x, rows, C, partial);
    }
    PF_LAUNCH_CHECK();
    return 0;
  });
}

// ---------------------------------------------------------------------------------------------
// finalize: 16 channels x 16 row-partial lanes per workgroup.  The kernel is a dependent-latency chain between a producer's
// statistics and the next launch that reads scale / shift (49 launches a step, nothing else of the student's stream in flight),
// so the levers are workgroups (C / 16 instead of C / 64) and loads in flight: a lane owns partial blocks part, part+16, ...
// and requests eight of them (32 loads) before it adds -- in ASCENDING block order, then the 16 lanes of a channel combine in
// ascending lane order through LDS: the summation order of rounds 1-5 (64 channels x 16 lanes, one block per trip), bit for bit.
// (A 64-lane tree per channel was 0.2 us faster and equally accurate -- every call within 1.5e-6 of a float64 two-pass result,
// tools/gpu/bn_finalize_audit.py -- but moved the bf16 gradient checks of the two small networks, whose per-variable bars
// compare noise with noise at the 0.05 level, across their margins: profiles/r06_bn_finalize_order.txt.)
// 13.8 -> 12.0 us per launch inside replays, 6.5 us launch by launch (profiles/r06_step_kernels_b256*.csv).
// ---------------------------------------------------------------------------------------------
template <int ACT>
__device__ __forceinline__ void y_range(float scale, float shift, float xmin, float xmax, float& ymin,
                                        float& ymax) {
  const float a = fmaf(scale, xmin, shift), b = fmaf(scale, xmax, shift);
  ymin = apply_act<ACT>(fminf(a, b));
  ymax = apply_act<ACT>(fmaxf(a, b));
}

#define BN_FIN_C 16                      // channels per block
#define BN_FIN_P 16                      // row-partial lanes per channel
#define BN_FIN_T (BN_FIN_P * BN_FIN_C)   // 256 threads
#define BN_FIN_U 8                       // partial blocks requested per trip
__global__ __launch_bounds__(BN_FIN_T) void k_bn_finalize(
    const float* __restrict__ partial, int n_blocks, int64_t rows, int C, const void* __restrict__ x_row0,
    int dtype, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ moving_mean, float* __restrict__ moving_var, float momentum, float eps,
    int training, int act, float* __restrict__ scale_shift, float* __restrict__ mean_invstd,
    uint32_t* __restrict__ slot) {
  __shared__ float l_s[BN_FIN_P][BN_FIN_C], l_ss[BN_FIN_P][BN_FIN_C], l_mn[BN_FIN_P][BN_FIN_C], l_mx[BN_FIN_P][BN_FIN_C];
  const int cl = threadIdx.x & (BN_FIN_C - 1), part = threadIdx.x / BN_FIN_C;
  const int c = blockIdx.x * BN_FIN_C + cl;
  const bool live = c < C;
  float s = 0.f, ss = 0.f, mn = INFINITY, mx = -INFINITY;
  // constants of the tail, requested before the partial sums so that their latency hides under the loop
  float piv = 0.f, g = 0.f, be = 0.f, mm = 0.f, mv = 0.f;
  if (live && part == 0) {
    g = gamma[c]; be = beta[c]; mm = moving_mean[c]; mv = moving_var[c];
    if (training) piv = (dtype == PF_F32) ? ((const float*)x_row0)[c] : bf16_to_f32(((const bf16_t*)x_row0)[c]);
  }
  if (live) {
    const int64_t step = (int64_t)BN_FIN_P * 4 * C;
    int b = part;
    for (; b + (BN_FIN_U - 1) * BN_FIN_P < n_blocks; b += BN_FIN_U * BN_FIN_P) {
      const float* p = partial + (int64_t)b * 4 * C + c;
      float v0[BN_FIN_U], v1[BN_FIN_U], v2[BN_FIN_U], v3[BN_FIN_U];
#pragma unroll
      for (int u = 0; u < BN_FIN_U; ++u) { v0[u] = p[u * step]; v1[u] = p[u * step + C]; v2[u] = p[u * step + 2 * C]; v3[u] = p[u * step + 3 * C]; }
#pragma unroll
      for (int u = 0; u < BN_FIN_U; ++u) {                 // ascending block order
        s += v0[u]; ss += v1[u];
        mn = fminf(mn, v2[u]); mx = fmaxf(mx, v3[u]);
      }
    }
    for (; b < n_blocks; b += BN_FIN_P) {
      const float* p = partial + (int64_t)b * 4 * C + c;
      s += p[0]; ss += p[C];
      mn = fminf(mn, p[2 * C]); mx = fmaxf(mx, p[3 * C]);
    }
  }
  l_s[part][cl] = s; l_ss[part][cl] = ss; l_mn[part][cl] = mn; l_mx[part][cl] = mx;
  __syncthreads();
  float ymin = INFINITY, ymax = -INFINITY;
  if (part == 0 && live) {
    s = l_s[0][cl]; ss = l_ss[0][cl]; mn = l_mn[0][cl]; mx = l_mx[0][cl];
#pragma unroll
    for (int p = 1; p < 16; ++p) {                       // fixed order: deterministic
      s += l_s[p][cl]; ss += l_ss[p][cl];
      mn = fminf(mn, l_mn[p][cl]); mx = fmaxf(mx, l_mx[p][cl]);
    }
    float mean, var;
    if (training) {
      const double n = (double)rows;
      const double m1 = (double)s / n;
      double v = (double)ss / n - m1 * m1;             // biased variance of (x - pivot) == of x
      if (v < 0.0) v = 0.0;
      mean = (float)((double)piv + m1);
      var = (float)v;
      // moving averages: tf.layers BN  moving -= (moving - batch) * (1 - momentum); the fused
      // kernel hands the UNBIASED variance to the moving average
      const float unbiased = (float)(v * (n / (n > 1.0 ? n - 1.0 : 1.0)));
      const float omm = 1.0f - momentum;
      moving_mean[c] = mm - (mm - mean) * omm;
      moving_var[c] = mv - (mv - unbiased) * omm;
    } else {
      mean = mm;
      var = mv;
    }
    const float invstd = 1.0f / sqrtf(var + eps);
    const float sc = g * invstd;
    const float sh = fmaf(-mean, sc, be);
    scale_shift[c] = sc;
    scale_shift[C + c] = sh;
    mean_invstd[c] = mean;
    mean_invstd[C + c] = invstd;
    if (act == PF_ACT_RELU) y_range<PF_ACT_RELU>(sc, sh, mn, mx, ymin, ymax);
    else if (act == PF_ACT_RELU6) y_range<PF_ACT_RELU6>(sc, sh, mn, mx, ymin, ymax);
    else y_range<PF_ACT_NONE>(sc, sh, mn, mx, ymin, ymax);
  }
  if (threadIdx.x < 64 && slot != nullptr) {             // wave 0 entire (lanes 16..63 carry the neutral elements)
    ymin = wave_min(ymin);
    ymax = wave_max(ymax);
    if (threadIdx.x == 0 && ymin <= ymax) {
      atomicMin(&slot[0], enc_f32(ymin));
      atomicMin(&slot[1], ~enc_f32(ymax));
    }
  }
}

extern "C" int pf_bn_finalize(const float* partial, int n_blocks, int64_t rows, int C,
                              const void* x_row0, int dtype, const float* gamma, const float* beta,
                              float* moving_mean, float* moving_var, float momentum, float eps,
                              int training, int act, float* scale_shift, float* mean_invstd,
                              uint32_t* slot, void* stream) {
  if (C <= 0) return (int)hipErrorInvalidValue;
  k_bn_finalize<<<(C + BN_FIN_C - 1) / BN_FIN_C, BN_FIN_T, 0, (hipStream_t)stream>>>(
      partial, n_blocks, rows, C, x_row0, dtype, gamma, beta, moving_mean, moving_var, momentum, eps,
      training, act, scale_shift, mean_invstd, slot);
  PF_LAUNCH_CHECK();
  return 0;
}

__global__ void k_bn_eval_scale_shift(const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ mm, const float* __restrict__ mv, float eps,
                                      int C, float* __restrict__ ss) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    const float invstd = 1.0f / sqrtf(mv[c] + eps);
    const float sc = gamma[c] * invstd;
    ss[c] = sc;
    ss[C + c] = fmaf(-mm[c], sc, beta[c]);
  }
}
extern "C" int pf_bn_eval_scale_shift(const float* gamma, const float* beta, const float* moving_mean,
                                      const float* moving_var, float eps, int C, float* scale_shift,
                                      void* stream) {
  k_bn_eval_scale_shift<<<(C + 255) / 256, 256, 0, (hipStream_t)stream>>>(gamma, beta, moving_mean, moving_var, eps, C, scale_shift);
  PF_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// forward pass 2:  q = fake_quant(act(scale*x + shift))
// ---------------------------------------------------------------------------------------------
template <typename T, int ACT, bool FAST>
__global__ __launch_bounds__(PF_THREADS) void k_bn_apply(const T* __restrict__ x, T* __restrict__ q,
                                                         int64_t rows, int C,
                                                         const float* __restrict__ scale_shift,
                                                         const uint32_t* __restrict__ slot, float k,
                                                         int quantize) {
  float alpha = 1.f, beta = 0.f;
  if (quantize) slot_alpha_beta(slot, alpha, beta);
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
      for (int j = 0; j < 8; ++j) {
        const float y = apply_act<ACT>(fmaf(sc[j], v[j], sh[j]));
        v[j] = quantize ? uq_point(y, alpha, beta, k) : y;
      }
      store8<T>(q + off, v);
    }
  } else {
    const int64_t n = rows * C;
    for (int64_t e = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * PF_THREADS) {
      const int c = (int)(e % C);
      const float y = apply_act<ACT>(fmaf(scale_shift[c], load_one<T>(x + e), scale_shift[C + c]));
      store_one<T>(q + e, quantize ? uq_point(y, alpha, beta, k) : y);
    }
  }
}

template <typename T>
static int launch_bn_apply(const T* x, T* q, int64_t rows, int C, const float* ss, int act,
                           const uint32_t* slot, float k, int quantize, hipStream_t st) {
  const bool fast = bn_fast_ok(C) && pf_aligned16(x) && pf_aligned16(q);
  const int grid = fast ? pf_grid_for(rows, (PF_THREADS / (C / 8)) * 2) : pf_grid_for(rows * C, PF_THREADS * 4);
  pf_with_act(act, [&](auto A) {
    pf_with_bool(fast, [&](auto F) {
      k_bn_apply<T, decltype(A)::value, decltype(F)::value><<<grid, PF_THREADS, 0, st>>>(x, q, rows, C, ss, slot, k, quantize);
    });
  });
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_bn_act_quant_apply(const void* x, void* q, int dtype, int64_t rows, int C,
                                     const float* scale_shift, int act, const uint32_t* slot, int bits,
                                     int quantize, void* stream) {
  if (rows <= 0 || C <= 0) return (int)hipErrorInvalidValue;
  if (quantize && (bits < 1 || bits > 32 || slot == nullptr)) return (int)hipErrorInvalidValue;
  const float k = uq_k_of_bits(quantize ? bits : 8);
  return bn_with_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    return launch_bn_apply<T>((const T*)x, (T*)q, rows, C, scale_shift, act, slot, k, quantize, (hipStream_t)stream);
  });
}

// ---------------------------------------------------------------------------------------------
// forward pass 2 of the network head:  pooled[b][c] = T( (sum_p q[b][p][c]) / HW ),  q never written
// ---------------------------------------------------------------------------------------------
// The last BN's activated map feeds nothing but the spatial mean, so pass 2 reduces it on the fly: q is the value k_bn_apply
// would have stored (same scale / shift, activation, uq_point, and the rounding to T), summed in float32 in ASCENDING pixel
// order p = 0 .. HW-1 by ONE thread per (image, channel) -- a fixed order, bit-deterministic -- and scaled by float32(1 / HW), the
// last step of aten's mean on the device (an accumulated sum times the ROUNDED reciprocal, not a division).
// FAST: a thread owns 8 consecutive channels of one image (16-byte loads, a wavefront reads 1 KiB contiguous per pixel);
// a 256-thread workgroup covers 256 / (C/8) images.  Otherwise one thread per (image, channel).
template <typename T, int ACT, bool FAST>
__global__ __launch_bounds__(PF_THREADS) void k_bn_apply_pool(const T* __restrict__ x, T* __restrict__ pooled,
                                                              int B, int HW, int C,
                                                              const float* __restrict__ scale_shift,
                                                              const uint32_t* __restrict__ slot, float k,
                                                              int quantize) {
  float alpha = 1.f, beta = 0.f;
  if (quantize) slot_alpha_beta(slot, alpha, beta);
  const float inv_hw = 1.0f / (float)HW;
  const int64_t item = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x;
  if (FAST) {
    const int G = C >> 3;
    if (item >= (int64_t)B * G) return;
    const int b = (int)(item / G), cg = (int)(item % G);
    float sc[8], sh[8], acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = scale_shift[(cg << 3) + j]; sh[j] = scale_shift[C + (cg << 3) + j]; acc[j] = 0.f; }
    const T* __restrict__ px = x + (int64_t)b * HW * C + (cg << 3);
#pragma unroll 7
    for (int p = 0; p < HW; ++p) {
      float v[8];
      load8<T>(px + (int64_t)p * C, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float y = apply_act<ACT>(fmaf(sc[j], v[j], sh[j]));
        acc[j] += round_to<T>(quantize ? uq_point(y, alpha, beta, k) : y);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] * inv_hw;
    store8<T>(pooled + (int64_t)b * C + (cg << 3), acc);
  } else {
    if (item >= (int64_t)B * C) return;
    const int b = (int)(item / C), c = (int)(item % C);
    const float sc = scale_shift[c], sh = scale_shift[C + c];
    const T* __restrict__ px = x + (int64_t)b * HW * C + c;
    float acc = 0.f;
    for (int p = 0; p < HW; ++p) {
      const float y = apply_act<ACT>(fmaf(sc, load_one<T>(px + (int64_t)p * C), sh));
      acc += round_to<T>(quantize ? uq_point(y, alpha, beta, k) : y);
    }
    store_one<T>(pooled + item, acc * inv_hw);
  }
}

// The pooled pass keeps the channel counts it took before the vector map was opened to every C % 8 == 0 (G = C / 8 a power of two):
// its FAST form has B * G threads walk HW pixels one after the other, and at 256 x 49 x 768 (bf16) that lost to the scalar form's
// eight times as many threads, 45.0 against 21.3 us (profiles/odd_channel_layers.txt).
static inline bool bn_pool_fast_ok(int C) { return bn_fast_ok(C) && ((C >> 3) & ((C >> 3) - 1)) == 0; }

template <typename T>
static int launch_bn_apply_pool(const T* x, T* pooled, int64_t rows, int C, int HW, const float* ss, int act,
                                const uint32_t* slot, float k, int quantize, hipStream_t st) {
  const bool fast = bn_pool_fast_ok(C) && pf_aligned16(x) && pf_aligned16(pooled);
  const int64_t B = rows / HW;
  const int64_t items = fast ? B * (C / 8) : B * C;
  const int64_t grid = (items + PF_THREADS - 1) / PF_THREADS;
  if (grid > 0x7FFFFFFF) return (int)hipErrorInvalidValue;
  pf_with_act(act, [&](auto A) {
    pf_with_bool(fast, [&](auto F) {
      k_bn_apply_pool<T, decltype(A)::value, decltype(F)::value><<<(int)grid, PF_THREADS, 0, st>>>(x, pooled, (int)B, HW, C, ss, slot, k, quantize);
    });
  });
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_bn_act_quant_pool(const void* x, void* pooled, int dtype, int64_t rows, int C,
                                    const float* scale_shift, int act, const uint32_t* slot, int bits,
                                    int quantize, int HW, void* stream) {
  if (rows <= 0 || C <= 0 || HW <= 0 || rows % HW != 0 || rows / HW > 0x7FFFFFFF) return (int)hipErrorInvalidValue;
  if (quantize && (bits < 1 || bits > 32 || slot == nullptr)) return (int)hipErrorInvalidValue;
  const float k = uq_k_of_bits(quantize ? bits : 8);
  return bn_with_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    return launch_bn_apply_pool<T>((const T*)x, (T*)pooled, rows, C, HW, scale_shift, act, slot, k, quantize, (hipStream_t)stream);
  });
}

// ---------------------------------------------------------------------------------------------
// backward: where dq comes from
// ---------------------------------------------------------------------------------------------
// The two backward passes below are templates over POOLED.  false: dq is the [rows][C] gradient of this BN's output, read as it
// is.  true (the network head, HW > 0): this BN's output feeds nothing but the spatial mean (pf_bn_act_quant_pool), so `dq` is the
// [B][C] gradient of the POOLED tensor and the value of row r = (b, p) is rebuilt on the fly,
// T(float(dq[b][c]) * float32(1 / HW)) -- bit for bit what autograd's cast / mean / cast chain writes into the expanded
// [B * HW][C] tensor on the device (aten divides a tensor by a host scalar as a product with the rounded reciprocal), which is then
// never stored or read.  Only the dq load depends on POOLED (and the head has no shortcut: the pooled apply pass drops the addend
// test): row order, splits and the partial layout are shared, so every sum and dx of the pooled form are bit-identical to the
// plain pass over the expanded tensor.  HW sits in the 4 bytes of padding behind C, which leaves every other kernel argument at
// its offset, and the plain instantiations never load it.  b = r / HW is a 32-bit division (a 64-bit one is a long software
// sequence per row in the loop): the pooled entry points require rows < 2^31 (bn_pooled_ok).
template <typename T>
__device__ __forceinline__ void pooled_dq8(const T* __restrict__ g, int64_t r, int C, int c0, int HW, float (&out)[8]) {
  const float inv_hw = 1.0f / (float)HW;
  load8<T>(g + (int64_t)((uint32_t)r / (uint32_t)HW) * C + c0, out);
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = round_to<T>(out[j] * inv_hw);
}
template <typename T>
__device__ __forceinline__ float pooled_dq1(const T* __restrict__ g, int64_t r, int C, int c, int HW) {
  return round_to<T>(load_one<T>(g + (int64_t)((uint32_t)r / (uint32_t)HW) * C + c) * (1.0f / (float)HW));
}
static inline bool bn_pooled_ok(int64_t rows, int HW) {
  return HW > 0 && rows > 0 && rows < ((int64_t)1 << 31) && rows % HW == 0;
}

// ---------------------------------------------------------------------------------------------
// backward pass 1: per-channel sum(dy), sum(dy * xhat),  dy = dq * act'(scale*x+shift)
// ---------------------------------------------------------------------------------------------
template <typename T, int ACT, bool POOLED>
__global__ __launch_bounds__(BN_BIG) void k_bn_bwd_stats_fast(const T* __restrict__ dq, const T* __restrict__ x,
                                                              int64_t rows, int C, int HW,
                                                              const float* __restrict__ scale_shift,
                                                              const float* __restrict__ mean_invstd,
                                                              float* __restrict__ partial, int nslab, int nsplit) {
  __shared__ float lds[(BN_BIG / 64) * 2 * 64];
  const int CG = bn_cg_of(C), slabC = CG * 8, RL = BN_BIG / CG;
  const int slab = blockIdx.x % nslab, split = blockIdx.x / nslab;
  const int cg = threadIdx.x % CG, rl = threadIdx.x / CG;
  const int c0 = slab * slabC + cg * 8;
  const bool live = c0 < C;                       // false: a group >= G of the guarded last slab
  float sc[8], sh[8], mu[8], is[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = live ? c0 + j : j;              // an idle lane reads channel j's constants and never uses them
    sc[j] = scale_shift[c]; sh[j] = scale_shift[C + c];
    mu[j] = mean_invstd[c]; is[j] = mean_invstd[C + c];
    s1[j] = 0.f; s2[j] = 0.f;
  }
#pragma unroll 2
  for (int64_t r = live ? (int64_t)split * RL + rl : rows; r < rows; r += (int64_t)nsplit * RL) {
    float g[8], v[8];
    const int64_t off = r * C + c0;
    if (POOLED) pooled_dq8<T>(dq, r, C, c0, HW, g);
    else load8<T>(dq + off, g);
    load8<T>(x + off, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float dy = g[j] * act_mask<ACT>(fmaf(sc[j], v[j], sh[j]));
      s1[j] += dy;
      s2[j] = fmaf(dy, (v[j] - mu[j]) * is[j], s2[j]);
    }
  }
  bn_wave_reduce8<0>(s1, CG); bn_wave_reduce8<0>(s2, CG);
  bn_lds_put<0>(s1, 0, 2, CG, lds); bn_lds_put<0>(s2, 1, 2, CG, lds);
  __syncthreads();
  float* out = partial + (int64_t)split * 2 * C + slab * slabC;
  const int nC = min(slabC, C - slab * slabC);    // channels of this slab that exist
  bn_lds_finish<0>(0, 2, nC, lds, out);
  bn_lds_finish<0>(1, 2, nC, lds, out + C);
}

template <typename T, int ACT, bool POOLED>
__global__ __launch_bounds__(PF_THREADS) void k_bn_bwd_stats_generic(const T* __restrict__ dq, const T* __restrict__ x,
                                                                     int64_t rows, int C, int HW,
                                                                     const float* __restrict__ scale_shift,
                                                                     const float* __restrict__ mean_invstd,
                                                                     float* __restrict__ partial) {
  const int c = blockIdx.x * PF_THREADS + threadIdx.x;
  if (c >= C) return;
  const float sc = scale_shift[c], sh = scale_shift[C + c], mu = mean_invstd[c], is = mean_invstd[C + c];
  float s1 = 0.f, s2 = 0.f;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const float v = load_one<T>(x + r * C + c);
    const float g = POOLED ? pooled_dq1<T>(dq, r, C, c, HW) : load_one<T>(dq + r * C + c);
    const float dy = g * act_mask<ACT>(fmaf(sc, v, sh));
    s1 += dy;
    s2 = fmaf(dy, (v - mu) * is, s2);
  }
  float* out = partial + (int64_t)blockIdx.y * 2 * C;
  out[c] = s1; out[C + c] = s2;
}

// HW = 0: dq is dense; HW > 0: the pooled gradient of HW pixels per image
template <typename T>
static int launch_bn_bwd_stats(const T* dq, const T* x, int64_t rows, int C, int HW, const float* ss,
                               const float* mi, int act, float* partial, int n_blocks, hipStream_t st) {
  const bool fast = bn_fast_ok(C) && pf_aligned16(x) && pf_aligned16(dq);
  const int nslab = fast ? bn_nslab_of(C) : 1;
  dim3 ggrid((C + PF_THREADS - 1) / PF_THREADS, n_blocks);
  pf_with_act(act, [&](auto A) {
    pf_with_bool(HW > 0, [&](auto P) {
      if (fast) k_bn_bwd_stats_fast<T, decltype(A)::value, decltype(P)::value><<<nslab * n_blocks, BN_BIG, 0, st>>>(dq, x, rows, C, HW, ss, mi, partial, nslab, n_blocks);
      else k_bn_bwd_stats_generic<T, decltype(A)::value, decltype(P)::value><<<ggrid, PF_THREADS, 0, st>>>(dq, x, rows, C, HW, ss, mi, partial);
    });
  });
  PF_LAUNCH_CHECK();
  return 0;
}

static int bn_bwd_stats_entry(const void* dq, const void* x, int dtype, int64_t rows, int C, int HW,
                              const float* scale_shift, const float* mean_invstd, int act, float* partial,
                              int n_blocks, void* stream) {
  return bn_with_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    return launch_bn_bwd_stats<T>((const T*)dq, (const T*)x, rows, C, HW, scale_shift, mean_invstd, act, partial, n_blocks, (hipStream_t)stream);
  });
}

extern "C" int pf_bn_bwd_stats(const void* dq, const void* x, int dtype, int64_t rows, int C,
                               const float* scale_shift, const float* mean_invstd, int act,
                               float* partial, int n_blocks, void* stream) {
  if (rows <= 0 || C <= 0 || n_blocks <= 0) return (int)hipErrorInvalidValue;
  return bn_bwd_stats_entry(dq, x, dtype, rows, C, 0, scale_shift, mean_invstd, act, partial, n_blocks, stream);
}

extern "C" int pf_bn_bwd_stats_pooled(const void* g, const void* x, int dtype, int64_t rows, int C, int HW,
                                      const float* scale_shift, const float* mean_invstd, int act,
                                      float* partial, int n_blocks, void* stream) {
  if (C <= 0 || n_blocks <= 0 || !bn_pooled_ok(rows, HW)) return (int)hipErrorInvalidValue;
  return bn_bwd_stats_entry(g, x, dtype, rows, C, HW, scale_shift, mean_invstd, act, partial, n_blocks, stream);
}

__global__ __launch_bounds__(PF_THREADS) void k_bn_bwd_finalize(const float* __restrict__ partial, int n_blocks,
                                                                int C, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta) {
  // 16 channels x 16 partial-row lanes per workgroup: the kernel is a dependent-latency chain (n_blocks <= 256 rows of
  // 2*C floats), so the lever is parallelism per channel -- 64 channels x 4 lanes took 13 us per launch, 49 launches a step.
  // Fixed summation order (lane-strided partial sums, then a fixed tree): deterministic.
  __shared__ float l1[16][17], l2[16][17];
  const int cl = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s1 = 0.f, s2 = 0.f;
  if (c < C)
    for (int b = part; b < n_blocks; b += 16) {
      const float* p = partial + (int64_t)b * 2 * C;
      s1 += p[c]; s2 += p[C + c];
    }
  l1[part][cl] = s1; l2[part][cl] = s2;
  __syncthreads();
  if (part == 0 && c < C) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a += l1[r][cl]; b += l2[r][cl]; }
    dbeta[c] = a;
    dgamma[c] = b;
  }
}

extern "C" int pf_bn_bwd_finalize(const float* partial, int n_blocks, int C, float* dgamma, float* dbeta,
                                  void* stream) {
  k_bn_bwd_finalize<<<(C + 15) / 16, PF_THREADS, 0, (hipStream_t)stream>>>(partial, n_blocks, C, dgamma, dbeta);
  PF_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// backward pass 2: dx = gamma*invstd * (dy - dbeta/n - xhat * dgamma/n)
// ---------------------------------------------------------------------------------------------
template <typename T, int ACT, bool FAST, bool POOLED>
__global__ __launch_bounds__(PF_THREADS) void k_bn_bwd_apply(const T* __restrict__ dq, const T* __restrict__ x,
                                                             T* __restrict__ dx, int64_t rows, int C, int HW,
                                                             const float* __restrict__ scale_shift,
                                                             const float* __restrict__ mean_invstd,
                                                             const float* __restrict__ dgamma,
                                                             const float* __restrict__ dbeta,
                                                             const T* __restrict__ addend) {
  // addend (optional): the gradient arriving through the block's identity shortcut, which shares x with
  // this BN -- dx_total = dx_bn + addend in the same pass (autograd would add them in a separate kernel).
  // Never with POOLED: tested at run time there, the dead branch costs the pooled loop 10 registers.
  const float inv_n = 1.0f / (float)rows;
  if (FAST) {
    const int G = C >> 3, RPS = PF_THREADS / G;
    const int cg = threadIdx.x % G, rsub = threadIdx.x / G;
    float sc[8], sh[8], mu[8], is[8], a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = (cg << 3) + j;
      sc[j] = scale_shift[c]; sh[j] = scale_shift[C + c];
      mu[j] = mean_invstd[c]; is[j] = mean_invstd[C + c];
      a[j] = dbeta[c] * inv_n; b[j] = dgamma[c] * inv_n;
    }
#pragma unroll 2
    for (int64_t r = pf_vec8_first_row(rsub, RPS, rows); r < rows; r += (int64_t)gridDim.x * RPS) {
      float g[8], v[8];
      const int64_t off = r * C + (cg << 3);
      if (POOLED) pooled_dq8<T>(dq, r, C, cg << 3, HW, g);
      else load8<T>(dq + off, g);
      load8<T>(x + off, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = bn_bwd_dx<ACT>(g[j], v[j], sc[j], sh[j], mu[j], is[j], a[j], b[j]);
      if (!POOLED && addend != nullptr) {
        float ad[8];
        load8<T>(addend + off, ad);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] += ad[j];
      }
      store8<T>(dx + off, g);
    }
  } else {
    const int64_t n = rows * C;
    for (int64_t e = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * PF_THREADS) {
      const int c = (int)(e % C);
      const float v = load_one<T>(x + e);
      const float sc = scale_shift[c];
      const float g = POOLED ? pooled_dq1<T>(dq, e / C, C, c, HW) : load_one<T>(dq + e);
      const float dy = g * act_mask<ACT>(fmaf(sc, v, scale_shift[C + c]));
      const float xh = (v - mean_invstd[c]) * mean_invstd[C + c];
      float o = sc * (dy - dbeta[c] * inv_n - xh * (dgamma[c] * inv_n));
      if (!POOLED && addend != nullptr) o += load_one<T>(addend + e);
      store_one<T>(dx + e, o);
    }
  }
}

// HW as in launch_bn_bwd_stats; addend may be null (which counts as aligned) and is null with HW > 0
template <typename T>
static int launch_bn_bwd_apply(const T* dq, const T* x, T* dx, int64_t rows, int C, int HW, const float* ss,
                               const float* mi, const float* dgamma, const float* dbeta, int act,
                               const T* addend, hipStream_t st) {
  const bool fast = bn_fast_ok(C) && pf_aligned16(x) && pf_aligned16(dq) && pf_aligned16(dx) && pf_aligned16(addend);
  const int grid = fast ? pf_grid_for(rows, (PF_THREADS / (C / 8)) * 2) : pf_grid_for(rows * C, PF_THREADS * 4);
  pf_with_act(act, [&](auto A) {
    pf_with_bool(fast, [&](auto F) {
      pf_with_bool(HW > 0, [&](auto P) {
        k_bn_bwd_apply<T, decltype(A)::value, decltype(F)::value, decltype(P)::value><<<grid, PF_THREADS, 0, st>>>(dq, x, dx, rows, C, HW, ss, mi, dgamma, dbeta, addend);
      });
    });
  });
  PF_LAUNCH_CHECK();
  return 0;
}

static int bn_bwd_apply_entry(const void* dq, const void* x, const void* addend, void* dx, int dtype, int64_t rows, int C,
                              int HW, const float* scale_shift, const float* mean_invstd, const float* dgamma,
                              const float* dbeta, int act, void* stream) {
  return bn_with_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    return launch_bn_bwd_apply<T>((const T*)dq, (const T*)x, (T*)dx, rows, C, HW, scale_shift, mean_invstd, dgamma, dbeta, act, (const T*)addend, (hipStream_t)stream);
  });
}

extern "C" int pf_bn_bwd_apply_add(const void* dq, const void* x, const void* addend, void* dx, int dtype,
                                   int64_t rows, int C, const float* scale_shift, const float* mean_invstd,
                                   const float* dgamma, const float* dbeta, int act, void* stream) {
  if (rows <= 0 || C <= 0) return (int)hipErrorInvalidValue;
  return bn_bwd_apply_entry(dq, x, addend, dx, dtype, rows, C, 0, scale_shift, mean_invstd, dgamma, dbeta, act, stream);
}

extern "C" int pf_bn_bwd_apply(const void* dq, const void* x, void* dx, int dtype, int64_t rows, int C,
                               const float* scale_shift, const float* mean_invstd, const float* dgamma,
                               const float* dbeta, int act, void* stream) {
  return pf_bn_bwd_apply_add(dq, x, nullptr, dx, dtype, rows, C, scale_shift, mean_invstd, dgamma, dbeta, act, stream);
}

extern "C" int pf_bn_bwd_apply_pooled(const void* g, const void* x, void* dx, int dtype, int64_t rows, int C, int HW,
                                      const float* scale_shift, const float* mean_invstd, const float* dgamma,
                                      const float* dbeta, int act, void* stream) {
  if (C <= 0 || !bn_pooled_ok(rows, HW)) return (int)hipErrorInvalidValue;
  return bn_bwd_apply_entry(g, x, nullptr, dx, dtype, rows, C, HW, scale_shift, mean_invstd, dgamma, dbeta, act, stream);
}
