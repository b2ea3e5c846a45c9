// The residual join of a ResNet-v1 block: batch-norm (no activation of its own) + shortcut + ReLU, forward and the
// gate pass of the backward, over NHWC activations viewed as a [rows][C] matrix.
//
//   forward : u = act(fmaf(scale[c], x, shift[c]) + r), ONE rounding to the storage type on the store (float32 storage: the
//             float32 operations as written; bf16 storage: the exact value rounded once, see bj_value_f64);
//             with a slot also the whole-tensor min / max of u AS STORED, folded into the slot (the range the quantiser
//             pf_uq_apply reads) -- 2 reads + 1 write per element instead of the BN apply pass, the sum, the activation's
//             min/max pass and its read of the sum (4 reads + 2 writes).
//   backward: g = dq * [fmaf(scale, x, shift) + r > 0], the gate recomputed from x and r (the quantised output does not
//             carry it: small positive values round to code 0), plus the per-block sums {sum g, sum g * xhat} in the
//             layout pf_bn_bwd_finalize reads.  pf_bn_bwd_finalize and pf_bn_bwd_apply(act = none) on g then give dx /
//             dgamma / dbeta of the BN; g itself is the shortcut's gradient.
//
// Reference semantics restated here (utils/external/resnet_model.py:202-254, _bottleneck_block_v1):
//   inputs = batch_norm(inputs, training, data_format); inputs += shortcut; inputs = tf.nn.relu(inputs)
//
// Work decomposition (both kernels): a 256-thread workgroup owns a SLAB of CG = min(C/8, 8) groups of 8 consecutive
// channels (16 B per lane for bf16, two 16-B accesses for float32; a wavefront reads whole 128-B lines) and one of
// `nsplit` interleaved row ranges; its 256 / CG row lanes walk the rows in a grid-stride loop.  scale / shift (and mean /
// invstd) of the 8 channels stay in registers.  The grid is capped (BJ_MAX_BLOCKS workgroups, at most BJ_MAX_SPLITS row
// splits, so that the partial sums [nsplit][2][C] stay a few MB and pf_bn_bwd_finalize a few microseconds).
#include "pf_common.h"

#define BJ_MAX_SPLITS 256
#define BJ_MAX_BLOCKS PF_MAX_GRID

struct BjPlan { int CG, RPS, nslab, nsplit; };

// rows > 0, C > 0, C % 8 == 0
static inline BjPlan bj_plan(int64_t rows, int C) {
  BjPlan p;
  const int G = C >> 3;
  p.CG = G < 8 ? G : 8;
  p.RPS = PF_THREADS / p.CG;                         // rows a workgroup covers per trip
  p.nslab = (G + p.CG - 1) / p.CG;
  int cap = BJ_MAX_BLOCKS / p.nslab;
  if (cap > BJ_MAX_SPLITS) cap = BJ_MAX_SPLITS;
  if (cap < 1) cap = 1;
  const int64_t need = (rows + p.RPS - 1) / p.RPS;   // one trip per workgroup until the cap, grid-stride beyond
  p.nsplit = (int)(need < cap ? need : cap);
  return p;
}

extern "C" int pf_bn_add_act_groups(int64_t rows, int C) {
  if (rows <= 0 || C <= 0 || (C % 8) != 0) return 0;
  return bj_plan(rows, C).nsplit;
}

// One output value in float32, ready for the store's single rounding to T.
// float32 storage: the three float32 operations of the unfused route (BN apply pass, add, ReLU), bit for bit.
// bf16 storage: fmaf and the add each round to float32, and the sum cancels (|u| < |scale * x + shift| for half of the elements), so
// the pair lands on the other side of a bf16 rounding boundary several times as often as the single fmaf of the BN apply pass does
// (11 against 3 elements of 8 * 10^5 on the 3137 x 256 test shape).  The kernel is HBM-bound with VALU slots to spare: the two
// operations run in float64 -- scale * x is exact there -- and the result goes to float32 with round-to-odd, which makes the store's
// round-to-nearest-even the ONE rounding of the exact value (float32 keeps 16 bits more than bf16).
template <typename T, int ACT>
__device__ __forceinline__ float bj_value_f32(float sc, float sh, float x, float r) {
  return apply_act<ACT>(fmaf(sc, x, sh) + r);
}
template <int ACT>
__device__ __forceinline__ float bj_value_f64(float sc, float sh, float x, float r) {
  double d = fma((double)sc, (double)x, (double)sh) + (double)r;
  if (ACT == PF_ACT_RELU) d = fmax(d, 0.0);
  float f = (float)d;                              // nearest
  const double back = (double)f;
  if (back != d) {                                 // inexact: truncate, then make the last bit odd
    uint32_t b = __float_as_uint(f);
    if (fabs(back) > fabs(d)) b -= 1u;
    f = __uint_as_float(b | 1u);
  }
  return f;
}

template <typename T, int ACT, bool SLOT>
__global__ __launch_bounds__(PF_THREADS) void k_bn_add_act_fwd(const T* __restrict__ x, const T* __restrict__ r,
                                                               T* __restrict__ u, int64_t rows, int C,
                                                               const float* __restrict__ scale_shift,
                                                               uint32_t* __restrict__ slot, int nslab, int nsplit, int CG) {
  __shared__ float lds[8];
  const int G = C >> 3, RPS = PF_THREADS / CG;
  const int slab = blockIdx.x % nslab, split = blockIdx.x / nslab;
  const int cg = slab * CG + (int)(threadIdx.x % CG), rl = threadIdx.x / CG;
  float mn = INFINITY, mx = -INFINITY;
  if (rl < RPS && cg < G) {
    const int c0 = cg << 3;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = scale_shift[c0 + j]; sh[j] = scale_shift[C + c0 + j]; }
#pragma unroll 2
    for (int64_t row = (int64_t)split * RPS + rl; row < rows; row += (int64_t)nsplit * RPS) {
      float v[8], s[8];
      const int64_t off = row * C + c0;
      load8<T>(x + off, v);
      load8<T>(r + off, s);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (std::is_same<T, float>::value) v[j] = bj_value_f32<T, ACT>(sc[j], sh[j], v[j], s[j]);
        else v[j] = bj_value_f64<ACT>(sc[j], sh[j], v[j], s[j]);
        if (SLOT) {
          const float q = round_to<T>(v[j]);         // the value the quantiser will read back
          mn = fminf(mn, q);
          mx = fmaxf(mx, q);
        }
      }
      store8<T>(u + off, v);
    }
  }
  if (SLOT) {
    block_minmax(mn, mx, lds);
    if (threadIdx.x == 0 && mn <= mx) {
      atomicMin(&slot[0], enc_f32(mn));
      atomicMin(&slot[1], ~enc_f32(mx));
    }
  }
}

// ADD: the block output has a second consumer (the next block's shortcut or projection) whose gradient arrives separately;
// dq + addend, rounded to the storage type as autograd's accumulation would store it, is gated in the same pass.
template <typename T, int ACT, bool ADD>
__global__ __launch_bounds__(PF_THREADS) void k_bn_add_act_bwd_gate(const T* __restrict__ dq, const T* __restrict__ addend,
                                                                    const T* __restrict__ x,
                                                                    const T* __restrict__ r, T* __restrict__ g,
                                                                    int64_t rows, int C,
                                                                    const float* __restrict__ scale_shift,
                                                                    const float* __restrict__ mean_invstd,
                                                                    float* __restrict__ partial, int nslab, int nsplit, int CG) {
  __shared__ float lds[2][PF_THREADS * 8];
  const int G = C >> 3, RPS = PF_THREADS / CG;
  const int slab = blockIdx.x % nslab, split = blockIdx.x / nslab;
  const int cg = slab * CG + (int)(threadIdx.x % CG), rl = threadIdx.x / CG;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  if (rl < RPS && cg < G) {
    const int c0 = cg << 3;
    float sc[8], sh[8], mu[8], is[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sc[j] = scale_shift[c0 + j]; sh[j] = scale_shift[C + c0 + j];
      mu[j] = mean_invstd[c0 + j]; is[j] = mean_invstd[C + c0 + j];
    }
#pragma unroll 2
    for (int64_t row = (int64_t)split * RPS + rl; row < rows; row += (int64_t)nsplit * RPS) {
      float d[8], v[8], s[8];
      const int64_t off = row * C + c0;
      load8<T>(dq + off, d);
      load8<T>(x + off, v);
      load8<T>(r + off, s);
      if (ADD) {
        float a[8];
        load8<T>(addend + off, a);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = round_to<T>(d[j] + a[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        d[j] = d[j] * act_mask<ACT>(fmaf(sc[j], v[j], sh[j]) + s[j]);     // 0 or dq: exact in the storage type
        s1[j] += d[j];
        s2[j] = fmaf(d[j], (v[j] - mu[j]) * is[j], s2[j]);
      }
      store8<T>(g + off, d);
    }
  }
  // the row lanes of a channel combine through LDS in ascending lane order: deterministic
#pragma unroll
  for (int j = 0; j < 8; ++j) { lds[0][threadIdx.x * 8 + j] = s1[j]; lds[1][threadIdx.x * 8 + j] = s2[j]; }
  __syncthreads();
  const int slabC = CG * 8;
  if ((int)threadIdx.x < slabC) {
    const int c = slab * slabC + (int)threadIdx.x;
    if (c < C) {
      float a = 0.f, b = 0.f;
      for (int l = 0; l < RPS; ++l) { a += lds[0][l * slabC + threadIdx.x]; b += lds[1][l * slabC + threadIdx.x]; }
      float* out = partial + (int64_t)split * 2 * C;
      out[c] = a;
      out[C + c] = b;
    }
  }
}

static inline bool bj_shape_ok(int64_t rows, int C, int act) {
  return rows > 0 && C > 0 && (C % 8) == 0 && (act == PF_ACT_NONE || act == PF_ACT_RELU);
}
static inline bool bj_tensor_ok(const void* p) { return p != nullptr && pf_aligned16(p); }

extern "C" int pf_bn_add_act_fwd(const void* x, const void* r, void* u, int dtype, int64_t rows, int C,
                                 const float* scale_shift, int act, uint32_t* slot, void* stream) {
  if (!bj_shape_ok(rows, C, act) || !bj_tensor_ok(x) || !bj_tensor_ok(r) || !bj_tensor_ok(u) || scale_shift == nullptr)
    return (int)hipErrorInvalidValue;
  if (dtype != PF_F32 && dtype != PF_BF16) return (int)hipErrorInvalidValue;
  const BjPlan p = bj_plan(rows, C);
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    pf_with_act(act, [&](auto A) {
      pf_with_bool(slot != nullptr, [&](auto S) {
        k_bn_add_act_fwd<T, decltype(A)::value, decltype(S)::value><<<p.nslab * p.nsplit, PF_THREADS, 0, st>>>(
            (const T*)x, (const T*)r, (T*)u, rows, C, scale_shift, slot, p.nslab, p.nsplit, p.CG);
      });
    });
  };
  if (dtype == PF_F32) launch((float*)nullptr);
  else launch((bf16_t*)nullptr);
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_bn_add_act_bwd_gate_add(const void* dq, const void* addend, const void* x, const void* r, void* g, int dtype,
                                          int64_t rows, int C, const float* scale_shift, const float* mean_invstd, int act,
                                          float* partial, void* stream) {
  if (addend != nullptr && !pf_aligned16(addend)) return (int)hipErrorInvalidValue;
  if (!bj_shape_ok(rows, C, act) || !bj_tensor_ok(dq) || !bj_tensor_ok(x) || !bj_tensor_ok(r) || !bj_tensor_ok(g) ||
      scale_shift == nullptr || mean_invstd == nullptr || partial == nullptr)
    return (int)hipErrorInvalidValue;
  if (dtype != PF_F32 && dtype != PF_BF16) return (int)hipErrorInvalidValue;
  const BjPlan p = bj_plan(rows, C);
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    pf_with_act(act, [&](auto A) {
      pf_with_bool(addend != nullptr, [&](auto D) {
        k_bn_add_act_bwd_gate<T, decltype(A)::value, decltype(D)::value><<<p.nslab * p.nsplit, PF_THREADS, 0, st>>>(
            (const T*)dq, (const T*)addend, (const T*)x, (const T*)r, (T*)g, rows, C, scale_shift, mean_invstd, partial, p.nslab,
            p.nsplit, p.CG);
      });
    });
  };
  if (dtype == PF_F32) launch((float*)nullptr);
  else launch((bf16_t*)nullptr);
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_bn_add_act_bwd_gate(const void* dq, const void* x, const void* r, void* g, int dtype, int64_t rows,
                                      int C, const float* scale_shift, const float* mean_invstd, int act,
                                      float* partial, void* stream) {
  return pf_bn_add_act_bwd_gate_add(dq, nullptr, x, r, g, dtype, rows, C, scale_shift, mean_invstd, act, partial, stream);
}
