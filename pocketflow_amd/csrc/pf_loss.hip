// K10 + K11: hard-label softmax cross-entropy and the distillation soft-label cross-entropy,
// forward AND backward in one row-wise kernel (one 256-thread workgroup per example; row
// reductions by 64-lane shuffles + 4-entry LDS).  Fixed summation order => bit-deterministic.
//
// Reference semantics restated here (paths under /root/reference):
//   nets/resnet_at_ilsvrc12.py:132   loss = tf.losses.softmax_cross_entropy(labels, outputs)
//   learners/distillation_helper.py:98-100
//       logits_soft = logits_pri / T ; labels_soft = softmax(logits_dst / T)
//       loss = loss_w_dst * tf.losses.softmax_cross_entropy(labels_soft, logits_soft)
//   (tf.losses.softmax_cross_entropy: per-example -sum_c l_c log_softmax(z)_c, mean over batch)
#include "pf_common.h"

__device__ __forceinline__ float block_max(float v, float* lds) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) lds[w] = v;
  __syncthreads();
  v = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
  __syncthreads();
  return v;
}

// block-wide FIRST arg-max (largest value, smallest index among equals) for a 256-thread block; valid in every thread
__device__ __forceinline__ int block_first_argmax(float v, int i) {
  __shared__ float lv[4];
  __shared__ int li[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) { lv[w] = v; li[w] = i; }
  __syncthreads();
  v = lv[0]; i = li[0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (lv[k] > v || (lv[k] == v && li[k] < i)) { v = lv[k]; i = li[k]; }
  __syncthreads();
  return i;
}

// HEAD = false: dz = both terms of dlogits summed, row_ws = {ce, ced} per row (pf_ce_distill_fwd_bwd; dz_soft is never loaded).
// HEAD = true: real labels AND the teacher in the training step's one loss launch (pf_ce_distill_head).  The two terms of dz are
// stored SEPARATELY, each rounded to TD (dz = hard term, dz_soft = soft term; the upstream gradients of the two losses are device
// scalars, k_ce_combine joins them), and row_ws has THREE floats per row: ce, ced and the row's rank = the number of logits
// strictly greater than the logit at the FIRST arg-max of the label row (tf.nn.in_top_k: in the top k  <=>  rank < k).  Every other
// expression is shared: the losses and both terms equal those of one HEAD = false launch without the teacher and one with the
// teacher and zero labels.
template <typename TS, typename TT, typename TD, bool DST, bool HEAD>
__global__ __launch_bounds__(PF_THREADS) void k_ce_distill(const TS* __restrict__ z_s,
                                                           const float* __restrict__ labels,
                                                           const TT* __restrict__ z_t, int B, int C,
                                                           float T, float loss_w,
                                                           TD* __restrict__ dz, float* __restrict__ row_ws,
                                                           TD* __restrict__ dz_soft) {
  __shared__ float lds[4];
  const int b = blockIdx.x;
  const TS* __restrict__ zs = z_s + (int64_t)b * C;
  const float* __restrict__ lab = labels + (int64_t)b * C;
  const TT* __restrict__ zt = DST ? (z_t + (int64_t)b * C) : nullptr;
  TD* __restrict__ d = dz + (int64_t)b * C;
  TD* __restrict__ d2 = (HEAD && DST) ? (dz_soft + (int64_t)b * C) : nullptr;

  // pass 1: row maxima
  float ms = -INFINITY, mt = -INFINITY;
  float lbest = -INFINITY;
  int ibest = 0x7FFFFFFF;
  for (int c = threadIdx.x; c < C; c += PF_THREADS) {
    ms = fmaxf(ms, load_one<TS>(zs + c));
    if (DST) mt = fmaxf(mt, load_one<TT>(zt + c));
    if (HEAD) {
      const float l = lab[c];
      if (l > lbest) { lbest = l; ibest = c; }       // ascending c per thread: the first of equals stays
    }
  }
  ms = block_max(ms, lds);
  if (DST) mt = block_max(mt, lds);
  const float msT = ms / T, mtT = mt / T;
  float tscore = 0.f, rank = 0.f;
  if (HEAD) {
    const int target = block_first_argmax(lbest, ibest);
    tscore = load_one<TS>(zs + (target < C ? target : 0));    // (a row of NaN / -inf labels: column 0)
  }

  // pass 2: sums of exponentials (hard: z_s ; soft: z_s/T and z_t/T) and sum of labels
  float se = 0.f, seT = 0.f, stT = 0.f, sl = 0.f;
  for (int c = threadIdx.x; c < C; c += PF_THREADS) {
    const float z = load_one<TS>(zs + c);
    se += expf(z - ms);
    sl += lab[c];
    if (HEAD) rank += (z > tscore) ? 1.0f : 0.0f;     // a count <= C < 2^24: exact in float32
    if (DST) {
      seT += expf(z / T - msT);
      stT += expf(load_one<TT>(zt + c) / T - mtT);
    }
  }
  se = block_sum(se, lds);
  sl = block_sum(sl, lds);
  if (DST) { seT = block_sum(seT, lds); stT = block_sum(stT, lds); }
  if (HEAD) rank = block_sum(rank, lds);
  const float lse = logf(se);
  const float lseT = DST ? logf(seT) : 0.f;

  // pass 3: per-example losses + dlogits
  const float invB = 1.0f / (float)B;
  const float wBT = DST ? (loss_w / ((float)B * T)) : 0.f;
  float ce = 0.f, ced = 0.f;
  for (int c = threadIdx.x; c < C; c += PF_THREADS) {
    const float z = load_one<TS>(zs + c);
    const float l = lab[c];
    const float lsm = (z - ms) - lse;                 // log_softmax(z_s)_c
    ce -= l * lsm;
    float g = (expf(lsm) * sl - l) * invB;
    if (DST) {
      const float lsmT = (z / T - msT) - lseT;        // log_softmax(z_s / T)_c
      const float pt = expf(load_one<TT>(zt + c) / T - mtT) / stT;   // softmax(z_t / T)_c
      ced -= pt * lsmT;
      // HEAD: what the sum below makes of zero labels, (+0) + wBT * (...), so a -0 product is stored as +0
      if (HEAD) store_one<TD>(d2 + c, 0.0f + wBT * (expf(lsmT) - pt));
      else g += wBT * (expf(lsmT) - pt);
    }
    store_one<TD>(d + c, g);
  }
  ce = block_sum(ce, lds);
  if (DST) ced = block_sum(ced, lds);
  if (threadIdx.x == 0) {
    const int W = HEAD ? 3 : 2;
    row_ws[W * b] = ce; row_ws[W * b + 1] = ced;
    if (HEAD) row_ws[W * b + 2] = rank;
  }
}

// losses[0] / losses[1] = the two loss terms.  HEAD (three floats per row): losses[2] / losses[3] = the top-1 / top-5 accuracy of
// the batch, (number of rows with rank < k) times float32(1 / B): the form of a float32 mean over B zeros and ones (an exact count
// scaled by the rounded reciprocal).
template <bool HEAD>
__global__ __launch_bounds__(PF_THREADS) void k_loss_finalize(const float* __restrict__ row_ws, int B,
                                                              float loss_w, float* __restrict__ losses) {
  __shared__ float lds[4];
  const int W = HEAD ? 3 : 2;
  float a = 0.f, d = 0.f, t1 = 0.f, t5 = 0.f;
  for (int b = threadIdx.x; b < B; b += PF_THREADS) {
    a += row_ws[W * b]; d += row_ws[W * b + 1];
    if (HEAD) {
      const float r = row_ws[W * b + 2];
      t1 += r < 1.0f ? 1.0f : 0.0f;
      t5 += r < 5.0f ? 1.0f : 0.0f;
    }
  }
  a = block_sum(a, lds);
  d = block_sum(d, lds);
  if (HEAD) { t1 = block_sum(t1, lds); t5 = block_sum(t5, lds); }
  if (threadIdx.x == 0) {
    losses[0] = a / (float)B;
    losses[1] = loss_w * (d / (float)B);
    if (HEAD) {
      const float inv = 1.0f / (float)B;
      losses[2] = t1 * inv;
      losses[3] = t5 * inv;
    }
  }
}

template <bool HEAD>
static int launch_ce_distill(const void* z_s, int zs_dtype, const float* labels, const void* z_t, int zt_dtype, int B,
                             int C, float tempr, float loss_w, float* losses, void* dz, void* dz_soft, int dz_dtype,
                             float* row_ws, hipStream_t st) {
#define PF_CE(TS, TT, TD)                                                                                   \
  do {                                                                                                      \
    if (z_t) k_ce_distill<TS, TT, TD, true, HEAD><<<B, PF_THREADS, 0, st>>>((const TS*)z_s, labels, (const TT*)z_t, B, C, tempr, loss_w, (TD*)dz, row_ws, (TD*)dz_soft); \
    else k_ce_distill<TS, TT, TD, false, HEAD><<<B, PF_THREADS, 0, st>>>((const TS*)z_s, labels, (const TT*)nullptr, B, C, tempr, loss_w, (TD*)dz, row_ws, (TD*)nullptr); \
  } while (0)
  const int key = zs_dtype * 4 + (z_t ? zt_dtype : zs_dtype) * 2 + dz_dtype;
  switch (key) {
    case 0: PF_CE(float, float, float); break;
    case 1: PF_CE(float, float, bf16_t); break;
    case 2: PF_CE(float, bf16_t, float); break;
    case 3: PF_CE(float, bf16_t, bf16_t); break;
    case 4: PF_CE(bf16_t, float, float); break;
    case 5: PF_CE(bf16_t, float, bf16_t); break;
    case 6: PF_CE(bf16_t, bf16_t, float); break;
    case 7: PF_CE(bf16_t, bf16_t, bf16_t); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef PF_CE
  k_loss_finalize<HEAD><<<1, PF_THREADS, 0, st>>>(row_ws, B, z_t ? loss_w : 0.0f, losses);
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_ce_distill_fwd_bwd(const void* z_s, int zs_dtype, const float* labels,
                                     const void* z_t, int zt_dtype, int B, int C, float tempr,
                                     float loss_w, float* losses, void* dz_s, int dz_dtype,
                                     float* row_ws, void* stream) {
  if (B <= 0 || C <= 0) return (int)hipErrorInvalidValue;
  return launch_ce_distill<false>(z_s, zs_dtype, labels, z_t, zt_dtype, B, C, tempr, loss_w, losses, dz_s, nullptr, dz_dtype,
                                  row_ws, (hipStream_t)stream);
}

extern "C" int pf_ce_distill_head(const void* z_s, int zs_dtype, const float* labels, const void* z_t,
                                  int zt_dtype, int B, int C, float tempr, float loss_w, float* losses,
                                  void* dz_hard, void* dz_soft, int dz_dtype, float* row_ws, void* stream) {
  if (B <= 0 || C <= 0 || B >= (1 << 24) || C >= (1 << 24) || (z_t && !dz_soft)) return (int)hipErrorInvalidValue;
  return launch_ce_distill<true>(z_s, zs_dtype, labels, z_t, zt_dtype, B, C, tempr, loss_w, losses, dz_hard, dz_soft, dz_dtype,
                                 row_ws, (hipStream_t)stream);
}

// backward of the one loss launch: dz = T( T(hard * T(g0)) + T(soft * T(g1)) ), g0 / g1 = the upstream gradients of the two loss
// terms (float32 device scalars) -- the roundings of `dz * g.to(dz.dtype)` per term and of the sum autograd forms of the two
// products.  A NULL scalar (or soft == NULL) drops its term: dz = T(hard * T(g0)) alone is what one term gave before.
template <typename T>
__global__ __launch_bounds__(PF_THREADS) void k_ce_combine(const T* __restrict__ hard, const T* __restrict__ soft,
                                                           const float* __restrict__ g0, const float* __restrict__ g1,
                                                           T* __restrict__ dz, int64_t n) {
  const bool h = g0 != nullptr, s = soft != nullptr && g1 != nullptr;
  const float a = h ? round_to<T>(*g0) : 0.f, b = s ? round_to<T>(*g1) : 0.f;
  for (int64_t e = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * PF_THREADS) {
    float r;
    if (h && s) r = round_to<T>(load_one<T>(hard + e) * a) + round_to<T>(load_one<T>(soft + e) * b);
    else if (h) r = load_one<T>(hard + e) * a;
    else r = load_one<T>(soft + e) * b;
    store_one<T>(dz + e, r);
  }
}

extern "C" int pf_ce_combine(const void* dz_hard, const void* dz_soft, const float* g0, const float* g1, void* dz,
                             int dtype, int64_t n, void* stream) {
  if (n <= 0 || !dz_hard || !dz || (!g0 && !(dz_soft && g1))) return (int)hipErrorInvalidValue;
  const int grid = pf_grid_for(n, PF_THREADS);
  if (dtype == PF_F32) k_ce_combine<float><<<grid, PF_THREADS, 0, (hipStream_t)stream>>>((const float*)dz_hard, (const float*)dz_soft, g0, g1, (float*)dz, n);
  else if (dtype == PF_BF16) k_ce_combine<bf16_t><<<grid, PF_THREADS, 0, (hipStream_t)stream>>>((const bf16_t*)dz_hard, (const bf16_t*)dz_soft, g0, g1, (bf16_t*)dz, n);
  else return (int)hipErrorInvalidValue;
  PF_LAUNCH_CHECK();
  return 0;
}
