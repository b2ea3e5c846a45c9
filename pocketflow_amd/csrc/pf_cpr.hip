// Channel selection of the 'chn-pruned-rmt' learner (reference learners/channel_pruning_rmt/learner.py): per convolution layer,
//   1. gather   -- the kh x kw input patches of the pruned network and the c_out output vectors of the full network at drawn output
//                  positions (__smpl_inputs_n_outputs :651-725), P[rows][kh*kw][c_in] and Y[rows][c_out] float32 (a copy: bit-exact);
//   2. Gram     -- X[n*c_out + o][c] = sum_k P[n][k][c] * W[k][c][o] over a secondary sample of rows, X^T X and X^T y in float64,
//                  both divided by ||X^T X||_F and cast to float32 (__solve_sparse_regression :727-772);
//   3. ISTA     -- m <- prox(m - lr * (A m - b), gamma * lr), cpr_ista_nb_iters float32 iterations per solve (:449-468, :774-813);
//   4. lstsq    -- cpr_lstsq_nb_iters Adam steps on  X^T (X W - Y) / N + wd * W  with X = P restricted to the kept channels
//                  (__build_meta_lstsq :470-523, :815-841).
// Every reduction has a fixed order: results do not depend on the schedule.  No workgroup waits on another.
#include "pf_common.h"

#define CPR_T 256

// ================================================================================================================================
// 1. gather.  Rows are crop-major, then batch: row = row0 + crop * B + b.  x: [B][H][W][C] (NHWC storage), y: [B][OH][OW][Co].
// The patch of output position (oh, ow) starts at input (oh * stride - pad_t, ow * stride - pad_l); taps outside [0, H) x [0, W) are
// zeros, which is what the reference's zero-initialised patch buffer holds there (and what a fixed-padded copy of x holds).
// ================================================================================================================================
template <typename TX, typename TY>
__global__ __launch_bounds__(CPR_T) void k_cpr_gather(const TX* __restrict__ x, const TY* __restrict__ y, const int* __restrict__ pos, int crops,
                                                      int B, int H, int W, int C, int OH, int OW, int Co, int kh, int kw, int stride, int pad_t,
                                                      int pad_l, float* __restrict__ P, float* __restrict__ Yo, int64_t row0) {
  const int kk = kh * kw;
  const int64_t n_rows = (int64_t)crops * B;
  const int64_t n_p = n_rows * kk * C, n_y = n_rows * Co;
  for (int64_t i = (int64_t)blockIdx.x * CPR_T + threadIdx.x; i < n_p + n_y; i += (int64_t)gridDim.x * CPR_T) {
    if (i < n_p) {
      const int c = (int)(i % C);
      const int k = (int)((i / C) % kk);
      const int64_t r = i / ((int64_t)C * kk);
      const int crop = (int)(r / B), b = (int)(r % B);
      const int oh = pos[2 * crop], ow = pos[2 * crop + 1];
      const int ih = oh * stride - pad_t + k / kw, iw = ow * stride - pad_l + k % kw;
      float v = 0.f;
      if (oh >= 0 && oh < OH && ow >= 0 && ow < OW && ih >= 0 && ih < H && iw >= 0 && iw < W)
        v = load_one<TX>(x + (((int64_t)b * H + ih) * W + iw) * C + c);
      P[(row0 + r) * kk * C + (int64_t)k * C + c] = v;
    } else {
      const int64_t j = i - n_p;
      const int o = (int)(j % Co);
      const int64_t r = j / Co;
      const int crop = (int)(r / B), b = (int)(r % B);
      const int oh = pos[2 * crop], ow = pos[2 * crop + 1];
      float v = 0.f;
      if (oh >= 0 && oh < OH && ow >= 0 && ow < OW) v = load_one<TY>(y + (((int64_t)b * OH + oh) * OW + ow) * Co + o);
      Yo[(row0 + r) * Co + o] = v;
    }
  }
}

template <typename TX>
static int launch_gather_y(const TX* x, const void* y, int y_dtype, const int* pos, int crops, int B, int H, int W, int C, int OH, int OW,
                           int Co, int kh, int kw, int stride, int pad_t, int pad_l, float* P, float* Y, int64_t row0, hipStream_t st) {
  const int64_t n = (int64_t)crops * B * ((int64_t)kh * kw * C + Co);
  const int grid = pf_grid_for(n, CPR_T);
  if (y_dtype == PF_F32)
    k_cpr_gather<TX, float><<<grid, CPR_T, 0, st>>>(x, (const float*)y, pos, crops, B, H, W, C, OH, OW, Co, kh, kw, stride, pad_t, pad_l, P, Y, row0);
  else if (y_dtype == PF_BF16)
    k_cpr_gather<TX, bf16_t><<<grid, CPR_T, 0, st>>>(x, (const bf16_t*)y, pos, crops, B, H, W, C, OH, OW, Co, kh, kw, stride, pad_t, pad_l, P, Y,
                                                     row0);
  else
    return (int)hipErrorInvalidValue;
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_cpr_gather(const void* x, int x_dtype, const void* y, int y_dtype, const int* pos, int crops, int B, int H, int W, int C,
                             int OH, int OW, int Co, int kh, int kw, int stride, int pad_t, int pad_l, float* P, float* Y, int64_t row0,
                             void* stream) {
  if (x == nullptr || y == nullptr || pos == nullptr || P == nullptr || Y == nullptr || crops <= 0 || B <= 0 || H <= 0 || W <= 0 || C <= 0 ||
      OH <= 0 || OW <= 0 || Co <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || row0 < 0)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == PF_F32)
    return launch_gather_y<float>((const float*)x, y, y_dtype, pos, crops, B, H, W, C, OH, OW, Co, kh, kw, stride, pad_t, pad_l, P, Y, row0, st);
  if (x_dtype == PF_BF16)
    return launch_gather_y<bf16_t>((const bf16_t*)x, y, y_dtype, pos, crops, B, H, W, C, OH, OW, Co, kh, kw, stride, pad_t, pad_l, P, Y, row0, st);
  return (int)hipErrorInvalidValue;
}

// ================================================================================================================================
// 2. Gram.  The feature matrix is extended by the response as one more column, Xe = [X | y] with Ce = C + 1 columns, so one
// symmetric product Xe^T Xe holds X^T X (the leading C x C block) and X^T y (column C).  Xe is materialised in float64 in chunks of
// CPR_GRAM_CHUNK rows (row r = n * Co + o of the secondary sample); a chunk's product is split over S row ranges into partial tiles
// (upper-triangular 64 x 64 tiles only: entry (c1, c2) and (c2, c1) are the same products in the same order), the partials are added
// into the float64 accumulator in split order.  float64 FMA throughout, as the reference computes this in NumPy float64.
// ================================================================================================================================
#define CPR_GRAM_CHUNK 8192
#define CPR_GT 64            // Gram tile edge
#define CPR_GK 16            // rows per LDS stage

static inline int cpr_gram_tiles(int Ce) { const int t = (Ce + CPR_GT - 1) / CPR_GT; return t * (t + 1) / 2; }
static inline int cpr_gram_splits(int Ce) {
  int s = 512 / cpr_gram_tiles(Ce);
  if (s < 1) s = 1;
  if (s > 16) s = 16;
  return s;
}

__global__ __launch_bounds__(CPR_T) void k_cpr_feat(const float* __restrict__ P, const float* __restrict__ Y, const int* __restrict__ idx,
                                                    const float* __restrict__ w, int kk, int C, int Co, int64_t r0, int64_t r1,
                                                    double* __restrict__ xe) {
  const int Ce = C + 1;
  const int64_t n_el = (r1 - r0) * Ce;
  for (int64_t i = (int64_t)blockIdx.x * CPR_T + threadIdx.x; i < n_el; i += (int64_t)gridDim.x * CPR_T) {
    const int c = (int)(i % Ce);
    const int64_t r = r0 + i / Ce;
    const int64_t n = idx[r / Co];
    const int o = (int)(r % Co);
    double v;
    if (c < C) {
      const float* p = P + n * kk * C + c;
      const float* wk = w + (int64_t)o * kk * C + c;      // KRSC: W[o][k][c]
      v = 0.0;
      for (int k = 0; k < kk; ++k) v = fma((double)p[(int64_t)k * C], (double)wk[(int64_t)k * C], v);
    } else {
      v = (double)Y[n * Co + o];
    }
    xe[i] = v;
  }
}

// partial[s][a][b] (a, b in the tile pair (ti <= tj)) = sum over rows of split s of xe[r][a] * xe[r][b]
__global__ __launch_bounds__(CPR_T) void k_cpr_gram_tile(const double* __restrict__ xe, int64_t rows, int Ce, double* __restrict__ partial) {
  __shared__ double sa[CPR_GK][CPR_GT];
  __shared__ double sb[CPR_GK][CPR_GT];
  int t = blockIdx.x, ti = 0;
  const int T = (Ce + CPR_GT - 1) / CPR_GT;
  while (t >= T - ti) { t -= T - ti; ++ti; }
  const int tj = ti + t;
  const int S = gridDim.y, s = blockIdx.y;
  const int64_t per = (rows + S - 1) / S;
  const int64_t ra = (int64_t)s * per, rb = (ra + per < rows) ? ra + per : rows;
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  double acc[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int64_t r = ra; r < rb; r += CPR_GK) {
    for (int e = threadIdx.x; e < CPR_GK * CPR_GT; e += CPR_T) {
      const int kr = e / CPR_GT, cc = e % CPR_GT;
      const int64_t rr = r + kr;
      const int ca = ti * CPR_GT + cc, cb = tj * CPR_GT + cc;
      const bool ok = rr < rb;
      sa[kr][cc] = (ok && ca < Ce) ? xe[rr * Ce + ca] : 0.0;
      sb[kr][cc] = (ok && cb < Ce) ? xe[rr * Ce + cb] : 0.0;
    }
    __syncthreads();
    for (int kr = 0; kr < CPR_GK; ++kr) {
      double a[4], b[4];
      for (int i = 0; i < 4; ++i) a[i] = sa[kr][ty + 16 * i];
      for (int j = 0; j < 4; ++j) b[j] = sb[kr][tx + 16 * j];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  double* out = partial + ((int64_t)s * gridDim.x + blockIdx.x) * CPR_GT * CPR_GT;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) out[(ty + 16 * i) * CPR_GT + tx + 16 * j] = acc[i][j];
}

static __device__ __forceinline__ int cpr_tile_index(int ti, int tj, int T) { return ti * T - ti * (ti - 1) / 2 + (tj - ti); }

// acc[a][b] += sum_s partial[s][tile(a, b)] (in split order); the lower triangle reads the mirrored entry
__global__ __launch_bounds__(CPR_T) void k_cpr_gram_add(const double* __restrict__ partial, int S, int n_tiles, int Ce, double* __restrict__ acc) {
  const int T = (Ce + CPR_GT - 1) / CPR_GT;
  const int64_t n = (int64_t)Ce * Ce;
  for (int64_t i = (int64_t)blockIdx.x * CPR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * CPR_T) {
    int a = (int)(i / Ce), b = (int)(i % Ce);
    if (a / CPR_GT > b / CPR_GT) { const int tmp = a; a = b; b = tmp; }
    const int tile = cpr_tile_index(a / CPR_GT, b / CPR_GT, T);
    const int64_t off = (int64_t)tile * CPR_GT * CPR_GT + (a % CPR_GT) * CPR_GT + (b % CPR_GT);
    double v = acc[i];
    for (int s = 0; s < S; ++s) v += partial[(int64_t)s * n_tiles * CPR_GT * CPR_GT + off];
    acc[i] = v;
  }
}

// one workgroup: norm[0] = sqrt(sum of squares of the leading C x C block), per-thread strided sums, then a fixed tree
__global__ __launch_bounds__(CPR_T) void k_cpr_gram_norm(const double* __restrict__ acc, int C, double* __restrict__ norm) {
  __shared__ double red[CPR_T];
  const int Ce = C + 1;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < (int64_t)C * C; i += CPR_T) {
    const double v = acc[(i / C) * Ce + i % C];
    s = fma(v, v, s);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = CPR_T / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) norm[0] = sqrt(red[0]);
}

__global__ __launch_bounds__(CPR_T) void k_cpr_gram_scale(const double* __restrict__ acc, const double* __restrict__ norm, int C,
                                                          float* __restrict__ xtx, float* __restrict__ xty) {
  const int Ce = C + 1;
  const double nrm = norm[0];
  const int64_t n = (int64_t)C * Ce;
  for (int64_t i = (int64_t)blockIdx.x * CPR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * CPR_T) {
    const int a = (int)(i / Ce), b = (int)(i % Ce);
    const float v = (float)(acc[i] / nrm);
    if (b < C) xtx[(int64_t)a * C + b] = v;
    else xty[a] = v;
  }
}

extern "C" int64_t pf_cpr_gram_ws(int C) {
  const int Ce = C + 1;
  return (int64_t)Ce * Ce + (int64_t)cpr_gram_splits(Ce) * cpr_gram_tiles(Ce) * CPR_GT * CPR_GT + (int64_t)CPR_GRAM_CHUNK * Ce + 1;
}

extern "C" int pf_cpr_gram(const float* P, const float* Y, const int* idx, int64_t n, int kk, int C, int Co, const float* w, double* ws,
                           int64_t ws_elems, float* xtx, float* xty, void* stream) {
  if (P == nullptr || Y == nullptr || idx == nullptr || w == nullptr || ws == nullptr || xtx == nullptr || xty == nullptr || n <= 0 || kk <= 0 ||
      C <= 0 || Co <= 0 || ws_elems < pf_cpr_gram_ws(C))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int Ce = C + 1;
  const int S = cpr_gram_splits(Ce), n_tiles = cpr_gram_tiles(Ce);
  double* acc = ws;
  double* partial = acc + (int64_t)Ce * Ce;
  double* xe = partial + (int64_t)S * n_tiles * CPR_GT * CPR_GT;
  double* norm = xe + (int64_t)CPR_GRAM_CHUNK * Ce;
  if (hipMemsetAsync(acc, 0, sizeof(double) * Ce * Ce, st) != hipSuccess) return (int)hipErrorInvalidValue;
  const int64_t rows = n * Co;
  for (int64_t r0 = 0; r0 < rows; r0 += CPR_GRAM_CHUNK) {
    const int64_t r1 = (r0 + CPR_GRAM_CHUNK < rows) ? r0 + CPR_GRAM_CHUNK : rows;
    k_cpr_feat<<<pf_grid_for((r1 - r0) * Ce, CPR_T), CPR_T, 0, st>>>(P, Y, idx, w, kk, C, Co, r0, r1, xe);
    PF_LAUNCH_CHECK();
    k_cpr_gram_tile<<<dim3((unsigned)n_tiles, (unsigned)S, 1), CPR_T, 0, st>>>(xe, r1 - r0, Ce, partial);
    PF_LAUNCH_CHECK();
    k_cpr_gram_add<<<pf_grid_for((int64_t)Ce * Ce, CPR_T), CPR_T, 0, st>>>(partial, S, n_tiles, Ce, acc);
    PF_LAUNCH_CHECK();
  }
  k_cpr_gram_norm<<<1, CPR_T, 0, st>>>(acc, C, norm);
  PF_LAUNCH_CHECK();
  k_cpr_gram_scale<<<pf_grid_for((int64_t)C * Ce, CPR_T), CPR_T, 0, st>>>(acc, norm, C, xtx, xty);
  PF_LAUNCH_CHECK();
  return 0;
}

// ================================================================================================================================
// 3. ISTA.  One launch per iteration: a wavefront per row c of A computes t = (A m)[c] (lane-strided fmaf, fixed butterfly), then
// TF's per-op chain  t = t - b; t = lr * t; g = m - t;  and the soft threshold of the reference's nested tf.where with thr = gamma * lr.
// Two mask buffers ping-pong; the last iteration writes the caller's mask and counts its non-zeros (integer atomics: exact).
// ================================================================================================================================
__global__ __launch_bounds__(CPR_T) void k_cpr_ista_iter(const float* __restrict__ A, const float* __restrict__ b, const float* __restrict__ m_in,
                                                         float* __restrict__ m_out, int C, float lr, float thr, int* __restrict__ nnz) {
  const int lane = threadIdx.x % PF_WAVE;
  const int c = blockIdx.x * (CPR_T / PF_WAVE) + threadIdx.x / PF_WAVE;
  if (c >= C) return;
  const float* a = A + (int64_t)c * C;
  float s = 0.f;
  for (int j = lane; j < C; j += PF_WAVE) s = fmaf(a[j], m_in[j], s);
  for (int off = PF_WAVE / 2; off > 0; off >>= 1) s = s + __shfl_xor(s, off, PF_WAVE);
  if (lane != 0) return;
  float t = s - b[c];
  t = lr * t;
  const float g = m_in[c] - t;
  const float v = g > thr ? g - thr : (g < -thr ? g + thr : 0.f);
  m_out[c] = v;
  if (nnz != nullptr && v != 0.f) atomicAdd(nnz, 1);
}

extern "C" int pf_cpr_ista(const float* A, const float* b, const float* m0, float* m_ws, float* mask, int C, float gamma, float lr, int iters,
                           int* nnz, void* stream) {
  if (A == nullptr || b == nullptr || m0 == nullptr || m_ws == nullptr || mask == nullptr || nnz == nullptr || C <= 0 || iters <= 0)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const float thr = gamma * lr;
  if (hipMemsetAsync(nnz, 0, sizeof(int), st) != hipSuccess) return (int)hipErrorInvalidValue;
  const int grid = (C + CPR_T / PF_WAVE - 1) / (CPR_T / PF_WAVE);
  for (int it = 0; it < iters; ++it) {
    const float* in = it == 0 ? m0 : m_ws + (int64_t)((it - 1) & 1) * C;
    float* out = it == iters - 1 ? mask : m_ws + (int64_t)(it & 1) * C;
    k_cpr_ista_iter<<<grid, CPR_T, 0, st>>>(A, b, in, out, C, lr, thr, it == iters - 1 ? nnz : nullptr);
    PF_LAUNCH_CHECK();
  }
  return 0;
}

// ================================================================================================================================
// 4. least squares.  P is [N][K] (K = kh*kw*C, HWIO order of the patch), W the [K][Co] matrix of the HWIO kernel; the kept columns
// of P (= rows of W) are listed in kidx[Kp].  Dropped columns hold exact zeros in the reference's x_mat, so they add exact zeros to
// both products: leaving them out changes no kept value.
//   resid:  R[n][o] = (sum_j P[n][kidx[j]] * W[kidx[j]][o]) - Y[n][o]
//   grad:   part[s][j][o] = sum_{n in split s} P[n][kidx[j]] * R[n][o]         (split-K over N, added in split order by adam)
//   adam:   g = (pos[r] < 0 ? 0 : sum_s part[s][pos[r]][o]) / N + wd * W;  m, v, W updated with TF's per-op rounding; c1 / c2 are the
//           float32 constants of (1 - beta1) / (1 - beta2), which the reference forms in double precision before TF rounds them.
// 64 x 64 output tiles, 16-deep LDS stages, 4 x 4 outputs per thread (strided by 16: conflict-free LDS reads), fmaf accumulation.
// ================================================================================================================================
#define CPR_MT 64
#define CPR_KT 16

__global__ __launch_bounds__(CPR_T) void k_cpr_resid(const float* __restrict__ P, int K, const int* __restrict__ kidx, int Kp,
                                                     const float* __restrict__ W, const float* __restrict__ Y, float* __restrict__ R, int64_t N,
                                                     int Co) {
  __shared__ float sa[CPR_KT][CPR_MT + 1];
  __shared__ float sb[CPR_KT][CPR_MT];
  const int64_t n0 = (int64_t)blockIdx.x * CPR_MT;
  const int o0 = blockIdx.y * CPR_MT;
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  float acc[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int j0 = 0; j0 < Kp; j0 += CPR_KT) {
    for (int e = threadIdx.x; e < CPR_KT * CPR_MT; e += CPR_T) {
      const int kr = e % CPR_KT, row = e / CPR_KT;         // A: consecutive threads along the patch row
      const int64_t n = n0 + row;
      const int j = j0 + kr;
      sa[kr][row] = (n < N && j < Kp) ? P[n * K + kidx[j]] : 0.f;
      const int kb = e / CPR_MT, col = e % CPR_MT;         // B: consecutive threads along the output channels
      const int jb = j0 + kb, o = o0 + col;
      sb[kb][col] = (jb < Kp && o < Co) ? W[(int64_t)kidx[jb] * Co + o] : 0.f;
    }
    __syncthreads();
    for (int kr = 0; kr < CPR_KT; ++kr) {
      float a[4], bv[4];
      for (int i = 0; i < 4; ++i) a[i] = sa[kr][ty + 16 * i];
      for (int j = 0; j < 4; ++j) bv[j] = sb[kr][tx + 16 * j];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
  for (int i = 0; i < 4; ++i) {
    const int64_t n = n0 + ty + 16 * i;
    if (n >= N) continue;
    for (int j = 0; j < 4; ++j) {
      const int o = o0 + tx + 16 * j;
      if (o < Co) R[n * Co + o] = acc[i][j] - Y[n * Co + o];
    }
  }
}

__global__ __launch_bounds__(CPR_T) void k_cpr_grad(const float* __restrict__ P, int K, const int* __restrict__ kidx, int Kp,
                                                    const float* __restrict__ R, int64_t N, int Co, float* __restrict__ part) {
  __shared__ float sa[CPR_KT][CPR_MT];
  __shared__ float sb[CPR_KT][CPR_MT];
  const int j0 = blockIdx.x * CPR_MT;
  const int o0 = blockIdx.y * CPR_MT;
  const int S = gridDim.z, s = blockIdx.z;
  const int64_t per = (N + S - 1) / S;
  const int64_t na = (int64_t)s * per, nb = (na + per < N) ? na + per : N;
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  float acc[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int64_t n0 = na; n0 < nb; n0 += CPR_KT) {
    for (int e = threadIdx.x; e < CPR_KT * CPR_MT; e += CPR_T) {
      const int kr = e / CPR_MT, col = e % CPR_MT;
      const int64_t n = n0 + kr;
      const int j = j0 + col, o = o0 + col;
      sa[kr][col] = (n < nb && j < Kp) ? P[n * K + kidx[j]] : 0.f;
      sb[kr][col] = (n < nb && o < Co) ? R[n * Co + o] : 0.f;
    }
    __syncthreads();
    for (int kr = 0; kr < CPR_KT; ++kr) {
      float a[4], bv[4];
      for (int i = 0; i < 4; ++i) a[i] = sa[kr][ty + 16 * i];
      for (int j = 0; j < 4; ++j) bv[j] = sb[kr][tx + 16 * j];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
  float* out = part + (int64_t)s * Kp * Co;
  for (int i = 0; i < 4; ++i) {
    const int j = j0 + ty + 16 * i;
    if (j >= Kp) continue;
    for (int jj = 0; jj < 4; ++jj) {
      const int o = o0 + tx + 16 * jj;
      if (o < Co) out[(int64_t)j * Co + o] = acc[i][jj];
    }
  }
}

__global__ __launch_bounds__(CPR_T) void k_cpr_adam(float* __restrict__ W, float* __restrict__ m, float* __restrict__ v,
                                                    const float* __restrict__ part, int S, const int* __restrict__ pos, int K, int Kp, int Co,
                                                    float n_smpls, float wd, float lr_t, float b1, float c1, float b2, float c2, float eps) {
  const int64_t n = (int64_t)K * Co;
  for (int64_t i = (int64_t)blockIdx.x * CPR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * CPR_T) {
    const int r = (int)(i / Co), o = (int)(i % Co);
    const int p = pos[r];
    float g = 0.f;
    if (p >= 0) {
      g = part[(int64_t)p * Co + o];
      for (int s = 1; s < S; ++s) g = g + part[((int64_t)s * Kp + p) * Co + o];
    }
    const float w = W[i];
    g = g / n_smpls;
    g = g + wd * w;                                           // grad = X^T R / N + loss_w_dcy * W
    const float mi = b1 * m[i] + c1 * g;                       // gacc1 = beta1 * gacc1 + (1 - beta1) * grad
    const float vi = b2 * v[i] + c2 * (g * g);                 // gacc2 = beta2 * gacc2 + (1 - beta2) * grad ** 2
    m[i] = mi;
    v[i] = vi;
    W[i] = w + (-lr_t * mi) / (sqrtf(vi) + eps);               // assign_add(-lrn_rate * gacc1 / (sqrt(gacc2) + epsilon))
  }
}

extern "C" int pf_cpr_lstsq_splits(int64_t N, int Kp, int Co) {
  const int64_t tiles = (int64_t)((Kp + CPR_MT - 1) / CPR_MT) * ((Co + CPR_MT - 1) / CPR_MT);
  int64_t s = tiles > 0 ? (1024 + tiles - 1) / tiles : 1;     // ~1024 workgroups in flight ...
  if (s > N / 512) s = N / 512;                                // ... and at least 512 rows per split
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  return (int)s;
}

extern "C" int pf_cpr_lstsq_step(const float* P, int K, const int* kidx, const int* pos, int Kp, const float* Y, float* R, int64_t N, int Co,
                                 float* W, float* m, float* v, float* part, float wd, float lr_t, float beta1, float beta2, float c1,
                                 float c2, float eps, void* stream) {
  if (P == nullptr || kidx == nullptr || pos == nullptr || Y == nullptr || R == nullptr || W == nullptr || m == nullptr || v == nullptr ||
      part == nullptr || K <= 0 || Kp < 0 || Kp > K || N <= 0 || Co <= 0)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  k_cpr_resid<<<dim3((unsigned)((N + CPR_MT - 1) / CPR_MT), (unsigned)((Co + CPR_MT - 1) / CPR_MT), 1), CPR_T, 0, st>>>(P, K, kidx, Kp, W, Y, R,
                                                                                                                      N, Co);
  PF_LAUNCH_CHECK();
  const int S = pf_cpr_lstsq_splits(N, Kp, Co);
  if (Kp > 0) {
    k_cpr_grad<<<dim3((unsigned)((Kp + CPR_MT - 1) / CPR_MT), (unsigned)((Co + CPR_MT - 1) / CPR_MT), (unsigned)S), CPR_T, 0, st>>>(P, K, kidx, Kp, R,
                                                                                                                              N, Co, part);
    PF_LAUNCH_CHECK();
  }
  k_cpr_adam<<<pf_grid_for((int64_t)K * Co, CPR_T), CPR_T, 0, st>>>(W, m, v, part, S, pos, K, Kp, Co, (float)N, wd, lr_t, beta1, c1, beta2, c2,
                                                                  eps);
  PF_LAUNCH_CHECK();
  return 0;
}

// R = X_kept W - Y alone (the losses the reference logs before and after the Adam steps)
extern "C" int pf_cpr_lstsq_resid(const float* P, int K, const int* kidx, int Kp, const float* W, const float* Y, float* R, int64_t N, int Co,
                                  void* stream) {
  if (P == nullptr || kidx == nullptr || W == nullptr || Y == nullptr || R == nullptr || K <= 0 || Kp < 0 || Kp > K || N <= 0 || Co <= 0)
    return (int)hipErrorInvalidValue;
  k_cpr_resid<<<dim3((unsigned)((N + CPR_MT - 1) / CPR_MT), (unsigned)((Co + CPR_MT - 1) / CPR_MT), 1), CPR_T, 0, (hipStream_t)stream>>>(
      P, K, kidx, Kp, W, Y, R, N, Co);
  PF_LAUNCH_CHECK();
  return 0;
}
