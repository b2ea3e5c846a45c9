// Dense layers on the matrix cores: Y[B][N] = X[B][K] W[N][K]^T + bias, dX = dY W, dW = dY^T X, db = column sums of dY.  bf16 storage,
// float32 accumulation, v_mfma_f32_16x16x32_bf16.  tf.layers.dense (graph.Dense) and MobileNet's logits: 2048 | 1280 | 1024 | 512 ->
// 1001, 64 -> 10, 1600 -> 256 -> 10.  What kept this layer off the MFMA kernels is the row pitch of Y / dY, N * 2 bytes: for N = 1001
// not a multiple of 16, nor of 4.  Here X, W, dX and dW (K % 32 == 0) are accessed in 16-byte pieces and Y / dY in 2- or 4-byte pieces;
// any N >= 1 and any B >= 1 are taken.
//
// Forward (k_dense_fwd).  Both operands are K-contiguous, so a 32-wide k-step takes its A (X) and B (W) fragments as ONE 16-byte global
// load per lane -- row lane & 15, k offset 8 * (lane >> 4) -- and nothing goes through LDS.  A workgroup of four wavefronts owns one
// 16-column fragment of N, one 256-row block of B and one slice of K; wavefront w takes the row fragments w, w + 4, w + 8, w + 12 (four
// accumulator blocks at most; a fragment behind B is skipped, a row behind B and a column behind N are zero registers, not loads).  The
// output has ceil(N / 16) * ceil(B / 256) tiles, 63 for the ResNet-50 head, so the contraction is split over S = pf_dense_splits(...)
// slices, a function of the shape alone: S divides K / 32, S <= 8 and tiles * S <= 512 (two workgroups per CU).  Slice z writes slab z
// of a float32 workspace [S][B][N]; k_dense_fold_y adds the slabs in ascending z, adds the bias, rounds once and stores Y in 4-byte
// pieces where Y's address allows and in 2-byte pieces where not.  S == 1: the first kernel adds the bias and stores Y itself.  No
// atomics, no arrival counters: the order of every sum is fixed by the shape.
//
// Backward-data (k_dense_bwd_data).  The contraction runs over n, the ragged axis of dY and the slow axis of W.  A workgroup owns 64
// columns of K (K % 64 == 32: the last tile has 32), one 256-row block and a slice of whole 32-wide n-steps; per step it stages
//   W  chunk [32 n][64 k], 16-byte loads, rows n >= N zero,                        pitch 160 bytes
//   dY chunk [256 b][32 n], 4-byte loads where the pair's address is a multiple of 4 and 2-byte loads where not (row parity: N is odd),
//            elements n >= N and rows b >= B zero,                                 pitch  80 bytes
// (zeros in BOTH operands: 0 * Inf is NaN) while the loads of the next step are already in flight in registers.  W is read with
// ds_read_b64_tr_b16, as k_wrw3x3n reads its operands: lane (q, l15) gives the address of row 4 q + (l15 >> 2) (+ 16 for the second
// read), column quad l15 & 3, and receives rows 4 q .. 4 q + 3 (+ 16) of column l15.  Bank arithmetic (64 banks of 4 bytes, a
// half-wavefront per pass): the eight 32-byte row pieces of a pass start at 160 r mod 256 = 0 160 64 224 128 32 192 96 -- eight
// distinct multiples of 32, all 64 banks once.  The dY fragment follows the same n order with two ds_read_b64 of row l15 at bytes 8 q
// and 32 + 8 q: row r starts at bank 20 r mod 64 = 0 20 40 60 16 36 56 12 32 52 8 28 48 4 24 44, sixteen distinct multiples of 4, the
// q = 0 | 1 lanes of a pass take banks +0 +1 | +2 +3 of them -- all 64 banks once.  Each lane ends with 4 consecutive k of one row: 16
// bytes of a float32 slab [S][B][K], folded by k_dense_fold_x in ascending order with 16-byte stores, or 8 bytes of dX when S == 1.
//
// Backward-filter (k_dense_wrw).  The contraction runs over b, the slow axis of both operands: 32-row chunks of dY [32 b][64 n] and
// X [32 b][64 k] are staged (pitch 160, as above) and both read transposed; the chunks are summed in ascending b inside the kernel, no
// split, no slab: ceil(N / 64) * ceil(K / 64) tiles (512 for the ResNet-50 head).  Wavefront w owns the 16 n of fragment w and all 64
// k.  The workgroups of the first K tile also sum their 64 dY columns from the staged chunk, ascending b, into db (float32).
#include "pf_mfma.h"

#define DN_THREADS 256
#define DN_WP 160             // pitch of a [32 rows][64 columns] bf16 chunk read transposed
#define DN_YP 80              // pitch of the [256 rows][32 columns] dY chunk of backward-data

struct DenseArgs {
  const bf16_t* A;      // forward: X [B][K]; backward: dY [B][N]
  const bf16_t* Wt;     // forward / backward-data: W [N][K]; backward-filter: X [B][K]
  const float* bias;    // forward: [N] or null
  void* out;            // Y [B][N] | dX [B][K] | dW [N][K]
  float* f32;           // the slabs; backward-filter: db [N] or null
  int B, K, N;
  int per;              // 32-wide steps of the contraction per slice
};

// two neighbouring bf16 of a row whose pitch is odd: one 4-byte load where the address allows, 2-byte loads where not; an element
// at or behind `n_end` is zero and is not loaded
__device__ __forceinline__ uint32_t dn_load_pair(const bf16_t* p, int n, int n_end) {
  if (n >= n_end) return 0u;
  if (n + 1 < n_end && (((uintptr_t)p) & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = p[0];
  if (n + 1 < n_end) v |= ((uint32_t)p[1]) << 16;
  return v;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
template <bool SLAB>
__global__ __launch_bounds__(DN_THREADS) void k_dense_fwd(const DenseArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int n = blockIdx.x * 16 + l15;
  const int b0 = blockIdx.y * 256;
  const int k0 = blockIdx.z * a.per * 32 + q * 8;
  const bool n_ok = n < a.N;
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};
  const bf16_t* wp = a.Wt + (int64_t)(n_ok ? n : 0) * a.K + k0;
  const bf16_t* xp[4];
  bool x_ok[4], f_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int fb = b0 + (wave + 4 * i) * 16;
    f_ok[i] = fb < a.B;                                                      // wave-uniform
    x_ok[i] = fb + l15 < a.B;
    xp[i] = a.A + (int64_t)(x_ok[i] ? fb + l15 : 0) * a.K + k0;
  }
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // two k-steps per trip, the next trip's ten loads in flight while this one multiplies (a step behind the slice: zeros, no load)
  u32x4_t wv[2], xv[2][4], wn[2], xn[2][4];
  auto load = [&](int s, u32x4_t (&w)[2], u32x4_t (&x)[2][4]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool s_ok = s + h < a.per;                                       // wave-uniform
      w[h] = zero4;
      if (s_ok && n_ok) w[h] = *reinterpret_cast<const u32x4_t*>(wp + (s + h) * 32);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[h][i] = zero4;
        if (s_ok && x_ok[i]) x[h][i] = *reinterpret_cast<const u32x4_t*>(xp[i] + (s + h) * 32);
      }
    }
  };
  load(0, wv, xv);
  for (int s = 0; s < a.per; s += 2) {
    load(s + 2, wn, xn);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(&wv[h]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (f_ok[i]) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&xv[h][i]), wf, acc[i], 0, 0, 0);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      wv[h] = wn[h];
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[h][i] = xn[h][i];
    }
  }

  // lane (q, l15): rows 4 q .. 4 q + 3 of the fragment, column n
  if (!n_ok) return;
  const float bias = (!SLAB && a.bias != nullptr) ? a.bias[n] : 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (f_ok[i]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = b0 + (wave + 4 * i) * 16 + q * 4 + r;
        if (b < a.B) {
          if (SLAB) a.f32[((int64_t)blockIdx.z * a.B + b) * a.N + n] = acc[i][r];
          else reinterpret_cast<bf16_t*>(a.out)[(int64_t)b * a.N + n] = f32_to_bf16(acc[i][r] + bias);
        }
      }
    }
}

// Y = bf16(slab 0 + slab 1 + ... + bias): two neighbouring elements per lane
__global__ __launch_bounds__(DN_THREADS) void k_dense_fold_y(const float* __restrict__ slabs, int S, const float* __restrict__ bias,
                                                           bf16_t* __restrict__ Y, int64_t total, int N) {
  const int64_t i = ((int64_t)blockIdx.x * DN_THREADS + threadIdx.x) * 2;
  if (i >= total) return;
  const bool two = i + 1 < total;
  float s0 = slabs[i], s1 = two ? slabs[i + 1] : 0.0f;
  for (int s = 1; s < S; ++s) {
    const float* p = slabs + (int64_t)s * total + i;
    s0 += p[0];
    if (two) s1 += p[1];
  }
  if (bias != nullptr) {
    s0 += bias[(int)(i % N)];
    if (two) s1 += bias[(int)((i + 1) % N)];
  }
  if (two && (((uintptr_t)Y) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(Y + i) = pack_bf16x2(s0, s1);
  } else {
    Y[i] = f32_to_bf16(s0);
    if (two) Y[i + 1] = f32_to_bf16(s1);
  }
}

// dX = bf16(slab 0 + slab 1 + ...): eight elements per lane, 16-byte stores
__global__ __launch_bounds__(DN_THREADS) void k_dense_fold_x(const float* __restrict__ slabs, int S, bf16_t* __restrict__ dX, int64_t total) {
  const int64_t i = ((int64_t)blockIdx.x * DN_THREADS + threadIdx.x) * 8;
  if (i >= total) return;
  float acc[8], v[8];
  load8<float>(slabs + i, acc);
  for (int s = 1; s < S; ++s) {
    load8<float>(slabs + (int64_t)s * total + i, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += v[e];
  }
  store8<bf16_t>(dX + i, acc);
}

// ---- backward-data ---------------------------------------------------------------------------------------------------------------------
template <bool SLAB>
__global__ __launch_bounds__(DN_THREADS) void k_dense_bwd_data(const DenseArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char ws[32 * DN_WP];
  __shared__ __attribute__((aligned(16))) unsigned char ys[256 * DN_YP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int kt = blockIdx.x * 64, b0 = blockIdx.y * 256;
  const int rows = (a.B - b0) < 256 ? (a.B - b0) : 256;
  const int steps = (a.N + 31) >> 5;
  const int step0 = blockIdx.z * a.per;
  const int step1 = (step0 + a.per) < steps ? (step0 + a.per) : steps;
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};
  const int nkf = (a.K - kt) >= 64 ? 4 : 2;                                  // 16-column fragments of this tile (K % 32 == 0)

  // staging maps: W chunk row wr, 16-byte piece wseg; dY chunk pair yp of rows yr, yr + 16, ...
  const int wr = tid >> 3, wseg = tid & 7;
  const bool wk_ok = kt + wseg * 8 < a.K;
  const int yp = tid & 15, yr = tid >> 4;
  u32x4_t wreg = zero4;
  uint32_t yreg[16];

  auto load = [&](int step) {
    const int n0 = step * 32;
    wreg = zero4;
    if (wk_ok && n0 + wr < a.N) wreg = *reinterpret_cast<const u32x4_t*>(a.Wt + (int64_t)(n0 + wr) * a.K + kt + wseg * 8);
    const int nn = n0 + 2 * yp;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = yr + 16 * i;
      yreg[i] = 0u;
      if (row < rows) yreg[i] = dn_load_pair(a.A + (int64_t)(b0 + row) * a.N + nn, nn, a.N);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) acc[i][kf] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const uint32_t wb = lds_addr(ws) + (uint32_t)((q * 4 + (l15 >> 2)) * DN_WP + (l15 & 3) * 8);
  if (step0 < step1) load(step0);
  for (int step = step0; step < step1; ++step) {
    __syncthreads();                                                         // every wavefront is done with the previous chunk
    *reinterpret_cast<u32x4_t*>(ws + wr * DN_WP + wseg * 16) = wreg;
#pragma unroll
    for (int i = 0; i < 16; ++i) *reinterpret_cast<uint32_t*>(ys + (yr + 16 * i) * DN_YP + yp * 4) = yreg[i];
    __syncthreads();
    if (step + 1 < step1) load(step + 1);
    pf_v4s wl[4], wh[4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      pf_tr_issue(wb + (uint32_t)(kf * 32), wl[kf]);
      pf_tr_issue(wb + (uint32_t)(16 * DN_WP + kf * 32), wh[kf]);
    }
    pf_lds_wait();
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) { PF_TIE(wl[kf]); PF_TIE(wh[kf]); }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int fr = (wave + 4 * i) * 16;
      if (fr < rows) {                                                       // wave-uniform
        const unsigned char* yrow = ys + (fr + l15) * DN_YP + q * 8;
        const uint2 lo = *reinterpret_cast<const uint2*>(yrow), hi = *reinterpret_cast<const uint2*>(yrow + 32);
        const u32x4_t yv = {lo.x, lo.y, hi.x, hi.y};
        const bf16x8 yf = *reinterpret_cast<const bf16x8*>(&yv);
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
          if (kf < nkf) acc[i][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf_join(wl[kf], wh[kf]), yf, acc[i][kf], 0, 0, 0);
      }
    }
  }

  // lane (q, l15): row l15 of the fragment, columns kt + 16 kf + 4 q .. + 3
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave + 4 * i) * 16 + l15;
    if (row < rows) {
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
        if (kf < nkf) {
          const int64_t at = (int64_t)(b0 + row) * a.K + kt + kf * 16 + q * 4;
          const f32x4 v = acc[i][kf];
          if (SLAB) *reinterpret_cast<float4*>(a.f32 + (int64_t)blockIdx.z * a.B * a.K + at) = make_float4(v[0], v[1], v[2], v[3]);
          else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(a.out) + at) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
        }
    }
  }
}

// ---- backward-filter -------------------------------------------------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(DN_THREADS) void k_dense_wrw(const DenseArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char ys[32 * DN_WP];      // dY chunk [32 b][64 n]
  __shared__ __attribute__((aligned(16))) unsigned char xs[32 * DN_WP];      // X  chunk [32 b][64 k]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int kt = blockIdx.x * 64, nt = blockIdx.y * 64;
  const int n_end = (a.N - nt) < 64 ? a.N : nt + 64;
  const int nkf = (a.K - kt) >= 64 ? 4 : 2;
  const int chunks = (a.B + 31) >> 5;
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};
  const bool sums = blockIdx.x == 0 && a.f32 != nullptr && tid < 64;          // db: wavefront 0 of the first K tile, one column per lane

  const int xr = tid >> 3, xseg = tid & 7;
  const bool xk_ok = kt + xseg * 8 < a.K;
  const int yp = tid & 31, yr = tid >> 5;
  const int nn = nt + 2 * yp;
  u32x4_t xreg = zero4;
  uint32_t yreg[4];

  auto load = [&](int c) {
    const int r0 = c * 32;
    xreg = zero4;
    if (xk_ok && r0 + xr < a.B) xreg = *reinterpret_cast<const u32x4_t*>(a.Wt + (int64_t)(r0 + xr) * a.K + kt + xseg * 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = r0 + yr + 8 * i;
      yreg[i] = 0u;
      if (b < a.B) yreg[i] = dn_load_pair(a.A + (int64_t)b * a.N + nn, nn, n_end);
    }
  };

  f32x4 acc[4];
#pragma unroll
  for (int kf = 0; kf < 4; ++kf) acc[kf] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float dbsum = 0.0f;
  const bool w_ok = nt + wave * 16 < a.N;                                    // wave-uniform: this wavefront's 16 n exist
  const uint32_t row_off = (uint32_t)((q * 4 + (l15 >> 2)) * DN_WP + (l15 & 3) * 8);
  const uint32_t yb = lds_addr(ys) + row_off + (uint32_t)(wave * 32), xb = lds_addr(xs) + row_off;

  load(0);
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();
    *reinterpret_cast<u32x4_t*>(xs + xr * DN_WP + xseg * 16) = xreg;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint32_t*>(ys + (yr + 8 * i) * DN_WP + yp * 4) = yreg[i];
    __syncthreads();
    if (c + 1 < chunks) load(c + 1);
    if (w_ok) {
      pf_v4s dl, dh, xl[4], xh[4];
      pf_tr_issue(yb, dl);
      pf_tr_issue(yb + (uint32_t)(16 * DN_WP), dh);
#pragma unroll
      for (int kf = 0; kf < 4; ++kf) {
        pf_tr_issue(xb + (uint32_t)(kf * 32), xl[kf]);
        pf_tr_issue(xb + (uint32_t)(16 * DN_WP + kf * 32), xh[kf]);
      }
      pf_lds_wait();
      PF_TIE(dl); PF_TIE(dh);
#pragma unroll
      for (int kf = 0; kf < 4; ++kf) { PF_TIE(xl[kf]); PF_TIE(xh[kf]); }
      const bf16x8 df = pf_join(dl, dh);
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
        if (kf < nkf) acc[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf_join(xl[kf], xh[kf]), df, acc[kf], 0, 0, 0);
    }
    if (sums) {
#pragma unroll 8
      for (int r = 0; r < 32; ++r) dbsum += bf16_to_f32(*reinterpret_cast<const bf16_t*>(ys + r * DN_WP + tid * 2));
    }
  }

  if (sums && nt + tid < a.N) a.f32[nt + tid] = dbsum;
  // lane (q, l15): row n = nt + 16 wave + l15, columns kt + 16 kf + 4 q .. + 3
  const int n = nt + wave * 16 + l15;
  if (n >= a.N) return;
#pragma unroll
  for (int kf = 0; kf < 4; ++kf)
    if (kf < nkf) {
      const int64_t at = (int64_t)n * a.K + kt + kf * 16 + q * 4;
      const f32x4 v = acc[kf];
      if (F32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out) + at) = make_float4(v[0], v[1], v[2], v[3]);
      else *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(a.out) + at) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static inline int dn_cdiv(int a, int b) { return (a + b - 1) / b; }

extern "C" int pf_dense_supported(int B, int K, int N) {
  const int64_t lim = (int64_t)1 << 31;
  return (B >= 1 && N >= 1 && K >= 32 && (K % 32) == 0 && (int64_t)B * K * 2 < lim && (int64_t)N * K * 4 < lim &&
          (int64_t)B * N * 2 < lim) ? 1 : 0;
}

extern "C" int pf_dense_splits(int B, int K, int N, int bwd_data) {
  if (!pf_dense_supported(B, K, N)) return 0;
  const int rb = dn_cdiv(B, 256);
  if (!bwd_data) {
    const int64_t tiles = (int64_t)dn_cdiv(N, 16) * rb;
    const int ksteps = K / 32;
    int S = 1;
    for (int d = 2; d <= 8 && d <= ksteps; ++d)
      if (ksteps % d == 0 && tiles * d <= 512) S = d;
    return S;
  }
  const int64_t tiles = (int64_t)dn_cdiv(K, 64) * rb;
  const int steps = dn_cdiv(N, 32);
  int cap = (int)(256 / tiles);
  cap = cap < 1 ? 1 : (cap > 8 ? 8 : cap);
  cap = cap < steps ? cap : steps;
  const int per = dn_cdiv(steps, cap);
  return dn_cdiv(steps, per);                                                // no empty slice
}

extern "C" int pf_dense_fwd(const void* X, const void* W, const float* bias, void* Y, int B, int K, int N, float* workspace,
                            int64_t ws_elems, void* stream) {
  const int S = pf_dense_splits(B, K, N, 0);
  if (S <= 0 || X == nullptr || W == nullptr || Y == nullptr || !pf_aligned16(X) || !pf_aligned16(W) || (((uintptr_t)Y) & 1) != 0 ||
      (S > 1 && (workspace == nullptr || !pf_aligned16(workspace) || ws_elems < (int64_t)S * B * N)))
    return (int)hipErrorInvalidValue;
  DenseArgs a;
  a.A = (const bf16_t*)X; a.Wt = (const bf16_t*)W; a.bias = bias; a.out = Y; a.f32 = workspace;
  a.B = B; a.K = K; a.N = N; a.per = K / 32 / S;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(dn_cdiv(N, 16), dn_cdiv(B, 256), S);
  if (S == 1) {
    k_dense_fwd<false><<<grid, DN_THREADS, 0, st>>>(a);
    PF_LAUNCH_CHECK();
    return 0;
  }
  k_dense_fwd<true><<<grid, DN_THREADS, 0, st>>>(a);
  PF_LAUNCH_CHECK();
  const int64_t total = (int64_t)B * N;
  k_dense_fold_y<<<(unsigned)((total + 2 * DN_THREADS - 1) / (2 * DN_THREADS)), DN_THREADS, 0, st>>>(workspace, S, bias, (bf16_t*)Y, total, N);
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_dense_bwd_data(const void* dY, const void* W, void* dX, int B, int K, int N, float* workspace, int64_t ws_elems,
                                 void* stream) {
  const int S = pf_dense_splits(B, K, N, 1);
  if (S <= 0 || dY == nullptr || W == nullptr || dX == nullptr || (((uintptr_t)dY) & 1) != 0 || !pf_aligned16(W) || !pf_aligned16(dX) ||
      (S > 1 && (workspace == nullptr || !pf_aligned16(workspace) || ws_elems < (int64_t)S * B * K)))
    return (int)hipErrorInvalidValue;
  DenseArgs a;
  a.A = (const bf16_t*)dY; a.Wt = (const bf16_t*)W; a.bias = nullptr; a.out = dX; a.f32 = workspace;
  a.B = B; a.K = K; a.N = N; a.per = dn_cdiv(dn_cdiv(N, 32), S);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(dn_cdiv(K, 64), dn_cdiv(B, 256), S);
  if (S == 1) {
    k_dense_bwd_data<false><<<grid, DN_THREADS, 0, st>>>(a);
    PF_LAUNCH_CHECK();
    return 0;
  }
  k_dense_bwd_data<true><<<grid, DN_THREADS, 0, st>>>(a);
  PF_LAUNCH_CHECK();
  const int64_t total = (int64_t)B * K;
  k_dense_fold_x<<<(unsigned)((total + 8 * DN_THREADS - 1) / (8 * DN_THREADS)), DN_THREADS, 0, st>>>(workspace, S, (bf16_t*)dX, total);
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_dense_wrw(const void* dY, const void* X, void* dW, int dw_dtype, float* db, int B, int K, int N, void* stream) {
  if (!pf_dense_supported(B, K, N) || dY == nullptr || X == nullptr || dW == nullptr || (((uintptr_t)dY) & 1) != 0 || !pf_aligned16(X) ||
      !pf_aligned16(dW) || (((uintptr_t)db) & 3) != 0 || (dw_dtype != PF_F32 && dw_dtype != PF_BF16))
    return (int)hipErrorInvalidValue;
  DenseArgs a;
  a.A = (const bf16_t*)dY; a.Wt = (const bf16_t*)X; a.bias = nullptr; a.out = dW; a.f32 = db;
  a.B = B; a.K = K; a.N = N; a.per = 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(dn_cdiv(K, 64), dn_cdiv(N, 64));
  if (dw_dtype == PF_F32) k_dense_wrw<true><<<grid, DN_THREADS, 0, st>>>(a);
  else k_dense_wrw<false><<<grid, DN_THREADS, 0, st>>>(a);
  PF_LAUNCH_CHECK();
  return 0;
}
