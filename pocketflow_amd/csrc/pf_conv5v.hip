// Fourth member of the few-channel convolution family: 5x5 / stride 1 / no padding ('VALID') with a BIAS, C in {3, 32} input and N in
// {32, 64} output channels, 5 <= Wd <= 64, any H >= 5: the two convolutions of LeNet @ CIFAR-10 (conv1 3 -> 32 on 32 x 32, conv2 32 -> 64
// on 14 x 14).  Forward, backward-data (C = 32) and backward-filter with the bias gradient, NHWC bf16 in and out, float32 accumulation on
// v_mfma_f32_16x16x32_bf16.  No atomics, every sum in an order fixed by the shape, no padded or im2col copy of anything in HBM.  Before
// this file conv2 was three MIOpen calls (every MFMA route refused a bias) and conv1 ran on the vector-ALU kernel of pf_convg.hip.
//
// Tiles.  A tile is TR output rows of one image, TR * Wo <= 128 pixels, the rows of an image dealt evenly (c5_rows).  Its input window,
// (TR + 4) x (Wo + 4) pixels, is staged ONCE in LDS and every tap is a shifted LDS address.  Wo = Wd - 4 has no divisibility (10 and
// 28 in LeNet), so the tile's pixels are walked 16 (forward) or 32 (backward-filter) at a time in LINEAR order over its rows and each
// lane derives (row, column) of its own pixel, hence its window address, as k_stem3x_wrw does.  A lane behind the tile's last pixel
// reads that last pixel again: a column of the MFMA of its own, which is not stored (forward) or meets zero rows of dY (filter).
//
// Forward, C = 32 | 64 per tap (k_conv5v<CK, N>).  Taps are folded into K, k = tap * CK + c, which is KRSC memory as it stands: 25 (CK =
// 32) or 50 (CK = 64) k-steps.  Wavefront w owns output channels 16 (w / WPB) .. + 15, WPB = 4 / (N / 16), and keeps their 25 | 50 weight
// fragments in registers for the life of the workgroup; the WPB wavefronts of a channel block take alternate pixel fragments.  Window by
// LDS-DMA, pixel pitch 2 CK + 16 bytes (80 | 144): sixteen consecutive pixels start at banks 20 i | 36 i mod 64 = sixteen distinct
// multiples of 4, so a 16-lane ds_read_b128 covers the 64 banks once; where a fragment wraps an output row the window
// address jumps by 4 pixels and up to four lanes pair up two to a bank.  Epilogue: + float32 bias of the lane's four channels, one
// rounding, 8-byte stores from the accumulators.  Backward-data is this kernel with (C, N) swapped on the flipped / transposed filter and
// pad 4: the padding enters the window as lanes with an out-of-range offset, no padded dY exists.
//
// Forward, C = 3 (k_conv5v_c3<NB>).  Pixels are staged padded to four channels (8 bytes), k = tap * 4 + c: 100 = four k-steps, lane group
// q of step j feeds taps 8 j + 2 q and + 1, two ds_read_b64.  Taps 25 .. 31 do not exist: their weights are zeros that were never loaded
// AND their operand is zeros in registers, not what lies behind the window (0 * Inf is NaN).  Weights go from global memory to
// registers; MFMA row i of block nb is channel 4 NB (i / 4) + 4 nb + i % 4, so a lane ends with 4 NB consecutive channels: 16-byte stores.
//
// Backward-filter (k_conv5v_wrw<N>, k_conv5v_wrw_c3<NB>).  dW[n][tap][c] = sum over pixels of dY[p][n] * X[window(p) + tap][c]: both
// operands pixel-major in LDS (X window and dY tile staged once per tile), fetched with the transposing reads of pf_mfma.h.  C = 32:
// one wavefront per (16 n) x (16 c) block, 4 (N = 32) or 8 (N = 64) wavefronts, each with all 25 taps = 100 accumulator registers.
// C = 3: a 16-column block is FOUR taps x 4 padded channels, 7 tap blocks x N / 16 channel blocks dealt to four wavefronts.  Persistent
// workgroups write one float32 slab [N][25][C] each, folded in fixed order by pf_wrw_reduce.  Slab count (pf_conv5v_wrw_slabs): the slabs written
// stay below FOUR times the operand bytes read, at most one per tile and 256.  db[n] = sum of dY comes from the dY tiles in LDS: a thread
// owns a channel pair and every G-th pixel row of each tile, a workgroup folds its G row groups ascending and leaves [N] partial sums
// behind the slabs, and the fold that sums the slabs sums those (pf_wrw_reduce, called for them first: they lie where its stage goes).
// Like its siblings the filter kernels assume FINITE activations (zero rows of dY multiply real pixels).
#include "pf_mfma.h"
#include "pf_buffer.h"

#define C5_THREADS 256
#define C5_TILE_PX 128
#define C5_FWD_GRID 256      // C = 32 | 64: every workgroup loads the whole filter (up to 100 KiB)
#define C5_FWD3_GRID 1024
#define C5_WRW_GRID 256

struct C5Args {
  const bf16_t* X;      // the pass's input [imgs][Hi][Wi][CK]
  const bf16_t* W;      // [N][5][5][CK]
  const float* bias;    // forward: [N] or null
  bf16_t* Y;            // [imgs][Ho][Wo][N]
  const bf16_t* dY;     // backward-filter: [imgs][Ho][Wo][N]
  float* slabs;         // backward-filter: [gridDim.x][N][25][C]
  float* db;            // backward-filter: [gridDim.x][N] partial sums behind the slabs, or null
  uint32_t x_bytes, y_bytes;
  int imgs, Hi, Wi, Ho, Wo;
  int P;                // front = back pad: 0, backward-data 4
  int TR, tiles_per_img, n_tiles;
  int WC;               // window columns = Wo + 4
  int wpix, nx, ny;     // window pixels; KiB of LDS of the window and (backward-filter) of the dY tile
};

// the window of tile (img, h0) by LDS-DMA: window pixel (wr, wc) is input pixel (h0 - P + wr, wc - P), zeros outside the input
template <int CK, int PITCH>
__device__ __forceinline__ void c5_stage_window(const C5Args& a, pf_rsrc_t rsX, unsigned char* dst, int img, int h0, int wave, int nwaves, int lane) {
  for (int I = wave; I < a.nx; I += nwaves) {                                // wave-uniform
    const int byte = I * 1024 + lane * 16;
    const int wp = byte / PITCH, ck = (byte - wp * PITCH) >> 4;
    const int wr = wp / a.WC, wc = wp - wr * a.WC;
    const int h = h0 - a.P + wr, x = wc - a.P;
    const bool ok = wp < a.wpix && ck < CK / 8 && x >= 0 && x < a.Wi && h >= 0 && h < a.Hi;
    const uint32_t voff = ok ? (uint32_t)((((img * a.Hi + h) * a.Wi + x) * CK + ck * 8) * 2) : PF_BUFFER_OOB;
    PF_BUFFER_LOAD_LDS16(rsX, dst + I * 1024, voff, 0);
  }
}
// ... of a three-channel image, one pixel per task, padded to four channels (any Wi: a row of 6 Wi bytes keeps no alignment)
__device__ __forceinline__ void c5_stage_window3(const C5Args& a, unsigned char* dst, int img, int h0, int tid) {
  for (int i = tid; i < a.wpix; i += C5_THREADS) {
    const int wr = i / a.WC, wc = i - wr * a.WC;
    uint32_t e0 = 0u, e1 = 0u, e2 = 0u;
    if (h0 + wr < a.Hi) {
      const bf16_t* src = a.X + ((int64_t)(img * a.Hi + h0 + wr) * a.Wi + wc) * 3;
      e0 = src[0]; e1 = src[1]; e2 = src[2];
    }
    *reinterpret_cast<uint2*>(dst + i * 8) = make_uint2(e0 | (e1 << 16), e2);
  }
}
// the dY tile, `rows` of PITCH bytes from linear pixel m0 on; rows >= valid and the pitch padding are zeros
template <int N, int PITCH>
__device__ __forceinline__ void c5_stage_dy(const C5Args& a, pf_rsrc_t rsY, unsigned char* dst, int m0, int valid, int wave, int nwaves, int lane) {
  for (int I = wave; I < a.ny; I += nwaves) {
    const int byte = I * 1024 + lane * 16;
    const int row = byte / PITCH, ck = (byte - row * PITCH) >> 4;
    const bool ok = row < valid && ck < N / 8;
    const uint32_t voff = ok ? (uint32_t)(((m0 + row) * N + ck * 8) * 2) : PF_BUFFER_OOB;
    PF_BUFFER_LOAD_LDS16(rsY, dst + I * 1024, voff, 0);
  }
}
// this lane's window pixel of the tile's linear pixel p (clamped to the tile's last), in pixels
__device__ __forceinline__ int c5_window_pixel(const C5Args& a, int p, int npix) {
  p = p < npix ? p : npix - 1;
  const int r = p / a.Wo;
  return r * a.WC + (p - r * a.Wo);
}

// ---- forward / backward-data, 32 | 64 channels per tap ------------------------------------------------------------------------------
template <int CK, int N>
__global__ __launch_bounds__(C5_THREADS) void k_conv5v(const C5Args a) {
  constexpr int PITCH = 2 * CK + 16, KH = CK / 32, NB = N / 16, WPB = 4 / NB;
  static_assert(NB == 2 || NB == 4, "N is 32 or 64");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int nb = wave / WPB, fs = wave - nb * WPB;

  // ---- this wavefront's 16 filters, once: k-step (tap, half) = 32 consecutive k of W[n][tap * CK + c], this lane's eight at + 8 q ----
  bf16x8 w[25][KH];
  {
    const bf16_t* wrow = a.W + (nb * 16 + l15) * (25 * CK) + q * 8;
#pragma unroll
    for (int t = 0; t < 25; ++t)
#pragma unroll
      for (int h = 0; h < KH; ++h) w[t][h] = *reinterpret_cast<const bf16x8*>(wrow + t * CK + h * 32);
  }
  float bias[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias[j] = a.bias != nullptr ? a.bias[nb * 16 + q * 4 + j] : 0.0f;

  const int rowb = a.WC * PITCH;
  const pf_rsrc_t rsX = PF_MAKE_RSRC(a.X, a.x_bytes);
  for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const int img = t / a.tiles_per_img, h0 = (t - img * a.tiles_per_img) * a.TR;
    c5_stage_window<CK, PITCH>(a, rsX, smem, img, h0, wave, C5_THREADS / 64, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int npix = ((a.Ho - h0) < a.TR ? (a.Ho - h0) : a.TR) * a.Wo;       // the tile's pixels inside the image
    const int nfrag = (npix + 15) >> 4;
    for (int f = fs; f < nfrag; f += WPB) {                                  // wave-uniform
      const int p = f * 16 + l15;
      const unsigned char* xb = smem + c5_window_pixel(a, p, npix) * PITCH + q * 16;
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int s = 0; s < 5; ++s)
#pragma unroll
          for (int h = 0; h < KH; ++h) {
            const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xb + r * rowb + s * PITCH + h * 64);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r * 5 + s][h], xf, acc, 0, 0, 0);
          }
      // lane (q, l15): output channels nb * 16 + 4 q .. + 3 of the tile's pixel p; the tile's pixels are contiguous in NHWC memory
      if (p < npix)
        *reinterpret_cast<uint2*>(a.Y + (((int64_t)img * a.Ho + h0) * a.Wo + p) * N + nb * 16 + q * 4) =
            make_uint2(pack_bf16x2(acc[0] + bias[0], acc[1] + bias[1]), pack_bf16x2(acc[2] + bias[2], acc[3] + bias[3]));
    }
    __syncthreads();                                                         // every wavefront is done reading the window
  }
}

// ---- forward, three channels ---------------------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(C5_THREADS) void k_conv5v_c3(const C5Args a) {
  constexpr int N = 16 * NB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;

  // ---- A fragments: taps 8 j + 2 q, + 1 x 4 channels of this lane's filter; c = 3 and taps >= 25: zeros, never loaded ----
  bf16x8 wf[NB][4];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = 4 * NB * (l15 >> 2) + 4 * nb + (l15 & 3);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      const int tap = 8 * j + 2 * q;
      if (tap < 25) {
        const bf16_t* src = a.W + (n * 25 + tap) * 3;
        const uint32_t e0 = src[0], e1 = src[1], e2 = src[2];
        v.x = e0 | (e1 << 16); v.y = e2;
        if (tap + 1 < 25) {
          const uint32_t f0 = src[3], f1 = src[4], f2 = src[5];
          v.z = f0 | (f1 << 16); v.w = f2;
        }
      }
      wf[nb][j] = *reinterpret_cast<const bf16x8*>(&v);
    }
  }
  float bias[NB][4];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 4; ++j) bias[nb][j] = a.bias != nullptr ? a.bias[4 * NB * q + 4 * nb + j] : 0.0f;

  // this lane's byte offsets of its two taps of k-step j inside the window; the fourth step has tap 24 alone, in lane group 0
  uint32_t toff[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      int tap = 8 * j + 2 * q + hh;
      tap = tap < 24 ? tap : 24;
      toff[j][hh] = (uint32_t)(((tap / 5) * a.WC + tap % 5) * 8);
    }

  for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const int img = t / a.tiles_per_img, h0 = (t - img * a.tiles_per_img) * a.TR;
    __syncthreads();                                                         // the previous tile's reads are done
    c5_stage_window3(a, smem, img, h0, tid);
    __syncthreads();
    const int npix = ((a.Ho - h0) < a.TR ? (a.Ho - h0) : a.TR) * a.Wo;
    const int nfrag = (npix + 15) >> 4;
    for (int f = wave; f < nfrag; f += C5_THREADS / 64) {
      const int p = f * 16 + l15;
      const unsigned char* xb = smem + c5_window_pixel(a, p, npix) * 8;
      f32x4 acc[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint2 lo = *reinterpret_cast<const uint2*>(xb + toff[j][0]);
        uint2 hi = make_uint2(0u, 0u);
        if (j < 3) hi = *reinterpret_cast<const uint2*>(xb + toff[j][1]);
        else if (q != 0) lo = make_uint2(0u, 0u);                            // taps 25 .. 31: a zero operand for the zero weights
        const uint4 xv = make_uint4(lo.x, lo.y, hi.x, hi.y);
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&xv);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb][j], xf, acc[nb], 0, 0, 0);
      }
      if (p >= npix) continue;
      // lane (q, l15): channels 4 NB q + 4 nb + j of pixel p, eight per store
      bf16_t* out = a.Y + (((int64_t)img * a.Ho + h0) * a.Wo + p) * N + 4 * NB * q;
#pragma unroll
      for (int h = 0; h < NB / 2; ++h)
        *reinterpret_cast<uint4*>(out + 8 * h) =
            make_uint4(pack_bf16x2(acc[2 * h][0] + bias[2 * h][0], acc[2 * h][1] + bias[2 * h][1]),
                       pack_bf16x2(acc[2 * h][2] + bias[2 * h][2], acc[2 * h][3] + bias[2 * h][3]),
                       pack_bf16x2(acc[2 * h + 1][0] + bias[2 * h + 1][0], acc[2 * h + 1][1] + bias[2 * h + 1][1]),
                       pack_bf16x2(acc[2 * h + 1][2] + bias[2 * h + 1][2], acc[2 * h + 1][3] + bias[2 * h + 1][3]));
    }
  }
}

// ---- backward-filter -----------------------------------------------------------------------------------------------------------------
// db: this thread's share of one staged dY tile -- channel pair tid % (N / 2), pixel rows tid / (N / 2), + G, ... (G = T / (N / 2))
template <int N, int T, int YP>
__device__ __forceinline__ void c5_db_tile(const unsigned char* ys, int npix, int tid, float& s0, float& s1) {
  for (int row = tid / (N / 2); row < npix; row += T / (N / 2)) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(ys + row * YP + (tid % (N / 2)) * 4);
    s0 += __uint_as_float(v << 16); s1 += __uint_as_float(v & 0xFFFF0000u);
  }
}
// ... and the workgroup's [N] partial sums: its G row groups, ascending.  red: [G][N] floats.
template <int N, int T>
__device__ __forceinline__ void c5_db_store(float* red, float* out, int tid, float s0, float s1) {
  red[(tid / (N / 2)) * N + 2 * (tid % (N / 2))] = s0;
  red[(tid / (N / 2)) * N + 2 * (tid % (N / 2)) + 1] = s1;
  __syncthreads();
  if (tid < N) {
    float tot = 0.0f;
    for (int g = 0; g < T / (N / 2); ++g) tot += red[g * N + tid];
    out[tid] = tot;
  }
}

// C = 32: wavefront (nb, cb) = 16 filters x 16 input channels x all 25 taps
template <int N>
__global__ __launch_bounds__((N / 16) * 128) void k_conv5v_wrw(const C5Args a) {
  constexpr int NW = (N / 16) * 2, XP = 96, YP = (N == 32) ? 96 : 160;      // pixel pitches: eight 32-byte rows cover the 64 banks once
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // input window | dY tile
  __shared__ float red[NW * 128];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int nb = wave >> 1, cb = wave & 1;
  const pf_rsrc_t rsX = PF_MAKE_RSRC(a.X, a.x_bytes);
  const pf_rsrc_t rsY = PF_MAKE_RSRC(a.dY, a.y_bytes);
  unsigned char* ys = smem + a.nx * 1024;
  // a transposing read takes from lane (q, l15) the 8 bytes of pixel row q * 4 + (l15 >> 2) (+ 16: the second read) at channel quad
  // l15 & 3; dY and X use the same pixel order, so the contraction is consistent
  const int pr = q * 4 + (l15 >> 2);
  const int rowb = a.WC * XP;

  f32x4 acc[25];
#pragma unroll
  for (int t = 0; t < 25; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float db0 = 0.0f, db1 = 0.0f;

  for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const int img = t / a.tiles_per_img, h0 = (t - img * a.tiles_per_img) * a.TR;
    const int npix = ((a.Ho - h0) < a.TR ? (a.Ho - h0) : a.TR) * a.Wo;
    c5_stage_window<32, XP>(a, rsX, smem, img, h0, wave, NW, lane);
    c5_stage_dy<N, YP>(a, rsY, ys, (img * a.Ho + h0) * a.Wo, npix, wave, NW, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (a.db != nullptr) c5_db_tile<N, NW * 64, YP>(ys, npix, tid, db0, db1);
    const int nkb = (npix + 31) >> 5;
    for (int kb = 0; kb < nkb; ++kb) {
      const unsigned char* dyb = ys + (kb * 32 + pr) * YP + nb * 32 + (l15 & 3) * 8;
      const bf16x8 df = pf_join(pf_tr_read(dyb), pf_tr_read(dyb + 16 * YP));
      const unsigned char* xlo = smem + c5_window_pixel(a, kb * 32 + pr, npix) * XP + cb * 32 + (l15 & 3) * 8;
      const unsigned char* xhi = smem + c5_window_pixel(a, kb * 32 + 16 + pr, npix) * XP + cb * 32 + (l15 & 3) * 8;
#pragma unroll
      for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int s = 0; s < 5; ++s)
          acc[r * 5 + s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              df, pf_join(pf_tr_read(xlo + r * rowb + s * XP), pf_tr_read(xhi + r * rowb + s * XP)), acc[r * 5 + s], 0, 0, 0);
    }
    __syncthreads();                                                         // every wavefront is done with the tile
  }
  if (a.db != nullptr) c5_db_store<N, NW * 64>(red, a.db + blockIdx.x * N, tid, db0, db1);
  // slab [N][25][32]: accumulator t holds rows n = nb * 16 + 4 q + j, column c = cb * 16 + l15 of tap t
  float* out = a.slabs + (int64_t)blockIdx.x * (N * 25 * 32) + (nb * 16 + q * 4) * (25 * 32) + cb * 16 + l15;
#pragma unroll
  for (int t = 0; t < 25; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j * (25 * 32) + t * 32] = acc[t][j];
}

// C = 3: pair p = 7 nb + tb -- channel block nb, taps 4 tb .. 4 tb + 3 --, wavefront w owns pairs PW w .. PW w + PW - 1
template <int NB>
__global__ __launch_bounds__(C5_THREADS) void k_conv5v_wrw_c3(const C5Args a) {
  constexpr int N = 16 * NB, PW = (7 * NB + 3) / 4, YP = (N == 32) ? 96 : 160;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // input window, 8 bytes a pixel | dY tile
  __shared__ float red[4 * 128];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const pf_rsrc_t rsY = PF_MAKE_RSRC(a.dY, a.y_bytes);
  unsigned char* ys = smem + a.nx * 1024;
  const int pr = q * 4 + (l15 >> 2);
  // the piece this lane addresses in a block of X: the padded pixel at tap 4 tb + (l15 & 3); taps 25 .. 27 read tap 24, not stored
  uint32_t toff[PW];
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    int tap = 4 * ((wave * PW + i) % 7) + (l15 & 3);
    tap = tap < 24 ? tap : 24;
    toff[i] = (uint32_t)(((tap / 5) * a.WC + tap % 5) * 8);
  }

  f32x4 acc[PW];
#pragma unroll
  for (int i = 0; i < PW; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float db0 = 0.0f, db1 = 0.0f;

  for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const int img = t / a.tiles_per_img, h0 = (t - img * a.tiles_per_img) * a.TR;
    const int npix = ((a.Ho - h0) < a.TR ? (a.Ho - h0) : a.TR) * a.Wo;
    __syncthreads();                                                         // the previous tile's reads are done
    c5_stage_dy<N, YP>(a, rsY, ys, (img * a.Ho + h0) * a.Wo, npix, wave, 4, lane);
    c5_stage_window3(a, smem, img, h0, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (a.db != nullptr) c5_db_tile<N, C5_THREADS, YP>(ys, npix, tid, db0, db1);
    const int nkb = (npix + 31) >> 5;
    for (int kb = 0; kb < nkb; ++kb) {
      const unsigned char* dyb = ys + (kb * 32 + pr) * YP + (l15 & 3) * 8;
      const unsigned char* xlo = smem + c5_window_pixel(a, kb * 32 + pr, npix) * 8;
      const unsigned char* xhi = smem + c5_window_pixel(a, kb * 32 + 16 + pr, npix) * 8;
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const int p = wave * PW + i;
        if (p < 7 * NB) {                                                    // wave-uniform
          const int nb = p / 7;
          const bf16x8 df = pf_join(pf_tr_read(dyb + nb * 32), pf_tr_read(dyb + nb * 32 + 16 * YP));
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, pf_join(pf_tr_read(xlo + toff[i]), pf_tr_read(xhi + toff[i])), acc[i], 0, 0, 0);
        }
      }
    }
  }
  if (a.db != nullptr) c5_db_store<N, C5_THREADS>(red, a.db + blockIdx.x * N, tid, db0, db1);
  // slab [N][25][3]: lane (q, l15) holds rows n = 16 nb + 4 q + j, column (tap = 4 tb + l15 / 4, c = l15 % 4)
  float* slab = a.slabs + (int64_t)blockIdx.x * (N * 75);
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int p = wave * PW + i;
    const int nb = p / 7, tap = 4 * (p - 7 * nb) + (l15 >> 2), c = l15 & 3;
    if (p < 7 * NB && tap < 25 && c < 3) {
#pragma unroll
      for (int j = 0; j < 4; ++j) slab[((16 * nb + 4 * q + j) * 25 + tap) * 3 + c] = acc[i][j];
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static bool c5_shape_ok(int H, int Wd, int C, int N) {
  return (C == 3 || C == 32) && (N == 32 || N == 64) && H >= 5 && Wd >= 5 && Wd <= 64;
}
// 31-bit byte offsets of both tensors
static bool c5_fits(int imgs, int H, int Wd, int C, int N) {
  return imgs > 0 && (int64_t)imgs * H * Wd * C * 2 < ((int64_t)1 << 31) && (int64_t)imgs * (H - 4) * (Wd - 4) * N * 2 < ((int64_t)1 << 31);
}
// output rows of a tile: at most C5_TILE_PX pixels, the rows of an image dealt evenly over its tiles
static int c5_rows(int Ho, int Wo) {
  const int maxr = C5_TILE_PX / Wo;                                          // >= 2: Wo <= 64
  const int tiles = (Ho + maxr - 1) / maxr;
  return (Ho + tiles - 1) / tiles;
}
// the tiling every kernel shares, for the pass Hi x Wi -> Ho x Wo with front pad P; `pitch`: bytes per window pixel
static void c5_fill(C5Args& a, int imgs, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int P, int pitch) {
  a.imgs = imgs; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.P = P;
  a.TR = c5_rows(Ho, Wo);
  a.tiles_per_img = (Ho + a.TR - 1) / a.TR;
  a.n_tiles = imgs * a.tiles_per_img;
  a.WC = Wo + 4;
  a.wpix = (a.TR + 4) * a.WC;
  a.nx = (a.wpix * pitch + 1023) / 1024;
  a.ny = 0;
  a.x_bytes = (uint32_t)((int64_t)imgs * Hi * Wi * Cin * 2);
  a.y_bytes = (uint32_t)((int64_t)imgs * Ho * Wo * Cout * 2);
  a.X = nullptr; a.W = nullptr; a.bias = nullptr; a.Y = nullptr; a.dY = nullptr; a.slabs = nullptr; a.db = nullptr;
}
static int c5_grid(int tiles, int cap) { return tiles < cap ? tiles : cap; }

extern "C" int pf_conv5v_supported(int H, int Wd, int C, int N, int k, int stride, int pad_h, int pad_w) {
  return (k == 5 && stride == 1 && pad_h == 0 && pad_w == 0 && c5_shape_ok(H, Wd, C, N)) ? 1 : 0;
}

extern "C" int pf_conv5v_fwd(const void* X, const void* W, const float* bias, void* Y, int imgs, int H, int Wd, int C, int N, void* stream) {
  if (!c5_shape_ok(H, Wd, C, N) || !c5_fits(imgs, H, Wd, C, N) || X == nullptr || W == nullptr || Y == nullptr || !pf_aligned16(Y) ||
      (((uintptr_t)bias) & 3) != 0 || (C == 32 ? (!pf_aligned16(X) || !pf_aligned16(W)) : ((((uintptr_t)X) | ((uintptr_t)W)) & 1) != 0))
    return (int)hipErrorInvalidValue;
  C5Args a;
  c5_fill(a, imgs, H, Wd, C, H - 4, Wd - 4, N, 0, C == 32 ? 80 : 8);
  a.X = (const bf16_t*)X; a.W = (const bf16_t*)W; a.bias = bias; a.Y = (bf16_t*)Y;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)a.nx * 1024;
  if (C == 3) {
    const int grid = c5_grid(a.n_tiles, C5_FWD3_GRID);
    return N == 32 ? pf_launch_lds(&k_conv5v_c3<2>, grid, C5_THREADS, lds, st, a) : pf_launch_lds(&k_conv5v_c3<4>, grid, C5_THREADS, lds, st, a);
  }
  const int grid = c5_grid(a.n_tiles, C5_FWD_GRID);
  return N == 32 ? pf_launch_lds(&k_conv5v<32, 32>, grid, C5_THREADS, lds, st, a) : pf_launch_lds(&k_conv5v<32, 64>, grid, C5_THREADS, lds, st, a);
}

// dX [imgs][H][Wd][C] = the full correlation of dY [imgs][H - 4][Wd - 4][N] with Wt [C][5][5][N], the flipped / transposed filter
extern "C" int pf_conv5v_bwd_data(const void* dY, const void* Wt, void* dX, int imgs, int H, int Wd, int C, int N, void* stream) {
  if (C != 32 || !c5_shape_ok(H, Wd, C, N) || !c5_fits(imgs, H, Wd, C, N) || dY == nullptr || Wt == nullptr || dX == nullptr ||
      !pf_aligned16(dY) || !pf_aligned16(Wt) || !pf_aligned16(dX))
    return (int)hipErrorInvalidValue;
  C5Args a;
  c5_fill(a, imgs, H - 4, Wd - 4, N, H, Wd, C, 4, 2 * N + 16);
  a.X = (const bf16_t*)dY; a.W = (const bf16_t*)Wt; a.Y = (bf16_t*)dX;
  hipStream_t st = (hipStream_t)stream;
  const int grid = c5_grid(a.n_tiles, C5_FWD_GRID);
  const size_t lds = (size_t)a.nx * 1024;
  return N == 32 ? pf_launch_lds(&k_conv5v<32, 32>, grid, C5_THREADS, lds, st, a) : pf_launch_lds(&k_conv5v<64, 32>, grid, C5_THREADS, lds, st, a);
}

// number of fp32 slabs pf_conv5v_wrw writes, one per workgroup, for pf_wrw_reduce and its workspace contract (0: not taken).  From
// the shape alone: the slab bytes written stay below FOUR times the operand bytes read (at the operand bytes, 15 workgroups at LeNet's
// conv2 and batch 128, the launch waits for their LDS reads); at most one slab per tile and C5_WRW_GRID.
extern "C" int pf_conv5v_wrw_slabs(int imgs, int H, int Wd, int C, int N) {
  if (!c5_shape_ok(H, Wd, C, N) || !c5_fits(imgs, H, Wd, C, N)) return 0;
  const int Ho = H - 4, Wo = Wd - 4;
  const int TR = c5_rows(Ho, Wo);
  const int64_t tiles = (int64_t)imgs * ((Ho + TR - 1) / TR);
  const int64_t operands = ((int64_t)imgs * H * Wd * C + (int64_t)imgs * Ho * Wo * N) * 2;
  int64_t S = 4 * operands / ((int64_t)N * 25 * C * 4);
  if (S > C5_WRW_GRID) S = C5_WRW_GRID;
  if (S > tiles) S = tiles;
  return S < 1 ? 1 : (int)S;
}

extern "C" int pf_conv5v_wrw(const void* dY, const void* X, void* dW, int dw_dtype, float* db, float* workspace, int imgs, int H, int Wd,
                             int C, int N, void* stream) {
  const int S = pf_conv5v_wrw_slabs(imgs, H, Wd, C, N);
  if (S <= 0 || dY == nullptr || X == nullptr || dW == nullptr || workspace == nullptr || !pf_aligned16(dY) || !pf_aligned16(dW) ||
      !pf_aligned16(workspace) || (((uintptr_t)db) & 3) != 0 || (C == 32 ? !pf_aligned16(X) : (((uintptr_t)X) & 1) != 0) ||
      (dw_dtype != PF_F32 && dw_dtype != PF_BF16))
    return (int)hipErrorInvalidValue;
  C5Args a;
  c5_fill(a, imgs, H, Wd, C, H - 4, Wd - 4, N, 0, C == 32 ? 96 : 8);
  a.ny = ((((a.TR * a.Wo + 31) >> 5) * 32) * (N == 32 ? 96 : 160) + 1023) / 1024;
  a.X = (const bf16_t*)X; a.dY = (const bf16_t*)dY; a.slabs = workspace;
  a.db = db != nullptr ? workspace + (int64_t)S * N * 25 * C : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)(a.nx + a.ny) * 1024;
  int r;
  if (C == 3) r = N == 32 ? pf_launch_lds(&k_conv5v_wrw_c3<2>, S, C5_THREADS, lds, st, a) : pf_launch_lds(&k_conv5v_wrw_c3<4>, S, C5_THREADS, lds, st, a);
  else r = N == 32 ? pf_launch_lds(&k_conv5v_wrw<32>, S, 256, lds, st, a) : pf_launch_lds(&k_conv5v_wrw<64>, S, 512, lds, st, a);
  if (r != 0) return r;
  if (db != nullptr && (r = pf_wrw_reduce(a.db, S, N, db, PF_F32, st)) != 0) return r;
  return pf_wrw_reduce(workspace, S, (int64_t)N * 25 * C, dW, dw_dtype, st);
}
