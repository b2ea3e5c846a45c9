// 3x3 / stride 1 / pad 1 convolutions with 16 or 32 input AND output channels (all four pairs) on image widths 16 | 32 | 48 | 64 and any
// height: the body of ResNet-20/32/56 @ CIFAR-10 (utils/external/resnet_model.py:92-103 with 16 / 32 filters; 11 of ResNet-20's 13 3x3
// layers behind the image convolution).  Forward (optionally + residual), backward-data (the same kernel, (C, N) swapped, on the flipped
// / transposed kernel) and backward-filter, ONE launch each.  Before this file these layers ran as im2col + the 1x1 kernels: a 9x-sized
// Xcol written and read back per pass (about 80 MB of traffic for a layer with 4 MB in and 4 MB out).
//
// A tap is 16 or 32 channels -- too narrow for the (tap, 64 channels) k-steps of pf_igemm.hip -- so the TAPS are folded into the K
// dimension of v_mfma_f32_16x16x32_bf16, k = tap * C + c (which is how KRSC memory is laid out already):
//   C = 32: nine k-steps, one tap each; lane group q = lane >> 4 reads channels 8q .. 8q + 7 of the tap's window pixel;
//   C = 16: FIVE k-steps, two taps each; q = 0, 1 read tap 2j, q = 2, 3 read tap 2j + 1 -- the tap shift is part of the lane's address.
//           The fifth step has only tap 8.  Two things must not happen to its q >= 2 lanes:
//             (1) their WEIGHT load, k = 144 .. 159, would run into the next filter (or past the buffer behind the last one): they get
//                 zeros WITHOUT a load (cn_weights);
//             (2) their INPUT operand must be zero as well, not whatever the window holds: 0 * Inf is NaN.  They read tap 8's address
//                 (inside the window) and the registers are replaced by zeros behind the wait (cn_fragment).
//
// Work split (k_conv3x3n).  A tile is TR whole image rows x all N output channels, TR = 4 for Wd <= 32, 2 above: 64 .. 128 output
// pixels = 4 .. 8 fragments of 16 (Wd % 16 == 0: a fragment never wraps an image row, so its window addresses are linear in the lane).
// Batch 128 at 32 x 32 gives 1024 tiles and at 16 x 16 gives 512: 4 / 2 workgroups on each of the 256 CUs, all of them resident at
// once (below) -- one workgroup's window travels while the others multiply, which is why there is ONE window per workgroup and no ring.
// Wavefront w takes fragments w, w + 4; every wavefront holds the WHOLE kernel (N x 9C bf16 = 9 .. 18 KiB over 64 lanes: 18 .. 72
// registers) for the life of the workgroup, read straight from KRSC memory.  The grid is min(tiles, 1024) persistent workgroups.
//
// Window.  (TR + 2) x (Wd + 2) pixels x C channels, staged ONCE per tile by LDS-DMA; padding rows / columns and the pitch padding are
// lanes with an out-of-range offset (zeros), as in pf_conv3x3_c64.hip.  Pixel pitch 2C + 16 bytes -- 80 (C = 32) or 48 (C = 16).  Bank
// arithmetic of a fragment read (ds_read_b128, sixteen lanes of one q = sixteen CONSECUTIVE window pixels, 64 banks of 4 bytes): pixel
// i starts at bank 20 i mod 64 = 0 20 40 60 16 36 56 12 32 52 8 28 48 4 24 44 (C = 32) or 12 i mod 64 = 0 12 24 36 48 60 8 20 32 44
// 56 4 16 28 40 52 (C = 16): sixteen distinct multiples of 4, so the sixteen 4-bank reads cover all 64 banks exactly once -- no
// conflict, for every tap (a tap only moves the first pixel).  With C = 16 the q < 2 and q >= 2 halves read different taps, each half
// again sixteen consecutive pixels.  At most 21 KiB (C = 32, Wd = 64).
//
// Output.  The MFMA leaves 4 consecutive output channels of pixel lane & 15 in each lane; a 16-pixel fragment is 16 N x 2 contiguous
// bytes of NHWC memory: 8 bytes per lane straight from the accumulators (RES: + the bf16 residual in float32, ONE rounding), no C tile
// through LDS.
//
// Backward-filter (k_wrw3x3n): dW[n][tap][c] = sum over pixels of dY[p][n] * X[p + tap][c].  The contraction runs over pixels, so both
// operands come from transposing LDS reads (ds_read_b64_tr_b16, as k_wrw2 / pf_wrw3x3_c64.hip): each lane supplies the address of ITS
// pixel row, which makes the window's row wrap and the tap shift free.  The X window and the dY tile (same tiles as forward) are staged
// once per tile; pitch 32 bytes (16 channels, dense) or 96 (32 channels): the eight 32-byte rows a half-wavefront reads then start at
// 0 32 .. 224 / 0 96 192 32 128 224 64 160 mod 256 -- all 64 banks once.  A workgroup is persistent over its tiles and keeps its share
// of the [N][9][C] float32 result in registers; the (N / 16) x (C / 16) x 9 accumulator blocks of 16 x 16 are split over the four
// wavefronts by block first, then by tap:
//     16 -> 16   1 block : taps {0 1 2} {3 4} {5 6} {7 8}           3 blocks = 12 accumulator registers at most
//     16 <-> 32  2 blocks: taps {0 .. 4} {5 .. 8} per block         5 blocks = 20
//     32 -> 32   4 blocks: one block per wavefront, all nine taps   9 blocks = 36
// One float32 slab [N][9][C] per workgroup (min(tiles, 256) of them: a slab is 9 .. 36 KiB, more would cost more traffic than the
// operands), folded by pf_wrw_reduce in a fixed order: deterministic, no atomics.  Rows of a tile past the image are zero rows of dY;
// like the other backward-filter kernels this one assumes FINITE activations (0 * Inf).
#include "pf_mfma.h"
#include "pf_buffer.h"

#define CN_THREADS 256
#define CN_FWD_GRID 1024
#define CN_WRW_GRID 256

struct Cn3Args {
  const bf16_t* X;      // [imgs][H][Wd][C]
  const bf16_t* W;      // [N][3][3][C]
  bf16_t* Y;            // [imgs][H][Wd][N]
  const bf16_t* R;      // residual, shape of Y (RES kernels only)
  const bf16_t* dY;     // backward-filter: [imgs][H][Wd][N]
  float* slabs;         // backward-filter: [gridDim.x][N][9][C]
  uint32_t x_bytes, y_bytes;
  int H, Wd, TR, tiles_per_img, n_tiles;
  int wpix, nx, ny;     // window pixels; 1 KiB LDS-DMA instructions of the window and (backward-filter) of the dY tile
};

// LDS reads beside a pending LDS-DMA come from inline asm and carry no wait: pf_lds_wait() and PF_TIE(reg) behind them (pf_mfma.h)
__device__ __forceinline__ void cn_read(uint32_t p, u32x4_t& v) { asm volatile("ds_read_b128 %0, %1" : "=&v"(v) : "v"(p) : "memory"); }

// one 1 KiB LDS-DMA instruction I of a [rows of `pitch` bytes] region: lane L fills bytes [I * 1024 + 16 L, + 16) = 16-byte group ck of
// row `row`; the caller turns (row, ck) into a byte offset of the tensor or PF_BUFFER_OOB (zeros)
template <int PITCH>
__device__ __forceinline__ void cn_slot(int I, int lane, int& row, int& ck) {
  const int byte = I * 1024 + lane * 16;
  row = byte / PITCH;
  ck = (byte - row * PITCH) >> 4;
}

// the input window of tile (img, h0) -> LDS at `dst`: window pixel (wr, wc) is image pixel (h0 - 1 + wr, wc - 1)
template <int C, int PITCH>
__device__ __forceinline__ void cn_stage_window(const Cn3Args& a, pf_rsrc_t rsX, unsigned char* dst, int img, int h0, int wave, int lane) {
  const int WC = a.Wd + 2;
  for (int I = wave; I < a.nx; I += CN_THREADS / 64) {                       // wave-uniform
    int wp, ck;
    cn_slot<PITCH>(I, lane, wp, ck);
    const int wr = wp / WC, wc = wp - wr * WC;
    const int h = h0 - 1 + wr, x = wc - 1;
    const bool ok = wp < a.wpix && ck < C / 8 && x >= 0 && x < a.Wd && h >= 0 && h < a.H;
    const uint32_t voff = ok ? (uint32_t)((((img * a.H + h) * a.Wd + x) * C + ck * 8) * 2) : PF_BUFFER_OOB;
    PF_BUFFER_LOAD_LDS16(rsX, dst + I * 1024, voff, 0);
  }
}

// ---- forward / backward-data ---------------------------------------------------------------------------------------------------------
template <int C, int N, bool RES>
__global__ __launch_bounds__(CN_THREADS, 2) void k_conv3x3n(const Cn3Args a) {
  constexpr int PITCH = 2 * C + 16, KS = (C == 32) ? 9 : 5, NB = N / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int WC = a.Wd + 2;
  const int fpr = a.Wd >> 4, nfrag = a.TR * fpr;                             // fragments per image row / per tile (4 .. 8)
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};

  // ---- the kernel, once: W[n][k], k = tap * C + c; k-step j = 32 consecutive k, this lane's eight at 32 j + 8 q ----------------
  bf16x8 w[NB][KS];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      u32x4_t v = zero4;
      if (!(C == 16 && j == 4 && q >= 2))                                    // (1) of the header: k >= 144 is not this filter's
        v = *reinterpret_cast<const u32x4_t*>(a.W + (nb * 16 + l15) * (9 * C) + j * 32 + q * 8);
      w[nb][j] = *reinterpret_cast<const bf16x8*>(&v);
    }

  // ---- this lane's byte offset of k-step j inside the window, relative to the fragment's pixel -----------------------------------
  uint32_t toff[KS];
#pragma unroll
  for (int j = 0; j < KS; ++j) {
    int tap = (C == 32) ? j : 2 * j + (q >> 1);
    tap = tap < 8 ? tap : 8;                                                 // (2): the fifth step's q >= 2 lanes read tap 8's pixel
    toff[j] = (uint32_t)(((tap / 3) * WC + tap % 3) * PITCH + ((C == 32) ? q : (q & 1)) * 16);
  }

  const pf_rsrc_t rsX = PF_MAKE_RSRC(a.X, a.x_bytes);
  for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const int img = t / a.tiles_per_img, h0 = (t - img * a.tiles_per_img) * a.TR;
    cn_stage_window<C, PITCH>(a, rsX, smem, img, h0, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    for (int f = wave; f < nfrag; f += CN_THREADS / 64) {                    // wave-uniform
      const int tr = f / fpr, c0 = (f - tr * fpr) * 16;
      if (h0 + tr >= a.H) break;                                             // the rows of the last tile behind the image
      const uint32_t xb = lds_addr(smem) + (uint32_t)((tr * WC + c0 + l15) * PITCH);
      f32x4 acc[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
      u32x4_t x[KS];
#pragma unroll
      for (int j = 0; j < KS; ++j) cn_read(xb + toff[j], x[j]);
      pf_lds_wait();
#pragma unroll
      for (int j = 0; j < KS; ++j) PF_TIE(x[j]);
      if (C == 16 && q >= 2) x[KS - 1] = zero4;                              // (2)
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&x[j]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[nb][j], xf, acc[nb], 0, 0, 0);
      }
      // lane (q, l15): output channels nb * 16 + 4 q .. + 3 of pixel (h0 + tr, c0 + l15)
      const int64_t m = (int64_t)((img * a.H + h0 + tr) * a.Wd + c0 + l15) * N + q * 4;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (RES) {
          const uint2 r = *reinterpret_cast<const uint2*>(a.R + m + nb * 16);
          acc[nb][0] += __uint_as_float(r.x << 16); acc[nb][1] += __uint_as_float(r.x & 0xFFFF0000u);
          acc[nb][2] += __uint_as_float(r.y << 16); acc[nb][3] += __uint_as_float(r.y & 0xFFFF0000u);
        }
        *reinterpret_cast<uint2*>(a.Y + m + nb * 16) = make_uint2(pack_bf16x2(acc[nb][0], acc[nb][1]), pack_bf16x2(acc[nb][2], acc[nb][3]));
      }
    }
    __builtin_amdgcn_s_barrier();                                            // every wavefront is done reading the window
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- backward-filter -----------------------------------------------------------------------------------------------------------------
template <int C, int N>
__global__ __launch_bounds__(CN_THREADS, 2) void k_wrw3x3n(const Cn3Args a) {
  constexpr int XP = (C == 16) ? 32 : 96, YP = (N == 16) ? 32 : 96;         // pixel pitches (header)
  constexpr int CB = C / 16, NBLK = (N / 16) * CB, WPB = 4 / NBLK;           // wavefronts per 16 x 16 block of (n, c)
  constexpr int MAXT = (WPB == 1) ? 9 : (WPB == 2 ? 5 : 3);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // input window | dY tile
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int WC = a.Wd + 2;
  const int blk = wave / WPB, tg = wave - blk * WPB;
  const int nb = blk / CB, cb = blk - nb * CB;
  const int tap0 = (WPB == 1) ? 0 : (WPB == 2 ? 5 * tg : (tg == 0 ? 0 : 1 + 2 * tg));
  const int ntap = (WPB == 1) ? 9 : (WPB == 2 ? 5 - tg : (tg == 0 ? 3 : 2));
  const int TP = a.TR * a.Wd, nkb = TP >> 5;                                 // tile pixels (a multiple of 32: TR is even), 32-pixel k-blocks
  const pf_rsrc_t rsX = PF_MAKE_RSRC(a.X, a.x_bytes);
  const pf_rsrc_t rsY = PF_MAKE_RSRC(a.dY, a.y_bytes);
  unsigned char* ys = smem + a.nx * 1024;

  // fragment addresses.  A transposing read takes, from lane (q, l15), 8 bytes of pixel row q * 4 + (l15 >> 2) (+ 16 for the second
  // read of a fragment) at channel quad l15 & 3 and leaves every lane with four pixels of ONE channel; dY and X use the same pixel
  // order, so the contraction is consistent.  dY rows are linear in the tile pixel, X rows go through the window map.
  const int pr = q * 4 + (l15 >> 2);
  const uint32_t dyb = lds_addr(ys) + (uint32_t)(pr * YP + nb * 32 + (l15 & 3) * 8);
  uint32_t xb[4][2];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int hi = 0; hi < 2; ++hi) {
      int p = kb * 32 + hi * 16 + pr;
      p = p < TP ? p : TP - 1;                                               // (kb >= nkb: never read)
      const int tr = p / a.Wd;
      xb[kb][hi] = lds_addr(smem) + (uint32_t)((tr * WC + (p - tr * a.Wd)) * XP + cb * 32 + (l15 & 3) * 8);
    }
  uint32_t toff[MAXT];                                                       // wave-uniform: the tap shifts of this wavefront's taps
#pragma unroll
  for (int e = 0; e < MAXT; ++e) {
    const int tap = (e < ntap) ? tap0 + e : tap0;
    toff[e] = (uint32_t)(((tap / 3) * WC + tap % 3) * XP);
  }

  f32x4 acc[MAXT];
#pragma unroll
  for (int e = 0; e < MAXT; ++e) acc[e] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const int img = t / a.tiles_per_img, h0 = (t - img * a.tiles_per_img) * a.TR;
    cn_stage_window<C, XP>(a, rsX, smem, img, h0, wave, lane);
    const int valid = ((a.H - h0) < a.TR ? (a.H - h0) : a.TR) * a.Wd;        // tile pixels inside the image; the rest: zero rows
    for (int I = wave; I < a.ny; I += CN_THREADS / 64) {
      int row, ck;
      cn_slot<YP>(I, lane, row, ck);
      const bool ok = row < valid && ck < N / 8;
      const uint32_t voff = ok ? (uint32_t)((((img * a.H + h0) * a.Wd + row) * N + ck * 8) * 2) : PF_BUFFER_OOB;
      PF_BUFFER_LOAD_LDS16(rsY, ys + I * 1024, voff, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      if (kb < nkb) {
        pf_v4s d[2], v[MAXT][2];
        pf_tr_issue(dyb + (uint32_t)(kb * 32 * YP), d[0]);
        pf_tr_issue(dyb + (uint32_t)((kb * 32 + 16) * YP), d[1]);
#pragma unroll
        for (int e = 0; e < MAXT; ++e) {
          pf_tr_issue(xb[kb][0] + toff[e], v[e][0]);
          pf_tr_issue(xb[kb][1] + toff[e], v[e][1]);
        }
        pf_lds_wait();
        PF_TIE(d[0]); PF_TIE(d[1]);
#pragma unroll
        for (int e = 0; e < MAXT; ++e) { PF_TIE(v[e][0]); PF_TIE(v[e][1]); }
        const bf16x8 df = pf_join(d[0], d[1]);
#pragma unroll
        for (int e = 0; e < MAXT; ++e)
          if (e < ntap) acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, pf_join(v[e][0], v[e][1]), acc[e], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_barrier();                                            // every wavefront is done with the tile
    __builtin_amdgcn_sched_barrier(0);
  }

  // slab [N][9][C]: accumulator block e holds rows n = nb * 16 + 4 q + r, column k = (tap0 + e) * C + cb * 16 + l15
  float* out = a.slabs + (int64_t)blockIdx.x * (N * 9 * C) + (nb * 16 + q * 4) * (9 * C) + cb * 16 + l15;
#pragma unroll
  for (int e = 0; e < MAXT; ++e)
    if (e < ntap) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[r * (9 * C) + (tap0 + e) * C] = acc[e][r];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static bool cn_shape_ok(int H, int Wd, int C, int N) {
  return (C == 16 || C == 32) && (N == 16 || N == 32) && H >= 1 && Wd >= 16 && Wd <= 64 && (Wd % 16) == 0;
}
// 31-bit byte offsets of both tensors
static bool cn_fits(int imgs, int H, int Wd, int C, int N) {
  return imgs > 0 && (int64_t)imgs * H * Wd * (C > N ? C : N) * 2 < ((int64_t)1 << 31);
}
// the tiling both kernels share; `pitch`: bytes per window pixel
static void cn_fill(Cn3Args& a, int imgs, int H, int Wd, int C, int N, int pitch) {
  a.H = H; a.Wd = Wd;
  a.TR = (Wd <= 32) ? 4 : 2;
  a.tiles_per_img = (H + a.TR - 1) / a.TR;
  a.n_tiles = imgs * a.tiles_per_img;
  a.wpix = (a.TR + 2) * (Wd + 2);
  a.nx = (a.wpix * pitch + 1023) / 1024;
  a.ny = 0;
  a.x_bytes = (uint32_t)((int64_t)imgs * H * Wd * C * 2);
  a.y_bytes = (uint32_t)((int64_t)imgs * H * Wd * N * 2);
  a.R = nullptr; a.dY = nullptr; a.slabs = nullptr;
}

extern "C" int pf_conv3x3n_supported(int H, int Wd, int C, int N, int stride, int pad_h, int pad_w) {
  return (stride == 1 && pad_h == 1 && pad_w == 1 && cn_shape_ok(H, Wd, C, N)) ? 1 : 0;
}

template <int C, int N>
static int cn_fwd_launch(const Cn3Args& a, hipStream_t st) {
  const int grid = a.n_tiles < CN_FWD_GRID ? a.n_tiles : CN_FWD_GRID;
  const size_t lds = (size_t)a.nx * 1024;
  if (a.R != nullptr) k_conv3x3n<C, N, true><<<grid, CN_THREADS, lds, st>>>(a);
  else k_conv3x3n<C, N, false><<<grid, CN_THREADS, lds, st>>>(a);
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_conv3x3n_fwd(const void* X, const void* W, void* Y, const void* R, int imgs, int H, int Wd, int C, int N, void* stream) {
  if (!cn_shape_ok(H, Wd, C, N) || !cn_fits(imgs, H, Wd, C, N) || X == nullptr || W == nullptr || Y == nullptr ||
      !pf_aligned16(X) || !pf_aligned16(W) || !pf_aligned16(Y) || !pf_aligned16(R))
    return (int)hipErrorInvalidValue;
  Cn3Args a;
  cn_fill(a, imgs, H, Wd, C, N, 2 * C + 16);
  a.X = (const bf16_t*)X; a.W = (const bf16_t*)W; a.Y = (bf16_t*)Y; a.R = (const bf16_t*)R;
  hipStream_t st = (hipStream_t)stream;
  if (C == 16) return N == 16 ? cn_fwd_launch<16, 16>(a, st) : cn_fwd_launch<16, 32>(a, st);
  return N == 16 ? cn_fwd_launch<32, 16>(a, st) : cn_fwd_launch<32, 32>(a, st);
}

// number of fp32 slabs pf_conv3x3n_wrw writes, one per workgroup, for pf_wrw_reduce and its workspace contract (0: not taken)
extern "C" int pf_conv3x3n_wrw_slabs(int imgs, int H, int Wd, int C, int N) {
  if (!cn_shape_ok(H, Wd, C, N) || !cn_fits(imgs, H, Wd, C, N)) return 0;
  const int TR = (Wd <= 32) ? 4 : 2;
  const int64_t tiles = (int64_t)imgs * ((H + TR - 1) / TR);
  return tiles < CN_WRW_GRID ? (int)tiles : CN_WRW_GRID;
}

template <int C, int N>
static int cn_wrw_launch(const Cn3Args& a, int S, hipStream_t st) {
  k_wrw3x3n<C, N><<<S, CN_THREADS, (size_t)(a.nx + a.ny) * 1024, st>>>(a);
  PF_LAUNCH_CHECK();
  return 0;
}

extern "C" int pf_conv3x3n_wrw(const void* dY, const void* X, void* dW, int dw_dtype, float* workspace, int imgs, int H, int Wd, int C,
                               int N, void* stream) {
  const int S = pf_conv3x3n_wrw_slabs(imgs, H, Wd, C, N);
  if (S <= 0 || dY == nullptr || X == nullptr || dW == nullptr || workspace == nullptr || !pf_aligned16(dY) || !pf_aligned16(X) ||
      !pf_aligned16(dW) || !pf_aligned16(workspace) || (dw_dtype != PF_F32 && dw_dtype != PF_BF16))
    return (int)hipErrorInvalidValue;
  Cn3Args a;
  cn_fill(a, imgs, H, Wd, C, N, C == 16 ? 32 : 96);
  a.ny = (a.TR * Wd * (N == 16 ? 32 : 96) + 1023) / 1024;
  a.X = (const bf16_t*)X; a.dY = (const bf16_t*)dY; a.slabs = workspace;
  a.W = nullptr; a.Y = nullptr;
  hipStream_t st = (hipStream_t)stream;
  int r;
  if (C == 16) r = (N == 16) ? cn_wrw_launch<16, 16>(a, S, st) : cn_wrw_launch<16, 32>(a, S, st);
  else r = (N == 16) ? cn_wrw_launch<32, 16>(a, S, st) : cn_wrw_launch<32, 32>(a, S, st);
  if (r != 0) return r;
  return pf_wrw_reduce(workspace, S, (int64_t)N * 9 * C, dW, dw_dtype, st);
}
