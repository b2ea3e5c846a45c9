// Third member of the stem family: 3x3 convolution of a 3-channel image at stride 1 OR 2 to any N % 8 == 0, 8 <= N <= 64, forward
// and backward-filter, NHWC bf16 with float32 accumulation on v_mfma_f32_16x16x32_bf16.  It takes what pf_stem3.hip (stride 2, N = 16 |
// 32, Wo % 16 == 0) refuses: the CIFAR ResNet-20/32/56 stem (3 -> 16, stride 1, pad 1, 32 x 32) and the MobileNet stems of width 8,
// 24 and 48 (depth multipliers 0.25 / 0.75 / 1.4), which ran on the vector-ALU kernel of pf_convg.hip before.
//
// Staging is the family's: a workgroup stages the input rows of its output strip ONCE in LDS, pixels padded from 3 to 4 channels
// (8 bytes), the image's first pixel at LDS pixel `pw`, zeros around it (stem_stage_row; rows outside the image are staged as zeros).
// The image is never copied or padded in HBM; no atomics; the order of every sum is fixed by the shape.
//
// Forward.  k' = s * 4 + c per kernel row r, one MFMA k-step per row, zero WEIGHTS at c = 3 and s >= 3.  A lane (l16, g) feeds taps
// (2g, 2g + 1) x 4 channels of output pixel ox = 16 pb + l16: sixteen bytes at LDS pixel STRIDE * ox + 2g of row STRIDE * orow + r.
//   * stride 2: the address is 16-byte aligned, one ds_read_b128 as in k_stem3x3_fwd.
//   * stride 1: at odd ox it is 8-byte aligned only.  Chosen here: TWO ds_read_b64 (the compiler pairs them into one ds_read2_b64); no
//     second staged copy, no lane permutation.  Bank picture: the lanes g = 2, 3 carry zero weights only and read the addresses of g = 0,
//     1 (g & 1), so the 64 lanes of one read touch the 18 consecutive padded pixels 16 pb .. 16 pb + 17 = 144 contiguous bytes = 36
//     consecutive banks of the 64: no two different dwords share a bank, lanes with the same address are one broadcast.
//   * weights are operand A, packed once per workgroup from global memory straight into registers.  MFMA row i of channel block nb is
//     output channel 4 NB (i / 4) + 4 nb + (i % 4), NB = 1 | 2 | 4 blocks for N <= 16 | 32 | 64, so a lane ends with 4 NB CONSECUTIVE
//     channels of its pixel: 8- / 16-byte stores straight from the accumulators, no C tile through LDS.  Rows n >= N carry zero weights
//     (W[n] is not loaded) and their pieces are not stored: N % 8 == 0 makes every 8- / 16-byte piece wholly inside or outside.
//   * a ragged last pixel block (Wo % 16 != 0) reads the row's last pixel again and stores nothing.
//   * output rows per item: 4 at stride 1 (6 staged rows), 8 at stride 2 (17): 128 x 32 x 32 gives 1024 resp. 256 items for 256 CUs.
//
// Backward-filter.  dW[n][r][s][c] = sum over pixels of dY[pixel][n] * X[window(pixel)][r][s][c]: the contraction runs over pixels, both
// operands are pixel-major in LDS and are fetched with ds_read_b64_tr_b16 as in k_stem3x3_wrw: dY in [8 pixels][16 channels] blocks
// filled by LDS-DMA (channels >= N and pixels behind the strip are out-of-range offsets: zeros), X pieces = one padded pixel each.  The
// 3 * ceil(N / 16) (channel block, kernel row) accumulators are dealt to the four wavefronts; pixels of a strip are taken 32 per step in
// linear order over its rows, so Wo needs no divisibility.  One float32 slab [N][27] per persistent workgroup, folded by pf_wrw_reduce.
//
// Pixels must be FINITE (as for pf_stem3.hip): zero weights / zero dY multiply real neighbouring pixels.
#include "pf_stem.h"

#define S3X_OROWS1 4                    // forward, stride 1: output rows per item
#define S3X_OROWS2 8                    // forward, stride 2

struct Stem3xArgs {
  const bf16_t* X;   // [imgs][H][Wd][3]
  const bf16_t* W;   // [N][3][3][3]
  bf16_t* Y;         // [imgs][Ho][Wo][N]
  int imgs, H, Wd, Ho, Wo, ph, pw;
  int strips, n_items;
  int rsb;           // LDS bytes per staged input row = (Wd + 8) * 8
  int N;
  int tsh;           // log2 of the threads that stage one row (the smallest power of two >= Wd / 2, 8 .. 128)
};
struct Stem3xWrwArgs {
  const bf16_t* dY;  // [imgs][Ho][Wo][N]
  const bf16_t* X;
  float* slabs;      // [S][N][27]
  int imgs, H, Wd, Ho, Wo, ph, pw;
  int strips, n_items;
  int rsb;
  int dy_bytes;
  int N;
  int tsh;
  int orows;         // output rows per item (s3x_wrw_rows)
};

// halo pixels of every staged row, once per workgroup: LDS pixels [0, pw) and [pw + Wd, Wd + 8)
template <class Args>
__device__ __forceinline__ void s3x_zero_halo(unsigned char* xs, const Args& a, int irows, int tid) {
  for (int t = tid; t < irows * 8; t += ST_THREADS) {
    const int row = t >> 3, h = t & 7;
    const int pp = h < a.pw ? h : a.Wd + h;
    *reinterpret_cast<uint2*>(xs + row * a.rsb + pp * 8) = make_uint2(0u, 0u);
  }
}
// the `irows` input rows from iy0 on of image `img`, 2^tsh threads per row and 256 >> tsh rows at a time
template <class Args>
__device__ __forceinline__ void s3x_stage(unsigned char* xs, const Args& a, int img, int iy0, int irows, int tid) {
  const int tpr = 1 << a.tsh;
  for (int row = tid >> a.tsh; row < irows; row += ST_THREADS >> a.tsh) {
    const int iy = iy0 + row;
    stem_stage_row(xs + row * a.rsb + a.pw * 8, a.X, ((int64_t)img * a.H + iy) * a.Wd * 3, iy >= 0 && iy < a.H, a.Wd >> 1, tid & (tpr - 1), tpr);
  }
}

template <int STRIDE, int NB>
__global__ __launch_bounds__(ST_THREADS) void k_stem3x_fwd(Stem3xArgs a) {
  constexpr int OROWS = STRIDE == 1 ? S3X_OROWS1 : S3X_OROWS2;
  constexpr int IROWS = STRIDE * OROWS + 3 - STRIDE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* xs = smem;                               // staged rows [IROWS][(Wd + 8)][4] bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, g = lane >> 4;

  // ---- A fragments: taps (2g, 2g + 1) x 4 channels of kernel row r of this lane's output channel; g >= 2, tap 3, c = 3, n >= N: zeros ----
  bf16x8 wf[NB][3];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = 4 * NB * (l16 >> 2) + 4 * nb + (l16 & 3);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (g < 2 && n < a.N) {
        const bf16_t* src = a.W + ((n * 3 + r) * 3 + 2 * g) * 3;
        const uint32_t e0 = src[0], e1 = src[1], e2 = src[2];
        v.x = e0 | (e1 << 16); v.y = e2;
        if (g == 0) {                                     // tap 1 exists, tap 3 does not
          const uint32_t f0 = src[3], f1 = src[4], f2 = src[5];
          v.z = f0 | (f1 << 16); v.w = f2;
        }
      }
      wf[nb][r] = *reinterpret_cast<const bf16x8*>(&v);
    }
  }
  s3x_zero_halo(xs, a, IROWS, tid);

  const int pblocks = (a.Wo + 15) >> 4;                   // 16-pixel blocks per output row, the last one ragged
  const int units = OROWS * pblocks;
  for (int item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    const int img = item / a.strips, strip = item - img * a.strips;
    const int oy0 = strip * OROWS;
    __syncthreads();                                      // the previous item's fragment reads are done
    s3x_stage(xs, a, img, STRIDE * oy0 - a.ph, IROWS, tid);
    __syncthreads();
    for (int u = wave; u < units; u += ST_THREADS / 64) {
      const int orow = u / pblocks, pb = u - orow * pblocks;
      const int oy = oy0 + orow;
      if (oy >= a.Ho) continue;
      const int ox = pb * 16 + l16;
      const int oxr = ox < a.Wo ? ox : a.Wo - 1;
      const unsigned char* base = xs + (STRIDE * orow) * a.rsb + (STRIDE * oxr + 2 * (g & 1)) * 8;
      f32x4 acc[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        uint4 xv;
        if constexpr (STRIDE == 2) {
          xv = *reinterpret_cast<const uint4*>(base + r * a.rsb);
        } else {
          const uint2 lo = *reinterpret_cast<const uint2*>(base + r * a.rsb), hi = *reinterpret_cast<const uint2*>(base + r * a.rsb + 8);
          xv = make_uint4(lo.x, lo.y, hi.x, hi.y);
        }
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&xv);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb][r], xf, acc[nb], 0, 0, 0);
      }
      if (ox >= a.Wo) continue;
      bf16_t* out = a.Y + (((int64_t)img * a.Ho + oy) * a.Wo + ox) * a.N;
      if constexpr (NB == 1) {                            // lane: pixel ox, channels 4g + j
        if (4 * g < a.N) *reinterpret_cast<uint2*>(out + 4 * g) = make_uint2(pack_bf16x2(acc[0][0], acc[0][1]), pack_bf16x2(acc[0][2], acc[0][3]));
      } else {                                            // channels 4 NB g + 4 nb + j, eight per store
#pragma unroll
        for (int h = 0; h < NB / 2; ++h) {
          const int c0 = 4 * NB * g + 8 * h;
          if (c0 < a.N)
            *reinterpret_cast<uint4*>(out + c0) = make_uint4(pack_bf16x2(acc[2 * h][0], acc[2 * h][1]), pack_bf16x2(acc[2 * h][2], acc[2 * h][3]),
                                                             pack_bf16x2(acc[2 * h + 1][0], acc[2 * h + 1][1]), pack_bf16x2(acc[2 * h + 1][2], acc[2 * h + 1][3]));
        }
      }
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// 3 -> N channels, 3x3, stride 1 | 2, N % 8 == 0 in 8 .. 64, FRONT pads in {0, 1}, any H >= 1, Wd % 8 == 0 in 16 .. 256 (the staged row
// and the two-pixel staging tasks).  Ho / Wo are the caller's; the last window may reach ONE row / column behind the image (symmetric pad
// 1, TF 'SAME'), so that every LDS read lies inside the staged rows: pixel STRIDE (Wo - 1) + 3 <= Wd + 2.
static bool s3x_shape_ok(int H, int Wd, int C, int N, int k, int stride, int ph, int pw, int Ho, int Wo) {
  return C == 3 && k == 3 && (stride == 1 || stride == 2) && N >= 8 && N <= 64 && (N % 8) == 0 && H >= 1 && Wd >= 16 && Wd <= 256 &&
         (Wd % 8) == 0 && ph >= 0 && ph <= 1 && pw >= 0 && pw <= 1 && Ho >= 1 && Wo >= 1 &&
         (int64_t)stride * (Wo - 1) + 2 - pw <= Wd && (int64_t)stride * (Ho - 1) + 2 - ph <= H;
}
static bool s3x_bytes_ok(int imgs, int H, int Wd, int N, int Ho, int Wo) {
  return imgs > 0 && (int64_t)imgs * H * Wd * 6 < ((int64_t)1 << 31) && stem_dy_fits(imgs, Ho, Wo, N);
}
static int s3x_tsh(int Wd) {
  int sh = 3;
  while ((1 << sh) < (Wd >> 1)) ++sh;
  return sh;
}

extern "C" int pf_conv_stem3x_supported(int H, int Wd, int C, int N, int k, int stride, int pad_h, int pad_w, int Ho, int Wo) {
  return s3x_shape_ok(H, Wd, C, N, k, stride, pad_h, pad_w, Ho, Wo) ? 1 : 0;
}

template <int STRIDE, int NB>
static int s3x_launch_fwd(const Stem3xArgs& a, hipStream_t st) {
  constexpr int OROWS = STRIDE == 1 ? S3X_OROWS1 : S3X_OROWS2;
  const size_t lds = (size_t)(STRIDE * OROWS + 3 - STRIDE) * a.rsb;
  return pf_launch_lds(&k_stem3x_fwd<STRIDE, NB>, stem_grid(a.n_items, 1024), ST_THREADS, lds, st, a);
}

extern "C" int pf_conv_stem3x_fwd(const void* X, const void* W, void* Y, int imgs, int H, int Wd, int N, int stride, int pad_h, int pad_w,
                                  int Ho, int Wo, void* stream) {
  Stem3xArgs a;
  if (!s3x_shape_ok(H, Wd, 3, N, 3, stride, pad_h, pad_w, Ho, Wo) || !s3x_bytes_ok(imgs, H, Wd, N, Ho, Wo) ||
      !stem_fill(a, X, Y, W, imgs, H, Wd, Ho, Wo, stride == 1 ? S3X_OROWS1 : S3X_OROWS2))
    return (int)hipErrorInvalidValue;
  a.W = (const bf16_t*)W; a.Y = (bf16_t*)Y; a.ph = pad_h; a.pw = pad_w; a.N = N; a.tsh = s3x_tsh(Wd);
  hipStream_t st = (hipStream_t)stream;
  const int nb = N <= 16 ? 1 : (N <= 32 ? 2 : 4);
  if (stride == 1) return nb == 1 ? s3x_launch_fwd<1, 1>(a, st) : nb == 2 ? s3x_launch_fwd<1, 2>(a, st) : s3x_launch_fwd<1, 4>(a, st);
  return nb == 1 ? s3x_launch_fwd<2, 1>(a, st) : nb == 2 ? s3x_launch_fwd<2, 2>(a, st) : s3x_launch_fwd<2, 4>(a, st);
}

// =================================================================================================================
// Backward-filter.  NB = ceil(N / 16) channel blocks in natural order; accumulator p = 3 nb + r; wavefront w owns p = PW w .. PW w + PW - 1,
// PW = ceil(3 NB / 4) (NB = 1: one kernel row each, the fourth wavefront only stages).
// =================================================================================================================
template <int STRIDE, int NB>
__global__ __launch_bounds__(ST_THREADS) void k_stem3x_wrw(Stem3xWrwArgs a) {
  constexpr int PW = (3 * NB + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int irows = STRIDE * a.orows + 3 - STRIDE;
  unsigned char* xs = smem;                                 // staged input rows [irows][(Wd + 8)][4] bf16
  unsigned char* dys = smem + irows * a.rsb;                // dY blocks [steps][4 pixel groups][NB channel blocks][8][16] bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const pf_rsrc_t rsY = PF_MAKE_RSRC(a.dY, a.dy_bytes);
  // role inside one LDS-DMA instruction: 1 KiB = four [8 pixels][16 channels] blocks, block index = pixel group * NB + channel block
  const int srow = (lane & 15) >> 1, sch = lane & 1;
  const int tr_off = (q & 1) * 128 + (l15 >> 2) * 32 + (l15 & 3) * 8;       // piece of the transposed read (as in k_stem3x3_wrw)
  const int pg_lo = q >> 1;
  const int p_lo = 8 * pg_lo + 4 * (q & 1) + (l15 >> 2);                    // the pixel (within a 32-pixel step) whose X piece this lane addresses
  const int steps = (a.orows * a.Wo + 31) >> 5;

  f32x4 acc[PW];
#pragma unroll
  for (int i = 0; i < PW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  s3x_zero_halo(xs, a, irows, tid);

  for (int item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    const int img = item / a.strips, strip = item - img * a.strips;
    const int oy0 = strip * a.orows;
    const int valid_px = ((a.Ho - oy0) < a.orows ? (a.Ho - oy0) : a.orows) * a.Wo;
    const int64_t m_base = ((int64_t)img * a.Ho + oy0) * a.Wo;
    __syncthreads();                                        // the previous item's reads are done
    // ---- dY: steps x 4 pixel groups x NB channel blocks, one LDS-DMA instruction per KiB; zeros behind the strip and behind channel N - 1 ----
    for (int id = wave; id < steps * NB; id += ST_THREADS / 64) {
      const int blk = id * 4 + (lane >> 4);
      const int pg = blk / NB, sb = blk - pg * NB;
      const int lin = pg * 8 + srow, ch0 = 16 * sb + 8 * sch;
      const uint32_t voff = (lin < valid_px && ch0 < a.N) ? (uint32_t)(((m_base + lin) * a.N + ch0) * 2) : PF_BUFFER_OOB;
      PF_BUFFER_LOAD_LDS16(rsY, dys + id * 1024, voff, 0);
    }
    s3x_stage(xs, a, img, STRIDE * oy0 - a.ph, irows, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // this lane's two pixels of a step, lin = 32 st + p_lo and + 16, as (output row of the strip, ox): advanced, never divided
    int ox0 = p_lo, or0 = 0, ox1 = p_lo + 16, or1 = 0;
    while (ox0 >= a.Wo) { ox0 -= a.Wo; ++or0; }
    while (ox1 >= a.Wo) { ox1 -= a.Wo; ++or1; }
    for (int st = 0; st < steps; ++st) {
      const unsigned char* dbase = dys + st * (4 * NB * 256) + tr_off;
      // (pixels behind the strip's rows meet zero dY: any staged pixel will do for them)
      const unsigned char* xlo = xs + (or0 < a.orows ? (STRIDE * or0) * a.rsb + (STRIDE * ox0) * 8 : 0) + (l15 & 3) * 8;
      const unsigned char* xhi = xs + (or1 < a.orows ? (STRIDE * or1) * a.rsb + (STRIDE * ox1) * 8 : 0) + (l15 & 3) * 8;
#pragma unroll
      for (int i = 0; i < PW; ++i) {
        const int p = wave * PW + i;
        if (p < 3 * NB) {
          const int nb = p / 3, r = p - 3 * nb;
          const pf_v4s dlo = pf_tr_read(dbase + (pg_lo * NB + nb) * 256);
          const pf_v4s dhi = pf_tr_read(dbase + ((pg_lo + 2) * NB + nb) * 256);
          const pf_v4s lo = pf_tr_read(xlo + r * a.rsb);
          const pf_v4s hi = pf_tr_read(xhi + r * a.rsb);
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf_join(dlo, dhi), pf_join(lo, hi), acc[i], 0, 0, 0);
        }
      }
      ox0 += 32; ox1 += 32;
      while (ox0 >= a.Wo) { ox0 -= a.Wo; ++or0; }
      while (ox1 >= a.Wo) { ox1 -= a.Wo; ++or1; }
    }
  }
  // ---- slab [N][3][3][3]: lane (q, l15) holds rows n = 16 nb + 4q + j, column k' = (s = l15 / 4, c = l15 % 4) of kernel row r ----
  float* slab = a.slabs + (int64_t)blockIdx.x * (a.N * 27);
  const int s = l15 >> 2, c = l15 & 3;
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int p = wave * PW + i;
    if (p < 3 * NB && s < 3 && c < 3) {
      const int nb = p / 3, r = p - 3 * nb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = 16 * nb + 4 * q + j;
        if (n < a.N) slab[n * 27 + (r * 3 + s) * 3 + c] = acc[i][j];
      }
    }
  }
}

// output rows per backward-filter item: about 256 pixels (8 x 32 on the CIFAR map, 2 x 112 on the 224 x 224 / 2 one), 1 .. 8 rows
static int s3x_wrw_rows(int Wo) {
  const int r = 256 / Wo;
  return r < 1 ? 1 : (r > 8 ? 8 : r);
}

// number of fp32 slabs pf_conv_stem3x_wrw writes, one per workgroup, for pf_wrw_reduce and its workspace contract (0: unsupported)
extern "C" int pf_conv_stem3x_wrw_slabs(int imgs, int H, int Wd, int N, int stride, int pad_h, int pad_w, int Ho, int Wo) {
  if (!s3x_shape_ok(H, Wd, 3, N, 3, stride, pad_h, pad_w, Ho, Wo) || !s3x_bytes_ok(imgs, H, Wd, N, Ho, Wo)) return 0;
  return stem_grid(imgs * stem_strips(Ho, s3x_wrw_rows(Wo)), 768);
}

template <int STRIDE, int NB>
static int s3x_launch_wrw(const Stem3xWrwArgs& a, int S, hipStream_t st) {
  const int steps = (a.orows * a.Wo + 31) >> 5;
  const size_t lds = (size_t)(STRIDE * a.orows + 3 - STRIDE) * a.rsb + (size_t)steps * NB * 1024;
  return pf_launch_lds(&k_stem3x_wrw<STRIDE, NB>, S, ST_THREADS, lds, st, a);
}

extern "C" int pf_conv_stem3x_wrw(const void* dY, const void* X, void* dW, int dw_dtype, float* workspace, int imgs, int H, int Wd, int N,
                                  int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream) {
  const int S = pf_conv_stem3x_wrw_slabs(imgs, H, Wd, N, stride, pad_h, pad_w, Ho, Wo);
  Stem3xWrwArgs a;
  if (S <= 0 || workspace == nullptr || dW == nullptr || !stem_fill(a, X, dY, nullptr, imgs, H, Wd, Ho, Wo, s3x_wrw_rows(Wo)))
    return (int)hipErrorInvalidValue;
  a.dY = (const bf16_t*)dY; a.slabs = workspace; a.ph = pad_h; a.pw = pad_w; a.N = N; a.tsh = s3x_tsh(Wd); a.orows = s3x_wrw_rows(Wo);
  a.dy_bytes = (int)stem_dy_bytes(imgs, Ho, Wo, N);
  hipStream_t st = (hipStream_t)stream;
  const int nb = (N + 15) / 16;
  int e;
  if (stride == 1) e = nb == 1 ? s3x_launch_wrw<1, 1>(a, S, st) : nb == 2 ? s3x_launch_wrw<1, 2>(a, S, st) : nb == 3 ? s3x_launch_wrw<1, 3>(a, S, st) : s3x_launch_wrw<1, 4>(a, S, st);
  else e = nb == 1 ? s3x_launch_wrw<2, 1>(a, S, st) : nb == 2 ? s3x_launch_wrw<2, 2>(a, S, st) : nb == 3 ? s3x_launch_wrw<2, 3>(a, S, st) : s3x_launch_wrw<2, 4>(a, S, st);
  if (e) return e;
  return pf_wrw_reduce(workspace, S, (int64_t)N * 27, dW, dw_dtype, st);
}
