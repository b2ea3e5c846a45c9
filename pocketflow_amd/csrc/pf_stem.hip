// The ResNet stem: 7x7 / stride 2 / pad 3 convolution of a 3-channel image to 64 channels
// (reference utils/external/resnet_model.py:478-486 initial conv2d_fixed_padding), NHWC bf16 -> NHWC bf16.
//
// Why its own kernel.  With C = 3 the implicit-GEMM kernel's "k = (tap, 64 channels)" tiling does not apply, and MIOpen
// spends 384 us on the 256 x 224 x 224 launch (77 MB in, 411 MB out: HBM floor ~80 us).  Layout of the problem on CDNA4:
//   * a workgroup owns one image and a strip of 8 output rows; the 21 input rows it needs are staged ONCE into LDS with
//     every pixel padded from 3 to 4 channels (8 bytes), 3 zero pixels left of the row and >= 5 right of it.  Then the
//     eight k-values a lane feeds to v_mfma_f32_16x16x32_bf16 -- taps (s, s+1) x 4 channels of kernel row r -- are ONE
//     aligned 16-byte LDS read at  row(2*oy + r) + (2*ox + s) * 8 B:  k' = r*32 + s*4 + c, 7 k-steps of 32 with the
//     weights of s = 7 and of c = 3 being zero (147 real of 224 k-values: 34 % padding, bought for conflict-free,
//     division-free, shuffle-free operand fetch);
//   * weights are operand A (rows = output channels), packed once per workgroup into the same k' order and kept in
//     REGISTERS for the whole launch (4 channel blocks x 7 k-steps x 4 VGPRs); the MFMA row -> channel map is chosen
//     such that a lane ends up with 16 CONSECUTIVE channels of its pixel: two 16-byte stores, no LDS transposition;
//   * persistent workgroups (2 per CU) loop over (image, strip) items, so the weight packing is paid once.
#include "pf_stem.h"

#define ST_OROWS 8                      // output rows per item
#define ST_IROWS (2 * ST_OROWS + 5)     // input rows staged per item
#define ST_N 64
#define ST_R 7
#define ST_WL_BYTES (ST_N * ST_R * 32 * 2)

__global__ __launch_bounds__(ST_THREADS) void k_stem7x7_fwd(StemArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* wl = smem;                               // packed weights [64][7][32] bf16
  unsigned char* xs = smem + ST_WL_BYTES;                 // staged rows [21][(Wd + 8)][4] bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, g = lane >> 4;

  // ---- pack the weights: chunk (n, r, q) = taps (2q, 2q+1) x 4 channels of kernel row r of output channel n ----
  for (int ch = tid; ch < ST_N * ST_R * 4; ch += ST_THREADS) {
    const int q = ch & 3, nr = ch >> 2;                   // nr = n*7 + r
    const bf16_t* src = a.W + ((int64_t)nr * 7 + 2 * q) * 3;
    uint32_t v[4];
    const uint32_t e0 = src[0], e1 = src[1], e2 = src[2];
    v[0] = e0 | (e1 << 16); v[1] = e2;
    if (q < 3) {
      const uint32_t f0 = src[3], f1 = src[4], f2 = src[5];
      v[2] = f0 | (f1 << 16); v[3] = f2;
    } else {
      v[2] = 0u; v[3] = 0u;                               // tap s = 7 does not exist
    }
    *reinterpret_cast<uint4*>(wl + ((int64_t)nr * 32 + q * 8) * 2) = make_uint4(v[0], v[1], v[2], v[3]);
  }
  // ---- zero the halo pixels of every staged row once (columns 0..2 and Wd+3..Wd+7 are never written again) ----
  for (int t = tid; t < ST_IROWS * 8; t += ST_THREADS) {
    const int row = t >> 3, h = t & 7;
    const int pp = h < 3 ? h : a.Wd + h;                  // 0,1,2, Wd+3 .. Wd+7
    *reinterpret_cast<uint2*>(xs + (int64_t)row * a.rsb + pp * 8) = make_uint2(0u, 0u);
  }
  __syncthreads();
  // ---- A fragments: MFMA row i of channel block nb is output channel 16*(i/4) + 4*nb + (i%4) ----
  bf16x8 wf[4][ST_R];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int n = 16 * (l16 >> 2) + 4 * nb + (l16 & 3);
#pragma unroll
    for (int r = 0; r < ST_R; ++r)
      wf[nb][r] = *reinterpret_cast<const bf16x8*>(wl + ((n * ST_R + r) * 32 + g * 8) * 2);
  }

  const int pairs = a.Wd >> 1;                            // two pixels (12 bytes) per staging task
  const int pblocks = a.Wo >> 4;                          // 16-pixel blocks per output row
  const int units = ST_OROWS * pblocks;
  for (int item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    const int img = item / a.strips, strip = item - img * a.strips;
    const int oy0 = strip * ST_OROWS, iy0 = 2 * oy0 - 3;
    __syncthreads();                                      // the previous item's fragment reads are done
    // ---- stage 21 input rows, 3 -> 4 channels ----
    for (int row = tid >> 7; row < ST_IROWS; row += 2) {     // (the first real pixel sits 24 bytes into the row: 8-byte stores)
      const int iy = iy0 + row;
      const bool live = iy >= 0 && iy < a.H;
      stem_stage_row(xs + (int64_t)row * a.rsb + 3 * 8, a.X + ((int64_t)img * a.H + (live ? iy : 0)) * a.Wd * 3, live, pairs, tid & 127, 128);
    }
    __syncthreads();
    // ---- 16-pixel x 64-channel units ----
    for (int u = wave; u < units; u += ST_THREADS / 64) {
      const int orow = u / pblocks, pb = u - orow * pblocks;
      const int oy = oy0 + orow;
      if (oy >= a.Ho) continue;
      const int ox = pb * 16 + l16;
      const unsigned char* base = xs + (int64_t)(2 * orow) * a.rsb + (2 * ox + 2 * g) * 8;
      f32x4 acc[4];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < ST_R; ++r) {
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(base + (int64_t)r * a.rsb);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb][r], xf, acc[nb], 0, 0, 0);
      }
      // lane: pixel ox, channels 16g + 4nb + j
      bf16_t* out = a.Y + (((int64_t)img * a.Ho + oy) * a.Wo + ox) * ST_N + 16 * g;
      const uint4 lo = make_uint4(pack_bf16x2(acc[0][0], acc[0][1]), pack_bf16x2(acc[0][2], acc[0][3]),
                                  pack_bf16x2(acc[1][0], acc[1][1]), pack_bf16x2(acc[1][2], acc[1][3]));
      const uint4 hi = make_uint4(pack_bf16x2(acc[2][0], acc[2][1]), pack_bf16x2(acc[2][2], acc[2][3]),
                                  pack_bf16x2(acc[3][0], acc[3][1]), pack_bf16x2(acc[3][2], acc[3][3]));
      *reinterpret_cast<uint4*>(out) = lo;
      *reinterpret_cast<uint4*>(out + 8) = hi;
    }
  }
}

// 1 when pf_conv_stem_fwd takes the shape (anything else stays with the caller's generic path)
extern "C" int pf_conv_stem_supported(int H, int Wd, int C, int N, int k, int stride, int pad) {
  return (C == 3 && N == ST_N && k == 7 && stride == 2 && pad == 3 && H > 0 && (H % 2) == 0 && Wd >= 32 && (Wd % 32) == 0 &&
          Wd <= 1024) ? 1 : 0;
}

extern "C" int pf_conv_stem_fwd(const void* X, const void* W, void* Y, int imgs, int H, int Wd, void* stream) {
  StemArgs a;
  if (!pf_conv_stem_supported(H, Wd, 3, ST_N, 7, 2, 3) || imgs <= 0 || !stem_fill(a, X, Y, W, imgs, H, Wd, H / 2, Wd / 2, ST_OROWS))
    return (int)hipErrorInvalidValue;
  a.W = (const bf16_t*)W; a.Y = (bf16_t*)Y;
  const size_t lds = (size_t)ST_WL_BYTES + (size_t)ST_IROWS * a.rsb;
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  return pf_launch_lds(&k_stem7x7_fwd, stem_grid(a.n_items, 512), ST_THREADS, lds, (hipStream_t)stream, a);
}


// =================================================================================================================
// Backward-filter of the stem:  dW[n][r][s][c] = sum over (img, oy, ox) of dY[img][oy][ox][n] * X[img][2oy+r-3][2ox+s-3][c]
// (Conv2DBackpropFilter of the same convolution).  Both operands are pixel-major in memory and the contraction runs over
// pixels, so both MFMA operands are fetched with the transposing LDS read ds_read_b64_tr_b16 (a lane supplies the address
// of a 4-element piece and receives a column):
//   * dY^T: two output rows of one image (2*Wo consecutive pixels) go to LDS by LDS-DMA in [8 pixels][16 channels]
//     blocks of 256 B, exactly the layout of k_wrw2 (pf_wrw.hip);
//   * X: the 9 input rows of the strip are staged as in the forward kernel (pixels padded to 4 channels).  A piece of
//     the transposed read -- 4 consecutive k' = (tap s, channels 0..3) of one pixel -- is then ONE padded pixel, 8 bytes
//     at row(2*oy + r) + (2*ox + s) * 8: overlapping windows of neighbouring output pixels cost nothing, every lane
//     supplies its own address.
// k' = r*32 + s*4 + c as in the forward kernel (14 blocks of 16; s = 7 and c = 3 are padding and are never written).
// Wavefront w: channel blocks {2(w&1), 2(w&1)+1} x kernel rows {0..3} (w < 2) or {4..6}; accumulators stay in registers
// over all (image, strip) items of the persistent workgroup; one fp32 slab [64][147] per workgroup, summed in a fixed
// order by pf_wrw_reduce (deterministic).
// =================================================================================================================
#define SW_OROWS 2
#define SW_IROWS (2 * SW_OROWS + 5)

__global__ __launch_bounds__(ST_THREADS) void k_stem7x7_wrw(StemWrwArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* xs = smem;                                 // staged input rows [9][(Wd + 8)][4] bf16
  unsigned char* dys = smem + SW_IROWS * a.rsb;             // dY blocks [steps][4 pixel groups][4 channel blocks][8][16] bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int nb0 = 2 * (wave & 1);                           // this wavefront's two 16-channel blocks
  const int r0 = (wave >> 1) ? 4 : 0, nr = (wave >> 1) ? 3 : 4;   // and its kernel rows
  const pf_rsrc_t rsY = PF_MAKE_RSRC(a.dY, a.dy_bytes);
  constexpr uint32_t OOB = 0x80000000u;
  const int sb = lane >> 4, srow = (lane & 15) >> 1, sch = lane & 1;        // role inside one LDS-DMA instruction
  const int tr_off = (q & 1) * 128 + (l15 >> 2) * 32 + (l15 & 3) * 8;       // piece of the transposed read (k_wrw2)
  const int pg_lo = q >> 1;
  const int p_lo = 8 * pg_lo + 4 * (q & 1) + (l15 >> 2);                    // the pixel (within a 32-pixel step) whose X piece this lane addresses
  const int steps = (SW_OROWS * a.Wo) >> 5;
  const int pairs = a.Wd >> 1;

  f32x4 acc[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[i][k] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = tid; t < SW_IROWS * 8; t += ST_THREADS) {    // halo pixels, once
    const int row = t >> 3, h = t & 7;
    const int pp = h < 3 ? h : a.Wd + h;
    *reinterpret_cast<uint2*>(xs + (int64_t)row * a.rsb + pp * 8) = make_uint2(0u, 0u);
  }

  for (int item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    const int img = item / a.strips, strip = item - img * a.strips;
    const int oy0 = strip * SW_OROWS, iy0 = 2 * oy0 - 3;
    const int valid_px = ((a.Ho - oy0) < SW_OROWS ? (a.Ho - oy0) : SW_OROWS) * a.Wo;
    const int64_t m_base = ((int64_t)img * a.Ho + oy0) * a.Wo;
    __syncthreads();                                        // the previous item's reads are done
    // ---- dY: steps x 4 pixel groups, one LDS-DMA instruction (1 KB) each ----
    for (int id = wave; id < steps * 4; id += ST_THREADS / 64) {
      const int lin = id * 8 + srow;                        // id = step*4 + pg
      const uint32_t voff = (lin < valid_px) ? (uint32_t)(((m_base + lin) * ST_N + 16 * sb + 8 * sch) * 2) : OOB;
      PF_BUFFER_LOAD_LDS16(rsY, dys + id * 1024, voff, 0);
    }
    // ---- X: 9 input rows, 3 -> 4 channels ----
    for (int row = tid >> 7; row < SW_IROWS; row += 2) {
      const int iy = iy0 + row;
      const bool live = iy >= 0 && iy < a.H;
      stem_stage_row(xs + (int64_t)row * a.rsb + 3 * 8, a.X + ((int64_t)img * a.H + (live ? iy : 0)) * a.Wd * 3, live, pairs, tid & 127, 128);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // ---- 32 pixels per step ----
    for (int st = 0; st < steps; ++st) {
      const unsigned char* dbase = dys + st * 4096;
      bf16x8 df[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const pf_v4s lo = pf_tr_read(dbase + (pg_lo * 4 + nb0 + i) * 256 + tr_off);
        const pf_v4s hi = pf_tr_read(dbase + ((pg_lo + 2) * 4 + nb0 + i) * 256 + tr_off);
        df[i] = pf_join(lo, hi);
      }
      // this lane's two X pixels of the step: lin -> (output row of the strip, ox)
      int lin = st * 32 + p_lo;
      int orow = lin >= a.Wo ? 1 : 0;
      const unsigned char* xlo = xs + (int64_t)(2 * orow + r0) * a.rsb + (2 * (lin - orow * a.Wo) + (l15 & 3)) * 8;
      lin += 16;
      orow = lin >= a.Wo ? 1 : 0;
      const unsigned char* xhi = xs + (int64_t)(2 * orow + r0) * a.rsb + (2 * (lin - orow * a.Wo) + (l15 & 3)) * 8;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        if (rr < nr) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const pf_v4s lo = pf_tr_read(xlo + (int64_t)rr * a.rsb + h * 32);
            const pf_v4s hi = pf_tr_read(xhi + (int64_t)rr * a.rsb + h * 32);
            const bf16x8 xf = pf_join(lo, hi);
#pragma unroll
            for (int i = 0; i < 2; ++i)
              acc[i][rr * 2 + h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[i], xf, acc[i][rr * 2 + h], 0, 0, 0);
          }
        }
      }
    }
  }
  // ---- slab [64][7][7][3]: lane (q, l15) holds rows n = 16*nb + 4q + j, column k' = (r, s = 4h + l15/4, c = l15%4) ----
  float* slab = a.slabs + (int64_t)blockIdx.x * (ST_N * 147);
  const int c = l15 & 3;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    if (rr < nr) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int s = 4 * h + (l15 >> 2);
        if (s < 7 && c < 3) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              slab[(16 * (nb0 + i) + 4 * q + j) * 147 + ((r0 + rr) * 7 + s) * 3 + c] = acc[i][rr * 2 + h][j];
        }
      }
    }
  }
}

// number of fp32 slabs pf_conv_stem_wrw writes, one per workgroup, for pf_wrw_reduce and its workspace contract (0: unsupported)
extern "C" int pf_conv_stem_wrw_slabs(int imgs, int H, int Wd) {
  if (!pf_conv_stem_supported(H, Wd, 3, ST_N, 7, 2, 3) || imgs <= 0 || Wd > 256 || !stem_dy_fits(imgs, H / 2, Wd / 2, ST_N)) return 0;
  return stem_grid(imgs * stem_strips(H / 2, SW_OROWS), 768);
}

extern "C" int pf_conv_stem_wrw(const void* dY, const void* X, void* dW, int dw_dtype, float* workspace, int imgs, int H,
                                int Wd, void* stream) {
  const int S = pf_conv_stem_wrw_slabs(imgs, H, Wd);
  StemWrwArgs a;
  if (S <= 0 || workspace == nullptr || !stem_fill(a, X, dY, nullptr, imgs, H, Wd, H / 2, Wd / 2, SW_OROWS)) return (int)hipErrorInvalidValue;
  a.dY = (const bf16_t*)dY; a.slabs = workspace;
  a.dy_bytes = (int)stem_dy_bytes(imgs, a.Ho, a.Wo, ST_N);
  const size_t lds = (size_t)SW_IROWS * a.rsb + (size_t)SW_OROWS * a.Wo * ST_N * 2;
  if (int e = pf_launch_lds(&k_stem7x7_wrw, S, ST_THREADS, lds, (hipStream_t)stream, a)) return e;
  return pf_wrw_reduce(workspace, S, (int64_t)ST_N * 147, dW, dw_dtype, (hipStream_t)stream);
}
