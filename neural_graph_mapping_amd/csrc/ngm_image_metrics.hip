// Scoring rendered frames: PSNR, SSIM and depth L1 in fp64 (evaluation.py:20-30, 46-62; the contract is the comment above
// ngm_image_metrics in include/ngm_hip.h).  pred / target are (B, H, W, 4) fp32, r g b depth interleaved: one 16-byte load
// fetches a pixel.  Three launches, no atomics, every sum in a fixed order:
//   k_im_pixels    a fixed number of workgroups per frame strides over the frame's pixels: squared colour differences inside the
//                  cropped region, |depth difference| and its count over the whole image -> one row of 3 doubles per workgroup
//   k_im_ssim      one workgroup per tile of IM_TH x IM_TW window positions of a frame: the tile and its 5-pixel halo of both
//                  images, clamped, staged in LDS as fp32 (a clamped fp32 value is its fp64 value); per channel a horizontal
//                  11-tap pass into an LDS image of five fp64 sums, then a vertical 11-tap pass and the SSIM quotient per
//                  window -> one double per workgroup
//   k_im_finish    one workgroup per frame adds the frame's rows (thread t takes rows t, t + 256, ..., then a fixed tree) and
//                  writes the eight numbers
// The grids of a frame depend on (H, W, crop) only and a frame's rows are its own, so frame b of a batch is scored exactly as
// the same frame alone.  Nothing below may be contracted into a fused multiply-add except where fma() is written: identical
// images then give the same five sums for x and y and the quotient is exactly 1.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ngm_workspace.h"

#pragma clang fp contract(off)

#define IM_T 256                         // threads per workgroup (4 waves)
#define IM_TW 32                         // window positions per tile, x
#define IM_TH 16                         // window positions per tile, y
#define IM_K 11                          // taps
#define IM_HR (IM_TH + IM_K - 1)         // tile rows with halo: 26
#define IM_HC (IM_TW + IM_K - 1)         // tile columns with halo: 42
#define IM_PIX_BLOCKS_MAX 128            // workgroups per frame of k_im_pixels
#define IM_PIX_ROW 3                     // doubles per row of k_im_pixels: squared colour error, |depth error|, depth pixels

struct ImWeights { double g[IM_K]; };

struct ImArgs {
  const float* pred;
  const float* target;
  double* out;
  double* ssim_rows;                     // [B][tiles]
  double* pix_rows;                      // [B][pix_blocks][IM_PIX_ROW]
  int B, H, W, crop;
  int h, w;                              // the cropped region's sides (0 when empty)
  int wh, ww;                            // window positions each way (0 when the region has fewer than 11 rows or columns)
  int tiles_x, tiles_y, tiles;           // tiles of a frame
  int pix_blocks;                        // workgroups of k_im_pixels per frame
};

// torch.clamp(v, 0, 1): NaN passes through both comparisons
__device__ __forceinline__ double im_clamp01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

// sum over the workgroup in a fixed order: lanes by halving strides, then the four waves in turn; the result is valid in thread 0
__device__ __forceinline__ double im_block_sum(double v, double* wave_part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                                         // wave_part may still be read from a previous call
  if (lane == 0) wave_part[wave] = v;
  __syncthreads();
  double s = wave_part[0];
#pragma unroll
  for (int k = 1; k < IM_T / 64; ++k) s = s + wave_part[k];
  return s;
}

__global__ __launch_bounds__(IM_T) void k_im_pixels(ImArgs a) {
  __shared__ double wave_part[IM_T / 64];
  const int b = blockIdx.x / a.pix_blocks, blk = blockIdx.x % a.pix_blocks;
  const int64_t hw = (int64_t)a.H * a.W;
  const float4* __restrict__ P = reinterpret_cast<const float4*>(a.pred) + (int64_t)b * hw;
  const float4* __restrict__ T = reinterpret_cast<const float4*>(a.target) + (int64_t)b * hw;
  const int r0 = a.crop, r1 = a.crop + a.h, c0 = a.crop, c1 = a.crop + a.w;   // h, w are 0 where the region is empty
  double sq = 0.0, dl = 0.0, dn = 0.0;
  for (int64_t i = (int64_t)blk * IM_T + threadIdx.x; i < hw; i += (int64_t)a.pix_blocks * IM_T) {
    const float4 p = P[i], t = T[i];
    const int row = (int)(i / a.W), col = (int)(i % a.W);
    if (row >= r0 && row < r1 && col >= c0 && col < c1) {
      const double d0 = im_clamp01((double)p.x) - im_clamp01((double)t.x);
      const double d1 = im_clamp01((double)p.y) - im_clamp01((double)t.y);
      const double d2 = im_clamp01((double)p.z) - im_clamp01((double)t.z);
      sq = sq + ((d0 * d0 + d1 * d1) + d2 * d2);
    }
    if (t.w != 0.0f) {                                                     // NaN takes part, -0.0 does not
      dl = dl + fabs((double)p.w - (double)t.w);
      dn = dn + 1.0;
    }
  }
  sq = im_block_sum(sq, wave_part);
  dl = im_block_sum(dl, wave_part);
  dn = im_block_sum(dn, wave_part);
  if (threadIdx.x == 0) {
    double* row = a.pix_rows + ((int64_t)b * a.pix_blocks + blk) * IM_PIX_ROW;
    row[0] = sq; row[1] = dl; row[2] = dn;
  }
}

__global__ __launch_bounds__(IM_T) void k_im_ssim(ImArgs a, ImWeights wt) {
  __shared__ float sx[3][IM_HR][IM_HC];                                    // clamped pred rgb of the tile and its halo
  __shared__ float sy[3][IM_HR][IM_HC];                                    // clamped target rgb
  __shared__ double hs[5][IM_HR][IM_TW];                                   // horizontal sums of one channel: mu_x, mu_y, xx, yy, xy
  __shared__ double wave_part[IM_T / 64];
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int ty = tile / a.tiles_x, tx = tile % a.tiles_x;
  const int wy0 = ty * IM_TH, wx0 = tx * IM_TW;                             // the tile's first window, in the region's coordinates
  const int64_t hw = (int64_t)a.H * a.W;
  const float4* __restrict__ P = reinterpret_cast<const float4*>(a.pred) + (int64_t)b * hw;
  const float4* __restrict__ T = reinterpret_cast<const float4*>(a.target) + (int64_t)b * hw;

  // stage: region pixel (wy0 + r, wx0 + c) = image pixel (crop + wy0 + r, crop + wx0 + c); outside the region: 0 (only windows
  // that do not count read those)
  for (int i = threadIdx.x; i < IM_HR * IM_HC; i += IM_T) {
    const int r = i / IM_HC, c = i % IM_HC;
    const int ry = wy0 + r, rx = wx0 + c;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), t = p;
    if (ry < a.h && rx < a.w) {
      const int64_t idx = (int64_t)(a.crop + ry) * a.W + (a.crop + rx);
      p = P[idx]; t = T[idx];
    }
    sx[0][r][c] = (float)im_clamp01((double)p.x); sx[1][r][c] = (float)im_clamp01((double)p.y); sx[2][r][c] = (float)im_clamp01((double)p.z);
    sy[0][r][c] = (float)im_clamp01((double)t.x); sy[1][r][c] = (float)im_clamp01((double)t.y); sy[2][r][c] = (float)im_clamp01((double)t.z);
  }
  __syncthreads();

  const double c1 = 1e-4, c2 = 9e-4;
  double acc = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    // horizontal pass: taps left to right, sum = fma(g, value, sum) starting from 0
    for (int i = threadIdx.x; i < IM_HR * IM_TW; i += IM_T) {
      const int r = i / IM_TW, c = i % IM_TW;
      double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
      for (int k = 0; k < IM_K; ++k) {
        const double x = (double)sx[ch][r][c + k], y = (double)sy[ch][r][c + k], g = wt.g[k];
        mx = fma(g, x, mx); my = fma(g, y, my);
        xx = fma(g, x * x, xx); yy = fma(g, y * y, yy); xy = fma(g, x * y, xy);
      }
      hs[0][r][c] = mx; hs[1][r][c] = my; hs[2][r][c] = xx; hs[3][r][c] = yy; hs[4][r][c] = xy;
    }
    __syncthreads();
    // vertical pass and the quotient, windows of the tile in row-major order
    for (int i = threadIdx.x; i < IM_TH * IM_TW; i += IM_T) {
      const int r = i / IM_TW, c = i % IM_TW;
      double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
      for (int k = 0; k < IM_K; ++k) {
        const double g = wt.g[k];
        mx = fma(g, hs[0][r + k][c], mx); my = fma(g, hs[1][r + k][c], my);
        xx = fma(g, hs[2][r + k][c], xx); yy = fma(g, hs[3][r + k][c], yy); xy = fma(g, hs[4][r + k][c], xy);
      }
      double vx = xx - mx * mx, vy = yy - my * my;
      vx = vx < 0.0 ? 0.0 : vx;                                            // max(., 0) that keeps NaN
      vy = vy < 0.0 ? 0.0 : vy;
      const double vxy = xy - mx * my;
      const double s = ((2.0 * mx * my + c1) * (2.0 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2));
      if (wy0 + r < a.wh && wx0 + c < a.ww) acc = acc + s;
    }
    __syncthreads();                                                       // hs is rewritten by the next channel
  }
  acc = im_block_sum(acc, wave_part);
  if (threadIdx.x == 0) a.ssim_rows[(int64_t)b * a.tiles + tile] = acc;
}

// thread t adds rows t, t + IM_T, ... in turn; the IM_T partial sums are then added by halving strides; valid in thread 0
__device__ __forceinline__ double im_rows_sum(const double* rows, int n, int stride, double* part) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += IM_T) v = v + rows[(int64_t)i * stride];
  __syncthreads();
  part[threadIdx.x] = v;
  __syncthreads();
  for (int off = IM_T / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + off];
    __syncthreads();
  }
  return part[0];
}

__global__ __launch_bounds__(IM_T) void k_im_finish(ImArgs a) {
  __shared__ double part[IM_T];
  const int b = blockIdx.x;
  const bool pixels = a.H > 0 && a.W > 0;
  const double* pr = a.pix_rows + (int64_t)b * a.pix_blocks * IM_PIX_ROW;
  const double ss = im_rows_sum(a.ssim_rows + (int64_t)b * a.tiles, a.tiles, 1, part);
  const double sq = im_rows_sum(pr + 0, pixels ? a.pix_blocks : 0, IM_PIX_ROW, part);
  const double dl = im_rows_sum(pr + 1, pixels ? a.pix_blocks : 0, IM_PIX_ROW, part);
  const double dn = im_rows_sum(pr + 2, pixels ? a.pix_blocks : 0, IM_PIX_ROW, part);
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double terms = 3.0 * (double)a.h * (double)a.w, windows = 3.0 * (double)a.wh * (double)a.ww;
  const double mse = terms > 0.0 ? sq / terms : nan;
  double* o = a.out + (int64_t)b * 8;
  o[0] = terms > 0.0 ? 10.0 * log10(1.0 / mse) : nan;                      // mse == 0: log10(inf) = +inf
  o[1] = windows > 0.0 ? ss / windows : nan;
  o[2] = dn > 0.0 ? dl / dn : nan;
  o[3] = mse;
  o[4] = terms;
  o[5] = windows;
  o[6] = dn;
  o[7] = 0.0;
}

// ------------------------------------------------------------------------------------------------ host
static void im_shape(ImArgs& a, int B, int H, int W, int crop) {
  a.B = B; a.H = H; a.W = W; a.crop = crop;
  const int64_t h = (int64_t)H - 2 * (int64_t)crop, w = (int64_t)W - 2 * (int64_t)crop;
  const bool region = h > 0 && w > 0;
  a.h = region ? (int)h : 0;
  a.w = region ? (int)w : 0;
  const bool windows = a.h >= IM_K && a.w >= IM_K;
  a.wh = windows ? a.h - (IM_K - 1) : 0;
  a.ww = windows ? a.w - (IM_K - 1) : 0;
  a.tiles_x = (a.ww + IM_TW - 1) / IM_TW;
  a.tiles_y = (a.wh + IM_TH - 1) / IM_TH;
  a.tiles = a.tiles_x * a.tiles_y;
  const int64_t hw = (int64_t)H * W;
  a.pix_blocks = (int)(hw == 0 ? 0 : (hw + 8 * IM_T - 1) / (8 * IM_T) < IM_PIX_BLOCKS_MAX ? (hw + 8 * IM_T - 1) / (8 * IM_T) : IM_PIX_BLOCKS_MAX);
}
static void im_layout(ImArgs& a, WsArena& ws) {
  a.ssim_rows = ws.take<double>((int64_t)a.B * a.tiles);
  a.pix_rows = ws.take<double>((int64_t)a.B * a.pix_blocks * IM_PIX_ROW);
}
int64_t ngm_image_metrics_bytes(int B, int H, int W, int crop) {
  ImArgs a = {};
  im_shape(a, B, H, W, crop);
  WsArena ws;
  im_layout(a, ws);
  return ws.bytes();
}
int ngm_launch_image_metrics(const float* pred, const float* target, int B, int H, int W, int crop, double* out, void* workspace,
                             int64_t workspace_bytes, hipStream_t st) {
  ImArgs a = {};
  im_shape(a, B, H, W, crop);
  a.pred = pred; a.target = target; a.out = out;
  WsArena ws(workspace);
  im_layout(a, ws);
  if (!ws.covers(workspace_bytes)) return 1;
  if (B == 0) return 0;
  ImWeights wt;
  double sum = 0.0;
  for (int i = 0; i < IM_K; ++i) { const double d = (i - 5) / 1.5; wt.g[i] = exp(-(d * d) / 2.0); sum += wt.g[i]; }
  for (int i = 0; i < IM_K; ++i) wt.g[i] /= sum;
  if (a.pix_blocks > 0) hipLaunchKernelGGL(k_im_pixels, dim3((unsigned)((int64_t)B * a.pix_blocks)), dim3(IM_T), 0, st, a);
  if (a.tiles > 0) hipLaunchKernelGGL(k_im_ssim, dim3((unsigned)((int64_t)B * a.tiles)), dim3(IM_T), 0, st, a, wt);
  hipLaunchKernelGGL(k_im_finish, dim3((unsigned)B), dim3(IM_T), 0, st, a);
  return 0;
}
