// SSIM as a training loss on gfx950 (G_lossfn_type 'ssim', the restated models/loss_ssim.py: kair_amd/models/
// model_plain.py SSIMLoss): mean over B, C, H, W of
//   S = (2 m1 m2 + C1)(2 s12 + C2) / ((m1^2 + m2^2 + C1)(s11 + s22 + C2)),
// the moments being depthwise 11x11 Gaussian (sigma 1.5) filterings with zero padding 5, and its analytic gradient.
// With a = dS/dm1, b = dS/dm11, c = dS/dm12 per pixel (the five filtered maps taken as independent; the window is
// symmetric and the padding zero, so the adjoint of the filter is the filter):
//   dL/dE(p) = weight / numel * [ (w*a)(p) + 2 E(p) (w*b)(p) + H(p) (w*c)(p) ].
//
// Two launches over 32 x 32 tiles of one image plane + a one-workgroup sum:
//   stats:  E and H tiles with a 5-pixel halo in LDS (42 x 42, zero outside the image) -> rows pass (11 taps, 42 rows
//           x 32 columns of the five maps) -> columns pass (each thread 4 consecutive rows of one column: 14 LDS reads
//           per map for 4 outputs) -> a, b, c planes to the workspace, the tile's sum of S to its own slot;
//   grad:   the same tile of a, b, c with the halo -> the two passes on three maps -> combined with E(p), H(p) and
//           stored in the caller's gradient layout; one workgroup walks the C channels of its tile, so the stores to
//           one row of channel slots come from one workgroup;
//   final:  the per-tile sums added in a fixed order (no float atomics: eager, graph replay and repeated calls are
//           bit-identical).
// LDS: both passes index consecutive lanes to consecutive columns (32 lanes = one tile row), so every ds_read_b32 /
// ds_write_b32 half-wave covers 32 consecutive dwords whatever the row stride: no bank conflicts.  fp32 accumulation.
#include "common.h"

namespace {

constexpr int TS = 32, HALO = 5, TW = TS + 2 * HALO;   // interior tile, halo, staged width
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

// exp(-x^2 / (2 * 1.5^2)), x = -5 .. 5, normalised to sum 1 in double (utils_image._gauss_window's 1-D factor),
// rounded to fp32
#define KAIR_SSIM_TAPS                                                                                         \
  {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055428e-01f, 2.660117149e-01f, \
   2.130055428e-01f, 1.093606874e-01f, 3.600077331e-02f, 7.598758209e-03f, 1.028380124e-03f}

// stage the (TW x TW) halo tile of one plane, zero outside the image
KAIR_DEV void stage_tile(const float* __restrict__ src, float* __restrict__ dst, int y0, int x0, int Hh, int Ww) {
  for (int i = threadIdx.x; i < TW * TW; i += 256) {
    const int r = i / TW, c = i - r * TW;
    const int y = y0 + r - HALO, x = x0 + c - HALO;
    dst[i] = (y >= 0 && y < Hh && x >= 0 && x < Ww) ? src[(long)y * Ww + x] : 0.f;
  }
}

// columns pass: 4 consecutive output rows (4 yg .. 4 yg + 3) of column tx from the rows-pass map hm [TW][TS]
KAIR_DEV void col_pass4(const float* __restrict__ hm, int tx, int yg, float out[4]) {
  constexpr float g[11] = KAIR_SSIM_TAPS;
  float v[14];
#pragma unroll
  for (int j = 0; j < 14; ++j) v[j] = hm[(4 * yg + j) * TS + tx];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) s = fmaf(g[k], v[j + k], s);
    out[j] = s;
  }
}

KAIR_DEV float block_sum256(float s, float* red) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// grid (tiles x, tiles y, B * C).  abc: three planes sets [3][B * C][Hh][Ww]; part: one slot per workgroup
__global__ __launch_bounds__(256) void ssim_stats_kernel(const float* __restrict__ E, const float* __restrict__ H,
                                                         float* __restrict__ abc, long N, float* __restrict__ part,
                                                         int Hh, int Ww) {
  __shared__ float sE[TW * TW], sH[TW * TW];
  __shared__ float hm[5][TW * TS];
  __shared__ float red[256];
  constexpr float g[11] = KAIR_SSIM_TAPS;
  const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
  const long base = (long)blockIdx.z * Hh * Ww;
  stage_tile(E + base, sE, y0, x0, Hh, Ww);
  stage_tile(H + base, sH, y0, x0, Hh, Ww);
  __syncthreads();
  for (int i = threadIdx.x; i < TW * TS; i += 256) {
    const int r = i / TS, x = i - r * TS;
    float m1 = 0.f, m2 = 0.f, m11 = 0.f, m22 = 0.f, m12 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float e = sE[r * TW + x + k], h = sH[r * TW + x + k];
      const float ge = g[k] * e, gh = g[k] * h;
      m1 += ge;
      m2 += gh;
      m11 = fmaf(ge, e, m11);
      m22 = fmaf(gh, h, m22);
      m12 = fmaf(ge, h, m12);
    }
    hm[0][i] = m1, hm[1][i] = m2, hm[2][i] = m11, hm[3][i] = m22, hm[4][i] = m12;
  }
  __syncthreads();
  const int tx = threadIdx.x & 31, yg = threadIdx.x >> 5;
  float m[5][4];
#pragma unroll
  for (int q = 0; q < 5; ++q) col_pass4(hm[q], tx, yg, m[q]);
  float ssum = 0.f;
  const int x = x0 + tx;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = y0 + 4 * yg + j;
    if (y < Hh && x < Ww) {
      const float m1 = m[0][j], m2 = m[1][j];
      const float s11 = m[2][j] - m1 * m1, s22 = m[3][j] - m2 * m2, s12 = m[4][j] - m1 * m2;
      const float A1 = 2.f * m1 * m2 + SSIM_C1, A2 = 2.f * s12 + SSIM_C2;
      const float B1 = m1 * m1 + m2 * m2 + SSIM_C1, B2 = s11 + s22 + SSIM_C2;
      const float rB1 = 1.f / B1, rB2 = 1.f / B2, rB = rB1 * rB2;
      const float S = A1 * A2 * rB;
      ssum += S;
      const long o = base + (long)y * Ww + x;
      abc[o] = 2.f * m2 * (A2 - A1) * rB - 2.f * m1 * S * (rB1 - rB2);   // dS/dm1
      abc[N + o] = -S * rB2;                                              // dS/dm11
      abc[2 * N + o] = 2.f * A1 * rB;                                     // dS/dm12
    }
  }
  const float t = block_sum256(ssum, red);
  if (threadIdx.x == 0) part[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
}

// grid (tiles x, tiles y, B).  NCHW: dE is the fp32 image gradient [B][C][Hh][Ww]; else rows of ldc slots per pixel
// of the [Hh / r, Ww / r] grid, slot = c r^2 + (y % r) r + x % r, slots >= C r^2 zero (kair_l1_loss's layout)
template <typename T, bool NCHW>
__global__ __launch_bounds__(256) void ssim_grad_kernel(const float* __restrict__ E, const float* __restrict__ H,
                                                        const float* __restrict__ abc, long N, T* __restrict__ dE,
                                                        int ldc, int r, float gscale, int C, int Hh, int Ww) {
  __shared__ float sP[3][TW * TW];
  __shared__ float hm[3][TW * TS];
  constexpr float g[11] = KAIR_SSIM_TAPS;
  const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS, b = blockIdx.z;
  const int tx = threadIdx.x & 31, yg = threadIdx.x >> 5;
  const int x = x0 + tx;
  const int hs = Hh / r, wsm = Ww / r, r2 = r * r;
  for (int c = 0; c < C; ++c) {
    const long base = ((long)b * C + c) * Hh * Ww;
#pragma unroll
    for (int q = 0; q < 3; ++q) stage_tile(abc + q * N + base, sP[q], y0, x0, Hh, Ww);
    __syncthreads();
    for (int i = threadIdx.x; i < TW * TS; i += 256) {
      const int rr = i / TS, xx = i - rr * TS;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        s0 = fmaf(g[k], sP[0][rr * TW + xx + k], s0);
        s1 = fmaf(g[k], sP[1][rr * TW + xx + k], s1);
        s2 = fmaf(g[k], sP[2][rr * TW + xx + k], s2);
      }
      hm[0][i] = s0, hm[1][i] = s1, hm[2][i] = s2;
    }
    __syncthreads();
    float w[3][4];
#pragma unroll
    for (int q = 0; q < 3; ++q) col_pass4(hm[q], tx, yg, w[q]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int y = y0 + 4 * yg + j;
      if (y < Hh && x < Ww) {
        const long o = base + (long)y * Ww + x;
        const float gv = gscale * (w[0][j] + 2.f * E[o] * w[1][j] + H[o] * w[2][j]);
        if constexpr (NCHW) {
          dE[o] = (T)gv;
        } else {
          const int gy = y / r, gx = x / r;
          const long pix = ((long)b * hs + gy) * wsm + gx;
          dE[pix * ldc + c * r2 + (y - gy * r) * r + (x - gx * r)] = (T)gv;
        }
      }
    }
    __syncthreads();   // (the next channel restages sP and rewrites hm)
  }
  if constexpr (!NCHW) {
    // the pad slots of each grid pixel, by the thread that holds its (y % r, x % r) = (0, 0) image pixel
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int y = y0 + 4 * yg + j;
      if (y < Hh && x < Ww && y % r == 0 && x % r == 0) {
        const long pix = ((long)b * hs + y / r) * wsm + x / r;
        for (int s = C * r2; s < ldc; ++s) dE[pix * ldc + s] = (T)0.f;
      }
    }
  }
}

__global__ void ssim_final_kernel(const float* __restrict__ part, long n, float scale, float* __restrict__ out) {
  __shared__ float red[256];
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) s += part[i];
  const float t = block_sum256(s, red);
  if (threadIdx.x == 0) out[0] = t * scale;
}

inline long tiles(int n) { return (n + TS - 1) / TS; }

// layout: 0 = rows (dtype, ldc, ps_r), 1 = NCHW fp32
int ssim_loss(const float* E, const float* H, float* loss_out, void* dE, int layout, int dtype, int ldc, int ps_r,
              float weight, int B, int C, int Hh, int Ww, void* workspace, void* stream) {
  KAIR_CHECK_ARG(E && H && loss_out && dE && workspace, "ssim_loss: null pointer");
  KAIR_CHECK_ARG(B > 0 && C > 0 && Hh > 0 && Ww > 0, "ssim_loss: empty image");
  KAIR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ssim_loss: workspace must be 16-byte aligned");
  KAIR_CHECK_ARG((long)Hh * Ww < (1L << 31) && (long)B * C <= 65535 && tiles(Hh) <= 65535,
                 "ssim_loss: image too large (plane < 2^31 pixels, B * C <= 65535, H <= 65535 * 32)");
  if (layout == 0) {
    KAIR_CHECK_ARG(dtype == KAIR_F32 || dtype == KAIR_BF16, "ssim_loss: gradient rows are fp32 or bf16");
    KAIR_CHECK_ARG(ps_r >= 1 && Hh % ps_r == 0 && Ww % ps_r == 0, "ssim_loss: image not divisible by ps_r");
    KAIR_CHECK_ARG((long)C * ps_r * ps_r <= ldc, "ssim_loss: C * ps_r^2 slots exceed ldc");
  }
  const long N = (long)B * C * Hh * Ww;
  const long nwg = (long)B * C * tiles(Hh) * tiles(Ww);
  float* abc = (float*)workspace;
  float* part = abc + 3 * N;
  hipStream_t s = (hipStream_t)stream;
  const float gs = (float)((double)weight / (double)N);
  const dim3 tg((unsigned)tiles(Ww), (unsigned)tiles(Hh), 1);
  KAIR_LAUNCH(ssim_stats_kernel, dim3(tg.x, tg.y, (unsigned)(B * C)), dim3(256), 0, s, E, H, abc, N, part, Hh, Ww);
  KAIR_CHECK_LAUNCH();
  const dim3 gg(tg.x, tg.y, (unsigned)B);
  if (layout == 1)
    KAIR_LAUNCH((ssim_grad_kernel<float, true>), gg, dim3(256), 0, s, E, H, abc, N, (float*)dE, 0, 1, gs, C, Hh, Ww);
  else if (dtype == KAIR_BF16)
    KAIR_LAUNCH((ssim_grad_kernel<bf16, false>), gg, dim3(256), 0, s, E, H, abc, N, (bf16*)dE, ldc, ps_r, gs, C, Hh, Ww);
  else
    KAIR_LAUNCH((ssim_grad_kernel<float, false>), gg, dim3(256), 0, s, E, H, abc, N, (float*)dE, ldc, ps_r, gs, C, Hh, Ww);
  KAIR_CHECK_LAUNCH();
  KAIR_LAUNCH(ssim_final_kernel, dim3(1), dim3(256), 0, s, part, nwg, gs, loss_out);
  KAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" long kair_ssim_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const long N = (long)B * C * H * W, nwg = (long)B * C * tiles(H) * tiles(W);
  return (4 * (3 * N + nwg) + 15) / 16 * 16;
}

extern "C" int kair_ssim_loss(const float* E, const float* H, float* loss_out, void* dE, int dtype, int ldc, int ps_r,
                              float weight, int B, int C, int Hh, int Ww, void* workspace, void* stream) {
  return ssim_loss(E, H, loss_out, dE, 0, dtype, ldc, ps_r, weight, B, C, Hh, Ww, workspace, stream);
}

extern "C" int kair_ssim_loss_nchw(const float* E, const float* H, float* loss_out, float* dE, float weight, int B, int C,
                                   int Hh, int Ww, void* workspace, void* stream) {
  return ssim_loss(E, H, loss_out, dE, 1, KAIR_F32, 0, 1, weight, B, C, Hh, Ww, workspace, stream);
}
