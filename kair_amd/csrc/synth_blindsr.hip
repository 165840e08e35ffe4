// Blind-SR (BSRGAN) training data on the MI355X: the per-sample degradation program of utils/utils_blindsr.py
// (draw_bsrgan / apply_op) for a whole batch.  Every sample has its own op order, its own image size at every step
// and its own blur kernel size, so a batch lives in a padded buffer [B][3][Hmax][Wmax] (row stride Wmax) of which
// sample b uses the top-left (h, w) corner, and a step ("slot") of the program is one launch that reads a row
// {op, h_in, w_in, h_out, w_out, i0, i1, quality, 8 floats} per sample and writes the other ping-pong buffer.
//
//   kair_bsr_crop     pool -> buffer: the PS^2 crop at (rnd_h, rnd_w), 8-way augment.
//   kair_bsr_kernels  the Gaussian kernels of every blur / blur + decimate row of the table, fp64 formula.
//   kair_bsr_ops      one slot: copy, blur (mirror boundary), resize (bilinear, bicubic a = -0.75, area, MATLAB
//                     bicubic x1/2), blur + decimate, noise (per channel, gray, correlated); a JPEG row is a copy here.
//   kair_bsr_finish   buffer -> L (the lq^2 crop) and pool -> H (the aligned lq sf crop of the augmented patch).
// The JPEG rows run on kair_jpeg_roundtrip_var (synth_jpeg.hip, beside the codec it shares).
//
// kair_bsr_ops: a workgroup owns one 16 x 64 tile of one sample's output, so the op switch is uniform per workgroup;
// tiles past the sample's (h_out, w_out) exit.  A thread computes 4 rows of one column, all three channels.
// Blur: out[i][j] = sum_{u, v} k[u][v] in[mirror(i + ks/2 - u)][mirror(j + ks/2 - v)] (scipy.ndimage.convolve,
// mode='mirror': the reflection that does not repeat the edge sample; the index folds as often as it takes), one fp32
// fmaf chain over (u, v) in row-major order.  The taps and the tile with its mirror-extended halo, (16 + ks - 1) x
// (64 + ks - 1) for the sample's own ks <= 25, are staged in 16.6 KB of static LDS per channel; lanes read consecutive
// words.  A larger ks does not fit and takes the one-thread-per-output loop over global memory, as blur + decimate
// always does (its input tile at sf 4 would be 94 KB); same chain, same bits.  Every output is clipped to [0, 1].
// Sizes and indices read from the table are clamped into the buffer, so a bad table cannot make an access leave it.
#include "synth_common.h"

namespace {

enum { BSR_COPY = 0, BSR_BLUR = 1, BSR_RESIZE = 2, BSR_BLURDEC = 3, BSR_NOISE = 4, BSR_JPEG = 5 };
enum { BSR_BILINEAR = 1, BSR_BICUBIC = 2, BSR_AREA = 3, BSR_MATLAB_HALF = 4 };
constexpr int BSR_TR = 16, BSR_TC = 64, BSR_KLDS = 25;
constexpr int BSR_LW = BSR_TC + BSR_KLDS - 1, BSR_LH = BSR_TR + BSR_KLDS - 1;

struct BsrArgs {
  const float* src;
  float* dst;
  int B, Hmax, Wmax, tiles_x;
  const int* tab;
  int tstride;
  const float* k;   // [B][kstride]
  long kstride;
  int kmax;         // largest ks with ks^2 <= kstride
  const int *ih, *iw;   // MATLAB x1/2 taps of an (mh_in, mw_in) image: [ceil(mh_in / 2)][P], [ceil(mw_in / 2)][P]
  const float *wh, *ww;
  int P, mh_in, mw_in;
  unsigned long long seed, stepkey;
  int direct;
};

KAIR_DEV int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
KAIR_DEV float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

KAIR_DEV int mirror(int x, int n) {
  if (n <= 1) return 0;
  const int p = 2 * n - 2;
  int m = x % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

KAIR_DEV double keys(double d) {
  constexpr double a = -0.75;
  d = fabs(d);
  if (d <= 1.0) return ((a + 2.0) * d - (a + 3.0)) * d * d + 1.0;
  if (d < 2.0) return ((a * d - 5.0 * a) * d + 8.0 * a) * d - 4.0 * a;
  return 0.0;
}

// one axis of a resize at output index i: n taps, tap k = (source index, weight); coordinates in fp64
struct Axis {
  int kind, n_in, i, x0, n, P;
  double s, lo, hi, f;
  const int* ti;
  const float* tw;
};

KAIR_DEV Axis axis_init(int kind, int n_in, int n_out, int i, const int* ti, const float* tw, int P) {
  Axis A{};
  A.kind = kind; A.n_in = n_in; A.i = i; A.ti = ti; A.tw = tw; A.P = P;
  A.s = (double)n_in / (double)n_out;
  if (kind == BSR_AREA) {
    A.lo = i * A.s;
    A.hi = (i + 1) * A.s;
    A.x0 = (int)floor(A.lo);
    A.n = max(min((int)ceil(A.hi), n_in) - A.x0, 0);
  } else if (kind == BSR_MATLAB_HALF) {
    A.n = P;
  } else {
    const double x = (i + 0.5) * A.s - 0.5;
    const double fl = floor(x);
    A.x0 = (int)fl;
    A.f = x - fl;
    A.n = kind == BSR_BILINEAR ? 2 : 4;
  }
  return A;
}

KAIR_DEV void axis_tap(const Axis& A, int k, int& idx, float& w) {
  if (A.kind == BSR_AREA) {
    const int y = A.x0 + k;
    const double ov = fmin(A.hi, y + 1.0) - fmax(A.lo, (double)y);
    idx = clampi(y, 0, A.n_in - 1);
    w = ov > 0.0 ? (float)(ov / A.s) : 0.f;
  } else if (A.kind == BSR_MATLAB_HALF) {
    idx = clampi(A.ti[(long)A.i * A.P + k], 0, A.n_in - 1);
    w = A.tw[(long)A.i * A.P + k];
  } else if (A.kind == BSR_BILINEAR) {
    idx = clampi(A.x0 + k, 0, A.n_in - 1);
    w = (float)(k ? A.f : 1.0 - A.f);
  } else {
    idx = clampi(A.x0 - 1 + k, 0, A.n_in - 1);
    w = (float)keys(A.f + 1.0 - k);
  }
}

__global__ __launch_bounds__(256) void bsr_ops_kernel(const BsrArgs a) {
  __shared__ float sK[BSR_KLDS * BSR_KLDS];
  __shared__ float sT[BSR_LH * BSR_LW];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, rg = tid >> 6;
  const int* row = a.tab + (long)b * a.tstride;
  const int op = row[0];
  const int h_in = clampi(row[1], 1, a.Hmax), w_in = clampi(row[2], 1, a.Wmax);
  const int h_out = clampi(row[3], 1, a.Hmax), w_out = clampi(row[4], 1, a.Wmax);
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int i0 = ty * BSR_TR, j0 = tx * BSR_TC;
  if (i0 >= h_out || j0 >= w_out) return;   // uniform per workgroup
  const long plane = (long)a.Hmax * a.Wmax;
  const float* sp = a.src + (long)b * 3 * plane;
  float* dp = a.dst + (long)b * 3 * plane;
  const int j = j0 + lane, ib = i0 + rg * 4;
  const float* fr = reinterpret_cast<const float*>(row + 8);

  if (op == BSR_BLUR || op == BSR_BLURDEC) {
    const int ks = clampi(row[5], 1, a.kmax);
    const int st = op == BSR_BLURDEC ? clampi(row[6], 1, 64) : 1;
    const float* kb = a.k + (long)b * a.kstride;
    const int c0 = ks / 2;
    if (op == BSR_BLUR && ks <= BSR_KLDS && !a.direct) {
      for (int t = tid; t < ks * ks; t += 256) sK[t] = kb[t];
      const int TR = BSR_TR + ks - 1, TW = BSR_TC + ks - 1;
      const int row0 = i0 + c0 - (ks - 1), col0 = j0 + c0 - (ks - 1);
      for (int c = 0; c < 3; ++c) {
        __syncthreads();   // the previous channel's reads are done (and, first, nothing)
        for (int r = rg; r < TR; r += 4) {
          const float* srow = sp + c * plane + (long)mirror(row0 + r, h_in) * a.Wmax;
          for (int cc = lane; cc < TW; cc += 64) sT[r * BSR_LW + cc] = srow[mirror(col0 + cc, w_in)];
        }
        __syncthreads();
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        // tap (u, v) of output (li, lane) reads tile row li + ks-1-u, column lane + ks-1-v
        for (int u = 0; u < ks; ++u) {
          const float* tr = sT + (rg * 4 + ks - 1 - u) * BSR_LW + lane + ks - 1;
          for (int v = 0; v < ks; ++v) {
            const float w = sK[u * ks + v];
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = fmaf(w, tr[m * BSR_LW - v], acc[m]);
          }
        }
        if (j < w_out) {
#pragma unroll
          for (int m = 0; m < 4; ++m)
            if (ib + m < h_out) dp[c * plane + (long)(ib + m) * a.Wmax + j] = clip01(acc[m]);
        }
      }
      return;
    }
    if (j >= w_out) return;
    for (int m = 0; m < 4; ++m) {
      const int i = ib + m;
      if (i >= h_out) break;
      for (int c = 0; c < 3; ++c) {
        const float* pc = sp + c * plane;
        float acc = 0.f;
        for (int u = 0; u < ks; ++u) {
          const float* srow = pc + (long)mirror(i * st + c0 - u, h_in) * a.Wmax;
          for (int v = 0; v < ks; ++v) acc = fmaf(kb[u * ks + v], srow[mirror(j * st + c0 - v, w_in)], acc);
        }
        dp[c * plane + (long)i * a.Wmax + j] = clip01(acc);
      }
    }
    return;
  }

  if (j >= w_out) return;
  if (op == BSR_RESIZE) {
    int kind = clampi(row[5], BSR_BILINEAR, BSR_MATLAB_HALF);
    // the uploaded MATLAB taps serve one input size; a row they do not fit resizes by area instead of reading past them
    if (kind == BSR_MATLAB_HALF && (!a.ih || h_in != a.mh_in || w_in != a.mw_in || h_out != (h_in + 1) / 2 ||
                                    w_out != (w_in + 1) / 2))
      kind = BSR_AREA;
    const Axis ax = axis_init(kind, w_in, w_out, j, a.iw, a.ww, a.P);
    for (int m = 0; m < 4; ++m) {
      const int i = ib + m;
      if (i >= h_out) break;
      const Axis ay = axis_init(kind, h_in, h_out, i, a.ih, a.wh, a.P);
      float acc[3] = {0.f, 0.f, 0.f};
      for (int p = 0; p < ay.n; ++p) {
        int y;
        float wy;
        axis_tap(ay, p, y, wy);
        float r[3] = {0.f, 0.f, 0.f};
        for (int q = 0; q < ax.n; ++q) {
          int x;
          float wx;
          axis_tap(ax, q, x, wx);
          const float* s0 = sp + (long)y * a.Wmax + x;
#pragma unroll
          for (int c = 0; c < 3; ++c) r[c] = fmaf(wx, s0[c * plane], r[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fmaf(wy, r[c], acc[c]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) dp[c * plane + (long)i * a.Wmax + j] = clip01(acc[c]);
    }
    return;
  }

  // elementwise ops: (h_out, w_out) is (h_in, w_in)
  for (int m = 0; m < 4; ++m) {
    const int i = ib + m;
    if (i >= h_out) break;
    const long o = (long)i * a.Wmax + j;
    float v[3] = {sp[o], sp[plane + o], sp[2 * plane + o]};
    if (op == BSR_NOISE) {
      const unsigned long long e = (unsigned long long)((long)b * 3 * plane + o);   // channel 0's element
      const int mode = row[5];
      const float sigma = fr[0];
      const float n0 = normal_at(e, a.seed, a.stepkey);
      if (mode == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = fmaf(sigma, n0, v[c]);
      } else {
        const float n1 = normal_at(e + plane, a.seed, a.stepkey), n2 = normal_at(e + 2 * plane, a.seed, a.stepkey);
        if (mode == 0) {
          v[0] = fmaf(sigma, n0, v[0]);
          v[1] = fmaf(sigma, n1, v[1]);
          v[2] = fmaf(sigma, n2, v[2]);
        } else {   // L n, L the lower factor {L00, L10, L11, L20, L21, L22}
          v[0] += fr[1] * n0;
          v[1] += fr[2] * n0 + fr[3] * n1;
          v[2] += fr[4] * n0 + fr[5] * n1 + fr[6] * n2;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = clip01(v[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dp[c * plane + o] = v[c];
  }
}

// grid (B, nslot), one workgroup per (sample, slot).  Evaluated in fp64 as kair_usr_gauss_kernels is, so the fp32
// result is the rounded formula; the sum is taken per thread, then over the threads in index order.
__global__ __launch_bounds__(256) void bsr_gauss_kernel(const int* __restrict__ tab, int tstride, int slot_stride, int B,
                                                        float* __restrict__ out, long kstride, int kmax) {
  __shared__ double red[256];
  __shared__ double total;
  const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int* row = tab + (long)b * tstride + (long)s * slot_stride;
  const int op = row[0];
  if (op != BSR_BLUR && op != BSR_BLURDEC) return;
  const int ks = clampi(row[5], 1, kmax), n = ks * ks;
  const int sf_k = op == BSR_BLURDEC ? row[6] : 1;
  const float* fr = reinterpret_cast<const float*>(row + 8);
  const double l1 = fr[0], l2 = fr[1], th = fr[2];
  const double cs = cos(th), sn = sin(th);
  const double a11 = cs * cs / l1 + sn * sn / l2, a12 = cs * sn * (1.0 / l1 - 1.0 / l2),
               a22 = sn * sn / l1 + cs * cs / l2;
  const double mu = ks / 2 + 0.5 * (sf_k - ks % 2);
  float* o = out + ((long)s * B + b) * kstride;
  double part = 0.0;
  for (int t = tid; t < n; t += 256) {
    const double zx = t % ks - mu, zy = t / ks - mu;
    part += exp(-0.5 * (a11 * zx * zx + 2.0 * a12 * zx * zy + a22 * zy * zy));
  }
  red[tid] = part;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int i = 0; i < 256; ++i) sum += red[i];
    total = sum;
  }
  __syncthreads();
  const double inv = 1.0 / total;
  for (int t = tid; t < n; t += 256) {
    const double zx = t % ks - mu, zy = t / ks - mu;
    o[t] = (float)(exp(-0.5 * (a11 * zx * zx + 2.0 * a12 * zx * zy + a22 * zy * zy)) * inv);
  }
}

struct BsrPool {
  const float* pool;
  int N, Hs, Ws, PS;
  const int* head;   // per sample {image, rnd_h, rnd_w, mode, lq_h, lq_w}
  int hstride;
};

// element (c, i, j) of sample b's augmented PS^2 crop
KAIR_DEV float bsr_patch(const BsrPool& p, const int* hd, int c, int i, int j) {
  const int image = clampi(hd[0], 0, p.N - 1), y0 = clampi(hd[1], 0, p.Hs - p.PS), x0 = clampi(hd[2], 0, p.Ws - p.PS);
  int si, sj;
  aug_src(hd[3] & 7, i, j, p.PS, si, sj);
  return p.pool[(((long)image * 3 + c) * p.Hs + y0 + si) * p.Ws + x0 + sj];
}

__global__ __launch_bounds__(256) void bsr_crop_kernel(const BsrPool p, int B, float* __restrict__ dst) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x, per = 3L * p.PS * p.PS;
  if (t >= B * per) return;
  const int b = (int)(t / per);
  long r = t - b * per;
  const int c = (int)(r / ((long)p.PS * p.PS));
  r -= (long)c * p.PS * p.PS;
  const int i = (int)(r / p.PS), j = (int)(r - (long)i * p.PS);
  dst[t] = bsr_patch(p, p.head + (long)b * p.hstride, c, i, j);
}

// [0, nL): L elements from the buffer; then the H elements from the pool
__global__ __launch_bounds__(256) void bsr_finish_kernel(const BsrPool p, int B, int sf, int lq, const float* __restrict__ src,
                                                         float* __restrict__ outL, float* __restrict__ outH) {
  const int hq = lq * sf;
  const long nL = (long)B * 3 * lq * lq, nH = (long)B * 3 * hq * hq;
  long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= nL + nH) return;
  const bool isH = t >= nL;
  if (isH) t -= nL;
  const int n = isH ? hq : lq;
  const int j = (int)(t % n);
  long r = t / n;
  const int i = (int)(r % n);
  r /= n;
  const int c = (int)(r % 3), b = (int)(r / 3);
  const int* hd = p.head + (long)b * p.hstride;
  const int lim = max(p.PS / sf - lq, 0);
  const int lh = clampi(hd[4], 0, lim), lw = clampi(hd[5], 0, lim);
  if (isH)
    outH[t] = bsr_patch(p, hd, c, lh * sf + i, lw * sf + j);
  else
    outL[t] = src[(((long)b * 3 + c) * p.PS + lh + i) * p.PS + lw + j];
}

int bsr_pool_args(BsrPool& p, const float* pool, int N, int C, int Hs, int Ws, const int* head, int hstride, int B, int PS) {
  KAIR_CHECK_ARG(pool && head, "bsr: null pointer");
  KAIR_CHECK_ARG(C == 3, "bsr: the blind-SR pipeline needs a 3-channel pool (got %d)", C);
  KAIR_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0 && B > 0 && PS > 0 && PS < (1 << 14) && hstride >= 6,
                 "bsr: bad sizes (N %d, %dx%d, B %d, PS %d, hstride %d)", N, Hs, Ws, B, PS, hstride);
  KAIR_CHECK_ARG(PS <= Hs && PS <= Ws, "bsr: pool images smaller than the patch (%d)", PS);
  p = BsrPool{pool, N, Hs, Ws, PS, head, hstride};
  return 0;
}

}  // namespace

extern "C" int kair_bsr_crop(const float* pool, int N, int C, int Hs, int Ws, const int* head, int hstride, int B, int PS,
                             float* dst, void* stream) {
  BsrPool p;
  if (int rc = bsr_pool_args(p, pool, N, C, Hs, Ws, head, hstride, B, PS)) return rc;
  KAIR_CHECK_ARG(dst, "bsr_crop: null pointer");
  const long total = (long)B * 3 * PS * PS;
  KAIR_CHECK_ARG((total + 255) / 256 < (1L << 31), "bsr_crop: too many elements");
  KAIR_LAUNCH(bsr_crop_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, B, dst);
  KAIR_CHECK_LAUNCH();
  return 0;
}

extern "C" int kair_bsr_finish(const float* pool, int N, int C, int Hs, int Ws, const int* head, int hstride, int B,
                               int PS, int sf, int lq, const float* src, float* outL, float* outH, void* stream) {
  BsrPool p;
  if (int rc = bsr_pool_args(p, pool, N, C, Hs, Ws, head, hstride, B, PS)) return rc;
  KAIR_CHECK_ARG(src && outL && outH, "bsr_finish: null pointer");
  KAIR_CHECK_ARG(sf > 0 && lq > 0 && PS % sf == 0 && (long)lq * sf <= PS,
                 "bsr_finish: bad sizes (PS %d, sf %d, lq %d)", PS, sf, lq);
  const long total = (long)B * 3 * lq * lq * (1 + (long)sf * sf);
  KAIR_CHECK_ARG((total + 255) / 256 < (1L << 31), "bsr_finish: too many elements");
  KAIR_LAUNCH(bsr_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, B, sf, lq,
              src, outL, outH);
  KAIR_CHECK_LAUNCH();
  return 0;
}

static int bsr_kmax(long kstride) {
  int k = 1;
  while ((long)(k + 1) * (k + 1) <= kstride && k < 255) ++k;
  return k;
}

extern "C" int kair_bsr_kernels(const int* table, int tstride, int slot_stride, int nslot, int B, float* out, long kstride,
                                void* stream) {
  KAIR_CHECK_ARG(table && out, "bsr_kernels: null pointer");
  KAIR_CHECK_ARG(B > 0 && nslot > 0 && nslot <= 65535 && slot_stride >= 16 && kstride >= 1 &&
                     tstride >= (long)(nslot - 1) * slot_stride + 16,
                 "bsr_kernels: bad sizes (B %d, nslot %d, strides %d %d, kstride %ld)", B, nslot, tstride, slot_stride,
                 kstride);
  KAIR_LAUNCH(bsr_gauss_kernel, dim3((unsigned)B, (unsigned)nslot), dim3(256), 0, (hipStream_t)stream, table, tstride,
              slot_stride, B, out, kstride, bsr_kmax(kstride));
  KAIR_CHECK_LAUNCH();
  return 0;
}

extern "C" int kair_bsr_ops(const float* src, float* dst, int B, int Hmax, int Wmax, const int* table, int tstride,
                            const float* k, long kstride, const int* taps_ih, const float* taps_wh, const int* taps_iw,
                            const float* taps_ww, int P, int taps_h_in, int taps_w_in, unsigned long long seed,
                            unsigned long long step, int slot, int direct, void* stream) {
  KAIR_CHECK_ARG(src && dst && table && src != dst, "bsr_ops: null pointer, or src and dst are one buffer");
  KAIR_CHECK_ARG(B > 0 && B <= 65535 && Hmax > 0 && Wmax > 0 && Hmax < (1 << 14) && Wmax < (1 << 14) && tstride >= 16 &&
                     slot >= 0 && slot < 8,
                 "bsr_ops: bad sizes (B %d, buffer %dx%d, tstride %d, slot %d)", B, Hmax, Wmax, tstride, slot);
  KAIR_CHECK_ARG(k && kstride >= 1, "bsr_ops: the blur kernels (kair_bsr_kernels) are missing, or a bad stride %ld",
                 kstride);
  const bool taps = taps_ih || taps_wh || taps_iw || taps_ww;
  KAIR_CHECK_ARG(!taps || (taps_ih && taps_wh && taps_iw && taps_ww && P > 0 && taps_h_in > 0 && taps_w_in > 0),
                 "bsr_ops: the MATLAB taps need all four tables, P and the input size they were made for");
  BsrArgs a{};
  a.src = src; a.dst = dst; a.B = B; a.Hmax = Hmax; a.Wmax = Wmax;
  a.tiles_x = (Wmax + BSR_TC - 1) / BSR_TC;
  a.tab = table; a.tstride = tstride;
  a.k = k; a.kstride = kstride; a.kmax = bsr_kmax(kstride);
  a.ih = taps_ih; a.wh = taps_wh; a.iw = taps_iw; a.ww = taps_ww; a.P = P; a.mh_in = taps_h_in; a.mw_in = taps_w_in;
  a.seed = seed; a.stepkey = step * 8ull + (unsigned)slot;
  a.direct = direct;
  const int tiles_y = (Hmax + BSR_TR - 1) / BSR_TR;
  KAIR_LAUNCH(bsr_ops_kernel, dim3((unsigned)(a.tiles_x * tiles_y), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  KAIR_CHECK_LAUNCH();
  return 0;
}
