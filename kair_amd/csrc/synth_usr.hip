// USRNet training data on the MI355X: the per-sample work of DatasetUSRNet.__getitem__
// (data/dataset_usrnet.py:46-113) for a whole batch, from an image pool resident in HBM.
//
//   kair_usr_gauss_kernels  utils_sisr.gen_kernel (utils_sisr.py:172-215): B anisotropic Gaussian blur kernels
//                           [B][kh][kw] from per-sample (lambda1, lambda2, theta, sf_k, mode_k), or rows of a
//                           caller's kernel bank, one workgroup per sample.
//   kair_synth_usr          H = aug(crop(pool)); L = (k (*) H, circular)[0::sf, 0::sf] (+ the uint8 truncation
//                           of ndimage.convolve on a uint8 patch) + sigma_b N(0, 1), one launch.
//   kair_usr_degrade        the same degradation of whole (rectangular) images, no crop / augment.
//
// Forward model, the one USRNet's p2o centring assumes:
//   L0[i][j] = sum_{u, v} k[u][v] H[(i sf + kh/2 - u) mod PH][(j sf + kw/2 - v) mod PW]
// with a true modulo (the index wraps more than once when the patch is smaller than the kernel).  Every output is
// one fp32 fmaf chain over (u, v) in row-major order in both kernels below, so the banded and the direct kernel,
// and any band split, give the same bits.
//
// Banded kernel: one workgroup per (sample, channel, band of L rows).  The kh x kw taps and the band's
// (nr - 1) sf + kh rows of H with their wrapped halo ((LW - 1) sf + kw columns) are staged in LDS once, read through
// the crop and augment map.  The tile is stored de-interleaved by column phase -- column cc at
// [row][cc % sf][cc / sf] -- so the lanes of a wave, which hold consecutive L columns j and read column
// j sf + d for a wave-uniform d, read consecutive LDS words at every sf (a plain row layout is a 2-way bank conflict
// at sf 4).  Each thread carries M outputs through one tap loop, so a tap is read from LDS once per M fmafs.
// Only the decimated outputs are computed.  Shapes whose kh-row band does not fit in LDS take the direct kernel
// (one thread per output, H read from global through the same maps).
#include "synth_common.h"

namespace {

struct UsrArgs {
  const float* src;   // [N][C][Hs][Ws]
  int N, C, Hs, Ws;
  const int* par;     // per sample {image, rnd_h, rnd_w, mode} at stride pstride; null: whole images (PH = Hs, PW = Ws)
  int pstride;
  int PH, PW, sf, LH, LW;
  const float* k;     // [B][kh][kw] at stride kstride (0: one kernel for every sample)
  long kstride;
  int kh, kw;
  const float* sigma;   // per sample at stride sstride; null: no noise
  int sstride, trunc8;
  unsigned long long seed, step;
  float* outH;   // null: not written
  float* outL;
  // banded kernel
  int nband, rpb, RS, PWp, p0, q0;
  FDiv dsf, dLW;
};

struct UsrGeo {
  const float* img;
  int mode;
};

// sample b, channel c: the plane its patch is cut from, offset to the crop's corner (clamped into the image)
KAIR_DEV UsrGeo usr_geo(const UsrArgs& a, int b, int c) {
  int image = b, y0 = 0, x0 = 0, mode = 0;
  if (a.par) {
    const int* p = a.par + (long)b * a.pstride;
    image = min(max(p[0], 0), a.N - 1);
    y0 = min(max(p[1], 0), a.Hs - a.PH);
    x0 = min(max(p[2], 0), a.Ws - a.PW);
    mode = p[3] & 7;
  }
  return UsrGeo{a.src + (((long)image * a.C + c) * a.Hs + y0) * a.Ws + x0, mode};
}

// H(i, j) of the augmented crop (mode != 0 only with PH == PW)
KAIR_DEV float usr_h(const UsrArgs& a, const UsrGeo& g, int i, int j) {
  int si, sj;
  aug_src(g.mode, i, j, a.PH, si, sj);
  return g.img[(long)si * a.Ws + sj];
}

KAIR_DEV int wrap(int x, int n) {
  const int m = x % n;
  return m < 0 ? m + n : m;
}

// L = (trunc8 ? floor(255 L0) / 255 : L0) + sigma_b N(0, 1); sigma_b == 0 adds nothing
KAIR_DEV float usr_finish(const UsrArgs& a, float acc, int b, long idx) {
  if (a.trunc8) acc = floorf(255.f * acc) / 255.f;
  if (a.sigma) {
    const float s = a.sigma[(long)b * a.sstride];
    if (s != 0.f) acc = fmaf(s, normal_at((unsigned long long)idx, a.seed, a.step), acc);
  }
  return acc;
}

constexpr int USR_E = 8;   // staged columns per lane and pass

template <int M>
__global__ __launch_bounds__(256) void usr_band_kernel(const UsrArgs a) {
  extern __shared__ float sm[];
  float* sK = sm;                  // [kh][kw]
  float* sT = sm + a.kh * a.kw;    // [rows of the band][sf phases][PWp]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sc = blockIdx.x / a.nband, band = blockIdx.x - sc * a.nband;
  const int b = sc / a.C, c = sc - (sc / a.C) * a.C;
  const UsrGeo g = usr_geo(a, b, c);
  // this band's share of the H crop
  if (a.outH) {
    float* oH = a.outH + (long)(b * a.C + c) * a.PH * a.PW;
    const int nH = a.PH * a.PW, hpb = (nH + a.nband - 1) / a.nband, h0 = band * hpb, h1 = min(nH, h0 + hpb);
    for (int t = h0 + tid; t < h1; t += 256) {
      const int i = t / a.PW;
      oH[t] = usr_h(a, g, i, t - i * a.PW);
    }
  }
  const int r0 = band * a.rpb, r1 = min(a.LH, r0 + a.rpb), nr = r1 - r0;
  if (nr <= 0) return;
  const float* kb = a.k + (long)b * a.kstride;
  for (int t = tid; t < a.kh * a.kw; t += 256) sK[t] = kb[t];
  // tile rows row0 .. row0 + TR - 1 and columns col0 .. col0 + TW - 1 of the periodic H; a wave per row
  const int TR = (nr - 1) * a.sf + a.kh, TW = (a.LW - 1) * a.sf + a.kw;
  const int row0 = r0 * a.sf + a.kh / 2 - (a.kh - 1), col0 = a.kw / 2 - (a.kw - 1);
  for (int rr = wv; rr < TR; rr += 4) {
    const int i = wrap(row0 + rr, a.PH);
    float* row = sT + rr * a.RS;
    int j = wrap(col0 + lane, a.PW);
    // USR_E loads in flight per lane before the LDS writes: the staging is bound by global latency
    for (int cc0 = lane; cc0 < TW; cc0 += 64 * USR_E) {
      float v[USR_E];
#pragma unroll
      for (int e = 0; e < USR_E; ++e) {
        v[e] = cc0 + 64 * e < TW ? usr_h(a, g, i, j) : 0.f;
        j += 64;
        if (j >= a.PW) j %= a.PW;
      }
#pragma unroll
      for (int e = 0; e < USR_E; ++e) {
        const int cc = cc0 + 64 * e;
        if (cc < TW) {
          const int q = fdiv(cc, a.dsf);
          row[(cc - q * a.sf) * a.PWp + q] = v[e];
        }
      }
    }
  }
  __syncthreads();
  // output (li, j) of the band: tap (u, v) reads tile row li sf + kh-1-u, column j sf + d with d = kw-1-v, which is
  // phase d % sf, word j + d / sf
  const int nitems = nr * a.LW;
  float* oL = a.outL + ((long)(b * a.C + c) * a.LH + r0) * a.LW;
  for (int t0 = 0; t0 < nitems; t0 += 256 * M) {
    int base[M];
    float acc[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int t = min(t0 + m * 256 + tid, nitems - 1);
      const int li = fdiv(t, a.dLW);
      base[m] = li * a.sf * a.RS + (t - li * a.LW);
      acc[m] = 0.f;
    }
    for (int u = 0; u < a.kh; ++u) {
      const float* kr = sK + u * a.kw;
      int off = (a.kh - 1 - u) * a.RS + a.p0 * a.PWp + a.q0, p = a.p0;
      for (int v = 0; v < a.kw; ++v) {
        const float w = kr[v];
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = fmaf(w, sT[base[m] + off], acc[m]);
        if (p == 0) {
          p = a.sf - 1;
          off += (a.sf - 1) * a.PWp - 1;
        } else {
          --p;
          off -= a.PWp;
        }
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int t = t0 + m * 256 + tid;
      if (t < nitems) oL[t] = usr_finish(a, acc[m], b, (oL - a.outL) + t);
    }
  }
}

// one thread per output element: [0, nH) -> H patch elements (outH given), then the L elements
__global__ __launch_bounds__(256) void usr_direct_kernel(const UsrArgs a, int B) {
  const long nH = a.outH ? (long)B * a.C * a.PH * a.PW : 0, nL = (long)B * a.C * a.LH * a.LW;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nH + nL) return;
  if (t < nH) {
    const int j = (int)(t % a.PW);
    long r = t / a.PW;
    const int i = (int)(r % a.PH);
    r /= a.PH;
    const UsrGeo g = usr_geo(a, (int)(r / a.C), (int)(r % a.C));
    a.outH[t] = usr_h(a, g, i, j);
    return;
  }
  const long e = t - nH;
  const int j = (int)(e % a.LW);
  long r = e / a.LW;
  const int i = (int)(r % a.LH);
  r /= a.LH;
  const int c = (int)(r % a.C), b = (int)(r / a.C);
  const UsrGeo g = usr_geo(a, b, c);
  const float* kb = a.k + (long)b * a.kstride;
  const int j0 = wrap(j * a.sf + a.kw / 2, a.PW);
  int y = wrap(i * a.sf + a.kh / 2, a.PH);
  float acc = 0.f;
  for (int u = 0; u < a.kh; ++u) {
    int x = j0;
    for (int v = 0; v < a.kw; ++v) {
      acc = fmaf(kb[u * a.kw + v], usr_h(a, g, y, x), acc);
      x = x == 0 ? a.PW - 1 : x - 1;
    }
    y = y == 0 ? a.PH - 1 : y - 1;
  }
  a.outL[e] = usr_finish(a, acc, b, e);
}

constexpr int USR_M = 4;                     // outputs per thread and tap loop
constexpr long USR_LDS_BYTES = 150 * 1024;   // of CDNA4's 160 KB per workgroup

int launch_usr(UsrArgs a, int B, int direct, hipStream_t s) {
  const long TW = (long)(a.LW - 1) * a.sf + a.kw;
  const long PWp = (TW + a.sf - 1) / a.sf, RS = PWp * a.sf;
  const long rows_fit = (USR_LDS_BYTES / 4 - (long)a.kh * a.kw) / RS;   // tile rows that fit beside the taps
  const long rpb_lds = rows_fit >= a.kh ? (rows_fit - a.kh) / a.sf + 1 : 0;
  const long nsc = (long)B * a.C;
  if (!direct && rpb_lds >= 1 && TW < (1L << 24)) {
    // bands of L rows: ~2048 workgroups over the batch (a 4-patch batch still fills the CUs), at most
    // 256 * USR_M outputs each (one pass of the tap loop), and the tile within LDS
    long nfill = 2048 / nsc;
    nfill = nfill < 1 ? 1 : (nfill > a.LH ? a.LH : nfill);
    long rpb = (a.LH + nfill - 1) / nfill;
    const long rpb_items = (256 * USR_M) / a.LW > 1 ? (256 * USR_M) / a.LW : 1;
    rpb = rpb < rpb_items ? rpb : rpb_items;
    rpb = rpb < rpb_lds ? rpb : rpb_lds;
    const long nband = (a.LH + rpb - 1) / rpb;
    KAIR_CHECK_ARG(nsc * nband < (1L << 31) && rpb * a.LW < (1L << 24), "synth_usr: too many workgroups");
    a.nband = (int)nband;
    a.rpb = (int)rpb;
    a.RS = (int)RS;
    a.PWp = (int)PWp;
    a.p0 = (a.kw - 1) % a.sf;
    a.q0 = (a.kw - 1) / a.sf;
    a.dsf = make_fdiv(a.sf);
    a.dLW = make_fdiv(a.LW);
    const size_t lds = (size_t)((long)a.kh * a.kw + ((rpb - 1) * a.sf + a.kh) * RS) * sizeof(float);
    KAIR_LAUNCH(usr_band_kernel<USR_M>, dim3((unsigned)(nsc * nband)), dim3(256), lds, s, a);
  } else {
    const long total = (a.outH ? nsc * a.PH * a.PW : 0) + nsc * a.LH * a.LW;
    KAIR_CHECK_ARG((total + 255) / 256 < (1L << 31), "synth_usr: too many elements");
    KAIR_LAUNCH(usr_direct_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, B);
  }
  KAIR_CHECK_LAUNCH();
  return 0;
}

// One workgroup per sample.  Evaluated in fp64 (625 taps per sample: free) so the fp32 result is the rounded
// formula; the sum is taken per thread, then over the threads in index order.
__global__ __launch_bounds__(256) void usr_gauss_kernel(const float* __restrict__ gpar, int gstride,
                                                        const int* __restrict__ kpar, int kstride,
                                                        const float* __restrict__ bank, int K, int ks,
                                                        float* __restrict__ out) {
  __shared__ double red[256];
  __shared__ double total;
  const int b = blockIdx.x, tid = threadIdx.x, n = ks * ks;
  const int* kp = kpar + (long)b * kstride;   // {source (0 Gaussian, 1 bank), bank_idx, sf_k, mode_k}
  const bool from_bank = kp[0] != 0 && bank != nullptr && K > 0;
  const float* row = from_bank ? bank + (long)min(max(kp[1], 0), K - 1) * n : nullptr;
  const float* gp = gpar + (long)b * gstride;   // {lambda1, lambda2, theta}
  const double l1 = gp[0], l2 = gp[1], th = gp[2];
  const double cs = cos(th), sn = sin(th);
  // Sigma = Q diag(l1, l2) Q^T, Q = [[cs, -sn], [sn, cs]]; its inverse = Q diag(1/l1, 1/l2) Q^T
  const double a11 = cs * cs / l1 + sn * sn / l2, a12 = cs * sn * (1.0 / l1 - 1.0 / l2),
               a22 = sn * sn / l1 + cs * cs / l2;
  const double mu = ks / 2 + 0.5 * (kp[2] - ks % 2);
  const int mode = from_bank ? 0 : (kp[3] & 7);
  float* o = out + (long)b * n;
  double part = 0.0;
  for (int t = tid; t < n; t += 256) {
    double v;
    if (from_bank) {
      v = row[t];
    } else {
      int y, x;
      aug_src(mode, t / ks, t % ks, ks, y, x);
      const double zx = x - mu, zy = y - mu;
      v = exp(-0.5 * (a11 * zx * zx + 2.0 * a12 * zx * zy + a22 * zy * zy));
    }
    part += v;
  }
  red[tid] = part;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += red[i];
    total = s;
  }
  __syncthreads();
  const double inv = 1.0 / total;
  for (int t = tid; t < n; t += 256) {
    double v;
    if (from_bank) {
      v = row[t];
    } else {
      int y, x;
      aug_src(mode, t / ks, t % ks, ks, y, x);
      const double zx = x - mu, zy = y - mu;
      v = exp(-0.5 * (a11 * zx * zx + 2.0 * a12 * zx * zy + a22 * zy * zy));
    }
    o[t] = (float)(v * inv);
  }
}

}  // namespace

extern "C" int kair_usr_gauss_kernels(const float* gpar, int gstride, const int* kpar, int kstride, const float* bank,
                                      int K, int B, int ksize, float* out, void* stream) {
  KAIR_CHECK_ARG(gpar && kpar && out, "usr_gauss_kernels: null pointer");
  KAIR_CHECK_ARG(B > 0 && ksize > 0 && ksize <= 4096 && gstride >= 3 && kstride >= 4 && K >= 0 && (K == 0 || bank),
                 "usr_gauss_kernels: bad sizes (B %d, ksize %d, strides %d %d, K %d)", B, ksize, gstride, kstride, K);
  KAIR_LAUNCH(usr_gauss_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, gpar, gstride, kpar, kstride, bank,
              K, ksize, out);
  KAIR_CHECK_LAUNCH();
  return 0;
}

extern "C" int kair_synth_usr(const float* pool, int N, int C, int Hs, int Ws, const int* params, int pstride, int B,
                              int PS, int sf, const float* k, int kh, int kw, const float* sigma, int sstride,
                              int trunc8, unsigned long long seed, unsigned long long step, float* outH, float* outL,
                              int direct, void* stream) {
  KAIR_CHECK_ARG(pool && params && k && outH && outL, "synth_usr: null pointer");
  KAIR_CHECK_ARG(N > 0 && C > 0 && Hs > 0 && Ws > 0 && B > 0 && sf > 0 && PS > 0 && PS % sf == 0 && kh > 0 && kw > 0 &&
                     kh <= 1024 && kw <= 1024 && pstride >= 4 && (!sigma || sstride >= 0),
                 "synth_usr: bad sizes (N %d, C %d, %dx%d, B %d, PS %d, sf %d, k %dx%d)", N, C, Hs, Ws, B, PS, sf, kh, kw);
  KAIR_CHECK_ARG(PS <= Hs && PS <= Ws, "synth_usr: pool images smaller than the patch");
  UsrArgs a{};
  a.src = pool; a.N = N; a.C = C; a.Hs = Hs; a.Ws = Ws;
  a.par = params; a.pstride = pstride;
  a.PH = PS; a.PW = PS; a.sf = sf; a.LH = PS / sf; a.LW = PS / sf;
  a.k = k; a.kstride = (long)kh * kw; a.kh = kh; a.kw = kw;
  a.sigma = sigma; a.sstride = sstride; a.trunc8 = trunc8;
  a.seed = seed; a.step = step;
  a.outH = outH; a.outL = outL;
  return launch_usr(a, B, direct, (hipStream_t)stream);
}

extern "C" int kair_usr_degrade(const float* x, int N, int C, int Hs, int Ws, int sf, const float* k, long kstride,
                                int kh, int kw, const float* sigma, int sstride, int trunc8, unsigned long long seed,
                                unsigned long long step, float* outL, int direct, void* stream) {
  KAIR_CHECK_ARG(x && k && outL, "usr_degrade: null pointer");
  KAIR_CHECK_ARG(N > 0 && C > 0 && Hs > 0 && Ws > 0 && sf > 0 && kh > 0 && kw > 0 && kh <= 1024 && kw <= 1024 &&
                     (kstride == 0 || kstride >= (long)kh * kw) && (!sigma || sstride >= 0),
                 "usr_degrade: bad sizes (N %d, C %d, %dx%d, sf %d, k %dx%d)", N, C, Hs, Ws, sf, kh, kw);
  UsrArgs a{};
  a.src = x; a.N = N; a.C = C; a.Hs = Hs; a.Ws = Ws;
  a.par = nullptr; a.pstride = 0;
  a.PH = Hs; a.PW = Ws; a.sf = sf; a.LH = (Hs + sf - 1) / sf; a.LW = (Ws + sf - 1) / sf;
  a.k = k; a.kstride = kstride; a.kh = kh; a.kw = kw;
  a.sigma = sigma; a.sstride = sstride; a.trunc8 = trunc8;
  a.seed = seed; a.step = step;
  a.outH = nullptr; a.outL = outL;
  return launch_usr(a, N, direct, (hipStream_t)stream);
}
