// SRMD training data on the MI355X: the per-sample work of DatasetSRMD.__getitem__ (data/dataset_srmd.py) for a
// whole batch, from an image pool resident in HBM.
//
//   kair_srmd_kernels  B anisotropic 15 x 15 Gaussian kernels (utils_sisr.anisotropic_gaussian) from per-sample
//                      (theta, l1, l2), and their PCA codes P @ vec_F(k), one workgroup per sample, one launch.
//   kair_synth_srmd    H = aug(crop(pool)); L = [bicubic_{1/sf}(k_b (*) H, circular) + sigma_b N(0, 1) | code_b | sigma_b],
//                      one launch: crop, augment, blur, both resize passes, noise and the map channels.
//
// Forward model (utils_sisr.srmd_degrade):
//   Bl[y][x] = sum_{u, v} k[u][v] H[(y + 7 - u) mod PS][(x + 7 - v) mod PS]            (ndimage.convolve, mode 'wrap')
//   L0 = Mh Bl Mw^T, the MATLAB-bicubic imresize by 1 / sf: ceil(4 sf) + 2 taps per axis, antialiased, the border
//   reflected (utils_image.bicubic_taps builds the taps on the host, as for kair_synth_sr), rows first, then columns,
//   each one fp32 fmaf chain in tap order.
//
// One workgroup per (sample, channel, band of L rows), the band scheme of synth_usr.hip.  The band's vertical taps
// touch a contiguous range of blurred rows; those rows' share of H, with a wrapped halo of 7 on every side, is staged in
// LDS through the crop and augment map, blurred into a second LDS tile (fp32: the blurred patch never leaves the CU),
// resized vertically into a third, and the horizontal pass writes L.  Neighbouring bands blur the rows their taps share
// twice: with ~1024 workgroups a batch that is 2-3 x the blur's 225 MACs per pixel, against a round trip of the blurred
// batch through HBM and two more launches for the separate form.  The blur keeps a column of 15 taps and 4 outputs of
// consecutive rows in registers, so a staged value is read from LDS once per 4 fmafs.  Every workgroup also writes its
// share of the H crop and of the sample's map channels.
#include "synth_common.h"

namespace {

constexpr int SRMD_KS = 15;     // kernel size
constexpr int SRMD_HALO = 7;    // SRMD_KS / 2
constexpr int SRMD_R = 4;       // blurred rows per thread
constexpr long SRMD_LDS_BYTES = 150 * 1024;   // of CDNA4's 160 KB per workgroup

struct SrmdArgs {
  const float* pool;   // [N][C][Hs][Ws]
  int N, C, Hs, Ws;
  const int* par;      // per sample {image, rnd_h, rnd_w, mode, ..., [scol] = float bits of sigma_b} at stride pstride
  int pstride, scol;
  int PS, sf, LS;
  const float* k;      // [B][15][15]
  const float* code;   // [B][ncode]
  int ncode, noise_ch;
  const float* wt;     // [LS][P] bicubic weights of a PS -> LS axis
  const int* it;       // [LS][P] reflected source indices
  int P;
  unsigned long long seed, step;
  float* outH;         // [B][C][PS][PS]
  float* outL;         // [B][C + ncode + noise_ch][LS][LS]
  int nband, rpb, TRmax, TRa, TWp;
};

KAIR_DEV int wrap_ps(int x, int n) {
  const int m = x % n;
  return m < 0 ? m + n : m;
}

__global__ __launch_bounds__(256) void srmd_band_kernel(const SrmdArgs a) {
  extern __shared__ float sm[];
  __shared__ int sLo, sHi;
  float* sK = sm;                                                  // [15][15]
  float* sT = sm + 256;                                            // [TRa + 14][TWp]: H rows lo - 7 .., columns -7 ..
  float* sB = sT + (a.TRa + 2 * SRMD_HALO) * a.TWp;                // [TRa][PS]: blurred rows lo ..
  float* sV = sB + a.TRa * a.PS;                                   // [rpb][PS]: the vertical pass
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sc = blockIdx.x / a.nband, band = blockIdx.x - sc * a.nband;
  const int b = sc / a.C, c = sc - (sc / a.C) * a.C;
  const int PS = a.PS, LS = a.LS, P = a.P;
  const int* pr = a.par + (long)b * a.pstride;
  const int image = min(max(pr[0], 0), a.N - 1), y0 = min(max(pr[1], 0), a.Hs - PS), x0 = min(max(pr[2], 0), a.Ws - PS);
  const int mode = pr[3] & 7;
  const float sigma = __int_as_float(pr[a.scol]);
  const float* img = a.pool + (((long)image * a.C + c) * a.Hs + y0) * a.Ws + x0;
  const int CL = a.C + a.ncode + a.noise_ch;
  // this workgroup's share of the H crop ...
  {
    float* oH = a.outH + (long)(b * a.C + c) * PS * PS;
    const int nH = PS * PS, hpb = (nH + a.nband - 1) / a.nband, h0 = band * hpb, h1 = min(nH, h0 + hpb);
    for (int t = h0 + tid; t < h1; t += 256) {
      const int i = t / PS;
      int si, sj;
      aug_src(mode, i, t - i * PS, PS, si, sj);
      oH[t] = img[(long)si * a.Ws + sj];
    }
  }
  // ... and of the sample's map channels: the code, then the noise level, constant over the LR grid
  {
    const int nmap = (a.ncode + a.noise_ch) * LS * LS, shares = a.C * a.nband;
    const int per = (nmap + shares - 1) / shares, m0 = (c * a.nband + band) * per, m1 = min(nmap, m0 + per);
    float* oM = a.outL + ((long)b * CL + a.C) * LS * LS;
    for (int t = m0 + tid; t < m1; t += 256) {
      const int ch = t / (LS * LS);
      oM[t] = ch < a.ncode ? a.code[(long)b * a.ncode + ch] : sigma;
    }
  }
  const int r0 = band * a.rpb, r1 = min(LS, r0 + a.rpb), nr = r1 - r0;
  if (nr <= 0) return;
  // the blurred rows the band's vertical taps read: [lo, hi)
  if (tid == 0) { sLo = PS; sHi = 0; }
  __syncthreads();
  {
    int lo = PS, hi = 0;
    for (int t = tid; t < nr * P; t += 256) {
      const int y = min(max(a.it[r0 * P + t], 0), PS - 1);
      lo = min(lo, y);
      hi = max(hi, y + 1);
    }
    atomicMin(&sLo, lo);
    atomicMax(&sHi, hi);
  }
  for (int t = tid; t < SRMD_KS * SRMD_KS; t += 256) sK[t] = a.k[(long)b * SRMD_KS * SRMD_KS + t];
  __syncthreads();
  const int lo = sLo;
  // TR <= (nr - 1) sf + P + 2 <= TRmax by the tap geometry (reflected indices fold inward); clamped anyway
  const int TR = min(sHi - lo, a.TRmax);
  // stage H: tile row tr is H row (lo - 7 + tr) mod PS, tile column tc is H column (tc - 7) mod PS; a wave per row
  const int TW = PS + 2 * SRMD_HALO;
  for (int tr = wv; tr < a.TRa + 2 * SRMD_HALO; tr += 4) {
    float* row = sT + tr * a.TWp;
    if (tr < TR + 2 * SRMD_HALO) {
      const int i = wrap_ps(lo - SRMD_HALO + tr, PS);
      for (int tc = lane; tc < TW; tc += 64) {
        int si, sj;
        aug_src(mode, i, wrap_ps(tc - SRMD_HALO, PS), PS, si, sj);
        row[tc] = img[(long)si * a.Ws + sj];
      }
    } else {
      for (int tc = lane; tc < TW; tc += 64) row[tc] = 0.f;
    }
  }
  __syncthreads();
  // blur: blurred row lo + y, column x = sum_{u, v} k[u][v] tile[y + 14 - u][x + 14 - v]
  for (int item = tid; item < (a.TRa / SRMD_R) * PS; item += 256) {
    const int g = item / PS, x = item - g * PS, yb = g * SRMD_R;
    float acc[SRMD_R];
#pragma unroll
    for (int r = 0; r < SRMD_R; ++r) acc[r] = 0.f;
    for (int v = 0; v < SRMD_KS; ++v) {
      float kc[SRMD_KS];
#pragma unroll
      for (int u = 0; u < SRMD_KS; ++u) kc[u] = sK[u * SRMD_KS + v];
      const float* col = sT + yb * a.TWp + x + 2 * SRMD_HALO - v;
#pragma unroll
      for (int rr = 0; rr < SRMD_R + SRMD_KS - 1; ++rr) {
        const float t = col[rr * a.TWp];
#pragma unroll
        for (int r = 0; r < SRMD_R; ++r) {
          const int u = SRMD_KS - 1 - (rr - r);
          if (u >= 0 && u < SRMD_KS) acc[r] = fmaf(kc[u], t, acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < SRMD_R; ++r) sB[(yb + r) * PS + x] = acc[r];
  }
  __syncthreads();
  // vertical pass: V[r][x] = sum_a wt[gy][a] Bl[it[gy][a]][x], gy = r0 + r
  for (int t = tid; t < nr * PS; t += 256) {
    const int r = t / PS, x = t - r * PS;
    const float* w = a.wt + (long)(r0 + r) * P;
    const int* ix = a.it + (long)(r0 + r) * P;
    float acc = 0.f;
    for (int q = 0; q < P; ++q) acc = fmaf(w[q], sB[min(max(ix[q] - lo, 0), TR - 1) * PS + x], acc);
    sV[t] = acc;
  }
  __syncthreads();
  // horizontal pass, noise, store
  for (int t = tid; t < nr * LS; t += 256) {
    const int r = t / LS, j = t - r * LS;
    const float* w = a.wt + (long)j * P;
    const int* ix = a.it + (long)j * P;
    float acc = 0.f;
    for (int q = 0; q < P; ++q) acc = fmaf(w[q], sV[r * PS + min(max(ix[q], 0), PS - 1)], acc);
    const long u = (((long)b * a.C + c) * LS + r0 + r) * LS + j;   // the element's index in the [B][C][LS][LS] block
    if (sigma != 0.f) acc = fmaf(sigma, normal_at((unsigned long long)u, a.seed, a.step), acc);
    a.outL[(((long)b * CL + c) * LS + r0 + r) * LS + j] = acc;
  }
}

// One workgroup per sample: the kernel in fp64 (225 taps: free) so that the fp32 result is the rounded formula, summed
// per thread and then over the threads in index order; the codes are 15 fp32 fmaf chains over the column-major kernel.
__global__ __launch_bounds__(256) void srmd_kernels_kernel(const float* __restrict__ kpar, int kstride,
                                                           const float* __restrict__ Pm, int ncode,
                                                           float* __restrict__ outK, float* __restrict__ outCode) {
  __shared__ double red[256];
  __shared__ double total;
  __shared__ float sK[SRMD_KS * SRMD_KS];
  const int b = blockIdx.x, tid = threadIdx.x, n = SRMD_KS * SRMD_KS;
  const float* kp = kpar + (long)b * kstride;   // {theta, l1, l2}
  const double th = kp[0], l1 = fmax((double)kp[1], 1e-6), l2 = fmax((double)kp[2], 1e-6);
  const double cs = cos(th), sn = sin(th);
  // Sigma = R diag(l1, l2) R^T, R = [[cs, -sn], [sn, cs]]; its inverse = R diag(1 / l1, 1 / l2) R^T
  const double a11 = cs * cs / l1 + sn * sn / l2, a12 = cs * sn * (1.0 / l1 - 1.0 / l2),
               a22 = sn * sn / l1 + cs * cs / l2;
  double v = 0.0;
  if (tid < n) {
    const double zy = tid / SRMD_KS - SRMD_HALO, zx = tid % SRMD_KS - SRMD_HALO;
    v = exp(-0.5 * (a11 * zx * zx + 2.0 * a12 * zx * zy + a22 * zy * zy));
  }
  red[tid] = v;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += red[i];
    total = s;
  }
  __syncthreads();
  if (tid < n) {
    const float kf = (float)(v / total);
    sK[tid] = kf;
    outK[(long)b * n + tid] = kf;
  }
  __syncthreads();
  if (tid < ncode) {
    const float* row = Pm + (long)tid * n;
    float acc = 0.f;
    for (int f = 0; f < n; ++f) acc = fmaf(row[f], sK[(f % SRMD_KS) * SRMD_KS + f / SRMD_KS], acc);   // vec_F: f = c 15 + r
    outCode[(long)b * ncode + tid] = acc;
  }
}

}  // namespace

extern "C" int kair_srmd_kernels(const float* kpar, int kstride, const float* P, int ncode, int B, float* out_k,
                                 float* out_code, void* stream) {
  KAIR_CHECK_ARG(kpar && P && out_k && out_code, "srmd_kernels: null pointer");
  KAIR_CHECK_ARG(B > 0 && kstride >= 3 && ncode > 0 && ncode <= 256, "srmd_kernels: bad sizes (B %d, stride %d, ncode %d)",
                 B, kstride, ncode);
  KAIR_LAUNCH(srmd_kernels_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, kpar, kstride, P, ncode, out_k,
              out_code);
  KAIR_CHECK_LAUNCH();
  return 0;
}

extern "C" int kair_synth_srmd(const float* pool, int N, int C, int Hs, int Ws, const int* params, int pstride, int scol,
                               int B, int PS, int sf, const float* k, const float* code, int ncode, int noise_ch,
                               const float* wt, const int* it, int P, unsigned long long seed, unsigned long long step,
                               float* outH, float* outL, void* stream) {
  KAIR_CHECK_ARG(pool && params && k && code && wt && it && outH && outL, "synth_srmd: null pointer");
  KAIR_CHECK_ARG(N > 0 && C > 0 && Hs > 0 && Ws > 0 && B > 0 && sf > 0 && PS > 0 && PS % sf == 0 && P > 0 && ncode >= 0 &&
                     (noise_ch == 0 || noise_ch == 1),
                 "synth_srmd: bad sizes (N %d, C %d, %dx%d, B %d, PS %d, sf %d, P %d, ncode %d)", N, C, Hs, Ws, B, PS, sf, P,
                 ncode);
  KAIR_CHECK_ARG(PS <= Hs && PS <= Ws && PS < (1 << 14), "synth_srmd: pool images smaller than the patch, or PS >= 16384");
  KAIR_CHECK_ARG(pstride >= 5 && scol >= 4 && scol < pstride, "synth_srmd: level column %d outside rows of %d ints", scol,
                 pstride);
  SrmdArgs a{};
  a.pool = pool; a.N = N; a.C = C; a.Hs = Hs; a.Ws = Ws;
  a.par = params; a.pstride = pstride; a.scol = scol;
  a.PS = PS; a.sf = sf; a.LS = PS / sf;
  a.k = k; a.code = code; a.ncode = ncode; a.noise_ch = noise_ch;
  a.wt = wt; a.it = it; a.P = P;
  a.seed = seed; a.step = step;
  a.outH = outH; a.outL = outL;
  // bands of L rows: ~1024 workgroups over the batch, and the three tiles within LDS
  const long nsc = (long)B * C;
  long nfill = 1024 / nsc;
  nfill = nfill < 1 ? 1 : (nfill > a.LS ? a.LS : nfill);
  long rpb = (a.LS + nfill - 1) / nfill;
  const long TWp = PS + 2 * SRMD_HALO + 1;
  long TRmax, TRa, lds;
  for (;;) {
    TRmax = (rpb - 1) * sf + P + 2;
    TRmax = TRmax < PS ? TRmax : PS;
    TRa = (TRmax + SRMD_R - 1) / SRMD_R * SRMD_R;
    lds = (256 + (TRa + 2 * SRMD_HALO) * TWp + TRa * PS + rpb * PS) * (long)sizeof(float);
    if (lds <= SRMD_LDS_BYTES || rpb == 1) break;
    rpb = (rpb + 1) / 2;
  }
  KAIR_CHECK_ARG(lds <= SRMD_LDS_BYTES, "synth_srmd: one L row of a %d-pixel patch at sf %d needs %ld bytes of LDS", PS, sf,
                 lds);
  const long nband = (a.LS + rpb - 1) / rpb;
  KAIR_CHECK_ARG(nsc * nband < (1L << 31), "synth_srmd: too many workgroups");
  a.nband = (int)nband; a.rpb = (int)rpb; a.TRmax = (int)TRmax; a.TRa = (int)TRa; a.TWp = (int)TWp;
  KAIR_LAUNCH(srmd_band_kernel, dim3((unsigned)(nsc * nband)), dim3(256), (size_t)lds, (hipStream_t)stream, a);
  KAIR_CHECK_LAUNCH();
  return 0;
}
