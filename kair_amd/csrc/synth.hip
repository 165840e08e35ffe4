// Training-patch synthesis on the MI355X: the per-sample work of
//   DatasetSR.__getitem__    data/dataset_sr.py:35-92   (modcrop'd H, MATLAB-bicubic x1/sf L of the
//                                                        whole image, aligned random crop, 8-way augment)
//   DatasetDnCNN.__getitem__ data/dataset_dncnn.py:50-75 (random crop, 8-way augment, L = H + sigma N)
//   DatasetFDnCNN.__getitem__ data/dataset_fdncnn.py    (the same with one sigma per sample and the noise-level
//                                                        map as L's last channel)
// for a whole batch in one launch, reading an image pool resident in HBM (fp32 NCHW, [0, 1]).
//
// The 8 augment modes: aug_src in synth_common.h.
// Bicubic: separable taps per output row / column (weights and symmetric-reflected source indices
// from calculate_weights_indices, utils_image.py:880-932, built on the host), summed rows-first then
// columns as imresize does (utils_image.py:938-1005).  AWGN: Philox-4x32-10 keyed by (seed, step),
// counter = element index, Box-Muller -- no bitwise pin to torch's CPU generator is possible (or
// meaningful); tests check the noise statistically.
#include "synth_common.h"

namespace {

// one thread per output element: [0, nH) -> H patch elements, [nH, nH + nL) -> L patch elements
__global__ __launch_bounds__(256) void synth_sr_kernel(const float* __restrict__ pool, int C, int Hs, int Ws,
                                                       const int4* __restrict__ par, int B, int PS, int sf,
                                                       const float* __restrict__ wh, const int* __restrict__ ih,
                                                       const float* __restrict__ ww, const int* __restrict__ iw, int P,
                                                       float* __restrict__ outH, float* __restrict__ outL) {
  const int LS = PS / sf;
  const long nH = (long)B * C * PS * PS, nL = (long)B * C * LS * LS;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nH + nL) return;
  if (t < nH) {
    const int j = (int)(t % PS);
    long r = t / PS;
    const int i = (int)(r % PS);
    r /= PS;
    const int c = (int)(r % C), b = (int)(r / C);
    const int4 pr = par[b];   // x = image, y = rnd_h (LQ rows), z = rnd_w, w = mode
    int si, sj;
    aug_src(pr.w, i, j, PS, si, sj);
    outH[t] = pool[(((long)pr.x * C + c) * Hs + (long)pr.y * sf + si) * Ws + (long)pr.z * sf + sj];
    return;
  }
  const long u = t - nH;
  const int j = (int)(u % LS);
  long r = u / LS;
  const int i = (int)(r % LS);
  r /= LS;
  const int c = (int)(r % C), b = (int)(r / C);
  const int4 pr = par[b];
  int si, sj;
  aug_src(pr.w, i, j, LS, si, sj);
  const int gy = pr.y + si, gx = pr.z + sj;   // row / column of the whole-image L
  const float* img = pool + ((long)pr.x * C + c) * Hs * Ws;
  float acc = 0.f;
  for (int bq = 0; bq < P; ++bq) {
    const float wb = ww[gx * P + bq];
    const int x = iw[gx * P + bq];
    float col = 0.f;
    for (int a = 0; a < P; ++a) col = fmaf(wh[gy * P + a], img[(long)ih[gy * P + a] * Ws + x], col);
    acc = fmaf(wb, col, acc);
  }
  outL[u] = acc;
}

// Separable form, one workgroup per (sample, channel, band of L source rows): the vertical bicubic
// pass for the band's L-rows over the source-column window the horizontal taps touch is staged in
// LDS once, then every L pixel of the band is P horizontal taps over it -- LS*W*P + LS*LS*P MACs
// instead of LS*LS*P*P, with the same summation order as synth_sr_kernel (each vertical sum over a,
// then over bq), so the output is bitwise the same.  Bands split each sample's work over several
// workgroups (a 4-patch batch would otherwise run on 12 CUs); each also writes its share of the
// (augmented) H crop.  Outputs are addressed through the inverse augment map (dihedral: an
// involution up to the transpose), so a band writes exactly the L pixels whose source row it holds.
// DPSR (kair_synth_dpsr, DatasetDPSR): the same pair, then L = [L + sigma_b * N(0, 1) | sigma_b]: outL is
// [B][C + 1][LS][LS], sigma_b the float in column scol of sample b's parameter row (rows of 4 pstr4 ints), the normals'
// counter the element index of the [B][C][LS][LS] noisy block (kair_synth_dn_map's convention); channel 0's workgroups
// write the level plane, one share per band.  sigma_b == 0 adds nothing, so L's image channels are task "sr"'s bytes.
// The table's image and corner are clamped into the pool.
template <bool DPSR>
__global__ __launch_bounds__(256) void synth_sr_sep_kernel(const float* __restrict__ pool, int N, int C, int Hs, int Ws,
                                                           const int4* __restrict__ par, int pstr4, int scol, int PS,
                                                           int sf, const float* __restrict__ wh,
                                                           const int* __restrict__ ih, const float* __restrict__ ww,
                                                           const int* __restrict__ iw, int P, int Wmax, int nband,
                                                           unsigned long long seed, unsigned long long step,
                                                           float* __restrict__ outH, float* __restrict__ outL) {
  extern __shared__ float sV[];   // [rows of the band][Wmax]
  __shared__ int sLo, sHi;
  const int tid = threadIdx.x;
  const int sc = blockIdx.x / nband, band = blockIdx.x - sc * nband;
  const int b = sc / C, c = sc - (sc / C) * C;
  int4 pr = par[(long)b * pstr4];   // x = image, y = rnd_h (LQ rows), z = rnd_w, w = mode
  const int LS = PS / sf;
  float sigma = 0.f;
  if (DPSR) {
    sigma = __int_as_float(((const int*)par)[(long)b * pstr4 * 4 + scol]);
    pr.x = min(max(pr.x, 0), N - 1);
    pr.y = min(max(pr.y, 0), Hs / sf - LS);
    pr.z = min(max(pr.z, 0), Ws / sf - LS);
    pr.w &= 7;
  }
  const int CL = DPSR ? C + 1 : C;
  const int rpb = (LS + nband - 1) / nband, r0 = band * rpb, r1 = min(LS, r0 + rpb), nr = r1 - r0;
  const float* img = pool + ((long)pr.x * C + c) * Hs * Ws;
  // this band's share of the H crop
  float* oH = outH + (long)(b * C + c) * PS * PS;
  const int hpb = (PS * PS + nband - 1) / nband, h0 = band * hpb, h1 = min(PS * PS, h0 + hpb);
  for (int t = h0 + tid; t < h1; t += 256) {
    const int i = t / PS, j = t - (t / PS) * PS;
    int si, sj;
    aug_src(pr.w, i, j, PS, si, sj);
    oH[t] = img[(long)(pr.y * sf + si) * Ws + pr.z * sf + sj];
  }
  if (DPSR && c == 0) {   // this band's share of the level plane
    float* oM = outL + ((long)b * CL + C) * LS * LS;
    const int mpb = (LS * LS + nband - 1) / nband, m0 = band * mpb, m1 = min(LS * LS, m0 + mpb);
    for (int t = m0 + tid; t < m1; t += 256) oM[t] = sigma;
  }
  if (nr <= 0) return;
  // source-column window of the horizontal taps of L columns pr.z .. pr.z + LS - 1
  if (tid == 0) { sLo = Ws; sHi = 0; }
  __syncthreads();
  int lo = Ws, hi = 0;
  for (int t = tid; t < LS * P; t += 256) {
    const int x = iw[(pr.z + t / P) * P + t - (t / P) * P];
    lo = min(lo, x);
    hi = max(hi, x + 1);
  }
  atomicMin(&sLo, lo);
  atomicMax(&sHi, hi);
  __syncthreads();
  lo = sLo;
  // W <= PS + P + 2 sf <= Wmax by the tap geometry (reflected indices fold inward); clamped anyway
  const int W = min(sHi - lo, Wmax);
  // vertical pass: V[r - r0][x - lo] = sum_a wh[gy][a] * img[ih[gy][a]][x], gy = pr.y + r
  for (int t = tid; t < nr * W; t += 256) {
    const int r = t / W, xo = t - (t / W) * W, gy = pr.y + r0 + r;
    float acc = 0.f;
    for (int a = 0; a < P; ++a) acc = fmaf(wh[gy * P + a], img[(long)ih[gy * P + a] * Ws + lo + xo], acc);
    sV[r * Wmax + xo] = acc;
  }
  __syncthreads();
  // horizontal pass for source rows si in [r0, r1); output pixel through the inverse augment map
  float* oL = outL + ((long)b * CL + c) * LS * LS;
  for (int t = tid; t < nr * LS; t += 256) {
    const int si = r0 + t / LS, sj = t - (t / LS) * LS;
    const int p = (pr.w & 2) ? LS - 1 - si : si, q = (pr.w & 4) ? LS - 1 - sj : sj;
    const int i = (pr.w & 1) ? q : p, j = (pr.w & 1) ? p : q;
    const int gx = pr.z + sj;
    float acc = 0.f;
    for (int bq = 0; bq < P; ++bq) acc = fmaf(ww[gx * P + bq], sV[(si - r0) * Wmax + iw[gx * P + bq] - lo], acc);
    if (DPSR && sigma > 0.f)
      acc += sigma * normal_at((unsigned long long)((((long)b * C + c) * LS + i) * LS + j), seed, step);
    oL[i * LS + j] = acc;
  }
}

// H = aug(crop(pool)); L = H + sigma * N(0, 1)   (sigma already divided by 255)
__global__ __launch_bounds__(256) void synth_dn_kernel(const float* __restrict__ pool, int C, int Hs, int Ws,
                                                       const int4* __restrict__ par, int B, int PS, float sigma,
                                                       unsigned long long seed, unsigned long long step,
                                                       float* __restrict__ outH, float* __restrict__ outL) {
  const long n = (long)B * C * PS * PS;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int j = (int)(t % PS);
  long r = t / PS;
  const int i = (int)(r % PS);
  r /= PS;
  const int c = (int)(r % C), b = (int)(r / C);
  const int4 pr = par[b];   // x = image, y = rnd_h, z = rnd_w, w = mode
  int si, sj;
  aug_src(pr.w, i, j, PS, si, sj);
  const float h = pool[(((long)pr.x * C + c) * Hs + pr.y + si) * Ws + pr.z + sj];
  outH[t] = h;
  outL[t] = h + sigma * normal_at((unsigned long long)t, seed, step);
}

// DatasetFDnCNN: H = aug(crop(pool)); L = [H + sigma_b * N(0, 1) | sigma_b], sigma_b the float in column scol of
// sample b's parameter row.  One thread per outL element, so both outputs are stored at consecutive addresses by
// consecutive lanes (outH within each channel plane) and the augment's gather stays on the pool read.  The normals'
// counter is the element index of the [B][C][PS][PS] noisy block -- synth_dn_kernel's, whose L an all-equal table
// reproduces bit for bit.  image / rnd_h / rnd_w are clamped into the pool.
template <bool MAP>
__global__ __launch_bounds__(256) void synth_dn_map_kernel(const float* __restrict__ pool, int N, int C, int Hs, int Ws,
                                                           const int* __restrict__ par, int pstride, int scol, int B,
                                                           int PS, unsigned long long seed, unsigned long long step,
                                                           float* __restrict__ outH, float* __restrict__ outL,
                                                           float* __restrict__ outC) {
  // MAP: outL [B][C + 1][PS][PS] with the level map as its last channel (DatasetFDnCNN); otherwise outL
  // [B][C][PS][PS] and the level itself in outC[b] (DatasetFFDNet) -- the same H, normals and levels either way
  const int CL = MAP ? C + 1 : C;
  const long n = (long)B * CL * PS * PS;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int j = (int)(t % PS);
  long r = t / PS;
  const int i = (int)(r % PS);
  r /= PS;
  const int c = (int)(r % CL), b = (int)(r / CL);
  const int* pr = par + (long)b * pstride;   // {image, rnd_h, rnd_w, mode}, ..., [scol] = float bits of sigma_b
  const float sigma = __int_as_float(pr[scol]);
  if (MAP && c == C) {
    outL[t] = sigma;
    return;
  }
  if (!MAP && c == 0 && i == 0 && j == 0) outC[b] = sigma;
  const int img = min(max(pr[0], 0), N - 1), rh = min(max(pr[1], 0), Hs - PS), rw = min(max(pr[2], 0), Ws - PS);
  int si, sj;
  aug_src(pr[3] & 7, i, j, PS, si, sj);
  const float h = pool[(((long)img * C + c) * Hs + rh + si) * Ws + rw + sj];
  const long u = (((long)b * C + c) * PS + i) * PS + j;
  outH[u] = h;
  outL[t] = h + sigma * normal_at((unsigned long long)u, seed, step);
}

long nblocks(long n) { return (n + 255) / 256; }

}  // namespace

extern "C" int kair_synth_sr(const float* pool, int C, int Hs, int Ws, const int* params, int B, int PS, int sf,
                             const float* wh, const int* ih, const float* ww, const int* iw, int P, float* outH,
                             float* outL, void* stream) {
  KAIR_CHECK_ARG(pool && params && wh && ih && ww && iw && outH && outL, "synth_sr: null pointer");
  KAIR_CHECK_ARG(C > 0 && Hs > 0 && Ws > 0 && B > 0 && sf > 0 && PS > 0 && PS % sf == 0 && P > 0,
                 "synth_sr: bad sizes (C %d, %dx%d, B %d, PS %d, sf %d, P %d)", C, Hs, Ws, B, PS, sf, P);
  KAIR_CHECK_ARG(PS <= Hs && PS <= Ws, "synth_sr: pool images smaller than the patch");
  // separable kernel when the staged vertical pass fits in LDS: the horizontal taps of LS L columns
  // span at most PS + 2P source columns (+ 2 sf of rounding slack)
  const int LS = PS / sf;
  const int Wmax = (PS + 2 * P + 2 * sf) < Ws ? (PS + 2 * P + 2 * sf) : Ws;
  // bands of L rows: ~2048 workgroups over the batch (B = 4: one L row per band)
  int nband = 2048 / (B * C);
  nband = nband < 1 ? 1 : (nband > LS ? LS : nband);
  const int rpb = (LS + nband - 1) / nband;
  const size_t lds = (size_t)rpb * Wmax * sizeof(float);
  if (lds <= 60 * 1024) {
    KAIR_LAUNCH(synth_sr_sep_kernel<false>, dim3((unsigned)(B * C * nband)), dim3(256), lds, (hipStream_t)stream, pool,
                0, C, Hs, Ws, (const int4*)params, 1, 0, PS, sf, wh, ih, ww, iw, P, Wmax, nband, 0ull, 0ull, outH, outL);
  } else {
    const long total = (long)B * C * PS * PS + (long)B * C * LS * LS;
    KAIR_LAUNCH(synth_sr_kernel, dim3((unsigned)nblocks(total)), dim3(256), 0, (hipStream_t)stream, pool, C, Hs, Ws,
                       (const int4*)params, B, PS, sf, wh, ih, ww, iw, P, outH, outL);
  }
  KAIR_CHECK_LAUNCH();
  return 0;
}

extern "C" int kair_synth_dn(const float* pool, int C, int Hs, int Ws, const int* params, int B, int PS, float sigma,
                             unsigned long long seed, unsigned long long step, float* outH, float* outL, void* stream) {
  KAIR_CHECK_ARG(pool && params && outH && outL, "synth_dn: null pointer");
  KAIR_CHECK_ARG(C > 0 && B > 0 && PS > 0 && PS <= Hs && PS <= Ws, "synth_dn: bad sizes");
  const long total = (long)B * C * PS * PS;
  KAIR_LAUNCH(synth_dn_kernel, dim3((unsigned)nblocks(total)), dim3(256), 0, (hipStream_t)stream, pool, C, Hs, Ws,
                     (const int4*)params, B, PS, sigma, seed, step, outH, outL);
  KAIR_CHECK_LAUNCH();
  return 0;
}

static int synth_dn_levels(const char* who, bool map, const float* pool, int N, int C, int Hs, int Ws, const int* params,
                           int pstride, int scol, int B, int PS, unsigned long long seed, unsigned long long step,
                           float* outH, float* outL, float* outC, void* stream) {
  KAIR_CHECK_ARG(pool && params && outH && outL && (map || outC), "%s: null pointer", who);
  KAIR_CHECK_ARG(N > 0 && C > 0 && B > 0 && PS > 0 && PS <= Hs && PS <= Ws, "%s: bad sizes", who);
  KAIR_CHECK_ARG(pstride >= 5 && scol >= 4 && scol < pstride, "%s: level column %d outside rows of %d ints", who, scol,
                 pstride);
  const long total = (long)B * (map ? C + 1 : C) * PS * PS;
  KAIR_CHECK_ARG(nblocks(total) < (1L << 31), "%s: too many elements", who);
  if (map)
    KAIR_LAUNCH(synth_dn_map_kernel<true>, dim3((unsigned)nblocks(total)), dim3(256), 0, (hipStream_t)stream, pool, N, C,
                Hs, Ws, params, pstride, scol, B, PS, seed, step, outH, outL, outC);
  else
    KAIR_LAUNCH(synth_dn_map_kernel<false>, dim3((unsigned)nblocks(total)), dim3(256), 0, (hipStream_t)stream, pool, N, C,
                Hs, Ws, params, pstride, scol, B, PS, seed, step, outH, outL, outC);
  KAIR_CHECK_LAUNCH();
  return 0;
}

extern "C" int kair_synth_dn_map(const float* pool, int N, int C, int Hs, int Ws, const int* params, int pstride, int scol,
                                 int B, int PS, unsigned long long seed, unsigned long long step, float* outH,
                                 float* outL, void* stream) {
  return synth_dn_levels("synth_dn_map", true, pool, N, C, Hs, Ws, params, pstride, scol, B, PS, seed, step, outH, outL,
                         nullptr, stream);
}

extern "C" int kair_synth_dn_level(const float* pool, int N, int C, int Hs, int Ws, const int* params, int pstride,
                                   int scol, int B, int PS, unsigned long long seed, unsigned long long step, float* outH,
                                   float* outL, float* outC, void* stream) {
  return synth_dn_levels("synth_dn_level", false, pool, N, C, Hs, Ws, params, pstride, scol, B, PS, seed, step, outH, outL,
                         outC, stream);
}

// DatasetDPSR batches in one launch: kair_synth_sr's crop, augment and both bicubic passes (the banded separable
// kernel, so L's image channels are its bytes), then per sample the level in column scol of its parameter row (rows
// of pstride ints, pstride % 4 == 0; columns 0-3 {image, rnd_h, rnd_w, mode} as kair_synth_sr's), the AWGN (Philox
// keyed by (seed, step), kair_synth_dn_map's convention) and the level plane.  outH [B][C][PS][PS], outL
// [B][C + 1][PS/sf][PS/sf].  wh / ih hold Hs/sf rows of P taps, ww / iw Ws/sf rows.
extern "C" int kair_synth_dpsr(const float* pool, int N, int C, int Hs, int Ws, const int* params, int pstride, int scol,
                               int B, int PS, int sf, const float* wh, const int* ih, const float* ww, const int* iw, int P,
                               unsigned long long seed, unsigned long long step, float* outH, float* outL, void* stream) {
  KAIR_CHECK_ARG(pool && params && wh && ih && ww && iw && outH && outL, "synth_dpsr: null pointer");
  KAIR_CHECK_ARG(N > 0 && C > 0 && Hs > 0 && Ws > 0 && B > 0 && sf > 0 && PS > 0 && PS % sf == 0 && P > 0,
                 "synth_dpsr: bad sizes (N %d, C %d, %dx%d, B %d, PS %d, sf %d, P %d)", N, C, Hs, Ws, B, PS, sf, P);
  KAIR_CHECK_ARG(Hs % sf == 0 && Ws % sf == 0, "synth_dpsr: the pool is not cropped to the scale");
  KAIR_CHECK_ARG(PS <= Hs && PS <= Ws, "synth_dpsr: pool images smaller than the patch");
  KAIR_CHECK_ARG(pstride >= 8 && pstride % 4 == 0 && scol >= 4 && scol < pstride,
                 "synth_dpsr: level column %d outside rows of %d ints (a multiple of 4, >= 8)", scol, pstride);
  KAIR_CHECK_ARG(((uintptr_t)params % 16) == 0, "synth_dpsr: the parameter table is not 16-byte aligned");
  const int LS = PS / sf;
  const int Wmax = (PS + 2 * P + 2 * sf) < Ws ? (PS + 2 * P + 2 * sf) : Ws;
  int nband = 2048 / (B * C);
  nband = nband < 1 ? 1 : (nband > LS ? LS : nband);
  const int rpb = (LS + nband - 1) / nband;
  const size_t lds = (size_t)rpb * Wmax * sizeof(float);
  KAIR_CHECK_ARG(lds <= 60 * 1024, "synth_dpsr: a band of %d L rows x %d columns does not fit the staged pass", rpb, Wmax);
  KAIR_CHECK_ARG((long)B * C * nband < (1L << 31), "synth_dpsr: too many workgroups");
  KAIR_LAUNCH(synth_sr_sep_kernel<true>, dim3((unsigned)(B * C * nband)), dim3(256), lds, (hipStream_t)stream, pool, N, C,
              Hs, Ws, (const int4*)params, pstride / 4, scol, PS, sf, wh, ih, ww, iw, P, Wmax, nband, seed, step, outH,
              outL);
  KAIR_CHECK_LAUNCH();
  return 0;
}
