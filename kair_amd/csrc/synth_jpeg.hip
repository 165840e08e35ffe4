// JPEG CAR training data on the MI355X: the lossy part of a baseline JPEG encode + decode (what cv2.imencode +
// cv2.imdecode do to a patch in DatasetJPEG.__getitem__, data/dataset_jpeg.py:40-96), from an image pool resident
// in HBM.  Entropy coding is lossless and is left out, so the round trip is libjpeg's 32-bit integer arithmetic and
// the result is the decoder's pixels bit for bit (utils/utils_jpeg.py is the host statement of the same numbers).
//
//   kair_jpeg_roundtrip  whole images [N][1 or 3][H][W]: gray JPEG, or RGB as 4:2:0 YCbCr with the h2v2 "fancy"
//                        upsampler; a quality per sample.
//   kair_jpeg_roundtrip_var  the colour round trip of a padded batch [N][3][Hmax][Wmax] whose sample n is the top-left
//                        (h, w) corner, with a quality per sample; quality 0 copies (the blind-SR program,
//                        synth_blindsr.hip, runs a JPEG step on some samples of a batch only).
//   kair_rgb2gray8       the two gray conversions of the loader: MATLAB rgb2ycbcr Y or OpenCV's COLOR_RGB2GRAY.
//   kair_synth_jpeg      a batch of DatasetJPEG items in one launch: (PS + 8)^2 crop, 8-way augment, uint8, gray
//                        conversion, JPEG round trip, second PS^2 crop at an offset in [0, 8] (so the 8 x 8 block grid
//                        does not sit at a fixed phase of the patch), H and L.
//
// A plane is coded in 8 x 8 blocks: edge replication to whole blocks, - 128, jfdctint (rows, then columns), division by
// 8 Q rounding half away from zero, multiplication by Q, jidctint (columns, then rows), + 128, clamp.
//
// Mapping: one lane per 8-sample row (then column, then row) of a block, so a wave holds 8 blocks and a 1-D transform
// is straight-line code on 8 registers.  The three transposes between the four passes go through LDS: a block is 8
// rows of 9 ints (72 per block), so the 64 lanes of a wave touch 64 distinct banks both when they write rows
// (bank 8 blk + 9 r + k) and when they read columns (8 blk + c + 9 k).  The quantiser divides with the integer
// division (divisor <= 2040): exact by construction.
//
// Gray: blocks are independent; a workgroup of 256 threads takes 32 blocks and writes its pixels straight to the
// outputs.  Colour needs the decoded chroma of the neighbouring blocks for the upsampler, so the planes are decoded
// first: for a training patch into LDS by one 1024-thread workgroup per sample (a 134^2 patch: 29 KB of planes), for
// whole images into the caller's workspace by the block-parallel grid and a second launch for the pixels.
#include "synth_common.h"

namespace {

__constant__ unsigned char kLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                        14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                        18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                        49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
__constant__ unsigned char kChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                          24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// FIX(x) = round(x 2^13) of jfdctint.c / jidctint.c
constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
              F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

KAIR_DEV int ds(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// the odd part both transforms share: (t4, t5, t6, t7) -> the four rotated sums
KAIR_DEV void dct_odd(int& t4, int& t5, int& t6, int& t7) {
  int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F1175;
  t4 *= F0298; t5 *= F2053; t6 *= F3072; t7 *= F1501;
  z1 *= -F0899; z2 *= -F2562;
  z3 = z3 * -F1961 + z5;
  z4 = z4 * -F0390 + z5;
  t4 += z1 + z3; t5 += z2 + z4; t6 += z2 + z3; t7 += z1 + z4;
}

template <bool FIRST> KAIR_DEV void fdct_pass(int (&d)[8]) {
  constexpr int n = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
  int t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) << 2 : ds(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) << 2 : ds(t10 - t11, 2);
  const int z1 = (t12 + t13) * F0541;
  d[2] = ds(z1 + t13 * F0765, n);
  d[6] = ds(z1 - t12 * F1847, n);
  dct_odd(t4, t5, t6, t7);
  d[7] = ds(t4, n); d[5] = ds(t5, n); d[3] = ds(t6, n); d[1] = ds(t7, n);
}

template <bool FIRST> KAIR_DEV void idct_pass(int (&d)[8]) {
  constexpr int n = FIRST ? 11 : 18;
  const int z1 = (d[2] + d[6]) * F0541;
  const int e2 = z1 - d[6] * F1847, e3 = z1 + d[2] * F0765;
  const int e0 = (d[0] + d[4]) << 13, e1 = (d[0] - d[4]) << 13;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
  dct_odd(t0, t1, t2, t3);
  d[0] = ds(t10 + t3, n); d[7] = ds(t10 - t3, n);
  d[1] = ds(t11 + t2, n); d[6] = ds(t11 - t2, n);
  d[2] = ds(t12 + t1, n); d[5] = ds(t12 - t1, n);
  d[3] = ds(t13 + t0, n); d[4] = ds(t13 - t0, n);
}

KAIR_DEV int clamp8(int v) { return min(max(v, 0), 255); }

struct JpegArgs {
  const float* src;    // [N][C][Hs][Ws]
  int N, C, Hs, Ws;
  const int* par;      // synth: per sample {image, rnd_h, rnd_w, mode, gray_mode, quality, rh2, rw2}; null: whole images
  int pstride;
  const int* quality;  // whole images: per sample at stride qstride
  int qstride;
  int PH, PW;          // the coded image: the (PS + 8)^2 patch, or Hs x Ws
  int PS;              // synth: side of the second crop
  int color;           // RGB coded as 4:2:0 YCbCr (C == 3)
  int bw0, nb0, bw1, nb1, nblk;   // blocks per row / per plane of the luma and chroma planes, blocks per sample
  int gps;             // block-parallel kernels: workgroups per sample
  float* outH;         // synth: the uncompressed crop
  float* outL;
  unsigned char* ws;   // whole colour images: decoded planes, plane_bytes per sample
  long plane_bytes;
};

struct JpegGeo {
  const float* img;   // channel 0 of the sample's image, at the crop's corner
  int mode, gray_mode, q, rh2, rw2;
};

KAIR_DEV JpegGeo jpeg_geo(const JpegArgs& a, int b) {
  JpegGeo g{};
  int image = b, y0 = 0, x0 = 0;
  if (a.par) {
    const int* p = a.par + (long)b * a.pstride;
    image = min(max(p[0], 0), a.N - 1);
    y0 = min(max(p[1], 0), a.Hs - a.PH);
    x0 = min(max(p[2], 0), a.Ws - a.PW);
    g.mode = p[3] & 7;
    g.gray_mode = p[4] != 0;
    g.q = p[5];
    g.rh2 = min(max(p[6], 0), 8);
    g.rw2 = min(max(p[7], 0), 8);
  } else {
    g.q = a.quality[(long)b * a.qstride];
  }
  g.q = min(max(g.q, 1), 100);
  g.img = a.src + ((long)image * a.C * a.Hs + y0) * a.Ws + x0;
  return g;
}

// uint8 sample of channel c at (i, j) of the coded image (the augmented crop, or the image itself)
KAIR_DEV int src8(const JpegArgs& a, const JpegGeo& g, int c, int i, int j) {
  int si = i, sj = j;
  if (a.par) aug_src(g.mode, i, j, a.PH, si, sj);
  const float v = g.img[((long)c * a.Hs + si) * a.Ws + sj];
  return (int)rintf(255.f * fminf(fmaxf(v, 0.f), 1.f));
}

// mode 0: utils_image.rgb2ycbcr(only_y) on the uint8 triple, round((65.481 R + 128.553 G + 24.966 B) / 255 + 16) in
// thousandths (an exact tie rounds up); mode 1: OpenCV's COLOR_RGB2GRAY
KAIR_DEV int gray_of(int mode, int R, int G, int B) {
  return mode == 0 ? 16 + (65481 * R + 128553 * G + 24966 * B + 127500) / 255000
                   : (4899 * R + 9617 * G + 1868 * B + 8192) >> 14;
}

KAIR_DEV int gray8(const JpegArgs& a, const JpegGeo& g, int i, int j) {
  if (a.C == 1) return src8(a, g, 0, i, j);
  return gray_of(g.gray_mode ? 1 : 0, src8(a, g, 0, i, j), src8(a, g, 1, i, j), src8(a, g, 2, i, j));
}

// sample (i, j) of plane pl over the padded block grid.  Gray and luma: edge replication.  Chroma: rows replicate
// the last downsampled row; a column past the image averages the replicated RGB columns with the bias of its own
// parity (libjpeg pads the full-resolution row to whole MCUs before it downsamples, and the bias alternates by column)
KAIR_DEV int plane_px(const JpegArgs& a, const JpegGeo& g, int pl, int i, int j) {
  if (!a.color) return gray8(a, g, min(i, a.PH - 1), min(j, a.PW - 1));
  if (pl == 0) {
    const int y = min(i, a.PH - 1), x = min(j, a.PW - 1);
    return (19595 * src8(a, g, 0, y, x) + 38470 * src8(a, g, 1, y, x) + 7471 * src8(a, g, 2, y, x) + 32768) >> 16;
  }
  i = min(i, (a.PH + 1) / 2 - 1);
  int sum = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int y = min(2 * i + (e >> 1), a.PH - 1), x = min(2 * j + (e & 1), a.PW - 1);
    const int R = src8(a, g, 0, y, x), G = src8(a, g, 1, y, x), B = src8(a, g, 2, y, x);
    sum += pl == 1 ? (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
                   : (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
  }
  return (sum + 1 + (j & 1)) >> 2;
}

// quantiser steps of quality q: sQ[0][64] luma, sQ[1][64] chroma (threads 0..127)
KAIR_DEV void make_tables(int q, int* sQ, int tid) {
  if (tid < 128) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int base = tid < 64 ? kLuma[tid] : kChroma[tid - 64];
    sQ[tid] = min(max((base * s + 50) / 100, 1), 255);
  }
}

// Block rows t in [t0, t1) of sample b (t = 8 block + row; blocks of plane 0, then 1, then 2) through the codec.
// Every thread of the workgroup calls this with the same range.  sT: 9 ints per thread.  The decoded row of 8 goes
// to sink(pl, i, j0, v, s): v the decoded samples, s the source samples, of row i, columns j0 .. j0 + 7 of plane pl.
template <typename Sink>
KAIR_DEV void code_blocks(const JpegArgs& a, const JpegGeo& g, const int* sQ, int* sT, int t0, int t1, Sink sink) {
  const int tid = threadIdx.x, nt = blockDim.x;
  int* blk = sT + (tid >> 3) * 72;
  const int r = tid & 7;
  for (int base = t0; base < t1; base += nt) {
    const int t = base + tid;
    const bool on = t < t1;
    int id = on ? t >> 3 : 0, pl = 0;
    if (id >= a.nb0) {
      id -= a.nb0;
      pl = 1;
      if (id >= a.nb1) { id -= a.nb1; pl = 2; }
    }
    const int bw = pl ? a.bw1 : a.bw0;
    const int by = id / bw, bx = id - by * bw;
    int d[8], s[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s[k] = on ? plane_px(a, g, pl, by * 8 + r, bx * 8 + k) : 128;
      d[k] = s[k] - 128;
    }
    fdct_pass<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) blk[r * 9 + k] = d[k];
    __syncthreads();
    // this lane now holds column r of its block
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = blk[k * 9 + r];
    fdct_pass<false>(d);
    const int* Q = sQ + (pl ? 64 : 0);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int q = Q[k * 8 + r], dv = q << 3;
      const int m = (abs(d[k]) + (dv >> 1)) / dv;
      d[k] = (d[k] < 0 ? -m : m) * q;
    }
    idct_pass<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) blk[k * 9 + r] = d[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = blk[r * 9 + k];
    idct_pass<false>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = clamp8(d[k] + 128);
    if (on) sink(pl, by * 8 + r, bx * 8, d, s);
  }
}

// pixel (i, j) of the decoded colour image from the decoded planes (row strides 8 bw0 / 8 bw1): h2v2 fancy
// upsampling of the chroma cropped to ceil(PH / 2) x ceil(PW / 2), then YCbCr -> RGB
KAIR_DEV void color_px(const JpegArgs& a, const unsigned char* p0, const unsigned char* p1, const unsigned char* p2, int i,
                       int j, int (&rgb)[3]) {
  const int ch = (a.PH + 1) / 2, cw = (a.PW + 1) / 2, cs = a.bw1 * 8;
  const int ci = i >> 1, cj = j >> 1;
  const int ni = (i & 1) ? min(ci + 1, ch - 1) : max(ci - 1, 0);
  const int nj = (j & 1) ? min(cj + 1, cw - 1) : max(cj - 1, 0);
  const int rnd = (j & 1) ? 7 : 8;
  int c[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const unsigned char* p = e ? p2 : p1;
    const int here = 3 * p[ci * cs + cj] + p[ni * cs + cj], side = 3 * p[ci * cs + nj] + p[ni * cs + nj];
    c[e] = ((3 * here + side + rnd) >> 4) - 128;
  }
  const int y = p0[i * (a.bw0 * 8) + j];
  rgb[0] = clamp8(y + ((91881 * c[1] + 32768) >> 16));
  rgb[1] = clamp8(y + ((-22554 * c[0] - 46802 * c[1] + 32768) >> 16));
  rgb[2] = clamp8(y + ((116130 * c[0] + 32768) >> 16));
}

// block counts of a PH x PW image; false when the block rows of a sample do not fit an int
__host__ __device__ inline bool jpeg_layout(JpegArgs& a) {
  const long bh0 = (a.PH + 7) / 8, bw0 = (a.PW + 7) / 8;
  const long bh1 = ((a.PH + 1) / 2 + 7) / 8, bw1 = ((a.PW + 1) / 2 + 7) / 8;
  const long nb0 = bh0 * bw0, nb1 = a.color ? bh1 * bw1 : 0, nblk = nb0 + 2 * nb1;
  if (nblk * 64 >= (1L << 31)) return false;
  a.bw0 = (int)bw0; a.nb0 = (int)nb0; a.bw1 = (int)bw1; a.nb1 = (int)nb1; a.nblk = (int)nblk;
  a.gps = (int)((nblk * 8 + 255) / 256);
  a.plane_bytes = nblk * 64;
  return true;
}

// block rows [t0, t1) of a colour sample decoded into its workspace w: plane 0, then 1, then 2, whole blocks
KAIR_DEV void planes_to_ws(const JpegArgs& a, const JpegGeo& g, const int* sQ, int* sT, int t0, int t1, unsigned char* w) {
  const long o1 = (long)a.nb0 * 64, o2 = o1 + (long)a.nb1 * 64;
  code_blocks(a, g, sQ, sT, t0, t1, [&](int pl, int i, int j0, const int (&v)[8], const int (&)[8]) {
    unsigned char* row = w + (pl == 0 ? 0 : pl == 1 ? o1 : o2) + (long)i * ((pl ? a.bw1 : a.bw0) * 8) + j0;
    *reinterpret_cast<uint2*>(row) = make_uint2(v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24,
                                                v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24);
  });
}

// gray (a.color == 0): grid = samples x gps workgroups of 256 threads = 32 blocks each; pixels go straight out.
// whole colour images (a.ws): the same grid decodes the three planes into the workspace.
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(const JpegArgs a) {
  __shared__ int sQ[128];
  __shared__ int sT[32 * 72];
  const int b = blockIdx.x / a.gps, grp = blockIdx.x - b * a.gps;
  const JpegGeo g = jpeg_geo(a, b);
  make_tables(g.q, sQ, threadIdx.x);
  __syncthreads();
  const int t0 = grp * 256, t1 = min(a.nblk * 8, t0 + 256);
  if (a.color) {
    planes_to_ws(a, g, sQ, sT, t0, t1, a.ws + (long)b * a.plane_bytes);
    return;
  }
  if (a.par) {
    float* oH = a.outH + (long)b * a.PS * a.PS;
    float* oL = a.outL + (long)b * a.PS * a.PS;
    code_blocks(a, g, sQ, sT, t0, t1, [&](int, int i, int j0, const int (&v)[8], const int (&s)[8]) {
      const int oi = i - g.rh2;
      if (oi < 0 || oi >= a.PS) return;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int oj = j0 + k - g.rw2;
        if (oj >= 0 && oj < a.PS) {
          oH[oi * a.PS + oj] = (float)s[k] / 255.f;
          oL[oi * a.PS + oj] = (float)v[k] / 255.f;
        }
      }
    });
  } else {
    float* o = a.outL + (long)b * a.PH * a.PW;
    code_blocks(a, g, sQ, sT, t0, t1, [&](int, int i, int j0, const int (&v)[8], const int (&)[8]) {
      if (i >= a.PH) return;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (j0 + k < a.PW) o[(long)i * a.PW + j0 + k] = (float)v[k] / 255.f;
    });
  }
}

// whole colour images, second launch: one thread per pixel of [N][PH][PW]
__global__ __launch_bounds__(256) void jpeg_color_finish_kernel(const JpegArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x, hw = (long)a.PH * a.PW;
  if (t >= a.N * hw) return;
  const int n = (int)(t / hw);
  const long p = t - n * hw;
  const int i = (int)(p / a.PW), j = (int)(p - (long)i * a.PW);
  const unsigned char* w = a.ws + (long)n * a.plane_bytes;
  int rgb[3];
  color_px(a, w, w + (long)a.nb0 * 64, w + (long)(a.nb0 + a.nb1) * 64, i, j, rgb);
#pragma unroll
  for (int c = 0; c < 3; ++c) a.outL[((long)n * 3 + c) * hw + p] = (float)rgb[c] / 255.f;
}

// colour training patches: one workgroup per sample, decoded planes in LDS, then the PS^2 crop of H and L
constexpr int JPEG_CT = 1024;
__global__ __launch_bounds__(JPEG_CT) void jpeg_synth_color_kernel(const JpegArgs a) {
  extern __shared__ int smem[];
  int* sQ = smem;                    // [128]
  int* sT = smem + 128;              // [JPEG_CT / 8][72]
  unsigned char* pl0 = reinterpret_cast<unsigned char*>(sT + (JPEG_CT / 8) * 72);
  unsigned char* pl1 = pl0 + a.nb0 * 64;
  unsigned char* pl2 = pl1 + a.nb1 * 64;
  const int b = blockIdx.x, tid = threadIdx.x;
  const JpegGeo g = jpeg_geo(a, b);
  make_tables(g.q, sQ, tid);
  __syncthreads();
  code_blocks(a, g, sQ, sT, 0, a.nblk * 8, [&](int pl, int i, int j0, const int (&v)[8], const int (&)[8]) {
    unsigned char* row = (pl == 0 ? pl0 : pl == 1 ? pl1 : pl2) + i * ((pl ? a.bw1 : a.bw0) * 8) + j0;
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = (unsigned char)v[k];
  });
  __syncthreads();
  const int n = a.PS * a.PS;
  float* oH = a.outH + (long)b * 3 * n;
  float* oL = a.outL + (long)b * 3 * n;
  for (int t = tid; t < n; t += JPEG_CT) {
    const int oi = t / a.PS, oj = t - oi * a.PS;
    const int i = oi + g.rh2, j = oj + g.rw2;
    int rgb[3];
    color_px(a, pl0, pl1, pl2, i, j, rgb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      oH[c * n + t] = (float)src8(a, g, c, i, j) / 255.f;
      oL[c * n + t] = (float)rgb[c] / 255.f;
    }
  }
}

__global__ __launch_bounds__(256) void rgb2gray8_kernel(const float* __restrict__ x, long n, long hw, int mode,
                                                        float* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const long img = t / hw, p = t - img * hw;
  const float* s = x + img * 3 * hw + p;
  int c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = (int)rintf(255.f * fminf(fmaxf(s[k * hw], 0.f), 1.f));
  out[t] = (float)gray_of(mode, c[0], c[1], c[2]) / 255.f;
}

// kair_jpeg_roundtrip_var: the arguments with sample b's own (h, w) and block layout (the workspace stride and the grid
// stay those of the padded size); false: quality 0, the sample is copied
KAIR_DEV bool jpeg_var_sample(const JpegArgs& a, const int* hw, int hwstride, int b, JpegArgs& s) {
  s = a;
  s.PH = min(max(hw[(long)b * hwstride], 1), a.Hs);
  s.PW = min(max(hw[(long)b * hwstride + 1], 1), a.Ws);
  jpeg_layout(s);
  s.gps = a.gps;
  s.plane_bytes = a.plane_bytes;
  return a.quality[(long)b * a.qstride] > 0;
}

__global__ __launch_bounds__(256) void jpeg_var_blocks_kernel(const JpegArgs a, const int* __restrict__ hw, int hwstride) {
  __shared__ int sQ[128];
  __shared__ int sT[32 * 72];
  const int b = blockIdx.x / a.gps, grp = blockIdx.x - b * a.gps;
  JpegArgs s;
  if (!jpeg_var_sample(a, hw, hwstride, b, s)) return;   // uniform per workgroup, as is the next test
  const int t0 = grp * 256, t1 = min(s.nblk * 8, t0 + 256);
  if (t0 >= t1) return;
  const JpegGeo g = jpeg_geo(s, b);
  make_tables(g.q, sQ, threadIdx.x);
  __syncthreads();
  planes_to_ws(s, g, sQ, sT, t0, t1, a.ws + (long)b * a.plane_bytes);
}

// one thread per pixel of [N][Hmax][Wmax]; pixels outside a sample's (h, w) are left alone
__global__ __launch_bounds__(256) void jpeg_var_finish_kernel(const JpegArgs a, const int* __restrict__ hw, int hwstride) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x, plane = (long)a.Hs * a.Ws;
  if (t >= a.N * plane) return;
  const int n = (int)(t / plane);
  const long p = t - n * plane;
  const int i = (int)(p / a.Ws), j = (int)(p - (long)i * a.Ws);
  JpegArgs s;
  const bool coded = jpeg_var_sample(a, hw, hwstride, n, s);
  if (i >= s.PH || j >= s.PW) return;
  const long o = (long)n * 3 * plane + p;
  if (!coded) {
    if (a.outL == a.src) return;   // in place: nothing to do
#pragma unroll
    for (int c = 0; c < 3; ++c) a.outL[o + c * plane] = a.src[o + c * plane];
    return;
  }
  const unsigned char* w = a.ws + (long)n * a.plane_bytes;
  int rgb[3];
  color_px(s, w, w + (long)s.nb0 * 64, w + (long)(s.nb0 + s.nb1) * 64, i, j, rgb);
#pragma unroll
  for (int c = 0; c < 3; ++c) a.outL[o + c * plane] = (float)rgb[c] / 255.f;
}

constexpr long JPEG_LDS_BYTES = 150 * 1024;   // of CDNA4's 160 KB per workgroup

}  // namespace

extern "C" long kair_jpeg_workspace_bytes(int N, int C, int H, int W) {
  if (C != 3 || N <= 0 || H <= 0 || W <= 0) return 0;
  JpegArgs a{};
  a.PH = H; a.PW = W; a.color = 1;
  return jpeg_layout(a) ? a.plane_bytes * N : -1;
}

extern "C" int kair_jpeg_roundtrip(const float* x, int N, int C, int H, int W, const int* quality, int qstride, float* out,
                                   void* workspace, void* stream) {
  KAIR_CHECK_ARG(x && quality && out, "jpeg_roundtrip: null pointer");
  KAIR_CHECK_ARG((C == 1 || C == 3) && N > 0 && H > 0 && W > 0 && qstride >= 0,
                 "jpeg_roundtrip: bad sizes (N %d, C %d, %dx%d, qstride %d)", N, C, H, W, qstride);
  KAIR_CHECK_ARG(C == 1 || W >= 5, "jpeg_roundtrip: colour images need a width of at least 5 (got %d)", W);
  KAIR_CHECK_ARG(C == 1 || workspace, "jpeg_roundtrip: colour images need the workspace (kair_jpeg_workspace_bytes)");
  JpegArgs a{};
  a.src = x; a.N = N; a.C = C; a.Hs = H; a.Ws = W;
  a.quality = quality; a.qstride = qstride;
  a.PH = H; a.PW = W; a.color = C == 3;
  a.outL = out; a.ws = (unsigned char*)workspace;
  KAIR_CHECK_ARG(jpeg_layout(a) && (long)N * a.gps < (1L << 31) && ((long)N * H * W + 255) / 256 < (1L << 31),
                 "jpeg_roundtrip: too many workgroups");
  hipStream_t s = (hipStream_t)stream;
  KAIR_LAUNCH(jpeg_blocks_kernel, dim3((unsigned)((long)N * a.gps)), dim3(256), 0, s, a);
  KAIR_CHECK_LAUNCH();
  if (a.color) {
    KAIR_LAUNCH(jpeg_color_finish_kernel, dim3((unsigned)(((long)N * H * W + 255) / 256)), dim3(256), 0, s, a);
    KAIR_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int kair_jpeg_roundtrip_var(const float* x, int N, int Hmax, int Wmax, const int* hw, int hwstride, int w_min,
                                       const int* quality, int qstride, float* out, void* workspace, void* stream) {
  KAIR_CHECK_ARG(x && hw && quality && out && workspace, "jpeg_roundtrip_var: null pointer");
  KAIR_CHECK_ARG(N > 0 && Hmax > 0 && Wmax > 0 && hwstride >= 2 && qstride >= 0,
                 "jpeg_roundtrip_var: bad sizes (N %d, buffer %dx%d, hwstride %d, qstride %d)", N, Hmax, Wmax, hwstride,
                 qstride);
  KAIR_CHECK_ARG(w_min >= 5 && w_min <= Wmax,
                 "jpeg_roundtrip_var: colour images need a width of at least 5 (the caller's lower bound is %d)", w_min);
  JpegArgs a{};
  a.src = x; a.N = N; a.C = 3; a.Hs = Hmax; a.Ws = Wmax;
  a.quality = quality; a.qstride = qstride;
  a.PH = Hmax; a.PW = Wmax; a.color = 1;
  a.outL = out; a.ws = (unsigned char*)workspace;
  KAIR_CHECK_ARG(jpeg_layout(a) && (long)N * a.gps < (1L << 31) && ((long)N * Hmax * Wmax + 255) / 256 < (1L << 31),
                 "jpeg_roundtrip_var: too many workgroups");
  hipStream_t s = (hipStream_t)stream;
  KAIR_LAUNCH(jpeg_var_blocks_kernel, dim3((unsigned)((long)N * a.gps)), dim3(256), 0, s, a, hw, hwstride);
  KAIR_CHECK_LAUNCH();
  KAIR_LAUNCH(jpeg_var_finish_kernel, dim3((unsigned)(((long)N * Hmax * Wmax + 255) / 256)), dim3(256), 0, s, a, hw,
              hwstride);
  KAIR_CHECK_LAUNCH();
  return 0;
}

extern "C" int kair_rgb2gray8(const float* x, int N, int H, int W, int mode, float* out, void* stream) {
  KAIR_CHECK_ARG(x && out, "rgb2gray8: null pointer");
  KAIR_CHECK_ARG(N > 0 && H > 0 && W > 0 && (mode == 0 || mode == 1), "rgb2gray8: bad sizes (N %d, %dx%d, mode %d)", N, H,
                 W, mode);
  const long hw = (long)H * W, n = N * hw;
  KAIR_CHECK_ARG((n + 255) / 256 < (1L << 31), "rgb2gray8: too many elements");
  KAIR_LAUNCH(rgb2gray8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, hw, mode, out);
  KAIR_CHECK_LAUNCH();
  return 0;
}

extern "C" int kair_synth_jpeg(const float* pool, int N, int C, int Hs, int Ws, const int* params, int pstride, int B,
                               int PS, int is_color, float* outH, float* outL, void* stream) {
  KAIR_CHECK_ARG(pool && params && outH && outL, "synth_jpeg: null pointer");
  KAIR_CHECK_ARG((C == 1 || C == 3) && N > 0 && Hs > 0 && Ws > 0 && B > 0 && PS > 0 && PS < (1 << 20) && pstride >= 8,
                 "synth_jpeg: bad sizes (N %d, C %d, %dx%d, B %d, PS %d, pstride %d)", N, C, Hs, Ws, B, PS, pstride);
  KAIR_CHECK_ARG(!is_color || C == 3, "synth_jpeg: a colour batch needs a 3-channel pool");
  KAIR_CHECK_ARG(PS + 8 <= Hs && PS + 8 <= Ws, "synth_jpeg: pool images smaller than the patch + 8 (%d)", PS + 8);
  JpegArgs a{};
  a.src = pool; a.N = N; a.C = C; a.Hs = Hs; a.Ws = Ws;
  a.par = params; a.pstride = pstride;
  a.PH = PS + 8; a.PW = PS + 8; a.PS = PS; a.color = is_color != 0;
  a.outH = outH; a.outL = outL;
  KAIR_CHECK_ARG(jpeg_layout(a) && (long)B * a.gps < (1L << 31), "synth_jpeg: too many workgroups");
  hipStream_t s = (hipStream_t)stream;
  if (a.color) {
    const long lds = (128 + (JPEG_CT / 8) * 72) * (long)sizeof(int) + a.plane_bytes;
    KAIR_CHECK_ARG(lds <= JPEG_LDS_BYTES, "synth_jpeg: the decoded planes of a colour %d-px patch do not fit in LDS", PS + 8);
    KAIR_LAUNCH(jpeg_synth_color_kernel, dim3((unsigned)B), dim3(JPEG_CT), (size_t)lds, s, a);
  } else {
    KAIR_LAUNCH(jpeg_blocks_kernel, dim3((unsigned)((long)B * a.gps)), dim3(256), 0, s, a);
  }
  KAIR_CHECK_LAUNCH();
  return 0;
}
