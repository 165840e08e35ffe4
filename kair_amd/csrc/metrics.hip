// Evaluation metrics on gfx950 with the uint8 semantics of utils_image.py (tensor2uint -> calculate_psnr /
// calculate_ssim, optionally on the Y channel of rgb2ycbcr): per image the exact sum of squared differences of the
// quantised values and the mean SSIM of the quantised 0..255 planes.  Not the SSIM loss of ssim.hip: the window runs
// over the fully overlapping region only (no padding), the data range is 255 and the input is quantised first.
//   q = rintf(__fmul_rn(clamp(x, 0, 1), 255.f))                  (tensor2uint: fp32 product, half to even)
//   Y = 16 + round_half_even((65481 r + 128553 g + 24966 b) / 255000), integer quotient and remainder
//   S = (2 m1 m2 + C1)(2 s12 + C2) / ((m1^2 + m2^2 + C1)(s11 + s22 + C2)),  C1 = 2.55^2, C2 = 7.65^2
// One launch over 32 x 32 tiles of the cropped region of one plane (a channel, or the Y plane built from the three
// channels) + a one-workgroup sum:
//   ssim:   quantised E and H tiles with a 5-pixel reach in LDS as bytes (42 x 42, 0 outside the cropped region) ->
//           rows pass (11 taps, 42 rows x 32 columns of the five moment maps) -> columns pass (each thread 4 consecutive
//           rows of one column, ssim.hip's scheme) -> S at the pixels that are valid window centres (the window inside
//           the region) -> the tile's integer SSE and its sum of S to its own workspace slot;
//   sse:    without KAIR_METRIC_SSIM no filter runs: the same tiles, read straight from memory, SSE only;
//   final:  per image, the slots added in a fixed order (no atomics: repeated calls are bit-identical), the SSIM sum
//           divided by planes x valid centres.
// Arithmetic.  The moments are differences of numbers near 255^2 = 65025 against C2 = 58.5: in fp32 E[x^2] - mu^2 of
// a flat region carries 65025 * 2^-24 = 4e-3 of absolute error, far above the 1e-6 the metric is held to against the
// float64 host path.  The five moments, the map and every sum are fp64; the taps are the float64 window of
// utils_image._gauss_window (ssim.hip's fp32 table is 3e-8 off per tap, so it is not shared).  The SSE is integer.
// LDS: 5 maps x 42 x 32 x 8 B = 53760 B + the byte tiles + the reduction rows = 61.4 KB static.  Both passes index
// consecutive lanes to consecutive columns: a half-wave's ds_read_b64 covers 64 consecutive dwords, one bank row.
#include "common.h"

namespace {

constexpr int TS = 32, HALO = 5, TW = TS + 2 * HALO, WIN = 2 * HALO + 1;
constexpr double MET_K1 = 0.01 * 255, MET_K2 = 0.03 * 255;
constexpr double MET_C1 = MET_K1 * MET_K1, MET_C2 = MET_K2 * MET_K2;

// exp(-x^2 / (2 * 1.5^2)), x = -5 .. 5, normalised to sum 1 in double: utils_image._gauss_window's 1-D factor
#define KAIR_METRIC_TAPS                                                                                    \
  {0.00102838008447911, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002, 0.2130055377112537, \
   0.26601172486179436, 0.2130055377112537, 0.10936068950970002, 0.03600077212843083, 0.007598758135239185, \
   0.00102838008447911}

struct Slot {
  unsigned long long sse;
  double ssum;
};
static_assert(sizeof(Slot) == 16, "one 16-byte workspace slot per tile");

KAIR_DEV int quantise(float x) { return (int)rintf(__fmul_rn(fminf(fmaxf(x, 0.f), 1.f), 255.f)); }

// 16 + round_half_even(N / 255000): N <= 255 * 219000 fits an int
KAIR_DEV int luma(int r, int g, int b) {
  const int N = 65481 * r + 128553 * g + 24966 * b;
  int q = N / 255000;
  const int rem = N - q * 255000;
  q += (rem > 127500 || (rem == 127500 && (q & 1))) ? 1 : 0;
  return 16 + q;
}

// the quantised value of one pixel of a plane: p the plane (Y: the R plane of the image), hw the plane stride
template <bool Y> KAIR_DEV int load_q(const float* __restrict__ p, long hw, long o) {
  if constexpr (Y) return luma(quantise(p[o]), quantise(p[o + hw]), quantise(p[o + 2 * hw]));
  else return quantise(p[o]);
}

// both block sums in one tree; the totals are returned to every thread and the rows may be reused afterwards
KAIR_DEV void block_sum256(double& s, unsigned long long& q, double* rs, unsigned long long* rq) {
  rs[threadIdx.x] = s, rq[threadIdx.x] = q;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) rs[threadIdx.x] += rs[threadIdx.x + o], rq[threadIdx.x] += rq[threadIdx.x + o];
    __syncthreads();
  }
  s = rs[0], q = rq[0];
  __syncthreads();
}

KAIR_DEV long slot_index() { return ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }

// grid (tiles x, tiles y, B * planes) over the cropped region Hr x Wr at offset `border` of the Hh x Ww planes
template <bool Y>
__global__ __launch_bounds__(256) void metrics_ssim_kernel(const float* __restrict__ E, const float* __restrict__ H,
                                                           Slot* __restrict__ part, int Hh, int Ww, int border, int Hr,
                                                           int Wr) {
  __shared__ unsigned char sE[TW * TW], sH[TW * TW];
  __shared__ double hm[5][TW * TS];
  __shared__ double rs[256];
  __shared__ unsigned long long rq[256];
  constexpr double g[WIN] = KAIR_METRIC_TAPS;
  const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
  const long hw = (long)Hh * Ww, base = (long)blockIdx.z * (Y ? 3 : 1) * hw;
  for (int i = threadIdx.x; i < TW * TW; i += 256) {
    const int r = i / TW, c = i - r * TW;
    const int y = y0 + r - HALO, x = x0 + c - HALO;   // region coordinates
    int e = 0, h = 0;
    if (y >= 0 && y < Hr && x >= 0 && x < Wr) {
      const long o = (long)(y + border) * Ww + (x + border);
      e = load_q<Y>(E + base, hw, o), h = load_q<Y>(H + base, hw, o);
    }
    sE[i] = (unsigned char)e, sH[i] = (unsigned char)h;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TW * TS; i += 256) {
    const int r = i / TS, x = i - r * TS;
    double m1 = 0., m2 = 0., m11 = 0., m22 = 0., m12 = 0.;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
      const double e = (double)sE[r * TW + x + k], h = (double)sH[r * TW + x + k];
      const double ge = g[k] * e, gh = g[k] * h;
      m1 += ge;
      m2 += gh;
      m11 = fma(ge, e, m11);
      m22 = fma(gh, h, m22);
      m12 = fma(ge, h, m12);
    }
    hm[0][i] = m1, hm[1][i] = m2, hm[2][i] = m11, hm[3][i] = m22, hm[4][i] = m12;
  }
  __syncthreads();
  const int tx = threadIdx.x & 31, yg = threadIdx.x >> 5;
  double m[5][4];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    double v[4 + WIN - 1];
#pragma unroll
    for (int j = 0; j < 4 + WIN - 1; ++j) v[j] = hm[q][(4 * yg + j) * TS + tx];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = 0.;
#pragma unroll
      for (int k = 0; k < WIN; ++k) s = fma(g[k], v[j + k], s);
      m[q][j] = s;
    }
  }
  double ssum = 0.;
  unsigned long long sse = 0;
  const int x = x0 + tx;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = y0 + 4 * yg + j;
    if (y < Hr && x < Wr) {
      const int si = (4 * yg + j + HALO) * TW + tx + HALO;
      const int d = (int)sE[si] - (int)sH[si];
      sse += (unsigned long long)(d * d);
    }
    if (y >= HALO && y < Hr - HALO && x >= HALO && x < Wr - HALO) {   // the window lies inside the region
      const double m1 = m[0][j], m2 = m[1][j];
      const double m1s = m1 * m1, m2s = m2 * m2, m1m2 = m1 * m2;
      const double s11 = m[2][j] - m1s, s22 = m[3][j] - m2s, s12 = m[4][j] - m1m2;
      ssum += ((2. * m1m2 + MET_C1) * (2. * s12 + MET_C2)) / ((m1s + m2s + MET_C1) * (s11 + s22 + MET_C2));
    }
  }
  block_sum256(ssum, sse, rs, rq);
  if (threadIdx.x == 0) part[slot_index()] = Slot{sse, ssum};
}

// the same tiles without the filter: SSE only
template <bool Y>
__global__ __launch_bounds__(256) void metrics_sse_kernel(const float* __restrict__ E, const float* __restrict__ H,
                                                          Slot* __restrict__ part, int Hh, int Ww, int border, int Hr,
                                                          int Wr) {
  __shared__ double rs[256];
  __shared__ unsigned long long rq[256];
  const int tx = threadIdx.x & 31, yg = threadIdx.x >> 5;
  const int x = blockIdx.x * TS + tx;
  const long hw = (long)Hh * Ww, base = (long)blockIdx.z * (Y ? 3 : 1) * hw;
  unsigned long long sse = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = blockIdx.y * TS + 4 * yg + j;
    if (y < Hr && x < Wr) {
      const long o = (long)(y + border) * Ww + (x + border);
      const int d = load_q<Y>(E + base, hw, o) - load_q<Y>(H + base, hw, o);
      sse += (unsigned long long)(d * d);
    }
  }
  double zero = 0.;
  block_sum256(zero, sse, rs, rq);
  if (threadIdx.x == 0) part[slot_index()] = Slot{sse, 0.};
}

// one workgroup: image b's slots [b * per_image, (b + 1) * per_image) in a fixed order; out [B][2]
__global__ __launch_bounds__(256) void metrics_final_kernel(const Slot* __restrict__ part, long per_image, int B,
                                                            double centres, int want_ssim, double* __restrict__ out) {
  __shared__ double rs[256];
  __shared__ unsigned long long rq[256];
  for (int b = 0; b < B; ++b) {
    double s = 0.;
    unsigned long long q = 0;
    for (long i = threadIdx.x; i < per_image; i += 256) {
      const Slot t = part[(long)b * per_image + i];
      s += t.ssum, q += t.sse;
    }
    block_sum256(s, q, rs, rq);
    if (threadIdx.x == 0) {
      out[2 * b] = (double)q;
      if (want_ssim) out[2 * b + 1] = s / centres;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// SSE -> dB with the host's bits.  calculate_psnr is 20 * log10(255 / sqrt(sse / count)) in float64: the division and
// the square root are correctly rounded everywhere, the C library's log10 is not, so a device log10 of its own differs
// from it in the last place on every fifth value.  The host's log10 is fdlibm's e_log10: with x = 2^k f,
//   i = (k < 0), f' = f 2^-i in [0.5, 2), y = k + i,   log10(x) = (y log10_2lo + ivln10 log(f')) + y log10_2hi,
// every operation rounded on its own (no FMA), around a log that is correctly rounded but for about 1 value in 2000 (glibc 2.35: 16 of 30000 sampled).
// So the same formula around a correctly rounded log gives the host's dB except where the host's own log is misrounded.
// log(f') = 2 atanh(s), s = (f' - 1) / (f' + 1), |s| <= 1/3, summed in double-double (37 odd terms: 9^-37 < 2^-117;
// error about 2^-98 relative), whose high word is the correctly rounded double.  One thread per image: the cost is nothing.
// Host and device run the same source (kair_psnr_db_ref is the host instance, tested against a multiprecision log).
#define KAIR_HD __host__ __device__ inline

struct dd {
  double hi, lo;
};

KAIR_HD dd two_sum(double a, double b) {
#pragma clang fp contract(off)
  const double s = a + b, bb = s - a;
  return dd{s, (a - (s - bb)) + (b - bb)};
}
KAIR_HD dd quick_two_sum(double a, double b) {   // |a| >= |b|
#pragma clang fp contract(off)
  const double s = a + b;
  return dd{s, b - (s - a)};
}
KAIR_HD dd dd_add(dd a, dd b) {
#pragma clang fp contract(off)
  const dd s = two_sum(a.hi, b.hi);
  return quick_two_sum(s.hi, s.lo + (a.lo + b.lo));
}
KAIR_HD dd dd_mul(dd a, dd b) {
#pragma clang fp contract(off)
  const double p = a.hi * b.hi;
  const double e = fma(a.hi, b.hi, -p);
  return quick_two_sum(p, e + (a.hi * b.lo + a.lo * b.hi));
}
KAIR_HD dd dd_neg(dd a) { return dd{-a.hi, -a.lo}; }
// a / b by three quotient digits, each from the exact remainder
KAIR_HD dd dd_div(dd a, dd b) {
#pragma clang fp contract(off)
  const double q1 = a.hi / b.hi;
  dd r = dd_add(a, dd_neg(dd_mul(b, dd{q1, 0.})));
  const double q2 = r.hi / b.hi;
  r = dd_add(r, dd_neg(dd_mul(b, dd{q2, 0.})));
  const double q3 = r.hi / b.hi;
  return dd_add(quick_two_sum(q1, q2), dd{q3, 0.});
}

// the correctly rounded log of f in [0.5, 2)
KAIR_HD double log_rounded(double f) {
  const dd s = dd_div(dd{f - 1., 0.}, two_sum(f, 1.));   // (f - 1 is exact on [0.5, 2])
  const dd s2 = dd_mul(s, s);
  dd sum{0., 0.};
#pragma unroll 1
  for (int k = 36; k >= 0; --k) sum = dd_add(dd_mul(sum, s2), dd_div(dd{1., 0.}, dd{(double)(2 * k + 1), 0.}));
  const dd r = dd_mul(s, sum);
  return 2. * r.hi;   // (r is normalised: r.hi is the sum rounded to nearest)
}

// fdlibm e_log10 of a positive, finite, normal x around log_rounded
KAIR_HD double log10_fdlibm(double x) {
#pragma clang fp contract(off)
  constexpr double ivln10 = 4.34294481903251816668e-01, log10_2hi = 3.01029995663611771306e-01,
                   log10_2lo = 3.69423907715893078616e-13;
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, x);
  const int k = (int)((bits >> 52) & 0x7ff) - 1023, i = k < 0 ? 1 : 0;
  const double f = __builtin_bit_cast(double, (bits & 0x000fffffffffffffULL) | ((unsigned long long)(0x3ff - i) << 52));
  const double y = (double)(k + i);
  const double z = y * log10_2lo + ivln10 * log_rounded(f);
  return z + y * log10_2hi;
}

// calculate_psnr from the exact SSE: inf at 0
KAIR_HD double psnr_db(double sse, double count) {
#pragma clang fp contract(off)
  if (!(sse > 0.)) return __builtin_huge_val();
  const double mse = sse / count;
  return 20. * log10_fdlibm(255. / sqrt(mse));
}

// (db may be sse: each thread reads its element before it writes it)
__global__ void psnr_db_kernel(const double* sse, long lds, double count, double* db, long ldd, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) db[i * ldd] = psnr_db(sse[i * lds], count);
}

inline long tiles(long n) { return (n + TS - 1) / TS; }

// planes per image, cropped region; false when the arguments describe no valid call
inline bool geometry(int B, int C, int Hh, int Ww, int border, int flags, int* P, long* Hr, long* Wr) {
  if (B <= 0 || (C != 1 && C != 3) || Hh <= 0 || Ww <= 0 || border < 0) return false;
  if ((flags & ~(KAIR_METRIC_Y | KAIR_METRIC_SSIM)) || ((flags & KAIR_METRIC_Y) && C != 3)) return false;
  *P = (flags & KAIR_METRIC_Y) ? 1 : C;
  *Hr = (long)Hh - 2L * border, *Wr = (long)Ww - 2L * border;
  if (*Hr <= 0 || *Wr <= 0) return false;
  if ((flags & KAIR_METRIC_SSIM) && (*Hr < WIN || *Wr < WIN)) return false;
  return true;
}

}  // namespace

extern "C" long kair_image_metrics_workspace_bytes(int B, int C, int H, int W, int border, int flags) {
  int P;
  long Hr, Wr;
  if (!geometry(B, C, H, W, border, flags, &P, &Hr, &Wr)) return 0;
  return (long)sizeof(Slot) * B * P * tiles(Hr) * tiles(Wr);
}

extern "C" int kair_image_metrics(const float* E, const float* H, double* out, int B, int C, int Hh, int Ww, int border,
                                  int flags, void* workspace, void* stream) {
  KAIR_CHECK_ARG(E && H && out && workspace, "image_metrics: null pointer");
  KAIR_CHECK_ARG(B > 0 && Hh > 0 && Ww > 0 && border >= 0, "image_metrics: empty image or negative border");
  KAIR_CHECK_ARG(C == 1 || C == 3, "image_metrics: C = %d (1 or 3)", C);
  KAIR_CHECK_ARG(!(flags & ~(KAIR_METRIC_Y | KAIR_METRIC_SSIM)), "image_metrics: unknown flag bits %d", flags);
  KAIR_CHECK_ARG(!(flags & KAIR_METRIC_Y) || C == 3, "image_metrics: the Y channel needs C = 3 (got %d)", C);
  int P;
  long Hr, Wr;
  KAIR_CHECK_ARG(geometry(B, C, Hh, Ww, border, flags, &P, &Hr, &Wr),
                 "image_metrics: the region left by border %d of %d x %d is empty%s", border, Hh, Ww,
                 (flags & KAIR_METRIC_SSIM) ? " or smaller than the 11 x 11 window" : "");
  KAIR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "image_metrics: workspace must be 16-byte aligned");
  KAIR_CHECK_ARG((long)Hh * Ww < (1L << 31) && (long)B * P <= 65535 && tiles(Hr) <= 65535,
                 "image_metrics: image too large (plane < 2^31 pixels, B * planes <= 65535, H <= 65535 * 32)");
  hipStream_t s = (hipStream_t)stream;
  Slot* part = (Slot*)workspace;
  const dim3 grid((unsigned)tiles(Wr), (unsigned)tiles(Hr), (unsigned)(B * P));
  const bool y = flags & KAIR_METRIC_Y, ssim = flags & KAIR_METRIC_SSIM;
  const int hr = (int)Hr, wr = (int)Wr;
  if (ssim && y)
    KAIR_LAUNCH((metrics_ssim_kernel<true>), grid, dim3(256), 0, s, E, H, part, Hh, Ww, border, hr, wr);
  else if (ssim)
    KAIR_LAUNCH((metrics_ssim_kernel<false>), grid, dim3(256), 0, s, E, H, part, Hh, Ww, border, hr, wr);
  else if (y)
    KAIR_LAUNCH((metrics_sse_kernel<true>), grid, dim3(256), 0, s, E, H, part, Hh, Ww, border, hr, wr);
  else
    KAIR_LAUNCH((metrics_sse_kernel<false>), grid, dim3(256), 0, s, E, H, part, Hh, Ww, border, hr, wr);
  KAIR_CHECK_LAUNCH();
  const long per_image = (long)P * grid.x * grid.y;
  const double centres = ssim ? (double)P * (double)(Hr - 2 * HALO) * (double)(Wr - 2 * HALO) : 1.;
  KAIR_LAUNCH(metrics_final_kernel, dim3(1), dim3(256), 0, s, part, per_image, B, centres, (int)ssim, out);
  KAIR_CHECK_LAUNCH();
  return 0;
}

extern "C" double kair_psnr_db_ref(double sse, double count) { return psnr_db(sse, count); }

extern "C" int kair_psnr_db(const double* sse, long lds, double* db, long ldd, int n, double count, void* stream) {
  KAIR_CHECK_ARG(sse && db, "psnr_db: null pointer");
  KAIR_CHECK_ARG(n > 0 && lds >= 1 && ldd >= 1, "psnr_db: n, lds, ldd must be positive");
  KAIR_CHECK_ARG(count >= 1., "psnr_db: count %g (the number of compared values, >= 1)", count);
  KAIR_LAUNCH(psnr_db_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, sse, lds, count, db, ldd, n);
  KAIR_CHECK_LAUNCH();
  return 0;
}
