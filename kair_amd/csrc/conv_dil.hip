// Dilated 3x3 convolution (stride 1, padding = dilation = d, d in 2..4) for gfx950: IRCNN's 64 -> 64 body convs
// (network_dncnn.IRCNN, dilations 2, 3, 4, 3, 2) and their input gradients, as the implicit GEMM
//   D[n][p] = sum_k W[n][k] X^T[k][p],  k = tap * C + c,  tap (dy, dx) reading pixel (y + d dy, x + d dx).
//
// conv3x3_wr (conv_wr.hip) is the model: the input tile and its halo live in LDS for the whole tile, the weight
// fragments (pack kind 15 forward -- only its hi halves, bf16(w), are read -- or kind 16 for the input gradient; both
// are k = tap * C + c, so dilation-independent) stream from global memory straight into MFMA registers
// (v_mfma_f32_16x16x32_bf16, fp32 accumulation), and each lane stores 4 consecutive channels of one pixel.
//
// What differs is the tile.  conv3x3_wr's tiles are row strips; with a halo of d on every side a one-row strip reads
// (1 + 2 d) x its own pixels, 9 x at d = 4.  Here a tile is DL_TY x DL_TX = 8 x 16 output pixels with a
// (8 + 2 d) x (16 + 2 d) halo:
//     d   halo pixels   / 128 tile pixels   LDS bytes (bf16, pixel stride C + 8 = 72)
//     2   12 x 20 = 240      1.88 x              34,560
//     3   14 x 22 = 308      2.41 x              44,352
//     4   16 x 24 = 384      3.00 x              55,296
// The kernel reserves the d = 4 size (55,296 B), so two workgroups share a CU's 160 KB: one fills its halo while the
// other multiplies.  A fragment row of 16 pixels is one tile row, so a lane's halo address is its pixel's plus a
// wave-uniform tap offset, exactly as in conv3x3_wr.
//
// Work split: 256 threads, the four waves as 2 (tile-row halves) x 2 (channel halves): a wave owns 4 tile rows x 32
// output channels = 4 x 2 accumulator fragments.  Per k-step of 32 that is 8 MFMAs per wave against 4 ds_read_b128 and
// 2 weight fragments (1 KiB wave loads, each shared by the two waves of a channel half through L1), a ring six k-steps
// deep.  (One wave per 16 channels of the whole tile, conv3x3_wr's narrow form, reads every halo fragment four times:
// 8 LDS reads per 8 MFMAs, LDS-bound.)  The k-loop (18 steps at C = 64) is fully unrolled: no barrier inside it.
//
// Ragged sizes: any H, W >= 1.  The grid is one workgroup per tile (B x ceil(H / 8) x ceil(W / 16)), not persistent;
// the halo fill writes zeros for every pixel outside image b (never the neighbouring image's rows), edge tiles mask
// their stores.  Contract: C = N = 64, bf16 image rows, d in 2..4 (kair_conv3x3_dil_ok); everything else is the generic
// dilated im2col operand of kair_gemm_nt (kair_operand.im_dil).
#include "common.h"

namespace {

constexpr int DL_TY = 8, DL_TX = 16, DL_C = 64, DL_PS = DL_C + 8, DL_MAXD = 4;
constexpr int DL_HALO = (DL_TY + 2 * DL_MAXD) * (DL_TX + 2 * DL_MAXD) * DL_PS;   // bf16 elements
constexpr int DL_NT = 256, DL_KS = 9 * DL_C / 32, DL_PD = 6;                     // threads, k-steps, weight ring depth
constexpr int DL_RM = 4, DL_RN = 2;
constexpr int DL_HP = (DL_HALO / DL_PS * (DL_C / 8) + DL_NT - 1) / DL_NT;        // 16-byte halo pieces per thread (12)

struct ConvDilArgs {
  const bf16* x; long ldx;           // NHWC image rows
  const bf16* w; int wstride;        // fragment blocks of 512: kind 15 (stride 2: hi, lo) or kind 16 (stride 1)
  const float* bias;                 // [64] or null
  void* out; int odt; long ldo;
  int act; float slope;
  int H, W, d, flip;
  int tilesX, tilesY;
  FDiv fhwd, ftx, fty;               // halo row width, tiles per row, tiles per column
};

__global__ __launch_bounds__(DL_NT, 2) void conv3x3_dil_kernel(const ConvDilArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 sH[DL_HALO];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int H = a.H, W = a.W, d = a.d;
  const int HWD = DL_TX + 2 * d, HR = DL_TY + 2 * d;
  const int halo_pieces = HR * HWD * (DL_C / 8);
  // this workgroup's tile
  const int t = blockIdx.x;
  const int trow = fdiv(t, a.ftx), tx = t - trow * a.tilesX;
  const int b = fdiv(trow, a.fty), ty = trow - b * a.tilesY;
  const int y0 = ty * DL_TY, x0 = tx * DL_TX;

  // this wave's weight fragments: n blocks 2 wn + rn, k-step s (one coalesced 1 KiB wave load each)
  const bf16* wb = a.w + ((long)(DL_RN * wn) * DL_KS * a.wstride) * 512 + lane * 8;
  auto wfrag = [&](int rn, int s) { return *(const bf16x8*)(wb + ((long)(rn * DL_KS + s) * a.wstride) * 512); };
  bf16x8 rb[DL_PD][DL_RN];
  auto issue_w = [&](int slot, int s) {
#pragma unroll
    for (int rn = 0; rn < DL_RN; ++rn) rb[slot][rn] = wfrag(rn, s);
  };
  // the first k-steps' weights in flight under the halo fill
#pragma unroll
  for (int u = 0; u < DL_PD; ++u) issue_w(u, u);
  float4 bias4[DL_RN];
#pragma unroll
  for (int rn = 0; rn < DL_RN; ++rn) {
    const int n = 32 * wn + 16 * rn + 4 * fq;
    bias4[rn] = a.bias ? *(const float4*)(a.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
  }

  {   // halo fill: every load issued, then written (one exposed memory latency); zeros outside image b
    uint4 v[DL_HP];
#pragma unroll
    for (int i = 0; i < DL_HP; ++i) {
      const int idx = tid + DL_NT * i;
      const int pix = idx >> 3, c8 = idx & 7;
      const int hr = fdiv(pix, a.fhwd), hc = pix - hr * HWD;
      const int y = y0 - d + hr, x = x0 - d + hc;
      const bool ok = idx < halo_pieces && y >= 0 && y < H && x >= 0 && x < W;
      v[i] = make_uint4(0, 0, 0, 0);
      if (ok) v[i] = *(const uint4*)(a.x + ((long)(b * H + y) * W + x) * a.ldx + c8 * 8);
    }
#pragma unroll
    for (int i = 0; i < DL_HP; ++i) {
      const int idx = tid + DL_NT * i;
      if (idx < halo_pieces) *(uint4*)(sH + (idx >> 3) * DL_PS + (idx & 7) * 8) = v[i];
    }
  }
  __syncthreads();   // halo visible

  int hb[DL_RM];     // halo element offset of each fragment row's centre pixel (+ this lane's 8 channels of a k-step)
#pragma unroll
  for (int i = 0; i < DL_RM; ++i) hb[i] = ((wm * DL_RM + i + d) * HWD + fr + d) * DL_PS + fq * 8;
  const int sd = a.flip ? -d : d;
  bf16x8 ra[2][DL_RM];   // activation fragments, one k-step ahead
  auto read_a = [&](int buf, int s) {
    const int tap = s / (DL_C / 32), c0 = (s - tap * (DL_C / 32)) * 32;
    const int dy = (tap / 3 - 1) * sd, dx = (tap - (tap / 3) * 3 - 1) * sd;
    const int off = (dy * HWD + dx) * DL_PS + c0;
#pragma unroll
    for (int i = 0; i < DL_RM; ++i) ra[buf][i] = *(const bf16x8*)(sH + hb[i] + off);
  };
  f32x4 acc[DL_RM][DL_RN];
#pragma unroll
  for (int i = 0; i < DL_RM; ++i)
#pragma unroll
    for (int rn = 0; rn < DL_RN; ++rn) acc[i][rn] = f32x4{0.f, 0.f, 0.f, 0.f};

  read_a(0, 0);
#pragma unroll
  for (int s = 0; s < DL_KS; ++s) {
    const int ab = s & 1, ws = s % DL_PD;
    if (s + 1 < DL_KS) read_a(ab ^ 1, s + 1);
#pragma unroll
    for (int i = 0; i < DL_RM; ++i)
#pragma unroll
      for (int rn = 0; rn < DL_RN; ++rn)
        acc[i][rn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rb[ws][rn], ra[ab][i], acc[i][rn], 0, 0, 0);
    if (s + DL_PD < DL_KS) issue_w(ws, s + DL_PD);
  }

  // epilogue: 4 consecutive channels of one pixel per lane; edge tiles mask their stores
  const int x = x0 + fr;
#pragma unroll
  for (int i = 0; i < DL_RM; ++i) {
    const int y = y0 + wm * DL_RM + i;
    if (y >= H || x >= W) continue;
    const long m = (long)(b * H + y) * W + x;
#pragma unroll
    for (int rn = 0; rn < DL_RN; ++rn) {
      const int n = 32 * wn + 16 * rn + 4 * fq;
      const float4 bb = bias4[rn];
      float v[4] = {acc[i][rn][0] + bb.x, acc[i][rn][1] + bb.y, acc[i][rn][2] + bb.z, acc[i][rn][3] + bb.w};
      if (a.act == KAIR_ACT_RELU) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], 0.f);
      } else if (a.act == KAIR_ACT_LEAKY) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = v[q] > 0.f ? v[q] : v[q] * a.slope;
      }
      const long o = m * a.ldo + n;
      if (a.odt == KAIR_BF16)
        *(bf16x4*)((bf16*)a.out + o) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
      else
        *(float4*)((float*)a.out + o) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

}  // namespace

/* 1 when kair_conv3x3_dil takes this conv (see kair_hip.h), else 0. */
extern "C" int kair_conv3x3_dil_ok(int dil, int C, int N) {
  return dil >= 2 && dil <= DL_MAXD && C == DL_C && N == DL_C;
}

extern "C" int kair_conv3x3_dil(const void* x, long ldx, int dil, int flip, const void* w, int w_kind, const float* bias,
                                int act, float slope, void* out, int out_dtype, long ldo, int B, int H, int W, int C,
                                int N, void* stream) {
  KAIR_CHECK_ARG(x && w && out && B > 0 && H > 0 && W > 0, "conv3x3_dil: null operand or empty image");
  KAIR_CHECK_ARG(kair_conv3x3_dil_ok(dil, C, N),
                 "conv3x3_dil: unsupported geometry (dilation %d, C %d, N %d): dilation 2..4 and C = N = 64", dil, C, N);
  KAIR_CHECK_ARG(w_kind == 15 || w_kind == 16, "conv3x3_dil: packed weight kind 15 (forward) or 16 (input gradient), got %d",
                 w_kind);
  KAIR_CHECK_ARG(out_dtype == KAIR_F32 || out_dtype == KAIR_BF16, "conv3x3_dil: output dtype");
  KAIR_CHECK_ARG(act == KAIR_ACT_NONE || act == KAIR_ACT_RELU || act == KAIR_ACT_LEAKY, "conv3x3_dil: act none, ReLU or LeakyReLU");
  KAIR_CHECK_ARG(ldx >= C && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0,
                 "conv3x3_dil: bf16 image rows 16-byte aligned, ldx >= C");
  KAIR_CHECK_ARG(ldo >= N && ldo % 4 == 0 && ((uintptr_t)out & 15) == 0, "conv3x3_dil: output rows");
  KAIR_CHECK_ARG(!bias || ((uintptr_t)bias & 15) == 0, "conv3x3_dil: bias alignment");
  const long M = (long)B * H * W;
  KAIR_CHECK_ARG(M * (ldx > ldo ? ldx : ldo) < (1L << 31), "conv3x3_dil: operands past 2^31 elements");
  ConvDilArgs a;
  a.x = (const bf16*)x; a.ldx = ldx; a.w = (const bf16*)w; a.wstride = w_kind == 15 ? 2 : 1; a.bias = bias;
  a.out = out; a.odt = out_dtype; a.ldo = ldo; a.act = act; a.slope = slope;
  a.H = H; a.W = W; a.d = dil; a.flip = flip ? 1 : 0;
  a.tilesX = (W + DL_TX - 1) / DL_TX; a.tilesY = (H + DL_TY - 1) / DL_TY;
  a.fhwd = make_fdiv(DL_TX + 2 * dil); a.ftx = make_fdiv(a.tilesX); a.fty = make_fdiv(a.tilesY);
  const long tiles = (long)B * a.tilesX * a.tilesY;
  KAIR_CHECK_ARG(tiles < (1L << 24), "conv3x3_dil: more than 2^24 tiles");
  KAIR_LAUNCH(conv3x3_dil_kernel, dim3((unsigned)tiles), dim3(DL_NT), 0, (hipStream_t)stream, a);
  KAIR_CHECK_LAUNCH();
  return 0;
}
