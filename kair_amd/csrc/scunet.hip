// SCUNet (Swin-Conv-UNet) reductions: the two gradient forms its transformer blocks need beside the shared kernels.
//   kair_qkvblk_colsum: the q/k/v bias gradient, the column sums of the head-blocked dq/dk/dv the window-attention
//     backward writes (head dim = head pad = 32 leaves no pad column for a ones column, and kair_colsum takes plain
//     rows only);
//   kair_table_transpose: the relative-position gradient [(2ws-1)^2][nh] of kair_window_attn_bwd brought into the
//     parameter's [nh][2ws-1][2ws-1] layout.
// Both are deterministic (fixed summation order, no atomics).
#include "common.h"

#define QCS_NB 64     // window chunks per (part, head)
#define QCS_HP 32     // head pad of the q/k/v layouts
#define QCS_TOK 64    // tokens per window

static inline int nblk_(long n, int b) { return (int)((n + b - 1) / b); }

// dqkv [3][nWin][nh][64][32]: block (b, ph) sums the windows b, b + nb, ... of (part, head) ph into part[ph][b][32]
template <typename T>
__global__ __launch_bounds__(256) void qkvblk_colsum_partial(const T* __restrict__ g, long nWin, int nh, int nb,
                                                             float* __restrict__ part) {
  __shared__ float red[8][QCS_HP];
  const int col = threadIdx.x % QCS_HP, rl = threadIdx.x / QCS_HP;
  const int ph = blockIdx.y, p = ph / nh, h = ph % nh;
  float acc = 0.f;
  for (long w = blockIdx.x; w < nWin; w += nb) {
    const T* base = g + (((long)p * nWin + w) * nh + h) * (QCS_TOK * QCS_HP);
#pragma unroll
    for (int t = rl; t < QCS_TOK; t += 8) acc += to_f(base[t * QCS_HP + col]);
  }
  red[rl][col] = acc;
  __syncthreads();
  if (rl == 0) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += red[i][col];
    part[((long)ph * nb + blockIdx.x) * QCS_HP + col] = s;
  }
}

// bias_grad[ph * hd + d] (+)= sum_b part[ph][b][d]
__global__ void qkvblk_colsum_final(const float* __restrict__ part, int nb, int hd, float* __restrict__ out,
                                    int accumulate) {
  const int ph = blockIdx.x, d = threadIdx.x;
  if (d >= hd) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += part[((long)ph * nb + b) * QCS_HP + d];
  float* o = out + (long)ph * hd + d;
  *o = accumulate ? *o + s : s;
}

extern "C" long kair_qkvblk_colsum_ws(int nh) { return nh > 0 ? (long)3 * nh * QCS_NB * QCS_HP : 0; }

extern "C" int kair_qkvblk_colsum(const void* dqkv, int dtype, long nWin, int nh, int hd, float* ws, float* bias_grad,
                                  int accumulate, void* stream) {
  KAIR_CHECK_ARG(dqkv && ws && bias_grad, "qkvblk_colsum: null pointer");
  KAIR_CHECK_ARG(nWin > 0 && nh > 0 && hd > 0 && hd <= QCS_HP, "qkvblk_colsum: nWin %ld, nh %d, head dim %d", nWin, nh, hd);
  KAIR_CHECK_ARG(dtype == KAIR_F32 || dtype == KAIR_BF16, "qkvblk_colsum: fp32 or bf16");
  const int nb = (int)(nWin < QCS_NB ? nWin : QCS_NB);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == KAIR_BF16)
    KAIR_LAUNCH(qkvblk_colsum_partial<bf16>, dim3(nb, 3 * nh), dim3(256), 0, s, (const bf16*)dqkv, nWin, nh, nb, ws);
  else
    KAIR_LAUNCH(qkvblk_colsum_partial<float>, dim3(nb, 3 * nh), dim3(256), 0, s, (const float*)dqkv, nWin, nh, nb, ws);
  KAIR_CHECK_LAUNCH();
  KAIR_LAUNCH(qkvblk_colsum_final, dim3(3 * nh), dim3(QCS_HP), 0, s, ws, nb, hd, bias_grad, accumulate);
  KAIR_CHECK_LAUNCH();
  return 0;
}

// dst[c][r] (+)= src[r][c]
__global__ void table_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int C,
                                       int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R * C) return;
  const int c = i / R, r = i % R;
  const float v = src[(long)r * C + c];
  dst[i] = accumulate ? dst[i] + v : v;
}

extern "C" int kair_table_transpose(const float* src, float* dst, int R, int C, int accumulate, void* stream) {
  KAIR_CHECK_ARG(src && dst && src != dst, "table_transpose: null or aliased pointers");
  KAIR_CHECK_ARG(R > 0 && C > 0 && (long)R * C < (1L << 30), "table_transpose: %d x %d", R, C);
  KAIR_LAUNCH(table_transpose_kernel, dim3(nblk_((long)R * C, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, R, C,
              accumulate);
  KAIR_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// kair_scu_block_fwd: SCUNet's narrow transformer Block (trans_dim C = 32 / 64, 1 / 2 heads of 32, window 8) in one
// launch, bf16 operands with fp32 accumulation.  One 256-thread workgroup per 8 x 8 window of the level's grid:
//   x (the window's 64 token rows, gathered through the shifted window map) -> LN1 -> q/k/v -> per head
//   softmax(q k^T scale + table[relidx] + region mask (-100)) v -> linear + residual -> LN2 -> fc1 -> GELU (erf) ->
//   fc2 + residual -> out (scattered back through the same map; out may be x).
// The fp32 token tile, the bf16 operands (LN output / O, q|k, v^T, probabilities, the 4C hidden tile) and the fp32
// scores live in LDS; nothing but x is read from and nothing but out written to the activation buffers.  The weights
// ([N][K] bf16 rows, the unfused GEMMs' packs) go from L2 straight into the MFMA B registers, each fragment once per
// workgroup.  Every product is v_mfma_f32_32x32x16_bf16 on 32 x 32 output tiles spread over the four waves; the
// softmax is one wave64 reduction per row.
// ---------------------------------------------------------------------------------------------------------------
#include "attn_common.h"

namespace {

struct ScuArgs {
  const float* x; long ldx; float* out; long ldo;
  const float *g1, *b1, *g2, *b2; float eps;
  const bf16 *wqkv, *wproj, *w1, *w2;
  const float *bqkv, *bproj, *bb1, *bb2;
  const float* table; float scale;
  int H, W, shift;
};

// acc = A[row0 .. row0+32)[0 .. K) . B[n0 .. n0+32)[0 .. K)^T, both row-major bf16 (A in LDS; B in LDS or global)
template <int K>
KAIR_DEV f32x16 tile_nt(const bf16* A, int lda, int row0, const bf16* B, int ldb, int n0, int lane) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const bf16* a = A + (row0 + (lane & 31)) * lda + 8 * (lane >> 5);
  const bf16* b = B + (long)(n0 + (lane & 31)) * ldb + 8 * (lane >> 5);
#pragma unroll
  for (int kb = 0; kb < K / 16; ++kb)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(a + 16 * kb), *(const bf16x8*)(b + 16 * kb), acc, 0, 0, 0);
  return acc;
}

// LayerNorm of the 16 rows of wave `wave` of the fp32 tile xs [64][C] into the bf16 operand A [64][lda]
template <int C>
KAIR_DEV void ln_rows(const float* xs, bf16* A, int lda, const float* g, const float* b, float eps, int wave, int lane) {
  const bool on = lane < C;
  const float gg = on ? g[lane] : 0.f, bb = on ? b[lane] : 0.f;
  for (int r = wave * 16; r < wave * 16 + 16; ++r) {
    const float v = on ? xs[r * C + lane] : 0.f;
    const float mean = wave_sum(v) * (1.f / C);
    const float d = on ? v - mean : 0.f;
    const float rstd = rsqrtf(wave_sum(d * d) * (1.f / C) + eps);
    if (on) A[r * lda + lane] = (bf16)(d * rstd * gg + bb);
  }
}

template <int C>
__global__ __launch_bounds__(256) void scu_block_fwd_kernel(ScuArgs p) {
  constexpr int NH = C / 32, LDA = C + 8, LDQ = 2 * C + 8, LDV = TOK + 8, LDS_ = TOK + 4, LDP = TOK + 8, LDH = 4 * C + 8;
  __shared__ __attribute__((aligned(16))) float xs[TOK * C];
  __shared__ __attribute__((aligned(16))) bf16 sA[TOK * LDA];
  __shared__ __attribute__((aligned(16))) bf16 sQK[TOK * LDQ];
  __shared__ __attribute__((aligned(16))) bf16 sVT[C * LDV];
  __shared__ __attribute__((aligned(16))) float sS[TOK * LDS_];
  __shared__ __attribute__((aligned(16))) bf16 sP[TOK * LDP];
  __shared__ __attribute__((aligned(16))) bf16 sH[TOK * LDH];
  __shared__ int tokrow[TOK];
  __shared__ int treg[TOK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int nWw = p.W / WS, nW = (p.H / WS) * nWw;
  const int g = blockIdx.x, img = g / nW, wi = g - img * nW;
  if (tid < TOK) {
    const int wy = wi / nWw, wx = wi - wy * nWw;
    int y = wy * WS + (tid >> 3) + p.shift, x = wx * WS + (tid & 7) + p.shift;
    if (y >= p.H) y -= p.H;
    if (x >= p.W) x -= p.W;
    tokrow[tid] = (img * p.H + y) * p.W + x;
    treg[tid] = token_region(wi, tid, p.H, p.W, p.shift);
  }
  __syncthreads();
  for (int i = tid; i < TOK * (C / 4); i += 256) {
    const int t = i / (C / 4), c4 = i - t * (C / 4);
    *(float4*)(xs + t * C + 4 * c4) = *(const float4*)(p.x + (long)tokrow[t] * p.ldx + 4 * c4);
  }
  __syncthreads();
  ln_rows<C>(xs, sA, LDA, p.g1, p.b1, p.eps, wave, lane);
  __syncthreads();
  // q | k -> sQK [64][2C], v -> sVT [C][64] (transposed: the contraction of P v runs over tokens)
  for (int tile = wave; tile < 2 * (3 * C / 32); tile += 4) {
    const int rt = tile & 1, nt = tile >> 1;
    const f32x16 acc = tile_nt<C>(sA, LDA, rt * 32, p.wqkv, C, nt * 32, lane);
    const int n = nt * 32 + l31;
    const float bias = p.bqkv[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rt * 32 + acc_row(r, hh);
      const bf16 v = (bf16)(acc[r] + bias);
      if (n < 2 * C) sQK[row * LDQ + n] = v;
      else sVT[(n - 2 * C) * LDV + row] = v;
    }
  }
  __syncthreads();
  for (int h = 0; h < NH; ++h) {
    {   // scores: one 32 x 32 tile per wave
      const int qt = wave & 1, kt = wave >> 1;
      const f32x16 acc = tile_nt<32>(sQK + h * 32, LDQ, qt * 32, sQK + C + h * 32, LDQ, kt * 32, lane);
      const int kj = kt * 32 + l31, rk = treg[kj];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = qt * 32 + acc_row(r, hh);
        float s = acc[r] * p.scale + p.table[relidx(qi, kj) * NH + h];
        if (p.shift > 0 && treg[qi] != rk) s += -100.f;
        sS[qi * LDS_ + kj] = s;
      }
    }
    __syncthreads();
    for (int r = wave * 16; r < wave * 16 + 16; ++r) {   // wave64 softmax: one key per lane
      const float s = sS[r * LDS_ + lane];
      const float e = __expf(s - wave_max(s));
      sP[r * LDP + lane] = (bf16)(e / wave_sum(e));
    }
    __syncthreads();
    if (wave < 2) {   // O_h = P v_h: [64][32], one row tile per wave
      const f32x16 acc = tile_nt<TOK>(sP, LDP, wave * 32, sVT + h * 32 * LDV, LDV, 0, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) sA[(wave * 32 + acc_row(r, hh)) * LDA + h * 32 + l31] = (bf16)acc[r];
    }
    __syncthreads();
  }
  // mid = x + linear(O)
  for (int tile = wave; tile < 2 * (C / 32); tile += 4) {
    const int rt = tile & 1, nt = tile >> 1;
    const f32x16 acc = tile_nt<C>(sA, LDA, rt * 32, p.wproj, C, nt * 32, lane);
    const int n = nt * 32 + l31;
    const float bias = p.bproj[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) xs[(rt * 32 + acc_row(r, hh)) * C + n] += acc[r] + bias;
  }
  __syncthreads();
  ln_rows<C>(xs, sA, LDA, p.g2, p.b2, p.eps, wave, lane);
  __syncthreads();
  for (int tile = wave; tile < 2 * (4 * C / 32); tile += 4) {
    const int rt = tile & 1, nt = tile >> 1;
    const f32x16 acc = tile_nt<C>(sA, LDA, rt * 32, p.w1, C, nt * 32, lane);
    const int n = nt * 32 + l31;
    const float bias = p.bb1[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) sH[(rt * 32 + acc_row(r, hh)) * LDH + n] = (bf16)gelu_erf(acc[r] + bias);
  }
  __syncthreads();
  for (int tile = wave; tile < 2 * (C / 32); tile += 4) {
    const int rt = tile & 1, nt = tile >> 1;
    const f32x16 acc = tile_nt<4 * C>(sH, LDH, rt * 32, p.w2, 4 * C, nt * 32, lane);
    const int n = nt * 32 + l31;
    const float bias = p.bb2[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rt * 32 + acc_row(r, hh);
      p.out[(long)tokrow[row] * p.ldo + n] = xs[row * C + n] + acc[r] + bias;
    }
  }
}

}  // namespace

extern "C" int kair_scu_block_fwd(const float* x, long ldx, float* out, long ldo, const float* gamma1, const float* beta1,
                                  const float* gamma2, const float* beta2, float eps, const void* wqkv, const float* bqkv,
                                  const void* wproj, const float* bproj, const void* w1, const float* b1, const void* w2,
                                  const float* b2, const float* table, float scale, int B, int H, int W, int C, int shift,
                                  void* stream) {
  KAIR_CHECK_ARG(x && out && gamma1 && beta1 && gamma2 && beta2 && wqkv && bqkv && wproj && bproj && w1 && b1 && w2 && b2 &&
                 table, "scu_block_fwd: null pointer");
  KAIR_CHECK_ARG(C == 32 || C == 64, "scu_block_fwd: trans_dim %d (32 or 64)", C);
  KAIR_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % WS == 0 && W % WS == 0 && (long)B * H * W < (1L << 24),
                 "scu_block_fwd: %d images of %d x %d tokens (multiples of 8, B*H*W < 2^24)", B, H, W);
  KAIR_CHECK_ARG(shift == 0 || shift == WS / 2, "scu_block_fwd: shift %d (0 or 4)", shift);
  KAIR_CHECK_ARG(ldx >= C && ldo >= C && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0, "scu_block_fwd: row strides / alignment");
  KAIR_CHECK_ARG((((uintptr_t)wqkv | (uintptr_t)wproj | (uintptr_t)w1 | (uintptr_t)w2) & 15) == 0,
                 "scu_block_fwd: weight packs must be 16-byte aligned");
  ScuArgs a{x, ldx, out, ldo, gamma1, beta1, gamma2, beta2, eps, (const bf16*)wqkv, (const bf16*)wproj, (const bf16*)w1,
            (const bf16*)w2, bqkv, bproj, b1, b2, table, scale, H, W, shift};
  const int nWin = B * (H / WS) * (W / WS);
  if (C == 32) KAIR_LAUNCH(scu_block_fwd_kernel<32>, dim3(nWin), dim3(256), 0, (hipStream_t)stream, a);
  else KAIR_LAUNCH(scu_block_fwd_kernel<64>, dim3(nWin), dim3(256), 0, (hipStream_t)stream, a);
  KAIR_CHECK_LAUNCH();
  return 0;
}
