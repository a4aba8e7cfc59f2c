// Training of the GRU speech-to-code generator (codebook/end2end.py around generate.py's Generator_gru): the kernels behind
// qpgesture_amd/end2end.py that the inference file (qpg_gen.hip) does not have.  Everything is f32, activations are
// channels-last rows, the weight layouts are those of qpg_gen.hip.  The training forward's convolutions are
// qpg_gen_conv1d_f32 without epilogue; the input projections, the head and every data gradient of a Linear are
// qpg_wavlm_gemm_f32.  What is here:
//
// gent_bn_part_kernel / gent_bn_finish_kernel   per-channel sum and sum of squares of [R][C] rows: a thread owns 4 adjacent
//                       channels of every (1024 / C)-th row of its block's row groups and adds in f64; the block's
//                       threads of one channel are added in thread order, the blocks' partials in a fixed order, both in
//                       f64.  The finish writes mean, biased variance and (optionally) the running statistics.
// gent_bn_apply_kernel  (x - mean) / sqrt(var + eps) * gamma + beta, LeakyReLU.
// gent_bn_bwd_part_kernel / _finish / _dx       the same two-stage sums for sum dyh and sum dyh xhat, dyh = dy times the
//                       LeakyReLU gate read from the forward's OUTPUT (y <= 0 passes slope), then dx elementwise.
// gent_conv_bwd_data_kernel   dx as a gather: a thread owns 4 input channels of one input frame s and collects the taps
//                       j = s - stride t of the at most ceil(16 / stride) output frames that cover it; a frame that no
//                       window covers has an empty loop and is written as 0.
// gent_rowgrad_kernel   dW[n][k] = sum_r dY[r][n] X(r)[k] on v_mfma_f32_16x16x4_f32 with the contraction over ROWS: per
//                       matrix step lane (i, g) feeds dY[r0 + g][n0 + i] (A) and X(r0 + g)[k0 + i] (B).  X(r) is a
//                       row pointer computed from r = (b, t): b bstride + (t + shift) tstride, a zero row when t + shift
//                       leaves [0, T) - the convolutions' windows of 16 Cin contiguous floats (tstride = stride Cin) and
//                       the Linears' rows (with the recurrence's previous-step pairing as shift) are the same kernel.
//                       One WAVE owns a 16 NT x 64 tile of dW for one slab of rows; db rides along as a product with a
//                       column of ones.  Slab partials go to the caller's workspace and gent_reduce_kernel adds them in
//                       a fixed order in f64.
// gent_conv_in1_wgrad_kernel  the first convolution's weight gradient (Cin = 1) on the VALU: a thread owns rows, a block
//                       8 channels x 16 taps of one slab.
// gent_gru_fwd_kernel   gen_gru_kernel of qpg_gen.hip, instruction for instruction, that also stores r, z, n and
//                       W_hn h + b_hn.
// gent_gru_bwd_kernel   backpropagation through time with the forward's ownership: one block owns 16 sequences of one
//                       direction for all T steps, a lane owns 4 units of one sequence - the same (sequence, units) as in
//                       the product W_hh^T dgh's accumulator, so dh never leaves its lane's registers; the step's dgh
//                       goes through LDS as the B operand, W_hh^T is streamed from L2.
// gent_ln_bwd_kernel    direction sum + LayerNorm backward, one wave per row, dgamma / dbeta as slab partials;
// gent_ce_bwd_kernel    (softmax - onehot) / R; gent_dropout_kernel  x mask scale.
//
// No launch waits on another block, no global atomics, every loop is bounded by an argument, row offsets are 64-bit.
#include "qpg_common.h"

namespace {

constexpr int TAPS = QPG_GEN_TAPS;
constexpr int GH = QPG_GEN_HIDDEN;
constexpr int GBT = QPG_GEN_GRU_BATCH_TILE;
constexpr int HLD = QPG_GEN_HEAD_LD;
constexpr int GWAVES = (GH + 15) / 16;
constexpr int HS_LD = GH + 4;
constexpr int KCH = (GH + 15) / 16;
constexpr int G3 = 3 * GH;                       // 600: a direction's gate rows
constexpr int DG_LD = G3 + 4;                    // LDS row stride of the step's dgh
constexpr int KCH3 = (G3 + 15) / 16;             // 38 16-k chunks of W_hh^T's rows, the last one half full
constexpr int MAX_SLABS = QPG_GEN_TRAIN_MAX_SLABS;
constexpr int SLAB_MIN_ROWS = QPG_GEN_TRAIN_SLAB_MIN_ROWS;
constexpr int BN_MAX_BLOCKS = QPG_GEN_BN_MAX_BLOCKS;

__device__ __forceinline__ float gent_rstd(float var, float eps) { return f_div(1.0f, f_sqrt(f_add(var, eps))); }

// ---- BatchNorm statistics.  part: ws doubles [blocks][2][C].  A thread owns 4 adjacent channels (one 16-byte load) of
// every (1024 / C)-th row of its block's row groups; bn_block_sums adds the block's threads of one channel in thread order.
constexpr int BN_ROW_FLOATS = 1024;              // floats a block takes per pass: 1024 / C rows

__device__ __forceinline__ void bn_block_sums(const double (&s)[4], const double (&q)[4], int C, double* __restrict__ part) {
  __shared__ double sh[2][BN_ROW_FLOATS];
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sh[0][tid * 4 + i] = s[i];
    sh[1][tid * 4 + i] = q[i];
  }
  __syncthreads();
  if (tid < C) {
    const int rpb = BN_ROW_FLOATS / C;
    double ts = 0.0, tq = 0.0;
    for (int k = 0; k < rpb; ++k) {
      ts = f_add(ts, sh[0][k * C + tid]);
      tq = f_add(tq, sh[1][k * C + tid]);
    }
    part[((int64_t)blockIdx.x * 2 + 0) * C + tid] = ts;
    part[((int64_t)blockIdx.x * 2 + 1) * C + tid] = tq;
  }
}

__global__ __launch_bounds__(256) void gent_bn_part_kernel(const float* __restrict__ x, int64_t R, int C, int64_t groups,
                                                           double* __restrict__ part) {
  const int tid = threadIdx.x;
  const int c4n = C >> 2, rpb = BN_ROW_FLOATS / C;
  const int c0 = (tid % c4n) * 4, rr = tid / c4n;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    const int64_t row = rg * rpb + rr;
    if (row < R) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + row * C + c0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[i] = f_add(s[i], (double)v[i]);
        q[i] = f_add(q[i], f_mul((double)v[i], (double)v[i]));
      }
    }
  }
  bn_block_sums(s, q, C, part);
}

// the blocks' partials in block order: lane k of a channel's 256 / C adds blocks k, k + 256 / C, .., then the lanes in order
__device__ __forceinline__ void bn_sum_partials(const double* __restrict__ part, int blocks, int C, double* s_out,
                                                double* q_out) {
  __shared__ double sh[2][256];
  const int tid = threadIdx.x;
  const int c = tid % C, k = tid / C, lanes = 256 / C;
  double s = 0.0, q = 0.0;
  for (int b = k; b < blocks; b += lanes) {
    s = f_add(s, part[((int64_t)b * 2 + 0) * C + c]);
    q = f_add(q, part[((int64_t)b * 2 + 1) * C + c]);
  }
  sh[0][tid] = s;
  sh[1][tid] = q;
  __syncthreads();
  s = 0.0;
  q = 0.0;
  if (tid < C)
    for (int i = 0; i < lanes; ++i) {
      s = f_add(s, sh[0][i * C + tid]);
      q = f_add(q, sh[1][i * C + tid]);
    }
  *s_out = s;
  *q_out = q;
}

__global__ __launch_bounds__(256) void gent_bn_finish_kernel(const double* __restrict__ part, int blocks, int64_t R, int C,
                                                             float* __restrict__ stat, float* __restrict__ rmean,
                                                             float* __restrict__ rvar, float momentum) {
  const int c = threadIdx.x;
  double s, q;
  bn_sum_partials(part, blocks, C, &s, &q);
  if (c >= C) return;
  const double mean = f_div(s, (double)R);
  double var = f_sub(f_div(q, (double)R), f_mul(mean, mean));
  if (var < 0.0) var = 0.0;
  stat[c] = (float)mean;
  stat[C + c] = (float)var;
  if (rmean) rmean[c] = f_add(f_mul(f_sub(1.0f, momentum), rmean[c]), f_mul(momentum, (float)mean));
  if (rvar) {
    const float unb = (float)f_mul(var, f_div((double)R, (double)(R - 1)));
    rvar[c] = f_add(f_mul(f_sub(1.0f, momentum), rvar[c]), f_mul(momentum, unb));
  }
}

__global__ __launch_bounds__(256) void gent_bn_apply_kernel(const float* __restrict__ x, int64_t total, int C,
                                                            const float* __restrict__ stat, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, float slope,
                                                            float* __restrict__ y) {
  const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;       // (C % 4 == 0: 4 channels of one row)
  if (e >= total) return;
  const int c0 = (int)(e % C);
  const f32x4 xv = *reinterpret_cast<const f32x4*>(x + e);
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + i;
    const float v = f_add(f_mul(f_mul(f_sub(xv[i], stat[c]), gent_rstd(stat[C + c], eps)), gamma[c]), beta[c]);
    o[i] = v > 0.0f ? v : f_mul(v, slope);
  }
  *reinterpret_cast<f32x4*>(y + e) = o;
}

// ---- BatchNorm backward.  part: ws doubles [blocks][2][C], then the two means [2][C]
__global__ __launch_bounds__(256) void gent_bn_bwd_part_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ dy, int64_t R, int C,
                                                               int64_t groups, const float* __restrict__ stat, float eps,
                                                               float slope, double* __restrict__ part) {
  const int tid = threadIdx.x;
  const int c4n = C >> 2, rpb = BN_ROW_FLOATS / C;
  const int c0 = (tid % c4n) * 4, rr = tid / c4n;
  float mean[4], rstd[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    mean[i] = stat[c0 + i];
    rstd[i] = gent_rstd(stat[C + c0 + i], eps);
  }
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    const int64_t row = rg * rpb + rr;
    if (row < R) {
      const int64_t e = row * C + c0;
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + e);
      const f32x4 yv = *reinterpret_cast<const f32x4*>(y + e);
      const f32x4 dv = *reinterpret_cast<const f32x4*>(dy + e);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = yv[i] > 0.0f ? dv[i] : f_mul(dv[i], slope);
        const float xh = f_mul(f_sub(xv[i], mean[i]), rstd[i]);
        s[i] = f_add(s[i], (double)d);
        q[i] = f_add(q[i], f_mul((double)d, (double)xh));
      }
    }
  }
  bn_block_sums(s, q, C, part);
}

__global__ __launch_bounds__(256) void gent_bn_bwd_finish_kernel(const double* __restrict__ part, int blocks, int64_t R,
                                                                 int C, double* __restrict__ means,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = threadIdx.x;
  double s, q;
  bn_sum_partials(part, blocks, C, &s, &q);
  if (c >= C) return;
  dbeta[c] = (float)s;
  dgamma[c] = (float)q;
  means[c] = f_div(s, (double)R);
  means[C + c] = f_div(q, (double)R);
}

__global__ __launch_bounds__(256) void gent_bn_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dy, int64_t total, int C,
                                                             const float* __restrict__ stat, const float* __restrict__ gamma,
                                                             float eps, float slope, const double* __restrict__ means,
                                                             float* __restrict__ dx) {
  const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= total) return;
  const int c0 = (int)(e % C);
  const f32x4 xv = *reinterpret_cast<const f32x4*>(x + e);
  const f32x4 yv = *reinterpret_cast<const f32x4*>(y + e);
  const f32x4 dv = *reinterpret_cast<const f32x4*>(dy + e);
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + i;
    const float rstd = gent_rstd(stat[C + c], eps);
    const float d = yv[i] > 0.0f ? dv[i] : f_mul(dv[i], slope);
    const float xh = f_mul(f_sub(xv[i], stat[c]), rstd);
    const float m1 = (float)means[c], m2 = (float)means[C + c];
    o[i] = f_mul(f_mul(gamma[c], rstd), f_sub(f_sub(d, m1), f_mul(xh, m2)));
  }
  *reinterpret_cast<f32x4*>(dx + e) = o;
}

// ---- convolution data gradient, a gather: dx[b][s][ci] = sum_{t, co} dy[b][t][co] w[co][s - stride t][ci].  WLDS: the
// weights (at most DATA_LDS_FLOATS) are staged in LDS, else they are read from L2.
constexpr int DATA_LDS_FLOATS = 8192;

template <bool WLDS>
__global__ __launch_bounds__(256) void gent_conv_bwd_data_kernel(const float* __restrict__ dy, int64_t Tin, int Cin,
                                                                 const float* __restrict__ w, int Cout, int stride,
                                                                 int64_t T, int64_t total, float* __restrict__ dx) {
  __shared__ __attribute__((aligned(16))) float wl[WLDS ? DATA_LDS_FLOATS : 4];
  if (WLDS) {
    const int nw = Cout * TAPS * Cin;
    for (int i = threadIdx.x * 4; i < nw; i += 1024)
      *reinterpret_cast<f32x4*>(wl + i) = *reinterpret_cast<const f32x4*>(w + i);
    __syncthreads();
  }
  const float* wsrc = WLDS ? wl : w;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c4n = Cin >> 2;
  const int c4 = (int)(e % c4n);
  const int64_t bs = e / c4n;
  const int64_t b = bs / Tin, s = bs - b * Tin;
  const int64_t t_hi = min(T - 1, s / stride);
  const int64_t t_lo = s < TAPS ? 0 : (s - (TAPS - 1) + stride - 1) / stride;
  const int wstep = TAPS * Cin;
  f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t t = t_lo; t <= t_hi; ++t) {
    const int j = (int)(s - t * stride);                 // 0 <= j < 16 by the bounds of t
    const float* dyp = dy + (b * T + t) * Cout;
    const float* wp = wsrc + j * Cin + c4 * 4;
    for (int co = 0; co < Cout; co += 4) {               // (Cout % 16 == 0)
      const f32x4 d = *reinterpret_cast<const f32x4*>(dyp + co);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wp + (co + u) * wstep);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fmaf(d[u], wv[q], acc[q]);
      }
    }
  }
  *reinterpret_cast<f32x4*>(dx + (b * Tin + s) * Cin + c4 * 4) = acc;
}

// ---- dW / db slab partials on the matrix cores; ws [slabs][N K + N]
struct RowGradArgs {
  const float* dY;
  const float* X;
  float* ws;
  int64_t ldy, bstride, tstride, T, R, rows_per_slab, slab_floats;
  int N, K, shift, nkg;
};

template <int NT>
__global__ __launch_bounds__(64) void gent_rowgrad_kernel(RowGradArgs a) {
  constexpr int KT = 4;
  const int lane = threadIdx.x;
  const int i = lane & 15, g = lane >> 4;
  const int ng = blockIdx.x / a.nkg, kg = blockIdx.x - ng * a.nkg;
  const int n0 = ng * 16 * NT, k0 = kg * 16 * KT;
  const int64_t r_beg = (int64_t)blockIdx.y * a.rows_per_slab;
  const int64_t r_end = min(a.R, r_beg + a.rows_per_slab);
  f32x4 acc[NT][KT], accb[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    accb[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) acc[nt][kt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  for (int64_t r0 = r_beg; r0 < r_end; r0 += 16) {       // 16 rows per trip: the loads of four matrix steps in flight
    float av[4][NT], bv[4][KT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = r0 + 4 * u + g;
      const bool rv = r < r_end;
      const int64_t b = rv ? r / a.T : 0;
      const int64_t tt = (rv ? r - b * a.T : 0) + a.shift;
      const bool xv = rv && tt >= 0 && tt < a.T;
      const float* xp = a.X + (xv ? b * a.bstride + tt * a.tstride : 0);
      const float* yp = a.dY + (rv ? r * a.ldy : 0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + nt * 16 + i;
        av[u][nt] = (rv && n < a.N) ? yp[n] : 0.0f;
      }
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const int k = k0 + kt * 16 + i;
        bv[u][kt] = (xv && k < a.K) ? xp[k] : 0.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
          acc[nt][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][nt], bv[u][kt], acc[nt][kt], 0, 0, 0);
        if (kg == 0) accb[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][nt], 1.0f, accb[nt], 0, 0, 0);
      }
  }
  float* wsl = a.ws + (int64_t)blockIdx.y * a.slab_floats;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + nt * 16 + 4 * g + q;
      if (n >= a.N) continue;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const int k = k0 + kt * 16 + i;
        if (k < a.K) wsl[(int64_t)n * a.K + k] = acc[nt][kt][q];
      }
      if (kg == 0 && i == 0) wsl[(int64_t)a.N * a.K + n] = accb[nt][q];
    }
}

// Cin = 1 on the VALU; ws as above with K = 16.  Block (slab, cg) owns channels 8 cg .. 8 cg + 7 of one slab: a THREAD
// owns every 256th row of the slab and keeps all 8 x 16 products' sums (and the 8 bias sums) in registers - 24 loads for
// 128 multiply-adds - in f32 over its few rows; the block's 256 threads are then added per value in thread order in f64.
__device__ __forceinline__ double in1_block_sum(float (*sh)[257], double (*sh2)[8], int n_values) {
  // sh[a][thread] holds value a of every thread: lane l of a value's 8 adds threads 32 l .. 32 l + 31, then the lanes
  const int a = threadIdx.x >> 3, l = threadIdx.x & 7;
  __syncthreads();
  double s = 0.0;
  if (a < n_values)
    for (int k = 0; k < 32; ++k) s = f_add(s, (double)sh[a][l * 32 + k]);
  sh2[a][l] = s;
  __syncthreads();
  s = 0.0;
  if ((int)threadIdx.x < n_values)
    for (int k = 0; k < 8; ++k) s = f_add(s, sh2[threadIdx.x][k]);
  __syncthreads();                                       // (sh and sh2 are free again)
  return s;
}

__global__ __launch_bounds__(256) void gent_conv_in1_wgrad_kernel(const float* __restrict__ x, int64_t Tin,
                                                                  const float* __restrict__ dy, int Cout, int stride,
                                                                  int64_t T, int64_t R, int64_t rows_per_slab,
                                                                  int64_t slab_floats, float* __restrict__ ws) {
  __shared__ float sh[32][257];
  __shared__ double sh2[32][8];
  const int tid = threadIdx.x, cg = blockIdx.y;
  const int64_t r_beg = (int64_t)blockIdx.x * rows_per_slab;
  const int64_t r_end = min(R, r_beg + rows_per_slab);
  float acc[8][TAPS], accb[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    accb[c] = 0.0f;
#pragma unroll
    for (int j = 0; j < TAPS; ++j) acc[c][j] = 0.0f;
  }
  for (int64_t r = r_beg + tid; r < r_end; r += 256) {
    const int64_t b = r / T, t = r - b * T;
    const float* xp = x + b * Tin + t * stride;
    float xs[TAPS];
#pragma unroll
    for (int j = 0; j < TAPS; ++j) xs[j] = xp[j];
    const f32x4* dp = reinterpret_cast<const f32x4*>(dy + r * Cout + cg * 8);
    const f32x4 d0 = dp[0], d1 = dp[1];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float d = c < 4 ? d0[c & 3] : d1[c & 3];
      accb[c] = f_add(accb[c], d);
#pragma unroll
      for (int j = 0; j < TAPS; ++j) acc[c][j] = fmaf(d, xs[j], acc[c][j]);
    }
  }
  float* wsl = ws + (int64_t)blockIdx.x * slab_floats;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {                 // 2 channels x 16 taps per pass through LDS
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
      for (int j = 0; j < TAPS; ++j) sh[c2 * TAPS + j][tid] = acc[pass * 2 + c2][j];
    const double s = in1_block_sum(sh, sh2, 32);
    if (tid < 32) wsl[(cg * 8 + pass * 2 + (tid >> 4)) * TAPS + (tid & 15)] = (float)s;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) sh[c][tid] = accb[c];
  const double sb = in1_block_sum(sh, sh2, 8);
  if (tid < 8) wsl[Cout * TAPS + cg * 8 + tid] = (float)sb;
}

// out[e] = sum over the slabs in f64 in a fixed order: a block owns 16 values; lane k of a value's 16 adds slabs k, k + 16,
// .. in slab order, then the 16 lanes are added in lane order.  e < n_w goes to dw, the rest to db (optional)
__global__ __launch_bounds__(256) void gent_reduce_kernel(const float* __restrict__ ws, int slabs, int64_t slab_floats,
                                                          int64_t n_w, float* __restrict__ dw, float* __restrict__ db) {
  __shared__ double sh[16][16];
  const int el = threadIdx.x & 15, lane = threadIdx.x >> 4;
  const int64_t e = (int64_t)blockIdx.x * 16 + el;
  double s = 0.0;
  if (e < slab_floats)
    for (int s0 = lane; s0 < slabs; s0 += 64) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = s0 + 16 * u < slabs ? ws[(int64_t)(s0 + 16 * u) * slab_floats + e] : 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u) s = f_add(s, (double)v[u]);
    }
  sh[lane][el] = s;
  __syncthreads();
  if (lane != 0 || e >= slab_floats) return;
  s = 0.0;
  for (int k = 0; k < 16; ++k) s = f_add(s, sh[k][el]);
  if (e < n_w) dw[e] = (float)s;
  else if (db) db[e - n_w] = (float)s;
}

// ---- the recurrence, training forward: gen_gru_kernel of qpg_gen.hip plus sv [B][T][2][4][H] = r, z, n, W_hn h + b_hn
__device__ __forceinline__ float gent_sigmoid(float v) { return f_div(1.0f, f_add(1.0f, expf(-v))); }

__global__ __launch_bounds__(GWAVES * 64) void gent_gru_fwd_kernel(const float* __restrict__ xp, const float* __restrict__ whh,
                                                                   const float* __restrict__ bhh, int B, int T,
                                                                   float* __restrict__ out, float* __restrict__ sv) {
  __shared__ __attribute__((aligned(16))) float hs[2][GBT][HS_LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y;
  const int j = lane & 15, g = lane >> 4;
  const int ua = min(wv * 16 + j, GH - 1);
  const float* wrow[3];
#pragma unroll
  for (int gate = 0; gate < 3; ++gate) wrow[gate] = whh + ((int64_t)(dir * 3 + gate) * GH + ua) * GH + 4 * g;
  const int u0 = wv * 16 + 4 * g;
  const bool uvalid = u0 < GH;
  const int64_t seq = (int64_t)blockIdx.x * GBT + j;
  const bool svalid = seq < B;
  const int64_t seqc = svalid ? seq : B - 1;
  const float* bhp = bhh + dir * 3 * GH + u0;
  for (int i = tid; i < 2 * GBT * HS_LD; i += GWAVES * 64) (&hs[0][0][0])[i] = 0.0f;
  __syncthreads();

  for (int step = 0; step < T; ++step) {
    const int t = dir ? T - 1 - step : step;
    const int cur = step & 1;
    f32x4 xg[3];
    const float* xrow = xp + ((seqc * T + t) * 2 + dir) * (3 * GH) + u0;
#pragma unroll
    for (int gate = 0; gate < 3; ++gate)
      xg[gate] = uvalid ? *reinterpret_cast<const f32x4*>(xrow + gate * GH) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 acc[3];
#pragma unroll
    for (int gate = 0; gate < 3; ++gate) acc[gate] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4 zero = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int c0 = 0; c0 < KCH; c0 += 4) {
      f32x4 hb[4], a[4][3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k0 = (c0 + i) * 16 + 4 * g;
        const bool kvalid = k0 < GH;
        hb[i] = kvalid ? *reinterpret_cast<const f32x4*>(&hs[cur][j][k0]) : zero;
#pragma unroll
        for (int gate = 0; gate < 3; ++gate)
          a[i][gate] = kvalid ? *reinterpret_cast<const f32x4*>(wrow[gate] + (c0 + i) * 16) : zero;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int gate = 0; gate < 3; ++gate)
            acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][gate][q], hb[i][q], acc[gate], 0, 0, 0);
    }
    if (uvalid) {
      const f32x4 hp = *reinterpret_cast<const f32x4*>(&hs[cur][j][u0]);
      f32x4 bh[3];
#pragma unroll
      for (int gate = 0; gate < 3; ++gate) bh[gate] = *reinterpret_cast<const f32x4*>(bhp + gate * GH);
      f32x4 hn, sr, sz, sn, sh;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float rr = gent_sigmoid(f_add(xg[0][r], f_add(acc[0][r], bh[0][r])));
        const float zz = gent_sigmoid(f_add(xg[1][r], f_add(acc[1][r], bh[1][r])));
        const float hh = f_add(acc[2][r], bh[2][r]);
        const float nn = tanhf(f_add(xg[2][r], f_mul(rr, hh)));
        hn[r] = f_add(f_mul(f_sub(1.0f, zz), nn), f_mul(zz, hp[r]));
        sr[r] = rr;
        sz[r] = zz;
        sn[r] = nn;
        sh[r] = hh;
      }
      *reinterpret_cast<f32x4*>(&hs[cur ^ 1][j][u0]) = hn;
      if (svalid) {
        *reinterpret_cast<f32x4*>(out + (seq * T + t) * (2 * GH) + dir * GH + u0) = hn;
        float* sp = sv + ((seq * T + t) * 2 + dir) * (4 * GH) + u0;
        *reinterpret_cast<f32x4*>(sp) = sr;
        *reinterpret_cast<f32x4*>(sp + GH) = sz;
        *reinterpret_cast<f32x4*>(sp + 2 * GH) = sn;
        *reinterpret_cast<f32x4*>(sp + 3 * GH) = sh;
      }
    }
    __syncthreads();
  }
}

// ---- backpropagation through time.  dout [B][T][2 H], sv as above, out the layer's forward output, whhT [2][H][3 H];
// dxp, dgh [B][T][2][3 H].  The walk is the forward's in reverse; h of the forward's previous step is out[t -+ 1].
__global__ __launch_bounds__(GWAVES * 64) void gent_gru_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ sv,
                                                                   const float* __restrict__ out,
                                                                   const float* __restrict__ whhT, int B, int T,
                                                                   float* __restrict__ dxp, float* __restrict__ dgh) {
  __shared__ __attribute__((aligned(16))) float dg[GBT][DG_LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y;
  const int j = lane & 15, g = lane >> 4;
  // A operand: row k = 16 wv + j of W_hh^T (past the end: row H - 1, its results land in rows nobody keeps)
  const int ka = min(wv * 16 + j, GH - 1);
  const float* wrow = whhT + ((int64_t)dir * GH + ka) * G3 + 4 * g;
  const int u0 = wv * 16 + 4 * g;
  const bool uvalid = u0 < GH;
  const int64_t seq = (int64_t)blockIdx.x * GBT + j;
  const bool svalid = seq < B;
  const int64_t seqc = svalid ? seq : B - 1;
  const f32x4 zero = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 dh = zero;                                       // d loss / d h of the step, units u0 .. u0 + 3 of sequence j

  for (int step = T - 1; step >= 0; --step) {
    const int t = dir ? T - 1 - step : step;
    f32x4 keep = zero;                                   // dh z: the part of dh that passes straight to the previous step
    if (uvalid) {
      const int64_t row = seqc * T + t;
      const f32x4 go = *reinterpret_cast<const f32x4*>(dout + row * (2 * GH) + dir * GH + u0);
      const float* sp = sv + (row * 2 + dir) * (4 * GH) + u0;
      const f32x4 sr = *reinterpret_cast<const f32x4*>(sp);
      const f32x4 sz = *reinterpret_cast<const f32x4*>(sp + GH);
      const f32x4 sn = *reinterpret_cast<const f32x4*>(sp + 2 * GH);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(sp + 3 * GH);
      f32x4 hp = zero;
      if (step > 0) {
        const int tp = dir ? t + 1 : t - 1;
        hp = *reinterpret_cast<const f32x4*>(out + (seqc * T + tp) * (2 * GH) + dir * GH + u0);
      }
      f32x4 ar, az, an, gn;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = f_add(go[r], dh[r]);
        const float dn = f_mul(d, f_sub(1.0f, sz[r]));
        const float dz = f_mul(d, f_sub(hp[r], sn[r]));
        keep[r] = f_mul(d, sz[r]);
        an[r] = f_mul(dn, f_sub(1.0f, f_mul(sn[r], sn[r])));
        ar[r] = f_mul(f_mul(f_mul(an[r], sh[r]), sr[r]), f_sub(1.0f, sr[r]));
        az[r] = f_mul(f_mul(dz, sz[r]), f_sub(1.0f, sz[r]));
        gn[r] = f_mul(an[r], sr[r]);
      }
      *reinterpret_cast<f32x4*>(&dg[j][u0]) = ar;
      *reinterpret_cast<f32x4*>(&dg[j][GH + u0]) = az;
      *reinterpret_cast<f32x4*>(&dg[j][2 * GH + u0]) = gn;
      if (svalid) {
        const int64_t o = (row * 2 + dir) * G3 + u0;
        *reinterpret_cast<f32x4*>(dxp + o) = ar;
        *reinterpret_cast<f32x4*>(dxp + o + GH) = az;
        *reinterpret_cast<f32x4*>(dxp + o + 2 * GH) = an;
        *reinterpret_cast<f32x4*>(dgh + o) = ar;
        *reinterpret_cast<f32x4*>(dgh + o + GH) = az;
        *reinterpret_cast<f32x4*>(dgh + o + 2 * GH) = gn;
      }
    }
    __syncthreads();                                     // the step's dgh is complete
    f32x4 acc = zero;
    if (step > 0) {                                      // (uniform: the first step's dh goes nowhere)
#pragma unroll 1
      for (int c0 = 0; c0 < KCH3; c0 += 4) {
        f32x4 hb[4], a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k0 = (c0 + i) * 16 + 4 * g;
          const bool kvalid = (c0 + i) < KCH3 && k0 < G3;
          hb[i] = kvalid ? *reinterpret_cast<const f32x4*>(&dg[j][k0]) : zero;
          a[i] = kvalid ? *reinterpret_cast<const f32x4*>(wrow + (c0 + i) * 16) : zero;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][q], hb[i][q], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dh[r] = f_add(keep[r], acc[r]);
    __syncthreads();                                     // nobody still reads the dgh the next step overwrites
  }
}

__device__ __forceinline__ float gent_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = f_add(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- direction sum + LayerNorm backward.  dy [R][HLD], x [R][2 H]; dx [R][2 H] (both halves the same); ws [slabs][2 H]
__global__ __launch_bounds__(256) void gent_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ gm, int64_t R, int64_t rows_per_slab,
                                                          float eps, float* __restrict__ dx, float* __restrict__ ws) {
  __shared__ double sh[4][2][GH];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r_beg = (int64_t)blockIdx.x * rows_per_slab;
  const int64_t r_end = min(R, r_beg + rows_per_slab);
  double ag[4] = {0.0, 0.0, 0.0, 0.0}, ab[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t row = r_beg + wv; row < r_end; row += 4) {
    const float* xr = x + row * (2 * GH);
    const float* dr = dy + row * HLD;
    float v[4], s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      v[i] = c < GH ? f_add(xr[c], xr[GH + c]) : 0.0f;
      s = f_add(s, v[i]);
    }
    const float mean = f_div(gent_wave_sum(s), (float)GH);
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float d = lane + 64 * i < GH ? f_sub(v[i], mean) : 0.0f;
      q = fmaf(d, d, q);
    }
    const float rstd = f_div(1.0f, f_sqrt(f_add(f_div(gent_wave_sum(q), (float)GH), eps)));
    float xh[4], dh[4], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      const bool ok = c < GH;
      const float d = ok ? dr[c] : 0.0f;
      xh[i] = ok ? f_mul(f_sub(v[i], mean), rstd) : 0.0f;
      dh[i] = ok ? f_mul(d, gm[c]) : 0.0f;
      s1 = f_add(s1, dh[i]);
      s2 = fmaf(dh[i], xh[i], s2);
      ag[i] = f_add(ag[i], f_mul((double)d, (double)xh[i]));
      ab[i] = f_add(ab[i], (double)d);
    }
    const float m1 = f_div(gent_wave_sum(s1), (float)GH), m2 = f_div(gent_wave_sum(s2), (float)GH);
    float* ox = dx + row * (2 * GH);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      if (c < GH) {
        const float o = f_mul(rstd, f_sub(f_sub(dh[i], m1), f_mul(xh[i], m2)));
        ox[c] = o;
        ox[GH + c] = o;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < GH) {
      sh[wv][0][c] = ag[i];
      sh[wv][1][c] = ab[i];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * GH; e += 256) {
    const int which = e / GH, c = e - which * GH;
    double s = 0.0;
    for (int w = 0; w < 4; ++w) s = f_add(s, sh[w][which][c]);
    ws[(int64_t)blockIdx.x * (2 * GH) + e] = (float)s;
  }
}

// ---- dlogits[r][c] = (softmax(l[r])[c] - (c == target[r])) / R; a target outside [0, N) gives a NaN row
__global__ __launch_bounds__(256) void gent_ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                          int64_t R, int N, float inv_r, float* __restrict__ dl) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* lr = logits + row * N;
  float m = -INFINITY;
  for (int c = lane; c < N; c += 64) m = fmaxf(m, lr[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float s = 0.0f;
  for (int c = lane; c < N; c += 64) s = f_add(s, expf(f_sub(lr[c], m)));
  s = gent_wave_sum(s);
  const int64_t tg = target[row];
  const bool ok = tg >= 0 && tg < N;
  float* dr = dl + row * N;
  for (int c = lane; c < N; c += 64) {
    const float p = f_div(expf(f_sub(lr[c], m)), s);
    dr[c] = ok ? f_mul(f_sub(p, c == tg ? 1.0f : 0.0f), inv_r) : __builtin_nanf("");
  }
}

__global__ __launch_bounds__(256) void gent_dropout_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                           int64_t n, float scale, float* __restrict__ y) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  y[e] = mask[e] ? f_mul(x[e], scale) : 0.0f;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// slabs and rows per slab of R rows for a workspace of ws_floats: at most MAX_SLABS, none under SLAB_MIN_ROWS rows
// (but one), as many as the workspace holds
inline void slab_plan(int64_t R, int64_t slab_floats, int64_t ws_floats, int* slabs, int64_t* rows) {
  int64_t s = ws_floats / slab_floats;
  s = std::min<int64_t>(s, MAX_SLABS);
  s = std::min<int64_t>(s, (R + SLAB_MIN_ROWS - 1) / SLAB_MIN_ROWS);
  s = std::max<int64_t>(s, 1);
  int64_t rp = (R + s - 1) / s;
  rp = (rp + 3) / 4 * 4;
  *rows = rp;
  *slabs = (int)((R + rp - 1) / rp);
}

inline int64_t bn_groups(int64_t R, int C) { return (R + BN_ROW_FLOATS / C - 1) / (BN_ROW_FLOATS / C); }

inline int bn_blocks(int64_t R, int C) { return (int)std::min<int64_t>(bn_groups(R, C), BN_MAX_BLOCKS); }

}  // namespace

#define GENT_UNSUP(cond, ...)       \
  do {                              \
    if (!(cond)) {                  \
      qpg_set_error(__VA_ARGS__);   \
      return QPG_EUNSUP;            \
    }                               \
  } while (0)

static inline bool gent_bn_channels(int C) { return C == 8 || C == 16 || C == 32 || C == 64; }

extern "C" int64_t qpg_gen_bn_ws_floats(int64_t R, int C) {
  if (R < 1 || !gent_bn_channels(C)) return 0;
  return 2 * ((int64_t)bn_blocks(R, C) * 2 * C + 2 * C);
}

extern "C" int qpg_gen_bn_stats_f32(qpg_ctx* ctx, void* stream, const float* x, int64_t R, int C, float* ws,
                                    int64_t ws_floats, float* stat, float* running_mean, float* running_var,
                                    float momentum) {
  QPG_REQUIRE(ctx, "qpg_gen_bn_stats_f32: null context");
  QPG_REQUIRE(x && ws && stat, "qpg_gen_bn_stats_f32: null pointer argument");
  QPG_REQUIRE(((uintptr_t)x & 15) == 0, "qpg_gen_bn_stats_f32: x must be 16-byte aligned");
  QPG_REQUIRE(R >= 2 && R <= ((int64_t)1 << 40), "qpg_gen_bn_stats_f32: need 2 <= R <= 2^40 rows (R %lld): a batch of one "
              "value per channel has no variance", (long long)R);
  GENT_UNSUP(gent_bn_channels(C), "qpg_gen_bn_stats_f32: C %d is not 8, 16, 32 or 64", C);
  QPG_REQUIRE(((uintptr_t)ws & 7) == 0 && ws_floats >= qpg_gen_bn_ws_floats(R, C),
              "qpg_gen_bn_stats_f32: ws must be 8-byte aligned and hold %lld floats (got %lld)",
              (long long)qpg_gen_bn_ws_floats(R, C), (long long)ws_floats);
  hipStream_t s = qpg_stream(stream);
  const int blocks = bn_blocks(R, C);
  const int64_t groups = bn_groups(R, C);
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(gent_bn_part_kernel, dim3(blocks), dim3(256), 0, s, x, R, C, groups, part);
  QPG_LAUNCH_CHECK("gent_bn_part_kernel");
  hipLaunchKernelGGL(gent_bn_finish_kernel, dim3(1), dim3(256), 0, s, part, blocks, R, C, stat, running_mean, running_var,
                     momentum);
  QPG_LAUNCH_CHECK("gent_bn_finish_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_bn_apply_f32(qpg_ctx* ctx, void* stream, const float* x, int64_t R, int C, const float* stat,
                                    const float* gamma, const float* beta, float eps, float slope, float* y) {
  QPG_REQUIRE(ctx, "qpg_gen_bn_apply_f32: null context");
  QPG_REQUIRE(x && stat && gamma && beta && y, "qpg_gen_bn_apply_f32: null pointer argument");
  QPG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "qpg_gen_bn_apply_f32: x and y must be 16-byte aligned");
  QPG_REQUIRE(R >= 1 && R <= ((int64_t)1 << 40), "qpg_gen_bn_apply_f32: need 1 <= R <= 2^40 rows (R %lld)", (long long)R);
  GENT_UNSUP(gent_bn_channels(C), "qpg_gen_bn_apply_f32: C %d is not 8, 16, 32 or 64", C);
  const int64_t total = R * C;
  QPG_REQUIRE(blocks_of(total) == (total + 255) / 256, "qpg_gen_bn_apply_f32: %lld values are too many", (long long)total);
  hipLaunchKernelGGL(gent_bn_apply_kernel, dim3(blocks_of(total / 4)), dim3(256), 0, qpg_stream(stream), x, total, C, stat, gamma,
                     beta, eps, slope, y);
  QPG_LAUNCH_CHECK("gent_bn_apply_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_bn_backward_f32(qpg_ctx* ctx, void* stream, const float* x, const float* y, const float* dy, int64_t R,
                                       int C, const float* stat, const float* gamma, float eps, float slope, float* ws,
                                       int64_t ws_floats, float* dgamma, float* dbeta, float* dx) {
  QPG_REQUIRE(ctx, "qpg_gen_bn_backward_f32: null context");
  QPG_REQUIRE(x && y && dy && stat && gamma && ws && dgamma && dbeta && dx, "qpg_gen_bn_backward_f32: null pointer argument");
  QPG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)dx & 15) == 0,
              "qpg_gen_bn_backward_f32: x, y, dy and dx must be 16-byte aligned");
  QPG_REQUIRE(R >= 2 && R <= ((int64_t)1 << 40), "qpg_gen_bn_backward_f32: need 2 <= R <= 2^40 rows (R %lld)", (long long)R);
  GENT_UNSUP(gent_bn_channels(C), "qpg_gen_bn_backward_f32: C %d is not 8, 16, 32 or 64", C);
  QPG_REQUIRE(((uintptr_t)ws & 7) == 0 && ws_floats >= qpg_gen_bn_ws_floats(R, C),
              "qpg_gen_bn_backward_f32: ws must be 8-byte aligned and hold %lld floats (got %lld)",
              (long long)qpg_gen_bn_ws_floats(R, C), (long long)ws_floats);
  const int64_t total = R * C;
  QPG_REQUIRE(blocks_of(total) == (total + 255) / 256, "qpg_gen_bn_backward_f32: %lld values are too many", (long long)total);
  hipStream_t s = qpg_stream(stream);
  const int blocks = bn_blocks(R, C);
  const int64_t groups = bn_groups(R, C);
  double* part = reinterpret_cast<double*>(ws);
  double* means = part + (int64_t)blocks * 2 * C;
  hipLaunchKernelGGL(gent_bn_bwd_part_kernel, dim3(blocks), dim3(256), 0, s, x, y, dy, R, C, groups, stat, eps, slope, part);
  QPG_LAUNCH_CHECK("gent_bn_bwd_part_kernel");
  hipLaunchKernelGGL(gent_bn_bwd_finish_kernel, dim3(1), dim3(256), 0, s, part, blocks, R, C, means, dgamma, dbeta);
  QPG_LAUNCH_CHECK("gent_bn_bwd_finish_kernel");
  hipLaunchKernelGGL(gent_bn_bwd_dx_kernel, dim3(blocks_of(total / 4)), dim3(256), 0, s, x, y, dy, total, C, stat, gamma, eps,
                     slope, means, dx);
  QPG_LAUNCH_CHECK("gent_bn_bwd_dx_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_conv1d_bwd_data_f32(qpg_ctx* ctx, void* stream, const float* dy, int B, int64_t Tin, int Cin,
                                           const float* w, int Cout, int stride, float* dx) {
  QPG_REQUIRE(ctx, "qpg_gen_conv1d_bwd_data_f32: null context");
  QPG_REQUIRE(dy && w && dx, "qpg_gen_conv1d_bwd_data_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && B <= 65535 && Cin >= 1 && Cout >= 1 && stride >= 1 && Tin >= TAPS && Tin <= ((int64_t)1 << 31),
              "qpg_gen_conv1d_bwd_data_f32: need 1 <= B <= 65535, Cin, Cout, stride >= 1 and %d <= Tin <= 2^31 (B %d, Cin %d, "
              "Cout %d, stride %d, Tin %lld)", TAPS, B, Cin, Cout, stride, (long long)Tin);
  GENT_UNSUP(gent_bn_channels(Cin) && Cout % 16 == 0 && Cout <= 64 && (stride == 3 || stride == 6),
             "qpg_gen_conv1d_bwd_data_f32: Cin %d must be 8, 16, 32 or 64, Cout %d a multiple of 16 up to 64, stride %d 3 or 6",
             Cin, Cout, stride);
  QPG_REQUIRE(((uintptr_t)w & 15) == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)dy & 15) == 0,
              "qpg_gen_conv1d_bwd_data_f32: dy, w and dx must be 16-byte aligned");
  const int64_t T = qpg_gen_conv_frames(Tin, stride);
  const int64_t total = (int64_t)B * Tin * (Cin / 4);
  QPG_REQUIRE(total <= ((int64_t)1 << 38), "qpg_gen_conv1d_bwd_data_f32: %lld outputs are too many", (long long)total);
  if (Cout * TAPS * Cin <= DATA_LDS_FLOATS)
    hipLaunchKernelGGL(gent_conv_bwd_data_kernel<true>, dim3(blocks_of(total)), dim3(256), 0, qpg_stream(stream), dy, Tin,
                       Cin, w, Cout, stride, T, total, dx);
  else
    hipLaunchKernelGGL(gent_conv_bwd_data_kernel<false>, dim3(blocks_of(total)), dim3(256), 0, qpg_stream(stream), dy, Tin,
                       Cin, w, Cout, stride, T, total, dx);
  QPG_LAUNCH_CHECK("gent_conv_bwd_data_kernel");
  return QPG_OK;
}

extern "C" int64_t qpg_gen_rowgrad_ws_floats(int N, int K, int slabs) {
  if (N < 1 || K < 1 || slabs < 1) return 0;
  return (int64_t)std::min(slabs, MAX_SLABS) * ((int64_t)N * K + N);
}

extern "C" int64_t qpg_gen_conv1d_wgrad_ws_floats(int Cin, int Cout, int slabs) {
  return qpg_gen_rowgrad_ws_floats(Cout, TAPS * Cin, slabs);
}

// the shared back half: slab partials by the matrix-core kernel, then the ordered f64 sum
static int gent_rowgrad_launch(hipStream_t s, const char* who, RowGradArgs a, float* dW, float* db, int64_t ws_floats) {
  a.slab_floats = (int64_t)a.N * a.K + a.N;
  int slabs;
  slab_plan(a.R, a.slab_floats, ws_floats, &slabs, &a.rows_per_slab);
  const int nt = a.N <= 16 ? 1 : a.N <= 32 ? 2 : 4;
  a.nkg = (a.K + 63) / 64;
  const dim3 grid((unsigned)(((a.N + 16 * nt - 1) / (16 * nt)) * a.nkg), (unsigned)slabs);
  switch (nt) {
    case 1: hipLaunchKernelGGL(gent_rowgrad_kernel<1>, grid, dim3(64), 0, s, a); break;
    case 2: hipLaunchKernelGGL(gent_rowgrad_kernel<2>, grid, dim3(64), 0, s, a); break;
    default: hipLaunchKernelGGL(gent_rowgrad_kernel<4>, grid, dim3(64), 0, s, a); break;
  }
  QPG_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(gent_reduce_kernel, dim3((unsigned)((a.slab_floats + 15) / 16)), dim3(256), 0, s, a.ws, slabs, a.slab_floats,
                     (int64_t)a.N * a.K, dW, db);
  QPG_LAUNCH_CHECK("gent_reduce_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_conv1d_bwd_weight_f32(qpg_ctx* ctx, void* stream, const float* x, int B, int64_t Tin, int Cin,
                                             const float* dy, int Cout, int stride, float* dw, float* db, float* ws,
                                             int64_t ws_floats) {
  QPG_REQUIRE(ctx, "qpg_gen_conv1d_bwd_weight_f32: null context");
  QPG_REQUIRE(x && dy && dw && db && ws, "qpg_gen_conv1d_bwd_weight_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && B <= 65535 && Cin >= 1 && Cout >= 1 && stride >= 1 && Tin >= TAPS && Tin <= ((int64_t)1 << 31),
              "qpg_gen_conv1d_bwd_weight_f32: need 1 <= B <= 65535, Cin, Cout, stride >= 1 and %d <= Tin <= 2^31 (B %d, Cin "
              "%d, Cout %d, stride %d, Tin %lld)", TAPS, B, Cin, Cout, stride, (long long)Tin);
  GENT_UNSUP((Cin == 1 && Cout % 8 == 0 && Cout <= 64) || (Cin % 4 == 0 && Cin <= 64 && Cout % 16 == 0 && Cout <= 64),
             "qpg_gen_conv1d_bwd_weight_f32: Cin %d must be 1 (Cout a multiple of 8) or a multiple of 4 (Cout of 16), both up "
             "to 64 (Cout %d)", Cin, Cout);
  const int64_t slab_floats = (int64_t)Cout * TAPS * Cin + Cout;
  QPG_REQUIRE(ws_floats >= slab_floats, "qpg_gen_conv1d_bwd_weight_f32: ws holds %lld floats, one slab needs %lld",
              (long long)ws_floats, (long long)slab_floats);
  const int64_t T = qpg_gen_conv_frames(Tin, stride);
  const int64_t R = (int64_t)B * T;
  hipStream_t s = qpg_stream(stream);
  QPG_REQUIRE(((uintptr_t)dy & 15) == 0, "qpg_gen_conv1d_bwd_weight_f32: dy must be 16-byte aligned");
  if (Cin == 1) {
    int slabs;
    int64_t rows;
    slab_plan(R, slab_floats, ws_floats, &slabs, &rows);
    hipLaunchKernelGGL(gent_conv_in1_wgrad_kernel, dim3(slabs, Cout / 8), dim3(256), 0, s, x, Tin, dy, Cout, stride, T, R, rows,
                       slab_floats, ws);
    QPG_LAUNCH_CHECK("gent_conv_in1_wgrad_kernel");
    hipLaunchKernelGGL(gent_reduce_kernel, dim3((unsigned)((slab_floats + 15) / 16)), dim3(256), 0, s, ws, slabs, slab_floats,
                       (int64_t)Cout * TAPS, dw, db);
    QPG_LAUNCH_CHECK("gent_reduce_kernel");
    return QPG_OK;
  }
  RowGradArgs a;
  a.dY = dy; a.X = x; a.ws = ws;
  a.ldy = Cout; a.bstride = Tin * Cin; a.tstride = (int64_t)stride * Cin; a.T = T; a.R = R;
  a.N = Cout; a.K = TAPS * Cin; a.shift = 0;
  return gent_rowgrad_launch(s, "gent_rowgrad_kernel (convolution)", a, dw, db, ws_floats);
}

extern "C" int qpg_gen_rowgrad_f32(qpg_ctx* ctx, void* stream, const float* dY, int64_t ldy, const float* X, int64_t ldx,
                                   int64_t R, int N, int K, int shift, int64_t T, float* dW, float* db, float* ws,
                                   int64_t ws_floats) {
  QPG_REQUIRE(ctx, "qpg_gen_rowgrad_f32: null context");
  QPG_REQUIRE(dY && X && dW && ws, "qpg_gen_rowgrad_f32: null pointer argument");
  QPG_REQUIRE(R >= 1 && R <= ((int64_t)1 << 40) && N >= 1 && K >= 1 && ldy >= N && ldx >= K && T >= 1,
              "qpg_gen_rowgrad_f32: need R, N, K, T >= 1, ldy >= N, ldx >= K (R %lld, N %d, K %d, ldy %lld, ldx %lld, T %lld)",
              (long long)R, N, K, (long long)ldy, (long long)ldx, (long long)T);
  QPG_REQUIRE(shift >= -1 && shift <= 1 && (shift == 0 || R % T == 0),
              "qpg_gen_rowgrad_f32: shift %d must be -1, 0 or 1, and with a shift R %lld a multiple of the period %lld", shift,
              (long long)R, (long long)T);
  GENT_UNSUP(N <= 4096 && K <= 4096, "qpg_gen_rowgrad_f32: N %d, K %d: at most 4096 each", N, K);
  const int64_t slab_floats = (int64_t)N * K + N;
  QPG_REQUIRE(ws_floats >= slab_floats, "qpg_gen_rowgrad_f32: ws holds %lld floats, one slab needs %lld", (long long)ws_floats,
              (long long)slab_floats);
  RowGradArgs a;
  a.dY = dY; a.X = X; a.ws = ws;
  a.ldy = ldy; a.tstride = ldx; a.R = R;
  a.N = N; a.K = K; a.shift = shift;
  if (shift == 0) {                                      // (no period: one batch member of R rows)
    a.T = R;
    a.bstride = 0;
  } else {
    a.T = T;
    a.bstride = T * ldx;
  }
  return gent_rowgrad_launch(qpg_stream(stream), "gent_rowgrad_kernel", a, dW, db, ws_floats);
}

extern "C" int qpg_gen_gru_layer_train_f32(qpg_ctx* ctx, void* stream, const float* xp, const float* whh, const float* bhh,
                                           int B, int T, int H, float* out, float* saved) {
  QPG_REQUIRE(ctx, "qpg_gen_gru_layer_train_f32: null context");
  QPG_REQUIRE(xp && whh && bhh && out && saved, "qpg_gen_gru_layer_train_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && T >= 1 && H >= 1, "qpg_gen_gru_layer_train_f32: need B, T, H >= 1 (B %d, T %d, H %d)", B, T, H);
  GENT_UNSUP(H == GH, "qpg_gen_gru_layer_train_f32: hidden width %d, the kernel is built for %d", H, GH);
  QPG_REQUIRE(((uintptr_t)xp & 15) == 0 && ((uintptr_t)whh & 15) == 0 && ((uintptr_t)bhh & 15) == 0 &&
              ((uintptr_t)out & 15) == 0 && ((uintptr_t)saved & 15) == 0,
              "qpg_gen_gru_layer_train_f32: xp, whh, bhh, out and saved must be 16-byte aligned");
  hipLaunchKernelGGL(gent_gru_fwd_kernel, dim3((unsigned)((B + GBT - 1) / GBT), 2), dim3(GWAVES * 64), 0, qpg_stream(stream),
                     xp, whh, bhh, B, T, out, saved);
  QPG_LAUNCH_CHECK("gent_gru_fwd_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_gru_layer_backward_f32(qpg_ctx* ctx, void* stream, const float* dout, const float* saved,
                                              const float* out, const float* whhT, int B, int T, int H, float* dxp,
                                              float* dgh) {
  QPG_REQUIRE(ctx, "qpg_gen_gru_layer_backward_f32: null context");
  QPG_REQUIRE(dout && saved && out && whhT && dxp && dgh, "qpg_gen_gru_layer_backward_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && T >= 1 && H >= 1, "qpg_gen_gru_layer_backward_f32: need B, T, H >= 1 (B %d, T %d, H %d)", B, T, H);
  GENT_UNSUP(H == GH, "qpg_gen_gru_layer_backward_f32: hidden width %d, the kernel is built for %d", H, GH);
  QPG_REQUIRE(((uintptr_t)dout & 15) == 0 && ((uintptr_t)saved & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
              ((uintptr_t)whhT & 15) == 0 && ((uintptr_t)dxp & 15) == 0 && ((uintptr_t)dgh & 15) == 0,
              "qpg_gen_gru_layer_backward_f32: every pointer must be 16-byte aligned");
  hipLaunchKernelGGL(gent_gru_bwd_kernel, dim3((unsigned)((B + GBT - 1) / GBT), 2), dim3(GWAVES * 64), 0, qpg_stream(stream),
                     dout, saved, out, whhT, B, T, dxp, dgh);
  QPG_LAUNCH_CHECK("gent_gru_bwd_kernel");
  return QPG_OK;
}

extern "C" int64_t qpg_gen_head_ln_bwd_ws_floats(int64_t R) {
  if (R < 1) return 0;
  return std::min<int64_t>(MAX_SLABS, (R + SLAB_MIN_ROWS - 1) / SLAB_MIN_ROWS) * 2 * GH;
}

extern "C" int qpg_gen_head_ln_backward_f32(qpg_ctx* ctx, void* stream, const float* dy, const float* x, const float* gamma,
                                            int64_t R, int H, float eps, float* ws, int64_t ws_floats, float* dgamma,
                                            float* dbeta, float* dx) {
  QPG_REQUIRE(ctx, "qpg_gen_head_ln_backward_f32: null context");
  QPG_REQUIRE(dy && x && gamma && ws && dgamma && dbeta && dx, "qpg_gen_head_ln_backward_f32: null pointer argument");
  QPG_REQUIRE(R >= 1 && R <= ((int64_t)1 << 32) && H >= 1, "qpg_gen_head_ln_backward_f32: need 1 <= R <= 2^32 rows and H >= 1 "
              "(R %lld, H %d)", (long long)R, H);
  GENT_UNSUP(H == GH, "qpg_gen_head_ln_backward_f32: hidden width %d, the kernel is built for %d", H, GH);
  QPG_REQUIRE(ws_floats >= 2 * GH, "qpg_gen_head_ln_backward_f32: ws holds %lld floats, one slab needs %d",
              (long long)ws_floats, 2 * GH);
  QPG_REQUIRE(dbeta == dgamma + GH, "qpg_gen_head_ln_backward_f32: dbeta must follow dgamma (dgamma + H)");
  int slabs;
  int64_t rows;
  slab_plan(R, 2 * GH, ws_floats, &slabs, &rows);
  hipStream_t s = qpg_stream(stream);
  hipLaunchKernelGGL(gent_ln_bwd_kernel, dim3(slabs), dim3(256), 0, s, dy, x, gamma, R, rows, eps, dx, ws);
  QPG_LAUNCH_CHECK("gent_ln_bwd_kernel");
  hipLaunchKernelGGL(gent_reduce_kernel, dim3((unsigned)((2 * GH + 15) / 16)), dim3(256), 0, s, ws, slabs, (int64_t)2 * GH, (int64_t)2 * GH,
                     dgamma, (float*)nullptr);
  QPG_LAUNCH_CHECK("gent_reduce_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_cross_entropy_backward_f32(qpg_ctx* ctx, void* stream, const float* logits, const int64_t* target,
                                                  int64_t R, int N, float* dlogits) {
  QPG_REQUIRE(ctx, "qpg_gen_cross_entropy_backward_f32: null context");
  QPG_REQUIRE(logits && target && dlogits, "qpg_gen_cross_entropy_backward_f32: null pointer argument");
  QPG_REQUIRE(R >= 1 && R <= ((int64_t)1 << 32) && N >= 1, "qpg_gen_cross_entropy_backward_f32: need 1 <= R <= 2^32 rows of "
              "N >= 1 (R %lld, N %d)", (long long)R, N);
  hipLaunchKernelGGL(gent_ce_bwd_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, qpg_stream(stream), logits, target, R, N,
                     (float)(1.0 / (double)R), dlogits);
  QPG_LAUNCH_CHECK("gent_ce_bwd_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_dropout_f32(qpg_ctx* ctx, void* stream, const float* x, const uint8_t* mask, int64_t n, float scale,
                                   float* y) {
  QPG_REQUIRE(ctx, "qpg_gen_dropout_f32: null context");
  QPG_REQUIRE(x && mask && y, "qpg_gen_dropout_f32: null pointer argument");
  QPG_REQUIRE(n >= 0 && n <= ((int64_t)1 << 38), "qpg_gen_dropout_f32: need 0 <= n <= 2^38 (n %lld)", (long long)n);
  if (n == 0) return QPG_OK;
  hipLaunchKernelGGL(gent_dropout_kernel, dim3(blocks_of(n)), dim3(256), 0, qpg_stream(stream), x, mask, n, scale, y);
  QPG_LAUNCH_CHECK("gent_dropout_kernel");
  return QPG_OK;
}
