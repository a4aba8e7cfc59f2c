// Training of the Periodic Auto-Encoder (DeepPhase, codebook/PAE.py:50-162 Model, :273-476 the training loop): one
// step's forward (train or eval mode), its backward and the AdamW update of Library/AdamWR/adamw.py.
//
// Model(135, 8, 240, 13, 4.0) per window (channel-major, positions after the arrow):
//   x0 (135, 240) -> conv1 (240 taps, pad 120) -> z1 (15, 241) -> BN, tanh -> h1 -> conv2 (pad 119) -> z2 (8, 240)
//   -> BN, tanh -> latent h2;  rfft of each latent channel -> f, a, b;  fc[e] (240 -> 2) -> v -> BN (over the batch)
//   -> vn -> atan2' / tpi = p;  signal s = a sin(tpi (f args + p)) + b (8, 240) -> deconv1 (pad 119) -> z3 (15, 239)
//   -> BN, tanh -> h3 -> deconv2 (pad 120) -> y (135, 240);  loss = 300 mean((y - x0)^2).
//
// Every convolution, its data gradient and its weight gradient go through two kernels:
//   corr_kernel   out[r][o] = sum over (loop index n, q) of src_n[r + q - pad] * coef_n[q][o]
//                 forward:     r = position t, q = tap k, n = input channel, coef = weight[o][n][k]
//                 data grad:   the same with the weights transposed and flipped (weight[n][o][K-1-k], pad K-1-pad)
//   wgrad_kernel  the same inner loop with r = tap k, q = position t, n = window b and coef = dy[b][o][t]: the
//                 partial weight gradient of a slab of windows; wred_kernel adds the slabs in slab order.
// A thread owns 4 rows (r, r + 64, r + 128, r + 192) x 4 output channels; the source rows and coefficients of 4 loop
// indices are staged in LDS per pass.  Every statistic (BN, spectrum, fc, loss, bias gradients) is an f64 sum in a
// fixed order: no atomics anywhere, so two runs of the same step are bit-identical.  The tile geometry and the spectrum
// head (DFT, f / a / b, fc dot product, atan2') are qpg_pae_model.h's, shared with phase extraction.
#include "qpg_pae_model.h"

namespace {

using namespace pae;

constexpr int C = QPG_PAE_CHANNELS;   // 135
constexpr int M = QPG_PAE_MID;        // 15
constexpr int E = QPG_PAE_EMBED;      // 8
constexpr int T = QPG_PAE_TIME;       // 240 (also the number of taps)
constexpr int L1 = T + 1;             // conv1 output positions
constexpr int L3 = T - 1;             // deconv1 output positions
constexpr double BN_EPS = 1e-5;
constexpr double MOMENTUM = 0.1;

// The layers, each stated once (offsets into the parameter / gradient block and the running statistics).
// Conv: (B, Cin, Lin) -> (B, Cout, Lout), T taps behind `pad` zeros; w = weight (Cout, Cin, T), b = bias (Cout).
struct Conv {
  int w, b, Cin, Lin, Cout, Lout, pad;
};
constexpr Conv CONV1{QPG_PAET_OFF_CONV1_W, QPG_PAET_OFF_CONV1_B, C, T, M, L1, T / 2};
constexpr Conv CONV2{QPG_PAET_OFF_CONV2_W, QPG_PAET_OFF_CONV2_B, M, L1, E, T, (T - 1) / 2};
constexpr Conv DECONV1{QPG_PAET_OFF_DECONV1_W, QPG_PAET_OFF_DECONV1_B, E, T, M, L3, (T - 1) / 2};
constexpr Conv DECONV2{QPG_PAET_OFF_DECONV2_W, QPG_PAET_OFF_DECONV2_B, M, L3, C, T, T / 2};

constexpr int BN_SLOT = 32;           // doubles per BN layer in the workspace's st and bs: [Cch] | [Cch], Cch <= 16
// Bn: BatchNorm over (B, Cch, L); p = weight (Cch) | bias (Cch) (the fc BNs: per e, weight (2) | bias (2)), st =
// running_mean | running_var laid out like p, slot = its BN_SLOT of the workspace's st (mean | invstd) and bs
// (dbeta | dgamma).
struct Bn {
  int p, st, Cch, L, slot;
};
constexpr Bn BN1{QPG_PAET_OFF_BN1, QPG_PAET_ST_BN1, M, L1, 0};
constexpr Bn BN2{QPG_PAET_OFF_BN2, QPG_PAET_ST_BN2, E, T, 1};
constexpr Bn FCBN{QPG_PAET_OFF_FCBN, QPG_PAET_ST_FCBN, 2 * E, 1, 2};
constexpr Bn BN3{QPG_PAET_OFF_BN3, QPG_PAET_ST_BN3, M, L3, 3};

constexpr int NCH = 4;                // loop indices staged per pass = the k of one MFMA
constexpr int XS = 528;               // LDS source row stride: r + q < 512, + 16 so that the 4 rows of a fragment
                                      // (lanes h = 0..3) fall on disjoint banks
constexpr int QL = 256;               // LDS coefficient rows (q)
constexpr int CS = QL * 16 + 16;      // LDS coefficient block stride (floats), + 16 for the same reason

// One staged pass: acc[j][row r0 + r][col c] += sum over h < 4, q of xs[h][r0 + r + q] cs[h][q][c], as one
// v_mfma_f32_16x16x4_f32 per (tile, q): A[r][h] = xs[h][r0 + r + q] (lane r = lane & 15, h = lane >> 4),
// B[h][c] = cs[h][q][c] (c = lane & 15), shared by the wave's 4 tiles.  Exact f32 products, f32 accumulation.
__device__ __forceinline__ void corr_stage(const float* __restrict__ xs, const float* __restrict__ cs, int w, int lane,
                                           const TileRange& tr, f32x4 (&acc)[4]) {
  const int r = lane & 15, h = lane >> 4;
  const float* xa = xs + h * XS + r;
  const float* cb = cs + h * CS + r;
  for (int q = tr.beg; q <= tr.end; ++q) {
    const float b = cb[q * 16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q >= tr.lo[j] && q <= tr.hi[j]) acc[j] = mfma4(xa[16 * (w + 4 * j) + q], b, acc[j]);
  }
}

// out[b][o][t] = bias[o] + sum_n sum_k coef(o, n, k) src[b][n][t + k - pad], t < Lout.  flip = 0: coef = w[o][n][k]
// (w is (Cout, Cin, T)); flip = 1: coef = w[n][o][T-1-k] (w is (Cin, Cout, T): the data gradient of that conv).
// grid (B, ceil(Cout / 16)), 256 threads; rows = positions t, q = taps k, 4 input channels per pass.
__global__ __launch_bounds__(256) void corr_kernel(const float* __restrict__ src, int Cin, int Lin,
                                                   const float* __restrict__ w, int flip,
                                                   const float* __restrict__ bias, int Cout, int Lout, int pad,
                                                   float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xs[NCH * XS];
  __shared__ __attribute__((aligned(16))) float cs[NCH * CS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x, o0 = blockIdx.y * 16;
  const TileRange tr = tile_ranges(wv, Lout, T, pad, Lin);
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int n0 = 0; n0 < Cin; n0 += NCH) {
    __syncthreads();
    for (int e = tid; e < NCH * 512; e += 256) {
      const int nn = e >> 9, i = e & 511, n = n0 + nn, pos = i - pad;
      xs[nn * XS + i] = (n < Cin && pos >= 0 && pos < Lin) ? src[((int64_t)b * Cin + n) * Lin + pos] : 0.0f;
    }
    for (int e = tid; e < NCH * 16 * QL; e += 256) {
      const int nn = e / (16 * QL), rem = e - nn * 16 * QL, ol = rem / QL, k = rem - ol * QL;
      const int n = n0 + nn, o = o0 + ol;
      float v = 0.0f;
      if (n < Cin && o < Cout && k < T) v = flip ? w[((int64_t)n * Cout + o) * T + (T - 1 - k)] : w[((int64_t)o * Cin + n) * T + k];
      cs[nn * CS + k * 16 + ol] = v;
    }
    __syncthreads();
    corr_stage(xs, cs, wv, lane, tr, acc);
  }
  const int o = o0 + (lane & 15);
  if (o >= Cout) return;
  const float bo = bias ? bias[o] : 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int t = tile_row(wv, j, lane, g);
      if (t < Lout) out[((int64_t)b * Cout + o) * Lout + t] = f_add(acc[j][g], bo);
    }
  }
}

// Partial weight gradient of the conv src (B, Cin, Lin) -> dy (B, Cout, Lout), pad: windows of slab s are
// [s B / S, (s+1) B / S);  part[s][o][n][k] = sum_b sum_t dy[b][o][t] src[b][n][t + k - pad].
// grid (Cin, ceil(Cout / 16), S), 256 threads; rows = taps k, q = positions t, 4 windows per pass.
__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ src, int B, int Cin, int Lin,
                                                    const float* __restrict__ dy, int Cout, int Lout, int pad,
                                                    float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[NCH * XS];
  __shared__ __attribute__((aligned(16))) float cs[NCH * CS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x, o0 = blockIdx.y * 16, s = blockIdx.z, S = gridDim.z;
  const int b_lo = (int)((int64_t)s * B / S), b_hi = (int)((int64_t)(s + 1) * B / S);
  const TileRange tr = tile_ranges(wv, T, Lout, pad, Lin);
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b0 = b_lo; b0 < b_hi; b0 += NCH) {
    __syncthreads();
    for (int e = tid; e < NCH * 512; e += 256) {
      const int bb = e >> 9, i = e & 511, b = b0 + bb, pos = i - pad;
      xs[bb * XS + i] = (b < b_hi && pos >= 0 && pos < Lin) ? src[((int64_t)b * Cin + n) * Lin + pos] : 0.0f;
    }
    for (int e = tid; e < NCH * 16 * QL; e += 256) {
      const int bb = e / (16 * QL), rem = e - bb * 16 * QL, ol = rem / QL, t = rem - ol * QL;
      const int b = b0 + bb, o = o0 + ol;
      cs[bb * CS + t * 16 + ol] = (b < b_hi && o < Cout && t < Lout) ? dy[((int64_t)b * Cout + o) * Lout + t] : 0.0f;
    }
    __syncthreads();
    corr_stage(xs, cs, wv, lane, tr, acc);
  }
  const int o = o0 + (lane & 15);
  if (o >= Cout) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k = tile_row(wv, j, lane, g);
      if (k < T) part[(((int64_t)s * Cout + o) * Cin + n) * T + k] = acc[j][g];
    }
  }
}

// dw[e] = sum over slabs s (in order) of part[s][e], in f64, rounded once
__global__ __launch_bounds__(256) void wred_kernel(const float* __restrict__ part, int S, int64_t n, float* __restrict__ dw) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc = f_add(acc, (double)part[s * n + e]);
  dw[e] = (float)acc;
}

// fixed-order block reduction of two f64 values (256 threads)
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red) {
  const int tid = threadIdx.x;
  red[tid] = a;
  red[256 + tid] = b;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      red[tid] = f_add(red[tid], red[tid + h]);
      red[256 + tid] = f_add(red[256 + tid], red[256 + tid + h]);
    }
    __syncthreads();
  }
  a = red[0];
  b = red[256];
  __syncthreads();
}

// BatchNorm statistics of channel c of Cch from s = sum x, ss = sum x^2 over its N values: st[c] = mean,
// st[Cch + c] = 1 / sqrt(var + eps) (f64; what bn_xhat reads).  train: batch mean and clamped biased variance, running
// statistics updated (momentum 0.1, unbiased variance); eval: the running statistics (s, ss unused).
template <class Int>
__device__ __forceinline__ void bn_statistics(int train, double s, double ss, Int N, float* rmean, float* rvar,
                                              double* st, int Cch, int c) {
  if (train) {
    const double mean = s / (double)N;
    const double var = fmax(f_sub(ss / (double)N, f_mul(mean, mean)), 0.0);
    st[c] = mean;
    st[Cch + c] = 1.0 / sqrt(f_add(var, BN_EPS));
    *rmean = (float)f_add(f_mul(1.0 - MOMENTUM, (double)*rmean), f_mul(MOMENTUM, mean));
    *rvar = (float)f_add(f_mul(1.0 - MOMENTUM, (double)*rvar), f_mul(MOMENTUM, var * (double)N / (double)(N - 1)));
  } else {
    st[c] = (double)*rmean;
    st[Cch + c] = 1.0 / sqrt(f_add((double)*rvar, BN_EPS));
  }
}

// BatchNorm statistics of channel c of z (B, Cch, L), one block per channel (f64 sums)
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ z, int B, int Cch, int L, int train,
                                                       float* __restrict__ rmean, float* __restrict__ rvar,
                                                       double* __restrict__ st) {
  __shared__ double red[512];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int64_t N = (int64_t)B * L;
  if (!train) {
    if (tid == 0) bn_statistics(0, 0.0, 0.0, N, rmean + c, rvar + c, st, Cch, c);
    return;
  }
  double s = 0.0, ss = 0.0;
  for (int64_t e = tid; e < N; e += 256) {
    const int64_t b = e / L, t = e - b * L;
    const double v = (double)z[(b * Cch + c) * L + t];
    s = f_add(s, v);
    ss = f_add(ss, f_mul(v, v));
  }
  block_sum2(s, ss, red);
  if (tid == 0) bn_statistics(1, s, ss, N, rmean + c, rvar + c, st, Cch, c);
}

__device__ __forceinline__ float bn_xhat(float z, const double* st, int Cch, int c) {
  return (float)f_mul(f_sub((double)z, st[c]), st[Cch + c]);
}

// h = tanh(gamma xhat + beta) over (B, Cch, L)
__global__ __launch_bounds__(256) void bn_tanh_kernel(const float* __restrict__ z, int64_t n, int Cch, int L,
                                                      const double* __restrict__ st, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ h) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int c = (int)((e / L) % Cch);
  h[e] = tanhf(f_add(f_mul(bn_xhat(z[e], st, Cch, c), gamma[c]), beta[c]));
}

// training batch: x0[b][c][0] = 0, x0[b][c][s] = pn[st + s][c] - pn[st + s - 1][c]   (PAE.py:367-369)
// validation:     x0[b][c][s] = pn[st + s + 1][c] - pn[st + s][c] (s < 239), x0[b][c][239] = 0   (:260-262)
// f32 differences of the normalised f32 poses.  A start outside 0 .. n_frames - 240 gives a NaN window.
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ pn, int64_t n_frames,
                                                     const int64_t* __restrict__ starts, int B, int train,
                                                     float* __restrict__ x0) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)B * C * T) return;
  const int b = (int)(e / (C * T));
  const int rem = (int)(e - (int64_t)b * C * T), c = rem / T, s = rem - c * T;
  const int64_t st = starts[b];
  float v;
  if (st < 0 || st > n_frames - T) {
    v = __builtin_nanf("");
  } else if (train) {
    v = s == 0 ? 0.0f : f_sub(pn[(st + s) * C + c], pn[(st + s - 1) * C + c]);
  } else {
    v = s == T - 1 ? 0.0f : f_sub(pn[(st + s + 1) * C + c], pn[(st + s) * C + c]);
  }
  x0[e] = v;
}

// per window b: spectrum of each latent channel (f64, bins 0..120) -> spec[b][e][m] = (Re, Im);  f, a, b -> pfab;
// fc[e] -> v[b][2e + j] (f64 dot product + bias, rounded once)
__global__ __launch_bounds__(256) void spectrum_kernel(const float* __restrict__ h2, const float* __restrict__ P,
                                                       double* __restrict__ spec, float* __restrict__ pfab,
                                                       float* __restrict__ v) {
  __shared__ float lat[E * T];
  __shared__ double tw[2 * T];
  __shared__ double pw[E * NB];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int e = tid; e < E * T; e += 256) lat[e] = h2[(int64_t)b * E * T + e];
  fill_twiddles(tw, tid);
  __syncthreads();
  for (int task = tid; task < E * NB; task += 256) {
    const int e = task / NB, m = task - e * NB;
    double re, im;
    dft_bin(lat + e * T, tw, m, re, im);
    double* o = spec + (((int64_t)b * E + e) * NB + m) * 2;
    o[0] = re;
    o[1] = im;
    pw[task] = m == 0 ? re : bin_power(re, im);
  }
  if (tid < 2 * E) {
    const int e = tid >> 1, j = tid & 1;
    const float* fc = P + QPG_PAET_OFF_FC + e * (2 * T + 2);   // fc.e.weight (2, 240), fc.e.bias (2)
    v[b * 2 * E + tid] = (float)f_add(fc_dot(fc + j * T, lat + e * T), (double)fc[2 * T + j]);
  }
  __syncthreads();
  if (tid < E) {
    const int e = tid;
    double sp, sfp;
    power_sums(P + QPG_PAET_OFF_FREQS, [&](int m) { return pw[e * NB + m]; }, sp, sfp);
    float* o = pfab + b * 4 * E;
    spectrum_fab(sp, sfp, pw[e * NB], o[E + e], o[2 * E + e], o[3 * E + e]);
  }
}

// fc BatchNorms (one block): column q = 2 e + j of v (B, 16) normalised over the batch (train) or with the running
// statistics (eval), then p = atan2'(vn[2e+1], vn[2e]) / tpi.  st: [16] mean, [16] 1/sqrt(var + eps).
__global__ __launch_bounds__(256) void fcbn_kernel(const float* __restrict__ v, int B, int train,
                                                   const float* __restrict__ P, float* __restrict__ stats,
                                                   double* __restrict__ st, float* __restrict__ vn,
                                                   float* __restrict__ pfab) {
  const int tid = threadIdx.x;
  if (tid < 2 * E) {
    const int q = tid, e = q >> 1, j = q & 1;
    float* rm = stats + FCBN.st + 4 * e + j;                   // bn.e: running_mean (2) | running_var (2)
    double s = 0.0, ss = 0.0;
    if (train) {
      for (int b = 0; b < B; ++b) {
        const double x = (double)v[b * 2 * E + q];
        s = f_add(s, x);
        ss = f_add(ss, f_mul(x, x));
      }
    }
    bn_statistics(train, s, ss, B, rm, rm + 2, st, 2 * E, q);
  }
  __syncthreads();
  const float tpi = P[QPG_PAET_OFF_TPI];
  for (int e = tid; e < B * E; e += 256) {
    const int b = e / E, k = e - b * E;
    float xy[2];
    for (int j = 0; j < 2; ++j) {
      const int q = 2 * k + j;
      const float* g = P + FCBN.p + 4 * k;                     // bn.k: weight (2) | bias (2)
      xy[j] = f_add(f_mul(bn_xhat(v[b * 2 * E + q], st, 2 * E, q), g[j]), g[2 + j]);
      vn[b * 2 * E + q] = xy[j];
    }
    pfab[b * 4 * E + k] = phase_of(xy[0], xy[1], tpi);
  }
}

__device__ __forceinline__ float signal_theta(const float* pf, float tpi, float arg, int e) {
  return f_mul(tpi, f_add(f_mul(pf[E + e], arg), pf[e]));
}

// s[b][e][t] = a sin(tpi (f args[t] + p)) + b
__global__ __launch_bounds__(256) void signal_kernel(const float* __restrict__ pfab, const float* __restrict__ P, int B,
                                                     float* __restrict__ s) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * E * T) return;
  const int b = (int)(i / (E * T)), rem = (int)(i - (int64_t)b * E * T), e = rem / T, t = rem - e * T;
  const float* pf = pfab + b * 4 * E;
  const float th = signal_theta(pf, P[QPG_PAET_OFF_TPI], P[QPG_PAET_OFF_ARGS + t], e);
  s[i] = f_add(f_mul(pf[2 * E + e], sinf(th)), pf[3 * E + e]);
}

// squared error per block of 4096 entries (f64), dy = 600 (y - x0) / n
constexpr int LOSS_CHUNK = 4096;
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ y, const float* __restrict__ x0, int64_t n,
                                                   float gscale, float* __restrict__ dy, double* __restrict__ part) {
  __shared__ double red[512];
  const int64_t base = (int64_t)blockIdx.x * LOSS_CHUNK;
  double s = 0.0, unused = 0.0;
  for (int i = threadIdx.x; i < LOSS_CHUNK; i += 256) {
    const int64_t e = base + i;
    if (e >= n) break;
    const float d = f_sub(y[e], x0[e]);
    s = f_add(s, f_mul((double)d, (double)d));
    if (dy) dy[e] = f_mul(gscale, d);
  }
  block_sum2(s, unused, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// loss = 300 * sum(part) / n (one block)
__global__ __launch_bounds__(256) void loss_final_kernel(const double* __restrict__ part, int nparts, int64_t n,
                                                         double* __restrict__ loss) {
  __shared__ double red[512];
  double s = 0.0, unused = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) s = f_add(s, part[i]);
  block_sum2(s, unused, red);
  if (threadIdx.x == 0) *loss = f_mul(300.0, s / (double)n);
}

// ---- backward

// g[c] = sum_{b,t} a[b][c][t] (f64, rounded once); one block per channel
__global__ __launch_bounds__(256) void chan_sum_kernel(const float* __restrict__ a, int B, int Cch, int L,
                                                       float* __restrict__ g) {
  __shared__ double red[512];
  const int c = blockIdx.x;
  const int64_t N = (int64_t)B * L;
  double s = 0.0, unused = 0.0;
  for (int64_t e = threadIdx.x; e < N; e += 256) {
    const int64_t b = e / L, t = e - b * L;
    s = f_add(s, (double)a[(b * Cch + c) * L + t]);
  }
  block_sum2(s, unused, red);
  if (threadIdx.x == 0) g[c] = (float)s;
}

// tanh' and BatchNorm backward, reduction half: dA = dh (1 - h^2); dbeta = sum dA, dgamma = sum dA xhat (per channel,
// f64); bs[c] = dbeta, bs[Cch + c] = dgamma
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ z, const float* __restrict__ h,
                                                            const float* __restrict__ dh, int B, int Cch, int L,
                                                            const double* __restrict__ st, double* __restrict__ bs,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double red[512];
  const int c = blockIdx.x;
  const int64_t N = (int64_t)B * L;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t e = threadIdx.x; e < N; e += 256) {
    const int64_t b = e / L, t = e - b * L, i = (b * Cch + c) * L + t;
    const float hv = h[i];
    const double da = (double)f_mul(dh[i], f_sub(1.0f, f_mul(hv, hv)));
    s0 = f_add(s0, da);
    s1 = f_add(s1, f_mul(da, (double)bn_xhat(z[i], st, Cch, c)));
  }
  block_sum2(s0, s1, red);
  if (threadIdx.x == 0) {
    bs[c] = s0;
    bs[Cch + c] = s1;
    dbeta[c] = (float)s0;
    dgamma[c] = (float)s1;
  }
}

// train-mode BatchNorm backward of one value: dz = gamma invstd (dA - dbeta / N - xhat dgamma / N)
__device__ __forceinline__ float bn_bwd_term(double da, double xh, double dbeta, double dgamma, double N, double gamma,
                                             double invstd) {
  const double r = f_sub(f_sub(da, dbeta / N), f_mul(xh, dgamma / N));
  return (float)f_mul(f_mul(gamma, invstd), r);
}

// tanh' and BatchNorm backward, apply half: dz from dA = dh (1 - h^2) and the sums of the reduction half
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ z, const float* __restrict__ h,
                                                           const float* __restrict__ dh, int64_t n, int Cch, int L,
                                                           int64_t N, const double* __restrict__ st,
                                                           const double* __restrict__ bs,
                                                           const float* __restrict__ gamma, float* __restrict__ dz) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int c = (int)((e / L) % Cch);
  const float hv = h[e];
  const double da = (double)f_mul(dh[e], f_sub(1.0f, f_mul(hv, hv)));
  dz[e] = bn_bwd_term(da, (double)bn_xhat(z[e], st, Cch, c), bs[c], bs[Cch + c], (double)N, (double)gamma[c],
                      st[Cch + c]);
}

// signal backward and atan2' backward, one thread per (b, e): dfab[b][0..2][e] = df, da, db (f64 sums over t);
// dvn[b][2e + j] from dp = sum_t ds a cos(theta) tpi through p = atan(y / x) / tpi (+- 1/2)
__global__ __launch_bounds__(256) void signal_bwd_kernel(const float* __restrict__ ds, const float* __restrict__ pfab,
                                                         const float* __restrict__ vn, const float* __restrict__ P,
                                                         int B, double* __restrict__ dfab, float* __restrict__ dvn) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * E) return;
  const int b = i / E, e = i - b * E;
  const float* pf = pfab + b * 4 * E;
  const float tpi = P[QPG_PAET_OFF_TPI];
  const double a = (double)pf[2 * E + e];
  double da = 0.0, db = 0.0, dth_arg = 0.0, dth = 0.0;
  const float* g = ds + ((int64_t)b * E + e) * T;
  for (int t = 0; t < T; ++t) {
    const float arg = P[QPG_PAET_OFF_ARGS + t];
    const double th = (double)signal_theta(pf, tpi, arg, e);
    const double gt = (double)g[t];
    da = f_add(da, f_mul(gt, sin(th)));
    db = f_add(db, gt);
    const double d = f_mul(f_mul(gt, a), cos(th));
    dth = f_add(dth, d);
    dth_arg = f_add(dth_arg, f_mul(d, (double)arg));
  }
  double* o = dfab + (int64_t)b * 3 * E;
  o[e] = f_mul(dth_arg, (double)tpi);
  o[E + e] = da;
  o[2 * E + e] = db;
  const double dp = f_mul(dth, (double)tpi);
  const double x = (double)vn[b * 2 * E + 2 * e], y = (double)vn[b * 2 * E + 2 * e + 1];
  const double r2 = f_add(f_mul(x, x), f_mul(y, y));
  const double dang = dp / (double)tpi;
  dvn[b * 2 * E + 2 * e] = (float)(-dang * y / r2);
  dvn[b * 2 * E + 2 * e + 1] = (float)(dang * x / r2);
}

// fc BatchNorm backward (train mode, over the batch) and the fc bias gradient; one block.  dv (B, 16).
__global__ __launch_bounds__(256) void fcbn_bwd_kernel(const float* __restrict__ v, const float* __restrict__ dvn,
                                                       int B, const double* __restrict__ st,
                                                       const float* __restrict__ P, float* __restrict__ G,
                                                       float* __restrict__ dv) {
  __shared__ double sums[4 * E * 2];
  const int tid = threadIdx.x;
  if (tid < 2 * E) {
    const int q = tid, e = q >> 1, j = q & 1;
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < B; ++b) {
      const double g = (double)dvn[b * 2 * E + q];
      s0 = f_add(s0, g);
      s1 = f_add(s1, f_mul(g, (double)bn_xhat(v[b * 2 * E + q], st, 2 * E, q)));
    }
    sums[q] = s0;
    sums[2 * E + q] = s1;
    G[FCBN.p + 4 * e + j] = (float)s1;                         // bn.e.weight
    G[FCBN.p + 4 * e + 2 + j] = (float)s0;                     // bn.e.bias
  }
  __syncthreads();
  for (int i = tid; i < B * 2 * E; i += 256) {
    const int q = i % (2 * E), k = q >> 1, j = q & 1;
    dv[i] = bn_bwd_term((double)dvn[i], (double)bn_xhat(v[i], st, 2 * E, q), sums[q], sums[2 * E + q], (double)B,
                        (double)P[FCBN.p + 4 * k + j], st[2 * E + q]);
  }
  __syncthreads();
  if (tid < 2 * E) {
    const int q = tid, e = q >> 1, j = q & 1;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s = f_add(s, (double)dv[b * 2 * E + q]);
    G[QPG_PAET_OFF_FC + e * (2 * T + 2) + 2 * T + j] = (float)s;
  }
}

// fc weight gradient: dW[e][j][u] = sum_b dv[b][2e + j] h2[b][e][u] (f64 in window order)
__global__ __launch_bounds__(256) void fc_wgrad_kernel(const float* __restrict__ dv, const float* __restrict__ h2, int B,
                                                       float* __restrict__ G) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * E * T) return;
  const int e = i / (2 * T), rem = i - e * 2 * T, j = rem / T, u = rem - j * T;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s = f_add(s, f_mul((double)dv[b * 2 * E + 2 * e + j], (double)h2[((int64_t)b * E + e) * T + u]));
  G[QPG_PAET_OFF_FC + e * (2 * T + 2) + j * T + u] = (float)s;
}

// latent gradient: through fc (sum_j dv W), the offset (db / 240) and the spectrum: with Pw = sum_m |X_m|^2 (m >= 1),
// F = sum_m freqs[m-1] |X_m|^2:  dL/d|X_m|^2 = df (freqs[m-1] - F / Pw) / (Pw ts) + da / (240 sqrt(Pw)) = g_m, and
// d|X_m|^2 / dh[u] = 2 (Re X_m cos(2 pi m u / 240) - Im X_m sin(2 pi m u / 240)).  One block per window.
__global__ __launch_bounds__(256) void latent_bwd_kernel(const double* __restrict__ spec, const double* __restrict__ dfab,
                                                         const float* __restrict__ dv, const float* __restrict__ P,
                                                         float* __restrict__ dh2) {
  __shared__ double tw[2 * T];
  __shared__ double gm[E * NB];
  __shared__ double rei[E * NB * 2];
  const int b = blockIdx.x, tid = threadIdx.x;
  fill_twiddles(tw, tid);
  for (int i = tid; i < E * NB * 2; i += 256) rei[i] = spec[(int64_t)b * E * NB * 2 + i];
  __syncthreads();
  if (tid < E) {
    const int e = tid;
    const float* fr = P + QPG_PAET_OFF_FREQS;
    double sp, sfp;
    power_sums(fr, [&](int m) { return bin_power(rei[(e * NB + m) * 2], rei[(e * NB + m) * 2 + 1]); }, sp, sfp);
    const double* d = dfab + (int64_t)b * 3 * E;
    const double df = d[e], da = d[E + e];
    const double fbar = sfp / sp;
    gm[e * NB] = 0.0;
    for (int m = 1; m < NB; ++m)
      gm[e * NB + m] = f_add(df * f_sub((double)fr[m - 1], fbar) / (sp * TIME_SCALE), da / ((double)T * sqrt(sp)));
  }
  __syncthreads();
  for (int i = tid; i < E * T; i += 256) {
    const int e = i / T, u = i - e * T;
    const double* d = dfab + (int64_t)b * 3 * E;
    double s = d[2 * E + e] / (double)T;
    const float* wf = P + QPG_PAET_OFF_FC + e * (2 * T + 2);
    s = f_add(s, f_mul((double)dv[b * 2 * E + 2 * e], (double)wf[u]));
    s = f_add(s, f_mul((double)dv[b * 2 * E + 2 * e + 1], (double)wf[T + u]));
    int idx = u;
    double acc = 0.0;
    for (int m = 1; m < NB; ++m) {
      const double re = rei[(e * NB + m) * 2], im = rei[(e * NB + m) * 2 + 1];
      acc = f_add(acc, f_mul(gm[e * NB + m], f_sub(f_mul(re, tw[2 * idx]), f_mul(im, tw[2 * idx + 1]))));
      idx += u;
      if (idx >= T) idx -= T;
    }
    dh2[(int64_t)b * E * T + i] = (float)f_add(s, f_mul(2.0, acc));
  }
}

// AdamW of Library/AdamWR/adamw.py, f32 like the reference's tensors:  p *= (1 - wd);  m = b1 m + (1 - b1) g;
// v = b2 v + (1 - b2) g g;  p += (-step_size m) / (sqrt(v) + eps)
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                    float keep, float b1, float omb1, float b2, float omb2,
                                                    float eps, float neg_step) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  const float mi = f_add(f_mul(m[i], b1), f_mul(omb1, gi));
  const float vi = f_add(f_mul(v[i], b2), f_mul(f_mul(omb2, gi), gi));
  m[i] = mi;
  v[i] = vi;
  const float pi = f_mul(p[i], keep);
  p[i] = f_add(pi, f_div(f_mul(neg_step, mi), f_add(f_sqrt(vi), eps)));
}

// ---- workspace layout (floats; every region starts at a multiple of 4 floats)
struct Ws {
  float *x0, *z1, *h1, *z2, *h2, *v, *vn, *pfab, *sig, *z3, *h3, *y, *dy, *dh3, *dz3, *ds, *dh2, *dz2, *dh1, *dz1,
      *dv, *dvn, *part;
  double *spec, *st, *bs, *dfab, *lpart, *loss;
  int64_t floats;
};

inline int64_t r4(int64_t n) { return (n + 3) & ~(int64_t)3; }
inline int n_slabs(int B) { return B < QPG_PAET_SLABS ? B : QPG_PAET_SLABS; }
inline int64_t loss_parts(int B) { return ((int64_t)B * C * T + LOSS_CHUNK - 1) / LOSS_CHUNK; }

Ws ws_layout(float* base, int B) {
  Ws w;
  int64_t o = 0;
  auto f = [&](int64_t n) { float* p = base ? base + o : nullptr; o += r4(n); return p; };
  auto d = [&](int64_t n) { double* p = base ? reinterpret_cast<double*>(base + o) : nullptr; o += r4(2 * n); return p; };
  const int64_t b = B;
  w.x0 = f(b * C * T);  w.z1 = f(b * M * L1);  w.h1 = f(b * M * L1);  w.z2 = f(b * E * T);  w.h2 = f(b * E * T);
  w.v = f(b * 2 * E);   w.vn = f(b * 2 * E);   w.pfab = f(b * 4 * E);  w.sig = f(b * E * T);
  w.z3 = f(b * M * L3); w.h3 = f(b * M * L3);  w.y = f(b * C * T);     w.dy = f(b * C * T);
  w.dh3 = f(b * M * L3); w.dz3 = f(b * M * L3); w.ds = f(b * E * T);   w.dh2 = f(b * E * T); w.dz2 = f(b * E * T);
  w.dh1 = f(b * M * L1); w.dz1 = f(b * M * L1); w.dv = f(b * 2 * E);   w.dvn = f(b * 2 * E);
  w.part = f((int64_t)n_slabs(B) * C * M * T);
  w.spec = d(b * E * NB * 2);
  w.st = d(4 * BN_SLOT);                     // per BN layer (Bn::slot): mean | invstd
  w.bs = d(4 * BN_SLOT);                     // backward sums per BN layer
  w.dfab = d(b * 3 * E);
  w.lpart = d(loss_parts(B));
  w.loss = d(1);
  w.floats = o;
  return w;
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }

// dgrad = 0: out = the convolution of src, + bias.  dgrad = 1: its data gradient, src = dL/d(output) -> out =
// dL/d(input): the same correlation with the weights transposed and flipped behind T - 1 - pad zeros, no bias.
int conv(hipStream_t s, const Conv& cv, int dgrad, const float* P, const float* src, int B, float* out) {
  const Conv c = dgrad ? Conv{cv.w, cv.b, cv.Cout, cv.Lout, cv.Cin, cv.Lin, T - 1 - cv.pad} : cv;
  hipLaunchKernelGGL(corr_kernel, dim3(B, (c.Cout + 15) / 16), dim3(256), 0, s, src, c.Cin, c.Lin, P + c.w, dgrad,
                     dgrad ? nullptr : P + c.b, c.Cout, c.Lout, c.pad, out);
  QPG_LAUNCH_CHECK("corr_kernel");
  return QPG_OK;
}

// weight and bias gradients of the convolution src -> dy into G
int wgrad(hipStream_t s, const Conv& cv, const float* src, const float* dy, int B, float* part, float* G) {
  const int S = n_slabs(B);
  hipLaunchKernelGGL(wgrad_kernel, dim3(cv.Cin, (cv.Cout + 15) / 16, S), dim3(256), 0, s, src, B, cv.Cin, cv.Lin, dy,
                     cv.Cout, cv.Lout, cv.pad, part);
  QPG_LAUNCH_CHECK("wgrad_kernel");
  const int64_t n = (int64_t)cv.Cout * cv.Cin * T;
  hipLaunchKernelGGL(wred_kernel, dim3(nblk(n)), dim3(256), 0, s, part, S, n, G + cv.w);
  QPG_LAUNCH_CHECK("wred_kernel");
  hipLaunchKernelGGL(chan_sum_kernel, dim3(cv.Cout), dim3(256), 0, s, dy, B, cv.Cout, cv.Lout, G + cv.b);
  QPG_LAUNCH_CHECK("chan_sum_kernel");
  return QPG_OK;
}

// h = tanh(BN(z)); S: the running statistics
int bn_fwd(hipStream_t s, const Bn& bn, const Ws& w, const float* P, float* S, const float* z, int B, int train,
           float* h) {
  double* st = w.st + BN_SLOT * bn.slot;
  hipLaunchKernelGGL(bn_stats_kernel, dim3(bn.Cch), dim3(256), 0, s, z, B, bn.Cch, bn.L, train, S + bn.st,
                     S + bn.st + bn.Cch, st);
  QPG_LAUNCH_CHECK("bn_stats_kernel");
  const int64_t n = (int64_t)B * bn.Cch * bn.L;
  hipLaunchKernelGGL(bn_tanh_kernel, dim3(nblk(n)), dim3(256), 0, s, z, n, bn.Cch, bn.L, st, P + bn.p,
                     P + bn.p + bn.Cch, h);
  QPG_LAUNCH_CHECK("bn_tanh_kernel");
  return QPG_OK;
}

// dz from dh through tanh and the train-mode BN; the BN's weight and bias gradients into G
int bn_bwd(hipStream_t s, const Bn& bn, const Ws& w, const float* P, float* G, const float* z, const float* h,
           const float* dh, int B, float* dz) {
  const double* st = w.st + BN_SLOT * bn.slot;
  double* bs = w.bs + BN_SLOT * bn.slot;
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(bn.Cch), dim3(256), 0, s, z, h, dh, B, bn.Cch, bn.L, st, bs, G + bn.p,
                     G + bn.p + bn.Cch);
  QPG_LAUNCH_CHECK("bn_bwd_reduce_kernel");
  const int64_t n = (int64_t)B * bn.Cch * bn.L;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(nblk(n)), dim3(256), 0, s, z, h, dh, n, bn.Cch, bn.L,
                     (int64_t)B * bn.L, st, bs, P + bn.p, dz);
  QPG_LAUNCH_CHECK("bn_bwd_apply_kernel");
  return QPG_OK;
}

#define QPG_TRY(x)              \
  do {                          \
    const int rc_ = (x);        \
    if (rc_ != QPG_OK) return rc_; \
  } while (0)

}  // namespace

extern "C" int qpg_pae_train_ws_floats(qpg_ctx* ctx, void* stream, int batch, int64_t* floats) {
  (void)stream;
  QPG_REQUIRE(ctx && floats, "qpg_pae_train_ws_floats: null pointer argument");
  QPG_REQUIRE(batch >= 2 && batch <= QPG_PAET_MAX_BATCH, "qpg_pae_train_ws_floats: batch %d outside 2..%d", batch,
              QPG_PAET_MAX_BATCH);
  *floats = ws_layout(nullptr, batch).floats;
  return QPG_OK;
}

extern "C" int qpg_pae_train_forward_f32(qpg_ctx* ctx, void* stream, const float* params, float* stats,
                                         const float* poses, int64_t n_frames, const int64_t* starts, int batch,
                                         int train, float* ws, int64_t ws_floats, double* loss) {
  QPG_REQUIRE(ctx, "qpg_pae_train_forward_f32: null context");
  QPG_REQUIRE(params && stats && poses && starts && ws, "qpg_pae_train_forward_f32: null pointer argument");
  QPG_REQUIRE(batch >= 2 && batch <= QPG_PAET_MAX_BATCH,
              "qpg_pae_train_forward_f32: batch %d outside 2..%d (BatchNorm over the batch needs two windows)", batch,
              QPG_PAET_MAX_BATCH);
  QPG_REQUIRE(n_frames >= T && n_frames <= ((int64_t)1 << 40),
              "qpg_pae_train_forward_f32: %lld pose frames, need 240 .. 2^40", (long long)n_frames);
  const Ws w = ws_layout(ws, batch);
  QPG_REQUIRE(ws_floats >= w.floats, "qpg_pae_train_forward_f32: workspace of %lld floats, %lld needed",
              (long long)ws_floats, (long long)w.floats);
  QPG_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "qpg_pae_train_forward_f32: workspace not 16-byte aligned");
  hipStream_t s = qpg_stream(stream);
  const int B = batch, tr = train ? 1 : 0;
  const float* P = params;
  float* S = stats;
  hipLaunchKernelGGL(gather_kernel, dim3(nblk((int64_t)B * C * T)), dim3(256), 0, s, poses, n_frames, starts, B, tr,
                     w.x0);
  QPG_LAUNCH_CHECK("gather_kernel");
  QPG_TRY(conv(s, CONV1, 0, P, w.x0, B, w.z1));
  QPG_TRY(bn_fwd(s, BN1, w, P, S, w.z1, B, tr, w.h1));
  QPG_TRY(conv(s, CONV2, 0, P, w.h1, B, w.z2));
  QPG_TRY(bn_fwd(s, BN2, w, P, S, w.z2, B, tr, w.h2));
  hipLaunchKernelGGL(spectrum_kernel, dim3(B), dim3(256), 0, s, w.h2, P, w.spec, w.pfab, w.v);
  QPG_LAUNCH_CHECK("spectrum_kernel");
  hipLaunchKernelGGL(fcbn_kernel, dim3(1), dim3(256), 0, s, w.v, B, tr, P, S, w.st + BN_SLOT * FCBN.slot, w.vn, w.pfab);
  QPG_LAUNCH_CHECK("fcbn_kernel");
  hipLaunchKernelGGL(signal_kernel, dim3(nblk((int64_t)B * E * T)), dim3(256), 0, s, w.pfab, P, B, w.sig);
  QPG_LAUNCH_CHECK("signal_kernel");
  QPG_TRY(conv(s, DECONV1, 0, P, w.sig, B, w.z3));
  QPG_TRY(bn_fwd(s, BN3, w, P, S, w.z3, B, tr, w.h3));
  QPG_TRY(conv(s, DECONV2, 0, P, w.h3, B, w.y));
  const int64_t n = (int64_t)B * C * T;
  const float gscale = (float)(600.0 / (double)n);
  hipLaunchKernelGGL(loss_kernel, dim3((unsigned)loss_parts(B)), dim3(256), 0, s, w.y, w.x0, n, gscale,
                     tr ? w.dy : nullptr, w.lpart);
  QPG_LAUNCH_CHECK("loss_kernel");
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, w.lpart, (int)loss_parts(B), n,
                     loss ? loss : w.loss);
  QPG_LAUNCH_CHECK("loss_final_kernel");
  return QPG_OK;
}

extern "C" int qpg_pae_train_backward_f32(qpg_ctx* ctx, void* stream, const float* params, int batch, float* ws,
                                          int64_t ws_floats, float* grads) {
  QPG_REQUIRE(ctx, "qpg_pae_train_backward_f32: null context");
  QPG_REQUIRE(params && ws && grads, "qpg_pae_train_backward_f32: null pointer argument");
  QPG_REQUIRE(batch >= 2 && batch <= QPG_PAET_MAX_BATCH, "qpg_pae_train_backward_f32: batch %d outside 2..%d", batch,
              QPG_PAET_MAX_BATCH);
  const Ws w = ws_layout(ws, batch);
  QPG_REQUIRE(ws_floats >= w.floats, "qpg_pae_train_backward_f32: workspace of %lld floats, %lld needed",
              (long long)ws_floats, (long long)w.floats);
  QPG_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "qpg_pae_train_backward_f32: workspace not 16-byte aligned");
  hipStream_t s = qpg_stream(stream);
  const int B = batch;
  const float* P = params;
  float* G = grads;
  // deconv2 -> dh3 -> BN3 -> dz3
  QPG_TRY(wgrad(s, DECONV2, w.h3, w.dy, B, w.part, G));
  QPG_TRY(conv(s, DECONV2, 1, P, w.dy, B, w.dh3));
  QPG_TRY(bn_bwd(s, BN3, w, P, G, w.z3, w.h3, w.dh3, B, w.dz3));
  // deconv1 -> ds
  QPG_TRY(wgrad(s, DECONV1, w.sig, w.dz3, B, w.part, G));
  QPG_TRY(conv(s, DECONV1, 1, P, w.dz3, B, w.ds));
  // signal, atan2', fc BN, fc, spectrum -> dh2
  hipLaunchKernelGGL(signal_bwd_kernel, dim3(nblk((int64_t)B * E)), dim3(256), 0, s, w.ds, w.pfab, w.vn, P, B, w.dfab,
                     w.dvn);
  QPG_LAUNCH_CHECK("signal_bwd_kernel");
  hipLaunchKernelGGL(fcbn_bwd_kernel, dim3(1), dim3(256), 0, s, w.v, w.dvn, B, w.st + BN_SLOT * FCBN.slot, P, G, w.dv);
  QPG_LAUNCH_CHECK("fcbn_bwd_kernel");
  hipLaunchKernelGGL(fc_wgrad_kernel, dim3(nblk(2 * E * T)), dim3(256), 0, s, w.dv, w.h2, B, G);
  QPG_LAUNCH_CHECK("fc_wgrad_kernel");
  hipLaunchKernelGGL(latent_bwd_kernel, dim3(B), dim3(256), 0, s, w.spec, w.dfab, w.dv, P, w.dh2);
  QPG_LAUNCH_CHECK("latent_bwd_kernel");
  // BN2 -> conv2 -> dh1 -> BN1 -> conv1
  QPG_TRY(bn_bwd(s, BN2, w, P, G, w.z2, w.h2, w.dh2, B, w.dz2));
  QPG_TRY(wgrad(s, CONV2, w.h1, w.dz2, B, w.part, G));
  QPG_TRY(conv(s, CONV2, 1, P, w.dz2, B, w.dh1));
  QPG_TRY(bn_bwd(s, BN1, w, P, G, w.z1, w.h1, w.dh1, B, w.dz1));
  QPG_TRY(wgrad(s, CONV1, w.x0, w.dz1, B, w.part, G));
  return QPG_OK;
}

extern "C" int qpg_pae_adamw_f32(qpg_ctx* ctx, void* stream, float* p, const float* g, float* m, float* v, int64_t n,
                                 double lr, double weight_decay, double beta1, double beta2, double eps,
                                 int64_t step) {
  QPG_REQUIRE(ctx, "qpg_pae_adamw_f32: null context");
  QPG_REQUIRE(p && g && m && v, "qpg_pae_adamw_f32: null pointer argument");
  QPG_REQUIRE(n >= 0 && step >= 1, "qpg_pae_adamw_f32: need n >= 0 and step >= 1 (n %lld, step %lld)", (long long)n,
              (long long)step);
  if (n == 0) return QPG_OK;
  // the scalars are formed in f64 and rounded to f32 once, as torch does with the Python floats of adamw.py
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  const double step_size = lr * sqrt(bc2) / bc1;
  hipLaunchKernelGGL(adamw_kernel, dim3(nblk(n)), dim3(256), 0, qpg_stream(stream), p, g, m, v, n,
                     (float)(1.0 - weight_decay), (float)beta1, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps, (float)(-step_size));
  QPG_LAUNCH_CHECK("adamw_kernel");
  return QPG_OK;
}
