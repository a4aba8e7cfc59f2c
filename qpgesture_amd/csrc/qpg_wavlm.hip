// WavLM feature extraction (inference): the kernels behind qpgesture_amd/wavlm.py.  Everything is f32; every matrix
// product runs on the f32 matrix cores (v_mfma_f32_32x32x2_f32: a k-ordered f32 FMA chain per output, no reduced
// precision), so a result does not depend on the batch it is computed in.
//
// Activations are channels-last rows [B][T][C].  That makes every convolution of the model a plain GEMM:
//   * feature-extractor layer i >= 1 (C -> C, k taps, stride s): output frame t reads the k*C CONTIGUOUS floats that
//     start at input frame s*t, so A is the input with a row stride of s*C and K = k*C; the weights are repacked once
//     to [Cout][k][Cin];
//   * pos_conv (grouped, k = 128, padding 64, last frame dropped): wavlm_pos_pad_kernel copies x to a zero-padded
//     group-major image [B][G][T + k - 1][Cg]; output frame t of group g reads the k*Cg contiguous floats that start
//     at its row t (row stride Cg), weights repacked to [G][Cg out][k][Cg in];
//   * the Linear layers are GEMMs as they stand.
// wavlm_gemm_kernel is the one GEMM: out = A W^T (+ bias) (GELU) (+ residual), batched over (outer, inner) with strides;
// an output is the k-ordered sum of its 512-product FMA chains.
//
// wavlm_conv0_kernel   layer 0 of the feature extractor (1 -> C channels, k = 10, s = 5) straight from the samples;
// wavlm_ln_kernel      LayerNorm over a row (two passes: mean, then the variance of the centred values), optional GELU;
// wavlm_gate_kernel    the gated relative-position factor gate_a (gate_b grep_a[h] - 1) + 2 per (row, head);
// wavlm_attn_kernel    one block per (batch, head, 16 queries): scores q k^T + gate * bias[k - q] from the [2T-1][H] table,
//                      max-subtracted softmax in LDS, times V.  No (B H, T, T) array exists in memory.
// wavlm_mask_rows_kernel   zeroes the rows a byte mask names (the padded frames of a ragged batch, ahead of pos_conv);
// wavlm_attn_tiled_kernel  the same attention for any T and with a key mask: one block per (batch, head, 128 queries)
//                      walks the keys in tiles of 64, K Q^T and V^T P^T on the f32 matrix cores, online softmax; LDS and
//                      registers do not grow with T.
#include "qpg_common.h"

namespace {

constexpr int HD = QPG_WAVLM_HEAD_DIM;       // 64
constexpr int TMAX = QPG_WAVLM_MAX_FRAMES;   // 256
constexpr int QT = 16;                       // queries per attention block

__device__ __forceinline__ float gelu_erf(float x) {
  return f_mul(f_mul(x, 0.5f), f_add(1.0f, erff(f_mul(x, 0.70710678118654752440f))));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = f_add(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- layer 0: out[b][t][c] = bias[c] + sum_j w[c][j] wav[b][s t + j]
constexpr int C0T = 8;                       // frames per thread
__global__ __launch_bounds__(256) void wavlm_conv0_kernel(const float* __restrict__ wav, int64_t n, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int C, int k, int s, int64_t T,
                                                          int64_t total, float* __restrict__ out) {
  // a thread owns channel c of C0T consecutive frames: a tap's weight is loaded once for all of them, and the samples a
  // wave reads are the same for its 64 channels
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const int64_t bt = e / C;
  const int64_t ntg = (T + C0T - 1) / C0T;
  const int64_t b = bt / ntg, t0 = (bt - b * ntg) * C0T;
  const int nt = (int)min((int64_t)C0T, T - t0);
  const float* x = wav + b * n + t0 * s;
  const float* wc = w + (int64_t)c * k;
  float acc[C0T];
#pragma unroll
  for (int i = 0; i < C0T; ++i) acc[i] = 0.0f;
  for (int j = 0; j < k; ++j) {
    const float wj = wc[j];
#pragma unroll
    for (int i = 0; i < C0T; ++i)
      if (i < nt) acc[i] = fmaf(wj, x[i * s + j], acc[i]);
  }
  const float bv = bias ? bias[c] : 0.0f;
  float* o = out + (b * T + t0) * C + c;
#pragma unroll
  for (int i = 0; i < C0T; ++i)
    if (i < nt) o[(int64_t)i * C] = bias ? f_add(acc[i], bv) : acc[i];
}

// ---- LayerNorm over rows of C, one wave per row
// (x and y carry no __restrict__: y may be x, each lane then reads and writes its own elements)
__global__ __launch_bounds__(256) void wavlm_ln_kernel(const float* x, const float* __restrict__ g,
                                                       const float* __restrict__ b, int64_t M, int C, float eps, int gelu,
                                                       float* y) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + row * C;
  float s = 0.0f;
  for (int c = lane; c < C; c += 64) s = f_add(s, xr[c]);
  const float mean = f_div(wave_sum(s), (float)C);
  float v = 0.0f;
  for (int c = lane; c < C; c += 64) {
    const float d = f_sub(xr[c], mean);
    v = fmaf(d, d, v);
  }
  const float rstd = f_div(1.0f, f_sqrt(f_add(f_div(wave_sum(v), (float)C), eps)));
  float* yr = y + row * C;
  for (int c = lane; c < C; c += 64) {
    float o = f_add(f_mul(f_mul(f_sub(xr[c], mean), rstd), g[c]), b[c]);
    if (gelu) o = gelu_erf(o);
    yr[c] = o;
  }
}

// ---- the GEMM: C[m][n] = epilogue(sum_k A[m][k] W[n][k])
// block tile 128 x 128: 2 x 2 waves of 2 x NT tiles of 32 x 32.  (NT = 1, a 128 x 64 tile, for pos_conv's 64 channels
// per group keeps all four waves busy and was measured at half the speed: 4.4 ms against 2.2 ms for 32 windows.)
constexpr int BM = 128, BK = 16, LDT = BM + 4, NT = 2, BN = 64 * NT;
constexpr int KCHUNK = 512;      // k per FMA chain; the chunks' sums are added in k order

struct GemmArgs {
  const float* A;
  const float* W;
  const float* bias;
  const float* R;
  float* C;
  int M, N, K, n_inner, gelu;
  int64_t lda, ldc, sA0, sA1, sW1, sB1, sC0, sC1;
};

__global__ __launch_bounds__(256) void wavlm_gemm_kernel(const GemmArgs p) {
  __shared__ __attribute__((aligned(16))) float As[2][BK][LDT];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN + 4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int z0 = blockIdx.z / p.n_inner, z1 = blockIdx.z - z0 * p.n_inner;
  const float* A = p.A + z0 * p.sA0 + z1 * p.sA1;
  const float* W = p.W + z1 * p.sW1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int wm = w >> 1, wn = w & 1;

  // loads: thread (kq, r) takes 4 consecutive k of rows r, r + 64 of A's tile and of the NT 64-row parts of W's; rows past the end are clamped to
  // the last valid row (their results are never stored)
  const int kq = tid & 3, r = tid >> 2;
  const float* ap[2];
  const float* bp[NT];
#pragma unroll
  for (int i = 0; i < 2; ++i) ap[i] = A + (int64_t)min(m0 + r + 64 * i, p.M - 1) * p.lda + kq * 4;
#pragma unroll
  for (int i = 0; i < NT; ++i) bp[i] = W + (int64_t)min(n0 + r + 64 * i, p.N - 1) * p.K + kq * 4;
  bool live[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      live[mt][nt] = (m0 + wm * 64 + mt * 32 < p.M) && (n0 + wn * 32 * NT + nt * 32 < p.N);

  // acc: the FMA chain of the current KCHUNK of k; tot: the sum of the finished chunks (blocked summation: a chain of
  // 8 192 products, pos_conv at width 1024, otherwise carries 8 192 roundings against the running sum)
  f32x16 acc[2][NT], tot[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[mt][nt][q] = tot[mt][nt][q] = 0.0f;

  f32x4 ra[2], rb[NT];
#pragma unroll
  for (int i = 0; i < 2; ++i) ra[i] = *reinterpret_cast<const f32x4*>(ap[i]);
#pragma unroll
  for (int i = 0; i < NT; ++i) rb[i] = *reinterpret_cast<const f32x4*>(bp[i]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int i = 0; i < 2; ++i) As[0][kq * 4 + j][r + 64 * i] = ra[i][j];
#pragma unroll
    for (int i = 0; i < NT; ++i) Bs[0][kq * 4 + j][r + 64 * i] = rb[i][j];
  }
  __syncthreads();

  const int nk = p.K / BK;
  const int lr = lane & 31, lk = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) {
#pragma unroll
      for (int i = 0; i < 2; ++i) ra[i] = *reinterpret_cast<const f32x4*>(ap[i] + (int64_t)(kt + 1) * BK);
#pragma unroll
      for (int i = 0; i < NT; ++i) rb[i] = *reinterpret_cast<const f32x4*>(bp[i] + (int64_t)(kt + 1) * BK);
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float a[2], b[NT];
#pragma unroll
      for (int t = 0; t < 2; ++t) a[t] = As[cur][kk + lk][wm * 64 + t * 32 + lr];
#pragma unroll
      for (int t = 0; t < NT; ++t) b[t] = Bs[cur][kk + lk][wn * 32 * NT + t * 32 + lr];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          if (live[mt][nt]) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
    if (!more || (kt + 1) % (KCHUNK / BK) == 0) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            tot[mt][nt][q] = f_add(tot[mt][nt][q], acc[mt][nt][q]);
            acc[mt][nt][q] = 0.0f;
          }
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) As[cur ^ 1][kq * 4 + j][r + 64 * i] = ra[i][j];
#pragma unroll
        for (int i = 0; i < NT; ++i) Bs[cur ^ 1][kq * 4 + j][r + 64 * i] = rb[i][j];
      }
    }
    __syncthreads();
  }

  // C/D layout of v_mfma_f32_32x32x2_f32: lane l, register q holds row (q & 3) + 8 (q >> 2) + 4 (l >> 5), column l & 31
  const int64_t zoff = z0 * p.sC0 + z1 * p.sC1;
  float* C = p.C + zoff;
  const float* R = p.R ? p.R + zoff : nullptr;
  const float* bias = p.bias ? p.bias + z1 * p.sB1 : nullptr;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = n0 + wn * 32 * NT + nt * 32 + lr;
      if (!live[mt][nt] || col >= p.N) continue;
      const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = m0 + wm * 64 + mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * lk;
        if (row >= p.M) continue;
        float v = f_add(tot[mt][nt][q], bv);
        if (p.gelu) v = gelu_erf(v);
        const int64_t o = (int64_t)row * p.ldc + col;
        if (R) v = f_add(v, R[o]);
        C[o] = v;
      }
    }
}

// ---- pos_conv's padded group-major image: P[b][g][r][c] = x[b][r - pad][g Cg + c], zero outside 0 <= r - pad < T
__global__ __launch_bounds__(256) void wavlm_pos_pad_kernel(const float* __restrict__ x, int T, int D, int G, int rows,
                                                            int pad, int64_t total, float* __restrict__ P) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int Cg = D / G;
  const int c = (int)(e % Cg);
  int64_t q = e / Cg;
  const int r = (int)(q % rows);
  q /= rows;
  const int g = (int)(q % G);
  const int64_t b = q / G;
  const int t = r - pad;
  P[e] = (t >= 0 && t < T) ? x[(b * T + t) * D + g * Cg + c] : 0.0f;
}

// ---- gate[m][h] = a (b grep_a[h] - 1) + 2, (a, b) = sigmoid of the two 4-sums of grep_linear(x[m][64 h .. 64 h + 63])
__global__ __launch_bounds__(256) void wavlm_gate_kernel(const float* __restrict__ x, const float* __restrict__ Wg,
                                                         const float* __restrict__ bg, const float* __restrict__ grep_a,
                                                         int64_t total, int H, float* __restrict__ gate) {
  __shared__ float w[8 * HD + 8];
  for (int i = threadIdx.x; i < 8 * HD + 8; i += 256) w[i] = i < 8 * HD ? Wg[i] : bg[i - 8 * HD];
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int h = (int)(e % H);
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + e * HD);     // row m, head h: m H 64 + h 64 = e 64
  float s[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) s[o] = 0.0f;
#pragma unroll 4
  for (int c4 = 0; c4 < HD / 4; ++c4) {
    const f32x4 xv = xr[c4];
#pragma unroll
    for (int o = 0; o < 8; ++o)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[o] = fmaf(xv[j], w[o * HD + c4 * 4 + j], s[o]);
  }
#pragma unroll
  for (int o = 0; o < 8; ++o) s[o] = f_add(s[o], w[8 * HD + o]);
  const float sa = f_add(f_add(s[0], s[1]), f_add(s[2], s[3]));
  const float sb = f_add(f_add(s[4], s[5]), f_add(s[6], s[7]));
  const float ga = f_div(1.0f, f_add(1.0f, expf(-sa)));
  const float gb = f_div(1.0f, f_add(1.0f, expf(-sb)));
  gate[e] = f_add(f_mul(ga, f_sub(f_mul(gb, grep_a[h]), 1.0f)), 2.0f);
}

// ---- attention: qkv [B T][3 D] (q already scaled), gate [B T][H], relb [2T-1][H] (entry k - q + T - 1), out [B T][D]
__global__ __launch_bounds__(256) void wavlm_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ gate,
                                                         const float* __restrict__ relb, int T, int H,
                                                         float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float qs[QT][HD];
  __shared__ float S[QT][TMAX];
  __shared__ float rb[2 * TMAX];
  __shared__ float gs[QT];
  __shared__ float rsum[QT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q0 = blockIdx.x * QT, h = blockIdx.y, b = blockIdx.z;
  const int D = H * HD;
  const int nq = min(QT, T - q0);
  const float* base = qkv + (int64_t)b * T * 3 * D + h * HD;

  for (int e = tid; e < QT * HD; e += 256) {
    const int qi = e >> 6, c = e & 63;
    qs[qi][c] = qi < nq ? base[(int64_t)(q0 + qi) * 3 * D + c] : 0.0f;
  }
  for (int e = tid; e < 2 * T - 1; e += 256) rb[e] = relb[(int64_t)e * H + h];
  if (tid < QT) gs[tid] = tid < nq ? gate[((int64_t)b * T + q0 + tid) * H + h] : 0.0f;
  __syncthreads();

  // scores: thread = key
  if (tid < T) {
    f32x4 kr[HD / 4];
    const f32x4* kp = reinterpret_cast<const f32x4*>(base + (int64_t)tid * 3 * D + D);
#pragma unroll
    for (int c4 = 0; c4 < HD / 4; ++c4) kr[c4] = kp[c4];
    for (int qi = 0; qi < nq; ++qi) {
      const f32x4* qp = reinterpret_cast<const f32x4*>(qs[qi]);
      float s = 0.0f;
#pragma unroll
      for (int c4 = 0; c4 < HD / 4; ++c4) {
        const f32x4 qv = qp[c4];
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(qv[j], kr[c4][j], s);
      }
      S[qi][tid] = f_add(s, f_mul(gs[qi], rb[tid - (q0 + qi) + T - 1]));
    }
  }
  __syncthreads();

  // softmax numerators (row maximum subtracted) and row sums: wave w owns rows w, w + 4, ..
  for (int qi = w; qi < nq; qi += 4) {
    float m = -INFINITY;
    for (int k = lane; k < T; k += 64) m = fmaxf(m, S[qi][k]);
    m = wave_max(m);
    float s = 0.0f;
    for (int k = lane; k < T; k += 64) {
      const float e = expf(f_sub(S[qi][k], m));
      S[qi][k] = e;
      s = f_add(s, e);
    }
    s = wave_sum(s);
    if (lane == 0) rsum[qi] = s;
  }
  __syncthreads();

  // P V: thread (d, qg) owns output channel d of queries 4 qg .. 4 qg + 3
  const int d = lane, qg = w;
  const float* vp = base + 2 * D + d;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
  for (int k = 0; k < T; ++k) {
    const float v = vp[(int64_t)k * 3 * D];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fmaf(S[qg * 4 + j][k], v, acc[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int qi = qg * 4 + j;
    if (qi < nq) out[((int64_t)b * T + q0 + qi) * D + h * HD + d] = f_div(acc[j], rsum[qi]);
  }
}

// ---- x[m][:] = 0 for the rows with row_mask[m] != 0 (the padded frames ahead of pos_conv); other rows are not written
__global__ __launch_bounds__(256) void wavlm_mask_rows_kernel(float* __restrict__ x, const uint8_t* __restrict__ row_mask,
                                                              int64_t total, int C) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  if (row_mask[e / C]) x[e] = 0.0f;
}

// ---- tiled attention: the operands of wavlm_attn_kernel plus key_mask [B][T] (nonzero: the key is excluded) or NULL.
// A block owns LQ = 128 queries of one (batch, head), 32 per wave, and walks the keys in tiles of LK = 64.  Both products
// are computed TRANSPOSED so that a query is a matrix-core COLUMN, i.e. one lane (and its partner lane + 32):
//   S^T [key][query] = K [key][d] Q^T [d][query]      A = K from LDS, B = the wave's Q fragment, held in registers;
//   O^T [d][query]   = V^T [d][key] P^T [key][query]  A = V from LDS, B = the S^T registers as they stand: register r of
//                      a lane holds key (r & 3) + 8 (r >> 2) + 4 (lane >> 5), and step r of the second product takes
//                      exactly that key pair, so P never travels through LDS.
// The running maximum m, the running sum l and the rescale factor are therefore per-lane scalars.  Online softmax: per
// key tile m' = max(m, tile max), alpha = exp(m - m'), l = l alpha + sum p, O = O alpha + P V; out = O / l at the end.
// A masked key (and a key past T in the last tile) is staged as zeros and its weight is SELECTED to 0, its score to -inf
// ahead of the maximum: nothing read from it reaches a result.  A tile without a valid key is skipped by the whole
// block, so m is finite from the first tile that is not.  Per (query tile, key tile) the LQ + LK - 1 table entries
// k - q in [k0 - q0 - (LQ - 1), k0 - q0 + LK - 1] are staged.
constexpr int LQ = 128, LK = 64, KLD = HD + 1;

__global__ __launch_bounds__(256) void wavlm_attn_tiled_kernel(const float* __restrict__ qkv, const float* __restrict__ gate,
                                                               const float* __restrict__ relb,
                                                               const uint8_t* __restrict__ key_mask, int T, int H,
                                                               float* __restrict__ out) {
  __shared__ float Ks[LK][KLD];
  __shared__ __attribute__((aligned(16))) float Vs[LK][HD];
  __shared__ float bs[LQ + LK];
  __shared__ int vf[LK];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lk = lane >> 5;
  const int q0 = blockIdx.x * LQ, h = blockIdx.y, b = blockIdx.z;
  const int D = H * HD;
  const float* base = qkv + (int64_t)b * T * 3 * D + h * HD;
  const uint8_t* km = key_mask ? key_mask + (int64_t)b * T : nullptr;
  const int ql = w * 32 + lr, q = q0 + ql;
  const bool qlive = q < T;

  // the wave's Q^T fragment: lane (lr, lk) holds channels 32 lk .. 32 lk + 31 of query lr; step j of the first product
  // pairs channel j (lanes < 32) with channel 32 + j (lanes >= 32)
  f32x4 qf[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    qf[i] = qlive ? *reinterpret_cast<const f32x4*>(base + (int64_t)q * 3 * D + 32 * lk + 4 * i) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const float g = qlive ? gate[((int64_t)b * T + q) * H + h] : 0.0f;
  float m = -INFINITY, l = 0.0f;
  f32x16 acc[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.0f;

  const int sr = tid >> 2, skq = tid & 3;              // staging: thread (sr, skq) takes 16 channels of key k0 + sr
  for (int k0 = 0; k0 < T; k0 += LK) {
    __syncthreads();
    const int key = k0 + sr;
    const bool valid = key < T && !(km && km[key]);
    const float* kp = base + (int64_t)min(key, T - 1) * 3 * D + D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = skq * 4 + 16 * i;
      f32x4 kv = {0.0f, 0.0f, 0.0f, 0.0f}, vv = {0.0f, 0.0f, 0.0f, 0.0f};
      if (valid) {
        kv = *reinterpret_cast<const f32x4*>(kp + d);
        vv = *reinterpret_cast<const f32x4*>(kp + D + d);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) Ks[sr][d + j] = kv[j];
      *reinterpret_cast<f32x4*>(&Vs[sr][d]) = vv;
    }
    if (skq == 0) vf[sr] = valid ? 1 : 0;
    if (tid < LQ + LK - 1) {                           // table entry of k - q = k0 - q0 - (LQ - 1) + tid
      const int64_t gi = (int64_t)k0 - q0 - (LQ - 1) + (T - 1) + tid;
      bs[tid] = (gi >= 0 && gi <= 2 * (int64_t)T - 2) ? relb[gi * H + h] : 0.0f;
    }
    if (!__syncthreads_or(valid ? 1 : 0)) continue;    // no valid key in the tile: the block skips it

    f32x16 s[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[st][r] = 0.0f;
#pragma unroll
      for (int j = 0; j < 32; ++j)
        s[st] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[st * 32 + lr][j + 32 * lk], qf[j >> 2][j & 3], s[st], 0, 0, 0);
    }
    float mt = -INFINITY;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kl = st * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        const float sc = f_add(s[st][r], f_mul(g, bs[kl - ql + LQ - 1]));
        s[st][r] = vf[kl] ? sc : -INFINITY;
        mt = fmaxf(mt, s[st][r]);
      }
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);
    const float alpha = expf(f_sub(m, mn));            // (m = -inf ahead of the first tile: 0)
    m = mn;
    float rs = 0.0f;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kl = st * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        const float p = vf[kl] ? expf(f_sub(s[st][r], mn)) : 0.0f;
        s[st][r] = p;
        rs = f_add(rs, p);
      }
    rs = f_add(rs, __shfl_xor(rs, 32, 64));
    l = f_add(f_mul(l, alpha), rs);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[dt][r] = f_mul(acc[dt][r], alpha);
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kl = st * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          acc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[kl][dt * 32 + lr], s[st][r], acc[dt], 0, 0, 0);
      }
  }
  if (!qlive) return;
  float* o = out + ((int64_t)b * T + q) * D + h * HD;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk] = f_div(acc[dt][r], l);
}

static inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

#define WAVLM_UNSUP(cond, ...)      \
  do {                              \
    if (!(cond)) {                  \
      qpg_set_error(__VA_ARGS__);   \
      return QPG_EUNSUP;            \
    }                               \
  } while (0)

extern "C" int64_t qpg_wavlm_conv_frames(int64_t t_in, int k, int s) {
  if (k < 1 || s < 1 || t_in < k) return 0;
  return (t_in - k) / s + 1;
}

extern "C" int qpg_wavlm_conv0_f32(qpg_ctx* ctx, void* stream, const float* wav, int B, int64_t n, const float* w,
                                   const float* bias, int C, int k, int s, float* out) {
  QPG_REQUIRE(ctx, "qpg_wavlm_conv0_f32: null context");
  QPG_REQUIRE(wav && w && out, "qpg_wavlm_conv0_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && C >= 1 && k >= 1 && s >= 1 && n >= k, "qpg_wavlm_conv0_f32: need B, C, k, s >= 1 and n >= k "
              "(B %d, C %d, k %d, s %d, n %lld)", B, C, k, s, (long long)n);
  const int64_t T = qpg_wavlm_conv_frames(n, k, s);
  const int64_t total = (int64_t)B * T * C;
  QPG_REQUIRE(total <= ((int64_t)1 << 38), "qpg_wavlm_conv0_f32: %lld outputs are more than 2^38", (long long)total);
  const int64_t threads = (int64_t)B * ((T + C0T - 1) / C0T) * C;
  hipLaunchKernelGGL(wavlm_conv0_kernel, dim3(blocks256(threads)), dim3(256), 0, qpg_stream(stream), wav, n, w, bias, C,
                     k, s, T, threads, out);
  QPG_LAUNCH_CHECK("wavlm_conv0_kernel");
  return QPG_OK;
}

extern "C" int qpg_wavlm_layernorm_f32(qpg_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta,
                                       int64_t M, int C, float eps, int gelu, float* y) {
  QPG_REQUIRE(ctx, "qpg_wavlm_layernorm_f32: null context");
  QPG_REQUIRE(x && gamma && beta && y, "qpg_wavlm_layernorm_f32: null pointer argument");
  QPG_REQUIRE(M >= 0 && M <= ((int64_t)1 << 32) && C >= 1, "qpg_wavlm_layernorm_f32: need 0 <= M <= 2^32 rows of C >= 1 "
              "(M %lld, C %d)", (long long)M, C);
  if (M == 0) return QPG_OK;
  hipLaunchKernelGGL(wavlm_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, qpg_stream(stream), x, gamma, beta, M,
                     C, eps, gelu, y);
  QPG_LAUNCH_CHECK("wavlm_ln_kernel");
  return QPG_OK;
}

extern "C" int qpg_wavlm_gemm_f32(qpg_ctx* ctx, void* stream, const float* A, int64_t lda, const float* W,
                                  const float* bias, const float* residual, float* out, int64_t ldc, int M, int N, int K,
                                  int gelu, int n_outer, int n_inner, int64_t a_outer, int64_t a_inner, int64_t w_inner,
                                  int64_t bias_inner, int64_t c_outer, int64_t c_inner) {
  QPG_REQUIRE(ctx, "qpg_wavlm_gemm_f32: null context");
  QPG_REQUIRE(A && W && out, "qpg_wavlm_gemm_f32: null pointer argument");
  QPG_REQUIRE(M >= 1 && N >= 1 && K >= 1 && n_outer >= 1 && n_inner >= 1 && (int64_t)n_outer * n_inner <= 65535,
              "qpg_wavlm_gemm_f32: need M, N, K >= 1 and 1 <= n_outer * n_inner <= 65535 (M %d, N %d, K %d, %d x %d)", M, N,
              K, n_outer, n_inner);
  QPG_REQUIRE((M + BM - 1) / BM <= 65535, "qpg_wavlm_gemm_f32: M %d is more than %d rows", M, 65535 * BM);
  WAVLM_UNSUP(K % BK == 0, "qpg_wavlm_gemm_f32: K %d is not a multiple of %d", K, BK);
  QPG_REQUIRE(lda >= 1 && ldc >= N && lda % 4 == 0 && a_outer % 4 == 0 && a_inner % 4 == 0 && w_inner % 4 == 0 &&
              ((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0,
              "qpg_wavlm_gemm_f32: A and W must be 16-byte aligned with strides that are multiples of 4 floats, ldc >= N "
              "(lda %lld, ldc %lld)", (long long)lda, (long long)ldc);
  GemmArgs p;
  p.A = A; p.W = W; p.bias = bias; p.R = residual; p.C = out;
  p.M = M; p.N = N; p.K = K; p.n_inner = n_inner; p.gelu = gelu;
  p.lda = lda; p.ldc = ldc; p.sA0 = a_outer; p.sA1 = a_inner; p.sW1 = w_inner; p.sB1 = bias_inner;
  p.sC0 = c_outer; p.sC1 = c_inner;
  const dim3 grid((unsigned)((N + BN - 1) / BN), (unsigned)((M + BM - 1) / BM), (unsigned)(n_outer * n_inner));
  hipLaunchKernelGGL(wavlm_gemm_kernel, grid, dim3(256), 0, qpg_stream(stream), p);
  QPG_LAUNCH_CHECK("wavlm_gemm_kernel");
  return QPG_OK;
}

extern "C" int qpg_wavlm_pos_pad_f32(qpg_ctx* ctx, void* stream, const float* x, int B, int T, int D, int groups, int taps,
                                     float* padded) {
  QPG_REQUIRE(ctx, "qpg_wavlm_pos_pad_f32: null context");
  QPG_REQUIRE(x && padded, "qpg_wavlm_pos_pad_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && T >= 1 && D >= 1 && groups >= 1 && taps >= 1 && D % groups == 0,
              "qpg_wavlm_pos_pad_f32: need B, T, taps >= 1 and D a multiple of groups (B %d, T %d, D %d, groups %d, taps %d)",
              B, T, D, groups, taps);
  const int rows = T + taps - 1;
  const int64_t total = (int64_t)B * rows * D;
  hipLaunchKernelGGL(wavlm_pos_pad_kernel, dim3(blocks256(total)), dim3(256), 0, qpg_stream(stream), x, T, D, groups, rows,
                     taps / 2, total, padded);
  QPG_LAUNCH_CHECK("wavlm_pos_pad_kernel");
  return QPG_OK;
}

extern "C" int qpg_wavlm_gate_f32(qpg_ctx* ctx, void* stream, const float* x_ln, const float* grep_w, const float* grep_b,
                                  const float* grep_a, int64_t M, int H, float* gate) {
  QPG_REQUIRE(ctx, "qpg_wavlm_gate_f32: null context");
  QPG_REQUIRE(x_ln && grep_w && grep_b && grep_a && gate, "qpg_wavlm_gate_f32: null pointer argument");
  QPG_REQUIRE(M >= 1 && H >= 1 && M * H <= ((int64_t)1 << 38), "qpg_wavlm_gate_f32: need M, H >= 1 (M %lld, H %d)",
              (long long)M, H);
  QPG_REQUIRE(((uintptr_t)x_ln & 15) == 0, "qpg_wavlm_gate_f32: x_ln must be 16-byte aligned");
  hipLaunchKernelGGL(wavlm_gate_kernel, dim3(blocks256(M * H)), dim3(256), 0, qpg_stream(stream), x_ln, grep_w, grep_b,
                     grep_a, M * H, H, gate);
  QPG_LAUNCH_CHECK("wavlm_gate_kernel");
  return QPG_OK;
}

extern "C" int qpg_wavlm_attention_f32(qpg_ctx* ctx, void* stream, const float* qkv, const float* gate, const float* relb,
                                       int B, int T, int H, float* out) {
  QPG_REQUIRE(ctx, "qpg_wavlm_attention_f32: null context");
  QPG_REQUIRE(qkv && gate && relb && out, "qpg_wavlm_attention_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && H >= 1 && H <= 65535,
              "qpg_wavlm_attention_f32: need 1 <= B, H <= 65535 and T >= 1 (B %d, T %d, H %d)", B, T, H);
  WAVLM_UNSUP(T <= TMAX, "qpg_wavlm_attention_f32: %d frames, the kernel takes at most %d", T, TMAX);
  QPG_REQUIRE(((uintptr_t)qkv & 15) == 0, "qpg_wavlm_attention_f32: qkv must be 16-byte aligned");
  hipLaunchKernelGGL(wavlm_attn_kernel, dim3((unsigned)((T + QT - 1) / QT), (unsigned)H, (unsigned)B), dim3(256), 0,
                     qpg_stream(stream), qkv, gate, relb, T, H, out);
  QPG_LAUNCH_CHECK("wavlm_attn_kernel");
  return QPG_OK;
}

extern "C" int qpg_wavlm_mask_rows_f32(qpg_ctx* ctx, void* stream, float* x, const uint8_t* row_mask, int64_t M, int C) {
  QPG_REQUIRE(ctx, "qpg_wavlm_mask_rows_f32: null context");
  QPG_REQUIRE(x && row_mask, "qpg_wavlm_mask_rows_f32: null pointer argument");
  QPG_REQUIRE(M >= 0 && C >= 1 && M <= ((int64_t)1 << 38) / C, "qpg_wavlm_mask_rows_f32: need M >= 0, C >= 1 and at most 2^38 "
              "elements (M %lld, C %d)", (long long)M, C);
  if (M == 0) return QPG_OK;
  hipLaunchKernelGGL(wavlm_mask_rows_kernel, dim3(blocks256(M * C)), dim3(256), 0, qpg_stream(stream), x, row_mask, M * C, C);
  QPG_LAUNCH_CHECK("wavlm_mask_rows_kernel");
  return QPG_OK;
}

extern "C" int qpg_wavlm_attention_tiled_f32(qpg_ctx* ctx, void* stream, const float* qkv, const float* gate,
                                             const float* relb, const uint8_t* key_mask, int B, int T, int H, float* out) {
  QPG_REQUIRE(ctx, "qpg_wavlm_attention_tiled_f32: null context");
  QPG_REQUIRE(qkv && gate && relb && out, "qpg_wavlm_attention_tiled_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && H >= 1 && H <= 65535,
              "qpg_wavlm_attention_tiled_f32: need 1 <= B, H <= 65535 and T >= 1 (B %d, T %d, H %d)", B, T, H);
  WAVLM_UNSUP(T <= QPG_WAVLM_MAX_FRAMES_LONG, "qpg_wavlm_attention_tiled_f32: %d frames, the kernel takes at most %d", T,
              QPG_WAVLM_MAX_FRAMES_LONG);
  QPG_REQUIRE(((uintptr_t)qkv & 15) == 0, "qpg_wavlm_attention_tiled_f32: qkv must be 16-byte aligned");
  hipLaunchKernelGGL(wavlm_attn_tiled_kernel, dim3((unsigned)((T + LQ - 1) / LQ), (unsigned)H, (unsigned)B), dim3(256), 0,
                     qpg_stream(stream), qkv, gate, relb, key_mask, T, H, out);
  QPG_LAUNCH_CHECK("wavlm_attn_tiled_kernel");
  return QPG_OK;
}
