// The GRU speech-to-code generator (codebook/generate/generate.py Generator_gru, inference): the kernels behind
// qpgesture_amd/generate.py.  Everything is f32.  Activations are channels-last rows [B][T][C], as in qpg_wavlm.hip, and
// the GRU's input projections and the head's Linear are calls of qpg_wavlm_gemm_f32; what is here is the rest.
//
// gen_conv_in1_kernel   the first convolution (1 -> Cout channels, 16 taps) straight from the samples, on the VALU: a thread
//                       owns 8 channels of one output frame, the weights sit in LDS;
// gen_conv_mfma_kernel  the other four as implicit GEMMs on v_mfma_f32_16x16x4_f32: output frame t reads the 16 Cin
//                       CONTIGUOUS floats that start at input frame stride * t, the weights are repacked to [Cout][16][Cin].
//                       A wave owns 32 frames x all Cout channels, a block CT = 128 frames of one batch member.  The last
//                       frame's window ends at sample stride (T - 1) + 15, so the (Tin - 16) % stride trailing frames are
//                       never addressed; frames past T in a tile are redirected to frame T - 1 and not stored;
//                       both end in the same epilogue: + bias, the eval-mode BatchNorm affine (optional), LeakyReLU (optional).
// gen_gru_kernel        the recurrence of one bidirectional layer.  ONE BLOCK OWNS GBT = 16 SEQUENCES OF ONE DIRECTION FOR
//                       ALL T STEPS: h lives in LDS (two copies, one barrier per step), W_hh is streamed from L2 every step.
//                       Wave w of 13 owns hidden units 16 w .. 16 w + 15 and computes their three gate rows for the 16
//                       sequences as W_hh (A, 16 units x 4 k) times h^T (B, 4 k x 16 sequences); the accumulator layout puts
//                       the r, z and n pre-activations of 4 units of one sequence in one lane, which finishes the step
//                       in registers.  No launch synchronises between blocks: there is no grid barrier, no cooperative
//                       launch and no flag in global memory, and one sequence's gate rows are never split over blocks.
//                       A matrix-core column is one sequence, so a sequence's bits depend neither on B nor on its place.
// gen_head_ln_kernel    direction sum + LayerNorm(200), written as rows of 208 with zero padding (the GEMM wants K % 16 == 0);
// gen_argmax_kernel     first index of a row's maximum;
// gen_ce_rows_kernel / gen_ce_mean_kernel   cross-entropy per row, then the mean over rows in f64 in a fixed order.
#include "qpg_common.h"

namespace {

constexpr int TAPS = QPG_GEN_TAPS;             // 16
constexpr int GH = QPG_GEN_HIDDEN;             // 200
constexpr int GBT = QPG_GEN_GRU_BATCH_TILE;    // 16 sequences per recurrence block
constexpr int CT = QPG_GEN_CONV_TIME_TILE;     // 128 output frames per convolution block
constexpr int HLD = QPG_GEN_HEAD_LD;           // 208
constexpr int GWAVES = (GH + 15) / 16;         // 13
constexpr int HS_LD = GH + 4;                  // LDS row stride of h
constexpr int KCH = (GH + 15) / 16;            // 16-k chunks of a gate row: 13, the last one half full

// + bias, (v - mean) / sqrt(var + eps) * g + b with bn = [4][Cout] (weight, bias, running_mean, running_var), LeakyReLU
__device__ __forceinline__ float gen_epilogue(float v, int c, int Cout, const float* __restrict__ bias,
                                              const float* __restrict__ bn, float eps, int act, float slope) {
  if (bias) v = f_add(v, bias[c]);
  if (bn) {
    const float inv = f_div(1.0f, f_sqrt(f_add(bn[3 * Cout + c], eps)));
    v = f_add(f_mul(f_mul(f_sub(v, bn[2 * Cout + c]), inv), bn[c]), bn[Cout + c]);
  }
  if (act) v = v > 0.0f ? v : f_mul(v, slope);
  return v;
}

// ---- Cin = 1: out[b][t][c] = epilogue(sum_j w[c][j] x[b][stride t + j])
__global__ __launch_bounds__(256) void gen_conv_in1_kernel(const float* __restrict__ x, int64_t Tin,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           const float* __restrict__ bn, float eps, int act, float slope,
                                                           int Cout, int stride, int64_t T, int64_t total,
                                                           float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float ws[64 * TAPS];
  for (int i = threadIdx.x; i < Cout * TAPS; i += 256) ws[i] = w[i];
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int ncg = Cout >> 3;
  const int cg = (int)(e % ncg);
  const int64_t bt = e / ncg;
  const int64_t b = bt / T, t = bt - b * T;
  const float* xp = x + b * Tin + t * stride;
  float xs[TAPS];
#pragma unroll
  for (int j = 0; j < TAPS; ++j) xs[j] = xp[j];
  float o[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const f32x4* wc = reinterpret_cast<const f32x4*>(ws + (cg * 8 + c) * TAPS);
    float acc = 0.0f;
#pragma unroll
    for (int j4 = 0; j4 < TAPS / 4; ++j4) {
      const f32x4 wv = wc[j4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(wv[j], xs[j4 * 4 + j], acc);
    }
    o[c] = gen_epilogue(acc, cg * 8 + c, Cout, bias, bn, eps, act, slope);
  }
  f32x4* op = reinterpret_cast<f32x4*>(out + (b * T + t) * Cout + cg * 8);
  op[0] = f32x4{o[0], o[1], o[2], o[3]};
  op[1] = f32x4{o[4], o[5], o[6], o[7]};
}

// ---- Cin % 4 == 0, Cout = 16 NT: the implicit GEMM.  Per 16 k, lane (j = lane & 15, g = lane >> 4) loads the 4
// consecutive k = k0 + 4 g .. + 3 of weight row j (A) and of frame j's window (B); matrix step q pairs the q-th of them
// across the four lane groups.  Accumulator register r of the lane is channel 16 nt + 4 g + r of frame j.
template <int NT>
__global__ __launch_bounds__(256) void gen_conv_mfma_kernel(const float* __restrict__ x, int64_t Tin, int Cin,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            const float* __restrict__ bn, float eps, int act, float slope,
                                                            int stride, int64_t T, float* __restrict__ out) {
  constexpr int Cout = 16 * NT;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.y;
  const int64_t t0 = (int64_t)blockIdx.x * CT + wv * 32;
  if (t0 >= T) return;                                  // (the kernel has no barrier)
  const int j = lane & 15, g = lane >> 4;
  const int K = TAPS * Cin;
  const float* xr[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int64_t t = min(t0 + mt * 16 + j, T - 1);
    xr[mt] = x + (b * Tin + t * stride) * Cin + 4 * g;
  }
  const float* wr[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wr[nt] = w + (int64_t)(nt * 16 + j) * K + 4 * g;
  f32x4 acc[NT][2];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int k0 = 0; k0 < K; k0 += 32) {                  // (K = 16 Cin is a multiple of 64)
    f32x4 a[2][NT], bb[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) a[h][nt] = *reinterpret_cast<const f32x4*>(wr[nt] + k0 + 16 * h);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) bb[h][mt] = *reinterpret_cast<const f32x4*>(xr[mt] + k0 + 16 * h);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
            acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][nt][q], bb[h][mt][q], acc[nt][mt], 0, 0, 0);
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int64_t t = t0 + mt * 16 + j;
    if (t >= T) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int c0 = nt * 16 + 4 * g;
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = gen_epilogue(acc[nt][mt][r], c0 + r, Cout, bias, bn, eps, act, slope);
      *reinterpret_cast<f32x4*>(out + (b * T + t) * Cout + c0) = o;
    }
  }
}

// ---- the recurrence.  xp [B][T][2][3 H] = W_ih x + b_ih of both directions (gates r, z, n), whh [2][3 H][H], bhh [2][3 H],
// out [B][T][2 H].  Direction 1 walks t = T - 1 .. 0 with the same instructions as direction 0.
__device__ __forceinline__ float gen_sigmoid(float v) { return f_div(1.0f, f_add(1.0f, expf(-v))); }

__global__ __launch_bounds__(GWAVES * 64) void gen_gru_kernel(const float* __restrict__ xp, const float* __restrict__ whh,
                                                              const float* __restrict__ bhh, int B, int T,
                                                              float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float hs[2][GBT][HS_LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y;
  const int j = lane & 15, g = lane >> 4;
  // A operand: gate rows of unit 16 wv + j (past the end: unit H - 1, its results land in rows nobody keeps)
  const int ua = min(wv * 16 + j, GH - 1);
  const float* wrow[3];
#pragma unroll
  for (int gate = 0; gate < 3; ++gate) wrow[gate] = whh + ((int64_t)(dir * 3 + gate) * GH + ua) * GH + 4 * g;
  // D: units u0 .. u0 + 3 of sequence b0 + j
  const int u0 = wv * 16 + 4 * g;
  const bool uvalid = u0 < GH;                           // (H % 4 == 0: all four or none)
  const int64_t seq = (int64_t)blockIdx.x * GBT + j;
  const bool svalid = seq < B;
  const int64_t seqc = svalid ? seq : B - 1;             // (a column past B repeats the last sequence and is not stored)
  const float* bhp = bhh + dir * 3 * GH + u0;            // (read per step: three registers instead of twelve)
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
    for (int c0 = 0; c0 < KCH; c0 += 4) {                // four 16-k chunks' loads in flight, no more: 128 registers
      f32x4 hb[4], a[4][3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k0 = (c0 + i) * 16 + 4 * g;
        const bool kvalid = k0 < GH;                     // (the last chunk holds 8 k: lane groups 2, 3 feed zeros)
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
      f32x4 hn;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float rr = gen_sigmoid(f_add(xg[0][r], f_add(acc[0][r], bh[0][r])));
        const float zz = gen_sigmoid(f_add(xg[1][r], f_add(acc[1][r], bh[1][r])));
        const float nn = tanhf(f_add(xg[2][r], f_mul(rr, f_add(acc[2][r], bh[2][r]))));
        hn[r] = f_add(f_mul(f_sub(1.0f, zz), nn), f_mul(zz, hp[r]));
      }
      *reinterpret_cast<f32x4*>(&hs[cur ^ 1][j][u0]) = hn;
      if (svalid) *reinterpret_cast<f32x4*>(out + (seq * T + t) * (2 * GH) + dir * GH + u0) = hn;
    }
    __syncthreads();        // h of this step is complete, and nobody still reads the copy the next step overwrites
  }
}

__device__ __forceinline__ float gen_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = f_add(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- y[row][0 .. H) = LayerNorm(x[row][0 .. H) + x[row][H .. 2 H)) g + b, y[row][H .. HLD) = 0; one wave per row
__global__ __launch_bounds__(256) void gen_head_ln_kernel(const float* __restrict__ x, const float* __restrict__ gm,
                                                          const float* __restrict__ bt, int64_t R, float eps,
                                                          float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + row * (2 * GH);
  float v[4], s = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < GH ? f_add(xr[c], xr[GH + c]) : 0.0f;
    s = f_add(s, v[i]);
  }
  const float mean = f_div(gen_wave_sum(s), (float)GH);
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float d = lane + 64 * i < GH ? f_sub(v[i], mean) : 0.0f;
    q = fmaf(d, d, q);
  }
  const float rstd = f_div(1.0f, f_sqrt(f_add(f_div(gen_wave_sum(q), (float)GH), eps)));
  float* yr = y + row * HLD;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < GH) yr[c] = f_add(f_mul(f_mul(f_sub(v[i], mean), rstd), gm[c]), bt[c]);
    else if (c < HLD) yr[c] = 0.0f;
  }
}

// ---- codes[row] = the lowest index of the row's maximum; one wave per row
__global__ __launch_bounds__(256) void gen_argmax_kernel(const float* __restrict__ logits, int64_t R, int N,
                                                         int64_t* __restrict__ codes) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* lr = logits + row * N;
  float best = -INFINITY;
  int bi = N;                                            // (a lane without a candidate loses every comparison)
  for (int c = lane; c < N; c += 64) {
    const float v = lr[c];
    if (v > best || bi == N) {
      best = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi < N && (bi == N || ov > best || (ov == best && oi < bi))) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) codes[row] = bi;
}

// ---- rowloss[row] = log(sum_c exp(l[c] - max)) + max - l[target]; a target outside [0, N) gives NaN and is not read
__global__ __launch_bounds__(256) void gen_ce_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                          int64_t R, int N, float* __restrict__ rowloss) {
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
  s = gen_wave_sum(s);
  if (lane == 0) {
    const int64_t tg = target[row];
    rowloss[row] = (tg >= 0 && tg < N) ? f_sub(f_add(logf(s), m), lr[tg]) : __builtin_nanf("");
  }
}

// one block: thread i adds rows i, i + 256, .. in f64, then a fixed tree over the 256 partial sums
__global__ __launch_bounds__(256) void gen_ce_mean_kernel(const float* __restrict__ rowloss, int64_t R,
                                                          float* __restrict__ loss) {
  __shared__ double part[256];
  double s = 0.0;
  for (int64_t r = threadIdx.x; r < R; r += 256) s = f_add(s, (double)rowloss[r]);
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] = f_add(part[threadIdx.x], part[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)f_div(part[0], (double)R);
}

}  // namespace

#define GEN_UNSUP(cond, ...)        \
  do {                              \
    if (!(cond)) {                  \
      qpg_set_error(__VA_ARGS__);   \
      return QPG_EUNSUP;            \
    }                               \
  } while (0)

extern "C" int64_t qpg_gen_conv_frames(int64_t t_in, int stride) {
  if (stride < 1 || t_in < TAPS) return 0;
  return (t_in - TAPS) / stride + 1;
}

extern "C" int qpg_gen_conv1d_f32(qpg_ctx* ctx, void* stream, const float* x, int B, int64_t Tin, int Cin, const float* w,
                                  const float* bias, const float* bn, float eps, int act, float slope, int Cout, int stride,
                                  float* out) {
  QPG_REQUIRE(ctx, "qpg_gen_conv1d_f32: null context");
  QPG_REQUIRE(x && w && out, "qpg_gen_conv1d_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && B <= 65535 && Cin >= 1 && Cout >= 1 && stride >= 1 && Tin >= TAPS && Tin <= ((int64_t)1 << 31),
              "qpg_gen_conv1d_f32: need 1 <= B <= 65535, Cin, Cout, stride >= 1 and %d <= Tin <= 2^31 (B %d, Cin %d, Cout %d, "
              "stride %d, Tin %lld)", TAPS, B, Cin, Cout, stride, (long long)Tin);
  const int64_t T = qpg_gen_conv_frames(Tin, stride);
  QPG_REQUIRE((Cin == 1 || ((uintptr_t)x & 15) == 0) && ((uintptr_t)w & 15) == 0 && ((uintptr_t)out & 15) == 0,
              "qpg_gen_conv1d_f32: x (with Cin > 1), w and out must be 16-byte aligned");
  hipStream_t s = qpg_stream(stream);
  if (Cin == 1) {
    GEN_UNSUP(Cout % 8 == 0 && Cout <= 64, "qpg_gen_conv1d_f32: with Cin 1, Cout %d is not a multiple of 8 up to 64", Cout);
    const int64_t total = (int64_t)B * T * (Cout / 8);
    QPG_REQUIRE(total <= ((int64_t)1 << 38), "qpg_gen_conv1d_f32: %lld outputs are too many", (long long)total);
    hipLaunchKernelGGL(gen_conv_in1_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, Tin, w, bias, bn, eps,
                       act, slope, Cout, stride, T, total, out);
    QPG_LAUNCH_CHECK("gen_conv_in1_kernel");
    return QPG_OK;
  }
  GEN_UNSUP(Cin % 4 == 0 && Cout % 16 == 0 && Cout <= 64,
            "qpg_gen_conv1d_f32: Cin %d must be 1 or a multiple of 4, Cout %d a multiple of 16 up to 64", Cin, Cout);
  const dim3 grid((unsigned)((T + CT - 1) / CT), (unsigned)B);
#define GEN_CONV_LAUNCH(NT)                                                                                              \
  hipLaunchKernelGGL(gen_conv_mfma_kernel<NT>, grid, dim3(256), 0, s, x, Tin, Cin, w, bias, bn, eps, act, slope, stride, T, \
                     out)
  switch (Cout / 16) {
    case 1: GEN_CONV_LAUNCH(1); break;
    case 2: GEN_CONV_LAUNCH(2); break;
    case 3: GEN_CONV_LAUNCH(3); break;
    default: GEN_CONV_LAUNCH(4); break;
  }
#undef GEN_CONV_LAUNCH
  QPG_LAUNCH_CHECK("gen_conv_mfma_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_gru_layer_f32(qpg_ctx* ctx, void* stream, const float* xp, const float* whh, const float* bhh, int B,
                                     int T, int H, float* out) {
  QPG_REQUIRE(ctx, "qpg_gen_gru_layer_f32: null context");
  QPG_REQUIRE(xp && whh && bhh && out, "qpg_gen_gru_layer_f32: null pointer argument");
  QPG_REQUIRE(B >= 1 && T >= 1 && H >= 1,
              "qpg_gen_gru_layer_f32: need B, T, H >= 1 (B %d, T %d, H %d)", B, T, H);
  GEN_UNSUP(H == GH, "qpg_gen_gru_layer_f32: hidden width %d, the kernel is built for %d", H, GH);
  QPG_REQUIRE(((uintptr_t)xp & 15) == 0 && ((uintptr_t)whh & 15) == 0 && ((uintptr_t)bhh & 15) == 0 &&
              ((uintptr_t)out & 15) == 0, "qpg_gen_gru_layer_f32: xp, whh, bhh and out must be 16-byte aligned");
  hipLaunchKernelGGL(gen_gru_kernel, dim3((unsigned)((B + GBT - 1) / GBT), 2), dim3(GWAVES * 64), 0, qpg_stream(stream), xp,
                     whh, bhh, B, T, out);
  QPG_LAUNCH_CHECK("gen_gru_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_head_ln_f32(qpg_ctx* ctx, void* stream, const float* x, const float* gamma, const float* beta,
                                   int64_t R, int H, float eps, float* y) {
  QPG_REQUIRE(ctx, "qpg_gen_head_ln_f32: null context");
  QPG_REQUIRE(x && gamma && beta && y, "qpg_gen_head_ln_f32: null pointer argument");
  QPG_REQUIRE(R >= 0 && R <= ((int64_t)1 << 32) && H >= 1, "qpg_gen_head_ln_f32: need 0 <= R <= 2^32 rows and H >= 1 "
              "(R %lld, H %d)", (long long)R, H);
  GEN_UNSUP(H == GH, "qpg_gen_head_ln_f32: hidden width %d, the kernel is built for %d", H, GH);
  if (R == 0) return QPG_OK;
  hipLaunchKernelGGL(gen_head_ln_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, qpg_stream(stream), x, gamma, beta, R,
                     eps, y);
  QPG_LAUNCH_CHECK("gen_head_ln_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_argmax_f32(qpg_ctx* ctx, void* stream, const float* logits, int64_t R, int N, int64_t* codes) {
  QPG_REQUIRE(ctx, "qpg_gen_argmax_f32: null context");
  QPG_REQUIRE(logits && codes, "qpg_gen_argmax_f32: null pointer argument");
  QPG_REQUIRE(R >= 0 && R <= ((int64_t)1 << 32) && N >= 1, "qpg_gen_argmax_f32: need 0 <= R <= 2^32 rows of N >= 1 "
              "(R %lld, N %d)", (long long)R, N);
  if (R == 0) return QPG_OK;
  hipLaunchKernelGGL(gen_argmax_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, qpg_stream(stream), logits, R, N, codes);
  QPG_LAUNCH_CHECK("gen_argmax_kernel");
  return QPG_OK;
}

extern "C" int qpg_gen_cross_entropy_f32(qpg_ctx* ctx, void* stream, const float* logits, const int64_t* target, int64_t R,
                                         int N, float* ws, float* loss) {
  QPG_REQUIRE(ctx, "qpg_gen_cross_entropy_f32: null context");
  QPG_REQUIRE(logits && target && ws && loss, "qpg_gen_cross_entropy_f32: null pointer argument");
  QPG_REQUIRE(R >= 1 && R <= ((int64_t)1 << 32) && N >= 1, "qpg_gen_cross_entropy_f32: need 1 <= R <= 2^32 rows of N >= 1 "
              "(R %lld, N %d)", (long long)R, N);
  hipLaunchKernelGGL(gen_ce_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, qpg_stream(stream), logits, target, R,
                     N, ws);
  QPG_LAUNCH_CHECK("gen_ce_rows_kernel");
  hipLaunchKernelGGL(gen_ce_mean_kernel, dim3(1), dim3(256), 0, qpg_stream(stream), ws, R, loss);
  QPG_LAUNCH_CHECK("gen_ce_mean_kernel");
  return QPG_OK;
}
