// vq-wav2vec code extraction (fairseq's Wav2VecModel.feature_extractor and GumbelVectorQuantizer.forward_idx, eval mode):
// the kernels behind qpgesture_amd/wavvq.py.  Everything is f32 over channels-last rows [B][T][C], as in qpg_wavlm.hip.
// Layer 0 is qpg_wavlm_conv0_f32, every later convolution and both Linears of the quantiser are qpg_wavlm_gemm_f32, and
// the per-group argmax is qpg_gen_argmax_f32 over the [R G][V] view of the logits; what is here is the rest.
//
// GroupNorm(1, C) normalises a WINDOW over all of its T C values, so one window's statistics span up to 26 MB (layer 0 of
// a 4 s window at C = 512) and a block per window would leave the machine empty at B = 1.  The window is cut into slabs of
// GN_SLAB consecutive floats, over time:
// wavvq_gn_stats_kernel   block (slab, b): sum and sum of squares of the slab in f64 (a thread adds its elements in index
//                         order, the block's 256 pairs go through a fixed tree) -> ws[(b S + slab)] = (sum, sum2) f64;
// wavvq_gn_finish_kernel  block b: the S pairs of window b added in f64 (thread i takes slabs i, i + 256, .. in order, then
//                         the same tree), mean and 1 / sqrt(var + eps) from the f64 sums -> two floats per window behind
//                         the partials.  f64 sums of f32 values and their squares: var = E[x^2] - mean^2 loses
//                         (mean / sigma)^2 x 2^-53 of its value, 1e-12 at a DC offset of 100 sigma;
// wavvq_gn_apply_kernel   block (slab, b): (v - mean) rstd gamma[c] + beta[c], then the epilogue (none / ReLU / ReLU and
//                         log(|v| + 1)), in place.
// The raw activations are read twice and written once; every access is a 16-byte vector per lane.  A slab's partial and a
// window's sums depend on the window's own values and T C alone: neither B nor the window's place in the batch enters.
// No atomics, no launch waits on another block.
// wavvq_relu_kernel       max(v, 0) in place (the hidden rows of the quantiser's weight_proj between its two GEMMs).
#include "qpg_common.h"

namespace {

constexpr int GN_SLAB = QPG_WAVVQ_GN_SLAB;      // 4096 floats = 16 KB: 4 vectors per thread
constexpr int GN_VEC = GN_SLAB / 4 / 256;       // f32x4 loads per thread and slab

static_assert(GN_SLAB % 1024 == 0, "a slab is a whole number of 256 x f32x4 passes");

// the block's 256 (a, b) pairs -> thread 0's (a, b): a fixed tree, so the result depends on the 256 inputs alone
__device__ __forceinline__ void gn_block_sum2(double& a, double& b, double (*part)[256]) {
  part[0][threadIdx.x] = a;
  part[1][threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      part[0][threadIdx.x] = f_add(part[0][threadIdx.x], part[0][threadIdx.x + o]);
      part[1][threadIdx.x] = f_add(part[1][threadIdx.x], part[1][threadIdx.x + o]);
    }
    __syncthreads();
  }
  a = part[0][0];
  b = part[1][0];
}

__global__ __launch_bounds__(256) void wavvq_gn_stats_kernel(const float* __restrict__ x, int64_t n, int S,
                                                             double* __restrict__ part_out) {
  __shared__ double part[2][256];
  const int64_t b = blockIdx.y;
  const int64_t e0 = (int64_t)blockIdx.x * GN_SLAB;
  const float* xw = x + b * n;
  f32x4 v[GN_VEC];
#pragma unroll
  for (int i = 0; i < GN_VEC; ++i) {
    const int64_t e = e0 + ((int64_t)i * 256 + threadIdx.x) * 4;         // (n % 4 == 0: a vector is inside or outside)
    v[i] = e < n ? *reinterpret_cast<const f32x4*>(xw + e) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int i = 0; i < GN_VEC; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)v[i][j];
      s = f_add(s, d);
      q = f_add(q, f_mul(d, d));
    }
  gn_block_sum2(s, q, part);
  if (threadIdx.x == 0) {
    double* o = part_out + (b * S + blockIdx.x) * 2;
    o[0] = s;
    o[1] = q;
  }
}

__global__ __launch_bounds__(256) void wavvq_gn_finish_kernel(const double* __restrict__ part_in, int64_t n, int S,
                                                              float eps, float* __restrict__ stat) {
  __shared__ double part[2][256];
  const int64_t b = blockIdx.x;
  const double* p = part_in + b * S * 2;
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < S; i += 256) {
    s = f_add(s, p[2 * i]);
    q = f_add(q, p[2 * i + 1]);
  }
  gn_block_sum2(s, q, part);
  if (threadIdx.x == 0) {
    const double mean = f_div(s, (double)n);
    double var = f_sub(f_div(q, (double)n), f_mul(mean, mean));
    if (!(var > 0.0)) var = 0.0;                                         // (silence: exactly 0; rounding may go below)
    stat[2 * b] = (float)mean;
    stat[2 * b + 1] = (float)f_div(1.0, sqrt(f_add(var, (double)eps)));
  }
}

template <int EPI>
__global__ __launch_bounds__(256) void wavvq_gn_apply_kernel(float* __restrict__ x, int64_t n, int C,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ stat) {
  const int64_t b = blockIdx.y;
  const int64_t e0 = (int64_t)blockIdx.x * GN_SLAB;
  float* xw = x + b * n;
  const float mean = stat[2 * b], rstd = stat[2 * b + 1];
  f32x4 v[GN_VEC];
#pragma unroll
  for (int i = 0; i < GN_VEC; ++i) {
    const int64_t e = e0 + ((int64_t)i * 256 + threadIdx.x) * 4;
    v[i] = e < n ? *reinterpret_cast<const f32x4*>(xw + e) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
#pragma unroll
  for (int i = 0; i < GN_VEC; ++i) {
    const int64_t e = e0 + ((int64_t)i * 256 + threadIdx.x) * 4;
    if (e >= n) continue;
    const int c = (int)(e % C);                                          // (C % 4 == 0: the vector stays in one row)
    const f32x4 g = gamma ? *reinterpret_cast<const f32x4*>(gamma + c) : f32x4{1.0f, 1.0f, 1.0f, 1.0f};
    const f32x4 bt = beta ? *reinterpret_cast<const f32x4*>(beta + c) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float r = f_add(f_mul(f_mul(f_sub(v[i][j], mean), rstd), g[j]), bt[j]);
      if (EPI >= QPG_WAVVQ_EPI_RELU) r = r > 0.0f ? r : 0.0f;
      if (EPI == QPG_WAVVQ_EPI_RELU_LOG) r = logf(f_add(fabsf(r), 1.0f));
      o[j] = r;
    }
    *reinterpret_cast<f32x4*>(xw + e) = o;
  }
}

__global__ __launch_bounds__(256) void wavvq_relu_kernel(float* __restrict__ x, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 v = reinterpret_cast<f32x4*>(x)[i];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.0f ? v[j] : 0.0f;
  reinterpret_cast<f32x4*>(x)[i] = v;
}

static inline int64_t gn_slabs(int64_t n) { return (n + GN_SLAB - 1) / GN_SLAB; }
static inline bool gn_shape_ok(int B, int64_t T, int C) {
  return B >= 1 && B <= 65535 && T >= 1 && C >= 1 && T <= ((int64_t)1 << 40) / C && gn_slabs(T * C) <= 0x7fffffff;
}

}  // namespace

#define WAVVQ_UNSUP(cond, ...)      \
  do {                              \
    if (!(cond)) {                  \
      qpg_set_error(__VA_ARGS__);   \
      return QPG_EUNSUP;            \
    }                               \
  } while (0)

extern "C" int64_t qpg_wavvq_groupnorm_ws_floats(int B, int64_t T, int C) {
  if (!gn_shape_ok(B, T, C)) return 0;
  return (int64_t)B * gn_slabs(T * C) * 4 + 2 * (int64_t)B;             // S (sum, sum2) f64 pairs + (mean, rstd) per window
}

extern "C" int qpg_wavvq_groupnorm_f32(qpg_ctx* ctx, void* stream, float* x, int B, int64_t T, int C, const float* gamma,
                                       const float* beta, float eps, int epilogue, float* ws, int64_t ws_floats) {
  QPG_REQUIRE(ctx, "qpg_wavvq_groupnorm_f32: null context");
  QPG_REQUIRE(x && ws, "qpg_wavvq_groupnorm_f32: null pointer argument");
  QPG_REQUIRE(gn_shape_ok(B, T, C), "qpg_wavvq_groupnorm_f32: need 1 <= B <= 65535, T, C >= 1 and T C <= 2^40 (B %d, T %lld, "
              "C %d)", B, (long long)T, C);
  QPG_REQUIRE(epilogue >= QPG_WAVVQ_EPI_NONE && epilogue <= QPG_WAVVQ_EPI_RELU_LOG && eps >= 0.0f,
              "qpg_wavvq_groupnorm_f32: epilogue %d is not 0, 1 or 2, or eps %g is negative", epilogue, (double)eps);
  WAVVQ_UNSUP(C % 4 == 0, "qpg_wavvq_groupnorm_f32: C %d is not a multiple of 4", C);
  QPG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)ws & 7) == 0 && (!gamma || ((uintptr_t)gamma & 15) == 0) &&
              (!beta || ((uintptr_t)beta & 15) == 0),
              "qpg_wavvq_groupnorm_f32: x, gamma and beta must be 16-byte aligned, ws 8-byte aligned");
  const int64_t need = qpg_wavvq_groupnorm_ws_floats(B, T, C);
  QPG_REQUIRE(ws_floats >= need, "qpg_wavvq_groupnorm_f32: ws holds %lld floats, %lld are needed", (long long)ws_floats,
              (long long)need);
  const int64_t n = T * C;
  const int S = (int)gn_slabs(n);
  double* part = reinterpret_cast<double*>(ws);
  float* stat = ws + (int64_t)B * S * 4;
  hipStream_t s = qpg_stream(stream);
  const dim3 grid((unsigned)S, (unsigned)B);
  hipLaunchKernelGGL(wavvq_gn_stats_kernel, grid, dim3(256), 0, s, x, n, S, part);
  QPG_LAUNCH_CHECK("wavvq_gn_stats_kernel");
  hipLaunchKernelGGL(wavvq_gn_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, part, n, S, eps, stat);
  QPG_LAUNCH_CHECK("wavvq_gn_finish_kernel");
  switch (epilogue) {
    case QPG_WAVVQ_EPI_NONE:
      hipLaunchKernelGGL(wavvq_gn_apply_kernel<QPG_WAVVQ_EPI_NONE>, grid, dim3(256), 0, s, x, n, C, gamma, beta, stat);
      break;
    case QPG_WAVVQ_EPI_RELU:
      hipLaunchKernelGGL(wavvq_gn_apply_kernel<QPG_WAVVQ_EPI_RELU>, grid, dim3(256), 0, s, x, n, C, gamma, beta, stat);
      break;
    default:
      hipLaunchKernelGGL(wavvq_gn_apply_kernel<QPG_WAVVQ_EPI_RELU_LOG>, grid, dim3(256), 0, s, x, n, C, gamma, beta, stat);
      break;
  }
  QPG_LAUNCH_CHECK("wavvq_gn_apply_kernel");
  return QPG_OK;
}

extern "C" int qpg_wavvq_relu_f32(qpg_ctx* ctx, void* stream, float* x, int64_t n) {
  QPG_REQUIRE(ctx, "qpg_wavvq_relu_f32: null context");
  QPG_REQUIRE(x, "qpg_wavvq_relu_f32: null pointer argument");
  QPG_REQUIRE(n >= 0 && n <= ((int64_t)1 << 40), "qpg_wavvq_relu_f32: need 0 <= n <= 2^40 (n %lld)", (long long)n);
  WAVVQ_UNSUP(n % 4 == 0, "qpg_wavvq_relu_f32: n %lld is not a multiple of 4", (long long)n);
  QPG_REQUIRE(((uintptr_t)x & 15) == 0, "qpg_wavvq_relu_f32: x must be 16-byte aligned");
  if (n == 0) return QPG_OK;
  hipLaunchKernelGGL(wavvq_relu_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, qpg_stream(stream), x, n / 4);
  QPG_LAUNCH_CHECK("wavvq_relu_kernel");
  return QPG_OK;
}

extern "C" int qpg_wavvq_group_argmax_f32(qpg_ctx* ctx, void* stream, const float* logits, int64_t R, int G, int V,
                                          int64_t* codes) {
  QPG_REQUIRE(ctx, "qpg_wavvq_group_argmax_f32: null context");
  QPG_REQUIRE(logits && codes, "qpg_wavvq_group_argmax_f32: null pointer argument");
  QPG_REQUIRE(R >= 0 && G >= 1 && V >= 1 && R <= ((int64_t)1 << 32) / G,
              "qpg_wavvq_group_argmax_f32: need R >= 0, G, V >= 1 and R G <= 2^32 (R %lld, G %d, V %d)", (long long)R, G, V);
  // a row of [G][V] logits is G contiguous rows of V: the per-group argmax is the row argmax of the [R G][V] view
  return qpg_gen_argmax_f32(ctx, stream, logits, R * G, V, codes);
}
