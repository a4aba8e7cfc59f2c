// Sentence embeddings (a BERT-shaped post-LN encoder, inference): the three kernels qpgesture_amd/sentence.py needs beside
// qpg_wavlm_gemm_f32 and qpg_wavlm_layernorm_f32 (qpg_wavlm.hip), which do every Linear and every LayerNorm of a block.
//
// Activations are PACKED RAGGED ROWS: sentence s owns the token rows seq_start[s] .. seq_start[s + 1] of an [R][D]
// array, nothing is padded and nothing is masked (a padded key's softmax weight is exactly 0 in the
// reference, a padded query is left out of its mean, so the packed form is the same function).
//
// bert_embed_ln_kernel   one wave per token row: word[id] + type[0] + pos[row - start of its sentence], LayerNorm (two
//                        passes, as wavlm_ln_kernel).  The row's sentence is found by bisection of seq_start.
// bert_attn_kernel       one wave per (sentence, head), head dim 32: K and V of the head staged in LDS as [L][32], one
//                        lane per query (two rounds for L > 64), every lane reads key j at the same LDS address (a
//                        broadcast), online softmax over the keys IN KEY ORDER with a 32-float accumulator in registers.
//                        A wave touches its own sentence only: a result cannot depend on what else is in the launch.
// bert_pool_kernel       one thread per (sentence, channel): the token rows added in token order, divided by L.
//
// What the device arrays hold is never trusted for an address: a sentence whose bounds are not 0 <= start < end <= R
// with end - start <= max_len, an id outside [0, vocab) and a position outside [0, max_pos) set a bit of the caller's
// error word and the rows concerned are not written.
#include "qpg_common.h"

namespace {

constexpr int HD = QPG_BERT_HEAD_DIM;        // 32
constexpr int LMAX = QPG_BERT_MAX_TOKENS;    // 128

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = f_add(v, __shfl_xor(v, o, 64));
  return v;
}

// start and length of sentence s, or false (error bit set) if the device array does not describe rows inside [0, R)
__device__ __forceinline__ bool sentence_rows(const int32_t* __restrict__ seq_start, int s, int64_t R, int max_len, int& a,
                                              int& L, int32_t* __restrict__ err) {
  a = seq_start[s];
  const int b = seq_start[s + 1];
  L = b - a;
  if (a < 0 || b <= a || (int64_t)b > R || L > max_len) {
    if ((threadIdx.x & 63) == 0) atomicOr(err, QPG_BERT_ERR_SEQ);
    return false;
  }
  return true;
}

// ---- embedding gather + LayerNorm, one wave per row
__global__ __launch_bounds__(256) void bert_embed_ln_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ seq_start,
                                                            int S, int64_t R, int max_len, const float* __restrict__ word,
                                                            int vocab, const float* __restrict__ pos, int max_pos,
                                                            const float* __restrict__ type0, const float* __restrict__ g,
                                                            const float* __restrict__ b, int D, float eps,
                                                            float* __restrict__ x, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  // the last s in [0, S) with seq_start[s] <= row (uniform over the wave)
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)seq_start[mid] <= row) lo = mid; else hi = mid - 1;
  }
  const int64_t a = seq_start[lo], e = seq_start[lo + 1];
  if (a > row || e <= row || e - a > max_len) {
    if (lane == 0) atomicOr(err, QPG_BERT_ERR_SEQ);
    return;
  }
  const int p = (int)(row - a);
  const int id = ids[row];
  if (id < 0 || id >= vocab || p >= max_pos) {
    if (lane == 0) atomicOr(err, (id < 0 || id >= vocab) ? QPG_BERT_ERR_ID : QPG_BERT_ERR_POS);
    return;
  }
  const float* wr = word + (int64_t)id * D;
  const float* pr = pos + (int64_t)p * D;
  float s = 0.0f;
  for (int c = lane; c < D; c += 64) s = f_add(s, f_add(f_add(wr[c], type0[c]), pr[c]));
  const float mean = f_div(wave_sum(s), (float)D);
  float v = 0.0f;
  for (int c = lane; c < D; c += 64) {
    const float d = f_sub(f_add(f_add(wr[c], type0[c]), pr[c]), mean);
    v = fmaf(d, d, v);
  }
  const float rstd = f_div(1.0f, f_sqrt(f_add(f_div(wave_sum(v), (float)D), eps)));
  float* xr = x + row * D;
  for (int c = lane; c < D; c += 64)
    xr[c] = f_add(f_mul(f_mul(f_sub(f_add(f_add(wr[c], type0[c]), pr[c]), mean), rstd), g[c]), b[c]);
}

// ---- attention, one wave per (sentence, head); LCAP: the longest sentence the block's LDS holds, WPB waves per block
template <int LCAP, int WPB>
__global__ __launch_bounds__(64 * WPB) void bert_attn_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ seq_start,
                                                             int S, int64_t R, int max_len, int H, float* __restrict__ out,
                                                             int32_t* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) float Ks[WPB][LCAP * HD];
  __shared__ __attribute__((aligned(16))) float Vs[WPB][LCAP * HD];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t pair = (int64_t)blockIdx.x * WPB + w;
  const int s = (int)(pair / H), h = (int)(pair - (int64_t)s * H);
  int a = 0, L = 0;
  const bool live = pair < (int64_t)S * H && sentence_rows(seq_start, s, R, max_len < LCAP ? max_len : LCAP, a, L, err);
  const int D = H * HD;
  const int64_t ld = 3 * (int64_t)D;
  const float* base = qkv + (int64_t)a * ld + h * HD;
  if (live) {
    // K and V rows of this head, 8 float4 per row: lane i of a trip takes float4 i of the [L][32] image
    for (int i = lane; i < L * (HD / 4); i += 64) {
      const int r = i >> 3, c = (i & 7) * 4;
      const float* src = base + (int64_t)r * ld + c;
      *reinterpret_cast<f32x4*>(&Ks[w][r * HD + c]) = *reinterpret_cast<const f32x4*>(src + D);
      *reinterpret_cast<f32x4*>(&Vs[w][r * HD + c]) = *reinterpret_cast<const f32x4*>(src + 2 * D);
    }
  }
  __syncthreads();             // (every wave of the block arrives here once, with or without a sentence)
  if (!live) return;
  for (int q0 = 0; q0 < L; q0 += 64) {
    const int qi = q0 + lane;
    if (qi >= L) continue;
    float q[HD], acc[HD];
    const float* qr = base + (int64_t)qi * ld;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(qr + c);
      q[c] = t.x; q[c + 1] = t.y; q[c + 2] = t.z; q[c + 3] = t.w;
    }
#pragma unroll
    for (int c = 0; c < HD; ++c) acc[c] = 0.0f;
    float m = -INFINITY, l = 0.0f;
    for (int j = 0; j < L; ++j) {
      const float* kj = &Ks[w][j * HD];
      const float* vj = &Vs[w][j * HD];
      float sc = 0.0f;
#pragma unroll
      for (int c = 0; c < HD; ++c) sc = fmaf(q[c], kj[c], sc);
      // online softmax: the running maximum is subtracted, numerator and sum are rescaled when it grows
      const float mn = fmaxf(m, sc);
      const float keep = expf(f_sub(m, mn));          // (first key: exp(-inf) = 0; an unchanged maximum: exactly 1)
      const float pj = expf(f_sub(sc, mn));
      l = f_add(f_mul(l, keep), pj);
#pragma unroll
      for (int c = 0; c < HD; ++c) acc[c] = fmaf(pj, vj[c], f_mul(acc[c], keep));
      m = mn;
    }
    float* o = out + (int64_t)(a + qi) * D + h * HD;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
      f32x4 t;
      t.x = f_div(acc[c], l); t.y = f_div(acc[c + 1], l); t.z = f_div(acc[c + 2], l); t.w = f_div(acc[c + 3], l);
      *reinterpret_cast<f32x4*>(o + c) = t;
    }
  }
}

// ---- mean over a sentence's token rows, in token order
__global__ __launch_bounds__(256) void bert_pool_kernel(const float* __restrict__ x, const int32_t* __restrict__ seq_start,
                                                        int S, int64_t R, int max_len, int D, float* __restrict__ out,
                                                        int32_t* __restrict__ err) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)S * D) return;
  const int s = (int)(e / D), c = (int)(e - (int64_t)s * D);
  const int a = seq_start[s], b = seq_start[s + 1];
  if (a < 0 || b <= a || (int64_t)b > R || b - a > max_len) {
    if (c == 0) atomicOr(err, QPG_BERT_ERR_SEQ);
    return;
  }
  float acc = 0.0f;
  for (int r = a; r < b; ++r) acc = f_add(acc, x[(int64_t)r * D + c]);
  out[e] = f_div(acc, (float)(b - a));
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

#define BERT_UNSUP(cond, ...)       \
  do {                              \
    if (!(cond)) {                  \
      qpg_set_error(__VA_ARGS__);   \
      return QPG_EUNSUP;            \
    }                               \
  } while (0)

// the conditions every entry point puts on the packed layout's sizes
#define BERT_LAYOUT(name)                                                                                             \
  QPG_REQUIRE(seq_start && err, name ": null pointer argument");                                                      \
  QPG_REQUIRE(S >= 1 && R >= S && R <= 0x7fffffffll && max_len >= 1,                                                  \
              name ": need S >= 1 sentences of at least one row, R < 2^31 rows, max_len >= 1 (S %d, R %lld, max_len %d)", \
              S, (long long)R, max_len)

extern "C" int qpg_bert_embed_ln_f32(qpg_ctx* ctx, void* stream, const int32_t* ids, const int32_t* seq_start, int S,
                                     int64_t R, int max_len, const float* word, int vocab, const float* pos, int max_pos,
                                     const float* type0, const float* gamma, const float* beta, int D, float eps, float* x,
                                     int32_t* err) {
  QPG_REQUIRE(ctx, "qpg_bert_embed_ln_f32: null context");
  QPG_REQUIRE(ids && word && pos && type0 && gamma && beta && x, "qpg_bert_embed_ln_f32: null pointer argument");
  BERT_LAYOUT("qpg_bert_embed_ln_f32");
  QPG_REQUIRE(vocab >= 1 && max_pos >= 1 && D >= 1, "qpg_bert_embed_ln_f32: need vocab, max_pos, D >= 1 (%d, %d, %d)", vocab,
              max_pos, D);
  QPG_REQUIRE(max_len <= max_pos, "qpg_bert_embed_ln_f32: sentences of up to %d tokens, the position table has %d rows",
              max_len, max_pos);
  hipLaunchKernelGGL(bert_embed_ln_kernel, dim3(blocks_of(R, 4)), dim3(256), 0, qpg_stream(stream), ids, seq_start, S, R,
                     max_len, word, vocab, pos, max_pos, type0, gamma, beta, D, eps, x, err);
  QPG_LAUNCH_CHECK("bert_embed_ln_kernel");
  return QPG_OK;
}

template <int LCAP, int WPB>
static void launch_attn(hipStream_t st, const float* qkv, const int32_t* seq_start, int S, int64_t R, int max_len, int H,
                        float* out, int32_t* err) {
  hipLaunchKernelGGL((bert_attn_kernel<LCAP, WPB>), dim3(blocks_of((int64_t)S * H, WPB)), dim3(64 * WPB), 0, st, qkv,
                     seq_start, S, R, max_len, H, out, err);
}

extern "C" int qpg_bert_attention_f32(qpg_ctx* ctx, void* stream, const float* qkv, const int32_t* seq_start, int S, int64_t R,
                                      int max_len, int H, float* out, int32_t* err) {
  QPG_REQUIRE(ctx, "qpg_bert_attention_f32: null context");
  QPG_REQUIRE(qkv && out, "qpg_bert_attention_f32: null pointer argument");
  BERT_LAYOUT("qpg_bert_attention_f32");
  QPG_REQUIRE(H >= 1 && H <= 1024 && (int64_t)S * H <= 0x7fffffffll, "qpg_bert_attention_f32: need 1 <= H <= 1024 heads and "
              "S * H < 2^31 (S %d, H %d)", S, H);
  BERT_UNSUP(max_len <= LMAX, "qpg_bert_attention_f32: sentences of up to %d tokens, the kernel takes at most %d", max_len,
             LMAX);
  QPG_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0, "qpg_bert_attention_f32: qkv and out must be 16-byte "
              "aligned");
  // the same arithmetic at every capacity: only the LDS a wave reserves (256 bytes per token) and so the waves a CU holds
  const hipStream_t st = qpg_stream(stream);
  if (max_len <= 16) launch_attn<16, 4>(st, qkv, seq_start, S, R, max_len, H, out, err);
  else if (max_len <= 32) launch_attn<32, 4>(st, qkv, seq_start, S, R, max_len, H, out, err);
  else if (max_len <= 64) launch_attn<64, 4>(st, qkv, seq_start, S, R, max_len, H, out, err);
  else launch_attn<LMAX, 2>(st, qkv, seq_start, S, R, max_len, H, out, err);
  QPG_LAUNCH_CHECK("bert_attn_kernel");
  return QPG_OK;
}

extern "C" int qpg_bert_mean_pool_f32(qpg_ctx* ctx, void* stream, const float* x, const int32_t* seq_start, int S, int64_t R,
                                      int max_len, int D, float* out, int32_t* err) {
  QPG_REQUIRE(ctx, "qpg_bert_mean_pool_f32: null context");
  QPG_REQUIRE(x && out, "qpg_bert_mean_pool_f32: null pointer argument");
  BERT_LAYOUT("qpg_bert_mean_pool_f32");
  QPG_REQUIRE(D >= 1 && (int64_t)S * D <= ((int64_t)1 << 38), "qpg_bert_mean_pool_f32: need D >= 1 and at most 2^38 outputs "
              "(S %d, D %d)", S, D);
  hipLaunchKernelGGL(bert_pool_kernel, dim3(blocks_of((int64_t)S * D, 256)), dim3(256), 0, qpg_stream(stream), x, seq_start,
                     S, R, max_len, D, out, err);
  QPG_LAUNCH_CHECK("bert_pool_kernel");
  return QPG_OK;
}
