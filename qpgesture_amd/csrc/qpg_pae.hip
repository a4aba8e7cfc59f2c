// Phase extraction: the inference half of the Periodic Auto-Encoder (DeepPhase, codebook/PAE.py:477-508 pose2phase and
// Model.forward :99-145 up to `params`), for every frame of many clips in one call.
//
// Frame i of a clip of T frames reads a 240-row window of velocities: row 0 is zero, row s (1..239) is vel[i + s - 121]
// (zero outside 0..T-2), vel = f32(pn[j+1] - pn[j]) with pn = (pose - mean) / std in f64.  Per window:
//   conv1 (135 -> 15, 240 taps, pad 120: 241 positions) -> BN -> tanh -> conv2 (15 -> 8, 240 taps, pad 119: 240) -> BN
//   -> tanh = latent;  rfft of each latent channel -> f, a, b;  fc[k] (240 -> 2) -> BN -> atan2' / 2 pi -> p.
//
// pae_vel_kernel      the velocities of the rows a chunk of frames reads, in f64 and rounded once (bit-identical to the
//                     reference's `.float()`), into the caller's workspace;
// pae_phase_kernel    one block of 4 waves per frame, everything else:
//   1. the frame's window, channel-major, into LDS (zero rows around it: the tiles below read 15 rows past each end);
//   2. conv1 as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32 products): rows = 16 output positions, columns =
//      the 15 (16) output channels, k = (tap, 4 input channels).  The A fragment of tile t0, tap k is a Hankel slice of
//      the window (positions t0 + k - 120 .. +15), read straight from LDS; the B fragment is one float per lane of the
//      host-packed weights [tap][channel group][lane], loaded once per tap and used by all of the wave's 4 tiles.
//      Tap ranges that only meet the zero padding of a tile are skipped: 2 922 (tile, tap) pairs x 34 channel groups =
//      99 348 MFMAs per frame, against 43 199 x 135 x 15 useful MACs (88 %).  Wave w owns tiles w, w+4, w+8, w+12
//      (732, 732, 732, 726 tile-taps: balanced).  Epilogue: (acc + bias) * alpha + beta (eval BN), tanh, into LDS;
//   3. conv2 the same way on the LDS image of conv1's output (15 tiles of 16 positions, k = (tap, 4 channels));
//   4. the spectrum head of qpg_pae_model.h (shared with training): DFT (f64 accumulation), f / a / b, the 8 fc layers
//      (f64 dot products, then the folded eval BN in f64) and atan2'.
// Nothing in a frame's arithmetic depends on the batch, the chunk or the clip offset it comes in (the window is staged
// the same way and every sum runs in a fixed order): results are bit-identical however the frames are grouped.
#include "qpg_pae_model.h"

namespace {

using namespace pae;

constexpr int C_IN = QPG_PAE_CHANNELS;      // 135
constexpr int CG1 = 34;                     // groups of 4 input channels (136)
constexpr int TAPS = QPG_PAE_TIME;          // 240
constexpr int E = QPG_PAE_EMBED;            // 8
constexpr int WS = QPG_PAE_WS_STRIDE;       // 136: floats per velocity row in the workspace
constexpr int LS = 272;                     // LDS row stride (floats) of a channel: 16 mod 32 -> the two 32-lane halves
                                            // of an A read (channel c, c+1) fall on disjoint banks
constexpr int LO = 16;                      // LDS column of window row s is s + LO
constexpr int HALO = QPG_PAE_HALO;          // 120

__device__ __forceinline__ int find_clip(const int64_t* __restrict__ off, int n_clips, int64_t g) {
  int lo = 0, hi = n_clips - 1;             // last c with off[c] <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void pae_vel_kernel(const double* __restrict__ pose, const double* __restrict__ mean,
                                                      const double* __restrict__ stdc, const int64_t* __restrict__ off,
                                                      int n_clips, int64_t n_total, int64_t frame0, int64_t rows,
                                                      float* __restrict__ ws) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * WS) return;
  const int64_t q = e / WS;
  const int ch = (int)(e - q * WS);
  const int64_t G = frame0 - HALO + q;      // velocity row G = pose row G+1 minus pose row G (same clip)
  float v = 0.0f;
  if (ch < C_IN && G >= 0 && G + 1 < n_total) {
    const int c = find_clip(off, n_clips, G);
    if (G + 1 < off[c + 1]) {
      const double a = f_div(f_sub(pose[(G + 1) * C_IN + ch], mean[ch]), stdc[ch]);
      const double b = f_div(f_sub(pose[G * C_IN + ch], mean[ch]), stdc[ch]);
      v = (float)f_sub(a, b);
    }
  }
  ws[e] = v;
}

// pae_phase_kernel writes its tap limits as literals: tile_ranges' general form costs the kernel about 75 scalar
// instructions per block ahead of the tap loop, which showed as 0.3 % of its time.  They are tile_ranges' all the same:
// conv1 is 241 positions x 240 taps over the 239 live window rows 1..239 (row 0 is zero) behind a pad of 121, with no
// empty tile, so its loop runs from the least lo to the greatest hi; conv2 is 240 x 240 over y1's 241 positions behind
// a pad of 119.
constexpr bool tap_limits_are_tile_ranges() {
  for (int w = 0; w < 4; ++w) {
    const TileRange c1 = tile_ranges(w, TAPS + 1, TAPS, HALO + 1, TAPS - 1);
    const TileRange c2 = tile_ranges(w, TAPS, TAPS, HALO - 1, TAPS + 1);
    for (int j = 0; j < 4; ++j) {
      const int t0 = 16 * (w + 4 * j);
      if (c1.lo[j] != imax(0, 106 - t0) || c1.hi[j] != imin(TAPS - 1, 359 - t0) || c1.lo[j] > c1.hi[j]) return false;
      if (c2.lo[j] != imax(0, 104 - t0) || c2.hi[j] != (t0 < TAPS ? imin(TAPS - 1, 359 - t0) : -1)) return false;
    }
  }
  return true;
}
static_assert(tap_limits_are_tile_ranges(), "pae_phase_kernel's literal tap limits no longer match tile_ranges");

__global__ __launch_bounds__(256) void pae_phase_kernel(const float* __restrict__ P, const int64_t* __restrict__ off,
                                                        int n_clips, int64_t frame0, const float* __restrict__ ws,
                                                        float* __restrict__ out, float* __restrict__ v_out,
                                                        float* __restrict__ lat_out) {
  __shared__ __attribute__((aligned(16))) float lds[CG1 * 4 * LS];   // 147 968 B
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, h = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);     // (uniform: the tap-range branches stay scalar)
  const int64_t gl = blockIdx.x;
  const int64_t g = frame0 + gl;
  const int c = find_clip(off, n_clips, g);
  const int64_t c0 = off[c], T = off[c + 1] - c0, i = g - c0;

  // ---- 1. window -> LDS, lds[ch][s + LO] (s = -16 .. 255; zero outside rows 1..239 and outside the clip)
  for (int e = tid; e < CG1 * 4 * LS; e += 256) {
    const int p = e / (CG1 * 4), ch = e - p * (CG1 * 4);
    const int s = p - LO;
    const int64_t j = i + s - (HALO + 1);   // velocity index inside the clip
    float v = 0.0f;
    if (ch < C_IN && s >= 1 && s < TAPS && j >= 0 && j <= T - 2) v = ws[(gl + s - 1) * WS + ch];   // row G - frame0 + HALO
    lds[ch * LS + p] = v;
  }
  __syncthreads();

  // ---- 2. conv1: tile j of wave w covers positions t0 = 16 (w + 4 j) .. +15; lane (r, h) reads position t0 + r at
  // channel 4 cg + h of tap k: window row s = t0 + r + k - 120
  const float* W1 = P + QPG_PAE_OFF_W1;
  f32x4 acc[4];
  int klo[4], khi[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t0 = 16 * (w + 4 * j);
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    klo[j] = max(0, 106 - t0);              // (tap_limits_are_tile_ranges)
    khi[j] = min(TAPS - 1, 359 - t0);
  }
  const int kbeg = min(min(klo[0], klo[1]), min(klo[2], klo[3]));
  const int kend = max(max(khi[0], khi[1]), max(khi[2], khi[3]));
  float bc[CG1], bn[CG1];
#pragma unroll
  for (int q = 0; q < CG1; ++q) bc[q] = W1[(kbeg * CG1 + q) * 64 + lane];
  for (int k = kbeg; k <= kend; ++k) {
    const int kn = k < kend ? k + 1 : k;
#pragma unroll
    for (int q = 0; q < CG1; ++q) bn[q] = W1[(kn * CG1 + q) * 64 + lane];
    const float* arow = lds + h * LS + r + k + LO - HALO;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k >= klo[j] && k <= khi[j]) {
        const float* a = arow + 16 * (w + 4 * j);
#pragma unroll
        for (int q = 0; q < CG1; ++q) acc[j] = mfma4(a[q * 4 * LS], bc[q], acc[j]);
      }
    }
#pragma unroll
    for (int q = 0; q < CG1; ++q) bc[q] = bn[q];
  }
  __syncthreads();                          // the window is dead: LDS is reused below

  // conv1 output y1[o][t + LO] (o < 16, positions -16 .. 255, zero outside 0..240)
  float* y1 = lds;                          // [16][LS]
  float* lat = lds + 16 * LS;               // [8][240]
  double* tw = reinterpret_cast<double*>(lat + E * TAPS);      // [240][2] cos, sin of 2 pi n / 240
  double* pw = tw + 2 * TAPS;               // [8][NB] |X_m|^2 (m >= 1), pw[e][0] = Re X_0
  float* vb = reinterpret_cast<float*>(pw + E * NB);           // [8][2] v
  for (int e = tid; e < 16 * LS; e += 256) y1[e] = 0.0f;
  __syncthreads();
  {
    const float* s1 = P + QPG_PAE_OFF_BN1;
    const float bias = s1[r], alpha = s1[16 + r], beta = s1[32 + r];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int t = tile_row(w, j, lane, g4);                // (the column, lane & 15 = r, is the channel)
        if (t <= TAPS && r < QPG_PAE_MID) y1[r * LS + t + LO] = tanhf(f_add(f_mul(f_add(acc[j][g4], bias), alpha), beta));
      }
    }
  }
  __syncthreads();

  // ---- 3. conv2: tile m = w + 4 j covers u0 = 16 m (tile 15 does not exist: 240 positions); lane reads y1 channel
  // 4 og + h at position u0 + r + k - 119
  {
    const float* W2 = P + QPG_PAE_OFF_W2;
    f32x4 a2[4];
    int lo2[4], hi2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int u0 = 16 * (w + 4 * j);
      a2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      lo2[j] = max(0, 104 - u0);            // (tap_limits_are_tile_ranges)
      hi2[j] = u0 < TAPS ? min(TAPS - 1, 359 - u0) : -1;
    }
    for (int k = 0; k < TAPS; ++k) {
      float b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) b[q] = W2[(k * 4 + q) * 64 + lane];
      const float* arow = y1 + h * LS + r + k + LO - (HALO - 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k >= lo2[j] && k <= hi2[j]) {
          const float* a = arow + 16 * (w + 4 * j);
#pragma unroll
          for (int q = 0; q < 4; ++q) a2[j] = mfma4(a[q * 4 * LS], b[q], a2[j]);
        }
      }
    }
    const float* s2 = P + QPG_PAE_OFF_BN2;
    const float bias = s2[r], alpha = s2[16 + r], beta = s2[32 + r];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int u = tile_row(w, j, lane, g4);
        if (u < TAPS && r < E) lat[r * TAPS + u] = tanhf(f_add(f_mul(f_add(a2[j][g4], bias), alpha), beta));
      }
    }
  }
  fill_twiddles(tw, tid);
  __syncthreads();

  // ---- 4. DFT of each latent channel (bins 0..120)
  for (int task = tid; task < E * NB; task += 256) {
    const int e = task / NB, m = task - e * NB;
    double re, im;
    dft_bin(lat + e * TAPS, tw, m, re, im);
    pw[task] = m == 0 ? re : bin_power(re, im);
  }
  // the 8 fc layers: v[e][j] = BN(fc_e(latent_e))_j (eval BN folded, in f64; rounded to f32 like the reference's tensor)
  if (tid < 2 * E) {
    const int o = tid, e = o >> 1;
    const double s = fc_dot(P + QPG_PAE_OFF_FC + o * TAPS, lat + e * TAPS);
    const float* fb = P + QPG_PAE_OFF_FCBN;
    vb[o] = (float)f_add(f_mul(f_add(s, (double)fb[o]), (double)fb[16 + o]), (double)fb[32 + o]);
  }
  __syncthreads();

  if (tid < E) {
    const int e = tid;
    double sp, sfp;
    power_sums(P + QPG_PAE_OFF_FREQ, [&](int m) { return pw[e * NB + m]; }, sp, sfp);
    float* o = out + gl * (4 * E);
    spectrum_fab(sp, sfp, pw[e * NB], o[E + e], o[2 * E + e], o[3 * E + e]);
    const float x = vb[2 * e], y = vb[2 * e + 1];
    o[e] = phase_of(x, y, P[QPG_PAE_OFF_TPI]);
    if (v_out) {
      v_out[gl * 2 * E + 2 * e] = x;
      v_out[gl * 2 * E + 2 * e + 1] = y;
    }
  }
  if (lat_out)
    for (int e = tid; e < E * TAPS; e += 256) lat_out[gl * E * TAPS + e] = lat[e];
}

}  // namespace

extern "C" int qpg_pae_phase_f32(qpg_ctx* ctx, void* stream, const float* params, const double* pose, const double* mean,
                                 const double* stdc, const int64_t* clip_off, int n_clips, int64_t n_total, int64_t frame0,
                                 int64_t n_frames, float* ws, int64_t ws_floats, float* out, float* v_out,
                                 float* latent_out) {
  QPG_REQUIRE(ctx, "qpg_pae_phase_f32: null context");
  QPG_REQUIRE(params && pose && mean && stdc && clip_off && ws && out, "qpg_pae_phase_f32: null pointer argument");
  QPG_REQUIRE(n_clips >= 1 && n_total >= 1 && n_total <= ((int64_t)1 << 40),
              "qpg_pae_phase_f32: need 1 <= n_clips and 1 <= n_total <= 2^40 (n_clips %d, n_total %lld)", n_clips,
              (long long)n_total);
  QPG_REQUIRE(frame0 >= 0 && n_frames >= 0 && n_frames <= QPG_PAE_MAX_CHUNK && frame0 <= n_total - n_frames,
              "qpg_pae_phase_f32: frames [%lld, +%lld) outside 0..%lld or more than %d per call", (long long)frame0,
              (long long)n_frames, (long long)n_total, QPG_PAE_MAX_CHUNK);
  QPG_REQUIRE(ws_floats >= (n_frames + 2 * HALO - 1) * (int64_t)WS,
              "qpg_pae_phase_f32: workspace of %lld floats, %lld needed", (long long)ws_floats,
              (long long)((n_frames + 2 * HALO - 1) * (int64_t)WS));
  if (n_frames == 0) return QPG_OK;
  const int64_t rows = n_frames + 2 * HALO - 1;
  const int64_t nv = rows * WS;
  hipLaunchKernelGGL(pae_vel_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, qpg_stream(stream), pose, mean,
                     stdc, clip_off, n_clips, n_total, frame0, rows, ws);
  QPG_LAUNCH_CHECK("pae_vel_kernel");
  hipLaunchKernelGGL(pae_phase_kernel, dim3((unsigned)n_frames), dim3(256), 0, qpg_stream(stream), params, clip_off,
                     n_clips, frame0, ws, out, v_out, latent_out);
  QPG_LAUNCH_CHECK("pae_phase_kernel");
  return QPG_OK;
}
