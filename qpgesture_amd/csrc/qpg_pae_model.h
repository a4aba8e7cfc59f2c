// The Periodic Auto-Encoder's model math that phase extraction (qpg_pae.hip) and training (qpg_pae_train.hip) both
// state: the MFMA tile geometry of their convolutions and the spectrum head (DeepPhase, codebook/PAE.py:99-145).
// Device inline functions over caller-owned storage; parameter layouts stay with the callers, which pass pointers.
// Every sum here runs in a fixed order, and both callers' tests pin these functions against f64: a change here changes
// the phases written into a gesture database and what training sees together.
#pragma once
#include "qpg_common.h"

namespace pae {

constexpr int TIME = QPG_PAE_TIME;            // 240 window rows = taps = DFT length
constexpr int NB = TIME / 2 + 1;              // rfft bins 0..120
constexpr double TIME_SCALE = 13.0 / 240.0;   // key_range / time_range

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Row tiles of a wave and the q range each one meets: wave w owns the 16-row tiles r0 = 16 (w + 4 j), j = 0..3.
// Source row i = r + q holds position i - pad (zero outside 0 .. Lin-1), so a tile only meets data for
// q in [pad - r0 - 15, pad - r0 + Lin - 1]; the rest of 0 .. nq-1 is padding and skipped.  Tiles at or past the
// row count get an empty range.
struct TileRange {
  int lo[4], hi[4], beg, end;
};

__host__ __device__ constexpr int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }

__host__ __device__ constexpr TileRange tile_ranges(int w, int rows, int nq, int pad, int Lin) {
  TileRange tr{};
  tr.beg = nq;
  tr.end = -1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r0 = 16 * (w + 4 * j);
    tr.lo[j] = imax(0, pad - r0 - 15);
    tr.hi[j] = r0 < rows ? imin(nq - 1, pad - r0 + Lin - 1) : -1;
    if (tr.lo[j] <= tr.hi[j]) {
      tr.beg = imin(tr.beg, tr.lo[j]);
      tr.end = imax(tr.end, tr.hi[j]);
    }
  }
  return tr;
}

// C/D fragment of v_mfma_f32_16x16x4_f32: column = lane & 15, row = 4 (lane >> 4) + register.  The row that
// register g of a lane holds in tile j of wave w:
__device__ __forceinline__ int tile_row(int w, int j, int lane, int g) { return 16 * (w + 4 * j) + 4 * (lane >> 4) + g; }

// ---- the spectrum head of one window: rfft of a latent channel y[240] -> f, a, b; fc (240 -> 2); atan2' / tpi

// tw[2 n], tw[2 n + 1] = cos, sin(2 pi n / 240), by the 256 threads of a block
__device__ __forceinline__ void fill_twiddles(double* tw, int tid) {
  for (int n = tid; n < TIME; n += 256) {
    double sn, cs;
    sincospi((double)n / (double)(TIME / 2), &sn, &cs);
    tw[2 * n] = cs;
    tw[2 * n + 1] = sn;
  }
}

// X_m = sum_u y[u] exp(-2 pi i m u / 240): f64 sums in u order
__device__ __forceinline__ void dft_bin(const float* y, const double* tw, int m, double& re, double& im) {
  re = 0.0;
  im = 0.0;
  int idx = 0;                                // m u mod 240
  for (int u = 0; u < TIME; ++u) {
    const double yu = (double)y[u];
    re = f_add(re, f_mul(yu, tw[2 * idx]));
    im = f_sub(im, f_mul(yu, tw[2 * idx + 1]));
    idx += m;
    if (idx >= TIME) idx -= TIME;
  }
}

__device__ __forceinline__ double bin_power(double re, double im) { return f_add(f_mul(re, re), f_mul(im, im)); }

// sp = sum_m |X_m|^2, sfp = sum_m freqs[m - 1] |X_m|^2 over bins m = 1..120 in order; power(m) = |X_m|^2
template <class Power>
__device__ __forceinline__ void power_sums(const float* freqs, Power power, double& sp, double& sfp) {
  sp = 0.0;
  sfp = 0.0;
  for (int m = 1; m < NB; ++m) {
    const double p = power(m);
    sp = f_add(sp, p);
    sfp = f_add(sfp, f_mul((double)freqs[m - 1], p));
  }
}

// frequency, amplitude and offset of a channel from its power sums and Re X_0, each rounded once
__device__ __forceinline__ void spectrum_fab(double sp, double sfp, double re0, float& f, float& a, float& b) {
  f = (float)f_div(f_div(sfp, sp), TIME_SCALE);
  a = (float)f_div(f_mul(2.0, sqrt(sp)), (double)TIME);
  b = (float)f_div(re0, (double)TIME);
}

// one row of an fc layer: sum_u w[u] y[u] in f64, in u order.  Bias, rounding and BatchNorm stay with the caller
// (folded eval BN in f64 for inference; bias, f32 rounding, then batch BN for training).
__device__ __forceinline__ double fc_dot(const float* w, const float* y) {
  double s = 0.0;
  for (int u = 0; u < TIME; ++u) s = f_add(s, f_mul((double)w[u], (double)y[u]));
  return s;
}

// the model's own atan2 (PAE.py:103-108) over tpi: atan(y / x), +- tpi / 2 where x < 0; NaN at (0, 0), +-pi/2 at x = 0
__device__ __forceinline__ float phase_of(float x, float y, float tpi) {
  float ang = atanf(f_div(y, x));
  if (x < 0.0f && y >= 0.0f) ang = f_add(ang, f_mul(0.5f, tpi));
  if (x < 0.0f && y < 0.0f) ang = f_sub(ang, f_mul(0.5f, tpi));
  return f_div(ang, tpi);
}

}  // namespace pae
