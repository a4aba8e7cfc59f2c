// Audio (WavLM) candidate sweep: float64 cosine distance of every query step against every
// database candidate, on the f64 matrix cores (v_mfma_f64_16x16x4_f64).
//
// Replaces CodeKNN.search_audio_cands(mode='wavlm_feat') (GestureKNN.py:666-691) and the
// feature stacking of data_processing.py:264-268.  A candidate is six frames of the
// interpolated WavLM track, two frames apart; the reference materialises each candidate as a
// 6144-d float64 row (8.85 MB per DB window).  Here candidates are *addressed*, never stored:
// a block gathers its 16 candidates' frames straight from the (N,180,1024) f32 base, so HBM
// traffic is the base array once (frames shared by two neighbouring candidates are re-touched
// within three loop iterations of the same wave and hit L1/L2).
//
// Tiling (gfx950, wave64):
//   block  = 256 threads = 4 waves (one per SIMD) -> 16 consecutive candidates x NT*16 queries
//   wave w = K-slice e in [w*F/4, (w+1)*F/4) of every tap  (split-K over the feature axis)
//   MFMA   A = candidates (row = lane&15, k = lane>>4), B = queries (col = lane&15), f64 acc
//   each lane loads 16 B of its candidate row per (e0, tap) and feeds four MFMA k-steps from it
//   partial sums of the 4 waves are reduced through LDS, turned into distances and stored as
//   128-B runs along the candidate axis of D[q][c].
#include "qpg_common.h"

#include <type_traits>

__global__ __launch_bounds__(1024) void audio_pack_queries_kernel(const float* __restrict__ qbase, int M, int T, int F,
                                                                  const int32_t* __restrict__ q_win,
                                                                  const int32_t* __restrict__ q_t, int n_taps,
                                                                  int tap_stride, float* __restrict__ q32,
                                                                  double* __restrict__ qn2) {
  // one block of 1024 threads per query (this kernel is on the critical path in front of the sweep: 6 iterations
  // per thread instead of 24); 16-B copies when F % 4 == 0; squared norm in f64, fixed reduction order
  const int q = blockIdx.x;
  const int w = q_win[q], t0 = q_t[q];
  const int K = n_taps * F;
  double s = 0.0;
  if ((F & 3) == 0) {
    const int K4 = K >> 2, F4 = F >> 2;
    for (int i = threadIdx.x; i < K4; i += blockDim.x) {
      const int tap = i / F4, e4 = i - tap * F4;
      const int t = t0 + tap * tap_stride;
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (t < T) v = reinterpret_cast<const f32x4*>(qbase + ((int64_t)w * T + t) * F)[e4];
      reinterpret_cast<f32x4*>(q32 + (int64_t)q * K)[i] = v;
      s += (double)v.x * (double)v.x;
      s += (double)v.y * (double)v.y;
      s += (double)v.z * (double)v.z;
      s += (double)v.w * (double)v.w;
    }
  } else {
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
      const int tap = i / F, e = i - tap * F;
      const int t = t0 + tap * tap_stride;
      const float vf = (t < T) ? qbase[((int64_t)w * T + t) * F + e] : 0.f;
      q32[(int64_t)q * K + i] = vf;
      s += (double)vf * (double)vf;
    }
  }
  __shared__ double red[16];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    qn2[q] = t;
  }
}

extern "C" int qpg_audio_pack_queries(qpg_ctx* ctx, void* stream, const float* qbase, int M, int T, int F,
                                      const int32_t* q_win, const int32_t* q_t, int Q, int n_taps, int tap_stride,
                                      float* q32, double* qn2) {
  QPG_REQUIRE(ctx && qbase && q_win && q_t && q32 && qn2 && M > 0 && T > 0 && F > 0 && Q >= 0 && n_taps > 0 &&
                  tap_stride > 0,
              "qpg_audio_pack_queries: bad argument");
  if (Q == 0) return QPG_OK;
  hipLaunchKernelGGL(audio_pack_queries_kernel, dim3(Q), dim3(1024), 0, qpg_stream(stream), qbase, M, T, F, q_win,
                     q_t, n_taps, tap_stride, q32, qn2);
  QPG_LAUNCH_CHECK("audio_pack_queries_kernel");
  return QPG_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// What the three sweeps below share: their arguments, the row of a lane on either side, the padded-tap rule, the
// split-K operand loads, stage issue pattern and reduction, and the epilogue of one (query, candidate) pair.
// ---------------------------------------------------------------------------------------------------------------
constexpr int NTAPS = 6;  // frames of a candidate; the tap schedules of the k loops are written out for six
// Waves of a split-K block (one per SIMD): each takes a quarter of the feature axis.  An 8-wave split (finer work units,
// 6.5 instead of 3.25 rounds of blocks at N_db=2048) measured slower on MI355X: 703 vs 629 us (r01 notes).
constexpr int KS = 4;
constexpr int MPL = 2;    // MFMAs named in front of every load of a split-K stage

template <int S>
struct IC {               // a stage number that a generic lambda can use as a constant
  static constexpr int value = S;
};

struct AudioArgs {
  const void* base;       // [N][T][F] the track: f32, or IEEE f16 in the kernels instantiated with HALF
  int N, T, F;
  const int32_t* cand_t;  // [G] first frame of every candidate of a window
  int G, tap_stride;      // candidate c = window c / G, frames cand_t[c % G] + tap * tap_stride
  const double* cn2;      // [N][G] squared norms of the candidates
  const float* q32;       // [Q][NTAPS * F] the packed queries (audio_pack_queries_kernel)
  const double* qn2;      // [Q] their squared norms
  int Q;
  int d_f32;              // D holds f32 (else f64)
  void* D;                // [Q][ldD] the distances
  int64_t ldD;
  const float* zeros;     // the context's zero page: what a tap at or past T reads
  int32_t* stats;         // the mixed sweeps' flag word ([1] |= 2: operand products may underflow f32); NULL: no flag
  int64_t c_begin, c_end; // candidates [c_begin, c_end) of the N * G
  int main_blocks;        // mx2: blocks past this many are split-K blocks over the candidates [c_end, c_tail_end)
  int64_t c_tail_end;
};

// Wave tile = MT*16 candidates x NT*16 queries.  Per (e0, tap) a lane loads MT + NT float4 (16 B each;
// the query operand is kept in f32 in memory — WavLM values are f32 — and widened in registers) and
// issues 4*MT*NT MFMAs, i.e. (MT+NT)*16 B of L1/L2 traffic per 4*MT*NT*64 matrix-pipe cycles.  At
// MT=1, NT=3 with f64 queries the kernel was L2->L1 bound (37 B/clk/CU, r01 v1 profile: 31 TF);
// MT=2, NT=3 with f32 queries needs 13 B/clk/CU.
// HALF: the base track is stored in f16 (BASELINE.json configs[4] "fp16 features"): one 16-byte load brings the lane's 8
// features, widened f16 -> f32 -> f64 in registers; the arithmetic is the same f64 as for an f32 base, applied to the
// f16-rounded values (so results match the oracle run on the rounded track, not on the original one).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// Candidate c of the launch, clamped to its last one (stores are masked): its first frame and the element offset of
// that frame's features in the track.
struct CandRow {
  int t0;
  int64_t off;
};
__device__ __forceinline__ CandRow cand_row(const AudioArgs& A, int64_t c) {
  if (c >= A.c_end) c = A.c_end - 1;
  const int j = (int)(c / A.G), g = (int)(c - (int64_t)j * A.G);
  const int t0 = A.cand_t[g];
  return {t0, ((int64_t)j * A.T + t0) * A.F};
}

// Packed row of query q, clamped to the last one (stores are masked).
__device__ __forceinline__ const float* query_row(const AudioArgs& A, int q) {
  if (q >= A.Q) q = A.Q - 1;
  return A.q32 + (int64_t)q * (NTAPS * A.F);
}

template <bool HALF>
using track_t = std::conditional_t<HALF, _Float16, float>;

// Where feature e0 of tap `tap` of a candidate row is read from; row + off is the lane's place in the row's first frame t0.
// Taps past the end of the window are zero padding (data_processing.py:266): the load is unconditional (a conditional
// load makes hipcc branch around it and drain vmcnt(0), which serialises the prefetch) and a padded tap reads the
// context's zero page instead of being selected to zero afterwards.
template <typename E>
struct TapSrc {
  const E* p;
  bool in_track;
};
template <typename E>
__device__ __forceinline__ TapSrc<E> tap_src(const AudioArgs& A, const E* row, int64_t off, int t0, int tap, int e0) {
  const bool ok = t0 + tap * A.tap_stride < A.T;
  const E* p = row + off + (int64_t)tap * A.tap_stride * A.F + e0;
  return {ok ? p : reinterpret_cast<const E*>(A.zeros), ok};
}

__device__ __forceinline__ void load8(const float* p, f32x4 (&v)[2]) {
  v[0] = *reinterpret_cast<const f32x4*>(p);
  v[1] = *reinterpret_cast<const f32x4*>(p + 4);
}

// The 8 features from e0 on of tap `tap` of MT candidate rows (element offsets aoff, first frames at0), widened to f32, and
// of NT query rows: one split-K operand buffer each.
template <int MT, bool HALF>
__device__ __forceinline__ void ks_load_cand(const AudioArgs& A, const int64_t (&aoff)[MT], const int (&at0)[MT], int e0,
                                             int tap, f32x4 (&a)[MT][2]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const track_t<HALF>* p = tap_src(A, static_cast<const track_t<HALF>*>(A.base), aoff[mt], at0[mt], tap, e0).p;
    if constexpr (HALF) {      // f16 base: one 16-byte load brings the lane's 8 features
      const f16x8 h = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[mt][0][i] = (float)h[i];
        a[mt][1][i] = (float)h[4 + i];
      }
    } else {
      load8(p, a[mt]);
    }
  }
}
template <int NT>
__device__ __forceinline__ void ks_load_query(const AudioArgs& A, const float* const (&brow)[NT], int e0, int tap,
                                              f32x4 (&b)[NT][2]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) load8(brow[nt] + tap * A.F + e0, b[nt]);
}

// Issue pattern of one (load next group, 8*MT*NT MFMAs of the current group) stage: the (MT+NT)*2 16-B loads are
// spread between the MFMAs — 2 MFMAs, 1 load, ... — instead of being issued as one burst in front of them, so the
// matrix pipe is never left waiting behind a queue of address computations and the loads still lead their use by
// a whole stage.  sched_barrier(0) closes the region.
template <int MT, int NT>
__device__ __forceinline__ void ks_stage_issue() {
#pragma unroll
  for (int sg = 0; sg < (MT + NT) * 2; ++sg) {
    __builtin_amdgcn_sched_group_barrier(0x008, MPL, 0);
    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
  }
  __builtin_amdgcn_sched_group_barrier(0x008, 8 * MT * NT - MPL * 2 * (MT + NT), 0);
  __builtin_amdgcn_sched_barrier(0);
}

// Epilogue of one pair: the distance from the dot product and the two squared norms (a = qn2[q], which the caller may
// hold for several pairs), stored as D says.  Operand products that underflow f32 would break the mixed sweeps' bound:
// |q||c| < 1e-16 raises the flag.  EXACT: the f64 sweep, which has no flag to raise and no f32 form of D.
template <bool EXACT>
__device__ __forceinline__ void store_pair(const AudioArgs& A, int q, int64_t cc, double dot, double a) {
  const double b = A.cn2[cc];
  const double p = a * b;
  if (!EXACT && p > 0.0 && p < 1e-32 && A.stats) atomicOr(&A.stats[1], 2);
  const double dd = cosine_from_dot(dot, a, b);
  if (!EXACT && A.d_f32) static_cast<float*>(A.D)[(int64_t)q * A.ldD + cc] = (float)dd;
  else static_cast<double*>(A.D)[(int64_t)q * A.ldD + cc] = dd;
}

// The partial sums of the KS waves are reduced through LDS, turned into distances and stored.  Output element
// o = ql*(16*MT) + cr (query-local, candidate row): consecutive threads walk the candidate axis, so each query row gets
// one (128*MT)-B store run.  EXACT names the sweep and with it the C/D layout of the sums: lane l, reg r holds query col
// l&15 and candidate row   v_mfma_f64_16x16x4_f64 (EXACT): (l>>4) + 4r        v_mfma_f32_16x16x4_f32: 4*(l>>4) + r
template <int MT, int NT, bool EXACT>
__device__ __forceinline__ void ks_reduce_store(const AudioArgs& A, const double (&red)[KS][MT * NT][4][64], int64_t c0, int q0) {
  __syncthreads();

  constexpr int CR = 16 * MT;
  for (int o = threadIdx.x; o < NT * 16 * CR; o += 64 * KS) {
    const int ql = o / CR, cr = o - ql * CR;
    const int nt = ql >> 4, qc = ql & 15;
    const int mt = cr >> 4, crr = cr & 15;
    const int r = EXACT ? crr >> 2 : crr & 3, l = ((EXACT ? crr & 3 : crr >> 2) << 4) | qc;
    const int t = mt * NT + nt;
    double dot = red[0][t][r][l];
#pragma unroll
    for (int k = 1; k < KS; ++k) dot += red[k][t][r][l];
    const int q = q0 + ql;
    const int64_t cc = c0 + cr;
    if (q < A.Q && cc < A.c_end) store_pair<EXACT>(A, q, cc, dot, A.qn2[q]);
  }
}

// The exact sweep: split-K blocks of MT = 2 tiles throughout, no stats word, f64 matrix.  The LDS-shared-query organisation
// of the mixed sweep for whole rounds of blocks was NOT faster for f64: at 64 cycles per MFMA the split-K kernel is already
// at the matrix pipe's pace (MI355X: 594 vs 590 us at Q = 48, 0.83 vs 0.81 of the roof at Q = 768, 0.79 vs 0.76 ms per step).
template <int NT, bool HALF>
__global__ __launch_bounds__(64 * KS) void audio_cosine_f64_kernel(const AudioArgs A) {
  constexpr int MT = 2;
  __shared__ double red[KS][MT * NT][4][64];  // [wave][tile][acc reg][lane]

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = lane & 15, kq = lane >> 4;
  const int64_t c0 = A.c_begin + (int64_t)blockIdx.x * (16 * MT);
  const int q0 = blockIdx.y * (NT * 16);

  // A side: this lane's candidate row in each of the MT tiles (element offsets into the base track)
  int64_t aoff[MT];
  int at0[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const CandRow cr = cand_row(A, c0 + mt * 16 + row);
    at0[mt] = cr.t0;
    aoff[mt] = cr.off + 8 * kq;
  }
  // B side: this lane's query column in each of the NT tiles
  const float* brow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    brow[nt] = query_row(A, q0 + nt * 16 + row) + 8 * kq;
  }

  f64x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f64x4){0.0, 0.0, 0.0, 0.0};

  // One operand buffer = 8 consecutive features per lane (two 16-B loads: a wave instruction pair
  // consumes whole 128-B lines of 16 rows) for each of the MT candidate and NT query tiles = 8 MFMA
  // k-steps.  Two buffers alternate so the loads of the next (tap, e) group are in flight while the
  // matrix pipe works on the current one (r01 PMC: 31 % of wave time was s_waitcnt before this).
  struct Buf {
    f32x4 a[MT][2], b[NT][2];
  };
  auto load = [&](Buf& u, int e0, int tap) {
    ks_load_cand<MT, HALF>(A, aoff, at0, e0, tap, u.a);
    ks_load_query(A, brow, e0, tap, u.b);
  };
  auto mma = [&](const Buf& u) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double bd[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bd[nt] = (double)u.b[nt][h][i];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const double ad = (double)u.a[mt][h][i];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad, bd[nt], acc[mt][nt], 0, 0, 0);
        }
      }
  };

  const int eBeg = w * (A.F / KS), eEnd = eBeg + (A.F / KS);
  Buf u0, u1;
  load(u0, eBeg, 0);
  auto stage = [&](Buf& next, int e0, int tap, const Buf& cur) {
    load(next, e0, tap);
    mma(cur);
    ks_stage_issue<MT, NT>();
  };
  for (int e0 = eBeg; e0 < eEnd; e0 += 32) {
    stage(u1, e0, 1, u0);
    stage(u0, e0, 2, u1);
    stage(u1, e0, 3, u0);
    stage(u0, e0, 4, u1);
    stage(u1, e0, 5, u0);
    const int en = (e0 + 32 < eEnd) ? e0 + 32 : eBeg;   // last prefetch wraps to a valid address, unused
    stage(u0, en, 0, u1);
  }

#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      red[w][mt * NT + nt][0][lane] = acc[mt][nt].x;
      red[w][mt * NT + nt][1][lane] = acc[mt][nt].y;
      red[w][mt * NT + nt][2][lane] = acc[mt][nt].z;
      red[w][mt * NT + nt][3][lane] = acc[mt][nt].w;
    }
  ks_reduce_store<MT, NT, true>(A, red, c0, q0);
}

// ---------------------------------------------------------------------------------------------------------------
// Mixed-precision sweep (round 2): the same tiling on the f32 matrix cores (v_mfma_f32_16x16x4_f32, twice the f64
// rate), made SAFE for an exact-result pipeline by bounding its error a priori:
//   * one f32 accumulator chain covers ONE stage = 8 MFMAs = 32 products (the chain restarts from C = 0 every
//     stage), and the finished chain is added into an f64 running sum on the VALU while the next stage's MFMAs run;
//   * an f32 FMA chain of n products has |error| <= gamma_n * sum|a_i b_i| <= gamma_n |a||b| (Cauchy-Schwarz), any
//     summation order, gamma_n = n u / (1 - n u), u = 2^-24; the f64 sums add < 1e-13 relative;
//   => |D_mx - D_exact| <= gamma_32 + 1e-13 < 1.92e-6 for every (query, candidate), data independent; + 1.2e-7 when
//      the matrix is stored in f32 (distances <= 2): QPG_AUDIO_MX_ERR = 2.05e-6 of include/qpg.h covers both forms
//      (tests/test_gpu_matching.py measures the actual maximum, ~1e-7).
// qpg_percode_select_mixed_f64 consumes this matrix: every comparison that decides an output (per-code minimum,
// rank order of the minima) and whose operands are closer than 2*QPG_AUDIO_MX_ERR is re-evaluated with an f64 dot
// product first and, when still closer than the near-tie eps, in the reference's own arithmetic.  Operand products
// that underflow f32 would break the bound: a pair with 0 < |q||c| < 1e-16 raises stats[1] |= 2.
// ---------------------------------------------------------------------------------------------------------------
constexpr int MX_OCC = 1;   // waves per SIMD the split-K register allocation is held to
// Both operands go through register rings of depth RING and are requested RING-1 stages (of 8*MT*NT MFMAs = 256*MT*NT
// matrix-pipe cycles) ahead: the candidate rows come from HBM (~2k cycles away under load), the query operand sits in the
// XCD's L2 (the whole query set is 1.2 MB).
template <int MT, int NT, bool HALF>
__device__ __forceinline__ void mx_ksplit_body(const AudioArgs A, const unsigned bx, const unsigned by) {
  constexpr int RING = 2;
  // candidates [c_begin, c_end) of the N*G; block (bx, by) = one tile, KS contraction slices (one wave each), reduced through LDS
  __shared__ double red[KS][MT * NT][4][64];  // [slice][tile][acc reg][lane]

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = lane & 15, kq = lane >> 4;
  const int64_t c0 = A.c_begin + (int64_t)bx * (16 * MT);
  const int q0 = by * (NT * 16);

  int64_t aoff[MT];
  int at0[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const CandRow cr = cand_row(A, c0 + mt * 16 + row);
    at0[mt] = cr.t0;
    aoff[mt] = cr.off + 8 * kq;
  }
  const float* brow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    brow[nt] = query_row(A, q0 + nt * 16 + row) + 8 * kq;
  }

  f64x4 sum[MT][NT];
  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      sum[mt][nt] = (f64x4){0.0, 0.0, 0.0, 0.0};
      acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

  struct BufA {
    f32x4 a[MT][2];
  };
  struct BufB {
    f32x4 b[NT][2];
  };
  auto loadA = [&](BufA& u, int e0, int tap) { ks_load_cand<MT, HALF>(A, aoff, at0, e0, tap, u.a); };
  auto loadB = [&](BufB& u, int e0, int tap) { ks_load_query(A, brow, e0, tap, u.b); };
  // one stage: the finished 32-product chain of every tile goes into its f64 sum, then a fresh chain starts from C = 0
  auto mma = [&](const BufA& ua, const BufB& ub) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            f32x4 cin = acc[mt][nt];
            if (h == 0 && i == 0) {
#pragma unroll
              for (int r = 0; r < 4; ++r) sum[mt][nt][r] += (double)cin[r];
              cin = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ua.a[mt][h][i], ub.b[nt][h][i], cin, 0, 0, 0);
          }
  };

  const int eBeg = w * (A.F / KS);
  const int ne = (A.F / KS) / 32;                       // feature groups of 32 per wave; stage s = (group s/6, tap s%6)
  const int nst = NTAPS * ne;
  // blocks start their walk over the feature groups at different offsets: all blocks read the SAME query rows, and in
  // lockstep they would all hit the same few L2 channels at any moment (only the order of the f64 additions changes)
  const int rot = (int)(bx % (unsigned)ne);
  auto eof = [&](int g) {                               // g in [0, 2*ne)
    g += rot;
    g = g >= ne ? g - ne : g;
    g = g >= ne ? g - ne : g;
    return eBeg + 32 * g;
  };
  BufA ra[RING];
  BufB rb[RING];
#pragma unroll
  for (int d = 0; d < RING - 1; ++d) loadB(rb[d], eof((d / NTAPS) % ne), d % NTAPS);
#pragma unroll
  for (int d = 0; d < RING - 1; ++d) loadA(ra[d], eof((d / NTAPS) % ne), d % NTAPS);
  for (int s0 = 0; s0 < nst; s0 += NTAPS) {
    const int g0 = s0 / NTAPS;
    auto stage = [&](auto jc) {
      constexpr int j = decltype(jc)::value;
      constexpr int jn = j + RING - 1;                  // the stage requested under this one's MFMAs
      int gn = g0 + jn / NTAPS;                         // prefetches past the end wrap to a valid address, unused
      gn = gn >= ne ? gn - ne : gn;
      gn = gn >= ne ? 0 : gn;
      // query loads first: the wait for them at the next stage must not also wait for the (younger, slower) HBM loads
      loadB(rb[jn % RING], eof(gn), jn % NTAPS);
      loadA(ra[jn % RING], eof(gn), jn % NTAPS);
      mma(ra[j % RING], rb[j % RING]);
      ks_stage_issue<MT, NT>();
    };
    stage(IC<0>{}); stage(IC<1>{}); stage(IC<2>{}); stage(IC<3>{}); stage(IC<4>{}); stage(IC<5>{});
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sum[mt][nt][r] += (double)acc[mt][nt][r];
        red[w][mt * NT + nt][r][lane] = sum[mt][nt][r];
      }
  ks_reduce_store<MT, NT, false>(A, red, c0, q0);
}

template <int MT, int NT, bool HALF>
__global__ __launch_bounds__(64 * KS, MX_OCC) void audio_cosine_mx_kernel(const AudioArgs A) {
  mx_ksplit_body<MT, NT, HALF>(A, blockIdx.x, blockIdx.y);
}

// ---------------------------------------------------------------------------------------------------------------
// mx2: the mixed-precision sweep with the QUERY tile shared through LDS.  Measured on MI355X (experiments/audio_mx):
// the split-K organisation above issues 40 row-scattered 16-B/lane loads per CU per 1536 matrix-pipe cycles and is
// bound by the texture-addresser, not by the matrix cores (47 % busy; removing the loads: 262 us instead of 465).
// Here the 4 waves of a block take 16 candidates each and ALL of K; the (48 queries x 64 features) tile of a stage is
// brought in ONCE per block by LDS-DMA (12 coalesced 1-KB pieces, 3 per wave) and read back as MFMA fragments with
// ds_read_b128 (XOR-swizzled at the source so every 16-lane group covers the 16 slots of a bank row); only the
// candidate rows (4 loads per wave-stage) still go global -> VGPR.  One barrier per stage of 48 MFMAs, two LDS
// buffers.  f32 chains are still cut every 32 products (two flushes per stage), so QPG_AUDIO_MX_ERR holds.
// ---------------------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* mx_lds_ptr_t;
constexpr int MX2_OCC = 2;  // waves per SIMD the register allocation is held to
// The 16-byte slot index of a piece inside its 256-byte LDS row is XORed with the row number.  A ds_read_b128 lane group is 16 rows, eight
// of them ({0-3,12-15} or {4-11}) at k-quarter kq and the other eight at kq^1, all reading sub-piece 4*i + kq: with
// slot = piece ^ row both eights land on disjoint slot sets ({4..11} is closed under ^1), i.e. conflict-free.
template <bool HALF>
__global__ __launch_bounds__(256, MX2_OCC) void audio_cosine_mx2_kernel(const AudioArgs A) {
  constexpr int NT = 3;                           // query tiles of a block: 48 queries
  // blocks past `main_blocks` are the split-K remainder (one 16-candidate tile each, candidates from c_end on): they
  // ride in the same launch so that they fill the CUs while the last round of 64-candidate blocks drains
  if (blockIdx.x >= (unsigned)A.main_blocks) {
    AudioArgs tail = A;
    tail.c_begin = A.c_end;
    tail.c_end = A.c_tail_end;
    mx_ksplit_body<1, NT, HALF>(tail, blockIdx.x - (unsigned)A.main_blocks, blockIdx.y);
    return;
  }
  constexpr int ROWB = 256;                       // bytes of one query row per stage (64 features)
  constexpr int STAGE_BYTES = NT * 16 * ROWB;     // 12 KB at NT = 3
  constexpr int PIECES = STAGE_BYTES / 1024;      // 1-KB DMA pieces (4 rows each)
  __shared__ __attribute__((aligned(1024))) unsigned char ring[2][STAGE_BYTES];

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = lane & 15, kq = lane >> 4;
  const int64_t c0 = A.c_begin + ((int64_t)blockIdx.x * 4 + w) * 16;
  const int q0 = blockIdx.y * (NT * 16);

  // candidate row of this lane (clamped; stores are masked)
  const CandRow cr = cand_row(A, c0 + row);
  const int at0 = cr.t0;
  // feature of (load i, k-quarter kq, element e) within a stage = 16*i + 4*kq + e: the four lanes of a row cover 64
  // contiguous bytes per load instruction (16 half lines per instruction; 16*kq + 4*i would touch 32)
  // f16 base (HALF): the lane's 16 features of a stage are two contiguous runs of 8 (one 16-byte load each):
  // feature of (i, kq, e) = 32*(i>>1) + 8*kq + 4*(i&1) + e, and the query fragments follow that order (boff below)
  const int64_t arow_off = cr.off + (HALF ? 8 : 4) * kq;
  const track_t<HALF>* arow = static_cast<const track_t<HALF>*>(A.base) + arow_off;
  // DMA source rows of this lane: piece pi covers tile rows 4*pi .. 4*pi+3, lane l -> row 4*pi + (l>>4), slot l&15
  const float* dsrc[PIECES / 4];
#pragma unroll
  for (int i = 0; i < PIECES / 4; ++i) {
    const int pi = w + 4 * i;
    const int R = 4 * pi + (lane >> 4);
    const int p = (lane & 15) ^ (R & 15);
    dsrc[i] = query_row(A, q0 + R) + 4 * p;
  }
  // fragment read offsets inside a stage buffer: tile nt, k-quarter i -> 16 bytes
  int boff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    boff[i] = row * ROWB + (((HALF ? 8 * (i >> 1) + 2 * kq + (i & 1) : 4 * i + kq) ^ row) << 4);

  f64x4 sum[NT];
  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    sum[nt] = (f64x4){0.0, 0.0, 0.0, 0.0};
    acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const int ng = A.F / 64;                           // feature groups of 64; stage s = (group s / 6, tap s % 6)
  const int nst = NTAPS * ng;
  // The DMA is issued from inline asm so that hipcc's wait-count model does not see it: with an LDS-DMA in the
  // queue the compiler waits vmcnt(0) at the first use of ANY ordinary load, which would drain the candidate
  // prefetches every stage.  Untracked entries only make its counted waits stricter (in-order completion), never
  // looser; the DMA's own completion is awaited explicitly before the stage barrier.
  const unsigned ring_lds = (unsigned)(size_t)(mx_lds_ptr_t)(&ring[0][0]);
  const unsigned w_u = (unsigned)__builtin_amdgcn_readfirstlane(w);
  auto issue_b = [&](int s, int slot) {
    const int tap = s % NTAPS, e0 = 64 * (s / NTAPS);
#pragma unroll
    for (int i = 0; i < PIECES / 4; ++i) {
      const float* gp = dsrc[i] + tap * A.F + e0;
      const unsigned la = ring_lds + (unsigned)slot * STAGE_BYTES + (w_u + 4 * i) * 1024;
      // m0 is the LDS base of the DMA.  Naming it as a clobber makes hipcc warn that it does not preserve reserved
      // registers across the statement - which matters only if the compiler itself keeps something in m0 around here.
      // It does not: in this translation unit m0 occurs nowhere but in these statements (on gfx9+ ordinary LDS, global
      // and MFMA instructions do not read m0), and tests/test_host_cpu.py::test_audio_object_uses_m0_only_in_the_dma_asm
      // holds the built object to that.  (The builtin form hides nothing from the wait-count model: see above.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gp), "s"(la) : "memory", "m0");
#pragma clang diagnostic pop
    }
  };
  auto load_a = [&](f32x4 (&a)[4], int s) {
    const TapSrc<track_t<HALF>> src = tap_src(A, arow, 0, at0, s % NTAPS, 64 * (s / NTAPS));
    if constexpr (HALF) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const f16x8 h = *reinterpret_cast<const f16x8*>(src.p + (src.in_track ? 32 * jj : 0));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[2 * jj][e] = (float)h[e];
          a[2 * jj + 1][e] = (float)h[4 + e];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(src.p + 16 * i);
    }
  };
  // candidate fragments: register ring of depth 3 (prefetched two stages = 96 MFMAs ahead: the rows come from HBM);
  // query tile: LDS double buffer, one stage ahead (L2-resident)
  f32x4 ra[3][4];
  issue_b(0, 0);
  load_a(ra[0], 0);
  load_a(ra[1], 1 % nst);
  for (int s0 = 0; s0 < nst; s0 += 3) {            // unrolled by the ring depth only (taps stay run-time: fewer live addresses)
   auto stage = [&](auto jc) {
    constexpr int jj = decltype(jc)::value;
    const int s = s0 + jj;
    f32x4 (&a)[4] = ra[jj % 3];
    // queue, oldest first: A(s) | DMA(s) x3 | A(s+1) x4 (x2 from an f16 base): the tile of this stage has landed
    // once no more than the A(s+1) loads are outstanding
    if (HALF) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    __builtin_amdgcn_s_barrier();                  // stage s landed for every wave; every wave is done with stage s-1
    __builtin_amdgcn_sched_barrier(0);
    const int sn = s + 1 < nst ? s + 1 : 0;        // (the last prefetches wrap to valid addresses, unused)
    const int sa = s + 2 < nst ? s + 2 : s + 2 - nst;
    issue_b(sn, (s + 1) & 1);
    load_a(ra[(jj + 2) % 3], sa);
    __builtin_amdgcn_sched_barrier(0);             // the prefetches stay in front of the stage's matrix work
    const unsigned char* S = &ring[s & 1][0];
    f32x4 b0[NT][2], b1[NT][2];
    auto read_b = [&](f32x4 (&b)[NT][2], int half) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 2; ++i) b[nt][i] = *reinterpret_cast<const f32x4*>(S + nt * 16 * ROWB + boff[2 * half + i]);
    };
    auto mma_half = [&](const f32x4 (&b)[NT][2], int half) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            f32x4 cin = acc[nt];
            if (i == 0 && e == 0) {   // a 32-product chain is complete: into the f64 sum
#pragma unroll
              for (int r = 0; r < 4; ++r) sum[nt][r] += (double)cin[r];
              cin = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2 * half + i][e], b[nt][i][e], cin, 0, 0, 0);
          }
    };
    read_b(b0, 0);
    __builtin_amdgcn_sched_barrier(0);
    read_b(b1, 1);                                  // the second half's fragments come in under the first half's MFMAs
    mma_half(b0, 0);
#pragma unroll
    for (int sg = 0; sg < NT * 2; ++sg) {
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    mma_half(b1, 1);
#pragma unroll
    for (int sg = 0; sg < 8; ++sg) __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);
    __builtin_amdgcn_sched_barrier(0);
   };
   stage(IC<0>{}); stage(IC<1>{}); stage(IC<2>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the wrapped prefetches
  // C/D layout of v_mfma_f32_16x16x4_f32: lane l, reg r holds (cand row = 4*(l>>4) + r, query col = l&15)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int q = q0 + nt * 16 + row;
    if (q >= A.Q) continue;
    const double a2 = A.qn2[q];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t cc = c0 + (4 * kq + r);
      if (cc >= A.c_end) continue;
      const double dot = sum[nt][r] + (double)acc[nt][r];
      store_pair<false>(A, q, cc, dot, a2);
    }
  }
}

// ---- host: one set of checks, one argument struct, one choice of instantiation --------------------------------------------
static int audio_args(AudioArgs* A, const char* name, qpg_ctx* ctx, const void* base, bool half, int N, int T, int F,
                      const int32_t* cand_t, int G, int n_taps, int tap_stride, const double* cn2, const float* q32,
                      const double* qn2, int Q, void* D, int d_f32, int64_t ldD, int32_t* stats) {
  QPG_REQUIRE(!half || (reinterpret_cast<uintptr_t>(base) % 16) == 0, "%s: base must be 16-byte aligned", name);
  QPG_REQUIRE(ctx && base && cand_t && cn2 && q32 && qn2 && D, "%s: null pointer", name);
  QPG_REQUIRE(N >= 0 && T > 0 && G > 0 && Q >= 0 && tap_stride > 0 && ldD >= (int64_t)N * G, "%s: bad size", name);
  if (n_taps != NTAPS || F <= 0 || (F % 128) != 0) {
    qpg_set_error("%s: compiled for n_taps=6 and F %% 128 == 0 (got n_taps=%d F=%d)", name, n_taps, F);
    return QPG_EUNSUP;
  }
  *A = AudioArgs{};
  A->base = base, A->N = N, A->T = T, A->F = F;
  A->cand_t = cand_t, A->G = G, A->tap_stride = tap_stride, A->cn2 = cn2;
  A->q32 = q32, A->qn2 = qn2, A->Q = Q;
  A->D = D, A->d_f32 = d_f32, A->ldD = ldD;
  A->zeros = ctx->zeros, A->stats = stats;
  A->c_begin = 0, A->c_end = (int64_t)N * G;      // every candidate; audio_cosine_mx() narrows the range per launch
  return QPG_OK;
}

template <typename K>
static int launch_sweep(K kernel, const char* label, void* stream, dim3 grid, const AudioArgs& A) {
  hipLaunchKernelGGL(kernel, grid, dim3(64 * KS), 0, qpg_stream(stream), A);
  QPG_LAUNCH_CHECK(label);
  return QPG_OK;
}
// f(HALF as a constant): the instantiation for an f16 or an f32 track
template <typename Fn>
static int for_track(bool half, Fn f) {
  return half ? f(std::true_type{}) : f(std::false_type{});
}
// f(NT as a constant, query tiles along y): the widest query tile that divides the work without an empty tail (48 queries = 3)
template <typename Fn>
static int for_query_tile(int Q, Fn f) {
  const int qt = (Q + 15) / 16;
  if (qt % 3 == 0) return f(IC<3>{}, qt / 3);
  if (qt % 4 == 0) return f(IC<4>{}, qt / 4);
  if (qt % 2 == 0) return f(IC<2>{}, qt / 2);
  return f(IC<1>{}, qt);
}

// split-K blocks of MT tiles over the candidates [A.c_begin, A.c_end)
template <int MT>
static int launch_audio_mx_q(void* stream, bool half, const AudioArgs& A) {
  return for_query_tile(A.Q, [&](auto nt, int qtiles_y) {
    const dim3 grid((unsigned)((A.c_end - A.c_begin + 16 * MT - 1) / (16 * MT)), (unsigned)qtiles_y);
    return for_track(half, [&](auto h) {
      return launch_sweep(audio_cosine_mx_kernel<MT, decltype(nt)::value, decltype(h)::value>, "audio_cosine_mx_kernel",
                          stream, grid, A);
    });
  });
}

static int audio_cosine_mx(const qpg_ctx* ctx, void* stream, bool half, AudioArgs A) {
  const int64_t C = A.c_end;
  // Work split.  mx2 blocks take 64 candidates x 48 queries; they are all resident at once (5 fit per CU), so the
  // launch is balanced when every CU holds the same number of them: whole multiples of n_cu blocks go to mx2, the
  // remaining candidates to split-K blocks of ONE 16-candidate tile (4 waves share it), which balance to a tile per CU.
  const int ny = (A.Q + 47) / 48;
  const int64_t nbx = C / 64;
  int64_t main_x;
  if (ny >= 4) main_x = nbx;
  else main_x = (nbx * ny / ctx->n_cu) * ctx->n_cu / ny;
  const int64_t c_mid = main_x * 64;
  const int64_t tail_tiles = (C - c_mid + 15) / 16;
  // a short remainder rides in the SAME launch (blocks main_x .. main_x + tail_tiles - 1: split-K, one tile each)
  const bool ride = main_x > 0 && tail_tiles > 0 && tail_tiles <= 4 * (int64_t)ctx->n_cu && ny == 1;
  if (main_x > 0) {
    A.c_end = c_mid;
    A.main_blocks = (int)main_x;
    A.c_tail_end = C;
    const dim3 grid((unsigned)(main_x + (ride ? tail_tiles : 0)), (unsigned)ny);
    const int rc = for_track(half, [&](auto h) {
      return launch_sweep(audio_cosine_mx2_kernel<decltype(h)::value>, "audio_cosine_mx2_kernel", stream, grid, A);
    });
    if (rc != QPG_OK) return rc;
  }
  if (c_mid == C || ride) return QPG_OK;
  A.c_begin = c_mid;
  A.c_end = C;
  if (tail_tiles * ny <= 4 * (int64_t)ctx->n_cu) return launch_audio_mx_q<1>(stream, half, A);
  return launch_audio_mx_q<2>(stream, half, A);
}

static int audio_cosine(void* stream, bool half, const AudioArgs& A) {
  return for_query_tile(A.Q, [&](auto nt, int qtiles_y) {
    const dim3 grid((unsigned)((A.c_end - A.c_begin + 31) / 32), (unsigned)qtiles_y);
    return for_track(half, [&](auto h) {
      return launch_sweep(audio_cosine_f64_kernel<decltype(nt)::value, decltype(h)::value>, "audio_cosine_f64_kernel",
                          stream, grid, A);
    });
  });
}

// the four entry points: mx = the mixed sweep (else the exact one, which writes f64 and has no stats word)
static int audio_sweep(const char* name, bool mx, bool half, qpg_ctx* ctx, void* stream, const void* base, int N, int T,
                       int F, const int32_t* cand_t, int G, int n_taps, int tap_stride, const double* cn2, const float* q32,
                       const double* qn2, int Q, void* D, int d_f32, int64_t ldD, int32_t* stats) {
  AudioArgs A;
  const int rc = audio_args(&A, name, ctx, base, half, N, T, F, cand_t, G, n_taps, tap_stride, cn2, q32, qn2, Q, D, d_f32,
                            ldD, stats);
  if (rc != QPG_OK || N == 0 || Q == 0) return rc;
  return mx ? audio_cosine_mx(ctx, stream, half, A) : audio_cosine(stream, half, A);
}

extern "C" int qpg_audio_cosine_mx(qpg_ctx* ctx, void* stream, const float* base, int N, int T, int F,
                                   const int32_t* cand_t, int G, int n_taps, int tap_stride, const double* cn2,
                                   const float* q32, const double* qn2, int Q, void* D, int d_is_f32, int64_t ldD,
                                   int32_t* stats) {
  return audio_sweep("qpg_audio_cosine_mx", true, false, ctx, stream, base, N, T, F, cand_t, G, n_taps, tap_stride, cn2, q32,
                     qn2, Q, D, d_is_f32, ldD, stats);
}

extern "C" int qpg_audio_cosine_mx_h(qpg_ctx* ctx, void* stream, const void* base_f16, int N, int T, int F,
                                     const int32_t* cand_t, int G, int n_taps, int tap_stride, const double* cn2,
                                     const float* q32, const double* qn2, int Q, void* D, int d_is_f32, int64_t ldD,
                                     int32_t* stats) {
  return audio_sweep("qpg_audio_cosine_mx_h", true, true, ctx, stream, base_f16, N, T, F, cand_t, G, n_taps, tap_stride, cn2,
                     q32, qn2, Q, D, d_is_f32, ldD, stats);
}

extern "C" int qpg_audio_cosine_f64(qpg_ctx* ctx, void* stream, const float* base, int N, int T, int F,
                                    const int32_t* cand_t, int G, int n_taps, int tap_stride, const double* cn2,
                                    const float* q32, const double* qn2, int Q, double* D, int64_t ldD) {
  return audio_sweep("qpg_audio_cosine_f64", false, false, ctx, stream, base, N, T, F, cand_t, G, n_taps, tap_stride, cn2,
                     q32, qn2, Q, D, 0, ldD, nullptr);
}

extern "C" int qpg_audio_cosine_f64_h(qpg_ctx* ctx, void* stream, const void* base_f16, int N, int T, int F,
                                      const int32_t* cand_t, int G, int n_taps, int tap_stride, const double* cn2,
                                      const float* q32, const double* qn2, int Q, double* D, int64_t ldD) {
  return audio_sweep("qpg_audio_cosine_f64_h", false, true, ctx, stream, base_f16, N, T, F, cand_t, G, n_taps, tap_stride,
                     cn2, q32, qn2, Q, D, 0, ldD, nullptr);
}
