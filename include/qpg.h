/*
 * qpg.h — C ABI of libqpg_hip.so: the MI355X (gfx950) implementation of QPGesture's
 * code-level motion-matching hot path (CodeKNN) and gesture VQ-VAE encode/quantise/decode.
 *
 * The reference (YoungSeng/QPGesture) is pure Python and has no FFI layer; each entry point
 * below names the reference interface it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer marked [dev] is a device pointer owned by the caller (the Python host keeps
 *     torch tensors alive); the library never allocates or frees caller-visible memory;
 *   - all work is enqueued on the hipStream_t passed as `void* stream` (0 = null stream) and
 *     is stream-ordered; no call synchronises the device;
 *   - every function returns QPG_OK (0) or a negative QPG_E* code and never throws;
 *     qpg_last_error() returns the text of the last failure on the calling thread;
 *   - no global mutable state except the per-device qpg_ctx.
 *   - tie rule everywhere: lowest index wins (== the reference's strict `<` first-wins scan,
 *     GestureKNN.py:686,717) and ranks are stable (documented deviation from NumPy's unstable
 *     default argsort, DESIGN.md "Tie contract").
 */
#ifndef QPG_H
#define QPG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPG_OK 0
#define QPG_EINVAL (-1)   /* bad argument (null pointer, size out of range)          */
#define QPG_EHIP (-2)     /* a HIP runtime call or kernel launch failed               */
#define QPG_EUNSUP (-3)   /* shape not supported by the compiled kernels              */

typedef struct qpg_ctx qpg_ctx;

int qpg_version(void);
/* First 16 hex digits of the SHA-256 over the sources the library was compiled from (every .hip and .h file of csrc/
 * in name order, then include/qpg.h: qpgesture_amd/build.py:source_hash()); "unstamped" for a build that bypassed build.py.  The Python binding
 * refuses to run a library whose id differs from the tree it sits in (it rebuilds it). */
const char* qpg_build_id(void);
/* One context per device, created by the host thread that drives that device.
 * PERFORMANCE NOTE for direct callers: the matcher is a chain of a dozen short dependent launches per clip, and the HIP
 * runtime hands their arguments to the command processor through device memory only when the environment variable
 * HIP_FORCE_DEV_KERNARG=1 is set BEFORE the process's first HIP call (the Python package sets it at import; measured
 * ~5 % of a clip, 0.347 -> 0.330 ms).  qpg_dev_kernarg() reports what this process will get: 1 = set, 0 = not set. */
int qpg_ctx_create(int device, qpg_ctx** out);
int qpg_dev_kernarg(void);
int qpg_ctx_destroy(qpg_ctx* ctx);
/* Per-context knobs (the library holds no other mutable state; a knob of one context never affects another):
 *   QPG_OPT_GATE_DEDUP_FROM_CHAINS  from how many chains per qpg_match_steps(_batch) launch the phase-gate table is
 *                                   deduplicated by the previous winner (default 1 = always; 0 = never: round 4's plain
 *                                   table, bit-identical results - the tests walk on both). */
#define QPG_OPT_GATE_DEDUP_FROM_CHAINS 0
/*   QPG_OPT_TAKES_STAGES            which of qpg_match_steps_takes' own kernels a call launches: bit 0 = step 0 of every
 *                                   take, bit 1 = the chase, bit 2 = the epilogue (default 7 = all).  Measurement only
 *                                   (tools/bench_takes.py times each kernel between two HIP events): a stage that is
 *                                   left out reads what an earlier full call left in the same workspace. */
#define QPG_OPT_TAKES_STAGES 1
/*   QPG_OPT_NOPHASE_STAGES          which of qpg_match_steps_nophase's two kernels a call launches: bit 0 = the tables, bit
 *                                   1 = the chase (default 3 = both).  Measurement only (tools/bench_nophase.py times each
 *                                   between two HIP events): a chase alone follows the tables an earlier full call left in
 *                                   the same workspace. */
#define QPG_OPT_NOPHASE_STAGES 2
#define QPG_OPT_COUNT 4
int qpg_ctx_set_option(qpg_ctx* ctx, int option, int value);
int qpg_ctx_get_option(qpg_ctx* ctx, int option, int* value);
int qpg_last_error(char* buf, size_t n);
/* Stream-ordered signal to the host: *dst = value (system-scope store by a one-thread kernel) once everything enqueued on
 * `stream` before this call has completed.  dst: [host-pinned, device-accessible or dev] i32.  The multi-lane replay
 * pipeline (qpgesture_amd.code_knn.GraphPipeline) polls it to learn that a replay's sweep is over. */
int qpg_signal_i32(qpg_ctx*, void* stream, int32_t* dst, int32_t value);
/* The doorbell of a pre-launched graph replay: a one-thread kernel that takes its sequence number seq = ++*counter
 * (counter: [dev] i32, zero-initialised by the caller, one per captured graph) and waits until *go - seq >= 0 (go:
 * [host-pinned, device-accessible] i32 the host stores to), at most timeout_ms (1..60000; a host that never rings cannot hang
 * the device).  As the FIRST node of a captured matching step it lets the host enqueue the next replay - hipGraphLaunch is
 * ~17 us of host time - while the current one still runs, and start it by a single store once the current results are read
 * and the next seeds written (qpgesture_amd.code_knn.ClipGraph(doorbell=True)). */
int qpg_doorbell_wait(qpg_ctx*, void* stream, int32_t* counter, const int32_t* go, int32_t timeout_ms);

/* ------------------------------------------------------------------------------------------
 * Database preparation (one-off per speaker DB; replaces the host-side feature windowing of
 * codebook/Speech2GestureMatching/data_processing.py:255-274, which materialises an
 * (N,180,6144) float64 stack — here nothing is materialised, only per-candidate norms).
 * ---------------------------------------------------------------------------------------- */

/* WavLM track resampling Tin -> Tout frames: F.interpolate(mode='linear', align_corners=True) in f32, bit-exact
 * with torch's CPU kernel (data_processing.py:258-261: 199 -> 180).  x: [dev] f32 [N][Tin][F]; out: [dev] f32 [N][Tout][F]. */
int qpg_wavlm_resample_f32(qpg_ctx*, void* stream, const float* x, int64_t N, int Tin, int F, int Tout, float* out);

/* out[r] = sum_e x[r][e]^2 in float64, r < rows.  x: [dev] f32 [rows][F]. */
int qpg_frame_norm2_f64(qpg_ctx*, void* stream, const float* x, int64_t rows, int F, double* out);

/* cn2[j][g] = sum_{i<n_taps} fn2[j][cand_t[g] + i*tap_stride]  (0 past T).
 * fn2: [dev] f64 [N][T]; cand_t: [dev] i32 [G]; cn2: [dev] f64 [N][G]. */
int qpg_audio_cand_norm2(qpg_ctx*, void* stream, const double* fn2, int N, int T, const int32_t* cand_t,
                         int G, int n_taps, int tap_stride, double* cn2);

/* Row-wise L2 normalisation with scikit-learn's float32 arithmetic, bit-exact
 * (sklearn.preprocessing.normalize as used by paired_cosine_distances; zero rows stay zero).
 * x, out: [dev] f32 [rows][D]. */
int qpg_l2_normalize_rows_f32(qpg_ctx*, void* stream, const float* x, int64_t rows, int D, float* out);
/* The text queries of a clip, gathered and normalised in one launch: out[r] = normalise(x[q_win[r]][q_row[r]][:])
 * (clip_context[int(i / n_db_frm * 30)] of window q_win[r], GestureKNN.py:549-551).  x: [dev] f32 [M][R][D];
 * q_win, q_row: [dev] i32 [Q] (caller guarantees 0 <= q_win < M, 0 <= q_row < R); out: [dev] f32 [Q][D]. */
int qpg_text_pack_queries_f32(qpg_ctx*, void* stream, const float* x, int M, int R, int D, const int32_t* q_win,
                              const int32_t* q_row, int Q, float* out);

/* ------------------------------------------------------------------------------------------
 * Candidate sweeps.  Replace CodeKNN.search_audio_cands(mode='wavlm_feat') and
 * CodeKNN.search_text_cands (GestureKNN.py:666-691, 708-721) for ALL Q query steps of a clip
 * at once: the scans depend only on the query position, never on the matching state.
 * Candidate index c = j*G + g (j = DB window, g = grid position) = the reference's scan order.
 * ---------------------------------------------------------------------------------------- */

/* Gather the audio queries of a clip into contiguous rows (values stay f32: WavLM features are f32
 * in the reference too, only the arithmetic is f64) and compute their squared norms in f64.
 * qbase: [dev] f32 [M][T][F] (interpolated WavLM of the test windows);
 * q_win/q_t: [dev] i32 [Q] window and start frame of each query (GestureKNN.py:565: clip_test[i]);
 * q32: [dev] f32 [Q][n_taps*F] out; qn2: [dev] f64 [Q] out (squared norms). */
int qpg_audio_pack_queries(qpg_ctx*, void* stream, const float* qbase, int M, int T, int F,
                           const int32_t* q_win, const int32_t* q_t, int Q, int n_taps, int tap_stride,
                           float* q32, double* qn2);

/* Cosine distance of every query against every audio candidate, float64 arithmetic
 * (the reference computes this distance in float64: data_processing.py:264, sklearn keeps f64):
 *   D[q][c] = 1 - <q, cand_c> / (|q| |cand_c|),  cand_c = concat_i base[j][cand_t[g] + i*tap_stride][:]
 * (== 0.5*|q/|q| - c/|c||^2 of sklearn.metrics.pairwise.paired_cosine_distances up to f64 rounding;
 * zero-norm rows follow sklearn: they stay zero vectors).
 * base: [dev] f32 [N][T][F]; cn2: [dev] f64 [N][G]; D: [dev] f64 [Q][N*G], row stride ldD elements. */
int qpg_audio_cosine_f64(qpg_ctx*, void* stream, const float* base, int N, int T, int F,
                         const int32_t* cand_t, int G, int n_taps, int tap_stride, const double* cn2,
                         const float* q32, const double* qn2, int Q, double* D, int64_t ldD);
/* The same sweep over a base track stored in IEEE f16 (BASELINE.json configs[4] "fp16 features": half the HBM bytes of
 * the dominant array).  Values are widened f16 -> f32 -> f64 in registers and the arithmetic is the same f64 as above,
 * i.e. the result is the reference's distance on the f16-ROUNDED track (cn2 must be computed from the rounded values
 * too).  base_f16: [dev] f16 [N][T][F], 16-byte aligned. */
int qpg_audio_cosine_f64_h(qpg_ctx*, void* stream, const void* base_f16, int N, int T, int F,
                           const int32_t* cand_t, int G, int n_taps, int tap_stride, const double* cn2,
                           const float* q32, const double* qn2, int Q, double* D, int64_t ldD);

/* MIXED-PRECISION form of qpg_audio_cosine_f64 (round 2; the default path of CodeKNN.sweep_audio): the same sweep on
 * the f32 matrix cores, with every f32 accumulation chain limited to 32 products and summed in f64, which bounds the
 * result's error A PRIORI: |D[q][c] - exact| <= QPG_AUDIO_MX_ERR for every pair, whatever the data (gamma_32 = 1.91e-6
 * for the f32 chains + 1.2e-7 for an f32-stored matrix + f64 noise; derivation: qpgesture_amd/csrc/qpg_audio.hip).
 * Meant to be consumed by qpg_percode_select_mixed_f64 (and, across row shards, qpg_merge_mixed_*), which re-evaluate
 * every comparison the bound leaves undecided, so the selected candidates and ranks are those of the f64 path.  stats: [dev] i32 [4] (may be NULL): [1] |= 2 if a pair with 0 < |q||c| < 1e-16 was met (operand products
 * could underflow f32, which the bound excludes). */
#define QPG_AUDIO_MX_ERR 2.05e-6
int qpg_audio_cosine_mx(qpg_ctx*, void* stream, const float* base, int N, int T, int F, const int32_t* cand_t, int G,
                        int n_taps, int tap_stride, const double* cn2, const float* q32, const double* qn2, int Q,
                        void* D, int d_is_f32, int64_t ldD, int32_t* stats);
/* D: [dev] [Q][N*G] with row stride ldD ELEMENTS, f64 — or f32 when d_is_f32 != 0: the matrix only feeds the select's
 * two streaming passes, and rounding it to f32 (<= 1.2e-7 on a distance <= 2) is part of QPG_AUDIO_MX_ERR. */

/* qpg_audio_cosine_mx over a base track stored in IEEE f16 (as qpg_audio_cosine_f64_h): same bound, on the rounded values. */
int qpg_audio_cosine_mx_h(qpg_ctx*, void* stream, const void* base_f16, int N, int T, int F, const int32_t* cand_t, int G,
                          int n_taps, int tap_stride, const double* cn2, const float* q32, const double* qn2, int Q,
                          void* D, int d_is_f32, int64_t ldD, int32_t* stats);

/* SPLIT-OPERAND f16 form of the mixed-precision sweep (round 3; the default audio sweep where the grid allows it):
 * same contract as qpg_audio_cosine_mx with a tighter a-priori bound (|D - exact| <= QPG_AUDIO_HL_ERR for every pair,
 * consumed by qpg_percode_select_mixed_f64 with eps1 >= 2 x that), with the products on the f16 matrix cores: every value is scaled by a power
 * of two and stored as two f16 numbers (h, l) with x = h + 2^-11 l (+ <= 2^-23 |x|), the h h' block sums of every MFMA
 * are added in f64, the cross terms run as f32 chains, and the database is read in a frame-major image in which every
 * frame occurs ONCE (super-rows of three frames: dot(q, cand g) = S[g][q first 3 taps] + S[g+1][q last 3 taps]) — the
 * sweep is HBM-bound.  Derivation of the bound and layouts: qpgesture_amd/csrc/qpg_audio_hl.hip.
 *   qpg_audio_hl_supported   1 if the candidate grid has the required shape: 6 taps, G = 26 grid positions
 *                            `cand_step` = 3 x tap_stride frames apart, F %% 128 == 0 (the reference's WavLM grid,
 *                            data_processing.py:264-268 / GestureKNN.py:672-690); else use qpg_audio_cosine_mx.
 *   qpg_audio_hl_pack_db     one-off: base [dev] f32 [N][T][F] -> image [dev] (qpg_audio_hl_db_bytes(N, F) bytes, 16-byte
 *                            aligned): per window [tile 0: k-block][plane][64 units][8 f16] then [tile 1: k-block][plane]
 *                            [44 units][8 f16] (its 11 live rows only: every byte of the image is read) + scale exponent.
 *   qpg_audio_hl_pack_queries per clip: q32 [dev] f32 [Q][6 F] (qpg_audio_pack_queries) -> image [dev]
 *                            (qpg_audio_hl_query_bytes(Q, F) bytes): chunks of 48 queries + one scale exponent per query.
 *   qpg_audio_cosine_hl      D [dev] [Q][N*G] (f32 if d_is_f32, else f64; row stride ldD elements).  cn2 [dev] f64 [N][G],
 *                            qn2 [dev] f64 [Q]: the UNSCALED squared norms (qpg_audio_cand_norm2 / qpg_audio_pack_queries).
 *                            stats[1] |= 2 if a non-zero operand's SCALED squared norm is < 2^16 (a database row whose
 *                            norm is below 1/64 .. 1/128 of the largest magnitude in the whole track: outside the range
 *                            the representation bound covers - the l planes' f16 subnormals; round 5, was < 1). */
#define QPG_AUDIO_HL_ERR 1.3e-6 /* a-priori bound of qpg_audio_cosine_hl: |D - exact| <= this for every pair in range */
int qpg_audio_hl_supported(int T, int F, int G, int n_taps, int tap_stride, int cand_step);
/* qpg_audio_pack_queries + qpg_audio_hl_pack_queries in ONE launch (the pair sits on a clip's critical path): gathers the
 * queries from qbase [dev] f32 [M][T][F] like qpg_audio_pack_queries (q32, qn2 are still written: the select's
 * re-evaluations read them) and writes the split-f16 image.  6 taps, F %% 32 == 0, F <= 2048. */
int qpg_audio_pack_queries_hl(qpg_ctx*, void* stream, const float* qbase, int M, int T, int F, const int32_t* q_win,
                              const int32_t* q_t, int Q, int n_taps, int tap_stride, float* q32, double* qn2, void* image,
                              int64_t image_bytes);
int64_t qpg_audio_hl_db_bytes(int N, int F);
int64_t qpg_audio_hl_query_bytes(int Q, int F);
int qpg_audio_hl_pack_db(qpg_ctx*, void* stream, const float* base, int N, int T, int F, int G, int n_taps, int tap_stride,
                         int cand_step, void* image, int64_t image_bytes);
int qpg_audio_hl_pack_queries(qpg_ctx*, void* stream, const float* q32, int Q, int F, void* image, int64_t image_bytes);
/* Round 4: a clip's WHOLE query side in one launch - qpg_audio_pack_queries_hl's work and the text side's query pack
 * (qpg_text_pack_queries_f32 + qpg_hl_pack_cols, bit-identical outputs): text_ctx [dev] f32 [Mt][R][Dt], tq_win / tq_row
 * [dev] i32 [Qt], qn_out [dev] f32 [Qt][Dt], cols_image [dev] qpg_hl_cols_bytes(Qt, Dt) bytes.  Dt %% 128 == 0. */
int qpg_clip_pack_hl(qpg_ctx*, void* stream, const float* qbase, int M, int T, int F, const int32_t* q_win,
                     const int32_t* q_t, int Q, int n_taps, int tap_stride, float* q32, double* qn2, void* image,
                     int64_t image_bytes, const float* text_ctx, int Mt, int R, int Dt, const int32_t* tq_win,
                     const int32_t* tq_row, int Qt, float* qn_out, void* cols_image, int64_t cols_bytes);
int qpg_audio_cosine_hl(qpg_ctx*, void* stream, const void* db_image, int N, int F, int G, const double* cn2,
                        const void* q_image, const double* qn2, int Q, void* D, int d_is_f32, int64_t ldD, int32_t* stats);
/* The same sweep over a track stored in IEEE f16 (round 5; BASELINE.json configs[4] "fp16 features"): an f16 value is
 * its own h plane, so the database image has ONE plane, no scale exponent and no representation error - half the bytes
 * (N x 27 rows x 3 F f16, every byte read once) and two products per element (h h', l' h) instead of three.  Same query
 * image (qpg_audio_pack_queries_hl / qpg_clip_pack_hl), same D, same bound QPG_AUDIO_HL_ERR on the ROUNDED track's exact
 * distances (cn2 = its candidates' squared norms), same select.  Reference data path: data_processing.py:255-274 (the
 * track), GestureKNN.py:666-691 (the scan).
 *   qpg_audio_hl1_supported  qpg_audio_hl_supported's grid and 3 F / 32 a multiple of 12 (F %% 128 == 0).
 *   qpg_audio_hl1_pack_db    one-off: base_f16 [dev] f16 [N][T][F] -> image [dev] (qpg_audio_hl1_db_bytes(N, F) bytes). */
int qpg_audio_hl1_supported(int T, int F, int G, int n_taps, int tap_stride, int cand_step);
int64_t qpg_audio_hl1_db_bytes(int N, int F);
int qpg_audio_hl1_pack_db(qpg_ctx*, void* stream, const void* base_f16, int N, int T, int F, int G, int n_taps,
                          int tap_stride, int cand_step, void* image, int64_t image_bytes);
int qpg_audio_cosine_hl1(qpg_ctx*, void* stream, const void* db_image, int N, int F, int G, const double* cn2,
                         const void* q_image, const double* qn2, int Q, void* D, int d_is_f32, int64_t ldD, int32_t* stats);
/* Hardware probe behind the bound's one measured constant: out[tile] = A[tile] (16 x 32 f16) . B[tile]^T (16 x 32 f16)
 * + C[tile] (16 x 16 f32, NULL = 0) exactly as ONE v_mfma_f32_16x16x32_f16 computes it; the tests compare it with exact
 * sums (kappa: error of a 32-product block sum in units of 2^-24 sum |products|). */
int qpg_probe_mfma_f16_tile(qpg_ctx*, void* stream, const void* a, const void* b, const float* c, int tiles, float* out);

/* One-off DB preparation for the text sweep: sklearn-normalise the grid rows x[j][cand_r[g]] (bit-exact,
 * as qpg_l2_normalize_rows_f32) and store them tiled for lane-per-candidate access:
 *   xt[c/64][e/4][c%64][e%4],  c = j*G + g   (a wave's 64 lanes read 64 consecutive 16-B pieces).
 * x: [dev] f32 [N][R][Dm]; xt: [dev] f32 [ceil(N*G/64)*64 * Dm]. */
int qpg_text_pack_candidates_f32(qpg_ctx*, void* stream, const float* x, int N, int R, int Dm,
                                 const int32_t* cand_r, int G, float* xt);

/* Cosine distance with scikit-learn's float32 arithmetic, bit-exact (GestureKNN.py:716 keeps f32):
 *   D[q][c] = 0.5 * einsum_sq(qn[q] - xn_c)     (NumPy einsum summation order)
 * xt: tiled normalised candidates from qpg_text_pack_candidates_f32 (C = N*G of them);
 * qn: [dev] f32 [Q][Dm] queries normalised by qpg_l2_normalize_rows_f32; D: [dev] f32 [Q][C]. */
int qpg_text_cosine_f32(qpg_ctx*, void* stream, const float* xt, int64_t C, int Dm, const float* qn, int Q,
                        float* D, int64_t ldD);

/* The same sweep with the per-code minimum FUSED into it (large query counts, BASELINE.json configs[2]: 1 000 queries x
 * 100 000 candidates): the Q x C distance matrix never reaches HBM.  Distances are bit-identical to
 * qpg_text_cosine_f32's; winner per (query, code) = minimum distance, lowest candidate index among equals.
 * cand_code: [dev] i16 [C] code of candidate c (outside [0,K): skipped, e.g. masked rows); tiles_per_chunk: 64-candidate
 * tiles per block (work granularity); `ws`: scratch of `qpg_text_percode_ws_bytes` bytes (one packed [Q][K] table; contents on entry are ignored);
 * out_dist [dev] f32 [Q][K] (`absent` where a code has no candidate), out_idx [dev] i32 [Q][K] = c + idx_base or -1,
 * out_rank optional [dev] i16 [Q][K] stable ranks; out_nn optional [dev] i32 [Q] the query's global nearest
 * neighbour over all codes (candidate index, -1 if there is no valid candidate).  K <= 1024. */
int64_t qpg_text_percode_ws_bytes(int64_t C, int Q, int K, int tiles_per_chunk);
int qpg_text_percode_f32(qpg_ctx*, void* stream, const float* xt, int64_t C, int Dm, const int16_t* cand_code, int K,
                         const float* qn, int Q, int tiles_per_chunk, int32_t idx_base, float absent, void* ws,
                         int64_t ws_bytes, float* out_dist, int32_t* out_idx, int16_t* out_rank, int32_t* out_nn);
/* fp16-STORAGE variant of the pair above (BASELINE.json "fp16 features"): qpg_text_pack_candidates_f16 stores the grid
 * rows ROUNDED to IEEE f16 (xh: [dev] f16, ceil(N*G/64)*64*Dm elements, tiled [c/64][e/8][c%64][e%8], 16-byte aligned)
 * and their sklearn norms computed from the rounded values (nrm: [dev] f32 [N*G]); qpg_text_percode_f16 widens,
 * normalises with sklearn's division and continues with the same f32 arithmetic: its tables are the reference's on
 * the f16-rounded database, bit for bit.  Half the HBM bytes of the dominant array; the sweep stays VALU-bound. */
int qpg_text_pack_candidates_f16(qpg_ctx*, void* stream, const float* x, int N, int R, int Dm, const int32_t* cand_r,
                                 int G, void* xh, float* nrm);
int qpg_text_percode_f16(qpg_ctx*, void* stream, const void* xh, const float* nrm, int64_t C, int Dm,
                         const int16_t* cand_code, int K, const float* qn, int Q, int32_t idx_base, float absent,
                         void* ws, int64_t ws_bytes, float* out_dist, int32_t* out_idx, int16_t* out_rank,
                         int32_t* out_nn);

/* BOUNDED PREFILTER + EXACT REFINE for the exact-f32 cosine family (round 3; BASELINE.json configs[2] and the matcher's
 * text side, GestureKNN.py:708-721): bit-identical tables to qpg_text_percode_f32 at a fraction of its VALU work.  Build
 * side (host, once; qpgesture_amd/sorted_rows.py): sklearn-normalise the rows (qpg_l2_normalize_rows_f32), drop masked rows,
 * keep per code only the FIRST of the rows the normalisation left at zero (zero_row), sort the rest by code (stable) into
 * segments padded to 16 rows with copies of the segment's first row, R %% 32 == 0.
 *   qpg_hl_pack_rows / qpg_hl_pack_cols   split-f16 fragment images of the sorted unit rows xs [dev] f32 [R][D] and of the
 *       normalised queries qn [dev] f32 [Q][D] (chunks of 96); sizes: qpg_hl_rows_bytes / qpg_hl_cols_bytes.  D %% 128 == 0.
 *   qpg_hl_gemm_distance   Dm [dev] f32 [Q][ldD >= R]: Dm[q][r] = 1 - <xs[r], qn[q]> on the f16 matrix cores (the kernel of
 *       qpg_audio_cosine_hl with a plain epilogue; |Dm - true| <= QPG_AUDIO_HL_ERR for unit-norm operands); tile_min
 *       (optional) [dev] f32 [Q][ldT >= R / 16]: the minimum of every 16-row tile, what the select reads first.
 *   qpg_percode_select_sorted_f32   per query: per-code minimum of Dm from the tile minima, every row within `band` of it
 *       evaluated in sklearn's exact f32 order (0.5 * einsum_sq(qn - xs)), minimum exact distance and lowest ORIGINAL index
 *       per code.  row_code [dev] i16 [R]: code of sorted row r (K <= 2048), | 0x4000 for padding rows, 0x1fff for the tail
 *       past the last segment; row_index [dev] i32 [R]: original index; zero_row [dev] i32 [K] or NULL: original index of the
 *       code's first all-zero row (-1: none) - it enters with the prefilter value 0.5; xs holds R + 1 rows, row R zeros;
 *       code_tile [dev] i32 [K + 1]: first 16-row tile of every code's segment (8 blocks per query take a range of codes
 *       each; ranks / nearest neighbours: a second small launch).  A band list is 2048 rows / 1024 opened tiles per block.
 *       `band` >= 2 x (prefilter error + sklearn's own rounding against the real value): derivation in
 *       csrc/qpg_sorted.hip (8.6e-5 at D = 512).  stats[1] |= 16 if a band list overflowed (its own bit, round 4): run
 *       qpg_text_percode_f32 instead.  out_rank optional: i16 [Q][K] ranks of the table rows (qpg_rank_rows_f32's);
 *       out_nn optional: the query's global nearest neighbour (original index).  idx_base is added to every index written;
 *       q_block / block_stride: the exchange layout of qpg_percode_select_f32 (row shards; no ranks / nn then). */
int64_t qpg_hl_rows_bytes(int64_t R, int D);
int64_t qpg_hl_cols_bytes(int Q, int D);
int qpg_hl_pack_rows(qpg_ctx*, void* stream, const float* xs, int64_t R, int D, void* image, int64_t image_bytes);
int qpg_hl_pack_cols(qpg_ctx*, void* stream, const float* qn, int Q, int D, void* image, int64_t image_bytes);
/* Round 6: the query side of a prefilter batch in ONE launch - qpg_l2_normalize_rows_f32 (sklearn's normalize, bit for bit)
 * + qpg_hl_pack_cols + qpg_perm32_rows_f32 on the RAW queries q [dev] f32 [Q][D]: qn_out (optional) [dev] f32 [Q][D] the
 * normalised rows, cols_image qpg_hl_cols_bytes(Q, D) bytes, qperm_out (optional) [dev] f32 [Q][D] the chain-permuted
 * normalised rows qpg_percode_select_bycode_f32 reads.  Outputs bit-identical to the three calls.  D %% 128 == 0. */
int qpg_hl_prepare_queries(qpg_ctx*, void* stream, const float* q, int Q, int D, float* qn_out, void* cols_image,
                           int64_t image_bytes, float* qperm_out);
int qpg_hl_gemm_distance(qpg_ctx*, void* stream, const void* rows_image, int64_t R, int D, const void* cols_image, int Q,
                         float* Dm, int64_t ldD, float* tile_min, int64_t ldT);
/* Round 4: the same GEMM WITHOUT its matrix - per (query, 16-row tile) the minimum and a 16-bit mask of the rows within
 * `band` of it (tile_min f32 / tile_mask u16 [dev] [Q][ldT >= R/16]).  A tile is opened by the select only if its minimum is
 * within the band of its code's minimum, and code minimum <= tile minimum, so the masked rows are a superset of the band's
 * rows: qpg_percode_select_sorted_f32 with `tile_mask` never reads Dm (may be NULL).  6 bytes per (query, tile) instead of
 * 64: cfg-3's 375 MB prefilter matrix is neither written nor read. */
int qpg_hl_gemm_tilemin(qpg_ctx*, void* stream, const void* rows_image, int64_t R, int D, const void* cols_image, int Q,
                        float band, float* tile_min, uint16_t* tile_mask, int64_t ldT);
/* Round 5, many queries per batch (BASELINE.json configs[2]): the prefilter on the h PLANES ALONE and the exact-order
 * evaluations BY CODE.
 *   qpg_hl_gemm_tilemin_h   one f16 MFMA per 16 x 16 x 32 block (the cross terms h l' + l h' and l l' are dropped: at most
 *       (2^-10 + 2^-22) |x||q| by Cauchy-Schwarz - `band` must cover it: sorted_rows.gemm_h_err), 64-row wave tiles; writes
 *       tile minima and row masks TILE-MAJOR: tile_min f32 / tile_mask u16 [dev] [R / 16][ldQ >= Q].  R %% 64 == 0,
 *       D %% 256 == 0.  Same images as qpg_hl_gemm_tilemin (the l planes are not read).
 *   qpg_perm32_rows_f32     y[r][32 G + 8 k + j] = x[r][16 (2 G + (j >> 2)) + 4 (3 - (j & 3)) + k]: inside every 32-element
 *       group (one 128-byte line) the four einsum chains of sklearn's f32 sum of squares become four 32-byte runs in visiting
 *       order (rows once at build time, the queries per batch).  D %% 32 == 0.
 *   qpg_percode_select_bycode_f32   the tables of qpg_percode_select_sorted_f32 (bit-identical), one block per (code, query
 *       range): the code's minimum per query from the tile-major minima, the opened tiles' masked rows listed as (query,
 *       row) pairs, every pair evaluated in the exact order by four lanes (one per chain) from the chain-permuted rows
 *       xs_perm [R + 1][D] / queries qn_perm [Q][D] - a segment's rows are fetched from HBM once for all queries (the by-query
 *       kernel gathers 2 KB per pair: 0.95 GB per 1 000 queries of cfg-3).  A block = one code, its rows staged through LDS tile by tile; a tile's pair list holds 1 024 pairs;
 *       overflow: stats[1] |= 16.  No exchange layout (q_block): single-GPU batches and per-shard tables only. */
int qpg_hl_gemm_tilemin_h(qpg_ctx*, void* stream, const void* rows_image, int64_t R, int D, const void* cols_image, int Q,
                          float band, float* tile_min_t, uint16_t* tile_mask_t, int64_t ldQ);
int qpg_perm32_rows_f32(qpg_ctx*, void* stream, const float* x, int64_t R, int D, float* y);
int qpg_percode_select_bycode_f32(qpg_ctx*, void* stream, const float* tile_min_t, const uint16_t* tile_mask_t, int64_t ldQ,
                                  int Q, int64_t R, const int16_t* row_code, const int32_t* row_index,
                                  const int32_t* zero_row, const int32_t* code_tile, int K, float band,
                                  const float* qn_perm, const float* xs_perm, int D, float absent, float* out_dist,
                                  int32_t* out_idx, int16_t* out_rank, int32_t* out_nn, int32_t* stats, int32_t idx_base);
int qpg_percode_select_sorted_f32(qpg_ctx*, void* stream, const float* Dm, int64_t ldD, const float* tile_min,
                                  const uint16_t* tile_mask /* or NULL: rows are taken from Dm */, int64_t ldT,
                                  int Q, int64_t R, const int16_t* row_code, const int32_t* row_index,
                                  const int32_t* zero_row, const int32_t* code_tile, int K, float band, const float* qn,
                                  const float* xs, int D, float absent, float* out_dist, int32_t* out_idx,
                                  int16_t* out_rank, int32_t* out_nn, int32_t* stats, int32_t idx_base, int q_block,
                                  int64_t block_stride);

/* vq-wav2vec audio sweep (the mode the paper describes; flags use_wavvq/use_feature of GestureKNN.py:557-560):
 * D[q][c] = Levenshtein distance (unit costs, python-Levenshtein distance()) between the 11-symbol strings of
 * query q and candidate c, symbol = g1*320+g2 (wavvq_distances(mode='combine'), GestureKNN.py:57-67).  Strings
 * are gathered in place from symbol tracks: string[i] = track[t + tap_off[i]] (0 outside the window), which is
 * the 6-back/5-forward stack of data_processing.py:297-335 without materialising it.
 * sym_db: [dev] i32 [N][T]; cand_t: [dev] i32 [G] (int(k) of the float grid); tap_off: HOST i32 [11];
 * sym_q: [dev] i32 [Mq][Tq]; q_win/q_t: [dev] i32 [Q]; D: [dev] f32 [Q][N*G] (exact small integers). */
int qpg_wavvq_lev_f32(qpg_ctx*, void* stream, const int32_t* sym_db, int N, int T, const int32_t* cand_t, int G,
                      const int32_t* tap_off, int n_taps, const int32_t* sym_q, int Mq, int Tq,
                      const int32_t* q_win, const int32_t* q_t, int Q, float* D, int64_t ldD);

/* Segmented min + argmin by code id in one launch: per query row the per-code minimum, its
 * first-wins candidate (lowest index among equal distances == the strict `<` scan of GestureKNN.py:686-689, 717-720),
 * `absent` / -1 for codes with no candidate, and optionally the stable ranks of the 512 minima.
 * D: [dev] [Q][ldD] distances; cand_code: [dev] i16 [C] code of candidate c (values outside [0,K) are skipped);
 * out_dist [Q][K], out_idx i32 [Q][K] = c + idx_base, out_rank i16 [Q][K] or NULL.  K <= 2048.
 * q_block > 0 (sharded database): the outputs are written in EXCHANGE layout - row q goes to row q % q_block of block
 * q / q_block, blocks `block_stride` BYTES apart starting at out_dist / out_idx (one block per destination rank of the
 * all-to-all, several arrays per block); out_rank must then be NULL (ranks are taken after the merge). */
int qpg_percode_select_f64(qpg_ctx*, void* stream, const double* D, int64_t ldD, int Q, const int16_t* cand_code,
                           int64_t C, int K, double absent, int32_t idx_base, double* out_dist, int32_t* out_idx,
                           int16_t* out_rank, int q_block, int64_t block_stride);
int qpg_percode_select_f32(qpg_ctx*, void* stream, const float* D, int64_t ldD, int Q, const int16_t* cand_code,
                           int64_t C, int K, float absent, int32_t idx_base, float* out_dist, int32_t* out_idx,
                           int16_t* out_rank, int q_block, int64_t block_stride);

/* qpg_percode_select_f64 with the NEAR-TIE GUARD (SURVEY.md §7 hard part 2).  The sweep's distances (dot-product
 * form on the f64 matrix cores) and the reference's (sklearn: 0.5*|q/|q| - c/|c||^2, NumPy einsum order,
 * GestureKNN.py:685) agree to ~1e-16 but can order two distances closer than that differently.  Candidates within `eps`
 * of their code's minimum (two or more) are re-evaluated in the reference's exact arithmetic and the winner taken by
 * (reference distance, index); minima of different codes within `eps` of each other are replaced by the
 * reference-arithmetic value of their winner before ranking.  All inside the launch; nothing is flagged on ordinary data.
 * base [dev] f32 [N][T][F], cand_t [dev] i32 [G], q32 [dev] f32 [Q][n_taps*F]: the sweep's own operands (C == N*G);
 * stats [dev] i32 [4]: [0] += re-evaluated (query, candidate) pairs, [1] |= 1 if more than 256 were flagged in one row
 * (the surplus keeps its sweep value). */
int qpg_percode_select_guarded_f64(qpg_ctx*, void* stream, const double* D, int64_t ldD, int Q, const int16_t* cand_code,
                                   int64_t C, int K, double absent, int32_t idx_base, double* out_dist, int32_t* out_idx,
                                   int16_t* out_rank, int q_block, int64_t block_stride, const float* base, int T, int F,
                                   const int32_t* cand_t, int G, int n_taps, int tap_stride, const float* q32, double eps,
                                   int32_t* stats, int base_is_f16);
/* base_is_f16 != 0 (here and in qpg_percode_select_mixed_f64): `base` points at an IEEE f16 track (as swept by
 * qpg_audio_cosine_f64_h / qpg_audio_cosine_mx_h); the re-evaluation then runs on the widened, i.e. rounded, values. */

/* UNCAPPED form of the guarded select (round 3): same arguments, results and arithmetic, but every list lives in `ws`
 * ([dev] qpg_percode_select_exact_ws_bytes(Q, C, K) bytes, 16-byte aligned, contents on entry are ignored; sized for ALL C
 * candidates of a row inside one band), so no population of near-ties can overflow it and stats[1] is never raised: the reference's scan
 * (GestureKNN.py:685-689) visits every candidate with a strict `<` and has no cap either.  This is the path the host
 * re-matches a clip on when a capped select or the mixed-precision sweep raised stats[1].  Five launches; K <= 1024. */
int64_t qpg_percode_select_exact_ws_bytes(int Q, int64_t C, int K);
int qpg_percode_select_exact_f64(qpg_ctx*, void* stream, const double* D, int64_t ldD, int Q, const int16_t* cand_code,
                                 int64_t C, int K, double absent, int32_t idx_base, double* out_dist, int32_t* out_idx,
                                 int16_t* out_rank, int q_block, int64_t block_stride, const float* base, int T, int F,
                                 const int32_t* cand_t, int G, int n_taps, int tap_stride, const float* q32, double eps,
                                 int32_t* stats, int base_is_f16, void* ws, int64_t ws_bytes);

/* Select for the matrix of qpg_audio_cosine_mx.  Same outputs as qpg_percode_select_guarded_f64.  Two sweep values
 * further apart than eps1 (>= 2 x QPG_AUDIO_MX_ERR) are ordered like the exact distances; inside that band
 *   tier 1: all candidates within eps1 of their code's minimum (if two or more) and the winners of codes whose minima
 *           are rank neighbours within eps1 get an f64 dot product (error ~1e-15, like qpg_audio_cosine_f64);
 *   tier 2: on those values, the near-tie guard above with band eps2 (the reference's own arithmetic; 0 = off).
 * out_dist holds the sweep value (error <= QPG_AUDIO_MX_ERR) for untouched codes, the re-evaluated one otherwise.
 * Pass out_rank: without it the minima of different codes are not protected against each other.
 * qn2 [dev] f64 [Q], cn2 [dev] f64 [C]: the sweep's squared norms.  stats [dev] i32 [4]: [0] += tier-2 pairs,
 * [1] |= 1 if a list overflowed (2048 tier-1 / 256 tier-2 entries per query; results then unguarded), [2] += tier-1
 * pairs.  K <= 512. */
int qpg_percode_select_mixed_f64(qpg_ctx*, void* stream, const void* D, int d_is_f32, int64_t ldD, int Q, const int16_t* cand_code,
                                 int64_t C, int K, double absent, int32_t idx_base, double* out_dist, int32_t* out_idx,
                                 int16_t* out_rank, int q_block, int64_t block_stride, const float* base, int T, int F,
                                 const int32_t* cand_t, int G, int n_taps, int tap_stride, const float* q32,
                                 const double* qn2, const double* cn2, double eps1, double eps2, int32_t* stats,
                                 void* ws, int64_t ws_bytes, int base_is_f16);
/* ws: [dev] scratch of qpg_percode_select_mixed_ws_bytes(Q, K) bytes, 16-byte aligned, ZERO-FILLED ONCE by the caller
 * (part of it is state the launches leave all-zero for the next call; a workspace may be reused for any smaller Q) - with
 * it the call is four launches (the row streamed by 8 blocks per query | lists | tier-1 dot products, 256 waves per query
 * | merge, tier 2, ranks; an f64 matrix: three, the lists' launch streams the row itself); NULL: one launch, each query's
 * work on its own CU.  qpg_percode_select_mixed_ws_stride(K): bytes per query - query q's tier-1 list length is the i32
 * at q x stride + 24 K (diagnostics). */
int64_t qpg_percode_select_mixed_ws_bytes(int Q, int K);
int64_t qpg_percode_select_mixed_ws_stride(int K);
/* The same call with the WALK-RELEVANCE CUT of its re-evaluation lists (f32 matrix + workspace + out_rank, no block layout).
 * The walk reads, per step and previous code p, only the code(s) with the smallest fused score
 *     pos_rank[p][c] + 0.05 freq_rank[c] + rank(c)          (GestureKNN.py:540-545, :574-576; order[0], order[:2] at :593)
 * so a code whose rank is CERTAINLY above every previous code's winning score can never be read: neither its rank among
 * near-tied neighbours nor its winner among near-tied candidates is settled in f64 (unless a code that can be read lies
 * within eps1 of it).  Such a code's table entries keep the sweep's values (|value - exact| <= eps1 / 2.1), its rank is its
 * position among them; every entry the walk can read - and therefore every selected code index - is what
 * qpg_percode_select_mixed_f64 returns.  pos_rank_t [dev] i16 [K][K]: the TRANSPOSE of qpg_match_steps' pos_rank
 * (pos_rank_t[c * K + p]); freq_rank [dev] i16 [K]; top_n: 1 with the text side, 2 without; probe: best-ranked codes the
 * bound on the winning score is taken over (0: 64). */
int qpg_percode_select_mixed_f64_cut(qpg_ctx*, void* stream, const void* D, int d_is_f32, int64_t ldD, int Q,
                                     const int16_t* cand_code, int64_t C, int K, double absent, int32_t idx_base,
                                     double* out_dist, int32_t* out_idx, int16_t* out_rank, int q_block, int64_t block_stride,
                                     const float* base, int T, int F, const int32_t* cand_t, int G, int n_taps,
                                     int tap_stride, const float* q32, const double* qn2, const double* cn2, double eps1,
                                     double eps2, int32_t* stats, void* ws, int64_t ws_bytes, int base_is_f16,
                                     const int16_t* pos_rank_t, const int16_t* freq_rank, int top_n, int probe);

/* Cross-shard merge when the shards swept with qpg_audio_cosine_mx (their tables are accurate to QPG_AUDIO_MX_ERR; each
 * shard's own select has settled the near-ties inside the shard).  Three steps around two more byte exchanges:
 *   qpg_merge_mixed_phase1_f64  (owner of a query block)  approximate merge of the W received tables (same layout
 *       arguments as qpg_merge_select_f64); every shard within eps1 of a code's merged minimum — when there are two or
 *       more — and the winners of codes whose merged minima are rank neighbours within eps1 become requests to the
 *       shard holding the candidate.  req: [dev] W blocks of req_stride bytes, block w = [i64 count][R x u64
 *       (q_local << 48 | code << 32 | global candidate)]: the send buffer of an all-to-all.  ws: [dev] scratch of
 *       qpg_merge_mixed_ws_bytes(Q, K, fl_cap) bytes, kept for phase 2 (fl_cap = flagged (code, shard) entries per
 *       query); contents on entry to phase 1 are ignored, phase 2 reads only what phase 1 wrote.  stats[1] |= 4 on request / flag-list overflow: every written request is valid and every counted flag
 *       entry written, the surplus is dropped and the clip must be re-matched (R = Q*K and fl_cap = K*W cannot overflow).
 *   qpg_shard_refine_f64        (every shard)  req_recv = the W request blocks received (block o from owner o); the
 *       exact f64 distance of every requested (query o*q_stride + q_local, candidate - cand_base) goes to resp block o
 *       ([R x f64], resp_stride bytes apart): the send buffer of the answering all-to-all.  reference_arithmetic != 0:
 *       the distance in the reference's own arithmetic instead (sklearn normalise + einsum-order sum, as tier 2).
 *   qpg_merge_mixed_phase2_f64  (owner)  winners among the re-evaluated contenders by (exact value, candidate), stable
 *       ranks over re-evaluated and untouched minima.  stats[3] += re-evaluated entries.  eps2 > 0: contenders of one
 *       code, or minima of rank-neighbour codes, closer than eps2 raise stats[1] |= 8 (dot-product responses cannot
 *       order them like the reference; the host re-matches the clip with reference-arithmetic responses and eps2 = 0).
 * The same three calls with eps1 = the near-tie band (1e-12), reference_arithmetic = 1 and eps2 = 0 are the cross-shard
 * TIER 2: the uncapped sharded path (CodeKNN, audio_precision "exact"). */
int64_t qpg_merge_mixed_ws_bytes(int Q, int K, int fl_cap);
/* Round 4: request slots are DETERMINISTIC - (query q, code k) -> shard w sits at slot q * (R / Q) + its position among q's
 * requests to w in code order, unused slots hold ~0 (R % Q == 0) - so every rank that merges the same tables builds the
 * same request blocks and, in the all-gather form, a shard refines its own block of its own run: no request exchange.
 * Block headers (8 bytes in front of the R slots of a request / response block): [i32 count (diagnostics) | i32 trouble
 * bits].  The bits TRAVEL WITH THE EXCHANGES: phase 1 ORs the W table blocks' flag words (at `flag_off` inside a table
 * block, < 0: none) into stats[1] and seeds the request headers; the shard refine ORs the received request headers into
 * stats[1] (stats may be NULL) and seeds the response headers; phase 2 ORs those in.  resp_stride >= 8 + 8 R. */
int qpg_merge_mixed_phase1_f64(qpg_ctx*, void* stream, const void* recv, int W, int64_t src_stride, int64_t dist_off,
                               int64_t idx_off, int Q, int K, double absent, double eps1, int R, void* req,
                               int64_t req_stride, void* ws, int64_t ws_bytes, int32_t* stats, int fl_cap,
                               int64_t flag_off);
int qpg_shard_refine_f64(qpg_ctx*, void* stream, const void* req_recv, int W, int64_t req_stride, int R, int q_stride,
                         int64_t cand_base, const float* base, int base_is_f16, int T, int F, const int32_t* cand_t, int G,
                         int n_taps, int tap_stride, const float* q32, const double* qn2, const double* cn2, void* resp,
                         int64_t resp_stride, int reference_arithmetic, int32_t* stats, int Rq);
/* The trouble word riding in an exchanged buffer: stamp = every one of nblk blocks' i32 at `off` := stats[1] (sender,
 * before the exchange); gather = stats[1] |= OR of the nblk received words (receiver). */
int qpg_flags_stamp(qpg_ctx*, void* stream, void* buf, int nblk, int64_t stride, int64_t off, const int32_t* stats);
int qpg_flags_gather(qpg_ctx*, void* stream, const void* buf, int nblk, int64_t stride, int64_t off, int32_t* stats);
int qpg_merge_mixed_phase2_f64(qpg_ctx*, void* stream, const void* recv, int W, int64_t src_stride, int64_t idx_off, int Q,
                               int K, double absent, const void* ws, int64_t ws_bytes, const void* resp_recv,
                               int64_t resp_stride, double* out_dist, int32_t* out_idx, int16_t* out_rank, int32_t* stats,
                               int fl_cap, double eps2);

/* Cross-shard min + index merge after the RCCL exchange (the all-reduce(min, index) `north_star`
 * names, as all-gather / all-to-all + this kernel): source w's tables start at recv + w*src_stride (+ dist_off for the
 * [Q][K] distances, + idx_off for the [Q][K] i32 global candidate indices, -1 = absent in that shard).  Winner per
 * (query, code): minimum distance, lowest index among equals.  out_rank (optional): stable ranks of the merged row.
 * _f64 only: eps2 > 0 with stats != NULL raises stats[1] |= 8 when two shards' minima of one code, or the merged minima
 * of rank-neighbour codes, are closer than eps2 (the shards settle near-ties inside themselves only; the host then
 * re-matches the clip on the uncapped path, whose merge compares such pairs in the reference's own arithmetic). */
int qpg_merge_select_f64(qpg_ctx*, void* stream, const void* recv, int W, int64_t src_stride, int64_t dist_off,
                         int64_t idx_off, int Q, int K, double absent, double* out_dist, int32_t* out_idx,
                         int16_t* out_rank, double eps2, int32_t* stats);
int qpg_merge_select_f32(qpg_ctx*, void* stream, const void* recv, int W, int64_t src_stride, int64_t dist_off,
                         int64_t idx_off, int Q, int K, float absent, float* out_dist, int32_t* out_idx,
                         int16_t* out_rank);

/* Stable ranks of each row: rank[q][c] = #{c' : d[c'] < d[c] or (d[c'] == d[c] and c' < c)}
 * (== np.argsort(kind='stable').argsort(); the reference calls the unstable default,
 * GestureKNN.py:553,574).  out: [dev] i16 [Q][K]. */
int qpg_rank_rows_f64(qpg_ctx*, void* stream, const double* d, int Q, int K, int16_t* out);
int qpg_rank_rows_f32(qpg_ctx*, void* stream, const float* d, int Q, int K, int16_t* out);

/* ------------------------------------------------------------------------------------------
 * State-dependent tail of CodeKNN.search_code_knn + the window loop of predict_code_from_audio
 * (GestureKNN.py:501-664, 785-813).
 * ---------------------------------------------------------------------------------------- */

/* out[p][c] = |sig[p] - sig[c]|_2 in f32 (f64 accumulation, one rounding), +inf on the diagonal
 * (GestureKNN.py:531-536: `1e10000` for the current code).  sig: [dev] f32 [K][Dm]; out: [dev] f32 [K][K]. */
int qpg_l2_table_f32(qpg_ctx*, void* stream, const float* sig, int K, int Dm, float* out);

#define QPG_MODE_AUD_TXT 0 /* shipped flags: audio top-1 vs text top-1, phase gate (GestureKNN.py:627-657) */
#define QPG_MODE_AUD 1     /* audio only: top-2 audio candidates through the phase gate (:593-608)          */
#define QPG_MODE_TXT 2     /* text only: top-2 text candidates through the phase gate (:610-625)            */
#define QPG_MODE_SERIAL_WALK 0x100 /* OR-ed into mode: force the one-wave sequential walk (validation of the tabulated one) */
#define QPG_MODE_PREFUSED 0x200    /* OR-ed into QPG_MODE_AUD_TXT: gate_tables [0] / [1] were filled by qpg_fuse_best_ranked */

/* Walk all M windows x `steps` matching steps of a clip on the device.
 *   aud_rank/txt_rank: [dev] i16 [Q][K] stable ranks of the per-code minima (Q = M*steps);
 *   aud_idx/txt_idx:   [dev] i32 [Q][K] winning candidate index j*G+g (-1 = code absent);
 *   pos_rank:          [dev] i16 [K][K] stable ranks of qpg_l2_table_f32 rows;
 *   freq_rank:         [dev] i16 [K] rank of 1-count/total (GestureKNN.py:481-499, 544);
 *   code:              [dev] i32 [N][code_ld]; *_cidx [G]: code column of a grid position;
 *   *_pslot [G]:       phase start frame int(k/398*240) of a grid position (GestureKNN.py:632);
 *   phase:             [dev] f32 [N][Tp][2][8] (phase shift, amplitude);
 *   seed_code/seed_phase [dev f32 8x16]: init_code_phase() draw (GestureKNN.py:462-473);
 *   gate_tables:       [dev] i32 [3][Q][K] scratch (contents on entry are ignored): the two phase-gate candidates for every (step, previous
 *                      code), and the gate outcome for every (step, previous code, previous vote) — both
 *                      tabulated in parallel, so that the sequential part is Q dependent 2-byte lookups;
 *   out_codes [dev] i32 [M][30]; out_phase [dev] f32 [M][steps][8][16]; out_vote [dev] i32 [M][steps];
 *   out_status [dev] i32 [2]: [0] = 1 if a code absent from the DB won a rank fusion (the reference raises
 *   IndexError there, GestureKNN.py:631-632); [1] = *guard_flags (0 if NULL): the trouble word stats[1] of the
 *   sweeps / selects that produced the tables (list overflow, norms outside the error bound's range, cross-shard
 *   near tie), copied by the walk's last kernel so that it leaves the device in the same D2H copy as the codes —
 *   the host must not use codes whose status[1] != 0 (CodeKNN re-matches such a clip on the uncapped exact path).
 * combined = (pos_rank + freq_rank*0.05) + rank in float64 in that order; argmin = lowest index. */
int qpg_match_steps(qpg_ctx*, void* stream, const int16_t* aud_rank, const int32_t* aud_idx,
                    const int16_t* txt_rank, const int32_t* txt_idx, const int16_t* pos_rank,
                    const int16_t* freq_rank, const int32_t* code, int code_ld, const int32_t* aud_cidx,
                    const int32_t* aud_pslot, int Ga, const int32_t* txt_cidx, const int32_t* txt_pslot, int Gt,
                    const float* phase, int Tp, int mode, int M, int steps, int K, int seed_code,
                    const float* seed_phase, int32_t* gate_tables, int32_t* out_codes, float* out_phase,
                    int32_t* out_vote, int32_t* out_status, const int32_t* guard_flags);
/* The same for several INDEPENDENT clips (chains) of M windows each in one set of launches (BASELINE configs[4]: 16 clips
 * per sweep): the tables hold the chains' steps back to back ([n_chains x M x steps][K]); seed_codes [dev] i32 [n_chains],
 * seed_phase [dev] f32 [n_chains][8][16]; outputs [n_chains][...] in the single-clip shapes; chain c's status pair at
 * out_status + c x status_stride (>= 2).  gate_tables: 3 x n_chains x M x steps x K i32.  M > 0. */
int qpg_match_steps_batch(qpg_ctx*, void* stream, const int16_t* aud_rank, const int32_t* aud_idx, const int16_t* txt_rank,
                          const int32_t* txt_idx, const int16_t* pos_rank, const int16_t* freq_rank, const int32_t* code,
                          int code_ld, const int32_t* aud_cidx, const int32_t* aud_pslot, int Ga, const int32_t* txt_cidx,
                          const int32_t* txt_pslot, int Gt, const float* phase, int Tp, int mode, int M, int steps, int K,
                          int n_chains, const int32_t* seed_codes, const float* seed_phase, int32_t* gate_tables,
                          int32_t* out_codes, float* out_phase, int32_t* out_vote, int32_t* out_status,
                          int64_t status_stride, const int32_t* guard_flags);
/* Several TAKES of ONE clip: the clip's tables (Q = M x steps rows, as for qpg_match_steps) walked from n_takes seeds in
 * one set of launches.  Nothing in front of the walk reads the seed, and of the walk only a take's first step does: the
 * rank fusion (unless QPG_MODE_PREFUSED) and the gate table run ONCE, through qpg_match_steps' kernels (the same bits as a
 * one-take call); then one kernel evaluates step 0 of every take, one chases all takes (64 per block: a window's gate
 * table is staged into LDS once per block, one lane per take) and one writes the results (a block per take).
 *   n_takes 1 .. QPG_TAKES_MAX; seed_codes [dev-readable] i32 [n_takes], every one in [0, K) (the caller checks);
 *   seed_phase [dev-readable] f32 [n_takes][8][16]; gate_tables [dev] i32 [3][Q][K] as for ONE clip;
 *   out_codes i32 [n_takes][M][30]; out_phase f32 [n_takes][M][steps][8][16]; out_vote i32 [n_takes][M][steps];
 *   take t's status pair at out_status + t x status_stride (>= 2), written last behind a system-scope fence;
 *   workspace [dev]: qpg_match_steps_takes_ws_bytes(n_takes, M, steps) bytes (the takes' trails of states; contents on
 *   entry are ignored).
 * mode: the three modality modes and QPG_MODE_PREFUSED as for qpg_match_steps.  Where the tabulated walk does not apply
 * (QPG_MODE_SERIAL_WALK, a geometry the tabulation refuses) the call returns QPG_EUNSUP before launching anything: the
 * caller walks the takes one at a time. */
#define QPG_TAKES_MAX 65536
size_t qpg_match_steps_takes_ws_bytes(int n_takes, int M, int steps);
int qpg_match_steps_takes(qpg_ctx*, void* stream, const int16_t* aud_rank, const int32_t* aud_idx, const int16_t* txt_rank,
                          const int32_t* txt_idx, const int16_t* pos_rank, const int16_t* freq_rank, const int32_t* code,
                          int code_ld, const int32_t* aud_cidx, const int32_t* aud_pslot, int Ga, const int32_t* txt_cidx,
                          const int32_t* txt_pslot, int Gt, const float* phase, int Tp, int mode, int M, int steps, int K,
                          int n_takes, const int32_t* seed_codes, const float* seed_phase, int32_t* gate_tables,
                          int32_t* out_codes, float* out_phase, int32_t* out_vote, int32_t* out_status,
                          int64_t status_stride, const int32_t* guard_flags, void* workspace, size_t workspace_bytes);
/* One modality's half of the rank fusion in front of the walk (GestureKNN.py:540-545 + :574-576 for the audio order,
 * :553-555 for the text order - two independent argsorts): T[q][p] = idx[q][argmin_c (pos_rank[p][c] + 0.05 freq_rank[c])
 * + rank[q][c]] (f64, that order of operations; lowest code among equal scores).  rank [dev] i16 [Q][K] (a permutation per
 * row), idx [dev] i32 [Q][K], T [dev] i32 [Q][K]: region [0] (audio) or [1] (text) of the walk's gate_tables.  Launched
 * behind each modality's select on ITS stream, the walk (qpg_match_steps* with QPG_MODE_PREFUSED) then starts at the gate
 * table and the join of the two streams has half a rank fusion less in front of it.  K % 16 == 0, K <= 4096. */
int qpg_fuse_best_ranked(qpg_ctx*, void* stream, const int16_t* rank, const int32_t* idx, const int16_t* pos_rank,
                         const int16_t* freq_rank, int Q, int K, int32_t* T);
/* (From how many chains per launch qpg_match_steps_batch deduplicates the gate table by the previous step's winner - one
 * evaluation per DISTINCT winner instead of one per (previous code, vote) state; same table, bit for bit - is the context's
 * QPG_OPT_GATE_DEDUP_FROM_CHAINS: qpg_ctx_set_option.) */

/* The walk WITHOUT the phase gate: the `not use_phase` branches of search_code_knn (GestureKNN.py:578-592) and the window
 * loop around them (:785-813), for n_chains independent clips of M windows x `steps` steps whose steps sit back to back in
 * the tables, as in qpg_match_steps_batch.  The tables and the database arguments are qpg_match_steps' (no phase track, no
 * phase slots).  Per step, with p the previous code (the chain's seed code at its first step, :466-467 / :517-520):
 *   pos_score = pos_rank[p] + freq_rank * 0.05                                                          (:540-545)
 *   QPG_MODE_AUD_TXT  combined = (pos_score + aud_rank[q]) + txt_rank[q]; c* = the code at position desired_k of the
 *                     sorted order; the 4 codes of the AUDIO candidate aud_idx[q][c*] are appended if the step's coin is
 *                     nonzero (`np.random.rand() > 0.5`), those of the TEXT candidate txt_idx[q][c*] otherwise (:578-586)
 *   QPG_MODE_AUD      combined = pos_score + aud_rank[q]; the audio candidate of c*, no coin                (:587-589)
 *   QPG_MODE_TXT      combined = pos_score + txt_rank[q]; the text candidate of c*, no coin.  (The reference indexes
 *                     aud_index_cands there, :591, a name that does not exist in that branch; this is the evident intent.)
 * all in float64 in that order of operations.  Equal scores are ordered by code index (the gated walk's rule; np.argsort
 * leaves their order open): position k is the k-th element of the order by (score, code).  0 <= desired_k <
 * QPG_NOPHASE_KMAX.  The next step's previous code is the 4th code of the appended block; a window keeps the first
 * min(4 steps, 30) of its codes and the next window starts from the last KEPT one (motion_output[-1][-1], :791-806), which
 * must come from the window's last step - a geometry where it does not (or Q per chain > 2048, or tables beyond the LDS)
 * returns QPG_EUNSUP before anything is launched.  K % 4 == 0, K <= 1024.
 *   seed_codes [dev-readable] i32 [n_chains]; coins [dev-readable] u8 [n_chains][M steps], nonzero = audio: required for
 *   QPG_MODE_AUD_TXT, ignored (may be NULL) otherwise; the tables / grids of a side the mode does not use may be NULL;
 *   out_codes i32 [n_chains][M][min(4 steps, 30)]; out_side i32 [n_chains][M steps]: 0 audio / 1 text;
 *   out_cand i32 [n_chains][M steps]: the appended candidate j x G + g (which database window and grid position the block
 *   came from); chain c's status pair at out_status + c x status_stride (>= 2), written last behind a system-scope fence:
 *   [0] = 1 if the chain reached a code without a candidate (the reference appends nothing there and returns a ragged
 *   result) or a seed / payload code outside [0, K) - the chain stops, the steps behind it hold -1 -, [1] = *guard_flags;
 *   workspace [dev], qpg_match_steps_nophase_ws_bytes(n_chains, M, steps, K) bytes: next u16 [Q][2][K] (Q = n_chains M
 *   steps; [q][s][p]: the previous code after step q when side s, 0 audio / 1 text, is taken from previous code p; 0xFFFF:
 *   none) followed by pick i32 [Q][2][K] (that side's candidate of c*, -1: none); a side the mode does not use holds
 *   0xFFFF / -1.  Contents on entry are ignored.  M == 0 writes the status pairs only.
 * Two launches: the tables for every (step, previous code), then one block per chain that follows next through LDS. */
#define QPG_NOPHASE_KMAX 16
size_t qpg_match_steps_nophase_ws_bytes(int n_chains, int M, int steps, int K);
int qpg_match_steps_nophase(qpg_ctx*, void* stream, const int16_t* aud_rank, const int32_t* aud_idx,
                            const int16_t* txt_rank, const int32_t* txt_idx, const int16_t* pos_rank,
                            const int16_t* freq_rank, const int32_t* code, int code_ld, const int32_t* aud_cidx, int Ga,
                            const int32_t* txt_cidx, int Gt, int mode, int desired_k, int M, int steps, int K, int n_chains,
                            const int32_t* seed_codes, const uint8_t* coins, int32_t* out_codes, int32_t* out_side,
                            int32_t* out_cand, int32_t* out_status, int64_t status_stride, const int32_t* guard_flags,
                            void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * Library-owned collectives of the row-sharded matcher (round 5).  The reference has no
 * collective (its would-be sites are the dormant calls of codebook/models/bottleneck.py:45,75-77); the row shards and
 * their min + index exchange are this build's.  One RCCL communicator per (process, device), created from a 128-byte
 * unique id the host carries to the ranks once; every call below is stream-ordered on the `stream` it is handed and makes
 * no host round trip, so a sharded step - kernels and collectives - is capturable as ONE hipGraph.  RCCL is bound lazily
 * (dlopen): without it only these entry points fail.
 *   qpg_comm_unique_id        rank 0: id [host] >= 128 bytes (ncclGetUniqueId).
 *   qpg_comm_create           every rank, collectively: the id, its rank, the world size -> *out.
 *   qpg_comm_allgather        recv [dev] world x bytes: block w = rank w's send [dev] (bytes).
 *   qpg_comm_alltoall         send / recv [dev] world blocks of `bytes`: block w goes to / came from rank w (out of place).
 *   qpg_comm_allreduce_max_i32  in place MAX (the agreed trouble word of an all-to-all step).
 *   qpg_allreduce_min_u64     in place MIN of packed (order-preserving f32 distance key << 32 | global candidate index)
 *                             tables: the global per-code winner with first-wins ties (GestureKNN.py:686-689) in one
 *                             collective - for tables whose values decide every comparison (text f32, Levenshtein);
 *                             qpg_pack_min_u64 / qpg_unpack_min_u64 convert (dist f32, idx i32; -1 = absent <-> all ones). */
typedef struct qpg_comm qpg_comm;
int qpg_comm_unique_id(void* id, int64_t id_bytes);
int qpg_comm_create(qpg_ctx*, const void* id, int64_t id_bytes, int rank, int world, qpg_comm** out);
int qpg_comm_destroy(qpg_comm*);
int qpg_comm_allgather(qpg_ctx*, void* stream, qpg_comm*, const void* send, void* recv, int64_t bytes);
int qpg_comm_alltoall(qpg_ctx*, void* stream, qpg_comm*, const void* send, void* recv, int64_t bytes);
int qpg_comm_allreduce_max_i32(qpg_ctx*, void* stream, qpg_comm*, int32_t* buf, int64_t count);
int qpg_allreduce_min_u64(qpg_ctx*, void* stream, qpg_comm*, uint64_t* buf, int64_t count);
int qpg_pack_min_u64(qpg_ctx*, void* stream, const float* dist, const int32_t* idx, int64_t n, uint64_t* packed);
int qpg_unpack_min_u64(qpg_ctx*, void* stream, const uint64_t* packed, int64_t n, float absent, float* dist, int32_t* idx);

/* ------------------------------------------------------------------------------------------
 * Gesture VQ-VAE (codebook/models/{vqvae,encdec,resnet,bottleneck}.py).  Activations are channels-last
 * [B][T][C] f32 — the layout of the pose tensors at VQVAE.encode/decode's API (vqvae.py:132-136 permutes
 * to NCT and back; here nothing is permuted).
 * ---------------------------------------------------------------------------------------- */

/* One 1-D convolution as an implicit GEMM on the f32 matrix cores (exact f32 FMA chains):
 *   y[b][t*out_stride+out_offset][co] = act_out( bias[co] + sum_{tap,ci} w[tap][ci][co] *
 *                                         act_in(x[b][t*in_stride + in_offset + tap*dil][ci]) ) (+ residual)
 * for t < T_out; input rows outside [0,T_in) are zero padding.  Serves nn.Conv1d(k4,s2,p1) (encdec.py:20),
 * the dilated k3 and 1x1 convolutions of ResConv1DBlock with its ReLUs and residual (resnet.py:31-46),
 * nn.Conv1d(k3) (encdec.py:24,39,113), the x.k^T GEMM of BottleneckBlock.quantise (bottleneck.py:123) and
 * nn.ConvTranspose1d(k4,s2,p1) (encdec.py:45) as two 2-tap launches, one per output parity.
 * w: [dev] f32 [taps][Cin_pad][Cout_pad] repacked weights (Cin_pad % 16 == 0, Cout_pad % 128 == 0, zero padded);
 * bias: [dev] f32 [Cout_pad] or NULL; residual: indexed like y, or NULL; y: [dev] f32 [B][T_y][Cout].
 * ws / ws_floats: optional [dev] f32 scratch; when given and the launch would not fill the chip (short sequences),
 * the contraction is split over up to 8 block groups whose partial sums are added in a fixed order (how many: by the
 * shapes and ws_floats, never by what ws holds - contents on entry are ignored). */
int qpg_conv1d_f32(qpg_ctx*, void* stream, const float* x, int B, int T_in, int Cin, const float* w,
                   const float* bias, int taps, int Cin_pad, int Cout, int Cout_pad, int in_stride, int in_offset,
                   int dil, int T_out, int out_stride, int out_offset, int T_y, const float* residual, int relu_in,
                   int relu_out, float* y, float* ws, int64_t ws_floats);

/* The same convolution in the TRANSPOSED formulation (csrc/qpg_convt.hip): y^T = W^T . x^T on v_mfma_f32_16x16x4_f32,
 * a wave owns 16 positions, activations go straight from the channels-last rows to registers, the weights stream
 * through LDS by LDS-DMA from a pre-packed image.  Same argument meaning as qpg_conv1d_f32 except:
 *   x rows have pitch Cx floats (Cx % 4 == 0, Cx >= Cin_pad, 16-byte aligned base): pad 135-channel pose rows
 *   with qpg_pad_channels_f32 first;
 *   wt: [dev] f32 T-pack  wt[nb][kb][g][nl][j] = W[k = 16 kb + 4 g + j][n = 128 nb + nl],  k = tap*Cin_pad + ci,
 *   zero padded, (taps*Cin_pad) % 64 == 0, Cout_pad % 128 == 0. */
int qpg_convt_f32(qpg_ctx*, void* stream, const float* x, int B, int T_in, int Cx, const float* wt, const float* bias,
                  int taps, int Cin_pad, int Cout, int Cout_pad, int in_stride, int in_offset, int dil, int T_out,
                  int out_stride, int out_offset, int T_y, const float* residual, int relu_in, int relu_out, float* y);
/* Two qpg_convt_f32 convolutions of the SAME input and shape whose outputs interleave - the even / odd output frames
 * of ConvTranspose1d(k4, s2, p1) (encdec.py:112-115: y[2m] = x[m-1].W3 + x[m].W1, y[2m+1] = x[m].W2 + x[m+1].W0) -
 * issued together: one launch on short sequences (a clip's decode), two otherwise.  (wt0, bias0, in_offset0,
 * out_offset0) and (wt1, ...) are the two halves; everything else as in qpg_convt_f32, no residual, no ReLU. */
int qpg_convt_pair_f32(qpg_ctx*, void* stream, const float* x, int B, int T_in, int Cx, const float* wt0,
                       const float* bias0, int in_offset0, int out_offset0, const float* wt1, const float* bias1,
                       int in_offset1, int out_offset1, int taps, int Cin_pad, int Cout, int Cout_pad, int in_stride,
                       int dil, int T_out, int out_stride, int T_y, float* y);
/* T-pack of a convolution's weights on the device: w [dev] f32 [taps x Cin_pad][Cout_pad] (qpg_conv1d_f32's layout, the one
 * the optimiser updates) -> out [dev] f32, the wt of qpg_convt_f32 (nb = 128) or one half of qpg_resblock_f32's wpack
 * (nb = 512 for the dilated convolution): taps x Cin_pad x (Cout_pad rounded up to nb) floats. */
int qpg_tpack_f32(qpg_ctx*, void* stream, const float* w, int taps, int Cin_pad, int Cout_pad, int nb, float* out);
/* y[r][0..Cp) = x[r][0..C) zero-extended (rows of 135 floats are not 16-byte aligned). */
int qpg_pad_channels_f32(qpg_ctx*, void* stream, const float* x, int64_t R, int C, int Cp, float* y);
/* One ResConv1DBlock of width 512 in ONE launch (resnet.py:31-46):  y = x + W2 . relu(W1 (*) relu(x) + b1) + b2,
 * W1 the dilated k3 convolution, W2 the 1x1 one; the hidden activation stays in the MFMA accumulators (the C/D
 * register layout of the first GEMM is the B-operand layout of the second).  x, y: [dev] f32 [B][T][512], x != y;
 * wpack: [dev] f32, 96 stages (T-pack NB = 512 of W1, k = tap*512 + ci) then 32 stages (T-pack NB = 128 of W2) of
 * 8192 floats each; b1, b2: [dev] f32 [512]; hidden: optional [dev] f32 [B][T][512] copy of relu(W1(*)relu(x)+b1). */
int qpg_resblock_f32(qpg_ctx*, void* stream, const float* x, int B, int T, int dil, const float* wpack,
                     const float* b1, const float* b2, float* y, float* hidden);

/* BottleneckBlock.quantise (bottleneck.py:120-126) after the GEMM: ids[r] = argmin_c (|z_r|^2 - 2 dot[r][c]) + kk[c]
 * (f32, that operation order, lowest index on ties).  z: [dev] f32 [R][E]; dot: [dev] f32 [R][K]; kk: [dev] f32 [K];
 * ids: [dev] i64 [R]; dmin / dsecond: optional [dev] f32 [R] best and runner-up distance (parity margin). */
int qpg_vq_argmin_f32(qpg_ctx*, void* stream, const float* z, const float* dot, const float* kk, int64_t R, int E,
                      int K, int64_t* ids, float* dmin, float* dsecond);

/* BottleneckBlock.dequantise (bottleneck.py:128-130): out[r][:] = k[ids[r]][:].  status: optional [dev] i32, set to 1
 * if an id is outside [0,K) (torch's F.embedding raises IndexError). */
int qpg_vq_gather_f32(qpg_ctx*, void* stream, const float* k, const int64_t* ids, int64_t R, int E, int K, float* out,
                      int32_t* status);

/* The convolution of qpg_conv1d_f32's contract on the f16 matrix cores with SPLIT operands (round 5, csrc/qpg_conv16.hip):
 * every value is h + l (two f16 numbers; weights pre-scaled by a power of two per layer), a product is three
 * v_mfma_f32_16x16x32_f16 (h l', l h', h h') accumulated in f32 - 3/16 of the f32 matrix time per flop, within ~1e-6
 * (relative to sum |products|) of the f32 FMA chains, NOT bit-identical: the host uses it under a margin check and keeps
 * the f32 kernels as the referee (qpgesture_amd/vqvae.py encode_f16x3; encdec.py:8-51, resnet.py:31-46 are the layers).
 *   qpg_conv16_image_bytes   bytes of the weight image of a (taps, Cin, Cout) layer (Cin counted as the activation rows'
 *                            channel count, a multiple of 8); the i32 at byte (that - 64) is the layer's scale exponent.
 *   qpg_conv16_pack_weights  w [dev] f32 [taps][Cin_pad_w][Cout_pad_w] (qpg_conv1d_f32's layout) -> image [dev].
 *   qpg_conv16_f32           x [dev] f32 [B][T_in][Cx] (Cx %% 8 == 0, Cx >= Cin, Cin %% 8 == 0; 16-byte aligned), geometry
 *                            as qpg_conv1d_f32; y [dev] f32 [B][T_y][Cout]; status [dev] i32 |= 1 if an activation's
 *                            magnitude exceeds the f16 range (the output is then meaningless: redo on the f32 kernels).
 *                            w_exp: the image's scale exponent, or QPG_CONV16_WEXP_FROM_IMAGE - the kernel reads it from the
 *                            image itself (training: the weights change every step, no host read-back per layer). */
#define QPG_CONV16_WEXP_FROM_IMAGE 0x7fff
int64_t qpg_conv16_image_bytes(int taps, int Cin, int Cout);
int qpg_conv16_pack_weights(qpg_ctx*, void* stream, const float* w, int taps, int Cin, int Cin_pad_w, int Cout, int Cout_pad_w,
                            void* image, int64_t image_bytes);
int qpg_conv16_f32(qpg_ctx*, void* stream, const float* x, int B, int T_in, int Cx, int Cin, const void* image, int w_exp,
                   const float* bias, int taps, int Cout, int in_stride, int in_offset, int dil, int T_out, int out_stride,
                   int out_offset, int T_y, const float* residual, int relu_in, int relu_out, float* y, int32_t* status);

/* Whole-network entry points: VQVAE.encode / VQVAE.decode (vqvae.py:152-181) as ONE call each, the layer
 * sequence of encdec.py:53-136 issued from C on the caller's stream (no host round trips between layers).
 * The model is a plain descriptor of repacked device tensors filled by the caller (qpgesture_amd/vqvae.py
 * builds it from the reference checkpoint's state_dict). */
#define QPG_VQ_MAX_DOWN 4
#define QPG_VQ_MAX_DEPTH 4
typedef struct {
  const float* w;    /* [dev] [taps][cin_pad][cout_pad] */
  const float* b;    /* [dev] [cout_pad] or NULL */
  int32_t taps, cin, cin_pad, cout, cout_pad;
  const float* wt;   /* [dev] optional T-pack (NB = 128) of the same weights for qpg_convt_f32, or NULL */
} qpg_conv_desc;
typedef struct {
  int32_t in_dim, width, emb, bins, down_t, depth, growth, reverse_dec;
  qpg_conv_desc enc_down[QPG_VQ_MAX_DOWN];                       /* Conv1d k4 s2 p1              (encdec.py:20) */
  qpg_conv_desc enc_res[QPG_VQ_MAX_DOWN][QPG_VQ_MAX_DEPTH][2];   /* [..][d][0] k3 dilated, [1] 1x1 (resnet.py:31-46) */
  qpg_conv_desc enc_out;                                         /* Conv1d k3                    (encdec.py:24) */
  qpg_conv_desc dec_in;                                          /* Conv1d k3                    (encdec.py:39) */
  qpg_conv_desc dec_res[QPG_VQ_MAX_DOWN][QPG_VQ_MAX_DEPTH][2];
  qpg_conv_desc dec_up_even[QPG_VQ_MAX_DOWN];                    /* ConvTranspose1d k4 s2 p1, output parity 0/1 (encdec.py:45) */
  qpg_conv_desc dec_up_odd[QPG_VQ_MAX_DOWN];
  qpg_conv_desc dec_out;                                         /* Conv1d k3 -> in_dim          (encdec.py:113) */
  qpg_conv_desc kT;                                              /* codebook^T as a 1-tap conv   (bottleneck.py:123) */
  const float* k;                                                /* [dev] [bins][emb] */
  const float* kk;                                               /* [dev] [bins] sum_e k^2 */
  /* optional (width == emb == 512): fused ResConv1DBlock weight images for qpg_resblock_f32, or NULL */
  const float* enc_res_pack[QPG_VQ_MAX_DOWN][QPG_VQ_MAX_DEPTH];
  const float* dec_res_pack[QPG_VQ_MAX_DOWN][QPG_VQ_MAX_DEPTH];
} qpg_vq_model;

/* floats of scratch the two calls below need for a batch of B sequences of T pose frames (contents on entry are ignored) */
int64_t qpg_vq_workspace_floats(const qpg_vq_model* m, int B, int T);
/* x: [dev] f32 [B][T][in_dim] (T %% 2^down_t == 0) -> ids [dev] i64 [B][T/2^down_t]; latent: optional [dev] f32
 * [B][T/2^down_t][emb] (pre-quantisation encoder output); margin: optional [dev] f32 [B][T/2^down_t] runner-up minus best. */
int qpg_vq_encode_f32(qpg_ctx*, void* stream, const qpg_vq_model* m, const float* x, int B, int T, float* ws,
                      int64_t ws_floats, int64_t* ids, float* latent, float* margin);
/* ids: [dev] i64 [B][L] -> out [dev] f32 [B][L*2^down_t][in_dim]; status [dev] i32: 1 if an id was out of range. */
int qpg_vq_decode_f32(qpg_ctx*, void* stream, const qpg_vq_model* m, const int64_t* ids, int B, int L, float* ws,
                      int64_t ws_floats, float* out, int32_t* status);

/* Post-decode pose conversion (VisualizeCodebook.py:148-149 + process/process_bvh.py:57-76): poses [dev]
 * f32 [T][J*9] normalised decoder output (J joints x row-major 3x3) -> de-normalise `p * stdc + mean` (f64; stdc already
 * clipped at 0.01) -> optional Savitzky-Golay smoothing in time (sg_mid [W], sg_head / sg_tail [W/2][W] coefficient tables
 * of scipy.signal.savgol_filter(x, W, 2, mode='interp'); NULL = no smoothing) -> orthogonalise each 3x3 like
 * scipy's Rotation.from_matrix (orthogonal polar factor) -> intrinsic Z-X-Y Euler angles in degrees, euler [dev] f64
 * [T][J*3].  status [dev] i32: raised to 1 if a matrix has a non-positive determinant (scipy raises ValueError). */
int qpg_pose_to_euler_f64(qpg_ctx*, void* stream, const float* poses, int64_t T, int J, const double* mean,
                          const double* stdc, const double* sg_mid, const double* sg_head, const double* sg_tail, int W,
                          double* euler, int32_t* status);

/* ---- Phase extraction: PAE inference (codebook/PAE.py:477-508 pose2phase, Model.forward :99-145 up to `params`) for
 * every frame of many clips in one call.  Model: PAE.Model(135, 8, 240, 13, 4.0) in eval mode.
 *   pose      [dev] f64 [n_total][135] the clips' `upper` rotation channels, concatenated;
 *   clip_off  [dev] i64 [n_clips + 1] clip c is rows clip_off[c] .. clip_off[c+1]-1 (clip_off[0] = 0, clip_off[n_clips] =
 *             n_total, non-decreasing: the caller's invariant); no window ever crosses a clip boundary;
 *   mean, stdc [dev] f64 [135] codebook.yml's data_mean and clip(data_std, 0.01);
 *   params    [dev] f32 [QPG_PAE_PARAM_FLOATS], packed by the host (qpgesture_amd/PAE.py:pack_params):
 *     W1   at QPG_PAE_OFF_W1   [240 taps][34 channel groups][64 lanes] = conv1.weight[o = lane & 15][c = 4 group +
 *          (lane >> 4)][tap] (0 for o = 15, c = 135): the B fragments of v_mfma_f32_16x16x4_f32;
 *     BN1  at QPG_PAE_OFF_BN1  [3][16] conv1.bias, alpha = bn_conv1.weight / sqrt(running_var + 1e-5),
 *          beta = bn_conv1.bias - running_mean * alpha (0 for o = 15): y = tanh((acc + bias) * alpha + beta);
 *     W2   at QPG_PAE_OFF_W2   [240][4][64] = conv2.weight[e = lane & 15][o = 4 group + (lane >> 4)][tap] (0 for e >= 8,
 *          o = 15);   BN2 at QPG_PAE_OFF_BN2 [3][16] as BN1 for conv2 / bn_conv2;
 *     FC   at QPG_PAE_OFF_FC   [8][2][240] fc[e].weight;  FCBN at QPG_PAE_OFF_FCBN [3][16] fc[e].bias, bn[e] alpha,
 *          beta at index 2 e + j;   FREQ at QPG_PAE_OFF_FREQ [120] the model's `freqs`;  TPI at QPG_PAE_OFF_TPI [1].
 * Frames frame0 .. frame0 + n_frames - 1 of the concatenation are computed (n_frames <= QPG_PAE_MAX_CHUNK);
 * out [dev] f32 [n_frames][4][8] = [p, f, a, b] x 8 channels (the reference's (T,4,1,8,1) array); v_out: optional [dev]
 * f32 [n_frames][8][2] the BN'd fc output (x, y) that p is the atan2' of; latent_out: optional [dev] f32
 * [n_frames][8][240].  ws: [dev] f32 scratch of at least (n_frames + 2 QPG_PAE_HALO - 1) * QPG_PAE_WS_STRIDE floats
 * (the f32 velocities of the rows the chunk reads; contents on entry are ignored).  A frame's result does not depend on frame0, n_frames or the
 * other clips (bit-identical however a batch is chunked).  n_frames = 0 is a no-op. */
#define QPG_PAE_CHANNELS 135
#define QPG_PAE_MID 15
#define QPG_PAE_EMBED 8
#define QPG_PAE_TIME 240
#define QPG_PAE_HALO 120
#define QPG_PAE_WS_STRIDE 136
#define QPG_PAE_MAX_CHUNK (1 << 22)
#define QPG_PAE_OFF_W1 0
#define QPG_PAE_OFF_BN1 522240
#define QPG_PAE_OFF_W2 522288
#define QPG_PAE_OFF_BN2 583728
#define QPG_PAE_OFF_FC 583776
#define QPG_PAE_OFF_FCBN 587616
#define QPG_PAE_OFF_FREQ 587664
#define QPG_PAE_OFF_TPI 587784
#define QPG_PAE_PARAM_FLOATS 587792
int qpg_pae_phase_f32(qpg_ctx*, void* stream, const float* params, const double* pose, const double* mean,
                      const double* stdc, const int64_t* clip_off, int n_clips, int64_t n_total, int64_t frame0,
                      int64_t n_frames, float* ws, int64_t ws_floats, float* out, float* v_out, float* latent_out);

/* ---- PAE training (codebook/PAE.py:273-476): one step of Model(135, 8, 240, 13, 4.0) on a batch of windows.
 *   params [dev] f32 [QPG_PAET_PARAM_FLOATS]: every parameter of the model, flat, in named_parameters() order
 *     (row-major torch shapes):  tpi [1] at QPG_PAET_OFF_TPI, args [240] at _ARGS, freqs [120] at _FREQS (these three
 *     are constants: no gradient, no update), conv1.weight (15, 135, 240) at _CONV1_W, conv1.bias [15] at _CONV1_B,
 *     bn_conv1.weight [15] | .bias [15] at _BN1, conv2.weight (8, 15, 240) at _CONV2_W, conv2.bias [8] at _CONV2_B,
 *     bn_conv2.weight [8] | .bias [8] at _BN2, fc.e.weight (2, 240) | fc.e.bias [2] at _FC + 482 e, bn.e.weight [2]
 *     | bn.e.bias [2] at _FCBN + 4 e, deconv1.weight (15, 8, 240) at _DECONV1_W, deconv1.bias [15] at _DECONV1_B,
 *     bn_deconv1.weight [15] | .bias [15] at _BN3, deconv2.weight (135, 15, 240) at _DECONV2_W, deconv2.bias [135]
 *     at _DECONV2_B.  The trainable parameters are the contiguous range from QPG_PAET_TRAINABLE to the end.
 *   grads  [dev] f32, the same layout (entries below QPG_PAET_TRAINABLE are left untouched).
 *   stats  [dev] f32 [QPG_PAET_STATS_FLOATS] BatchNorm running statistics: running_mean | running_var of bn_conv1
 *     at QPG_PAET_ST_BN1 (15 | 15), bn_conv2 at _ST_BN2 (8 | 8), bn.e at _ST_FCBN + 4 e (2 | 2), bn_deconv1 at
 *     _ST_BN3 (15 | 15).  num_batches_tracked is the caller's count of training forwards.
 *   poses  [dev] f32 [n_frames][135]: normalised poses (pose - mean) / clip(std, 0.01) in f64, rounded once, of one
 *     or many clips concatenated;  starts [dev] i64 [batch]: window b is poses[starts[b] .. starts[b] + 239] (the
 *     caller keeps windows inside their clip; a start outside 0 .. n_frames - 240 yields a NaN window).
 *   ws     [dev] f32 scratch of qpg_pae_train_ws_floats(batch) floats, 16-byte aligned; contents on entry to the forward
 *     are ignored.  The forward leaves every activation there for the backward of the same batch; nothing is allocated and nothing waits for the host. */
#define QPG_PAET_OFF_TPI 0
#define QPG_PAET_OFF_ARGS 1
#define QPG_PAET_OFF_FREQS 241
#define QPG_PAET_TRAINABLE 361
#define QPG_PAET_OFF_CONV1_W 361
#define QPG_PAET_OFF_CONV1_B 486361
#define QPG_PAET_OFF_BN1 486376
#define QPG_PAET_OFF_CONV2_W 486406
#define QPG_PAET_OFF_CONV2_B 515206
#define QPG_PAET_OFF_BN2 515214
#define QPG_PAET_OFF_FC 515230
#define QPG_PAET_OFF_FCBN 519086
#define QPG_PAET_OFF_DECONV1_W 519118
#define QPG_PAET_OFF_DECONV1_B 547918
#define QPG_PAET_OFF_BN3 547933
#define QPG_PAET_OFF_DECONV2_W 547963
#define QPG_PAET_OFF_DECONV2_B 1033963
#define QPG_PAET_PARAM_FLOATS 1034098
#define QPG_PAET_ST_BN1 0
#define QPG_PAET_ST_BN2 30
#define QPG_PAET_ST_FCBN 46
#define QPG_PAET_ST_BN3 78
#define QPG_PAET_STATS_FLOATS 108
#define QPG_PAET_MAX_BATCH 65536
#define QPG_PAET_SLABS 16            /* weight gradients: windows split into min(batch, 16) slabs, added in order */
/* floats [host] i64: the scratch floats a batch of 2 .. QPG_PAET_MAX_BATCH windows needs (refused outside). */
int qpg_pae_train_ws_floats(qpg_ctx*, void* stream, int batch, int64_t* floats);
/* Forward of a batch: train = 1 is training mode (zero velocity row first, BatchNorm over the batch, running
 * statistics updated, dL/dy kept in ws for the backward); train = 0 is eval mode (zero row last, the running
 * statistics; nothing is updated).  loss: optional [dev] f64 scalar, 300 * mean((y - x)^2).  batch >= 2. */
int qpg_pae_train_forward_f32(qpg_ctx*, void* stream, const float* params, float* stats, const float* poses,
                              int64_t n_frames, const int64_t* starts, int batch, int train, float* ws,
                              int64_t ws_floats, double* loss);
/* Backward of the last training-mode forward on ws (same params, same batch): every trainable gradient into grads
 * (overwritten, not accumulated). */
int qpg_pae_train_backward_f32(qpg_ctx*, void* stream, const float* params, int batch, float* ws, int64_t ws_floats,
                               float* grads);
/* AdamW of Library/AdamWR/adamw.py on n f32 values: p = p * (1 - weight_decay) (weight decay not scaled by lr), then
 * m = beta1 m + (1 - beta1) g, v = beta2 v + (1 - beta2) g^2, p -= step_size * m / (sqrt(v) + eps) with step_size =
 * lr sqrt(1 - beta2^step) / (1 - beta1^step).  step >= 1 counts this update.  (qpg_adam_step_f32 is torch.optim.Adam.) */
int qpg_pae_adamw_f32(qpg_ctx*, void* stream, float* p, const float* g, float* m, float* v, int64_t n, double lr,
                      double weight_decay, double beta1, double beta2, double eps, int64_t step);

/* ---- VQ-VAE training step (codebook/train.py:120-148): VQVAE.forward's loss terms, the bottleneck statistics,
 * the EMA codebook update, the loss gradient and Adam.  Reductions are ordered two-stage sums in f64
 * (deterministic).  `ws` is a caller-owned scratch of at least qpg_vq_reduce_ws_bytes() bytes; here and in
 * the calls below its contents on entry are ignored. ---- */
int64_t qpg_vq_reduce_ws_bytes(void);

/* vqvae.py:244-267.  x_out, x_target: [dev] f32 [B][T][C].  commit_loss: optional [dev] f32 scalar.
 * out6 [dev] f32 = {loss, recons (L1), regularization, velocity, acceleration, commit} with
 * loss = recons + w_commit*commit + w_reg*regularization + w_vel*velocity + w_acc*acceleration. */
int qpg_vq_loss_f32(qpg_ctx*, void* stream, const float* x_out, const float* x_target, int B, int T, int C,
                    const float* commit_loss, float w_commit, float w_reg, float w_vel, float w_acc, void* ws,
                    int64_t ws_bytes, float* out6);
/* d loss / d x_out of the same terms (what autograd produces for vqvae.py:244-267; sign(0) = 0), times `upstream`. */
int qpg_vq_loss_grad_f32(qpg_ctx*, void* stream, const float* x_out, const float* x_target, int B, int T, int C,
                         float w_reg, float w_vel, float w_acc, float upstream, float* d_x_out);

/* BottleneckBlock.forward statistics (bottleneck.py:96-118, 125, 176): z [dev] f32 [R][E] encoder output rows,
 * zq [dev] f32 [R][E] their dequantised codes (qpg_vq_gather_f32, taken BEFORE the EMA update like :169), dmin
 * optional [dev] f32 [R] (from qpg_vq_argmin_f32).
 * out3 [dev] f32 = {commit_loss = |zq-z|^2/(R E), fit = mean(dmin), prenorm = |z-mean(z)|/sqrt(R E)}. */
int qpg_vq_latent_stats_f32(qpg_ctx*, void* stream, const float* z, const float* zq, const float* dmin, int64_t R,
                            int E, void* ws, int64_t ws_bytes, float* out3);
/* d_z = d_zq (straight-through, bottleneck.py:179; optional) + scale * d commit_loss / d z (zq detached). */
int qpg_vq_commit_grad_f32(qpg_ctx*, void* stream, const float* z, const float* zq, int64_t R, int E, float scale,
                           const float* d_zq, float* d_z);

/* BottleneckBlock.update_k (bottleneck.py:63-94) in two halves so that the caller can all-reduce the batch sums
 * across ranks in between (bottleneck.py:73-75):
 *   qpg_vq_code_sums_f32: batch_sum[c][:] = sum of z rows assigned to c, batch_elem[c] = count (exact).  Order, fixed
 *   and so run-to-run bit-identical: the rows are taken in chunks of 1024; within a chunk a code's rows are added in
 *   ascending row order (f32, from +0), then the partials of the chunks holding rows of the code are added in chunk
 *   order (f32, from +0).  For a code spanning several chunks this is not the plain ascending-row f32 sum;
 *   qpg_vq_ema_update_f32: k_sum/k_elem EMA (mu), k = k_sum/k_elem where k_elem >= threshold else k_rand; also
 *   refreshes kT ([E][ldkT] transposed copy, optional) and kk ([K] squared norms, optional) used by the quantiser,
 *   out4 [dev] f32 = {entropy, used_curr, usage, dk}.  ws: >= K doubles.
 * kk[c] is sum_e k[c][e]^2 accumulated in f64 and rounded once to f32; qpg_vq_code_norms_f32 computes it for a given
 * k (K x E) with exactly the same arithmetic (VQVAE uses it after init_k and when it loads a checkpoint), so such a
 * codebook gets the kk an EMA step would have left. */
int64_t qpg_vq_code_sums_ws_bytes(int64_t R, int E, int K);
int qpg_vq_code_sums_f32(qpg_ctx*, void* stream, const float* z, const int64_t* ids, int64_t R, int E, int K,
                         float* batch_sum, float* batch_elem, void* ws, int64_t ws_bytes);
int qpg_vq_ema_update_f32(qpg_ctx*, void* stream, float* k, float* k_sum, float* k_elem, const float* batch_sum,
                          const float* batch_elem, const float* k_rand, float mu, float threshold, int K, int E,
                          float* kT, int ldkT, float* kk, void* ws, int64_t ws_bytes, float* out4);
int qpg_vq_code_norms_f32(qpg_ctx*, void* stream, const float* k, int K, int E, float* kk);

/* torch.optim.Adam single step as train.py:71 configures it (no weight decay / amsgrad), over a flat buffer. */
int qpg_adam_step_f32(qpg_ctx*, void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                      int64_t n, float lr, float beta1, float beta2, float eps, int64_t step);

/* Backward of the convolution layers (what autograd computes for nn.Conv1d / nn.ConvTranspose1d in
 * encdec.py:20-45,113 and resnet.py:31-46), on the same channels-last activations and packed weights.
 *
 * qpg_conv1d_bwd_data_f32: dx = conv(dy, W^T) with the forward layer's packed weights read in place.
 *   dy [dev] f32 [B][T_in][C_dy] (C_dy = the forward layer's Cout); w_fwd [taps_fwd][fwd_Cin_pad][fwd_Cout_pad];
 *   input tap j of THIS convolution uses weight tap tap_base + j*tap_step (a stride-1 layer: taps, base taps-1,
 *   step -1; the strided down-convolution: one call per output parity with 2 taps, base 3 / 2, step -2; the
 *   transposed convolution's parity sets: base 1, step -1, dilation 2).  Geometry arguments as qpg_conv1d_f32.
 *   gate: optional, indexed like dx — result zeroed where gate <= 0 (the ReLU in front of the forward layer);
 *   residual: optional, added after the gate (skip connection / accumulation of a second parity set).
 * qpg_conv1d_bwd_weight_f32: dw [taps][Cin_pad][Cout_pad] (packed like the weights, fully overwritten) and
 *   db [Cout_pad] (optional; accumulate_bias != 0 adds to it: the two parity sets of a transposed convolution
 *   share one bias) from the layer input x (relu_in as in the forward call) and dy.  The position axis is
 *   split over thread blocks; ws holds the partial sums (qpg_conv1d_wgrad_ws_floats(taps,Cin_pad,Cout_pad,splits)
 *   floats for `splits` partials; more workspace = more parallelism, 1 partial is the minimum; contents on entry are
 *   ignored, here and in qpg_conv1d_bwd_data_f32's split-K scratch). */
int qpg_conv1d_bwd_data_f32(qpg_ctx*, void* stream, const float* dy, int B, int T_in, int C_dy, const float* w_fwd,
                            int taps, int fwd_Cin, int fwd_Cin_pad, int fwd_Cout_pad, int tap_base, int tap_step,
                            int in_stride, int in_offset, int dil, int T_out, int out_stride, int out_offset, int T_y,
                            const float* gate, const float* residual, float* dx, float* ws, int64_t ws_floats);
int64_t qpg_conv1d_wgrad_ws_floats(int taps, int Cin_pad, int Cout_pad, int splits);
int qpg_conv1d_bwd_weight_f32(qpg_ctx*, void* stream, const float* x, int B, int T_in, int Cin, const float* dy,
                              int taps, int Cin_pad, int Cout, int Cout_pad, int in_stride, int in_offset, int dil,
                              int T_out, int out_stride, int out_offset, int T_y, int relu_in, float* dw, float* db,
                              int accumulate_bias, float* ws, int64_t ws_floats);

/* ---- WavLM feature extraction (process/WavLM/WavLM.py extract_features, inference, no masks): the stage kernels that
 * qpgesture_amd/wavlm.py chains.  All arrays [dev] f32, activations channels-last rows [B][T][C]; every matrix product is
 * a k-ordered f32 FMA chain on the f32 matrix cores, so no result depends on the batch it is computed in.  Supported:
 * extractor_mode "layer_norm", layer_norm_first, gelu, gated relative-position bias, head dim QPG_WAVLM_HEAD_DIM, at
 * most QPG_WAVLM_MAX_FRAMES frames per window in the transformer. ---- */
#define QPG_WAVLM_HEAD_DIM 64
#define QPG_WAVLM_MAX_FRAMES 256

/* Output frames of an unpadded Conv1d: (t_in - k) / s + 1, 0 if t_in < k. */
int64_t qpg_wavlm_conv_frames(int64_t t_in, int k, int s);

/* Layer 0 of the conv feature extractor (WavLM.py:400-403, Conv1d(1, C, k, stride s)): wav [B][n] raw samples,
 * w [C][k], bias [C] or NULL; out [B][T0][C], T0 = qpg_wavlm_conv_frames(n, k, s), before the layer's norm. */
int qpg_wavlm_conv0_f32(qpg_ctx*, void* stream, const float* wav, int B, int64_t n, const float* w, const float* bias,
                        int C, int k, int s, float* out);

/* LayerNorm over each of M rows of C (biased variance of the centred values, eps inside the root), times gamma plus
 * beta, then the exact (erf) GELU if gelu != 0.  y may be x. */
int qpg_wavlm_layernorm_f32(qpg_ctx*, void* stream, const float* x, const float* gamma, const float* beta, int64_t M,
                            int C, float eps, int gelu, float* y);

/* The one GEMM of the model, batched over z = (outer o, inner i), o < n_outer, i < n_inner:
 *   out_z[m][n] = f(sum_k A_z[m][k] W_i[n][k] + bias_i[n]) + residual_z[m][n],   m < M, n < N, f = GELU if gelu != 0
 * A_z = A + o a_outer + i a_inner with row stride lda (rows may overlap: a strided convolution over channels-last input
 * is this with lda = stride * C and K = taps * C), W_i = W + i w_inner rows of K, bias_i = bias + i bias_inner (NULL: no
 * bias), out_z = out + o c_outer + i c_inner with row stride ldc; residual (NULL: none) is laid out like out and may be
 * out.  The sum over k is taken in chains of 512 products whose results are added in k order.  K must be a multiple of
 * 16 (QPG_EUNSUP otherwise); A, W 16-byte aligned, their strides multiples of 4 floats. */
int qpg_wavlm_gemm_f32(qpg_ctx*, void* stream, const float* A, int64_t lda, const float* W, const float* bias,
                       const float* residual, float* out, int64_t ldc, int M, int N, int K, int gelu, int n_outer,
                       int n_inner, int64_t a_outer, int64_t a_inner, int64_t w_inner, int64_t bias_inner, int64_t c_outer,
                       int64_t c_inner);

/* Input image of pos_conv (WavLM.py:514-527: grouped Conv1d, padding taps / 2, an even kernel's last frame dropped):
 * padded [B][groups][T + taps - 1][D / groups], row r of group g = x[b][r - taps / 2][g D / groups ..], zero outside the
 * clip.  Output frame t of a group is then the GEMM row that starts at its row t (lda = D / groups, K = taps D / groups). */
int qpg_wavlm_pos_pad_f32(qpg_ctx*, void* stream, const float* x, int B, int T, int D, int groups, int taps,
                          float* padded);

/* Gated relative-position factor (modules.py:523-533): x_ln [M][H][64] the layer-normed block input, grep_w [8][64],
 * grep_b [8], grep_a [H]; gate [M][H] = a (b grep_a[h] - 1) + 2 with a, b = sigmoid of the sums of outputs 0..3, 4..7. */
int qpg_wavlm_gate_f32(qpg_ctx*, void* stream, const float* x_ln, const float* grep_w, const float* grep_b,
                       const float* grep_a, int64_t M, int H, float* gate);

/* Self-attention of one block: qkv [B T][3 H 64] (q | k | v, q already scaled by 64^-0.5), gate [B T][H], relb
 * [2T - 1][H] the position-bias table (entry k - q + T - 1: bias of key k seen from query q), out [B T][H 64] =
 * softmax_k(q k^T + gate[q] relb[k - q]) v per (batch, head), the row maximum subtracted before exp.  The (T, T) scores
 * live in LDS only.  T > QPG_WAVLM_MAX_FRAMES: QPG_EUNSUP, nothing launched. */
int qpg_wavlm_attention_f32(qpg_ctx*, void* stream, const float* qkv, const float* gate, const float* relb, int B, int T,
                            int H, float* out);

/* x[m][0 .. C) = 0 for every row m < M with row_mask[m] != 0 ([dev] uint8 [M]); the other rows are not written.  The
 * reference's `x[padding_mask] = 0` ahead of pos_conv (WavLM.py:574-575). */
int qpg_wavlm_mask_rows_f32(qpg_ctx*, void* stream, float* x, const uint8_t* row_mask, int64_t M, int C);

/* The same attention for long and for ragged inputs: the operands of qpg_wavlm_attention_f32 plus key_mask, [dev] uint8
 * [B][T] (nonzero: the key is excluded for every query of its batch member) or NULL (no key excluded).  A block owns 128
 * queries of one (batch, head) and walks the keys in tiles of 64: both products run on the f32 matrix cores, the softmax
 * is online (running maximum; numerator and sum rescaled per key tile), and per tile pair only the 191 table entries it
 * can address are staged, so neither LDS nor registers grow with T.  A masked key contributes nothing: the result is
 * bit-identical whatever qkv holds at masked keys (NaN and Inf included).  Rows of masked QUERIES are computed like any
 * other.  The caller guarantees at least one valid key per batch member (a member without one gets NaN rows).
 * 1 <= T <= QPG_WAVLM_MAX_FRAMES_LONG, above it QPG_EUNSUP with nothing launched. */
#define QPG_WAVLM_MAX_FRAMES_LONG 32768
int qpg_wavlm_attention_tiled_f32(qpg_ctx*, void* stream, const float* qkv, const float* gate, const float* relb,
                                  const uint8_t* key_mask, int B, int T, int H, float* out);

/* ---- Sentence embeddings (a BERT-shaped post-LN encoder as sentence-transformers wraps it, inference): the three kernels
 * qpgesture_amd/sentence.py chains with qpg_wavlm_gemm_f32 and qpg_wavlm_layernorm_f32.  Activations are PACKED RAGGED
 * ROWS: sentence s < S owns the token rows seq_start[s] .. seq_start[s + 1] of an [R][D] f32 array, seq_start [dev] i32
 * [S + 1] with seq_start[0] = 0 and seq_start[S] = R; nothing is padded, nothing is masked.  max_len is the caller's
 * statement of the longest sentence; it sizes the launch and is what the host-side checks see.  What the device arrays
 * hold is never trusted for an address: sentence bounds that are not 0 <= start < end <= R with end - start <= max_len,
 * an id outside [0, vocab) and a position >= max_pos OR a bit into *err ([dev] i32, zeroed by the caller, read when it
 * synchronises) and the rows concerned are not written.  A sentence's result does not depend on which other sentences
 * share the launch. ---- */
#define QPG_BERT_HEAD_DIM 32
#define QPG_BERT_MAX_TOKENS 128
#define QPG_BERT_ERR_SEQ 1 /* *err bit: seq_start does not describe rows inside [0, R) of at most max_len each */
#define QPG_BERT_ERR_ID 2  /* *err bit: an id outside [0, vocab)                                                */
#define QPG_BERT_ERR_POS 4 /* *err bit: a token position >= max_pos                                             */

/* x[r] = LayerNorm((word[ids[r]] + type0) + pos[r - seq_start[s(r)]]) gamma + beta (biased variance of the centred values,
 * eps inside the root): ids [dev] i32 [R], word [vocab][D], pos [max_pos][D], type0 [D] (token type 0's row), x [R][D].
 * max_len > max_pos: QPG_EINVAL, nothing launched. */
int qpg_bert_embed_ln_f32(qpg_ctx*, void* stream, const int32_t* ids, const int32_t* seq_start, int S, int64_t R,
                          int max_len, const float* word, int vocab, const float* pos, int max_pos, const float* type0,
                          const float* gamma, const float* beta, int D, float eps, float* x, int32_t* err);

/* Self-attention of one block: qkv [R][3 H 32] (q | k | v, q already scaled by 32^-0.5), out [R][H 32] = softmax_k(q k^T) v
 * per (sentence, head) over the sentence's own rows, the running maximum subtracted before exp, the sum over the keys taken
 * in key order for every query.  max_len > QPG_BERT_MAX_TOKENS: QPG_EUNSUP, nothing launched.  qkv, out 16-byte aligned. */
int qpg_bert_attention_f32(qpg_ctx*, void* stream, const float* qkv, const int32_t* seq_start, int S, int64_t R, int max_len,
                           int H, float* out, int32_t* err);

/* out[s] = (sum of x[r] over the rows of sentence s, in token order) / (their number): x [R][D], out [S][D]. */
int qpg_bert_mean_pool_f32(qpg_ctx*, void* stream, const float* x, const int32_t* seq_start, int S, int64_t R, int max_len,
                           int D, float* out, int32_t* err);

/* ---- The GRU speech-to-code generator (codebook/generate/generate.py Generator_gru, inference): the stage kernels that
 * qpgesture_amd/generate.py chains with qpg_wavlm_gemm_f32.  All arrays [dev] f32 unless stated, activations
 * channels-last rows [B][T][C].  No launch of this section synchronises between blocks. ---- */
#define QPG_GEN_TAPS 16            /* taps of every convolution of the WavEncoder                          */
#define QPG_GEN_HIDDEN 200         /* the GRU's hidden width: the only one the recurrence kernel is built for */
#define QPG_GEN_GRU_BATCH_TILE 16  /* sequences one recurrence block owns                                  */
#define QPG_GEN_CONV_TIME_TILE 128 /* output frames one convolution block owns (Cin > 1)                   */
#define QPG_GEN_HEAD_LD 208        /* row stride of qpg_gen_head_ln_f32's output (QPG_GEN_HIDDEN padded to 16) */

/* Output frames of an unpadded 16-tap Conv1d: (t_in - 16) / stride + 1, 0 if t_in < 16. */
int64_t qpg_gen_conv_frames(int64_t t_in, int stride);

/* Conv1d(Cin, Cout, 16, stride), no padding, with an optional epilogue:
 *   out[b][t][co] = act(bn(bias[co] + sum_{j < 16, ci < Cin} w[co][j][ci] x[b][stride t + j][ci])),  t < T =
 *   qpg_gen_conv_frames(Tin, stride)
 * x [B][Tin][Cin] (Cin == 1: the raw samples [B][Tin]); w [Cout][16][Cin] - torch's [Cout][Cin][16] with the last two
 * axes swapped; bias [Cout] or NULL; bn [4][Cout] = BatchNorm1d's weight, bias, running_mean, running_var, applied as
 * (v - mean) / sqrt(var + eps) * weight + bias, or NULL (no BatchNorm); act != 0: LeakyReLU, v < 0 -> slope v; out
 * [B][T][Cout].  The (Tin - 16) % stride trailing input frames that no output window covers are never read.  Cin == 1 runs
 * on the VALU (Cout a multiple of 8, <= 64); Cin a multiple of 4 is an implicit GEMM with K = 16 Cin on the f32 matrix
 * cores (Cout a multiple of 16, <= 64); anything else QPG_EUNSUP, nothing launched.  w, out and, with Cin > 1, x 16-byte aligned. */
int qpg_gen_conv1d_f32(qpg_ctx*, void* stream, const float* x, int B, int64_t Tin, int Cin, const float* w,
                       const float* bias, const float* bn, float eps, int act, float slope, int Cout, int stride, float* out);

/* The recurrence of one bidirectional GRU layer (torch.nn.GRU, h0 = 0, gate order r, z, n):
 *   xp  [B][T][2][3 H]  W_ih x + b_ih of direction 0 | direction 1 (one qpg_wavlm_gemm_f32 with N = 6 H),
 *   whh [2][3 H][H], bhh [2][3 H],
 *   out [B][T][2 H]     h_t of direction 0 | direction 1; direction 1 walks t = T - 1 .. 0.
 *   r = s(xp_r + (W_hr h + b_hr)), z = s(xp_z + (W_hz h + b_hz)), n = tanh(xp_n + r (W_hn h + b_hn)), h' = (1 - z) n + z h.
 * One block owns QPG_GEN_GRU_BATCH_TILE sequences of one direction for all T steps (h in LDS, W_hh streamed from L2 per
 * step); a sequence's output bits depend neither on B nor on its position in the batch, and the two directions run the
 * same instructions.  H != QPG_GEN_HIDDEN: QPG_EUNSUP, nothing launched.  All pointers 16-byte aligned. */
int qpg_gen_gru_layer_f32(qpg_ctx*, void* stream, const float* xp, const float* whh, const float* bhh, int B, int T, int H,
                          float* out);

/* The head's first half: y[r][0 .. H) = LayerNorm(x[r][0 .. H) + x[r][H .. 2 H)) gamma + beta (biased variance of the
 * centred values, eps inside the root), y[r][H .. QPG_GEN_HEAD_LD) = 0.  x [R][2 H] (a GRU layer's output), y
 * [R][QPG_GEN_HEAD_LD]: the A operand of the head's qpg_wavlm_gemm_f32 against out.weight padded to the same stride.
 * H != QPG_GEN_HIDDEN: QPG_EUNSUP. */
int qpg_gen_head_ln_f32(qpg_ctx*, void* stream, const float* x, const float* gamma, const float* beta, int64_t R, int H,
                        float eps, float* y);

/* codes[r] = argmax_c logits[r][c]: logits [R][N], codes [dev] i64 [R].  ON EXACT TIES THE LOWEST INDEX WINS (a row of
 * equal values gives 0).  Rows are assumed NaN-free. */
int qpg_gen_argmax_f32(qpg_ctx*, void* stream, const float* logits, int64_t R, int N, int64_t* codes);

/* loss[0] = mean_r (log sum_c exp(logits[r][c]) - logits[r][target[r]]), F.cross_entropy's default reduction: logits
 * [R][N], target [dev] i64 [R], loss [dev] f32 [1].  The row terms are f32 (the row maximum subtracted before exp), their
 * mean is accumulated in f64 in a fixed order.  A target outside [0, N) is not used as an index: its row term, and so the
 * loss, is NaN.  ws: [dev] f32 scratch of R floats (the row terms); contents on entry are ignored. */
int qpg_gen_cross_entropy_f32(qpg_ctx*, void* stream, const float* logits, const int64_t* target, int64_t R, int N,
                              float* ws, float* loss);

/* ---- Training of the same generator (codebook/end2end.py): the stage kernels that qpgesture_amd/end2end.py chains with
 * qpg_gen_conv1d_f32 (bn = NULL, act = 0: the training forward's convolutions), qpg_wavlm_gemm_f32 (input projections,
 * head, and every data gradient of a Linear against a transposed weight copy), qpg_gen_head_ln_f32,
 * qpg_gen_cross_entropy_f32 and qpg_adam_step_f32.  All arrays [dev] f32 unless stated, activations channels-last rows,
 * weights in the layouts of the section above.  Every sum over rows is two-stage and fixed-order: f32 or f64 partials
 * per block or slab, added in block / slab order in f64, so two runs from the same state are bit-identical; there are no
 * global atomics and no launch waits on another block.  Workspaces are caller-owned, their contents on entry are ignored.
 * Gradients are overwritten, not accumulated. ---- */
#define QPG_GEN_TRAIN_MAX_SLABS 1024    /* most row slabs a weight gradient is split into                                */
#define QPG_GEN_TRAIN_SLAB_MIN_ROWS 64  /* no slab is planned smaller than this (a single slab may be)                   */
#define QPG_GEN_BN_MAX_BLOCKS 1024      /* most partials of a BatchNorm sum; a block takes 1024 / C rows per pass        */
#define QPG_GEN_GRU_SAVED 4             /* planes the training recurrence saves per (b, t, direction): r, z, n, W_hn h + b_hn */

/* BatchNorm1d in train() mode over [R][C] rows (R = B T_i), C in {8, 16, 32, 64} (else QPG_EUNSUP), R >= 2.
 * qpg_gen_bn_stats_f32: stat [2][C] = the batch mean and the BIASED variance per channel, both from f64 sums of x and
 *   x^2 (block b owns the row groups b, b + blocks, .. of 1024 / C rows; blocks = min(groups, QPG_GEN_BN_MAX_BLOCKS)).
 *   running_mean / running_var (each optional): r = (1 - momentum) r + momentum v with v the mean, resp. the UNBIASED
 *   variance var R / (R - 1).
 * qpg_gen_bn_apply_f32: y = leaky((x - mean) / sqrt(var + eps) * gamma + beta), v <= 0 -> slope v.  y may be x.
 * qpg_gen_bn_backward_f32: with dyh = dy where y > 0, slope dy where y <= 0 (y: the forward's OUTPUT; at exactly 0 the
 *   slope, as torch does), xhat = (x - mean) / sigma: dbeta = sum dyh, dgamma = sum dyh xhat, dx = (gamma / sigma) (dyh -
 *   mean(dyh) - xhat mean(dyh xhat)).  x is the forward's input, stat what qpg_gen_bn_stats_f32 wrote.  dx may be dy.
 * ws: 8-byte aligned, at least qpg_gen_bn_ws_floats(R, C) floats (it holds f64 partials); x, y, dy, dx 16-byte aligned. */
int64_t qpg_gen_bn_ws_floats(int64_t R, int C);
int qpg_gen_bn_stats_f32(qpg_ctx*, void* stream, const float* x, int64_t R, int C, float* ws, int64_t ws_floats, float* stat,
                         float* running_mean, float* running_var, float momentum);
int qpg_gen_bn_apply_f32(qpg_ctx*, void* stream, const float* x, int64_t R, int C, const float* stat, const float* gamma,
                         const float* beta, float eps, float slope, float* y);
int qpg_gen_bn_backward_f32(qpg_ctx*, void* stream, const float* x, const float* y, const float* dy, int64_t R, int C,
                            const float* stat, const float* gamma, float eps, float slope, float* ws, int64_t ws_floats,
                            float* dgamma, float* dbeta, float* dx);

/* Data gradient of qpg_gen_conv1d_f32's convolution, a gather:
 *   dx[b][s][ci] = sum over t with 0 <= s - stride t < 16, t < T, and co of dy[b][t][co] w[co][s - stride t][ci]
 * dy [B][T][Cout], T = qpg_gen_conv_frames(Tin, stride), w the forward's [Cout][16][Cin], dx [B][Tin][Cin].  EVERY frame
 * of dx is written: the (Tin - 16) % stride trailing frames that no window covers get exactly 0.  Cin in {8, 16, 32, 64},
 * Cout a multiple of 16 up to 64, stride 3 or 6; anything else QPG_EUNSUP.  dy, w, dx 16-byte aligned. */
int qpg_gen_conv1d_bwd_data_f32(qpg_ctx*, void* stream, const float* dy, int B, int64_t Tin, int Cin, const float* w,
                                int Cout, int stride, float* dx);

/* Weight and bias gradient of the same convolution: dw [Cout][16][Cin] (the forward's layout), db [Cout] from the layer
 * input x [B][Tin][Cin] and dy [B][T][Cout] (16-byte aligned).  Cin == 1 runs on the VALU (a thread owns every 256th row
 * of a slab and all 8 x 16 sums of a channel group, the block's threads are added in f64 in thread order);
 * Cin a multiple of 4 is an implicit GEMM on the f32 matrix cores with the contraction over the (b, t) rows of 16 Cin
 * contiguous floats, as the forward reads them; db is the product with a column of ones.  The B T rows are split into
 * slabs - as many as ws holds (ws_floats / (Cout 16 Cin + Cout)), at most QPG_GEN_TRAIN_MAX_SLABS, none under
 * QPG_GEN_TRAIN_SLAB_MIN_ROWS rows - whose partials are added in slab order in f64.  The uncovered trailing input
 * frames are never read.  Shapes as qpg_gen_conv1d_f32, else QPG_EUNSUP. */
int64_t qpg_gen_conv1d_wgrad_ws_floats(int Cin, int Cout, int slabs);
int qpg_gen_conv1d_bwd_weight_f32(qpg_ctx*, void* stream, const float* x, int B, int64_t Tin, int Cin, const float* dy,
                                  int Cout, int stride, float* dw, float* db, float* ws, int64_t ws_floats);

/* Weight gradient of a Linear, the same matrix-core kernel over plain rows:
 *   dW[n][k] = sum_r dY[r][n] X[r + shift][k],  db[n] = sum_r dY[r][n]   (db optional),  n < N, k < K
 * dY rows of ldy, X rows of ldx floats, dW [N][K] contiguous.  shift in {-1, 0, 1} with the period T: row r = (b, t), t =
 * r % T, pairs with X's row (b, t + shift), and with a ZERO row when t + shift leaves [0, T) - the recurrence's W_hh
 * gradient pairs dgh of step t with h of the previous step of its direction and never reaches across a batch member; db
 * takes every row regardless.  With shift == 0, T is ignored.  Slabs and ws as above with qpg_gen_rowgrad_ws_floats(N,
 * K, slabs).  N, K <= 4096. */
int64_t qpg_gen_rowgrad_ws_floats(int N, int K, int slabs);
int qpg_gen_rowgrad_f32(qpg_ctx*, void* stream, const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t R, int N,
                        int K, int shift, int64_t T, float* dW, float* db, float* ws, int64_t ws_floats);

/* qpg_gen_gru_layer_f32 for training: the same recurrence, instruction for instruction (out is bit-equal), that also
 * leaves saved [B][T][2][QPG_GEN_GRU_SAVED][H] = r, z, n and W_hn h + b_hn per (b, t, direction, unit). */
int qpg_gen_gru_layer_train_f32(qpg_ctx*, void* stream, const float* xp, const float* whh, const float* bhh, int B, int T,
                                int H, float* out, float* saved);

/* Backpropagation through time of one bidirectional layer.  dout [B][T][2 H] the gradient at the layer's output, saved
 * and out what qpg_gen_gru_layer_train_f32 left, whhT [2][H][3 H] the transposed W_hh per direction;
 *   dxp [B][T][2][3 H]  the gradient at the input projection xp (gates r, z, n),
 *   dgh [B][T][2][3 H]  the gradient at W_hh h + b_hh (it differs from dxp in the n gate: times r).
 * The forward's ownership: one block owns QPG_GEN_GRU_BATCH_TILE sequences of one direction and walks its steps in
 * reverse; a lane keeps dh of its 4 units of one sequence in registers, the step's dgh goes through LDS into the
 * product W_hh^T dgh on the matrix cores (a column is one sequence, so a sequence's bits depend neither on B nor on its
 * position).  The weight gradients are NOT accumulated here: they are qpg_gen_rowgrad_f32 over dxp (W_ih, b_ih) and
 * over dgh with shift -1 / +1 (W_hh, b_hh of direction 0 / 1).  H != QPG_GEN_HIDDEN: QPG_EUNSUP.  All pointers 16-byte
 * aligned. */
int qpg_gen_gru_layer_backward_f32(qpg_ctx*, void* stream, const float* dout, const float* saved, const float* out,
                                   const float* whhT, int B, int T, int H, float* dxp, float* dgh);

/* Backward of qpg_gen_head_ln_f32: dy [R][QPG_GEN_HEAD_LD] (columns >= H ignored), x [R][2 H] the forward's input; dx
 * [R][2 H] gets the LayerNorm's input gradient in BOTH halves (the direction sum), dgamma [H] and dbeta [H] - which must
 * be dgamma + H - the row sums of dy xhat and dy (slab partials from f64 accumulators, added in f64).  ws: at least
 * qpg_gen_head_ln_bwd_ws_floats(R) floats for full parallelism, 2 H at the least. */
int64_t qpg_gen_head_ln_bwd_ws_floats(int64_t R);
int qpg_gen_head_ln_backward_f32(qpg_ctx*, void* stream, const float* dy, const float* x, const float* gamma, int64_t R,
                                 int H, float eps, float* ws, int64_t ws_floats, float* dgamma, float* dbeta, float* dx);

/* Backward of qpg_gen_cross_entropy_f32: dlogits[r][c] = (softmax(logits[r])[c] - (c == target[r])) / R. */
int qpg_gen_cross_entropy_backward_f32(qpg_ctx*, void* stream, const float* logits, const int64_t* target, int64_t R, int N,
                                       float* dlogits);

/* Inverted dropout on a given mask: y[e] = mask[e] ? x[e] * scale : 0, mask [dev] uint8 [n], scale = 1 / (1 - p).  The
 * backward is the same call on the gradient.  y may be x. */
int qpg_gen_dropout_f32(qpg_ctx*, void* stream, const float* x, const uint8_t* mask, int64_t n, float scale, float* y);

/* ---- vq-wav2vec code extraction (fairseq's Wav2VecModel.feature_extractor and GumbelVectorQuantizer.forward_idx in eval
 * mode): what qpgesture_amd/wavvq.py chains with qpg_wavlm_conv0_f32 (layer 0) and qpg_wavlm_gemm_f32 (every later
 * convolution, lda = stride C, K = taps C, n_outer = B; both Linears of the quantiser).  All arrays [dev] f32 unless
 * stated, activations channels-last rows [B][T][C]. ---- */
#define QPG_WAVVQ_GN_SLAB 4096     /* floats of a window one block of the GroupNorm's passes owns */
#define QPG_WAVVQ_EPI_NONE 0       /* qpg_wavvq_groupnorm_f32's epilogue: none                    */
#define QPG_WAVVQ_EPI_RELU 1       /*   max(v, 0)                                                 */
#define QPG_WAVVQ_EPI_RELU_LOG 2   /*   log(|max(v, 0)| + 1): the feature extractor's last layer  */

/* GroupNorm(1, C) per window, in place: with mean and the BIASED variance over all T C values of window b,
 *   x[b][t][c] = epilogue((x[b][t][c] - mean_b) / sqrt(var_b + eps) * gamma[c] + beta[c])
 * gamma, beta [C] or NULL (1, resp. 0: a non-affine norm).  Three launches over slabs of QPG_WAVVQ_GN_SLAB consecutive
 * floats of a window: f64 (sum, sum of squares) per slab into ws, the slabs of a window added in slab order in f64 (mean
 * and variance from the f64 sums, so a mean far above the standard deviation does not cancel the variance; a constant
 * window has variance 0 and comes out as beta), then the apply pass.  The activations are read twice and written once.
 * A window's result depends neither on B nor on its position in the batch; no atomics.  C must be a multiple of 4
 * (QPG_EUNSUP otherwise, nothing launched); x, gamma, beta 16-byte aligned.
 * ws: 8-byte aligned, at least qpg_wavvq_groupnorm_ws_floats(B, T, C) floats (QPG_EINVAL below that, nothing launched);
 * contents on entry are ignored. */
int64_t qpg_wavvq_groupnorm_ws_floats(int B, int64_t T, int C);
int qpg_wavvq_groupnorm_f32(qpg_ctx*, void* stream, float* x, int B, int64_t T, int C, const float* gamma,
                            const float* beta, float eps, int epilogue, float* ws, int64_t ws_floats);

/* x[e] = max(x[e], 0) for e < n, in place: the ReLU between the two Linears of the quantiser's weight_proj (their biases
 * are the GEMM's).  n a multiple of 4 (QPG_EUNSUP otherwise), x 16-byte aligned. */
int qpg_wavvq_relu_f32(qpg_ctx*, void* stream, float* x, int64_t n);

/* codes[r][g] = argmax_v logits[r][g][v]: logits [R][G][V], codes [dev] i64 [R][G] - forward_idx's indices.  ON EXACT TIES
 * THE LOWEST INDEX WINS, as torch.max does (a group of equal values gives 0).  It is qpg_gen_argmax_f32 over the
 * [R G][V] view of the logits.  Rows are assumed NaN-free. */
int qpg_wavvq_group_argmax_f32(qpg_ctx*, void* stream, const float* logits, int64_t R, int G, int V, int64_t* codes);

/* ---- BVH ingestion (process/beat_data_to_lmdb.py:21-88 process_bvh(modetype='rotation'); qpgesture_amd/process_bvh.py):
 * motion text -> channel table -> the `upper` rotation features, and the data_mean / data_std column statistics.  All f64,
 * no atomics, every sum in a fixed order. ---- */
#define QPG_BVH_BLOCK_BYTES 4096        /* bytes of text one block of the parse kernels owns                          */
#define QPG_BVH_MAX_TOKEN 1024          /* a longer run of non-whitespace bytes counts as a byte that fits no token   */
#define QPG_BVH_INFO_TOKENS 0           /* info[]: tokens in the whole text                                           */
#define QPG_BVH_INFO_FALLBACK 1         /*         fallback tokens among the first n_values (may exceed fb_cap)       */
#define QPG_BVH_INFO_STATUS 2           /*         OR of the QPG_BVH_ST_* bits, 0 = the values are complete           */
#define QPG_BVH_ST_BADBYTE 1            /* one of the first n_values tokens does not fit the grammar                  */
#define QPG_BVH_ST_SHORT 2              /* the text holds fewer than n_values tokens                                  */
#define QPG_BVH_ST_OVERFLOW 4           /* more fallback tokens than fb_cap: fb_list holds the first fb_cap only      */
#define QPG_BVH_PLACEHOLDER_BITS 0x7ff8000000627668      /* value slot of a fallback or bad token: a quiet NaN ("bvh") */

/* The motion block of a BVH file (the bytes after the `Frame Time:` line), parsed on the device.
 *   text     [dev] u8 [n_bytes], 16-byte aligned.  Whitespace is space, tab, CR, LF; a token starts at a non-whitespace byte
 *            that follows whitespace or the start of the text and runs to the next whitespace byte or the end.  Newlines
 *            carry no meaning: like pymo, the first n_values tokens are the values in sequence, the rest is ignored (it is
 *            counted, not parsed).  No byte at or past n_bytes is read.
 *   values   [dev] f64 [n_values]: values[t] = token t, for t < min(n_values, info[TOKENS]); later slots are not written.
 *            Grammar  [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?.  A token whose significant digits are an
 *            integer m <= 2^53 (at most 19 digits read) and whose net decimal exponent k is in [-22, 22] is m * 10^k or
 *            m / 10^k: one correctly rounded operation on exact operands, the value strtod and Python's float() return;
 *            the sign is applied by negation ("-0.000000" is -0.0).  Every other well-formed token is a FALLBACK token:
 *            its slot holds QPG_BVH_PLACEHOLDER_BITS and it is listed for the host to parse.
 *   fb_list  [dev] i64 [fb_cap][2]: (token index, byte offset of its first byte) of the fallback tokens, in token order;
 *            rows info[FALLBACK] .. fb_cap - 1 are not written.
 *   info     [dev] i64 [3], see QPG_BVH_INFO_*; every entry is written by every call.
 *   ws       [dev] 8-byte aligned, at least qpg_bvh_parse_ws_bytes(n_bytes) bytes; contents on entry are ignored.
 * Five launches: token starts per block, a scan of the block counts, one thread per token start parses its token, a scan of
 * the blocks' fallback counts (it also writes info), the blocks with fallback tokens list them. */
int64_t qpg_bvh_parse_ws_bytes(int64_t n_bytes);
int qpg_bvh_parse_motion_f64(qpg_ctx*, void* stream, const uint8_t* text, int64_t n_bytes, int64_t n_values, double* values,
                             int64_t* fb_list, int fb_cap, int64_t* info, void* ws, int64_t ws_bytes);

/* Channel table -> rotation features, one launch.  values [dev] f64 [F][C]; output frame t < T reads input row t * rate
 * ((T - 1) * rate < F).  col, mirror_col [dev] i32 [J][3] (entries in [0, C): the caller's invariant), mirror_sign [dev] f64
 * [J][3].  The three angles of joint j are values[row][col[j][0..2]], in degrees, used as scipy's intrinsic 'ZXY' whatever
 * channels the file names (beat_data_to_lmdb.py:80-85 does the same): R = Rz(a0) Rx(a1) Ry(a2), row-major, into
 * upper [dev] f64 [T][9 J].  upper_mirror (optional, with both mirror tables): the same from
 * mirror_sign[j][k] * values[row][mirror_col[j][k]]. */
int qpg_bvh_rotation_f64(qpg_ctx*, void* stream, const double* values, int64_t F, int C, int rate, int64_t T, int J,
                         const int32_t* col, const int32_t* mirror_col, const double* mirror_sign, double* upper,
                         double* upper_mirror);

/* mean [dev] f64 [D] and population standard deviation stdv [dev] f64 [D] (np.std, ddof 0) of the columns of x [dev] f64
 * [N][D], N >= 1.  Two passes (the mean, then the squared deviations from it), each a two-stage sum in a fixed order.  A
 * column whose minimum equals its maximum gets that value as its mean and a std of exactly 0.
 * ws: at least qpg_column_stats_ws_doubles(N, D) doubles; contents on entry are ignored. */
int64_t qpg_column_stats_ws_doubles(int64_t N, int D);
int qpg_column_stats_f64(qpg_ctx*, void* stream, const double* x, int64_t N, int D, double* mean, double* stdv, double* ws,
                         int64_t ws_doubles);

/* ------------------------------------------------------------------------------------------
 * NOT part of the product library: measurement hooks of the kernel experiments.  They are compiled (and exported) only
 * with -DQPG_DEBUG_HOOKS (tools/build_variant.sh <source> <name> "-DQPG_DEBUG_HOOKS": a variant library the tools load
 * through QPG_LIB_PATH); in libqpg_hip.so what each of the three sets is a compile-time constant and the symbols
 * do not exist (tests/test_host_cpu.py asserts that).  Process-wide where they exist.
 * ---------------------------------------------------------------------------------------- */
#ifdef QPG_DEBUG_HOOKS
int qpg_debug_gemm64_waves(int nw);                  /* waves per block of qpg_hl_gemm_tilemin_h's kernel: 4 (default) or 8 */
int qpg_debug_convt_shape(int nq, int pd);           /* force the short-sequence convolution kernel's block shape */
int qpg_debug_convt_opts(int deep_ring, int xcd_map);/* deep fragment ring / XCD map of that kernel (measured, off) */
#endif

#ifdef __cplusplus
}
#endif
#endif /* QPG_H */
