// BVH ingestion: the motion block of a .bvh file -> the raw channel table -> the database's
// `upper` rotation features, and the per-column statistics every config carries as data_mean / data_std.
//   process/pymo/parsers.py:216-261      _parse_motion: frames x channels tokens, float() of each
//   process/beat_data_to_lmdb.py:58-65   DownSampler, RootTransformer('hip_centric'), Mirror('X'), JointSelector, ...
//   process/beat_data_to_lmdb.py:79-86   Rotation.from_euler('ZXY', angles, degrees=True).as_matrix() per frame
//   process/beat_data_to_lmdb.py:255-258 np.mean / np.std over all frames
// Everything is f64 and deterministic: no atomics anywhere, every sum in a fixed order, every word of scratch written
// before it is read.
#include "qpg_common.h"

// ---- parse ------------------------------------------------------------------------------------------------------------
// A block owns QPG_BVH_BLOCK_BYTES bytes of the text, a thread 16 consecutive ones.  A token STARTS at a non-whitespace
// byte whose predecessor is whitespace (or that is byte 0); its index is the number of starts before it: the starts of
// the earlier blocks (count kernel + scan kernel) plus the starts before it in its own block (LDS scan).  The thread that
// owns a start parses the token, reading on past its own 16 bytes and past the block's bytes up to n_bytes.
constexpr int BVH_THREADS = 256;
constexpr int BVH_CHUNK = 16;
static_assert(BVH_THREADS * BVH_CHUNK == QPG_BVH_BLOCK_BYTES, "a block is 256 threads x 16 bytes");

__device__ __forceinline__ bool bvh_is_space(unsigned c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }

// bit i of the result: byte off + i starts a token.  Bytes at or past n_bytes count as whitespace.
__device__ __forceinline__ unsigned bvh_start_mask(const uint8_t* __restrict__ text, int64_t n_bytes, int64_t off) {
  if (off >= n_bytes) return 0u;
  uint8_t b[BVH_CHUNK];
  if (off + BVH_CHUNK <= n_bytes) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + off);       // (text is 16-byte aligned: the entry point's check)
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < BVH_CHUNK; ++i) b[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  } else {
#pragma unroll
    for (int i = 0; i < BVH_CHUNK; ++i) b[i] = off + i < n_bytes ? text[off + i] : (uint8_t)' ';
  }
  bool prev = off == 0 || bvh_is_space(text[off - 1]);
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < BVH_CHUNK; ++i) {
    const bool sp = bvh_is_space(b[i]);
    if (!sp && prev) m |= 1u << i;
    prev = sp;
  }
  return m;
}

// exclusive prefix of one int per thread over the block, in thread order; *total = the block's sum.  sh: BVH_THREADS ints.
__device__ __forceinline__ int bvh_block_excl_scan(int v, int* sh, int* total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int d = 1; d < BVH_THREADS; d <<= 1) {
    const int add = tid >= d ? sh[tid - d] : 0;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  const int incl = sh[tid];
  *total = sh[BVH_THREADS - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(BVH_THREADS) void bvh_count_kernel(const uint8_t* __restrict__ text, int64_t n_bytes,
                                                                int32_t* __restrict__ cnt) {
  __shared__ int sh[BVH_THREADS];
  const int64_t off = ((int64_t)blockIdx.x * BVH_THREADS + threadIdx.x) * BVH_CHUNK;
  int total;
  bvh_block_excl_scan(__popc(bvh_start_mask(text, n_bytes, off)), sh, &total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// One block: base[b] = sum of cnt[0 .. b-1] (i64), in block order.  finish == 0: info[TOKENS] = the total.
// finish == 1 (cnt = the blocks' fallback counts): info[FALLBACK] = the total, info[STATUS] = the status word, from the
// blocks' bad-byte flags, info[TOKENS] (written by the first scan) and the total.
__global__ __launch_bounds__(1024) void bvh_scan_kernel(const int32_t* __restrict__ cnt, int64_t nb,
                                                        int64_t* __restrict__ base, int finish,
                                                        const int32_t* __restrict__ bad, int64_t n_values, int fb_cap,
                                                        int64_t* __restrict__ info) {
  __shared__ int64_t sh[1024];
  __shared__ int sbad[1024];
  const int tid = threadIdx.x;
  int64_t carry = 0;
  int anybad = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
    const int64_t b = b0 + tid;
    const int64_t v = b < nb ? (int64_t)cnt[b] : 0;
    if (finish && b < nb) anybad |= bad[b];
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int64_t add = tid >= d ? sh[tid - d] : 0;
      __syncthreads();
      sh[tid] += add;
      __syncthreads();
    }
    if (b < nb) base[b] = carry + sh[tid] - v;
    carry += sh[1023];
    __syncthreads();
  }
  sbad[tid] = anybad;
  __syncthreads();
  if (tid == 0) {
    if (!finish) {
      info[QPG_BVH_INFO_TOKENS] = carry;
    } else {
      int any = 0;
      for (int i = 0; i < 1024; ++i) any |= sbad[i];
      int64_t st = any ? QPG_BVH_ST_BADBYTE : 0;
      if (info[QPG_BVH_INFO_TOKENS] < n_values) st |= QPG_BVH_ST_SHORT;
      if (carry > (int64_t)fb_cap) st |= QPG_BVH_ST_OVERFLOW;
      info[QPG_BVH_INFO_FALLBACK] = carry;
      info[QPG_BVH_INFO_STATUS] = st;
    }
  }
}

// 10^k, k = 0 .. 22: every one is an f64 exactly
__device__ const double BVH_POW10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                         1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

enum { BVH_TOK_EXACT = 0, BVH_TOK_FALLBACK = 1, BVH_TOK_BAD = 2 };

// The token that starts at byte `off`:  [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?  up to the next
// whitespace byte or n_bytes.  EXACT: the significant digits fit a u64 of at most 2^53 and the net decimal exponent k is
// in [-22, 22]: mantissa x 10^k or mantissa / 10^k is ONE correctly rounded f64 operation on two exact operands, which is
// what strtod returns.  FALLBACK: well formed, but not of that kind (the host's float() decides).  BAD: a byte that the
// grammar has no place for, or a token longer than QPG_BVH_MAX_TOKEN bytes.
__device__ __forceinline__ int bvh_parse_token(const uint8_t* __restrict__ text, int64_t n_bytes, int64_t off,
                                               double* value) {
  int64_t i = off;
  const int64_t end = off + QPG_BVH_MAX_TOKEN < n_bytes ? off + QPG_BVH_MAX_TOKEN : n_bytes;
  unsigned c = text[i];
  bool neg = false;
  if (c == '+' || c == '-') {
    neg = c == '-';
    ++i;
  }
  unsigned long long mant = 0;
  int nsig = 0, nint = 0, nfrac = 0, e10 = 0;
  bool toolong = false;
  auto digit = [&](unsigned d) {
    if (mant != 0 || d != 0) {
      if (nsig < 19) {
        mant = mant * 10ull + d;
        ++nsig;
      } else {
        toolong = true;
      }
    }
  };
  for (; i < end; ++i, ++nint) {
    c = text[i];
    if (c < '0' || c > '9') break;
    digit(c - '0');
  }
  if (i < end && text[i] == '.') {
    for (++i; i < end; ++i, ++nfrac) {
      c = text[i];
      if (c < '0' || c > '9') break;
      digit(c - '0');
    }
  }
  if (nint + nfrac == 0) return BVH_TOK_BAD;
  if (i < end && (text[i] == 'e' || text[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < end && (text[i] == '+' || text[i] == '-')) {
      eneg = text[i] == '-';
      ++i;
    }
    int ne = 0;
    for (; i < end; ++i, ++ne) {
      c = text[i];
      if (c < '0' || c > '9') break;
      if (e10 < 100000) e10 = e10 * 10 + (int)(c - '0');
    }
    if (ne == 0) return BVH_TOK_BAD;
    if (eneg) e10 = -e10;
  }
  if (i < n_bytes && (i >= end || !bvh_is_space(text[i]))) return BVH_TOK_BAD;
  double v;
  if (toolong) return BVH_TOK_FALLBACK;
  if (mant == 0) {
    v = 0.0;
  } else {
    const int k = e10 - nfrac;            // (|e10| <= 100009, nfrac <= QPG_BVH_MAX_TOKEN: no overflow)
    if (mant > (1ull << 53) || k < -22 || k > 22) return BVH_TOK_FALLBACK;
    v = k >= 0 ? f_mul((double)mant, BVH_POW10[k]) : f_div((double)mant, BVH_POW10[-k]);
  }
  *value = neg ? -v : v;                  // negation, so that "-0.000000" is -0.0
  return BVH_TOK_EXACT;
}

// EMIT == false: values[t] for every token t < n_values of the block (a fallback token: the placeholder), and the block's
// fallback count and bad-byte flag.  EMIT == true (after the second scan, blocks with fallback tokens only): the block's
// fallback tokens into fb_list[fb_base[block] + rank in the block], as (token index, byte offset), slots below fb_cap.
template <bool EMIT>
__global__ __launch_bounds__(BVH_THREADS) void bvh_parse_kernel(const uint8_t* __restrict__ text, int64_t n_bytes,
                                                                const int64_t* __restrict__ base, int64_t n_values,
                                                                double* __restrict__ values, int32_t* __restrict__ fbcnt,
                                                                int32_t* __restrict__ bad,
                                                                const int64_t* __restrict__ fb_base,
                                                                int64_t* __restrict__ fb_list, int fb_cap) {
  __shared__ int sh[BVH_THREADS];
  if (EMIT && fbcnt[blockIdx.x] == 0) return;          // (uniform over the block)
  const int64_t off = ((int64_t)blockIdx.x * BVH_THREADS + threadIdx.x) * BVH_CHUNK;
  unsigned m = bvh_start_mask(text, n_bytes, off);
  int total;
  int64_t tok = base[blockIdx.x] + bvh_block_excl_scan(__popc(m), sh, &total);
  // at most 8 starts in 16 bytes; the classes of this thread's tokens, 2 bits each, for the fallback ranks
  unsigned cls = 0;
  int nfb = 0, nbad = 0, n = 0;
  for (unsigned mm = m; mm; mm &= mm - 1, ++n) {
    if (tok + n >= n_values) break;                     // pymo reads frames x channels tokens and ignores the rest
    const int64_t o = off + (__ffs(mm) - 1);
    double v = 0.0;
    const int c = bvh_parse_token(text, n_bytes, o, &v);
    cls |= (unsigned)c << (2 * n);
    nfb += c == BVH_TOK_FALLBACK;
    nbad += c == BVH_TOK_BAD;
    if (!EMIT) values[tok + n] = c == BVH_TOK_EXACT ? v : __longlong_as_double(QPG_BVH_PLACEHOLDER_BITS);
  }
  int fbtotal;
  const int fbrank = bvh_block_excl_scan(nfb, sh, &fbtotal);
  if (!EMIT) {
    int badtotal;
    bvh_block_excl_scan(nbad, sh, &badtotal);
    if (threadIdx.x == 0) {
      fbcnt[blockIdx.x] = fbtotal;
      bad[blockIdx.x] = badtotal != 0;
    }
  } else {
    int64_t slot = fb_base[blockIdx.x] + fbrank;
    int k = 0;
    for (unsigned mm = m; mm && k < n; mm &= mm - 1, ++k) {
      if (((cls >> (2 * k)) & 3u) != BVH_TOK_FALLBACK) continue;
      if (slot < (int64_t)fb_cap) {
        fb_list[2 * slot] = tok + k;
        fb_list[2 * slot + 1] = off + (__ffs(mm) - 1);
      }
      ++slot;
    }
  }
}

static inline int64_t bvh_blocks(int64_t n_bytes) { return (n_bytes + QPG_BVH_BLOCK_BYTES - 1) / QPG_BVH_BLOCK_BYTES; }

// ws: per block  i64 base | i64 fb_base | i32 cnt | i32 fbcnt | i32 bad | i32 (pad)
extern "C" int64_t qpg_bvh_parse_ws_bytes(int64_t n_bytes) {
  if (n_bytes < 0) return -1;
  const int64_t nb = bvh_blocks(n_bytes);
  return (nb > 0 ? nb : 1) * 32;
}

extern "C" int qpg_bvh_parse_motion_f64(qpg_ctx* ctx, void* stream, const uint8_t* text, int64_t n_bytes,
                                        int64_t n_values, double* values, int64_t* fb_list, int fb_cap, int64_t* info,
                                        void* ws, int64_t ws_bytes) {
  QPG_REQUIRE(ctx && info && ws && n_bytes >= 0 && n_values >= 0 && fb_cap >= 0, "qpg_bvh_parse_motion_f64: bad argument");
  QPG_REQUIRE((n_bytes == 0 || text) && (n_values == 0 || values) && (fb_cap == 0 || fb_list),
              "qpg_bvh_parse_motion_f64: a null array");
  QPG_REQUIRE(((uintptr_t)text & 15) == 0 && ((uintptr_t)ws & 7) == 0,
              "qpg_bvh_parse_motion_f64: text must be 16-byte and ws 8-byte aligned");
  const int64_t nb = bvh_blocks(n_bytes);
  QPG_REQUIRE(nb <= 0x7fffffff, "qpg_bvh_parse_motion_f64: text of more than 2^31 blocks");
  QPG_REQUIRE(ws_bytes >= qpg_bvh_parse_ws_bytes(n_bytes), "qpg_bvh_parse_motion_f64: ws_bytes %lld < %lld",
              (long long)ws_bytes, (long long)qpg_bvh_parse_ws_bytes(n_bytes));
  int64_t* base = reinterpret_cast<int64_t*>(ws);
  int64_t* fb_base = base + nb;
  int32_t* cnt = reinterpret_cast<int32_t*>(fb_base + nb);
  int32_t* fbcnt = cnt + nb;
  int32_t* bad = fbcnt + nb;
  hipStream_t s = qpg_stream(stream);
  if (nb > 0) {
    hipLaunchKernelGGL(bvh_count_kernel, dim3((unsigned)nb), dim3(BVH_THREADS), 0, s, text, n_bytes, cnt);
    QPG_LAUNCH_CHECK("bvh_count_kernel");
  }
  hipLaunchKernelGGL(bvh_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, nb, base, 0, bad, n_values, fb_cap, info);
  QPG_LAUNCH_CHECK("bvh_scan_kernel");
  if (nb > 0) {
    hipLaunchKernelGGL(bvh_parse_kernel<false>, dim3((unsigned)nb), dim3(BVH_THREADS), 0, s, text, n_bytes, base, n_values,
                       values, fbcnt, bad, fb_base, fb_list, fb_cap);
    QPG_LAUNCH_CHECK("bvh_parse_kernel");
  }
  hipLaunchKernelGGL(bvh_scan_kernel, dim3(1), dim3(1024), 0, s, fbcnt, nb, fb_base, 1, bad, n_values, fb_cap, info);
  QPG_LAUNCH_CHECK("bvh_scan_kernel");
  if (nb > 0 && fb_cap > 0) {
    hipLaunchKernelGGL(bvh_parse_kernel<true>, dim3((unsigned)nb), dim3(BVH_THREADS), 0, s, text, n_bytes, base, n_values,
                       values, fbcnt, bad, fb_base, fb_list, fb_cap);
    QPG_LAUNCH_CHECK("bvh_parse_kernel");
  }
  return QPG_OK;
}

// ---- features ---------------------------------------------------------------------------------------------------------
// One thread per (output frame, joint): three angles in the file's channel order, degrees, used as scipy's intrinsic
// 'ZXY':  R = Rz(a0) Rx(a1) Ry(a2), row-major.  The mirror copy reads sign x values[row][mirror_col] instead.
__device__ __forceinline__ void bvh_zxy_matrix(double a0, double a1, double a2, double* __restrict__ out) {
  const double RAD = 0.017453292519943295;               // pi / 180 (np.deg2rad's factor)
  double sz, cz, sx, cx, sy, cy;
  sincos(a0 * RAD, &sz, &cz);
  sincos(a1 * RAD, &sx, &cx);
  sincos(a2 * RAD, &sy, &cy);
  out[0] = cz * cy - sz * sx * sy;
  out[1] = -sz * cx;
  out[2] = cz * sy + sz * sx * cy;
  out[3] = sz * cy + cz * sx * sy;
  out[4] = cz * cx;
  out[5] = sz * sy - cz * sx * cy;
  out[6] = -cx * sy;
  out[7] = sx;
  out[8] = cx * cy;
}

__global__ __launch_bounds__(256) void bvh_rotation_kernel(const double* __restrict__ values, int64_t C, int64_t rate,
                                                           int64_t T, int J, const int32_t* __restrict__ col,
                                                           const int32_t* __restrict__ mirror_col,
                                                           const double* __restrict__ mirror_sign,
                                                           double* __restrict__ upper, double* __restrict__ upper_mirror) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * J) return;
  const int64_t t = i / J;
  const int j = (int)(i - t * J);
  const double* row = values + t * rate * C;
  bvh_zxy_matrix(row[col[3 * j]], row[col[3 * j + 1]], row[col[3 * j + 2]], upper + i * 9);
  if (upper_mirror)
    bvh_zxy_matrix(mirror_sign[3 * j] * row[mirror_col[3 * j]], mirror_sign[3 * j + 1] * row[mirror_col[3 * j + 1]],
                   mirror_sign[3 * j + 2] * row[mirror_col[3 * j + 2]], upper_mirror + i * 9);
}

extern "C" int qpg_bvh_rotation_f64(qpg_ctx* ctx, void* stream, const double* values, int64_t F, int C, int rate, int64_t T,
                                    int J, const int32_t* col, const int32_t* mirror_col, const double* mirror_sign,
                                    double* upper, double* upper_mirror) {
  QPG_REQUIRE(ctx && col && F >= 0 && C > 0 && rate > 0 && T >= 0 && J > 0, "qpg_bvh_rotation_f64: bad argument");
  QPG_REQUIRE(!upper_mirror || (mirror_col && mirror_sign), "qpg_bvh_rotation_f64: the mirror copy needs its two tables");
  QPG_REQUIRE(T == 0 || (values && upper && (T - 1) * (int64_t)rate < F),
              "qpg_bvh_rotation_f64: frame (T - 1) * rate is outside the %lld input frames", (long long)F);
  if (T == 0) return QPG_OK;
  // the tables are device arrays: their entries are the caller's invariant (0 <= col < C), checked by rotation_tables
  const int64_t n = T * J;
  QPG_REQUIRE((n + 255) / 256 <= 0x7fffffff, "qpg_bvh_rotation_f64: too many frames");
  hipLaunchKernelGGL(bvh_rotation_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, qpg_stream(stream), values,
                     (int64_t)C, (int64_t)rate, T, J, col, mirror_col, mirror_sign, upper, upper_mirror);
  QPG_LAUNCH_CHECK("bvh_rotation_kernel");
  return QPG_OK;
}

// ---- column statistics ------------------------------------------------------------------------------------------------
// mean and population standard deviation per column of x [N][D], two passes (the mean, then the squared deviations from
// it), each in two stages with a fixed order: the rows are cut into `nch` chunks of `rows` consecutive rows; a block of
// 64 columns x 4 row lanes sums its chunk (lane g takes rows g, g + 4, ..; the four lanes are added 0, 1, 2, 3), then one
// thread per column adds the chunks' partial sums in chunk order.  Pass 1 also carries each column's minimum and maximum:
// a column whose minimum equals its maximum is constant, its mean is that value (N equal addends do not always sum to N
// times the value) and its deviations, hence its std, are exactly 0.
constexpr int STATS_COLS = 64, STATS_LANES = 4;

__global__ __launch_bounds__(STATS_COLS* STATS_LANES) void column_partial_kernel(const double* __restrict__ x, int64_t N,
                                                                                 int D, int64_t rows,
                                                                                 const double* __restrict__ mean,
                                                                                 double* __restrict__ psum,
                                                                                 double* __restrict__ pmin,
                                                                                 double* __restrict__ pmax) {
  __shared__ double ssum[STATS_LANES][STATS_COLS], smin[STATS_LANES][STATS_COLS], smax[STATS_LANES][STATS_COLS];
  const int c = threadIdx.x % STATS_COLS, g = threadIdx.x / STATS_COLS;
  const int d = blockIdx.x * STATS_COLS + c;
  const int64_t r0 = (int64_t)blockIdx.y * rows;
  const int64_t r1 = r0 + rows < N ? r0 + rows : N;
  double s = 0.0, lo = INFINITY, hi = -INFINITY;
  if (d < D) {
    const double mu = mean ? mean[d] : 0.0;
    for (int64_t r = r0 + g; r < r1; r += STATS_LANES) {
      const double v = x[r * D + d];
      if (mean) {
        const double dv = f_sub(v, mu);
        s = f_add(s, f_mul(dv, dv));
      } else {
        s = f_add(s, v);
        lo = fmin(lo, v);
        hi = fmax(hi, v);
      }
    }
  }
  ssum[g][c] = s;
  smin[g][c] = lo;
  smax[g][c] = hi;
  __syncthreads();
  if (g == 0 && d < D) {
    for (int k = 1; k < STATS_LANES; ++k) {
      s = f_add(s, ssum[k][c]);
      lo = fmin(lo, smin[k][c]);
      hi = fmax(hi, smax[k][c]);
    }
    const int64_t o = (int64_t)blockIdx.y * D + d;
    psum[o] = s;
    if (!mean) {
      pmin[o] = lo;
      pmax[o] = hi;
    }
  }
}

__global__ __launch_bounds__(256) void column_final_kernel(const double* __restrict__ psum, const double* __restrict__ pmin,
                                                           const double* __restrict__ pmax, int64_t nch, int D, int64_t N,
                                                           int second, double* __restrict__ out) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  double s = 0.0, lo = INFINITY, hi = -INFINITY;
  for (int64_t k = 0; k < nch; ++k) {
    s = f_add(s, psum[k * D + d]);
    if (!second) {
      lo = fmin(lo, pmin[k * D + d]);
      hi = fmax(hi, pmax[k * D + d]);
    }
  }
  if (second)
    out[d] = sqrt(f_div(s, (double)N));
  else
    out[d] = lo == hi ? lo : f_div(s, (double)N);
}

static inline int64_t stats_chunks(int64_t N, int64_t* rows) {
  int64_t nch = (N + 255) / 256;
  if (nch > 1024) nch = 1024;
  if (nch < 1) nch = 1;
  *rows = (N + nch - 1) / nch;
  return (N + *rows - 1) / *rows;
}

extern "C" int64_t qpg_column_stats_ws_doubles(int64_t N, int D) {
  if (N <= 0 || D <= 0) return -1;
  int64_t rows;
  return 3 * stats_chunks(N, &rows) * D;
}

extern "C" int qpg_column_stats_f64(qpg_ctx* ctx, void* stream, const double* x, int64_t N, int D, double* mean,
                                    double* stdv, double* ws, int64_t ws_doubles) {
  QPG_REQUIRE(ctx && x && mean && stdv && ws && N > 0 && D > 0, "qpg_column_stats_f64: bad argument");
  QPG_REQUIRE(ws_doubles >= qpg_column_stats_ws_doubles(N, D), "qpg_column_stats_f64: ws_doubles %lld < %lld",
              (long long)ws_doubles, (long long)qpg_column_stats_ws_doubles(N, D));
  int64_t rows;
  const int64_t nch = stats_chunks(N, &rows);
  double* psum = ws;
  double* pmin = ws + nch * D;
  double* pmax = pmin + nch * D;
  hipStream_t s = qpg_stream(stream);
  const dim3 grid((unsigned)((D + STATS_COLS - 1) / STATS_COLS), (unsigned)nch), block(STATS_COLS * STATS_LANES);
  const dim3 fgrid((unsigned)((D + 255) / 256));
  hipLaunchKernelGGL(column_partial_kernel, grid, block, 0, s, x, N, D, rows, (const double*)nullptr, psum, pmin, pmax);
  QPG_LAUNCH_CHECK("column_partial_kernel");
  hipLaunchKernelGGL(column_final_kernel, fgrid, dim3(256), 0, s, psum, pmin, pmax, nch, D, N, 0, mean);
  QPG_LAUNCH_CHECK("column_final_kernel");
  hipLaunchKernelGGL(column_partial_kernel, grid, block, 0, s, x, N, D, rows, (const double*)mean, psum, pmin, pmax);
  QPG_LAUNCH_CHECK("column_partial_kernel");
  hipLaunchKernelGGL(column_final_kernel, fgrid, dim3(256), 0, s, psum, pmin, pmax, nch, D, N, 1, stdv);
  QPG_LAUNCH_CHECK("column_final_kernel");
  return QPG_OK;
}
