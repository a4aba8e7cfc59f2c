"""Test-side statement of what the EXACT text sweeps (csrc/qpg_text.hip) and the edit-distance sweep (csrc/qpg_lev.hip)
must return, bit for bit (not itself a test; plain NumPy), and the table of cases.

Both families are exact by contract - sklearn's f32 cosine distance in NumPy-einsum order, unit-cost Levenshtein distance on
11-symbol strings - and both referee other tests, so the referee here is NumPy alone: oracle.knn_oracle (einsum_sq,
l2_normalize, lev) and tests/select_ref (exact_text, tables).  This module adds
  * the images the pack kernels must write (pack_f32: [tile][Dm/4][64][4] of normalised rows; pack_f16: [tile][Dm/8][64][8]
    of rows rounded to f16 + the norms of the ROUNDED values) and which of their bytes are padding,
  * the distances (dist_f32, dist_f16), the fused tables (percode) and the edit-distance matrix (lev_matrix),
  * three WRONG arithmetics of the same sum (wrong_dists) for the negative control,
  * the cases (Case / LevCase and the tables SWEEP_CASES, PERCODE_CASES, HALF_CASES, LEV_CASES), shared by
    tests/test_text_contract_cpu.py - which checks the conditions on them without a GPU - and
    tests/test_gpu_text_contract.py."""
import functools

import numpy as np

from oracle import knn_oracle as O
from tests import select_ref as S

ABSENT = np.float32(1e3)
THRESHOLD = np.float32(10) * np.finfo(np.float32).eps          # sklearn: a norm below 10 eps becomes 1
TINY = np.float32(1e-8)                                        # entries of the tiny rows: far below THRESHOLD, squares 1e-16
F32_MIN_NORMAL = np.finfo(np.float32).tiny
CONTROL_ROWS = 130                                             # rows a negative control is taken over at the least


# ---- images ------------------------------------------------------------------------------------------------------------
def grid_rows(ctx, cand_r):
    """Candidate c = j * G + g is ctx[j][cand_r[g]].  -> f32 [N * G][Dm] (a copy)."""
    ctx = np.asarray(ctx, np.float32)
    cand_r = np.asarray(cand_r).reshape(-1)
    return np.ascontiguousarray(ctx[:, cand_r, :]).reshape(ctx.shape[0] * len(cand_r), ctx.shape[2])


def _tiled(rows, piece, fill):
    """rows [C][Dm] -> ([ntile][Dm/piece][64][piece] flattened, live mask of the same shape): lane = c % 64."""
    C, Dm = rows.shape
    ntile = (C + 63) // 64
    padded = np.full((ntile * 64, Dm), fill, rows.dtype)
    padded[:C] = rows
    live = np.zeros((ntile * 64, Dm), bool)
    live[:C] = True
    shape = (ntile, 64, Dm // piece, piece)
    return (np.ascontiguousarray(padded.reshape(shape).transpose(0, 2, 1, 3)).reshape(-1),
            np.ascontiguousarray(live.reshape(shape).transpose(0, 2, 1, 3)).reshape(-1))


def pack_f32(ctx, cand_r):
    """What qpg_text_pack_candidates_f32 writes: (image f32 [ntile * Dm * 64], live bool of the same length, xn f32 [C][Dm]
    the sklearn-normalised rows).  Lanes of the last tile at or past C are padding (live False): the kernel leaves them as
    the caller filled them; here they hold NaN."""
    xn = O.l2_normalize(grid_rows(ctx, cand_r))
    image, live = _tiled(xn, 4, np.float32(np.nan))
    return image, live, xn


def pack_f16(ctx, cand_r):
    """What qpg_text_pack_candidates_f16 writes: (image f16 [ntile * Dm * 64], live, nrm f32 [C], x16 f16 [C][Dm]).  The rows
    are rounded to f16 (nearest even, f16 subnormals kept) and stored UNscaled; the norm is the einsum-order f32 norm of the
    rounded values, 1 where it is below 10 eps."""
    x16 = grid_rows(ctx, cand_r).astype(np.float16)
    nrm = np.sqrt(O.einsum_sq(x16.astype(np.float32)))
    nrm = np.where(nrm < THRESHOLD, np.float32(1), nrm).astype(np.float32)
    image, live = _tiled(x16, 8, np.float16(np.nan))
    return image, live, nrm, x16


# ---- distances -----------------------------------------------------------------------------------------------------------
def dist_f32(qn, xn):
    """0.5 * einsum_sq(qn - xn) in f32 for every (query, row) of already normalised rows.  f32 [Q][C]."""
    return S.exact_text(qn, xn)


def dist_f16(qn, x16, nrm):
    """The f16-storage sweep: widen to f32, divide element by element by the norm in f32, then the same sum."""
    xn = np.asarray(x16, np.float16).astype(np.float32) / np.asarray(nrm, np.float32)[:, None]
    return S.exact_text(qn, xn.astype(np.float32))


def _sq_diffs(qn, xn):
    d = np.asarray(qn, np.float32)[:, None, :] - np.asarray(xn, np.float32)[None, :, :]
    return d, d * d


def wrong_dists(qn, xn):
    """The same distances in three arithmetics that are NOT sklearn's: {name: f32 [Q][C]}.
      fma    the einsum order with each multiply-add fused (product exact in f64, one rounding of the sum);
      order  the four 4-element groups of a 16-element block visited u = 0, 1, 2, 3 instead of 3, 2, 1, 0;
      serial a plain left-to-right sum of the squared differences."""
    d, sq = _sq_diffs(qn, xn)
    Q, C, Dm = d.shape
    half = np.float32(0.5)
    blocks = d.reshape(Q, C, Dm // 16, 4, 4)
    acc = np.zeros((Q, C, 4), np.float32)
    for g in range(Dm // 16):
        for u in (3, 2, 1, 0):
            seg = blocks[:, :, g, u, :].astype(np.float64)
            acc = (seg * seg + acc.astype(np.float64)).astype(np.float32)
    fma = half * ((acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3]))
    sqb = sq.reshape(Q, C, Dm // 16, 4, 4)
    acc = np.zeros((Q, C, 4), np.float32)
    for g in range(Dm // 16):
        for u in (0, 1, 2, 3):
            acc = sqb[:, :, g, u, :] + acc
    order = half * ((acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3]))
    acc = np.zeros((Q, C), np.float32)
    for e in range(Dm):
        acc = acc + sq[:, :, e]
    return {"fma": fma, "order": order, "serial": half * acc}


# ---- tables --------------------------------------------------------------------------------------------------------------
def percode(D, code, K, absent=ABSENT, idx_base=0):
    """The fused select's outputs for the distance matrix D [Q][C]: (dist [Q][K], idx [Q][K], rank [Q][K], nn [Q]).
    Per code the minimum and its first-wins candidate (lowest index among equals) + idx_base; codes outside [0, K) are
    skipped, a code without candidate gives `absent` and -1; rank: the stable ranks of the K minima; nn: the lowest
    candidate index (+ idx_base) among the equal minima over all codes, -1 if no code has a candidate."""
    dist, idx, rank = S.tables(D, code, K, D.dtype.type(absent))
    have = idx >= 0
    nn = np.full(D.shape[0], -1, np.int64)
    for q in range(D.shape[0]):
        if have[q].any():
            best = dist[q, have[q]].min()
            nn[q] = idx[q, have[q] & (dist[q] == best)].min() + idx_base
    return dist, np.where(have, idx + idx_base, -1), rank, nn


def tie_counts(D, code, K):
    """(number of (query, code) pairs whose minimum is attained by two or more candidates with bit-equal distances, number
    of queries whose global minimum is shared by two or more codes)."""
    D = np.asarray(D)
    code = np.asarray(code).reshape(-1).astype(np.int64)
    dist, idx, _ = S.tables(D, code, K, D.dtype.type(ABSENT))
    pairs = 0
    for k in np.flatnonzero((idx >= 0).any(axis=0)):
        cols = np.flatnonzero(code == k)
        pairs += int(((D[:, cols] == dist[:, [k]]).sum(axis=1) >= 2).sum())
    key = np.where(idx >= 0, dist, np.inf)
    at_min = (key == key.min(axis=1, keepdims=True)) & (idx >= 0)
    return pairs, int((at_min.sum(axis=1) >= 2).sum())


# ---- the text cases ------------------------------------------------------------------------------------------------------
def _cand_r(rng, R, G):
    """G distinct rows of the R in an order that is no prefix of the rows (where R allows one)."""
    r = rng.permutation(R)[:G].astype(np.int32)
    if np.array_equal(r, np.arange(G)) and R > 1:
        r = (R - 1 - r).astype(np.int32)
    return r


def _norm(v, half):
    v = np.asarray(v, np.float32)
    if half:
        v = v.astype(np.float16).astype(np.float32)
    return np.float32(np.sqrt(O.einsum_sq(v)))


def _scaled(u, want):
    """u scaled to a norm next to the threshold: the first scale s0 (1 + k 2^-16), k = +-1, +-2, ... by which `want(row)`
    holds (s0 puts the norm on the threshold; the steps are far coarser than the norm's own rounding)."""
    s0 = float(THRESHOLD) / float(np.sqrt(O.einsum_sq(u)))
    for k in range(1, 4000):
        for sign in (1, -1):
            row = (u * np.float32(s0 * (1.0 + sign * k * 2.0 ** -16))).astype(np.float32)
            if want(row):
                return row
    raise AssertionError("no scale found")


class Case:
    """Seeded standard-normal rows ctx [N][R][Dm] and queries [Q][Dm] with the edge cases planted (C = N G >= 12):
      c = 0            a candidate with code K: past the table, skipped
      c = 1            the SOURCE row; candidates 2 and C - 2 (code ka, as the source) and 8, 9 and, from 65 candidates on,
                       C // 2 (code kb) are exact copies of it - ka and kb hold nothing else, so both minima are tied inside
                       their code and with each other
      c = 3, C - 1     all-zero rows (the last lane of the last tile among them)
      c = 4            a tiny row, entries +-1e-8: normalisation leaves it alone; every entry rounds to f16 zero
      c = 5, 6         rows just below / just above the 10 eps norm threshold (`below`, `above`; half: judged on the rounded row)
      c = 7            half only: two entries of 14.4 x 2^-24: norm 20.36 x 2^-24, above the threshold (20 x 2^-24); rounded to
                       f16 (14, 14) x 2^-24: norm 19.8 x 2^-24, below it
      q = Q - 1        2 x the source row (Q >= 2): its normalised row IS the source's, distance 0 to the copies
      q = Q // 2       an all-zero query (Q >= 3)
    Codes uniform in [0, K) with a tenth of the unplanted candidates masked to -1 and one code without any candidate
    (K >= 2).  With K < 4 the copies share one code with everything else; with C < 12 nothing is planted."""

    def __init__(self, name, N, R, G, Dm, Q, K, seed, half=False):
        self.name, self.N, self.R, self.G, self.Dm, self.Q, self.K, self.half = name, N, R, G, Dm, Q, K, half
        rng = np.random.default_rng(seed)
        C = self.C = N * G
        ctx = rng.standard_normal((N, R, Dm), dtype=np.float32)
        self.cand_r = _cand_r(rng, R, G)
        q = rng.standard_normal((Q, Dm), dtype=np.float32)
        code = rng.integers(0, K, size=C).astype(np.int16)
        planted = set()
        self.below = self.above = self.f16_only_below = None
        self.empty_code = None

        def put(c, row):
            ctx[c // G, self.cand_r[c % G]] = row

        if K >= 2:
            self.empty_code = int(rng.integers(0, K))
            code[code == self.empty_code] = (self.empty_code + 1) % K
        if C >= 12:
            src = grid_rows(ctx, self.cand_r)[1].copy()
            ka = kb = 1 if self.empty_code == 0 else 0
            if K >= 4:
                ka, kb = [k for k in range(K) if k != self.empty_code][:2]
                spare = [k for k in range(K) if k not in (ka, kb, self.empty_code)] or [ka]
                for c in np.flatnonzero((code == ka) | (code == kb)):
                    code[c] = spare[c % len(spare)]
            self.copies = {1: ka, 2: ka, C - 2: ka, 8: kb, 9: kb}
            if C >= 65:
                self.copies[C // 2] = kb
            planted = set(self.copies) | {0, 3, C - 1, 4, 5, 6, 7}
            for c, k in self.copies.items():
                put(c, src)
                code[c] = k
            put(3, 0.0)
            put(C - 1, 0.0)
            put(4, TINY * np.where(rng.random(Dm) < 0.5, -1, 1).astype(np.float32))
            u = rng.standard_normal(Dm, dtype=np.float32)
            self.below, self.above = 5, 6
            put(5, _scaled(u, lambda r: _norm(r, half) < THRESHOLD))
            put(6, _scaled(u, lambda r: _norm(r, half) >= THRESHOLD))
            if half:
                self.f16_only_below = 7
                row = np.zeros(Dm, np.float32)
                row[0] = row[Dm - 1] = np.float32(14.4 * 2.0 ** -24)
                put(7, row)
            code[0] = K
            if Q >= 2:
                q[Q - 1] = np.float32(2) * (src.astype(np.float16).astype(np.float32) if half else src)
            if Q >= 3:
                q[Q // 2] = 0.0
        free = np.setdiff1d(np.arange(C), sorted(planted))               # a tenth of the candidates masked, none of the planted
        code[rng.choice(free, size=min(len(free), (C + 5) // 10), replace=False)] = -1
        self.ctx, self.q, self.code = ctx, q, code
        self.qn = O.l2_normalize(q)

    @functools.cached_property
    def rows(self):
        return grid_rows(self.ctx, self.cand_r)

    @functools.cached_property
    def packed(self):
        """pack_f16's or pack_f32's tuple."""
        return pack_f16(self.ctx, self.cand_r) if self.half else pack_f32(self.ctx, self.cand_r)

    @functools.cached_property
    def xn(self):
        """The normalised rows the sweep sees, f32 [C][Dm]."""
        if self.half:
            _, _, nrm, x16 = self.packed
            return (x16.astype(np.float32) / nrm[:, None]).astype(np.float32)
        return self.packed[2]

    @functools.cached_property
    def D(self):
        """The exact distances, f32 [Q][C]."""
        if self.half:
            _, _, nrm, x16 = self.packed
            return dist_f16(self.qn, x16, nrm)
        return dist_f32(self.qn, self.xn)

    def tables(self, idx_base=0):
        return percode(self.D, self.code, self.K, ABSENT, idx_base)

    @property
    def ties(self):
        """A "ties" case: the two copy-only codes exist and there are enough queries for 20 tied (query, code) pairs."""
        return self.C >= 12 and self.K >= 4 and self.Q >= 10


# Geometries (N, R, G) by candidate count; cand_r is a seeded non-prefix choice of G of the R rows.
GEOMETRY = {1: (1, 1, 1), 12: (3, 5, 4), 64: (16, 5, 4), 65: (13, 6, 5), 512: (64, 9, 8), 513: (27, 20, 19), 546: (21, 30, 26),
            1000: (40, 30, 25)}
SWEEP_QS = (1, 2, 3, 8, 9, 24, 25, 96, 97, 100)     # both sides of every dispatch edge of qpg_text_cosine_f32; a last group that
#                                                     the clamp fills: <2,4> Q = 3, <6,4> 9, <4,4> 25, <12,4> 97 and 100


def _sweep_cases():
    """Test 1: one sweep over Q at C = 546 (Dm = 16: nk = 1, both prefetches wrap; Dm = 48) and one over C and Dm at Q = 9
    (<6,4>, a last group of 3) and Q = 100 (<12,4>, three blocks, a last group of 4)."""
    out = {}
    for Dm in (16, 48):
        for Q in SWEEP_QS:
            out["c546_d%d_q%d" % (Dm, Q)] = dict(C=546, Dm=Dm, Q=Q)
    for C in (1, 12, 64, 65, 546):
        for Dm in (16, 48, 384):
            for Q in (9, 100):
                out.setdefault("c%d_d%d_q%d" % (C, Dm, Q), dict(C=C, Dm=Dm, Q=Q))
    return out


SWEEP_CASES = _sweep_cases()
# Tests 3 and 4: (C, Q, K, Dm).  Tiles: 1, 2, 8, 9, 16.  The LDS form takes 12 queries per block, the LDS-free form 96.
PERCODE_CASES = {
    "c1_q1_k1": dict(C=1, Q=1, K=1, Dm=16),
    "c65_q11_k7": dict(C=65, Q=11, K=7, Dm=16),
    "c512_q12_k512": dict(C=512, Q=12, K=512, Dm=16),
    "c513_q97_k7_d384": dict(C=513, Q=97, K=7, Dm=384),          # 9 tiles x 2 query blocks: a ragged XCD group
    "c1000_q13_k1024": dict(C=1000, Q=13, K=1024, Dm=16),        # the largest table of the LDS form (96 KB)
    "c1000_q95_k512_d384": dict(C=1000, Q=95, K=512, Dm=384),
    "c513_q96_k1": dict(C=513, Q=96, K=1, Dm=16),
    "c65_q97_k1024": dict(C=65, Q=97, K=1024, Dm=16),
}
HALF_CASES = {
    "c1_q1_k1": dict(C=1, Q=1, K=1, Dm=16),
    "c65_q11_k7": dict(C=65, Q=11, K=7, Dm=16),
    "c512_q96_k1_d48": dict(C=512, Q=96, K=1, Dm=48),
    "c513_q97_k512_d384": dict(C=513, Q=97, K=512, Dm=384),
    "c1000_q13_k1024": dict(C=1000, Q=13, K=1024, Dm=16),
    "c1000_q12_k7_d384": dict(C=1000, Q=12, K=7, Dm=384),
}


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    p = SWEEP_CASES[name]
    N, R, G = GEOMETRY[p["C"]]
    return Case("sweep/" + name, N, R, G, p["Dm"], p["Q"], 16, seed=1000 + sorted(SWEEP_CASES).index(name))


@functools.lru_cache(maxsize=None)
def percode_case(name, half=False):
    table = HALF_CASES if half else PERCODE_CASES
    p = table[name]
    N, R, G = GEOMETRY[p["C"]]
    return Case(("half/" if half else "percode/") + name, N, R, G, p["Dm"], p["Q"], p["K"],
                seed=(3000 if half else 2000) + sorted(table).index(name), half=half)


def all_cases():
    """Every text case of the three tables, by its name."""
    for n in SWEEP_CASES:
        yield sweep_case(n)
    for n in PERCODE_CASES:
        yield percode_case(n)
    for n in HALF_CASES:
        yield percode_case(n, True)


def control_rows(case):
    """The rows a negative control is taken over: the case's own normalised rows, topped up to CONTROL_ROWS with unit rows
    from the case's distribution (a share of a row of 1 or 12 entries says nothing); exact copies of a query are left out
    per query by the caller."""
    xn = case.xn
    if xn.shape[0] < CONTROL_ROWS:
        rng = np.random.default_rng(case.C * 1000 + case.Dm)
        extra = rng.standard_normal((CONTROL_ROWS - xn.shape[0], case.Dm), dtype=np.float32)
        if case.half:
            extra = extra.astype(np.float16).astype(np.float32)
        xn = np.concatenate([xn, O.l2_normalize(extra)])
    return xn


# ---- the edit-distance sweep ---------------------------------------------------------------------------------------------
LEV_T = 40


def tap_offsets(T):
    """The 11 taps of a vq-wav2vec feature row: 6 backward taps -int((5 - i) s), 5 forward taps int(i s), s = T / 30
    (qpgesture_amd.code_knn.wavvq_tap_offsets; the CPU test checks the two agree)."""
    s = T / 30
    return [-int((5 - i) * s) for i in range(6)] + [int(i * s) for i in range(1, 6)]


def gather(track, t, taps):
    """The string of frame t: track[t + off] per tap, 0 outside the window."""
    T = len(track)
    return tuple(int(track[t + o]) if 0 <= t + o < T else 0 for o in taps)


def lev_matrix(sym_db, cand_t, taps, sym_q, q_win, q_t):
    """Unit-cost edit distance between the zero-padded 11-symbol strings of every query (sym_q[q_win][q_t + taps]) and every
    candidate c = j * G + g (sym_db[j][cand_t[g] + taps]).  f32 [Q][N * G] of exact small integers."""
    cand = [gather(sym_db[j], int(t), taps) for j in range(sym_db.shape[0]) for t in cand_t]
    ids = {}
    cid = np.array([ids.setdefault(s, len(ids)) for s in cand])
    uniq = list(ids)
    out = np.empty((len(q_win), len(cand)), np.float32)
    memo = {}
    for q, (w, t) in enumerate(zip(q_win, q_t)):
        a = gather(sym_q[int(w)], int(t), taps)
        if a not in memo:
            memo[a] = np.array([O.lev(a, b) for b in uniq], np.float32)
        out[q] = memo[a][cid]
    return out


class LevCase:
    """T = 40 frames, the product's tap formula.  Symbols from a small alphabet (so that strings share symbols) with a few
    large ones (g1 320 + g2 up to 102 399) and REAL zeros at both ends of some windows, next to the zero padding.  cand_t
    holds 0 and T - 1 where G allows both; q_t covers 0, T - 1 and a middle frame where Q allows."""

    def __init__(self, name, N, G, Q, seed, K=16, Mq=3):
        self.name, self.N, self.G, self.Q, self.K, self.Mq, self.T = name, N, G, Q, K, Mq, LEV_T
        T = LEV_T
        rng = np.random.default_rng(seed)
        self.taps = tap_offsets(T)
        alphabet = np.array([0, 1, 2, 3, 7, 319 * 320 + 319], np.int32)
        self.sym_db = alphabet[rng.integers(0, len(alphabet), size=(N, T))]
        self.sym_q = alphabet[rng.integers(0, len(alphabet), size=(Mq, T))]
        self.sym_db[0, :3] = 0                                    # real zeros where the back taps are padded ...
        self.sym_db[N - 1, T - 3:] = 0                            # ... and where the forward taps are
        self.sym_q[0, :2] = 0
        self.sym_q[Mq - 1, T - 2:] = 0
        self.sym_q[1] = self.sym_db[N // 2]                       # a query window that IS a database window (distance 0)
        t = rng.integers(0, T, size=G).astype(np.int32)
        if G >= 2:
            t[:2] = (T - 1, 0)
        else:
            t[0] = T - 1 if N == 1 else 0
        self.cand_t = t
        self.q_win = rng.integers(0, Mq, size=Q).astype(np.int32)
        self.q_t = rng.integers(0, T, size=Q).astype(np.int32)
        edge = [(Mq - 1, T - 1), (0, 0), (1, T // 2)][:Q]
        self.q_win[:len(edge)] = [w for w, _ in edge]
        self.q_t[:len(edge)] = [f for _, f in edge]
        if Q > 1024:
            self.q_win[1024:], self.q_t[1024:] = Mq - 1, T - 1    # the one-query last chunk reads the last frame
        self.C = N * G
        code = rng.integers(0, K - 1, size=self.C).astype(np.int16)        # code K - 1 has no candidate
        code[rng.random(self.C) < 0.1] = -1
        self.code = code

    @functools.cached_property
    def D(self):
        return lev_matrix(self.sym_db, self.cand_t, self.taps, self.sym_q, self.q_win, self.q_t)


# name: (N, G, Q).  C = 1, 255, 256, 257 (the 256-candidate blocks) at Q = 1 and 7; the 1024-query chunks at C = 12.
LEV_CASES = {
    "c1_q1": (1, 1, 1), "c255_q7": (15, 17, 7), "c256_q7": (16, 16, 7), "c257_q7": (257, 1, 7), "c257_q1": (257, 1, 1),
    "c12_q1024": (3, 4, 1024), "c12_q1025": (3, 4, 1025),
}


@functools.lru_cache(maxsize=None)
def lev_case(name):
    N, G, Q = LEV_CASES[name]
    return LevCase(name, N, G, Q, seed=4000 + sorted(LEV_CASES).index(name))
