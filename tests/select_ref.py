"""Test-side statement of what a BOUNDED SELECT must return for any admissible input (not itself a test; plain NumPy).

The split-f16 / mixed-precision paths rest on a two-part argument: (1) a sweep or prefilter is within an a-priori bound E of
the exact value, (2) a select settles in exact arithmetic every comparison that a band slightly wider than 2 E leaves open.
The selects take the approximate distances as an ARGUMENT and re-evaluate from the operands, so part 2 can be tested on its
own: hand them exact distances + worst-case error of full width E and require the exact tables.  This module holds
  * the exact values (exact_audio: extended-precision accumulation; exact_text: sklearn's f32 order, oracle.knn_oracle),
  * the tables they imply (tables; fuse_best for the walk's rank fusion),
  * the noise patterns (noisy: zero / rademacher / swap / one_sided, each checked to stay within E AFTER the rounding to
    the matrix's storage type),
  * the conditions an input has to meet for the verdict to be determined by the input alone (admissible, TextCase.verdict),
  * the cases themselves (AUDIO_CASES, PRODUCT_CASE, TextCase), shared by tests/test_select_contract_cpu.py - which checks the
    conditions without a GPU - and tests/test_gpu_select_contract.py."""
import functools

import numpy as np

T_AUD, G_AUD, N_TAPS, TAP_STRIDE = 180, 26, 6, 2
ABSENT = 1e3
BAND_RATIO = 2.1                    # eps1 / E: AUDIO_HL_BAND / AUDIO_HL_ERR of qpgesture_amd/code_knn.py
MIX_LIST = 2048                     # tier-1 entries per query of qpg_percode_select_mixed_f64 (include/qpg.h)
SORT_LIST = 2048                    # band rows per block of qpg_percode_select_sorted_f32
BYC_LIST = 1024                     # (query, row) pairs per tile of qpg_percode_select_bycode_f32
NOISES = ("zero", "rademacher", "swap", "one_sided")
GAP = 1e-10                         # condition (a): distances that matter are bit-identical by construction or further apart


# ---- exact values --------------------------------------------------------------------------------------------------------
def cand_rows(base, cand_t, n_taps, tap_stride):
    """The candidates as rows: cand[j * G + g] = concat_i base[j][cand_t[g] + i * tap_stride] (zeros past T).  f32."""
    base = np.asarray(base, np.float32)
    N, T, F = base.shape
    G = len(cand_t)
    out = np.zeros((N, G, n_taps, F), np.float32)
    for g, t0 in enumerate(cand_t):
        for i in range(n_taps):
            t = int(t0) + i * tap_stride
            if t < T:
                out[:, g, i] = base[:, t]
    return out.reshape(N * G, n_taps * F)


def row_ids(rows):
    """id[c] == id[c'] iff rows c and c' are bit-identical (signed zeros: the bit pattern decides, like the operands)."""
    _, inv = np.unique(np.ascontiguousarray(rows).view(np.uint32), axis=0, return_inverse=True)
    return inv.reshape(-1)


def exact_audio(base, cand_t, n_taps, tap_stride, q32):
    """f64 distances 1 - <q, c> / sqrt(|q|^2 |c|^2) of every query against every candidate, from the f32 operands,
    accumulated in np.longdouble (64-bit mantissa here: ~1e-19 per term) and rounded ONCE to f64.  Degenerate rows follow
    the library's rule (qpg_common.h cosine_from_dot == sklearn's normalize, which leaves a row with norm < 10 eps
    unscaled): an all-zero candidate is at 0.5 from a non-zero query, 0 from a zero one.  Bit-identical candidate rows get
    bit-identical distances (the value is computed once per distinct row)."""
    assert np.finfo(np.longdouble).nmant >= 63, "exact_audio needs an extended-precision long double"
    rows = cand_rows(base, cand_t, n_taps, tap_stride)
    uniq, inv = np.unique(rows.view(np.uint32), axis=0, return_inverse=True)
    c = uniq.view(np.float32).astype(np.longdouble)
    q = np.asarray(q32, np.float32).astype(np.longdouble)
    dot = q @ c.T
    qn2, cn2 = (q * q).sum(1), (c * c).sum(1)
    nq, nc = np.sqrt(qn2), np.sqrt(cn2)
    tiny = np.longdouble(10.0 * np.finfo(np.float64).eps)
    zq, zc = nq < tiny, nc < tiny
    a = np.where(zq, qn2, np.longdouble(1))[:, None]
    b = np.where(zc, cn2, np.longdouble(1))[None, :]
    den = np.where(zq, np.longdouble(1), nq)[:, None] * np.where(zc, np.longdouble(1), nc)[None, :]
    cross = dot / den
    d = np.where(zq[:, None] | zc[None, :], np.longdouble(0.5) * (a + b - 2 * cross), np.longdouble(1) - cross)
    return np.ascontiguousarray(d.astype(np.float64)[:, inv.reshape(-1)])


def exact_text(qn, xn):
    """sklearn's f32 cosine distance of already NORMALISED rows, bit for bit: 0.5 * einsum_sq(qn - xn).  f32 [Q][C]."""
    from oracle import knn_oracle as O
    qn, xn = np.asarray(qn, np.float32), np.asarray(xn, np.float32)
    out = np.empty((qn.shape[0], xn.shape[0]), np.float32)
    for i in range(qn.shape[0]):
        out[i] = np.float32(0.5) * O.einsum_sq(qn[i][None] - xn)
    return out


# ---- tables --------------------------------------------------------------------------------------------------------------
def tables(D, cand_code, K, absent):
    """Per-code minimum of D [Q][C], its first-wins candidate (lowest index among equals, -1: no candidate) and the stable
    ranks of the K minima (np.argsort(kind='stable').argsort()); codes outside [0, K) are skipped."""
    D = np.asarray(D)
    code = np.asarray(cand_code).reshape(-1).astype(np.int64)
    Q = D.shape[0]
    dist = np.full((Q, K), absent, D.dtype)
    idx = np.full((Q, K), -1, np.int64)
    for k in np.unique(code[(code >= 0) & (code < K)]):
        cols = np.flatnonzero(code == k)                      # ascending: argmin's first hit is the lowest index
        j = D[:, cols].argmin(axis=1)
        dist[:, k] = D[np.arange(Q), cols[j]]
        idx[:, k] = cols[j]
    rank = np.argsort(np.argsort(dist, axis=1, kind="stable"), axis=1, kind="stable")
    return dist, idx, rank


def fused_scores(pos_rank, freq_rank, rank_row):
    """(pos_rank[p][c] + freq_rank[c] * 0.05) + rank_row[c] in f64, in that order of operations -> f64 [P][K]."""
    fixed = np.asarray(pos_rank).astype(np.float64) + np.asarray(freq_rank).astype(np.float64)[None, :] * 0.05
    return fixed + np.asarray(rank_row).astype(np.float64)[None, :]


def fuse_best(pos_rank, freq_rank, rank, top_n=1):
    """The walk's rank fusion: per (query, previous code p) the top_n (1 or 2) codes with the smallest score
    (pos_rank[p][c] + 0.05 freq_rank[c]) + rank[q][c] in f64, lowest code among equals.  -> int [Q][K][top_n].
    A plain argmin over the values given: the rows of `rank` need not be permutations."""
    Q, K = rank.shape
    out = np.empty((Q, pos_rank.shape[0], top_n), np.int64)
    rows = np.arange(pos_rank.shape[0])
    for q in range(Q):
        s = fused_scores(pos_rank, freq_rank, rank[q])
        for n in range(top_n):
            out[q, :, n] = s.argmin(axis=1)                    # (the first hit: the lowest code)
            s[rows, out[q, :, n]] = np.inf
    return out


# ---- noise ---------------------------------------------------------------------------------------------------------------
def noisy(kind, exact, cand_code, K, E, dtype, seed=0):
    """D_in of storage type `dtype` with max |D_in - exact| <= E AFTER the rounding to that type (asserted here):
      zero        no noise (f32: the rounding alone);
      rademacher  +-E per entry, seeded;
      swap        inside each code the exact winner gets +E and every other candidate -E; across codes the winner follows
                  the parity of its code's exact rank (even: +E, odd: -E) - every same-code pair of an even-ranked code and
                  every (even, odd) pair of rank neighbours closer than 2 E arrives in reversed order;
      one_sided   +E on odd candidate indices, 0 on even ones: moves minima, never by more than E.
    The amplitude is E minus one spacing of the storage type at the largest value, which the rounding may add back."""
    exact = np.asarray(exact, np.float64)
    dtype = np.dtype(dtype)
    amp = float(E) - float(np.spacing(dtype.type(np.abs(exact).max() + E)))
    assert amp > 0 or kind == "zero", "E is below the rounding of the storage type"
    Q, C = exact.shape
    if kind == "zero":
        noise = np.zeros_like(exact)
    elif kind == "rademacher":
        rng = np.random.Generator(np.random.PCG64(seed))
        noise = amp * (2.0 * rng.integers(0, 2, size=exact.shape) - 1.0)
    elif kind == "one_sided":
        noise = np.zeros_like(exact)
        noise[:, 1::2] = amp
    elif kind == "swap":
        _, idx, rank = tables(exact, cand_code, K, ABSENT)
        noise = np.full_like(exact, -amp)
        qq, kk = np.nonzero(idx >= 0)
        noise[qq, idx[qq, kk]] = np.where(rank[qq, kk] % 2 == 0, amp, -amp)
    else:
        raise ValueError(kind)
    D_in = (exact + noise).astype(dtype)
    assert np.abs(D_in.astype(np.float64) - exact).max() <= E, kind
    return D_in


def reversals(exact, D_in, cand_code, K):
    """(same-code, rank-neighbour) comparisons that D_in shows the select in REVERSED order: codes whose lowest D_in entry
    is not their exact winner (and not an exact tie with it), and exact rank neighbours whose D_in minima are ordered the
    other way round."""
    ed, ei, er = tables(exact, cand_code, K, ABSENT)
    nd, ni, _ = tables(np.asarray(D_in, np.float64), cand_code, K, ABSENT)
    Q = exact.shape[0]
    present = ei >= 0
    same = present & (ni != ei) & (exact[np.arange(Q)[:, None], np.where(present, ni, 0)] > ed)
    order = np.argsort(er, axis=1)                              # code at exact rank r
    a, b = order[:, :-1], order[:, 1:]
    rows = np.arange(Q)[:, None]
    nb = present[rows, a] & present[rows, b] & (ed[rows, a] < ed[rows, b]) & (nd[rows, a] > nd[rows, b])
    return int(same.sum()), int(nb.sum())


# ---- conditions on the inputs ----------------------------------------------------------------------------------------------
def admissible(exact, cand_code, K, eps1, E, eps2, row_id=None, capacity=MIX_LIST, min_mean=32):
    """The conditions under which the contract's verdict is determined by the input (checked on the CPU before any kernel):
      (a) any two exact distances that MATTER - contenders of one code (within eps1 + 2 E of its minimum) and the per-code
          minima - are either bit-equal because their operand rows are bit-identical (row_id), or more than 1e-10 apart:
          tier 2 (band eps2 < 1e-10) and the reference's own last bits stay out of the verdict;
      (b) the reference's upper bound on what the select may list - candidates of a code within eps1 + 2 E of its minimum
          where there are two or more, plus the winners of rank-neighbour minima within eps1 + 2 E (whatever lies within
          eps1 of an approximate minimum lies within eps1 + 2 E of the exact one) - is at most half the list capacity;
      (c) that bound is at least `min_mean` per query on average: the band is populated.
    Returns dict(ok, why, listed_max, listed_mean, band_members, rank_members)."""
    exact = np.asarray(exact, np.float64)
    code = np.asarray(cand_code).reshape(-1).astype(np.int64)
    Q, C = exact.shape
    w = eps1 + 2.0 * E
    why = []
    if not eps2 < GAP:
        why.append("eps2 >= 1e-10")
    ed, ei, er = tables(exact, code, K, ABSENT)
    valid = (code >= 0) & (code < K)
    listed = np.zeros(Q, np.int64)
    n_band = n_rank = 0
    bad_a = 0
    for q in range(Q):
        cmin = np.where(valid, ed[q, np.where(valid, code, 0)], -np.inf)
        cont = np.flatnonzero(valid & (exact[q] <= cmin + w))                      # contenders, every code
        o = cont[np.lexsort((exact[q, cont], code[cont]))]                         # by (code, value)
        same = code[o][1:] == code[o][:-1]
        gap = exact[q, o][1:] - exact[q, o][:-1]
        close = same & (gap <= GAP)
        if row_id is None:
            bad_a += int((close & (gap != 0)).sum())
        else:
            bad_a += int((close & ~((gap == 0) & (row_id[o][1:] == row_id[o][:-1]))).sum())
        cnt = np.bincount(code[cont], minlength=K)
        nb = int(cnt[cnt >= 2].sum())
        ks = np.flatnonzero(ei[q] >= 0)
        ks = ks[np.argsort(ed[q, ks], kind="stable")]
        g = np.diff(ed[q, ks])
        closem = g <= GAP
        if row_id is None:
            bad_a += int((closem & (g != 0)).sum())
        else:
            wr = row_id[ei[q, ks]]
            bad_a += int((closem & ~((g == 0) & (wr[1:] == wr[:-1]))).sum())
        near = np.zeros(len(ks), bool)
        near[1:] |= g <= w
        near[:-1] |= g <= w
        nr = int(near.sum())
        listed[q] = nb + nr
        n_band += nb
        n_rank += nr
    if bad_a:
        why.append("(a) %d pairs of distances that matter are closer than 1e-10 without being identical rows" % bad_a)
    if listed.max() > capacity // 2:
        why.append("(b) up to %d listed entries per query, more than half the capacity %d" % (listed.max(), capacity))
    if listed.mean() < min_mean:
        why.append("(c) %.1f listed entries per query on average, fewer than %d" % (listed.mean(), min_mean))
    return dict(ok=not why, why="; ".join(why), listed_max=int(listed.max()), listed_mean=float(listed.mean()),
                band_members=n_band / Q, rank_members=n_rank / Q)


def has_gap_below(exact, cand_code, K, limit):
    """Negative controls: is there a same-code pair (winner, other) or a pair of rank-neighbour minima whose exact gap is
    positive and below `limit`?  With the swap noise such a pair arrives reversed by more than a band of 1.05 E shows."""
    exact = np.asarray(exact, np.float64)
    code = np.asarray(cand_code).reshape(-1).astype(np.int64)
    ed, ei, er = tables(exact, code, K, ABSENT)
    valid = (code >= 0) & (code < K)
    n_same = n_rank = 0
    for q in range(exact.shape[0]):
        cmin = np.where(valid, ed[q, np.where(valid, code, 0)], -np.inf)
        gap = exact[q] - cmin
        even = valid & (er[q, np.where(valid, code, 0)] % 2 == 0)             # (the swap only bites in even-ranked codes)
        n_same += int((even & (gap > GAP) & (gap < limit)).sum())
        ks = np.flatnonzero(ei[q] >= 0)
        ks = ks[np.argsort(ed[q, ks], kind="stable")]
        g = np.diff(ed[q, ks])
        n_rank += int(((g > GAP) & (g < limit))[0::2].sum())                   # (even, odd) neighbours
    return n_same, n_rank


# ---- the audio cases -------------------------------------------------------------------------------------------------------
class AudioCase:
    """A small database + queries with the planted edge cases, its exact distances and reference tables.  Geometry: T = 180,
    G = 26 grid positions 6 frames apart, 6 taps of stride 2 (the product's), F features (32 unless stated)."""

    def __init__(self, name, N, Q, K, E, seed=0, F=32, half=False, crowded=None, eps1=None, shards=(), one_code=None):
        self.name, self.N, self.Q, self.K, self.E, self.F, self.half = name, N, Q, K, float(E), F, half
        self.eps1 = BAND_RATIO * self.E if eps1 is None else float(eps1)
        self.eps2 = 1e-12
        self.shards = tuple(shards)
        rng = np.random.Generator(np.random.PCG64(seed))
        T, G = T_AUD, G_AUD
        base = rng.standard_normal((N, T, F), dtype=np.float32)
        C = N * G
        n_present = min(int(np.ceil(0.85 * K)), max(C // 4, min(C, 10)))   # several codes have no candidate at all
        present = np.sort(rng.choice(K, size=n_present, replace=False))
        code = present[rng.integers(0, n_present, size=(N, G))].astype(np.int16)
        if crowded is not None:
            # test_mixed_on_a_crowded_database's construction at this geometry: 40 windows are copies of 4 source windows
            # perturbed by relative noise from 10^crowded to 1e-4, every other one with its source's codes
            for i in range(40):
                src, dst = i % 4, 8 + i
                eps = 10.0 ** rng.uniform(crowded, -4.0)
                base[dst] = (base[src] * (1.0 + eps * rng.standard_normal(base[src].shape))).astype(np.float32)
                if i % 2 == 0:
                    code[dst] = code[src]
        if N >= 8:
            code[3, 2:] = code[3, :2].repeat(12)                           # (the all-zero window below: two codes' worth of ties)
        if N >= 48:
            base[3] = 0.0                                                  # an all-zero window
            base[5], code[5] = base[1], code[1]                            # exact copies: same codes (lowest index wins) ...
            base[40], code[40] = base[1], code[1]                          # ... one of them in another row shard (W = 2, 3)
            base[20] = base[2]                                             # ... and with its own codes (equal minima)
        elif N >= 8:
            base[3] = 0.0
            base[5], code[5] = base[1], code[1]
            base[6] = base[2]
        if half:
            self.base16 = base.astype(np.float16)
            base = self.base16.astype(np.float32)                          # everything is defined on the rounded track
        code = code.reshape(-1)
        code[rng.random(C) < 0.03] = -1                                    # masked candidates
        if one_code is not None:
            # the tier-1 list's overflow: every frame is one vector u plus noise of relative size `a`, so every candidate row
            # is [u] * 6 + noise, and ALL of them carry one code.  Query 0 is [u] * 6 itself: its distances are second order
            # in the noise (~a^2 / 2, spread ~a^2 / 10) - all inside one band.  Every other query is an ordinary random row:
            # its distances vary in first order (~a / sqrt(6 F)) and only a few candidates are near the minimum.
            code_k, a = one_code
            u = rng.standard_normal(F, dtype=np.float32)
            base = (u[None, None, :] * (1.0 + a * rng.standard_normal((N, T, F), dtype=np.float32))).astype(np.float32)
            code = np.full(C, code_k, np.int16)
        self.base, self.cand_code = base, code
        self.cand_t = (np.arange(G) * 6).astype(np.int32)
        self.q32 = rng.standard_normal((Q, N_TAPS * F), dtype=np.float32)
        if one_code is not None:
            self.q32[0] = np.tile(u, N_TAPS)
        self.C = C

    @functools.cached_property
    def rows(self):
        return cand_rows(self.base, self.cand_t, N_TAPS, TAP_STRIDE)

    @functools.cached_property
    def row_id(self):
        return row_ids(self.rows)

    @functools.cached_property
    def cn2(self):
        return (self.rows.astype(np.float64) ** 2).sum(1)

    @functools.cached_property
    def qn2(self):
        return (self.q32.astype(np.float64) ** 2).sum(1)

    @functools.cached_property
    def exact(self):
        return exact_audio(self.base, self.cand_t, N_TAPS, TAP_STRIDE, self.q32)

    @functools.cached_property
    def ref(self):
        return tables(self.exact, self.cand_code, self.K, ABSENT)

    @functools.cached_property
    def verdict(self):
        return admissible(self.exact, self.cand_code, self.K, self.eps1, self.E, self.eps2, row_id=self.row_id)


# name -> constructor arguments.  E per case is the value at which `admissible` holds (tests/test_select_contract_cpu.py
# checks it and prints the band populations); the (N, Q, K) list, the f16 track and the product band are the issue's.
# overflow: N = 80 windows x G = 26 = 2080 candidates under ONE code, all within the band of query 0 - more than the
# MIX_LIST = 2048 entries of a tier-1 list, so the mixed select must raise stats[1] & 1; query 1 has an ordinary row.  Not in
# AUDIO_CASES: its verdict is NOT determined by the input (condition (b) fails by construction), and what it is for is the
# state the overflow path leaves in the workspace (tests/test_gpu_scratch_contract.py).
# (E = 1e-5 with a band of 4e-4: query 0's spread, ~2.7e-4, fits inside eps1 - 2 E; query 1's, ~1e-2, is 25 bands wide.)
OVERFLOW_CASE = dict(N=80, Q=2, K=96, E=1e-5, eps1=4e-4, seed=9, one_code=(3, 0.02))


def band_counts(c, eps):
    """Per query of case c: candidates (valid code) within eps of their code's exact minimum."""
    code = c.cand_code.astype(np.int64)
    valid = (code >= 0) & (code < c.K)
    ed = c.ref[0]
    cmin = np.where(valid[None], ed[:, np.where(valid, code, 0)], -np.inf)
    return (valid[None] & (c.exact <= cmin + eps)).sum(axis=1)


AUDIO_CASES = {
    "base": dict(N=48, Q=48, K=96, E=1e-3, seed=1, shards=(2, 3)),
    "odd": dict(N=37, Q=5, K=7, E=3e-3, seed=2),
    "one_window": dict(N=1, Q=1, K=512, E=1e-1, seed=3),
    "wide": dict(N=48, Q=200, K=512, E=3e-3, seed=4),
    "f16_track": dict(N=48, Q=48, K=96, E=1e-3, seed=5, half=True),
    "wavlm_width": dict(N=9, Q=6, K=16, E=2e-3, seed=6, F=1024),          # the LDS-staged tier-1 path (6 taps x 1024)
}
# The product band: E, eps1 are the product's constants (passed by the tests); the database is the crowded construction with
# relative noise from 6e-8 (one f32 ulp) to 1e-4.  Thousands of values inside a 5e-6 band put, at 48 queries, a dozen pairs
# closer than 1e-10 at every seed (condition (a)); 12 queries and this seed have none.
PRODUCT_CASE = dict(N=48, Q=12, K=96, seed=28, crowded=-7.2)


@functools.lru_cache(maxsize=None)
def audio_case(name):
    if name == "overflow":
        return AudioCase(name, **OVERFLOW_CASE)
    return AudioCase(name, **AUDIO_CASES[name])


@functools.lru_cache(maxsize=None)
def product_case(E, eps1):
    return AudioCase("product_band", E=E, eps1=eps1, **PRODUCT_CASE)


def signature_tables(K, seed=11, dim=16):
    """A seeded signature table and frequency ranks for the walk-relevance cut: sig f32 [K][dim], freq_rank i16 [K]; the
    pose ranks are taken from it by the library (qpg_l2_table_f32 + qpg_rank_rows_f32)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((K, dim), dtype=np.float32), rng.permutation(K).astype(np.int16)


# ---- the text case -----------------------------------------------------------------------------------------------------------
def sorted_layout(xn, codes, K):
    """NumPy restatement of qpgesture_amd.sorted_rows.SortedRows' row order (the GPU test checks the two agree): rows with a
    code in [0, K) that the normalisation did not leave at zero, without exact duplicates of an earlier row of the same code,
    sorted by code (stable), every segment padded to 16 rows (copies of its first row), the total to 64.
    -> row_index i32 [R] (-1: padding), src i32 [R] (the original row whose VALUES a slot holds, -1: the tail), seg_code
    [R] (-1: tail), zero_row i32 [K]."""
    xn = np.asarray(xn, np.float32)
    codes = np.asarray(codes).astype(np.int64)
    valid = (codes >= 0) & (codes < K)
    zero = (xn.astype(np.float64) ** 2).sum(1) < 0.5
    zero_row = np.full(K, -1, np.int32)
    for i in np.flatnonzero(valid & zero)[::-1]:
        zero_row[codes[i]] = i
    rid = row_ids(xn)
    row_index, src, seg = [], [], []
    for k in range(K):
        seen, mine = set(), []
        for i in np.flatnonzero(valid & ~zero & (codes == k)):
            if rid[i] not in seen:
                seen.add(rid[i])
                mine.append(i)
        pad = (-len(mine)) % 16
        row_index += mine + [-1] * pad
        src += mine + [mine[0]] * pad if mine else []
        seg += [k] * (len(mine) + pad)
    R = max((len(seg) + 63) // 64 * 64, 64)
    tail = R - len(seg)
    return (np.array(row_index + [-1] * tail, np.int32), np.array(src + [-1] * tail, np.int32),
            np.array(seg + [-1] * tail, np.int32), zero_row)


class TextCase:
    """D = 128, ~1 500 rows, K = 40: a few all-zero rows, exact duplicates, masked rows, codes with 1, 16 and 17 rows (the
    segment padding's edges) and one code with no row."""

    def __init__(self, n=1500, D=128, K=40, Q=300, band=2.0e-2, seed=21):
        from oracle import knn_oracle as O
        rng = np.random.Generator(np.random.PCG64(seed))
        self.n, self.D, self.K, self.Q, self.band = n, D, K, Q, float(band)
        self.e = self.band / BAND_RATIO
        X = rng.standard_normal((n, D), dtype=np.float32)
        code = rng.integers(4, K, size=n).astype(np.int32)              # codes 0 .. 3 are dealt by hand:
        code[:1] = 0                                                     # one row
        code[1:17] = 1                                                   # sixteen: a full tile, no padding
        code[17:34] = 2                                                  # seventeen: one row into a second tile
        #                                                                  code 3: no row at all
        X[100:106] = 0.0                                                 # all-zero embeddings (several codes)
        X[700:704] = X[699]                                              # exact duplicates under one code ...
        code[699:704] = 9
        X[800] = X[799]                                                  # ... and under two codes
        code[799], code[800] = 10, 11
        valid = rng.random(n) < 0.9
        valid[:34] = True
        self.codes_masked = np.where(valid, code, -1).astype(np.int32)
        q = rng.standard_normal((Q, D), dtype=np.float32)
        q[7] = 3.0 * X[699]                                              # a query that IS a (duplicated) row
        self.X, self.q = X, q
        self.xn, self.qn = O.l2_normalize(X), O.l2_normalize(q)

    @functools.cached_property
    def layout(self):
        return sorted_layout(self.xn, self.codes_masked, self.K)

    @functools.cached_property
    def d_sk(self):
        """sklearn's f32 value of every query against every ORIGINAL row."""
        return exact_text(self.qn, self.xn)

    @functools.cached_property
    def ref(self):
        """The exact sweep's tables: distances f32, first-wins indices, ranks, global nearest neighbours."""
        dist, idx, rank = tables(self.d_sk, self.codes_masked, self.K, np.float32(ABSENT))
        key = np.where(idx >= 0, dist, np.float32(np.inf))
        best = key.argmin(axis=1)                                         # (ties between codes: resolved below by index)
        nn = np.empty(self.Q, np.int64)
        for qi in range(self.Q):
            ks = np.flatnonzero(key[qi] == key[qi, best[qi]])
            nn[qi] = idx[qi, ks].min()
        return dist, idx, rank, nn

    @functools.cached_property
    def d_sorted(self):
        """d_sk in the sorted layout, f32 [Q][R]: a padding row holds its segment's first row's value, the tail +inf."""
        _, src, _, _ = self.layout
        out = np.full((self.Q, len(src)), np.inf, np.float32)
        live = src >= 0
        out[:, live] = self.d_sk[:, src[live]]
        return out

    def noisy(self, kind, amp_scale=1.0, seed=0):
        """Dm_in f32 [Q][R] = d_sorted + noise, |noise| <= e = band / 2.1 after the f32 rounding (asserted); padding rows
        get their own noise.  `swap` is taken over the sorted rows with the padding rows as ordinary members of their code."""
        row_index, src, seg, _ = self.layout
        live = src >= 0
        e = self.e * amp_scale
        D_in = np.full(self.d_sorted.shape, np.inf, np.float32)
        D_in[:, live] = noisy(kind, self.d_sorted[:, live].astype(np.float64), seg[live], self.K, e, np.float32, seed)
        return D_in

    @functools.cached_property
    def verdict(self):
        """Capacities (include/qpg.h): 2048 band rows / 1024 opened tiles per block of the by-query select - R <= 2048 cannot
        overflow either; 1024 (query, row) pairs per TILE of the by-code select - bounded here: a pair can be listed only if
        the row's exact value is within 2 band + 2 e of its code's exact minimum (mask: within band of the tile minimum,
        tile: within band of the code minimum, each approximate value within e).  That is an upper bound, so staying at or
        below the capacity rules an overflow out; the half-capacity margin of the audio cases is not available here: with
        300 queries the one-tile code of 16 rows alone gets 2 - 3 pairs per query at any band that leaves 32 rows per query
        beyond the winners."""
        row_index, src, seg, zero_row = self.layout
        R = len(src)
        why = []
        if R > SORT_LIST:
            why.append("R = %d rows could overflow the by-query list" % R)
        d = self.d_sorted.astype(np.float64)
        live = row_index >= 0
        dist = self.ref[0].astype(np.float64)
        cmin = np.where(seg >= 0, dist[:, np.where(seg >= 0, seg, 0)], -np.inf)           # [Q][R]
        pairs = (live[None] & (d <= cmin + 2 * self.band + 2 * self.e)).reshape(self.Q, R // 16, 16).sum(axis=(0, 2))
        first = np.flatnonzero(np.r_[True, seg[16::16] != seg[:-16:16]] & (seg[::16] >= 0))  # a code's first tile: + its zero row
        zc = seg[first * 16]
        pairs[first] += ((zero_row[zc] >= 0)[None] & (0.5 <= dist[:, zc] + self.band + 2 * self.e)).sum(axis=0)
        if pairs.max() > BYC_LIST:
            why.append("up to %d pairs in one tile, more than the %d the list holds" % (pairs.max(), BYC_LIST))
        members = (live[None] & (d <= cmin + self.band + 2 * self.e)).sum(axis=1)         # rows the band can hold, per query
        extra = members - (self.ref[1] >= 0).sum(axis=1)                                  # ... beyond one per present code
        if extra.mean() < 32:
            why.append("%.1f band rows per query beyond the winners, fewer than 32" % extra.mean())
        return dict(ok=not why, why="; ".join(why), R=R, tile_pairs_max=int(pairs.max()), band_rows_mean=float(members.mean()),
                    extra_mean=float(extra.mean()))


@functools.lru_cache(maxsize=None)
def text_case():
    return TextCase()
