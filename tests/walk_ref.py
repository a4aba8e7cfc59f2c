"""Test-side statement of what the WALK (qpgesture_amd/csrc/qpg_tail.hip: rank fusion, phase gate, tabulated gate and
chase, serial walk, batch and takes forms) must return for the arguments of qpg_match_steps.  Plain NumPy, no torch, no
GPU; not itself a test.

  * the contract: stable_rank, fuse (tests/select_ref.fuse_best), gate (oracle.knn_oracle.cosine_pair: sklearn's f32 order
    and its 10 eps rule), walk (the literal sequential walk), gate_table + chase (every (step, previous code, previous vote)
    outcome tabulated, a walk is then Q lookups);
  * deliberately wrong VARIANTS of it (the negative controls of tests/test_walk_contract_cpu.py);
  * the adversarial inputs (circulant / boundary / not-a-permutation / random fusion tables, the phase database with
    planted ties, near ties, zero and barely-normalisable blocks, idx tables with absent codes) and the CASES shared by
    tests/test_walk_contract_cpu.py - which pins this file to the reference's goldens and checks that the inputs bite -
    and tests/test_gpu_walk_contract.py.

Layouts are the device's: phase f32 [N][Tp][16] (channels 0 and 2 of the dense phase side by side), a candidate index
ci = j * G + g reads head = phase[j, ps : ps + 8], tail = phase[j, ps + 24 : ps + 32] (ps = pslot[g]) and the payload
code[j, cidx[g] : cidx[g] + 4].  An ABSENT candidate (table entry -1) is read as candidate 0 and raises status[0] - what
include/qpg.h documents (the reference project raises IndexError there)."""
import functools
import types

import numpy as np

from oracle import knn_oracle as O
from tests import select_ref as R

STEP_CODES = 4
EPS10 = np.float32(10.0) * np.finfo(np.float32).eps          # sklearn's "do not scale" threshold, ~1.19e-6


# ---- the contract ------------------------------------------------------------------------------------------------------------
def stable_rank(x):
    """np.argsort(kind='stable').argsort() along the last axis."""
    x = np.asarray(x)
    return np.argsort(np.argsort(x, axis=-1, kind="stable"), axis=-1, kind="stable")


def fuse(pos_rank, freq_rank, rank_rows, top_n=1):
    """Winning codes of the rank fusion for all (q, p): (pos_rank[p][c] + freq_rank[c] * 0.05) + rank[q][c] in f64 in that
    order, stable argmin (lowest code among equal scores), the top 2 for the one-modality modes.  Rows of `rank_rows` that
    are not permutations are taken as the values they are.  -> int64 [Q][K][top_n]."""
    return R.fuse_best(np.asarray(pos_rank), np.asarray(freq_rank), np.asarray(rank_rows), top_n)


def gate_vectors(prev, head):
    """a = rows prev[-5:] + head[:3], b = rows prev[-3:] + head[:5] of two (..., 8, 16) blocks -> two (..., 128) f32."""
    prev, head = np.asarray(prev, np.float32), np.asarray(head, np.float32)
    lead = np.broadcast_shapes(prev.shape[:-2], head.shape[:-2])
    prev, head = np.broadcast_to(prev, lead + (8, 16)), np.broadcast_to(head, lead + (8, 16))
    a = np.concatenate((prev[..., -5:, :], head[..., :3, :]), axis=-2).reshape(lead + (128,))
    b = np.concatenate((prev[..., -3:, :], head[..., :5, :]), axis=-2).reshape(lead + (128,))
    return a, b


def gate(prev, head):
    """Phase-gate score of a candidate's head block after the previous block (GestureKNN.py:636), sklearn's f32 paired
    cosine distance, over any leading dimensions."""
    a, b = gate_vectors(prev, head)
    return O.cosine_pair(a, b)


def gate_no_eps_rule(prev, head):
    """VARIANT: normalises by the norm whatever its size (no `norm < 10 eps -> leave unscaled`)."""
    a, b = gate_vectors(prev, head)
    with np.errstate(all="ignore"):
        an = a / np.sqrt(O.einsum_sq(a))[..., None]
        bn = b / np.sqrt(O.einsum_sq(b))[..., None]
        return np.float32(0.5) * O.einsum_sq(an - bn)


def vote_of(s0, s1):
    """list.index(min): the second candidate only if strictly better."""
    return (s1 < s0).astype(np.int64)


def vote_le(s0, s1):
    """VARIANT: the second candidate on ties."""
    return (s1 <= s0).astype(np.int64)


# fusion variants (negative controls): same signature as `fuse`
def fuse_ties_high(pos_rank, freq_rank, rank_rows, top_n=1):
    """VARIANT: the HIGHEST code among equal scores."""
    K = rank_rows.shape[1]
    out = R.fuse_best(pos_rank[:, ::-1], freq_rank[::-1], rank_rows[:, ::-1], top_n)
    return K - 1 - out


def _fuse_by(score_fn, pos_rank, freq_rank, rank_rows, top_n):
    Q, K = rank_rows.shape
    out = np.empty((Q, pos_rank.shape[0], top_n), np.int64)
    rows = np.arange(pos_rank.shape[0])
    for q in range(Q):
        s = score_fn(pos_rank.astype(np.int64), freq_rank.astype(np.int64), rank_rows[q].astype(np.int64))
        for n in range(top_n):
            out[q, :, n] = s.argmin(axis=1)
            s[rows, out[q, :, n]] = np.iinfo(np.int64).max if s.dtype == np.int64 else np.inf
    return out


def fuse_int_scaled(pos_rank, freq_rank, rank_rows, top_n=1):
    """VARIANT: exact integer arithmetic 20 (pos + rank) + freq instead of the f64 sum with its roundings."""
    return _fuse_by(lambda p, f, r: 20 * (p + r[None, :]) + f[None, :], pos_rank, freq_rank, rank_rows, top_n)


def fuse_freq_last(pos_rank, freq_rank, rank_rows, top_n=1):
    """VARIANT: (pos + rank) + freq * 0.05 - the other association."""
    return _fuse_by(lambda p, f, r: (p + r[None, :]).astype(np.float64) + f.astype(np.float64)[None, :] * 0.05,
                    pos_rank, freq_rank, rank_rows, top_n)


def fuse_scan(pos_rank, freq_rank, rank_rows, stop_at_equal=False, round_ranks=64):
    """The branch-and-bound scan of fuse_best_ranked_kernel restated: codes visited in rank order, `round_ranks` at a time,
    until the next round's first rank EXCEEDS the best score so far (stop_at_equal: VARIANT that stops at `>=`); argmin
    (lowest code among equals) over what was visited.  Permutation rows only.  -> int64 [Q][K][1]."""
    Q, K = rank_rows.shape
    out = np.empty((Q, pos_rank.shape[0], 1), np.int64)
    nr = (K + round_ranks - 1) // round_ranks
    for q in range(Q):
        r = rank_rows[q].astype(np.int64)
        assert np.array_equal(np.sort(r), np.arange(K)), "fuse_scan takes permutation rows"
        s = R.fused_scores(pos_rank, freq_rank, r)                               # [P][K] in code order
        by_rank = s[:, np.argsort(r)]
        pad = np.full((s.shape[0], nr * round_ranks - K), np.inf)
        best = np.minimum.accumulate(np.concatenate((by_rank, pad), 1).reshape(s.shape[0], nr, round_ranks).min(2), axis=1)
        nxt = (np.arange(nr) + 1) * round_ranks                                   # first rank of the round after round k
        stop = (nxt[None, :] >= best) if stop_at_equal else (nxt[None, :] > best)
        stop[:, -1] = True
        visited = nxt[stop.argmax(axis=1)]                                        # ranks [0, visited) were scanned
        out[q, :, 0] = np.where(r[None, :] < visited[:, None], s, np.inf).argmin(axis=1)
    return out


# ---- a problem: the arguments of qpg_match_steps -------------------------------------------------------------------------------
class Problem(types.SimpleNamespace):
    """aud_rank / txt_rank i16 [Q][K], aud_idx / txt_idx i32 [Q][K], pos_rank i16 [K][K], freq_rank i16 [K], code i32
    [N][code_ld], aud_cidx / aud_pslot [Ga], txt_cidx / txt_pslot [Gt], phase f32 [N][Tp][16], M, steps, K; seeds:
    seed_codes [S], seed_phases [S][8][16]."""

    @property
    def Q(self):
        return self.M * self.steps

    @property
    def codes_per_window(self):
        return min(STEP_CODES * self.steps, 30)

    def grids(self, mode):
        """(G, cidx, pslot) of the grid behind table 0 and behind table 1 (qpg.h: modes 0 / 1 / 2)."""
        a = (len(self.aud_cidx), self.aud_cidx, self.aud_pslot)
        t = (len(self.txt_cidx), self.txt_cidx, self.txt_pslot)
        return {0: (a, t), 1: (a, a), 2: (t, t)}[mode]

    def tables(self, mode, fuse_fn=fuse, rows=None):
        """The two gate-candidate tables T0 / T1 int64 [Q][K] (candidate index, -1: the winning code is absent) - what
        qpg_match_steps leaves in regions [0] / [1] of gate_tables - and the winning codes W0 / W1."""
        if fuse_fn is fuse and rows is None:
            cache = self.__dict__.setdefault("_tables", {})
            if mode not in cache:
                cache[mode] = self.tables(mode, rows=slice(0, self.Q))
            return cache[mode]
        rows = slice(0, self.Q) if rows is None else rows
        q = np.arange(self.aud_rank[rows].shape[0])[:, None]
        if mode == 0:
            W0 = fuse_fn(self.pos_rank, self.freq_rank, self.aud_rank[rows])[..., 0]
            W1 = fuse_fn(self.pos_rank, self.freq_rank, self.txt_rank[rows])[..., 0]
            return self.aud_idx[rows][q, W0].astype(np.int64), self.txt_idx[rows][q, W1].astype(np.int64), W0, W1
        rank, idx = (self.aud_rank, self.aud_idx) if mode == 1 else (self.txt_rank, self.txt_idx)
        W = fuse_fn(self.pos_rank, self.freq_rank, rank[rows], 2)
        return idx[rows][q, W[..., 0]].astype(np.int64), idx[rows][q, W[..., 1]].astype(np.int64), W[..., 0], W[..., 1]


def cand(P, grid, ci):
    """Window, head-block start frame and payload column of candidates `ci` (any shape) of one grid; -1 reads candidate 0."""
    G, cidx, pslot = grid
    cc = np.where(np.asarray(ci) < 0, 0, ci).astype(np.int64)
    j, g = cc // G, cc % G
    return j, np.asarray(pslot, np.int64)[g], np.asarray(cidx, np.int64)[g]


def _blocks(P, j, start):
    """phase[j, start : start + 8] for arrays j / start -> (..., 8, 16)."""
    return P.phase[np.asarray(j)[..., None], np.asarray(start)[..., None] + np.arange(8)]


def cand_head(P, grid, ci):
    j, ps, _ = cand(P, grid, ci)
    return _blocks(P, j, ps)


def cand_tail(P, grid, ci):
    j, ps, _ = cand(P, grid, ci)
    return _blocks(P, j, ps + 24)


def cand_pay(P, grid, ci):
    j, _, cx = cand(P, grid, ci)
    return P.code[np.asarray(j)[..., None], np.asarray(cx)[..., None] + np.arange(STEP_CODES)].astype(np.int64)


def walk(P, mode, seed_code, seed_phase, T=None, gate_fn=gate, vote_fn=vote_of):
    """The literal sequential walk of one clip.  -> codes int64 [M][codes_per_window], vote [M][steps], phase_out f32
    [M][steps][8][16], status0 (1: a visited (step, previous code) has an absent entry in either table)."""
    T0, T1 = (P.tables(mode) if T is None else T)[:2]
    g0, g1 = P.grids(mode)
    cpw = P.codes_per_window
    prev_code, prev = int(seed_code), np.asarray(seed_phase, np.float32)
    codes = np.empty((P.M, cpw), np.int64)
    votes = np.empty((P.M, P.steps), np.int64)
    phases = np.empty((P.M, P.steps, 8, 16), np.float32)
    bad = 0
    for w in range(P.M):
        win = []
        for s in range(P.steps):
            q = w * P.steps + s
            c = (T0[q, prev_code], T1[q, prev_code])
            bad |= int(c[0] < 0 or c[1] < 0)
            s0 = gate_fn(prev, cand_head(P, g0, c[0]))
            s1 = gate_fn(prev, cand_head(P, g1, c[1]))
            fi = int(vote_fn(np.asarray(s0), np.asarray(s1)))
            grid = g1 if fi else g0
            pay = cand_pay(P, grid, c[fi])
            prev = cand_tail(P, grid, c[fi])
            win.extend(int(v) for v in pay)
            prev_code = int(pay[-1])
            votes[w, s] = fi
            phases[w, s] = prev
        codes[w] = win[:cpw]
        prev_code = win[cpw - 1]                 # the next window is seeded by the last KEPT code (and the last phase block)
    return codes, votes, phases, bad


def gate_table(P, mode, T=None, gate_fn=gate, vote_fn=vote_of):
    """Outcome of every (step q >= 1, previous code pp, previous vote kp): G[q][2 pp + kp] = (p << 1) | vote, p = the
    previous code step q sees when candidate T_kp[q - 1][pp] won step q - 1.  Row 0 is the seed's (step0).  Needs the kept
    code that seeds the next window to come from the window's last step (steps <= 8).  -> int64 [Q][2K]."""
    T0, T1 = (P.tables(mode) if T is None else T)[:2]
    g = P.grids(mode)
    last = P.codes_per_window - 1
    assert last // STEP_CODES == P.steps - 1, "the state is not a function of the previous step's winner"
    off_last = last % STEP_CODES
    Q, K = T0.shape
    G = np.zeros((Q, 2 * K), np.int64)
    if Q < 2:
        return G
    q = np.arange(1, Q)[:, None]
    off = np.where(q % P.steps == 0, off_last, STEP_CODES - 1)                   # a window's first step: the last KEPT code
    for kp in (0, 1):
        ci = (T1 if kp else T0)[:-1]                                             # [Q - 1][K]: the winner of step q - 1
        prev = cand_tail(P, g[kp], ci)
        p = np.take_along_axis(cand_pay(P, g[kp], ci), np.broadcast_to(off, ci.shape)[..., None], axis=-1)[..., 0]
        s0 = gate_fn(prev, cand_head(P, g[0], T0[q, p]))
        s1 = gate_fn(prev, cand_head(P, g[1], T1[q, p]))
        G[1:, kp::2] = (p << 1) | vote_fn(s0, s1)
    return G


def step0(P, mode, seed_codes, seed_phases, T=None, gate_fn=gate, vote_fn=vote_of):
    """(seed code << 1) | vote of every seed's first step -> int64 [S]."""
    T0, T1 = (P.tables(mode) if T is None else T)[:2]
    g = P.grids(mode)
    p = np.asarray(seed_codes, np.int64)
    prev = np.asarray(seed_phases, np.float32)
    s0 = gate_fn(prev, cand_head(P, g[0], T0[0, p]))
    s1 = gate_fn(prev, cand_head(P, g[1], T1[0, p]))
    return (p << 1) | vote_fn(s0, s1)


def chase(P, mode, G, sigma0, T=None):
    """Q lookups per seed.  sigma0 [S] from step0.  -> dict(sig [Q][S], codes [S][M][cpw], vote [S][M][steps], phase
    [S][M][steps][8][16], status0 [S])."""
    T0, T1 = (P.tables(mode) if T is None else T)[:2]
    g = P.grids(mode)
    Q = T0.shape[0]
    S = len(sigma0)
    sig = np.empty((Q, S), np.int64)
    sig[0] = sigma0
    for q in range(1, Q):
        sig[q] = G[q, sig[q - 1]]
    p, fi = sig >> 1, sig & 1
    q = np.arange(Q)[:, None]
    c0, c1 = T0[q, p], T1[q, p]
    tail = np.where((fi == 1)[..., None, None], cand_tail(P, g[1], c1), cand_tail(P, g[0], c0))
    pay = np.where((fi == 1)[..., None], cand_pay(P, g[1], c1), cand_pay(P, g[0], c0))          # [Q][S][4]
    M, steps, cpw = Q // P.steps, P.steps, P.codes_per_window
    codes = pay.transpose(1, 0, 2).reshape(S, M, steps * STEP_CODES)[:, :, :cpw]
    return dict(sig=sig, codes=np.ascontiguousarray(codes), vote=np.ascontiguousarray(fi.T.reshape(S, M, steps)),
                phase=np.ascontiguousarray(tail.transpose(1, 0, 2, 3).reshape(S, M, steps, 8, 16)),
                status0=((c0 < 0) | (c1 < 0)).any(axis=0).astype(np.int64))


def solve(P, mode, seed_codes=None, seed_phases=None, T=None, gate_fn=gate, vote_fn=vote_of):
    """gate_table + step0 + chase for the problem's seeds (or the ones given)."""
    T = P.tables(mode) if T is None else T
    sc = P.seed_codes if seed_codes is None else seed_codes
    sp = P.seed_phases if seed_phases is None else seed_phases
    G = gate_table(P, mode, T, gate_fn, vote_fn)
    out = chase(P, mode, G, step0(P, mode, sc, sp, T, gate_fn, vote_fn), T)
    out["G"] = G
    return out


def census(P, mode, sol, seed_phases=None, T=None):
    """What the gates of the REACHED states (those some seed of `sol` visits) look like: exact ties between two different
    head blocks, near ties (margin nonzero, at most 4 ulp of the larger score), evaluations with one / both gate vectors
    under the 10 eps rule, votes of each kind.  Counts of distinct (step, previous block, previous code) states."""
    T0, T1 = (P.tables(mode) if T is None else T)[:2]
    g = P.grids(mode)
    sp = P.seed_phases if seed_phases is None else seed_phases
    sig = sol["sig"]
    Q, S = sig.shape
    out = dict(states=0, ties=0, near=0, tiny_one=0, tiny_both=0, vote0=0, vote1=0)
    for q in range(Q):
        p = sig[q] >> 1
        if q == 0:
            prev = np.asarray(sp, np.float32)
            key = np.stack([p, np.unique(prev.reshape(S, -1), axis=0, return_inverse=True)[1].reshape(-1)], 1)
        else:
            pf = sig[q - 1] & 1
            pc0, pc1 = T0[q - 1, sig[q - 1] >> 1], T1[q - 1, sig[q - 1] >> 1]
            pci = np.where(pf == 1, pc1, pc0)
            prev = np.where((pf == 1)[:, None, None], cand_tail(P, g[1], pc1), cand_tail(P, g[0], pc0))
            key = np.stack([p, 2 * np.where(pci < 0, 0, pci) + pf], 1)
        _, first = np.unique(key, axis=0, return_index=True)
        p, prev = p[first], prev[first]
        c0, c1 = T0[q, p], T1[q, p]
        h0, h1 = cand_head(P, g[0], c0), cand_head(P, g[1], c1)
        s0, s1 = gate(prev, h0), gate(prev, h1)
        j0, ps0, _ = cand(P, g[0], c0)
        j1, ps1, _ = cand(P, g[1], c1)
        differ = (j0 != j1) | (ps0 != ps1)
        margin = np.abs(s0.astype(np.float64) - s1.astype(np.float64))
        ulp = np.spacing(np.maximum(s0, s1)).astype(np.float64)
        out["states"] += len(first)
        out["ties"] += int(((s0 == s1) & differ).sum())
        out["near"] += int(((margin > 0) & (margin <= 4 * ulp)).sum())
        for h in (h0, h1):
            a, b = gate_vectors(prev, h)
            ta, tb = np.sqrt(O.einsum_sq(a)) < EPS10, np.sqrt(O.einsum_sq(b)) < EPS10
            out["tiny_one"] += int((ta ^ tb).sum())
            out["tiny_both"] += int((ta & tb).sum())
        out["vote1"] += int((s1 < s0).sum())
        out["vote0"] += int((~(s1 < s0)).sum())
    return out


# ---- fusion inputs -------------------------------------------------------------------------------------------------------------
def _relabel(perm, pos, freq, *ranks):
    """Rename code c to perm[c] everywhere."""
    inv = np.argsort(perm)
    return (pos[inv][:, inv],  freq[inv]) + tuple(r[:, inv] for r in ranks)


def circulant_tables(K, Q, shift, seed, swaps=True, row0=0):
    """pos_rank[p][c] = (p - 1 - c) mod K (a permutation per row, p itself last), freq_rank[c] = (K - 1 - c + shift) mod
    K, rank rows = the identity with the adjacent pairs (i, i + 1), i = q mod 22, + 22, ..., swapped (a second set of rows
    with i = (q + 11) mod 22 for the other modality); everything then relabelled by a seeded permutation of the codes.
    Without the swaps: every previous code has its own winner, at every depth 0 .. K - 1 of the rank order.
    -> pos i16 [K][K], freq i16 [K], rank_a i16 [Q][K], rank_b i16 [Q][K]."""
    c = np.arange(K)
    pos = (c[:, None] - 1 - c[None, :]) % K
    freq = (K - 1 - c + shift) % K
    ranks = []
    for off in (0, 11):
        r = np.tile(c, (Q, 1))
        if swaps:
            for q in range(Q):
                i = np.arange((q + row0 + off) % 22, K - 1, 22)
                r[q, i], r[q, i + 1] = r[q, i + 1].copy(), r[q, i].copy()
        ranks.append(r)
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(K)
    return tuple(x.astype(np.int16) for x in _relabel(perm, pos, freq, *ranks))


SHIFTS = tuple(range(0, 512, 32))
CIRCULANT_SEED = 3000        # (of the relabellings tried, one that leaves >= 3 tasks where integer arithmetic differs)


@functools.lru_cache(maxsize=None)
def circulant_set(K=512, Q=22):
    """The 16 circulant databases of the fusion tests: shifts 0, 32, ..., 480 -> [(pos, freq, rank_a, rank_b)]."""
    return [circulant_tables(K, Q, s % K, CIRCULANT_SEED + s) for s in SHIFTS]


def random_tables(K, Q, seed, tie_free=False):
    """The control: seeded permutations (pose rows with p itself last).  tie_free: a rank row is drawn again until none of
    its K tasks has an exact tie at the fused minimum or an argmin that integer arithmetic would place elsewhere (random
    tables have about one such task in a thousand; the control of the negative controls has none)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = np.stack([rng.permutation(K) for _ in range(K)])
    for p in range(K):
        at = np.flatnonzero(pos[p] == K - 1)[0]
        pos[p, at], pos[p, p] = pos[p, p], K - 1
    freq = rng.permutation(K)

    def row():
        while True:
            r = rng.permutation(K)
            if not tie_free:
                return r
            st = tie_stats(pos, freq, r[None])
            if st["ties"] == 0 and st["int_differs"] == 0:
                return r
    ra = np.stack([row() for _ in range(Q)])
    rb = np.stack([row() for _ in range(Q)])
    return tuple(x.astype(np.int16) for x in (pos, freq, ra, rb))


BOUNDARIES = (64, 128, 192, 448)


def boundary_tables(K, Q, deep_first, seed):
    """A planted tie at score exactly B = BOUNDARIES[q % 4] (those below K) in every task (q, p) with p % 4 == q % 4: code
    `deep` sits at rank B with zero pose and frequency part, code `shallow` at rank 3 + q % 4 with pose rank B - 1 - rank
    and frequency rank 20 (20 * 0.05 == 1.0 exactly in f64); every other code of such a task scores above B.  deep_first:
    deep < shallow in code index - the winner is the one BEYOND the round the scan could stop at; otherwise the shallow one
    wins and the deep one must not.  Rank rows are permutations; pose rows of the planted tasks are not (values in
    [0, K), which is all the kernels assume).  -> pos, freq, rank_a, rank_b (i16), planted bool [Q][K], deep, shallow."""
    assert 20.0 * 0.05 == 1.0
    rng = np.random.Generator(np.random.PCG64(seed))
    Bs = [b for b in BOUNDARIES if b < K] or [K // 2]
    lo, hi = sorted(rng.choice(K, 2, replace=False).tolist())
    deep, shallow = (lo, hi) if deep_first else (hi, lo)
    freq = rng.permutation(K)
    for code, val in ((deep, 0), (shallow, 20)):
        at = np.flatnonzero(freq == val)[0]
        freq[at], freq[code] = freq[code], val
    pos, ranks, _, _ = random_tables(K, Q, seed + 1)
    pos = pos.astype(np.int64)
    planted = np.zeros((Q, K), bool)
    rows = []
    for q in range(Q):
        B, rs = Bs[q % len(Bs)], 3 + q % len(Bs)
        r = np.empty(K, np.int64)
        others = np.setdiff1d(np.arange(K), [deep, shallow])
        r[others] = rng.permutation(np.setdiff1d(np.arange(K), [B, rs]))
        r[deep], r[shallow] = B, rs
        rows.append(r)
    rank = np.stack(rows)
    for p in range(K):
        cls = p % len(Bs)
        qs = np.arange(cls, Q, len(Bs))
        if p in (deep, shallow) or not len(qs):
            continue
        B = Bs[cls]
        pos[p] = rng.integers(B + 1, K, size=K)                         # every other code: score > B whatever its rank
        pos[p, deep], pos[p, shallow] = 0, B - 1 - (3 + cls)
        planted[qs, p] = True
    s = [R.fused_scores(pos, freq, rank[q]) for q in range(Q)]
    for q in range(Q):
        for p in np.flatnonzero(planted[q]):
            B = Bs[p % len(Bs)]
            assert s[q][p, deep] == B == s[q][p, shallow] and (np.delete(s[q][p], [deep, shallow]) > B).all()
    rb = np.stack([rank[(q + 1) % Q] for q in range(Q)])
    return pos.astype(np.int16), freq.astype(np.int16), rank.astype(np.int16), rb.astype(np.int16), planted, deep, shallow


def nonperm_tables(K, seed):
    """Two rank rows that are not permutations: row 0 holds one rank twice (another one is missing), row 1 holds a rank
    outside [0, K) (one above, one negative entry); row 2 is a permutation (the control inside the same call).  Fusion in
    isolation only - the walk is never fed these."""
    pos, freq, ra, _ = random_tables(K, 3, seed)
    ra = ra.astype(np.int64)
    ra[0, np.flatnonzero(ra[0] == 5)[0]] = 6
    ra[1, np.flatnonzero(ra[1] == 0)[0]] = K + 5
    ra[1, np.flatnonzero(ra[1] == 1)[0]] = -3
    return pos, freq, ra.astype(np.int16)


def tie_stats(pos, freq, rank):
    """Over all tasks (q, p): exact f64 ties at the fused minimum; of those, tasks where the lowest tied code sits at a
    deeper rank than another tied code; tasks whose argmin differs from integer-scaled arithmetic; the winners' depths."""
    ties = deeper = differ = 0
    depth = []
    for q in range(rank.shape[0]):
        s = R.fused_scores(pos, freq, rank[q])
        m = s.min(axis=1)
        tied = s == m[:, None]
        win = s.argmin(axis=1)
        r = rank[q].astype(np.int64)
        multi = tied.sum(axis=1) > 1
        ties += int(multi.sum())
        shallowest = np.where(tied, r[None, :], np.iinfo(np.int64).max).min(axis=1)
        deeper += int((multi & (r[win] > shallowest)).sum())
        si = 20 * (pos.astype(np.int64) + r[None, :]) + freq.astype(np.int64)[None, :]
        differ += int((si.argmin(axis=1) != win).sum())
        depth.append(r[win])
    return dict(ties=ties, deeper=deeper, int_differs=differ, depth=np.stack(depth))


# ---- the database and the cases ------------------------------------------------------------------------------------------------
TP = 48                      # heads live in frames [0, 24), tails in [24, 48): pslot <= 16, and pslot + 32 == Tp at 16
CODE_LD = 32                 # cidx + 4 <= code_ld, with equality at cidx = 28
N_SEEDS = 1000


def _grid(G, mul, add, parity=None):
    g = np.arange(G)
    pslot = (g * mul + add) % 17
    cidx = (g * 3 + add) % 29
    if parity is not None:                                              # even / odd start frames only
        return cidx.astype(np.int32), (2 * ((g * mul) % 8) + parity).astype(np.int32)
    if G > 1:
        pslot[-1], cidx[-1] = 16, 28                                    # both edges on one grid position
    return cidx.astype(np.int32), pslot.astype(np.int32)


def _database(K, N, Q, Ga, Gt, rng, disjoint_slots=False):
    """Standard-normal phase database, random codes below K, idx tables that are injective per row, grids, seeds (every
    code 0 .. K - 1; six phase blocks, one of them all-zero).  disjoint_slots (the control): the two grids share no start
    frame, so no two candidates of one step read the same head block and the database holds no exact gate tie."""
    assert N * Ga >= K and N * Gt >= K
    phase = rng.standard_normal((N, TP, 16), dtype=np.float32)
    code = rng.integers(0, K, size=(N, CODE_LD)).astype(np.int32)
    aud_idx = np.stack([rng.permutation(N * Ga)[:K] for _ in range(Q)]).astype(np.int32)
    txt_idx = np.stack([rng.permutation(N * Gt)[:K] for _ in range(Q)]).astype(np.int32)
    a_cidx, a_pslot = _grid(Ga, 5, 0, 0 if disjoint_slots else None)
    t_cidx, t_pslot = _grid(Gt, 7, 3, 1 if disjoint_slots else None)
    blocks = rng.standard_normal((6, 8, 16), dtype=np.float32)
    blocks[5] = 0.0
    i = np.arange(N_SEEDS)
    return dict(phase=phase, code=code, aud_idx=aud_idx, txt_idx=txt_idx, aud_cidx=a_cidx, aud_pslot=a_pslot,
                txt_cidx=t_cidx, txt_pslot=t_pslot, seed_codes=(i % K).astype(np.int32),
                seed_phases=np.ascontiguousarray(blocks[(i // K + i) % 6]))


PLANTS = ("tie", "near", "zero_both", "zero_one", "split", "below", "above")


def plant(P, mode, rng, per_step=3, max_step=24):
    """Plants the gate cases where the walks of P's seeds GO (the reached states of the tables of `mode` under the database
    as it is): for a reached state (step q, previous winner, candidates c0 / c1)
      tie        head(c1) := head(c0)                           exact gate tie between two different candidates
      near       head(c1) := head(c0), 2 elements one ulp off   near tie
      zero_both  tail(previous winner) := 0, head(c0)[:5] := 0  both gate vectors under the 10 eps rule (all-zero blocks)
      zero_one   ... head(c1)[:3] := 0                          one of them
      split / below / above   ... head(c0)[:5] scaled so that the gate vectors' norms fall on both sides of / just below /
                 just above 10 eps = 1.19e-6
    Step 0 states take the zero-phase seeds for the kinds that need a vanishing previous block.  Frames that an earlier
    plant wrote or relies on are left alone.  A plant moves walks, so what is finally there is COUNTED by census()."""
    g = P.grids(mode)
    T0, T1 = P.tables(mode)[:2]
    sol = solve(P, mode, T=(T0, T1))
    sig = sol["sig"]
    used = P.__dict__.setdefault("_planted_frames", set())          # shared by the passes for the three modes
    zero_seed = ~np.asarray(P.seed_phases).reshape(len(P.seed_codes), -1).any(axis=1)

    def frames(j, lo, n=8):
        return {(int(j), f) for f in range(int(lo), int(lo) + n)}

    count = {k: 0 for k in PLANTS}
    for q in range(min(sig.shape[0], max_step)):
        key = np.stack([sig[q], sig[q - 1] if q else zero_seed.astype(np.int64)], 1)
        order = rng.permutation(np.unique(key, axis=0, return_index=True)[1])        # one seed per distinct state
        n_here = 2 * len(PLANTS) if q == 0 else per_step                 # step 0 has a state per seed: each kind twice
        for kind in [PLANTS[(per_step * q + i) % len(PLANTS)] for i in range(n_here)]:
            for s in order:
                p = int(sig[q, s] >> 1)
                c0, c1 = int(T0[q, p]), int(T1[q, p])
                if c0 < 0 or c1 < 0:
                    continue
                j0, ps0, _ = cand(P, g[0], c0)
                j1, ps1, _ = cand(P, g[1], c1)
                need_zero_prev = kind not in ("tie", "near")
                touch = frames(j0, ps0) | frames(j1, ps1)
                if (j0, ps0) == (j1, ps1):
                    continue
                if q == 0:
                    if need_zero_prev != bool(zero_seed[s]):
                        continue
                    tj = None
                else:
                    pf = int(sig[q - 1, s] & 1)
                    pci = int((T1 if pf else T0)[q - 1, sig[q - 1, s] >> 1])
                    if pci < 0:
                        continue
                    tj, tps, _ = cand(P, g[pf], pci)
                    tj, tps = int(tj), int(tps)
                    if need_zero_prev:
                        touch |= frames(tj, tps + 24)
                if touch & used:
                    continue
                used |= touch
                h0 = P.phase[j0, ps0:ps0 + 8]
                if need_zero_prev and tj is not None:
                    P.phase[tj, tps + 24:tps + 32] = 0.0
                if kind == "tie":
                    P.phase[j1, ps1:ps1 + 8] = h0
                elif kind == "near":
                    # one ulp up in the first n of a fixed order of the 80 elements the gate reads, n grown until the two
                    # scores differ (a few ulp-sized changes mostly round away: the scores stay EQUAL)
                    prev = P.seed_phases[s] if tj is None else P.phase[tj, tps + 24:tps + 32].copy()
                    at = rng.permutation(80)
                    for n in (3, 8, 16, 32, 64, 80):
                        h = h0.copy()
                        h.reshape(-1)[at[:n]] = np.nextafter(h.reshape(-1)[at[:n]], np.float32(np.inf))
                        if gate(prev, h) != gate(prev, h0):
                            break
                    P.phase[j1, ps1:ps1 + 8] = h
                elif kind == "zero_both":
                    P.phase[j0, ps0:ps0 + 5] = 0.0
                elif kind == "zero_one":
                    P.phase[j1, ps1:ps1 + 3] = 0.0
                else:
                    # |a| = norm of head rows [:3] (48 values), |b| = of rows [:5] (80 values): |b| ~ 1.29 |a|
                    na = float(np.sqrt((h0[:3].astype(np.float64) ** 2).sum()))
                    nb = float(np.sqrt((h0[:5].astype(np.float64) ** 2).sum()))
                    scale = {"split": 1.10e-6 / na, "below": 1.17e-6 / nb, "above": 1.21e-6 / na}[kind]
                    P.phase[j0, ps0:ps0 + 5] = (h0[:5] * np.float32(scale)).astype(np.float32)
                count[kind] += 1
                break
    return count


def with_absent(P, mode, kind, n_seeds=64):
    """A copy of P whose idx tables hold a few -1 (codes absent from the database): kind 'unvisited' - only at (step, code)
    pairs that no walk of the first n_seeds seeds reads; 'losing' - at the LOSING candidate of a state such a walk visits
    (checked here: it still loses when read as candidate 0, and the seeds' walks keep their codes).  mode 0."""
    assert mode == 0
    base = solve(P, mode, P.seed_codes[:n_seeds], P.seed_phases[:n_seeds])
    T0, T1, W0, W1 = P.tables(mode)
    sig = base["sig"]
    Pn = Problem(**{**{k: v for k, v in P.__dict__.items() if k != "_tables"}, "aud_idx": P.aud_idx.copy(),
                    "txt_idx": P.txt_idx.copy()})
    done = 0
    for q in range(1, sig.shape[0]):
        p = np.unique(sig[q] >> 1)
        if kind == "unvisited":
            for W, idx in ((W0, Pn.aud_idx), (W1, Pn.txt_idx)):
                free = np.setdiff1d(W[q], W[q, p])
                if len(free) and done < 6:
                    idx[q, free[0]] = -1
                    done += 1
        else:
            s = int(q % sig.shape[1])
            ps, fi = int(sig[q, s] >> 1), int(sig[q, s] & 1)
            W, idx = (W0, Pn.aud_idx) if fi else (W1, Pn.txt_idx)              # the table of the candidate that lost
            keep = idx[q, W[q, ps]]
            idx[q, W[q, ps]] = -1
            Pn.__dict__.pop("_tables", None)                                    # (the tables follow the idx arrays)
            trial = solve(Pn, mode, P.seed_codes[:n_seeds], P.seed_phases[:n_seeds])
            if np.array_equal(trial["codes"], base["codes"]) and np.array_equal(trial["sig"], base["sig"]):
                done += 1
            else:
                idx[q, W[q, ps]] = keep
            if done >= 3:
                break
    assert done >= 1, "no place for an absent code"
    Pn.__dict__.pop("_tables", None)
    return Pn


# name -> recipe.  K = 512 / N = 32 / M = 3 / steps = 8 is the shape the issue sets for the main comparisons; the others are
# the smallest at which the named path is taken.
CASES = {
    "main": dict(K=512, N=32, M=3, steps=8, Ga=26, Gt=20, recipe="circulant", shift=32, seed=101),
    "distinct": dict(K=512, N=32, M=3, steps=8, Ga=26, Gt=20, recipe="distinct", shift=0, seed=102, plant_modes=(0, 1, 2)),
    "boundary": dict(K=512, N=32, M=1, steps=8, Ga=26, Gt=20, recipe="boundary", seed=103),
    "boundary_r": dict(K=512, N=32, M=1, steps=8, Ga=26, Gt=20, recipe="boundary", seed=103, deep_first=False),
    "boundary528": dict(K=528, N=32, M=1, steps=8, Ga=26, Gt=20, recipe="boundary", seed=120),
    "random": dict(K=512, N=32, M=3, steps=8, Ga=26, Gt=20, recipe="random", seed=104, plant_modes=()),
    "m1": dict(K=512, N=32, M=1, steps=8, Ga=26, Gt=20, recipe="circulant", shift=64, seed=105),
    "batch": dict(K=512, N=32, M=10, steps=8, Ga=26, Gt=20, recipe="circulant", shift=96, seed=106, plant_modes=()),
    "k528": dict(K=528, N=32, M=3, steps=8, Ga=26, Gt=20, recipe="circulant", shift=32, seed=107),
    "k500": dict(K=500, N=32, M=2, steps=8, Ga=26, Gt=20, recipe="circulant", shift=32, seed=108),
    "k64_g64x1": dict(K=64, N=64, M=3, steps=8, Ga=64, Gt=1, recipe="circulant", shift=32, seed=109),
    "k64_s1": dict(K=64, N=8, M=3, steps=1, Ga=26, Gt=20, recipe="circulant", shift=32, seed=110),
    "k64_s3": dict(K=64, N=8, M=3, steps=3, Ga=26, Gt=20, recipe="circulant", shift=32, seed=111),
    "k64_s7": dict(K=64, N=8, M=3, steps=7, Ga=26, Gt=20, recipe="circulant", shift=32, seed=112),
    "k64_s8": dict(K=64, N=8, M=3, steps=8, Ga=26, Gt=20, recipe="circulant", shift=32, seed=113),
    "k64_s9": dict(K=64, N=8, M=3, steps=9, Ga=26, Gt=20, recipe="circulant", shift=32, seed=114, plant_modes=()),
    "k64_s16": dict(K=64, N=8, M=3, steps=16, Ga=26, Gt=20, recipe="circulant", shift=32, seed=115, plant_modes=()),
    "q2048": dict(K=16, N=8, M=256, steps=8, Ga=26, Gt=20, recipe="circulant", shift=32, seed=116, plant_modes=()),
    "m257": dict(K=16, N=8, M=257, steps=8, Ga=26, Gt=20, recipe="circulant", shift=32, seed=117, plant_modes=()),
    "k1024": dict(K=1024, N=64, M=2, steps=8, Ga=26, Gt=20, recipe="circulant", shift=32, seed=118),
    "k768_s16": dict(K=768, N=48, M=2, steps=16, Ga=26, Gt=20, recipe="circulant", shift=32, seed=119, plant_modes=()),
}
ADVERSARIAL = ("main", "distinct", "boundary", "k528", "k500", "k64_g64x1", "k64_s7", "k1024")


@functools.lru_cache(maxsize=None)
def case(name):
    """The Problem of a case (built once; nobody writes to it afterwards), with .plants {mode: counts}."""
    c = dict(CASES[name])
    K, Q = c["K"], c["M"] * c["steps"]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    recipe = c["recipe"]
    if recipe in ("circulant", "distinct"):
        pos, freq, ra, rb = circulant_tables(K, Q, c["shift"], c["seed"], swaps=recipe == "circulant")
    elif recipe == "boundary":
        pos, freq, ra, rb = boundary_tables(K, Q, c.get("deep_first", True), c["seed"])[:4]
    else:
        pos, freq, ra, rb = random_tables(K, Q, c["seed"], tie_free=True)
    P = Problem(name=name, K=K, N=c["N"], M=c["M"], steps=c["steps"], pos_rank=pos, freq_rank=freq, aud_rank=ra,
                txt_rank=rb, Tp=TP, code_ld=CODE_LD, **_database(K, c["N"], Q, c["Ga"], c["Gt"], rng, disjoint_slots=recipe == "random"))
    P.plants = {}
    if c["steps"] <= 8:
        for mode in c.get("plant_modes", (0,)):
            P.plants[mode] = plant(P, mode, rng)
    return P
