"""Test-side statement of the walk WITHOUT the phase gate (search_code_knn(use_phase=False), GestureKNN.py:578-592, and the
window loop around it, :785-813): what qpg_match_steps_nophase must leave in its workspace and outputs for a
tests/walk_ref.Problem.  Plain NumPy, no torch, no GPU; not itself a test.

Per step, with p the previous code:
  mode 0 (audio + text)  combined = (pos_score + aud_rank) + txt_rank;  c* = position k of the sorted order;  the step's
                         coin picks the audio (nonzero) or the text candidate of c*                              (:578-586)
  mode 1 (audio)         combined = pos_score + aud_rank, the audio candidate of c*                             (:587-589)
  mode 2 (text)          combined = pos_score + txt_rank, the text candidate of c* (the reference's :591 names a variable
                         that does not exist there; this is its evident intent)
pos_score = pos_rank[p] + freq_rank * 0.05, everything f64 in that order.  Equal scores in code order (the library's rule).
The next previous code is the 4th code of the appended block; a window keeps codes_per_window of its codes and the next
window starts from the last KEPT one."""
import numpy as np

from tests import walk_ref as W

KMAX = 16                    # QPG_NOPHASE_KMAX
NONE16 = 0xFFFF


def scores(P, mode, q):
    """combined[p][c] of step q for every previous code p, f64 [K][K]."""
    pos = P.pos_rank.astype(np.float64) + (P.freq_rank.astype(np.float64) * 0.05)[None, :]
    if mode == 0:
        return (pos + P.aud_rank[q].astype(np.float64)[None, :]) + P.txt_rank[q].astype(np.float64)[None, :]
    return pos + (P.aud_rank if mode == 1 else P.txt_rank)[q].astype(np.float64)[None, :]


def orders(P, mode):
    """The first KMAX codes of the order by (score, code) for every (q, p): int64 [Q][K][KMAX] (built once per problem)."""
    cache = P.__dict__.setdefault("_nophase_orders", {})
    if mode not in cache:
        Q = (P.aud_rank if mode != 2 else P.txt_rank).shape[0]
        out = np.empty((Q, P.pos_rank.shape[0], KMAX), np.int64)
        rows = np.arange(P.pos_rank.shape[0])
        for q in range(Q):
            s = scores(P, mode, q)
            for k in range(KMAX):                 # (argmin: the lowest code among equal scores; KMAX passes beat a full sort)
                out[q, :, k] = s.argmin(axis=1)
                s[rows, out[q, :, k]] = np.inf
        cache[mode] = out
    return cache[mode]


def sides_of(mode):
    return {0: (0, 1), 1: (0,), 2: (1,)}[mode]


def tables(P, mode, k, M=None):
    """next int64 [Q][2][K] (NONE16: no state) and pick int64 [Q][2][K] (-1: none) - qpg_match_steps_nophase's workspace.
    M: windows per chain (the window geometry repeats every M x steps rows; default the problem's)."""
    cstar = orders(P, mode)[:, :, k]                                           # [Q][K]
    Q, K = cstar.shape
    nxt = np.full((Q, 2, K), NONE16, np.int64)
    pick = np.full((Q, 2, K), -1, np.int64)
    q = np.arange(Q)[:, None]
    off = np.where(q % P.steps == P.steps - 1, (P.codes_per_window - 1) % W.STEP_CODES, W.STEP_CODES - 1)
    for s in sides_of(mode):
        idx, cidx, G = (P.txt_idx, P.txt_cidx, len(P.txt_cidx)) if s else (P.aud_idx, P.aud_cidx, len(P.aud_cidx))
        cand = idx[q, cstar].astype(np.int64)
        cand = np.where(cand < 0, -1, cand)
        cc = np.where(cand < 0, 0, cand)
        j, g = cc // G, cc % G
        cv = P.code[j, np.asarray(cidx, np.int64)[g] + off].astype(np.int64)
        pick[:, s] = cand
        nxt[:, s] = np.where((cand >= 0) & (cv >= 0) & (cv < K), cv, NONE16)
    return nxt, pick


def walk(P, mode, k, seed_code, coins=None, M=None, q0=0, tabs=None):
    """One chain of M windows over table rows [q0, q0 + M steps).  coins: [M steps], nonzero = audio (mode 0).
    -> dict(codes int64 [M][codes_per_window], side [M steps], cand [M steps], status0); what the chain does not reach: -1."""
    M = P.M if M is None else M
    nxt, pick = tables(P, mode, k) if tabs is None else tabs
    K = nxt.shape[2]
    Q, cpw = M * P.steps, P.codes_per_window
    side = np.full(Q, -1, np.int64)
    cand = np.full(Q, -1, np.int64)
    blocks = np.full((Q, W.STEP_CODES), -1, np.int64)
    p, bad = int(seed_code), 0
    if not 0 <= p < K:
        bad = 1
    for q in range(Q if not bad else 0):
        s = sides_of(mode)[0] if mode else (0 if coins[q] else 1)
        side[q], cand[q] = s, pick[q0 + q, s, p]
        if cand[q] >= 0:
            cidx, G = (P.txt_cidx, len(P.txt_cidx)) if s else (P.aud_cidx, len(P.aud_cidx))
            j, g = divmod(int(cand[q]), G)
            blocks[q] = P.code[j, int(cidx[g]):int(cidx[g]) + W.STEP_CODES]
        n = int(nxt[q0 + q, s, p])
        if n == NONE16:
            bad = 1
            break
        p = n
    codes = blocks.reshape(M, P.steps * W.STEP_CODES)[:, :cpw]
    return dict(codes=np.ascontiguousarray(codes), side=side, cand=cand, status0=bad)


def kth_stable(score, k):
    """Position k of the order by (score, index) of one score row."""
    return int(np.argsort(np.asarray(score), kind="stable")[k])


def replay_golden(g):
    """A golden fixture of tests/golden/make_golden_nophase.py walked from what it captured: per step the code at position
    desired_k of the captured combined_score under the (score, code) order, the captured coin, the captured payloads.
    -> (knn_pred int64 [M][30], chosen codes [Q], sides [Q])."""
    k = int(g["desired_k"])
    comb, coins = g["step_combined_score"], g["coins"]
    two = "txt_pay" in g.files
    Q = comb.shape[0]
    steps = 8
    M = Q // steps
    result, chosen, sides = [], [], []
    for q in range(Q):
        c = kth_stable(comb[q], k)
        s = (0 if coins[q] > 0.5 else 1) if two else 0
        pay = (g["txt_pay"] if s else g["aud_pay"])[q, c]
        result.append([int(v) for v in pay if v >= 0])
        chosen.append(c)
        sides.append(s)
    pred = np.array([sum(result[w * steps:(w + 1) * steps], [])[:30] for w in range(M)], np.int64)
    return pred, np.array(chosen), np.array(sides)
