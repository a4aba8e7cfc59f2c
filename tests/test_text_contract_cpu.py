"""The CPU half of the exact-text / edit-distance contract (tests/text_ref.py; the kernels: tests/test_gpu_text_contract.py):
the NumPy statement agrees with the oracle's C restatement and with a brute-force edit distance, and every case of the
tables meets the conditions under which a bit-for-bit comparison means something - no subnormal square, the planted ties
and threshold rows are what they claim, and three wrong arithmetics of the same sum are told apart in at least 5 % of the
entries of every query row.  Figures are printed (pytest -s)."""
import functools

import numpy as np
import pytest

from oracle import knn_oracle as O
from tests import text_ref as R

CHUNK = 16                                   # queries per evaluation of the [Q][C][Dm] differences
MIN_SHARE = 0.05
MIN_TIED_PAIRS = 20


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- pins ------------------------------------------------------------------------------------------------------------------
def test_dist_f32_equals_the_c_restatement_bit_for_bit():
    """R > 1, G > 1, a non-prefix cand_r, masked codes, a code past the table, copies, zero, tiny and threshold rows, a zero
    query: the per-code tables of dist_f32(l2_normalize ...) are qpg_ref_text_scan's, distances bit for bit."""
    from oracle import cref
    c = R.Case("pin", 13, 6, 5, 48, 11, 7, seed=5)
    assert c.R > 1 and c.G > 1 and (c.code == -1).any() and not np.array_equal(c.cand_r, np.arange(c.G))
    want_d, want_i = cref.text_scan(c.ctx, c.cand_r, c.code.reshape(c.N, c.G).astype(np.int32), np.arange(c.G), c.q, K=c.K)
    D = R.dist_f32(O.l2_normalize(c.q), O.l2_normalize(R.grid_rows(c.ctx, c.cand_r)))
    dist, idx, _, _ = R.percode(D, c.code, c.K, R.ABSENT)
    assert np.array_equal(_bits(dist), _bits(want_d)) and np.array_equal(idx, want_i)
    assert (idx == -1).any() and (idx >= 0).any()


def test_pack_images_put_candidate_c_in_lane_c_mod_64():
    """The two layouts, element by element, on a case with a ragged last tile."""
    c = R.percode_case("c65_q11_k7")
    image, live, xn = R.pack_f32(c.ctx, c.cand_r)
    h = R.percode_case("c65_q11_k7", True)
    image16, live16, nrm, x16 = R.pack_f16(h.ctx, h.cand_r)
    assert image.size == image16.size == 2 * 64 * 16 and live.sum() == live16.sum() == 65 * 16
    for cand, e in ((0, 0), (63, 15), (64, 0), (64, 15), (17, 6)):
        at = (cand // 64) * 16 * 64 + ((e // 4) * 64 + cand % 64) * 4 + e % 4
        assert live[at] and _bits(image[at:at + 1]) == _bits(xn[cand, e:e + 1])
        at = (cand // 64) * 16 * 64 + ((e // 8) * 64 + cand % 64) * 8 + e % 8
        assert live16[at] and image16[at:at + 1].view(np.uint16) == x16[cand, e:e + 1].view(np.uint16)
    assert np.isnan(image[~live]).all() and np.isnan(image16[~live16]).all() and not np.isnan(image[live]).any()
    j, g = divmod(17, c.G)
    assert np.array_equal(xn[17], O.l2_normalize(c.ctx[j, c.cand_r[g]][None])[0])
    assert nrm[4] == 1 and not x16[4].any()                              # the tiny row: f16 zeros, norm 0 -> 1


def _lev_brute(a, b):
    """Edit distance by its recursive definition (memoised), not the row-by-row DP of knn_oracle.lev."""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (a[i - 1] != b[j - 1]))
    return d(len(a), len(b))


def test_lev_matrix_equals_the_brute_force_distance():
    from qpgesture_amd.code_knn import wavvq_tap_offsets
    for T in (40, 398):
        assert R.tap_offsets(T) == wavvq_tap_offsets(T)
    rng = np.random.default_rng(0)
    T, taps = R.LEV_T, R.tap_offsets(R.LEV_T)
    sym_db = rng.integers(0, 4, size=(4, T)).astype(np.int32)
    sym_q = rng.integers(0, 4, size=(4, T)).astype(np.int32)
    sym_q[1] = sym_db[2]                                                  # equal strings at equal frames
    sym_q[2] = sym_db[1] + 1000                                           # disjoint alphabets: every symbol substituted
    sym_q[3, :-1] = sym_db[3, 1:]                                         # a shift by one frame
    cand_t = np.array([0, 39, 20, 7], np.int32)
    q_win = np.repeat(np.arange(4), 4).astype(np.int32)
    q_t = np.tile(np.array([0, 39, 20, 6], np.int32), 4)
    D = R.lev_matrix(sym_db, cand_t, taps, sym_q, q_win, q_t)
    assert D.dtype == np.float32 and D.shape == (16, 16)
    for q in range(16):
        a = [sym_q[q_win[q], q_t[q] + o] if 0 <= q_t[q] + o < T else 0 for o in taps]
        for j in range(4):
            for g in range(4):
                b = [sym_db[j, cand_t[g] + o] if 0 <= cand_t[g] + o < T else 0 for o in taps]
                assert D[q, j * 4 + g] == _lev_brute(tuple(a), tuple(b))
    assert (D[4:7, 2 * 4:2 * 4 + 3].diagonal() == 0).all()                # window 1 against database window 2, same frames
    assert D[10, 1 * 4 + 2] == 11                                         # disjoint, no padding on either side (frame 20)
    assert D[8, 1 * 4 + 0] == 6                                           # disjoint at frame 0: the 5 padded back taps match
    assert D[15, 3 * 4 + 3] == 0                                          # the shifted window at frame 6 IS the window at 7 ...
    assert D[12, 3 * 4 + 0] <= 3                                          # ... at equal frames: drop one, swap one, add one
    for a, b, want in (((1, 2, 3), (1, 2, 3), 0), ((1, 2, 3), (4, 5, 6), 3), ((1, 2, 3, 4), (2, 3, 4, 5), 2), ((), (1, 2), 2)):
        assert O.lev(a, b) == _lev_brute(a, b) == want


# ---- conditions, per case -----------------------------------------------------------------------------------------------
def _case_params():
    return [pytest.param(c, id=c) for c in
            ["sweep/" + n for n in R.SWEEP_CASES] + ["percode/" + n for n in R.PERCODE_CASES] + ["half/" + n for n in R.HALF_CASES]]


def _case(cid):
    kind, name = cid.split("/")
    return R.sweep_case(name) if kind == "sweep" else R.percode_case(name, kind == "half")


def _copies(qn, xn):
    """[Q][C]: row c is bit for bit query q."""
    return (_bits(qn)[:, None, :] == _bits(xn)[None, :, :]).all(axis=2)


@pytest.mark.parametrize("cid", _case_params())
def test_case_conditions(cid):
    c = _case(cid)
    assert c.name == cid
    tiny = R.F32_MIN_NORMAL
    # -- no subnormal square: in the norms (raw values as the kernels read them) and in the distances of live pairs
    raw = c.packed[3].astype(np.float32) if c.half else c.rows
    for v in (raw, c.q):
        sq = v * v
        assert not ((sq != 0) & (sq < tiny)).any(), "a squared entry is subnormal"
    for q0 in range(0, c.Q, CHUNK):
        d, sq = R._sq_diffs(c.qn[q0:q0 + CHUNK], c.xn)
        assert not ((sq != 0) & (sq < tiny)).any() and not ((d != 0) & (np.abs(d) < tiny)).any(), "a subnormal difference"
    # -- what was planted is there
    if c.C >= 12:
        norms = np.sqrt(O.einsum_sq(raw))
        # ("just": 1 % in f32; the f16-rounded rows are made of a few units of 2^-24 per entry and move in coarser steps)
        near = 0.1 if c.half else 0.01
        assert (1 - near) * R.THRESHOLD < norms[c.below] < R.THRESHOLD <= norms[c.above] < (1 + near) * R.THRESHOLD
        assert not raw[3].any() and not raw[c.C - 1].any() and 0 < np.sqrt(O.einsum_sq(c.rows[4])) < 0.5 * R.THRESHOLD
        assert np.abs(c.xn[c.below]).max() < 1e-5 and abs(float(O.einsum_sq(c.xn[c.above])) - 1) < 1e-5
        if c.half:
            f32_norm = np.sqrt(O.einsum_sq(c.rows[c.f16_only_below]))
            assert f32_norm >= R.THRESHOLD > norms[c.f16_only_below] > 0 and c.packed[2][c.f16_only_below] == 1
            assert c.rows[4].all() and not raw[4].any()                   # entries that round to f16 zero
        src = _bits(raw[1])
        assert all(np.array_equal(_bits(raw[i]), src) for i in c.copies)
        assert (c.code == -1).any() or c.C == 12
        assert c.code[0] == c.K and (c.code < c.K).sum() == c.C - 1
        if c.Q >= 2:
            assert _copies(c.qn[c.Q - 1:], c.xn)[0, list(c.copies)].all()  # 2 x the source normalises to the source's row
        if c.Q >= 3:
            assert not c.qn[c.Q // 2].any()
    if c.K >= 2:
        assert c.empty_code not in c.code
    pairs, shared = R.tie_counts(c.D, c.code, c.K)
    print("TEXTCONTRACT %-32s ties: %d (query, code) pairs tied inside the code, %d queries with a shared global minimum"
          % (cid, pairs, shared))
    if c.ties:
        assert pairs >= MIN_TIED_PAIRS and shared >= 1
    # -- negative control
    xn = R.control_rows(c)
    worst = {}
    for q0 in range(0, c.Q, CHUNK):
        qn = c.qn[q0:q0 + CHUNK]
        right = _bits(R.dist_f32(qn, xn))
        judged = ~_copies(qn, xn)
        assert (judged.sum(axis=1) >= R.CONTROL_ROWS - 16).all()
        for name, D in R.wrong_dists(qn, xn).items():
            share = ((_bits(D) != right) & judged).sum(axis=1) / judged.sum(axis=1)
            worst[name] = min(worst.get(name, 1.0), float(share.min()))
    print("TEXTCONTRACT %-32s control over %d rows, lowest share of differing entries in a query row: %s"
          % (cid, xn.shape[0], "  ".join("%s %.1f %%" % (n, 100 * s) for n, s in sorted(worst.items()))))
    assert min(worst.values()) >= MIN_SHARE, worst


@pytest.mark.parametrize("name", list(R.LEV_CASES))
def test_lev_case_conditions(name):
    """Both paddings are read, next to real zeros; the matrix is small integers with ties inside codes."""
    c = R.lev_case(name)
    T = c.T
    assert len(c.taps) == 11 and min(c.taps) < 0 < max(c.taps)
    if c.G >= 2:
        assert 0 in c.cand_t and T - 1 in c.cand_t
    if c.Q >= 3:
        assert {0, T - 1} <= set(c.q_t.tolist()) and ((c.q_t > 6) & (c.q_t < T - 7)).any()
    assert c.q_win.max() == c.Mq - 1 and (c.sym_db[0, :3] == 0).all() and (c.sym_db[-1, T - 3:] == 0).all()
    assert c.sym_db.max() == 319 * 320 + 319
    D = c.D
    assert np.array_equal(D, np.round(D)) and D.min() >= 0 and D.max() <= 11
    pairs, shared = R.tie_counts(D, c.code, c.K)
    print("TEXTCONTRACT lev/%-28s ties: %d (query, code) pairs tied inside the code, %d queries with a shared global minimum"
          % (name, pairs, shared))
    if c.C >= 255 and c.Q >= 7:
        assert pairs >= MIN_TIED_PAIRS and shared >= 1
