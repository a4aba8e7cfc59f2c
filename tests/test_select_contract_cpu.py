"""The CPU half of the select contract (tests/select_ref.py; the kernels: tests/test_gpu_select_contract.py): the exact
reference agrees with the oracle's C restatement, every noise pattern stays within its amplitude after the rounding to the
matrix's storage type, the `swap` pattern really hands the select reversed comparisons, and every case of the GPU test's
table meets the conditions under which its verdict is determined by the input (`admissible`).  The band populations are
printed (pytest -s)."""
import numpy as np
import pytest

from tests import select_ref as R
from tests.helpers import fixture_arrays, load_golden


def _product():
    from qpgesture_amd.code_knn import AUDIO_HL_BAND, AUDIO_HL_ERR
    assert abs(AUDIO_HL_BAND / AUDIO_HL_ERR - R.BAND_RATIO) < 1e-12
    return R.product_case(AUDIO_HL_ERR, AUDIO_HL_BAND)


def _all_audio_cases():
    return [R.audio_case(n) for n in R.AUDIO_CASES] + [_product()]


def test_exact_audio_reproduces_the_oracle_on_a_shipped_golden():
    from oracle import cref, knn_oracle as O
    g = load_golden("shipped_n48_m2_s0")
    ntr, nte, s0, s1, s2, s3, mf = [int(v) for v in g["meta"]]
    A = fixture_arrays(ntr, nte, s0, s1, s2, s3)
    q = np.stack([O.wavlm_feat_rows(A["te_interp"], 0, [24 * s])[0] for s in range(6)])
    cand_t = np.arange(26) * 6
    d_ref, i_ref = cref.audio_scan(A["tr_interp"], cand_t, A["code"], np.arange(26), q)
    D = R.exact_audio(A["tr_interp"], cand_t, 6, 2, q.astype(np.float32))
    dist, idx, rank = R.tables(D, A["code"][:, :26].reshape(-1), 512, R.ABSENT)
    assert np.array_equal(idx, i_ref)
    assert np.abs(dist - d_ref).max() <= 1e-13
    assert np.array_equal(dist[:6], np.where(g["aud_dist"][:6] == 1e3, 1e3, dist[:6]))      # the same codes are absent
    assert np.abs(dist - g["aud_dist"][:6]).max() <= 1e-13                                  # ... and the REFERENCE's values


def test_exact_audio_reproduces_the_oracle_on_a_small_case_with_planted_rows():
    from oracle import cref
    c = R.audio_case("odd")                                    # zero window, exact copies, masked candidates, an absent code
    d_ref, i_ref = cref.audio_scan(c.base, c.cand_t, c.cand_code.reshape(c.N, 26).astype(np.int32), np.arange(26),
                                   c.q32.astype(np.float64), K=c.K)
    dist, idx, rank = c.ref
    assert np.array_equal(idx, i_ref)
    assert np.abs(dist - d_ref).max() <= 1e-13
    assert (idx == -1).any() and (c.cand_code == -1).any()
    zero = c.exact[:, 3 * 26:4 * 26]
    assert np.array_equal(zero, np.full_like(zero, 0.5))       # the library's degenerate-row rule: exactly 0.5
    assert np.array_equal(c.exact[:, 26:52], c.exact[:, 5 * 26:6 * 26])       # bit-identical rows: bit-identical distances


def test_tables_first_wins_and_stable_ranks():
    D = np.array([[3.0, 1.0, 1.0, 2.0, 0.5, 2.0]])
    dist, idx, rank = R.tables(D, [0, 1, 1, 2, 7, -1], 4, 1e3)
    assert dist.tolist() == [[3.0, 1.0, 2.0, 1e3]] and idx.tolist() == [[0, 1, 3, -1]] and rank.tolist() == [[2, 0, 1, 3]]
    dist, idx, rank = R.tables(np.array([[1.0, 1.0]]), [1, 0], 2, 1e3)
    assert rank.tolist() == [[0, 1]]                           # equal minima: the lower code ranks first


@pytest.mark.parametrize("kind", R.NOISES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_noise_stays_within_its_amplitude_after_rounding(kind, dtype):
    for c in _all_audio_cases():
        D_in = R.noisy(kind, c.exact, c.cand_code, c.K, c.E, dtype, seed=3)      # (asserts the bound itself)
        err = np.abs(D_in.astype(np.float64) - c.exact).max()
        assert D_in.dtype == dtype and err <= c.E
        if kind != "zero":
            assert err >= 0.9 * c.E                            # ... and uses the width: this is worst-case noise
    t = R.text_case()
    live = t.layout[1] >= 0
    err = np.abs(t.noisy(kind)[:, live].astype(np.float64) - t.d_sorted[:, live]).max()
    assert err <= t.e and (kind == "zero" or err >= 0.9 * t.e)


def test_swap_noise_reverses_same_code_and_rank_neighbour_pairs():
    for c in _all_audio_cases():
        for dtype in (np.float32, np.float64):
            D_in = R.noisy("swap", c.exact, c.cand_code, c.K, c.E, dtype)
            same, nb = R.reversals(c.exact, D_in, c.cand_code, c.K)
            print("%-12s %s: %d same-code and %d rank-neighbour comparisons arrive reversed" % (c.name, np.dtype(dtype).name, same, nb))
            assert same >= 1 and nb >= 1
        assert R.reversals(c.exact, R.noisy("zero", c.exact, c.cand_code, c.K, c.E, np.float64), c.cand_code, c.K) == (0, 0)
    t = R.text_case()
    live = t.layout[1] >= 0
    same, _ = R.reversals(t.d_sorted[:, live].astype(np.float64), t.noisy("swap")[:, live], t.layout[2][live], t.K)
    print("text: %d same-code comparisons arrive reversed" % same)
    assert same >= 1


def test_every_gpu_case_is_admissible():
    for c in _all_audio_cases():
        v = c.verdict
        print("%-12s N=%d Q=%d K=%d F=%d E=%.3g eps1=%.3g: admissible=%s; listed-pair bound max %d (capacity %d), mean %.1f "
              "(%.1f same-code candidates + %.1f rank-neighbour winners per query) %s"
              % (c.name, c.N, c.Q, c.K, c.F, c.E, c.eps1, v["ok"], v["listed_max"], R.MIX_LIST, v["listed_mean"],
                 v["band_members"], v["rank_members"], v["why"]))
        assert v["ok"], (c.name, v["why"])
    t = R.text_case()
    v = t.verdict
    print("text         n=%d D=%d K=%d Q=%d band=%.3g e=%.3g: admissible=%s; R=%d, by-code pair bound max %d per tile (capacity "
          "%d), %.1f band rows per query (%.1f beyond the winners) %s"
          % (t.n, t.D, t.K, t.Q, t.band, t.e, v["ok"], v["R"], v["tile_pairs_max"], R.BYC_LIST, v["band_rows_mean"],
             v["extra_mean"], v["why"]))
    assert v["ok"], v["why"]


@pytest.mark.parametrize("name,listed_max", [("odd", 27), ("base", 46), ("f16_track", 44), ("wavlm_width", 38)])
def test_f64_select_cases_are_admissible_at_eps_1e_12(name, listed_max):
    """The condition that keeps the direct test of qpg_percode_select_guarded_f64 / _exact_f64 decisive: handed the exact
    distances (E = 0) with a band of 1e-12, nothing that matters is closer than 1e-10 unless its rows are identical, at most
    half of the guarded select's 256-entry list is used, and the band is not empty."""
    c = R.audio_case(name)
    v = R.admissible(c.exact, c.cand_code, c.K, 1e-12, 0.0, 1e-12, row_id=c.row_id, capacity=256, min_mean=1)
    print("%-12s eps=1e-12: admissible=%s; listed max %d (capacity 256), %.1f same-code candidates + %.1f rank-neighbour "
          "winners per query %s" % (name, v["ok"], v["listed_max"], v["band_members"], v["rank_members"], v["why"]))
    assert v["ok"], v["why"]
    assert v["listed_max"] == listed_max
    assert name == "odd" or v["rank_members"] > 3


def test_negative_controls_are_determined_by_their_inputs():
    """A band of 1.05 E under swap noise of amplitude E cannot hold a pair whose exact gap is below 0.95 E (the two arrive
    2 E - gap > 1.05 E apart, reversed): such pairs exist in the cases the GPU negative controls use."""
    c = R.audio_case("base")
    same, nb = R.has_gap_below(c.exact, c.cand_code, c.K, 0.95 * c.E)
    print("base: %d same-code and %d rank-neighbour pairs with an exact gap below 0.95 E" % (same, nb))
    assert same >= 1 or nb >= 1
    t = R.text_case()
    live = t.layout[1] >= 0
    same, _ = R.has_gap_below(t.d_sorted[:, live].astype(np.float64), t.layout[2][live], t.K, 0.95 * t.e)
    print("text: %d same-code pairs with an exact gap below 0.95 e" % same)
    assert same >= 1


def test_the_text_case_has_its_planted_rows():
    t = R.text_case()
    row_index, src, seg, zero_row = t.layout
    n_rows = np.bincount(seg[row_index >= 0], minlength=t.K)
    assert n_rows[0] == 1 and n_rows[1] == 16 and n_rows[2] == 17 and n_rows[3] == 0
    assert (zero_row >= 0).sum() >= 2 and (t.codes_masked < 0).sum() > 50
    assert n_rows[9] < (t.codes_masked == 9).sum()             # the exact duplicates of a code were dropped by the builder
    dist, idx, rank, nn = t.ref
    assert (idx[:, 3] == -1).all() and nn[7] == 699            # the absent code; the query that is a (duplicated) row
    assert len(src) % 64 == 0 and (seg[::16] == seg[15::16]).all()          # a tile lies inside one code


def test_the_overflow_case_overflows_query_0_and_leaves_query_1_ordinary():
    """tests/test_gpu_scratch_contract.py's `overflow` case: 2080 candidates under one code.  Whatever matrix within E of the
    exact distances the select is handed, a candidate within eps1 - 2 E of its code's exact minimum is within eps1 of the
    approximate one: query 0 has more of those than a tier-1 list holds, so the list MUST overflow.  A candidate outside
    eps1 + 2 E cannot be listed: query 1 stays below half the capacity."""
    c = R.audio_case("overflow")
    assert c.C == 80 * 26 == 2080 > R.MIX_LIST and (c.cand_code == 3).all() and c.Q == 2
    surely, possibly = R.band_counts(c, c.eps1 - 2 * c.E), R.band_counts(c, c.eps1 + 2 * c.E)
    print("overflow case: query 0 lists %d .. %d of %d candidates, query 1 %d .. %d (capacity %d)"
          % (surely[0], possibly[0], c.C, surely[1], possibly[1], R.MIX_LIST))
    assert surely[0] > R.MIX_LIST
    assert possibly[1] < R.MIX_LIST // 2
    assert surely[1] >= 1 and np.ptp(c.exact[1]) > 10 * c.eps1           # an ordinary row: a spread far wider than the band
