"""CPU side of the walk contract (tests/walk_ref.py; the kernels are compared with it in tests/test_gpu_walk_contract.py):
  * the NumPy walk is PINNED to what the reference project produced - knn_pred, vote and phase_out of every shipped_*
    golden and of the two wavvq goldens (modes 0 and 1) - from the arrays qpg_match_steps consumes;
  * chase(gate_table) == the literal walk on every adversarial case; gate == sklearn's paired cosine distance;
  * the adversarial inputs meet the CONDITIONS that make them adversarial (ties at the fused minimum, winners at every
    depth of the rank order, 1 024 distinct gate keys in a step, reached gate ties / near ties / 10 eps evaluations);
  * NEGATIVE CONTROLS: each deliberately wrong variant of the reference disagrees with it on the adversarial inputs and
    agrees on the random-permutation control.
Lines starting with WALKREF carry the measured counts (profiles/walk_contract.md)."""
import functools

import numpy as np
import pytest

from oracle import knn_oracle as O
from qpgesture_amd import synth
from tests import select_ref as R
from tests import walk_ref as W
from tests.helpers import load_golden

SHIPPED = ["shipped_n48_m2_s0", "shipped_n64_m3_s10", "shipped_n256_m2_s70", "shipped_neartie_n48_m2_s30",
           "shipped_texttie_n48_m2_s40", "shipped_nearsilent_n48_m2_s50", "shipped_speechlike_n48_m2_s60"]
WAVVQ = [("wavvq_aud_txt_n40_m2_s20", 0), ("wavvq_aud_n40_m2_s20", 1)]


# ---- the reference against the goldens ---------------------------------------------------------------------------------------
def _pos_rank(sig):
    """Stable ranks of the pose-signature distances |sig[p] - sig[c]| (f32 difference, one rounding of the norm to f32,
    +inf for the code itself: qpg_l2_table_f32 + qpg_rank_rows_f32 - the library's statement; the reference's f32
    np.linalg.norm can order two nearly equal distances the other way, DESIGN.md "Tie contract")."""
    sig = np.asarray(sig, np.float32)
    d = np.empty((sig.shape[0],) * 2, np.float32)
    for p in range(sig.shape[0]):
        diff = (sig[p][None] - sig).astype(np.float32)
        d[p] = np.sqrt((diff.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
        d[p, p] = np.inf
    return W.stable_rank(d)


def _golden_ranks(g, dist_key, score_key):
    """The rank rows the reference itself used: step_combined_score - step_pos_score.  They are the stable ranks of the
    golden distances wherever a distance is unique in its row; among EQUAL distances (absent codes at 1e+3, repeated
    context rows, integer Levenshtein distances) the reference's unstable argsort chose an order of its own, and the walk
    is pinned on that order - as tests/test_gpu_matching.py::_build takes the reference's frequency ranks."""
    rank = np.rint(g[score_key] - g["step_pos_score"]).astype(np.int64)
    dist = np.asarray(g[dist_key])
    stable = W.stable_rank(dist)
    for q in range(rank.shape[0]):
        assert np.array_equal(np.sort(rank[q]), np.arange(rank.shape[1]))
        by_rank = dist[q][np.argsort(rank[q])]
        assert (np.diff(by_rank) >= 0).all()                                    # a valid ranking of these distances
        _, inv, cnt = np.unique(dist[q], return_inverse=True, return_counts=True)
        lone = cnt[inv.reshape(-1)] == 1
        assert np.array_equal(rank[q][lone], stable[q][lone])
    return rank


def _golden_problem(name, wavvq=False):
    g = load_golden(name)
    ntr, nte, s0, s1, s2, s3, mf = [int(v) for v in g["meta"]]
    variant = (str(g["variant"]) or None) if "variant" in g.files else None
    dim = 1024 if variant else 8                       # (the variants draw from the rng AFTER arrays of the track's width)
    tr, te, code = synth.make_db(ntr, s0, dim), synth.make_db(nte, s1, dim), synth.make_codes(ntr, s2)
    synth.apply_variant(tr, te, code, variant)
    ph = tr["phase_dense"]
    ks, kint, cidx = O.audio_grid(398, 398 / 30) if wavvq else O.audio_grid(180, 6)
    at = {k: i for i, k in enumerate(kint)}
    tk = list(range(0, 240 - 32, 8))
    P = W.Problem(K=512, M=nte, steps=8, pos_rank=_pos_rank(synth.make_signature(s3)),
                  freq_rank=np.asarray(g["step_freq_score"]), code=np.asarray(code),
                  phase=np.ascontiguousarray(np.concatenate((ph[:, :, 0], ph[:, :, 2]), axis=2)),
                  aud_cidx=np.array(cidx), aud_pslot=np.array([O.phase_slot(k) for k in kint]),
                  txt_cidx=np.array([k // 8 for k in tk]), txt_pslot=np.array([O.phase_slot(k) for k in tk]),
                  aud_rank=None, aud_idx=None, txt_rank=None, txt_idx=None)
    gj, gk = g["aud_aux"][..., 0], g["aud_aux"][..., 1]
    P.aud_idx = np.where(gj >= 0, gj * len(kint) + np.vectorize(lambda k: at.get(int(k), 0))(gk), -1)
    P.aud_rank = _golden_ranks(g, "aud_dist", "step_combined_score")
    if "txt_aux" in g.files:
        gj, gk = g["txt_aux"][..., 0], g["txt_aux"][..., 1]
        P.txt_idx = np.where(gj >= 0, gj * 26 + gk // 8, -1)
        P.txt_rank = _golden_ranks(g, "txt_dist", "step_combined_score_")
    return P, g


def _check_golden(P, g, mode):
    codes, votes, phases, bad = W.walk(P, mode, int(g["init_code"]), g["init_phase"])
    assert bad == 0
    assert np.array_equal(codes, g["knn_pred"])
    if mode == 0:                                    # (the one-modality golden recorded the codes only)
        assert np.array_equal(votes, g["vote"])
        assert phases.dtype == np.float32 and np.array_equal(phases, g["phase_out"])
    else:
        assert g["vote"].size == 0
    # ... and the tabulated form of the reference gives the same walk
    sol = W.solve(P, mode, [int(g["init_code"])], np.asarray(g["init_phase"])[None])
    assert np.array_equal(sol["codes"][0], codes) and np.array_equal(sol["vote"][0], votes)
    assert np.array_equal(sol["phase"][0], phases)


@pytest.mark.parametrize("name", SHIPPED)
def test_reference_walk_equals_the_shipped_goldens(name):
    P, g = _golden_problem(name)
    _check_golden(P, g, 0)


@pytest.mark.parametrize("name,mode", WAVVQ)
def test_reference_walk_equals_the_wavvq_goldens(name, mode):
    P, g = _golden_problem(name, wavvq=True)
    _check_golden(P, g, mode)


def test_gate_equals_sklearn_bit_for_bit():
    pd = pytest.importorskip("sklearn.metrics.pairwise")
    P = W.case("distinct")
    T0, T1 = P.tables(0)[:2]
    g = P.grids(0)
    p = P.seed_codes
    for head in (W.cand_head(P, g[0], T0[0, p]), W.cand_head(P, g[1], T1[0, p])):
        a, b = W.gate_vectors(P.seed_phases, head)
        want = pd.paired_distances(a, b, metric="cosine")
        got = W.gate(P.seed_phases, head)
        assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want)
        tiny = (np.sqrt(O.einsum_sq(a)) < W.EPS10) | (np.sqrt(O.einsum_sq(b)) < W.EPS10)
        assert tiny.any() and not tiny.all()                 # the 10 eps rule is part of what was compared


@pytest.mark.parametrize("name", W.ADVERSARIAL + ("random",))
def test_chase_of_the_gate_table_equals_the_literal_walk(name):
    P = W.case(name)
    n = 50
    pick = np.r_[np.arange(0, len(P.seed_codes), len(P.seed_codes) // n)[:n]]
    for mode in (0, 1, 2):
        sol = W.solve(P, mode, P.seed_codes[pick], P.seed_phases[pick])
        for i, s in enumerate(pick if mode == 0 else pick[:8]):
            codes, votes, phases, bad = W.walk(P, mode, P.seed_codes[s], P.seed_phases[s])
            assert np.array_equal(codes, sol["codes"][i]) and np.array_equal(votes, sol["vote"][i])
            assert np.array_equal(phases, sol["phase"][i]) and bad == sol["status0"][i]


# ---- conditions on the inputs ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _circulant_stats():
    tot = dict(ties=0, deeper=0, int_differs=0)
    for pos, freq, ra, _ in W.circulant_set():
        st = W.tie_stats(pos, freq, ra)
        for k in tot:
            tot[k] += st[k]
    return tot


def test_circulant_recipe_ties_and_depth():
    """16 databases x 22 rows x 512 previous codes."""
    tot = _circulant_stats()
    print("WALKREF circulant ties %(ties)d lowest_index_deeper %(deeper)d int_scaled_differs %(int_differs)d" % tot)
    assert tot["ties"] >= 10000 and tot["deeper"] >= 5000 and tot["int_differs"] >= 3


def test_random_recipe_is_the_weak_control():
    pos, freq, ra, _ = W.random_tables(512, 24, 104)                # (as drawn: the control of the controls is tie-free)
    st = W.tie_stats(pos, freq, ra)
    print("WALKREF random ties %d deepest_winner %d mean_depth %.1f" % (st["ties"], st["depth"].max(), st["depth"].mean()))
    assert st["ties"] < 100 and st["depth"].max() < 128


def test_distinct_winners_fill_the_dedup_hash_and_every_depth():
    P = W.case("distinct")
    T0, T1, W0, W1 = P.tables(0)
    keys = [len(np.unique(T0[q])) + len(np.unique(T1[q])) for q in range(P.Q)]
    depth = np.take_along_axis(P.aud_rank.astype(np.int64), W0, axis=1)
    print("WALKREF distinct keys_per_step %d..%d depth>=64 %d depth>=448 %d of %d" %
          (min(keys), max(keys), (depth >= 64).sum(), (depth >= 448).sum(), depth.size))
    assert max(keys[1:]) == 1024                                  # (candidate, table) keys of one step q >= 1
    assert np.array_equal(np.unique(depth), np.arange(512))       # every depth of the rank order
    assert (depth >= 64).sum() == 10752 and (depth >= 448).sum() == 1536


@pytest.mark.parametrize("deep_first", [True, False])
def test_boundary_recipe_plants_the_tie_on_the_round_boundary(deep_first):
    pos, freq, ra, rb, planted, deep, shallow = W.boundary_tables(512, 8, deep_first, 103)
    win = W.fuse(pos, freq, ra)[..., 0]
    assert planted.sum() >= 8 * 120 and (deep < shallow) == deep_first
    assert (win[planted] == min(deep, shallow)).all()
    for q in range(8):
        B = W.BOUNDARIES[q % 4]
        assert ra[q, deep] == B and ra[q, shallow] < 64            # one inside the first round, one ON a later round's start


@pytest.mark.parametrize("name", ["distinct", "main", "k528", "k64_s7", "k1024"])
def test_gate_cases_are_reached(name):
    """Among the states the tested seeds reach (all 1 000 seeds: the takes test walks every one of them)."""
    P = W.case(name)
    for mode in ((0, 1, 2) if name == "distinct" else (0,)):
        c = W.census(P, mode, W.solve(P, mode))
        print("WALKREF reached %s mode %d %s" % (name, mode, " ".join("%s %d" % kv for kv in c.items())))
        if name == "distinct":
            assert min(c["ties"], c["near"], c["tiny_one"], c["tiny_both"], c["vote0"], c["vote1"]) >= 1, c
        assert c["vote0"] >= 1 and c["vote1"] >= 1


def test_absent_codes_variants():
    P = W.case("distinct")
    n = 64
    base = W.solve(P, 0, P.seed_codes[:n], P.seed_phases[:n])
    un = W.with_absent(P, 0, "unvisited")
    lo = W.with_absent(P, 0, "losing")
    su, sl = (W.solve(X, 0, P.seed_codes[:n], P.seed_phases[:n]) for X in (un, lo))
    assert (un.aud_idx < 0).sum() + (un.txt_idx < 0).sum() >= 2 and (un.tables(0)[0] < 0).any()
    assert not su["status0"].any() and np.array_equal(su["codes"], base["codes"])
    assert sl["status0"].any() and not sl["status0"].all() and np.array_equal(sl["codes"], base["codes"])
    print("WALKREF absent unvisited_entries %d losing_seeds_flagged %d of %d" %
          ((un.tables(0)[0] < 0).sum() + (un.tables(0)[1] < 0).sum(), sl["status0"].sum(), n))


# ---- negative controls -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fusion_inputs(kind):
    """[(pos, freq, rank rows, the reference's winners)]"""
    if kind == "circulant":
        sets = [t[:3] for t in W.circulant_set()]
    elif kind == "boundary":
        sets = [W.boundary_tables(512, 8, d, 103)[:3] for d in (True, False)]
    else:
        sets = [W.random_tables(512, 22, 104, tie_free=True)[:3]]
    return [t + (W.fuse(*t)[..., 0],) for t in sets]


def _fusion_differs(variant, kind):
    return sum(int((variant(pos, freq, ra)[..., 0] != want).sum()) for pos, freq, ra, want in _fusion_inputs(kind))


FUSION_VARIANTS = {
    "ties_to_highest_code": (W.fuse_ties_high, ("circulant", "boundary")),
    "integer_scaled_scores": (W.fuse_int_scaled, ("circulant",)),
    "scan_stops_at_equal": (functools.partial(W.fuse_scan, stop_at_equal=True), ("boundary",)),
}


@pytest.mark.parametrize("name", sorted(FUSION_VARIANTS))
def test_fusion_variants_are_caught(name):
    variant, by = FUSION_VARIANTS[name]
    for kind in by:
        n = _fusion_differs(variant, kind)
        print("WALKREF control %s on %s: %d table entries differ" % (name, kind, n))
        assert n > 0
    assert _fusion_differs(variant, "random") == 0


def test_the_scan_as_the_kernel_does_it_is_the_plain_argmin():
    """fuse_scan with the kernel's rule (`base > best` stops) on every recipe; the other association of the sum,
    (pos + rank) + freq * 0.05, never differs on these tables, so it is no control."""
    for kind in ("circulant", "boundary", "random"):
        assert _fusion_differs(W.fuse_scan, kind) == 0
        assert _fusion_differs(W.fuse_freq_last, kind) == 0


GATE_VARIANTS = {
    "second_candidate_on_ties": dict(vote_fn=W.vote_le),
    "no_10_eps_rule": dict(gate_fn=W.gate_no_eps_rule),
}


@pytest.mark.parametrize("name", sorted(GATE_VARIANTS))
def test_gate_variants_are_caught(name):
    kw = GATE_VARIANTS[name]
    P = W.case("distinct")
    good, bad = W.solve(P, 0), W.solve(P, 0, **kw)
    n_walks = int((good["codes"] != bad["codes"]).any(axis=(1, 2)).sum())
    n_table = int((good["G"] != bad["G"]).sum())
    print("WALKREF control %s: %d of %d walks differ, %d gate-table entries" % (name, n_walks, len(P.seed_codes), n_table))
    assert n_walks > 0 and n_table > 0
    C = W.case("random")                                         # no planted gate case: the variants agree
    good, bad = W.solve(C, 0), W.solve(C, 0, **kw)
    assert np.array_equal(good["codes"], bad["codes"]) and np.array_equal(good["G"], bad["G"])
