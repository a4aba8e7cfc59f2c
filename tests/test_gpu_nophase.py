"""GPU tests of matching without the phase gate: qpg_match_steps_nophase through the C ABI against the NumPy
statement of its contract (tests/nophase_ref.py) on the walk tests' adversarial tables, then CodeKNN(use_phase=False) and
the command line against the goldens the reference itself produced (tests/golden/make_golden_nophase.py).

EVERY comparison is exact (integers): the next / pick tables of the workspace, codes, sides, candidates, status pairs."""
import functools

import numpy as np
import pytest

from tests import nophase_ref as NR
from tests import walk_ref as W
from tests.helpers import fixture_arrays, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FOUR = (0, 5, 300, 777)
TILE = 3                       # the tables' rows, three times back to back: three chains over the same steps


def _t(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


class _Device:
    """A problem's arrays on the device, the step tables tiled TILE times (uploaded once per problem object)."""

    def __init__(self, P):
        self.P = P
        tile = lambda a: np.tile(np.asarray(a), (TILE, 1))
        self.aud_rank, self.txt_rank = _t(tile(P.aud_rank), np.int16), _t(tile(P.txt_rank), np.int16)
        self.aud_idx, self.txt_idx = _t(tile(P.aud_idx), np.int32), _t(tile(P.txt_idx), np.int32)
        self.pos_rank, self.freq_rank = _t(P.pos_rank, np.int16), _t(P.freq_rank, np.int16)
        self.code = _t(P.code, np.int32)
        self.a_cidx, self.t_cidx = _t(P.aud_cidx, np.int32), _t(P.txt_cidx, np.int32)
        # nothing the kernels index with may leave its array
        assert int(P.aud_cidx.max()) + 4 <= P.code.shape[1] and int(P.txt_cidx.max()) + 4 <= P.code.shape[1]
        assert int(P.aud_idx.max()) < P.code.shape[0] * len(P.aud_cidx)
        assert int(P.txt_idx.max()) < P.code.shape[0] * len(P.txt_cidx)
        assert P.aud_rank.shape == P.txt_rank.shape == P.aud_idx.shape == P.txt_idx.shape == (P.Q, P.K)
        assert P.pos_rank.shape == (P.K, P.K) and P.freq_rank.shape == (P.K,)


@functools.lru_cache(maxsize=None)
def _device(name):
    return _Device(W.case(name))


def _call(D, mode, k, seeds, coins=None, guard=None, tables=False, drop=(), M=None, steps=None, stride=2, made=None, ws=None,
          ws_state=None, outs=None):
    """One qpg_match_steps_nophase call over len(seeds) chains -> the outputs as NumPy arrays (everything is pre-filled
    with -9 / 0xEEEE: a word the call did not write shows).  coins: [n_chains][M steps] or None.  drop: argument names
    passed as NULL.  tables: also the workspace's next / pick.  made: a list that receives the workspace and the output
    tensors before the call (for a call that raises).  ws: the caller's workspace (an i16 tensor of at least the stated
    size) instead of the 0xEEEE one; ws_state: the size to state; outs: the caller's output tensors (codes, side, cand, status) instead of the -9 ones."""
    import torch
    from qpgesture_amd import _lib
    P = D.P
    M = P.M if M is None else M
    steps = P.steps if steps is None else steps
    n, Q = len(seeds), len(seeds) * M * steps
    cpw = min(4 * steps, 30)
    rows = slice(0, max(Q, 1))
    ws_bytes = int(_lib.load().qpg_match_steps_nophase_ws_bytes(n, max(M, 1), steps, P.K))
    if ws is None:
        ws = torch.full((ws_bytes // 2,), -4370, dtype=torch.int16, device=DEV)               # 0xEEEE
    ws_bytes = ws_bytes if ws_state is None else ws_state
    o = outs if outs is not None else {
        k_: torch.full(shape, -9, dtype=torch.int32, device=DEV)
        for k_, shape in dict(codes=(n, max(M, 1), cpw), side=(n, max(M, 1) * steps), cand=(n, max(M, 1) * steps),
                              status=(n, stride)).items()}
    if made is not None:
        made.extend([ws] + list(o.values()))
    a = dict(aud_rank=D.aud_rank[rows], aud_idx=D.aud_idx[rows], txt_rank=D.txt_rank[rows], txt_idx=D.txt_idx[rows],
             aud_cidx=D.a_cidx, txt_cidx=D.t_cidx, coins=None if coins is None else _t(np.asarray(coins) != 0, np.uint8),
             ws=ws)
    for name in drop:
        a[name] = None
    _lib.call("qpg_match_steps_nophase", DEV, a["aud_rank"], a["aud_idx"], a["txt_rank"], a["txt_idx"], D.pos_rank,
              D.freq_rank, D.code, P.code.shape[1], a["aud_cidx"], len(P.aud_cidx), a["txt_cidx"], len(P.txt_cidx), mode, k, M,
              steps, P.K, n, _t(seeds, np.int32), a["coins"], o["codes"], o["side"], o["cand"], o["status"], stride,
              None if guard is None else _t([guard], np.int32), a["ws"], 0 if a["ws"] is None else ws_bytes)
    torch.cuda.synchronize()
    out = {k_: v.cpu().numpy() for k_, v in o.items()}
    if tables:
        raw = ws.cpu().numpy()
        nb = Q * 2 * P.K
        out["next"] = raw[:nb].view(np.uint16).astype(np.int64).reshape(Q, 2, P.K)
        out["pick"] = raw[nb:nb + 2 * nb].view(np.int32).astype(np.int64).reshape(Q, 2, P.K)
    return out


def _check_walks(got, P, mode, k, seeds, coins, guard, tabs, M=None):
    for c, seed in enumerate(seeds):
        ref = NR.walk(P, mode, k, seed, None if coins is None else coins[c], M=M, tabs=tabs)
        assert np.array_equal(got["codes"][c], ref["codes"]), (c, seed)
        assert np.array_equal(got["side"][c], ref["side"]) and np.array_equal(got["cand"][c], ref["cand"])
        assert got["status"][c, :2].tolist() == [ref["status0"], 0 if guard is None else guard]


def _coin_kinds(Q, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [np.ones((n, Q), bool), np.zeros((n, Q), bool), rng.random((n, Q)) > 0.5]


@pytest.mark.parametrize("name", ["main", "boundary", "k528", "k500", "k64_s7", "k1024"])
def test_tables_and_walks_vs_the_numpy_statement(name):
    """All three modes, desired_k 0 / 1 / 3 / 15: the workspace's next / pick tables for every (step, side, previous code);
    then four seeds one chain at a time and three chains in one call, coins all audio / all text / random, guard_flags
    NULL and 5."""
    D = _device(name)
    P = D.P
    seeds = [int(P.seed_codes[s]) for s in FOUR]
    n_walks = 0
    for mode in (0, 1, 2):
        for k in (0, 1, 3, 15):
            tabs = NR.tables(P, mode, k)
            kinds = _coin_kinds(P.Q, 3, 7 * k + mode) if mode == 0 else [None]
            first = _call(D, mode, k, seeds[:3], kinds[-1], tables=True)
            assert np.array_equal(first["next"], np.tile(tabs[0], (3, 1, 1)))
            assert np.array_equal(first["pick"], np.tile(tabs[1], (3, 1, 1)))
            for ci, coins in enumerate(kinds):
                for guard in (None, 5):
                    got = _call(D, mode, k, seeds[1:], coins, guard, stride=2 if guard is None else 5)
                    _check_walks(got, P, mode, k, seeds[1:], coins, guard, tabs)
                    for i, s in enumerate(seeds):
                        one = None if coins is None else coins[i % 3][None]
                        _check_walks(_call(D, mode, k, [s], one, guard), P, mode, k, [s], one, guard, tabs)
                        n_walks += 1
    assert n_walks == (3 + 1 + 1) * 4 * 2 * 4


def _with_tables(P, pos, freq, ra, rb, M, steps):
    """P's database under other fusion tables and another window geometry (Q = M steps rows)."""
    Q = M * steps
    keep = {k: v for k, v in P.__dict__.items() if not k.startswith("_")}
    keep.update(pos_rank=pos, freq_rank=freq, aud_rank=ra[:Q], txt_rank=rb[:Q], aud_idx=P.aud_idx[:Q], txt_idx=P.txt_idx[:Q],
                M=M, steps=steps)
    return W.Problem(**keep)


def _check_tables_only(Pn, modes, ks):
    D = _Device(Pn)
    for mode in modes:
        for k in ks:
            got = _call(D, mode, k, [0], np.ones((1, Pn.Q), bool) if mode == 0 else None, tables=True)
            ref = NR.tables(Pn, mode, k)
            assert np.array_equal(got["next"], ref[0]) and np.array_equal(got["pick"], ref[1]), (mode, k)


def _n_tied(Pn, mode, k):
    """(step, previous code) tasks whose score at position k equals a neighbour's."""
    n = 0
    for q in range(Pn.Q):
        o = np.sort(NR.scores(Pn, mode, q), axis=1)
        n += int(((o[:, k] == o[:, k + 1]) | ((o[:, k] == o[:, k - 1]) if k else False)).sum())
    return n


@pytest.mark.parametrize("i", range(len(W.SHIFTS)))
def test_ties_on_the_circulant_tables(i):
    """Position k on the 16 circulant table sets of the walk tests (22 steps each: 11 windows of 2), whose two-way minima
    tie.  The three-way sum on every set, the two-way sums on the first."""
    pos, freq, ra, rb = W.circulant_set()[i]
    Pn = _with_tables(W.case("main"), pos, freq, ra, rb, 11, 2)
    assert Pn.Q == 22
    _check_tables_only(Pn, (0, 1, 2) if i == 0 else (0,), (0, 1, 15))


def test_ties_when_the_two_rank_rows_sum_to_a_constant():
    """txt_rank[c] = K - 1 - aud_rank[c]: the three-way score is the pose / frequency part plus a constant - no bound by a
    rank row could stop a scan early, and a tie of the pose / frequency part would be a tie of every step."""
    pos, freq, ra, _ = W.circulant_set()[1]
    rb = (ra.shape[1] - 1 - ra.astype(np.int64)).astype(np.int16)
    Pn = _with_tables(W.case("main"), pos, freq, ra, rb, 11, 2)
    assert (Pn.aud_rank.astype(np.int64) + Pn.txt_rank == Pn.K - 1).all()
    _check_tables_only(Pn, (0,), (0, 1, 15))


def test_ties_everywhere():
    """Scores that are small integers: every task has dozens of codes at the score of position k (counted), so the code
    there is decided by the code index alone.  (Rank rows that are no permutations: scored as the values they are.)"""
    K = 512
    c = np.arange(K)
    pos = ((c[:, None] + c[None, :]) % 4).astype(np.int16)
    freq = (20 * (c % 3)).astype(np.int16)                      # 20 * 0.05 == 1.0 and 40 * 0.05 == 2.0 exactly in f64
    assert 20 * 0.05 == 1.0 and 40 * 0.05 == 2.0
    q = np.arange(22)[:, None]
    ra, rb = ((7 * c[None, :] + q) % 5).astype(np.int16), ((3 * c[None, :] + 2 * q) % 3).astype(np.int16)
    Pn = _with_tables(W.case("main"), pos, freq, ra, rb, 11, 2)
    for k in (0, 1, 15):
        assert _n_tied(Pn, 0, k) == 22 * K and _n_tied(Pn, 1, k) == 22 * K
    _check_tables_only(Pn, (0, 1, 2), (0, 1, 15))


def test_rank_rows_that_are_not_permutations():
    """A rank held twice, a rank outside [0, K), a negative one: every code is scored as the values are."""
    pos, freq, ra = W.nonperm_tables(512, 77)
    assert not np.array_equal(np.sort(ra[0]), np.arange(512)) and ra[1].max() >= 512 and ra[1].min() < 0
    Pn = _with_tables(W.case("main"), pos, freq, ra, ra[::-1].copy(), 3, 1)
    _check_tables_only(Pn, (0, 1, 2), (0, 3, 15))


def test_absent_codes():
    """A code without a candidate AT position k on the chain's way: status[0] == 1, the chain stops there and the steps
    behind it hold -1.  The same code taken away at the positions beside k: status 0, nothing changes.  And the walk tests'
    tables with absent codes, whatever they do to these chains."""
    P = W.case("main")
    k, seed = 1, int(P.seed_codes[5])
    coins = _coin_kinds(P.Q, 1, 3)[2]
    base = NR.walk(P, 0, k, seed, coins[0])
    assert base["status0"] == 0
    nxt, _ = NR.tables(P, 0, k)
    prev, q_hit = seed, 10
    for q in range(q_hit):
        prev = int(nxt[q, base["side"][q], prev])
    order = NR.orders(P, 0)[q_hit, prev]

    def without(positions):
        keep = {k_: v for k_, v in P.__dict__.items() if not k_.startswith("_")}
        keep.update(aud_idx=P.aud_idx.copy(), txt_idx=P.txt_idx.copy())
        for pos_ in positions:
            keep["aud_idx"][q_hit, order[pos_]] = keep["txt_idx"][q_hit, order[pos_]] = -1
        return W.Problem(**keep)

    hit = without([k])
    got = _call(_Device(hit), 0, k, [seed], coins, guard=5)
    ref = NR.walk(hit, 0, k, seed, coins[0])
    assert ref["status0"] == 1 and got["status"][0].tolist() == [1, 5]
    assert np.array_equal(got["side"][0], ref["side"]) and (got["side"][0, q_hit + 1:] == -1).all()
    assert np.array_equal(got["cand"][0], ref["cand"]) and (got["cand"][0, q_hit:] == -1).all()
    assert np.array_equal(got["codes"][0], ref["codes"]) and np.array_equal(got["codes"][0, 0], base["codes"][0])
    miss = without([k - 1, k + 1, 15])
    got = _call(_Device(miss), 0, k, [seed], coins)
    assert got["status"][0].tolist() == [0, 0] and np.array_equal(got["codes"][0], base["codes"])
    assert np.array_equal(got["cand"][0], base["cand"])
    # a seed outside [0, K): no state at all
    got = _call(_device("main"), 0, k, [P.K], coins)
    assert got["status"][0].tolist() == [1, 0] and (got["codes"] == -1).all() and (got["side"] == -1).all()
    for kind in ("unvisited", "losing"):
        Pa = W.with_absent(P, 0, kind)
        assert (Pa.aud_idx < 0).sum() + (Pa.txt_idx < 0).sum() >= 1
        Da = _Device(Pa)
        for k2 in (0, 3):
            tabs = NR.tables(Pa, 0, k2)
            seeds = [int(P.seed_codes[s]) for s in FOUR[:3]]
            c3 = _coin_kinds(P.Q, 3, 11)[2]
            got = _call(Da, 0, k2, seeds, c3, tables=True)
            assert np.array_equal(got["next"], np.tile(tabs[0], (3, 1, 1)))
            _check_walks(got, Pa, 0, k2, seeds, c3, None, tabs)


def test_error_returns():
    """A geometry the tabulation refuses: QPG_EUNSUP and nothing written.  Bad arguments: QPG_EINVAL, nothing written.
    M == 0: the status pairs alone."""
    from qpgesture_amd import _lib
    D = _device("main")
    P = D.P
    coins = np.ones((1, 9 * 2), bool)

    def untouched(**kw):
        import torch
        made = []
        with pytest.raises(RuntimeError) as e:
            _call(D, made=made, **kw)
        torch.cuda.synchronize()
        assert (made[0] == -4370).all() and all((t == -9).all() for t in made[1:])
        return e

    e = untouched(mode=0, k=0, seeds=[1], coins=coins, M=2, steps=9)
    assert e.type is _lib.Unsupported and "geometry" in str(e.value)
    ok = np.ones((1, P.Q), bool)
    for kw in (dict(k=16), dict(k=-1), dict(drop=("aud_rank",)), dict(drop=("txt_idx",)), dict(drop=("coins",)),
               dict(drop=("ws",)), dict(mode=3), dict(mode=0x100)):
        args = dict(mode=0, k=0)
        args.update(kw)
        e = untouched(seeds=[1], coins=ok, **args)
        assert e.type is RuntimeError and "(-1)" in str(e.value), kw
    # a one-sided mode needs neither the other side nor the coins
    got = _call(D, 1, 0, [1], None, drop=("txt_rank", "txt_idx", "txt_cidx"))
    _check_walks(got, P, 1, 0, [1], None, None, NR.tables(P, 1, 0))
    got = _call(D, 2, 0, [1], None, drop=("aud_rank", "aud_idx", "aud_cidx"))
    _check_walks(got, P, 2, 0, [1], None, None, NR.tables(P, 2, 0))
    got = _call(D, 1, 0, [1, 2], None, guard=7, M=0, drop=("ws",))
    assert got["status"].tolist() == [[0, 7], [0, 7]] and (got["codes"] == -9).all()


# ---- the matcher and the command line against the reference's goldens ------------------------------------------------------------
WAVLM = ["nophase_audtxt_n48_m2_s0", "nophase_aud_n48_m2_s0", "nophase_audtxt_k3_n48_m2_s0"]
WAVVQ = ["nophase_wavvq_aud_n40_m2_s20", "nophase_wavvq_audtxt_n40_m2_s20"]


@functools.lru_cache(maxsize=None)
def _inputs(meta, wavvq, freq_from, variant=None):
    import torch
    from qpgesture_amd.code_knn import GestureDB
    ntr, nte, s0, s1, s2, s3 = meta
    A = fixture_arrays(ntr, nte, s0, s1, s2, s3, wavlm_dim=8 if wavvq else 1024, variant=variant)
    db = GestureDB(A["code"], A["tr_interp"], A["tr_ctx"], A["tr_phase"], A["sig"], device=DEV,
                   freq_rank=load_golden(freq_from)["step_freq_score"], wavvq=A["tr_wavvq"] if wavvq else None)
    te_i = torch.from_numpy(A["te_wavvq"] if wavvq else A["te_interp"]).to(DEV)
    te_c = torch.from_numpy(np.ascontiguousarray(A["te_ctx"])).to(DEV)
    return db, te_i, te_c, nte


def _golden_matcher(name, **kw):
    from qpgesture_amd.code_knn import MODE_AUD, MODE_AUD_TXT, CodeKNN
    g = load_golden(name)
    wavvq = name in WAVVQ
    db, te_i, te_c, M = _inputs(tuple(int(v) for v in g["meta"][:6]), wavvq, (WAVVQ if wavvq else WAVLM)[0])
    knn = CodeKNN(db, use_wavlm=not wavvq, use_wavvq=wavvq, use_phase=False, desired_k=int(g["desired_k"]),
                  rng=np.random.RandomState(int(g["np_seed"])), **kw)
    return g, knn, te_i, te_c, M, (MODE_AUD_TXT if "txt_pay" in g.files else MODE_AUD)


def _golden_picks(g, knn):
    """The candidates j * G + g of the reference's blocks, from its captured [j, k]."""
    db = knn.db
    two = "txt_pay" in g.files
    a_ks, a_G = (db.vq_k, db.Gv) if knn.use_wavvq else (db.aud_k, db.Ga)
    out = []
    for q, c in enumerate(g["step_chosen"]):
        text = two and not g["coins"][q] > 0.5
        j, kk = (g["txt_aux"] if text else g["aud_aux"])[q, c]
        out.append(j * db.Gt + db.txt_k.index(kk) if text else j * a_G + a_ks.index(kk))
    return np.array(out).reshape(-1, 8)


def _check_golden(g, knn, out):
    codes, phases, sides = out
    assert codes.dtype == np.int64 and np.array_equal(codes, g["knn_pred"])
    assert phases.shape == (2, 0, 8, 16) and phases.dtype == np.float32
    want_sides = np.where(g["coins"] > 0.5, 0, 1) if "txt_pay" in g.files else np.zeros(16, np.int64)
    assert sides.dtype == np.int32 and np.array_equal(sides, want_sides.reshape(2, 8))
    assert np.array_equal(knn.last_picks, _golden_picks(g, knn))
    assert knn._last_rank_cut is False and knn.fallbacks == 0


@pytest.mark.parametrize("name", WAVLM)
def test_match_clip_vs_the_reference(name):
    """CodeKNN(use_phase=False).match_clip from the reference's seed of np.random: its knn_pred, its sides (from its coins),
    the candidates its blocks came from; the generator ends where the reference's loop leaves it."""
    g, knn, te_i, te_c, M, mode = _golden_matcher(name)
    _check_golden(g, knn, knn.match_clip(te_i, te_c, M, mode=mode))
    rs = np.random.RandomState(int(g["np_seed"]))
    rs.randint(0, knn.n_db_seq), rs.randint(0, knn.n_db_frm - 8)
    if mode == 0:
        assert np.array_equal(rs.rand(16), g["coins"])
    assert knn.rng.randint(0, 1 << 30) == rs.randint(0, 1 << 30)
    # explicit state: the same clip again
    out = knn.match_clip(te_i, te_c, M, mode=mode, seed_code=int(g["init_code"]),
                         coins=(g["coins"] > 0.5) if mode == 0 else None)
    _check_golden(g, knn, out)


@pytest.mark.parametrize("name", WAVVQ)
def test_wavvq_fixtures_vs_the_reference(name):
    """The reference's one well-formed no-phase route.  NOT a match_clip golden: Levenshtein distances are small integers
    and tie massively, and the reference ranks them with NumPy's UNSTABLE argsort (GestureKNN.py:574), so its rank rows are
    not a function of the distances alone and match_clip under the library's stable ranks need not return its knn_pred.
    What is asserted, unconditionally: the distances and winners are the reference's, exactly; WALKED FROM THE REFERENCE'S
    OWN CAPTURED RANK ROWS (CodeKNN.walk on the matcher's tables with those rows put in) the device gives its knn_pred,
    sides and candidates; match_clip under the stable ranks equals the NumPy statement on the matcher's tables.
    Only where this host's NumPy happens to order the ties as the reference's did (it prints whether), match_clip with
    host_ranks - the command line's --tie_rule numpy - is compared with knn_pred as well."""
    import torch
    g, knn, te_i, te_c, M, mode = _golden_matcher(name)
    db = knn.db
    seed, coins = int(g["init_code"]), ((g["coins"] > 0.5) if mode == 0 else None)
    T = knn.sweep_tables(te_i, te_c, M, mode)
    assert np.array_equal(T["aud_d"].cpu().numpy().astype(np.float64), g["aud_dist"])            # exact integers
    at = {k: i for i, k in enumerate(db.vq_k)}
    gj, gk = g["aud_aux"][..., 0], g["aud_aux"][..., 1]
    assert np.array_equal(T["aud_idx"].cpu().numpy(), np.where(gj >= 0, gj * db.Gv + np.vectorize(lambda k: at.get(k, 0))(gk), -1))
    stable = knn.match_clip(te_i, te_c, M, mode=mode, seed_code=seed, coins=coins)
    ref = NR.walk(_problem_of(knn, T, M, aud_cidx=db.vq_cidx_host), mode, 0, seed, coins)
    assert ref["status0"] == 0 and np.array_equal(stable[0], ref["codes"]) and np.array_equal(stable[2].reshape(-1), ref["side"])
    Tr = dict(T)
    Tr["aud_rank"] = _t(g["step_aud_score"], np.int16)
    if mode == 0:
        assert np.array_equal(T["txt_d"].cpu().numpy(), g["txt_dist"])
        Tr["txt_rank"] = _t(g["step_txt_score"], np.int16)
    _check_golden(g, knn, knn.walk(Tr, M, 0, mode, seed_code=seed, coins=coins))
    # (the dtype the reference's list becomes is part of NumPy's tie order: int64 / float32 for a row in which every code
    #  has a candidate, float64 with a 1e+3 placeholder in it - CodeKNN.numpy_ranks)
    full = (gj >= 0).all(axis=1)
    here = [np.array_equal(np.stack([(np.array([int(x) for x in r]) if full[q] else np.array(list(r))).argsort().argsort()
                                     for q, r in enumerate(g["aud_dist"])]), g["step_aud_score"])]
    if mode == 0:
        tfull = (g["txt_aux"][..., 0] >= 0).all(axis=1)
        here.append(np.array_equal(np.stack([np.array(list(r if tfull[q] else r.astype(np.float64))).argsort().argsort()
                                             for q, r in enumerate(g["txt_dist"])]), g["step_txt_score"]))
    print("host NumPy reproduces the reference's tie order: %s" % all(here))
    if all(here):
        knn.host_ranks = True
        _check_golden(g, knn, knn.match_clip(te_i, te_c, M, mode=mode, seed_code=seed, coins=coins))


@pytest.mark.parametrize("name", WAVLM)
@pytest.mark.parametrize("how", ["f64", "exact", "serial_walk"])
def test_match_clip_on_the_other_audio_paths(name, how):
    g, knn, te_i, te_c, M, mode = _golden_matcher(name)
    if how == "serial_walk":
        knn.serial_walk = True                      # (a knob of the gated walk: nothing here reads it)
    else:
        knn.audio_precision = how
    _check_golden(g, knn, knn.match_clip(te_i, te_c, M, mode=mode))
    assert knn._last_audio_exact == (how == "exact") and (how == "serial_walk" or not knn._last_audio_mixed)


def test_a_gated_matcher_on_the_same_inputs_is_untouched():
    from qpgesture_amd.code_knn import CodeKNN
    g = load_golden("shipped_n48_m2_s0")
    db, te_i, te_c, M = _inputs(tuple(int(v) for v in g["meta"][:6]), False, WAVLM[0])
    assert np.array_equal(load_golden(WAVLM[0])["step_freq_score"], g["step_freq_score"])
    knn = CodeKNN(db, rng=np.random.RandomState(123456), desired_k=3)
    codes, phases, votes = knn.match_clip(te_i, te_c, M)
    assert np.array_equal(codes, g["knn_pred"]) and np.array_equal(votes, g["vote"]) and phases.shape == (2, 8, 8, 16)
    assert knn._last_rank_cut is True and knn.last_picks is None


def _problem_of(knn, T, M, aud_cidx=None):
    """The tables of sweep_tables as a tests/walk_ref problem."""
    db = knn.db
    cpu = lambda k: None if T[k] is None else T[k].cpu().numpy()
    return W.Problem(aud_rank=cpu("aud_rank"), txt_rank=cpu("txt_rank"), aud_idx=cpu("aud_idx"), txt_idx=cpu("txt_idx"),
                     pos_rank=db.pos_rank.cpu().numpy(), freq_rank=db.freq_rank.cpu().numpy(), code=db.code_host,
                     aud_cidx=np.asarray(db.aud_cidx_host if aud_cidx is None else aud_cidx), txt_cidx=np.asarray(db.txt_rows_host), M=M, steps=8, K=db.K)


def test_the_walk_relevance_cut_never_feeds_this_walk():
    """On the mid-size database the cut (QPG_RANK_CUT at its default) leaves codes unsettled that the two-way winner cannot
    be - and the three-way winner or position 3 can.  The no-phase clip equals the statement walked over the SETTLED tables
    (sweep_tables(for_walk=False)), and the select it ran had no cut."""
    from qpgesture_amd.code_knn import MODE_AUD_TXT, CodeKNN
    g = load_golden("shipped_n256_m2_s70")
    db, te_i, te_c, M = _inputs(tuple(int(v) for v in g["meta"][:6]), False, "shipped_n256_m2_s70")
    gated = CodeKNN(db, rng=np.random.RandomState(1))
    assert gated.rank_cut
    T = gated.sweep_tables(te_i, te_c, M, MODE_AUD_TXT, for_walk=False)
    assert gated._last_rank_cut is False
    P = _problem_of(gated, T, M)
    gated.sweep_tables(te_i, te_c, M, MODE_AUD_TXT, for_walk=True)
    assert gated._last_rank_cut is True                       # (what a gated clip takes on this database)
    coins = np.random.RandomState(3).rand(16) > 0.5
    for k in (0, 3):
        knn = CodeKNN(db, use_phase=False, desired_k=k, rng=np.random.RandomState(1))
        codes, _, sides = knn.match_clip(te_i, te_c, M, seed_code=17, coins=coins)
        ref = NR.walk(P, 0, k, 17, coins)
        assert ref["status0"] == 0 and np.array_equal(codes, ref["codes"])
        assert np.array_equal(sides.reshape(-1), ref["side"]) and np.array_equal(knn.last_picks.reshape(-1), ref["cand"])
        assert knn._last_rank_cut is False


def test_guard_overflow_rematches_from_the_same_seed_and_coins():
    """The near-silent clip overflows the capped lists: the no-phase clip is matched again on the exact path, counted, from
    the seed and the coins drawn ONCE, and equals the statement on the exact tables."""
    from qpgesture_amd.code_knn import CodeKNN
    g = load_golden("shipped_nearsilent_n48_m2_s50")
    db, te_i, te_c, M = _inputs(tuple(int(v) for v in g["meta"][:6]), False, "shipped_nearsilent_n48_m2_s50",
                                str(g["variant"]))
    knn = CodeKNN(db, use_phase=False, desired_k=1, rng=np.random.RandomState(123456))
    codes, _, sides = knn.match_clip(te_i, te_c, M, return_tables=True)
    assert knn.fallbacks == 1 and knn.audio_precision == "mixed" and knn.mixed_stats()["flags"] == 0
    assert knn._last_audio_exact
    rs = np.random.RandomState(123456)
    i, j = rs.randint(0, db.N), rs.randint(0, 180 - 8)
    seed, coins = int(db.code_host[i, j // 30]), rs.rand(16) > 0.5
    assert knn.rng.randint(0, 1 << 30) == rs.randint(0, 1 << 30)            # drawn once, not once per attempt
    ref = NR.walk(_problem_of(knn, knn.tables, M), 0, 1, seed, coins)
    assert ref["status0"] == 0 and np.array_equal(codes, ref["codes"])
    assert np.array_equal(sides.reshape(-1), ref["side"]) and np.array_equal(sides.reshape(-1), np.where(coins, 0, 1))


def _same_members(a, b):
    import zipfile
    za, zb = zipfile.ZipFile(a), zipfile.ZipFile(b)
    ia, ib = za.infolist(), zb.infolist()
    assert [i.filename for i in ia] == [i.filename for i in ib]
    for x, y in zip(ia, ib):
        assert (x.CRC, x.file_size, x.compress_size) == (y.CRC, y.file_size, y.compress_size)
        assert za.read(x.filename) == zb.read(y.filename)


def _cli(tmp_path):
    from qpgesture_amd import GestureKNN as cli
    from qpgesture_amd import synth
    paths = synth.write_npz_set(str(tmp_path / "npz"), 48, 2)
    argv = []
    for k, v in paths.items():
        argv += ["--" + k, v]

    def run(name, *extra):
        out = str(tmp_path / (name + ".npz"))
        cli.main(argv + ["--out_knn_filename", out, "--db_cache", "off"] + list(extra))
        return out
    return run


@pytest.mark.parametrize("extra, golden", [(["--no_phase"], WAVLM[0]), (["--no_phase", "-k", "3"], WAVLM[2])])
def test_the_command_line_writes_the_reference_s_file(tmp_path, extra, golden):
    """--no_phase [--desired_k 3]: the reference's knn_pred (shape, dtype) plus knn_sides / knn_cand."""
    g, z = load_golden(golden), np.load(_cli(tmp_path)("nophase", *extra))
    assert sorted(z.files) == ["knn_cand", "knn_pred", "knn_sides"]
    assert z["knn_pred"].dtype == g["knn_pred"].dtype == np.int64 and z["knn_pred"].shape == g["knn_pred"].shape
    assert np.array_equal(z["knn_pred"], g["knn_pred"])
    assert z["knn_sides"].dtype == np.int32 and np.array_equal(z["knn_sides"].reshape(-1), np.where(g["coins"] > 0.5, 0, 1))
    assert z["knn_cand"].dtype == np.int32 and z["knn_cand"].shape == (2, 8) and (z["knn_cand"] >= 0).all()


def test_desired_k_without_no_phase_changes_nothing(tmp_path):
    """--desired_k 3 alone: the file written without the flag, member for member (the reference's phase branches never read
    it either)."""
    run = _cli(tmp_path)
    plain, ignored = run("plain"), run("k3_ignored", "--desired_k", "3")
    _same_members(plain, ignored)
    assert np.load(plain).files == ["knn_pred"]
    assert np.array_equal(np.load(plain)["knn_pred"], load_golden("shipped_n48_m2_s0")["knn_pred"])


def test_refusals_on_a_real_matcher():
    from qpgesture_amd.code_knn import ClipPipeline, CodeKNN, GraphPipeline
    g = load_golden(WAVLM[0])
    db, te_i, te_c, M = _inputs(tuple(int(v) for v in g["meta"][:6]), False, WAVLM[0])
    knn = CodeKNN(db, use_phase=False, rng=np.random.RandomState(1))
    T = knn.sweep_tables(te_i, te_c, M)
    for call in (lambda: knn.match_clip_takes(te_i, te_c, M, n_takes=2),
                 lambda: knn.walk_takes(T, M, [1, 2], np.zeros((2, 8, 16), np.float32)),
                 lambda: knn.capture_clip_graph(M),
                 lambda: ClipPipeline(db, use_phase=False),
                 lambda: GraphPipeline(db, M, use_phase=False)):
        with pytest.raises(NotImplementedError, match="phase gate"):
            call()
    knn.force_sharded = True
    with pytest.raises(NotImplementedError, match="row-sharded"):
        knn.match_clip(te_i, te_c, M)
