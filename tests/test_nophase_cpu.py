"""CPU tests of matching without the phase gate: the NumPy statement of its contract (tests/nophase_ref.py)
against the goldens the reference itself produced (tests/golden/make_golden_nophase.py), the matcher's draws, the plan, the
command-line flags, the header."""
import types

import numpy as np
import pytest

from qpgesture_amd import GestureKNN, _lib, inference
from qpgesture_amd import code_knn as ck
from tests import nophase_ref as NR
from tests import walk_ref as W
from tests.helpers import load_golden

GOLDENS = ["nophase_audtxt_n48_m2_s0", "nophase_aud_n48_m2_s0", "nophase_audtxt_k3_n48_m2_s0",
           "nophase_wavvq_aud_n40_m2_s20", "nophase_wavvq_audtxt_n40_m2_s20"]


@pytest.mark.parametrize("name", GOLDENS)
def test_the_numpy_statement_reproduces_the_reference(name):
    """From a golden's captured scores, coins and payloads: the code at position desired_k under the (score, code) order
    is the reference's choice at every step, the blocks of the chosen sides are its knn_pred, and the previous code every
    step scored against (the one code with pose rank 511: `1e10000`, GestureKNN.py:533-534) is the seed, then the 4th code
    of the previous block, and at a window's first step the 30th KEPT code of the window before - offset 1 of its last
    block, not 3."""
    g = load_golden(name)
    pred, chosen, sides = NR.replay_golden(g)
    assert g["knn_pred"].dtype == np.int64 and g["knn_pred"].shape == (2, 30)
    assert np.array_equal(pred, g["knn_pred"]) and np.array_equal(chosen, g["step_chosen"])
    two = "txt_pay" in g.files
    assert len(g["coins"]) == (16 if two else 0)
    freq = g["step_freq_score"].astype(np.float64) * 0.05
    k = int(g["desired_k"])
    for q in range(16):
        if q == 0:
            prev = int(g["init_code"])
        elif q % 8 == 0:
            prev = int(g["knn_pred"][q // 8 - 1, 29])
            last_block = (g["txt_pay"] if sides[q - 1] else g["aud_pay"])[q - 1, chosen[q - 1]]
            assert prev == last_block[(30 - 1) % 4]
        else:
            prev = int((g["txt_pay"] if sides[q - 1] else g["aud_pay"])[q - 1, chosen[q - 1], 3])
        pose = g["step_pos_score"][q] - freq
        assert int(np.argmax(pose)) == prev and round(float(pose[prev])) == 511
        # the fixture is one where the reference's unstable order IS the stable one at position k
        o = np.sort(g["step_combined_score"][q])
        assert o[k] != o[k + 1] and (k == 0 or o[k - 1] != o[k])


def test_the_statement_on_a_walk_problem():
    """nophase_ref on a tests/walk_ref problem: position k by the literal sort, every k; one side's tables in the one-sided
    modes; a window's last step reads offset (30 - 1) % 4; a chain stops at a code without a candidate."""
    P = W.case("k64_s7")
    assert P.codes_per_window == 28 and P.steps == 7
    for mode in (0, 1, 2):
        for k in (0, 1, 15):
            nxt, pick = NR.tables(P, mode, k)
            for q, p in ((0, 0), (6, 63), (20, 17)):
                s = NR.scores(P, mode, q)[p]
                c = sorted(range(P.K), key=lambda i: (s[i], i))[k]
                for side in NR.sides_of(mode):
                    idx, cidx, G = ((P.txt_idx, P.txt_cidx, len(P.txt_cidx)) if side else
                                    (P.aud_idx, P.aud_cidx, len(P.aud_cidx)))
                    assert pick[q, side, p] == idx[q, c]
                    j, g = divmod(int(idx[q, c]), G)
                    off = 3 if q % 7 != 6 else (28 - 1) % 4
                    assert nxt[q, side, p] == P.code[j, cidx[g] + off]
                for side in set((0, 1)) - set(NR.sides_of(mode)):
                    assert (nxt[:, side] == NR.NONE16).all() and (pick[:, side] == -1).all()
    coins = np.arange(P.Q) % 3 == 0
    a = NR.walk(P, 0, 1, 5, coins)
    assert a["status0"] == 0 and a["codes"].shape == (3, 28) and np.array_equal(a["side"], np.where(coins, 0, 1))
    assert (a["codes"] >= 0).all() and (a["cand"] >= 0).all()
    # the same chain, with the candidate of its 10th step taken away
    nxt, pick = NR.tables(P, 0, 1)
    nxt, pick = nxt.copy(), pick.copy()
    trail = [5]
    for q in range(9):
        trail.append(int(nxt[q, a["side"][q], trail[-1]]))
    nxt[9, a["side"][9], trail[9]], pick[9, a["side"][9], trail[9]] = NR.NONE16, -1
    b = NR.walk(P, 0, 1, 5, coins, tabs=(nxt, pick))
    assert b["status0"] == 1 and np.array_equal(b["side"][:10], a["side"][:10]) and (b["side"][10:] == -1).all()
    assert np.array_equal(b["codes"].reshape(-1)[:36], a["codes"].reshape(-1)[:36]) and (b["cand"][9:] == -1).all()


class _StubMatcher(ck.CodeKNN):
    """A no-phase CodeKNN whose device work is replaced by records of what it was asked for."""

    def __init__(self, seed, overflow=0, **kw):
        import torch
        rs = np.random.RandomState(99)
        fake = types.SimpleNamespace(step_sz=6, T=180, N=7, device=torch.device("cpu"), n_local=7, world=1, K=512, Ga=26,
                                     F=8, Dt=384, feature_dtype="f32", hl_bound_ok=True, hl_image=None, txt_sorted=None,
                                     hl_planes=2, code_host=rs.randint(0, 512, (7, 30)).astype(np.int64),
                                     phase_host=rs.standard_normal((7, 240, 2, 8)).astype(np.float32))
        super().__init__(fake, rng=np.random.RandomState(seed), use_phase=False, **kw)
        self.seen, self.sweeps, self.overflow = [], [], overflow

    def sweep_tables(self, *a, **k):
        self.sweeps.append((k.get("for_walk"), self.audio_precision))
        return {}

    def walk(self, T, M, off=0, mode=0, seed_code=None, seed_phase=None, coins=None, **k):
        self.seen.append((int(seed_code), None if coins is None else np.asarray(coins).copy()))
        if self.overflow:
            self.overflow -= 1
            raise ck.GuardOverflow(ck.FLAG_LIST_OVERFLOW)
        return np.zeros((M, 30), np.int64), np.zeros((M, 0, 8, 16), np.float32), np.zeros((M, 8), np.int32)


def test_a_matcher_draws_the_seed_then_the_coins_like_the_reference():
    """Seed (two randint, GestureKNN.py:463-464), then M * steps successive rand() (:581); the generator ends where the
    reference's does; one-sided modes draw no coin; explicit seed / coins draw nothing; a re-match replays both."""
    import torch
    M = 3
    x, c = torch.zeros((M, 180, 8)), torch.zeros((M, 30, 384))
    knn = _StubMatcher(5)
    assert knn.n_steps() == 8
    out = knn.match_clip(x, c, M)
    assert out[0].shape == (M, 30) and out[1].shape == (M, 0, 8, 16) and out[2].shape == (M, 8)
    rs = np.random.RandomState(5)
    i, j = rs.randint(0, 7), rs.randint(0, 180 - 8)
    want_seed = int(knn.db.code_host[i, j // 30])
    want_coins = np.array([rs.rand() > 0.5 for _ in range(M * 8)])
    (seed, coins), = knn.seen
    assert seed == want_seed and np.array_equal(coins, want_coins) and 0 < want_coins.sum() < M * 8
    sa, sb = knn.rng.get_state(), rs.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    assert knn.sweeps == [(False, "mixed")]                                    # never the walk-relevance cut's tables
    # the code alone, after the same two draws
    k2, r2 = _StubMatcher(5), np.random.RandomState(5)
    r2.randint(0, 7), r2.randint(0, 172)
    assert k2.init_code_phase() == want_seed and k2.rng.randint(0, 1 << 30) == r2.randint(0, 1 << 30)
    # audio only: no coin is drawn
    k3, r3 = _StubMatcher(6), np.random.RandomState(6)
    k3.match_clip(x, c, M, mode=ck.MODE_AUD)
    r3.randint(0, 7), r3.randint(0, 172)
    assert k3.seen[0][1] is None and k3.rng.randint(0, 1 << 30) == r3.randint(0, 1 << 30)
    # explicit state draws nothing
    before = knn.rng.get_state()[1].copy()
    knn.match_clip(x, c, M, seed_code=9, coins=np.ones(M * 8, bool))
    assert np.array_equal(before, knn.rng.get_state()[1]) and knn.seen[-1][0] == 9 and knn.seen[-1][1].all()
    # a guard overflow: the clip again on the exact path, from the SAME seed and coins, drawn once
    k4 = _StubMatcher(5, overflow=1)
    k4.match_clip(x, c, M)
    assert len(k4.seen) == 2 and k4.seen[0][0] == k4.seen[1][0] == want_seed
    assert np.array_equal(k4.seen[0][1], want_coins) and np.array_equal(k4.seen[1][1], want_coins)
    assert k4.fallbacks == 1 and k4.sweeps == [(False, "mixed"), (False, "exact")] and k4.audio_precision == "mixed"
    sa = k4.rng.get_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    # an empty clip draws its seed and no coin
    k5, r5 = _StubMatcher(8), np.random.RandomState(8)
    e = k5.match_clip(x[:0], c[:0], 0)
    r5.randint(0, 7), r5.randint(0, 172)
    assert e[0].shape == (0, 30) and e[1].shape == (0, 0, 8, 16) and not k5.sweeps
    assert k5.rng.randint(0, 1 << 30) == r5.randint(0, 1 << 30)


def test_refusals_of_a_no_phase_matcher():
    import torch
    knn = _StubMatcher(1)
    x, c = torch.zeros((2, 180, 8)), torch.zeros((2, 30, 384))
    for call in (lambda: knn.match_clip_takes(x, c, 2, n_takes=2),
                 lambda: ck.CodeKNN.walk_takes(knn, {}, 2, [1], np.zeros((1, 8, 16), np.float32)),
                 lambda: knn.capture_clip_graph(2),
                 lambda: ck.CodeKNN.walk(knn, {}, 2, sync=False),
                 lambda: ck.ClipPipeline(knn.db, use_phase=False),
                 lambda: ck.GraphPipeline(knn.db, 2, use_phase=False)):
        with pytest.raises(NotImplementedError, match="phase gate"):
            call()
    knn.force_sharded = True
    with pytest.raises(NotImplementedError, match="row-sharded"):
        knn.match_clip(x, c, 2)
    for bad in (-1, 16):
        with pytest.raises(ValueError):
            _StubMatcher(1, desired_k=bad)
    assert _StubMatcher(1, desired_k=15).desired_k == 15
    # a gated matcher keeps ignoring desired_k (the reference's phase branches never read it)
    assert ck.CodeKNN(knn.db, desired_k=99).use_phase


def test_plan_nophase():
    kn, db = ck.Knobs(), ck.DBFacts(2048, 2048, 1, 512, 26, 1024, 384)
    for mode in (ck.MODE_AUD_TXT, ck.MODE_AUD, ck.MODE_TXT):
        for k in (0, 3, 15):
            p = ck.plan_nophase(kn, db, 6, 8, mode, k)
            assert p.path == "kernel" and p.for_walk is False and "settled" in p.reason
    # the settled tables: the step plan of for_walk=False has neither the cut nor the prefused gate tables, with the
    # matcher's defaults (rank_cut on, split_fuse on), where the gated walk's plan has both
    settled, gated = ck.plan_step(kn, db, 6, 8, ck.MODE_AUD_TXT, for_walk=False), ck.plan_step(kn, db, 6, 8, for_walk=True)
    assert settled.audio.cut_top_n == 0 and not settled.split_fuse
    assert gated.audio.cut_top_n == 1 and gated.split_fuse
    for k in (-1, 16):
        assert ck.plan_nophase(kn, db, 6, 8, 0, k).path == "unsupported"
    assert "row-sharded" in ck.plan_nophase(kn, db._replace(world=2), 6, 8, 0, 0).reason
    assert "row-sharded" in ck.plan_nophase(kn._replace(force_sharded=True), db, 6, 8, 0, 0).reason
    for M, steps, K in ((6, 9, 512), (257, 8, 512), (2, 8, 2048), (2, 8, 510), (2, 16, 768)):
        p = ck.plan_nophase(kn, db._replace(K=K), M, steps, 0, 0)
        assert p.path == "unsupported" and "geometry" in p.reason, (M, steps, K)
    for M, steps, K in ((256, 8, 512), (3, 7, 64), (2, 8, 1024), (2, 8, 500), (0, 8, 512)):
        assert ck.plan_nophase(kn, db._replace(K=K), M, steps, 0, 0).path == "kernel", (M, steps, K)
    assert ck.plan_nophase(kn, db, 6, 8, 0x200, 0).path == "unsupported"


def test_command_line_flags(capsys):
    p = GestureKNN.build_parser()
    a = p.parse_args([])
    assert a.no_phase is False and a.desired_k == 0
    a = p.parse_args(["--no_phase", "--desired_k", "3", "--mode", "audio"])
    assert a.no_phase is True and a.desired_k == 3 and a.mode == "audio"
    assert p.parse_args(["-k", "3"]).no_phase is False
    GestureKNN.check_args(p, p.parse_args(["--no_phase", "--n_takes", "1"]))
    GestureKNN.check_args(p, p.parse_args(["--desired_k", "99", "--n_takes", "4"]))     # ignored without --no_phase
    for bad in (["--no_phase", "--n_takes", "2"], ["--no_phase", "-k", "16"], ["--no_phase", "-k", "-1"]):
        with pytest.raises(SystemExit):
            GestureKNN.main(bad)                      # refused before anything is loaded
    assert "--no_phase with --n_takes > 1" in capsys.readouterr().err
    need = []
    for k in ("test_data", "train_database", "train_codebook", "codebook_signature", "train_wavlm", "test_wavlm", "config",
              "VQVAE_model_path"):
        need += ["--" + k, "x"]
    a = inference.build_parser().parse_args(need + ["--no_phase", "--desired_k", "3"])
    assert a.no_phase is True and a.desired_k == 3
    assert inference.nophase_flags() == [] and inference.nophase_flags(True, 3) == ["--no_phase", "--desired_k", "3"]
    b = p.parse_args(inference.nophase_flags(True, 3))
    assert b.no_phase and b.desired_k == 3


def test_the_header_declares_the_entry_point():
    protos, consts = _lib.parse_header()
    assert consts["QPG_NOPHASE_KMAX"] == 16 == NR.KMAX == _lib.QPG_NOPHASE_KMAX
    f = protos["qpg_match_steps_nophase"]
    assert f.on_stream and not f.hook and len(f.argtypes) == 30 and f.restype is _lib.ctypes.c_int
    assert f.argtypes[28:] == [_lib.c_void_p, _lib.ctypes.c_size_t] and f.argtypes[26] is _lib.ctypes.c_int64
    ws = protos["qpg_match_steps_nophase_ws_bytes"]
    assert ws.restype is _lib.ctypes.c_size_t and ws.argtypes == [_lib.ctypes.c_int] * 4 and not ws.on_stream
    assert {"qpg_match_steps_nophase", "qpg_match_steps_nophase_ws_bytes"} <= set(_lib.declared_symbols())
