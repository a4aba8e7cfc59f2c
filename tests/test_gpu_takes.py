"""GPU tests of the multi-take walk (qpg_match_steps_takes, CodeKNN.walk_takes / match_clip_takes): S takes
of one clip from one sweep equal S one-take matches, bit for bit; against the oracle on the reference-generated fixtures;
trouble words, absent codes, bad seeds, shards.  Every comparison is exact integer / bit equality."""
import numpy as np
import pytest

from tests.helpers import fixture_arrays, load_golden

pytestmark = pytest.mark.gpu


def _db(N, seed, F=1024, speechlike=False):
    from qpgesture_amd import synth
    from qpgesture_amd.data_processing import interp_wavlm
    tr = synth.make_db(N, seed, F)
    if speechlike:
        synth.speechlike_transform(tr, seed + 7)
    return dict(interp=interp_wavlm(tr["wavlm"]), ctx=np.ascontiguousarray(tr["context"].squeeze(2)),
                code=synth.make_codes(N, seed + 1), phase=tr["phase_dense"], sig=synth.make_signature(seed + 2))


def _seeds(rs, S, K=512):
    """S random seeds; several takes share a seed CODE (different phase blocks), two share a whole seed."""
    sc = rs.randint(0, K, size=S).astype(np.int64)
    sp = rs.standard_normal((S, 8, 16)).astype(np.float32)
    if S >= 8:
        sc[S // 2], sc[S // 2 + 1], sc[S - 1] = sc[0], sc[0], sc[1]
        sp[S - 1] = sp[1]                                    # take S - 1 IS take 1
    return sc, sp


def _equal(got, want_list, what=""):
    """got: (codes [S..], phases, votes) of the takes; want_list[s]: (codes, phases, votes) of take s alone."""
    for s, w in enumerate(want_list):
        assert got[0][s].dtype == np.int64 and np.array_equal(got[0][s], w[0]), "%s take %d: codes" % (what, s)
        assert np.array_equal(got[2][s], w[2]), "%s take %d: votes" % (what, s)
        ph = np.asarray(w[1])
        assert got[1][s].dtype == np.float32 and got[1][s].shape == ph.shape
        assert np.array_equal(got[1][s].view(np.uint32), np.ascontiguousarray(ph, np.float32).view(np.uint32)) and \
            np.array_equal(got[1][s], ph), "%s take %d: phase blocks" % (what, s)


@pytest.fixture(scope="module", params=[False, True], ids=["synthetic", "speechlike"])
def fullsize(request):
    import torch
    from qpgesture_amd.code_knn import GestureDB
    N, M = 2048, 6
    d = _db(N, 41, speechlike=request.param)
    dev = torch.device("cuda:0")
    db = GestureDB(d["code"], d["interp"], d["ctx"], d["phase"], d["sig"], device=dev)
    te = _db(M, 97, speechlike=request.param)
    return db, torch.from_numpy(te["interp"]).to(dev), torch.from_numpy(te["ctx"]).to(dev), M


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_takes_equal_one_take_matches_full_size(fullsize, mode):
    """N = 2048, 64 seeds (repeated seed codes, one repeated seed): every take's codes, votes and phase blocks are those of
    match_clip with that seed - from match_clip_takes, and from walk_takes on for_walk tables, on exact (return_tables)
    tables and on host-ranked tables.  One take equals walk()."""
    from qpgesture_amd.code_knn import CodeKNN
    db, te_i, te_c, M = fullsize
    knn = CodeKNN(db, rng=np.random.RandomState(2))
    sc, sp = _seeds(np.random.RandomState(100 + mode), 64)
    want = [knn.match_clip(te_i, te_c, M, mode=mode, seed_code=int(sc[s]), seed_phase=sp[s]) for s in range(64)]
    r = knn.match_clip_takes(te_i, te_c, M, seed_codes=sc, seed_phases=sp, mode=mode)
    assert knn.fallbacks == 0
    assert r.codes.shape == (64, M, 30) and r.phases.shape == (64, M, 8, 8, 16) and r.votes.shape == (64, M, 8)
    _equal(r, want, "match_clip_takes")
    assert np.array_equal(r.seed_codes, sc) and r.first_shared_code[63] == 0          # take 63 is take 1 again
    assert r.n_distinct == len({w[0].tobytes() for w in want})
    Tw = knn.sweep_tables(te_i, te_c, M, mode=mode, for_walk=True)
    assert (Tw.get("gate_tables") is not None) == (mode == 0)                          # (prefused where the fusion is split)
    _equal(knn.walk_takes(Tw, M, sc, sp, mode=mode), want, "for_walk tables")
    Tx = knn.sweep_tables(te_i, te_c, M, mode=mode)
    _equal(knn.walk_takes(Tx, M, sc, sp, mode=mode), want, "exact tables")
    one = knn.walk_takes(Tx, M, sc[5:6], sp[5:6], mode=mode)
    alone = knn.walk(Tx, M, mode=mode, seed_code=int(sc[5]), seed_phase=sp[5])
    _equal(one, [alone], "one take")
    # device results without a wait
    oc, op, ov, st = knn.walk_takes(Tx, M, sc, sp, mode=mode, sync=False)
    assert st.cpu().numpy().tolist() == [[0, 0]] * 64
    _equal((oc.cpu().numpy().astype(np.int64), op.cpu().numpy(), ov.cpu().numpy()), want, "sync=False")
    # windows [2, 5) of the tables
    part = knn.walk_takes(Tx, 3, sc[:8], sp[:8], mode=mode, window_offset=2)
    _equal(part, [knn.walk(Tx, 3, 2, mode=mode, seed_code=int(sc[s]), seed_phase=sp[s]) for s in range(8)], "offset")
    knn.host_ranks = True
    Th = knn.sweep_tables(te_i, te_c, M, mode=mode)
    want_h = [knn.match_clip(te_i, te_c, M, mode=mode, seed_code=int(sc[s]), seed_phase=sp[s]) for s in range(0, 64, 4)]
    got_h = knn.walk_takes(Th, M, sc[::4], sp[::4], mode=mode)
    _equal(got_h, want_h, "host ranks")


def test_1024_takes_and_a_one_window_clip(fullsize):
    """S = 1024 (every code seeds two takes) against walk() on the same tables; M = 1 against match_clip; the serial walk
    (where the multi-take kernels do not apply) falls back to one walk per take, with the same results."""
    from qpgesture_amd.code_knn import CodeKNN, plan_takes
    db, te_i, te_c, M = fullsize
    knn = CodeKNN(db, rng=np.random.RandomState(3))
    rs = np.random.RandomState(9)
    sc = np.concatenate((np.arange(512), rs.permutation(512))).astype(np.int64)
    sp = rs.standard_normal((1024, 8, 16)).astype(np.float32)
    T = knn.sweep_tables(te_i, te_c, M, for_walk=True)
    got = knn.walk_takes(T, M, sc, sp)
    _equal(got, [knn.walk(T, M, seed_code=int(sc[s]), seed_phase=sp[s]) for s in range(1024)], "1024 takes")
    sc1, sp1 = _seeds(rs, 64)
    r = knn.match_clip_takes(te_i[:1].contiguous(), te_c[:1].contiguous(), 1, seed_codes=sc1, seed_phases=sp1)
    _equal(r, [knn.match_clip(te_i[:1].contiguous(), te_c[:1].contiguous(), 1, seed_code=int(sc1[s]), seed_phase=sp1[s])
               for s in range(64)], "M = 1")
    knn.serial_walk = True
    assert plan_takes(knn._knobs(), knn._facts(), M, 8, 16, serial_walk=True).path == "per_take"
    T = knn.sweep_tables(te_i, te_c, M)
    _equal(knn.walk_takes(T, M, sc[500:516], sp[500:516]), [(got[0][s], got[1][s], got[2][s]) for s in range(500, 516)],
           "serial fallback")


def test_the_library_refuses_the_serial_walk_with_eunsup(fullsize):
    """qpg_match_steps_takes with QPG_MODE_SERIAL_WALK: QPG_EUNSUP and a message, nothing launched."""
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.code_knn import CodeKNN
    db, te_i, te_c, M = fullsize
    knn = CodeKNN(db)
    T = knn.sweep_tables(te_i, te_c, M)
    dev, S, Q = db.device, 4, M * 8
    z = lambda *shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)          # noqa: E731
    ws = torch.full((int(_lib.load().qpg_match_steps_takes_ws_bytes(S, M, 8)),), 0x3C, dtype=torch.uint8, device=dev)    # (contents on entry are ignored)
    with pytest.raises(_lib.Unsupported, match="tabulated walk"):
        _lib.call("qpg_match_steps_takes", dev, T["aud_rank"], T["aud_idx"], T["txt_rank"], T["txt_idx"], db.pos_rank,
                  db.freq_rank, db.code, db.code.shape[1], db.aud_cidx, db.aud_pslot, db.Ga, db.txt_cidx, db.txt_pslot,
                  db.Gt, db.phase, db.Tp, _lib.QPG_MODE_SERIAL_WALK, M, 8, db.K, S, z(S), z(S, 8, 16, dt=torch.float32),
                  z(3, Q, db.K), z(S, M, 30), z(S, M, 8, 8, 16, dt=torch.float32), z(S, M, 8), z(S, 2), 2, None, ws,
                  ws.numel())


def _oracle_clip(ok, te_i, te_c, M, seed_code, seed_phase):
    """The oracle's window loop (oracle/knn_oracle.py predict_code_from_audio, GestureKNN.py:785-813) with an EXPLICIT
    first seed: window 0 starts from (seed_code, seed_phase), window w > 0 from the previous window's 30th code and last
    phase block."""
    from oracle import knn_oracle as O
    motion, phases, votes = [], [], []
    for w in range(M):
        def clip(i, w=w):
            return O.wavlm_feat_rows(te_i, w, [i])[0]
        c0 = motion[-1][-1] if w > 0 else seed_code
        p0 = phases[-1][-1] if w > 0 else seed_phase
        m, p, v = ok.search_code_knn(clip, te_c[w], seed_code=c0, seed_phase=p0)
        motion.append(m)
        phases.append(p)
        votes.append(v)
    return np.array(motion), np.array(phases), np.array(votes)


@pytest.mark.parametrize("name", ["shipped_n48_m2_s0", "shipped_n64_m3_s10"])
def test_takes_vs_oracle_on_the_reference_fixtures(name):
    """16 successive init_code_phase() draws of the oracle from RandomState(123456): take 0 is the fixture's knn_pred (the
    reference CLI's own run), every take is the oracle's clip from that seed, n_distinct is the oracle's count.  NumPy ranks
    in the oracle, its freq_rank() handed to the database.  Condition: the oracle met no tied decision for the seed; on
    shipped_n48_m2_s0 none of the 16 may tie, on shipped_n64_m3_s10 a seed that ties with NumPy ranks is left out (that
    seed and no other: an exact tie is ordered by NumPy's unstable sort, which the device's stable ranks need not follow)."""
    import torch
    from oracle import knn_oracle as O
    from qpgesture_amd import takes
    from qpgesture_amd.code_knn import CodeKNN, GestureDB
    g = load_golden(name)
    ntr, nte, s0, s1, s2, s3, mf = [int(v) for v in g["meta"]]
    A = fixture_arrays(ntr, nte, s0, s1, s2, s3)
    M = mf if mf else nte
    ok = O.CodeKNNOracle(A["code"], A["sig"], A["tr_phase"], A["tr_ctx"], wavlm_interp=A["tr_interp"],
                         rng=np.random.RandomState(123456), rank_kind="numpy", scan="c")
    draws = [ok.init_code_phase() for _ in range(16)]
    want, used = [], []
    for s, (c, p) in enumerate(draws):
        ok.tied_decisions = 0
        w = _oracle_clip(ok, A["te_interp"], A["te_ctx"], M, int(c), np.asarray(p, np.float32))
        if ok.tied_decisions:
            assert name == "shipped_n64_m3_s10", "seed %d ties on %s" % (s, name)
            print("%s: seed %d left out (%d tied decisions in the oracle)" % (name, s, ok.tied_decisions))
            continue
        want.append(w)
        used.append(s)
    assert used and used[0] == 0, "the reference's own seed must be usable"
    assert np.array_equal(want[0][0], g["knn_pred"])                          # (the oracle itself, on the reference's run)
    dev = "cuda:0"
    db = GestureDB(A["code"], A["tr_interp"], A["tr_ctx"], A["tr_phase"], A["sig"], device=dev, freq_rank=ok.freq_rank())
    knn = CodeKNN(db, rng=np.random.RandomState(123456))
    sc = np.array([int(draws[s][0]) for s in used], np.int64)
    sp = np.stack([np.asarray(draws[s][1], np.float32) for s in used])
    te_i = torch.from_numpy(A["te_interp"]).to(dev)
    te_c = torch.from_numpy(np.ascontiguousarray(A["te_ctx"])).to(dev)
    r = knn.match_clip_takes(te_i, te_c, M, seed_codes=sc, seed_phases=sp)
    assert np.array_equal(r.codes[0], g["knn_pred"]) and np.array_equal(r.votes[0], g["vote"])
    assert np.array_equal(r.phases[0], g["phase_out"])
    _equal(r, want, "oracle")
    n_oracle = takes.n_distinct(np.stack([w[0] for w in want]))
    print("%s: %d distinct code sequences among %d takes" % (name, n_oracle, len(used)))
    assert r.n_distinct == n_oracle
    assert np.array_equal(r.first_shared_code, takes.first_shared_code(np.stack([w[0] for w in want])))
    # the matcher's own draws are the oracle's: same rng, same two randint calls per seed
    r2 = knn.match_clip_takes(te_i, te_c, M, n_takes=16)
    assert np.array_equal(r2.seed_codes, [int(d[0]) for d in draws])
    assert np.array_equal(r2.codes[used], r.codes)


def test_a_raised_trouble_word_rematches_the_tables_once_for_all_takes():
    """The forced-overflow data (3 000 near-copies of one window): the capped lists overflow, the TABLES are matched again
    on the uncapped path - once - and all takes are walked from them: they equal the takes of an audio_precision "exact"
    matcher."""
    import torch
    from qpgesture_amd.code_knn import CodeKNN, GestureDB
    from tests.test_gpu_guard_overflow import _crowded
    A = _crowded(3000)
    dev = "cuda:0"
    db = GestureDB(A["code"], A["tr_interp"], A["tr_ctx"], A["tr_phase"], A["sig"], device=dev)
    te_i = torch.from_numpy(A["te_interp"]).to(dev)
    te_c = torch.from_numpy(np.ascontiguousarray(A["te_ctx"])).to(dev)
    sc, sp = _seeds(np.random.RandomState(4), 16)
    knn = CodeKNN(db, rng=np.random.RandomState(7))
    r = knn.match_clip_takes(te_i, te_c, 2, seed_codes=sc, seed_phases=sp)
    assert knn.fallbacks == 1 and knn.mixed_stats()["flags"] == 0
    kx = CodeKNN(db, rng=np.random.RandomState(7))
    kx.audio_precision = "exact"
    rx = kx.match_clip_takes(te_i, te_c, 2, seed_codes=sc, seed_phases=sp)
    assert kx.fallbacks == 0
    _equal(r, [(rx.codes[s], rx.phases[s], rx.votes[s]) for s in range(16)], "re-matched")
    _equal(r, [kx.match_clip(te_i, te_c, 2, seed_code=int(sc[s]), seed_phase=sp[s]) for s in range(16)], "exact one-take")


def test_errors_absent_code_bad_seeds_shards():
    import torch
    from qpgesture_amd import synth
    from qpgesture_amd.code_knn import CodeKNN, GestureDB
    from qpgesture_amd.data_processing import interp_wavlm
    A = _db(1, 600, F=128)
    A["code"][:] = 7                                                       # a single code in the whole DB
    te = synth.make_db(1, 601, 128)
    db = GestureDB(A["code"], A["interp"], A["ctx"], A["phase"], A["sig"], device="cuda:0")
    knn = CodeKNN(db, rng=np.random.RandomState(3))
    te_i = torch.from_numpy(interp_wavlm(te["wavlm"])).cuda()
    te_c = torch.from_numpy(np.ascontiguousarray(te["context"].squeeze(2))).cuda()
    with pytest.raises(IndexError, match="take "):
        # previous code is 7 itself -> pos_dist[7] = inf -> its fused rank is worst -> an absent code wins
        knn.match_clip_takes(te_i, te_c, 1, n_takes=4)
    sp = np.zeros((2, 8, 16), np.float32)
    for bad_codes, bad_phases in (([0, 512], sp), ([-1, 3], sp), ([1, 2], sp[:1]), ([], sp[:0]), ([0.5, 1.0], sp),
                                  ([[1, 2]], sp)):
        with pytest.raises(ValueError):
            knn.match_clip_takes(te_i, te_c, 1, seed_codes=bad_codes, seed_phases=bad_phases)
    with pytest.raises(ValueError):
        knn.match_clip_takes(te_i, te_c, 1)                                 # neither n_takes nor seeds
    with pytest.raises(ValueError):
        knn.match_clip_takes(te_i, te_c, 1, n_takes=3, seed_codes=[1, 2], seed_phases=sp)
    empty = knn.match_clip_takes(te_i, te_c, 0, n_takes=3)
    assert empty.codes.shape == (3, 0, 30) and empty.n_distinct == 1
    knn.force_sharded = True                                                # the row-shard code path
    T = dict(aud_rank=None, aud_idx=None, txt_rank=None, txt_idx=None)
    with pytest.raises(NotImplementedError, match="shard"):
        knn.walk_takes(T, 1, [1, 2], sp)
    with pytest.raises(NotImplementedError, match="shard"):
        knn.capture_clip_graph(1, n_takes=2)


def test_captured_replays_with_takes(fullsize):
    """capture_clip_graph(..., n_takes=16): a replay equals match_clip_takes; replays with fresh seeds stay correct after
    eager clips in between; the several-clips accessors read the takes; the default capture's results are unchanged."""
    import torch
    from qpgesture_amd.code_knn import CodeKNN
    db, te_i, te_c, M = fullsize
    knn = CodeKNN(db, rng=np.random.RandomState(11))
    rs = np.random.RandomState(12)
    g = knn.capture_clip_graph(M, audio=te_i, context=te_c, n_takes=16)
    assert g.n_takes == 16
    for rnd in range(4):
        sc, sp = _seeds(rs, 16)
        r = g.run_takes(sc, sp)
        want = knn.match_clip_takes(te_i, te_c, M, seed_codes=sc, seed_phases=sp)
        _equal(r, [(want.codes[s], want.phases[s], want.votes[s]) for s in range(16)], "replay %d" % rnd)
        assert r.n_distinct == want.n_distinct and np.array_equal(r.first_shared_code, want.first_shared_code)
        ints = g.run_ints(sc, sp)                                           # the several-clips layout, takes for clips
        assert np.array_equal(g.codes(ints), want.codes) and g.statuses(ints).tolist() == [[0, 0]] * 16
        for _ in range(10):                                                 # eager clips in between
            knn.match_clip(te_i, te_c, M, seed_code=int(sc[0]), seed_phase=sp[0])
    # an eager call with more takes grows the matcher's workspace; the capture keeps the one it recorded
    ws_before = knn._takes_ws.data_ptr()
    knn.match_clip_takes(te_i, te_c, M, n_takes=300)
    assert knn._takes_ws.data_ptr() != ws_before and g._takes_ws.data_ptr() == ws_before
    hold = [torch.zeros((1 << 16,), dtype=torch.uint8, device=te_i.device) for _ in range(8)]      # (what could reuse it)
    _equal(g.run_takes(sc, sp), [(want.codes[s], want.phases[s], want.votes[s]) for s in range(16)], "after growth")
    assert all(int(h.sum()) == 0 for h in hold)
    assert g.captures == 1 and knn.fallbacks == 0
    # the default capture: one take, the results of today's replay
    g1 = knn.capture_clip_graph(M, audio=te_i, context=te_c)
    assert g1.n_takes == 1 and g1.CL == 1
    out = g1.run(te_i, te_c, int(sc[3]), sp[3])
    assert np.array_equal(out[0].numpy(), want.codes[3]) and np.array_equal(out[2].numpy(), want.votes[3])
    assert np.array_equal(out[1].cpu().numpy(), want.phases[3]) and out[3].tolist() == [0, 0]
    alone = knn.match_clip(te_i, te_c, M, seed_code=int(sc[3]), seed_phase=sp[3])
    assert np.array_equal(out[0].numpy(), alone[0])
    with pytest.raises(ValueError):
        g.run_takes(sc[:4], sp[:4])
    for kw in (dict(n_clips=2), dict(doorbell=True)):
        with pytest.raises(NotImplementedError):
            knn.capture_clip_graph(M, n_takes=4, **kw)
    with pytest.raises(ValueError):
        knn.capture_clip_graph(M, n_takes=0)


def test_a_flagged_replay_goes_through_match_clip_takes():
    """A captured replay on the forced-overflow data raises its trouble word: run_takes returns the takes of the re-matched
    tables (match_clip_takes), never the flagged codes, and later replays do not inherit the word."""
    import torch
    from qpgesture_amd.code_knn import CodeKNN, GestureDB
    from tests.test_gpu_guard_overflow import _crowded
    A = _crowded(3000)
    dev = "cuda:0"
    db = GestureDB(A["code"], A["tr_interp"], A["tr_ctx"], A["tr_phase"], A["sig"], device=dev)
    te_i = torch.from_numpy(A["te_interp"]).to(dev)
    te_c = torch.from_numpy(np.ascontiguousarray(A["te_ctx"])).to(dev)
    sc, sp = _seeds(np.random.RandomState(4), 8)
    knn = CodeKNN(db, rng=np.random.RandomState(7))
    g = knn.capture_clip_graph(2, audio=te_i, context=te_c, n_takes=8)
    r = g.run_takes(sc, sp)
    assert knn.fallbacks == 1
    kx = CodeKNN(db, rng=np.random.RandomState(7))
    kx.audio_precision = "exact"
    rx = kx.match_clip_takes(te_i, te_c, 2, seed_codes=sc, seed_phases=sp)
    _equal(r, [(rx.codes[s], rx.phases[s], rx.votes[s]) for s in range(8)], "flagged replay")
    r2 = g.run_takes(sc, sp)
    assert knn.fallbacks == 2 and np.array_equal(r2.codes, rx.codes)
