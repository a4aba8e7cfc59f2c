"""CPU tests of the multi-take feature: the C ABI's declaration and binding, the coalescence report
(first_shared_code / n_distinct), the plan function's decisions, the command lines' new flags, and the rng contract of
CodeKNN.match_clip_takes (a matcher whose device work is stubbed out)."""
import ctypes
import types

import numpy as np
import pytest

from qpgesture_amd import _lib, takes
from qpgesture_amd import code_knn as ck


def test_match_steps_takes_is_declared_and_bound():
    protos, consts = _lib.parse_header()
    assert "qpg_match_steps_takes" in protos and "qpg_match_steps_takes_ws_bytes" in protos
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    p = protos["qpg_match_steps_takes"]
    # qpg_match_steps_batch's arguments (n_takes in the place of n_chains) + the workspace and its size
    batch = protos["qpg_match_steps_batch"]
    assert p.on_stream and not p.hook and p.restype is I
    assert p.argtypes == batch.argtypes + [P, ctypes.c_size_t]
    assert p.argtypes[22:26] == [I, P, P, P] and p.argtypes[30:32] == [L, P]
    w = protos["qpg_match_steps_takes_ws_bytes"]
    assert not w.on_stream and w.restype is ctypes.c_size_t and w.argtypes == [I, I, I]
    assert consts["QPG_TAKES_MAX"] >= 1024 and _lib.QPG_TAKES_MAX == consts["QPG_TAKES_MAX"]
    lib = _lib.load()
    assert "qpg_match_steps_takes" in _lib.declared_symbols() and hasattr(lib, "qpg_match_steps_takes")
    # the trail of states: one u16 per (take, step) + the takes' first steps
    assert lib.qpg_match_steps_takes_ws_bytes(64, 6, 8) >= 2 * (64 + 64 * 48)
    assert lib.qpg_match_steps_takes_ws_bytes(1024, 6, 8) >= 2 * (1024 + 1024 * 48)
    assert lib.qpg_match_steps_takes_ws_bytes(0, 6, 8) == 0
    # argument checks happen before anything touches a device
    assert lib.qpg_match_steps_takes(*[None if t is P else 0 for t in p.argtypes]) == _lib.QPG_EINVAL
    assert "qpg_match_steps_takes" in _lib.last_error()
    assert issubclass(_lib.Unsupported, RuntimeError)
    assert 0 < _lib.QPG_OPT_TAKES_STAGES < _lib.QPG_OPT_COUNT               # (measurement knob of tools/bench_takes.py)


def _brute_first_shared(c):
    S, L = c.shape
    out = []
    for s in range(S):
        best = L
        for k in range(L):
            if any((c[e, k:] == c[s, k:]).all() for e in range(s)):
                best = k
                break
        out.append(best)
    return np.array(out, np.int64)


def test_first_shared_code_and_n_distinct_vs_brute_force():
    rs = np.random.RandomState(0)
    for trial in range(200):
        S, M = rs.randint(1, 9), rs.randint(1, 3)
        L = M * rs.randint(1, 7)
        c = rs.randint(0, 4, size=(S, L))
        for _ in range(rs.randint(0, 4)):                   # planted shared suffixes and duplicates
            a, b = rs.randint(0, S, 2)
            k = rs.randint(0, L + 1)
            c[b, k:] = c[a, k:]
        want = _brute_first_shared(c)
        assert np.array_equal(takes.first_shared_code(c), want), (trial, c)
        assert np.array_equal(takes.first_shared_code(c.reshape(S, M, L // M)), want)          # [S, M, 30]-shaped input
        assert takes.n_distinct(c) == len({r.tobytes() for r in c})
        assert takes.n_distinct(c) == S - int(((want == 0) & (np.arange(S) > 0)).sum())
    c = np.array([[1, 2, 3, 4], [5, 2, 3, 4], [1, 2, 3, 4], [9, 9, 9, 9], [9, 9, 9, 4]])
    assert takes.first_shared_code(c).tolist() == [4, 1, 0, 4, 3] and takes.n_distinct(c) == 4
    assert takes.first_shared_code(c[:1]).tolist() == [4]
    assert takes.n_distinct(np.zeros((3, 0, 30), np.int64)) == 1 and takes.n_distinct(np.zeros((0, 2, 30))) == 0
    assert takes.first_shared_code(np.zeros((3, 0, 30), np.int64)).tolist() == [0, 0, 0]


def test_plan_takes_decisions():
    db = ck.DBFacts(2048, 2048, 1, 512, 26, 1024, 384)
    kn = ck.Knobs()
    assert ck.plan_takes(kn, db, 6, 8, 64) == ck.TakesPlan("kernel", "")
    assert ck.plan_takes(kn, db, 1, 8, 1).path == "kernel" and ck.plan_takes(kn, db, 6, 8, 1024).path == "kernel"
    # tables ranked on the host, the wavvq sweep's tables, exact tables: the kernels read ranks and candidates only
    assert ck.plan_takes(kn._replace(host_ranks=True), db, 6, 8, 64).path == "kernel"
    assert ck.plan_takes(kn._replace(use_wavvq=True), db, 6, 8, 64).path == "kernel"
    assert ck.plan_takes(kn._replace(audio_precision="exact"), db, 6, 8, 64).path == "kernel"
    # the one-wave sequential walk / geometries the tabulation refuses: one walk per take
    p = ck.plan_takes(kn, db, 6, 8, 64, serial_walk=True)
    assert p.path == "per_take" and "serial" in p.reason
    assert ck.plan_takes(kn, db, 6, 7, 64).path == "kernel"                 # 28 codes kept: the last one is the last step's
    assert ck.plan_takes(kn, db, 6, 9, 64).path == "per_take"               # the 30th code is not the last step's
    assert ck.plan_takes(kn, db, 257, 8, 64).path == "per_take"             # more than 2048 steps per clip
    assert ck.plan_takes(kn, db._replace(K=2048), 6, 8, 64).path == "per_take"          # the double buffer leaves 64 KB
    assert ck.plan_takes(kn, db, 6, 8, _lib.QPG_TAKES_MAX + 1).path == "per_take"
    # row shards: not at all
    for p in (ck.plan_takes(kn, db._replace(world=2, n_local=1024), 6, 8, 64),
              ck.plan_takes(kn._replace(force_sharded=True), db, 6, 8, 64)):
        assert p.path == "unsupported" and "shard" in p.reason


def test_command_line_flags_and_defaults():
    from qpgesture_amd import GestureKNN, VisualizeCodebook, inference
    p = GestureKNN.build_parser()
    assert p.parse_args([]).n_takes == 1 and p.parse_args(["--n_takes", "16"]).n_takes == 16
    with pytest.raises(SystemExit):
        p.parse_args(["--n_takes", "many"])
    v = VisualizeCodebook.build_parser()
    assert v.parse_args([]).takes is None
    assert v.parse_args(["--takes", "all"]).takes == "all" and v.parse_args(["--takes", "3"]).takes == 3
    for bad in ("-1", "some", "1.5"):
        with pytest.raises(SystemExit):
            v.parse_args(["--takes", bad])
    codes = np.arange(4 * 2 * 30).reshape(4, 2, 30)
    assert VisualizeCodebook.select_takes(codes, "all")[0] == [0, 1, 2, 3]
    ix, c = VisualizeCodebook.select_takes(codes, 2)
    assert ix == [2] and c.shape == (1, 2, 30) and np.array_equal(c[0], codes[2])
    with pytest.raises(IndexError):
        VisualizeCodebook.select_takes(codes, 4)
    need = sum((["--" + k, "x"] for k in ("test_data", "train_database", "train_codebook", "codebook_signature", "train_wavlm",
                                          "test_wavlm", "config", "VQVAE_model_path")), [])
    a = inference.build_parser().parse_args(need)
    assert a.n_takes == 1 and a.takes is None
    a = inference.build_parser().parse_args(need + ["--n_takes", "8", "--takes", "all"])
    assert a.n_takes == 8 and a.takes == "all"
    assert inference.takes_flags() == [] and inference.takes_flags(8, "all") == ["--n_takes", "8", "--takes", "all"]
    assert inference.takes_flags(1, 2) == ["--takes", "2"]
    # the flags reach the two command lines they belong to
    assert GestureKNN.build_parser().parse_args(inference.takes_flags(8, None)).n_takes == 8
    assert VisualizeCodebook.build_parser().parse_args(inference.takes_flags(1, "all")).takes == "all"


class _StubMatcher(ck.CodeKNN):
    """A CodeKNN whose device work is replaced by records of what it was asked for."""

    def __init__(self, seed):
        import torch
        rs = np.random.RandomState(99)
        fake = types.SimpleNamespace(step_sz=6, T=180, N=7, device=torch.device("cpu"), n_local=7, world=1, K=512, Ga=26,
                                     F=8, Dt=384, feature_dtype="f32", hl_bound_ok=True, hl_image=None, txt_sorted=None,
                                     hl_planes=2, code_host=rs.randint(0, 512, (7, 30)).astype(np.int64),
                                     phase_host=rs.standard_normal((7, 240, 2, 8)).astype(np.float32))
        super().__init__(fake, rng=np.random.RandomState(seed))
        self.seen, self.sweeps = [], 0

    def sweep_tables(self, *a, **k):
        self.sweeps += 1
        return {}

    def walk(self, T, M, off=0, mode=0, seed_code=None, seed_phase=None, **k):
        self.seen.append((int(seed_code), np.asarray(seed_phase).copy()))
        return np.zeros((M, 30), np.int64), np.zeros((M, 8, 8, 16), np.float32), np.zeros((M, 8), np.int32)

    def walk_takes(self, T, M, seed_codes, seed_phases, mode=0, **k):
        S = len(seed_codes)
        self.seen.extend((int(c), np.asarray(p).copy()) for c, p in zip(seed_codes, seed_phases))
        codes = np.repeat(np.asarray(seed_codes)[:, None, None], M * 30, axis=1).reshape(S, M, 30).astype(np.int64)
        return codes, np.zeros((S, M, 8, 8, 16), np.float32), np.zeros((S, M, 8), np.int32)


def test_match_clip_takes_consumes_the_rng_as_successive_match_clips_do():
    import torch
    S, M = 9, 3
    x, c = torch.zeros((M, 180, 8)), torch.zeros((M, 30, 384))
    a, b = _StubMatcher(5), _StubMatcher(5)
    for _ in range(S):
        a.match_clip(x, c, M)
    r = b.match_clip_takes(x, c, M, n_takes=S)
    assert a.sweeps == S and b.sweeps == 1                              # ONE sweep for all takes
    assert [s[0] for s in a.seen] == [s[0] for s in b.seen] == r.seed_codes.tolist()
    assert all(np.array_equal(p[1], q[1]) for p, q in zip(a.seen, b.seen))
    sa, sb = a.rng.get_state(), b.rng.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]          # the rng ends in the same state
    assert a.rng.randint(0, 1 << 30) == b.rng.randint(0, 1 << 30)
    assert r.codes.shape == (S, M, 30) and r.n_distinct == len(set(r.seed_codes.tolist()))
    assert np.array_equal(r.first_shared_code, takes.first_shared_code(r.codes))
    # explicit seeds draw nothing
    before = b.rng.get_state()[1].copy()
    b.match_clip_takes(x, c, M, seed_codes=[1, 2], seed_phases=np.zeros((2, 8, 16), np.float32))
    assert np.array_equal(before, b.rng.get_state()[1])
    # an empty clip still draws its seeds (match_clip draws before it looks at the clip)
    e, f = _StubMatcher(6), _StubMatcher(6)
    for _ in range(4):
        e.match_clip(x[:0], c[:0], 0)
    out = f.match_clip_takes(x[:0], c[:0], 0, n_takes=4)
    assert out.codes.shape == (4, 0, 30) and e.rng.randint(0, 1 << 30) == f.rng.randint(0, 1 << 30) and f.sweeps == 0
    for bad in (dict(n_takes=0), dict(), dict(seed_codes=[512], seed_phases=np.zeros((1, 8, 16))),
                dict(seed_codes=[1, 2], seed_phases=np.zeros((1, 8, 16)))):
        with pytest.raises(ValueError):
            b.match_clip_takes(x, c, M, **bad)
