"""The walk's kernels (qpgesture_amd/csrc/qpg_tail.hip) against the NumPy statement of their contract (tests/walk_ref.py,
pinned to the reference's goldens by tests/test_walk_contract_cpu.py) on inputs built to break them: fused minima that
tie, winners at every depth of the rank order and on the boundary of a scan round, 1 024 distinct keys in the dedup hash,
gate ties / near ties / barely normalisable gate vectors, absent codes.  Through the C ABI (GestureDB fixes K = 512).

EVERY comparison is exact: candidate tables (regions [0] / [1] of gate_tables, the layout QPG_MODE_PREFUSED documents), the
u16 gate table of the tabulated forms (region [2]), codes, votes, status words equal; phase blocks bit-equal."""
import functools

import numpy as np
import pytest

from tests import walk_ref as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SERIAL, PREFUSED = 0x100, 0x200
FOUR = (0, 5, 300, 777)                       # seeds of the one-clip calls; 5 carries the all-zero phase block


def _t(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


class _Device:
    """A Problem's arrays on the device (uploaded once per problem object)."""

    def __init__(self, P):
        self.P = P
        self.aud_rank, self.txt_rank = _t(P.aud_rank, np.int16), _t(P.txt_rank, np.int16)
        self.aud_idx, self.txt_idx = _t(P.aud_idx, np.int32), _t(P.txt_idx, np.int32)
        self.pos_rank, self.freq_rank = _t(P.pos_rank, np.int16), _t(P.freq_rank, np.int16)
        self.code, self.phase = _t(P.code, np.int32), _t(P.phase, np.float32)
        self.a_cidx, self.a_pslot = _t(P.aud_cidx, np.int32), _t(P.aud_pslot, np.int32)
        self.t_cidx, self.t_pslot = _t(P.txt_cidx, np.int32), _t(P.txt_pslot, np.int32)
        assert int(P.aud_pslot.max()) + 32 <= P.phase.shape[1] and int(P.txt_pslot.max()) + 32 <= P.phase.shape[1]
        assert int(P.aud_cidx.max()) + 4 <= P.code.shape[1] and int(P.txt_cidx.max()) + 4 <= P.code.shape[1]
        assert int(P.aud_idx.max()) < P.phase.shape[0] * len(P.aud_cidx)
        assert int(P.txt_idx.max()) < P.phase.shape[0] * len(P.txt_cidx)
        assert 0 <= int(P.code.min()) and int(P.code.max()) < P.K

    def head(self, rows, mode, M):
        P = self.P
        return (self.aud_rank[rows], self.aud_idx[rows], self.txt_rank[rows], self.txt_idx[rows], self.pos_rank,
                self.freq_rank, self.code, P.code.shape[1], self.a_cidx, self.a_pslot, len(P.aud_cidx), self.t_cidx,
                self.t_pslot, len(P.txt_cidx), self.phase, P.phase.shape[1], mode, M, P.steps, P.K)


@functools.lru_cache(maxsize=None)
def _device(name, variant=None):
    P = W.case(name)
    if variant is not None:
        P = W.with_absent(P, 0, variant)
    return _Device(P)


def _outputs(P, n, M, chains=1):
    import torch
    Q = chains * M * P.steps
    return dict(gate=torch.full((3, Q, P.K), -9, dtype=torch.int32, device=DEV),
                codes=torch.full((n, M, P.codes_per_window), -9, dtype=torch.int32, device=DEV),
                phase=torch.full((n, M, P.steps, 8, 16), float("nan"), dtype=torch.float32, device=DEV),
                vote=torch.full((n, M, P.steps), -9, dtype=torch.int32, device=DEV))


def _prefuse(D, rows, o, Q):
    from qpgesture_amd import _lib
    _lib.call("qpg_fuse_best_ranked", DEV, D.aud_rank[rows], D.aud_idx[rows], D.pos_rank, D.freq_rank, Q, D.P.K, o["gate"][0])
    _lib.call("qpg_fuse_best_ranked", DEV, D.txt_rank[rows], D.txt_idx[rows], D.pos_rank, D.freq_rank, Q, D.P.K, o["gate"][1])


def _gate_u16(o, Q, K):
    return o["gate"][2].contiguous().view(__import__("torch").int16).cpu().numpy().view(np.uint16).reshape(Q, 2 * K)


def _match(D, mode, flags, seed, guard=None):
    """One qpg_match_steps call -> numpy outputs, the two candidate tables and the raw third region."""
    import torch
    from qpgesture_amd import _lib
    P = D.P
    o = _outputs(P, 1, P.M)
    status = torch.full((2,), -9, dtype=torch.int32, device=DEV)
    rows = slice(0, P.Q)
    if flags & PREFUSED:
        _prefuse(D, rows, o, P.Q)
    g = None if guard is None else _t([guard], np.int32)
    _lib.call("qpg_match_steps", DEV, *D.head(rows, mode | flags, P.M), int(P.seed_codes[seed]),
              _t(P.seed_phases[seed], np.float32), o["gate"], o["codes"][0], o["phase"][0], o["vote"][0], status, g)
    torch.cuda.synchronize()
    return dict(codes=o["codes"][0].cpu().numpy(), phase=o["phase"][0].cpu().numpy(), vote=o["vote"][0].cpu().numpy(),
                status=status.cpu().numpy(), T0=o["gate"][0].cpu().numpy(), T1=o["gate"][1].cpu().numpy(),
                G=_gate_u16(o, P.Q, P.K))


def _tabulated(P, flags):
    """Does this call take the tabulated form?  (tabulated_walk_ok of qpg_tail.hip, restated from include/qpg.h: the kept
    code that seeds the next window comes from the window's last step, at most 2 048 steps, 64 KiB of staged tables.)"""
    return (not flags & SERIAL and (P.codes_per_window - 1) // 4 == P.steps - 1 and P.Q <= 2048
            and 8 * P.steps * P.K <= 64 * 1024)


def _check_tables(got, ref_T):
    assert np.array_equal(got["T0"], ref_T[0]) and np.array_equal(got["T1"], ref_T[1])


def _check_walk(got, sol, i, guard):
    assert np.array_equal(got["codes"], sol["codes"][i])
    assert np.array_equal(got["vote"], sol["vote"][i])
    assert np.array_equal(got["phase"].view(np.uint32), sol["phase"][i].view(np.uint32))       # bit-equal
    assert got["status"].tolist() == [int(sol["status0"][i]), 0 if guard is None else guard]


def _check_gate_table(got, sol):
    """Region [2]: every (step >= 1, previous code, previous vote) outcome, and the seed's step."""
    assert np.array_equal(got["G"][1:], sol["G"][1:])
    assert got["G"][0, 0] == sol["sig"][0, 0]


def _run_case(name, mode, forms, seeds=FOUR, dedups=(1,), prefused=(False,), variant=None):
    """All combinations of `forms` (0 / SERIAL) x dedup option x plain / prefused, each seed once with guard_flags NULL and
    once holding 5.  Returns how many calls took the tabulated form."""
    from qpgesture_amd import _lib
    D = _device(name, variant)
    P = D.P
    seeds = list(seeds)
    ref_T = P.tables(mode)
    sol = W.solve(P, mode, P.seed_codes[seeds], P.seed_phases[seeds]) if P.steps <= 8 else None
    n_tab = 0
    try:
        for dedup in dedups:
            _lib.set_option(DEV, _lib.QPG_OPT_GATE_DEDUP_FROM_CHAINS, dedup)
            for form in forms:
                for pre in prefused:
                    for i, s in enumerate(seeds):
                        guard = (None, 5)[i % 2]
                        got = _match(D, mode, form | (PREFUSED if pre else 0), s, guard)
                        _check_tables(got, ref_T)
                        if sol is None:                      # steps > 8: the literal walk is the only statement
                            c, v, ph, bad = W.walk(P, mode, P.seed_codes[s], P.seed_phases[s])
                            one = dict(codes=c[None], vote=v[None], phase=ph[None], status0=[bad])
                            _check_walk(got, one, 0, guard)
                            continue
                        _check_walk(got, sol, i, guard)
                        if _tabulated(P, form):
                            n_tab += 1
                            one = dict(G=sol["G"], sig=sol["sig"][:, i:i + 1])
                            _check_gate_table(got, one)
    finally:
        _lib.set_option(DEV, _lib.QPG_OPT_GATE_DEDUP_FROM_CHAINS, 1)
    return n_tab


# ---- fusion ------------------------------------------------------------------------------------------------------------------
def _fuse_direct(pos, freq, rank, seed=0):
    """qpg_fuse_best_ranked on one table set, with a seeded injective idx table -> the kernel's T, and that idx."""
    import torch
    from qpgesture_amd import _lib
    Q, K = rank.shape
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.stack([rng.permutation(4 * K)[:K] for _ in range(Q)]).astype(np.int32)
    T = torch.full((Q, K), -9, dtype=torch.int32, device=DEV)
    _lib.call("qpg_fuse_best_ranked", DEV, _t(rank, np.int16), _t(idx, np.int32), _t(pos, np.int16), _t(freq, np.int16), Q, K, T)
    torch.cuda.synchronize()
    return T.cpu().numpy(), idx


def _fuse_want(pos, freq, rank, idx):
    return idx[np.arange(rank.shape[0])[:, None], W.fuse(pos, freq, rank)[..., 0]]


def test_fuse_best_ranked_on_the_circulant_databases():
    """16 databases x 22 rows x 512 previous codes: 15 688 tasks with an exact tie at the minimum, winners up to the last
    rank; both modalities' rows."""
    for n, (pos, freq, ra, rb) in enumerate(W.circulant_set()):
        for rank in (ra, rb):
            got, idx = _fuse_direct(pos, freq, rank, n)
            assert np.array_equal(got, _fuse_want(pos, freq, rank, idx)), n


@pytest.mark.parametrize("K", [64, 528, 1024])
def test_fuse_best_ranked_other_sizes(K):
    for swaps in (True, False):
        pos, freq, ra, rb = W.circulant_tables(K, 22, 32, 77, swaps=swaps)
        got, idx = _fuse_direct(pos, freq, ra, K)
        assert np.array_equal(got, _fuse_want(pos, freq, ra, idx))


@pytest.mark.parametrize("K", [512, 528])
@pytest.mark.parametrize("deep_first", [True, False])
def test_fuse_best_ranked_tie_on_a_round_boundary(K, deep_first):
    """Score exactly B = 64 / 128 / 192 / 448 twice: at rank B (the first rank of a scan round that starts only if
    `base > best` is false) and inside the first round; the lower code wins, whichever of the two it is."""
    pos, freq, ra, rb, planted, deep, shallow = W.boundary_tables(K, 8, deep_first, 103)
    got, idx = _fuse_direct(pos, freq, ra, 3)
    want = _fuse_want(pos, freq, ra, idx)
    assert planted.sum() >= 8 * (K // 4 - 2)
    q, p = np.nonzero(planted)
    assert np.array_equal(want[q, p], idx[q, min(deep, shallow)])
    assert np.array_equal(got, want)


def test_fuse_best_ranked_rows_that_are_no_permutation():
    """A duplicated rank, a rank outside [0, K): the kernel's documented full-scan path = the plain argmin over the values."""
    pos, freq, ra = W.nonperm_tables(512, 31)
    got, idx = _fuse_direct(pos, freq, ra, 4)
    assert np.array_equal(got, _fuse_want(pos, freq, ra, idx))


def test_fuse_best_ranked_random_control():
    pos, freq, ra, rb = W.random_tables(512, 24, 104)
    got, idx = _fuse_direct(pos, freq, ra, 5)
    assert np.array_equal(got, _fuse_want(pos, freq, ra, idx))


# ---- the walk ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ["main", "distinct"])
def test_walk_at_the_product_size(name, mode):
    """K = 512, N = 32, M = 3, steps = 8: tabulated and serial, gate dedup off and on, plain and prefused (two-modality
    mode).  `distinct` puts 1 024 keys into the dedup kernel's hash at every step and holds every planted gate case."""
    n = _run_case(name, mode, (0, SERIAL), dedups=(0, 1), prefused=(False, True) if mode == 0 else (False,))
    assert n == (16 if mode == 0 else 8)


@pytest.mark.parametrize("name", ["random", "m1", "boundary", "boundary_r", "boundary528", "k528", "k500", "k64_g64x1",
                                  "k64_s1", "k64_s3", "k64_s7", "k64_s8"])
def test_walk_other_shapes(name):
    """The control; M = 1; the boundary tables through qpg_match_steps (K = 512 and 528); K = 528 (plain gate table: K >
    512); K = 500 (fuse_best_kernel: K % 16 != 0); K = 64 with grids of 64 and 1 positions; 1, 3, 7, 8 steps a window."""
    P = W.case(name)
    for mode in (0, 1, 2):
        n = _run_case(name, mode, (0, SERIAL), seeds=FOUR[:2] if mode else FOUR,
                      prefused=(False, True) if mode == 0 and P.K % 16 == 0 else (False,))
        assert n > 0


@pytest.mark.parametrize("name", ["k64_s9", "k64_s16"])
def test_walk_more_than_eight_steps_is_serial(name):
    """9 and 16 steps: 30 of the 36 / 64 codes of a window are kept and code 29 - from the window's 8th step - seeds the next
    window, so the state is no function of the previous step's winner: both forms asked for run the serial walk."""
    for mode in (0, 1, 2):
        assert _run_case(name, mode, (0, SERIAL)) == 0


def test_walk_at_the_tabulated_limit_and_past_it():
    """M x steps = 2 048 (the chase's limit) tabulated and serial; M = 257 (2 056 steps) routes itself to the serial walk."""
    assert _run_case("q2048", 0, (0, SERIAL), seeds=(0, 5), dedups=(0, 1)) == 4
    assert _run_case("m257", 0, (0,), seeds=(0, 5)) == 0


@pytest.mark.parametrize("variant", ["unvisited", "losing"])
def test_walk_with_absent_codes(variant):
    """-1 in the idx tables: where no walk goes, status[0] stays 0; at the losing candidate of a visited state it is 1 (the
    reference project raises there) and the codes are those of the winners."""
    seeds = tuple(range(0, 64, 4))
    n = _run_case("distinct", 0, (0, SERIAL), seeds=seeds, dedups=(0, 1), variant=variant)
    assert n == 2 * len(seeds)
    P = _device("distinct", variant).P
    flagged = W.solve(P, 0, P.seed_codes[:64], P.seed_phases[:64])["status0"]
    assert flagged.any() == (variant == "losing")


# ---- the LDS limits of the walk's own launches ---------------------------------------------------------------------------------
def test_walk_at_the_largest_tables_the_header_admits():
    """K = 1 024 at 8 steps: 64 KiB of staged gate tables next to the chase's static LDS (tabulated) / of candidate tables
    next to the walk's (serial).  16 steps at K = 768: 96 KiB (serial).  The launchers raise the kernels' limit."""
    assert _run_case("k1024", 0, (0, SERIAL), seeds=FOUR[:2]) == 2
    assert _run_case("k1024", 1, (0,), seeds=FOUR[:2]) == 2
    assert _run_case("k768_s16", 0, (SERIAL,), seeds=FOUR[:2]) == 0


# ---- batch and takes ---------------------------------------------------------------------------------------------------------
def _chain_problem(P, c, M):
    rows = slice(c * M * P.steps, (c + 1) * M * P.steps)
    d = {k: v for k, v in P.__dict__.items() if k != "_tables"}
    d.update(M=M, aud_rank=P.aud_rank[rows], txt_rank=P.txt_rank[rows], aud_idx=P.aud_idx[rows], txt_idx=P.txt_idx[rows])
    return W.Problem(**d)


@pytest.mark.parametrize("stride", [2, 3])
@pytest.mark.parametrize("n_chains", [1, 2, 5])
def test_walk_batch(n_chains, stride):
    """qpg_match_steps_batch: chains of M = 2 windows back to back in the tables, each with its own seed."""
    import torch
    from qpgesture_amd import _lib
    D = _device("batch")
    P, M = D.P, 2
    Qc = M * P.steps
    seeds = [3 + 211 * c for c in range(n_chains)]
    seeds[-1] = 5                                             # (the all-zero phase block)
    refs = []
    for c in range(n_chains):
        Pc = _chain_problem(P, c, M)
        refs.append((Pc.tables(0), W.solve(Pc, 0, P.seed_codes[[seeds[c]]], P.seed_phases[[seeds[c]]])))
    rows = slice(0, n_chains * Qc)
    try:
        for dedup in (0, 1):
            _lib.set_option(DEV, _lib.QPG_OPT_GATE_DEDUP_FROM_CHAINS, dedup)
            for mode_flags in (0, PREFUSED):
                o = _outputs(P, n_chains, M, n_chains)
                status = torch.full((n_chains * stride,), -9, dtype=torch.int32, device=DEV)
                if mode_flags:
                    _prefuse(D, rows, o, n_chains * Qc)
                _lib.call("qpg_match_steps_batch", DEV, *D.head(rows, mode_flags, M), n_chains, _t(P.seed_codes[seeds], np.int32),
                          _t(P.seed_phases[seeds], np.float32), o["gate"], o["codes"], o["phase"], o["vote"], status, stride,
                          _t([5], np.int32))
                torch.cuda.synchronize()
                st = status.cpu().numpy().reshape(n_chains, stride)
                G = _gate_u16(o, n_chains * Qc, P.K)
                assert (st[:, 2:] == -9).all()
                for c, (T, sol) in enumerate(refs):
                    cr = slice(c * Qc, (c + 1) * Qc)
                    got = dict(codes=o["codes"][c].cpu().numpy(), phase=o["phase"][c].cpu().numpy(),
                               vote=o["vote"][c].cpu().numpy(), status=st[c, :2], T0=o["gate"][0][cr].cpu().numpy(),
                               T1=o["gate"][1][cr].cpu().numpy(), G=G[cr])
                    _check_tables(got, T)
                    _check_walk(got, sol, 0, 5)
                    _check_gate_table(got, sol)
    finally:
        _lib.set_option(DEV, _lib.QPG_OPT_GATE_DEDUP_FROM_CHAINS, 1)


def _takes(D, mode, n_takes, stride=2, fill=0x3C, ws=None, ws_bytes=None, o=None, status=None):
    """One qpg_match_steps_takes call.  The workspace's contents on entry are ignored by the library: it is byte-filled with
    `fill` (not zeros), or the caller hands its own `ws` (u8) and the size to state."""
    import torch
    from qpgesture_amd import _lib
    P = D.P
    o = _outputs(P, n_takes, P.M) if o is None else o
    if status is None:
        status = torch.full((n_takes * stride,), -9, dtype=torch.int32, device=DEV)
    nb = int(_lib.load().qpg_match_steps_takes_ws_bytes(n_takes, P.M, P.steps))
    if ws is None:
        ws = torch.full((max(nb, 16),), fill, dtype=torch.uint8, device=DEV)
    nb = nb if ws_bytes is None else ws_bytes
    _lib.call("qpg_match_steps_takes", DEV, *D.head(slice(0, P.Q), mode, P.M), n_takes, _t(P.seed_codes[:n_takes], np.int32),
              _t(P.seed_phases[:n_takes], np.float32), o["gate"], o["codes"], o["phase"], o["vote"], status, stride, None,
              ws, nb)
    torch.cuda.synchronize()
    return o, status.cpu().numpy().reshape(n_takes, stride)


@pytest.mark.parametrize("n_takes", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("name", ["distinct", "main"])
def test_walk_takes(name, n_takes):
    """qpg_match_steps_takes: the seeds cover every code 0 .. K - 1 and six phase blocks (one all-zero); every take against
    the chase of the reference's gate table - the walks that reach the planted gate cases are among them."""
    D = _device(name)
    P = D.P
    for mode in ((0, 1, 2) if n_takes == 1000 else (0,)):
        sol = W.solve(P, mode, P.seed_codes[:n_takes], P.seed_phases[:n_takes])
        o, st = _takes(D, mode, n_takes, stride=2 + n_takes % 2)
        assert np.array_equal(o["gate"][0].cpu().numpy(), P.tables(mode)[0])
        assert np.array_equal(o["gate"][1].cpu().numpy(), P.tables(mode)[1])
        assert np.array_equal(_gate_u16(o, P.Q, P.K)[1:], sol["G"][1:])
        assert np.array_equal(o["codes"].cpu().numpy(), sol["codes"])
        assert np.array_equal(o["vote"].cpu().numpy(), sol["vote"])
        assert np.array_equal(o["phase"].cpu().numpy().view(np.uint32), sol["phase"].view(np.uint32))
        assert np.array_equal(st[:, 0], sol["status0"]) and (st[:, 1] == 0).all() and (st[:, 2:] == -9).all()


def test_walk_takes_refuses_what_the_tabulation_cannot_do():
    """steps = 9: QPG_EUNSUP before anything is launched (the outputs stay as they were)."""
    from qpgesture_amd import _lib
    D = _device("k64_s9")
    with pytest.raises(_lib.Unsupported):
        _takes(D, 0, 4)
