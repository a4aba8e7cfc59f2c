"""The exact text sweeps (csrc/qpg_text.hip) and the edit-distance sweep (csrc/qpg_lev.hip) against NumPy (tests/text_ref.py),
every entry called directly through the C ABI: qpg_text_pack_candidates_f32 / _f16, qpg_l2_normalize_rows_f32,
qpg_text_pack_queries_f32, qpg_text_cosine_f32, qpg_text_percode_f32 / _f16, qpg_wavvq_lev_f32 (+ qpg_percode_select_f32 and
qpg_rank_rows_f32 on its matrix).  The referee is NumPy, never a kernel, and every comparison is exact: bit patterns for
distances, images and norms, equality for indices, ranks and nearest neighbours.

Outputs are pre-filled with sentinels (NaN in float arrays - the ldD > C padding columns, the padding lanes of an image's last
tile and one trailing element or row included - and -9 in integer tables): a write outside the contract fails an assertion.
What the cases are chosen for is in tests/text_ref.py; the conditions they meet are checked by
tests/test_text_contract_cpu.py.  One TEXTCONTRACT line per test with the paths entered and the wall time (pytest -s)."""
import ctypes
import time

import numpy as np
import pytest

from tests import text_ref as R

pytestmark = pytest.mark.gpu

TILES_PER_CHUNK = (1, 2, 3, 8, 1000)      # LDS-free; chunk counts that do not divide 9 or 16 tiles; one tile per wave; one chunk
IDX_BASES = (0, 5000)


# ---- device plumbing ---------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda:0")


def _to(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device=_dev())


def _m9(n, dtype):
    import torch
    return torch.full((n,), -9, dtype=dtype, device=_dev())


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


NAN_BITS = np.array([np.nan], np.float32).view(np.uint32)[0]


def _call(name, *args):
    from qpgesture_amd import _lib
    _lib.call(name, _dev(), *args)


def _sync():
    import torch
    torch.cuda.synchronize()


def _pack_and_check_f32(c):
    """qpg_text_pack_candidates_f32 on the case: live bytes are pack_f32's, padding lanes and the trailing element untouched.
    -> the device image (without the trailing element)."""
    image, live, _ = c.packed
    xt = _nan(image.size + 1)
    _call("qpg_text_pack_candidates_f32", _to(c.ctx), c.N, c.R, c.Dm, _to(c.cand_r), c.G, xt)
    _sync()
    got = _u32(xt)
    assert np.array_equal(got[:-1][live], image.view(np.uint32)[live]), c.name + ": image"
    assert (got[:-1][~live] == NAN_BITS).all() and got[-1] == NAN_BITS, c.name + ": padding lanes or the element past the image written"
    return xt[:-1]


def _normalised_queries(c):
    """qpg_l2_normalize_rows_f32 on the case's queries, held to knn_oracle.l2_normalize.  -> [dev] f32 [Q][Dm]."""
    qn = _nan(c.Q + 1, c.Dm)
    _call("qpg_l2_normalize_rows_f32", _to(c.q), c.Q, c.Dm, qn)
    _sync()
    got = _u32(qn)
    assert np.array_equal(got[:c.Q], c.qn.view(np.uint32)) and (got[c.Q] == NAN_BITS).all(), c.name + ": normalised queries"
    return qn[:c.Q]


# ---- test 1: qpg_text_pack_candidates_f32 + qpg_l2_normalize_rows_f32 + qpg_text_cosine_f32 -------------------------------
def _instantiation(Q):
    return "<12,4>" if Q > 96 else "<4,4>" if Q > 24 else "<6,4>" if Q > 8 else "<2,4>" if Q > 2 else "<1,2>"


@pytest.mark.parametrize("name", list(R.SWEEP_CASES))
def test_plain_sweep_against_numpy(name):
    t0 = time.perf_counter()
    c = R.sweep_case(name)
    want = c.D.view(np.uint32)
    xt, qn = _pack_and_check_f32(c), _normalised_queries(c)
    for pad in (0, 3):
        D = _nan(c.Q + 1, c.C + pad)
        _call("qpg_text_cosine_f32", xt, c.C, c.Dm, qn, c.Q, D, D.stride(0))
        _sync()
        got = _u32(D)
        assert np.array_equal(got[:c.Q, :c.C], want), "%s ldD = C + %d: %d of %d distances differ" % (
            name, pad, int((got[:c.Q, :c.C] != want).sum()), want.size)
        assert (got[:c.Q, c.C:] == NAN_BITS).all() and (got[c.Q] == NAN_BITS).all(), name + ": wrote outside [0:Q][0:C]"
    per = {"<12,4>": 48, "<4,4>": 16, "<6,4>": 24, "<2,4>": 8, "<1,2>": 2}[_instantiation(c.Q)]
    print("TEXTCONTRACT plain sweep %-18s text_cosine_f32_kernel%s, %d tiles x %d query blocks, nk = %d, ldD = C and C + 3: %.2f s"
          % (name, _instantiation(c.Q), (c.C + 63) // 64, (c.Q + per - 1) // per, c.Dm // 16, time.perf_counter() - t0))


def test_the_sweep_cases_enter_every_instantiation_with_a_ragged_last_group():
    """The table itself: each of the five instantiations runs with a last query group that the clamp q = Q - 1 fills, and
    with Dm = 16 (nk = 1)."""
    ragged = {}
    for p in R.SWEEP_CASES.values():
        inst = _instantiation(p["Q"])
        qb = int(inst[1:-1].split(",")[0])
        if p["Q"] % qb and p["Dm"] == 16:
            ragged[inst] = p["Q"]
    assert set(ragged) >= {"<12,4>", "<4,4>", "<6,4>", "<2,4>"}, ragged          # (<1,2> holds one query per wave: never ragged)
    assert {_instantiation(p["Q"]) for p in R.SWEEP_CASES.values() if p["Dm"] == 16} == {"<12,4>", "<4,4>", "<6,4>", "<2,4>", "<1,2>"}


# ---- test 2: qpg_text_pack_queries_f32 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 5, 63, 64, 65])
@pytest.mark.parametrize("Dm", [48, 384])
def test_query_pack_gathers_and_normalises(Q, Dm):
    """Four threads per row, 64 rows per block: Q = 63, 64, 65 put the last group before, at and behind a block's end."""
    from oracle import knn_oracle as O
    t0 = time.perf_counter()
    c = R.Case("queries", 3, 5, 5, Dm, 1, 16, seed=50 + Dm)             # (M, R) = (3, 5): zero, tiny and threshold rows included
    M, Rr = c.N, c.R
    rng = np.random.default_rng(Q)
    win = rng.integers(0, M, size=Q).astype(np.int32)
    row = rng.integers(0, Rr, size=Q).astype(np.int32)
    win[0], row[0] = M - 1, Rr - 1                                       # the last row of the last window
    planted = [divmod(i, c.G) for i in (3, 4, 5, 6)][:max(Q - 2, 0)]     # zero, tiny, below and above the threshold
    for i, (j, g) in enumerate(planted):
        win[1 + i], row[1 + i] = j, c.cand_r[g]
    if Q >= 5:
        win[-1], row[-1] = win[0], row[0]                                # repeated pairs, in two different blocks at Q = 65 ...
        win[Q // 2], row[Q // 2] = win[1], row[1]
    want = O.l2_normalize(c.ctx[win, row])
    out = _nan(Q + 1, Dm)
    _call("qpg_text_pack_queries_f32", _to(c.ctx), M, Rr, Dm, _to(win), _to(row), Q, out)
    _sync()
    got = _u32(out)
    assert np.array_equal(got[:Q], want.view(np.uint32)) and (got[Q] == NAN_BITS).all()
    print("TEXTCONTRACT query pack Q=%d Dm=%d l2_normalize_rows_kernel<gather>, %d blocks: %.2f s"
          % (Q, Dm, (Q * 4 + 255) // 256, time.perf_counter() - t0))


# ---- tests 3 and 4: the fused per-code minimum ------------------------------------------------------------------------------
def _check_tables(c, label, run):
    """run(idx_base, out_dist, out_idx, out_rank, out_nn) with and without the optional outputs, at both index bases."""
    import torch
    Q, K = c.Q, c.K
    for idx_base in IDX_BASES:
        dist, idx, rank, nn = c.tables(idx_base)
        for optional in (True, False):
            od, oi = _nan(Q * K + 1), _m9(Q * K + 1, torch.int32)
            orank = _m9(Q * K + 1, torch.int16) if optional else None
            onn = _m9(Q + 1, torch.int32) if optional else None
            run(idx_base, od, oi, orank, onn)
            _sync()
            what = "%s %s idx_base=%d optional=%s" % (c.name, label, idx_base, optional)
            gd, gi = _u32(od), oi.cpu().numpy()
            assert gd[-1] == NAN_BITS and gi[-1] == -9, what + ": wrote past a table"
            assert np.array_equal(gd[:-1].reshape(Q, K), dist.view(np.uint32)), "%s: %d of %d minima differ" % (
                what, int((gd[:-1].reshape(Q, K) != dist.view(np.uint32)).sum()), Q * K)
            assert np.array_equal(gi[:-1].reshape(Q, K), idx), what + ": winners"
            if optional:
                gr, gn = orank.cpu().numpy(), onn.cpu().numpy()
                assert gr[-1] == -9 and gn[-1] == -9, what + ": wrote past a table"
                assert np.array_equal(gr[:-1].reshape(Q, K), rank), what + ": ranks"
                assert np.array_equal(gn[:-1], nn), what + ": nearest neighbours"


def _workspace(Q, K, tiles_per_chunk, C):
    """The scratch of exactly qpg_text_percode_ws_bytes bytes inside a buffer with 8 more behind it."""
    import torch
    from qpgesture_amd import _lib
    nbytes = int(_lib.load().qpg_text_percode_ws_bytes(C, Q, K, tiles_per_chunk))
    assert nbytes == Q * K * 8
    return torch.full((nbytes + 8,), 0xAB, dtype=torch.uint8, device=_dev()), nbytes


@pytest.mark.parametrize("name", list(R.PERCODE_CASES))
def test_fused_per_code_minimum_against_numpy(name):
    t0 = time.perf_counter()
    c = R.percode_case(name)
    xt, qn = _pack_and_check_f32(c), _normalised_queries(c)
    code = _to(c.code)
    ntile = (c.C + 63) // 64
    for tpc in TILES_PER_CHUNK:
        ws, nbytes = _workspace(c.Q, c.K, tpc, c.C)

        def run(idx_base, od, oi, orank, onn):
            _call("qpg_text_percode_f32", xt, c.C, c.Dm, code, c.K, qn, c.Q, tpc, idx_base, float(R.ABSENT), ws, nbytes,
                  od, oi, orank, onn)
        _check_tables(c, "tiles_per_chunk=%d" % tpc, run)
        assert bool((ws[nbytes:] == 0xAB).all()), "%s: wrote past the workspace" % name
    print("TEXTCONTRACT fused f32 %-22s gmin<12,8,false> %d blocks (%d tiles, %d query blocks); percode<12,8> with %s chunks x %d "
          "query blocks, %d B LDS; merge with and without ranks / nn: %.2f s"
          % (name, (ntile + 7) // 8 * ((c.Q + 95) // 96) * 8, ntile, (c.Q + 95) // 96,
             "/".join(str((ntile + t - 1) // t) for t in TILES_PER_CHUNK[1:]), (c.Q + 11) // 12, 12 * c.K * 8,
             time.perf_counter() - t0))


def test_fused_per_code_minimum_of_an_empty_candidate_set():
    """C = 0, Q = 3: both organisations return QPG_OK with `absent` everywhere, idx = -1, nn = -1 (ranks: 0 .. K - 1, the
    stable ranks of equal values)."""
    import torch
    t0 = time.perf_counter()
    Q, K, Dm = 3, 7, 16
    xt, qn = _nan(64 * Dm), _to(np.random.default_rng(0).standard_normal((Q, Dm), dtype=np.float32))
    code = _to(np.zeros(1, np.int16))
    for tpc in (1, 2):
        ws, nbytes = _workspace(Q, K, tpc, 0)
        od, oi, orank, onn = _nan(Q * K + 1), _m9(Q * K + 1, torch.int32), _m9(Q * K + 1, torch.int16), _m9(Q + 1, torch.int32)
        _call("qpg_text_percode_f32", xt, 0, Dm, code, K, qn, Q, tpc, 0, float(R.ABSENT), ws, nbytes, od, oi, orank, onn)
        _sync()
        assert np.array_equal(od.cpu().numpy()[:-1], np.full(Q * K, R.ABSENT, np.float32)) and _u32(od)[-1] == NAN_BITS
        assert np.array_equal(oi.cpu().numpy(), np.r_[np.full(Q * K, -1), -9])
        assert np.array_equal(onn.cpu().numpy(), np.r_[np.full(Q, -1), -9])
        assert np.array_equal(orank.cpu().numpy(), np.r_[np.tile(np.arange(K), Q), -9])
    print("TEXTCONTRACT fused f32 C=0: no sweep launch in either organisation, fill + merge: %.2f s" % (time.perf_counter() - t0))


def test_fused_per_code_minimum_refuses_a_short_workspace():
    import torch
    c = R.percode_case("c65_q11_k7")
    image, _, _ = c.packed
    xt, qn, code = _to(image), _to(c.qn), _to(c.code)
    for tpc in (1, 2):
        ws, nbytes = _workspace(c.Q, c.K, tpc, c.C)
        od, oi = _nan(c.Q * c.K), _m9(c.Q * c.K, torch.int32)
        with pytest.raises(RuntimeError, match="workspace too small"):
            _call("qpg_text_percode_f32", xt, c.C, c.Dm, code, c.K, qn, c.Q, tpc, 0, float(R.ABSENT), ws, nbytes - 1, od, oi,
                  None, None)
        _sync()
        assert bool((ws == 0xAB).all()) and bool(torch.isnan(od).all()) and bool((oi == -9).all())      # nothing ran


@pytest.mark.parametrize("name", list(R.HALF_CASES))
def test_f16_storage_pack_and_fused_minimum_against_numpy(name):
    import torch
    t0 = time.perf_counter()
    c = R.percode_case(name, True)
    image, live, nrm, _ = c.packed
    xh = torch.full((image.size + 8,), -1, dtype=torch.int16, device=_dev())            # 0xFFFF: an f16 NaN in every slot
    dn = _nan(c.C + 1)
    _call("qpg_text_pack_candidates_f16", _to(c.ctx), c.N, c.R, c.Dm, _to(c.cand_r), c.G, xh, dn)
    _sync()
    got = xh.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:-8][live], image.view(np.uint16)[live]), name + ": f16 image"
    assert (got[:-8][~live] == 0xFFFF).all() and (got[-8:] == 0xFFFF).all(), name + ": padding lanes or bytes past the image written"
    assert np.array_equal(_u32(dn)[:-1], nrm.view(np.uint32)) and _u32(dn)[-1] == NAN_BITS, name + ": norms of the rounded rows"
    qn, code = _normalised_queries(c), _to(c.code)
    ws, nbytes = _workspace(c.Q, c.K, 1, c.C)

    def run(idx_base, od, oi, orank, onn):
        _call("qpg_text_percode_f16", xh, dn, c.C, c.Dm, code, c.K, qn, c.Q, idx_base, float(R.ABSENT), ws, nbytes, od, oi,
              orank, onn)
    _check_tables(c, "f16", run)
    assert bool((ws[nbytes:] == 0xAB).all())
    ntile = (c.C + 63) // 64
    print("TEXTCONTRACT fused f16 %-22s text_pack_candidates_h_kernel %d blocks; gmin<12,8,true> %d blocks (%d tiles, %d query "
          "blocks); merge with and without ranks / nn: %.2f s"
          % (name, (c.C * 4 + 255) // 256, (ntile + 7) // 8 * ((c.Q + 95) // 96) * 8, ntile, (c.Q + 95) // 96,
             time.perf_counter() - t0))


# ---- test 5: qpg_wavvq_lev_f32 ----------------------------------------------------------------------------------------------
def _lev_call(c, taps, D):
    host_taps = (ctypes.c_int32 * len(taps))(*taps)
    _call("qpg_wavvq_lev_f32", _to(c.sym_db), c.N, c.T, _to(c.cand_t), c.G, host_taps, len(taps), _to(c.sym_q), c.Mq, c.T,
          _to(c.q_win), _to(c.q_t), c.Q, D, D.stride(0))


@pytest.mark.parametrize("name", list(R.LEV_CASES))
def test_edit_distance_sweep_and_its_tables_against_numpy(name):
    import torch
    from tests import select_ref as S
    t0 = time.perf_counter()
    c = R.lev_case(name)
    Q, C, K = c.Q, c.C, c.K
    D = _nan(Q + 1, C + 3)
    _lev_call(c, c.taps, D)
    _sync()
    got = _u32(D)
    assert np.array_equal(got[:Q, :C], c.D.view(np.uint32)), "%s: %d of %d distances differ" % (
        name, int((got[:Q, :C] != c.D.view(np.uint32)).sum()), Q * C)
    assert (got[:Q, C:] == NAN_BITS).all() and (got[Q] == NAN_BITS).all(), name + ": wrote outside [0:Q][0:C]"
    dist, idx, rank = S.tables(c.D, c.code, K, R.ABSENT)
    od, oi, orank = _nan(Q * K + 1), _m9(Q * K + 1, torch.int32), _m9(Q * K + 1, torch.int16)
    _call("qpg_percode_select_f32", D, D.stride(0), Q, _to(c.code), C, K, float(R.ABSENT), 0, od, oi, orank, 0, 0)
    orank2 = _m9(Q * K + 1, torch.int16)
    _call("qpg_rank_rows_f32", od, Q, K, orank2)
    _sync()
    assert np.array_equal(_u32(od)[:-1].reshape(Q, K), dist.view(np.uint32)) and _u32(od)[-1] == NAN_BITS, name + ": minima"
    assert np.array_equal(oi.cpu().numpy(), np.r_[idx.reshape(-1), -9]), name + ": first-wins winners among equal integers"
    for r in (orank, orank2):
        assert np.array_equal(r.cpu().numpy(), np.r_[rank.reshape(-1), -9]), name + ": stable ranks of tied minima"
    print("TEXTCONTRACT edit distance %-10s wavvq_lev_kernel %d launch(es) x %d blocks, last chunk %d queries; select + ranks: %.2f s"
          % (name, (Q + 1023) // 1024, (C + 255) // 256, (Q - 1) % 1024 + 1, time.perf_counter() - t0))


@pytest.mark.parametrize("n_taps", [10, 12, 6])
def test_edit_distance_sweep_refuses_other_string_lengths(n_taps):
    from qpgesture_amd import _lib
    c = R.lev_case("c1_q1")
    D = _nan(c.Q + 1, c.C + 3)
    taps = (c.taps + [7])[:n_taps]
    with pytest.raises(_lib.Unsupported, match="11-symbol"):
        _lev_call(c, taps, D)
    _sync()
    assert (_u32(D) == NAN_BITS).all()
