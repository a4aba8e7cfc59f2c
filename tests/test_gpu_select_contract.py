"""What the bounded selects must return for ANY admissible input (the contract of include/qpg.h, stated in
tests/select_ref.py): they are handed the exact distances plus worst-case error of full width E - not the benign, nearly
zero-mean error the real sweeps produce, which sits several times inside the bound and hardly touches the band - and must
return the tables of the exact arithmetic.
  audio  qpg_percode_select_mixed_f64 (workspace form and one-launch form, f32 and f64 matrix, f32 and f16 track), its
         walk-relevance cut and the three-call cross-shard merge: winners = per-code argmin of the exact f64 distances
         (lowest index among equals), ranks = their stable ranks, distances within 1e-13 where something was re-evaluated
         and within E elsewhere, stats[1] == 0;
  text   qpg_percode_select_sorted_f32 (prefilter matrix / tile masks) and qpg_percode_select_bycode_f32: the exact sweep's
         tables bit for bit.
Every case's conditions (tests/select_ref.py: admissible) are checked on the CPU by tests/test_select_contract_cpu.py; two
negative controls show that the noise bites: a band of 1.05 E must give a wrong table.  Lines starting with CONTRACT carry
the measured list counts (profiles/select_contract.md)."""
import functools

import numpy as np
import pytest

from tests import select_ref as R
from tests.helpers import merge_mixed_by_hand
from tests.prefilter_ref import mask_rule

pytestmark = pytest.mark.gpu

T, G = R.T_AUD, R.G_AUD


def _case(name):
    if name == "product_band":
        from qpgesture_amd.code_knn import AUDIO_HL_BAND, AUDIO_HL_ERR
        return R.product_case(AUDIO_HL_ERR, AUDIO_HL_BAND)
    return R.audio_case(name)


@functools.lru_cache(maxsize=None)
def _operands(name, lo=0, hi=None):
    """The select's operands of windows [lo, hi) of a case on the device (a row shard, or the whole database)."""
    import torch
    c = _case(name)
    hi = c.N if hi is None else hi
    dev = torch.device("cuda:0")
    base = torch.from_numpy(np.ascontiguousarray((c.base16 if c.half else c.base)[lo:hi])).to(dev)
    return dict(dev=dev, base=base, half=int(c.half), cand_t=torch.from_numpy(c.cand_t).to(dev),
                q32=torch.from_numpy(c.q32).to(dev), qn2=torch.from_numpy(c.qn2).to(dev),
                cn2=torch.from_numpy(np.ascontiguousarray(c.cn2[lo * G:hi * G])).to(dev),
                code=torch.from_numpy(np.ascontiguousarray(c.cand_code[lo * G:hi * G])).to(dev), C=(hi - lo) * G)


@functools.lru_cache(maxsize=None)
def _workspace(K):
    """ONE workspace per K, zero-filled once, sized for the largest Q of the table and reused by every case of that K."""
    import torch
    from qpgesture_amd import _lib
    cases = [_case(n) for n in list(R.AUDIO_CASES) + ["product_band"]]
    Qmax = max(c.Q for c in cases if c.K == K)
    return torch.zeros((int(_lib.load().qpg_percode_select_mixed_ws_bytes(Qmax, K)),), dtype=torch.uint8, device="cuda:0")


def _mixed(name, D_in, eps1, eps2, use_ws, lo=0, hi=None, ld_pad=0, idx_base=0, out=None, cut=None, ranks=True, ws=None, rank_out=None):
    """One call of the mixed select (or its cut form) on D_in [Q][C] (f32 or f64; NaN in the ld_pad padding columns).
    ws: the caller's own workspace (u8, zero-filled once) instead of the shared one of _workspace(K).
    -> dist, idx, rank (numpy), stats [4], tier-1 list length per query (workspace form; else None)."""
    import torch
    from qpgesture_amd import _lib
    c, o = _case(name), _operands(name, lo, hi)
    dev, Q, K, C = o["dev"], D_in.shape[0], c.K, o["C"]
    assert D_in.shape == (Q, C)
    D = torch.full((Q, C + ld_pad), float("nan"), dtype=torch.float32 if D_in.dtype == np.float32 else torch.float64, device=dev)
    D[:, :C] = torch.from_numpy(D_in).to(dev)
    if out is None:
        dist = torch.full((Q, K), float("nan"), dtype=torch.float64, device=dev)
        idx = torch.full((Q, K), -7, dtype=torch.int32, device=dev)
    else:
        dist, idx = out
    rank = (torch.full((Q, K), -7, dtype=torch.int16, device=dev) if rank_out is None else rank_out) if ranks else None
    stats = torch.zeros((4,), dtype=torch.int32, device=dev)
    ws = (_workspace(K) if ws is None else ws) if use_ws else None
    args = [D, int(D_in.dtype == np.float32), D.stride(0), Q, o["code"], C, K, R.ABSENT, idx_base, dist, idx, rank, 0, 0,
            o["base"], T, c.F, o["cand_t"], G, R.N_TAPS, R.TAP_STRIDE, o["q32"][:Q], o["qn2"][:Q], o["cn2"], float(eps1),
            float(eps2), stats, ws, ws.numel() if use_ws else 0, o["half"]]
    if cut is None:
        _lib.call("qpg_percode_select_mixed_f64", dev, *args)
    else:
        _lib.call("qpg_percode_select_mixed_f64_cut", dev, *args, cut["pos_t"], cut["freq"], cut["top_n"], 0)
    torch.cuda.synchronize()
    n1 = None
    if use_ws:
        stride = int(_lib.load().qpg_percode_select_mixed_ws_stride(K))
        n1 = ws.view(torch.int32)[torch.arange(Q, device=dev) * (stride // 4) + 6 * K].cpu().numpy()   # i32 at q stride + 24 K
    return (dist.cpu().numpy(), idx.cpu().numpy(), None if rank is None else rank.cpu().numpy().astype(np.int64),
            stats.cpu().numpy(), n1)


def _must_refine(D_in, code, K, eps1, ranks=True):
    """What the header makes the select re-evaluate, from the matrix it is given: codes with two or more candidates within
    eps1 of their minimum and - when ranks are asked for - codes whose minimum is within eps1 of a rank neighbour's.
    -> bool [Q][K], listed pairs per query, the approximate minima."""
    D = np.asarray(D_in, np.float64)
    m, mi, _ = R.tables(D, code, K, R.ABSENT)
    code = np.asarray(code).astype(np.int64)
    valid = (code >= 0) & (code < K)
    inband = valid[None] & (D <= m[:, np.where(valid, code, 0)] + eps1)
    cnt = np.stack([np.bincount(code[inband[q]], minlength=K) for q in range(D.shape[0])])
    must = cnt >= 2
    pairs = np.where(must, cnt, 0).sum(axis=1)
    if not ranks:
        return must, pairs, m
    order = np.argsort(np.where(mi >= 0, m, np.inf), axis=1, kind="stable")
    rows = np.arange(D.shape[0])[:, None]
    a, b = order[:, :-1], order[:, 1:]
    close = (mi[rows, a] >= 0) & (mi[rows, b] >= 0) & (m[rows, b] - m[rows, a] < eps1)
    nb = np.zeros_like(must)
    nb[np.broadcast_to(rows, a.shape)[close], a[close]] = True
    nb[np.broadcast_to(rows, b.shape)[close], b[close]] = True
    return must | nb, pairs + (nb & ~must).sum(axis=1), m


def _check_tables(c, got, D_in, eps1, idx_base=0, ref=None, code=None):
    """The contract on one result: winners, ranks, distances, stats[1]."""
    dist, idx, rank, stats, n1 = got
    rd, ri, rr = c.ref if ref is None else ref
    code = c.cand_code if code is None else code
    Q = dist.shape[0]
    assert stats[1] == 0
    assert np.array_equal(idx, np.where(ri[:Q] >= 0, ri[:Q] + idx_base, -1))
    if rank is not None:
        assert np.array_equal(rank, rr[:Q])
    present = ri[:Q] >= 0
    assert np.array_equal(dist[~present], np.full((~present).sum(), R.ABSENT))
    must, pairs, approx = _must_refine(D_in, code, c.K, eps1, ranks=rank is not None)
    err = np.abs(dist - rd[:Q])
    assert err[present & must].max(initial=0.0) <= 1e-13          # re-evaluated: the f64 table's own bar (helpers.aud_tol)
    rest = present & ~must
    assert ((err <= 1e-13) | (dist == approx))[rest].all()        # elsewhere: the value it was given (or a re-evaluated one)
    assert err[present].max(initial=0.0) <= c.E                   # ... which is within E
    assert stats[2] >= pairs.sum()                                # everything the band holds was evaluated
    if n1 is not None:
        assert n1.sum() == stats[2] and (n1 >= pairs).all() and n1.max() <= R.MIX_LIST
    return pairs


def _both_forms(name, D_in, eps1, eps2, **kw):
    a = _mixed(name, D_in, eps1, eps2, True, **kw)
    b = _mixed(name, D_in, eps1, eps2, False, **kw)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)                   # workspace form == one launch, bit for bit
    assert np.array_equal(a[3], b[3])
    return a


@pytest.mark.parametrize("d_is_f32", [1, 0])
@pytest.mark.parametrize("noise", R.NOISES)
@pytest.mark.parametrize("name", list(R.AUDIO_CASES) + ["product_band"])
def test_mixed_select_returns_the_exact_tables(name, noise, d_is_f32):
    """Every shape of the table (the base case; N = 37 / Q = 5 / K = 7; one window under K = 512; Q = 200 under K = 512; the
    f16 track, whose reference is computed on the widened values; F = 1024, where tier 1 stages the query in LDS; the
    product's own E and band on the crowded database) x every noise pattern x both matrix types x both launch forms."""
    c = _case(name)
    D_in = R.noisy(noise, c.exact, c.cand_code, c.K, c.E, np.float32 if d_is_f32 else np.float64, seed=5)
    got = _both_forms(name, D_in, c.eps1, c.eps2)
    pairs = _check_tables(c, got, D_in, c.eps1)
    print("CONTRACT mixed %s %s %s: E=%.3g eps1=%.3g bound<=%d/query; must-list %.1f/query; tier-1 %.1f/query (max %d), tier-2 %d"
          % (name, noise, "f32" if d_is_f32 else "f64", c.E, c.eps1, c.verdict["listed_max"], pairs.mean(),
             got[3][2] / c.Q, got[4].max(), got[3][0]))


@pytest.mark.parametrize("d_is_f32", [1, 0])
@pytest.mark.parametrize("ld_pad,idx_base", [(3, 1000), (8, 0), (5, 26 * 7)])
def test_mixed_select_row_stride_and_index_base(ld_pad, idx_base, d_is_f32):
    """ldD > C with NaN in the padding columns (3 / 5: rows that are not 16-byte aligned - the scalar streaming path) and a
    non-zero idx_base; a smaller Q than the workspace was sized for."""
    c = _case("base")
    D_in = R.noisy("swap", c.exact, c.cand_code, c.K, c.E, np.float32 if d_is_f32 else np.float64)
    for Q in (c.Q, 7):
        got = _both_forms("base", D_in[:Q], c.eps1, c.eps2, ld_pad=ld_pad, idx_base=idx_base)
        _check_tables(c, got, D_in[:Q], c.eps1, idx_base=idx_base)


def test_mixed_select_negative_control_a_band_of_1_05_E_is_too_narrow():
    """The same swap input with eps1 = 1.05 E: pairs with an exact gap below 0.95 E arrive more than the band apart in
    reversed order (tests/test_select_contract_cpu.py asserts they exist), so a winner or a rank must come out wrong - the
    noise bites, and a select whose band were too narrow would be caught."""
    c = _case("base")
    same, nb = R.has_gap_below(c.exact, c.cand_code, c.K, 0.95 * c.E)
    assert same >= 1 or nb >= 1
    D_in = R.noisy("swap", c.exact, c.cand_code, c.K, c.E, np.float32)
    for use_ws in (True, False):
        dist, idx, rank, stats, _ = _mixed("base", D_in, 1.05 * c.E, c.eps2, use_ws)
        wrong_idx, wrong_rank = int((idx != c.ref[1]).sum()), int((rank != c.ref[2]).sum())
        print("CONTRACT negative control (audio, eps1 = 1.05 E, ws=%s): %d wrong winners, %d wrong ranks" % (use_ws, wrong_idx, wrong_rank))
        assert wrong_idx + wrong_rank >= 1


@functools.lru_cache(maxsize=None)
def _cut_tables(K):
    """pos_rank (qpg_l2_table_f32 + qpg_rank_rows_f32 of a seeded signature table), its transpose and freq_rank."""
    import torch
    from qpgesture_amd import _lib
    dev = torch.device("cuda:0")
    sig, freq = R.signature_tables(K)
    sd = torch.from_numpy(sig).to(dev)
    tab = torch.empty((K, K), dtype=torch.float32, device=dev)
    _lib.call("qpg_l2_table_f32", dev, sd, K, sig.shape[1], tab)
    pos = torch.empty((K, K), dtype=torch.int16, device=dev)
    _lib.call("qpg_rank_rows_f32", dev, tab, K, K, pos)
    torch.cuda.synchronize()
    return dict(pos=pos, pos_t=pos.t().contiguous(), freq=torch.from_numpy(freq).to(dev), pos_np=pos.cpu().numpy(), freq_np=freq)


@pytest.mark.parametrize("top_n", [1, 2])
@pytest.mark.parametrize("noise", R.NOISES)
@pytest.mark.parametrize("name", ["base", "wide"])
def test_cut_select_agrees_on_everything_the_walk_reads(name, noise, top_n):
    """qpg_percode_select_mixed_f64_cut leaves codes the walk can never read unsettled.  top_n = 1: qpg_fuse_best_ranked on
    its tables == the NumPy fusion on the reference tables; top_n = 2: the two best codes per previous code, and their
    winners, agree; whatever it leaves approximate is within E."""
    import torch
    from qpgesture_amd import _lib
    c = _case(name)
    ct = _cut_tables(c.K)
    D_in = R.noisy(noise, c.exact, c.cand_code, c.K, c.E, np.float32, seed=6)
    dist, idx, rank, stats, n1 = _mixed(name, D_in, c.eps1, c.eps2, True, cut=dict(pos_t=ct["pos_t"], freq=ct["freq"], top_n=top_n))
    rd, ri, rr = c.ref
    assert stats[1] == 0
    assert sorted(rank[0].tolist()) == list(range(c.K))                              # still a permutation per row
    present = ri >= 0
    assert np.abs(dist - rd)[present].max() <= c.E and np.array_equal(idx >= 0, present)
    want = R.fuse_best(ct["pos_np"], ct["freq_np"], rr, top_n)                       # [Q][K][top_n] codes
    got = R.fuse_best(ct["pos_np"], ct["freq_np"], rank, top_n)
    assert np.array_equal(got, want)
    rows = np.arange(c.Q)[:, None, None]
    assert np.array_equal(idx[rows, want], ri[rows, want])                           # ... and their winners
    read = np.zeros_like(present)
    read[np.broadcast_to(rows, want.shape), want] = True
    assert np.array_equal(rank[read], rr[read])
    if top_n == 1:
        dev = ct["pos"].device
        Tt = torch.empty((c.Q, c.K), dtype=torch.int32, device=dev)
        _lib.call("qpg_fuse_best_ranked", dev, torch.from_numpy(rank.astype(np.int16)).to(dev),
                  torch.from_numpy(idx).to(dev), ct["pos"], ct["freq"], c.Q, c.K, Tt)
        torch.cuda.synchronize()
        assert np.array_equal(Tt.cpu().numpy(), ri[rows[:, :, 0], want[:, :, 0]])
    full = _mixed(name, D_in, c.eps1, c.eps2, True)
    print("CONTRACT cut %s %s top_n=%d: tier-1 %.1f/query with the cut, %.1f without; %d of %d entries differ from the full select's"
          % (name, noise, top_n, stats[2] / c.Q, full[3][2] / c.Q, int((rank != full[2]).sum() + (idx != full[1]).sum()), 2 * idx.size))


@pytest.mark.parametrize("noise", ["rademacher", "swap", "one_sided"])
@pytest.mark.parametrize("W", [2, 3])
def test_cross_shard_merge_returns_the_exact_tables(W, noise):
    """W row shards of the base case, each with its own adversarial matrix (independent noise) through the mixed select
    (no ranks: they are taken after the merge), then phase 1 / shard refine / phase 2 with the exchanges by hand.  The exact
    copies of window 1 sit in windows 5 and 40: contenders of one code straddle the shard boundary for W = 2 and 3 (window
    20 = window 2 with its own codes: equal minima from two shards).  The merged winners and ranks are the reference's over
    the whole database; phase 2 runs with eps2 = 0 - bit-identical rows give bit-identical responses and fall back to the
    index - so no trouble bit is raised."""
    import torch
    c = _case("base")
    dev = torch.device("cuda:0")
    Q, K = c.Q, c.K
    bounds = [round(w * c.N / W) for w in range(W + 1)]
    src_stride = Q * K * 12
    recv = torch.zeros((W * src_stride,), dtype=torch.uint8, device=dev)
    shards, t1 = [], 0
    for w in range(W):
        lo, hi = bounds[w], bounds[w + 1]
        code = c.cand_code[lo * G:hi * G]
        ex = np.ascontiguousarray(c.exact[:, lo * G:hi * G])
        D_in = R.noisy(noise, ex, code, K, c.E, np.float32, seed=100 + w)
        blk = recv[w * src_stride:(w + 1) * src_stride]
        out = (blk[:Q * K * 8].view(torch.float64).view(Q, K), blk[Q * K * 8:].view(torch.int32).view(Q, K))
        got = _mixed("base", D_in, c.eps1, c.eps2, True, lo=lo, hi=hi, idx_base=lo * G, out=out, ranks=False)
        ref_w = R.tables(ex, code, K, R.ABSENT)
        _check_tables(c, got, D_in, c.eps1, idx_base=lo * G, ref=ref_w, code=code)       # the shard's own table
        t1 += int(got[3][2])
        o = _operands("base", lo, hi)
        shards.append(dict(cand_base=lo * G, base=o["base"], base_is_f16=o["half"], T=T, F=c.F, cand_t=o["cand_t"], G=G,
                           tap_stride=R.TAP_STRIDE, q32=o["q32"], qn2=o["qn2"], cn2=o["cn2"]))
    assert 5 < bounds[1] <= 40 and (c.cand_code[1 * G:2 * G] >= 0).any()                 # windows 1, 5 | ... | window 40
    d, ix, rk, st, counts = merge_mixed_by_hand(recv, W, src_stride, 0, Q * K * 8, Q, K, c.eps1, 0.0, shards,
                                                R=Q * K, fl_cap=K * W)
    rd, ri, rr = c.ref
    print("CONTRACT merge W=%d %s: shard tier-1 %.1f/query; requests per shard %s; cross-shard re-evaluations %d; flags %d"
          % (W, noise, t1 / Q, counts, int(st[3]), int(st[1])))
    assert st[1] == 0 and min(counts) > 0 and st[3] == sum(counts)
    assert np.array_equal(ix.cpu().numpy(), ri)
    assert np.array_equal(rk.cpu().numpy().astype(np.int64), rr)
    assert np.abs(d.cpu().numpy() - rd)[ri >= 0].max() <= c.E


def _f64_select(name, which, D, q_block=0, block_stride=0, out=None, ranks=True, ws=None, ws_bytes=None, rank_out=None):
    """qpg_percode_select_guarded_f64 / _exact_f64 on the f64 matrix D (device) with eps = 1e-12.  Plain tables are prefilled
    with sentinels; `out` = (dist, idx) views of an exchange buffer.  -> dist, idx, rank (device tensors), stats (numpy)."""
    import torch
    from qpgesture_amd import _lib
    c, o = _case(name), _operands(name)
    dev, Q, K, C = o["dev"], c.Q, c.K, o["C"]
    if out is None:
        out = (torch.full((Q, K), float("nan"), dtype=torch.float64, device=dev), torch.full((Q, K), -7, dtype=torch.int32, device=dev))
    rank = (torch.full((Q, K), -7, dtype=torch.int16, device=dev) if rank_out is None else rank_out) if ranks else None
    stats = torch.zeros((4,), dtype=torch.int32, device=dev)
    args = [D, D.stride(0), Q, o["code"], C, K, R.ABSENT, 0, out[0], out[1], rank, q_block, block_stride, o["base"], T, c.F,
            o["cand_t"], G, R.N_TAPS, R.TAP_STRIDE, o["q32"], 1e-12, stats, o["half"]]
    if which == "exact":
        if ws is None:
            ws = torch.empty((int(_lib.load().qpg_percode_select_exact_ws_bytes(Q, C, K)),), dtype=torch.uint8, device=dev)
        args += [ws, ws.numel() if ws_bytes is None else ws_bytes]
    _lib.call("qpg_percode_select_%s_f64" % which, dev, *args)
    torch.cuda.synchronize()
    return out[0], out[1], rank, stats.cpu().numpy()


@pytest.mark.parametrize("name", ["odd", "base", "f16_track", "wavlm_width"])
def test_guarded_and_exact_selects_settle_ties_like_the_reference(name):
    """The f64 selects on the exact distances themselves, called directly.  The cases hold bit-identical candidate rows
    inside one code, in two codes and in an all-zero window, so both guard levels (candidates of a code, minima of rank
    neighbours) fire; tests/test_select_contract_cpu.py checks that nothing else that matters lies inside the band.  Both
    must return the reference's winners and ranks, distances within 1e-13, the same tables bit for bit, no overflow - and
    for `base` the same rows in the exchange layout (16 queries per block, 64 bytes of padding between blocks)."""
    import torch
    c = _case(name)
    D = torch.from_numpy(c.exact).to("cuda:0")
    rd, ri, rr = c.ref
    present = ri >= 0
    got = {}
    for which in ("guarded", "exact"):
        dist, idx, rank, stats = _f64_select(name, which, D)
        got[which] = dist, idx, rank
        d = dist.cpu().numpy()
        print("CONTRACT %s %s: %d pairs re-evaluated, worst distance error %.3g" % (which, name, stats[0], np.abs(d - rd)[present].max()))
        assert np.array_equal(idx.cpu().numpy(), ri)
        assert np.array_equal(rank.cpu().numpy().astype(np.int64), rr)
        assert np.abs(d - rd)[present].max() <= 1e-13
        assert np.array_equal(d[~present], np.full((~present).sum(), R.ABSENT))
        assert stats[1] == 0 and stats[0] > 0
    for a, b in zip(got["guarded"], got["exact"]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    if name != "base":
        return
    qb, K = 16, c.K
    blk = qb * K * 12                                        # a block: dist f64 [qb][K] | idx i32 [qb][K] | 64 bytes of padding
    for which in ("guarded", "exact"):
        # (without a rank output the rank-level guard does not run, so the minima it would have re-evaluated keep the values
        # they were given: the rows are those of the plain layout WITHOUT ranks - same winners, distances within 1e-13)
        pd, pi, _, pstats = _f64_select(name, which, D, ranks=False)
        assert torch.equal(pi, got[which][1]) and np.abs(pd.cpu().numpy() - rd)[present].max() <= 1e-13
        buf = torch.full(((c.Q // qb) * (blk + 64),), 0x5A, dtype=torch.uint8, device="cuda:0")
        out = (buf[:qb * K * 8].view(torch.float64), buf[qb * K * 8:blk].view(torch.int32))
        _, _, _, stats = _f64_select(name, which, D, q_block=qb, block_stride=blk + 64, out=out, ranks=False)
        assert stats[1] == 0 and stats[0] > 0 and stats[0] == pstats[0]
        blocks = buf.view(c.Q // qb, blk + 64)
        assert torch.equal(blocks[:, :qb * K * 8].contiguous().view(-1), pd.view(torch.uint8).view(-1))
        assert torch.equal(blocks[:, qb * K * 8:blk].contiguous().view(-1), pi.view(torch.uint8).view(-1))
        assert bool((blocks[:, blk:] == 0x5A).all())


# ---- text ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _text_device():
    """The text case on the device: SortedRows of the library-normalised rows (== the oracle's, bit for bit), whose layout
    must be the one tests/select_ref.py states; the exact sweep's tables must be the NumPy reference's."""
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.sorted_rows import SortedRows
    t = R.text_case()
    dev = torch.device("cuda:0")
    Xd = torch.from_numpy(t.X).to(dev)
    xn = torch.empty_like(Xd)
    _lib.call("qpg_l2_normalize_rows_f32", dev, Xd, t.n, t.D, xn)
    qd = torch.from_numpy(t.q).to(dev)
    qn = torch.empty_like(qd)
    _lib.call("qpg_l2_normalize_rows_f32", dev, qd, t.Q, t.D, qn)
    assert np.array_equal(xn.cpu().numpy().view(np.uint32), t.xn.view(np.uint32))
    assert np.array_equal(qn.cpu().numpy().view(np.uint32), t.qn.view(np.uint32))
    sr = SortedRows(xn, torch.from_numpy(t.codes_masked).to(dev), t.K, dev)
    row_index, src, seg, zero_row = t.layout
    assert sr.R == len(src) and np.array_equal(sr.row_index.cpu().numpy(), row_index)
    assert np.array_equal(sr.zero_row.cpu().numpy(), zero_row)
    live = src >= 0
    assert np.array_equal(sr.xs[:sr.R].cpu().numpy()[live], t.xn[src[live]])
    assert np.array_equal(sr.row_code.cpu().numpy()[live] & 0x1fff, seg[live])
    qperm = torch.empty_like(qn)
    _lib.call("qpg_perm32_rows_f32", dev, qn, t.Q, t.D, qperm)
    # the exact sweep (qpg_text_cosine_f32 + qpg_percode_select_f32) == the NumPy reference, bit for bit
    xt = torch.zeros((((t.n + 63) // 64) * 64 * t.D,), dtype=torch.float32, device=dev)
    _lib.call("qpg_text_pack_candidates_f32", dev, Xd.view(t.n, 1, t.D), t.n, 1, t.D, torch.zeros((1,), dtype=torch.int32, device=dev), 1, xt)
    Dx = torch.empty((t.Q, t.n), dtype=torch.float32, device=dev)
    _lib.call("qpg_text_cosine_f32", dev, xt, t.n, t.D, qn, t.Q, Dx, Dx.stride(0))
    ed = torch.empty((t.Q, t.K), dtype=torch.float32, device=dev)
    ei = torch.empty((t.Q, t.K), dtype=torch.int32, device=dev)
    er = torch.empty((t.Q, t.K), dtype=torch.int16, device=dev)
    _lib.call("qpg_percode_select_f32", dev, Dx, Dx.stride(0), t.Q, torch.from_numpy(t.codes_masked.astype(np.int16)).to(dev),
              t.n, t.K, float(R.ABSENT), 0, ed, ei, er, 0, 0)
    torch.cuda.synchronize()
    assert np.array_equal(Dx.cpu().numpy(), t.d_sk)
    rd, ri, rr, rn = t.ref
    assert np.array_equal(ed.cpu().numpy(), rd) and np.array_equal(ei.cpu().numpy(), ri) and np.array_equal(er.cpu().numpy(), rr)
    return dict(dev=dev, sr=sr, qn=qn, qperm=qperm)


def _text_select(form, Dm_in, band, Q, idx_base=0):
    """One of the three ways to feed Dm_in [Q][R]: 'matrix' (Dm + tile minima), 'masks' (tile minima + row masks, Dm = NULL),
    'bycode' (tile-major minima / masks, chain-permuted operands).  -> dist, idx, rank, nn, stats, listed rows."""
    import torch
    from qpgesture_amd import _lib
    t, o = R.text_case(), _text_device()
    dev, sr = o["dev"], o["sr"]
    Rr, nt = sr.R, sr.R // 16
    Dm_in = np.ascontiguousarray(Dm_in[:Q])
    tiles = Dm_in.reshape(Q, nt, 16)
    tmin = tiles.min(axis=2)
    # the GEMMs' rule (tests/prefilter_ref.py, held against the kernels by tests/test_gpu_prefilter_contract.py): bit r iff
    # Dm[r] <= tile minimum + f32(band), in f32
    mask = mask_rule(Dm_in, band)
    # what the select's rule lists from these inputs (by-query / by-code forms agree): opened tiles' rows, padding never
    seg = t.layout[2]
    cmin = np.full((Q, t.K), np.inf, np.float32)
    np.minimum.at(cmin, (np.arange(Q)[:, None], np.where(seg[::16] >= 0, seg[::16], 0)[None, :]), np.where(seg[::16] >= 0, tmin, np.inf))
    zr = t.layout[3] >= 0
    cmin[:, zr] = np.minimum(cmin[:, zr], np.float32(0.5))
    opened = (seg[::16] >= 0)[None] & (tmin <= cmin[:, np.where(seg[::16] >= 0, seg[::16], 0)] + np.float32(band))
    real = (t.layout[0] >= 0).reshape(nt, 16)
    if form == "matrix":
        inrow = tiles <= (cmin[:, np.where(seg >= 0, seg, 0)].reshape(Q, nt, 16) + np.float32(band))
    else:
        inrow = ((mask[:, :, None] >> np.arange(16, dtype=np.uint16)) & 1).astype(bool)
    listed = int((opened[:, :, None] & inrow & real[None]).sum())
    dist = torch.full((Q, t.K), float("nan"), dtype=torch.float32, device=dev)
    idx = torch.full((Q, t.K), -7, dtype=torch.int32, device=dev)
    rank = torch.full((Q, t.K), -7, dtype=torch.int16, device=dev)
    nn = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    stats = torch.zeros((4,), dtype=torch.int32, device=dev)
    qn, qperm = o["qn"][:Q].contiguous(), o["qperm"][:Q].contiguous()
    if form == "bycode":
        ldq = (Q + 15) // 16 * 16
        tmin_t = torch.full((nt, ldq), float("inf"), dtype=torch.float32, device=dev)
        tmin_t[:, :Q] = torch.from_numpy(np.ascontiguousarray(tmin.T)).to(dev)
        mask_t = torch.zeros((nt, ldq), dtype=torch.int16, device=dev)
        mask_t[:, :Q] = torch.from_numpy(np.ascontiguousarray(mask.T).view(np.int16)).to(dev)
        _lib.call("qpg_percode_select_bycode_f32", dev, tmin_t, mask_t, ldq, Q, Rr, sr.row_code, sr.row_index, sr.zero_row,
                  sr.code_tile, t.K, float(band), qperm, sr.xs_perm(), t.D, float(R.ABSENT), dist, idx, rank, nn, stats, idx_base)
    else:
        Dm = torch.from_numpy(Dm_in).to(dev) if form == "matrix" else None
        tm = torch.from_numpy(tmin).to(dev)
        mk = torch.from_numpy(mask.view(np.int16)).to(dev) if form == "masks" else None
        _lib.call("qpg_percode_select_sorted_f32", dev, Dm, Rr, tm, mk, nt, Q, Rr, sr.row_code, sr.row_index, sr.zero_row,
                  sr.code_tile, t.K, float(band), qn, sr.xs, t.D, float(R.ABSENT), dist, idx, rank, nn, stats, idx_base, 0, 0)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), idx.cpu().numpy(), rank.cpu().numpy().astype(np.int64), nn.cpu().numpy(), stats.cpu().numpy(), listed


@pytest.mark.parametrize("Q,idx_base", [(300, 0), (5, 0), (300, 4096)])
@pytest.mark.parametrize("noise", R.NOISES)
def test_text_selects_return_the_exact_sweeps_tables(noise, Q, idx_base):
    """Dm_in = sklearn's f32 value + noise of amplitude band / 2.1 (padding rows: their segment's first row's value + their
    own noise), fed three ways; all three must equal the exact sweep's tables bit for bit - distances, indices, ranks, nearest
    neighbours - without the overflow bit."""
    t = R.text_case()
    Dm_in = t.noisy(noise, seed=8)
    rd, ri, rr, rn = t.ref
    for form in ("matrix", "masks", "bycode"):
        dist, idx, rank, nn, stats, listed = _text_select(form, Dm_in, t.band, Q, idx_base)
        assert (stats[1] & 16) == 0, form
        assert np.array_equal(dist.view(np.uint32), rd[:Q].view(np.uint32)), form
        assert np.array_equal(idx, np.where(ri[:Q] >= 0, ri[:Q] + idx_base, -1)), form
        assert np.array_equal(rank, rr[:Q]), form
        assert np.array_equal(nn, rn[:Q] + idx_base), form
        print("CONTRACT text %s %s Q=%d: band=%.3g e=%.3g; %.1f rows evaluated per query (from the inputs, by the select's rule)"
              % (form, noise, Q, t.band, t.e, listed / Q))


def test_text_select_negative_control_a_band_of_1_05_e_is_too_narrow():
    t = R.text_case()
    live = t.layout[1] >= 0
    same, _ = R.has_gap_below(t.d_sorted[:, live].astype(np.float64), t.layout[2][live], t.K, 0.95 * t.e)
    assert same >= 1
    Dm_in = t.noisy("swap")
    for form in ("matrix", "bycode"):
        dist, idx, rank, nn, stats, _ = _text_select(form, Dm_in, 1.05 * t.e, t.Q)
        wrong = int((idx != t.ref[1]).sum())
        print("CONTRACT negative control (text %s, band = 1.05 e): %d wrong winners" % (form, wrong))
        assert wrong >= 1
