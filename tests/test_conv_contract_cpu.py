"""The forward-kernel contract of tests/conv_ref.py checked without a GPU: the f64 definition against torch's own
convolutions, the restated launch rules at hand-computed points, every bound against every planted fault at every case
of the GPU case table (for 256, 304 and 64 CUs), the case table against the set of kernel variants the production
shapes can reach, and the quantiser's inputs (at least 90 % of the rows decided by the reference alone)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

N_CUS = (256, 304, 64)


def _tables():
    return {n: R.cases(n) for n in N_CUS}


TABLES = _tables()


# ----------------------------------------------------------------------------------------------------------------
# the definition
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps,s,pad_,dil", [(3, 1, 3, 3), (4, 2, 1, 1), (1, 1, 0, 1), (3, 1, 9, 9)])
def test_conv_ref_is_torch_conv1d(taps, s, pad_, dil):
    g = torch.Generator().manual_seed(taps * 10 + dil)
    B, T, Cin, Cout = 3, 8, 5, 7
    x = torch.randn((B, T, Cin), generator=g, dtype=torch.float64)
    w = torch.randn((taps, Cin, Cout), generator=g, dtype=torch.float64)
    b = torch.randn((Cout,), generator=g, dtype=torch.float64)
    T_out = T // s
    res = torch.randn((B, T_out, Cout), generator=g, dtype=torch.float64)
    ref, absref = R.conv_ref(x, w, b, (s, -pad_, dil, T_out, 1, 0, T_out), True, True, res)
    want = F.relu(F.conv1d(F.relu(x).transpose(1, 2), w.permute(2, 1, 0), b, stride=s, padding=pad_, dilation=dil))
    want = want.transpose(1, 2)[:, :T_out] + res
    assert float((ref - want).abs().max()) < 1e-12
    wabs = F.conv1d(F.relu(x).transpose(1, 2), w.abs().permute(2, 1, 0), b.abs(), stride=s, padding=pad_, dilation=dil)
    assert float((absref - (wabs.transpose(1, 2)[:, :T_out] + res.abs())).abs().max()) < 1e-12
    assert bool((absref >= ref.abs() - 1e-12).all())
    rows = torch.tensor([0, T_out, B * T_out - 1])
    sub, _ = R.conv_ref(x, w, b, (s, -pad_, dil, T_out, 1, 0, T_out), True, True, res, rows=rows)
    assert torch.equal(sub, ref.reshape(B * T_out, Cout)[rows])


def test_pair_halves_are_conv_transpose1d():
    c = R._case("pair", "t", 3, 5, Cin=6, Cout=4, taps=2, out_stride=2, nz=2)
    x, W, bias, _ = R.make_inputs(c)
    want = R.pair_ref_torch(x, W, bias)
    got = torch.zeros_like(want)
    for w, h in R.pair_halves(c, W):
        ref, _ = R.conv_ref(x, w, bias, R.geom_of(h))
        got[:, h["out_offset"]::2] = ref
    assert float((got - want).abs().max()) < 1e-12


def test_resblock_ref_is_the_block():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 6, 512), generator=g, dtype=torch.float64)
    w1 = torch.randn((3, 512, 512), generator=g, dtype=torch.float64) / 40
    w2 = torch.randn((1, 512, 512), generator=g, dtype=torch.float64) / 20
    b1, b2 = torch.randn((512,), generator=g, dtype=torch.float64), torch.randn((512,), generator=g, dtype=torch.float64)
    h, y, ah, ay = R.resblock_ref(x, w1, b1, w2, b2, 2)
    xc = x.transpose(1, 2)
    hw = F.relu(F.conv1d(F.relu(xc), w1.permute(2, 1, 0), b1, padding=2, dilation=2))
    yw = xc + F.conv1d(hw, w2.permute(2, 1, 0), b2)
    assert float((h - hw.transpose(1, 2)).abs().max()) < 1e-11 and float((y - yw.transpose(1, 2)).abs().max()) < 1e-11
    assert bool((ah >= h - 1e-12).all()) and bool((ay >= y.abs() - 1e-11).all())
    # the absolute contraction goes through both layers
    assert float((ay - (x.abs() + ah @ w2[0].abs() + b2.abs())).abs().max()) < 1e-11


# ----------------------------------------------------------------------------------------------------------------
# the launch rules at points worked out by hand from the launchers
# ----------------------------------------------------------------------------------------------------------------
def test_conv1d_plan_points():
    ws = 8 * 2048 * 512
    # 256 CUs, 512 -> 512: 4 column blocks; M = 30: 4 blocks, ceil(256 / 4) = 64 -> 8; k3: total 96
    assert R.conv1d_plan(30, 512, 512, 512, 512, 3, True, True, ws, 256) == (1, True, True, 8)
    assert R.conv1d_plan(30, 512, 512, 512, 512, 1, True, True, ws, 256) == (1, True, True, 4)      # total / 8 = 4
    assert R.conv1d_plan(30, 135, 144, 512, 512, 1, True, True, ws, 256) == (1, False, True, 1)     # total = 9 < 16
    assert R.conv1d_plan(30, 135, 144, 512, 512, 4, True, True, ws, 256) == (1, False, True, 4)     # total = 36
    assert R.conv1d_plan(30, 512, 512, 512, 512, 3, True, True, None, 256) == (1, True, True, 1)
    assert R.conv1d_plan(30, 512, 512, 512, 512, 3, True, True, 2 * 30 * 512, 256) == (1, True, True, 2)
    assert R.conv1d_plan(30, 512, 512, 512, 512, 3, True, True, 30 * 512 * 3 // 2, 256) == (1, True, True, 1)
    assert R.conv1d_plan(30, 512, 512, 512, 512, 3, False, True, ws, 256)[1] is False
    assert R.conv1d_plan(30, 512, 512, 135, 256, 3, True, True, ws, 256)[2] is False
    assert R.conv1d_plan(30, 512, 512, 512, 512, 3, True, False, ws, 256)[2] is False
    # 40 blocks of 64 rows x 4: ceil(256 / 160) = 2; 64 x 4 = 256 blocks: no split
    assert R.conv1d_plan(40 * 64, 512, 512, 512, 512, 3, True, True, ws, 256)[3] == 2
    assert R.conv1d_plan(64 * 64, 512, 512, 512, 512, 3, True, True, ws, 256)[3] == 1
    assert R.conv1d_plan(64 * 256 - 1, 512, 512, 512, 512, 3, True, True, ws, 256)[0] == 1
    assert R.conv1d_plan(64 * 256, 512, 512, 512, 512, 3, True, True, ws, 256)[0] == 2
    assert R.conv1d_plan(128 * 256 - 1, 512, 512, 135, 256, 3, True, True, ws, 256)[0] == 1
    assert R.conv1d_plan(128 * 256, 512, 512, 135, 256, 3, True, True, ws, 256)[0] == 2


def test_convt_plan_points():
    # 256 CUs, Cout_pad 512: generic from ceil(M / 64) * 8 >= 768, i.e. 96 row blocks
    assert R.convt_plan(95 * 64, 3, 512, 512, 1, 1, 256)[0] == "small"
    assert R.convt_plan(95 * 64 + 1, 3, 512, 512, 1, 1, 256) == ("generic", True)
    assert R.convt_plan(47 * 64, 2, 512, 512, 2, 0, 256)[0] == "small"                # the pair: twice the blocks
    assert R.convt_plan(47 * 64 + 1, 2, 512, 512, 2, 0, 256) == ("generic", False)
    # block shapes: M = 16: 8 / 16 / 32 blocks -> costs 5 / 3 / 2: nq = 1; 129..256 rows: nq = 2; 257..512: nq = 4
    assert R.convt_plan(16, 3, 512, 512, 1, 0, 256) == ("small", False, 4, 1)
    assert R.convt_plan(129, 3, 512, 512, 1, 0, 256) == ("small", False, 4, 2)
    assert R.convt_plan(257, 3, 512, 512, 1, 0, 256) == ("small", False, 4, 4)
    # ring depth: the 144-channel k4 layer has 36 16-k blocks, not a multiple of 8
    assert R.convt_plan(16, 4, 144, 512, 1, 0, 256) == ("small", False, 0, 1)
    assert R.convt_plan(16, 1, 512, 512, 1, 0, 256)[2] == 4 and R.convt_plan(16, 2, 512, 512, 2, 0, 256)[2] == 4


def test_resblock_fused_points():
    assert not R.resblock_fused(1, 191 * 64, 256) and R.resblock_fused(1, 191 * 64 + 1, 256)
    assert R.resblock_fused(256, 60, 256) and not R.resblock_fused(256, 30, 256)      # T = 30 takes two launches


def test_chains():
    assert R.conv1d_chains(3, 512, 1) == [1536, 3] and R.conv1d_chains(3, 512, 8) == [192, 8, 3]
    assert R.conv1d_chains(4, 144, 4) == [144, 4, 3]
    assert R.convt_chains(("generic", False), 3, 512) == [1536, 3]
    assert R.convt_chains(("small", False, 4, 1), 3, 512) == [192, 8, 3]
    assert R.convt_chains(("small", False, 0, 1), 4, 144) == [80, 8, 3]               # 5 of 36 blocks per wave


# ----------------------------------------------------------------------------------------------------------------
# coverage of the kernel variants
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cu", N_CUS)
def test_case_table_hits_every_reachable_variant(n_cu):
    want = R.reachable(n_cu)
    got = R.hit(TABLES[n_cu], n_cu)
    assert got[0] == want[0] == {(1, True), (1, False), (2, True), (2, False)}
    assert got[1] == want[1] == {True, False}
    assert got[2] == want[2] == {1, 2, "interior", 8}
    assert got[3] == want[3], (sorted(got[3] ^ want[3], key=str))
    small = {p for p in want[3] if p[0] == "small"}
    assert {p[3] for p in small} == {1, 2, 4} and {p[2] for p in small} == {0, 4}
    assert ("generic", True) in want[3] and ("generic", False) in want[3]
    assert all(p[2] == 4 for p in small if p[1])                                       # pd = 0 only without ReLU: the k4 144 layer


@pytest.mark.parametrize("n_cu", N_CUS)
def test_case_table_shapes(n_cu):
    """What the issue asks of the shapes: both sides of every rule, with the thresholds of this CU count."""
    t = {c["kernel"] + " " + c["name"]: c for c in TABLES[n_cu]}
    assert len(t) == len(TABLES[n_cu])                                                  # names are unique
    big, small = t["conv1d 1x1 128-row tiles"], t["conv1d 1x1 64-row tiles below the rule"]
    assert big["M"] >= 64 * n_cu > small["M"] and big["M"] - small["M"] == 30
    assert big["M"] % 128 and small["M"] % 128
    assert R.conv1d_variant(big, n_cu)[0] == 2 and R.conv1d_variant(small, n_cu)[0] == 1
    assert R.conv1d_variant(t["conv1d k4 s2 Cin=135 128-row tiles"], n_cu)[:2] == (2, False)
    for name, ks in [("split ks=8", 8), ("split capped by total/8", 4), ("split ws of two slabs", 2),
                     ("split ws of 1.5 slabs", 1), ("split total=9", 1), ("M=63 k3 d3 relu no ws", 1)]:
        assert R.conv1d_variant(t["conv1d " + name], n_cu)[3] == ks, name
    for mis in ("x", "y", "res"):
        v = R.conv1d_variant(t["conv1d 1x1 res misaligned " + mis], n_cu)
        assert v[1] == (mis != "x") and v[2] == (mis == "x")
    assert {t["conv1d " + n]["M"] for n in ("M=1 T_in=1 k3 d3", "M=63 k3 d3 relu", "M=64 k3 d3 res",
                                            "M=65 k3 d3 relu res")} == {1, 63, 64, 65}
    for layer in R.CONVT_LAYERS:
        lo = next(c for c in TABLES[n_cu] if c["name"].startswith(layer + " largest small"))
        hi = next(c for c in TABLES[n_cu] if c["name"].startswith(layer + " smallest generic"))
        assert hi["M"] == lo["M"] + 1
        assert R.convt_variant(lo, n_cu)[0] == "small" and R.convt_variant(hi, n_cu)[0] == "generic"
        nqs = {R.convt_variant(c, n_cu)[3] for c in TABLES[n_cu]
               if c["name"].startswith(layer + " nq=") and R.convt_variant(c, n_cu)[0] == "small"}
        assert nqs == {1, 2, 4}, (layer, nqs)
    assert any(c["kernel"] == "convt" and c["M"] % 16 and c["B"] > 1 and c["T_out"] % 16 for c in TABLES[n_cu])
    assert any(c["kernel"] in ("convt", "conv1d") and c["T_in"] < c["dil"] for c in TABLES[n_cu])
    assert {c["M"] for c in TABLES[n_cu] if c["kernel"] == "res"} >= {63, 64, 65, 24}
    assert {c["M"] for c in TABLES[n_cu] if c["kernel"] == "conv16"} >= {1, 127, 128, 129}


# ----------------------------------------------------------------------------------------------------------------
# the bounds reject every planted fault
# ----------------------------------------------------------------------------------------------------------------
def _case_ids():
    seen, out = set(), []
    for n in N_CUS:
        for c in TABLES[n]:
            key = (c["kernel"], c["name"], c["M"])
            if key not in seen:                    # a case that does not depend on the CU count is checked once ...
                seen.add(key)
                out.append((n, c))
    return out


def _singles(c, x, w, bias, res):
    """The single convolutions of a case: [(w, bias, residual, case)]."""
    if c["kernel"] == "pair":
        return [(wh, bias, None, h) for wh, h in R.pair_halves(c, w)]
    return [(w, bias, res, c)]


FAULTS_SEEN = {}


@pytest.mark.parametrize("n_cu,case", _case_ids(), ids=lambda v: v if isinstance(v, int) else v["kernel"] + ":" + v["name"])
def test_bound_rejects_every_planted_fault(n_cu, case):
    _plant(case)


def _plant(case):
    # ... but with the chains of every CU count whose table holds it (the split count moves with n_cu)
    x, w, bias, res = R.make_inputs(case)
    rows = R.sample_rows(case)
    for n in N_CUS:
        if not any(c["kernel"] == case["kernel"] and c["name"] == case["name"] and c["M"] == case["M"] for c in TABLES[n]):
            continue
        if case["kernel"] == "res":
            h, y, ah, ay = R.resblock_ref(x, w[0], bias[0], w[1], bias[1], case["dil"], rows)
            gh, gy = R.gamma(*R.RES_CHAINS_H), R.gamma(*R.RES_CHAINS_Y)
            assert R.bound_ratio(h.float(), h, ah, gh) <= 1.0 and R.bound_ratio(y.float(), y, ay, gy) <= 1.0
            for label, fault in R.faults_of(case, n):
                fh, fy = R.resblock_eval(x, w[0], bias[0], w[1], bias[1], case["dil"], rows, fault=fault)
                if torch.equal(fy, y):
                    continue
                FAULTS_SEEN.setdefault("res", set()).add(label)
                assert R.bound_ratio(fy, y, ay, gy) > 1.0, (label, n)
                if not torch.equal(fh, h):
                    assert R.bound_ratio(fh, h, ah, gh) > 1.0, (label, n)
            continue
        for w1, b1, r1, c1 in _singles(case, x, w, bias, res):
            geom = R.geom_of(c1)
            ref, absref = R.conv_ref(x, w1, b1, geom, c1["relu_in"], c1["relu_out"], r1, rows)
            if case["kernel"] == "conv16":
                full = R.conv16_bound(R.conv_ref(x, w1, b1, geom, c1["relu_in"], c1["relu_out"], r1)[1], w1, x.shape, geom,
                                      R.pad(c1["Cin"], 8))
                bound, g = full.reshape(-1, full.shape[-1])[rows], 1.0
            else:
                bound, g = absref, R.gamma(*R.chains_of(c1, n))
            assert R.bound_ratio(ref.float(), ref, bound, g) <= 1.0
            for label, fault in R.faults_of(c1, n):
                bad = R.conv_eval(x, w1, b1, geom, c1["relu_in"], c1["relu_out"], r1, rows, fault=fault,
                                  cin_pad=c1["Cin_pad"])
                if torch.equal(bad, ref):          # the fault does not exist at this shape (no halo row, a dead last tap)
                    continue
                FAULTS_SEEN.setdefault(case["kernel"], set()).add(label)
                assert R.bound_ratio(bad, ref, bound, g) > 1.0, (label, n, R.bound_ratio(bad, ref, bound, g))


def test_every_fault_was_planted_on_every_kernel():
    """No fault of the list is absent from a kernel family's cases."""
    if not FAULTS_SEEN:                            # (run on its own: plant them here)
        for _, c in _case_ids():
            _plant(c)
    base = {"one tap dropped", "a tap shifted by one position", "halo row from the neighbouring batch item",
            "last 16-channel K slice dropped", "bias doubled", "relu_in omitted", "residual omitted"}
    assert FAULTS_SEEN["conv1d"] == base | {"one split partial dropped", "the other output parity written"}
    assert FAULTS_SEEN["convt"] == base | {"one split partial dropped", "the other output parity written"}
    assert FAULTS_SEEN["pair"] >= {"one tap dropped", "halo row from the neighbouring batch item",
                                   "the other output parity written", "one split partial dropped"}
    assert FAULTS_SEEN["res"] == base
    assert FAULTS_SEEN["conv16"] == base | {"the other output parity written", "the l.h' term dropped"}


# ----------------------------------------------------------------------------------------------------------------
# the quantiser
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,E,K,ties", R.ARGMIN_SETS)
def test_argmin_inputs_are_decided(R_, E, K, ties):
    z, dot, kk = R.argmin_inputs(R_, E, K, seed=R_ + E + K, ties=ties)
    d, dmin, dsec, ids, b = R.argmin_ref(z, dot, kk)
    assert d.shape == (R_, K) and np.array_equal(dmin, d.min(axis=1))
    tied = np.arange(R_) % 3 != 2 if ties else np.zeros(R_, bool)
    decided = (dsec - dmin) > 2 * b
    # without planted columns: 90 % of all rows; planted ties are undecided by construction (a gap of exactly 0), there
    # the 90 % is of the other rows
    assert not decided[tied].any()
    assert decided[~tied].mean() >= 0.9
    if ties:
        grp = ties[0]
        assert np.array_equal(ids[tied], np.full(int(tied.sum()), min(grp)))
        assert np.array_equal(dsec[tied], dmin[tied])
    if K == 1:
        assert np.isinf(dsec).all() and (ids == 0).all()
    # a runner-up taken from one lane only (columns c % 64 of the winner's lane) is outside the bound somewhere
    if K >= 128 and R_ >= 4:
        lane_sec = np.array([np.sort(d[r, ids[r] % 64::64])[1] for r in range(R_)])
        assert (np.abs(lane_sec - dsec) > b).any()


def test_shape_lists_cover_the_issue():
    assert {s[0] for s in R.ARGMIN_SHAPES} == {1, 3, 4, 5, 1030}
    assert {s[1] for s in R.ARGMIN_SHAPES} == {4, 60, 64, 512}
    assert {s[2] for s in R.ARGMIN_SHAPES} == {1, 63, 64, 65, 512}
    ties = [g for s in R.ARGMIN_SHAPES for g in s[3]]
    assert any(len(g) == 2 and g[1] == g[0] + 1 for g in ties) and any(len(g) == 2 and g[1] == g[0] + 64 for g in ties)
    assert any(len(g) == 3 for g in ties)
    assert any(g[0] == 0 and g[-1] == s[2] - 1 for s in R.ARGMIN_SHAPES for g in s[3])
