"""The CPU half of the audio-sweep contract (tests/audio_ref.py; the kernels: tests/test_gpu_audio_contract.py): the
NumPy statement of the sweep agrees with the oracle and with its C restatement, the `grid` family is as exact as it claims,
the `samesign` family really separates a 32-product f32 chain from an uncut one, and the guard predicates mark what the
families planted and nothing else.  Figures are printed (pytest -s)."""
import numpy as np
import pytest

from tests import audio_ref as R

GRID_A = (np.array([0, 7, 3, 12, 14], np.int32), 6, 2)          # T = 23: the last two candidates have padded taps
T_A = 23


def _hl_grid(tap_stride):
    return (np.arange(26, dtype=np.int32) * 3 * tap_stride, 6, tap_stride)


def test_stack_pads_taps_beyond_the_track_with_zeros():
    base = np.arange(2 * 5 * 2, dtype=np.float32).reshape(2, 5, 2) + 1.0
    rows = R.stack(base, [0, 3, 4], 3, 2).reshape(2, 3, 3, 2)
    assert np.array_equal(rows[1, 0], base[1, [0, 2, 4]])
    assert np.array_equal(rows[0, 1, 0], base[0, 3]) and not rows[0, 1, 1:].any()   # frames 5, 7: padding, NOT window 1's
    assert np.array_equal(rows[1, 2, 0], base[1, 4]) and not rows[1, 2, 1:].any()


@pytest.mark.parametrize("name", ["dense", "zeros", "neardup", "spiky"])
def test_distance_equals_the_oracles_cosine_rows(name):
    """oracle.knn_oracle.cosine_rows is sklearn's 0.5 |q/|q| - c/|c||^2 in einsum order; `distance` is 1 - <q,c>/(|q||c|).
    Both are f64 evaluations of the same number with an error of their own of at most gamma_K: the bar is twice
    audio_ref.f64_bar."""
    from oracle import knn_oracle as O
    c = R.family(name, 7, T_A, 128, 9, GRID_A)
    rows = R.stack(c.base, c.cand_t, c.n_taps, c.tap_stride)
    D = R.distance(c.q32, rows)
    want = np.stack([O.cosine_rows(q, rows) for q in c.q32.astype(np.float64)])
    err = np.abs(D - want).max()
    print("%s: max |distance - cosine_rows| = %.3g (bar %.3g)" % (name, err, 2 * R.f64_bar(128)))
    assert err <= 2 * R.f64_bar(128)
    if name == "zeros":
        zero = D.reshape(9, 7, 5)[:8, 1]
        assert np.array_equal(zero, np.full_like(zero, 0.5))       # zero candidate rows: exactly 0.5 ...
        assert np.array_equal(D[8].reshape(7, 5)[1], np.zeros(5))  # ... and exactly 0 against the zero query
        assert np.array_equal(D[8].reshape(7, 5)[3], np.full(5, 0.5))


def test_distance_equals_the_c_restatements_per_code_minima():
    from oracle import cref
    c = R.family("dense", 6, T_A, 128, 4, GRID_A)
    rng = np.random.default_rng(3)
    code = rng.integers(0, 8, size=(6, 5)).astype(np.int32)
    d_ref, i_ref = cref.audio_scan(c.base, c.cand_t, code, np.arange(5), c.q32.astype(np.float64), K=8,
                                   ntaps=c.n_taps, stride=c.tap_stride)
    D = R.distance(c.q32, R.stack(c.base, c.cand_t, c.n_taps, c.tap_stride))
    flat = code.reshape(-1)
    for k in range(8):
        sel = np.flatnonzero(flat == k)
        if len(sel) == 0:
            assert (d_ref[:, k] == 1e3).all()
            continue
        assert np.array_equal(sel[np.argmin(D[:, sel], axis=1)], i_ref[:, k])
        assert np.abs(D[:, sel].min(axis=1) - d_ref[:, k]).max() <= 2 * R.f64_bar(128)


@pytest.mark.parametrize("F", [128, 256])
def test_grid_family_is_exact_in_f32_in_any_order(F):
    c = R.family("grid", 3, T_A, F, 4, GRID_A)
    rows = R.stack(c.base, c.cand_t, c.n_taps, c.tap_stride)
    exact = c.q32.astype(np.float64) @ rows.T
    k64 = np.rint(c.base.astype(np.float64) * 64)
    assert np.array_equal(k64 / 64, c.base) and np.abs(k64).max() <= 64
    assert np.array_equal(c.base.astype(np.float16).astype(np.float32), c.base)         # the f16 track is the same track
    # the f64 sums are integers in units of 2^-12 below 2^24: whatever BLAS did, this IS the exact dot
    units = exact * 4096
    assert np.array_equal(units, np.rint(units)) and np.abs(units).max() < 2 ** 24
    assert np.abs(c.q32.astype(np.float64))[:, None, :].__mul__(np.abs(rows)[None]).sum(-1).max() * 4096 < 2 ** 24
    rows32 = rows.astype(np.float32)
    fwd = R.f32_chain_dot(c.q32, rows32)                                                # ONE f32 chain, forward
    shuf = R.f32_chain_dot(c.q32, rows32, order=np.random.default_rng(1).permutation(6 * F))
    assert np.array_equal(fwd, exact) and np.array_equal(shuf, exact)
    cn2, qn2 = R.norms(c.base, c.cand_t, c.q32, c.n_taps, c.tap_stride)
    rev = (rows[:, ::-1] ** 2).cumsum(axis=1)[:, -1]
    assert np.array_equal(cn2, rev) and np.array_equal(cn2 * 4096, np.rint(cn2 * 4096))  # order-independent: exact
    assert np.array_equal(qn2 * 4096, np.rint(qn2 * 4096))
    assert np.array_equal(R.frame_norm2(c.base).reshape(-1) * 4096, np.rint(R.frame_norm2(c.base).reshape(-1) * 4096))


@pytest.mark.parametrize("F", [128, 256])
def test_samesign_family_tells_a_cut_chain_from_an_uncut_one(F):
    """A NumPy model of SEQUENTIAL f32 chains (audio_ref.f32_chain_dot) on the `samesign` family, error relative to
    |q||c| (= the error of the distance).  Chains of 32, the kernels' contract, must stay under AUDIO_MX_ERR; ONE uncut
    chain over the 6 F products must exceed 4 x AUDIO_MX_ERR: a sweep that stopped flushing its f32 accumulators into the
    f64 sums would fail tests/test_gpu_audio_contract.py on this family, which |Gaussian| data (the same uncut chain: printed, under the bound) never shows.
    Chains of 64 are NOT distinguishable from the bound by any input: gamma_64 = 3.8e-6 is the worst case over all data
    and all summation orders, this family reaches 2^-20 = 9.5e-7 with them - inside AUDIO_MX_ERR = gamma_32 + slack.  The
    figure is printed and nothing is asserted about it.
    Where a kernel's chain would end if it were never cut: the LDS-shared-query organisation (mx2) runs a lane's whole
    contraction through one accumulator (6 F products: the uncut figure); a split-K wave owns a quarter of the features
    (6 F / 4 products: 1.2 x the bound at F = 128, 2.5 x at F = 256 - so the split-K cases of the GPU test carry this family
    at F = 256).  The device's own figure on this family, 3.58e-07 in every organisation, is this model's figure for
    chains of 32 to the last digit: the f32 matrix core accumulates like a sequential chain here.
    The split-f16 sweeps (hl, hl1) are a different matter.  Their instruction sums 32 exact products in a wide adder and
    rounds ONCE, so a chain that was never cut would add one f32 rounding of the running sum per instruction: at most
    3 F / 32 = 12 (F = 128) or 24 (F = 256) roundings of 2^-24 each, 7e-7 or 1.4e-6 in the worst case, against a bound of
    1.3e-6 that budgets 7.75e-7 for the chains as they are.  No input at these widths separates the two; this family is
    exact there (a power of two times 1 + 2^-15 has a power of two as its h plane).  The hl tests below F = 1024 check the
    bound, the padding, the tiling and the guards - not the cut of the chains."""
    from qpgesture_amd.code_knn import AUDIO_MX_ERR
    c = R.family("samesign", 6, T_A, F, 3, (np.array([0, 7], np.int32), 6, 2))
    rows = R.stack(c.base, c.cand_t, c.n_taps, c.tap_stride)
    cn2, qn2 = R.norms(c.base, c.cand_t, c.q32, c.n_taps, c.tap_stride)
    scale = np.sqrt(qn2)[:, None] * np.sqrt(cn2)[None, :]
    exact = c.q32.astype(np.float64) @ rows.T
    rel = {}
    for chain in (32, 64, 6 * F // 4, None):
        rel[chain] = (np.abs(R.f32_chain_dot(c.q32, rows.astype(np.float32), chain) - exact) / scale).max()
    g = np.random.default_rng(0)
    gq, gr = np.abs(g.standard_normal((3, 6 * F))).astype(np.float32), np.abs(g.standard_normal((12, 6 * F))).astype(np.float32)
    gauss = (np.abs(R.f32_chain_dot(gq, gr) - gq.astype(np.float64) @ gr.astype(np.float64).T)
             / (np.linalg.norm(gq.astype(np.float64), axis=1)[:, None] * np.linalg.norm(gr.astype(np.float64), axis=1)[None])).max()
    print("F=%d samesign: chains of 32 %.3g, of 64 %.3g, of %d (a split-K wave's share) %.3g, uncut %.3g; |Gaussian| uncut "
          "%.3g; AUDIO_MX_ERR %.3g" % (F, rel[32], rel[64], 6 * F // 4, rel[6 * F // 4], rel[None], gauss, AUDIO_MX_ERR))
    assert rel[32] <= AUDIO_MX_ERR
    assert rel[None] > 4 * AUDIO_MX_ERR
    if F == 256:
        assert rel[6 * F // 4] > 2 * AUDIO_MX_ERR
    assert gauss < AUDIO_MX_ERR                                   # what random data says about the same uncut chain


@pytest.mark.parametrize("name", R.FAMILIES)
def test_guard_predicates_mark_the_planted_rows_and_nothing_else(name):
    """On the grid the mx kernels are tested on, on an hl grid with padding, and on the f16-rounded track: the predicate
    equals the planted mask on every live candidate, and every operand is at least 2^4 (hl) / 2^10 and 4 (mx, above and
    below) away from its threshold (the device's norms differ from NumPy's in the last bits only)."""
    for grid, T, N, Q in ((GRID_A, T_A, 13, 48), (_hl_grid(1), 78, 9, 49)):
        c = R.family(name, N, T, 128, Q, grid)
        for half in (False, True):
            base = c.base.astype(np.float16).astype(np.float32) if half else c.base
            cn2, qn2 = R.norms(base, c.cand_t, c.q32, c.n_taps, c.tap_stride)
            live = (qn2 > 0)[:, None] & (cn2 > 0)[None, :]
            mx, hl = R.mx_guard(qn2, cn2), R.hl_guard(base, c.q32, qn2, cn2)
            assert np.array_equal(mx, R.planted_mask(c, "mx") & live), (name, half)
            assert np.array_equal(hl, R.planted_mask(c, "hl") & live), (name, half)
            assert bool(c.plant_mx) == (name == "tiny") and bool(c.plant_hl) == (name in ("tiny", "quiet"))
            p = qn2[:, None] * cn2[None, :]
            assert not ((p > 0) & ~mx & (p < R.MX_GUARD_P * 1024)).any() and (p[mx] < R.MX_GUARD_P / 4).all()
            assert np.array_equal(R.hl_guard(base, c.q32, qn2, cn2 / 16)[live], R.hl_guard(base, c.q32, qn2, cn2 * 16)[live])


def test_hl_exponent_brackets_the_largest_magnitude():
    for amax in (1.0, 0.999, 4.7, 2.0 ** -30, 65504.0, 1024.0 * 6.5):
        e = R.hl_exponent(amax)
        assert 2.0 ** 14 <= amax * 2.0 ** e < 2.0 ** 15
    assert R.hl_exponent(0.0) == 0
