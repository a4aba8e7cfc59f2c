"""The CPU half of the prefilter GEMMs' contract (tests/prefilter_ref.py; the kernels: tests/test_gpu_prefilter_contract.py):
the emulated number format obeys the representation term of the error budget (csrc/qpg_audio_hl.hip's header), the input
families are unit-norm, the h planes alone are within the Cauchy-Schwarz term of sorted_rows.gemm_h_err of the true
value, and - for the reference alone - the mask verdicts the GPU test relies on are decisive: few undecided bits per
family, and enough bits that MUST be set beyond the argmin and that MUST be clear for a wrong mask to show.
The shares are printed (pytest -s)."""
import functools

import numpy as np
import pytest

from tests import prefilter_ref as P

DIMS = (128, 384, 512, 640, 1024)
Q_CPU, TILES, SEED = 48, 8, 1
LIVE_FAMILIES = [f for f in P.FAMILIES if f != "zeros"]


def errs(D):
    """(bound of the matrix forms whatever kernel runs, chain + f32 epilogue of the h-plane form) at width D."""
    from qpgesture_amd.sorted_rows import HL_GEMM_ERR, gemm32_err
    return max(HL_GEMM_ERR, gemm32_err(D)), gemm32_err(D) - 5.2e-7 + 1.2e-7


@functools.lru_cache(maxsize=None)
def _inputs(name, D):
    qn = P.queries(Q_CPU, D, SEED)
    xs = P.family(name, qn, TILES, SEED)
    xs.setflags(write=False)
    qn.setflags(write=False)
    return xs, qn


@functools.lru_cache(maxsize=None)
def _verdicts(name, D):
    """The two settings of the GPU test: (full-precision forms against `exact`, h-plane form against `exact_h`)."""
    from qpgesture_amd.sorted_rows import prefilter_band, prefilter_band_h
    xs, qn = _inputs(name, D)
    e_full, e_chain = errs(D)
    return (P.mask_verdict(P.exact(xs, qn), prefilter_band(D), e_full),
            P.mask_verdict(P.exact_h(xs, qn), prefilter_band_h(D), e_chain))


def test_exponent_lands_the_maximum_in_its_binade():
    rng = np.random.default_rng(7)
    for amax in list(np.exp(rng.uniform(np.log(1e-20), np.log(1e20), 200)).astype(np.float32)) + [1.0, 0.5, 2.0 ** -14]:
        e = P.exponent(amax)
        assert 2.0 ** 14 <= float(amax) * 2.0 ** e < 2.0 ** 15
    assert P.exponent(1.0) == 14 and P.exponent(np.float32(1.0) - np.float32(2.0 ** -24)) == 15
    for amax in (0.0, -0.0, np.inf, np.nan):
        assert P.exponent(amax) == 0
    assert P.row_exponent(np.zeros((16, 128), np.float32)) == 0
    assert P.query_exponents(np.zeros((2, 128), np.float32)).tolist() == [0, 0]


@pytest.mark.parametrize("D", DIMS)
def test_split_identity_within_the_representation_term(D):
    """x 2^e = h + 2^-11 l + delta, |delta| <= 2^-23 |x 2^e| + 2^-36 (x - h is exact and below half an ulp of h; l keeps 11
    bits of it, or is an f16 subnormal with an absolute error of 2^-25 2^-11), h is x 2^e rounded to f16."""
    for name in LIVE_FAMILIES:
        xs, qn = _inputs(name, D)
        for x, e in [(xs, P.row_exponent(xs))] + [(q, eq) for q, eq in zip(qn[:6], P.query_exponents(qn[:6]))]:
            h, l = P.split(x, e)
            assert h.dtype == np.float16 and l.dtype == np.float16
            scaled = x.astype(np.float64) * 2.0 ** e
            assert np.abs(scaled).max(initial=0.0) < 2.0 ** 15
            delta = scaled - h.astype(np.float64) - l.astype(np.float64) * 2.0 ** -11
            assert (np.abs(delta) <= 2.0 ** -23 * np.abs(scaled) + 2.0 ** -36).all()
            assert np.array_equal(h, scaled.astype(np.float32).astype(np.float16))
            assert (np.abs(scaled - h.astype(np.float64)) <= 2.0 ** -11 * np.abs(scaled) + 2.0 ** -25).all()


@pytest.mark.parametrize("D", DIMS)
def test_families_are_unit_norm_or_zero(D):
    qn = _inputs("dense", D)[1]
    nq = np.sqrt((qn.astype(np.float64) ** 2).sum(axis=1))
    assert nq[3] == 0.0 and (np.abs(np.delete(nq, 3) - 1.0) <= 1e-6).all()
    assert 3 not in P.live_queries(qn).tolist() and P.live_queries(qn).size == Q_CPU - 1
    for name in P.FAMILIES:
        xs = _inputs(name, D)[0]
        assert xs.shape == (16 * TILES, D) and xs.dtype == np.float32 and np.isfinite(xs).all()
        n = np.sqrt((xs.astype(np.float64) ** 2).sum(axis=1))
        assert (n == 0.0).all() if name == "zeros" else (np.abs(n - 1.0) <= 1e-6).all()
    spiky = _inputs("spiky", D)[0]
    assert (np.sort(np.abs(spiky[:16]), axis=1)[:, -1] == 1.0).all() and (np.sort(np.abs(spiky[:16]), axis=1)[:, -2] == 0).all()
    assert P.row_exponent(spiky) == 14
    cancel, qn = _inputs("cancel", D)
    ex = P.exact(cancel, qn)
    four = P.live_queries(qn)[:4]
    assert (np.abs(ex[four, np.arange(4)]) <= 1e-6).all() and (np.abs(ex[four, 4 + np.arange(4)] - 2.0) <= 1e-6).all()
    # a cancelling row against its own query: sum |products| = 1, the dot product three orders below it
    own = np.abs(np.abs(cancel[8:, None, :]) - np.abs(qn[None, :, :])).max(axis=2).argmin(axis=1)
    assert (np.abs(ex[own, 8 + np.arange(own.size)] - 1.0) <= 1e-3).all()
    assert (np.abs(cancel[8:].astype(np.float64) * qn[own]).sum(axis=1) >= 1.0 - 1e-6).all()


@pytest.mark.parametrize("D", DIMS)
def test_h_planes_within_the_cauchy_schwarz_term(D):
    """|exact_h - exact| <= (2^-10 + 2^-22) |x||q|: the dropped terms h l' + l h' + l l' of sorted_rows.gemm_h_err."""
    worst = 0.0
    for name in P.FAMILIES:
        xs, qn = _inputs(name, D)
        worst = max(worst, float(np.abs(P.exact_h(xs, qn) - P.exact(xs, qn)).max()))
        if name == "zeros":
            assert np.array_equal(P.exact_h(xs, qn), np.ones((Q_CPU, 16 * TILES)))
    print("PREFILTER-REF D=%d: max |exact_h - exact| = %.3g (term %.3g)" % (D, worst, 2.0 ** -10 + 2.0 ** -22))
    assert worst <= 2.0 ** -10 + 2.0 ** -22


def test_mask_rule_and_verdict_on_a_hand_made_tile():
    band, E = 1e-3, 1e-5
    ref = np.full((1, 16), 1.0)
    ref[0, :4] = [0.5, 0.5 + band - 3 * E, 0.5 + band, 0.5 + band + 3 * E]
    v = P.mask_verdict(ref, band, E)
    assert v.shape == (1, 1, 16) and v[0, 0, :4].tolist() == [1, 1, 0, -1] and (v[0, 0, 4:] == -1).all()
    m = P.mask_rule(ref.astype(np.float32), band)
    assert m.dtype == np.uint16 and m.shape == (1, 1) and m[0, 0] & 0b1011 == 0b0011 and m[0, 0] >> 4 == 0
    assert P.mask_bits(m)[0, 0].tolist() == [bool(m[0, 0] >> r & 1) for r in range(16)]
    assert P.mask_rule(np.ones((2, 32), np.float32), 0.0).tolist() == [[0xffff, 0xffff]] * 2


@pytest.mark.parametrize("D", DIMS)
def test_few_mask_bits_are_undecided_for_the_reference_alone(D):
    """The caps the GPU test relies on: per family at most 10 % of the mask bits are left open by the a-priori bounds."""
    for name in P.FAMILIES:
        for setting, v in zip(("full", "h"), _verdicts(name, D)):
            share = float((v == 0).mean())
            print("PREFILTER-REF D=%d %-9s %-4s undecided %.4f  set %.4f  clear %.4f"
                  % (D, name, setting, share, (v == 1).mean(), (v == -1).mean()))
            assert share <= 0.10, (name, D, setting, share)


def test_enough_bits_are_decided_each_way():
    """Over the non-zero families together, in both settings: at least 1 % of all bits must be set BEYOND each tile's
    argmin (whose bit any rule sets) and at least 1 % must be clear."""
    for k, setting in enumerate(("full", "h")):
        v = np.concatenate([_verdicts(name, D)[k].reshape(-1, 16) for name in LIVE_FAMILIES for D in DIMS])
        beyond = float(((v == 1).sum() - v.shape[0]) / v.size)
        clear = float((v == -1).mean())
        print("PREFILTER-REF %-4s must-set beyond the argmin %.4f  must-clear %.4f" % (setting, beyond, clear))
        assert ((v == 1).sum(axis=1) >= 1).all()              # the argmin itself is always decided
        assert beyond >= 0.01 and clear >= 0.01


def test_layout_reference_images_decode_to_their_inputs_and_cover_every_byte_once():
    """tests/hl_layout_ref.py against itself, on random input with a zero query, one element that sets the exponent and
    values whose l is an f16 subnormal: read back the way the GEMMs read them (whole fragments, reshaped), the five images
    hold h = fl16(x 2^e) and an l with x 2^e - h - l (resp. 2^-11 l) within 2^-11 of |x 2^e - h| plus half a subnormal f16
    step (2^-25; 2^-36 under the 2^-11), zero pieces in the padding slots - and every 16-byte unit of the fragments is
    written exactly once."""
    from tests import hl_layout_ref as L
    rng = np.random.default_rng(11)

    def values(*shape):
        x = (rng.standard_normal(shape) * np.exp(rng.uniform(np.log(1e-12), 0.0, shape))).astype(np.float32)
        x.reshape(-1)[rng.integers(0, x.size)] = 300.0                      # sets the exponent
        return x

    def check(planes, x, e, lscale, tiny):
        xs = np.asarray(x, np.float32) * np.float32(2.0) ** np.asarray(e, np.float32)
        h = planes[0].astype(np.float32)
        assert np.array_equal(planes[0], xs.astype(np.float16))
        r = (xs - h).astype(np.float64)
        assert np.all(np.abs(r - planes[1].astype(np.float64) * lscale) <= 2.0 ** -11 * np.abs(r) + tiny)
        assert np.any((planes[1] != 0) & (np.abs(planes[1].astype(np.float64)) < 2.0 ** -14)), "no subnormal l in the input"

    F, N, T = 128, 3, 157
    base = values(N, T, F)
    img = L.db_image(base, 6, 2, 2)
    assert np.all(img.writes == 1) and img.frags.size == N * (3 * F // 32) * 2 * 108 * 16
    rows = L.super_rows(base, 6, 2)
    assert not rows[:, 26, F:].any() and rows[:, 26, :F].any()            # T = 157: frames 158 and 160 lie beyond the track
    check(L.db_decode(img, N, F, 2), rows, img.exps[0], 1.0, 2.0 ** -25)
    b16 = base.astype(np.float16)
    img1 = L.db_image(b16, 6, 2, 1)
    assert np.all(img1.writes == 1) and img1.exps[0] == 0 and img1.frags.size * 2 == img.frags.size
    assert np.array_equal(L.db_decode(img1, N, F, 1)[0], L.super_rows(b16, 6, 2))

    for Q, builder, K, halves, qc, lscale, tiny in ((49, L.audio_query_image, 3 * F, 2, L.QC, 1.0, 2.0 ** -25),
                                                    (97, L.cols_image, 384, 1, L.GQC, 2.0 ** -11, 2.0 ** -36)):
        q = values(Q, halves * K)
        q[3] = 0.0
        img = builder(q)
        slots = -(-Q // qc) * qc
        assert np.all(img.writes == 1) and img.frags.size == slots * halves * K * 4 and img.exps.size == slots
        assert img.exps[3] == 0 and np.all(img.exps[Q:] == 0)
        planes = L.cols_decode(img, K, halves, qc)
        assert not planes[:, Q:].any() and not planes[:, 3].any()
        check(planes[:, :Q], q, img.exps[:Q, None], lscale, tiny)

    x = values(96, 384)
    img = L.rows_image(x)
    assert np.all(img.writes == 1) and img.frags.size == x.size * 4
    check(L.rows_decode(img, 384), x, img.exps[0], 2.0 ** -11, 2.0 ** -36)
