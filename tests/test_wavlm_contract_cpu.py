"""The bounds of tests/wavlm_ref.py, checked without a device (profiles/wavlm_contract.md holds the printed figures).

Soundness: every case of tests/test_gpu_wavlm_contract.py (the tables of wavlm_ref, shared) is evaluated in NumPy f32 in
the order the kernels state - sequential chains of 512 products whose sums are added in k order, two-pass LayerNorm over
lanes and shuffle steps, max-subtracted softmax - with a multiply-add rounded twice where the device's FMA rounds once,
so it errs on the large side.  Its bound_ratio against the f64 value must be <= 1: a correct f32 evaluation is inside
the bounds.

Teeth: seven mutated REFERENCES, each a mistake a kernel of this family could make at one of its edges, must be outside
the bound of the case named for them.  For each, whether the earlier instrument (max |error| over the tensor against
8 x the max f32 error over the tensor, tests/test_gpu_wavlm.py) would have flagged it is printed as a record."""
import numpy as np
import pytest

from tests import wavlm_ref as R


def _report(kind, name, r):
    print("WAVLMCPU %s %s: err/bound %.3f" % (kind, name, r))


# ---- soundness ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_gemm_f32_is_inside_the_bound(name):
    p = R.gemm_case(name)
    val, bnd = R.gemm_problem_bound(p)
    assert np.isfinite(val).all() and np.isfinite(bnd).all()          # no NaN padding was gathered
    r = R.ratio(R.gemm_problem_f32(p), val, bnd)
    _report("gemm", name, r)
    assert r <= 1.0


@pytest.mark.parametrize("T,C,k,s,with_bias", R.CONV0_CASES)
def test_conv0_f32_is_inside_the_bound(T, C, k, s, with_bias):
    c = R.conv0_case(T, C, k, s, with_bias)
    val, bnd = R.conv0_bound(c["wav"], c["w"], c["bias"], k, s)
    assert val.shape == (c["B"], T, C)
    r = R.ratio(R.conv0_f32(c["wav"], c["w"], c["bias"], k, s), val, bnd)
    _report("conv0", "T=%d C=%d k=%d s=%d bias=%d" % (T, C, k, s, with_bias), r)
    assert r <= 1.0


@pytest.mark.parametrize("M,C,gelu", R.LN_CASES)
def test_layernorm_f32_is_inside_the_bound(M, C, gelu):
    c = R.layernorm_case(M, C)
    val, bnd = R.layernorm_bound(c["x"], c["g"], c["b"], gelu)
    r = R.ratio(R.layernorm_f32(c["x"], c["g"], c["b"], gelu), val, bnd)
    _report("layernorm", "M=%d C=%d gelu=%d" % (M, C, gelu), r)
    assert r <= 1.0


def test_layernorm_bound_follows_the_conditioning():
    """Row by row: the large-mean row's bound is orders of magnitude above a plain row's, which stays near f32's roundoff
    of an O(1) value - what one allowance for the whole tensor cannot do."""
    c = R.layernorm_case(5, 768)
    _, bnd = R.layernorm_bound(c["x"], c["g"], c["b"], 0)
    plain, large = bnd[0].max(), bnd[4].max()
    print("WAVLMCPU layernorm bound: plain row %.2e, large-mean row %.2e" % (plain, large))
    assert plain < 2e-5 and large > 100 * plain


@pytest.mark.parametrize("M,H,kind", R.GATE_CASES)
def test_gate_f32_is_inside_the_bound(M, H, kind):
    c = R.gate_case(M, H, kind)
    val, bnd = R.gate_bound(c["h"], c["gw"], c["gb"], c["ga"], H)
    got = R.gate_f32(c["h"], c["gw"], c["gb"], c["ga"], H)
    assert np.isfinite(got).all() and np.isfinite(val).all()
    if kind == "saturated" and M * H >= 255:
        s = (c["h"].astype(np.float64).reshape(M, H, 64) @ c["gw"].astype(np.float64).T + c["gb"]).reshape(M, H, 2, 4).sum(-1)
        assert s.max() > 100.0 and s.min() < -100.0
    r = R.ratio(got, val, bnd)
    _report("gate", "MH=%d %s" % (M * H, kind), r)
    assert r <= 1.0


@pytest.mark.parametrize("T,B,H,kind", R.ATT_CASES)
def test_attention_f32_is_inside_the_bound(T, B, H, kind):
    c = R.attention_case(T, B, H, kind)
    args = (c["q"], c["k"], c["v"], c["gate"], c["relb"], H)
    val, bnd = R.attention_bound(*args)
    if kind == "zero q":
        assert np.allclose(val, np.repeat(c["v"].astype(np.float64).mean(1, keepdims=True), T, 1), rtol=0, atol=1e-14)
    r = R.ratio(R.attention_f32(*args), val, bnd)
    _report("attention", "T=%d B=%d H=%d %s" % (T, B, H, kind), r)
    assert r <= 1.0


@pytest.mark.parametrize("T", R.POS_T)
def test_pos_conv_f32_is_inside_the_bound(T):
    c = R.pos_case(T)
    ops = R.pos_operands(R.pos_image(c["x"], c["G"], c["K"]), c["w"], c["bias"], c["x"])
    val, bnd = R.gemm_bound(*ops[:3], 1, ops[3])
    # the image form is the grouped convolution of the model's restatement
    weff = c["w"].reshape(c["G"], c["Cg"], c["K"], c["Cg"]).transpose(0, 1, 3, 2).reshape(c["D"], c["Cg"], c["K"])
    want = R.pos_conv(c["x"].astype(np.float64), weff.astype(np.float64), c["bias"], c["G"])
    assert np.abs(R.pos_back(val) - want).max() < 1e-12
    r = R.ratio(R.gemm_f32(*ops[:3], 1, ops[3]), val, bnd)
    _report("pos_conv", "T=%d D=%d" % (T, c["D"]), r)
    assert r <= 1.0


# ---- negative controls ----------------------------------------------------------------------------------------------
def _control(name, mutated, val, bnd, f32):
    """The mutated reference must be outside the bound; whether 8 x e32 in the max norm would have seen it is a record."""
    r = R.ratio(mutated, val, bnd)
    e32 = float(np.abs(np.asarray(f32, np.float64) - val).max())
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.abs(np.asarray(mutated, np.float64) - val))) if np.isfinite(mutated).any() else np.inf
    if not np.isfinite(mutated).all():
        err = np.inf
    old = err > 8.0 * e32
    print("WAVLMCONTROL %s: err/bound %.3g; max-norm check (err %.3g against 8 x e32 = %.3g) %s"
          % (name, r, err, 8.0 * e32, "flags it" if old else "MISSES it"))
    assert r > 1.0, name
    return old


def test_control_gemm_last_k_tile_left_out_in_the_tail_row_tile():
    """K = 528: the 16 products behind the first chunk dropped for the rows of the last 32-row tile (row 64 alone)."""
    p = R.gemm_case("65x129x528")
    val, bnd = R.gemm_problem_bound(p)
    q = dict(p, a=p["a"].copy())
    for m in range(64, p["M"]):
        q["a"][m * p["lda"] + 512:m * p["lda"] + 528] = 0.0
    _control("gemm K=528, last k-tile dropped in the tail row tile", R.gemm_problem_bound(q)[0], val, bnd,
             R.gemm_problem_f32(p))


def test_control_batched_gemm_bias_of_the_previous_group():
    p = R.gemm_case("batched")
    val, bnd = R.gemm_problem_bound(p)
    q = dict(p, bias=np.roll(p["bias"].reshape(p["n_inner"], p["N"]), 1, axis=0).reshape(-1))
    _control("batched gemm, bias of group g - 1", R.gemm_problem_bound(q)[0], val, bnd, R.gemm_problem_f32(p))


def test_control_residual_read_at_ldc_equal_n():
    """ldc = N + 8: the residual gathered with a row stride of N reads other rows' values and the NaN padding columns."""
    p = R.gemm_case("ldc=N+8")
    val, bnd = R.gemm_problem_bound(p)
    A, Wt, bias, res = R.gemm_gather(p, r_ldc=p["N"])
    assert not np.isfinite(res).all()
    mutated = R.gemm_bound(A, Wt, bias, p["gelu"], np.nan_to_num(res, nan=0.0))[0]
    _control("gemm residual read at ldc = N", mutated, val, bnd, R.gemm_problem_f32(p))


def test_control_position_table_read_at_q_minus_k():
    c = R.attention_case(17, 3, 3)
    args = (c["q"], c["k"], c["v"], c["gate"], c["relb"], 3)
    val, bnd = R.attention_bound(*args)
    _control("attention, table at q - k", R.attention_bound(*args, swap_table=True)[0], val, bnd, R.attention_f32(*args))


def test_control_last_key_left_out_at_65():
    """T = 65: key 64 is the one key of the second 64-lane pass of the row maximum and the row sum."""
    c = R.attention_case(65, 3, 3)
    args = (c["q"], c["k"], c["v"], c["gate"], c["relb"], 3)
    val, bnd = R.attention_bound(*args)
    mutated = val.copy()
    mutated[1, 40] = R.attention_bound(*args, keys=64)[0][1, 40]                   # one softmax row (all heads of it)
    _control("attention T=65, last key left out of one row", mutated, val, bnd, R.attention_f32(*args))


def test_control_layernorm_mean_over_64_of_65_channels():
    c = R.layernorm_case(5, 65)
    val, bnd = R.layernorm_bound(c["x"], c["g"], c["b"], 0)
    _control("layernorm C=65, mean over the first 64", R.layernorm_bound(c["x"], c["g"], c["b"], 0, mean_channels=64)[0],
             val, bnd, R.layernorm_f32(c["x"], c["g"], c["b"], 0))


def test_control_conv0_last_frame_of_a_group_reads_the_next_frame():
    c = R.conv0_case(17, 64, 10, 5, 1)
    val, bnd = R.conv0_bound(c["wav"], c["w"], c["bias"], 10, 5)
    _control("conv0, frame 7 of a group of 8 reads frame 8's samples",
             R.conv0_bound(c["wav"], c["w"], c["bias"], 10, 5, shift_last_of_8=True)[0], val, bnd,
             R.conv0_f32(c["wav"], c["w"], c["bias"], 10, 5))
