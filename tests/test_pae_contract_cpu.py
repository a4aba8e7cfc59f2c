"""tests/pae_ref.py without a GPU: the f64 restatement against the reference's own outputs (tests/golden/pae_s11.npz), the
conditions under which the cases of tests/test_gpu_pae_contract.py bite (asserted: they are not measurements), and the
negative controls - each wrong arithmetic csrc/qpg_pae.hip could have, restated in f64, must leave the bound the device
is held to at the entries it touches."""
import os

import numpy as np
import pytest

from qpgesture_amd import PAE, synth
from qpgesture_amd.checkpoint import load_config
from tests import pae_ref as R
from tests.helpers import load_golden


def _share(name, wrong, ref, bound, need):
    """Share of the touched entries (those the wrong arithmetic changes at all) that leave the bound."""
    err = np.abs(wrong - ref)
    touched = err > 0
    assert touched.any(), name + ": touches nothing"
    r = err[touched] / bound[touched]
    share = float((r > 1).mean())
    print("PAECONTROL %-46s touched %6d  over the bound %5.1f %%  median ratio %.3g" % (name, touched.sum(), 100 * share,
                                                                                      np.median(r)))
    assert share >= need and (r > 1).any(), "%s: only %.1f %% of the touched entries leave the bound" % (name, 100 * share)
    return share


# ---- the restatement against the reference's f32 run ------------------------------------------------------------------
def test_ref_reproduces_the_reference_golden():
    g = load_golden("pae_s11")
    P = R.block("seed11")[0]
    cfg = load_config(os.path.join(os.path.dirname(PAE.__file__), "configs", "codebook.yml"))
    mean, std = np.asarray(cfg.data_mean), np.clip(np.asarray(cfg.data_std), 0.01, None)
    for name, frames in (("long", (0, 350, 699)), ("one", (0,)), ("still", (200,)), ("short", (0, 50, 99, 149))):
        c = g["clip_" + name]
        n = int(c[0])
        pose = synth.make_pae_motion(n, int(c[1]), None if c[2] < 0 else (int(c[2]), int(c[3])))
        r = R.forward(P, dict(pose=pose, mean=mean, std=std, off=np.array([0, n], np.int64)), list(frames))
        sel = list(g["lat_frames_" + name])
        for b, i in enumerate(frames):
            ref = g["phase_" + name][i].reshape(4, 8)
            assert np.all(np.abs(r["out"][b, 1:] - ref[1:]) <= 1e-4 * np.abs(ref[1:]) + 1e-6), (name, i)
            assert np.abs((r["out"][b, 0] - ref[0] + 0.5) % 1.0 - 0.5).max() < 1e-4, (name, i)
            assert np.abs(r["v"][b] - g["v_" + name][i]).max() < 1e-4
            if i in sel:
                assert np.abs(r["latent"][b] - g["lat_" + name][sel.index(i)]).max() < 1e-5


def test_unpack_inverts_pack_params():
    sd = R.seed_sd(29)
    Pd = R.unpack(PAE.pack_params(sd))
    assert np.array_equal(Pd["w1"], sd["conv1.weight"]) and np.array_equal(Pd["w2"], sd["conv2.weight"])
    assert np.array_equal(Pd["b1"], sd["conv1.bias"]) and np.array_equal(Pd["fb"][3], sd["fc.3.bias"])
    assert np.array_equal(Pd["fc"][5], sd["fc.5.weight"]) and Pd["tpi"] == sd["tpi"][0]


# ---- the probe blocks are what they claim -------------------------------------------------------------------------------
def test_probe_blocks():
    for name in ("conv1A", "conv1B", "conv1C", "conv1D", "sparseA", "sparseB", "signedA", "signedB"):
        Pd = R.block(name)[1]
        assert R.is_selector(Pd["w2"], Pd["b2"], Pd["a2"], Pd["be2"]), name
    sel = [R.block("conv1" + s)[1]["w2"] for s in "ABCD"]
    seen = [{(int(o), u + int(k) - 119) for e, o, k in zip(*np.nonzero(w)) for u in range(240)} for w in sel]
    # A and B: all 15 channels and all of positions 0..240; with C and D every (channel, position)
    assert {o for o, t in seen[0] | seen[1]} == set(range(15)) and {t for o, t in seen[0] | seen[1]} == set(range(241))
    assert seen[0] | seen[1] | seen[2] | seen[3] == {(o, t) for o in range(15) for t in range(241)}
    Pd = R.block("conv2")[1]
    assert R.is_selector(Pd["w1"], Pd["b1"], Pd["a1"], Pd["be1"])
    assert sorted(np.nonzero(Pd["w1"])[2]) == sorted(R.SEL_TAPS) and len(set(R.SEL_CHANS)) == 15
    w = R.block("sparseA")[1]["w1"]
    o, c, k = np.nonzero(w)
    assert sorted(c) == list(range(135)) and np.all(o == c % 15)
    assert len(set(k)) == 135 and set(k) >= {0, 239} | set(range(100, 126))
    assert np.all((np.abs(w[w != 0]) >= 0.5) & (np.abs(w[w != 0]) <= 2.0))
    assert np.all(R.block("signedA")[1]["w1"] >= 0) and np.all(R.velocities(R.inputs("signed")) >= 0)


def test_atan_blocks_carry_the_pair_table():
    """v = (0 alpha + beta) must be the table's pair bit for bit, the signs of the zeros included; (0, 0) exactly zero."""
    lat = np.zeros((1, 8, 240))
    for b in (0, 1):
        Pd = R.block("atan%d" % b)[1]
        assert not Pd["fc"].any() and not Pd["fb"].any()
        v = R.head(Pd, lat)["v"].astype(np.float32)[0]
        assert np.array_equal(v.view(np.uint32), R.ATAN_PAIRS[8 * b:8 * b + 8].view(np.uint32))
        p = R.atan2p(v, Pd["tpi"])
        want = R.ATAN_P[8 * b:8 * b + 8]
        assert np.array_equal(np.isnan(p), np.isnan(want)) and np.nanmax(np.abs(p - want)) < 1e-7
    assert R.ATAN_PAIRS[9].view(np.uint32).tolist() == [0, 0] and np.isnan(R.ATAN_P).sum() == 1
    r = np.abs(R.ATAN_PAIRS[:, 1].astype(np.float64) / np.where(R.ATAN_PAIRS[:, 0] == 0, np.nan, R.ATAN_PAIRS[:, 0]))
    assert np.nanmax(r) > 0.9e6 and np.nanmin(r[r > 0]) < 1.1e-6
    quad = {(bool(x < 0), bool(y < 0)) for x, y in R.ATAN_PAIRS[:4]}
    assert len(quad) == 4


# ---- conditions -----------------------------------------------------------------------------------------------------
def _tanh_share(Pd, ref, stage):
    z, a, be = ref["z" + stage], Pd["a" + stage].astype(np.float64), Pd["be" + stage].astype(np.float64)
    return float((np.abs(z * a[None, :, None] + be[None, :, None]) < 1.5).mean())


@pytest.mark.parametrize("blk,inp", R.CONV1_CASES + R.CONV2_CASES + R.HEAD_CASES)
def test_tanh_arguments_are_in_range(blk, inp):
    """A saturated tanh hides errors: at least 80 % of the checked arguments have |arg| < 1.5."""
    P, Pd, I, ref = R.case(blk, inp)
    s1, s2 = _tanh_share(Pd, ref, "1"), _tanh_share(Pd, ref, "2")
    print("PAECONDITION %s/%s: |tanh arg| < 1.5 at %.1f %% (conv1), %.1f %% (conv2)" % (blk, inp, 100 * s1, 100 * s2))
    assert s1 >= 0.8 and s2 >= 0.8


def test_saturating_input_fails_the_condition():
    """The condition is not vacuous: white velocities of sigma 1.0 saturate conv1's tanh."""
    P, Pd = R.block("conv1A")
    I = R.input_white(5, (500,), sigma=1.0)
    ref = R.forward(P, I, [250, 251])
    s1 = _tanh_share(Pd, ref, "1")
    print("PAECONDITION sigma 1.0: |tanh arg| < 1.5 at %.1f %%" % (100 * s1))
    assert s1 < 0.8


@pytest.mark.parametrize("blk,inp", R.HEAD_CASES)
def test_dft_is_not_degenerate(blk, inp):
    ref = R.case(blk, inp)[3]
    print("PAECONDITION %s/%s: smallest AC share of the latent's energy %.3g" % (blk, inp, ref["ac"].min()))
    assert ref["ac"].min() >= 1e-8


def test_inputs_are_what_they_claim():
    I = R.inputs("white")
    assert tuple(np.diff(I["off"])) == R.WHITE_LENS and 0 in np.diff(I["off"]) and len(I["frames"]) >= 35
    v = R.velocities(I)
    inside = np.ones(v.shape[0], bool)
    inside[I["off"][1:][np.diff(I["off"]) > 0] - 1] = False
    assert abs(v[inside].std() - 0.05) < 0.002 and not v[~inside].any()
    S = R.inputs("step")
    v = R.velocities(S)
    assert np.flatnonzero(np.abs(v).sum(1)).tolist() == [R.STEP_AT] and np.all(v[R.STEP_AT] != 0)
    win = R.windows(S, S["frames"], v)
    for b, s in enumerate(R.STEP_ROWS):
        rows = np.flatnonzero(np.abs(win[b]).sum(0)).tolist()
        assert rows == ([] if s in (0, 240) else [s]), s
    # every conv1 position of a step window depends on one tap: 135 products and the bias
    assert R.case("conv1A", "step")[3]["n1"].max() == 136
    H = R.input_velocity_bits(17)
    assert np.abs(H["mean"]).max() > 500 and (H["std"] == 0.01).any() and H["std"].max() > 0.5


# ---- negative controls --------------------------------------------------------------------------------------------------
def _wrong_latent(Pd, I, ref, variant):
    if variant in ("row0", "late", "cross"):
        return R.stages(Pd, R.windows(I, I["frames"], None if variant == "cross" else ref["vel"], variant))["latent"]
    kw = {"lo1": dict(drop1=R.DROP1_LO), "hi1": dict(drop1=R.DROP1_HI), "lo2": dict(drop2=R.DROP2_LO),
          "hi2": dict(drop2=R.DROP2_HI), "no240": dict(no240=True)}[variant]
    return R.stages(Pd, ref["win"], **kw)["latent"]


# variant, what it is, designated cases, smallest share of the touched entries that must leave the bound
CONTROLS = [
    ("lo1", "conv1 lower tap limit 107 - t0", [("conv1A", "step"), ("conv1B", "step"), ("conv1A", "white"), ("sparseA", "step")], 0.0),
    ("hi1", "conv1 upper tap limit 358 - t0", [("conv1A", "step"), ("conv1B", "step"), ("conv1B", "white"), ("sparseB", "step")], 0.0),
    ("lo2", "conv2 lower tap limit 105 - u0", [("conv2", "white")], 0.0),
    ("hi2", "conv2 upper tap limit 358 - u0", [("conv2", "white")], 0.0),
    ("no240", "y1 position 240 missing", [("conv1B", "white"), ("conv1B", "step"), ("conv2", "white")], 0.5),
    ("row0", "window row 0 carries vel[i - 121]", [("conv1A", "white"), ("conv1A", "step"), ("conv2", "white")], 0.5),
    ("late", "window one row late", [("conv1A", "white"), ("conv1B", "step"), ("sparseA", "white"), ("conv2", "white")], 0.5),
    ("cross", "velocity kept across a clip boundary", [("conv1A", "white"), ("conv1B", "white"), ("conv2", "white")], 0.5),
]


@pytest.mark.parametrize("variant,what,cases,need", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_wrong_arithmetic_leaves_the_bound(variant, what, cases, need):
    lowest = 1.0
    for blk, inp in cases:
        P, Pd, I, ref = R.case(blk, inp)
        wrong = _wrong_latent(Pd, I, ref, variant)
        lowest = min(lowest, _share("%s: %s/%s" % (what, blk, inp), wrong, ref["latent"], R.latent_bound(blk, Pd, ref), need))
    print("PAECONTROL %s: lowest share %.1f %%" % (what, 100 * lowest))


def test_wrong_tap_limits_touch_the_cut_tiles():
    """The (position, tap) pairs a wrong limit loses: the last / first position of every tile whose range is cut."""
    assert [t for t, k in R.DROP1_LO] == [15, 31, 47, 63, 79, 95, 111] and all(t + k - 120 == 1 for t, k in R.DROP1_LO)
    assert [t for t, k in R.DROP1_HI] == [128, 144, 160, 176, 192, 208, 224, 240]
    assert all(t + k - 120 == 239 for t, k in R.DROP1_HI)
    assert [u for u, k in R.DROP2_LO] == [15, 31, 47, 63, 79, 95, 111] and all(u + k - 119 == 0 for u, k in R.DROP2_LO)
    assert [u for u, k in R.DROP2_HI] == [128, 144, 160, 176, 192, 208, 224] and all(u + k - 119 == 240 for u, k in R.DROP2_HI)


def test_wrong_velocity_arithmetic_changes_bits():
    """(p1 - p0) / std, or f32 poses, instead of the f64 difference of normalised poses rounded once."""
    I = R.input_velocity_bits(17)
    v = R.velocities(I)
    for variant in ("div_after", "f32_pose"):
        w = R.velocities(I, variant)
        live = v != 0
        share = float((w.view(np.uint32) != v.view(np.uint32))[live].mean())
        print("PAECONTROL velocity %s: %.1f %% of the non-zero velocities differ in their bits" % (variant, 100 * share))
        assert share > 0
    w = R.velocities(I, "cross")
    ends = I["off"][1:-1][np.diff(I["off"])[:-1] > 0] - 1
    assert not v[ends].any() and np.all(np.abs(w[ends]).sum(1) > 0)


def test_wrong_atan_branch_is_half_a_turn_off():
    for idx in (7, 8):                                                       # (-, +0.0) and (-, -0.0)
        v = R.ATAN_PAIRS[idx]
        right, wrong = R.atan2p(v, R.TPI32), R.atan2p(v, R.TPI32, strict=True)
        print("PAECONTROL atan2' y > 0 at (%g, %g): %g instead of %g" % (v[0], v[1], wrong, right))
        assert right == 0.5 and abs(wrong - right) == 0.5
