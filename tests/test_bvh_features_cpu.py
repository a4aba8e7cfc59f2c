"""BVH ingestion, host side (qpgesture_amd/process_bvh.py) and the NumPy restatement (tests/bvh_ref.py) against what the
reference's own pymo + scipy computed on two synthetic files (tests/golden/bvh_features_*.npz, written by
tests/golden/make_golden_bvh_features.py).  No GPU: the kernels' tests are tests/test_gpu_bvh_features.py."""
import os

import numpy as np
import pytest

from tests import bvh_ref as B
from tests.helpers import load_golden

GOLDENS = ("bvh_features_zxy", "bvh_features_xyz")


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_golden(name):
    """values bitwise; upper / upper_mirror: the f64 restatement's error against the longdouble one is at most 4 x the
    reference's own (scipy goes through quaternions), both measured here."""
    g = load_golden(name)
    data = g["bvh"].tobytes()
    header, F, ft, motion = B.split_file(data)
    names = B.channel_names(header)
    assert (F, len(names)) == g["values"].shape == (41, 75)
    vals = B.parse_values(motion, F * len(names)).reshape(F, -1)
    assert np.array_equal(vals.view(np.int64), g["values"].view(np.int64))
    for fps, T in ((60, 20), (20, 7)):
        up, um = B.features(vals, names, ft, fps)
        upl, uml = B.features(vals, names, ft, fps, dtype=np.longdouble)
        for got, ld, want in ((up, upl, g["upper_%d" % fps]), (um, uml, g["upper_mirror_%d" % fps])):
            assert got.shape == want.shape == (T, 135) and got.dtype == np.float64
            e_ref, e_got = np.abs(want - ld).max(), np.abs(got - ld).max()
            print(name, fps, "reference vs longdouble %.3e, restatement vs longdouble %.3e" % (e_ref, e_got))
            assert 0 < e_ref < 1e-15 and e_got <= 4 * e_ref
        assert np.abs(up - um).max() > 0.1                  # the mirror copy is another array


def test_the_two_goldens_pin_file_order_and_signs_by_name():
    """Zrotation Xrotation Yrotation vs Xrotation Yrotation Zrotation: the same table positions feed the angles (file order
    used as 'ZXY'), the mirror signs follow the channel NAMES."""
    tabs = {}
    for name in GOLDENS:
        header = B.split_file(load_golden(name)["bvh"].tobytes())[0]
        tabs[name] = B.tables(B.channel_names(header))
    (c0, m0, s0), (c1, m1, s1) = tabs["bvh_features_zxy"], tabs["bvh_features_xyz"]
    assert np.array_equal(c0, c1) and np.array_equal(m0, m1)
    assert np.array_equal(s0, np.tile([-1.0, 1.0, -1.0], (15, 1))) and np.array_equal(s1, np.tile([1.0, -1.0, -1.0], (15, 1)))


def test_exact_path_alone_covers_fixed_point_text():
    """The arithmetic of the parse kernel's exact path, restated: for %.6f text of |x| < 10^4 - what BVH exporters write -
    it equals float() on every one of 200 000 tokens, with no token left to the fallback list; and which tokens it leaves."""
    rng = np.random.default_rng(1)
    toks = [b"%.6f" % x for x in rng.uniform(-9999.999999, 9999.999999, size=200000)]
    got = np.array([B.exact_value(t) for t in toks], np.float64)                 # (a None would make this an object array)
    assert np.array_equal(got.view(np.int64), np.array([float(t) for t in toks]).view(np.int64))
    for t in (b"-0.000000", b"1e-05", b"-1.5E+2", b".5", b"5.", b"+.25", b"007", b"1.e2", b"9007199254740992", b"1e22", b"0e999"):
        v = B.exact_value(t)
        assert v == float(t) and np.signbit(v) == np.signbit(float(t)), t
    for t in (b"0.12345678901234567890123", b"1e300", b"9007199254740993", b"1e23", b"-2.5e-23", b"12345678901234567890"):
        assert B.exact_value(t) is None, t
    for t in (b"abc", b"1.5.2", b"--1", b"1e", b"-", b".", b"nan", b"1,5"):
        with pytest.raises(ValueError):
            B.exact_value(t)


def _record(text):
    from qpgesture_amd import process_bvh as P
    head, frames, ft, off = P.split_bvh(text.encode())
    skel, names, root = P.parse_hierarchy(head)
    return P.BVHRecord(None, names, skel, ft, root, frames, None), off


def test_hierarchy_parse():
    text = B.bvh_text(np.zeros((3, B.n_channels())), order="ZXY", frametime=1 / 120.0)
    rec, off = _record(text)
    order = B.joint_order()
    assert rec.root_name == "Hips" and rec.header_frames == 3 and abs(rec.frametime - 1 / 120.0) < 1e-8
    assert [j for j in rec.skeleton if not j.endswith("_Nub")] == order
    assert sorted(j for j in rec.skeleton if j.endswith("_Nub")) == sorted(
        n + "_Nub" for n in ("Head", "RightHandIndex1", "LeftHandIndex1", "RightFoot", "LeftFoot"))
    assert rec.skeleton["Head_Nub"]["parent"] == "Head" and rec.skeleton["Head_Nub"]["channels"] == []
    assert rec.skeleton["Head_Nub"]["offsets"] == [0.0, 4.0, 0.0] and rec.skeleton["Spine"]["offsets"] == [0.0, 10.5, -1.25]
    assert rec.skeleton["Spine3"]["children"] == ["Neck", "RightShoulder", "LeftShoulder"]
    assert rec.skeleton["Hips"]["parent"] is None and rec.skeleton["Hips"]["order"] == "ZXY"
    assert rec.skeleton["Hips"]["channels"] == ["Xposition", "Yposition", "Zposition", "Zrotation", "Xrotation", "Yrotation"]
    assert rec.channel_names == B.channel_names(B.split_file(text.encode())[0])
    assert rec.channel_names[6:9] == [("Spine", "Zrotation"), ("Spine", "Xrotation"), ("Spine", "Yrotation")]
    assert len(rec.channel_names) == 75
    assert text.encode()[off:].split()[0] == b"0.000000"        # the motion block starts right after the frame time
    for broken in (text.replace("HIERARCHY", "HIERARCHIE"), text.replace("MOTION", "MOTIONS"),
                   text.replace("JOINT Neck\n", "JOINT Neck\n{\n", 1)):
        with pytest.raises(ValueError):
            _record(broken)


def test_rotation_tables():
    from qpgesture_amd import process_bvh as P
    for order in ("ZXY", "XYZ"):
        text = B.bvh_text(np.zeros((2, B.n_channels())), order=order)
        rec, _ = _record(text)
        col, mcol, sign = P.rotation_tables(rec)
        wc, wm, ws = B.tables(rec.channel_names)
        assert np.array_equal(col, wc) and np.array_equal(mcol, wm) and np.array_equal(sign, ws)
        assert col.dtype == mcol.dtype == np.int32 and sign.dtype == np.float64 and col.shape == (15, 3)
        names = ["%s_%s" % jc for jc in rec.channel_names]
        for n, j in enumerate(P.TARGET_JOINTS):
            partner = j.replace("Left", "Right") if "Left" in j else j.replace("Right", "Left")
            assert (partner != j) == (n >= 7)
            for k in range(3):
                assert names[col[n, k]] == "%s_%srotation" % (j, order[k])
                assert names[mcol[n, k]] == "%s_%srotation" % (partner, order[k])
                assert sign[n, k] == {"X": 1.0, "Y": -1.0, "Z": -1.0}[order[k]]
    # exact names: a finger joint does not stand in for the hand, one joint alone
    c1, m1, _ = P.rotation_tables(rec, joints=["RightHandIndex1"])
    assert names[c1[0, 0]] == "RightHandIndex1_Xrotation" and names[m1[0, 0]] == "LeftHandIndex1_Xrotation"
    # the three refusals
    with pytest.raises(ValueError, match="not in the file"):
        P.rotation_tables(rec, joints=["Spine", "Spine4"])
    text = B.bvh_text(np.zeros((2, B.n_channels())), order="XYZ")
    lines = text.split("\n")
    i = [k for k, l in enumerate(lines) if l.strip() == "JOINT Neck"][0]
    assert "CHANNELS 3" in lines[i + 3]
    lines[i + 3] = lines[i + 3].replace("CHANNELS 3 Xrotation Yrotation Zrotation", "CHANNELS 2 Xrotation Yrotation")
    with pytest.raises(ValueError, match="not three"):
        P.rotation_tables(_record("\n".join(lines))[0])
    with pytest.raises(ValueError, match="no mirror partner"):
        P.rotation_tables(_record(text.replace("LeftForeArm", "LForeArm"))[0],
                          joints=[j for j in P.TARGET_JOINTS if j != "LeftForeArm"])


@pytest.mark.parametrize("F", [1, 2, 3, 41])
@pytest.mark.parametrize("rate", [1, 2, 6])
def test_row_ranges(F, rate):
    from qpgesture_amd import process_bvh as P
    assert P.n_output_frames(F, rate) == len(range(0, F - 1, rate)) == len(np.arange(F)[0:-1:rate]) == len(B.rows(F, rate))
    if F == 1:
        assert P.n_output_frames(F, rate) == 0


def test_frame_rate():
    from qpgesture_amd import process_bvh as P
    assert P.frame_rate(0.00833333, 60) == 2 and P.frame_rate(0.00833333, 20) == 6 and P.frame_rate(1 / 60.0, 60) == 1
    with pytest.warns(UserWarning, match="not dividable"):
        assert P.frame_rate(0.01, 30) == 3
    with pytest.raises(ValueError):
        P.frame_rate(1 / 30.0, 60)


def _speaker_dir(tmp_path, lengths, mfcc_lengths=None):
    prefix = "speaker_1_state_0"
    base = tmp_path / prefix
    for sub in ("Rotation", "Wav") + (("MFCC",) if mfcc_lengths else ()):
        os.makedirs(base / sub)
    rng = np.random.default_rng(5)
    arrays = {}
    for name, n in lengths.items():
        poses = rng.standard_normal((n, 135))
        wav = rng.standard_normal(int(n / 60 * 16000) + 777).astype(np.float32)
        np.savez(base / "Rotation" / (name + ".npz"), upper=poses)
        np.savez(base / "Wav" / (name + ".npz"), wav=wav)
        arrays[name] = (poses, wav)
        if mfcc_lengths:
            np.savez(base / "MFCC" / (name + ".npz"), mfcc=rng.standard_normal((mfcc_lengths[name], 13)))
    return prefix, arrays


def test_make_dataset_windows_and_splits(tmp_path):
    from qpgesture_amd import process_bvh as P
    lengths = {"1_wayne_0_1_8": 100, "1_wayne_0_9_16": 47, "1_wayne_0_103_110": 61, "1_wayne_0_111_118": 24,
               "1_wayne_0_81_86": 90, "1_wayne_0_17_24": 23}
    prefix, arrays = _speaker_dir(tmp_path, lengths)
    for mode, stride in (("noduplication", 24), ("duplication", 5)):
        written = P.make_dataset(str(tmp_path), prefix, n_frames=24, fps=60, mode=mode, subdivision_stride=5)
        assert sorted(written) == ["test", "train", "validation"]
        want = {"train": ["1_wayne_0_17_24", "1_wayne_0_1_8", "1_wayne_0_9_16"], "test": ["1_wayne_0_103_110"],
                "validation": ["1_wayne_0_111_118"]}                        # sorted file order; 81_86 is skipped
        for split, names in want.items():
            path = str(tmp_path / prefix / ("%s_%s_%d.npz" % (prefix, split, stride)))
            assert written[split] == path
            z = np.load(path)
            assert sorted(z.files) == ["body", "wav"]
            body, wav = [], []
            for n in names:
                poses, w = arrays[n]
                count = (lengths[n] - 24) // stride + 1 if lengths[n] >= 24 else 0
                for i in range(count):
                    body.append(poses[i * stride:i * stride + 24])
                    a0 = int(np.floor(i * stride / 60 * 16000))
                    wav.append(w[:int(np.floor(lengths[n] / 60 * 16000))][a0:a0 + 6400])
            assert z["body"].shape == (len(body), 24, 135) and z["body"].dtype == np.float64
            assert np.array_equal(z["body"], np.array(body)) and np.array_equal(z["wav"], np.array(wav))
            assert z["wav"].shape == (len(body), 6400) and z["wav"].dtype == np.float32
    with pytest.raises(ValueError):
        P.make_dataset(str(tmp_path), prefix, mode="overlap")


def test_make_dataset_with_mfcc(tmp_path):
    """Where MFCC/ exists the reference's MINLEN = min(len(poses), len(mfcc)) cuts both, and `mfcc` is written."""
    from qpgesture_amd import process_bvh as P
    lengths = {"1_wayne_0_1_8": 100, "1_wayne_0_103_110": 61}
    prefix, arrays = _speaker_dir(tmp_path, lengths, mfcc_lengths={"1_wayne_0_1_8": 70, "1_wayne_0_103_110": 90})
    written = P.make_dataset(str(tmp_path), prefix, n_frames=24, mode="noduplication")
    z = np.load(written["train"])
    assert sorted(z.files) == ["body", "mfcc", "wav"]
    assert z["body"].shape == (2, 24, 135) and z["mfcc"].shape == (2, 24, 13)     # MINLEN 70, not 100: 2 windows, not 4
    assert np.array_equal(z["body"][1], arrays["1_wayne_0_1_8"][0][24:48])
    assert np.load(written["test"])["body"].shape == (2, 24, 135) and np.load(written["validation"])["body"].shape[0] == 0
    os.remove(tmp_path / prefix / "MFCC" / "1_wayne_0_1_8.npz")
    P.make_dataset(str(tmp_path), prefix, n_frames=24, mode="noduplication")        # a whole split without MFCC is fine
    os.rename(tmp_path / prefix / "Rotation" / "1_wayne_0_103_110.npz", tmp_path / prefix / "Rotation" / "1_wayne_0_2_3.npz")
    np.savez(tmp_path / prefix / "Wav" / "1_wayne_0_2_3.npz", wav=np.zeros(50000, np.float32))
    np.savez(tmp_path / prefix / "MFCC" / "1_wayne_0_2_3.npz", mfcc=np.zeros((90, 13)))
    with pytest.raises(ValueError, match="some recordings only"):
        P.make_dataset(str(tmp_path), prefix, n_frames=24, mode="noduplication")


def test_selected_files_and_stats_format(tmp_path):
    from qpgesture_amd import process_bvh as P
    os.makedirs(tmp_path / "Motion")
    for f in ("10_kieks_0_1_8.bvh", "10_kieks_1_1_8.bvh", "1_wayne_0_1_8.bvh", "10_kieks_0_9_16.bvh", "10_kieks_0_9_16.txt",
              "10_kieks_0_9.bvh"):
        open(tmp_path / "Motion" / f, "w").close()
    assert P.selected_files(str(tmp_path), "speaker_10_state_0") == ["10_kieks_0_1_8.bvh", "10_kieks_0_9_16.bvh"]
    assert P.format_stats(np.array([0.967764, -0.00000001]), np.array([0.5, 1e-5])) == ["[0.96776, -0.00000]",
                                                                                         "[0.50000, 0.00001]"]
    assert [P.split_of(p) for p in ("a/1_w_0_81_86.npz", "a/1_w_0_103_110.npz", "a/1_w_0_111_118.npz", "a/1_w_0_1_8.npz")] \
        == [None, "test", "validation", "train"]


def test_process_bvh_on_a_broken_file(tmp_path, capsys):
    """The reference's return shape: (None, None), here with the reason printed; 'position' is out of scope."""
    from qpgesture_amd import process_bvh as P
    path = str(tmp_path / "broken.bvh")
    with open(path, "w") as f:
        f.write(B.bvh_text(np.zeros((3, B.n_channels()))).replace("Frame Time:", "Frame Tempo:"))
    assert P.process_bvh(path, modetype="rotation", fps=60) == (None, None)
    assert "broken.bvh" in capsys.readouterr().out
    assert P.process_bvh(str(tmp_path / "absent.bvh"), modetype="rotation") == (None, None)
    with pytest.raises(NotImplementedError):
        P.process_bvh(path, modetype="position")


def test_step2_is_dispatched():
    import inspect
    from qpgesture_amd import make_beat_dataset, process_bvh as P
    assert "process_speaker" in inspect.getsource(make_beat_dataset.main)
    a = P.build_parser().parse_args(["--save_dir", "D", "--prefix", "speaker_2_state_1", "--gpu", "1", "--stats"])
    assert (a.save_dir, a.prefix, a.gpu, a.stats, a.n_frames) == ("D", "speaker_2_state_1", "1", True, 240)
