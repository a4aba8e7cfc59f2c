"""BVH ingestion on the device (csrc/qpg_bvh.hip through qpgesture_amd/process_bvh.py): the motion-text parser bit for bit
against Python's float(), the rotation features against the reference's own pymo + scipy output
(tests/golden/bvh_features_*.npz) and the longdouble restatement (tests/bvh_ref.py), the round trip through
qpg_pose_to_euler_f64, the column statistics against NumPy and longdouble, scratch independence, and the CLI.

Tolerances.  Parse: none, the bits of float().  Features and statistics: the kernel's maximum error against the longdouble
restatement may be at most 4 x the reference's own error against it (scipy goes through quaternions, NumPy sums row by
row); the margin covers the device's f64 sin / cos differing from the host's by an ulp or two.  Both sides are measured
and printed here; the figures of record are in DESIGN.md §4.17."""
import os

import numpy as np
import pytest

from tests import bvh_ref as B
from tests import poison
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDENS = ("bvh_features_zxy", "bvh_features_xyz")
BLOCK = 4096


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _raw_parse(data, n_values, cap=8, pattern=0x00):
    """qpg_bvh_parse_motion_f64 by hand: the text sits directly in front of a fence of non-whitespace bytes (a read past
    n_bytes would lengthen the last token), every output and the workspace are pre-filled with `pattern` between fences.
    Returns (values, info, fallback list rows actually listed)."""
    import torch
    from qpgesture_amd import _lib
    n = len(data)
    tg = poison.guarded(n, 0x20, tail=4096, device=DEV)
    if n:
        tg.buf.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    values, vg = poison.fenced((n_values,), torch.float64, pattern, device=DEV)
    fb, fg = poison.fenced((max(cap, 1), 2), torch.int64, pattern, device=DEV)
    info, ig = poison.fenced((3,), torch.int64, pattern, device=DEV)
    ws_bytes = int(_lib.load().qpg_bvh_parse_ws_bytes(n))
    assert ws_bytes % 8 == 0 and ws_bytes >= 32
    wg = poison.guarded(ws_bytes, pattern, device=DEV)
    _lib.call("qpg_bvh_parse_motion_f64", DEV, tg.buf, n, n_values, values, fb, cap, info, wg.buf, ws_bytes)
    torch.cuda.synchronize()
    for g, what in ((tg, "text"), (vg, "values"), (fg, "fallback list"), (ig, "info"), (wg, "workspace")):
        g.assert_tail_intact(what)
    assert bytes(tg.buf.cpu().numpy().tobytes()) == bytes(data)
    info = info.cpu().numpy()
    return values.cpu().numpy(), info, fb.cpu().numpy()[:min(int(info[1]), cap)]


def _want(data, n_values):
    return np.array([float(t) for t in data.split()[:n_values]], np.float64)


def _fixed_text(rng, n_tokens, per_line=7):
    """%.6f text of |x| < 10^4, a newline every per_line tokens."""
    v = rng.uniform(-9999.999999, 9999.999999, size=n_tokens)
    v[rng.integers(0, n_tokens, size=max(n_tokens // 10, 1))] = 0.0
    toks = ["%.6f" % x for x in v]
    return "".join(t + ("\n" if (i + 1) % per_line == 0 else " ") for i, t in enumerate(toks)).encode()


def _check_exact(data, n_values, fallbacks=0):
    want = _want(data, n_values)
    assert len(want) == n_values
    got, info, _ = _raw_parse(data, n_values)
    assert info.tolist() == [len(data.split()), fallbacks, 0]
    assert np.array_equal(_bits(got), _bits(want))
    return got


@pytest.mark.parametrize("F,C", [(1, 1), (3, 7), (41, 84), (158, 7)])
def test_parse_fixed_point_text_is_float_bit_for_bit(F, C):
    """(158 x 7: about three blocks of text.)  For %.6f text of |x| < 10^4 the integer-mantissa path alone must do: a
    fallback count of 0, so the host's float() cannot hide a broken kernel."""
    data = _fixed_text(np.random.default_rng(F * 100 + C), F * C, per_line=C)
    if (F, C) == (158, 7):
        assert 2.5 * BLOCK < len(data) < 3.5 * BLOCK
    _check_exact(data, F * C)
    _check_exact(data.rstrip(), F * C)                       # no trailing newline: the last token ends the text


def _text_of_length(rng, n_bytes):
    """Exactly n_bytes bytes, ending in a token (no trailing whitespace); the slack is a run of spaces after token 0."""
    toks = _fixed_text(rng, n_bytes // 8, per_line=5).split()
    text, k = b"", 0
    while len(text) + 1 + len(toks[k]) <= n_bytes - 8:
        text += (b" " if text else b"") + toks[k]
        k += 1
    head, _, rest = text.partition(b" ")
    text = head + b" " * (1 + n_bytes - len(text)) + rest
    assert len(text) == n_bytes and not text[-1:].isspace()
    return text


@pytest.mark.parametrize("n_bytes", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1])
def test_parse_text_lengths_around_a_block(n_bytes):
    data = _text_of_length(np.random.default_rng(n_bytes), n_bytes)
    _check_exact(data, len(data.split()))


@pytest.mark.parametrize("start", [BLOCK - 1, BLOCK, 2 * BLOCK - 1, BLOCK - 16, BLOCK - 3])
def test_parse_token_across_a_block_boundary(start):
    """A token whose first byte is the last byte of a block (or of a thread's 16 bytes) and that runs on into the next: the
    thread that owns the start reads on."""
    rng = np.random.default_rng(start)
    head = _text_of_length(rng, start - 1) + b" "
    data = head + b"-7123.250001 " + _fixed_text(rng, 40)
    assert data[start:start + 1] == b"-" and data[start - 1:start] == b" "
    got = _check_exact(data, len(data.split()))
    assert got[len(head.split())] == -7123.250001


def test_parse_whitespace_and_token_forms():
    data = b" \t\r\n  1.5\t-2.25\r\n3.0    4.0\n\n\t5.5 -0.000000 1e-05 -1.5E+2 .5 5. +.25 0 -0 007 1.e2 12345.678901e-3\r\n6.5"
    got = _check_exact(data, 17)
    assert got[5] == 0.0 and np.signbit(got[5]) and np.signbit(got[12]) and not np.signbit(got[11])
    assert got[6] == 1e-05 and got[7] == -150.0 and got[8] == 0.5 and got[9] == 5.0 and got[-1] == 6.5
    # pymo reads frames x channels tokens and ignores the rest: neither a later odd token nor a later bad one counts
    got, info, fb = _raw_parse(b"1.0 2.0 3.0 1e300 x", 3)
    assert info.tolist() == [5, 0, 0] and got.tolist() == [1.0, 2.0, 3.0] and len(fb) == 0
    # nothing at all
    for empty in (b"", b" \n\t "):
        assert _raw_parse(empty, 0)[1].tolist() == [0, 0, 0]


LONG = [b"0.12345678901234567890123", b"1e300", b"-123456789012345678901", b"1e-300", b"9007199254740993", b"1e23",
        b"-2.5e-23", b"0.000000000000000000000001", b"179769313486231570000e290"]


def test_parse_fallback_tokens_are_listed_and_patched():
    """k planted tokens the exact path cannot take (20+ digits, a mantissa above 2^53, exponents outside +-22): the fallback
    count is exactly k, the list names them in token order with their byte offsets, their slots hold the placeholder, and
    the host's patched result is float() bit for bit."""
    from qpgesture_amd import _lib, process_bvh as P
    rng = np.random.default_rng(9)
    toks = _fixed_text(rng, 900).split()
    where = sorted(rng.choice(len(toks), size=len(LONG), replace=False).tolist())
    where[0], where[-1] = 0, len(toks) - 1
    for w, t in zip(where, LONG):
        toks[w] = t
    data = b" ".join(toks)
    assert len(data) > 2 * BLOCK
    want = _want(data, len(toks))
    got, info, fb = _raw_parse(data, len(toks), cap=16)
    assert info.tolist() == [len(toks), len(LONG), 0]
    assert fb[:, 0].tolist() == where
    for (idx, off), t in zip(fb.tolist(), LONG):
        assert data[off:off + len(t)] == t and (off == 0 or data[off - 1:off] == b" ")
    mask = np.zeros(len(toks), bool)
    mask[where] = True
    assert np.array_equal(_bits(got[~mask]), _bits(want[~mask]))
    assert (_bits(got[mask]) == _lib.QPG_BVH_PLACEHOLDER_BITS).all()
    vals, n_tokens, n_fb = P.parse_motion(data, len(toks), DEV)
    assert (n_tokens, n_fb) == (len(toks), len(LONG)) and np.array_equal(_bits(vals.cpu().numpy()), _bits(want))
    # list overflow: the bit, the true count, the first rows; the host then parses the whole block on the CPU
    got2, info2, fb2 = _raw_parse(data, len(toks), cap=2)
    assert info2.tolist() == [len(toks), len(LONG), _lib.QPG_BVH_ST_OVERFLOW] and fb2[:, 0].tolist() == where[:2]
    assert np.array_equal(_bits(got2), _bits(got))
    vals, _, _ = P.parse_motion(data, len(toks), DEV, fb_capacity=2)
    assert np.array_equal(_bits(vals.cpu().numpy()), _bits(want))


@pytest.mark.parametrize("bad", [b"abc", b"1.5.2", b"--1", b"1e", b"-", b".", b"1e+", b"0x10", b"1,5", b"nan", b"1" * 1025])
def test_parse_bad_byte_status(bad):
    """Status returns, not faults; the other tokens keep their values."""
    from qpgesture_amd import _lib, process_bvh as P
    data = b"1.5 " + bad + b" 2.5\n"
    got, info, _ = _raw_parse(data, 3)
    assert info.tolist() == [3, 0, _lib.QPG_BVH_ST_BADBYTE] and got[0] == 1.5 and got[2] == 2.5
    assert _bits(got[1:2])[0] == _lib.QPG_BVH_PLACEHOLDER_BITS
    assert _raw_parse(b"1.5 2.5 " + bad, 3)[1][2] == _lib.QPG_BVH_ST_BADBYTE            # at the very end of the text
    with pytest.raises(ValueError, match="not a number"):
        P.parse_motion(data, 3, DEV)


def test_parse_too_few_tokens_status(tmp_path):
    from qpgesture_amd import _lib, process_bvh as P
    data = _fixed_text(np.random.default_rng(4), 20)
    got, info, _ = _raw_parse(data, 21)
    assert info.tolist() == [20, 0, _lib.QPG_BVH_ST_SHORT] and np.array_equal(_bits(got[:20]), _bits(_want(data, 20)))
    # read_bvh: frames='header' refuses the file, frames='count' reads the whole frames that are there
    values = np.round(np.random.default_rng(5).uniform(-170, 170, size=(9, B.n_channels(B.UPPER_ONLY))), 6)
    text = B.bvh_text(values, skeleton=B.UPPER_ONLY, frames=12).encode()
    path = str(tmp_path / "short.bvh")
    with open(path, "wb") as f:
        f.write(text[:-30])                                  # the header says 12 frames; 8 whole frames and a part
    with pytest.raises(ValueError, match="8 whole frames"):
        P.read_bvh(path, device=DEV)
    assert P.process_bvh(path, modetype="rotation", fps=60) == (None, None)
    rec = P.read_bvh(path, frames="count", device=DEV)
    assert rec.header_frames == 12 and rec.values.shape == (8, 51)
    assert np.array_equal(_bits(rec.values.cpu().numpy()), _bits(values[:8]))


# ---- features -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_error():
    """The reference's own maximum error against the longdouble restatement, over both goldens and both rates."""
    e = 0.0
    for name in GOLDENS:
        g = load_golden(name)
        for fps in (60, 20):
            upl, uml = B.file_features(g["bvh"].tobytes(), fps, dtype=np.longdouble)
            e = max(e, float(np.abs(g["upper_%d" % fps] - upl).max()), float(np.abs(g["upper_mirror_%d" % fps] - uml).max()))
    assert 1e-16 < e < 1e-15
    return e


def _write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


@pytest.mark.parametrize("name", GOLDENS)
def test_features_vs_reference_golden(name, tmp_path, reference_error):
    from qpgesture_amd import process_bvh as P
    g = load_golden(name)
    data = g["bvh"].tobytes()
    path = _write(tmp_path, name + ".bvh", data)
    rec = P.read_bvh(path, device=DEV)
    assert np.array_equal(_bits(rec.values.cpu().numpy()), _bits(g["values"])) and rec.n_tokens == 41 * 75
    assert abs(rec.frametime - 1 / 120.0) < 1e-8 and rec.root_name == "Hips" and len(rec.channel_names) == 75
    for fps, T in ((60, 20), (20, 7)):
        up, um = P.bvh_to_rotation(path, fps=fps, device=DEV)
        upl, uml = B.file_features(data, fps, dtype=np.longdouble)
        for got, ld, want, what in ((up, upl, g["upper_%d" % fps], "upper"), (um, uml, g["upper_mirror_%d" % fps], "mirror")):
            assert got.shape == (T, 135) and got.dtype == np.float64
            e_ref, e_got = float(np.abs(want - ld).max()), float(np.abs(got - ld).max())
            print("%s %d fps %s: reference vs longdouble %.3e, kernel vs longdouble %.3e" % (name, fps, what, e_ref, e_got))
            assert e_got <= 4 * e_ref and e_got <= 4 * reference_error
            assert np.abs(got - want).max() <= e_got + e_ref
        only, none = P.bvh_to_rotation(path, fps=fps, mirror=False, device=DEV)
        assert none is None and np.array_equal(_bits(only), _bits(up))
    assert P.process_bvh(path, modetype="rotation", fps=20)[1].shape == (7, 135)


@pytest.mark.parametrize("F", [1, 2, 3])
def test_features_edge_rows_and_one_joint(F, tmp_path, reference_error):
    """F = 1 gives no row at all, F = 2 and 3 one or two: values[0:-1:rate] always drops the last frame.  J = 1."""
    from qpgesture_amd import process_bvh as P
    values = B.planted_angles(np.random.default_rng(F), F, B.n_channels())
    data = B.bvh_text(values, order="ZXY").encode()
    path = _write(tmp_path, "edge.bvh", data)
    for fps, rate in ((120, 1), (60, 2), (20, 6)):
        T = len(range(0, F - 1, rate))
        for joints in (B.TARGET_JOINTS, ["LeftArm"]):
            up, um = P.bvh_to_rotation(path, fps=fps, device=DEV, joints=joints)
            upl, uml = B.file_features(data, fps, joints=joints, dtype=np.longdouble)
            assert up.shape == um.shape == upl.shape == (T, 9 * len(joints))
            if T:
                assert np.abs(up - upl).max() <= 4 * reference_error and np.abs(um - uml).max() <= 4 * reference_error


def test_round_trip_through_pose_to_euler(tmp_path):
    """bvh -> upper -> normalise -> qpg_pose_to_euler_f64 gives the file's angles back, to that kernel's 1e-4 degrees; the
    X angle (the middle one of 'ZXY') stays inside +-80 degrees, away from gimbal lock."""
    from qpgesture_amd import bvh, process_bvh as P
    rng = np.random.default_rng(77)
    F, C = 62, B.n_channels(B.UPPER_ONLY)
    values = np.round(rng.uniform(-170, 170, size=(F, C)), 6)
    values[:, 7::3] = np.round(rng.uniform(-80, 80, size=(F, 15)), 6)          # Xrotation of the 15 joints
    path = _write(tmp_path, "rt.bvh", B.bvh_text(values, order="ZXY", skeleton=B.UPPER_ONLY).encode())
    upper, _ = P.bvh_to_rotation(path, fps=120, device=DEV)
    assert upper.shape == (F - 1, 135)
    mean, std = P.pose_stats(upper, DEV)
    poses_n = ((upper - mean) / np.clip(std, a_min=0.01, a_max=None)).astype(np.float32)
    euler = bvh.poses_to_euler(poses_n, mean, std, device=DEV)
    order = B.joint_order(B.UPPER_ONLY)
    cols = np.concatenate([6 + 3 * (order.index(j) - 1) + np.arange(3) for j in B.TARGET_JOINTS])
    d = np.abs(euler - values[:F - 1, cols])
    d = np.minimum(d, 360.0 - d)
    print("round trip: max %.3e degrees" % d.max())
    assert d.max() < 1e-4


# ---- statistics ---------------------------------------------------------------------------------------------------------
def _stats_data(N, D=135, seed=3):
    rng = np.random.default_rng(seed + N)
    x = rng.standard_normal((N, D)) * rng.uniform(0.01, 0.9, size=D) + rng.uniform(-1, 1, size=D)
    x[:, 64] = 0.1                                           # constant (N x 0.1 does not always sum to N times 0.1)
    x[:, 100] = 1.0 + 1e-5 * rng.standard_normal(N)          # mean 1, spread 1e-5: the reference's data_std has such columns
    return x


@pytest.mark.parametrize("N", [1, 2, 1000])
def test_column_stats(N):
    from qpgesture_amd import process_bvh as P
    x = _stats_data(N)
    mean, std = P.pose_stats(x, DEV)
    assert mean.shape == std.shape == (135,) and mean.dtype == std.dtype == np.float64
    ml, sl = B.column_stats(x, np.longdouble)
    e_np = (float(np.abs(np.mean(x, axis=0) - ml).max()), float(np.abs(np.std(x, axis=0) - sl).max()))
    e_got = (float(np.abs(mean - ml).max()), float(np.abs(std - sl).max()))
    print("N = %d: NumPy vs longdouble mean %.3e std %.3e, kernel vs longdouble mean %.3e std %.3e" % (N, *e_np, *e_got))
    assert mean[64] == 0.1 and std[64] == 0.0 and not np.signbit(std[64])
    assert e_got[0] <= 4 * e_np[0] and e_got[1] <= 4 * e_np[1]
    if N == 1000:
        assert abs(std[100] / 1e-5 - 1) < 0.2                # the tight column keeps its spread: no cancellation
    if N == 1:
        assert np.array_equal(_bits(mean), _bits(x[0])) and not std.any()
    # a list of arrays is their concatenation
    if N == 1000:
        m2, s2 = P.pose_stats([x[:333], x[333:]], DEV)
        assert np.array_equal(_bits(m2), _bits(mean)) and np.array_equal(_bits(s2), _bits(std))
        assert P.format_stats(mean, std)[0].startswith("[") and len(P.format_stats(mean, std)[1].split(", ")) == 135


# ---- scratch ------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_scratch(tmp_path):
    """Each kernel gives the same bits whatever its workspace and its not-yet-written outputs held (tests/poison.py)."""
    import torch
    from qpgesture_amd import _lib, process_bvh as P
    rng = np.random.default_rng(21)
    toks = _fixed_text(rng, 1200).split()
    toks[3], toks[700], toks[1199] = LONG[0], LONG[1], LONG[2]
    data = b"\n".join(toks)
    parsed, feats, stats = {}, {}, {}
    g = load_golden(GOLDENS[0])
    values = torch.from_numpy(g["values"]).to(DEV)
    names = B.channel_names(B.split_file(g["bvh"].tobytes())[0])
    tabs = [torch.from_numpy(t).to(DEV) for t in B.tables(names)]
    x = torch.from_numpy(_stats_data(700)).to(DEV)
    n_ws = int(_lib.load().qpg_column_stats_ws_doubles(700, 135))
    for label, pattern in poison.FILLS.items():
        v, info, fb = _raw_parse(data, 1200, cap=4, pattern=pattern)
        parsed[label] = (_bits(v).tobytes(), info.tobytes(), fb.tobytes())
        up, ug = poison.fenced((20, 135), torch.float64, pattern, device=DEV)
        um, mg = poison.fenced((20, 135), torch.float64, pattern, device=DEV)
        _lib.call("qpg_bvh_rotation_f64", DEV, values, 41, 75, 2, 20, 15, tabs[0], tabs[1], tabs[2], up, um)
        ug.assert_tail_intact("upper")
        mg.assert_tail_intact("upper_mirror")
        feats[label] = (up.cpu().numpy().tobytes(), um.cpu().numpy().tobytes())
        mean, eg = poison.fenced((135,), torch.float64, pattern, device=DEV)
        std, sg = poison.fenced((135,), torch.float64, pattern, device=DEV)
        wg = poison.guarded(n_ws * 8, pattern, device=DEV)
        _lib.call("qpg_column_stats_f64", DEV, x, 700, 135, mean, std, wg.buf, n_ws)
        for gd in (eg, sg, wg):
            gd.assert_tail_intact("column stats")
        stats[label] = (mean.cpu().numpy().tobytes(), std.cpu().numpy().tobytes())
    for results in (parsed, feats, stats):
        assert all(r == results["zeros_00"] for r in results.values())
    assert np.array_equal(np.frombuffer(feats["zeros_00"][0], np.float64).reshape(20, 135),
                          P.record_to_rotation(P.BVHRecord(values, names, None, 1 / 120.0, "Hips", 41, 41 * 75), 60,
                                               tables=B.tables(names))[0].cpu().numpy())


def test_entry_points_refuse_bad_arguments():
    import torch
    from qpgesture_amd import _lib
    v = torch.zeros((4, 6), dtype=torch.float64, device=DEV)
    t = torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    s = torch.ones((1, 3), dtype=torch.float64, device=DEV)
    out = torch.zeros((4, 9), dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="outside"):                      # row (T - 1) * rate = 4 of 4 frames
        _lib.call("qpg_bvh_rotation_f64", DEV, v, 4, 6, 2, 3, 1, t, t, s, out, None)
    with pytest.raises(RuntimeError, match="mirror"):
        _lib.call("qpg_bvh_rotation_f64", DEV, v, 4, 6, 1, 3, 1, t, None, None, out, out)
    ws = torch.zeros((8,), dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="ws_doubles"):
        _lib.call("qpg_column_stats_f64", DEV, v, 4, 6, out, out, ws, 8)
    text = torch.full((64,), 0x31, dtype=torch.uint8, device=DEV)
    info = torch.zeros((3,), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.call("qpg_bvh_parse_motion_f64", DEV, text[1:], 63, 1, v, None, 0, info, ws, 64)
    with pytest.raises(RuntimeError, match="ws_bytes"):
        _lib.call("qpg_bvh_parse_motion_f64", DEV, text, 64, 1, v, None, 0, info, ws, 8)


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, capsys):
    """Two tiny BVH files plus Wav/: the written names, keys, shapes and dtypes, and `body` = bvh_to_rotation's windows."""
    from qpgesture_amd import make_beat_dataset, process_bvh as P
    rng = np.random.default_rng(31)
    prefix, frames = "speaker_1_state_0", {"1_wayne_0_1_8": 101, "1_wayne_0_103_110": 61}
    os.makedirs(tmp_path / "Motion")
    os.makedirs(tmp_path / prefix / "Wav")
    C = B.n_channels(B.UPPER_ONLY)
    for name, F in frames.items():
        values = np.round(rng.uniform(-170, 170, size=(F, C)), 6)
        _write(tmp_path / "Motion", name + ".bvh", B.bvh_text(values, skeleton=B.UPPER_ONLY).encode())
        np.savez(tmp_path / prefix / "Wav" / (name + ".npz"), wav=rng.standard_normal(16000).astype(np.float32))
    _write(tmp_path / "Motion", "2_scott_0_1_8.bvh", b"another speaker's file is not even opened")
    written = P.main(["--save_dir", str(tmp_path), "--prefix", prefix, "--gpu", "0", "--stats", "--n_frames", "24"])
    out = capsys.readouterr().out.splitlines()
    assert [os.path.basename(w) for w in written] == ["1_wayne_0_103_110.npz", "1_wayne_0_1_8.npz"]
    ups = {}
    for name, F in frames.items():
        for sub, fps, T in (("Rotation", 60, (F - 1) // 2), ("Rotation_20fps", 20, len(range(0, F - 1, 6)))):
            z = np.load(tmp_path / prefix / sub / (name + ".npz"))
            assert z.files == ["upper"] and z["upper"].shape == (T, 135) and z["upper"].dtype == np.float64
            want = P.bvh_to_rotation(str(tmp_path / "Motion" / (name + ".bvh")), fps=fps, device=DEV)[0]
            assert np.array_equal(_bits(z["upper"]), _bits(want))
        ups[name] = np.load(tmp_path / prefix / "Rotation" / (name + ".npz"))["upper"]
    for split, name, n in (("train", "1_wayne_0_1_8", 2), ("test", "1_wayne_0_103_110", 1)):
        z = np.load(tmp_path / prefix / ("%s_%s_24.npz" % (prefix, split)))
        assert sorted(z.files) == ["body", "wav"] and z["body"].shape == (n, 24, 135) and z["body"].dtype == np.float64
        assert z["wav"].shape == (n, 6400) and z["wav"].dtype == np.float32
        assert np.array_equal(z["body"], ups[name][:24 * n].reshape(n, 24, 135))
    assert np.load(tmp_path / prefix / ("%s_validation_24.npz" % prefix))["body"].shape[0] == 0
    i = out.index("data mean/std")
    mean, std = P.pose_stats([ups["1_wayne_0_103_110"], ups["1_wayne_0_1_8"]], DEV)
    assert out[i + 1:i + 3] == P.format_stats(mean, std)
    # make_beat_dataset --step 2 is the same call (its windows are 240 frames: none from files this short)
    os.remove(tmp_path / prefix / "Rotation" / "1_wayne_0_1_8.npz")
    make_beat_dataset.main(["--save_dir", str(tmp_path), "--prefix", prefix, "--gpu", "0", "--step", "2"])
    assert np.array_equal(np.load(tmp_path / prefix / "Rotation" / "1_wayne_0_1_8.npz")["upper"], ups["1_wayne_0_1_8"])
    assert np.load(tmp_path / prefix / ("%s_train_240.npz" % prefix))["body"].shape[0] == 0
