"""NumPy restatement of BVH ingestion (qpgesture_amd/process_bvh.py, csrc/qpg_bvh.hip): the tokenizer, the column
tables, the frame slicing, Euler -> matrix and the column statistics - the last two in f64 and in np.longdouble, the
yardstick the kernels' and the reference's own errors are measured against.  Independent of the package: nothing here
imports it.  Also the writer of the synthetic BVH files the tests and tests/golden/make_golden_bvh_features.py use."""
import re

import numpy as np

TARGET_JOINTS = ['Spine', 'Spine1', 'Spine2', 'Spine3', 'Neck', 'Neck1', 'Head',
                 'RightShoulder', 'RightArm', 'RightForeArm', 'RightHand',
                 'LeftShoulder', 'LeftArm', 'LeftForeArm', 'LeftHand']

# (name, parent) in file order: Hips, the 15 target joints, one finger per hand, legs; leaves get an End Site
SKELETON = [("Hips", None), ("Spine", "Hips"), ("Spine1", "Spine"), ("Spine2", "Spine1"), ("Spine3", "Spine2"),
            ("Neck", "Spine3"), ("Neck1", "Neck"), ("Head", "Neck1"),
            ("RightShoulder", "Spine3"), ("RightArm", "RightShoulder"), ("RightForeArm", "RightArm"),
            ("RightHand", "RightForeArm"), ("RightHandIndex1", "RightHand"),
            ("LeftShoulder", "Spine3"), ("LeftArm", "LeftShoulder"), ("LeftForeArm", "LeftArm"),
            ("LeftHand", "LeftForeArm"), ("LeftHandIndex1", "LeftHand"),
            ("RightUpLeg", "Hips"), ("RightLeg", "RightUpLeg"), ("RightFoot", "RightLeg"),
            ("LeftUpLeg", "Hips"), ("LeftLeg", "LeftUpLeg"), ("LeftFoot", "LeftLeg")]
UPPER_ONLY = SKELETON[:12] + SKELETON[13:17]             # Hips + the 15 target joints: the smallest usable file


def joint_order(skeleton=SKELETON):
    """Depth-first order of the joints, i.e. the order their channels take in the file."""
    kids = {n: [c for c, p in skeleton if p == n] for n, _ in skeleton}
    out = []

    def walk(n):
        out.append(n)
        for c in kids[n]:
            walk(c)
    walk([n for n, p in skeleton if p is None][0])
    return out


def bvh_text(values, order="ZXY", skeleton=SKELETON, frametime=1.0 / 120.0, fmt="%.6f", frames=None, newline="\n"):
    """A BVH file as a str.  values [F][6 + 3 (joints - 1)]: the root's 3 positions + 3 rotations, then 3 rotations per
    joint, in joint_order().  `order`: the rotation channels' order, e.g. 'ZXY' -> Zrotation Xrotation Yrotation."""
    kids = {n: [c for c, p in skeleton if p == n] for n, _ in skeleton}
    rot = " ".join("%srotation" % a for a in order)
    lines = ["HIERARCHY"]

    def emit(n, depth):
        ind = "  " * depth
        root = depth == 0
        lines.append("%s%s %s" % (ind, "ROOT" if root else "JOINT", n))
        lines.append(ind + "{")
        lines.append("%s  OFFSET %.6f %.6f %.6f" % (ind, 0.0, 0.0 if root else 10.5, 0.0 if root else -1.25))
        lines.append("%s  CHANNELS %s" % (ind, "6 Xposition Yposition Zposition " + rot if root else "3 " + rot))
        for c in kids[n]:
            emit(c, depth + 1)
        if not kids[n]:
            lines.extend([ind + "  End Site", ind + "  {", ind + "    OFFSET 0.000000 4.000000 0.000000", ind + "  }"])
        lines.append(ind + "}")
    emit(joint_order(skeleton)[0], 0)
    values = np.asarray(values, np.float64)
    lines += ["MOTION", "Frames: %d" % (values.shape[0] if frames is None else frames), "Frame Time: %.8f" % frametime]
    for row in values:
        lines.append(" ".join(fmt % v for v in row))
    return newline.join(lines) + newline


def n_channels(skeleton=SKELETON):
    return 6 + 3 * (len(skeleton) - 1)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def split_file(data):
    """bytes -> (header str, Frames, Frame Time, motion bytes)."""
    m = re.search(rb"MOTION\s+Frames\s*:\s*(\S+)\s+Frame\s+Time\s*:\s*(\S+)", data)
    return data[:m.start()].decode(), int(float(m.group(1))), float(m.group(2)), data[m.end():]


def channel_names(header):
    """[(joint, channel)] in file order; an End Site has no channels."""
    names, joint = [], None
    for line in header.splitlines():
        w = line.split()
        if w and w[0] in ("ROOT", "JOINT"):
            joint = w[1]
        elif w and w[0] == "CHANNELS":
            names.extend((joint, c) for c in w[2:2 + int(w[1])])
    return names


def tokens(motion):
    """Whitespace is space, tab, CR, LF; a token is a maximal run of other bytes."""
    return [t for t in re.split(rb"[ \t\r\n]+", motion) if t]


def parse_values(motion, n_values):
    """float() of the first n_values tokens, the rest is ignored (pymo/parsers.py:252-256)."""
    return np.array([float(t) for t in tokens(motion)[:n_values]], np.float64)


_NUMBER = re.compile(rb"([+-]?)(?:(\d+)(?:\.(\d*))?|\.(\d+))(?:[eE]([+-]?\d+))?")


def exact_value(token):
    """The parse kernel's exact path on one token (bytes): the significant digits as an integer m (at most 19 of them,
    m <= 2^53) and the net decimal exponent k in [-22, 22] give m * 10^k or m / 10^k - one correctly rounded f64
    operation on exact operands - with the sign applied by negation.  None: a well-formed token for the fallback list.
    ValueError: not in the grammar."""
    m = _NUMBER.fullmatch(token)
    if m is None or len(token) > 1024:
        raise ValueError(token)
    sign, ip, fp, fp2, ex = m.groups()
    ip, fp = ip or b"", (fp if fp2 is None else fp2) or b""
    digits = (ip + fp).lstrip(b"0")
    if len(digits) > 19:
        return None
    mant, k = int(digits or b"0"), int(ex or 0) - len(fp)
    if mant == 0:
        v = 0.0
    elif mant > 2 ** 53 or not -22 <= k <= 22:
        return None
    else:
        v = float(mant) * float(10 ** k) if k >= 0 else float(mant) / float(10 ** -k)
    return -v if sign == b"-" else v


def tables(names, joints=TARGET_JOINTS):
    """(col, mirror_col, mirror_sign) [J][3]: see process_bvh.rotation_tables."""
    pos = {"%s_%s" % jc: i for i, jc in reversed(list(enumerate(names)))}
    col, mcol, sign = [], [], []
    for j in joints:
        rots = [c for jj, c in names if jj == j and c.endswith("rotation")]
        p = j.replace("Left", "Right") if "Left" in j else j.replace("Right", "Left")
        col.append([pos["%s_%s" % (j, c)] for c in rots])
        mcol.append([pos["%s_%s" % (p, c)] for c in rots])
        sign.append([{"X": 1.0, "Y": -1.0, "Z": -1.0}[c[0]] for c in rots])
    return np.array(col, np.int32), np.array(mcol, np.int32), np.array(sign, np.float64)


def rows(F, rate):
    """DownSampler: values[0:-1:rate]."""
    return np.arange(F)[0:-1:rate]


def pi_of(dtype):
    return dtype(4) * np.arctan(dtype(1))


def euler_to_matrix(angles_deg, dtype=np.float64):
    """[..., 3] degrees -> [..., 9]: R = Rz(a0) Rx(a1) Ry(a2) row-major, scipy's intrinsic 'ZXY'."""
    a = np.asarray(angles_deg).astype(dtype) * (pi_of(dtype) / dtype(180))
    sz, cz = np.sin(a[..., 0]), np.cos(a[..., 0])
    sx, cx = np.sin(a[..., 1]), np.cos(a[..., 1])
    sy, cy = np.sin(a[..., 2]), np.cos(a[..., 2])
    return np.stack([cz * cy - sz * sx * sy, -sz * cx, cz * sy + sz * sx * cy,
                     sz * cy + cz * sx * sy, cz * cx, sz * sy - cz * sx * cy,
                     -cx * sy, sx, cx * cy], axis=-1)


def features(values, names, frametime, fps, joints=TARGET_JOINTS, dtype=np.float64):
    """(upper, upper_mirror) [T][9 J] of the channel table values [F][C]."""
    rate = round(1.0 / frametime) // fps
    col, mcol, sign = tables(names, joints)
    v = np.asarray(values)[rows(len(values), rate)]
    T = v.shape[0]
    up = euler_to_matrix(v[:, col], dtype).reshape(T, 9 * len(joints))
    um = euler_to_matrix(v[:, mcol] * sign, dtype).reshape(T, 9 * len(joints))
    return up, um


def file_features(data, fps, joints=TARGET_JOINTS, dtype=np.float64):
    header, F, ft, motion = split_file(data)
    names = channel_names(header)
    vals = parse_values(motion, F * len(names)).reshape(F, len(names))
    return features(vals, names, ft, fps, joints, dtype)


def column_stats(x, dtype=np.float64):
    """(mean, std) per column, two passes, ddof 0."""
    x = np.asarray(x).astype(dtype)
    mean = x.sum(axis=0) / dtype(x.shape[0])
    return mean, np.sqrt(((x - mean) ** 2).sum(axis=0) / dtype(x.shape[0]))


def planted_angles(rng, F, C, bound=170.0):
    """Angles uniform in +-bound, rounded to the file's 6 decimals, some planted at exactly 0, +-90, +-180."""
    v = np.round(rng.uniform(-bound, bound, size=(F, C)), 6)
    special = np.array([0.0, 90.0, -90.0, 180.0, -180.0, -0.0])
    idx = rng.choice(F * C, size=max(F * C // 12, 1), replace=False)
    v.reshape(-1)[idx] = special[rng.integers(0, len(special), size=idx.size)]
    return v
