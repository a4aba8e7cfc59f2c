#!/usr/bin/env python
"""BVH ingestion, measured (profiles/bvh_bench.md): a synthetic BEAT-sized recording - Hips plus 75 joints, 231 channels,
120 fps, `--seconds` long, %.6f text, written by this script - through qpgesture_amd/process_bvh.py, stage by stage:

    read      the file into host memory
    upload    the motion block's bytes to the device
    parse     qpg_bvh_parse_motion_f64 (five launches) + the host's look at the status
    features  qpg_bvh_rotation_f64 at 60 fps, both copies
    whole     bvh_to_rotation(path, fps=60): file -> two NumPy arrays

and, on the same machine, the baseline: numpy.loadtxt of the motion block + the f64 NumPy restatement of the features.
Wall clock around a device synchronise, median of --repeat calls after a warm-up.  Prints one JSON line.

    python tools/bench_bvh.py --seconds 60
    python tools/bench_bvh.py --reference <checkout> --seconds 5 --cpu-only     # the reference's own pipeline, once

--reference times process_bvh's pipeline of the reference (pymo parser, pandas pipeline, the scipy loop, assembled as in
tests/golden/make_golden_bvh_features.py) once on the same file; with --cpu-only nothing touches a GPU."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TARGET = ['Spine', 'Spine1', 'Spine2', 'Spine3', 'Neck', 'Neck1', 'Head', 'RightShoulder', 'RightArm', 'RightForeArm',
          'RightHand', 'LeftShoulder', 'LeftArm', 'LeftForeArm', 'LeftHand']


def skeleton():
    """(name, parent) x 76 in file order: Hips, the upper-body chain, 24 finger joints per hand, 2 x 4 leg joints."""
    sk = [("Hips", None), ("Spine", "Hips"), ("Spine1", "Spine"), ("Spine2", "Spine1"), ("Spine3", "Spine2"),
          ("Neck", "Spine3"), ("Neck1", "Neck"), ("Head", "Neck1"), ("HeadEnd", "Head"), ("Jaw", "Head")]
    for side in ("Right", "Left"):
        sk += [(side + "Shoulder", "Spine3"), (side + "Arm", side + "Shoulder"), (side + "ForeArm", side + "Arm"),
               (side + "ForeArmRoll", side + "ForeArm"), (side + "Hand", side + "ForeArmRoll")]
        for finger in ("Thumb", "Index", "Middle", "Ring", "Pinky"):
            parent = side + "Hand"
            for k in range(0 if finger != "Thumb" else 1, 5):           # (k = 0: the metacarpal)
                sk.append(("%sHand%s%d" % (side, finger, k), parent))
                parent = sk[-1][0]
    for side in ("Right", "Left"):
        sk += [(side + "UpLeg", "Hips"), (side + "Leg", side + "UpLeg"), (side + "Foot", side + "Leg"),
               (side + "ToeBase", side + "Foot")]
    assert len(sk) == 76
    return sk


def write_bvh(path, seconds, seed=0):
    sk = skeleton()
    kids = {n: [c for c, p in sk if p == n] for n, _ in sk}
    rot = "Zrotation Xrotation Yrotation"
    lines = ["HIERARCHY"]

    def emit(n, depth):
        ind = "  " * depth
        lines.extend(["%s%s %s" % (ind, "JOINT" if depth else "ROOT", n), ind + "{", ind + "  OFFSET 0.000000 9.500000 0.250000",
                      "%s  CHANNELS %s" % (ind, "3 " + rot if depth else "6 Xposition Yposition Zposition " + rot)])
        for c in kids[n]:
            emit(c, depth + 1)
        if not kids[n]:
            lines.extend([ind + "  End Site", ind + "  {", ind + "    OFFSET 0.000000 3.000000 0.000000", ind + "  }"])
        lines.append(ind + "}")
    emit("Hips", 0)
    F, C = int(round(seconds * 120)), 6 + 3 * (len(sk) - 1)
    lines += ["MOTION", "Frames: %d" % F, "Frame Time: 0.008333"]
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
        for f0 in range(0, F, 1200):
            v = rng.uniform(-170.0, 170.0, size=(min(1200, F - f0), C))
            f.write("".join(" ".join(["%.6f"] * C) % tuple(row) + "\n" for row in v))
    return F, C, len(lines)


def euler_to_matrix(a):
    a = np.deg2rad(a)
    sz, cz, sx, cx, sy, cy = np.sin(a[..., 0]), np.cos(a[..., 0]), np.sin(a[..., 1]), np.cos(a[..., 1]), np.sin(a[..., 2]), \
        np.cos(a[..., 2])
    return np.stack([cz * cy - sz * sx * sy, -sz * cx, cz * sy + sz * sx * cy, sz * cy + cz * sx * sy, cz * cx,
                     sz * sy - cz * sx * cy, -cx * sy, sx, cx * cy], axis=-1)


def numpy_baseline(path, header_lines, tables, rate):
    t0 = time.perf_counter()
    values = np.loadtxt(path, skiprows=header_lines, dtype=np.float64, ndmin=2)
    t1 = time.perf_counter()
    col, mcol, sign = tables
    v = values[0:-1:rate]
    up = euler_to_matrix(v[:, col]).reshape(len(v), -1)
    um = euler_to_matrix(v[:, mcol] * sign).reshape(len(v), -1)
    t2 = time.perf_counter()
    return values, up, um, t1 - t0, t2 - t1


def reference_pipeline(checkout, path, fps=60):
    import types
    sys.modules.setdefault("transforms3d", types.ModuleType("transforms3d"))
    sys.path.insert(0, os.path.join(checkout, "process"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import contextlib
    import io
    import make_golden_bvh_features as G
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        _, up, um = G.reference_features(path, fps, TARGET)
    return up, um, time.perf_counter() - t0


def median_time(fn, repeat, sync):
    fn()
    sync()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--reference", default=None, help="a checkout of the reference: time its own pipeline once")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--keep", default=None, help="write the synthetic file here instead of a temporary directory")
    args = ap.parse_args()
    tmp = tempfile.TemporaryDirectory()
    path = args.keep or os.path.join(tmp.name, "1_synthetic_0_1_1.bvh")
    t0 = time.perf_counter()
    F, C, header_lines = write_bvh(path, args.seconds)
    res = {"bench": "bvh", "seconds": args.seconds, "frames": F, "channels": C, "file_MB": round(os.path.getsize(path) / 1e6, 2),
           "write_s": round(time.perf_counter() - t0, 2)}
    if args.reference:
        up, um, t = reference_pipeline(args.reference, path)
        res["reference_process_bvh_60fps_s"] = round(t, 3)
        res["reference_shape"] = list(up.shape)
    if not args.cpu_only:
        import torch
        from qpgesture_amd import process_bvh as P
        assert torch.cuda.is_available(), "bench_bvh.py needs a GPU (or --cpu-only with --reference)"
        dev = torch.device("cuda:0")
        sync = torch.cuda.synchronize

        def read():
            with open(path, "rb") as f:
                return f.read()
        t_read, data = median_time(read, args.repeat, lambda: None)
        head, frames, ft, off = P.split_bvh(data)
        motion = np.frombuffer(data, np.uint8, offset=off)
        t_up, text = median_time(lambda: torch.from_numpy(motion.copy()).to(dev), args.repeat, sync)
        t_parse, parsed = median_time(lambda: P.parse_motion(motion, F * C, dev, text=text), args.repeat, sync)
        assert parsed[1] == F * C and parsed[2] == 0, parsed[1:]
        rec = P.read_bvh(path, device=dev)
        tables = P.rotation_tables(rec)
        t_feat, (up_d, um_d) = median_time(lambda: P.record_to_rotation(rec, 60, True, tables=tables), args.repeat, sync)
        t_whole, (up, um) = median_time(lambda: P.bvh_to_rotation(path, fps=60, device=dev), args.repeat, sync)
        t_stats, _ = median_time(lambda: P.pose_stats(up_d, dev), args.repeat, sync)
        res.update(read_ms=round(t_read * 1e3, 2), upload_ms=round(t_up * 1e3, 2), parse_ms=round(t_parse * 1e3, 2),
                   features_ms=round(t_feat * 1e3, 3), stats_ms=round(t_stats * 1e3, 3), whole_ms=round(t_whole * 1e3, 2),
                   parse_GBps=round(len(motion) / t_parse / 1e9, 2), out_frames=int(up.shape[0]))
        if not args.no_baseline:
            values, bu, bm, t_load, t_np = numpy_baseline(path, header_lines, tables, P.frame_rate(ft, 60))
            res.update(loadtxt_ms=round(t_load * 1e3, 1), numpy_features_ms=round(t_np * 1e3, 2),
                       baseline_ms=round((t_load + t_np) * 1e3, 1), ratio=round((t_load + t_np) / t_whole, 1),
                       values_equal=bool(np.array_equal(values.view(np.int64), rec.values.cpu().numpy().view(np.int64))),
                       max_abs_diff=float(max(np.abs(bu - up).max(), np.abs(bm - um).max())))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
