"""BVH ingestion: a recorded `.bvh` file -> the `upper` rotation array (T, 135) f64 that is
`Rotation/<name>.npz`, the `body` column of every dataset file - process_bvh(..., modetype='rotation') of the reference's
process/beat_data_to_lmdb.py:21-88, and step 2 of its process/make_beat_dataset.py (:99-258) as far as motion goes.

    upper, upper_mirror = bvh_to_rotation("1_wayne_0_1_8.bvh", fps=60)          # (T, 135) f64 each
    mean, std = pose_stats([upper], "cuda:0")                                     # codebook.yml's data_mean / data_std
    python -m qpgesture_amd.process_bvh --save_dir ../dataset/BEAT --prefix speaker_10_state_0 --gpu 0 --stats

The reference goes through `pymo` (a regex tokenizer and one Python float() per token), a pandas pipeline (DownSampler,
RootTransformer('hip_centric'), Mirror('X'), JointSelector, ConstantsRemover, Numpyfier) and one scipy
Rotation.from_euler('ZXY') call per frame.  Here the hierarchy - a few hundred lines of text - is parsed in plain Python,
and everything that scales with the recording runs on the device (csrc/qpg_bvh.hip):
    qpg_bvh_parse_motion_f64   the motion block's bytes -> the channel table [F][C] f64, bit for bit Python's float()
    qpg_bvh_rotation_f64       down-sampling, joint selection, mirroring and Euler -> matrix in one launch
    qpg_column_stats_f64       np.mean / np.std over all frames (the `data mean/std` lines)
The pandas pipeline reduces to three small tables (rotation_tables): which column feeds which angle, which column feeds
the mirrored angle, and with which sign.

Deviations from the reference, all documented in INTEGRATION.md:
  * joints are matched by their EXACT name; the reference's JointSelector takes every column that CONTAINS `<name>_`
    (the same columns for BEAT's skeleton, where no joint name is the tail of another);
  * a file that holds fewer frames than its header says raises ValueError (process_bvh: (None, None), like the
    reference); frames='count' reads the frames that are there instead of rewriting the file (remake_beat_bvh);
  * make_dataset writes `mfcc` only where MFCC/<name>.npz exists (MFCC extraction is not part of this project);
  * failures name their reason (the reference's bare `except` returns (None, None) for all of them).
Out of scope: modetype='position' (forward kinematics), pymo's inverse pipeline and BVHWriter, audio and transcripts."""
import argparse
import collections
import glob
import math
import os
import re
import warnings

import numpy as np
import torch

from . import _lib
from .bvh import TARGET_JOINTS

ROTATIONS = ("Xrotation", "Yrotation", "Zrotation")
MIRROR_SIGN = {"X": 1.0, "Y": -1.0, "Z": -1.0}          # pymo Mirror(axis='X'), preprocessing.py:501-502
FALLBACK_CAPACITY = 4096
_WS = b" \t\r\n"

# values: device f64 [F][C]; channel_names: [(joint, channel)] in file order; skeleton: {joint: {'parent', 'channels',
# 'offsets', 'order', 'children'}} in file order, end sites as '<parent>_Nub' (pymo's names and fields)
BVHRecord = collections.namedtuple("BVHRecord", "values channel_names skeleton frametime root_name header_frames n_tokens")

_MOTION_RE = re.compile(rb"MOTION\s+Frames\s*:\s*(\S+)\s+Frame\s+Time\s*:\s*(\S+)")


def parse_hierarchy(text):
    """The HIERARCHY section of a BVH file (str).  Returns (skeleton, channel_names, root_name) as pymo's BVHParser
    builds them (pymo/parsers.py:106-214)."""
    tok = text.replace("{", " { ").replace("}", " } ").split()
    if len(tok) < 3 or tok[0] != "HIERARCHY" or tok[1] != "ROOT":
        raise ValueError("not a BVH hierarchy: it starts with %r" % " ".join(tok[:2]))
    skeleton, channel_names, stack = {}, [], []
    root_name = tok[2]
    i = 1
    while i < len(tok):
        t = tok[i]
        if t in ("ROOT", "JOINT", "End"):
            parent = stack[-1] if stack else None
            name = parent + "_Nub" if t == "End" else tok[i + 1]
            if i + 2 >= len(tok) or tok[i + 2] != "{":
                raise ValueError("BVH hierarchy: expected '{' after %s %s" % (t, tok[i + 1]))
            if name in skeleton:
                raise ValueError("BVH hierarchy: joint %r appears twice" % name)
            skeleton[name] = {"parent": parent, "channels": [], "offsets": [], "order": "", "children": []}
            if parent is not None:
                skeleton[parent]["children"].append(name)
            stack.append(name)
            i += 3
        elif t == "OFFSET":
            skeleton[stack[-1]]["offsets"] = [float(v) for v in tok[i + 1:i + 4]]
            i += 4
        elif t == "CHANNELS":
            n = int(tok[i + 1])
            chans = tok[i + 2:i + 2 + n]
            if len(chans) != n:
                raise ValueError("BVH hierarchy: CHANNELS %d of %s is cut short" % (n, stack[-1]))
            order = ""
            for c in chans:                              # (pymo/parsers.py:141-144: reset by a non-rotation channel)
                order = order + c[0] if c in ROTATIONS else ""
            skeleton[stack[-1]]["channels"] = chans
            skeleton[stack[-1]]["order"] = order
            channel_names.extend((stack[-1], c) for c in chans)
            i += 2 + n
        elif t == "}":
            if not stack:
                raise ValueError("BVH hierarchy: unbalanced '}'")
            stack.pop()
            i += 1
        else:
            raise ValueError("BVH hierarchy: unexpected token %r" % t)
    if stack:
        raise ValueError("BVH hierarchy: unbalanced '{'")
    return skeleton, channel_names, root_name


def split_bvh(data):
    """bytes of a whole BVH file -> (hierarchy text, header frame count, frame time, offset of the motion block)."""
    m = _MOTION_RE.search(data)
    if m is None:
        raise ValueError("no MOTION / Frames: / Frame Time: header")
    try:
        frames = int(float(m.group(1)))                  # (pymo/parsers.py:228)
        frametime = float(m.group(2))
    except ValueError:
        raise ValueError("unreadable Frames / Frame Time: %r, %r" % (m.group(1), m.group(2)))
    return data[:m.start()].decode("ascii", errors="replace"), frames, frametime, m.end()


def _token_at(data, off):
    end = off
    while end < len(data) and data[end] not in _WS:
        end += 1
    return bytes(data[off:end]).decode("ascii")


def parse_motion(data, n_values, device="cuda:0", fb_capacity=FALLBACK_CAPACITY, text=None):
    """The motion block `data` (bytes or a u8 array) through qpg_bvh_parse_motion_f64: the first n_values tokens as a device
    f64 tensor [n_values].  Returns (values, n_tokens, n_fallback).  `text`: the same bytes already on the device.
    Tokens the kernel cannot convert exactly (more than 19 digits, an exponent outside +-22) come back as a list and are
    parsed here with float() and patched in; if the list overflows, the whole block is parsed on the CPU.  A byte that
    fits no token raises ValueError.  n_tokens < n_values is the caller's to judge: the values are then incomplete."""
    dev = torch.device(device)
    host = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8)
    if text is None:
        text = torch.from_numpy(host.copy() if not host.flags.writeable else host).to(dev)
    n = int(text.numel())
    values = torch.empty((int(n_values),), dtype=torch.float64, device=dev)
    fb = torch.empty((max(int(fb_capacity), 1), 2), dtype=torch.int64, device=dev)
    info = torch.empty((3,), dtype=torch.int64, device=dev)
    ws_bytes = int(_lib.load().qpg_bvh_parse_ws_bytes(n))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
    _lib.call("qpg_bvh_parse_motion_f64", dev, text if n else None, n, int(n_values), values if n_values else None, fb,
              int(fb_capacity), info, ws, ws_bytes)
    n_tokens, n_fb, status = (int(v) for v in info.cpu().tolist())
    if status & _lib.QPG_BVH_ST_BADBYTE:
        raise ValueError("the motion block holds a token that is not a number")
    if status & _lib.QPG_BVH_ST_OVERFLOW:
        # cannot be silently unguarded: more odd tokens than the list holds -> every token through float(), on the CPU
        toks = host.tobytes().split()[:int(n_values)]
        vals = np.array([float(t) for t in toks], np.float64)
        values[:len(vals)] = torch.from_numpy(vals).to(dev)
        return values, n_tokens, n_fb
    if n_fb:
        lst = fb[:n_fb].cpu().numpy()
        vals = np.array([float(_token_at(host, int(off))) for off in lst[:, 1]], np.float64)
        values[torch.from_numpy(lst[:, 0].copy()).to(dev)] = torch.from_numpy(vals).to(dev)
    return values, n_tokens, n_fb


def read_bvh(path, frames="header", device="cuda:0"):
    """Read a BVH file: the hierarchy in Python, the motion block on the device.  frames='header': the file must hold the
    header's `Frames:` x channels tokens (ValueError otherwise - the case the reference's remake_beat_bvh rewrites the
    file for); frames='count': as many whole frames as the block holds, n_tokens // channels."""
    if frames not in ("header", "count"):
        raise ValueError("frames must be 'header' or 'count'")
    with open(path, "rb") as f:
        data = bytearray(os.fstat(f.fileno()).st_size)       # (writable: the upload below needs no second host copy)
        del data[f.readinto(data):]
    head, header_frames, frametime, off = split_bvh(data)
    skeleton, channel_names, root_name = parse_hierarchy(head)
    C = len(channel_names)
    if C == 0:
        raise ValueError("%s: no channels" % path)
    motion = np.frombuffer(data, np.uint8, offset=off)
    dev = torch.device(device)
    text = torch.from_numpy(motion).to(dev)
    if frames == "count":
        _, n_tokens, _ = parse_motion(motion, 0, dev, text=text)
        F = n_tokens // C
    else:
        F = header_frames
    if F < 0:
        raise ValueError("%s: Frames: %d" % (path, F))
    values, n_tokens, _ = parse_motion(motion, F * C, dev, text=text)
    if n_tokens < F * C:
        raise ValueError("%s: the header promises %d frames x %d channels, the file holds %d values (%d whole frames)"
                         % (path, F, C, n_tokens, n_tokens // C))
    return BVHRecord(values.view(F, C), channel_names, skeleton, frametime, root_name, header_frames, n_tokens)


def rotation_tables(record, joints=TARGET_JOINTS):
    """(col, mirror_col, mirror_sign), each [J][3], from names alone - what DownSampler .. Numpyfier of the reference's
    pipeline amount to for the selected joints:
      col[j][k]          position, in file order, of `<joint j>_<its k-th rotation channel>`; the joint is matched by its
                         EXACT name (the reference's JointSelector matches `(name + '_') in column`);
      mirror_col[j][k]   the same channel of the mirror partner: Left <-> Right in the name, else the joint itself;
      mirror_sign[j][k]  by the channel's name: X +1, Y -1, Z -1 (Mirror(axis='X')).
    ValueError when a selected joint is missing, lacks three rotation channels, or its partner (or the partner's channel)
    is missing - the reference returns (None, None) through a bare `except` for each of these."""
    pos = {}
    for i, (j, c) in enumerate(record.channel_names):
        pos.setdefault("%s_%s" % (j, c), i)
    J = len(joints)
    col, mcol = np.zeros((J, 3), np.int32), np.zeros((J, 3), np.int32)
    sign = np.zeros((J, 3), np.float64)
    for n, joint in enumerate(joints):
        if joint not in record.skeleton:
            raise ValueError("joint %r is not in the file" % joint)
        rots = [c for c in record.skeleton[joint]["channels"] if c in ROTATIONS]
        if len(rots) != 3 or len(set(rots)) != 3:
            raise ValueError("joint %r has rotation channels %r, not three" % (joint, rots))
        if "Left" in joint:
            partner = joint.replace("Left", "Right")
        elif "Right" in joint:
            partner = joint.replace("Right", "Left")
        else:
            partner = joint
        if partner not in record.skeleton:
            raise ValueError("joint %r has no mirror partner %r in the file" % (joint, partner))
        for k, c in enumerate(rots):
            if "%s_%s" % (partner, c) not in pos:
                raise ValueError("mirror partner %r of %r has no %s channel" % (partner, joint, c))
            col[n, k] = pos["%s_%s" % (joint, c)]
            mcol[n, k] = pos["%s_%s" % (partner, c)]
            sign[n, k] = MIRROR_SIGN[c[0]]
    return col, mcol, sign


def frame_rate(frametime, fps):
    """DownSampler's rate (pymo/preprocessing.py:1096-1099): round(1 / frametime) // fps; warns when it does not divide."""
    if not frametime > 0:
        raise ValueError("Frame Time %r" % frametime)
    orig = round(1.0 / frametime)
    rate = orig // int(fps)
    if orig % int(fps) != 0:
        warnings.warn("error orig_fps (%d) is not dividable with tgt_fps (%d)" % (orig, fps))
    if rate < 1:
        raise ValueError("cannot sample %d fps from a %d fps recording" % (fps, orig))
    return rate


def n_output_frames(F, rate):
    """Rows DownSampler keeps: values[0:-1:rate] - the last frame is always dropped."""
    return len(range(0, F - 1, rate))


def record_to_rotation(record, fps=60, mirror=True, joints=TARGET_JOINTS, tables=None):
    """(upper, upper_mirror) as device f64 tensors [T][9 J] from a read_bvh record (upper_mirror None without mirror)."""
    dev = record.values.device
    F, C = record.values.shape
    rate = frame_rate(record.frametime, fps)
    T = n_output_frames(F, rate)
    col, mcol, sign = tables if tables is not None else rotation_tables(record, joints)
    J = col.shape[0]
    upper = torch.empty((T, 9 * J), dtype=torch.float64, device=dev)
    upper_m = torch.empty((T, 9 * J), dtype=torch.float64, device=dev) if mirror else None
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    _lib.call("qpg_bvh_rotation_f64", dev, record.values, F, C, rate, T, J, d(col), d(mcol), d(sign), upper, upper_m)
    return upper, upper_m


def bvh_to_rotation(path, fps=60, mirror=True, device="cuda:0", joints=TARGET_JOINTS, frames="header"):
    """(upper, upper_mirror): f64 NumPy arrays (T, 9 J) - out_matrix[0], out_matrix[1] of the reference's process_bvh.
    Rows are the file's frames range(0, F - 1, rate), rate = round(1 / frametime) // fps."""
    rec = read_bvh(path, frames=frames, device=device)
    upper, upper_m = record_to_rotation(rec, fps, mirror, joints)
    return upper.cpu().numpy(), (upper_m.cpu().numpy() if mirror else None)


def process_bvh(gesture_filename, modetype=None, fps=20, output_data_pipe=None, device="cuda:0"):
    """process_bvh of the reference (beat_data_to_lmdb.py:21): (poses, poses_mirror) for modetype='rotation', or
    (None, None) - with the reason printed - for a file it cannot use.  output_data_pipe is accepted and ignored (no
    fitted pipeline exists to be saved)."""
    if modetype == "position":
        raise NotImplementedError("modetype='position' (forward kinematics) is out of scope")
    if modetype != "rotation":
        raise ValueError("modetype must be 'rotation'")
    try:
        return bvh_to_rotation(gesture_filename, fps=fps, mirror=True, device=device)
    except (ValueError, OSError) as e:
        print("process_bvh: %s: %s" % (gesture_filename, e))
        return None, None


def pose_stats(arrays, device="cuda:0"):
    """(mean, std) f64 [D] over the concatenated rows of `arrays` (one array or a list of [n_i][D] arrays / tensors):
    np.mean(np.vstack(arrays), 0), np.std(..., 0) of make_lmdb_gesture_dataset (:255-258), through qpg_column_stats_f64."""
    dev = torch.device(device)
    if isinstance(arrays, (np.ndarray, torch.Tensor)):
        arrays = [arrays]
    x = torch.cat([torch.as_tensor(a).to(dev, torch.float64).reshape(-1, a.shape[-1]) for a in arrays]).contiguous()
    N, D = x.shape
    if N == 0:
        raise ValueError("pose_stats: no rows")
    mean = torch.empty((D,), dtype=torch.float64, device=dev)
    std = torch.empty((D,), dtype=torch.float64, device=dev)
    n_ws = int(_lib.load().qpg_column_stats_ws_doubles(N, D))
    ws = torch.empty((n_ws,), dtype=torch.float64, device=dev)
    _lib.call("qpg_column_stats_f64", dev, x, N, D, mean, std, ws, n_ws)
    return mean.cpu().numpy(), std.cpu().numpy()


def format_stats(mean, std):
    """The two lines after 'data mean/std' in the reference's format (:261-262)."""
    return [str(["{:0.5f}".format(e) for e in v]).replace("'", "") for v in (mean, std)]


def split_of(path):
    """The reference's split rule on the file's path (make_beat_dataset.py:208-213); None = skipped."""
    if "81_86" in path:
        return None
    if "103" in path:
        return "test"
    if "111" in path:
        return "validation"
    return "train"


def make_dataset(save_dir, prefix, n_frames=240, fps=60, mode="duplication", subdivision_stride=30):
    """make_dataset of the reference (make_beat_dataset.py:191-258): cut every Rotation/<name>.npz of a speaker into
    windows of n_frames frames (stride n_frames for mode='noduplication', subdivision_stride for 'duplication') with
    their 16 kHz audio from Wav/<name>.npz, and write <prefix>_<split>_<stride>.npz with `body` and `wav`.
    Where MFCC/<name>.npz exists the reference's MINLEN = min(len(poses), len(mfcc)) holds and `mfcc` is written too;
    where it does not, MINLEN = len(poses) and the key is left out (a split is all or nothing: a split with some MFCC
    files missing raises).  Returns {split: path}."""
    if mode not in ("duplication", "noduplication"):
        raise ValueError("mode must be 'duplication' or 'noduplication'")
    base = os.path.join(save_dir, prefix)
    subname = {"train": [], "validation": [], "test": []}
    for f in sorted(glob.glob(os.path.join(base, "Rotation") + "/*.npz")):
        split = split_of(f)
        if split is not None:
            subname[split].append(f)
    print(len(subname["train"]), len(subname["validation"]), len(subname["test"]))
    stride = n_frames if mode == "noduplication" else subdivision_stride
    written = {}
    for split, files in subname.items():
        poses_data, mfcc_data, audio_data, have_mfcc = [], [], [], []
        for f in files:
            name = os.path.split(f)[1][:-4]
            poses = np.load(f)["upper"]
            wav = np.load(os.path.join(base, "Wav", name + ".npz"))["wav"]
            mfcc_path = os.path.join(base, "MFCC", name + ".npz")
            mfcc = np.load(mfcc_path)["mfcc"] if os.path.exists(mfcc_path) else None
            have_mfcc.append(mfcc is not None)
            MINLEN = len(poses) if mfcc is None else min(len(poses), len(mfcc))
            poses = poses[:MINLEN]
            wav = wav[:math.floor(MINLEN / fps * 16000)]
            for i in range(math.floor((MINLEN - n_frames) / stride) + 1):
                start_idx = i * stride
                poses_data.append(poses[start_idx:start_idx + n_frames])
                if mfcc is not None:
                    mfcc_data.append(mfcc[:MINLEN][start_idx:start_idx + n_frames])
                audio_start = math.floor(start_idx / fps * 16000)
                audio_data.append(wav[audio_start:audio_start + int(n_frames / fps * 16000)])
        if any(have_mfcc) and not all(have_mfcc):
            raise ValueError("split %r: MFCC/ holds files for some recordings only" % split)
        arrays = {"body": np.array(poses_data), "wav": np.array(audio_data)}
        if any(have_mfcc):
            arrays["mfcc"] = np.array(mfcc_data)
        dst = os.path.join(base, prefix + "_" + split + "_" + str(stride) + ".npz")
        np.savez_compressed(dst, **arrays)
        written[split] = dst
    return written


def selected_files(save_dir, prefix):
    """The files of <save_dir>/Motion the reference's name filter selects for `prefix` = speaker_<id>_state_<state>
    (make_beat_dataset.py:112, :156-157): <speaker>_<name>_<state>_<begin>_<end>.bvh."""
    _, speaker, _, state = prefix.split("_")
    out = []
    for f in sorted(os.listdir(os.path.join(save_dir, "Motion"))):
        parts = f[:-4].split("_") if f.endswith(".bvh") else []
        if len(parts) == 5 and parts[0] == speaker and parts[2] == state:
            out.append(f)
    return out


def process_speaker(save_dir, prefix, gpu="0", stats=False, n_frames=240):
    """Step 2 of the reference's make_beat_dataset.py as far as motion goes: Rotation/ (60 fps) and Rotation_20fps/ for the
    speaker's files (each file is read and parsed once for both rates), then make_dataset(mode='noduplication') where
    <prefix>/Wav exists.  Returns the written Rotation/ paths."""
    dev = torch.device("cuda:%s" % gpu)
    base = os.path.join(save_dir, prefix)
    for sub in ("Rotation", "Rotation_20fps"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    written, all_poses = [], []
    for f in selected_files(save_dir, prefix):
        print(f)
        try:
            rec = read_bvh(os.path.join(save_dir, "Motion", f), device=dev)
            tables = rotation_tables(rec)
            p60 = record_to_rotation(rec, 60, False, tables=tables)[0]
            p20 = record_to_rotation(rec, 20, False, tables=tables)[0]
        except ValueError as e:
            print("process_bvh: %s: %s" % (f, e))
            continue
        dst = os.path.join(base, "Rotation", f[:-4] + ".npz")
        np.savez_compressed(dst, upper=p60.cpu().numpy())
        np.savez_compressed(os.path.join(base, "Rotation_20fps", f[:-4] + ".npz"), upper=p20.cpu().numpy())
        written.append(dst)
        if stats:
            all_poses.append(p60)
    if stats and all_poses:
        print("data mean/std")
        for line in format_stats(*pose_stats(all_poses, dev)):
            print(line)
    if os.path.isdir(os.path.join(base, "Wav")):
        make_dataset(save_dir, prefix, n_frames=n_frames, mode="noduplication")
    return written


def build_parser():
    p = argparse.ArgumentParser(description="BVH -> Rotation/*.npz and the windowed dataset files")
    p.add_argument("--save_dir", type=str, default="../dataset/BEAT")
    p.add_argument("--prefix", type=str, default="speaker_10_state_0")
    p.add_argument("--gpu", type=str, default="0")
    p.add_argument("--stats", action="store_true", help="print the `data mean/std` lines over the 60 fps poses")
    p.add_argument("--n_frames", type=int, default=240)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    return process_speaker(args.save_dir, args.prefix, gpu=args.gpu, stats=args.stats, n_frames=args.n_frames)


if __name__ == "__main__":
    main()
