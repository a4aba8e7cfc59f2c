"""Phase extraction (qpg_pae_phase_f32) throughput on one GPU: prints one JSON line.

A seeded batch of ~100 000 frames (28 clips of 3 600 frames, synth.make_pae_motion) through PAE.pose2phase_clips'
launches, timed with device events after warm-up, median of --reps runs.  FLOPs are the DIRECT-FORM count of one
frame's forward pass (conv1 over the 43 199 non-zero (position, tap) pairs x 135 x 15 MACs, conv2 over 43 200 x 15 x 8,
the fc layers, 2 FLOP per MAC: 185.35 MFLOP), not what the kernel issues (it also multiplies padding); the fraction is
against the 157.3 TF f32 matrix peak.  Baselines on the same GPU: a batched torch formulation (unfold to windows +
F.conv1d, --torch-frames frames) and the reference's batch-1 loop (Model.forward once per frame, --loop-frames frames).

    python tools/bench_pae.py [--clips 28] [--frames 3600] [--reps 7] [--torch-frames 8192] [--loop-frames 500]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from qpgesture_amd import PAE, _lib, synth  # noqa: E402
from qpgesture_amd.checkpoint import load_config  # noqa: E402

FLOP_PER_FRAME = 2.0 * (43199 * 135 * 15 + 43200 * 15 * 8 + 8 * 2 * 240)
PEAK_F32_TF = 157.3


def events_median(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), ts


class TorchPAE:
    """The reference's eval-mode forward up to `params`, in plain torch (baselines only)."""

    def __init__(self, sd, dev):
        self.t = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd.items()}

    def bn(self, x, n):
        t = self.t
        return F.batch_norm(x, t[n + ".running_mean"], t[n + ".running_var"], t[n + ".weight"], t[n + ".bias"], False)

    def __call__(self, win):                     # win (B, 135, 240)
        t = self.t
        y = torch.tanh(self.bn(F.conv1d(win, t["conv1.weight"], t["conv1.bias"], padding=120), "bn_conv1"))
        y = torch.tanh(self.bn(F.conv1d(y, t["conv2.weight"], t["conv2.bias"], padding=119), "bn_conv2"))
        X = torch.fft.rfft(y, dim=2)
        pw = X.abs()[:, :, 1:] ** 2
        f = torch.sum(t["freqs"] * pw, dim=2) / torch.sum(pw, dim=2) / (13 / 240)
        a = 2 * torch.sqrt(torch.sum(pw, dim=2)) / 240
        b = X.real[:, :, 0] / 240
        ps = []
        for e in range(8):
            v = self.bn(F.linear(y[:, e], t["fc.%d.weight" % e], t["fc.%d.bias" % e]), "bn.%d" % e)
            ang = torch.atan(v[:, 1] / v[:, 0])
            ang = torch.where((v[:, 0] < 0) & (v[:, 1] >= 0), ang + 0.5 * t["tpi"], ang)
            ang = torch.where((v[:, 0] < 0) & (v[:, 1] < 0), ang - 0.5 * t["tpi"], ang)
            ps.append(ang / t["tpi"])
        return torch.stack([torch.stack(ps, 1), f, a, b], 1)


def torch_windows(vel_pad, i0, n):
    """Windows of frames i0 .. i0+n-1 from the zero-padded velocities (T + 238, 135): (n, 135, 240), row 0 zero."""
    w = vel_pad[i0:i0 + n + 238].t().unfold(1, 239, 1).permute(1, 0, 2)             # (n, 135, 239)
    return F.pad(w, (1, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=28)
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--torch-frames", type=int, default=8192)
    ap.add_argument("--torch-batch", type=int, default=1024)
    ap.add_argument("--loop-frames", type=int, default=500)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synth.make_pae_state_dict(11)
    net = PAE.Model(sd, device=dev)
    cfg = load_config(os.path.join(os.path.dirname(PAE.__file__), "configs", "codebook.yml"))
    mean, std = np.asarray(cfg.data_mean), np.clip(np.asarray(cfg.data_std), 0.01, None)
    poses = [synth.make_pae_motion(args.frames, 1000 + c) for c in range(args.clips)]
    n = args.clips * args.frames

    # the device path: the same launches as pose2phase_clips, inputs resident (host transfers excluded)
    chunk = min(args.chunk, n)
    pose = torch.from_numpy(np.concatenate(poses)).to(dev)
    off = torch.from_numpy(np.arange(args.clips + 1, dtype=np.int64) * args.frames).to(dev)
    mean_t, std_t = torch.from_numpy(mean.copy()).to(dev), torch.from_numpy(std.copy()).to(dev)
    ws = torch.empty((chunk + 239) * 136, dtype=torch.float32, device=dev)
    out = torch.empty((n, 4, 8), dtype=torch.float32, device=dev)

    def run():
        for f0 in range(0, n, chunk):
            nf = min(chunk, n - f0)
            _lib.call("qpg_pae_phase_f32", dev, net.params, pose, mean_t, std_t, off, args.clips, n, f0, nf, ws,
                      ws.numel(), out[f0:f0 + nf], None, None)
    t_dev, ts = events_median(run, args.reps)
    got = out.cpu().numpy()
    end_to_end = time.perf_counter()
    PAE.pose2phase_clips(net, poses, mean, std, chunk=args.chunk)
    torch.cuda.synchronize()
    end_to_end = time.perf_counter() - end_to_end

    # batched torch: unfold + F.conv1d (windows of the first clip, --torch-batch frames per call)
    tp = TorchPAE(sd, dev)
    pn = (poses[0] - mean) / std
    vel = torch.from_numpy((pn[1:] - pn[:-1]).astype(np.float32)).to(dev)
    vel_pad = F.pad(vel, (0, 0, 120, 119))
    nt = min(args.torch_frames, args.frames)

    def run_torch():
        for i0 in range(0, nt, args.torch_batch):
            m = min(args.torch_batch, nt - i0)
            tp(torch_windows(vel_pad, i0, m))
    with torch.no_grad():
        t_torch, _ = events_median(run_torch, max(3, args.reps // 2), warmup=1)
        ref = tp(torch_windows(vel_pad, 0, 256)).cpu().numpy()
        nl = min(args.loop_frames, args.frames)

        def run_loop():
            for i in range(nl):
                tp(torch_windows(vel_pad, i, 1))
        t_loop, _ = events_median(run_loop, 3, warmup=1)
    g = got[:256, 1:]
    agree = float(np.max(np.abs(g - ref[:, 1:]) / np.maximum(np.abs(ref[:, 1:]), 1e-2)))

    fps = n / t_dev
    rec = {
        "tool": "bench_pae", "frames": n, "clips": args.clips, "frames_per_clip": args.frames, "chunk": chunk,
        "reps": args.reps, "time_s_median": t_dev, "time_s_all": ts, "frames_per_s": fps,
        "us_per_frame": 1e6 * t_dev / n,
        "flop_per_frame_direct_form": FLOP_PER_FRAME,
        "achieved_tflops_direct_form": fps * FLOP_PER_FRAME / 1e12,
        "fraction_of_f32_matrix_peak": fps * FLOP_PER_FRAME / 1e12 / PEAK_F32_TF,
        "conv1_share_of_direct_flops": 43199 * 135 * 15 * 2 / FLOP_PER_FRAME,
        "end_to_end_s_incl_host_copies": end_to_end,
        "torch_batched_frames_per_s": nt / t_torch, "torch_batched_frames": nt, "torch_batch": args.torch_batch,
        "loop_batch1_frames_per_s": nl / t_loop, "loop_batch1_frames": nl,
        "speedup_vs_torch_batched": fps / (nt / t_torch), "speedup_vs_batch1_loop": fps / (nl / t_loop),
        "max_rel_diff_fab_vs_torch_first256": agree,
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
