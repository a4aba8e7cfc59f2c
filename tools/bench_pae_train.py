#!/usr/bin/env python
"""PAE training step throughput: ms per step (forward + backward + AdamW) at batch B, windows/s and TFLOP/s by the
direct-form count of useful work (zero-padding taps excluded), against a torch f32 autograd formulation of the same
step (written below: Model.forward, 300 * MSE, backward, the reference's AdamW with bias correction) on the same GPU.
Device events, median of --iters after --warmup.

    python tools/bench_pae_train.py [--batch 256] [--iters 9] [--warmup 3] [--json out.json] [--no-torch]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qpgesture_amd import PAE_train as PT, synth  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_TF = 157.3          # MI355X f32 matrix peak


def _useful_macs(cin, cout, lin, pad):
    """Products of a 240-tap conv over one window that meet real (non-padding) input."""
    lout = lin + 2 * pad - PT.TIME + 1
    t = np.arange(lout)[:, None] + np.arange(PT.TIME)[None, :] - pad
    return int(((t >= 0) & (t < lin)).sum()) * cin * cout


def step_flops(B):
    """Direct-form FLOPs of one step's useful work: every convolution's forward, data gradient (not conv1's) and
    weight gradient, 2 per product that meets real input (the zero-padding taps are not counted)."""
    convs = [(135, 15, 240, 120, False), (15, 8, 241, 119, True), (8, 15, 240, 119, True), (15, 135, 239, 120, True)]
    return B * sum(2 * _useful_macs(ci, co, li, pd) * (3 if dg else 2) for ci, co, li, pd, dg in convs)


def torch_step_fn(sd, x, dev):
    """The same update in torch f32 autograd: Model.forward (PAE.py:99-145), 300 * MSE, backward, AdamW
    (adamw.py: p *= 1 - wd, bias-corrected step)."""
    p = {k: torch.as_tensor(v).to(dev).float().clone().requires_grad_(k not in ("tpi", "args", "freqs") and "running" not in k
                                                      and "num_batches" not in k)
         for k, v in sd.items()}
    train = [v for v in p.values() if v.requires_grad]
    mom = [(torch.zeros_like(v), torch.zeros_like(v)) for v in train]
    state = {"step": 0}
    T = PT.TIME

    def bn(z, name):
        return F.batch_norm(z, p[name + ".running_mean"], p[name + ".running_var"], p[name + ".weight"],
                            p[name + ".bias"], training=True, momentum=0.1, eps=1e-5)

    def step():
        B = x.shape[0]
        h = torch.tanh(bn(F.conv1d(x.reshape(B, 135, T), p["conv1.weight"], p["conv1.bias"], padding=120), "bn_conv1"))
        h = torch.tanh(bn(F.conv1d(h, p["conv2.weight"], p["conv2.bias"], padding=119), "bn_conv2"))
        rf = torch.fft.rfft(h, dim=2)
        pw = rf.abs()[:, :, 1:] ** 2
        f = (p["freqs"] * pw).sum(2) / pw.sum(2) / (13 / T)
        a = 2 * torch.sqrt(pw.sum(2)) / T
        b = rf.real[:, :, 0] / T
        ps = []
        for e in range(8):
            v = bn(F.linear(h[:, e], p["fc.%d.weight" % e], p["fc.%d.bias" % e]), "bn.%d" % e)
            ang = torch.atan(v[:, 1] / v[:, 0])
            ang = torch.where((v[:, 0] < 0) & (v[:, 1] >= 0), ang + 0.5 * p["tpi"], ang)
            ang = torch.where((v[:, 0] < 0) & (v[:, 1] < 0), ang - 0.5 * p["tpi"], ang)
            ps.append(ang / p["tpi"])
        ph = torch.stack(ps, 1)
        s = a[..., None] * torch.sin(p["tpi"] * (f[..., None] * p["args"] + ph[..., None])) + b[..., None]
        h = torch.tanh(bn(F.conv1d(s, p["deconv1.weight"], p["deconv1.bias"], padding=119), "bn_deconv1"))
        y = F.conv1d(h, p["deconv2.weight"], p["deconv2.bias"], padding=120)
        for v in train:
            v.grad = None
        (300 * F.mse_loss(y.reshape(B, -1), x)).backward()
        state["step"] += 1
        t = state["step"]
        ss = 1e-4 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        with torch.no_grad():
            for v, (m, s2) in zip(train, mom):
                v.mul_(1 - 1e-5)
                m.mul_(0.9).add_(v.grad, alpha=0.1)
                s2.mul_(0.999).addcmul_(v.grad, v.grad, value=0.001)
                v.addcdiv_(m, s2.sqrt().add_(1e-8), value=-ss)
    return step


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch leg (profiling runs)")
    a = ap.parse_args()
    dev, B = "cuda:0", a.batch
    pn = np.concatenate([PT.normalise(synth.make_pae_motion(600, 50 + i), 0.0, 1.0) for i in range(4)])
    starts_all = PT.window_starts([600] * 4)
    rng = np.random.default_rng(0)
    starts = torch.from_numpy(rng.choice(starts_all, B, replace=False)).to(dev)
    tr = PT.Trainer(synth.make_pae_state_dict(11), batch=B, device=dev)
    tr.set_data(pn)

    def hip_step():
        tr.forward(starts, train=True)
        tr.backward()
        tr.step(1e-4, 1e-5)
    ms = timed(hip_step, a.iters, a.warmup)

    ms_torch = None
    if not a.no_torch:
        tv = torch.stack([torch.from_numpy(pn[i:i + PT.TIME]) for i in starts.cpu().numpy()])
        xt = torch.cat((torch.zeros(B, 1, 135), tv[:, 1:] - tv[:, :-1]), 1).transpose(2, 1).reshape(B, -1).to(dev)
        ms_torch = timed(torch_step_fn(synth.make_pae_state_dict(11), xt, dev), a.iters, a.warmup)
    fl = step_flops(B)
    res = {"batch": B, "ms_per_step": ms, "windows_per_s": B / ms * 1e3, "useful_tflops": fl / ms / 1e9,
           "useful_frac_of_f32_matrix_peak": fl / ms / 1e9 / PEAK_TF, "useful_gflop_per_step": fl / 1e9,
           "torch_f32_ms_per_step": ms_torch, "speedup_vs_torch": ms_torch / ms if ms_torch else None}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
