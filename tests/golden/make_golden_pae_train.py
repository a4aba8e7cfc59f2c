#!/usr/bin/env python
"""Golden vectors for PAE training (qpgesture_amd/PAE_train.py) from the REFERENCE's own code (codebook/PAE.py Model,
Library/AdamWR/adamw.py AdamW, Library/AdamWR/cyclic_scheduler.py CyclicLRWithRestarts), imported from the reference
tree on the build container only, exactly as make_golden_pae.py does.

Setup: seeded weights (synth.make_pae_state_dict(SEED)) in the reference's PAE.Model on the CPU; 16 windows at stride 1
of one seeded clip (synth.make_pae_motion(255, MOTION_SEED)), normalised with codebook.yml's mean / clip(std, 0.01) in
f64 and rounded once to f32 like the reference's dataset.  One validation pass (eval mode, zero row last, batches of 4
in order), then 3 training steps (train mode, zero row first) on batches of a seeded permutation, with the reference's
AdamW and CyclicLRWithRestarts(batch_size=1, epoch_size=4, restart_period=10, t_mult=2, policy="cosine") stepped the
way PAE.py:340-379 steps them.  Committed are only OUTPUTS (and the batch indices the steps used)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from qpgesture_amd import synth  # noqa: E402

SEED, MOTION_SEED, N_WIN, BATCH, STEPS = 11, 31, 16, 4, 3
SAMPLES = 97                     # strided samples per parameter / gradient
SCHED_EPOCH_SIZE, SCHED_EPOCHS = 5, 80


def samples_index(n):
    return np.unique(np.linspace(0, n - 1, SAMPLES).round().astype(np.int64))


def main():
    import yaml
    from make_golden_pae import reference_module, REF
    PAE = reference_module()
    from Library.AdamWR import adamw, cyclic_scheduler

    torch.manual_seed(0)
    net = PAE.Model(input_channels=135, embedding_channels=8, time_range=240, key_range=13, window=4.0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_pae_state_dict(SEED).items()})
    cfg = yaml.safe_load(open(os.path.join(REF, "configs", "codebook.yml")))
    mean = np.array(cfg["data_mean"]).squeeze()
    std = np.clip(np.array(cfg["data_std"]).squeeze(), a_min=0.01, a_max=None)
    pose = synth.make_pae_motion(N_WIN + 239, MOTION_SEED)
    pn = torch.from_numpy((pose - mean) / std).float()                      # (255, 135)
    wins = torch.stack([pn[i:i + 240] for i in range(N_WIN)])               # (16, 240, 135)

    def batch_of(tv, train):
        z = torch.zeros(tv.shape[0], 1, tv.shape[2])
        d = tv[:, 1:, :] - tv[:, :-1, :]
        x = torch.cat((z, d), 1) if train else torch.cat((d, z), 1)
        return x.transpose(2, 1).reshape(tv.shape[0], -1)

    out = {"meta": np.array([SEED, MOTION_SEED, N_WIN, BATCH, STEPS], np.int64)}
    sd = net.state_dict()
    out["sd_keys"] = np.array(list(sd.keys()))
    out["sd_shapes"] = np.array([";".join(str(d) for d in v.shape) for v in sd.values()])
    out["sd_dtypes"] = np.array([str(v.dtype).replace("torch.", "") for v in sd.values()])

    # validation pass (evaluate_testset): eval mode, batches in order, mean of the per-batch losses
    net.eval()
    mse = torch.nn.MSELoss()
    vals = []
    with torch.no_grad():
        for i in range(0, N_WIN, BATCH):
            x = batch_of(wins[i:i + BATCH], False)
            y, _, _, _ = net(x)
            vals.append(float(300 * mse(y, x)))
    out["val_losses"] = np.array(vals)
    out["val_loss"] = np.array(np.mean(vals))

    # training steps
    net.train()
    opt = adamw.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-4)
    sched = cyclic_scheduler.CyclicLRWithRestarts(optimizer=opt, batch_size=1, epoch_size=N_WIN // BATCH,
                                                  restart_period=10, t_mult=2, policy="cosine")
    g = torch.Generator().manual_seed(23456)
    perm = torch.randperm(N_WIN, generator=g).numpy()
    out["perm"] = perm.astype(np.int64)
    sched.step()
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    losses, lrs, wds = [], [], []
    for s in range(STEPS):
        idx = perm[s * BATCH:(s + 1) * BATCH]
        x = batch_of(wins[idx], True)
        y, latent, signal, params = net(x)
        loss = 300 * mse(y, x)
        opt.zero_grad()
        loss.backward()
        lrs.append(opt.param_groups[0]["lr"])
        wds.append(opt.param_groups[0]["weight_decay"])
        if s == 0:
            for k, name in enumerate("pfab"):
                out["step1_" + name] = params[k].detach().squeeze(2).numpy().astype(np.float32)
        for n, p in net.named_parameters():
            if p.grad is None:
                continue
            gr = p.grad.detach().reshape(-1).numpy()
            out["gnorm_%d_%s" % (s, n)] = np.array(np.linalg.norm(gr.astype(np.float64)))
            out["g_%d_%s" % (s, n)] = gr[samples_index(gr.size)].astype(np.float32)
        opt.step()
        sched.batch_step()
        for n, p in net.named_parameters():
            if p.requires_grad:
                pr = p.detach().reshape(-1).numpy()
                out["p_%d_%s" % (s, n)] = pr[samples_index(pr.size)].astype(np.float32)
        for n, b in net.named_buffers():
            out["buf_%d_%s" % (s, n)] = b.detach().numpy().copy()
        losses.append(float(loss))
    out["losses"] = np.array(losses)
    out["lrs"], out["wds"] = np.array(lrs), np.array(wds)
    out["trainable"] = np.array(names)

    # (lr, wd) of every update over SCHED_EPOCHS epochs of SCHED_EPOCH_SIZE updates (restarts at 10, 30, 70)
    p0 = torch.nn.Parameter(torch.zeros(3))
    opt2 = adamw.AdamW([p0], lr=1e-4, weight_decay=1e-4)
    sc2 = cyclic_scheduler.CyclicLRWithRestarts(optimizer=opt2, batch_size=1, epoch_size=SCHED_EPOCH_SIZE,
                                                restart_period=10, t_mult=2, policy="cosine")
    trace = []
    for ep in range(SCHED_EPOCHS):
        sc2.step()
        for _ in range(SCHED_EPOCH_SIZE):
            trace.append((opt2.param_groups[0]["lr"], opt2.param_groups[0]["weight_decay"]))
            sc2.batch_step()
    out["sched_trace"] = np.array(trace)
    out["sched_meta"] = np.array([SCHED_EPOCH_SIZE, SCHED_EPOCHS], np.int64)

    # AdamW on small tensors, 5 steps, varying lr and weight decay
    rng = np.random.default_rng(5)
    p_init = rng.standard_normal(37).astype(np.float32)
    grads = (rng.standard_normal((5, 37)) * np.array([1.0, 1e-3, 10.0, 1e-6, 0.5])[:, None]).astype(np.float32)
    lr_wd = np.array([[1e-3, 1e-4], [5e-4, 0.0], [1e-2, 3e-3], [1e-4, 1e-2], [2e-3, 5e-5]])
    pa = torch.nn.Parameter(torch.from_numpy(p_init.copy()))
    opt3 = adamw.AdamW([pa], lr=1e-3, weight_decay=1e-4)
    ptrace = []
    for k in range(5):
        opt3.param_groups[0]["lr"], opt3.param_groups[0]["weight_decay"] = float(lr_wd[k, 0]), float(lr_wd[k, 1])
        pa.grad = torch.from_numpy(grads[k].copy())
        opt3.step()
        ptrace.append(pa.detach().numpy().copy())
    out["adamw_p0"], out["adamw_g"], out["adamw_lr_wd"] = p_init, grads, lr_wd
    out["adamw_p"] = np.stack(ptrace)
    path = os.path.join(HERE, "pae_train_s%d.npz" % SEED)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; losses", losses, "val", out["val_loss"])


if __name__ == "__main__":
    main()
