#!/usr/bin/env python
"""Golden vectors for TRAINING the GRU speech-to-code generator, from the REFERENCE module (imported from
/root/reference; build container only), as make_golden_generator.py does for inference: the same seeded weights
(qpgesture_amd.synth.make_generator_state_dict) and audio (synth.make_wav) are loaded into the reference's own
Generator_gru, which runs in train() mode with model.project.dropout = 0.0, in f32 and, after .double(), in f64.

    python tests/golden/make_golden_generator_train.py        ->  tests/golden/generator_train.npz

Runs (prefix r<i>_): (B 3, n 64 000), (B 17, n 7 810: T = 2), (B 2, n 5 866: T = 1).  Per run: loss64, loss32, the seeded
target; per parameter <key> the f64 gradient at every GRAD_STEP-th entry (g_<key>), max |g64| (m_<key>), the sum of the f64
gradient (s_<key>), e32 = max |g32 - g64| over the WHOLE tensor (e_<key>) and max |g32| (n_<key>: the scale for the four
convolution biases in front of a train-mode BatchNorm, whose true gradient is zero); the eight running statistics after
the step (f64, whole) with their e32.

traj_*: 4 Adam updates (lr 0.0002, betas (0.99, 0.999), torch.optim.Adam) at B = 4 with a different seeded batch per
update: losses64, losses32.

Asserted before writing: the four pre-BatchNorm biases have max |g64| <= 1e-9; at T = 1 all four weight_hh gradients are
exactly 0; no tensor's e32 is 0 except those.

win_*: what the reference's own window sampling (data_loader/data_preprocessor.py:121-139, read from the reference's file
and executed as it stands - lmdb is not importable here) gives for the clips in WINDOW_CASES: per case the number of
windows and, per window, its start frame, audio start, audio length, first code and number of codes."""
import copy
import math
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from qpgesture_amd import synth  # noqa: E402

REF = "/root/reference/codebook"
SEED_W, SEED_WAV, SEED_TARGET = 29, 31, 32
RUNS = ((3, 64000), (17, 7810), (2, 5866))
GRAD_STEP = 61
TRAJ_B, TRAJ_N, TRAJ_UPDATES, LR, BETAS = 4, 64000, 4, 0.0002, (0.99, 0.999)
ZERO_BIASES = tuple("WavEncoder.feat_extractor.%d.bias" % (3 * i) for i in range(4))
# (pose frames, audio samples, raw codes, stride): at, one below and one above a window; strides that are no multiple of 8
WINDOW_CASES = ((240, 64000, 30, 10), (239, 64000, 30, 10), (241, 64267, 31, 10), (600, 160000, 75, 10), (600, 160000, 75, 7),
                (600, 160000, 70, 13))


def build_model(sd):
    import torch
    sys.path.insert(0, os.path.join(REF, "generate"))
    from generate import Generator_gru
    model = Generator_gru()
    model.load_state_dict({k[len("module."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.train()
    model.project.dropout = 0.0
    return model


def frames(n):
    for s in (3, 3, 6, 6, 6):
        n = (n - 16) // s + 1
    return n


def grads_of(model, wav, target, dtype):
    import torch
    model.zero_grad()
    _, loss = model(torch.from_numpy(wav).to(dtype), torch.from_numpy(target))
    loss.backward()
    g = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()}
    stats = {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    return float(loss.detach()), g, stats


def one_run(sd, B, n, i):
    m32 = build_model(sd)
    m64 = copy.deepcopy(m32).double()
    import torch
    wav = np.ascontiguousarray(synth.make_wav(SEED_WAV + i, B, n))
    T = frames(n)
    target = np.random.Generator(np.random.PCG64(SEED_TARGET + i)).integers(0, 512, (B, T)).astype(np.int64)
    l32, g32, s32 = grads_of(m32, wav, target, torch.float32)
    l64, g64, s64 = grads_of(m64, wav, target, torch.float64)
    pre = "r%d_" % i
    out = {pre + "B": np.int64(B), pre + "n": np.int64(n), pre + "target": target, pre + "loss64": np.float64(l64),
           pre + "loss32": np.float64(l32)}
    for k in g64:
        a64, a32 = g64[k].reshape(-1), g32[k].reshape(-1).astype(np.float64)
        e32 = float(np.abs(a32 - a64).max())
        out[pre + "g_" + k] = a64[::GRAD_STEP].copy()
        out[pre + "m_" + k] = np.float64(np.abs(a64).max())
        out[pre + "s_" + k] = np.float64(a64.sum())
        out[pre + "e_" + k] = np.float64(e32)
        out[pre + "n_" + k] = np.float64(np.abs(a32).max())
        if k in ZERO_BIASES:
            assert np.abs(a64).max() <= 1e-9, (k, np.abs(a64).max())
        elif T == 1 and "weight_hh" in k:
            assert np.all(a64 == 0) and np.all(a32 == 0), k
        else:
            assert e32 > 0, (pre, k)
    for k in s64:
        out[pre + "v_" + k] = s64[k]
        out[pre + "e_" + k] = np.float64(np.abs(s32[k].astype(np.float64) - s64[k]).max())
        assert out[pre + "e_" + k] > 0, (pre, k)
    print("%s B %d n %d T %d: loss %.8f (f32 off by %.2e); zero biases |g64| <= %.1e, |g32| <= %.1e" % (
        pre, B, n, T, l64, abs(l32 - l64), max(out[pre + "m_" + k] for k in ZERO_BIASES),
        max(out[pre + "n_" + k] for k in ZERO_BIASES)))
    return out


def trajectory(sd):
    import torch
    losses = {}
    for dtype in (torch.float32, torch.float64):
        model = build_model(sd)
        if dtype == torch.float64:
            model = model.double()
        opt = torch.optim.Adam(model.parameters(), lr=LR, betas=BETAS)
        ls = []
        for u in range(TRAJ_UPDATES):
            wav = synth.make_wav(SEED_WAV + 100 + u, TRAJ_B, TRAJ_N)
            target = np.random.Generator(np.random.PCG64(SEED_TARGET + 100 + u)).integers(0, 512, (TRAJ_B, frames(TRAJ_N)))
            opt.zero_grad()
            _, loss = model(torch.from_numpy(wav).to(dtype), torch.from_numpy(target.astype(np.int64)))
            loss.backward()
            opt.step()
            ls.append(float(loss))
        losses[dtype] = np.array(ls, np.float64)
    print("trajectory: losses64 %s, |f32 - f64| %s" % (losses[torch.float64], np.abs(losses[torch.float32] - losses[torch.float64])))
    return dict(traj_losses64=losses[torch.float64], traj_losses32=losses[torch.float32], traj_B=np.int64(TRAJ_B),
                traj_n=np.int64(TRAJ_N), traj_seed_wav=np.int64(SEED_WAV + 100), traj_seed_target=np.int64(SEED_TARGET + 100))


def reference_windows(n_frames, n_audio, n_codes_raw, stride):
    """[(start frame, audio start, audio length, first code, number of codes)] by lines 121-139 of the reference's
    data_preprocessor.py."""
    with open(os.path.join(REF, "data_loader", "data_preprocessor.py")) as f:
        src = f.read().split("\n")
    body = textwrap.dedent("\n".join(src[120:139]))
    rec = []
    ns = dict(math=math, np=np, rec=rec, clip_skeleton=np.zeros((n_frames, 3)), clip_audio_raw=np.arange(n_audio, dtype=np.float32),
              clip_codes_raw=np.arange(1000, 1000 + n_codes_raw),
              self=types.SimpleNamespace(n_poses=240, subdivision_stride=stride, n_codes=30, skeleton_resampling_fps=60,
                                         audio_sample_length=64000))
    exec(body + "\n    rec.append((start_idx, audio_start, len(sample_audio), int(sample_codes[0]) if len(sample_codes) else -1, "
         "len(sample_codes)))\n", ns)
    return rec


def main():
    sd = synth.make_generator_state_dict(SEED_W)
    out = dict(seed_w=np.int64(SEED_W), seed_wav=np.int64(SEED_WAV), seed_target=np.int64(SEED_TARGET), grad_step=np.int64(GRAD_STEP),
               n_runs=np.int64(len(RUNS)))
    for i, (B, n) in enumerate(RUNS):
        out.update(one_run(sd, B, n, i))
    out.update(trajectory(sd))
    cases, counts, rows = [], [], []
    for case in WINDOW_CASES:
        rec = reference_windows(*case)
        cases.append(case)
        counts.append(len(rec))
        rows += rec
    out.update(win_cases=np.array(cases, np.int64), win_counts=np.array(counts, np.int64),
               win_rows=np.array(rows, np.int64).reshape(-1, 5))
    print("windows:", list(zip(cases, counts)))
    path = os.path.join(HERE, "generator_train.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
