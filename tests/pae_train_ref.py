"""Test-side restatement of one PAE training step (codebook/PAE.py Model.forward, 300 * MSELoss, the reference's AdamW)
in torch autograd at a chosen dtype: float64 is the checker of the device kernels (tests/test_gpu_pae_train.py), float32
is pinned to the reference's own steps by tests/test_pae_train_cpu.py.  Not product code."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from qpgesture_amd import PAE_train as PT

T, E, C, M = PT.TIME, PT.EMBED, PT.IN_CH, PT.MID_CH
BN_EPS = 1e-5


def params_from_flat(P, dtype=torch.float64, requires_grad=True):
    """Flat parameter vector -> {name: leaf tensor} (trainable ones require grad)."""
    P = torch.as_tensor(np.asarray(P) if not isinstance(P, torch.Tensor) else P).detach().cpu()
    out = {}
    for n, shape in PT.PARAMS:
        v = P[PT.OFF[n]:PT.OFF[n] + int(np.prod(shape))].reshape(shape).to(dtype).clone()
        out[n] = v.requires_grad_(requires_grad and PT.OFF[n] >= PT.TRAINABLE)
    return out


def stats_from_flat(S, dtype=torch.float64):
    S = torch.as_tensor(np.asarray(S) if not isinstance(S, torch.Tensor) else S).detach().cpu()
    return {n: S[PT.ST_OFF[n]:PT.ST_OFF[n] + shape[0]].to(dtype).clone() for n, shape in PT.STATS}


def windows_input(pn, starts, train):
    """Channel-major batch (B, 135 * 240) of f32 velocity windows: zero row first (train) or last (eval), differences
    taken in the dtype of pn (f32 like the reference's dataset output)."""
    tv = torch.stack([torch.as_tensor(pn[s:s + T]) for s in starts])
    d = tv[:, 1:, :] - tv[:, :-1, :]
    z = torch.zeros(tv.shape[0], 1, tv.shape[2], dtype=tv.dtype)
    x = torch.cat((z, d), 1) if train else torch.cat((d, z), 1)
    return x.transpose(2, 1).reshape(tv.shape[0], -1)


def _bn(x, p, st, name, train):
    rm, rv = st[name + ".running_mean"], st[name + ".running_var"]
    return F.batch_norm(x, rm, rv, p[name + ".weight"], p[name + ".bias"], training=train, momentum=0.1, eps=BN_EPS)


def _atan2p(y, x, tpi):
    ans = torch.atan(y / x)
    ans = torch.where((x < 0) & (y >= 0), ans + 0.5 * tpi, ans)
    return torch.where((x < 0) & (y < 0), ans - 0.5 * tpi, ans)


def forward(p, st, x, train):
    """Model.forward on x (B, 32400); st's running statistics are updated in place in train mode.  Returns a dict of
    every intermediate (z1, h1, z2, h2, v, vn, p, f, a, b, sig, z3, h3, y) and the loss."""
    B = x.shape[0]
    r = {}
    x0 = x.reshape(B, C, T)
    r["z1"] = F.conv1d(x0, p["conv1.weight"], p["conv1.bias"], padding=T // 2)
    r["h1"] = torch.tanh(_bn(r["z1"], p, st, "bn_conv1", train))
    r["z2"] = F.conv1d(r["h1"], p["conv2.weight"], p["conv2.bias"], padding=(T - 1) // 2)
    h2 = torch.tanh(_bn(r["z2"], p, st, "bn_conv2", train))
    r["h2"] = h2
    rf = torch.fft.rfft(h2, dim=2)
    power = rf.abs()[:, :, 1:] ** 2
    ts = PT.KEYS / T
    r["f"] = torch.sum(p["freqs"] * power, dim=2) / torch.sum(power, dim=2) / ts
    r["a"] = 2 * torch.sqrt(torch.sum(power, dim=2)) / T
    r["b"] = rf.real[:, :, 0] / T
    vs, vns, ps = [], [], []
    for e in range(E):
        v = F.linear(h2[:, e, :], p["fc.%d.weight" % e], p["fc.%d.bias" % e])
        vn = _bn(v, p, st, "bn.%d" % e, train)
        vs.append(v)
        vns.append(vn)
        ps.append(_atan2p(vn[:, 1], vn[:, 0], p["tpi"]) / p["tpi"])
    r["v"], r["vn"] = torch.stack(vs, 1), torch.stack(vns, 1)          # (B, 8, 2)
    r["p"] = torch.stack(ps, 1)
    sig = r["a"][:, :, None] * torch.sin(p["tpi"] * (r["f"][:, :, None] * p["args"] + r["p"][:, :, None])) + \
        r["b"][:, :, None]
    r["sig"] = sig
    r["z3"] = F.conv1d(sig, p["deconv1.weight"], p["deconv1.bias"], padding=(T - 1) // 2)
    r["h3"] = torch.tanh(_bn(r["z3"], p, st, "bn_deconv1", train))
    r["y"] = F.conv1d(r["h3"], p["deconv2.weight"], p["deconv2.bias"], padding=T // 2)
    r["loss"] = PT.LOSS_WEIGHT * F.mse_loss(r["y"].reshape(B, -1), x)
    return r


def grads_flat(p):
    """Gradients of the trainable leaves as one flat f64 numpy vector in the parameter layout (zeros below)."""
    G = np.zeros(PT.PARAM_FLOATS)
    for n, shape in PT.PARAMS:
        if p[n].grad is not None:
            G[PT.OFF[n]:PT.OFF[n] + int(np.prod(shape))] = p[n].grad.detach().double().reshape(-1).numpy()
    return G


def adamw_step(p, g, m, v, lr, wd, step, betas=PT.BETAS, eps=PT.EPS):
    """adamw.py's update restated on arrays (float64 when given float64); returns (p, m, v)."""
    b1, b2 = betas
    p = p * (1 - wd)
    m = m * b1 + (1 - b1) * g
    v = v * b2 + (1 - b2) * g * g
    step_size = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
    return p - step_size * m / (v ** 0.5 + eps), m, v


def ws_regions(B):
    """The workspace layout of csrc/qpg_pae_train.hip (ws_layout) for batch B: {name: (float offset, shape, dtype)}.
    Every region starts at a multiple of 4 floats; the f64 regions follow the f32 ones."""
    L1, L3, NB = T + 1, T - 1, T // 2 + 1
    S = min(B, 16)
    f32 = [("x0", (B, C, T)), ("z1", (B, M, L1)), ("h1", (B, M, L1)), ("z2", (B, E, T)), ("h2", (B, E, T)),
           ("v", (B, E, 2)), ("vn", (B, E, 2)), ("pfab", (B, 4, E)), ("sig", (B, E, T)), ("z3", (B, M, L3)),
           ("h3", (B, M, L3)), ("y", (B, C, T)), ("dy", (B, C, T)), ("dh3", (B, M, L3)), ("dz3", (B, M, L3)),
           ("ds", (B, E, T)), ("dh2", (B, E, T)), ("dz2", (B, E, T)), ("dh1", (B, M, L1)), ("dz1", (B, M, L1)),
           ("dv", (B, E, 2)), ("dvn", (B, E, 2)), ("part", (S, C * M * T))]
    f64 = [("spec", (B, E, NB, 2)), ("st", (4, 32)), ("bs", (4, 32)), ("dfab", (B, 3, E)),
           ("lpart", ((B * C * T + 4095) // 4096,)), ("loss", (1,))]
    out, o = {}, 0
    for name, shape in f32:
        out[name] = (o, shape, torch.float32)
        o += (int(np.prod(shape)) + 3) // 4 * 4
    for name, shape in f64:
        out[name] = (o, shape, torch.float64)
        o += (2 * int(np.prod(shape)) + 3) // 4 * 4
    out["_floats"] = o
    return out


def ws_get(ws, B, name):
    """A region of a device workspace as a float64 CPU tensor."""
    o, shape, dt = ws_regions(B)[name]
    n = int(np.prod(shape))
    if dt == torch.float32:
        v = ws[o:o + n]
    else:
        v = ws[o:o + 2 * n].view(torch.float64)
    return v.detach().cpu().double().reshape(shape)
