"""NumPy restatement of the GRU speech-to-code generator (the reference's Generator_gru in eval mode), stage by stage, in
the dtype asked for: f64 is the tests' reference, an f32 run gives the error scale e32 of a per-kernel contract test.
Written from the model's definition (torch.nn's documented Conv1d / BatchNorm1d / GRU / LayerNorm / Linear formulas), not
from the device code.  Activations are channels-last [B][T][C]; weights keep torch's layouts."""
import numpy as np

TAPS, HIDDEN, CODES = 16, 200, 512
STRIDES = (3, 3, 6, 6, 6)
BN_EPS = LN_EPS = 1e-5
SLOPE = 0.3


def frames(t_in, stride):
    return 0 if t_in < TAPS else (t_in - TAPS) // stride + 1


def strip(sd):
    """The state dict as f64-exact NumPy arrays without the DataParallel prefix."""
    out = {}
    for k, v in sd.items():
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        out[k[7:] if k.startswith("module.") else k] = v
    return out


def conv1d(x, w, bias, stride, bn=None, slope=None, dtype=np.float64):
    """x [B][Tin][Cin], w [Cout][Cin][16] (torch's), bias [Cout] or None, bn = (weight, bias, mean, var) or None."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    T = frames(x.shape[1], stride)
    idx = stride * np.arange(T)[:, None] + np.arange(TAPS)[None, :]
    y = np.einsum("btjc,ocj->bto", x[:, idx, :], w)
    if bias is not None:
        y = y + np.asarray(bias, dtype)
    if bn is not None:
        g, b, mean, var = (np.asarray(a, dtype) for a in bn)
        y = (y - mean) / np.sqrt(var + dtype(BN_EPS)) * g + b
    if slope is not None:
        y = np.where(y > 0, y, y * dtype(slope))
    return y.astype(dtype)


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def gru_direction(x, w_ih, w_hh, b_ih, b_hh, reverse, dtype=np.float64):
    x = np.asarray(x, dtype)
    w_ih, w_hh, b_ih, b_hh = (np.asarray(a, dtype) for a in (w_ih, w_hh, b_ih, b_hh))
    B, T, _ = x.shape
    H = w_hh.shape[1]
    h = np.zeros((B, H), dtype)
    out = np.zeros((B, T, H), dtype)
    gi_all = x @ w_ih.T + b_ih
    with np.errstate(over="ignore"):
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            gi, gh = gi_all[:, t], h @ w_hh.T + b_hh
            r = sigmoid(gi[:, :H] + gh[:, :H])
            z = sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h = ((1 - z) * n + z * h).astype(dtype)
            out[:, t] = h
    return out


def gru_layer(x, w_ih, w_hh, b_ih, b_hh, dtype=np.float64):
    """w_ih [2][3H][In], w_hh [2][3H][H], b_ih, b_hh [2][3H] -> [B][T][2H] (direction 0 | direction 1)."""
    return np.concatenate([gru_direction(x, w_ih[d], w_hh[d], b_ih[d], b_hh[d], bool(d), dtype) for d in (0, 1)], -1)


def head(y, ln_g, ln_b, out_w, out_b, dtype=np.float64):
    """y [.., 2H] -> (LayerNorm of the direction sum [.., H], logits [.., N])."""
    y = np.asarray(y, dtype)
    H = y.shape[-1] // 2
    s = y[..., :H] + y[..., H:]
    mean = s.mean(-1, keepdims=True)
    var = ((s - mean) ** 2).mean(-1, keepdims=True)
    ln = ((s - mean) / np.sqrt(var + dtype(LN_EPS)) * np.asarray(ln_g, dtype) + np.asarray(ln_b, dtype)).astype(dtype)
    return ln, (ln @ np.asarray(out_w, dtype).T + np.asarray(out_b, dtype)).astype(dtype)


def argmax(logits):
    return np.argmax(logits, -1).astype(np.int64)          # (the first maximum)


def cross_entropy(logits, target, dtype=np.float64):
    logits = np.asarray(logits, dtype).reshape(-1, logits.shape[-1])
    target = np.asarray(target).reshape(-1)
    m = logits.max(-1, keepdims=True)
    lse = np.log(np.exp(logits - m).sum(-1)) + m[:, 0]
    return dtype((lse - logits[np.arange(len(target)), target]).mean())


def gru_weights(p, layer):
    tags = ["_l%d" % layer, "_l%d_reverse" % layer]
    return tuple(np.stack([p["project.%s%s" % (n, t)] for t in tags]) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def forward(sd, wav, dtype=np.float64):
    """Every stage of the model on wav [B][n]: dict(enc, gru0, gru1, ln, logits, codes)."""
    p = strip(sd)
    x = np.asarray(wav, dtype)[:, :, None]
    for i, s in enumerate(STRIDES):
        pre = "WavEncoder.feat_extractor.%d." % (3 * i)
        bn = None
        if i < 4:
            q = "WavEncoder.feat_extractor.%d." % (3 * i + 1)
            bn = (p[q + "weight"], p[q + "bias"], p[q + "running_mean"], p[q + "running_var"])
        x = conv1d(x, p[pre + "weight"], p[pre + "bias"], s, bn, SLOPE if i < 4 else None, dtype)
    g0 = gru_layer(x, *gru_weights(p, 0), dtype=dtype)
    g1 = gru_layer(g0, *gru_weights(p, 1), dtype=dtype)
    ln, logits = head(g1, p["norm.weight"], p["norm.bias"], p["out.weight"], p["out.bias"], dtype)
    return dict(enc=x, gru0=g0, gru1=g1, ln=ln, logits=logits, codes=argmax(logits))
