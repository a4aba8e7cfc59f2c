"""NumPy restatement of the WavLM forward pass (inference, no masks), written from the model's mathematics: the
reference the GPU kernels of qpg_wavlm.hip are tested against.  Every function takes `dt` (np.float64 for the reference
value, np.float32 for the size of f32's own rounding error at that stage) and works on channels-last arrays [B][T][C].
tests/test_wavlm_cpu.py pins it against the goldens of tests/golden/make_golden_wavlm.py to 1e-9."""
import math

import numpy as np

from qpgesture_amd import wavlm as W

try:
    from scipy.special import erf as _erf
except ImportError:                                            # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x):
    return (x * x.dtype.type(0.5) * (1 + _erf(x * x.dtype.type(math.sqrt(0.5))).astype(x.dtype))).astype(x.dtype)


def layer_norm(x, g, b, eps=1e-5):
    dt = x.dtype.type
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    return (d / np.sqrt(var + dt(eps)) * g.astype(x.dtype) + b.astype(x.dtype)).astype(x.dtype)


def conv1d(x, w, b, stride):
    """x [B][T][Cin], w [Cout][Cin][k] (torch layout), no padding -> [B][T_out][Cout]."""
    B, T, Cin = x.shape
    Cout, _, k = w.shape
    To = (T - k) // stride + 1
    win = np.stack([x[:, j:j + stride * (To - 1) + 1:stride] for j in range(k)], 2)      # [B][To][k][Cin]
    y = win.reshape(B, To, k * Cin) @ w.transpose(2, 1, 0).reshape(k * Cin, Cout).astype(x.dtype)
    return (y + b.astype(x.dtype)) if b is not None else y


def feature_extractor(sd, cfg, wav, dt, upto=None):
    """The conv stack on (B, n) samples -> [B][T][C]; `upto` = number of layers to run (default all)."""
    x = np.asarray(wav, dt)[:, :, None]
    layers = W.conv_layers_of(cfg)
    for i, (_, k, s) in enumerate(layers[:upto]):
        p = "feature_extractor.conv_layers.%d." % i
        b = sd[p + "0.bias"] if cfg.get("conv_bias", False) else None
        x = conv1d(x, np.asarray(sd[p + "0.weight"], dt), None if b is None else np.asarray(b, dt), s)
        x = gelu(layer_norm(x, np.asarray(sd[p + "2.1.weight"], dt), np.asarray(sd[p + "2.1.bias"], dt)))
    return x


def linear(x, w, b):
    return x @ w.T.astype(x.dtype) + b.astype(x.dtype)


def pos_conv(x, weff, bias, groups):
    """x + GELU(grouped conv): x [B][T][D], weff [D][D/groups][k] (folded), padding k // 2, an even kernel's last output
    frame dropped."""
    B, T, D = x.shape
    k = weff.shape[2]
    Cg = D // groups
    pad = k // 2
    xp = np.zeros((B, T + k - 1, D), x.dtype)
    xp[:, pad:pad + T] = x
    y = np.empty_like(x)
    for g in range(groups):
        win = np.stack([xp[:, j:j + T, g * Cg:(g + 1) * Cg] for j in range(k)], 2)        # [B][T][k][Cg]
        wg = weff[g * Cg:(g + 1) * Cg].astype(x.dtype)                                   # [Cg out][Cg in][k]
        y[:, :, g * Cg:(g + 1) * Cg] = win.reshape(B, T, k * Cg) @ wg.transpose(2, 1, 0).reshape(k * Cg, Cg)
    return x + gelu(y + bias.astype(x.dtype))


def gate(h, grep_w, grep_b, grep_a, H):
    """[B][T][H] row factors gate_a (gate_b grep_a - 1) + 2 from the layer-normed block input h [B][T][D]."""
    B, T, D = h.shape
    dt = h.dtype
    s = h.reshape(B, T, H, D // H) @ grep_w.T.astype(dt) + grep_b.astype(dt)               # [B][T][H][8]
    ab = 1 / (1 + np.exp(-s.reshape(B, T, H, 2, 4).sum(-1)))
    return (ab[..., 0] * (ab[..., 1] * grep_a.reshape(H).astype(dt) - 1) + 2).astype(dt)


def position_bias(rel_emb, T, num_buckets, max_distance, dt):
    """[H][T][T]: entry (h, q, k) = rel_emb[bucket(k - q)][h]."""
    rel = np.arange(T)[None, :] - np.arange(T)[:, None]
    return np.asarray(rel_emb, dt)[W.relative_position_buckets(rel, num_buckets, max_distance)].transpose(2, 0, 1)


def attention(q, k, v, gate_f, bias, H, bias_scale=1.0):
    """q (scaled), k, v [B][T][D], gate_f [B][T][H], bias [H][T][T] -> [B][T][D]."""
    B, T, D = q.shape
    dt = q.dtype

    def heads(a):
        return a.reshape(B, T, H, D // H).transpose(0, 2, 1, 3)
    s = heads(q) @ heads(k).transpose(0, 1, 3, 2)                                         # [B][H][T][T]
    s = s + gate_f.transpose(0, 2, 1)[..., None] * (bias[None] * dt.type(bias_scale))
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    p = e / e.sum(-1, keepdims=True)
    return (p @ heads(v)).transpose(0, 2, 1, 3).reshape(B, T, D).astype(dt)


def block(sd, cfg, i, x, bias):
    dt = x.dtype
    H = cfg["encoder_attention_heads"]
    p = "encoder.layers.%d." % i
    a = p + "self_attn."

    def P(name):
        return np.asarray(sd[name], dt)
    h = layer_norm(x, P(p + "self_attn_layer_norm.weight"), P(p + "self_attn_layer_norm.bias"))
    gf = gate(h, P(a + "grep_linear.weight"), P(a + "grep_linear.bias"), P(a + "grep_a"), H)
    q = linear(h, P(a + "q_proj.weight"), P(a + "q_proj.bias")) * dt.type((x.shape[2] // H) ** -0.5)
    ctx = attention(q, linear(h, P(a + "k_proj.weight"), P(a + "k_proj.bias")),
                    linear(h, P(a + "v_proj.weight"), P(a + "v_proj.bias")), gf, bias, H)
    x = x + linear(ctx, P(a + "out_proj.weight"), P(a + "out_proj.bias"))
    h = layer_norm(x, P(p + "final_layer_norm.weight"), P(p + "final_layer_norm.bias"))
    return x + linear(gelu(linear(h, P(p + "fc1.weight"), P(p + "fc1.bias"))), P(p + "fc2.weight"), P(p + "fc2.bias"))


def forward(sd, cfg, wav, dt=np.float64):
    """dict(features, pos_conv, block0, out): the conv stack's output, x + GELU(pos_conv(x)), the first block's output
    and the final result, all [B][T][.] in dtype dt."""
    cfg = dict(W.CFG_DEFAULTS, **cfg)
    D, H = cfg["encoder_embed_dim"], cfg["encoder_attention_heads"]

    def P(name):
        return np.asarray(sd[name], dt)
    taps = {}
    f = feature_extractor(sd, cfg, wav, dt)
    taps["features"] = f
    x = layer_norm(f, P("layer_norm.weight"), P("layer_norm.bias"))
    if f.shape[2] != D:
        x = linear(x, P("post_extract_proj.weight"), P("post_extract_proj.bias"))
    weff = W.fold_weight_norm(sd["encoder.pos_conv.0.weight_g"], sd["encoder.pos_conv.0.weight_v"])
    if dt == np.float32:
        weff = weff.astype(np.float32)
    x = pos_conv(x, weff, P("encoder.pos_conv.0.bias"), cfg["conv_pos_groups"])
    taps["pos_conv"] = x
    bias = position_bias(sd["encoder.layers.0.self_attn.relative_attention_bias.weight"], x.shape[1],
                         cfg["num_buckets"], cfg["max_distance"], dt)
    for i in range(cfg["encoder_layers"]):
        x = block(sd, cfg, i, x, bias)
        if i == 0:
            taps["block0"] = x
    taps["out"] = layer_norm(x, P("encoder.layer_norm.weight"), P("encoder.layer_norm.bias"))
    return taps
