"""NumPy restatement of the sentence encoder (a BERT-shaped post-LN encoder with mean-token pooling, as
sentence-transformers wraps transformers' BertModel) and of the reference's text-slot arithmetic, written from the model's
definition.  Every function runs in the dtype of its activations: f64 for the reference value, f32 for e32, the f32
evaluation's own error.  tests/test_sentence_cpu.py pins it to tests/golden/sentence_*.npz (transformers' f64 run) at 1e-9.

Sentences are handled one at a time, unpadded: that is what the packed layout of qpg_bert.hip computes, and what the padded,
masked batch of the reference equals (a padded key's weight is exactly 0, a padded query is left out of the mean)."""
import math

import numpy as np

try:
    from scipy.special import erf as _erf
except ImportError:                                            # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])

HEAD_DIM = 32


def gelu(x):
    return (x * x.dtype.type(0.5) * (1 + _erf(x * x.dtype.type(math.sqrt(0.5))).astype(x.dtype))).astype(x.dtype)


def layer_norm(x, g, b, eps):
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    return (d / np.sqrt(var + x.dtype.type(eps)) * g + b).astype(x.dtype)


def cast(sd, dt):
    return {k: np.asarray(v).astype(dt) for k, v in sd.items()}


def embed_ln(sd, ids, eps):
    """(L, D): LayerNorm((word[ids] + type[0]) + pos[0 .. L)) of one sentence."""
    e = "embeddings."
    x = sd[e + "word_embeddings.weight"][np.asarray(ids)] + sd[e + "token_type_embeddings.weight"][0]
    x = x + sd[e + "position_embeddings.weight"][:len(ids)]
    return layer_norm(x, sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"], eps)


def attention(q, k, v, H):
    """q, k, v (L, H 32), q NOT yet scaled -> (L, H 32): per head softmax(q k^T / sqrt 32) v, the row maximum subtracted."""
    L = q.shape[0]
    dt = q.dtype.type
    qh, kh, vh = (a.reshape(L, H, HEAD_DIM).transpose(1, 0, 2) for a in (q, k, v))
    s = qh @ kh.transpose(0, 2, 1) * dt(HEAD_DIM ** -0.5)
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    return (p @ vh).transpose(1, 0, 2).reshape(L, H * HEAD_DIM).astype(q.dtype)


def attention_prescaled(qkv, H):
    """The kernel's operand: qkv (L, 3 H 32) = q | k | v with q already scaled -> (L, H 32)."""
    L, D = qkv.shape[0], qkv.shape[1] // 3
    qh, kh, vh = (qkv[:, i * D:(i + 1) * D].reshape(L, H, HEAD_DIM).transpose(1, 0, 2) for i in range(3))
    s = qh @ kh.transpose(0, 2, 1)
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    return (p @ vh).transpose(1, 0, 2).reshape(L, D).astype(qkv.dtype)


def block(sd, i, x, H, eps):
    """Block i on one sentence's rows (L, D): LN(x + dense(attention(x))), then LN(x + fc2(gelu(fc1 x)))."""
    p = "encoder.layer.%d." % i
    a = p + "attention.self."

    def lin(name, t):
        return t @ sd[name + ".weight"].T + sd[name + ".bias"]
    att = attention(lin(a + "query", x), lin(a + "key", x), lin(a + "value", x), H)
    x = layer_norm(x + lin(p + "attention.output.dense", att), sd[p + "attention.output.LayerNorm.weight"],
                   sd[p + "attention.output.LayerNorm.bias"], eps)
    h = gelu(lin(p + "intermediate.dense", x))
    return layer_norm(x + lin(p + "output.dense", h), sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"], eps)


def mean_pool(x):
    """(D,): the token rows of (L, D) added in token order, divided by L."""
    return np.add.accumulate(x, axis=0)[-1] / x.dtype.type(x.shape[0])


def encode(sd, cfg, seqs, dt=np.float64):
    """{'pooled': (S, D), 'embed': (R, D), 'layer0': (R, D)}: the packed rows of the id lists `seqs`, in dtype dt."""
    sd = cast(sd, dt)
    H, eps = cfg["num_attention_heads"], cfg.get("layer_norm_eps", 1e-12)
    pooled, embed, layer0 = [], [], []
    for ids in seqs:
        x = embed_ln(sd, ids, eps)
        embed.append(x)
        for i in range(cfg["num_hidden_layers"]):
            x = block(sd, i, x, H, eps)
            if i == 0:
                layer0.append(x)
        pooled.append(mean_pool(x))
    return dict(pooled=np.stack(pooled), embed=np.concatenate(embed), layer0=np.concatenate(layer0))


def code_sentences(words, n_windows, n_frames=240, fps=60, num_frames_code=30):
    """The sentences of make_txt_dataset's code slots, restated: per window the words whose midpoint lies before its end
    (and that no earlier window took) go to slot int((start mod 4 + (end mod 4, or 4 where that is 0)) * 60 / 2 / 8); slot
    j's sentence is the words of slots max(j - 3, 0) .. min(j + 3, 29) in slot order, joined by blanks."""
    step = int(n_frames / num_frames_code)
    period = n_frames // fps
    left = list(words)
    out = []
    for i in range(n_windows):
        end_time = (i * n_frames + n_frames) / fps
        mine = []
        while left != [] and (left[0][0] + left[0][1]) / 2 < end_time:
            mine.append(left.pop(0))
        slots = {}
        for start, end, word in mine:
            e = end % period
            if e == 0:
                e = period
            slots.setdefault(int((start % period + e) * 60 / 2 / step), []).append(word)
        for j in range(num_frames_code):
            got = []
            for n in range(max(j - 3, 0), min(j + 4, num_frames_code)):
                got += slots.get(n, [])
            out.append(" ".join(got))
    return out
