"""NumPy restatement of what whole-recording WavLM extraction adds to tests/wavlm_ref.py: the forward pass with a
padding mask and with layer taps (pinned to tests/golden/wavlm_long_*.npz, wavlm_ragged.npz, wavlm_layers.npz at 1e-9 by
tests/test_wavlm_long_cpu.py), and the contract of qpg_wavlm_attention_tiled_f32: its f64 value with an entrywise bound
from the inputs alone, an f32 evaluation in the kernel's order, and the mistakes a tiled masked kernel could make."""
import numpy as np

from oracle.vqtrain_oracle import U, gamma
from qpgesture_amd import wavlm as W
from tests import wavlm_ref as R

LQ, LK = 128, 64            # QPG: queries per block and keys per tile of wavlm_attn_tiled_kernel
EPI = R.EPI


# ---- the forward pass with a padding mask and layer taps ------------------------------------------------------------
def frame_mask(padding_mask, T):
    """WavLM.forward_padding_mask: the n % T trailing columns dropped, viewed as (B, T, -1), a frame is masked when ALL
    of its samples are."""
    pm = np.asarray(padding_mask, bool)
    extra = pm.shape[1] % T
    if extra:
        pm = pm[:, :-extra]
    return pm.reshape(pm.shape[0], T, -1).all(-1)


def attention_masked(q, k, v, gate_f, bias, H, key_mask=None):
    """R.attention with the masked keys ([B][T] bool) excluded for every query of their batch member."""
    B, T, D = q.shape
    dt = q.dtype

    def heads(a):
        return a.reshape(B, T, H, D // H).transpose(0, 2, 1, 3)
    s = heads(q) @ heads(k).transpose(0, 1, 3, 2)
    s = s + gate_f.transpose(0, 2, 1)[..., None] * bias[None]
    if key_mask is not None:
        s = np.where(np.asarray(key_mask, bool)[:, None, None, :], -np.inf, s)
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    return (p @ heads(v)).transpose(0, 2, 1, 3).reshape(B, T, D).astype(dt)


def block_masked(sd, cfg, i, x, bias, key_mask=None):
    dt = x.dtype
    H = cfg["encoder_attention_heads"]
    p = "encoder.layers.%d." % i
    a = p + "self_attn."

    def P(name):
        return np.asarray(sd[name], dt)
    h = R.layer_norm(x, P(p + "self_attn_layer_norm.weight"), P(p + "self_attn_layer_norm.bias"))
    gf = R.gate(h, P(a + "grep_linear.weight"), P(a + "grep_linear.bias"), P(a + "grep_a"), H)
    q = R.linear(h, P(a + "q_proj.weight"), P(a + "q_proj.bias")) * dt.type((x.shape[2] // H) ** -0.5)
    ctx = attention_masked(q, R.linear(h, P(a + "k_proj.weight"), P(a + "k_proj.bias")),
                           R.linear(h, P(a + "v_proj.weight"), P(a + "v_proj.bias")), gf, bias, H, key_mask)
    x = x + R.linear(ctx, P(a + "out_proj.weight"), P(a + "out_proj.bias"))
    h = R.layer_norm(x, P(p + "final_layer_norm.weight"), P(p + "final_layer_norm.bias"))
    return x + R.linear(R.gelu(R.linear(h, P(p + "fc1.weight"), P(p + "fc1.bias"))), P(p + "fc2.weight"), P(p + "fc2.bias"))


def forward_long(sd, cfg, wav, dt=np.float64, padding_mask=None, output_layer=None):
    """The reference's extract_features in inference, its order kept (WavLM.py:311-375, 572-612):
      the conv stack over the samples as given, layer_norm, the frame mask, post_extract_proj ("front_end");
      masked frames of x set to 0, THEN x + GELU(pos_conv(x)) ("pos_conv": the encoder works in place, so this is also
      what the reference hands out as res["features"], i.e. for ret_conv=True);
      the blocks, masked frames excluded as keys, padded query rows computed like any other;
      output_layer = k (1-based): block k's output WITHOUT the final LayerNorm, layer_results = the encoder input and
      the outputs of blocks 1..k as (T, B, D); output_layer None: the final LayerNorm, no layer results.
    -> dict(front_end, pos_conv, x, frame_mask (None without padding_mask), layer_results)."""
    cfg = dict(W.CFG_DEFAULTS, **cfg)
    D = cfg["encoder_embed_dim"]

    def P(name):
        return np.asarray(sd[name], dt)
    f = R.feature_extractor(sd, cfg, wav, dt)
    x = R.layer_norm(f, P("layer_norm.weight"), P("layer_norm.bias"))
    fm = None if padding_mask is None else frame_mask(padding_mask, f.shape[1])
    if f.shape[2] != D:
        x = R.linear(x, P("post_extract_proj.weight"), P("post_extract_proj.bias"))
    res = {"front_end": x, "frame_mask": fm}
    if fm is not None:
        x = np.where(fm[..., None], dt(0), x)
    weff = W.fold_weight_norm(sd["encoder.pos_conv.0.weight_g"], sd["encoder.pos_conv.0.weight_v"])
    if dt == np.float32:
        weff = weff.astype(np.float32)
    x = R.pos_conv(x, weff, P("encoder.pos_conv.0.bias"), cfg["conv_pos_groups"])
    res["pos_conv"] = x
    bias = R.position_bias(sd["encoder.layers.0.self_attn.relative_attention_bias.weight"], x.shape[1],
                           cfg["num_buckets"], cfg["max_distance"], dt)
    lr = [] if output_layer is None else [x.transpose(1, 0, 2)]
    for i in range(cfg["encoder_layers"] if output_layer is None else output_layer):
        x = block_masked(sd, cfg, i, x, bias, fm)
        if output_layer is not None:
            lr.append(x.transpose(1, 0, 2))
    if output_layer is None:
        x = R.layer_norm(x, P("encoder.layer_norm.weight"), P("encoder.layer_norm.bias"))
    res.update(x=x, layer_results=lr)
    return res


# ---- qpg_wavlm_attention_tiled_f32 ----------------------------------------------------------------------------------
def attention_tiled_bound(q, k, v, gate_f, relb, H, key_mask=None, key_tile=LK):
    """(value, bound), f64, of the tiled attention: q (scaled), k, v [B][T][H 64], gate_f [B][T][H], relb [2T-1][H] (entry
    k - q + T - 1), key_mask [B][T] (nonzero: excluded) or None.  R.attention_bound's derivation over the VALID keys of
    each batch member - masked keys enter neither the value nor the bound, whatever k and v hold there:
      score  ds = gamma(64) sum |q||k| + 2 U |gate bias|, the maximum taken over the valid keys;
      row    (2 max ds + gamma(n) + 8 U) sum_k p_k |v_k| with n the member's valid keys: a masked key is staged as zeros
             and its weight is an exact 0, so what it adds to the numerator chain and to the row sum is exact;
      s-max  U (sum p t |v| + (sum p t)(sum p |v|)), t_k = max - s_k.  The kernel subtracts the RUNNING maximum m_j of
             key k's tile and later multiplies by exp(m_j - m_j+1), exp(m_j+1 - m_j+2), ..: the subtractions' roundings
             are U (|s_k - m_j| + (m_j+1 - m_j) + ..) = U t_k, the same sum, since the running maximum only rises;
      online what the rescaling adds per key tile that holds a valid key: one expf and one product on the running
             numerator and on the running sum.  The factor is the SAME float for both, but it reaches only the keys of
             the earlier tiles, so it perturbs their weights relative to the later ones: EPI per live tile in the
             coefficient.
    An output whose member has no valid key has no value (NaN, bound inf); the caller excludes such members."""
    B, T, D = q.shape
    qh, kh = (R._heads(R._f64(a), H) for a in (q, k))
    valid = np.ones((B, T), bool) if key_mask is None else ~np.asarray(key_mask).astype(bool)
    vh = R._heads(np.where(valid[..., None], R._f64(v), 0.0), H)                            # (NaN at a masked key: never read)
    kh = np.where(valid[:, None, :, None], kh, 0.0)
    relb = R._f64(relb)
    idx = np.arange(T)[None, :] - np.arange(T)[:, None] + T - 1
    gb = R._f64(gate_f).transpose(0, 2, 1)[..., None] * relb[idx].transpose(2, 0, 1)[None]  # [B][H][q][k]
    vk = valid[:, None, None, :]
    s = np.where(vk, qh @ kh.transpose(0, 1, 3, 2) + gb, -np.inf)
    ds = np.where(vk, gamma(64) * (np.abs(qh) @ np.abs(kh).transpose(0, 1, 3, 2)) + 2 * U * np.abs(gb), 0.0)
    with np.errstate(invalid="ignore"):
        t = np.where(vk, s.max(-1, keepdims=True) - s, 0.0)
    e = np.where(vk, np.exp(-t), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = e / e.sum(-1, keepdims=True)
    nvalid = valid.sum(-1)
    pad = np.zeros((B, -(-T // key_tile) * key_tile), bool)
    pad[:, :T] = valid
    live = pad.reshape(B, -1, key_tile).any(-1).sum(-1)
    chain = np.array([gamma(max(int(n), 1)) + EPI * int(lt) for n, lt in zip(nvalid, live)])[:, None, None, None]
    coef = 2 * ds.max(-1, keepdims=True) + chain + EPI + U * (p * t).sum(-1, keepdims=True)
    back = lambda a: a.transpose(0, 2, 1, 3).reshape(B, T, D)                               # noqa: E731
    val, bnd = back(p @ vh), back(coef * (p @ np.abs(vh)) + U * ((p * t) @ np.abs(vh)))
    dead = (nvalid == 0)[:, None, None]
    return np.where(dead, np.nan, val), np.where(dead, np.inf, bnd)


# the order in which the kernel's two products visit a tile's keys and the 64 channels: step r of the second product
# takes keys (r & 3) + 8 (r >> 2) and that + 4 of each 32-key half; step j of the first channels j and 32 + j
KEY_ORDER = np.array([st * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk for st in range(2) for r in range(16) for lk in range(2)])
CH_ORDER = np.array([j + 32 * lk for j in range(32) for lk in range(2)])
FAULTS = ("mask ignored", "mask on queries", "window off by one", "table at q - k", "last tile dropped", "no rescale")


def attention_tiled_eval(q, k, v, gate_f, relb, H, key_mask=None, dt=np.float32, fault=None):
    """The tiled attention in dtype dt in the kernel's order: per key tile of LK the score chains over the channels
    (CH_ORDER), + gate * bias; the tile maximum, the running maximum, alpha = exp(m - m'); the weights exp(s - m'), their
    sum by register and lane half; l = l alpha + sum, O = O alpha, then the numerator chain over the tile's keys
    (KEY_ORDER); one divide at the end.  A product and an add are rounded separately where the device's FMA rounds once.
    Masked keys are skipped (the kernel adds an exact 0 for them), a tile without a valid key is skipped as a whole.
    fault: one of FAULTS - the mistakes the controls of tests/test_wavlm_long_cpu.py evaluate in f64."""
    assert fault is None or fault in FAULTS
    B, T, D = q.shape
    qh, kh, vh = (R._heads(np.asarray(a, dt), H) for a in (q, k, v))
    gate_f, relb = np.asarray(gate_f, dt), np.asarray(relb, dt)
    mask = np.zeros((B, T), bool) if key_mask is None else np.asarray(key_mask).astype(bool)
    valid = ~mask if fault not in ("mask ignored", "mask on queries") else np.ones((B, T), bool)
    qs = np.arange(T)
    out = np.zeros((B, H, T, 64), dt)
    tiles = list(range(0, T, LK))
    if fault == "last tile dropped":
        tiles = tiles[:-1]
    for b in range(B):
        m, l = np.full((H, T), -np.inf, dt), np.zeros((H, T), dt)
        acc = np.zeros((H, T, 64), dt)
        for k0 in tiles:
            order = k0 + KEY_ORDER
            order = order[order < T]
            ks = order[valid[b, order]]                        # the tile's valid keys in the numerator chain's order
            if len(ks) == 0:
                continue
            s = np.zeros((H, T, len(ks)), dt)
            kt, vt = kh[b][:, ks], vh[b][:, ks]                # [H][keys][64]
            for c in CH_ORDER:
                s = s + qh[b][:, :, None, c] * kt[:, None, :, c]
            idx = ks[None, :] - qs[:, None] + T - 1
            if fault == "table at q - k":
                idx = qs[:, None] - ks[None, :] + T - 1
            if fault == "window off by one" and k0 > 0:        # the staged window of a later tile starts one entry late
                idx = np.minimum(idx + 1, 2 * T - 2)
            s = s + gate_f[b].T[..., None] * relb[idx].transpose(2, 0, 1)
            mn = np.maximum(m, s.max(-1))
            with np.errstate(invalid="ignore"):
                alpha = np.exp(m - mn)
            p = np.exp(s - mn[..., None])
            half = ((ks - k0) >> 2) & 1                        # the lane half (lane >> 5) that holds the key
            rs = [np.zeros((H, T), dt), np.zeros((H, T), dt)]
            for j in np.argsort(((ks - k0) >> 5) * 64 + (((ks - k0) & 31) >> 3) * 4 + ((ks - k0) & 3), kind="stable"):
                rs[half[j]] = rs[half[j]] + p[..., j]          # (per lane: registers in order st, r)
            if fault != "no rescale":
                l, acc = l * alpha, acc * alpha[..., None]
            l = l + (rs[0] + rs[1])
            for j in range(len(ks)):
                acc = acc + p[..., j, None] * vt[:, None, j, :]
            m = mn
        with np.errstate(invalid="ignore", divide="ignore"):
            out[b] = acc / l[..., None]
        if fault == "mask on queries":
            out[b][:, mask[b]] = 0
    assert out.dtype == dt
    return out.transpose(0, 2, 1, 3).reshape(B, T, D)


# ---- the cases (shared by the CPU and the GPU tests) ----------------------------------------------------------------
TILED_T = (1, 17, LK - 1, LK, LK + 1, LQ - 1, LQ, LQ + 1, 255, 256, 257, 300, 513, 1031)       # LQ + 1 = 2 LK + 1
MASKS = ("none", "1 valid", "LK-1 valid", "LK+1 valid", "T-1 valid", "hole")


def mask_of(kind, T, B):
    """[B][T] uint8 (1: excluded) or None.  Suffix masks leave the first n keys; "hole" masks an interior stretch that
    covers a whole key tile and parts of its neighbours, plus a lone key, and differs per batch member.  None when T is too
    short for the kind."""
    if kind == "none":
        return None
    mk = np.zeros((B, T), np.uint8)
    if kind == "hole":
        if T < 3 * LK:
            return None
        for b in range(B):
            mk[b, LK - 3 - b:2 * LK + 5 + b] = 1               # all of tile 1, the end of tile 0, the start of tile 2
            mk[b, T - 2 - b] = 1
        return mk
    n = {"1 valid": 1, "LK-1 valid": LK - 1, "LK+1 valid": LK + 1, "T-1 valid": T - 1}[kind]
    if not 1 <= n < T:
        return None
    mk[:, n:] = 1
    return mk


TILED_CASES = ([(T, B, H, mk, "random") for T in TILED_T for (B, H) in ((1, 1), (3, 3)) for mk in MASKS
                if mk == "none" or mask_of(mk, T, B) is not None]
               + [(300, 3, 3, "none", kind) for kind in ("zero q", "one hot", "gate 0")])


def tiled_case(T, B, H, mk, kind="random"):
    """R.attention_case plus key_mask; k and v hold NaN at the masked keys."""
    c = R.attention_case(T, B, H, kind)
    c["key_mask"] = mask_of(mk, T, B)
    if c["key_mask"] is not None:
        dead = c["key_mask"].astype(bool)
        c["k"], c["v"] = c["k"].copy(), c["v"].copy()
        c["k"][dead] = np.nan
        c["v"][dead] = np.nan
    return c


def tiled_bound_of(c):
    return attention_tiled_bound(c["q"], c["k"], c["v"], c["gate"], c["relb"], c["H"], c["key_mask"])
