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


# =====================================================================================================================
# The contract of the qpg_wavlm_* entry points: for each stage the f64 value AND a bound on every entry of the f32
# result, from the stage's inputs alone (tests/test_wavlm_contract_cpu.py, tests/test_gpu_wavlm_contract.py,
# DESIGN.md 4.10).  Constants: U = 2^-24 and oracle.vqtrain_oracle.gamma(n1, n2, ..) = 4 U sum sqrt(n_i) + 2 U, the
# coefficient of a value that went through f32 accumulation chains of those lengths (operand and store rounding in the
# 2 U); an element-wise tail of a handful of roundings gets 8 U of the magnitudes it combines, one add 2 U.
# Every function below named *_bound returns (value, bound), both f64, bound >= 0, and reads nothing of the device.
# =====================================================================================================================
from oracle.vqtrain_oracle import U, bound_ratio, gamma  # noqa: E402

EPI = 8 * U                 # erff / expf and the three or four roundings around them
KCHUNK = 512                # QPG: k per FMA chain of wavlm_gemm_kernel
# sup |GELU'(x)| = sup |Phi(x) + x phi(x)| = 1.1289.. (at x = sqrt 2): an error e ahead of the GELU is at most this
# times e behind it
GELU_LIP = 1.13
SENTINEL = 7.0


def _f64(a):
    return np.asarray(a, np.float64)


def ratio(got, val, bnd):
    """Largest |got - val| / bnd over the entries; inf if any entry of got is not finite."""
    got = _f64(got)
    if not np.isfinite(got).all():
        return float("inf")
    return bound_ratio(got, _f64(val), _f64(bnd), 1.0)


def _gelu_tail(pre, bnd):
    """GELU behind a value `pre` known to `bnd`: the error carried through (GELU_LIP) plus x * 0.5, x * sqrt(.5), erff,
    1 +, * - EPI of |pre| + 1 (|GELU(x)| <= |x|, the erf factor is at most 2)."""
    return gelu(pre), GELU_LIP * bnd + EPI * (np.abs(pre) + 1.0)


# ---- GEMM -----------------------------------------------------------------------------------------------------------
def gemm_bound(A, Wt, bias=None, gelu_on=0, residual=None):
    """A [.., M, K], Wt [.., N, K] (broadcast over the leading axes), bias [.., 1, N] or [N], residual [.., M, N].
    An output is sum_k a w over ceil(K / 512) FMA chains of min(K, 512) products each, the chains' sums added in k order
    (one more chain of that many terms), plus the bias: every partial sum is at most S = sum |a||w| + |bias| in size, so
    |error| <= gamma(min(K, 512), ceil(K / 512)) S.  GELU: _gelu_tail.  Residual: one more add, 2 U (|value| + |r|)."""
    A, Wt = _f64(A), _f64(Wt)
    K = A.shape[-1]
    pre = A @ np.swapaxes(Wt, -1, -2)
    mag = np.abs(A) @ np.abs(np.swapaxes(Wt, -1, -2))
    if bias is not None:
        pre, mag = pre + _f64(bias), mag + np.abs(_f64(bias))
    val, bnd = pre, gamma(min(K, KCHUNK), -(-K // KCHUNK)) * mag
    if gelu_on:
        val, bnd = _gelu_tail(pre, bnd)
    if residual is not None:
        r = _f64(residual)
        bnd = bnd + 2 * U * (np.abs(val) + np.abs(r))
        val = val + r
    return val, bnd


def gemm_f32(A, Wt, bias=None, gelu_on=0, residual=None):
    """The same in f32 in the kernel's stated order: k ascending, a product and an add each rounded (two roundings where
    the FMA has one), a fresh chain every 512 k, the chains' sums added in k order."""
    A, Wt = np.asarray(A, np.float32), np.asarray(Wt, np.float32)
    K = A.shape[-1]
    shape = np.broadcast_shapes(A.shape[:-2], Wt.shape[:-2]) + (A.shape[-2], Wt.shape[-2])
    acc, tot = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    for k in range(K):
        acc = acc + A[..., :, None, k] * Wt[..., None, :, k]
        if (k + 1) % KCHUNK == 0 or k + 1 == K:
            tot, acc = tot + acc, np.zeros(shape, np.float32)
    assert tot.dtype == np.float32
    if bias is not None:
        tot = tot + np.asarray(bias, np.float32)
    if gelu_on:
        tot = gelu(tot)
    if residual is not None:
        tot = tot + np.asarray(residual, np.float32)
    return tot


def gemm_problem(name, M, N, K, bias=True, gelu_on=0, res=False, lda=None, ldc=None, n_outer=1, n_inner=1, form="plain",
                 inplace=False, seed=0):
    """One qpg_wavlm_gemm_f32 call as flat f32 buffers and the arguments.  A's padding (between rows when lda > K, behind
    the last row) and the residual's padding columns hold NaN; `out0` is what the output buffer holds before the call
    (SENTINEL, or the residual for the in-place form).
      plain    one problem, rows lda apart;
      conv     the conv stack's form: n_outer batches of T_in = s (M - 1) + k frames of C = N channels, lda = s C,
               K = k C, so that a batch's last row ends at the batch's last float and the next batch follows directly;
      batched  n_outer x n_inner problems, W, bias and the output's column block per inner."""
    rng = np.random.Generator(np.random.PCG64([seed, M, N, K]))
    lda = K if lda is None else lda
    p = dict(name=name, M=M, N=N, K=K, gelu=int(gelu_on), n_outer=n_outer, n_inner=n_inner, lda=lda, inplace=inplace,
             a_outer=0, a_inner=0, w_inner=0, bias_inner=0, c_outer=0, c_inner=0)
    tail = np.full(16, np.nan, np.float32)
    if form == "plain":
        assert n_outer == n_inner == 1
        a = np.full((M - 1) * lda + K, np.nan, np.float32)
        for m in range(M):
            a[m * lda:m * lda + K] = rng.standard_normal(K)
        p["ldc"] = N if ldc is None else ldc
    elif form == "conv":
        C, k, s = N, K // N, lda // N
        assert n_inner == 1 and K == k * C and lda == s * C
        t_in = s * (M - 1) + k
        a = rng.standard_normal(n_outer * t_in * C).astype(np.float32)
        p.update(a_outer=t_in * C, ldc=N if ldc is None else ldc)
        p["c_outer"] = M * p["ldc"]
    else:
        assert form == "batched"
        a = rng.standard_normal(n_outer * n_inner * M * K).astype(np.float32)
        p["ldc"] = n_inner * N if ldc is None else ldc
        p.update(a_outer=n_inner * M * K, a_inner=M * K, w_inner=N * K, bias_inner=N, c_outer=M * p["ldc"], c_inner=N)
    p["a"] = np.concatenate([a, tail])
    p["w"] = (rng.standard_normal(n_inner * N * K) / np.sqrt(K)).astype(np.float32)
    p["bias"] = (rng.standard_normal(n_inner * N) * 0.5).astype(np.float32) if bias else None
    idx = gemm_index(p)
    size = int(idx["out"].max()) + 1 + 8
    p["out0"] = np.full(size, SENTINEL, np.float32)
    p["r"] = None
    if res:
        r = np.full(size, np.nan, np.float32)
        r[idx["out"]] = rng.standard_normal(idx["out"].shape)
        if inplace:
            p["out0"][idx["out"]] = r[idx["out"]]
        p["r"] = r
    return p


def gemm_index(p):
    """Flat offsets of a problem: a [Z0][Z1][M][K], w [Z1][N][K], bias [Z1][1][N], out [Z0][Z1][M][N]."""
    z0, z1 = np.arange(p["n_outer"])[:, None, None, None], np.arange(p["n_inner"])[None, :, None, None]
    m = np.arange(p["M"])[None, None, :, None]
    n, k = np.arange(p["N"])[None, None, None, :], np.arange(p["K"])[None, None, None, :]
    return dict(a=z0 * p["a_outer"] + z1 * p["a_inner"] + m * p["lda"] + k,
                w=(z1 * p["w_inner"] + np.arange(p["N"])[None, None, :, None] * p["K"] + k)[0],
                bias=(z1 * p["bias_inner"] + n)[0],
                out=z0 * p["c_outer"] + z1 * p["c_inner"] + m * p["ldc"] + n)


def gemm_gather(p, r_ldc=None):
    """(A, Wt, bias, residual) of a problem, gathered from its buffers (r_ldc: read the residual with another stride)."""
    idx = gemm_index(p)
    res = None
    if p["r"] is not None:
        ri = idx["out"] if r_ldc is None else gemm_index(dict(p, ldc=r_ldc, c_outer=p["c_outer"] // p["ldc"] * r_ldc))["out"]
        res = p["r"][ri]
    return p["a"][idx["a"]], p["w"][idx["w"]], None if p["bias"] is None else p["bias"][idx["bias"]], res


def gemm_problem_bound(p):
    return gemm_bound(*gemm_gather(p)[:3], p["gelu"], gemm_gather(p)[3])


def gemm_problem_f32(p):
    return gemm_f32(*gemm_gather(p)[:3], p["gelu"], gemm_gather(p)[3])


def _g(name, M, N, K, **kw):
    return name, dict(M=M, N=N, K=K, **kw)


GEMM_CASES = dict([
    _g("1x1x32", 1, 1, 32),                                   # the smallest admitted shape
    _g("129x48x16", 129, 48, 16),                             # one k-tile, a partial second column tile, a row past a row tile
    _g("65x129x528", 65, 129, 528),                           # a column past a column tile, a chunk plus one k-tile
    _g("200x160x512", 200, 160, 512),                         # exactly one chunk
    _g("64x96x1536", 64, 96, 1536),                           # three chunks
    _g("98x768x3072", 98, 768, 3072), _g("98x3072x768", 98, 3072, 768),        # the base widths
    _g("lda=K+12", 70, 40, 64, lda=76),
    _g("ldc=N+8", 70, 40, 64, ldc=48, res=True),
] + [_g("epilogue b%dg%dr%d" % (b, g, r), 64, 32, 64, bias=bool(b), gelu_on=g, res=bool(r))
     for b in (0, 1) for g in (0, 1) for r in (0, 1)] + [
    _g("in place K=1024", 130, 72, 1024, res=True, inplace=True),
    _g("conv form", 397, 64, 192, lda=128, n_outer=3, form="conv", bias=False),
    _g("batched", 130, 48, 32, n_outer=2, n_inner=3, form="batched", gelu_on=1, res=True, ldc=152),
])


def gemm_case(name):
    return gemm_problem(name, **GEMM_CASES[name])


# ---- conv0 ----------------------------------------------------------------------------------------------------------
def conv0_windows(wav, k, s, shift_last_of_8=False):
    """[B][T][k]: frame t's samples wav[b][s t + j]."""
    n = wav.shape[1]
    T = (n - k) // s + 1
    t = np.arange(T)
    if shift_last_of_8:                                       # (a negative control: frame 7 of a group reads frame 8's)
        t = np.where((t % 8 == 7) & (t + 1 < T), t + 1, t)
    return wav[:, t[:, None] * s + np.arange(k)[None, :]]


def conv0_bound(wav, w, bias, k, s, **kw):
    """out[b][t][c] = bias[c] + sum_j w[c][j] wav[b][s t + j]: one FMA chain of k products, then the bias:
    gamma(k) (sum |w||x| + |bias|)."""
    win, w = conv0_windows(_f64(wav), k, s, **kw), _f64(w)
    val, mag = win @ w.T, np.abs(win) @ np.abs(w).T
    if bias is not None:
        val, mag = val + _f64(bias), mag + np.abs(_f64(bias))
    return val, gamma(k) * mag


def conv0_f32(wav, w, bias, k, s):
    win, w = conv0_windows(np.asarray(wav, np.float32), k, s), np.asarray(w, np.float32)
    acc = np.zeros(win.shape[:2] + (w.shape[0],), np.float32)
    for j in range(k):
        acc = acc + win[:, :, None, j] * w[None, None, :, j]
    return acc + np.asarray(bias, np.float32) if bias is not None else acc


CONV0_CASES = [(T, C, k, s, b) for T in (1, 7, 8, 9, 17) for (C, k, s) in ((64, 10, 5), (5, 3, 2), (64, 1, 1))
               for b in (1, 0)]


def conv0_case(T, C, k, s, with_bias, B=3):
    """B rows of exactly n = s (T - 1) + k samples, one after the other; NaN behind the last."""
    rng = np.random.Generator(np.random.PCG64([11, T, C, k, s]))
    n = s * (T - 1) + k
    return dict(B=B, n=n, T=T, C=C, k=k, s=s, wav=rng.standard_normal((B, n)).astype(np.float32),
                w=rng.standard_normal((C, k)).astype(np.float32),
                bias=rng.standard_normal(C).astype(np.float32) if with_bias else None)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
def layernorm_bound(x, g, b, gelu_on=0, eps=1e-5, mean_channels=None):
    """Rows of C.  The kernel: lane l adds x[l], x[l + 64], .. (ceil(C / 64) terms), six shuffle steps add the lanes,
    / C; the same for sum d^2 of the centred d = x - mean; rstd = 1 / sqrt(var + eps); (d rstd) g + b.
      mean   |dm| <= gamma(ceil(C / 64), 6) mean|x|                                   (G below);
      d      |dd| <= dm + U |d|                                       (the mean's error, and the subtraction's rounding);
      var    sum (d + e)^2 / C with e = -dm + (rounding of d): the cross term with the common shift is 2 dm sum d / C = 0,
             what is left is dm^2 + 2 U var, and the summation adds G var (positive terms): dvar <= (G + 2 U) var + dm^2;
      rstd   relative error dvar / (2 (var + eps)) + 3 U                                  (the add, the sqrt, the divide);
      out    |g| rstd dd + |g xhat| rel(rstd) + 4 U (|g xhat| + |b|)                            (two products, one add).
    A row of large mean earns a large dm and with it a large bound; a well-conditioned row a tight one.
    mean_channels: a negative control, the mean over the first that many channels only."""
    x, g, b = _f64(x), _f64(g), _f64(b)
    C = x.shape[-1]
    G = gamma(-(-C // 64), 6)
    mean = x.mean(-1, keepdims=True) if mean_channels is None else x[..., :mean_channels].mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    dm = G * np.abs(x).mean(-1, keepdims=True)
    dd = dm + U * np.abs(d)
    rel = 0.5 * ((G + 2 * U) * var + dm * dm) / (var + eps) + 3 * U
    gx = g * d * rstd
    val = gx + b
    bnd = np.abs(g) * rstd * dd + np.abs(gx) * rel + 4 * U * (np.abs(gx) + np.abs(b))
    return _gelu_tail(val, bnd) if gelu_on else (val, bnd)


def _lane_sums32(terms):
    """f32 [.., n] -> [..]: lane l adds terms l, l + 64, .. in order, then wave_sum's xor steps 32, 16, .., 1."""
    n = terms.shape[-1]
    pad = np.zeros(terms.shape[:-1] + (-(-n // 64) * 64,), np.float32)
    pad[..., :n] = terms
    pad = pad.reshape(terms.shape[:-1] + (-1, 64))
    s = np.zeros(terms.shape[:-1] + (64,), np.float32)
    for i in range(pad.shape[-2]):
        s = s + pad[..., i, :]
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., np.arange(64) ^ o]
    return s[..., 0]


def layernorm_f32(x, g, b, gelu_on=0, eps=1e-5):
    x, g, b = (np.asarray(a, np.float32) for a in (x, g, b))
    C = np.float32(x.shape[-1])
    mean = (_lane_sums32(x) / C)[..., None]
    d = x - mean
    rstd = (np.float32(1) / np.sqrt(_lane_sums32(d * d) / C + np.float32(eps)))[..., None]
    y = d * rstd * g + b
    assert y.dtype == np.float32
    return gelu(y) if gelu_on else y


LN_CASES = [(M, C, ge) for M in (1, 3, 4, 5) for C in (1, 4, 63, 64, 65, 768) for ge in (0, 1)]


def layernorm_case(M, C, seed=0):
    """Rows of differing scale and offset; with M >= 3 the last row has a mean of 1000 against a spread of 0.01 and the one
    before it is constant (variance 0)."""
    rng = np.random.Generator(np.random.PCG64([21, M, C, seed]))
    x = rng.standard_normal((M, C)) * rng.uniform(0.1, 3.0, (M, 1)) + rng.standard_normal((M, 1))
    if M >= 3:
        x[M - 1] = 1000.0 + 0.01 * rng.standard_normal(C)
        x[M - 2] = 0.37
    return dict(M=M, C=C, x=x.astype(np.float32), g=rng.uniform(0.6, 1.4, C).astype(np.float32),
                b=(rng.standard_normal(C) * 0.1).astype(np.float32))


# ---- gate -----------------------------------------------------------------------------------------------------------
def gate_bound(h, gw, gb, ga, H):
    """h [M][H 64].  Each of the 8 sums is one FMA chain of 64 and its bias: gamma(64) (sum |x||w| + |bias|).  A 4-sum
    adds four of them in two levels: their errors, and 2 U of the sum of their sizes.  sigmoid' = sig (1 - sig) carries
    that through; expf, 1 +, 1 / add 4 U sig - so a saturated sigmoid (expf overflows to inf, or underflows to 0) is
    within its bound at exactly 0 or 1.  gate = a (b grep_a - 1) + 2: the two errors through their partial derivatives,
    and 4 U of the magnitudes the four operations combine."""
    M = h.shape[0]
    x, gw, gb, ga = _f64(h).reshape(M, H, 64), _f64(gw), _f64(gb), _f64(ga).reshape(H)
    s = x @ gw.T + gb
    ds = gamma(64) * (np.abs(x) @ np.abs(gw).T + np.abs(gb))
    s4 = s.reshape(M, H, 2, 4)
    sums = s4.sum(-1)
    dsum = ds.reshape(M, H, 2, 4).sum(-1) + 2 * U * np.abs(s4).sum(-1)
    sig = 1.0 / (1.0 + np.exp(-sums))
    dsig = sig * (1.0 - sig) * dsum + 4 * U * sig
    a, b, da, db = sig[..., 0], sig[..., 1], dsig[..., 0], dsig[..., 1]
    val = a * (b * ga - 1.0) + 2.0
    bnd = np.abs(b * ga - 1.0) * da + a * np.abs(ga) * db + 4 * U * (a * (np.abs(b * ga) + 1.0) + 2.0)
    return val, bnd


def gate_f32(h, gw, gb, ga, H):
    M = h.shape[0]
    x, gw, gb, ga = (np.asarray(a, np.float32) for a in (h, gw, gb, ga))
    x = x.reshape(M, H, 64)
    s = np.zeros((M, H, 8), np.float32)
    for c in range(64):
        s = s + x[:, :, None, c] * gw[None, None, :, c]
    s = (s + gb).reshape(M, H, 2, 2, 2)
    sums = s[..., 0] + s[..., 1]
    sums = sums[..., 0] + sums[..., 1]
    with np.errstate(over="ignore"):
        sig = np.float32(1) / (np.float32(1) + np.exp(-sums))
    out = sig[..., 0] * (sig[..., 1] * ga.reshape(H) - np.float32(1)) + np.float32(2)
    assert out.dtype == np.float32
    return out


GATE_CASES = [(M, H, kind) for (M, H) in ((1, 1), (85, 3), (128, 2), (257, 1)) for kind in ("random", "saturated")]


def gate_case(M, H, kind):
    """saturated: weights scaled so that the 4-sums reach +-100 and beyond, where expf overflows."""
    rng = np.random.Generator(np.random.PCG64([31, M, H]))
    h = rng.standard_normal((M, H * 64)).astype(np.float32)
    gw, gb = rng.standard_normal((8, 64)) / 8, rng.standard_normal(8) * 0.1
    if kind == "saturated":
        gw = gw * 60.0
    return dict(M=M, H=H, h=h, gw=gw.astype(np.float32), gb=gb.astype(np.float32),
                ga=rng.uniform(0.5, 1.5, H).astype(np.float32))


# ---- attention ------------------------------------------------------------------------------------------------------
def _heads(a, H):
    B, T, D = a.shape
    return a.reshape(B, T, H, D // H).transpose(0, 2, 1, 3)


def attention_bound(q, k, v, gate_f, relb, H, swap_table=False, keys=None):
    """q (scaled), k, v [B][T][H 64], gate_f [B][T][H], relb [2T-1][H] (entry k - q + T - 1).
      score  s = (FMA chain of 64) + gate * bias: ds = gamma(64) sum |q||k| + 2 U |gate bias|   (the product, the add);
      row    the numerators are exp(s - max), so an error ds_k of the scores moves every softmax weight by a factor within
             exp(+-2 max_k ds); expf, the product e v and the divide are a few roundings: 8 U; the numerator sum_k e_k v_k is
             a chain of T, and the row sum is shorter: gamma(T).  To first order
             |error| <= (2 max_k ds + gamma(T) + 8 U) sum_k p_k |v_k|,  p the f64 softmax;
      s-max  one rounding that structure leaves out: the f32 subtraction s_k - max is off by U |s_k - max|, which is the
             relative error it gives e_k (40 U on a key 40 below the maximum - whose weight is e^-40).  Through the
             numerator and the row sum it adds U (sum_k p_k t_k |v_k| + (sum_k p_k t_k)(sum_k p_k |v_k|)), t_k = |s_k - max|.
    swap_table / keys: negative controls (the table read at q - k; only the first `keys` keys)."""
    B, T, D = q.shape
    qh, kh, vh = (_heads(_f64(a), H) for a in (q, k, v))
    relb = _f64(relb)
    idx = np.arange(T)[None, :] - np.arange(T)[:, None]
    bias = relb[(-idx if swap_table else idx) + T - 1].transpose(2, 0, 1)                  # [H][q][k]
    gb = _f64(gate_f).transpose(0, 2, 1)[..., None] * bias[None]                             # [B][H][q][k]
    s = qh @ kh.transpose(0, 1, 3, 2) + gb
    ds = gamma(64) * (np.abs(qh) @ np.abs(kh).transpose(0, 1, 3, 2)) + 2 * U * np.abs(gb)
    if keys is not None:
        s, ds, vh = s[..., :keys], ds[..., :keys], vh[:, :, :keys]
    t = s.max(-1, keepdims=True) - s
    e = np.exp(-t)
    p = e / e.sum(-1, keepdims=True)
    coef = 2 * ds.max(-1, keepdims=True) + gamma(T) + EPI + U * (p * t).sum(-1, keepdims=True)
    back = lambda a: a.transpose(0, 2, 1, 3).reshape(B, T, D)                               # noqa: E731
    return back(p @ vh), back(coef * (p @ np.abs(vh)) + U * ((p * t) @ np.abs(vh)))


def attention_f32(q, k, v, gate_f, relb, H):
    """f32 in the kernel's order: score chains over the 64 channels, + gate * bias; row maximum subtracted, expf, the row
    sum by lanes and shuffles; the numerator a chain over the keys; one divide."""
    B, T, D = q.shape
    qh, kh, vh = (_heads(np.asarray(a, np.float32), H) for a in (q, k, v))
    idx = np.arange(T)[None, :] - np.arange(T)[:, None] + T - 1
    bias = np.asarray(relb, np.float32)[idx].transpose(2, 0, 1)
    s = np.zeros((B, H, T, T), np.float32)
    for c in range(64):
        s = s + qh[:, :, :, None, c] * kh[:, :, None, :, c]
    s = s + np.asarray(gate_f, np.float32).transpose(0, 2, 1)[..., None] * bias[None]
    e = np.exp(s - s.max(-1, keepdims=True))
    rsum = _lane_sums32(e)
    acc = np.zeros((B, H, T, 64), np.float32)
    for j in range(T):
        acc = acc + e[:, :, :, j, None] * vh[:, :, None, j, :]
    out = acc / rsum[..., None]
    assert out.dtype == np.float32
    return out.transpose(0, 2, 1, 3).reshape(B, T, D)


ATT_T = (1, 15, 16, 17, 63, 64, 65, 255, 256)
ATT_CASES = ([(T, B, H, "random") for T in ATT_T for (B, H) in ((1, 1), (3, 3))]
             + [(65, 3, 3, kind) for kind in ("zero q", "one hot", "gate 0")])


def attention_case(T, B, H, kind="random"):
    """random: an asymmetric random table.  zero q: q and the table 0, every output the plain mean of v.  one hot: the
    table times 40, scores reach +-100 and rows are one-hot.  gate 0: the table switched off."""
    rng = np.random.Generator(np.random.PCG64([41, T, B, H]))
    D = H * 64
    q = (rng.standard_normal((B, T, D)) * 0.35).astype(np.float32)
    k, v = (rng.standard_normal((B, T, D)).astype(np.float32) for _ in range(2))
    gate_f = rng.uniform(0.7, 2.4, (B, T, H)).astype(np.float32)
    relb = rng.standard_normal((2 * T - 1, H)).astype(np.float32)
    if kind == "zero q":
        q, relb = np.zeros_like(q), np.zeros_like(relb)
    elif kind == "one hot":
        relb = relb * np.float32(40.0)
    elif kind == "gate 0":
        gate_f = np.zeros_like(gate_f)
    return dict(T=T, B=B, H=H, q=q, k=k, v=v, gate=gate_f, relb=relb)


# ---- pos_pad + the batched GEMM at the base width -------------------------------------------------------------------
POS_T = (1, 17, 130)
POS_D, POS_G, POS_K = 768, 16, 128


def pos_case(T, B=2):
    rng = np.random.Generator(np.random.PCG64([51, T]))
    D, G, K = POS_D, POS_G, POS_K
    Cg = D // G
    return dict(T=T, B=B, D=D, G=G, K=K, Cg=Cg, rows=T + K - 1, x=rng.standard_normal((B, T, D)).astype(np.float32),
                w=(rng.standard_normal((G, Cg, K * Cg)) / np.sqrt(Cg * K) * 2.0).astype(np.float32),   # [G][out][k][in]
                bias=(rng.standard_normal(D) * 0.1).astype(np.float32))


def pos_image(x, G, K):
    """qpg_wavlm_pos_pad_f32's image [B][G][T + K - 1][Cg]: x group-major behind K // 2 rows of zeros."""
    B, T, D = x.shape
    img = np.zeros((B, G, T + K - 1, D // G), x.dtype)
    img[:, :, K // 2:K // 2 + T] = x.reshape(B, T, G, D // G).transpose(0, 2, 1, 3)
    return img


def pos_operands(img, w, bias, x):
    """The batched GEMM's (A [B][G][T][K Cg], Wt [G][Cg][K Cg], bias [G][1][Cg], residual [B][G][T][Cg]) from the padded
    image: output frame t of group g reads the K Cg contiguous floats that start at its row t."""
    B, G, rows, Cg = img.shape
    w = w.reshape(G, Cg, -1)
    KC = w.shape[-1]
    T = rows - KC // Cg + 1
    flat = img.reshape(B, G, rows * Cg)
    A = flat[:, :, (np.arange(T) * Cg)[:, None] + np.arange(KC)[None, :]]
    return A, w, bias.reshape(G, 1, Cg), x.reshape(B, T, G, Cg).transpose(0, 2, 1, 3)


def pos_back(y):
    """[B][G][T][Cg] -> [B][T][D]."""
    B, G, T, Cg = y.shape
    return y.transpose(0, 2, 1, 3).reshape(B, T, G * Cg)
