"""WavLM feature extraction on the GPU: what the reference's wav_to_wavlm / wav2wavlm (process/make_beat_dataset.py
:328-385) get from `model.extract_features(wav)[0]` - inference of 4 s windows by default; with long_inputs=True whole
recordings of up to MAX_FRAMES_LONG frames (10.9 min), and at any length ragged batches (padding_mask) and the
per-layer outputs (output_layer, ret_layer_results, ret_conv) of the reference's signature.

    from qpgesture_amd.wavlm import WavLM, load_wavlm
    model = load_wavlm("WavLM-Large.pt", device="cuda:0")        # {'cfg': dict, 'model': state_dict}
    feats = model.extract_features(wav)[0]                       # (B, n) f32 -> (B, T, D) f32 on the device

    python -m qpgesture_amd.wavlm --wav clip.wav --WavLM_model_path WavLM-Large.pt --out test_wavlm.npz
    python -m qpgesture_amd.wavlm --wav clip.wav --WavLM_model_path WavLM-Large.pt --whole [--layer k]

The forward pass is a chain of the qpg_wavlm_* kernels of include/qpg.h; there is no torch
fallback: a configuration the kernels do not take raises NotImplementedError naming the field.  As in the reference the
input is not normalised although the Large cfg says normalize=True (`normalize_input=True` turns it on)."""
import argparse
import ast
import os

import numpy as np

MAX_FRAMES = 256          # QPG_WAVLM_MAX_FRAMES
MAX_FRAMES_LONG = 32768   # QPG_WAVLM_MAX_FRAMES_LONG (qpg_wavlm_attention_tiled_f32)
HEAD_DIM = 64             # QPG_WAVLM_HEAD_DIM
WINDOW = 64000            # 4 s at 16 kHz
SAMPLE_RATE = 16000

# the fields this module reads, with the values a cfg that omits them gets
CFG_DEFAULTS = dict(extractor_mode="default", encoder_layers=12, encoder_embed_dim=768, encoder_ffn_embed_dim=3072,
                    encoder_attention_heads=12, activation_fn="gelu", layer_norm_first=False,
                    conv_feature_layers="[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2", conv_bias=False,
                    normalize=False, conv_pos=128, conv_pos_groups=16, relative_position_embedding=False,
                    num_buckets=320, max_distance=1280, gru_rel_pos=False)


class WavLMConfig:
    """The checkpoint's cfg dict as attributes (fields it omits: CFG_DEFAULTS)."""

    def __init__(self, cfg=None):
        self.__dict__.update(CFG_DEFAULTS)
        if cfg is not None:
            self.update(cfg)

    def update(self, cfg):
        self.__dict__.update(cfg if isinstance(cfg, dict) else cfg.__dict__)


def _as_dict(cfg):
    return dict(CFG_DEFAULTS, **(cfg if isinstance(cfg, dict) else cfg.__dict__))


def conv_layers_of(cfg):
    """[(channels, kernel, stride), ...] of cfg['conv_feature_layers'] (a Python list expression of integer tuples)."""
    node = ast.parse(_as_dict(cfg)["conv_feature_layers"].strip(), mode="eval").body

    def ev(n):
        if isinstance(n, ast.BinOp) and isinstance(n.op, ast.Add):
            return ev(n.left) + ev(n.right)
        if isinstance(n, ast.BinOp) and isinstance(n.op, ast.Mult):
            a, b = ev(n.left), ev(n.right)
            return a * b
        return ast.literal_eval(n)
    return [tuple(int(v) for v in layer) for layer in ev(node)]


def check_supported(cfg):
    """Raise NotImplementedError naming the first cfg field the kernels do not take."""
    c = _as_dict(cfg)

    def need(field, ok, what):
        if not ok:
            raise NotImplementedError("WavLM cfg field %s = %r is not supported (%s)" % (field, c[field], what))
    need("extractor_mode", c["extractor_mode"] == "layer_norm", "only 'layer_norm'")
    need("layer_norm_first", bool(c["layer_norm_first"]), "only pre-LN blocks")
    need("activation_fn", c["activation_fn"] == "gelu", "only 'gelu'")
    need("relative_position_embedding", bool(c["relative_position_embedding"]), "the relative position bias is required")
    need("gru_rel_pos", bool(c["gru_rel_pos"]), "the gated relative position bias is required")
    D, F, H = c["encoder_embed_dim"], c["encoder_ffn_embed_dim"], c["encoder_attention_heads"]
    need("encoder_embed_dim", D % 64 == 0 and D > 0, "a multiple of 64")
    need("encoder_ffn_embed_dim", F % 64 == 0 and F > 0, "a multiple of 64")
    need("encoder_attention_heads", H > 0 and H * HEAD_DIM == D, "head dim must be %d" % HEAD_DIM)
    need("conv_pos_groups", c["conv_pos_groups"] > 0 and D % (4 * c["conv_pos_groups"]) == 0,
         "encoder_embed_dim / groups must be a multiple of 4")
    need("conv_pos", c["conv_pos"] >= 1 and c["conv_pos"] * (D // c["conv_pos_groups"]) % 16 == 0,
         "conv_pos * encoder_embed_dim / conv_pos_groups must be a multiple of 16")
    need("num_buckets", c["num_buckets"] >= 4 and c["num_buckets"] % 4 == 0, "a multiple of 4")
    need("max_distance", c["max_distance"] > c["num_buckets"] // 4, "above num_buckets / 4")
    need("encoder_layers", c["encoder_layers"] >= 1, "at least one block")
    try:
        layers = conv_layers_of(c)
        ok = (len(layers) >= 1 and all(len(x) == 3 and min(x) >= 1 for x in layers)
              and all(x[0] == layers[0][0] for x in layers) and layers[0][0] % 64 == 0)
    except (ValueError, SyntaxError, TypeError):
        ok = False
    need("conv_feature_layers", ok, "[(C,k0,s0)] + [(C,k,s)]* with C a multiple of 64")


def frames_of(n, layers):
    """Frame count after each conv layer for n samples (0 once the input is shorter than a kernel)."""
    out = []
    for _, k, s in layers:
        n = (n - k) // s + 1 if n >= k else 0
        out.append(n)
    return out


def relative_position_buckets(rel, num_buckets=320, max_distance=800):
    """Bucket of each relative position k - q (modules.py:417-442, bidirectional): half the buckets per sign, exact below
    a quarter, logarithmic up to max_distance.  The log range is evaluated in f32 in the reference's operation order
    (f32 ratio, f32 log, divided by the f64 constant rounded to f32, times the f32 bucket count, truncated)."""
    rel = np.asarray(rel, np.int64)
    nb = num_buckets // 2
    out = (rel > 0).astype(np.int64) * nb
    n = np.abs(rel)
    max_exact = nb // 2
    nf = np.maximum(n, 1).astype(np.float32)
    large = np.log(nf / np.float32(max_exact)) / np.float32(np.log(max_distance / max_exact)) * np.float32(nb - max_exact)
    large = np.minimum(max_exact + large.astype(np.int64), nb - 1)
    return out + np.where(n < max_exact, n, large)


def fold_weight_norm(g, v):
    """Effective pos_conv weight of weight_norm(dim=2): g v / ||v||, the norm over dims (0, 1) per kernel position.
    f64 in, f64 out (rounded once to f32 when it is loaded)."""
    g, v = np.asarray(g, np.float64), np.asarray(v, np.float64)
    return g * v / np.sqrt((v * v).sum(axis=(0, 1), keepdims=True))


def window_bounds(n_samples, n_frames=240, fps=60):
    """[(start, end)] sample ranges of a clip's windows by the arithmetic of process/make_test_data.py:17-33: the clip
    holds n_samples / 16000 * fps motion frames, floor((that - n_frames) / n_frames) + 1 whole windows of n_frames fit,
    window i starts at floor(i n_frames / fps * 16000) and is int(n_frames / fps * 16000) samples long.  A trailing part
    shorter than a window is dropped, as there."""
    import math
    minlen = n_samples / SAMPLE_RATE * fps
    num = math.floor((minlen - n_frames) / n_frames) + 1
    out = []
    for i in range(max(num, 0)):
        start = math.floor(i * n_frames / fps * SAMPLE_RATE)
        out.append((start, start + int(n_frames / fps * SAMPLE_RATE)))
    return out


class WavLM:
    """WavLM(cfg, device): the reference's WavLM(cfg).eval() for extract_features in inference.
    long_inputs=True (additive, off: more than MAX_FRAMES frames raise as before) admits up to MAX_FRAMES_LONG frames
    through the tiled attention kernel; a call of at most MAX_FRAMES frames without padding_mask takes the same launches
    and gives the same bits either way.
    normalize_input=True (additive, off as in the reference) normalises EACH WINDOW to zero mean and unit variance before
    the conv stack, so that a window's features do not depend on its batch; the upstream recipe's
    `layer_norm(wav, wav.shape)` takes one mean over the whole tensor, which is the same thing for its one-clip calls."""

    def __init__(self, cfg, device="cuda:0", normalize_input=False, long_inputs=False):
        import torch
        check_supported(cfg)
        self.cfg = WavLMConfig(_as_dict(cfg))
        self.device = torch.device(device)
        self.normalize_input = bool(normalize_input)
        self.long_inputs = bool(long_inputs)
        self.conv_layers = conv_layers_of(cfg)
        self.p = None
        self._relb = {}
        self._ws = {}

    # ---- parameters
    def load_state_dict(self, sd):
        import torch
        c = self.cfg
        D, H = c.encoder_embed_dim, c.encoder_attention_heads

        def get(name):
            if name not in sd:
                raise KeyError("WavLM state_dict lacks %r" % name)
            v = sd[name]
            return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)

        p = {"conv": []}
        cin = 1
        for i, (ch, k, s) in enumerate(self.conv_layers):
            pre = "feature_extractor.conv_layers.%d." % i
            w = get(pre + "0.weight")
            if w.shape != (ch, cin, k):
                raise ValueError("%s0.weight has shape %s, the cfg says %s" % (pre, w.shape, (ch, cin, k)))
            p["conv"].append(dict(w=dev(w.transpose(0, 2, 1).reshape(ch, k * cin)),      # [Cout][k][Cin]
                                  b=dev(get(pre + "0.bias")) if c.conv_bias else None,
                                  g=dev(get(pre + "2.1.weight")), beta=dev(get(pre + "2.1.bias"))))
            cin = ch
        p["ln_g"], p["ln_b"] = dev(get("layer_norm.weight")), dev(get("layer_norm.bias"))
        p["proj_w"] = dev(get("post_extract_proj.weight")) if cin != D else None
        p["proj_b"] = dev(get("post_extract_proj.bias")) if cin != D else None
        K, G = c.conv_pos, c.conv_pos_groups
        Cg = D // G
        weff = fold_weight_norm(get("encoder.pos_conv.0.weight_g"), get("encoder.pos_conv.0.weight_v"))     # [D][Cg][K]
        p["pos_w"] = dev(weff.reshape(G, Cg, Cg, K).transpose(0, 1, 3, 2))                                 # [G][Cg out][K][Cg in]
        p["pos_b"] = dev(get("encoder.pos_conv.0.bias"))
        p["rel_emb"] = get("encoder.layers.0.self_attn.relative_attention_bias.weight").astype(np.float32)   # [buckets][H]
        scaling = np.float32(HEAD_DIM ** -0.5)                 # (a power of two: folding it into q's weights is exact)
        p["layers"] = []
        for i in range(c.encoder_layers):
            pre = "encoder.layers.%d." % i
            a = pre + "self_attn."
            wq, bq = get(a + "q_proj.weight") * scaling, get(a + "q_proj.bias") * scaling
            p["layers"].append(dict(
                ln1_g=dev(get(pre + "self_attn_layer_norm.weight")), ln1_b=dev(get(pre + "self_attn_layer_norm.bias")),
                qkv_w=dev(np.concatenate([wq, get(a + "k_proj.weight"), get(a + "v_proj.weight")], 0)),
                qkv_b=dev(np.concatenate([bq, get(a + "k_proj.bias"), get(a + "v_proj.bias")], 0)),
                out_w=dev(get(a + "out_proj.weight")), out_b=dev(get(a + "out_proj.bias")),
                grep_w=dev(get(a + "grep_linear.weight")), grep_b=dev(get(a + "grep_linear.bias")),
                grep_a=dev(get(a + "grep_a").reshape(H)),
                ln2_g=dev(get(pre + "final_layer_norm.weight")), ln2_b=dev(get(pre + "final_layer_norm.bias")),
                fc1_w=dev(get(pre + "fc1.weight")), fc1_b=dev(get(pre + "fc1.bias")),
                fc2_w=dev(get(pre + "fc2.weight")), fc2_b=dev(get(pre + "fc2.bias"))))
        p["fin_g"], p["fin_b"] = dev(get("encoder.layer_norm.weight")), dev(get("encoder.layer_norm.bias"))
        self.p = p
        self._relb = {}
        return self

    def position_bias_table(self, T):
        """[2T-1][H] device table: entry k - q + T - 1 is layer 0's bias embedding of bucket(k - q); every block reads it."""
        import torch
        if T not in self._relb:
            if T > MAX_FRAMES:                   # whole recordings come in every length: one long table is kept
                for old in [t for t in self._relb if t > MAX_FRAMES]:
                    del self._relb[old]
            b = relative_position_buckets(np.arange(-(T - 1), T), self.cfg.num_buckets, self.cfg.max_distance)
            self._relb[T] = torch.from_numpy(np.ascontiguousarray(self.p["rel_emb"][b])).to(self.device)
        return self._relb[T]

    # ---- the forward pass
    def _workspace(self, B, n):
        """Device buffers for a (B, n) call; kept, and reused by every later call that fits (wav_to_wavlm: sized once)."""
        import torch
        c = self.cfg
        fr = frames_of(n, self.conv_layers)
        C, D, F = self.conv_layers[0][0], c.encoder_embed_dim, c.encoder_ffn_embed_dim
        T = fr[-1]
        rows = T + c.conv_pos - 1
        need = dict(a=B * fr[0] * C, b=B * (fr[1] if len(fr) > 1 else 0) * C, x=B * T * D, y=B * T * D, h=B * T * D,
                    att=B * T * D, qkv=B * T * 3 * D, ffn=B * T * max(F, 1), pad=B * rows * D,
                    gate=B * T * c.encoder_attention_heads)
        for k, v in need.items():
            if k not in self._ws or self._ws[k].numel() < v:
                self._ws[k] = torch.empty(max(v, 4), dtype=torch.float32, device=self.device)
        return self._ws

    def extract_features(self, source, padding_mask=None, mask=False, ret_conv=False, output_layer=None,
                         ret_layer_results=False):
        """(B, n) f32 samples -> ((B, T, D) f32 device tensor, frame mask): the reference's signature and return shape
        (WavLM.py:323-375), its quirks included.
          padding_mask       (B, n) bool, True = padding.  A frame is masked when all of its n // T samples are (the n % T
                             trailing columns dropped); the conv stack still runs over the samples as given; masked frames
                             are zeroed behind post_extract_proj and excluded as keys in every block; their own rows are
                             computed like any other.  Returned: the (B, T) bool frame mask on the device (None without
                             padding_mask).  A batch member without a valid frame raises ValueError (the reference
                             returns NaN rows).
          output_layer = k   (1-based) block k's output WITHOUT the final LayerNorm - k = encoder_layers is not None;
                             later blocks are not launched.
          ret_layer_results  the first result becomes (feature, layer_results): with output_layer = k the k + 1 pairs
                             (x, None), x (T, B, D) - the encoder input behind pos_conv, then each block's output -
                             and without output_layer an EMPTY list, as in the reference.
          ret_conv           the feature is the encoder's input instead.  The reference hands out the tensor its encoder
                             then works on in place, so this is x + GELU(pos_conv(x)) (masked frames zeroed first): the
                             stage _forward names "pos_conv", not the projection's raw output."""
        if self.p is None:
            raise RuntimeError("WavLM.extract_features: load_state_dict() first")
        if mask:
            raise NotImplementedError("WavLM.extract_features: mask is not supported (inference only)")
        if output_layer is not None and not 1 <= int(output_layer) <= self.cfg.encoder_layers:
            raise ValueError("WavLM.extract_features: output_layer %r is not in 1 .. %d" % (output_layer,
                                                                                          self.cfg.encoder_layers))
        if padding_mask is None and output_layer is None and not ret_conv and not ret_layer_results:
            return self._forward(source), None
        extra = {}
        feature = self._forward(source, padding_mask=padding_mask, output_layer=output_layer, extra=extra)
        if ret_conv:
            feature = extra["encoder_input"]
        if ret_layer_results:
            feature = (feature, [(x, None) for x in extra["layer_results"]])
        return feature, extra["frame_mask"]

    def frame_mask(self, padding_mask, T):
        """(B, T) bool NumPy frame mask of a (B, n) sample mask: forward_padding_mask of the reference (WavLM.py:311-321)."""
        import torch
        pm = padding_mask.detach().cpu().numpy() if isinstance(padding_mask, torch.Tensor) else np.asarray(padding_mask)
        pm = pm.astype(bool)
        if pm.ndim != 2:
            raise ValueError("WavLM.extract_features: padding_mask must be (B, n_samples), got %s" % (pm.shape,))
        extra = pm.shape[1] % T
        if extra:
            pm = pm[:, :-extra]
        return pm.reshape(pm.shape[0], T, -1).all(-1)

    def _forward(self, source, on_stage=None, padding_mask=None, output_layer=None, extra=None):
        """The launches of one call.  on_stage(name, result), if given, is called at the stage boundaries with a view of
        the workspace: "start" (None), "features" (conv stack, [B][T][C]), "front_end" (after post_extract_proj),
        "pos_conv" (x + GELU(pos_conv(x))), "block0" (the first block's output), "blocks" (the returned result) - and
        after every other launch with that launch's output: "conv<i>" / "conv<i>_norm" ([B][frames of layer i][C]),
        "front_norm" (the layer_norm ahead of post_extract_proj), "pos_pad" ([B][G][T + taps - 1][D / G]) and, per
        block, "block<i>.ln1", ".gate", ".qkv", ".att", ".out_proj", ".ln2", ".fc1", ".fc2".  A view is valid until the
        next launch (LayerNorms and residual GEMMs run in place).  The tests copy the views, tools/bench_wavlm.py
        records a device event per stage.
        padding_mask: see extract_features; one more stage, "front_mask" (front_end with the masked frames zeroed), and
        every block's attention excludes the masked frames as keys.  output_layer = k: blocks k, k + 1, .. (0-based) are
        not launched and "blocks" is block k - 1's output, copied.  extra, a dict, receives frame_mask (device bool or
        None), encoder_input (a copy of "pos_conv") and layer_results (copies, (T, B, D); empty without output_layer).
        More than MAX_FRAMES frames or a padding_mask route the attention to qpg_wavlm_attention_tiled_f32."""
        import torch
        from . import _lib
        wav = torch.as_tensor(source, dtype=torch.float32).to(self.device)
        if wav.dim() != 2:
            raise ValueError("WavLM.extract_features: source must be (B, n_samples), got %s" % (tuple(wav.shape),))
        if self.normalize_input:                 # each window by its own mean and variance (eps 1e-5)
            wav = torch.nn.functional.layer_norm(wav, wav.shape[1:])
        wav = wav.contiguous()
        B, n = wav.shape
        c, dev = self.cfg, self.device
        fr = frames_of(n, self.conv_layers)
        T = fr[-1]
        if T < 1:
            raise ValueError("WavLM.extract_features: %d samples are fewer than one frame's receptive field" % n)
        if T > MAX_FRAMES and not self.long_inputs:
            raise NotImplementedError("WavLM.extract_features: %d samples give %d frames, the attention kernel takes at most "
                                      "%d (cut the input into 4 s windows)" % (n, T, MAX_FRAMES))
        if T > MAX_FRAMES_LONG:
            raise NotImplementedError("WavLM.extract_features: %d samples give %d frames, the tiled attention kernel takes "
                                      "at most %d" % (n, T, MAX_FRAMES_LONG))
        fm = key_mask = None
        if padding_mask is not None:
            if self.normalize_input:
                raise NotImplementedError("WavLM.extract_features: padding_mask with normalize_input=True is not supported "
                                          "(the window statistics would include the padding)")
            fm_host = self.frame_mask(padding_mask, T)
            if fm_host.shape[0] != B:
                raise ValueError("WavLM.extract_features: padding_mask has %d rows, source %d" % (fm_host.shape[0], B))
            empty = np.flatnonzero(fm_host.all(-1))
            if len(empty):
                raise ValueError("WavLM.extract_features: batch member %d has no valid frame under padding_mask" % empty[0])
            fm = torch.from_numpy(fm_host).to(self.device)
            key_mask = fm.to(torch.uint8).contiguous()
        tiled = T > MAX_FRAMES or key_mask is not None
        C, D, F, H = self.conv_layers[0][0], c.encoder_embed_dim, c.encoder_ffn_embed_dim, c.encoder_attention_heads
        ws, p = self._workspace(B, n), self.p
        call = _lib.call

        def mark(stage, flat=None, width=0, rows=None):
            if on_stage is not None:
                rows = T if rows is None else rows
                on_stage(stage, None if flat is None else flat[:B * rows * width].view(B, rows, width))

        def gemm(A, lda, W, bias, res, out, ldc, M, N, K, gelu=0, n_outer=1, n_inner=1, a_outer=0, a_inner=0, w_inner=0,
                 bias_inner=0, c_outer=0, c_inner=0):
            call("qpg_wavlm_gemm_f32", dev, A, lda, W, bias, res, out, ldc, M, N, K, gelu, n_outer, n_inner, a_outer,
                 a_inner, w_inner, bias_inner, c_outer, c_inner)

        def ln(x, g, b, M, Cc, gelu, y):
            call("qpg_wavlm_layernorm_f32", dev, x, g, b, M, Cc, 1e-5, gelu, y)

        # conv feature extractor: [Conv1d, LayerNorm over channels, GELU] per layer, channels-last
        mark("start")
        k0, s0 = self.conv_layers[0][1:]
        L0 = p["conv"][0]
        cur, nxt = ws["a"], ws["b"]
        call("qpg_wavlm_conv0_f32", dev, wav, B, n, L0["w"], L0["b"], C, k0, s0, cur)
        mark("conv0", cur, C, fr[0])
        ln(cur, L0["g"], L0["beta"], B * fr[0], C, 1, cur)
        mark("conv0_norm", cur, C, fr[0])
        for i in range(1, len(self.conv_layers)):
            _, k, s = self.conv_layers[i]
            L = p["conv"][i]
            gemm(cur, s * C, L["w"], L["b"], None, nxt, C, fr[i], C, k * C, n_outer=B, a_outer=fr[i - 1] * C,
                 c_outer=fr[i] * C)
            mark("conv%d" % i, nxt, C, fr[i])
            ln(nxt, L["g"], L["beta"], B * fr[i], C, 1, nxt)
            mark("conv%d_norm" % i, nxt, C, fr[i])
            cur, nxt = nxt, cur
        M = B * T
        mark("features", cur, C)
        # layer_norm -> post_extract_proj
        x, y, h = ws["x"], ws["y"], ws["h"]
        if p["proj_w"] is not None:
            ln(cur, p["ln_g"], p["ln_b"], M, C, 0, cur)
            mark("front_norm", cur, C)
            gemm(cur, C, p["proj_w"], p["proj_b"], None, x, D, M, D, C)
        else:
            ln(cur, p["ln_g"], p["ln_b"], M, C, 0, x)
        mark("front_end", x, D)
        if fm is not None:                       # x[padding_mask] = 0 ahead of pos_conv and of the residual add
            call("qpg_wavlm_mask_rows_f32", dev, x, key_mask, M, D)
            mark("front_mask", x, D)
        # x + GELU(pos_conv(x))
        K, G = c.conv_pos, c.conv_pos_groups
        Cg, rows = D // G, T + c.conv_pos - 1
        call("qpg_wavlm_pos_pad_f32", dev, x, B, T, D, G, K, ws["pad"])
        if on_stage is not None:
            on_stage("pos_pad", ws["pad"][:B * rows * D].view(B, G, rows, Cg))
        gemm(ws["pad"], Cg, p["pos_w"], p["pos_b"], x, y, D, T, Cg, K * Cg, gelu=1, n_outer=B, n_inner=G,
             a_outer=G * rows * Cg, a_inner=rows * Cg, w_inner=Cg * K * Cg, bias_inner=Cg, c_outer=T * D, c_inner=Cg)
        x = y
        relb = self.position_bias_table(T)
        mark("pos_conv", x, D)

        def tap(flat):                           # (T, B, D), a copy: the blocks run in place
            return flat[:M * D].view(B, T, D).transpose(0, 1).clone(memory_format=torch.contiguous_format)
        if extra is not None:
            extra["frame_mask"] = fm
            extra["encoder_input"] = x[:M * D].view(B, T, D).clone()
            extra["layer_results"] = [] if output_layer is None else [tap(x)]
        n_blocks = len(p["layers"]) if output_layer is None else int(output_layer)
        for i, L in enumerate(p["layers"][:n_blocks]):
            blk = "block%d." % i
            ln(x, L["ln1_g"], L["ln1_b"], M, D, 0, h)
            mark(blk + "ln1", h, D)
            call("qpg_wavlm_gate_f32", dev, h, L["grep_w"], L["grep_b"], L["grep_a"], M, H, ws["gate"])
            mark(blk + "gate", ws["gate"], H)
            gemm(h, D, L["qkv_w"], L["qkv_b"], None, ws["qkv"], 3 * D, M, 3 * D, D)
            mark(blk + "qkv", ws["qkv"], 3 * D)
            if tiled:
                call("qpg_wavlm_attention_tiled_f32", dev, ws["qkv"], ws["gate"], relb, key_mask, B, T, H, ws["att"])
            else:
                call("qpg_wavlm_attention_f32", dev, ws["qkv"], ws["gate"], relb, B, T, H, ws["att"])
            mark(blk + "att", ws["att"], D)
            gemm(ws["att"], D, L["out_w"], L["out_b"], x, x, D, M, D, D)
            mark(blk + "out_proj", x, D)
            ln(x, L["ln2_g"], L["ln2_b"], M, D, 0, h)
            mark(blk + "ln2", h, D)
            gemm(h, D, L["fc1_w"], L["fc1_b"], None, ws["ffn"], F, M, F, D, gelu=1)
            mark(blk + "fc1", ws["ffn"], F)
            gemm(ws["ffn"], F, L["fc2_w"], L["fc2_b"], x, x, D, M, D, F)
            mark(blk + "fc2", x, D)
            if i == 0:
                mark("block0", x, D)
            if extra is not None and output_layer is not None:
                extra["layer_results"].append(tap(x))
        if output_layer is not None:             # block k's output as it stands: no final LayerNorm
            out = x[:M * D].view(B, T, D).clone()
            mark("blocks", out, D)
            return out
        out = torch.empty((B, T, D), dtype=torch.float32, device=dev)
        ln(x, p["fin_g"], p["fin_b"], M, D, 0, out)
        mark("blocks", out, D)
        return out


def load_wavlm(path, device="cuda:0", normalize_input=False, long_inputs=False):
    """The reference's wavlm_init: a checkpoint {'cfg': dict, 'model': state_dict} -> a loaded WavLM."""
    import torch
    ck = torch.load(path, map_location="cpu")
    return WavLM(ck["cfg"], device=device, normalize_input=normalize_input,
                 long_inputs=long_inputs).load_state_dict(ck["model"])


def wav2wavlm(wav, model, device=None):
    """wav2wavlm of the reference (make_beat_dataset.py:328-334): a whole 1-D clip -> (1, T, D) f32 NumPy through a
    long_inputs model (`device` is accepted for the reference's signature; the model's own device is used)."""
    wav = np.ascontiguousarray(wav, np.float32)
    if wav.ndim != 1:
        raise ValueError("wav2wavlm: a 1-D clip is required, got %s" % (wav.shape,))
    print(wav.shape)
    return model.extract_features(wav[None])[0].detach().cpu().numpy()


def wav_to_wavlm(save_dir, prefix, wavlm_model_path, gpu="0", batch=32, n_frames=240,
                 splits=("train", "validation", "test"), model=None):
    """wav_to_wavlm of the reference (make_beat_dataset.py:361-385): <prefix>_<split>_240.npz['wav'] (N, 64000) ->
    <prefix>_<split>_240_WavLM.npz['wavlm'] (N, T, D) f32, `batch` windows per call through one workspace."""
    if model is None:
        model = load_wavlm(wavlm_model_path, device="cuda:%s" % gpu)
    written = {}
    for key in splits:
        src = os.path.join(save_dir, prefix, prefix + '_' + key + '_' + str(n_frames) + '.npz')
        if not os.path.exists(src):
            continue
        wav = np.load(src)['wav']
        print(wav.shape)
        out = [model.extract_features(np.ascontiguousarray(wav[i:i + batch], np.float32))[0].cpu().numpy()
               for i in range(0, len(wav), batch)]
        dst = os.path.join(save_dir, prefix, prefix + '_' + key + '_' + str(n_frames) + '_WavLM.npz')
        np.savez_compressed(dst, wavlm=np.concatenate(out, 0) if out else np.zeros((0, 0, 0), np.float32))
        written[key] = dst
    return written


def read_wav_16k(path):
    """Mono f32 samples in [-1, 1) of a 16 kHz PCM .wav (standard library `wave`); any other rate is refused."""
    import wave
    with wave.open(path, "rb") as f:
        rate, width, ch, n = f.getframerate(), f.getsampwidth(), f.getnchannels(), f.getnframes()
        if rate != SAMPLE_RATE:
            raise ValueError("%s is sampled at %d Hz: WavLM takes 16000 Hz PCM and this tool does not resample" % (path, rate))
        if width not in (2, 4):
            raise ValueError("%s has %d-byte samples: 16- or 32-bit PCM is required" % (path, width))
        raw = f.readframes(n)
    a = np.frombuffer(raw, "<i2" if width == 2 else "<i4").astype(np.float32) / np.float32(2 ** (8 * width - 1))
    return a.reshape(-1, ch).mean(axis=1).astype(np.float32) if ch > 1 else a


def cut_windows(wav):
    """(M, 64000) f32: the clip's whole 4 s windows (window_bounds)."""
    wav = np.asarray(wav, np.float32)
    bounds = window_bounds(len(wav))
    if not bounds:
        raise ValueError("the clip has %d samples: shorter than one 4 s window (%d)" % (len(wav), WINDOW))
    return np.stack([wav[a:b] for a, b in bounds])


def main(argv=None):
    ap = argparse.ArgumentParser(description="WavLM features of one 16 kHz clip, in 4 s windows")
    ap.add_argument("--wav", required=True)
    ap.add_argument("--WavLM_model_path", required=True)
    ap.add_argument("--out", default="test_wavlm.npz")
    ap.add_argument("--gpu", type=str, default="0")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--whole", action="store_true", help="the whole clip in one call, (1, T, D), instead of 4 s windows")
    ap.add_argument("--layer", type=int, default=None, help="with --whole: block k's output (1-based) instead of the last")
    args = ap.parse_args(argv)
    if args.whole:
        model = load_wavlm(args.WavLM_model_path, device="cuda:%s" % args.gpu, long_inputs=True)
        wav = read_wav_16k(args.wav)
        feats = (wav2wavlm(wav, model) if args.layer is None else
                 model.extract_features(wav[None], output_layer=args.layer)[0].cpu().numpy())
        np.savez_compressed(args.out, wavlm=feats)
        print(args.out, feats.shape)
        return args.out
    if args.layer is not None:
        ap.error("--layer needs --whole")
    windows = cut_windows(read_wav_16k(args.wav))
    model = load_wavlm(args.WavLM_model_path, device="cuda:%s" % args.gpu)
    out = [model.extract_features(windows[i:i + args.batch])[0].cpu().numpy() for i in range(0, len(windows), args.batch)]
    np.savez_compressed(args.out, wavlm=np.concatenate(out, 0))
    print(args.out, np.concatenate(out, 0).shape)
    return args.out


if __name__ == "__main__":
    main()
