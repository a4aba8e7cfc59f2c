"""vq-wav2vec code extraction on the GPU: the producer of the `wavvq` track.  What the reference gets from fairseq in
process/make_test_data.py:43-64 and process/make_beat_dataset.py:388-429 (wav_to_vq) -

    z = model.feature_extractor(wav);  _, idxs = model.vector_quantizer.forward_idx(z)

- for the Gumbel model (vq-wav2vec.pt), inference only, without fairseq:

    from qpgesture_amd.wavvq import load_wavvq
    model = load_wavvq("vq-wav2vec.pt", device="cuda:0")
    idx = model.forward_idx(wav)                 # (B, n) f32 -> (B, T, G) int64 on the device; 64 000 samples: (B, 398, 2)

The model, restated from fairseq's published Wav2VecModel (no fairseq program text is in this package; no real checkpoint
has been run through it - INTEGRATION.md):
  feature extractor   per layer (C, k, s) of args.conv_feature_layers: Conv1d(Cin, C, k, stride s, no bias), Dropout
                      (identity), GroupNorm(1, C, eps 1e-5) - ONE mean and biased variance over all T x C values of a
                      window, then the per-channel weight and bias -, ReLU; log(|x| + 1) after the last layer.  The input
                      is used as given, without normalisation.
  quantiser           weight_proj = Linear(C, H), ReLU, Linear(H, G V) (vq_depth 2; one Linear(C, G V) at depth 1); the
                      logits viewed as [G][V]; idx[b][t][g] = argmax_v, the lowest index on exact ties.
The launches: qpg_wavlm_conv0_f32, qpg_wavlm_gemm_f32 for every later convolution and both
Linears, qpg_wavvq_groupnorm_f32, qpg_wavvq_relu_f32, qpg_wavvq_group_argmax_f32.  There is no torch fallback: a
configuration the kernels do not take raises NotImplementedError naming the field."""
import os

import numpy as np

from .wavlm import conv_layers_of, frames_of

EPS = 1e-5
EPI_NONE, EPI_RELU, EPI_RELU_LOG = 0, 1, 2       # QPG_WAVVQ_EPI_*
L0_BUDGET_BYTES = 1 << 30       # a call is cut into chunks whose layer-0 activations stay under this (real geometry: 40 windows)

# the fields this module reads, with the values an args that omits them gets (fairseq's defaults where it has the field)
ARGS_DEFAULTS = dict(conv_feature_layers="[(512, 10, 5), (512, 8, 4), (512, 4, 2), (512, 4, 2), (512, 4, 2), (512, 1, 1), "
                                         "(512, 1, 1), (512, 1, 1)]",
                     activation="relu", skip_connections_feat=False, log_compression=True, non_affine_group_norm=False,
                     vq_type="gumbel", vq_groups=2, vq_vars=320, vq_depth=2)


def _as_dict(args):
    if args is None:
        return dict(ARGS_DEFAULTS)
    return dict(ARGS_DEFAULTS, **(args if isinstance(args, dict) else vars(args)))


def check_supported(args):
    """Raise NotImplementedError naming the first args field the kernels do not take."""
    a = _as_dict(args)

    def need(field, ok, what):
        if not ok:
            raise NotImplementedError("vq-wav2vec args field %s = %r is not supported (%s)" % (field, a[field], what))
    need("skip_connections_feat", not a["skip_connections_feat"], "no skip connections in the feature extractor")
    need("activation", a["activation"] == "relu", "only 'relu'")
    need("log_compression", bool(a["log_compression"]), "the log compression is required")
    need("vq_type", a["vq_type"] == "gumbel", "only the Gumbel quantiser; the k-means quantiser is not implemented")
    need("vq_depth", a["vq_depth"] in (1, 2), "weight_proj of one or two Linears")
    need("vq_groups", isinstance(a["vq_groups"], int) and a["vq_groups"] >= 1, "at least one group")
    need("vq_vars", isinstance(a["vq_vars"], int) and a["vq_vars"] >= 1, "at least one variable per group")
    try:
        layers = conv_layers_of(a)
        ok = (len(layers) >= 1 and all(len(x) == 3 and min(x) >= 1 for x in layers)
              and all(x[0] == layers[0][0] for x in layers) and layers[0][0] % 16 == 0)
    except (ValueError, SyntaxError, TypeError):
        ok = False
    need("conv_feature_layers", ok, "[(C,k,s), ...] with one width C, a multiple of 16")


def receptive_field(layers):
    """Samples one output frame of the conv stack sees (945 for the vq-wav2vec list): the shortest input with a frame."""
    r = 1
    for _, k, s in reversed(layers):
        r = (r - 1) * s + k
    return r


class WavVQ:
    """WavVQ(args, device): fairseq's Wav2VecModel(args).eval() as far as feature_extractor and
    vector_quantizer.forward_idx go.  `args` is the checkpoint's args (argparse.Namespace or dict; omitted fields:
    ARGS_DEFAULTS) or a geometry of synth (WAVVQ_TINY, WAVVQ_GUMBEL)."""

    def __init__(self, args=None, device="cuda:0", l0_budget_bytes=L0_BUDGET_BYTES):
        import torch
        check_supported(args)
        self.args = _as_dict(args)
        self.device = torch.device(device)
        self.conv_layers = conv_layers_of(self.args)
        self.C = self.conv_layers[0][0]
        self.G, self.V = int(self.args["vq_groups"]), int(self.args["vq_vars"])
        self.l0_budget_bytes = int(l0_budget_bytes)
        self.p = None
        self._ws = {}

    # ---- parameters
    def load_state_dict(self, sd):
        import torch
        C, G, V = self.C, self.G, self.V

        def get(name, shape=None):
            if name not in sd:
                raise KeyError("vq-wav2vec state_dict lacks %r" % name)
            v = sd[name]
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if shape is not None and tuple(v.shape) != tuple(shape):
                raise ValueError("%s has shape %s, the args say %s" % (name, tuple(v.shape), tuple(shape)))
            return v

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)

        p = {"conv": []}
        cin = 1
        for i, (ch, k, s) in enumerate(self.conv_layers):
            pre = "feature_extractor.conv_layers.%d." % i
            w = get(pre + "0.weight", (ch, cin, k))
            if pre + "0.bias" in sd:
                raise NotImplementedError("vq-wav2vec state_dict has %s0.bias: convolutions with a bias are not supported" % pre)
            affine = (pre + "2.weight") in sd or (pre + "2.bias") in sd
            if affine and self.args["non_affine_group_norm"]:
                raise ValueError("args say non_affine_group_norm, the state_dict has %s2.weight" % pre)
            p["conv"].append(dict(w=dev(w.transpose(0, 2, 1).reshape(ch, k * cin)),                  # [Cout][k][Cin]
                                  g=dev(get(pre + "2.weight", (ch,))) if affine else None,           # absent: weight 1, bias 0
                                  beta=dev(get(pre + "2.bias", (ch,))) if affine else None))
            cin = ch
        wp = "vector_quantizer.weight_proj."
        if self.args["vq_depth"] == 2:
            w0 = get(wp + "0.0.weight")
            if w0.ndim != 2 or w0.shape[1] != C or w0.shape[0] % 16 != 0:
                raise NotImplementedError("%s0.0.weight has shape %s: [H][%d] with H a multiple of 16 is required"
                                          % (wp, tuple(w0.shape), C))
            H = w0.shape[0]
            p["head"] = [(dev(w0), dev(get(wp + "0.0.bias", (H,)))),
                         (dev(get(wp + "1.weight", (G * V, H))), dev(get(wp + "1.bias", (G * V,))))]
        else:
            p["head"] = [(dev(get(wp + "weight", (G * V, C))), dev(get(wp + "bias", (G * V,))))]
        self.H = p["head"][0][0].shape[0] if len(p["head"]) == 2 else 0
        self.p = p
        return self

    # ---- the forward pass
    def frames(self, n):
        """Frames the stack gives for n samples (0 below the receptive field)."""
        return frames_of(n, self.conv_layers)[-1]

    def max_chunk(self, n):
        """Windows of n samples per launch chain: the layer-0 activations [B][T0][C] f32 stay under l0_budget_bytes."""
        t0 = max(frames_of(n, self.conv_layers)[0], 1)
        return max(1, min(65535, self.l0_budget_bytes // (t0 * self.C * 4)))

    def _workspace(self, B, n):
        import torch
        from . import _lib
        fr = frames_of(n, self.conv_layers)
        C, R = self.C, B * fr[-1]
        lib = _lib.load()
        need = dict(a=B * fr[0] * C, b=B * (fr[1] if len(fr) > 1 else 0) * C,
                    gn=max(lib.qpg_wavvq_groupnorm_ws_floats(B, t, C) for t in fr),
                    hid=R * self.H, logits=R * self.G * self.V)
        for k, v in need.items():
            if k not in self._ws or self._ws[k].numel() < v:
                self._ws[k] = torch.empty(max(v, 4), dtype=torch.float32, device=self.device)
        return self._ws

    def _prepare(self, wav):
        import torch
        if self.p is None:
            raise RuntimeError("WavVQ: load_state_dict() first")
        wav = torch.as_tensor(wav, dtype=torch.float32).to(self.device)
        if wav.dim() != 2:
            raise ValueError("WavVQ: the input must be (B, n_samples), got %s" % (tuple(wav.shape),))
        B, n = wav.shape
        if B < 1:
            raise ValueError("WavVQ: an empty batch")
        if self.frames(n) < 1:
            raise ValueError("WavVQ: %d samples are fewer than one frame's receptive field (%d)"
                             % (n, receptive_field(self.conv_layers)))
        return wav.contiguous()

    def _chain(self, wav, upto, on_stage=None):
        """The launches for one chunk (B, n): upto "features" -> z view [B][T][C]; "logits" -> ([B][T][G V] view, None);
        "codes" -> (logits view, codes (B, T, G) i64, a fresh tensor).  Views are valid until the next call.
        on_stage(name), if given, is called ahead of the first launch ("start") and after each launch group: "conv<i>",
        "norm<i>", "head" (tools/bench_wavvq.py records a device event per stage)."""
        import torch
        from . import _lib
        B, n = wav.shape
        C, G, V, dev, p = self.C, self.G, self.V, self.device, self.p
        fr = frames_of(n, self.conv_layers)
        T = fr[-1]
        ws = self._workspace(B, n)
        call = _lib.call
        last = len(self.conv_layers) - 1

        def mark(name):
            if on_stage is not None:
                on_stage(name)

        def norm(x, i):
            L = p["conv"][i]
            call("qpg_wavvq_groupnorm_f32", dev, x, B, fr[i], C, L["g"], L["beta"], EPS,
                 EPI_RELU_LOG if i == last else EPI_RELU, ws["gn"], ws["gn"].numel())
            mark("norm%d" % i)

        def gemm(A, lda, W, bias, out, M, N, K, n_outer=1, a_outer=0, c_outer=0):
            call("qpg_wavlm_gemm_f32", dev, A, lda, W, bias, None, out, N, M, N, K, 0, n_outer, 1, a_outer, 0, 0, 0,
                 c_outer, 0)

        k0, s0 = self.conv_layers[0][1:]
        cur, nxt = ws["a"], ws["b"]
        mark("start")
        call("qpg_wavlm_conv0_f32", dev, wav, B, n, p["conv"][0]["w"], None, C, k0, s0, cur)
        mark("conv0")
        norm(cur, 0)
        for i in range(1, last + 1):
            _, k, s = self.conv_layers[i]
            gemm(cur, s * C, p["conv"][i]["w"], None, nxt, fr[i], C, k * C, n_outer=B, a_outer=fr[i - 1] * C,
                 c_outer=fr[i] * C)
            mark("conv%d" % i)
            norm(nxt, i)
            cur, nxt = nxt, cur
        z = cur[:B * T * C].view(B, T, C)
        if upto == "features":
            return z
        R = B * T
        x = cur
        if len(p["head"]) == 2:
            (w0, b0), (w1, b1) = p["head"]
            gemm(x, C, w0, b0, ws["hid"], R, self.H, C)
            call("qpg_wavvq_relu_f32", dev, ws["hid"], R * self.H)
            gemm(ws["hid"], self.H, w1, b1, ws["logits"], R, G * V, self.H)
        else:
            w1, b1 = p["head"][0]
            gemm(x, C, w1, b1, ws["logits"], R, G * V, C)
        logits = ws["logits"][:R * G * V].view(B, T, G * V)
        if upto == "logits":
            mark("head")
            return logits, None
        codes = torch.empty((B, T, G), dtype=torch.int64, device=dev)
        call("qpg_wavvq_group_argmax_f32", dev, ws["logits"], R, G, V, codes)
        mark("head")
        return logits, codes

    def _chunks(self, wav):
        wav = self._prepare(wav)
        step = self.max_chunk(wav.shape[1])
        return [wav[i:i + step] for i in range(0, wav.shape[0], step)]

    def features(self, wav):
        """z = feature_extractor(wav): (B, n) f32 -> (B, T, C) f32 on the device, channels last (fairseq's is (B, C, T))."""
        import torch
        return torch.cat([self._chain(c, "features").clone() for c in self._chunks(wav)])

    def logits(self, wav):
        """weight_proj(z) viewed as (B, T, G, V) f32 on the device: what forward_idx takes the argmax of."""
        import torch
        out = torch.cat([self._chain(c, "logits")[0].clone() for c in self._chunks(wav)])
        return out.view(out.shape[0], out.shape[1], self.G, self.V)

    def forward_idx(self, wav):
        """(B, n) f32 samples -> (B, T, G) int64 on the device: the indices of vector_quantizer.forward_idx(z)."""
        import torch
        return torch.cat([self._chain(c, "codes")[1] for c in self._chunks(wav)])


def load_wavvq(path, device="cuda:0"):
    """A fairseq-layout checkpoint {'args': argparse.Namespace, 'model': OrderedDict, ...} -> a loaded WavVQ, without
    fairseq.  The plain form {'args': dict, 'model': state_dict} is taken as well."""
    import pickle
    import torch
    try:
        ck = torch.load(path, map_location="cpu", weights_only=False)
    except (ModuleNotFoundError, AttributeError, pickle.UnpicklingError) as e:
        raise RuntimeError(
            "%s cannot be unpickled here (%s: %s): the checkpoint refers to a module that is not installed.  On a machine "
            "that has it, re-save the file in the plain form and load that:\n"
            "    ck = torch.load(%r, map_location='cpu')\n"
            "    torch.save({'args': vars(ck['args']), 'model': ck['model']}, 'vq-wav2vec.plain.pt')"
            % (path, type(e).__name__, e, os.path.basename(path))) from e
    if not isinstance(ck, dict) or "model" not in ck:
        raise ValueError("%s is not a checkpoint of the form {'args': ..., 'model': state_dict}" % path)
    args = ck.get("args")
    if args is None and isinstance(ck.get("cfg"), dict):          # (newer fairseq: cfg['model'] holds the same fields)
        args = ck["cfg"].get("model")
    if args is None:
        raise ValueError("%s has no 'args': re-save it as {'args': dict, 'model': state_dict}" % path)
    return WavVQ(args, device=device).load_state_dict(ck["model"])


def wav_to_vq(save_dir, prefix, wavvq_model_path, gpu="0", batch=32, n_frames=240,
              splits=("train", "validation", "test"), model=None):
    """wav_to_vq of the reference (make_beat_dataset.py:388-429): <prefix>_<split>_240.npz['wav'] (N, 64000) ->
    <prefix>_<split>_240_WavVQ.npz['wavvq'] (N, 398, 2) int64, `batch` windows per call."""
    if model is None:
        model = load_wavvq(wavvq_model_path, device="cuda:%s" % gpu)
    written = {}
    for key in splits:
        src = os.path.join(save_dir, prefix, prefix + '_' + key + '_' + str(n_frames) + '.npz')
        if not os.path.exists(src):
            continue
        wav = np.load(src)['wav']
        print(wav.shape)
        out = [model.forward_idx(np.ascontiguousarray(wav[i:i + batch], np.float32)).cpu().numpy()
               for i in range(0, len(wav), batch)]
        dst = os.path.join(save_dir, prefix, prefix + '_' + key + '_' + str(n_frames) + '_WavVQ.npz')
        np.savez_compressed(dst, wavvq=np.concatenate(out, 0) if out else np.zeros((0, 0, model.G), np.int64))
        written[key] = dst
    return written
