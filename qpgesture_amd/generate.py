"""The GRU speech-to-code generator on the GPU: the reference's baseline WITHOUT motion matching, codebook/inference.py's
wav -> Generator_gru.sample -> 30 codes per 4 s window -> VQVAE.decode -> poses (the model: codebook/generate/generate.py
:9-31 WavEncoder, :312-350 Generator_gru).  Inference only; the trainer that writes the checkpoint is qpgesture_amd/end2end.py.

    from qpgesture_amd.generate import load_generator, cut_windows
    model = load_generator("end2end_checkpoint_080.bin", device="cuda:0")
    codes = model.codes(cut_windows(audio))          # (M, 30) int64 on the device
    zs = model.sample(windows)                       # [int64 (1, M * 30)], what VQVAE.decode takes

    python -m qpgesture_amd.generate --wav clip.wav --end2end_model_path E.bin --config codebook.yml \\
        --VQVAE_model_path CK.bin --save_path DIR --prefix P [--max_frames N] [--no_bvh]

One sample() is twelve launches of include/qpg.h's qpg_gen_* kernels and qpg_wavlm_gemm_f32: five
convolutions, per GRU layer the input projection of both directions (one GEMM) and the recurrence, the direction sum +
LayerNorm, the 512-way Linear and the row argmax (on exact ties the lowest index).  Everything is f32 and nothing leaves
the device before the codes.  A window's result does not depend on what it is batched with.  There is no torch fallback:
a shape the kernels do not take raises."""
import argparse
import math
import os

import numpy as np

TAPS = 16                                   # QPG_GEN_TAPS
HIDDEN = 200                                # QPG_GEN_HIDDEN
HEAD_LD = 208                               # QPG_GEN_HEAD_LD
CODES = 512
CONVS = ((1, 8, 3), (8, 16, 3), (16, 32, 6), (32, 64, 6), (64, 32, 6))        # (Cin, Cout, stride); BatchNorm + LeakyReLU after the first four
SLOPE, BN_EPS, LN_EPS = 0.3, 1e-5, 1e-5
MIN_SAMPLES = 5866                          # the shortest input that yields a frame
WINDOW = 64000
MAX_BATCH = 4096                            # windows per pass (a pass's buffers are 1.2 MB per window)


def conv_frames(n, stride):
    return 0 if n < TAPS else (n - TAPS) // stride + 1


def n_frames(n):
    """Code slots T of an n-sample input (64 000 -> 30)."""
    for _, _, s in CONVS:
        n = conv_frames(n, s)
    return n


class Generator_gru:
    """Generator_gru(device).load_state_dict(sd): the reference's module in eval mode."""

    def __init__(self, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        self.hidden_size, self.output_size = HIDDEN, CODES
        self.p = None
        self._ws = {}

    def load_state_dict(self, sd):
        """The reference's state_dict (torch tensors or arrays), with or without DataParallel's `module.` prefix.
        `num_batches_tracked` entries are ignored; the first missing or mis-shaped tensor is named."""
        import torch
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}

        def get(name, shape):
            if name not in sd:
                raise KeyError("generator state_dict lacks %r" % name)
            v = sd[name]
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if tuple(v.shape) != tuple(shape):
                raise ValueError("%s has shape %s, the model wants %s" % (name, tuple(v.shape), tuple(shape)))
            return v.astype(np.float32)

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)

        p = dict(convs=[], gru=[])
        for i, (cin, cout, stride) in enumerate(CONVS):
            pre = "WavEncoder.feat_extractor.%d." % (3 * i)
            w = get(pre + "weight", (cout, cin, TAPS))
            layer = dict(w=dev(w.transpose(0, 2, 1)), b=dev(get(pre + "bias", (cout,))), bn=None, cin=cin, cout=cout,
                         stride=stride)                                                         # w: [Cout][16][Cin]
            if i < 4:
                q = "WavEncoder.feat_extractor.%d." % (3 * i + 1)
                layer["bn"] = dev(np.stack([get(q + n, (cout,)) for n in ("weight", "bias", "running_mean", "running_var")]))
            p["convs"].append(layer)
        H = HIDDEN
        for layer, nin in ((0, CONVS[-1][1]), (1, 2 * H)):
            tags = ("_l%d" % layer, "_l%d_reverse" % layer)
            p["gru"].append(dict(
                nin=nin,
                w_ih=dev(np.concatenate([get("project.weight_ih" + t, (3 * H, nin)) for t in tags])),        # [6H][In]
                b_ih=dev(np.concatenate([get("project.bias_ih" + t, (3 * H,)) for t in tags])),
                w_hh=dev(np.stack([get("project.weight_hh" + t, (3 * H, H)) for t in tags])),                 # [2][3H][H]
                b_hh=dev(np.stack([get("project.bias_hh" + t, (3 * H,)) for t in tags]))))
        out_w = np.zeros((CODES, HEAD_LD), np.float32)
        out_w[:, :H] = get("out.weight", (CODES, H))
        p.update(ln_g=dev(get("norm.weight", (H,))), ln_b=dev(get("norm.bias", (H,))), out_w=dev(out_w),
                 out_b=dev(get("out.bias", (CODES,))))
        self.p = p
        return self

    # ---- the forward pass
    def _buffer(self, key, n, dtype):
        """A kept device buffer of at least n elements (contents are whatever the last pass left: every stage writes all
        it later reads)."""
        import torch
        if key not in self._ws or self._ws[key].numel() < n:
            self._ws[key] = torch.empty(max(int(n), 4), dtype=dtype, device=self.device)
        return self._ws[key]

    def _wav(self, wav):
        import torch
        if isinstance(wav, torch.Tensor):
            x = wav.detach()
        else:
            x = torch.from_numpy(np.ascontiguousarray(wav, np.float32))
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[0] < 1:
            raise ValueError("Generator_gru: wav must be (B, n) or (n,), got %s" % (tuple(x.shape),))
        if x.shape[1] < MIN_SAMPLES:
            raise ValueError("Generator_gru: %d samples yield no frame, at least %d are needed" % (x.shape[1], MIN_SAMPLES))
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def _pass(self, x, logits, on_stage=None):
        """The launches of one pass over x (B, n) on the device; logits (B T, 512) is written.  on_stage(name, view), if
        given, is called behind every launch: "start" (None), "conv1" .. "conv5" ([B][T_i][C_i]), per GRU layer
        "gru<i>.proj" ([B T][1200]) and "gru<i>" ([B][T][400]), "ln" ([B T][208], columns 200.. zero), "logits".  A view
        is valid until the next pass."""
        import torch
        from . import _lib
        if self.p is None:
            raise RuntimeError("Generator_gru: load_state_dict() first")
        dev, p, call = self.device, self.p, _lib.call
        B, n = x.shape
        if on_stage is not None:
            on_stage("start", None)
        cur, t_in = x, n
        for i, L in enumerate(p["convs"]):
            T = conv_frames(t_in, L["stride"])
            out = self._buffer("conv%d" % i, B * T * L["cout"], torch.float32)
            call("qpg_gen_conv1d_f32", dev, cur, B, t_in, L["cin"], L["w"], L["b"], L["bn"], BN_EPS, 1 if i < 4 else 0, SLOPE,
                 L["cout"], L["stride"], out)
            if on_stage is not None:
                on_stage("conv%d" % (i + 1), out[:B * T * L["cout"]].view(B, T, L["cout"]))
            cur, t_in = out, T
        T, R, H = t_in, B * t_in, HIDDEN
        proj = self._buffer("proj", R * 6 * H, torch.float32)
        for i, L in enumerate(p["gru"]):
            call("qpg_wavlm_gemm_f32", dev, cur, L["nin"], L["w_ih"], L["b_ih"], None, proj, 6 * H, R, 6 * H, L["nin"], 0, 1, 1,
                 0, 0, 0, 0, 0, 0)
            if on_stage is not None:
                on_stage("gru%d.proj" % i, proj[:R * 6 * H].view(R, 6 * H))
            out = self._buffer("gru%d" % i, R * 2 * H, torch.float32)
            call("qpg_gen_gru_layer_f32", dev, proj, L["w_hh"], L["b_hh"], B, T, H, out)
            if on_stage is not None:
                on_stage("gru%d" % i, out[:R * 2 * H].view(B, T, 2 * H))
            cur = out
        ln = self._buffer("ln", R * HEAD_LD, torch.float32)
        call("qpg_gen_head_ln_f32", dev, cur, p["ln_g"], p["ln_b"], R, H, LN_EPS, ln)
        if on_stage is not None:
            on_stage("ln", ln[:R * HEAD_LD].view(R, HEAD_LD))
        call("qpg_wavlm_gemm_f32", dev, ln, HEAD_LD, p["out_w"], p["out_b"], None, logits, CODES, R, CODES, HEAD_LD, 0, 1, 1,
             0, 0, 0, 0, 0, 0)
        if on_stage is not None:
            on_stage("logits", logits)

    def logits(self, wav, on_stage=None, max_batch=MAX_BATCH):
        """(B, T, 512) f32 on the device.  More than max_batch windows go through in several passes, which changes no bit."""
        import torch
        x = self._wav(wav)
        B, T = x.shape[0], n_frames(x.shape[1])
        out = torch.empty((B, T, CODES), dtype=torch.float32, device=self.device)
        for b0 in range(0, B, max_batch):
            b1 = min(B, b0 + max_batch)
            self._pass(x[b0:b1], out[b0:b1].view(-1, CODES), on_stage)
        return out

    def codes(self, wav, on_stage=None, max_batch=MAX_BATCH):
        """(B, T) int64 on the device: per window and code slot the index of the largest logit (the lowest on a tie)."""
        import torch
        from . import _lib
        logits = self.logits(wav, on_stage, max_batch)
        B, T, _ = logits.shape
        codes = torch.empty((B, T), dtype=torch.int64, device=self.device)
        _lib.call("qpg_gen_argmax_f32", self.device, logits, B * T, CODES, codes)
        if on_stage is not None:
            on_stage("codes", codes)
        return codes

    def sample(self, x):
        """[int64 (1, B T)] on the device: the batch flattened into one row, as the reference's loop over it does."""
        return [self.codes(x).reshape(1, -1)]

    def forward(self, x, target=None):
        """(logits (B, T, 512), loss): loss = F.cross_entropy(logits.view(-1, 512), target.view(-1)) as a 0-d f32 device
        tensor, None without a target."""
        import torch
        from . import _lib
        logits = self.logits(x)
        if target is None:
            return logits, None
        R = logits.shape[0] * logits.shape[1]
        t = torch.as_tensor(target).reshape(-1)
        if t.numel() != R:
            raise ValueError("Generator_gru.forward: %d targets for %d code slots" % (t.numel(), R))
        t = t.to(device=self.device, dtype=torch.int64).contiguous()
        if int(t.min()) < 0 or int(t.max()) >= CODES:
            raise ValueError("Generator_gru.forward: targets must lie in [0, %d)" % CODES)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        _lib.call("qpg_gen_cross_entropy_f32", self.device, logits, t, R, CODES, self._buffer("ce", R, torch.float32), loss)
        return logits, loss[0]

    __call__ = forward


def load_generator(path, device="cuda:0"):
    """The reference's end2end checkpoint {'args', 'epoch', 'model_dict'} (or a bare state_dict) -> a loaded Generator_gru."""
    from .checkpoint import load_checkpoint
    return Generator_gru(device=device).load_state_dict(load_checkpoint(path)["model_dict"])


def cut_windows(audio, n_poses=240, fps=60, max_frames=None, sr=16000):
    """(M, 64000) f32: the windows codebook/inference.py:30-41, :67-75 feeds the model, its arithmetic taken literally.
    unit_time = sr * n_poses / fps samples (a float); a clip shorter than one unit is one window, otherwise
    ceil((len - unit) / unit) + 1; window i starts at floor(i * unit_time), is 64 000 samples long and zero-padded.  With
    max_frames the reference compares the window count against (max_frames / fps) / n_poses - a number of the order of
    0.25, so the branch is practically always taken - and then uses int(max_frames / n_poses) windows, whatever the clip's
    length: later windows are all zeros, or the clip's tail is dropped."""
    audio = np.asarray(audio, np.float32).reshape(-1)
    clip_length = audio.shape[0]
    unit_time = sr * n_poses / fps
    if clip_length < unit_time:
        num_subdivision = 1
    else:
        num_subdivision = math.ceil((clip_length - unit_time) / unit_time) + 1
    if max_frames is not None and num_subdivision >= (max_frames / fps) / n_poses:
        num_subdivision = int(max_frames / n_poses)
    out = np.zeros((num_subdivision, WINDOW), np.float32)
    for i in range(num_subdivision):
        start = math.floor(i * unit_time)
        piece = audio[start:start + WINDOW]
        out[i, :len(piece)] = piece
    return out


def main(wav, end2end_model_path, config, VQVAE_model_path, save_path, prefix, max_frames=0, no_bvh=False, gpu="0",
         smoothing=False):
    """codebook/inference.py's main(): all windows of the clip in ONE batched sample(), the flattened codes in ONE
    VQVAE.decode pass (:84), de-normalised; writes <save_path>/code<prefix>.npy and generate<prefix>.npy (the reference's
    names) and, unless no_bvh, <prefix>_euler.npy and <prefix>_generated.bvh.  max_frames 0 means None.
    Returns (poses (240 M, 135), codes int64 (M, 30))."""
    from . import wavlm
    from .VisualizeCodebook import _model
    from .checkpoint import denormalize_poses, load_config
    device = "cuda:%s" % gpu
    audio = wavlm.read_wav_16k(wav)
    windows = cut_windows(audio, max_frames=(int(max_frames) or None))
    print('num_subdivision: {}, unit_time: {}, clip_length: {}'.format(len(windows), float(WINDOW), len(audio)))
    cfg = load_config(config)
    vq = _model(cfg, VQVAE_model_path, gpu)
    model = load_generator(end2end_model_path, device=device)
    zs = model.sample(windows)
    out_code = zs[0].reshape(len(windows), -1).cpu().numpy()
    poses = vq.decode(zs).squeeze(0).cpu().numpy()
    out_poses = denormalize_poses(poses, cfg.data_mean, cfg.data_std)
    os.makedirs(save_path, exist_ok=True)
    print(out_poses.shape)
    print(out_code.shape)
    np.save(os.path.join(save_path, 'code' + prefix + '.npy'), out_code)
    np.save(os.path.join(save_path, 'generate' + prefix + '.npy'), out_poses)
    if not no_bvh:
        from . import bvh
        euler = bvh.poses_to_euler(poses, cfg.data_mean, cfg.data_std, smoothing=smoothing, device=device)
        np.save(os.path.join(save_path, prefix + '_euler.npy'), euler)
        bvh.write_bvh(os.path.join(save_path, prefix + '_generated.bvh'), euler)
    return out_poses, out_code


def build_parser():
    p = argparse.ArgumentParser(description="speech to gesture codes with the GRU generator (no matching), decoded to poses")
    for k in ("wav", "end2end_model_path", "config", "VQVAE_model_path", "save_path", "prefix"):
        p.add_argument("--" + k, required=True)
    p.add_argument("--max_frames", type=int, default=0, help="the reference's MAX_FRAMES (0: none); see INTEGRATION.md")
    p.add_argument("--no_bvh", action="store_true")
    p.add_argument("--smoothing", action="store_true")
    p.add_argument("--gpu", type=str, default="0")
    return p


def _cli(argv=None):
    return main(**vars(build_parser().parse_args(argv)))


if __name__ == "__main__":
    _cli()
