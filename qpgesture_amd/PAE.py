"""Phase extraction: the inference stage of the reference's codebook/PAE.py (the Periodic Auto-Encoder, DeepPhase) on
the device.

    python -m qpgesture_amd.PAE --config codebook.yml --gpu 0 --stage inference \
        [--PAE_model_path ../pretrained_model/PAE_checkpoint_070.bin] \
        [--rotation_dir ../dataset/BEAT/speaker_10_state_0/Rotation] [--phase_dir ../dataset/BEAT/speaker_10_state_0/Phase]

turns every `<rotation_dir>/<name>.npz['upper']` (T, 135) into `<phase_dir>/<name>.npz['phase']` float32 (T, 4, 1, 8, 1)
= [p, f, a, b] per frame (PAE.py:536-565), skipping files that exist.  Same flags as codebook/configs/parse_args.py; the
defaults of the three path flags (additive) are the reference's hard-coded paths.  `--stage train` (PAE
training) is `python -m qpgesture_amd.PAE_train`.

The reference runs Model.forward once per frame on a 240-frame window (PAE.py:477-508); here every frame of many clips
goes through one C-ABI call (qpg_pae_phase_f32, csrc/qpg_pae.hip): velocities on the device in f64, conv1 / conv2 on the
f32 matrix cores, DFT, fc layers and atan2' in the same kernel.  The reconstruction half (deconv*) is not built."""
import argparse
import os

import numpy as np
import torch

from . import _lib

# Model(135, 8, 240, 13, 4.0): the dimensions and the layout of qpg_pae_phase_f32's buffers are include/qpg.h's
IN_CH, MID_CH, EMBED, TIME = _lib.QPG_PAE_CHANNELS, _lib.QPG_PAE_MID, _lib.QPG_PAE_EMBED, _lib.QPG_PAE_TIME
KEYS, WINDOW = 13, 4.0
HALO, WS_STRIDE, MAX_CHUNK = _lib.QPG_PAE_HALO, _lib.QPG_PAE_WS_STRIDE, _lib.QPG_PAE_MAX_CHUNK
OFF = {k[len("QPG_PAE_OFF_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("QPG_PAE_OFF_")}
PARAM_FLOATS = _lib.QPG_PAE_PARAM_FLOATS
BN_EPS = 1e-5


def param_specs():
    """(name, shape) of every parameter in named_parameters() order (tpi, args, freqs first: not trainable)."""
    s = [("tpi", (1,)), ("args", (TIME,)), ("freqs", (TIME // 2,)),
         ("conv1.weight", (MID_CH, IN_CH, TIME)), ("conv1.bias", (MID_CH,)),
         ("bn_conv1.weight", (MID_CH,)), ("bn_conv1.bias", (MID_CH,)),
         ("conv2.weight", (EMBED, MID_CH, TIME)), ("conv2.bias", (EMBED,)),
         ("bn_conv2.weight", (EMBED,)), ("bn_conv2.bias", (EMBED,))]
    s += [x for e in range(EMBED) for x in (("fc.%d.weight" % e, (2, TIME)), ("fc.%d.bias" % e, (2,)))]
    s += [x for e in range(EMBED) for x in (("bn.%d.weight" % e, (2,)), ("bn.%d.bias" % e, (2,)))]
    s += [("deconv1.weight", (MID_CH, EMBED, TIME)), ("deconv1.bias", (MID_CH,)),
          ("bn_deconv1.weight", (MID_CH,)), ("bn_deconv1.bias", (MID_CH,)),
          ("deconv2.weight", (IN_CH, MID_CH, TIME)), ("deconv2.bias", (IN_CH,))]
    return s


PARAMS = param_specs()
BN_LAYERS = [("bn_conv1", MID_CH), ("bn_conv2", EMBED)] + [("bn.%d" % e, 2) for e in range(EMBED)] + \
    [("bn_deconv1", MID_CH)]
STATS = [(bn + "." + k, (n,)) for bn, n in BN_LAYERS for k in ("running_mean", "running_var")]     # the buffers
# what phase extraction reads from a checkpoint: the encoder half (no `args`, the deconv* half is ignored)
REQUIRED = {k: shape for k, shape in PARAMS + STATS if k != "args" and "deconv" not in k}


def bn_fold(sd, name):
    """Eval-mode BatchNorm as y = x * alpha + beta: alpha = weight / sqrt(running_var + eps), beta = bias -
    running_mean * alpha (f64, rounded to f32)."""
    w, b = sd[name + ".weight"].astype(np.float64), sd[name + ".bias"].astype(np.float64)
    alpha = w / np.sqrt(sd[name + ".running_var"].astype(np.float64) + BN_EPS)
    return alpha.astype(np.float32), (b - sd[name + ".running_mean"].astype(np.float64) * alpha).astype(np.float32)


def pack_params(sd):
    """State dict (numpy, no prefix) -> the f32 parameter block of qpg_pae_phase_f32 (layout: include/qpg.h)."""
    P = np.zeros(PARAM_FLOATS, np.float32)
    lane = np.arange(64)
    # W1[tap][group][lane] = conv1.weight[o = lane & 15][c = 4 group + (lane >> 4)][tap]
    w1 = np.zeros((16, 136, TIME), np.float32)
    w1[:MID_CH, :IN_CH] = sd["conv1.weight"]
    c = 4 * np.arange(34)[:, None] + (lane >> 4)[None, :]                              # [group][lane]
    P[OFF["W1"]:OFF["BN1"]] = w1[(lane & 15)[None, :], c, :].transpose(2, 0, 1).reshape(-1)
    w2 = np.zeros((16, 16, TIME), np.float32)
    w2[:EMBED, :MID_CH] = sd["conv2.weight"]
    o = 4 * np.arange(4)[:, None] + (lane >> 4)[None, :]
    P[OFF["W2"]:OFF["BN2"]] = w2[(lane & 15)[None, :], o, :].transpose(2, 0, 1).reshape(-1)
    for key, conv, bn, n in (("BN1", "conv1", "bn_conv1", MID_CH), ("BN2", "conv2", "bn_conv2", EMBED)):
        blk = P[OFF[key]:OFF[key] + 48].reshape(3, 16)
        blk[0, :n] = sd[conv + ".bias"]
        blk[1, :n], blk[2, :n] = bn_fold(sd, bn)
    P[OFF["FC"]:OFF["FCBN"]] = np.stack([sd["fc.%d.weight" % e] for e in range(EMBED)]).reshape(-1)
    blk = P[OFF["FCBN"]:OFF["FCBN"] + 48].reshape(3, 16)
    for e in range(EMBED):
        blk[0, 2 * e:2 * e + 2] = sd["fc.%d.bias" % e]
        blk[1, 2 * e:2 * e + 2], blk[2, 2 * e:2 * e + 2] = bn_fold(sd, "bn.%d" % e)
    P[OFF["FREQ"]:OFF["FREQ"] + TIME // 2] = sd["freqs"]
    P[OFF["TPI"]] = sd["tpi"][0]
    return P


def state_dict_from(obj, shapes=REQUIRED):
    """A checkpoint path, a loaded checkpoint dict or a state dict -> {name: numpy} without `module.`; refuses a key of
    `shapes` ({name: shape}) that is missing or has another shape."""
    if isinstance(obj, (str, os.PathLike)):
        from .checkpoint import load_checkpoint
        obj = load_checkpoint(obj)
    if isinstance(obj, dict) and "model_dict" in obj:
        obj = obj["model_dict"]
    sd = {}
    for k, v in obj.items():
        k = k[len("module."):] if k.startswith("module.") else k
        sd[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    missing = sorted(k for k in shapes if k not in sd)
    if missing:
        raise ValueError("PAE checkpoint lacks %s" % ", ".join(missing))
    for k, shape in shapes.items():
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError("PAE checkpoint: %s has shape %s, expected %s" % (k, tuple(sd[k].shape), shape))
    return sd


class Model:
    """PAE.Model(input_channels=135, embedding_channels=8, time_range=240, key_range=13, window=4.0) in eval mode, for
    phase extraction only: `checkpoint` is a path to the reference's torch.save({'args', 'epoch', 'model_dict'}), that
    dict, or a bare state dict (keys with or without `module.`).  `freqs` and `tpi` come from the checkpoint."""

    input_channels, embedding_channels, time_range, key_range, window = IN_CH, EMBED, TIME, KEYS, WINDOW

    def __init__(self, checkpoint, device="cuda:0"):
        self.device = torch.device(device)
        self.state_dict = state_dict_from(checkpoint)
        self.time_scale = KEYS / TIME
        self.params = torch.from_numpy(pack_params(self.state_dict)).to(self.device)


def _chunks(n, size):
    for f0 in range(0, n, size):
        yield f0, min(size, n - f0)


def pose2phase_clips(network, poses, data_mean=None, std=None, chunk=65536, return_v=False, return_latent=False):
    """Phase of every frame of every clip in `poses` (a list of (T_c, 135) arrays): a list of float32 (T_c, 4, 1, 8, 1)
    arrays [p, f, a, b] (pose2phase of the reference, clip by clip).  data_mean / std: codebook.yml's data_mean and
    clip(data_std, 0.01) (the package's codebook.yml when omitted).  The clips are concatenated and computed `chunk`
    frames per launch; return_v / return_latent add the BN'd fc outputs (T_c, 8, 2) = (x, y) and the latents
    (T_c, 8, 240) (the result is then a tuple of lists)."""
    if data_mean is None or std is None:
        from .checkpoint import load_config
        cfg = load_config(os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs", "codebook.yml"))
        data_mean = cfg.data_mean if data_mean is None else data_mean
        std = np.clip(np.asarray(cfg.data_std, np.float64), 0.01, None) if std is None else std
    dev = network.device
    lens = []
    for p in poses:
        p = np.asarray(p)
        if p.ndim != 2 or p.shape[1] != IN_CH or p.shape[0] < 1:
            raise ValueError("a clip must be (T >= 1, %d), got %s" % (IN_CH, p.shape))
        lens.append(p.shape[0])
    n = int(sum(lens))
    chunk = max(1, min(int(chunk), MAX_CHUNK, n))
    pose = torch.from_numpy(np.concatenate([np.asarray(p, np.float64) for p in poses])).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    mean_t = torch.from_numpy(np.asarray(data_mean, np.float64).reshape(IN_CH).copy()).to(dev)
    std_t = torch.from_numpy(np.asarray(std, np.float64).reshape(IN_CH).copy()).to(dev)
    ws = torch.empty((chunk + 2 * HALO - 1) * WS_STRIDE, dtype=torch.float32, device=dev)
    out = torch.empty((n, 4, EMBED), dtype=torch.float32, device=dev)
    v = torch.empty((n, EMBED, 2), dtype=torch.float32, device=dev) if return_v else None
    lat = torch.empty((n, EMBED, TIME), dtype=torch.float32, device=dev) if return_latent else None
    for f0, nf in _chunks(n, chunk):
        _lib.call("qpg_pae_phase_f32", dev, network.params, pose, mean_t, std_t, off, len(lens), n, f0, nf, ws,
                  ws.numel(), out[f0:f0 + nf], None if v is None else v[f0:f0 + nf],
                  None if lat is None else lat[f0:f0 + nf])
    bounds = np.concatenate([[0], np.cumsum(lens)])
    res = out.cpu().numpy().reshape(n, 4, 1, EMBED, 1)
    phases = [res[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    if not (return_v or return_latent):
        return phases
    extra = [x.cpu().numpy() for x in (v, lat) if x is not None]
    return (phases,) + tuple([e[a:b] for a, b in zip(bounds[:-1], bounds[1:])] for e in extra)


def pose2phase(network, pose, data_mean, std):
    """PAE.py:477 pose2phase(network, pose, data_mean, std): (T, 135) -> float32 (T, 4, 1, 8, 1) [p, f, a, b]."""
    return pose2phase_clips(network, [pose], data_mean, std)[0]


def build_parser():
    p = argparse.ArgumentParser(description='Codebook')
    p.add_argument('--config', default='./configs/codebook.yml')
    p.add_argument('--gpu', type=str, default='0')
    p.add_argument('--no_cuda', type=list, default=['0'])
    p.add_argument('--prefix', type=str, required=False, default='knn_pred_wavvq')
    p.add_argument('--save_path', type=str, required=False, default="./Speech2GestureMatching/output/")
    p.add_argument('--code_path', type=str, required=False)
    p.add_argument('--VQVAE_model_path', type=str, required=False)
    p.add_argument('--BEAT_path', type=str, default="../dataset/orig_BEAT/speakers/")
    p.add_argument('--save_dir', type=str, default="../dataset/BEAT")
    p.add_argument('--step', type=str, default="1")
    p.add_argument('--stage', type=str, default="train")
    # additive: the paths PAE.py hard-codes (:548, :560-561), and the frames per launch
    p.add_argument('--PAE_model_path', type=str, default="../pretrained_model/PAE_checkpoint_070.bin")
    p.add_argument('--rotation_dir', type=str, default="../dataset/BEAT/speaker_10_state_0/Rotation")
    p.add_argument('--phase_dir', type=str, default="../dataset/BEAT/speaker_10_state_0/Phase")
    p.add_argument('--chunk', type=int, default=65536)
    return p


def inference(model_path, rotation_dir, phase_dir, config, gpu="0", chunk=65536):
    """The inference stage (PAE.py:541-565): every Rotation file without a Phase file of the same name, all in one
    batch.  Returns the list of files written."""
    net = Model(model_path, device="cuda:%s" % gpu)
    data_mean = np.array(config.data_mean).squeeze()
    std = np.clip(np.array(config.data_std).squeeze(), a_min=0.01, a_max=None)
    if not os.path.exists(phase_dir):
        os.mkdir(phase_dir)
    todo, poses = [], []
    for item in sorted(os.listdir(rotation_dir)):
        if os.path.exists(os.path.join(phase_dir, item)):
            print(item, 'exists')
            continue
        todo.append(item)
        poses.append(np.load(os.path.join(rotation_dir, item))['upper'])
    if not todo:
        return []
    phases = pose2phase_clips(net, poses, data_mean, std, chunk=chunk)
    written = []
    for item, pose, phase in zip(todo, poses, phases):
        assert phase.shape[0] == pose.shape[0]
        np.savez_compressed(os.path.join(phase_dir, item), phase=phase)
        written.append(os.path.join(phase_dir, item))
    return written


def main(argv=None):
    from .checkpoint import load_config
    args = build_parser().parse_args(argv)
    if args.stage != "inference":
        raise SystemExit("this module runs --stage inference (phase extraction) only; --stage %s is out of scope "
                         "here: PAE training is `python -m qpgesture_amd.PAE_train`" % args.stage)
    return inference(args.PAE_model_path, args.rotation_dir, args.phase_dir, load_config(args.config), gpu=args.gpu,
                     chunk=args.chunk)


if __name__ == "__main__":
    main()
