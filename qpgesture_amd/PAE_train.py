"""PAE training on the device: the `--stage train` of the reference's codebook/PAE.py (PAE.py:273-476).

    python -m qpgesture_amd.PAE_train --config codebook.yml --gpu 0 [--train_data DIR|FILE] [--val_data DIR|FILE]
        [--synthetic N] [--epochs E] [--batch_size B] [--model_save_path DIR] [--max_updates U] [--resume CKPT]

Model(135, 8, 240, 13, 4.0) trained with 300 * MSE on velocity windows, the reference's AdamW (adamw.py: weight
decay p *= 1 - wd, not scaled by lr) and CyclicLRWithRestarts(batch_size=1, epoch_size=len(train_loader),
restart_period=10, t_mult=2, policy="cosine") (restated in Schedule).  Each epoch: a validation pass (eval mode, zero
velocity row last, mean of the per-batch losses), PAE_checkpoint_best.bin when it improves, PAE_checkpoint_{epoch:03d}.bin
every save_per_epochs epochs, then shuffled drop_last batches (train mode, zero row first) with one line per update.
A checkpoint is the reference's {'args', 'epoch', 'model_dict'} (keys without `module.`), loadable by PAE.Model for
phase extraction; `optimizer` and `schedule` ride along as additive keys so that --resume continues exactly.

One step is three C-ABI calls (csrc/qpg_pae_train.hip): forward (train or eval), backward and AdamW, all on flat
buffers (the parameter layout of include/qpg.h) and one caller-owned workspace; a step allocates nothing and does not
wait for the host."""
import argparse
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from .PAE import (EMBED, IN_CH, KEYS, MID_CH, PARAMS, STATS, TIME, WINDOW, build_parser as pae_parser,
                  state_dict_from)

LOSS_WEIGHT = 300.0
LR, WEIGHT_DECAY, BETAS, EPS = 1e-4, 1e-4, (0.9, 0.999), 1e-8
RESTART_PERIOD, T_MULT, MIN_LR = 10, 2, 1e-7
SEED = 23456
PAE_DEFAULTS = dict(epochs=100, save_per_epochs=10, n_poses=240, subdivision_stride=1,
                    model_save_path="./output/train_PAE", name="PAE")


def _offsets(specs):
    off, o = {}, 0
    for n, shape in specs:
        off[n] = o
        o += int(np.prod(shape))
    return off, o


OFF, PARAM_FLOATS = _offsets(PARAMS)
TRAINABLE = OFF["conv1.weight"]                                   # QPG_PAET_TRAINABLE
ST_OFF, STATS_FLOATS = _offsets(STATS)


def state_dict_keys():
    """The reference Model's state_dict() keys in order (parameters and buffers interleaved per module)."""
    keys = ["tpi", "args", "freqs"]
    mods = [("conv1", "c"), ("bn_conv1", "b"), ("conv2", "c"), ("bn_conv2", "b")]
    mods += [("fc.%d" % e, "c") for e in range(EMBED)] + [("bn.%d" % e, "b") for e in range(EMBED)]
    mods += [("deconv1", "c"), ("bn_deconv1", "b"), ("deconv2", "c")]
    for m, kind in mods:
        keys += [m + ".weight", m + ".bias"]
        if kind == "b":
            keys += [m + ".running_mean", m + ".running_var", m + ".num_batches_tracked"]
    return keys


def init_state_dict(seed=SEED):
    """Fresh weights with torch's default initialisation (Conv1d / Linear: kaiming-uniform weights and uniform biases;
    BatchNorm: weight 1, bias 0, running statistics 0 / 1), drawn in the reference's construction order from
    torch.manual_seed(seed).  The reference builds its model before it seeds (PAE.py:590-600 vs :312-317), so its
    initial weights depend on the process's unseeded RNG state and cannot be reproduced; this is the same
    distribution from a fixed seed."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {"tpi": torch.tensor([2.0 * np.pi], dtype=torch.float32),
          "args": torch.from_numpy(np.linspace(-WINDOW / 2, WINDOW / 2, TIME, dtype=np.float32)),
          "freqs": torch.fft.rfftfreq(TIME)[1:] * (TIME * (KEYS / TIME)) / WINDOW}

    def uniform(shape, bound):
        return (torch.rand(shape, generator=g, dtype=torch.float32) * 2.0 - 1.0) * bound

    def conv(name, cout, cin, k):
        fan_in = cin * max(k, 1)
        bound = 1.0 / math.sqrt(fan_in)            # kaiming_uniform_(a=sqrt(5)) and the bias rule of nn.Conv1d
        sd[name + ".weight"] = uniform((cout, cin, k) if k else (cout, cin), bound)
        sd[name + ".bias"] = uniform((cout,), bound)

    def bn(name, n):
        sd[name + ".weight"], sd[name + ".bias"] = torch.ones(n), torch.zeros(n)
        sd[name + ".running_mean"], sd[name + ".running_var"] = torch.zeros(n), torch.ones(n)
        sd[name + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)

    conv("conv1", MID_CH, IN_CH, TIME)
    bn("bn_conv1", MID_CH)
    conv("conv2", EMBED, MID_CH, TIME)
    bn("bn_conv2", EMBED)
    for e in range(EMBED):
        conv("fc.%d" % e, 2, TIME, 0)
        bn("bn.%d" % e, 2)
    conv("deconv1", MID_CH, EMBED, TIME)
    bn("bn_deconv1", MID_CH)
    conv("deconv2", IN_CH, MID_CH, TIME)
    return {k: sd[k] for k in state_dict_keys()}


def pack(sd):
    """State dict (keys with or without `module.`) -> (params f32 [PARAM_FLOATS], stats f32 [STATS_FLOATS],
    num_batches_tracked); refuses a missing key or a wrong shape."""
    sd = state_dict_from(sd, dict(PARAMS + STATS))
    P, S = np.zeros(PARAM_FLOATS, np.float32), np.zeros(STATS_FLOATS, np.float32)
    for table, out, offs in ((PARAMS, P, OFF), (STATS, S, ST_OFF)):
        for n, _ in table:
            out[offs[n]:offs[n] + sd[n].size] = sd[n].reshape(-1)
    return P, S, int(sd.get("bn_conv1.num_batches_tracked", 0))


def unpack(P, S, nbt):
    """Inverse of pack: the reference's state_dict (CPU tensors, its key order, dtypes and shapes)."""
    P, S = np.asarray(P, np.float32), np.asarray(S, np.float32)
    sd = {}
    for k in state_dict_keys():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(int(nbt), dtype=torch.int64)
        elif k in OFF:
            shape = dict(PARAMS)[k]
            sd[k] = torch.from_numpy(P[OFF[k]:OFF[k] + int(np.prod(shape))].reshape(shape).copy())
        else:
            sd[k] = torch.from_numpy(S[ST_OFF[k]:ST_OFF[k] + dict(STATS)[k][0]].copy())
    return sd


class Schedule:
    """CyclicLRWithRestarts(batch_size=1, epoch_size, restart_period=10, t_mult=2, policy="cosine", min_lr=1e-7) as the
    reference drives it: epoch_start() once per epoch before its batches (the scheduler's step()), after_update() after
    every optimiser step (batch_step()); `lr` and `wd` are what the next update uses.  Within an epoch of n updates the
    cosine position runs over torch.linspace(0, 1, n + 1) (f32 values); lr = min_lr + (base - min_lr) eta, wd = base_wd
    eta sqrt(1 / (n period)); the period restarts (x t_mult) once the epoch count within it passes the period, after
    the update that found it."""

    def __init__(self, epoch_size, base_lr=LR, base_wd=WEIGHT_DECAY, period=RESTART_PERIOD, t_mult=T_MULT,
                 min_lr=MIN_LR):
        self.epoch_size, self.base_lr, self.base_wd, self.min_lr = int(epoch_size), base_lr, base_wd, min_lr
        self.period, self.t_mult = int(math.ceil(period)), t_mult
        self.t_epoch, self.epoch, self.it, self.restarts = -1, -1, 0, 0
        self.lr, self.wd = base_lr, base_wd
        self._fracs = []

    def epoch_start(self):
        self.epoch += 1
        self.t_epoch += 1
        self._fracs = torch.linspace(0, 1, self.epoch_size + 1).tolist()
        self.it = 0
        self.after_update()

    def after_update(self):
        if self.it >= len(self._fracs):
            raise StopIteration("more updates in the epoch than the schedule's epoch_size")
        t_cur = self.t_epoch + self._fracs[self.it]
        self.it += 1
        eta = 0.5 * (1.0 + math.cos(math.pi * (t_cur / self.period)))
        self.lr = self.min_lr + (self.base_lr - self.min_lr) * eta
        self.wd = self.base_wd * eta * math.sqrt(1.0 / (self.epoch_size * self.period))
        if self.t_epoch % self.period < self.t_epoch:
            self.period = int(math.ceil(self.period * self.t_mult))
            self.restarts += 1
            self.t_epoch = 0

    def state(self):
        return dict(epoch_size=self.epoch_size, period=self.period, t_epoch=self.t_epoch, epoch=self.epoch, it=self.it,
                    restarts=self.restarts, lr=self.lr, wd=self.wd)

    def load(self, st):
        for k, v in st.items():
            setattr(self, k, v)
        self._fracs = torch.linspace(0, 1, self.epoch_size + 1).tolist()


def window_starts(lengths, n_poses=TIME, stride=1):
    """Global start frames of every window of clips of the given lengths, concatenated: clip c yields starts
    off_c + i * stride for i in 0 .. floor((T_c - n_poses) / stride) (none when T_c < n_poses)."""
    out, off = [], 0
    for T in lengths:
        T = int(T)
        n = (T - n_poses) // stride + 1 if T >= n_poses else 0
        out.append(off + np.arange(n, dtype=np.int64) * stride)
        off += T
    return np.concatenate(out) if out else np.zeros(0, np.int64)


class Trainer:
    """Flat f32 parameters / gradients (include/qpg.h layout, named_parameters() order), AdamW moments, BatchNorm
    running statistics and one workspace for `batch` windows on `device`.  set_data() uploads the normalised poses;
    forward(starts, train) / backward() / step(lr, wd) make one update; state_dict() is the reference's."""

    def __init__(self, state_dict=None, batch=256, device="cuda:0", seed=SEED):
        if batch < 2:
            raise ValueError("batch must be >= 2 (train-mode BatchNorm over the batch), got %d" % batch)
        self.device, self.batch = torch.device(device), int(batch)
        sd = init_state_dict(seed) if state_dict is None else state_dict
        P, S, self.num_batches_tracked = pack(sd)
        self.params = torch.from_numpy(P).to(self.device)
        self.stats = torch.from_numpy(S).to(self.device)
        self.grads = torch.zeros(PARAM_FLOATS, dtype=torch.float32, device=self.device)
        n = PARAM_FLOATS - TRAINABLE
        self.m = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.v = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.adam_steps = 0
        wsf = ctypes.c_int64(0)
        _lib.call("qpg_pae_train_ws_floats", self.device, self.batch, ctypes.addressof(wsf))
        self.ws = torch.empty(int(wsf.value), dtype=torch.float32, device=self.device)
        self.loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.poses, self.n_frames = None, 0

    def set_data(self, poses_norm):
        """(n_frames, 135) normalised poses (already f32-rounded as the reference's dataset does)."""
        p = torch.as_tensor(np.ascontiguousarray(poses_norm, np.float32) if not isinstance(poses_norm, torch.Tensor)
                            else poses_norm, dtype=torch.float32)
        if p.ndim != 2 or p.shape[1] != IN_CH or p.shape[0] < TIME:
            raise ValueError("poses must be (n >= 240, 135), got %s" % (tuple(p.shape),))
        self.poses, self.n_frames = p.to(self.device).contiguous(), int(p.shape[0])

    def check_starts(self, starts):
        s = np.asarray(starts, np.int64)
        if s.ndim != 1 or s.shape[0] != self.batch:
            raise ValueError("need %d window starts, got %s" % (self.batch, s.shape))
        if s.min() < 0 or s.max() > self.n_frames - TIME:
            raise ValueError("window start outside 0..%d" % (self.n_frames - TIME))
        return s

    def forward(self, starts, train=True):
        """starts: (batch,) host array of checked window starts or a device i64 tensor (the caller's checked copy).
        Returns the loss as a device f64 scalar (no synchronisation)."""
        if not isinstance(starts, torch.Tensor):
            starts = torch.from_numpy(self.check_starts(starts)).to(self.device)
        elif (starts.dtype != torch.int64 or starts.device != self.device or starts.ndim != 1
              or starts.numel() != self.batch or not starts.is_contiguous()):
            # (a device tensor's values are not read back here; a start outside the data gives a NaN window)
            raise ValueError("device window starts must be a contiguous int64 (%d,) tensor on %s" %
                             (self.batch, self.device))
        _lib.call("qpg_pae_train_forward_f32", self.device, self.params, self.stats, self.poses, self.n_frames, starts,
                  self.batch, 1 if train else 0, self.ws, self.ws.numel(), self.loss)
        if train:
            self.num_batches_tracked += 1
        return self.loss

    def backward(self):
        _lib.call("qpg_pae_train_backward_f32", self.device, self.params, self.batch, self.ws, self.ws.numel(),
                  self.grads)

    def step(self, lr, weight_decay):
        self.adam_steps += 1
        _lib.call("qpg_pae_adamw_f32", self.device, self.params[TRAINABLE:], self.grads[TRAINABLE:], self.m, self.v,
                  self.m.numel(), float(lr), float(weight_decay), BETAS[0], BETAS[1], EPS, self.adam_steps)

    def state_dict(self):
        return unpack(self.params.cpu().numpy(), self.stats.cpu().numpy(), self.num_batches_tracked)

    def load_state_dict(self, sd):
        P, S, self.num_batches_tracked = pack(sd)
        self.params.copy_(torch.from_numpy(P))
        self.stats.copy_(torch.from_numpy(S))

    def optimizer_state(self):
        return {"step": self.adam_steps, "exp_avg": self.m.cpu(), "exp_avg_sq": self.v.cpu()}

    def load_optimizer_state(self, st):
        self.adam_steps = int(st["step"])
        self.m.copy_(st["exp_avg"])
        self.v.copy_(st["exp_avg_sq"])


# ---------------------------------------------------------------------------------------------------------------------
# data

def normalise(pose, mean, std):
    """(pose - mean) / std in f64, rounded once to f32 (lmdb_data_loader.py:65-69)."""
    return ((np.asarray(pose, np.float64) - mean) / std).astype(np.float32)


def load_windows_source(path, mean, std, stride):
    """A directory of Rotation-style *.npz['upper'] clips (windows at `stride`) or an .npz / .npy array of windows
    (N, 240, 135) (each its own clip).  Returns (normalised f32 poses (n, 135), window starts)."""
    if os.path.isdir(path):
        clips = [np.load(os.path.join(path, f))["upper"] for f in sorted(os.listdir(path)) if f.endswith(".npz")]
    else:
        arr = np.load(path)
        if isinstance(arr, np.lib.npyio.NpzFile):
            arr = arr[arr.files[0]]
        arr = np.asarray(arr)
        if arr.ndim != 3 or arr.shape[1:] != (TIME, IN_CH):
            raise ValueError("%s: windows must be (N, 240, 135), got %s" % (path, arr.shape))
        clips, stride = list(arr), TIME
    clips = [c for c in clips if c.shape[0] >= TIME]
    if not clips:
        raise ValueError("%s holds no clip of 240 frames or more" % path)
    starts = window_starts([c.shape[0] for c in clips], TIME, stride)
    return normalise(np.concatenate(clips), mean, std), starts


def synthetic_source(n_windows, seed, mean, std, clip_len=600):
    """n_windows windows at stride 1 of seeded synthetic clips (synth.make_pae_motion)."""
    from . import synth
    per = clip_len - TIME + 1
    clips = [synth.make_pae_motion(clip_len, seed + i) for i in range((n_windows + per - 1) // per)]
    starts = window_starts([clip_len] * len(clips))[:n_windows]
    return normalise(np.concatenate(clips), mean, std), starts


# ---------------------------------------------------------------------------------------------------------------------
# the training loop (PAE.py:273-476 without the plots)

def validate(tr, starts):
    """Mean of the per-batch eval-mode losses over the drop_last batches in order (evaluate_testset)."""
    nb = len(starts) // tr.batch
    if nb == 0:
        return float("nan")
    dev_starts = torch.from_numpy(np.asarray(starts[:nb * tr.batch], np.int64)).to(tr.device)
    tot = torch.zeros((), dtype=torch.float64, device=tr.device)
    for i in range(nb):
        tot += tr.forward(dev_starts[i * tr.batch:(i + 1) * tr.batch], train=False)[0]
    return float(tot) / nb


def save_checkpoint(path, args, epoch, tr, sched, rng_state, best):
    torch.save({"args": args, "epoch": epoch, "model_dict": tr.state_dict(),
                "optimizer": tr.optimizer_state(), "schedule": sched.state(), "rng": rng_state, "best": best}, path)


def train(args, cfg):
    """Run the loop; returns (per-update losses, checkpoint paths written, the Trainer)."""
    pae = dict(PAE_DEFAULTS)
    pae.update({k: v for k, v in dict(getattr(cfg, "PAE", {}) or {}).items()})
    epochs = args.epochs if args.epochs is not None else int(pae["epochs"])
    save_dir = args.model_save_path or pae["model_save_path"]
    batch = args.batch_size if args.batch_size is not None else int(getattr(cfg, "batch_size", 256))
    stride = int(pae["subdivision_stride"])
    mean = np.asarray(cfg.data_mean, np.float64).reshape(-1)
    std = np.clip(np.asarray(cfg.data_std, np.float64).reshape(-1), 0.01, None)
    if args.synthetic:
        tr_pose, tr_starts = synthetic_source(args.synthetic, 1000, mean, std)
        va_pose, va_starts = synthetic_source(max(batch, args.synthetic // 8), 5000, mean, std)
    else:
        tr_pose, tr_starts = load_windows_source(args.train_data, mean, std, stride)
        va_pose, va_starts = load_windows_source(args.val_data or args.train_data, mean, std, stride)
    dev = "cuda:%s" % args.gpu
    ckpt = None
    if args.resume:
        from .checkpoint import load_checkpoint
        ckpt = load_checkpoint(args.resume)
    tr = Trainer(None if ckpt is None else ckpt["model_dict"], batch=batch, device=dev, seed=args.seed)
    # one buffer holds both sources: validation windows follow the training poses
    tr.set_data(np.concatenate([tr_pose, va_pose]))
    va_starts = va_starts + tr_pose.shape[0]
    n_batches = len(tr_starts) // batch
    if n_batches == 0:
        raise SystemExit("fewer training windows (%d) than one batch (%d)" % (len(tr_starts), batch))
    sched = Schedule(n_batches)
    rng = np.random.default_rng(args.seed)
    best, epoch0 = (1e6, 0), 0
    if ckpt is not None and "optimizer" in ckpt:
        tr.load_optimizer_state(ckpt["optimizer"])
        sched.load(ckpt["schedule"])
        rng.bit_generator.state = ckpt["rng"]
        best, epoch0 = tuple(ckpt["best"]), int(ckpt["epoch"])
    elif ckpt is not None:
        epoch0 = int(ckpt.get("epoch", 0))
    os.makedirs(save_dir, exist_ok=True)
    name = pae["name"]
    losses, written, updates = [], [], 0
    for epoch in range(epoch0, epochs):
        resumed_here = ckpt is not None and "optimizer" in ckpt and epoch == epoch0
        if not resumed_here:
            loss_eval = validate(tr, va_starts)
            print("loss on validation: {:.3f}".format(loss_eval))
            if loss_eval < best[0]:
                print(" *** BEST VALIDATION LOSS : {:.3f}".format(loss_eval))
                best = (loss_eval, epoch)
                p = os.path.join(save_dir, "{}_checkpoint_best.bin".format(name))
                save_checkpoint(p, args, epoch, tr, sched, rng.bit_generator.state, best)
                written.append(p)
            if epoch % int(pae["save_per_epochs"]) == 0:
                p = os.path.join(save_dir, "{}_checkpoint_{:03d}.bin".format(name, epoch))
                save_checkpoint(p, args, epoch, tr, sched, rng.bit_generator.state, best)
                written.append(p)
        sched.epoch_start()
        perm = rng.permutation(len(tr_starts))[:n_batches * batch]
        dev_starts = torch.from_numpy(tr_starts[perm].astype(np.int64)).to(tr.device)
        for i in range(n_batches):
            loss = tr.forward(dev_starts[i * batch:(i + 1) * batch], train=True)
            tr.backward()
            tr.step(sched.lr, sched.wd)
            sched.after_update()
            lv = float(loss)
            losses.append(lv)
            print("> epoch [{}] updates[{}] updates[{}] loss[{:.8f}]".format(epoch, i + 1, updates, lv))
            updates += 1
            if args.max_updates and updates >= args.max_updates:
                return losses, written, tr
    return losses, written, tr


def build_parser():
    p = pae_parser()
    p.description = "PAE training"
    # additive
    p.add_argument("--train_data", type=str, default=None)
    p.add_argument("--val_data", type=str, default=None)
    p.add_argument("--synthetic", type=int, default=0)
    p.add_argument("--epochs", type=int, default=None)
    p.add_argument("--batch_size", type=int, default=None)
    p.add_argument("--model_save_path", type=str, default=None)
    p.add_argument("--max_updates", type=int, default=0)
    p.add_argument("--resume", type=str, default=None)
    p.add_argument("--seed", type=int, default=SEED)
    return p


def main(argv=None):
    from .checkpoint import load_config
    args = build_parser().parse_args(argv)
    if args.stage != "train":
        raise SystemExit("PAE_train runs --stage train; phase extraction is `python -m qpgesture_amd.PAE --stage "
                         "inference`")
    if not args.synthetic and not args.train_data:
        raise SystemExit("give --train_data (or --synthetic N)")
    cfg_path = args.config
    if not os.path.exists(cfg_path):
        cfg_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs", "codebook.yml")
    return train(args, load_config(cfg_path))


if __name__ == "__main__":
    main()
