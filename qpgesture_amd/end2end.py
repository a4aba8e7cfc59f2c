"""Training of the GRU speech-to-code generator on the device: the reference's codebook/end2end.py (:46-137) around
generate.py's Generator_gru, as PAE_train.py is to PAE.py.

    python -m qpgesture_amd.end2end --config codebook.yml --gpu 0 --train_data X.npz --val_data Y.npz [--synthetic N]
        [--epochs E] [--batch_size B] [--max_updates U] [--resume CKPT] [--model_save_path DIR]

The model runs in train() mode: the four BatchNorm1d layers use batch statistics over (B, T_i) with biased variance and
update running_mean / running_var with momentum 0.1 and unbiased variance; nn.GRU(dropout=0.1) drops layer 0's output on
its way into layer 1 (scale 1 / 0.9) and nothing else; the loss is F.cross_entropy over the B T rows; the optimiser is
optim.Adam(lr, betas) without scheduler or weight decay.  Each epoch (1 .. epochs) starts with a validation pass in eval
mode over drop_last batches (mean of the per-batch losses), writes <name>_checkpoint_best.bin when that improves on 100.0,
else <name>_checkpoint_{epoch:03d}.bin every save_per_epochs epochs - {'args', 'epoch', 'model_dict'} with DataParallel's
`module.` keys, loadable by generate.load_generator - and then runs the shuffled drop_last training batches with the
reference's log line per update.  `optimizer`, `rng` (shuffle), `dropout_rng`, `updates` and `best` ride along as additive
keys so that --resume continues bit-identically.

One update is a chain of include/qpg.h's stage kernels: parameters and gradients live in ONE flat
f32 buffer each, in the layout LAYOUT declares (the kernels' layouts: convolution weights [Cout][16][Cin], the two
directions of a GRU tensor adjacent, out.weight padded to rows of QPG_GEN_HEAD_LD), and qpgesture_amd.optim.Adam steps
over them in one launch.  Buffers are kept between updates: an update allocates nothing after the first of its shape,
and step() does not wait for the host.  The dropout mask comes from a seeded torch.Generator on the device; it cannot match
torch's own dropout stream, so only the distribution is the reference's (`mask=` overrides it, dropout=0 skips the stage).
The reference does not seed its initialisation either: init_state_dict() draws torch's default initialisation from a fixed
seed.

Data: .npz files with `audio` (N, 64000) f32 and `codes` (N, 30) int64.  The reference's own loader no longer yields codes
(data_loader/lmdb_data_loader.py:61-74); sample_windows() restates data_preprocessor.py:_sample_from_clip's arithmetic and
build_dataset() makes the codes with the package's VQVAE.encode."""
import argparse
import math
import os

import numpy as np
import torch

from . import _lib
from .generate import (BN_EPS, CODES, CONVS, HEAD_LD, HIDDEN, LN_EPS, SLOPE, TAPS, WINDOW, Generator_gru, conv_frames,
                       n_frames, MIN_SAMPLES)
from .optim import Adam

LR, BETAS, MOMENTUM, DROPOUT, SEED = 0.0002, (0.99, 0.999), 0.1, 0.1, 23456
END2END_DEFAULTS = dict(lr=LR, betas=list(BETAS), epochs=100, save_per_epochs=10, name="end2end",
                        model_save_path="./output/train_end2end")
WS_CAP_FLOATS = 16 << 20                   # most workspace a weight gradient's slab partials get (64 MB)
H = HIDDEN
assert TAPS == _lib.QPG_GEN_TAPS and H == _lib.QPG_GEN_HIDDEN and HEAD_LD == _lib.QPG_GEN_HEAD_LD
SAVED = _lib.QPG_GEN_GRU_SAVED


def _layout():
    """[(torch key, stored shape, kind)] in flat order.  kind "conv": stored [Cout][16][Cin], torch's is its
    transpose(1, 2); "head": stored [512][HEAD_LD] with zero columns past H, torch's is [:, :H]; "plain": as torch's."""
    out = []
    for i, (cin, cout, _) in enumerate(CONVS):
        pre = "WavEncoder.feat_extractor.%d." % (3 * i)
        out += [(pre + "weight", (cout, TAPS, cin), "conv"), (pre + "bias", (cout,), "plain")]
        if i < 4:
            q = "WavEncoder.feat_extractor.%d." % (3 * i + 1)
            out += [(q + "weight", (cout,), "plain"), (q + "bias", (cout,), "plain")]
    for layer, nin in ((0, CONVS[-1][1]), (1, 2 * H)):
        tags = ("_l%d" % layer, "_l%d_reverse" % layer)
        for name, shape in (("weight_ih", (3 * H, nin)), ("bias_ih", (3 * H,)), ("weight_hh", (3 * H, H)),
                            ("bias_hh", (3 * H,))):
            out += [("project.%s%s" % (name, t), shape, "plain") for t in tags]       # direction 0 | direction 1
    out += [("norm.weight", (H,), "plain"), ("norm.bias", (H,), "plain"), ("out.weight", (CODES, HEAD_LD), "head"),
            ("out.bias", (CODES,), "plain")]
    return out


LAYOUT = _layout()
OFF, SHAPE, KIND = {}, {}, {}
PARAM_FLOATS = 0
for _k, _s, _kind in LAYOUT:
    OFF[_k], SHAPE[_k], KIND[_k] = PARAM_FLOATS, _s, _kind
    PARAM_FLOATS += int(np.prod(_s))
    assert OFF[_k] % 4 == 0                # (every tensor 16-byte aligned in the flat buffers)
BN_KEYS = ["WavEncoder.feat_extractor.%d." % (3 * i + 1) for i in range(4)]


def torch_shape(key):
    s = SHAPE[key]
    return (s[0], s[2], s[1]) if KIND[key] == "conv" else (s[0], H) if KIND[key] == "head" else s


def view(flat, key):
    """The tensor `key` of a flat buffer as a view in torch's shape."""
    v = flat[OFF[key]:OFF[key] + int(np.prod(SHAPE[key]))].view(SHAPE[key])
    return v.transpose(1, 2) if KIND[key] == "conv" else v[:, :H] if KIND[key] == "head" else v


def state_dict_keys():
    """Generator_gru().state_dict()'s keys in torch's order."""
    keys = []
    for i in range(5):
        keys += ["WavEncoder.feat_extractor.%d.%s" % (3 * i, n) for n in ("weight", "bias")]
        if i < 4:
            keys += [BN_KEYS[i] + n for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    for layer in range(2):
        for suffix in ("", "_reverse"):
            keys += ["project.%s_l%d%s" % (n, layer, suffix) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return keys + ["norm.weight", "norm.bias", "out.weight", "out.bias"]


def _strip(sd):
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def pack(sd):
    """State dict (keys with or without `module.`) -> (params f32 [PARAM_FLOATS], running f32 [4][2][64] (mean, var; the
    first C_i of each row used), num_batches_tracked [4]); the first missing or mis-shaped tensor is named."""
    sd = _strip(sd)

    def get(name, shape):
        if name not in sd:
            raise KeyError("generator state_dict lacks %r" % name)
        v = sd[name]
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if tuple(v.shape) != tuple(shape):
            raise ValueError("%s has shape %s, the model wants %s" % (name, tuple(v.shape), tuple(shape)))
        return v.astype(np.float32)

    P = torch.zeros(PARAM_FLOATS, dtype=torch.float32)
    for k, _, _ in LAYOUT:
        view(P, k).copy_(torch.from_numpy(get(k, torch_shape(k))))
    S = np.zeros((4, 2, 64), np.float32)
    nbt = []
    for i, q in enumerate(BN_KEYS):
        c = CONVS[i][1]
        S[i, 0, :c], S[i, 1, :c] = get(q + "running_mean", (c,)), get(q + "running_var", (c,))
        nbt.append(int(np.asarray(sd.get(q + "num_batches_tracked", 0))))
    return P.numpy(), S, nbt


def unpack(P, S, nbt, prefix=""):
    """Inverse of pack: the reference's state_dict (CPU tensors, torch's key order, shapes and dtypes)."""
    P = torch.from_numpy(np.ascontiguousarray(P, np.float32))
    sd = {}
    for k in state_dict_keys():
        if k in OFF:
            sd[prefix + k] = view(P, k).contiguous().clone()
        else:
            i = BN_KEYS.index(k[:k.rindex(".") + 1])
            c = CONVS[i][1]
            if k.endswith("num_batches_tracked"):
                sd[prefix + k] = torch.tensor(int(nbt[i]), dtype=torch.int64)
            else:
                sd[prefix + k] = torch.from_numpy(np.array(S[i, 0 if k.endswith("running_mean") else 1, :c], np.float32))
    return sd


def init_state_dict(seed=SEED):
    """Fresh weights with torch's default initialisation, from CPU torch.nn modules built in the reference's construction
    order (generate.py:9-26, :312-321) under a forked RNG seeded with `seed`.  The reference does not seed before it
    builds its model, so its initial weights cannot be reproduced; this is the same distribution from a fixed seed."""
    nn = torch.nn
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        layers = []
        for i, (cin, cout, stride) in enumerate(CONVS):
            layers.append(nn.Conv1d(cin, cout, TAPS, stride=stride))
            if i < 4:
                layers += [nn.BatchNorm1d(cout), nn.LeakyReLU(SLOPE)]
        enc = nn.Sequential(*layers)
        gru = nn.GRU(input_size=CONVS[-1][1], hidden_size=H, num_layers=2, dropout=DROPOUT, bidirectional=True,
                     batch_first=True)
        norm, out = nn.LayerNorm(H), nn.Linear(H, CODES)
    sd = {}
    for pre, mod in (("WavEncoder.feat_extractor.", enc), ("project.", gru), ("norm.", norm), ("out.", out)):
        sd.update({pre + k: v.detach().clone() for k, v in mod.state_dict().items()})
    return {k: sd[k] for k in state_dict_keys()}


class GeneratorTrainer:
    """GeneratorTrainer(device, lr, betas, dropout, seed): flat parameters / gradients (LAYOUT), Adam moments, BatchNorm
    running statistics and kept activation buffers on `device`.  forward_backward(wav, target) leaves the gradients in
    `grads`; step() adds the Adam update; eval_loss() runs the inference model (generate.Generator_gru) on the same
    weights."""

    def __init__(self, device="cuda:0", lr=LR, betas=BETAS, dropout=DROPOUT, seed=SEED, state_dict=None):
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError("dropout must lie in [0, 1), got %r" % (dropout,))
        self.device, self.dropout, self.seed = torch.device(device), float(dropout), int(seed)
        self.params = torch.zeros(PARAM_FLOATS, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros(PARAM_FLOATS, dtype=torch.float32, device=self.device)
        self.running = torch.zeros((4, 2, 64), dtype=torch.float32, device=self.device)
        self.stat = torch.zeros((4, 2, 64), dtype=torch.float32, device=self.device)     # the last batch's mean, variance
        self.num_batches_tracked = [0, 0, 0, 0]
        self.opt = Adam((self.params, self.grads), lr=lr, betas=betas)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(self.seed)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._ws = {}
        self._eval = Generator_gru(device=self.device)
        self.on_stage = None                  # on_stage(name), if set, is called behind every stage's launches (bench)
        self.load_state_dict(init_state_dict(seed) if state_dict is None else state_dict)

    init_state_dict = staticmethod(init_state_dict)      # GeneratorTrainer.init_state_dict(seed): the module's function

    # ---- state
    def load_state_dict(self, sd):
        """The reference's state_dict, with or without DataParallel's `module.` prefix, num_batches_tracked included."""
        P, S, self.num_batches_tracked = pack(sd)
        self.params.copy_(torch.from_numpy(P))
        self.running.copy_(torch.from_numpy(S))
        return self

    def state_dict(self, prefix="module."):
        return unpack(self.params.cpu().numpy(), self.running.cpu().numpy(), self.num_batches_tracked, prefix)

    def gradients(self):
        """{torch key: view of the flat gradient buffer in torch's shape}."""
        return {k: view(self.grads, k) for k, _, _ in LAYOUT}

    def parameters(self):
        return {k: view(self.params, k) for k, _, _ in LAYOUT}

    def _stored(self, flat, key):
        return flat[OFF[key]:OFF[key] + int(np.prod(SHAPE[key]))]

    def _pair(self, flat, name, layer):
        """Both directions of a GRU tensor as one contiguous run."""
        k0 = "project.%s_l%d" % (name, layer)
        n = int(np.prod(SHAPE[k0]))
        return flat[OFF[k0]:OFF[k0] + 2 * n]

    def _buffer(self, key, n, dtype=torch.float32):
        if key not in self._ws or self._ws[key].numel() < n:
            self._ws[key] = torch.empty(max(int(n), 4), dtype=dtype, device=self.device)
        return self._ws[key]

    def _wav(self, wav):
        x = wav.detach() if isinstance(wav, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(wav, np.float32))
        if x.dim() != 2 or x.shape[0] < 1:
            raise ValueError("GeneratorTrainer: wav must be (B, n), got %s" % (tuple(x.shape),))
        if x.shape[1] < MIN_SAMPLES:
            raise ValueError("GeneratorTrainer: %d samples yield no frame, at least %d are needed" % (x.shape[1], MIN_SAMPLES))
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def _target(self, target, R):
        if isinstance(target, torch.Tensor) and target.is_cuda:
            t = target.reshape(-1)              # (not read back: a code outside [0, 512) gives a NaN loss)
        else:
            t = np.asarray(target.cpu() if isinstance(target, torch.Tensor) else target).reshape(-1)
            if t.size and (t.min() < 0 or t.max() >= CODES):
                raise ValueError("GeneratorTrainer: targets must lie in [0, %d)" % CODES)
            t = torch.from_numpy(t.astype(np.int64))
        if t.numel() != R:
            raise ValueError("GeneratorTrainer: %d targets for %d code slots" % (t.numel(), R))
        return t.to(device=self.device, dtype=torch.int64).contiguous()

    def _workspace(self, B, lens):
        lib = _lib.load()
        R = B * lens[-1]
        want = lambda rows: max(1, min(_lib.QPG_GEN_TRAIN_MAX_SLABS, -(-rows // _lib.QPG_GEN_TRAIN_SLAB_MIN_ROWS)))
        need = [lib.qpg_gen_bn_ws_floats(B * lens[i + 1], CONVS[i][1]) for i in range(4)]
        need += [lib.qpg_gen_conv1d_wgrad_ws_floats(cin, cout, want(B * lens[i + 1])) for i, (cin, cout, _) in enumerate(CONVS)]
        need += [lib.qpg_gen_rowgrad_ws_floats(N, K, want(R)) for N, K in ((CODES, HEAD_LD), (6 * H, 2 * H), (6 * H, CONVS[-1][1]),
                                                                         (3 * H, H))]
        need.append(lib.qpg_gen_head_ln_bwd_ws_floats(R))
        floor = 6 * H * 2 * H + 6 * H                                   # one slab of the largest gradient
        return self._buffer("ws", max(floor, min(WS_CAP_FLOATS, max(need))))

    # ---- one update
    def forward_backward(self, wav, target, mask=None):
        """Train-mode forward (running statistics updated), loss, and every gradient into `grads`.  wav (B, n), target
        (B, T) codes, mask optional uint8 / bool (B, T, 400): the dropout mask of layer 0's output (nonzero keeps).
        Returns the loss as a 0-d f32 device tensor (a view of a kept buffer: the next update overwrites it)."""
        dev, call = self.device, _lib.call
        x = self._wav(wav)
        B, n = x.shape
        lens = [n]
        for _, _, s in CONVS:
            lens.append(conv_frames(lens[-1], s))
        T = lens[-1]
        R = B * T
        tgt = self._target(target, R)
        ws = self._workspace(B, lens)
        wsn = ws.numel()
        P, G = self.params, self.grads
        st = self._stored
        conv_keys = ["WavEncoder.feat_extractor.%d." % (3 * i) for i in range(5)]
        drop = mask is not None or self.dropout > 0.0
        if mask is not None:
            m = torch.as_tensor(mask)
            if m.numel() != R * 2 * H:
                raise ValueError("GeneratorTrainer: the mask has %d entries, layer 0's output %d" % (m.numel(), R * 2 * H))
            m = (m != 0).to(device=dev).contiguous().view(torch.uint8).reshape(-1)
        elif drop:
            u = self._buffer("rand", R * 2 * H)[:R * 2 * H]
            u.uniform_(generator=self.gen)
            mb = self._buffer("mask", R * 2 * H, torch.bool)[:R * 2 * H]
            torch.ge(u, self.dropout, out=mb)
            m = mb.view(torch.uint8)
        scale = 1.0 / (1.0 - self.dropout)
        mark = self.on_stage or (lambda name: None)
        mark("start")

        # forward
        cur, raw, act = x, [], []
        for i, (cin, cout, s) in enumerate(CONVS):
            Ri = B * lens[i + 1]
            c = self._buffer("c%d" % i, Ri * cout)
            call("qpg_gen_conv1d_f32", dev, cur, B, lens[i], cin, st(P, conv_keys[i] + "weight"), st(P, conv_keys[i] + "bias"),
                 None, BN_EPS, 0, SLOPE, cout, s, c)
            raw.append(c)
            cur = c
            mark("conv fwd")
            if i < 4:
                call("qpg_gen_bn_stats_f32", dev, c, Ri, cout, ws, wsn, self.stat[i], self.running[i, 0], self.running[i, 1],
                     MOMENTUM)
                a = self._buffer("a%d" % i, Ri * cout)
                call("qpg_gen_bn_apply_f32", dev, c, Ri, cout, self.stat[i], st(P, BN_KEYS[i] + "weight"),
                     st(P, BN_KEYS[i] + "bias"), BN_EPS, SLOPE, a)
                act.append(a)
                cur = a
                self.num_batches_tracked[i] += 1
                mark("bn fwd")
        proj = self._buffer("proj", R * 6 * H)
        outs, svs, inp, in1 = [], [], cur, None
        for L, nin in ((0, CONVS[-1][1]), (1, 2 * H)):
            call("qpg_wavlm_gemm_f32", dev, inp, nin, self._pair(P, "weight_ih", L), self._pair(P, "bias_ih", L), None, proj,
                 6 * H, R, 6 * H, nin, 0, 1, 1, 0, 0, 0, 0, 0, 0)
            mark("gru input gemm")
            out = self._buffer("gru%d" % L, R * 2 * H)
            sv = self._buffer("sv%d" % L, R * 2 * SAVED * H)
            call("qpg_gen_gru_layer_train_f32", dev, proj, self._pair(P, "weight_hh", L), self._pair(P, "bias_hh", L), B, T, H,
                 out, sv)
            mark("gru fwd recurrence")
            outs.append(out)
            svs.append(sv)
            inp = out
            if L == 0 and drop:
                inp = self._buffer("drop", R * 2 * H)
                call("qpg_gen_dropout_f32", dev, out, m, R * 2 * H, scale, inp)
            if L == 0:
                mark("dropout")
                in1 = inp                                                # layer 1's input
        ln = self._buffer("ln", R * HEAD_LD)
        call("qpg_gen_head_ln_f32", dev, outs[1], st(P, "norm.weight"), st(P, "norm.bias"), R, H, LN_EPS, ln)
        logits = self._buffer("logits", R * CODES)
        call("qpg_wavlm_gemm_f32", dev, ln, HEAD_LD, st(P, "out.weight"), st(P, "out.bias"), None, logits, CODES, R, CODES,
             HEAD_LD, 0, 1, 1, 0, 0, 0, 0, 0, 0)
        call("qpg_gen_cross_entropy_f32", dev, logits, tgt, R, CODES, self._buffer("ce", R), self.loss)
        mark("head fwd + loss")

        # backward: the head
        dlog = self._buffer("dlogits", R * CODES)
        call("qpg_gen_cross_entropy_backward_f32", dev, logits, tgt, R, CODES, dlog)
        call("qpg_gen_rowgrad_f32", dev, dlog, CODES, ln, HEAD_LD, R, CODES, HEAD_LD, 0, 1, st(G, "out.weight"),
             st(G, "out.bias"), ws, wsn)
        out_wT = self._buffer("out_wT", HEAD_LD * CODES)[:HEAD_LD * CODES].view(HEAD_LD, CODES)
        out_wT.copy_(st(P, "out.weight").view(CODES, HEAD_LD).t())
        dln = self._buffer("dln", R * HEAD_LD)
        call("qpg_wavlm_gemm_f32", dev, dlog, CODES, out_wT, None, None, dln, HEAD_LD, R, HEAD_LD, CODES, 0, 1, 1, 0, 0, 0, 0,
             0, 0)
        dout = self._buffer("dout", R * 2 * H)
        call("qpg_gen_head_ln_backward_f32", dev, dln, outs[1], st(P, "norm.weight"), R, H, LN_EPS, ws, wsn,
             st(G, "norm.weight"), st(G, "norm.bias"), dout)
        mark("head bwd")
        # backward: the recurrences
        dxp, dgh = self._buffer("dxp", R * 6 * H), self._buffer("dgh", R * 6 * H)
        d = None
        for L, nin, xin in ((1, 2 * H, in1), (0, CONVS[-1][1], raw[4])):
            whhT = self._buffer("whhT%d" % L, 2 * H * 3 * H)[:2 * H * 3 * H].view(2, H, 3 * H)
            whhT.copy_(self._pair(P, "weight_hh", L).view(2, 3 * H, H).transpose(1, 2))
            call("qpg_gen_gru_layer_backward_f32", dev, dout, svs[L], outs[L], whhT, B, T, H, dxp, dgh)
            mark("gru bwd recurrence")
            call("qpg_gen_rowgrad_f32", dev, dxp, 6 * H, xin, nin, R, 6 * H, nin, 0, 1, self._pair(G, "weight_ih", L),
                 self._pair(G, "bias_ih", L), ws, wsn)
            gw, gb = self._pair(G, "weight_hh", L), self._pair(G, "bias_hh", L)
            for dr in (0, 1):
                call("qpg_gen_rowgrad_f32", dev, dgh[dr * 3 * H:], 6 * H, outs[L][dr * H:], 2 * H, R, 3 * H, H,
                     1 if dr else -1, T, gw[dr * 3 * H * H:], gb[dr * 3 * H:], ws, wsn)
            mark("gru weight grads")
            wihT = self._buffer("wihT%d" % L, nin * 6 * H)[:nin * 6 * H].view(nin, 6 * H)
            wihT.copy_(self._pair(P, "weight_ih", L).view(6 * H, nin).t())
            if L == 1:
                call("qpg_wavlm_gemm_f32", dev, dxp, 6 * H, wihT, None, None, dout, nin, R, nin, 6 * H, 0, 1, 1, 0, 0, 0, 0, 0,
                     0)
                if drop:
                    call("qpg_gen_dropout_f32", dev, dout, m, R * 2 * H, scale, dout)
            else:
                d = self._buffer("d4", R * nin)
                call("qpg_wavlm_gemm_f32", dev, dxp, 6 * H, wihT, None, None, d, nin, R, nin, 6 * H, 0, 1, 1, 0, 0, 0, 0, 0, 0)
            mark("gru data grad gemm")
        # backward: the encoder
        for i in range(4, -1, -1):
            cin, cout, s = CONVS[i]
            xin = x if i == 0 else act[i - 1]
            call("qpg_gen_conv1d_bwd_weight_f32", dev, xin, B, lens[i], cin, d, cout, s, st(G, conv_keys[i] + "weight"),
                 st(G, conv_keys[i] + "bias"), ws, wsn)
            mark("conv%d weight grad" % (i + 1))
            if i > 0:
                Rp = B * lens[i]
                da = self._buffer("da%d" % (i - 1), Rp * cin)
                call("qpg_gen_conv1d_bwd_data_f32", dev, d, B, lens[i], cin, st(P, conv_keys[i] + "weight"), cout, s, da)
                mark("conv data grad")
                call("qpg_gen_bn_backward_f32", dev, raw[i - 1], act[i - 1], da, Rp, cin, self.stat[i - 1],
                     st(P, BN_KEYS[i - 1] + "weight"), BN_EPS, SLOPE, ws, wsn, st(G, BN_KEYS[i - 1] + "weight"),
                     st(G, BN_KEYS[i - 1] + "bias"), da)
                mark("bn bwd")
                d = da
        return self.loss[0]

    def step(self, wav, target, mask=None):
        """forward_backward + Adam; the loss as a device scalar, nothing waits for the host."""
        loss = self.forward_backward(wav, target, mask)
        self.opt.step()
        if self.on_stage:
            self.on_stage("adam")
        return loss

    def eval_model(self):
        """generate.Generator_gru in eval mode over views of THESE weights (and a copy of the running statistics)."""
        P, p = self.params, dict(convs=[], gru=[])
        for i, (cin, cout, stride) in enumerate(CONVS):
            pre = "WavEncoder.feat_extractor.%d." % (3 * i)
            bn = None
            if i < 4:
                bn = torch.stack([self._stored(P, BN_KEYS[i] + "weight"), self._stored(P, BN_KEYS[i] + "bias"),
                                  self.running[i, 0, :cout], self.running[i, 1, :cout]]).contiguous()
            p["convs"].append(dict(w=self._stored(P, pre + "weight"), b=self._stored(P, pre + "bias"), bn=bn, cin=cin,
                                   cout=cout, stride=stride))
        for L, nin in ((0, CONVS[-1][1]), (1, 2 * H)):
            p["gru"].append(dict(nin=nin, w_ih=self._pair(P, "weight_ih", L), b_ih=self._pair(P, "bias_ih", L),
                                 w_hh=self._pair(P, "weight_hh", L), b_hh=self._pair(P, "bias_hh", L)))
        p.update(ln_g=self._stored(P, "norm.weight"), ln_b=self._stored(P, "norm.bias"), out_w=self._stored(P, "out.weight"),
                 out_b=self._stored(P, "out.bias"))
        self._eval.p = p
        return self._eval

    def eval_loss(self, wav, target):
        """The eval-mode loss (running statistics, no dropout) as a 0-d device tensor, through generate.Generator_gru."""
        x = self._wav(wav)
        return self.eval_model().forward(x, self._target(target, x.shape[0] * n_frames(x.shape[1])))[1]


# ---------------------------------------------------------------------------------------------------------------------
# data

def sample_windows(audio_raw, code_raw, n_pose_frames, n_poses=240, stride=10, n_codes=30, fps=60, audio_sample_length=WINDOW):
    """(audio (M, 64000) f32, codes (M, n_codes) int64, start frames): data_preprocessor.py:_sample_from_clip's arithmetic
    for a clip of n_pose_frames poses, taken literally: MINLEN = min(poses, int(len(audio) * 60 / 16000), len(codes) * 8),
    floor((MINLEN - n_poses) / stride) + 1 windows; window i starts at pose frame i * stride, its audio at
    floor(start / len(poses) * len(audio)), its codes are code_raw[start // (n_poses // n_codes) : fin // (n_poses //
    n_codes)].  A window whose audio slice comes out shorter than 64 000 samples raises (the reference would fail when it
    collates the batch)."""
    audio_raw = np.asarray(audio_raw, np.float32).reshape(-1)
    code_raw = np.asarray(code_raw).flatten()
    n_pose_frames = int(n_pose_frames)
    MINLEN = min(n_pose_frames, int(len(audio_raw) * 60 / 16000), len(code_raw) * 8)
    num_subdivision = math.floor((MINLEN - n_poses) / stride) + 1
    per = n_poses // n_codes
    audio, codes, starts = [], [], []
    for i in range(max(num_subdivision, 0)):
        start_idx = i * stride
        fin_idx = start_idx + n_poses
        sample_codes = code_raw[start_idx // per:fin_idx // per]
        audio_start = math.floor(start_idx / n_pose_frames * len(audio_raw))
        sample_audio = audio_raw[audio_start:audio_start + audio_sample_length]
        if len(sample_audio) != audio_sample_length:
            raise ValueError("window %d (pose frame %d) has %d audio samples, %d are needed: the clip's audio is too short "
                             "for its poses" % (i, start_idx, len(sample_audio), audio_sample_length))
        if len(sample_codes) != n_codes:
            raise ValueError("window %d (pose frame %d) has %d codes, %d are needed" % (i, start_idx, len(sample_codes), n_codes))
        audio.append(sample_audio)
        codes.append(sample_codes.astype(np.int64))
        starts.append(start_idx)
    if not audio:
        return np.zeros((0, audio_sample_length), np.float32), np.zeros((0, n_codes), np.int64), np.zeros(0, np.int64)
    return np.stack(audio), np.stack(codes), np.array(starts, np.int64)


def build_dataset(clips, vq, n_poses=240, stride=10, n_codes=30):
    """clips: iterable of (poses (F, D) normalised as the VQ-VAE wants them, audio_raw (n,) at 16 kHz).  Per clip code_raw =
    vq.encode of the whole clip cut to a multiple of 8 frames (one code per 8 frames), then sample_windows.  Returns
    dict(audio (N, 64000) f32, codes (N, 30) int64), what np.savez writes as a training file."""
    audio, codes = [], []
    for poses, audio_raw in clips:
        poses = np.asarray(poses, np.float32)
        F = poses.shape[0] // 8 * 8
        x = torch.from_numpy(poses[None, :F]).to(vq.device)
        code_raw = vq.encode(x)[0].reshape(-1).cpu().numpy()
        a, c, _ = sample_windows(audio_raw, code_raw, poses.shape[0], n_poses=n_poses, stride=stride, n_codes=n_codes)
        audio.append(a)
        codes.append(c)
    return dict(audio=np.concatenate(audio), codes=np.concatenate(codes))


def load_npz(path):
    d = np.load(path)
    audio, codes = np.asarray(d["audio"], np.float32), np.asarray(d["codes"], np.int64)
    if audio.ndim != 2 or codes.ndim != 2 or audio.shape[0] != codes.shape[0] or n_frames(audio.shape[1]) != codes.shape[1]:
        raise ValueError("%s: want audio (N, n) and codes (N, T(n)), got %s and %s" % (path, audio.shape, codes.shape))
    if codes.size and (codes.min() < 0 or codes.max() >= CODES):
        raise ValueError("%s: codes outside [0, %d)" % (path, CODES))
    return audio, codes


def synthetic_data(n, seed):
    """n seeded windows (synth.make_wav) with seeded random codes."""
    from . import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    return synth.make_wav(seed, n, WINDOW), rng.integers(0, CODES, (n, n_frames(WINDOW))).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the loop (end2end.py:46-137 without DataParallel, tensorboard and lmdb)

def validate(tr, audio, codes, batch):
    """Mean of the per-batch eval-mode losses over the drop_last batches in order (evaluate_testset)."""
    nb = len(audio) // batch
    if nb == 0:
        return float("nan")
    tot = torch.zeros((), dtype=torch.float64, device=tr.device)
    for i in range(nb):
        tot += tr.eval_loss(audio[i * batch:(i + 1) * batch], codes[i * batch:(i + 1) * batch]).double()
    return float(tot) / nb


def save_checkpoint(path, args, epoch, tr, rng_state, best, updates):
    torch.save({"args": args, "epoch": epoch, "model_dict": tr.state_dict(prefix="module."),
                "optimizer": tr.opt.state_dict(), "rng": rng_state, "dropout_rng": tr.gen.get_state().cpu(),
                "best": best, "updates": updates}, path)


def settings(cfg):
    e = dict(END2END_DEFAULTS)
    e.update(dict(getattr(cfg, "end2end", {}) or {}))
    return e


def train(args, cfg, log=print):
    """Run the loop; returns (per-update losses, checkpoint paths written, the trainer)."""
    e = settings(cfg)
    epochs = args.epochs if args.epochs is not None else int(e["epochs"])
    save_dir = args.model_save_path or e["model_save_path"]
    batch = args.batch_size if args.batch_size is not None else int(getattr(cfg, "batch_size", 256))
    if args.synthetic:
        tr_audio, tr_codes = synthetic_data(args.synthetic, 1000)
        va_audio, va_codes = synthetic_data(max(batch, args.synthetic // 4), 5000)
    else:
        tr_audio, tr_codes = load_npz(args.train_data)
        va_audio, va_codes = load_npz(args.val_data or args.train_data)
    n_batches = len(tr_audio) // batch
    if n_batches == 0:
        raise SystemExit("fewer training windows (%d) than one batch (%d)" % (len(tr_audio), batch))
    log('len of train loader:{}, len of test loader:{}'.format(n_batches, len(va_audio) // batch))
    dev = torch.device("cuda:%s" % args.gpu)
    ckpt = None
    if args.resume:
        from .checkpoint import load_checkpoint
        ckpt = load_checkpoint(args.resume)
    tr = GeneratorTrainer(device=dev, lr=float(e["lr"]), betas=tuple(e["betas"]), seed=args.seed,
                          state_dict=None if ckpt is None else ckpt["model_dict"])
    tr_audio_d, tr_codes_d = torch.from_numpy(tr_audio).to(dev), torch.from_numpy(tr_codes).to(dev)
    va_audio_d, va_codes_d = torch.from_numpy(va_audio).to(dev), torch.from_numpy(va_codes).to(dev)
    rng = np.random.default_rng(args.seed)
    best, epoch0, updates = (1e+2, 0), 1, 0
    resumed = ckpt is not None and "optimizer" in ckpt
    if resumed:
        tr.opt.load_state_dict(ckpt["optimizer"])
        rng.bit_generator.state = ckpt["rng"]
        tr.gen.set_state(ckpt["dropout_rng"])
        best, epoch0, updates = tuple(ckpt["best"]), int(ckpt["epoch"]), int(ckpt["updates"])
    elif ckpt is not None and ckpt.get("epoch") is not None:
        epoch0 = int(ckpt["epoch"])
    os.makedirs(save_dir, exist_ok=True)
    name = e["name"]
    losses, written = [], []
    from datetime import datetime
    for epoch in range(epoch0, epochs + 1):
        log('Epoch: {}'.format(epoch))
        if not (resumed and epoch == epoch0):                 # (the checkpoint was written behind this epoch's validation)
            loss_eval = validate(tr, va_audio_d, va_codes_d, batch)
            log('loss on validation: {:.3f}'.format(loss_eval))
            is_best = loss_eval < best[0]
            if is_best:
                log(' *** BEST VALIDATION LOSS : {:.3f}'.format(loss_eval))
                best = (loss_eval, epoch)
            else:
                log(' best validation loss so far: {:.3f} at EPOCH {}'.format(best[0], best[1]))
            if is_best or epoch % int(e["save_per_epochs"]) == 0:
                if is_best:
                    save_name = '{}/{}_checkpoint_best.bin'.format(save_dir, name)
                else:
                    save_name = '{}/{}_checkpoint_{:03d}.bin'.format(save_dir, name, epoch)
                save_checkpoint(save_name, args, epoch, tr, rng.bit_generator.state, best, updates)
                written.append(save_name)
                log('Saved the checkpoint')
        perm = torch.from_numpy(rng.permutation(len(tr_audio))[:n_batches * batch]).to(dev)
        start = datetime.now()
        for i in range(n_batches):
            idx = perm[i * batch:(i + 1) * batch]
            lv = float(tr.step(tr_audio_d[idx], tr_codes_d[idx]))
            losses.append(lv)
            stats_str = ' '.join('{}[{:.8f}]'.format(k, v) for k, v in (('updates', updates), ('loss', lv)))
            remaining = str((datetime.now() - start) / (i + 1) * (n_batches - i - 1)).split('.')[0]
            log('> epoch [{}] updates[{}] {} eta[{}]'.format(epoch, i + 1, stats_str, remaining))
            updates += 1
            if args.max_updates and len(losses) >= args.max_updates:
                return losses, written, tr
    log('--------- Final best loss values ---------')
    log('diff mean: {:.3f} at EPOCH {}'.format(best[0], best[1]))
    return losses, written, tr


def build_parser():
    p = argparse.ArgumentParser(description="GRU speech-to-code generator training (the reference's end2end.py)")
    p.add_argument("--config", type=str, default="./configs/codebook.yml")
    p.add_argument("--gpu", type=str, default="0")
    p.add_argument("--train_data", type=str, default=None, help=".npz with audio (N, 64000) f32 and codes (N, 30) int64")
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
    if not args.synthetic and not args.train_data:
        raise SystemExit("give --train_data (or --synthetic N)")
    cfg_path = args.config
    if not os.path.exists(cfg_path):
        cfg_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs", "codebook.yml")
    return train(args, load_config(cfg_path))


if __name__ == "__main__":
    main()
