"""A torch-autograd restatement of the generator's TRAINING forward (codebook/generate/generate.py Generator_gru in
train() mode under codebook/end2end.py's loss), in f64 or f32, with an explicit dropout mask: plumbing-level
torch.nn.functional, the recurrence written out step by step.  tests/test_generator_train_cpu.py pins it to the golden
vectors taken from the reference module; the GPU tests compare the device against it on their own inputs."""
import numpy as np
import torch
import torch.nn.functional as F

CONVS = ((1, 8, 3), (8, 16, 3), (16, 32, 6), (32, 64, 6), (64, 32, 6))
H, SLOPE, MOMENTUM = 200, 0.3, 0.1
ZERO_GRAD_BIASES = tuple("WavEncoder.feat_extractor.%d.bias" % (3 * i) for i in range(4))     # in front of a train-mode BatchNorm
PARAM_KEYS = None


def param_keys(sd):
    return [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def strip(sd):
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def tensors(sd, dtype=torch.float64, grad=True):
    """{key: leaf tensor} of a state dict (arrays or tensors, with or without `module.`)."""
    out = {}
    for k, v in strip(sd).items():
        t = torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v))
        if k.endswith("num_batches_tracked"):
            out[k] = t.clone()
            continue
        t = t.to(dtype).clone()
        if grad and not k.endswith(("running_mean", "running_var")):
            t.requires_grad_(True)
        out[k] = t
    return out


def gru_direction(x, w_ih, w_hh, b_ih, b_hh, reverse):
    B, T, _ = x.shape
    xp = F.linear(x, w_ih, b_ih)
    h = x.new_zeros((B, H))
    outs = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        gh = F.linear(h, w_hh, b_hh)
        r = torch.sigmoid(xp[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(xp[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(xp[:, t, 2 * H:] + r * gh[:, 2 * H:])
        h = (1.0 - z) * n + z * h
        outs[t] = h
    return torch.stack(outs, 1)


def forward(p, wav, target=None, mask=None, drop_p=0.0, train=True):
    """p: tensors(); wav (B, n) tensor of p's dtype; mask (B, T, 400) or None.  Returns (logits (B, T, 512), loss or None,
    {running key: value after the step}).  train: batch statistics and the running update (p itself is not modified);
    eval: the running statistics, no dropout."""
    x = wav.unsqueeze(1)
    running = {}
    for i, (_, cout, stride) in enumerate(CONVS):
        pre = "WavEncoder.feat_extractor.%d." % (3 * i)
        x = F.conv1d(x, p[pre + "weight"], p[pre + "bias"], stride=stride)
        if i < 4:
            q = "WavEncoder.feat_extractor.%d." % (3 * i + 1)
            rm, rv = p[q + "running_mean"].clone(), p[q + "running_var"].clone()
            x = F.batch_norm(x, rm, rv, p[q + "weight"], p[q + "bias"], training=train, momentum=MOMENTUM, eps=1e-5)
            running[q + "running_mean"], running[q + "running_var"] = rm, rv
            x = F.leaky_relu(x, SLOPE)
    x = x.transpose(1, 2)
    for layer in range(2):
        outs = []
        for suffix in ("", "_reverse"):
            tag = "_l%d%s" % (layer, suffix)
            outs.append(gru_direction(x, p["project.weight_ih" + tag], p["project.weight_hh" + tag], p["project.bias_ih" + tag],
                                      p["project.bias_hh" + tag], bool(suffix)))
        x = torch.cat(outs, -1)
        if layer == 0 and train and mask is not None:
            x = x * mask.to(x.dtype) / (1.0 - drop_p)
    s = x[:, :, :H] + x[:, :, H:]
    s = F.layer_norm(s, (H,), p["norm.weight"], p["norm.bias"], 1e-5)
    logits = F.linear(s, p["out.weight"], p["out.bias"])
    loss = None
    if target is not None:
        loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), target.reshape(-1))
    return logits, loss, running


def loss_and_grads(sd, wav, target, mask=None, drop_p=0.0, dtype=torch.float64):
    """(loss float, {key: gradient array in dtype}, {running key: array}) of one training forward + backward."""
    p = tensors(sd, dtype)
    _, loss, running = forward(p, torch.as_tensor(np.asarray(wav)).to(dtype), torch.as_tensor(np.asarray(target)).long(),
                               None if mask is None else torch.as_tensor(np.asarray(mask)), drop_p, True)
    loss.backward()
    grads = {k: p[k].grad.numpy() for k in param_keys(p)}
    return float(loss.detach()), grads, {k: v.detach().numpy() for k, v in running.items()}


def eval_loss(sd, wav, target, dtype=torch.float64):
    p = tensors(sd, dtype, grad=False)
    with torch.no_grad():
        return float(forward(p, torch.as_tensor(np.asarray(wav)).to(dtype), torch.as_tensor(np.asarray(target)).long(),
                             train=False)[1])
