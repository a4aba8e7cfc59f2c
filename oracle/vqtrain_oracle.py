"""ORACLE (test infrastructure, not product): float64 references of the VQ-VAE training-step kernels and the a-priori
f32 error bounds the tests hold them to (tests/test_gpu_vqtrain_kernels.py, tests/test_vqtrain_oracle_cpu.py).

Convolution gradients are torch autograd in float64 of F.conv1d / F.conv_transpose1d / the residual block
x + conv1(relu(conv3_dil(relu(x)))), on channels-last (B, T, C) activations.  The bound of every entry is

    |got - ref| <= gamma * (|x| * |dy|)

where `*` is the same contraction taken on absolute values (the same autograd call on |x|, |w|, |dy| with the ReLUs
replaced by the identity, so that every product the kernel adds is counted with its magnitude), and

    gamma = LAMBDA * u * sum_i sqrt(n_i) + 2 u,     u = 2^-24,

n_i the lengths of the f32 accumulation chains the value went through (the contraction of each launch along the
chain, plus the number of split partials added afterwards), 2 u for the rounding of stored operands and the final
store.  This is the probabilistic rounding-error bound of an inner product (Higham & Mary, SIAM J. Sci. Comput.
41(5), 2019: |error| <= lambda sqrt(n) u sum|a_i b_i| with probability >= 1 - 2 exp(-lambda^2 (1-u)^2 / 2)); LAMBDA = 4
puts that failure probability per entry below 1e-3, and the entries the tests see are far below the bound (their
largest err / bound is printed).  The deterministic worst case, n u, is not used: at the 61 440-position weight
gradients of a batch-256 step it is 3.7e-3 of the absolute contraction, loose enough to let a dropped position row,
a shifted tap or a doubled bias pass (tests/test_vqtrain_oracle_cpu.py shows the bound used here rejects each).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
LAMBDA = 4.0


def gamma(*chains):
    """f32 error coefficient of a value computed through accumulation chains of the given lengths."""
    return LAMBDA * U * sum(math.sqrt(max(int(n), 1)) for n in chains) + 2 * U


def _f64(a):
    return torch.as_tensor(a).detach().to("cpu", torch.float64)


def _layer(kind, x, ws, bs, dil, exact):
    """Forward of one tape operation on channels-first f64 x.  exact=False: the ReLUs become identities (the
    contraction on absolute values)."""
    relu = F.relu if exact else (lambda v: v)
    if kind == "conv3":
        return F.conv1d(x, ws[0], bs[0], padding=1)
    if kind == "down":
        return F.conv1d(x, ws[0], bs[0], stride=2, padding=1)
    if kind == "up":
        return F.conv_transpose1d(x, ws[0], bs[0], stride=2, padding=1)
    if kind == "res":
        h = relu(F.conv1d(relu(x), ws[0], bs[0], padding=dil, dilation=dil))
        return x + F.conv1d(h, ws[1], bs[1])
    raise ValueError(kind)


def layer_grads(kind, x, dy, ws, bs, dil=1):
    """Gradients of one tape operation and their bounds' contraction.
    kind: "conv3" (k3 s1 p1), "down" (k4 s2 p1), "up" (ConvTranspose1d k4 s2 p1, weight (Cin, Cout, 4)) or "res"
    (ws = (w3, w1), bs = (b3, b1), dilation dil).  x: (B, T, Cin) input, dy: (B, T_out, Cout) gradient of the output,
    weights in torch's layouts.  Returns (grads, absgrads): dicts with dx (B, T, Cin), dw [..], db [..] as f64 tensors;
    absgrads is the same autograd call on |x|, |w|, |dy| with identity for ReLU."""
    out = []
    for exact in (True, False):
        f = (lambda a: a) if exact else torch.abs
        xt = f(_f64(x)).permute(0, 2, 1).contiguous().requires_grad_(True)
        wt = [f(_f64(w)).requires_grad_(True) for w in ws]
        bt = [_f64(b).requires_grad_(True) for b in bs]
        y = _layer(kind, xt, wt, bt, dil, exact)
        g = f(_f64(dy)).permute(0, 2, 1)
        assert y.shape == g.shape, (y.shape, g.shape)
        r = torch.autograd.grad(y, [xt] + wt + bt, g)
        n = len(ws)
        out.append(dict(dx=r[0].permute(0, 2, 1).contiguous(), dw=list(r[1:1 + n]), db=list(r[1 + n:])))
        del xt, wt, bt, y, g, r
    return out[0], out[1]


def bound_ratio(got, ref, absref, g):
    """Largest |got - ref| / (g * absref) over the entries (0 / 0 counts as 0; a nonzero error over a zero bound as
    inf).  <= 1 means every entry is inside its bound."""
    got, ref, absref = _f64(got), _f64(ref), _f64(absref)
    assert got.shape == ref.shape == absref.shape, (got.shape, ref.shape, absref.shape)
    err = (got - ref).abs()
    bnd = g * absref
    ok0 = (err == 0)
    r = torch.where(ok0, torch.zeros_like(err), err / torch.where(bnd > 0, bnd, torch.full_like(bnd, 1e-300)))
    return float(r.max()) if r.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------
# code sums (qpg_vq_code_sums_f32)
# ----------------------------------------------------------------------------------------------------------------
CODE_SUMS_CHUNK = 1024


def code_sums_ref(z, ids, K):
    """f64 sums of the rows of z (R, E) per code and exact counts: (sums (K, E) f64, counts (K,) int64,
    abs_sums (K, E) f64)."""
    z = np.asarray(z, np.float64)
    ids = np.asarray(ids, np.int64)
    s = np.zeros((K, z.shape[1]), np.float64)
    a = np.zeros((K, z.shape[1]), np.float64)
    np.add.at(s, ids, z)
    np.add.at(a, ids, np.abs(z))
    return s, np.bincount(ids, minlength=K).astype(np.int64), a


def code_sums_bound(counts, abs_sums, ref):
    """|got - ref| per entry: n_c u sum|z| (the f32 chain of a code's n_c rows) + u |ref| (its final rounding)."""
    return counts[:, None].astype(np.float64) * U * abs_sums + U * np.abs(ref)


def code_sums_chunked_f32(z, ids, K, chunk=CODE_SUMS_CHUNK):
    """What qpg_vq_code_sums_f32 promises, restated in f32: within each chunk of `chunk` rows a code's rows are added
    in ascending row order from +0; the chunk partials of the chunks that hold rows of the code are then added in
    chunk order from +0.  (Not the plain ascending sum over all rows: the partials are rounded per chunk.)"""
    z = np.asarray(z, np.float32)
    ids = np.asarray(ids, np.int64)
    R, E = z.shape
    tot = np.zeros((K, E), np.float32)
    for r0 in range(0, R, chunk):
        part = np.zeros((K, E), np.float32)
        seen = np.zeros(K, bool)
        for r in range(r0, min(R, r0 + chunk)):
            c = ids[r]
            part[c] = part[c] + z[r]
            seen[c] = True
        tot[seen] = tot[seen] + part[seen]
    return tot


# ----------------------------------------------------------------------------------------------------------------
# Adam (qpg_adam_step_f32)
# ----------------------------------------------------------------------------------------------------------------
def adam_step_f64(p, g, m, v, lr, b1, b2, eps, step):
    """One Adam step (torch.optim.Adam, no weight decay / amsgrad) in float64 with the coefficients as given: pass
    the f32-rounded lr / betas / eps the kernel receives to isolate the kernel's own rounding.  Returns (p, m, v)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps))
    return p, m, v
