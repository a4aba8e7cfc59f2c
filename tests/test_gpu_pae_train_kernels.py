"""Every kernel of a PAE training step (csrc/qpg_pae_train.hip) against float64, stage by stage.

Each stage's f64 reference is fed the DEVICE's own inputs of that stage (read from the step's workspace,
tests/pae_train_ref.ws_regions), so a failure names the stage that broke.  Contractions are held entry by entry to
gamma(n) * (|a| * |b|) with oracle.vqtrain_oracle's gamma / bound_ratio (n the f32 accumulation chain, plus the slabs
a weight gradient adds in f64); element-wise stages to a few units of roundoff of the magnitudes they combine, as
each check states.  The largest err / bound of every stage is printed.  All entries are compared, so the padding
positions at both ends of every convolution are included; the batch holds the first window of the data and one ending
at its last frame."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv1d_input, conv1d_weight

from oracle.vqtrain_oracle import bound_ratio, gamma
from qpgesture_amd import PAE_train as PT, synth
from tests import pae_train_ref as R
from tests.test_gpu_pae_train import _data, _starts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
T, E, C, M = PT.TIME, PT.EMBED, PT.IN_CH, PT.MID_CH
EPS = 1e-5


def _bn_train(z, dims):
    mean = z.mean(dims, keepdim=True)
    var = ((z - mean) ** 2).mean(dims, keepdim=True)
    return (z - mean) / torch.sqrt(var + EPS), 1.0 / torch.sqrt(var + EPS)


def _bn_bwd(z, h, dh, gam, dims):
    """Train-mode BatchNorm + tanh backward in f64 and its bound magnitude (|dh| carries the roundoff of the f32
    dA = dh (1 - h^2))."""
    xh, inv = _bn_train(z, dims)
    da = dh * (1 - h * h)
    dz = gam * inv * (da - da.mean(dims, keepdim=True) - xh * (da * xh).mean(dims, keepdim=True))
    mag = (gam * inv).abs() * (dh.abs() + dh.abs().mean(dims, keepdim=True) + xh.abs() * (dh * xh).abs().mean(dims, keepdim=True))
    return dz, mag, da.sum(dims), (da * xh).sum(dims), dh.abs().sum(dims), (dh * xh).abs().sum(dims)


class Step:
    def __init__(self, B):
        pn, all_starts = _data()
        self.B = B
        self.tr = PT.Trainer(synth.make_pae_state_dict(11), batch=B, device=DEV)
        self.tr.set_data(pn)
        self.starts = _starts(all_starts, B, 3)
        self.tr.forward(self.starts, train=True)
        self.tr.backward()
        self.pn = pn
        self.p = R.params_from_flat(self.tr.params.cpu(), requires_grad=False)
        self.G = self.tr.grads.cpu().double()
        self.ws = self.tr.ws
        assert self.ws.numel() == R.ws_regions(B)["_floats"], "the workspace mirror disagrees with the library"
        self.ratios = {}

    def get(self, name):
        return R.ws_get(self.ws, self.B, name)

    def grad(self, name):
        shape = dict(PT.PARAMS)[name]
        return self.G[PT.OFF[name]:PT.OFF[name] + int(np.prod(shape))].reshape(shape)

    def check(self, label, got, ref, absref, g):
        r = bound_ratio(got, ref, absref, g)
        self.ratios[label] = r
        assert r <= 1.0, (label, r)


def _conv(st, label, out, x, w, b, pad):
    ref = F.conv1d(x, w, b, padding=pad)
    mag = F.conv1d(x.abs(), w.abs(), b.abs(), padding=pad)
    st.check(label, out, ref, mag, gamma(w.shape[1] * T))


def _wgrad(st, label, x, dy, wname, pad):
    w = st.p[wname]
    S = min(st.B, 16)
    ref = conv1d_weight(x, w.shape, dy, padding=pad)
    mag = conv1d_weight(x.abs(), w.shape, dy.abs(), padding=pad)
    st.check(label + " weight grad", st.grad(wname), ref, mag, gamma(-(-st.B // S) * dy.shape[2], S))
    bname = wname.replace(".weight", ".bias")
    st.check(label + " bias grad", st.grad(bname), dy.sum((0, 2)), dy.abs().sum((0, 2)), gamma(1))


def _dgrad(st, label, got, x_shape, dy, wname, pad):
    w = st.p[wname]
    ref = conv1d_input(x_shape, w, dy, padding=pad)
    mag = conv1d_input(x_shape, w.abs(), dy.abs(), padding=pad)
    st.check(label + " data grad", got, ref, mag, gamma(w.shape[0] * T))


def _bn_fwd(st, label, z, h, bn):
    xh, _ = _bn_train(z, (0, 2))
    gam, bet = st.p[bn + ".weight"][None, :, None], st.p[bn + ".bias"][None, :, None]
    # xhat rounded once, times gamma, plus beta, tanhf: <= 4 roundings of |gamma xhat| + |beta| + 1
    st.check(label, h, torch.tanh(gam * xh + bet), (gam * xh).abs() + bet.abs() + 1, 8 * U)


def _bn_back(st, label, z, h, dh, dz, bn):
    gam = st.p[bn + ".weight"][None, :, None]
    ref, mag, dbeta, dgam, m0, m1 = _bn_bwd(z, h, dh, gam, (0, 2))
    st.check(label + " BN backward", dz, ref, mag, 8 * U)
    st.check(label + " BN weight grad", st.grad(bn + ".weight"), dgam, m1, 8 * U)
    st.check(label + " BN bias grad", st.grad(bn + ".bias"), dbeta, m0, 8 * U)


@pytest.mark.parametrize("B", [256, 2])
def test_every_stage_against_f64(B):
    st = Step(B)
    p = st.p
    x0 = st.get("x0")
    want_x0 = R.windows_input(torch.from_numpy(st.pn), st.starts, True).reshape(B, C, T).double()
    assert torch.equal(x0, want_x0), "gather: the f32 velocity differences are not bit-identical"

    # ---- forward
    z1, h1, z2, h2 = st.get("z1"), st.get("h1"), st.get("z2"), st.get("h2")
    _conv(st, "conv1", z1, x0, p["conv1.weight"], p["conv1.bias"], T // 2)
    _bn_fwd(st, "bn_conv1 + tanh", z1, h1, "bn_conv1")
    _conv(st, "conv2", z2, h1, p["conv2.weight"], p["conv2.bias"], (T - 1) // 2)
    _bn_fwd(st, "bn_conv2 + tanh", z2, h2, "bn_conv2")

    v, vn, pfab = st.get("v"), st.get("vn"), st.get("pfab")
    wfc = torch.stack([p["fc.%d.weight" % e] for e in range(E)])                # (8, 2, 240)
    bfc = torch.stack([p["fc.%d.bias" % e] for e in range(E)])                  # (8, 2)
    st.check("fc", v, torch.einsum("bet,ejt->bej", h2, wfc) + bfc,
             torch.einsum("bet,ejt->bej", h2.abs(), wfc.abs()) + bfc.abs(), gamma(1))
    gfc = torch.stack([p["bn.%d.weight" % e] for e in range(E)])
    bfcn = torch.stack([p["bn.%d.bias" % e] for e in range(E)])
    xh_v, inv_v = _bn_train(v, (0,))
    st.check("fc BN", vn, gfc * xh_v + bfcn, (gfc * xh_v).abs() + bfcn.abs(), 8 * U)
    rf = torch.fft.rfft(h2, dim=2)
    pw = rf.abs()[:, :, 1:] ** 2
    ts = PT.KEYS / T
    f_ref = (p["freqs"] * pw).sum(2) / pw.sum(2) / ts
    a_ref = 2 * torch.sqrt(pw.sum(2)) / T
    b_ref = rf.real[:, :, 0] / T
    tpi = p["tpi"]
    for k, (name, ref) in enumerate((("f", f_ref), ("a", a_ref), ("b", b_ref))):
        # f64 DFT and sums, rounded once: 2 u of the value (|X_0| / 240 for the offset)
        mag = ref.abs() if name != "b" else h2.abs().sum(2) / T
        st.check("spectrum " + name, pfab[:, k + 1], ref, mag, 4 * U)
    p_ref = R._atan2p(vn[:, :, 1], vn[:, :, 0], tpi) / tpi
    # f32 y / x, atanf, +- tpi / 2, / tpi: a few roundings of |angle| + pi, over tpi
    st.check("atan2'", pfab[:, 0], p_ref, (p_ref.abs() * tpi + math.pi) / tpi, 8 * U)

    sig = st.get("sig")
    a, f, pp, bb = pfab[:, 2, :, None], pfab[:, 1, :, None], pfab[:, 0, :, None], pfab[:, 3, :, None]
    th = tpi * (f * p["args"] + pp)
    # theta formed in f32 (3 roundings of |tpi f args| + |tpi p|), sinf, a *, + b
    st.check("signal", sig, a * torch.sin(th) + bb,
             a.abs() * ((tpi * f * p["args"]).abs() + (tpi * pp).abs() + 1) + bb.abs(), 8 * U)
    z3, h3, y = st.get("z3"), st.get("h3"), st.get("y")
    _conv(st, "deconv1", z3, sig, p["deconv1.weight"], p["deconv1.bias"], (T - 1) // 2)
    _bn_fwd(st, "bn_deconv1 + tanh", z3, h3, "bn_deconv1")
    _conv(st, "deconv2", y, h3, p["deconv2.weight"], p["deconv2.bias"], T // 2)

    loss = st.tr.loss.cpu()[0]                                  # (the caller-given loss buffer)
    n = B * C * T
    d = y - x0
    st.check("loss", loss, 300 * (d * d).sum() / n, 300 * (d * d).sum() / n, 4 * U)
    dy = st.get("dy")
    st.check("loss gradient", dy, 600.0 / n * d, 600.0 / n * (y.abs() + x0.abs()), 4 * U)

    # ---- backward
    _wgrad(st, "deconv2", h3, dy, "deconv2.weight", T // 2)
    dh3 = st.get("dh3")
    _dgrad(st, "deconv2", dh3, h3.shape, dy, "deconv2.weight", T // 2)
    dz3 = st.get("dz3")
    _bn_back(st, "bn_deconv1", z3, h3, dh3, dz3, "bn_deconv1")
    _wgrad(st, "deconv1", sig, dz3, "deconv1.weight", (T - 1) // 2)
    ds = st.get("ds")
    _dgrad(st, "deconv1", ds, sig.shape, dz3, "deconv1.weight", (T - 1) // 2)

    # signal and atan2' backward (per window and channel: f64 sums over t of f32-theta terms)
    dfab, dvn = st.get("dfab"), st.get("dvn")
    args = p["args"]
    sn, cs = torch.sin(th), torch.cos(th)
    dth = ds * a * cs
    want = (tpi * (dth * args).sum(2), (ds * sn).sum(2), ds.sum(2))
    mag_t = ds.abs() * (1 + a.abs()) * (1 + (tpi * f * args).abs() + (tpi * pp).abs()) * tpi * (1 + args.abs())
    for k, name in enumerate(("df", "da", "db")):
        st.check("signal backward " + name, dfab[:, k], want[k], mag_t.sum(2), 8 * U)
    dp = tpi * dth.sum(2)
    x, yv = vn[:, :, 0], vn[:, :, 1]
    r2 = x * x + yv * yv
    dvn_ref = torch.stack((-dp / tpi * yv / r2, dp / tpi * x / r2), -1)
    dvn_mag = (tpi * mag_t.sum(2) / tpi / r2)[..., None] * torch.stack((yv.abs(), x.abs()), -1) + dvn_ref.abs()
    st.check("atan2' backward", dvn, dvn_ref, dvn_mag, 8 * U)
    # fc BatchNorm backward over the batch, fc gradients
    dv = st.get("dv")
    dv_ref = gfc * inv_v * (dvn - dvn.mean(0) - xh_v * (dvn * xh_v).mean(0))
    dv_mag = (gfc * inv_v).abs() * (dvn.abs() + dvn.abs().mean(0) + xh_v.abs() * (dvn * xh_v).abs().mean(0))
    st.check("fc BN backward", dv, dv_ref, dv_mag, 8 * U)
    for e in range(E):
        st.check("fc BN weight grad", st.grad("bn.%d.weight" % e), (dvn * xh_v).sum(0)[e],
                 (dvn * xh_v).abs().sum(0)[e], 8 * U)
        st.check("fc BN bias grad", st.grad("bn.%d.bias" % e), dvn.sum(0)[e], dvn.abs().sum(0)[e], 8 * U)
        st.check("fc weight grad", st.grad("fc.%d.weight" % e), torch.einsum("bj,bt->jt", dv[:, e], h2[:, e]),
                 torch.einsum("bj,bt->jt", dv[:, e].abs(), h2[:, e].abs()), gamma(1))
    # DFT backward: autograd of f, a, b, fc(h2) in f64 with the device's df, da, db, dv as upstream gradients
    h2l = h2.clone().requires_grad_(True)
    rfl = torch.fft.rfft(h2l, dim=2)
    pwl = rfl.abs()[:, :, 1:] ** 2
    fl = (p["freqs"] * pwl).sum(2) / pwl.sum(2) / ts
    al = 2 * torch.sqrt(pwl.sum(2)) / T
    bl = rfl.real[:, :, 0] / T
    vl = torch.einsum("bet,ejt->bej", h2l, wfc)
    (fl * dfab[:, 0] + al * dfab[:, 1] + bl * dfab[:, 2] + (vl * dv).sum(2)).sum().backward()
    psum = pw.sum(2)
    gm = (dfab[:, 0, :, None] * (p["freqs"] - (p["freqs"] * pw).sum(2, keepdim=True) / psum[..., None]).abs()
          / (psum[..., None] * ts)).abs() + (dfab[:, 1, :, None] / (T * torch.sqrt(psum[..., None]))).abs()
    spec_mag = 2 * torch.einsum("bem,bem->be", gm, (rf.real[:, :, 1:].abs() + rf.imag[:, :, 1:].abs()))[..., None]
    dh2_mag = torch.einsum("bej,ejt->bet", dv.abs(), wfc.abs()) + dfab[:, 2, :, None].abs() / T + spec_mag
    dh2 = st.get("dh2")
    st.check("DFT + fc backward", dh2, h2l.grad, dh2_mag, gamma(T))

    dz2 = st.get("dz2")
    _bn_back(st, "bn_conv2", z2, h2, dh2, dz2, "bn_conv2")
    _wgrad(st, "conv2", h1, dz2, "conv2.weight", (T - 1) // 2)
    dh1 = st.get("dh1")
    _dgrad(st, "conv2", dh1, h1.shape, dz2, "conv2.weight", (T - 1) // 2)
    dz1 = st.get("dz1")
    _bn_back(st, "bn_conv1", z1, h1, dh1, dz1, "bn_conv1")
    _wgrad(st, "conv1", x0, dz1, "conv1.weight", T // 2)

    print("\nB=%d largest err / bound per stage:" % B)
    for k, r in st.ratios.items():
        print("  %-28s %.3g" % (k, r))


def test_adamw_entry_point_matches_reference_trace():
    """qpg_pae_adamw_f32 against the reference AdamW's 5 steps with varying lr and weight decay (golden trace): the
    f64 restatement per step (itself pinned to the trace on the CPU) bounds the device's f32 update."""
    import os
    from qpgesture_amd import _lib
    gold = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pae_train_s11.npz")))
    p = torch.from_numpy(gold["adamw_p0"].copy()).to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for k in range(5):
        lr, wd = (float(x) for x in gold["adamw_lr_wd"][k])
        g = torch.from_numpy(gold["adamw_g"][k].copy()).to(DEV)
        p64, m64, v64 = (t.cpu().double().numpy() for t in (p, m, v))
        want, _, _ = R.adamw_step(p64, g.cpu().double().numpy(), m64, v64, lr, wd, k + 1)
        _lib.call("qpg_pae_adamw_f32", DEV, p, g, m, v, p.numel(), lr, wd, 0.9, 0.999, 1e-8, k + 1)
        got = p.cpu().double().numpy()
        # one step: f32 roundings of p (1 - wd) and of the normalised step of size <= lr * sqrt(1 - b2^t) / (1 - b1^t)
        step = lr * math.sqrt(1 - 0.999 ** (k + 1)) / (1 - 0.9 ** (k + 1))
        assert np.all(np.abs(got - want) <= 8 * U * (np.abs(want) + 4 * step)), k
        np.testing.assert_allclose(got, gold["adamw_p"][k], rtol=0, atol=2e-6 * (1 + np.abs(got)).max())
