"""The generator's TRAINING kernels one by one (the qpg_gen_* training section of include/qpg.h) against NumPy / torch in
f64 fed the device's own inputs of that stage, at the kernels' block, slab and tile edges, with tests/poison.py fences on
outputs and poisoned scratch.

Tolerance: |device - f64| <= MARGIN = 8 x e32 per tensor, e32 = max |f32 run - f64 run| of the same restatement on the
same inputs.  Each check prints its ratio first."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from qpgesture_amd import _lib
from qpgesture_amd import generate as G
from tests import poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 8.0
H = 200
GBT = 16
NAN_FILL = poison.FILLS["ones_ff"]
TD = {np.float64: torch.float64, np.float32: torch.float32}


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C", copy=True)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def out_of(shape, dtype=torch.float32):
    return poison.fenced(shape, dtype, NAN_FILL, device=DEV)


def scratch(n):
    """n floats of NaN-poisoned workspace between fences."""
    g = poison.guarded(int(n) * 4, NAN_FILL, device=DEV)
    return g.view(torch.float32), g


def check(name, got, ref64, ref32, scale=None):
    got = host(got).astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert np.isfinite(got).all(), name
    e32 = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) if scale is None else scale
    err = float(np.abs(got - ref64).max())
    print("%s: err %.3e e32 %.3e ratio %.2f" % (name, err, e32, err / e32 if e32 else float(err > 0)))
    assert err <= MARGIN * e32, "%s: |device - f64| = %.3e > %g x e32 (%.3e)" % (name, err, MARGIN, e32)


def test_constants_match_the_header():
    assert (_lib.QPG_GEN_TRAIN_MAX_SLABS, _lib.QPG_GEN_TRAIN_SLAB_MIN_ROWS, _lib.QPG_GEN_BN_MAX_BLOCKS, _lib.QPG_GEN_GRU_SAVED) == (
        1024, 64, 1024, 4)
    lib = _lib.load()
    assert lib.qpg_gen_rowgrad_ws_floats(512, 208, 3) == 3 * (512 * 208 + 512)
    assert lib.qpg_gen_conv1d_wgrad_ws_floats(8, 16, 2) == 2 * (16 * 128 + 16)
    assert lib.qpg_gen_bn_ws_floats(2, 8) == 2 * (2 * 8 + 2 * 8) and lib.qpg_gen_bn_ws_floats(10, 12) == 0


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------
def bn_rows(C):
    rpb = 1024 // C              # rows a block takes per pass
    edge = _lib.QPG_GEN_BN_MAX_BLOCKS * rpb          # the row count at which every block has exactly one row group
    return [2, 3, rpb - 1, rpb, rpb + 1, edge - 1, edge, edge + 1, 2 * edge + 5]


def bn_backward_np(x, y, dy, mean, var, gamma, dtype):
    x, y, dy, mean, var, gamma = (np.asarray(a, dtype) for a in (x, y, dy, mean, var, gamma))
    R = x.shape[0]
    rstd = (1.0 / np.sqrt(var + dtype(1e-5))).astype(dtype)
    dyh = np.where(y > 0, dy, dy * dtype(0.3)).astype(dtype)
    xh = ((x - mean) * rstd).astype(dtype)
    dbeta, dgamma = dyh.sum(0, dtype=dtype), (dyh * xh).sum(0, dtype=dtype)
    dx = (gamma * rstd) * (dyh - dbeta / dtype(R) - xh * (dgamma / dtype(R)))
    return dx.astype(dtype), dgamma, dbeta


@pytest.mark.parametrize("C", [8, 16, 32, 64])
def test_batchnorm_stats_apply_backward_at_block_edges(C):
    rng = rng_of(400 + C)
    gamma = (rng.uniform(0.6, 1.4, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    gamma[0], gamma[1] = -abs(gamma[0]), 0.0                     # a negative gamma; gamma = beta = 0: outputs exactly 0
    beta = (rng.standard_normal(C) * 0.1).astype(np.float32)
    beta[1] = 0.0
    for R in bn_rows(C):
        x = (rng.standard_normal((R, C)) * rng.uniform(0.5, 2.0, C) + rng.standard_normal(C)).astype(np.float32)
        dy = rng.standard_normal((R, C)).astype(np.float32)
        rm0, rv0 = (rng.standard_normal(C) * 0.05).astype(np.float32), rng.uniform(0.05, 0.2, C).astype(np.float32)
        n_ws = _lib.load().qpg_gen_bn_ws_floats(R, C)
        ws, ws_guard = scratch(n_ws)
        stat, st_guard = out_of((2, C))
        rm, rv = dev(rm0), dev(rv0)
        xd = dev(x)
        _lib.call("qpg_gen_bn_stats_f32", DEV, xd, R, C, ws, n_ws, stat, rm, rv, 0.1)
        refs = {}
        for dt in (np.float64, np.float32):
            xx = x.astype(dt)
            mean = xx.mean(0, dtype=dt)
            var = ((xx - mean) ** 2).mean(0, dtype=dt)
            refs[dt] = (mean, var, (1 - dt(0.1)) * rm0.astype(dt) + dt(0.1) * mean,
                        (1 - dt(0.1)) * rv0.astype(dt) + dt(0.1) * var * dt(R) / dt(R - 1))
        tag = "bn C %d R %d " % (C, R)
        check(tag + "mean", stat[0], refs[np.float64][0], refs[np.float32][0])
        check(tag + "var", stat[1], refs[np.float64][1], refs[np.float32][1])
        check(tag + "running_mean", rm, refs[np.float64][2], refs[np.float32][2])
        check(tag + "running_var (R / (R - 1))", rv, refs[np.float64][3], refs[np.float32][3])
        # without running statistics nothing else changes
        stat2, _ = out_of((2, C))
        _lib.call("qpg_gen_bn_stats_f32", DEV, xd, R, C, ws, n_ws, stat2, None, None, 0.1)
        assert torch.equal(stat2, stat)
        # apply, on the device's own statistics
        y, y_guard = out_of((R, C))
        _lib.call("qpg_gen_bn_apply_f32", DEV, xd, R, C, stat, dev(gamma), dev(beta), 1e-5, 0.3, y)
        sm, sv = host(stat[0]), host(stat[1])
        ys = {}
        for dt in (np.float64, np.float32):
            v = (x.astype(dt) - sm.astype(dt)) * (1.0 / np.sqrt(sv.astype(dt) + dt(1e-5))).astype(dt) * gamma.astype(dt) + beta.astype(dt)
            ys[dt] = np.where(v > 0, v, v * dt(0.3))
        check(tag + "apply", y, ys[np.float64], ys[np.float32])
        assert np.all(host(y)[:, 1] == 0)
        # backward, on the device's own y and statistics
        dx, dx_guard = out_of((R, C))
        dgb, dgb_guard = out_of((2, C))
        _lib.call("qpg_gen_bn_backward_f32", DEV, xd, y, dev(dy), R, C, stat, dev(gamma), 1e-5, 0.3, ws, n_ws, dgb[0], dgb[1], dx)
        b64 = bn_backward_np(x, host(y), dy, sm, sv, gamma, np.float64)
        b32 = bn_backward_np(x, host(y), dy, sm, sv, gamma, np.float32)
        for name, got, i in ((tag + "dx", dx, 0), (tag + "dgamma", dgb[0], 1), (tag + "dbeta", dgb[1], 2)):
            check(name, got, b64[i], b32[i])
        for g in (ws_guard, st_guard, y_guard, dx_guard, dgb_guard):
            g.assert_tail_intact(tag)


def test_batchnorm_refuses_other_widths_and_single_rows():
    x = torch.zeros(4096, device=DEV)
    for C in (4, 12, 128):
        with pytest.raises(_lib.Unsupported):
            _lib.call("qpg_gen_bn_stats_f32", DEV, x, 8, C, x, 4096, x, None, None, 0.1)
        with pytest.raises(_lib.Unsupported):
            _lib.call("qpg_gen_bn_apply_f32", DEV, x, 8, C, x, x, x, 1e-5, 0.3, x)
        with pytest.raises(_lib.Unsupported):
            _lib.call("qpg_gen_bn_backward_f32", DEV, x, x, x, 8, C, x, x, 1e-5, 0.3, x, 4096, x, x, x)
    with pytest.raises(RuntimeError):
        _lib.call("qpg_gen_bn_stats_f32", DEV, x, 1, 8, x, 4096, x, None, None, 0.1)


# ---- convolution gradients ------------------------------------------------------------------------------------------------
def conv_grads(x, w, bias, dy, stride, dtype):
    """torch autograd on nn.Conv1d's arithmetic: x (B, Tin, Cin), w (Cout, Cin, 16), dy (B, T, Cout) -> dx, dw, db."""
    xt = torch.from_numpy(x.astype(dtype)).transpose(1, 2).contiguous().requires_grad_(True)
    wt = torch.from_numpy(w.astype(dtype)).requires_grad_(True)
    bt = torch.from_numpy(bias.astype(dtype)).requires_grad_(True)
    y = F.conv1d(xt, wt, bt, stride=stride)
    y.backward(torch.from_numpy(dy.astype(dtype)).transpose(1, 2))
    return xt.grad.transpose(1, 2).numpy(), wt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("layer", range(5))
def test_conv_gradients_shapes_tile_edges_and_uncovered_tail(layer):
    cin, cout, stride = G.CONVS[layer]
    rng = rng_of(500 + layer)
    w = (rng.standard_normal((cout, cin, 16)) * 2.0 / np.sqrt(cin * 16)).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    w_dev = dev(w.transpose(0, 2, 1))
    lib = _lib.load()
    for B in (1, 3):
        for T in (1, 2, 63, 64, 65, 127, 128, 129):              # the slab floor of 64 rows, the forward's 128-frame tile
            for rem in (0, stride - 1):
                t_in = stride * (T - 1) + 16 + rem
                x = rng.standard_normal((B, t_in, cin)).astype(np.float32)
                dy = rng.standard_normal((B, T, cout)).astype(np.float32)
                r64, r32 = conv_grads(x, w, bias, dy, stride, np.float64), conv_grads(x, w, bias, dy, stride, np.float32)
                tag = "conv%d B %d T %d rem %d " % (layer + 1, B, T, rem)
                xd = dev(x)
                if rem:
                    xd[:, t_in - rem:, :] = float("nan")         # never read by the weight gradient
                n_ws = lib.qpg_gen_conv1d_wgrad_ws_floats(cin, cout, 8)
                ws, ws_guard = scratch(n_ws)
                runs = []
                for _ in range(2):
                    dw, dw_guard = out_of((cout, 16, cin))
                    db, db_guard = out_of((cout,))
                    _lib.call("qpg_gen_conv1d_bwd_weight_f32", DEV, xd, B, t_in, cin, dev(dy), cout, stride, dw, db, ws, n_ws)
                    runs.append((dw.clone(), db.clone()))
                    dw_guard.assert_tail_intact(tag + "dw")
                    db_guard.assert_tail_intact(tag + "db")
                    ws.fill_(123.0)                               # (scratch contents on entry are ignored)
                ws_guard.assert_tail_intact(tag + "ws")
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), tag
                check(tag + "dw", runs[0][0], r64[1].transpose(0, 2, 1), r32[1].transpose(0, 2, 1))
                check(tag + "db", runs[0][1], r64[2], r32[2])
                if layer == 0:
                    continue
                dx, dx_guard = out_of((B, t_in, cin))
                _lib.call("qpg_gen_conv1d_bwd_data_f32", DEV, dev(dy), B, t_in, cin, w_dev, cout, stride, dx)
                check(tag + "dx", dx, r64[0], r32[0])
                if rem:
                    assert np.all(host(dx)[:, t_in - rem:] == 0), tag + "uncovered frames"
                dx_guard.assert_tail_intact(tag + "dx")


def test_conv_gradients_refuse_what_they_are_not_built_for():
    x = torch.zeros(1 << 16, device=DEV)
    for cin, cout, stride in ((4, 16, 3), (8, 24, 3), (8, 16, 2), (128, 16, 3), (1, 16, 3)):
        with pytest.raises(_lib.Unsupported):
            _lib.call("qpg_gen_conv1d_bwd_data_f32", DEV, x, 1, 16, cin, x, cout, stride, x)
    for cin, cout in ((1, 12), (2, 16), (8, 24), (8, 80)):
        with pytest.raises(_lib.Unsupported):
            _lib.call("qpg_gen_conv1d_bwd_weight_f32", DEV, x, 1, 16, cin, x, cout, 3, x, x, x, 1 << 16)


# ---- the recurrence -------------------------------------------------------------------------------------------------------
def gru_weights(seed):
    rng = rng_of(seed)
    b = 3.0 / np.sqrt(H)
    return rng.uniform(-b, b, (2, 3 * H, H)).astype(np.float32), rng.uniform(-b, b, (2, 3 * H)).astype(np.float32)


def gru_train_device(xp, w_hh, b_hh):
    B, T = xp.shape[:2]
    out, og = out_of((B, T, 2 * H))
    sv, sg = out_of((B, T, 2, 4, H))
    _lib.call("qpg_gen_gru_layer_train_f32", DEV, dev(xp), dev(w_hh), dev(b_hh), B, T, H, out, sv)
    og.assert_tail_intact("gru out")
    sg.assert_tail_intact("gru saved")
    return out, sv


def gru_backward_device(dout, sv, out, w_hh):
    B, T = dout.shape[:2]
    dxp, g1 = out_of((B, T, 2, 3 * H))
    dgh, g2 = out_of((B, T, 2, 3 * H))
    whhT = dev(np.ascontiguousarray(w_hh.transpose(0, 2, 1)))
    _lib.call("qpg_gen_gru_layer_backward_f32", DEV, dev(dout) if isinstance(dout, np.ndarray) else dout, sv, out, whhT, B, T, H,
              dxp, dgh)
    g1.assert_tail_intact("dxp")
    g2.assert_tail_intact("dgh")
    return dxp, dgh


def gru_ref(xp, w_hh, b_hh, dout, dtype):
    """out, saved, dxp, dgh by torch autograd with the projection xp as the leaf."""
    td = TD[dtype]
    xpt = torch.from_numpy(xp.astype(dtype)).requires_grad_(True)
    wt, bt = torch.from_numpy(w_hh.astype(dtype)), torch.from_numpy(b_hh.astype(dtype))
    B, T = xp.shape[:2]
    outs, ghs, saved = [], {}, np.zeros((B, T, 2, 4, H), dtype)
    for d in (0, 1):
        h = torch.zeros((B, H), dtype=td)
        o = [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            probe = torch.zeros((B, 3 * H), dtype=td, requires_grad=True)    # its gradient is the one at W_hh h + b_hh
            gh = F.linear(h, wt[d], bt[d]) + probe
            ghs[(d, t)] = probe
            r = torch.sigmoid(xpt[:, t, d, :H] + gh[:, :H])
            z = torch.sigmoid(xpt[:, t, d, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(xpt[:, t, d, 2 * H:] + r * gh[:, 2 * H:])
            h = (1.0 - z) * n + z * h
            o[t] = h
            for i, v in enumerate((r, z, n, gh[:, 2 * H:])):
                saved[:, t, d, i] = v.detach().numpy()
        outs.append(torch.stack(o, 1))
    out = torch.cat(outs, -1)
    out.backward(torch.from_numpy(dout.astype(dtype)))
    dgh = np.zeros((B, T, 2, 3 * H), dtype)
    for (d, t), gh in ghs.items():
        dgh[:, t, d] = gh.grad.numpy()
    return out.detach().numpy(), saved, xpt.grad.numpy(), dgh


@pytest.mark.parametrize("T", [1, 2, 31])
def test_gru_training_forward_and_backward(T):
    w_hh, b_hh = gru_weights(600 + T)
    rng = rng_of(700 + T)
    Bmax = GBT + 1
    xp = (rng.standard_normal((Bmax, T, 2, 3 * H)) * 1.5).astype(np.float32)
    dout = rng.standard_normal((Bmax, T, 2 * H)).astype(np.float32)
    # forward: out bit-equal to the inference kernel's, the saved planes against f64
    out, sv = gru_train_device(xp, w_hh, b_hh)
    plain = torch.empty((Bmax, T, 2 * H), dtype=torch.float32, device=DEV)
    _lib.call("qpg_gen_gru_layer_f32", DEV, dev(xp), dev(w_hh), dev(b_hh), Bmax, T, H, plain)
    assert torch.equal(out, plain)
    r64, r32 = gru_ref(xp, w_hh, b_hh, dout, np.float64), gru_ref(xp, w_hh, b_hh, dout, np.float32)
    check("gru train T %d saved" % T, sv, r64[1], r32[1])
    full = gru_backward_device(dout, sv, out, w_hh)
    check("gru backward T %d dxp" % T, full[0], r64[2], r32[2])
    check("gru backward T %d dgh" % T, full[1], r64[3], r32[3])
    # a sequence's bits depend neither on B nor on its position
    for sl in (slice(0, 1), slice(0, GBT), slice(GBT, Bmax), slice(3, 9)):
        o, s = gru_train_device(xp[sl], w_hh, b_hh)
        assert torch.equal(o, plain[sl])
        part = gru_backward_device(np.ascontiguousarray(dout[sl]), s, o, w_hh)
        assert torch.equal(part[0], full[0][sl]) and torch.equal(part[1], full[1][sl]), sl
    # direction symmetry: swapped weights on the time-flipped input give the flipped, swapped result
    xs = np.ascontiguousarray(xp[:, ::-1, ::-1])
    ds = np.ascontiguousarray(np.concatenate([dout[:, ::-1, H:], dout[:, ::-1, :H]], -1))
    ws_, bs_ = np.ascontiguousarray(w_hh[::-1]), np.ascontiguousarray(b_hh[::-1])
    o, s = gru_train_device(xs, ws_, bs_)
    sw = gru_backward_device(ds, s, o, ws_)
    assert torch.equal(sw[0], full[0].flip(1).flip(2)) and torch.equal(sw[1], full[1].flip(1).flip(2))


def test_gru_backward_saturated_gates_stay_finite():
    w_hh, b_hh = gru_weights(7)
    rng = rng_of(8)
    B, T = 5, 4
    xp = (rng.choice([-40.0, 40.0], (B, T, 2, 3 * H)) + rng.standard_normal((B, T, 2, 3 * H))).astype(np.float32)
    dout = rng.standard_normal((B, T, 2 * H)).astype(np.float32)
    out, sv = gru_train_device(xp, w_hh, b_hh)
    dxp, dgh = gru_backward_device(dout, sv, out, w_hh)
    assert torch.isfinite(dxp).all() and torch.isfinite(dgh).all() and torch.isfinite(sv).all()
    r64, r32 = gru_ref(xp, w_hh, b_hh, dout, np.float64), gru_ref(xp, w_hh, b_hh, dout, np.float32)
    check("gru backward saturated dxp", dxp, r64[2], r32[2])


def test_gru_training_refuses_other_widths():
    x = torch.zeros(1 << 14, device=DEV)
    with pytest.raises(_lib.Unsupported):
        _lib.call("qpg_gen_gru_layer_train_f32", DEV, x, x, x, 1, 1, 100, x, x)
    with pytest.raises(_lib.Unsupported):
        _lib.call("qpg_gen_gru_layer_backward_f32", DEV, x, x, x, x, 1, 1, 100, x, x)


# ---- the row-contraction weight gradient ----------------------------------------------------------------------------------
def rowgrad_np(dY, X, shift, T, dtype):
    dY, X = dY.astype(dtype), X.astype(dtype)
    if shift:
        Xs = np.zeros_like(X).reshape(-1, T, X.shape[1])
        X3 = X.reshape(-1, T, X.shape[1])
        if shift < 0:
            Xs[:, 1:] = X3[:, :-1]
        else:
            Xs[:, :-1] = X3[:, 1:]
        X = Xs.reshape(X.shape)
    return dY.T @ X, dY.sum(0, dtype=dtype)


@pytest.mark.parametrize("N,K,ldx", [(512, 208, 208), (1200, 32, 32), (1200, 400, 400), (600, 200, 400)])
def test_rowgrad_model_shapes_row_counts_and_slabs(N, K, ldx):
    rng = rng_of(N + K)
    lib = _lib.load()
    for R in (1, 15, 16, 17, 481):
        ldy = N if N != 600 else 1200
        dYf = rng.standard_normal((R, ldy)).astype(np.float32)
        Xf = rng.standard_normal((R, ldx)).astype(np.float32)
        off_y, off_x = (600, 200) if N == 600 else (0, 0)       # direction 1's half of the rows
        dY, X = dYf[:, off_y:off_y + N], Xf[:, off_x:off_x + K]
        n_ws = lib.qpg_gen_rowgrad_ws_floats(N, K, 4)
        ws, ws_guard = scratch(n_ws)
        dW, wg = out_of((N, K))
        db, bg = out_of((N,))
        _lib.call("qpg_gen_rowgrad_f32", DEV, dev(dYf).reshape(-1)[off_y:], ldy, dev(Xf).reshape(-1)[off_x:], ldx, R, N, K, 0, 1,
                  dW, db, ws, n_ws)
        r64, r32 = rowgrad_np(dY, X, 0, 1, np.float64), rowgrad_np(dY, X, 0, 1, np.float32)
        tag = "rowgrad N %d K %d R %d " % (N, K, R)
        check(tag + "dW", dW, r64[0], r32[0])
        check(tag + "db", db, r64[1], r32[1])
        for g in (ws_guard, wg, bg):
            g.assert_tail_intact(tag)
        # a single slab (the smallest workspace) gives the same within rounding, and two runs the same bits
        dW1, _ = out_of((N, K))
        _lib.call("qpg_gen_rowgrad_f32", DEV, dev(dYf).reshape(-1)[off_y:], ldy, dev(Xf).reshape(-1)[off_x:], ldx, R, N, K, 0, 1,
                  dW1, None, ws, N * K + N)
        check(tag + "dW, one slab", dW1, r64[0], r32[0])
        dW2, _ = out_of((N, K))
        _lib.call("qpg_gen_rowgrad_f32", DEV, dev(dYf).reshape(-1)[off_y:], ldy, dev(Xf).reshape(-1)[off_x:], ldx, R, N, K, 0, 1,
                  dW2, None, ws, n_ws)
        assert torch.equal(dW2, dW)


@pytest.mark.parametrize("T", [1, 2, 31])
@pytest.mark.parametrize("shift", [-1, 1])
def test_rowgrad_shift_never_reaches_across_a_batch_member(T, shift):
    rng = rng_of(900 + T + shift)
    B, N, K = 5, 600, 200
    R = B * T
    dY, X = rng.standard_normal((R, N)).astype(np.float32), rng.standard_normal((R, K)).astype(np.float32)
    n_ws = _lib.load().qpg_gen_rowgrad_ws_floats(N, K, 4)
    ws, ws_guard = scratch(n_ws)
    dW, wg = out_of((N, K))
    db, bg = out_of((N,))
    _lib.call("qpg_gen_rowgrad_f32", DEV, dev(dY), N, dev(X), K, R, N, K, shift, T, dW, db, ws, n_ws)
    r64, r32 = rowgrad_np(dY, X, shift, T, np.float64), rowgrad_np(dY, X, shift, T, np.float32)
    if T == 1:
        assert np.all(host(dW) == 0) and np.all(host(db) != 0)
    else:
        check("rowgrad shift %d T %d dW" % (shift, T), dW, r64[0], r32[0])
    check("rowgrad shift %d T %d db" % (shift, T), db, r64[1], r32[1])
    for g in (ws_guard, wg, bg):
        g.assert_tail_intact("rowgrad shift")


def test_rowgrad_refuses_what_it_is_not_built_for():
    x = torch.zeros(1 << 14, device=DEV)
    with pytest.raises(_lib.Unsupported):
        _lib.call("qpg_gen_rowgrad_f32", DEV, x, 5000, x, 16, 1, 5000, 16, 0, 1, x, None, x, 1 << 14)
    with pytest.raises(RuntimeError):
        _lib.call("qpg_gen_rowgrad_f32", DEV, x, 16, x, 16, 7, 16, 16, 1, 3, x, None, x, 1 << 14)      # R no multiple of T


# ---- head: LayerNorm backward, cross-entropy backward, dropout ------------------------------------------------------------
def ln_backward_ref(x, dy, gamma, beta, dtype):
    xt = torch.from_numpy(x.astype(dtype)).requires_grad_(True)
    g = torch.from_numpy(gamma.astype(dtype)).requires_grad_(True)
    b = torch.from_numpy(beta.astype(dtype)).requires_grad_(True)
    y = F.layer_norm(xt[:, :H] + xt[:, H:], (H,), g, b, 1e-5)
    y.backward(torch.from_numpy(dy[:, :H].astype(dtype)))
    return xt.grad.numpy(), g.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("R", [1, 3, 63, 64, 65, 257])
def test_head_layernorm_backward(R):
    rng = rng_of(1000 + R)
    x = rng.standard_normal((R, 2 * H)).astype(np.float32)
    dy = rng.standard_normal((R, G.HEAD_LD)).astype(np.float32)
    dy[:, H:] = np.nan                                           # the padding columns are ignored
    gamma, beta = rng.uniform(0.6, 1.4, H).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    n_ws = _lib.load().qpg_gen_head_ln_bwd_ws_floats(R)
    ws, ws_guard = scratch(n_ws)
    dx, xg = out_of((R, 2 * H))
    dgb, gg = out_of((2, H))
    _lib.call("qpg_gen_head_ln_backward_f32", DEV, dev(dy), dev(x), dev(gamma), R, H, 1e-5, ws, n_ws, dgb[0], dgb[1], dx)
    r64, r32 = ln_backward_ref(x, dy, gamma, beta, np.float64), ln_backward_ref(x, dy, gamma, beta, np.float32)
    check("ln backward R %d dx" % R, dx, r64[0], r32[0])
    check("ln backward R %d dgamma" % R, dgb[0], r64[1], r32[1])
    check("ln backward R %d dbeta" % R, dgb[1], r64[2], r32[2])
    assert torch.equal(dx[:, :H], dx[:, H:])
    for g in (ws_guard, xg, gg):
        g.assert_tail_intact("ln backward")
    with pytest.raises(_lib.Unsupported):
        _lib.call("qpg_gen_head_ln_backward_f32", DEV, dev(dy), dev(x), dev(gamma), R, 100, 1e-5, ws, n_ws, dgb[0], dgb[1], dx)


@pytest.mark.parametrize("R", [1, 4, 5, 61])
def test_cross_entropy_backward(R):
    rng = rng_of(1100 + R)
    logits = (rng.standard_normal((R, 512)) * 3.0).astype(np.float32)
    target = rng.integers(0, 512, R)
    target[0], target[-1] = 0, 511
    dl, g = out_of((R, 512))
    _lib.call("qpg_gen_cross_entropy_backward_f32", DEV, dev(logits), dev(target, np.int64), R, 512, dl)
    refs = {}
    for dt in (np.float64, np.float32):
        lt = torch.from_numpy(logits.astype(dt)).requires_grad_(True)
        F.cross_entropy(lt, torch.from_numpy(target)).backward()
        refs[dt] = lt.grad.numpy()
    check("cross-entropy backward R %d" % R, dl, refs[np.float64], refs[np.float32])
    rows = host(dl).astype(np.float64).sum(1)
    assert np.abs(rows).max() <= 512 * 2.0 ** -23 / R, rows     # (softmax - onehot) sums to 0 within f32 rounding of its terms
    g.assert_tail_intact("dlogits")


def test_dropout_masks():
    rng = rng_of(1200)
    n = 1000
    x = rng.standard_normal(n).astype(np.float32)
    scale = np.float32(1.0 / 0.9)
    for name, mask in (("ones", np.ones(n, np.uint8)), ("zeros", np.zeros(n, np.uint8)), ("mixed", (rng.random(n) >= 0.1).astype(np.uint8))):
        y, g = out_of((n,))
        _lib.call("qpg_gen_dropout_f32", DEV, dev(x), dev(mask, np.uint8), n, float(scale), y)
        assert np.array_equal(host(y), np.where(mask != 0, x * scale, np.float32(0.0))), name
        g.assert_tail_intact("dropout")
