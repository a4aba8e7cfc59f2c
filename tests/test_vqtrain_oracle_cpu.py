"""The comparison helpers of tests/test_gpu_vqtrain_kernels.py must be able to fail (CPU only).

A float32 computation of a layer's gradients (torch autograd on the CPU) stands in for the kernel: it must pass the
bound of oracle/vqtrain_oracle.py against the float64 reference, and the same bound, at the same shape and gamma,
must reject a reference that is wrong in the ways a kernel goes wrong - a position row missing from the contraction,
a tap reading the wrong position, a 128-channel output tile left at zero, the bias added twice."""
import numpy as np
import pytest
import torch

from oracle import vqtrain_oracle as VT


def _f32_grads(kind, x, dy, ws, bs, dil=1):
    xt = x.permute(0, 2, 1).contiguous().requires_grad_(True)
    wt = [w.clone().requires_grad_(True) for w in ws]
    bt = [b.clone().requires_grad_(True) for b in bs]
    y = VT._layer(kind, xt, wt, bt, dil, True)
    r = torch.autograd.grad(y, [xt] + wt + bt, dy.permute(0, 2, 1))
    return dict(dx=r[0].permute(0, 2, 1), dw=list(r[1:1 + len(ws)]), db=list(r[1 + len(ws):]))


@pytest.mark.parametrize("B,T", [(8, 60), (256, 30)])
def test_conv_bound_accepts_f32_and_rejects_wrong_references(B, T):
    g = torch.Generator().manual_seed(11)
    C = 512
    x = torch.randn(B, T, C, generator=g)
    dy = torch.randn(B, T, C, generator=g)
    w = torch.randn(C, C, 3, generator=g) / np.sqrt(3 * C)
    b = torch.randn(C, generator=g) * 0.05
    ref, absref = VT.layer_grads("conv3", x, dy, [w], [b])
    got = _f32_grads("conv3", x, dy, [w], [b])
    M = B * T
    g_w = VT.gamma(M, 32)                   # positions, then up to 32 split partials
    g_x = VT.gamma(3 * C, 8)                # taps x channels, then up to 8 split-K partials

    def ratios(r):
        return (VT.bound_ratio(got["dw"][0], r["dw"][0], absref["dw"][0], g_w),
                VT.bound_ratio(got["db"][0], r["db"][0], absref["db"][0], g_w),
                VT.bound_ratio(got["dx"], r["dx"], absref["dx"], g_x))
    ok = ratios(ref)
    assert max(ok) <= 1.0, ok

    # one position row dropped from the contraction
    dy_drop = dy.clone()
    dy_drop[B // 2, T // 3] = 0
    r_drop, _ = VT.layer_grads("conv3", x, dy_drop, [w], [b])
    rw, rb, rx = ratios(r_drop)
    assert rw > 1.0 and rb > 1.0 and rx > 1.0, (rw, rb, rx)

    # tap 0 shifted by one position: it reads the position tap 1 reads
    r_shift = dict(ref, dw=[ref["dw"][0].clone()])
    r_shift["dw"][0][:, :, 0] = ref["dw"][0][:, :, 1]
    w_shift = torch.stack((torch.zeros_like(w[:, :, 0]), w[:, :, 0] + w[:, :, 1], w[:, :, 2]), dim=2)
    r_shift["dx"] = VT.layer_grads("conv3", x, dy, [w_shift], [b])[0]["dx"]
    rw, _, rx = ratios(r_shift)
    assert rw > 1.0 and rx > 1.0, (rw, rx)

    # one 128-channel output tile zeroed (weight gradient: output channels; data gradient: input channels)
    r_tile = dict(ref, dw=[ref["dw"][0].clone()], dx=ref["dx"].clone())
    r_tile["dw"][0][128:256] = 0
    r_tile["dx"][..., 256:384] = 0
    rw, _, rx = ratios(r_tile)
    assert rw > 1.0 and rx > 1.0, (rw, rx)

    # the bias accumulated twice
    r_bias = dict(ref, db=[2 * ref["db"][0]])
    assert ratios(r_bias)[1] > 1.0


def test_weight_bound_at_the_largest_production_M():
    """The weight-gradient bound is widest where the position contraction is longest: M = 256 x 240 = 61 440 (gamma
    grows like sqrt(M)).  There, at the same gamma the GPU test uses (M positions, up to 64 split partials), the f32
    gradients pass and dW still rejects a dropped position row, a shifted tap and a zeroed 128-channel tile; db rejects
    the doubled bias.  db alone would not see the dropped row: its bound, gamma * sum|dy| ~ 6e-5 x 0.8 M ~ 3 for unit
    dy, is about one entry of dy.  The kernel computes db in the same launch from the same staged rows as dW, so a row
    the launch loses shows in dW.  (Entries of dW and db depend on the channel counts only through how many there are:
    narrow layers, 64 -> 256, keep the float64 reference cheap.)"""
    g = torch.Generator().manual_seed(16)
    B, T, Ci, Co = 256, 240, 64, 256
    x = torch.randn(B, T, Ci, generator=g)
    dy = torch.randn(B, T, Co, generator=g)
    w = torch.randn(Co, Ci, 3, generator=g) / np.sqrt(3 * Ci)
    b = torch.randn(Co, generator=g) * 0.05
    ref, absref = VT.layer_grads("conv3", x, dy, [w], [b])
    got = _f32_grads("conv3", x, dy, [w], [b])
    gw = VT.gamma(B * T, 64)

    def rw(r):
        return VT.bound_ratio(got["dw"][0], r, absref["dw"][0], gw)
    assert rw(ref["dw"][0]) <= 1.0
    assert VT.bound_ratio(got["db"][0], ref["db"][0], absref["db"][0], gw) <= 1.0
    dy_drop = dy.clone()
    dy_drop[100, 77] = 0
    assert rw(VT.layer_grads("conv3", x, dy_drop, [w], [b])[0]["dw"][0]) > 1.0
    shifted = ref["dw"][0].clone()
    shifted[:, :, 0] = ref["dw"][0][:, :, 1]
    assert rw(shifted) > 1.0
    tile = ref["dw"][0].clone()
    tile[128:256] = 0
    assert rw(tile) > 1.0
    assert VT.bound_ratio(got["db"][0], 2 * ref["db"][0], absref["db"][0], gw) > 1.0


def test_residual_block_bound_accepts_f32_and_rejects_a_dropped_row():
    g = torch.Generator().manual_seed(12)
    B, T, C, dil = 16, 30, 512, 3
    x = torch.randn(B, T, C, generator=g)
    dy = torch.randn(B, T, C, generator=g)
    w3 = torch.randn(C, C, 3, generator=g) * 1.4 / np.sqrt(3 * C)
    w1 = torch.randn(C, C, 1, generator=g) * 0.5 / np.sqrt(C)
    b3, b1 = torch.randn(C, generator=g) * 0.05, torch.randn(C, generator=g) * 0.05
    ref, absref = VT.layer_grads("res", x, dy, [w3, w1], [b3, b1], dil)
    got = _f32_grads("res", x, dy, [w3, w1], [b3, b1], dil)
    M = B * T
    g_w1, g_w3, g_x = VT.gamma(M, 32), VT.gamma(C, M, 32), VT.gamma(C, 3 * C, 8)
    assert VT.bound_ratio(got["dw"][1], ref["dw"][1], absref["dw"][1], g_w1) <= 1.0
    assert VT.bound_ratio(got["dw"][0], ref["dw"][0], absref["dw"][0], g_w3) <= 1.0
    assert VT.bound_ratio(got["db"][0], ref["db"][0], absref["db"][0], g_w3) <= 1.0
    assert VT.bound_ratio(got["dx"], ref["dx"], absref["dx"], g_x) <= 1.0
    dy_drop = dy.clone()
    dy_drop[3, 7] = 0
    r_drop, _ = VT.layer_grads("res", x, dy_drop, [w3, w1], [b3, b1], dil)
    assert VT.bound_ratio(got["dw"][1], r_drop["dw"][1], absref["dw"][1], g_w1) > 1.0
    assert VT.bound_ratio(got["dw"][0], r_drop["dw"][0], absref["dw"][0], g_w3) > 1.0


def test_code_sums_bound_accepts_chunked_f32_and_rejects_a_dropped_row():
    rng = np.random.Generator(np.random.PCG64(13))
    R, E, K = 7680, 64, 512
    z = rng.standard_normal((R, E)).astype(np.float32)
    ids = rng.integers(0, K, R)
    got = VT.code_sums_chunked_f32(z, ids, K)
    ref, cnt, ab = VT.code_sums_ref(z, ids, K)
    bound = VT.code_sums_bound(cnt, ab, ref)
    assert np.all(np.abs(got - ref) <= bound)
    keep = np.ones(R, bool)
    keep[4321] = False
    ref2, cnt2, ab2 = VT.code_sums_ref(z[keep], ids[keep], K)
    assert not np.all(np.abs(got - ref2) <= VT.code_sums_bound(cnt2, ab2, ref2))
    assert not np.array_equal(cnt2, np.bincount(ids, minlength=K))


def test_code_sums_chunked_order_is_not_the_plain_ascending_sum():
    """The chunk-ordered f32 restatement differs from a single ascending pass somewhere once a code spans chunks
    (the partials are rounded per chunk): the contract text must not promise the latter."""
    rng = np.random.Generator(np.random.PCG64(14))
    R, E, K = 3 * 1024 + 5, 256, 4
    z = (rng.standard_normal((R, E)) * np.exp(rng.standard_normal((R, 1)))).astype(np.float32)
    ids = rng.integers(0, K, R)
    chunked = VT.code_sums_chunked_f32(z, ids, K)
    plain = VT.code_sums_chunked_f32(z, ids, K, chunk=R)
    assert not np.array_equal(chunked, plain)


def test_adam_f64_step_matches_torch_adam_first_step():
    """adam_step_f64 is torch.optim.Adam's update (no weight decay): one step from zero moments, in float64."""
    rng = np.random.Generator(np.random.PCG64(15))
    p0 = rng.standard_normal(1000)
    g = rng.standard_normal(1000)
    p = torch.tensor(p0, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.5, 0.999), eps=1e-8)
    for step in (1, 2):
        p.grad = torch.tensor(g * step)
        opt.step()
    ours, m, v = VT.adam_step_f64(p0, g, np.zeros(1000), np.zeros(1000), 1e-3, 0.5, 0.999, 1e-8, 1)
    ours, m, v = VT.adam_step_f64(ours, 2 * g, m, v, 1e-3, 0.5, 0.999, 1e-8, 2)
    np.testing.assert_allclose(ours, p.detach().numpy(), rtol=0, atol=1e-15)
