"""The entry points of qpg_wavvq.hip alone against NumPy f64, at the smallest shapes where they can go wrong:
qpg_wavvq_groupnorm_f32 (+ its workspace query), qpg_wavvq_relu_f32, qpg_wavvq_group_argmax_f32.

GroupNorm tolerance, from the arithmetic and not from the kernel's output: the statistics are f64 sums, so mean and rstd
reach the apply pass as correctly rounded f32 values; v - mean carries mean's rounding |mean| 2^-24 and its own, and the
three operations behind it (times rstd, times gamma, plus beta) and rstd's rounding one each, relative to a magnitude of
at most Y = max |xhat gamma| + max |beta|; the ReLU is exact and log(|v| + 1) (one addition, a logf of <= 2 ulp, slope
<= 1) adds three more.  TOL = 2^-24 (8 Y + |mean| rstd max |gamma|).  Each check prints its measured error first."""
import numpy as np
import pytest
import torch

from qpgesture_amd import _lib
from tests import poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
SLAB = _lib.CONSTANTS.get("QPG_WAVVQ_GN_SLAB", 4096)
U = 2.0 ** -24


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def ws_floats(B, T, C):
    return int(_lib.load().qpg_wavvq_groupnorm_ws_floats(B, T, C))


def gn_ref(x, g, b, epi):
    """(f64 result, tolerance per window) of GroupNorm(1, C) over x (B, T, C) f32."""
    x = x.astype(np.float64)
    mean = x.mean(axis=(1, 2), keepdims=True)
    var = ((x - mean) ** 2).mean(axis=(1, 2), keepdims=True)
    rstd = 1.0 / np.sqrt(var + EPS)
    y = (x - mean) * rstd * g.astype(np.float64) + b.astype(np.float64)
    Y = np.abs((x - mean) * rstd * g).max(axis=(1, 2)) + np.abs(b).max()
    tol = U * (8 * Y + np.abs(mean[:, 0, 0]) * rstd[:, 0, 0] * np.abs(g).max())
    if epi >= 1:
        y = np.maximum(y, 0.0)
    if epi == 2:
        y = np.log(np.abs(y) + 1.0)
    return y, tol


def gn_run(x, g, b, epi, ws=None, n_ws=None):
    B, T, C = x.shape
    xd = torch.from_numpy(x).to(DEV).contiguous()
    gd = None if g is None else torch.from_numpy(g).to(DEV)
    bd = None if b is None else torch.from_numpy(b).to(DEV)
    if ws is None:
        ws = torch.zeros(ws_floats(B, T, C), dtype=torch.float32, device=DEV)
    _lib.call("qpg_wavvq_groupnorm_f32", DEV, xd, B, T, C, gd, bd, EPS, epi, ws, ws.numel() if n_ws is None else n_ws)
    return xd


def affine(C, seed):
    r = rng(seed)
    g = (r.uniform(0.6, 1.4, C) * np.where(np.arange(C) % 3 == 1, -1.0, 1.0)).astype(np.float32)      # a third negative
    return g, (r.standard_normal(C) * 0.3).astype(np.float32)


def check(name, got, x, g, b, epi):
    want, tol = gn_ref(x, g, b, epi)
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), name
    err = np.abs(got - want).max(axis=(1, 2))
    print("%s: err %s tol %s ratio %.2f" % (name, err, tol, float((err / tol).max())))
    assert (err <= tol).all(), (name, err, tol)


# T C below one slab, exactly one, one plus a row, a single frame; rows that straddle slab ends (C = 20); the real width
SHAPES = [(1, 100, 16), (3, 100, 16), (1, SLAB // 16, 16), (3, SLAB // 16, 16), (1, SLAB // 16 + 1, 16),
          (3, SLAB // 16 + 1, 16), (1, 1, 16), (3, 1, 16), (2, 1000, 20), (2, SLAB // 512 + 1, 512), (1, 2 * SLAB // 4 + 3, 4)]


@pytest.mark.parametrize("B,T,C", SHAPES)
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_groupnorm_against_f64(B, T, C, epi):
    x = (rng(B * 1000 + T + C).standard_normal((B, T, C)) * 1.7 + 0.4).astype(np.float32)
    g, b = affine(C, 7)
    assert ws_floats(B, T, C) == B * (-(-T * C // SLAB)) * 4 + 2 * B
    check("gn B%d T%d C%d epi%d" % (B, T, C, epi), gn_run(x, g, b, epi), x, g, b, epi)


@pytest.mark.parametrize("epi", [0, 1, 2])
def test_groupnorm_silence_gives_beta(epi):
    """An all-zero window: variance 0, xhat 0, the output is beta (then the epilogue) exactly; its neighbour is untouched by it."""
    B, T, C = 2, SLAB // 16 + 5, 16
    x = rng(3).standard_normal((B, T, C)).astype(np.float32)
    x[0] = 0.0
    g, b = affine(C, 8)
    got = gn_run(x, g, b, epi)
    want = b.copy()
    if epi >= 1:
        want = np.maximum(want, np.float32(0))
    if epi == 2:
        want64 = np.log(np.abs(want.astype(np.float64)) + 1.0)
        # (|v| + 1 rounds once, slope <= 1 behind it; logf within 2 ulp of a result below max(1, .))
        assert np.abs(got[0].cpu().numpy() - want64).max() <= 3 * U * max(1.0, float(want64.max()))
    else:
        assert np.array_equal(got[0].cpu().numpy(), np.broadcast_to(want, (T, C)))
    assert torch.equal(got[0], got[0, :1].expand(T, C))
    check("silence neighbour", got[1:], x[1:], g, b, epi)


def test_groupnorm_dc_offset_100_sigma():
    """A window whose mean is 100 times its standard deviation: sums of squares in f32 would lose the variance."""
    B, T, C = 2, 700, 16
    x = (100.0 + rng(4).standard_normal((B, T, C))).astype(np.float32)
    x[1] = (-250.0 + 2.5 * rng(5).standard_normal((T, C))).astype(np.float32)
    g, b = affine(C, 9)
    for epi in (0, 2):
        check("dc offset epi%d" % epi, gn_run(x, g, b, epi), x, g, b, epi)


def test_groupnorm_without_affine():
    x = rng(6).standard_normal((2, 300, 16)).astype(np.float32)
    one, zero = np.ones(16, np.float32), np.zeros(16, np.float32)
    got = gn_run(x, None, None, 1)
    check("non-affine", got, x, one, zero, 1)
    assert torch.equal(got, gn_run(x, one, zero, 1))


@pytest.mark.parametrize("T", [100, SLAB // 16 + 1, 1000])
def test_window_bits_do_not_depend_on_the_batch(T):
    C = 16
    x = rng(T).standard_normal((3, T, C)).astype(np.float32)
    x[1] += 3.0
    g, b = affine(C, 10)
    whole = gn_run(x, g, b, 2)
    for i in range(3):
        assert torch.equal(gn_run(x[i:i + 1].copy(), g, b, 2)[0], whole[i]), i
    assert torch.equal(gn_run(x[::-1].copy(), g, b, 2), whole.flip(0))


def test_groupnorm_workspace_one_short_and_refusals():
    B, T, C = 3, SLAB // 16 + 1, 16
    x = rng(11).standard_normal((B, T, C)).astype(np.float32)
    g, b = affine(C, 11)
    need = ws_floats(B, T, C)
    ws = torch.zeros(need, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="ws holds") as e:
        out = gn_run(x, g, b, 1, ws=ws, n_ws=need - 1)
    assert not isinstance(e.value, _lib.Unsupported)
    xd = torch.from_numpy(x).to(DEV)
    before = xd.clone()
    with pytest.raises(RuntimeError):
        _lib.call("qpg_wavvq_groupnorm_f32", DEV, xd, B, T, C, torch.from_numpy(g).to(DEV), torch.from_numpy(b).to(DEV), EPS, 1,
                  ws, need - 1)
    assert torch.equal(xd, before) and not ws.any()                      # nothing was launched
    out = gn_run(x, g, b, 1, ws=ws, n_ws=need)                           # exactly enough
    check("ws exact", out, x, g, b, 1)
    x6 = torch.zeros((1, 8, 6), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.Unsupported, match="multiple of 4"):
        _lib.call("qpg_wavvq_groupnorm_f32", DEV, x6, 1, 8, 6, None, None, EPS, 0, ws, need)
    with pytest.raises(RuntimeError, match="epilogue"):
        _lib.call("qpg_wavvq_groupnorm_f32", DEV, xd, B, T, C, None, None, EPS, 3, ws, need)
    assert torch.equal(xd, before)
    assert ws_floats(0, 5, 16) == 0 and ws_floats(1, 0, 16) == 0 and ws_floats(70000, 5, 16) == 0


@pytest.mark.parametrize("fill", sorted(poison.FILLS))
def test_groupnorm_ignores_what_the_workspace_held(fill):
    B, T, C = 3, 2 * SLAB // 16 + 7, 16
    x = rng(12).standard_normal((B, T, C)).astype(np.float32)
    g, b = affine(C, 12)
    clean = gn_run(x, g, b, 2)
    need = ws_floats(B, T, C)
    guard = poison.guarded(need * 4, poison.FILLS[fill], device=DEV)
    got = gn_run(x, g, b, 2, ws=guard.view(torch.float32))
    assert torch.equal(got, clean)
    guard.assert_tail_intact("groupnorm workspace")


def test_relu():
    x = rng(13).standard_normal(4 * 1000 + 4).astype(np.float32)
    x[:4] = [-0.0, 0.0, -1e-30, 1e-30]
    xd = torch.from_numpy(x).to(DEV)
    _lib.call("qpg_wavvq_relu_f32", DEV, xd, x.size)
    assert np.array_equal(xd.cpu().numpy(), np.maximum(x, np.float32(0)))
    with pytest.raises(_lib.Unsupported, match="multiple of 4"):
        _lib.call("qpg_wavvq_relu_f32", DEV, xd, 6)
    _lib.call("qpg_wavvq_relu_f32", DEV, xd, 0)


def argmax(logits):
    R, G, V = logits.shape
    ld = torch.from_numpy(logits).to(DEV)
    codes = torch.full((R, G), -7, dtype=torch.int64, device=DEV)
    _lib.call("qpg_wavvq_group_argmax_f32", DEV, ld, R, G, V, codes)
    return codes.cpu().numpy()


@pytest.mark.parametrize("G,V", [(2, 320), (2, 20), (3, 7), (1, 65), (2, 64)])
def test_group_argmax(G, V):
    R = 9
    logits = rng(G * 100 + V).standard_normal((R, G, V)).astype(np.float32)
    logits[0] = 0.25                                           # a row of equal values: 0 in every group
    logits[1, :, 0] = logits[1, :, V - 1] = 9.0                # a tie between the first and the last index: the first
    logits[2, G - 1, V - 1] = 11.0                             # the maximum at the last index of the last group
    logits[3, 0, V // 2] = logits[3, 0, V // 2 + 1] = 8.0      # neighbours tie: the lower
    logits[4] = -np.inf                                        # equal again
    got = argmax(logits)
    want = np.argmax(logits.astype(np.float64), axis=-1)       # (NumPy: the first maximum, as torch.max)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert not got[0].any() and not got[1].any() and got[2, G - 1] == V - 1 and got[3, 0] == V // 2 and not got[4].any()
