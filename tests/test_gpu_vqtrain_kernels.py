"""The VQ-VAE training-step kernels against float64 references computed on the host, at the production shapes of
configs/codebook.yml (batch 256, width / emb_width / l_bins 512, 240-frame windows: 7 680 latent rows, up to 61 440
positions per convolution) and at the edges where the kernels change path.

Convolutions: every kind of operation VQVAE._bwd_tape performs, through the model's own _wgrad / _dgrad with the
tape's arguments, against autograd in f64 of F.conv1d / F.conv_transpose1d / the residual block, fed the weights
VQVAE.state_dict() exports.  Each entry is held to gamma * (|x| * |dy|) (oracle/vqtrain_oracle.py: gamma from the
lengths of the f32 accumulation chains, the contraction taken on absolute values); the largest err / bound of each
kernel is printed at the end of the module (run with -s to see it).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RATIOS = {}          # kernel -> largest err / bound seen
HITS = {"big": set(), "small": set(), "S": set()}


def _note(kernel, r):
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def _report():
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    yield
    print("\nlargest err / bound per kernel: " + ", ".join("%s %.3g" % kv for kv in sorted(RATIOS.items())))
    print("bwd_data tiles hit: big %s, small %s; bwd_weight splits S: %s"
          % (sorted(HITS["big"]), sorted(HITS["small"]), sorted(HITS["S"])))


@pytest.fixture(scope="module")
def model():
    import os
    import torch
    from qpgesture_amd import synth
    from qpgesture_amd.checkpoint import load_config
    from qpgesture_amd.vqvae import VQVAE
    cfg = load_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpgesture_amd",
                                   "configs", "codebook.yml"))
    hps = dict(cfg["VQVAE"])
    assert hps["width"] == hps["emb_width"] == hps["l_bins"] == 512 and cfg["batch_size"] == 256
    m = VQVAE(hps, 135, device="cuda:0").load_state_dict(synth.make_vqvae_state_dict(21))
    m.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    m.sd = m.state_dict()
    return m


# ----------------------------------------------------------------------------------------------------------------
# 1. convolution backward, operation by operation
# ----------------------------------------------------------------------------------------------------------------
ENC = "encoders.0.level_blocks.0.model"
DEC = "decoders.0.level_blocks.0.model"


def _big_tiles(m, M, fwd_cin_pad):
    """conv_launch's rule (csrc/qpg_vqvae.hip) for a backward-data launch: its output channels are the forward layer's
    input channels, padded to 128."""
    cout_pad = (fwd_cin_pad + 127) // 128 * 128
    return M * (cout_pad // 128) >= 128 * 2 * m.n_cu


def _splits(m, c, M, ws_floats):
    """qpg_conv1d_bwd_weight_f32's split count."""
    tiles = c.taps * ((c.cin_pad + 127) // 128) * (c.cout_pad // 128)
    S = max(1, 4 * m.n_cu // tiles)
    S = min(S, (M + 63) // 64)
    return min(S, ws_floats // (c.taps * c.cin_pad * c.cout_pad + c.cout_pad))


def _buf(shape, misalign=False):
    """Device tensor of `shape`; misalign: a view one float into a larger buffer (4-byte aligned, not 16)."""
    import torch
    n = int(np.prod(shape))
    b = torch.empty((n + 1 if misalign else n,), dtype=torch.float32, device="cuda:0")
    return (b[1:] if misalign else b).view(*shape)


def _dev(t, misalign=False):
    d = _buf(tuple(t.shape), misalign)
    d.copy_(t)
    return d


def _wgrad(m, c, x, dy, B, T_in, T_out, ws=None, **kw):
    """VQVAE._wgrad, optionally with an explicit workspace (its size caps the split count).  Returns the split count S
    the kernel RAN, read from the workspace: it is filled with NaN first, and split s writes its whole partial tile
    ws[s n_w : (s + 1) n_w) (the bias partials follow at S n_w, far short of the next tile's last entry), so S is the
    number of partial tiles whose last entry is no longer NaN.  It must equal what _splits predicts."""
    import torch
    from qpgesture_amd import _lib
    if ws is None:
        ws = m._wgrad_ws()
    n_w = c.taps * c.cin_pad * c.cout_pad
    cap = ws.numel() // n_w
    assert cap * c.cout_pad < n_w
    ws.fill_(float("nan"))
    _lib.call("qpg_conv1d_bwd_weight_f32", m.device, x, B, T_in, c.cin, dy, c.taps, c.cin_pad, c.cout, c.cout_pad,
              kw.get("in_stride", 1), kw.get("in_offset", 0), kw.get("dil", 1), T_out, kw.get("out_stride", 1),
              kw.get("out_offset", 0), kw.get("T_y", T_out), int(kw.get("relu_in", False)), c.dw, c.db,
              int(kw.get("acc_bias", False)), ws, ws.numel())
    S = int((~torch.isnan(ws[n_w - 1::n_w][:cap])).sum())
    assert S == _splits(m, c, B * T_out, ws.numel()), (S, _splits(m, c, B * T_out, ws.numel()))
    HITS["S"].add(S)
    return S


def _dgrad(m, c, dy, B, T_in, T_out, *a, **kw):
    M = B * T_out
    HITS["big" if _big_tiles(m, M, c.cin_pad) else "small"].add(M)
    return m._dgrad(c, dy, B, T_in, T_out, *a, **kw)


def _grads_of(m, names):
    g = m.named_gradients()
    return [g[n + ".weight"] for n in names], [g[n + ".bias"] for n in names]


def _check(kernel, what, got, ref, absref, g):
    from oracle import vqtrain_oracle as VT
    r = VT.bound_ratio(got, ref, absref, g)
    _note(kernel, r)
    assert r <= 1.0, "%s: %s err / bound = %.3g (gamma %.3g)" % (kernel, what, r, g)
    return r


def _rand(g, *shape, scale=1.0):
    import torch
    return torch.randn(*shape, generator=g) * scale


def _ops(m):
    """name -> (kind, convs, names, dil): one entry per operation kind of the tape."""
    return {
        "enc_out": ("conv3", [m.enc_out], ["%s.3" % ENC], 1),
        "dec_in": ("conv3", [m.dec_in], [DEC + ".0"], 1),
        "dec_out": ("conv3", [m.dec_out], ["decoders.0.out"], 1),
        "down0": ("down", [m.enc_down[0][0]], ["%s.0.0" % ENC], 1),
        "down1": ("down", [m.enc_down[1][0]], ["%s.1.0" % ENC], 1),
        "res_d1": ("res", list(m.dec_up[2][0][2]), ["%s.3.0.model.2.model.%d" % (DEC, j) for j in (1, 3)], 1),
        "res_d3": ("res", list(m.enc_down[1][1][1]), ["%s.1.1.model.1.model.%d" % (ENC, j) for j in (1, 3)], 3),
        "res_d9": ("res", list(m.enc_down[0][1][2]), ["%s.0.1.model.2.model.%d" % (ENC, j) for j in (1, 3)], 9),
        "up2": ("up", [m.dec_up[2][1], m.dec_up[2][2]], ["%s.3.1" % DEC], 1),
        "up0": ("up", [m.dec_up[0][1], m.dec_up[0][2]], ["%s.1.1" % DEC], 1),
    }


def _run_op(m, op, B, T, seed, wgrad_ws=None, mis_x=False, mis_dy=False, mis_out=False):
    """One tape operation on the GPU exactly as VQVAE._bwd_tape issues it, and its f64 reference."""
    import torch
    import torch.nn.functional as F
    from oracle import vqtrain_oracle as VT
    kind, convs, names, dil = _ops(m)[op]
    g = torch.Generator().manual_seed(seed)
    c0 = convs[0]
    cin = c0.cin
    if kind == "up":
        T_out, cout = 2 * T, convs[0].cout
    elif kind == "down":
        T_out, cout = T // 2, c0.cout
    elif kind == "res":
        T_out, cout = T, convs[1].cout
    else:
        T_out, cout = T, c0.cout
    x = _rand(g, B, T, cin)
    dy = _rand(g, B, T_out, cout)
    ws = [m.sd[n + ".weight"] for n in names]
    bs = [m.sd[n + ".bias"] for n in names]
    if kind == "res":
        # the tape's h = relu(conv3(relu(x))), rounded to f32 as the forward stores it
        xc = x.double().permute(0, 2, 1)
        h = F.relu(F.conv1d(F.relu(xc), ws[0].double(), bs[0].double(), padding=dil, dilation=dil))
        h = h.permute(0, 2, 1).float().contiguous()
        del xc
    xd, dyd = _dev(x, mis_x), _dev(dy, mis_dy)
    S = []
    if kind == "conv3":
        c = c0
        S.append(_wgrad(m, c, xd, dyd, B, T, T, wgrad_ws, in_offset=-1))
        out = _buf((B, T, c.cin), mis_out) if mis_out else None
        dx = _dgrad(m, c, dyd, B, T, T, 3, 2, -1, in_offset=-1, out=out)
        chains_w, chains_x = [B * T], [3 * c.cout, 8]
    elif kind == "down":
        c, To = c0, T // 2
        S.append(_wgrad(m, c, xd, dyd, B, T, To, wgrad_ws, in_stride=2, in_offset=-1))
        dx = _buf((B, T, c.cin), mis_out)
        _dgrad(m, c, dyd, B, To, To, 2, 3, -2, in_offset=-1, out_stride=2, out_offset=0, T_y=T, out=dx)
        _dgrad(m, c, dyd, B, To, To, 2, 2, -2, in_offset=0, out_stride=2, out_offset=1, T_y=T, out=dx)
        chains_w, chains_x = [B * To], [2 * c.cout, 8]
    elif kind == "res":
        c3, c1 = convs
        hd = _dev(h)
        S.append(_wgrad(m, c1, hd, dyd, B, T, T, wgrad_ws))
        dh = _dgrad(m, c1, dyd, B, T, T, 1, 0, 1, gate=hd)
        S.append(_wgrad(m, c3, xd, dh, B, T, T, wgrad_ws, in_offset=-dil, dil=dil, relu_in=True))
        out = _buf((B, T, c3.cin), mis_out) if mis_out else None
        dx = _dgrad(m, c3, dh, B, T, T, 3, 2, -1, in_offset=-dil, dil=dil, gate=xd, residual=dyd, out=out)
        chains_w, chains_x = [B * T], [c1.cout, 8, 3 * c3.cout, 8]
    else:
        even, odd = convs
        S.append(_wgrad(m, even, xd, dyd, B, T, T, wgrad_ws, in_offset=-1, out_stride=2, out_offset=0, T_y=2 * T))
        S.append(_wgrad(m, odd, xd, dyd, B, T, T, wgrad_ws, in_offset=0, out_stride=2, out_offset=1, T_y=2 * T,
                        acc_bias=True))
        dx = _dgrad(m, even, dyd, B, 2 * T, T, 2, 1, -1, in_stride=2, in_offset=0, dil=2)
        # (the tape's aliasing: residual and out are the same tensor)
        dx = _dgrad(m, odd, dyd, B, 2 * T, T, 2, 1, -1, in_stride=2, in_offset=-1, dil=2, residual=dx, out=dx)
        chains_w, chains_x = [B * T, 2], [2 * even.cout, 8, 2 * odd.cout, 8]
    torch.cuda.synchronize()
    got_dx = dx.cpu()
    got_w, got_b = _grads_of(m, names)
    del xd, dyd, dx
    # (res: the reference's dW1 contracts the f64 h, the kernel the f32 copy - covered by the 2 u of gamma)
    ref, absref = VT.layer_grads(kind, x, dy, ws, bs, dil)
    Smax = max(S)
    gw = VT.gamma(*(chains_w + [Smax]))
    gx = VT.gamma(*chains_x)
    tag = "%s B=%d T=%d" % (op, B, T)
    if kind == "res":
        _check("bwd_weight", tag + " dW1", got_w[1], ref["dw"][1], absref["dw"][1], gw)
        _check("bwd_weight", tag + " db1", got_b[1], ref["db"][1], absref["db"][1], gw)
        g3 = VT.gamma(*(chains_w + [Smax, c1.cout, 8]))
        _check("bwd_weight", tag + " dW3", got_w[0], ref["dw"][0], absref["dw"][0], g3)
        _check("bwd_weight", tag + " db3", got_b[0], ref["db"][0], absref["db"][0], g3)
    else:
        _check("bwd_weight", tag + " dW", got_w[0], ref["dw"][0], absref["dw"][0], gw)
        _check("bwd_weight", tag + " db", got_b[0], ref["db"][0], absref["db"][0], gw)
    _check("bwd_data", tag + " dx", got_dx, ref["dx"], absref["dx"], gx)
    return S


# production shapes: batch 256 on the levels of a step (both sides of the big-tile rule for backward-data)
PROD = [("dec_out", 240), ("enc_out", 30), ("dec_in", 30), ("res_d1", 240), ("res_d3", 60), ("res_d9", 120),
        ("down0", 240), ("down1", 120), ("up2", 120), ("up0", 30)]


@pytest.mark.parametrize("op,T", PROD)
def test_conv_backward_batch256(model, op, T):
    import gc
    S = _run_op(model, op, 256, T, seed=100 + PROD.index((op, T)))
    assert max(S) > 1
    gc.collect()


def test_conv_backward_tiles_both_sides_of_the_big_tile_rule(model):
    """Backward-data on each side of conv_launch's 128-row tile rule, the threshold computed from this device's CU
    count: the smallest batch of 30-position sequences at or above it, and the largest below it (width 512)."""
    m = model
    m_big = 128 * 2 * m.n_cu // 4                  # M * (Cout_pad / 128) >= 256 n_cu, Cout_pad = 512
    b_big = -(-m_big // 30)
    b_small = (m_big - 1) // 30
    assert _big_tiles(m, b_big * 30, 512) and not _big_tiles(m, b_small * 30, 512)
    _run_op(m, "dec_in", b_big, 30, seed=14)
    _run_op(m, "dec_in", b_small, 30, seed=15)
    print("n_cu %d: backward-data at M = %d (128-row tiles) and M = %d (64-row tiles)"
          % (m.n_cu, b_big * 30, b_small * 30))


@pytest.mark.parametrize("op", ["enc_out", "down0", "up0", "res_d3"])
def test_conv_backward_tail_positions(model, op):
    """B * T_out not a multiple of 16: the weight gradient's last chunk and last split are short."""
    B, T = 37, 30 if op != "down0" else 62
    _run_op(model, op, B, T, seed=7)


def test_conv_backward_weight_split_counts(model):
    """The split counts the kernel ran (read from the workspace, see _wgrad): S = 1 with a workspace of exactly one
    partial; the n_cu-driven S = 4 n_cu / tiles (48 tiles for a 512 -> 512 k3 layer) at a batch long enough that the
    rows do not cap it; S capped by the rows (four 16-position chunks per split) at B = 5, T = 40.  (B = 37, T = 30 -
    the tail case - is row-capped too on 256 CUs: 18 < 21.)"""
    import torch
    m = model
    c = m.dec_in
    one = torch.empty((c.taps * c.cin_pad * c.cout_pad + c.cout_pad,), dtype=torch.float32, device="cuda:0")
    assert _run_op(m, "dec_in", 37, 30, seed=8, wgrad_ws=one) == [1]
    s_cu = 4 * m.n_cu // 48
    B = -(-64 * s_cu // 30)
    assert _run_op(m, "dec_in", B, 30, seed=8) == [s_cu] and s_cu > 1
    S = _run_op(m, "dec_in", 5, 40, seed=9)
    assert S == [(5 * 40 + 63) // 64] and S[0] < s_cu, S
    print("bwd_weight split counts run: 1, %d (n_cu-driven, B = %d), %d (row-capped); all cases: %s"
          % (s_cu, B, S[0], sorted(HITS["S"])))


@pytest.mark.parametrize("op", ["dec_in", "res_d1"])
def test_conv_backward_data_split_k(model, op):
    """A short sequence at width 512: backward-data splits its contraction over blockIdx.z (ks > 1)."""
    _run_op(model, op, 1, 30, seed=10)


@pytest.mark.parametrize("which", ["x", "dy", "out"])
def test_conv_backward_unaligned_operands(model, which):
    """Pointers one float off 16-byte alignment: wgrad VECX / VECY false with Cin = Cout = 512, backward-data's scalar
    activation loads (vec false) and scalar epilogue (vec_out false)."""
    _run_op(model, "enc_out", 7, 30, seed=11, mis_x=which == "x", mis_dy=which == "dy", mis_out=which == "out")
    _run_op(model, "res_d3", 7, 30, seed=12, mis_x=which == "x", mis_dy=which == "dy", mis_out=which == "out")


def test_conv_backward_dilation_beyond_the_sequence(model):
    """T = 8 < dilation 9: every tap but the centre reads padding."""
    _run_op(model, "res_d9", 3, 8, seed=13)


# ----------------------------------------------------------------------------------------------------------------
# 2. code sums
# ----------------------------------------------------------------------------------------------------------------
def _ids(pattern, R, K, rng):
    if pattern == "uniform":
        return rng.integers(0, K, R)
    if pattern == "popular":                     # one code holds 90 % of the rows, spread over every chunk
        ids = rng.integers(0, K, R)
        ids[rng.random(R) < 0.9] = 7
        return ids
    if pattern == "half_absent":
        return rng.integers(0, K // 2, R) * 2
    if pattern == "last_code":
        return np.full(R, K - 1)
    if pattern == "last_chunk":                  # code 5 only in the last (partial) chunk
        ids = rng.integers(0, K - 1, R)
        ids[ids >= 5] += 1
        ids[(R - 1) // 1024 * 1024:] = 5
        return ids
    raise ValueError(pattern)


CS_CASES = ([(R, E, "uniform") for R in (1, 1023, 1024, 1025, 7680, 3 * 1024 + 5) for E in (4, 64, 512, 1024)]
            + [(R, E, p) for R in (7680, 3 * 1024 + 5) for E in (64, 512)
               for p in ("popular", "half_absent", "last_code", "last_chunk")])


def _code_sums(z, ids, K, ws_bytes=None):
    import torch
    from qpgesture_amd import _lib
    R, E = z.shape
    lib = _lib.load()
    need = int(lib.qpg_vq_code_sums_ws_bytes(R, E, K))
    ws = torch.empty((max(need, 1) if ws_bytes is None else ws_bytes,), dtype=torch.uint8, device="cuda:0")
    bsum = torch.empty((K, E), dtype=torch.float32, device="cuda:0")
    belem = torch.empty((K,), dtype=torch.float32, device="cuda:0")
    _lib.call("qpg_vq_code_sums_f32", "cuda:0", z, ids, R, E, K, bsum, belem, ws, ws.numel())
    return bsum, belem


@pytest.mark.parametrize("R,E,pattern", CS_CASES)
def test_code_sums(R, E, pattern):
    import torch
    from oracle import vqtrain_oracle as VT
    K = 512
    rng = np.random.Generator(np.random.PCG64(R * 7 + E))
    z = rng.standard_normal((R, E)).astype(np.float32)
    ids = _ids(pattern, R, K, rng)
    zd, idd = torch.from_numpy(z).cuda(), torch.from_numpy(ids.astype(np.int64)).cuda()
    s1, n1 = _code_sums(zd, idd, K)
    s2, n2 = _code_sums(zd, idd, K)
    s1, n1, s2, n2 = s1.cpu().numpy(), n1.cpu().numpy(), s2.cpu().numpy(), n2.cpu().numpy()
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32)) and np.array_equal(n1, n2)     # repeatable
    ref, cnt, ab = VT.code_sums_ref(z, ids, K)
    assert np.array_equal(n1, cnt.astype(np.float32))                                           # exact counts
    bound = VT.code_sums_bound(cnt, ab, ref)
    err = np.abs(s1 - ref)
    r = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0)))
    _note("code_sums", r)
    assert r <= 1.0, "code sums err / bound = %.3g" % r
    # the documented order: chunk-ordered sums of ascending per-chunk partials, bit for bit
    chunked = VT.code_sums_chunked_f32(z, ids, K)
    assert np.array_equal(s1.view(np.uint32), chunked.view(np.uint32))


def test_code_sums_refusals():
    import torch
    from qpgesture_amd import _lib
    K, R = 512, 100
    ids = torch.zeros((R,), dtype=torch.int64, device="cuda:0")
    for E in (6, 1028):
        with pytest.raises(RuntimeError):
            _code_sums(torch.zeros((R, E), device="cuda:0"), ids, K)
    z = torch.zeros((R, 64), device="cuda:0")
    need = int(_lib.load().qpg_vq_code_sums_ws_bytes(R, 64, K))
    with pytest.raises(RuntimeError):
        _code_sums(z, ids, K, ws_bytes=need - 1)
    _code_sums(z, ids, K, ws_bytes=need)


# ----------------------------------------------------------------------------------------------------------------
# 3. EMA update
# ----------------------------------------------------------------------------------------------------------------
def _ema_ref(z, ids, k, k_sum, k_elem, k_rand, mu, threshold):
    import torch
    from oracle import vqvae_oracle as VO
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)      # noqa: E731
    kn, ks, ke, met = VO.ema_update(f(z), torch.as_tensor(np.asarray(ids, np.int64)), f(k), f(k_sum), f(k_elem),
                                    f(k_rand), mu=mu, threshold=threshold)
    return kn.numpy(), ks.numpy(), ke.numpy(), {a: float(b) for a, b in met.items()}


def _ema_compare(got, ref, old, mu, threshold, floors=True):
    """got / ref: (k, k_sum, k_elem, kk, out4 | metrics); old: (k_sum, k_elem, bsum, belem) before the update."""
    k, ks, ke, kk, out4 = got
    rk, rks, rke, met = ref
    oks, oke, bsum, belem = old
    a = np.float64(mu)
    b = 1.0 - a
    # k_sum / k_elem: two products and a sum, each rounded once in f32
    bs = 3 * U * (a * np.abs(oks) + b * np.abs(bsum))
    be = 3 * U * (a * np.abs(oke) + b * np.abs(belem))
    assert np.all(np.abs(ks - rks) <= bs), float(np.max(np.abs(ks - rks) / np.maximum(bs, 1e-300)))
    assert np.all(np.abs(ke - rke) <= be)
    kept = rke >= threshold
    assert np.array_equal(ke >= threshold, kept)
    # kept codes: k_sum / k_elem (3 u each) and a correctly rounded division; restarted codes: the k_rand row exactly
    bk = (bs / np.maximum(rke, 1e-300)[:, None] + np.abs(rk) * (be / np.maximum(rke, 1e-300))[:, None] + U * np.abs(rk))
    rr = np.where(np.abs(k - rk) > 0, np.abs(k - rk) / np.maximum(bk, 1e-300), 0)[kept]
    r = float(rr.max()) if rr.size else 0.0
    _note("ema_update", r)
    assert r <= 1.0, "k err / bound = %.3g" % r
    assert np.array_equal(k[~kept], rk[~kept])
    # kk = |k|^2 of the kernel's own k, accumulated in f64 and rounded once
    kk_ref = np.sum(k.astype(np.float64) ** 2, axis=1)
    assert np.all(np.abs(kk - kk_ref) <= U * kk_ref * 1.0001)
    # metrics: counts exact; entropy / dk within their f32 bounds, and their floors (the training metrics) equal
    ent, used, usage, dk = (float(v) for v in out4)
    assert used == met["used_curr"] and usage == met["usage"]
    assert abs(ent - met["entropy"]) <= 1e-5 * abs(met["entropy"]) + 1e-6, (ent, met["entropy"])
    assert abs(dk - met["dk"]) <= 1e-5 * abs(met["dk"]) + 1e-12, (dk, met["dk"])
    if floors:
        for v, w in ((ent, met["entropy"]), (dk, met["dk"])):
            assert np.floor(v) == np.floor(w), (v, w)


def _ema_inputs(K, E, rng):
    """Codebook state and a batch with planted edges: code 0 lands on threshold exactly (kept), code 1 one ulp below
    (restarted), codes 2..9 get no rows; batch sums exact in f32."""
    R = 6 * K
    z = (rng.integers(-64, 64, (R, E)) / 8.0).astype(np.float32)
    ids = rng.integers(10, K, R)
    ids[0], ids[1] = 0, 1
    k = rng.standard_normal((K, E)).astype(np.float32)
    k_sum = rng.standard_normal((K, E)).astype(np.float32)
    k_elem = rng.uniform(0.1, 4.0, K).astype(np.float32)
    k_elem[0], k_elem[1] = 1.0, np.nextafter(np.float32(1.0), np.float32(0.0))
    k_rand = rng.standard_normal((K, E)).astype(np.float32)
    bsum = np.zeros((K, E), np.float64)
    np.add.at(bsum, ids, z.astype(np.float64))
    belem = np.bincount(ids, minlength=K).astype(np.float64)
    ne = 0.99 * k_elem[2:].astype(np.float64) + 0.01 * belem[2:]        # keep the other codes off the threshold
    k_elem[2:][np.abs(ne - 1.0) < 1e-3] += np.float32(0.01)
    assert belem[0] == belem[1] == 1 and np.all(belem[2:10] == 0)
    return z, ids, k, k_sum, k_elem, k_rand, bsum.astype(np.float32), belem.astype(np.float32)


def _ema_gpu(k, k_sum, k_elem, bsum, belem, k_rand, mu, threshold, ldkT):
    import torch
    from qpgesture_amd import _lib
    K, E = k.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    kd, ksd, ked = d(k), d(k_sum), d(k_elem)
    kT = torch.full((E, ldkT), 7.0, device="cuda:0")
    kk = torch.empty((K,), device="cuda:0")
    ws = torch.empty((8 * K,), dtype=torch.uint8, device="cuda:0")
    out = torch.empty((4,), device="cuda:0")
    _lib.call("qpg_vq_ema_update_f32", "cuda:0", kd, ksd, ked, d(bsum), d(belem), d(k_rand), mu, threshold, K, E, kT,
              ldkT, kk, ws, ws.numel(), out)
    return kd.cpu().numpy(), ksd.cpu().numpy(), ked.cpu().numpy(), kk.cpu().numpy(), out.cpu().numpy(), kT.cpu().numpy()


@pytest.mark.parametrize("K,E,ldkT", [(96, 64, 128), (512, 512, 512)])
def test_ema_update_vs_f64(K, E, ldkT):
    rng = np.random.Generator(np.random.PCG64(K + E))
    mu, thr = float(np.float32(0.99)), 1.0          # the kernel's mu is f32: the reference uses the same value
    z, ids, k, k_sum, k_elem, k_rand, bsum, belem = _ema_inputs(K, E, rng)
    got = _ema_gpu(k, k_sum, k_elem, bsum, belem, k_rand, mu, thr, ldkT)
    ref = _ema_ref(z, ids, k, k_sum, k_elem, k_rand, mu, thr)
    # precondition: no code but the planted two within rounding distance of the threshold
    near = np.abs(ref[2] - thr) < 1e-4
    assert list(np.nonzero(near)[0]) == [0, 1], np.nonzero(near)
    assert ref[2][0] == 1.0 and got[2][0] == 1.0 and got[2][1] < 1.0
    _ema_compare(got[:5], ref, (k_sum, k_elem, bsum, belem), mu, thr)
    assert not np.array_equal(got[0][0], k_rand[0]) and np.array_equal(got[0][1], k_rand[1])   # kept / restarted
    kT = got[5]
    assert np.array_equal(kT[:, :K], got[0].T) and np.all(kT[:, K:] == 7.0)


def test_ema_update_mu_one_moves_nothing():
    rng = np.random.Generator(np.random.PCG64(3))
    K, E = 96, 64
    z, ids, k, k_sum, k_elem, k_rand, bsum, belem = _ema_inputs(K, E, rng)
    k_elem = np.maximum(k_elem, 1.5).astype(np.float32)                  # every code kept
    k = (k_sum / k_elem[:, None]).astype(np.float32)
    kn, ks, ke, kk, out, kT = _ema_gpu(k, k_sum, k_elem, bsum, belem, k_rand, 1.0, 1.0, 128)
    assert np.array_equal(ks, k_sum) and np.array_equal(ke, k_elem) and np.array_equal(kn, k)
    assert float(out[3]) == 0.0


def test_update_k_production_shape_and_refresh_quantiser(model):
    """VQVAE._update_k at R = 7 680, E = K = 512 (code sums, broadcast, EMA) against the f64 EMA with the same k_rand;
    then _refresh_quantiser() (init_k's path) and load_state_dict() of the exported state (a checkpoint restore) must
    leave kT and kk bit-identical to what the EMA step wrote."""
    import torch
    m = model
    R, E, K = 7680, 512, 512
    rng = np.random.Generator(np.random.PCG64(99))
    z = (rng.standard_normal((R, E)) * 0.5).astype(np.float32)
    ids = rng.integers(0, K, R)
    ids[rng.random(R) < 0.3] = 11                                        # a popular code across every chunk
    k0, ks0 = m.k.cpu().numpy().copy(), (m.k.cpu().numpy() * 2).astype(np.float32)
    ke0 = rng.uniform(0.5, 3.0, K).astype(np.float32)
    m.k_sum, m.k_elem = torch.from_numpy(ks0).cuda(), torch.from_numpy(ke0).cuda()
    m.mu = float(np.float32(0.99))
    zd = torch.from_numpy(z).cuda()
    torch.manual_seed(1234)
    out = m._update_k(zd, torch.from_numpy(ids.astype(np.int64)).cuda())
    torch.manual_seed(1234)
    k_rand = z[torch.randperm(R)[:K].numpy()]
    ref = _ema_ref(z, ids, k0, ks0, ke0, k_rand, m.mu, m.threshold)
    got = (m.k.cpu().numpy(), m.k_sum.cpu().numpy(), m.k_elem.cpu().numpy(), m.kk.cpu().numpy(), out.cpu().numpy())
    # (the batch sums went through f32: their rounding, n_c u sum|z|, is within the k_sum bound's slack for these rows)
    assert np.abs(got[1] - ref[1]).max() <= 1e-5 * max(1.0, np.abs(ref[1]).max())
    assert np.abs(got[2] - ref[2]).max() <= 4 * U * np.abs(ref[2]).max()
    assert float(got[4][1]) == ref[3]["used_curr"] and float(got[4][2]) == ref[3]["usage"]
    kept = ref[2] >= m.threshold
    assert np.array_equal(got[0][~kept], ref[0][~kept]) and np.abs(got[0] - ref[0]).max() <= 1e-5
    kT, kk = m.kT.w.clone(), m.kk.clone()
    m._refresh_quantiser()
    torch.cuda.synchronize()
    assert torch.equal(m.kT.w, kT), "kT differs after _refresh_quantiser"
    n_diff = int((m.kk != kk).sum())
    assert n_diff == 0, "_refresh_quantiser changed kk in %d codes" % n_diff
    # a checkpoint restore (train.py --resume: load_state_dict) leaves them bit-identical too
    m.load_state_dict(m.state_dict())
    torch.cuda.synchronize()
    assert torch.equal(m.kT.w, kT), "kT differs after load_state_dict"
    n_diff = int((m.kk != kk).sum())
    assert n_diff == 0, "load_state_dict changed kk in %d codes" % n_diff


# ----------------------------------------------------------------------------------------------------------------
# 4. Adam
# ----------------------------------------------------------------------------------------------------------------
def _grad_seq(n, steps, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.standard_normal(n).astype(np.float32)
    out = []
    for s in range(steps):
        g = base * rng.uniform(0.5, 2.0, n).astype(np.float32) * np.where(rng.random(n) < 0.3, -1, 1)
        g[::7] = 0.0                              # exact zeros
        g[1::11] = 1e-30                          # tiny: g * g underflows
        g[2::13] = 1e4 * (1 if s % 2 else -1)      # huge, flipping sign every step
        out.append(g.astype(np.float32))
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
@pytest.mark.parametrize("betas", [(0.5, 0.999), (0.9, 0.999)])
def test_adam_vs_f64_and_torch(n, betas):
    """200 steps, MultiStepLR milestones at 60 and 140, a state_dict round trip at step 100.

    Tight: every step is replayed in f64 from the kernel's own state with the f32 lr / betas / eps it receives
    (adam_step_f64): m within 2 u, v within 3 u of their terms, the update within 1e-6 relative plus the final
    rounding of p.
    Loose: torch.optim.Adam on CPU f32 over the whole run.  torch keeps beta2 in double for 1 - beta2 and the bias
    correction, the kernel uses f32(beta2) = beta2 + d2 (d2 = 1.29e-8 for 0.999): 1 - beta2 differs by d2 / (1 - beta2)
    = 1.3e-5 relative, and bc2 = 1 - beta2^t by t d2 / bc2 <= d2 / (1 - beta2) (t beta2^(t-1) (1 - beta2) <= bc2), so
    v / bc2 - and with it sqrt(v / bc2) - moves by at most rho2 = 2 d2 / (1 - beta2) + 200 d2 relative (the second term:
    the beta2^(t-k) weights of old gradients, t - k <= 200); beta1 likewise (d1 = 2.4e-8 for 0.9, 0 for 0.5):
    rho1 = 2 d1 / (1 - beta1) + 200 d1.  Each step's update therefore differs by <= (rho1 + rho2 + 16 u) |update|
    (16 u: the f32 roundings of the two implementations, torch's lerp form of m included), and p by the sum of that
    over the steps plus one rounding of p per step (u |p|)."""
    import torch
    from oracle import vqtrain_oracle as VT
    from qpgesture_amd.optim import Adam, MultiStepLR
    steps, lr = 200, 3e-3
    rng = np.random.Generator(np.random.PCG64(n))
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = _grad_seq(n, steps, n + 1)
    f32 = lambda v: float(np.float32(v))         # noqa: E731
    b1f, b2f, epsf = f32(betas[0]), f32(betas[1]), f32(1e-8)

    p = torch.from_numpy(p0.copy()).cuda()
    gbuf = torch.zeros_like(p)
    opt = Adam((p, gbuf), lr=lr, betas=betas)
    sch = MultiStepLR(opt, [60, 140], 0.1)
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    topt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=1e-8)
    tsch = torch.optim.lr_scheduler.MultiStepLR(topt, [60, 140], 0.1)
    d1, d2 = abs(b1f - betas[0]), abs(b2f - betas[1])
    rho = 2 * d1 / (1 - betas[0]) + steps * d1 + 2 * d2 / (1 - betas[1]) + steps * d2 + 16 * U
    drift = np.zeros(n)
    worst_tight = 0.0
    for s in range(1, steps + 1):
        g = grads[s - 1]
        gbuf.copy_(torch.from_numpy(g))
        pb, mb, vb = p.cpu().numpy(), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()
        lr_now = opt.lr
        opt.step()
        pa, ma, va = p.cpu().numpy(), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()
        rp, rm, rv = VT.adam_step_f64(pb, g, mb, vb, f32(lr_now), b1f, b2f, epsf, s)
        # m: two products and a sum, each rounded once (<= u relative each); v: three roundings on the g^2 term
        # ((1 - b2) g) g, two on b2 v (+ f32 underflow of g^2 for the 1e-30 gradients)
        tm = b1f * np.abs(mb) + (1 - b1f) * np.abs(g.astype(np.float64))
        tv = b2f * np.abs(vb) + (1 - b2f) * g.astype(np.float64) ** 2
        assert np.all(np.abs(ma - rm) <= 2 * U * tm + 1e-45), s
        assert np.all(np.abs(va - rv) <= 3 * U * tv + 1e-45), s
        upd_ref = pb.astype(np.float64) - rp
        e = np.abs((pb.astype(np.float64) - pa) - upd_ref)
        # ~8 roundings in the update (bc1, sqrt(bc2), lr / bc1, sqrt, /, + eps, /, *): 1e-6 > 16 u; then the rounding of
        # p - update to f32, <= u |p - update|
        # (relative to the update m's terms would give: a sign flip can cancel m far below its own rounding)
        mag = np.abs(upd_ref) * np.divide(tm, np.abs(rm), out=np.zeros(n), where=rm != 0)
        tb = 1e-6 * mag + U * (np.abs(pb) + np.abs(upd_ref)) + 1e-30
        worst_tight = max(worst_tight, float(np.max(e / tb)))
        assert np.all(e <= tb), (s, float(np.max(e / tb)))
        tp.grad = torch.from_numpy(g.copy())
        tbefore = tp.detach().numpy().astype(np.float64).copy()
        st = topt.state.get(tp, {})
        m_prev = st["exp_avg"].numpy().astype(np.float64).copy() if "exp_avg" in st else np.zeros(n)
        t_lr = topt.param_groups[0]["lr"]
        topt.step()
        v_now = topt.state[tp]["exp_avg_sq"].numpy().astype(np.float64)
        # the update's magnitude without cancellation in m
        mag = (t_lr / (1 - betas[0] ** s) * (betas[0] * np.abs(m_prev) + (1 - betas[0]) * np.abs(g))
               / (np.sqrt(v_now) / np.sqrt(1 - betas[1] ** s) + 1e-8))
        rho_s = rho + (s + 4 / (1 - betas[0])) * U          # + rounding carried in v (s steps) and m (decaying)
        drift += rho_s * mag + U * np.abs(tbefore)
        sch.step()
        tsch.step()
        if s == 100:
            sd = opt.state_dict()
            p_mid = p.clone()
    _note("adam_tight", worst_tight)
    tdiff = np.abs(p.cpu().numpy().astype(np.float64) - tp.detach().numpy())
    r = float(np.max(np.where(tdiff > 0, tdiff / np.maximum(drift, 1e-300), 0)))
    _note("adam_vs_torch", r)
    assert r <= 1.0, "parameter drift from torch.optim.Adam / derived bound = %.3g" % r

    # state_dict round trip at step 100, then the same 100 steps: bit-identical
    p2 = p_mid.clone()
    g2 = torch.zeros_like(p2)
    opt2 = Adam((p2, g2), lr=lr, betas=betas)
    opt2.load_state_dict(sd)
    sch2 = MultiStepLR(opt2, [60, 140], 0.1)
    sch2.base_lr, sch2.epoch = lr, 100
    for s in range(101, steps + 1):
        g2.copy_(torch.from_numpy(grads[s - 1]))
        opt2.step()
        sch2.step()
    assert torch.equal(p2, p)


# ----------------------------------------------------------------------------------------------------------------
# 5. loss, loss gradient, latent statistics, commit gradient
# ----------------------------------------------------------------------------------------------------------------
def _loss_inputs(B, T, C, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    # values on a 2^-10 grid below 2^6: every difference / second difference the kernels form is exact in f32, so the
    # signs they take are the exact ones and the planted zeros are exact zeros on both sides
    grid = lambda t: torch.round(t * 1024) / 1024         # noqa: E731
    x = grid(torch.randn(B, T, C, generator=g))
    xo = grid(x + 0.3 * torch.randn(B, T, C, generator=g))
    xo[0, :, 0] = x[0, :, 0]                                        # x_out - x == 0
    if T >= 4:
        xo[0, :, 1] = x[0, :, 1] + 0.25                             # first differences equal (constant offset)
        x[0, 1:4, 2] = 1.0                                          # constant stretches: first / second differences 0
        xo[0, 1:4, 2] = 2.0
        xo[0, :, 3] = x[0, :, 3] + 0.5 * torch.arange(T, dtype=torch.float32)   # second differences equal
    return x, xo


@pytest.mark.parametrize("B,T", [(256, 240), (4, 3), (6, 8)])
def test_loss_and_loss_grad_vs_f64(model, B, T):
    import torch
    from oracle import vqvae_oracle as VO
    from qpgesture_amd import _lib
    m, C = model, 135
    x, xo = _loss_inputs(B, T, C, B + T)
    commit = torch.tensor([0.37], device="cuda:0")
    ws = m._red_ws()
    out6 = torch.empty((6,), device="cuda:0")
    # distinct weights per term (and an upstream gradient != 1), so that a weight on the wrong term shows
    w_com, w_reg, w_vel, w_acc, up = 0.02, 0.3, 0.7, 1.3, 0.5
    _lib.call("qpg_vq_loss_f32", "cuda:0", xo.cuda(), x.cuda(), B, T, C, commit, w_com, w_reg, w_vel, w_acc, ws,
              ws.numel(), out6)
    xl = xo.double().requires_grad_(True)
    loss, met = VO.losses(x.double(), xl, torch.tensor(0.37, dtype=torch.float64), hps_commit=w_com, vel=w_vel,
                          acc=w_acc, reg=w_reg)
    loss.backward(torch.tensor(up, dtype=torch.float64))
    got = out6.cpu().numpy().astype(np.float64)
    # exact terms (reg: one rounding of a^2) summed in f64, one f32 rounding of the mean: 2 u relative
    for i, kk in ((1, "recons_loss"), (2, "regularization"), (3, "velocity_loss"), (4, "acceleration_loss")):
        ref = float(met[kk])
        r = abs(got[i] - ref) / (2 * U * abs(ref) + 1e-30)
        _note("loss", r)
        assert r <= 1.0, (kk, got[i], ref)
    r = abs(got[0] - float(loss)) / (8 * U * float(sum(abs(float(v)) for v in (met["recons_loss"],
            met["regularization"] * w_reg, met["velocity_loss"] * w_vel, met["acceleration_loss"] * w_acc,
            0.37 * w_com))) + 1e-30)
    _note("loss", r)
    assert r <= 1.0 and got[5] == np.float32(0.37)
    dxo = torch.empty((B, T, C), device="cuda:0")
    _lib.call("qpg_vq_loss_grad_f32", "cuda:0", xo.cuda(), x.cuda(), B, T, C, w_reg, w_vel, w_acc, up, dxo)
    got = dxo.cpu().numpy().astype(np.float64)
    ref = xl.grad.numpy()
    # exact signs: the error is the f32 rounding of the weights (1/n) and of the sum of <= 9 terms, each <= 4/n2 or
    # 0.3 * 2 |a| * 2 / n2, times weights <= 1.3 (a sign error or a misplaced weight would be a whole term)
    n2 = B * max(T - 2, 1) * C
    err = np.abs(got - ref)
    amax = float((xo[:, 2:] + xo[:, :-2] - 2 * xo[:, 1:-1]).abs().max()) if T > 2 else 0.0
    bound = 16 * U * (np.abs(ref) + w_acc * up * (9 + 9 * 1.2 * amax) / n2) + 1e-30
    r = float(np.max(err / bound))
    _note("loss_grad", r)
    assert r <= 1.0, "loss gradient err / bound = %.3g" % r


def test_latent_stats_vs_f64():
    """commit, fit, prenorm at R = 7 680, E = 512, with latents whose |mean| >> std (prenorm = sqrt(s2 - n mean^2))."""
    import torch
    from qpgesture_amd import _lib
    R, E = 7680, 512
    g = torch.Generator().manual_seed(5)
    for shift in (0.0, 30.0):
        z = torch.randn(R, E, generator=g) * 0.2 + shift
        zq = z + 0.1 * torch.randn(R, E, generator=g)
        dmin = torch.rand(R, generator=g) * 3
        ws = torch.empty((int(_lib.load().qpg_vq_reduce_ws_bytes()),), dtype=torch.uint8, device="cuda:0")
        out = torch.empty((3,), device="cuda:0")
        _lib.call("qpg_vq_latent_stats_f32", "cuda:0", z.cuda(), zq.cuda(), dmin.cuda(), R, E, ws, ws.numel(), out)
        got = out.cpu().numpy().astype(np.float64)
        zd, zqd = z.double(), zq.double()
        n = R * E
        commit = float(((zqd - zd) ** 2).sum() / n)       # the kernel squares the f32 difference: 3 u per term
        fit = float(dmin.double().mean())
        prenorm = float(torch.norm(zd - zd.mean()) / np.sqrt(n))
        assert abs(got[0] - commit) <= 4 * U * commit and abs(got[1] - fit) <= 2 * U * fit
        # s2 - n mean^2 in f64: cancellation costs ~ n mean^2 * 2^-52 * n^0.5 of the variance
        dev_bound = 2 * U * prenorm + (float(zd.mean()) ** 2 * 2.0 ** -52 * np.sqrt(n)) / max(prenorm, 1e-30)
        r = abs(got[2] - prenorm) / dev_bound
        _note("latent_stats", r)
        assert r <= 1.0, (shift, got[2], prenorm)


@pytest.mark.parametrize("with_dzq", [False, True])
def test_commit_grad_vs_f64(with_dzq):
    import torch
    from qpgesture_amd import _lib
    R, E, scale = 7680, 512, 0.02
    g = torch.Generator().manual_seed(6)
    z, zq = torch.randn(R, E, generator=g), torch.randn(R, E, generator=g)
    dzq = torch.randn(R, E, generator=g) * 1e-6 if with_dzq else None
    dz = torch.empty((R, E), device="cuda:0")
    _lib.call("qpg_vq_commit_grad_f32", "cuda:0", z.cuda(), zq.cuda(), R, E, scale, None if dzq is None else dzq.cuda(),
              dz)
    zd = z.double().requires_grad_(True)
    commit = ((zq.double() - zd) ** 2).sum() / (R * E)
    (scale * commit).backward()
    ref = zd.grad.numpy() + (dzq.double().numpy() if with_dzq else 0)
    got = dz.cpu().numpy().astype(np.float64)
    term = np.abs(zd.grad.numpy())
    bound = 6 * U * term + (2 * U * np.abs(ref) if with_dzq else 0) + 1e-45
    r = float(np.max(np.abs(got - ref) / bound))
    _note("commit_grad", r)
    assert r <= 1.0
