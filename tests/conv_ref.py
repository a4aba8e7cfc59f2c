"""Contract of the VQ-VAE's forward kernels (csrc/qpg_vqvae.hip, qpg_convt.hip, qpg_conv16.hip), stated apart from them:
the convolution of include/qpg.h in float64, the a-priori f32 error bound of every kernel from its accumulation
structure, the launchers' choice of kernel restated as pure functions of the shape and the CU count, the quantiser's
argmin in float64, the table of cases the GPU test runs and planted faults the bounds must reject.

Used by tests/test_conv_contract_cpu.py (no GPU: the bounds reject every planted fault at every case, the case table hits
every kernel variant the production shapes can reach) and tests/test_gpu_conv_contract.py (the kernels against all this).

Activations are channels-last (B, T, C); weights [tap][Cin][Cout]; geometry as in include/qpg.h:
    y[b][t * out_stride + out_offset] = act_out(bias + sum_{tap, ci} w[tap][ci] act_in(x[b][t * in_stride + in_offset + tap * dil][ci])) (+ residual)
for t < T_out, input rows outside [0, T_in) zero.  An entry passes when |got - ref| <= gamma(chains) * absref
(oracle/vqtrain_oracle.py), absref the same contraction on |act_in(x)|, |w|, |bias|, |residual| without the output ReLU.
"""
import collections
import math

import numpy as np
import torch

from oracle.vqtrain_oracle import U, bound_ratio, gamma  # noqa: F401  (re-exported: the tests use these, not copies)

SENTINEL = 7.0
Geom = collections.namedtuple("Geom", "in_stride in_offset dil T_out out_stride out_offset T_y")


def pad(n, m):
    return (n + m - 1) // m * m


def _f64(a):
    return None if a is None else torch.as_tensor(a).detach().to("cpu", torch.float64)


# ----------------------------------------------------------------------------------------------------------------
# the definition
# ----------------------------------------------------------------------------------------------------------------
def _w_exp(w):
    """qpg_conv16_pack_weights' scale exponent (conv16_wexp_kernel): max |w| 2^e in [2^9, 2^10)."""
    amax = float(w.abs().max())
    return 10 - math.frexp(amax)[1] if amax > 0 else 0


def conv_eval(x, w, bias, geom, relu_in, relu_out, residual, rows=None, absolute=False, fault=None, cin_pad=None):
    """The convolution in f64 at the output positions `rows` (flat m = b * T_out + t; all of them by default) ->
    (len(rows), Cout).  residual is indexed like y: (B, T_y, Cout).  absolute: the contraction on magnitudes.
    fault: a planted defect (see faults_of) as (name, argument); cin_pad: the K axis' channel padding the fault's k indices
    count in (k = tap * cin_pad + ci)."""
    x, w, bias, residual = _f64(x), _f64(w), _f64(bias), _f64(residual)
    g = Geom(*geom)
    B, T_in, Cin = x.shape
    taps, _, Cout = w.shape
    cin_pad = cin_pad or Cin
    name, arg = fault if fault else (None, None)
    M = B * g.T_out
    rows = torch.arange(M) if rows is None else torch.as_tensor(rows, dtype=torch.int64)
    if name == "parity":                  # the rows looked at were never written
        return torch.full((rows.numel(), Cout), SENTINEL, dtype=torch.float64)
    b, t = rows // g.T_out, rows % g.T_out
    xa = torch.relu(x) if relu_in and name != "no_relu_in" else x
    if absolute:
        xa, w = xa.abs(), w.abs()
        bias = None if bias is None else bias.abs()
        residual = None if residual is None else residual.abs()
    xf = xa.reshape(B * T_in, Cin)
    acc = torch.zeros((rows.numel(), Cout), dtype=torch.float64)
    for tap in range(taps):
        if name == "drop_tap" and tap == arg:
            continue
        t_in = t * g.in_stride + g.in_offset + tap * g.dil + (1 if name == "shift_tap" and tap == arg else 0)
        flat = b * T_in + t_in
        ok = (t_in >= 0) & (t_in < T_in)
        if name == "halo":                # the neighbouring batch item's row where padding belongs
            ok = (flat >= 0) & (flat < B * T_in)
        xg = xf[flat.clamp(0, B * T_in - 1)] * ok[:, None].to(torch.float64)
        wt = w[tap]
        if name == "drop_k":              # k in [lo, hi) left out of the contraction
            lo, hi = arg[0] - tap * cin_pad, arg[1] - tap * cin_pad
            if lo < Cin and hi > 0:
                wt = wt.clone()
                wt[max(lo, 0):max(min(hi, Cin), 0)] = 0.0
        acc += xg @ wt
        if name == "drop_lh":             # split-f16: the (weight l plane) x (activation h plane) product missing
            e = _w_exp(w)
            ws = wt * 2.0 ** e
            wl = (ws - ws.to(torch.float16).double()).to(torch.float16).double()
            acc -= (xg.to(torch.float16).double() @ wl) * 2.0 ** -e
    if bias is not None:
        acc = acc + bias * (2.0 if name == "bias2" else 1.0)
    if relu_out and not absolute:
        acc = torch.relu(acc)
    if residual is not None and name != "no_res":
        acc = acc + residual[b, t * g.out_stride + g.out_offset]
    return acc


def conv_ref(x, w, bias, geom, relu_in=False, relu_out=False, residual=None, rows=None):
    """(ref, absref) in f64: (B, T_out, Cout) (or (len(rows), Cout))."""
    g = Geom(*geom)
    out = [conv_eval(x, w, bias, g, relu_in, relu_out, residual, rows, absolute) for absolute in (False, True)]
    if rows is None:
        out = [o.view(x.shape[0], g.T_out, -1) for o in out]
    return out[0], out[1]


def resblock_eval(x, w1, b1, w2, b2, dil, rows=None, absolute=False, fault=None):
    """ResConv1DBlock (resnet.py:31-46), y = x + W2 . relu(W1 (*) relu(x) + b1) + b2 in f64 at `rows` -> (h, y).  The
    absolute contraction goes through both layers (oracle/vqtrain_oracle.py "res").  Faults on either layer: the first
    layer takes the convolution's, "no_res" and "bias2" hit the second."""
    x = _f64(x)
    B, T, C = x.shape
    g1 = Geom(1, -dil, dil, T, 1, 0, T)
    name = fault[0] if fault else None
    f1 = fault if name not in ("no_res", "bias2", None) else None
    h = conv_eval(x, w1, b1, g1, True, True, None, rows, absolute, f1, 512)
    M = B * T
    rows = torch.arange(M) if rows is None else torch.as_tensor(rows, dtype=torch.int64)
    w2, b2 = _f64(w2), _f64(b2)
    xr = x.reshape(M, C)[rows]
    if absolute:
        w2, b2, xr = w2.abs(), b2.abs(), xr.abs()
    y = h @ w2[0] + b2 * (2.0 if name == "bias2" else 1.0)
    if name != "no_res":
        y = y + xr
    return h, y


def resblock_ref(x, w1, b1, w2, b2, dil, rows=None):
    """(h_ref, y_ref, abs_h, abs_y) in f64, (B, T, 512) each (or per row of `rows`)."""
    h, y = resblock_eval(x, w1, b1, w2, b2, dil, rows)
    ah, ay = resblock_eval(x, w1, b1, w2, b2, dil, rows, absolute=True)
    if rows is None:
        h, y, ah, ay = (v.view(x.shape) for v in (h, y, ah, ay))
    return h, y, ah, ay


# ----------------------------------------------------------------------------------------------------------------
# the launch rules, restated (n_cu: the device's CU count)
# ----------------------------------------------------------------------------------------------------------------
def conv1d_plan(M, Cin, Cin_pad, Cout, Cout_pad, taps, aligned_x, aligned_out, ws_floats, n_cu):
    """conv_launch (csrc/qpg_vqvae.hip:320-342) -> (MT, VEC, vec_out, ks).  aligned_x: x 16-byte aligned; aligned_out: y,
    residual, bias all 16-byte aligned (or absent); ws_floats: None without a workspace."""
    vec = Cin % 4 == 0 and bool(aligned_x)                                     # :322
    big = M * (Cout_pad // 128) >= 128 * 2 * n_cu                              # :324
    BM = 128 if big else 64
    blocks = -(-M // BM) * (Cout_pad // 128)                                   # :326
    total = taps * (Cin_pad // 16)                                             # :327
    ks = 1
    if ws_floats is not None and blocks < n_cu and total >= 16:                # :331
        ks = min(-(-n_cu // blocks), 8, total // 8)                            # :332-334
        if ks * M * Cout_pad > ws_floats:                                      # :335
            ks = int(ws_floats // (M * Cout_pad))
        if ks < 2:                                                             # :336
            ks = 1
    vec_out = Cout % 4 == 0 and M < 2 ** 31 and bool(aligned_out)              # :341
    return (2 if big else 1, vec, vec_out, ks)


def convt_plan(M, taps, Cin_pad, Cout_pad, nz, relu_in, n_cu):
    """convt_launch (csrc/qpg_convt.hip:603-653) -> ("small", relu, pd, nq) | ("generic", relu)."""
    relu = bool(relu_in)
    if -(-M // 64) * (Cout_pad // 128) * 2 * nz >= 3 * n_cu:                   # :603
        return ("generic", relu)
    nq, best = 4, 0
    for cand in (4, 2, 1):                                                     # :610-617
        blocks = -(-M // 16) * (Cout_pad // (16 * cand)) * nz
        cost = -(-blocks // n_cu) * (cand + 1)
        if cand == 4 or cost < best:
            best, nq = cost, cand
    nkb = taps * Cin_pad // 64 * 4
    per = -(-nkb // 8)                                                         # :618
    pd = 4 if nkb % 8 == 0 and per % 4 == 0 else 0                             # :619
    return ("small", relu, pd, nq)


def resblock_fused(B, T, n_cu):
    """VqWalk::resnet (csrc/qpg_vqvae.hip:585) and VQVAE._fused_block_fills_chip: the one-launch block where its
    64-position tiles fill the chip."""
    return -(-(B * T) // 64) * 4 >= 3 * n_cu


def ks_class(ks):
    return ks if ks in (1, 2, 8) else "interior"


# ----------------------------------------------------------------------------------------------------------------
# chains and bounds
# ----------------------------------------------------------------------------------------------------------------
def conv1d_chains(taps, Cin_pad, ks):
    """conv1d_mfma_f32_kernel: one accumulator per entry over the block's K slices of 16 in order; split-K: ceil(total /
    ks) slices per partial (:169), the partials added in slice order by conv_splitk_reduce_kernel (:309); then bias, ReLU,
    residual."""
    total = taps * (Cin_pad // 16)
    return [total * 16, 3] if ks == 1 else [-(-total // ks) * 16, ks, 3]


def convt_chains(plan, taps, Cin_pad):
    """convt_f32_kernel: one accumulator over K.  convt_small_f32_kernel: its 8 waves take ceil(nkb / 8) 16-k blocks each
    (:457; K / 8 when that divides, more for the 144-channel k4 layer: 5 of 36 blocks), the 8 partials added in wave
    order (:527)."""
    K = taps * Cin_pad
    if plan[0] == "generic":
        return [K, 3]
    return [-(-(K // 16) // 8) * 16, 8, 3]


RES_CHAINS_H = [1536, 2]
# y: the accumulators of the second GEMM start from residual + bias (resblock_fused_f32_kernel phase 2) and then run the
# 512-long chain - the table's lengths in another order; the hidden activation's error enters through |W2|, which
# gamma(both layers' chains) * abs_y covers (abs_y = |x| + |W2| abs_h + |b2|)
RES_CHAINS_Y = [1536, 2, 512, 2]


def conv16_bound(absref, w, x_shape, geom, cin):
    """The header of csrc/qpg_conv16.hip: (K / 32 * 1.3 * 2^-24 + 2^-21) * absref + 2^-25 * sum |w| over the in-range taps
    of the output channel (the subnormal l planes of small activations).  K = taps x Cin rounded up to the 32-wide slice.
    absref (B, T_out, Cout); w [taps][Cin][Cout]."""
    g = Geom(*geom)
    B, T_in = x_shape[0], x_shape[1]
    taps = w.shape[0]
    K = taps * pad(cin, 32)
    wsum = _f64(w).abs().sum(dim=1)                                            # (taps, Cout)
    t = torch.arange(g.T_out)
    extra = torch.zeros((g.T_out, w.shape[2]), dtype=torch.float64)
    for tap in range(taps):
        t_in = t * g.in_stride + g.in_offset + tap * g.dil
        extra += ((t_in >= 0) & (t_in < T_in)).to(torch.float64)[:, None] * wsum[tap][None]
    return (K / 32 * 1.3 * 2.0 ** -24 + 2.0 ** -21) * _f64(absref) + 2.0 ** -25 * extra[None].expand(B, -1, -1)


def ratio_to(got, ref, bound):
    """Largest |got - ref| / bound over the entries (bound an array; 0 / 0 counts as 0)."""
    return bound_ratio(got, ref, bound, 1.0)


# ----------------------------------------------------------------------------------------------------------------
# the quantiser
# ----------------------------------------------------------------------------------------------------------------
def argmin_ref(z, dot, kk):
    """f64 distances sum z^2 - 2 dot + kk from the f32 inputs -> (d64 (R, K), dmin, dsecond, ids, b): the row minimum, the
    second minimum (the minimum again when it occurs twice; +inf for K = 1), the lowest minimising index, and the
    per-row f32 bound b = (gamma(ceil(E / 64), 6) + 2 u) (xx + 2 |dot| + kk) at the widest column: vq_argmin_kernel adds
    z^2 by fmaf per lane (ceil(E / 64) terms), six butterfly adds, then 2 dot is exact, one subtraction, one addition."""
    z, dot, kk = (np.asarray(a, np.float64) for a in (z, dot, kk))
    R, E = z.shape
    xx = (z * z).sum(axis=1)
    d = xx[:, None] - 2.0 * dot + kk[None]
    ids = d.argmin(axis=1)                                                     # (first occurrence)
    srt = np.sort(d, axis=1)
    dmin = srt[:, 0]
    dsec = srt[:, 1] if d.shape[1] > 1 else np.full(R, np.inf)
    mag = (xx[:, None] + 2.0 * np.abs(dot) + np.abs(kk)[None]).max(axis=1)
    b = (gamma(-(-E // 64), 6) + 2 * U) * mag
    return d, dmin, dsec, ids, b


def argmin_inputs(R, E, K, seed, ties=()):
    """z (R, E), dot (R, K), kk (K,) f32 made by the test (not by the GEMM): unit-scale distances, so that the gap between
    a row's two best of K columns is far above 2 b for nearly every row.  ties: groups of columns made equal (same dot in
    every row, same kk) and pulled below every other column in the rows r % 3 != 2 - there they ARE the minimum."""
    rng = np.random.Generator(np.random.PCG64(seed))
    z = (rng.standard_normal((R, E)) / math.sqrt(E)).astype(np.float32)
    dot = rng.standard_normal((R, K)).astype(np.float32)
    kk = (1.0 + rng.random(K)).astype(np.float32)
    for grp in ties:
        c0 = grp[0]
        win = (np.arange(R) % 3 != 2)
        dot[win, c0] = 6.0 + rng.random(int(win.sum())).astype(np.float32)
        for c in grp[1:]:
            dot[:, c] = dot[:, c0]
            kk[c] = kk[c0]
    return z, dot, kk


ARGMIN_SHAPES = [  # (R, E, K, tie groups): every R, E, K of the list at least once; ties inside a lane (c, c + 64), across
    # lanes (c, c + 1), first / last column, three columns over two lanes
    (1, 4, 1, ()), (3, 60, 63, ((0, 62),)), (4, 64, 64, ((7, 8),)), (5, 512, 65, ((0, 64),)), (5, 4, 512, ((3, 67),)),
    (1030, 512, 512, ((100, 101),)), (1030, 60, 65, ()), (3, 64, 512, ((9, 73, 74),)), (4, 512, 512, ((0, 511),)),
    (1, 60, 64, ()), (5, 64, 63, ((20, 21),)),
]
# the input sets the tests run: every shape without planted columns (at least 90 % of ALL rows decided), and again with
# them (the planted rows are ties by construction; at least 90 % of the others decided)
ARGMIN_SETS = [s[:3] + ((),) for s in ARGMIN_SHAPES] + [s for s in ARGMIN_SHAPES if s[3]]


# ----------------------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------------------
def _case(kernel, name, B, T_in, **kw):
    c = dict(kernel=kernel, name=name, B=B, T_in=T_in, Cin=512, Cout=512, taps=3, s=1, off=None, dil=1, out_stride=1,
             out_offset=0, relu_in=0, relu_out=0, res=False, mis=None, ws="full", cx_extra=0, nz=1, fused=None)
    c.update(kw)
    if c["off"] is None:
        c["off"] = -c["dil"] * (c["taps"] // 2)
    c["T_out"] = T_in // c["s"]
    c["T_y"] = c["T_out"] * c["out_stride"]
    c["M"] = B * c["T_out"]
    c["Cin_pad"] = pad(c["Cin"], 16)
    c["Cout_pad"] = pad(c["Cout"], 128)
    c["seed"] = 1 + sum(ord(ch) * (i + 1) for i, ch in enumerate(kernel + name)) % 100000
    return c


def geom_of(c):
    return Geom(c["s"], c["off"], c["dil"], c["T_out"], c["out_stride"], c["out_offset"], c["T_y"])


def _split(M):
    """(B, T) with B * T == M and B > 1 where M allows it (sequences of at least 2 positions, as short as possible above
    7: batch boundaries fall inside tiles)."""
    for T in list(range(7, 200)) + [2, 3, 4, 5, 6]:
        if M % T == 0 and M // T > 1:
            return M // T, T
    return 1, M


FULL_WS_SLABS = 8


def ws_floats_of(c):
    """Workspace of a conv1d case in floats (None: no workspace).  "full": room for 8 slabs; a number: that many
    [M][Cout_pad] slabs."""
    if c["ws"] == "none":
        return None
    slab = c["M"] * c["Cout_pad"]
    return FULL_WS_SLABS * slab + 64 if c["ws"] == "full" else int(c["ws"] * slab)


# the layer shapes of the production model (width = emb = l_bins = 512, 135 pose channels) a convolution entry point sees:
# (name, taps, Cin, Cout, in_stride, relu_in, relu_out, residual)
LAYERS = [
    ("down0", 4, 135, 512, 2, 0, 0, False),        # Conv1d(k4, s2, p1) on the pose rows (144 padded channels)
    ("down", 4, 512, 512, 2, 0, 0, False),
    ("res3", 3, 512, 512, 1, 1, 1, False),         # the dilated convolution of a ResConv1DBlock
    ("res1", 1, 512, 512, 1, 0, 0, True),          # its 1x1 convolution + residual
    ("conv3", 3, 512, 512, 1, 0, 0, False),
    ("out", 3, 512, 135, 1, 0, 0, False),
    ("up", 2, 512, 512, 1, 0, 0, False),           # one parity of ConvTranspose1d(k4, s2, p1); convt: the pair, nz = 2
    ("kT", 1, 512, 512, 1, 0, 0, False),           # the quantiser's x . k^T
]


def _layer_case(kernel, layer, tag, M, dil=1, **kw):
    name, taps, cin, cout, s, ri, ro, res = next(l for l in LAYERS if l[0] == layer)
    B, T_out = _split(M)
    off = -1 if s == 2 else None
    return _case(kernel, "%s %s" % (layer, tag), B, T_out * s, Cin=cin, Cout=cout, taps=taps, s=s, off=off,
                 dil=dil, relu_in=ri, relu_out=ro, res=res, **kw)


def _pair_case(tag, M, **kw):
    B, T = _split(M)
    return _case("pair", "up %s" % tag, B, T, taps=2, out_stride=2, nz=2, **kw)


def convt_variant(c, n_cu):
    return convt_plan(c["M"], c["taps"], c["Cin_pad"], c["Cout_pad"], c["nz"], c["relu_in"], n_cu)


def conv1d_variant(c, n_cu):
    return conv1d_plan(c["M"], c["Cin"], c["Cin_pad"], c["Cout"], c["Cout_pad"], c["taps"], c["mis"] != "x",
                       c["mis"] not in ("y", "res"), ws_floats_of(c), n_cu)


CONVT_LAYERS = ["down0", "res3", "res1", "out", "up"]     # (down, conv3, kT run the variants of res1 / res3 without ReLU)


def _convt_layer_case(layer, tag, M, **kw):
    return _pair_case(tag, M, **kw) if layer == "up" else _layer_case("convt", layer, tag, M, **kw)


def cases(n_cu):
    """The GPU test's cases for a device of n_cu CUs (thresholds computed, not hard-coded)."""
    out = []
    # ---- qpg_conv1d_f32
    edge = [
        _case("conv1d", "M=1 T_in=1 k3 d3", 1, 1, dil=3),
        _case("conv1d", "M=63 k3 d3 relu", 7, 9, dil=3, relu_in=1, relu_out=1),
        _case("conv1d", "M=64 k3 d3 res", 4, 16, dil=3, res=True),
        _case("conv1d", "M=65 k3 d3 relu res", 5, 13, dil=3, relu_in=1, relu_out=1, res=True),
        _case("conv1d", "T=8 d9 relu", 3, 8, dil=9, relu_in=1, relu_out=1),
        _case("conv1d", "k4 s2 Cin=135", 3, 26, Cin=135, taps=4, s=2, off=-1),
        _case("conv1d", "Cout=135", 2, 35, Cout=135),
        _case("conv1d", "k2 parity 0", 2, 9, taps=2, off=-1, out_stride=2, out_offset=0),
        _case("conv1d", "k2 parity 1", 2, 9, taps=2, off=0, out_stride=2, out_offset=1),
    ]
    for c in edge:
        out.append(c)
        out.append(dict(c, name=c["name"] + " no ws", ws="none"))
    for mis in ("x", "y", "res"):
        out.append(_case("conv1d", "1x1 res misaligned %s" % mis, 5, 13, taps=1, res=True, mis=mis, ws="none"))
    m_big = 64 * n_cu                                    # M * (512 / 128) >= 256 n_cu
    b_big, b_small = -(-m_big // 30), (m_big - 1) // 30
    out.append(_case("conv1d", "1x1 128-row tiles", b_big, 30, taps=1, res=True))
    out.append(_case("conv1d", "1x1 64-row tiles below the rule", b_small, 30, taps=1, relu_in=1))
    out.append(_case("conv1d", "k3 128-row tiles", b_big, 30, relu_out=1))
    out.append(_case("conv1d", "k4 s2 Cin=135 128-row tiles", -(-m_big // 15), 30, Cin=135, taps=4, s=2, off=-1))
    out += [
        _case("conv1d", "split ks=8", 2, 15),
        _case("conv1d", "split capped by total/8", 2, 15, taps=1),
        _case("conv1d", "split ws of two slabs", 2, 15, ws=2),
        _case("conv1d", "split ws of 1.5 slabs", 2, 15, ws=1.5),
        _case("conv1d", "split total=9", 2, 15, Cin=135, taps=1),
    ]
    # ---- qpg_convt_f32 / qpg_convt_pair_f32: per layer shape both sides of the small / generic rule and the smallest M of
    # every block shape the small kernel takes on it
    for layer in CONVT_LAYERS:
        probe = _convt_layer_case(layer, "", 1)
        lim = 1
        while convt_plan(lim, probe["taps"], probe["Cin_pad"], probe["Cout_pad"], probe["nz"], 0, n_cu)[0] == "small":
            lim += 64 if lim > 1 else 63                 # (the rule moves at multiples of 64 only)
        m_hi = lim - 63                                  # the smallest generic M; m_hi - 1 the largest small one
        dil = 3 if layer == "res3" else 1
        out.append(_convt_layer_case(layer, "largest small", m_hi - 1, dil=dil))
        out.append(_convt_layer_case(layer, "smallest generic", m_hi, dil=dil))
        seen = set()
        for M in range(1, m_hi):
            v = convt_plan(M, probe["taps"], probe["Cin_pad"], probe["Cout_pad"], probe["nz"], probe["relu_in"], n_cu)
            if v[3] not in seen:
                seen.add(v[3])
                out.append(_convt_layer_case(layer, "nq=%d" % v[3], M, dil=dil))
    out += [
        _case("convt", "M=65 k3 d3 relu Cx+4", 5, 13, dil=3, relu_in=1, relu_out=1, cx_extra=4),
        _case("convt", "M=21 1x1 res", 3, 7, taps=1, res=True),
        _case("convt", "T=1 k3", 3, 1),
        _case("convt", "T=8 d9 relu", 3, 8, dil=9, relu_in=1, relu_out=1),
        _case("convt", "k4 s2 Cin=135 Cx+4", 3, 26, Cin=135, taps=4, s=2, off=-1, cx_extra=4),
        _case("convt", "Cout=135 M=70", 2, 35, Cout=135),
        _case("convt", "k2 parity 1", 2, 9, taps=2, off=0, out_stride=2, out_offset=1),
        _case("pair", "up T=1", 3, 1, taps=2, out_stride=2, nz=2),
        _case("pair", "up M=65", 5, 13, taps=2, out_stride=2, nz=2),
    ]
    # ---- qpg_resblock_f32
    for B, T, dil in [(2, 30, 9), (3, 50, 3), (1, 64, 1), (7, 120, 9), (1, 3, 1), (3, 8, 9), (7, 9, 3), (4, 16, 3),
                      (5, 13, 3)]:
        out.append(_case("res", "B=%d T=%d d%d" % (B, T, dil), B, T, dil=dil, relu_in=1, relu_out=1, res=True))
    # ---- qpg_conv16_f32 (Cin: the real channels; the kernel sees them padded to a multiple of 8)
    out += [
        _case("conv16", "M=1", 1, 1, dil=3),
        _case("conv16", "M=127", 1, 127, dil=3, relu_in=1, relu_out=1),
        _case("conv16", "M=128", 4, 32, dil=3, res=True),
        _case("conv16", "M=129", 3, 43, dil=3, relu_in=1, relu_out=1, res=True),
        _case("conv16", "k4 s2 Cin=135", 2, 24, Cin=135, taps=4, s=2, off=-1),
        _case("conv16", "1x1 res Cx+8", 5, 13, taps=1, res=True, cx_extra=8),
        _case("conv16", "Cout=135", 1, 70, Cout=135),
        _case("conv16", "k4 s2", 2, 50, taps=4, s=2, off=-1),
        _case("conv16", "k2 parity 0", 2, 9, taps=2, off=-1, out_stride=2, out_offset=0),
        _case("conv16", "k2 parity 1", 2, 9, taps=2, off=0, out_stride=2, out_offset=1),
        _case("conv16", "T=8 d9 relu", 3, 8, dil=9, relu_in=1, relu_out=1),
        _case("conv16", "one slice", 2, 40, Cin=32, Cout=128, taps=1),
        _case("conv16", "two slices", 2, 40, Cin=64, Cout=128, taps=1),
        _case("conv16", "several blocks d9", 7, 120, dil=9, relu_in=1, relu_out=1),
    ]
    return out


def variant_of(c, n_cu):
    """The kernel variant a case runs on a device of n_cu CUs, as the restated rules name it."""
    k = c["kernel"]
    if k == "conv1d":
        return ("conv1d",) + conv1d_variant(c, n_cu)
    if k in ("convt", "pair"):
        return ("convt",) + convt_variant(c, n_cu)
    return (k,)


def chains_of(c, n_cu):
    k = c["kernel"]
    if k == "conv1d":
        return conv1d_chains(c["taps"], c["Cin_pad"], conv1d_variant(c, n_cu)[3])
    if k in ("convt", "pair"):
        return convt_chains(convt_variant(c, n_cu), c["taps"], c["Cin_pad"])
    raise ValueError(k)


def reachable(n_cu):
    """What the production model's layer shapes can reach under the restated rules, B * T from 1 past every threshold:
    conv1d -> (set of (MT, VEC), set of vec_out, set of ks classes); convt -> set of plans.  conv1d as the model calls
    it: aligned tensors, a workspace of 8 x 2048 x 512 floats (VQ_SPLITK_ROWS, csrc/qpg_vqvae.hip:500,523)."""
    ms = sorted(set(range(1, 2200)) | {64 * k + d for k in range(1, 2 * n_cu + 40) for d in (-1, 0, 1)})
    mtvec, vout, ksc, tplans = set(), set(), set(), set()
    for name, taps, cin, cout, s, ri, ro, res in LAYERS:
        cin_pad, cout_pad = pad(cin, 16), pad(cout, 128)
        for M in ms:
            p = conv1d_plan(M, cin, cin_pad, cout, cout_pad, taps, True, True, 8 * 2048 * 512, n_cu)
            mtvec.add(p[:2])
            vout.add(p[2])
            ksc.add(ks_class(p[3]))
            tplans.add(convt_plan(M, taps, cin_pad, cout_pad, 2 if name == "up" else 1, ri, n_cu))
    return mtvec, vout, ksc, tplans


def hit(case_list, n_cu):
    mtvec, vout, ksc, tplans = set(), set(), set(), set()
    for c in case_list:
        v = variant_of(c, n_cu)
        if v[0] == "conv1d":
            mtvec.add(v[1:3])
            vout.add(v[3])
            ksc.add(ks_class(v[4]))
        elif v[0] == "convt":
            tplans.add(v[1:])
    return mtvec, vout, ksc, tplans


# ----------------------------------------------------------------------------------------------------------------
# inputs and planted faults
# ----------------------------------------------------------------------------------------------------------------
def make_inputs(c):
    """x (B, T_in, Cin), w [taps][Cin][Cout], bias (Cout,), residual (B, T_y, Cout) or None - f32 CPU tensors, both signs
    everywhere.  conv16: a loud and a quiet frame (the quiet one's l planes are f16 subnormals).  res: (w1, b1, w2, b2)
    in place of (w, bias).  pair: w is the ConvTranspose1d weight's two halves, see pair_halves."""
    g = torch.Generator().manual_seed(c["seed"])
    B, T_in, Cin, Cout, taps = c["B"], c["T_in"], c["Cin"], c["Cout"], c["taps"]
    x = torch.randn((B, T_in, Cin), generator=g)
    if c["kernel"] == "conv16" and T_in > 5:
        x[0, 3] *= 40.0
        x[0, 5] *= 1e-3
    if c["kernel"] == "res":
        w1 = torch.randn((3, 512, 512), generator=g) * 1.4 / math.sqrt(1536)
        w2 = torch.randn((1, 512, 512), generator=g) * 0.5 / math.sqrt(512)
        b1, b2 = torch.randn((512,), generator=g) * 0.05, torch.randn((512,), generator=g) * 0.05
        return x, (w1, w2), (b1, b2), None
    if c["kernel"] == "pair":
        W = torch.randn((Cin, Cout, 4), generator=g) / math.sqrt(2 * Cin)      # ConvTranspose1d weight [Cin][Cout][k]
        bias = torch.randn((Cout,), generator=g) * 0.1
        return x, W, bias, None
    w = torch.randn((taps, Cin, Cout), generator=g) / math.sqrt(taps * Cin)
    bias = torch.randn((Cout,), generator=g) * 0.1
    res = torch.randn((B, c["T_y"], Cout), generator=g) if c["res"] else None
    return x, w, bias, res


def pair_halves(c, W):
    """ConvTranspose1d(k4, s2, p1) as two 2-tap convolutions (encdec.py:112-115): y[2m] = x[m-1].W3 + x[m].W1,
    y[2m+1] = x[m].W2 + x[m+1].W0 -> [(w [2][Cin][Cout], single-convolution case)] for the even and the odd frames."""
    we = torch.stack((W[:, :, 3], W[:, :, 1]))
    wo = torch.stack((W[:, :, 2], W[:, :, 0]))
    return [(we, dict(c, kernel="convt", off=-1, out_offset=0)), (wo, dict(c, kernel="convt", off=0, out_offset=1))]


def pair_ref_torch(x, W, bias):
    """torch's own conv_transpose1d in f64, channels-last."""
    y = torch.nn.functional.conv_transpose1d(x.double().transpose(1, 2), W.double(), bias.double(), stride=2, padding=1)
    return y.transpose(1, 2).contiguous()


def sample_rows(c):
    """Output positions the CPU test plants faults at: all of a short case; the first and last 96 and the first batch
    boundary's neighbourhood of a long one (a fault rejected there is rejected)."""
    M, T = c["M"], c["T_out"]
    if M <= 400:
        return torch.arange(M)
    r = set(range(96)) | set(range(M - 96, M)) | set(range(max(T - 12, 0), min(T + 12, M)))
    return torch.tensor(sorted(r))


def live_tap(c):
    """A tap that reads a real row at some output position (T < dil: only the centre one does)."""
    for tap in range(c["taps"]):
        for t in (0, c["T_out"] - 1, c["T_out"] // 2):
            if 0 <= t * c["s"] + c["off"] + tap * c["dil"] < c["T_in"]:
                return tap
    raise AssertionError("no live tap")


def faults_of(c, n_cu):
    """The planted faults that exist at a case: (label, fault) with fault as conv_eval takes it."""
    K = c["taps"] * c["Cin_pad"]
    tap = live_tap(c)
    f = [("one tap dropped", ("drop_tap", tap)), ("a tap shifted by one position", ("shift_tap", tap)),
         ("halo row from the neighbouring batch item", ("halo", None)),
         ("last 16-channel K slice dropped", ("drop_k", (K - 16, K))), ("bias doubled", ("bias2", None))]
    if c["relu_in"]:
        f.append(("relu_in omitted", ("no_relu_in", None)))
    if c["res"]:
        f.append(("residual omitted", ("no_res", None)))
    if c["out_stride"] == 2:
        f.append(("the other output parity written", ("parity", None)))
    k = c["kernel"]
    if k == "conv1d":
        ks = conv1d_variant(c, n_cu)[3]
        if ks > 1:
            per = -(-(K // 16) // ks) * 16
            f.append(("one split partial dropped", ("drop_k", (0, per))))
    if k == "convt" and convt_variant(c, n_cu)[0] == "small":
        f.append(("one split partial dropped", ("drop_k", (0, -(-(K // 16) // 8) * 16))))
    if k == "conv16":
        f.append(("the l.h' term dropped", ("drop_lh", None)))
    return f
