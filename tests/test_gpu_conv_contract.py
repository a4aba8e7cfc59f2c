"""The VQ-VAE's forward kernels - qpg_conv1d_f32, qpg_convt_f32, qpg_convt_pair_f32, qpg_resblock_f32, qpg_conv16_f32,
qpg_vq_argmin_f32, qpg_vq_gather_f32 - each called directly and held to the contract of tests/conv_ref.py: the f64
definition, the a-priori bound of the kernel variant the restated launch rule names for this device's CU count, at the
shapes where the kernels change path (tests/test_conv_contract_cpu.py shows the bounds reject planted faults there).

Every input lies inside a larger buffer of NaN rows (and NaN columns where the contract allows a wider pitch), every
output between sentinel rows that must come back untouched; with out_stride = 2 the other parity keeps its sentinel.
The largest err / bound per kernel variant and the variants run are printed at the end of the module (-s)."""
import numpy as np
import pytest

from tests import conv_ref as R

pytestmark = pytest.mark.gpu

G = 4                      # guard rows on either side (4 rows of 135 floats keep the 16-byte alignment)
RATIOS = {}                # variant -> largest err / bound
SPLITS = {}                # case -> split count read back from the workspace
NAMES = {k: [c["name"] for c in R.cases(256) if c["kernel"] == k] for k in ("conv1d", "convt", "pair", "res", "conv16")}


def _note(variant, r):
    RATIOS[variant] = max(RATIOS.get(variant, 0.0), r)


@pytest.fixture(scope="module")
def dev():
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    d = torch.device("cuda:0")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    table = R.cases(n_cu)
    by_name = {(c["kernel"], c["name"]): c for c in table}
    yield dict(dev=d, n_cu=n_cu, table=table, case=lambda k, n: by_name[(k, n)])
    print("\nn_cu %d; largest err / bound per kernel variant:" % n_cu)
    for v, r in sorted(RATIOS.items(), key=lambda kv: str(kv[0])):
        print("  %-60s %.3g" % (v, r))
    print("split counts read back from the workspace: %s" % sorted(SPLITS.items()))


# ----------------------------------------------------------------------------------------------------------------
# guarded buffers
# ----------------------------------------------------------------------------------------------------------------
def _guarded_in(x, pitch, nan_from, mis=False):
    """x (B, T, C) f32 CPU -> device view (B, T, pitch) in the middle of a NaN-filled buffer with G rows of NaN on either
    side; columns [C, nan_from) zero (channel padding the kernel reads), [nan_from, pitch) NaN (never read).  mis: the
    view starts one float off 16-byte alignment."""
    import torch
    B, T, C = x.shape
    n = (B * T + 2 * G) * pitch
    buf = torch.full((n + 4,), float("nan"), dtype=torch.float32, device="cuda:0")
    v = buf[1:n + 1] if mis else buf[:n]
    mid = v[G * pitch:(G + B * T) * pitch].view(B, T, pitch)
    mid[..., :C] = x.to("cuda:0")
    mid[..., C:nan_from] = 0.0
    assert (mid.data_ptr() % 16 == 0) != bool(mis)
    return mid


def _guarded_out(B, T_y, C, mis=False, init=None):
    """(whole buffer view (B * T_y + 2 G, C), the output view (B, T_y, C)): everything the sentinel (or `init` in the
    middle: a residual that lives in guarded memory too)."""
    import torch
    n = (B * T_y + 2 * G) * C
    buf = torch.full((n + 4,), R.SENTINEL, dtype=torch.float32, device="cuda:0")
    v = (buf[1:n + 1] if mis else buf[:n]).view(B * T_y + 2 * G, C)
    mid = v[G:G + B * T_y].view(B, T_y, C)
    if init is not None:
        mid.copy_(init)
    assert (mid.data_ptr() % 16 == 0) != bool(mis)
    return v, mid


def _guards_intact(whole, what):
    assert bool((whole[:G] == R.SENTINEL).all()) and bool((whole[-G:] == R.SENTINEL).all()), what + ": guard rows written"


def _written_rows(c, y):
    """The rows of y (B, T_y, C) the launch owns; asserts the other parity kept its sentinel."""
    got = y[:, c["out_offset"]::c["out_stride"]][:, :c["T_out"]]
    if c["out_stride"] == 2:
        other = y[:, 1 - c["out_offset"]::2]
        assert bool((other == R.SENTINEL).all()), c["name"] + ": the other output parity was written"
    return got


def _check(variant, c, got, ref, bound, g):
    r = R.bound_ratio(got.cpu(), ref, bound, g)
    _note(variant, r)
    print("%s %s (M=%d): err / bound %.3g" % (variant, c["name"], c["M"], r))
    assert r <= 1.0, "%s %s: err / bound = %.3g" % (variant, c["name"], r)


def _bias_dev(bias, cout_pad):
    import torch
    bp = torch.zeros((cout_pad,), device="cuda:0")
    bp[:bias.numel()] = bias.to("cuda:0")
    return bp


# ----------------------------------------------------------------------------------------------------------------
# qpg_conv1d_f32
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES["conv1d"])
def test_conv1d(dev, name):
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.vqvae import _Conv
    c, n_cu = dev["case"]("conv1d", name), dev["n_cu"]
    x, w, bias, res = R.make_inputs(c)
    conv = _Conv(w, bias, dev["dev"])                                   # [tap][Cin_pad][Cout_pad], bias [Cout_pad]
    assert (conv.cin_pad, conv.cout_pad) == (c["Cin_pad"], c["Cout_pad"])
    B, T_in, Cin, Cout = c["B"], c["T_in"], c["Cin"], c["Cout"]
    xd = _guarded_in(x, Cin, Cin, mis=c["mis"] == "x")
    ywhole, y = _guarded_out(B, c["T_y"], Cout, mis=c["mis"] == "y")
    rwhole, rd = _guarded_out(B, c["T_y"], Cout, mis=c["mis"] == "res", init=res) if res is not None else (None, None)
    wsf = R.ws_floats_of(c)
    ws = torch.full((wsf,), float("nan"), device="cuda:0") if wsf is not None else None
    plan = R.conv1d_variant(c, n_cu)
    _lib.call("qpg_conv1d_f32", dev["dev"], xd, B, T_in, Cin, conv.w, conv.b, c["taps"], c["Cin_pad"], Cout, c["Cout_pad"],
              c["s"], c["off"], c["dil"], c["T_out"], c["out_stride"], c["out_offset"], c["T_y"], rd, c["relu_in"],
              c["relu_out"], y, ws, wsf or 0)
    torch.cuda.synchronize()
    # the split count that RAN: split z writes its whole slab ws[z][M][Cout_pad], the last entry included
    ks_ran = 1
    if ws is not None:
        slab = c["M"] * c["Cout_pad"]
        n_slab = wsf // slab
        last = ws[slab - 1::slab][:n_slab]
        written = int((~torch.isnan(last)).sum())
        assert bool((~torch.isnan(last[:written])).all())
        ks_ran = max(written, 1)
    SPLITS[name] = ks_ran
    assert ks_ran == plan[3], "split count %d, conv_launch's rule says %d" % (ks_ran, plan[3])
    _guards_intact(ywhole, name)
    if rwhole is not None:
        _guards_intact(rwhole, name + " residual")
        assert torch.equal(rd.cpu(), res)
    ref, absref = R.conv_ref(x, w, bias, R.geom_of(c), c["relu_in"], c["relu_out"], res)
    _check(("conv1d",) + plan, c, _written_rows(c, y), ref, absref, R.gamma(*R.chains_of(c, n_cu)))


# ----------------------------------------------------------------------------------------------------------------
# qpg_convt_f32 / qpg_convt_pair_f32
# ----------------------------------------------------------------------------------------------------------------
def _convt_call(dev, c, xd, w, bias_dev, rd, y):
    from qpgesture_amd import _lib
    from qpgesture_amd.vqvae import tpack
    wt = tpack(w.to(dev["dev"]), c["Cin_pad"], 128)
    _lib.call("qpg_convt_f32", dev["dev"], xd, c["B"], c["T_in"], xd.shape[-1], wt, bias_dev, c["taps"], c["Cin_pad"],
              c["Cout"], c["Cout_pad"], c["s"], c["off"], c["dil"], c["T_out"], c["out_stride"], c["out_offset"], c["T_y"],
              rd, c["relu_in"], c["relu_out"], y)
    return wt


@pytest.mark.parametrize("name", NAMES["convt"])
def test_convt(dev, name):
    import torch
    c, n_cu = dev["case"]("convt", name), dev["n_cu"]
    x, w, bias, res = R.make_inputs(c)
    xd = _guarded_in(x, c["Cin_pad"] + c["cx_extra"], c["Cin_pad"])
    ywhole, y = _guarded_out(c["B"], c["T_y"], c["Cout"])
    rwhole, rd = _guarded_out(c["B"], c["T_y"], c["Cout"], init=res) if res is not None else (None, None)
    _convt_call(dev, c, xd, w, _bias_dev(bias, c["Cout_pad"]), rd, y)
    torch.cuda.synchronize()
    _guards_intact(ywhole, name)
    ref, absref = R.conv_ref(x, w, bias, R.geom_of(c), c["relu_in"], c["relu_out"], res)
    plan = R.convt_variant(c, n_cu)
    _check(("convt",) + plan, c, _written_rows(c, y), ref, absref, R.gamma(*R.chains_of(c, n_cu)))


@pytest.mark.parametrize("name", NAMES["pair"])
def test_convt_pair(dev, name):
    """The pair against torch's conv_transpose1d in f64 and against two single launches: bit for bit where convt_launch
    names the same kernel for the pair (twice the blocks) and for one half."""
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.vqvae import tpack
    c, n_cu = dev["case"]("pair", name), dev["n_cu"]
    x, W, bias, _ = R.make_inputs(c)
    B, T = c["B"], c["T_in"]
    xd = _guarded_in(x, 512, 512)
    bd = _bias_dev(bias, 512)
    (we, he), (wo, ho) = R.pair_halves(c, W)
    y1whole, y1 = _guarded_out(B, 2 * T, 512)
    wte, wto = tpack(we.to(dev["dev"]), 512, 128), tpack(wo.to(dev["dev"]), 512, 128)
    _lib.call("qpg_convt_pair_f32", dev["dev"], xd, B, T, 512, wte, bd, -1, 0, wto, bd, 0, 1, 2, 512, 512, 512, 1, 1, T, 2,
              2 * T, y1)
    y2whole, y2 = _guarded_out(B, 2 * T, 512)
    for wh, h in ((we, he), (wo, ho)):
        _convt_call(dev, dict(h, nz=1), xd, wh, bd, None, y2)
    torch.cuda.synchronize()
    _guards_intact(y1whole, name)
    _guards_intact(y2whole, name)
    plan2, plan1 = R.convt_variant(c, n_cu), R.convt_variant(dict(c, nz=1), n_cu)
    if plan1 == plan2:
        assert torch.equal(y1, y2), "pair != two single launches of the same kernel"
    want = R.pair_ref_torch(x, W, bias)
    absref = torch.zeros_like(want)
    for wh, h in ((we, he), (wo, ho)):
        ref_h, abs_h = R.conv_ref(x, wh, bias, R.geom_of(h))
        assert float((ref_h - want[:, h["out_offset"]::2]).abs().max()) < 1e-11     # the halves ARE the transposed convolution
        absref[:, h["out_offset"]::2] = abs_h
    _check(("convt",) + plan2, c, y1, want, absref, R.gamma(*R.convt_chains(plan2, 2, 512)))
    _check(("convt",) + plan1, dict(c, name=name + " (two launches)"), y2, want, absref,
           R.gamma(*R.convt_chains(plan1, 2, 512)))


# ----------------------------------------------------------------------------------------------------------------
# qpg_resblock_f32
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES["res"])
def test_resblock(dev, name):
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.vqvae import tpack
    c = dev["case"]("res", name)
    x, (w1, w2), (b1, b2), _ = R.make_inputs(c)
    B, T, dil, d = c["B"], c["T_in"], c["dil"], dev["dev"]
    pack = torch.cat((tpack(w1.to(d), 512, 512), tpack(w2.to(d), 512, 128))).contiguous()
    assert pack.numel() == 128 * 8192
    xd = _guarded_in(x, 512, 512)
    ywhole, y = _guarded_out(B, T, 512)
    hwhole, h = _guarded_out(B, T, 512)
    y2whole, y2 = _guarded_out(B, T, 512)
    _lib.call("qpg_resblock_f32", d, xd, B, T, dil, pack, b1.to(d), b2.to(d), y, h)
    _lib.call("qpg_resblock_f32", d, xd, B, T, dil, pack, b1.to(d), b2.to(d), y2, None)
    torch.cuda.synchronize()
    for whole in (ywhole, hwhole, y2whole):
        _guards_intact(whole, name)
    assert torch.equal(y, y2), "hidden=None changes the block's output"
    h_ref, y_ref, ah, ay = R.resblock_ref(x, w1, b1, w2, b2, dil)
    _check(("res", "hidden"), c, h, h_ref, ah, R.gamma(*R.RES_CHAINS_H))
    _check(("res", "y"), c, y, y_ref, ay, R.gamma(*R.RES_CHAINS_Y))


# ----------------------------------------------------------------------------------------------------------------
# qpg_conv16_f32
# ----------------------------------------------------------------------------------------------------------------
def _conv16_image(d, w, cin8):
    import torch
    from qpgesture_amd import _lib
    taps, cin, cout = w.shape
    cin_pw, cout_pw = R.pad(cin, 16), R.pad(cout, 128)
    wp = torch.zeros((taps, cin_pw, cout_pw), device=d)
    wp[:, :cin, :cout] = w.to(d)
    nb = int(_lib.load().qpg_conv16_image_bytes(taps, cin8, cout))
    img = torch.empty((nb,), dtype=torch.uint8, device=d)
    _lib.call("qpg_conv16_pack_weights", d, wp, taps, cin8, cin_pw, cout, cout_pw, img, nb)
    w_exp = int(img[nb - 64:nb - 60].view(torch.int32).item())
    assert w_exp == R._w_exp(w)
    return img, w_exp


def _conv16_call(d, c, xd, cin8, img, w_exp, bd, rd, y, st):
    from qpgesture_amd import _lib
    _lib.call("qpg_conv16_f32", d, xd, c["B"], c["T_in"], xd.shape[-1], cin8, img, w_exp, bd, c["taps"], c["Cout"], c["s"],
              c["off"], c["dil"], c["T_out"], c["out_stride"], c["out_offset"], c["T_y"], rd, c["relu_in"], c["relu_out"], y, st)


@pytest.mark.parametrize("name", NAMES["conv16"])
def test_conv16(dev, name):
    import torch
    from qpgesture_amd import _lib
    c, d = dev["case"]("conv16", name), dev["dev"]
    x, w, bias, res = R.make_inputs(c)
    cin8 = R.pad(c["Cin"], 8)
    img, w_exp = _conv16_image(d, w, cin8)
    xd = _guarded_in(x, cin8 + c["cx_extra"], cin8)
    bd = _bias_dev(bias, c["Cout_pad"])
    rwhole, rd = _guarded_out(c["B"], c["T_y"], c["Cout"], init=res) if res is not None else (None, None)
    st = torch.zeros((1,), dtype=torch.int32, device=d)
    ywhole, y = _guarded_out(c["B"], c["T_y"], c["Cout"])
    _conv16_call(d, c, xd, cin8, img, w_exp, bd, rd, y, st)
    y2whole, y2 = _guarded_out(c["B"], c["T_y"], c["Cout"])
    _conv16_call(d, c, xd, cin8, img, _lib.QPG_CONV16_WEXP_FROM_IMAGE, bd, rd, y2, st)
    torch.cuda.synchronize()
    _guards_intact(ywhole, name)
    _guards_intact(y2whole, name)
    assert int(st.item()) == 0, "status set on clean data"
    assert torch.equal(y, y2), "the exponent read from the image gives another result than the host's"
    ref, absref = R.conv_ref(x, w, bias, R.geom_of(c), c["relu_in"], c["relu_out"], res)
    bound = R.conv16_bound(absref, w, x.shape, R.geom_of(c), cin8)
    _check(("conv16",), c, _written_rows(c, y), ref, bound, 1.0)


def test_conv16_status_bit(dev):
    """status |= 1 exactly when an activation the launch USES leaves the f16 range: not for a row only the clamped loads
    of padded taps touch, not for a column past Cin, not for a negative value the input ReLU removes."""
    import torch
    d = dev["dev"]
    # k1 s2 off -3 over 20 rows: positions read rows 2 t - 3 = -3, -1, 1, .., 15; row 0 is where out-of-range taps clamp
    # to, and no position's tap
    c = R._case("conv16", "status", 2, 20, Cin=64, Cout=128, taps=1, s=2, off=-3)
    c.update(T_out=10, T_y=10, M=20)
    x, w, bias, _ = R.make_inputs(c)
    img, w_exp = _conv16_image(d, w, 64)
    bd = _bias_dev(bias, 128)

    def run(edit, relu_in=0, extra=8):
        xe = x.clone()
        xd = _guarded_in(xe, 64 + extra, 64)
        edit(xd)
        st = torch.zeros((1,), dtype=torch.int32, device=d)
        whole, y = _guarded_out(2, 10, 128)
        _conv16_call(d, dict(c, relu_in=relu_in), xd, 64, img, w_exp, bd, None, y, st)
        torch.cuda.synchronize()
        _guards_intact(whole, "status")
        return int(st.item()), y.clone()

    def put(r, col, v):
        def f(xd):
            xd[1, r, col] = v
        return f

    s0, y0 = run(lambda xd: None)
    assert s0 == 0
    ref, absref = R.conv_ref(x, w, bias, R.geom_of(c))
    _check(("conv16",), c, y0, ref, R.conv16_bound(absref, w, x.shape, R.geom_of(c), 64), 1.0)
    assert run(put(1, 5, 1e5))[0] == 1                                   # a live position
    assert run(put(1, 5, float("nan")))[0] == 1
    assert run(put(1, 5, float("inf")))[0] == 1
    s, y = run(put(0, 5, 1e5))                                           # the clamp target of the padded taps: masked
    assert s == 0 and torch.equal(y, y0)
    s, y = run(put(2, 5, 1e5))                                           # an even row: never read
    assert s == 0 and torch.equal(y, y0)
    s, y = run(put(1, 64 + 2, 1e5))                                      # a column past Cin
    assert s == 0 and torch.equal(y, y0)
    assert run(put(1, 5, -1e5), relu_in=1)[0] == 0                       # removed by the input ReLU
    assert run(put(1, 5, -1e5), relu_in=0)[0] == 1


# ----------------------------------------------------------------------------------------------------------------
# qpg_vq_argmin_f32 / qpg_vq_gather_f32
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,E,K,ties", R.ARGMIN_SETS)
def test_vq_argmin(dev, R_, E, K, ties):
    import torch
    from qpgesture_amd import _lib
    d = dev["dev"]
    z, dot, kk = R.argmin_inputs(R_, E, K, seed=R_ + E + K, ties=ties)
    d64, dmin, dsec, ids_ref, b = R.argmin_ref(z, dot, kk)
    zd = _guarded_in(torch.from_numpy(z)[None], E, E)
    dd = _guarded_in(torch.from_numpy(dot)[None], K, K)
    kd = torch.from_numpy(kk).to(d)
    ids = torch.full((R_ + 2,), -77, dtype=torch.int64, device=d)
    owhole, o = _guarded_out(1, 2, R_)                                   # row 0: dmin, row 1: dsecond
    _lib.call("qpg_vq_argmin_f32", d, zd, dd, kd, R_, E, K, ids[1:R_ + 1], o[0, 0], o[0, 1])
    torch.cuda.synchronize()
    _guards_intact(owhole, "argmin")
    assert int(ids[0]) == -77 and int(ids[-1]) == -77
    got = ids[1:R_ + 1].cpu().numpy()
    gmin, gsec = o[0, 0].cpu().numpy().astype(np.float64), o[0, 1].cpu().numpy().astype(np.float64)
    assert ((got >= 0) & (got < K)).all()
    decided = (dsec - dmin) > 2 * b
    assert np.array_equal(got[decided], ids_ref[decided])
    assert (d64[np.arange(R_), got] - dmin <= 2 * b).all()
    r_min = float((np.abs(gmin - dmin) / b).max())
    _note(("argmin", "dmin"), r_min)
    assert r_min <= 1.0
    if K == 1:
        assert np.isposinf(gsec).all()
    else:
        r_sec = float((np.abs(gsec - dsec) / b).max())
        _note(("argmin", "dsecond"), r_sec)
        assert r_sec <= 1.0
    if ties:
        tied = np.arange(R_) % 3 != 2
        assert np.array_equal(got[tied], np.full(int(tied.sum()), min(ties[0]))), "not the lowest index among equal distances"
        assert np.array_equal(gsec[tied], gmin[tied]), "dsecond != dmin although the minimum occurs twice"
    print("argmin R=%d E=%d K=%d: %d of %d rows decided" % (R_, E, K, int(decided.sum()), R_))


def test_vq_gather(dev):
    import torch
    from qpgesture_amd import _lib
    d = dev["dev"]
    g = torch.Generator().manual_seed(4)
    K, E, R_ = 10, 8, 37
    k = torch.randn((K, E), generator=g)
    ids = torch.randint(0, K, (R_,), generator=g)
    kd, st = k.to(d), torch.zeros((1,), dtype=torch.int32, device=d)
    whole, out = _guarded_out(1, R_, E)
    _lib.call("qpg_vq_gather_f32", d, kd, ids.to(d), R_, E, K, out, st)
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and torch.equal(out[0].cpu(), k[ids])
    bad = ids.clone()
    bad[3], bad[20] = -1, K
    whole2, out2 = _guarded_out(1, R_, E)
    _lib.call("qpg_vq_gather_f32", d, kd, bad.to(d), R_, E, K, out2, st)
    torch.cuda.synchronize()
    want = k[bad.clamp(0, K - 1)]
    want[3], want[20] = k[0], k[0]
    assert int(st.item()) == 1 and torch.equal(out2[0].cpu(), want)
    _guards_intact(whole, "gather")
    _guards_intact(whole2, "gather")


def test_duplicated_codebook_rows_through_the_model():
    """Two equal codebook rows: quantise and the whole-network encode return the LOWER id and a margin of exactly 0 on
    latents equal to that row (the two columns of the x . k^T GEMM and the two norms are the same operations on the same
    numbers)."""
    import torch
    from qpgesture_amd import synth
    from qpgesture_amd.vqvae import VQVAE
    sd = synth.make_vqvae_state_dict(7)
    key = next(n for n in sd if n.endswith("bottleneck.level_blocks.0.k"))      # (with or without the "module." prefix)
    m = VQVAE(None, input_dim=135, device="cuda:0").load_state_dict(sd)
    x = torch.randn((2, 64, 135), generator=torch.Generator().manual_seed(9)).cuda()
    _, lat = m.encode_fused(x, return_latent=True)
    k = torch.as_tensor(np.array(sd[key], dtype=np.float32, copy=True))
    lo, hi, lo2, hi2 = 5, 300, 70, 71                                    # (c, c + 295): other lanes; (c, c + 1): neighbours
    k[lo] = k[hi] = lat[0, 3].cpu()
    k[lo2] = k[hi2] = lat[1, 6].cpu()
    sd2 = dict(sd)
    sd2[key] = k.numpy() if isinstance(sd[key], np.ndarray) else k
    m2 = VQVAE(None, input_dim=135, device="cuda:0").load_state_dict(sd2)
    z = k[[lo, hi, lo2, hi2, lo]].view(1, 5, -1).cuda()
    ids, margin = m2.quantise(z, return_margin=True)
    assert ids.cpu().tolist() == [[lo, lo, lo2, lo2, lo]] and margin.cpu().tolist() == [[0.0] * 5]
    ids2, lat2, mar2 = m2.encode_fused(x, return_latent=True, return_margin=True)
    assert torch.equal(lat2, lat)
    assert int(ids2[0, 3]) == lo and float(mar2[0, 3]) == 0.0
    assert int(ids2[1, 6]) == lo2 and float(mar2[1, 6]) == 0.0


def test_variants_run_are_the_reachable_set(dev):
    """The case table of THIS device's CU count names every kernel variant the production shapes reach on it (and the
    variants the cases above recorded are those)."""
    n_cu = dev["n_cu"]
    want, got = R.reachable(n_cu), R.hit(dev["table"], n_cu)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3]
    ran = {v for v in RATIOS if v[0] in ("conv1d", "convt")}
    named = {R.variant_of(c, n_cu) for c in dev["table"] if c["kernel"] in ("conv1d", "convt", "pair")}
    named |= {("convt",) + R.convt_variant(dict(c, nz=1), n_cu) for c in dev["table"] if c["kernel"] == "pair"}
    if ran:                                                              # (the whole module ran)
        assert ran <= named
    print("conv1d (MT, VEC) %s, vec_out %s, ks %s" % (sorted(got[0]), sorted(got[1]), sorted(got[2], key=str)))
    print("convt plans: %s" % sorted(got[3], key=str))
