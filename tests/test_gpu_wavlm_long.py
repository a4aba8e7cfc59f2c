"""Whole-recording, ragged and layer-tap WavLM extraction on the device.

The kernel: qpg_wavlm_attention_tiled_f32, called directly, against the f64 value and the ENTRYWISE bound of
tests/wavlm_long_ref.py (derivation there; tests/test_wavlm_long_cpu.py shows that an f32 evaluation in the kernel's order
is inside it and six mistakes are outside) on the shared table TILED_CASES - every T at, one below and one above the 128
queries of a block and the 64 keys of a tile, two key tiles plus one, the old kernel's 256-frame cap and beyond, every
mask kind - with NaN at the masked keys of k and v, NaN behind every input and a sentinel behind the output.  Its
invariants are held bit for bit.

The model: the reference's f64 results (tests/golden/wavlm_long_*.npz, wavlm_ragged.npz, wavlm_layers.npz) within 8 x the
fixture's e32, the project's end-to-end criterion; the masked model launch by launch against each stage's bound on the
device's own inputs; the routing between the two attention kernels; wav2wavlm and the --whole CLI."""
import numpy as np
import pytest
import torch

from qpgesture_amd import _lib, synth
from qpgesture_amd import wavlm as W
from tests import wavlm_long_ref as L
from tests import wavlm_ref as R
from tests.test_wavlm_long_cpu import CFG, golden, ragged_audio, weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = R.SENTINEL
MARGIN = 8.0
NAN_TAIL = np.full(16, np.nan, np.float32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def dev_padded(a):
    return dev(np.concatenate([np.asarray(a, np.float32).ravel(), NAN_TAIL]))


def dev_mask(mk):
    return None if mk is None else torch.from_numpy(np.ascontiguousarray(mk, np.uint8)).to(DEV)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def held(name, got, val, bnd):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == val.shape, (name, got.shape, val.shape)
    r = R.ratio(got, val, bnd)
    print("WAVLMLONG %s: err/bound %.3f" % (name, r))
    assert r <= 1.0, (name, r)


def run_tiled(c, B=None, qkv=None, gate=None, relb=None, mask="case", margin=8):
    """The case's call -> [B][T][D] device result; the margin of `margin` floats on either side of it must keep its
    sentinel."""
    B = c["B"] if B is None else B
    T, H = c["T"], c["H"]
    n = B * T * H * 64
    qkv = dev_padded(np.concatenate([c["q"], c["k"], c["v"]], 2)) if qkv is None else qkv
    buf = torch.full((n + 2 * margin,), SENT, dtype=torch.float32, device=DEV)
    mk = dev_mask(c["key_mask"]) if isinstance(mask, str) else mask
    _lib.call("qpg_wavlm_attention_tiled_f32", DEV, qkv, dev_padded(c["gate"]) if gate is None else gate,
              dev_padded(c["relb"]) if relb is None else relb, mk, B, T, H, buf[margin:])
    assert bool((buf[:margin] == SENT).all()) and bool((buf[margin + n:] == SENT).all())
    return buf[margin:margin + n].view(B, T, H * 64)


# ---- the kernel against its bound -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,H,mk,kind", L.TILED_CASES)
def test_tiled_attention(T, B, H, mk, kind):
    c = L.tiled_case(T, B, H, mk, kind)
    if c["key_mask"] is not None:
        assert np.isnan(c["k"]).any() and np.isnan(c["v"]).any()
    if kind == "one hot":
        assert np.abs(c["gate"][..., None, :] * c["relb"][None, None]).max() > 100.0      # expf of a raw score overflows
    val, bnd = L.tiled_bound_of(c)
    held("tiled T=%d B=%d H=%d mask=%s %s" % (T, B, H, mk, kind), run_tiled(c), val, bnd)


# ---- invariants, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,mk", [(65, "none"), (300, "hole"), (257, "LK+1 valid")])
def test_tiled_does_not_depend_on_batch_or_head_position(T, mk):
    c = L.tiled_case(T, 3, 3, mk)
    full = run_tiled(c)
    assert bool(torch.isfinite(full).all())
    qkv = np.concatenate([c["q"], c["k"], c["v"]], 2)
    for b in range(3):
        alone = run_tiled(c, B=1, qkv=dev_padded(qkv[b]), gate=dev_padded(c["gate"][b]),
                          mask=None if c["key_mask"] is None else dev_mask(c["key_mask"][b:b + 1]))
        assert torch.equal(alone[0], full[b]), b
    perm = [2, 0, 1]
    cols = np.concatenate([np.arange(64) + 64 * h for h in perm])
    pc = dict(c, q=c["q"][:, :, cols], k=c["k"][:, :, cols], v=c["v"][:, :, cols], gate=c["gate"][:, :, perm],
              relb=c["relb"][:, perm])
    assert torch.equal(run_tiled(pc), full[:, :, torch.from_numpy(cols).to(DEV)])


@pytest.mark.parametrize("T,mk", [(129, "1 valid"), (300, "hole"), (300, "T-1 valid")])
def test_masked_keys_are_never_read_into_a_result(T, mk):
    """NaN, Inf and finite garbage at the masked keys of k and v give the same bits, and they are finite."""
    c = L.tiled_case(T, 3, 3, mk)
    dead = c["key_mask"].astype(bool)
    nan = run_tiled(c)
    assert bool(torch.isfinite(nan).all())
    rng = np.random.Generator(np.random.PCG64(7))
    for fill in (np.inf, -np.inf, 0.0, None):
        k, v = c["k"].copy(), c["v"].copy()
        k[dead] = rng.standard_normal((int(dead.sum()), k.shape[2])) * 50 if fill is None else fill
        v[dead] = rng.standard_normal((int(dead.sum()), v.shape[2])) * 50 if fill is None else fill
        assert torch.equal(run_tiled(dict(c, k=k, v=v)), nan), fill


@pytest.mark.parametrize("T", [17, 300])
def test_null_mask_equals_an_all_zero_mask(T):
    c = L.tiled_case(T, 3, 3, "none")
    assert torch.equal(run_tiled(c, mask=None), run_tiled(c, mask=dev_mask(np.zeros((3, T), np.uint8))))


def test_a_wide_margin_around_the_output_is_untouched():
    for T in (1, 127, 129, 300):
        run_tiled(L.tiled_case(T, 3, 3, "none"), margin=4096)


def test_tiled_refusals_leave_the_output_untouched():
    cap = _lib.QPG_WAVLM_MAX_FRAMES_LONG
    assert cap >= 32768 and cap == W.MAX_FRAMES_LONG and _lib.QPG_WAVLM_MAX_FRAMES == 256
    H = 1
    qkv = torch.zeros((8 * 3 * 64 + 4,), dtype=torch.float32, device=DEV)
    gate, relb = torch.ones((8, H), device=DEV), torch.zeros((15, H), device=DEV)
    o = torch.full((8 * 64,), SENT, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.Unsupported, match="%d frames" % (cap + 1)):       # nothing is launched: the sizes are not read
        _lib.call("qpg_wavlm_attention_tiled_f32", DEV, qkv, gate, relb, None, 1, cap + 1, H, o)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _lib.call("qpg_wavlm_attention_tiled_f32", DEV, qkv[1:], gate, relb, None, 1, 8, H, o)
    for B, Hh in ((0, 1), (65536, 1), (1, 0), (1, 65536)):
        with pytest.raises(RuntimeError, match="65535"):
            _lib.call("qpg_wavlm_attention_tiled_f32", DEV, qkv, gate, relb, None, B, 8, Hh, o)
    with pytest.raises(RuntimeError, match="T >= 1"):
        _lib.call("qpg_wavlm_attention_tiled_f32", DEV, qkv, gate, relb, None, 1, 0, H, o)
    torch.cuda.synchronize()
    assert bool((o == SENT).all())


@pytest.mark.parametrize("M,C", [(1, 1), (5, 64), (85, 3), (300, 128)])
def test_mask_rows(M, C):
    """qpg_wavlm_mask_rows_f32: the named rows become 0 (whatever they held, NaN included), every other float keeps its
    bits, the sentinel behind the last row stays."""
    rng = np.random.Generator(np.random.PCG64([61, M, C]))
    x = rng.standard_normal((M, C)).astype(np.float32)
    mk = (rng.uniform(size=M) < 0.4).astype(np.uint8)
    mk[M - 1] = 1
    x[mk.astype(bool), ::2] = np.nan
    buf = torch.cat([dev(x).ravel(), torch.full((8,), SENT, dtype=torch.float32, device=DEV)])
    _lib.call("qpg_wavlm_mask_rows_f32", DEV, buf, dev_mask(mk), M, C)
    want = np.where(mk.astype(bool)[:, None], np.float32(0), x)
    assert np.array_equal(_np(buf[:M * C]).reshape(M, C), want) and bool((buf[M * C:] == SENT).all())
    _lib.call("qpg_wavlm_mask_rows_f32", DEV, buf, dev_mask(mk), 0, C)                 # no rows: nothing launched
    with pytest.raises(RuntimeError, match="C >= 1"):
        _lib.call("qpg_wavlm_mask_rows_f32", DEV, buf, dev_mask(mk), M, 0)


# ---- the model ------------------------------------------------------------------------------------------------------
_models = {}


def model_of(seed, long_inputs):
    key = (seed, long_inputs)
    if key not in _models:
        _models[key] = W.WavLM(CFG, device=DEV, long_inputs=long_inputs).load_state_dict(weights(seed))
    return _models[key]


def within(name, got, want, e32):
    got = _np(got).astype(np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), name
    err = float(np.abs(got - want).max())
    print("WAVLMLONG %s: err %.3e e32 %.3e ratio %.2f" % (name, err, e32, err / e32))
    assert err <= MARGIN * e32, "%s: |device - f64| = %.3e > %g x e32 (%.3e)" % (name, err, MARGIN, e32)


@pytest.mark.parametrize("T", [324, 1031])
def test_long_fixture(T):
    g = golden("wavlm_long_%d" % T)
    wseed, aseed, B, n = (int(v) for v in g["meta"][:4])
    model = model_of(wseed, True)
    out, fm = model.extract_features(synth.make_wav(aseed, B, n))
    assert fm is None and out.shape == (1, T, CFG["encoder_embed_dim"]) and out.dtype == torch.float32 and out.is_cuda
    within("long T=%d" % T, out[:, torch.from_numpy(g["rows"]).to(DEV)], g["out"], float(g["e32"]))
    assert torch.equal(model.extract_features(synth.make_wav(aseed, B, n))[0], out)       # the workspace is reusable


def test_ragged_fixture():
    g = golden("wavlm_ragged")
    sd, wav, mask, _ = ragged_audio(g)
    for model in (model_of(int(g["meta"][0]), False), model_of(int(g["meta"][0]), True)):    # 99 frames: no opt-in needed
        out, fm = model.extract_features(wav, padding_mask=torch.from_numpy(mask))
        assert fm.dtype == torch.bool and fm.is_cuda and np.array_equal(_np(fm), g["frame_mask"])
        within("ragged, all rows", out, g["out"], float(g["e32"]))
    assert torch.equal(model.extract_features(wav, padding_mask=mask)[0], out)             # (a NumPy mask is taken too)
    # the masked result differs from the unmasked one on the VALID rows of the padded members
    plain = model.extract_features(wav)[0]
    assert float((plain[1, :62] - out[1, :62]).abs().max()) > 1e-3
    with pytest.raises(NotImplementedError, match="normalize_input"):
        W.WavLM(CFG, device=DEV, normalize_input=True).load_state_dict(sd).extract_features(wav, padding_mask=mask)


def test_layers_fixture():
    g = golden("wavlm_layers")
    sd, wav, _, _ = ragged_audio(g)
    model = model_of(int(g["meta"][0]), False)
    rows = torch.from_numpy(g["rows"]).to(DEV)
    for k in (1, 2):
        (feat, lr), fm = model.extract_features(wav, output_layer=k, ret_layer_results=True)
        assert fm is None and len(lr) == k + 1 and all(z is None for _, z in lr)
        within("output_layer=%d" % k, feat[:, rows], g["feat_%d" % k], float(g["e32_feat_%d" % k]))
        for i, (x, _) in enumerate(lr):
            assert x.shape == (99, 3, CFG["encoder_embed_dim"]) and x.is_contiguous()
            within("output_layer=%d layer result %d" % (k, i), x[rows], g["lr_%d_%d" % (k, i)],
                   float(g["e32_lr_%d_%d" % (k, i)]))
        assert torch.equal(lr[-1][0].transpose(0, 1), feat)
        assert len({x.data_ptr() for x, _ in lr} | {feat.data_ptr()}) == k + 2            # copies, not views of one buffer
        assert torch.equal(model.extract_features(wav, output_layer=k)[0], feat)
    last = model.extract_features(wav)[0]
    assert float((feat - last).abs().max()) > 0.1                     # output_layer = encoder_layers: no final LayerNorm
    (feat2, lr2), _ = model.extract_features(wav, ret_layer_results=True)
    assert lr2 == [] and torch.equal(feat2, last)                     # as in the reference: empty without output_layer
    conv = model.extract_features(wav, ret_conv=True)[0]
    within("ret_conv", conv[:, rows], g["conv"], float(g["e32_conv"]))
    with pytest.raises(NotImplementedError, match="mask"):
        model.extract_features(wav, mask=True)
    for k in (0, 3):
        with pytest.raises(ValueError, match="output_layer"):
            model.extract_features(wav, output_layer=k)


def test_masked_model_launch_by_launch():
    """The ragged batch (B = 3, T = 99, valid frames 99 / 62 / 22), two blocks: every launch's output against its f64 value
    and bound computed from the DEVICE's own input of that launch, as tests/test_gpu_wavlm_contract.py does for the
    unmasked model; the attention against attention_tiled_bound with the frame mask."""
    g = golden("wavlm_ragged")
    sd, wav, mask, _ = ragged_audio(g)
    cfg = dict(CFG)
    model = model_of(int(g["meta"][0]), False)
    taps = {}
    out = model._forward(wav, lambda stage, view: taps.__setitem__(stage, None if view is None else _np(view.clone())),
                         padding_mask=mask)
    assert torch.equal(model.extract_features(wav, padding_mask=mask)[0], out)            # the callbacks change nothing
    layers = model.conv_layers
    B, n = wav.shape
    fr = W.frames_of(n, layers)
    T, C = fr[-1], layers[0][0]
    D, F, H = cfg["encoder_embed_dim"], cfg["encoder_ffn_embed_dim"], cfg["encoder_attention_heads"]
    fm = g["frame_mask"]
    p = model.p
    seen = {"start"}

    def check(stage, val, bnd):
        seen.add(stage)
        held("masked " + stage, taps[stage], val, bnd)

    L0 = p["conv"][0]
    check("conv0", *R.conv0_bound(wav, _np(L0["w"]), _np(L0["b"]), layers[0][1], layers[0][2]))
    for i, (_, k, s) in enumerate(layers):
        Li = p["conv"][i]
        if i >= 1:
            prev = taps["conv%d_norm" % (i - 1)].reshape(B, -1)
            A = prev[:, (np.arange(fr[i]) * s * C)[:, None] + np.arange(k * C)[None, :]]
            check("conv%d" % i, *R.gemm_bound(A, _np(Li["w"]), _np(Li["b"])))
        check("conv%d_norm" % i, *R.layernorm_bound(taps["conv%d" % i], _np(Li["g"]), _np(Li["beta"]), 1))
    assert np.array_equal(taps["features"], taps["conv%d_norm" % (len(layers) - 1)])
    seen.add("features")
    check("front_norm", *R.layernorm_bound(taps["features"], _np(p["ln_g"]), _np(p["ln_b"])))
    check("front_end", *R.gemm_bound(taps["front_norm"], _np(p["proj_w"]), _np(p["proj_b"])))
    assert np.array_equal(taps["front_mask"], np.where(fm[..., None], np.float32(0), taps["front_end"]))
    assert (taps["front_mask"][fm] == 0).all() and (taps["front_end"][fm] != 0).any()
    seen.add("front_mask")
    G, K = cfg["conv_pos_groups"], cfg["conv_pos"]
    img = R.pos_image(taps["front_mask"], G, K)
    assert np.array_equal(taps["pos_pad"], img)
    seen.add("pos_pad")
    ops = R.pos_operands(img, _np(p["pos_w"]), _np(p["pos_b"]), taps["front_mask"])
    val, bnd = R.gemm_bound(*ops[:3], 1, ops[3])
    check("pos_conv", R.pos_back(val), R.pos_back(bnd))
    relb = _np(model.position_bias_table(T))
    x = "pos_conv"
    for i, Li in enumerate(p["layers"]):
        blk = "block%d." % i
        Li = {k: _np(v) for k, v in Li.items()}
        check(blk + "ln1", *R.layernorm_bound(taps[x], Li["ln1_g"], Li["ln1_b"]))
        h = taps[blk + "ln1"]
        check(blk + "gate", *(a.reshape(B, T, H) for a in R.gate_bound(h.reshape(B * T, D), Li["grep_w"], Li["grep_b"],
                                                                     Li["grep_a"], H)))
        check(blk + "qkv", *R.gemm_bound(h, Li["qkv_w"], Li["qkv_b"]))
        qkv = taps[blk + "qkv"]
        check(blk + "att", *L.attention_tiled_bound(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], taps[blk + "gate"],
                                                    relb, H, fm))
        check(blk + "out_proj", *R.gemm_bound(taps[blk + "att"], Li["out_w"], Li["out_b"], 0, taps[x]))
        check(blk + "ln2", *R.layernorm_bound(taps[blk + "out_proj"], Li["ln2_g"], Li["ln2_b"]))
        check(blk + "fc1", *R.gemm_bound(taps[blk + "ln2"], Li["fc1_w"], Li["fc1_b"], 1))
        check(blk + "fc2", *R.gemm_bound(taps[blk + "fc1"], Li["fc2_w"], Li["fc2_b"], 0, taps[blk + "out_proj"]))
        x = blk + "fc2"
    assert np.array_equal(taps["block0"], taps["block0.fc2"])
    seen.add("block0")
    check("blocks", *R.layernorm_bound(taps[x], _np(p["fin_g"]), _np(p["fin_b"])))
    assert np.array_equal(taps["blocks"], _np(out))
    assert seen == set(taps), sorted(set(taps) ^ seen)
    assert len(taps) == 1 + 2 * len(layers) + 1 + 5 + 8 * len(p["layers"]) + 2


# ---- routing --------------------------------------------------------------------------------------------------------
def _calls(model, *args, **kw):
    """(result, [entry point names]) of one _forward."""
    names = []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = spy                                             # (_forward looks _lib.call up when it runs)
    try:
        out = model._forward(*args, **kw)
    finally:
        _lib.call = real
    return out, names


def test_routing():
    g = golden("wavlm_long_324")
    wseed, aseed, _, n324 = (int(v) for v in g["meta"][:4])
    default, long_ = model_of(wseed, False), model_of(wseed, True)
    wav = synth.make_wav(aseed, 2, n324)
    # 199 frames, no mask: the same launches and the same bits with and without long_inputs
    a, names_a = _calls(default, wav[:, :64000])
    b, names_b = _calls(long_, wav[:, :64000])
    assert a.shape == (2, 199, 128) and torch.equal(a, b) and names_a == names_b
    assert "qpg_wavlm_attention_f32" in names_a and "qpg_wavlm_attention_tiled_f32" not in names_a
    # 324 frames: the default model raises as before, naming the frames; the opt-in runs the tiled kernel
    with pytest.raises(NotImplementedError, match="324 frames"):
        default.extract_features(wav)
    _, names = _calls(long_, wav)
    assert names.count("qpg_wavlm_attention_tiled_f32") == 2 and "qpg_wavlm_attention_f32" not in names
    # a padding mask routes to the tiled kernel at any T; past 256 frames it needs the opt-in too
    mask = np.zeros(wav.shape, bool)
    mask[1, 50000:] = True
    _, names = _calls(default, wav[:, :64000], padding_mask=mask[:, :64000])
    assert names.count("qpg_wavlm_attention_tiled_f32") == 2 and "qpg_wavlm_attention_f32" not in names
    with pytest.raises(NotImplementedError, match="324 frames"):
        default.extract_features(wav, padding_mask=mask)
    assert long_.extract_features(wav, padding_mask=mask)[0].shape == (2, 324, 128)
    # a member without a valid frame: ValueError before any launch
    mask[0] = True
    before = _lib.n_calls
    with pytest.raises(ValueError, match="batch member 0"):
        long_.extract_features(wav, padding_mask=mask)
    assert _lib.n_calls == before


def test_output_layer_does_not_launch_later_blocks():
    g = golden("wavlm_layers")
    sd, wav, _, _ = ragged_audio(g)
    model = model_of(int(g["meta"][0]), False)
    stages = []
    model._forward(wav, lambda stage, view: stages.append(stage), output_layer=1)
    assert "block0.fc2" in stages and not [s for s in stages if s.startswith("block1.")] and stages[-1] == "blocks"
    stages2 = []
    model._forward(wav, lambda stage, view: stages2.append(stage), output_layer=2)
    assert "block1.fc2" in stages2


# ---- wav2wavlm and the --whole CLI ----------------------------------------------------------------------------------
def test_wav2wavlm_and_the_whole_cli(tmp_path):
    """A 6.5 s clip (324 frames) written with `wave`: wav2wavlm and --whole give the long_inputs model's (1, T, D) on the
    clip's samples, --layer k block k's output; without --whole the windowed output is what it was."""
    import wave
    g = golden("wavlm_long_324")
    wseed = int(g["meta"][0])
    ck = str(tmp_path / "wavlm.pt")
    torch.save({"cfg": dict(CFG), "model": {k: torch.from_numpy(v) for k, v in weights(wseed).items()}}, ck)
    pcm = np.round(synth.make_wav(91, 1, 104000)[0] * 32767).astype("<i2")
    with wave.open(str(tmp_path / "clip.wav"), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    samples = pcm.astype(np.float32) / np.float32(32768.0)
    model = model_of(wseed, True)
    want = model.extract_features(samples[None])[0].cpu().numpy()
    got = W.wav2wavlm(samples, model, DEV)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (1, 324, 128)
    assert np.array_equal(got, want)
    ref = L.forward_long(weights(wseed), CFG, samples[None])["x"]
    within("wav2wavlm against the restatement", torch.from_numpy(got), ref, float(g["e32"]))
    out = W.main(["--wav", str(tmp_path / "clip.wav"), "--WavLM_model_path", ck, "--out", str(tmp_path / "w.npz"), "--whole"])
    f = np.load(out)
    assert f.files == ["wavlm"] and np.array_equal(f["wavlm"], want)
    out = W.main(["--wav", str(tmp_path / "clip.wav"), "--WavLM_model_path", ck, "--out", str(tmp_path / "l.npz"), "--whole",
                  "--layer", "1"])
    assert np.array_equal(np.load(out)["wavlm"], model.extract_features(samples[None], output_layer=1)[0].cpu().numpy())
    out = W.main(["--wav", str(tmp_path / "clip.wav"), "--WavLM_model_path", ck, "--out", str(tmp_path / "q.npz")])
    assert np.load(out)["wavlm"].shape == (1, 199, 128)
    with pytest.raises(ValueError, match="1-D"):
        W.wav2wavlm(samples[None], model)
