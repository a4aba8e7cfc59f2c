"""WavLM feature extraction on the device (qpg_wavlm.hip, qpgesture_amd/wavlm.py) against the f64 restatement of
tests/wavlm_ref.py (itself pinned to the reference's f64 run by tests/test_wavlm_cpu.py).

Tolerances: a stage's bound is 8 x e32, e32 = max |f32 evaluation - f64 evaluation| of the same stage - for the end-to-end
fixtures the reference model's own f32 run, read from the fixture; for a single kernel the NumPy f32 evaluation of
wavlm_ref on the test's inputs.  The device's error is rounding noise of the same kind, over sequential FMA chains where
torch / NumPy sum in blocks: hence the margin.  Each test prints its measured ratio before asserting."""
import os

import numpy as np
import pytest
import torch

from qpgesture_amd import _lib, synth
from qpgesture_amd import wavlm as W
from tests import wavlm_ref as R
from tests.test_wavlm_cpu import fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 8.0


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def check(name, got, ref64, ref32):
    """got (device result, f32) within MARGIN x e32 of ref64; e32 from the f32 evaluation of the same stage."""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert np.isfinite(got).all(), name
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    err = float(np.abs(got - ref64).max())
    print("%s: err %.3e e32 %.3e ratio %.2f" % (name, err, e32, err / e32 if e32 > 0 else 0.0))
    assert err <= MARGIN * e32, "%s: |device - f64| = %.3e > %g x e32 (%.3e)" % (name, err, MARGIN, e32)


def run_with_taps(model, wav):
    """(result, {stage: copy}) of one forward pass: the stage views of WavLM._forward, copied as they are handed out."""
    taps = {}
    out = model._forward(wav, lambda stage, view: taps.__setitem__(stage, None if view is None else view.clone()))
    return out, taps


_models = {}


def model_of(cfg_name, seed, cfg):
    key = (cfg_name, seed)
    if key not in _models:
        sd = synth.make_wavlm_state_dict(seed, cfg)
        _models[key] = (W.WavLM(cfg, device=DEV).load_state_dict(sd), sd)
    return _models[key]


# ---- conv feature extractor: layer 0 and the strided conv GEMMs -----------------------------------------------------
@pytest.mark.parametrize("conv_bias", [True, False])
@pytest.mark.parametrize("n,B", [(400, 2), (16000, 3), (64000, 2)])
def test_conv_stack(n, B, conv_bias):
    """T = 1 (the receptive field), 49 and 199; the 64 000-sample case runs the odd row counts 12 799 / 6 399 / ... over the
    GEMM's 128-row tiles, per batch."""
    cfg = dict(synth.WAVLM_TINY, conv_bias=conv_bias)
    model, sd = model_of("tiny_bias%d" % conv_bias, 51, cfg)
    wav = synth.make_wav(60 + n % 7, B, n)
    out, taps = run_with_taps(model, wav)
    T = W.frames_of(n, model.conv_layers)[-1]
    assert out.shape == (B, T, 128) and taps["features"].shape == (B, T, 64)
    check("conv n=%d bias=%d" % (n, conv_bias), taps["features"], R.feature_extractor(sd, cfg, wav, np.float64),
          R.feature_extractor(sd, cfg, wav, np.float32))


def test_conv0_alone():
    """Layer 0 before its norm: every (frame, channel) of a short clip, with the bias."""
    rng = _rng(3)
    B, n, C, k, s = 2, 1003, 64, 10, 5
    wav, w, b = rng.standard_normal((B, n)), rng.standard_normal((C, 1, k)), rng.standard_normal(C)
    wav, w, b = (a.astype(np.float32) for a in (wav, w, b))
    T = (n - k) // s + 1
    assert _lib.load().qpg_wavlm_conv_frames(n, k, s) == T
    out = torch.empty((B, T, C), dtype=torch.float32, device=DEV)
    _lib.call("qpg_wavlm_conv0_f32", DEV, dev(wav), B, n, dev(w.reshape(C, k)), dev(b), C, k, s, out)
    check("conv0", out, R.conv1d(wav.astype(np.float64)[:, :, None], w.astype(np.float64), b.astype(np.float64), s),
          R.conv1d(wav[:, :, None], w, b, s))


# ---- LayerNorm (+ GELU) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("gelu", [0, 1])
@pytest.mark.parametrize("C", [64, 512, 1024])
def test_layernorm(C, gelu):
    """1 003 rows (4 per block: a tail block); the second half has a mean of 1000 against a spread of 0.01."""
    rng = _rng(100 + C)
    M = 1003
    x = rng.standard_normal((M, C)) * rng.uniform(0.1, 3.0, (M, 1)) + rng.standard_normal((M, 1))
    x[M // 2:] = 1000.0 + 0.01 * rng.standard_normal((M - M // 2, C))
    x = x.astype(np.float32)
    g, b = rng.uniform(0.6, 1.4, C).astype(np.float32), (rng.standard_normal(C) * 0.1).astype(np.float32)
    y = torch.empty((M, C), dtype=torch.float32, device=DEV)
    _lib.call("qpg_wavlm_layernorm_f32", DEV, dev(x), dev(g), dev(b), M, C, 1e-5, gelu, y)

    def ref(dt):
        r = R.layer_norm(x.astype(dt), g.astype(dt), b.astype(dt))
        return R.gelu(r) if gelu else r
    for lo, hi, what in ((0, M // 2, "plain"), (M // 2, M, "large mean")):
        check("layernorm C=%d gelu=%d %s" % (C, gelu, what), y[lo:hi], ref(np.float64)[lo:hi], ref(np.float32)[lo:hi])
    xin = dev(x)
    _lib.call("qpg_wavlm_layernorm_f32", DEV, xin, dev(g), dev(b), M, C, 1e-5, gelu, xin)          # in place
    assert torch.equal(xin, y)


# ---- pos_conv ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 1024])
@pytest.mark.parametrize("T", [1, 49, 199, 256])
def test_pos_conv(T, D):
    """x + GELU(grouped conv, 128 taps, padding 64, last frame dropped): T below and above the kernel length."""
    rng = _rng(200 + T + D)
    B, G, K = 2, 16, 128
    Cg = D // G
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    weff = (rng.standard_normal((D, Cg, K)) / np.sqrt(Cg * K) * 2.0).astype(np.float32)
    bias = (rng.standard_normal(D) * 0.1).astype(np.float32)
    rows = T + K - 1
    xd = dev(x)
    padded = torch.full((B * G * rows * Cg + 64,), 7.0, dtype=torch.float32, device=DEV)
    _lib.call("qpg_wavlm_pos_pad_f32", DEV, xd, B, T, D, G, K, padded)
    img = padded[:B * G * rows * Cg].view(B, G, rows, Cg).cpu().numpy()
    want = np.zeros((B, G, rows, Cg), np.float32)
    want[:, :, K // 2:K // 2 + T] = x.reshape(B, T, G, Cg).transpose(0, 2, 1, 3)
    assert np.array_equal(img, want) and bool((padded[B * G * rows * Cg:] == 7.0).all())
    w = dev(weff.reshape(G, Cg, Cg, K).transpose(0, 1, 3, 2))
    y = torch.empty((B, T, D), dtype=torch.float32, device=DEV)
    _lib.call("qpg_wavlm_gemm_f32", DEV, padded, Cg, w, dev(bias), xd, y, D, T, Cg, K * Cg, 1, B, G, G * rows * Cg,
              rows * Cg, Cg * K * Cg, Cg, T * D, Cg)
    check("pos_conv T=%d D=%d" % (T, D), y, R.pos_conv(x.astype(np.float64), weff.astype(np.float64), bias, G),
          R.pos_conv(x, weff, bias, G))


# ---- gate and attention -----------------------------------------------------------------------------------------
def _attention_case(T, H, seed, bias_scale=1.0):
    rng = _rng(seed)
    B, D = 2, H * 64
    q = (rng.standard_normal((B, T, D)) * 0.35).astype(np.float32)
    k = rng.standard_normal((B, T, D)).astype(np.float32)
    v = rng.standard_normal((B, T, D)).astype(np.float32)
    gate = rng.uniform(0.7, 2.4, (B, T, H)).astype(np.float32)
    relb = (rng.standard_normal((2 * T - 1, H)) * bias_scale).astype(np.float32)
    idx = np.arange(T)[None, :] - np.arange(T)[:, None] + T - 1                       # [q][k] -> k - q + T - 1
    bias = relb[idx].transpose(2, 0, 1)                                               # [H][T][T]
    return B, D, q, k, v, gate, relb, bias


def _run_attention(B, T, H, q, k, v, gate, relb):
    qkv = dev(np.concatenate([q, k, v], 2))
    out = torch.empty((B, T, H * 64), dtype=torch.float32, device=DEV)
    _lib.call("qpg_wavlm_attention_f32", DEV, qkv, dev(gate), dev(relb), B, T, H, out)
    return out


@pytest.mark.parametrize("H", [2, 16])
@pytest.mark.parametrize("T", [1, 49, 199, 256])
def test_attention(T, H):
    B, D, q, k, v, gate, relb, bias = _attention_case(T, H, 300 + T + H)
    out = _run_attention(B, T, H, q, k, v, gate, relb)
    f64 = [a.astype(np.float64) for a in (q, k, v, gate, bias)]
    check("attention T=%d H=%d" % (T, H), out, R.attention(*f64, H), R.attention(q, k, v, gate, bias, H))
    # the same table under another block's gates
    gate2 = (gate[::-1] * 0.5 + 0.3).astype(np.float32).copy()
    out2 = _run_attention(B, T, H, q, k, v, gate2, relb)
    f64[3] = gate2.astype(np.float64)
    check("attention T=%d H=%d, second gate" % (T, H), out2, R.attention(*f64, H), R.attention(q, k, v, gate2, bias, H))


def test_attention_near_one_hot_rows():
    """The bias table times 20: scores reach +-150 and rows are near one-hot.  exp() of an unshifted score overflows f32."""
    T, H = 199, 2
    B, D, q, k, v, gate, relb, bias = _attention_case(T, H, 77, bias_scale=20.0)
    assert np.abs(gate[..., None, :].transpose(0, 3, 1, 2) * bias[None]).max() > 100.0
    out = _run_attention(B, T, H, q, k, v, gate, relb)
    f64 = [a.astype(np.float64) for a in (q, k, v, gate, bias)]
    check("attention near one-hot", out, R.attention(*f64, H), R.attention(q, k, v, gate, bias, H))


@pytest.mark.parametrize("H", [2, 16])
def test_gate(H):
    rng = _rng(400 + H)
    B, T = 2, 199
    h = rng.standard_normal((B, T, H * 64)).astype(np.float32)
    gw, gb = (rng.standard_normal((8, 64)) / 8).astype(np.float32), (rng.standard_normal(8) * 0.1).astype(np.float32)
    ga = rng.uniform(0.5, 1.5, H).astype(np.float32)
    out = torch.empty((B, T, H), dtype=torch.float32, device=DEV)
    _lib.call("qpg_wavlm_gate_f32", DEV, dev(h), dev(gw), dev(gb), dev(ga), B * T, H, out)
    check("gate H=%d" % H, out, R.gate(h.astype(np.float64), gw, gb, ga, H), R.gate(h, gw, gb, ga, H))


# ---- the Linear GEMMs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,gelu,residual", [(128, 256, 1, False), (128, 384, 0, False), (256, 128, 0, True),
                                               (1024, 192, 1, False), (1024, 1024, 0, True), (4096, 128, 0, True),
                                               (4096, 64, 1, True)])
def test_linear_gemm(K, N, gelu, residual):
    """M = 2 x 199 rows (three full row tiles and a tail of 14), every K of the model, N with and without a column tail."""
    rng = _rng(500 + K + N)
    M = 398
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = (rng.standard_normal(N) * 0.1).astype(np.float32)
    r = rng.standard_normal((M, N)).astype(np.float32) if residual else None
    out = torch.full((M + 1, N), 7.0, dtype=torch.float32, device=DEV)
    _lib.call("qpg_wavlm_gemm_f32", DEV, dev(a), K, dev(w), dev(b), None if r is None else dev(r), out, N, M, N, K, gelu,
              1, 1, 0, 0, 0, 0, 0, 0)
    assert bool((out[M] == 7.0).all())                                                # nothing past the last row

    def ref(dt):
        y = R.linear(a.astype(dt), w.astype(dt), b.astype(dt))
        y = R.gelu(y) if gelu else y
        return y + r.astype(dt) if residual else y
    check("gemm K=%d N=%d gelu=%d res=%d" % (K, N, gelu, residual), out[:M], ref(np.float64), ref(np.float32))


def test_gemm_refuses_a_k_tail():
    a = torch.zeros((4, 24), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.Unsupported, match="multiple of 16"):
        _lib.call("qpg_wavlm_gemm_f32", DEV, a, 24, a, None, None, a, 24, 4, 4, 24, 0, 1, 1, 0, 0, 0, 0, 0, 0)


# ---- end to end -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny_1s", "wide"])
def test_end_to_end_fixture(name):
    """The three fixtures within 8 x e32 of the reference's f64 result, e32 = the reference's own f32 error (from the
    fixture), on the result and on the three intermediate results."""
    g, cfg, sd, wav, _ = fixture(name)
    model, _ = model_of(name.split("_")[0], int(g["meta"][0]), cfg)
    out, taps = run_with_taps(model, torch.from_numpy(wav))
    assert torch.equal(taps["blocks"], out) and out.dtype == torch.float32 and out.is_cuda
    cstep = int(g["meta"][5])
    bad = []
    for tap, got, rows, e32 in (("features", taps["features"], g["tap_rows"], float(g["e32_features"])),
                                ("pos_conv", taps["pos_conv"], g["tap_rows"], float(g["e32_pos_conv"])),
                                ("block0", taps["block0"], g["tap_rows"], float(g["e32_block0"])),
                                ("out", out, g["rows"], float(g["e32"]))):
        a = got.cpu().numpy().astype(np.float64)[:, rows][:, :, ::cstep]
        want = g["out"] if tap == "out" else g[tap]
        assert a.shape == want.shape, tap
        err = float(np.abs(a - want).max())
        print("%s %s: err %.3e e32 %.3e ratio %.2f" % (name, tap, err, e32, err / e32))
        if not err <= MARGIN * e32:
            bad.append((tap, err, e32))
    assert not bad, bad
    # a second call through the same workspace gives the same bits; the public call has the reference's return shape
    again, pad = model.extract_features(torch.from_numpy(wav))
    assert pad is None and torch.equal(again, out)


def test_batches_do_not_leak():
    """B = 2 equals two B = 1 calls bit for bit, in either order of the workspace's use."""
    g, cfg, sd, wav, _ = fixture("tiny")
    model, _ = model_of("tiny", int(g["meta"][0]), cfg)
    both = model.extract_features(wav)[0]
    one = [model.extract_features(wav[i:i + 1])[0] for i in range(2)]
    assert torch.equal(both[0], one[0][0]) and torch.equal(both[1], one[1][0])
    assert not torch.equal(both[0], both[1])
    assert torch.equal(model.extract_features(wav)[0], both)


def test_normalize_input_is_per_window():
    """normalize_input=True: each window to zero mean / unit variance (eps 1e-5) on its own, so a window's features still
    do not depend on its batch; the result is the plain model's on the windows normalised in f32 beforehand."""
    g, cfg, sd, wav, _ = fixture("tiny_1s")
    plain, _ = model_of("tiny", int(g["meta"][0]), cfg)
    norm = W.WavLM(cfg, device=DEV, normalize_input=True).load_state_dict(sd)
    w = torch.from_numpy(wav * np.array([[1.0], [3.0], [0.25]], np.float32) + np.float32(0.1)).to(DEV)
    got = norm.extract_features(w)[0]
    mean = w.mean(1, keepdim=True)
    pre = (w - mean) / torch.sqrt(((w - mean) ** 2).mean(1, keepdim=True) + 1e-5)
    want = plain.extract_features(pre)[0]
    e32 = float(g["e32"])
    err = float((got - want).abs().max())
    print("normalize_input: |got - prenormalised| %.3e (e32 %.3e)" % (err, e32))
    assert err <= MARGIN * e32                      # (two f32 evaluations of the same normalisation)
    assert torch.equal(norm.extract_features(w[1:2])[0][0], got[1])
    assert not torch.equal(got, plain.extract_features(w)[0])


def _samples_for(T, layers):
    n = 400
    while W.frames_of(n, layers)[-1] < T:
        n += 1
    return n


def test_frame_limit():
    """256 frames run and agree with the restatement; 257 raise - in Python before anything is launched, and in the
    attention entry point as QPG_EUNSUP with its output untouched."""
    g, cfg, sd, _, _ = fixture("tiny")
    model, _ = model_of("tiny", int(g["meta"][0]), cfg)
    n256, n257 = _samples_for(256, model.conv_layers), _samples_for(257, model.conv_layers)
    assert W.frames_of(n256, model.conv_layers)[-1] == 256 and W.frames_of(n257 - 1, model.conv_layers)[-1] == 256
    wav = synth.make_wav(9, 1, n257)
    out = model.extract_features(wav[:, :n256])[0]
    assert out.shape == (1, 256, 128)
    check("T=256 end to end", out, R.forward(sd, cfg, wav[:, :n256], np.float64)["out"],
          R.forward(sd, cfg, wav[:, :n256], np.float32)["out"])
    with pytest.raises(NotImplementedError, match="257 frames"):
        model.extract_features(wav)
    T, H = 257, 2
    qkv = torch.zeros((T, 3 * H * 64), dtype=torch.float32, device=DEV)
    o = torch.full((T, H * 64), 7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.Unsupported, match="257 frames"):
        _lib.call("qpg_wavlm_attention_f32", DEV, qkv, torch.ones((T, H), device=DEV), torch.zeros((2 * T - 1, H), device=DEV),
                  1, T, H, o)
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    with pytest.raises(ValueError, match="receptive field"):
        model.extract_features(wav[:, :399])


# ---- the dataset step and the CLIs ------------------------------------------------------------------------------
def _write_checkpoint(path, cfg, sd):
    torch.save({"cfg": dict(cfg), "model": {k: torch.from_numpy(v) for k, v in sd.items()}}, path)


def test_wav_to_wavlm_writes_the_reference_files(tmp_path):
    g, cfg, sd, _, _ = fixture("tiny")
    ck = str(tmp_path / "wavlm.pt")
    _write_checkpoint(ck, cfg, sd)
    prefix = "speaker_10_state_0"
    os.makedirs(tmp_path / prefix)
    wavs = {"train": synth.make_wav(70, 3, 64000), "test": synth.make_wav(71, 1, 64000)}
    for split, w in wavs.items():
        np.savez(str(tmp_path / prefix / ("%s_%s_240.npz" % (prefix, split))), wav=w, body=np.zeros((len(w), 1)))
    written = W.wav_to_wavlm(str(tmp_path), prefix, ck, gpu="0", batch=2)
    assert set(written) == {"train", "test"}                                            # validation split absent
    model, _ = model_of("tiny", int(g["meta"][0]), cfg)
    for split, w in wavs.items():
        assert written[split] == str(tmp_path / prefix / ("%s_%s_240_WavLM.npz" % (prefix, split)))
        f = np.load(written[split])
        assert f.files == ["wavlm"]
        assert f["wavlm"].dtype == np.float32 and f["wavlm"].shape == (len(w), 199, 128)
        # batches of 2 (+1) give what one call gives: a window's features do not depend on its batch
        assert np.array_equal(f["wavlm"], model.extract_features(w)[0].cpu().numpy())


def test_make_beat_dataset_step3_with_and_without_wavlm(tmp_path):
    """Without --WavLM_model_path step 3 writes the code files and nothing else; with it, the same code files (bytes)
    and the WavLM files next to them."""
    from qpgesture_amd import make_beat_dataset as cli
    g, cfg, sd, _, _ = fixture("tiny")
    ck_w, ck_v = str(tmp_path / "wavlm.pt"), str(tmp_path / "ck.bin")
    _write_checkpoint(ck_w, cfg, sd)
    torch.save({"args": {}, "epoch": 1,
                "model_dict": {k: torch.from_numpy(v) for k, v in synth.make_vqvae_state_dict(7).items()}}, ck_v)
    cfg_path = os.path.join(os.path.dirname(os.path.abspath(cli.__file__)), "configs", "codebook.yml")
    prefix = "speaker_10_state_0"
    rng = _rng(12)
    for d in ("a", "b"):
        os.makedirs(tmp_path / d / prefix)
    for split, n in (("train", 3), ("test", 1)):
        body, wav = rng.standard_normal((n, 240, 135)), synth.make_wav(80 + n, n, 64000)
        for d in ("a", "b"):
            np.savez(str(tmp_path / d / prefix / ("%s_%s_240.npz" % (prefix, split))), body=body, wav=wav)
    base = ["--config", cfg_path, "--prefix", prefix, "--gpu", "0", "--step", "3", "--VQVAE_model_path", ck_v]
    out_a = cli.main(base + ["--save_dir", str(tmp_path / "a")])
    out_b = cli.main(base + ["--save_dir", str(tmp_path / "b"), "--WavLM_model_path", ck_w])
    names = lambda d: sorted(os.listdir(str(tmp_path / d / prefix)))                   # noqa: E731
    codes = ["%s_%s_240_code.npz" % (prefix, s) for s in ("test", "train")]
    inputs = ["%s_%s_240.npz" % (prefix, s) for s in ("test", "train")]
    assert names("a") == sorted(inputs + codes)
    assert names("b") == sorted(inputs + codes + ["%s_%s_240_WavLM.npz" % (prefix, s) for s in ("test", "train")])
    assert set(out_a) == set(out_b) == {"train", "test"}
    for split in ("train", "test"):
        assert open(out_a[split], "rb").read() == open(out_b[split], "rb").read()
        f = np.load(str(tmp_path / "b" / prefix / ("%s_%s_240_WavLM.npz" % (prefix, split))))
        assert f["wavlm"].dtype == np.float32 and f["wavlm"].shape[1:] == (199, 128)


def test_query_cli(tmp_path):
    """--wav: a 16 kHz PCM clip of two windows and a bit -> wavlm (2, 199, D) that equals the model on the two cuts."""
    import wave
    g, cfg, sd, _, _ = fixture("tiny")
    ck = str(tmp_path / "wavlm.pt")
    _write_checkpoint(ck, cfg, sd)
    pcm = np.round(synth.make_wav(90, 1, 2 * 64000 + 777)[0] * 32767).astype("<i2")
    with wave.open(str(tmp_path / "clip.wav"), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    out = W.main(["--wav", str(tmp_path / "clip.wav"), "--WavLM_model_path", ck, "--out", str(tmp_path / "q.npz")])
    got = np.load(out)["wavlm"]
    assert got.dtype == np.float32 and got.shape == (2, 199, 128)
    model, _ = model_of("tiny", int(g["meta"][0]), cfg)
    want = model.extract_features((pcm.astype(np.float32) / 32768.0)[:128000].reshape(2, 64000))[0].cpu().numpy()
    assert np.array_equal(got, want)
