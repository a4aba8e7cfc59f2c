"""WavLM feature extraction, the host side: the NumPy restatement the GPU tests lean on against the reference's own
f64 results (tests/golden/make_golden_wavlm.py), the bucket table, the weight-norm folding, the cfg checks and the
window cutting of the --wav CLI."""
import os

import numpy as np
import pytest

from qpgesture_amd import synth
from qpgesture_amd import wavlm as W
from tests import wavlm_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"tiny": synth.WAVLM_TINY, "tiny_1s": synth.WAVLM_TINY, "wide": synth.WAVLM_WIDE}
_cache = {}


def fixture(name):
    """(golden arrays, cfg, state dict, wav, f64 taps of wavlm_ref) - computed once per session."""
    if name not in _cache:
        g = dict(np.load(os.path.join(GOLDEN, "wavlm_%s.npz" % name)))
        wseed, aseed, B, n = (int(v) for v in g["meta"][:4])
        cfg = FIXTURES[name]
        sd = synth.make_wavlm_state_dict(wseed, cfg)
        wav = synth.make_wav(aseed, B, n)
        _cache[name] = (g, cfg, sd, wav, R.forward(sd, cfg, wav, np.float64))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_reproduces_the_reference_in_f64(name):
    g, _, _, _, taps = fixture(name)
    assert 1e-6 < float(g["e32"]) < 2e-5                      # (the reference's own f32 error: rounding noise, rms-1 output)
    got = taps["out"][:, g["rows"]][:, :, g["cols"]]
    assert got.shape == g["out"].shape and g["out"].dtype == np.float64
    assert np.abs(got - g["out"]).max() < 1e-9
    for tap in ("features", "pos_conv", "block0"):
        cols = g["cols"] if taps[tap].shape[2] == taps["out"].shape[2] else np.arange(0, taps[tap].shape[2], int(g["meta"][5]))
        got = taps[tap][:, g["tap_rows"]][:, :, cols]
        assert got.shape == g[tap].shape, tap
        assert np.abs(got - g[tap]).max() < 1e-9, tap


def test_frame_counts():
    layers = W.conv_layers_of(synth.WAVLM_LARGE)
    assert layers == [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2
    assert W.frames_of(64000, layers) == [12799, 6399, 3199, 1599, 799, 399, 199]
    assert W.frames_of(400, layers)[-1] == 1 and W.frames_of(399, layers)[-1] == 0
    assert W.frames_of(16000, layers)[-1] == 49


def test_bucket_table_equals_the_reference_at_every_offset():
    g = fixture("tiny")[0]
    off = np.arange(-255, 256)
    got = W.relative_position_buckets(off, 320, 800)
    assert got.dtype == np.int64 and g["buckets"].shape == (511,)
    assert np.array_equal(got, g["buckets"])
    assert got[255] == 0 and got[255 + 79] == 160 + 79 and got[255 - 79] == 79       # exact below 80, per sign
    assert got[255 + 199] > 160 + 80 and got.max() < 320                            # the log range is reached at T = 199


def test_weight_norm_folding_equals_the_reference():
    g, _, sd, _, _ = fixture("tiny_1s")
    weff = W.fold_weight_norm(sd["encoder.pos_conv.0.weight_g"], sd["encoder.pos_conv.0.weight_v"])
    assert weff.shape == sd["encoder.pos_conv.0.weight_v"].shape
    want = g["weff"]
    assert np.abs(weff[::8] - want).max() <= 1e-7 * np.abs(want).max()
    assert np.all(np.abs(weff[::8] - want) <= 1e-7 * np.abs(want) + 1e-300)
    # the f32 image the device gets carries one rounding
    assert np.abs(weff.astype(np.float32)[::8] - want).max() <= 6e-8 * np.abs(want).max()


@pytest.mark.parametrize("field,value", [
    ("extractor_mode", "default"), ("layer_norm_first", False), ("activation_fn", "glu"), ("activation_fn", "relu"),
    ("relative_position_embedding", False), ("gru_rel_pos", False), ("encoder_embed_dim", 96),
    ("encoder_ffn_embed_dim", 200), ("encoder_attention_heads", 4),
    ("conv_feature_layers", "[(64,10,5)] + [(32,3,2)] * 2"), ("conv_feature_layers", "[(48,10,5)]"),
    ("conv_pos", 3), ("conv_pos", 0)])
def test_unsupported_cfg_field_is_named(field, value):
    cfg = dict(synth.WAVLM_TINY, **{field: value})
    with pytest.raises(NotImplementedError, match=field):
        W.check_supported(cfg)
    with pytest.raises(NotImplementedError, match=field):
        W.WavLM(cfg, device="cpu")


def test_supported_cfgs_pass_and_defaults_are_the_base_model():
    for cfg in (synth.WAVLM_TINY, synth.WAVLM_WIDE, synth.WAVLM_LARGE):
        W.check_supported(cfg)
    with pytest.raises(NotImplementedError, match="extractor_mode"):
        W.check_supported({})                                  # (the defaults are the post-LN Base model)
    c = W.WavLMConfig(synth.WAVLM_LARGE)
    assert c.encoder_layers == 24 and c.normalize is True and c.max_distance == 800


@pytest.mark.parametrize("n", [63999, 64000, 64001, 127999, 128000, 128001, 400840, 10])
def test_window_cutting_equals_make_test_data(n):
    # whole 4 s windows back to back, a shorter rest dropped: window i is samples [64000 i, 64000 i + 64000)
    want = [(64000 * i, 64000 * i + 64000) for i in range(n // 64000)]
    assert W.window_bounds(n) == want
    if want:
        clip = np.arange(n, dtype=np.float32)
        cut = W.cut_windows(clip)
        assert cut.shape == (len(want), 64000) and cut.dtype == np.float32
        for row, (a, b) in zip(cut, want):
            assert np.array_equal(row, clip[a:b])
    else:
        with pytest.raises(ValueError, match="shorter than one"):
            W.cut_windows(np.zeros(n, np.float32))


def test_wav_reader_refuses_other_sample_rates(tmp_path):
    import wave
    pcm = (np.sin(np.arange(800) * 0.05) * 12000).astype("<i2")
    for rate in (16000, 44100):
        with wave.open(str(tmp_path / ("r%d.wav" % rate)), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(rate)
            f.writeframes(pcm.tobytes())
    got = W.read_wav_16k(str(tmp_path / "r16000.wav"))
    assert got.dtype == np.float32 and np.array_equal(got, pcm.astype(np.float32) / 32768.0)
    with pytest.raises(ValueError, match="44100 Hz"):
        W.read_wav_16k(str(tmp_path / "r44100.wav"))


def test_synth_state_dict_is_seeded_and_non_trivial():
    a, b = synth.make_wavlm_state_dict(5), synth.make_wavlm_state_dict(5)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert "encoder.pos_conv.0.weight_g" in a and "encoder.layers.1.self_attn.relative_attention_bias.weight" not in a
    assert a["feature_extractor.conv_layers.0.0.bias"].shape == (64,)           # (the tiny cfg has conv_bias)
    assert "feature_extractor.conv_layers.0.0.bias" not in synth.make_wavlm_state_dict(5, synth.WAVLM_WIDE)
    for k, v in a.items():
        if v.ndim == 1 or "grep_a" in k or "weight_g" in k:
            assert np.abs(v).max() > 0 and not np.all(v == 1.0), k
    w = synth.make_wav(3, 2, 1000)
    assert w.shape == (2, 1000) and w.dtype == np.float32 and np.array_equal(w, synth.make_wav(3, 2, 1000))
