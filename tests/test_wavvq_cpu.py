"""vq-wav2vec code extraction without a GPU: the torch restatement (tests/wavvq_model_ref.py) against the recorded f64
fixture (tests/golden/wavvq_model.npz, make_golden_wavvq_model.py), the fixture's own conditions, the checkpoint loader,
every refusal, the frame arithmetic and make_test_data's files with the model stubbed by the restatement.

The frame arithmetic: one output frame of the vq-wav2vec stack sees 4, 10, 22 frames of layers 3, 2, 1, 92 frames of layer
0 and so 91 x 5 + 10 = 465 samples: 464 samples give no frame and 465 one.  The request for this feature names 944 / 945
for that edge; those lengths give 3 and 4 frames (an edge of the frame count too) and are checked here as what they are."""
import argparse
import os
import wave

import numpy as np
import pytest
import torch

from qpgesture_amd import make_test_data, synth, wavvq
from qpgesture_amd.wavlm import frames_of
from tests import wavvq_model_ref as R

_cache = {}
CODE_CAP = 0.01          # at most this share of a case's positions may be left out of the exact code comparison


def golden(golden_dir):
    if "g" not in _cache:
        _cache["g"] = dict(np.load(os.path.join(golden_dir, "wavvq_model.npz")))
    return _cache["g"]


def compared_positions(g, name, logit_bar):
    """Mask of the (b, t, g) whose recorded f64 margin exceeds twice the logit bar: there a run within the bar of the f64
    logits must give the f64 code.  Asserts the cap on what is left out."""
    mask = g[name + "_margin"] > 2 * logit_bar
    left = int((~mask).sum())
    assert left <= CODE_CAP * mask.size, "%s: %d of %d positions left out" % (name, left, mask.size)
    return mask


@pytest.mark.parametrize("name", list(R.CASES))
def test_f32_restatement_against_the_golden(golden_dir, name):
    g = golden(golden_dir)
    geom, sd, wav = R.case_inputs(name)
    rows = R.FULL_ROWS if name == "full" else slice(None)
    m64, m32 = R.WavVQRef(geom, sd, torch.float64), R.WavVQRef(geom, sd, torch.float32)
    z64, l64 = m64.features(wav).numpy(), m64.logits(wav).numpy()
    assert np.abs(z64[:, rows] - g[name + "_z"]).max() <= 1e-12 and np.abs(l64[:, rows] - g[name + "_logits"]).max() <= 1e-12
    assert np.array_equal(m64.forward_idx(wav).numpy(), g[name + "_codes"])
    assert np.allclose(R.top2_margin(l64), g[name + "_margin"], rtol=0, atol=1e-12)
    # the f32 run: within twice its own recorded error (thread counts reorder torch's sums), codes equal wherever the
    # margin clears that, nothing left out
    for tap, got in (("z", m32.features(wav)), ("logits", m32.logits(wav))):
        want = z64 if tap == "z" else l64
        err, e32 = float(np.abs(got.numpy().astype(np.float64) - want).max()), float(g[name + "_e32_" + tap])
        print("%s %s: f32 err %.3e recorded %.3e" % (name, tap, err, e32))
        assert err <= 2 * e32
    mask = compared_positions(g, name, 2 * float(g[name + "_e32_logits"]))
    assert mask.all()
    assert np.array_equal(m32.forward_idx(wav).numpy(), g[name + "_codes"])


def test_fixture_conditions(golden_dir):
    g = golden(golden_dir)
    assert int(g["seed_tiny"]) == R.SEED_TINY and int(g["seed_full"]) == R.SEED_FULL
    for name, (kind, _, _, B, n, _, _) in R.CASES.items():
        geom = R.geometry(kind)
        T = frames_of(n, wavvq.conv_layers_of(geom))[-1]
        assert g[name + "_codes"].shape == (B, T, geom["vq_groups"]) and g[name + "_codes"].dtype == np.int64
        assert 0 <= g[name + "_codes"].min() and g[name + "_codes"].max() < geom["vq_vars"]
        assert float(g[name + "_margin"].min()) >= 64 * float(g[name + "_e32_logits"]) and int(g[name + "_codes32_diff"]) == 0
        assert 0 < float(g[name + "_e32_z"]) < 1e-4 and 0 < float(g[name + "_e32_logits"]) < 1e-4
    assert g["full_codes"].shape == (1, 398, 2) and g["n465_codes"].shape == (2, 1, 2)
    assert frames_of(3200, wavvq.conv_layers_of(synth.WAVVQ_TINY))[0] % 2 == 1
    assert frames_of(4001, wavvq.conv_layers_of(synth.WAVVQ_TINY))[0] % 2 == 1
    sd = synth.make_wavvq_state_dict(R.SEED_TINY)
    for i in range(8):                                           # GroupNorm weights and biases are not 1 and 0
        w, b = sd["feature_extractor.conv_layers.%d.2.weight" % i], sd["feature_extractor.conv_layers.%d.2.bias" % i]
        assert np.abs(w - 1).min() > 0 and np.abs(b).min() > 0
    assert any((sd["feature_extractor.conv_layers.%d.2.weight" % i] < 0).any() for i in range(8))


def test_frame_arithmetic():
    layers = wavvq.conv_layers_of(synth.WAVVQ_GUMBEL)
    assert layers == [(512, 10, 5), (512, 8, 4), (512, 4, 2), (512, 4, 2), (512, 4, 2), (512, 1, 1), (512, 1, 1), (512, 1, 1)]
    assert frames_of(64000, layers) == [12799, 3198, 1598, 798, 398, 398, 398, 398]          # the reference's (6, 398, 2)
    assert wavvq.receptive_field(layers) == 465
    assert frames_of(464, layers)[-1] == 0 and frames_of(465, layers)[-1] == 1
    assert frames_of(944, layers)[-1] == 3 and frames_of(945, layers)[-1] == 4
    assert frames_of(9, layers) == [0] * 8
    m = wavvq.WavVQ(synth.WAVVQ_TINY, device="cpu")
    assert [m.frames(n) for n in (464, 465, 469, 470, 944, 945, 3200, 64000)] == [0, 1, 1, 1, 3, 4, 18, 398]
    # chunking: the layer-0 activations of a chunk stay under the budget
    big = wavvq.WavVQ(synth.WAVVQ_GUMBEL, device="cpu")
    assert big.max_chunk(64000) == (1 << 30) // (12799 * 512 * 4) == 40
    assert wavvq.WavVQ(synth.WAVVQ_GUMBEL, device="cpu", l0_budget_bytes=1).max_chunk(64000) == 1
    assert 12799 * 512 * 4 * big.max_chunk(64000) <= wavvq.L0_BUDGET_BYTES


def test_short_window_raises():
    m = wavvq.WavVQ(synth.WAVVQ_TINY, device="cpu").load_state_dict(synth.make_wavvq_state_dict(1))
    for n in (1, 9, 464):
        with pytest.raises(ValueError, match="receptive field"):
            m.forward_idx(np.zeros((1, n), np.float32))
    with pytest.raises(ValueError, match="B, n_samples"):
        m.forward_idx(np.zeros(3200, np.float32))
    with pytest.raises(RuntimeError, match="load_state_dict"):
        wavvq.WavVQ(synth.WAVVQ_TINY, device="cpu").forward_idx(np.zeros((1, 3200), np.float32))


@pytest.mark.parametrize("field,value,word", [
    ("skip_connections_feat", True, "skip_connections_feat"), ("activation", "gelu", "activation"),
    ("vq_type", "kmeans", "vq_type"), ("log_compression", False, "log_compression"), ("vq_depth", 3, "vq_depth"),
    ("conv_feature_layers", "[(512, 10, 5), (256, 8, 4)]", "conv_feature_layers"),
    ("conv_feature_layers", "[(24, 10, 5), (24, 8, 4)]", "conv_feature_layers"),
    ("conv_feature_layers", "[(512, 10, 5), __import__('os')]", "conv_feature_layers"),
    ("vq_groups", 0, "vq_groups")])
def test_refusals_name_the_field(field, value, word):
    with pytest.raises(NotImplementedError, match=word):
        wavvq.WavVQ(dict(synth.WAVVQ_TINY, **{field: value}), device="cpu")
    with pytest.raises(NotImplementedError, match=word):
        wavvq.check_supported(argparse.Namespace(**dict(synth.WAVVQ_TINY, **{field: value})))


def test_state_dict_handling():
    sd = synth.make_wavvq_state_dict(2)
    assert {"vector_quantizer.vars", "feature_aggregator.conv_layers.0.0.weight",
            "wav2vec_predictions.project_to_steps.bias"} <= set(sd)                           # present and ignored
    m = wavvq.WavVQ(synth.WAVVQ_TINY, device="cpu").load_state_dict(sd)
    assert (m.C, m.H, m.G, m.V) == (16, 32, 2, 20) and len(m.p["conv"]) == 8 and len(m.p["head"]) == 2
    assert tuple(m.p["conv"][1]["w"].shape) == (16, 8 * 16)
    w = sd["feature_extractor.conv_layers.1.0.weight"]                                        # [C][Cin][k] -> [C][k][Cin]
    assert np.array_equal(m.p["conv"][1]["w"].numpy().reshape(16, 8, 16), w.transpose(0, 2, 1))
    big = synth.make_wavvq_state_dict(2, synth.WAVVQ_GUMBEL)
    assert big["vector_quantizer.weight_proj.0.0.weight"].shape == (1024, 512)
    assert big["vector_quantizer.weight_proj.1.weight"].shape == (640, 1024)
    with pytest.raises(KeyError, match="conv_layers.3.0.weight"):
        wavvq.WavVQ(synth.WAVVQ_TINY, device="cpu").load_state_dict(
            {k: v for k, v in sd.items() if k != "feature_extractor.conv_layers.3.0.weight"})
    with pytest.raises(ValueError, match="shape"):
        wavvq.WavVQ(dict(synth.WAVVQ_TINY, vq_vars=21), device="cpu").load_state_dict(sd)
    # a non-affine GroupNorm: the keys are absent, weight 1 and bias 0 are implied
    plain = {k: v for k, v in sd.items() if not k.endswith((".2.weight", ".2.bias"))}
    m2 = wavvq.WavVQ(dict(synth.WAVVQ_TINY, non_affine_group_norm=True), device="cpu").load_state_dict(plain)
    assert all(L["g"] is None and L["beta"] is None for L in m2.p["conv"])
    assert not any(k.endswith((".2.weight", ".2.bias"))
                   for k in synth.make_wavvq_state_dict(2, dict(synth.WAVVQ_TINY, non_affine_group_norm=True)))
    with pytest.raises(ValueError, match="non_affine_group_norm"):
        wavvq.WavVQ(dict(synth.WAVVQ_TINY, non_affine_group_norm=True), device="cpu").load_state_dict(sd)
    # depth 1: a single Linear under weight_proj.{weight,bias}
    g1 = dict(synth.WAVVQ_TINY, vq_depth=1)
    sd1 = synth.make_wavvq_state_dict(2, g1)
    assert sd1["vector_quantizer.weight_proj.weight"].shape == (40, 16)
    m1 = wavvq.WavVQ(g1, device="cpu").load_state_dict(sd1)
    assert len(m1.p["head"]) == 1 and m1.H == 0
    ref = R.WavVQRef(g1, sd1, torch.float64)
    assert tuple(ref.forward_idx(synth.make_wav(1, 1, 3200)).shape) == (1, 18, 2)


def test_loader_takes_both_layouts(tmp_path):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_wavvq_state_dict(3).items()}
    plain, fair = str(tmp_path / "plain.pt"), str(tmp_path / "fairseq.pt")
    torch.save({"args": dict(synth.WAVVQ_TINY), "model": sd}, plain)
    import collections
    torch.save({"args": argparse.Namespace(arch="wav2vec", **synth.WAVVQ_TINY), "model": collections.OrderedDict(sd),
                "optimizer_history": [], "extra_state": {}}, fair)
    a, b = wavvq.load_wavvq(plain, device="cpu"), wavvq.load_wavvq(fair, device="cpu")
    assert a.conv_layers == b.conv_layers and (a.G, a.V, a.H) == (b.G, b.V, b.H) == (2, 20, 32)
    for La, Lb in zip(a.p["conv"], b.p["conv"]):
        assert torch.equal(La["w"], Lb["w"]) and torch.equal(La["g"], Lb["g"])
    torch.save({"model": sd}, plain)
    with pytest.raises(ValueError, match="'args'"):
        wavvq.load_wavvq(plain, device="cpu")
    torch.save([1, 2], plain)
    with pytest.raises(ValueError, match="not a checkpoint"):
        wavvq.load_wavvq(plain, device="cpu")


def test_loader_says_how_to_resave_when_a_module_is_absent(tmp_path):
    import pickle
    import sys
    import types
    mod = types.ModuleType("absent_pkg_of_the_test")

    class Task:
        pass
    Task.__module__, Task.__qualname__ = "absent_pkg_of_the_test", "Task"
    mod.Task = Task
    sys.modules["absent_pkg_of_the_test"] = mod
    path = str(tmp_path / "ck.pt")
    try:
        torch.save({"args": dict(synth.WAVVQ_TINY), "model": {}, "task": Task()}, path, pickle_protocol=pickle.DEFAULT_PROTOCOL)
    finally:
        del sys.modules["absent_pkg_of_the_test"]
    with pytest.raises(RuntimeError, match=r"re-save the file in the plain form[\s\S]*'args': vars"):
        wavvq.load_wavvq(path, device="cpu")


class StubModel:
    """forward_idx by the f64 restatement on the CPU: what make_test_data gets instead of the device model."""

    def __init__(self, geom, sd):
        self.ref, self.calls = R.WavVQRef(geom, sd, torch.float64), []

    def forward_idx(self, wav):
        self.calls.append(tuple(np.shape(wav)))
        return self.ref.forward_idx(wav)


def write_wav(path, samples, rate=16000):
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(np.round(samples * 32767.0).astype("<i2").tobytes())


def test_make_test_data_files_keys_and_shapes(tmp_path):
    n = 2 * 64000 + 40000                                       # two whole windows, the rest is dropped as in the reference
    clip = synth.make_wav(9, 1, n)[0]
    wav_path = str(tmp_path / "my clip.wav")
    write_wav(wav_path, clip)
    stub = StubModel(synth.WAVVQ_TINY, synth.make_wavvq_state_dict(4))
    out = str(tmp_path / "out" / "dir")
    paths = make_test_data.process_audio(None, wav_path, out, "0", batch=1, model=stub)
    assert sorted(os.listdir(out)) == ["my clip_wav.npz", "testing_data.npz", "wav_240.npz", "wavvq_240.npz"]
    assert stub.calls == [(1, 64000), (1, 64000)]
    whole = np.load(paths["wav"])["wav"]
    assert whole.shape == (n,) and whole.dtype == np.float32
    win = np.load(paths["windows"])["wav"]
    assert win.shape == (2, 64000) and np.array_equal(win[0], whole[:64000]) and np.array_equal(win[1], whole[64000:128000])
    vq = np.load(paths["wavvq"])
    assert list(vq.keys()) == ["wavvq"] and vq["wavvq"].shape == (2, 398, 2) and vq["wavvq"].dtype == np.int64
    assert np.array_equal(vq["wavvq"], stub.ref.forward_idx(win).numpy())
    td = np.load(paths["testing_data"])
    assert sorted(td.keys()) == sorted(("wav",) + make_test_data.PLACEHOLDERS)
    assert set(make_test_data.PLACEHOLDERS) == {"body", "mfcc", "txt", "aux", "energy", "pitch", "volume", "context", "phase"}
    assert np.array_equal(td["wav"], win)
    for k in make_test_data.PLACEHOLDERS:
        assert td[k].shape == (2, 2, 2) and td[k].dtype == np.float64 and not td[k].any()
    short = str(tmp_path / "short.wav")
    write_wav(short, clip[:63999])
    with pytest.raises(ValueError, match="shorter than one window"):
        make_test_data.process_audio(None, short, out, model=stub)
    other = str(tmp_path / "r8k.wav")
    write_wav(other, clip[:70000], rate=8000)
    with pytest.raises(ValueError, match="16000"):
        make_test_data.process_audio(None, other, out, model=stub)


def test_make_beat_dataset_has_the_flag():
    from qpgesture_amd import make_beat_dataset
    a = make_beat_dataset.build_parser().parse_args(["--WavVQ_model_path", "vq.pt"])
    assert a.WavVQ_model_path == "vq.pt" and a.WavLM_model_path is None
    assert make_beat_dataset.build_parser().parse_args([]).WavVQ_model_path is None
