"""vq-wav2vec code extraction end to end on the device (qpgesture_amd/wavvq.py over qpg_wavvq.hip, the WavLM layer-0 kernel
and the WavLM GEMM) against the torch restatement's f64 run of the same seeded weights and audio
(tests/golden/wavvq_model.npz; weights and audio are regenerated from synth).

Bars.  e32 = max |the restatement's f32 run - its f64 run| over a case's whole tensor, read from the fixture.  z and the
logits of the device run stay within FACTOR x e32 of the f64 values; the codes equal the f64 codes at every (frame, group)
whose recorded f64 margin exceeds twice the logit bar, and at most 1 % of a case's positions may fall below that (with
these seeds none does: the smallest margin is 205 x e32).  FACTOR is twice the worst ratio device error / e32 measured on
an MI355X over all cases (profiles/wavvq_bench.md has the table); the kernels are deterministic, the margin of two is for
inputs the fixtures do not cover.  Each check prints its ratio first."""
import os
import wave

import numpy as np
import pytest
import torch

from qpgesture_amd import synth, wavvq
from tests import wavvq_model_ref as R
from tests.test_wavvq_cpu import compared_positions, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 3.12          # 2 x 1.56, the worst measured ratio (n465 logits)
_models = {}


def model_of(name):
    kind, seed_w = R.CASES[name][:2]
    if (kind, seed_w) not in _models:
        geom, sd, _ = R.case_inputs(name)
        _models[(kind, seed_w)] = wavvq.WavVQ(geom, device=DEV).load_state_dict(sd)
    return _models[(kind, seed_w)]


def check(name, got, ref64, e32):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert np.isfinite(got).all(), name
    err = float(np.abs(got - ref64).max())
    print("%s: err %.3e e32 %.3e ratio %.2f" % (name, err, e32, err / e32))
    assert err <= FACTOR * e32, "%s: |device - f64| = %.3e > %g x e32 (%.3e)" % (name, err, FACTOR, e32)


@pytest.mark.parametrize("name", list(R.CASES))
def test_features_logits_and_codes_against_f64(golden_dir, name):
    g = golden(golden_dir)
    _, _, wav = R.case_inputs(name)
    model = model_of(name)
    rows = torch.from_numpy(R.FULL_ROWS).to(DEV) if name == "full" else slice(None)
    z, logits = model.features(wav), model.logits(wav)
    assert z.dtype == torch.float32 and tuple(logits.shape[2:]) == (model.G, model.V)
    check(name + " z", z[:, rows], g[name + "_z"], float(g[name + "_e32_z"]))
    check(name + " logits", logits[:, rows], g[name + "_logits"], float(g[name + "_e32_logits"]))
    codes = model.forward_idx(wav)
    want = g[name + "_codes"]
    assert codes.dtype == torch.int64 and codes.device.type == "cuda" and tuple(codes.shape) == want.shape
    mask = compared_positions(g, name, FACTOR * float(g[name + "_e32_logits"]))
    got = codes.cpu().numpy()
    print("%s codes: %d of %d positions compared, %d differ" % (name, int(mask.sum()), mask.size, int((got != want)[mask].sum())))
    assert np.array_equal(got[mask], want[mask])
    assert torch.equal(codes, logits.max(dim=-1)[1])             # the codes are the argmax of the logits the model hands out


def test_silent_window_next_to_a_loud_one(golden_dir):
    _, _, wav = R.case_inputs("silent")
    assert not wav[0].any() and np.abs(wav[1]).max() > 0.3
    model = model_of("silent")
    both = model.logits(wav)
    assert torch.isfinite(both).all()
    assert torch.equal(both[0], both[0, :1].expand_as(both[0]))                    # silence: every frame is the same row
    assert torch.equal(model.logits(wav[:1])[0], both[0]) and torch.equal(model.logits(wav[1:])[0], both[1])


def test_a_window_does_not_depend_on_its_batch():
    _, _, wav = R.case_inputs("n4001")
    model = model_of("n4001")
    whole = model.logits(wav)
    codes = model.forward_idx(wav)
    for i in range(3):
        assert torch.equal(model.logits(wav[i:i + 1])[0], whole[i]), i
    assert torch.equal(model.logits(wav[::-1].copy()), whole.flip(0))
    # chunks of one window (a budget below two windows' layer-0 activations): the same bits
    geom, sd, _ = R.case_inputs("n4001")
    small = wavvq.WavVQ(geom, device=DEV, l0_budget_bytes=799 * 16 * 4).load_state_dict(sd)
    assert small.max_chunk(4001) == 1
    assert torch.equal(small.logits(wav), whole) and torch.equal(small.forward_idx(wav), codes)
    assert torch.equal(small.features(wav), model.features(wav))


@pytest.mark.parametrize("change", [dict(vq_depth=1), dict(non_affine_group_norm=True)], ids=["depth1", "non_affine"])
def test_geometry_variants_against_f64(change):
    """A single-Linear weight_proj and a GroupNorm without weight and bias: no fixture, the restatement runs here (tiny
    geometry, 18 frames) in f64 and f32 and the bar is the same FACTOR x e32."""
    geom = dict(synth.WAVVQ_TINY, **change)
    sd = synth.make_wavvq_state_dict(R.SEED_TINY, geom)
    wav = synth.make_wav(57, 2, 3200)
    l64 = R.WavVQRef(geom, sd, torch.float64).logits(wav)
    e32 = float((R.WavVQRef(geom, sd, torch.float32).logits(wav).double() - l64).abs().max())
    model = wavvq.WavVQ(geom, device=DEV).load_state_dict(sd)
    check("%s logits" % sorted(change)[0], model.logits(wav), l64.numpy(), e32)
    margin = R.top2_margin(l64)
    mask = margin > 2 * FACTOR * e32
    assert (~mask).sum() <= 0.01 * mask.size
    assert np.array_equal(model.forward_idx(wav).cpu().numpy()[mask], l64.max(-1)[1].numpy()[mask])


def test_refusals_on_the_device():
    model = model_of("n465")
    with pytest.raises(ValueError, match="receptive field"):
        model.forward_idx(np.zeros((2, 464), np.float32))
    one = model.forward_idx(np.zeros((1, 465), np.float32))
    assert tuple(one.shape) == (1, 1, 2)


def _write_wav(path, samples):
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.round(samples * 32767.0).astype("<i2").tobytes())


def test_wav_to_bvh_codes_end_to_end(tmp_path):
    """A wav and a synthetic checkpoint through make_test_data, a synth database whose train_wavvq came from wav_to_vq,
    matched in --mode wavvq_audio: the matched codes equal those of the same match fed the restatement's codes.  The
    seeds are chosen so that every one of the 26 windows' f64 margins clears 13 x e32: the device codes ARE the
    restatement's, which is asserted first."""
    from qpgesture_amd import GestureKNN as knn_cli
    from qpgesture_amd import make_beat_dataset, make_test_data
    N, M, prefix = 24, 2, "speaker_1_state_0"
    geom, sd = synth.WAVVQ_TINY, synth.make_wavvq_state_dict(R.SEED_TINY)
    ck = str(tmp_path / "vq-wav2vec.pt")
    import argparse
    torch.save({"args": argparse.Namespace(**geom), "model": {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    ref = R.WavVQRef(geom, sd, torch.float64)
    paths = synth.write_npz_set(str(tmp_path / "npz"), N, M, wavlm_dim=8)
    # database side: <prefix>_train_240.npz['wav'] -> wav_to_vq -> <prefix>_train_240_WavVQ.npz
    save_dir = str(tmp_path / "BEAT")
    os.makedirs(os.path.join(save_dir, prefix))
    train_wav = synth.make_wav(85, N, 64000)
    np.savez(os.path.join(save_dir, prefix, prefix + "_train_240.npz"), wav=train_wav)
    written = wavvq.wav_to_vq(save_dir, prefix, ck, gpu="0", batch=16)
    assert list(written) == ["train"] and written["train"].endswith(prefix + "_train_240_WavVQ.npz")
    train_vq = np.load(written["train"])["wavvq"]
    assert train_vq.shape == (N, 398, 2) and train_vq.dtype == np.int64
    want_train = ref.forward_idx(train_wav).numpy()
    assert np.array_equal(train_vq, want_train), "%d train codes differ" % int((train_vq != want_train).sum())
    assert make_beat_dataset.build_parser().parse_args(["--WavVQ_model_path", ck]).WavVQ_model_path == ck
    # query side: clip.wav -> make_test_data -> wavvq_240.npz
    clip = synth.make_wav(72, 1, M * 64000 + 5000)[0]
    wav_path = str(tmp_path / "clip.wav")
    _write_wav(wav_path, clip)
    out = make_test_data.main(["--audio_path", wav_path, "--save_path", str(tmp_path / "clip"), "--wavvq_model_path", ck,
                               "--gpu", "0"])
    test_vq = np.load(out["wavvq"])["wavvq"]
    want_test = ref.forward_idx(np.load(out["windows"])["wav"]).numpy()
    assert test_vq.shape == (M, 398, 2) and np.array_equal(test_vq, want_test)

    def match(train_wavvq, test_wavvq, tag):
        argv = []
        for k, v in dict(paths, train_wavvq=train_wavvq, test_wavvq=test_wavvq).items():
            argv += ["--" + k, v]
        dst = str(tmp_path / (tag + ".npz"))
        # (--no_phase: with the phase gate the wavvq modes draw their first phase slice from a 398-frame range on a
        # 240-frame track, which the default seed misses - in the reference too)
        knn_cli.main(argv + ["--mode", "wavvq_audio", "--no_phase", "--out_knn_filename", dst, "--db_cache", "off"])
        return np.load(dst)["knn_pred"]
    got = match(written["train"], out["wavvq"], "device")
    ref_train, ref_test = str(tmp_path / "ref_train.npz"), str(tmp_path / "ref_test.npz")
    np.savez(ref_train, wavvq=want_train)
    np.savez(ref_test, wavvq=want_test)
    want = match(ref_train, ref_test, "restatement")
    assert got.ndim == 2 and got.shape[0] == M and got.dtype == np.int64 and np.array_equal(got, want)
