"""The GRU speech-to-code generator end to end on the device (qpgesture_amd/generate.py over qpg_gen.hip and the WavLM
GEMM) against the reference model's f64 run of the same seeded weights and audio (tests/golden/generator_*.npz; weights and
audio are regenerated from synth, nothing here imports the reference).

Tolerance: every tap of the device run is within MARGIN = 8 x e32 of the f64 value, e32 = max |the reference's f32 run -
its f64 run| over the whole tensor of the same tap, read from the fixture (the rule of tests/test_gpu_wavlm.py and
tests/test_gpu_sentence.py).  Each check prints its ratio first.  The fixtures were chosen with a smallest top-2 logit gap
of at least 64 x e32_logits, so the codes are compared EXACTLY, at every position.
Measured on an MI355X: see the table in profiles/generator_bench.md."""
import os
import wave

import numpy as np
import pytest
import torch

from qpgesture_amd import generate as G
from qpgesture_amd import synth
from tests.test_generator_cpu import TAPS, runs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 8.0
NAMES = ["full", "n5866", "n7810", "n66000"]
STAGE_OF = dict(enc="conv5", gru0="gru0", gru1="gru1", ln="ln", logits="logits")
_state = {}


def model_of(golden_dir):
    if "model" not in _state:
        _state["model"] = G.Generator_gru(device=DEV).load_state_dict(runs(golden_dir)[0][4])
    return _state["model"]


def run_of(golden_dir, name):
    return next(r for r in runs(golden_dir) if r[0] == name)


def check(name, got, ref64, e32):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert np.isfinite(got).all(), name
    err = float(np.abs(got - ref64).max())
    print("%s: err %.3e e32 %.3e ratio %.2f" % (name, err, e32, err / e32))
    assert err <= MARGIN * e32, "%s: |device - f64| = %.3e > %g x e32 (%.3e)" % (name, err, MARGIN, e32)


@pytest.mark.parametrize("name", NAMES)
def test_taps_and_codes_against_f64(golden_dir, name):
    _, g, pre, wav, _ = run_of(golden_dir, name)
    model = model_of(golden_dir)
    taps = {}
    codes = model.codes(wav, on_stage=lambda stage, view: taps.__setitem__(stage, None if view is None else view.clone()))
    rows = torch.from_numpy(g[pre + "tap_rows"].astype(np.int64)).to(DEV)
    for tap in TAPS:
        t = taps[STAGE_OF[tap]]
        t = t.reshape(-1, t.shape[-1])
        if tap == "ln":
            assert not t[:, G.HIDDEN:].any()                  # the padding columns the head's GEMM reads
            t = t[:, :G.HIDDEN]
        check("%s %s" % (name, tap), t[rows], g[pre + tap], float(g[pre + "e32_" + tap]))
    want = g[pre + "codes"]
    assert codes.dtype == torch.int64 and codes.device.type == "cuda" and tuple(codes.shape) == want.shape
    assert np.array_equal(codes.cpu().numpy(), want), "%d of %d codes differ" % (
        int((codes.cpu().numpy() != want).sum()), want.size)
    assert torch.equal(codes, taps["codes"]) and torch.equal(codes, model.codes(torch.from_numpy(wav).to(DEV)))


def test_sample_is_the_flattened_codes(golden_dir):
    _, g, _, wav, _ = run_of(golden_dir, "full")
    model = model_of(golden_dir)
    out = model.sample(wav)
    assert isinstance(out, list) and len(out) == 1
    z = out[0]
    assert z.dtype == torch.int64 and z.device.type == "cuda" and tuple(z.shape) == (1, 6 * 30)
    assert torch.equal(z, model.codes(wav).reshape(1, -1))
    assert np.array_equal(z.cpu().numpy(), g["codes"].reshape(1, -1))
    one = model.codes(wav[2])                                     # (n,) is a batch of one
    assert tuple(one.shape) == (1, 30) and np.array_equal(one.cpu().numpy()[0], g["codes"][2])
    with pytest.raises(ValueError, match="5865"):
        model.codes(np.zeros(5865, np.float32))


@pytest.mark.parametrize("name", NAMES)
def test_forward_loss_against_f64(golden_dir, name):
    _, g, pre, wav, _ = run_of(golden_dir, name)
    model = model_of(golden_dir)
    logits, none = model.forward(wav)
    assert none is None and tuple(logits.shape) == g[pre + "codes"].shape + (512,) and logits.dtype == torch.float32
    logits2, loss = model(wav, g[pre + "target"])
    assert torch.equal(logits, logits2) and loss.dtype == torch.float32 and loss.dim() == 0 and loss.device.type == "cuda"
    l64, e32 = float(g[pre + "loss64"]), abs(float(g[pre + "loss32"]) - float(g[pre + "loss64"]))
    err = abs(float(loss) - l64)
    print("%s loss: device %.8f f64 %.8f err %.3e e32 %.3e ratio %.2f" % (name, float(loss), l64, err, e32, err / e32))
    assert err <= MARGIN * e32
    with pytest.raises(ValueError, match="targets"):
        model.forward(wav, np.full(g[pre + "codes"].shape, 512))


def test_any_split_of_the_batch_gives_the_same_bits(golden_dir):
    _, _, _, wav, _ = run_of(golden_dir, "full")
    model = model_of(golden_dir)
    whole = model.logits(wav).clone()
    for cut in (1, 3):
        parts = torch.cat([model.logits(wav[:cut]).clone(), model.logits(wav[cut:]).clone()])
        assert torch.equal(parts, whole), cut
    assert torch.equal(model.logits(wav, max_batch=4), whole)
    assert torch.equal(model.logits(wav[::-1].copy()), whole.flip(0))
    big = np.concatenate([wav] * 3)[:17]                          # two recurrence tiles, the second one partial
    assert torch.equal(model.logits(big)[12:17], whole[:5])


def _write_wav(path, samples):
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(samples.astype("<i2").tobytes())


def test_cli_end_to_end(golden_dir, tmp_path):
    from qpgesture_amd import VisualizeCodebook as vis
    from qpgesture_amd import wavlm
    from qpgesture_amd.checkpoint import denormalize_poses, load_config
    from qpgesture_amd.vqvae import VQVAE
    n = int(2.3 * 64000)
    pcm = np.round(synth.make_wav(31, 1, n)[0] * 32767.0).astype(np.int16)
    wav_path = str(tmp_path / "clip.wav")
    _write_wav(wav_path, pcm)
    gen_sd = runs(golden_dir)[0][4]
    vq_sd = dict(synth.make_vqvae_state_dict(7))
    # (the output convolution scaled down and its bias dropped: the de-normalised poses stay close to the configuration's
    # mean pose - proper rotation matrices, which the BVH step accepts; tests/test_gpu_takes_cli.py does the same)
    vq_sd["module.decoders.0.out.weight"] = vq_sd["module.decoders.0.out.weight"] * np.float32(0.02)
    vq_sd["module.decoders.0.out.bias"] = vq_sd["module.decoders.0.out.bias"] * np.float32(0.0)
    e2e, ck = str(tmp_path / "E.bin"), str(tmp_path / "CK.bin")
    torch.save({"args": {}, "epoch": 80, "model_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in gen_sd.items()}}, e2e)
    torch.save({"args": {}, "epoch": 1, "model_dict": {k: torch.from_numpy(v) for k, v in vq_sd.items()}}, ck)
    cfg_path = os.path.join(os.path.dirname(os.path.abspath(vis.__file__)), "configs", "codebook.yml")
    out = str(tmp_path / "out")
    poses, codes = G._cli(["--wav", wav_path, "--end2end_model_path", e2e, "--config", cfg_path, "--VQVAE_model_path", ck,
                           "--save_path", out, "--prefix", "P"])
    assert codes.shape == (3, 30) and codes.dtype == np.int64
    audio = wavlm.read_wav_16k(wav_path)
    assert len(audio) == n
    hand = np.zeros((3, 64000), np.float32)
    hand[0], hand[1], hand[2, :n - 128000] = audio[:64000], audio[64000:128000], audio[128000:]
    model = model_of(golden_dir)
    assert np.array_equal(codes, model.sample(hand)[0].cpu().numpy().reshape(3, 30))
    cfg = load_config(cfg_path)
    vq = VQVAE(cfg.VQVAE, 15 * 9, device=DEV).load_state_dict(vq_sd)
    want = denormalize_poses(vq.decode([torch.from_numpy(codes.reshape(1, -1))]).squeeze(0).cpu().numpy(), cfg.data_mean,
                             cfg.data_std)
    assert poses.shape == (3 * 240, 135) and np.array_equal(poses, want)
    assert np.array_equal(np.load(os.path.join(out, "codeP.npy")), codes)
    assert np.array_equal(np.load(os.path.join(out, "generateP.npy")), poses)
    assert os.path.exists(os.path.join(out, "P_generated.bvh")) and os.path.exists(os.path.join(out, "P_euler.npy"))
    out15 = str(tmp_path / "out15")
    poses15, codes15 = G._cli(["--wav", wav_path, "--end2end_model_path", e2e, "--config", cfg_path, "--VQVAE_model_path", ck,
                               "--save_path", out15, "--prefix", "Q", "--max_frames", "3600", "--no_bvh"])
    assert codes15.shape == (15, 30) and poses15.shape == (15 * 240, 135)
    assert np.array_equal(codes15[:3], codes)
    assert (codes15[3:] == codes15[3]).all()                      # the windows past the clip are all zeros: one window, twelve times
    assert not os.path.exists(os.path.join(out15, "Q_generated.bvh"))
