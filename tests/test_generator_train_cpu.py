"""Generator training without a GPU: the f64 restatement (tests/generator_train_ref.py) is pinned to the golden vectors
taken from the reference module (tests/golden/make_golden_generator_train.py); sample_windows against the reference's own
window arithmetic; the flat layout's pack / unpack round trip; the parser."""
import os

import numpy as np
import pytest
import torch

from qpgesture_amd import end2end, synth

from tests import generator_train_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generator_train.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def run_inputs(gold, i):
    B, n = int(gold["r%d_B" % i]), int(gold["r%d_n" % i])
    return synth.make_generator_state_dict(int(gold["seed_w"])), synth.make_wav(int(gold["seed_wav"]) + i, B, n), gold["r%d_target" % i]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_restatement_is_pinned_to_the_reference(gold, i):
    """Both sides f64: per tensor |restated - golden| <= 1e-9 max|g64| on the sampled entries and on the sum (four orders
    below e32, far above f64 rounding); the four zero-gradient biases stay under the golden's own 1e-9; loss and running
    statistics likewise."""
    sd, wav, target = run_inputs(gold, i)
    loss, grads, running = ref.loss_and_grads(sd, wav, target)
    pre, step = "r%d_" % i, int(gold["grad_step"])
    assert abs(loss - float(gold[pre + "loss64"])) <= 1e-9 * abs(float(gold[pre + "loss64"]))
    worst = 0.0
    for k, g in grads.items():
        m = float(gold[pre + "m_" + k])
        if k in ref.ZERO_GRAD_BIASES:
            assert np.abs(g).max() <= 1e-9, k
            continue
        if m == 0.0:
            assert np.all(g == 0), k
            continue
        err = np.abs(g.reshape(-1)[::step] - gold[pre + "g_" + k]).max() / m
        serr = abs(g.sum() - float(gold[pre + "s_" + k])) / (m * max(1.0, np.sqrt(g.size)))
        worst = max(worst, err, serr)
        assert err <= 1e-9 and serr <= 1e-9, (k, err, serr)
    for k, v in running.items():
        assert np.abs(v - gold[pre + "v_" + k]).max() <= 1e-9 * max(1.0, np.abs(v).max()), k
    print("run %d: worst relative gradient error %.2e" % (i, worst))


def test_sample_windows_matches_the_reference_lines(gold):
    rows, at = gold["win_rows"], 0
    for (n_frames, n_audio, n_raw, stride), count in zip(gold["win_cases"], gold["win_counts"]):
        want = rows[at:at + count]
        at += count
        audio_raw, code_raw = np.arange(n_audio, dtype=np.float32), np.arange(1000, 1000 + n_raw)
        short = [r for r in want if r[2] != 64000 or r[4] != 30]
        if short:
            with pytest.raises(ValueError):
                end2end.sample_windows(audio_raw, code_raw, n_frames, stride=int(stride))
            continue
        audio, codes, starts = end2end.sample_windows(audio_raw, code_raw, n_frames, stride=int(stride))
        assert len(audio) == count and audio.shape[1:] == (64000,) and codes.shape[1:] == (30,) and codes.dtype == np.int64
        for a, c, s, r in zip(audio, codes, starts, want):
            assert s == r[0] and a[0] == r[1] and a[-1] == r[1] + 63999 and c[0] == r[3] and c[-1] == r[3] + 29


def test_sample_windows_raises_on_short_audio():
    # MINLEN (whole pose frames of audio) admits the window, its slice of the clip is one sample short of what is asked for
    with pytest.raises(ValueError, match="audio"):
        end2end.sample_windows(np.zeros(64000, np.float32), np.arange(30), 240, stride=10, audio_sample_length=64001)
    assert len(end2end.sample_windows(np.zeros(64000, np.float32), np.arange(30), 240, stride=10)[0]) == 1


def test_pack_unpack_round_trip():
    sd = synth.make_generator_state_dict(5)
    P, S, nbt = end2end.pack(sd)
    assert P.shape == (end2end.PARAM_FLOATS,) and nbt == [1000] * 4
    back = end2end.unpack(P, S, nbt, prefix="module.")
    assert list(back) == ["module." + k for k in end2end.state_dict_keys()]
    for k, v in sd.items():
        assert tuple(back[k].shape) == tuple(np.asarray(v).shape), k
        assert np.array_equal(back[k].numpy(), np.asarray(v)), k
    # the stored layouts: convolution weights [Cout][16][Cin], out.weight rows of 208 with zero padding
    flat = torch.from_numpy(P)
    w = np.asarray(sd["module.WavEncoder.feat_extractor.3.weight"])
    o = end2end.OFF["WavEncoder.feat_extractor.3.weight"]
    assert np.array_equal(P[o:o + w.size].reshape(16, 16, 8), w.transpose(0, 2, 1))
    o = end2end.OFF["out.weight"]
    assert np.all(P[o:o + 512 * 208].reshape(512, 208)[:, 200:] == 0)
    assert end2end.view(flat, "out.weight").shape == (512, 200)
    total = sum(int(np.prod(end2end.torch_shape(k))) for k, _, _ in end2end.LAYOUT)
    assert total == sum(np.asarray(v).size for k, v in sd.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    with pytest.raises(KeyError):
        end2end.pack({k: v for k, v in sd.items() if not k.endswith("norm.bias")})


def test_init_state_dict_is_seeded_and_torch_shaped():
    a, b, c = end2end.init_state_dict(3), end2end.init_state_dict(3), end2end.init_state_dict(4)
    assert list(a) == end2end.state_dict_keys()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["out.weight"], c["out.weight"])
    assert float(a["WavEncoder.feat_extractor.1.weight"].min()) == 1.0 and int(a["WavEncoder.feat_extractor.1.num_batches_tracked"]) == 0
    assert float(a["project.weight_hh_l1_reverse"].abs().max()) <= 1.0 / np.sqrt(200.0)


def test_parser_and_settings():
    a = end2end.build_parser().parse_args(["--synthetic", "32", "--batch_size", "8", "--epochs", "2", "--max_updates", "6"])
    assert (a.synthetic, a.batch_size, a.epochs, a.max_updates, a.resume, a.gpu) == (32, 8, 2, 6, None, "0")
    from qpgesture_amd.checkpoint import AttrDict
    e = end2end.settings(AttrDict({}))
    assert (e["lr"], tuple(e["betas"]), e["epochs"], e["save_per_epochs"], e["name"]) == (0.0002, (0.99, 0.999), 100, 10, "end2end")
    assert end2end.settings(AttrDict({"end2end": {"epochs": 3}}))["epochs"] == 3
