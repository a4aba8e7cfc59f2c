"""Training the generator on the device (qpgesture_amd/end2end.py) end to end: every gradient, the loss and the running
statistics against the f64 restatement (tests/generator_train_ref.py, itself pinned to the reference module's golden
vectors by tests/test_generator_train_cpu.py), the update against the library's own Adam, the golden 4-update trajectory,
determinism, resume, the eval side, that it learns, and the command line.

Tolerance: per tensor |device - f64| <= 8 e32, e32 = max |f32 run - f64 run| of the restatement on the same inputs; for
the four convolution biases in front of a train-mode BatchNorm, whose true gradient is zero, e32 is max |g32| of that
tensor.  Parameters after an update are never compared with a reference (a gradient within rounding of zero moves its
parameter by +-lr under Adam); eval-mode losses are compared only on the device's OWN trained weights."""
import os

import numpy as np
import pytest
import torch

from qpgesture_amd import end2end, synth
from qpgesture_amd.generate import load_generator, n_frames
from qpgesture_amd.optim import Adam
from tests import generator_train_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 8.0
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generator_train.npz")
SHAPES = ((3, 64000), (17, 7810), (2, 5866), (1, 66000))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def inputs(gold, i):
    """Runs 0..2 are the golden's own; run 3 (B 1, n 66 000) follows the same seeding."""
    B, n = SHAPES[i]
    wav = synth.make_wav(int(gold["seed_wav"]) + i, B, n)
    target = np.random.Generator(np.random.PCG64(int(gold["seed_target"]) + i)).integers(0, 512, (B, n_frames(n))).astype(np.int64)
    if i < 3:
        assert np.array_equal(target, gold["r%d_target" % i])
    return synth.make_generator_state_dict(int(gold["seed_w"])), wav, target


def compare(tag, loss, grads, running, r64, r32):
    worst = 0.0
    for name, got, a64, a32, zero in ([("loss", np.float64(loss), np.float64(r64[0]), np.float64(r32[0]), False)] +
                                      [(k, grads[k], r64[1][k], r32[1][k], k in ref.ZERO_GRAD_BIASES) for k in r64[1]] +
                                      [(k, running[k], r64[2][k], r32[2][k], False) for k in r64[2]]):
        got, a64, a32 = np.asarray(got, np.float64), np.asarray(a64, np.float64), np.asarray(a32, np.float64)
        assert got.shape == a64.shape and np.isfinite(got).all(), (tag, name)
        e32 = float(np.abs(a32).max()) if zero else float(np.abs(a32 - a64).max())
        err = float(np.abs(got - a64).max())
        ratio = err / e32 if e32 else float(err > 0)
        worst = max(worst, ratio)
        print("%s %s: err %.3e e32 %.3e ratio %.2f" % (tag, name, err, e32, ratio))
        assert err <= MARGIN * e32, "%s %s: |device - f64| = %.3e > %g x e32 (%.3e)" % (tag, name, err, MARGIN, e32)
    print("%s: worst ratio %.2f" % (tag, worst))


def device_run(sd, wav, target, mask=None, dropout=0.0):
    tr = end2end.GeneratorTrainer(device=DEV, dropout=dropout, state_dict=sd)
    loss = float(tr.forward_backward(wav, target, mask=mask))
    grads = {k: v.detach().cpu().numpy() for k, v in tr.gradients().items()}
    after = {k: v.numpy() for k, v in tr.state_dict(prefix="").items()}
    running = {k: v for k, v in after.items() if k.endswith(("running_mean", "running_var"))}
    assert all(int(after[q + "num_batches_tracked"]) == 1001 for q in end2end.BN_KEYS)
    return loss, grads, running


@pytest.mark.parametrize("i", range(4))
def test_gradients_end_to_end(gold, i):
    sd, wav, target = inputs(gold, i)
    r64, r32 = ref.loss_and_grads(sd, wav, target), ref.loss_and_grads(sd, wav, target, dtype=torch.float32)
    loss, grads, running = device_run(sd, wav, target)
    compare("B %d n %d" % SHAPES[i], loss, grads, running, r64, r32)
    if i < 3:                                                    # the reference module's own numbers, sampled
        pre, step = "r%d_" % i, int(gold["grad_step"])
        assert abs(loss - float(gold[pre + "loss64"])) <= MARGIN * abs(float(gold[pre + "loss32"]) - float(gold[pre + "loss64"]))
        for k, g in grads.items():
            e32 = float(gold[pre + ("n_" if k in ref.ZERO_GRAD_BIASES else "e_") + k])
            err = float(np.abs(g.reshape(-1)[::step].astype(np.float64) - gold[pre + "g_" + k]).max())
            assert err <= MARGIN * e32, (k, err, e32)
    # once more with a seeded mask at p = 0.1, against the restatement given the same mask
    B, T = target.shape
    mask = (np.random.Generator(np.random.PCG64(77 + i)).random((B, T, 400)) >= 0.1).astype(np.uint8)
    m64 = ref.loss_and_grads(sd, wav, target, mask=mask, drop_p=0.1)
    m32 = ref.loss_and_grads(sd, wav, target, mask=mask, drop_p=0.1, dtype=torch.float32)
    loss, grads, running = device_run(sd, wav, target, mask=mask, dropout=0.1)
    compare("B %d n %d dropout" % SHAPES[i], loss, grads, running, m64, m32)


def test_update_is_the_librarys_adam(gold):
    sd, wav, target = inputs(gold, 1)
    a = end2end.GeneratorTrainer(device=DEV, dropout=0.0, state_dict=sd)
    b = end2end.GeneratorTrainer(device=DEV, dropout=0.0, state_dict=sd)
    a.step(wav, target)
    b.forward_backward(wav, target)
    params = b.params.clone()
    opt = Adam((params, b.grads.clone()), lr=end2end.LR, betas=end2end.BETAS)
    opt.step()
    assert torch.equal(a.params, params) and not torch.equal(a.params, b.params)
    # the padding columns of out.weight stay exactly zero
    o = end2end.OFF["out.weight"]
    assert bool((a.params[o:o + 512 * 208].view(512, 208)[:, 200:] == 0).all())


def test_trajectory_of_four_updates(gold):
    sd = synth.make_generator_state_dict(int(gold["seed_w"]))
    tr = end2end.GeneratorTrainer(device=DEV, dropout=0.0, state_dict=sd)
    B, n = int(gold["traj_B"]), int(gold["traj_n"])
    losses = []
    for u in range(len(gold["traj_losses64"])):
        wav = synth.make_wav(int(gold["traj_seed_wav"]) + u, B, n)
        target = np.random.Generator(np.random.PCG64(int(gold["traj_seed_target"]) + u)).integers(0, 512, (B, n_frames(n)))
        losses.append(float(tr.step(wav, target.astype(np.int64))))
    err = np.abs(np.array(losses) - gold["traj_losses64"]).max()
    scale = np.abs(gold["traj_losses32"] - gold["traj_losses64"]).max()
    print("trajectory: losses %s, max err %.3e, scale %.3e, ratio %.2f" % (losses, err, scale, err / scale))
    assert err <= MARGIN * scale


def small_batches(n_updates, B=4, n=7810):
    out = []
    for u in range(n_updates):
        out.append((synth.make_wav(900 + u, B, n), np.random.Generator(np.random.PCG64(950 + u)).integers(0, 512, (B, n_frames(n)))))
    return out


def test_three_updates_twice_from_one_seed_are_bit_identical():
    sd = end2end.init_state_dict(11)
    runs = []
    for _ in range(2):
        tr = end2end.GeneratorTrainer(device=DEV, dropout=0.1, seed=5, state_dict=sd)
        for wav, target in small_batches(3):
            tr.step(wav, target)
        runs.append((tr.params.clone(), tr.running.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    other = end2end.GeneratorTrainer(device=DEV, dropout=0.1, seed=6, state_dict=sd)
    for wav, target in small_batches(3):
        other.step(wav, target)
    assert not torch.equal(other.params, runs[0][0])            # (the dropout stream matters)


def cli_args(tmp_path, extra):
    cfg = tmp_path / "cfg.yml"
    cfg.write_text("batch_size: 8\nend2end:\n  lr: 0.0002\n  betas: [0.99, 0.999]\n  epochs: 2\n  save_per_epochs: 1\n"
                   "  name: end2end\n  model_save_path: %s\n" % (tmp_path / "unused"))
    return end2end.build_parser().parse_args(["--config", str(cfg), "--synthetic", "16", "--batch_size", "8"] + extra)


def test_resume_continues_bit_identically(tmp_path):
    from qpgesture_amd.checkpoint import load_config
    quiet = lambda *a: None
    a = cli_args(tmp_path, ["--epochs", "2", "--model_save_path", str(tmp_path / "a")])
    losses_a, _, tr_a = end2end.train(a, load_config(a.config), log=quiet)
    assert len(losses_a) == 4
    # 2 updates (epoch 1), the checkpoint written at the head of epoch 2, then --resume for the other 2
    ckpts = sorted(os.listdir(tmp_path / "a"))
    assert "end2end_checkpoint_best.bin" in ckpts
    from qpgesture_amd.checkpoint import load_checkpoint
    at2 = [p for p in (str(tmp_path / "a" / c) for c in ckpts) if load_checkpoint(p)["epoch"] == 2]
    assert at2, ckpts
    b = cli_args(tmp_path, ["--epochs", "2", "--model_save_path", str(tmp_path / "b"), "--resume", at2[0]])
    losses_b, _, tr_b = end2end.train(b, load_config(b.config), log=quiet)
    assert losses_b == losses_a[2:]
    assert torch.equal(tr_a.params, tr_b.params) and torch.equal(tr_a.running, tr_b.running)
    assert torch.equal(tr_a.opt.exp_avg_sq, tr_b.opt.exp_avg_sq)


def test_eval_side_checkpoint_loads_and_matches(tmp_path):
    sd = end2end.init_state_dict(13)
    tr = end2end.GeneratorTrainer(device=DEV, dropout=0.1, seed=3, state_dict=sd)
    for wav, target in small_batches(2):
        tr.step(wav, target)
    wav, target = small_batches(3)[2]
    path = str(tmp_path / "ck.bin")
    end2end.save_checkpoint(path, None, 1, tr, None, (100.0, 0), 2)
    model = load_generator(path, device=DEV)
    loss_model = float(model.forward(wav, target)[1])
    loss_eval = float(tr.eval_loss(wav, target))
    assert loss_model == loss_eval
    own = tr.state_dict(prefix="")
    l64, l32 = ref.eval_loss(own, wav, target), ref.eval_loss(own, wav, target, dtype=torch.float32)
    print("eval loss %.8f, f64 %.8f, f32 off by %.3e, device off by %.3e" % (loss_eval, l64, abs(l32 - l64), abs(loss_eval - l64)))
    assert abs(loss_eval - l64) <= MARGIN * abs(l32 - l64)


def test_it_learns():
    wav, target = synth.make_wav(41, 8, 64000), np.random.Generator(np.random.PCG64(42)).integers(0, 512, (8, 30))
    tr = end2end.GeneratorTrainer(device=DEV, lr=end2end.LR, betas=end2end.BETAS, dropout=0.1, seed=1)
    wav_d, target_d = torch.from_numpy(wav).to(DEV), torch.from_numpy(target).to(DEV)
    losses = [tr.step(wav_d, target_d).clone() for _ in range(40)]
    first, last = float(losses[0]), float(losses[-1])
    print("loss %.4f -> %.4f (x %.3f)" % (first, last, last / first))
    assert last <= 0.75 * first


def test_command_line(tmp_path, capsys):
    from qpgesture_amd.checkpoint import load_checkpoint
    end2end.main(["--config", "missing.yml", "--synthetic", "32", "--batch_size", "8", "--epochs", "2", "--max_updates", "6",
                  "--model_save_path", str(tmp_path)])
    out = capsys.readouterr().out
    assert out.count("loss on validation:") == 2 and out.count("> epoch [") == 6
    assert "> epoch [1] updates[1] updates[0.00000000] loss[" in out
    ck = load_checkpoint(str(tmp_path / "end2end_checkpoint_best.bin"))
    assert {"args", "epoch", "model_dict"} <= set(ck)
    assert list(ck["model_dict"]) == ["module." + k for k in end2end.state_dict_keys()]
    load_generator(str(tmp_path / "end2end_checkpoint_best.bin"), device=DEV)


def test_build_dataset_codes_are_the_vqvaes_at_the_sampled_slices(tmp_path):
    from qpgesture_amd.vqvae import VQVAE
    hps = dict(width=64, emb_width=64, l_bins=96)
    vq = VQVAE(dict(vel=1, acc=1, commit=0.02, l_mu=0.99, reg=0.3, **hps), input_dim=135, device=DEV)
    vq.load_state_dict(synth.make_vqvae_state_dict(7, hps)).eval()
    rng = np.random.Generator(np.random.PCG64(61))
    F_ = 403                                                     # not a multiple of 8: the last 3 frames have no code
    poses = rng.standard_normal((F_, 135)).astype(np.float32)
    audio = synth.make_wav(62, 1, int(F_ * 16000 / 60) + 1)[0]
    data = end2end.build_dataset([(poses, audio)], vq, stride=13)
    codes_all = vq.encode(torch.from_numpy(poses[None, :400]))[0].reshape(-1).cpu().numpy()
    assert len(np.unique(codes_all)) > 4
    n = (400 - 240) // 13 + 1
    assert data["audio"].shape == (n, 64000) and data["codes"].shape == (n, 30) and data["codes"].dtype == np.int64
    for i in range(n):
        start = 13 * i
        assert np.array_equal(data["codes"][i], codes_all[start // 8:(start + 240) // 8])
        a0 = int(np.floor(start / F_ * len(audio)))
        assert np.array_equal(data["audio"][i], audio[a0:a0 + 64000])
    path = str(tmp_path / "train.npz")
    np.savez(path, **data)
    back = end2end.load_npz(path)
    assert np.array_equal(back[0], data["audio"]) and np.array_equal(back[1], data["codes"])
