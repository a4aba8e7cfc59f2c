"""PAE training, host side (no GPU): the schedule, AdamW, the test-side step restatement against the reference's own
steps (tests/golden/pae_train_s11.npz), window enumeration, the parameter layout and the CLI."""
import os

import numpy as np
import pytest
import torch

from qpgesture_amd import PAE_train as PT, synth
from qpgesture_amd.checkpoint import load_config
from tests import pae_train_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pae_train_s11.npz")
CFG = os.path.join(os.path.dirname(PT.__file__), "configs", "codebook.yml")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def golden_windows(gold):
    seed, mseed, n_win = (int(v) for v in gold["meta"][:3])
    cfg = load_config(CFG)
    mean = np.asarray(cfg.data_mean, np.float64)
    std = np.clip(np.asarray(cfg.data_std, np.float64), 0.01, None)
    pn = PT.normalise(synth.make_pae_motion(n_win + 239, mseed), mean, std)
    return synth.make_pae_state_dict(seed), pn


def test_schedule_matches_reference_trace(gold):
    n, epochs = (int(v) for v in gold["sched_meta"])
    s = PT.Schedule(n)
    got = []
    for _ in range(epochs):
        s.epoch_start()
        for _ in range(n):
            got.append((s.lr, s.wd))
            s.after_update()
    got = np.array(got)
    want = gold["sched_trace"]
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert s.restarts == 3                         # restarts at epochs 10, 30 and 70


def test_adamw_restatement_matches_reference(gold):
    p = gold["adamw_p0"].astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for k in range(5):
        lr, wd = gold["adamw_lr_wd"][k]
        p, m, v = R.adamw_step(p, gold["adamw_g"][k].astype(np.float64), m, v, lr, wd, k + 1)
        np.testing.assert_allclose(p, gold["adamw_p"][k], rtol=0, atol=2e-6 * (1 + np.abs(p)).max())


def test_layout_and_state_dict_round_trip(gold):
    sd = synth.make_pae_state_dict(3)
    P, S, nbt = PT.pack(sd)
    assert P.size == PT.PARAM_FLOATS == 1034098 and S.size == PT.STATS_FLOATS == 108 and nbt == 1000
    back = PT.unpack(P, S, nbt)
    assert list(back) == list(gold["sd_keys"])
    for k, shape, dt in zip(gold["sd_keys"], gold["sd_shapes"], gold["sd_dtypes"]):
        assert tuple(back[k].shape) == tuple(int(d) for d in shape.split(";") if d), k
        assert str(back[k].dtype).replace("torch.", "") == dt, k
        np.testing.assert_array_equal(back[k].numpy(), np.asarray(sd[k]))
    # `module.` prefixes are accepted; the parameter order is named_parameters()'s
    P2, _, _ = PT.pack({"module." + k: v for k, v in sd.items()})
    np.testing.assert_array_equal(P, P2)
    trainable = [n for n, _ in PT.PARAMS if PT.OFF[n] >= PT.TRAINABLE]
    assert trainable == list(gold["trainable"])
    with pytest.raises(ValueError):
        PT.pack({k: v for k, v in sd.items() if k != "conv2.bias"})
    init = PT.init_state_dict(7)
    assert list(init) == list(gold["sd_keys"])
    assert torch.equal(init["conv1.weight"], PT.init_state_dict(7)["conv1.weight"])
    assert float(init["conv1.weight"].abs().max()) <= 1 / np.sqrt(135 * 240)


def test_header_offsets_match_layout():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(PT.__file__)), "include", "qpg.h")).read()
    want = {"OFF_TPI": "tpi", "OFF_ARGS": "args", "OFF_FREQS": "freqs", "OFF_CONV1_W": "conv1.weight",
            "OFF_CONV1_B": "conv1.bias", "OFF_BN1": "bn_conv1.weight", "OFF_CONV2_W": "conv2.weight",
            "OFF_CONV2_B": "conv2.bias", "OFF_BN2": "bn_conv2.weight", "OFF_FC": "fc.0.weight", "OFF_FCBN": "bn.0.weight",
            "OFF_DECONV1_W": "deconv1.weight", "OFF_DECONV1_B": "deconv1.bias", "OFF_BN3": "bn_deconv1.weight",
            "OFF_DECONV2_W": "deconv2.weight", "OFF_DECONV2_B": "deconv2.bias"}
    for macro, name in want.items():
        assert "#define QPG_PAET_%s %d\n" % (macro, PT.OFF[name]) in hdr, macro
    assert "#define QPG_PAET_PARAM_FLOATS %d\n" % PT.PARAM_FLOATS in hdr
    assert "#define QPG_PAET_TRAINABLE %d\n" % PT.TRAINABLE in hdr
    for macro, name in (("ST_BN1", "bn_conv1"), ("ST_BN2", "bn_conv2"), ("ST_FCBN", "bn.0"), ("ST_BN3", "bn_deconv1")):
        assert "#define QPG_PAET_%s %d\n" % (macro, PT.ST_OFF[name + ".running_mean"]) in hdr
    assert PT.OFF["fc.1.weight"] - PT.OFF["fc.0.weight"] == 482 and PT.OFF["bn.1.weight"] - PT.OFF["bn.0.weight"] == 4


def test_window_enumeration():
    # floor((T - 240) / stride) + 1 windows per clip, none for a clip shorter than 240
    got = PT.window_starts([239, 240, 250, 100, 245], 240, 1)
    want = np.concatenate([[239], 479 + np.arange(11), 829 + np.arange(6)])     # clip offsets 0, 239, 479, 729, 829
    np.testing.assert_array_equal(got, want)
    got = PT.window_starts([300, 512], 240, 32)
    np.testing.assert_array_equal(got, np.concatenate([[0, 32], 300 + 32 * np.arange((512 - 240) // 32 + 1)]))
    assert PT.window_starts([10, 20], 240, 1).size == 0


BIAS_BEFORE_BN = {"conv1.bias", "conv2.bias", "deconv1.bias"} | {"fc.%d.bias" % e for e in range(8)}


def assert_params_close(got, gold, s, n, gtol):
    """Sampled parameters after step s: within 1e-6 (+ 1e-5 relative), except weights whose gradient is below the
    gradient tolerance in some step so far - Adam normalises such a noise gradient to a +-lr move of either sign."""
    want = gold["p_%d_%s" % (s, n)]
    bad = np.abs(got - want) > 1e-6 + 1e-5 * float(np.abs(want).max())
    tiny = np.zeros_like(bad)
    for k in range(s + 1):
        tiny |= np.abs(gold["g_%d_%s" % (k, n)]) < gtol
    assert not (bad & ~tiny).any(), (n, s, np.flatnonzero(bad & ~tiny)[:5])
    assert np.abs(got - want).max() <= 2.5 * (s + 1) * 1e-4, n        # a noise-driven weight moves <= lr per step


def test_restatement_reproduces_reference_steps(gold):
    """The f32 restatement run the reference's way (validation pass, then 3 steps with AdamW and the schedule) lands
    on the golden losses, gradients, parameters and running statistics: the checker is the reference's model."""
    sd, pn = golden_windows(gold)
    P, S, nbt = PT.pack(sd)
    B, n_win = int(gold["meta"][3]), int(gold["meta"][2])
    p = R.params_from_flat(P, torch.float32)
    st = R.stats_from_flat(S, torch.float32)
    pn_t = torch.from_numpy(pn)
    with torch.no_grad():
        vals = [float(R.forward(p, st, R.windows_input(pn_t, range(i, i + B), False), False)["loss"])
                for i in range(0, n_win, B)]
    np.testing.assert_allclose(vals, gold["val_losses"], rtol=2e-5)
    sched = PT.Schedule(n_win // B)
    sched.epoch_start()
    m = {n: torch.zeros_like(v) for n, v in p.items()}
    v2 = {n: torch.zeros_like(v) for n, v in p.items()}
    perm = gold["perm"]
    for s in range(3):
        x = R.windows_input(pn_t, perm[s * B:(s + 1) * B], True)
        r = R.forward(p, st, x, True)
        for t in p.values():
            t.grad = None
        r["loss"].backward()
        np.testing.assert_allclose(float(r["loss"].detach()), gold["losses"][s], rtol=2e-5)
        assert (sched.lr, sched.wd) == pytest.approx((gold["lrs"][s], gold["wds"][s]), rel=1e-12)
        if s == 0:
            for k in "pfab":
                np.testing.assert_allclose(r[k].detach().numpy(), gold["step1_" + k], rtol=1e-4, atol=2e-5)
        gtol = {}
        for n in gold["trainable"]:
            g = p[n].grad.reshape(-1).numpy()
            idx = np.unique(np.linspace(0, g.size - 1, 97).round().astype(np.int64))
            gn = float(gold["gnorm_%d_%s" % (s, n)])
            if n in BIAS_BEFORE_BN:
                # the true gradient is 0 (train-mode BN removes the mean): both sides hold rounding noise
                scale = float(gold["gnorm_%d_%s" % (s, n.replace(".bias", ".weight"))])
                gtol[n] = 1e-5 * scale
                assert np.linalg.norm(g) < gtol[n] and gn < gtol[n], n
                continue
            gtol[n] = 2e-3 * gn / np.sqrt(g.size) + 1e-9
            np.testing.assert_allclose(np.linalg.norm(g.astype(np.float64)), gn, rtol=1e-3, atol=1e-9)
            np.testing.assert_allclose(g[idx], gold["g_%d_%s" % (s, n)], rtol=0, atol=gtol[n])
        with torch.no_grad():
            for n in gold["trainable"]:
                pn_, m[n], v2[n] = R.adamw_step(p[n], p[n].grad, m[n], v2[n], sched.lr, sched.wd, s + 1)
                p[n].copy_(pn_)
        sched.after_update()
        for n in gold["trainable"]:
            idx = np.unique(np.linspace(0, p[n].numel() - 1, 97).round().astype(np.int64))
            assert_params_close(p[n].detach().reshape(-1).numpy()[idx], gold, s, n, gtol[n])
        for n, _ in PT.STATS:
            np.testing.assert_allclose(st[n].numpy(), gold["buf_%d_%s" % (s, n)], rtol=1e-4, atol=1e-6)
        assert int(gold["buf_%d_bn_conv1.num_batches_tracked" % s]) == nbt + s + 1


def test_cli_arguments():
    a = PT.build_parser().parse_args(["--config", "x.yml", "--gpu", "1", "--synthetic", "512", "--epochs", "2",
                                      "--batch_size", "64", "--max_updates", "5", "--model_save_path", "out"])
    assert (a.stage, a.gpu, a.synthetic, a.epochs, a.batch_size, a.max_updates, a.model_save_path, a.seed) == \
        ("train", "1", 512, 2, 64, 5, "out", 23456)
    with pytest.raises(SystemExit):
        PT.main(["--stage", "inference"])
    with pytest.raises(SystemExit):
        PT.main([])                                   # no data
    from qpgesture_amd import PAE
    with pytest.raises(SystemExit, match="out of scope"):
        PAE.main(["--stage", "train"])
