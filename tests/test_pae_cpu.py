"""Phase extraction (qpgesture_amd/PAE.py), the host side: checkpoint loading, refusals, CLI parsing and the parameter
block of qpg_pae_phase_f32 against its definition (include/qpg.h) - including an f64 walk of the kernel's own index maps
over that block, for a few frames, against the reference's outputs (tests/golden/pae_s11.npz)."""
import os

import numpy as np
import pytest
import torch

from qpgesture_amd import PAE, synth
from qpgesture_amd.checkpoint import load_config
from tests.helpers import load_golden

SEED = 11


def _save(tmp_path, sd, name="pae.bin"):
    p = str(tmp_path / name)
    torch.save({"args": {"x": 1}, "epoch": 70, "model_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, p)
    return p


def test_checkpoint_loads_with_and_without_module_prefix(tmp_path):
    a = PAE.state_dict_from(_save(tmp_path, synth.make_pae_state_dict(SEED), "a.bin"))
    b = PAE.state_dict_from(_save(tmp_path, synth.make_pae_state_dict(SEED, prefix="module."), "b.bin"))
    assert set(PAE.REQUIRED) <= set(a) and set(a) == set(b)
    for k in PAE.REQUIRED:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(PAE.pack_params(a), PAE.pack_params(b))


def test_checkpoint_refuses_missing_key_and_wrong_shape(tmp_path):
    sd = synth.make_pae_state_dict(SEED)
    del sd["bn.3.running_var"]
    with pytest.raises(ValueError, match="bn.3.running_var"):
        PAE.state_dict_from(_save(tmp_path, sd))
    sd = synth.make_pae_state_dict(SEED)
    sd["conv1.weight"] = sd["conv1.weight"][:, :, :239]
    with pytest.raises(ValueError, match="conv1.weight"):
        PAE.state_dict_from(sd)


def test_cli_arguments():
    p = PAE.build_parser()
    a = p.parse_args(["--config", "c.yml", "--gpu", "0", "--stage", "inference"])
    assert (a.config, a.gpu, a.stage) == ("c.yml", "0", "inference")
    assert a.PAE_model_path == "../pretrained_model/PAE_checkpoint_070.bin"
    assert a.rotation_dir == "../dataset/BEAT/speaker_10_state_0/Rotation"
    assert a.phase_dir == "../dataset/BEAT/speaker_10_state_0/Phase"
    a = p.parse_args(["--stage", "inference", "--rotation_dir", "R", "--phase_dir", "Ph", "--PAE_model_path", "m.bin"])
    assert (a.rotation_dir, a.phase_dir, a.PAE_model_path) == ("R", "Ph", "m.bin")
    with pytest.raises(SystemExit, match="out of scope"):
        PAE.main(["--stage", "train"])


def test_param_block_matches_its_definition():
    """include/qpg.h: W1[tap][group][lane] = conv1.weight[lane & 15][4 group + (lane >> 4)][tap] (0 for o = 15, c = 135),
    W2 likewise for conv2 (0 for e >= 8, o = 15), BN blocks [bias, alpha, beta] with alpha = weight / sqrt(var + eps)."""
    sd = PAE.state_dict_from(synth.make_pae_state_dict(SEED))
    P = PAE.pack_params(sd)
    assert P.shape == (PAE.PARAM_FLOATS,) and P.dtype == np.float32
    w1 = P[PAE.OFF["W1"]:PAE.OFF["BN1"]].reshape(240, 34, 64)
    for (tap, grp, lane) in [(0, 0, 0), (239, 33, 63), (17, 5, 22), (120, 33, 47), (3, 33, 15), (100, 12, 31)]:
        o, c = lane & 15, 4 * grp + (lane >> 4)
        want = sd["conv1.weight"][o, c, tap] if (o < 15 and c < 135) else 0.0
        assert w1[tap, grp, lane] == want, (tap, grp, lane)
    w2 = P[PAE.OFF["W2"]:PAE.OFF["BN2"]].reshape(240, 4, 64)
    for (tap, grp, lane) in [(0, 0, 0), (239, 3, 55), (5, 2, 7), (9, 1, 8), (200, 3, 23)]:
        e, o = lane & 15, 4 * grp + (lane >> 4)
        want = sd["conv2.weight"][e, o, tap] if (e < 8 and o < 15) else 0.0
        assert w2[tap, grp, lane] == want, (tap, grp, lane)
    for key, conv, bn, n in (("BN1", "conv1", "bn_conv1", 15), ("BN2", "conv2", "bn_conv2", 8)):
        blk = P[PAE.OFF[key]:PAE.OFF[key] + 48].reshape(3, 16)
        alpha = sd[bn + ".weight"] / np.sqrt(sd[bn + ".running_var"].astype(np.float64) + 1e-5)
        assert np.array_equal(blk[0, :n], sd[conv + ".bias"]) and not blk[:, n:].any()
        assert np.allclose(blk[1, :n], alpha, rtol=1e-7)
        assert np.allclose(blk[2, :n], sd[bn + ".bias"] - sd[bn + ".running_mean"] * alpha, rtol=1e-6, atol=1e-8)
    fc = P[PAE.OFF["FC"]:PAE.OFF["FCBN"]].reshape(8, 2, 240)
    fb = P[PAE.OFF["FCBN"]:PAE.OFF["FCBN"] + 48].reshape(3, 8, 2)
    for e in range(8):
        assert np.array_equal(fc[e], sd["fc.%d.weight" % e]) and np.array_equal(fb[0, e], sd["fc.%d.bias" % e])
        assert np.allclose(fb[1, e], sd["bn.%d.weight" % e] / np.sqrt(sd["bn.%d.running_var" % e] + 1e-5), rtol=1e-6)
    assert np.array_equal(P[PAE.OFF["FREQ"]:PAE.OFF["FREQ"] + 120], sd["freqs"]) and P[PAE.OFF["TPI"]] == sd["tpi"][0]


def _kernel_walk(P, vel, T, i):
    """What pae_phase_kernel computes for frame i of a clip (f64): the window staged at LDS column s + 16, conv1 reading
    column t + k - 104 and conv2 column u + k - 103 through the packed W1 / W2, BN blocks, DFT, fc, atan2'."""
    O = PAE.OFF
    L = np.zeros((136, 272))
    for p in range(272):
        s, j = p - 16, i + p - 16 - 121
        if 1 <= s < 240 and 0 <= j <= T - 2:
            L[:135, p] = vel[j]
    W1 = P[O["W1"]:O["BN1"]].astype(np.float64).reshape(240, 136, 16)
    W2 = P[O["W2"]:O["BN2"]].astype(np.float64).reshape(240, 16, 16)
    b1, b2, fb = (P[O[k]:O[k] + 48].astype(np.float64).reshape(3, 16) for k in ("BN1", "BN2", "FCBN"))
    y1 = np.zeros((16, 272))
    k = np.arange(240)
    for t in range(241):
        col = t + k - 104
        ok = (col >= 0) & (col < 272)
        y1[:, t + 16] = np.tanh((np.einsum("ck,kco->o", L[:, col[ok]], W1[ok]) + b1[0]) * b1[1] + b1[2])
    lat = np.zeros((8, 240))
    for u in range(240):
        col = u + k - 103
        ok = (col >= 0) & (col < 272)
        lat[:, u] = np.tanh((np.einsum("ck,kce->e", y1[:, col[ok]], W2[ok]) + b2[0]) * b2[1] + b2[2])[:8]
    X = np.fft.rfft(lat, axis=1)
    pw = np.abs(X[:, 1:]) ** 2
    f = pw @ P[O["FREQ"]:O["FREQ"] + 120].astype(np.float64) / pw.sum(1) / (13 / 240)
    a, b = 2 * np.sqrt(pw.sum(1)) / 240, X[:, 0].real / 240
    fc = P[O["FC"]:O["FCBN"]].astype(np.float64).reshape(8, 2, 240)
    v = ((np.einsum("eju,eu->ej", fc, lat) + fb[0].reshape(8, 2)) * fb[1].reshape(8, 2) + fb[2].reshape(8, 2))
    v = v.astype(np.float32)
    tpi = P[O["TPI"]]
    with np.errstate(all="ignore"):
        ang = np.arctan(v[:, 1] / v[:, 0])
    ang = np.where((v[:, 0] < 0) & (v[:, 1] >= 0), ang + np.float32(0.5) * tpi, ang)
    ang = np.where((v[:, 0] < 0) & (v[:, 1] < 0), ang - np.float32(0.5) * tpi, ang)
    return np.stack([ang / tpi, f, a, b]), v, lat


def test_kernel_index_maps_reproduce_the_reference():
    g = load_golden("pae_s11")
    P = PAE.pack_params(PAE.state_dict_from(synth.make_pae_state_dict(int(g["meta"][0]))))
    cfg = load_config(os.path.join(os.path.dirname(PAE.__file__), "configs", "codebook.yml"))
    mean, std = np.asarray(cfg.data_mean), np.clip(np.asarray(cfg.data_std), 0.01, None)
    for name, frames in (("long", (0, 350, 699)), ("one", (0,)), ("still", (200,))):
        c = g["clip_" + name]
        T = int(c[0])
        pose = synth.make_pae_motion(T, int(c[1]), None if c[2] < 0 else (int(c[2]), int(c[3])))
        pn = (pose - mean) / std
        vel = (pn[1:] - pn[:-1]).astype(np.float32).astype(np.float64)
        for i in frames:
            ph, v, lat = _kernel_walk(P, vel, T, i)
            ref = g["phase_" + name][i].reshape(4, 8)
            assert np.all(np.abs(ph[1:] - ref[1:]) <= 1e-4 * np.abs(ref[1:]) + 1e-6), (name, i)
            assert np.abs((ph[0] - ref[0] + 0.5) % 1.0 - 0.5).max() < 1e-4, (name, i)
            assert np.abs(v - g["v_" + name][i]).max() < 1e-4
            sel = list(g["lat_frames_" + name])
            if i in sel:
                assert np.abs(lat - g["lat_" + name][sel.index(i)]).max() < 1e-5
