"""Phase extraction on the device (qpg_pae_phase_f32 through qpgesture_amd/PAE.py) against what the REFERENCE's own
pose2phase computed (tests/golden/pae_s11.npz, captured by tests/golden/make_golden_pae.py).
Bars: f, a, b within 1e-4 relative or 1e-6 absolute; the circular phase distance within 1e-4 wherever |v| >= 1e-2;
NaN / inf exactly where the reference has them.  Grouping frames differently (batch order, chunks) is bit-identical."""
import os

import numpy as np
import pytest
import torch

from qpgesture_amd import PAE, synth
from qpgesture_amd.checkpoint import load_config
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

NAMES = ("long", "short", "one", "still")


@pytest.fixture(scope="module")
def setup():
    g = load_golden("pae_s11")
    net = PAE.Model(synth.make_pae_state_dict(int(g["meta"][0])), device="cuda:0")
    cfg = load_config(os.path.join(os.path.dirname(PAE.__file__), "configs", "codebook.yml"))
    mean, std = np.asarray(cfg.data_mean), np.clip(np.asarray(cfg.data_std), 0.01, None)
    poses = {}
    for n in NAMES:
        c = g["clip_" + n]
        poses[n] = synth.make_pae_motion(int(c[0]), int(c[1]), None if c[2] < 0 else (int(c[2]), int(c[3])))
    return g, net, mean, std, poses


def check_phase(got, ref, v_ref):
    """got / ref (T, 4, 1, 8, 1) [p, f, a, b]; v_ref (T, 8, 2) the reference's pre-atan2' pair."""
    got, ref = got.reshape(-1, 4, 8).astype(np.float64), ref.reshape(-1, 4, 8).astype(np.float64)
    bad_ref, bad_got = ~np.isfinite(ref), ~np.isfinite(got)
    assert np.array_equal(bad_ref, bad_got), "non-finite values differ: %d ref, %d got" % (bad_ref.sum(), bad_got.sum())
    ok = ~bad_ref
    fab, rfab = got[:, 1:], ref[:, 1:]
    m = ok[:, 1:]
    err = np.abs(fab - rfab)[m]
    assert np.all(err <= np.maximum(1e-4 * np.abs(rfab[m]), 1e-6)), "f/a/b: max err %g" % err.max()
    big = (np.abs(v_ref).max(-1) >= 1e-2) & ok[:, 0]
    dp = np.abs((got[:, 0] - ref[:, 0] + 0.5) % 1.0 - 0.5)[big]
    assert big.sum() > 0.9 * big.size and np.all(dp <= 1e-4), "p: max circular err %g" % dp.max()


def test_phase_vs_reference_golden(setup):
    g, net, mean, std, poses = setup
    for n in NAMES:
        got, v, lat = (x[0] for x in PAE.pose2phase_clips(net, [poses[n]], mean, std, return_v=True, return_latent=True))
        T = poses[n].shape[0]
        assert got.shape == (T, 4, 1, 8, 1) and got.dtype == np.float32
        check_phase(got, g["phase_" + n], g["v_" + n])
        assert np.abs(v - g["v_" + n]).max() < 1e-4
        # (a 32 400-term f32 chain per conv1 output: ~1e-5 from the reference's own order, bounded well below tanh's range)
        assert np.abs(lat[g["lat_frames_" + n]] - g["lat_" + n]).max() < 5e-5
    one = PAE.pose2phase(net, poses["short"], mean, std)            # the reference's signature
    check_phase(one, g["phase_short"], g["v_short"])


def test_batch_order_and_grouping_are_bit_identical(setup):
    g, net, mean, std, poses = setup
    alone = {n: PAE.pose2phase_clips(net, [poses[n]], mean, std)[0] for n in NAMES}
    fwd = PAE.pose2phase_clips(net, [poses[n] for n in NAMES], mean, std)
    rev = PAE.pose2phase_clips(net, [poses[n] for n in reversed(NAMES)], mean, std)
    small = PAE.pose2phase_clips(net, [poses[n] for n in NAMES], mean, std, chunk=97)
    for k, n in enumerate(NAMES):
        for other in (fwd[k], rev[len(NAMES) - 1 - k], small[k]):
            assert np.array_equal(alone[n].view(np.uint32), other.view(np.uint32)), n


def test_long_clip_chunked_matches_unchunked(setup):
    g, net, mean, std, poses = setup
    pose = synth.make_pae_motion(5000, 77)
    whole = PAE.pose2phase_clips(net, [pose], mean, std, chunk=5000)[0]
    parts = PAE.pose2phase_clips(net, [pose], mean, std, chunk=1777)[0]      # 3 workspace chunks
    assert np.isfinite(whole).all()
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))


def test_entry_point_refuses_bad_arguments(setup):
    from qpgesture_amd import _lib
    g, net, mean, std, poses = setup
    dev = net.device
    pose = torch.zeros((10, 135), dtype=torch.float64, device=dev)
    off = torch.tensor([0, 10], dtype=torch.int64, device=dev)
    m = torch.zeros(135, dtype=torch.float64, device=dev)
    out = torch.empty((10, 4, 8), device=dev)
    ws = torch.empty((10 + 239) * 136, device=dev)
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("qpg_pae_phase_f32", dev, net.params, pose, m, m, off, 1, 10, 0, 10, ws, ws.numel() - 1, out, None, None)
    with pytest.raises(RuntimeError, match="outside"):
        _lib.call("qpg_pae_phase_f32", dev, net.params, pose, m, m, off, 1, 10, 5, 10, ws, ws.numel(), out, None, None)
    _lib.call("qpg_pae_phase_f32", dev, net.params, pose, m, m, off, 1, 10, 0, 0, ws, ws.numel(), out, None, None)


def test_cli_writes_reference_phase_files(setup, tmp_path):
    from qpgesture_amd.data_processing import densify_phase
    g, net, mean, std, poses = setup
    rot, ph = tmp_path / "Rotation", tmp_path / "Phase"
    rot.mkdir()
    np.savez_compressed(str(rot / "a_long.npz"), upper=poses["long"])
    np.savez_compressed(str(rot / "b_still.npz"), upper=poses["still"])
    ck = str(tmp_path / "PAE_checkpoint_070.bin")
    torch.save({"args": {}, "epoch": 70, "model_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in
                                                        synth.make_pae_state_dict(int(g["meta"][0])).items()}}, ck)
    cfg = os.path.join(os.path.dirname(PAE.__file__), "configs", "codebook.yml")
    args = ["--config", cfg, "--gpu", "0", "--stage", "inference", "--PAE_model_path", ck, "--rotation_dir", str(rot),
            "--phase_dir", str(ph)]
    written = PAE.main(args)
    assert sorted(os.path.basename(w) for w in written) == ["a_long.npz", "b_still.npz"]
    for f, n in (("a_long.npz", "long"), ("b_still.npz", "still")):
        z = np.load(str(ph / f))
        assert list(z.keys()) == ["phase"]
        assert z["phase"].dtype == np.float32 and z["phase"].shape == (poses[n].shape[0], 4, 1, 8, 1)
        # make_beat_dataset cuts the column into 240-frame slices; the loader densifies them
        n_sl = poses[n].shape[0] // 240
        got = densify_phase(z["phase"][:n_sl * 240].reshape(n_sl, 240, 4, 1, 8, 1))
        ref = g["phase_" + n][:n_sl * 240].reshape(n_sl, 240, 4, 1, 8, 1)
        assert got.shape == (n_sl, 240, 4, 8)
        check_phase(got.reshape(-1, 4, 1, 8, 1), ref.reshape(-1, 4, 1, 8, 1), g["v_" + n][:n_sl * 240])
    before = os.path.getmtime(str(ph / "a_long.npz"))
    os.remove(str(ph / "b_still.npz"))
    written = PAE.main(args)                                               # the existing file is skipped
    assert [os.path.basename(w) for w in written] == ["b_still.npz"]
    assert os.path.getmtime(str(ph / "a_long.npz")) == before
