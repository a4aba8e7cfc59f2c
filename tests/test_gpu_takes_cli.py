"""GPU tests of the command lines' several-takes flags on a fixture set: GestureKNN --n_takes, VisualizeCodebook --takes,
the inference wrapper passing both through."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's decode tolerance (tests/test_gpu_vqvae.py)


def _knn_argv(paths, out, *extra):
    argv = []
    for k, v in paths.items():
        argv += ["--" + k, v]
    return argv + ["--out_knn_filename", out, "--db_cache", "off"] + list(extra)


def _same_archive(a, b):
    """Two .npz files hold the same bytes: the same members in the same order, each with the same compressed bytes, sizes
    and checksum.  (The whole files also carry each member's modification time, the second the writer ran.)"""
    import zipfile
    za, zb = zipfile.ZipFile(a), zipfile.ZipFile(b)
    ia, ib = za.infolist(), zb.infolist()
    assert [i.filename for i in ia] == [i.filename for i in ib]
    for x, y in zip(ia, ib):
        assert (x.CRC, x.file_size, x.compress_size, x.compress_type) == (y.CRC, y.file_size, y.compress_size, y.compress_type)
        assert za.read(x.filename) == zb.read(y.filename)
    ra, rb = open(a, "rb").read(), open(b, "rb").read()
    assert len(ra) == len(rb)
    if [i.date_time for i in ia] == [i.date_time for i in ib]:
        assert ra == rb


def _checkpoint(tmp_path, rotations=False):
    """The seeded synthetic VQ-VAE checkpoint.  rotations: the output convolution scaled down and its bias dropped, so that
    the de-normalised poses stay close to the configuration's mean pose - proper rotation matrices, which the Euler step
    accepts (the plain seeded weights decode to matrices with non-positive determinants, tests/test_gpu_vqvae.py)."""
    import torch
    from qpgesture_amd import synth
    sd = dict(synth.make_vqvae_state_dict(7))
    if rotations:
        sd["module.decoders.0.out.weight"] = sd["module.decoders.0.out.weight"] * np.float32(0.02)
        sd["module.decoders.0.out.bias"] = sd["module.decoders.0.out.bias"] * np.float32(0.0)
    ck = str(tmp_path / ("codebook_checkpoint_%d.bin" % int(rotations)))
    torch.save({"args": {"name": "codebook"}, "epoch": 3, "model_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    return sd, ck


def test_gesture_knn_n_takes(tmp_path, capsys):
    """--n_takes 1: the file is the one written without the flag, byte for byte.  --n_takes 4: knn_pred unchanged, take 0 is
    knn_pred, every take is match_clip from that take's seed (the seeds: four successive draws from np.random seeded like
    the command line), the coalescence report is there and printed."""
    import torch
    from qpgesture_amd import GestureKNN as cli
    from qpgesture_amd import synth, takes
    from qpgesture_amd.code_knn import CodeKNN, GestureDB
    from qpgesture_amd.data_processing import load_db_codebook
    paths = synth.write_npz_set(str(tmp_path / "npz"), 48, 2)
    plain, one, four = (str(tmp_path / n) for n in ("plain.npz", "one.npz", "four.npz"))
    want = cli.main(_knn_argv(paths, plain))
    cli.main(_knn_argv(paths, one, "--n_takes", "1"))
    _same_archive(plain, one)
    capsys.readouterr()
    cli.main(_knn_argv(paths, four, "--n_takes", "4"))
    printed = capsys.readouterr().out
    z = np.load(four)
    assert sorted(z.files) == ["knn_pred", "knn_pred_takes", "take_first_shared_code", "take_seed_codes"]
    assert z["knn_pred"].dtype == np.int64 and np.array_equal(z["knn_pred"], want)
    assert np.array_equal(z["knn_pred"], np.load(plain)["knn_pred"])
    tk = z["knn_pred_takes"]
    assert tk.dtype == np.int64 and tk.shape == (4,) + want.shape and np.array_equal(tk[0], want)
    assert z["take_seed_codes"].shape == (4,) and z["take_first_shared_code"].shape == (4,)
    assert np.array_equal(z["take_first_shared_code"], takes.first_shared_code(tk))
    assert "n_distinct %d" % takes.n_distinct(tk) in printed
    # the takes, one match_clip each, from the command line's own stream of draws
    L = load_db_codebook(paths["train_database"], paths["train_codebook"], paths["test_data"], paths["train_wavlm"],
                         paths["test_wavlm"], paths["train_wavvq"], paths["test_wavvq"], device="cuda:0")
    code = np.asarray(L.code)
    cnt = np.bincount(code.reshape(-1), minlength=512)[:512]
    freq_rank = np.array(list(np.where(cnt > 0, 1 - cnt / cnt.sum(), 1.0))).argsort().argsort()
    db = GestureDB(L.code, L.train_wavlm, L.train_context, L.train_phase, np.load(paths["codebook_signature"])["signature"],
                   device="cuda:0", freq_rank=freq_rank)
    knn = CodeKNN(db, rng=np.random.RandomState(cli.seed_value))
    M = want.shape[0]
    te_i, te_c = L.test_wavlm[:M].contiguous(), torch.from_numpy(L.test_context[:M]).to("cuda:0")
    for s in range(4):
        sc, sp = knn.init_code_phase()
        assert sc == z["take_seed_codes"][s]
        assert np.array_equal(knn.match_clip(te_i, te_c, M, seed_code=sc, seed_phase=sp)[0], tk[s]), s


def test_visualize_codebook_takes_and_the_inference_wrapper(tmp_path):
    """--takes all / an index: every take decoded in one batch is, within the decode tolerance, the oracle's decode of that
    take's codes; the files carry the take's index; the default (no --takes) is untouched.  The wrapper passes --n_takes
    and --takes through."""
    import torch
    from oracle import vqvae_oracle as VO
    from qpgesture_amd import VisualizeCodebook as vis
    from qpgesture_amd import inference, synth
    from qpgesture_amd.checkpoint import denormalize_poses, load_config
    sd, ck = _checkpoint(tmp_path)
    cfg_path = os.path.join(os.path.dirname(os.path.abspath(vis.__file__)), "configs", "codebook.yml")
    cfg = load_config(cfg_path)
    paths = synth.write_npz_set(str(tmp_path / "npz"), 48, 2)
    db = {k: paths[k] for k in ("train_database", "train_codebook", "codebook_signature", "train_wavlm", "test_wavlm",
                                "train_wavvq", "test_wavvq")}
    fold = str(tmp_path / "utt")
    pred, poses = inference.main(paths["test_data"], cfg_path, ck, output_fold=fold, no_bvh=True,
                                 knn_extra=["--db_cache", "off"], n_takes=4, takes="all", **db)
    z = np.load(os.path.join(fold, "knn_pred.npz"))
    tk = z["knn_pred_takes"]
    assert tk.shape == (4,) + pred.shape and np.array_equal(tk[0], pred) and np.array_equal(z["knn_pred"], pred)
    assert poses.shape == (4, 240 * pred.shape[0], 135)
    name = os.path.basename(paths["test_data"])[:-4]
    prefix = "result_" + name
    with torch.no_grad():
        want = VO.decode(sd, tk.reshape(4, -1)).numpy()
    for k in range(4):
        gen = np.load(os.path.join(fold, prefix, "generate%s_take%d.npy" % (prefix, k)))
        code = np.load(os.path.join(fold, prefix, "code%s_take%d.npy" % (prefix, k)))
        assert code.shape == (1, 30 * pred.shape[0]) and np.array_equal(code[0], tk[k].flatten())
        assert np.array_equal(gen, poses[k])
        assert np.abs(gen - denormalize_poses(want[k], cfg.data_mean, cfg.data_std)).max() < TOL, k
    assert not os.path.exists(os.path.join(fold, prefix, "generate%s.npy" % prefix))       # --takes writes the takes only
    # one take by index; the default decodes knn_pred as before
    res = os.path.join(fold, "knn_pred.npz")
    common = ["--config", cfg_path, "--gpu", "0", "--code_path", res, "--VQVAE_model_path", ck, "--stage", "inference",
              "--save_path", str(tmp_path), "--no_bvh"]
    p2, c2 = vis.main(common + ["--prefix", "one", "--takes", "2"])
    assert p2.shape == (1, 240 * pred.shape[0], 135) and np.array_equal(c2[0], tk[2].flatten())
    assert sorted(os.listdir(str(tmp_path / "one"))) == ["codeone_take2.npy", "generateone_take2.npy"]
    assert np.abs(p2[0] - denormalize_poses(want[2], cfg.data_mean, cfg.data_std)).max() < TOL
    p0, c0 = vis.main(common + ["--prefix", "dflt"])
    assert sorted(os.listdir(str(tmp_path / "dflt"))) == ["codedflt.npy", "generatedflt.npy"]
    assert p0.shape == (240 * pred.shape[0], 135) and np.abs(p0 - poses[0]).max() < TOL
    with pytest.raises(IndexError):
        vis.main(common + ["--prefix", "bad", "--takes", "4"])
    plain = str(tmp_path / "plain.npz")
    np.savez_compressed(plain, knn_pred=pred)
    with pytest.raises(KeyError):
        vis.main(common[:4] + ["--code_path", plain] + common[6:] + ["--prefix", "bad", "--takes", "all"])


@pytest.mark.parametrize("smoothing", [False, True])
def test_euler_files_are_those_of_each_take_alone(tmp_path, smoothing):
    """<prefix>_take<k>_euler.npy == bvh.poses_to_euler of take k's poses ALONE (row k of the batched decode), bit for bit -
    with --smoothing too: the Savitzky-Golay window never reaches from one take into the next, which the table of the
    concatenated takes shows it would.  (Takes differ, so their tables differ.)"""
    import torch
    from qpgesture_amd import VisualizeCodebook as vis
    from qpgesture_amd import bvh
    from qpgesture_amd.checkpoint import load_config
    from qpgesture_amd.vqvae import VQVAE
    sd, ck = _checkpoint(tmp_path, rotations=True)
    cfg_path = os.path.join(os.path.dirname(os.path.abspath(vis.__file__)), "configs", "codebook.yml")
    cfg = load_config(cfg_path)
    tk = np.random.Generator(np.random.PCG64(12)).integers(0, 512, size=(3, 2, 30), dtype=np.int64)
    res = str(tmp_path / "takes.npz")
    np.savez_compressed(res, knn_pred=tk[0], knn_pred_takes=tk)
    vis.main(["--config", cfg_path, "--gpu", "0", "--code_path", res, "--VQVAE_model_path", ck, "--stage", "inference",
              "--save_path", str(tmp_path), "--prefix", "e", "--takes", "all"] + (["--smoothing"] if smoothing else []))
    model = VQVAE(cfg.VQVAE, 15 * 9, device="cuda:0")
    model.load_state_dict(sd)
    poses = model.decode([torch.from_numpy(tk.reshape(3, -1))])
    eulers = []
    for k in range(3):
        want = bvh.poses_to_euler(poses[k], cfg.data_mean, cfg.data_std, smoothing=smoothing)
        got = np.load(str(tmp_path / "e" / ("e_take%d_euler.npy" % k)))
        assert got.shape == (480, 45) and np.array_equal(got, want), k
        txt = open(str(tmp_path / "e" / ("e_take%d_generated.bvh" % k))).read()
        assert txt.startswith("HIERARCHY") and "Frames: 480" in txt
        eulers.append(got)
    assert not np.array_equal(eulers[0], eulers[1])
    joined = bvh.poses_to_euler(poses.reshape(-1, 135), cfg.data_mean, cfg.data_std, smoothing=smoothing)
    same = np.array_equal(joined, np.concatenate(eulers))
    assert same == (not smoothing)              # (smoothed across the seams the concatenation differs there)
