#!/usr/bin/env python
"""Golden vectors for the phase extraction (PAE inference) from the REFERENCE model (imported from /root/reference;
build container only).  No PAE checkpoint ships with the reference, so the weights are seeded
(qpgesture_amd.synth.make_pae_state_dict) and loaded into the reference's own PAE.Model through load_state_dict; the
motion is seeded and smooth (synth.make_pae_motion), normalised with codebook.yml's mean / std, and run through the
reference's own pose2phase (PAE.py:477-508).  Committed are only OUTPUTS, per clip: `phase` (T,4,1,8,1) [p,f,a,b],
the pre-atan2' pair `v` (T,8,2) = (x, y) and the latent (8,240) of a few sampled frames."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from qpgesture_amd import synth  # noqa: E402

REF = "/root/reference/codebook"
SEED = 11
# (name, frames, motion seed, motionless stretch)
CLIPS = (("long", 700, 21, None), ("short", 150, 22, None), ("one", 1, 23, None), ("still", 400, 24, (120, 260)))
LATENT_FRAMES = 4


def reference_module():
    for name in ("lmdb", "configargparse"):
        sys.modules[name] = types.ModuleType(name)
    ed = types.ModuleType("easydict")

    class EasyDict(dict):
        __getattr__ = dict.__getitem__
    ed.EasyDict = EasyDict
    sys.modules["easydict"] = ed
    dl = types.ModuleType("data_loader")
    dl.__path__ = []
    ld = types.ModuleType("data_loader.lmdb_data_loader")
    ld.TrinityDataset = object
    sys.modules["data_loader"], sys.modules["data_loader.lmdb_data_loader"] = dl, ld
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF)
    import PAE
    PAE.mydevice = torch.device("cpu")
    return PAE


def main():
    import yaml
    PAE = reference_module()
    net = PAE.Model(input_channels=135, embedding_channels=8, time_range=240, key_range=13, window=4.0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_pae_state_dict(SEED).items()})
    net = net.eval()
    cfg = yaml.safe_load(open(os.path.join(REF, "configs", "codebook.yml")))
    data_mean = np.array(cfg["data_mean"]).squeeze()
    std = np.clip(np.array(cfg["data_std"]).squeeze(), a_min=0.01, a_max=None)

    rec = {"v": [], "lat": []}
    atan2 = net.atan2

    def atan2_rec(y, x):
        rec["v"].append(torch.stack([x, y], -1).detach().clone())
        return atan2(y, x)
    net.atan2 = atan2_rec
    fwd = net.forward

    def fwd_rec(x):
        out = fwd(x)
        rec["lat"].append(out[1][0].detach().clone())
        return out
    net.forward = fwd_rec

    out = {"meta": np.array([SEED, LATENT_FRAMES], np.int64)}
    with torch.no_grad():
        for name, T, mseed, still in CLIPS:
            rec["v"].clear()
            rec["lat"].clear()
            pose = synth.make_pae_motion(T, mseed, still)
            phase = PAE.pose2phase(net, pose, data_mean, std)
            v = torch.stack(rec["v"]).reshape(T, 8, 1, 2)[:, :, 0].numpy()          # one (1,2) per channel and frame
            sel = np.unique(np.linspace(0, T - 1, LATENT_FRAMES).round().astype(np.int64))
            out["phase_" + name] = phase.astype(np.float32)
            out["v_" + name] = v.astype(np.float32)
            out["lat_frames_" + name] = sel
            out["lat_" + name] = np.stack([rec["lat"][i].numpy() for i in sel]).astype(np.float32)
            out["clip_" + name] = np.array([T, mseed, -1 if still is None else still[0], -1 if still is None else still[1]],
                                           np.int64)
            ph = phase.reshape(T, 4, 8)
            print(name, phase.shape, phase.dtype, "p", np.nanmin(ph[:, 0]), np.nanmax(ph[:, 0]),
                  "f", ph[:, 1].min(), ph[:, 1].max(), "a", ph[:, 2].min(), ph[:, 2].max(),
                  "|v| min", np.abs(v).max(-1).min(), "latent absmax", np.abs(out["lat_" + name]).max(),
                  "nan", int(np.isnan(ph).sum()))
    np.savez_compressed(os.path.join(HERE, "pae_s%d.npz" % SEED), **out)


if __name__ == "__main__":
    main()
