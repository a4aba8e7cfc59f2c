#!/usr/bin/env python
"""Golden vectors for the vq-wav2vec code extraction (qpgesture_amd/wavvq.py) from the torch restatement
tests/wavvq_model_ref.py run in f64 on the CPU.  No vq-wav2vec checkpoint ships with the reference, so weights and audio
are seeded (qpgesture_amd.synth.make_wavvq_state_dict / make_wav); the tests regenerate them from the seeds.

    python tests/golden/make_golden_wavvq_model.py          # writes tests/golden/wavvq_model.npz

Per case of wavvq_model_ref.CASES, with the case's name and an underscore in front of every key:
  codes        the f64 codes (B, T, G) int64
  margin       the f64 top-2 gap of the logits per (frame, group), (B, T, G)
  z, logits    the f64 features (B, T, C) and logits (B, T, G, V); for the full-size case only the frames FULL_ROWS
  e32_z, e32_logits   max |f32 restatement - f64 restatement| over the WHOLE tensor: the unit the device kernels' error is
               measured in
  codes32_diff the number of positions at which the f32 restatement's codes differ from the f64 ones
Asserted before anything is written: the smallest margin of every case is at least MIN_MARGIN_E32 = 64 times the case's
e32_logits (so for any tolerance factor up to 32 no position has to be left out of the exact code comparison) and the f32
restatement gives the f64 codes everywhere.  If a seed fails, change the seed."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import wavvq_model_ref as R  # noqa: E402

MIN_MARGIN_E32 = 64.0


def main():
    import torch
    out = dict(seed_tiny=np.int64(R.SEED_TINY), seed_full=np.int64(R.SEED_FULL))
    for name in R.CASES:
        geom, sd, wav = R.case_inputs(name)
        m64, m32 = R.WavVQRef(geom, sd, torch.float64), R.WavVQRef(geom, sd, torch.float32)
        z64, l64 = m64.features(wav), m64.logits(wav)
        z32, l32 = m32.features(wav), m32.logits(wav)
        codes, codes32 = l64.max(-1)[1].numpy(), l32.max(-1)[1].numpy()
        margin = R.top2_margin(l64)
        e32_z = float((z32.double() - z64).abs().max())
        e32_l = float((l32.double() - l64).abs().max())
        diff = int((codes != codes32).sum())
        print("%-7s B %d T %d: e32 z %.2e logits %.2e; min margin %.2e = %.0f x e32_logits; %d distinct codes; f32 codes "
              "differ at %d" % (name, codes.shape[0], codes.shape[1], e32_z, e32_l, margin.min(), margin.min() / e32_l,
                                len(np.unique(codes)), diff))
        assert margin.min() >= MIN_MARGIN_E32 * e32_l and diff == 0, name
        rows = R.FULL_ROWS if name == "full" else np.arange(codes.shape[1])
        out.update({name + "_codes": codes.astype(np.int64), name + "_margin": margin,
                    name + "_z": z64.numpy()[:, rows], name + "_logits": l64.numpy()[:, rows],
                    name + "_e32_z": np.float64(e32_z), name + "_e32_logits": np.float64(e32_l),
                    name + "_codes32_diff": np.int64(diff)})
    path = os.path.join(HERE, "wavvq_model.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
