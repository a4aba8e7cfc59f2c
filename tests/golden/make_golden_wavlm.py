#!/usr/bin/env python
"""Golden vectors for the WavLM feature extraction from the REFERENCE model (imported from /root/reference; build
container only).  No WavLM checkpoint ships with the reference, so weights and audio are seeded
(qpgesture_amd.synth.make_wavlm_state_dict / make_wav) and loaded into the reference's own WavLM through
load_state_dict; the model runs in f64 (model.double(), its f32-forcing norms evaluated in f64 too) and in f32.  Committed are only OUTPUTS, per fixture:
  out       f64 result of extract_features(wav)[0] (subsampled rows / columns in `wide`: rows, cols),
  e32       max |y_f32 - y_f64| over the FULL result: the reference's own f32 error,
  features / pos_conv / block0 (+ e32_<tap>)   three intermediate results in f64, on tap_rows (and cols),
  weff      (tiny_1s) every 8th output channel of the model's effective pos_conv weight, f64,
  buckets   (tiny) _relative_positions_bucket of every offset in [-255, 255].
f64 is stored as f64: tests/wavlm_ref.py is pinned against these files to 1e-9."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from qpgesture_amd import synth  # noqa: E402

REF = "/root/reference/process/WavLM"
# name, cfg, weight seed, wav seed, B, n, row step of the output, column step, row step of the taps
FIXTURES = (("tiny", synth.WAVLM_TINY, 31, 41, 2, 64000, 1, 1, 4),
            ("tiny_1s", synth.WAVLM_TINY, 31, 42, 3, 16000, 1, 1, 1),
            ("wide", synth.WAVLM_WIDE, 32, 43, 1, 64000, 4, 4, 4))


def run(model, wav):
    taps = {}
    hooks = [
        model.feature_extractor.register_forward_hook(
            lambda m, i, o: taps.__setitem__("features", o.transpose(1, 2).detach().clone())),
        model.encoder.layers[0].register_forward_pre_hook(
            lambda m, a: taps.__setitem__("pos_conv", a[0].transpose(0, 1).detach().clone())),
        model.encoder.layers[0].register_forward_hook(
            lambda m, i, o: taps.__setitem__("block0", o[0].transpose(0, 1).detach().clone())),
    ]
    with torch.no_grad():
        taps["out"] = model.extract_features(wav)[0].detach().clone()
    for h in hooks:
        h.remove()
    return {k: v.numpy() for k, v in taps.items()}


def main():
    sys.path.insert(0, REF)
    from WavLM import WavLM, WavLMConfig
    for name, cfg, wseed, aseed, B, n, rstep, cstep, tstep in FIXTURES:
        sd = synth.make_wavlm_state_dict(wseed, cfg)
        wav = synth.make_wav(aseed, B, n)
        model = WavLM(WavLMConfig(dict(cfg))).eval()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        y32 = run(model, torch.from_numpy(wav))
        model = model.double()
        # two pieces of the model cast to f32 whatever its dtype: the conv stack's norms (Fp32LayerNorm) and the
        # blocks' activation (gelu(x.float())).  For the f64 run both evaluate the same function in f64 instead.
        for m in model.modules():
            if type(m).__name__ == "Fp32LayerNorm":
                m.forward = torch.nn.LayerNorm.forward.__get__(m)
            if type(m).__name__ == "TransformerSentenceEncoderLayer":
                m.activation_fn = torch.nn.functional.gelu
        y64 = run(model, torch.from_numpy(wav).double())
        out = {"meta": np.array([wseed, aseed, B, n, rstep, cstep, tstep], np.int64),
               "rows": np.arange(0, y64["out"].shape[1], rstep), "cols": np.arange(0, y64["out"].shape[2], cstep),
               "tap_rows": np.arange(0, y64["out"].shape[1], tstep)}
        out["out"] = y64["out"][:, ::rstep, ::cstep]
        out["e32"] = np.array(np.abs(y32["out"].astype(np.float64) - y64["out"]).max())
        for tap in ("features", "pos_conv", "block0"):
            out[tap] = y64[tap][:, ::tstep, ::cstep]
            out["e32_" + tap] = np.array(np.abs(y32[tap].astype(np.float64) - y64[tap]).max())
        if name == "tiny_1s":
            out["weff"] = model.encoder.pos_conv[0].weight.detach().numpy()[::8]
        if name == "tiny":
            off = torch.arange(-255, 256, dtype=torch.long)
            out["buckets"] = model.encoder.layers[0].self_attn._relative_positions_bucket(off).numpy().astype(np.int64)
        path = os.path.join(HERE, "wavlm_%s.npz" % name)
        np.savez_compressed(path, **out)
        print(name, y64["out"].shape, "rms", float(np.sqrt((y64["out"] ** 2).mean())), "e32", float(out["e32"]),
              {t: float(out["e32_" + t]) for t in ("features", "pos_conv", "block0")}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
