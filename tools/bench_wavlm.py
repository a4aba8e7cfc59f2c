"""WavLM feature extraction (qpgesture_amd/wavlm.py) throughput on one GPU at WavLM-Large size: prints one JSON line.

Seeded weights (synth.make_wavlm_state_dict of the Large cfg) and seeded 4 s windows (synth.make_wav), --batch windows
per call as wav_to_wavlm runs them, inputs resident.  The three stages - front end (conv stack, layer_norm,
post_extract_proj), pos_conv, the transformer blocks with the final norm - are timed between device events that
are recorded at the stage boundaries of WavLM._forward; median of --reps runs after warm-up.  FLOPs are the model's
direct-form count (2 per multiply-add of every convolution, Linear and attention product, nothing for norms and
activations); the fraction is against the 157.3 TF f32 matrix peak.

    python tools/bench_wavlm.py [--batch 32] [--reps 5] [--layers 24]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qpgesture_amd import synth  # noqa: E402
from qpgesture_amd import wavlm as W  # noqa: E402

PEAK_F32_TF = 157.3


def stage_flops(cfg, n):
    """Direct-form FLOP of one window per stage."""
    layers = W.conv_layers_of(cfg)
    fr = W.frames_of(n, layers)
    C, D, F = layers[0][0], cfg["encoder_embed_dim"], cfg["encoder_ffn_embed_dim"]
    T = fr[-1]
    front, cin = 0.0, 1
    for (c, k, _), t in zip(layers, fr):
        front += 2.0 * t * c * cin * k
        cin = c
    front += 2.0 * T * C * D if C != D else 0.0
    pos = 2.0 * T * D * (D // cfg["conv_pos_groups"]) * cfg["conv_pos"]
    block = 2.0 * T * D * D * 4 + 2.0 * T * D * F * 2 + 2.0 * 2 * T * T * D + 2.0 * T * D * 8
    return {"front_end": front, "pos_conv": pos, "blocks": block * cfg["encoder_layers"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = dict(synth.WAVLM_LARGE, encoder_layers=args.layers)
    model = W.WavLM(cfg, device=dev).load_state_dict(synth.make_wavlm_state_dict(1, cfg))
    wav = torch.from_numpy(synth.make_wav(2, args.batch, W.WINDOW)).to(dev)
    for _ in range(2):
        out = model.extract_features(wav)[0]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    times = {"front_end": [], "pos_conv": [], "blocks": [], "total": []}
    for _ in range(args.reps):
        ev = {}

        def on_stage(stage, _view):
            ev[stage] = torch.cuda.Event(enable_timing=True)
            ev[stage].record()
        model._forward(wav, on_stage)
        torch.cuda.synchronize()
        for a, b in (("start", "front_end"), ("front_end", "pos_conv"), ("pos_conv", "blocks")):
            times[b].append(ev[a].elapsed_time(ev[b]) * 1e-3)
        times["total"].append(ev["start"].elapsed_time(ev["blocks"]) * 1e-3)
    fl = stage_flops(cfg, W.WINDOW)
    fl["total"] = sum(fl.values())
    rec = {"tool": "bench_wavlm", "batch": args.batch, "layers": args.layers, "reps": args.reps,
           "gflop_per_window": {k: v / 1e9 for k, v in fl.items()}, "device": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        t = float(np.median(ts))
        tf = args.batch * fl[k] / t / 1e12
        rec[k] = {"time_s_median": t, "tflops": tf, "fraction_of_f32_matrix_peak": tf / PEAK_F32_TF}
    rec["windows_per_s"] = args.batch / rec["total"]["time_s_median"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
