"""WavLM feature extraction (qpgesture_amd/wavlm.py) throughput on one GPU at WavLM-Large size: prints one JSON line.

Seeded weights (synth.make_wavlm_state_dict of the Large cfg) and seeded 4 s windows (synth.make_wav), --batch windows
per call as wav_to_wavlm runs them, inputs resident.  The three stages - front end (conv stack, layer_norm,
post_extract_proj), pos_conv, the transformer blocks with the final norm - are timed between device events that
are recorded at the stage boundaries of WavLM._forward; median of --reps runs after warm-up.  FLOPs are the model's
direct-form count (2 per multiply-add of every convolution, Linear and attention product, nothing for norms and
activations); the fraction is against the 157.3 TF f32 matrix peak.

    python tools/bench_wavlm.py [--batch 32] [--reps 5] [--layers 24]

--seconds S [--batch B]: one whole clip of S seconds per batch member (default B = 1) through a long_inputs model - the
tiled attention kernel past 256 frames.  A device event per stage of WavLM._forward; recorded per run: the three stage
times, the attention launches' time summed over the blocks with its TFLOP/s counted as 4 T^2 D per layer and batch
member, attention's share of the blocks' time, and torch.cuda.max_memory_allocated.  The record is appended to
profiles/wavlm_long_bench.json and profiles/wavlm_long_bench.md is rewritten from that file.

--attention-ab: qpg_wavlm_attention_tiled_f32 against qpg_wavlm_attention_f32 by direct entry-point calls on identical
inputs (B = 32, T = 256, H = 16), alternating, --reps rounds of 20 launches each; appended to the same record file.

    python tools/bench_wavlm.py --seconds 600 [--batch 1] [--reps 3]
    python tools/bench_wavlm.py --attention-ab [--reps 7]"""
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


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_JSON = os.path.join(ROOT, "profiles", "wavlm_long_bench.json")
LONG_MD = os.path.join(ROOT, "profiles", "wavlm_long_bench.md")
CROSSOVER_FRAMES = 6150          # 2 (4 D^2 + 2 D F) = 4 T D at Large: attention costs what the linear layers cost


def append_long_record(rec):
    """Append to profiles/wavlm_long_bench.json (a JSON list) and rewrite the .md table from the whole list."""
    try:
        with open(LONG_JSON) as f:
            recs = json.load(f)
    except (OSError, ValueError):
        recs = []
    recs.append(rec)
    with open(LONG_JSON, "w") as f:
        json.dump(recs, f, indent=1)
    lines = ["# Whole-recording WavLM (tools/bench_wavlm.py --seconds / --attention-ab)", "",
             "Device events per stage of `WavLM._forward`, medians over the runs of one call.  Attention FLOP are",
             "`4 T^2 D` per layer and batch member; the share of peak is against the %.1f TF f32 matrix peak; the model's"
             % PEAK_F32_TF,
             "crossover (attention = linear layers) is at %d frames (2 min)." % CROSSOVER_FRAMES, "",
             "| seconds | B | T | layers | front end s | pos_conv s | blocks s | attention s | attention TF/s | of peak | "
             "attention / blocks | T / crossover | peak memory GB |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        if r.get("mode") == "seconds":
            lines.append("| %g | %d | %d | %d | %.4f | %.4f | %.4f | %.4f | %.1f | %.3f | %.3f | %.2f | %.2f |" % (
                r["seconds"], r["batch"], r["frames"], r["layers"], r["front_end"]["time_s_median"],
                r["pos_conv"]["time_s_median"], r["blocks"]["time_s_median"], r["attention"]["time_s_median"],
                r["attention"]["tflops"], r["attention"]["fraction_of_f32_matrix_peak"], r["attention_share_of_blocks"],
                r["frames"] / CROSSOVER_FRAMES, r["max_memory_allocated_bytes"] / 1e9))
    ab = [r for r in recs if r.get("mode") == "attention_ab"]
    if ab:
        lines += ["", "## Tiled kernel against qpg_wavlm_attention_f32 (B = 32, T = 256, H = 16, alternating)", "",
                  "| rounds x launches | old kernel ms (median, min - max) | tiled kernel ms (median, min - max) | tiled / old | "
                  "max abs difference of the outputs |", "|---|---|---|---|---|"]
        for r in ab:
            lines.append("| %d x %d | %.4f (%.4f - %.4f) | %.4f (%.4f - %.4f) | %.3f | %.2e |" % (
                r["rounds"], r["launches"], r["old_ms"]["median"], r["old_ms"]["min"], r["old_ms"]["max"],
                r["tiled_ms"]["median"], r["tiled_ms"]["min"], r["tiled_ms"]["max"],
                r["tiled_ms"]["median"] / r["old_ms"]["median"], r["max_abs_difference"]))
    with open(LONG_MD, "w") as f:
        f.write("\n".join(lines) + "\n")


def run_seconds(args, dev):
    B = args.batch or 1
    n = int(round(args.seconds * W.SAMPLE_RATE))
    cfg = dict(synth.WAVLM_LARGE, encoder_layers=args.layers)
    model = W.WavLM(cfg, device=dev, long_inputs=True).load_state_dict(synth.make_wavlm_state_dict(1, cfg))
    wav = torch.from_numpy(synth.make_wav(2, B, n)).to(dev)
    T = W.frames_of(n, model.conv_layers)[-1]
    D = cfg["encoder_embed_dim"]
    torch.cuda.reset_peak_memory_stats()
    out = model.extract_features(wav)[0]                 # warm-up: code objects, the workspace, the bias table
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and out.shape == (B, T, D)
    peak = int(torch.cuda.max_memory_allocated())
    times = {"front_end": [], "pos_conv": [], "blocks": [], "attention": [], "total": []}
    for _ in range(args.reps):
        ev = []

        def on_stage(stage, _view):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((stage, e))
        model._forward(wav, on_stage)
        torch.cuda.synchronize()
        at = dict(ev)
        for a, b in (("start", "front_end"), ("front_end", "pos_conv"), ("pos_conv", "blocks")):
            times[b].append(at[a].elapsed_time(at[b]) * 1e-3)
        times["total"].append(at["start"].elapsed_time(at["blocks"]) * 1e-3)
        times["attention"].append(sum(ev[i - 1][1].elapsed_time(e) for i, (s, e) in enumerate(ev) if s.endswith(".att"))
                                  * 1e-3)
    fl = stage_flops(cfg, n)
    fl["attention"] = 4.0 * T * T * D * args.layers
    fl["total"] = fl["front_end"] + fl["pos_conv"] + fl["blocks"]
    rec = {"tool": "bench_wavlm", "mode": "seconds", "seconds": args.seconds, "batch": B, "frames": T, "layers": args.layers,
           "reps": args.reps, "device": torch.cuda.get_device_name(0), "max_memory_allocated_bytes": peak,
           "crossover_frames": CROSSOVER_FRAMES}
    for k, ts in times.items():
        t = float(np.median(ts))
        tf = B * fl[k] / t / 1e12
        rec[k] = {"time_s_median": t, "time_s_min": float(min(ts)), "time_s_max": float(max(ts)), "tflops": tf,
                  "fraction_of_f32_matrix_peak": tf / PEAK_F32_TF}
    rec["attention_share_of_blocks"] = rec["attention"]["time_s_median"] / rec["blocks"]["time_s_median"]
    append_long_record(rec)
    print(json.dumps(rec))


def run_attention_ab(args, dev):
    from qpgesture_amd import _lib
    B, T, H, launches = 32, 256, 16, 20
    D = H * W.HEAD_DIM
    g = torch.Generator(device="cpu").manual_seed(3)
    qkv = torch.randn((B * T, 3 * D), generator=g)
    qkv[:, :D] *= 0.35
    qkv = qkv.to(dev)
    gate = (torch.rand((B * T, H), generator=g) * 1.7 + 0.7).to(dev)
    relb = torch.randn((2 * T - 1, H), generator=g).to(dev)
    outs = {"old": torch.empty((B * T, D), device=dev), "tiled": torch.empty((B * T, D), device=dev)}

    def launch(which):
        if which == "old":
            _lib.call("qpg_wavlm_attention_f32", dev, qkv, gate, relb, B, T, H, outs["old"])
        else:
            _lib.call("qpg_wavlm_attention_tiled_f32", dev, qkv, gate, relb, None, B, T, H, outs["tiled"])
    for which in ("old", "tiled", "old", "tiled"):
        for _ in range(5):
            launch(which)
    torch.cuda.synchronize()
    ms = {"old": [], "tiled": []}
    for _ in range(args.reps):
        for which in ("old", "tiled"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                launch(which)
            b.record()
            torch.cuda.synchronize()
            ms[which].append(a.elapsed_time(b) / launches)
    flop = 4.0 * T * T * D * B
    rec = {"tool": "bench_wavlm", "mode": "attention_ab", "B": B, "T": T, "H": H, "rounds": args.reps, "launches": launches,
           "device": torch.cuda.get_device_name(0),
           "max_abs_difference": float((outs["old"] - outs["tiled"]).abs().max())}
    for which in ("old", "tiled"):
        med = float(np.median(ms[which]))
        rec[which + "_ms"] = {"median": med, "min": float(min(ms[which])), "max": float(max(ms[which])),
                              "tflops": flop / (med * 1e-3) / 1e12}
    append_long_record(rec)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None, help="windows per call (default 32); with --seconds clips (default 1)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--seconds", type=float, default=None, help="whole clips of this length through a long_inputs model")
    ap.add_argument("--attention-ab", action="store_true", help="the tiled attention kernel against the 256-frame one")
    args = ap.parse_args()
    dev = "cuda:0"
    if not torch.cuda.is_available():
        raise SystemExit("bench_wavlm: no GPU")
    if args.attention_ab:
        return run_attention_ab(args, dev)
    if args.seconds is not None:
        return run_seconds(args, dev)
    args.batch = args.batch or 32
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
