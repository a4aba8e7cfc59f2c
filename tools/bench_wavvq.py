"""vq-wav2vec code extraction (qpgesture_amd/wavvq.py) at the real geometry on one GPU: prints one JSON line.

Per batch size B (windows of 64 000 samples -> 398 x 2 codes): WavVQ.forward_idx from samples on the device to codes on the
device, wall clock around a synchronise, median of --reps calls after a warm-up, as windows/s; and the device time of every
stage - a device event behind each launch group, the median over the same calls of the time between consecutive events -
summed into the GroupNorm passes (norm0 .. norm7), the convolutions (conv0 .. conv7) and the head (two GEMMs, ReLU,
argmax), each with its share of the total.  `groupnorm_bytes_per_s` is what the GroupNorm passes moved - every activation
read twice and written once, 12 bytes per value - over their device time; `norm0` alone is given too (26 MB per window).
Beside it the same network from torch.nn.Conv1d / GroupNorm / Linear (tests/wavvq_model_ref.py) with the same seeded
weights on the same device in f32, timed the same way end to end, and the number of code slots on which the two differ.

    python tools/bench_wavvq.py [--batches 1,16,32] [--reps 7]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qpgesture_amd import _lib, synth, wavvq  # noqa: E402
from qpgesture_amd.wavlm import frames_of  # noqa: E402
from tests.wavvq_model_ref import WavVQRef  # noqa: E402

WINDOW = 64000


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,32")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wavvq: no GPU")
    dev = "cuda:0"
    geom = synth.WAVVQ_GUMBEL
    sd = synth.make_wavvq_state_dict(1, geom)
    model = wavvq.WavVQ(geom, device=dev).load_state_dict(sd)
    ref = WavVQRef(geom, sd, torch.float32, device=dev)
    fr = frames_of(WINDOW, model.conv_layers)
    rec = {"tool": "bench_wavvq", "samples_per_window": WINDOW, "frames": fr[-1], "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "batches": {}}
    base = synth.make_wav(2, 8, WINDOW)
    for B in (int(b) for b in args.batches.split(",")):
        x = torch.from_numpy(base).to(dev).repeat((B + 7) // 8, 1)[:B].contiguous()
        x = x * torch.linspace(0.5, 1.5, B, device=dev)[:, None]          # (no two windows alike)
        n0 = _lib.n_calls
        codes = model.forward_idx(x)                                      # warm-up: code objects, the kept buffers
        launches = _lib.n_calls - n0
        t_med, t_min, t_max = wall(lambda: model.forward_idx(x), args.reps)
        stages = {}
        for _ in range(args.reps):
            ev = []

            def on_stage(stage):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append((stage, e))
            model._chain(x, "codes", on_stage=on_stage)
            torch.cuda.synchronize()
            for (_, a), (stage, b) in zip(ev[:-1], ev[1:]):
                stages.setdefault(stage, []).append(a.elapsed_time(b) * 1e-3)
        dev_s = {k: float(np.median(v)) for k, v in stages.items()}
        total = sum(dev_s.values())
        groups = {"groupnorm": sum(v for k, v in dev_s.items() if k.startswith("norm")),
                  "convolutions": sum(v for k, v in dev_s.items() if k.startswith("conv")), "head": dev_s["head"]}
        gn_bytes = 12.0 * B * model.C * sum(fr)
        one = {"windows_per_s": B / t_med, "time_s_median": t_med, "time_s_min": t_min, "time_s_max": t_max,
               "launches_per_call": launches, "device_s": dict(dev_s, total=total),
               "device_s_groups": groups, "share": {k: v / total for k, v in groups.items()},
               "groupnorm_bytes_per_s": gn_bytes / groups["groupnorm"],
               "norm0_bytes_per_s": 12.0 * B * model.C * fr[0] / dev_s["norm0"]}
        with torch.no_grad():
            ref_codes = ref.forward_idx(x)                                # warm-up: MIOpen picks its algorithms
            r_med, r_min, r_max = wall(lambda: ref.forward_idx(x), args.reps)
        one["torch_nn"] = {"windows_per_s": B / r_med, "time_s_median": r_med, "time_s_min": r_min, "time_s_max": r_max,
                           "codes_that_differ": int((ref_codes != codes).sum()), "code_slots": int(codes.numel())}
        one["speedup_vs_torch_nn"] = r_med / t_med
        rec["batches"][str(B)] = one
        print("bench_wavvq: B %d: %.1f windows/s, torch.nn %.1f" % (B, B / t_med, B / r_med), file=sys.stderr, flush=True)
        del x, ref_codes
        torch.cuda.empty_cache()
    rec["windows_per_s"] = rec["batches"][str(max(int(b) for b in rec["batches"]))]["windows_per_s"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
