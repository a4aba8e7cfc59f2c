"""The GRU speech-to-code generator (qpgesture_amd/generate.py) on one GPU: prints one JSON line.

Per batch size B (windows of 64 000 samples; 6 is one 24 s clip, 2048 a database): Generator_gru.sample from samples on
the device to codes on the device, wall clock around a synchronise, median of --reps calls after a warm-up, as windows/s;
and the device time of every stage - a device event behind each launch, the median over the same calls of the time
between consecutive events: conv1 .. conv5, the GRU input GEMMs (gru0.proj, gru1.proj), the recurrences (gru0, gru1) and
the head (ln + logits + codes).  Beside them the same model built HERE from torch.nn.Conv1d / BatchNorm1d / LeakyReLU /
GRU / LayerNorm / Linear with the same seeded weights on the same device, in eval mode under no_grad, timed the same way
end to end (its argmax included) and per part (encoder, GRU, head), and the number of code slots on which its codes differ
from the kernels'.  `launches_per_sample` counts the library's launches of one sample() call.

    python tools/bench_generator.py [--batches 1,6,256,2048] [--reps 7]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qpgesture_amd import _lib  # noqa: E402
from qpgesture_amd import generate as G  # noqa: E402
from qpgesture_amd import synth  # noqa: E402


class TorchGenerator(torch.nn.Module):
    """The same network from torch.nn modules (parameter names as in the seeded state dict)."""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        layers = []
        for i, (cin, cout, stride) in enumerate(G.CONVS):
            layers.append(nn.Conv1d(cin, cout, G.TAPS, stride=stride))
            if i < 4:
                layers += [nn.BatchNorm1d(cout), nn.LeakyReLU(G.SLOPE)]
        self.WavEncoder = nn.Module()
        self.WavEncoder.feat_extractor = nn.Sequential(*layers)
        self.project = nn.GRU(G.CONVS[-1][1], G.HIDDEN, num_layers=2, bidirectional=True, batch_first=True)
        self.norm = nn.LayerNorm(G.HIDDEN)
        self.out = nn.Linear(G.HIDDEN, G.CODES)

    def encoder(self, x):
        return self.WavEncoder.feat_extractor(x.unsqueeze(1)).transpose(1, 2)

    def head(self, y):
        return self.out(self.norm(y[:, :, :G.HIDDEN] + y[:, :, G.HIDDEN:])).argmax(-1)

    def forward(self, x):
        return self.head(self.project(self.encoder(x))[0])


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
    ap.add_argument("--batches", default="1,6,256,2048")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generator: no GPU")
    dev = "cuda:0"
    sd = synth.make_generator_state_dict(1)
    model = G.Generator_gru(device=dev).load_state_dict(sd)
    ref = TorchGenerator().eval()
    ref.load_state_dict({k[7:]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    ref = ref.to(dev)
    rec = {"tool": "bench_generator", "samples_per_window": G.WINDOW, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "batches": {}}
    base = synth.make_wav(2, 8, G.WINDOW)
    for B in (int(b) for b in args.batches.split(",")):
        x = torch.from_numpy(base).to(dev).repeat((B + 7) // 8, 1)[:B].contiguous()
        x = x * torch.linspace(0.5, 1.5, B, device=dev)[:, None]          # (no two windows alike)
        n0 = _lib.n_calls
        codes = model.sample(x)[0]                                        # warm-up: code objects, the kept buffers
        launches = _lib.n_calls - n0
        torch.cuda.synchronize()
        t_med, t_min, t_max = wall(lambda: model.sample(x), args.reps)
        stages = {}
        for _ in range(args.reps):
            ev = []

            def on_stage(stage, _view):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append((stage, e))
            model.codes(x, on_stage=on_stage)
            torch.cuda.synchronize()
            for (_, a), (stage, b) in zip(ev[:-1], ev[1:]):
                stages.setdefault(stage, []).append(a.elapsed_time(b) * 1e-3)
        dev_s = {k: float(np.median(v)) for k, v in stages.items()}
        dev_s["head"] = dev_s.pop("ln") + dev_s.pop("logits") + dev_s.pop("codes")
        one = {"windows_per_s": B / t_med, "time_s_median": t_med, "time_s_min": t_min, "time_s_max": t_max,
               "device_s": dict(dev_s, total=sum(dev_s.values())), "launches_per_sample": launches}
        with torch.no_grad():
            ref_codes = ref(x)                                            # warm-up: MIOpen picks its algorithms
            torch.cuda.synchronize()
            r_med, r_min, r_max = wall(lambda: ref(x), args.reps)
            enc = ref.encoder(x)
            y = ref.project(enc)[0]
            parts = {"encoder": wall(lambda: ref.encoder(x), args.reps)[0], "gru": wall(lambda: ref.project(enc), args.reps)[0],
                     "head": wall(lambda: ref.head(y), args.reps)[0]}
        one["torch_nn"] = {"windows_per_s": B / r_med, "time_s_median": r_med, "time_s_min": r_min, "time_s_max": r_max,
                           "wall_s": parts, "codes_that_differ": int((ref_codes.reshape(-1) != codes.reshape(-1)).sum()),
                           "code_slots": int(codes.numel())}
        one["speedup_vs_torch_nn"] = r_med / t_med
        rec["batches"][str(B)] = one
        del x, enc, y, ref_codes
        torch.cuda.empty_cache()
    rec["windows_per_s"] = rec["batches"][str(max(int(b) for b in rec["batches"]))]["windows_per_s"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
