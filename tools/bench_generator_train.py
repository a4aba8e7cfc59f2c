"""One training update of the GRU speech-to-code generator (qpgesture_amd/end2end.py) on one GPU: prints one JSON line.

Per batch size B (windows of 64 000 samples, 30 code slots each): GeneratorTrainer.step - train-mode forward, loss,
backward and Adam, nothing read back - wall clock around a synchronise, median of --reps calls after a warm-up, and the
device time per stage (a device event behind every stage's launches, the median over the same number of calls, summed
over the stages of a kind).  Beside it the same update from torch.nn modules built HERE (Conv1d / BatchNorm1d / LeakyReLU
/ GRU(dropout=0.1) / LayerNorm / Linear, F.cross_entropy, torch.optim.Adam) with the same seeded weights on the same
device in train() mode, timed the same way, and the first update's loss of both.

    python tools/bench_generator_train.py [--batches 1,16,256] [--reps 7]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qpgesture_amd import _lib  # noqa: E402
from qpgesture_amd import end2end  # noqa: E402
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
        self.project = nn.GRU(G.CONVS[-1][1], G.HIDDEN, num_layers=2, dropout=end2end.DROPOUT, bidirectional=True,
                              batch_first=True)
        self.norm = nn.LayerNorm(G.HIDDEN)
        self.out = nn.Linear(G.HIDDEN, G.CODES)

    def forward(self, x, target):
        y = self.project(self.WavEncoder.feat_extractor(x.unsqueeze(1)).transpose(1, 2))[0]
        logits = self.out(self.norm(y[:, :, :G.HIDDEN] + y[:, :, G.HIDDEN:]))
        return torch.nn.functional.cross_entropy(logits.view(-1, G.CODES), target.view(-1))


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
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generator_train: no GPU")
    dev = "cuda:0"
    sd = synth.make_generator_state_dict(1)
    rec = {"tool": "bench_generator_train", "samples_per_window": G.WINDOW, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "batches": {}}
    base = synth.make_wav(2, 8, G.WINDOW)
    for B in (int(b) for b in args.batches.split(",")):
        x = torch.from_numpy(base).to(dev).repeat((B + 7) // 8, 1)[:B].contiguous()
        x = x * torch.linspace(0.5, 1.5, B, device=dev)[:, None]          # (no two windows alike)
        target = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).integers(0, G.CODES, (B, 30))).to(dev)
        tr = end2end.GeneratorTrainer(device=dev, state_dict=sd)
        n0 = _lib.n_calls
        first = float(tr.step(x, target))                                 # warm-up: code objects, the kept buffers
        launches = _lib.n_calls - n0
        tr.step(x, target)
        t_med, t_min, t_max = wall(lambda: tr.step(x, target), args.reps)
        stages = {}
        for _ in range(args.reps):
            ev = []

            def on_stage(stage):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append((stage, e))
            tr.on_stage = on_stage
            tr.step(x, target)
            tr.on_stage = None
            torch.cuda.synchronize()
            one_call = {}
            for (_, a), (stage, b) in zip(ev[:-1], ev[1:]):
                one_call[stage] = one_call.get(stage, 0.0) + a.elapsed_time(b) * 1e-3
            for k, v in one_call.items():
                stages.setdefault(k, []).append(v)
        dev_s = {k: float(np.median(v)) for k, v in stages.items()}
        one = {"updates_per_s": 1.0 / t_med, "time_s_median": t_med, "time_s_min": t_min, "time_s_max": t_max,
               "first_loss": first, "device_s": dict(dev_s, total=sum(dev_s.values())), "calls_per_update": launches}
        ref = TorchGenerator()
        ref.load_state_dict({k[7:]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        ref = ref.to(dev).train()
        opt = torch.optim.Adam(ref.parameters(), lr=end2end.LR, betas=end2end.BETAS)
        losses = []

        def ref_step():
            opt.zero_grad()
            loss = ref(x, target)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        ref_step()                                                        # warm-up: MIOpen picks its algorithms
        ref_step()
        torch.cuda.synchronize()
        r_med, r_min, r_max = wall(ref_step, args.reps)
        one["torch_nn"] = {"updates_per_s": 1.0 / r_med, "time_s_median": r_med, "time_s_min": r_min, "time_s_max": r_max,
                           "first_loss": float(losses[0])}
        one["speedup_vs_torch_nn"] = r_med / t_med
        rec["batches"][str(B)] = one
        del x, tr, ref, opt, losses
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
