"""Micro-benchmark of the audio sweeps alone, through their four C entry points.

    python tools/bench_audio.py                      # the list: {f64, mx} x {f32 track, f16 track} x Q in {48, 768}
    python tools/bench_audio.py mx f16 48            # one configuration (for rocprofv3 --pmc passes)
    python tools/bench_audio.py ... --seconds 0.2    # length of a timed window (default 1 s)

N = 2048 windows, T = 180, F = 1024, G = 26.  Every configuration runs behind its own warm-up and is timed between two
device events over as many calls as fill the window; one line per configuration, then one JSON line with all of them.
QPG_LIB_PATH selects another build of the library (qpgesture_amd/_lib.py), e.g. the parent commit's for an A/B."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from qpgesture_amd import _lib

N, T, F, G = 2048, 180, 1024, 26
dev = torch.device("cuda:0")


def sweep(kind, track, Q):
    """A callable that runs one sweep of `kind` ('f64' | 'mx') over a `track` ('f32' | 'f16') base for Q queries."""
    base = torch.randn((N, T, F), device=dev)
    if track == "f16":
        base = base.half()
    q32 = torch.randn((Q, 6 * F), device=dev)
    qn2 = (q32.double() ** 2).sum(1)
    cn2 = torch.rand((N, G), device=dev, dtype=torch.float64) + 6000
    cand_t = torch.arange(G, device=dev, dtype=torch.int32) * 6
    D = torch.empty((Q, N * G), device=dev, dtype=torch.float64)
    name = "qpg_audio_cosine_" + kind + ("_h" if track == "f16" else "")
    if kind == "mx":
        return lambda: _lib.call(name, dev, base, N, T, F, cand_t, G, 6, 2, cn2, q32, qn2, Q, D, 0, D.stride(0), None)
    return lambda: _lib.call(name, dev, base, N, T, F, cand_t, G, 6, 2, cn2, q32, qn2, Q, D, D.stride(0))


def timed(run, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters          # ms per call


def measure(kind, track, Q, seconds):
    run = sweep(kind, track, Q)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    iters = max(10, int(1.3 * seconds * 1e3 / timed(run, 10)) + 1)    # the second warm-up sizes the window
    ms = timed(run, iters)
    tf = 2.0 * Q * N * G * 6 * F / ms / 1e9
    print("%-3s %s Q=%-4d %9.1f us  %6.2f TF  (%d calls, %.2f s)" % (kind, track, Q, ms * 1e3, tf, iters, ms * iters / 1e3),
          flush=True)
    return {"kind": kind, "track": track, "Q": Q, "us": round(ms * 1e3, 2), "calls": iters}


if __name__ == "__main__":
    args = sys.argv[1:]
    seconds = float(args.pop(args.index("--seconds") + 1)) if "--seconds" in args else 1.0
    args = [a for a in args if a != "--seconds"]
    if args:
        if len(args) != 3 or args[0] not in ("f64", "mx") or args[1] not in ("f32", "f16"):
            sys.exit("usage: bench_audio.py [f64|mx f32|f16 Q] [--seconds S]")
        configs = [(args[0], args[1], int(args[2]))]
    else:
        configs = [(k, t, q) for k in ("f64", "mx") for t in ("f32", "f16") for q in (48, 768)]
    print(json.dumps({"lib": _lib.LIB_PATH, "configs": [measure(k, t, q, seconds) for k, t, q in configs]}))
