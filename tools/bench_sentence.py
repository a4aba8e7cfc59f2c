"""Sentence embeddings (qpgesture_amd/sentence.py) throughput on one GPU at MiniLM size: prints one JSON line.

The workload is the context column of a 2048-window database: 61 440 code-slot sentences, 30 % of them empty
([CLS] [SEP]), the others 3 .. 24 tokens long (seeded, uniform), random ids - so only the empty ones repeat.  Seeded
weights (synth.make_bert_state_dict of BERT_MINILM).  Timed: SentenceEncoder.encode_ids from id lists on the host to the
(S, 384) result on the device, wall clock around a synchronise, median of --reps calls after a warm-up - with the
duplicates encoded once (the default) and with every sentence encoded (--no-dedup semantics, reported beside it).  One more
call records a device event behind every launch of every pass; the time between events is summed per kind of launch:
GEMM (q | k | v, attention output, fc1, fc2), attention, other (embedding + LayerNorm, the LayerNorms, the mean pool).

    python tools/bench_sentence.py [--sentences 61440] [--reps 5] [--budget 32768]

For comparison the reference (process/make_beat_dataset.py:563-564) makes one SentenceTransformer.encode call per code slot,
one sentence per call: 61 440 calls of a six-block model for this workload.  Its time has not been measured here."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qpgesture_amd import sentence as S  # noqa: E402
from qpgesture_amd import synth  # noqa: E402


def make_sentences(n, seed=5, vocab=30522):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = np.where(rng.random(n) < 0.3, 2, rng.integers(3, 25, n))
    return [[101] + [int(i) for i in rng.integers(1000, vocab, L - 2)] + [102] for L in lengths]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=61440)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=int, default=S.TOKEN_BUDGET)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sentence: no GPU")
    dev = "cuda:0"
    cfg = synth.BERT_MINILM
    model = S.SentenceEncoder(cfg, device=dev, token_budget=args.budget).load_state_dict(synth.make_bert_state_dict(1, cfg))
    seqs = make_sentences(args.sentences)
    tokens = sum(len(s) for s in seqs)
    distinct = len({tuple(s) for s in seqs})
    rec = {"tool": "bench_sentence", "sentences": len(seqs), "tokens": tokens, "distinct_sentences": distinct,
           "token_budget": args.budget, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for key, dedup in (("dedup", True), ("every_sentence", False)):
        out = model.encode_ids(seqs, dedup=dedup)                  # warm-up: code objects, the workspace
        torch.cuda.synchronize()
        assert out.shape == (len(seqs), cfg["hidden_size"]) and bool(torch.isfinite(out).all())
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            model.encode_ids(seqs, dedup=dedup)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        t = float(np.median(ts))
        rec[key] = {"time_s_median": t, "time_s_min": float(min(ts)), "time_s_max": float(max(ts)),
                    "sentences_per_s": len(seqs) / t, "tokens_per_s": tokens / t}
        ev = []

        def on_stage(stage, _view):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((stage, e))
        model.encode_ids(seqs, dedup=dedup, on_stage=on_stage)
        torch.cuda.synchronize()
        split = {"gemm": 0.0, "attention": 0.0, "other": 0.0}
        for (_, a), (stage, b) in zip(ev[:-1], ev[1:]):
            if stage == "start":
                continue                                           # (between two passes: the host's packing, not a launch)
            kind = stage.rsplit(".", 1)[-1]
            split["gemm" if kind in ("qkv", "out", "fc1", "fc2") else "attention" if kind == "att" else "other"] += \
                a.elapsed_time(b) * 1e-3
        rec[key]["device_s"] = dict(split, total=sum(split.values()), passes=sum(1 for s, _ in ev if s == "start"))
    rec["sentences_per_s"] = rec["dedup"]["sentences_per_s"]
    rec["tokens_per_s"] = rec["dedup"]["tokens_per_s"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
