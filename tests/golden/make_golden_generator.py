#!/usr/bin/env python
"""Golden vectors for the GRU speech-to-code generator from the REFERENCE model (imported from /root/reference; build
container only).  No end2end checkpoint ships with the reference, so weights and audio are seeded
(qpgesture_amd.synth.make_generator_state_dict / make_wav) and loaded into the reference's own Generator_gru, which is
run in eval mode in f32 and, after .double(), in f64.

    python tests/golden/make_golden_generator.py

generator_full.npz    B = 6 windows of 64 000 samples (T = 30)
generator_edges.npz   B = 3 at each of n = 5 866 (T = 1), 7 810 (T = 2) and 66 000 (T = 31); keys carry the prefix n<n>_

Per run: `codes` at every position (B, T); for each tap (enc: the WavEncoder's output, gru0 / gru1: the GRU layers'
outputs, ln: the LayerNorm output, logits) the f64 values on `tap_rows` of the flattened (B T) rows and e32_<tap> = max
|f32 run - f64 run| over the WHOLE tensor; `target` (seeded) with the cross-entropy loss64 and loss32; min_margin, the
smallest top-2 gap of the f64 logits.  The wav and the weights are not stored: the tests regenerate them from the seeds.

Asserted before anything is written: min_margin >= 64 e32_logits in every run (so codes within the tests' 8 e32 tolerance
of the f64 logits are the f64 codes: exact code equality needs no exclusions), no exact ties among the logits, at least 8
distinct codes in the full fixture, and the f32 run's codes equal the f64 run's.  If a seed fails, change the seed.

cut_*: what the reference's own window arithmetic (codebook/inference.py:30-41 and :67-75, read from the reference's file
and executed as they stand, not restated here) gives for a ramp of each length in CUT_LENGTHS, without max_frames and
with max_frames = 3600: per case the number of windows and, per window, its start sample and its count of clip samples
(the rest is the zero padding)."""
import math
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from qpgesture_amd import synth  # noqa: E402

REF = "/root/reference/codebook"
SEED_W, SEED_WAV, SEED_TARGET = 29, 22, 23
TAPS = ("enc", "gru0", "gru1", "ln", "logits")
TAP_STEP = {"full": 7, "edges": 5}
EDGE_LENGTHS = (5866, 7810, 66000)
CUT_LENGTHS = (1, 63999, 64000, 64001, 128000, 150000)
CUT_MAX_FRAMES = 3600


def build_model(sd):
    import torch
    sys.path.insert(0, os.path.join(REF, "generate"))
    from generate import Generator_gru
    model = Generator_gru().eval()
    model.load_state_dict({k[len("module."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model


def run(model, wav, dtype):
    """The reference's forward(), with its intermediate tensors."""
    import torch
    with torch.no_grad():
        x = torch.from_numpy(wav).to(dtype)
        enc = model.WavEncoder(x)
        gru = model.project
        outs, inp = [], enc
        for layer in range(2):                      # the stacked layers one by one (eval: no dropout between them)
            one = torch.nn.GRU(inp.shape[-1], model.hidden_size, 1, bidirectional=True, batch_first=True).to(dtype).eval()
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                for suffix in ("", "_reverse"):
                    getattr(one, "%s_l0%s" % (n, suffix)).copy_(getattr(gru, "%s_l%d%s" % (n, layer, suffix)))
            inp, _ = one(inp)
            outs.append(inp)
        both, _ = gru(enc, None)
        assert torch.equal(both, outs[1]) or float((both - outs[1]).abs().max()) < (1e-12 if dtype == torch.float64 else 1e-5)
        s = both[:, :, :model.hidden_size] + both[:, :, model.hidden_size:]
        ln = model.norm(s)
        logits, _ = model(x)
        assert float((logits - model.out(ln)).abs().max()) == 0.0
        code = model.sample(x)[0]
    return dict(enc=enc.numpy(), gru0=outs[0].numpy(), gru1=outs[1].numpy(), ln=ln.numpy(), logits=logits.numpy(),
                sample=code.numpy())


def one_run(model32, model64, wav, seed_target, step, prefix=""):
    import torch
    r32, r64 = run(model32, wav, torch.float32), run(model64, wav, torch.float64)
    B, T, N = r64["logits"].shape
    codes = np.argmax(r64["logits"], -1).astype(np.int64)
    assert np.array_equal(r64["sample"], codes.reshape(1, -1)) and r64["sample"].dtype == np.int64
    assert np.array_equal(r32["sample"], r64["sample"]), "the f32 run's codes differ from the f64 run's"
    top2 = np.sort(r64["logits"].reshape(-1, N), -1)[:, -2:]
    min_margin = float((top2[:, 1] - top2[:, 0]).min())
    for row in r64["logits"].reshape(-1, N):
        assert len(np.unique(row)) == N, "exact logit ties"
    rows = np.arange(0, B * T, step)
    out = {prefix + "codes": codes, prefix + "tap_rows": rows.astype(np.int32), prefix + "min_margin": np.float64(min_margin)}
    for tap in TAPS:
        a64, a32 = r64[tap], r32[tap]
        out[prefix + tap] = a64.reshape(B * T, -1)[rows]
        out[prefix + "e32_" + tap] = np.float64(np.abs(a32.astype(np.float64) - a64).max())
    assert min_margin >= 64 * out[prefix + "e32_logits"], (prefix, min_margin, out[prefix + "e32_logits"])
    target = np.random.Generator(np.random.PCG64(seed_target)).integers(0, N, (B, T))
    with torch.no_grad():
        t = torch.from_numpy(target)
        l64 = float(model64(torch.from_numpy(wav).double(), t)[1])
        l32 = float(model32(torch.from_numpy(wav), t)[1])
    out.update({prefix + "target": target.astype(np.int64), prefix + "loss64": np.float64(l64), prefix + "loss32": np.float64(l32)})
    print("%s B %d T %d: %d distinct codes, min margin %.3e = %.0f x e32_logits; e32 %s; |gru| max %.3f; loss %.6f (f32 off by %.2e)"
          % (prefix or "full", B, T, len(np.unique(codes)), min_margin, min_margin / out[prefix + "e32_logits"],
             " ".join("%s %.2e" % (tap, out[prefix + "e32_" + tap]) for tap in TAPS), np.abs(r64["gru1"]).max(), l64,
             abs(l32 - l64)))
    return out


def reference_cut(length, max_frames):
    """(start, clip samples) per window, by lines 30-41 and 67-75 of the reference's inference.py."""
    with open(os.path.join(REF, "inference.py")) as f:
        src = f.read().split("\n")
    head = textwrap.dedent("\n".join(src[29:41]))
    loop = textwrap.dedent("\n".join(src[66:75]))
    ns = dict(math=math, np=np, audio_raw=np.arange(1, length + 1, dtype=np.float32), audio_sr=16000, max_frames=max_frames,
              args=types.SimpleNamespace(n_poses=240, motion_resampling_framerate=60), windows=[], print=lambda *a: None)
    exec(head, ns)
    exec(loop + "\n    windows.append(in_audio)\n", ns)
    assert len(ns["windows"]) == ns["num_subdivision"] and all(len(w) == 64000 for w in ns["windows"])
    spans = []
    for w in ns["windows"]:
        valid = int(np.count_nonzero(w))
        assert np.all(w[valid:] == 0)
        spans.append((int(w[0]) - 1 if valid else -1, valid))
    return spans


def main():
    import copy
    sd = synth.make_generator_state_dict(SEED_W)
    model32 = build_model(sd)
    model64 = copy.deepcopy(model32).double()
    full = dict(seed_w=np.int64(SEED_W), seed_wav=np.int64(SEED_WAV), seed_target=np.int64(SEED_TARGET))
    full.update(one_run(model32, model64, synth.make_wav(SEED_WAV, 6, 64000), SEED_TARGET, TAP_STEP["full"]))
    assert len(np.unique(full["codes"])) >= 8, "fewer than 8 distinct codes"
    n_cases, starts, valid, lens, maxf = [], [], [], [], []
    for L in CUT_LENGTHS:
        for mf in (None, CUT_MAX_FRAMES):
            spans = reference_cut(L, mf)
            lens.append(L)
            maxf.append(0 if mf is None else mf)
            n_cases.append(len(spans))
            starts += [s for s, _ in spans]
            valid += [v for _, v in spans]
    full.update(cut_len=np.array(lens, np.int64), cut_max_frames=np.array(maxf, np.int64), cut_n=np.array(n_cases, np.int64),
                cut_start=np.array(starts, np.int64), cut_valid=np.array(valid, np.int64))
    print("cut_windows:", list(zip(lens, maxf, n_cases)))
    edges = dict(seed_w=np.int64(SEED_W), seed_wav=np.int64(SEED_WAV + 1), seed_target=np.int64(SEED_TARGET + 1),
                 lengths=np.array(EDGE_LENGTHS, np.int64))
    for n in EDGE_LENGTHS:
        # (the same seeded audio for every length: its first n samples)
        edges.update(one_run(model32, model64, np.ascontiguousarray(synth.make_wav(SEED_WAV + 1, 3, 66000)[:, :n]),
                             SEED_TARGET + 1, TAP_STEP["edges"], "n%d_" % n))
    for name, d in (("generator_full.npz", full), ("generator_edges.npz", edges)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
