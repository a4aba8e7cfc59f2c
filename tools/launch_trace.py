"""What one matching step launches, as data: every C-ABI launch (_lib.call and the launch half of _lib.prepare), every
torch.cuda.Event.record and every Stream.wait_event / wait_stream, in host order, for a grid of matcher configurations and
for the VQ-VAE's entry points (`vqvae/*`: inference, training steps, the refresh after one).

    python tools/launch_trace.py out.json            # {cell: [entry, ...]}; prints the number of entries per cell
    python tools/launch_trace.py --diff a.json b.json   # exit status 1 and the first differing entry of every unequal cell

An entry of a launch is [entry point, stream ordinal, arguments]: scalars by value, integers that are addresses (pinned
seed / result blocks, doorbell and signal words) as "ptr", tensors as [dtype, numel].  Streams and events are numbered in
order of first appearance inside a cell.  The tool uses the package's public API only, so the same file runs on two trees:
a change of the host code that must leave the launches alone is checked by running it on both and comparing the files."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def diff(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = 0
    for cell in sorted(set(a) | set(b)):
        ea, eb = a.get(cell), b.get(cell)
        if ea == eb:
            print("%-44s %4d entries  equal" % (cell, len(ea)))
            continue
        bad += 1
        if ea is None or eb is None:
            print("%-44s only in %s" % (cell, pb if ea is None else pa))
            continue
        i = next((i for i, (x, y) in enumerate(zip(ea, eb)) if x != y), min(len(ea), len(eb)))
        print("%-44s %d / %d entries  DIFFER at %d:\n   %s\n   %s" % (cell, len(ea), len(eb), i, ea[i:i + 1], eb[i:i + 1]))
    print("%d cells, %d differ" % (len(set(a) | set(b)), bad))
    return 1 if bad else 0


if len(sys.argv) == 4 and sys.argv[1] == "--diff":
    sys.exit(diff(sys.argv[2], sys.argv[3]))

import numpy as np
import torch

from qpgesture_amd import _lib, synth
from qpgesture_amd.code_knn import MODE_AUD, MODE_AUD_TXT, MODE_TXT, CodeKNN, GestureDB
from tests.helpers import fixture_arrays, load_golden

dev = torch.device("cuda:0")
log, streams, events = [], {}, {}


def _ordinal(table, key, keep=None):
    if key not in table:
        table[key] = (len(table), keep)          # (the object is kept: its id / handle cannot be reused inside a cell)
    return table[key][0]


def _stream(s=None):
    s = torch.cuda.current_stream(dev) if s is None else s
    return _ordinal(streams, s.cuda_stream)


def _arg(a):
    if isinstance(a, torch.Tensor):
        return [str(a.dtype).replace("torch.", ""), a.numel()]
    if isinstance(a, bool) or a is None or isinstance(a, (float, str)):
        return a
    if isinstance(a, (int, np.integer)):
        return "ptr" if abs(int(a)) >= 1 << 32 else int(a)
    if isinstance(a, np.floating):
        return float(a)
    if isinstance(a, ctypes.Array):
        return list(a)
    if isinstance(a, ctypes.c_void_p):
        return "ptr"
    return type(a).__name__


_call, _prepare = _lib.call, _lib.prepare
_record, _wait_event, _wait_stream = torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream


def call(name, device, *args):
    log.append([name, _stream(), [_arg(a) for a in args]])
    return _call(name, device, *args)


def prepare(name, device, *args):
    launch, stream = _prepare(name, device, *args), _stream()          # (it launches on the stream that is current NOW)

    def traced():
        log.append([name, stream, [_arg(a) for a in args]])
        return launch()
    return traced


def record(self, stream=None):
    log.append(["<event.record>", _stream(stream), _ordinal(events, id(self), self)])
    return _record(self) if stream is None else _record(self, stream)


def wait_event(self, event):
    log.append(["<stream.wait_event>", _stream(self), _ordinal(events, id(event), event)])
    return _wait_event(self, event)


def wait_stream(self, stream):
    log.append(["<stream.wait_stream>", _stream(self), _stream(stream)])
    return _wait_stream(self, stream)


def traced(fn):
    """Run fn() with the wrappers in place; returns its entries."""
    log.clear(), streams.clear(), events.clear()
    _stream()                                                           # the caller's stream is ordinal 0
    _lib.call, _lib.prepare = call, prepare
    torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = record, wait_event, wait_stream
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.call, _lib.prepare = _call, _prepare
        torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = (
            _record, _wait_event, _wait_stream)
    return [list(e) for e in log]


def tensors(A):
    return (torch.from_numpy(np.ascontiguousarray(A["te_interp"], np.float32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(A["te_ctx"], np.float32)).to(dev))


def vqvae_cells(cells):
    """The codec's entry points, on a full-width model (T-packed kernels) and a reduced-width one (no T-packs: the f32
    per-layer kernels; the split-f16 entry points are exercised at full width only, like everywhere else in the project).
    Two shapes: (8, 3200) frames - resnet levels of 1600 / 800 / 400 positions, on both sides of the fused-block rule with
    256 CUs - and (1, 360), below it on every level."""
    from qpgesture_amd.optim import Adam
    from qpgesture_amd.vqvae import VQVAE

    def cell(name, fn):
        cells[name] = traced(fn)
        print("%-44s %4d entries" % (name, len(cells[name])), flush=True)

    def step(m, opt, x):
        m(x)
        m.backward()
        opt.step()

    small = dict(width=64, emb_width=64, l_bins=96)
    for mname, hps in (("w512", None), ("w64", small)):
        for B, T in ((8, 3200), (1, 360)):
            torch.manual_seed(11)                                       # (init_k / update_k draw from the CPU generator)
            m = VQVAE(hps, 135, device=dev).load_state_dict(synth.make_vqvae_state_dict(7, hps))
            x = torch.randn((B, T, 135), device=dev, generator=torch.Generator(device=dev).manual_seed(6))
            ids = m.encode(x)[0]
            pre = "vqvae/%s/%dx%d/" % (mname, B, T)
            cell(pre + "encode", lambda: m.encode(x))
            cell(pre + "encode_latent/f32", lambda: m.encode_latent(x))
            cell(pre + "quantise/margin", lambda: m.quantise(m.encode_latent(x), return_margin=True))
            cell(pre + "decode", lambda: m.decode([ids[:, :30]]))
            cell(pre + "forward/eval", lambda: m.eval()(x))
            if hps is None:
                cell(pre + "encode_latent/f16x3", lambda: m.encode_latent(x, precision="f16x3"))
                cell(pre + "encode_f16x3", lambda: m.encode_f16x3(x))
                cell(pre + "encode_f16x3_device", lambda: m.encode_f16x3_device(x))
                cell(pre + "decode_f16x3/force", lambda: m.decode_f16x3([ids], force=True))
            opt = Adam(m.parameters(), lr=1e-4, betas=(0.5, 0.999))
            m.train()
            for fused in (True, False):
                m.train_fused = fused
                cell(pre + "train/2_steps/fused=%d" % fused, lambda: (step(m, opt, x), step(m, opt, x)))
            m.train_fused = True
            if hps is None:
                m.train_precision = "f16x3"
                cell(pre + "train/step/f16x3", lambda: step(m, opt, x))
                m.train_precision = "f32"
                m.eval()
                cell(pre + "after_step/decode_f16x3", lambda: m.decode_f16x3([ids], force=True))
                m.train()
                step(m, opt, x)
            m.eval()
            cell(pre + "after_step/encode", lambda: m.encode(x))


def main(out_path):
    cells = {}
    vqvae_cells(cells)
    A = fixture_arrays(96, 3, 5, 6, 7, 8)
    M = 3
    te_i, te_c = tensors(A)
    db = GestureDB(A["code"], A["tr_interp"], A["tr_ctx"], A["tr_phase"], A["sig"], device=dev)

    def matcher(d=db, **knobs):
        knn = CodeKNN(d, rng=np.random.RandomState(3))
        for k, v in knobs.items():
            setattr(knn, k, v)
        return knn

    def clip(name, knn, mode=MODE_AUD_TXT, tables=False, ti=te_i, tc=te_c, m=M):
        cells[name] = traced(lambda: knn.match_clip(ti, tc, m, mode=mode, return_tables=tables))
        print("%-44s %4d entries" % (name, len(cells[name])), flush=True)

    for mname, mode in (("aud_txt", MODE_AUD_TXT), ("aud", MODE_AUD), ("txt", MODE_TXT)):
        clip("clip/%s" % mname, matcher(), mode)
        clip("clip/%s/return_tables" % mname, matcher(), mode, tables=True)
    flips = {"audio_precision=f64": dict(audio_precision="f64"), "audio_precision=exact": dict(audio_precision="exact"),
             "audio_kernel=mx": dict(audio_kernel="mx"), "text_kernel=valu": dict(text_kernel="valu"),
             "fused_pack=off": dict(fused_pack=False), "split_fuse=off": dict(split_fuse=False),
             "rank_cut=off": dict(rank_cut=False), "tie_eps=0": dict(tie_eps=0.0), "host_ranks": dict(host_ranks=True),
             "mixed_single_launch": dict(mixed_single_launch=True), "serial_walk": dict(serial_walk=True),
             "order=text_after_sweep": dict(text_after_sweep=True, audio_first=False),
             "order=text_first": dict(text_after_sweep=False, audio_first=False),
             "order=audio_first": dict(text_after_sweep=False, audio_first=True),
             "order=one_stream": dict(overlap_sweeps=False)}
    for name, knobs in flips.items():
        clip("knob/" + name, matcher(**knobs))
    clip("knob/bench_events", matcher(kernel_events=[], kernel_events_every=1))

    db16 = GestureDB(A["code"], A["tr_interp"], A["tr_ctx"], A["tr_phase"], A["sig"], device=dev, feature_dtype="f16")
    clip("f16/aud_txt", matcher(db16))
    clip("f16/audio_kernel=mx", matcher(db16, audio_kernel="mx"))
    clip("f16/audio_precision=f64", matcher(db16, audio_precision="f64"))

    Av = fixture_arrays(40, 2, 20, 21, 22, 23, wavlm_dim=8)
    dbv = GestureDB(Av["code"], Av["tr_interp"], Av["tr_ctx"], Av["tr_phase"], Av["sig"], device=dev, wavvq=Av["tr_wavvq"])
    tv = torch.from_numpy(np.ascontiguousarray(Av["te_wavvq"])).to(dev)
    tcv = tensors(Av)[1]
    for name, knobs in (("wavvq/aud_txt", {}), ("wavvq/order=text_after_sweep", dict(text_after_sweep=True, audio_first=False))):
        knn = CodeKNN(dbv, use_wavlm=False, use_wavvq=True, rng=np.random.RandomState(2))
        for k, v in knobs.items():
            setattr(knn, k, v)
        code0 = int(Av["code"][0, 0])               # (a seed the wavvq mode's own draw cannot give: GestureKNN.py:464-469)
        cells[name] = traced(lambda: knn.match_clip(tv, tcv, 2, seed_code=code0, seed_phase=np.zeros((8, 16), np.float32)))
        print("%-44s %4d entries" % (name, len(cells[name])), flush=True)

    rng = np.random.RandomState(9)
    for clips in (2, 16):                       # 16 x 3 windows x 8 steps: beyond split_fuse_max_steps
        knn = matcher()
        ti, tc = te_i.repeat(clips, 1, 1), te_c.repeat(clips, 1, 1)
        seeds, phases = rng.randint(0, 512, size=clips), rng.standard_normal((clips, 8, 16)).astype(np.float32)
        name = "walk_batch/%d_clips" % clips
        cells[name] = traced(lambda: knn.walk_batch(knn.sweep_tables(ti, tc, clips * M, for_walk=True), M, clips, seeds,
                                                    phases))
        print("%-44s %4d entries" % (name, len(cells[name])), flush=True)

    # several takes of one clip: on the tables' own (prefused) gate tables, and fusing the ranks itself
    seeds, phases = rng.randint(0, 512, size=5), rng.standard_normal((5, 8, 16)).astype(np.float32)
    for name, for_walk in (("walk_takes/prefused", True), ("walk_takes/own_fusion", False)):
        knn = matcher()
        cells[name] = traced(lambda: knn.walk_takes(knn.sweep_tables(te_i, te_c, M, for_walk=for_walk), M, seeds, phases))
        print("%-44s %4d entries" % (name, len(cells[name])), flush=True)

    sc, sp = matcher().init_code_phase()
    from qpgesture_amd.vqvae import VQVAE
    enc = VQVAE(None, 135, device=dev).load_state_dict(synth.make_vqvae_state_dict(7))
    x = torch.randn((4, 240, 135), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    graphs = [("graph/plain", {}, None), ("graph/sweep_signal", dict(sweep_signal=True), None),
              ("graph/aud/sweep_signal", dict(sweep_signal=True, mode=MODE_AUD), None),
              ("graph/encoder_at_start", dict(encoder=enc, encode_input=x), "start"),
              ("graph/encoder_behind_sweep", dict(encoder=enc, encode_input=x), "sweep_end")]
    for name, kw, enc_at in graphs:             # the first run: two eager warm-up bodies, the capture, one replay
        if enc_at is not None:
            os.environ["QPG_ENCODE_AT"] = enc_at
        knn = matcher()
        cells[name] = traced(lambda: knn.capture_clip_graph(M, audio=te_i, context=te_c, **kw).run(te_i, te_c, sc, sp))
        os.environ.pop("QPG_ENCODE_AT", None)
        print("%-44s %4d entries" % (name, len(cells[name])), flush=True)

    # the row-shard path on one rank over RCCL (world_size 1): both exchange forms, mixed / f64 / exact shards
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        shard = {"mixed": dict(sharded_mixed_min_gflop=0.0), "f64": dict(sharded_mixed_min_gflop=1e9),
                 "exact": dict(audio_precision="exact"), "mixed_mx": dict(sharded_mixed_min_gflop=0.0, audio_kernel="mx")}
        for pname, knobs in shard.items():
            for form, owner in (("all_to_all", True), ("all_gather", False)):
                knn = matcher(force_sharded=True, **knobs)
                name = "sharded/%s/%s" % (pname, form)
                cells[name] = traced(lambda: knn.walk(knn.sweep_tables(te_i, te_c, M, owner_blocks=owner, for_walk=True),
                                                      M, seed_code=sc, seed_phase=sp))
                print("%-44s %4d entries" % (name, len(cells[name])), flush=True)
    finally:
        dist.destroy_process_group()

    # the two re-match paths: a near-silent clip overflows the capped audio lists (-> "exact"), an all-zero text query the
    # prefilter's band list (-> the exact-order text sweep)
    g = load_golden("shipped_nearsilent_n48_m2_s50")
    ntr, nte, s0, s1, s2, s3, _ = [int(v) for v in g["meta"]]
    An = fixture_arrays(ntr, nte, s0, s1, s2, s3, variant=(str(g["variant"]) or None) if "variant" in g.files else None)
    dbn = GestureDB(An["code"], An["tr_interp"], An["tr_ctx"], An["tr_phase"], An["sig"], device=dev,
                    freq_rank=g["step_freq_score"])
    knn = CodeKNN(dbn, rng=np.random.RandomState(123456))
    clip("rematch/audio_overflow", knn, ti=tensors(An)[0], tc=tensors(An)[1], m=nte)
    assert knn.fallbacks == 1
    Az = fixture_arrays(700, 3, 5, 6, 7, 8)
    Az["te_ctx"][0, :, :] = 0.0
    dbz = GestureDB(Az["code"], Az["tr_interp"], Az["tr_ctx"], Az["tr_phase"], Az["sig"], device=dev)
    knn = matcher(dbz)
    clip("rematch/text_overflow", knn, ti=tensors(Az)[0], tc=tensors(Az)[1])
    assert knn.fallbacks == 1 and knn.text_fallbacks == 1
    json.dump(cells, open(out_path, "w"))
    print("%d cells, %d entries -> %s" % (len(cells), sum(len(v) for v in cells.values()), out_path))


if __name__ == "__main__":
    main(sys.argv[1])
