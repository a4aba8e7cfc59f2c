"""Matching without the phase gate against the gated matcher, measured on the bench configuration (2048 DB
windows, a 24 s clip = 6 windows, bench.py's data), in ONE process:

  match_clip_gated_ms / match_clip_nophase_ms   host clock around CodeKNN.match_clip (sweeps + walk + wait), the two matchers
                       alternating clip by clip, medians over --steps rounds; the no-phase matcher at every --k
  sweep_for_walk_ms / sweep_settled_ms          sweep_tables(for_walk=True) - the gated clip's tables: walk-relevance cut,
                       prefused gate tables - against sweep_tables(for_walk=False) - what a no-phase clip takes - between two
                       HIP events, alternating
  walk_gated_events_ms   qpg_match_steps on the for_walk tables (gate table + chase; the fusion ran behind the selects) and
  walk_gated_fused_events_ms   on the settled tables (fusion + gate table + chase: 3 launches), between two HIP events
  walk_nophase_events_ms       qpg_match_steps_nophase on the settled tables (2 launches), between two HIP events
  table_ms / chase_ms          its two kernels alone, each between two HIP events (the context's QPG_OPT_NOPHASE_STAGES
                       option makes a call launch one of them)
  rows_scanned_share           the share of a rank row the k-th selection reads per (step, previous code): the table kernel
                       scores every code once whatever k is (no bound stops it), so 1.0 by construction - reported so that a
                       later bounded scan has a figure to beat

and prints ONE JSON line.  `--out FILE` also writes it to FILE.

    python tools/bench_nophase.py --steps 200 --warmup 20 --out profiles/nophase_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n-db", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--k", type=int, nargs="+", default=[0, 3, 15])
    ap.add_argument("--out", default=None)
    return ap


def med_ms(xs):
    return round(1e3 * statistics.median(xs), 5)


def main(argv=None):
    a = build_parser().parse_args(argv)
    import torch
    import bench
    from qpgesture_amd import _lib, synth
    from qpgesture_amd.code_knn import MODE_AUD_TXT, CodeKNN, GestureDB
    from qpgesture_amd.data_processing import interp_wavlm
    if not torch.cuda.is_available():
        raise SystemExit("bench_nophase.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, M = a.n_db, a.windows
    interp, ctx = bench.chunked_db(N, 0, N, seed=0)
    phase = np.random.Generator(np.random.PCG64(5)).standard_normal((N, 240, 4, 8)).astype(np.float32)
    db = GestureDB(synth.make_codes(N, 2), interp, ctx, phase, synth.make_signature(3), device=dev)
    clip = synth.make_db(M, 1000)
    te_i = torch.from_numpy(interp_wavlm(clip["wavlm"])).to(dev)
    te_c = torch.from_numpy(np.ascontiguousarray(clip["context"].squeeze(2))).to(dev)
    gated = CodeKNN(db, rng=np.random.RandomState(123456))
    seed_code, seed_phase = gated.init_code_phase()
    steps = gated.n_steps()
    coins = np.random.RandomState(7).rand(M * steps) > 0.5

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def events_ms(fn, iters=50):
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(statistics.median(ts), 5)

    def run_gated():
        return gated.match_clip(te_i, te_c, M, seed_code=seed_code, seed_phase=seed_phase)

    rows = []
    for k in a.k:
        knn = CodeKNN(db, use_phase=False, desired_k=k, rng=np.random.RandomState(1))

        def run_nophase():
            return knn.match_clip(te_i, te_c, M, seed_code=seed_code, coins=coins)

        for _ in range(a.warmup):
            run_gated()
            run_nophase()
        t_g, t_n = [], []
        for _ in range(a.steps):
            t_g.append(clock(run_gated))
            t_n.append(clock(run_nophase))
        # the walk alone on the settled tables, and its two kernels (the raw entry point on device buffers: a call that
        # launches one kernel of the two writes no status word for CodeKNN.walk to wait for)
        T = knn.sweep_tables(te_i, te_c, M, MODE_AUD_TXT, for_walk=False)
        Q = M * steps
        ws = torch.empty((int(_lib.load().qpg_match_steps_nophase_ws_bytes(1, M, steps, db.K)),), dtype=torch.uint8,
                         device=dev)
        seed_d = torch.tensor([seed_code], dtype=torch.int32, device=dev)
        coins_d = torch.from_numpy(coins.astype(np.uint8)).to(dev)
        o_codes, o_side, o_cand, o_status = (torch.empty((n,), dtype=torch.int32, device=dev) for n in (M * 30, Q, Q, 2))

        def walk():
            _lib.call("qpg_match_steps_nophase", dev, T["aud_rank"], T["aud_idx"], T["txt_rank"], T["txt_idx"], db.pos_rank,
                      db.freq_rank, db.code, db.code.shape[1], db.aud_cidx, db.Ga, db.txt_cidx, db.Gt, MODE_AUD_TXT, k, M,
                      steps, db.K, 1, seed_d, coins_d, o_codes, o_side, o_cand, o_status, 2, None, ws, ws.numel())

        walk()
        both = events_ms(walk)
        stage = {}
        try:
            for name, mask in (("table_ms", 1), ("chase_ms", 2)):
                _lib.set_option(dev, _lib.QPG_OPT_NOPHASE_STAGES, mask)
                stage[name] = events_ms(walk)
        finally:
            _lib.set_option(dev, _lib.QPG_OPT_NOPHASE_STAGES, 3)
        torch.cuda.synchronize(dev)
        codes, _, sides = run_nophase()
        assert np.array_equal(o_codes.cpu().numpy().reshape(M, 30), codes) and o_status.cpu().numpy().tolist() == [0, 0]
        rows.append(dict(desired_k=k, match_clip_gated_ms=med_ms(t_g), match_clip_nophase_ms=med_ms(t_n),
                         walk_nophase_events_ms=both, **stage, rows_scanned_share=1.0, rank_cut=bool(knn._last_rank_cut),
                         audio_sides=int((sides == 0).sum()), fallbacks=int(knn.fallbacks)))
    # the two kinds of tables, and the gated walk on each
    sweeps = {True: [], False: []}
    for i in range(a.warmup + 50):
        for fw in (True, False):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gated.sweep_tables(te_i, te_c, M, MODE_AUD_TXT, for_walk=fw)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                sweeps[fw].append(e0.elapsed_time(e1))
    Tw = gated.sweep_tables(te_i, te_c, M, MODE_AUD_TXT, for_walk=True)
    cut = bool(gated._last_rank_cut)
    Ts = gated.sweep_tables(te_i, te_c, M, MODE_AUD_TXT, for_walk=False)
    walk_w = events_ms(lambda: gated.walk(Tw, M, 0, MODE_AUD_TXT, seed_code, seed_phase, sync=False))
    walk_s = events_ms(lambda: gated.walk(Ts, M, 0, MODE_AUD_TXT, seed_code, seed_phase, sync=False))
    out = dict(tool="bench_nophase", n_db=N, windows=M, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(dev), sweep_for_walk_ms=round(statistics.median(sweeps[True]), 5),
               sweep_settled_ms=round(statistics.median(sweeps[False]), 5), for_walk_rank_cut=cut,
               walk_gated_events_ms=walk_w, walk_gated_fused_events_ms=walk_s, nophase=rows)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
