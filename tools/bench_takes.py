"""Several takes of one clip from one sweep, measured on the bench configuration (2048 DB windows, a 24 s
clip = 6 windows, bench.py's data): for S in {1, 8, 64, 512}

  replay_takes_ms      one captured replay with n_takes = S (capture_clip_graph(..., n_takes=S)), host clock around
                       launch + wait, median over --steps replays
  replay_one_x_S_ms    S replays of the ONE-take graph (today's route for S takes), alternating with the above in the same
                       process: per round one takes-replay, then S one-take replays
  extra_over_one_ms    replay_takes_ms - the median ONE-take replay measured in that same alternation
  sweep_plus_walks_ms  sweep_tables once + S x walk() (the closest low-level route before this feature)
  step0_ms / chase_ms / epilogue_ms   the three take kernels alone, each between two HIP events (the context's
                       QPG_OPT_TAKES_STAGES option makes a call launch one of them; a timed call = the gate table, which is
                       timed alone as gate_table_ms, + that kernel), medians of 50
  walk_takes_events_ms the whole multi-take walk (gate table + the three) between two events, walk_one_take_events_ms the
                       same call with one seed
  n_distinct           different code sequences among the S takes (seeds: S successive init_code_phase() draws)
  decode_batched_ms / decode_singles_ms   VQVAE.decode of the S takes as one (S, 30 M) batch against S decodes of (1, 30 M)

and prints ONE JSON line.  `--out FILE` also writes it to FILE.

    python tools/bench_takes.py --steps 200 --warmup 20 --out profiles/takes_bench.json
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
    ap.add_argument("--takes", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=None)
    return ap


def med_ms(xs):
    return round(1e3 * statistics.median(xs), 5)


def main(argv=None):
    a = build_parser().parse_args(argv)
    import torch
    import bench
    from qpgesture_amd import _lib, synth
    from qpgesture_amd.code_knn import CodeKNN, GestureDB
    from qpgesture_amd.data_processing import interp_wavlm
    if not torch.cuda.is_available():
        raise SystemExit("bench_takes.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, M = a.n_db, a.windows
    interp, ctx = bench.chunked_db(N, 0, N, seed=0)
    phase = np.random.Generator(np.random.PCG64(5)).standard_normal((N, 240, 4, 8)).astype(np.float32)
    db = GestureDB(synth.make_codes(N, 2), interp, ctx, phase, synth.make_signature(3), device=dev)
    knn = CodeKNN(db, rng=np.random.RandomState(123456))
    clip = synth.make_db(M, 1000)
    te_i = torch.from_numpy(interp_wavlm(clip["wavlm"])).to(dev)
    te_c = torch.from_numpy(np.ascontiguousarray(clip["context"].squeeze(2))).to(dev)
    draws = [knn.init_code_phase() for _ in range(max(a.takes))]
    codes_all = np.array([d[0] for d in draws], np.int64)
    phases_all = np.stack([d[1] for d in draws]).astype(np.float32)

    g1 = knn.capture_clip_graph(M, audio=te_i, context=te_c)
    for _ in range(a.warmup):
        g1.run_ints(int(codes_all[0]), phases_all[0])
    model = None
    if not a.no_decode:
        from qpgesture_amd.vqvae import VQVAE
        model = VQVAE(None, 135, device=dev).load_state_dict(synth.make_vqvae_state_dict(7))

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def events_ms(fn, iters):
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return round(statistics.median(ts), 5)

    rows = []
    for S in a.takes:
        sc, sp = codes_all[:S], phases_all[:S]
        gS = knn.capture_clip_graph(M, audio=te_i, context=te_c, n_takes=S) if S > 1 else g1
        seedS = (sc, sp) if S > 1 else (int(sc[0]), sp[0])
        for _ in range(a.warmup):
            gS.run_ints(*seedS)
        t_takes, t_one, t_S_ones = [], [], []
        rounds = max(8, a.steps // max(1, S // 8))            # (S one-take replays per round: fewer rounds for large S)
        for _ in range(rounds):
            t_takes.append(clock(lambda: gS.run_ints(*seedS)))
            per = [clock(lambda s=s: g1.run_ints(int(sc[s]), sp[s])) for s in range(S)]
            t_one.extend(per)
            t_S_ones.append(sum(per))
        # the low-level route: one sweep + S walks
        def sweep_walks():
            T = knn.sweep_tables(te_i, te_c, M, for_walk=True)
            for s in range(S):
                knn.walk(T, M, seed_code=int(sc[s]), seed_phase=sp[s], sync="ints")
        for _ in range(2):
            sweep_walks()
        t_sw = [clock(sweep_walks) for _ in range(max(4, rounds // 4))]
        # the walk alone, eager, by events: all takes / one take (same tables: fusion prefused, gate table, then the takes)
        T = knn.sweep_tables(te_i, te_c, M, for_walk=True)
        sc_d = (sc, sp)
        walk_S = events_ms(lambda: knn.walk_takes(T, M, sc_d[0], sc_d[1], sync=False), 50)
        walk_1 = events_ms(lambda: knn.walk_takes(T, M, sc_d[0][:1], sc_d[1][:1], sync=False), 50)
        stage_ms = {}
        try:
            for name, mask in (("gate_table", 0), ("step0", 1), ("chase", 2), ("epilogue", 4)):
                _lib.set_option(dev, _lib.QPG_OPT_TAKES_STAGES, mask)
                stage_ms[name] = events_ms(lambda: knn.walk_takes(T, M, sc_d[0], sc_d[1], sync=False), 50)
        finally:
            _lib.set_option(dev, _lib.QPG_OPT_TAKES_STAGES, 7)
        gate_ms = stage_ms.pop("gate_table")
        stage_ms = {k + "_ms": round(v - gate_ms, 5) for k, v in stage_ms.items()}
        res = gS.run_takes(sc, sp) if S > 1 else None
        want = knn.match_clip_takes(te_i, te_c, M, seed_codes=sc, seed_phases=sp)
        if res is not None:
            assert np.array_equal(res.codes, want.codes) and np.array_equal(res.votes, want.votes)
        row = dict(n_takes=S, replay_takes_ms=med_ms(t_takes), replay_one_ms=med_ms(t_one),
                   replay_one_x_S_ms=med_ms(t_S_ones), extra_over_one_ms=round(med_ms(t_takes) - med_ms(t_one), 5),
                   sweep_plus_walks_ms=med_ms(t_sw), walk_takes_events_ms=walk_S, walk_one_take_events_ms=walk_1,
                   gate_table_ms=gate_ms, **stage_ms, n_distinct=int(want.n_distinct), rounds=rounds)
        if model is not None:
            ids = torch.from_numpy(want.codes.reshape(S, -1)).to(dev)
            for _ in range(3):
                model.decode([ids])
                model.decode([ids[:1]])
            torch.cuda.synchronize(dev)

            def batched():
                model.decode([ids])
                torch.cuda.synchronize(dev)

            def singles():
                for s in range(S):
                    model.decode([ids[s:s + 1]])
                torch.cuda.synchronize(dev)
            n_it = max(3, 40 // max(1, S // 8))
            row["decode_batched_ms"] = med_ms([clock(batched) for _ in range(n_it)])
            row["decode_singles_ms"] = med_ms([clock(singles) for _ in range(n_it)])
        rows.append(row)
        del gS
    out = dict(tool="bench_takes", n_db=N, windows=M, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(dev), takes=rows)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
