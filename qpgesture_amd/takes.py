"""Several TAKES of one clip: the clip matched from many seeds at once.

A matched clip depends on the draw of init_code_phase() (GestureKNN.py:462-473) and on nothing else that is random; the
sweeps, the per-code minima, their ranks, the fused candidate tables and the phase-gate table of every step but the first
are functions of the clip and the database alone.  So S takes cost one sweep, one select chain, one rank fusion and one gate
table, plus S evaluations of step 0 and S chases side by side (qpg_match_steps_takes).  Take s is what the s-th of S
successive CodeKNN.match_clip calls on the clip returns.

The walk is a deterministic map on at most 2K states per step: two takes that reach the same state stay together, so S
seeds give FEWER than S different gestures.  first_shared_code / n_distinct say how many, and from where on takes agree.

CodeKNN.walk_takes / CodeKNN.match_clip_takes are thin methods over the functions of this module."""
from typing import NamedTuple

import numpy as np

from .constant import num_frames_code


def first_shared_code(codes):
    """codes: int [S, ...] (take s's sequence is codes[s] flattened, L = M x 30 codes).  For every take s the smallest
    index k such that some EARLIER take equals take s from k to the end (L if none does): 0 marks a duplicate of an earlier
    take, a small k a take that joined an earlier one early.  Pure NumPy."""
    c = np.asarray(codes)
    S = c.shape[0]
    c = c.reshape(S, -1)
    L = c.shape[1]
    out = np.full((S,), L, np.int64)
    for s in range(1, S if L else 0):
        eq = c[:s, ::-1] == c[s, ::-1]                          # from the end backwards
        run = np.where(eq.all(axis=1), L, np.argmin(eq, axis=1))   # length of the common suffix with each earlier take
        out[s] = L - int(run.max())
    return out


def n_distinct(codes):
    """Number of different code sequences among the takes."""
    c = np.asarray(codes)
    if c.size == 0:                 # (no takes, or takes of an empty clip: all the same empty sequence)
        return min(c.shape[0], 1)
    return int(np.unique(c.reshape(c.shape[0], -1), axis=0).shape[0])


class TakesResult(NamedTuple):
    codes: np.ndarray               # int64 [S, M, 30]
    phases: np.ndarray              # f32 [S, M, steps, 8, 16]
    votes: np.ndarray               # i32 [S, M, steps]
    seed_codes: np.ndarray          # int64 [S]
    first_shared_code: np.ndarray   # int64 [S]: first_shared_code(codes)
    n_distinct: int


def make_result(codes, phases, votes, seed_codes):
    return TakesResult(codes, phases, votes, np.asarray(seed_codes, np.int64).reshape(-1), first_shared_code(codes),
                       n_distinct(codes))


def check_seeds(seed_codes, seed_phases, K):
    """(int64 [S], f32 [S][8][16]) or ValueError."""
    import torch
    sc = np.asarray(seed_codes)
    if sc.ndim != 1 or sc.size < 1 or not np.issubdtype(sc.dtype, np.integer):
        raise ValueError("takes: seed_codes must be a non-empty 1-d sequence of integers")
    sc = sc.astype(np.int64)
    if (sc < 0).any() or (sc >= K).any():
        raise ValueError("takes: every seed code must lie in [0, %d)" % K)
    if isinstance(seed_phases, torch.Tensor):
        seed_phases = seed_phases.detach().cpu().numpy()
    sp = np.asarray(seed_phases, np.float32)
    if sp.size != sc.size * 128:
        raise ValueError("takes: seed_phases must hold [n_takes][8][16] floats (got %d for %d takes)" % (sp.size, sc.size))
    return sc, np.ascontiguousarray(sp.reshape(sc.size, 8, 16))


def check_statuses(status):
    """status: int [S][2] on the host.  The trouble word is the clip's (every take carries the same copy); an absent code
    that won a fusion is a take's own."""
    from .code_knn import GuardOverflow
    st = np.asarray(status).reshape(-1, 2)
    if (st[:, 1] != 0).any():
        raise GuardOverflow(int(st[:, 1].max()))
    bad = np.nonzero(st[:, 0])[0]
    if bad.size:
        raise IndexError("take %d: a code that never occurs in the database won a rank fusion "
                         "(the reference raises IndexError at GestureKNN.py:631-632)" % int(bad[0]))


def draw_seeds(knn, n_takes):
    """n_takes successive init_code_phase() draws from the matcher's rng: what n_takes match_clip calls would draw."""
    if n_takes is None or int(n_takes) < 1:
        raise ValueError("takes: n_takes >= 1 or explicit seeds wanted")
    draws = [knn.init_code_phase() for _ in range(int(n_takes))]
    return np.array([d[0] for d in draws], np.int64), np.stack([d[1] for d in draws]).astype(np.float32)


def walk_takes(knn, T, n_windows, seed_codes, seed_phases, mode, window_offset=0, sync=True, seed_ptrs=None,
               out_pin=None, n_takes=None):
    """CodeKNN.walk_takes (its docstring has the interface)."""
    import torch
    from . import _lib
    from .code_knn import plan_takes
    db, dev = knn.db, knn.db.device
    M, steps = int(n_windows), knn.n_steps()
    if seed_ptrs is None:
        sc, sp = check_seeds(seed_codes, seed_phases, db.K)
        S = sc.size
    else:
        S = int(n_takes)
    plan = plan_takes(knn._knobs(), knn._facts(), M, steps, S, serial_walk=knn.serial_walk)
    if plan.path == "unsupported":
        raise NotImplementedError("walk_takes: " + plan.reason)
    n_c, n_v = M * num_frames_code, M * steps
    if M == 0:
        out = (np.zeros((S, 0, num_frames_code), np.int64), np.zeros((S, 0, steps, 8, 16), np.float32),
               np.zeros((S, 0, steps), np.int32))
        return out if sync else tuple(torch.from_numpy(a).to(dev) for a in out) + (torch.zeros((S, 2), dtype=torch.int32,
                                                                                              device=dev),)
    if plan.path == "kernel":
        if seed_ptrs is None:
            sc_d = torch.as_tensor(sc.astype(np.int32), device=dev)
            sp_d = torch.as_tensor(sp, device=dev).contiguous()
        else:
            sc_d, sp_d = int(seed_ptrs[0]), int(seed_ptrs[1])
        out_phase = torch.empty((S, M, steps, 8, 16), dtype=torch.float32, device=dev)
        if out_pin is not None:             # codes [S][M*30] | votes [S][M*steps] | status [S][2] in pinned host memory
            assert out_pin.numel() >= S * (n_c + n_v + 2)
            base = out_pin.data_ptr()
            oc, ov, st = base, base + 4 * S * n_c, base + 4 * S * (n_c + n_v)
        else:
            ints_d = torch.empty((S * (n_c + n_v + 2),), dtype=torch.int32, device=dev)
            oc = ints_d[:S * n_c].view(S, M, num_frames_code)
            ov = ints_d[S * n_c:S * (n_c + n_v)].view(S, M, steps)
            st = ints_d[S * (n_c + n_v):].view(S, 2)
        q0, Q = int(window_offset) * steps, M * steps
        head, gate, mode_w = knn._walk_args(T, q0, Q, Q, mode, q0 == 0)
        nb = int(_lib.load().qpg_match_steps_takes_ws_bytes(S, M, steps))
        ws = knn._takes_ws = _grown_ws(knn._takes_ws, nb, dev)
        try:
            _lib.call("qpg_match_steps_takes", dev, *head, mode_w, M, steps, db.K, S, sc_d, sp_d, gate, oc, out_phase, ov,
                      st, 2, knn._guard_stats[1:2], ws, ws.numel())
        except _lib.Unsupported:
            # (the library refuses a geometry the plan let through: nothing was launched; the takes one at a time)
            if seed_ptrs is not None:
                raise
            plan = plan._replace(path="per_take")
        else:
            knn._last_gate_tables = gate
            if out_pin is not None or not sync:
                if out_pin is None:
                    knn._last_ints = ints_d
                return oc, out_phase, ov, st
            phases = out_phase.cpu().numpy()
            ints = ints_d.cpu().numpy()
            check_statuses(ints[S * (n_c + n_v):])
            return (ints[:S * n_c].reshape(S, M, num_frames_code).astype(np.int64), phases,
                    ints[S * n_c:S * (n_c + n_v)].reshape(S, M, steps).copy())
    # per take: S walks of the same tables (the one-wave sequential walk, or a geometry the tabulation refuses)
    if seed_ptrs is not None:
        raise NotImplementedError("walk_takes: the captured form needs the tabulated walk (" + plan.reason + ")")
    if sync:
        res = []
        for s in range(S):
            try:
                res.append(knn.walk(T, M, window_offset, mode, int(sc[s]), sp[s]))
            except IndexError as e:
                raise IndexError("take %d: %s" % (s, e)) from None
        return tuple(np.stack([r[i] for r in res]) for i in range(3))
    res = [knn.walk(T, M, window_offset, mode, int(sc[s]), sp[s], sync=False) for s in range(S)]
    return tuple(torch.stack([r[i] for r in res]) for i in range(4))


def _grown_ws(buf, nbytes, dev):
    import torch
    if buf is not None and buf.numel() >= nbytes:
        return buf
    return torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)


def match_clip_takes(knn, test_interp, test_context, n_windows, n_takes=None, seed_codes=None, seed_phases=None,
                     mode=None):
    """CodeKNN.match_clip_takes (its docstring has the interface).  Written against the matcher's public methods
    (init_code_phase, sweep_tables, walk_takes, clear_flags) and switches only."""
    from .code_knn import FLAG_TEXT_OVERFLOW, GuardOverflow, MODE_AUD_TXT
    mode = MODE_AUD_TXT if mode is None else mode
    if seed_codes is None:                      # drawn ONCE, all of them in front of the sweep: a re-match walks the same takes
        seed_codes, seed_phases = draw_seeds(knn, n_takes)
    elif n_takes is not None and int(n_takes) != len(seed_codes):
        raise ValueError("takes: n_takes = %d but %d seed codes given" % (int(n_takes), len(seed_codes)))
    seed_codes, seed_phases = check_seeds(seed_codes, seed_phases, knn.db.K)

    def run(for_walk):
        T = knn.sweep_tables(test_interp, test_context, n_windows, mode, for_walk=for_walk)
        return knn.walk_takes(T, n_windows, seed_codes, seed_phases, mode=mode)

    def run_exact():
        prev = knn.audio_precision
        knn.clear_flags()
        knn.audio_precision = "exact"
        knn.fallbacks += 1
        try:
            return run(False)
        finally:
            knn.audio_precision = prev

    if n_windows == 0:                          # an empty clip (the reference's loop body never runs, :785)
        S, steps = seed_codes.size, knn.n_steps()
        return make_result(np.zeros((S, 0, num_frames_code), np.int64), np.zeros((S, 0, steps, 8, 16), np.float32),
                           np.zeros((S, 0, steps), np.int32), seed_codes)
    test_interp = test_interp.contiguous()
    try:
        out = run(True)
    except GuardOverflow as e:
        # the TABLES are made again, once, by the routes of CodeKNN.match_clip / rematch; all takes walk them
        if knn.audio_precision == "exact":
            knn.clear_flags()
            raise RuntimeError("the uncapped path raised flags 0x%x: this is a bug" % e.flags)
        if e.flags == FLAG_TEXT_OVERFLOW and knn.text_kernel == "mfma":
            knn.clear_flags()
            knn.fallbacks += 1
            knn.text_fallbacks += 1
            knn.text_kernel = "valu"
            try:
                out = run(False)
            except GuardOverflow:               # the audio side of this clip is in trouble as well
                out = run_exact()
            finally:
                knn.text_kernel = "mfma"
        else:
            out = run_exact()
    return make_result(out[0], out[1], out[2], seed_codes)
