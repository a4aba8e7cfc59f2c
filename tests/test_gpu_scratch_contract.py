"""The scratch contract through the C ABI ("Scratch contract"; the audit: profiles/scratch_contract.md): the
documented outputs of an entry point are the same bits whatever its workspace, its scratch tables and its not-yet-written
output memory held before the call; it never writes past the size its *_ws_bytes function states, and refuses a workspace
one unit short before launching anything.

One table of rows, one test body.  Per (row, case):
  (a) the call under every fill of tests/poison.py FILLS - workspace of EXACTLY the stated size between fences, every
      output pre-filled with the same pattern between fences of its own - twice with zeros (the determinism baseline), and
      once on a STALE workspace: the one the row's larger companion case has just left, untouched.  All runs bit-equal;
      equal to the reference of the row's existing contract test (case tables and references are imported, not restated);
      every fence intact.
  (b) the same call with the workspace one unit short: an error, workspace and outputs still hold their prefill.
The workspace of qpg_percode_select_mixed_f64 / _cut is the documented exception ("ZERO-FILLED ONCE by the caller"): it is
only ever handed zeros here, and its test is the reuse half alone (test_mixed_select_leaves_its_workspace_reusable).

One SCRATCH line per (row, case) with the wall time (pytest -s)."""
import functools
import time

import numpy as np
import pytest

from tests import poison as P
from tests import select_ref as SR
from tests import text_ref as TR
from tests import walk_ref as WR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _torch():
    import torch
    return torch


class Outs:
    """A call's outputs: each pre-filled with the run's pattern, between fences of its own."""

    def __init__(self, pattern):
        self.pattern, self.items = pattern, {}

    def new(self, name, shape, dtype):
        t, g = P.fenced(shape, dtype, self.pattern, device=DEV)
        self.items[name] = (t, g)
        return t

    def collect(self, **views):
        """-> name -> NumPy copy (views: name -> function of the array, for the documented region of an output)."""
        _torch().cuda.synchronize()
        got = {}
        for name, (t, g) in self.items.items():
            g.assert_tail_intact(name)
            a = t.cpu().numpy()
            got[name] = views[name](a) if name in views else a
        return got

    def assert_untouched(self):
        _torch().cuda.synchronize()
        for name, (t, g) in self.items.items():
            g.assert_tail_intact(name)
            assert bool((g.buf == self.pattern).all()), "%s was written by a call that failed" % name


def _refused(o, fn):
    """fn() must fail with the library's error before anything is launched."""
    with pytest.raises(RuntimeError, match="too small|workspace|bad size"):
        fn()
    o.assert_untouched()


# ---- rows ----------------------------------------------------------------------------------------------------------------
class TextRow:
    """qpg_text_percode_f32 (both organisations: tiles_per_chunk 1 and 3) / _f16.  case = (name, tiles_per_chunk)."""
    unit = 1

    def __init__(self, half):
        self.half = half
        self.name = "text_percode_f16" if half else "text_percode_f32"
        names = list(TR.HALF_CASES if half else TR.PERCODE_CASES)
        want = ["c65_q11_k7", "c513_q97_k512_d384"] if half else ["c65_q11_k7", "c513_q97_k7_d384", "c1000_q13_k1024"]
        assert set(want) <= set(names)
        big = want[-1]
        tpcs = (1,) if half else (1, 3)
        self.cases = [(n, t) for n in [big] + want[:-1] for t in tpcs]
        self.companion = {c: (big, c[1]) for c in self.cases}

    @functools.lru_cache(maxsize=None)
    def _operands(self, name):
        from tests import test_gpu_text_contract as TT
        torch = _torch()
        c = TR.percode_case(name, self.half)
        if not self.half:
            return c, (TT._pack_and_check_f32(c),), TT._normalised_queries(c), TT._to(c.code)
        image, live, nrm, _ = c.packed
        xh = torch.zeros((image.size,), dtype=torch.int16, device=DEV)
        dn = torch.zeros((c.C,), dtype=torch.float32, device=DEV)
        TT._call("qpg_text_pack_candidates_f16", TT._to(c.ctx), c.N, c.R, c.Dm, TT._to(c.cand_r), c.G, xh, dn)
        return c, (xh, dn), TT._normalised_queries(c), TT._to(c.code)

    def need(self, case):
        from qpgesture_amd import _lib
        c = TR.percode_case(case[0], self.half)
        return int(_lib.load().qpg_text_percode_ws_bytes(c.C, c.Q, c.K, case[1]))

    def run(self, case, ws, stated, pat, refuse=False):
        from tests import test_gpu_text_contract as TT
        torch = _torch()
        c, img, qn, code = self._operands(case[0])
        o = Outs(pat)
        od, oi = o.new("dist", (c.Q, c.K), torch.float32), o.new("idx", (c.Q, c.K), torch.int32)
        orank, onn = o.new("rank", (c.Q, c.K), torch.int16), o.new("nn", (c.Q,), torch.int32)
        tail = (5000, float(TR.ABSENT), ws, stated, od, oi, orank, onn)
        if self.half:
            fn = lambda: TT._call("qpg_text_percode_f16", img[0], img[1], c.C, c.Dm, code, c.K, qn, c.Q, *tail)      # noqa: E731
        else:
            fn = lambda: TT._call("qpg_text_percode_f32", img[0], c.C, c.Dm, code, c.K, qn, c.Q, case[1], *tail)    # noqa: E731
        if refuse:
            return _refused(o, fn)
        fn()
        return o.collect()

    def check(self, case, got):
        c = TR.percode_case(case[0], self.half)
        dist, idx, rank, nn = c.tables(5000)
        assert np.array_equal(got["dist"].view(np.uint32), dist.view(np.uint32)) and np.array_equal(got["idx"], idx)
        assert np.array_equal(got["rank"], rank) and np.array_equal(got["nn"], nn)


class ExactRow:
    """qpg_percode_select_exact_f64 on the exact distances of the audio cases `base` and `odd`."""
    name, unit = "select_exact", 1
    cases = ["base", "odd"]
    companion = {"base": "base", "odd": "base"}

    def need(self, case):
        from qpgesture_amd import _lib
        c = SR.audio_case(case)
        return int(_lib.load().qpg_percode_select_exact_ws_bytes(c.Q, c.C, c.K))

    def run(self, case, ws, stated, pat, refuse=False):
        from tests import test_gpu_select_contract as TS
        torch = _torch()
        c = SR.audio_case(case)
        D = torch.from_numpy(c.exact).to(DEV)
        o = Outs(pat)
        out = (o.new("dist", (c.Q, c.K), torch.float64), o.new("idx", (c.Q, c.K), torch.int32))
        rank = o.new("rank", (c.Q, c.K), torch.int16)
        res = {}

        def fn():
            res["stats"] = TS._f64_select(case, "exact", D, out=out, rank_out=rank, ws=ws, ws_bytes=stated)[3]
        if refuse:
            return _refused(o, fn)
        fn()
        return dict(o.collect(), stats=res["stats"])

    def check(self, case, got):
        c = SR.audio_case(case)
        rd, ri, rr = c.ref
        present = ri >= 0
        assert np.array_equal(got["idx"], ri) and np.array_equal(got["rank"].astype(np.int64), rr)
        assert np.abs(got["dist"] - rd)[present].max() <= 1e-13                  # (the existing contract test's bar)
        assert np.array_equal(got["dist"][~present], np.full((~present).sum(), SR.ABSENT))
        assert got["stats"][1] == 0 and got["stats"][0] > 0


class MergeRow:
    """qpg_merge_mixed_phase1_f64 -> qpg_shard_refine_f64 -> qpg_merge_mixed_phase2_f64 on case `base`, W = 3 and 2 row
    shards, through tests/helpers.merge_mixed_by_hand: the workspace is filled before phase 1 only; phase 2 reads what
    phase 1 left."""
    name, unit = "merge_mixed", 1
    cases = [3, 2]
    companion = {3: 3, 2: 3}

    @functools.lru_cache(maxsize=None)
    def _inputs(self, W):
        """The W shards' tables in the all-gather layout, each from the mixed select on its own adversarial matrix - the
        set-up of test_cross_shard_merge_returns_the_exact_tables."""
        from tests import test_gpu_select_contract as TS
        torch = _torch()
        c = SR.audio_case("base")
        Q, K, G = c.Q, c.K, SR.G_AUD
        bounds = [round(w * c.N / W) for w in range(W + 1)]
        src_stride = Q * K * 12
        recv = torch.zeros((W * src_stride,), dtype=torch.uint8, device=DEV)
        shards = []
        for w in range(W):
            lo, hi = bounds[w], bounds[w + 1]
            code = c.cand_code[lo * G:hi * G]
            D_in = SR.noisy("swap", np.ascontiguousarray(c.exact[:, lo * G:hi * G]), code, K, c.E, np.float32, seed=100 + w)
            blk = recv[w * src_stride:(w + 1) * src_stride]
            out = (blk[:Q * K * 8].view(torch.float64).view(Q, K), blk[Q * K * 8:].view(torch.int32).view(Q, K))
            TS._mixed("base", D_in, c.eps1, c.eps2, True, lo=lo, hi=hi, idx_base=lo * G, out=out, ranks=False)
            op = TS._operands("base", lo, hi)
            shards.append(dict(cand_base=lo * G, base=op["base"], base_is_f16=op["half"], T=SR.T_AUD, F=c.F, cand_t=op["cand_t"],
                               G=G, tap_stride=SR.TAP_STRIDE, q32=op["q32"], qn2=op["qn2"], cn2=op["cn2"]))
        return recv, src_stride, shards

    def need(self, W):
        from qpgesture_amd import _lib
        c = SR.audio_case("base")
        return int(_lib.load().qpg_merge_mixed_ws_bytes(c.Q, c.K, c.K * W))

    def run(self, W, ws, stated, pat, refuse=False):
        from tests.helpers import merge_mixed_by_hand
        torch = _torch()
        c = SR.audio_case("base")
        recv, src_stride, shards = self._inputs(W)
        o = Outs(pat)
        out = (o.new("dist", (c.Q, c.K), torch.float64), o.new("idx", (c.Q, c.K), torch.int32),
               o.new("rank", (c.Q, c.K), torch.int16))
        res = {}

        def fn():
            res["r"] = merge_mixed_by_hand(recv, W, src_stride, 0, c.Q * c.K * 8, c.Q, c.K, c.eps1, 0.0, shards, R=c.Q * c.K,
                                           fl_cap=c.K * W, ws=ws, ws_bytes=stated, out=out)
        if refuse:
            return _refused(o, fn)
        fn()
        return dict(o.collect(), stats=res["r"][3], counts=np.array(res["r"][4]))

    def check(self, W, got):
        c = SR.audio_case("base")
        rd, ri, rr = c.ref
        assert got["stats"][1] == 0 and got["counts"].min() > 0 and got["stats"][3] == got["counts"].sum()
        assert np.array_equal(got["idx"], ri) and np.array_equal(got["rank"].astype(np.int64), rr)
        assert np.abs(got["dist"] - rd)[ri >= 0].max() <= c.E


class TakesRow:
    """qpg_match_steps_takes: walk case k64_s8 with 65 takes, then `main` with 64.  The gate_tables argument is scratch too
    (include/qpg.h: "gate_tables: [dev] i32 [3][Q][K] scratch") and is pre-filled like the workspace; regions [0], [1] and
    rows 1 .. Q - 1 of [2] are what the existing contract test holds to its reference, and are compared here.  Row 0 of [2]
    belongs to the seed's own step, which a takes call evaluates per take into the workspace: excluded, as scratch."""
    name, unit = "match_steps_takes", 1
    cases = [("k64_s8", 65), ("main", 64)]
    companion = {("k64_s8", 65): ("k64_s8", 65), ("main", 64): ("k64_s8", 65)}
    STRIDE = 3

    def need(self, case):
        from qpgesture_amd import _lib
        Pm = WR.case(case[0])
        return int(_lib.load().qpg_match_steps_takes_ws_bytes(case[1], Pm.M, Pm.steps))

    def run(self, case, ws, stated, pat, refuse=False):
        from tests import test_gpu_walk_contract as WT
        torch = _torch()
        D = WT._device(case[0])
        Pm, n = D.P, case[1]
        o = Outs(pat)
        outs = dict(gate=o.new("gate", (3, Pm.Q, Pm.K), torch.int32), codes=o.new("codes", (n, Pm.M, Pm.codes_per_window), torch.int32),
                    phase=o.new("phase", (n, Pm.M, Pm.steps, 8, 16), torch.float32), vote=o.new("vote", (n, Pm.M, Pm.steps), torch.int32))
        status = o.new("status", (n * self.STRIDE,), torch.int32)
        fn = lambda: WT._takes(D, 0, n, stride=self.STRIDE, ws=ws, ws_bytes=stated, o=outs, status=status)      # noqa: E731
        if refuse:
            return _refused(o, fn)
        fn()
        Q, K = Pm.Q, Pm.K
        got = o.collect(status=lambda a: a.reshape(n, self.STRIDE)[:, :2].copy(),       # "take t's status pair at out_status + t x status_stride"
                        phase=lambda a: a.view(np.uint32))
        gate = got.pop("gate")
        got["T0"], got["T1"] = gate[0], gate[1]
        got["G"] = np.ascontiguousarray(gate[2]).view(np.uint16).reshape(Q, 2 * K)[1:].copy()
        return got

    def check(self, case, got):
        Pm, n = WR.case(case[0]), case[1]
        sol = WR.solve(Pm, 0, Pm.seed_codes[:n], Pm.seed_phases[:n])
        assert np.array_equal(got["T0"], Pm.tables(0)[0]) and np.array_equal(got["T1"], Pm.tables(0)[1])
        assert np.array_equal(got["G"], sol["G"][1:])
        assert np.array_equal(got["codes"], sol["codes"]) and np.array_equal(got["vote"], sol["vote"])
        assert np.array_equal(got["phase"], sol["phase"].view(np.uint32))
        assert np.array_equal(got["status"][:, 0], sol["status0"]) and (got["status"][:, 1] == 0).all()


class NoPhaseRow:
    """qpg_match_steps_nophase on k64_s7, both sides with coins, desired_k = 1: three chains, then one.  The workspace's
    next / pick tables are documented (include/qpg.h) and compared as well."""
    name, unit = "match_steps_nophase", 2
    cases = [3, 1]
    companion = {3: 3, 1: 3}
    MODE, KPOS, STRIDE = 0, 1, 3

    def _seeds(self, n):
        Pm = WR.case("k64_s7")
        return [int(Pm.seed_codes[s]) for s in (0, 5, 300)][:n]

    def need(self, n):
        from qpgesture_amd import _lib
        Pm = WR.case("k64_s7")
        return int(_lib.load().qpg_match_steps_nophase_ws_bytes(n, Pm.M, Pm.steps, Pm.K))

    def run(self, n, ws, stated, pat, refuse=False):
        from tests import test_gpu_nophase as TN
        torch = _torch()
        D = TN._device("k64_s7")
        Pm = D.P
        cpw = min(4 * Pm.steps, 30)
        coins = TN._coin_kinds(Pm.Q, n, 11)[2]
        o = Outs(pat)
        outs = dict(codes=o.new("codes", (n, Pm.M, cpw), torch.int32), side=o.new("side", (n, Pm.M * Pm.steps), torch.int32),
                    cand=o.new("cand", (n, Pm.M * Pm.steps), torch.int32), status=o.new("status", (n, self.STRIDE), torch.int32))
        res = {}

        def fn():
            res["r"] = TN._call(D, self.MODE, self.KPOS, self._seeds(n), coins, 5, tables=True, stride=self.STRIDE,
                                ws=ws.view(torch.int16), ws_state=stated, outs=outs)
        if refuse:
            return _refused(o, fn)
        fn()
        got = o.collect(status=lambda a: a[:, :2].copy())
        got["next"], got["pick"] = res["r"]["next"], res["r"]["pick"]
        return got

    def check(self, n, got):
        from tests import nophase_ref as NR
        from tests import test_gpu_nophase as TN
        Pm = WR.case("k64_s7")
        tabs = NR.tables(Pm, self.MODE, self.KPOS)
        coins = TN._coin_kinds(Pm.Q, n, 11)[2]
        assert np.array_equal(got["next"], np.tile(tabs[0], (n, 1, 1))) and np.array_equal(got["pick"], np.tile(tabs[1], (n, 1, 1)))
        TN._check_walks(got, Pm, self.MODE, self.KPOS, self._seeds(n), coins, 5, tabs)



@functools.lru_cache(maxsize=None)
def _vq64():
    """The width-64 model of test_backward_vs_autograd_small_width and its state dict."""
    from qpgesture_amd import synth
    from qpgesture_amd.vqvae import VQVAE
    hps = dict(width=64, emb_width=64, l_bins=96)
    sd = synth.make_vqvae_state_dict(7, hps)
    m = VQVAE(dict(vel=1, acc=1, commit=0.02, l_mu=0.99, reg=0.3, **hps), input_dim=135, device=DEV).load_state_dict(sd)
    return m.eval(), sd, hps


def _vq_x(B, T):
    from tests.test_gpu_vqvae_train import _x
    return _x(B)[:, :T].contiguous()


class VqRow:
    """qpg_vq_encode_f32, then qpg_vq_decode_f32 of its ids, both on ONE workspace of qpg_vq_workspace_floats floats, at
    (B, T) = (3, 96) and (1, 8).  Reference: the oracle's functional forward (oracle/vqvae_oracle.py), as in
    test_backward_vs_autograd_small_width: ids equal, x_out within 1e-4."""
    name, unit = "vq_encode_decode", 4
    cases = [(3, 96), (1, 8)]
    companion = {(3, 96): (3, 96), (1, 8): (3, 96)}

    def need(self, case):
        import ctypes
        from qpgesture_amd import _lib
        m = _vq64()[0]
        return 4 * int(_lib.load().qpg_vq_workspace_floats(ctypes.byref(m._desc), case[0], case[1]))

    def run(self, case, ws, stated, pat, refuse=False):
        from qpgesture_amd import _lib
        torch = _torch()
        m = _vq64()[0]
        B, T = case
        L = T // m.hop
        x = _vq_x(B, T).to(DEV)
        wsf = ws.view(torch.float32)
        o = Outs(pat)
        ids, lat = o.new("ids", (B, L), torch.int64), o.new("latent", (B, L, m.emb), torch.float32)
        mar, out = o.new("margin", (B, L), torch.float32), o.new("x_out", (B, T, m.input_dim), torch.float32)
        status = torch.zeros((1,), dtype=torch.int32, device=DEV)
        enc = lambda: _lib.call("qpg_vq_encode_f32", m.device, m._desc, x, B, T, wsf, stated // 4, ids, lat, mar)      # noqa: E731
        if refuse:
            _refused(o, enc)
            ids.zero_()                                 # (valid ids for the decoder's own refusal)
            with pytest.raises(RuntimeError, match="too small"):
                _lib.call("qpg_vq_decode_f32", m.device, m._desc, ids, B, L, wsf, stated // 4, out, status)
            torch.cuda.synchronize()
            assert bool((o.items["x_out"][1].buf == pat).all())
            return None
        enc()
        _lib.call("qpg_vq_decode_f32", m.device, m._desc, ids, B, L, wsf, stated // 4, out, status)
        return dict(o.collect(), status=status.cpu().numpy())

    def check(self, case, got):
        import torch
        from oracle import vqvae_oracle as VO
        _, sd, hps = _vq64()
        sdt = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in sd.items()}
        xo_ref, _, _, _, ids_ref = VO.forward(sdt, _vq_x(*case), hps=hps, training=False, commit=0.02, reg=0.3)
        assert np.array_equal(got["ids"], ids_ref.numpy()) and got["status"][0] == 0
        assert np.abs(got["x_out"] - xo_ref.detach().numpy()).max() < 1e-4
        assert np.isfinite(got["latent"]).all() and (got["margin"] >= 0).all()


class ReduceRow:
    """qpg_vq_loss_f32 at (B, T) = (4, 3) (companion (6, 8)) and qpg_vq_latent_stats_f32 on the reduce workspace of
    qpg_vq_reduce_ws_bytes bytes: inputs and f64 references of test_gpu_vqtrain_kernels.py."""
    unit = 1
    W = (0.02, 0.3, 0.7, 1.3)

    def __init__(self, which):
        self.which, self.name = which, "vq_" + which
        self.cases = [(6, 8), (4, 3)] if which == "loss" else [(7680, 512)]
        self.companion = {c: self.cases[0] for c in self.cases}

    def need(self, case):
        from qpgesture_amd import _lib
        return int(_lib.load().qpg_vq_reduce_ws_bytes())

    @functools.lru_cache(maxsize=None)
    def _inputs(self, case):
        import torch
        if self.which == "loss":
            from tests.test_gpu_vqtrain_kernels import _loss_inputs
            return _loss_inputs(case[0], case[1], 135, case[0] + case[1])
        g = torch.Generator().manual_seed(5)
        z = torch.randn(*case, generator=g) * 0.2
        return z, z + 0.1 * torch.randn(*case, generator=g), torch.rand(case[0], generator=g) * 3

    def run(self, case, ws, stated, pat, refuse=False):
        from qpgesture_amd import _lib
        torch = _torch()
        o = Outs(pat)
        if self.which == "loss":
            x, xo = self._inputs(case)
            out = o.new("out6", (6,), torch.float32)
            commit = torch.tensor([0.37], device=DEV)
            fn = lambda: _lib.call("qpg_vq_loss_f32", DEV, xo.to(DEV), x.to(DEV), case[0], case[1], 135, commit, *self.W, ws,      # noqa: E731
                                   stated, out)
        else:
            z, zq, dmin = self._inputs(case)
            out = o.new("out3", (3,), torch.float32)
            fn = lambda: _lib.call("qpg_vq_latent_stats_f32", DEV, z.to(DEV), zq.to(DEV), dmin.to(DEV), case[0], case[1], ws,      # noqa: E731
                                   stated, out)
        if refuse:
            return _refused(o, fn)
        fn()
        return o.collect()

    def check(self, case, got):
        import torch
        from tests.test_gpu_vqtrain_kernels import U
        if self.which == "loss":
            from oracle import vqvae_oracle as VO
            x, xo = self._inputs(case)
            w_com, w_reg, w_vel, w_acc = self.W
            _, met = VO.losses(x.double(), xo.double(), torch.tensor(0.37, dtype=torch.float64), hps_commit=w_com, vel=w_vel,
                               acc=w_acc, reg=w_reg)
            g6 = got["out6"].astype(np.float64)
            for i, kk in ((1, "recons_loss"), (2, "regularization"), (3, "velocity_loss"), (4, "acceleration_loss")):
                assert abs(g6[i] - float(met[kk])) <= 2 * U * abs(float(met[kk])) + 1e-30, kk      # (the existing test's bound)
            assert got["out6"][5] == np.float32(0.37)
        else:
            z, zq, dmin = self._inputs(case)
            n = z.numel()
            commit = float(((zq.double() - z.double()) ** 2).sum() / n)
            fit = float(dmin.double().mean())
            g3 = got["out3"].astype(np.float64)
            assert abs(g3[0] - commit) <= 4 * U * commit and abs(g3[1] - fit) <= 2 * U * fit


class CodeSumsRow:
    """qpg_vq_code_sums_f32 at the smallest CS_CASES entry (R = 1, E = 4) after (1025, 64): the documented summation order,
    bit for bit (oracle.vqtrain_oracle.code_sums_chunked_f32), exact counts."""
    name, unit, K = "vq_code_sums", 1, 512

    def __init__(self):
        from tests.test_gpu_vqtrain_kernels import CS_CASES
        small = min(CS_CASES, key=lambda c: (c[0] * c[1], c[0]))
        assert small == (1, 4, "uniform") and (1025, 64, "uniform") in CS_CASES
        self.cases = [(1025, 64, "uniform"), small]
        self.companion = {c: self.cases[0] for c in self.cases}

    def need(self, case):
        from qpgesture_amd import _lib
        return int(_lib.load().qpg_vq_code_sums_ws_bytes(case[0], case[1], self.K))

    @functools.lru_cache(maxsize=None)
    def _inputs(self, case):
        from tests.test_gpu_vqtrain_kernels import _ids
        R, E, pattern = case
        rng = np.random.Generator(np.random.PCG64(R * 7 + E))
        z = rng.standard_normal((R, E)).astype(np.float32)
        return z, _ids(pattern, R, self.K, rng)

    def run(self, case, ws, stated, pat, refuse=False):
        from qpgesture_amd import _lib
        torch = _torch()
        z, ids = self._inputs(case)
        o = Outs(pat)
        bsum, belem = o.new("batch_sum", (self.K, case[1]), torch.float32), o.new("batch_elem", (self.K,), torch.float32)
        zd, idd = torch.from_numpy(z).to(DEV), torch.from_numpy(ids.astype(np.int64)).to(DEV)
        fn = lambda: _lib.call("qpg_vq_code_sums_f32", DEV, zd, idd, case[0], case[1], self.K, bsum, belem, ws, stated)      # noqa: E731
        if refuse:
            return _refused(o, fn)
        fn()
        return o.collect()

    def check(self, case, got):
        from oracle import vqtrain_oracle as VT
        z, ids = self._inputs(case)
        assert np.array_equal(got["batch_elem"], np.bincount(ids, minlength=self.K).astype(np.float32))
        assert np.array_equal(got["batch_sum"].view(np.uint32), VT.code_sums_chunked_f32(z, ids, self.K).view(np.uint32))


class EmaRow:
    """qpg_vq_ema_update_f32 at (K, E, ldkT) = (96, 64, 128): ws of K doubles; inputs, f64 reference and bounds of
    test_ema_update_vs_f64."""
    name, unit = "vq_ema_update", 1
    cases = [(96, 64, 128)]
    companion = {(96, 64, 128): (96, 64, 128)}
    MU, THR = float(np.float32(0.99)), 1.0

    def need(self, case):
        return 8 * case[0]                              # include/qpg.h: "ws: >= K doubles"

    @functools.lru_cache(maxsize=None)
    def _inputs(self, case):
        from tests.test_gpu_vqtrain_kernels import _ema_inputs
        return _ema_inputs(case[0], case[1], np.random.Generator(np.random.PCG64(case[0] + case[1])))

    def run(self, case, ws, stated, pat, refuse=False):
        from qpgesture_amd import _lib
        torch = _torch()
        K, E, ldkT = case
        z, ids, k, k_sum, k_elem, k_rand, bsum, belem = self._inputs(case)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
        kd, ksd, ked = d(k), d(k_sum), d(k_elem)                                # in / out: the state, not scratch
        o = Outs(pat)
        kT, kk, out4 = o.new("kT", (E, ldkT), torch.float32), o.new("kk", (K,), torch.float32), o.new("out4", (4,), torch.float32)
        fn = lambda: _lib.call("qpg_vq_ema_update_f32", DEV, kd, ksd, ked, d(bsum), d(belem), d(k_rand), self.MU, self.THR, K,      # noqa: E731
                               E, kT, ldkT, kk, ws, stated, out4)
        if refuse:
            _refused(o, fn)
            assert np.array_equal(kd.cpu().numpy(), k) and np.array_equal(ksd.cpu().numpy(), k_sum)
            return None
        fn()
        got = o.collect(kT=lambda a: a[:, :K].copy())       # (columns K .. ldkT - 1 are not the transposed copy's: untouched)
        return dict(got, k=kd.cpu().numpy(), k_sum=ksd.cpu().numpy(), k_elem=ked.cpu().numpy())

    def check(self, case, got):
        from tests.test_gpu_vqtrain_kernels import _ema_compare, _ema_ref
        z, ids, k, k_sum, k_elem, k_rand, bsum, belem = self._inputs(case)
        ref = _ema_ref(z, ids, k, k_sum, k_elem, k_rand, self.MU, self.THR)
        _ema_compare((got["k"], got["k_sum"], got["k_elem"], got["kk"], got["out4"]), ref, (k_sum, k_elem, bsum, belem),
                     self.MU, self.THR)
        assert np.array_equal(got["kT"], got["k"].T)


class ConvRow:
    """qpg_conv1d_f32's split-K scratch on the smallest tests/conv_ref.py case that splits ("M=1 T_in=1 k3 d3": one row, 96
    K slices) after "M=65 k3 d3 relu res".  The workspace is OPTIONAL and its size only sets the split count (include/qpg.h:
    "the contraction is split over up to 8 block groups"), so there is no short-workspace refusal to test: `unit` is None.
    (qpg_convt_f32 takes no workspace at all.)"""
    name, unit = "conv1d_split_k", None
    cases = ["M=65 k3 d3 relu res", "M=1 T_in=1 k3 d3"]
    companion = {c: "M=65 k3 d3 relu res" for c in cases}

    @functools.lru_cache(maxsize=None)
    def _case(self, name):
        from tests import conv_ref as CR
        n_cu = _torch().cuda.get_device_properties(0).multi_processor_count
        c = {x["name"]: x for x in CR.cases(n_cu) if x["kernel"] == "conv1d"}[name]
        assert CR.conv1d_variant(c, n_cu)[3] > 1, "%s does not take the split path" % name
        return c, n_cu, CR.make_inputs(c)

    def need(self, case):
        from tests import conv_ref as CR
        return 4 * CR.ws_floats_of(self._case(case)[0])

    def run(self, case, ws, stated, pat, refuse=False):
        from qpgesture_amd import _lib
        from qpgesture_amd.vqvae import _Conv
        torch = _torch()
        c, n_cu, (x, w, bias, res) = self._case(case)
        conv = _Conv(w, bias, torch.device(DEV))
        o = Outs(pat)
        y = o.new("y", (c["B"], c["T_y"], c["Cout"]), torch.float32)
        rd = res.to(DEV) if res is not None else None
        _lib.call("qpg_conv1d_f32", DEV, x.to(DEV).contiguous(), c["B"], c["T_in"], c["Cin"], conv.w, conv.b, c["taps"], c["Cin_pad"],
                  c["Cout"], c["Cout_pad"], c["s"], c["off"], c["dil"], c["T_out"], c["out_stride"], c["out_offset"], c["T_y"], rd,
                  c["relu_in"], c["relu_out"], y, ws.view(torch.float32), stated // 4)
        return o.collect()

    def check(self, case, got):
        from tests import conv_ref as CR
        import torch
        c, n_cu, (x, w, bias, res) = self._case(case)
        assert c["out_stride"] == 1 and c["T_y"] == c["T_out"]
        ref, absref = CR.conv_ref(x, w, bias, CR.geom_of(c), c["relu_in"], c["relu_out"], res)
        r = CR.bound_ratio(torch.from_numpy(got["y"]), ref, absref, CR.gamma(*CR.chains_of(c, n_cu)))
        assert r <= 1.0, "%s: err / bound = %.3g" % (case, r)


class ConvBackwardRow:
    """qpg_conv1d_bwd_weight_f32 (partial-sum workspace for 4 splits) of the width-64 model's dec_in layer (k3 s1 p1,
    64 -> 64), or qpg_conv1d_bwd_data_f32 (split-K scratch) of its dec_out layer (k3 s1 p1, 64 -> 135: dy has 135
    channels, 27 K slices - the narrowest layer of that model whose backward-data splits; dec_in's 12 slices do not), at
    (B, T) = (1, 30) after (3, 96); f64 reference and bound of oracle/vqtrain_oracle.py (layer_grads, gamma), as in
    test_gpu_vqtrain_kernels.py.  bwd_weight refuses a workspace smaller than ONE partial (more only buys parallelism);
    bwd_data's scratch is optional like qpg_conv1d_f32's.  That the split ran is read from the workspace under the 0xFF
    fill: slab z's last entry is no longer NaN."""
    cases = [(3, 96), (1, 30)]
    companion = {c: (3, 96) for c in cases}
    SPLITS = 4

    def __init__(self, which):
        self.which, self.name = which, "conv1d_bwd_" + which
        self.unit = 4 if which == "weight" else None

    def _layer(self):
        m, sd, _ = _vq64()
        name, c = (("module.decoders.0.level_blocks.0.model.0", m.dec_in) if self.which == "weight"
                   else ("module.decoders.0.out", m.dec_out))
        return m, c, sd[name + ".weight"], sd[name + ".bias"]

    def _floats(self, splits):
        from qpgesture_amd import _lib
        c = self._layer()[1]
        return int(_lib.load().qpg_conv1d_wgrad_ws_floats(c.taps, c.cin_pad, c.cout_pad, splits))

    def need(self, case):
        if self.which == "weight":
            return 4 * self._floats(self.SPLITS)
        c = self._layer()[1]
        return 4 * (8 * case[0] * case[1] * ((c.cin_pad + 127) // 128 * 128) + 64)      # room for 8 slabs [M][Cout_pad]

    def short_stated(self, case):
        return 4 * (self._floats(1) - 1)

    @functools.lru_cache(maxsize=None)
    def _inputs(self, case):
        import torch
        c = self._layer()[1]
        g = torch.Generator().manual_seed(31 + case[1])
        return torch.randn(case[0], case[1], c.cin, generator=g), torch.randn(case[0], case[1], c.cout, generator=g)

    def run(self, case, ws, stated, pat, refuse=False):
        from qpgesture_amd import _lib
        torch = _torch()
        m, c, _, _ = self._layer()
        B, T = case
        x, dy = self._inputs(case)
        xd, dyd = x.to(DEV), dy.to(DEV)
        wsf = ws.view(torch.float32)[:stated // 4] if refuse else ws.view(torch.float32)
        o = Outs(pat)
        if self.which == "weight":
            dw, db = o.new("dw", (c.taps, c.cin_pad, c.cout_pad), torch.float32), o.new("db", (c.cout_pad,), torch.float32)
            fn = lambda: _lib.call("qpg_conv1d_bwd_weight_f32", DEV, xd, B, T, c.cin, dyd, c.taps, c.cin_pad, c.cout, c.cout_pad,      # noqa: E731
                                   1, -1, 1, T, 1, 0, T, 0, dw, db, 0, wsf, stated // 4)
        else:
            dx = o.new("dx", (B, T, c.cin), torch.float32)
            fn = lambda: _lib.call("qpg_conv1d_bwd_data_f32", DEV, dyd, B, T, c.cout, c.w, 3, c.cin, c.cin_pad, c.cout_pad, 2, -1,      # noqa: E731
                                   1, -1, 1, T, 1, 0, T, None, None, dx, wsf, stated // 4)
        if refuse:
            return _refused(o, fn)
        fn()
        got = o.collect()                                   # (dw: "packed like the weights, fully overwritten" - padding included)
        if self.which == "data" and pat == 0xFF:            # conv_launch's rule gives 3 splits here (27 slices / 8): at least 2 ran
            slab = B * T * ((c.cin_pad + 127) // 128 * 128)
            assert not bool(torch.isnan(wsf[slab - 1])) and not bool(torch.isnan(wsf[2 * slab - 1])), "backward-data did not split"
        return got

    def check(self, case, got):
        from oracle import vqtrain_oracle as VT
        _, c, w, b = self._layer()
        x, dy = self._inputs(case)
        ref, absref = VT.layer_grads("conv3", x, dy, [w], [b], 1)
        M = case[0] * case[1]
        if self.which == "weight":
            g = VT.gamma(M, self.SPLITS)
            dw = np.transpose(got["dw"][:, :c.cin, :c.cout], (2, 1, 0)).copy()   # [tap][ci][co] -> torch's (co, ci, tap)
            assert VT.bound_ratio(dw, ref["dw"][0], absref["dw"][0], g) <= 1.0
            assert VT.bound_ratio(got["db"][:c.cout].copy(), ref["db"][0], absref["db"][0], g) <= 1.0
        else:
            assert VT.bound_ratio(got["dx"], ref["dx"], absref["dx"], VT.gamma(3 * c.cout, 8)) <= 1.0


class PaePhaseRow:
    """qpg_pae_phase_f32 on tests/pae_ref.py's velocity-bits input (clips of 1, 5, 0, 130, 2, 300, 77 frames): the whole
    batch in one chunk, then its last frame alone.  The workspace AFTER the call is documented (include/qpg.h: "the f32
    velocities of the rows the chunk reads") and is held to pae_ref.workspace_image bit for bit, as in
    test_velocities_are_the_f64_difference_rounded_once; out / v / latent are compared across the fills."""
    name, unit = "pae_phase", 4

    def __init__(self):
        self.cases = ["all", "last"]
        self.companion = {c: "all" for c in self.cases}

    @functools.lru_cache(maxsize=None)
    def _inp(self):
        from tests import pae_ref as PR
        return PR.input_velocity_bits(17)

    def _chunk(self, case):
        n = int(self._inp()["off"][-1])
        return (0, n) if case == "all" else (n - 1, 1)

    def need(self, case):
        from qpgesture_amd import PAE
        return 4 * (self._chunk(case)[1] + 2 * PAE.HALO - 1) * PAE.WS_STRIDE

    def run(self, case, ws, stated, pat, refuse=False):
        from qpgesture_amd import _lib
        from tests import pae_ref as PR
        from tests import test_gpu_pae_contract as TP
        torch = _torch()
        f0, n = self._chunk(case)
        pose, mean, std, off = TP.dev_input(self._inp())
        Pd = TP.dev_block("seed11")
        o = Outs(pat)
        out, v = o.new("out", (n, 4, PR.E), torch.float32), o.new("v", (n, PR.E, 2), torch.float32)
        lat = o.new("latent", (n, PR.E, PR.T), torch.float32)
        wsf = ws.view(torch.float32)
        fn = lambda: _lib.call("qpg_pae_phase_f32", DEV, Pd, pose, mean, std, off, off.numel() - 1, pose.shape[0], f0, n, wsf,      # noqa: E731
                               stated // 4, out, v, lat)
        if refuse:
            return _refused(o, fn)
        fn()
        got = o.collect()
        got["ws"] = wsf[:stated // 4].cpu().numpy()
        return got

    def check(self, case, got):
        from qpgesture_amd import PAE
        from tests import pae_ref as PR
        f0, n = self._chunk(case)
        want = PR.workspace_image(PR.velocities(self._inp()), f0, n)
        assert np.array_equal(got["ws"].reshape(-1, PAE.WS_STRIDE).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))
        assert np.isfinite(got["latent"]).all()


class PaeTrainRow:
    """qpg_pae_train_forward_f32 + _backward_f32 at B = 2: the workspace is filled before the forward only, the backward
    reads the forward's activations.  The loss, every gradient byte and the running statistics are compared across the
    fills, and with what PAE_train.Trainer (held to the f64 restatement by test_step_matches_f64_restatement[2]) computes."""
    name, unit = "pae_train_fwd_bwd", 4
    cases = [4, 2]
    companion = {4: 4, 2: 4}

    @functools.lru_cache(maxsize=None)
    def _setup(self, B):
        from qpgesture_amd import PAE_train as PT
        from qpgesture_amd import synth
        from tests.test_gpu_pae_train import _data, _starts
        pn, all_starts = _data(n_clips=2, T=300)
        sd = synth.make_pae_state_dict(11)
        P, S, _ = PT.pack(sd)
        return sd, pn, _starts(all_starts, B, 3), P, S

    def need(self, B):
        import ctypes
        from qpgesture_amd import _lib
        n = ctypes.c_int64(0)
        _lib.call("qpg_pae_train_ws_floats", _torch().device(DEV), B, ctypes.addressof(n))
        return 4 * int(n.value)

    def run(self, B, ws, stated, pat, refuse=False):
        from qpgesture_amd import PAE_train as PT
        from qpgesture_amd import _lib
        torch = _torch()
        sd, pn, starts, P, S = self._setup(B)
        dev = torch.device(DEV)
        params, poses = torch.from_numpy(P).to(dev), torch.from_numpy(np.ascontiguousarray(pn, np.float32)).to(dev)
        st = torch.from_numpy(starts.astype(np.int64)).to(dev)
        stats = torch.from_numpy(S.copy()).to(dev)                              # in / out: the running statistics
        wsf = ws.view(torch.float32)
        o = Outs(pat)
        loss = o.new("loss", (1,), torch.float64)
        grads = o.new("grads", (PT.PARAM_FLOATS,), torch.float32)
        fwd = lambda: _lib.call("qpg_pae_train_forward_f32", dev, params, stats, poses, poses.shape[0], st, B, 1, wsf, stated // 4,      # noqa: E731
                                loss)
        if refuse:
            _refused(o, fwd)
            with pytest.raises(RuntimeError, match="workspace"):
                _lib.call("qpg_pae_train_backward_f32", dev, params, B, wsf, stated // 4, grads)
            o.assert_untouched()
            assert np.array_equal(stats.cpu().numpy(), S)
            return None
        fwd()
        _lib.call("qpg_pae_train_backward_f32", dev, params, B, wsf, stated // 4, grads)
        torch.cuda.synchronize()
        # include/qpg.h: "grads [dev] f32, the same layout (entries below QPG_PAET_TRAINABLE are left untouched)"
        assert bool((grads[:PT.TRAINABLE].view(torch.uint8) == pat).all()), "gradient entries below QPG_PAET_TRAINABLE were written"
        return dict(o.collect(grads=lambda a: a[PT.TRAINABLE:].copy()), stats=stats.cpu().numpy())

    def check(self, B, got):
        from qpgesture_amd import PAE_train as PT
        sd, pn, starts, P, S = self._setup(B)
        tr = PT.Trainer(sd, batch=B, device=DEV)
        tr.set_data(pn)
        loss = tr.forward(starts, train=True).cpu().numpy()
        tr.backward()
        assert np.array_equal(got["loss"].view(np.uint64), loss.view(np.uint64))
        assert np.array_equal(got["grads"].view(np.uint32), tr.grads[PT.TRAINABLE:].cpu().numpy().view(np.uint32))
        assert np.array_equal(got["stats"].view(np.uint32), tr.stats.cpu().numpy().view(np.uint32))
        assert np.isfinite(got["grads"]).all() and np.isfinite(got["loss"]).all()


ROWS = [TextRow(False), TextRow(True), ExactRow(), MergeRow(), TakesRow(), NoPhaseRow(), VqRow(), ReduceRow("loss"),
        ReduceRow("latent_stats"), CodeSumsRow(), EmaRow(), ConvRow(), ConvBackwardRow("weight"), ConvBackwardRow("data"),
        PaePhaseRow(), PaeTrainRow()]
PARAMS = [pytest.param(r, c, id="%s-%s" % (r.name, "_".join(str(x) for x in (c if isinstance(c, tuple) else (c,)))))
          for r in ROWS for c in r.cases]


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), \
            "%s: output %r differs (%d of %d bytes)" % (what, k, int((x.view(np.uint8) != y.view(np.uint8)).sum()), x.nbytes)


@pytest.mark.parametrize("row,case", PARAMS)
def test_results_do_not_depend_on_what_the_workspace_held(row, case):
    _drive(row, case)


class _ControlRow:
    """Not a library call: a torch "op" with a 64-byte workspace.  leaky: it returns what the workspace's first four floats
    held (made finite) - a read before any write; sound: it writes them first."""
    unit, cases, companion = 4, [0], {0: 0}

    def __init__(self, leaky):
        self.leaky, self.name = leaky, "control_leaky" if leaky else "control_sound"

    def need(self, case):
        return 64

    def run(self, case, ws, stated, pat, refuse=False):
        torch = _torch()
        o = Outs(pat)
        y = o.new("y", (4,), torch.float32)
        if refuse:
            def fn():
                raise RuntimeError("control: workspace too small")
            return _refused(o, fn)
        w = ws.view(torch.float32)[:4]
        if not self.leaky:
            w.fill_(2.0)
        y.copy_(torch.nan_to_num(w, nan=7.0).clamp(-9.0, 9.0) * 3.0)
        return o.collect()

    def check(self, case, got):
        pass


def test_control_the_driver_catches_a_read_before_write():
    """The driver itself: an op that reads its workspace before writing it fails under the fills; the same op with the
    write in front passes."""
    _drive(_ControlRow(False), 0)
    with pytest.raises(AssertionError, match="output 'y' differs"):
        _drive(_ControlRow(True), 0)


def _drive(row, case):
    t0 = time.perf_counter()
    need = row.need(case)
    assert need > (row.unit or 0)
    base = None
    for label, pat in [("zeros_00 (again)", 0x00)] + list(P.FILLS.items()):
        g = P.guarded(need, pat, device=DEV)
        got = row.run(case, g.buf, need, pat)
        g.assert_tail_intact("%s %s %s: workspace" % (row.name, case, label))
        if base is None:
            base = got
            row.check(case, got)                       # ... and what is bit-equal to it below meets the reference too
        else:
            _same(base, got, "%s %s under %s vs zeros" % (row.name, case, label))      # (zeros vs zeros: the determinism baseline)
    # stale: the workspace the larger companion case has just left, reused as it is
    comp = row.companion[case]
    need_c = row.need(comp)
    g = P.guarded(max(need, need_c), 0xEE, device=DEV)
    row.run(comp, g.buf[:need_c], need_c, 0xEE)
    got = row.run(case, g.buf[:need], need, 0xEE)
    g.assert_tail_intact("%s %s stale: workspace" % (row.name, case))
    _same(base, got, "%s %s on the workspace %s left" % (row.name, case, comp))
    # (b) one unit short: refused before anything is launched (unit None: the workspace is optional, nothing to refuse)
    if row.unit is not None:
        short = row.short_stated(case) if hasattr(row, "short_stated") else need - row.unit
        g = P.guarded(need, 0x3C, device=DEV)
        row.run(case, g.buf, short, 0x3C, refuse=True)
        g.assert_tail_intact("%s %s short: workspace" % (row.name, case))
        assert bool((g.buf == 0x3C).all()), "%s %s: a refused call wrote its workspace" % (row.name, case)
    print("SCRATCH %-22s %-28s ws %8d B, 6 runs + stale (after %s) + short: %.2f s"
          % (row.name, case, need, comp, time.perf_counter() - t0))


# ---- the documented exception: qpg_percode_select_mixed_f64 / _cut ---------------------------------------------------------
@pytest.mark.parametrize("d_is_f32", [1, 0])
@pytest.mark.parametrize("cut", [False, True])
def test_mixed_select_leaves_its_workspace_reusable(cut, d_is_f32):
    """include/qpg.h: the workspace is "ZERO-FILLED ONCE by the caller (part of it is state the launches leave all-zero for
    the next call; a workspace may be reused for any smaller Q)".  It is handed nothing but zeros here.  ONE workspace,
    zeroed once, takes `wide` (Q = 200, K = 512), then `overflow` (2080 candidates of one code inside query 0's band: the
    tier-1 list overflows, stats[1] & 1 - the path where a clean-up is most likely to be skipped), then `odd` and
    `one_window`; each of the last two gives the bits it gives on a freshly zeroed workspace, with stats[1] == 0.  (The cut
    form needs the f32 matrix: its f64 combination runs the plain call.)"""
    from qpgesture_amd import _lib
    from tests import test_gpu_select_contract as TS
    torch = _torch()
    if cut and not d_is_f32:
        cut = False                                   # "f32 matrix + workspace + out_rank" (include/qpg.h): the plain form on f64
    seq = ["wide", "overflow", "odd", "one_window"]
    cases = {n: SR.audio_case(n) for n in seq}
    need = max(int(_lib.load().qpg_percode_select_mixed_ws_bytes(c.Q, c.K)) for c in cases.values())
    dt = np.float32 if d_is_f32 else np.float64

    def call(name, ws):
        c = cases[name]
        D_in = SR.noisy("zero" if name == "overflow" else "swap", c.exact, c.cand_code, c.K, c.E, dt, seed=5)
        kw = {}
        if cut:
            ct = TS._cut_tables(c.K)
            kw["cut"] = dict(pos_t=ct["pos_t"], freq=ct["freq"], top_n=1)
        return TS._mixed(name, D_in, c.eps1, c.eps2, True, ws=ws, **kw)

    g = P.guarded(need, 0x00, device=DEV)
    reused = {n: call(n, g.buf) for n in seq}
    g.assert_tail_intact("mixed select workspace")
    assert reused["wide"][3][1] == 0
    assert reused["overflow"][3][1] & 1, "the overflow case did not overflow the tier-1 list"
    for name in ("odd", "one_window"):
        fresh = call(name, P.guarded(need, 0x00, device=DEV).buf)
        assert fresh[3][1] == 0 and reused[name][3][1] == 0
        for x, y, what in zip(reused[name][:4], fresh[:4], ("dist", "idx", "rank", "stats")):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), \
                "%s after wide + overflow: %s differs from the freshly zeroed workspace's" % (name, what)
        if not cut:
            D_in = SR.noisy("swap", cases[name].exact, cases[name].cand_code, cases[name].K, cases[name].E, dt, seed=5)
            TS._check_tables(cases[name], reused[name], D_in, cases[name].eps1)


def test_mixed_select_refuses_a_short_workspace():
    from qpgesture_amd import _lib
    from tests import test_gpu_select_contract as TS
    torch = _torch()
    c = SR.audio_case("odd")
    need = int(_lib.load().qpg_percode_select_mixed_ws_bytes(c.Q, c.K))
    D_in = SR.noisy("swap", c.exact, c.cand_code, c.K, c.E, np.float32, seed=5)
    o = Outs(0x3C)
    out = (o.new("dist", (c.Q, c.K), torch.float64), o.new("idx", (c.Q, c.K), torch.int32))
    rank = o.new("rank", (c.Q, c.K), torch.int16)
    g = P.guarded(need, 0x00, device=DEV)
    _refused(o, lambda: TS._mixed("odd", D_in, c.eps1, c.eps2, True, ws=g.buf[:need - 1], out=out, rank_out=rank))
    g.assert_tail_intact()
    assert bool((g.buf == 0).all())
