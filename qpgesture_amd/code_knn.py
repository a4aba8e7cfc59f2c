"""Host side of the code-level motion matcher: mirrors the reference's `CodeKNN` /
`predict_code_from_audio` interface (codebook/Speech2GestureMatching/GestureKNN.py:422-813)
on top of the C ABI of libqpg_hip.so.  Python here is plumbing: it owns the device tensors,
the index tables and the call order; every distance, minimum, rank and matching step runs in
the hand-written HIP kernels.  No CPU fallback exists.

Design difference from the reference (same results): the audio and text scans depend only on
the query position, never on the running (code, phase) state, so all Q = 8*M scans of a clip are
issued as two batched sweeps, and the sequential part walks (Q,512) tables on the device.
"""
import ctypes
from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .parallel import allreduce_max_, allreduce_min_index, exchange_bytes, shard_rows
from .sorted_rows import SortedRows

from .constant import (ABSENT_DIST, NUM_AUDIO_FEAT_FRAMES, STEP_SZ, WAVVQ_GROUP_SIZE, codebook_size, num_frames,
                       num_frames_code)

MODE_AUD_TXT, MODE_AUD, MODE_TXT = _lib.QPG_MODE_AUD_TXT, _lib.QPG_MODE_AUD, _lib.QPG_MODE_TXT
# mixed-precision audio sweep: a-priori error bound of qpg_audio_cosine_mx (QPG_AUDIO_MX_ERR of include/qpg.h) and the
# band inside which qpg_percode_select_mixed_f64 re-evaluates (two values further apart than 2 x the bound are ordered
# like the exact distances; 5 % margin on top)
AUDIO_MX_ERR = _lib.QPG_AUDIO_MX_ERR
AUDIO_MX_BAND = 2.1 * AUDIO_MX_ERR
# the split-operand f16 sweep (qpg_audio_cosine_hl, QPG_AUDIO_HL_ERR): a tighter bound, a narrower band.  (Round 4's
# 32-row kernel runs the cross products through the h h' chains, cross terms first: the same budget, csrc/qpg_audio_hl.hip.)
AUDIO_HL_ERR = _lib.QPG_AUDIO_HL_ERR
AUDIO_HL_BAND = 2.1 * AUDIO_HL_ERR

# bits of the trouble word the sweeps / selects raise (stats[1] of include/qpg.h) and the walk carries out with the codes
FLAG_LIST_OVERFLOW, FLAG_SMALL_NORMS, FLAG_REQUEST_OVERFLOW, FLAG_CROSS_SHARD_TIE = 1, 2, 4, 8
# the text prefilter's band list overflowed (a zero-norm context query, thousands of repeated embeddings): only the TEXT side
# has to run again, on the exact-order sweep - the audio tables of the clip stand
FLAG_TEXT_OVERFLOW = 16


_PIN_SENTINEL = -1234567          # never a status word (flag bits are small non-negative integers)


def _wait_pinned(pin_np, stream, watch=None):
    """Host side of the zero-copy results: spin on the status word (the walk's last store, behind a system-scope fence),
    then make sure no other word still holds the sentinel - a store that the fabric delivered late is waited for, never
    copied as it is (codes / votes / flags can not take the sentinel's value) - and return a copy.  After ~2 ms without the
    word (a failed launch would never write it) the stream is synchronised the ordinary way.
    watch: the words to spin on (a view of pin_np: every clip's status word when one replay walks several clips - each
    chain's block writes its own pair last); default the buffer's last word."""
    if watch is None:
        watch = pin_np[-1:]
    for _ in range(40000):
        if watch[-1] != _PIN_SENTINEL and (watch.size == 1 or not (watch == _PIN_SENTINEL).any()):
            break
    else:
        stream.synchronize()
        if (watch == _PIN_SENTINEL).any():
            raise RuntimeError("the walk did not write its status word")
    out = pin_np.copy()
    if (out == _PIN_SENTINEL).any():
        stream.synchronize()
        out = pin_np.copy()
        if (out == _PIN_SENTINEL).any():
            raise RuntimeError("the walk left result words unwritten")
    return out


class GuardOverflow(RuntimeError):
    """The capped near-tie machinery of the fast audio paths could not guarantee the reference's candidates for this
    clip (a re-evaluation list overflowed, operand norms left the error bound's range, or shard minima tied across the
    exchange).  `flags` holds the FLAG_* bits.  CodeKNN.match_clip / ClipPipeline.collect / the CLI catch it and
    re-match the clip on the uncapped path (audio_precision "exact"); codes of a flagged clip are never returned."""

    def __init__(self, flags):
        super().__init__("near-tie guard raised flags 0x%x: results of the capped path are not guaranteed" % flags)
        self.flags = int(flags)


# ----------------------------------------------------------------------------------------------
# index grids — literal restatement of the reference's float loops; tiny, host-side, done once
# ----------------------------------------------------------------------------------------------
def audio_grid(n_db_frm, step_sz):
    """Grid of search_audio_cands (GestureKNN.py:672-690): k = 0, step, 2*step, ... while
    k < n_db_frm - 4*step, with step_sz possibly a float (398/30 in wavvq mode) accumulated
    sequentially.  Returns int(k) and int(k/step_sz) per grid position."""
    kint, cidx = [], []
    k = 0
    while k < n_db_frm - STEP_SZ * step_sz:
        kint.append(int(k))
        cidx.append(int(k / step_sz))
        k += step_sz
    return kint, cidx


def text_grid():
    """Grid of search_text_cands (GestureKNN.py:713-720): k = 0,8,..,200; row/code column k//8."""
    ks = list(range(0, num_frames - STEP_SZ * 8, 8))
    return ks, [k // 8 for k in ks]


def phase_slot(k):
    """Phase start frame of a candidate: int(k/398*240) whatever unit k is in (GestureKNN.py:632)."""
    return int(k / 398 * 240)


def wavvq_tap_offsets(T):
    """Frame offsets of the 11 taps of a wavvq feature row (data_processing.py:281, 297-317):
    6 backward taps shifted by int((5-i)*s), then 5 forward taps shifted by int(i*s), s = T/30."""
    s = T / num_frames_code
    return [-int((NUM_AUDIO_FEAT_FRAMES - i - 1) * s) for i in range(NUM_AUDIO_FEAT_FRAMES)] + \
           [int(i * s) for i in range(1, NUM_AUDIO_FEAT_FRAMES)]


def _i32(x, dev):
    if isinstance(x, torch.Tensor):
        return x
    return torch.as_tensor(np.asarray(x, np.int32), device=dev)


class ExchangeLayout:
    """Byte layout of the (minimum, index) tables a rank contributes to the cross-shard exchange: `nblk` blocks (one
    per destination rank for the owner-partitioned all-to-all, one in all for the all-gather) of `Qb` query rows,
    each block = [aud_d f64 | aud_i i32 | txt_d f32 | txt_i i32] (the modalities in use), every array Qb*K entries,
    then one 8-byte slot whose first i32 is the sender's TROUBLE WORD (qpg_flags_stamp: the bits travel with the tables
    instead of in their own all-reduce).
    The select kernels write straight into it (no packing pass); qpg_merge_select_* reads the received copy.
    A layout (and its send buffer) is built once per shape and kept by the matcher (CodeKNN._layout)."""

    def __init__(self, Qtot, K, nblk, parts, audio_f64, device):
        assert Qtot % nblk == 0, "query rows must split evenly over the ranks"
        self.Qb, self.K, self.nblk, self.parts = Qtot // nblk, K, nblk, list(parts)
        n = self.Qb * K
        self.off, o = {}, 0
        for p in self.parts:
            dsz = 8 if (p == "aud" and audio_f64) else 4
            self.off[p + "_d"], o = o, o + n * dsz
            self.off[p + "_i"], o = o, o + n * 4
            o = (o + 7) // 8 * 8
        self.off["flags"], o = o, o + 8
        self.block_bytes = o
        self.dtype = {p: (torch.float64 if (p == "aud" and audio_f64) else torch.float32) for p in self.parts}
        self.send = torch.zeros((nblk * self.block_bytes,), dtype=torch.uint8, device=device)

    def views(self, p):
        """(dist, idx) tensors aliasing block 0's arrays of modality p + the select kernel's layout arguments."""
        n = self.Qb * self.K
        dsz = 8 if self.dtype[p] == torch.float64 else 4
        d = self.send[self.off[p + "_d"]:self.off[p + "_d"] + n * dsz].view(self.dtype[p])
        i = self.send[self.off[p + "_i"]:self.off[p + "_i"] + n * 4].view(torch.int32)
        return d, i, (self.Qb if self.nblk > 1 else 0), (self.block_bytes if self.nblk > 1 else 0)


class GestureDB:
    """A speaker database resident in HBM (what load_db_codebook + CodeKNN.__init__ build).

    Layout:
      base   f32 [n_local][180][F]   interpolated WavLM frames of this rank's row shard
      cn2    f64 [n_local][26]       squared norm of each audio candidate (6 frames)
      ctxt   f32 [C/64][96][64][4]   text candidates (26 grid rows per window), sklearn-normalised, tiled
      code   i32 [N][30]             replicated (payloads of winners are looked up from it)
      phase  f32 [N][240][2][8]      replicated (phase shift, amplitude)
      pos_rank i16 [512][512], freq_rank i16 [512]
    Rows [lo, hi) of the N DB windows live on this rank; candidate indices are global.
    """

    def __init__(self, code, wavlm_interp, context, phase_dense, signature, device="cuda:0",
                 freq_rank=None, pos_rank=None, rank=0, world=1, wavvq=None, feature_dtype="f32", hl_image=True,
                 text_prefilter=True):
        dev = torch.device(device)
        if feature_dtype not in ("f32", "f16"):
            raise ValueError("feature_dtype must be 'f32' or 'f16'")
        self.feature_dtype = feature_dtype
        if dev.type != "cuda":
            raise RuntimeError("GestureDB needs a HIP device (got %s); there is no CPU path" % dev)
        _lib.load()
        self.device = dev
        self.rank, self.world = rank, world
        code = np.asarray(code)
        self.N = N = code.shape[0]
        self.lo, self.hi = shard_rows(N, rank, world)
        self.n_local = self.hi - self.lo
        self.K = codebook_size
        self.code_host = code.astype(np.int64)
        self.code = _i32(code, dev).contiguous()
        self.code_local = self.code[self.lo:self.hi].contiguous()

        self.T, self.F = wavlm_interp.shape[1], wavlm_interp.shape[2]
        if isinstance(wavlm_interp, torch.Tensor):        # already on the device (interp_wavlm_device)
            self.base = wavlm_interp[self.lo:self.hi].to(dev, torch.float32).contiguous()
        else:
            self.base = torch.from_numpy(np.ascontiguousarray(wavlm_interp[self.lo:self.hi], np.float32)).to(dev)
        self.step_sz = self.T // num_frames_code                      # GestureKNN.py:432
        kint, cidx = audio_grid(self.T, self.step_sz)
        self.aud_k, self.aud_cidx_host = kint, cidx
        self.Ga = len(kint)
        self.aud_t = _i32(kint, dev)
        self.aud_cidx = _i32(cidx, dev)
        self.aud_pslot = _i32([phase_slot(k) for k in kint], dev)
        self.tap_stride = 2                                           # FRAME_INTERVAL-2, data_processing.py:266
        # code of every local candidate c = j*G + g in scan order (i16): what the one-launch select kernels index
        local = code[self.lo:self.hi]
        self.aud_cand_code = self._cand_code(local, cidx, dev)

        # vq-wav2vec track (optional; the mode the paper describes): symbols g1*320+g2, float grid of 398/30
        self.has_wavvq = wavvq is not None
        if self.has_wavvq:
            vq = np.asarray(wavvq[self.lo:self.hi])
            self.Tv = wavvq.shape[1]
            self.vq_sym = _i32(vq[..., 0].astype(np.int64) * WAVVQ_GROUP_SIZE + vq[..., 1], dev).contiguous()
            self.vq_step = self.Tv / num_frames_code                              # GestureKNN.py:436
            vk, vc = audio_grid(self.Tv, self.vq_step)
            self.vq_k, self.vq_cidx_host = vk, vc
            self.Gv = len(vk)
            self.vq_t = _i32(vk, dev)
            self.vq_cidx = _i32(vc, dev)
            self.vq_pslot = _i32([phase_slot(k) for k in vk], dev)
            self.vq_taps = wavvq_tap_offsets(self.Tv)
            self.vq_cand_code = self._cand_code(local, vc, dev)

        ks, rows = text_grid()
        self.txt_k, self.txt_rows_host = ks, rows
        self.Gt = len(ks)
        self.txt_r = _i32(rows, dev)
        self.txt_cidx = self.txt_r
        self.txt_pslot = _i32([phase_slot(k) for k in ks], dev)
        self.txt_cand_code = self._cand_code(local, rows, dev)

        # per-candidate squared norms (f64) without materialising the 6144-d windows
        fn2 = torch.empty((self.n_local, self.T), dtype=torch.float64, device=dev)
        self.cn2 = torch.empty((self.n_local, self.Ga), dtype=torch.float64, device=dev)
        if feature_dtype == "f16":
            # f16 storage of the dominant array (half the HBM bytes); norms are those of the ROUNDED values, which the
            # sweep widens in registers (qpg_audio_cosine_f64_h): the distances are the reference's on the rounded track
            self.base = self.base.to(torch.float16).contiguous()
        if self.n_local:
            src = self.base if feature_dtype == "f32" else self.base.float()
            _lib.call("qpg_frame_norm2_f64", dev, src, self.n_local * self.T, self.F, fn2)
            del src
            _lib.call("qpg_audio_cand_norm2", dev, fn2, self.n_local, self.T, self.aud_t, self.Ga,
                      NUM_AUDIO_FEAT_FRAMES, self.tap_stride, self.cn2)

        # split-operand f16 image of the track for the HBM-bound sweep (qpg_audio_cosine_hl): every frame once, in MFMA
        # fragment order; built when the grid has the reference's shape (6 taps 2 frames apart, 26 positions 6 apart)
        self.hl_image = None
        lib = _lib.load()
        # the bounded (split-f16) paths rest on one measured property of the matrix core: re-measured once per process
        # and device (selfcheck.mfma_bound_ok); a device that fails it gets the f64 sweep and the exact-order text sweep
        self.hl_bound_ok, self.hl_bound_report = (True, {"skipped": True})
        if (hl_image or text_prefilter) and self.n_local:
            from .selfcheck import mfma_bound_ok
            self.hl_bound_ok, self.hl_bound_report = mfma_bound_ok(dev)
            if not self.hl_bound_ok:
                hl_image = text_prefilter = False
        # (feature_dtype "f16", round 5: an f16 value is its own h plane - a ONE-plane image, half the bytes, two products
        # per element instead of three: qpg_audio_cosine_hl1)
        self.hl_planes = 2 if feature_dtype == "f32" else 1
        supported = lib.qpg_audio_hl_supported if feature_dtype == "f32" else lib.qpg_audio_hl1_supported
        if (hl_image and self.n_local and len(kint) > 1 and
                kint == [i * (kint[1] - kint[0]) for i in range(len(kint))] and
                supported(self.T, self.F, self.Ga, NUM_AUDIO_FEAT_FRAMES, self.tap_stride, kint[1] - kint[0])):
            if feature_dtype == "f32":
                nb = int(lib.qpg_audio_hl_db_bytes(self.n_local, self.F))
                self.hl_image = torch.empty((nb,), dtype=torch.uint8, device=dev)
                _lib.call("qpg_audio_hl_pack_db", dev, self.base, self.n_local, self.T, self.F, self.Ga,
                          NUM_AUDIO_FEAT_FRAMES, self.tap_stride, kint[1] - kint[0], self.hl_image, nb)
            else:
                nb = int(lib.qpg_audio_hl1_db_bytes(self.n_local, self.F))
                self.hl_image = torch.empty((nb,), dtype=torch.uint8, device=dev)
                _lib.call("qpg_audio_hl1_pack_db", dev, self.base, self.n_local, self.T, self.F, self.Ga,
                          NUM_AUDIO_FEAT_FRAMES, self.tap_stride, kint[1] - kint[0], self.hl_image, nb)

        ctx = np.ascontiguousarray(context[self.lo:self.hi], np.float32)
        self.R, self.Dt = context.shape[1], context.shape[2]
        ctx_d = torch.from_numpy(ctx).to(dev)
        self.Ct = self.n_local * self.Gt
        # normalised grid rows, tiled [C/64][Dt/4][64][4] for lane-per-candidate access
        self.ctxt = torch.zeros((((self.Ct + 63) // 64) * 64 * self.Dt,), dtype=torch.float32, device=dev)
        if self.n_local:
            _lib.call("qpg_text_pack_candidates_f32", dev, ctx_d, self.n_local, self.R, self.Dt, self.txt_r,
                      self.Gt, self.ctxt)
        # text candidates sorted by code + their split-f16 image for the bounded prefilter (sorted_rows.SortedRows,
        # csrc/qpg_sorted.hip): rows normalised by the kernel the exact sweep's candidates are normalised by
        self.txt_sorted = None
        if text_prefilter and self.n_local and self.Dt % 128 == 0 and self.K < 0x2000:
            rows_f = ctx_d[:, torch.as_tensor(np.asarray(rows, np.int64), device=dev), :].reshape(self.Ct, self.Dt)
            rows_n = torch.empty_like(rows_f)
            _lib.call("qpg_l2_normalize_rows_f32", dev, rows_f.contiguous(), self.Ct, self.Dt, rows_n)
            self.txt_sorted = SortedRows(rows_n, self.txt_cand_code[:self.Ct], self.K, dev)
            # batches of >= 256 text queries (six clips or more per sweep) take the h-plane prefilter + the by-code select
            # (round 5: every row is then wanted by several queries); a single clip's 48 queries stay on the by-query path
            self.txt_sorted.by_code = True
            del rows_f, rows_n
        del ctx_d

        ph = np.ascontiguousarray(np.asarray(phase_dense, np.float32)[:, :, [0, 2], :])
        self.Tp = ph.shape[1]
        self.phase = torch.from_numpy(ph).to(dev)
        self.phase_host = ph

        sig = torch.from_numpy(np.ascontiguousarray(signature, np.float32)).to(dev)
        self.signature = sig
        if pos_rank is None:
            pd = torch.empty((self.K, self.K), dtype=torch.float32, device=dev)
            _lib.call("qpg_l2_table_f32", dev, sig, self.K, sig.shape[1], pd)
            self.pos_dist = pd
            self.pos_rank = torch.empty((self.K, self.K), dtype=torch.int16, device=dev)
            _lib.call("qpg_rank_rows_f32", dev, pd, self.K, self.K, self.pos_rank)
        else:
            self.pos_rank = torch.as_tensor(np.asarray(pos_rank, np.int16), device=dev).contiguous()

        # code_to_freq (GestureKNN.py:481-499): 1 - count/total, 1 for unseen codes; rank of it (:544)
        cnt = np.bincount(code.reshape(-1), minlength=self.K)[:self.K]
        self.freq_dist = np.where(cnt > 0, 1 - cnt / cnt.sum(), 1.0)
        # (the walk-relevance cut of the select reads a code's column: qpg_percode_select_mixed_f64_cut)
        self.pos_rank_t = self.pos_rank.t().contiguous()
        if freq_rank is None:
            fd = torch.from_numpy(self.freq_dist[None].copy()).to(dev)
            self.freq_rank = torch.empty((1, self.K), dtype=torch.int16, device=dev)
            _lib.call("qpg_rank_rows_f64", dev, fd, 1, self.K, self.freq_rank)
            self.freq_rank = self.freq_rank[0].contiguous()
        else:
            self.freq_rank = torch.as_tensor(np.asarray(freq_rank, np.int16), device=dev).contiguous()

    # -- prepared-database cache (round 5; db_cache.py): what the constructor built, written once, restored without a
    #    single build launch - the drop-in CLI's second and later invocations (GestureKNN.py:816-845 reloads everything)
    def save(self, path, key="", sources=None):
        from . import db_cache
        return db_cache.save(self, path, key, sources=sources)

    @classmethod
    def load(cls, path, device="cuda:0", key=None):
        """The GestureDB saved at `path`, or None (missing / foreign / keyed differently).  The bounded paths' one
        measured hardware property is re-measured on THIS device (selfcheck.mfma_bound_ok): a device that fails it keeps
        the restored object but not its split-f16 images."""
        from . import db_cache
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("GestureDB needs a HIP device (got %s); there is no CPU path" % dev)
        _lib.load()
        db = db_cache.load(path, dev, key)
        if db is None:
            return None
        if db.hl_image is not None or db.txt_sorted is not None:
            from .selfcheck import mfma_bound_ok
            db.hl_bound_ok, db.hl_bound_report = mfma_bound_ok(dev)
            if not db.hl_bound_ok:
                db.hl_image = db.txt_sorted = None
        return db

    @staticmethod
    def _cand_code(code_local, cidx, dev):
        cc = np.ascontiguousarray(code_local[:, np.asarray(cidx, np.int64)].reshape(-1))
        cc = np.where((cc >= 0) & (cc < 32767), cc, -1).astype(np.int16)        # out-of-range ids are skipped
        return torch.from_numpy(cc if cc.size else np.zeros((1,), np.int16)).to(dev)

    @property
    def idx_base(self):
        return self.lo


# ----------------------------------------------------------------------------------------------
# the plan of a sweep / of a step: which kernels, in which order.  Pure functions of plain values (no torch, no library):
# CodeKNN computes a plan once per call and its methods carry it out; the decisions are tested on the CPU
# ----------------------------------------------------------------------------------------------
# the switches of a CodeKNN that a plan reads (documented where CodeKNN.__init__ sets them; the defaults are its own)
Knobs = namedtuple("Knobs", "audio_precision audio_kernel text_kernel tie_eps mixed_single_launch sharded_mixed "
                   "sharded_mixed_min_gflop force_sharded overlap_sweeps text_after_sweep audio_first fused_pack rank_cut "
                   "split_fuse split_fuse_max_steps host_ranks use_wavvq",
                   defaults=("mixed", "hl", "mfma", 1e-12, False, True, 20.0, False, True, True, None, True, True, True,
                             256, False, False))
# what a plan needs to know about a GestureDB
DBFacts = namedtuple("DBFacts", "n_local N world K Ga F Dt feature_dtype hl_bound_ok has_hl_image has_txt_sorted hl_planes",
                     defaults=("f32", True, True, True, 2))


class AudioPlan(NamedTuple):
    path: str           # the select that settles the sweep's matrix: "mixed" | "exact" | "guarded" | "plain"
    kernel: str         # the sweep kernel qpg_audio_cosine_<kernel>: "hl" | "hl1" | "mx" | "mx_h" | "f64" | "f64_h"
    band: float         # what the mixed select / merge re-evaluates: AUDIO_HL_BAND / AUDIO_MX_BAND (0: not mixed)
    cut_top_n: int      # walk-relevance cut of the mixed select: 0 = off, 1 (audio + text), 2 (audio only)
    fused_rank: bool    # the select writes the ranks as well


class StepPlan(NamedTuple):
    audio: Optional[AudioPlan]      # None: no WavLM audio side (MODE_TXT, or the wavvq sweep, which has one path)
    text: Optional[str]             # "mfma" | "valu"; None: no text side (MODE_AUD)
    sharded: bool                   # per-shard tables into the exchange layout, merged behind one collective
    exchange: Optional[str]         # sharded: "all_to_all" (owner blocks) | "all_gather"
    clip_pack: bool                 # both query packs in one launch (qpg_clip_pack_hl)
    split_fuse: bool                # each side's half of the rank fusion behind its own select, into the gate tables
    overlap: bool                   # the text side on the side stream
    order: Optional[str]            # overlap: "text_first" | "text_after_sweep" | "audio_first"


def plan_audio(kn, db, Q, want_rank=False, reduce=True, out_given=False, cut_top_n=0):
    """The AudioPlan of one WavLM sweep of Q queries (CodeKNN.sweep_audio's arguments; out_given: `out` is not None)."""
    C = db.n_local * db.Ga
    fused_rank = want_rank and db.world == 1
    local_final = fused_rank and reduce and not out_given           # one GPU: this select decides everything
    shard_part = (db.world > 1 or kn.force_sharded) and not reduce and out_given     # row shard: sweep_tables merges
    # (the same number on every rank - the largest shard's - so that all ranks take the same path: the mixed merge has
    # two more collectives than the f64 one)
    gflop = 2e-9 * Q * (-(-db.N // db.world) * db.Ga) * NUM_AUDIO_FEAT_FRAMES * db.F
    guard = kn.tie_eps > 0 and C > 0
    half = db.feature_dtype == "f16"
    if (kn.audio_precision == "mixed" and guard and db.K <= 512 and db.hl_bound_ok and
            (local_final or (shard_part and kn.sharded_mixed and gflop >= kn.sharded_mixed_min_gflop))):
        hl = kn.audio_kernel == "hl" and db.has_hl_image
        kernel = ("hl" if db.hl_planes == 2 else "hl1") if hl else ("mx_h" if half else "mx")
        cut = cut_top_n if (cut_top_n in (1, 2) and local_final and not kn.mixed_single_launch) else 0
        return AudioPlan("mixed", kernel, AUDIO_HL_BAND if hl else AUDIO_MX_BAND, cut, fused_rank)
    path = "exact" if (kn.audio_precision == "exact" and guard) else ("guarded" if guard else "plain")
    return AudioPlan(path, "f64_h" if half else "f64", 0.0, 0, fused_rank)


def plan_text(kn, db, Q, reduce=True, out_given=False):
    """ "mfma" (bounded prefilter over the sorted image + exact band evaluation) or "valu" (the exact-order sweep) for one
    text sweep of Q queries (CodeKNN.sweep_text's arguments)."""
    mfma = (kn.text_kernel == "mfma" and db.has_txt_sorted and Q > 0 and kn.audio_precision != "exact" and
            ((not out_given and reduce and db.world == 1) or (out_given and not reduce)))
    return "mfma" if mfma else "valu"


def plan_step(kn, db, M, steps, mode=MODE_AUD_TXT, for_walk=False, owner_blocks=False):
    """The StepPlan of CodeKNN.sweep_tables over M windows of `steps` matching steps each."""
    Q = M * steps
    sharded = db.world > 1 or kn.force_sharded
    audio = text = None
    if mode != MODE_TXT and not kn.use_wavvq:
        cut = 0
        if for_walk and kn.rank_cut and not sharded and not kn.host_ranks:
            cut = 1 if mode == MODE_AUD_TXT else 2
        audio = plan_audio(kn, db, Q, want_rank=not sharded, reduce=not sharded, out_given=sharded, cut_top_n=cut)
    if mode != MODE_AUD:
        text = plan_text(kn, db, Q, reduce=not sharded, out_given=sharded)
    split = (for_walk and mode == MODE_AUD_TXT and not sharded and not kn.host_ranks and kn.split_fuse and
             db.K % 16 == 0 and db.K <= 4096 and Q <= kn.split_fuse_max_steps)
    overlap = mode == MODE_AUD_TXT and kn.overlap_sweeps
    mfma_text = kn.text_kernel == "mfma" and db.has_txt_sorted and kn.audio_precision != "exact"
    # (the pack is the split-f16 sweep's: it follows the audio plan.  An hl image exists only for Ga > 1, so the plan's
    # `n_local * Ga > 0` is the `n_local > 0` this decision used to ask on every database that can be built)
    clip_pack = (overlap and not kn.use_wavvq and mfma_text and audio.kernel in ("hl", "hl1") and db.Dt % 128 == 0 and
                 kn.fused_pack)
    audio_first = mfma_text if kn.audio_first is None else bool(kn.audio_first)
    after = overlap and kn.text_after_sweep and not audio_first and not kn.use_wavvq
    order = None
    if overlap:
        order = "audio_first" if audio_first else ("text_after_sweep" if after else "text_first")
    exchange = ("all_to_all" if owner_blocks else "all_gather") if sharded else None
    return StepPlan(audio, text, sharded, exchange, clip_pack, split, overlap, order)


class TakesPlan(NamedTuple):
    path: str           # "kernel": qpg_match_steps_takes | "per_take": one walk() per take | "unsupported"
    reason: str         # why not "kernel" ("" when it is)


def plan_takes(kn, db, M, steps, n_takes, serial_walk=False):
    """How CodeKNN.walk_takes walks n_takes takes of a clip of M windows x `steps` steps: the multi-take kernels, or the
    per-take fallback where the tabulated walk does not apply (the conditions are those of the library's
    tabulated_walk_ok, csrc/qpg_tail.hip, which answers QPG_EUNSUP for the same cases), or not at all (row shards).
    host_ranks tables, for_walk tables and the wavvq sweep's tables are all walked by the kernels: they only read ranks and
    candidate indices."""
    if db.world > 1 or kn.force_sharded:
        return TakesPlan("unsupported", "takes of a row-sharded database are not implemented (the merged tables would serve; "
                                        "nothing tests them)")
    if serial_walk:
        return TakesPlan("per_take", "the one-wave sequential walk was asked for (serial_walk)")
    K = db.K
    last_idx = min(steps * 4, num_frames_code) - 1
    if (last_idx // 4 != steps - 1 or M * steps > 2048 or 2 * steps * 2 * K * 2 > 64 * 1024 or (steps * 2 * K) % 8 or
            2 * K > 65536):
        return TakesPlan("per_take", "the tabulated walk does not take this geometry (steps = %d, K = %d, %d steps per clip)"
                         % (steps, K, M * steps))
    if not 1 <= n_takes <= _lib.QPG_TAKES_MAX:
        return TakesPlan("per_take", "n_takes outside [1, %d]" % _lib.QPG_TAKES_MAX)
    return TakesPlan("kernel", "")


class NoPhasePlan(NamedTuple):
    path: str           # "kernel": qpg_match_steps_nophase | "unsupported"
    for_walk: bool      # what sweep_tables is asked for: always False (fully settled tables, see below)
    reason: str         # why "unsupported"; for "kernel": why the tables are the settled ones


def plan_nophase(kn, db, M, steps, mode, desired_k):
    """How a matcher without the phase gate (CodeKNN(use_phase=False)) matches a clip of M windows x `steps` steps.
    The walk-relevance cut (AudioPlan.cut_top_n) and the prefused gate tables (StepPlan.split_fuse) never feed this walk:
    the cut proves that a code cannot take the first (or first two) places of the TWO-way fusion pos + rank, and the
    three-way winner (pos + aud + txt) and position desired_k are outside that proof - so the tables are always those of
    sweep_tables(for_walk=False), exact everywhere.  Row shards are not implemented; the geometry conditions are the
    library's (walk_geom, csrc/qpg_tail.hip: QPG_EUNSUP for the same cases)."""
    if mode not in (MODE_AUD_TXT, MODE_AUD, MODE_TXT):
        return NoPhasePlan("unsupported", False, "mode %r is not one of MODE_AUD_TXT / MODE_AUD / MODE_TXT" % (mode,))
    if db.world > 1 or kn.force_sharded:
        return NoPhasePlan("unsupported", False, "matching without the phase gate on a row-sharded database is not "
                                                 "implemented (the merged tables would serve; nothing tests them)")
    if not 0 <= desired_k < min(_lib.QPG_NOPHASE_KMAX, db.K):
        return NoPhasePlan("unsupported", False, "desired_k %d outside [0, %d)" % (desired_k, _lib.QPG_NOPHASE_KMAX))
    K = db.K
    last_idx = min(steps * 4, num_frames_code) - 1
    if (steps < 1 or steps * 4 > 64 or K % 4 or K > 1024 or last_idx // 4 != steps - 1 or M * steps > 2048 or
            2 * steps * 2 * K * 2 > 64 * 1024 or (steps * 2 * K) % 8):
        return NoPhasePlan("unsupported", False, "the tabulated walk does not take this geometry (steps = %d, K = %d, %d "
                                                 "steps per clip)" % (steps, K, M * steps))
    return NoPhasePlan("kernel", False, "the walk-relevance cut covers the two-way fusion's first places only: position "
                                        "%d of the %s-way order reads fully settled tables"
                       % (desired_k, "three" if mode == MODE_AUD_TXT else "two"))


# what CodeKNN._sweep_audio leaves: the per-shard (not yet reduced) tables, the sweep's matrix, the packed queries (the
# sharded merge re-evaluates requested pairs from them) and the AudioPlan that was carried out
AudioResult = namedtuple("AudioResult", "dist idx rank D q32 qn2 plan")


def _grown(buf, nbytes, dev, zero=False):
    """`buf` if it holds nbytes, else a new byte buffer of that size (zero: zero-filled)."""
    if buf is not None and buf.numel() >= nbytes:
        return buf
    return (torch.zeros if zero else torch.empty)((nbytes,), dtype=torch.uint8, device=dev)


class CodeKNN:
    """Mirror of the reference's CodeKNN (GestureKNN.py:422-721) over a GestureDB."""

    def __init__(self, db, use_wavlm=True, use_wavvq=False, use_phase=True, use_txt=True, rng=None, desired_k=0):
        """use_phase=False: the reference's matching without the phase gate (GestureKNN.py:578-592):
        position `desired_k` of the fused order, a coin per step between the audio and the text candidate; match_clip then
        returns (codes, phases [M,0,8,16], sides).  desired_k is read by such a matcher only (as in the reference)."""
        if use_wavlm == use_wavvq:
            raise ValueError("exactly one of use_wavlm / use_wavvq (GestureKNN.py:431-438)")
        if use_wavvq and not db.has_wavvq:
            raise ValueError("GestureDB was built without a wavvq track")
        self.db = db
        self.use_wavvq = use_wavvq
        if use_wavvq:                                                       # GestureKNN.py:435-438
            self.step_sz, self.n_db_frm = db.vq_step, db.Tv
        else:                                                               # :431-434
            self.step_sz, self.n_db_frm = db.step_sz, db.T
        self.n_db_seq = db.N
        self.use_phase, self.use_txt = use_phase, use_txt
        if not use_phase and not 0 <= int(desired_k) < _lib.QPG_NOPHASE_KMAX:
            raise ValueError("desired_k must be in [0, %d) (got %r)" % (_lib.QPG_NOPHASE_KMAX, desired_k))
        self.desired_k = int(desired_k)
        self.last_picks = None              # no-phase matcher: the candidate j * G + g every step appended, i32 [M, steps]
        self.rng = rng if rng is not None else np.random
        self.overlap_sweeps = True          # text sweep on a second HIP stream underneath the audio sweep
        self.text_after_sweep = True        # ... started when the audio sweep ends, i.e. underneath the audio SELECT ...
        self.audio_first = None             # no ordering between the two streams; None: auto (sweep_tables)
        self.serial_walk = False            # True: force the one-wave sequential walk (tests compare the two)
        # Near-tie guard of the audio select (qpg_percode_select_guarded_f64): candidates / code minima closer than
        # tie_eps are re-evaluated in the reference's own arithmetic inside the select launch.  0 disables it.
        self.tie_eps = 1e-12
        self._guard_stats = torch.zeros((4,), dtype=torch.int32, device=db.device)
        # audio_precision "mixed" (default): the sweep runs on the f32 matrix cores with an a-priori error bound
        # (qpg_audio_cosine_mx, |error| <= AUDIO_MX_ERR) and the select re-evaluates every comparison the bound leaves
        # open with f64 dot products, then the near-tie guard (qpg_percode_select_mixed_f64): same candidates and ranks
        # as "f64", the sweep at twice the matrix rate.  Taken only where the select sees every comparison that
        # follows (single-GPU DB, ranks fused, guard on; f32 or f16 base); everything else runs the f64 sweep.
        # "exact" (round 3): the f64 sweep + the UNCAPPED guard (qpg_percode_select_exact_f64; across shards a
        # reference-arithmetic request / response round): no list that can overflow, whatever the data.  It is the path
        # a clip is re-matched on when the faster ones raise their trouble word (GuardOverflow), and can be selected
        # outright.  fallbacks counts the clips that took it that way.
        self.audio_precision = "mixed"
        # kernel of the mixed-precision sweep: "hl" = split-operand f16 matrix cores on the frame-major image (HBM-bound;
        # needs GestureDB.hl_image), "mx" = the f32 matrix cores on the f32 / f16 base.  Same bound, same select.
        self.audio_kernel = "hl"
        # text_kernel "mfma" (round 3, default where the DB holds the sorted image: one GPU): bounded split-f16 prefilter
        # over the candidates sorted by code + exact sklearn-order evaluation of every code's band (bit-identical tables;
        # an overflowing band list raises the trouble word and the clip is re-matched on the exact sweep); "valu": the
        # exact-order sweep of every pair (qpg_text_cosine_f32).
        self.text_kernel = "mfma"
        # column image / prefilter matrix / tile minima of the text prefilter: per matcher (= per stream), never on the
        # shared GestureDB.txt_sorted - the lanes of a ClipPipeline run their text sides concurrently
        self._txt_scratch = {}
        self.fallbacks = 0
        # a clip's audio AND text query packs in one launch (qpg_clip_pack_hl; False / QPG_FUSED_PACK=0: round 3's separate
        # launches - tests and measurements compare the two)
        import os as _os
        self.fused_pack = _os.environ.get("QPG_FUSED_PACK", "1") != "0"
        # Walk-relevance cut (round 4, last hours): when the tables go straight into the walk (match_clip without
        # return_tables, ClipGraph, ClipPipeline, bench.py's step: sweep_tables(for_walk=True)) the select settles in f64
        # only what the walk can read - codes whose rank is certainly above every step's winning fused score keep their
        # sweep values (include/qpg.h: qpg_percode_select_mixed_f64_cut).  The codes the walk returns are the same; the
        # tables sweep_tables() hands to anyone else are exact everywhere, as before.  QPG_RANK_CUT=0: off.
        self.rank_cut = _os.environ.get("QPG_RANK_CUT", "1") != "0"
        self.rank_cut_probe = 64
        self.mixed_single_launch = False    # True: the select's tier-1 work stays inside one launch (tests compare both)
        self.split_fuse = True              # the rank fusion per modality behind its select (False: one launch in the walk)
        self.split_fuse_max_steps = 256     # ... for sweeps of at most this many matching steps
        # Row-sharded DB: the shards sweep in mixed precision too and the cross-shard merge re-evaluates what their
        # bounded tables leave open through a request / response exchange (sweep_tables; qpg_merge_mixed_*).
        # Two more (small) exchanges buy a sweep at ~1.6x the rate, so it is used where the shard's sweep is long enough
        # to pay for them: at least sharded_mixed_min_gflop per rank and step (24 s clip x 2048 windows = 31 GFLOP).
        self.sharded_mixed = True
        # force_sharded: take the row-shard code path (exchange layout, collectives, merge kernels) even with world == 1,
        # so that a one-GPU box can execute it over RCCL (backend nccl, world_size 1): tests / bench only
        self.force_sharded = False
        self.sharded_mixed_min_gflop = 20.0
        self.mixed_requests = None          # request slots per (owner, shard) pair and step; None: 16384 / world
        # host_ranks (the CLI's --tie_rule numpy): rank the (Q,512) audio / text minima with the reference's own
        # `np.array(x).argsort().argsort()` on the host, so that EXACT ties between codes (structural in real text
        # embeddings: silent frames share one vector) get NumPy's unstable-sort order like the reference's.
        self.host_ranks = False

        # state that appears with use: caches per shape / clip length / knobs, the side stream and its events, grown buffers
        self._qpos, self._qcache, self._layouts, self._mm_cache, self._pinned_ints, self._plans = None, {}, {}, {}, {}, {}
        self._side_stream = self._side_gate = self._side_done = self._sweep_event = None
        self._mix_ws = self._exact_ws = self._hl_qimage = self._takes_ws = self._nophase_ws = None
        self._pinned_nophase = None
        # bench.py: HIP events around the sweep kernel of every kernel_events_every-th call, appended to kernel_events
        # (a list; None: off), taken from kernel_event_pool while it lasts (events created ahead of the timed region)
        self.kernel_events, self.kernel_events_every, self.kernel_event_pool, self._ev_calls = None, 1, None, 0
        # diagnostics of the last sweep / walk: tests, tools and bench.py read them, nothing in the package decides by them
        self.text_fallbacks, self.tables, self._last_mix_Q = 0, None, 0
        self._last_audio_mixed = self._last_audio_exact = self._last_audio_hl = False
        self._last_text_mfma = self._last_rank_cut = False
        self._last_D_aud = self._last_q32 = self._last_qn2 = self._last_ints = self._last_gate_tables = None

    def _knobs(self):
        return Knobs(self.audio_precision, self.audio_kernel, self.text_kernel, self.tie_eps, self.mixed_single_launch,
                     self.sharded_mixed, self.sharded_mixed_min_gflop, self.force_sharded, self.overlap_sweeps,
                     self.text_after_sweep, self.audio_first, self.fused_pack, self.rank_cut, self.split_fuse,
                     self.split_fuse_max_steps, self.host_ranks, self.use_wavvq)

    def _facts(self):
        db = self.db
        return DBFacts(db.n_local, db.N, db.world, db.K, db.Ga, db.F, db.Dt, db.feature_dtype, db.hl_bound_ok,
                       db.hl_image is not None, db.txt_sorted is not None, db.hl_planes)

    def _audio_grid(self):
        db = self.db
        if self.use_wavvq:
            return db.vq_cidx, db.vq_pslot, db.Gv
        return db.aud_cidx, db.aud_pslot, db.Ga

    def query_positions(self):
        """Matching-step positions of a window: i = 0, 4*step, ... while i < n (GestureKNN.py:528,659);
        with the float wavvq step the literal accumulation is kept."""
        key = (self.n_db_frm, self.step_sz)
        if self._qpos is not None and self._qpos[0] == key:          # (twice per clip, in front of its first launch)
            return self._qpos[1]
        pos, i = [], 0
        while i < self.n_db_frm:
            pos.append(i)
            i += STEP_SZ * self.step_sz
        self._qpos = (key, pos)
        return pos

    # -- init (GestureKNN.py:462-473): same two draws from the (seeded) NumPy global stream ------
    def init_code_phase(self):
        db = self.db
        i = self.rng.randint(0, self.n_db_seq)
        j = self.rng.randint(0, self.n_db_frm - int(num_frames / num_frames_code))
        code = int(db.code_host[i, j // num_frames_code])
        if not self.use_phase:                                     # :466-467: the same two draws, the code alone
            return code
        P = db.phase_host[i, j:j + 8]                              # (8,2,8)
        if P.shape[0] != 8:
            # wavvq mode draws j up to 389 on a 240-frame phase track (GestureKNN.py:464-469): the reference's
            # np.array(result_phase) then raises "inhomogeneous shape" on NumPy >= 1.24
            raise ValueError("init_code_phase drew frame %d: phase slice has %d rows, not 8 "
                             "(the reference fails on this draw too); use another seed" % (j, P.shape[0]))
        return code, np.concatenate((P[:, 0], P[:, 1]), axis=1).astype(np.float32)

    # -- batched sweeps ------------------------------------------------------------------------
    def _tables_out(self, Q, dtype, out, with_rank):
        """(dist, idx, rank, q_block, block_stride) a select writes: the views of the sharded path's exchange layout
        `out` (written in place, merged after the collective) or new [Q,K] tables."""
        K, dev = self.db.K, self.db.device
        dist, idx, qb, bs = out if out is not None else (torch.empty((Q, K), dtype=dtype, device=dev),
                                                         torch.empty((Q, K), dtype=torch.int32, device=dev), 0, 0)
        return dist, idx, (torch.empty((Q, K), dtype=torch.int16, device=dev) if with_rank else None), qb, bs

    def _select_plain(self, D, cand_code, C, G, out, with_rank):
        """First-wins per-code minimum of a distance matrix D [Q, C] whose candidates lie on a grid of G positions per
        window: (dist, idx, rank or None)."""
        db, Q = self.db, D.shape[0]
        dist, idx, rank, qb, bs = self._tables_out(Q, D.dtype, out, with_rank)
        _lib.call("qpg_percode_select_f64" if D.dtype == torch.float64 else "qpg_percode_select_f32", db.device, D,
                  D.stride(0), Q, cand_code, C, db.K, float(ABSENT_DIST), db.idx_base * G, dist, idx, rank, qb, bs)
        return dist, idx, rank

    def _finish(self, dist, idx, rank, want_rank, reduce):
        """What the public sweeps return: the tables as they are (not reduce: a sharded caller combines several in one
        exchange, sweep_tables), or min-reduced across ranks, with the ranks if asked."""
        if not reduce:
            return dist, idx
        dist, idx = self._reduce_min(dist, idx)
        if want_rank:
            return dist, idx, (rank if rank is not None else self.rank_rows(dist))
        return dist, idx

    def _sweep_timer(self):
        """The (start, end) events for this call's sweep kernel, or None (kernel_events off, or not this call's turn)."""
        if self.kernel_events is None:
            return None
        if self.kernel_events_every > 1:
            self._ev_calls += 1
            if self._ev_calls % self.kernel_events_every:
                return None
        return (self.kernel_event_pool.pop() if self.kernel_event_pool else
                (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))

    def sweep_audio(self, qbase, q_win, q_t, tap_stride=None, want_rank=False, reduce=True, out=None, prepacked=None,
                    cut_top_n=None):
        """Per-code best audio candidate for every query: returns (dist f64 [Q,512], idx i32 [Q,512])
        with global candidate indices j*26+g (-1 = code absent), min-reduced across ranks; with
        want_rank also the stable ranks i16 [Q,512]."""
        Q = int(q_win.shape[0]) if isinstance(q_win, torch.Tensor) else len(q_win)
        plan = plan_audio(self._knobs(), self._facts(), Q, want_rank, reduce, out is not None, cut_top_n or 0)
        r = self._sweep_audio(plan, qbase, q_win, q_t, tap_stride, out, prepacked)
        return self._finish(r.dist, r.idx, r.rank, want_rank, reduce)

    def _sweep_audio(self, plan, qbase, q_win, q_t, tap_stride=None, out=None, prepacked=None, sweep_event=None,
                     after_sweep=None):
        """The WavLM audio side as `plan` (an AudioPlan) says: query pack, sweep, select -> AudioResult.
        prepacked = (q32, qn2, ...): sweep_tables packed the clip's whole query side in one launch.  Directly behind the
        sweep kernel on the current stream: after_sweep() is called (ClipGraph: the encode leg forks there / the sweep
        signal is raised) and sweep_event is recorded (sweep_tables: the text side starts behind the sweep)."""
        db, dev = self.db, self.db.device
        Q = int(q_win.shape[0]) if isinstance(q_win, torch.Tensor) else len(q_win)
        qbase = qbase.contiguous()
        M, T, F = qbase.shape
        ts = db.tap_stride if tap_stride is None else tap_stride
        if prepacked is not None:
            q32, qn2 = prepacked[0], prepacked[1]
        else:
            q32 = torch.empty((Q, NUM_AUDIO_FEAT_FRAMES * F), dtype=torch.float32, device=dev)
            qn2 = torch.empty((Q,), dtype=torch.float64, device=dev)
        C = db.n_local * db.Ga
        mixed, use_hl, half = plan.path == "mixed", plan.kernel in ("hl", "hl1"), db.feature_dtype == "f16"
        # the mixed-precision sweep stores its matrix in f32: it only feeds the select's two streaming passes
        D = torch.empty((Q, max(C, 1)), dtype=torch.float32 if mixed else torch.float64, device=dev)
        timer = self._sweep_timer()
        sweep_fn = "qpg_audio_cosine_" + plan.kernel
        if use_hl:                    # gather + norms + split-f16 image in ONE launch
            qi = self._hl_qimage = _grown(self._hl_qimage, int(_lib.load().qpg_audio_hl_query_bytes(Q, db.F)), dev)
            # the sweep's arguments are converted BEFORE the pack goes out: its launch follows the pack's at once
            sweep_launch = _lib.prepare(sweep_fn, dev, db.hl_image, db.n_local, db.F, db.Ga, db.cn2, qi,
                                        qn2, Q, D, 1, D.stride(0), self._guard_stats)
            if prepacked is None:
                _lib.call("qpg_audio_pack_queries_hl", dev, qbase, M, T, F, _i32(q_win, dev), _i32(q_t, dev), Q,
                          NUM_AUDIO_FEAT_FRAMES, ts, q32, qn2, qi, qi.numel())
        else:
            assert prepacked is None, "the one-launch clip pack feeds the split-f16 sweep only"
            _lib.call("qpg_audio_pack_queries", dev, qbase, M, T, F, _i32(q_win, dev), _i32(q_t, dev), Q,
                      NUM_AUDIO_FEAT_FRAMES, ts, q32, qn2)
        if timer is not None:
            timer[0].record(torch.cuda.current_stream(dev))          # (the events bracket the sweep kernel alone)
        if use_hl:
            sweep_launch()
        else:
            strides = (1, D.stride(0), self._guard_stats) if mixed else (D.stride(0),)     # (mx: + the trouble word)
            _lib.call(sweep_fn, dev, db.base, db.n_local, db.T, db.F, db.aud_t, db.Ga, NUM_AUDIO_FEAT_FRAMES,
                      db.tap_stride, db.cn2, q32, qn2, Q, D, *strides)
        if timer is not None:
            timer[1].record(torch.cuda.current_stream(dev))
            self.kernel_events.append(timer)
        if after_sweep is not None:
            after_sweep()
        if sweep_event is not None:
            sweep_event.record(torch.cuda.current_stream(dev))
        if plan.path == "plain":
            dist, idx, rank = self._select_plain(D, db.aud_cand_code, C, db.Ga, out, plan.fused_rank)
        else:
            dist, idx, rank, qb, bs = self._tables_out(Q, torch.float64, out, plan.fused_rank)
            tables = (Q, db.aud_cand_code, C, db.K, float(ABSENT_DIST), db.idx_base * db.Ga, dist, idx, rank, qb, bs)
            # what the guards re-evaluate a pair from, in the reference's own arithmetic
            track = (db.base, db.T, db.F, db.aud_t, db.Ga, NUM_AUDIO_FEAT_FRAMES, db.tap_stride, q32)
        if mixed:
            # (zero-filled ONCE: the select's streamed state is all-zero between launches, qpg.h)
            ws = self._mix_ws = _grown(self._mix_ws, int(_lib.load().qpg_percode_select_mixed_ws_bytes(Q, db.K)), dev,
                                       zero=True)
            single = self.mixed_single_launch        # the select's tier-1 work inside one launch: no workspace
            sel_args = (D, 1, D.stride(0), *tables, *track, qn2, db.cn2, plan.band, float(self.tie_eps),
                        self._guard_stats, None if single else ws, 0 if single else ws.numel(), int(half))
            try:
                if plan.cut_top_n:
                    _lib.call("qpg_percode_select_mixed_f64_cut", dev, *sel_args, db.pos_rank_t, db.freq_rank,
                              int(plan.cut_top_n), int(self.rank_cut_probe))
                else:
                    _lib.call("qpg_percode_select_mixed_f64", dev, *sel_args)
            except Exception:
                # a failed launch between the streaming pass and the list pass would leave streamed state behind that
                # later clips consume silently (the kernels only restore the all-zero state when all of them ran)
                self._mix_ws = None
                raise
        elif plan.path == "exact":
            ws = self._exact_ws = _grown(self._exact_ws, int(_lib.load().qpg_percode_select_exact_ws_bytes(Q, C, db.K)),
                                         dev)
            _lib.call("qpg_percode_select_exact_f64", dev, D, D.stride(0), *tables, *track, float(self.tie_eps),
                      self._guard_stats, int(half), ws, ws.numel())
        elif plan.path == "guarded":
            _lib.call("qpg_percode_select_guarded_f64", dev, D, D.stride(0), *tables, *track, float(self.tie_eps),
                      self._guard_stats, int(half))
        self._last_audio_mixed, self._last_audio_exact, self._last_audio_hl = mixed, plan.path == "exact", use_hl
        self._last_rank_cut, self._last_D_aud, self._last_q32, self._last_qn2 = plan.cut_top_n > 0, D, q32, qn2
        if mixed:
            self._last_mix_Q = Q
        return AudioResult(dist, idx, rank, D, q32, qn2, plan)

    def sweep_text(self, queries, want_rank=False, reduce=True, normalised=False, out=None, cols_packed=False, kind=None):
        """queries: f32 [Q,384] on the device (already sklearn-normalised if `normalised`).
        Returns (dist f32 [Q,512], idx i32 [Q,512][, rank]).  kind: what plan_text planned for this call (sweep_tables)."""
        db, dev = self.db, self.db.device
        Q = queries.shape[0]
        if normalised:
            qn = queries
        else:
            qn = torch.empty_like(queries)
            _lib.call("qpg_l2_normalize_rows_f32", dev, queries, Q, db.Dt, qn)
        if kind is None:
            kind = plan_text(self._knobs(), self._facts(), Q, reduce, out is not None)
        self._last_text_mfma = kind == "mfma"
        if kind == "mfma":
            # (row shard: straight into the exchange buffer, global indices, merged later; one GPU: idx_base is 0)
            dist, idx, rank, qb, bs = self._tables_out(Q, torch.float32, out, want_rank and out is None)
            db.txt_sorted.select(qn, float(ABSENT_DIST), self._guard_stats, dist=dist, idx=idx, rank=rank,
                                 idx_base=db.idx_base * db.Gt, q_block=qb, block_stride=bs, scratch=self._txt_scratch,
                                 cols_packed=cols_packed)
        else:
            D = torch.empty((Q, max(db.Ct, 1)), dtype=torch.float32, device=dev)
            _lib.call("qpg_text_cosine_f32", dev, db.ctxt, db.Ct, db.Dt, qn, Q, D, D.stride(0))
            dist, idx, rank = self._select_plain(D, db.txt_cand_code, db.Ct, db.Gt, out, want_rank and db.world == 1)
        return self._finish(dist, idx, rank, want_rank, reduce)

    def sweep_audio_wavvq(self, test_wavvq, q_win, q_t, want_rank=False, reduce=True, out=None):
        """vq-wav2vec audio sweep: test_wavvq (M,398,2) ints (device tensor or array).  Distances are exact
        small integers (Levenshtein), returned as f32 [Q,512] with the winners' global candidate indices."""
        db, dev = self.db, self.db.device
        tw = torch.as_tensor(test_wavvq).to(dev)
        sym_q = (tw[..., 0].to(torch.int64) * WAVVQ_GROUP_SIZE + tw[..., 1].to(torch.int64)).to(torch.int32).contiguous()
        Q = int(q_win.shape[0]) if isinstance(q_win, torch.Tensor) else len(q_win)
        C = db.n_local * db.Gv
        D = torch.empty((Q, max(C, 1)), dtype=torch.float32, device=dev)
        taps = (ctypes.c_int32 * len(db.vq_taps))(*db.vq_taps)
        _lib.call("qpg_wavvq_lev_f32", dev, db.vq_sym, db.n_local, db.Tv, db.vq_t, db.Gv, taps, len(db.vq_taps),
                  sym_q, sym_q.shape[0], sym_q.shape[1], _i32(q_win, dev), _i32(q_t, dev), Q, D, D.stride(0))
        dist, idx, rank = self._select_plain(D, db.vq_cand_code, C, db.Gv, out, want_rank and db.world == 1)
        self._last_D_aud = D
        return self._finish(dist, idx, rank, want_rank, reduce)

    def _reduce_min(self, dist, idx):
        """Cross-shard min + index: all-reduce(MIN) on the distances, then
        all-reduce(MIN) on the indices of the ranks that hold that minimum.  Shards are contiguous
        row blocks, so the lowest index == the reference's first-wins scan order."""
        if self.db.world == 1:
            return dist, idx
        return allreduce_min_index(dist, idx)

    def guard_stats(self):
        """(pairs re-evaluated in the reference's arithmetic so far, trouble flag) of the near-tie guard; the flag is
        set by a list overflow or, on the mixed-precision path, by operand norms small enough to void its error bound."""
        v = self._guard_stats.cpu().numpy()
        return int(v[0]), bool(v[1])

    def mixed_stats(self):
        """Mixed-precision audio path: pairs re-evaluated with an f64 dot product so far (tier 1), pairs re-evaluated
        in the reference's arithmetic (tier 2), raw flag word (1 = list overflow, 2 = norms below the bound's range)."""
        v = self._guard_stats.cpu().numpy()
        return {"tier1_pairs": int(v[2]), "tier2_pairs": int(v[0]), "flags": int(v[1])}

    def tier1_list_lengths(self):
        """Entries of every query's tier-1 re-evaluation list in the last mixed-precision select (capacity 2048 each):
        read back from the select's workspace.  Diagnostics (bench.py --data speechlike, tests): what the caps see."""
        ws, Q = self._mix_ws, self._last_mix_Q
        if ws is None or not Q:
            return np.zeros((0,), np.int64)
        K = self.db.K
        stride = int(_lib.load().qpg_percode_select_mixed_ws_stride(K))
        w = ws[:Q * stride].view(Q, stride)[:, 24 * K:24 * K + 4].contiguous().view(torch.int32)
        return w.cpu().numpy().reshape(-1).astype(np.int64)

    def clear_flags(self):
        self._guard_stats[1:2].zero_()

    @staticmethod
    def numpy_ranks(dist, idx=None, integer=False):
        """The reference's rank expression (GestureKNN.py:553, 574) on the host: np.array(list).argsort().argsort().
        The dtype of that array is part of the tie behaviour (NumPy's sort kernels differ per dtype) and follows from
        what the list holds: the `1e+3` placeholders are Python floats, the distances NumPy scalars of the metric's
        dtype (np.float64 audio, np.float32 text, Python ints for the Levenshtein audio).  So a row in which EVERY code
        has a candidate is sorted in the distances' own dtype (float32 text, int64 wavvq), and a row with an absent
        code as float64 - reproduced here row by row (`idx` < 0 marks absent codes; `integer`: Levenshtein row)."""
        d = dist.detach().cpu().numpy()
        present = None if idx is None else (idx.detach().cpu().numpy() >= 0)
        out = np.empty(d.shape, np.int16)
        for r_, row in enumerate(d):
            full = present is not None and bool(present[r_].all())
            if full and integer:
                arr = np.array([int(x) for x in row])                    # list of Python ints -> int64
            elif full:
                arr = np.array(list(row))                                # list of np.float32 / np.float64 scalars
            else:
                arr = np.array(list(row.astype(np.float64)))             # a Python float in the list: float64
            out[r_] = arr.argsort().argsort()
        return torch.from_numpy(out).to(dist.device)

    def rank_rows(self, dist):
        out = torch.empty(dist.shape, dtype=torch.int16, device=dist.device)
        name = "qpg_rank_rows_f64" if dist.dtype == torch.float64 else "qpg_rank_rows_f32"
        _lib.call(name, self.db.device, dist.contiguous(), dist.shape[0], dist.shape[1], out)
        return out

    # -- reference-shaped single-query API (GestureKNN.py:666-691, 708-721) --------------------------
    def _unpack(self, dist, idx, G, ks, cidx):
        d = dist[0].cpu().numpy()
        ix = idx[0].cpu().numpy()
        code = self.db.code_host
        dists, pays, aux = [], [], []
        for c in range(self.db.K):
            if ix[c] < 0:
                dists.append(ABSENT_DIST)
                pays.append([])
                aux.append([])
            else:
                j, g = divmod(int(ix[c]), G)
                dists.append(d[c])
                pays.append(code[j, cidx[g]:cidx[g] + STEP_SZ])
                aux.append([j, ks[g]])
        return dists, pays, aux

    def search_audio_cands(self, clip_input, mode="wavlm_feat"):
        """clip_input: one 6144-d WavLM feature row (6 taps x 1024).  Same return triple as the
        reference: per-code distance list, per-code 4-code payload (or []), per-code [j, k] (or [])."""
        db = self.db
        if mode == "wavvq_feat":
            # clip_input: 22 numbers = 11 taps x (g1,g2) (data_processing.py:317); hand them to the kernel as a
            # 1-window track whose tap gather reproduces exactly those 11 symbols
            v = np.asarray(clip_input).reshape(11, 2).astype(np.int64)
            track = np.zeros((1, db.Tv, 2), np.int64)
            t0 = -min(db.vq_taps)
            for i, off in enumerate(db.vq_taps):
                track[0, t0 + off] = v[i]
            dist, idx = self.sweep_audio_wavvq(track, [0], [t0])
            return self._unpack(dist, idx, db.Gv, db.vq_k, db.vq_cidx_host)
        if mode != "wavlm_feat":
            raise NotImplementedError(mode)
        q = torch.as_tensor(np.asarray(clip_input, np.float32).reshape(1, NUM_AUDIO_FEAT_FRAMES, db.F),
                            device=db.device).contiguous()
        dist, idx = self.sweep_audio(q, [0], [0], tap_stride=1)
        return self._unpack(dist, idx, db.Ga, db.aud_k, db.aud_cidx_host)

    def search_text_cands(self, clip_input, mode="wavvq_feat"):
        db = self.db
        q = torch.as_tensor(np.asarray(clip_input, np.float32).reshape(1, db.Dt), device=db.device).contiguous()
        dist, idx = self.sweep_text(q)
        return self._unpack(dist, idx, db.Gt, db.txt_k, db.txt_rows_host)

    # -- whole clip ---------------------------------------------------------------------------------
    def n_steps(self):
        return len(self.query_positions())

    def _query_index(self, M):
        """(window, frame, context row) of every query of M windows: device tensors, built once per clip length (also
        keeps H2D copies out of graphs)."""
        if M not in self._qcache:
            pos, dev = self.query_positions(), self.db.device
            qw = np.repeat(np.arange(M), len(pos))
            qt = np.tile(np.array([int(i) for i in pos]), M)                  # clip_test[int(i)]  (:559, :565)
            rows_ = [int(i / self.n_db_frm * 30) for i in pos] * M           # GestureKNN.py:549, 551
            self._qcache[M] = (_i32(qw, dev), _i32(qt, dev), _i32(np.asarray(rows_), dev))
        return self._qcache[M]

    def _fork_side(self):
        """The side stream, started behind everything enqueued on the current stream so far."""
        dev = self.db.device
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(dev)
            # (wait_stream() makes a new event per call; two cached events do the same for ~5 us less host time per
            # clip, most of it in front of the step's first launch)
            self._side_gate, self._side_done = torch.cuda.Event(), torch.cuda.Event()
            self._sweep_event = torch.cuda.Event()          # (the end of the audio sweep: re-recorded by every clip)
        if dev.index is None or dev.index == torch.cuda.current_device():
            self._side_gate.record()            # (the current stream: no Stream object in front of the step's launches)
        else:
            self._side_gate.record(torch.cuda.current_stream(dev))
        self._side_stream.wait_event(self._side_gate)
        return self._side_stream

    def _clip_pack(self, test_interp, test_context, q_win, q_t, q_row, Q):
        """The clip's WHOLE query side in one launch (qpg_clip_pack_hl: the audio gather / norms / split-f16 image AND
        the text queries' gather / sklearn normalisation / column image) -> (q32, qn2, qn).  Behind the 32-row sweep,
        which holds every register of every CU, two separate text packs would not get a wave slot before it is over."""
        db, dev = self.db, self.db.device
        q32 = torch.empty((Q, NUM_AUDIO_FEAT_FRAMES * db.F), dtype=torch.float32, device=dev)
        qn2 = torch.empty((Q,), dtype=torch.float64, device=dev)
        qi = self._hl_qimage = _grown(self._hl_qimage, int(_lib.load().qpg_audio_hl_query_bytes(Q, db.F)), dev)
        qn = torch.empty((Q, db.Dt), dtype=torch.float32, device=dev)
        cols = db.txt_sorted.cols_buffer(Q, self._txt_scratch)
        tc, ti = test_context.contiguous(), test_interp.contiguous()
        _lib.call("qpg_clip_pack_hl", dev, ti, ti.shape[0], db.T, db.F, q_win, q_t, Q, NUM_AUDIO_FEAT_FRAMES,
                  db.tap_stride, q32, qn2, qi, qi.numel(), tc, tc.shape[0], tc.shape[1], db.Dt, q_win, q_row, Q, qn, cols,
                  cols.numel())
        return q32, qn2, qn

    def sweep_tables(self, test_interp, test_context, n_windows, mode=MODE_AUD_TXT, owner_blocks=False, for_walk=False,
                     after_sweep=None):
        """Both batched sweeps + ranks for all Q = n_windows*steps query positions (the windows may
        belong to several clips).  test_interp: f32 [M,180,F]; test_context: f32 [M,30,384] (device).
        Returns a dict of device tensors: aud_d/aud_idx/aud_rank, txt_d/txt_idx/txt_rank.
        owner_blocks (sharded DB only): the windows are `world` equal blocks and this rank only needs the final
        tables of block `rank` — one all-to-all instead of two all-reduces; the returned tables then hold only that
        block's Q/world rows.
        for_walk: the tables go straight into walk() and nowhere else - the audio select may then leave unsettled what the
        walk can not read (CodeKNN.rank_cut; the returned tables are exact only where the walk reads them).
        after_sweep: called directly behind the WavLM audio sweep kernel's launch (ClipGraph forks its encode leg /
        raises its sweep signal there); the wavvq sweep does not call it."""
        db, dev = self.db, self.db.device
        M, steps = n_windows, self.n_steps()
        if test_interp.shape[0] < M or (mode != MODE_AUD and test_context.shape[0] < M):
            # the reference indexes test_wavlm_feat[i] / test_context[i] for i < n_test_seq (GestureKNN.py:788-800)
            raise IndexError("n_windows=%d but the test arrays hold %d audio / %d context windows"
                             % (M, test_interp.shape[0], test_context.shape[0]))
        want = (db.Tv, 2) if self.use_wavvq else (db.T, db.F)
        if tuple(test_interp.shape[1:]) != want:
            raise ValueError("test audio windows have shape %s, database expects %s"
                             % (tuple(test_interp.shape[1:]), want))
        q_win, q_t, q_row = self._query_index(M)
        Q = M * steps
        key = (self._knobs(), self._facts(), M, steps, mode, for_walk, owner_blocks)     # (every value the plan reads)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = plan_step(*key)
        sharded = plan.sharded
        T = dict(aud_d=None, aud_idx=None, aud_rank=None, txt_d=None, txt_idx=None, txt_rank=None)
        # split fusion: the rank fusion in front of the walk is two independent argmins (audio order, text order:
        # GestureKNN.py:574-576, :553-555) - each side's half goes out behind its own select on its own stream
        # (qpg_fuse_best_ranked) into the walk's gate tables, which the walk then takes as they are (QPG_MODE_PREFUSED)
        gtab = torch.empty((3, max(M, 1) * steps, db.K), dtype=torch.int32, device=dev) if plan.split_fuse else None
        # sharded: the per-shard tables go straight into the exchange buffer (ExchangeLayout)
        lay = self._layout(Q, owner_blocks, mode) if sharded else None
        # The two sweeps are independent until the walk: with both modalities on, the text side runs on a second HIP
        # stream beside the audio side
        side = self._fork_side() if plan.overlap else None
        packed = None
        if plan.clip_pack:
            packed = self._clip_pack(test_interp, test_context, q_win, q_t, q_row, Q)
            self._side_gate.record(torch.cuda.current_stream(dev))          # the side stream starts BEHIND the pack
            side.wait_event(self._side_gate)

        def keep(p_, g, r):          # a side's tables + its half of the rank fusion, on the stream its select ran on
            T[p_ + "_d"], T[p_ + "_idx"], T[p_ + "_rank"] = r[0], r[1], (None if sharded else r[2])
            if gtab is not None:
                _lib.call("qpg_fuse_best_ranked", dev, r[2], r[1], db.pos_rank, db.freq_rank, Q, db.K, gtab[g])

        def text_pack():
            # gather clip_context[int(i/n*30)] of every step + sklearn normalisation in one launch
            tc = test_context.contiguous()
            qn = torch.empty((Q, db.Dt), dtype=torch.float32, device=dev)
            _lib.call("qpg_text_pack_queries_f32", dev, tc, tc.shape[0], tc.shape[1], db.Dt, q_win, q_row, Q, qn)
            return qn

        def text_side(qn=None):
            if packed is not None:
                qn = packed[2]
            elif qn is None:
                qn = text_pack()
            keep("txt", 1, self.sweep_text(qn, want_rank=not sharded, reduce=not sharded, normalised=True,
                                           out=lay.views("txt") if sharded else None, cols_packed=packed is not None,
                                           kind=plan.text))

        # The planned order of the two sides (DESIGN.md section 4.2 has the measurements): "text_first": the text side is
        # enqueued first; "text_after_sweep": audio side first, the text side waits on its stream for the END of the
        # audio sweep and fills the CUs the audio select leaves idle; "audio_first": audio side first, no ordering
        # between the streams - the text GEMM trickles through under the sweep.
        if plan.order == "text_first":
            with torch.cuda.stream(side):
                text_side()
        aud = None
        if mode != MODE_TXT:
            out = lay.views("aud") if sharded else None
            if self.use_wavvq:
                r = self.sweep_audio_wavvq(test_interp, q_win, q_t, want_rank=not sharded, reduce=not sharded, out=out)
            else:
                aud = self._sweep_audio(plan.audio, test_interp, q_win, q_t, out=out, prepacked=packed,
                                        sweep_event=self._sweep_event if plan.order == "text_after_sweep" else None,
                                        after_sweep=after_sweep)
                r = self._finish(aud.dist, aud.idx, aud.rank, not sharded, not sharded)
            keep("aud", 0, r)
        if plan.order == "text_after_sweep":
            with torch.cuda.stream(side):
                qn_early = None if packed is not None else text_pack()    # one small block, next to the audio sweep
                side.wait_event(self._sweep_event)
                text_side(qn_early)
        elif plan.order == "audio_first":
            with torch.cuda.stream(side):
                text_side()
        if plan.overlap:
            self._side_done.record(side)
            torch.cuda.current_stream(dev).wait_event(self._side_done)
            # The text tables are allocated on `side` and consumed on `main`.  No record_stream() (measured +15 us per
            # clip for the allocator's events): a freed block can only be reused by a later `side` allocation, and every
            # use of `side` starts by waiting for `main` above, i.e. after main's consumers of the block.
        elif mode != MODE_AUD:
            text_side()
        if sharded:
            self._merge_shards(lay, owner_blocks, T, aud)
        if self.host_ranks:
            for p_ in ("aud", "txt"):
                if T[p_ + "_d"] is not None:
                    T[p_ + "_rank"] = self.numpy_ranks(T[p_ + "_d"], T[p_ + "_idx"],
                                                       integer=(p_ == "aud" and self.use_wavvq))
        if gtab is not None:
            T["gate_tables"] = gtab         # [0], [1]: both modalities' candidates for every (step, previous code)
        return T

    def _layout(self, Q, owner_blocks, mode):
        """The ExchangeLayout (+ send buffer) of this shape: one per shape, reused by every clip (stream-ordered: the
        previous clip's exchange has read it)."""
        parts = tuple(p_ for p_, off in (("aud", MODE_TXT), ("txt", MODE_AUD)) if mode != off)
        key = (Q, self.db.world if owner_blocks else 1, parts, not self.use_wavvq)
        if key not in self._layouts:
            self._layouts[key] = ExchangeLayout(key[0], self.db.K, key[1], parts, key[3], self.db.device)
        return self._layouts[key]

    def _merge_shards(self, lay, owner_blocks, T, aud):
        """The sharded step's second half: ONE collective for both modalities (all-to-all when every rank only needs its
        own clip's rows, all-gather otherwise), then one merge launch per modality into T: min distance, lowest global
        index among equals, ranks.  The trouble word rides in the blocks (ExchangeLayout "flags"): stamped here, ORed in
        by the receivers.  aud: the AudioResult of this rank's WavLM sweep (None: wavvq or no audio side)."""
        db, dev = self.db, self.db.device
        _lib.call("qpg_flags_stamp", dev, lay.send, lay.nblk, lay.block_bytes, lay.off["flags"], self._guard_stats)
        recv = exchange_bytes(lay.send, db.world, owner_blocks)
        src_stride = lay.block_bytes if owner_blocks else lay.send.numel()
        gathered = False
        for p_ in lay.parts:
            d = torch.empty((lay.Qb, db.K), dtype=lay.dtype[p_], device=dev)
            ix = torch.empty((lay.Qb, db.K), dtype=torch.int32, device=dev)
            rk = torch.empty((lay.Qb, db.K), dtype=torch.int16, device=dev)
            wavlm_aud = p_ == "aud" and aud is not None
            if wavlm_aud and aud.plan.path in ("mixed", "exact"):
                self._merge_mixed(recv, src_stride, lay, owner_blocks, d, ix, rk, aud.q32, aud.qn2, aud.plan)
                gathered = True
            elif lay.dtype[p_] == torch.float64:
                # (f64 sweep + capped guard per shard: near-ties ACROSS shards / codes are detected here and
                # re-matched on the exact path; exact integer distances of the wavvq mode need no guard)
                guard = wavlm_aud and self.tie_eps > 0
                _lib.call("qpg_merge_select_f64", dev, recv, db.world, src_stride, lay.off[p_ + "_d"],
                          lay.off[p_ + "_i"], lay.Qb, db.K, float(ABSENT_DIST), d, ix, rk,
                          float(self.tie_eps) if guard else 0.0, self._guard_stats if guard else None)
            else:
                _lib.call("qpg_merge_select_f32", dev, recv, db.world, src_stride,
                          lay.off[p_ + "_d"], lay.off[p_ + "_i"], lay.Qb, db.K, float(ABSENT_DIST), d, ix, rk)
            T[p_ + "_d"], T[p_ + "_idx"], T[p_ + "_rank"] = d, ix, rk
        if not gathered:            # (the mixed merge's prologue ORs the received words in itself)
            _lib.call("qpg_flags_gather", dev, recv, db.world, src_stride, lay.off["flags"], self._guard_stats)
        # Every rank must take the same decision about a re-match (it is a collective path).  Bits raised BEFORE an
        # exchange reach every rank with it.  In the all-gather form every rank then runs the same merge on the same
        # bytes, so the bits the merge itself raises (cross-shard near-ties) are the same everywhere: no collective.
        # In the all-to-all form each owner merges its own query block: those last bits still take a 4-byte MAX
        # all-reduce, on the device, stream-ordered - the walk carries the agreed value out with the codes.
        if owner_blocks:
            allreduce_max_(self._guard_stats[1:2], force=self.force_sharded)

    def _merge_mixed(self, recv, src_stride, lay, owner_blocks, d, ix, rk, q32, qn2, plan):
        """Cross-shard merge of audio tables whose comparisons are not all decided by their values:
        approximate merge + requests, re-evaluation of the requested pairs where the rows live (from this rank's packed
        queries q32 / qn2), final merge + ranks.  plan: the AudioPlan the tables were made by.
        Request slots are deterministic (qpg_merge_mixed_phase1_f64), so:
          all-gather form (every rank holds every shard's tables and runs the same merge): a shard refines ITS block of
            its OWN phase-1 run - no request exchange; ONE all-gather of the responses.  Two collectives per clip in all.
          all-to-all form (every rank owns one query block): the owner's requests travel to the shards and the responses
            back: two more all-to-alls.
        Mixed-precision tables: band = 2.1 x the sweep's bound, responses = f64 dot-product distances; what those leave
        within tie_eps raises FLAG_CROSS_SHARD_TIE.  Path "exact" (f64 tables of the uncapped select): band = tie_eps,
        responses in the reference's own arithmetic, request and flag lists sized for the worst case - the cross-shard
        tier 2, which cannot overflow and flags nothing."""
        db, dev = self.db, self.db.device
        W, Qb, K = db.world, lay.Qb, db.K
        exact = plan.path == "exact"
        if exact:
            Rq, fl_cap, band = K, K * W, float(self.tie_eps)
        else:
            # slots per (query, shard): ~70 / W requests per query are usual with the split-f16 band
            Rq = int(self.mixed_requests) if self.mixed_requests else max(64, 512 // W)
            fl_cap, band = 1024, plan.band
        R = Qb * Rq
        req_stride = resp_stride = 8 + 8 * R
        key = (exact, W, R)
        bufs = self._mm_cache.get(key)
        need_ws = int(_lib.load().qpg_merge_mixed_ws_bytes(Qb, K, fl_cap))
        if bufs is None or bufs[2].numel() < need_ws:
            bufs = self._mm_cache[key] = (torch.empty((W * req_stride,), dtype=torch.uint8, device=dev),
                                          torch.empty((W * resp_stride,), dtype=torch.uint8, device=dev),
                                          torch.empty((need_ws,), dtype=torch.uint8, device=dev))
        req, resp, ws = bufs
        _lib.call("qpg_merge_mixed_phase1_f64", dev, recv, W, src_stride, lay.off["aud_d"], lay.off["aud_i"], Qb, K,
                  float(ABSENT_DIST), band, R, req, req_stride, ws, ws.numel(), self._guard_stats, fl_cap,
                  lay.off["flags"])
        half = int(db.feature_dtype == "f16")
        refine = (db.idx_base * db.Ga, db.base, half, db.T, db.F, db.aud_t, db.Ga, NUM_AUDIO_FEAT_FRAMES, db.tap_stride,
                  q32, qn2, db.cn2, resp, resp_stride, int(exact), self._guard_stats, Rq)
        if owner_blocks:
            req_recv = exchange_bytes(req, W, True)
            # block o of req_recv comes from owner o: its queries are rows o*Qb .. of this rank's packed query set
            _lib.call("qpg_shard_refine_f64", dev, req_recv, W, req_stride, R, Qb, *refine)
            resp_recv = exchange_bytes(resp, W, True)
        else:
            # every rank ran the same phase 1: block `rank` of MY request buffer is what owner(s) would have sent me
            mine = req[db.rank * req_stride:(db.rank + 1) * req_stride]
            _lib.call("qpg_shard_refine_f64", dev, mine, 1, req_stride, R, 0, *refine)
            resp_recv = exchange_bytes(resp[:resp_stride], W, False)
        _lib.call("qpg_merge_mixed_phase2_f64", dev, recv, W, src_stride, lay.off["aud_i"], Qb, K, float(ABSENT_DIST), ws,
                  ws.numel(), resp_recv, resp_stride, d, ix, rk, self._guard_stats, fl_cap,
                  0.0 if exact else float(self.tie_eps))

    # -- the walk ------------------------------------------------------------------------------------
    def _seed_phase_tensor(self, seed_phase):
        if isinstance(seed_phase, torch.Tensor):
            return seed_phase.to(self.db.device, torch.float32).contiguous()
        return torch.as_tensor(np.asarray(seed_phase, np.float32), device=self.db.device).contiguous()

    def _walk_args(self, T, q0, Qt, rows, mode, prefusable):
        """The arguments every walk over table rows [q0, q0 + Qt) starts with (the mode word, M, steps and K follow them),
        the gate tables to use and the mode word.  The tables' own gate tables are taken as they are (QPG_MODE_PREFUSED)
        when they cover exactly these rows and `prefusable`; otherwise the walk fuses the ranks itself into a scratch
        table of `rows` rows."""
        db = self.db
        gate = T.get("gate_tables")
        prefused = prefusable and gate is not None and mode == MODE_AUD_TXT and gate.shape[1] == Qt
        if not prefused:
            gate = torch.empty((3, rows, db.K), dtype=torch.int32, device=db.device)
        a_cidx, a_pslot, a_G = self._audio_grid()
        tabs = [None if T[k] is None else T[k][q0:q0 + Qt] for k in ("aud_rank", "aud_idx", "txt_rank", "txt_idx")]
        head = (*tabs, db.pos_rank, db.freq_rank, db.code, db.code.shape[1], a_cidx, a_pslot, a_G, db.txt_cidx,
                db.txt_pslot, db.Gt, db.phase, db.Tp)
        return head, gate, mode | (_lib.QPG_MODE_PREFUSED if prefused else 0)

    def _launch_walk(self, T, q0, Qt, rows, mode, prefusable, M, steps, seed, sp, outs, chains=None):
        """The walk over table rows [q0, q0 + Qt): qpg_match_steps (chains None; seed: the seed code) or
        qpg_match_steps_batch (`chains` independent clips back to back; seed: their i32 seed codes in device-readable
        memory).  sp: the f32 [8][16] seed phase block(s); outs = (codes, phases, votes, status).  Returns _walk_args' gate."""
        db, dev = self.db, self.db.device
        head, gate, mode_w = self._walk_args(T, q0, Qt, rows, mode, prefusable)
        if chains is None and self.serial_walk:
            mode_w |= _lib.QPG_MODE_SERIAL_WALK
        guard = self._guard_stats[1:2]
        if chains is None:
            _lib.call("qpg_match_steps", dev, *head, mode_w, M, steps, db.K, seed, sp, gate, *outs, guard)
        else:
            _lib.call("qpg_match_steps_batch", dev, *head, mode_w, M, steps, db.K, chains, seed, sp, gate, *outs, 2, guard)
        return gate

    def draw_coins(self, n):
        """The coins of n matching steps of a no-phase clip: `np.random.rand() > 0.5` per step (GestureKNN.py:581) - n
        successive draws from the matcher's rng, True = the audio candidate."""
        return np.asarray(self.rng.rand(int(n))).reshape(-1) > 0.5

    def _refuse_nophase(self, what):
        if not self.use_phase:
            raise NotImplementedError("%s is not implemented for a matcher without the phase gate (use_phase=False): "
                                      "match_clip / walk are" % what)

    def _walk_nophase(self, T, n_windows, window_offset, mode, seed_code, coins):
        """walk() of a matcher without the phase gate: qpg_match_steps_nophase over the tables' rows (two launches).  The
        seed code and the coins are read from, and the integer results written to, ONE pinned host buffer (zero-copy; the
        status pair is the walk's last store).  -> (codes int64 [M, 30], phases f32 [M, 0, 8, 16], sides i32 [M, steps]);
        last_picks = the appended candidates i32 [M, steps]."""
        db, dev = self.db, self.db.device
        M, steps, K = int(n_windows), self.n_steps(), self.db.K
        plan = plan_nophase(self._knobs(), self._facts(), M, steps, mode, self.desired_k)
        if plan.path != "kernel":
            raise NotImplementedError(plan.reason)
        Q, cpw = M * steps, min(4 * steps, num_frames_code)
        if seed_code is None:
            seed_code = self.init_code_phase()
        if not 0 <= int(seed_code) < K:
            raise ValueError("seed code %r outside [0, %d)" % (seed_code, K))
        if mode == MODE_AUD_TXT:
            if coins is None:
                coins = self.draw_coins(Q)
            coins = np.asarray(coins).reshape(-1) != 0
            if coins.size != Q:
                raise ValueError("coins: one per matching step (%d), got %d" % (Q, coins.size))
        n_in, n_out = 1 + (Q + 3) // 4, M * cpw + 2 * Q + 2           # seed | coins (u8) || codes | sides | cands | status
        pin = self._pinned_nophase              # ONE pinned buffer, grown to the longest clip seen (this call drains it)
        if pin is None or pin.numel() < n_in + n_out:
            pin = self._pinned_nophase = torch.empty((n_in + n_out,), dtype=torch.int32).pin_memory()
        pin_np = pin.numpy()
        pin_np[0] = int(seed_code)
        if mode == MODE_AUD_TXT:
            pin_np[1:n_in].view(np.uint8)[:Q] = coins
        out_np = pin_np[n_in:n_in + n_out]
        out_np.fill(_PIN_SENTINEL)
        base = pin.data_ptr()
        o_codes = base + 4 * n_in
        o_side, o_cand, o_status = o_codes + 4 * M * cpw, o_codes + 4 * (M * cpw + Q), o_codes + 4 * (M * cpw + 2 * Q)
        ws = self._nophase_ws = _grown(self._nophase_ws,
                                       int(_lib.load().qpg_match_steps_nophase_ws_bytes(1, max(M, 1), steps, K)), dev)
        q0 = window_offset * steps
        tabs = [None if T[k] is None else T[k][q0:q0 + Q] for k in ("aud_rank", "aud_idx", "txt_rank", "txt_idx")]
        a_cidx, _, a_G = self._audio_grid()
        _lib.call("qpg_match_steps_nophase", dev, *tabs, db.pos_rank, db.freq_rank, db.code, db.code.shape[1], a_cidx, a_G,
                  db.txt_cidx, db.Gt, mode, self.desired_k, M, steps, K, 1, base, base + 4 if mode == MODE_AUD_TXT else None,
                  o_codes, o_side, o_cand, o_status, 2, self._guard_stats[1:2], ws, ws.numel())
        ints = _wait_pinned(out_np, torch.cuda.current_stream(dev))
        self.check_status(ints[-2:])
        self.last_picks = ints[M * cpw + Q:M * cpw + 2 * Q].reshape(M, steps).copy()
        codes = ints[:M * cpw].reshape(M, cpw).astype(np.int64)
        return codes, np.zeros((M, 0, 8, 16), np.float32), ints[M * cpw:M * cpw + Q].reshape(M, steps).copy()

    def walk(self, T, n_windows, window_offset=0, mode=MODE_AUD_TXT, seed_code=None, seed_phase=None, sync=True,
             seed_ptrs=None, out_pin=None, n_chains=1, coins=None):
        """Device-side walk of windows [window_offset, window_offset+n_windows) of the tables.
        sync=True: (codes, phases, votes) as NumPy arrays; sync=False: device tensors (+ the status pair), nothing waited
        for, `_last_ints` = codes | votes | status on the device; sync="ints": the integer results only, as ONE host array
        codes | votes | status - the walk's last kernel writes them straight into pinned host memory (zero-copy) and the
        stream is synchronised: no D2H copy launch behind the walk (bench.py's step; ~5 us of a 0.33 ms clip).
        seed_ptrs = (address of an i32 seed code, address of its f32 [8][16] phase block), both readable by the device
        (ClipGraph: pinned host memory the host rewrites before every replay - the seed is then DATA, not a kernel
        argument, and one captured graph serves every clip); out_pin: a pinned int32 tensor [M*30 + M*steps + 2] the
        integer results go to (with sync=False: nothing is waited for).
        n_chains > 1 (with seed_ptrs and out_pin: ClipGraph over several clips): that many INDEPENDENT clips of n_windows
        windows whose steps sit back to back in the tables from window_offset on; seed_ptrs then address i32 [n_chains]
        seed codes and f32 [n_chains][8][16] phase blocks, out_pin holds codes [n_chains][M*30] | votes [n_chains][M*steps]
        | status [n_chains][2]."""
        db, dev = self.db, self.db.device
        M, steps = n_windows, self.n_steps()
        CL = int(n_chains)
        if not self.use_phase:
            # (GestureKNN.py:578-592: coins [M * steps], True / nonzero = the audio candidate; drawn here if not given)
            if sync is not True or seed_ptrs is not None or out_pin is not None or CL != 1:
                self._refuse_nophase("walk(sync=%r, seed_ptrs, out_pin, n_chains)" % (sync,))
            return self._walk_nophase(T, n_windows, window_offset, mode, seed_code, coins)
        assert CL == 1 or (seed_ptrs is not None and out_pin is not None), "several chains: the graph path only"
        if seed_ptrs is not None:
            sp = int(seed_ptrs[1])
        else:
            if seed_code is None:
                seed_code, seed_phase = self.init_code_phase()
            sp = self._seed_phase_tensor(seed_phase)
        # codes | votes | status (2) in ONE buffer: the integer results leave in a single D2H copy, no gather kernel
        # before it.  status[0] = an absent code won a rank fusion, status[1] = the sweeps' / selects' trouble word
        # (copied by the walk's last kernel from _guard_stats[1]): a clip whose word is not 0 is never returned.
        n_c, n_v = M * num_frames_code, M * steps
        host = sync is True or sync == "ints"
        if out_pin is not None or host:
            pin = out_pin
            if pin is None:
                # pinned (device-visible) host memory, one buffer per clip length: safe to reuse because this call does
                # not return before the stream has drained and the values have been copied out of it
                if M not in self._pinned_ints:
                    self._pinned_ints[M] = torch.empty((n_c + n_v + 2,), dtype=torch.int32).pin_memory()
                pin = self._pinned_ints[M]
                # every word is a sentinel until the walk has written it; the status word is the walk's LAST store (behind
                # a system-scope fence), the others are checked as well before the buffer is copied (_wait_pinned)
                pin_np = pin.numpy()
                pin_np.fill(_PIN_SENTINEL)
            assert not (host and out_pin is not None) and pin.numel() >= CL * (n_c + n_v + 2)
            base = pin.data_ptr()
            out_codes, out_vote, status = base, base + 4 * CL * n_c, base + 4 * CL * (n_c + n_v)
        else:
            ints_d = torch.empty((n_c + n_v + 2,), dtype=torch.int32, device=dev)
            out_codes = ints_d[:n_c].view(M, num_frames_code)
            out_vote = ints_d[n_c:n_c + n_v].view(M, steps)
            status = ints_d[n_c + n_v:]                                  # always written by the walk kernels
        out_phase = torch.empty((CL * M, steps, 8, 16), dtype=torch.float32, device=dev)
        q0 = window_offset * steps
        outs = (out_codes, out_phase, out_vote, status)
        prefusable = q0 == 0 and M > 0 and not self.serial_walk
        if seed_ptrs is not None:           # through the batch entry: the seed codes are read from memory by the kernels
            self._launch_walk(T, q0, CL * M * steps, max(CL * M, 1) * steps, mode, prefusable, M, steps,
                              int(seed_ptrs[0]), sp, outs, chains=CL)
        else:
            self._launch_walk(T, q0, M * steps, max(M, 1) * steps, mode, prefusable, M, steps, int(seed_code), sp, outs)
        if out_pin is not None:
            return out_codes, out_phase, out_vote, status
        if not host:
            self._last_ints = ints_d
            return out_codes, out_phase, out_vote, status
        if sync == "ints":
            # the host watches the last word instead of sleeping in hipStreamSynchronize (~3.5 us sooner per clip); after
            # ~2 ms without it (a failed launch would never write it) the stream is synchronised the ordinary way
            return _wait_pinned(pin_np, torch.cuda.current_stream(dev))
        phases = out_phase.cpu().numpy()                    # (synchronises the stream: the pinned integers are complete)
        ints = pin.numpy().copy()
        self.check_status(ints[n_c + n_v:])
        codes = ints[:n_c].reshape(M, num_frames_code).astype(np.int64)
        votes = ints[n_c:n_c + n_v].reshape(M, steps).copy()
        return codes, phases, votes

    def walk_batch(self, T, n_windows, n_clips, seed_codes, seed_phases, mode=MODE_AUD_TXT):
        """Device-side walk of n_clips INDEPENDENT clips of n_windows windows each, whose steps sit back to back in the
        tables (one batched sweep: bench.py --clips 16, BASELINE configs[4]), in one set of launches
        (qpg_match_steps_batch).  seed_codes: ints [n_clips]; seed_phases: f32 [n_clips][8][16] (array or device tensor).
        Returns the device tensors (codes i32 [n_clips][M][30], phases f32 [n_clips][M][steps][8][16], votes i32
        [n_clips][M][steps]) and leaves `_last_ints` = i32 [n_clips][M*30 + M*steps + 2] (codes | votes | status per clip:
        ONE D2H copy)."""
        db, dev = self.db, self.db.device
        M, steps, CL = n_windows, self.n_steps(), int(n_clips)
        seeds = np.asarray(seed_codes, np.int64).reshape(-1)
        if seeds.shape[0] != CL or (seeds < 0).any() or (seeds >= db.K).any():
            raise ValueError("walk_batch: one seed code in [0, %d) per clip" % db.K)
        sc = torch.as_tensor(seeds.astype(np.int32), device=dev)
        sp = self._seed_phase_tensor(seed_phases)
        if sp.numel() != CL * 128:
            raise ValueError("walk_batch: seed_phases must hold [n_clips][8][16] floats")
        n_c, n_v = M * num_frames_code, M * steps
        status_d = torch.empty((CL, 2), dtype=torch.int32, device=dev)
        codes_d = torch.empty((CL, M, num_frames_code), dtype=torch.int32, device=dev)
        votes_d = torch.empty((CL, M, steps), dtype=torch.int32, device=dev)
        out_phase = torch.empty((CL, M, steps, 8, 16), dtype=torch.float32, device=dev)
        Qt = CL * M * steps
        gate = self._launch_walk(T, 0, Qt, Qt, mode, True, M, steps, sc, sp, (codes_d, out_phase, votes_d, status_d),
                                 chains=CL)
        self._last_ints = torch.cat((codes_d.view(CL, n_c), votes_d.view(CL, n_v), status_d), dim=1)
        self._last_gate_tables = gate                       # (tests compare the candidate tables of the two fusion paths)
        return codes_d, out_phase, votes_d

    def walk_takes(self, T, n_windows, seed_codes, seed_phases, mode=MODE_AUD_TXT, window_offset=0, sync=True,
                   seed_ptrs=None, out_pin=None, n_takes=None):
        """Windows [window_offset, window_offset + n_windows) of the tables walked from SEVERAL seeds in one set of launches
        (qpg_match_steps_takes; takes.py).  T: any dict sweep_tables returns on one GPU (for_walk or not,
        host_ranks, the wavvq sweep).  seed_codes: ints [S]; seed_phases: f32 [S][8][16].
        sync=True: (codes int64 [S, M, 30], phases f32 [S, M, steps, 8, 16], votes i32 [S, M, steps]) as NumPy arrays, every
        take's status checked (GuardOverflow; IndexError naming the take); sync=False: the device tensors + status [S][2],
        nothing waited for.  Take s is what walk() returns for seed s.  Which route is taken - the multi-take kernels or S
        calls of walk() - is plan_takes' decision; a row-sharded database raises NotImplementedError.
        seed_ptrs / out_pin / n_takes (ClipGraph): seeds read from, integer results written to pinned host memory, in
        walk()'s several-chains layout with takes in the place of clips."""
        from . import takes
        self._refuse_nophase("walk_takes")
        return takes.walk_takes(self, T, n_windows, seed_codes, seed_phases, mode, window_offset, sync, seed_ptrs, out_pin,
                                n_takes)

    def match_clip_takes(self, test_interp, test_context, n_windows, n_takes=None, seed_codes=None, seed_phases=None,
                         mode=MODE_AUD_TXT):
        """One clip from several seeds: ONE sweep, one walk_takes.  Seeds not given: n_takes successive init_code_phase()
        draws from the matcher's rng - take s is then what the s-th of n_takes successive match_clip calls on this clip
        returns, and the rng ends in the same state.  A raised trouble word re-matches the tables once, by match_clip's
        routes, and walks all takes from them.  Returns a takes.TakesResult: codes, phases, votes, seed_codes,
        first_shared_code (from which code on a take repeats an earlier one) and n_distinct."""
        from . import takes
        self._refuse_nophase("match_clip_takes")
        return takes.match_clip_takes(self, test_interp, test_context, n_windows, n_takes, seed_codes, seed_phases, mode)

    @staticmethod
    def check_status(status):
        """status: the walk's two status ints on the host.  Raises what must never be ignored."""
        if int(status[1]) != 0:
            raise GuardOverflow(int(status[1]))
        if int(status[0]) != 0:
            raise IndexError("a code that never occurs in the database won a rank fusion "
                             "(the reference raises IndexError at GestureKNN.py:631-632)")

    def capture_clip_graph(self, n_windows, mode=MODE_AUD_TXT, n_sweep_windows=None, window_offset=0, audio=None,
                           context=None, owner_blocks=False, n_clips=1, encoder=None, encode_input=None,
                           encode_precision="f32", sweep_signal=False, doorbell=False, n_takes=1):
        """Capture the whole per-clip launch sequence (pack, both sweeps, per-code argmin passes, ranks,
        rank-fusion tables, walk) into one HIP graph for a fixed clip shape.  Returns a ClipGraph whose
        run(test_audio, test_context, seed_code, seed_phase) replays it; results are device tensors.
        n_sweep_windows > n_windows sweeps more windows than it walks (several clips per sweep: bench.py N>1).
        audio / context: bind the graph to the caller's resident input tensors instead of static copies.
        n_clips > 1 (round 5; BASELINE configs[4]): that many independent clips of n_windows windows per replay, ONE
        batched sweep and one set of walk launches for all of them (their steps back to back in the tables).
        encoder / encode_input: a VQVAE and a resident pose batch f32 [B][T][C] whose encode (make_beat_dataset.py:314-316)
        runs INSIDE the capture on a branch of its own beside the match - one replay = the fused encode + match step.
        n_takes > 1: ONE clip per replay walked from n_takes seeds behind its one sweep (walk_takes); seeds
        and results in the several-clips layout with takes in the place of clips (ClipGraph.run_takes / run_ints).  One GPU,
        n_clips == 1, no encode leg, no doorbell.  With the default the capture is unchanged, node for node."""
        from .replay import ClipGraph
        self._refuse_nophase("capture_clip_graph")
        return ClipGraph(self, n_windows, mode, n_sweep_windows or n_windows * n_clips, window_offset, audio, context,
                         owner_blocks, n_clips, encoder, encode_input, encode_precision, sweep_signal, doorbell, n_takes)

    def _tables_and_walk(self, test_interp, test_context, n_windows, mode, seed_code, seed_phase, return_tables,
                         for_walk=False, coins=None):
        if not self.use_phase:
            for_walk = False                # (plan_nophase: the walk-relevance cut and the prefused tables never feed this walk)
        T = self.sweep_tables(test_interp, test_context, n_windows, mode, for_walk=for_walk)
        if return_tables:
            self.tables = T
        if not self.use_phase:
            return self.walk(T, n_windows, 0, mode, seed_code, coins=coins)
        return self.walk(T, n_windows, 0, mode, seed_code, seed_phase)

    def match_clip(self, test_interp, test_context, n_windows, mode=MODE_AUD_TXT, seed_code=None,
                   seed_phase=None, return_tables=False, coins=None):
        """All windows of one clip: two batched sweeps + rank kernels + one device-side tail walk.
        Returns (codes int64 [M,30], phases f32 [M,8,8,16], votes [M,8]) as NumPy arrays.
        A clip for which the capped near-tie machinery raised its trouble word (GuardOverflow) is matched again on
        the uncapped path before anything is returned (on a sharded DB every rank sees the same word and re-matches).
        A matcher without the phase gate (use_phase=False) returns (codes int64 [M,30], phases f32 [M,0,8,16], sides i32
        [M,steps]: 0 audio / 1 text) and keeps the appended candidates as last_picks; its state is the seed code and, with
        both modalities on, the clip's M * steps coins (`coins`; drawn from the rng behind the seed if not given, like
        that many successive rand() calls of the reference's loop)."""
        coins_kw = {}
        if not self.use_phase:
            plan = plan_nophase(self._knobs(), self._facts(), n_windows, self.n_steps(), mode, self.desired_k)
            if plan.path != "kernel":
                raise NotImplementedError(plan.reason)
            if seed_code is None:                   # seed, then coins, both drawn ONCE: a re-match replays them
                seed_code = self.init_code_phase()
            if coins is None and mode == MODE_AUD_TXT:
                coins = self.draw_coins(n_windows * self.n_steps())
            seed_phase, coins_kw = None, dict(coins=coins)
        elif seed_code is None:                     # drawn ONCE: a re-match starts from the same state
            seed_code, seed_phase = self.init_code_phase()
        if n_windows == 0:                          # an empty clip (the reference's loop body never runs, :785)
            n_blocks = self.n_steps() if self.use_phase else 0
            return (np.zeros((0, num_frames_code), np.int64), np.zeros((0, n_blocks, 8, 16), np.float32),
                    np.zeros((0, self.n_steps()), np.int32))
        clip = (test_interp.contiguous(), test_context, n_windows, mode, seed_code, seed_phase, return_tables)
        try:
            return self._tables_and_walk(*clip, for_walk=not return_tables, **coins_kw)
        except GuardOverflow as e:
            if self.audio_precision == "exact":
                self.clear_flags()          # (the sticky word must not poison the clips after this one)
                raise RuntimeError("the uncapped path raised flags 0x%x: this is a bug" % e.flags)
            return self.rematch(e.flags, *clip, **coins_kw)

    def rematch(self, flags, test_interp, test_context, n_windows, mode, seed_code, seed_phase, return_tables=False,
                coins=None):
        """The clip again on a path that cannot raise `flags`: only the text prefilter overflowed (FLAG_TEXT_OVERFLOW alone)
        -> the same audio path with the text side on the exact-order sweep; anything else -> audio_precision "exact"
        (f64 sweep + uncapped guard, which also takes the exact-order text sweep).  Clears the trouble word."""
        clip = (test_interp, test_context, n_windows, mode, seed_code, seed_phase, return_tables)
        if flags == FLAG_TEXT_OVERFLOW and self.text_kernel == "mfma":
            self.clear_flags()
            self.fallbacks += 1
            self.text_fallbacks += 1
            self.text_kernel = "valu"
            try:
                return self._tables_and_walk(*clip, coins=coins)
            except GuardOverflow:               # the audio side of this clip is in trouble as well
                return self.rematch_exact(*clip, coins=coins)
            finally:
                self.text_kernel = "mfma"
        return self.rematch_exact(*clip, coins=coins)

    def rematch_exact(self, test_interp, test_context, n_windows, mode, seed_code, seed_phase, return_tables=False,
                      coins=None):
        """The clip again with audio_precision "exact" (f64 sweep + uncapped guard); clears the trouble word."""
        prev = self.audio_precision
        self.clear_flags()
        self.audio_precision = "exact"
        self.fallbacks += 1
        try:
            return self._tables_and_walk(test_interp, test_context, n_windows, mode, seed_code, seed_phase, return_tables,
                                         coins=coins)
        finally:
            self.audio_precision = prev




def predict_code_from_audio(db, test_interp, test_context, n_windows, mode=MODE_AUD_TXT, rng=None, use_phase=True,
                            desired_k=0):
    """predict_code_from_audio (GestureKNN.py:724-813) for the shipped flags (use_phase=False: without the phase gate, at
    position desired_k, :578-592); returns (M,30) int64."""
    knn = CodeKNN(db, rng=rng, use_phase=use_phase, desired_k=desired_k)
    codes, _, _ = knn.match_clip(test_interp, test_context, n_windows, mode=mode)
    return codes


# The captured / pipelined replays live in replay.py since round 6 (this module was 2 000 lines).  Every caller imports them
# from here, so the names resolve lazily (PEP 562; replay.py imports THIS module, whichever of the two is imported first).
_REPLAY_NAMES = ("ClipGraph", "ClipPipeline", "GraphPipeline", "SerialReplayer")


def __getattr__(name):
    if name in _REPLAY_NAMES:
        from . import replay
        return getattr(replay, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
