"""The scratch contract on the host objects ("Scratch contract"): every object that keeps grow-only scratch
between calls is built and run through a sequence of calls - long first, then short, then across a path threshold - under
tests/poison.py's poisoned_alloc (0xFF and 0x3C: every torch.empty / empty_like / np.empty of the package returns
pattern-filled memory, the not-yet-written result tensors included), and every call's documented results are compared BIT
FOR BIT with the same call on a fresh object, built and run without poisoning.  The fresh objects' results are held to
their references by the objects' own tests.  A sequence during which the package drew no poisoned allocation has shown
nothing and fails.  Seeds and coins are passed explicitly.

One REUSE line per test with the allocations served per module (pytest -s; profiles/scratch_contract.md)."""
import functools

import numpy as np
import pytest

from tests import poison as P
from tests import select_ref as SR
from tests.helpers import fixture_arrays

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATTERNS = (0xFF, 0x3C)


def _flat(x, out=None, path=""):
    """Every array in a result (nested tuples / lists / dicts / NamedTuples of tensors, arrays and numbers), copied to the
    host at once (a result may be a view of scratch the next call reuses) -> [(path, ndarray)]."""
    import torch
    out = [] if out is None else out
    if x is None:
        out.append((path, np.zeros(0, np.uint8)))
    elif isinstance(x, torch.Tensor):
        out.append((path, x.detach().cpu().contiguous().numpy().copy()))
    elif isinstance(x, np.ndarray):
        out.append((path, np.ascontiguousarray(x).copy()))
    elif isinstance(x, dict):
        for k in x:
            _flat(x[k], out, "%s[%r]" % (path, k))
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            _flat(v, out, "%s[%d]" % (path, i))
    elif isinstance(x, (bool, int, float, np.generic)):
        out.append((path, np.asarray(x)))
    else:
        raise TypeError("%s: %r is not a result this test can compare" % (path, type(x)))
    return out


def _sequence(monkeypatch, label, build, calls, owners):
    """owners: the module(s) of the object under test - THEIR poisoned allocations are what the test is about (the weight
    generators of qpgesture_amd.synth draw np.empty too).  calls: [(name, function(object) -> result)].  Fresh: one new,
    unpoisoned object PER CALL.  Poisoned: ONE object, built and run under the pattern, all calls in order."""
    import torch
    want = []
    for name, call in calls:
        want.append(_flat(call(build())))
    torch.cuda.synchronize()
    for pat in PATTERNS:
        with P.poisoned_alloc(monkeypatch, pat) as served:
            obj = build()
            got = [_flat(call(obj)) for _, call in calls]
            torch.cuda.synchronize()
        n = served.from_modules(*owners)
        print("REUSE %-28s fill 0x%02X: %d poisoned allocations from %s (%s); by dtype %s"
              % (label, pat, n, "/".join(owners), ", ".join("%s %d" % kv for kv in sorted(served.by_module.items())),
                 served.by_dtype))
        assert n > 0, "%s: the object under test drew no poisoned allocation - the test has shown nothing" % label
        for (name, _), w, g in zip(calls, want, got):
            assert [p for p, _ in w] == [p for p, _ in g], (label, name)
            for (path, a), (_, b) in zip(w, g):
                assert a.dtype == b.dtype and a.shape == b.shape, (label, name, path, a.dtype, b.dtype, a.shape, b.shape)
                same = np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))
                assert same, "%s, call %s, fill 0x%02X: result%s differs from a fresh object's in %d of %d bytes" % (
                    label, name, pat, path, int((a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)).sum()), a.nbytes)


# ---- CodeKNN ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clip():
    """The arrays of the shipped_n48_m2_s0 fixture's size with three test windows, and one explicit seed."""
    A = fixture_arrays(48, 3, 0, 1, 2, 3)
    rs = np.random.RandomState(99)
    seeds = dict(code=int(rs.randint(0, 512)), phase=rs.standard_normal((8, 16)).astype(np.float32),
                 codes=rs.randint(0, 512, size=65).astype(np.int32), phases=rs.standard_normal((65, 8, 16)).astype(np.float32))
    return A, seeds


def _db():
    from qpgesture_amd.code_knn import GestureDB
    A, _ = _clip()
    return GestureDB(A["code"], A["tr_interp"], A["tr_ctx"], A["tr_phase"], A["sig"], device=DEV)


def _inputs(M):
    import torch
    A, _ = _clip()
    return (torch.from_numpy(np.ascontiguousarray(A["te_interp"][:M])).to(DEV),
            torch.from_numpy(np.ascontiguousarray(A["te_ctx"][:M])).to(DEV))


def _tensors(T):
    import torch
    return {k: v for k, v in T.items() if isinstance(v, (torch.Tensor, np.ndarray))}


@pytest.mark.parametrize("precision,single", [("mixed", False), ("mixed", True), ("f64", False), ("exact", False)])
def test_code_knn_long_then_short_clips(monkeypatch, precision, single):
    """match_clip(return_tables=True) with M = 3 -> 1 -> 2 windows in every modality mode on ONE matcher: codes, phases,
    votes and every table (distances, winners, ranks) - _mix_ws, _exact_ws, _hl_qimage, the text prefilter's scratch, the
    gate tables, the pinned result buffers."""
    from qpgesture_amd.code_knn import CodeKNN
    _, seeds = _clip()

    def build():
        knn = CodeKNN(_db(), rng=np.random.RandomState(5))
        knn.audio_precision, knn.mixed_single_launch = precision, single
        return knn

    def call(M, mode):
        def run(knn):
            te_i, te_c = _inputs(M)
            res = knn.match_clip(te_i, te_c, M, mode=mode, seed_code=seeds["code"], seed_phase=seeds["phase"], return_tables=True)
            return res, _tensors(knn.tables)
        return "M=%d mode=%d" % (M, mode), run
    _sequence(monkeypatch, "CodeKNN %s%s" % (precision, " single-launch" if single else ""), build,
              [call(M, mode) for M in (3, 1, 2) for mode in (0, 1, 2)], owners=("qpgesture_amd.code_knn",))


def test_code_knn_takes_many_then_few(monkeypatch):
    """match_clip_takes with 65 takes, then 3, on one matcher (_takes_ws, the takes' pinned buffers)."""
    from qpgesture_amd.code_knn import CodeKNN
    _, seeds = _clip()

    def call(n):
        def run(knn):
            te_i, te_c = _inputs(2)
            r = knn.match_clip_takes(te_i, te_c, 2, seed_codes=seeds["codes"][:n], seed_phases=seeds["phases"][:n])
            return r.codes, r.phases, r.votes
        return "%d takes" % n, run
    _sequence(monkeypatch, "CodeKNN takes", lambda: CodeKNN(_db(), rng=np.random.RandomState(5)), [call(65), call(3)],
              owners=("qpgesture_amd.takes",))


def test_code_knn_without_the_phase_gate(monkeypatch):
    """A use_phase=False matcher with M = 3 -> 1 (_nophase_ws, _pinned_nophase): codes, sides and the appended candidates."""
    from qpgesture_amd.code_knn import CodeKNN
    _, seeds = _clip()

    def call(M):
        def run(knn):
            te_i, te_c = _inputs(M)
            coins = np.random.default_rng(M).random(M * knn.n_steps()) > 0.5
            res = knn.match_clip(te_i, te_c, M, seed_code=seeds["code"], coins=coins)
            return res, knn.last_picks
        return "M=%d" % M, run
    _sequence(monkeypatch, "CodeKNN use_phase=False", lambda: CodeKNN(_db(), use_phase=False, rng=np.random.RandomState(5)),
              [call(3), call(1)], owners=("qpgesture_amd.code_knn",))


# ---- SortedRows / CosineIndex ------------------------------------------------------------------------------------------------
def _text_queries(Q):
    import torch
    t = SR.text_case()
    return torch.from_numpy(t.qn[:Q].copy()).to(DEV), torch.from_numpy(t.q[:Q].copy()).to(DEV)


def test_sorted_rows_with_one_caller_scratch(monkeypatch):
    """SortedRows.select with ONE caller scratch dict (cols, tmin, tmask, tmin_t, tmask_t, qperm, Dm), d = 128, 1500 rows:
    Q = 300 (by-code path; by_code_min_q is 256) -> 48 (by-query) -> 257 -> 5, select_raw at 300 after 48, and the prefilter
    matrix (use_masks=False) once."""
    import torch
    from qpgesture_amd.constant import ABSENT_DIST
    from qpgesture_amd.sorted_rows import SortedRows
    t = SR.text_case()

    def build():
        sr = SortedRows(torch.from_numpy(t.xn).to(DEV), torch.from_numpy(t.codes_masked).to(DEV), t.K, DEV)
        sr.by_code = True
        assert sr.by_code_min_q == 256 and sr.uses_by_code(257) and not sr.uses_by_code(255)
        sr.test_scratch = {}
        return sr

    def call(Q, raw=False, masks=True):
        def run(sr):
            qn, q = _text_queries(Q)
            stats = torch.zeros((4,), dtype=torch.int32, device=DEV)
            nn = torch.empty((Q,), dtype=torch.int32, device=DEV)
            rank = torch.empty((Q, t.K), dtype=torch.int16, device=DEV)
            sr.use_masks = masks
            try:
                if raw:
                    dist, idx, nn = sr.select_raw(q, float(ABSENT_DIST), stats, nn=nn, rank=rank, scratch=sr.test_scratch)
                else:
                    dist, idx, nn = sr.select(qn, float(ABSENT_DIST), stats, nn=nn, rank=rank, scratch=sr.test_scratch)
            finally:
                sr.use_masks = True
            return dist, idx, nn, rank, stats
        return "Q=%d%s%s" % (Q, " raw" if raw else "", "" if masks else " matrix"), run
    _sequence(monkeypatch, "SortedRows", build,
              [call(300), call(48), call(257), call(5), call(48), call(300, raw=True), call(48, masks=False), call(5, masks=False)],
              owners=("qpgesture_amd.sorted_rows",))


@pytest.mark.parametrize("method", ["mfma", "valu"])
def test_cosine_index_long_then_short_batches(monkeypatch, method):
    """cfg3.CosineIndex at its smallest D (128): the same Q sequence; "mfma" keeps _scratch, "valu" keeps _ws."""
    from qpgesture_amd.cfg3 import CosineIndex
    t = SR.text_case()

    def build():
        ix = CosineIndex(t.X, t.codes_masked, None, n_codes=t.K, device=DEV, method=method)
        assert ix.method == method
        return ix

    def call(Q):
        return "Q=%d" % Q, lambda ix: ix.query(_text_queries(Q)[1])
    _sequence(monkeypatch, "CosineIndex %s" % method, build, [call(300), call(48), call(257), call(5)],
              owners=("qpgesture_amd.cfg3",))


# ---- WavLM -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_inputs", [False, True])
def test_wavlm_long_then_short_batches(monkeypatch, long_inputs):
    """WavLM._ws on the tiny configuration: (B, n) = (1, 16000) -> (3, 400) -> (2, 4000); with long_inputs also a ragged
    padding_mask; without, the layer taps (ret_layer_results)."""
    import torch
    from qpgesture_amd import synth
    from qpgesture_amd import wavlm as W
    from tests.test_wavlm_long_cpu import CFG, weights

    def build():
        return W.WavLM(CFG, device=DEV, long_inputs=long_inputs).load_state_dict(weights(3))

    def call(B, n, **kw):
        def run(model):
            wav = synth.make_wav(17, B, n)
            if kw.get("ragged"):
                mask = np.zeros((B, n), bool)
                mask[1, n - n // 3:] = True
                return model.extract_features(wav, padding_mask=torch.from_numpy(mask))
            if kw.get("layers"):
                return model.extract_features(wav, output_layer=2, ret_layer_results=True)
            return model.extract_features(wav)
        return "B=%d n=%d %s" % (B, n, sorted(kw)), run
    calls = [call(1, 16000), call(3, 400), call(2, 4000)]
    calls += [call(2, 4000, ragged=True), call(1, 16000)] if long_inputs else [call(2, 4000, layers=True), call(3, 400)]
    _sequence(monkeypatch, "WavLM long_inputs=%s" % long_inputs, build, calls, owners=("qpgesture_amd.wavlm",))


# ---- VQVAE -------------------------------------------------------------------------------------------------------------------
def _vqvae(train):
    import torch
    from qpgesture_amd import synth
    from qpgesture_amd.vqvae import VQVAE
    hps = dict(width=64, emb_width=64, l_bins=96)
    sd = synth.make_vqvae_state_dict(7, hps)
    m = VQVAE(dict(vel=1, acc=1, commit=0.02, l_mu=0.99, reg=0.3, **hps), input_dim=135, device=DEV).load_state_dict(sd)
    if not train:
        return m.eval()
    m.train()
    m.k_init = True                                   # (test_backward_vs_autograd_small_width's state: the codebook as loaded,
    m.k_sum, m.k_elem = m.k.clone(), torch.ones(96, device=DEV)      # an EMA with mu = 1 that leaves it untouched - so a
    m.mu = 1.0                                        # fresh object is in the state the reused one is in at every call)
    return m


def _poses(B, T):
    import torch
    rng = np.random.Generator(np.random.PCG64(8))
    return torch.from_numpy(rng.standard_normal((B, 240, 135)).astype(np.float32)[:, :T].copy()).to(DEV)


def test_vqvae_encode_decode_long_then_short(monkeypatch):
    """VQVAE (width 64) encode / decode at (B, T) = (5, 240) -> (1, 8) -> (3, 96): _grown, _split_ws, the C workspace."""
    def call(B, T):
        def run(m):
            ids = m.encode(_poses(B, T))
            return ids, m.decode(ids)
        return "B=%d T=%d" % (B, T), run
    _sequence(monkeypatch, "VQVAE encode/decode", lambda: _vqvae(False), [call(5, 240), call(1, 8), call(3, 96)],
              owners=("qpgesture_amd.vqvae",))


def test_vqvae_training_step_after_a_larger_one(monkeypatch):
    """One training forward + backward at B = 3 after one at B = 5 (_grown, _split_ws, _rws): x_out, loss, metrics and all
    named gradients."""
    import torch

    def call(B):
        def run(m):
            torch.manual_seed(0)
            xo, loss, met = m(_poses(B, 96))
            m.backward()
            return xo, loss, dict(met), dict(m.named_gradients())
        return "B=%d" % B, run
    _sequence(monkeypatch, "VQVAE train", lambda: _vqvae(True), [call(5), call(3)], owners=("qpgesture_amd.vqvae",))


# ---- PAE ---------------------------------------------------------------------------------------------------------------------
def test_pae_phase_extraction_in_chunks(monkeypatch):
    """PAE.pose2phase_clips: clips of 500, 1 and 240 frames with chunk=97 (the workspace is reused chunk after chunk), with
    the fc outputs and the latents."""
    from qpgesture_amd import PAE, synth

    def run(net):
        clips = [synth.make_pae_motion(n, 60 + i) for i, n in enumerate((500, 1, 240))]
        return PAE.pose2phase_clips(net, clips, chunk=97, return_v=True, return_latent=True)
    _sequence(monkeypatch, "PAE.pose2phase_clips", lambda: PAE.Model(synth.make_pae_state_dict(11), device=DEV),
              [("500+1+240 frames, chunk 97", run)], owners=("qpgesture_amd.PAE",))


def test_pae_trainer_one_step(monkeypatch):
    """PAE_train.Trainer at B = 2 (Trainer.ws): one forward + backward + AdamW step; the whole training state."""
    from qpgesture_amd import PAE_train as PT
    from qpgesture_amd import synth
    from tests.test_gpu_pae_train import _data, _starts
    pn, all_starts = _data(n_clips=2, T=300)
    sd = synth.make_pae_state_dict(11)

    def build():
        tr = PT.Trainer(sd, batch=2, device=DEV)
        tr.set_data(pn)
        return tr

    def run(tr):
        loss = tr.forward(_starts(all_starts, 2, 3), train=True).clone()
        tr.backward()
        grads = tr.grads.clone()
        tr.step(1e-3, 1e-4)
        return loss, grads, tr.params, tr.stats, tr.m, tr.v, tr.num_batches_tracked
    _sequence(monkeypatch, "PAE_train.Trainer", build, [("one step", run)], owners=("qpgesture_amd.PAE_train",))
