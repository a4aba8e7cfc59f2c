"""Shared fixtures for the parity tests: regenerate the synthetic inputs of a golden fixture."""
import os
import tempfile

import numpy as np

from qpgesture_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def fixture_arrays(n_train, n_test, s_train, s_test, s_code, s_sig, wavlm_dim=1024, variant=None):
    """In-memory version of synth.write_npz_set (same seeds -> same bytes), already windowed the way
    data_processing.load_db_codebook leaves them: interpolated WavLM, squeezed context, dense phase."""
    from oracle import knn_oracle as O
    tr = synth.make_db(n_train, s_train, wavlm_dim)
    te = synth.make_db(n_test, s_test, wavlm_dim)
    code = synth.make_codes(n_train, s_code)
    synth.apply_variant(tr, te, code, variant)
    return dict(
        code=code, sig=synth.make_signature(s_sig),
        tr_interp=O.interp_wavlm(tr["wavlm"]), te_interp=O.interp_wavlm(te["wavlm"]),
        tr_ctx=tr["context"].squeeze(2), te_ctx=te["context"].squeeze(2),
        tr_phase=tr["phase_dense"], te_phase=te["phase_dense"],
        tr_wavvq=tr["wavvq"], te_wavvq=te["wavvq"])


def aud_tol(knn):
    """Tolerance of the audio distance TABLE against the reference's f64 values: 1e-13 for the f64 sweep; the sweep's
    a-priori bound for the mixed-precision path (untouched minima keep the sweep value; winners and ranks are exact
    either way and asserted separately)."""
    from qpgesture_amd.code_knn import AUDIO_MX_ERR
    mixed = knn.audio_precision == "mixed" and knn.db.world == 1 and knn.tie_eps > 0
    return AUDIO_MX_ERR if mixed else 1e-13


# ---- the stand-alone C-ABI entry points, driven by hand (test scaffolding: the product calls the fused forms) ----------
def sweep_audio_unfused(knn, qbase, q_win, q_t):
    """Distance matrix (qpg_audio_cosine_f64), then the unguarded qpg_percode_select_f64: same tables as CodeKNN.sweep_audio's
    f64 path on tie-free data."""
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.code_knn import _i32
    from qpgesture_amd.constant import ABSENT_DIST, NUM_AUDIO_FEAT_FRAMES
    db, dev = knn.db, knn.db.device
    Q = len(q_win)
    qbase = qbase.contiguous()
    M, T, F = qbase.shape
    q32 = torch.empty((Q, NUM_AUDIO_FEAT_FRAMES * F), dtype=torch.float32, device=dev)
    qn2 = torch.empty((Q,), dtype=torch.float64, device=dev)
    _lib.call("qpg_audio_pack_queries", dev, qbase, M, T, F, _i32(q_win, dev), _i32(q_t, dev), Q,
              NUM_AUDIO_FEAT_FRAMES, db.tap_stride, q32, qn2)
    D = torch.empty((Q, max(db.n_local * db.Ga, 1)), dtype=torch.float64, device=dev)
    _lib.call("qpg_audio_cosine_f64", dev, db.base, db.n_local, db.T, db.F, db.aud_t, db.Ga,
              NUM_AUDIO_FEAT_FRAMES, db.tap_stride, db.cn2, q32, qn2, Q, D, D.stride(0))
    dist = torch.empty((Q, db.K), dtype=torch.float64, device=dev)
    idx = torch.empty((Q, db.K), dtype=torch.int32, device=dev)
    _lib.call("qpg_percode_select_f64", dev, D, D.stride(0), Q, db.aud_cand_code, db.n_local * db.Ga, db.K,
              float(ABSENT_DIST), db.idx_base * db.Ga, dist, idx, None, 0, 0)
    return dist, idx, D


def sweep_text_unfused(knn, queries):
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.constant import ABSENT_DIST
    db, dev = knn.db, knn.db.device
    Q = queries.shape[0]
    qn = torch.empty_like(queries)
    _lib.call("qpg_l2_normalize_rows_f32", dev, queries, Q, db.Dt, qn)
    D = torch.empty((Q, max(db.Ct, 1)), dtype=torch.float32, device=dev)
    _lib.call("qpg_text_cosine_f32", dev, db.ctxt, db.Ct, db.Dt, qn, Q, D, D.stride(0))
    dist = torch.empty((Q, db.K), dtype=torch.float32, device=dev)
    idx = torch.empty((Q, db.K), dtype=torch.int32, device=dev)
    _lib.call("qpg_percode_select_f32", dev, D, D.stride(0), Q, db.txt_cand_code, db.Ct, db.K, float(ABSENT_DIST),
              db.idx_base * db.Gt, dist, idx, None, 0, 0)
    return dist, idx, D


def merge_mixed_by_hand(recv, W, src_stride, dist_off, idx_off, Q, K, eps1, eps2, shards, R=4096, fl_cap=1024, ws=None,
                        ws_bytes=None, out=None):
    """The cross-shard merge of mixed-precision tables (qpg_merge_mixed_phase1_f64 -> qpg_shard_refine_f64 on every shard ->
    qpg_merge_mixed_phase2_f64) on ONE device, for one owner that holds all Q queries, with the two byte exchanges done by
    hand.  recv: what the all-gather leaves on every rank (W table blocks src_stride bytes apart, distances at dist_off,
    global candidate indices at idx_off).  shards: per row shard a dict with the arguments of ITS refine call - cand_base
    (global index of its first candidate), base, base_is_f16, T, F, cand_t, G, tap_stride, q32, qn2, cn2.
    ws: the caller's workspace (u8, at least qpg_merge_mixed_ws_bytes; contents on entry are ignored: it is handed to
    phase 1 as it is and phase 2 reads what phase 1 left); ws_bytes: the size to state instead of ws.numel(); out: the
    caller's (dist, idx, rank) tensors.  Returns (dist, idx, rank, stats as numpy, requests per shard)."""
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.constant import ABSENT_DIST
    dev = recv.device
    req_stride, resp_stride = 8 + 8 * R, 8 + 8 * R
    req = torch.zeros((W * req_stride,), dtype=torch.uint8, device=dev)
    if ws is None:
        ws = torch.empty((int(_lib.load().qpg_merge_mixed_ws_bytes(Q, K, fl_cap)),), dtype=torch.uint8, device=dev)
    ws_bytes = ws.numel() if ws_bytes is None else ws_bytes
    stats = torch.zeros((4,), dtype=torch.int32, device=dev)
    _lib.call("qpg_merge_mixed_phase1_f64", dev, recv, W, src_stride, dist_off, idx_off, Q, K, float(ABSENT_DIST), eps1, R,
              req, req_stride, ws, ws_bytes, stats, fl_cap, -1)
    counts = [int(req[w * req_stride:w * req_stride + 4].view(torch.int32)[0]) for w in range(W)]   # header: count | flags
    resp_recv = torch.zeros((W * resp_stride,), dtype=torch.uint8, device=dev)
    for w in range(W):                                       # all-to-all by hand: owner 0's block w -> shard w's block 0
        req_recv = torch.full((W * req_stride,), 255, dtype=torch.uint8, device=dev)      # (unused slots / blocks: ~0)
        for b in range(W):
            req_recv[b * req_stride:b * req_stride + 8] = 0                       # headers: count | flags
        req_recv[:req_stride] = req[w * req_stride:(w + 1) * req_stride]
        resp = torch.zeros((W * resp_stride,), dtype=torch.uint8, device=dev)
        s = shards[w]
        _lib.call("qpg_shard_refine_f64", dev, req_recv, W, req_stride, R, 0, int(s["cand_base"]), s["base"],
                  int(s["base_is_f16"]), s["T"], s["F"], s["cand_t"], s["G"], 6, s["tap_stride"], s["q32"], s["qn2"], s["cn2"],
                  resp, resp_stride, 0, None, R // Q)
        resp_recv[w * resp_stride:(w + 1) * resp_stride] = resp[:resp_stride]
    d, ix, rk = out if out is not None else (torch.empty((Q, K), dtype=torch.float64, device=dev),
                                             torch.empty((Q, K), dtype=torch.int32, device=dev),
                                             torch.empty((Q, K), dtype=torch.int16, device=dev))
    _lib.call("qpg_merge_mixed_phase2_f64", dev, recv, W, src_stride, idx_off, Q, K, float(ABSENT_DIST), ws, ws_bytes,
              resp_recv, resp_stride, d, ix, rk, stats, fl_cap, eps2)
    torch.cuda.synchronize()
    return d, ix, rk, stats.cpu().numpy(), counts


def decode_layers(m, ids, kernel="f32"):
    """Layer-by-layer decode through the per-layer entry points (qpg_vq_gather_f32, then the model's walk over its decoder
    plan on one kernel family; "f32": qpg_conv1d_f32): same result as VQVAE.decode(), which makes ONE C call."""
    import torch
    from qpgesture_amd import _lib
    ids = torch.as_tensor(ids).to(m.device, torch.int64).contiguous()
    B, L = ids.shape
    status = torch.zeros((1,), dtype=torch.int32, device=m.device)
    x = torch.empty((B, L, m.emb), dtype=torch.float32, device=m.device)
    _lib.call("qpg_vq_gather_f32", m.device, m.k, ids, B * L, m.emb, m.bins, x, status)
    return m._walk(m.dec_plan, x, B, L, kernel)
