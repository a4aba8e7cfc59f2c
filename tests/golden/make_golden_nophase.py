#!/usr/bin/env python
"""Golden vectors of the reference's matching WITHOUT the phase gate (search_code_knn(use_phase=False),
GestureKNN.py:578-592), by running the REFERENCE (imported from /root/reference the way make_golden.py does, with its
Levenshtein stand-in).  Runs only in the build container; only the OUTPUTS are committed.

Two routes:
  wavvq fixtures   the unmodified predict_code_from_audio(use_phase=False, use_wavvq=True, use_feature=True, ...): the
                   reference's one well-formed no-phase route (GestureKNN.py:792-793).
  WavLM fixtures   the window loop of predict_code_from_audio (:785-809) restated around the unmodified
                   search_code_knn(use_phase=False, use_wavlm=True, use_feature=True, ...), because the reference's own
                   WavLM call at :802 drops the flags (use_phase / use_txt / use_aud never reach search_code_knn).

Captured per fixture:
  knn_pred                 (M,30) int64
  init_code                the init_code_phase() draw (:462-467: the code alone)
  coins                    every np.random.rand() the run made, in order (one per step in the two-sided mode, none otherwise)
  step_combined_score      combined_score at the end of every step (:579 three-way / :575 two-way), f64 [Q][512]
  step_pos_score           pos_score (:540-545), f64 [Q][512]
  step_chosen              combined_sorted_idx[desired_k], [Q]
  step_freq_score          freq_score (:544), i16 [512] (the reference's own unstable ranking of the code frequencies)
  step_aud_score / step_txt_score   aud_score / txt_score (:574, :553), i16 [Q][512]: the rank rows as the reference's
                           unstable argsort ordered their equal distances (the Levenshtein distances of the wavvq
                           fixtures are small integers and tie massively; codes absent from the database tie at 1e+3)
  aud_pay / txt_pay        the per-code 4-code payloads of search_audio_cands / search_text_cands, i16 [Q][512][4] (-1: none)
  aud_aux / txt_aux        their [j, k], i32 [Q][512][2]
  aud_dist / txt_dist      the per-code distances
  desired_k, np_seed, meta

The reference's np.argsort is unstable; the library's rule is (score, code index).  The two agree at position k when the
score there differs from its neighbours', which this script ASSERTS for every step of every fixture (a fixture that fails
it gets another np_seed below - none needed one so far).

Usage: python tests/golden/make_golden_nophase.py [--only NAME]
"""
import argparse
import os
import runpy
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
REF_DIR = "/root/reference/codebook/Speech2GestureMatching"

from qpgesture_amd import synth  # noqa: E402
from make_golden import _lev  # noqa: E402

FIXTURES = {
    # name: (n_train, n_test, seeds(train, test, code, sig), route, use_txt, desired_k, np_seed)
    # (the WavLM fixtures draw from the seed the reference sets at import, 123456; the wavvq ones from make_golden.py's 2)
    "nophase_audtxt_n48_m2_s0": (48, 2, (0, 1, 2, 3), "wavlm", True, 0, 123456),
    "nophase_aud_n48_m2_s0": (48, 2, (0, 1, 2, 3), "wavlm", False, 0, 123456),
    "nophase_audtxt_k3_n48_m2_s0": (48, 2, (0, 1, 2, 3), "wavlm", True, 3, 123456),
    "nophase_wavvq_aud_n40_m2_s20": (40, 2, (20, 21, 22, 23), "wavvq", False, 0, 2),
    "nophase_wavvq_audtxt_n40_m2_s20": (40, 2, (20, 21, 22, 23), "wavvq", True, 0, 2),
}


def run_reference(paths, route, use_txt, desired_k, np_seed):
    stub = types.ModuleType("Levenshtein")
    stub.distance = _lev
    sys.modules["Levenshtein"] = stub
    argv = ["GestureKNN.py"]
    for k, v in paths.items():
        argv += ["--" + k, v]
    argv += ["--desired_k", str(desired_k)]
    old_argv, old_cwd, old_path, old_rand = sys.argv, os.getcwd(), list(sys.path), np.random.rand
    sys.argv = argv
    os.chdir(REF_DIR)
    sys.path.insert(0, REF_DIR)
    cap = dict(aud=[], txt=[], steps=[], init=[], coins=[])
    try:
        g = runpy.run_path(os.path.join(REF_DIR, "GestureKNN.py"), run_name="ref")
        K = g["CodeKNN"]
        orig_aud, orig_txt, orig_init, orig_knn = (K.search_audio_cands, K.search_text_cands, K.init_code_phase,
                                                   K.search_code_knn)

        def wrap_aud(self, clip_input, mode="audio"):
            r = orig_aud(self, clip_input, mode)
            cap["aud"].append(r)
            return r

        def wrap_txt(self, clip_input, mode="wavvq_feat"):
            r = orig_txt(self, clip_input, mode)
            cap["txt"].append(r)
            return r

        def wrap_init(self):
            r = orig_init(self)
            cap["init"].append(r)
            return r

        def wrap_rand(*a):
            r = old_rand(*a)
            cap["coins"].append(float(r))
            return r

        code_obj = orig_knn.__code__
        step_line = 659                     # last statement of the while body: `i += STEP_SZ * self.step_sz`

        def local_trace(frame, event, arg):
            if event == "line" and frame.f_lineno == step_line:
                L = frame.f_locals
                cap["steps"].append(dict(combined_score=np.array(L["combined_score"], np.float64),
                                         pos_score=np.array(L["pos_score"], np.float64),
                                         freq_score=np.array(L["freq_score"], np.int64),
                                         aud_score=np.array(L["aud_score"], np.int64),
                                         txt_score=np.array(L["txt_score"], np.int64) if "txt_score" in L else None,
                                         chosen=int(L["combined_sorted_idx"][L["desired_k"]])))
            return local_trace

        def global_trace(frame, event, arg):
            return local_trace if frame.f_code is code_obj else None

        def wrap_knn(self, *a, **kw):
            sys.settrace(global_trace)
            try:
                return orig_knn(self, *a, **kw)
            finally:
                sys.settrace(None)

        K.search_audio_cands, K.search_text_cands = wrap_aud, wrap_txt
        K.init_code_phase, K.search_code_knn = wrap_init, wrap_knn
        np.random.rand = wrap_rand
        a = g["args"]
        from data_processing import load_db_codebook, calc_data_stats
        L = load_db_codebook(a.train_database, a.train_codebook, a.test_data, a.train_wavlm, a.test_wavlm, a.train_wavvq,
                             a.test_wavvq)
        (train_mfcc, train_code, test_mfcc, train_feat, test_feat, train_wavlm, test_wavlm, train_wavlm_feat,
         test_wavlm_feat, speech_features, test_speech_features, train_speech_features_feat, test_speech_features_feat,
         train_wavvq_feat, test_wavvq_feat, train_phase, test_phase, train_context, test_context) = L
        T = lambda x: x.transpose((0, 2, 1))
        st = {}
        for nm, (x, y) in dict(mfcc=(train_mfcc, test_mfcc), feat=(train_feat, test_feat),
                               speech_features=(speech_features, test_speech_features),
                               speech_features_feat=(train_speech_features_feat, test_speech_features_feat)).items():
            m_, s_, _, _ = calc_data_stats(T(x), T(y))
            st[nm + "_train_mean"], st[nm + "_train_std"] = m_, s_
        t0 = time.time()
        np.random.seed(np_seed)
        if route == "wavvq":
            knn_pred = g["predict_code_from_audio"](
                train_mfcc, train_code, test_mfcc, st, train_feat, test_feat, train_wavlm, test_wavlm, train_wavlm_feat,
                test_wavlm_feat, speech_features, test_speech_features, train_speech_features_feat,
                test_speech_features_feat, train_wavvq_feat, test_wavvq_feat, train_phase, test_phase, train_context,
                test_context, use_feature=True, use_wavlm=False, use_freq=False, use_speechfeat=False, use_wavvq=True,
                use_phase=False, use_txt=use_txt, use_aud=True, frames=0)
        else:
            # predict_code_from_audio's preparation (:730-778) and window loop (:785-809), with the flags passed on
            nd = g["normalize_data"]
            knn = K(mfcc_train=T(nd(train_mfcc, st["mfcc_train_mean"], st["mfcc_train_std"])), code_train=train_code,
                    feat_train=T(nd(train_feat, st["feat_train_mean"], st["feat_train_std"])), wavlm_train=T(train_wavlm),
                    wavlm_train_feat=T(train_wavlm_feat),
                    speech_features=T(nd(speech_features, st["speech_features_train_mean"],
                                         st["speech_features_train_std"])),
                    speech_features_feat=T(nd(train_speech_features_feat, st["speech_features_feat_train_mean"],
                                              st["speech_features_feat_train_std"])),
                    wavvq_train_feat=T(train_wavvq_feat), phase_train=T(train_phase), context_train=T(train_context),
                    use_wavlm=True, use_wavvq=False, use_phase=False, use_txt=use_txt)
            tw, tc = T(test_wavlm_feat), T(test_context)
            motion_output = []
            for i in range(test_wavvq_feat.shape[0]):
                pred_motion, _ = knn.search_code_knn(
                    clip_test=tw[i], desired_k=desired_k, use_wavlm=True, use_feature=True, use_freq=False,
                    seed_code=motion_output[-1][-1] if i > 0 else None, use_wavvq=False, use_phase=False, use_txt=use_txt,
                    clip_context=tc[i] if use_txt else None, use_aud=True)
                motion_output.append(pred_motion)
            knn_pred = np.array(motion_output)
        wall = time.time() - t0
    finally:
        np.random.rand = old_rand
        sys.argv = old_argv
        os.chdir(old_cwd)
        sys.path[:] = old_path

    def pack(trip):
        dist = np.array([np.asarray(t[0], np.float64) for t in trip])
        pay = np.full((len(trip), 512, 4), -1, np.int64)
        aux = np.full((len(trip), 512, 2), -1, np.int64)
        for s, t in enumerate(trip):
            for c in range(512):
                if len(t[1][c]):
                    p = np.asarray(t[1][c])
                    pay[s, c, :len(p)] = p
                    aux[s, c] = t[2][c]
        return dist, pay.astype(np.int16), aux.astype(np.int32)

    res = {"knn_pred": knn_pred, "ref_wall_s": np.float64(wall), "init_code": np.int64(cap["init"][0]),
           "coins": np.array(cap["coins"], np.float64), "desired_k": np.int64(desired_k), "np_seed": np.int64(np_seed)}
    assert len(cap["init"]) == 1, "the seed is drawn for the first window only"
    res["aud_dist"], res["aud_pay"], res["aud_aux"] = pack(cap["aud"])
    if cap["txt"]:
        d, res["txt_pay"], res["txt_aux"] = pack(cap["txt"])
        res["txt_dist"] = d.astype(np.float32)
        assert np.array_equal(res["txt_dist"].astype(np.float64), d), "text distances are not float32 values"
    res["step_combined_score"] = np.array([s["combined_score"] for s in cap["steps"]])
    res["step_pos_score"] = np.array([s["pos_score"] for s in cap["steps"]])
    res["step_chosen"] = np.array([s["chosen"] for s in cap["steps"]], np.int64)
    res["step_freq_score"] = cap["steps"][0]["freq_score"].astype(np.int16)
    res["step_aud_score"] = np.array([s["aud_score"] for s in cap["steps"]]).astype(np.int16)
    if use_txt:
        res["step_txt_score"] = np.array([s["txt_score"] for s in cap["steps"]]).astype(np.int16)
    # the reference's unstable order is the stable one at position k only if the score there has no equal neighbour
    k = desired_k
    for q, s in enumerate(res["step_combined_score"]):
        o = np.sort(s)
        assert (k == 0 or o[k - 1] != o[k]) and o[k] != o[k + 1], \
            "step %d: the score at position %d ties with a neighbour - move this fixture's np_seed" % (q, k)
        assert np.argsort(s, kind="stable")[k] == res["step_chosen"][q]
    assert len(res["coins"]) == (len(cap["steps"]) if use_txt else 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    for name, (ntr, nte, seeds, route, use_txt, k, np_seed) in FIXTURES.items():
        if a.only and a.only != name:
            continue
        with tempfile.TemporaryDirectory() as td:
            paths = synth.write_npz_set(td, ntr, nte, *seeds, wavlm_dim=1024 if route == "wavlm" else 8)
            res = run_reference(paths, route, use_txt, k, np_seed)
        res["meta"] = np.array([ntr, nte, *seeds, 0], np.int64)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **res)
        print(name, "knn_pred", res["knn_pred"].shape, str(res["knn_pred"].dtype), "ref wall %.1fs" % res["ref_wall_s"],
              "coins", len(res["coins"]), flush=True)


if __name__ == "__main__":
    main()
