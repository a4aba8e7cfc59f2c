"""The host side of the sentence embeddings (qpgesture_amd/sentence.py) and the f64 restatement the GPU tests compare
against (tests/sentence_ref.py), without a GPU: the restatement against transformers' f64 run (tests/golden/sentence_*.npz,
written by tests/golden/make_golden_sentence.py), the tokenizer against transformers.BertTokenizer's recorded ids, the
reference's slot arithmetic, check_supported, the seeded weights and the CLI's parser."""
import os

import numpy as np
import pytest

from qpgesture_amd import sentence as S
from qpgesture_amd import synth
from tests import sentence_ref as R

CFGS = {"tiny": synth.BERT_TINY, "minilm": synth.BERT_MINILM}
LENGTHS = [2, 3, 9, 31, 32, 33, 63, 64, 65, 127, 128]
_cache = {}


def fixture(golden_dir, name):
    """(golden arrays, id lists, state dict, f64 restatement, f32 restatement) of a fixture, computed once per session and
    shared with the GPU tests; nothing in it is modified."""
    if name not in _cache:
        g = dict(np.load(os.path.join(golden_dir, "sentence_%s.npz" % name)))
        seqs = [[int(i) for i in g["ids"][a:b]] for a, b in zip(g["seq_start"][:-1], g["seq_start"][1:])]
        sd = synth.make_bert_state_dict(int(g["seed"]), CFGS[name])
        _cache[name] = (g, seqs, sd, R.encode(sd, CFGS[name], seqs, np.float64), R.encode(sd, CFGS[name], seqs, np.float32))
    return _cache[name]


@pytest.mark.parametrize("name", ["tiny", "minilm"])
def test_restatement_reproduces_golden(golden_dir, name):
    g, seqs, sd, r64, r32 = fixture(golden_dir, name)
    assert [len(s) for s in seqs] == LENGTHS
    rows = g["tap_rows"]
    for tap, got in (("pooled", r64["pooled"]), ("embed", r64["embed"][rows]), ("layer0", r64["layer0"][rows])):
        err = np.abs(got - g[tap]).max()
        print("%s %s: |restatement - transformers f64| = %.3e" % (name, tap, err))
        assert got.shape == g[tap].shape and err <= 1e-9
    # the f32 restatement's own error is of the size of the recorded e32 (the GPU tests' unit), not far below it
    for tap, key in (("pooled", "e32"), ("embed", "e32_embed"), ("layer0", "e32_layer0")):
        e = np.abs(r32[tap].astype(np.float64) - r64[tap]).max()
        print("%s %s: e32 restated %.3e recorded %.3e" % (name, tap, e, float(g[key])))
        assert 0.1 * float(g[key]) <= e <= 10 * float(g[key])
    assert np.abs(g["pooled"]).max() > 1.0


def _token_cases(golden_dir):
    t = np.load(os.path.join(golden_dir, "sentence_tokens.npz"))
    for key, lower in (("lower", True), ("cased", False)):
        st = t["start_" + key]
        yield lower, [str(s) for s in t["strings"]], [[int(i) for i in t["ids_" + key][a:b]] for a, b in zip(st[:-1], st[1:])]


def test_tokenizer_equals_recorded_ids(golden_dir):
    seen = 0
    for lower, strings, want in _token_cases(golden_dir):
        tok = S.WordPiece(synth.make_vocab(), do_lower_case=lower)
        for s, w in zip(strings, want):
            assert tok.encode(s) == w, (lower, s, tok.encode(s), w)
            seen += 1
        assert tok.encode("") == [tok.cls_id, tok.sep_id] == [2, 3]
        assert max(len(w) for w in want) == 128 and tok.encode("a" * 101) == [2, 1, 3]
    assert seen >= 40


def test_tokenizer_equals_transformers(tmp_path):
    transformers = pytest.importorskip("transformers")
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(synth.make_vocab()) + "\n", encoding="utf-8")
    texts = ["", "Hello, world!", " so  you can speak ", "naïve café", "中 and 文", "un-speakable (hands)", "q" * 120,
             "hello " * 200, "it's 1 2 3"]
    for lower in (True, False):
        ref = transformers.BertTokenizer(str(vocab), do_lower_case=lower)
        tok = S.WordPiece(str(vocab), do_lower_case=lower, max_seq_length=64)
        for t in texts:
            assert tok.encode(t) == ref(t.strip(), truncation=True, max_length=64)["input_ids"], (lower, t)


def test_check_supported_names_the_field():
    ok = dict(synth.BERT_MINILM)
    S.check_supported(ok)
    S.check_supported(synth.BERT_TINY, 128)
    for field, value in (("hidden_act", "relu"), ("hidden_act", "gelu_new"), ("position_embedding_type", "relative_key"),
                         ("num_attention_heads", 6), ("hidden_size", 392), ("intermediate_size", 1000)):
        with pytest.raises(NotImplementedError, match=field):
            S.check_supported(dict(ok, **{field: value}))
    with pytest.raises(NotImplementedError, match="num_attention_heads"):
        S.check_supported(dict(ok, num_attention_heads=0))
    with pytest.raises(NotImplementedError, match="max_seq_length"):
        S.check_supported(ok, 256)
    with pytest.raises(NotImplementedError, match="max_seq_length"):
        S.check_supported(dict(ok, max_position_embeddings=64), 128)


def test_seeded_weights():
    a, b, c = (synth.make_bert_state_dict(s, synth.BERT_TINY) for s in (5, 5, 6))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert any(not np.array_equal(a[k], c[k]) for k in a)
    assert a["embeddings.word_embeddings.weight"].shape == (97, 64)
    assert a["embeddings.position_embeddings.weight"].shape == (512, 64)
    assert a["encoder.layer.1.intermediate.dense.weight"].shape == (128, 64)
    for k, v in a.items():                                   # nothing is all zeros or all ones
        assert np.std(v) > 0.05, k
    q, val = a["encoder.layer.0.attention.self.query.weight"], a["encoder.layer.0.attention.self.value.weight"]
    assert 1.6 < np.std(q) / np.std(val) < 2.4             # the query / key gain of 2
    assert len(synth.make_vocab()) == synth.BERT_TINY["vocab_size"]
    assert synth.BERT_MINILM["hidden_size"] == 384 and synth.BERT_MINILM["vocab_size"] == 30522


TRANSCRIPT = [
    (0.10, 0.30, "so"), (0.30, 0.52, "you"), (1.95, 2.40, "can"),
    (3.60, 4.00, "see"),          # ends exactly on a multiple of 4 s: end % 4 == 0 counts as 4, slot 28
    (3.90, 4.06, "that"),         # straddles the boundary, midpoint 3.98 < 4: window 0, slot int((3.9 + 0.06) * 3.75) = 14
    (3.97, 4.10, "this"),         # straddles it, midpoint 4.035: window 1
    (4.50, 4.70, "hand"),
    # window 2 (8 .. 12 s) has no word
    (12.00, 12.20, "moves"), (15.70, 15.99, "up"),
]


def test_code_sentences_equals_restatement(tmp_path):
    path = tmp_path / "clip.txt"
    path.write_text("".join("%r\t%r\t%s\n" % w for w in TRANSCRIPT) + "\n", encoding="utf-8")
    words = S.read_transcript(str(path))
    assert words == [list(w) for w in TRANSCRIPT] and all(isinstance(w[0], float) for w in words)
    got = S.code_sentences(words, 4)
    assert len(got) == 120 and got == R.code_sentences(words, 4)
    assert words == [list(w) for w in TRANSCRIPT]            # the caller's list is not consumed
    w0 = got[:30]
    assert w0[0] == "so you" and "see" in w0[28] and "see" in w0[25] and "see" not in w0[24]
    assert "that" in w0[14] and "that" not in w0[29] and "this" not in " ".join(w0)
    assert "this" in " ".join(got[30:60]) and "hand" in got[30 + int((0.5 + 0.7) * 3.75)]
    assert got[60:90] == [""] * 30
    assert "moves" in got[90] and "up" in got[119]
    assert S.code_sentences(words, 1) == got[:30]


def test_cli_parser():
    a = S.build_parser().parse_args(["--transcript", "t.txt", "--model", "dir", "--windows", "7", "--out", "x.npz"])
    assert (a.transcript, a.model, a.windows, a.out, a.gpu) == ("t.txt", "dir", 7, "x.npz", "0")
    assert S.build_parser().parse_args(["--transcript", "t", "--model", "d", "--windows", "1", "--gpu", "3"]).gpu == "3"
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(["--model", "dir", "--windows", "7"])


def test_load_refuses_other_pooling_and_normalize(tmp_path):
    import json
    d = tmp_path / "m"
    (d / "1_Pooling").mkdir(parents=True)
    (d / "1_Pooling" / "config.json").write_text(json.dumps(dict(word_embedding_dimension=64, pooling_mode_cls_token=True,
                                                                 pooling_mode_mean_tokens=False)))
    with pytest.raises(NotImplementedError, match="pooling_mode_cls_token"):
        S.load_sentence_model(str(d), device="cpu")
    (d / "modules.json").write_text(json.dumps([dict(idx=0, type="sentence_transformers.models.Transformer"),
                                                dict(idx=2, type="sentence_transformers.models.Normalize")]))
    with pytest.raises(NotImplementedError, match="Normalize"):
        S.load_sentence_model(str(d), device="cpu")
