"""Sentence embeddings end to end on the device (qpgesture_amd/sentence.py over qpg_bert.hip and the WavLM GEMM / LayerNorm)
against transformers' f64 run of the same seeded weights (tests/golden/sentence_*.npz; the weights are regenerated from
synth, nothing here imports transformers).

Tolerance: the device result is within MARGIN = 8 x e32 of the f64 value, e32 = max |transformers' f32 run - its f64 run|
of the same tap, read from the fixture (the rule of tests/test_gpu_wavlm.py).  Each check prints its ratio first.
Measured on an MI355X: see the table in profiles/sentence_bench.md."""
import json
import os

import numpy as np
import pytest
import torch

from qpgesture_amd import data_processing, synth
from qpgesture_amd import sentence as S
from tests.test_sentence_cpu import CFGS, _token_cases, fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 8.0
_models = {}


def model_of(golden_dir, name):
    if name not in _models:
        _models[name] = S.SentenceEncoder(CFGS[name], device=DEV).load_state_dict(fixture(golden_dir, name)[2])
    return _models[name]


def check(name, got, ref64, e32):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert np.isfinite(got).all(), name
    err = float(np.abs(got - ref64).max())
    print("%s: err %.3e e32 %.3e ratio %.2f" % (name, err, e32, err / e32))
    assert err <= MARGIN * e32, "%s: |device - f64| = %.3e > %g x e32 (%.3e)" % (name, err, MARGIN, e32)


@pytest.mark.parametrize("name", ["tiny", "minilm"])
def test_encode_ids_against_f64(golden_dir, name):
    g, seqs, _, _, _ = fixture(golden_dir, name)
    model = model_of(golden_dir, name)
    check(name + " pooled", model.encode_ids(seqs), g["pooled"], float(g["e32"]))
    taps = {}
    out = model._forward(seqs, on_stage=lambda stage, view: taps.__setitem__(stage, None if view is None else view.clone()))
    assert torch.equal(out, taps["pooled"]) and torch.equal(out, model.encode_ids(seqs))
    rows = torch.from_numpy(g["tap_rows"].astype(np.int64)).to(DEV)
    check(name + " embed", taps["embed"][rows], g["embed"], float(g["e32_embed"]))
    check(name + " layer0", taps["layer0"][rows], g["layer0"], float(g["e32_layer0"]))


def test_encode_strings_equals_encode_ids(golden_dir):
    sd = synth.make_bert_state_dict(4, synth.BERT_TINY)
    for lower, strings, ids in _token_cases(golden_dir):
        tok = S.WordPiece(synth.make_vocab(), do_lower_case=lower)
        model = S.SentenceEncoder(synth.BERT_TINY, device=DEV, tokenizer=tok).load_state_dict(sd)
        got = model.encode(strings, convert_to_numpy=False)
        assert got.shape == (len(strings), 64) and got.dtype == torch.float32 and got.device.type == "cuda"
        assert torch.equal(got, model.encode_ids(ids))
        as_np = model.encode(strings)
        assert isinstance(as_np, np.ndarray) and as_np.dtype == np.float32 and np.array_equal(as_np, got.cpu().numpy())
        one = model.encode(strings[2])
        assert one.shape == (64,) and np.array_equal(one, as_np[2])
    with pytest.raises(RuntimeError, match="tokenizer"):
        S.SentenceEncoder(synth.BERT_TINY, device=DEV).load_state_dict(sd).encode(["a"])


@pytest.mark.parametrize("name,budgets", [("tiny", [1, 2, 64, 129, 300]), ("minilm", [128, 200])])
def test_any_split_of_the_token_budget_gives_the_same_bits(golden_dir, name, budgets):
    _, seqs, _, _, _ = fixture(golden_dir, name)
    model = model_of(golden_dir, name)
    whole = model.encode_ids(seqs, token_budget=1 << 20)
    for b in budgets:
        assert torch.equal(model.encode_ids(seqs, token_budget=b), whole), b
    assert torch.equal(model.encode_ids(seqs[::-1], token_budget=97), whole.flip(0))


def test_duplicates_are_encoded_once_with_the_same_bits(golden_dir):
    _, seqs, _, _, _ = fixture(golden_dir, "tiny")
    model = model_of(golden_dir, "tiny")
    empty = [2, 3]
    many = [empty, seqs[2], empty, seqs[5], seqs[2], empty, seqs[0], empty]
    a = model.encode_ids(many, dedup=True)
    b = model.encode_ids(many, dedup=False)
    assert a.shape == (8, 64) and torch.equal(a, b)
    assert torch.equal(a[0], a[5]) and torch.equal(a[1], a[4]) and torch.equal(a[6], a[0])      # (seqs[0] is [CLS] [SEP] too)
    seen = []
    forward = model._forward
    model._forward = lambda s, **kw: (seen.append(len(s)), forward(s, **kw))[1]
    try:
        model.encode_ids(many)
    finally:
        del model._forward
    assert seen == [len({tuple(s) for s in many})]
    assert model.encode_ids([]).shape == (0, 64)
    with pytest.raises(ValueError, match="token ids"):
        model.encode_ids([[2, 97, 3]])
    with pytest.raises(ValueError, match="max_seq_length"):
        model.encode_ids([[2] * 129])


def write_model_dir(path, cfg, sd, lower=True, max_seq_length=128):
    os.makedirs(os.path.join(path, "1_Pooling"))
    dump = lambda name, obj: open(os.path.join(path, name), "w").write(json.dumps(obj))         # noqa: E731
    dump("config.json", dict(cfg, architectures=["BertModel"]))
    dump("tokenizer_config.json", dict(do_lower_case=lower))
    dump("sentence_bert_config.json", dict(max_seq_length=max_seq_length, do_lower_case=False))
    dump("modules.json", [dict(idx=0, name="0", path="", type="sentence_transformers.models.Transformer"),
                          dict(idx=1, name="1", path="1_Pooling", type="sentence_transformers.models.Pooling")])
    dump(os.path.join("1_Pooling", "config.json"), dict(word_embedding_dimension=cfg["hidden_size"],
                                                         pooling_mode_cls_token=False, pooling_mode_mean_tokens=True,
                                                         pooling_mode_max_tokens=False, pooling_mode_mean_sqrt_len_tokens=False))
    with open(os.path.join(path, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(synth.make_vocab()) + "\n")
    full = {"bert." + k: torch.from_numpy(v) for k, v in sd.items()}
    full["bert.embeddings.position_ids"] = torch.arange(cfg["max_position_embeddings"]).unsqueeze(0)
    full["bert.pooler.dense.weight"] = torch.zeros(cfg["hidden_size"], cfg["hidden_size"])
    full["bert.pooler.dense.bias"] = torch.zeros(cfg["hidden_size"])
    torch.save(full, os.path.join(path, "pytorch_model.bin"))


# MiniLM's width (the matcher's context rows are 384 wide) over the small vocabulary, two blocks: quick to seed and load
CFG_384 = dict(synth.BERT_MINILM, vocab_size=97, num_hidden_layers=2)
TRANSCRIPT = [(0.10, 0.30, "so"), (0.30, 0.52, "you"), (1.95, 2.40, "speak"), (3.60, 4.00, "and"), (3.97, 4.10, "we"),
              (4.50, 4.70, "hand"), (12.00, 12.20, "gestures"), (15.70, 15.99, "Hello")]


def test_model_directory_transcript_and_cli(tmp_path):
    sd = synth.make_bert_state_dict(8, CFG_384)
    mdir = str(tmp_path / "model")
    write_model_dir(mdir, CFG_384, sd, max_seq_length=64)
    model = S.load_sentence_model(mdir, device=DEV)
    assert model.max_seq_length == 64 and model.tokenizer.do_lower_case and model.dim == 384
    direct = S.SentenceEncoder(CFG_384, device=DEV, tokenizer=S.WordPiece(synth.make_vocab(), True, 64),
                               max_seq_length=64).load_state_dict(sd)
    texts = ["hello world", "", "we speak , and you ?", "hello " * 100]
    assert np.array_equal(model.encode(texts), direct.encode(texts))

    transcript = tmp_path / "clip.txt"
    transcript.write_text("".join("%r\t%r\t%s\n" % w for w in TRANSCRIPT), encoding="utf-8")
    M = 4
    context = S.txt_to_context(str(transcript), M, model)
    assert context.shape == (M, 30, 1, 384) and context.dtype == np.float32 and np.isfinite(context).all()
    sentences = S.code_sentences(S.read_transcript(str(transcript)), M)
    assert np.array_equal(context.reshape(M * 30, 384), model.encode(sentences))
    empty = model.encode("")
    assert np.array_equal(context[2, :, 0], np.broadcast_to(empty, (30, 384)))                   # the window without words
    assert not np.array_equal(context[0, 0, 0], empty)

    out = str(tmp_path / "test_txt.npz")
    assert S.main(["--transcript", str(transcript), "--model", mdir, "--windows", str(M), "--out", out, "--gpu", "0"]) == out
    assert np.array_equal(np.load(out)["context"], context)
    wavlm, wavvq = str(tmp_path / "wavlm.npz"), str(tmp_path / "wavvq.npz")
    np.savez(wavlm, wavlm=np.zeros((M, 199, 8), np.float32))
    np.savez(wavvq, wavvq=np.zeros((M, 398, 2), np.int64))
    side = data_processing.load_test_side(out, wavlm, wavvq)
    assert side["test_context"].shape == (M, 30, 384) and np.array_equal(side["test_context"], context[:, :, 0])


def test_load_refuses_a_directory_without_weights(tmp_path):
    mdir = str(tmp_path / "model")
    write_model_dir(mdir, synth.BERT_TINY, synth.make_bert_state_dict(8, synth.BERT_TINY))
    os.remove(os.path.join(mdir, "pytorch_model.bin"))
    with pytest.raises(FileNotFoundError, match="pytorch_model.bin"):
        S.load_sentence_model(mdir, device=DEV)
