"""Writes tests/golden/sentence_tiny.npz, sentence_minilm.npz and sentence_tokens.npz.  Needs `transformers` (run where
it is installed; the tests read the committed outputs only).

    python tests/golden/make_golden_sentence.py

The model is transformers.BertModel(config, add_pooling_layer=False) with eager attention - the class sentence-transformers
wraps - loaded with synth.make_bert_state_dict's seeded weights, run on PADDED batches with an attention mask in f32 and,
after .double(), in f64, then mean-pooled with the mask as sentence-transformers' Pooling does.  Committed per fixture: the
input ids, the f64 pooled embeddings, the f64 embedding-stage output and block 0's output on every TAP_STEP-th packed row,
and for each of the three e32 = max |f32 run - f64 run| (over all rows, not only the kept ones).
Before anything is written the generator asserts the premise of the packed layout: a sentence run alone equals the same
sentence inside the padded batch to 1e-12 in f64.

sentence_tokens.npz: what transformers.BertTokenizer gives on synth.make_vocab() for STRINGS, with and without
lower-casing, truncated at 128 tokens."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from qpgesture_amd import synth  # noqa: E402

LENGTHS = [2, 3, 9, 31, 32, 33, 63, 64, 65, 127, 128]
TAP_STEP = 11
SEEDS = {"tiny": 11, "minilm": 12}
CFGS = {"tiny": synth.BERT_TINY, "minilm": synth.BERT_MINILM}
CLS, SEP = 2, 3                      # their rows in synth.make_vocab()

STRINGS = ["", " hello world ", "hello, world!", "!!!...??", "Hello The I", "café naïve", "中文 hello中world",
           "zzzqqq xylophone9", "a" * 101, "a" * 100, "hello world " * 80, "the gesture speaking", "unspeakable handed",
           "so-so (we) speak.", "tab\tand\nnewline", "it's", "I speak", "HELLO WORLD", "hello\u00a0world",
           "x\u0000y\ufffdz\u200bw", "gestures walked slowly", "  ", "we speak , and you ?"]


def make_ids(name):
    rng = np.random.Generator(np.random.PCG64(SEEDS[name] + 100))
    vocab = CFGS[name]["vocab_size"]
    seqs = []
    for n, L in enumerate(LENGTHS):
        body = rng.integers(5, vocab, L - 2)
        if L >= 9:
            body[0], body[1] = vocab - 1, 0            # the table's last row and its first ([PAD] as an ordinary token)
        seqs.append([CLS] + [int(i) for i in body] + [SEP])
    return seqs


def run(model, seqs, dtype):
    """Padded batch -> (pooled (S, D), embed rows (R, D), block-0 rows (R, D)), packed (padding rows dropped)."""
    import torch
    S, T = len(seqs), max(len(s) for s in seqs)
    ids = torch.zeros((S, T), dtype=torch.long)
    mask = torch.zeros((S, T), dtype=torch.long)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = torch.tensor(s)
        mask[i, :len(s)] = 1
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    last, hs = out.last_hidden_state, out.hidden_states
    m = mask.to(dtype).unsqueeze(-1)
    pooled = (last * m).sum(1) / torch.clamp(m.sum(1), min=1e-9)
    keep = mask.bool()
    return pooled.numpy(), hs[0][keep].numpy(), hs[1][keep].numpy()


def build_model(cfg, sd):
    import torch
    from transformers import BertConfig, BertModel
    config = BertConfig(**{k: v for k, v in cfg.items() if k != "model_type"})
    config._attn_implementation = "eager"
    model = BertModel(config, add_pooling_layer=False).eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    return model


def make_fixture(name):
    import torch
    cfg = CFGS[name]
    sd = synth.make_bert_state_dict(SEEDS[name], cfg)
    seqs = make_ids(name)
    model = build_model(cfg, sd)
    p32, e32_, l32 = run(model, seqs, torch.float32)
    model = model.double()
    p64, e64, l64 = run(model, seqs, torch.float64)
    for i, s in enumerate(seqs):                       # the premise of the packed form
        alone = run(model, [s], torch.float64)[0][0]
        assert np.abs(alone - p64[i]).max() <= 1e-12, (name, i, np.abs(alone - p64[i]).max())
    rows = np.arange(0, e64.shape[0], TAP_STEP)
    seq_start = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    out = dict(ids=np.concatenate(seqs).astype(np.int32), seq_start=seq_start, seed=np.int64(SEEDS[name]),
               pooled=p64, e32=np.float64(np.abs(p32 - p64).max()),
               tap_rows=rows.astype(np.int32),
               embed=e64[rows], e32_embed=np.float64(np.abs(e32_ - e64).max()),
               layer0=l64[rows], e32_layer0=np.float64(np.abs(l32 - l64).max()))
    path = os.path.join(HERE, "sentence_%s.npz" % name)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; e32 %.3e embed %.3e layer0 %.3e; |pooled| max %.2f" % (
        out["e32"], out["e32_embed"], out["e32_layer0"], np.abs(p64).max()))


def make_tokens():
    from transformers import BertTokenizer
    with tempfile.TemporaryDirectory() as d:
        vocab = os.path.join(d, "vocab.txt")
        with open(vocab, "w", encoding="utf-8") as f:
            f.write("\n".join(synth.make_vocab()) + "\n")
        out = dict(strings=np.array(STRINGS))
        for lower in (True, False):
            tok = BertTokenizer(vocab, do_lower_case=lower)
            ids = [tok(s.strip(), truncation=True, max_length=128)["input_ids"] for s in STRINGS]
            key = "lower" if lower else "cased"
            out["ids_" + key] = np.concatenate(ids).astype(np.int32)
            out["start_" + key] = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.int32)
            print(key, [len(i) for i in ids])
    np.savez_compressed(os.path.join(HERE, "sentence_tokens.npz"), **out)


if __name__ == "__main__":
    make_tokens()
    for fixture in ("tiny", "minilm"):
        make_fixture(fixture)
