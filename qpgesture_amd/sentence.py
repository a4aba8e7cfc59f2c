"""Sentence embeddings on the GPU: the `context` column of the matcher's text track, what the reference's
make_txt_dataset (process/make_beat_dataset.py:446-447, :538-566) gets from
`SentenceTransformer('paraphrase-MiniLM-L6-v2').encode([sentence])`, one call per code slot.

    from qpgesture_amd.sentence import load_sentence_model, txt_to_context
    model = load_sentence_model("paraphrase-MiniLM-L6-v2/", device="cuda:0")     # a sentence-transformers model directory
    emb = model.encode(["so you can see", ""])                                   # (2, 384) f32 NumPy
    context = txt_to_context("Transcripts/clip.txt", n_windows, model)           # (M, 30, 1, 384) f32

    python -m qpgesture_amd.sentence --transcript clip.txt --model DIR --windows M --out test_txt.npz [--gpu 0]

WordPiece is the package's own BertTokenizer (no runtime dependency on transformers); SentenceEncoder is a BERT-shaped
post-LN encoder with mean-token pooling, a chain of qpg_bert_* and qpg_wavlm_gemm / layernorm kernels of include/qpg.h over
PACKED RAGGED ROWS: no padding, no mask, and a sentence's embedding does not depend on what it is
batched with - so identical sentences are encoded once.  There is no torch fallback: a configuration the kernels do not
take raises NotImplementedError naming the field."""
import argparse
import json
import os
import unicodedata

import numpy as np

HEAD_DIM = 32             # QPG_BERT_HEAD_DIM
MAX_TOKENS = 128          # QPG_BERT_MAX_TOKENS
TOKEN_BUDGET = 32768      # token rows per pass (the workspace is 4 (5 D + F) bytes per row: 0.45 GB at MiniLM size)

CFG_DEFAULTS = dict(hidden_act="gelu", position_embedding_type="absolute", layer_norm_eps=1e-12, type_vocab_size=2,
                    max_position_embeddings=512)


def _as_dict(config):
    return dict(CFG_DEFAULTS, **(config if isinstance(config, dict) else config.__dict__))


def check_supported(config, max_seq_length=MAX_TOKENS):
    """Raise NotImplementedError naming the first field the kernels do not take (config: a config.json dict;
    max_seq_length: sentence_bert_config.json's)."""
    c = dict(_as_dict(config), max_seq_length=max_seq_length)

    def need(field, ok, what):
        if not ok:
            raise NotImplementedError("sentence model field %s = %r is not supported (%s)" % (field, c.get(field), what))
    for field in ("hidden_size", "num_attention_heads", "intermediate_size", "num_hidden_layers", "vocab_size"):
        need(field, isinstance(c.get(field), int) and c[field] >= 1, "a positive integer is required")
    need("hidden_act", c["hidden_act"] == "gelu", "only 'gelu' (the exact erf form)")
    need("position_embedding_type", c["position_embedding_type"] in (None, "absolute"), "only absolute position embeddings")
    D, H, F = c["hidden_size"], c["num_attention_heads"], c["intermediate_size"]
    need("hidden_size", D % 16 == 0, "a multiple of 16")
    need("intermediate_size", F % 16 == 0, "a multiple of 16")
    need("num_attention_heads", H * HEAD_DIM == D, "hidden_size / num_attention_heads must be %d" % HEAD_DIM)
    need("max_seq_length", 2 <= int(max_seq_length) <= min(MAX_TOKENS, c["max_position_embeddings"]),
         "from 2 to %d tokens, and no more than max_position_embeddings" % MAX_TOKENS)


# ---- the tokenizer ---------------------------------------------------------------------------------------------------
def _is_whitespace(ch):
    return ch in " \t\n\r" or unicodedata.category(ch) in ("Zs", "Zl", "Zp")


def _is_control(ch):
    return ch not in "\t\n\r" and unicodedata.category(ch).startswith("C")


def _is_punctuation(ch):
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(cp):
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F or
            0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


class WordPiece:
    """BertTokenizer: text clean-up (NUL, U+FFFD and control characters dropped, every whitespace a blank), CJK characters
    as words of their own, with do_lower_case accents stripped (NFD, combining marks dropped) and lower-casing, whitespace
    split, every punctuation character a word of its own, then greedy longest-match word pieces ('##' continues a word; a
    word of more than 100 characters, or one with a part no piece matches, is [UNK]).  encode() adds [CLS] .. [SEP] and
    truncates to max_seq_length tokens, both specials included.  `vocab`: a vocab.txt path or the list of its lines.
    Special tokens written out in the text ("[SEP]") are not recognised: they tokenize like any other text."""

    MAX_WORD_CHARS = 100

    def __init__(self, vocab, do_lower_case=True, max_seq_length=MAX_TOKENS):
        if isinstance(vocab, (str, bytes, os.PathLike)):
            with open(vocab, "r", encoding="utf-8") as f:
                vocab = [line.rstrip("\n") for line in f]
        self.vocab = {tok: i for i, tok in enumerate(vocab)}
        self.do_lower_case = bool(do_lower_case)
        self.max_seq_length = int(max_seq_length)
        for tok in ("[UNK]", "[CLS]", "[SEP]"):
            if tok not in self.vocab:
                raise ValueError("WordPiece: the vocabulary lacks %s" % tok)
        self.unk_id, self.cls_id, self.sep_id = (self.vocab[t] for t in ("[UNK]", "[CLS]", "[SEP]"))

    def words(self, text):
        """The words ahead of the word-piece step."""
        out = []
        for ch in text:
            cp = ord(ch)
            if cp == 0 or cp == 0xFFFD or _is_control(ch):
                continue
            if _is_whitespace(ch):
                out.append(" ")
            elif _is_cjk(cp):
                out.append(" " + ch + " ")
            else:
                out.append(ch)
        text = "".join(out)
        if self.do_lower_case:
            text = "".join(ch for ch in unicodedata.normalize("NFD", text) if unicodedata.category(ch) != "Mn").lower()
        words = []
        for word in text.split():
            cur = ""
            for ch in word:
                if _is_punctuation(ch):
                    if cur:
                        words.append(cur)
                    words.append(ch)
                    cur = ""
                else:
                    cur += ch
            if cur:
                words.append(cur)
        return words

    def pieces(self, word):
        if len(word) > self.MAX_WORD_CHARS:
            return [self.unk_id]
        out, start = [], 0
        while start < len(word):
            end = len(word)
            while end > start:
                piece = ("##" if start else "") + word[start:end]
                if piece in self.vocab:
                    break
                end -= 1
            if end == start:
                return [self.unk_id]
            out.append(self.vocab[piece])
            start = end
        return out

    def encode(self, text, max_seq_length=None):
        """[CLS] pieces [SEP] ids of str(text).strip(), at most max_seq_length of them."""
        n = self.max_seq_length if max_seq_length is None else int(max_seq_length)
        ids = [i for w in self.words(str(text).strip()) for i in self.pieces(w)]
        return [self.cls_id] + ids[:max(n - 2, 0)] + [self.sep_id]


# ---- the encoder -----------------------------------------------------------------------------------------------------
class SentenceEncoder:
    """SentenceEncoder(config, device): transformers' BertModel(config, add_pooling_layer=False).eval() followed by
    sentence-transformers' mean-token pooling.  `tokenizer` (a WordPiece) is needed by encode(), not by encode_ids()."""

    def __init__(self, config, device="cuda:0", tokenizer=None, max_seq_length=MAX_TOKENS, token_budget=TOKEN_BUDGET):
        import torch
        check_supported(config, max_seq_length)
        self.config = _as_dict(config)
        self.device = torch.device(device)
        self.tokenizer = tokenizer
        self.max_seq_length = int(max_seq_length)
        self.token_budget = int(token_budget)
        self.p = None
        self._ws = {}

    @property
    def dim(self):
        return self.config["hidden_size"]

    def load_state_dict(self, sd):
        import torch
        c = self.config
        D, F, V = c["hidden_size"], c["intermediate_size"], c["vocab_size"]
        sd = {(k[5:] if k.startswith("bert.") else k): v for k, v in sd.items()}

        def get(name, shape):
            if name not in sd:
                raise KeyError("sentence model state_dict lacks %r" % name)
            v = sd[name]
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if tuple(v.shape) != tuple(shape):
                raise ValueError("%s has shape %s, the config says %s" % (name, tuple(v.shape), tuple(shape)))
            return v

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)

        e = "embeddings."
        p = dict(word=dev(get(e + "word_embeddings.weight", (V, D))),
                 pos=dev(get(e + "position_embeddings.weight", (c["max_position_embeddings"], D))),
                 type0=dev(get(e + "token_type_embeddings.weight", (c["type_vocab_size"], D))[0]),
                 ln_g=dev(get(e + "LayerNorm.weight", (D,))), ln_b=dev(get(e + "LayerNorm.bias", (D,))), layers=[])
        scaling = HEAD_DIM ** -0.5               # (not a power of two: scaled in f64, rounded to f32 once)
        for i in range(c["num_hidden_layers"]):
            pre = "encoder.layer.%d." % i
            a = pre + "attention.self."
            wq = get(a + "query.weight", (D, D)).astype(np.float64) * scaling
            bq = get(a + "query.bias", (D,)).astype(np.float64) * scaling
            p["layers"].append(dict(
                qkv_w=dev(np.concatenate([wq, get(a + "key.weight", (D, D)), get(a + "value.weight", (D, D))], 0)),
                qkv_b=dev(np.concatenate([bq, get(a + "key.bias", (D,)), get(a + "value.bias", (D,))], 0)),
                out_w=dev(get(pre + "attention.output.dense.weight", (D, D))),
                out_b=dev(get(pre + "attention.output.dense.bias", (D,))),
                ln1_g=dev(get(pre + "attention.output.LayerNorm.weight", (D,))),
                ln1_b=dev(get(pre + "attention.output.LayerNorm.bias", (D,))),
                fc1_w=dev(get(pre + "intermediate.dense.weight", (F, D))), fc1_b=dev(get(pre + "intermediate.dense.bias", (F,))),
                fc2_w=dev(get(pre + "output.dense.weight", (D, F))), fc2_b=dev(get(pre + "output.dense.bias", (D,))),
                ln2_g=dev(get(pre + "output.LayerNorm.weight", (D,))), ln2_b=dev(get(pre + "output.LayerNorm.bias", (D,)))))
        self.p = p
        return self

    # ---- the forward pass
    def _workspace(self, R, S):
        """Device buffers for a pass of R token rows in S sentences; kept, and reused by every later pass that fits."""
        import torch
        D, F = self.config["hidden_size"], self.config["intermediate_size"]
        need = dict(x=(R * D, torch.float32), qkv=(R * 3 * D, torch.float32), att=(R * D, torch.float32),
                    ffn=(R * F, torch.float32), ids=(R, torch.int32), seq=(S + 1, torch.int32))
        for k, (n, dt) in need.items():
            if k not in self._ws or self._ws[k].numel() < n:
                self._ws[k] = torch.empty(max(n, 4), dtype=dt, device=self.device)
        if "err" not in self._ws:
            self._ws["err"] = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._ws

    def _check_err(self):
        from . import _lib
        word = int(self._ws["err"].item())
        if word:
            self._ws["err"].zero_()
            what = [n for n, bit in (("sentence bounds", _lib.QPG_BERT_ERR_SEQ), ("a token id", _lib.QPG_BERT_ERR_ID),
                                     ("a token position", _lib.QPG_BERT_ERR_POS)) if word & bit]
            raise RuntimeError("SentenceEncoder: the kernels refused %s (error word %d)" % (" and ".join(what), word))

    def _forward(self, seqs, out=None, on_stage=None, check=True):
        """The launches of one pass: `seqs`, a list of id lists, in the order given -> (S, D) f32 on the device (written
        to `out` if given).  on_stage(name, view), if given, is called behind every launch with a view of its output:
        "start" (None), "embed" (the packed [R][D] rows), per block "layer<i>.qkv", ".att", ".out", ".ln1", ".fc1", ".fc2"
        and "layer<i>" (the block's output rows), then "pooled" (S, D).  A view is valid until the next launch (the
        blocks run in place).  The tests copy the views, tools/bench_sentence.py records a device event per stage.
        check=False leaves the device's error word unread (encode_ids reads it once, behind its last pass)."""
        import torch
        from . import _lib
        if self.p is None:
            raise RuntimeError("SentenceEncoder: load_state_dict() first")
        c, dev, p = self.config, self.device, self.p
        D, F, H = c["hidden_size"], c["intermediate_size"], c["num_attention_heads"]
        eps = float(c["layer_norm_eps"])
        lens = np.fromiter((len(s) for s in seqs), np.int64, len(seqs))
        S = len(seqs)
        if S == 0:
            return torch.empty((0, D), dtype=torch.float32, device=dev) if out is None else out
        if lens.min() < 1:
            raise ValueError("SentenceEncoder: a sentence without tokens")
        R, max_len = int(lens.sum()), int(lens.max())
        if max_len > MAX_TOKENS:
            raise NotImplementedError("SentenceEncoder: a sentence of %d tokens, the attention kernel takes at most %d"
                                      % (max_len, MAX_TOKENS))
        seq_host = np.zeros(S + 1, np.int32)
        np.cumsum(lens, out=seq_host[1:])
        ids_host = np.fromiter((i for s in seqs for i in s), np.int32, R)
        if ids_host.min() < 0 or ids_host.max() >= c["vocab_size"]:
            raise ValueError("SentenceEncoder: token ids must lie in [0, %d)" % c["vocab_size"])
        ws = self._workspace(R, S)
        ids, seq, err = ws["ids"][:R], ws["seq"][:S + 1], ws["err"]
        ids.copy_(torch.from_numpy(ids_host))
        seq.copy_(torch.from_numpy(seq_host))
        x, qkv, att, ffn = ws["x"], ws["qkv"], ws["att"], ws["ffn"]
        if out is None:
            out = torch.empty((S, D), dtype=torch.float32, device=dev)
        call = _lib.call

        def mark(stage, t=None):
            if on_stage is not None:
                on_stage(stage, x[:R * D].view(R, D) if t is None else t)

        def gemm(A, lda, W, bias, res, o, ldc, N, K, gelu=0):
            call("qpg_wavlm_gemm_f32", dev, A, lda, W, bias, res, o, ldc, R, N, K, gelu, 1, 1, 0, 0, 0, 0, 0, 0)

        def ln(g, b):
            call("qpg_wavlm_layernorm_f32", dev, x, g, b, R, D, eps, 0, x)

        if on_stage is not None:
            on_stage("start", None)
        call("qpg_bert_embed_ln_f32", dev, ids, seq, S, R, max_len, p["word"], c["vocab_size"], p["pos"],
             c["max_position_embeddings"], p["type0"], p["ln_g"], p["ln_b"], D, eps, x, err)
        mark("embed")
        for i, L in enumerate(p["layers"]):
            blk = "layer%d." % i
            gemm(x, D, L["qkv_w"], L["qkv_b"], None, qkv, 3 * D, 3 * D, D)
            mark(blk + "qkv", qkv[:R * 3 * D].view(R, 3 * D))
            call("qpg_bert_attention_f32", dev, qkv, seq, S, R, max_len, H, att, err)
            mark(blk + "att", att[:R * D].view(R, D))
            gemm(att, D, L["out_w"], L["out_b"], x, x, D, D, D)             # x + dense(attention)
            mark(blk + "out")
            ln(L["ln1_g"], L["ln1_b"])
            mark(blk + "ln1")
            gemm(x, D, L["fc1_w"], L["fc1_b"], None, ffn, F, F, D, gelu=1)
            mark(blk + "fc1", ffn[:R * F].view(R, F))
            gemm(ffn, F, L["fc2_w"], L["fc2_b"], x, x, D, D, F)             # x + fc2(gelu(fc1 x))
            mark(blk + "fc2")
            ln(L["ln2_g"], L["ln2_b"])
            mark("layer%d" % i)
        call("qpg_bert_mean_pool_f32", dev, x, seq, S, R, max_len, D, out, err)
        mark("pooled", out)
        if check:
            self._check_err()
        return out

    def encode_ids(self, ids_list, token_budget=None, dedup=True, on_stage=None):
        """(S, D) f32 device tensor: the embeddings of S id lists ([CLS] .. [SEP] included), in the order given.  Identical
        lists are encoded once (dedup), the distinct ones are sorted by length and cut into passes of at most
        token_budget token rows (at least one sentence each): neither changes a bit of any result.  on_stage: handed to
        every pass (_forward)."""
        import torch
        budget = self.token_budget if token_budget is None else int(token_budget)
        seqs = [tuple(int(i) for i in s) for s in ids_list]
        D = self.config["hidden_size"]
        if not seqs:
            return torch.empty((0, D), dtype=torch.float32, device=self.device)
        too_long = max(len(s) for s in seqs)
        if too_long > self.max_seq_length:
            raise ValueError("SentenceEncoder: a sentence of %d tokens, max_seq_length is %d" % (too_long,
                                                                                               self.max_seq_length))
        if dedup:
            index = {}
            which = np.fromiter((index.setdefault(s, len(index)) for s in seqs), np.int64, len(seqs))
            distinct = list(index)
        else:
            which, distinct = np.arange(len(seqs)), seqs
        order = sorted(range(len(distinct)), key=lambda k: len(distinct[k]))
        rank = np.empty(len(order), np.int64)
        rank[order] = np.arange(len(order))
        out = torch.empty((len(distinct), D), dtype=torch.float32, device=self.device)
        k0 = 0
        while k0 < len(order):
            k1, rows = k0, 0
            while k1 < len(order) and (k1 == k0 or rows + len(distinct[order[k1]]) <= budget):
                rows += len(distinct[order[k1]])
                k1 += 1
            self._forward([distinct[k] for k in order[k0:k1]], out=out[k0:k1], on_stage=on_stage, check=False)
            k0 = k1
        self._check_err()
        return out.index_select(0, torch.from_numpy(rank[which]).to(self.device))

    def encode(self, sentences, batch_size=32, convert_to_numpy=True, token_budget=None):
        """SentenceTransformer.encode: a list of sentences -> (S, D) f32, a single str -> (D,); NumPy, or with
        convert_to_numpy=False a device tensor.  batch_size is accepted for the signature: the work is cut by token rows
        (token_budget), not by sentences."""
        if self.tokenizer is None:
            raise RuntimeError("SentenceEncoder.encode: no tokenizer (load_sentence_model sets one; or use encode_ids)")
        single = isinstance(sentences, str)
        texts = [sentences] if single else list(sentences)
        emb = self.encode_ids([self.tokenizer.encode(t, self.max_seq_length) for t in texts], token_budget=token_budget)
        if single:
            emb = emb[0]
        return emb.cpu().numpy() if convert_to_numpy else emb


def _read_json(path, default=None):
    if not os.path.exists(path):
        if default is None:
            raise FileNotFoundError("sentence model directory lacks %s" % os.path.basename(path))
        return default
    with open(path, "r", encoding="utf-8") as f:
        return json.load(f)


def load_sentence_model(path, device="cuda:0"):
    """A sentence-transformers model directory (Transformer + mean-token Pooling) -> a loaded SentenceEncoder with its
    tokenizer: config.json, vocab.txt, tokenizer_config.json (do_lower_case), sentence_bert_config.json (max_seq_length),
    1_Pooling/config.json, modules.json and pytorch_model.bin or model.safetensors."""
    import torch
    for mod in _read_json(os.path.join(path, "modules.json"), default=[]):
        kind = str(mod.get("type", "")).rsplit(".", 1)[-1]
        if kind not in ("Transformer", "Pooling"):
            raise NotImplementedError("sentence model module %r is not supported (only Transformer and Pooling)" % mod.get("type"))
    pool = _read_json(os.path.join(path, "1_Pooling", "config.json"))
    modes = {k: v for k, v in pool.items() if k.startswith("pooling_mode_")}
    if not modes.get("pooling_mode_mean_tokens") or any(v for k, v in modes.items() if k != "pooling_mode_mean_tokens"):
        raise NotImplementedError("sentence model pooling %r is not supported (only pooling_mode_mean_tokens)"
                                  % sorted(k for k, v in modes.items() if v))
    config = _read_json(os.path.join(path, "config.json"))
    tok_cfg = _read_json(os.path.join(path, "tokenizer_config.json"), default={})
    sb_cfg = _read_json(os.path.join(path, "sentence_bert_config.json"), default={})
    max_seq_length = int(sb_cfg.get("max_seq_length") or MAX_TOKENS)
    do_lower = bool(sb_cfg.get("do_lower_case", False) or tok_cfg.get("do_lower_case", True))
    tokenizer = WordPiece(os.path.join(path, "vocab.txt"), do_lower_case=do_lower, max_seq_length=max_seq_length)
    if len(tokenizer.vocab) > config["vocab_size"]:
        raise ValueError("vocab.txt has %d entries, config.json's vocab_size is %d" % (len(tokenizer.vocab),
                                                                                     config["vocab_size"]))
    model = SentenceEncoder(config, device=device, tokenizer=tokenizer, max_seq_length=max_seq_length)
    if os.path.exists(os.path.join(path, "pytorch_model.bin")):
        sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu")
    elif os.path.exists(os.path.join(path, "model.safetensors")):
        try:
            from safetensors.numpy import load_file
        except ImportError:
            raise RuntimeError("%s holds model.safetensors only and the safetensors package is not installed: install it, or "
                               "convert the weights to pytorch_model.bin" % path)
        sd = load_file(os.path.join(path, "model.safetensors"))
    else:
        raise FileNotFoundError("sentence model directory %s has neither pytorch_model.bin nor model.safetensors" % path)
    return model.load_state_dict(sd)


# ---- the text half of make_txt_dataset -------------------------------------------------------------------------------
def read_transcript(path):
    """[[start, end, word], ...] of a transcript's `start \\t end \\t word` lines (make_beat_dataset.py:490-496; the times
    are read with float(), not eval())."""
    words = []
    with open(path, "r", encoding="utf-8") as f:
        for line in f.readlines():
            content = line.strip().split("\t")
            if content == [""]:
                continue
            if len(content) < 3:
                raise ValueError("%s: not a `start \\t end \\t word` line: %r" % (path, line))
            words.append([float(content[0]), float(content[1]), content[2]])
    return words


def code_sentences(words, n_windows, n_frames=240, fps=60, num_frames_code=30):
    """The n_windows x num_frames_code sentences the reference encodes (make_beat_dataset.py:538-564, mode
    'noduplication': stride = n_frames), window-major.  Its float operations are kept as they are: the words are consumed
    across windows while their midpoint lies before the window's end; a word's slot is
    int((start % 4 + (end % 4 or 4)) * 60 / 2 / 8) - the literal 60 included - so a word that straddles a window boundary
    lands mid-window, as there; a slot's sentence joins the words of slots j - 3 .. j + 3 with ' '."""
    stride = n_frames
    step_sz = int(stride / num_frames_code)
    stride_time = stride // fps
    out, k = [], 0
    for i in range(n_windows):
        end_time = (i * stride + n_frames) / fps
        slots = [[] for _ in range(num_frames_code)]
        while k < len(words) and (words[k][0] + words[k][1]) / 2 < end_time:
            tmp = words[k]
            k += 1
            slots[int((tmp[0] % stride_time + (tmp[1] % stride_time if tmp[1] % stride_time != 0 else stride_time))
                      * 60 / 2 / step_sz)].append(tmp[2])
        for j in range(num_frames_code):
            near = slots[(j - 3 if j - 3 > 0 else 0):(j + 4 if j + 4 < num_frames_code else num_frames_code)]
            out.append(" ".join(w for slot in near for w in slot))
    return out


def txt_to_context(transcript, n_windows, model, n_frames=240, fps=60, num_frames_code=30):
    """(n_windows, num_frames_code, 1, D) f32: the `context` array of the reference's *_txt.npz for one transcript
    (a path, or the list read_transcript returns)."""
    words = read_transcript(transcript) if isinstance(transcript, (str, bytes, os.PathLike)) else transcript
    sentences = code_sentences(words, n_windows, n_frames, fps, num_frames_code)
    emb = model.encode(sentences)
    return np.ascontiguousarray(emb.reshape(n_windows, num_frames_code, 1, emb.shape[-1]), np.float32)


def build_parser():
    ap = argparse.ArgumentParser(description="sentence embeddings of a transcript's code slots: the matcher's context column")
    ap.add_argument("--transcript", required=True, help="lines of start <tab> end <tab> word")
    ap.add_argument("--model", required=True, help="a sentence-transformers model directory")
    ap.add_argument("--windows", type=int, required=True, help="number of 4 s windows")
    ap.add_argument("--out", default="test_txt.npz")
    ap.add_argument("--gpu", type=str, default="0")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    model = load_sentence_model(args.model, device="cuda:%s" % args.gpu)
    context = txt_to_context(args.transcript, args.windows, model)
    np.savez_compressed(args.out, context=context)
    print(args.out, context.shape)
    return args.out


if __name__ == "__main__":
    main()
