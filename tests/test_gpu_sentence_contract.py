"""The three kernels of qpg_bert.hip, each alone, against the f64 restatement of tests/sentence_ref.py on packed ragged rows.

Tolerance: the project's rule (tests/test_gpu_wavlm.py) - the device result is within MARGIN = 8 x e32 of the f64 value,
e32 = max |NumPy f32 evaluation of sentence_ref - f64 evaluation| on the test's own inputs.  Each check prints its measured
ratio before asserting.  Shapes are a few hundred rows: every sentence length at which the attention kernel changes its
LDS capacity (16 / 32 / 64 / 128) or its number of query rounds (64 / 65), on both sides."""
import numpy as np
import pytest
import torch

from qpgesture_amd import _lib, synth
from qpgesture_amd import sentence as S
from tests import poison
from tests import sentence_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 8.0
CANARY = 7.0
LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128]


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def starts(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def err_word():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def check(name, got, ref64, ref32):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert np.isfinite(got).all(), name
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    err = float(np.abs(got - ref64).max())
    print("%s: err %.3e e32 %.3e ratio %.2f" % (name, err, e32, err / e32 if e32 > 0 else 0.0))
    assert err <= MARGIN * e32, "%s: |device - f64| = %.3e > %g x e32 (%.3e)" % (name, err, MARGIN, e32)


# ---- attention ------------------------------------------------------------------------------------------------------
def attention(qkv, lengths, H, max_len=None, extra_rows=3):
    """(out [R + extra_rows][H 32] with the canary behind row R, error word) of one launch."""
    R_ = int(sum(lengths))
    out = torch.full((R_ + extra_rows, H * 32), CANARY, dtype=torch.float32, device=DEV)
    err = err_word()
    _lib.call("qpg_bert_attention_f32", DEV, dev(qkv), dev(starts(lengths), np.int32), len(lengths), R_,
              max(lengths) if max_len is None else max_len, H, out, err)
    return out, int(err.item())


def attention_ref(qkv, lengths, H, dt):
    st = starts(lengths)
    return np.concatenate([R.attention_prescaled(qkv[a:b].astype(dt), H) for a, b in zip(st[:-1], st[1:])])


def qkv_case(H, kind):
    """plain: q, k N(0, 1) scaled to scores of spread ~2.  sharp: keys in near-duplicate pairs and q = 4 k, so that a
    query's own pair scores ~128 (exp overflows f32 unless the maximum is subtracted) and shares the weight."""
    rng = _rng(7, H, kind == "sharp")
    R_, D = sum(LENGTHS), H * 32
    q, k, v = (rng.standard_normal((R_, D)) for _ in range(3))
    if kind == "sharp":
        k[1::2] = k[0:-1:2][:len(k[1::2])] + 0.02 * rng.standard_normal(k[1::2].shape)
        q = 4.0 * k
    else:
        q = q * (2.0 / np.sqrt(32.0))
    return np.concatenate([q, k, v], 1).astype(np.float32)


@pytest.mark.parametrize("kind", ["plain", "sharp"])
@pytest.mark.parametrize("H", [2, 12])
def test_attention(H, kind):
    qkv = qkv_case(H, kind)
    out, err = attention(qkv, LENGTHS, H)
    R_ = sum(LENGTHS)
    assert err == 0 and bool((out[R_:] == CANARY).all())
    ref64, ref32 = attention_ref(qkv, LENGTHS, H, np.float64), attention_ref(qkv, LENGTHS, H, np.float32)
    if kind == "sharp":
        st = starts(LENGTHS)
        top = max(float((qkv[a:b, :32].astype(np.float64) @ qkv[a:b, H * 32:H * 32 + 32].astype(np.float64).T).max())
                  for a, b in zip(st[:-1], st[1:]))
        assert top > 100.0
    check("attention H=%d %s" % (H, kind), out[:R_], ref64, ref32)


def test_attention_does_not_depend_on_the_launch():
    """Every sentence alone (its own LDS capacity, max_len = its length) and among the others in reversed order: the
    same bits as in the mixed launch."""
    H = 12
    qkv = qkv_case(H, "plain")
    st = starts(LENGTHS)
    mixed, _ = attention(qkv, LENGTHS, H)
    order = list(range(len(LENGTHS)))[::-1]
    rev, err = attention(np.concatenate([qkv[st[i]:st[i + 1]] for i in order]), [LENGTHS[i] for i in order], H)
    assert err == 0
    at = 0
    for i in order:
        L = LENGTHS[i]
        assert torch.equal(rev[at:at + L], mixed[st[i]:st[i + 1]]), "reversed order, L = %d" % L
        at += L
        alone, err = attention(qkv[st[i]:st[i + 1]], [L], H)
        assert err == 0 and torch.equal(alone[:L], mixed[st[i]:st[i + 1]]), "alone, L = %d" % L


def test_attention_refuses_129_tokens():
    H = 2
    qkv = _rng(9).standard_normal((129, 3 * H * 32)).astype(np.float32)
    out = torch.full((129, H * 32), CANARY, dtype=torch.float32, device=DEV)
    err = err_word()
    with pytest.raises(_lib.Unsupported):
        _lib.call("qpg_bert_attention_f32", DEV, dev(qkv), dev(starts([129]), np.int32), 1, 129, 129, H, out, err)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and int(err.item()) == 0
    assert _lib.QPG_BERT_MAX_TOKENS == 128 == S.MAX_TOKENS and _lib.QPG_BERT_HEAD_DIM == 32 == S.HEAD_DIM


def test_attention_refuses_bounds_the_device_array_contradicts():
    """max_len says 64, the device's seq_start holds a sentence of 65: its rows are not written, the others are, and the
    error word says so."""
    H = 2
    lengths = [5, 65, 7]
    qkv = _rng(10).standard_normal((sum(lengths), 3 * H * 32)).astype(np.float32)
    out, err = attention(qkv, lengths, H, max_len=64)
    assert err == _lib.QPG_BERT_ERR_SEQ
    assert bool((out[5:70] == CANARY).all()) and not bool((out[:5] == CANARY).any()) and not bool((out[70:77] == CANARY).any())
    good, _ = attention(qkv, lengths, H)
    assert torch.equal(out[:5], good[:5]) and torch.equal(out[70:77], good[70:77])


# ---- embedding gather + LayerNorm ------------------------------------------------------------------------------------
def embed_case(D):
    rng = _rng(21, D)
    vocab, max_pos = 53, 128
    sd = {"embeddings.word_embeddings.weight": rng.standard_normal((vocab, D)) * 0.5,
          "embeddings.position_embeddings.weight": rng.standard_normal((max_pos, D)) * 0.5,
          "embeddings.token_type_embeddings.weight": rng.standard_normal((2, D)) * 0.5,
          "embeddings.LayerNorm.weight": rng.uniform(0.6, 1.4, D), "embeddings.LayerNorm.bias": rng.standard_normal(D) * 0.1}
    sd = {k: v.astype(np.float32) for k, v in sd.items()}
    lengths = [1, 128, 5, 3]
    seqs = [[int(i) for i in rng.integers(0, vocab, L)] for L in lengths]
    seqs[1][127], seqs[1][0], seqs[0][0], seqs[3][2] = vocab - 1, 0, vocab - 1, 0
    return sd, seqs, vocab, max_pos


def embed(sd, seqs, vocab, max_pos, D, max_len=None, extra_rows=5):
    e = "embeddings."
    lengths = [len(s) for s in seqs]
    R_ = sum(lengths)
    x = torch.full((R_ + extra_rows, D), CANARY, dtype=torch.float32, device=DEV)
    err = err_word()
    _lib.call("qpg_bert_embed_ln_f32", DEV, dev(np.concatenate(seqs), np.int32), dev(starts(lengths), np.int32), len(seqs),
              R_, max(lengths) if max_len is None else max_len, dev(sd[e + "word_embeddings.weight"]), vocab,
              dev(sd[e + "position_embeddings.weight"]), max_pos, dev(sd[e + "token_type_embeddings.weight"][0]),
              dev(sd[e + "LayerNorm.weight"]), dev(sd[e + "LayerNorm.bias"]), D, 1e-12, x, err)
    return x, int(err.item())


@pytest.mark.parametrize("D", [64, 384])
def test_embed_ln(D):
    """ids 0 and vocab - 1, position 127 (the table's last row), a one-token sentence; 137 rows: a tail block."""
    sd, seqs, vocab, max_pos = embed_case(D)
    x, err = embed(sd, seqs, vocab, max_pos, D)
    R_ = sum(len(s) for s in seqs)
    assert err == 0 and bool((x[R_:] == CANARY).all())

    def ref(dt):
        return np.concatenate([R.embed_ln(R.cast(sd, dt), s, 1e-12) for s in seqs])
    check("embed_ln D=%d" % D, x[:R_], ref(np.float64), ref(np.float32))


def test_embed_ln_refuses_what_it_cannot_read():
    D = 64
    sd, seqs, vocab, max_pos = embed_case(D)
    good, _ = embed(sd, seqs, vocab, max_pos, D)
    bad = [list(s) for s in seqs]
    bad[2][1], bad[3][0] = vocab, -1                          # rows 130 and 134
    x, err = embed(sd, bad, vocab, max_pos, D)
    assert err == _lib.QPG_BERT_ERR_ID
    keep = np.ones(len(good), bool)
    keep[[130, 134]] = False
    assert bool((x[[130, 134]] == CANARY).all()) and torch.equal(x[torch.from_numpy(keep).to(DEV)],
                                                                good[torch.from_numpy(keep).to(DEV)])
    with pytest.raises(RuntimeError, match="position table"):       # 128 tokens against a table of 127 rows: host check
        embed(sd, seqs, vocab, 127, D)
    short = dict(sd, **{"embeddings.position_embeddings.weight": sd["embeddings.position_embeddings.weight"][:127]})
    x, err = embed(short, seqs, vocab, 127, D, max_len=100)    # the device's bounds contradict max_len: sentence 1 refused
    assert err == _lib.QPG_BERT_ERR_SEQ and bool((x[1:129] == CANARY).all()) and torch.equal(x[129:137], good[129:137])


# ---- mean pool ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 100])
def test_mean_pool(D):
    lengths = [1, 128, 3]
    rng = _rng(31, D)
    x = (rng.standard_normal((sum(lengths), D)) + 0.5).astype(np.float32)
    out = torch.full((len(lengths) + 2, D), CANARY, dtype=torch.float32, device=DEV)
    err = err_word()
    _lib.call("qpg_bert_mean_pool_f32", DEV, dev(x), dev(starts(lengths), np.int32), len(lengths), sum(lengths), 128, D, out,
              err)
    assert int(err.item()) == 0 and bool((out[3:] == CANARY).all())
    assert torch.equal(out[0], dev(x[0]))                                                   # L = 1: the row itself
    st = starts(lengths)

    def ref(dt):
        return np.stack([R.mean_pool(x[a:b].astype(dt)) for a, b in zip(st[:-1], st[1:])])
    check("mean_pool D=%d" % D, out[:3], ref(np.float64), ref(np.float32))


# ---- scratch --------------------------------------------------------------------------------------------------------
def test_workspace_contents_do_not_matter():
    """The encoder's workspace (token rows, q | k | v, attention, FFN, ids, bounds) byte-filled with every pattern of
    tests/poison.py ahead of a pass: the same bits as on a fresh workspace."""
    model = S.SentenceEncoder(synth.BERT_TINY, device=DEV).load_state_dict(synth.make_bert_state_dict(3, synth.BERT_TINY))
    rng = _rng(41)
    seqs = [[2] + [int(i) for i in rng.integers(5, 97, L - 2)] + [3] for L in (2, 17, 33, 65, 128, 2, 9)]
    base = model._forward(seqs).clone()
    assert set(model._ws) == {"x", "qkv", "att", "ffn", "ids", "seq", "err"}
    for name, pattern in poison.FILLS.items():
        for key, buf in model._ws.items():
            if key != "err":                                  # (the error word is state, zero between calls)
                poison.fill(buf, pattern)
        out = torch.empty_like(base)
        poison.fill(out, pattern)
        assert torch.equal(model._forward(seqs, out=out), base), name
