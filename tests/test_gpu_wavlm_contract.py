"""The qpg_wavlm_* entry points of qpg_wavlm.hip, called directly, against the f64 values and the ENTRYWISE bounds of
tests/wavlm_ref.py (derivations there; tests/test_wavlm_contract_cpu.py shows that a correct f32 evaluation is inside
them and that seven edge mistakes are outside).  The cases are wavlm_ref's tables: the smallest shapes at which each
path can go wrong - tile edges of the GEMM (128 x 128 block, 32 x 32 matrix-core tiles, 16-wide k-tiles, 512-wide
chunks), the 16-query blocks and 64-lane passes of the attention, the 4 rows per block of the LayerNorm, the 256 threads
per block of the gate, the 8 frames per thread of conv0.

Every output buffer is pre-filled with a sentinel and is longer than the result; the padding of every input (between
A's rows when lda > K, behind the last row, the residual's padding columns) holds NaN, so a read outside a row's floats
shows in a stored result and a write outside the result in the sentinel.  All comparisons are entry by entry,
err <= bound; the largest err / bound of each case is printed as a line starting WAVLMCONTRACT
(profiles/wavlm_contract.md).  Placement independence is bit for bit."""
import numpy as np
import pytest
import torch

from qpgesture_amd import _lib, synth
from qpgesture_amd import wavlm as W
from tests import wavlm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = R.SENTINEL
NAN_TAIL = np.full(16, np.nan, np.float32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def dev_padded(a):
    """a, flat, with NaN behind it."""
    return dev(np.concatenate([np.asarray(a, np.float32).ravel(), NAN_TAIL]))


def sentinel(n, extra=8):
    return torch.full((n + extra,), SENT, dtype=torch.float32, device=DEV)


def say(name, r):
    print("WAVLMCONTRACT %s: err/bound %.3f" % (name, r))


def held(name, got, val, bnd):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == val.shape, (name, got.shape, val.shape)
    r = R.ratio(got, val, bnd)
    say(name, r)
    assert r <= 1.0, (name, r)


def tail_untouched(buf, n):
    return bool((buf[n:] == SENT).all())


# ---- GEMM -----------------------------------------------------------------------------------------------------------
def gemm_call(p, a, w, bias, r, out, M=None):
    _lib.call("qpg_wavlm_gemm_f32", DEV, a, p["lda"], w, bias, r, out, p["ldc"], p["M"] if M is None else M, p["N"],
              p["K"], p["gelu"], p["n_outer"], p["n_inner"], p["a_outer"], p["a_inner"], p["w_inner"], p["bias_inner"],
              p["c_outer"], p["c_inner"])


def run_gemm(p):
    """The problem's call on copies of its buffers -> the whole output buffer (device tensor)."""
    out = dev(p["out0"])
    r = out if p["inplace"] else dev(p["r"])
    gemm_call(p, dev(p["a"]), dev(p["w"]), dev(p["bias"]), r, out)
    return out


@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_gemm(name):
    p = R.gemm_case(name)
    got = run_gemm(p).cpu().numpy()
    idx = R.gemm_index(p)["out"]
    val, bnd = R.gemm_problem_bound(p)
    outside = np.ones(len(got), bool)
    outside[idx] = False
    assert outside.sum() >= 8 and np.array_equal(got[outside], p["out0"][outside]), name     # padding columns, the tail
    held("gemm " + name, got[idx], val, bnd)


@pytest.mark.parametrize("what", ["lda % 4", "A off by one float", "ldc < N", "65536 problems"])
def test_gemm_refusals_leave_the_output_untouched(what):
    p = R.gemm_problem("refusal", 8, 8, 32)
    a = dev(np.zeros(4096, np.float32))
    out = sentinel(4096)
    if what == "lda % 4":
        p["lda"] = 34
    elif what == "A off by one float":
        a = a[1:]
    elif what == "ldc < N":
        p["ldc"] = 7
    else:
        p.update(n_outer=256, n_inner=256)
    with pytest.raises(RuntimeError, match="65535" if what == "65536 problems" else "16-byte aligned"):
        gemm_call(p, a, dev(p["w"]), dev(p["bias"]), None, out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_gemm_rows_do_not_depend_on_the_call_they_are_in():
    """Rows [r0, r1) computed alone are the same rows of the full call, bit for bit: r0, r1 at and off the 128-row block
    and the 32-row tile, GELU and residual on, K = 528."""
    p = R.gemm_problem("placement", 300, 72, 528, gelu_on=1, res=True)
    a, w, bias, r = dev(p["a"]), dev(p["w"]), dev(p["bias"]), dev(p["r"])
    full = dev(p["out0"])
    gemm_call(p, a, w, bias, r, full)
    N, ldc = p["N"], p["ldc"]
    for r0, r1 in ((0, 128), (128, 300), (5, 133), (127, 129), (32, 64), (299, 300), (0, 300)):
        part = sentinel((r1 - r0) * ldc)
        gemm_call(p, a[r0 * p["lda"]:], w, bias, r[r0 * ldc:], part, M=r1 - r0)
        assert torch.equal(part[:(r1 - r0) * ldc], full[r0 * ldc:r1 * ldc]), (r0, r1)
        assert tail_untouched(part, (r1 - r0) * ldc)
    assert N == ldc


def test_gemm_batch_member_equals_the_unbatched_call():
    p = R.gemm_case("batched")
    a, w, bias, r = dev(p["a"]), dev(p["w"]), dev(p["bias"]), dev(p["r"])
    batched = dev(p["out0"])
    gemm_call(p, a, w, bias, r, batched)
    idx = torch.from_numpy(R.gemm_index(p)["out"]).to(DEV)
    one = dict(p, n_outer=1, n_inner=1)
    for z0 in range(p["n_outer"]):
        for z1 in range(p["n_inner"]):
            alone = dev(p["out0"])
            zoff = z0 * p["c_outer"] + z1 * p["c_inner"]
            gemm_call(one, a[z0 * p["a_outer"] + z1 * p["a_inner"]:], w[z1 * p["w_inner"]:], bias[z1 * p["bias_inner"]:],
                      r[zoff:], alone[zoff:])
            assert torch.equal(alone[idx[z0, z1]], batched[idx[z0, z1]]), (z0, z1)
            mask = torch.ones_like(alone, dtype=torch.bool)
            mask[idx[z0, z1].reshape(-1)] = False
            assert bool((alone[mask] == SENT).all()), (z0, z1)


# ---- pos_pad + the batched GEMM at the base width (Cg = 48) ---------------------------------------------------------
@pytest.mark.parametrize("T", R.POS_T)
def test_pos_conv_base_width(T):
    c = R.pos_case(T)
    B, D, G, K, Cg, rows = c["B"], c["D"], c["G"], c["K"], c["Cg"], c["rows"]
    x = dev_padded(c["x"])
    n_img = B * G * rows * Cg
    padded = sentinel(n_img, 64)
    _lib.call("qpg_wavlm_pos_pad_f32", DEV, x, B, T, D, G, K, padded)
    img = R.pos_image(c["x"], G, K)
    assert np.array_equal(padded[:n_img].cpu().numpy().reshape(img.shape), img) and tail_untouched(padded, n_img)
    padded[n_img:] = float("nan")                                    # behind the last group's last row
    y = sentinel(B * T * D)
    _lib.call("qpg_wavlm_gemm_f32", DEV, padded, Cg, dev(c["w"]), dev(c["bias"]), x, y, D, T, Cg, K * Cg, 1, B, G,
              G * rows * Cg, rows * Cg, Cg * K * Cg, Cg, T * D, Cg)
    assert tail_untouched(y, B * T * D)
    ops = R.pos_operands(img, c["w"], c["bias"], c["x"])
    val, bnd = R.gemm_bound(*ops[:3], 1, ops[3])
    held("pos_conv T=%d D=%d" % (T, D), y[:B * T * D].view(B, T, D), R.pos_back(val), R.pos_back(bnd))


# ---- attention ------------------------------------------------------------------------------------------------------
def run_attention(c, B=None, qkv=None, gate=None, relb=None):
    B = c["B"] if B is None else B
    T, H = c["T"], c["H"]
    qkv = dev_padded(np.concatenate([c["q"], c["k"], c["v"]], 2)) if qkv is None else qkv
    out = sentinel(B * T * H * 64)
    _lib.call("qpg_wavlm_attention_f32", DEV, qkv, dev_padded(c["gate"]) if gate is None else gate,
              dev_padded(c["relb"]) if relb is None else relb, B, T, H, out)
    assert tail_untouched(out, B * T * H * 64)
    return out[:B * T * H * 64].view(B, T, H * 64)


@pytest.mark.parametrize("T,B,H,kind", R.ATT_CASES)
def test_attention(T, B, H, kind):
    c = R.attention_case(T, B, H, kind)
    val, bnd = R.attention_bound(c["q"], c["k"], c["v"], c["gate"], c["relb"], H)
    if kind == "one hot":
        assert np.abs(c["gate"][..., None, :] * c["relb"][None, None]).max() > 100.0      # expf of a raw score overflows
    held("attention T=%d B=%d H=%d %s" % (T, B, H, kind), run_attention(c), val, bnd)


@pytest.mark.parametrize("T", [17, 65, 256])
def test_attention_does_not_depend_on_batch_or_head_position(T):
    c = R.attention_case(T, 3, 3)
    H, D = 3, 192
    full = run_attention(c)
    qkv = np.concatenate([c["q"], c["k"], c["v"]], 2)
    for b in range(3):
        alone = run_attention(c, B=1, qkv=dev_padded(qkv[b]), gate=dev_padded(c["gate"][b]))
        assert torch.equal(alone[0], full[b]), b
    perm = [2, 0, 1]
    cols = np.concatenate([np.arange(64) + 64 * h for h in perm])
    pc = dict(c, q=c["q"][:, :, cols], k=c["k"][:, :, cols], v=c["v"][:, :, cols], gate=c["gate"][:, :, perm],
              relb=c["relb"][:, perm])
    assert torch.equal(run_attention(pc), full[:, :, torch.from_numpy(cols).to(DEV)])
    assert D == full.shape[2]


# ---- gate -----------------------------------------------------------------------------------------------------------
def run_gate(h, c, M):
    H = c["H"]
    out = sentinel(M * H)
    _lib.call("qpg_wavlm_gate_f32", DEV, h, dev(c["gw"]), dev(c["gb"]), dev(c["ga"]), M, H, out)
    assert tail_untouched(out, M * H)
    return out[:M * H].view(M, H)


@pytest.mark.parametrize("M,H,kind", R.GATE_CASES)
def test_gate(M, H, kind):
    c = R.gate_case(M, H, kind)
    h = dev_padded(c["h"])
    got = run_gate(h, c, M)
    assert bool(torch.isfinite(got).all())
    val, bnd = R.gate_bound(c["h"], c["gw"], c["gb"], c["ga"], H)
    held("gate MH=%d %s" % (M * H, kind), got, val, bnd)
    for m in sorted({0, M // 2, M - 1}):                              # a row alone: the same bits
        assert torch.equal(run_gate(h[m * H * 64:], c, 1)[0], got[m]), m


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
def run_layernorm(x, c, M, gelu, y=None):
    C = c["C"]
    out = sentinel(M * C) if y is None else y
    _lib.call("qpg_wavlm_layernorm_f32", DEV, x, dev(c["g"]), dev(c["b"]), M, C, 1e-5, gelu, out)
    return out


@pytest.mark.parametrize("M,C,gelu", R.LN_CASES)
def test_layernorm(M, C, gelu):
    c = R.layernorm_case(M, C)
    x = dev_padded(c["x"])
    out = run_layernorm(x, c, M, gelu)
    assert tail_untouched(out, M * C)
    got = out[:M * C].view(M, C)
    val, bnd = R.layernorm_bound(c["x"], c["g"], c["b"], gelu)
    held("layernorm M=%d C=%d gelu=%d" % (M, C, gelu), got, val, bnd)
    if M >= 3:                                                        # the constant row: variance 0, finite, beta's image
        assert bool(torch.isfinite(got[M - 2]).all())
    inplace = x.clone()
    run_layernorm(inplace, c, M, gelu, y=inplace)
    assert torch.equal(inplace[:M * C], out[:M * C]) and bool(torch.isnan(inplace[M * C:]).all())
    for m in range(M):                                                # a row alone: the same bits
        assert torch.equal(run_layernorm(x[m * C:], c, 1, gelu)[:C], got[m]), m


# ---- conv0 ----------------------------------------------------------------------------------------------------------
def run_conv0(c, wav=None, B=None, n=None):
    B, n = c["B"] if B is None else B, c["n"] if n is None else n
    T = (n - c["k"]) // c["s"] + 1
    out = sentinel(B * T * c["C"])
    _lib.call("qpg_wavlm_conv0_f32", DEV, dev_padded(c["wav"]) if wav is None else wav, B, n, dev(c["w"]), dev(c["bias"]),
              c["C"], c["k"], c["s"], out)
    assert tail_untouched(out, B * T * c["C"])
    return out[:B * T * c["C"]].view(B, T, c["C"])


@pytest.mark.parametrize("T,C,k,s,with_bias", R.CONV0_CASES)
def test_conv0(T, C, k, s, with_bias):
    c = R.conv0_case(T, C, k, s, with_bias)
    assert _lib.load().qpg_wavlm_conv_frames(c["n"], k, s) == T
    got = run_conv0(c)
    val, bnd = R.conv0_bound(c["wav"], c["w"], c["bias"], k, s)
    held("conv0 T=%d C=%d k=%d s=%d bias=%d" % (T, C, k, s, with_bias), got, val, bnd)


@pytest.mark.parametrize("C,k,s", [(64, 10, 5), (5, 3, 2)])
def test_conv0_frames_do_not_depend_on_the_call_they_are_in(C, k, s):
    """The first T' frames of a T = 17 call are the T' call's, for T' on both sides of the 8 frames a thread owns; a
    batch row alone gives the row's bits."""
    c = R.conv0_case(17, C, k, s, 1)
    full = run_conv0(c)
    for T2 in (1, 7, 8, 9, 16):
        n2 = s * (T2 - 1) + k
        assert torch.equal(run_conv0(c, wav=dev_padded(c["wav"][:, :n2]), n=n2), full[:, :T2]), T2
    for b in range(c["B"]):
        assert torch.equal(run_conv0(c, wav=dev_padded(c["wav"][b]), B=1)[0], full[b]), b


# ---- the whole model, launch by launch ------------------------------------------------------------------------------
def _base_width_cfg():
    return synth._wavlm_cfg(2, 768, 3072, 12, 512)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


@pytest.mark.parametrize("which", ["tiny", "base width"])
def test_model_launch_by_launch(which):
    """B = 2, one second (T = 49), two blocks.  on_stage hands out every launch's output; each launch's f64 value and
    bound are computed from the DEVICE's own input of that launch (the earlier callbacks' copies), so a failure names
    the launch.  Block 1 is held exactly as block 0."""
    cfg = dict(synth.WAVLM_TINY) if which == "tiny" else _base_width_cfg()
    sd = synth.make_wavlm_state_dict(23, cfg)
    model = W.WavLM(cfg, device=DEV).load_state_dict(sd)
    B, n = 2, 16000
    wav = synth.make_wav(24, B, n)
    taps = {}
    out = model._forward(wav, lambda stage, view: taps.__setitem__(stage, None if view is None else _np(view.clone())))
    plain = model._forward(wav)
    assert torch.equal(plain, out)                                    # the callbacks change nothing
    layers = model.conv_layers
    fr = W.frames_of(n, layers)
    T, C = fr[-1], layers[0][0]
    D, F, H = cfg["encoder_embed_dim"], cfg["encoder_ffn_embed_dim"], cfg["encoder_attention_heads"]
    assert T == 49
    p = model.p
    seen = {"start"}

    def check(stage, val, bnd):
        seen.add(stage)
        held("%s %s" % (which, stage), taps[stage], val, bnd)

    # the conv stack
    L0 = p["conv"][0]
    check("conv0", *R.conv0_bound(wav, _np(L0["w"]), _np(L0["b"]), layers[0][1], layers[0][2]))
    for i, (_, k, s) in enumerate(layers):
        L = p["conv"][i]
        if i >= 1:
            prev = taps["conv%d_norm" % (i - 1)].reshape(B, -1)
            A = prev[:, (np.arange(fr[i]) * s * C)[:, None] + np.arange(k * C)[None, :]]
            assert A.shape == (B, fr[i], k * C)
            check("conv%d" % i, *R.gemm_bound(A, _np(L["w"]), _np(L["b"])))
        check("conv%d_norm" % i, *R.layernorm_bound(taps["conv%d" % i], _np(L["g"]), _np(L["beta"]), 1))
    last = "conv%d_norm" % (len(layers) - 1)
    assert np.array_equal(taps["features"], taps[last]) and taps["features"].shape == (B, T, C)
    seen.add("features")
    # layer_norm, post_extract_proj, pos_conv
    check("front_norm", *R.layernorm_bound(taps["features"], _np(p["ln_g"]), _np(p["ln_b"])))
    check("front_end", *R.gemm_bound(taps["front_norm"], _np(p["proj_w"]), _np(p["proj_b"])))
    G, K = cfg["conv_pos_groups"], cfg["conv_pos"]
    img = R.pos_image(taps["front_end"], G, K)
    assert np.array_equal(taps["pos_pad"], img)
    seen.add("pos_pad")
    ops = R.pos_operands(img, _np(p["pos_w"]), _np(p["pos_b"]), taps["front_end"])
    val, bnd = R.gemm_bound(*ops[:3], 1, ops[3])
    check("pos_conv", R.pos_back(val), R.pos_back(bnd))
    # the blocks
    relb = _np(model.position_bias_table(T))
    x = "pos_conv"
    for i, L in enumerate(p["layers"]):
        blk = "block%d." % i
        L = {k: _np(v) for k, v in L.items()}
        check(blk + "ln1", *R.layernorm_bound(taps[x], L["ln1_g"], L["ln1_b"]))
        h = taps[blk + "ln1"]
        check(blk + "gate", *(a.reshape(B, T, H) for a in R.gate_bound(h.reshape(B * T, D), L["grep_w"], L["grep_b"],
                                                                     L["grep_a"], H)))
        check(blk + "qkv", *R.gemm_bound(h, L["qkv_w"], L["qkv_b"]))
        qkv = taps[blk + "qkv"]
        check(blk + "att", *R.attention_bound(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], taps[blk + "gate"], relb, H))
        check(blk + "out_proj", *R.gemm_bound(taps[blk + "att"], L["out_w"], L["out_b"], 0, taps[x]))
        check(blk + "ln2", *R.layernorm_bound(taps[blk + "out_proj"], L["ln2_g"], L["ln2_b"]))
        check(blk + "fc1", *R.gemm_bound(taps[blk + "ln2"], L["fc1_w"], L["fc1_b"], 1))
        assert taps[blk + "fc1"].shape == (B, T, F)
        check(blk + "fc2", *R.gemm_bound(taps[blk + "fc1"], L["fc2_w"], L["fc2_b"], 0, taps[blk + "out_proj"]))
        x = blk + "fc2"
    assert np.array_equal(taps["block0"], taps["block0.fc2"])
    seen.add("block0")
    check("blocks", *R.layernorm_bound(taps[x], _np(p["fin_g"]), _np(p["fin_b"])))
    assert np.array_equal(taps["blocks"], _np(out))
    assert seen == set(taps), sorted(set(taps) ^ seen)
    assert len(taps) == 1 + 2 * len(layers) + 1 + 4 + 8 * len(p["layers"]) + 2
