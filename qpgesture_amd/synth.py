"""Synthetic inputs with the reference's on-disk schema.

No real BEAT database or checkpoint ships with the reference, so every test,
golden vector and bench line is driven by these generators.  Everything is
drawn from numpy.random.Generator(PCG64(seed)) so that the GPU box can
regenerate byte-identical inputs from a seed instead of shipping them.
"""
import os
import numpy as np

from .constant import codebook_size, num_frames, num_frames_code


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def make_codes(n_seq, seed, force_all_present=True):
    """(n_seq, 30) int64 code ids; every code forced present on grid rows 0..25 when it fits.

    Presence has to hold on the 26 grid positions the scans visit
    (GestureKNN.py:673-675, 713-714), not merely somewhere in the row.
    """
    rng = _rng(seed)
    code = rng.integers(0, codebook_size, size=(n_seq, num_frames_code), dtype=np.int64)
    if force_all_present and n_seq * 26 >= codebook_size:
        slots = rng.permutation(n_seq * 26)[:codebook_size]
        code[slots // 26, slots % 26] = np.arange(codebook_size)
    return code


def make_db(n_seq, seed, wavlm_dim=1024, with_body=False):
    """Dict of arrays for one split (train or test) of a speaker database."""
    rng = _rng(seed)
    d = {}
    d["mfcc"] = rng.standard_normal((n_seq, num_frames, 14)).astype(np.float32)
    d["energy"] = rng.random((n_seq, num_frames)).astype(np.float32)
    d["pitch"] = rng.random((n_seq, num_frames)).astype(np.float32)
    d["volume"] = rng.random((n_seq, num_frames)).astype(np.float32)
    d["context"] = rng.standard_normal((n_seq, num_frames_code, 1, 384)).astype(np.float32)
    # dense phase: (n, 240, 4, 8); index 0 = phase shift p, 2 = amplitude a (PAE.py:505-508)
    d["phase_dense"] = rng.standard_normal((n_seq, num_frames, 4, 8)).astype(np.float32)
    d["wavlm"] = rng.standard_normal((n_seq, 199, wavlm_dim)).astype(np.float32)
    d["wavvq"] = rng.integers(0, 320, size=(n_seq, 398, 2), dtype=np.int64)
    if with_body:
        d["body"] = rng.standard_normal((n_seq, num_frames, 135)).astype(np.float32)
    return d


def make_signature(seed):
    return _rng(seed).standard_normal((codebook_size, 135)).astype(np.float32)


def phase_dense_to_object(phase_dense):
    """(n,240,4,8) f32 -> object array (n,240,4) of torch tensors shaped (1,8,1).

    That is the layout PAE.py:505-508 / fix_device_bug.py:14-22 leave in the
    reference's *_txt_2.npz files.
    """
    import torch
    n, t, c, _ = phase_dense.shape
    out = np.empty((n, t, c), dtype=object)
    for i in range(n):
        for j in range(t):
            for k in range(c):
                out[i, j, k] = torch.from_numpy(phase_dense[i, j, k].copy()).reshape(1, 8, 1)
    return out


def apply_variant(tr, te, code, variant):
    """Planted structure on top of the seeded arrays (in place), shared by the golden generator and the tests.

    'neartie': audio near-ties below the rounding noise of any distance formula (SURVEY.md §7 hard part 2).  The two
        test windows are DB windows 5 and 9, so every query has a candidate at distance exactly 0; DB windows 20 / 30
        are copies of 5 / 9 with a few elements moved by one float32 ulp and the SAME code row (two candidates of one
        code within ~1e-19 of each other), 21 / 31 the same with their own code rows (minima of two different codes
        within ~1e-19), 22 an exact duplicate of 5 with the same codes (exact tie: first index wins).
    'texttie': repeated context rows, as real BEAT data has (every silent code frame carries the identical
        encode(['']) embedding, make_beat_dataset.py:556-565): many codes tie EXACTLY in txt_dist, often at distance 0,
        and the reference ranks them with NumPy's unstable argsort.
    'nearsilent': a near-silent stretch, as a speaker DB has between utterances: DB windows 8..37 and test window 0
        carry ONE quiet feature vector (amplitude 1e-3) in every frame, the copies differing by about one float32 ulp
        per element (8..12 are bit-identical), 22 of the 30 windows sharing six codes.  All 30 x 26 = 780 candidates of
        that stretch then sit within ~1e-14 of each other for a quiet query (about 130 per crowded code) - more than
        any fixed-size near-tie list holds - and the reference's strict `<` scan (GestureKNN.py:685-689) still has an
        answer for every one of them in its own arithmetic.
    'speechlike': feature statistics closer to real WavLM tracks than i.i.d. N(0,1): AR(1) in time (rho = 0.95) on
        rank-64 mixtures over the 1024 features plus a small full-rank residual, 10 % near-silent frames (amplitude
        1e-3 around a common quiet vector), and context rows that repeat over a few code frames (words spanning
        frames) with 20 % silence embeddings."""
    if variant is None:
        return
    if variant == "neartie":
        w = tr["wavlm"]
        te["wavlm"][0], te["wavlm"][1] = w[5], w[9]

        def ulp(src, stride):
            x = src.copy()
            flat = x.reshape(x.shape[0], -1)
            flat[:, ::stride] = np.nextafter(flat[:, ::stride], np.float32(np.inf))
            return x
        w[20], w[21] = ulp(w[5], 97), ulp(w[5], 89)
        w[30], w[31] = ulp(w[9], 97), ulp(w[9], 89)
        w[22] = w[5]
        code[20], code[30], code[22] = code[5], code[9], code[5]
    elif variant == "texttie":
        rng = _rng(777)
        sil = rng.standard_normal((384,)).astype(np.float32)           # the "silence" embedding
        ctx = tr["context"]
        mask = rng.random(ctx.shape[:2]) < 0.35
        ctx[mask] = sil
        for j in range(0, ctx.shape[0], 3):                            # words spanning several code frames
            ctx[j, 10:14] = ctx[j, 10]
        tq = te["context"]
        tq[:, ::4] = sil                                               # silent query frames: distance exactly 0
    elif variant == "nearsilent":
        rng = _rng(778)
        F = tr["wavlm"].shape[2]
        quiet = (rng.standard_normal((F,)) * 1e-3).astype(np.float32)

        def stretch(n):
            x = np.broadcast_to(quiet, (n, 199, F)).astype(np.float32)
            flip = rng.integers(-1, 2, size=x.shape)                    # -1 / 0 / +1 ulp per element
            up = np.nextafter(x, np.float32(np.inf))
            dn = np.nextafter(x, np.float32(-np.inf))
            return np.where(flip > 0, up, np.where(flip < 0, dn, x)).astype(np.float32)
        w = tr["wavlm"]
        w[8:38] = stretch(30)
        w[8:13] = quiet                                                 # bit-identical windows: exact ties, first wins
        code[8:30] = 100 + rng.integers(0, 6, size=(22, code.shape[1]))  # six crowded codes; 30..37 keep their own
        te["wavlm"][0] = stretch(1)[0]
    elif variant == "speechlike":
        speechlike_transform(tr, 779)
        speechlike_transform(te, 780)
    else:
        raise ValueError(variant)


def speechlike_transform(d, seed):
    """In place: give one split of a synthetic database (make_db) feature statistics closer to real WavLM / sentence-
    embedding tracks (see apply_variant 'speechlike').  `seed` drives the temporal processes; the mixing matrix, the
    quiet vector and the silence embedding are common to all splits and chunks (one speaker, one room)."""
    rng = _rng(seed)
    n, T, F = d["wavlm"].shape
    mix = (_rng(783).standard_normal((64, F)) / 8.0).astype(np.float32) if seed not in (779, 780) else \
        (rng.standard_normal((64, F)) / 8.0).astype(np.float32)
    z = np.empty((n, T, 64), np.float32)
    z[:, 0] = rng.standard_normal((n, 64))
    innov = (rng.standard_normal((n, T, 64)) * np.sqrt(1 - 0.95 ** 2)).astype(np.float32)
    for t in range(1, T):
        z[:, t] = 0.95 * z[:, t - 1] + innov[:, t]
    x = z @ mix + 0.05 * d["wavlm"]                              # low-rank, slowly varying + a little of the rest
    quiet = (_rng(781).standard_normal((F,)) * 1e-3).astype(np.float32)
    sil = rng.random((n, T)) < 0.10
    x[sil] = quiet * (1.0 + 1e-3 * rng.standard_normal((int(sil.sum()), F)).astype(np.float32))
    d["wavlm"][...] = x.astype(np.float32)
    ctx = d["context"]
    silence = _rng(782).standard_normal((384,)).astype(np.float32)
    for j in range(n):
        r = 0
        while r < ctx.shape[1]:
            span = int(rng.integers(1, 5))
            ctx[j, r:r + span] = silence if rng.random() < 0.2 else ctx[j, r]
            r += span


def write_npz_set(outdir, n_train, n_test, seed_train=0, seed_test=1, seed_code=2, seed_sig=3,
                  wavlm_dim=1024, variant=None):
    """Write the 8 npz files GestureKNN.py's CLI takes; returns the path dict (flag -> path)."""
    os.makedirs(outdir, exist_ok=True)
    tr = make_db(n_train, seed_train, wavlm_dim)
    te = make_db(n_test, seed_test, wavlm_dim)
    code = make_codes(n_train, seed_code)
    sig = make_signature(seed_sig)
    apply_variant(tr, te, code, variant)
    p = {k: os.path.join(outdir, v) for k, v in dict(
        train_database="train_240_txt_2.npz", test_data="test_240_txt_2.npz",
        train_codebook="train_240_code.npz", codebook_signature="code.npz",
        train_wavlm="train_240_WavLM.npz", test_wavlm="test_240_WavLM.npz",
        train_wavvq="train_240_WavVQ.npz", test_wavvq="test_wavvq_240.npz").items()}
    for d, path in ((tr, p["train_database"]), (te, p["test_data"])):
        np.savez(path, mfcc=d["mfcc"], energy=d["energy"], pitch=d["pitch"], volume=d["volume"],
                 context=d["context"], phase=phase_dense_to_object(d["phase_dense"]))
    np.savez(p["train_codebook"], code=code)
    np.savez(p["codebook_signature"], signature=sig)
    np.savez(p["train_wavlm"], wavlm=tr["wavlm"])
    np.savez(p["test_wavlm"], wavlm=te["wavlm"])
    np.savez(p["train_wavvq"], wavvq=tr["wavvq"])
    np.savez(p["test_wavvq"], wavvq=te["wavvq"])
    return p


def write_npz_set_dense(outdir, n_train, n_test, chunked_db=None, seed_code=2, seed_sig=3):
    """The 8 npz files of the CLI at bench size (n_train in the thousands), generated in 64-window chunks, with the phase
    track written as a DENSE f32 (n,240,4,8) array (data_processing.densify_phase accepts it; the reference's object
    array of pickled torch tensors takes ~0.2 s per DB window to write and to read back).  Returns the path dict."""
    os.makedirs(outdir, exist_ok=True)

    def chunks(n, seed0):
        parts = [make_db(min(64, n - c0), seed0 * 100003 + c0 // 64) for c0 in range(0, n, 64)]
        return {k: np.concatenate([p_[k] for p_ in parts]) for k in parts[0]}
    tr, te = chunks(n_train, 0), chunks(n_test, 1)
    p = {k: os.path.join(outdir, v) for k, v in dict(
        train_database="train_240_txt_2.npz", test_data="test_240_txt_2.npz",
        train_codebook="train_240_code.npz", codebook_signature="code.npz",
        train_wavlm="train_240_WavLM.npz", test_wavlm="test_240_WavLM.npz",
        train_wavvq="train_240_WavVQ.npz", test_wavvq="test_wavvq_240.npz").items()}
    for d, path in ((tr, p["train_database"]), (te, p["test_data"])):
        np.savez(path, mfcc=d["mfcc"], energy=d["energy"], pitch=d["pitch"], volume=d["volume"],
                 context=d["context"], phase=np.ascontiguousarray(d["phase_dense"], np.float32))
    np.savez(p["train_codebook"], code=make_codes(n_train, seed_code))
    np.savez(p["codebook_signature"], signature=make_signature(seed_sig))
    np.savez(p["train_wavlm"], wavlm=tr["wavlm"])
    np.savez(p["test_wavlm"], wavlm=te["wavlm"])
    np.savez(p["train_wavvq"], wavvq=tr["wavvq"])
    np.savez(p["test_wavvq"], wavvq=te["wavvq"])
    return p


# ----------------------------------------------------------------------------------------------
# gesture VQ-VAE: seeded weights with the reference's checkpoint key names
# ----------------------------------------------------------------------------------------------
VQVAE_HPS = dict(input_dim=135, width=512, emb_width=512, l_bins=512, down_t=3, stride_t=2, depth=3,
                 dilation_growth_rate=3, reverse_decoder_dilation=True)


def make_vqvae_state_dict(seed, hps=None, prefix="module."):
    """No pretrained checkpoint ships with the reference (pretrained_model/ is an empty placeholder),
    so parity runs use seeded weights with the checkpoint's exact key names and shapes
    (train.py:114-116 saves a DataParallel state_dict: keys carry `module.`)."""
    h = dict(VQVAE_HPS, **(hps or {}))
    rng = _rng(seed)
    W, E, Cin, K = h["width"], h["emb_width"], h["input_dim"], h["l_bins"]
    sd = {}

    def conv(name, cout, cin, k, gain=1.0):
        sd[prefix + name + ".weight"] = (rng.standard_normal((cout, cin, k)) * gain / np.sqrt(cin * k)).astype(np.float32)
        sd[prefix + name + ".bias"] = (rng.standard_normal((cout,)) * 0.05).astype(np.float32)

    def resnet(name):
        for d in range(h["depth"]):
            conv("%s.model.%d.model.1" % (name, d), W, W, 3, 1.4)
            conv("%s.model.%d.model.3" % (name, d), W, W, 1, 0.5)

    enc = "encoders.0.level_blocks.0.model"
    for i in range(h["down_t"]):
        conv("%s.%d.0" % (enc, i), W, Cin if i == 0 else W, 2 * h["stride_t"])
        resnet("%s.%d.1" % (enc, i))
    conv("%s.%d" % (enc, h["down_t"]), E, W, 3)
    dec = "decoders.0.level_blocks.0.model"
    conv(dec + ".0", W, E, 3)
    for i in range(h["down_t"]):
        resnet("%s.%d.0" % (dec, i + 1))
        # ConvTranspose1d weight is (C_in, C_out, k)
        sd[prefix + "%s.%d.1.weight" % (dec, i + 1)] = (rng.standard_normal((W, W, 2 * h["stride_t"]))
                                                        / np.sqrt(W * 2)).astype(np.float32)
        sd[prefix + "%s.%d.1.bias" % (dec, i + 1)] = (rng.standard_normal((W,)) * 0.05).astype(np.float32)
    conv("decoders.0.out", Cin, E, 3)
    sd[prefix + "bottleneck.level_blocks.0.k"] = rng.standard_normal((K, E)).astype(np.float32)
    return sd


# ----------------------------------------------------------------------------------------------
# Periodic Auto-Encoder (DeepPhase, codebook/PAE.py): seeded weights with the reference's key names
# ----------------------------------------------------------------------------------------------
PAE_HPS = dict(input_channels=135, embedding_channels=8, time_range=240, key_range=13, window=4.0)


def make_pae_state_dict(seed, prefix=""):
    """No PAE checkpoint ships with the reference either.  Seeded PAE.Model(135, 8, 240, 13, 4.0) weights with the
    reference's key names and shapes (the reference saves the bare model's state_dict: no `module.`).  The batch-norm
    layers get non-trivial running statistics and affine parameters, scaled so that on smooth unit-amplitude
    normalised motion (make_pae_motion) both tanh layers work mostly in their non-saturated range."""
    rng = _rng(seed)
    C, E, T = PAE_HPS["input_channels"], PAE_HPS["embedding_channels"], PAE_HPS["time_range"]
    M = C // 9
    ts = PAE_HPS["key_range"] / T
    sd = {}

    def f32(a):
        return np.ascontiguousarray(a, np.float32)

    def conv(name, cout, cin, gain):
        sd[prefix + name + ".weight"] = f32(rng.standard_normal((cout, cin, T)) * gain / np.sqrt(cin * T))
        sd[prefix + name + ".bias"] = f32(rng.standard_normal(cout) * 0.05)

    def bn(name, n, mean_scale, var_scale):
        sd[prefix + name + ".weight"] = f32(rng.uniform(0.6, 1.4, n) * rng.choice([-1.0, 1.0], n))
        sd[prefix + name + ".bias"] = f32(rng.standard_normal(n) * 0.1)
        sd[prefix + name + ".running_mean"] = f32(rng.standard_normal(n) * mean_scale)
        sd[prefix + name + ".running_var"] = f32(rng.uniform(0.5, 2.0, n) * var_scale)
        sd[prefix + name + ".num_batches_tracked"] = np.array(1000, np.int64)

    sd[prefix + "tpi"] = np.array([2.0 * np.pi], np.float32)
    sd[prefix + "args"] = np.linspace(-PAE_HPS["window"] / 2, PAE_HPS["window"] / 2, T, dtype=np.float32)
    sd[prefix + "freqs"] = f32(np.fft.rfftfreq(T)[1:] * (T * ts) / PAE_HPS["window"])
    conv("conv1", M, C, 6.0)
    bn("bn_conv1", M, 0.05, 0.6)
    conv("conv2", E, M, 2.0)
    bn("bn_conv2", E, 0.05, 0.5)
    for i in range(E):
        sd[prefix + "fc.%d.weight" % i] = f32(rng.standard_normal((2, T)) / np.sqrt(T) * 3.0)
        sd[prefix + "fc.%d.bias" % i] = f32(rng.standard_normal(2) * 0.05)
        bn("bn.%d" % i, 2, 0.05, 0.5)
    conv("deconv1", M, E, 1.0)
    bn("bn_deconv1", M, 0.05, 1.0)
    conv("deconv2", C, M, 1.0)
    return sd


def make_pae_motion(T, seed, still=None):
    """(T, 135) f64 smooth synthetic `upper` rotation channels: mean + std * (unit-amplitude sum of sinusoids with
    0.5-4 s periods at 60 fps), so that the normalised motion is O(1) and its velocities O(0.05).  `still` = (a, b):
    frames a..b-1 hold frame a's pose (a stretch of zero velocity)."""
    from .checkpoint import load_config
    cfg = load_config(os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs", "codebook.yml"))
    mean, std = np.asarray(cfg.data_mean, np.float64), np.clip(np.asarray(cfg.data_std, np.float64), 0.01, None)
    rng = _rng(seed)
    t = np.arange(T, dtype=np.float64)[:, None]
    sig = np.zeros((T, mean.shape[0]))
    for _ in range(3):
        period = rng.uniform(30.0, 240.0, mean.shape[0])
        sig += rng.uniform(0.2, 0.6, mean.shape[0]) * np.sin(2 * np.pi * t / period + rng.uniform(0, 2 * np.pi, mean.shape[0]))
    if still is not None:
        a, b = still
        sig[a:b] = sig[a]
    return mean + std * sig


# ----------------------------------------------------------------------------------------------
# WavLM (process/WavLM/WavLM.py): seeded weights with the reference's key names, and seeded audio
# ----------------------------------------------------------------------------------------------
def _wavlm_cfg(layers, dim, ffn, heads, conv):
    return dict(extractor_mode="layer_norm", encoder_layers=layers, encoder_embed_dim=dim, encoder_ffn_embed_dim=ffn,
                encoder_attention_heads=heads, activation_fn="gelu", layer_norm_first=True,
                conv_feature_layers="[(%d,10,5)] + [(%d,3,2)] * 4 + [(%d,2,2)] * 2" % (conv, conv, conv), conv_bias=False,
                normalize=True, conv_pos=128, conv_pos_groups=16, relative_position_embedding=True, num_buckets=320,
                max_distance=800, gru_rel_pos=True)


WAVLM_TINY = dict(_wavlm_cfg(2, 128, 256, 2, 64), conv_bias=True)      # every kernel path at the smallest widths
WAVLM_WIDE = _wavlm_cfg(2, 1024, 4096, 16, 512)        # WavLM-Large's tile shapes, two blocks
WAVLM_LARGE = _wavlm_cfg(24, 1024, 4096, 16, 512)      # WavLM-Large.pt's cfg


def make_wavlm_state_dict(seed, cfg=None):
    """No WavLM checkpoint ships with the reference.  Seeded weights with the key names and shapes of the reference's
    WavLM(cfg).state_dict() (`cfg` a dict in the checkpoint's form, default WAVLM_TINY).  Biases, LayerNorm weights, the
    weight-norm gains and grep_a are non-trivial; the scales keep activations O(1) through every block."""
    from .wavlm import conv_layers_of
    cfg = dict(WAVLM_TINY if cfg is None else cfg)
    rng = _rng(seed)
    D, F, H = cfg["encoder_embed_dim"], cfg["encoder_ffn_embed_dim"], cfg["encoder_attention_heads"]
    sd = {}

    def f32(a):
        return np.ascontiguousarray(a, np.float32)

    def vec(name, n, scale=0.1):
        sd[name] = f32(rng.standard_normal(n) * scale)

    def norm(name, n):
        sd[name + ".weight"] = f32(rng.uniform(0.6, 1.4, n))
        vec(name + ".bias", n)

    def linear(name, nout, nin, gain=1.0):
        sd[name + ".weight"] = f32(rng.standard_normal((nout, nin)) * gain / np.sqrt(nin))
        vec(name + ".bias", nout)

    sd["mask_emb"] = f32(rng.uniform(0.0, 1.0, D))
    cin = 1
    for i, (c, k, s) in enumerate(conv_layers_of(cfg)):
        sd["feature_extractor.conv_layers.%d.0.weight" % i] = f32(rng.standard_normal((c, cin, k)) * 1.4 / np.sqrt(cin * k))
        if cfg.get("conv_bias", False):
            vec("feature_extractor.conv_layers.%d.0.bias" % i, c)
        norm("feature_extractor.conv_layers.%d.2.1" % i, c)
        cin = c
    if cin != D:
        linear("post_extract_proj", D, cin)
    K, G = cfg.get("conv_pos", 128), cfg.get("conv_pos_groups", 16)
    vec("encoder.pos_conv.0.bias", D)
    sd["encoder.pos_conv.0.weight_g"] = f32(rng.uniform(0.5, 1.5, (1, 1, K)))
    sd["encoder.pos_conv.0.weight_v"] = f32(rng.standard_normal((D, D // G, K)) * 0.05)
    for i in range(cfg["encoder_layers"]):
        p = "encoder.layers.%d." % i
        sd[p + "self_attn.grep_a"] = f32(rng.uniform(0.5, 1.5, (1, H, 1, 1)))
        if i == 0:
            sd[p + "self_attn.relative_attention_bias.weight"] = f32(rng.standard_normal((cfg["num_buckets"], H)))
        for n in ("k_proj", "v_proj", "q_proj"):
            linear(p + "self_attn." + n, D, D, 1.5)
        linear(p + "self_attn.out_proj", D, D)
        linear(p + "self_attn.grep_linear", 8, D // H)
        norm(p + "self_attn_layer_norm", D)
        linear(p + "fc1", F, D)
        linear(p + "fc2", D, F)
        norm(p + "final_layer_norm", D)
    norm("encoder.layer_norm", D)
    norm("layer_norm", cin)
    return sd


def make_wav(seed, B, n):
    """(B, n) f32 seeded audio at 16 kHz: a few harmonics under a slow envelope plus noise, peak around 0.3 - not
    normalised, like the samples the reference feeds the model."""
    rng = _rng(seed)
    t = np.arange(n, dtype=np.float64)[None, :] / 16000.0
    wav = np.zeros((B, n))
    for _ in range(4):
        f = rng.uniform(90.0, 1800.0, (B, 1))
        wav += rng.uniform(0.02, 0.1, (B, 1)) * np.sin(2 * np.pi * (f * t + rng.uniform(0, 1, (B, 1))))
    wav *= 0.6 + 0.4 * np.sin(2 * np.pi * (rng.uniform(1.0, 4.0, (B, 1)) * t + rng.uniform(0, 1, (B, 1))))
    wav += rng.standard_normal((B, n)) * 0.02
    return np.ascontiguousarray(wav, np.float32)


# ----------------------------------------------------------------------------------------------
# Sentence encoder (transformers' BertModel as sentence-transformers wraps it): seeded weights with BertModel's key
# names, and a small word list in vocab.txt's form
# ----------------------------------------------------------------------------------------------
def _bert_cfg(hidden, layers, heads, ffn, vocab):
    return dict(model_type="bert", hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
                intermediate_size=ffn, vocab_size=vocab, max_position_embeddings=512, type_vocab_size=2,
                hidden_act="gelu", layer_norm_eps=1e-12, position_embedding_type="absolute", pad_token_id=0)


BERT_TINY = _bert_cfg(64, 2, 2, 128, 97)             # every kernel path at the smallest widths
BERT_MINILM = _bert_cfg(384, 6, 12, 1536, 30522)     # paraphrase-MiniLM-L6-v2's config.json


def make_bert_state_dict(seed, cfg=None):
    """No MiniLM checkpoint ships with the reference.  Seeded weights with the key names and shapes of
    transformers.BertModel(config, add_pooling_layer=False).state_dict() (`cfg` a config.json dict, default BERT_TINY).
    Linear weights N(0, 1 / fan_in) with the query and key weights times 2 (gain 1 gives near-uniform softmax rows, which
    would test nothing; 3 makes the f32 evaluation itself chaotic), embeddings N(0, 0.5^2), biases and LayerNorm gains
    non-trivial."""
    cfg = dict(BERT_TINY if cfg is None else cfg)
    rng = _rng(seed)
    D, F = cfg["hidden_size"], cfg["intermediate_size"]
    sd = {}

    def f32(a):
        return np.ascontiguousarray(a, np.float32)

    def norm(name, n):
        sd[name + ".weight"] = f32(rng.uniform(0.6, 1.4, n))
        sd[name + ".bias"] = f32(rng.standard_normal(n) * 0.1)

    def linear(name, nout, nin, gain=1.0):
        sd[name + ".weight"] = f32(rng.standard_normal((nout, nin)) * gain / np.sqrt(nin))
        sd[name + ".bias"] = f32(rng.standard_normal(nout) * 0.1)

    sd["embeddings.word_embeddings.weight"] = f32(rng.standard_normal((cfg["vocab_size"], D)) * 0.5)
    sd["embeddings.position_embeddings.weight"] = f32(rng.standard_normal((cfg["max_position_embeddings"], D)) * 0.5)
    sd["embeddings.token_type_embeddings.weight"] = f32(rng.standard_normal((cfg.get("type_vocab_size", 2), D)) * 0.5)
    norm("embeddings.LayerNorm", D)
    for i in range(cfg["num_hidden_layers"]):
        p = "encoder.layer.%d." % i
        linear(p + "attention.self.query", D, D, 2.0)
        linear(p + "attention.self.key", D, D, 2.0)
        linear(p + "attention.self.value", D, D)
        linear(p + "attention.output.dense", D, D)
        norm(p + "attention.output.LayerNorm", D)
        linear(p + "intermediate.dense", F, D)
        linear(p + "output.dense", D, F)
        norm(p + "output.LayerNorm", D)
    return sd


def make_vocab():
    """A 97-entry vocab.txt word list (BERT_TINY's vocab_size): the five specials, punctuation, single letters and
    digits as whole words and as ## pieces, a few words and pieces, one accented-stripped word and one CJK character."""
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ".", ",", "!", "?", "'", "-", "(", ")"]
    words += list("abcdefghijklmnopqrstuvwxyz")
    words += ["##" + c for c in "abcdefghijklmnopqrstuvwxyz"]
    words += ["the", "and", "you", "so", "is", "it", "to", "of", "hello", "world", "gesture", "speak", "hand", "we",
              "un", "##ing", "##ed", "##er", "##ly", "##able", "cafe", "naive", "Hello", "The", "I",
              "中", "文", "0", "1", "2", "##0", "##1"]
    assert len(words) == 97 and len(set(words)) == 97
    return words


# ----------------------------------------------------------------------------------------------
# The GRU speech-to-code generator (codebook/generate/generate.py Generator_gru): seeded weights with the reference's
# key names
# ----------------------------------------------------------------------------------------------
GENERATOR_CONVS = [(1, 8, 3), (8, 16, 3), (16, 32, 6), (32, 64, 6), (64, 32, 6)]      # (Cin, Cout, stride), 16 taps each
GENERATOR_HIDDEN, GENERATOR_CODES = 200, 512


def make_generator_state_dict(seed, prefix="module."):
    """No end2end checkpoint ships with the reference.  Seeded Generator_gru() weights with the reference's key names and
    shapes (end2end.py saves a DataParallel state_dict: keys carry `module.`).  Every tensor is drawn uniform within
    torch's default bound 1 / sqrt(fan_in) times a gain: convolutions x 2, GRU x 3, out.weight x 4 - at torch's own
    scales a 4 s window yields one or two distinct codes and the recurrence barely matters - and the BatchNorm running
    statistics and affines are drawn away from (0, 1)."""
    rng = _rng(seed)
    H, C = GENERATOR_HIDDEN, GENERATOR_CODES
    sd = {}

    def f32(a):
        return np.ascontiguousarray(a, np.float32)

    def uniform(name, shape, fan_in, gain=1.0):
        b = gain / np.sqrt(fan_in)
        sd[prefix + name] = f32(rng.uniform(-b, b, shape))

    enc = "WavEncoder.feat_extractor."
    for i, (cin, cout, _) in enumerate(GENERATOR_CONVS):
        uniform(enc + "%d.weight" % (3 * i), (cout, cin, 16), cin * 16, 2.0)
        uniform(enc + "%d.bias" % (3 * i), (cout,), cin * 16)
        if i < 4:
            bn = enc + "%d." % (3 * i + 1)
            sd[prefix + bn + "weight"] = f32(rng.uniform(0.6, 1.4, cout) * rng.choice([-1.0, 1.0], cout))
            sd[prefix + bn + "bias"] = f32(rng.standard_normal(cout) * 0.1)
            sd[prefix + bn + "running_mean"] = f32(rng.standard_normal(cout) * 0.05)
            sd[prefix + bn + "running_var"] = f32(rng.uniform(0.05, 0.2, cout))
            sd[prefix + bn + "num_batches_tracked"] = np.array(1000, np.int64)
    for layer, nin in ((0, 32), (1, 2 * H)):
        for suffix in ("", "_reverse"):
            tag = "_l%d%s" % (layer, suffix)
            uniform("project.weight_ih" + tag, (3 * H, nin), H, 3.0)
            uniform("project.weight_hh" + tag, (3 * H, H), H, 3.0)
            uniform("project.bias_ih" + tag, (3 * H,), H, 3.0)
            uniform("project.bias_hh" + tag, (3 * H,), H, 3.0)
    sd[prefix + "norm.weight"] = f32(rng.uniform(0.6, 1.4, H))
    sd[prefix + "norm.bias"] = f32(rng.standard_normal(H) * 0.1)
    uniform("out.weight", (C, H), H, 4.0)
    uniform("out.bias", (C,), H)
    return sd


# ----------------------------------------------------------------------------------------------
# vq-wav2vec (fairseq's Wav2VecModel with a GumbelVectorQuantizer): seeded weights with the checkpoint's key names
# ----------------------------------------------------------------------------------------------
WAVVQ_LAYERS = [(10, 5), (8, 4), (4, 2), (4, 2), (4, 2), (1, 1), (1, 1), (1, 1)]      # (kernel, stride) of vq-wav2vec.pt


def _wavvq_geom(width, hidden, groups, variables):
    return dict(conv_feature_layers=str([(width, k, s) for k, s in WAVVQ_LAYERS]), activation="relu",
                skip_connections_feat=False, log_compression=True, non_affine_group_norm=False, vq_type="gumbel",
                vq_groups=groups, vq_vars=variables, vq_depth=2, vq_hidden=hidden)


WAVVQ_TINY = _wavvq_geom(16, 32, 2, 20)          # the real kernel / stride list at the narrowest width the GEMM takes
WAVVQ_GUMBEL = _wavvq_geom(512, 1024, 2, 320)    # vq-wav2vec.pt (Gumbel): 64 000 samples -> 398 frames x 2 codes


def make_wavvq_state_dict(seed, geom=None):
    """No vq-wav2vec checkpoint ships with the reference.  Seeded weights with the key names and shapes of fairseq's
    Wav2VecModel.state_dict() for `geom` (a dict of the checkpoint's args, default WAVVQ_TINY; `vq_hidden` - not a fairseq
    arg, the loader reads the width off the weights - is the quantiser's hidden width, 2 C in the real model).  The
    GroupNorm weights are drawn away from 1 (some negative) and its biases away from 0; the second Linear's gain spreads
    the logits so that the top-2 margins stand clear of f32 rounding.  The keys the extraction ignores
    (vector_quantizer.vars, feature_aggregator.*, wav2vec_predictions.*) are present, one of each."""
    from .wavlm import conv_layers_of
    geom = dict(WAVVQ_TINY if geom is None else geom)
    rng = _rng(seed)
    sd = {}

    def f32(a):
        return np.ascontiguousarray(a, np.float32)

    cin = 1
    for i, (c, k, s) in enumerate(conv_layers_of(geom)):
        pre = "feature_extractor.conv_layers.%d." % i
        sd[pre + "0.weight"] = f32(rng.standard_normal((c, cin, k)) * 1.4 / np.sqrt(cin * k))
        if not geom.get("non_affine_group_norm", False):
            sd[pre + "2.weight"] = f32(rng.uniform(0.6, 1.4, c) * rng.choice([-1.0, 1.0], c, p=[0.25, 0.75]))
            sd[pre + "2.bias"] = f32(rng.standard_normal(c) * 0.1 + 0.2)
        cin = c
    G, V, H = geom["vq_groups"], geom["vq_vars"], geom.get("vq_hidden", 2 * cin)
    wp = "vector_quantizer.weight_proj."
    if geom.get("vq_depth", 1) == 1:
        sd[wp + "weight"] = f32(rng.standard_normal((G * V, cin)) * 3.0 / np.sqrt(cin))
        sd[wp + "bias"] = f32(rng.standard_normal(G * V) * 0.1)
    else:
        sd[wp + "0.0.weight"] = f32(rng.standard_normal((H, cin)) * 1.4 / np.sqrt(cin))
        sd[wp + "0.0.bias"] = f32(rng.standard_normal(H) * 0.1)
        sd[wp + "1.weight"] = f32(rng.standard_normal((G * V, H)) * 3.0 / np.sqrt(H))
        sd[wp + "1.bias"] = f32(rng.standard_normal(G * V) * 0.1)
    sd["vector_quantizer.vars"] = f32(rng.standard_normal((1, G * V, 4)))
    sd["feature_aggregator.conv_layers.0.0.weight"] = f32(rng.standard_normal((4, 4, 2)))
    sd["wav2vec_predictions.project_to_steps.bias"] = f32(rng.standard_normal(4))
    return sd
