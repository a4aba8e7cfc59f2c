"""NumPy statement of what the split-f16 prefilter GEMMs promise (include/qpg.h, csrc/qpg_audio_hl.hip, sorted_rows.py) and
the seeded inputs their contract tests run on.  No torch, no GPU: tests/test_prefilter_contract_cpu.py checks this module
and its inputs on the CPU, tests/test_gpu_prefilter_contract.py holds the kernels to it.

Operands: xs f32 [R][D] unit-norm rows (all-zero rows: padding), qn f32 [Q][D] unit-norm or all-zero queries.
  exponent / split   the images' number format: one power of two per image (rows) or per query, then h = fl16(x 2^e),
                     l = fl16((x 2^e - h) 2^11);
  exact              1 - <x, q> in f64: what qpg_hl_gemm_distance / _tilemin approximate within HL_GEMM_ERR / gemm32_err;
  exact_h            1 - (sum h h') 2^-(e_c + e_q) in f64: what qpg_hl_gemm_tilemin_h computes up to its f32 accumulation
                     chain and f32 epilogue (and what is within 2^-10 + 2^-22 of `exact`: Cauchy-Schwarz);
  mask_rule          bit r of a tile's mask iff value_r <= tile minimum + f32(band), compared in f32;
  mask_verdict       what a mask bit must be when the values are only known within E."""
import numpy as np

FAMILIES = ("dense", "spiky", "cancel", "neardup", "nearquery", "zeros")
ULP = 2.0 ** -22          # one f32 unit in [2, 4): covers the rounding of (minimum + band) for values <= 2 + band, twice over


def exponent(amax):
    """hl_exponent: e with amax 2^e in [2^14, 2^15); 0 for amax == 0 / inf / nan; |e| <= 100."""
    amax = np.float32(amax)
    if not (amax > 0) or amax > np.float32(3.0e38):
        return 0
    e = 15 - int(np.frexp(amax)[1])            # amax = f 2^e', f in [0.5, 1)
    return max(-100, min(100, e))


def split(x, e):
    """split_hl on x 2^e: (h, l) float16 arrays.  The scaling is an f32 multiplication by a power of two, x - h is exact in
    f32, both casts round to nearest even (NumPy's f32 -> f16 conversion does)."""
    xs = np.asarray(x, np.float32) * np.float32(2.0 ** int(e))
    h = xs.astype(np.float16)
    r = xs - h.astype(np.float32)
    l = (r * np.float32(2048.0)).astype(np.float16)
    return h, l


def row_exponent(xs):
    """The ONE exponent of a row image (qpg_hl_pack_rows: meta[0])."""
    return exponent(np.abs(np.asarray(xs, np.float32)).max(initial=0.0))


def query_exponents(qn):
    """One exponent per query (qpg_hl_pack_cols), 0 for a zero query."""
    return np.array([exponent(m) for m in np.abs(np.asarray(qn, np.float32)).max(axis=1)], np.int64)


def exact(xs, qn):
    """1 - qn @ xs.T in f64 -> [Q][R]."""
    return 1.0 - np.asarray(qn, np.float64) @ np.asarray(xs, np.float64).T


def exact_h(xs, qn):
    """1 - (sum h h') 2^-(e_c + e_q) in f64 from the emulated h planes -> [Q][R].  (11-bit significands: the products and,
    for D <= 2^20, their sums are exact in f64.)"""
    e_c, e_q = row_exponent(xs), query_exponents(qn)
    hx = split(xs, e_c)[0].astype(np.float64)
    hq = np.stack([split(q, e)[0] for q, e in zip(np.asarray(qn, np.float32), e_q)]).astype(np.float64)
    return 1.0 - (hq @ hx.T) * np.ldexp(1.0, -(e_c + e_q))[:, None]


def tile_min(D):
    """Minimum of every 16-row tile of [Q][R] -> [Q][R / 16] (same dtype)."""
    D = np.asarray(D)
    return D.reshape(D.shape[0], -1, 16).min(axis=2)


def mask_rule(D32, band):
    """The GEMMs' row masks from the f32 values they hold, [Q][R] -> u16 [Q][R / 16]: bit r iff
    D32[16 t + r] <= tile minimum + f32(band), the sum and the comparison in f32."""
    D32 = np.asarray(D32)
    assert D32.dtype == np.float32
    tiles = D32.reshape(D32.shape[0], -1, 16)
    lim = tiles.min(axis=2)[:, :, None] + np.float32(band)
    assert lim.dtype == np.float32
    bits = (tiles <= lim).astype(np.uint16)
    return (bits << np.arange(16, dtype=np.uint16)).sum(axis=2).astype(np.uint16)


def mask_bits(mask):
    """u16 [Q][T] -> bool [Q][T][16]."""
    return ((np.asarray(mask).astype(np.uint16)[:, :, None] >> np.arange(16, dtype=np.uint16)) & 1).astype(bool)


def mask_verdict(ref, band, E):
    """What a mask computed from values within E of ref [Q][R] (f64) must hold, i8 [Q][R / 16][16]: +1 must be set, -1 must
    be clear, 0 undecided.  A value is within E of its reference and so is the tile's minimum (min is 1-Lipschitz), the limit
    minimum + f32(band) is rounded once (< ULP): the bit is set whenever ref <= ref minimum + band - 2 E - ULP and clear
    whenever ref > ref minimum + band + 2 E + ULP."""
    ref = np.asarray(ref, np.float64)
    tiles = ref.reshape(ref.shape[0], -1, 16)
    m = tiles.min(axis=2)[:, :, None]
    b = float(np.float32(band))
    v = np.zeros(tiles.shape, np.int8)
    v[tiles <= m + b - 2.0 * E - ULP] = 1
    v[tiles > m + b + 2.0 * E + ULP] = -1
    return v


# ---- seeded inputs --------------------------------------------------------------------------------------------------------
def _unit(v):
    """Rows of v (f64) normalised in f64, stored as f32: norms within a few 2^-24 of 1."""
    v = np.asarray(v, np.float64)
    return (v / np.sqrt((v * v).sum(axis=-1, keepdims=True))).astype(np.float32)


def queries(Q, D, seed):
    """Gaussian unit queries f32 [Q][D]; query 3 is all zero when Q > 3."""
    rng = np.random.default_rng([seed, Q, D, 0x51])
    qn = _unit(rng.standard_normal((Q, D)))
    if Q > 3:
        qn[3] = 0.0
    return qn


def live_queries(qn):
    """Indices of the non-zero queries: the ones a row source may draw."""
    return np.nonzero(np.abs(qn).max(axis=1) > 0)[0]


def _balanced_signs(q, rng):
    """Signs s with sum s_i q_i |q_i| ~ 0: a random half of the elements gets random signs (a residual of ~1 / sqrt(D)); the
    other half, in descending order of q_i^2 (their sum, ~1/2, is far above that residual), each gets the sign that brings
    the running sum back towards zero: once it has crossed zero it stays within the current q_i^2, so it ends within the
    smallest square of that half."""
    p = np.asarray(q, np.float64)
    p = p * np.abs(p)
    n = p.shape[0]
    perm = rng.permutation(n)
    s = np.empty(n)
    s[perm[:n // 2]] = rng.choice([-1.0, 1.0], n // 2)
    run = float((s[perm[:n // 2]] * p[perm[:n // 2]]).sum())
    rest = perm[n // 2:]
    for i in rest[np.argsort(-np.abs(p[rest]), kind="stable")]:
        s[i] = -1.0 if (run > 0) == (p[i] > 0) else 1.0
        run += s[i] * p[i]
    return s


def family(name, qn, n_tiles, seed):
    """n_tiles 16-row tiles of family `name` for the queries qn -> f32 [16 n_tiles][D], unit rows (zeros: all zero).
      dense      Gaussian, normalised;
      spiky      one element ~1, the rest ~1e-3; tile 0: sixteen one-hot rows (an element of exactly 1 sets the exponent);
      cancel     tile t: sixteen rows s_i |q_i| of ONE live query q with balanced random signs - sum |products| = 1, dot
                 product ~0 (below 1e-3), the worst case of an accumulation bound, the tile's values for that query
                 inside or astride the band;
                 tile 0 starts with +q and -q of four live queries (distances 0 and 2);
      neardup    tile t: a Gaussian unit row and 15 copies perturbed by eps u (u a unit direction), eps log-uniform in
                 [1e-7, 1e-2]: the tile's values straddle the band;
      nearquery  the same around a live query, eps in [1e-4, 1e-1] (distances eps^2 / 2);
      zeros      all-zero rows."""
    qn = np.asarray(qn, np.float32)
    D = qn.shape[1]
    rng = np.random.default_rng([seed, D, qn.shape[0], FAMILIES.index(name)])
    live = live_queries(qn)
    n = 16 * n_tiles
    if name == "zeros":
        return np.zeros((n, D), np.float32)
    if name == "dense":
        return _unit(rng.standard_normal((n, D)))
    if name == "spiky":
        x = 1e-3 * rng.standard_normal((n, D))
        x[np.arange(n), rng.integers(0, D, n)] = rng.choice([-1.0, 1.0], n)
        x = _unit(x)
        x[:16] = 0.0
        x[np.arange(16), rng.choice(D, 16, replace=False)] = 1.0
        return x
    if name == "cancel":
        x = np.empty((n, D), np.float32)
        for t in range(n_tiles):
            q = qn[live[rng.integers(0, live.size)]]
            for r in range(16):
                x[16 * t + r] = (_balanced_signs(q, rng) * np.abs(q.astype(np.float64))).astype(np.float32)
        four = live[np.arange(4) % live.size]
        x[0:4] = qn[four]
        x[4:8] = -qn[four]
        return x
    if name in ("neardup", "nearquery"):
        lo, hi = (1e-7, 1e-2) if name == "neardup" else (1e-4, 1e-1)
        x = np.empty((n, D), np.float32)
        for t in range(n_tiles):
            base = (_unit(rng.standard_normal(D)) if name == "neardup" else qn[live[t % live.size]]).astype(np.float64)
            eps = np.exp(rng.uniform(np.log(lo), np.log(hi), 15))
            u = _unit(rng.standard_normal((15, D))).astype(np.float64)
            x[16 * t] = base
            x[16 * t + 1:16 * t + 16] = _unit(base[None] + eps[:, None] * u)
        return x
    raise ValueError(name)


def rows_mixed(R, qn, seed):
    """An image of R rows (R % 16 == 0): tiles of the five non-zero families in rotation, the rotation starting at `seed`,
    the last tile `zeros`.  -> xs f32 [R][D], family index per tile (into FAMILIES)."""
    nt = R // 16
    fam = np.array([(t + seed) % 5 for t in range(nt)])
    fam[-1] = FAMILIES.index("zeros")
    return _assemble(fam, qn, seed), fam


def rows_dense_with_probes(R, qn, seed):
    """The many-item image: `dense` everywhere but for one tile of every other family at the head of the first, a middle
    and the last 256-row block (the last tile of the image stays `zeros`)."""
    nt = R // 16
    fam = np.zeros(nt, np.int64)
    nrb = (R + 255) // 256
    for rb in sorted({0, nrb // 2, nrb - 1}):
        for k in range(1, 6):
            if 16 * rb + k - 1 < nt:
                fam[16 * rb + k - 1] = k
    fam[-1] = FAMILIES.index("zeros")
    return _assemble(fam, qn, seed), fam


def _assemble(fam, qn, seed):
    xs = np.empty((16 * fam.size, qn.shape[1]), np.float32)
    for k, name in enumerate(FAMILIES):
        at = np.nonzero(fam == k)[0]
        if at.size:
            xs.reshape(fam.size, 16, -1)[at] = family(name, qn, at.size, seed).reshape(at.size, 16, -1)
    return xs
