"""The audio sweep as a statement in NumPy f64 (no torch, no GPU) and the seeded inputs its kernels are held to
(tests/test_audio_contract_cpu.py checks this module; tests/test_gpu_audio_contract.py holds every audio entry point of
csrc/qpg_audio.hip and csrc/qpg_audio_hl.hip to it).

The operation (data_processing.py:264-268, GestureKNN.py:666-691): candidate (j, g) of a track base [N][T][F] is the
n_taps frames cand_t[g] + i * tap_stride of window j laid end to end, a frame at or past T being ZEROS; its distance to a
query row q is 1 - <q, c> / (|q| |c|), with sklearn's rule for a row whose norm is below 10 eps (it is left unscaled) as
cosine_from_dot of csrc/qpg_common.h states it.

The input families (`family`) are what a sweep can get wrong without Gaussian data noticing: exact dot products (`grid`),
roundings that all point the same way (`samesign`), cancellation, dynamic range, near-duplicates, degenerate rows, and the
operands the kernels' validity guards exist for (`tiny`, `quiet`).  What the guards must flag is decided here, from the
inputs alone (`mx_guard`, `hl_guard`), and each family names the rows it planted for them."""
import collections

import numpy as np

N_TAPS = 6
TINY_NORM = 10.0 * np.finfo(np.float64).eps      # sklearn _handle_zeros_in_scale, f64
MX_GUARD_P = 1e-32                               # qpg_audio_cosine_mx: 0 < |q|^2 |c|^2 < this raises stats[1] |= 2
HL_NORM2_MIN = 65536.0                           # qpg_audio_cosine_hl: a scaled squared norm below this raises it
U32, U64 = 2.0 ** -24, 2.0 ** -53


# ---- the operation ---------------------------------------------------------------------------------------------------
def stack(base, cand_t, n_taps=N_TAPS, tap_stride=2):
    """The candidate rows in f64: [N * G][n_taps * F], row j * G + g; a tap whose frame is >= T is zero."""
    base = np.asarray(base)
    N, T, F = base.shape
    G = len(cand_t)
    out = np.zeros((N, G, n_taps, F), np.float64)
    for g, t0 in enumerate(cand_t):
        for i in range(n_taps):
            t = int(t0) + i * tap_stride
            if t < T:
                out[:, g, i] = base[:, t]
    return out.reshape(N * G, n_taps * F)


def frame_norm2(base):
    """Squared norm of every frame, f64 [N][T]."""
    b = np.asarray(base, np.float64)
    return np.einsum("ntf,ntf->nt", b, b)


def norms(base, cand_t, q, n_taps=N_TAPS, tap_stride=2):
    """(cn2 [N * G], qn2 [Q]) in f64."""
    rows = stack(base, cand_t, n_taps, tap_stride)
    q = np.asarray(q, np.float64)
    return np.einsum("ck,ck->c", rows, rows), np.einsum("qk,qk->q", q, q)


def distance(q, rows):
    """[Q][C] f64: 1 - <q, c> / (|q| |c|); a row with norm < 10 eps is left unscaled (cosine_from_dot)."""
    q = np.asarray(q, np.float64)
    rows = np.asarray(rows, np.float64)
    qn2, cn2 = np.einsum("qk,qk->q", q, q), np.einsum("ck,ck->c", rows, rows)
    return distance_from_dot(q @ rows.T, qn2, cn2)


def distance_from_dot(dot, qn2, cn2):
    nq, nc = np.sqrt(qn2), np.sqrt(cn2)
    zq, zc = nq < TINY_NORM, nc < TINY_NORM
    den = np.where(zq, 1.0, nq)[:, None] * np.where(zc, 1.0, nc)[None, :]
    cross = dot / den
    degenerate = 0.5 * (np.where(zq, qn2, 1.0)[:, None] + np.where(zc, cn2, 1.0)[None, :] - 2.0 * cross)
    return np.where(zq[:, None] | zc[None, :], degenerate, 1.0 - cross)


def f64_bar(F, n_taps=N_TAPS):
    """What an f64 sweep may differ from `distance` by: the f64 dot's own gamma_K, K = n_taps F, on both sides, and the
    epilogue's handful of roundings - relative to |q||c|, i.e. absolute on the distance."""
    return (2 * n_taps * F + 16) * U64


# ---- the guards, from the inputs -------------------------------------------------------------------------------------
def mx_guard(qn2, cn2):
    """[Q][C] bool: the pairs qpg_audio_cosine_mx / _mx_h must flag (f32 operand products may underflow)."""
    p = np.asarray(qn2)[:, None] * np.asarray(cn2)[None, :]
    return (p > 0.0) & (p < MX_GUARD_P)


def hl_exponent(amax):
    """e with amax 2^e in [2^14, 2^15) (0 for amax == 0): the scale exponent of a split-f16 image."""
    amax = float(amax)
    if not amax > 0.0:
        return 0
    return int(np.clip(15 - np.frexp(np.float32(amax))[1], -100, 100))


def hl_guard(base, q, qn2, cn2):
    """[Q][C] bool: the pairs qpg_audio_cosine_hl must flag - a candidate or a query whose SCALED squared norm is below
    HL_NORM2_MIN (the database has one exponent, from the largest magnitude of the whole track; a query has its own)."""
    e_c = hl_exponent(np.abs(np.asarray(base)).max())
    q = np.asarray(q)
    e_q = np.array([hl_exponent(m) for m in np.abs(q).max(axis=1)])
    cn2, qn2 = np.asarray(cn2), np.asarray(qn2)
    c_bad = (cn2 > 0.0) & (np.ldexp(cn2, 2 * e_c) < HL_NORM2_MIN)
    q_bad = (qn2 > 0.0) & (np.ldexp(qn2, 2 * e_q) < HL_NORM2_MIN)
    return q_bad[:, None] | c_bad[None, :]


# ---- a model of the f32 accumulate ----------------------------------------------------------------------------------------
def f32_chain_dot(q32, rows32, chain=None, order=None):
    """<q, c> for every pair as a SEQUENTIAL f32 chain over the products in `order`, cut every `chain` products: a finished
    chain is added to an f64 sum and the next one starts from 0 (chain=None: one uncut chain).  [Q][C] f64."""
    q32, rows32 = np.asarray(q32, np.float32), np.asarray(rows32, np.float32)
    K = q32.shape[1]
    order = np.arange(K) if order is None else np.asarray(order)
    total = np.zeros((q32.shape[0], rows32.shape[0]), np.float64)
    acc = np.zeros(total.shape, np.float32)
    for n, k in enumerate(order):
        if chain and n % chain == 0:
            total += acc
            acc = np.zeros_like(acc)
        acc = (acc + q32[:, k, None] * rows32[None, :, k]).astype(np.float32)
    return total + acc


# ---- input families -------------------------------------------------------------------------------------------------
FAMILIES = ("grid", "samesign", "dense", "cancel", "spiky", "neardup", "zeros", "tiny", "quiet")
SAMESIGN_K0 = (4, 5, 6, 7, 8, 9)

Case = collections.namedtuple("Case", "name base q32 cand_t n_taps tap_stride plant_mx plant_hl")
Case.__doc__ = """base f32 [N][T][F], q32 f32 [Q][n_taps F]; plant_mx: the (query, window) pairs planted for the mx guard,
plant_hl: the windows planted for the hl guard (every query)."""


def row32(base, j, t0, n_taps, tap_stride):
    """Candidate / query row (window j, first frame t0) in the track's own f32: a gather, padded taps zero."""
    N, T, F = base.shape
    r = np.zeros((n_taps, F), np.float32)
    for i in range(n_taps):
        if t0 + i * tap_stride < T:
            r[i] = base[j, t0 + i * tap_stride]
    return r.reshape(-1)


def family(name, N, T, F, Q, grid, seed=0):
    """One seeded input of family `name`; grid = (cand_t, n_taps, tap_stride).

    grid      every value k 2^-6, |k| <= 64: for F <= 256 every product (k k' 2^-12, |k k'| <= 2^12) and every partial sum
              (< 6 F 2^12 <= 2^22.6 units) is exact in f32, in f16 x f16 and in f64, in any order - every kernel must return
              the exact dot, only its epilogue rounds; the squared norms are exact too.
    samesign  queries: all ones times a power of two per query; window j: every value 1 + 2^(k0 - 24) - 2^-23 with
              k0 = SAMESIGN_K0[j % 6].  Once a running f32 sum has reached 2^k0 that value's tail is below half an ulp and is
              rounded DOWN on every addition - an error that grows with the chain instead of averaging out.
    dense     Gaussian.
    cancel    features in pairs (x, -x), 16 times Gaussian, against query pairs (y, y (1 + k 2^-12)), |k| <= 2: products of
              size 16 that cancel to a dot ~1e-4 of |q||c|.
    spiky     values Gaussian times 2^-10 .. 2^0, and one feature per frame (and per query tap) of magnitude
              2^10 (1 + |Gaussian|).
    neardup   Gaussian track; query i IS a candidate (even i) or a candidate times 1 + 2^-20 Gaussian (odd i); the first
              of them is the last candidate of the last window (the one with the most padding).
    zeros     Gaussian with window 0 zero from frame T / 2 on, window 1 all zero, window 2 live ONLY in its first frames -
              where the padded taps of window 1 would land if the guard let them run on: window 1's candidates must still be
              exact zero rows - and the last query zero.
    tiny      Gaussian; window N / 2 times 2^-12 (it survives the rounding to f16) and query Q / 2 times 2^-52:
              0 < |q|^2 |c|^2 ~ 2e-33 < 1e-32 for that pair's candidates and for no other.
    quiet     Gaussian; window N / 2 times 2^-12: its scaled squared norm is ~768 2^-24 2^24 < HL_NORM2_MIN."""
    cand_t, n_taps, tap_stride = grid
    cand_t = np.asarray(cand_t, np.int32)
    rng = np.random.default_rng([seed, FAMILIES.index(name), N, T, F, Q])
    K = n_taps * F
    plant_mx, plant_hl = [], []
    if name == "grid":
        base = (rng.integers(-64, 65, size=(N, T, F)) / 64.0).astype(np.float32)
        q = (rng.integers(-64, 65, size=(Q, K)) / 64.0).astype(np.float32)
    elif name == "samesign":
        k0 = np.array(SAMESIGN_K0)[np.arange(N) % len(SAMESIGN_K0)]
        v = (1.0 + 2.0 ** (k0 - 24.0) - 2.0 ** -23).astype(np.float32)
        base = np.broadcast_to(v[:, None, None], (N, T, F)).copy()
        q = np.broadcast_to((2.0 ** rng.integers(-6, 7, size=Q)).astype(np.float32)[:, None], (Q, K)).copy()
    else:
        base = rng.standard_normal((N, T, F)).astype(np.float32)
        q = rng.standard_normal((Q, K)).astype(np.float32)
    if name == "cancel":
        base *= 16.0
        base[:, :, 1::2] = -base[:, :, 0::2]
        q[:, 1::2] = q[:, 0::2] * (1.0 + 2.0 ** -12 * rng.integers(-2, 3, size=(Q, K // 2))).astype(np.float32)
    if name == "spiky":
        base *= (2.0 ** rng.integers(-10, 1, size=base.shape)).astype(np.float32)
        spike = (1024.0 * (1.0 + np.abs(rng.standard_normal((N, T)))) * rng.choice([-1.0, 1.0], size=(N, T)))
        np.put_along_axis(base, rng.integers(0, F, size=(N, T, 1)), spike[..., None].astype(np.float32), axis=2)
        q *= (2.0 ** rng.integers(-10, 1, size=q.shape)).astype(np.float32)
        qs = q.reshape(Q, n_taps, F)
        spike = 1024.0 * (1.0 + np.abs(rng.standard_normal((Q, n_taps)))) * rng.choice([-1.0, 1.0], size=(Q, n_taps))
        np.put_along_axis(qs, rng.integers(0, F, size=(Q, n_taps, 1)), spike[..., None].astype(np.float32), axis=2)
    if name == "neardup":
        G = len(cand_t)
        pick = rng.integers(0, N * G, size=Q)
        pick[0] = N * G - 1 - int(np.argmax(cand_t[::-1]))           # the last window's latest candidate
        for i, c in enumerate(pick):
            r = row32(base, int(c) // G, int(cand_t[int(c) % G]), n_taps, tap_stride)
            if i % 2:
                r = (r * (1.0 + 2.0 ** -20 * rng.standard_normal(K))).astype(np.float32)
            q[i] = r
    if name == "zeros":
        base[0, T // 2:] = 0.0
        if N > 1:
            base[1] = 0.0
        if N > 2:
            base[2, min(T, (n_taps - 1) * tap_stride + 1):] = 0.0
        if Q > 1:
            q[Q - 1] = 0.0
    if name in ("tiny", "quiet") and N > 1:
        base[N // 2] *= np.float32(2.0 ** -12)
        plant_hl.append(N // 2)
    if name == "tiny" and N > 1:
        q[Q // 2] *= np.float32(2.0 ** -52)
        plant_mx.append((Q // 2, N // 2))
    return Case(name, base, q, cand_t, n_taps, tap_stride, plant_mx, plant_hl)


def planted_mask(case, which):
    """[Q][C] bool of what the family planted for the `which` ('mx' / 'hl') guard."""
    N, G, Q = case.base.shape[0], len(case.cand_t), case.q32.shape[0]
    m = np.zeros((Q, N, G), bool)
    if which == "mx":
        for qi, j in case.plant_mx:
            m[qi, j] = True
    else:
        for j in case.plant_hl:
            m[:, j] = True
    return m.reshape(Q, N * G)
