"""The seven split-f16 pack entry points against the format itself (tests/hl_layout_ref.py): every byte of every image equal
to what the format prescribes for the input, the exponents behind the fragments (live queries) resp. meta[0] of the 64-byte
tail, zero pieces in the padding slots, and guard bytes around every output buffer untouched.  The other tests reach these
images only through a GEMM or by comparing two packers with each other.

Shapes: the smallest at which each rule can go wrong - F = 128 (KB = 12, the least the grid check admits) and 256; one and
three windows; T = 180 (every frame inside the track) and 157 (the last super-row's frames 158, 160 beyond it: zero-filled);
Q = 1, 48, 49 (a second audio chunk with 47 padding slots); D = 128, 384; R = 32, 96; Q = 1, 96, 97 for the column image.
Inputs: log-uniform magnitudes over twelve decades (l planes with f16 subnormals), one element that sets the exponent, an
all-zero query (exponent 0).
The normalised text queries (qn) come from oracle.knn_oracle.l2_normalize - NumPy, in einsum's order - not from
tests/helpers.py: what helpers.py offers is a call to qpg_l2_normalize_rows_f32, which runs the same einsum_norm_f32 as
the packs under test."""
import functools

import numpy as np
import pytest

from tests import hl_layout_ref as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, FILL = 256, 0xA5
TS, STEP, G, TAPS = 2, 6, 26, 6


def values(seed, *shape):
    rng = np.random.default_rng([seed] + list(shape))
    x = (rng.standard_normal(shape) * np.exp(rng.uniform(np.log(1e-12), 0.0, shape))).astype(np.float32)
    x.reshape(-1)[rng.integers(0, x.size)] = 300.0                          # sets the exponent of its image / query
    return x


class Guarded:
    """An output buffer of nbytes between two guard zones, all of it pre-filled with FILL."""

    def __init__(self, nbytes, dtype=None):
        import torch
        self.n = int(nbytes)
        self.full = torch.full((self.n + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
        self.buf = self.full[GUARD:GUARD + self.n]
        if dtype is not None:
            self.buf = self.buf.view(dtype)

    def bytes(self):
        """The payload as a NumPy uint8 array, after checking the guards."""
        full = self.full.cpu().numpy()
        assert np.all(full[:GUARD] == FILL) and np.all(full[GUARD + self.n:] == FILL), "bytes outside the buffer were written"
        return full[GUARD:GUARD + self.n]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)                 # (a copy: the shared inputs are read-only)


def lib_call(*args):
    from qpgesture_amd import _lib
    _lib.call(args[0], DEV, *args[1:])


def size_of(name, *args):
    from qpgesture_amd import _lib
    return int(getattr(_lib.load(), name)(*args))


def assert_cols_image(got, want, Q):
    """A column / audio query image: the fragments byte for byte, the exponents of the live queries."""
    nf = want.frags.size
    assert got.size == nf + 4 * want.exps.size
    assert np.array_equal(got[:nf], want.frags)
    assert np.array_equal(got[nf:].view(np.int32)[:Q], want.exps[:Q])


# ---- audio database images ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def track(N, T, F):
    x = values(1, N, T, F)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("T", [180, 157])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("F", [128, 256])
def test_audio_database_image_two_planes(F, N, T):
    base = track(N, T, F)
    want = L.db_image(base, STEP, TS, 2)
    nb = size_of("qpg_audio_hl_db_bytes", N, F)
    assert nb == want.frags.size + L.META_BYTES
    out = Guarded(nb)
    lib_call("qpg_audio_hl_pack_db", dev(base), N, T, F, G, TAPS, TS, STEP, out.buf, nb)
    got = out.bytes()
    assert np.array_equal(got[:want.frags.size], want.frags)
    assert got[want.frags.size:].view(np.int32)[0] == want.exps[0]


@pytest.mark.parametrize("T", [180, 157])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("F", [128, 256])
def test_audio_database_image_one_plane(F, N, T):
    base = track(N, T, F).astype(np.float16)
    want = L.db_image(base, STEP, TS, 1)
    nb = size_of("qpg_audio_hl1_db_bytes", N, F)
    assert nb == want.frags.size
    out = Guarded(nb)
    lib_call("qpg_audio_hl1_pack_db", dev(base), N, T, F, G, TAPS, TS, STEP, out.buf, nb)
    assert np.array_equal(out.bytes(), want.frags)


# ---- audio query image: from packed queries, and the two gathering packs ----------------------------------------------------------
M_Q, T_Q = 2, 157


@functools.lru_cache(maxsize=None)
def clip(F, Q):
    """A clip's track [M_Q][T_Q][F], the (window, first frame) of Q queries and the queries themselves [Q][6 F]: query 3 reads
    twelve silent frames (a zero query), the last one starts at frame 150 (its taps 158, 160 lie beyond the track)."""
    rng = np.random.default_rng([2, F, Q])
    x = values(2, M_Q, T_Q, F)
    x[1, 40:52] = 0.0
    win = rng.integers(0, M_Q, Q).astype(np.int32)
    t0 = rng.integers(0, T_Q - 2 * TAPS, Q).astype(np.int32)
    if Q > 3:
        win[3], t0[3] = 1, 40
    t0[Q - 1] = 150
    q32 = np.zeros((Q, TAPS, F), np.float32)
    for q in range(Q):
        for tap in range(TAPS):
            t = t0[q] + tap * TS
            if t < T_Q:
                q32[q, tap] = x[win[q], t]
    q32 = q32.reshape(Q, TAPS * F)
    assert (Q <= 3 or not q32[3].any()) and q32[Q - 1, :4 * F].any() and not q32[Q - 1, 4 * F:].any()
    for a in (x, win, t0, q32):
        a.setflags(write=False)
    return x, win, t0, q32


@functools.lru_cache(maxsize=None)
def audio_query_ref(F, Q):
    return L.audio_query_image(clip(F, Q)[3])


@pytest.mark.parametrize("Q", [1, 48, 49])
@pytest.mark.parametrize("F", [128, 256])
def test_audio_query_image_from_packed_queries(F, Q):
    want = audio_query_ref(F, Q)
    nb = size_of("qpg_audio_hl_query_bytes", Q, F)
    out = Guarded(nb)
    lib_call("qpg_audio_hl_pack_queries", dev(clip(F, Q)[3]), Q, F, out.buf, nb)
    assert_cols_image(out.bytes(), want, Q)


def assert_audio_gather(F, Q, q32_out, qn2_out, image_out):
    q32 = clip(F, Q)[3]
    assert np.array_equal(q32_out.bytes().view(np.float32).reshape(Q, -1), q32)
    qn2 = (q32.astype(np.float64) ** 2).sum(axis=1)
    got = qn2_out.bytes().view(np.float64)
    print("qn2: largest relative difference %.3g" % np.max(np.abs(got - qn2) / np.maximum(qn2, 1e-300)))
    assert np.all(np.abs(got - qn2) <= 1e-12 * qn2)                       # (the kernel's own summation order)
    assert_cols_image(image_out.bytes(), audio_query_ref(F, Q), Q)


@pytest.mark.parametrize("Q", [1, 48, 49])
@pytest.mark.parametrize("F", [128, 256])
def test_audio_query_image_from_the_gathering_pack(F, Q):
    import torch
    x, win, t0, _ = clip(F, Q)
    nb = size_of("qpg_audio_hl_query_bytes", Q, F)
    q32, qn2, image = Guarded(Q * TAPS * F * 4, torch.float32), Guarded(Q * 8, torch.float64), Guarded(nb)
    lib_call("qpg_audio_pack_queries_hl", dev(x), M_Q, T_Q, F, dev(win), dev(t0), Q, TAPS, TS, q32.buf, qn2.buf, image.buf, nb)
    assert_audio_gather(F, Q, q32, qn2, image)


# ---- column image: from normalised queries, and the two normalising packs -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raw_queries(Q, D):
    """Raw (not normalised) queries [Q][D]; query 3 is all zero when Q > 3."""
    q = values(3, Q, D)
    if Q > 3:
        q[3] = 0.0
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def normalised(Q, D):
    """sklearn's f32 normalisation in the reference's (NumPy einsum's) order, and the column image of the result."""
    from oracle import knn_oracle as O
    qn = O.l2_normalize(raw_queries(Q, D))
    assert qn.dtype == np.float32
    qn.setflags(write=False)
    return qn, L.cols_image(qn)


@pytest.mark.parametrize("Q", [1, 96, 97])
@pytest.mark.parametrize("D", [128, 384])
def test_column_image(D, Q):
    qn, want = normalised(Q, D)
    nb = size_of("qpg_hl_cols_bytes", Q, D)
    out = Guarded(nb)
    lib_call("qpg_hl_pack_cols", dev(qn), Q, D, out.buf, nb)
    assert_cols_image(out.bytes(), want, Q)


@pytest.mark.parametrize("Q", [1, 96, 97])
@pytest.mark.parametrize("D", [128, 384])
def test_column_image_from_raw_queries(D, Q):
    import torch
    qn, want = normalised(Q, D)
    nb = size_of("qpg_hl_cols_bytes", Q, D)
    qn_out, out = Guarded(Q * D * 4, torch.float32), Guarded(nb)
    lib_call("qpg_hl_prepare_queries", dev(raw_queries(Q, D)), Q, D, qn_out.buf, out.buf, nb, None)
    assert np.array_equal(qn_out.bytes().view(np.int32), qn.view(np.int32).reshape(-1))
    assert_cols_image(out.bytes(), want, Q)


@pytest.mark.parametrize("R", [32, 96])
@pytest.mark.parametrize("D", [128, 384])
def test_row_image(D, R):
    x = values(4, R, D)
    want = L.rows_image(x)
    nb = size_of("qpg_hl_rows_bytes", R, D)
    assert nb == want.frags.size + L.META_BYTES
    out = Guarded(nb)
    lib_call("qpg_hl_pack_rows", dev(x), R, D, out.buf, nb)
    got = out.bytes()
    assert np.array_equal(got[:want.frags.size], want.frags)
    assert got[want.frags.size:].view(np.int32)[0] == want.exps[0]


# ---- a clip's whole query side in one launch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,Q,Dt,Qt", [(128, 1, 128, 1), (128, 49, 384, 96), (256, 48, 128, 97), (256, 49, 384, 97)])
def test_clip_pack_writes_both_images(F, Q, Dt, Qt):
    """qpg_clip_pack_hl: the audio side as the gathering pack, the text side = context rows gathered by (window, row),
    normalised like the reference, and their column image."""
    import torch
    x, win, t0, _ = clip(F, Q)
    Mt, R = 4, 30
    slot = np.random.default_rng([5, Dt, Qt]).permutation(Mt * R)[:Qt]          # every query its own context row
    twin, trow = (slot // R).astype(np.int32), (slot % R).astype(np.int32)
    ctx = values(5, Mt, R, Dt)
    ctx.reshape(Mt * R, Dt)[slot] = raw_queries(Qt, Dt)
    qn, want_cols = normalised(Qt, Dt)
    nb, nbt = size_of("qpg_audio_hl_query_bytes", Q, F), size_of("qpg_hl_cols_bytes", Qt, Dt)
    q32, qn2, image = Guarded(Q * TAPS * F * 4, torch.float32), Guarded(Q * 8, torch.float64), Guarded(nb)
    qn_out, cols = Guarded(Qt * Dt * 4, torch.float32), Guarded(nbt)
    lib_call("qpg_clip_pack_hl", dev(x), M_Q, T_Q, F, dev(win), dev(t0), Q, TAPS, TS, q32.buf, qn2.buf, image.buf, nb,
             dev(ctx), Mt, R, Dt, dev(twin), dev(trow), Qt, qn_out.buf, cols.buf, nbt)
    assert_audio_gather(F, Q, q32, qn2, image)
    assert np.array_equal(qn_out.bytes().view(np.int32), qn.view(np.int32).reshape(-1))
    assert_cols_image(cols.bytes(), want_cols, Qt)
