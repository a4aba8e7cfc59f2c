"""NumPy statement of the split-f16 operand images (csrc/qpg_audio_hl.hip: hl_split8, hl_store_col_piece, hl_db_unit,
hl_db_piece, the image views) - the byte image the FORMAT prescribes for given inputs.  No torch, no GPU:
tests/test_prefilter_contract_cpu.py checks this module against itself (the images decode back to their inputs, every
fragment byte is written once), tests/test_gpu_pack_layout.py holds the pack kernels to it, byte for byte.

The format: every value is scaled by a power of two (prefilter_ref.exponent of the largest magnitude: one exponent per
database / row image, one per query) and stored as two f16 numbers,
  generic split   h = fl16(x 2^e), l = fl16((x 2^e - h) 2^11)         (prefilter_ref.split: row and column images)
  audio split     h = fl16(x 2^e), l = fl16(x 2^e - h)                  (audio database and query images)
in 16-BYTE PIECES of eight consecutive elements k .. k + 7, placed in MFMA fragment order: a fragment is [64 lanes][8 f16],
lane = (row or query) % 16 + 16 * ((k % 32) / 8), one fragment per (16 rows or queries, k-block of 32 elements, plane).

  audio database, PL planes (2: h | l, from f32; 1: the f16 track itself, no scaling), per window
      [tile 0: KB k-blocks][PL planes][64 units]  then  [tile 1: KB][PL][44 units],      KB = 3 F / 32
      row of a window = SUPER-ROW i < 27 = frames step i + tap_stride {0, 1, 2} side by side (3 F elements; frames beyond
      the track are zeros); tile 0 = super-rows 0..15 (unit = i + 16 kg), tile 1 = super-rows 16..26 (unit = 11 kg + i - 16)
      two planes: + 64 bytes of metadata, int32 [0] = the exponent
  audio query image   [chunk of 48 queries][KB][6 column tiles][2 planes][64 lanes][8], column tile = half * 3 + (q % 48) / 16
      (half 0 / 1 = the first / last three taps of the query), then int32 exponents [chunks * 48]
  row image           [R / 32][2 row tiles][KB = D / 32][2 planes][64][8], then 64 bytes of metadata, int32 [0] = the exponent
  column image        [chunk of 96 queries][KB][6 column tiles][2 planes][64][8], column tile = (q % 96) / 16, then int32
      exponents [chunks * 96]
Padding slots (queries past Q in the last chunk) are zero pieces; their exponent words, like the metadata tail beyond
[0], are not part of the format.

Every builder returns an Image: frags (uint8, the fragment bytes), exps (the int32 exponents: [1] or [chunks * QC], padding
slots 0), writes (how often each 16-byte unit was written)."""
import collections

import numpy as np

from tests.prefilter_ref import exponent, split

ROWS, SUB, QC, GQC, CT, T1_UNITS, META_BYTES = 27, 3, 48, 96, 6, 44, 64
Image = collections.namedtuple("Image", "frags exps writes")


def split_audio(x, e):
    """split_hl_audio on x 2^e: (h, l) float16 arrays, l = fl16(x 2^e - h) at its true scale."""
    xs = np.asarray(x, np.float32) * np.float32(2.0 ** int(e))
    h = xs.astype(np.float16)
    return h, (xs - h.astype(np.float32)).astype(np.float16)


def _amax(x):
    return np.abs(np.asarray(x, np.float32)).max(initial=0.0)


def _put(units, writes, u, pieces):
    units[u] = pieces
    np.add.at(writes, u, 1)


def _image(units, exps, writes):
    return Image(units.view(np.uint8).reshape(-1), np.asarray(exps, np.int32).reshape(-1), writes)


# ---- audio database ---------------------------------------------------------------------------------------------------------
def db_image(base, step, tap_stride, planes):
    """base [N][T][F]: f32 (planes = 2) or f16 (planes = 1)."""
    base = np.asarray(base)
    assert base.dtype == (np.float32 if planes == 2 else np.float16)
    N, T, F = base.shape
    KB, K8 = SUB * F // 32, SUB * F // 8
    win = KB * planes * (64 + T1_UNITS)
    units = np.zeros((N * win, 8), np.float16)
    writes = np.zeros(N * win, np.int64)
    e = exponent(_amax(base)) if planes == 2 else 0
    k = np.arange(K8) * 8
    kb, kg, sub, f = k // 32, (k % 32) // 8, k // F, k % F
    for j in range(N):
        for i in range(ROWS):
            t = step * i + tap_stride * sub
            x = np.zeros((K8, 8), base.dtype)
            ok = t < T
            x[ok] = base[j][t[ok][:, None], f[ok][:, None] + np.arange(8)]
            if i < 16:
                u, stride = j * win + kb * planes * 64 + i + 16 * kg, 64
            else:
                u, stride = j * win + KB * planes * 64 + kb * planes * T1_UNITS + 11 * kg + (i - 16), T1_UNITS
            if planes == 2:
                h, l = split_audio(x, e)
                _put(units, writes, u, h)
                _put(units, writes, u + stride, l)
            else:
                _put(units, writes, u, x)
    return _image(units, [e], writes)


def db_decode(img, N, F, planes):
    """The reader's view of a database image: -> [planes][N][27 super-rows][3 F] f16."""
    KB = SUB * F // 32
    w = np.asarray(img.frags).view(np.float16).reshape(N, KB * planes * (64 + T1_UNITS) * 8)
    t0 = w[:, :KB * planes * 64 * 8].reshape(N, KB, planes, 4, 16, 8)                 # [kb][plane][kg][row][8]
    t1 = w[:, KB * planes * 64 * 8:].reshape(N, KB, planes, 4, 11, 8)
    rows = np.concatenate([t0, t1], axis=4)                                            # [N][kb][plane][kg][27][8]
    return rows.transpose(2, 0, 4, 1, 3, 5).reshape(planes, N, ROWS, SUB * F)


def super_rows(base, step, tap_stride):
    """base [N][T][F] -> [N][27][3 F]: the rows a database image holds (zeros beyond the track)."""
    base = np.asarray(base)
    N, T, F = base.shape
    out = np.zeros((N, ROWS, SUB, F), base.dtype)
    for i in range(ROWS):
        for s in range(SUB):
            t = step * i + tap_stride * s
            if t < T:
                out[:, i, s] = base[:, t]
    return out.reshape(N, ROWS, SUB * F)


# ---- column images: the audio query image and the generic column image -----------------------------------------------------------
def _cols(rows, halves, qc, splitter):
    """rows [Q][halves * K]: query q's K elements of half `half` go to column tile half * 3 + (q % qc) / 16."""
    rows = np.asarray(rows, np.float32)
    Q, K = rows.shape[0], rows.shape[1] // halves
    KB, chunks = K // 32, (Q + qc - 1) // qc
    units = np.zeros((chunks * KB * CT * 2 * 64, 8), np.float16)
    writes = np.zeros(units.shape[0], np.int64)
    exps = np.zeros(chunks * qc, np.int32)
    k = np.arange(K // 8) * 8
    kb, kg = k // 32, (k % 32) // 8
    for q in range(chunks * qc):
        live = q < Q
        if live:
            exps[q] = exponent(_amax(rows[q]))
        chunk, qq = q // qc, q % qc
        for half in range(halves):
            x = rows[q, half * K:(half + 1) * K].reshape(-1, 8) if live else np.zeros((K // 8, 8), np.float32)
            h, l = splitter(x, exps[q])
            piece = ((chunk * KB + kb) * CT + half * 3 + qq // 16) * 2
            lane = qq % 16 + 16 * kg
            _put(units, writes, piece * 64 + lane, h)
            _put(units, writes, (piece + 1) * 64 + lane, l)
    return _image(units, exps, writes)


def audio_query_image(q32):
    """q32 [Q][6 F] f32 (six taps of F features)."""
    return _cols(q32, 2, QC, split_audio)


def cols_image(q):
    """q [Q][D] f32."""
    return _cols(q, 1, GQC, split)


def cols_decode(img, K, halves, qc):
    """The reader's view of a column image: -> [2 planes][chunks * qc query slots][halves * K] f16."""
    KB = K // 32
    w = np.asarray(img.frags).view(np.float16).reshape(-1, KB, CT, 2, 4, 16, 8)       # [chunk][kb][ct][plane][kg][q % 16][8]
    chunks = w.shape[0]
    w = w.transpose(3, 0, 2, 5, 1, 4, 6).reshape(2, chunks, CT * 16, K)               # [plane][chunk][ct * 16 + q % 16][k]
    if halves == 2:                                                                   # ct = half * 3 + qq / 16
        w = w.reshape(2, chunks, 2, qc, K).transpose(0, 1, 3, 2, 4)
    return w.reshape(2, chunks * qc, halves * K)


# ---- row image ------------------------------------------------------------------------------------------------------------------
def rows_image(x):
    """x [R][D] f32, R % 32 == 0."""
    x = np.asarray(x, np.float32)
    R, D = x.shape
    KB = D // 32
    units = np.zeros((R * D // 8 * 2, 8), np.float16)
    writes = np.zeros(units.shape[0], np.int64)
    e = exponent(_amax(x))
    k = np.arange(D // 8) * 8
    kb, kg = k // 32, (k % 32) // 8
    for row in range(R):
        i, j = row % 32, row // 32
        h, l = split(x[row].reshape(-1, 8), e)
        piece = ((j * 2 + i // 16) * KB + kb) * 2
        lane = i % 16 + 16 * kg
        _put(units, writes, piece * 64 + lane, h)
        _put(units, writes, (piece + 1) * 64 + lane, l)
    return _image(units, [e], writes)


def rows_decode(img, D):
    """The reader's view of a row image: -> [2 planes][R][D] f16."""
    KB = D // 32
    w = np.asarray(img.frags).view(np.float16).reshape(-1, KB, 2, 4, 16, 8)           # [16-row tile][kb][plane][kg][row][8]
    return w.transpose(2, 0, 4, 1, 3, 5).reshape(2, -1, D)
