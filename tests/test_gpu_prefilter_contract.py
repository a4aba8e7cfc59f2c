"""The first half of the prefilter's contract: the split-f16 GEMMs are within their A-PRIORI bounds of the real-number
1 - <x, q>, and their tile minima and row masks are what include/qpg.h says (the second half - given ANY values inside the
bound the selects return the exact sweep's tables - is tests/test_gpu_select_contract.py).  Every entry point is called
directly, at the smallest shapes where its kernel can go wrong, on the adversarial rows of tests/prefilter_ref.py, into
NaN / zero pre-filled outputs with oversized leading dimensions and a guard row.

Dispatch (part of what is tested):
  qpg_hl_gemm_distance / qpg_hl_gemm_tilemin   Q <= 48: hl_gemm16_kernel (f64 block sums), bound sorted_rows.HL_GEMM_ERR;
                                               Q  > 48: hl_gemm32_kernel (f32 chains over K), bound gemm32_err(D), persistent
                                               blocks = min(items, CUs), items = ceil(R / 256) x ceil(Q / 96);
  qpg_hl_gemm_tilemin_h                        hl_gemm64h_kernel<6, PAIR = (D / 128 even), 4>, R % 64 == 0, blocks =
                                               min(items, 2 CUs), same items; against the h planes' exact sum within the
                                               chain + f32 epilogue (gemm32_err(D) - 5.2e-7 + 1.2e-7), against the true
                                               value within gemm_h_err(D).
Both persistent kernels take the XCD-aware item order only when their block count is a multiple of 8.

No bar here is tuned to what the kernels return: each is one of the project's own bounds (qpgesture_amd.sorted_rows), the
chain term named above, or bit equality.  A mask word is never 0 (the minimum's own bit is always set), so 0 is the masks'
"never written" value.  Lines starting with PREFILTER carry the measured worst error / bound."""
import numpy as np
import pytest

from tests import prefilter_ref as P

pytestmark = pytest.mark.gpu

# (R, Q, D): what each is the smallest case of
CASES = [
    (64, 1, 128),       # hl_gemm16_kernel, one trip of its two-stage loop, one 16-query tile partly live; gemm64h with a
    (64, 5, 128),       # single stage (not PAIR); Q = 5: the zero query (3) is in
    (64, 48, 128),      # the last Q on hl_gemm16_kernel
    (96, 48, 384),      # the matcher's width; three 32-row groups in a block of four; the h form must refuse R % 64 != 0
    (320, 49, 384),     # first Q on hl_gemm32_kernel; ten row groups = row blocks of 8 + 2
    (320, 97, 384),     # a second chunk with ONE live query; item count not a multiple of 8
    (576, 100, 512),    # gemm64h PAIR; nine 64-row groups = three row blocks of four waves, the last with one live wave
    (576, 200, 640),    # 20-instruction chains (gemm32_err beyond 16); five stages (not PAIR); three chunks
    (1024, 96, 1024),   # 32-instruction chains; exactly one full chunk
]


def _bits(a):
    """The storage of a numpy array as integers (NaN payloads and signed zeros compare as what they are)."""
    return a.view({4: np.int32, 2: np.int16}[a.dtype.itemsize])


def _untouched_outside(after, before, n0, n1):
    """True iff nothing but [0:n0][0:n1] differs from the pre-filled array."""
    outside = np.ones(after.shape, bool)
    outside[:n0, :n1] = False
    return bool((_bits(after)[outside] == _bits(before)[outside]).all())


class _Images:
    """xs / qn packed on the device: the row image and the column image, as the product packs them."""

    def __init__(self, xs, qn):
        import torch
        from qpgesture_amd import _lib
        self.dev = torch.device("cuda:0")
        lib = _lib.load()
        self.R, self.D, self.Q = xs.shape[0], xs.shape[1], qn.shape[0]
        self.xs_t = torch.from_numpy(xs).to(self.dev)
        self.qn_t = torch.from_numpy(qn).to(self.dev)
        # the pack kernels write every fragment the GEMMs read (the last column chunk's padding queries as zeros): what the
        # images held before is ignored, so they start from a plausible non-zero pattern, not from zeros
        self.rows = torch.full((int(lib.qpg_hl_rows_bytes(self.R, self.D)),), 0x3C, dtype=torch.uint8, device=self.dev)
        self.cols = torch.full((int(lib.qpg_hl_cols_bytes(self.Q, self.D)),), 0x3C, dtype=torch.uint8, device=self.dev)
        _lib.call("qpg_hl_pack_rows", self.dev, self.xs_t, self.R, self.D, self.rows, self.rows.numel())
        _lib.call("qpg_hl_pack_cols", self.dev, self.qn_t, self.Q, self.D, self.cols, self.cols.numel())

    def exponents(self):
        """(meta[0], the live queries' exponents) read from the images: the first i32 of the row image's last 64 bytes; the
        i32 array behind the chunks x (D / 32) x 6 x 2 x 1024 fragment bytes of the column image."""
        chunks = (self.Q + 95) // 96
        meta = self.rows[-64:].cpu().numpy().view(np.int32)
        qexp = self.cols[chunks * (self.D // 32) * 6 * 2 * 1024:].cpu().numpy().view(np.int32)
        return int(meta[0]), qexp[:self.Q].astype(np.int64)


class _Outputs:
    """Pre-filled outputs with slack: ldD = R + 8, ldT = R / 16 + 3, ldQ = Q rounded up to 16, plus 16; one guard row each."""

    def __init__(self, im):
        import torch
        R, Q, dev = im.R, im.Q, im.dev
        self.ldD, self.ldT, self.ldQ = R + 8, R // 16 + 3, (Q + 15) // 16 * 16 + 16
        nan = float("nan")
        self.t = dict(Dm=torch.full((Q + 1, self.ldD), nan, dtype=torch.float32, device=dev),
                      tmin_d=torch.full((Q + 1, self.ldT), nan, dtype=torch.float32, device=dev),
                      tmin_m=torch.full((Q + 1, self.ldT), nan, dtype=torch.float32, device=dev),
                      mask_m=torch.zeros((Q + 1, self.ldT), dtype=torch.int16, device=dev),
                      tmin_h=torch.full((R // 16 + 1, self.ldQ), nan, dtype=torch.float32, device=dev),
                      mask_h=torch.zeros((R // 16 + 1, self.ldQ), dtype=torch.int16, device=dev))
        self.before = {k: v.cpu().numpy() for k, v in self.t.items()}

    def fetch(self):
        import torch
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def _run(xs, qn):
    """All three entry points on (xs, qn) -> images, outputs object, fetched arrays, whether the h form accepted the shape."""
    from qpgesture_amd import _lib
    from qpgesture_amd.sorted_rows import prefilter_band, prefilter_band_h
    im = _Images(xs, qn)
    o = _Outputs(im)
    R, Q, D, t = im.R, im.Q, im.D, o.t
    _lib.call("qpg_hl_gemm_distance", im.dev, im.rows, R, D, im.cols, Q, t["Dm"], o.ldD, t["tmin_d"], o.ldT)
    _lib.call("qpg_hl_gemm_tilemin", im.dev, im.rows, R, D, im.cols, Q, float(prefilter_band(D)), t["tmin_m"], t["mask_m"],
              o.ldT)
    h_ok = R % 64 == 0
    if h_ok:
        _lib.call("qpg_hl_gemm_tilemin_h", im.dev, im.rows, R, D, im.cols, Q, float(prefilter_band_h(D)), t["tmin_h"],
                  t["mask_h"], o.ldQ)
    else:
        with pytest.raises(RuntimeError):
            _lib.call("qpg_hl_gemm_tilemin_h", im.dev, im.rows, R, D, im.cols, Q, float(prefilter_band_h(D)), t["tmin_h"],
                      t["mask_h"], o.ldQ)
    return im, o, o.fetch(), h_ok


def _check(xs, qn, tag):
    """Items 1-6 of the contract on one image.  Every figure is printed before anything is asserted; all misses are
    reported together."""
    from qpgesture_amd.sorted_rows import HL_GEMM_ERR, gemm32_err, gemm_h_err, prefilter_band, prefilter_band_h
    R, D, Q, T = xs.shape[0], xs.shape[1], qn.shape[0], xs.shape[0] // 16
    im, o, got, h_ok = _run(xs, qn)
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(what)

    band, band_h = prefilter_band(D), prefilter_band_h(D)
    E = HL_GEMM_ERR if Q <= 48 else gemm32_err(D)                 # the dispatch rule: <= 48 queries stay on the 16-row kernel
    E_chain = gemm32_err(D) - 5.2e-7 + 1.2e-7
    kern = "gemm16" if Q <= 48 else "gemm32"
    nx = np.sqrt((xs.astype(np.float64) ** 2).sum(axis=1))
    nq = np.sqrt((qn.astype(np.float64) ** 2).sum(axis=1))
    zero_tile = (nx.reshape(T, 16) == 0).all(axis=1)
    zero_q = nq == 0
    assert zero_tile[-1] and (Q <= 3 or zero_q[3])
    ex = P.exact(xs, qn)

    # 1. coverage: everything inside written, nothing outside touched
    Dm, tmin_d, tmin_m = got["Dm"][:Q, :R], got["tmin_d"][:Q, :T], got["tmin_m"][:Q, :T]
    mask_m = got["mask_m"][:Q, :T].view(np.uint16)
    need(not np.isnan(Dm).any(), "Dm: %d values never written" % np.isnan(Dm).sum())
    need(not np.isnan(tmin_d).any() and not np.isnan(tmin_m).any(), "tile_min: values never written")
    need((mask_m != 0).all(), "tile_mask: %d words never written" % (mask_m == 0).sum())
    for k, n0, n1 in (("Dm", Q, R), ("tmin_d", Q, T), ("tmin_m", Q, T), ("mask_m", Q, T)):
        need(_untouched_outside(got[k], o.before[k], n0, n1), "%s: written outside [%d][%d]" % (k, n0, n1))
    if h_ok:
        tmin_h = np.ascontiguousarray(got["tmin_h"][:T, :Q].T)
        mask_h = np.ascontiguousarray(got["mask_h"][:T, :Q].T).view(np.uint16)
        need(not np.isnan(tmin_h).any(), "tile_min_t: %d values never written" % np.isnan(tmin_h).sum())
        need((mask_h != 0).all(), "tile_mask_t: %d words never written" % (mask_h == 0).sum())
        for k in ("tmin_h", "mask_h"):
            need(_untouched_outside(got[k], o.before[k], T, Q), "%s: written outside [%d][%d]" % (k, T, Q))
    else:
        for k in ("tmin_h", "mask_h"):
            need(np.array_equal(_bits(got[k]), _bits(o.before[k])), "%s: touched by a refused call" % k)

    # 2. the matrix forms within their bound of the real value; zero operands give exactly 1
    bound = E * nq[:, None] * nx[None, :]
    err = np.abs(Dm.astype(np.float64) - ex)
    live = bound > 0
    r2 = float((err[live] / bound[live]).max())
    print("PREFILTER %s R=%d Q=%d D=%d %s matrix: worst |Dm - exact| / bound = %.3f (bound %.3g)" % (tag, R, Q, D, kern, r2, E))
    need(r2 <= 1.0, "matrix form outside its bound: %.3f x %.3g" % (r2, E))
    need((Dm[~live] == np.float32(1.0)).all(), "zero rows / the zero query do not give exactly 1.0f")

    # 3. the forms agree bit for bit; the masks are the f32 rule on the kernel's own values
    need(np.array_equal(_bits(tmin_d), _bits(P.tile_min(Dm))), "qpg_hl_gemm_distance: tile_min is not the minimum of its Dm")
    need(np.array_equal(_bits(tmin_d), _bits(tmin_m)), "tile_min of qpg_hl_gemm_tilemin differs from qpg_hl_gemm_distance's")
    need(np.array_equal(mask_m, P.mask_rule(Dm, band)), "tile_mask is not mask_rule(Dm, band)")
    v_full = P.mask_verdict(ex, band, E * float((nq.max() * nx.max())))
    und_full = float((v_full == 0).mean())
    need(und_full <= 0.10, "full-precision setting: %.3f of the mask bits undecided" % und_full)
    b_m = P.mask_bits(mask_m)
    need(b_m[v_full == 1].all() and not b_m[v_full == -1].any(), "tile_mask contradicts the verdict of the exact values")

    # 6. exponents
    e_c, e_q = im.exponents()
    need(e_c == P.row_exponent(xs), "meta[0] = %d, expected %d" % (e_c, P.row_exponent(xs)))
    need(np.array_equal(e_q, P.query_exponents(qn)), "query exponents differ")
    if not h_ok:
        print("PREFILTER %s R=%d Q=%d D=%d gemm64h: refused (R %% 64 != 0)" % (tag, R, Q, D))
        assert not bad, "\n".join(bad)
        return

    # 4. the h-plane form against the h planes' exact sum: chain + f32 epilogue
    ex_h = P.exact_h(xs, qn)
    r4 = float(np.abs(tmin_h.astype(np.float64) - P.tile_min(ex_h)).max() / E_chain)
    r5 = float(np.abs(tmin_h.astype(np.float64) - P.tile_min(ex)).max() / gemm_h_err(D))
    print("PREFILTER %s R=%d Q=%d D=%d gemm64h%s tile minima: worst error / bound = %.3f against the h planes (bound %.3g), "
          "%.3f against the true value (bound %.3g)" % (tag, R, Q, D, " PAIR" if (D // 128) % 2 == 0 else "", r4, E_chain, r5,
                                                        gemm_h_err(D)))
    need(r4 <= 1.0, "h-plane minima outside chain + epilogue: %.3f x %.3g" % (r4, E_chain))
    v_h = P.mask_verdict(ex_h, band_h, E_chain)
    und_h = float((v_h == 0).mean())
    print("PREFILTER %s R=%d Q=%d D=%d undecided mask bits: %.4f (full), %.4f (h)" % (tag, R, Q, D, und_full, und_h))
    need(und_h <= 0.10, "h setting: %.3f of the mask bits undecided" % und_h)
    b_h = P.mask_bits(mask_h)
    need(b_h[v_h == 1].all(), "%d mask bits that must be set are clear" % (~b_h[v_h == 1]).sum())
    need(not b_h[v_h == -1].any(), "%d mask bits that must be clear are set" % b_h[v_h == -1].sum())
    arg = ex_h.reshape(Q, T, 16).argmin(axis=2)
    need(np.take_along_axis(b_h, arg[:, :, None], axis=2).all(), "a tile's argmin row is not in its mask")
    z = zero_q[:, None] | zero_tile[None, :]
    need((tmin_h[z] == np.float32(1.0)).all() and (mask_h[z] == 0xffff).all(), "zero tiles / the zero query: not 1.0f / 0xffff")

    # 5. ... and against the true value
    need(r5 <= 1.0, "h-plane minima outside gemm_h_err: %.3f x %.3g" % (r5, gemm_h_err(D)))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("R,Q,D", CASES, ids=["%dx%dx%d" % c for c in CASES])
def test_prefilter_gemms_at_the_smallest_shapes(R, Q, D):
    seed = CASES.index((R, Q, D))
    qn = P.queries(Q, D, seed)
    xs, _ = P.rows_mixed(R, qn, seed)
    _check(xs, qn, "small")


def test_prefilter_gemms_with_more_items_than_blocks():
    """Both persistent kernels with blocks that run more than one item, in the XCD-aware order: Q = 769 (nine chunks, the
    last with one live query), D = 128, R = 256 (2 CUs // 9 + 3)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Q, D = 769, 128
    R = 256 * (2 * cus // 9 + 3)
    chunks = (Q + 95) // 96
    items = (R + 255) // 256 * chunks                 # the same for both kernels: row blocks of 8 x 32 and of 4 x 64 rows
    blocks32, blocks64 = min(items, cus), min(items, 2 * cus)
    numbers = "CUs %d, R %d, items %d, blocks %d (gemm32) / %d (gemm64h)" % (cus, R, items, blocks32, blocks64)
    print("PREFILTER many:", numbers)
    if not (items > blocks32 and items > blocks64 and blocks32 % 8 == 0 and blocks64 % 8 == 0):
        pytest.skip("this device does not give persistent blocks several items in the XCD-aware order: " + numbers)
    qn = P.queries(Q, D, 11)
    xs, _ = P.rows_dense_with_probes(R, qn, 11)
    _check(xs, qn, "many")


def test_prefilter_entry_points_refuse_bad_arguments():
    """R % 32 != 0, D % 128 != 0, ldQ < Q, band < 0, a row image one byte too small: each raises and writes nothing."""
    import torch
    from qpgesture_amd import _lib
    qn = P.queries(5, 128, 3)
    xs, _ = P.rows_mixed(64, qn, 3)
    im = _Images(xs, qn)
    o = _Outputs(im)
    t, dev, R, Q, D = o.t, im.dev, im.R, im.Q, im.D
    rows_before = im.rows.clone()
    calls = {
        "distance R % 32": ("qpg_hl_gemm_distance", im.rows, 48, D, im.cols, Q, t["Dm"], o.ldD, t["tmin_d"], o.ldT),
        "tilemin R % 32": ("qpg_hl_gemm_tilemin", im.rows, 48, D, im.cols, Q, 1e-4, t["tmin_m"], t["mask_m"], o.ldT),
        "tilemin_h R % 32": ("qpg_hl_gemm_tilemin_h", im.rows, 48, D, im.cols, Q, 1e-3, t["tmin_h"], t["mask_h"], o.ldQ),
        "pack_rows R % 32": ("qpg_hl_pack_rows", im.xs_t, 48, D, im.rows, im.rows.numel()),
        "distance D % 128": ("qpg_hl_gemm_distance", im.rows, R, 64, im.cols, Q, t["Dm"], o.ldD, t["tmin_d"], o.ldT),
        "tilemin D % 128": ("qpg_hl_gemm_tilemin", im.rows, R, 64, im.cols, Q, 1e-4, t["tmin_m"], t["mask_m"], o.ldT),
        "tilemin_h D % 128": ("qpg_hl_gemm_tilemin_h", im.rows, R, 64, im.cols, Q, 1e-3, t["tmin_h"], t["mask_h"], o.ldQ),
        "pack_rows D % 128": ("qpg_hl_pack_rows", im.xs_t, R, 64, im.rows, im.rows.numel()),
        "pack_cols D % 128": ("qpg_hl_pack_cols", im.qn_t, Q, 64, im.cols, im.cols.numel()),
        "tilemin_h ldQ < Q": ("qpg_hl_gemm_tilemin_h", im.rows, R, D, im.cols, Q, 1e-3, t["tmin_h"], t["mask_h"], Q - 1),
        "tilemin band < 0": ("qpg_hl_gemm_tilemin", im.rows, R, D, im.cols, Q, -1e-6, t["tmin_m"], t["mask_m"], o.ldT),
        "tilemin_h band < 0": ("qpg_hl_gemm_tilemin_h", im.rows, R, D, im.cols, Q, -1e-6, t["tmin_h"], t["mask_h"], o.ldQ),
        "pack_rows image too small": ("qpg_hl_pack_rows", im.xs_t, R, D, im.rows, im.rows.numel() - 1),
    }
    cols_before = im.cols.clone()
    accepted = []
    for what, (name, *args) in calls.items():
        try:
            _lib.call(name, dev, *args)
        except RuntimeError:
            continue
        accepted.append(what)
    assert not accepted, "accepted: %s" % accepted
    got = o.fetch()
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(o.before[k])), "%s touched by a refused call" % k
    assert torch.equal(im.rows, rows_before) and torch.equal(im.cols, cols_before)
