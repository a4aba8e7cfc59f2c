"""Every audio sweep against NumPy f64 (tests/audio_ref.py), called directly: qpg_audio_pack_queries, qpg_frame_norm2_f64,
qpg_audio_cand_norm2, qpg_audio_cosine_f64 / _f64_h / _mx / _mx_h, and qpg_audio_hl_pack_db / _hl1_pack_db /
_hl_pack_queries followed by qpg_audio_cosine_hl / _hl1.  The referee is NumPy, never a kernel: the distances AND the
norms the device computes are compared with audio_ref's; the sweeps are then fed the device's own candidate norms, as in
the product.

What the cases are chosen for (none of it runs at the workload's T = 180, G = 26, cand_t = 6 g, tap_stride = 2):
  * candidate-side padding: taps at or past T, on a cand_t that is no arithmetic progression, tap_stride 1, 2 and 3, a
    grid whose only live tap is tap 0, hl grids that end inside the last super-rows;
  * the track is a 16-byte-aligned view into a larger buffer with 16 F NaN values on either side and the outputs are
    NaN-filled matrices with ldD = C + 8 and a guard row: a padding guard that lets a tap run on, a tile that is not
    written or a store outside [0:Q][0:C] fails an assertion - nothing here can fault;
  * every organisation of qpg_audio_cosine_mx (`mx_plan` restates audio_cosine_mx's arithmetic; the cases that need a
    device of 256 CUs say so), every query-tile shape of the split-K kernels, ragged candidate and query tiles, F = 128
    and, where a second trip of a k loop matters, 256;
  * inputs whose roundings do not average out (audio_ref.family).

Bars (audio_ref / the project's own constants; none is tuned to what the kernels return):
  grid family   norms bit for bit; every f64 matrix within 2^-48 of the reference (the dot is exact; two square roots, a
                multiply, a divide and a subtract on numbers <= 2: < 6e-16, the hl epilogue's fast_rsqrt_f64 adds 2 x 1e-15)
  all families  an f32-stored matrix is the kernel's f64 matrix rounded once; zero rows and zero queries are exact
  others        f64 sweeps (2 K + 16) 2^-53, K = 6 F; mx / mx_h AUDIO_MX_ERR; hl / hl1 AUDIO_HL_ERR - on every pair the
                kernel's own guard does not flag; f16-base forms are judged on the f16-rounded track
  flags         stats[1] & 2 exactly when audio_ref's predicate marks a pair; stats[1] == 0 otherwise
One AUDIOCONTRACT line per entry point, family and case: worst error over its bar (pytest -s)."""
import numpy as np
import pytest

from tests import audio_ref as R

pytestmark = pytest.mark.gpu

SLACK_FRAMES = 16                    # NaN frames in front of and behind the track (the longest overrun a grid here could make: 15)
GRID_EXACT = 2.0 ** -48
T_A, CAND_A = 23, (0, 7, 3, 12, 14)  # stride 2: candidate 14's last tap is padded; stride 3: the last taps of 12 and 14


def _cand_t(G, T=T_A):
    """G start frames in [0, T): CAND_A, [T - 1] (only tap 0 is live), or a seeded draw with repeats that is no progression."""
    if G == 5:
        return np.array(CAND_A, np.int32)
    if G == 1:
        return np.array([T - 1], np.int32)
    t = np.random.default_rng(G).integers(0, T, size=G).astype(np.int32)
    t[:3] = (T - 1, 0, T - 2)
    return t


# ---- device plumbing ---------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda:0")


def _track(base, half):
    """base [N][T][F] on the device as a 16-byte-aligned view into a NaN-filled buffer (f16 if half)."""
    import torch
    N, T, F = base.shape
    slack = SLACK_FRAMES * F
    buf = torch.full((2 * slack + N * T * F,), float("nan"), dtype=torch.float16 if half else torch.float32, device=_dev())
    view = buf[slack:slack + N * T * F].view(N, T, F)
    view.copy_(torch.from_numpy(base.astype(np.float16) if half else base))
    assert view.data_ptr() % 16 == 0 and view.is_contiguous() and bool(torch.isnan(buf[:slack]).all())
    return view, buf


def _nan_out(Q, C, f32):
    import torch
    return torch.full((Q + 1, C + 8), float("nan"), dtype=torch.float32 if f32 else torch.float64, device=_dev())


def _live(D, Q, C, what):
    """The live part of a NaN-prefilled output: every entry written (a NaN read from the slack around the track shows up
    here too), nothing outside [0:Q][0:C] touched (bitwise)."""
    import torch
    bits = torch.int32 if D.dtype == torch.float32 else torch.int64
    fresh = torch.full_like(D, float("nan"))
    probe = D.clone()
    probe[:Q, :C] = fresh[:Q, :C]
    assert torch.equal(probe.view(bits), fresh.view(bits)), what + ": wrote outside [0:Q][0:C]"
    live = D[:Q, :C].cpu().numpy()
    assert not np.isnan(live).any(), "%s: %d entries unwritten or NaN" % (what, int(np.isnan(live).sum()))
    return live


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _reference(c, half):
    """(track the kernels see as f32, cn2, qn2, D) in NumPy; half: everything on the f16-rounded track."""
    base = c.base.astype(np.float16).astype(np.float32) if half else c.base
    rows = R.stack(base, c.cand_t, c.n_taps, c.tap_stride)
    q = c.q32.astype(np.float64)
    cn2, qn2 = np.einsum("ck,ck->c", rows, rows), np.einsum("qk,qk->q", q, q)          # (= audio_ref.norms)
    return base, cn2, qn2, R.distance_from_dot(q @ rows.T, qn2, cn2)


def _device_norms(c, track32, cn2_ref, what):
    """qpg_frame_norm2_f64 + qpg_audio_cand_norm2 on the device track, held to NumPy: bit for bit on `grid`, else the f64
    sum's own gamma on both sides.  -> cn2 [dev]."""
    import torch
    from qpgesture_amd import _lib
    dev = _dev()
    N, T, F = track32.shape
    G = len(c.cand_t)
    fn2 = torch.full((N * T + 1,), float("nan"), dtype=torch.float64, device=dev)
    _lib.call("qpg_frame_norm2_f64", dev, track32, N * T, F, fn2)
    cn2 = torch.full((N * G + 1,), float("nan"), dtype=torch.float64, device=dev)
    _lib.call("qpg_audio_cand_norm2", dev, fn2, N, T, torch.from_numpy(c.cand_t).to(dev), G, c.n_taps, c.tap_stride, cn2)
    torch.cuda.synchronize()
    fn2_h, cn2_h = fn2.cpu().numpy(), cn2.cpu().numpy()
    assert np.isnan(fn2_h[-1]) and np.isnan(cn2_h[-1]), what + ": a norm kernel wrote past its output"
    fn2_ref = R.frame_norm2(track32.cpu().numpy()).reshape(-1)
    if c.name == "grid":
        assert np.array_equal(fn2_h[:-1], fn2_ref) and np.array_equal(cn2_h[:-1], cn2_ref), what + ": norms not exact"
    else:
        assert (np.abs(fn2_h[:-1] - fn2_ref) <= 2 * F * R.U64 * fn2_ref).all(), what
        assert (np.abs(cn2_h[:-1] - cn2_ref) <= 2 * c.n_taps * F * R.U64 * cn2_ref).all(), what
    assert np.array_equal(cn2_h[:-1] == 0, cn2_ref == 0)
    return cn2[:-1]


def _judge(entry, c, label, D, D32, ref, bar, flagged, qn2, cn2):
    """The bars of one entry point on one input; D: its f64 matrix, D32: its f32-stored matrix (or None)."""
    ok = ~flagged
    if c.name == "grid":
        bar = GRID_EXACT
    err = np.abs(D - ref)
    worst = float(err[ok].max())
    worst32 = float(np.abs(D32.astype(np.float64) - ref)[ok].max()) if D32 is not None else 0.0
    line = "AUDIOCONTRACT %-24s %-9s %-28s worst/bar %.3g (f64 matrix %.3g%s, bar %.3g)%s" % (
        entry, c.name, label, max(worst, 0.0 if c.name == "grid" else worst32) / bar, worst,
        ", f32 matrix %.3g" % worst32 if D32 is not None else "", bar,
        "; %d flagged pairs not judged, worst there %.3g" % (int(flagged.sum()), float(err[flagged].max())) if flagged.any() else "")
    print(line)
    assert worst <= bar, line
    if D32 is not None:
        assert np.array_equal(D32, D.astype(np.float32)), entry + ": the f32 matrix is not the f64 matrix rounded once"
        if c.name != "grid":
            assert worst32 <= bar, line
    zq, zc = qn2 == 0, cn2 == 0
    for M, want in ((D, ref),) + (((D32, ref.astype(np.float32)),) if D32 is not None else ()):
        assert np.array_equal(M[zq], want[zq]) and np.array_equal(M[:, zc], want[:, zc]), entry + ": zero rows / queries not exact"


# ---- qpg_audio_cosine_f64 / _f64_h / _mx / _mx_h ------------------------------------------------------------------------
def mx_plan(Q, C, n_cu):
    """audio_cosine_mx's work split (csrc/qpg_audio.hip), restated: which organisation a call takes."""
    ny, nbx = (Q + 47) // 48, C // 64
    main_x = nbx if ny >= 4 else (nbx * ny // n_cu) * n_cu // ny
    c_mid = main_x * 64
    tail = (C - c_mid + 15) // 16
    ride = main_x > 0 and 0 < tail <= 4 * n_cu and ny == 1
    qt = (Q + 15) // 16
    nt = 3 if qt % 3 == 0 else 4 if qt % 4 == 0 else 2 if qt % 2 == 0 else 1
    big = "ny>=4" if ny >= 4 else "ny<4"
    if main_x > 0 and c_mid == C:
        return "mx2 alone (%s)" % big
    if ride:
        return "mx2 + riding tail (ny=1)"
    mt = 1 if tail * ny <= 4 * n_cu else 2
    if main_x > 0:
        return "mx2 (%s) + split-K<%d> tail NT=%d" % (big, mt, nt) if ny >= 4 else "mx2 (ny<4) + split-K<%d> tail, c_begin != 0" % mt
    return "split-K<%d> NT=%d" % (mt, nt)


# id: (N, G, tap_stride, Q, F, families).  C = N G.  The comments name the organisation on a device of 256 CUs.
MX_CASES = {
    "c65_q48_s2": (13, 5, 2, 48, 128, R.FAMILIES),                                         # split-K<1> NT=3, ragged candidate tile
    "c65_q64_s3": (13, 5, 3, 64, 128, ("grid", "dense", "zeros", "samesign", "neardup")),   # NT=4, two padded taps
    "c65_q32_s2_f256": (13, 5, 2, 32, 256, ("grid", "dense", "samesign", "cancel")),  # NT=2, two trips (rot = bx % 2)
    "c65_q16_s1": (13, 5, 1, 16, 128, ("grid", "dense", "spiky")),                   # NT=1, tap_stride 1 (no padding)
    "c64_q5_last": (64, 1, 2, 5, 128, ("grid", "dense", "zeros")),                   # cand_t = [T-1]: only tap 0 is live
    "c65_q80_s3": (13, 5, 3, 80, 128, ("grid", "dense", "tiny")),                    # NT=1 x 5 query tiles
    "c64_q145_last": (64, 1, 2, 145, 128, ("grid", "dense", "samesign", "tiny")),    # mx2 alone, ny = 4
    "c64_q200_last": (64, 1, 3, 200, 128, ("grid", "dense")),                        # mx2 alone, ny = 5, ragged query tile
    "c65_q145_s3": (13, 5, 3, 145, 128, ("grid", "dense", "zeros")),                 # mx2 + split-K<1> tail NT=2
    "c65_q200_s2": (13, 5, 2, 200, 128, ("grid", "dense", "zeros", "tiny", "cancel")),   # mx2 + split-K<1> tail NT=1
    "c130_q145_s2_f256": (26, 5, 2, 145, 256, ("grid", "dense", "samesign", "spiky")),   # two mx2 blocks + tail, 4 k groups
    "c130_q200_s3": (26, 5, 3, 200, 128, ("grid", "dense", "neardup")),
    "c16406_q48": (631, 26, 2, 48, 128, ("grid", "dense", "samesign", "tiny", "zeros")),  # 256 CUs: mx2 + riding tail
    "c8216_q96": (316, 26, 3, 96, 128, ("grid", "dense", "samesign", "tiny")),            # 256 CUs: mx2 + tail from c_begin = 8192
    "c8192_q80": (256, 32, 2, 80, 128, ("grid", "dense", "samesign")),                    # 256 CUs: c_mid == C at ny = 2
    "c5500_q144": (220, 25, 2, 144, 128, ("grid", "dense", "tiny", "zeros")),             # 256 CUs: launch_audio_mx_q<2>
}
WANT_256 = {"split-K<1> NT=1", "split-K<1> NT=2", "split-K<1> NT=3", "split-K<1> NT=4", "mx2 alone (ny>=4)",
            "mx2 (ny>=4) + split-K<1> tail NT=1", "mx2 (ny>=4) + split-K<1> tail NT=2", "mx2 + riding tail (ny=1)",
            "mx2 (ny<4) + split-K<1> tail, c_begin != 0", "mx2 alone (ny<4)", "split-K<2> NT=3"}


def _mx_params():
    return [pytest.param(cid, fam, id="%s-%s" % (cid, fam)) for cid, v in MX_CASES.items() for fam in v[5]]


def _run_f64_and_mx(c, half):
    """One input through the f64 and the mixed sweep (f64 and f32 matrix) on the f32 or the f16 track."""
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.code_knn import AUDIO_MX_ERR
    dev = _dev()
    N, T, F = c.base.shape
    G, Q = len(c.cand_t), c.q32.shape[0]
    C = N * G
    base, cn2_ref, qn2_ref, ref = _reference(c, half)
    track, _keep = _track(base, half)
    sfx = "_h" if half else ""
    label = "N=%d G=%d s=%d Q=%d F=%d" % (N, G, c.tap_stride, Q, F)
    cn2 = _device_norms(c, track.float() if half else track, cn2_ref, "norms" + sfx + " " + label)
    cand_t = torch.from_numpy(c.cand_t).to(dev)
    q32 = torch.from_numpy(c.q32).to(dev)
    qn2 = torch.from_numpy(qn2_ref).to(dev)
    grid = (cand_t, G, c.n_taps, c.tap_stride, cn2, q32, qn2, Q)
    D64 = _nan_out(Q, C, False)
    _lib.call("qpg_audio_cosine_f64" + sfx, dev, track, N, T, F, *grid, D64, D64.stride(0))
    stats = torch.zeros((4,), dtype=torch.int32, device=dev)
    Dmx, Dmx32 = _nan_out(Q, C, False), _nan_out(Q, C, True)
    _lib.call("qpg_audio_cosine_mx" + sfx, dev, track, N, T, F, *grid, Dmx, 0, Dmx.stride(0), stats)
    stats32 = torch.zeros((4,), dtype=torch.int32, device=dev)
    _lib.call("qpg_audio_cosine_mx" + sfx, dev, track, N, T, F, *grid, Dmx32, 1, Dmx32.stride(0), stats32)
    torch.cuda.synchronize()
    none = np.zeros(ref.shape, bool)
    flagged = R.mx_guard(qn2_ref, cn2_ref)
    _judge("qpg_audio_cosine_f64" + sfx, c, label, _live(D64, Q, C, "f64" + sfx), None, ref, R.f64_bar(F), none, qn2_ref, cn2_ref)
    _judge("qpg_audio_cosine_mx" + sfx, c, label, _live(Dmx, Q, C, "mx" + sfx), _live(Dmx32, Q, C, "mx" + sfx + " f32"), ref,
           AUDIO_MX_ERR, flagged, qn2_ref, cn2_ref)
    for st in (stats.cpu().numpy(), stats32.cpu().numpy()):
        assert bool(st[1] & 2) == bool(flagged.any()) and (st[1] & ~2) == 0, (sfx, st, int(flagged.sum()))
    assert bool(flagged.any()) == (c.name == "tiny")


@pytest.mark.parametrize("cid,fam", _mx_params())
def test_f64_and_mixed_sweeps_against_numpy(cid, fam):
    N, G, stride, Q, F, _ = MX_CASES[cid]
    print("%s: %s on %d CUs" % (cid, mx_plan(Q, N * G, _n_cu()), _n_cu()))
    c = R.family(fam, N, T_A, F, Q, (_cand_t(G), 6, stride))
    _run_f64_and_mx(c, half=False)
    _run_f64_and_mx(c, half=True)


def test_every_organisation_of_the_mixed_sweep_is_reached():
    """Which organisation each case took on this device (printed), and on a device of 256 CUs: all of them.
    launch_audio_mx_q<2> (split-K blocks of 32 candidates) needs main_x == 0 and more than 4 n_cu tail blocks: at 256 CUs
    that is ceil(C / 16) ny > 1024 with (C / 64) ny < 256 - C in 5457..5503 at ny = 3 and nothing at ny = 1, 2 - or
    ny >= 4 with ceil((C % 64) / 16) ny > 1024, i.e. Q > 12288: no workload of the matcher takes it."""
    n_cu = _n_cu()
    taken = {}
    for cid, (N, G, stride, Q, F, fams) in MX_CASES.items():
        taken.setdefault(mx_plan(Q, N * G, n_cu), []).append(cid)
    for org, cids in sorted(taken.items()):
        print("AUDIOCONTRACT organisation %-46s %s" % (org, " ".join(cids)))
    assert {mx_plan(Q, N * G, 256) for N, G, s, Q, F, f in MX_CASES.values()} == WANT_256      # the table itself
    if n_cu == 256:
        assert set(taken) == WANT_256
    # the window of launch_audio_mx_q<2> at 256 CUs, from the same arithmetic
    assert [C for C in range(1, 20000) if mx_plan(144, C, 256).startswith("split-K<2>")] == list(range(5457, 5504))
    assert not any(mx_plan(Q, C, 256).startswith("split-K<2>") for Q in (48, 96, 192, 12288) for C in range(1, 20000))


# ---- qpg_audio_pack_queries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["grid", "dense", "zeros", "spiky"])
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_query_pack_gathers_pads_and_norms(fam, stride):
    """q32 is a gather (bit for bit, padded taps zero, nothing read from behind the track); qn2 against NumPy."""
    import torch
    from qpgesture_amd import _lib
    dev = _dev()
    N, T, F, Q = 5, T_A, 128, 19
    c = R.family(fam, N, T, F, 1, (_cand_t(5), 6, stride))
    rng = np.random.default_rng(stride)
    q_win = rng.integers(0, N, size=Q).astype(np.int32)
    q_t = rng.integers(0, T, size=Q).astype(np.int32)
    q_win[:3], q_t[:3] = N - 1, (T - 1, T - 1 - 5 * stride, 0)      # the LAST window: only tap 0 live / just fits / all live
    want = np.stack([R.row32(c.base, int(w), int(t), 6, stride) for w, t in zip(q_win, q_t)])
    track, _keep = _track(c.base, False)
    q32 = torch.full((Q + 1, 6 * F), float("nan"), dtype=torch.float32, device=dev)
    qn2 = torch.full((Q + 1,), float("nan"), dtype=torch.float64, device=dev)
    _lib.call("qpg_audio_pack_queries", dev, track, N, T, F, torch.from_numpy(q_win).to(dev), torch.from_numpy(q_t).to(dev),
              Q, 6, stride, q32, qn2)
    torch.cuda.synchronize()
    got, n2 = q32.cpu().numpy(), qn2.cpu().numpy()
    assert np.isnan(got[Q]).all() and np.isnan(n2[Q])
    assert np.array_equal(got[:Q], want)
    n2_ref = np.einsum("qk,qk->q", want.astype(np.float64), want.astype(np.float64))
    if fam == "grid":
        assert np.array_equal(n2[:Q], n2_ref)
    else:
        assert (np.abs(n2[:Q] - n2_ref) <= 2 * 6 * F * R.U64 * n2_ref).all()


# ---- qpg_audio_hl_pack_db / _hl1_pack_db / _hl_pack_queries -> qpg_audio_cosine_hl / _hl1 ---------------------------------
HL_FAMILIES = tuple(f for f in R.FAMILIES if f != "tiny")        # (`tiny` is the f32 sweeps' guard; `quiet` is this one's)
# id: (N, T, tap_stride, Q, F, families): G = 26, candidates 3 x tap_stride apart; 8 windows per block, chunks of 48 queries
HL_CASES = {
    "t78_n9_q49": (9, 78, 1, 49, 128, HL_FAMILIES),                               # frames 78..80 of the last super-rows padded
    "t157_n17_q97": (17, 157, 2, 97, 128, ("grid", "dense", "zeros", "quiet", "spiky")),   # frames 157..160 padded
    "t180_n8_q48": (8, 180, 2, 48, 128, ("grid", "dense", "samesign", "quiet")),  # the workload's grid: no padding
    "t78_n1_q1": (1, 78, 1, 1, 128, ("grid", "dense")),
    "t78_n1_q97": (1, 78, 1, 97, 128, ("grid", "cancel")),
    "t157_n17_q1_f256": (17, 157, 2, 1, 256, ("grid", "dense", "samesign", "quiet")),      # a second trip of both k loops
    "t157_n8_q48_f256": (8, 157, 2, 48, 256, ("grid", "neardup")),
}


def _hl_params():
    return [pytest.param(cid, fam, id="%s-%s" % (cid, fam)) for cid, v in HL_CASES.items() for fam in v[5]]


def _run_hl(c, one_plane):
    import torch
    from qpgesture_amd import _lib
    from qpgesture_amd.code_knn import AUDIO_HL_ERR
    dev = _dev()
    lib = _lib.load()
    N, T, F = c.base.shape
    G, Q, s = len(c.cand_t), c.q32.shape[0], c.tap_stride
    C = N * G
    base, cn2_ref, qn2_ref, ref = _reference(c, one_plane)
    track, _keep = _track(base, one_plane)
    sfx = "hl1" if one_plane else "hl"
    label = "N=%d T=%d s=%d Q=%d F=%d" % (N, T, s, Q, F)
    cn2 = _device_norms(c, track.float() if one_plane else track, cn2_ref, "norms " + sfx + " " + label)
    assert (lib.qpg_audio_hl1_supported if one_plane else lib.qpg_audio_hl_supported)(T, F, G, 6, s, 3 * s)
    nbytes = int((lib.qpg_audio_hl1_db_bytes if one_plane else lib.qpg_audio_hl_db_bytes)(N, F))
    # images pre-filled with 0xFF (an f16 NaN in every slot): a piece a pack kernel leaves out turns into a NaN in D
    img = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device=dev)
    _lib.call("qpg_audio_hl1_pack_db" if one_plane else "qpg_audio_hl_pack_db", dev, track, N, T, F, G, 6, s, 3 * s, img, nbytes)
    qbytes = int(lib.qpg_audio_hl_query_bytes(Q, F))
    qi = torch.full((qbytes + 16,), 0xFF, dtype=torch.uint8, device=dev)
    q32 = torch.from_numpy(c.q32).to(dev)
    _lib.call("qpg_audio_hl_pack_queries", dev, q32, Q, F, qi, qbytes)
    qn2 = torch.from_numpy(qn2_ref).to(dev)
    entry = "qpg_audio_cosine_" + sfx
    D, D32 = _nan_out(Q, C, False), _nan_out(Q, C, True)
    st, st32 = (torch.zeros((4,), dtype=torch.int32, device=dev) for _ in range(2))
    _lib.call(entry, dev, img, N, F, G, cn2, qi, qn2, Q, D, 0, D.stride(0), st)
    _lib.call(entry, dev, img, N, F, G, cn2, qi, qn2, Q, D32, 1, D32.stride(0), st32)
    torch.cuda.synchronize()
    assert bool((img[nbytes:] == 0xFF).all()) and bool((qi[qbytes:] == 0xFF).all()), sfx + ": a pack kernel wrote past its image"
    flagged = np.zeros(ref.shape, bool) if one_plane else R.hl_guard(base, c.q32, qn2_ref, cn2_ref)
    _judge(entry, c, label, _live(D, Q, C, sfx), _live(D32, Q, C, sfx + " f32"), ref, AUDIO_HL_ERR, flagged, qn2_ref, cn2_ref)
    for stats in (st.cpu().numpy(), st32.cpu().numpy()):
        assert bool(stats[1] & 2) == bool(flagged.any()) and (stats[1] & ~2) == 0, (sfx, stats, int(flagged.sum()))
    assert bool(flagged.any()) == (c.name == "quiet" and not one_plane and N > 1)


@pytest.mark.parametrize("cid,fam", _hl_params())
def test_split_f16_sweeps_against_numpy(cid, fam):
    N, T, s, Q, F, _ = HL_CASES[cid]
    c = R.family(fam, N, T, F, Q, (np.arange(26, dtype=np.int32) * 3 * s, 6, s))
    _run_hl(c, one_plane=False)
    _run_hl(c, one_plane=True)
