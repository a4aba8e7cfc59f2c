"""csrc/qpg_pae.hip (qpg_pae_phase_f32) stage by stage against the f64 restatement of tests/pae_ref.py, through the C ABI.

Every call gets a NaN-filled workspace of exactly (n_frames + 239) * 136 floats followed by a NaN tail that must stay NaN,
and outputs filled with a sentinel with one spare row that must keep it.  Bounds, cases and the probe blocks are
pae_ref's; tests/test_pae_contract_cpu.py shows that each case's bound rejects the wrong tap limits, the missing position
240, a live window row 0, a shifted window and a velocity across a clip boundary.  Each test prints
`PAECONTRACT <case>: err/bound, err/e32, seconds` (profiles/pae_contract.md); err/e32 is recorded, not asserted."""
import time

import numpy as np
import pytest
import torch

from qpgesture_amd import PAE, _lib
from tests import pae_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.0
TAIL = 4096
U, ELEM = R.U, R.ELEM
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev_block(name):
    if ("P", name) not in _cache:
        _cache["P", name] = torch.from_numpy(np.array(R.block(name)[0])).to(DEV)
    return _cache["P", name]


def dev_input(inp):
    key = ("I", id(inp))
    if key not in _cache:
        _cache[key] = (inp, tuple(torch.from_numpy(np.ascontiguousarray(inp[k])).to(DEV) for k in ("pose", "mean", "std", "off")))
    return _cache[key][1]


def run(P, inp, frame0, n, extras=True):
    """One call: (out (n, 4, 8), v (n, 8, 2), latent (n, 8, 240), workspace (n + 239, 136)) as numpy; the guards asserted."""
    pose, mean, std, off = dev_input(inp)
    need = (n + 2 * PAE.HALO - 1) * PAE.WS_STRIDE
    ws = torch.full((need + TAIL,), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((n + 1, 4, R.E), SENT, dtype=torch.float32, device=DEV)
    v = torch.full((n + 1, R.E, 2), SENT, dtype=torch.float32, device=DEV) if extras else None
    lat = torch.full((n + 1, R.E, R.T), SENT, dtype=torch.float32, device=DEV) if extras else None
    _lib.call("qpg_pae_phase_f32", DEV, P, pose, mean, std, off, off.numel() - 1, pose.shape[0], frame0, n, ws, need, out, v,
              lat)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[need:]).all()), "the workspace's tail was written"
    for x in (out, v, lat):
        assert x is None or bool((x[n] == SENT).all()), "a row past n_frames was written"
    got = [None if x is None else x[:n].cpu().numpy() for x in (out, v, lat)]
    return got[0], got[1], got[2], ws[:need].cpu().numpy().reshape(-1, PAE.WS_STRIDE)


def run_frames(block_name, inp, frames):
    """The listed global frames, one call each (n_frames = 1), stacked; cached per (block, input)."""
    key = ("F", block_name, id(inp))
    if key not in _cache:
        P = dev_block(block_name)
        parts = [run(P, inp, g, 1)[:3] for g in frames]
        _cache[key] = tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    return _cache[key]


# ---- velocities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties", "white"])
def test_velocities_are_the_f64_difference_rounded_once(name):
    """The workspace after the call, bit for bit: f32(pn[G+1] - pn[G]) inside a clip, zero at a clip's last frame, before
    row 0, from the last pose row on and in column 135.  `ties`: means up to 1e3, stds at the 0.01 floor, steps at f32
    rounding ties, clip lengths 1, 5, 0, 130, 2, 300, 77 (boundaries inside every halo)."""
    t0 = time.time()
    inp = R.input_velocity_bits(17) if name == "ties" else R.inputs("white")
    n = int(inp["off"][-1])
    chunks = inp.get("chunks", [(0, n), (0, 1), (n - 1, 1), (1089, 1)])
    vel = R.velocities(inp)
    P = dev_block("seed11")
    live = 0
    for f0, nf in chunks:
        ws = run(P, inp, f0, nf)[3]
        want = R.workspace_image(vel, f0, nf)
        assert ws.shape == want.shape and not np.isnan(ws).any()
        bad = np.argwhere(_bits(ws) != _bits(want))
        assert bad.size == 0, "chunk (%d, %d): %d entries differ, first at row %d channel %d" % (f0, nf, len(bad), *bad[0])
        assert not ws[:, R.C].any()
        live += int((want != 0).sum())
    print("PAECONTRACT velocities %s: %d chunks, %d live entries bit-identical, err/bound 0, err/e32 0, %.1f s"
          % (name, len(chunks), live, time.time() - t0))


# ---- conv1 and conv2, each behind a selector --------------------------------------------------------------------------
@pytest.mark.parametrize("blk,inp", R.CONV1_CASES + R.CONV2_CASES, ids=["%s-%s" % c for c in R.CONV1_CASES + R.CONV2_CASES])
def test_convolution_stage_within_its_bound(blk, inp):
    t0 = time.time()
    P, Pd, I, ref = R.case(blk, inp)
    lat = run_frames(blk, I, I["frames"])[2]
    assert np.isfinite(lat).all()
    bound = R.latent_bound(blk, Pd, ref)
    r = R.ratio(lat, ref["latent"], bound)
    e32 = R.e32_ratio(lat, ref["latent"], R.stages(Pd, ref["win"], torch.float32)["latent"])
    print("PAECONTRACT %s/%s: %d frames, err/bound %.3f, err/e32 %.2f, %.1f s" % (blk, inp, len(I["frames"]), r, e32,
                                                                                 time.time() - t0))
    assert r <= 1.0, "%s/%s: |device - f64| is %.3f of its bound" % (blk, inp, r)


# ---- DFT, fc, atan2' on the device's own latent -------------------------------------------------------------------------
@pytest.mark.parametrize("blk,inp", R.HEAD_CASES, ids=["%s-%s" % c for c in R.HEAD_CASES])
def test_dft_fc_atan_from_the_devices_latent(blk, inp):
    t0 = time.time()
    P, Pd, I, ref = R.case(blk, inp)
    out, v, lat = run_frames(blk, I, I["frames"])
    assert np.isfinite(out).all() and np.isfinite(v).all() and np.isfinite(lat).all()
    H = R.head(Pd, lat)
    assert H["ac"].min() >= 1e-8
    H32 = R.head(Pd, lat, np.float32)
    tpi = float(Pd["tpi"])
    p_ref = R.atan2p(v, tpi)
    stages = [("f", out[:, 1], H["f"], np.abs(H["f"]), H32["f"]), ("a", out[:, 2], H["a"], np.abs(H["a"]), H32["a"]),
              ("b", out[:, 3], H["b"], np.abs(lat.astype(np.float64)).mean(2), H32["b"]),
              ("v", v, H["v"], H["vmag"], H32["v"]),
              ("p", out[:, 0], p_ref, (np.abs(p_ref) * tpi + np.pi) / tpi, R.atan2p(v, tpi).astype(np.float32))]
    worst = 0.0
    for name, got, want, mag, w32 in stages:
        r = R.ratio(got, want, ELEM * mag)
        e32 = R.e32_ratio(got, want, w32.astype(np.float64))
        print("PAECONTRACT %s/%s %s: err/bound %.3f, err/e32 %.2f" % (blk, inp, name, r, e32))
        worst = max(worst, r)
    print("PAECONTRACT %s/%s head: err/bound %.3f, %.1f s" % (blk, inp, worst, time.time() - t0))
    assert worst <= 1.0


def test_atan_pair_table():
    """fc = 0: v must be the table's pair bit for bit (the signs of the zeros included) at every frame; p the table's
    value - NaN at (0, 0) and nowhere else, and in p only; exactly + 1/2 at (-, +0.0) and at (-, -0.0)."""
    t0 = time.time()
    I = R.inputs("short")
    n = int(I["off"][-1])
    worst = 0.0
    for b in (0, 1):
        out, v, lat = run(dev_block("atan%d" % b), I, 0, n)[:3]
        pairs, want = R.ATAN_PAIRS[8 * b:8 * b + 8], R.ATAN_P[8 * b:8 * b + 8]
        assert np.array_equal(_bits(v), np.broadcast_to(_bits(pairs), v.shape))
        assert np.isfinite(out[:, 1:]).all() and np.isfinite(lat).all()
        assert np.array_equal(np.isnan(out[:, 0]), np.broadcast_to(np.isnan(want), (n, 8)))
        ok = ~np.isnan(want)
        worst = max(worst, R.ratio(out[:, 0][:, ok], np.broadcast_to(want[ok], (n, ok.sum())),
                                   ELEM * (np.abs(want[ok]) * R.TPI32 + np.pi) / R.TPI32))
        for e in range(8):
            if pairs[e][0] < 0 and pairs[e][1] == 0:
                assert np.all(out[:, 0, e] == 0.5), pairs[e]
    print("PAECONTRACT atan pairs: %d frames x 16 pairs, err/bound %.3f, err/e32 n/a, %.1f s" % (n, worst, time.time() - t0))
    assert worst <= 1.0


# ---- grouping -------------------------------------------------------------------------------------------------------
def test_grouping_is_bit_identical_and_stays_inside_its_rows():
    """The white frames computed one per call equal a contiguous run over all eleven clips (the empty one included);
    a call without v_out / latent_out equals one with them.  (run() asserts the spare rows and the workspace tail.)"""
    t0 = time.time()
    P, Pd, I, ref = R.case("seed11", "white")
    n = int(I["off"][-1])
    single = run_frames("seed11", I, I["frames"])
    whole = run(dev_block("seed11"), I, 0, n)
    for a, b in zip(single, whole[:3]):
        assert np.array_equal(_bits(a), _bits(b[I["frames"]]))
    bare = run(dev_block("seed11"), I, 0, n, extras=False)
    assert bare[1] is None and np.array_equal(_bits(bare[0]), _bits(whole[0]))
    part = run(dev_block("seed11"), I, 1000, 300)                           # across the empty clip at 1089
    assert np.array_equal(_bits(part[0]), _bits(whole[0][1000:1300])) and np.array_equal(_bits(part[2]), _bits(whole[2][1000:1300]))
    print("PAECONTRACT grouping: %d frames one per call = one run of %d, err/bound 0, err/e32 0, %.1f s"
          % (len(I["frames"]), n, time.time() - t0))
