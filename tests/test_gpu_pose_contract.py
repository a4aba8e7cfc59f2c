"""qpg_pose_to_euler_f64 (csrc/qpg_pose.hip) at its edges, through the C ABI, against tests/pose_ref.py (NumPy f64: polar
factor by SVD, closed-form Z-X-Y angles; pinned to scipy by tests/test_pose_ref_cpu.py).

Bars: angles within 1e-9 degrees away from gimbal lock (|b| <= 89 degrees) - the f64 roundoff of the polar factor, about
2e-16 / sigma_min, times 1 / cos b <= 57 and 57.3 degrees per radian is about 1e-11; next to the lock (|sin b| =
1 - 1e-10) the rotation rebuilt from the returned angles within 1e-12 per entry of the polar factor."""
import numpy as np
import pytest
import torch

from qpgesture_amd import _lib, bvh
from tests import pose_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.0


def call(poses32, mean, std, tables=None, W=15):
    """(euler (T, 3 J), status) of one call; one spare output row must keep its sentinel."""
    T, C = poses32.shape
    J = C // 9
    p = torch.from_numpy(np.ascontiguousarray(poses32, np.float32)).to(DEV)
    m, s = (torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV) for a in (mean, std))
    tabs = [None] * 3 if tables is None else [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in tables]
    out = torch.full((T + 1, 3 * J), SENT, dtype=torch.float64, device=DEV)
    status = torch.zeros((1,), dtype=torch.int32, device=DEV)
    _lib.call("qpg_pose_to_euler_f64", DEV, p, T, J, m, s, tabs[0], tabs[1], tabs[2], W, out, status)
    torch.cuda.synchronize()
    assert bool((out[T] == SENT).all())
    return out[:T].cpu().numpy(), int(status.item())


def from_f64(mats):
    """(J, 3, 3) f64 matrices handed over exactly: poses 0, std 1, mean = the matrices (two frames)."""
    J = mats.shape[0]
    return np.zeros((2, 9 * J), np.float32), mats.reshape(9 * J), np.ones(9 * J)


@pytest.mark.parametrize("T,J", [(37, 15), (300, 1)])
def test_strongly_non_orthogonal_inputs(T, J):
    """Noise of up to 0.3 per entry on every matrix: the Newton polar iteration from far away; T J = 555 and 300 threads
    (three and two blocks, the last partly empty)."""
    p, mean, std = R.noisy_rotations(3 + J, T, J)
    got, status = call(p, mean, std)
    want, _ = R.pose_to_euler(p, mean, std)
    free = np.repeat(np.abs(want[:, 1::3]) <= 89.0, 3, axis=1)
    err = R.wrap_diff(got, want)
    print("POSECONTRACT noisy T=%d J=%d: max err %.3g deg over %d angles" % (T, J, err[free].max(), free.sum()))
    assert status == 0 and free.mean() > 0.9 and err[free].max() <= 1e-9
    assert np.abs(got[:, 1::3]).max() <= 90.0 and np.abs(got).max() <= 180.0


def _lock_cases():
    a = np.array([10.0, -75.0, 130.0, -160.0, 0.0, 45.0, 179.0, -20.0])
    c = np.array([25.0, 40.0, -100.0, 170.0, 33.0, -45.0, 5.0, -0.5])
    sb = np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0])
    return a, c, sb


def test_exact_gimbal_lock_in_f64():
    """b = +-90 degrees exactly (sin b = +-1, cos b = 0, c != 0): the third angle is 0, the first a + c (a - c)."""
    a, c, sb = _lock_cases()
    got, status = call(*from_f64(R.rot_zxy(a, 0.0, c, sb=sb, cb=0.0)))
    e = got.reshape(2, -1, 3)
    assert status == 0 and np.all(e[:, :, 2] == 0.0) and np.abs(e[:, :, 1] - 90.0 * sb).max() <= 1e-9
    err = R.wrap_diff(e[:, :, 0], a + sb * c).max()
    print("POSECONTRACT lock f64: first angle within %.3g deg of a +- c" % err)
    assert err <= 1e-9


def test_exact_gimbal_lock_rounded_to_f32():
    """The same matrices as f32 input (0 and +-1 stay exact, the 2x2 block is rounded): still the lock branch; the first
    angle is the polar factor's, and a + c (a - c) to f32 rounding."""
    a, c, sb = _lock_cases()
    p = R.rot_zxy(a, 0.0, c, sb=sb, cb=0.0).reshape(1, -1).astype(np.float32)
    mean, std = np.zeros(p.shape[1]), np.ones(p.shape[1])
    got, status = call(p, mean, std)
    want, _ = R.pose_to_euler(p, mean, std)
    e = got.reshape(-1, 3)
    assert status == 0 and np.all(e[:, 2] == 0.0) and np.abs(e[:, 1] - 90.0 * sb).max() <= 1e-9
    err = R.wrap_diff(e[:, 0], want.reshape(-1, 3)[:, 0]).max()
    print("POSECONTRACT lock f32: first angle within %.3g deg of the polar factor's, %.3g of a +- c"
          % (err, R.wrap_diff(e[:, 0], a + sb * c).max()))
    assert err <= 1e-9 and R.wrap_diff(e[:, 0], a + sb * c).max() <= 1e-5


def test_just_outside_the_lock_branch():
    """|sin b| = 1 - 1e-10 (cos b = 1.4e-5): a and c are separately defined but ill-conditioned, so the ROTATION rebuilt
    from the returned angles is compared with the polar factor, 1e-12 per entry."""
    a, c, sgn = _lock_cases()
    sb = sgn * (1.0 - 1e-10)
    cb = np.sqrt((1.0 - sb) * (1.0 + sb))
    mats = R.rot_zxy(a, 0.0, c, sb=sb, cb=cb)
    got, status = call(*from_f64(mats))
    e = got.reshape(2, -1, 3)
    assert status == 0 and np.all(e[:, :, 2] != 0.0) and np.all(np.abs(e[:, :, 1]) < 90.0)
    rebuilt = R.rot_zxy(e[..., 0], e[..., 1], e[..., 2])
    err = np.abs(rebuilt - R.polar(mats)[None]).max()
    print("POSECONTRACT near lock: rebuilt rotation within %.3g per entry of the polar factor" % err)
    assert err <= 1e-12


def test_bad_determinants_raise_status_and_leave_neighbours_alone():
    """A reflection and an exactly singular matrix (joint 0 is handed over without arithmetic: mean 0, std 1): status 1,
    their three angles 0, every other angle bit for bit what a call without them gives."""
    p, mean, std = R.noisy_rotations(77, 3, 5, noise=0.1)
    mean[:9], std[:9] = 0.0, 1.0
    p[:, :9] = R.rot_zxy(20.0, 30.0, 40.0).reshape(9)
    good, status = call(p, mean, std)
    want, _ = R.pose_to_euler(p, mean, std)
    assert status == 0 and R.wrap_diff(good, want).max() <= 1e-9
    bad = p.copy()
    m = R.denormalise(p, mean, std).reshape(3, 5, 3, 3)
    bad[1, 18:27] = (((m[1, 2] @ np.diag([1.0, 1.0, -1.0])).reshape(9) - mean[18:27]) / std[18:27]).astype(np.float32)
    bad[2, :9] = [1.0, 2.0, 3.0, 0.5, -1.0, 0.25, 2.5, 3.0, 6.25]            # row 2 = 2 row 0 + row 1: det is exactly 0
    seen = R.denormalise(bad, mean, std).reshape(3, 5, 3, 3)
    assert np.linalg.det(seen[1, 2]) < -0.5 and abs(np.linalg.det(seen[2, 0])) < 1e-12
    got, status = call(bad, mean, std)
    e, g = got.reshape(3, 5, 3), good.reshape(3, 5, 3)
    assert status == 1 and np.all(e[1, 2] == 0.0) and np.all(e[2, 0] == 0.0)
    keep = np.ones((3, 5), bool)
    keep[1, 2] = keep[2, 0] = False
    assert np.array_equal(e[keep], g[keep])


@pytest.mark.parametrize("W", [3, 15])
def test_smoothing_head_middle_and_tail(W):
    """T = W (no interior frame but the middle one), W + 1 and 2 W: every head and tail row, against bvh.savgol_tables
    applied in NumPy."""
    tables = bvh.savgol_tables(W, 2)
    for T in (W, W + 1, 2 * W):
        p, mean, std = R.smooth_rotations(10 * W + T, T, 2)
        got, status = call(p, mean, std, tables, W)
        want, _ = R.pose_to_euler(p, mean, std, tables)
        plain, _ = R.pose_to_euler(p, mean, std)
        free = np.repeat(np.abs(want[:, 1::3]) <= 89.0, 3, axis=1)
        err = R.wrap_diff(got, want)
        print("POSECONTRACT smoothing W=%d T=%d: max err %.3g deg" % (W, T, err[free].max()))
        assert status == 0 and free.all() and err.max() <= 1e-9
        if W > 3:                                                            # (a parabola through 3 points is the points)
            assert R.wrap_diff(want, plain).max() > 1e-3                     # the smoothing does something


def test_smoothing_refusals():
    p, mean, std = R.smooth_rotations(1, 16, 2)
    with pytest.raises(RuntimeError, match="odd window"):
        call(p, mean, std, bvh.savgol_tables(15, 2), 14)                     # an even W
    with pytest.raises(RuntimeError, match="odd window"):
        call(p[:14], mean, std, bvh.savgol_tables(15, 2), 15)                # T < W
