"""tests/pose_ref.py without a GPU: the NumPy reference against scipy's Rotation.from_matrix(..).as_euler('ZXY') (where
scipy imports) and against its own closed form, and the conditions of the cases tests/test_gpu_pose_contract.py runs."""
import numpy as np
import pytest

from tests import pose_ref as R


@pytest.mark.parametrize("T,J", [(37, 15), (300, 1)])
def test_noisy_inputs_are_well_conditioned(T, J):
    p, mean, std = R.noisy_rotations(3 + J, T, J)
    m = R.denormalise(p, mean, std).reshape(T, J, 3, 3)
    s = np.linalg.svd(m, compute_uv=False)
    assert (T * J) % 256 and s[..., 2].min() >= 0.5 and np.linalg.det(m).min() > 0
    assert np.abs(m - R.polar(m)).max() > 0.2                                # strongly non-orthogonal
    e, r = R.pose_to_euler(p, mean, std)
    assert (np.abs(e[:, 1::3]) <= 89.0).mean() > 0.9
    print("POSECONDITION T=%d J=%d: sigma_min %.3f, max |m - polar| %.3f" % (T, J, s[..., 2].min(), np.abs(m - R.polar(m)).max()))


def test_reference_matches_scipy():
    Rot = pytest.importorskip("scipy.spatial.transform").Rotation
    p, mean, std = R.noisy_rotations(18, 37, 15)
    e, r = R.pose_to_euler(p, mean, std)
    m = R.denormalise(p, mean, std).reshape(-1, 3, 3)
    want = Rot.from_matrix(m).as_euler("ZXY", degrees=True).reshape(e.shape)
    free = np.repeat(np.abs(e[:, 1::3]) <= 89.0, 3, axis=1)
    assert free.mean() > 0.9 and R.wrap_diff(e, want)[free].max() < 1e-9


def test_closed_form_round_trips():
    rng = np.random.Generator(np.random.PCG64(5))
    a, b, c = rng.uniform(-180, 180, 500), rng.uniform(-89, 89, 500), rng.uniform(-180, 180, 500)
    e = R.euler_zxy(R.rot_zxy(a, b, c))
    assert R.wrap_diff(e, np.stack([a, b, c], -1)).max() < 1e-9
    # exact lock: the first angle is a + c at b = +90 and a - c at b = -90, the third 0
    for sb, sign in ((1.0, 1.0), (-1.0, -1.0)):
        e = R.euler_zxy(R.rot_zxy(a, 0.0, c, sb=sb, cb=0.0))
        assert np.all(e[:, 2] == 0) and np.all(e[:, 1] == 90.0 * sign) and R.wrap_diff(e[:, 0], a + sign * c).max() < 1e-9


def test_smoothing_matches_scipy():
    sg = pytest.importorskip("scipy.signal")
    from qpgesture_amd import bvh
    rng = np.random.Generator(np.random.PCG64(6))
    for W in (3, 15):
        for T in (W, W + 1, 2 * W):
            x = rng.standard_normal((T, 4))
            assert np.abs(R.smooth(x, bvh.savgol_tables(W, 2)) - sg.savgol_filter(x, W, 2, axis=0, mode="interp")).max() < 1e-12
