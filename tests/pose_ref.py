"""NumPy f64 reference of qpg_pose_to_euler_f64 (include/qpg.h): de-normalise, optional Savitzky-Golay smoothing, the
orthogonal polar factor U V^T of each 3x3 by np.linalg.svd (what scipy's Rotation.from_matrix takes), and the closed form
of R = Rz(a) Rx(b) Ry(c) for the intrinsic Z-X-Y angles in degrees.  tests/test_pose_ref_cpu.py pins it to scipy."""
import numpy as np

LOCK = 1.0 - 1e-14                    # |sin b| from here on is gimbal lock: the third angle is 0, like scipy


def polar(m):
    """(.., 3, 3) -> the orthogonal polar factor U V^T."""
    u, _, vt = np.linalg.svd(m)
    return u @ vt


def euler_zxy(r):
    """(.., 3, 3) rotations -> (.., 3) degrees (a, b, c) of Rz(a) Rx(b) Ry(c): R21 = sin b, R01 = -sin a cos b,
    R11 = cos a cos b, R20 = -cos b sin c, R22 = cos b cos c, b = atan2(R21, |(R20, R22)|); at lock a = atan2(R10, R00) (= a + c or a - c), c = 0."""
    sb = np.clip(r[..., 2, 1], -1.0, 1.0)
    lock = np.abs(sb) >= LOCK
    a = np.where(lock, np.arctan2(r[..., 1, 0], r[..., 0, 0]), np.arctan2(-r[..., 0, 1], r[..., 1, 1]))
    c = np.where(lock, 0.0, np.arctan2(-r[..., 2, 0], r[..., 2, 2]))
    b = np.where(lock, np.arcsin(sb), np.arctan2(sb, np.hypot(r[..., 2, 0], r[..., 2, 2])))
    return np.degrees(np.stack([a, b, c], -1))


def rot_zxy(a, b, c, sb=None, cb=None):
    """Rz(a) Rx(b) Ry(c) from degrees (.., 3, 3); sb / cb override sin b / cos b (an exact +-1 / 0, or 1 - 1e-10)."""
    a, b, c = (np.radians(np.asarray(x, np.float64)) for x in (a, b, c))
    sa, ca, sc, cc = np.sin(a), np.cos(a), np.sin(c), np.cos(c)
    sb = np.sin(b) if sb is None else np.asarray(sb, np.float64)
    cb = np.cos(b) if cb is None else np.asarray(cb, np.float64)
    sa, ca, sc, cc, sb, cb = np.broadcast_arrays(sa, ca, sc, cc, sb, cb)
    return np.stack([np.stack([ca * cc - sa * sb * sc, -sa * cb, ca * sc + sa * sb * cc], -1),
                     np.stack([sa * cc + ca * sb * sc, ca * cb, sa * sc - ca * sb * cc], -1),
                     np.stack([-cb * sc, sb, cb * cc], -1)], -2)


def denormalise(poses32, mean, std):
    """(T, 9 J) f32 -> f64 p * std + mean (a product, then a sum)."""
    return np.asarray(poses32, np.float32).astype(np.float64) * std + mean


def smooth(x, tables):
    """scipy.signal.savgol_filter(x, W, 2, axis=0, mode='interp') from bvh.savgol_tables' (mid, head, tail)."""
    mid, head, tail = tables
    W, h, T = mid.shape[0], mid.shape[0] // 2, x.shape[0]
    y = np.empty_like(x)
    for t in range(T):
        if t < h:
            y[t] = head[t] @ x[:W]
        elif t >= T - h:
            y[t] = tail[t - (T - h)] @ x[T - W:]
        else:
            y[t] = mid @ x[t - h:t - h + W]
    return y


def pose_to_euler(poses32, mean, std, tables=None):
    """(T, 9 J) -> (T, 3 J) degrees and the polar factors (T, J, 3, 3)."""
    m = denormalise(poses32, mean, std)
    if tables is not None:
        m = smooth(m, tables)
    r = polar(m.reshape(m.shape[0], -1, 3, 3))
    return euler_zxy(r).reshape(m.shape[0], -1), r


def wrap_diff(a, b):
    d = np.abs(a - b) % 360.0
    return np.minimum(d, 360.0 - d)                                          # +-180 is one angle


# ---- inputs ---------------------------------------------------------------------------------------------------------
def noisy_rotations(seed, T, J, noise=0.3):
    """(poses32 (T, 9 J), mean, std): random rotations plus uniform noise of up to `noise` per entry (halved until the
    smallest singular value is >= 0.5 and the determinant positive), normalised with a random mean / std and rounded
    to f32 - the matrices the kernel sees are denormalise(poses32, mean, std)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ang = rng.uniform(-180.0, 180.0, (3, T, J))
    m = rot_zxy(ang[0], ang[1] * (85.0 / 180.0), ang[2])
    e = rng.uniform(-noise, noise, m.shape)
    for _ in range(8):
        bad = (np.linalg.svd(m + e, compute_uv=False)[..., 2] < 0.55) | (np.linalg.det(m + e) <= 0)
        e[bad] *= 0.5
    mean, std = rng.standard_normal(9 * J), rng.uniform(0.5, 2.0, 9 * J)
    return (((m + e).reshape(T, 9 * J) - mean) / std).astype(np.float32), mean, std


def smooth_rotations(seed, T, J):
    """A slowly turning sequence with small noise (smoothing it keeps every matrix well conditioned)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(T)[:, None]
    a, b, c = (rng.uniform(-150, 150, J) + rng.uniform(-4, 4, J) * t for _ in range(3))
    m = rot_zxy(a, b * 0.25, c) + rng.uniform(-0.05, 0.05, (T, J, 3, 3))
    mean, std = rng.standard_normal(9 * J), rng.uniform(0.5, 2.0, 9 * J)
    return ((m.reshape(T, 9 * J) - mean) / std).astype(np.float32), mean, std
