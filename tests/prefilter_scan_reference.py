"""numpy restatement of the two steps PrefilteringNodelet::cloud_callback takes on the raw scan (apps/prefiltering_nodelet.cpp): deskewing
(:293-354) and the base_link_frame transform (:122-150), float32 where upstream is float and float64 where it is double, operation
for operation.  The chain behind them is tests/prefilter_reference.py.  The switch constants carry the names of the
dgs_prefilter_scan_params fields.

numpy rounds every elementwise float32 / float64 operation once and never fuses a multiply with an add, which is what upstream's
scalar code does without -ffast-math.  `fma=True` is the variant a contracting compiler would produce for the rotation; it exists so
that a test can find points on which the two decide differently.
"""
import numpy as np

import prefilter_reference as R

F = np.float32
D = np.float64
DESKEW_NORM_ORDER = 0          # dgs_prefilter_scan_params.deskew_norm_order default: (x² + y²) + (z² + w²)
TRANSFORM_SETS_W = 1           # dgs_prefilter_scan_params.transform_sets_w default: the transformed point's fourth float is 1.0f
NORM_ORDERS = (0, 1, 2)
SCAN_PERIOD = 0.1              # private_nh.param<double>("scan_period", 0.1) (:340)


def select_imu(queue, stamp):
    """Literal transcription of :318-328 over a Python list of (stamp, payload): -> chosen element; the list is edited in place.
    The caller has checked that the queue is not empty (:295-297)."""
    imu_msg = queue[0]                       # sensor_msgs::ImuConstPtr imu_msg = imu_queue.front();
    loc = 0                                  # auto loc = imu_queue.begin();
    while loc != len(queue):                 # for(; loc != imu_queue.end(); loc++) {
        imu_msg = queue[loc]                 # imu_msg = (*loc);
        if queue[loc][0] > stamp:            # if((*loc)->header.stamp > stamp) {
            break                            # break;
        loc += 1
    del queue[0:loc]                         # imu_queue.erase(imu_queue.begin(), loc);
    return imu_msg


def ang_v_of(angular_velocity):
    """Eigen::Vector3f ang_v(imu.x, imu.y, imu.z); ang_v *= -1 (:330-331)."""
    return np.asarray(angular_velocity, D).astype(F) * F(-1.0)


def _fma(a, b, c):
    # float32 fused multiply-add: the product of two float32 is exact in float64
    return (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)


def quaternions(n, angular_velocity, scan_period=SCAN_PERIOD, deskew_norm_order=DESKEW_NORM_ORDER):
    """delta_q.inverse() for every point index 0..n-1 (:345-347): float32 arrays (x, y, z, w)."""
    ang_v = ang_v_of(angular_velocity)
    i = np.arange(n, dtype=np.int64).astype(D)               # static_cast<double>(i)
    delta_t = D(scan_period) * i / D(n)                      # scan_period * (double)i / cloud->size(), left to right
    half = delta_t / 2.0
    qx, qy, qz = ((half * D(ang_v[k])).astype(F) for k in range(3))
    qw = np.ones(n, F)
    xx, yy, zz, ww = qx * qx, qy * qy, qz * qz, qw * qw
    if deskew_norm_order == 0:
        n2 = (xx + yy) + (zz + ww)
    elif deskew_norm_order == 1:
        n2 = (xx + zz) + (yy + ww)
    elif deskew_norm_order == 2:
        n2 = ((xx + yy) + zz) + ww
    else:
        raise ValueError("deskew_norm_order")
    ok = n2 > F(0)                                           # else the zero quaternion
    safe = np.where(ok, n2, F(1))
    z = np.zeros(n, F)
    return (np.where(ok, -qx / safe, z), np.where(ok, -qy / safe, z), np.where(ok, -qz / safe, z), np.where(ok, qw / safe, z))


def deskew(cloud, angular_velocity=None, scan_period=SCAN_PERIOD, deskew_norm_order=DESKEW_NORM_ORDER, fma=False):
    """deskewing (:293-354).  angular_velocity None is the empty IMU queue: the input bits come back."""
    c = np.array(cloud, F, copy=True)
    if angular_velocity is None or c.shape[0] == 0:
        return c
    with np.errstate(all="ignore"):
        ix, iy, iz, iw = quaternions(c.shape[0], angular_velocity, scan_period, deskew_norm_order)
        vx, vy, vz = c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy()
        if not fma:
            # Eigen's _transformVector: uv = q.vec x v; uv += uv; (v + w * uv) + q.vec x uv
            ux = iy * vz - iz * vy
            uy = iz * vx - ix * vz
            uz = ix * vy - iy * vx
            ux, uy, uz = ux + ux, uy + uy, uz + uz
            c[:, 0] = (vx + iw * ux) + (iy * uz - iz * uy)
            c[:, 1] = (vy + iw * uy) + (iz * ux - ix * uz)
            c[:, 2] = (vz + iw * uz) + (ix * uy - iy * ux)
        else:
            ux = _fma(iy, vz, -(iz * vy))
            uy = _fma(iz, vx, -(ix * vz))
            uz = _fma(ix, vy, -(iy * vx))
            ux, uy, uz = ux + ux, uy + uy, uz + uz
            c[:, 0] = _fma(iw, ux, vx) + _fma(iy, uz, -(iz * uy))
            c[:, 1] = _fma(iw, uy, vy) + _fma(iz, ux, -(ix * uz))
            c[:, 2] = _fma(iw, uz, vz) + _fma(ix, uy, -(iy * ux))
    return c                                                 # the fourth float is copied (:349)


def deskew_exact(xyz, index, n, angular_velocity, scan_period=SCAN_PERIOD, rotation_only=False):
    """Independent float64 formula for float64 points [m,3] at point indices `index`, nothing rounded to float but ang_v itself.
    Upstream multiplies by delta_q.inverse() = conj(q) / |q|², which is not a unit quaternion, through _transformVector, which
    assumes one.  With R the rotation by the unit quaternion conj(q) / |q|, that product is exactly v + (R v - v) / |q|²: the
    rotation, pulled back towards v by the factor 1 / |q|² = 1 / (1 + |delta_t/2 * ang_v|²).  rotation_only returns R v."""
    ang_v = ang_v_of(angular_velocity).astype(D)
    half = D(scan_period) * np.asarray(index, D) / D(n) / 2.0
    q = np.stack([np.ones_like(half), half * ang_v[0], half * ang_v[1], half * ang_v[2]], 1)
    n2 = np.sum(q * q, axis=1)
    q = q / np.sqrt(n2)[:, None]
    w, x, y, z = q[:, 0], -q[:, 1], -q[:, 2], -q[:, 3]        # the inverse of a unit quaternion is its conjugate
    rot = np.empty((q.shape[0], 3, 3), D)
    rot[:, 0, 0] = 1 - 2 * (y * y + z * z); rot[:, 0, 1] = 2 * (x * y - w * z); rot[:, 0, 2] = 2 * (x * z + w * y)
    rot[:, 1, 0] = 2 * (x * y + w * z); rot[:, 1, 1] = 1 - 2 * (x * x + z * z); rot[:, 1, 2] = 2 * (y * z - w * x)
    rot[:, 2, 0] = 2 * (x * z - w * y); rot[:, 2, 1] = 2 * (y * z + w * x); rot[:, 2, 2] = 1 - 2 * (x * x + y * y)
    v = np.asarray(xyz, D)
    rv = np.einsum("nab,nb->na", rot, v)
    return rv if rotation_only else v + (rv - v) / n2[:, None]


def centered(matrix):
    """transform_isometry with m(0,3) = m(1,3) = 0 (:141-142) -> (matrix float64 [4,4], lidar_position float64 [3])."""
    m = np.array(matrix, D).reshape(4, 4)
    m[0, 3] = 0.0
    m[1, 3] = 0.0
    return m, m[:3, 3].copy()


def transform(cloud, matrix=None, transform_sets_w=TRANSFORM_SETS_W):
    """pcl::transformPointCloud(cloud, out, Matrix4d) (:146), the non-dense branch: a non-finite point is copied as it is."""
    c = np.array(cloud, F, copy=True)
    if matrix is None or c.shape[0] == 0:
        return c
    m = np.asarray(matrix, D).reshape(4, 4)
    with np.errstate(all="ignore"):
        x, y, z = c[:, 0].astype(D), c[:, 1].astype(D), c[:, 2].astype(D)
        fin = np.isfinite(c[:, 0]) & np.isfinite(c[:, 1]) & np.isfinite(c[:, 2])
        for r in range(3):
            v = (((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]).astype(F)
            c[fin, r] = v[fin]
        if transform_sets_w:
            c[fin, 3] = F(1.0)
    return c


def head(cloud, angular_velocity=None, base_link_transform=None, scan_period=SCAN_PERIOD, deskew_norm_order=DESKEW_NORM_ORDER,
         transform_sets_w=TRANSFORM_SETS_W, fma=False):
    """cloud_callback :120-150 -> (cloud, lidar_position)."""
    c = deskew(cloud, angular_velocity, scan_period, deskew_norm_order, fma)
    if base_link_transform is None:
        return c, np.zeros(3, D)
    m, lidar = centered(base_link_transform)
    return transform(c, m, transform_sets_w), lidar


def filter_scan(cloud, params=None, angular_velocity=None, base_link_transform=None, scan_period=SCAN_PERIOD,
                deskew_norm_order=DESKEW_NORM_ORDER, transform_sets_w=TRANSFORM_SETS_W, orc=None):
    """cloud_callback :111-164 -> (filtered3d, filtered2d, lidar_position, info of prefilter_reference.cloud_callback)."""
    c, lidar = head(cloud, angular_velocity, base_link_transform, scan_period, deskew_norm_order, transform_sets_w)
    f3, f2, info = R.cloud_callback(c, params, tuple(lidar), orc)
    return f3, f2, lidar, info


def base_link_matrix(yaw=0.3, pitch=-0.05, translation=(0.4, -0.2, 1.7)):
    """A yaw / pitch / translation isometry as the tf lookup would give it (float64 [4,4])."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], D)
    ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], D)
    m = np.eye(4)
    m[:3, :3] = rz @ ry
    m[:3, 3] = translation
    return m
