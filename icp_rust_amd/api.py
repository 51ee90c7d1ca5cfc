"""Host-side mirror of the reference crate's public interface (src/lib.rs:12-26) over the
C ABI: same names, same argument meaning, same failure behaviour.

    Transform, Icp2d, Icp3d, residual, error, huber_error, estimate_transform,
    gauss_newton_update, weighted_gauss_newton_update, norm, se2, so2

`Option::None` becomes Python `None`; the reference's two panics (empty `dst`, NaN
residual) become `IcpError`.  All compute runs in libicp_mi355x.so on the GPU.
Point sets are numpy arrays (n x 2 / n x 3 float64, C order = `&[Vector2]`/`&[Vector3]`)
or CUDA torch tensors of the same shape, which are used in place (no copy).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import IcpError, Pose, check, lib  # noqa: F401

_dp = C.POINTER(C.c_double)


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _host(a, dim):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size == 0:
        a = a.reshape(0, dim)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError(f"expected an (n, {dim}) float64 array, got {a.shape}")
    return a


def _ptr(a):
    return C.c_void_p(a.ctypes.data if a.size else None)


def _dev_points(t, dim, device, what="points"):
    """A device-tensor argument of the C ABI: contiguous float64 (n, dim) on the handle's GPU.  Anything
    else (float32, a strided slice such as pts[:, :3], a 2-column tensor for Icp3d, another GPU) would be
    read out of bounds or misread by the kernels, so it is refused here."""
    if not _is_device_tensor(t):
        raise ValueError(f"{what}: expected a CUDA tensor")
    if t.dim() != 2 or t.shape[1] != dim or str(t.dtype) != "torch.float64" or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous (n, {dim}) float64 CUDA tensor, got "
                         f"{tuple(t.shape)} {t.dtype} contiguous={t.is_contiguous()}")
    if device is not None and t.device.index != device:
        raise ValueError(f"{what}: tensor lives on cuda:{t.device.index}, the handle on cuda:{device}")
    return t


def _dev_index(t, n, device, what="idx"):
    """A device index buffer: contiguous 4-byte integers, at least n of them, on the handle's GPU."""
    if not _is_device_tensor(t):
        raise ValueError(f"{what}: expected a CUDA tensor")
    if t.dim() != 1 or t.element_size() != 4 or t.dtype.is_floating_point or not t.is_contiguous() or t.shape[0] < n:
        raise ValueError(f"{what}: expected a contiguous int32/uint32 CUDA tensor of length >= {n}")
    if device is not None and t.device.index != device:
        raise ValueError(f"{what}: tensor lives on cuda:{t.device.index}, the handle on cuda:{device}")
    return t


def _vec(v, n):
    a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"expected {n} values")
    return a


def _voxel_size(voxel_size):
    v = float(voxel_size)
    if not (np.isfinite(v) and v >= np.finfo(np.float64).tiny):
        raise ValueError(f"a voxel size must be finite and at least DBL_MIN, got {v}")
    return v


def voxel_downsample(points, voxel_size, return_index=False, device=-1):
    """EXTENSION (icp_voxel_downsample[_device], include/icp_mi355x.h section 22): the first point of every voxel, in
    order.  The cell of a point is floor(p / voxel_size) per axis in f64; two points share a voxel iff their cells
    are equal; a point with a NaN or infinite coordinate is dropped.  `points` is (n, 2) or (n, 3): a numpy array
    (or anything numpy converts) gives numpy arrays; a contiguous float64 CUDA tensor gives CUDA tensors, computed on
    torch's current stream.  Returns the kept points; with return_index=True also their indices in `points`
    (ascending; uint32 in numpy, int32 bits in torch)."""
    v = _voxel_size(voxel_size)
    kept = C.c_size_t(0)
    if _is_device_tensor(points):
        import torch

        if points.dim() != 2 or points.shape[1] not in (2, 3):
            raise ValueError(f"points: expected (n, 2) or (n, 3), got {tuple(points.shape)}")
        dim = points.shape[1]
        _dev_points(points, dim, None if device < 0 else device)
        n = points.shape[0]
        out = torch.empty_like(points)
        index = torch.empty(max(n, 1), dtype=torch.int32, device=points.device) if return_index else None
        with torch.cuda.device(points.device):
            stream = torch.cuda.current_stream().cuda_stream
            check(lib().icp_voxel_downsample_device(dim, C.c_void_p(points.data_ptr()), n, v, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(index.data_ptr()) if return_index else None,
                                                    C.byref(kept), points.device.index, C.c_void_p(stream)),
                  "icp_voxel_downsample_device")
        out = out[:kept.value]
        return (out, index[:kept.value]) if return_index else out
    p = np.ascontiguousarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] not in (2, 3):
        raise ValueError(f"points: expected (n, 2) or (n, 3), got {p.shape}")
    n, dim = p.shape
    out = np.empty((max(n, 1), dim), dtype=np.float64)
    index = np.zeros(max(n, 1), dtype=np.uint32) if return_index else None
    check(lib().icp_voxel_downsample(dim, _ptr(p), n, v, C.c_void_p(out.ctypes.data),
                                     C.c_void_p(index.ctypes.data) if return_index else None, C.byref(kept),
                                     int(device)), "icp_voxel_downsample")
    out = out[:kept.value].copy()
    return (out, index[:kept.value].copy()) if return_index else out


def voxel_centroids(points, voxel_size, return_counts=False, return_index=False, return_inverse=False, device=-1):
    """EXTENSION (icp_voxel_centroids[_device], include/icp_mi355x.h section 25): the mean of the points of every
    occupied voxel.  Membership is voxel_downsample's (the cell is floor(p / voxel_size) per axis in f64; a point with a
    NaN or infinite coordinate is in no voxel); the voxels come in ascending order of their lowest member index, which
    is the order of voxel_downsample's kept points; a sum is the fixed fold tree of section 9 over the members in
    ascending index, then one division by the count: the same bytes from every call.  `points` is (n, 2) or (n, 3): a
    numpy array (or anything numpy converts) gives numpy arrays; a contiguous float64 CUDA tensor gives CUDA tensors,
    computed on torch's current stream.  Returns the means, then -- each only if asked for, in this order -- the
    members per voxel (return_counts), every voxel's lowest member index (return_index: voxel_downsample's index) and
    per point the number of its voxel, 0xffffffff for a dropped point (return_inverse); uint32 in numpy, int32 bits in
    torch."""
    v = _voxel_size(voxel_size)
    voxels = C.c_size_t(0)
    if _is_device_tensor(points):
        import torch

        if points.dim() != 2 or points.shape[1] not in (2, 3):
            raise ValueError(f"points: expected (n, 2) or (n, 3), got {tuple(points.shape)}")
        dim = points.shape[1]
        _dev_points(points, dim, None if device < 0 else device)
        n = points.shape[0]
        means = torch.empty_like(points)

        def words(wanted):
            return torch.empty(max(n, 1), dtype=torch.int32, device=points.device) if wanted else None

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None

        counts, index, inverse = words(return_counts), words(return_index), words(return_inverse)
        with torch.cuda.device(points.device):
            stream = torch.cuda.current_stream().cuda_stream
            check(lib().icp_voxel_centroids_device(dim, C.c_void_p(points.data_ptr()), n, v, ptr(means), ptr(counts),
                                                   ptr(index), ptr(inverse), C.byref(voxels), points.device.index,
                                                   C.c_void_p(stream)), "icp_voxel_centroids_device")
        k = voxels.value
        out = [means[:k]]
        out += [counts[:k]] if return_counts else []
        out += [index[:k]] if return_index else []
        out += [inverse[:n]] if return_inverse else []
        return tuple(out) if len(out) > 1 else out[0]
    p = np.ascontiguousarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] not in (2, 3):
        raise ValueError(f"points: expected (n, 2) or (n, 3), got {p.shape}")
    n, dim = p.shape
    means = np.empty((max(n, 1), dim), dtype=np.float64)
    counts, index, inverse = (np.zeros(max(n, 1), dtype=np.uint32) if wanted else None
                              for wanted in (return_counts, return_index, return_inverse))

    def ptr(a):
        return C.c_void_p(a.ctypes.data) if a is not None else None

    check(lib().icp_voxel_centroids(dim, _ptr(p), n, v, ptr(means), ptr(counts), ptr(index), ptr(inverse),
                                    C.byref(voxels), int(device)), "icp_voxel_centroids")
    k = voxels.value
    out = [means[:k].copy()]
    out += [counts[:k].copy()] if return_counts else []
    out += [index[:k].copy()] if return_index else []
    out += [inverse[:n].copy()] if return_inverse else []
    return tuple(out) if len(out) > 1 else out[0]


def _mirrored(packed, dim, xp):
    """(V, dim (dim + 1) / 2) packed second moments (xx, xy, yy / xx, xy, xz, yy, yz, zz) -> (V, dim, dim) symmetric: a
    pure copy of the packed values (xp: numpy or torch)"""
    pairs = [(a, b) for a in range(dim) for b in range(a, dim)]
    at = {ab: k for k, ab in enumerate(pairs)}
    order = [at[(min(a, b), max(a, b))] for a in range(dim) for b in range(dim)]
    if xp is np:
        return np.ascontiguousarray(packed[:, order]).reshape(-1, dim, dim)
    return packed[:, order].reshape(-1, dim, dim).contiguous()


def voxel_covariances(points, voxel_size, ddof=1, return_means=True, return_counts=False, return_index=False,
                      return_inverse=False, packed=False, device=-1):
    """EXTENSION (icp_voxel_covariances[_device], include/icp_mi355x.h section 26): the covariance of the points of
    every occupied voxel about the voxel's mean.  Membership, the order of the voxels and the means are
    voxel_centroids' (section 25), bit for bit; a second moment is the fixed fold tree of section 9 over the products
    (x_a - m_a) (x_b - m_b) of the members in ascending index, then one division by count - ddof (ddof 0 or 1; a voxel
    with count <= ddof gets +0.0): the same bytes from every call.  `points` is (n, 2) or (n, 3): a numpy array (or
    anything numpy converts) gives numpy arrays; a contiguous float64 CUDA tensor gives CUDA tensors, computed on torch's
    current stream.  Returns the covariances, (V, dim, dim) symmetric -- the mirroring is a copy -- or, with packed=True,
    (V, dim (dim + 1) / 2) in the order xx, xy, yy / xx, xy, xz, yy, yz, zz; then -- each only if asked for, in this
    order -- the means (return_means, on by default), the members per voxel (return_counts), every voxel's lowest member
    index (return_index) and per point the number of its voxel, 0xffffffff for a dropped point (return_inverse); uint32
    in numpy, int32 bits in torch."""
    v = _voxel_size(voxel_size)
    if ddof not in (0, 1) or isinstance(ddof, bool):
        raise ValueError(f"ddof must be 0 or 1, got {ddof!r}")
    ddof = int(ddof)
    voxels = C.c_size_t(0)
    if _is_device_tensor(points):
        import torch

        if points.dim() != 2 or points.shape[1] not in (2, 3):
            raise ValueError(f"points: expected (n, 2) or (n, 3), got {tuple(points.shape)}")
        dim = points.shape[1]
        _dev_points(points, dim, None if device < 0 else device)
        n, ns = points.shape[0], dim * (dim + 1) // 2
        cov = torch.empty((max(n, 1), ns), dtype=torch.float64, device=points.device)
        means = torch.empty_like(points) if return_means else None

        def words(wanted):
            return torch.empty(max(n, 1), dtype=torch.int32, device=points.device) if wanted else None

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None

        counts, index, inverse = words(return_counts), words(return_index), words(return_inverse)
        with torch.cuda.device(points.device):
            stream = torch.cuda.current_stream().cuda_stream
            check(lib().icp_voxel_covariances_device(dim, C.c_void_p(points.data_ptr()), n, v, ddof, ptr(cov), ptr(means),
                                                     ptr(counts), ptr(index), ptr(inverse), C.byref(voxels),
                                                     points.device.index, C.c_void_p(stream)),
                  "icp_voxel_covariances_device")
            k = voxels.value
            out = [cov[:k] if packed else _mirrored(cov[:k], dim, torch)]
        out += [means[:k]] if return_means else []
        out += [counts[:k]] if return_counts else []
        out += [index[:k]] if return_index else []
        out += [inverse[:n]] if return_inverse else []
        return tuple(out) if len(out) > 1 else out[0]
    p = np.ascontiguousarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] not in (2, 3):
        raise ValueError(f"points: expected (n, 2) or (n, 3), got {p.shape}")
    n, dim = p.shape
    cov = np.empty((max(n, 1), dim * (dim + 1) // 2), dtype=np.float64)
    means = np.empty((max(n, 1), dim), dtype=np.float64) if return_means else None
    counts, index, inverse = (np.zeros(max(n, 1), dtype=np.uint32) if wanted else None
                              for wanted in (return_counts, return_index, return_inverse))

    def ptr(a):
        return C.c_void_p(a.ctypes.data) if a is not None else None

    check(lib().icp_voxel_covariances(dim, _ptr(p), n, v, ddof, ptr(cov), ptr(means), ptr(counts), ptr(index),
                                      ptr(inverse), C.byref(voxels), int(device)), "icp_voxel_covariances")
    k = voxels.value
    out = [cov[:k].copy() if packed else _mirrored(cov[:k], dim, np)]
    out += [means[:k].copy()] if return_means else []
    out += [counts[:k].copy()] if return_counts else []
    out += [index[:k].copy()] if return_index else []
    out += [inverse[:n].copy()] if return_inverse else []
    return tuple(out) if len(out) > 1 else out[0]


def _list_length(k, most, what="k"):
    if int(k) != k or not 1 <= int(k) <= most:
        raise ValueError(f"{what} must be an integer in [1, {most}], got {k}")
    return int(k)


def _radius_rule(radius, min_neighbours):
    r = float(radius)
    if not r >= 0.0:  # (also a NaN)
        raise ValueError(f"a radius must be >= 0 (or +inf), got {r}")
    if int(min_neighbours) != min_neighbours or min_neighbours < 0:
        raise ValueError(f"min_neighbours must be a count, got {min_neighbours}")
    return r, int(min_neighbours)


def _count_rule(radius, cap):
    r, _ = _radius_rule(radius, 0)
    if cap is None:
        return r, 0xFFFFFFFF
    if int(cap) != cap or not 1 <= int(cap) <= 0xFFFFFFFF:
        raise ValueError(f"cap must be an integer in [1, 2^32 - 1] (or None: the full count), got {cap}")
    return r, int(cap)


def _statistical_rule(k, std_ratio):
    ratio = float(std_ratio)
    if ratio != ratio:
        raise ValueError("std_ratio must not be NaN")
    return _list_length(k, 31), ratio


def _filter_cloud(points, what, rule):
    """the module-level filters: a temporary handle on `points`, one removal, the kept points (and their indices) from
    its new_index table.  numpy in, numpy out; a contiguous float64 CUDA tensor in, CUDA tensors out."""
    on_device = _is_device_tensor(points)
    if on_device:
        if points.dim() != 2 or points.shape[1] not in (2, 3):
            raise ValueError(f"{what}: expected (n, 2) or (n, 3), got {tuple(points.shape)}")
        dim, n = points.shape[1], points.shape[0]
        _dev_points(points, dim, None, what)
        p = points
    else:
        p = np.ascontiguousarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] not in (2, 3):
            raise ValueError(f"{what}: expected (n, 2) or (n, 3), got {p.shape}")
        n, dim = p.shape
    if n == 0:
        kept = np.zeros(0, dtype=np.uint32)
    else:
        icp = (Icp2d if dim == 2 else Icp3d)(p)
        try:
            _, new_index = rule(icp)
        finally:
            icp.close()
        kept = np.flatnonzero(new_index != 0xFFFFFFFF).astype(np.uint32)
    if on_device:
        import torch

        index = torch.from_numpy(kept.astype(np.int64)).to(points.device)
        return points[index], index.to(torch.int32)
    return p[kept], kept


def remove_radius_outliers(points, radius, min_neighbours, return_index=False):
    """EXTENSION (icp_remove_radius_outliers, include/icp_mi355x.h section 23): the points with at least
    `min_neighbours` points, themselves included, within `radius` (d^2 <= radius * radius), in order.  `points` as for
    voxel_downsample; with return_index=True also the kept points' ascending indices."""
    r, need = _radius_rule(radius, min_neighbours)
    out, index = _filter_cloud(points, "points", lambda icp: icp.remove_radius_outliers(r, need, return_index=True))
    return (out, index) if return_index else out


def remove_statistical_outliers(points, k, std_ratio, return_index=False):
    """EXTENSION (icp_remove_statistical_outliers, section 23): the points whose mean distance to their k nearest other
    points is not above mean + std_ratio * deviation of that figure over the cloud, in order."""
    kk, ratio = _statistical_rule(k, std_ratio)
    out, index = _filter_cloud(points, "points",
                               lambda icp: icp.remove_statistical_outliers(kk, ratio, return_index=True))
    return (out, index) if return_index else out


class Transform:
    """`icp::Transform` (src/transform.rs:6-51)."""

    __slots__ = ("pose",)

    def __init__(self, param=None):
        """Transform::new(&param) (src/transform.rs:13-16); no argument = identity."""
        self.pose = Pose()
        if param is None:
            lib().icp_transform_identity(C.byref(self.pose))
        else:
            p = _vec(param, 3)
            lib().icp_transform_new(p.ctypes.data_as(_dp), C.byref(self.pose))

    @staticmethod
    def new(param):
        return Transform(param)

    @staticmethod
    def identity():
        return Transform()

    @staticmethod
    def from_rt(rot, t):
        """rot: 2x2 (row-major numpy), t: 2 (src/transform.rs:18-20)."""
        r = np.asarray(rot, dtype=np.float64).reshape(2, 2)
        cm = np.array([r[0, 0], r[1, 0], r[0, 1], r[1, 1]])
        tt = _vec(t, 2)
        o = Transform()
        lib().icp_transform_from_rt(cm.ctypes.data_as(_dp), tt.ctypes.data_as(_dp), C.byref(o.pose))
        return o

    @staticmethod
    def from_pose(pose):
        o = Transform()
        C.memmove(C.byref(o.pose), C.byref(pose), C.sizeof(Pose))
        return o

    @property
    def rot(self):
        p = self.pose
        return np.array([[p.r00, p.r01], [p.r10, p.r11]])

    @property
    def t(self):
        return np.array([self.pose.tx, self.pose.ty])

    def transform(self, landmark):
        p = _vec(landmark, 2)
        out = np.zeros(2)
        lib().icp_transform_apply(C.byref(self.pose), p.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
        return out

    def inverse(self):
        o = Transform()
        lib().icp_transform_inverse(C.byref(self.pose), C.byref(o.pose))
        return o

    def __mul__(self, rhs):
        o = Transform()
        lib().icp_transform_mul(C.byref(self.pose), C.byref(rhs.pose), C.byref(o.pose))
        return o

    def as_array(self):
        return np.array(self.pose.as_tuple())

    def __repr__(self):
        return f"Transform(rot={self.rot.tolist()}, t={self.t.tolist()})"


class _Se2:
    """`icp::se2` (src/se2.rs)."""

    @staticmethod
    def exp(param):
        p = _vec(param, 3)
        m = np.zeros(9)
        lib().icp_se2_exp(p.ctypes.data_as(_dp), m.ctypes.data_as(_dp))
        return m.reshape(3, 3)

    @staticmethod
    def log(transform):
        m = _vec(transform, 9)
        p = np.zeros(3)
        lib().icp_se2_log(m.ctypes.data_as(_dp), p.ctypes.data_as(_dp))
        return p

    @staticmethod
    def get_rt(transform):
        m = _vec(transform, 9)
        r = np.zeros(4)
        t = np.zeros(2)
        lib().icp_se2_get_rt(m.ctypes.data_as(_dp), r.ctypes.data_as(_dp), t.ctypes.data_as(_dp))
        return r.reshape(2, 2), t

    @staticmethod
    def calc_rt(param):
        T = Transform(param)
        return T.rot, T.t


class _So2:
    """`icp::so2` (src/so2.rs)."""

    @staticmethod
    def exp(theta):
        m = np.zeros(4)
        lib().icp_so2_exp(float(theta), m.ctypes.data_as(_dp))
        return np.array([[m[0], m[2]], [m[1], m[3]]])

    new_rotation2 = exp

    @staticmethod
    def log(rotation):
        r = np.asarray(rotation, dtype=np.float64).reshape(2, 2)
        cm = np.array([r[0, 0], r[1, 0], r[0, 1], r[1, 1]])
        return lib().icp_so2_log(cm.ctypes.data_as(_dp))


se2 = _Se2()
so2 = _So2()


def norm(matrix):
    """`icp::norm` (src/norm.rs:19-21)."""
    m = np.asarray(matrix, dtype=np.float64)
    m = np.asfortranarray(m.reshape(m.shape[0], -1))
    return lib().icp_norm(m.ctypes.data_as(_dp), m.shape[0], m.shape[1])


def residual(transform, src, dst):
    """`icp::residual` (src/lib.rs:34-36)."""
    return transform.transform(src) - _vec(dst, 2)


def _pairs(src, dst):
    a = _host(src, 2)
    b = _host(dst, 2)
    if a.shape != b.shape:
        raise ValueError("src and dst differ in length")  # debug_assert_eq!, src/lib.rs:223
    return a, b


def error(transform, src, dst):
    """`icp::error` (src/lib.rs:38-43)."""
    a, b = _pairs(src, dst)
    out = C.c_double()
    check(lib().icp_error(C.byref(transform.pose), _ptr(a), _ptr(b), a.shape[0], C.byref(out)), "error")
    return out.value


def huber_error(transform, src, dst):
    """`icp::huber_error` (src/lib.rs:45-50)."""
    a, b = _pairs(src, dst)
    out = C.c_double()
    check(lib().icp_huber_error(C.byref(transform.pose), _ptr(a), _ptr(b), a.shape[0], C.byref(out)),
          "huber_error")
    return out.value


def gauss_newton_update(transform, src, dst):
    """`icp::gauss_newton_update` (src/lib.rs:191-216) -> Param or None."""
    a, b = _pairs(src, dst)
    d = np.zeros(3)
    rc = check(lib().icp_gauss_newton_update(C.byref(transform.pose), _ptr(a), _ptr(b), a.shape[0],
                                             d.ctypes.data_as(_dp)), "gauss_newton_update",
               allow=(_lib.NONE,))
    return None if rc == _lib.NONE else d


def weighted_gauss_newton_update(transform, src, dst):
    """`icp::weighted_gauss_newton_update` (src/lib.rs:218-261) -> Param or None."""
    a, b = _pairs(src, dst)
    d = np.zeros(3)
    rc = check(lib().icp_weighted_gauss_newton_update(C.byref(transform.pose), _ptr(a), _ptr(b),
                                                      a.shape[0], d.ctypes.data_as(_dp)),
               "weighted_gauss_newton_update", allow=(_lib.NONE,))
    return None if rc == _lib.NONE else d


def residual_stddevs(transform, src, dst):
    """stats::calc_stddevs over the residuals (src/stats.rs:49-60 at src/lib.rs:236)."""
    a, b = _pairs(src, dst)
    s = np.zeros(2)
    rc = check(lib().icp_residual_stddevs(C.byref(transform.pose), _ptr(a), _ptr(b), a.shape[0],
                                          s.ctypes.data_as(_dp)), "residual_stddevs", allow=(_lib.NONE,))
    return None if rc == _lib.NONE else s


def estimate_transform(src, dst, return_inner_iters=False):
    """`icp::estimate_transform` (src/lib.rs:59-84)."""
    a, b = _pairs(src, dst)
    o = Transform()
    inner = C.c_uint32(0)
    check(lib().icp_estimate_transform(_ptr(a), _ptr(b), a.shape[0], C.byref(o.pose), C.byref(inner)),
          "estimate_transform")
    return (o, inner.value) if return_inner_iters else o


def reduce_geometry(n):
    b, t = C.c_int(), C.c_int()
    lib().icp_reduce_geometry(n, C.byref(b), C.byref(t))
    return b.value, t.value


def gn_path_counters(icp=None):
    """(window started, window missed, short pipeline, radix path, speculative searches confirmed,
    discarded) counts of a handle (default: the scratch handle behind the free functions)."""
    out = (C.c_uint64 * 6)()
    check(lib().icp_gn_path_counters(icp._h if icp is not None else None, out), "icp_gn_path_counters")
    return tuple(int(x) for x in out)


def gn_filed_counters(icp=None):
    """(evaluations with filed candidates -- finished by k_win_pick / k_win_pick2 --, window evaluations still to take
    the second pass) of a handle (default: the scratch handle behind the free functions)."""
    out = (C.c_uint64 * 2)()
    check(lib().icp_gn_filed_counters(icp._h if icp is not None else None, out), "icp_gn_filed_counters")
    return tuple(int(x) for x in out)


def gn_loop_counters(icp=None):
    """(launches, evaluations served, launches that handed an evaluation back) of the one-launch inner loop"""
    out = (C.c_uint64 * 3)()
    check(lib().icp_gn_loop_counters(icp._h if icp is not None else None, out), "icp_gn_loop_counters")
    return tuple(int(x) for x in out)


def gn_loop_timeouts(icp):
    """launches of the one-launch inner loop that gave up their bounded wait (not fully resident)"""
    out = C.c_uint64(0)
    check(lib().icp_gn_loop_timeouts(icp._h, C.byref(out)), "icp_gn_loop_timeouts")
    return int(out.value)


def fixed_point_skips(icp):
    """outer iterations not run because the pose had stopped moving (their inner counts are 0, the result the same bits)"""
    out = C.c_uint64(0)
    check(lib().icp_fixed_point_skips(icp._h, C.byref(out)), "icp_fixed_point_skips")
    return int(out.value)


def run_ahead_counters(icp):
    """(run-ahead searches whose device-derived pose the host confirmed bit for bit, ... that it did not)"""
    out = (C.c_uint64 * 2)()
    check(lib().icp_run_ahead_counters(icp._h, out), "icp_run_ahead_counters")
    return tuple(int(x) for x in out)


def nn_cert_counters(icp):
    """(searches that checked certificates so far, queries whose certificate failed in the last of them)"""
    out = (C.c_uint64 * 2)()
    check(lib().icp_nn_cert_counters(icp._h, out), "icp_nn_cert_counters")
    return int(out[0]), int(out[1])


class Quality:
    """The quality of a pose (`icp_quality`, include/icp_mi355x.h section 9) -- an extension beyond the reference.
    n source points; inliers, those whose nearest target lies within the distance bound; fitness = inliers / n;
    inlier_rmse and inlier_sum_d2 of the inliers' squared distances; error and huber_error, the reference's icp::error /
    huber_error of the correspondences at the pose (src/lib.rs:38-50); information, the 3 x 3 SE(2) information matrix
    of the inlier pairs in (x, y, theta) (the jtj of gauss_newton_update at identity, src/lib.rs:191-216)."""

    __slots__ = ("n", "inliers", "fitness", "inlier_rmse", "inlier_sum_d2", "error", "huber_error", "information")

    def __init__(self, q):
        self.n, self.inliers = int(q.n), int(q.inliers)
        self.fitness, self.inlier_rmse, self.inlier_sum_d2 = q.fitness, q.inlier_rmse, q.inlier_sum_d2
        self.error, self.huber_error = q.error, q.huber_error
        self.information = np.array(q.information[:], dtype=np.float64).reshape(3, 3)

    def as_array(self):
        """the float fields in struct order (fitness, inlier_rmse, inlier_sum_d2, error, huber_error, information
        row-major): what a bit-for-bit comparison compares, next to n and inliers"""
        return np.array([self.fitness, self.inlier_rmse, self.inlier_sum_d2, self.error, self.huber_error,
                         *self.information.ravel()])

    def __repr__(self):
        return (f"Quality(n={self.n}, inliers={self.inliers}, fitness={self.fitness:.6g}, "
                f"inlier_rmse={self.inlier_rmse:.6g}, error={self.error:.6g}, huber_error={self.huber_error:.6g})")


class _NormalQuality:
    """What PlaneQuality and LineQuality share; `_RESIDUAL` ("plane" / "line") names the residual and with it the two
    attributes <residual>_rmse and <residual>_sum_r2, which the code here reaches as _rmse and _sum_r2."""

    __slots__ = ()
    _RESIDUAL = None

    def __init_subclass__(cls):
        # (the subclass's two slot descriptors under a second name: plain attribute access, nothing looked up by name
        # per object -- a batch builds one object per item)
        cls._FIELDS = (cls._RESIDUAL + "_rmse", cls._RESIDUAL + "_sum_r2")
        cls._rmse, cls._sum_r2 = (cls.__dict__[name] for name in cls._FIELDS)

    def __init__(self, q):
        rmse, sum_r2 = self._FIELDS
        self.n, self.inliers = int(q.n), int(q.inliers)
        self.fitness, self.inlier_rmse, self.inlier_sum_d2 = q.fitness, q.inlier_rmse, q.inlier_sum_d2
        self._rmse, self._sum_r2 = getattr(q, rmse), getattr(q, sum_r2)
        self.error, self.huber_error = q.error, q.huber_error
        self.information = np.array(q.information[:], dtype=np.float64).reshape(3, 3)
        self.translation_eig = np.array(q.translation_eig[:], dtype=np.float64)

    def as_array(self):
        """the float fields in struct order (fitness, inlier_rmse, inlier_sum_d2, <residual>_rmse, <residual>_sum_r2,
        error, huber_error, information row-major, translation_eig): what a bit-for-bit comparison compares, next to n
        and inliers"""
        return np.array([self.fitness, self.inlier_rmse, self.inlier_sum_d2, self._rmse, self._sum_r2, self.error,
                         self.huber_error, *self.information.ravel(), *self.translation_eig])

    def weak_direction(self):
        """the unit vector of the xy plane along which the translation is observed least: the eigenvector of lmin of the
        2 x 2 translation block (numpy.linalg.eigh; a convenience, no bit claim)"""
        _, vecs = np.linalg.eigh(self.information[:2, :2])
        return vecs[:, 0]

    def __repr__(self):
        return (f"{type(self).__name__}(n={self.n}, inliers={self.inliers}, fitness={self.fitness:.6g}, "
                f"inlier_rmse={self.inlier_rmse:.6g}, {self._FIELDS[0]}={self._rmse:.6g}, "
                f"translation_eig=({self.translation_eig[0]:.6g}, {self.translation_eig[1]:.6g}))")


class PlaneQuality(_NormalQuality):
    """The quality of a pose under the point-to-plane residual (`icp_plane_quality`, include/icp_mi355x.h section 13) --
    an extension beyond the reference.  n, inliers, fitness, inlier_rmse and inlier_sum_d2 as in Quality (same bits at
    the same pose and bound); plane_rmse and plane_sum_r2 of the inliers' squared plane residuals; error and
    huber_error, the folds of p2 and rho(p2) over all points; information, the 3 x 3 SE(2) information matrix the plane
    residual gives on the inlier pairs in (x, y, theta), rank-deficient where the scene is; translation_eig, the
    eigenvalues (lmin, lmax) of its 2 x 2 translation block."""

    __slots__ = ("n", "inliers", "fitness", "inlier_rmse", "inlier_sum_d2", "plane_rmse", "plane_sum_r2", "error",
                 "huber_error", "information", "translation_eig")
    _RESIDUAL = "plane"


class LineQuality(_NormalQuality):
    """The quality of a pose under the point-to-line residual (`icp_line_quality`, include/icp_mi355x.h section 16) -- an
    extension beyond the reference.  n, inliers, fitness, inlier_rmse and inlier_sum_d2 as in Quality (same bits at the
    same pose and bound); line_rmse and line_sum_r2 of the inliers' squared line residuals; error and huber_error, the
    folds of p2 and rho(p2) over all points; information, the 3 x 3 SE(2) information matrix the line residual gives on
    the inlier pairs in (x, y, theta), rank-deficient where the scene is; translation_eig, the eigenvalues (lmin, lmax)
    of its 2 x 2 translation block."""

    __slots__ = ("n", "inliers", "fitness", "inlier_rmse", "inlier_sum_d2", "line_rmse", "line_sum_r2", "error",
                 "huber_error", "information", "translation_eig")
    _RESIDUAL = "line"


class _Icp:
    DIM = 0

    def __init__(self, dst, device=-1, nn_mode=_lib.NN_AUTO):
        """Icp2d::new / Icp3d::new (src/lib.rs:97-102, 139-144)."""
        self._h = C.c_void_p()
        self._keep = None
        self._device = None      # GPU index, known once a device tensor has been seen
        self._own_stream = True  # the handle runs on its private streams (icp_set_stream not called)
        if _is_device_tensor(dst):
            dev = dst.device.index if device < 0 else device
            _dev_points(dst, self.DIM, dev, "dst")
            self._keep = dst  # borrowed for the handle's lifetime, like `&'a [Vector]`
            self._device = dev
            self.m = dst.shape[0]
            self._after_producer(dst)
            check(lib().icp_create_device(C.byref(self._h), self.DIM, C.c_void_p(dst.data_ptr()),
                                          self.m, dev), "icp_create_device")
        else:
            d = _host(dst, self.DIM)
            self.m = d.shape[0]
            check(lib().icp_create(C.byref(self._h), self.DIM, _ptr(d), self.m, device), "icp_create")
        if nn_mode != _lib.NN_AUTO:
            check(lib().icp_set_nn_mode(self._h, nn_mode), "icp_set_nn_mode")

    def _after_producer(self, t):
        """The handle's private streams are not ordered against the torch stream that produced a device
        tensor (include/icp_mi355x.h: "device inputs must be complete when the call is made"): wait for
        torch's current stream on that device.  Not needed -- and not done -- once icp_set_stream has put
        the handle on the caller's stream, where everything is ordered."""
        if self._own_stream:
            import torch

            torch.cuda.current_stream(t.device).synchronize()

    def _dev(self, t, what):
        if self._device is None:
            self._device = t.device.index
        _dev_points(t, self.DIM, self._device, what)
        self._after_producer(t)
        return t

    def _dev_pairs(self, t, what):
        if self._device is None:
            self._device = t.device.index
        _dev_points(t, 2, self._device, what)
        self._after_producer(t)
        return t

    def last_fold_order(self, n, with_cells=False):
        """The order in which the last estimate() call on this handle folded its sums over the `n` source
        points (icp_last_fold_order): perm[k] = caller's index of the k-th folded point (identity when the
        call took no cell-sorted snapshot); with_cells=True also returns the sort keys."""
        perm = np.zeros(max(n, 1), dtype=np.uint32)
        cell = np.zeros(max(n, 1), dtype=np.uint32)
        check(lib().icp_last_fold_order(self._h, n, C.c_void_p(perm.ctypes.data), C.c_void_p(cell.ctypes.data)),
              "icp_last_fold_order")
        perm = perm[:n].astype(np.int64)
        return (perm, cell[:n]) if with_cells else perm

    def sort_source_device(self, d_src, transform):
        """(sorted copy, permutation) of a device-resident source cloud in the fold order of an estimate call
        that starts at `transform` (icp_sort_source_device)."""
        import torch

        self._dev(d_src, "src")
        out = torch.empty_like(d_src)
        perm = torch.empty(max(d_src.shape[0], 1), dtype=torch.int32, device=d_src.device)
        check(lib().icp_sort_source_device(self._h, C.c_void_p(d_src.data_ptr()), d_src.shape[0],
                                           C.byref(transform.pose), C.c_void_p(out.data_ptr()),
                                           C.c_void_p(perm.data_ptr())), "icp_sort_source_device")
        check(lib().icp_synchronize(self._h), "icp_synchronize")  # (produced on the handle's stream)
        return out, perm[:d_src.shape[0]]

    # -- the reference's method ------------------------------------------------------
    def estimate(self, src, initial_transform, max_iter, return_info=False, max_correspondence_distance=None):
        """Icp2d::estimate / Icp3d::estimate (src/lib.rs:105-130, 148-173).  return_info=True also
        returns the last correspondence indices and the inner-iteration counts; "inner" only the
        counts (no index buffer, no device-to-host copy).
        EXTENSION (include/icp_mi355x.h section 10): with max_correspondence_distance = r the estimator of every
        outer iteration sees only the pairs with d2 <= r * r (icp_estimate_gated[_device]; evaluate()'s inlier
        rule), and return_info also returns the per-iteration inlier counts, after the inner counts.  None calls
        what it always called and returns what it always returned."""
        if max_correspondence_distance is not None:
            return self._estimate_gated(src, initial_transform, max_iter, return_info,
                                        float(max_correspondence_distance))
        o = Transform()
        inner = np.zeros(max(max_iter, 1), dtype=np.uint32)
        if _is_device_tensor(src):
            import torch

            self._dev(src, "src")
            n = src.shape[0]
            want_idx = bool(return_info) and return_info != "inner"
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=src.device) if want_idx else None
            check(lib().icp_estimate_device(self._h, C.c_void_p(src.data_ptr()), n,
                                            C.byref(initial_transform.pose), max_iter, C.byref(o.pose),
                                            C.c_void_p(idx.data_ptr()) if want_idx else None,
                                            C.c_void_p(inner.ctypes.data)), "icp_estimate_device")
            if return_info == "inner":
                return o, inner[:max_iter]
            if return_info:
                return o, idx[:n].cpu().numpy().view(np.uint32), inner[:max_iter]
            return o
        s = _host(src, self.DIM)
        n = s.shape[0]
        # (the reference returns the transform alone: the last correspondences are copied back only on request --
        # 113 KB and a stream synchronisation per 28k-point frame otherwise)
        want_idx = bool(return_info) and return_info != "inner"
        idx = np.zeros(max(n, 1), dtype=np.uint32) if want_idx else None
        check(lib().icp_estimate(self._h, _ptr(s), n, C.byref(initial_transform.pose), max_iter,
                                 C.byref(o.pose), C.c_void_p(idx.ctypes.data) if want_idx else None,
                                 C.c_void_p(inner.ctypes.data)), "icp_estimate")
        if return_info == "inner":
            return o, inner[:max_iter]
        if return_info:
            return o, idx[:n], inner[:max_iter]
        return o

    def _estimate_gated(self, src, initial_transform, max_iter, return_info, r):
        """estimate() with a maximum correspondence distance: icp_estimate_gated[_device]."""
        if not r >= 0.0:  # (also a NaN)
            raise ValueError(f"max_correspondence_distance must be >= 0 (or +inf), got {r}")
        o = Transform()
        inner = np.zeros(max(max_iter, 1), dtype=np.uint32)
        inl = np.zeros(max(max_iter, 1), dtype=np.uint32)
        want_idx = bool(return_info) and return_info != "inner"
        if _is_device_tensor(src):
            import torch

            self._dev(src, "src")
            n = src.shape[0]
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=src.device) if want_idx else None
            check(lib().icp_estimate_gated_device(self._h, C.c_void_p(src.data_ptr()), n,
                                                  C.byref(initial_transform.pose), max_iter, r, C.byref(o.pose),
                                                  C.c_void_p(idx.data_ptr()) if want_idx else None,
                                                  C.c_void_p(inner.ctypes.data), C.c_void_p(inl.ctypes.data)),
                  "icp_estimate_gated_device")
            if want_idx:
                idx = idx[:n].cpu().numpy().view(np.uint32)
        else:
            s = _host(src, self.DIM)
            n = s.shape[0]
            idx = np.zeros(max(n, 1), dtype=np.uint32) if want_idx else None
            check(lib().icp_estimate_gated(self._h, _ptr(s), n, C.byref(initial_transform.pose), max_iter, r,
                                           C.byref(o.pose), C.c_void_p(idx.ctypes.data) if want_idx else None,
                                           C.c_void_p(inner.ctypes.data), C.c_void_p(inl.ctypes.data)),
                  "icp_estimate_gated")
            if want_idx:
                idx = idx[:n]
        if return_info == "inner":
            return o, inner[:max_iter], inl[:max_iter]
        if return_info:
            return o, idx, inner[:max_iter], inl[:max_iter]
        return o

    def gate_pairs_device(self, d_src, transform, d_idx, max_correspondence_distance, d_a, d_b, d_kept=None):
        """The gate alone (icp_gate_pairs_device): the pairs of the points with d2 <= r * r, dense and in the
        order of d_src, into d_a / d_b (n x 2); d_kept (optional, n words) receives their positions.  Returns
        their number."""
        self._dev(d_src, "src")
        n = d_src.shape[0]
        _dev_index(d_idx, n, self._device, "d_idx")
        for t, what in ((d_a, "d_a"), (d_b, "d_b")):
            _dev_points(t, 2, self._device, what)
            if t.shape[0] < n:
                raise ValueError(f"{what}: holds {t.shape[0]} pairs, {n} are needed")
        if d_kept is not None:
            _dev_index(d_kept, n, self._device, "d_kept")
        kept = C.c_size_t(0)
        check(lib().icp_gate_pairs_device(self._h, C.c_void_p(d_src.data_ptr()), n, C.byref(transform.pose),
                                          C.c_void_p(d_idx.data_ptr()), float(max_correspondence_distance),
                                          C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr()),
                                          C.c_void_p(d_kept.data_ptr()) if d_kept is not None else None,
                                          C.byref(kept)), "icp_gate_pairs_device")
        return int(kept.value)

    # -- EXTENSION (not in the reference): the quality of a pose, include/icp_mi355x.h section 9 --
    def evaluate(self, src, transform, max_correspondence_distance=float("inf"), return_indices=False):
        """The Quality of `transform` (icp_evaluate[_device]): the handle's exact correspondences at that pose, the
        inliers within max_correspondence_distance, the reference's error / huber_error and the SE(2) information
        matrix.  The handle's registration state is left as it was.  return_indices=True also returns the
        correspondences (caller order).  numpy arrays or contiguous float64 CUDA tensors (used in place)."""
        return self._evaluate(_lib.QualityStruct, Quality, "icp_evaluate", src, transform,
                              max_correspondence_distance, return_indices)

    def _evaluate(self, struct, wrap, symbol, src, transform, r, return_indices):
        """evaluate, evaluate_point_to_plane and evaluate_point_to_line behind their guards: `symbol` (host arrays) or
        `symbol`_device (device tensors) fills a `struct`, returned as a `wrap`"""
        q, r = struct(), float(r)
        if _is_device_tensor(src):
            import torch

            self._dev(src, "src")
            n = src.shape[0]
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=src.device) if return_indices else None
            check(getattr(lib(), symbol + "_device")(self._h, C.c_void_p(src.data_ptr()), n, C.byref(transform.pose), r,
                                                     C.byref(q), C.c_void_p(idx.data_ptr()) if return_indices else None),
                  symbol + "_device")
            return (wrap(q), idx[:n].cpu().numpy().view(np.uint32)) if return_indices else wrap(q)
        s = _host(src, self.DIM)
        n = s.shape[0]
        idx = np.zeros(max(n, 1), dtype=np.uint32) if return_indices else None
        check(getattr(lib(), symbol)(self._h, _ptr(s), n, C.byref(transform.pose), r, C.byref(q),
                                     C.c_void_p(idx.ctypes.data) if return_indices else None), symbol)
        return (wrap(q), idx[:n]) if return_indices else wrap(q)

    def set_single_launch(self, enable=True):
        """small clouds: whole estimate in one launch (default on); off = the general host-driven path"""
        check(lib().icp_set_single_launch(self._h, int(bool(enable))), "icp_set_single_launch")

    def single_launch_counters(self):
        out = (C.c_uint64 * 3)()
        check(lib().icp_single_launch_counters(self._h, out), "icp_single_launch_counters")
        return tuple(int(x) for x in out)

    # -- stage-level access (device tensors), used by the sharded driver and the bench --
    def set_stream(self, stream_ptr):
        check(lib().icp_set_stream(self._h, C.c_void_p(stream_ptr)), "icp_set_stream")
        self._own_stream = False

    def use_own_stream(self):
        check(lib().icp_use_own_stream(self._h), "icp_use_own_stream")
        self._own_stream = True

    def correspond_device(self, d_src, transform, d_a, d_b, d_idx=None):
        n = self._dev(d_src, "d_src").shape[0]
        for t, what in ((d_a, "d_a"), (d_b, "d_b")):
            if t is not None and self._dev_pairs(t, what).shape[0] < n:
                raise ValueError(f"{what}: needs {n} rows")
        if d_idx is not None:
            _dev_index(d_idx, n, self._device, "d_idx")
        check(lib().icp_correspond_device(self._h, C.c_void_p(d_src.data_ptr()), d_src.shape[0],
                                          C.byref(transform.pose),
                                          C.c_void_p(d_a.data_ptr()) if d_a is not None else None,
                                          C.c_void_p(d_b.data_ptr()) if d_b is not None else None,
                                          C.c_void_p(d_idx.data_ptr()) if d_idx is not None else None),
              "icp_correspond_device")

    def materialize_pairs_device(self, d_src, transform, d_idx, d_a, d_b):
        n = self._dev(d_src, "d_src").shape[0]
        _dev_index(d_idx, n, self._device, "d_idx")
        for t, what in ((d_a, "d_a"), (d_b, "d_b")):
            if self._dev_pairs(t, what).shape[0] < n:
                raise ValueError(f"{what}: needs {n} rows")
        check(lib().icp_materialize_pairs_device(self._h, C.c_void_p(d_src.data_ptr()), d_src.shape[0],
                                                 C.byref(transform.pose), C.c_void_p(d_idx.data_ptr()),
                                                 C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr())),
              "icp_materialize_pairs_device")

    def prepare_source_device(self, d_src, transform):
        self._dev(d_src, "d_src")
        check(lib().icp_prepare_source_device(self._h, C.c_void_p(d_src.data_ptr()), d_src.shape[0],
                                              C.byref(transform.pose)), "icp_prepare_source_device")

    def estimate_transform_device(self, d_a, d_b):
        if self._dev_pairs(d_a, "d_a").shape[0] != self._dev_pairs(d_b, "d_b").shape[0]:
            raise ValueError("d_a and d_b differ in length")  # debug_assert_eq!, src/lib.rs:223
        o = Transform()
        inner = C.c_uint32(0)
        check(lib().icp_estimate_transform_device(self._h, C.c_void_p(d_a.data_ptr()),
                                                  C.c_void_p(d_b.data_ptr()), d_a.shape[0],
                                                  C.byref(o.pose), C.byref(inner)),
              "icp_estimate_transform_device")
        return o, inner.value

    def nn_search_device(self, d_q, d_idx):
        _dev_index(d_idx, self._dev(d_q, "d_q").shape[0], self._device, "d_idx")
        check(lib().icp_nn_search_device(self._h, C.c_void_p(d_q.data_ptr()), d_q.shape[0],
                                         C.c_void_p(d_idx.data_ptr())), "icp_nn_search_device")

    def nn_search(self, q):
        """exact NN indices of host points (test/observability helper)."""
        import torch

        qq = torch.from_numpy(_host(q, self.DIM)).cuda()
        idx = torch.empty(max(qq.shape[0], 1), dtype=torch.int32, device=qq.device)
        self.nn_search_device(qq, idx)
        self.synchronize()
        return idx[: qq.shape[0]].cpu().numpy().view(np.uint32)

    # -- EXTENSION (not in the reference): a target cloud that grows, for scan-to-map ------
    def append(self, points, transform=None):
        """Append `points` to the target cloud, moved by `transform` first if given (exactly
        Transform::transform on xy, z kept).  Afterwards the handle behaves like a fresh
        Icp*::new on the concatenated cloud (include/icp_mi355x.h section 6)."""
        tp = C.byref(transform.pose) if transform is not None else None
        if _is_device_tensor(points):
            self._dev(points, "points")
            check(lib().icp_append_targets_device(self._h, C.c_void_p(points.data_ptr()), points.shape[0], tp),
                  "icp_append_targets_device")
        else:
            p = _host(points, self.DIM)
            check(lib().icp_append_targets(self._h, _ptr(p), p.shape[0], tp), "icp_append_targets")
        self._keep = None  # the cloud now lives in the handle's own storage
        self.m = self.target_count

    def append_counters(self):
        """(appends served by moving the search grid's sorted records, appends that rebuilt the grid)"""
        out = (C.c_uint64 * 2)()
        check(lib().icp_grid_append_counters(self._h, out), "icp_grid_append_counters")
        return int(out[0]), int(out[1])

    def crop(self, center, radius, return_index=False):
        """Keep the targets inside the xy disc of `radius` around `center` (two values: a caller crops around
        transform.t) and remove the others (icp_crop_targets, include/icp_mi355x.h section 11): target i is kept iff
        (x - cx)^2 + (y - cy)^2 <= radius^2.  The kept targets keep their order and their normals; afterwards the
        handle behaves like a fresh Icp*::new on the kept cloud.  Returns the number of targets removed; with
        return_index=True also new_index (uint32, one per old target: its new index, 0xffffffff if removed)."""
        c = _vec(center, 2)
        r = float(radius)
        if not r >= 0.0 or np.isnan(c).any():  # (also a NaN radius)
            raise ValueError(f"crop needs a centre without NaN and a radius >= 0 (or +inf), got {c.tolist()}, {r}")
        m_before = self.target_count
        index = np.zeros(max(m_before, 1), dtype=np.uint32) if return_index else None
        removed = C.c_size_t(0)
        check(lib().icp_crop_targets(self._h, c.ctypes.data_as(_dp), r,
                                     C.c_void_p(index.ctypes.data) if return_index else None, C.byref(removed)),
              "icp_crop_targets")
        if removed.value:
            self._keep = None  # the kept cloud lives in the handle's own storage
        self.m = self.target_count
        return (int(removed.value), index[:m_before]) if return_index else int(removed.value)

    def crop_counters(self):
        """(crops served by moving the search grid's sorted records, crops that rebuilt the grid)"""
        out = (C.c_uint64 * 2)()
        check(lib().icp_grid_crop_counters(self._h, out), "icp_grid_crop_counters")
        return int(out[0]), int(out[1])

    def thin(self, voxel_size, return_index=False):
        """Keep the first target of every voxel of size `voxel_size` and remove the others (icp_thin_targets,
        include/icp_mi355x.h section 22; the rule is voxel_downsample's).  Like crop: the kept targets keep their
        order and their normals, and afterwards the handle behaves like a fresh Icp*::new on the kept cloud.  Returns
        the number of targets removed; with return_index=True also new_index (uint32, one per old target: its new
        index, 0xffffffff if removed)."""
        v = _voxel_size(voxel_size)
        m_before = self.target_count
        index = np.zeros(max(m_before, 1), dtype=np.uint32) if return_index else None
        removed = C.c_size_t(0)
        check(lib().icp_thin_targets(self._h, v, C.c_void_p(index.ctypes.data) if return_index else None,
                                     C.byref(removed)), "icp_thin_targets")
        if removed.value:
            self._keep = None  # the kept cloud lives in the handle's own storage
        self.m = self.target_count
        return (int(removed.value), index[:m_before]) if return_index else int(removed.value)

    def thin_counters(self):
        """(thins served by moving the search grid's sorted records, thins that rebuilt the grid)"""
        out = (C.c_uint64 * 2)()
        check(lib().icp_grid_thin_counters(self._h, out), "icp_grid_thin_counters")
        return int(out[0]), int(out[1])

    # -- EXTENSION (not in the reference): neighbour lists and outlier removal, include/icp_mi355x.h section 23 --
    def neighbours(self, k, first=0, count=None):
        """(idx uint32, d2 float64), both (count, k): for each target of [first, first + count) its min(k, m) nearest
        targets, itself included, ordered by (d^2, index); rows padded with 0xffffffff / +inf (icp_target_neighbours)."""
        k = _list_length(k, 32)
        count = self.target_count - first if count is None else int(count)
        idx = np.empty((max(count, 0), k), dtype=np.uint32)
        d2 = np.empty((max(count, 0), k), dtype=np.float64)
        check(lib().icp_target_neighbours(self._h, k, int(first), count, _ptr(idx), _ptr(d2)), "icp_target_neighbours")
        return idx, d2

    def _removal(self, entry, call, return_index):
        m_before = self.target_count
        index = np.zeros(max(m_before, 1), dtype=np.uint32) if return_index else None
        removed = C.c_size_t(0)
        check(call(C.c_void_p(index.ctypes.data) if return_index else None, C.byref(removed)), entry)
        if removed.value:
            self._keep = None  # the kept cloud lives in the handle's own storage
        self.m = self.target_count
        return int(removed.value), (index[:m_before] if return_index else None)

    def remove_radius_outliers(self, radius, min_neighbours, return_index=False):
        """Remove the targets with fewer than `min_neighbours` targets, themselves included, within `radius` (d^2 <=
        radius * radius; icp_remove_radius_outliers).  Like crop: order and normals are kept and the handle then
        behaves like a fresh one on the kept cloud.  Returns the number removed; with return_index=True also new_index."""
        r, need = _radius_rule(radius, min_neighbours)
        removed, index = self._removal("icp_remove_radius_outliers",
                                       lambda ix, rm: lib().icp_remove_radius_outliers(self._h, r, need, ix, rm),
                                       return_index)
        return (removed, index) if return_index else removed

    def remove_statistical_outliers(self, k=16, std_ratio=2.0, return_index=False, return_stats=False):
        """Remove the targets whose mean distance to their k nearest other targets exceeds mean + std_ratio * deviation
        of that figure over all targets (icp_remove_statistical_outliers).  Returns the number removed, then new_index
        (return_index) and (mean, deviation, threshold) (return_stats) where asked for."""
        kk, ratio = _statistical_rule(k, std_ratio)
        stats = (C.c_double * 3)()
        removed, index = self._removal(
            "icp_remove_statistical_outliers",
            lambda ix, rm: lib().icp_remove_statistical_outliers(self._h, kk, ratio, ix, rm, stats), return_index)
        out = (removed,) + ((index,) if return_index else ()) + ((tuple(float(s) for s in stats),) if return_stats else ())
        return out if len(out) > 1 else removed

    def outlier_counters(self):
        """(outlier filters served by moving the search grid's sorted records, filters that rebuilt the grid)"""
        out = (C.c_uint64 * 2)()
        check(lib().icp_grid_outlier_counters(self._h, out), "icp_grid_outlier_counters")
        return int(out[0]), int(out[1])

    # -- EXTENSION (not in the reference): queries of arbitrary points and removal by mask, icp_mi355x.h section 24 --
    def _query_points(self, points, what="points"):
        """(pointer, n, on_device, device) of a query cloud: a contiguous float64 CUDA tensor goes to the device
        entries, anything else through numpy to the host entries"""
        if _is_device_tensor(points):
            self._dev(points, what)
            return C.c_void_p(points.data_ptr() if points.shape[0] else None), points.shape[0], True, points.device, points
        p = _host(points, self.DIM)
        return _ptr(p), p.shape[0], False, None, p

    def query(self, points, k, transform=None):
        """(idx uint32, d2 float64), both (n, k): for each of the n `points`, moved by `transform` first if given
        (Transform::transform on xy, z kept), its min(k, m) nearest targets by (d^2, index); rows padded with
        0xffffffff / +inf; a point with a NaN coordinate gets padding only (icp_query_neighbours[_device]).  numpy in
        gives numpy out; a contiguous float64 CUDA tensor gives CUDA tensors (idx as int32 bits)."""
        k = _list_length(k, 32)
        ptr, n, on_device, device, keep = self._query_points(points)
        tp = C.byref(transform.pose) if transform is not None else None
        if on_device:
            import torch

            idx = torch.empty((n, k), dtype=torch.int32, device=device)
            d2 = torch.empty((n, k), dtype=torch.float64, device=device)
            check(lib().icp_query_neighbours_device(self._h, ptr, n, tp, k, C.c_void_p(idx.data_ptr() if n else None),
                                                    C.c_void_p(d2.data_ptr() if n else None)),
                  "icp_query_neighbours_device")
            if self._own_stream:
                self.synchronize()  # (torch's streams are not ordered behind the handle's private one)
            return idx, d2
        idx = np.empty((n, k), dtype=np.uint32)
        d2 = np.empty((n, k), dtype=np.float64)
        check(lib().icp_query_neighbours(self._h, ptr, n, tp, k, _ptr(idx), _ptr(d2)), "icp_query_neighbours")
        return idx, d2

    def count_within(self, points, radius, transform=None, cap=None):
        """uint32 (n,): for each of `points` (moved by `transform` first if given) the number of targets with d^2 <=
        radius * radius, at most `cap` (None: the full count; a count stops at cap, which keeps a large radius cheap).
        points=None: the targets themselves, in index order (then no transform); `count_within(None, r, cap=n) >= n`
        is the keep rule of remove_radius_outliers(r, n) (icp_count_within[_device])."""
        r, cp = _count_rule(radius, cap)
        if points is None:
            if transform is not None:
                raise ValueError("count_within(None, ...) counts around the targets themselves: no transform")
            n = self.target_count
            counts = np.empty(n, dtype=np.uint32)
            check(lib().icp_count_within(self._h, None, n, None, r, cp, _ptr(counts)), "icp_count_within")
            return counts
        ptr, n, on_device, device, keep = self._query_points(points)
        tp = C.byref(transform.pose) if transform is not None else None
        if n == 0 and not on_device:  # (no points have no address, and to the C entry no address means "the targets")
            return np.empty(0, dtype=np.uint32)
        if on_device:
            import torch

            counts = torch.empty(n, dtype=torch.int32, device=device)
            if n == 0:
                return counts
            check(lib().icp_count_within_device(self._h, ptr, n, tp, r, cp, C.c_void_p(counts.data_ptr() if n else None)),
                  "icp_count_within_device")
            if self._own_stream:
                self.synchronize()
            return counts
        counts = np.empty(n, dtype=np.uint32)
        check(lib().icp_count_within(self._h, ptr, n, tp, r, cp, _ptr(counts)), "icp_count_within")
        return counts

    def remove(self, keep, return_index=False):
        """Remove the targets i with keep[i] == 0 (`keep`: one value per target, anything numpy reads as a truth value,
        or a CUDA bool / uint8 tensor; icp_remove_targets[_device]).  Like crop: order and normals are kept and the
        handle then behaves like a fresh one on the kept cloud.  Returns the number removed; with return_index=True also
        new_index (uint32, one per old target: its new index, 0xffffffff if removed)."""
        if _is_device_tensor(keep):
            if keep.dim() != 1 or keep.element_size() != 1 or keep.dtype.is_floating_point or not keep.is_contiguous():
                raise ValueError(f"keep: expected a contiguous 1-D bool / uint8 CUDA tensor, got {tuple(keep.shape)} "
                                 f"{keep.dtype}")
            if self._device is not None and keep.device.index != self._device:
                raise ValueError(f"keep: tensor lives on cuda:{keep.device.index}, the handle on cuda:{self._device}")
            if keep.shape[0] != self.target_count:
                raise ValueError(f"keep: expected {self.target_count} values, got {keep.shape[0]}")
            self._after_producer(keep)
            entry, arg = "icp_remove_targets_device", C.c_void_p(keep.data_ptr())
        else:
            mask = np.asarray(keep)
            if mask.ndim != 1:
                raise ValueError(f"keep: expected one value per target, got shape {mask.shape}")
            mask = np.ascontiguousarray(mask != 0, dtype=np.uint8)
            if mask.shape[0] != self.target_count:
                raise ValueError(f"keep: expected {self.target_count} values, got {mask.shape[0]}")
            entry, arg = "icp_remove_targets", C.c_void_p(mask.ctypes.data)
        if self.target_count == 0:  # (nothing to remove, and an empty mask has no address to hand over)
            return (0, np.zeros(0, dtype=np.uint32)) if return_index else 0
        removed, index = self._removal(entry, lambda ix, rm: getattr(lib(), entry)(self._h, arg, ix, rm), return_index)
        return (removed, index) if return_index else removed

    def remove_counters(self):
        """(removals by mask served by moving the search grid's sorted records, removals that rebuilt the grid)"""
        out = (C.c_uint64 * 2)()
        check(lib().icp_grid_remove_counters(self._h, out), "icp_grid_remove_counters")
        return int(out[0]), int(out[1])

    def query_counters(self):
        """(query / count calls whose lanes ran in cell order, calls served in the caller's order)"""
        out = (C.c_uint64 * 2)()
        check(lib().icp_query_counters(self._h, out), "icp_query_counters")
        return int(out[0]), int(out[1])

    def reserve(self, capacity):
        check(lib().icp_reserve_targets(self._h, int(capacity)), "icp_reserve_targets")
        self._keep = None if capacity > self.m else self._keep

    @property
    def target_count(self):
        return int(lib().icp_target_count(self._h))

    def read_targets(self, first=0, count=None):
        count = self.target_count - first if count is None else count
        out = np.empty((count, self.DIM), dtype=np.float64)
        check(lib().icp_read_targets(self._h, first, count, C.c_void_p(out.ctypes.data)), "icp_read_targets")
        return out

    # -- EXTENSION (not in the reference): point-to-plane residuals, include/icp_mi355x.h section 7 --
    def compute_normals(self, k=10):
        """Unit normals of the target points from their k nearest targets (3-D handles)."""
        check(lib().icp_compute_target_normals(self._h, int(k)), "icp_compute_target_normals")

    def update_normals(self, k=10):
        """Normals for the targets appended since compute_normals / update_normals (from the cloud as it is
        now); the older targets keep theirs."""
        check(lib().icp_update_target_normals(self._h, int(k)), "icp_update_target_normals")

    def read_normals(self, first=0, count=None):
        count = self.target_count - first if count is None else count
        out = np.empty((count, 3), dtype=np.float64)
        check(lib().icp_read_target_normals(self._h, first, count, C.c_void_p(out.ctypes.data)),
              "icp_read_target_normals")
        return out

    def estimate_point_to_plane(self, src, initial_transform, max_iter, return_info=False,
                                max_correspondence_distance=None):
        """Icp3d::estimate with the residual n_q . (T p - q) (extension; needs compute_normals()).

        `max_correspondence_distance=r` (include/icp_mi355x.h section 12): the inner loop of each outer iteration sees
        only the pairs whose nearest target lies within r of the moved source point (d2 <= r * r, evaluate's inlier
        rule), in the caller's order; `return_info` then returns (T, idx, inner, inliers).  None: the ungated call."""
        return self._estimate_normal("icp_estimate_point_to_plane", src, initial_transform, max_iter, return_info,
                                     max_correspondence_distance)

    def _estimate_normal(self, stem, src, initial_transform, max_iter, return_info, bound):
        """the four entries `stem`[_gated][_device] of a registration under a normal residual (plane or line)"""
        gated = bound is not None
        r = float(bound) if gated else 0.0
        if gated and not r >= 0.0:  # (also a NaN)
            raise ValueError(f"max_correspondence_distance must be >= 0 (or +inf), got {bound!r}")
        o = Transform()
        inner = np.zeros(max(max_iter, 1), dtype=np.uint32)
        inl = np.zeros(max(max_iter, 1), dtype=np.uint32)
        on_device = _is_device_tensor(src)
        if on_device:
            import torch

            self._dev(src, "src")
            n = src.shape[0]
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=src.device) if return_info else None
            sp, ip = C.c_void_p(src.data_ptr()), (C.c_void_p(idx.data_ptr()) if return_info else None)
        else:
            s = _host(src, self.DIM)
            n = s.shape[0]
            idx = np.zeros(max(n, 1), dtype=np.uint32)
            sp, ip = _ptr(s), C.c_void_p(idx.ctypes.data)
        name = stem + ("_gated" if gated else "") + ("_device" if on_device else "")
        args = [self._h, sp, n, C.byref(initial_transform.pose), max_iter] + ([r] if gated else [])
        args += [C.byref(o.pose), ip, C.c_void_p(inner.ctypes.data)] + ([C.c_void_p(inl.ctypes.data)] if gated else [])
        check(getattr(lib(), name)(*args), name)
        if not return_info:
            return o
        idx = idx[:n].cpu().numpy().view(np.uint32) if on_device else idx[:n]
        return (o, idx, inner[:max_iter], inl[:max_iter]) if gated else (o, idx, inner[:max_iter])

    # -- EXTENSION (not in the reference): the quality of a pose under the plane residual, section 13 --
    def evaluate_point_to_plane(self, src, transform, max_correspondence_distance=float("inf"), return_indices=False):
        """The PlaneQuality of `transform` (icp_evaluate_point_to_plane[_device]; 3-D handles, needs current normals):
        the handle's exact correspondences at that pose, the inliers within max_correspondence_distance, the plane
        residual's RMSE, error / huber_error and the SE(2) information matrix it gives.  The handle's registration
        state is left as it was.  return_indices=True also returns the correspondences (caller order).  numpy arrays or
        contiguous float64 CUDA tensors (used in place)."""
        if self.DIM != 3:
            raise ValueError("evaluate_point_to_plane needs a 3-D handle (Icp3d): a 2-D cloud has no normals")
        return self._evaluate(_lib.PlaneQualityStruct, PlaneQuality, "icp_evaluate_point_to_plane", src, transform,
                              max_correspondence_distance, return_indices)

    def gate_plane_pairs_device(self, d_src, transform, d_idx, r, d_pairs, d_kept=None):
        """The gate of a gated point-to-plane registration alone (icp_gate_plane_pairs_device): for the inliers of the
        search result `d_idx` at `transform`, in the order of d_src, the eight doubles of a pair (ax, ay, qx, qy, dz, nx,
        ny, nz) in d_pairs (n x 8 float64) and their source positions in d_kept (n int32, optional).  Returns their
        number."""
        import torch

        r = float(r)
        if not r >= 0.0:
            raise ValueError(f"the bound must be >= 0 (or +inf), got {r!r}")
        n = self._dev(d_src, "d_src").shape[0]
        _dev_index(d_idx, n, self._device, "d_idx")
        if not (_is_device_tensor(d_pairs) and d_pairs.dtype == torch.float64 and d_pairs.is_contiguous()
                and d_pairs.dim() == 2 and d_pairs.shape[1] == 8 and d_pairs.shape[0] >= n
                and d_pairs.device.index == self._device):
            raise ValueError(f"d_pairs: needs a contiguous float64 device tensor of at least {n} x 8 on the handle's device")
        if d_kept is not None:
            _dev_index(d_kept, n, self._device, "d_kept")
        kept = C.c_size_t(0)
        check(lib().icp_gate_plane_pairs_device(self._h, C.c_void_p(d_src.data_ptr()), n, C.byref(transform.pose),
                                                C.c_void_p(d_idx.data_ptr()), r, C.c_void_p(d_pairs.data_ptr()),
                                                C.c_void_p(d_kept.data_ptr()) if d_kept is not None else None,
                                                C.byref(kept)), "icp_gate_plane_pairs_device")
        return int(kept.value)

    # -- EXTENSION (not in the reference): point-to-line residuals for 2-D handles, include/icp_mi355x.h section 14 --
    def _need_2d(self, what):
        if self.DIM != 2:
            raise ValueError(f"{what} needs a 2-D handle (Icp2d); a 3-D handle registers with compute_normals() / "
                             "estimate_point_to_plane()")

    def compute_line_normals(self, k=10):
        """Unit line normals of the target points from their k nearest targets (2-D handles)."""
        self._need_2d("compute_line_normals")
        check(lib().icp_compute_target_line_normals(self._h, int(k)), "icp_compute_target_line_normals")

    def update_line_normals(self, k=10):
        """Line normals for the targets appended since compute_line_normals / update_line_normals (from the cloud as
        it is now); the older targets keep theirs."""
        self._need_2d("update_line_normals")
        check(lib().icp_update_target_line_normals(self._h, int(k)), "icp_update_target_line_normals")

    def read_line_normals(self, first=0, count=None):
        self._need_2d("read_line_normals")
        count = self.target_count - first if count is None else count
        out = np.empty((count, 2), dtype=np.float64)
        check(lib().icp_read_target_line_normals(self._h, first, count, C.c_void_p(out.ctypes.data)),
              "icp_read_target_line_normals")
        return out

    def estimate_point_to_line(self, src, initial_transform, max_iter, return_info=False,
                               max_correspondence_distance=None):
        """Icp2d::estimate with the residual n_q . (T p - q), n_q the line normal of the matched target (extension;
        needs compute_line_normals()).  Returns what estimate_point_to_plane returns: the Transform, with
        return_info=True (T, idx, inner).

        `max_correspondence_distance=r`: the inner loop of each outer iteration sees only the pairs whose nearest
        target lies within r of the moved source point (d2 <= r * r), in the caller's order; `return_info` then returns
        (T, idx, inner, inliers).  None: the ungated call."""
        self._need_2d("estimate_point_to_line")
        return self._estimate_normal("icp_estimate_point_to_line", src, initial_transform, max_iter, return_info,
                                     max_correspondence_distance)

    # -- EXTENSION (not in the reference): the quality of a pose under the line residual, section 16 --
    def evaluate_point_to_line(self, src, transform, max_correspondence_distance=float("inf"), return_indices=False):
        """The LineQuality of `transform` (icp_evaluate_point_to_line[_device]; 2-D handles, needs current line
        normals): the handle's exact correspondences at that pose, the inliers within max_correspondence_distance, the
        line residual's RMSE, error / huber_error and the SE(2) information matrix it gives.  The handle's registration
        state is left as it was.  return_indices=True also returns the correspondences (caller order).  numpy arrays or
        contiguous float64 CUDA tensors (used in place)."""
        self._need_2d("evaluate_point_to_line")
        return self._evaluate(_lib.LineQualityStruct, LineQuality, "icp_evaluate_point_to_line", src, transform,
                              max_correspondence_distance, return_indices)

    def profile_enable(self, every=1):
        """Time every `every`-th NN search launch with HIP events (0 / False: off)."""
        check(lib().icp_profile_enable(self._h, int(every)), "icp_profile_enable")

    def profile_read(self):
        """(summed NN-kernel device time in ms, launches) since the last read."""
        ms, k = C.c_double(), C.c_uint64()
        check(lib().icp_profile_read(self._h, C.byref(ms), C.byref(k)), "icp_profile_read")
        return ms.value, k.value

    def synchronize(self):
        check(lib().icp_synchronize(self._h), "icp_synchronize")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().icp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Icp2d(_Icp):
    """`icp::Icp2d` (src/lib.rs:91-131)."""

    DIM = 2


class Icp3d(_Icp):
    """`icp::Icp3d` (src/lib.rs:133-174): 3-D nearest neighbours, SE(2) pose on the xy-plane."""

    DIM = 3


class IcpMulti:
    """Icp{2,3}d over several GPUs from one process (icp_create_multi): same result as one GPU, bit for
    bit.  `device_ids` may repeat a device (virtual ranks)."""

    def __init__(self, dst, device_ids, dim=3):
        self.dim = dim
        d = _host(dst, dim)
        ids = (C.c_int * len(device_ids))(*[int(x) for x in device_ids])
        self._h = C.c_void_p()
        check(lib().icp_create_multi(C.byref(self._h), dim, _ptr(d), d.shape[0], ids, len(device_ids)),
              "icp_create_multi")

    def estimate(self, src, initial_transform, max_iter, return_info=False):
        s = _host(src, self.dim)
        n = s.shape[0]
        o = Transform()
        idx = np.zeros(max(n, 1), dtype=np.uint32)
        inner = np.zeros(max(max_iter, 1), dtype=np.uint32)
        check(lib().icp_multi_estimate(self._h, _ptr(s), n, C.byref(initial_transform.pose), max_iter, C.byref(o.pose),
                                       C.c_void_p(idx.ctypes.data), C.c_void_p(inner.ctypes.data)), "icp_multi_estimate")
        return (o, idx[:n], inner[:max_iter]) if return_info else o

    def append(self, points, transform=None):
        """EXTENSION (icp_multi_append_targets): every rank appends the points, moved by `transform`, to its replica of
        the target cloud"""
        p = _host(points, self.dim)
        check(lib().icp_multi_append_targets(self._h, _ptr(p), p.shape[0],
                                             C.byref(transform.pose) if transform is not None else None),
              "icp_multi_append_targets")

    def crop(self, center, radius):
        """EXTENSION (icp_multi_crop_targets): every rank crops its replica of the target cloud to the xy disc;
        returns the number of targets removed"""
        c = _vec(center, 2)
        removed = C.c_size_t(0)
        check(lib().icp_multi_crop_targets(self._h, c.ctypes.data_as(_dp), float(radius), C.byref(removed)),
              "icp_multi_crop_targets")
        return int(removed.value)

    def thin(self, voxel_size):
        """EXTENSION (icp_multi_thin_targets): every rank thins its replica of the target cloud to one target per
        voxel; returns the number of targets removed"""
        removed = C.c_size_t(0)
        check(lib().icp_multi_thin_targets(self._h, _voxel_size(voxel_size), C.byref(removed)),
              "icp_multi_thin_targets")
        return int(removed.value)

    @property
    def target_count(self):
        return int(lib().icp_multi_target_count(self._h))

    def counters(self):
        out = (C.c_uint64 * 2)()
        check(lib().icp_multi_counters(self._h, out), "icp_multi_counters")
        return int(out[0]), int(out[1])

    def compute_target_normals(self, k=8):
        """EXTENSION (icp_multi_compute_target_normals): every rank computes the normals of its replica of the target cloud"""
        check(lib().icp_multi_compute_target_normals(self._h, int(k)), "icp_multi_compute_target_normals")

    def update_target_normals(self, k=8):
        check(lib().icp_multi_update_target_normals(self._h, int(k)), "icp_multi_update_target_normals")

    def estimate_point_to_plane(self, src, initial_transform, max_iter, return_info=False,
                                max_correspondence_distance=None):
        """EXTENSION (icp_multi_estimate_point_to_plane): search sharded over the ranks, inner loop replicated.
        `max_correspondence_distance=r` (icp_multi_estimate_point_to_plane_gated): every rank gates the whole cloud
        first; `return_info` then returns (T, idx, inner, inliers)"""
        if max_correspondence_distance is not None:
            r = float(max_correspondence_distance)
            if not r >= 0.0:  # (also a NaN)
                raise ValueError(f"max_correspondence_distance must be >= 0 (or +inf), got {max_correspondence_distance!r}")
        s = _host(src, 3)
        n = s.shape[0]
        o = Transform()
        idx = np.zeros(max(n, 1), dtype=np.uint32)
        inner = np.zeros(max(max_iter, 1), dtype=np.uint32)
        if max_correspondence_distance is not None:
            inl = np.zeros(max(max_iter, 1), dtype=np.uint32)
            check(lib().icp_multi_estimate_point_to_plane_gated(self._h, _ptr(s), n, C.byref(initial_transform.pose),
                                                                max_iter, r, C.byref(o.pose), C.c_void_p(idx.ctypes.data),
                                                                C.c_void_p(inner.ctypes.data), C.c_void_p(inl.ctypes.data)),
                  "icp_multi_estimate_point_to_plane_gated")
            return (o, idx[:n], inner[:max_iter], inl[:max_iter]) if return_info else o
        check(lib().icp_multi_estimate_point_to_plane(self._h, _ptr(s), n, C.byref(initial_transform.pose), max_iter,
                                                      C.byref(o.pose), C.c_void_p(idx.ctypes.data), C.c_void_p(inner.ctypes.data)),
              "icp_multi_estimate_point_to_plane")
        return (o, idx[:n], inner[:max_iter]) if return_info else o

    def loop_counters(self):
        """(launches per rank, evaluations served, launches that handed an evaluation back) of the one-launch inner loop"""
        out = (C.c_uint64 * 3)()
        check(lib().icp_multi_loop_counters(self._h, out), "icp_multi_loop_counters")
        return tuple(int(x) for x in out)

    def pipe_iterations(self):
        """outer iterations served by the pipelined sharded evaluation (csrc/pipe.hip) over the life of the object"""
        out = C.c_uint64(0)
        check(lib().icp_multi_pipe_iterations(self._h, C.byref(out)), "icp_multi_pipe_iterations")
        return int(out.value)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().icp_destroy_multi(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IcpBatch:
    """Many small registrations in one call (icp_batch_*, include/icp_mi355x.h section 8) -- an extension beyond the
    reference, which registers one pair per Icp{2,3}d::estimate.  Item i's result is what
    Icp{2,3}d(dst_i).estimate(src_i, init_i, max_iter) returns on its own handle, bit for bit; items of up to 1024
    source and 2048 target points run as one workgroup each of a single launch, larger ones one by one.  One call in
    flight per object."""

    def __init__(self, dim, device=-1):
        if dim not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        self.DIM = dim
        self._device = device if device >= 0 else None
        self._b = C.c_void_p()
        check(lib().icp_batch_create(C.byref(self._b), dim, device), "icp_batch_create")

    def _pack(self, clouds, what):
        """one array for all clouds; an entry that is the same object as an earlier one is packed once and shared"""
        seen, parts, firsts, counts, at = {}, [], [], [], 0
        for c in clouds:
            if id(c) not in seen:
                a = _host(c, self.DIM)
                seen[id(c)] = (at, a.shape[0])
                parts.append(a)
                at += a.shape[0]
            f, k = seen[id(c)]
            firsts.append(f)
            counts.append(k)
        packed = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, self.DIM))
        return packed, firsts, counts

    def _pack_items(self, srcs, dsts, inits):
        """what the calls over lists of clouds hand to their *_packed twins: (src, dst, items)"""
        srcs, dsts = list(srcs), list(dsts)
        if len(srcs) != len(dsts):
            raise ValueError(f"{len(srcs)} source clouds for {len(dsts)} target clouds")
        src, sf, sn = self._pack(srcs, "src")
        dst, df, dm = self._pack(dsts, "dst")
        return src, dst, list(zip(sf, sn, df, dm, self._inits(inits, len(srcs))))

    @staticmethod
    def _inits(inits, count):
        if inits is None:
            return [Transform() for _ in range(count)]
        if isinstance(inits, Transform):
            return [inits] * count
        inits = list(inits)
        if len(inits) != count:
            raise ValueError(f"{len(inits)} initial transforms for {count} items")
        return inits

    @staticmethod
    def _bound(max_correspondence_distance):
        """the gated entries' max_dist, or None for the ungated ones; refused here, before the library is reached"""
        if max_correspondence_distance is None:
            return None
        r = float(max_correspondence_distance)
        if not r >= 0.0:  # (also a NaN)
            raise ValueError(f"max_correspondence_distance must be >= 0 (or +inf), got {max_correspondence_distance!r}")
        return r

    def estimate(self, srcs, dsts, inits, max_iter, return_info=False, allow_failures=False,
                 max_correspondence_distance=None):
        """Register srcs[i] against dsts[i] from inits[i] (a list, one Transform for all, or None: identity).  Returns
        the list of Transforms; with return_info also the per-item indices, the inner counts (count x max_iter) and the
        statuses.  A failed item raises IcpError naming it, unless allow_failures=True (its Transform is then None).

        `max_correspondence_distance=r` (icp_batch_estimate_gated*, section 21): item i is what
        Icp{2,3}d(dsts[i]).estimate(srcs[i], inits[i], max_iter, max_correspondence_distance=r) returns, bit for bit --
        the inner loop of each outer iteration sees only the pairs within r; `return_info` then returns (Ts, idxs,
        inner, status, inliers), inliers count x max_iter.  None: the ungated call."""
        src, dst, items = self._pack_items(srcs, dsts, inits)
        return self.estimate_packed(src, dst, items, max_iter, return_info, allow_failures, max_correspondence_distance)

    def estimate_packed(self, src, dst, items, max_iter, return_info=False, allow_failures=False,
                        max_correspondence_distance=None):
        """The same over pre-packed clouds: `items` = [(src_first, n, dst_first, m, init Transform), ...] ranges of
        `src` / `dst` (ranges may overlap).  numpy arrays go through icp_batch_estimate[_gated]; contiguous float64 CUDA
        tensors through icp_batch_estimate[_gated]_device, in place."""
        return self._estimate_packed(src, dst, items, max_iter, return_info, allow_failures, None,
                                     self._bound(max_correspondence_distance))

    def _estimate_packed(self, src, dst, items, max_iter, return_info, allow_failures, line_k, max_dist=None,
                         normals_entry="icp_batch_estimate_point_to_line"):
        """estimate_packed (line_k None), estimate_point_to_line_packed (line_k = the normals' neighbours) and
        estimate_point_to_plane_packed (normals_entry: its entry, which takes the same arguments); max_dist: the gated
        entries of each, which also fill the inlier counts"""
        count = len(items)
        name = "icp_batch_estimate" if line_k is None else normals_entry
        name = what = name + ("" if max_dist is None else "_gated")
        kargs = [] if line_k is None else [int(line_k)]
        gargs = [] if max_dist is None else [float(max_dist)]
        arr = (_lib.BatchItem * max(count, 1))()
        for i, (f, n, g, m, T) in enumerate(items):
            arr[i].src_first, arr[i].n, arr[i].dst_first, arr[i].m = int(f), int(n), int(g), int(m)
            C.memmove(C.byref(arr[i].init), C.byref(T.pose), C.sizeof(Pose))
        out = (Pose * max(count, 1))()
        status = np.zeros(max(count, 1), dtype=np.int32)
        inner = np.zeros(max(count * max_iter, 1), dtype=np.uint32)
        inl = np.zeros(max(count * max_iter, 1), dtype=np.uint32)
        iargs = [] if max_dist is None else [C.c_void_p(inl.ctypes.data)]
        total = sum(int(it[1]) for it in items)
        want_idx = bool(return_info)
        if _is_device_tensor(src) or _is_device_tensor(dst):
            import torch

            if self._device is None:
                self._device = src.device.index
            _dev_points(src, self.DIM, self._device, "src")
            _dev_points(dst, self.DIM, self._device, "dst")
            for t in (src, dst):  # (the batch's own stream is not ordered against the producer's)
                torch.cuda.current_stream(t.device).synchronize()
            idx = torch.zeros(max(total, 1), dtype=torch.int32, device=src.device) if want_idx else None
            name += "_device"
            check(getattr(lib(), name)(self._b, C.c_void_p(src.data_ptr()), src.shape[0], C.c_void_p(dst.data_ptr()),
                                       dst.shape[0], arr, count, *kargs, max_iter, *gargs, out,
                                       C.c_void_p(status.ctypes.data), C.c_void_p(idx.data_ptr()) if want_idx else None,
                                       C.c_void_p(inner.ctypes.data), *iargs), name)
            idx = idx.cpu().numpy().view(np.uint32) if want_idx else None
        else:
            s, d = _host(src, self.DIM), _host(dst, self.DIM)
            idx = np.zeros(max(total, 1), dtype=np.uint32) if want_idx else None
            check(getattr(lib(), name)(self._b, _ptr(s), s.shape[0], _ptr(d), d.shape[0], arr, count, *kargs, max_iter,
                                       *gargs, out, C.c_void_p(status.ctypes.data),
                                       C.c_void_p(idx.ctypes.data) if want_idx else None,
                                       C.c_void_p(inner.ctypes.data), *iargs), name)
        status = status[:count]
        Ts = []
        for i in range(count):
            if status[i] != _lib.OK:
                if not allow_failures:
                    raise IcpError(int(status[i]), f"{what} item {i}")
                Ts.append(None)
            else:
                Ts.append(Transform.from_pose(out[i]))
        if not return_info:
            return Ts
        idxs, at = [], 0
        for it in items:
            idxs.append(idx[at:at + int(it[1])])
            at += int(it[1])
        info = (Ts, idxs, inner[:count * max_iter].reshape(count, max_iter), status)
        return info if max_dist is None else info + (inl[:count * max_iter].reshape(count, max_iter),)

    def estimate_hypotheses(self, src, dst, inits, max_iter, max_correspondence_distance=None):
        """One scan against one map from K initial poses (one shared src range and dst range: nothing is copied per
        hypothesis).  Returns (Transforms, errors): errors[k] is huber_error of the k-th result on its last
        correspondences (src/lib.rs:45-50, xy of the points), so that the caller can keep the best hypothesis.
        (evaluate() scores poses on the device instead, on the correspondences AT each returned pose.)
        `max_correspondence_distance=r`: every hypothesis is registered with the gate (estimate_packed); the errors are
        scored as without it, on the last correspondences of all points."""
        s, d = _host(src, self.DIM), _host(dst, self.DIM)
        inits = self._inits(inits, len(inits) if not isinstance(inits, Transform) else 1)
        items = [(0, s.shape[0], 0, d.shape[0], T) for T in inits]
        Ts, idxs = self.estimate_packed(s, d, items, max_iter, return_info=True,
                                        max_correspondence_distance=max_correspondence_distance)[:2]
        a = np.ascontiguousarray(s[:, :2])
        errs = [huber_error(T, a, np.ascontiguousarray(d[ix.astype(np.int64), :2])) for T, ix in zip(Ts, idxs)]
        return Ts, np.array(errs)

    # -- EXTENSION: the same with the point-to-line residual (icp_batch_estimate_point_to_line*, section 15) --
    def _need_2d(self, what):
        if self.DIM != 2:
            raise ValueError(f"{what} needs a 2-D batch (IcpBatch(2)): the line residual is section 14's, for 2-D scans")

    def estimate_point_to_line(self, srcs, dsts, inits, max_iter, k=10, return_info=False, allow_failures=False,
                               max_correspondence_distance=None):
        """estimate() with the point-to-line residual: item i is what Icp2d(dsts[i]) returns after
        compute_line_normals(k) from estimate_point_to_line(srcs[i], inits[i], max_iter), bit for bit; items of up to
        1024 source and 2048 target points run as one workgroup each (normals included), the others one by one.

        `max_correspondence_distance=r` (icp_batch_estimate_point_to_line_gated*, section 17): item i is what that
        single call returns with the same r -- the inner loop of each outer iteration sees only the pairs within r;
        `return_info` then returns (Ts, idxs, inner, status, inliers), inliers count x max_iter.  None: the ungated call."""
        self._need_2d("estimate_point_to_line")
        src, dst, items = self._pack_items(srcs, dsts, inits)
        return self.estimate_point_to_line_packed(src, dst, items, max_iter, k, return_info, allow_failures,
                                                  max_correspondence_distance)

    def estimate_point_to_line_packed(self, src, dst, items, max_iter, k=10, return_info=False, allow_failures=False,
                                      max_correspondence_distance=None):
        """The same over pre-packed clouds (`items` as for estimate_packed; K hypotheses share one src and one dst range).
        numpy arrays go through icp_batch_estimate_point_to_line[_gated]; contiguous float64 CUDA tensors through
        icp_batch_estimate_point_to_line[_gated]_device, in place."""
        self._need_2d("estimate_point_to_line_packed")
        if not 3 <= int(k) <= 16:
            raise ValueError(f"k must be in [3, 16], got {k!r}")
        return self._estimate_packed(src, dst, items, max_iter, return_info, allow_failures, int(k),
                                     self._bound(max_correspondence_distance))

    # -- EXTENSION: the same with the point-to-plane residual for 3-D items (icp_batch_estimate_point_to_plane*,
    # section 18) --
    def _need_3d(self, what):
        if self.DIM != 3:
            raise ValueError(f"{what} needs a 3-D batch (IcpBatch(3)): the plane residual is for 3-D clouds")

    def estimate_point_to_plane(self, srcs, dsts, inits, max_iter, k=10, return_info=False, allow_failures=False,
                                max_correspondence_distance=None):
        """estimate() with the point-to-plane residual: item i is what Icp3d(dsts[i]) returns after compute_normals(k)
        from estimate_point_to_plane(srcs[i], inits[i], max_iter), bit for bit; items of up to 1024 source and 2048
        target points run as one workgroup each (normals included), the others one by one.

        `max_correspondence_distance=r` (icp_batch_estimate_point_to_plane_gated*, section 19): item i is what that
        single call returns with the same r -- the inner loop of each outer iteration sees only the pairs within r (3-D
        distance); `return_info` then returns (Ts, idxs, inner, status, inliers), inliers count x max_iter.  None: the
        ungated call."""
        self._need_3d("estimate_point_to_plane")
        src, dst, items = self._pack_items(srcs, dsts, inits)
        return self.estimate_point_to_plane_packed(src, dst, items, max_iter, k, return_info, allow_failures,
                                                   max_correspondence_distance)

    def estimate_point_to_plane_packed(self, src, dst, items, max_iter, k=10, return_info=False, allow_failures=False,
                                       max_correspondence_distance=None):
        """The same over pre-packed clouds (`items` as for estimate_packed; K hypotheses share one src and one dst range).
        numpy arrays go through icp_batch_estimate_point_to_plane[_gated]; contiguous float64 CUDA tensors through
        icp_batch_estimate_point_to_plane[_gated]_device, in place."""
        self._need_3d("estimate_point_to_plane_packed")
        if not 3 <= int(k) <= 16:
            raise ValueError(f"k must be in [3, 16], got {k!r}")
        return self._estimate_packed(src, dst, items, max_iter, return_info, allow_failures, int(k),
                                     self._bound(max_correspondence_distance), "icp_batch_estimate_point_to_plane")

    def plane_counters(self):
        """(items served in a batch launch, items served one by one, launches, launches not made for want of LDS) of
        estimate_point_to_plane*"""
        out = (C.c_uint64 * 4)()
        check(lib().icp_batch_plane_counters(self._b, out), "icp_batch_plane_counters")
        return tuple(int(x) for x in out)

    def plane_gated_counters(self):
        """(items served in a batch launch, items served one by one, launches, launches not made for want of LDS) of
        estimate_point_to_plane*(..., max_correspondence_distance=r)"""
        out = (C.c_uint64 * 4)()
        check(lib().icp_batch_plane_gated_counters(self._b, out), "icp_batch_plane_gated_counters")
        return tuple(int(x) for x in out)

    def line_counters(self):
        """(items served in a batch launch, items served one by one, launches, launches not made for want of LDS) of
        estimate_point_to_line*"""
        out = (C.c_uint64 * 4)()
        check(lib().icp_batch_line_counters(self._b, out), "icp_batch_line_counters")
        return tuple(int(x) for x in out)

    def line_gated_counters(self):
        """(items served in a batch launch, items served one by one, launches, launches not made for want of LDS) of
        estimate_point_to_line*(..., max_correspondence_distance=r)"""
        out = (C.c_uint64 * 4)()
        check(lib().icp_batch_line_gated_counters(self._b, out), "icp_batch_line_gated_counters")
        return tuple(int(x) for x in out)

    # -- the quality of many poses in one call (icp_batch_evaluate*, include/icp_mi355x.h section 9) --
    def evaluate(self, srcs, dsts, transforms, max_correspondence_distance=float("inf"), allow_failures=False,
                 return_status=False):
        """The Quality of transforms[i] for srcs[i] against dsts[i] (a list, one Transform for all, or None: identity):
        item i equals Icp{2,3}d(dsts[i]).evaluate(srcs[i], transforms[i], max_correspondence_distance), bit for bit.
        A failed item raises IcpError naming it, unless allow_failures=True (its Quality is then None);
        return_status=True also returns the statuses."""
        src, dst, items = self._pack_items(srcs, dsts, transforms)
        return self.evaluate_packed(src, dst, items, max_correspondence_distance, allow_failures, return_status)

    def evaluate_packed(self, src, dst, items, max_correspondence_distance=float("inf"), allow_failures=False,
                        return_status=False):
        """The same over pre-packed clouds: `items` = [(src_first, n, dst_first, m, Transform), ...] ranges of `src` /
        `dst` (ranges may overlap).  numpy arrays go through icp_batch_evaluate; contiguous float64 CUDA tensors through
        icp_batch_evaluate_device, in place."""
        return self._evaluate_packed(_lib.QualityStruct, Quality, "icp_batch_evaluate", src, dst, items, [],
                                     float(max_correspondence_distance), allow_failures, return_status)

    def _evaluate_packed(self, struct, wrap, symbol, src, dst, items, kargs, r, allow_failures, return_status):
        """evaluate_packed, evaluate_point_to_line_packed and evaluate_point_to_plane_packed (kargs: the normals'
        neighbours) behind their guards:
        `symbol` (host arrays) or `symbol`_device (device tensors) fills one `struct` per item, returned as `wrap`s"""
        count = len(items)
        arr = (_lib.BatchItem * max(count, 1))()
        for i, (f, n, g, m, T) in enumerate(items):
            arr[i].src_first, arr[i].n, arr[i].dst_first, arr[i].m = int(f), int(n), int(g), int(m)
            C.memmove(C.byref(arr[i].init), C.byref(T.pose), C.sizeof(Pose))
        out = (struct * max(count, 1))()
        status = np.zeros(max(count, 1), dtype=np.int32)
        if _is_device_tensor(src) or _is_device_tensor(dst):
            import torch

            if self._device is None:
                self._device = src.device.index
            _dev_points(src, self.DIM, self._device, "src")
            _dev_points(dst, self.DIM, self._device, "dst")
            for t in (src, dst):  # (the batch's own stream is not ordered against the producer's)
                torch.cuda.current_stream(t.device).synchronize()
            check(getattr(lib(), symbol + "_device")(self._b, C.c_void_p(src.data_ptr()), src.shape[0],
                                                     C.c_void_p(dst.data_ptr()), dst.shape[0], arr, count, *kargs, r,
                                                     out, C.c_void_p(status.ctypes.data)), symbol + "_device")
        else:
            s, d = _host(src, self.DIM), _host(dst, self.DIM)
            check(getattr(lib(), symbol)(self._b, _ptr(s), s.shape[0], _ptr(d), d.shape[0], arr, count, *kargs, r, out,
                                         C.c_void_p(status.ctypes.data)), symbol)
        status = status[:count]
        qs = []
        for i in range(count):
            if status[i] != _lib.OK:
                if not allow_failures:
                    raise IcpError(int(status[i]), f"{symbol} item {i}")
                qs.append(None)
            else:
                qs.append(wrap(out[i]))
        return (qs, status) if return_status else qs

    # -- the same under the point-to-line residual (icp_batch_evaluate_point_to_line*, section 16) --
    def evaluate_point_to_line(self, srcs, dsts, transforms, k=10, max_correspondence_distance=float("inf"),
                               allow_failures=False, return_status=False):
        """The LineQuality of transforms[i] for srcs[i] against dsts[i] (a list, one Transform for all, or None:
        identity): item i equals what Icp2d(dsts[i]) returns after compute_line_normals(k) from
        evaluate_point_to_line(srcs[i], transforms[i], max_correspondence_distance), bit for bit; items of up to 1024
        source and 2048 target points run as one workgroup each of a single launch (normals included), the others one
        by one.  A failed item raises IcpError naming it, unless allow_failures=True (its LineQuality is then None);
        return_status=True also returns the statuses."""
        self._need_2d("evaluate_point_to_line")
        src, dst, items = self._pack_items(srcs, dsts, transforms)
        return self.evaluate_point_to_line_packed(src, dst, items, k, max_correspondence_distance, allow_failures,
                                                  return_status)

    def evaluate_point_to_line_packed(self, src, dst, items, k=10, max_correspondence_distance=float("inf"),
                                      allow_failures=False, return_status=False):
        """The same over pre-packed clouds (`items` as for evaluate_packed; K hypotheses share one src and one dst
        range).  numpy arrays go through icp_batch_evaluate_point_to_line; contiguous float64 CUDA tensors through
        icp_batch_evaluate_point_to_line_device, in place."""
        self._need_2d("evaluate_point_to_line_packed")
        if not 3 <= int(k) <= 16:
            raise ValueError(f"k must be in [3, 16], got {k!r}")
        r = float(max_correspondence_distance)
        if not r >= 0.0:  # (also a NaN)
            raise ValueError(f"max_correspondence_distance must be >= 0 (or +inf), got {max_correspondence_distance!r}")
        return self._evaluate_packed(_lib.LineQualityStruct, LineQuality, "icp_batch_evaluate_point_to_line", src, dst,
                                     items, [int(k)], r, allow_failures, return_status)

    def line_quality_counters(self):
        """(items scored in a batch launch, items scored one by one, launches, launches not made for want of LDS) of
        evaluate_point_to_line*"""
        out = (C.c_uint64 * 4)()
        check(lib().icp_batch_line_quality_counters(self._b, out), "icp_batch_line_quality_counters")
        return tuple(int(x) for x in out)

    # -- the same under the point-to-plane residual for 3-D items (icp_batch_evaluate_point_to_plane*, section 20) --
    def evaluate_point_to_plane(self, srcs, dsts, transforms, k=10, max_correspondence_distance=float("inf"),
                                allow_failures=False, return_status=False):
        """The PlaneQuality of transforms[i] for srcs[i] against dsts[i] (a list, one Transform for all, or None:
        identity): item i equals what Icp3d(dsts[i]) returns after compute_normals(k) from
        evaluate_point_to_plane(srcs[i], transforms[i], max_correspondence_distance), bit for bit; items of up to 1024
        source and 2048 target points run as one workgroup each of a single launch (normals included), the others one
        by one.  A failed item raises IcpError naming it, unless allow_failures=True (its PlaneQuality is then None);
        return_status=True also returns the statuses."""
        self._need_3d("evaluate_point_to_plane")
        src, dst, items = self._pack_items(srcs, dsts, transforms)
        return self.evaluate_point_to_plane_packed(src, dst, items, k, max_correspondence_distance, allow_failures,
                                                   return_status)

    def evaluate_point_to_plane_packed(self, src, dst, items, k=10, max_correspondence_distance=float("inf"),
                                       allow_failures=False, return_status=False):
        """The same over pre-packed clouds (`items` as for evaluate_packed; K hypotheses share one src and one dst
        range).  numpy arrays go through icp_batch_evaluate_point_to_plane; contiguous float64 CUDA tensors through
        icp_batch_evaluate_point_to_plane_device, in place."""
        self._need_3d("evaluate_point_to_plane_packed")
        if not 3 <= int(k) <= 16:
            raise ValueError(f"k must be in [3, 16], got {k!r}")
        r = float(max_correspondence_distance)
        if not r >= 0.0:  # (also a NaN)
            raise ValueError(f"max_correspondence_distance must be >= 0 (or +inf), got {max_correspondence_distance!r}")
        return self._evaluate_packed(_lib.PlaneQualityStruct, PlaneQuality, "icp_batch_evaluate_point_to_plane", src, dst,
                                     items, [int(k)], r, allow_failures, return_status)

    def plane_quality_counters(self):
        """(items scored in a batch launch, items scored one by one, launches, launches not made for want of LDS) of
        evaluate_point_to_plane*"""
        out = (C.c_uint64 * 4)()
        check(lib().icp_batch_plane_quality_counters(self._b, out), "icp_batch_plane_quality_counters")
        return tuple(int(x) for x in out)

    def evaluate_counters(self):
        """(items evaluated in a batch launch, items evaluated one by one, launches)"""
        out = (C.c_uint64 * 3)()
        check(lib().icp_batch_evaluate_counters(self._b, out), "icp_batch_evaluate_counters")
        return tuple(int(x) for x in out)

    def gated_counters(self):
        """(items served in a batch launch, items served one by one, launches, launches not made for want of LDS) of
        estimate*(..., max_correspondence_distance=r)"""
        out = (C.c_uint64 * 4)()
        check(lib().icp_batch_gated_counters(self._b, out), "icp_batch_gated_counters")
        return tuple(int(x) for x in out)

    def counters(self):
        """(items served in a batch launch, items served one by one, launches, launches not made for want of LDS)"""
        out = (C.c_uint64 * 4)()
        check(lib().icp_batch_counters(self._b, out), "icp_batch_counters")
        return tuple(int(x) for x in out)

    def close(self):
        if getattr(self, "_b", None) is not None and self._b.value:
            lib().icp_batch_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
