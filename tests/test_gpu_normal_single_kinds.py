"""The single-handle entries of the two normal residuals -- point-to-line on a 2-D handle, point-to-plane on a 3-D one --
whose kernels and host paths share one body per piece (csrc/normal_single_device.hpp, gate_plane.hip, api_normal.hip):
the normals, the gather, the gate, the outer loop, the staging of a host cloud and the handle check.  One body of tests
runs for both dimensions, bit for bit, at the sizes where a shared piece can go wrong where two copies could not: n
around the workspace floor (256) and the gate's tile (1 024), m around the normals kernel's workgroup (64 lanes) and below
k, k at both ends of its range.  No cloud here has a NaN coordinate: the two dimensions treat those differently today
(DESIGN.md section 9q)."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_rust_amd as I
from icp_rust_amd import _lib
from test_gpu_normal_batch_kinds import bits, corner, scan

pytestmark = pytest.mark.gpu

INF = float("inf")
NS = (1, 2, 255, 256, 257, 1023, 1024, 1025)
MS = (3, 64, 65, 300)
KS = (3, 16)
MAX_ITER = 2
DIMS = (2, 3)


def fresh(dim, dst, k=None):
    icp = (I.Icp2d if dim == 2 else I.Icp3d)(dst)
    if k is not None:
        compute(icp, k)
    return icp


def compute(icp, k):
    icp.compute_line_normals(k) if icp.DIM == 2 else icp.compute_normals(k)


def update(icp, k):
    icp.update_line_normals(k) if icp.DIM == 2 else icp.update_normals(k)


def read(icp):
    return icp.read_line_normals() if icp.DIM == 2 else icp.read_normals()


def estimate(icp, src, T, max_iter, r=None):
    """[pose bits, last indices, inner counts (, inliers)]"""
    f = icp.estimate_point_to_line if icp.DIM == 2 else icp.estimate_point_to_plane
    got = f(src, T, max_iter, return_info=True, max_correspondence_distance=r)
    return [bits(got[0].as_array())] + [np.asarray(a) for a in got[1:]]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def clouds():
    """{dim: ({m: targets}, {n: scan of the 300 targets})}, made once and left unchanged"""
    out = {}
    for dim in DIMS:
        rng = np.random.default_rng(8000 + dim)
        dsts = {m: corner(rng, dim, m) for m in MS}
        out[dim] = (dsts, {n: scan(rng, dsts[300], n) for n in NS})
    return out


@pytest.mark.parametrize("dim", DIMS)
def test_host_entry_equals_device_entry_and_a_gate_at_infinity_equals_no_gate(dim, clouds):
    dsts, srcs = clouds[dim]
    T = I.Transform([0.01, -0.02, 0.005])
    for m in MS:
        for k in KS:
            icp = fresh(dim, dsts[m], k)
            for n in NS:
                src = srcs[n]
                d_src = torch.from_numpy(src).cuda()
                host = estimate(icp, src, T, MAX_ITER)
                assert len(host[1]) == n and len(host[2]) == MAX_ITER and host[1].max() < m
                assert same(host, estimate(icp, d_src, T, MAX_ITER)), (m, k, n)
                for s in (src, d_src):
                    gated = estimate(icp, s, T, MAX_ITER, INF)
                    assert same(gated[:3], host), (m, k, n)
                    assert gated[3].tolist() == [n] * MAX_ITER, (m, k, n, gated[3])
            icp.close()


@pytest.mark.parametrize("dim", DIMS)
def test_no_iteration_and_clouds_of_no_and_one_point_return_the_initial_pose(dim, clouds):
    dsts, srcs = clouds[dim]
    T = I.Transform([0.3, -0.2, 0.1])
    want = bits(T.as_array())
    for m, k in ((3, 3), (65, 16)):
        icp = fresh(dim, dsts[m], k)
        for r in (None, INF, 0.5):
            for n in (0, 1, 257):
                src = srcs[n] if n else np.zeros((0, dim))
                for s in (src, torch.from_numpy(src).cuda()):
                    got = estimate(icp, s, T, 0, r)
                    assert np.array_equal(got[0], want) and len(got[2]) == 0, (m, k, r, n)
                    if n <= 1:  # fewer than two pairs: check_input_size, no update in any iteration
                        got = estimate(icp, s, T, 3, r)
                        assert np.array_equal(got[0], want) and got[2].tolist() == [0, 0, 0], (m, k, r, n, got)
        icp.close()


@pytest.mark.parametrize("dim", DIMS)
def test_after_an_append_the_update_keeps_the_old_rows_and_gives_the_new_ones_a_fresh_handles_bits(dim, clouds):
    """tests/test_gpu_line.py's statement (test_after_an_append_the_normals_are_stale_...), for both dimensions: the older
    rows are kept bit for bit; the appended rows come from their neighbours in the cloud as it is NOW -- which is what a
    fresh handle on the concatenated cloud computes for those rows, and only for those"""
    dsts, srcs = clouds[dim]
    for m, extra_m, k in ((64, 65, 3), (65, 3, 16), (300, 64, 16), (3, 300, 3)):
        dst = dsts[m]
        extra = np.ascontiguousarray(dsts[extra_m] + 0.01)
        icp = fresh(dim, dst, k)
        before = read(icp)
        icp.append(extra)
        for r in (None, 0.5):
            with pytest.raises(I.IcpError) as e:  # the appended targets have no normal yet
                estimate(icp, srcs[257], I.Transform(), 1, r)
            assert e.value.status == _lib.BAD_ARGUMENT
        with pytest.raises(I.IcpError):
            read(icp)
        with pytest.raises(I.IcpError) as e:  # one neighbourhood size per cloud
            update(icp, k + 1)
        assert e.value.status == _lib.BAD_ARGUMENT
        update(icp, k)
        got = read(icp)
        assert got.shape == (m + extra_m, dim)
        assert np.array_equal(bits(got[:m]), bits(before)), (m, extra_m, k)
        whole = fresh(dim, np.concatenate([dst, extra]), k)
        assert np.array_equal(bits(got[m:]), bits(read(whole)[m:])), (m, extra_m, k)
        whole.close()
        assert estimate(icp, srcs[257], I.Transform(), 1)[1].max() < m + extra_m  # usable again
        icp.close()


@pytest.mark.parametrize("dim", DIMS)
def test_a_handle_of_the_other_dimension_is_refused_by_every_entry(dim, clouds):
    """the entries of dimension `dim` on a handle of the other one: ICP_BAD_ARGUMENT from each, before anything runs"""
    other = 5 - dim
    dsts, _ = clouds[other]
    L = I.lib()
    stem = "icp_estimate_point_to_line" if dim == 2 else "icp_estimate_point_to_plane"
    word = "line_" if dim == 2 else ""
    n = 4
    src = np.ascontiguousarray(np.random.default_rng(8100).uniform(-1.0, 1.0, (n, dim)))
    d_src = torch.from_numpy(src).cuda()
    d_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_pairs = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    T, out = I.Transform().pose, _lib.Pose()
    idx, inner, inl = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    ip, np_, lp = (C.c_void_p(a.ctypes.data) for a in (idx, inner, inl))
    buf = np.zeros((300, 3))
    for with_normals in (False, True):
        icp = fresh(other, dsts[65], 8 if with_normals else None)
        h = icp._h
        assert getattr(L, f"icp_compute_target_{word}normals")(h, 8) == _lib.BAD_ARGUMENT
        assert getattr(L, f"icp_update_target_{word}normals")(h, 8) == _lib.BAD_ARGUMENT
        rc = getattr(L, f"icp_read_target_{word}normals")(h, 0, 65, C.c_void_p(buf.ctypes.data))
        if dim == 3 and with_normals:
            # section 7's read never asks for the dimension: it hands out the stored m x 3 rows, a line normal and +0.0
            assert rc == _lib.OK
            assert np.array_equal(bits(buf[:65, :2]), bits(icp.read_line_normals()))
            assert np.array_equal(bits(buf[:65, 2]), bits(np.zeros(65)))
        else:
            assert rc == _lib.BAD_ARGUMENT
        for s, li in ((C.c_void_p(src.ctypes.data), ip), (C.c_void_p(d_src.data_ptr()), C.c_void_p(d_idx.data_ptr()))):
            dev = "" if li is ip else "_device"
            assert getattr(L, stem + dev)(h, s, n, C.byref(T), 1, C.byref(out), li, np_) == _lib.BAD_ARGUMENT
            assert getattr(L, stem + "_gated" + dev)(h, s, n, C.byref(T), 1, 0.5, C.byref(out), li, np_, lp) == \
                _lib.BAD_ARGUMENT
        if dim == 3:
            kept = C.c_size_t(7)
            assert L.icp_gate_plane_pairs_device(h, C.c_void_p(d_src.data_ptr()), n, C.byref(T),
                                                 C.c_void_p(d_idx.data_ptr()), 0.5, C.c_void_p(d_pairs.data_ptr()), None,
                                                 C.byref(kept)) == _lib.BAD_ARGUMENT
            assert kept.value == 0
        icp.close()
