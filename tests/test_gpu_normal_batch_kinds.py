"""The six batch entries whose kernels share one body per kind (csrc/normal_batch_device.hpp): the point-to-line and the
point-to-plane estimate, each plain and gated, and the two pose qualities.  Every item equals, bit for bit, what the
single calls return on a fresh handle -- Icp2d(dst_i) + compute_line_normals(k) for a 2-D item, Icp3d(dst_i) +
compute_normals(k) for a 3-D one, then the entry's single estimate or evaluation -- at the smallest shapes at which a body
written once for both dimensions can go wrong where two copies could not: one point against one target; two fold blocks
against targets that are no multiple of 64; k clamped to the targets; a NaN in a target's LAST coordinate (the 2-D body
must not look for a third one), which hands the item back to the single calls; and for the gated entries a bound that
keeps no pair, one that keeps exactly one, and +inf, which is the ungated entry.  No expected status or figure is
invented here: the single calls give them."""
import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib

pytestmark = pytest.mark.gpu

INF = float("inf")
MAX_ITER = 4
ENTRIES = ("line", "line_gated", "plane", "plane_gated", "line_quality", "plane_quality")


def dim_of(entry):
    return 2 if entry.startswith("line") else 3


def gated(entry):
    return entry.endswith("_gated")


def quality(entry):
    return entry.endswith("_quality")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ------------------------------------------------------------------ the single calls and the batch, in one shape

def single(entry, dst, src, T, k, r):
    """(status, [arrays]) of the single calls on a fresh handle; r: the bound (None: the ungated estimate)"""
    icp = None
    try:
        icp = (I.Icp2d if dim_of(entry) == 2 else I.Icp3d)(dst)
        if dim_of(entry) == 2:
            icp.compute_line_normals(k)
        else:
            icp.compute_normals(k)
        if quality(entry):
            q = (icp.evaluate_point_to_line if dim_of(entry) == 2 else icp.evaluate_point_to_plane)(src, T, r)
            return _lib.OK, [np.array([q.n, q.inliers], dtype=np.uint64), bits(q.as_array())]
        estimate = icp.estimate_point_to_line if dim_of(entry) == 2 else icp.estimate_point_to_plane
        got = estimate(src, T, MAX_ITER, return_info=True, max_correspondence_distance=r)
        return _lib.OK, [bits(got[0].as_array())] + [np.asarray(a) for a in got[1:]]
    except I.IcpError as e:
        return e.status, None
    finally:
        if icp is not None:
            icp.close()


def batch(entry, B, items, k, r):
    """[(status, [arrays])] per item of one batch call, in single()'s shape, and how the entry's counters moved"""
    srcs, dsts, Ts = (list(x) for x in zip(*items))
    name = {"line": "line_counters", "line_gated": "line_gated_counters", "plane": "plane_counters",
            "plane_gated": "plane_gated_counters", "line_quality": "line_quality_counters",
            "plane_quality": "plane_quality_counters"}[entry]
    before = getattr(B, name)()
    out = []
    if quality(entry):
        call = B.evaluate_point_to_line if dim_of(entry) == 2 else B.evaluate_point_to_plane
        qs, status = call(srcs, dsts, list(Ts), k, r, allow_failures=True, return_status=True)
        for q, st in zip(qs, status):
            out.append((int(st), None if q is None else [np.array([q.n, q.inliers], dtype=np.uint64), bits(q.as_array())]))
    else:
        call = B.estimate_point_to_line if dim_of(entry) == 2 else B.estimate_point_to_plane
        got = call(srcs, dsts, list(Ts), MAX_ITER, k, return_info=True, allow_failures=True, max_correspondence_distance=r)
        poses, idxs, inner, status = got[:4]
        for i in range(len(items)):
            if status[i] != _lib.OK:
                out.append((int(status[i]), None))
                continue
            arrays = [bits(poses[i].as_array()), idxs[i], inner[i]] + ([got[4][i]] if len(got) == 5 else [])
            out.append((int(status[i]), arrays))
    moved_by = tuple(a - b for a, b in zip(getattr(B, name)(), before))
    return out, moved_by


def assert_same(entry, items, k, r, got):
    for i, ((src, dst, T), (status, arrays)) in enumerate(zip(items, got)):
        want_status, want = single(entry, dst, src, T, k, r)
        assert status == want_status, (entry, i, status, want_status)
        if want is None:
            assert arrays is None, (entry, i)
            continue
        assert len(arrays) == len(want), (entry, i)
        for j, (a, b) in enumerate(zip(arrays, want)):
            assert np.array_equal(a, b), (entry, i, j, a, b)


# ------------------------------------------------------------------ the items

def corner(rng, dim, m):
    """m targets on two walls that meet in a corner (2-D: the lines x = 3 and y = -2; 3-D: the planes x = 3 and
    z = 0), 1 mm of noise: every neighbourhood of three or more has a normal"""
    a, b = rng.uniform(-2.0, 2.0, m), rng.uniform(0.0, 2.0, m)
    first = np.arange(m) % 2 == 0
    if dim == 2:
        dst = np.where(first[:, None], np.stack([np.full(m, 3.0), a], axis=1), np.stack([a + 1.0, np.full(m, -2.0)], axis=1))
    else:
        dst = np.where(first[:, None], np.stack([np.full(m, 3.0), a, b], axis=1), np.stack([a + 1.0, b - 2.0, np.zeros(m)], axis=1))
    return np.ascontiguousarray(dst + rng.normal(0.0, 1e-3, dst.shape))


def scan(rng, dst, n):
    """n targets drawn with replacement, 2 mm of noise, turned and shifted a little in the plane"""
    src = dst[rng.integers(0, len(dst), n)] + rng.normal(0.0, 2e-3, (n, dst.shape[1]))
    c, s = np.cos(0.01), np.sin(0.01)
    x, y = src[:, 0].copy(), src[:, 1].copy()
    src[:, 0], src[:, 1] = c * x - s * y + 0.02, s * x + c * y - 0.015
    return np.ascontiguousarray(src)


def shapes(dim):
    """[(src, dst, T)]: n = 1, m = 1; n = 513 (two fold blocks), m = 65 (mp = 128, two wavefronts of lists); a NaN in the
    last coordinate of one target"""
    rng = np.random.default_rng(7000 + dim)
    one = rng.uniform(-1.0, 1.0, (1, dim))
    dst = corner(rng, dim, 65)
    bad = corner(rng, dim, 40)
    bad[17, dim - 1] = np.nan
    T = I.Transform([0.01, -0.02, 0.005])
    return [(np.ascontiguousarray(one + 0.25), one, I.Transform()), (scan(rng, dst, 513), dst, T),
            (scan(rng, corner(rng, dim, 40), 30), bad, T)]


@pytest.fixture(scope="module")
def batches():
    made = {2: I.IcpBatch(2), 3: I.IcpBatch(3)}
    yield made
    for b in made.values():
        b.close()


def bound_of(entry):
    """the bound the shape tests run with: none for the plain estimate; one that splits the scan's pairs otherwise"""
    return None if not (gated(entry) or quality(entry)) else 0.004


# ------------------------------------------------------------------ the tests

@pytest.mark.parametrize("entry", ENTRIES)
def test_smallest_shapes_and_a_nan_in_the_last_coordinate_equal_the_single_calls(entry, batches):
    items = shapes(dim_of(entry))
    got, (served, one_by_one, launches, refused) = batch(entry, batches[dim_of(entry)], items, 3, bound_of(entry))
    assert_same(entry, items, 3, bound_of(entry), got)
    # the NaN target's item, and only that one, was handed back and served one by one: in the launch the 2-D body read
    # its y and no z, the 3-D body its z
    assert refused == 0 and launches >= 1 and (served, one_by_one) == (2, 1), (served, one_by_one, launches, refused)


@pytest.mark.parametrize("entry", ENTRIES)
def test_k_above_the_targets_is_clamped_to_them(entry, batches):
    dim = dim_of(entry)
    rng = np.random.default_rng(7100 + dim)
    dst = corner(rng, dim, 5)
    items = [(scan(rng, dst, 7), dst, I.Transform())]
    got, (served, one_by_one, _, refused) = batch(entry, batches[dim], items, 16, bound_of(entry))
    assert_same(entry, items, 16, bound_of(entry), got)
    assert (served, one_by_one, refused) == (1, 0, 0)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if gated(e)])
def test_gate_that_keeps_none_one_and_all(entry, batches):
    dim, B = dim_of(entry), batches[dim_of(entry)]
    rng = np.random.default_rng(7200 + dim)
    dst = corner(rng, dim, 65)
    T = I.Transform([0.01, -0.02, 0.005])
    # none: disjoint clouds under a bound of 0 -- the identity update, inlier counts 0
    far = [(np.ascontiguousarray(scan(rng, dst, 100) + 50.0), dst, T)]
    got, moved_by = batch(entry, B, far, 3, 0.0)
    assert_same(entry, far, 3, 0.0, got)
    assert got[0][0] == _lib.OK and not got[0][1][3].any() and not got[0][1][2].any() and moved_by[:2] == (1, 0)
    assert np.array_equal(got[0][1][0], bits(T.as_array()))
    # one: a single source point within millimetres of its target, the others 50 away; at the identity
    src = np.ascontiguousarray(scan(rng, dst, 100) + 50.0)
    src[41] = dst[9] + 1e-3
    lone = [(src, dst, I.Transform())]
    got, moved_by = batch(entry, B, lone, 3, 0.5)
    assert_same(entry, lone, 3, 0.5, got)
    assert got[0][0] == _lib.OK and (got[0][1][3] == 1).all() and moved_by[:2] == (1, 0), (got[0], moved_by)
    # all: +inf is the ungated entry's pose, indices and inner counts
    items = shapes(dim)[:2]
    got, _ = batch(entry, B, items, 3, INF)
    assert_same(entry, items, 3, INF, got)
    plain, _ = batch(entry[:-len("_gated")], B, items, 3, None)
    for (st, arrays), (pst, parrays), (src, _, _) in zip(got, plain, items):
        assert st == pst == _lib.OK
        for a, b in zip(arrays[:3], parrays):
            assert np.array_equal(a, b)
        assert (arrays[3] == len(src)).all()
