"""The scalar-residual estimators on the GPU -- point-to-plane (Icp3d.estimate_point_to_plane) and point-to-line
(Icp2d.estimate_point_to_line), their device-tensor and gated entries, the batched line kernel and the multi-rank plane
call -- against the CPU statement of the definition folded in the device's order
(parity_util.oracle_plane_in_device_order: orc_p2pl_estimate with sum_mode 1 and icp_reduce_geometry(n)).  In every
case status, pose bits, indices and inner counts are EQUAL; nothing is compared with another device call.  The oracle
is fed the device's normals (the normals kernels have their own tests: test_p2plane.py, test_gpu_line.py).

The scenes are those of tests/test_plane_reference.py, where the oracle's tree order is itself held to a long-double
witness and to a hand-written butterfly.  The sizes are the smallest at which each branch of reduce_geometry and of the
fold is taken: 2 and 3 (the least the estimator accepts, even and odd), 63/64/65 (a wave), 511/512/513 (one block to
two), 1 024/1 025 (the gate's tile), 131 072/131 073 (a thread folds a second pair), 2^20 and 2^20 + 1 (a block per
4 096 pairs)."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from parity_util import oracle_plane_in_device_order
from test_gpu_gated_plane import d2_of
from test_line_abi import lift
from test_p2plane import moved
from test_plane_reference import NORMALS_K, SCENES, bits, lifted, noisy_targets

pytestmark = pytest.mark.gpu

INF = float("inf")
SMALL = [2, 3, 63, 64, 65, 511, 512, 513, 1024, 1025]
ENTRY_SIZES = [65, 513, 1025]
FAMILY = {"noisy": "noisy", "far": "noisy", "ties": "walls", "sigma0": "walls", "heavy": "heavy"}  # scenes sharing targets
# the finite bound of a gated case: it removes some pairs and keeps others.  On the walls the bounds are distances that
# sources sit at exactly (d2 = r * r with nothing rounded: `<=` keeps them).  sigma0: 1/8, the tied run's own distance --
# the run and the sources nearer the wall stay, still more than half of them tied.  ties: 1/8 + 24/512 -- the run and
# all but the seven farthest steps stay, the run less than half of them.
# noisy: about the displacement of the scan under its true pose (3-D: (0.05, -0.04, 0.015); 2-D: (0.03, -0.02, 0.01)).
GATE = {(3, "noisy"): 0.06, (2, "noisy"): 0.03, "heavy": 0.25, "far": 0.25, "ties": 0.125 + 24.0 / 512.0, "sigma0": 0.125}


def gate(dim, scene):
    return GATE.get((dim, scene), GATE.get(scene))


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.set_threads(16)
    yield
    O.set_threads(1)


class Target:
    """a handle with its normals computed, the device's normals (lifted) and the oracle's kd-tree of the lifted targets"""

    def __init__(self, dim, dst):
        self.dim, self.dst = dim, dst
        self.icp = I.Icp3d(dst) if dim == 3 else I.Icp2d(dst)
        if dim == 3:
            self.icp.compute_normals(NORMALS_K)
            self.normals = self.icp.read_normals()
        else:
            self.icp.compute_line_normals(NORMALS_K)
            self.normals = lift(self.icp.read_line_normals())
        self.tree = O.KdTree(lifted(dim, dst))

    def estimate(self, src, init, iters, **kw):
        f = self.icp.estimate_point_to_plane if self.dim == 3 else self.icp.estimate_point_to_line
        return f(src, init, iters, return_info=True, **kw)

    def oracle(self, src, init, iters):
        return oracle_plane_in_device_order(self.icp, self.tree, self.normals, lifted(self.dim, src), init, iters)


@pytest.fixture(scope="module")
def targets():
    made = {}

    def get(dim, scene):
        key = (dim, FAMILY[scene])
        if key not in made:
            made[key] = Target(dim, SCENES[scene](dim, 2)[0])
        return made[key]

    yield get
    for t in made.values():
        t.icp.close()


def assert_equal_to_the_oracle(got, want, what):
    T, idx, inner = got[:3]
    rc, oT, oidx, oinner = want
    assert rc == O.OK, what
    assert np.array_equal(idx, oidx), what
    assert np.array_equal(inner, oinner), (what, inner.tolist(), oinner.tolist())
    assert np.array_equal(bits(T), bits(oT)), (what, T.as_array(), oT.as_array())


def check_premise(scene, n, init, oT, oinner):
    """what the scene is for, asserted on the ORACLE's run"""
    if scene == "sigma0":
        assert not oinner.any() and np.array_equal(bits(oT), bits(init))
    elif n >= 63:
        assert oinner.sum() > 0, (scene, n, oinner.tolist())


# ------------------------------------------------------------------ the host entries, every scene at every small size

@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("dim", [3, 2])
def test_small_sizes_equal_the_tree_oracle(targets, dim, scene, n):
    t = targets(dim, scene)
    dst, src, init = SCENES[scene](dim, n)
    assert np.array_equal(dst, t.dst)
    got = t.estimate(src, init, 4)
    want = t.oracle(src, init, 4)
    print(f"dim {dim} {scene} n={n}: inner {got[2].tolist()}")
    assert_equal_to_the_oracle(got, want, (dim, scene, n))
    check_premise(scene, n, init, want[1], want[3])


@pytest.mark.parametrize("n", [131_072, 131_073])
@pytest.mark.parametrize("scene", ["noisy", "ties"])
@pytest.mark.parametrize("dim", [3, 2])
def test_a_second_pair_per_thread_equals_the_tree_oracle(targets, dim, scene, n):
    assert I.reduce_geometry(n) == (256, 512)
    t = targets(dim, scene)
    _, src, init = SCENES[scene](dim, n)
    got = t.estimate(src, init, 2)
    want = t.oracle(src, init, 2)
    print(f"dim {dim} {scene} n={n}: inner {got[2].tolist()}")
    assert_equal_to_the_oracle(got, want, (dim, scene, n))
    check_premise(scene, n, init, want[1], want[3])


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 1])
@pytest.mark.parametrize("dim", [3, 2])
def test_past_2_to_the_20_equals_the_tree_oracle(targets, dim, n):
    """2^20: 256 blocks whose threads fold eight pairs; 2^20 + 1: a block per 4 096 pairs, 257 of them.  The sources
    are drawn with replacement from the same small room."""
    assert I.reduce_geometry(n)[0] == (256 if n == 1 << 20 else 257)
    t = targets(dim, "noisy")
    _, src, init = SCENES["noisy"](dim, n)
    got = t.estimate(src, init, 1)
    want = t.oracle(src, init, 1)
    print(f"dim {dim} noisy n={n}: inner {got[2].tolist()}")
    assert_equal_to_the_oracle(got, want, (dim, n))
    assert want[3].sum() > 0


# ------------------------------------------------------------------ degenerate inputs

@pytest.mark.parametrize("dim", [3, 2])
def test_degenerate_targets_and_sources_equal_the_tree_oracle(targets, dim):
    init = I.Transform([0.01, 0.02, 0.005])
    _, src, _ = SCENES["noisy"](dim, 65)
    # one and two targets: fewer than three neighbours, every normal is zero, every residual is zero, sigma is 0
    for m in (1, 2):
        t = Target(dim, np.ascontiguousarray(noisy_targets(dim)[:m]))
        try:
            assert not t.normals.any()
            got, want = t.estimate(src, init, 3), t.oracle(src, init, 3)
            assert_equal_to_the_oracle(got, want, (dim, "targets", m))
            assert not got[2].any() and np.array_equal(bits(got[0]), bits(init))
        finally:
            t.icp.close()
    t = targets(dim, "noisy")
    # no source point, and one: check_input_size -- no update
    for n in (0, 1):
        got, want = t.estimate(src[:n], init, 3), t.oracle(src[:n], init, 3)
        assert_equal_to_the_oracle(got, want, (dim, "sources", n))
        assert not got[2].any() and np.array_equal(bits(got[0]), bits(init))
    # a NaN in the source: the status on both sides
    bad = src.copy()
    bad[17, 1] = np.nan
    with pytest.raises(I.IcpError) as e:
        t.estimate(bad, init, 2)
    assert e.value.status == _lib.NAN_INPUT
    assert t.oracle(bad, init, 2)[0] == O.NAN


# ------------------------------------------------------------------ the device-tensor entry

@pytest.mark.parametrize("n", ENTRY_SIZES)
@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("dim", [3, 2])
def test_the_device_tensor_entry_equals_the_tree_oracle(targets, dim, scene, n):
    import torch

    t = targets(dim, scene)
    _, src, init = SCENES[scene](dim, n)
    got = t.estimate(torch.from_numpy(src).cuda(), init, 4)
    want = t.oracle(src, init, 4)
    assert_equal_to_the_oracle(got, want, (dim, scene, n))
    check_premise(scene, n, init, want[1], want[3])


# ------------------------------------------------------------------ the gated entries

def oracle_chain(t, src, init, iters, r):
    """The gated definition one outer iteration at a time, on the CPU alone: the indices of ALL points under T_k (the
    oracle's exact search), section 12's d2 in numpy, the kept points in the caller's order, one outer iteration of
    the tree oracle on them with reduce_geometry(kept).  Returns (pose, the last iteration's indices, inner, inliers)."""
    src3, dst3 = lifted(t.dim, src), t.tree.dst
    T = init
    idx = np.zeros(len(src), dtype=np.uint32)
    inner, inl = np.zeros(iters, dtype=np.uint32), np.zeros(iters, dtype=np.uint32)
    for k in range(iters):
        rc, idx = t.tree.search(moved(src3, T))
        assert rc == O.OK
        d2 = d2_of(src3, T, dst3[idx])[3]
        keep = d2 <= r * r
        inl[k] = keep.sum()
        rc, oT, _, oinner = oracle_plane_in_device_order(t.icp, t.tree, t.normals, src3[keep], T, 1)
        assert rc == O.OK
        T, inner[k] = I.Transform.from_pose(oT), oinner[0]
    return T, idx, inner, inl


@pytest.mark.parametrize("n", ENTRY_SIZES)
@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("dim", [3, 2])
def test_the_gated_entries_equal_the_tree_oracle_chained_on_the_kept_points(targets, dim, scene, n):
    import torch

    t = targets(dim, scene)
    _, src, init = SCENES[scene](dim, n)
    for r in (INF, gate(dim, scene)):
        oT, oidx, oinner, oinl = oracle_chain(t, src, init, 4, r)
        for s in (src, torch.from_numpy(src).cuda()):
            T, idx, inner, inl = t.estimate(s, init, 4, max_correspondence_distance=r)
            what = (dim, scene, n, r, type(s).__name__)
            assert np.array_equal(inl, oinl), (what, inl.tolist(), oinl.tolist())
            assert np.array_equal(inner, oinner), (what, inner.tolist(), oinner.tolist())
            assert np.array_equal(idx, oidx), what
            assert np.array_equal(bits(T), bits(oT)), (what, T.as_array(), oT.as_array())
        print(f"dim {dim} {scene} n={n} r={r}: inliers {oinl.tolist()}, inner {oinner.tolist()}")
        if r == INF:
            assert np.all(oinl == n)
        else:
            assert 0 < oinl[0] < n  # the bound removes some pairs and keeps others
            if scene in ("ties", "sigma0"):  # ... and all of the tied run
                assert oinl[0] >= ((2 * n) // 5 if scene == "ties" else (3 * n) // 5 + 1)
        check_premise(scene, n, init, oT, oinner)


# ------------------------------------------------------------------ the batched line kernel

def test_one_batched_line_call_equals_the_tree_oracle_item_by_item(targets):
    scenes = ["noisy", "ties", "sigma0", "heavy", "far"]
    sizes = [2, 3, 65, 513, 1024]
    shared = {}  # (one packed copy per distinct target cloud)
    srcs, dsts, what = [], [], []
    for scene in scenes:
        t = targets(2, scene)
        assert len(t.dst) <= 2048
        for n in sizes:
            srcs.append(SCENES[scene](2, n)[1])
            dsts.append(shared.setdefault(FAMILY[scene], t.dst))
            what.append((scene, n))
    inits = [I.Transform() for _ in srcs]
    B = I.IcpBatch(2)
    Ts, idxs, inner, status = B.estimate_point_to_line(srcs, dsts, inits, 4, k=NORMALS_K, return_info=True)
    served, one_by_one, _, refused = B.line_counters()
    B.close()
    print(f"served {served}, one by one {one_by_one}")
    assert served + one_by_one == len(srcs) and refused == 0
    for i, (scene, n) in enumerate(what):
        assert status[i] == _lib.OK
        want = targets(2, scene).oracle(srcs[i], inits[i], 4)
        assert_equal_to_the_oracle((Ts[i], idxs[i], inner[i]), want, ("batch", scene, n))
        check_premise(scene, n, inits[i], want[1], want[3])


# ------------------------------------------------------------------ the multi-rank plane call

@pytest.mark.parametrize("scene", ["noisy", "ties"])
def test_two_virtual_ranks_equal_the_tree_oracle(targets, scene):
    t = targets(3, scene)
    _, src, init = SCENES[scene](3, 1025)
    multi = I.IcpMulti(t.dst, [0, 0])
    try:
        multi.compute_target_normals(NORMALS_K)
        got = multi.estimate_point_to_plane(src, init, 4, return_info=True)
    finally:
        multi.close()
    want = t.oracle(src, init, 4)
    assert_equal_to_the_oracle(got, want, ("multi", scene))
    check_premise(scene, 1025, init, want[1], want[3])
