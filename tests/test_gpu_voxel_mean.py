"""EXTENSION beyond the reference (include/icp_mi355x.h section 25): voxel centroids -- per occupied voxel the mean, the
count and the lowest index, per point the number of its voxel.  Both entries are held to the numpy restatement of the rule
(tests/test_voxel_mean_abi.py: centroids_of): the means byte for byte, the integers exactly."""
import ctypes as C

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib, harness, synth
from test_gpu_crop import _same_bytes
from test_voxel_abi import boundary_input, kept_index_of, special_input
from test_voxel_mean_abi import GONE, centroids_of, fold

pytestmark = pytest.mark.gpu


def by_host(p, v):
    out = I.voxel_centroids(p, v, return_counts=True, return_index=True, return_inverse=True)
    assert out[0].dtype == np.float64 and all(a.dtype == np.uint32 for a in out[1:])
    return out


def by_device(p, v):
    import torch

    out = I.voxel_centroids(torch.from_numpy(np.ascontiguousarray(p)).cuda(), v, return_counts=True, return_index=True,
                            return_inverse=True)
    assert all(t.is_cuda for t in out) and out[0].dtype == torch.float64
    return (out[0].cpu().numpy(),) + tuple(t.cpu().numpy().view(np.uint32) for t in out[1:])


def assert_is_the_restatement(p, v, entries=(by_host, by_device)):
    p = np.ascontiguousarray(p)
    want = centroids_of(p, v)
    for entry in entries:
        mean, count, first, voxel_of = entry(p, v)
        name = entry.__name__
        assert len(mean) == len(count) == len(first) == len(want[0]) and len(voxel_of) == len(p), name
        assert np.array_equal(count, want[1]), name
        assert np.array_equal(first, want[2]), name
        assert np.array_equal(voxel_of, want[3]), name
        assert _same_bytes(mean, want[0]), (name, np.flatnonzero((mean != want[0]).any(axis=1))[:5])
    return want


# --------------------------------------------------------------------------------- sizes ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 200_000])
@pytest.mark.parametrize("dim", [2, 3])
def test_centroids_equal_the_restatement(dim, n):
    """sizes around a wave, a tile of 1 024 and several tiles; rows with NaN, +-inf and +-0.0 among the points"""
    rng = np.random.default_rng(100 * n + dim)
    p = np.ascontiguousarray(rng.normal(size=(n, dim)) * 2.0)
    if n >= 63:
        for row, x in zip(rng.choice(n, 8, replace=False), (np.nan, np.inf, -np.inf, 0.0, -0.0, -0.0, 0.0, np.nan)):
            p[row, rng.integers(dim)] = x
    want = assert_is_the_restatement(p, 0.5)
    assert n == 1 or len(want[0]) < n
    assert n < 63 or np.count_nonzero(want[3] == GONE) >= 3
    assert n < 1023 or want[1].max() >= 2


# ---------------------------------------------------------------- the edges of the fold tree ----
def tree_edge_cloud(dim, c, seed):
    """one voxel of exactly c members (v = 1e6) whose magnitudes spread over twelve decades, 10^-6 .. 10^6, so that a
    wrong association changes bits.  The members of a voxel share their sign on an axis (the cell 0 holds [0, v), the
    cell -1 holds [-v, 0)), so the signs are mixed across the axes: axis 0 is positive, the others negative.  The
    members are interleaved by index with the points of other voxels (one to three points each), so that they are
    contiguous only after the sort.  Returns the cloud and the members' indices."""
    rng = np.random.default_rng(seed)
    v = 1e6
    members = 10.0 ** rng.uniform(-6.0, 5.99, (c, dim))
    members[:, 1:] *= -1.0
    others = max(c, 40)
    cell = rng.integers(2, 2 + others // 2, others)  # cells 2 ..: one to a few points each
    rest = np.empty((others, dim))
    rest[:, 0] = (cell + rng.uniform(0.01, 0.99, others)) * v
    rest[:, 1:] = -(10.0 ** rng.uniform(-6.0, 5.99, (others, dim - 1)))
    p = np.concatenate([members, rest])
    where = rng.permutation(len(p))
    cloud = np.empty_like(p)
    cloud[where] = p
    return np.ascontiguousarray(cloud), np.sort(where[:c]), v


@pytest.mark.parametrize("c", [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65_536, 65_537])
@pytest.mark.parametrize("dim", [2, 3])
def test_a_voxel_at_an_edge_of_the_fold_tree(dim, c):
    def tells(p, idx, mean):
        """do the members tell the tree from a left fold and from numpy's pairwise mean (on some axis each)"""
        left = np.zeros(dim)
        for row in p[idx]:
            left = left + row
        return (any(mean[a] != left[a] / c for a in range(dim)) and
                any(mean[a] != np.mean(p[idx, a]) for a in range(dim)))

    # one or two values have one association only; from three on, the first seed whose members tell the orders apart
    # (decided on the CPU, on the inputs and the restatement alone: without that the test would show nothing)
    for seed in range(1000 * c + dim, 1000 * c + dim + 64 * 7, 7):
        p, idx, v = tree_edge_cloud(dim, c, seed)
        want = centroids_of(p, v)
        r = want[3][idx[0]]
        if c < 3 or tells(p, idx, want[0][r]):
            break
    assert want[1][r] == c and np.array_equal(np.flatnonzero(want[3] == r), idx)
    assert c == 1 or idx[-1] - idx[0] >= c  # interleaved with the points of other voxels
    assert c < 3 or tells(p, idx, want[0][r])
    assert all(want[0][r, a] == fold(p[idx, a]) / np.float64(c) for a in range(dim))
    assert_is_the_restatement(p, v)


# ------------------------------------------------------------------ the sort's digit edges ----
@pytest.mark.parametrize("voxels", [2047, 2048, 2049])
def test_voxel_numbers_around_one_sort_digit(voxels):
    """the sort underneath takes digits of up to 11 bits (csrc/qsort.hip: kRsMaxBits): 2 047 voxel numbers fit one
    digit, 2 048 do not; every second voxel has two members, and once every point is alone (the keys are sized by n)"""
    rng = np.random.default_rng(voxels)
    cell = np.concatenate([np.arange(voxels), np.arange(0, voxels, 2)])
    p = np.zeros((len(cell), 3))
    p[:, 0] = (cell + rng.uniform(0.1, 0.9, len(cell))) * 0.5
    p[:, 1:] = rng.uniform(0.1, 0.4, (len(cell), 2))
    p = np.ascontiguousarray(p[rng.permutation(len(p))])
    want = assert_is_the_restatement(p, 0.5)
    assert len(want[0]) == voxels and np.count_nonzero(want[1] == 2) == (voxels + 1) // 2
    alone = np.ascontiguousarray(p[want[2]])
    want = assert_is_the_restatement(alone, 0.5)
    assert len(want[0]) == voxels and _same_bytes(want[0], alone)


def test_two_to_the_22_plus_one_points_alone_in_their_voxels():
    """three digits of the sort, every point its own voxel: the means are the input's bytes (checked on the device)"""
    import torch

    n, v = (1 << 22) + 1, 0.25
    g = torch.Generator(device="cuda").manual_seed(5)
    k = torch.randperm(n, device="cuda", generator=g)
    d_p = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    d_p[:, 0] = k.double() * v + 0.125  # (exact: multiples of 1 / 8 far below 2^53)
    d_p[:, 1], d_p[:, 2] = -0.0, 0.7
    mean, count, first, voxel_of = I.voxel_centroids(d_p, v, return_counts=True, return_index=True, return_inverse=True)
    assert len(mean) == len(count) == len(first) == len(voxel_of) == n
    assert torch.equal(mean.view(torch.int64), d_p.view(torch.int64))  # (bits: the -0.0 column stays -0.0)
    assert bool((count == 1).all())
    ramp = torch.arange(n, device="cuda", dtype=torch.int32)
    assert torch.equal(first, ramp) and torch.equal(voxel_of, ramp)
    del mean, count, first, voxel_of, d_p
    I.lib().icp_trim_pool()


# ------------------------------------------------------------ inputs that catch a wrong rule ----
@pytest.mark.parametrize("name", ["boundary", "specials_0.1", "specials_1e-3", "specials_1e300", "overflow", "huge",
                                  "one_voxel", "distinct"])
@pytest.mark.parametrize("dim", [2, 3])
def test_centroids_of_the_inputs_that_catch_a_wrong_rule(dim, name):
    if name == "boundary":  # a product with 1 / v instead of the division merges other neighbours
        p, v = boundary_input(dim), 0.1
    elif name.startswith("specials"):
        p, v = special_input(dim), float(name.split("_")[1])
    elif name == "overflow":  # 1e308 / 1e-3 = +inf: a cell coordinate like any other
        p, v = np.concatenate([special_input(dim), special_input(dim)[[9, 11]]]), 1e-3
    elif name == "huge":  # 1e308 + 1e308 overflows: the voxel's mean is +inf; its mirror image is another voxel
        p, v = np.full((7, dim), 0.5), 1e300
        p[:, 0] = [1e308, -1e308, 1e308, 3.0, -1e308, 1e308, -3.0]
    elif name == "one_voxel":  # three levels of the tree, every member in one segment
        p, v = np.random.default_rng(1).uniform(0.0, 1.0, (65_536 + 300, dim)), 1.0
    else:  # no two points share a voxel
        k = np.random.default_rng(2).permutation(70_001)
        p, v = np.zeros((70_001, dim)), 0.25
        p[:, 0], p[:, dim - 1] = k * 0.25 + 0.125, (k % 7) * 0.25
    p = np.ascontiguousarray(p)
    want = assert_is_the_restatement(p, v)
    if name == "one_voxel":
        assert np.array_equal(want[1], [len(p)]) and np.array_equal(want[2], [0])
    if name == "distinct":
        assert len(want[0]) == len(p) and _same_bytes(want[0], p)
    if name == "huge":
        assert np.array_equal(want[2], [0, 1, 3, 6]) and np.array_equal(want[1], [3, 2, 1, 1])
        assert want[0][0, 0] == np.inf and want[0][1, 0] == -np.inf and want[0][2, 0] == 3.0
        assert not np.isnan(want[0]).any()
    if name == "overflow":
        assert 9 in want[2] and 11 in want[2] and want[1][want[3][9]] == 2 and want[1][want[3][11]] == 2


# ------------------------------------------------------------------------ nullable outputs ----
@pytest.mark.parametrize("dim", [2, 3])
def test_every_output_is_optional_on_its_own(dim):
    import torch

    n = 5_000
    p = np.ascontiguousarray(np.random.default_rng(5 + dim).normal(size=(n, dim)))
    want = centroids_of(p, 0.25)
    k = len(want[0])
    d_p = torch.from_numpy(p).cuda()
    masks = [tuple(j == i for j in range(4)) for i in range(4)] + [(False,) * 4, (True, False, False, True)]
    for mask in masks:
        host = [np.zeros((n, dim)), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)]
        args = [C.c_void_p(a.ctypes.data) if on else None for a, on in zip(host, mask)]
        voxels = C.c_size_t(0)
        rc = I.lib().icp_voxel_centroids(dim, C.c_void_p(p.ctypes.data), n, 0.25, *args, C.byref(voxels), -1)
        assert rc == _lib.OK and voxels.value == k, mask
        dev = [torch.zeros_like(d_p)] + [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
        args = [C.c_void_p(t.data_ptr()) if on else None for t, on in zip(dev, mask)]
        voxels = C.c_size_t(0)
        rc = I.lib().icp_voxel_centroids_device(dim, C.c_void_p(d_p.data_ptr()), n, 0.25, *args, C.byref(voxels), -1, None)
        assert rc == _lib.OK and voxels.value == k, mask
        got_dev = [dev[0].cpu().numpy()] + [t.cpu().numpy().view(np.uint32) for t in dev[1:]]
        for got in (host, got_dev):
            assert not mask[0] or _same_bytes(got[0][:k], want[0])
            assert not mask[1] or np.array_equal(got[1][:k], want[1])
            assert not mask[2] or np.array_equal(got[2][:k], want[2])
            assert not mask[3] or np.array_equal(got[3], want[3])
            for j in range(4):  # what was not asked for is not written
                assert mask[j] or not got[j].any()
    voxels = C.c_size_t(7)
    assert I.lib().icp_voxel_centroids(dim, None, 0, 0.25, None, None, None, None, C.byref(voxels), -1) == _lib.OK
    assert voxels.value == 0
    voxels = C.c_size_t(7)
    assert I.lib().icp_voxel_centroids_device(dim, None, 0, 0.25, None, None, None, None, C.byref(voxels), -1,
                                              None) == _lib.OK
    assert voxels.value == 0
    assert len(I.voxel_centroids(np.zeros((0, dim)), 0.25)) == 0
    assert _same_bytes(I.voxel_centroids(p, 0.25), want[0])  # (the means alone: an array, not a tuple)


# ------------------------------------------------------------------ agreement with thinning ----
@pytest.mark.parametrize("dim", [2, 3])
def test_the_first_index_is_the_thinning_s_and_the_inverse_counts_the_members(dim):
    rng = np.random.default_rng(40 + dim)
    p = np.ascontiguousarray(rng.normal(size=(60_000, dim)) * 1.5)
    p[rng.choice(len(p), 20, replace=False), 0] = np.nan
    mean, count, first, voxel_of = by_host(p, 0.2)
    kept, index = I.voxel_downsample(p, 0.2, return_index=True)
    assert np.array_equal(first, index) and np.array_equal(first, kept_index_of(p, 0.2))
    valid = voxel_of != GONE
    assert np.count_nonzero(~valid) == 20
    assert np.array_equal(np.bincount(voxel_of[valid], minlength=len(count)), count)
    assert np.array_equal(voxel_of[first], np.arange(len(first)))


# ----------------------------------------------------------------------------- determinism ----
def test_two_calls_and_another_stream_give_identical_bytes():
    import torch

    rng = np.random.default_rng(8)
    p = np.ascontiguousarray(rng.normal(size=(300_000, 3)) * 3.0)
    p[:70_000] = rng.uniform(0.0, 0.3, (70_000, 3))  # one voxel above 65 536 members: the lists filled by atomics
    a, b = by_host(p, 0.3), by_host(p, 0.3)
    assert a[1].max() > 65_536
    assert all(_same_bytes(x, y) for x, y in zip(a, b))
    d_p = torch.from_numpy(p).cuda()
    kw = dict(return_counts=True, return_index=True, return_inverse=True)
    with torch.cuda.stream(torch.cuda.Stream()):
        c = I.voxel_centroids(d_p, 0.3, **kw)
    d = I.voxel_centroids(d_p, 0.3, **kw)
    for x, y, z in zip(c, d, a):
        assert torch.equal(x, y)
        assert _same_bytes(x.cpu().numpy().view(z.dtype), z)
    assert _same_bytes(d_p.cpu().numpy(), p)  # the input is never written


# ------------------------------------------------------------------------------- the harness ----
def test_scan_to_map_on_centroids_registers_the_restatement_s_first_scan():
    pk = synth.synthetic_scan3d_packets(4 * synth.PACKETS_PER_FRAME)
    seen = []

    def factory(dst):
        seen.append(np.array(dst, copy=True))
        return I.Icp3d(dst)

    Ts, path, world = harness.run_scan_to_map(pk, max_iter=5, icp_factory=factory, scan_voxel=0.05,
                                              scan_voxel_centroids=True)
    frame0 = harness.remove_invalid_values(np.asarray(pk[:synth.PACKETS_PER_FRAME], dtype=np.float64))
    want = centroids_of(frame0, 0.05)[0]
    assert len(Ts) == 3 and len(seen) == 1 and 0 < len(want) < len(frame0)
    assert _same_bytes(seen[0], want)
    assert world.target_count > len(want) and np.isfinite(path).all()
    world.close()
