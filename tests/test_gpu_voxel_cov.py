"""EXTENSION beyond the reference (include/icp_mi355x.h section 26): voxel covariances -- per occupied voxel the second
moments about the mean, beside section 25's mean, count, lowest index and point-to-voxel map.  Both entries are held to
the numpy restatement of the rule (tests/test_voxel_cov_abi.py: covariances_of): covariances and means byte for byte (a
NaN matches a NaN: host and device differ in the default NaN's sign bit), the integers exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib
from test_gpu_crop import _same_bytes
from test_gpu_voxel_mean import tree_edge_cloud
from test_voxel_abi import boundary_input, special_input
from test_voxel_cov_abi import PAIRS, divided, moments_of, same_bits_but_nans
from test_voxel_mean_abi import GONE, fold

pytestmark = pytest.mark.gpu

ALL = dict(return_means=True, return_counts=True, return_index=True, return_inverse=True, packed=True)


def by_host(p, v, ddof):
    out = I.voxel_covariances(p, v, ddof, **ALL)
    assert out[0].dtype == out[1].dtype == np.float64 and all(a.dtype == np.uint32 for a in out[2:])
    return out


def by_device(p, v, ddof):
    import torch

    out = I.voxel_covariances(torch.from_numpy(np.ascontiguousarray(p)).cuda(), v, ddof, **ALL)
    assert all(t.is_cuda for t in out) and out[0].dtype == out[1].dtype == torch.float64
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) + tuple(t.cpu().numpy().view(np.uint32) for t in out[2:])


def assert_is_the_restatement(p, v, ddofs=(0, 1), entries=(by_host, by_device), want=None):
    """both entries, both divisors, against the restatement (computed once: the divisor only enters at the end)"""
    p = np.ascontiguousarray(p)
    S, w_mean, w_count, w_first, w_of = want if want is not None else moments_of(p, v)
    for ddof in ddofs:
        w_cov = divided(S, w_count, ddof)
        for entry in entries:
            cov, mean, count, first, voxel_of = entry(p, v, ddof)
            name = (entry.__name__, ddof)
            assert len(cov) == len(mean) == len(count) == len(first) == len(w_count) and len(voxel_of) == len(p), name
            assert cov.shape == (len(w_count), len(PAIRS[p.shape[1]])), name
            assert np.array_equal(count, w_count), name
            assert np.array_equal(first, w_first), name
            assert np.array_equal(voxel_of, w_of), name
            assert same_bits_but_nans(mean, w_mean), (name, np.flatnonzero((mean != w_mean).any(axis=1))[:5])
            assert same_bits_but_nans(cov, w_cov), (name, np.flatnonzero((cov != w_cov).any(axis=1))[:5],
                                                    w_count[np.flatnonzero((cov != w_cov).any(axis=1))[:5]])
    return S, w_mean, w_count, w_first, w_of


# --------------------------------------------------------------------------------- sizes ----
@functools.lru_cache(maxsize=None)
def sized_cloud(dim, n):
    rng = np.random.default_rng(100 * n + dim)
    p = np.ascontiguousarray(rng.normal(size=(n, dim)) * 2.0)
    if n >= 63:
        for row, x in zip(rng.choice(n, 8, replace=False), (np.nan, np.inf, -np.inf, 0.0, -0.0, -0.0, 0.0, np.nan)):
            p[row, rng.integers(dim)] = x
    return p, moments_of(p, 0.5)


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 200_000])
@pytest.mark.parametrize("dim", [2, 3])
def test_covariances_equal_the_restatement(dim, n, ddof):
    """sizes around a wave, a tile of 1 024 and several tiles; rows with NaN, +-inf and +-0.0 among the points"""
    p, want = sized_cloud(dim, n)
    assert_is_the_restatement(p, 0.5, ddofs=(ddof,), want=want)
    count = want[2]
    assert n == 1 or len(count) < n
    assert n < 63 or np.count_nonzero(want[4] == GONE) >= 3
    assert n < 1023 or count.max() >= 2


# ---------------------------------------------------------------- the edges of the fold tree ----
def packed_moments(p, idx, mean, sum_of):
    """S[ab] = sum_of(products of the members' deviations from `mean`), packed"""
    d = p[idx] - mean
    return np.array([sum_of(d[:, a] * d[:, b]) for a, b in PAIRS[p.shape[1]]])


@pytest.mark.parametrize("c", [1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65_536, 65_537,
                               131_073])
@pytest.mark.parametrize("dim", [2, 3])
def test_a_voxel_at_an_edge_of_the_fold_tree(dim, c):
    """one voxel of exactly c members interleaved with other voxels' points (tree_edge_cloud: magnitudes over twelve
    decades, so most deviations are negative and a few large ones positive: the sums cancel); 131 073 members are three
    records, so the top level pads"""
    def tells(p, idx, mean):
        """do the members tell the tree from a left fold (np.cumsum is one) and from np.cov (on some entry each)"""
        tree = packed_moments(p, idx, mean, fold) / np.float64(c - 1)
        left = packed_moments(p, idx, mean, lambda t: np.cumsum(t)[-1]) / np.float64(c - 1)
        full = np.cov(p[idx].T, ddof=1)
        numpy_s = np.array([full[a, b] for a, b in PAIRS[dim]])
        return bool((tree != left).any() and (tree != numpy_s).any())

    # up to two values have one association only; from three on, the first seed whose members tell the orders apart
    # (decided on the CPU, on the inputs and the restated mean alone: without that the test would show nothing)
    for seed in range(1000 * c + dim, 1000 * c + dim + 64 * 7, 7):
        p, idx, v = tree_edge_cloud(dim, c, seed)
        mean = np.array([fold(p[idx, a]) / np.float64(c) for a in range(dim)])
        if c < 3 or tells(p, idx, mean):
            break
    assert c < 3 or tells(p, idx, mean)
    want = moments_of(p, v)
    r = want[4][idx[0]]
    assert want[2][r] == c and np.array_equal(np.flatnonzero(want[4] == r), idx)
    assert c == 1 or idx[-1] - idx[0] >= c  # interleaved with the points of other voxels
    assert _same_bytes(want[1][r], mean) and _same_bytes(want[0][r], packed_moments(p, idx, mean, fold))
    if c >= 3:
        d = p[idx] - mean
        assert (d.min(axis=0) < 0.0).all() and (d.max(axis=0) > 0.0).all()  # mixed signs inside every sum
    assert_is_the_restatement(p, v, want=want)


def test_a_wave_whose_voxels_mix_every_size_class():
    """the first 64 voxels (one wave of the fold launch: a lane per voxel) take their sizes from every class -- 1, 2 .. 8,
    9 .. 16, 17 .. 32, 33 .. 256 and above 256 -- in turns, so every narrow round, both ends of every ballot skip, the
    wave loop and the work list run in one wave; a second wave holds the classes in blocks"""
    rng = np.random.default_rng(77)
    classes = [(1,), (2, 3, 8), (9, 13, 16), (17, 25, 32), (33, 100, 256), (257, 300)]
    sizes = [classes[k % 6][(k // 6) % len(classes[k % 6])] for k in range(64)]
    sizes += [s for cl in classes for s in cl for _ in range(4)][:64]
    for dim in (2, 3):
        v = 0.5
        cell = np.concatenate([np.arange(len(sizes)), np.repeat(np.arange(len(sizes)), np.array(sizes) - 1)])
        p = np.empty((len(cell), dim))
        p[:, 0] = (cell + rng.uniform(0.05, 0.95, len(cell))) * v
        p[:, 1:] = rng.uniform(-0.45, -0.05, (len(cell), dim - 1)) * v
        tail = rng.permutation(np.arange(len(sizes), len(cell)))  # the first member of voxel k is point k
        p = np.ascontiguousarray(np.concatenate([p[:len(sizes)], p[tail]]))
        want = assert_is_the_restatement(p, v)
        assert np.array_equal(want[2], sizes) and np.array_equal(want[3], np.arange(len(sizes)))


# ------------------------------------------------------------ inputs that catch a wrong rule ----
@pytest.mark.parametrize("name", ["boundary", "specials_0.1", "specials_1e-3", "specials_1e300", "overflow", "huge",
                                  "products_overflow", "far_away", "one_voxel"])
@pytest.mark.parametrize("dim", [2, 3])
def test_covariances_of_the_inputs_that_catch_a_wrong_rule(dim, name):
    if name == "boundary":  # a product with 1 / v instead of the division merges other neighbours
        p, v = boundary_input(dim), 0.1
    elif name.startswith("specials"):
        p, v = special_input(dim), float(name.split("_")[1])
    elif name == "overflow":  # 1e308 / 1e-3 = +inf: a cell coordinate like any other
        p, v = np.concatenate([special_input(dim), special_input(dim)[[9, 11]]]), 1e-3
    elif name == "huge":  # 1e308 + 1e308 overflows: the mean is +inf, the deviations -inf, the other axes' are 0.0: NaN
        p, v = np.full((7, dim), 0.5), 1e300
        p[:, 0] = [1e308, -1e308, 1e308, 3.0, -1e308, 1e308, -3.0]
    elif name == "products_overflow":  # 1e200-sized deviations of both signs: +inf on the diagonal, NaN beside it
        p, v = np.full((9, dim), 1.0), 1e300
        p[:4, :2] = [[0.0, 0.0], [2e200, 2e200], [2e200, 0.0], [0.0, 2e200]]
        p[4:, 0] = [-1e200, -3e200, -1e200, -2e200, -1e250]  # a second voxel: the products of one sign, +inf only
    elif name == "far_away":  # 1e6 from the origin in voxels of 0.1: what a one-pass E[xx] - mm cannot do
        rng = np.random.default_rng(6)
        p, v = rng.normal(size=(20_000, dim)) * 0.2 + np.array([[1e6, -1e6, 2e6]])[:, :dim], 0.1
    else:  # three levels of the tree, every member in one segment
        p, v = np.random.default_rng(1).uniform(0.0, 1.0, (65_536 + 300, dim)), 1.0
    p = np.ascontiguousarray(p)
    S, mean, count, first, voxel_of = assert_is_the_restatement(p, v)
    diag = [k for k, (a, b) in enumerate(PAIRS[dim]) if a == b]
    assert (S[:, diag] >= 0.0).all()  # never negative, never a NaN
    if name == "one_voxel":
        assert np.array_equal(count, [len(p)]) and np.array_equal(first, [0])
    if name == "huge":
        assert np.array_equal(count, [3, 2, 1, 1]) and mean[0, 0] == np.inf and S[0, 0] == np.inf and np.isnan(S[0, 1])
    if name == "products_overflow":
        assert np.array_equal(count, [4, 5]) and S[0, 0] == np.inf and np.isnan(S[0, 1]) and S[1, 0] == np.inf
        assert not np.isnan(S[1]).any()
    if name == "far_away":
        assert count.max() >= 8 and np.isfinite(S).all()


# ------------------------------------------------------------------------ nullable outputs ----
@pytest.mark.parametrize("dim", [2, 3])
def test_every_output_but_the_covariances_is_optional_on_its_own(dim):
    import torch

    n, ns = 5_000, len(PAIRS[dim])
    p = np.ascontiguousarray(np.random.default_rng(5 + dim).normal(size=(n, dim)))
    S, w_mean, w_count, w_first, w_of = moments_of(p, 0.25)
    want = [divided(S, w_count, 1), w_mean, w_count, w_first, w_of]
    k = len(w_count)
    d_p = torch.from_numpy(p).cuda()
    masks = [tuple(j == i for j in range(4)) for i in range(4)] + [(False,) * 4, (True, False, False, True)]
    for mask in masks:
        mask = (True,) + mask  # (cov is required)
        host = [np.zeros((n, ns)), np.zeros((n, dim))] + [np.zeros(n, dtype=np.uint32) for _ in range(3)]
        args = [C.c_void_p(a.ctypes.data) if on else None for a, on in zip(host, mask)]
        voxels = C.c_size_t(0)
        rc = I.lib().icp_voxel_covariances(dim, C.c_void_p(p.ctypes.data), n, 0.25, 1, *args, C.byref(voxels), -1)
        assert rc == _lib.OK and voxels.value == k, mask
        dev = [torch.zeros((n, ns), dtype=torch.float64, device="cuda"), torch.zeros_like(d_p)]
        dev += [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
        args = [C.c_void_p(t.data_ptr()) if on else None for t, on in zip(dev, mask)]
        voxels = C.c_size_t(0)
        rc = I.lib().icp_voxel_covariances_device(dim, C.c_void_p(d_p.data_ptr()), n, 0.25, 1, *args, C.byref(voxels), -1,
                                                  None)
        assert rc == _lib.OK and voxels.value == k, mask
        got_dev = [dev[0].cpu().numpy(), dev[1].cpu().numpy()] + [t.cpu().numpy().view(np.uint32) for t in dev[2:]]
        for got in (host, got_dev):
            assert _same_bytes(got[0][:k], want[0])
            assert not mask[1] or _same_bytes(got[1][:k], want[1])
            assert not mask[2] or np.array_equal(got[2][:k], want[2])
            assert not mask[3] or np.array_equal(got[3][:k], want[3])
            assert not mask[4] or np.array_equal(got[4], want[4])
            for j in range(5):  # what was not asked for is not written
                assert mask[j] or not got[j].any()
    spare = np.zeros(6)
    for entry, tail in (("icp_voxel_covariances", (-1,)), ("icp_voxel_covariances_device", (-1, None))):
        voxels = C.c_size_t(7)
        rc = getattr(I.lib(), entry)(dim, None, 0, 0.25, 1, C.c_void_p(spare.ctypes.data), None, None, None, None,
                                     C.byref(voxels), *tail)
        assert rc == _lib.OK and voxels.value == 0
    assert I.voxel_covariances(np.zeros((0, dim)), 0.25, return_means=False).shape == (0, dim, dim)
    # the Python shapes: symmetric by default, a copy of the packed values; the covariances alone are an array
    full = I.voxel_covariances(p, 0.25, return_means=False)
    assert full.shape == (k, dim, dim)
    for j, (a, b) in enumerate(PAIRS[dim]):
        assert _same_bytes(full[:, a, b], want[0][:, j]) and _same_bytes(full[:, b, a], want[0][:, j])
    d_full, d_mean = I.voxel_covariances(d_p, 0.25)
    assert _same_bytes(d_full.cpu().numpy(), full) and _same_bytes(d_mean.cpu().numpy(), w_mean)
    assert _same_bytes(I.voxel_covariances(p, 0.25, ddof=0, return_means=False, packed=True), divided(S, w_count, 0))


# --------------------------------------------------------------- agreement with the centroids ----
@pytest.mark.parametrize("dim", [2, 3])
def test_everything_but_the_covariances_is_the_centroids_bytes(dim):
    import torch

    rng = np.random.default_rng(40 + dim)
    p = np.ascontiguousarray(rng.normal(size=(60_000, dim)) * 1.5)
    p[:400] = rng.uniform(0.0, 0.2, (400, dim))  # a voxel above 256 members: its mean comes from the second launch
    p[rng.choice(len(p), 20, replace=False), 0] = np.nan
    kw = dict(return_counts=True, return_index=True, return_inverse=True)
    centroids = I.voxel_centroids(p, 0.2, **kw)
    assert centroids[1].max() > 256
    for ddof in (0, 1):
        got = I.voxel_covariances(p, 0.2, ddof, **kw)
        assert all(_same_bytes(x, y) for x, y in zip(got[1:], centroids))
    d_p = torch.from_numpy(p).cuda()
    d_centroids, d_got = I.voxel_centroids(d_p, 0.2, **kw), I.voxel_covariances(d_p, 0.2, **kw)
    assert all(torch.equal(x, y) for x, y in zip(d_got[1:], d_centroids))
    assert all(_same_bytes(x.cpu().numpy().view(y.dtype), y) for x, y in zip(d_centroids, centroids))


# ----------------------------------------------------------------------------- determinism ----
def test_two_calls_and_another_stream_give_identical_bytes():
    import torch

    rng = np.random.default_rng(8)
    p = np.ascontiguousarray(rng.normal(size=(300_000, 3)) * 3.0)
    p[:70_000] = rng.uniform(0.0, 0.3, (70_000, 3))  # one voxel above 65 536 members: the lists filled by atomics
    a, b = by_host(p, 0.3, 1), by_host(p, 0.3, 1)
    assert a[2].max() > 65_536
    assert all(_same_bytes(x, y) for x, y in zip(a, b))
    d_p = torch.from_numpy(p).cuda()
    with torch.cuda.stream(torch.cuda.Stream()):
        c = I.voxel_covariances(d_p, 0.3, 1, **ALL)
    d = I.voxel_covariances(d_p, 0.3, 1, **ALL)
    for x, y, z in zip(c, d, a):
        assert torch.equal(x, y)
        assert _same_bytes(x.cpu().numpy().view(z.dtype), z)
    assert _same_bytes(d_p.cpu().numpy(), p)  # the input is never written
