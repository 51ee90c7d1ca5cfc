"""Lattice clouds whose k-nearest sets are decided by the tie rule, for tests/test_knn_ties.py: every coordinate is an
integer multiple of a power of two, so every squared distance is exact in double and a tie is a tie on the device as on
the CPU.  A cloud keeps its integer lattice coordinates next to the float64 points, so that the tests can recompute
every d^2 in integer arithmetic.  Also here: the brute-force k-nearest lists by (d^2, index), what the tie rule decides
on a cloud (share of ties at the k-th place, conditioning of the covariance, effect of the WRONG rule "ties by highest
index"), and the CPU statements of the normals, each computed once per (cloud, k) and shared by the tests."""
import functools

import numpy as np

import oracle_ffi as O
from test_line_abi import line_normals_numpy

SEED = 20240  # of the row permutations
FAR = (2 ** 20, -(2 ** 19), 2 ** 10)  # |p| large, the searches' 1e-9 |p| slack still small against a cell
X31 = (2 ** 31, 0, 0)                 # the slack exceeds the cloud: no ring can be covered
SPLIT_AT = 2 ** 13                    # the split clouds' halves sit at x = -+2^13, at a spacing of 2^-12
LISTED = 17                           # neighbours kept per row: k <= 16 and the one behind them


class Cloud:
    """pts[i] = lattice[i] * 2^-shift, exactly; rows permuted with a fixed seed"""

    def __init__(self, name, lattice, shift, permute=True):
        lattice = np.asarray(lattice, dtype=np.int64)
        if permute:
            lattice = lattice[np.random.default_rng(SEED).permutation(len(lattice))]
        self.name, self.shift, self.dim = name, int(shift), lattice.shape[1]
        self.lattice = np.ascontiguousarray(lattice)
        assert np.abs(self.lattice).max(initial=0) < 2 ** 52
        self.pts = np.ascontiguousarray(self.lattice.astype(np.float64) * 2.0 ** -self.shift)
        self.spacing = 2.0 ** -self.shift
        self.m = len(self.pts)

    def __repr__(self):
        return self.name


def box(*n):
    """the lattice points of an n[0] x n[1] (x n[2]) box, x fastest"""
    axes = np.meshgrid(*[np.arange(k, dtype=np.int64) for k in n], indexing="ij")
    return np.stack([a.ravel(order="F") for a in axes], axis=1)


def shifted(lat, offset, shift):
    return lat + np.asarray(offset[:lat.shape[1]], dtype=np.int64) * 2 ** shift


def split(lat, shift):
    """the lower half of the x columns at x = -2^13 + ..., the upper half at x = +2^13 + ..."""
    half = (int(lat[:, 0].max()) + 1) // 2
    out = lat.copy()
    low = lat[:, 0] < half
    out[low, 0] = lat[low, 0] - SPLIT_AT * 2 ** shift
    out[~low, 0] = lat[~low, 0] - half + SPLIT_AT * 2 ** shift
    return out


@functools.lru_cache(maxsize=None)
def cloud(name):
    """base[+variant]: slab, slabdup, strip200x3, lat40x30, strip300x2, stripdup; variants far, x31, split"""
    base, _, variant = name.partition("+")
    lat = {"slab": lambda: box(24, 24, 2), "slabdup": lambda: np.repeat(box(12, 12, 2), 3, axis=0),
           "strip200x3": lambda: box(200, 3), "lat40x30": lambda: box(40, 30), "strip300x2": lambda: box(300, 2),
           "stripdup": lambda: np.repeat(box(150, 2), 3, axis=0)}[base]()
    shift = 3
    if variant == "far":
        lat = shifted(lat, FAR, shift)
    elif variant == "x31":
        lat = shifted(lat, X31, shift)
    elif variant == "split":
        shift = 12
        lat = split(lat, shift)
    else:
        assert variant == "", name
    return Cloud(name, lat, shift)


TINY_NAMES = ("one3", "two3", "three3", "five3", "cube", "one2", "two2", "three2", "five2", "square")


@functools.lru_cache(maxsize=None)
def tiny(name):
    """clouds of a few points, not permuted: too few for a normal, k clipped to m, and the cube and the square"""
    lat = {"one3": [[1, 2, 3]], "two3": [[1, 2, 3], [2, 2, 3]],
           "three3": [[0, 0, 0], [1, 0, 0], [0, 2, 0]],
           "five3": [[0, 0, 0], [1, 0, 0], [0, 2, 0], [3, 3, 0], [1, 1, 1]],
           "cube": box(2, 2, 2),
           "one2": [[1, 2]], "two2": [[1, 2], [2, 2]],
           "three2": [[0, 0], [1, 0], [0, 2]],
           "five2": [[0, 0], [1, 0], [0, 2], [3, 3], [5, 4]],
           "square": box(2, 2)}[name]
    return Cloud(name, lat, 3, permute=False)


def by_name(name):
    """the cloud of that name, whichever builder makes it (their names are disjoint)"""
    return tiny(name) if name in TINY_NAMES else cloud(name)


# the (cloud, k) the tie rule is tested on (the issue's table: measured shares, with margin to the thresholds)
PLANE_CASES = [("slab", k) for k in (4, 5, 7, 10, 16)] + [("slab+far", k) for k in (5, 7)] + \
              [("slab+x31", k) for k in (5, 7, 16)] + [("slab+split", k) for k in (5, 7)] + [("slabdup", 7)]
LINE_BASES = [("strip200x3", (3, 8, 16)), ("lat40x30", (8, 10)), ("strip300x2", (3, 5))]
LINE_CASES = [(b + v, k) for v in ("", "+far", "+x31") for b, ks in LINE_BASES for k in ks] + \
             [("strip200x3+split", k) for k in (3, 8, 16)] + [("stripdup", 6)]
LINE_CLOUDS = list(dict.fromkeys(name for name, _ in LINE_CASES))
ILL_CAP = {"slabdup": 0.05}  # the one cloud with ill-conditioned rows: at most this share of them


def d2_float(c, rows=None):
    """d^2 of every row against every target as the kernels and the CPU statements form it: the differences of the
    float64 coordinates, (dx dx + dy dy) + dz dz"""
    p = c.pts if rows is None else c.pts[rows]
    d = p[:, None, :] - c.pts[None, :, :]
    dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    return dd + d[..., 2] * d[..., 2] if c.dim == 3 else dd


def d2_integer(c):
    """the same in integer arithmetic on the lattice coordinates, in units of spacing^2"""
    d = c.lattice[:, None, :] - c.lattice[None, :, :]
    assert np.abs(d).max(initial=0) < 2 ** 30  # (squares and their sum stay inside int64)
    return (d * d).sum(axis=2)


@functools.lru_cache(maxsize=None)
def _neighbours(name):
    c = by_name(name)
    dd = d2_float(c)
    nb = np.argsort(dd, axis=1, kind="stable")[:, :LISTED]  # (stable: equal d2 in index order)
    return nb, np.take_along_axis(dd, nb, axis=1)


def neighbours(c):
    """(indices, d2) of each row's first min(m, 17) targets by (d2, index)"""
    return _neighbours(c.name)


def tie_share(c, k):
    """the share of rows whose k-th and (k+1)-th neighbours are equally far: the set depends on the tie rule"""
    _, dd = neighbours(c)
    kk = min(k, c.m)
    if kk >= c.m:
        return 0.0
    return float(np.mean(dd[:, kk - 1] == dd[:, kk]))


def ill_conditioned(c, k):
    """per row: are the two smallest eigenvalues of the neighbourhood's covariance closer than 1e-6 of the largest?
    (from the lattice coordinates relative to the row's own: small integers, so a far offset costs nothing)"""
    nb, _ = neighbours(c)
    kk = min(k, c.m)
    q = (c.lattice[nb[:, :kk]] - c.lattice[:, None, :]).astype(np.float64)
    q = q - q.mean(axis=1, keepdims=True)
    ev = np.linalg.eigvalsh(np.einsum("rjs,rjt->rst", q, q))
    return (ev[:, 1] - ev[:, 0]) < 1e-6 * ev[:, -1]


def _statement(pts, k):
    if pts.shape[1] == 2:
        return line_normals_numpy(pts, k)
    O.set_threads(16)
    try:
        return O.p2pl_normals(pts, k)
    finally:
        O.set_threads(1)


@functools.lru_cache(maxsize=None)
def _reference(name, k):
    c = by_name(name)
    out = _statement(c.pts, k)
    out.setflags(write=False)
    return out


def reference(c, k):
    """the CPU statement's normals: O.p2pl_normals (3-D, three columns) or line_normals_numpy (2-D, two columns)"""
    return _reference(c.name, k)


@functools.lru_cache(maxsize=None)
def _wrong_rule(name, k):
    c = by_name(name)
    out = np.ascontiguousarray(_statement(np.ascontiguousarray(c.pts[::-1]), k)[::-1])
    out.setflags(write=False)
    return out


def wrong_rule(c, k):
    """the normals under "ties by HIGHEST index": the CPU statement on the reversed cloud, reversed"""
    return _wrong_rule(c.name, k)


def moved_share(c, k):
    """the share of rows whose normal the wrong rule moves by more than 1e-3"""
    return float(np.mean(np.max(np.abs(reference(c, k) - wrong_rule(c, k)), axis=1) > 1e-3))
