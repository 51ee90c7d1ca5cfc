"""Clouds on which the f32 screens of the 1-NN engines cannot tell targets apart, for tests/test_blind_clouds.py (what
the clouds are, on the CPU) and tests/test_gpu_nn_blind.py (every engine against exact_nn on them).

Every engine promises the index of the exact f64 nearest neighbour, lowest index on ties, and gets its speed from an
f32 screen in front of the f64 test.  A screen's margin only matters where the gap between the best and the second-best
target is below the f32 resolution of a coordinate relative to the grid origin, about 2^-23 |q - lo|.  Here a box of
extent 1024 holds KNOTS of 32 targets c + s z, z integer in [-4, 4]^dim, at steps s = 2^-j from tens of f32 ulps down
to 1/256 of one (and 2^-30, where a knot is ONE f32 value), each with 64 queries c + s zq / 4, zq integer in
[-20, 20]^dim: quarter steps keep every d^2 exact in f64, half steps tie 2^dim targets.  Every coordinate is an integer
multiple of 2^-32 and is kept as such (int64) beside the float64 points, so that a test can redo d^2 in integers.

  dyadic knots   centres on multiples of 2^-4 in the upper half of the box: |c - lo| in [512, 1024], f32 ulp 2^-14..2^-13
  column knots   some of them with z[:, 0] = 0: 32 targets that share x bit for bit (a run of equal keys in the
                 one-workgroup kernels' x-sorted walk, one grid row per knot)
  face knots     centred on interior cell faces, edges and corners of the target grid, fl(lo[d] + c h[d]) by the grid's
                 documented geometry (_geometry): the 32 targets lie in at least two cells along the chosen axes
  bulk           targets on multiples of 2^-10 in [0, 1024), and (0, ...) and (1024, ...) pin the box
  +offset        the same cloud moved by (2^20, -2^19, 2^10)[:dim], still exact (at most 53 significant bits)
  tiny           m = 600 (8 knots, 2 of them column knots), 512 queries: the one-workgroup kernels' sizes

The rows of the targets are permuted: the lowest index of a tie is not the first in its cell or in a sweep of x."""
import functools

import numpy as np

UNIT = 32             # coordinates are integers in units of 2^-UNIT
E = 1024              # the box's extent on every axis
SEED = 40960
OFFSET = (2 ** 20, -(2 ** 19), 2 ** 10)
PER_KNOT, Q_PER_KNOT = 32, 64
BULK = 6000           # m = BULK + 2 + 60 * 32 = 7922
BULK_FULL = 16384 - 2 - 60 * PER_KNOT   # m = 16 384: whole tiles of the sweep, whatever the chunking
BULK_SMALL = 1800     # m = 3722: chunks of the sweep below one tile even at the sizes of its 2 / 4 / 8 queries per lane
BULK_QUERIES = 256
# the steps 2^-j of the dyadic knots: a few at tens of ulps, most where the screen is blind, four collapsed in f32
J_DYADIC = [9, 10, 11, 12] + [13, 14, 15, 16, 17, 18] * 2 + [14, 16, 18] + [19] * 6 + [20] * 6 + [21] * 6 + [22] * 7 + [30] * 4
N_COLUMN = 8
J_FACE = [12, 13, 14, 15, 16, 17, 18, 19, 20, 14, 16, 18]
J_TINY, COLUMN_TINY = [12, 14, 16, 18, 19, 20, 22, 30], (1, 5)


def _geometry(dst):
    """(origin, cell sizes, cells per axis) of the target grid (nn_grid.hip: build_grid, below its caps)"""
    lo, hi = dst.min(0), dst.max(0)
    ext = hi - lo
    live = ext > 1e-9 * ext.max()
    hh = (2.0 * np.prod(ext[live]) / len(dst)) ** (1.0 / live.sum())
    h = np.full(dst.shape[1], hh)
    h[0] = hh / 4.0
    n = np.where(live, np.floor(ext / h) + 1, 1).astype(np.int64)
    return lo, h, n


def cells(dst, pts):
    """the grid cell of `pts` per axis, as the build bins a target (nn_grid.hip: cell_coord)"""
    lo, h, n = _geometry(dst)
    return np.clip(np.floor((pts - lo) * (1.0 / h)), 0, n - 1).astype(np.int64)


def to_float(lat):
    """lattice coordinates -> float64, exactly"""
    lat = np.asarray(lat, dtype=np.int64)
    assert np.abs(lat).max(initial=0) < 2 ** 53
    out = np.ascontiguousarray(lat.astype(np.float64) * 2.0 ** -UNIT)
    assert np.array_equal((out * 2.0 ** UNIT).astype(np.int64), lat)
    return out


class Cloud:
    """dst / q: float64 targets and UNIQUE queries; dst_lat / q_lat: the same as int64 multiples of 2^-32;
    knot_of_t / knot_of_q: the knot of a target / query (-1: bulk); kind[k], j[k], axes[k]: what knot k is, its step
    2^-j and (face knots) the axes along which it straddles a cell boundary"""

    def __init__(self, name, dst_lat, q_lat, knot_of_t, knot_of_q, kind, j, axes):
        self.name, self.dim = name, dst_lat.shape[1]
        self.dst_lat, self.q_lat = np.ascontiguousarray(dst_lat), np.ascontiguousarray(q_lat)
        self.dst, self.q = to_float(dst_lat), to_float(q_lat)
        self.knot_of_t, self.knot_of_q = knot_of_t, knot_of_q
        self.kind, self.j, self.axes = list(kind), list(j), list(axes)
        self.m, self.nq = len(self.dst), len(self.q)
        for a in (self.dst, self.q, self.dst_lat, self.q_lat, self.knot_of_t, self.knot_of_q):
            a.setflags(write=False)

    def __repr__(self):
        return self.name

    @property
    def knot_queries(self):
        return self.knot_of_q >= 0

    @property
    def dyadic_queries(self):
        """queries of the knots whose centres are multiples of 2^-4 (all but the face knots)"""
        return np.array([k >= 0 and self.kind[k] != "face" for k in self.knot_of_q])


def _build(dim, bulk, tiny):
    rng = np.random.default_rng(SEED + 10 * dim + bulk)
    js = list(J_TINY if tiny else J_DYADIC)
    column = set(COLUMN_TINY) if tiny else set(int(k) for k in rng.choice(len(js) - 4, size=N_COLUMN, replace=False))
    faces = [] if tiny else list(J_FACE)
    m = bulk + 2 + (len(js) + len(faces)) * PER_KNOT
    one = 1 << UNIT
    stub = np.zeros((m, dim))
    stub[-1] = E
    lo, h, n = _geometry(stub)  # lo, hi and m are known before the first point is drawn

    t_lat = [np.zeros((1, dim), dtype=np.int64), np.full((1, dim), E * one, dtype=np.int64),
             rng.integers(0, E << 10, size=(bulk, dim)).astype(np.int64) << (UNIT - 10)]
    t_knot = [np.full(2 + bulk, -1, dtype=np.int64)]
    q_lat, q_knot, kind, axes = [], [], [], []

    def knot(c_lat, j, z):
        k = len(kind)
        zq = rng.integers(-20, 21, size=(Q_PER_KNOT, dim)).astype(np.int64)
        t_lat.append(c_lat + (z << (UNIT - j)))
        q_lat.append(c_lat + (zq << (UNIT - j - 2)))
        t_knot.append(np.full(PER_KNOT, k, dtype=np.int64))
        q_knot.append(np.full(Q_PER_KNOT, k, dtype=np.int64))

    for k, j in enumerate(js):
        c_lat = rng.integers(512 * 16, 1023 * 16, size=dim).astype(np.int64) << (UNIT - 4)
        z = rng.integers(-4, 5, size=(PER_KNOT, dim)).astype(np.int64)
        if k in column:
            z[:, 0] = 0
        knot(c_lat, j, z)
        kind.append("collapsed" if j == 30 else ("column" if k in column else "dyadic"))
        axes.append(())
    # faces (one axis), edges (two) and corners (all; in two dimensions an edge is a corner)
    choices = [(d,) for d in range(dim)] * 2 + [(0, 1), (0, dim - 1), (1, dim - 1), (0, 1)] + [tuple(range(dim))] * 2
    for j, ax in zip(faces, choices + choices):
        ax = tuple(sorted(set(ax)))
        c_lat = rng.integers(64 * 16, 1023 * 16, size=dim).astype(np.int64) << (UNIT - 4)
        for d in ax:
            c = int(rng.integers(2, n[d] - 2))
            c_lat[d] = int(np.rint((lo[d] + c * h[d]) * 2.0 ** 24)) << (UNIT - 24)  # fl(lo + c h), to 2^-24
        z = rng.integers(-4, 5, size=(PER_KNOT, dim)).astype(np.int64)
        knot(c_lat, j, z)
        kind.append("face")
        axes.append(ax)
    if not tiny:  # queries that belong to no knot, some of them outside the box
        q_lat.append(rng.integers(-64 << 10, (E + 64) << 10, size=(BULK_QUERIES, dim)).astype(np.int64) << (UNIT - 10))
        q_knot.append(np.full(BULK_QUERIES, -1, dtype=np.int64))

    t_lat, t_knot = np.concatenate(t_lat), np.concatenate(t_knot)
    assert len(t_lat) == m
    perm = rng.permutation(m)
    return t_lat[perm], np.concatenate(q_lat), t_knot[perm], np.concatenate(q_knot), kind, js + faces, axes


def check_straddle(c):
    """every face knot's targets lie in at least two cells along each of its axes, by the restated geometry -- with
    distances between them far below the f32 ulp there"""
    lo, h, n = _geometry(c.dst)
    assert np.array_equal(lo, c.dst.min(0)) and (np.all(n >= 8) or not any(c.axes)), (lo, n)
    cell = cells(c.dst, c.dst)
    for k, ax in enumerate(c.axes):
        mine = c.knot_of_t == k
        for d in ax:
            got = np.unique(cell[mine, d])
            assert len(got) >= 2 and 0 < got.min() and got.max() < n[d] - 1, (c.name, k, d, got)
            assert 2.0 ** -c.j[k] * 8 < 0.01 * h[d]


@functools.lru_cache(maxsize=None)
def cloud(dim, variant="plain", bulk=BULK):
    """variant: plain, offset or tiny (m = 600, 512 queries; `bulk` is then ignored)"""
    tiny = variant == "tiny"
    t_lat, q_lat, t_knot, q_knot, kind, js, axes = _build(dim, 600 - 2 - len(J_TINY) * PER_KNOT if tiny else bulk, tiny)
    if variant == "offset":
        off = np.array(OFFSET[:dim], dtype=np.int64) << UNIT
        t_lat, q_lat = t_lat + off, q_lat + off
    else:
        assert variant in ("plain", "tiny"), variant
    c = Cloud(f"blind{dim}-{variant}-{len(t_lat)}", t_lat, q_lat, t_knot, q_knot, kind, js, axes)
    c.key = (dim, variant, bulk)
    assert np.array_equal(c.dst.min(0), to_float(t_lat.min(0)[None])[0]) and np.all(c.dst.max(0) - c.dst.min(0) == E)
    check_straddle(c)
    return c


def d2_matrix(dst, q):
    """the contract's (dx dx + dy dy) + dz dz in float64, every product and sum rounded on its own: len(q) x len(dst)"""
    dx = q[:, 0, None] - dst[None, :, 0]
    dy = q[:, 1, None] - dst[None, :, 1]
    d2 = dx * dx + dy * dy
    if dst.shape[1] == 3:
        dz = q[:, 2, None] - dst[None, :, 2]
        d2 = d2 + dz * dz
    return d2


def nearest(dst, q):
    """exact_nn's indices alone"""
    idx = np.empty(len(q), dtype=np.uint32)
    for i in range(0, len(q), 128):  # (small blocks: the temporaries stay in cache)
        idx[i:i + 128] = np.argmin(d2_matrix(dst, q[i:i + 128]), axis=1)
    return idx


def exact_nn(dst, q):
    """(index of the nearest target by the contract's float64 d^2, first minimum; the gap sqrt(d2 of the second-best
    target) - sqrt(d2 of the best); whether the minimum is tied), per query"""
    idx = np.empty(len(q), dtype=np.uint32)
    gap = np.empty(len(q))
    tied = np.empty(len(q), dtype=bool)
    for i in range(0, len(q), 500):
        d2 = d2_matrix(dst, q[i:i + 500])
        idx[i:i + 500] = np.argmin(d2, axis=1)
        if dst.shape[0] > 1:
            two = np.partition(d2, 1, axis=1)[:, :2]
            gap[i:i + 500] = np.sqrt(two[:, 1]) - np.sqrt(two[:, 0])
            tied[i:i + 500] = two[:, 0] == two[:, 1]
        else:
            gap[i:i + 500], tied[i:i + 500] = np.inf, False
    return idx, gap, tied


@functools.lru_cache(maxsize=None)
def _reference(dim, variant, bulk):
    c = cloud(dim, variant, bulk)
    out = exact_nn(c.dst, c.q)
    for a in out:
        a.setflags(write=False)
    return out


def reference(c):
    """exact_nn of a cloud's own queries, computed once"""
    return _reference(*c.key)


def tiled(c, n):
    """(n queries, their exact_nn indices): the unique queries repeated, cut at n"""
    reps = n // c.nq + 1
    return np.ascontiguousarray(np.tile(c.q, (reps, 1))[:n]), np.tile(reference(c)[0], reps)[:n]


def f32_ulp_at(c, q=None):
    """the f32 resolution of a coordinate relative to the grid origin, at every query: ulp_f32(|q - lo|)"""
    q = c.q if q is None else q
    return np.spacing(np.sqrt(((q - c.dst.min(0)) ** 2).sum(1)).astype(np.float32)).astype(np.float64)


def screen_model(dst, q, ec_factor=1.0):
    """A numpy model of the documented screen of k_nn_brute_scr (nn_brute.hip), one chunk: f32 coordinates relative to
    the origin of the screen (the centre of the targets' box), s32 evaluated in f32, skipped iff s32 > thr with thr
    taken from the running best -- (float)((sqrt(best) + ec)^2 * 1.000004) * 1.000001f + 1e-37f, ec = (max |q - org| +
    2 scale) * 1.2e-7 * sqrt(3) --, ascending target order, strict `<` in the exact test.  `ec_factor` scales ec
    (0: the margin dropped).  Returns the indices."""
    f = np.float32
    dim = dst.shape[1]
    lo, hi = dst.min(0), dst.max(0)
    org = 0.5 * (lo + hi)
    hh = _geometry(dst)[1][-1]
    scale = max(np.abs(lo).max(), np.abs(hi).max()) + hh  # build_grid: GridParams::scale
    out = np.empty(len(q), dtype=np.uint32)
    pf = np.ascontiguousarray((dst - org).astype(f).T)  # dim x m
    for i in range(0, len(q), 1024):
        qq = q[i:i + 1024]
        a = qq - org
        qf = a.astype(f)
        ec = (np.abs(a).max(1) + 2.0 * scale) * 1.2e-7 * 1.7320508075688774 * ec_factor
        dx = qf[None, :, 0] - pf[0][:, None]  # m x nq
        dy = qf[None, :, 1] - pf[1][:, None]
        s32 = dx * dx + dy * dy
        if dim == 3:
            dz = qf[None, :, 2] - pf[2][:, None]
            s32 = s32 + dz * dz
        assert s32.dtype == f
        d2 = np.ascontiguousarray(d2_matrix(dst, qq).T)
        best = np.full(len(qq), np.inf)
        thr = np.full(len(qq), np.inf, dtype=f)
        bi = np.zeros(len(qq), dtype=np.uint32)
        for k in range(len(dst)):
            better = (s32[k] <= thr) & (d2[k] < best)
            if better.any():
                best[better] = d2[k][better]
                bi[better] = k
                rr = np.sqrt(best[better]) + ec[better]
                thr[better] = (rr * rr * 1.000004).astype(f) * f(1.000001) + f(1e-37)
        out[i:i + 1024] = bi
    return out
