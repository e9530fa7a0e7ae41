"""slam_vmap_coarsen restated in Python (docs/VOXEL_MAP.md section 11.1): a dict of Python ints, written from the contract
and not from the C++, and the inputs tests/test_vmap_coarsen.py (the restatement against maps built directly at the coarser
leaf by tests/cpp/vmap_oracle.cpp and vmap_gicp_oracle.cpp) and tests/test_gpu_vmap_coarsen.py (the device against the
restatement) share."""
import math
import struct

import numpy as np

import vmap_cases as K

F = np.float32
HALF = 1 << 20
FIELD = (1 << 21) - 1
U32, U64 = (1 << 32) - 1, (1 << 64) - 1
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # xx xy xz yy yz zz
MUT_NONE, MUT_TRUNCATE, MUT_NO_CROSS, MUT_FULL_L, MUT_ADD_CARVE = 0, 1, 2, 3, 4
# (finer leaf, coarser leaf) of the four-cloud case; every finer leaf is a multiple of 2^-16 m, so the moments travel
LEAF_PAIRS = ((0.25, 0.5), (0.25, 1.0), (0.25, 2.0), (0.375, 1.5))
PLAIN_ONLY = (0.30, 0.60)                                           # L = 314 573 is no multiple of 16: sums and counts only


def key_of(ix, iy, iz):
    return ((int(iz) + HALF) << 42) | ((int(iy) + HALF) << 21) | (int(ix) + HALF)


def cells_of(key):
    key = int(key)
    return [((key >> s) & FIELD) - HALF for s in (0, 21, 42)]


def i64(v):
    """a Python int as the int64 a wrapping add leaves"""
    v &= U64
    return v - (1 << 64) if v >> 63 else v


def same_double(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def shift_of(src_leaf, dst_leaf):
    """j with dst_leaf == ldexp(src_leaf, j) bit for bit, 1 <= j <= 8; None otherwise"""
    for j in range(1, 9):
        if same_double(math.ldexp(src_leaf, j), dst_leaf):
            return j
    return None


def moments_split(src_leaf):
    """whether floor(d / 16) splits over the finer cells: the leaf is a multiple of 2^-16 m"""
    return math.ldexp(src_leaf, 16).is_integer()


class CoarseMap:
    """The coarser map as a dict: key -> [count, [3 sums], [3 E], [6 M], seen, miss], all Python ints.  coarsen() raises
    ValueError where the library answers SLAM_E_INVALID."""

    def __init__(self, leaf, moments=False, mutation=MUT_NONE):
        self.leaf, self.moments, self.mutation = float(leaf), moments, mutation
        self.v, self.n_points = {}, 0

    @property
    def n_voxels(self):
        return len(self.v)

    def coarsen(self, src_leaf, rec, src_moments=None, unchecked=False):
        """rec: the finer map's records under the readers' names (key, count, sums, with moments E and M, optionally seen
        and miss, which only the mutation looks at); src_moments: whether the finer map has distributions (default: as
        this one); unchecked: the moments' arithmetic at a leaf whose moments the contract refuses, to show why"""
        src_moments = self.moments if src_moments is None else src_moments
        j = shift_of(src_leaf, self.leaf)
        if j is None:
            raise ValueError("the leaves do not nest")
        if src_moments != self.moments:
            raise ValueError("distributions on one side only")
        if self.moments and not moments_split(src_leaf) and not unchecked:
            raise ValueError("floor(d / 16) does not split")
        unit = int(round(src_leaf * 2.0 ** 20)) // 16 if self.moments else 0         # L / 16
        if self.mutation == MUT_FULL_L:
            unit *= 16
        for i in range(len(rec["key"])):
            cell = cells_of(rec["key"][i])
            if self.mutation == MUT_TRUNCATE:
                parent = [int(c / 2 ** j) for c in cell]                               # towards zero
            else:
                parent = [c >> j for c in cell]                                        # Python's shift floors
            n = int(rec["count"][i])
            r = self.v.setdefault(key_of(*parent), [0, [0, 0, 0], [0, 0, 0], [0] * 6, 0, 0])
            r[0] += n
            for k in range(3):
                r[1][k] += int(rec["sums"][i][k])
            if self.moments:
                s = [(cell[k] - (parent[k] << j)) * unit for k in range(3)]
                E = [int(x) for x in rec["E"][i]]
                for k in range(3):
                    r[2][k] += E[k] + n * s[k]
                for m, (k, l) in enumerate(PAIRS):
                    cross = 0 if self.mutation == MUT_NO_CROSS else s[k] * E[l] + s[l] * E[k]
                    r[3][m] += int(rec["M"][i][m]) + cross + n * s[k] * s[l]
            if self.mutation == MUT_ADD_CARVE and "seen" in rec:
                r[4] += int(rec["seen"][i])
                r[5] += int(rec["miss"][i])
            self.n_points += n

    def records(self):
        """what the key-ordered readers return: key u64, count u32, sums [n, 3], E [n, 3], M [n, 6] i64, seen, miss u32"""
        ks = sorted(self.v)
        rows = [self.v[k] for k in ks]
        n = len(ks)
        return dict(key=np.array(ks, np.uint64).reshape(n), count=np.array([r[0] & U32 for r in rows], np.uint32).reshape(n),
                    sums=np.array([[i64(x) for x in r[1]] for r in rows], np.int64).reshape(n, 3),
                    E=np.array([[i64(x) for x in r[2]] for r in rows], np.int64).reshape(n, 3),
                    M=np.array([[i64(x) for x in r[3]] for r in rows], np.int64).reshape(n, 6),
                    seen=np.array([r[4] & U32 for r in rows], np.uint32).reshape(n), miss=np.array([r[5] & U32 for r in rows], np.uint32).reshape(n))


def coarsened(src_leaf, dst_leaf, recs, moments, mutation=MUT_NONE):
    """the records of an empty coarser map after coarsening each of `recs` into it"""
    m = CoarseMap(dst_leaf, moments, mutation)
    for rec in recs if isinstance(recs, (list, tuple)) else [recs]:
        m.coarsen(src_leaf, rec)
    return m.records()


def same_records(got, want, fields):
    return all(got[f].dtype == want[f].dtype and got[f].shape == want[f].shape and got[f].tobytes() == want[f].tobytes() for f in fields)


# ------------------------------------------------------------------ inputs
def eight_children(leaf=1.0, parent=(-1, 0, 2)):
    """A parent at 2 leaf with all eight children occupied, one point each at the child's corner + (1/4, 1/2, 3/4) leaf.
    With u = L / 16: e = (u / 4, u / 2, 3 u / 4) in every child and s = o u with o in {0, 1}^3, so by hand
    E'_k = 8 e_k + 4 u and M'_kl = sum over o of (e_k + o_k u) (e_l + o_l u).  At leaf 1, u = 65 536:
    E' = (393 216, 524 288, 655 360) and M'_xx = 4 * 16 384^2 + 4 * 81 920^2 = 27 917 287 424."""
    pts, cells = [], []
    for oz in (0, 1):
        for oy in (0, 1):
            for ox in (0, 1):
                c = (2 * parent[0] + ox, 2 * parent[1] + oy, 2 * parent[2] + oz)
                cells.append(c)
                pts.append(((c[0] + 0.25) * leaf, (c[1] + 0.5) * leaf, (c[2] + 0.75) * leaf))
    u = int(round(leaf * 2.0 ** 20)) // 16
    e = (u // 4, u // 2, 3 * u // 4)
    E = [8 * e[k] + 4 * u for k in range(3)]
    M = [sum((e[k] + ((o >> k) & 1) * u) * (e[l] + ((o >> l) & 1) * u) for o in range(8)) for k, l in PAIRS]
    return np.array(pts, F), cells, key_of(*parent), E, M


def around_zero(leaf=0.25):
    """Two points in each of the cells -9 .. 8 on x (y in cell -1, z in cell 0): for shifts 1, 2 and 3 the cells -1, -2 and
    2^j - 1 and their neighbours on both sides of zero.  Truncation sends cell -1 to parent 0, where floor says -1."""
    xs = [(c + f) * leaf for c in range(-9, 9) for f in (0.25, 0.625)]
    return np.array([(x, -0.5 * leaf, 0.5 * leaf) for x in xs], F)


def parent_corner(leaf=0.25):
    """A point exactly on the corner of the parent (1, -1, 0) at 2 leaf: child cell (2, -2, 0), o = 0 and e = 0 on every
    axis, so every moment stays zero; and a second point of the same parent in child (3, -1, 1)."""
    return np.array([(2 * leaf, -2 * leaf, 0.0), (3.5 * leaf, -0.75 * leaf, 1.25 * leaf)], F)


def chain(n):
    """n points, one per voxel at leaf 0.25, filling parents at 0.5 two by two along x (negative cells included)"""
    c = np.arange(n, dtype=np.float64) - n // 2
    return np.stack([(c + 0.3) * 0.25, np.full(n, -0.1), np.full(n, 0.6)], axis=1).astype(F)


FOUR_CLOUDS = K.FOUR_CLOUDS
ORDERS = K.ORDERS
SIZES = K.SIZES
