"""The voxel map's absorb and snapshot file restated in Python (docs/VOXEL_MAP.md section 10): a dict of Python ints for the
records, and a writer and a reader of the version 1 file written from the table of section 10.4 with `struct`, not from the
C++.  tests/test_vmap_snapshot.py holds the library's parser to it without a device, tests/test_gpu_vmap_snapshot.py the
device."""
import math
import struct

import numpy as np

ALL_ONES = (1 << 64) - 1
FIELD = (1 << 21) - 1
CARVE, MOMENTS = 1, 2
HEADER = 96
U32, U64 = (1 << 32) - 1, (1 << 64) - 1


def key_of(ix, iy, iz):
    return ((int(iz) + (1 << 20)) << 42) | ((int(iy) + (1 << 20)) << 21) | (int(ix) + (1 << 20))


def key_valid(k):
    """section 1's keys: not all ones, bit 63 clear, no 21-bit field above 2^21 - 2"""
    k = int(k)
    return k != ALL_ONES and not k >> 63 and all((k >> s) & FIELD <= FIELD - 1 for s in (0, 21, 42))


def i64(v):
    """a Python int as the int64 the device's wrapping add leaves"""
    v &= U64
    return v - (1 << 64) if v >> 63 else v


class RefMap:
    """absorb on a dict: key -> [count, [3 sums], seen, miss, [3 E], [6 M]], all Python ints"""

    def __init__(self, moments=False, carved=False):
        self.v, self.moments, self.carved = {}, moments, carved
        self.n_points = 0

    @property
    def n_voxels(self):
        return len(self.v)

    def absorb(self, key, count, sums, seen=None, miss=None, E3=None, M6=None):
        """the number of records rejected; ValueError where the library answers SLAM_E_INVALID"""
        if (seen is None) != (miss is None) or (E3 is None) != (M6 is None):
            raise ValueError("half a pair")
        n = len(key)
        if n == 0:
            return 0
        if (E3 is not None) != self.moments:
            raise ValueError("moments must match the map")
        if seen is not None:
            self.carved = True
        sums = np.asarray(sums).reshape(n, 3)
        rejected = 0
        for i in range(n):
            k, c = int(key[i]), int(count[i])
            if not key_valid(k) or c == 0:
                rejected += 1
                continue
            r = self.v.setdefault(k, [0, [0, 0, 0], 0, 0, [0, 0, 0], [0] * 6])
            r[0] += c
            for a in range(3):
                r[1][a] += int(sums[i][a])
            if seen is not None:
                r[2] += int(seen[i])
                r[3] += int(miss[i])
            if E3 is not None:
                e, m = np.asarray(E3).reshape(n, 3)[i], np.asarray(M6).reshape(n, 6)[i]
                for a in range(3):
                    r[4][a] += int(e[a])
                for a in range(6):
                    r[5][a] += int(m[a])
            self.n_points += c
        return rejected

    def records(self):
        """what the key-ordered readers return: dict of key u64, count u32, sums i64 [n, 3], seen, miss u32, E [n, 3], M [n, 6] i64"""
        ks = sorted(self.v)
        rows = [self.v[k] for k in ks]
        n = len(ks)
        return dict(key=np.array(ks, np.uint64).reshape(n), count=np.array([r[0] & U32 for r in rows], np.uint32).reshape(n),
                    sums=np.array([[i64(s) for s in r[1]] for r in rows], np.int64).reshape(n, 3),
                    seen=np.array([r[2] & U32 for r in rows], np.uint32).reshape(n), miss=np.array([r[3] & U32 for r in rows], np.uint32).reshape(n),
                    E=np.array([[i64(s) for s in r[4]] for r in rows], np.int64).reshape(n, 3),
                    M=np.array([[i64(s) for s in r[5]] for r in rows], np.int64).reshape(n, 6))


DEFAULT_DIST = dict(min_points=6, flat_ratio=4.0, line_ratio=0.01, epsilon=1e-3, max_miss_num=0, max_miss_den=0)


def payload_bytes(n, flags):
    return 8 * n + (4 * n + 7) // 8 * 8 + 24 * n + (8 * n if flags & CARVE else 0) + (72 * n if flags & MOMENTS else 0)


def write_file(leaf, rec, n_points=None, carved=False, dist=None):
    """The bytes of a version 1 file.  rec: the dict of RefMap.records() (or the readers' arrays under the same names);
    carved: seen and miss travel; dist: the distribution parameters (a dict) when E and M travel."""
    key = np.ascontiguousarray(rec["key"], "<u8")
    n = len(key)
    flags = (CARVE if carved else 0) | (MOMENTS if dist is not None else 0)
    count = np.ascontiguousarray(rec["count"], "<u4")
    if n_points is None:
        n_points = int(count.astype(np.uint64).sum())
    d = dist or dict(min_points=0, flat_ratio=0.0, line_ratio=0.0, epsilon=0.0, max_miss_num=0, max_miss_den=0)
    head = struct.pack("<8sIIdqqiiiIdddQQ", b"SLAMVMAP", 1, flags, float(leaf), n, int(n_points), d["min_points"], d["max_miss_num"],
                       d["max_miss_den"], 0, d["flat_ratio"], d["line_ratio"], d["epsilon"], payload_bytes(n, flags), 0)
    assert len(head) == HEADER
    out = [head, key.tobytes(), count.tobytes(), b"\0" * ((4 * n + 7) // 8 * 8 - 4 * n), np.ascontiguousarray(rec["sums"], "<i8").tobytes()]
    if carved:
        out += [np.ascontiguousarray(rec["seen"], "<u4").tobytes(), np.ascontiguousarray(rec["miss"], "<u4").tobytes()]
    if dist is not None:
        out += [np.ascontiguousarray(rec["E"], "<i8").tobytes(), np.ascontiguousarray(rec["M"], "<i8").tobytes()]
    return b"".join(out)


def read_file(b):
    """The fields and arrays of a valid file as a dict; ValueError (with the rule) for any other bytes."""
    def need(ok, why):
        if not ok:
            raise ValueError(why)
    need(len(b) >= HEADER, "shorter than the header")
    (magic, version, flags, leaf, n, n_points, min_points, miss_num, miss_den, zero32, flat, line, eps, payload,
     zero64) = struct.unpack("<8sIIdqqiiiIdddQQ", b[:HEADER])
    need(magic == b"SLAMVMAP", "magic")
    need(version == 1, "version")
    need(flags & ~3 == 0, "unknown flags")
    need(zero32 == 0 and zero64 == 0, "reserved fields")
    need(math.isfinite(leaf) and leaf > 0, "leaf")
    if flags & MOMENTS:
        need(leaf <= 8.0, "leaf above 8 with moments")
        need(min_points >= 1 and flat >= 0 and line >= 0 and eps > 0 and miss_num >= 0 and miss_den >= 0, "distribution parameters")
    else:
        need(b[40:80] == b"\0" * 40, "offsets 40 .. 79 without moments")
    need(0 <= n <= 1 << 30, "n")
    need(payload == payload_bytes(n, flags), "payload figure")
    need(len(b) == HEADER + payload, "length")
    o = HEADER

    def take(dt, m, room=None):
        nonlocal o
        a = np.frombuffer(b, dt, m, o)
        o += a.nbytes if room is None else room
        return a
    out = dict(flags=flags, leaf=leaf, n=n, n_points=n_points, key=take("<u8", n))
    pad_from = o + 4 * n
    out["count"] = take("<u4", n, (4 * n + 7) // 8 * 8)
    need(b[pad_from:o] == b"\0" * (o - pad_from), "padding")
    out["sums"] = take("<i8", 3 * n).reshape(n, 3)
    if flags & CARVE:
        out["seen"], out["miss"] = take("<u4", n), take("<u4", n)
    if flags & MOMENTS:
        out["E"], out["M"] = take("<i8", 3 * n).reshape(n, 3), take("<i8", 6 * n).reshape(n, 6)
        out["dist"] = dict(min_points=min_points, flat_ratio=flat, line_ratio=line, epsilon=eps, max_miss_num=miss_num, max_miss_den=miss_den)
    keys = [int(k) for k in out["key"]]
    need(all(key_valid(k) for k in keys), "a key section 1 does not allow")
    need(all(a < c for a, c in zip(keys, keys[1:])), "keys not strictly ascending")
    need(all(int(c) >= 1 for c in out["count"]), "a zero count")
    need(sum(int(c) for c in out["count"]) == n_points, "n_points")
    return out


def valid(b):
    try:
        read_file(b)
        return True
    except ValueError:
        return False


def small_records(n=5, seed=11):
    """n records with every plane filled, keys ascending: the good file of the CPU tests (n = 5: an odd count array, so padding)"""
    rng = np.random.default_rng(seed)
    cells = sorted({(int(a), int(b), int(c)) for a, b, c in rng.integers(-40, 40, (4 * n, 3))}, key=lambda c: key_of(*c))[:n]
    key = np.array(sorted(key_of(*c) for c in cells), np.uint64)
    return dict(key=key, count=rng.integers(1, 900, n).astype(np.uint32), sums=rng.integers(-2 ** 40, 2 ** 40, (n, 3)),
                seen=rng.integers(0, 9, n).astype(np.uint32), miss=rng.integers(0, 9, n).astype(np.uint32),
                E=rng.integers(-2 ** 30, 2 ** 30, (n, 3)), M=rng.integers(0, 2 ** 50, (n, 6)))


def _patched(b, off, fmt, value):
    return b[:off] + struct.pack(fmt, value) + b[off + struct.calcsize(fmt):]


def malformed_files(leaf=1.0):
    """name -> bytes, each broken in one way; built from the good file of small_records() with both flags"""
    rec = small_records()
    n = len(rec["key"])
    good = write_file(leaf, rec, carved=True, dist=DEFAULT_DIST)
    k0 = HEADER                                  # the keys
    c0 = HEADER + 8 * n                          # the counts
    out = {"bad_magic": b"SLAMVMAQ" + good[8:], "version_2": _patched(good, 8, "<I", 2), "unknown_flag": _patched(good, 12, "<I", 7),
           "truncated_by_one": good[:-1], "one_too_long": good + b"\0",
           "keys_equal": _patched(good, k0 + 8, "<Q", int(rec["key"][0])),
           "keys_descending": _patched(_patched(good, k0, "<Q", int(rec["key"][1])), k0 + 8, "<Q", int(rec["key"][0])),
           "field_of_2p21_minus_1": _patched(good, k0 + 8 * (n - 1), "<Q", (int(rec["key"][n - 1]) & ~(FIELD << 21)) | (FIELD << 21)),
           "bit_63": _patched(good, k0 + 8 * (n - 1), "<Q", int(rec["key"][n - 1]) | 1 << 63),
           "zero_count": _patched(good, c0 + 4, "<I", 0),
           "n_points_off_by_one": _patched(good, 32, "<q", int(rec["count"].sum()) + 1),
           "padding_not_zero": _patched(good, c0 + 4 * n, "<I", 1),
           "leaf_zero": _patched(good, 16, "<d", 0.0), "leaf_nan": _patched(good, 16, "<d", float("nan")),
           "leaf_9_with_moments": _patched(good, 16, "<d", 9.0), "n_minus_one": _patched(good, 24, "<q", -1)}
    assert n % 2 == 1 and all(b != good for b in out.values())
    return good, out


def carve_example():
    """Section 10.1's hand-worked pair of maps.  Voxels X and Y; two scans.  Scan 1 has an endpoint in X and crosses nothing;
    scan 2 has an endpoint in Y and its ray crosses X.
      one map, both scans:     after scan 1  X (seen 1, miss 0);  after scan 2  X (1, 1), Y (1, 0)
      map A takes scan 1, map B scan 2: B never holds X, and a carve charges existing voxels only, so scan 2's miss on X is
      lost:                    A: X (1, 0);   B: Y (1, 0);   absorbed: X (1, 0), Y (1, 0)
    The sum equals the joint carve on Y, which every contributing map that saw it held, and differs on X."""
    X, Y = key_of(1, 0, 0), key_of(3, 0, 0)
    joint = {X: (1, 1), Y: (1, 0)}
    a = dict(key=[X], count=[1], sums=[[1, 0, 0]], seen=[1], miss=[0])
    b = dict(key=[Y], count=[1], sums=[[3, 0, 0]], seen=[1], miss=[0])
    return X, Y, joint, a, b
