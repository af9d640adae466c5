"""Host restatements of include/lidargs_knn.h (tests/test_knn_cpu.py, tests/test_knn_gpu.py).

dist3_brute      the distCUDA2 contract in numpy float32, all pairs (small clouds)
dist3_kdtree     the same from 8 cKDTree candidates per point re-evaluated in float32, with dist3_brute's rule for every point whose
                 float32 third best is not clearly below the float64 8th candidate (large clouds)
voxelize_reference    the reference expression np.unique(np.round(data / voxel_size), axis=0) * voxel_size (after its shuffle)
voxelize_restatement  the device's arithmetic in numpy: int64 keys relative to the minimum, packed into 32-bit words, LSD order
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def _finish(best):
    """best: float32 [n, >=3] candidate distances (FLT_MAX = none) -> ((b0 + b1) + b2) / 3 in float32."""
    if best.shape[1] < 3:
        best = np.concatenate([best, np.full((best.shape[0], 3 - best.shape[1]), FLT_MAX, np.float32)], 1)
    b = np.sort(np.partition(best, 2, axis=1)[:, :3], axis=1) if best.shape[1] > 3 else np.sort(best, axis=1)
    with np.errstate(over="ignore"):
        return ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3.0)


def _sqd(q, p):
    """float32 d = dx*dx + dy*dy + dz*dz, dx = p.x - q.x, broadcast; not-below-FLT_MAX and NaN -> FLT_MAX."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = p[..., 0] - q[..., 0]; dy = p[..., 1] - q[..., 1]; dz = p[..., 2] - q[..., 2]
        d = (dx * dx + dy * dy) + dz * dz
    return np.where(d < FLT_MAX, d, FLT_MAX).astype(np.float32)


def dist3_brute(x, rows=None, chunk=512):
    """The contract for the points `rows` (default all) of float32 x [P, 3], every other point a candidate."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    P = x.shape[0]
    rows = np.arange(P) if rows is None else np.asarray(rows)
    out = np.empty(rows.shape[0], np.float32)
    for a in range(0, rows.shape[0], chunk):
        r = rows[a:a + chunk]
        d = _sqd(x[r][:, None, :], x[None, :, :])
        d[np.arange(r.shape[0]), r] = FLT_MAX                          # self, by index
        out[a:a + chunk] = _finish(d)
    return out


def dist3_kdtree(x, workers=16, margin=4e-6):
    """dist3_brute for large finite-heavy clouds: the 3 best float32 distances among the 8 float64-nearest candidates (self removed by index)
    are the true 3 best unless a point outside them can round below: every outside point has float64 distance >= D8, hence float32 distance
    >= D8 (1 - ~1e-6); points whose float32 third best is not below D8 (1 - margin), or that have fewer than 8 finite candidates, go to
    brute force.  Returns (result, number of brute-forced points)."""
    from scipy.spatial import cKDTree
    x = np.ascontiguousarray(x, dtype=np.float32)
    P = x.shape[0]
    fin = np.isfinite(x).all(1)
    out = np.full(P, np.float32(np.inf), np.float32)
    idx_f = np.nonzero(fin)[0]
    xf = x[idx_f].astype(np.float64)
    tree = cKDTree(xf)
    k = min(9, xf.shape[0])
    D, I = tree.query(xf, k=k, workers=workers)
    D, I = D.reshape(len(idx_f), k), I.reshape(len(idx_f), k)
    gi = idx_f[I]                                                      # global indices of the candidates
    selfpos = gi == idx_f[:, None]
    has_self = selfpos.any(1)
    drop = np.where(has_self, np.argmax(selfpos, 1), k - 1)            # self, or (duplicates hid it) the farthest candidate
    keep = np.ones_like(selfpos); keep[np.arange(len(idx_f)), drop] = False
    cand = gi[keep].reshape(len(idx_f), k - 1)
    d64 = D[keep].reshape(len(idx_f), k - 1)
    d32 = _sqd(x[idx_f][:, None, :], x[cand])
    res = _finish(d32)
    b3 = np.sort(d32, 1)[:, 2] if k - 1 >= 3 else np.full(len(idx_f), FLT_MAX, np.float32)
    D8 = (d64[:, -1] ** 2) if k - 1 >= 1 else np.zeros(len(idx_f))
    unsure = (k < 9) | ~(b3.astype(np.float64) <= D8 * (1.0 - margin))
    out[idx_f] = res
    bad = idx_f[unsure]
    if bad.size:
        out[bad] = dist3_brute(x, bad, chunk=16)
    return out, int(bad.size)


def voxelize_reference(data, voxel_size):
    return np.unique(np.round(data / voxel_size), axis=0) * voxel_size


def voxelize_restatement(data, voxel_size):
    """What csrc/knn.hip computes, in numpy: q = rint(data / v) in the precision numpy uses for data / v, int64 per axis, key = the axes'
    offsets from their minimum packed MSB-first (x most significant) into the bits their spans need, sorted LSD over 32-bit words
    (stable), groups of equal keys, out = q * v.  Returns (rows, number of 32-bit words of the key)."""
    q = np.round(data / voxel_size)
    dt = q.dtype
    v = dt.type(voxel_size)
    P = q.shape[0]
    if P == 0:
        return np.empty((0, 3), dt), 0
    if not np.isfinite(q).all() or np.abs(q).max() >= 2.0 ** 62:
        raise RuntimeError("voxelize_sample: a row is not finite, or data / voxel_size reaches 2^62")
    qi = q.astype(np.int64)
    mn = qi.min(0)
    u = [(qi[:, c] - mn[c]).astype(np.uint64) for c in range(3)]
    bits = [int(u[c].max()).bit_length() for c in range(3)]
    shift = [bits[1] + bits[2], bits[2], 0]
    total = sum(bits)
    words = (total + 31) // 32
    perm = np.arange(P)
    for w in range(words):
        lo = 32 * w
        word = np.zeros(P, np.uint64)
        for c in range(3):
            a, e = shift[c], shift[c] + bits[c]
            if bits[c] == 0 or e <= lo or a >= lo + 32:
                continue
            uc = u[c][perm]
            word |= (uc << np.uint64(a - lo)) if a >= lo else (uc >> np.uint64(lo - a))
        word &= np.uint64(0xFFFFFFFF)
        perm = perm[np.argsort(word, kind="stable")]
    s = qi[perm]
    head = np.ones(P, bool)
    head[1:] = (s[1:] != s[:-1]).any(1)
    return s[head].astype(dt) * v, words
