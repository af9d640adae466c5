"""A numpy restatement of the integer stage of csrc/binning.hip between and behind its sorts: the exclusive scan, the instance emit
and the tile ranges.  Vectorised (13 M instances in about a second); tests/test_binning_cpu.py holds it against a brute-force loop over
tiles, tests/test_binning_gpu.py holds the kernels against it, word for word.

A span record is (xspan, rowspan) = (x0 | x1 << 16, lo | hi << 16): tile columns [x0, x1) of 16 pixels, pixel rows [lo, hi); xspan == 0
says "no instances", whatever the row span holds.  x1 may pass tiles_x (a span across the seam of the panorama): the columns behind the
seam are x - tiles_x.  With tile height th = 1 << sh the span touches the tile rows lo >> sh .. (hi - 1) >> sh."""
import numpy as np

SCAN_BLOCK = 1024           # records per block of the instance offsets / elements per block of the scan
NO_CAP = 0xFFFFFFFF
EMPTY_COMPACT = 0xFFFFFFFF


def scan(x):
    """(exclusive prefix sums cut to 32 bits, total cut to 32 bits) of u32 x."""
    c = np.cumsum(x.astype(np.uint64), dtype=np.uint64)
    out = np.zeros(x.size, np.uint64)
    out[1:] = c[:-1]
    total = int(c[-1]) if x.size else 0
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32), total & 0xFFFFFFFF


def _shift(th):
    sh = int(th).bit_length() - 1
    assert th == 1 << sh
    return sh


def fields(spans):
    """(x0, x1, lo, hi) as int64 columns of u32[P][2] records."""
    s = np.asarray(spans, np.uint32).reshape(-1, 2).astype(np.int64)
    return s[:, 0] & 0xFFFF, s[:, 0] >> 16, s[:, 1] & 0xFFFF, s[:, 1] >> 16


def make_spans(x0, x1, lo, hi):
    """u32[P][2] records from the four fields (arrays or scalars, broadcast)."""
    x0, x1, lo, hi = np.broadcast_arrays(*(np.atleast_1d(np.asarray(a, np.int64)) for a in (x0, x1, lo, hi)))
    assert (x0 >= 0).all() and (x1 <= 0xFFFF).all() and (lo >= 0).all() and (hi <= 0xFFFF).all()
    return np.stack([x0 | (x1 << 16), lo | (hi << 16)], 1).astype(np.uint32)


def counts(spans, th):
    """Instances of every record: (x1 - x0) * (tile rows touched); 0 for an empty column span."""
    sh = _shift(th)
    x0, x1, lo, hi = fields(spans)
    cols = x1 - x0
    rows = ((hi - 1) >> sh) - (lo >> sh) + 1
    return np.where(cols > 0, cols * rows, 0)


def block_counts(spans, th):
    """Instances of every block of SCAN_BLOCK consecutive records."""
    c = counts(spans, th)
    nb = (c.size + SCAN_BLOCK - 1) // SCAN_BLOCK
    return np.concatenate([c, np.zeros(nb * SCAN_BLOCK - c.size, np.int64)]).reshape(nb, SCAN_BLOCK).sum(1)


def emit(ids, spans, th, tiles_x, cap=NO_CAP):
    """(tile ids, values, total): the instance list of the records in order -- per record row-major (tile row outer, column inner),
    tile = ((lo >> sh) + ry) * tiles_x + (x0 + rx, minus tiles_x once if >= tiles_x), value = ids[i] -- cut to min(total, cap)."""
    sh = _shift(th)
    x0, x1, lo, _ = fields(spans)
    cnt = counts(spans, th)
    total = int(cnt.sum())
    m = min(total, int(cap))
    start = np.cumsum(cnt) - cnt
    last = int(np.searchsorted(start, m, side="left"))                 # records that start in front of the cut
    own = np.repeat(np.arange(last, dtype=np.int64), cnt[:last])[:m]
    jj = np.arange(m, dtype=np.int64) - start[own]
    cols = (x1 - x0)[own]
    ry = jj // np.maximum(cols, 1)
    tx = x0[own] + (jj - ry * cols)
    tx -= np.where(tx >= tiles_x, tiles_x, 0)
    tile = ((lo >> sh)[own] + ry) * tiles_x + tx
    return tile.astype(np.uint32), np.asarray(ids, np.uint32)[own], total


def pack_compact(spans):
    """The 4-byte form of the records: x0 | (x1 - x0 - 1) << 8 | lo << 16 | (hi - 1) << 24, 0xFFFFFFFF for "no instances"."""
    x0, x1, lo, hi = fields(spans)
    full = x1 > x0
    assert (x0[full] <= 255).all() and (x1[full] - x0[full] <= 256).all() and (lo[full] <= 255).all() and (hi[full] >= 1).all() and (hi[full] <= 256).all()
    w = x0 | ((x1 - x0 - 1) << 8) | (lo << 16) | ((hi - 1) << 24)
    assert not (w[full] == EMPTY_COMPACT).any(), "x0 = 255, x1 = 511, lo = 255, hi = 256 has no compact form"
    return np.where(full, w, EMPTY_COMPACT).astype(np.uint32)


def unpack_compact(words):
    """u32[P][2] records of the 4-byte form; "no instances" comes back as (0, 0)."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    x0, nx, lo, hi = w & 255, ((w >> 8) & 255) + 1, (w >> 16) & 255, (w >> 24) + 1
    s = make_spans(x0, x0 + nx, lo, hi)
    s[w == EMPTY_COMPACT] = 0
    return s


def ranges(keys_sorted, R, tiles):
    """u32[tiles][2] = (first, last + 1) position of every tile among the first R ascending keys, (0, 0) for a tile without keys."""
    k = np.asarray(keys_sorted)[:R].astype(np.int64)
    t = np.arange(tiles, dtype=np.int64)
    first, end = np.searchsorted(k, t, side="left"), np.searchsorted(k, t, side="right")
    some = end > first
    return np.stack([np.where(some, first, 0), np.where(some, end, 0)], 1).astype(np.uint32)


def tile_lists(ids, spans, th, tiles_x, tiles):
    """The chain a frame runs: emit -> stable sort by tile -> ranges.  (values in tile order, ranges)."""
    tile, val, total = emit(ids, spans, th, tiles_x)
    perm = np.argsort(tile, kind="stable")
    return val[perm], ranges(tile[perm], total, tiles)


# ---- records for the tests (both the CPU test of this file and the GPU test use them) ---------------------------------------------------
def random_spans(rng, P, tiles_x, H, compact=False, empty=0.2, seam=0.1):
    """Valid random records on a tiles_x x H grid: mostly narrow, some wide, `seam` of them across the seam (x1 > tiles_x, never wider
    than the grid), `empty` of them without instances -- with a random row span, which must not be looked at (0 rows included)."""
    nx = np.where(rng.random(P) < 0.1, rng.integers(1, tiles_x + 1, P), rng.integers(1, min(tiles_x, 6) + 1, P))
    x0 = rng.integers(0, tiles_x, P)
    wrap = rng.random(P) < seam
    x0 = np.where(wrap, x0, np.minimum(x0, tiles_x - nx))              # x1 <= tiles_x unless the span wraps
    lo = rng.integers(0, H, P)
    hi = np.where(rng.random(P) < 0.5, lo + 1 + rng.integers(0, 9, P), rng.integers(1, H + 1, P))
    hi = np.minimum(np.maximum(hi, lo + 1), H)
    if compact:                                                         # the one record the 4-byte form cannot hold
        clash = (x0 == 255) & (nx == 256) & (lo == 255) & (hi == 256)
        lo = np.where(clash, 254, lo)
    s = make_spans(x0, x0 + nx, lo, hi)
    none = rng.random(P) < empty
    s[none, 0] = 0
    s[none, 1] = rng.integers(0, 1 << 32, int(none.sum()), dtype=np.uint64).astype(np.uint32)
    if compact:
        s[none, 1] = 0                                                  # (what the 4-byte form brings back)
    return s


def row_edge_spans(th, H, tiles_x):
    """lo and hi on, one below and one above every multiple of th in [0, H], every pair with hi > lo; 1..3 columns, some across the seam."""
    v = np.unique(np.clip(np.concatenate([np.arange(0, H + 1, th) + d for d in (-1, 0, 1)]), 0, H))
    lo, hi = np.meshgrid(v[v < H], v[v >= 1], indexing="ij")
    keep = hi > lo
    lo, hi = lo[keep], hi[keep]
    k = np.arange(lo.size)
    nx = 1 + k % 3
    x0 = (k * 7) % tiles_x
    return make_spans(x0, x0 + nx, lo, hi)


def column_edge_spans(tiles_x, H, th):
    """x1 == tiles_x, x1 == tiles_x + 1, x0 == tiles_x - 1 with a span as wide as the grid, x0 = 0 and x0 = tiles_x as wide as the
    grid, single columns at both ends: each over one, two and all tile rows."""
    cols = [(tiles_x - 1, tiles_x), (tiles_x - 3, tiles_x), (0, tiles_x), (tiles_x - 1, tiles_x + 1), (tiles_x - 2, tiles_x + 1), (1, tiles_x + 1),
            (tiles_x - 1, 2 * tiles_x - 1), (tiles_x - 1, 2 * tiles_x - 2), (0, 1)]
    if 2 * tiles_x <= 0xFFFF and tiles_x <= 255:
        cols.append((tiles_x, 2 * tiles_x))
    rows = [(0, 1), (th - 1, th + 1), (0, H), (H - 1, H)]
    return np.concatenate([make_spans(a, b, lo, hi) for a, b in cols for lo, hi in rows])
