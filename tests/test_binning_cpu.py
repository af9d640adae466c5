"""tests/binning_ref.py, the numpy restatement the GPU tests of the scan, the instance emit and the tile ranges compare against, held
against a brute-force loop: for every tile, the Gaussians in range order whose span covers it, the seam wrap included.  It shares no
arithmetic with the restatement (no division, no instance positions): a tile row is covered if the span's pixel rows and the tile's overlap,
a tile column if it or its image behind the seam lies in [x0, x1)."""
import numpy as np
import pytest

import binning_ref as ref


def brute_force_lists(ids, spans, th, tiles_x, tiles_y):
    lists = []
    recs = [tuple(int(v) for v in r) for r in np.stack(ref.fields(spans), 1)]
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            here = []
            for i, (x0, x1, lo, hi) in enumerate(recs):
                if x1 <= x0:
                    continue
                if not (lo < (ty + 1) * th and hi > ty * th):           # pixel rows [lo, hi) against the tile's [ty th, (ty + 1) th)
                    continue
                here += [int(ids[i])] * ((x0 <= tx < x1) + (x0 <= tx + tiles_x < x1))
            lists.append(here)
    return lists


def check_chain(spans, th, tiles_x, tiles_y, rng):
    P = spans.shape[0]
    ids = (rng.permutation(P) * 5 + 2).astype(np.uint32)
    want = brute_force_lists(ids, spans, th, tiles_x, tiles_y)
    vals, rg = ref.tile_lists(ids, spans, th, tiles_x, tiles_x * tiles_y)
    assert vals.size == sum(len(w) for w in want) == int(ref.counts(spans, th).sum())
    for t, w in enumerate(want):
        first, end = (int(v) for v in rg[t])
        if not w:
            assert (first, end) == (0, 0), t
        else:
            assert end - first == len(w) and vals[first:end].tolist() == w, (t, first, end)


@pytest.mark.parametrize("th", [4, 8, 16, 32])
def test_random_records(th):
    rng = np.random.default_rng(th)
    tiles_x, H = 11, 70                                                 # (the last tile row is a partial one at every height)
    check_chain(ref.random_spans(rng, 300, tiles_x, H, seam=0.3), th, tiles_x, (H + th - 1) // th, rng)


@pytest.mark.parametrize("th", [4, 8, 16, 32])
def test_edge_records(th):
    rng = np.random.default_rng(th + 100)
    tiles_x, H = 7, 2 * th + 3
    tiles_y = (H + th - 1) // th
    check_chain(ref.row_edge_spans(th, H, tiles_x), th, tiles_x, tiles_y, rng)
    check_chain(ref.column_edge_spans(tiles_x, H, th), th, tiles_x, tiles_y, rng)


def test_emit_order_and_cut():
    """Row-major inside a record, records in order; the cut keeps the first min(total, cap) instances and reports the whole need."""
    spans = ref.make_spans([2, 0, 4], [5, 0, 7], [3, 9, 0], [9, 9, 1])    # 3 columns x tile rows 0..2 at th 4; empty; columns 4, 5, 0 (seam at 6)
    ids = np.array([70, 80, 90], np.uint32)
    tile, val, total = ref.emit(ids, spans, 4, 6)
    assert total == 12 and tile.tolist() == [2, 3, 4, 8, 9, 10, 14, 15, 16, 4, 5, 0] and val.tolist() == [70] * 9 + [90] * 3
    for cap in (0, 1, 9, 10, 11, 12, 13, ref.NO_CAP):
        t, v, n = ref.emit(ids, spans, 4, 6, cap)
        assert n == 12 and t.tolist() == tile[:cap].tolist() and v.tolist() == val[:cap].tolist()
    assert ref.block_counts(spans, 4).tolist() == [12]


def test_compact_records_round_trip():
    rng = np.random.default_rng(7)
    spans = np.concatenate([ref.random_spans(rng, 2000, 256, 256, compact=True), ref.make_spans([255, 0, 255], [511, 256, 256], [254, 255, 255], [256, 256, 256])])
    assert np.array_equal(ref.unpack_compact(ref.pack_compact(spans)), spans)
    with pytest.raises(AssertionError):
        ref.pack_compact(ref.make_spans(255, 511, 255, 256))            # the word that says "no instances"


def test_scan_and_ranges():
    x = np.array([3, 0, 0xFFFFFFFF, 5, 0, 1], np.uint32)
    out, total = ref.scan(x)
    assert out.tolist() == [0, 3, 3, 2, 7, 7] and total == 8            # (cut to 32 bits)
    assert ref.scan(np.zeros(0, np.uint32))[1] == 0
    keys = np.array([1, 1, 4, 4, 4, 6, 0, 0], np.uint32)                # (the two behind R = 6 are not looked at)
    assert ref.ranges(keys, 6, 8).tolist() == [[0, 0], [0, 2], [0, 0], [0, 0], [2, 5], [0, 0], [5, 6], [0, 0]]
    assert ref.ranges(keys, 0, 3).tolist() == [[0, 0]] * 3
