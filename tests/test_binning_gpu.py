"""The integer stage of csrc/binning.hip between and behind its sorts -- the exclusive scan, the instance emit, the tile ranges --
word for word against the numpy restatement of tests/binning_ref.py (itself held against a brute-force loop by tests/test_binning_cpu.py).

The library's own launchers are reached through the test hooks of the C ABI (`lidargs_debug_exclusive_scan`,
`lidargs_debug_emit_instances`, `lidargs_debug_tile_ranges`) at the smallest shapes at which a branch changes:

    scan      one / two / three trips of k_scan_partials (1 048 576 | 1 048 577 | 2 097 159 elements), in place, with and without a total
    emit      4- and 8-byte span records, 16- and 32-bit tile keys, block sums scanned or added up by the emit itself; the windows of a
              wave (owners by carry, empty waves and blocks); tile rows at every multiple of the tile height; the seam; the float
              reciprocal for every width 1..256 and across its switch to the integer division at 2^22; the capacity cut
    ranges    16-byte loads behind R, a count on the device, prezeroed and self-zeroing, the work-list counters
    chain     emit -> tile sort -> ranges on 20 000 records, per key width

Every comparison is `np.array_equal` on integers.  Every device array lies between 64 guard words that must come back untouched (`Buf`
of tests/test_sort_gpu.py); outputs start out as 0xFF bytes and are exactly as long as what must be written.

The float branch of the division runs every width 1..256 with the 64 tile rows a compact record can span (2.1 M instances per form); with
the 16 384 rows a full record can span the same sweep would be 539 M instances, so the large quotients of the full form are those of
widths 1..3 over 16 384 rows and of the three records around 2^22."""
import ctypes as C

import numpy as np
import pytest

import binning_ref as ref
from test_sort_gpu import Buf, Pairs, _binding, _key_words, _same, _stream

pytestmark = pytest.mark.gpu

FORMS = [(0, 4), (0, 2), (1, 4), (1, 2)]       # (compact, key_bytes)
FORM_IDS = ["full_keys32", "full_keys16", "compact_keys32", "compact_keys16"]
GRID_X, GRID_H = 166, 64                       # a 2650 x 64 image: 166 x 16 tiles at tile height 4


def _sync():
    import torch
    torch.cuda.synchronize()


def _ids(rng, P):
    return (rng.permutation(P).astype(np.uint64) * 7 + 3).astype(np.uint32)     # distinct, not the positions


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = [0, 1, 255, 256, 1023, 1024, 1025, 4097, 1048576, 1048577, 2097159]
SCAN_KINDS = ["ones", "zeros", "flags_with_long_runs_of_zeros", "counts_0_to_15", "total_above_2_to_31"]


def _scan_input(kind, rng, n):
    if kind == "ones":
        return np.ones(n, np.uint32)
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "flags_with_long_runs_of_zeros":           # runs of 1500 and 2600 zeros (longer than one block, than two) between short runs of ones
        x = (np.arange(n) % 4211 < 111).astype(np.uint32)
        x[(np.arange(n) % 4211 >= 1611) & (np.arange(n) % 4211 < 1611 + 5)] = 1
        return x
    if kind == "counts_0_to_15":
        return rng.integers(0, 16, n).astype(np.uint32)
    if kind == "total_above_2_to_31":                     # 3.0e9 spread over the elements, the remainder on the last one
        x = np.full(n, 3_000_000_000 // max(n, 1), np.uint32)
        if n:
            x[-1] += np.uint32(3_000_000_000 - int(x.astype(np.uint64).sum()))
            assert (1 << 31) < int(x.astype(np.uint64).sum()) < (1 << 32)
        return x
    raise ValueError(kind)


def check_scan(x, with_total, in_place, what):
    lib = _binding()._lib
    n = x.size
    src = Buf(x)
    dst = src if in_place else Buf.filled(n)
    total = Buf.filled(1)
    scratch = Buf.filled(int(lib.lidargs_debug_scan_scratch_words(n)), 0xEE)      # (what a frame before left there)
    rc = lib.lidargs_debug_exclusive_scan(n, src.ptr, dst.ptr, total.ptr if with_total else None, scratch.ptr, _stream())
    assert rc == 0, (what, _binding()._err())
    _sync()
    want, want_total = ref.scan(x)
    scratch.read()
    _same(f"{what} scan", dst.read(), want)
    if not in_place:
        _same(f"{what} input", src.read(), x)
    _same(f"{what} total", total.read(), np.array([want_total if with_total else 0xFFFFFFFF], np.uint32))


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan(n, hip_lib_built):
    assert int(_binding()._lib.lidargs_debug_scan_scratch_words(n)) >= (n + 1023) // 1024
    rng = np.random.default_rng(n)
    for kind in SCAN_KINDS:
        x = _scan_input(kind, rng, n)
        for with_total in (True, False):
            check_scan(x, with_total, False, f"n={n} {kind} total_out={with_total}")


@pytest.mark.parametrize("n", [1025, 1048577])
def test_scan_in_place(n, hip_lib_built):
    rng = np.random.default_rng(n + 1)
    for kind in SCAN_KINDS:
        check_scan(_scan_input(kind, rng, n), True, True, f"in place n={n} {kind}")


def test_scan_refuses_what_it_cannot_launch(hip_lib_built):
    lib = _binding()._lib
    b = Buf.filled(80)
    assert lib.lidargs_debug_exclusive_scan(8, None, b.ptr, None, b.ptr, _stream()) < 0
    assert lib.lidargs_debug_exclusive_scan(8, b.ptr, b.ptr, None, None, _stream()) < 0
    assert lib.lidargs_debug_exclusive_scan(1 << 31, b.ptr, b.ptr, None, b.ptr, _stream()) < 0
    _sync()
    b.read()


# ---- emit ---------------------------------------------------------------------------------------------------------------------------
def check_emit(spans, ids, th, tiles_x, tiles_y, compact, key_bytes, cap=ref.NO_CAP, with_ranges=True, what=""):
    """One record list through lidargs_debug_emit_instances in both forms of the block sums; returns the instance total."""
    lib = _binding()._lib
    P = spans.shape[0]
    tiles = tiles_x * tiles_y
    want_tile, want_val, total = ref.emit(ids, spans, th, tiles_x, cap)
    m = min(total, cap)
    assert want_tile.size == m and total < (1 << 32) and (m == 0 or int(want_tile.max()) < min(tiles, 1 << (8 * key_bytes)))
    records = ref.pack_compact(spans) if compact else spans.reshape(-1)
    blocks = ref.block_counts(spans, th).astype(np.uint32)
    for scan_block_sums in (0, 1):
        w = f"{what} scan_block_sums={scan_block_sums}"
        b_ids, b_rec = Buf(ids), Buf(records)
        b_off, b_total = Buf.filled(blocks.size), Buf.filled(1)
        b_tile, b_val = Buf.filled(m if key_bytes == 4 else (m + 1) // 2), Buf.filled(m)
        b_rng = Buf.filled(2 * tiles) if with_ranges else None
        rc = lib.lidargs_debug_emit_instances(P, compact, th, tiles_x, tiles_y, b_ids.ptr, b_rec.ptr, b_off.ptr, b_total.ptr, scan_block_sums, key_bytes,
                                              b_tile.ptr, b_val.ptr, cap, b_rng.ptr if b_rng else None, _stream())
        assert rc == 0, (w, _binding()._err())
        _sync()
        _same(f"{w} ids", b_ids.read(), ids)
        _same(f"{w} records", b_rec.read(), records)
        # the full need, whatever the cut: scanned block sums and the total, or the sums as they are (the total is then the caller's)
        _same(f"{w} block_off", b_off.read(), ref.scan(blocks)[0] if scan_block_sums else blocks)
        _same(f"{w} total_out", b_total.read(), np.array([total if scan_block_sums else 0xFFFFFFFF], np.uint32))
        _same(f"{w} values", b_val.read(), want_val)                   # (the guards right behind m: nothing behind the cut is written)
        _same(f"{w} tiles", b_tile.read(), _key_words(want_tile, key_bytes))       # (an odd m of 16-bit keys: the half word behind stays 0xFFFF)
        if b_rng:
            _same(f"{w} ranges", b_rng.read(), np.zeros(2 * tiles, np.uint32))
    return total


@pytest.mark.parametrize("compact,key_bytes", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("P", [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17])
def test_emit_random_records(P, compact, key_bytes, hip_lib_built):
    rng = np.random.default_rng(P * 8 + compact * 4 + key_bytes)
    spans = ref.random_spans(rng, P, GRID_X, GRID_H, compact=bool(compact))
    if P == 1:
        spans = ref.make_spans(160, 171, 3, 41)                         # (not an empty one: 11 columns across the seam x 11 tile rows)
    check_emit(spans, _ids(rng, P), 4, GRID_X, GRID_H // 4, compact, key_bytes, what=f"P={P}")


def _span_of_count(c):
    """A record of exactly c instances on the 166 x 16 grid: the fewest tile rows r with c = nx * r, nx <= 166."""
    if c == 0:
        return (0, 0, 0, 0)
    r = next(r for r in range(1, 17) if c % r == 0 and c // r <= GRID_X)
    return (5, 5 + c // r, 2, 4 * (r - 1) + 3)


def _window_counts(kind, P):
    i = np.arange(P)
    lane = i % 64
    if kind == "every_count_1":
        return np.ones(P, np.int64)
    if kind == "only_the_last_lane":
        return np.where((lane == 63) | (i == P - 1), 3, 0)
    if kind == "lane_0_empty_lane_1_of_200":                # lane 1 owns slots 0..199: the whole of three windows and a part of the fourth, by carry
        return np.where(lane == 1, 200, np.where((lane > 1) & (lane % 5 == 0), 1, 0))
    if kind == "every_count_64":
        return np.full(P, 64, np.int64)
    if kind == "every_count_65":
        return np.full(P, 65, np.int64)
    if kind == "counts_64_and_65":
        return np.where(lane % 2 == 0, 64, 65)
    if kind == "empty_wave_between_two_full_ones":
        return np.where((i // 64) % 3 == 1, 0, 2)
    if kind == "empty_block_in_front":                      # block_off[1] - block_off[0] = 0 (every record of the first block empty)
        return np.where(i < 1024, 0, 7)
    raise ValueError(kind)


WINDOW_KINDS = ["every_count_1", "only_the_last_lane", "lane_0_empty_lane_1_of_200", "every_count_64", "every_count_65", "counts_64_and_65",
                "empty_wave_between_two_full_ones", "empty_block_in_front"]


@pytest.mark.parametrize("compact,key_bytes", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("P", [64, 1025, 2 * 1024 + 70])
@pytest.mark.parametrize("kind", WINDOW_KINDS)
def test_emit_window_structure(kind, P, compact, key_bytes, hip_lib_built):
    """(P = 64: one wave, so the patterns that need a second wave or block reduce to a full wave, and to no instances at all -- a total
    of 0; 2118: an empty block in front of a full block and a partial one.)"""
    counts = _window_counts(kind, P)
    spans = ref.make_spans(*np.array([_span_of_count(int(c)) for c in counts]).T)
    assert np.array_equal(ref.counts(spans, 4), counts)
    rng = np.random.default_rng(P)
    check_emit(spans, _ids(rng, P), 4, GRID_X, GRID_H // 4, compact, key_bytes, what=f"{kind} P={P}")


@pytest.mark.parametrize("compact,key_bytes", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("th", [4, 8, 16, 32])
def test_emit_tile_rows(th, compact, key_bytes, hip_lib_built):
    """lo and hi on, one below and one above every multiple of the tile height, up to lo = 255, hi = 256 (the compact form's last)."""
    H, tiles_x = 256, 5
    spans = ref.row_edge_spans(th, H, tiles_x)
    lo, hi = ref.fields(spans)[2:]
    assert ((lo == 255) & (hi == 256)).any() and ((lo == 0) & (hi == 256)).any()
    rng = np.random.default_rng(th)
    check_emit(spans, _ids(rng, spans.shape[0]), th, tiles_x, H // th, compact, key_bytes, what=f"tile rows th={th}")


@pytest.mark.parametrize("compact,key_bytes", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("tiles_x", [GRID_X, 256])
def test_emit_columns_and_seam(tiles_x, compact, key_bytes, hip_lib_built):
    """x1 == tiles_x, tiles_x + 1; x0 == tiles_x - 1 as wide as the grid; at 256 columns the compact extremes x0 = 255, nx = 256."""
    spans = ref.column_edge_spans(tiles_x, GRID_H, 4)
    x0, x1 = ref.fields(spans)[:2]
    assert ((x0 == tiles_x - 1) & (x1 - x0 == tiles_x)).any() and (x1 == tiles_x).any() and (x1 == tiles_x + 1).any()
    rng = np.random.default_rng(tiles_x)
    check_emit(spans, _ids(rng, spans.shape[0]), 4, tiles_x, GRID_H // 4, compact, key_bytes, what=f"columns tiles_x={tiles_x}")


@pytest.mark.parametrize("compact,key_bytes", FORMS, ids=FORM_IDS)
def test_emit_division_by_every_width(compact, key_bytes, hip_lib_built):
    """Every nx in 1..256 over 64 tile rows at tile height 4 (the most a compact record spans): quotients 0..63 by the float reciprocal.
    (One call: x0 alternates between 0 and the seam, so that rx takes every value on both sides of it.)"""
    nx = np.arange(1, 257)
    x0 = np.where(nx % 2 == 0, 0, 255 - nx // 3)
    spans = ref.make_spans(x0, x0 + nx, 0, 256)
    rng = np.random.default_rng(5)
    assert check_emit(spans, _ids(rng, 256), 4, 256, 64, compact, key_bytes, what="every width") == 64 * 257 * 128


def test_emit_division_large_quotients_of_narrow_spans(hip_lib_built):
    """nx = 1, 2, 3 over the 16 384 tile rows a full record can span: quotients up to 16 383 by the float reciprocal."""
    spans = ref.make_spans([7, 9, 8], [8, 11, 11], [0, 3, 1], [65535, 65533, 65534])
    assert ref.counts(spans, 4).tolist() == [16384, 2 * 16384, 3 * 16384]
    check_emit(spans, np.array([11, 5, 8], np.uint32), 4, 10, 16384, 0, 4, with_ranges=False, what="narrow spans")


@pytest.mark.parametrize("nx,rows,tiles_x,th,x0", [(257, 16384, 300, 4, 100), (4097, 1025, 4100, 32, 2), (65535, 65, 65535, 16, 0)],
                         ids=["257x16384", "4097x1025", "65535x65"])
def test_emit_division_around_2_to_22(nx, rows, tiles_x, th, x0, hip_lib_built):
    """One record of a little more than 2^22 instances: the float reciprocal up to instance 4 194 303, the integer division behind it."""
    spans = ref.make_spans(x0, x0 + nx, th - 1, min(th * rows - 1, 65535))
    total = int(ref.counts(spans, th)[0])
    assert total == nx * rows and 4194305 <= total <= 4300000
    check_emit(spans, np.array([0x01234567], np.uint32), th, tiles_x, rows, 0, 4, with_ranges=False, what=f"nx={nx} rows={rows}")


def test_emit_division_where_the_float_estimate_is_one_too_large(hip_lib_built):
    """nx = 4071 over 1030 tile rows, 4 193 130 instances, all below 2^22: at the last column of rows 1024..1029 (instance 4 172 774 and
    every 4071st behind it) the device's float estimate of jj / nx comes out one too large and the downward correction step sets it right.
    (Found by evaluating the estimate on the device for every width up to 65 535 at both extreme remainders of every quotient below 2^22:
    it is one too large at 28 places, all beyond instance 4.15 M, and never too small.)"""
    nx, rows, th = 4071, 1030, 32
    spans = ref.make_spans(20, 20 + nx, 5, th * rows - 7)
    assert int(ref.counts(spans, th)[0]) == nx * rows == 4193130 < (1 << 22)
    check_emit(spans, np.array([0x00C0FFEE], np.uint32), th, 4100, rows, 0, 4, with_ranges=False, what=f"nx={nx} rows={rows}")


@pytest.mark.parametrize("compact,key_bytes", FORMS, ids=FORM_IDS)
def test_emit_capacity(compact, key_bytes, hip_lib_built):
    """Enqueue-only frames: nothing at or behind min(total, cap) is written, and the total is still the full need."""
    P = 1025
    rng = np.random.default_rng(77 + compact + key_bytes)
    spans = ref.random_spans(rng, P, GRID_X, GRID_H, compact=bool(compact))
    ids = _ids(rng, P)
    total = int(ref.counts(spans, 4).sum())
    for cap in (0, 1, (total // 2) | 1, total - 1, total, total + 1):    # (an odd cut: with 16-bit keys the other half of the last word stays)
        check_emit(spans, ids, 4, GRID_X, GRID_H // 4, compact, key_bytes, cap=cap, what=f"cap={cap} of {total}")


def test_emit_refuses_what_no_frame_asks_for(hip_lib_built):
    lib = _binding()._lib
    b = Buf.filled(64)

    def call(P=8, compact=0, th=4, tx=16, ty=16, key_bytes=4, cap=ref.NO_CAP):
        return lib.lidargs_debug_emit_instances(P, compact, th, tx, ty, b.ptr, b.ptr, b.ptr, b.ptr, 1, key_bytes, b.ptr, b.ptr, cap, None, _stream())

    assert call(th=2) < 0 and call(th=12) < 0 and call(th=64) < 0
    assert call(key_bytes=1) < 0 and call(key_bytes=8) < 0
    assert call(key_bytes=2, tx=257, ty=256) < 0                        # 65 792 tiles
    assert call(compact=1, tx=257) < 0
    assert call(tx=65536, ty=65536) < 0 and call(tx=0) < 0
    assert call(cap=1 << 32) < 0
    assert call(P=0) == 0                                               # nothing is launched
    _sync()
    b.read()


# ---- tile ranges --------------------------------------------------------------------------------------------------------------------
RANGE_KINDS = ["one_tile", "every_tile", "first_and_last_tile", "random_with_many_empty_tiles", "steps_between_two_threads_and_two_blocks"]


def _sorted_keys(kind, rng, R, tiles):
    i = np.arange(R)
    if kind == "one_tile":
        return np.full(R, tiles - 1 - (tiles - 1) // 3, np.int64)
    if kind == "every_tile":                                # every tile as often as the others (R >= tiles), or the last R tiles once each
        return np.sort(i % tiles) if R >= tiles else i + (tiles - R)
    if kind == "first_and_last_tile":
        return np.where(i < (R + 1) // 2, 0, tiles - 1)
    if kind == "random_with_many_empty_tiles":
        some = rng.choice(tiles, max(1, tiles // 8), replace=False)
        return np.sort(some[rng.integers(0, some.size, R)])
    if kind == "steps_between_two_threads_and_two_blocks":  # thread 0 holds keys 0..7, block 0 keys 0..2047
        return np.minimum((i >= 8) * (tiles // 2) + (i >= 2048) * (tiles - 1 - tiles // 2), tiles - 1)
    raise ValueError(kind)


def check_tile_ranges(keys, R, tiles, key_bytes, prezeroed, r_dev, rng, what):
    """keys: the R sorted ones.  Behind min(R, r_dev), up to R rounded up to 8, lie keys that must not be looked at: other TILES OF THE
    GRID in descending order (a kernel that looked at them would write wrong ranges, and never outside the array)."""
    lib = _binding()._lib
    count = R if r_dev is None else min(R, r_dev)
    room = (R + 7) // 8 * 8
    held = np.concatenate([keys[:count], np.sort(rng.integers(0, tiles, room - count))[::-1]]).astype(np.uint32)
    b_keys = Buf(_key_words(held, key_bytes))
    b_cnt = Buf(np.array([r_dev], np.uint32)) if r_dev is not None else None
    b_rng = Buf(np.zeros(2 * tiles, np.uint32)) if prezeroed else Buf.filled(2 * tiles)
    b_zero, b_kept = Buf.filled(300), Buf.filled(300)
    give_zero = (R + tiles + prezeroed) % 3 != 0                        # zero = NULL with n_zero = 300 in a third of the calls: nothing is touched
    rc = lib.lidargs_debug_tile_ranges(R, key_bytes, b_keys.ptr, b_cnt.ptr if b_cnt else None, b_rng.ptr, tiles, b_zero.ptr if give_zero else None, 300,
                                       prezeroed, _stream())
    assert rc == 0, (what, _binding()._err())
    _sync()
    _same(f"{what} keys", b_keys.read(), _key_words(held, key_bytes))
    if b_cnt:
        _same(f"{what} count", b_cnt.read(), np.array([r_dev], np.uint32))
    _same(f"{what} ranges", b_rng.read().reshape(tiles, 2), ref.ranges(held, count, tiles))
    _same(f"{what} counters", b_zero.read(), np.full(300, 0 if give_zero else 0xFFFFFFFF, np.uint32))
    b_kept.read()


@pytest.mark.parametrize("key_bytes", [4, 2], ids=["keys_32", "keys_16"])
@pytest.mark.parametrize("R", [1, 7, 8, 9, 2047, 2048, 2049, 100003])
def test_tile_ranges(R, key_bytes, hip_lib_built):
    rng = np.random.default_rng(R + key_bytes)
    for tiles in (1, GRID_X * 16, 65536):
        for kind in RANGE_KINDS:
            keys = _sorted_keys(kind, rng, R, tiles)
            assert keys.size == R and (np.diff(keys) >= 0).all() and 0 <= keys[0] and keys[-1] < tiles
            for prezeroed in (1, 0):
                check_tile_ranges(keys, R, tiles, key_bytes, prezeroed, None, rng, f"R={R} tiles={tiles} {kind} prezeroed={prezeroed}")
            for n, r_dev in enumerate((0, 1, R - 1, R, R + 5)):
                check_tile_ranges(keys, R, tiles, key_bytes, (n + R) & 1, r_dev, rng, f"R={R} tiles={tiles} {kind} R_dev={r_dev}")


@pytest.mark.parametrize("key_bytes", [4, 2], ids=["keys_32", "keys_16"])
def test_tile_ranges_without_instances(key_bytes, hip_lib_built):
    rng = np.random.default_rng(0)
    for tiles in (1, GRID_X * 16, 65536):
        for prezeroed in (1, 0):
            check_tile_ranges(np.zeros(0, np.int64), 0, tiles, key_bytes, prezeroed, None, rng, f"R=0 tiles={tiles} prezeroed={prezeroed}")


def test_tile_ranges_refuses_what_it_cannot_read(hip_lib_built):
    lib = _binding()._lib
    b = Buf(np.zeros(64, np.uint32))
    off = C.c_void_p(b.ptr.value + 4)
    assert lib.lidargs_debug_tile_ranges(8, 4, off, None, b.ptr, 4, None, 0, 0, _stream()) < 0              # not 16-byte aligned
    assert lib.lidargs_debug_tile_ranges(8, 3, b.ptr, None, b.ptr, 4, None, 0, 0, _stream()) < 0
    assert lib.lidargs_debug_tile_ranges(8, 2, b.ptr, None, b.ptr, 65537, None, 0, 0, _stream()) < 0
    assert lib.lidargs_debug_tile_ranges(8, 4, None, None, b.ptr, 4, None, 0, 0, _stream()) < 0
    assert lib.lidargs_debug_tile_ranges(8, 4, b.ptr, None, None, 4, None, 0, 0, _stream()) < 0
    _sync()
    b.read()


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bytes", [4, 2], ids=["keys_32", "keys_16"])
def test_emit_sort_ranges_chain(key_bytes, hip_lib_built):
    """What a frame queues behind its range sort, on 20 000 records: per tile the Gaussians in range order."""
    lib = _binding()._lib
    P, th, tiles_x, tiles_y = 20000, 4, GRID_X, GRID_H // 4
    tiles = tiles_x * tiles_y
    bits = (tiles - 1).bit_length()
    rng = np.random.default_rng(key_bytes)
    spans, ids = ref.random_spans(rng, P, tiles_x, GRID_H), _ids(rng, P)
    want_val, want_rng = ref.tile_lists(ids, spans, th, tiles_x, tiles)
    R = want_val.size
    # the sorted lists are wanted on the a side: a sort that ends on the other side gets its input there (as bin_frame places it)
    flip = int(lib.lidargs_debug_sort_result_side(R, bits))
    p = Pairs(np.zeros(R, np.uint32), np.zeros(R, np.uint32), key_bytes)     # (the emit writes every one of the R pairs of the input side)
    b_ids, b_rec, b_off, b_total, b_rng = Buf(ids), Buf(spans.reshape(-1)), Buf.filled((P + 1023) // 1024), Buf.filled(1), Buf.filled(2 * tiles)
    rc = lib.lidargs_debug_emit_instances(P, 0, th, tiles_x, tiles_y, b_ids.ptr, b_rec.ptr, b_off.ptr, b_total.ptr, 0, key_bytes, p.key[flip].ptr,
                                          p.val[flip].ptr, ref.NO_CAP, b_rng.ptr, _stream())
    assert rc == 0, _binding()._err()
    side = p.sort(in_side=flip, end=bits)
    assert side == 0
    rc = lib.lidargs_debug_tile_ranges(R, key_bytes, p.key[0].ptr, None, b_rng.ptr, tiles, None, 0, 1, _stream())
    assert rc == 0, _binding()._err()
    _sync()
    for b in (b_ids, b_rec, b_off, b_total):
        b.read()
    got_key, got_val = p.result(0)
    _same("values in tile order", got_val, want_val)
    _same("ranges", b_rng.read().reshape(tiles, 2), want_rng)
    _same("sorted tiles", got_key, np.repeat(np.arange(tiles, dtype=np.uint32), (want_rng[:, 1] - want_rng[:, 0]).astype(np.int64)))
