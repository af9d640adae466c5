"""The ORDER the hand-written sorts of csrc/binning.hip produce, bit for bit against `numpy.argsort(..., kind="stable")`.

Five subsystems stand on these sorts (the range sort of the Gaussians, the per-tile instance sort, anchor growing, distCUDA2,
voxelize_sample) and every other test sees them only through what is built on top: rendered images under a parity budget, or a few fixed
sizes with 32-bit keys.  Here the library's own launchers are reached through the test hooks of the C ABI (`lidargs_debug_sort_pairs`,
`lidargs_debug_range_sort_buckets`, ...) at every size, digit width and form at which the pass structure takes another branch:

    single launch (<= 4096 pairs) / general passes          2048- / 4096-key blocks            k_radix_digit_prefix<2> / <4> / <8>
    the two-level cross-block prefix (> 2048 blocks)        pass widths 1..11                  16-bit keys
    a device-side pair count                                begin_bit > 0 with a key bias      both tails
    the bucketed range sort: LDS path / bucket_sort_slow at 7168 | 7169 pairs, 1024 and 2048 intervals

A sort has one right answer: every comparison is `np.array_equal` on integers.  The reference of every case is the same -- the digit
field f = (km(key) >> begin_bit) & ((1 << (end_bit - begin_bit)) - 1), km the identity or (key == 0xFFFFFFFF ? cull : key - kmin), and
perm = the stable argsort of f: raw keys and values on the returned side are key[perm] and val[perm].  Every array the hooks see lies
between 64 guard words that must come back untouched; the b sides and the tail's destination start out as 0xFF bytes."""
import ctypes as C

import numpy as np
import pytest

from util import run_child

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5EA7C0DE
CULLED = 0xFFFFFFFF
DEFAULT_DIGIT = 8           # SORT_RADIX_BITS
SPAN_SLOTS = 64             # LG_INST_SLOTS


def _binding():
    from diff_lidargs_rasterization import _C as binding
    return binding


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """A device array of u32 words between two guards."""

    def __init__(self, payload):
        import torch
        payload = np.ascontiguousarray(payload)
        assert payload.dtype == np.uint32 and payload.ndim == 1
        guard = np.full(GUARD, SENTINEL, np.uint32)
        self.words = payload.size
        self.t = torch.from_numpy(np.concatenate([guard, payload, guard]).view(np.int32)).cuda()

    @classmethod
    def filled(cls, words, byte=0xFF):
        return cls(np.full(words, byte * 0x01010101, np.uint32))

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 4 * GUARD)

    def read(self):
        """The payload, after checking both guards."""
        full = self.t.cpu().numpy().view(np.uint32)
        assert np.array_equal(full[:GUARD], np.full(GUARD, SENTINEL, np.uint32)), "guard in front of the array was written"
        assert np.array_equal(full[GUARD + self.words:], np.full(GUARD, SENTINEL, np.uint32)), "guard behind the array was written"
        return full[GUARD:GUARD + self.words]


def _key_words(keys, key_bytes):
    """Keys as u32 words (16-bit keys packed two to a word, the odd one padded with 0xFFFF, which must stay)."""
    if key_bytes == 4:
        return keys.astype(np.uint32)
    k = keys.astype(np.uint16)
    if k.size & 1:
        k = np.concatenate([k, np.array([0xFFFF], np.uint16)])
    return k.view(np.uint32)


def _stable_argsort(f):
    """np.argsort(f, kind="stable").  Above 2 M keys of more than 16 bits the same permutation is composed of two stable argsorts on the
    low and the high 16 bits (numpy sorts 16-bit integers by counting, 32-bit ones by merging: 0.7 s against 1.6 s at 8 M keys)."""
    top = int(f.max()) if f.size else 0
    if top < (1 << 16):
        return np.argsort(f.astype(np.uint16), kind="stable")
    if f.size <= (1 << 21):
        return np.argsort(f, kind="stable")
    assert top < (1 << 32)
    p1 = np.argsort((f & 0xFFFF).astype(np.uint16), kind="stable")
    p2 = np.argsort((f[p1] >> 16).astype(np.uint16), kind="stable")
    return p1[p2]


def _field(keys, begin, end, bias):
    k = keys.astype(np.uint64)
    if bias is not None:
        kmin, cull = bias
        k = np.where(k == CULLED, np.uint64(cull), (k - np.uint64(kmin)) & np.uint64(0xFFFFFFFF))
    return (k >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)


def _same(what, got, want):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0] if got.shape == want.shape else np.array([0])
        raise AssertionError(f"{what}: {bad.size} of {want.shape[0]} differ; first at {bad[0]}: got {got[bad[0]]!r}, expected {want[bad[0]]!r}")


class Pairs:
    """The ping-pong arrays of one sort on the device, and the calls on them."""

    def __init__(self, keys, vals, key_bytes=4, scratch_bits=DEFAULT_DIGIT):
        self.lib = _binding()._lib
        self.n, self.key_bytes = int(keys.size), key_bytes
        kw = _key_words(keys, key_bytes)
        self.key = [Buf(kw), Buf.filled(kw.size)]
        # without values the sort is told that they are the positions: val_a is then never read, and starts out as 0xFF bytes as well
        self.val = [Buf(vals.astype(np.uint32)) if vals is not None else Buf.filled(self.n), Buf.filled(self.n)]
        self.scratch = Buf.filled(int(self.lib.lidargs_debug_sort_scratch_words(self.n, scratch_bits)), 0xEE)   # (what a frame before left there)
        self.bufs = self.key + self.val + [self.scratch]

    def sort(self, in_side=0, begin=0, end=None, max_bits=0, scratch_bits=0, n_dev=None, positions=False, bias=None, tail_mode=0,
             tail_src=None, tail_dst=None):
        """One call of lidargs_debug_sort_pairs with the `in_side` arrays as its a side; the side (of THESE arrays) the result lies on."""
        import torch
        end = 8 * self.key_bytes if end is None else end
        nd = None
        if n_dev is not None:
            nd = Buf(np.array([n_dev], np.uint32)); self.bufs.append(nd)
        for b in (tail_src, tail_dst):
            if b is not None and b not in self.bufs:
                self.bufs.append(b)
        a, b = in_side, in_side ^ 1
        kmin, cull = bias if bias is not None else (0, 0)
        rc = self.lib.lidargs_debug_sort_pairs(self.n, self.key_bytes, self.key[a].ptr, self.key[b].ptr, self.val[a].ptr, self.val[b].ptr, begin, end,
                                               max_bits, scratch_bits, self.scratch.ptr, nd.ptr if nd else None, int(positions), int(bias is not None),
                                               int(kmin), int(cull), tail_mode, tail_src.ptr if tail_src else None,
                                               tail_dst.ptr if tail_dst else None, _stream())
        assert rc in (0, 1), (rc, _binding()._err())
        torch.cuda.synchronize()
        return rc ^ in_side

    def guards(self):
        for b in self.bufs:
            b.read()

    def result(self, side, count=None):
        """(keys, values) of the first `count` pairs on `side`; every guard is checked."""
        self.guards()
        count = self.n if count is None else count
        kw = self.key[side].read()
        if self.key_bytes == 2 and (self.n & 1):
            assert kw.view(np.uint16)[self.n] == 0xFFFF, "the half word behind the last 16-bit key was written"
        keys = kw if self.key_bytes == 4 else kw.view(np.uint16)
        return keys[:count].astype(np.uint32), self.val[side].read()[:count]


def _distinct_values(rng, n):
    return (rng.permutation(n).astype(np.uint64) * 7 + 3).astype(np.uint32)         # distinct, not the positions (n < 2^29)


def check_sort(keys, vals=None, key_bytes=4, begin=0, end=None, max_bits=0, scratch_bits=0, n_dev=None, bias=None, want_side=None, what=""):
    """One sort without a tail against the stable argsort.  vals = None: the values are the positions.  Returns the side."""
    end = 8 * key_bytes if end is None else end
    digit = max_bits or DEFAULT_DIGIT
    p = Pairs(keys, vals, key_bytes, scratch_bits or digit)
    side = p.sort(begin=begin, end=end, max_bits=max_bits, scratch_bits=scratch_bits, n_dev=n_dev, positions=vals is None, bias=bias)
    m = p.n if n_dev is None else min(p.n, n_dev)
    got_k, got_v = p.result(side, m)
    if m:
        perm = _stable_argsort(_field(keys[:m], begin, end, bias)) if end > begin else np.arange(m)
        src_v = vals[:m].astype(np.uint32) if vals is not None else np.arange(m, dtype=np.uint32)
        _same(f"{what} values", got_v, src_v[perm])
        _same(f"{what} keys", got_k, keys[:m].astype(np.uint32)[perm])
        if vals is None and begin == 0:
            _same(f"{what} positions", got_v, perm.astype(np.uint32))
    if want_side == "default":          # (h) default digits, no tail: where the frame's tile sort expects the result
        assert side == p.lib.lidargs_debug_sort_result_side(p.n, end), (what, side)
    elif want_side is not None:
        assert side == want_side, (what, side)
    return side


def _random_keys(rng, n, bits=32):
    return rng.integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)


def test_the_reference_composed_of_two_argsorts_is_the_stable_argsort():
    rng = np.random.default_rng(1)
    f = _random_keys(rng, (1 << 21) + 5, 18).astype(np.uint64) << np.uint64(9)      # ties in both halves
    assert np.array_equal(_stable_argsort(f), np.argsort(f, kind="stable"))


# ---- a. sizes at every structural edge (32-bit random keys, end_bit = 32, default digits, distinct random values) --------------------
# scratch_bits = 11, as the range sort carves it: room for the 2048-key blocks up to 4 Mi pairs
EDGES = ([("single_launch", n) for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096)]
         + [("blocks_of_2048", n) for n in (4097, 6143, 8191, 8193)]
         + [("digit_prefix_2_to_4", 512 * 2048 - 1), ("digit_prefix_2_to_4", 512 * 2048 + 1),
            ("digit_prefix_4_to_8", 1024 * 2048 - 1), ("digit_prefix_4_to_8", 1024 * 2048 + 1),
            ("last_with_blocks_of_2048", 4194304), ("first_with_blocks_of_4096", 4194305)])


@pytest.mark.parametrize("branch,n", EDGES, ids=[f"{b}-{n}" for b, n in EDGES])
def test_sizes_at_every_structural_edge(branch, n, hip_lib_built):
    rng = np.random.default_rng(n)
    check_sort(_random_keys(rng, n), _distinct_values(rng, n), scratch_bits=11, want_side="default", what=f"{branch} n={n}")


@pytest.mark.parametrize("max_bits,end", [(0, 32), (11, 31)], ids=["digits_8", "digits_11_end_bit_31"])
def test_two_level_cross_block_prefix(max_bits, end, hip_lib_built):
    """2049 blocks of 4096 keys: three chunks of the cross-block prefix, k_radix_chunk_prefix over them."""
    n = 8388609
    rng = np.random.default_rng(n + max_bits)
    check_sort(_random_keys(rng, n), _distinct_values(rng, n), end=end, max_bits=max_bits, scratch_bits=11,
               want_side="default" if max_bits == 0 else 1, what=f"two-level n={n}")


@pytest.mark.parametrize("n", [4097, 8193, 1024 * 4096 + 1])
def test_blocks_of_4096_when_the_scratch_has_no_room_for_half_blocks(n, hip_lib_built):
    """scratch_bits = the digit width, as the tile sort carves it: 4096-key blocks at every size."""
    rng = np.random.default_rng(n + 1)
    check_sort(_random_keys(rng, n), _distinct_values(rng, n), scratch_bits=DEFAULT_DIGIT, want_side="default", what=f"n={n}")


# ---- b. every pass width ------------------------------------------------------------------------------------------------------------
def _keys_for_field(rng, n, begin, end):
    """Random bits inside [begin, end); every second key has random bits outside the field as well, which the sort must ignore."""
    mask = ((1 << (end - begin)) - 1) << begin
    k = _random_keys(rng, n) & np.uint32(mask)
    k[1::2] |= _random_keys(rng, (n // 2)) & np.uint32(~mask & 0xFFFFFFFF)
    return k


@pytest.mark.parametrize("max_bits", [0, 9, 11], ids=["digits_8", "digits_9", "digits_11"])
@pytest.mark.parametrize("n", [3001, 6143], ids=["single_launch_3001", "general_6143"])
def test_every_pass_width(n, max_bits, hip_lib_built):
    """end_bit 1..32, split evenly over passes of at most 8 / 9 / 11 bits: widths 1..11."""
    rng = np.random.default_rng(n * 13 + max_bits)
    vals = _distinct_values(rng, n)
    for end in range(1, 33):
        check_sort(_keys_for_field(rng, n, 0, end), vals, end=end, max_bits=max_bits, scratch_bits=11, what=f"n={n} bits [0, {end}) digits {max_bits}")


@pytest.mark.parametrize("max_bits", [0, 9, 11], ids=["digits_8", "digits_9", "digits_11"])
@pytest.mark.parametrize("begin", [3, 8])
@pytest.mark.parametrize("n", [3001, 6143], ids=["single_launch_3001", "general_6143"])
def test_begin_bit(n, begin, max_bits, hip_lib_built):
    rng = np.random.default_rng(n * 17 + begin * 3 + max_bits)
    vals = _distinct_values(rng, n)
    for end in (begin + 1, 17, 26, 32):
        check_sort(_keys_for_field(rng, n, begin, end), vals, begin=begin, end=end, max_bits=max_bits, scratch_bits=11,
                   what=f"n={n} bits [{begin}, {end}) digits {max_bits}")


# ---- c. adversarial key sets --------------------------------------------------------------------------------------------------------
def _adversarial_keys(kind, rng, n):
    if kind == "all_equal":
        return np.full(n, 0x9E3779B9, np.uint32)
    if kind == "two_values":
        return np.where(rng.integers(0, 2, n) == 1, 0xC0000001, 0x3FFFFFFE).astype(np.uint32)
    if kind == "sorted":
        return np.sort(_random_keys(rng, n))
    if kind == "reversed":
        return np.sort(_random_keys(rng, n))[::-1].copy()
    if kind == "top_bit_only":
        return (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(31)).astype(np.uint32)
    if kind == "one_digit_in_the_first_pass":
        return (_random_keys(rng, n) & np.uint32(0xFFFFFF00)) | np.uint32(0x5A)
    if kind == "runs_of_70_identical_keys":        # (1000 runs at n = 70 001; only the stable order is right)
        return _random_keys(rng, n // 70 + 1, 10)[np.arange(n) // 70] * np.uint32(0x00400801)
    raise ValueError(kind)


@pytest.mark.parametrize("n", [6143, 70001])
@pytest.mark.parametrize("kind", ["all_equal", "two_values", "sorted", "reversed", "top_bit_only", "one_digit_in_the_first_pass",
                                  "runs_of_70_identical_keys"])
def test_adversarial_key_sets(kind, n, hip_lib_built):
    rng = np.random.default_rng(n + len(kind))
    check_sort(_adversarial_keys(kind, rng, n), _distinct_values(rng, n), scratch_bits=11, want_side="default", what=f"{kind} n={n}")


# ---- d. 16-bit keys -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 4096, 4097, 8193, 1048577])
def test_16_bit_keys(n, hip_lib_built):
    rng = np.random.default_rng(n + 16)
    vals = _distinct_values(rng, n)
    for end in range(1, 17):
        check_sort(_keys_for_field(rng, n, 0, end) & np.uint32(0xFFFF) if end < 16 else _random_keys(rng, n, 16), vals, key_bytes=2, end=end,
                   want_side="default", what=f"16-bit n={n} bits [0, {end})")


@pytest.mark.parametrize("n", [65, 4097, 8193])
@pytest.mark.parametrize("kind", ["all_equal", "two_values"])
def test_16_bit_keys_with_few_values(kind, n, hip_lib_built):
    rng = np.random.default_rng(n + 160)
    keys = np.full(n, 65535, np.uint32) if kind == "all_equal" else np.where(rng.integers(0, 2, n) == 1, 65535, 0x0180).astype(np.uint32)
    check_sort(keys, _distinct_values(rng, n), key_bytes=2, want_side="default", what=f"16-bit {kind} n={n}")


# ---- e. the pair count on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bytes", [4, 2], ids=["keys_32", "keys_16"])
@pytest.mark.parametrize("n", [4096, 4097, 8193, 12293], ids=["single_launch_4096", "capacity_4097", "capacity_8193", "capacity_12293"])
def test_device_side_count(n, key_bytes, hip_lib_built):
    """Enqueue-only frames: the launches cover the capacity, *n_dev pairs are sorted; what lies behind them is unspecified."""
    rng = np.random.default_rng(n + key_bytes)
    keys, vals = _random_keys(rng, n, 8 * key_bytes), _distinct_values(rng, n)
    for count in ((0, 1, 4095) if n == 4096 else (0, 1, 64, 2047, 2048, 2049, n - 1, n)):
        check_sort(keys, vals, key_bytes=key_bytes, n_dev=count, scratch_bits=11 if key_bytes == 4 else 0, what=f"capacity {n}, count {count}")


# ---- f. the LSD range sort as a frame cuts it in two calls --------------------------------------------------------------------------
def _range_keys(kind, rng, P, culled=0.3):
    if kind == "ranges_2_to_80":
        r = rng.uniform(2.0, 80.0, P)
    elif kind == "ranges_0.4_to_4.8":
        r = rng.uniform(0.4, 4.8, P)
    elif kind == "one_range":
        r = np.full(P, 17.25)
    else:
        raise ValueError(kind)
    keys = r.astype(np.float32).view(np.uint32).copy()
    keys[rng.random(P) < culled] = CULLED
    return keys


def _tail_source(rng, P, mode, empty=None):
    """The per-value records of a tail and, per value, what the tail leaves at the value's final place.  `empty`: the ids whose record
    is "no instances" (mode 1: 0xFFFFFFFF, mode 2: a zero column span)."""
    if mode == 1:
        src = _random_keys(rng, P)
        if empty is not None:
            src[empty] = CULLED
        return src, src
    src = _random_keys(rng, 4 * P).reshape(P, 4)
    if empty is not None:
        src[empty, :2] = 0
    return src.reshape(-1), np.stack([src[:, 1], src[:, 0]], 1)       # (y, x) of the u32x4 record


def _range_sort_plan(keys):
    """(kmin, cull, end_bit, max_bits) of the second call, as the frame's binning works them out from the smallest and largest key."""
    lib = _binding()._lib
    valid = keys[keys != CULLED]
    lo, hi = (int(valid.min()), int(valid.max())) if valid.size else (CULLED, 0)
    plan = (C.c_uint * 4)()
    assert lib.lidargs_debug_range_sort_rest(lo, hi, plan) == 0
    kmin, cull, end, max_bits = (int(x) for x in plan)
    if valid.size:
        assert kmin == lo & ~255 and cull == ((hi - kmin) | 255) + 1
    assert end >= 9 and cull < (1 << end) and max_bits in (8, 9)
    return kmin, cull, end, max_bits


@pytest.mark.parametrize("mode", [1, 2], ids=["tail_u32", "tail_u32x4"])
@pytest.mark.parametrize("P", [5000, 100003])
@pytest.mark.parametrize("kind", ["ranges_2_to_80", "ranges_0.4_to_4.8", "one_range"])
def test_range_sort_cut_in_two_calls(kind, P, mode, hip_lib_built):
    rng = np.random.default_rng(P + mode)
    keys = _range_keys(kind, rng, P)
    kmin, cull, end, max_bits = _range_sort_plan(keys)
    p = Pairs(keys, None, 4, 11)
    first = p.sort(begin=0, end=8, max_bits=8, scratch_bits=11, positions=True)
    src, rec = _tail_source(rng, P, mode)
    tail_src, tail_dst = Buf(src), Buf.filled(P * mode)
    side = p.sort(in_side=first, begin=8, end=end, max_bits=max_bits, scratch_bits=11, bias=(kmin, cull), tail_mode=mode, tail_src=tail_src, tail_dst=tail_dst)
    _, ids = p.result(side)
    perm = _stable_argsort(keys.astype(np.uint64))                     # (the culled keys are the largest: last, in index order)
    _same("ids in range order", ids, perm.astype(np.uint32))
    _same("tail records", tail_dst.read().reshape(P, mode), rec[perm].reshape(P, mode))


# ---- g. the bucketed range sort -----------------------------------------------------------------------------------------------------
BUCKET_CAP = 7168           # pairs of a bucket on the LDS path (BSORT_CAP); one more goes through bucket_sort_slow


def _crowded_bucket(rng, P, crowd):
    """`crowd` ranges inside ONE of the sort's equal-width intervals of the span [2, 80] (0.076 m wide at 1024 intervals, 0.038 at 2048:
    40.00 .. 40.02 lies well inside interval 498 / 997), the two ends of the span once each, the rest at least 2 m away from the crowd."""
    rest = P - crowd - 2
    r = np.concatenate([[2.0, 80.0], 40.0 + 0.02 * rng.random(crowd), np.where(rng.random(rest) < 0.5, rng.uniform(2.0, 38.0, rest), rng.uniform(42.0, 80.0, rest))])
    r = r.astype(np.float32)
    for bins in (1024, 2048):           # the interval of every range, in the kernel's fp32 arithmetic: the crowd is alone in its interval
        d = np.minimum(bins - 2, ((r - np.float32(2.0)) * (np.float32(bins - 1) / np.float32(78.0))).astype(np.int64))
        assert np.unique(d[2:2 + crowd]).size == 1 and int((d == d[2]).sum()) == crowd
    return rng.permutation(r).view(np.uint32).copy()


def _bucket_keys(kind, rng, P):
    if kind == "random_ranges":
        return _range_keys("ranges_2_to_80", rng, P)
    if kind == "40_distinct_ranges":
        keys = rng.uniform(2.0, 80.0, 40).astype(np.float32)[rng.integers(0, 40, P)].view(np.uint32).copy()
        keys[rng.random(P) < 0.3] = CULLED
        return keys
    if kind == "two_ranges":
        return np.where(rng.integers(0, 2, P) == 1, np.float32(61.5), np.float32(3.25)).astype(np.float32).view(np.uint32).copy()
    if kind == "one_range":
        return _range_keys("one_range", rng, P)
    if kind == "80_percent_culled":
        return _range_keys("ranges_2_to_80", rng, P, culled=0.8)
    if kind == "all_culled":
        return np.full(P, CULLED, np.uint32)
    if kind == "bucket_of_7168":
        return _crowded_bucket(rng, P, BUCKET_CAP)
    if kind == "bucket_of_7169":
        return _crowded_bucket(rng, P, BUCKET_CAP + 1)
    if kind == "bucket_of_20000":
        return _crowded_bucket(rng, P, 20000)
    if kind == "small_bucket_spanning_26_key_bits":    # 1 mm .. 7 cm in the first interval, fewer than 7168 of them: the LDS path's four passes; beyond
        few = rng.random(P) < 0.15                     # the 19 key bits the form that sorts (key, position) words can hold
        r = np.where(few, np.exp(rng.uniform(np.log(1e-3), np.log(0.07), P)), rng.uniform(0.1, 80.0, P))
        return r.astype(np.float32).view(np.uint32).copy()
    raise ValueError(kind)


BUCKET_CASES = [("random_ranges", 30011), ("40_distinct_ranges", 30011), ("two_ranges", 30011), ("one_range", 30011), ("80_percent_culled", 30011),
                ("all_culled", 30011), ("bucket_of_7168", 30011), ("bucket_of_7169", 30011), ("bucket_of_20000", 30011),
                ("small_bucket_spanning_26_key_bits", 30011), ("random_ranges", 4097)]


def _key_span(keys, spread):
    """u32[64][2] = (~smallest, largest) visible key per slot, as the preprocess' blocks leave them: every block's keys folded into
    one of the slots (spread), or the frame's span in slot 0 alone; untouched slots hold (0, 0)."""
    span = np.zeros((SPAN_SLOTS, 2), np.uint32)
    idx = np.nonzero(keys != CULLED)[0]
    for slot in (range(SPAN_SLOTS) if spread else [0]):
        k = keys[idx[idx // 256 % SPAN_SLOTS == slot]] if spread else keys[idx]
        if k.size:
            span[slot] = (~k.min(), k.max())
    return span.reshape(-1)


def check_bucketed_range_sort(kind, P, mode, spread):
    import torch
    lib = _binding()._lib
    rng = np.random.default_rng(P + len(kind))
    keys = _bucket_keys(kind, rng, P)
    src, rec = _tail_source(rng, P, mode, empty=keys == CULLED)
    key = [Buf(keys), Buf.filled(P)]
    ids = [Buf.filled(P), Buf.filled(P)]
    scratch = Buf.filled(int(lib.lidargs_debug_sort_scratch_words(P, 11)), 0xEE)
    span, tail_src, tail_dst = Buf(_key_span(keys, spread)), Buf(src), Buf.filled(2 * P)      # (2 P words in either mode: the 4-byte records ride in the second half)
    rc = lib.lidargs_debug_range_sort_buckets(P, key[0].ptr, key[1].ptr, ids[0].ptr, ids[1].ptr, scratch.ptr, span.ptr, mode, tail_src.ptr, tail_dst.ptr, _stream())
    assert rc == 0, _binding()._err()
    torch.cuda.synchronize()
    for b in key + ids + [scratch, span, tail_src]:
        b.read()
    perm = _stable_argsort(keys.astype(np.uint64))
    _same(f"{kind} ids in range order", ids[0].read(), perm.astype(np.uint32))
    _same(f"{kind} tail records", tail_dst.read()[:P * mode].reshape(P, mode), rec[perm].reshape(P, mode))


@pytest.mark.parametrize("spread", [True, False], ids=["span_over_the_slots", "span_in_slot_0"])
@pytest.mark.parametrize("mode", [1, 2], ids=["tail_u32", "tail_u32x4"])
@pytest.mark.parametrize("kind,P", BUCKET_CASES, ids=[f"{k}-{P}" for k, P in BUCKET_CASES])
def test_bucketed_range_sort(kind, P, mode, spread, hip_lib_built):
    check_bucketed_range_sort(kind, P, mode, spread)


def test_bucketed_range_sort_is_refused_where_no_frame_takes_it(hip_lib_built):
    lib = _binding()._lib
    b = Buf.filled(4096 * 2)
    assert lib.lidargs_debug_range_sort_buckets(4096, b.ptr, b.ptr, b.ptr, b.ptr, b.ptr, b.ptr, 1, b.ptr, b.ptr, _stream()) < 0
    assert lib.lidargs_debug_sort_pairs(8, 2, b.ptr, b.ptr, b.ptr, b.ptr, 1, 16, 0, 0, b.ptr, None, 0, 0, 0, 0, 0, None, None, _stream()) < 0    # begin_bit
    assert lib.lidargs_debug_sort_pairs(8, 2, b.ptr, b.ptr, b.ptr, b.ptr, 0, 16, 9, 0, b.ptr, None, 0, 0, 0, 0, 0, None, None, _stream()) < 0    # wide digits
    assert lib.lidargs_debug_sort_pairs(8, 2, b.ptr, b.ptr, b.ptr, b.ptr, 0, 16, 0, 0, b.ptr, None, 0, 1, 0, 9, 0, None, None, _stream()) < 0    # bias
    assert lib.lidargs_debug_sort_pairs(8, 2, b.ptr, b.ptr, b.ptr, b.ptr, 0, 16, 0, 0, b.ptr, None, 0, 0, 0, 0, 1, b.ptr, b.ptr, _stream()) < 0  # tail
    assert lib.lidargs_debug_sort_pairs(8, 4, b.ptr, b.ptr, b.ptr, b.ptr, 0, 33, 0, 0, b.ptr, None, 0, 0, 0, 0, 0, None, None, _stream()) < 0    # end_bit
    b.read()


# ---- i. the forms an environment variable selects, read once per process: one child each --------------------------------------------
def _child_no_small_sort():
    for n in (1, 63, 65, 4096):          # three passes of the general form end on the b side; the single launch would bring them home
        rng = np.random.default_rng(n)
        check_sort(_random_keys(rng, n), _distinct_values(rng, n), scratch_bits=11, want_side="default", what=f"general n={n}")
        assert check_sort(_random_keys(rng, n), _distinct_values(rng, n), end=24, scratch_bits=11, want_side="default", what=f"general n={n} 24 bits") == 1
        check_sort(_random_keys(rng, n, 16), _distinct_values(rng, n), key_bytes=2, want_side="default", what=f"general 16-bit n={n}")


def _child_small_sort_up_to_16384():
    for n, general in ((4097, 0), (16383, 0), (16384, 0), (16385, 1)):
        rng = np.random.default_rng(n)
        check_sort(_random_keys(rng, n), _distinct_values(rng, n), scratch_bits=11, want_side="default", what=f"n={n}")
        assert check_sort(_random_keys(rng, n), _distinct_values(rng, n), end=24, scratch_bits=11, want_side="default", what=f"n={n} 24 bits") == general
        check_sort(_random_keys(rng, n, 16), _distinct_values(rng, n), key_bytes=2, want_side="default", what=f"16-bit n={n}")
        check_sort(_random_keys(rng, n), _distinct_values(rng, n), n_dev=n - 1, scratch_bits=11, what=f"n={n} count {n - 1}")


def _child_sort_items_16():
    for n in (4097, 8193):               # room for half blocks, and the variable says 4096-key blocks
        rng = np.random.default_rng(n)
        check_sort(_random_keys(rng, n), _distinct_values(rng, n), scratch_bits=11, want_side="default", what=f"n={n}")
        check_sort(_random_keys(rng, n), None, end=31, max_bits=11, scratch_bits=11, what=f"n={n} digits 11")


def _child_buckets_2048():
    for kind, P in BUCKET_CASES:
        for mode in (1, 2):
            check_bucketed_range_sort(kind, P, mode, spread=True)
    check_bucketed_range_sort("random_ranges", 30011, 1, spread=False)


CHILDREN = {"no_single_launch_sort": ({"LIDARGS_NO_SMALL_SORT": "1"}, _child_no_small_sort),
            "single_launch_sort_up_to_16384": ({"LIDARGS_SMALL_SORT_MAX": "16384"}, _child_small_sort_up_to_16384),
            "sort_blocks_of_4096": ({"LIDARGS_SORT_ITEMS": "16"}, _child_sort_items_16),
            "range_sort_2048_intervals": ({"LIDARGS_RANGE_SORT_BUCKET_BITS": "11"}, _child_buckets_2048)}


@pytest.mark.parametrize("name", list(CHILDREN))
def test_forms_selected_by_the_environment(name, hip_lib_built):
    run_child("import test_sort_gpu as t\nt.CHILDREN[sys.argv[1]][1]()\nprint('OK')", CHILDREN[name][0], (name,), timeout=300)
