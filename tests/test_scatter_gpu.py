"""GPU tests of the torch_scatter stand-in: scatter_max / scatter_min on the device against the numpy restatement tests/scatter_ref.py,
bit for bit (values, signed zeros, NaNs and the winning positions), at the small shapes where the kernels can go wrong: one element, the
sizes around a wave (63, 64, 65), several workgroups with a ragged tail (4097), one, 32 and 33 columns, an outer dimension, every form of
index, maximum and no contention, empty groups, ties, +-0, +-inf, NaN and `out=` initial values.  Then torch's own device reduction, the
gradient, the reference's own call, and the C ABI with index values outside the groups between sentinel-filled guards."""
import ctypes

import numpy as np
import pytest
import torch

import scatter_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS = ("max", "min")
LEVELS = np.float32([-2.0, -0.0, 0.0, 1.5])                  # ties on purpose, and both zeros
SPECIAL = np.float32([np.inf, -np.inf, np.nan, np.nan])


def fns(op):
    import torch_scatter as ts
    return (ts.scatter_max, ref.scatter_max) if op == "max" else (ts.scatter_min, ref.scatter_min)


def tied_values(rng, shape):
    """Values from four levels, with about 3 % of +-inf and NaN (and at least one of each when there is room)."""
    v = LEVELS[rng.integers(0, 4, shape)]
    flat = v.reshape(-1)
    k = min(flat.size // 2, max(4, flat.size // 32))
    where = rng.choice(flat.size, k, replace=False)
    flat[where] = SPECIAL[np.arange(k) % 4]
    return flat.reshape(shape)


def index_of(rng, kind, shape, dim, G):
    """(the index as the device call gets it, the same index as numpy) for src of `shape` reduced along `dim` into G groups."""
    E = shape[dim]
    if kind == "full":                                       # differs per column
        ix = rng.integers(0, G, shape)
        return torch.from_numpy(ix).to(DEV), ix
    ix = rng.integers(0, G, E)
    if kind == "one_group":
        ix[:] = 0
    elif kind == "own_group":
        ix = rng.permutation(E)
    t = torch.from_numpy(ix).to(DEV)
    if kind == "expand":                                     # stride 0 everywhere but at dim, the reference's form
        view = [1] * len(shape)
        view[dim] = E
        t = t.view(view).expand(shape)
        assert all(st == 0 for k, (st, n) in enumerate(zip(t.stride(), shape)) if k != dim % len(shape) and n > 1)
    return t, ix


def check(op, src, t_index, np_index, dim, out=None, dim_size=None):
    """Device against restatement, bit for bit, twice."""
    dev_fn, ref_fn = fns(op)
    want_v, want_a = ref_fn(src, np_index, dim=dim, out=out, dim_size=dim_size)
    t_src = torch.from_numpy(src).to(DEV)
    got = []
    for _ in range(2):
        t_out = None if out is None else torch.tensor(out, device=DEV)     # (a copy: the call writes into it)
        v, a = dev_fn(t_src, t_index, dim=dim, out=t_out, dim_size=dim_size)
        assert out is None or v is t_out
        assert v.dtype == torch.float32 and a.dtype == torch.int64 and v.shape == a.shape == want_v.shape
        got.append((v.cpu().numpy(), a.cpu().numpy()))
    assert np.array_equal(got[0][1], want_a), "arg"
    assert ref.same_bits(got[0][0], want_v), "values"
    assert ref.same_bits(got[0][0], got[1][0]) and ref.same_bits(got[0][1], got[1][1]), "two calls differ"
    return want_v, want_a


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("B", [1, 32, 33])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 4097])
def test_rows_by_columns_with_the_expanded_index(op, E, B):
    rng = np.random.default_rng(E * 100 + B)
    G = E // 3 + 1
    src = tied_values(rng, (E, B))
    t, ix = index_of(rng, "expand", src.shape, 0, G)
    v, a = check(op, src, t, ix, 0)
    if E == 4097:
        assert np.isnan(v).any() and np.isinf(v).any() and (a < E).any()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("kind", ["1d", "expand", "full"])
@pytest.mark.parametrize("shape,dim", [((65, 3, 11), 0), ((3, 65, 33), 1), ((3, 33, 65), -1), ((3, 4097, 2), 1), ((4097,), 0)])
def test_three_dimensions_every_dim_and_every_form_of_index(op, kind, shape, dim):
    rng = np.random.default_rng(sum(shape) + dim)
    src = tied_values(rng, shape)
    t, ix = index_of(rng, kind, shape, dim, 7)
    check(op, src, t, ix, dim)


@pytest.mark.parametrize("op", OPS)
def test_contention_empty_groups_and_odd_layouts(op):
    rng = np.random.default_rng(5)
    src = tied_values(rng, (4097, 2))
    for kind in ("one_group", "own_group"):                  # every element to one key; every element its own
        t, ix = index_of(rng, kind, src.shape, 0, 4097)
        v, a = check(op, src, t, ix, 0)
        assert v.shape[0] == (1 if kind == "one_group" else 4097)
    t, ix = index_of(rng, "1d", src.shape, 0, 40)
    v, a = check(op, src, t, ix, 0, dim_size=64)             # trailing empty groups: (0, E)
    assert not v[ix.max() + 1:].any() and (a[ix.max() + 1:] == 4097).all() and v.shape[0] == 64
    # a src that is not contiguous, and an index whose expanded view has no three strides (it is copied)
    dev_fn, ref_fn = fns(op)
    base = tied_values(rng, (33, 65))
    ix = rng.integers(0, 9, 65)
    v, a = dev_fn(torch.from_numpy(base).to(DEV).t(), torch.from_numpy(ix).to(DEV), dim=0)
    want = ref_fn(np.ascontiguousarray(base.T), ix, dim=0)
    assert ref.same_bits(v.cpu().numpy(), want[0]) and np.array_equal(a.cpu().numpy(), want[1])
    src4 = tied_values(rng, (2, 3, 65, 4))
    ix4 = rng.integers(0, 9, (1, 3, 65, 4))
    v, a = dev_fn(torch.from_numpy(src4).to(DEV), torch.from_numpy(ix4).to(DEV), dim=2)
    want = ref_fn(src4, np.broadcast_to(ix4, src4.shape), dim=2)
    assert ref.same_bits(v.cpu().numpy(), want[0]) and np.array_equal(a.cpu().numpy(), want[1])
    # nothing to reduce, nothing to write: answered without a native call
    v, a = dev_fn(torch.zeros(0, 4, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), dim=0, dim_size=3)
    assert v.shape == a.shape == (3, 4) and not v.any() and (a == 0).all()
    v, a = dev_fn(torch.zeros(0, 4, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), dim=0)
    assert v.shape == a.shape == (0, 4)
    v, a = dev_fn(torch.zeros(5, 0, device=DEV), torch.arange(5, device=DEV), dim=0)
    assert v.shape == a.shape == (5, 0)


@pytest.mark.parametrize("op", OPS)
def test_initial_values_that_win_tie_and_lose(op):
    rng = np.random.default_rng(9)
    E, B, G = 257, 33, 40
    src = tied_values(rng, (E, B))
    t, ix = index_of(rng, "expand", src.shape, 0, 30)        # groups 30 .. 39 have no member: their initial values stay
    out = tied_values(rng, (G, B))                           # the same levels: wins, ties and losses all occur, and NaN / inf initial values
    out[5].view(np.uint32)[:] = 0xFFC12345                   # a NaN with a payload, kept bit for bit where it is the initial value
    v, a = check(op, src, t, ix, 0, out=out)
    kept = a == E
    assert kept[30:].all() and ref.same_bits(v[30:], out[30:]) and kept[:30].any() and (~kept[:30]).any()
    assert ref.same_bits(v[kept], out[kept]) and (v[5].view(np.uint32) == 0xFFC12345).all()
    won = ~kept & ~np.isnan(v)
    beats = (lambda x, y: x > y) if op == "max" else (lambda x, y: x < y)
    assert won.any() and not beats(out[won], v[won]).any()
    # an `out` that is not contiguous comes back as the same tensor, filled
    import torch_scatter as ts
    dev_fn, ref_fn = fns(op)
    wide = torch.from_numpy(np.ascontiguousarray(out.T)).to(DEV)                           # [B, G]; its transpose is the [G, B] out
    got_v, got_a = dev_fn(torch.from_numpy(src).to(DEV), t, dim=0, out=wide.t())
    assert got_v.data_ptr() == wide.data_ptr() and ref.same_bits(wide.t().cpu().numpy(), v) and np.array_equal(got_a.cpu().numpy(), a)
    assert ref.same_bits(ts.scatter(torch.from_numpy(src).to(DEV), t, dim=0, out=torch.tensor(out, device=DEV), reduce=op).cpu().numpy(), v)


@pytest.mark.parametrize("op", OPS)
def test_values_equal_torch_device_scatter_reduce_bit_for_bit(op):
    """NaN-free data without tied zeros: there a maximum has one answer, and torch's own device op must give it too."""
    dev_fn, _ = fns(op)
    g = torch.Generator().manual_seed(3)
    src = torch.randn(4097, 33, generator=g).to(DEV)
    idx = torch.randint(0, 1300, (4097,), generator=g).to(DEV)
    full = idx.unsqueeze(1).expand(-1, 33)
    v, a = dev_fn(src, full, dim=0, dim_size=1400)
    want = torch.zeros(1400, 33, device=DEV).scatter_reduce_(0, full, src, "amax" if op == "max" else "amin", include_self=False)
    assert torch.equal(v.view(torch.int32), want.view(torch.int32))
    hit = a < 4097
    assert torch.equal(src.gather(0, a.clamp(max=4096))[hit], v[hit]) and not v[~hit].any()


@pytest.mark.parametrize("op", OPS)
def test_backward_equals_the_restated_gradient(op):
    import torch_scatter as ts
    dev_fn, ref_fn = fns(op)
    rng = np.random.default_rng(21)
    for shape, dim, kind in (((4097, 33), 0, "expand"), ((3, 65, 33), 1, "1d"), ((3, 33, 65), -1, "full")):
        src = LEVELS[rng.integers(0, 4, shape)]              # ties: the whole gradient goes to the lowest position, none to the others
        t, ix = index_of(rng, kind, shape, dim, 50)
        t_src = torch.from_numpy(src).to(DEV).requires_grad_()
        v, a = dev_fn(t_src, t, dim=dim, dim_size=60)
        assert v.requires_grad and not a.requires_grad
        node = v.grad_fn                                     # (behind the view that gives the result src's rank)
        while not hasattr(node, "saved_tensors"):
            node = node.next_functions[0][0]
        saved = node.saved_tensors                           # nothing but the index and arg
        assert len(saved) == 2 and all(s.dtype == torch.int64 for s in saved) and saved[0].untyped_storage().data_ptr() == t.untyped_storage().data_ptr()
        grad_out = rng.standard_normal(tuple(v.shape)).astype(np.float32)
        v.backward(torch.from_numpy(grad_out).to(DEV))
        want = ref.scatter_extreme_grad(grad_out, ix, a.cpu().numpy(), shape, dim)
        assert ref.same_bits(t_src.grad.cpu().numpy(), want) and np.count_nonzero(want) <= a.numel()
        with torch.no_grad():
            assert dev_fn(t_src, t, dim=dim)[0].grad_fn is None
    # through the C ABI into a buffer of 0xFF bytes: every element of grad_src is written
    E, B, G = 4097, 33, 60
    src = LEVELS[rng.integers(0, 4, (E, B))]
    ix = rng.integers(-1, G + 1, E)                          # with values outside the groups: their gradient is 0
    a = ref_fn(src, ix, dim=0, dim_size=G, skip_bad=True)[1]
    grad_out = rng.standard_normal((G, B)).astype(np.float32)
    t_ix, t_a, t_go = torch.from_numpy(ix).to(DEV), torch.from_numpy(a).to(DEV), torch.from_numpy(grad_out).to(DEV)
    grad_src = torch.full((E, B), -1, dtype=torch.int32, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    assert ts._lib.lidargs_scatter_extreme_backward(1, E, B, G, p(t_ix), 0, 1, 0, p(t_a), p(t_go), p(grad_src), ts._stream(t_ix)) == 0
    assert ref.same_bits(grad_src.view(torch.float32).cpu().numpy(), ref.scatter_extreme_grad(grad_out, ix, a, (E, B), 0))


def test_the_reference_call_on_5000_features():
    """scene/gaussian_model.py:742: scatter_max(new_feat, inverse_indices.unsqueeze(1).expand(-1, new_feat.size(1)), dim=0)[0][remove_duplicates]"""
    from torch_scatter import scatter_max
    rng = np.random.default_rng(742)
    feat = rng.standard_normal((5000, 32)).astype(np.float32)
    _, inv = np.unique(rng.integers(0, 12, (5000, 3)), axis=0, return_inverse=True)        # voxel coordinates -> about 1 700 groups
    inv = inv.reshape(-1)
    G = int(inv.max()) + 1
    assert 1500 < G < 1800
    keep = rng.random(G) < 0.6
    new_feat, inverse_indices, remove_duplicates = torch.from_numpy(feat).to(DEV), torch.from_numpy(inv).to(DEV), torch.from_numpy(keep).to(DEV)
    got = scatter_max(new_feat, inverse_indices.unsqueeze(1).expand(-1, new_feat.size(1)), dim=0)[0][remove_duplicates]
    want = ref.scatter_max(feat, inv, dim=0)[0][keep]
    assert got.shape == (int(keep.sum()), 32) and ref.same_bits(got.cpu().numpy(), want)


@pytest.mark.parametrize("op", OPS)
def test_c_abi_skips_index_values_outside_the_groups_and_writes_inside_its_buffers_only(op, monkeypatch):
    import torch_scatter as ts
    dev_fn, ref_fn = fns(op)
    rng = np.random.default_rng(77)
    E, B, G, guard = 4097, 33, 50, 8                         # guard rows of B elements on both sides of out, arg and the scratch
    src = tied_values(rng, (E, B))
    ix = rng.integers(0, G, E)
    ix[rng.choice(E, 400, replace=False)] = np.resize(np.int64([-1, G, G + 1, 1 << 40, -(1 << 62), np.iinfo(np.int64).min, np.iinfo(np.int64).max]), 400)
    want_v, want_a = ref_fn(src, ix, dim=0, dim_size=G, skip_bad=True)
    t_src, t_ix = torch.from_numpy(src).to(DEV), torch.from_numpy(ix).to(DEV)
    rows = G + 2 * guard
    out = torch.full((rows, B), -7.25, device=DEV)
    arg = torch.full((rows, B), -99, dtype=torch.int64, device=DEV)
    scratch = torch.full((rows, B), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)     # (the keys are 8 bytes an element, as arg)
    nb = ts._lib.lidargs_scatter_scratch_bytes(G * B)
    assert nb == G * B * 8
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = ts._lib.lidargs_scatter_extreme(ts.MAX if op == "max" else ts.MIN, 1, E, B, G, p(t_src), p(t_ix), 0, 1, 0, 0,
                                         p(out[guard:]), p(arg[guard:]), p(scratch[guard:]), nb, ts._stream(t_src))
    assert rc == 0, ts._lib.lidargs_scatter_last_error()
    out, arg, scratch = out.cpu().numpy(), arg.cpu().numpy(), scratch.cpu().numpy()
    for buf, sentinel in ((out, -7.25), (arg, -99), (scratch, 0x5A5A5A5A5A5A5A5A)):
        assert (buf[:guard] == sentinel).all() and (buf[guard + G:] == sentinel).all()
    assert ref.same_bits(out[guard:guard + G], want_v) and np.array_equal(arg[guard:guard + G], want_a)
    # the Python binding reads the index's range and raises instead
    for bad in (-1, G):
        one = t_ix.clamp(0, G - 1).clone()
        one[E // 2] = bad
        with pytest.raises(IndexError, match="outside the"):
            dev_fn(t_src, one, dim=0, dim_size=G)
    # scratch filled with 0xFF bytes before the library sees it: nothing is assumed about its content
    good = torch.from_numpy(np.where((ix >= 0) & (ix < G), ix, 0)).to(DEV)
    with pytest.raises(IndexError, match="outside the"):      # the number of groups is out's
        dev_fn(t_src, good, dim=0, out=torch.zeros(int(good.max()), B, device=DEV))
    first = dev_fn(t_src, good, dim=0, dim_size=G)
    monkeypatch.setenv("LIDARGS_POISON_SCRATCH", "1")
    again = dev_fn(t_src, good, dim=0, dim_size=G)
    assert ref.same_bits(first[0].cpu().numpy(), again[0].cpu().numpy()) and torch.equal(first[1], again[1])


def test_the_front_refuses_what_does_not_broadcast_and_what_the_key_cannot_hold():
    import torch_scatter as ts
    src, index = torch.zeros(4, 3, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="HIP device"):
        ts.scatter_max(src, index.cpu(), dim=0)
    with pytest.raises(RuntimeError, match="does not broadcast"):
        ts.scatter_max(src, index[:3], dim=0)
    with pytest.raises(RuntimeError, match="does not broadcast"):
        ts.scatter_max(src, torch.zeros(4, 2, dtype=torch.int64, device=DEV), dim=0)
    with pytest.raises(RuntimeError, match="out of range"):
        ts.scatter_max(src, index, dim=2)
    with pytest.raises(RuntimeError, match="does not match"):
        ts.scatter_max(src, index, dim=0, out=torch.zeros(2, 4, device=DEV))
    huge = torch.zeros(1, device=DEV).expand(1 << 31)        # a shape, no memory
    with pytest.raises(RuntimeError, match=r"below 2\^31"):
        ts.scatter_max(huge, torch.zeros(1, dtype=torch.int64, device=DEV).expand(1 << 31))
