"""The numpy restatement of scatter_max / scatter_min (include_scatter/lidargs_scatter.h): the definition the device is compared with.

A plain loop over the elements in position order.  An element replaces what a group holds only if it is strictly greater (max) or
smaller (min) under the total order in which +0.0 > -0.0, or if it is a NaN and what the group holds is not: so the lowest position wins
among equal values, the first NaN wins its group, and a NaN result is the canonical quiet NaN.  A group starts from `out`'s value if
`out` is given (a kept initial value keeps its bits and has arg = E) and otherwise holds nothing: then it ends as (0, E).
`skip_bad` restates what the kernels do with an index value outside [0, G) through the C ABI: the element takes part in nothing."""
import numpy as np

MAX, MIN = 0, 1


def _rank(op, x):
    """int64 ranks of float32 values that compare like the values do here: the float's bits mapped to the total order with -0.0 < +0.0
    (1 .. 2^32 - 2), and every NaN at the winning end (max: 2^32, min: -1), so that a NaN beats every number and no NaN beats a NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    r = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(x), (1 << 32) if op == MAX else -1, r)


def broadcast_index(index, shape, dim):
    """torch_scatter's `broadcast`: a 1-D index goes to `dim`, missing trailing dimensions are added, then it is expanded."""
    index = np.asarray(index)
    dim = dim % len(shape)
    if index.ndim == 1:
        index = index.reshape((1,) * dim + index.shape)
    index = index.reshape(index.shape + (1,) * (len(shape) - index.ndim))
    return np.broadcast_to(index, shape)


def scatter_extreme(op, src, index, dim=-1, out=None, dim_size=None, skip_bad=False):
    """(out float32, arg int64) of src (float32, any rank >= 1) and index (int64, 1-D or broadcastable)."""
    src = np.asarray(src, dtype=np.float32)
    dim = dim % src.ndim
    idx = broadcast_index(index, src.shape, dim)
    E = src.shape[dim]
    if out is not None:
        G = out.shape[dim]
    elif dim_size is not None:
        G = int(dim_size)
    else:
        G = int(np.asarray(index).max()) + 1 if np.asarray(index).size else 0
    s = np.moveaxis(src, dim, 0).reshape(E, -1)
    ix = np.moveaxis(idx, dim, 0).reshape(E, -1)
    C = s.shape[1]
    shape = (G,) + np.moveaxis(src, dim, 0).shape[1:]
    init = np.zeros((G, C), dtype=np.float32) if out is None else np.moveaxis(np.asarray(out, dtype=np.float32), dim, 0).reshape(G, C)
    nothing = -2 if op == MAX else (1 << 32) + 1              # what a group that holds nothing compares as: every element beats it
    held = (np.full((G, C), nothing, dtype=np.int64) if out is None else _rank(op, init)).tolist()
    arg = np.full((G, C), E, dtype=np.int64).tolist()
    rank, groups = _rank(op, s).tolist(), ix.tolist()
    for e in range(E):                                        # position order; strict comparison: the first of equals stays
        for c in range(C):
            g = groups[e][c]
            if not 0 <= g < G:
                if skip_bad:
                    continue
                raise IndexError(g)
            if rank[e][c] > held[g][c] if op == MAX else rank[e][c] < held[g][c]:
                held[g][c], arg[g][c] = rank[e][c], e
    arg = np.array(arg, dtype=np.int64).reshape(G, C)
    val = init.copy()                                         # a kept initial value keeps its bits; an empty group is 0
    won = arg < E
    if won.any():
        picked = s[arg[won], np.nonzero(won)[1]]
        val[won] = np.where(np.isnan(picked), np.float32(np.nan), picked)          # a NaN result is the canonical quiet NaN
    return np.moveaxis(val.reshape(shape), 0, dim), np.moveaxis(arg.reshape(shape), 0, dim)


def scatter_max(src, index, dim=-1, out=None, dim_size=None, **kw):
    return scatter_extreme(MAX, src, index, dim, out, dim_size, **kw)


def scatter_min(src, index, dim=-1, out=None, dim_size=None, **kw):
    return scatter_extreme(MIN, src, index, dim, out, dim_size, **kw)


def scatter_extreme_grad(grad_out, index, arg, src_shape, dim=-1):
    """grad_src: grad_out at the `arg` positions, 0 everywhere else (an element whose index value is outside the groups gets 0)."""
    dim = dim % len(src_shape)
    idx = np.moveaxis(broadcast_index(index, src_shape, dim), dim, 0)
    go, ar = np.moveaxis(np.asarray(grad_out, dtype=np.float32), dim, 0), np.moveaxis(np.asarray(arg), dim, 0)
    G, E = ar.shape[0], idx.shape[0]
    if G == 0 or idx.size == 0:
        return np.moveaxis(np.zeros(idx.shape, dtype=np.float32), 0, dim)
    ok = (idx >= 0) & (idx < G)
    group = np.where(ok, idx, 0)
    position = np.arange(E).reshape((E,) + (1,) * (idx.ndim - 1))
    won = ok & (np.take_along_axis(ar, group, 0) == position)
    return np.moveaxis(np.where(won, np.take_along_axis(go, group, 0), np.float32(0)).astype(np.float32), 0, dim)


def same_bits(a, b):
    """Equal bit for bit (NaNs and signed zeros included), same shape and dtype."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
