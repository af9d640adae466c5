"""GPU tests of the range-shell path through the C ABI shell entry points
(lidargs_forward_shell / lidargs_render_shell / lidargs_backward_shell).

Only one GPU is available to the tests, so N virtual ranks run as N Python threads on cuda:0 with
an in-memory communicator; the collectives' semantics are the same as TorchDistComm's (which the
world_size-2 gloo tests cover on CPU).  Expected result: the plain single-process oracle."""
import threading

import numpy as np
import pytest
import torch

import lidargs_scenes as sc
from util import GRAD_KEYS_SR, make_settings, oracle_forward_backward, parity, to_torch

pytestmark = pytest.mark.gpu


class ThreadComm:
    """All ranks live in one process: all_gather/all_reduce through shared slots + a barrier.

    The virtual ranks share ONE device and ONE stream, and the library's contract is one caller thread per stream
    (INTEGRATION.md section 3), so the rank threads take turns: a rank holds `turn` whenever it runs (library calls, torch ops)
    and gives it up only while it waits at a collective.  The schedule is then that of a single caller interleaving the ranks
    phase by phase, which is what N processes on N GPUs amount to -- without 8 threads enqueueing on one stream at once."""

    class Shared:
        def __init__(self, world):
            self.world, self.slots, self.barrier = world, [None] * world, threading.Barrier(world)
            self.turn = threading.Lock()

    def __init__(self, shared, rank):
        self.sh, self.rank, self.world = shared, rank, shared.world
        self.sh.turn.acquire()               # released while waiting in _exchange and by finish()

    def finish(self):
        if self.sh.turn.locked():
            try:
                self.sh.turn.release()
            except RuntimeError:
                pass

    def _wait(self):
        self.sh.turn.release()
        try:
            self.sh.barrier.wait(timeout=240)
        finally:
            self.sh.turn.acquire()

    def _exchange(self, t):
        torch.cuda.synchronize()
        self.sh.slots[self.rank] = t
        self._wait()
        vals = list(self.sh.slots)
        self._wait()
        return vals

    def all_gather(self, t):
        return torch.stack(self._exchange(t.contiguous().clone()), 0)

    def broadcast(self, t, src=0):
        return self._exchange(t)[src].clone()

    def all_reduce(self, t):
        t.copy_(torch.stack(self._exchange(t.clone()), 0).sum(0))
        return t

    def all_reduce_async(self, t):
        self.all_reduce(t)
        return lambda: None

    def all_reduce_max_async(self, t):
        t.copy_(torch.stack(self._exchange(t.clone()), 0).max(0).values)
        return lambda: None

    def all_to_all_rows(self, t, send_counts, recv_counts):
        vals = self._exchange((t.contiguous().clone(), list(send_counts)))
        parts = []
        for src, (ts, sc) in enumerate(vals):
            o = sum(sc[:self.rank])
            parts.append(ts[o:o + sc[self.rank]])
            assert sc[self.rank] == recv_counts[src]
        return torch.cat(parts, 0)

    def reduce_scatter_rows(self, t):
        rows = t.shape[0] // self.world
        full = torch.stack(self._exchange(t.clone()), 0).sum(0)
        return full[self.rank * rows:(self.rank + 1) * rows].clone()


def _run_rank(shared, rank, scene, W, H, grads, grad_sync, results, wedges=False, edges=None, frames=1, enqueue=False, ship_live=None):
    """Drives lidargs_dist.shell_forward / shell_backward (or the wedge pair) directly: torch's autograd engine executes all
    CUDA nodes on ONE worker thread per device, which would serialise (and deadlock) the virtual ranks."""
    comm = None
    try:
        import lidargs_dist
        torch.cuda.set_device(0)
        comm = ThreadComm(shared, rank)
        st = to_torch(scene)
        gc, gd, go = (torch.from_numpy(g).cuda() for g in grads)
        if wedges:
            mod = lidargs_dist.WedgeRasterizer(make_settings(st, W, H), comm, grad_sync=grad_sync, edges=edges)
            fwd, bwd = lidargs_dist.wedge_forward, lidargs_dist.wedge_backward
        else:
            mod = lidargs_dist.ShellRasterizer(make_settings(st, W, H), comm, grad_sync=grad_sync)
            fwd, bwd = lidargs_dist.shell_forward, lidargs_dist.shell_backward
        mod.enqueue_only = enqueue
        if ship_live is not None:
            mod.ship_live = ship_live
        elif int(st["means3D"].shape[0]) < 1_000_000:
            mod.ship_live = int(st["means3D"].shape[0]) % 2 == 1      # both forms of the gradient exchange at test sizes ("auto" turns the live form on for the full-size cfg4 frames only)
        for _ in range(frames):          # (enqueue-only: the first frame is an ordinary one and teaches the plan its capacities)
            (color, depth, occ, radii), saved = fwd(mod, st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"])
            g = bwd(mod, saved, gc, gd, go)
        if grad_sync == "shard":         # [rows_r, w] chunks -> dense [P, w] with zeros outside, so that the checks of "reduce_scatter" apply
            P = int(st["means3D"].shape[0])
            base, n = lidargs_dist.shard_rows(P, comm.world, rank)
            dense = {}
            for k, t in g.items():
                assert t.shape[0] == n, (k, t.shape, n)
                dense[k] = torch.zeros((P,) + tuple(t.shape[1:]), device=t.device); dense[k][base:base + n] = t
            g = dense
        mod.plan.check()
        results[rank] = dict(enqueue_only_frames=mod.plan.frames, color=color.cpu().numpy(), depth=depth.cpu().numpy(), occ=occ.cpu().numpy(), radii=radii.cpu().numpy(),
                             dL_dmeans3D=g["means3D"].cpu().numpy(), dL_dmeans2D=g["means2D"].cpu().numpy(),
                             dL_dcolors=g["colors"].cpu().numpy(), dL_dopacity=g["opacities"].cpu().numpy(),
                             dL_dscales=g["scales"].cpu().numpy(), dL_drotations=g["rotations"].cpu().numpy())
    except Exception as e:  # pragma: no cover
        results[rank] = e
        shared.barrier.abort()
    finally:
        if comm is not None:
            comm.finish()


CASES = [
    ("w1", 1, "shell", 8000, 16, 512, 51, (0.0, 0.0), "all_reduce"),
    ("w2_bg", 2, "street", 20000, 16, 512, 52, (0.3, 0.6), "all_reduce"),
    ("w4_dense", 4, "street", 60000, 32, 800, 53, (0.2, 0.1), "all_reduce"),
    ("w4_sparse_exchange", 4, "street", 50001, 32, 800, 54, (0.0, 0.2), "reduce_scatter"),
    ("w3_dense_exchange", 3, "shell", 20000, 16, 512, 55, (0.1, 0.0), "reduce_scatter_dense"),
    ("w4_shard", 4, "street", 50003, 32, 800, 56, (0.1, 0.2), "shard"),      # round 6: the rank's own chunk of every gradient (lidargs_shell_unpack_grad_rows_chunk)
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_shell_path_on_hip_matches_oracle(case, hip_lib_built):
    name, world, kind, P, H, W, seed, bg, grad_sync = case
    scene = sc.make_scene(kind, P, H, seed, random_view=True)
    scene["bg"] = np.array(bg, np.float32)
    grads = sc.upstream_grads(H, W, seed)
    ref = oracle_forward_backward(scene, W, H, grads)
    shared = ThreadComm.Shared(world)
    results = [None] * world
    threads = [threading.Thread(target=_run_rank, args=(shared, r, scene, W, H, grads, grad_sync, results)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=480)
    assert not any(t.is_alive() for t in threads), "virtual ranks hung"
    for r in results:
        if isinstance(r, Exception):
            raise r
        assert r is not None
    for r in range(world):
        mism = int((results[r]["radii"] != ref["radii"]).sum())
        assert mism <= max(1, int(1e-4 * P))
        for k in ("color", "depth", "occ"):
            parity(f"{k}@r{r}", results[r][k], ref[k], verbose=(r == 0))
    rows = (P + world - 1) // world
    for k in GRAD_KEYS_SR:
        if grad_sync == "all_reduce":
            full = results[0][k]
        else:       # rank r holds rows [r*rows, (r+1)*rows) and zeros elsewhere
            full = np.zeros_like(ref[k])
            for r in range(world):
                sl = slice(r * rows, min(P, (r + 1) * rows))
                full[sl] = results[r][k][sl]
                outside = np.ones(P, bool); outside[sl] = False
                assert float(np.abs(results[r][k][outside]).max(initial=0.0)) == 0.0
        parity(k, full, ref[k])


@pytest.mark.parametrize("P,H,W", [(6000, 16, 512), (300, 8, 64)], ids=["fused_plan", "one_segment"])
def test_single_shell_straight_through_the_abi(P, H, W, hip_lib_built):
    """A direct C-ABI caller renders ONE shell: lidargs_forward_shell with T_in = NULL, T_out = NULL, transmittance_pass = 0, then
    lidargs_backward_shell.  (lidargs_dist always goes through a transmittance pass, so nothing else in the suite takes this route.)
    The forward used to infer "this is a shell" from those three arguments, picked the fused blend for such a call, and the shell
    backward -- which walks the slot grid with the segmented launches' flags and limits -- read planes and flags nobody had written
    (round-3 advisor finding).  The mode is now the entry point's.  Expected: the plain path's image and gradients."""
    import ctypes as C
    import lidargs_dist
    from util import hip_forward_backward
    scene = sc.make_scene("street", P, H, 77, random_view=True)
    grads = sc.upstream_grads(H, W, 77)
    plain = hip_forward_backward(scene, W, H, grads)
    st = to_torch(scene)
    be = lidargs_dist.HipShellBackend()
    _C, lib = be._C, be.lib
    dev = st["means3D"].device
    geom, binning, img = _C._Scratch(dev), _C._Scratch(dev), _C._Scratch(dev)
    N = H * W
    out = torch.full((4 * N,), float("nan"), dtype=torch.float32, device=dev)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    p = _C._ptr
    inf = float("inf")
    with torch.cuda.device(dev):
        R = lib.lidargs_forward_shell(_C._alloc_cb, geom.user, _C._alloc_cb, binning.user, _C._alloc_cb, img.user, C.c_int(P), p(st["bg"]),
                                      C.c_int(W), C.c_int(H), p(st["means3D"]), p(st["colors"]), p(st["opacities"]), p(st["scales"]),
                                      C.c_float(1.0), p(st["rotations"]), None, p(st["viewmatrix"]), p(st["beams"]), C.c_int(80), C.c_int(0),
                                      C.c_float(-inf), C.c_float(inf), None, C.c_int(0), p(out), p(out[2 * N:]), p(out[3 * N:]), None,
                                      p(radii), None, C.c_int(0), _C._stream(dev))
    assert R >= 0, _C._last_error() if hasattr(_C, "_last_error") else R
    gb, bb, ib = geom.take(), binning.take(), img.take()
    color, depth, occ = out[:2 * N].view(2, H, W), out[2 * N:3 * N].view(1, H, W), out[3 * N:].view(1, H, W)
    assert np.array_equal(radii.cpu().numpy(), plain["radii"])
    for k, v in (("color", color), ("depth", depth), ("occ", occ)):
        parity("single shell " + k, v.cpu().numpy(), plain[k])
    widths = (3, 4, 2, 1, 3, 4)
    slab = torch.full((P * sum(widths),), float("nan"), dtype=torch.float32, device=dev)
    parts, o = [], 0
    for w in widths:
        parts.append(slab[o:o + P * w].view(P, w)); o += P * w
    g_m3, g_m2, g_col, g_op, g_sc, g_rot = parts
    gc, gd, go = (torch.from_numpy(g).to(dev).contiguous() for g in grads)
    with torch.cuda.device(dev):
        rc = lib.lidargs_backward_shell(C.c_int(P), C.c_int(R), p(st["bg"]), C.c_int(W), C.c_int(H), p(st["means3D"]), p(st["colors"]),
                                        p(st["scales"]), C.c_float(1.0), p(st["rotations"]), None, p(st["viewmatrix"]), p(st["beams"]),
                                        p(radii), p(gb), p(bb), p(ib), None, None, p(gc), p(gd), p(go), p(g_m2), None, p(g_op), p(g_col),
                                        None, p(g_m3), None, None, None, None, p(g_sc), p(g_rot), C.c_int(0), _C._stream(dev))
    assert rc >= 0, rc
    for k, v in (("dL_dmeans3D", g_m3), ("dL_dmeans2D", g_m2), ("dL_dcolors", g_col), ("dL_dopacity", g_op), ("dL_dscales", g_sc),
                 ("dL_drotations", g_rot)):
        parity("single shell " + k, v.cpu().numpy().reshape(plain[k].shape), plain[k])


def test_rccl_collectives_world_of_one(hip_lib_built):
    """Only one GPU is visible to the tests, so RCCL can only be exercised with a world of one -- which still checks every
    torch.distributed call the product makes (dtypes, shapes, split lists, async handle) against the real backend, and the
    whole shell path with TorchDistComm in place of the in-memory communicator."""
    import os
    import socket
    import torch.distributed as dist
    import lidargs_dist
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        comm = lidargs_dist.TorchDistComm()
        dev = torch.device("cuda", 0)
        t = torch.arange(12, dtype=torch.float32, device=dev).view(3, 4)
        assert torch.equal(comm.all_gather(t), t.unsqueeze(0))
        r = torch.arange(5, dtype=torch.int32, device=dev)
        wait = comm.all_reduce_async(r); wait()
        assert torch.equal(r, torch.arange(5, dtype=torch.int32, device=dev))
        rows = torch.randn(7, 18, device=dev)
        assert torch.equal(comm.all_to_all_rows(rows, [7], [7]), rows)
        assert comm.all_to_all_rows(rows[:0], [0], [0]).shape == (0, 18)
        assert torch.equal(comm.all_to_all_rows(r.view(-1, 1), [5], [5]).view(-1), r)
        assert torch.equal(comm.reduce_scatter_rows(rows), rows)
        assert torch.equal(comm.all_reduce(rows.clone()), rows)
        assert torch.equal(comm.broadcast(rows.clone(), 0), rows)
        # the whole path on the RCCL communicator
        kind, P, H, W, seed = "street", 20000, 16, 512, 61
        scene = sc.make_scene(kind, P, H, seed, random_view=True)
        grads = sc.upstream_grads(H, W, seed)
        ref = oracle_forward_backward(scene, W, H, grads)
        st = to_torch(scene)
        mod = lidargs_dist.ShellRasterizer(make_settings(st, W, H), comm, grad_sync="reduce_scatter")
        (color, depth, occ, radii), saved = lidargs_dist.shell_forward(mod, st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"])
        g = lidargs_dist.shell_backward(mod, saved, *(torch.from_numpy(x).cuda() for x in grads))
        parity("color", color.cpu().numpy(), ref["color"]); parity("depth", depth.cpu().numpy(), ref["depth"])
        parity("dL_dmeans3D", g["means3D"].cpu().numpy(), ref["dL_dmeans3D"])
        parity("dL_drotations", g["rotations"].cpu().numpy(), ref["dL_drotations"])
    finally:
        dist.destroy_process_group()


def test_shell_exchange_helpers_match_framework_ops(hip_lib_built):
    """lidargs_shell_{pack,unpack}_grad_rows, _chunk_counts, _scatter_radii against the framework ops they replace (bit for bit:
    they only move data), including empty inputs and both dense layouts."""
    import lidargs_dist
    be = lidargs_dist.HipShellBackend()
    g = torch.Generator(device="cpu").manual_seed(5)
    P, world = 10007, 3
    for M in (0, 1, 4321):
        idx = torch.sort(torch.randperm(P, generator=g)[:M]).values.to(torch.int32).cuda()
        grads = {k: torch.randn((M, w), generator=g).cuda() for k, w in lidargs_dist.GRAD_WIDTHS}
        rows = be.pack_rows(grads, idx)
        ref_rows = torch.cat([grads[k] for k, _ in lidargs_dist.GRAD_WIDTHS] + [idx.view(torch.float32).view(-1, 1)], dim=1)
        assert torch.equal(rows.view(torch.int32), ref_rows.view(torch.int32))
        ref_dense = torch.zeros((P, lidargs_dist.GRAD_COLS), device="cuda")
        ref_dense[idx.long()] = ref_rows[:, :lidargs_dist.GRAD_COLS]
        assert torch.equal(be.unpack_rows(rows, P), ref_dense)
        flat, o = be.unpack_rows(rows, P, blocked=True), 0
        for k, w in lidargs_dist.GRAD_WIDTHS:
            assert torch.equal(flat[o * P:(o + w) * P].view(P, w), ref_dense[:, o:o + w]), k
            o += w
        chunk = lidargs_dist._chunk_rows(P, world)
        counts = torch.full((world,), -1.0, device="cuda")
        be.chunk_counts(idx, chunk, world, counts)
        ref_counts = torch.bincount(idx.long() // chunk, minlength=world).float()
        assert torch.equal(counts, ref_counts)
        radii_shell = torch.randint(1, 50, (M,), generator=g).to(torch.int32).cuda()
        ref_radii = torch.zeros(P, dtype=torch.int32, device="cuda")
        ref_radii[idx.long()] = radii_shell
        assert torch.equal(be.scatter_radii(idx, radii_shell, P), ref_radii)


@pytest.mark.parametrize("world", [1, 3, 8])
def test_selection_leaves_the_split_sizes_of_the_gradient_exchange(world, hip_lib_built):
    """select(..., chunks=...): the all-to-all's split sizes come out of the selection's own gather launch (read off the scan), in
    the ordinary and the enqueue-only form, shells and wedges -- equal to a bincount of the selected indices over the index chunks."""
    import types
    import lidargs_dist
    be = lidargs_dist.HipShellBackend()
    kind, P, H, W, seed = "street", 30011, 16, 512, 93
    st = to_torch(sc.make_scene(kind, P, H, seed, random_view=True))
    inp = dict(means3D=st["means3D"], colors=st["colors"], opacities=st["opacities"], scales=st["scales"], rotations=st["rotations"],
               viewmatrix=st["viewmatrix"], W=W, H=H, scale_modifier=1.0)
    chunk = lidargs_dist._chunk_rows(P, world)
    for wedge in (False, True):
        sel = (lambda plan, chunks: be.select_wedge(inp, 64, 256, plan, chunks=chunks)) if wedge else (lambda plan, chunks: be.select(inp, 12.0, 30.0, plan, chunks=chunks))
        idx0, _ = sel(None, None)
        M = int(idx0.shape[0])
        assert 0 < M < P
        ref = torch.bincount(idx0.long() // chunk, minlength=world).float()
        counts = torch.full((world,), -1.0, device="cuda")
        idx1, _ = sel(None, (chunk, world, counts))
        assert torch.equal(idx1, idx0) and torch.equal(counts, ref)
        plan = types.SimpleNamespace(rows=M + 100, status=torch.zeros(18, dtype=torch.int32).pin_memory())
        counts.fill_(-1.0)
        idx2, s2 = sel(plan, (chunk, world, counts))
        torch.cuda.synchronize()
        assert torch.equal(idx2[:M], idx0) and bool((idx2[M:] == 0x7F7F7F7F).all()) and torch.equal(counts, ref)
        assert s2["n_valid"].tolist() == [M, M] and plan.status[16:].tolist() == [M, M]
        plan.rows = M // 2                                                       # over capacity: clamped, and reported
        idx3, s3 = sel(plan, (chunk, world, counts))
        torch.cuda.synchronize()
        assert torch.equal(idx3, idx0[:M // 2]) and s3["n_valid"].tolist() == [M // 2, M] and float(counts.sum()) == M // 2


@pytest.mark.parametrize("world", [1, 3, 8])
def test_live_rows_of_the_gradient_exchange(world, hip_lib_built):
    """Round 6: lidargs_shell_pack_grad_rows_live_count / _live -- only the rows that carry a gradient travel.  Against framework ops: the same
    rows per destination chunk (as sets: the order inside a group is free), the same counts; rows with an index outside [0, P) (the tail of
    a capacity-sized selection), all-zero frames and a frame where every row is live included."""
    import lidargs_dist
    from dist_backend_oracle import OracleShellBackend
    be, ob = lidargs_dist.HipShellBackend(), OracleShellBackend()
    rng = np.random.default_rng(7 + world)
    P, M = 100_003, 41_000
    chunk = lidargs_dist._chunk_rows(P, world)
    for frac in (0.0, 0.03, 1.0):
        idx = np.sort(rng.choice(P, M - 50, replace=False)).astype(np.int32)
        idx = np.concatenate([idx, np.full(50, 0x7F7F7F7F, np.int32)])
        g = {k: rng.normal(size=(M, w)).astype(np.float32) for k, w in lidargs_dist.GRAD_WIDTHS}
        dead = rng.random(M) >= frac
        for k in g:
            g[k][dead] = 0.0
        if frac == 0.03:
            g["opacities"][5] = 1e-30; g["rotations"][7, 3] = -0.0        # one tiny value is live, a negative zero is not
        tg = {k: torch.from_numpy(v).cuda() for k, v in g.items()}
        ti = torch.from_numpy(idx).cuda()
        cnt = be.count_rows_live(tg, ti, P, chunk, world)
        send = cnt[:world].tolist()
        rows = be.pack_rows_live(tg, ti, P, chunk, world, cnt, sum(send))
        cg, ci = {k: torch.from_numpy(v) for k, v in g.items()}, torch.from_numpy(idx)
        rcnt = ob.count_rows_live(cg, ci, P, chunk, world)
        rsend = rcnt[:world].tolist()
        rrows = ob.pack_rows_live(cg, ci, P, chunk, world, rcnt, sum(rsend))
        assert send == rsend and sum(send) == rows.shape[0], (frac, send, rsend)
        rows = rows.cpu()
        o = 0
        for d in range(world):
            a, b = rows[o:o + send[d]], rrows[o:o + send[d]]
            ka = torch.argsort(a[:, 17].contiguous().view(torch.int32)); kb = torch.argsort(b[:, 17].contiguous().view(torch.int32))
            assert torch.equal(a[ka].view(torch.int32), b[kb].view(torch.int32)), (frac, d)
            o += send[d]


@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 3_000_017])
def test_one_launch_selection_equals_the_two_step_one(P, hip_lib_built, monkeypatch):
    """Round 6: k_select_fused (test + scan by decoupled look-back over the blocks + gather, one launch) against rounds 2-5's flags -> scan ->
    gather: the same rows in the same (ascending index) order, bit for bit, shells and wedges, at block-boundary sizes and at 3 M rows
    (2930 blocks looking back), with split sizes; run twice (the look-back's words are zeroed per call)."""
    import lidargs_dist
    st = to_torch(sc.make_scene("street", P, 16, 95, random_view=True))
    inp = dict(means3D=st["means3D"], colors=st["colors"], opacities=st["opacities"], scales=st["scales"], rotations=st["rotations"],
               viewmatrix=st["viewmatrix"], W=512, H=16, scale_modifier=1.0)
    world = 8
    chunk = lidargs_dist._chunk_rows(P, world)
    for wedge in (False, True):
        out = {}
        for fused in (False, True):
            monkeypatch.setattr(lidargs_dist, "_SELECT_FUSED", fused)
            be = lidargs_dist.HipShellBackend()
            for rep in range(2):
                counts = torch.full((world,), -1.0, device="cuda")
                idx, sel = (be.select_wedge(inp, 64, 256, None, chunks=(chunk, world, counts)) if wedge else be.select(inp, 12.0, 30.0, None, chunks=(chunk, world, counts)))
                out[(fused, rep)] = (idx.clone(), {k: sel[k].clone() for k in ("means3D", "colors", "opacities", "scales", "rotations")}, counts.clone())
        ref = out[(False, 0)]
        for key, (idx, rows, counts) in out.items():
            assert torch.equal(idx, ref[0]) and torch.equal(counts, ref[2]), (P, wedge, key)
            for k in rows:
                assert torch.equal(rows[k], ref[1][k]), (P, wedge, key, k)
        if P > 2000:
            assert 0 < int(ref[0].shape[0]) < P


def test_cfg4_sharded_over_8_virtual_ranks_at_full_size(hip_lib_built):
    """BASELINE config 4 in its stated form, as far as one GPU allows: the 8 M-Gaussian 128 x 4096 scene sharded into 8 range
    shells, every shell driven through the product path (lidargs_shell_select -> forward phase 1 -> transmittance -> phase 2 ->
    compose -> backward -> pack / all-to-all / unpack) by its own virtual rank.  The composed image and the index-chunked
    gradients must equal the plain single-GPU path within the summation-order band, and the oracle on an azimuth wedge.
    (What stays untested here: RCCL with more than one rank.)"""
    from test_fullsize_gpu import _wedge_subset
    from util import hip_forward_backward
    world, grad_sync = 8, "reduce_scatter"
    kind, P, H, W, seed = sc.BASELINE_CONFIGS["cfg4"]
    scene = sc.make_scene(kind, P, H, seed)
    grads = sc.upstream_grads(H, W, seed)
    plain = hip_forward_backward(scene, W, H, grads)
    shared = ThreadComm.Shared(world)
    results = [None] * world
    threads = [threading.Thread(target=_run_rank, args=(shared, r, scene, W, H, grads, grad_sync, results)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=900)
    assert not any(t.is_alive() for t in threads), "virtual ranks hung"
    for r in results:
        if isinstance(r, Exception):
            raise r
        assert r is not None
    # every rank composed the same image; it equals the plain path's (different summation order across shells: 1e-4 metric)
    for r in range(world):
        assert np.array_equal(results[r]["radii"], plain["radii"]), f"radii differ on rank {r}"
        for k in ("color", "depth", "occ"):
            if r:
                assert np.array_equal(results[r][k], results[0][k]), (k, r)
            else:
                parity(f"cfg4x8.{k} vs plain", results[0][k], plain[k])
    rows = (P + world - 1) // world
    full = {}
    for k in GRAD_KEYS_SR:
        full[k] = np.zeros_like(plain[k])
        for r in range(world):
            sl = slice(r * rows, min(P, (r + 1) * rows))
            full[k][sl] = results[r][k][sl]
            outside = np.ones(P, bool); outside[sl] = False
            assert float(np.abs(results[r][k][outside]).max(initial=0.0)) == 0.0, (k, r)
        parity(f"cfg4x8.{k} vs plain", full[k], plain[k])
    # and against the oracle, on a wedge (as tests/test_fullsize_gpu.py does for the plain path)
    c0 = (W // 2 - 64) // 16 * 16
    c1 = c0 + 128
    keep = _wedge_subset(scene, W, plain["radii"], c0, c1)
    sub = dict(scene)
    for k in ("means3D", "scales", "rotations", "opacities", "colors"):
        sub[k] = np.ascontiguousarray(scene[k][keep])
    ref = oracle_forward_backward(sub, W, H, grads)
    for k in ("color", "depth", "occ"):
        parity(f"cfg4x8.{k}[{c0}:{c1}] vs oracle", results[0][k][..., c0:c1], ref[k][..., c0:c1])
    rws = np.nonzero(keep)[0]
    m2 = ref["fwd"].array("means2D").reshape(-1, 2)
    rx = ref["fwd"].array("radii_xy").reshape(-1, 2)[:, 0].astype(np.float64)
    inside = (ref["radii"] > 0) & (np.floor((m2[:, 0] - rx) / 16.0) * 16 >= c0) & (np.floor((m2[:, 0] + rx + 15.0) / 16.0) * 16 <= c1)
    assert inside.sum() > 2000
    for k in GRAD_KEYS_SR:
        parity(f"cfg4x8.{k}[wedge] vs oracle", full[k][rws[inside]], ref[k][inside])


# ---- column wedges -------------------------------------------------------------------------------------------------------------
def _virtual_ranks(world, scene, W, H, grads, grad_sync, wedges, edges=None, timeout=900, frames=1, enqueue=False, ship_live=None):
    shared = ThreadComm.Shared(world)
    results = [None] * world
    threads = [threading.Thread(target=_run_rank, args=(shared, r, scene, W, H, grads, grad_sync, results, wedges, edges, frames, enqueue, ship_live)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "virtual ranks hung"
    for r in results:
        if isinstance(r, Exception):
            raise r
        assert r is not None
    return results


def _assemble(results, ref_like, P, world, grad_sync):
    rows = (P + world - 1) // world
    full = {}
    for k in GRAD_KEYS_SR:
        if grad_sync == "all_reduce":
            full[k] = results[0][k]
            continue
        full[k] = np.zeros_like(ref_like[k])
        for r in range(world):
            sl = slice(r * rows, min(P, (r + 1) * rows))
            full[k][sl] = results[r][k][sl]
            outside = np.ones(P, bool); outside[sl] = False
            assert float(np.abs(results[r][k][outside]).max(initial=0.0)) == 0.0, (k, r)
    return full


WEDGE_CASES = [
    ("w1", 1, "shell", 8000, 16, 512, 81, (0.0, 0.0), "all_reduce", None),
    ("w2_bg", 2, "street", 20000, 16, 512, 82, (0.3, 0.6), "all_reduce", None),
    ("w4_dense", 4, "street", 60000, 32, 800, 83, (0.2, 0.1), "reduce_scatter", None),
    ("w3_ragged", 3, "shell", 20001, 18, 500, 84, (0.1, 0.0), "reduce_scatter", None),                   # W % 16 != 0, odd P
    ("w5_one_tile_wedges", 5, "street", 30000, 64, 600, 85, (0.0, 0.2), "reduce_scatter", [0, 16, 32, 304, 592, 600]),
    ("w4_shard", 4, "street", 40003, 32, 800, 86, (0.1, 0.1), "shard", None),            # round 6 (boundary Gaussians' rows are added inside the chunk)
]


@pytest.mark.parametrize("case", WEDGE_CASES, ids=[c[0] for c in WEDGE_CASES])
def test_wedge_path_on_hip_matches_plain_and_oracle(case, hip_lib_built):
    """Column wedges through the C ABI (lidargs_wedge_select_count / lidargs_forward_wedge / lidargs_backward / pack / unpack-add)
    by virtual ranks: the composed image must be BIT-IDENTICAL to the plain single-GPU forward (a rank's tile lists are the
    complete lists), radii equal, gradients within the summation-order band of the plain path and within parity of the oracle."""
    from util import hip_forward_backward
    name, world, kind, P, H, W, seed, bg, grad_sync, edges = case
    scene = sc.make_scene(kind, P, H, seed, random_view=True)
    scene["bg"] = np.array(bg, np.float32)
    grads = sc.upstream_grads(H, W, seed)
    plain = hip_forward_backward(scene, W, H, grads)
    ref = oracle_forward_backward(scene, W, H, grads)
    results = _virtual_ranks(world, scene, W, H, grads, grad_sync, True, edges)
    for r in range(world):
        assert np.array_equal(results[r]["radii"], plain["radii"])
        for k in ("color", "depth", "occ"):
            assert np.array_equal(results[r][k], plain[k]), (k, r)      # bit for bit
    full = _assemble(results, ref, P, world, grad_sync)
    for k in GRAD_KEYS_SR:
        parity(f"{k} vs plain", full[k], plain[k], verbose=False)
        parity(k, full[k], ref[k])


def test_cfg4_column_wedges_over_8_virtual_ranks_at_full_size(hip_lib_built):
    """BASELINE config 4 (8 M Gaussians @ 128 x 4096) over 8 column wedges: image bit-identical to the plain single-GPU path,
    index-chunked gradients within the summation-order band."""
    from util import hip_forward_backward
    world, grad_sync = 8, "reduce_scatter"
    kind, P, H, W, seed = sc.BASELINE_CONFIGS["cfg4"]
    scene = sc.make_scene(kind, P, H, seed)
    grads = sc.upstream_grads(H, W, seed)
    plain = hip_forward_backward(scene, W, H, grads)
    results = _virtual_ranks(world, scene, W, H, grads, grad_sync, True)
    for r in range(world):
        assert np.array_equal(results[r]["radii"], plain["radii"]), f"radii differ on rank {r}"
        for k in ("color", "depth", "occ"):
            assert np.array_equal(results[r][k], plain[k]), (k, r)
    full = _assemble(results, plain, P, world, grad_sync)
    for k in GRAD_KEYS_SR:
        parity(f"cfg4 wedges x8 {k} vs plain", full[k], plain[k])


@pytest.mark.parametrize("wedges,grad_sync", [(False, "reduce_scatter"), (True, "reduce_scatter"), (False, "all_reduce")],
                         ids=["shells", "wedges", "shells_all_reduce"])
def test_enqueue_only_rank_frames_match_ordinary_ones(wedges, grad_sync, hip_lib_built):
    """`module.enqueue_only`: after one ordinary frame a rank's frames read nothing back -- capacity-row selection with the count on the
    device (lidargs_*_select_enqueue, k_preprocess' n_valid), capacity-sized binning (lidargs_forward_*_enqueue), the all-to-all's
    split sizes and the status words through pinned memory.  Same radii; images and gradients equal to the ordinary frames' up to
    the grouping of the partial sums (the segment plan follows the capacity), and within parity of the oracle."""
    world, kind, P, H, W, seed = 4, "street", 60000, 32, 800, 91
    scene = sc.make_scene(kind, P, H, seed, random_view=True)
    scene["bg"] = np.array((0.2, 0.1), np.float32)
    grads = sc.upstream_grads(H, W, seed)
    ref = oracle_forward_backward(scene, W, H, grads)
    plain = _virtual_ranks(world, scene, W, H, grads, grad_sync, wedges)
    res = _virtual_ranks(world, scene, W, H, grads, grad_sync, wedges, frames=3, enqueue=True)
    for r in range(world):
        assert res[r]["enqueue_only_frames"] == 2 and plain[r]["enqueue_only_frames"] == 0
        assert np.array_equal(res[r]["radii"], plain[r]["radii"])
        for k in ("color", "depth", "occ"):
            parity(f"{k} rank {r} vs ordinary", res[r][k], plain[r][k], verbose=False)
            parity(f"{k} rank {r}", res[r][k], ref[k], verbose=False)
    full, full_plain = _assemble(res, ref, P, world, grad_sync), _assemble(plain, ref, P, world, grad_sync)
    for k in GRAD_KEYS_SR:
        parity(f"{k} vs ordinary", full[k], full_plain[k], verbose=False)
        parity(k, full[k], ref[k])


@pytest.mark.parametrize("wedges", [False, True], ids=["shells", "wedges"])
@pytest.mark.parametrize("what", ["rows", "instances"])
def test_enqueue_only_rank_frame_over_its_capacity_is_reported(wedges, what, hip_lib_built):
    """A frame that selected more rows, or needed more list instances, than its capacities: nothing is written out of bounds, and
    the plan raises (at the next look at its status words) and grows."""
    import lidargs_dist
    kind, P, H, W, seed = "street", 20000, 16, 512, 92
    st = to_torch(sc.make_scene(kind, P, H, seed, random_view=True))
    gc, gd, go = (torch.from_numpy(g).cuda() for g in sc.upstream_grads(H, W, seed))
    mod = (lidargs_dist.WedgeRasterizer if wedges else lidargs_dist.ShellRasterizer)(make_settings(st, W, H))
    mod.enqueue_only = True
    fwd, bwd = (lidargs_dist.wedge_forward, lidargs_dist.wedge_backward) if wedges else (lidargs_dist.shell_forward, lidargs_dist.shell_backward)
    args = (st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"])
    out0, saved = fwd(mod, *args)                      # ordinary frame: teaches the plan
    g0 = bwd(mod, saved, gc, gd, go)
    rows, inst = mod.plan.rows, mod.plan.instances
    assert rows > 0 and inst > 0
    if what == "rows":
        mod.plan.rows = 1000
    else:
        mod.plan.instances = 4096
    out1, saved = fwd(mod, *args)
    with pytest.raises(RuntimeError, match="enqueue-only rank frame"):      # the frame's own backward reports it, in every sync mode
        bwd(mod, saved, gc, gd, go)
    assert (mod.plan.rows if what == "rows" else mod.plan.instances) >= (rows if what == "rows" else inst) / 1.3      # grown back
    out2, saved = fwd(mod, *args)                      # the next frame has room again
    g2 = bwd(mod, saved, gc, gd, go)
    mod.plan.check()
    assert torch.equal(out2[3], out0[3])
    for a, b in zip(out2[:3], out0[:3]):
        parity("image after regrowth", a.cpu().numpy(), b.cpu().numpy(), verbose=False)
    for k in g0:
        parity(f"{k} after regrowth", g2[k].cpu().numpy(), g0[k].cpu().numpy(), verbose=False)


def test_wedge_with_no_gaussian_in_reach(hip_lib_built):
    """A rank whose columns no Gaussian can reach (the scene covers half of the azimuth range): zero selected rows through
    every stage (select, forward, backward, pack, all-to-all, unpack) -- its columns come out as background, nothing hangs."""
    from util import hip_forward_backward
    world, grad_sync = 4, "reduce_scatter"
    P, H, W, seed = 12000, 16, 512, 91
    scene = sc.make_scene("shell", P, H, seed)
    az = np.arctan2(scene["means3D"][:, 1], scene["means3D"][:, 0])
    keep = (az > 0.2) & (az < 2.9)                      # projected columns ~ [20, 240) of 512: the last two wedges stay empty
    for k in ("means3D", "scales", "rotations", "opacities", "colors"):
        scene[k] = np.ascontiguousarray(scene[k][keep])
    P = int(keep.sum())
    scene["bg"] = np.array([0.4, 0.1], np.float32)
    grads = sc.upstream_grads(H, W, seed)
    plain = hip_forward_backward(scene, W, H, grads)
    results = _virtual_ranks(world, scene, W, H, grads, grad_sync, True, [0, 128, 256, 384, 512])
    assert float(np.abs(plain["color"][0][:, 400:] - 0.4).max()) == 0.0     # really empty there
    for r in range(world):
        assert np.array_equal(results[r]["radii"], plain["radii"])
        for k in ("color", "depth", "occ"):
            assert np.array_equal(results[r][k], plain[k]), (k, r)
    full = _assemble(results, plain, P, world, grad_sync)
    for k in GRAD_KEYS_SR:
        parity(f"{k} vs plain", full[k], plain[k], verbose=False)


@pytest.mark.parametrize("wedges", [False, True], ids=["shells", "wedges"])
def test_empty_model_with_live_rows_forced_on(wedges, hip_lib_built):
    """P = 0 with `ship_live` forced on: an empty model has no index chunks to count live rows into (lidargs_shell_pack_grad_rows_live_count
    refuses chunk_rows = 0), so its exchange ships every selected row -- none.  Every rank: the background image, no radii, empty gradients."""
    world, H, W, seed = 2, 16, 512, 97
    scene = sc.make_scene("street", 1000, H, seed, random_view=True)
    for k in ("means3D", "scales", "rotations", "opacities", "colors"):
        scene[k] = np.ascontiguousarray(scene[k][:0])
    scene["bg"] = np.array([0.3, 0.6], np.float32)
    results = _virtual_ranks(world, scene, W, H, sc.upstream_grads(H, W, seed), "reduce_scatter", wedges, ship_live=True)
    bg = np.broadcast_to(scene["bg"].reshape(2, 1, 1), (2, H, W))
    for r in range(world):
        assert results[r]["radii"].shape == (0,)
        assert np.array_equal(results[r]["color"], bg) and not results[r]["depth"].any() and not results[r]["occ"].any()
        for k, w in zip(GRAD_KEYS_SR, (3, 4, 2, 1, 3, 4)):
            assert results[r][k].shape == (0, w), (k, r)


# ---- bench.py's sharded legs ------------------------------------------------------------------------------------------------------
def _bench(*args, env=None, timeout=900):
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *args], env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_bench_sharded_legs_with_a_world_of_one(hip_lib_built):
    """The code the driver's N > 1 bench runs (both cuts timed one after the other over the RCCL communicator, rebalancing rounds,
    one JSON line carrying `cuts`, `config.sharding`, `rccl_ranks`, `roofline`) with the only world this box can form."""
    j = _bench("--workload", "cfg2", "--fwd-bwd", "--steps", "4", "--warmup", "2", "--no-cpu-baseline", env={"LIDARGS_BENCH_FORCE_SHELLS": "1"})
    assert j["rccl_ranks"] == 1 and set(j["cuts"]) == {"shells", "wedges"}
    assert j["config"]["sharding"] in ("1 range shells", "1 column wedges")
    assert abs(j["value"] - max(c["value"] for c in j["cuts"].values())) < 1e-6 * j["value"]
    assert j["roofline"].get("frac", 0) > 0, j["roofline"]
    for c in j["cuts"].values():
        assert c["ms_per_step"] > 0 and len(c["edges"]) == 2


def test_bench_two_ranks_sharing_one_device(hip_lib_built):
    """`python bench.py --gpus 2` end to end on a one-GPU box: LIDARGS_BENCH_ONE_DEVICE=1 puts both self-launched ranks on device 0 and routes the
    collectives through gloo with host staging.  Everything of the N > 1 bench but RCCL itself runs: the launcher, the rendezvous, both cuts with
    their rebalancing rounds (an all-gather of the ranks' measured times), the max over the ranks, rank 0's single JSON line."""
    j = _bench("--gpus", "2", "--workload", "cfg2", "--fwd-bwd", "--steps", "4", "--warmup", "2", "--no-cpu-baseline", env={"LIDARGS_BENCH_ONE_DEVICE": "1"}, timeout=1500)
    assert j["n_gpus"] == 2 and j["rccl_ranks"] == 2 and set(j["cuts"]) == {"shells", "wedges"}
    assert j["config"]["sharding"] in ("2 range shells", "2 column wedges")
    assert abs(j["value"] - max(c["value"] for c in j["cuts"].values())) < 1e-6 * j["value"]
    for c in j["cuts"].values():
        assert c["ms_per_step"] > 0 and len(c["edges"]) == 3


def test_bench_two_ranks_over_rccl(hip_lib_built):
    """`python bench.py --gpus 2` with no launcher in front: self-launched ranks, RCCL over xGMI, both cuts.  Needs two devices."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip(f"RCCL with more than one rank needs two HIP devices; this box has {n} (covered by gloo world-2 on CPU and by "
                    f"virtual ranks on one GPU)")
    j = _bench("--gpus", "2", "--workload", "cfg2", "--fwd-bwd", "--steps", "5", "--warmup", "2")
    assert j["n_gpus"] == 2 and j["rccl_ranks"] == 2 and set(j["cuts"]) == {"shells", "wedges"}


@pytest.mark.gpu
def test_enqueue_only_overflow_survives_a_second_forward(hip_lib_built):
    """Two forwards with no backward between them (an eval render, or a frame whose backward comes later): the second forward's status
    copy reuses the pinned words, so the first frame's overflow must be read -- and raised -- before it is queued (round-4 advisor finding:
    a non-waiting look returned early with the host running ahead, and the flag was overwritten)."""
    import lidargs_dist
    kind, P, H, W, seed = "street", 20000, 16, 512, 93
    st = to_torch(sc.make_scene(kind, P, H, seed, random_view=True))
    mod = lidargs_dist.ShellRasterizer(make_settings(st, W, H))
    mod.enqueue_only = True
    args = (st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"])
    with torch.no_grad():
        lidargs_dist.shell_forward(mod, *args)         # ordinary frame: teaches the plan
        mod.plan.instances = 4096
        lidargs_dist.shell_forward(mod, *args)         # over its capacity; nobody looks yet
        with pytest.raises(RuntimeError, match="enqueue-only rank frame"):
            lidargs_dist.shell_forward(mod, *args)     # the next frame reads the old status first
        lidargs_dist.shell_forward(mod, *args)         # capacities were raised: fine again
        mod.plan.check()
