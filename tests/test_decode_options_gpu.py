"""GPU tests of the decode's two model options: `neural_gaussians.generate_neural_gaussians` on a model with a feature bank
(use_feat_bank=True) and / or per-camera appearance embeddings (appearance_dim > 0) against (i) the fixture made by executing the
reference function + torch autograd (tests/golden/make_decode_options_golden.py) and (ii) the float64 restatement
tests/decode_options_ref.py on shapes the fixture lacks.  Tolerances are the plain decode's (tests/test_neural_gaussians_gpu.py):
parity() as it is for outputs and tensor gradients, rtol 5e-4 for parameter gradients (sums over all anchors, fp32 accumulation order)."""
import ctypes
import functools
import types

import numpy as np
import pytest

import decode_options_ref as ref
import lidargs_scenes as sc
from util import parity

pytestmark = pytest.mark.gpu
UP_SHAPES = lambda M: ((M, 3), (M, 2), (M, 1), (M, 3), (M, 4))


def run_hip(p, cam, vis, uid=0, ups=None, wrap_embeddings=False, pc=None, backward_twice=False):
    """Outputs (and, with `ups`, gradients under the names of decode_options_ref.run) of the product function on the model dict `p`."""
    import torch
    from neural_gaussians import generate_neural_gaussians
    pc = pc or ref.to_torch_model(p)
    if wrap_embeddings:                                                  # scene/embedding.py: the module holds the nn.Embedding as .embedding
        pc.get_appearance, pc.get_appearance_rd = (types.SimpleNamespace(embedding=e) for e in (pc.get_appearance, pc.get_appearance_rd))
    camera = types.SimpleNamespace(camera_center=torch.from_numpy(np.asarray(cam, np.float32)).cuda(), uid=uid)
    vmask = None if vis is None else torch.from_numpy(np.asarray(vis)).cuda()
    res = {}
    for _ in range(2 if backward_twice else 1):
        outs = generate_neural_gaussians(camera, pc, vmask, is_training=True)
        res = {k: v.detach().cpu().numpy() for k, v in zip(ref.OUT_KEYS, outs)}
        res["mask"] = outs[6].cpu().numpy()
        if ups is not None:
            torch.autograd.backward(list(outs[:5]), [torch.from_numpy(u).cuda() for u in ups])
    if ups is not None:
        if wrap_embeddings:
            pc.get_appearance, pc.get_appearance_rd = pc.get_appearance.embedding, pc.get_appearance_rd.embedding
        res.update(ref.model_grads(pc))
    return res


def compare(r, e, p, out_prefix=""):
    """HIP result `r` against expectations `e` (outputs under out_prefix + name, gradients under g_ + name): the plain decode's rules."""
    flips = int((r["mask"] != e[out_prefix + "mask"]).sum())
    assert flips == 0, f"{flips} opacity-sign flips"
    for k in ref.OUT_KEYS:
        parity(k, r[k], e[out_prefix + k])
    for k in ref.TENSOR_KEYS:
        parity("d" + k, r["g_" + k], e["g_" + k])
    for k in ref.param_keys(p):
        parity("d" + k, r["g_" + k], e["g_" + k], rtol=5e-4)


@pytest.mark.parametrize("tag", ["c", "d", "e", "f"])
def test_options_match_reference_golden(tag, hip_lib_built):
    p, cam, vis, uid, exp = ref.load_case(tag)
    r = run_hip(p, cam, vis, uid, [exp["up_" + k] for k in ("xyz", "color", "opacity", "scaling", "rot")])
    compare(r, exp, p, out_prefix="out_")
    if "emb_color" in p:
        for k in ("g_emb_color", "g_emb_raydrop"):                       # dense, as nn.Embedding's: only the camera's row is touched
            assert r[k].shape == p[k[2:]].shape and (np.delete(r[k], uid, axis=0) == 0).all() and np.abs(r[k][uid]).max() > 0
        assert r["g_color_W1"].shape == p["color_W1"].shape and r["g_raydrop_W1"].shape == p["raydrop_W1"].shape
    assert (r["g_anchor_feat"][~vis] == 0).all() and (r["g_anchor"][~vis] == 0).all()


# Shapes the fixture lacks, against the float64 restatement.  4099 anchors: 129 rounds of 32 with a ragged last one, more than one
# workgroup in every kernel and more than one row of partial sums; the seed is one where no opacity of the float64 reference lies within
# 5e-5 of the mask's edge (asserted), so a float32 sum cannot move an offset across it.  1 anchor; 33 anchors without a visibility mask.
# 70 001 anchors: 2188 rounds, more than the 2048 workgroups of k_bank_forward and the 1024 of k_bank_backward, so workgroups walk their
# grid-stride loops two and three times with a ragged last round -- the rows requested one round ahead are real ones, the flag and rows
# are carried into the next round, the LDS row of upstream gradients is reused behind the second barrier, a lane's 35 parameter sums
# run over several rounds -- and k_bank_fold adds the full 1024 partial rows (the product's size, 333 k anchors, is ~10 rounds each).
RANDOM = {
    "grid_stride_70001": dict(N=70001, k=4, seed=331, flags=(True, True, False), bank=True, A=32, vis=True, uid=1, steady_mask=True),
    "both_4099": dict(N=4099, k=6, seed=212, flags=(True, True, True), bank=True, A=32, vis=True, uid=2),
    "one_anchor": dict(N=1, k=4, seed=211, flags=(True, False, True), bank=True, A=8, vis=None, uid=0),
    "no_mask_33": dict(N=33, k=5, seed=223, flags=(False, True, False), bank=True, A=32, vis=None, uid=1),
}


@functools.lru_cache(maxsize=None)
def random_reference(name):
    c = RANDOM[name]
    p, cam, vis, rng = _draw(c)
    e = ref.run(p, cam, vis, c["uid"], lambda M: [rng.normal(size=s).astype(np.float32) for s in UP_SHAPES(M)])
    return p, cam, vis, c["uid"], e


def _draw(c):
    p, cam, vis, rng = sc.make_anchor_model(c["N"], c["k"], c["seed"], c["flags"])
    p = ref.random_options(p, c["seed"], bank=c["bank"], A=c["A"])
    if c.get("steady_mask"):
        # At this many opacities some always fall within float32 rounding of 0, and one flip shifts every later output row.  The mask is not
        # what this case is about: the opacity head gets small weights and biases of +-0.5, so every other offset is selected, far from the edge.
        p["opacity_W2"] = p["opacity_W2"] * np.float32(0.02)
        p["opacity_b2"] = np.where(np.arange(c["k"]) % 2 == 0, 0.5, -0.5).astype(np.float32)
    return p, cam, (vis if c["vis"] else None), rng


@pytest.mark.parametrize("name", list(RANDOM))
def test_options_match_restatement(name, hip_lib_built):
    p, cam, vis, uid, e = random_reference(name)
    assert float(np.abs(e["neural_opacity"]).min()) >= 5e-5, "pick another seed: an opacity of the reference sits on the mask's edge"
    r = run_hip(p, cam, vis, uid, e["ups"], wrap_embeddings=(name == "both_4099"))
    compare(r, e, p)
    for k in ("g_emb_color", "g_emb_raydrop"):
        assert (np.delete(r[k], uid, axis=0) == 0).all()


def test_grid_stride_rounds_are_reproducible(hip_lib_built):
    """The 70 001-anchor case twice: every gradient the bank kernels write or feed bit-equal (several rounds per workgroup, 1024 partial
    rows folded in a fixed order), and the invisible anchors' rows exactly zero."""
    p, cam, vis, uid, e = random_reference("grid_stride_70001")
    one, again = run_hip(p, cam, vis, uid, e["ups"]), run_hip(p, cam, vis, uid, e["ups"])
    for k in ref.OUT_KEYS + ("mask",):
        assert np.array_equal(one[k], again[k]), k
    for k in ref.TENSOR_KEYS + tuple(ref.param_keys(p)):
        assert np.array_equal(one["g_" + k], again["g_" + k]), k
    assert (one["g_anchor_feat"][~vis] == 0).all() and (one["g_anchor"][~vis] == 0).all() and np.abs(one["g_bank_W1"]).max() > 0


def test_nothing_visible(hip_lib_built):
    p, cam, vis, uid, _ = random_reference("no_mask_33")
    ups = [np.zeros(s, np.float32) for s in UP_SHAPES(0)]
    r = run_hip(p, cam, np.zeros(33, bool), uid, ups)
    assert r["xyz"].shape == (0, 3) and r["rot"].shape == (0, 4) and r["neural_opacity"].shape == (0, 1) and r["mask"].shape == (0,)
    for k in ref.TENSOR_KEYS + tuple(ref.param_keys(p)):
        assert r["g_" + k].shape == np.shape(p[k]) and (r["g_" + k] == 0).all(), k


def _plain_and(p_plain, p_opt, cam, vis, seed):
    """The plain decode of `p_plain` and the decode with options of `p_opt`, same upstream gradients."""
    plain = run_hip(p_plain, cam, vis, 0, None)
    rng = np.random.default_rng(seed)
    ups = [rng.normal(size=s).astype(np.float32) for s in UP_SHAPES(plain["xyz"].shape[0])]
    return run_hip(p_plain, cam, vis, 0, ups), run_hip(p_opt, cam, vis, 1, ups)


def test_zero_appearance_columns_are_bit_neutral(hip_lib_built):
    """W1[:, din:] = 0: b1_eff = b1 + 0 and the packed W1 is the plain model's, so the decode sees the same bits -- every output and every
    gradient the two models share is identical to the plain decode's, whatever the embeddings hold."""
    p, cam, vis, _ = sc.make_anchor_model(1500, 6, 301, (True, False, True))
    q = ref.random_options(p, 301, bank=False, A=32)
    for m in ("color", "raydrop"):
        q[m + "_W1"][:, 36:] = 0
    a, b = _plain_and(p, q, cam, vis, 302)
    for k in ref.OUT_KEYS + ("mask",):
        assert np.array_equal(a[k], b[k]), k
    for k in ref.TENSOR_KEYS + tuple(ref.param_keys(p)):
        ga, gb = a["g_" + k], b["g_" + k]
        assert np.array_equal(ga, gb[:, :36] if k in ("color_W1", "raydrop_W1") else gb), k
    assert (b["g_emb_color"] == 0).all() and np.abs(b["g_color_W1"][:, 36:]).max() > 0      # de = 0^T db1;  dW1[:, din:] = db1 (x) e


def test_bank_with_weights_0_0_1_is_bit_neutral(hip_lib_built):
    """W2 = 0 and b2 = (-1e4, -1e4, 0): the logits are b2 exactly, exp(-1e4) = 0, w = (0, 0, 1) exactly, feat' = feat -- bit-identical to
    the decode without a bank, gradients included (the bank passes dL_dfeat' through and adds an exact zero to dL_danchor)."""
    p, cam, vis, _ = sc.make_anchor_model(1500, 5, 311, (False, True, True))
    q = ref.random_options(p, 311, bank=True, A=0)
    q["bank_W2"][:] = 0
    q["bank_b2"] = np.array([-1e4, -1e4, 0.0], np.float32)
    a, b = _plain_and(p, q, cam, vis, 312)
    for k in ref.OUT_KEYS + ("mask",):
        assert np.array_equal(a[k], b[k]), k
    for k in ref.TENSOR_KEYS + tuple(ref.param_keys(p)):
        assert np.array_equal(a["g_" + k], b["g_" + k]), k
    for k in ("bank_W1", "bank_b1", "bank_W2", "bank_b2"):
        assert np.isfinite(b["g_" + k]).all()
    assert (b["g_bank_W1"] == 0).all() and (b["g_bank_b2"] == 0).all()    # dz = w (dw - w.dw) = 0 at a one-hot w


def test_backward_is_reproducible_and_accumulates(hip_lib_built):
    """Two backward runs of one frame: bit-equal bank and embedding gradients (fixed summation order, no atomics).  Two frames of the
    same camera without zeroing .grad: the sums, as torch accumulates them -- x + x = 2x exactly -- and only row uid of the embeddings."""
    p, cam, vis, uid, e = random_reference("both_4099")
    one, again = run_hip(p, cam, vis, uid, e["ups"]), run_hip(p, cam, vis, uid, e["ups"])
    new = [k for k in ref.param_keys(p) if k.startswith(("bank_", "emb_"))] + ["color_W1", "raydrop_W1", "anchor", "anchor_feat"]
    for k in new:
        assert np.array_equal(one["g_" + k], again["g_" + k]), k
    twice = run_hip(p, cam, vis, uid, e["ups"], backward_twice=True)
    for k in new:
        assert np.array_equal(twice["g_" + k], 2 * one["g_" + k]), k
    assert (np.delete(twice["g_emb_color"], uid, axis=0) == 0).all() and np.abs(twice["g_emb_color"][uid]).max() > 0


def test_bank_forward_through_the_c_abi_writes_every_row(hip_lib_built):
    """lidargs_ng_bank_forward on an output prefilled with NaN: rows of visible anchors are feat', rows of invisible anchors are ZEROS
    (the decode's tile kernels load the rows of a whole tile before they know the flags: none is left unwritten, see the header)."""
    import torch
    import neural_gaussians as prod
    from diff_lidargs_rasterization import _C as base
    p, cam, vis, uid, e = random_reference("both_4099")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    feat, anchor, W1, b1, W2, b2 = (t(p[k]) for k in ("anchor_feat", "anchor", "bank_W1", "bank_b1", "bank_W2", "bank_b2"))
    mask = t(vis).view(torch.uint8)
    out = torch.full((4099, 32), float("nan"), device="cuda")
    camv = (ctypes.c_float * 3)(*[float(c) for c in cam])
    rc = prod._options_lib().lidargs_ng_bank_forward(4099, base._ptr(mask), base._ptr(feat), base._ptr(anchor), camv, base._ptr(W1), base._ptr(b1),
                                           base._ptr(W2), base._ptr(b2), base._ptr(out), base._stream(out.device))
    assert rc == 0
    got = out.cpu().numpy()
    assert np.isfinite(got[vis]).all() and (got[~vis] == 0).all() and (~vis).sum() > 0
    T = {k: torch.from_numpy(np.asarray(p[k], np.float64)) for k in ("bank_W1", "bank_b1", "bank_W2", "bank_b2")}
    ob = torch.from_numpy(p["anchor"][vis].astype(np.float64)) - torch.from_numpy(np.asarray(cam, np.float64))
    dist = ob.norm(dim=1, keepdim=True)
    w = ref.mlp(torch.cat([ob / dist, dist], 1), T["bank_W1"], T["bank_b1"], T["bank_W2"], T["bank_b2"], lambda z: torch.softmax(z, 1)).numpy()
    f = p["anchor_feat"][vis].astype(np.float64)
    want = np.tile(f[:, ::4], (1, 4)) * w[:, 0:1] + np.tile(f[:, ::2], (1, 2)) * w[:, 1:2] + f * w[:, 2:3]
    parity("feat'", got[vis], want)


def test_refusals_on_the_device(hip_lib_built):
    import torch
    from torch import nn
    from neural_gaussians import generate_neural_gaussians
    p, cam, vis, uid, _ = random_reference("no_mask_33")
    camera = types.SimpleNamespace(camera_center=torch.from_numpy(np.asarray(cam, np.float32)).cuda(), uid=3)
    pc = ref.to_torch_model(p)
    with pytest.raises(IndexError):                                      # three cameras: uid 3 is out of range, as nn.Embedding says
        generate_neural_gaussians(camera, pc)
    camera.uid = 0
    good = pc.get_appearance
    pc.get_appearance = nn.Embedding(3, 32)                              # weights left on the host
    with pytest.raises(RuntimeError, match="HIP device"):
        generate_neural_gaussians(camera, pc)
    pc.get_appearance = torch.jit.trace(good, (torch.zeros(1, dtype=torch.long, device="cuda"),))
    with pytest.raises(NotImplementedError, match="get_appearance"):
        generate_neural_gaussians(camera, pc)
    pc.get_appearance = good
    pc.get_featurebank_mlp = nn.Sequential(nn.Linear(4, 32), nn.ReLU(True), nn.Linear(32, 3)).cuda()
    with pytest.raises(NotImplementedError, match="feature-bank"):
        generate_neural_gaussians(camera, pc)
    pc.get_featurebank_mlp = pc.mlp_feature_bank
    assert generate_neural_gaussians(camera, pc)[0].shape[1] == 3       # and the model as built decodes
