"""Generates tests/golden/decode_options_golden.npz by EXECUTING the reference's own `generate_neural_gaussians`
(gaussian_renderer/__init__.py:17-119 of the reference checkout) on CPU torch, forward and autograd backward, for models built with the two
options the plain decode's fixture (make_neural_gaussians_golden.py) leaves off: use_feat_bank=True and appearance_dim > 0.

As there, the function's source is read from the reference checkout at run time and executed (nothing of it is stored here), and
the `pc` it receives is a plain object carrying the tensors and the modules built as GaussianModel.__init__ and set_appearance declare
them (scene/gaussian_model.py:105-142, :199-202, minus .cuda(); the appearance modules are the nn.Embedding that scene/embedding.py:69
wraps).

    python tests/golden/make_decode_options_golden.py

Size: the file stays below neural_gaussians_golden.npz's.  The inputs, the parameters and the upstream gradients keep 4 mantissa bits
(any float32 input is as good as another, and these compress to a third), and half of the anchors are visible; what the reference
computes from them -- outputs and gradients -- is stored as it comes.  Per case the generator asserts min |neural_opacity| >= 5e-5, so that a float32
reordering of the opacity MLP's sums cannot move an offset across the mask.
"""
import os
import types

import numpy as np
import torch
from torch import nn

from make_neural_gaussians_golden import reference_function

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decode_options_golden.npz")
MLPS = ("opacity", "cov", "color", "raydrop")
# tag: N, k, use_feat_bank, appearance_dim, (add_opacity_dist, add_cov_dist, add_color_dist), uid, number of cameras, seed
CASES = {
    "c": (400, 6, False, 32, (True, True, True), 3, 5, 11),
    "d": (300, 5, True, 0, (False, True, False), 0, 1, 12),
    "e": (200, 10, True, 8, (True, False, True), 0, 1, 13),
    "f": (97, 4, True, 32, (True, True, False), 4, 5, 14),
}


def coarse(t):
    """t with 4 mantissa bits kept (round to nearest): still plain float32 values."""
    bits = t.detach().contiguous().view(torch.int32)
    return ((bits + (1 << 18)) & ~((1 << 19) - 1)).view(torch.float32)


def build_pc(N, k, bank, A, flags, cameras, seed):
    g = torch.Generator().manual_seed(seed)
    feat_dim, hidden = 32, 32
    pc = types.SimpleNamespace()
    pc.use_feat_bank, pc.appearance_dim, pc.n_offsets, pc.color_channel = bank, A, k, 2
    pc.add_opacity_dist, pc.add_cov_dist, pc.add_color_dist = flags
    torch.manual_seed(seed)
    mk = lambda din, dout, act: nn.Sequential(nn.Linear(din, hidden), nn.ReLU(True), nn.Linear(hidden, dout), *([act] if act else []))
    if bank:
        pc.mlp_feature_bank = nn.Sequential(nn.Linear(3 + 1, hidden), nn.ReLU(True), nn.Linear(hidden, 3), nn.Softmax(dim=1))
        pc.get_featurebank_mlp = pc.mlp_feature_bank
    pc.mlp_opacity = mk(feat_dim + 3 + int(flags[0]), k, nn.Tanh())
    pc.mlp_cov = mk(feat_dim + 3 + int(flags[1]), 7 * k, None)
    pc.mlp_color = mk(feat_dim + 3 + int(flags[2]) + A, (pc.color_channel - 1) * k, nn.Sigmoid())
    pc.mlp_raydrop = mk(feat_dim + 3 + int(flags[2]) + A, k, nn.Sigmoid())
    pc.get_opacity_mlp, pc.get_cov_mlp, pc.get_color_mlp, pc.get_raydrop_mlp = pc.mlp_opacity, pc.mlp_cov, pc.mlp_color, pc.mlp_raydrop
    if A > 0:
        pc.embedding_appearance, pc.embedding_appearance_rd = nn.Embedding(cameras, A), nn.Embedding(cameras, A)
        pc.get_appearance, pc.get_appearance_rd = pc.embedding_appearance, pc.embedding_appearance_rd
    with torch.no_grad():
        for module in vars(pc).values():
            if isinstance(module, nn.Module):
                for prm in module.parameters():
                    prm.copy_(coarse(prm))
    pc._anchor_feat = coarse(torch.randn(N, feat_dim, generator=g) * 0.5).requires_grad_(True)
    pc._anchor = coarse(torch.randn(N, 3, generator=g) * 10.0).requires_grad_(True)
    pc.get_anchor = pc._anchor
    pc._offset = coarse(torch.randn(N, k, 3, generator=g) * 0.3).requires_grad_(True)
    pc.get_scaling_leaf = coarse(torch.exp(torch.randn(N, 6, generator=g) * 0.3 - 1.0)).requires_grad_(True)     # get_scaling, :213-214
    pc.get_scaling = pc.get_scaling_leaf
    pc.rotation_activation = torch.nn.functional.normalize                           # gaussian_model.py:47
    return pc, g


def run(tag, out):
    N, k, bank, A, flags, uid, cameras, seed = CASES[tag]
    fn = reference_function()
    pc, g = build_pc(N, k, bank, A, flags, cameras, seed)
    cam = types.SimpleNamespace(camera_center=torch.tensor([0.3, -0.2, 1.1]), uid=uid)
    vis = torch.rand(N, generator=g) > 0.5
    xyz, color, opacity, scaling, rot, neural_opacity, mask = fn(cam, pc, vis, is_training=True)
    margin = float(neural_opacity.detach().abs().min())
    assert margin >= 5e-5, f"case {tag}: min |neural_opacity| = {margin:.2e}: change the seed"
    ups = [coarse(torch.randn(t.shape, generator=g)) for t in (xyz, color, opacity, scaling, rot)]
    loss = sum((u * t).sum() for u, t in zip(ups, (xyz, color, opacity, scaling, rot)))
    loss.backward()
    npy = lambda t: t.detach().numpy().astype(np.float32)
    out.update({f"{tag}_N": N, f"{tag}_k": k, f"{tag}_flags": np.array(flags), f"{tag}_bank": bank, f"{tag}_A": A, f"{tag}_uid": uid,
                f"{tag}_cam": npy(cam.camera_center), f"{tag}_vis": vis.numpy(),
                f"{tag}_anchor_feat": npy(pc._anchor_feat), f"{tag}_anchor": npy(pc._anchor), f"{tag}_offset": npy(pc._offset),
                f"{tag}_scaling_in": npy(pc.get_scaling_leaf)})
    mods = [(name, getattr(pc, "mlp_" + name)) for name in MLPS] + ([("bank", pc.mlp_feature_bank)] if bank else [])
    for name, mlp in mods:
        out[f"{tag}_{name}_W1"], out[f"{tag}_{name}_b1"] = npy(mlp[0].weight), npy(mlp[0].bias)
        out[f"{tag}_{name}_W2"], out[f"{tag}_{name}_b2"] = npy(mlp[2].weight), npy(mlp[2].bias)
        out[f"{tag}_g_{name}_W1"], out[f"{tag}_g_{name}_b1"] = npy(mlp[0].weight.grad), npy(mlp[0].bias.grad)
        out[f"{tag}_g_{name}_W2"], out[f"{tag}_g_{name}_b2"] = npy(mlp[2].weight.grad), npy(mlp[2].bias.grad)
    if A > 0:
        out[f"{tag}_emb_color"], out[f"{tag}_emb_raydrop"] = npy(pc.embedding_appearance.weight), npy(pc.embedding_appearance_rd.weight)
        out[f"{tag}_g_emb_color"], out[f"{tag}_g_emb_raydrop"] = npy(pc.embedding_appearance.weight.grad), npy(pc.embedding_appearance_rd.weight.grad)
    for name, t in (("xyz", xyz), ("color", color), ("opacity", opacity), ("scaling", scaling), ("rot", rot), ("neural_opacity", neural_opacity)):
        out[f"{tag}_out_{name}"] = npy(t)
    out[f"{tag}_out_mask"] = mask.numpy()
    for name, u in zip(("xyz", "color", "opacity", "scaling", "rot"), ups):
        out[f"{tag}_up_{name}"] = npy(u)
    out[f"{tag}_g_anchor_feat"], out[f"{tag}_g_anchor"] = npy(pc._anchor_feat.grad), npy(pc._anchor.grad)
    out[f"{tag}_g_offset"], out[f"{tag}_g_scaling"] = npy(pc._offset.grad), npy(pc.get_scaling_leaf.grad)
    print(f"case {tag}: n = {int(vis.sum())} of {N}, M = {int(mask.sum())} of {mask.numel()}, min |neural_opacity| = {margin:.2e}")


if __name__ == "__main__":
    out = {}
    for tag in CASES:
        run(tag, out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
