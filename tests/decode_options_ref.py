"""The anchor decode WITH the two model options -- the feature bank and the per-camera appearance embedding -- restated in torch
(gaussian_renderer/__init__.py:17-119, every branch), forward and autograd backward, in float64 unless another dtype is asked for.
TEST INFRASTRUCTURE ONLY: the expectation for shapes the fixture (tests/golden/decode_options_golden.npz) lacks, and itself pinned
against that fixture by tests/test_decode_options_cpu.py.

A model is a dict of numpy arrays as lidargs_scenes.make_anchor_model draws it (anchor_feat, anchor, offset, scaling,
{opacity,cov,color,raydrop}_{W1,b1,W2,b2}, add_*_dist) plus, optionally,
    bank_W1 [32,4], bank_b1 [32], bank_W2 [3,32], bank_b2 [3]        use_feat_bank=True
    emb_color [num,A], emb_raydrop [num,A]                            appearance_dim = A (color_W1 and raydrop_W1 are [32, din + A])
"""
import numpy as np
import torch
import torch.nn.functional as F

MLPS = ("opacity", "cov", "color", "raydrop")
TENSOR_KEYS = ("anchor_feat", "anchor", "offset", "scaling")
OUT_KEYS = ("xyz", "color", "opacity", "scaling", "rot", "neural_opacity")


def param_keys(p):
    keys = [f"{m}_{q}" for m in MLPS + (("bank",) if "bank_W1" in p else ()) for q in ("W1", "b1", "W2", "b2")]
    return keys + (["emb_color", "emb_raydrop"] if "emb_color" in p else [])


def mlp(x, W1, b1, W2, b2, act):
    y = F.linear(F.relu(F.linear(x, W1, b1)), W2, b2)
    return act(y) if act is not None else y


def generate(T, cam, visible_mask, flags, uid=0):
    """T: dict name -> tensor (the model's arrays, see the module docstring); returns the 7-tuple of the training path."""
    anchor = T["anchor"]
    if visible_mask is None:
        visible_mask = torch.ones(anchor.shape[0], dtype=torch.bool, device=anchor.device)
    feat, anc, offs, scal = T["anchor_feat"][visible_mask], anchor[visible_mask], T["offset"][visible_mask], T["scaling"][visible_mask]   # :22-25
    n, k = anc.shape[0], offs.shape[1]
    ob = anc - cam                                                        # :28
    dist = ob.norm(dim=1, keepdim=True)                                   # :32
    view = ob / dist                                                      # :34
    if "bank_W1" in T:                                                    # :37-47
        w = mlp(torch.cat([view, dist], dim=1), *(T["bank_" + q] for q in ("W1", "b1", "W2", "b2")), lambda z: torch.softmax(z, dim=1))
        feat = feat[:, ::4].repeat(1, 4) * w[:, 0:1] + feat[:, ::2].repeat(1, 2) * w[:, 1:2] + feat * w[:, 2:3]
    x_d = torch.cat([feat, view, dist], dim=1)                            # :50
    x_nd = torch.cat([feat, view], dim=1)                                 # :51
    pick = lambda f: x_d if f else x_nd
    P = lambda m: tuple(T[f"{m}_{q}"] for q in ("W1", "b1", "W2", "b2"))
    neural_opacity = mlp(pick(flags[0]), *P("opacity"), torch.tanh).reshape(-1, 1)          # :60-66
    mask = (neural_opacity > 0.0).view(-1)                                # :67-68
    opacity = neural_opacity[mask]                                        # :71
    x_color = x_raydrop = pick(flags[2])
    if "emb_color" in T:                                                  # :52-56, :73-79: every row takes the camera's embedding row
        idx = torch.full((n,), int(uid), dtype=torch.long, device=anchor.device)
        x_color = torch.cat([x_color, F.embedding(idx, T["emb_color"])], dim=1)
        x_raydrop = torch.cat([x_raydrop, F.embedding(idx, T["emb_raydrop"])], dim=1)
    color = mlp(x_color, *P("color"), torch.sigmoid).reshape(n * k, 1)     # :76-85
    raydrop = mlp(x_raydrop, *P("raydrop"), torch.sigmoid).reshape(n * k, 1)
    color = torch.cat([color, raydrop], dim=1)                            # :87
    scale_rot = mlp(pick(flags[1]), *P("cov"), None).reshape(n * k, 7)     # :90-94
    offsets = offs.reshape(-1, 3)                                         # :97
    rep = torch.cat([scal, anc], dim=-1).repeat_interleave(k, dim=0)      # :100-101
    masked = torch.cat([rep, color, scale_rot, offsets], dim=-1)[mask]    # :102-103
    scaling_repeat, repeat_anchor, color, scale_rot, offsets = masked.split([6, 3, 2, 7, 3], dim=-1)
    scaling_out = scaling_repeat[:, 3:] * torch.sigmoid(scale_rot[:, :3])  # :107
    rot = F.normalize(scale_rot[:, 3:7])                                  # :108
    xyz = repeat_anchor + offsets * scaling_repeat[:, :3]                 # :111-112
    return xyz, color, opacity, scaling_out, rot, neural_opacity, mask


def flags_of(p):
    return (bool(p["add_opacity_dist"]), bool(p["add_cov_dist"]), bool(p["add_color_dist"]))


def run(p, cam, vis, uid=0, ups=None, dtype=torch.float64):
    """Forward, and backward when `ups` is given: the five upstream gradients (xyz, color, opacity, scaling, rot), or a callable
    M -> those five (the number of selected pairs is only known after the forward).  Returns a dict of numpy arrays: the outputs
    under their names, `mask`, `ups`, and the gradients under g_<name> for every tensor and parameter of the model."""
    leaf = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
    T = {name: leaf(p[name]) for name in TENSOR_KEYS + tuple(param_keys(p))}
    visible = None if vis is None else torch.from_numpy(np.asarray(vis, bool))
    outs = generate(T, torch.from_numpy(np.asarray(cam)).to(dtype), visible, flags_of(p), uid)
    res = {name: o.detach().numpy() for name, o in zip(OUT_KEYS, outs)}
    res["mask"] = outs[6].numpy()
    if ups is not None:
        if callable(ups):
            ups = ups(int(outs[0].shape[0]))
        res["ups"] = [np.asarray(u, np.float32) for u in ups]
        sum((o * torch.from_numpy(u).to(dtype)).sum() for o, u in zip(outs[:5], res["ups"])).backward()
        for name, t in T.items():
            res["g_" + name] = (t.grad if t.grad is not None else torch.zeros_like(t)).numpy()
    return res


def random_options(p, seed, bank=True, A=0, cameras=3):
    """`p` (a model of lidargs_scenes.make_anchor_model) with a feature bank and / or an appearance embedding of width A added."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    q = dict(p)
    if bank:
        q["bank_W1"], q["bank_b1"] = f(32, 4) / np.float32(2.0), 0.1 * f(32)
        q["bank_W2"], q["bank_b2"] = f(3, 32) / np.float32(5.6), 0.1 * f(3)
        q["bank_W1"][:, 3] /= np.float32(10.0)                              # the distance input is ~10x the view components
    if A > 0:
        q["emb_color"], q["emb_raydrop"] = f(cameras, A), f(cameras, A)
        for m in ("color", "raydrop"):
            q[m + "_W1"] = np.concatenate([p[m + "_W1"], f(32, A) / np.float32(6.0)], axis=1)
    return q


def load_case(tag, path=None):
    """A case of the fixture: (model dict, cam, vis, uid, expectations) -- `exp` holds out_*, up_* and g_* as the reference gave them."""
    import os
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_options_golden.npz")
    z = np.load(path)
    flags = z[f"{tag}_flags"]
    p = dict(add_opacity_dist=bool(flags[0]), add_cov_dist=bool(flags[1]), add_color_dist=bool(flags[2]), scaling=z[f"{tag}_scaling_in"])
    for name in ("anchor_feat", "anchor", "offset"):
        p[name] = z[f"{tag}_{name}"]
    names = [f"{m}_{q}" for m in MLPS + (("bank",) if bool(z[f"{tag}_bank"]) else ()) for q in ("W1", "b1", "W2", "b2")]
    names += ["emb_color", "emb_raydrop"] if int(z[f"{tag}_A"]) > 0 else []
    for name in names:
        p[name] = z[f"{tag}_{name}"]
    exp = {key[len(tag) + 1:]: z[key] for key in z.files if key.startswith((tag + "_out_", tag + "_g_", tag + "_up_"))}
    return p, z[f"{tag}_cam"], z[f"{tag}_vis"], int(z[f"{tag}_uid"]), exp


def to_torch_model(p, device="cuda"):
    """The `pc` generate_neural_gaussians reads, for a model dict with options: lidargs_scenes.anchor_model_to_torch plus the
    feature-bank MLP and the two appearance modules declared as GaussianModel declares them (scene/gaussian_model.py:105-111, :199-202)."""
    import lidargs_scenes as sc
    from torch import nn
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    pc = sc.anchor_model_to_torch(p, device)
    if "bank_W1" in p:
        seq = nn.Sequential(nn.Linear(4, 32), nn.ReLU(True), nn.Linear(32, 3), nn.Softmax(dim=1)).to(device)
        with torch.no_grad():
            seq[0].weight.copy_(t(p["bank_W1"])); seq[0].bias.copy_(t(p["bank_b1"])); seq[2].weight.copy_(t(p["bank_W2"])); seq[2].bias.copy_(t(p["bank_b2"]))
        pc.use_feat_bank, pc.mlp_feature_bank, pc.get_featurebank_mlp = True, seq, seq
    if "emb_color" in p:
        pc.appearance_dim = int(p["emb_color"].shape[1])
        for attr, key in (("get_appearance", "emb_color"), ("get_appearance_rd", "emb_raydrop")):
            emb = nn.Embedding(*p[key].shape).to(device)
            with torch.no_grad():
                emb.weight.copy_(t(p[key]))
            setattr(pc, attr, emb)
    return pc


def model_grads(pc):
    """{g_<name>: numpy} of every tensor and parameter of a `pc` after a backward, under the names of `run`."""
    g = lambda t: t.grad.detach().cpu().numpy()
    res = dict(g_anchor_feat=g(pc._anchor_feat), g_anchor=g(pc._anchor), g_offset=g(pc._offset), g_scaling=g(pc.get_scaling))
    seqs = [(m, getattr(pc, "mlp_" + m)) for m in MLPS] + ([("bank", pc.mlp_feature_bank)] if getattr(pc, "use_feat_bank", False) else [])
    for m, seq in seqs:
        res[f"g_{m}_W1"], res[f"g_{m}_b1"], res[f"g_{m}_W2"], res[f"g_{m}_b2"] = g(seq[0].weight), g(seq[0].bias), g(seq[2].weight), g(seq[2].bias)
    if getattr(pc, "appearance_dim", 0) > 0:
        res["g_emb_color"], res["g_emb_raydrop"] = g(pc.get_appearance.weight), g(pc.get_appearance_rd.weight)
    return res
