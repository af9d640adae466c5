"""Device time of the tinycudann stand-in on the reference's ray-drop refinement network -- two Frequency encodings (3 and 2 inputs,
12 frequencies), torch.cat, a 120 -> 128 x 4 -> 1 ReLU / Sigmoid MLP -- forward alone and forward + backward (MSE against a 0/1 target,
as scene/extre_train_raydrop.py trains), beside the same model as framework ops on the same box (torch.sin / torch.cat, F.linear, relu,
sigmoid, autograd: tests/tcnn_ref.py in float32).
    python tools/time_tcnn.py [--rows 169600,67980] [--iters I] [--native-only] [--json FILE]
169 600 rows are one 64 x 2650 frame, 67 980 one 66 x 1030 KITTI frame.  Times are device events around `iters` calls, three
interleaved passes per leg, medians reported; the MLP alone (encoded features given) is timed too, with the algorithmic FLOPs of its
matrix products (2 * rows * parameters forward, three times that forward + backward) over its time.  No number here is a pass
criterion."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lidar-gs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import warnings
import torch
import torch.nn.functional as F_
import build_hip
import tcnn_ref as ref
import tinycudann as tcnn

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="169600,67980")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--native-only", action="store_true")
ap.add_argument("--json", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"
DEV = "cuda:0"
H, N_OUT = 4, 1

with warnings.catch_warnings():
    warnings.simplefilter("ignore")                    # the reference's "degree" keys
    enc_dir = tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "Frequency", "degree": 4}).cuda()
    enc_i_d = tcnn.Encoding(n_input_dims=2, encoding_config={"otype": "Frequency", "degree": 6}).cuda()
unet = tcnn.Network(n_input_dims=enc_dir.n_output_dims + enc_i_d.n_output_dims, n_output_dims=N_OUT, network_config={
    "otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": 128, "n_hidden_layers": H}).cuda()
params_fw = unet.params.detach().clone().requires_grad_()


def make(rows):
    g = torch.Generator().manual_seed(rows)
    dirs = F_.normalize(torch.randn(rows, 3, generator=g), dim=1).to(DEV)
    i_d = torch.cat((torch.rand(rows, 1, generator=g), torch.rand(rows, 1, generator=g) * 80), dim=1).to(DEV)
    target = (torch.rand(rows, 1, generator=g) < 0.5).float().to(DEV)
    feats = torch.cat((enc_dir(dirs), enc_i_d(i_d)), dim=1)
    native = lambda: unet(torch.cat((enc_dir(dirs), enc_i_d(i_d)), dim=1))
    framework = lambda: ref.mlp(torch.cat((ref.encode(dirs, 12, dtype=torch.float32), ref.encode(i_d, 12, dtype=torch.float32)), dim=1),
                                params_fw, H, N_OUT, True, dtype=torch.float32)
    return dict(native=native, framework=framework, native_mlp=lambda: unet(feats),
                framework_mlp=lambda: ref.mlp(feats, params_fw, H, N_OUT, True, dtype=torch.float32)), target


def run(fn, target, backward):
    unet.params.grad = None
    params_fw.grad = None
    if not backward:
        with torch.no_grad():
            return fn()
    F_.mse_loss(fn(), target).backward()


def timeit(fn, target, backward):
    for _ in range(3):
        run(fn, target, backward)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(a.iters):
        run(fn, target, backward)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / a.iters


res = dict(device=torch.cuda.get_device_name(0), box=build_hip.box_id(), build=build_hip.build_id(), iters=a.iters,
           model=f"Frequency(3, F=12) + Frequency(2, F=12) -> {unet.n_input_dims} -> 128 x {H} -> {N_OUT}, ReLU, Sigmoid, float32",
           forward_row_tile=tcnn.FORWARD_ROW_TILE, backward_row_tile=tcnn.BACKWARD_ROW_TILE, rows=[])
for rows in (int(r) for r in a.rows.split(",")):
    legs, target = make(rows)
    if a.native_only:
        legs = {k: v for k, v in legs.items() if k.startswith("native")}
    times = {(k, b): [] for k in legs for b in (False, True)}
    for _ in range(3):                                     # interleaved: every leg sees the same box state
        for (k, b) in times:
            times[(k, b)].append(timeit(legs[k], target, b))
    flops = 2 * rows * unet.params.numel()
    row = dict(rows=rows, backward_blocks=tcnn._lib.lidargs_tcnn_backward_blocks(rows), mlp_forward_gflop=round(flops / 1e9, 3))
    for (k, b), ts in times.items():
        row[f"{k}_{'forward_backward' if b else 'forward'}_ms"] = round(statistics.median(ts), 4)
        row[f"{k}_{'forward_backward' if b else 'forward'}_all"] = [round(t, 4) for t in ts]
    for b, mult in ((False, 1), (True, 3)):
        t = row[f"native_mlp_{'forward_backward' if b else 'forward'}_ms"]
        row[f"native_mlp_{'forward_backward' if b else 'forward'}_tflops"] = round(mult * flops / (t * 1e-3) / 1e12, 2)
    res["rows"].append(row)
    for b in (False, True):
        what = "forward+backward" if b else "forward         "
        key = "forward_backward" if b else "forward"
        line = f"rows {rows:7d} {what}: native {row[f'native_{key}_ms']:.3f} ms (MLP alone {row[f'native_mlp_{key}_ms']:.3f} ms, {row[f'native_mlp_{key}_tflops']:.1f} TFLOP/s)"
        if not a.native_only:
            line += f" vs framework ops {row[f'framework_{key}_ms']:.3f} ms (MLP alone {row[f'framework_mlp_{key}_ms']:.3f} ms)"
        print(line)
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
