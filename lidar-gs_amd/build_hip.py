"""Compile the gfx950 rasterizer into an in-tree shared library (no torch involved).

    python lidar-gs_amd/build_hip.py [--force]

Output: lidar-gs_amd/diff_lidargs_rasterization/liblidargs_hip.so  (git-ignored, travels with gpurun)
        lidar-gs_amd/lidargs_optim/liblidargs_optim.so             (the optimizer step: csrc/adam.hip alone, include_optim/)
        lidar-gs_amd/liblidargs_decode_options.so                  (feature bank + appearance in front of the decode: csrc/decode_options.hip alone, include_decode/)
        lidar-gs_amd/tinycudann/liblidargs_tcnn.so                 (the tinycudann stand-in: csrc/raydrop_mlp.hip alone, include_tcnn/)
        lidar-gs_amd/liblidargs_rangeview.so                       (point cloud <-> range image: csrc/range_view.hip alone, include_rangeview/)

Per-file flags: the per-Gaussian kernels (preprocess.hip) are HBM-bound, so they are built with
-ffp-contract=off: every expression rounds as written, which keeps the unit vectors s = p/|p| that
feed the cancellation-prone blend difference (s - q) bit-identical to an un-fused evaluation.
The blend kernels (render.hip) keep FMA contraction.  The sharded path's file (shard.hip) holds kernels of both kinds and says
which is which by `#pragma clang fp contract` in front of each part: a flag would speak for the whole file.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
OUT = os.path.join(HERE, "diff_lidargs_rasterization", "liblidargs_hip.so")
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fno-gpu-rdc", "-Wall",
          "-Wno-unused-function", "-Wno-unused-value"]
SOURCES = {
    "api.hip": [],
    "preprocess.hip": ["-ffp-contract=off"],
    "binning.hip": [],
    "shard.hip": [],   # pragmas, not a flag: its selection and gradient-row kernels round as written (the selection must agree with k_preprocess bit for bit), its image folds fuse
    "render.hip": ["-fno-slp-vectorize"],  # the packed-fp32 pairs are written out (v2f); the SLP vectorizer pairs the rest up at the price of moves
    "neural_gaussians.hip": [],
    "lidar_loss.hip": [],
    "chamfer.hip": ["-ffp-contract=off"],        # the squared distance must round as the reference writes it: the argmin index is compared bit for bit
    "surfel.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],   # ray/plane hit point cancels ~3 digits: round as the reference writes it
    "anchor_growing.hip": ["-ffp-contract=off"],   # anchor + offset * scaling is two roundings in torch: the voxel an offset falls into is compared bit for bit
    "knn.hip": ["-ffp-contract=off"],              # the 3-NN squared distances and the voxel quotients are compared bit for bit; the box bound prunes exactly only without contraction
    "metrics.hip": ["-ffp-contract=off"],          # the SSIM map and the float32 means round as scikit-image / torch write them
}
# The optimizer's library: a target of its own, so that liblidargs_hip.so exports exactly what include/ declares.
OPTIM_OUT = os.path.join(HERE, "lidargs_optim", "liblidargs_optim.so")
OPTIM_INCLUDE = os.path.join(HERE, "..", "include_optim")
OPTIM_SOURCES = {
    "adam.hip": ["-ffp-contract=off"],             # torch's op-by-op roundings; the steps its device kernels fuse are written as fmaf
}
# The decode's two model options (use_feat_bank, appearance_dim > 0): new entry points beside the decode's, a target and a header
# directory of their own like the optimizer's.
DECODE_OUT = os.path.join(HERE, "liblidargs_decode_options.so")
DECODE_INCLUDE = os.path.join(HERE, "..", "include_decode")
DECODE_SOURCES = {
    "decode_options.hip": [],
}
# The tinycudann stand-in (frequency encoding, fused MLP): a target and a header directory of its own, like the two above.
TCNN_OUT = os.path.join(HERE, "tinycudann", "liblidargs_tcnn.so")
TCNN_INCLUDE = os.path.join(HERE, "..", "include_tcnn")
TCNN_SOURCES = {
    "raydrop_mlp.hip": [],
}
# The range-view conversion (point cloud -> range image and back): a target and a header directory of its own, like the three above.
RANGEVIEW_OUT = os.path.join(HERE, "liblidargs_rangeview.so")
RANGEVIEW_INCLUDE = os.path.join(HERE, "..", "include_rangeview")
RANGEVIEW_SOURCES = {
    "range_view.hip": ["-ffp-contract=off"],       # the row and the column of a point are compared pixel for pixel with the reference's float32 evaluation
}
_OWN_TARGET = {**OPTIM_SOURCES, **DECODE_SOURCES, **TCNN_SOURCES, **RANGEVIEW_SOURCES}          # sources that are not part of liblidargs_hip.so


def build_id():
    """A content hash of everything the libraries are built from (csrc/, the public headers of both, this file): the same on every box that holds the
    same sources -- what the profile tools stamp their summaries with and bench.py compares against (the GPU boxes have no .git)."""
    import hashlib
    h = hashlib.sha1()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)) + sorted(
        os.path.join(HERE, "..", "include", f) for f in os.listdir(os.path.join(HERE, "..", "include"))) + sorted(
        os.path.join(OPTIM_INCLUDE, f) for f in os.listdir(OPTIM_INCLUDE)) + sorted(
        os.path.join(DECODE_INCLUDE, f) for f in os.listdir(DECODE_INCLUDE)) + sorted(
        os.path.join(TCNN_INCLUDE, f) for f in os.listdir(TCNN_INCLUDE)) + sorted(
        os.path.join(RANGEVIEW_INCLUDE, f) for f in os.listdir(RANGEVIEW_INCLUDE)) + [os.path.abspath(__file__)]
    for f in files:
        h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:12]


def box_id():
    """The GPU's unique id as rocm-smi prints it (the boxes all call themselves `runc`), or None."""
    try:
        import re
        out = subprocess.run(["rocm-smi", "--showuniqueid"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"Unique ID:\s*(0x[0-9a-fA-F]+|\w+)", out)
        if m:
            return m.group(1)
    except Exception:
        pass
    return None


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def needs_build():
    return _stale(OUT, [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f not in _OWN_TARGET]
                  + [os.path.join(HERE, "..", "include", "lidargs_rasterizer.h"), __file__])


def optim_needs_build():
    return _stale(OPTIM_OUT, [os.path.join(CSRC, f) for f in OPTIM_SOURCES]
                  + [os.path.join(OPTIM_INCLUDE, f) for f in os.listdir(OPTIM_INCLUDE)] + [__file__])


def decode_needs_build():
    return _stale(DECODE_OUT, [os.path.join(CSRC, f) for f in DECODE_SOURCES]
                  + [os.path.join(DECODE_INCLUDE, f) for f in os.listdir(DECODE_INCLUDE)] + [__file__])


def tcnn_needs_build():
    return _stale(TCNN_OUT, [os.path.join(CSRC, f) for f in TCNN_SOURCES]
                  + [os.path.join(TCNN_INCLUDE, f) for f in os.listdir(TCNN_INCLUDE)] + [__file__])


def rangeview_needs_build():
    return _stale(RANGEVIEW_OUT, [os.path.join(CSRC, f) for f in RANGEVIEW_SOURCES]
                  + [os.path.join(RANGEVIEW_INCLUDE, f) for f in os.listdir(RANGEVIEW_INCLUDE)] + [__file__])


def build(force=False, verbose=False):
    """Up-to-date check and build under an exclusive file lock: the ranks of `bench.py --gpus N` (one process per GPU) all call this
    at start-up, and only the first may compile -- the others wait and then find the library up to date.  The link goes to a
    temporary name and is moved into place, so a process that loaded the library earlier never sees a half-written file.
    Builds the five libraries, each when its own dependencies are newer; returns the main library's path."""
    if not force and not needs_build() and not optim_needs_build() and not decode_needs_build() and not tcnn_needs_build() \
            and not rangeview_needs_build():
        return OUT
    import fcntl
    os.makedirs(OBJ, exist_ok=True)
    with open(os.path.join(OBJ, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or needs_build():
                _build_locked(SOURCES, OUT, verbose)
            if force or optim_needs_build():
                _build_locked(OPTIM_SOURCES, OPTIM_OUT, verbose)
            if force or decode_needs_build():
                _build_locked(DECODE_SOURCES, DECODE_OUT, verbose)
            if force or tcnn_needs_build():
                _build_locked(TCNN_SOURCES, TCNN_OUT, verbose)
            if force or rangeview_needs_build():
                _build_locked(RANGEVIEW_SOURCES, RANGEVIEW_OUT, verbose)
            return OUT
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(sources, out, verbose):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra_all = os.environ.get("LIDARGS_EXTRA_HIPCC_FLAGS", "").split()      # instrumented builds of the tools (e.g. -DLG_LANE_STATS), never the product's

    def compile_one(item):
        src, extra = item
        obj = os.path.join(OBJ, src.replace(".hip", ".o"))
        cmd = [hipcc] + COMMON + extra + extra_all + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(compile_one, sources.items()))
    tmp = out + ".tmp.%d" % os.getpid()
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fno-gpu-rdc"] + objs + ["-o", tmp]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(tmp, out)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
