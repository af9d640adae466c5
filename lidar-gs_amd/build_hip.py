"""Compile the gfx950 rasterizer into an in-tree shared library (no torch involved).

    python lidar-gs_amd/build_hip.py [--force]

Output: lidar-gs_amd/diff_lidargs_rasterization/liblidargs_hip.so  (git-ignored, travels with gpurun)

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


def build_id():
    """A content hash of everything the library is built from (csrc/, the public headers, this file): the same on every box that holds the
    same sources -- what the profile tools stamp their summaries with and bench.py compares against (the GPU boxes have no .git)."""
    import hashlib
    h = hashlib.sha1()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)) + sorted(
        os.path.join(HERE, "..", "include", f) for f in os.listdir(os.path.join(HERE, "..", "include"))) + [os.path.abspath(__file__)]
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


def needs_build():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "lidargs_rasterizer.h"), __file__]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """Up-to-date check and build under an exclusive file lock: the ranks of `bench.py --gpus N` (one process per GPU) all call this
    at start-up, and only the first may compile -- the others wait and then find the library up to date.  The link goes to a
    temporary name and is moved into place, so a process that loaded the library earlier never sees a half-written file."""
    if not force and not needs_build():
        return OUT
    import fcntl
    os.makedirs(OBJ, exist_ok=True)
    with open(os.path.join(OBJ, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not needs_build():
                return OUT
            return _build_locked(verbose)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(verbose):
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
        objs = list(ex.map(compile_one, SOURCES.items()))
    tmp = OUT + ".tmp.%d" % os.getpid()
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fno-gpu-rdc"] + objs + ["-o", tmp]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(tmp, OUT)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
