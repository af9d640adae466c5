"""Compile the gfx950 libraries into in-tree shared libraries (no torch involved).

    python lidar-gs_amd/build_hip.py [--force]

TARGETS below is the one description of what is built: per library its name, its output (git-ignored), its sources with their per-file
flags, and the directory of the public headers that declare exactly what it exports.  `hip` is the main library (the rasterizers and
everything include/ declares); every other entry is a single source with a header directory of its own, so that liblidargs_hip.so
exports exactly what include/ declares.  Staleness (stale, deps), the build loop (build) and the content hash (build_id, build_id_files)
are all derived from the table, and so is what the Python side loads (lidargs_abi.library takes a library's path, headers, version
function and the name in its error messages from its entry): a further library is one more entry.

A target's `include` and `prefix` are its primary, versioned interface (<prefix>_abi_version, <prefix>_last_error); `families` names what
else the library exports: per family a header directory and a symbol prefix of its own.  Only `hip` has any.  Its pose-gradient entry
points (`pose`: the 3-D rasterizer's, `surfel_pose`: the surfel rasterizer's, kept apart so that include_pose/ stays the 3-D form's
three functions) run lidargs_backward's and lidargs_surfel_backward's host sequences and share the process-wide state, and sweep-motion
compensation (`sweep`, csrc/sweep_motion.hip: a warp of the means in front of either rasterizer) reports through lidargs_last_error and
every .hip of csrc/ belongs to a target: so all three are part of liblidargs_hip.so and not libraries of their own, while include/ and the
library's lidargs_* exports stay the drop-in boundary for the reference's interfaces.  A family's headers are rebuilt for, hashed and
typed exactly as the primary ones are (header_dirs); a further family is one more record in the `hip` entry, one header, and one line of
tests/native_lib_checks.FAMILIES.

Per-file flags: the per-Gaussian kernels (preprocess.hip) are HBM-bound, so they are built with
-ffp-contract=off: every expression rounds as written, which keeps the unit vectors s = p/|p| that
feed the cancellation-prone blend difference (s - q) bit-identical to an un-fused evaluation.
The blend kernels (render.hip) keep FMA contraction.  The sharded path's file (shard.hip) holds kernels of both kinds and says
which is which by `#pragma clang fp contract` in front of each part: a flag would speak for the whole file.
"""
import collections
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
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
    "sweep_motion.hip": ["-ffp-contract=on"],      # fused only inside an expression: the backward's two forms (with and without the reduced gradients) round dL_dmeans3D alike
}
# sources: {file of csrc/: [per-file flags]}; include: its header directory; prefix: of its symbols (<prefix>_abi_version, <prefix>_last_error,
# the macro <PREFIX>_ABI_VERSION); package: the importer that the loader's error messages name (lidargs_abi.library); families: further
# (name, header directory, symbol prefix) records of entry points that the same library exports (the docstring says which and why)
Family = collections.namedtuple("Family", "name include prefix")
Target = collections.namedtuple("Target", "name out sources include prefix package families", defaults=((),))
TARGETS = {t.name: t for t in (
    Target("hip", OUT, SOURCES, os.path.join(ROOT, "include"), "lidargs", "diff_lidargs_rasterization", (
        Family("pose", os.path.join(ROOT, "include_pose"), "lgpose"),
        Family("surfel_pose", os.path.join(ROOT, "include_surfel_pose"), "lgsfpose"),
        Family("sweep", os.path.join(ROOT, "include_sweep"), "lgsweep"))),
    Target("optim", os.path.join(HERE, "lidargs_optim", "liblidargs_optim.so"), {
        "adam.hip": ["-ffp-contract=off"],         # torch's op-by-op roundings; the steps its device kernels fuse are written as fmaf
    }, os.path.join(ROOT, "include_optim"), "lidargs_optim", "lidargs_optim"),
    # the decode's two model options (use_feat_bank, appearance_dim > 0): entry points beside the decode's
    Target("decode_options", os.path.join(HERE, "liblidargs_decode_options.so"), {
        "decode_options.hip": [],
    }, os.path.join(ROOT, "include_decode"), "lidargs_ng_options", "neural_gaussians"),
    # the tinycudann stand-in (frequency encoding, fused MLP)
    Target("tcnn", os.path.join(HERE, "tinycudann", "liblidargs_tcnn.so"), {
        "raydrop_mlp.hip": [],
    }, os.path.join(ROOT, "include_tcnn"), "lidargs_tcnn", "tinycudann"),
    # the range-view conversion (point cloud -> range image and back)
    Target("rangeview", os.path.join(HERE, "liblidargs_rangeview.so"), {
        "range_view.hip": ["-ffp-contract=off"],   # the row and the column of a point are compared pixel for pixel with the reference's float32 evaluation
    }, os.path.join(ROOT, "include_rangeview"), "lidargs_rv", "range_view"),
    # the torch_scatter stand-in (scatter_max / scatter_min with the winning position)
    Target("scatter", os.path.join(HERE, "torch_scatter", "liblidargs_scatter.so"), {
        "scatter.hip": [],
    }, os.path.join(ROOT, "include_scatter"), "lidargs_scatter", "torch_scatter"),
)}


def all_targets():
    return list(TARGETS.values())


def _listed(d, keep=lambda f: True):
    return sorted(os.path.join(d, f) for f in os.listdir(d) if keep(f))


def header_dirs(target):
    """Every header directory of a target: the primary one first, then its families' in the table's order."""
    return [target.include] + [f.include for f in target.families]


def deps(target):
    """What a library is rebuilt for: its own sources, every shared file of csrc/ that is not a .hip (headers and .inc, whichever
    target includes them: more than needed, never less), every header of its header directories and this file."""
    return ([os.path.join(CSRC, f) for f in target.sources] + _listed(CSRC, lambda f: not f.endswith(".hip"))
            + [h for d in header_dirs(target) for h in _listed(d)] + [os.path.abspath(__file__)])


def stale(target):
    if not os.path.exists(target.out):
        return True
    t = os.path.getmtime(target.out)
    return any(os.path.getmtime(d) > t for d in deps(target))


def build_id_files():
    """Everything the libraries are built from: csrc/, every target's public headers (header_dirs), this file."""
    return _listed(CSRC) + [h for t in TARGETS.values() for d in header_dirs(t) for h in _listed(d)] + [os.path.abspath(__file__)]


def build_id():
    """A content hash of build_id_files() (name, then contents): the same on every box that holds the same sources -- what the
    profile tools stamp their summaries with and bench.py compares against (the GPU boxes have no .git)."""
    import hashlib
    h = hashlib.sha1()
    for f in build_id_files():
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


def build(force=False, verbose=False):
    """Up-to-date check and build under an exclusive file lock: the ranks of `bench.py --gpus N` (one process per GPU) all call this
    at start-up, and only the first may compile -- the others wait and then find the library up to date.  The link goes to a
    temporary name and is moved into place, so a process that loaded the library earlier never sees a half-written file.
    Builds every library of TARGETS that is stale; returns the main library's path."""
    if not force and not any(stale(t) for t in all_targets()):
        return OUT
    import fcntl
    os.makedirs(OBJ, exist_ok=True)
    with open(os.path.join(OBJ, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            for t in all_targets():
                if force or stale(t):
                    _build_locked(t, verbose)
            return OUT
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(target, verbose):
    sources, out = target.sources, target.out
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
