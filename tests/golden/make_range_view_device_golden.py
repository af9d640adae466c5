"""Generate tests/golden/range_view_device_golden.npz by EXECUTING the reference's own numpy range-view code on margin-masked points.

Run where a checkout of the reference is at hand; its path is the argument:

    python tests/golden/make_range_view_device_golden.py REFERENCE_ROOT

As make_rangeview_golden.py does, the pure numpy functions are pulled out of utils/lidar_utils.py's AST at generation time and exec'd in a
scratch namespace (the module itself cannot be imported).  Nothing of the reference's source text is written to this repository: the .npz
holds inputs and outputs only.  Made under NumPy >= 2 (float32 scalars stay float32 against Python numbers).

What differs from rangeview_golden.npz: the points went through tests/range_view_ref.decision_margin_mask, so that their pixel does not
depend on the last bits of atan2 -- these outputs are what a float32 device evaluation must reproduce EXACTLY.

Cases (tag -> beam table, H x W): u16 / w16 / n16 uniform / waymo / neartie at 16 x 512, u64 / w64 / n64 at 64 x 2650, fov = fov mode
lidar_K = (2.0, 26.9) at 16 x 500.  Per case: points, pano, intensities, back (the reference's back-projection of that image),
dirs (its unit rays, pano_to_lidar of a constant-1 image; kept for w16 and fov).
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "lidar-gs_amd"))
sys.path.insert(0, os.path.join(HERE, ".."))
import lidargs_scenes as sc  # noqa: E402
import range_view_ref as ref  # noqa: E402

REF = os.path.join(sys.argv[1], "utils", "lidar_utils.py") if len(sys.argv) > 1 else None
WANTED = ["find_closest_label", "lidar_to_pano_with_intensities", "pano_to_lidar_with_intensities", "pano_to_lidar", "get_beam_inclinations"]
CASES = {"u16": ("uniform", 16, 512, 1200, 21), "w16": ("waymo", 16, 512, 1200, 22), "n16": ("neartie", 16, 512, 1200, 23),
         "u64": ("uniform", 64, 2650, 1200, 24), "w64": ("waymo", 64, 2650, 1200, 25), "n64": ("neartie", 64, 2650, 1200, 26),
         "fov": (None, 16, 500, 1200, 27)}
LIDAR_K = (2.0, 26.9)
DIRS_OF = ("w16", "fov")          # the ray tables kept (the 64 x 2650 ones would be megabytes)


def load_reference_functions():
    assert REF is not None, "usage: make_range_view_device_golden.py REFERENCE_ROOT"
    tree = ast.parse(open(REF).read(), REF)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in body) == sorted(WANTED), [n.name for n in body]
    ns = {"np": np}
    exec(compile(ast.Module(body=body, type_ignores=[]), REF, "exec"), ns)
    return ns


def main():
    assert int(np.__version__.split(".")[0]) >= 2, np.__version__
    ns = load_reference_functions()
    out = {"numpy_version": np.__version__, "lidar_K": np.array(LIDAR_K)}
    for tag, (kind, H, W, N, seed) in CASES.items():
        rng = np.random.default_rng(seed)
        beams = None if kind is None else np.ascontiguousarray(sc.beam_table(H, kind))
        rows = dict(beam_inclinations=beams) if beams is not None else dict(lidar_K=LIDAR_K)
        pts = ref.masked_points(rng, N, H, W, beams, None if beams is not None else LIDAR_K)
        pano, inten = ns["lidar_to_pano_with_intensities"](pts, H, W, max_depth=80, **rows)
        back = ns["pano_to_lidar_with_intensities"](pano, inten, **rows)
        dirs = ns["pano_to_lidar"](np.ones((H, W)), **rows)
        out.update({f"{tag}_H": H, f"{tag}_W": W, f"{tag}_points": pts, f"{tag}_pano": pano.astype(np.float32), f"{tag}_intensities": inten.astype(np.float32),
                    f"{tag}_back": back})
        if tag in DIRS_OF:
            assert np.array_equal(dirs.astype(np.float32), dirs)                 # (the reference's rays are float32 values: i, j and the tables are)
            out[f"{tag}_dirs"] = dirs.astype(np.float32).reshape(H, W, 3)
        assert np.array_equal(pano.astype(np.float32), pano) and np.array_equal(inten.astype(np.float32), inten)   # (float32 values held in float64)
        if beams is not None:
            out[f"{tag}_beams"] = beams
    dst = os.path.join(HERE, "range_view_device_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
