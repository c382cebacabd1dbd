"""Object bounds at the reference's native map shape (sceneObject.get_bound, vmap.py:287-384, for every object before a
checkpoint, train.py:533): 51 objects (the background + 50) x 20 keyframes of 1200 x 680 (synthetic.native_bound_map:
the background in half of every keyframe, each object in 1-5 %).  Reports the keyframe scan against the HBM time of
the bytes it reads, emit + sort + centroids, the host hulls, the search kernel, the whole ops.object_bounds call and
its peak extra device memory.  Prints one JSON line.  Run on the GPU box."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openobj_amd import ops, synthetic  # noqa: E402

HBM_TBPS = 6.3             # measured device copy rate (MI355X_MICROARCH.md)


def main():
    dev = "cuda:0"
    objs = synthetic.native_bound_map(dev)
    torch.cuda.synchronize()
    ops.object_bounds(objs)                                   # warm-up: code objects, the sort's algorithm choice
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        st = {}
        t0 = time.perf_counter()
        res = ops.object_bounds(objs, stats=st)
        torch.cuda.synchronize()
        st["total_ms"] = 1e3 * (time.perf_counter() - t0)
        st["peak_extra_bytes"] = torch.cuda.max_memory_allocated() - base
        runs.append(st)
    t0 = time.perf_counter()
    for _ in range(3):
        ops.object_bounds(objs)
    torch.cuda.synchronize()
    plain_ms = 1e3 * (time.perf_counter() - t0) / 3
    best = min(runs, key=lambda s: s["total_ms"])
    hbm_ms = best["scan_bytes"] / (HBM_TBPS * 1e12) * 1e3
    out = {
        "objects": len(objs), "keyframes": objs[0].n_keyframes, "W": objs[0].frames_width, "H": objs[0].frames_height,
        "points": best["points"], "voxels": best["voxels"], "chunks": best["chunks"],
        "scan_ms": round(best["scan_ms"], 3), "scan_bytes": best["scan_bytes"], "scan_hbm_ms": round(hbm_ms, 3),
        "scan_over_hbm": round(best["scan_ms"] / hbm_ms, 2),
        "emit_sort_centroids_ms": round(best["centroid_ms"], 3),
        "voxels_call_ms": round(1e3 * best["voxels_s"], 2), "host_hull_ms": round(1e3 * best["hull_s"], 2),
        "search_kernel_ms": round(best["search_ms"], 3), "search_call_ms": round(1e3 * best["search_s"], 2),
        "object_bounds_ms": round(best["total_ms"], 2), "object_bounds_ms_no_stats": round(plain_ms, 2),
        "peak_extra_MiB": round(max(s["peak_extra_bytes"] for s in runs) / 2 ** 20, 1),
        "hull_vertices_max": int(max(best["hull_vertices"])), "candidates_max": int(max(best["candidates"])),
        "boxes": sum(b is not None for _, b in res),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
