"""Mask-graph timings (objnerf_maskgraph.hip) -> profiles/maskgraph_bench.json.

    python tools/maskgraph_bench.py [--out profiles/maskgraph_bench.json] [--reps 5]

At the native shape, 200 frames of 1200 x 680 with 30 masks each (N = 6 000 masks):
- the segmented DBSCAN in points per second on one frame's mask clouds (30 planar patches of 816 000 / 30 pixels, eps
  0.05, min_points 100), against scikit-learn's DBSCAN with 16 threads on the first 3 of those clouds where it is
  installed, else against the numpy / scipy restatement of tests/maskgraph_util.py (the record says which);
- the affinity pass (the whole call: norms, W, edge counts) in ms and as a share of the 157 TF fp32 MFMA peak
  (2 N^2 (384 + 512 + 96) flop); the peak of objnerf_mfma_peak's loop on the device is recorded beside it;
- the 2-D term as the difference of the pass with and without it (not a timing of its own);
- the ray / box pass on 20 of the 200 frames (it is linear in the frames);
- the cloud overlap of 30 clouds of 20 000 points against scipy.spatial.cKDTree.
No speed target: the record is the deliverable."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from openobj_amd import ops  # noqa: E402

F32_MFMA = 157.3e12
FRAMES, W_IMG, H_IMG, MASKS = 200, 1200, 680, 30


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def measured_mfma_peak(dev):
    """flop/s of objnerf_mfma_peak's saturated fp32 MFMA loop on this device (as bench.py --full measures it)."""
    from openobj_amd import _lib
    n_wg, iters = 1024, 10000
    sink = torch.empty(n_wg * 256, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for it in (2000, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(_lib.lib().objnerf_mfma_peak(0, it, n_wg, sink.data_ptr(), st), "objnerf_mfma_peak")
        e1.record()
        torch.cuda.synchronize()
    return 4096.0 * 4 * iters * 4 * n_wg / (e0.elapsed_time(e1) * 1e-3)


def mask_clouds(rs):
    """One frame's clouds: 30 patches of a 1200 x 680 image at 600 px focal length, 1.5 .. 4 m away, with 2 % of the
    pixels 0.5 m behind the surface (what the DBSCAN removes)."""
    n = W_IMG * H_IMG // MASKS
    side = int(np.sqrt(n))
    clouds = []
    for k in range(MASKS):
        v, u = np.mgrid[0:side, 0:side]
        z = rs.uniform(1.5, 4.0) + 0.001 * u + 0.0005 * v + rs.normal(0, 0.002, u.shape)
        z[rs.rand(*z.shape) < 0.02] += 0.5
        p = np.stack([(u - side / 2) * z / 600.0, (v - side / 2) * z / 600.0, z], -1).reshape(-1, 3)
        clouds.append(p + [3.0 * k, 0.0, 0.0])
    return clouds


def bench_dbscan(rs, reps):
    clouds = mask_clouds(rs)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    r = {"clouds": len(clouds), "points": int(off[-1]), "eps": 0.05, "min_points": 100}
    r["plan_s"] = timed(lambda: ops.DbscanPlan(pts, off, 0.05), reps)
    plan = ops.DbscanPlan(pts, off, 0.05)
    r["run_s"] = timed(lambda: plan.run(100), reps)
    r["points_per_s"] = r["points"] / (r["plan_s"] + r["run_s"])
    labels = plan.run(100).cpu().numpy()
    sub = 3                                               # the CPU side on the first clouds only: it is slow
    n_sub = int(off[sub])
    try:
        from sklearn.cluster import DBSCAN
        t = time.perf_counter()
        want = np.concatenate([DBSCAN(eps=0.05, min_samples=100, n_jobs=16).fit_predict(c) for c in clouds[:sub]])
        r["baseline"] = "sklearn.cluster.DBSCAN, n_jobs=16"
    except ImportError:
        import maskgraph_util as U
        t = time.perf_counter()
        want = np.concatenate([U.dbscan_labels(c, 0.05, 100) for c in clouds[:sub]])
        r["baseline"] = "numpy / scipy restatement (tests/maskgraph_util.py)"
    r["baseline_s"] = time.perf_counter() - t
    r["baseline_points"] = n_sub
    r["baseline_points_per_s"] = n_sub / r["baseline_s"]
    r["labels_equal_baseline"] = bool(np.array_equal(labels[:n_sub], want))
    r["noise_fraction"] = float((labels == -1).mean())
    return r


def bench_affinity(rs, reps):
    N, dc, dl = FRAMES * MASKS, 384, 512
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    cap = torch.randn(N, dc, device=dev, generator=g)
    clip = torch.randn(N, dl, device=dev, generator=g)
    color = torch.rand(N, 96, device=dev, generator=g) * 100
    lo = rs.uniform(-3, 3, (N, 3))
    boxes = torch.from_numpy(np.concatenate([lo, lo + rs.uniform(0.2, 2.0, (N, 3))], 1)).to(dev)
    c0 = rs.randint(0, 60, (FRAMES, N, 2))
    b2 = torch.from_numpy(np.concatenate([c0, c0 + rs.randint(1, 50, (FRAMES, N, 2))], 2).astype(np.int32)).to(dev)
    r = {"N": N, "d_cap": dc, "d_clip": dl, "F": FRAMES}
    w = (0.3, 0.3, 0.3, 0.2, 0.0)
    t = timed(lambda: ops.mask_affinity(boxes, cap, clip, color, None, w), reps)
    r["affinity_no2d_ms"] = t * 1e3
    r["affinity_no2d_mfma_fraction"] = 2.0 * N * N * (dc + dl + 96) / t / F32_MFMA
    t = timed(lambda: ops.mask_affinity(boxes, cap, clip, color, b2, w[:4] + (0.2,)), max(1, reps // 2))
    r["affinity_ms"] = t * 1e3
    r["affinity_mfma_fraction"] = 2.0 * N * N * (dc + dl + 96) / t / F32_MFMA
    r["geo2d_term_ms_by_difference"] = r["affinity_ms"] - r["affinity_no2d_ms"]      # not a timing of its own
    r["fp32_mfma_peak_flops"] = F32_MFMA
    r["fp32_mfma_peak_measured_flops"] = measured_mfma_peak(dev)
    for k in ("affinity_no2d", "affinity"):
        r[k + "_share_of_measured_peak"] = r[k + "_mfma_fraction"] * F32_MFMA / r["fp32_mfma_peak_measured_flops"]
    return r


def bench_ray_boxes(rs, reps):
    N = FRAMES * MASKS
    dev = torch.device("cuda")
    F = 20                                                # a tenth of the frames; the pass is linear in F
    depth = torch.from_numpy(rs.randint(500, 5000, (F, H_IMG, W_IMG)).astype(np.uint16).view(np.int16)).to(dev)
    twc = torch.eye(4, dtype=torch.float64, device=dev).repeat(F, 1, 1)
    lo = rs.uniform(-3, 3, (N, 3))
    boxes = torch.from_numpy(np.concatenate([lo, lo + rs.uniform(0.2, 2.0, (N, 3))], 1)).to(dev)
    t = timed(lambda: ops.mask_ray_boxes(depth, twc, boxes, 600.0, 600.0, 599.5, 339.5), reps)
    tests = F * N * (W_IMG // 10) * (H_IMG // 10)
    return {"N": N, "frames_timed": F, "ms": t * 1e3, "ray_box_tests_per_s": tests / t,
            "ms_at_200_frames": t * 1e3 * FRAMES / F}


def bench_overlap(rs, reps):
    from scipy.spatial import cKDTree
    C, n = 30, 20000
    clouds = [rs.uniform(0, 1, (n, 3)) * [1.5, 1.5, 0.3] + [0.6 * (k % 6), 0.6 * (k // 6), 0.0] for k in range(C)]
    off = np.arange(C + 1) * n
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    r = {"C": C, "points_per_cloud": n, "dis_thre": 0.02}
    r["gpu_s"] = timed(lambda: ops.cloud_overlap(pts, off, 0.02), reps)
    got = ops.cloud_overlap(pts, off, 0.02).cpu().numpy()
    t = time.perf_counter()
    want = np.zeros((C, C), np.int64)
    for b in range(C):
        tree = cKDTree(clouds[b])
        for a in range(C):
            d, _ = tree.query(clouds[a], workers=16)
            want[a, b] = (d < 0.02).sum()
    r["ckdtree_s"] = time.perf_counter() - t
    r["counts_equal"] = bool(np.array_equal(got, want))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskgraph_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    res = {"device": torch.cuda.get_device_name(0), "shape": {"frames": FRAMES, "W": W_IMG, "H": H_IMG, "masks": MASKS}}
    for name, fn in (("dbscan", bench_dbscan), ("affinity", bench_affinity), ("ray_boxes", bench_ray_boxes),
                     ("overlap", bench_overlap)):
        res[name] = fn(rs, a.reps)
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
