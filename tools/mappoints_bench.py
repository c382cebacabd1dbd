"""Labelling a cloud against the native map (openobj_amd/map_points.py, objnerf_mappoints.hip) -> profiles/mappoints_bench.txt.

    python tools/mappoints_bench.py [--points 2000000] [--out profiles/mappoints_bench.txt] [--reps 5]

Shape: the native map of tools/bound_bench.py -- 50 hidden-32 objects and the hidden-128 background, every box fitted by
ops.object_bounds to synthetic.native_bound_map's keyframes -- with randomly initialised networks whose out_alpha.bias is
set to 1, so that a candidate is occupied as a mesh vertex of a trained map is (a freshly initialised network is occupied
almost nowhere and the head pass would have nothing to do).  Two clouds, both measured:
  room     drawn uniformly in the room, the axis-aligned hull of all boxes.  The generator's objects are thin slabs in
           front of the background surface, so most of this cloud is free space that no box contains;
  surface  half of the points uniformly inside the background's box, half inside object boxes (the object drawn
           uniformly): where the vertices of a room mesh lie.
The cloud size (2 M points by default) is an ASSUMPTION about the order of a room mesh's vertex count, not a measured
figure.

Records: pairs per point; the time of every pass (device events, a synchronise per pass, median of 4 x reps calls) and of
the whole call with and without the feature (host clock; the call and the baseline ALTERNATE in one process, every sample
repeats its call until it covers about 0.3 s, median / min / max over reps samples); the ragged fused kernel's pairs/s beside
eval_kernel's points/s on the same number of points laid out rectangularly (ops.eval_points, code this change does not
touch); the head pass's bytes written over the plain-store HBM rate; and the baseline a user had before MapPoints: per-object
Trainer.eval_points (with the feature) / Trainer._eval_grid (without) over ALL points, a box mask and a running arg-max in
torch."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openobj_amd import cfg as ocfg  # noqa: E402
from openobj_amd import map_points, ops, synthetic, trainer  # noqa: E402

HBM_STORE = 6.1e12          # plain stores, measured (MI355X_MICROARCH.md: 6.0-6.2 TB/s)


def make_map(dev, seed=0):
    kf = synthetic.native_bound_map(dev, seed=seed)
    boxes = [b for _, b in ops.object_bounds(kf)]
    del kf
    torch.cuda.empty_cache()
    torch.manual_seed(seed)
    objects = []
    for k, box in enumerate(boxes):
        if box is None:
            continue
        c = ocfg.Config(ocfg.replica_room0_config(train_device=dev))
        c.obj_id = k
        c.hidden_feature_size = 128 if k == 0 else 32
        c.obj_scale = 5.0 if k == 0 else 2.0
        t = trainer.Trainer(c)
        with torch.no_grad():
            t.fc_occ_map.out_alpha.bias.fill_(1.0)
        objects.append(map_points.MapObject(t, box, obj_id=k, class_id=k % 20))
    return objects


def in_box(box, n, dev, g):
    u = torch.rand(n, 3, device=dev, generator=g) - 0.5
    ext = torch.tensor(np.asarray(box.extent), device=dev, dtype=torch.float32)
    R = torch.tensor(np.asarray(box.R), device=dev, dtype=torch.float32)
    c = torch.tensor(np.asarray(box.center), device=dev, dtype=torch.float32)
    return (u * ext) @ R.T + c


def make_cloud(kind, objects, n, dev, g):
    if kind == "room":
        lo, hi = room(objects)
        return (torch.rand(n, 3, device=dev, generator=g) * torch.tensor(hi - lo, device=dev, dtype=torch.float32)
                + torch.tensor(lo, device=dev, dtype=torch.float32)).contiguous()
    fg = objects[1:]
    per = (n - n // 2) // len(fg)
    parts = [in_box(objects[0].bbox, n - per * len(fg), dev, g)] + [in_box(o.bbox, per, dev, g) for o in fg]
    pts = torch.cat(parts)
    return pts[torch.randperm(n, device=dev, generator=g)].contiguous()


def room(objects):
    corners = np.concatenate([np.asarray(o.bbox.points3d) for o in objects])
    return corners.min(0), corners.max(0)


WINDOW_S = 0.3             # every timed sample repeats its call until it covers about this much work


def paired(fa, fb, reps):
    """fa and fb (each ends in a synchronise) timed ALTERNATELY in one process: per sample, as many calls in a row as
    fill WINDOW_S; -> ((median, min, max) seconds per call of fa, the same of fb, calls per sample of each)."""
    n = []
    for fn in (fa, fb):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        n.append(max(1, int(np.ceil(WINDOW_S / max(time.perf_counter() - t0, 1e-6)))))
    ts = ([], [])
    for _ in range(reps):
        for i, fn in enumerate((fa, fb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n[i]):
                fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) / n[i])
    return tuple((float(np.median(t)), float(min(t)), float(max(t))) for t in ts) + (n,)


def events(fn, reps, inner=20):
    """Device events around `inner` launches in a row, median over reps -> seconds per launch."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / inner)
    return float(np.median(ts))


def baseline(objects, mp, pts, with_feat):
    """What a user did before MapPoints: every object over all N points, then the arg-max in torch (foreground first)."""
    N, dev = pts.shape[0], pts.device
    best = {g: torch.full((N,), 0.5, device=dev) for g in (0, 1)}            # occupied means occ > 0.5
    obj = {g: torch.full((N,), -1, dtype=torch.int32, device=dev) for g in (0, 1)}
    feat = {g: torch.zeros(N, mp.feat_dim, device=dev) for g in (0, 1)} if with_feat else None
    for k, o in enumerate(objects):
        if with_feat:
            occ, _, clip = o.trainer.eval_points(pts, chunk_size=N)
        else:
            occ, _ = o.trainer._eval_grid(pts)
        rec = mp.boxes[k]
        local = (pts - rec[0:3]) @ rec[3:12].view(3, 3)
        better = (local.abs() <= rec[12:15]).all(dim=1) & (occ > best[int(mp.is_bg[k])])
        g = int(mp.is_bg[k])
        best[g] = torch.where(better, occ, best[g])
        obj[g] = torch.where(better, torch.full_like(obj[g], k), obj[g])
        if with_feat:
            feat[g] = torch.where(better[:, None], clip, feat[g])
    fg = obj[0] >= 0
    out = torch.where(fg, obj[0], obj[1])
    occ = torch.where(fg, best[0], best[1])                  # the winner's occupancy (0.5 without one)
    if with_feat:
        return out, torch.where(fg[:, None], feat[0], feat[1]), occ
    return out, None, occ


def measure(kind, objects, mp, a, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    pts = make_cloud(kind, objects, a.points, dev, g)
    lo, hi = room(objects)
    N, K = a.points, mp.K
    r = {"cloud": kind, "points": N, "objects": K, "hidden32_objects": K - len(mp.wide),
         "room_min": [round(float(v), 3) for v in lo], "room_max": [round(float(v), 3) for v in hi]}
    # passes (device events, a synchronise per pass) -- warm, then the median of 4 x reps calls
    for feat in (False, True):
        mp.label(pts, want_color=True, want_feat=feat)
        runs = []
        for _ in range(4 * a.reps):
            st = {}
            out = mp.label(pts, want_color=True, want_feat=feat, stats=st)
            runs.append(st)
        tag = "feat" if feat else "nofeat"
        for key in ("candidates_ms", "eval32_ms", "wide_ms", "resolve_ms") + (("head_ms",) if feat else ()):
            r[f"{key[:-3]}_{tag}_ms"] = round(float(np.median([s[key] for s in runs])), 3)
        r["pairs"], r["pairs32"], r["calls_per_label"] = runs[0]["pairs"], runs[0]["pairs32"], runs[0]["calls"]
        # the whole call and the baseline, alternating, each sample about WINDOW_S of work
        (lm, lmin, lmax), (bm, bmin, bmax), n = paired(lambda: mp.label(pts, want_color=True, want_feat=feat),
                                                       lambda: baseline(objects, mp, pts, feat), a.reps)
        r[f"label_{tag}_s"] = round(lm, 5)
        r[f"label_{tag}_s_min_max"] = [round(lmin, 5), round(lmax, 5)]
        r[f"baseline_{tag}_s"] = round(bm, 5)
        r[f"baseline_{tag}_s_min_max"] = [round(bmin, 5), round(bmax, 5)]
        r[f"calls_per_sample_{tag}"] = n
        r[f"speedup_{tag}"] = round(bm / lm, 2)
    winners = int((out["obj"] >= 0).sum())
    r["pairs_per_point"] = round(r["pairs"] / N, 3)
    r["winners"] = winners
    r["labelled_fraction"] = round(winners / N, 4)
    r["eval32_pairs_per_s_nofeat"] = round(r["pairs32"] / (r["eval32_nofeat_ms"] * 1e-3), 1)
    r["eval32_pairs_per_s_feat"] = round(r["pairs32"] / (r["eval32_feat_ms"] * 1e-3), 1)
    head_bytes = winners * mp.feat_dim * 4
    r["head_bytes"] = head_bytes
    r["head_fraction_of_hbm_store_rate"] = round(head_bytes / (r["head_feat_ms"] * 1e-3) / HBM_STORE, 4)
    # eval_kernel, rectangular, on the same number of points
    k32 = K - len(mp.wide)
    n_rect = max(1, r["pairs32"] // k32)
    rect = torch.rand(k32, n_rect, 3, device=dev, generator=g) * 2 - 1
    for feat in (False, True):
        t = events(lambda: ops.eval_points(mp.arena, rect, want_hfeat=feat), a.reps)
        r[f"eval_kernel_points_per_s_{'feat' if feat else 'nofeat'}"] = round(k32 * n_rect / t, 1)
    r["ragged_over_eval_kernel_nofeat"] = round(r["eval32_pairs_per_s_nofeat"] / r["eval_kernel_points_per_s_nofeat"], 3)
    r["ragged_over_eval_kernel_feat"] = round(r["eval32_pairs_per_s_feat"] / r["eval_kernel_points_per_s_feat"], 3)
    del rect
    # does the baseline label the same points?  It ranks by occupancy = sigmoid(alpha), which saturates (to 1.0f, or to
    # equal values for close alphas), and keeps the first object; label() ranks by alpha.  Counted, not assumed: of the
    # points that disagree, how many have the SAME occupancy for the two winners (a tie the baseline cannot see).
    b_obj, _, b_occ = baseline(objects, mp, pts, False)
    differ = b_obj != out["obj"]
    mine = torch.where(out["obj"] >= 0, ops.occupancy(out["alpha"].contiguous()), torch.full_like(b_occ, 0.5))
    r["baseline_label_agreement"] = round(float((~differ).float().mean()), 6)
    r["baseline_disagreements"] = int(differ.sum())
    r["baseline_disagreements_with_equal_occupancy"] = int((differ & (mine == b_occ)).sum())
    r["expected_gain_K_over_pairs_per_point"] = round(K / r["pairs_per_point"], 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mappoints_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = "cuda:0"
    objects = make_map(dev)
    mp = map_points.MapPoints(objects, device=dev, bg_ids=(0,), pair_budget_bytes=8 << 30)
    res = {"device": torch.cuda.get_device_name(0),
           "cloud_size_note": "2 M points is an assumption about the order of a room mesh, not a measured figure",
           "clouds": [measure(kind, objects, mp, a, dev) for kind in ("room", "surface")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("tools/mappoints_bench.py -- see its docstring for the shape, the two clouds and what each figure is\n")
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
