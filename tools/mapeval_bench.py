"""Geometry evaluation at native size (openobj_amd/map_eval.py, objnerf_mapeval.hip) -> profiles/mapeval_bench.txt.

    python tools/mapeval_bench.py [--objects 51] [--dim 192] [--samples 10000] [--scene-samples 200000] [--reps 5]
                                  [--out profiles/mapeval_bench.txt]

A seeded map of `objects` closed meshes, each the ops.marching_cubes surface of an analytic volume (a sphere whose radius
is modulated by a few harmonics; about 100 k vertices / 200 k faces at --dim 192), and a perturbed copy of every one as
"ground truth" (other harmonic amplitudes, a small shift).  Times, with device events, after a warm-up, the variants
ALTERNATING inside every repetition (median / min / max over the repetitions):
  sample   one ops.mesh_sample call over all 2 K object segments and the two scene segments;
  build    ops.NearestPlan: cell keys and the two sorts;
  search   both directions of NearestPlan.query, per object (K segments of --samples points) and at scene level (one
           segment of --scene-samples points a side), over a sweep of the cell factor and of the last ring R of tier 1,
           and with the queries handed over as drawn or sorted by cell by this tool (query_sorted below);
  stats    ops.seg_stats over the per-object distances;
and, on the identical points, two baselines: scipy.spatial.cKDTree(...).query(workers=16) on the host (build + query,
host clock, the points already on the host) and a chunked fp64 torch.cdist arg-min on the GPU (device events).  The
search's distances and rows are compared with both baselines', in both directions, and at scene level one case leaves
every query to the brute-force tier (the predicted side moved 50 m away).  The sample counts are ASSUMED sizes (map_eval's docstring)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openobj_amd import ops  # noqa: E402


def make_mesh(dim, dev, g, amp, shift):
    """A closed surface: |p| = 0.38 (1 + sum of three harmonics) in the unit cube centred on the origin."""
    ax = (torch.arange(dim, device=dev, dtype=torch.float32) + 0.5) / dim - 0.5
    x, y, z = torch.meshgrid(ax - float(shift[0]), ax - float(shift[1]), ax - float(shift[2]), indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z).clamp(min=1e-6)
    k, p, amp = [float(v) for v in g["k"]], [float(v) for v in g["p"]], [float(v) for v in amp]
    mod = amp[0] * torch.sin(k[0] * x / r + p[0]) + amp[1] * torch.sin(k[1] * y / r + p[1]) \
        + amp[2] * torch.sin(k[2] * z / r + p[2])
    vol = 0.38 * (1.0 + mod) - r
    v, f, _ = ops.marching_cubes(vol, 0.0)
    return v.double() / dim - 0.5, f


def make_map(K, dim, dev, seed):
    rng = np.random.default_rng(seed)
    sides = ([], [])
    for k in range(K):
        g = {"k": rng.integers(2, 6, 3).astype(np.float32), "p": rng.uniform(0, 6.28, 3).astype(np.float32)}
        amp = rng.uniform(0.03, 0.08, 3)
        centre = torch.tensor([1.5 * (k % 8), 1.5 * ((k // 8) % 8), 0.0], dtype=torch.float64, device=dev)
        size = float(rng.uniform(0.3, 1.2))                    # metres
        for si, (a, sh) in enumerate(((amp, np.zeros(3)), (amp * rng.uniform(0.9, 1.1, 3), rng.normal(0, 0.004, 3)))):
            v, f = make_mesh(dim, dev, g, a, sh)
            sides[si].append((v * size + centre, f))
    return sides


def pack(sides, n_obj, n_scene, dev):
    """The segment layout of map_eval.compare: pred objects, gt objects, pred scene, gt scene."""
    verts, faces, face_off, samp_off, base, row = [], [], [0], [0], [], 0
    for side in sides:
        b = []
        for v, f in side:
            b.append(row)
            verts.append(v)
            row += len(v)
        base.append(b)
    for si, side in enumerate(sides):
        for (v, f), b in zip(side, base[si]):
            faces.append(f + b)
            face_off.append(face_off[-1] + len(f))
            samp_off.append(samp_off[-1] + n_obj)
    for si, side in enumerate(sides):
        for (v, f), b in zip(side, base[si]):
            faces.append(f + b)
        face_off.append(face_off[-1] + sum(len(f) for _, f in side))
        samp_off.append(samp_off[-1] + n_scene)
    return torch.cat(verts), torch.cat(faces).contiguous(), face_off, samp_off


def ev_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_variants(variants, reps, host=()):
    """{name: callable} -> {name: (median, min, max)} in ms; the variants alternate inside every repetition."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for rep in range(reps):
        print(f"  .. repetition {rep + 1} of {reps}", flush=True)
        for k, fn in variants.items():
            if k in host:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t[k].append(1e3 * (time.perf_counter() - t0))
            else:
                t[k].append(ev_time(fn))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in t.items()}


def query_sorted(plan, qry, off):
    """plan.query with the queries handed over sorted by cell (a grid of their own, the plan's side) and the answers
    scattered back: the launch geometry the ring kernel's comment asks about (neighbouring lanes walk the same runs)."""
    keys, _ = ops.cell_keys(qry, off, plan.cell)
    order = ops._sort_in_segments(keys, torch.as_tensor(off), qry.device)[1]
    sd, si = plan.query(qry[order].contiguous(), off)
    d2, idx = torch.empty_like(sd), torch.empty_like(si)
    d2[order], idx[order] = sd, si
    return d2, idx


def cdist_nearest(q, r, chunk=2048):
    d = torch.empty(len(q), dtype=torch.float64, device=q.device)
    i = torch.empty(len(q), dtype=torch.int64, device=q.device)
    for a in range(0, len(q), chunk):
        m, j = torch.cdist(q[a:a + chunk], r).min(dim=1)
        d[a:a + chunk], i[a:a + chunk] = m, j
    return d, i


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--objects", type=int, default=51)
    ap.add_argument("--dim", type=int, default=192)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--scene-samples", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--factors", type=float, nargs="+", default=[0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    ap.add_argument("--rings", type=int, nargs="+", default=[1, 2, 3, 4, 6])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapeval_bench.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    K, n, ns = a.objects, a.samples, a.scene_samples
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def row(name, t):
        say(f"  {name:<44s} {t[0]:10.3f} ms   (min {t[1]:.3f}, max {t[2]:.3f})")

    sides = make_map(K, a.dim, dev, 0)
    V, F, face_off, samp_off = pack(sides, n, ns, dev)
    nv = [len(v) for v, _ in sides[0]]
    nf = [len(f) for _, f in sides[0]]
    say(f"mapeval_bench: {torch.cuda.get_device_name(0)}; {K} objects a side, dim {a.dim}: vertices {min(nv)} .. {max(nv)} "
        f"(mean {np.mean(nv):.0f}), faces {min(nf)} .. {max(nf)} (mean {np.mean(nf):.0f}); {len(V)} vertices and {len(F)} face "
        f"rows in the call; {n} samples per object and side, {ns} per scene and side (assumed sizes); {a.reps} repetitions")
    del sides
    pts, tri = ops.mesh_sample(V, F, face_off, samp_off, 0)
    say("\nsampling and statistics")
    obj = {"pred": pts[:K * n], "gt": pts[K * n:2 * K * n]}
    scn = {"pred": pts[2 * K * n:2 * K * n + ns], "gt": pts[2 * K * n + ns:]}
    off_o, off_s = [i * n for i in range(K + 1)], [0, ns]
    d_acc = torch.sqrt(ops.NearestPlan(obj["gt"], off_o).query(obj["pred"], off_o)[0])
    t = run_variants({"mesh_sample": lambda: ops.mesh_sample(V, F, face_off, samp_off, 0),
                      "seg_stats": lambda: ops.seg_stats(d_acc, off_o, (0.05, 0.01))}, a.reps)
    row(f"mesh_sample, {len(pts)} samples, {len(face_off) - 1} segments", t["mesh_sample"])
    row(f"seg_stats, {len(d_acc)} distances, {K} segments", t["seg_stats"])

    for level, P, off in (("objects", obj, off_o), ("scene", scn, off_s)):
        nq = len(P["pred"])
        say(f"\n{level}: {len(off) - 1} segment(s), {nq} points a side, both directions")
        # the baselines, and the answers they give
        hp, hg = P["pred"].cpu().numpy(), P["gt"].cpu().numpy()
        from scipy.spatial import cKDTree
        kd = {}

        def kdtree():
            for s in range(len(off) - 1):
                p, g = hp[off[s]:off[s + 1]], hg[off[s]:off[s + 1]]
                kd[("a", s)] = cKDTree(g).query(p, workers=16)
                kd[("c", s)] = cKDTree(p).query(g, workers=16)

        cd = {}

        def cdist():
            for s in range(len(off) - 1):
                p, g = P["pred"][off[s]:off[s + 1]], P["gt"][off[s]:off[s + 1]]
                cd[("a", s)] = cdist_nearest(p, g)
                cd[("c", s)] = cdist_nearest(g, p)

        auto = ops.NearestPlan(P["gt"], off)
        spacing = auto.cell / ops.NEAREST_CELL_FACTOR
        say(f"  spacing from extents and counts {spacing:.5f} m; the default factor: {ops.NEAREST_CELL_FACTOR:g}; R default: the "
            f"library's NN_RINGS")

        def search(f, rings, sort, build=True):
            """f = None: the plan chooses the cell itself (point bounds, a copy to the host), as a user's call does."""
            plans = {}
            cell = None if f is None else f * spacing

            def fn():
                if build or not plans:
                    plans["g"], plans["p"] = ops.NearestPlan(P["gt"], off, cell), ops.NearestPlan(P["pred"], off, cell)
                if build == "only":
                    return
                if sort:
                    query_sorted(plans["g"], P["pred"], off)
                    query_sorted(plans["p"], P["gt"], off)
                else:
                    plans["g"].query(P["pred"], off, max_rings=rings)
                    plans["p"].query(P["gt"], off, max_rings=rings)
            return fn

        f0 = ops.NEAREST_CELL_FACTOR
        variants = {"k-d tree on the host, 16 workers (build + query)": kdtree,
                    "torch.cdist fp64 arg-min on the GPU, chunked": cdist,
                    f"grid build only (2 plans), factor {f0:g}": search(f0, 0, True, "only"),
                    "build (cell = None: chosen by the plan) + search": search(None, 0, False)}
        if level == "scene":
            # every query left open by tier 1: the predicted side moved 50 m away, one direction
            far = (P["pred"] + torch.tensor([50.0, 0.0, 0.0], dtype=torch.float64, device=dev)).contiguous()
            plan_far = ops.NearestPlan(P["gt"], off, f0 * spacing)
            variants["all queries open (pred moved 50 m), pred -> gt only"] = lambda: plan_far.query(far, off)
            variants["the same by torch.cdist"] = lambda: cdist_nearest(far, P["gt"])
        for f in a.factors:
            variants[f"search, factor {f:g}, R default, sorted"] = search(f, 0, True, False)
            variants[f"search, factor {f:g}, R default, as drawn"] = search(f, 0, False, False)
        for r in a.rings:
            for f in (f0 / 2, f0, f0 * 2):
                variants[f"search, factor {f:g}, R {r}, as drawn"] = search(f, r, False, False)
        t = run_variants(variants, a.reps, host=("k-d tree on the host, 16 workers (build + query)",))
        for k in variants:
            row(k, t[k])
        # agreement of the three answers, both directions
        ours = {"a": auto.query(P["pred"], off), "c": ops.NearestPlan(P["pred"], off).query(P["gt"], off)}
        for tag, name in (("a", "pred -> gt"), ("c", "gt -> pred")):
            d = torch.sqrt(ours[tag][0])
            idx = ours[tag][1]
            hd, hidx = d.cpu().numpy(), idx.cpu().numpy()
            worst, same, cworst, csame, cbits = 0.0, 0, 0.0, 0, 0
            for s in range(len(off) - 1):
                dt, it = kd[(tag, s)]
                worst = max(worst, float(np.max(np.abs(hd[off[s]:off[s + 1]] - dt) / np.maximum(dt, 1e-300))))
                same += int(np.count_nonzero(hidx[off[s]:off[s + 1]] == it + off[s]))
                dc, ic = cd[(tag, s)]
                ds = d[off[s]:off[s + 1]]
                cworst = max(cworst, float(((dc - ds).abs() / ds.clamp(min=1e-300)).max()))
                csame += int((ic + off[s] == idx[off[s]:off[s + 1]]).sum())
                cbits += int((dc == ds).sum())
            say(f"  {name}, against the k-d tree: largest relative difference of a distance {worst:.3e}; the same row for "
                f"{same} of {nq} queries")
            say(f"  {name}, against torch.cdist: largest relative difference of a distance {cworst:.3e}; the same distance "
                f"to the last bit for {cbits}, the same row for {csame} of {nq} queries")
        del cd
        del kd

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
