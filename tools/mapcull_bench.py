"""Culling a map to what the frames observed, at native size (openobj_amd/map_cull.py, objnerf_meshcull.hip)
-> profiles/mapcull_bench.txt.

    python tools/mapcull_bench.py [--objects 51] [--dim 192] [--frames 200] [--batch 32] [--width 1200] [--height 680]
                                  [--reps 3] [--decode-frames 32] [--out profiles/mapcull_bench.txt]

A seeded map of `objects` closed meshes, each the ops.marching_cubes surface of an analytic volume (about 100 k vertices
/ 200 k faces at --dim 192; the generator of tools/mapeval_bench.py), spread over a wall-sized patch 6 m in front of a
camera that pans and turns over `frames` synthetic frames; each depth image is what its pose measures of the plane through
the objects' centres, rippled by 5 cm and with 5 % invalid pixels, so about the front half of every object is seen.  Times, with device events, after a
warm-up, the variants ALTERNATING inside every repetition (median / min / max over the repetitions):
  views     ops.vertex_views over all vertices, the frames in batches of --batch (the depth already on the device);
  compact   ops.mesh_compact of all meshes back to back, rule "all" and "any" (count, the read-back of the two totals, emit);
and the same rule and the same compaction written in torch on the GPU (fp64 element-wise operations in the rule's order,
frame by frame; masks, a cumulative sum and index_select), whose results must equal the kernels' exactly.  Separately,
on the host clock: decoding --decode-frames 16-bit PNG depth images of that size into [W, H] fp32 metres (what
dataset.depth_and_pose does per frame) and copying them to the device -- the part of a real run no kernel shortens."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from openobj_amd import dataset, map_cull, ops  # noqa: E402
from mapeval_bench import ev_time, make_mesh  # noqa: E402


def make_map(K, dim, dev, seed):
    rng = np.random.default_rng(seed)
    verts, faces, vert_off = [], [], [0]
    for k in range(K):
        g = {"k": rng.integers(2, 6, 3).astype(np.float32), "p": rng.uniform(0, 6.28, 3).astype(np.float32)}
        v, f = make_mesh(dim, dev, g, rng.uniform(0.03, 0.08, 3), np.zeros(3))
        centre = torch.tensor([1.1 * (k % 9) - 4.4, 1.1 * (k // 9) - 2.75, 6.0], dtype=torch.float64, device=dev)
        verts.append(v * float(rng.uniform(0.3, 1.2)) + centre)
        faces.append(f + vert_off[-1])
        vert_off.append(vert_off[-1] + len(v))
    return torch.cat(verts).contiguous(), torch.cat(faces).contiguous(), vert_off


def make_frames(n, W, H, intr, dev, seed):
    """T_WC [n, 4, 4] (a pan along x with a slow yaw) and depth [n, W, H] fp32: what each pose measures of the plane
    z = 6 m through the objects' centres, with a ripple of 5 cm and 5 % zeros."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = intr
    T = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        a = 0.25 * np.sin(2 * np.pi * i / n)
        T[i, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        T[i, :3, 3] = [2.0 * (i / max(n - 1, 1) - 0.5), 0.1 * np.cos(7.0 * i / n), 0.0]
    gen = torch.Generator(device=dev).manual_seed(seed)
    u = torch.arange(W, device=dev, dtype=torch.float32)[:, None]
    v = torch.arange(H, device=dev, dtype=torch.float32)[None, :]
    depth = torch.empty(n, W, H, dtype=torch.float32, device=dev)
    for i in range(n):
        R = T[i, :3, :3]
        dz = float(R[2, 0]) * (u - cx) / fx + float(R[2, 1]) * (v - cy) / fy + float(R[2, 2])      # the ray's world z per unit depth
        d = (6.0 - float(T[i, 2, 3])) / dz
        d = d + 0.05 * torch.sin(u / 90.0 + float(rng.uniform(0, 6.28))) * torch.cos(v / 70.0 + float(rng.uniform(0, 6.28)))
        d[torch.rand(W, H, device=dev, generator=gen) < 0.05] = 0.0
        depth[i] = d
    return T, depth


def torch_views(verts, T_CW, depth, intr, z_min, eps, margin):
    """The rule of objnerf_vertex_views in torch fp64, one frame at a time (every operation a kernel of its own)."""
    fx, fy, cx, cy = intr
    W, H = depth.shape[1:]
    px, py, pz = verts[:, 0].contiguous(), verts[:, 1].contiguous(), verts[:, 2].contiguous()
    views = torch.zeros(len(verts), dtype=torch.int32, device=verts.device)
    M = T_CW.reshape(-1, 12).cpu().tolist()
    for f, m in enumerate(M):
        xc = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3]
        yc = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7]
        zc = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11]
        iu = torch.floor((fx * xc) / zc + cx + 0.5)
        iv = torch.floor((fy * yc) / zc + cy + 0.5)
        inside = (zc > z_min) & (iu >= margin) & (iu <= W - 1 - margin) & (iv >= margin) & (iv <= H - 1 - margin)
        flat = torch.where(inside, iu * H + iv, torch.zeros_like(iu)).long()
        d = depth[f].reshape(-1)[flat].double()
        views += (inside & (d > 0) & (zc <= d + eps)).int()
    return views


def torch_compact(keep, faces, rule):
    k = keep.bool()[faces.long()]
    stay = k.all(dim=1) if rule == "all" else k.any(dim=1)
    face_old = torch.nonzero(stay).reshape(-1)
    kept = faces.long()[face_old]
    used = torch.zeros(len(keep), dtype=torch.bool, device=keep.device)
    used[kept.reshape(-1)] = True
    old_of_new = torch.nonzero(used).reshape(-1)
    new_of_old = torch.where(used, torch.cumsum(used.int(), 0, dtype=torch.int32) - 1, torch.full_like(used, -1, dtype=torch.int32))
    return {"new_of_old": new_of_old, "old_of_new": old_of_new.int(), "faces": new_of_old[kept], "face_old": face_old.int()}


def run_variants(variants, reps):
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for rep in range(reps):
        print(f"  .. repetition {rep + 1} of {reps}", flush=True)
        for k, fn in variants.items():
            t[k].append(ev_time(fn))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in t.items()}


def decode_times(n, W, H, dev, reps):
    """Host clock, per frame: PNG -> [W, H] fp32 metres as dataset.py does it, and the copy to the device."""
    from PIL import Image
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as tmp:
        yy, xx = np.mgrid[0:H, 0:W]
        for i in range(n):
            img = (6000 + 300 * np.sin(xx / 90.0 + i) * np.cos(yy / 70.0) + rng.integers(0, 8, (H, W))).astype(np.uint16)
            Image.fromarray(img).save(os.path.join(tmp, "depth_%d.png" % i))
        dec, up = [], []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            frames = []
            for i in range(n):
                d = dataset._read_image(os.path.join(tmp, "depth_%d.png" % i)).transpose(1, 0).astype(np.float32) * np.float32(1e-3)
                d[d > 8.0] = 0.0
                frames.append(d)
            batch = np.stack(frames)
            t1 = time.perf_counter()
            torch.from_numpy(batch).to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep:                                            # the first pass warms the page cache
                dec.append(1e3 * (t1 - t0) / n)
                up.append(1e3 * (t2 - t1) / n)
    stat = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    return stat(dec), stat(up)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--objects", type=int, default=51)
    ap.add_argument("--dim", type=int, default=192)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--decode-frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapcull_bench.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    W, H, B = a.width, a.height, a.batch
    intr = (0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def row(name, t, unit="ms"):
        say(f"  {name:<58s} {t[0]:10.3f} {unit}   (min {t[1]:.3f}, max {t[2]:.3f})")

    verts, faces, vert_off = make_map(a.objects, a.dim, dev, 0)
    T_WC, depth = make_frames(a.frames, W, H, intr, dev, 0)
    T_CW = torch.from_numpy(map_cull.world_to_camera(T_WC)).to(dev)
    nv = np.diff(vert_off)
    say(f"mapcull_bench: {torch.cuda.get_device_name(0)}; {a.objects} objects, dim {a.dim}: vertices {nv.min()} .. {nv.max()} "
        f"(mean {nv.mean():.0f}), {len(verts)} vertices and {len(faces)} faces in all; {a.frames} frames of {W} x {H} in "
        f"batches of {B}; z_min 0, eps {map_cull.EPS} (an assumed value), margin 0, min_views 1; {a.reps} repetitions")
    kw = dict(z_min=0.0, eps=map_cull.EPS, margin=0)

    def views_kernel():
        out = torch.zeros(len(verts), dtype=torch.int32, device=dev)
        for b0 in range(0, a.frames, B):
            ops.vertex_views(verts, T_CW[b0:b0 + B], depth[b0:b0 + B], intr, out=out, **kw)
        return out

    say("\nvisibility counts")
    t = run_variants({"k": views_kernel, "t": lambda: torch_views(verts, T_CW, depth, intr, **kw)}, a.reps)
    pairs = float(len(verts)) * a.frames
    row(f"ops.vertex_views, {pairs:.3g} vertex-frame pairs", t["k"])
    row("the same rule in torch fp64, frame by frame", t["t"])
    say(f"  kernel: {pairs / t['k'][0] / 1e6:.1f} G pairs/s; torch / kernel = {t['t'][0] / t['k'][0]:.1f}")
    views, tviews = views_kernel(), torch_views(verts, T_CW, depth, intr, **kw)
    same = bool(torch.equal(views, tviews))
    say(f"  the two agree exactly: {same} ({int((views != tviews).sum())} of {len(verts)} counts differ); "
        f"{int((views > 0).sum())} vertices seen at least once, the largest count {int(views.max())}")

    say("\ncompaction (all meshes back to back)")
    keep = (views >= 1).to(torch.uint8)
    variants = {}
    for rule in ("all", "any"):
        variants[f"ops.mesh_compact, rule {rule}"] = lambda rule=rule: ops.mesh_compact(keep, faces, rule)
        variants[f"masks + cumsum + gathers in torch, rule {rule}"] = lambda rule=rule: torch_compact(keep, faces, rule)
    t = run_variants(variants, a.reps)
    for k in variants:
        row(k, t[k])
    for rule in ("all", "any"):
        r, w = ops.mesh_compact(keep, faces, rule), torch_compact(keep, faces, rule)
        ok = all(torch.equal(r[k], w[k]) for k in r)
        same = same and ok
        say(f"  rule {rule}: {len(r['old_of_new'])} of {len(verts)} vertices and {len(r['face_old'])} of {len(faces)} faces "
            f"stay; the two agree exactly: {ok}")

    say(f"\nframe decode on the host ({a.decode_frames} 16-bit PNG files of {W} x {H}, per frame, host clock)")
    dec, up = decode_times(a.decode_frames, W, H, dev, a.reps)
    row("PNG -> [W, H] fp32 metres (Pillow, scale, transpose)", dec)
    row("copy to the device", up)
    k_frame = ev_time(views_kernel) / a.frames
    say(f"  per frame: decode {dec[0]:.3f} ms + copy {up[0]:.3f} ms on the host against {k_frame:.3f} ms of vertex_views "
        f"for {len(verts)} vertices")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    if not same:
        raise SystemExit("the kernels and the torch form disagree")


if __name__ == "__main__":
    main()
