"""The mesh rasteriser at the native map (openobj_amd/map_raster.py, objnerf_mapraster.hip) -> profiles/mapraster_bench.txt.

    python tools/raster_bench.py [--out profiles/mapraster_bench.txt] [--reps 5] [--objects 51] [--no-baseline]

Shape (ASSUMED sizes, the layout of tools/regions_bench.py): 51 objects, each a 400 x 250 vertex sheet = 100 000 vertices
and 198 702 faces in cell order, 5.1 M vertices and 10.1 M faces in all, laid out as a floor of 16 m x 10 m; 1200 x 680
pixels, fx = fy = 600.  Three views: `inside` (a camera 2 m above a corner looking across the floor: most faces are
sub-pixel), `close-up` (15 cm above one sheet looking down: a cell is 16 pixels, so every face it sees takes the large
path) and `overview` (12 m above the middle: no large face at all; the view of the torch baseline).

Timed with device events around windows of calls of about 0.3 s (after a warm-up call; median, min .. max over --reps
windows), per pass through the diagnostic `_passes` mask of ops.raster_visibility: the vertex pass, the clears and the
face pass, the face pass with the large-face pass (the large pass is the difference), the resolve pass, and the whole
MapRaster.render call with its read-back (wall clock).  The `stats` counters of each view stand beside them.

Baseline: the visibility pass restated in torch on the device -- the vertex projection in fp64, the up-to-4 x 4 candidate
pixels of every face whose box holds a sample, the same keys, an int64 `amin` scatter -- timed once after a warm-up run,
its keys asserted EQUAL to the kernel's on the view without large faces."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from openobj_amd import map_raster, ops, query  # noqa: E402
from regions_bench import WINDOW_S, native_map, timed  # noqa: E402

W, H, INTR = 1200, 680, (600.0, 600.0, 599.5, 339.5)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


VIEWS = (("inside", look_at((0.5, 0.5, 2.5), (9.0, 6.0, 0.5))),
         ("close-up", look_at((0.8, 0.5, 0.65), (0.8, 0.5, 0.5), up=(0.0, 1.0, 0.0))),
         ("overview", look_at((7.8, 5.0, 12.5), (7.8, 5.0, 0.5), up=(0.0, 1.0, 0.0))))


def torch_visibility(verts, faces, hide_f, T_CW, intr, z_near, chunk=1 << 21):
    """The visibility pass in torch: -> key int64 [W, H] (-1 = nothing drawn).  Faces with a box larger than 4 x 4 pixels
    are NOT handled (the caller checks that the view has none)."""
    fx, fy, cx, cy = intr
    M = T_CW.reshape(12)
    p = verts
    cam = [((M[4 * r] * p[:, 0] + M[4 * r + 1] * p[:, 1]) + M[4 * r + 2] * p[:, 2]) + M[4 * r + 3] for r in range(3)]
    X = torch.floor(((fx * cam[0]) / cam[2] + cx) * 256.0 + 0.5)
    Y = torch.floor(((fy * cam[1]) / cam[2] + cy) * 256.0 + 0.5)
    ok = (cam[2] >= z_near) & (X.abs() <= 2.0 ** 25) & (Y.abs() <= 2.0 ** 25)
    Xi, Yi = torch.where(ok, X, torch.zeros_like(X)).long(), torch.where(ok, Y, torch.zeros_like(Y)).long()
    iz = 1.0 / cam[2]
    BIG = torch.iinfo(torch.int64).max
    key = torch.full((W * H,), BIG, dtype=torch.int64, device=verts.device)
    di = torch.arange(4, device=verts.device).repeat_interleave(4)[None]
    dj = torch.arange(4, device=verts.device).repeat(4)[None]
    for f0 in range(0, faces.shape[0], chunk):
        f = faces[f0:f0 + chunk].long()
        fid = torch.arange(f0, f0 + f.shape[0], device=verts.device)
        x, y = Xi[f], Yi[f]
        A = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        i0, i1 = ((x.min(1).values + 255) >> 8).clamp(min=0), (x.max(1).values >> 8).clamp(max=W - 1)
        j0, j1 = ((y.min(1).values + 255) >> 8).clamp(min=0), (y.max(1).values >> 8).clamp(max=H - 1)
        keep = ok[f].all(1) & (A != 0) & (i0 <= i1) & (j0 <= j1) & ~hide_f[f0:f0 + f.shape[0]]
        f, fid, x, y, A, i0, i1, j0, j1 = (t[keep] for t in (f, fid, x, y, A, i0, i1, j0, j1))
        sw = A < 0                                                                  # swap corners 1 and 2
        o1, o2 = torch.where(sw, 2, 1)[:, None], torch.where(sw, 1, 2)[:, None]
        x = torch.cat([x[:, :1], x.gather(1, o1), x.gather(1, o2)], 1)
        y = torch.cat([y[:, :1], y.gather(1, o1), y.gather(1, o2)], 1)
        z = iz[f]
        z = torch.cat([z[:, :1], z.gather(1, o1), z.gather(1, o2)], 1)
        A = A.abs()
        i, j = i0[:, None] + di, j0[:, None] + dj                                      # [n, 16] candidates
        inside = (i <= i1[:, None]) & (j <= j1[:, None])
        px, py = 256 * i, 256 * j

        def E(a, b):
            return (x[:, b, None] - x[:, a, None]) * (py - y[:, a, None]) - (y[:, b, None] - y[:, a, None]) * (px - x[:, a, None])

        w0, w1, w2 = E(1, 2), E(2, 0), E(0, 1)
        cover = inside & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
        q = (w0.double() * z[:, 0, None] + w1.double() * z[:, 1, None]) + w2.double() * z[:, 2, None]
        d = (A.double()[:, None] / q).float()
        k = (d.view(torch.int32).long() << 32) | fid[:, None]
        key.scatter_reduce_(0, (i * H + j)[cover], k[cover], reduce="amin")
    return torch.where(key == BIG, torch.full_like(key, -1), key).reshape(W, H)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapraster_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--objects", type=int, default=51)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    all_obj, _, _ = native_map(a.objects)
    mq = query.MapQuery(all_obj, dev)
    mr = map_raster.MapRaster(mq)
    verts, faces, face_off, _ = mq.mesh_buffers()
    V, F, S = mq.V, int(faces.shape[0]), mq.S
    colors = mq.color_by_rgb()
    hide = torch.zeros(S, dtype=torch.uint8, device=dev)
    ids = torch.arange(1, S + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.raster_workspace_bytes(V, F), dtype=torch.uint8, device=dev)
    lines = [f"mesh rasteriser at the native map: {S} objects x 400 x 250 sheet = {V} vertices, {F} faces (assumed sizes), "
             f"{W} x {H} pixels",
             f"{torch.cuda.get_device_name(0)}; device events, windows of ~{WINDOW_S} s, {a.reps} windows: median (min .. max) ms",
             "context, not a like-for-like ratio: MapView.render of a native view through the networks is recorded in README.md "
             "at about 490 ms (an earlier commit, other inputs)"]
    for name, T_WC in VIEWS:
        T_CW = torch.from_numpy(map_raster.camera_rows(T_WC)).to(dev)
        vis = lambda passes=0: ops.raster_visibility(verts, faces, face_off, hide, T_CW, INTR, W, H, 0.05, ws=ws, _passes=passes)
        key, stats, status, _ = vis()
        res = lambda: ops.raster_resolve(verts, faces, face_off, ids, colors, ws, key, T_WC[:3, 3])
        out = res()
        st = dict(zip(ops.RASTER_STATS, stats.cpu().tolist()))
        painted, seen = int((out["winner"] >= 0).sum()), int((out["counts"] > 0).sum())
        assert int(status.item()) == 0 and sum(st.values()) == F and int(out["counts"].sum()) == painted
        t_all, t_v, t_f, t_fl, t_r = (timed(fn, a.reps) for fn in (vis, lambda: vis(1), lambda: vis(2), lambda: vis(6), res))
        key2 = vis()[0]
        assert torch.equal(key2, key), "a later run gave other keys"
        walls = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mr.render(T_WC, INTR, W, H, colors=colors)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        walls = walls[1:]
        fmt = lambda t: f"{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f}) ms   [{t[3]} calls a window]"
        lines += [f"view {name}: {painted} of {W * H} pixels painted, {seen} objects seen; faces: " +
                  ", ".join(f"{k} {v}" for k, v in st.items()),
                  f"  visibility   {fmt(t_all)}", f"    vertices   {fmt(t_v)}", f"    faces      {fmt(t_f)}   (with the clears)",
                  f"    large      {t_fl[0] - t_f[0]:8.3f} ms   (faces + large {t_fl[0]:.3f} ms, less faces)",
                  f"  resolve      {fmt(t_r)}",
                  f"  render       {np.median(walls):8.3f} ({min(walls):.3f} .. {max(walls):.3f}) ms wall, with the read-back of three images"]
        if a.no_baseline or st["large"] != 0:
            continue
        hide_f = torch.zeros(F, dtype=torch.bool, device=dev)
        torch_visibility(verts, faces, hide_f, T_CW, INTR, 0.05)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tkey = torch_visibility(verts, faces, hide_f, T_CW, INTR, 0.05)
        e1.record()
        e1.synchronize()
        t_torch = e0.elapsed_time(e1)
        assert torch.equal(tkey, key), "the torch restatement of the visibility pass disagrees"
        lines.append(f"  torch visibility {t_torch:8.3f} ms = {t_torch / t_all[0]:.1f} x visibility (keys equal)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
