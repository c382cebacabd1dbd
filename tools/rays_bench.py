"""The ray caster at the native map (openobj_amd/map_rays.py, objnerf_maprays.hip) -> profiles/maprays_bench.txt.

    python tools/rays_bench.py [--out profiles/maprays_bench.txt] [--reps 5] [--objects 51] [--no-baseline]

Shape (ASSUMED sizes, the map of tools/raster_bench.py): 51 objects, each a 400 x 250 vertex sheet, 5.1 M vertices and
10.1 M faces in all, a floor of 16 m x 10 m.  Ray sets: the 1200 x 680 = 816 000 pixel rays of raster_bench's `inside` and
`overview` views (map_rays.view_rays) and a 64 x 2 048 lidar sweep from 1 m above the middle of the floor (elevations
-60 .. 0 degrees).

Timed with device events around windows of calls of about 0.3 s (after a warm-up call; median, min .. max over --reps
windows): the build (Morton codes, the stable sort, slots + leaves + levels, each separately) and, per leaf size 2, 4, 8
and per traversal order, the first-hit cast and the any-hit cast of every ray set, with the node visits and face tests a
ray from `stats`; the resolve pass; MapRaster's visibility pass on the same view for context only (another algorithm, with
snapped vertices).  Every cast's keys are asserted equal across leaf sizes and orders.

Baseline: the same rule restated in torch as brute force on the device -- every ray against every face, the slab gate, the
triangle sequence, the key, an `amin` over the faces -- on ONE object's 198 702 faces and 4 096 of the `overview` rays
that look at it (8.1e8 pairs, in blocks of 64 rays: the largest product that runs in reasonable time; the whole map
times a view would be 8e12 pairs), timed once after a warm-up block, its keys asserted EQUAL to the kernel's."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from openobj_amd import map_raster, map_rays, ops, query  # noqa: E402
from raster_bench import H, INTR, VIEWS, W  # noqa: E402
from regions_bench import WINDOW_S, native_map, timed  # noqa: E402

INF = float("inf")


def torch_keys(verts, faces, pad, o, d, block=64):
    """The rule of include/objnerf_hip.h in torch, every op one call (so it rounds once): -> key int64 [N] (-1: no hit).
    All faces valid and none hidden (the caller's mesh); window [0, inf)."""
    p = verts[faces.long()]                                            # [F, 3, 3]
    p0, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    lo, hi = p.amin(dim=1) - pad, p.amax(dim=1) + pad
    fid = torch.arange(faces.shape[0], device=verts.device)
    cross = lambda a, b: torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    out = []
    BIG = torch.iinfo(torch.int64).max
    for s in range(0, o.shape[0], block):
        oo, dd = o[s:s + block, None], d[s:s + block, None]            # [n, 1, 3]
        inv = 1.0 / dd
        par = ~torch.isfinite(inv)
        a, b = (lo[None] - oo) * inv, (hi[None] - oo) * inv
        near = torch.where(par, torch.full_like(a, -INF), torch.fmin(a, b))
        far = torch.where(par, torch.full_like(a, INF), torch.fmax(a, b))
        tn = torch.fmax(torch.fmax(near[..., 0], near[..., 1]), near[..., 2])
        tf = torch.fmin(torch.fmin(far[..., 0], far[..., 1]), far[..., 2])
        ok = (~par | ((lo[None] <= oo) & (oo <= hi[None]))).all(dim=-1) & (tn <= tf) & (tf >= 0.0)
        pv = cross(dd, e2[None])
        det = dot(e1[None], pv)
        tv = oo - p0[None]
        qv = cross(tv, e1[None])
        U, Vv, T = dot(tv, pv), dot(dd, qv), dot(e2[None], qv)
        neg = det < 0
        det, U, Vv, T = (torch.where(neg, -x, x) for x in (det, U, Vv, T))
        t = T / det + 0.0
        hit = ok & (det != 0) & (U >= 0) & (Vv >= 0) & (U + Vv <= det) & (t >= 0.0) & (tn <= t)
        k = (t.float().view(torch.int32).long() << 32) | fid[None]
        out.append(torch.where(hit, k, torch.full_like(k, BIG)).amin(dim=1))
    k = torch.cat(out)
    return torch.where(k == BIG, torch.full_like(k, -1), k)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maprays_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--objects", type=int, default=51)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    all_obj, _, _ = native_map(a.objects)
    mq = query.MapQuery(all_obj, dev)
    verts, faces, face_off, _ = mq.mesh_buffers()
    V, F, S = mq.V, int(faces.shape[0]), mq.S
    hide = torch.zeros(S, dtype=torch.uint8, device=dev)
    ids = torch.arange(1, S + 1, dtype=torch.int32, device=dev)
    pad = ops.rays_default_pad(verts)
    fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f}) ms   [{t[3]} calls a window]"
    lines = [f"ray caster at the native map: {S} objects x 400 x 250 sheet = {V} vertices, {F} faces (assumed sizes); pad "
             f"{pad:.3g} (assumed: 2^-20 of the largest extent)",
             f"{torch.cuda.get_device_name(0)}; device events, windows of ~{WINDOW_S} s, {a.reps} windows: median (min .. max) ms"]
    sets = {}
    for name, T_WC in VIEWS:
        if name != "close-up":
            sets[name] = (map_rays.view_rays(T_WC, INTR, W, H), T_WC)
    T_WS = np.eye(4)
    T_WS[:3, 3] = (7.8, 5.0, 1.5)
    sets["lidar 64 x 2048"] = (map_rays.lidar_rays(T_WS, 2048, 64, -60.0, 0.0), None)
    dev_rays = {k: tuple(torch.from_numpy(x).to(dev) for x in v[0]) for k, v in sets.items()}
    # ------------------------------------------------------------------------------------------------------ the build
    for leaf in (2, 4, 8):
        box = ops.rays_scene_box(verts)
        codes = ops.rays_build(verts, faces, face_off, pad, leaf, box=box, _stage=1)
        order = torch.sort(codes, stable=True)[1]
        ws = torch.zeros(ops.rays_workspace_bytes(F, leaf), dtype=torch.uint8, device=dev)
        t_c = timed(lambda: ops.rays_build(verts, faces, face_off, pad, leaf, box=box, _stage=1, _codes=codes), a.reps)
        t_s = timed(lambda: torch.sort(codes, stable=True), a.reps)
        t_l = timed(lambda: ops.rays_build(verts, faces, face_off, pad, leaf, ws=ws, box=box, _stage=2, _order=order), a.reps)
        again = ws.clone()
        ops.rays_build(verts, faces, face_off, pad, leaf, ws=ws, box=box, _stage=2, _order=order)
        assert torch.equal(again, ws), "a second build gave other bytes"
        lines += [f"leaf {leaf}: {ops.rays_node_count(F, leaf)} nodes, workspace {ws.numel() / 2 ** 20:.1f} MiB; build "
                  f"{t_c[0] + t_s[0] + t_l[0]:.3f} ms",
                  f"    codes      {fmt(t_c)}", f"    sort       {fmt(t_s)}   (torch.sort, stable)",
                  f"    levels     {fmt(t_l)}   (slots, leaves and {int(np.log2(ops.rays_node_count(F, leaf))) - 1} level launches)"]
        for name, (o, d) in dev_rays.items():
            n = o.shape[0]
            ref = None
            for fixed in (False, True):
                cast = lambda any_hit: ops.rays_cast(verts, faces, face_off, hide, ws, pad, o, d, 0.0, INF, leaf, any_hit,
                                                     _fixed_order=fixed)
                key, stats, status = cast(False)
                hit, astats, _ = cast(True)
                assert int(status.item()) == 0 and torch.equal(hit != 0, key != -1)
                if name not in KEYS:
                    KEYS[name] = key
                assert torch.equal(KEYS[name], key), "another leaf size or order gave other keys"
                st, ast = stats.cpu().tolist(), astats.cpu().tolist()
                t_f, t_a = timed(lambda: cast(False), a.reps), timed(lambda: cast(True), a.reps)
                order_name = "fixed order " if fixed else "nearer first"
                lines += [f"  {name}, {order_name}: {st[1]} of {n} rays hit",
                          f"    first hit  {fmt(t_f)}   {n / t_f[0] / 1e3:7.1f} M rays/s, {st[3] / n:6.1f} node visits, {st[4] / n:5.1f} face tests a ray",
                          f"    any hit    {fmt(t_a)}   {n / t_a[0] / 1e3:7.1f} M rays/s, {ast[3] / n:6.1f} node visits, {ast[4] / n:5.1f} face tests a ray"]
            if leaf == 4:
                t_r = timed(lambda: ops.rays_resolve(verts, faces, face_off, ids, o, d, KEYS[name]), a.reps)
                lines.append(f"    resolve    {fmt(t_r)}")
                T_WC = sets[name][1]
                if T_WC is not None:
                    T_CW = torch.from_numpy(map_raster.camera_rows(T_WC)).to(dev)
                    rws = torch.empty(ops.raster_workspace_bytes(V, F), dtype=torch.uint8, device=dev)
                    t_v = timed(lambda: ops.raster_visibility(verts, faces, face_off, hide, T_CW, INTR, W, H, 0.05, ws=rws), a.reps)
                    rkey = ops.raster_visibility(verts, faces, face_off, hide, T_CW, INTR, W, H, 0.05, ws=rws)[0].reshape(-1)
                    same = int(((rkey & 0xFFFFFFFF) == (KEYS[name] & 0xFFFFFFFF)).sum())
                    lines.append(f"    for context only: MapRaster's visibility pass on this view {fmt(t_v)}; the two name the same "
                                 f"face (or none) at {same} of {n} pixels")
    # ---------------------------------------------------------------------------------------------------- the baseline
    if not a.no_baseline:
        f1 = int(face_off[1].item())
        v1 = int(faces[:f1].max().item()) + 1
        sv, sf, soff = verts[:v1].contiguous(), faces[:f1].contiguous(), face_off[:2].contiguous()
        o, d = dev_rays["overview"]
        first = (KEYS["overview"] != -1) & ((KEYS["overview"] & 0xFFFFFFFF) < f1)
        sel = torch.nonzero(first).reshape(-1)[:3584]
        sel = torch.cat([sel, torch.nonzero(~first).reshape(-1)[:512]])
        so, sd = o[sel].contiguous(), d[sel].contiguous()
        sws, _ = ops.rays_build(sv, sf, soff, pad, 4)
        kern = lambda: ops.rays_cast(sv, sf, soff, hide[:1], sws, pad, so, sd, 0.0, INF, 4)[0]
        key = kern()
        torch_keys(sv, sf, pad, so[:64], sd[:64])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tkey = torch_keys(sv, sf, pad, so, sd)
        e1.record()
        e1.synchronize()
        t_torch, t_k = e0.elapsed_time(e1), timed(kern, a.reps)
        assert torch.equal(tkey, key), "the torch restatement of the rule disagrees"
        lines.append(f"baseline: brute force in torch, {f1} faces x {len(sel)} rays = {f1 * len(sel):.3g} pairs "
                     f"({int((key != -1).sum())} rays hit): {t_torch:.1f} ms; the kernel on the same mesh and rays {t_k[0]:.3f} ms "
                     f"= {t_torch / t_k[0]:.0f} x (keys equal)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


KEYS = {}

if __name__ == "__main__":
    main()
