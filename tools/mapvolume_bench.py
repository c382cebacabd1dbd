"""The navigation volume of the native map (openobj_amd/map_volume.py, objnerf_mapvolume.hip) -> profiles/mapvolume_bench.txt.

    python tools/mapvolume_bench.py [--out profiles/mapvolume_bench.txt] [--reps 5] [--radius 0.25]

Shape: the native map of tools/mappoints_bench.py (50 hidden-32 objects and the hidden-128 background, the boxes of
synthetic.native_bound_map), voxelised twice: a cube of 256^3 voxels over the room, and a slab of 1024 x 1024 x 16 voxels
over its lower part projected along z to 1024 x 1024 x 1 (the 2-D case of a ground robot).  That tool sets every network's
out_alpha.bias to 1, which fills each box; here the background's is set to -1 instead: its box is the whole room, and a room
that is occupied everywhere has no free space to plan in.  The background is still a candidate of every voxel and is still
evaluated, so voxelise pays for all 51 objects; the 50 objects are the obstacles.

Every pass is timed with device events around a window of calls that covers about 0.3 s (after a warm-up call; median, min
and max over --reps windows), beside the same definition restated in torch on the device; the torch outputs are asserted
EQUAL to the kernels'.  clearance is also compared with scipy.ndimage.distance_transform_edt on the host where scipy is
installed (the distances only: its choice among equidistant sites is not specified); clearance is timed once more on
random 256^3 grids of density 0.02, 0.3 and 0.9, where no source chunk can be skipped.  reach's time includes the host's
read-back of the changed words, once per batch of 16 rounds."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from openobj_amd import map_points, map_volume, ops  # noqa: E402
import mappoints_bench  # noqa: E402

WINDOW_S = 0.3
INF64 = 1 << 40
ABSENT = (0x7FFFFFFF << 32) | 0xFFFFFFFF


def timed(fn, reps):
    """-> (median, min, max) ms per call: device events around windows of calls, each about WINDOW_S long."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    inner = max(1, int(np.ceil(WINDOW_S / max(time.perf_counter() - t0, 1e-6))))
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ts)), float(min(ts)), float(max(ts)), inner


# ------------------------------------------------------------------------------------------- the definitions in torch
def torch_project(label, axis):
    ax = 2 - axis
    occ = label >= 0
    first = occ.to(torch.uint8).argmax(dim=ax, keepdim=True)
    return torch.where(occ.any(dim=ax, keepdim=True), label.gather(ax, first), torch.full_like(first, -1, dtype=torch.int32)).to(torch.int32)


def torch_clearance(label, budget=1 << 27):
    """Three passes of min over the line of key + (d * d << 32) on packed int64 keys, in chunks of `budget` elements."""
    nz, ny, nx = label.shape
    idx = torch.arange(nz * ny * nx, device=label.device, dtype=torch.int64).view(nz, ny, nx)
    key = torch.where(label >= 0, idx, torch.full_like(idx, ABSENT))
    for ax in (2, 1, 0):
        n = key.shape[ax]
        k = key.movedim(ax, -1).reshape(-1, n)
        i = torch.arange(n, device=label.device, dtype=torch.int64)
        dd = ((i[:, None] - i[None, :]) ** 2) << 32
        out = torch.empty_like(k)
        rows = max(1, budget // (n * n))
        for r0 in range(0, k.shape[0], rows):
            kk = k[r0:r0 + rows]
            cand = torch.where((kk == ABSENT)[:, None, :], kk[:, None, :], kk[:, None, :] + dd[None])
            out[r0:r0 + rows] = cand.min(dim=2).values
        shape = list(key.movedim(ax, -1).shape)
        key = out.view(shape).movedim(-1, ax).contiguous()
    return (key >> 32).to(torch.int32), (key & 0xFFFFFFFF).to(torch.int32).where(key != ABSENT, torch.tensor(-1, dtype=torch.int32, device=label.device))


def torch_reach(label, dist2, r2, start, check_every=16):
    """Sweeps of cost = min(cost, shifted cost + w) over the 26 shifts until a sweep changes nothing -> (cost, sweeps)."""
    nz, ny, nx = label.shape
    trav = (label < 0) & (dist2 >= r2)
    cost = torch.full((nz, ny, nx), INF64, dtype=torch.int64, device=label.device)
    cost.view(-1)[start] = 0
    sweeps = 0
    while True:
        before = cost.clone()
        for _ in range(check_every):
            p = torch.nn.functional.pad(cost, (1, 1, 1, 1, 1, 1), value=INF64)
            best = cost
            for dx, dy, dz in map_volume.NEIGHBOURS:
                w = 2 + abs(dx) + abs(dy) + abs(dz)
                best = torch.minimum(best, p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx] + w)
            cost = torch.where(trav, best, cost)
            sweeps += 1
        if torch.equal(before, cost):
            break
    return torch.where(cost >= INF64, torch.full_like(cost, -1), cost).to(torch.int32), sweeps


def torch_goals(label, dist2, site, cost, r2, K):
    n = label.numel()
    lab, d2, st, c = label.view(-1), dist2.view(-1), site.view(-1), cost.view(-1)
    ok = (lab < 0) & (d2 >= r2) & (c != -1) & (st >= 0)
    k = lab[st.clamp(min=0).long()].long()
    ok &= (k >= 0) & (k < K)
    key = (d2.long() << 32) | torch.arange(n, device=label.device, dtype=torch.int64)
    table = torch.full((K,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=label.device)
    table.scatter_reduce_(0, k[ok], key[ok], reduce="amin")
    return torch.where(table == torch.iinfo(torch.int64).max, torch.full_like(table, -1), table)


def fmt(what, t, base=None, extra=""):
    s = f"{what:<28s} {t[0]:10.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]  x{t[3]}"
    if base is not None:
        s += f"   torch {base[0]:10.3f} ms  [{base[1]:.3f}, {base[2]:.3f}]  x{base[3]}   torch / kernel {base[0] / t[0]:.2f}"
    return s + extra


def dense_clearance(side, dev, reps, lines):
    """clearance alone on seeded random grids: the map above is sparse, which lets the passes skip most source chunks; at
    these densities every chunk holds a site and the brute force runs in full."""
    lines.append(f"== clearance on random {side}^3 grids (a voxel occupied with the given probability, seed 1)")
    for density in (0.02, 0.3, 0.9):
        g = torch.Generator(device=dev).manual_seed(1)
        occ = torch.rand(side, side, side, device=dev, generator=g) < density
        label = torch.where(occ, 0, -1).to(torch.int32)
        vol = map_volume.MapVolume(None, (0, 0, 0), 1.0, (side,) * 3, device=dev, label=label, obj_ids=[0])
        d2, site = vol.clearance()
        td2, tsite = torch_clearance(label)
        assert torch.equal(d2, td2) and torch.equal(site, tsite), "clearance: torch differs"
        del td2, tsite
        lines.append(fmt(f"clearance, density {density}", timed(vol.clearance, reps), timed(lambda: torch_clearance(label), 2)))
        print(lines[-1], flush=True)


# --------------------------------------------------------------------------------------------------------------- a grid
def run_grid(name, vol, radius, reps, lines, scipy_edt):
    nx, ny, nz = vol.dims
    label = vol.label
    occ = int((label >= 0).sum())
    lines.append(f"== {name}: {nx} x {ny} x {nz} = {vol.n_voxels} voxels of {float(vol.voxel):.5f} m, {occ} occupied "
                 f"({100.0 * occ / vol.n_voxels:.2f} %)")

    def row(what, t, base=None, extra=""):
        lines.append(fmt(what, t, base, extra))
        print(lines[-1], flush=True)

    # clearance
    d2, site = vol.clearance()
    td2, tsite = torch_clearance(label)
    assert torch.equal(d2, td2) and torch.equal(site, tsite), "clearance: torch differs"
    del td2, tsite
    row("clearance", timed(vol.clearance, reps), timed(lambda: torch_clearance(label), max(2, reps // 2)))
    if scipy_edt is not None:
        host = (label < 0).cpu().numpy()
        t0 = time.perf_counter()
        d = scipy_edt(host)
        dt = time.perf_counter() - t0
        if occ:
            assert np.array_equal(np.rint(d * d).astype(np.int64), d2.cpu().numpy().astype(np.int64)), "clearance: scipy differs"
        lines.append(f"{'  scipy edt (host, once)':<28s} {dt * 1e3:10.1f} ms   squared distances equal")
    # reach: from the most open voxel
    r2 = map_volume.radius_to_r2(radius, float(vol.voxel))
    open_d2 = torch.where(label < 0, d2, torch.full_like(d2, -1))
    start = int(open_d2.view(-1).argmax())
    start_pt = vol.position([start])[0]
    stats = {}
    cost = vol.reach(start_pt, radius, stats=stats)
    assert vol.start_voxel == start
    tcost, sweeps = torch_reach(label, d2, r2, start)
    assert torch.equal(cost, tcost), "reach: torch differs"
    del tcost
    reached = int((cost != -1).sum())
    row("reach", timed(lambda: vol.reach(start_pt, radius), reps), timed(lambda: torch_reach(label, d2, r2, start), 2),
        f"   r2 {r2}, {stats['rounds']} rounds in {stats['batches']} batches (cap {stats['round_cap']}), torch {sweeps} sweeps, "
        f"{reached} of {stats['traversable']} traversable voxels reached, max cost {int(vol.cost_u32().max(initial=0, where=vol.cost_u32() != 0xFFFFFFFF))}")
    # goals
    K = vol.K
    table = ops.volume_goals(label, d2, site, cost, vol.dims, r2, K)
    assert torch.equal(table, torch_goals(label, d2, site, cost, r2, K)), "goals: torch differs"
    g = vol.goals()
    row("goals", timed(lambda: ops.volume_goals(label, d2, site, cost, vol.dims, r2, K), reps),
        timed(lambda: torch_goals(label, d2, site, cost, r2, K), reps), f"   {int((g['voxel'] >= 0).sum())} of {K} objects have a goal")
    # paths: to every goal
    gv = g["voxel"][g["voxel"] >= 0]
    if len(gv):
        paths = vol.paths(gv)
        cap = max(len(p) for p in paths)
        row("paths", timed(lambda: vol.paths_raw(gv, cap), reps), None,
            f"   {len(gv)} walks, {min(len(p) for p in paths)} .. {cap} voxels")
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapvolume_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.25)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--slab", type=int, default=1024)
    ap.add_argument("--band", type=int, default=16, help="z-planes of the slab before it is projected")
    a = ap.parse_args()
    dev = "cuda:0"
    try:
        from scipy.ndimage import distance_transform_edt as scipy_edt
    except ImportError:
        scipy_edt = None
    objects = mappoints_bench.make_map(dev)
    with torch.no_grad():                     # (see the docstring: the background is evaluated, and occupies nothing)
        objects[0].trainer.fc_occ_map.out_alpha.bias.fill_(-1.0)
    mp = map_points.MapPoints(objects, device=dev)
    lo, hi = mappoints_bench.room(objects)
    side = float((hi - lo).max())
    lines = [f"map: {mp.K} objects, room {np.round(lo, 3).tolist()} .. {np.round(hi, 3).tolist()}, robot radius {a.radius} m, "
             f"{torch.cuda.get_device_name(0)}",
             "pass: median ms per call [min, max] over windows of xN calls (device events)"]

    def voxelised(origin, voxel, dims, what):
        vol = map_volume.MapVolume(mp, origin, voxel, dims)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vol.voxelise()
        torch.cuda.synchronize()
        lines.append(f"voxelise {what}: {(time.perf_counter() - t0) * 1e3:.1f} ms (once, host clock; MapPoints.label on "
                     f"{vol.n_voxels} centres in slabs of {map_volume.SLAB_POINTS})")
        return vol

    vol = voxelised(lo, side / a.side, (a.side,) * 3, "cube")
    run_grid("cube", vol, a.radius, a.reps, lines, scipy_edt)
    del vol
    torch.cuda.empty_cache()
    dense_clearance(a.side, dev, a.reps, lines)
    vox = side / a.slab
    vol = voxelised(lo, vox, (a.slab, a.slab, a.band), "slab")
    label = vol.label
    flat = vol.project(2)
    assert torch.equal(flat.label, torch_project(label, 2)), "project: torch differs"
    t, tb = timed(lambda: vol.project(2), a.reps), timed(lambda: torch_project(label, 2), a.reps)
    lines.append(f"{'project z (1024 x 1024 x 16)':<28s} {t[0]:10.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]  x{t[3]}   torch {tb[0]:10.3f} ms  "
                 f"[{tb[1]:.3f}, {tb[2]:.3f}]  x{tb[3]}   torch / kernel {tb[0] / t[0]:.2f}")
    del vol
    run_grid("projected slab", flat, a.radius, a.reps, lines, scipy_edt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
