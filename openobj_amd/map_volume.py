"""A navigation volume of the map on the GPU: where can a robot of a given radius stand, how far is every such place from
a start, and where does it come closest to each object?

    python -m openobj_amd.map_volume --logdir DIR --voxel V [--bounds x0 y0 z0 x1 y1 z1] [--project-axis A]
                                     [--radius R --start X Y Z [--goal-ids ...]] --out DIR

The grid is axis-aligned in world coordinates: origin fp32 [3], voxel fp32 (metres), dims = (nx, ny, nz); the linear index of
voxel (x, y, z) is idx = (z * ny + y) * nx + x and its centre, per component, origin + (float(i) + 0.5f) * voxel in fp32.
Everything stored per voxel is an integer with exactly one right value (objnerf_mapvolume.hip):

* label int32 [nz, ny, nx]   MapPoints.label of the centre: the position in the object list, -1 where nothing is occupied.
                             OCCUPIED iff label >= 0; the background counts (its walls and floor are obstacles);
* dist2, site int32          clearance(): the smallest dx^2 + dy^2 + dz^2 (voxel units) to an occupied voxel and that voxel's
                             linear index, the LOWEST index among several at that distance; INT32_MAX / -1 on an empty grid;
* cost uint32                reach(start, radius): the length of the shortest 26-connected path (3 / 4 / 5 for a face / edge /
                             corner move) from the start voxel through TRAVERSABLE voxels -- not occupied and
                             dist2 >= r2 = ceil((radius / voxel)^2) -- 0xFFFFFFFF where there is none;
* goals()                    voxel u FACES object k iff label[site[u]] == k; the goal of k is the reached voxel facing it with
                             the smallest (dist2, idx);
* paths(goal_voxels)         the voxels from each goal back to the start: the predecessor of u is the first neighbour v in
                             NEIGHBOURS that is traversable and has cost[v] + w(v, u) == cost[u].

project(axis) collapses an axis (a column is occupied iff any voxel in it is, its label the first occupied one's): the 2-D
case for ground robots, the grid's extent along the axis being the robot's body band.

The CLI writes volume.npz and, with --radius, nav.json: per requested object (or every object) its id, class, goal
position, clearance in metres, path cost and the path's polyline from the start to the goal."""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, ops

INF_COST = 0xFFFFFFFF
INT32_MAX = 2 ** 31 - 1
SLAB_POINTS = 1 << 20                  # voxel centres per MapPoints.label call of voxelise()
# the order in which a path tries the neighbours of a voxel: (dx, dy, dz), dz slowest, dx fastest, the centre left out
NEIGHBOURS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def grid_from_boxes(centers, rotations, extents, voxel: float, pad: float = 0.0):
    """The axis-aligned hull of the corners c + R (+-e / 2) of all boxes, grown by pad and rounded outwards to whole voxels,
    in fp64 -> (origin fp64 [3], dims).  The grid's origin is a whole multiple of the voxel."""
    voxel = float(voxel)
    if not voxel > 0 or pad < 0:
        raise _lib.ObjnerfError(f"map volume: voxel = {voxel}, pad = {pad}")
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for c, R, e in zip(centers, rotations, extents):
        c, R, e = np.asarray(c, np.float64).reshape(3), np.asarray(R, np.float64).reshape(3, 3), np.asarray(e, np.float64).reshape(3)
        corners = c[None, :] + (signs * (0.5 * e)[None, :]) @ R.T
        lo, hi = np.minimum(lo, corners.min(0)), np.maximum(hi, corners.max(0))
    if not np.all(np.isfinite(lo)):
        raise _lib.ObjnerfError("map volume: no box")
    i0 = np.floor((lo - pad) / voxel)
    i1 = np.ceil((hi + pad) / voxel)
    dims = tuple(int(v) for v in np.maximum(i1 - i0, 1))
    return i0 * voxel, ops.volume_check_dims(dims)


def grid_from_bounds(bounds, voxel: float):
    """bounds = x0 y0 z0 x1 y1 z1 -> (origin fp64 [3], dims): the upper side rounded outwards to whole voxels."""
    b = np.asarray(bounds, np.float64).reshape(-1)
    voxel = float(voxel)
    if b.shape != (6,) or not voxel > 0 or not np.all(b[3:] > b[:3]):
        raise _lib.ObjnerfError(f"map volume: bounds {b.tolist()} (x0 y0 z0 x1 y1 z1, upper > lower), voxel {voxel}")
    dims = tuple(int(v) for v in np.maximum(np.ceil((b[3:] - b[:3]) / voxel), 1))
    return b[:3].copy(), ops.volume_check_dims(dims)


def radius_to_r2(radius: float, voxel: float) -> int:
    """ceil((radius / voxel)^2) in fp64: a voxel is far enough from every obstacle iff dist2 >= r2."""
    radius, voxel = float(radius), float(voxel)
    if not radius >= 0 or not voxel > 0:
        raise _lib.ObjnerfError(f"map volume: radius = {radius}, voxel = {voxel}")
    r2 = math.ceil((radius / voxel) ** 2)
    if r2 > INT32_MAX:
        raise _lib.ObjnerfError(f"map volume: radius {radius} is {radius / voxel:.0f} voxels: r2 does not fit 31 bits")
    return int(r2)


def centres_host(origin, voxel, dims, index) -> np.ndarray:
    """The fp32 centres of the voxels `index` (linear), as the kernel computes them."""
    nx, ny, nz = dims
    idx = np.asarray(index, np.int64).reshape(-1)
    ijk = np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], axis=1).astype(np.float32)
    return np.asarray(origin, np.float32)[None, :] + (ijk + np.float32(0.5)) * np.float32(voxel)


class MapVolume:
    def __init__(self, mp, origin, voxel: float, dims: Sequence[int], device=None, label=None, obj_ids=None,
                 class_ids=None):
        """mp: a map_points.MapPoints (None for a volume that is loaded or given its labels).  label: int32 [nz, ny, nx]."""
        self.dims = ops.volume_check_dims(dims)
        self.voxel = np.float32(voxel)
        if not float(self.voxel) > 0:
            raise _lib.ObjnerfError(f"MapVolume: voxel = {voxel}")
        self.origin = np.asarray(origin, np.float64).reshape(-1).astype(np.float32)
        if self.origin.shape != (3,) or not np.all(np.isfinite(self.origin)):
            raise _lib.ObjnerfError(f"MapVolume: origin {origin}")
        self.mp = mp
        self.device = torch.device(device if device is not None else (mp.device if mp is not None else "cuda:0"))
        if mp is not None:
            obj_ids, class_ids = mp.obj_ids.cpu().numpy(), mp.class_ids.cpu().numpy()
        self.obj_ids = np.zeros(0, np.int64) if obj_ids is None else np.asarray(obj_ids, np.int64).reshape(-1)
        self.class_ids = np.full(len(self.obj_ids), -1, np.int64) if class_ids is None else np.asarray(class_ids, np.int64).reshape(-1)
        if self.class_ids.shape != self.obj_ids.shape:
            raise _lib.ObjnerfError("MapVolume: obj_ids and class_ids differ in length")
        self.label = self.dist2 = self.site = self.cost = None
        self.r2 = self.start_voxel = None
        if label is not None:
            self.set_label(label)

    # ------------------------------------------------------------------------------------------------------ the grid
    @property
    def shape(self):
        return (self.dims[2], self.dims[1], self.dims[0])

    @property
    def n_voxels(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    @property
    def K(self) -> int:
        """Rows of the goal table: the objects of the list, or what the labels need."""
        return max(len(self.obj_ids), 1)

    @classmethod
    def from_logdir(cls, logdir: str, voxel: float, bounds=None, pad: float = 0.0, device="cuda:0", bg_ids=(0,)):
        from . import map_points
        mp = map_points.MapPoints.from_logdir(logdir, device, bg_ids=bg_ids)
        return cls.from_map(mp, voxel, bounds=bounds, pad=pad)

    @classmethod
    def from_map(cls, mp, voxel: float, bounds=None, pad: float = 0.0):
        if bounds is not None:
            origin, dims = grid_from_bounds(bounds, voxel)
        else:
            origin, dims = grid_from_boxes([o.bbox.center for o in mp.objects], [o.bbox.R for o in mp.objects],
                                           [o.bbox.extent for o in mp.objects], voxel, pad)
        return cls(mp, origin, voxel, dims)

    def set_label(self, label) -> None:
        label = torch.as_tensor(label)
        if tuple(label.shape) != self.shape:
            raise _lib.ObjnerfError(f"MapVolume: label {tuple(label.shape)} for a grid of {self.shape}")
        self.label = label.to(self.device, torch.int32).contiguous()
        self.dist2 = self.site = self.cost = None
        self.r2 = self.start_voxel = None

    def centres(self, z0: int = 0, nzs: Optional[int] = None) -> torch.Tensor:
        """The centres [nzs * ny * nx, 3] of a slab of z-planes, on the device."""
        nzs = self.dims[2] - z0 if nzs is None else nzs
        return ops.volume_centres(self.dims, self.origin, float(self.voxel), z0, nzs, self.device)

    def position(self, index) -> np.ndarray:
        return centres_host(self.origin, self.voxel, self.dims, index)

    def voxel_of(self, point) -> int:
        """The voxel that holds a world point (fp64 floor), -1 outside the grid."""
        p = np.asarray(point, np.float64).reshape(-1)
        if p.shape != (3,) or not np.all(np.isfinite(p)):
            raise _lib.ObjnerfError(f"MapVolume: point {point}")
        ijk = np.floor((p - self.origin.astype(np.float64)) / float(self.voxel)).astype(np.int64)
        if np.any(ijk < 0) or np.any(ijk >= np.asarray(self.dims)):
            return -1
        return int((ijk[2] * self.dims[1] + ijk[1]) * self.dims[0] + ijk[0])

    def voxelise(self, slab_points: int = SLAB_POINTS) -> torch.Tensor:
        """label [nz, ny, nx] through MapPoints.label, a slab of z-planes at a time: the cloud of all centres never exists."""
        if self.mp is None:
            raise _lib.ObjnerfError("MapVolume.voxelise: this volume has no map (it was loaded or given its labels)")
        nx, ny, nz = self.dims
        step = max(1, int(slab_points) // (nx * ny))
        label = torch.empty(self.shape, dtype=torch.int32, device=self.device)
        for z0 in range(0, nz, step):
            n = min(step, nz - z0)
            label[z0:z0 + n] = self.mp.label(self.centres(z0, n))["obj"].view(n, ny, nx)
        self.set_label(label)
        return self.label

    def _need(self, what: str, attr: str):
        v = getattr(self, attr)
        if v is None:
            raise _lib.ObjnerfError(f"MapVolume.{what}: call {'voxelise' if attr == 'label' else 'reach'}() first")
        return v

    def project(self, axis: int) -> "MapVolume":
        """A new volume with the axis (0 = x, 1 = y, 2 = z) collapsed to length 1."""
        label = ops.volume_project(self._need("project", "label"), self.dims, axis)
        dims = list(self.dims)
        dims[axis] = 1
        return MapVolume(None, self.origin, self.voxel, dims, device=self.device, label=label, obj_ids=self.obj_ids,
                         class_ids=self.class_ids)

    # ------------------------------------------------------------------------------------------------------ the passes
    def clearance(self):
        """-> (dist2, site) int32 [nz, ny, nx], kept on the volume."""
        self.dist2, self.site = ops.volume_clearance(self._need("clearance", "label"), self.dims)
        return self.dist2, self.site

    def reach(self, start, radius: float, stats: Optional[dict] = None) -> torch.Tensor:
        """cost [nz, ny, nx] from the voxel that holds the world point `start`, for a robot of `radius` metres: int32
        storage of the unsigned costs (cost_u32() gives them as numpy uint32).  Raises for a start outside the grid or in
        a voxel that is not traversable."""
        label = self._need("reach", "label")
        r2 = radius_to_r2(radius, float(self.voxel))
        u = self.voxel_of(start)
        if u < 0:
            raise _lib.ObjnerfError(f"MapVolume.reach: start {list(np.asarray(start, np.float64))} lies outside the grid")
        if self.dist2 is None:
            self.clearance()
        if int(label.view(-1)[u]) >= 0 or int(self.dist2.view(-1)[u]) < r2:
            raise _lib.ObjnerfError(f"MapVolume.reach: the start voxel {u} is not traversable (label {int(label.view(-1)[u])}, "
                                    f"dist2 {int(self.dist2.view(-1)[u])} < r2 {r2})")
        self.cost = ops.volume_reach(label, self.dist2, self.dims, r2, u, stats=stats)
        self.r2, self.start_voxel = r2, u
        return self.cost

    def cost_u32(self) -> np.ndarray:
        return self._need("cost_u32", "cost").cpu().numpy().view(np.uint32)

    def goals(self) -> dict:
        """After reach(): per object (numpy) voxel int64 [K] (-1: no reached voxel faces it), position fp32 [K, 3] (NaN),
        dist2 int64 [K] (-1) and cost int64 [K] (0xFFFFFFFF)."""
        cost = self._need("goals", "cost")
        table = ops.volume_goals(self.label, self.dist2, self.site, cost, self.dims, self.r2, self.K).cpu().numpy()
        has = table != -1
        key = table.view(np.uint64)
        voxel = np.where(has, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
        dist2 = np.where(has, (key >> np.uint64(32)).astype(np.int64), -1)
        pos = np.full((len(table), 3), np.nan, np.float32)
        cst = np.full(len(table), INF_COST, np.int64)
        if has.any():
            pos[has] = self.position(voxel[has])
            picked = cost.view(-1)[torch.from_numpy(voxel[has]).to(self.device)].cpu().numpy()
            cst[has] = picked.view(np.uint32).astype(np.int64)
        return {"voxel": voxel, "position": pos, "dist2": dist2, "cost": cst}

    def paths_raw(self, goal_voxels, cap: int, out: Optional[torch.Tensor] = None):
        """-> (out int32 [G, cap], len int32 [G]) on the device; len is negative where a path has more than cap voxels."""
        cost = self._need("paths", "cost")
        g = torch.as_tensor(np.asarray(goal_voxels, np.int64).reshape(-1)).to(self.device, torch.int32)
        return ops.volume_paths(self.label, self.dist2, cost, self.dims, self.r2, g, cap, out=out)

    def paths(self, goal_voxels):
        """-> a list of int64 arrays, the voxels from each goal back to the start (empty for a goal that is not reached)."""
        goals = np.asarray(goal_voxels, np.int64).reshape(-1)
        if len(goals) == 0:
            return []
        flat = self.cost_u32().reshape(-1)
        ok = (goals >= 0) & (goals < self.n_voxels)
        c = np.where(ok, flat[np.clip(goals, 0, self.n_voxels - 1)], INF_COST).astype(np.int64)
        cap = int(max(1, (np.where(c == INF_COST, 0, c) // 3 + 2).max()))
        out, ln = self.paths_raw(goals, cap)
        out, ln = out.cpu().numpy(), ln.cpu().numpy()
        if (ln < 0).any():
            raise _lib.ObjnerfError("MapVolume.paths: a path is longer than cost / 3 + 2 voxels: not a volume reach() wrote")
        return [out[i, :ln[i]].astype(np.int64) for i in range(len(goals))]

    # ------------------------------------------------------------------------------------------------------ files
    def save(self, path: str) -> str:
        """volume.npz under `path` (or `path` itself when it ends in .npz): the grid, label, dist2, object and class ids."""
        self._need("save", "label")
        if self.dist2 is None:
            self.clearance()
        if not path.endswith(".npz"):
            os.makedirs(path, exist_ok=True)
            path = os.path.join(path, "volume.npz")
        np.savez_compressed(path, origin=self.origin, voxel=np.float32(self.voxel), dims=np.asarray(self.dims, np.int32),
                            label=self.label.cpu().numpy(), dist2=self.dist2.cpu().numpy(), obj_ids=self.obj_ids,
                            class_ids=self.class_ids)
        return path

    @classmethod
    def load(cls, path: str, device="cuda:0") -> "MapVolume":
        if not path.endswith(".npz"):
            path = os.path.join(path, "volume.npz")
        d = np.load(path)
        v = cls(None, d["origin"], float(d["voxel"]), [int(x) for x in d["dims"]], device=device, label=d["label"],
                obj_ids=d["obj_ids"], class_ids=d["class_ids"])
        if tuple(d["dist2"].shape) != v.shape:
            raise _lib.ObjnerfError(f"MapVolume.load: dist2 {d['dist2'].shape} for a grid of {v.shape}")
        v.dist2 = torch.from_numpy(d["dist2"].astype(np.int32)).to(v.device)       # (site comes back with clearance())
        return v


# ----------------------------------------------------------------------------------------------------------------- CLI
def navigation(vol: MapVolume, goal_ids=None) -> list:
    """After reach(): the nav.json records of the requested object ids (None: every object)."""
    g = vol.goals()
    rows = range(len(vol.obj_ids)) if goal_ids is None else [int(np.nonzero(vol.obj_ids == i)[0][0]) for i in goal_ids]
    rows = list(rows)
    paths = vol.paths([g["voxel"][k] for k in rows])
    out = []
    for k, p in zip(rows, paths):
        has = g["voxel"][k] >= 0
        out.append({"id": int(vol.obj_ids[k]), "class": int(vol.class_ids[k]),
                    "goal": g["position"][k].astype(float).tolist() if has else None,
                    "clearance_m": float(math.sqrt(g["dist2"][k]) * float(vol.voxel)) if has else None,
                    "cost": int(g["cost"][k]) if has else None,
                    "path": vol.position(p[::-1]).astype(float).tolist()})           # from the start to the goal
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--logdir", required=True)
    ap.add_argument("--voxel", type=float, required=True, help="metres")
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--pad", type=float, default=0.0)
    ap.add_argument("--project-axis", type=int, default=None, choices=(0, 1, 2))
    ap.add_argument("--radius", type=float, default=None, help="metres; with --start: reach, goals, paths -> nav.json")
    ap.add_argument("--start", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--goal-ids", type=int, nargs="*", default=None)
    ap.add_argument("--bg-ids", type=int, nargs="*", default=[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not a.voxel > 0:
        ap.error(f"--voxel {a.voxel}: a positive length")
    if a.pad < 0:
        ap.error(f"--pad {a.pad}")
    if (a.radius is None) != (a.start is None):
        ap.error("--radius and --start go together")
    if a.radius is not None and a.radius < 0:
        ap.error(f"--radius {a.radius}")
    if a.goal_ids is not None and a.radius is None:
        ap.error("--goal-ids needs --radius and --start")
    if a.bounds is not None and not all(hi > lo for lo, hi in zip(a.bounds[:3], a.bounds[3:])):
        ap.error("--bounds x0 y0 z0 x1 y1 z1: every upper bound above the lower one")
    return a


def main(argv=None):
    a = parse_args(argv)
    vol = MapVolume.from_logdir(a.logdir, a.voxel, bounds=a.bounds, pad=a.pad, device=a.device, bg_ids=a.bg_ids)
    vol.voxelise()
    if a.project_axis is not None:
        vol = vol.project(a.project_axis)
    vol.clearance()
    os.makedirs(a.out, exist_ok=True)
    vol.save(a.out)
    print(f"grid {vol.dims} at {vol.origin.tolist()}, voxel {float(vol.voxel)}: {int((vol.label >= 0).sum())} occupied voxels")
    if a.radius is not None:
        if a.goal_ids is not None:
            missing = [i for i in a.goal_ids if i not in set(vol.obj_ids.tolist())]
            if missing:
                raise _lib.ObjnerfError(f"--goal-ids: no object {missing} in the map")
        stats = {}
        vol.reach(a.start, a.radius, stats=stats)
        nav = {"start": list(a.start), "radius": a.radius, "r2": vol.r2, "rounds": stats["rounds"],
               "objects": navigation(vol, a.goal_ids)}
        with open(os.path.join(a.out, "nav.json"), "w") as fh:
            json.dump(nav, fh, indent=1)
        print(f"{sum(o['goal'] is not None for o in nav['objects'])} of {len(nav['objects'])} objects reachable, "
              f"{stats['rounds']} rounds")
    return vol


if __name__ == "__main__":
    main()
