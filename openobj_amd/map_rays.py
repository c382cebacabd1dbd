"""Rays against the exported map: what an arbitrary ray first hits, and whether two points see each other, on the GPU
over the meshes of map_vis.pkl.gz (objnerf_maprays.hip).  The reference has no counterpart.

    python -m openobj_amd.map_rays cast --logdir DIR [--compact] (--rays FILE.npy | --lidar T.txt --beams N_AZ N_EL EL_MIN
        EL_MAX) [--t-min A --t-max B] [--mode rgb ...] [--hide ceiling ...] --out DIR
    python -m openobj_amd.map_rays sight --logdir DIR [--compact] --nav nav.json [--eye-height H --up-axis K]
        [--hide ...] --out DIR

cast: FILE.npy holds [N, 6] rows (origin, direction); --lidar takes one 4 x 4 sensor-to-world matrix and casts n_az x n_el
beams between the elevations el_min and el_max (degrees).  It writes hits.npz (MapRays.cast's arrays) and hits.ply (the
hit points, coloured by --mode as map_query colours the map).  sight: reads the goals that map_volume wrote into nav.json
and adds, per object with a goal, whether the goal position raised by H along the up axis sees the object's nearest
vertex; it writes sight.json.  Every argument is checked before the device is touched.

The result of a ray is defined without the hierarchy and equals a plain numpy specification (tests/maprays_util.py):
one slab sequence, one Moeller-Trumbore sequence, the minimum of (bits of the fp32 t << 32 | face).  Directions are not
normalised: t is in units of d.  Moeller-Trumbore in floating point is not watertight: a ray exactly through a shared
edge may in principle miss both neighbours."""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, Optional

import numpy as np

LEAF = 4                                # faces per leaf: an ASSUMED default


# ---------------------------------------------------------------------------------------------------- ray generators
def _pose(T, what):
    T = np.asarray(T, np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError(f"{what}: a finite 4 x 4 matrix, got {T.shape}")
    return T


def view_rays(T_WC, intrinsics, W: int, H: int):
    """The rasteriser's sample points as rays: T_WC [4, 4] camera to world, intrinsics (fx, fy, cx, cy) -> (origins,
    dirs) fp64 [W H, 3], pixel (i, j) at row i H + j; d = R ((i - cx) / fx, (j - cy) / fy, 1), so t is the depth along
    the optical axis."""
    T = _pose(T_WC, "view_rays: T_WC")
    intr = [np.float64(x) for x in intrinsics]
    W, H = int(W), int(H)
    if len(intr) != 4 or W < 1 or H < 1 or not (intr[0] != 0 and intr[1] != 0):
        raise ValueError("view_rays: intrinsics (fx, fy, cx, cy) with fx, fy != 0, W, H >= 1")
    fx, fy, cx, cy = intr
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="ij")
    x, y = ((i - cx) / fx).reshape(-1), ((j - cy) / fy).reshape(-1)
    R = T[:3, :3]
    d = np.stack([(R[k, 0] * x + R[k, 1] * y) + R[k, 2] for k in range(3)], axis=1)
    return np.broadcast_to(T[:3, 3], d.shape).copy(), d


def lidar_rays(T_WS, n_az: int, n_el: int, el_min: float, el_max: float):
    """A spinning lidar at the pose T_WS [4, 4] (sensor to world; x forward, z up): n_az azimuths 2 pi a / n_az, n_el
    elevations from el_min to el_max (degrees, both included; n_el = 1: el_min) -> (origins, dirs) fp64 [n_az n_el, 3],
    beam (a, e) at row a n_el + e; the directions have unit length in the sensor frame, so t is the range."""
    T = _pose(T_WS, "lidar_rays: T_WS")
    n_az, n_el = int(n_az), int(n_el)
    if n_az < 1 or n_el < 1 or not (-90.0 <= float(el_min) <= float(el_max) <= 90.0):
        raise ValueError("lidar_rays: n_az, n_el >= 1 and -90 <= el_min <= el_max <= 90 (degrees)")
    az = 2.0 * np.pi * np.arange(n_az, dtype=np.float64) / n_az
    el = np.deg2rad(np.linspace(float(el_min), float(el_max), n_el) if n_el > 1 else np.array([float(el_min)]))
    a, e = np.meshgrid(az, el, indexing="ij")
    s = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1).reshape(-1, 3)
    d = s @ T[:3, :3].T
    return np.broadcast_to(T[:3, 3], d.shape).copy(), d


def _rays(a, what):
    a = np.ascontiguousarray(np.asarray(a, np.float64))
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{what}: fp64 [N, 3], got {a.shape}")
    return a


# ------------------------------------------------------------------------------------------------------- the device side
class MapRays:
    """First hit and line of sight against a MapQuery's meshes.  The hierarchy is built once, here."""

    def __init__(self, mq, leaf: int = LEAF, pad: Optional[float] = None, dataset_name: Optional[str] = None,
                 scene_name: str = "room_0"):
        """mq: a query.MapQuery (dense or compact).  leaf: faces per leaf (a private knob: the results do not depend on
        it).  pad: how far every face's box is grown (None: 2^-20 times the largest finite extent of the vertices)."""
        from . import ops
        self.mq, self.dev = mq, mq.dev
        self.dataset_name, self.scene_name = dataset_name, scene_name
        self.leaf = int(leaf)
        if self.leaf < 1:
            raise ValueError(f"MapRays: leaf {leaf}: at least 1")
        verts, faces, face_off, _ = mq.mesh_buffers()
        self.pad = ops.rays_default_pad(verts) if pad is None else float(pad)
        if not (self.pad >= 0.0 and np.isfinite(self.pad)):
            raise ValueError(f"MapRays: pad {pad} must be finite and not negative")
        self.ws, self.build_status = ops.rays_build(verts, faces, face_off, self.pad, self.leaf)

    def _window(self, w, n, name):
        import torch
        if np.ndim(w) == 0:
            return float(w)
        w = np.ascontiguousarray(np.asarray(w, np.float64))
        if w.shape != (n,):
            raise ValueError(f"MapRays.cast: {name}: a number or [{n}] values, got {w.shape}")
        if name == "t_min" and not (w >= 0.0).all():
            raise ValueError("MapRays.cast: t_min must not be negative")
        return torch.from_numpy(w).to(self.dev)

    def cast(self, origins, dirs, t_min=0.0, t_max=float("inf"), hide=(), ids="obj", any_hit: bool = False,
             to_host: bool = True, _fixed_order: Optional[bool] = None) -> Dict:
        """origins, dirs [N, 3] (d is not normalised; t is in units of d); the window t_min >= 0 .. t_max: numbers, or one
        value per ray.  hide, ids: what MapRaster.render takes.  -> dict(hit bool [N], t fp32 [N] (inf), face, winner
        (the object's position), maskid, vertex int32 [N] (-1; maskid 0), bary fp64 [N, 2], point, normal fp64 [N, 3]
        (NaN; the normal has unit length and faces the ray's origin), stats {name: count} (ops.RAYS_STATS), status).
        vertex is the row of MapQuery.features, of the colour arrays and of PartRegions.label.  any_hit: only hit, stats
        and status (the walk stops at the first hit found).  to_host=False: device tensors, the normal unnormalised.
        _fixed_order: the traversal order, which decides no result (None: the nearer child first for the first hit, the
        fixed order for any-hit, each the faster of the two as measured: profiles/maprays_bench.txt)."""
        import torch
        from . import map_raster, ops
        mq, dev = self.mq, self.dev
        o, d = _rays(origins, "MapRays.cast: origins"), _rays(dirs, "MapRays.cast: dirs")
        if o.shape != d.shape:
            raise ValueError(f"MapRays.cast: {o.shape[0]} origins for {d.shape[0]} directions")
        n = o.shape[0]
        t0, t1 = self._window(t_min, n, "t_min"), self._window(t_max, n, "t_max")
        if isinstance(t0, float) and not t0 >= 0.0:
            raise ValueError(f"MapRays.cast: t_min {t0} must not be negative")
        if isinstance(t1, float) and t1 != t1:
            raise ValueError("MapRays.cast: t_max is a NaN")
        hide_m = map_raster.hide_mask(mq, hide, self.dataset_name, self.scene_name, "MapRays")
        ids_v = map_raster.ids_of(mq, ids, "MapRays")
        verts, faces, face_off, _ = mq.mesh_buffers()
        od, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        if _fixed_order is None:
            _fixed_order = bool(any_hit)
        key, stats, status = ops.rays_cast(verts, faces, face_off, torch.from_numpy(hide_m).to(dev), self.ws, self.pad, od, dd,
                                           t0, t1, self.leaf, any_hit, self.build_status.clone(), _fixed_order)
        if any_hit:
            out = {"hit": key != 0}
        else:
            out = ops.rays_resolve(verts, faces, face_off, torch.from_numpy(ids_v).to(dev), od, dd, key)
            out["hit"] = out["hit"] != 0
            out["key"] = key
        out.update(stats=stats, status=status)
        if not to_host:
            return out
        res = {k: v.cpu().numpy() for k, v in out.items() if k != "key"}
        res["stats"] = dict(zip(ops.RAYS_STATS, (int(x) for x in res["stats"])))
        res["status"] = int(res["status"][0])
        if not any_hit:
            with np.errstate(all="ignore"):
                res["normal"] = res["normal"] / np.linalg.norm(res["normal"], axis=1, keepdims=True)
        return res

    def occluded(self, a, b, hide=()) -> np.ndarray:
        """bool [N]: does anything lie on the segment a -> b (both [N, 3])?  Any-hit with d = b - a, window [0, 1]."""
        a, b = _rays(a, "MapRays.occluded: a"), _rays(b, "MapRays.occluded: b")
        if a.shape != b.shape:
            raise ValueError("MapRays.occluded: as many a as b")
        return self.cast(a, b - a, 0.0, 1.0, hide=hide, any_hit=True)["hit"]

    def sees(self, eyes, targets, objects, hide=()) -> np.ndarray:
        """bool [N]: the first hit on the segment eyes[n] -> targets[n] is none, or belongs to the object at position
        objects[n]: the robot at a goal sees the thing it came for, not the wall in front of it."""
        a, b = _rays(eyes, "MapRays.sees: eyes"), _rays(targets, "MapRays.sees: targets")
        obj = np.asarray(objects, np.int64).reshape(-1)
        if a.shape != b.shape or obj.shape != (a.shape[0],):
            raise ValueError("MapRays.sees: eyes, targets [N, 3] and objects [N]")
        r = self.cast(a, b - a, 0.0, 1.0, hide=hide)
        return ~r["hit"] | (r["winner"] == obj)


# ----------------------------------------------------------------------------------------------------------------- CLI
def write_points_ply(path: str, points, colors) -> None:
    """An ASCII PLY of points fp64 [n, 3] with colours uint8 [n, 3]."""
    p, c = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(colors, np.uint8).reshape(-1, 3)
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\nelement vertex {len(p)}\nproperty double x\nproperty double y\nproperty double z\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        for q, k in zip(p, c):
            fh.write(f"{float(q[0])!r} {float(q[1])!r} {float(q[2])!r} {int(k[0])} {int(k[1])} {int(k[2])}\n")


def sight_records(cast, mq, nav: dict, eye_height: float = 0.0, up_axis: int = 2, hide=()) -> list:
    """The `sight` mode on the host: cast(origins, dirs, t_min, t_max, hide=...) is MapRays.cast (a test passes the
    specification).  Per object of nav["objects"] -> {"id", "eye", "target", "sees", "blocker"}: eye = the goal raised by
    eye_height along up_axis, target = the object's vertex nearest to the eye, sees = the first hit on the segment is
    none or the object itself, blocker = the id of the object hit first where it is another (else None).  Objects
    without a goal, or that the map does not hold, get sees = None."""
    keys = [int(k) for k in mq.keys]
    rows, eyes, tgts, objs = [], [], [], []
    for rec in nav.get("objects", []):
        row = {"id": int(rec["id"]), "eye": None, "target": None, "sees": None, "blocker": None}
        rows.append(row)
        if rec.get("goal") is None or row["id"] not in keys:
            continue
        p = keys.index(row["id"])
        eye = np.asarray(rec["goal"], np.float64).reshape(3).copy()
        eye[up_axis] += float(eye_height)
        v = np.asarray(mq.all_obj[mq.keys[p]]["mesh"].vertices, np.float64).reshape(-1, 3)
        if not len(v) or not np.isfinite(eye).all():
            continue
        tgt = v[int(np.argmin(((v - eye) ** 2).sum(axis=1)))]
        row["eye"], row["target"] = eye.tolist(), tgt.tolist()
        eyes.append(eye), tgts.append(tgt), objs.append((p, row))
    if eyes:
        a, b = np.array(eyes), np.array(tgts)
        r = cast(a, b - a, 0.0, 1.0, hide=hide)
        for n, (p, row) in enumerate(objs):
            w = int(r["winner"][n])
            row["sees"] = bool(not r["hit"][n] or w == p)
            row["blocker"] = None if row["sees"] else keys[w]
    return rows


def _parse(argv):
    from . import map_query, map_raster
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("command", choices=("cast", "sight"))
    map_query.add_map_arguments(ap)
    for act in ap._actions:
        if act.dest == "mode":
            act.required, act.default = False, "rgb"
    ap.add_argument("--rays", help="cast: an .npy file of [N, 6] rows (origin, direction)")
    ap.add_argument("--lidar", help="cast: a text file with one 4 x 4 sensor-to-world matrix")
    ap.add_argument("--beams", nargs=4, type=float, metavar=("N_AZ", "N_EL", "EL_MIN", "EL_MAX"))
    ap.add_argument("--t-min", type=float, default=0.0)
    ap.add_argument("--t-max", type=float, default=float("inf"))
    ap.add_argument("--nav", help="sight: the nav.json of map_volume")
    ap.add_argument("--eye-height", type=float, default=0.0)
    ap.add_argument("--up-axis", type=int, default=2, choices=(0, 1, 2))
    ap.add_argument("--hide", nargs="*", default=[], help="ceiling, most, hidden (MapQuery.hidden_sets) or positions")
    ap.add_argument("--leaf", type=int, default=LEAF)
    a = ap.parse_args(argv)
    if a.leaf < 1:
        ap.error(f"--leaf {a.leaf}: at least 1")
    if a.command == "cast":
        if a.nav is not None:
            ap.error("--nav goes with sight")
        if (a.rays is None) == (a.lidar is None):
            ap.error("cast: either --rays or --lidar")
        if not a.t_min >= 0.0 or a.t_max != a.t_max or a.t_max < a.t_min:
            ap.error(f"--t-min {a.t_min} --t-max {a.t_max}: 0 <= t_min <= t_max")
        if a.rays is not None:
            if a.beams is not None:
                ap.error("--beams goes with --lidar")
            if not os.path.isfile(a.rays):
                ap.error(f"--rays: no such file {a.rays}")
            r = np.load(a.rays)
            if r.ndim != 2 or r.shape[1] != 6:
                ap.error(f"--rays: {a.rays} holds {r.shape}, rays are [N, 6]")
            a.origins, a.dirs = np.ascontiguousarray(r[:, :3], np.float64), np.ascontiguousarray(r[:, 3:], np.float64)
        else:
            if a.beams is None:
                ap.error("--lidar needs --beams n_az n_el el_min el_max")
            if not os.path.isfile(a.lidar):
                ap.error(f"--lidar: no such file {a.lidar}")
            if a.beams[0] != int(a.beams[0]) or a.beams[1] != int(a.beams[1]):
                ap.error("--beams: n_az and n_el are whole numbers")
            try:
                a.origins, a.dirs = lidar_rays(map_raster.load_pose(a.lidar), int(a.beams[0]), int(a.beams[1]), a.beams[2],
                                               a.beams[3])
            except ValueError as e:
                ap.error(str(e))
    else:
        if a.rays is not None or a.lidar is not None or a.beams is not None:
            ap.error("--rays, --lidar and --beams go with cast")
        if a.nav is None or not os.path.isfile(a.nav):
            ap.error(f"sight needs --nav: no such file {a.nav}")
        try:
            with open(a.nav) as fh:
                a.nav_doc = json.load(fh)
        except ValueError as e:
            ap.error(f"--nav: {a.nav}: {e}")
        if not isinstance(a.nav_doc, dict) or not isinstance(a.nav_doc.get("objects"), list):
            ap.error(f"--nav: {a.nav} has no list of objects: is it map_volume's nav.json?")
        if not np.isfinite(a.eye_height):
            ap.error(f"--eye-height {a.eye_height} must be finite")
    named = [h for h in a.hide if not h.lstrip("-").isdigit()]
    for h in named:
        if h not in ("ceiling", "most", "hidden"):
            ap.error(f"--hide {h}: ceiling, most, hidden or positions")
    if named and not a.dataset:
        ap.error(f"--hide {named[0]} needs --dataset")
    all_obj, queries = map_query.check_map_arguments(ap, a)
    for h in a.hide:
        if h not in named and not 0 <= int(h) < len(all_obj):
            ap.error(f"--hide {h}: positions in [0, {len(all_obj)})")
    return a, all_obj, queries


def main(argv=None):
    a, all_obj, q = _parse(argv)
    from . import map_query
    from . import query as oquery
    mq = oquery.MapQuery(all_obj, a.device)
    mr = MapRays(mq, a.leaf, dataset_name=a.dataset, scene_name=a.scene)
    os.makedirs(a.out, exist_ok=True)
    if a.command == "sight":
        doc = {"nav": a.nav, "eye_height": a.eye_height, "up_axis": a.up_axis,
               "objects": sight_records(mr.cast, mq, a.nav_doc, a.eye_height, a.up_axis, a.hide)}
        with open(os.path.join(a.out, "sight.json"), "w") as fh:
            json.dump(doc, fh, indent=1)
        seen = sum(1 for o in doc["objects"] if o["sees"])
        print(f"{seen} of {len(doc['objects'])} objects seen from their goals")
        return doc
    r = mr.cast(a.origins, a.dirs, a.t_min, a.t_max, hide=a.hide)
    np.savez(os.path.join(a.out, "hits.npz"), origins=a.origins, dirs=a.dirs, status=r["status"],
             stats=np.array(list(r["stats"].values()), np.int64),
             **{k: r[k] for k in ("hit", "t", "face", "winner", "maskid", "vertex", "bary", "point", "normal")})
    colors = map_query.colors_for_mode(mq, a.mode, q, a.top, a.color_yaml).cpu().numpy()
    hit = r["hit"]
    rgb = np.round(np.clip(colors[r["vertex"][hit]].astype(np.float64), 0.0, 1.0) * 255).astype(np.uint8)
    write_points_ply(os.path.join(a.out, "hits.ply"), r["point"][hit], rgb)
    print(f"{int(hit.sum())} of {len(hit)} rays hit; {r['stats']['node_visits'] / max(len(hit), 1):.1f} node visits, "
          f"{r['stats']['face_tests'] / max(len(hit), 1):.1f} face tests a ray")
    return r


__all__ = ["MapRays", "view_rays", "lidar_rays", "sight_records", "write_points_ply", "LEAF"]

if __name__ == "__main__":
    main()
