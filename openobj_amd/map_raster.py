"""Headless views of the exported map: the meshes of map_vis.pkl.gz rasterised on the GPU under any colouring MapQuery
makes (objnerf_mapraster.hip) -- what the reference's Open3D window shows (vis_interaction.py, keys R, S,
I, O, F, P, H), as images, and the way back from a pixel to a map vertex.

    python -m openobj_amd.map_raster --logdir DIR [--compact] --mode {rgb,class,instance,partfeat,object,part}
        (--config scene.json [--frames a:b:s] | --pose T.txt --size W H --intrinsics fx fy cx cy)
        [--clip-query F.npy --sbert-query F.npy --part-query F.npy --top N --color-yaml PATH --dataset Replica|Scannet
         --scene NAME] [--hide ceiling ...] [--shading none] [--depth-scale S] --out DIR

--mode and the query arguments are map_query's (one dispatch, map_query.colors_for_mode).  --config takes the poses of
the scene's dataset (frame ids as map_view writes them); --pose takes one 4 x 4 camera-to-world matrix from a text file
and writes frame 0.  Per frame rgb_<id>.png, depth_<id>.png and maskid_<id>.png are written through map_view.write_view,
so `python -m openobj_amd.map_view_eval --renders DIR` scores them as they are; visible.json holds, per frame, the objects
seen and their pixel counts, the face counters and the status word.  --hide names sets of MapQuery.hidden_sets (ceiling,
most, hidden; they need --dataset) or positions.  Every argument is checked before the device is touched.

The result of a view is defined by integers and equals a plain Python specification (tests/mapraster_util.py): fixed-point
edge functions, a 64-bit minimum per pixel, one fp64 sequence for the depth.  There is no near-plane clipping: a face
with a corner in front of z_near is dropped (and counted)."""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, Optional, Sequence

import numpy as np

AMBIENT = 0.35                          # the headlight's floor: an ASSUMED value, not a measured one
Z_NEAR = 0.05
BOUND = float(2 ** 25)
NO_DEPTH = 100.0                        # ViewBuffers' and objnerf_view_merge's "nothing painted"
SHADINGS = ("headlight", "none")


# ---------------------------------------------------------------------------------------------------- host arithmetic
def camera_rows(T_WC) -> np.ndarray:
    """T_WC [4, 4] -> the upper 3 x 4 of inverse(T_WC), inverted here in fp64 (as map_cull.world_to_camera does)."""
    T = np.asarray(T_WC, np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError(f"map_raster: T_WC must be a finite 4 x 4 matrix, got {T.shape}")
    return np.ascontiguousarray(np.linalg.inv(T)[:3, :])


def project_vertices(p, T_CW, intrinsics):
    """The vertex sequence of the specification on the host: p fp64 [..., 3] -> (X, Y fp64: floor(u 256 + 0.5), iz fp64,
    zc), every operation one numpy call, so rounded once."""
    p, M = np.asarray(p, np.float64), np.asarray(T_CW, np.float64).reshape(12)
    fx, fy, cx, cy = (np.float64(x) for x in intrinsics)
    with np.errstate(all="ignore"):
        xc, yc, zc = (((M[4 * r] * p[..., 0] + M[4 * r + 1] * p[..., 1]) + M[4 * r + 2] * p[..., 2]) + M[4 * r + 3]
                      for r in range(3))
        X = np.floor(((fx * xc) / zc + cx) * 256.0 + 0.5)
        Y = np.floor(((fy * yc) / zc + cy) * 256.0 + 0.5)
        return X, Y, 1.0 / zc, zc


def pick_points(corners, pixels, T_CW, intrinsics, z_near: float = Z_NEAR):
    """The 3-D point under a pixel from the read-back rows: corners fp64 [n, 3, 3] (the world vertices of the winning
    faces, in the faces' own order), pixels [n, 2] as (w, h) -> (points fp64 [n, 3] = sum b_k p_k, b fp64 [n, 3] in the
    corners' own order); NaN rows where the face is not drawn or does not cover the pixel.  The specification's sequence:
    int64 edge functions of the fixed-point positions, t_k = w_k iz_k, q = (t0 + t1) + t2, b_k = t_k / q."""
    c = np.asarray(corners, np.float64).reshape(-1, 3, 3)
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    n = len(c)
    pts, b = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    if n == 0:
        return pts, b
    X, Y, iz, zc = project_vertices(c, T_CW, intrinsics)
    with np.errstate(invalid="ignore"):
        ok = ((zc >= z_near) & (np.abs(X) <= BOUND) & (np.abs(Y) <= BOUND)).all(axis=1)
    Xi, Yi = np.where(ok[:, None], X, 0).astype(np.int64), np.where(ok[:, None], Y, 0).astype(np.int64)
    A = (Xi[:, 1] - Xi[:, 0]) * (Yi[:, 2] - Yi[:, 0]) - (Yi[:, 1] - Yi[:, 0]) * (Xi[:, 2] - Xi[:, 0])
    sgn = np.where(A < 0, -1, 1)                               # (swapping corners 1 and 2 negates every edge function)
    Px, Py = 256 * px[:, 0], 256 * px[:, 1]

    def E(a, bb):
        return ((Xi[:, bb] - Xi[:, a]) * (Py - Yi[:, a]) - (Yi[:, bb] - Yi[:, a]) * (Px - Xi[:, a])) * sgn

    w = np.stack([E(1, 2), E(2, 0), E(0, 1)], axis=1)
    ok &= (A != 0) & (w >= 0).all(axis=1)
    t = w.astype(np.float64) * iz
    # q in the swapped order: (t0 + t1) + t2 where A > 0, (t0 + t2) + t1 where A < 0
    q = np.where(A < 0, (t[:, 0] + t[:, 2]) + t[:, 1], (t[:, 0] + t[:, 1]) + t[:, 2])
    with np.errstate(all="ignore"):
        bb = t / q[:, None]
        first, second = np.where(A < 0, 2, 1), np.where(A < 0, 1, 2)
        r = np.arange(n)
        p = (bb[:, 0, None] * c[:, 0] + bb[r, first, None] * c[r, first]) + bb[r, second, None] * c[r, second]
    pts[ok], b[ok] = p[ok], bb[ok]
    return pts, b


# ------------------------------------------------------------------ what the mask-id image holds; what is hidden
def ids_of(mq, ids, who: str = "MapRaster") -> np.ndarray:
    """"obj": the map's keys; "class": every object's class_id; else one value per object -> int32 [S].  (Shared with
    map_rays.MapRays.)"""
    if isinstance(ids, str):
        if ids == "obj":
            v = [int(k) for k in mq.keys]
        elif ids == "class":
            v = [int(mq.all_obj[k].get("class_id", 0)) for k in mq.keys]
        else:
            raise ValueError(f"{who}: ids {ids!r}: 'obj', 'class' or one value per object")
    else:
        v = [int(x) for x in ids]
    if len(v) != mq.S:
        raise ValueError(f"{who}: {len(v)} ids for {mq.S} objects")
    return np.asarray(v, np.int32)


def hide_mask(mq, hide, dataset_name=None, scene_name: str = "room_0", who: str = "MapRaster") -> np.ndarray:
    """Positions, or names of MapQuery.hidden_sets() sets ("ceiling", "most", "hidden") -> uint8 [S]."""
    S = mq.S
    out = np.zeros(S, np.uint8)
    sets = None
    for h in ([hide] if isinstance(hide, (str, int, np.integer)) else list(hide)):
        if isinstance(h, str) and not h.lstrip("-").isdigit():
            if sets is None:
                sets = mq.hidden_sets(dataset_name, scene_name)
            if h not in ("ceiling", "most", "hidden"):
                raise ValueError(f"{who}: hide {h!r}: a position or one of ceiling, most, hidden")
            out[[int(p) for p in sets[h]]] = 1
        else:
            p = int(h)
            if not 0 <= p < S:
                raise ValueError(f"{who}: hide {p}: positions in [0, {S})")
            out[p] = 1
    return out


# ------------------------------------------------------------------------------------------------------- the device side
class MapRaster:
    """Views of a MapQuery's meshes.  render() rasterises one view; pick() and visible() read the last one."""

    def __init__(self, mq, dataset_name: Optional[str] = None, scene_name: str = "room_0"):
        """mq: a query.MapQuery (dense or compact).  dataset_name / scene_name: what MapQuery.hidden_sets takes, for hide
        sets given by name."""
        self.mq = mq
        self.dev = mq.dev
        self.dataset_name, self.scene_name = dataset_name, scene_name
        self.last = None                # the device dict of the last view
        self._view = None               # (T_CW, intrinsics, z_near) of the last view
        self._ws = None

    # ------------------------------------------------------------------------------------------------------------
    def ids_of(self, ids) -> np.ndarray:
        """"obj": the map's keys; "class": every object's class_id; else one value per object -> int32 [S]."""
        return ids_of(self.mq, ids)

    def hide_mask(self, hide) -> np.ndarray:
        """Positions, or names of MapQuery.hidden_sets() sets ("ceiling", "most", "hidden") -> uint8 [S]."""
        return hide_mask(self.mq, hide, self.dataset_name, self.scene_name)

    def render(self, T_WC, intrinsics, W: int, H: int, colors=None, hide=(), ids="obj", shading: str = "headlight",
               background=(255, 255, 255), z_near: float = Z_NEAR, to_host: bool = True, ambient: float = AMBIENT,
               _small_box: int = -1):
        """One view: T_WC [4, 4] camera to world, intrinsics (fx, fy, cx, cy), images [W, H].  colors: a [V, 3] device
        tensor of any MapQuery.color_by_* call (None: color_by_rgb()).  -> render_view.ViewBuffers (rgb uint8 [W, H, 3],
        maskid int32, depth fp32); to_host=False: the dict of device tensors {"rgb", "maskid", "depth", "winner"} that
        ViewEval.add takes, plus "face", "vertex" (int32 [W, H], -1 = nothing), "counts" (int64 [S]), "stats" (int64 [8],
        ops.RASTER_STATS), "status" (int32 [1]) and "key"."""
        import torch
        from . import ops
        from .render_view import ViewBuffers
        if shading not in SHADINGS:
            raise ValueError(f"MapRaster.render: shading {shading!r}: one of {SHADINGS}")
        mq, dev = self.mq, self.dev
        T_CW = camera_rows(T_WC)
        cam = np.asarray(T_WC, np.float64)[:3, 3]
        intr = tuple(float(x) for x in intrinsics)
        if len(intr) != 4:
            raise ValueError("MapRaster.render: intrinsics (fx, fy, cx, cy)")
        hide_m, ids_v = self.hide_mask(hide), self.ids_of(ids)
        verts, faces, face_off, _ = mq.mesh_buffers()
        if colors is None:
            colors = mq.color_by_rgb()
        if tuple(colors.shape) != (mq.V, 3):
            raise ValueError(f"MapRaster.render: colors [{mq.V}, 3], got {tuple(colors.shape)}")
        need = ops.raster_workspace_bytes(int(verts.shape[0]), int(faces.shape[0]))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        key, stats, status, ws = ops.raster_visibility(verts, faces, face_off, torch.from_numpy(hide_m).to(dev),
                                                       torch.from_numpy(T_CW).to(dev), intr, W, H, z_near, ws=self._ws,
                                                       _small_box=_small_box)
        out = ops.raster_resolve(verts, faces, face_off, torch.from_numpy(ids_v).to(dev), colors.to(dev, torch.float32), ws,
                                 key, cam, ambient, shading == "headlight", background)
        out.update(key=key, stats=stats, status=status)
        self.last, self._view = out, (T_CW, intr, float(z_near))
        if not to_host:
            return out
        buf = ViewBuffers.__new__(ViewBuffers)
        buf.rgb, buf.maskid, buf.depth = (out[k].cpu().numpy() for k in ("rgb", "maskid", "depth"))
        return buf

    def _need_view(self):
        if self.last is None:
            raise RuntimeError("MapRaster: no view rendered yet")
        return self.last

    def pick(self, pixels) -> Dict[str, np.ndarray]:
        """pixels [n, 2] as (w, h) of the last view -> dict(key: the object's key (-1: nothing there or outside the view),
        object: its position, face, vertex: packed ids (-1), point fp64 [n, 3] (NaN), depth fp32 [n] (100)).  vertex is
        the row of MapQuery.features, of the colour arrays and of PartRegions.label."""
        import torch
        last = self._need_view()
        mq = self.mq
        px = np.asarray(pixels, np.int64).reshape(-1, 2)
        W, H = last["winner"].shape
        inside = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
        flat = torch.from_numpy(np.where(inside, px[:, 0] * H + px[:, 1], 0)).to(self.dev)
        rows = {k: last[k].reshape(-1)[flat].cpu().numpy() for k in ("winner", "face", "vertex", "depth")}
        hit = inside & (rows["winner"] >= 0)
        obj = np.where(hit, rows["winner"], -1).astype(np.int64)
        face = np.where(hit, rows["face"], -1).astype(np.int64)
        verts, faces, _, _ = mq.mesh_buffers()
        fsel = torch.from_numpy(face[hit]).to(self.dev)
        corners = verts[faces[fsel].long()].cpu().numpy() if int(hit.sum()) else np.zeros((0, 3, 3))
        T_CW, intr, z_near = self._view
        point = np.full((len(px), 3), np.nan)
        point[hit] = pick_points(corners, px[hit], T_CW, intr, z_near)[0]
        return {"key": np.array([mq.keys[p] if p >= 0 else -1 for p in obj]), "object": obj, "face": face,
                "vertex": np.where(hit, rows["vertex"], -1).astype(np.int64), "point": point,
                "depth": np.where(hit, rows["depth"], np.float32(NO_DEPTH)).astype(np.float32)}

    def visible(self, min_pixels: int = 1) -> Dict:
        """{object key: pixels} of the objects that win at least min_pixels pixels of the last view, in the map's order."""
        counts = self._need_view()["counts"].cpu().numpy()
        return {k: int(c) for k, c in zip(self.mq.keys, counts) if c >= max(int(min_pixels), 1)}


# ----------------------------------------------------------------------------------------------------------------- CLI
def load_pose(path: str) -> np.ndarray:
    T = np.loadtxt(path, dtype=np.float64)
    if T.size != 16:
        raise ValueError(f"--pose: {path} holds {T.size} numbers, a 4 x 4 matrix has 16")
    return T.reshape(4, 4)


def _parse(argv):
    from . import map_query
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    map_query.add_map_arguments(ap, extra_modes=("partfeat",))
    ap.add_argument("--config", help="the scene's config: the camera and the poses of its dataset")
    ap.add_argument("--frames", default=None, help="a:b:s over the samples of the config's dataset (default: all)")
    ap.add_argument("--pose", help="a text file with one 4 x 4 camera-to-world matrix")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--intrinsics", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"))
    ap.add_argument("--hide", nargs="*", default=[], help="ceiling, most, hidden (MapQuery.hidden_sets) or positions")
    ap.add_argument("--shading", choices=SHADINGS, default="headlight")
    ap.add_argument("--ids", choices=("obj", "class"), default="obj", help="what maskid_<id>.png holds")
    ap.add_argument("--depth-scale", type=float, default=None, help="16-bit depth PNGs of round(depth * S)")
    ap.add_argument("--z-near", type=float, default=Z_NEAR)
    a = ap.parse_args(argv)
    if (a.config is None) == (a.pose is None):
        ap.error("the camera: either --config or --pose")
    if a.pose is not None:
        if a.size is None or a.intrinsics is None:
            ap.error("--pose needs --size W H and --intrinsics fx fy cx cy")
        if a.frames is not None:
            ap.error("--frames needs --config")
        if not os.path.isfile(a.pose):
            ap.error(f"--pose: no such file {a.pose}")
        try:
            a.T_WC = load_pose(a.pose)
            camera_rows(a.T_WC)
        except (ValueError, np.linalg.LinAlgError) as e:
            ap.error(str(e))
    else:
        if a.size is not None or a.intrinsics is not None:
            ap.error("--size and --intrinsics go with --pose; --config brings its own camera")
        if not os.path.isfile(a.config):
            ap.error(f"--config: no such file {a.config}")
    if a.size is not None and not (1 <= a.size[0] <= 65536 and 1 <= a.size[1] <= 65536):
        ap.error(f"--size {a.size[0]} {a.size[1]}: sides in [1, 65536]")
    if not a.z_near > 0.0:
        ap.error(f"--z-near {a.z_near} must be positive")
    if a.depth_scale is not None and not a.depth_scale > 0.0:
        ap.error(f"--depth-scale {a.depth_scale} must be positive")
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
    from . import map_query, map_view
    from . import query as oquery
    if a.config is not None:
        from . import dataset
        from .cfg import Config
        c = Config(a.config)
        if c.dataset_format not in ("Replica", "ScanNet"):
            raise ValueError("Dataset format {} not found".format(c.dataset_format))
        ds = (dataset.Replica if c.dataset_format == "Replica" else dataset.ScanNet)(c)
        W, H, intr = int(c.W), int(c.H), (float(c.fx), float(c.fy), float(c.cx), float(c.cy))
        views = [(int(ds.start + i * ds.stride), np.asarray(ds.depth_and_pose(i)[1], np.float64))
                 for i in map_view.parse_frames(a.frames, len(ds))]
    else:
        W, H, intr = a.size[0], a.size[1], tuple(a.intrinsics)
        views = [(0, a.T_WC)]
    mq = oquery.MapQuery(all_obj, a.device)
    colors = map_query.colors_for_mode(mq, a.mode, q, a.top, a.color_yaml)
    mr = MapRaster(mq, a.dataset, a.scene)
    doc = {"mode": a.mode, "size": [W, H], "intrinsics": list(intr), "frames": []}
    for frame_id, T_WC in views:
        buf = mr.render(T_WC, intr, W, H, colors=colors, hide=a.hide, ids=a.ids, shading=a.shading, z_near=a.z_near)
        map_view.write_view(a.out, frame_id, buf, a.depth_scale)
        seen = mr.visible()
        from . import ops
        doc["frames"].append({"frame": frame_id, "visible": [{"id": int(k), "pixels": n} for k, n in seen.items()],
                              "stats": dict(zip(ops.RASTER_STATS, (int(x) for x in mr.last["stats"].cpu().tolist()))),
                              "status": int(mr.last["status"].item())})
        print(f"frame {frame_id}: {len(seen)} objects seen, {sum(seen.values())} of {W * H} pixels painted")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "visible.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    return doc


__all__ = ["MapRaster", "ids_of", "hide_mask", "camera_rows", "project_vertices", "pick_points", "load_pose", "AMBIENT", "Z_NEAR", "SHADINGS"]

if __name__ == "__main__":
    main()
