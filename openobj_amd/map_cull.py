"""Cull meshes to the surface the frames of a sequence could have observed, before they are scored.

    python -m openobj_amd.map_cull --config scene.json --in DIR --out DIR [--stride N] [--eps E] [--min-views M]
        [--margin PX] [--face-rule all|any] [--device cuda:0]

This is the step vMAP's, iMAP's and NICE-SLAM's evaluations run first, on the prediction and on the ground truth alike:
the back of a sofa against the wall, the floor under a bed and the inside of a closed marching-cubes shell were never
seen by the sensor, so neither side is charged for them.  The reference dropped its evaluation, so nothing here has a
counterpart in it.  It reads DIR/obj_<id>.ply, the depth images and poses of the sequence the config names, and writes
the culled obj_<id>.ply (vertex colours and normals follow their vertices) plus cull.json.

A vertex p is SEEN by a frame when, with M the upper 3 x 4 of inverse(T_WC) (inverted here in float64), in fp64 with
every operation rounded once (objnerf_vertex_views):

    xc = ((M[0] px + M[1] py) + M[2] pz) + M[3]     (yc, zc likewise)           zc > z_min
    iu = floor((fx xc) / zc + cx + 0.5),  iv = floor((fy yc) / zc + cy + 0.5)   margin <= iu <= W - 1 - margin, iv likewise
    d = depth[iu, iv] > 0  and  zc <= d + eps

so a vertex in free space in front of the measured surface counts as seen (it is observed to be wrong, which accuracy
should charge) and one more than eps behind it does not.  A vertex stays when at least min_views frames see it; a face
stays when all ("all") or any ("any") of its corners do; the output holds the kept faces in their order and exactly the
vertices they use, in their order (objnerf_mesh_cull_count / _emit).  eps = 0.05 m is an ASSUMED value (vMAP's script
was not available; it equals the shipped configs' other_eps): the parameters are written into every output file, and
only runs made with the same values compare.

The module imports without a GPU; the bindings load on first use.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, Iterable, Sequence, Tuple

import numpy as np

from . import mesh

Z_MIN, EPS, MARGIN, MIN_VIEWS, FACE_RULE = 0.0, 0.05, 0, 1, "all"     # eps: an assumed value (module docstring)


def world_to_camera(T_WC) -> np.ndarray:
    """[B, 4, 4] camera -> world poses -> the [B, 3, 4] world -> camera rows the visibility rule takes (float64)."""
    T = np.asarray(T_WC, np.float64).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.linalg.inv(T)[:, :3, :]) if len(T) else np.zeros((0, 3, 4))


def _as_mesh(m) -> Tuple[np.ndarray, np.ndarray]:
    v, f = (m.vertices, m.faces) if isinstance(m, mesh.TriMesh) else m
    return np.ascontiguousarray(v, np.float64).reshape(-1, 3), np.ascontiguousarray(f, np.int64).reshape(-1, 3)


def _config(cfg):
    from .cfg import Config
    return cfg if isinstance(cfg, Config) else Config(cfg)


def intrinsics_of(cfg) -> Tuple[float, float, float, float]:
    c = _config(cfg)
    return float(c.fx), float(c.fy), float(c.cx), float(c.cy)


def frame_batches(cfg, stride: int = 1, batch: int = 32):
    """Yields (T_WC float64 [B, 4, 4], depth float32 [B, W, H]) numpy arrays over every `stride`-th sample of the
    config's dataset (the dataset applies the config's own start and stride first), `batch` frames at a time, the last
    batch ragged.  Reads depth images and poses only."""
    from . import dataset
    c = _config(cfg)
    if c.dataset_format not in ("Replica", "ScanNet"):
        raise ValueError("Dataset format {} not found".format(c.dataset_format))
    ds = (dataset.Replica if c.dataset_format == "Replica" else dataset.ScanNet)(c)
    if stride < 1 or batch < 1:
        raise ValueError("frame_batches: stride and batch must be positive")
    ids = list(range(0, len(ds), int(stride)))
    for b0 in range(0, len(ids), int(batch)):
        pairs = [ds.depth_and_pose(i) for i in ids[b0:b0 + int(batch)]]
        yield (np.stack([np.asarray(p[1], np.float64) for p in pairs]),
               np.stack([np.asarray(p[0], np.float32) for p in pairs]))


def count_views(meshes, batches: Iterable, intrinsics: Sequence[float], z_min: float = Z_MIN, eps: float = EPS,
                margin: int = MARGIN, device="cuda:0"):
    """meshes: {id: (vertices, faces) or mesh.TriMesh}, or a sequence of such dicts (pred, ground truth, ...).  batches:
    an iterable of (T_WC [B, 4, 4], depth [B, W, H]) as frame_batches yields.  The vertices of ALL meshes go into one
    array and the frames are walked once.  -> (views, n_frames): views {id: int32 [V_id]} (a list of such dicts for a
    sequence of dicts), the number of frames that see each vertex."""
    import torch
    from . import ops
    single = isinstance(meshes, dict)
    dicts = [meshes] if single else list(meshes)
    keys, parts = [], []
    for di, d in enumerate(dicts):
        for k in d:
            keys.append((di, k))
            parts.append(_as_mesh(d[k])[0])
    dev = torch.device(device)
    verts = torch.from_numpy(np.concatenate(parts) if parts else np.zeros((0, 3))).to(dev)
    views = torch.zeros(len(verts), dtype=torch.int32, device=dev)
    n_frames = 0
    for T_WC, depth in batches:
        T_CW = torch.from_numpy(world_to_camera(T_WC)).to(dev)
        depth = torch.as_tensor(np.ascontiguousarray(depth, np.float32) if isinstance(depth, np.ndarray) else depth)
        ops.vertex_views(verts, T_CW, depth.to(dev), intrinsics, z_min, eps, margin, out=views)
        n_frames += int(T_CW.shape[0])
    host = views.cpu().numpy()
    out, row = [dict() for _ in dicts], 0
    for (di, k), p in zip(keys, parts):
        out[di][k] = host[row:row + len(p)].copy()
        row += len(p)
    return (out[0] if single else out), n_frames


def cull(meshes: Dict, views: Dict, min_views: int = MIN_VIEWS, rule: str = FACE_RULE, device="cuda:0"):
    """meshes {id: (vertices, faces) or TriMesh}, views {id: int32 [V_id]} from count_views -> (culled {id: (vertices
    float64 [Vn, 3], faces int64 [Fn, 3])}, old_of_new {id: int64 [Vn]}): a vertex is kept when views >= min_views, a
    face by `rule`; vertices[new] = input vertices[old_of_new[new]], so colours and features are carried along by the
    same index.  The meshes are compacted back to back in one call; a mesh left without faces is returned empty."""
    import torch
    from . import ops
    ids = list(meshes)
    ms = [_as_mesh(meshes[k]) for k in ids]
    vert_off = np.concatenate([[0], np.cumsum([len(v) for v, _ in ms])]).astype(np.int64)
    face_off = np.concatenate([[0], np.cumsum([len(f) for _, f in ms])]).astype(np.int64)
    for k, (v, _) in zip(ids, ms):
        if np.asarray(views[k]).shape != (len(v),):
            raise ValueError(f"cull: views[{k!r}] does not have one entry per vertex")
    if vert_off[-1] >= 2 ** 31:
        raise ValueError("cull: at most 2^31 - 1 vertices at once")
    keep = np.concatenate([np.asarray(views[k]) >= int(min_views) for k in ids]) if ids else np.zeros(0, bool)
    faces = np.concatenate([f + o for (_, f), o in zip(ms, vert_off[:-1])]) if ids else np.zeros((0, 3), np.int64)
    if faces.size and (faces.min() < -2 ** 31 or faces.max() >= 2 ** 31):
        raise ValueError("cull: a face index does not fit int32")
    dev = torch.device(device)
    r = ops.mesh_compact(torch.from_numpy(keep.astype(np.uint8)).to(dev), torch.from_numpy(faces.astype(np.int32)).to(dev), rule)
    old_of_new = r["old_of_new"].cpu().numpy().astype(np.int64)
    face_old = r["face_old"].cpu().numpy().astype(np.int64)
    new_faces = r["faces"].cpu().numpy().astype(np.int64)
    # meshes stored back to back stay back to back and in order
    nv = np.searchsorted(old_of_new, vert_off)
    nf = np.searchsorted(face_old, face_off)
    culled, back = {}, {}
    for j, k in enumerate(ids):
        o = old_of_new[nv[j]:nv[j + 1]] - vert_off[j]
        culled[k] = (ms[j][0][o], new_faces[nf[j]:nf[j + 1]] - nv[j])
        back[k] = o
    return culled, back


def _sizes(before: Dict, after: Dict) -> Dict:
    return {str(k): {"vertices": [int(len(_as_mesh(before[k])[0])), int(len(after[k][0]))],
                     "faces": [int(len(_as_mesh(before[k])[1])), int(len(after[k][1]))]} for k in before}


def add_arguments(ap: argparse.ArgumentParser, prefix: str = "") -> None:
    """The culling parameters as command-line options (--<prefix>stride, ...), shared with openobj_amd.map_eval."""
    ap.add_argument(f"--{prefix}stride", type=int, default=1, help="every N-th sample of the config's dataset")
    ap.add_argument(f"--{prefix}eps", type=float, default=EPS, help="metres behind the measured depth that still count "
                    "as seen (an assumed value)")
    ap.add_argument(f"--{prefix}min-views", type=int, default=MIN_VIEWS, help="frames that must see a vertex")
    ap.add_argument(f"--{prefix}margin", type=int, default=MARGIN, help="pixels of the image border that do not count")
    ap.add_argument(f"--{prefix}face-rule", choices=("all", "any"), default=FACE_RULE,
                    help="a face stays when all / any of its corners are kept")


def parameters(stride, eps, min_views, margin, face_rule) -> Dict:
    return {"z_min": Z_MIN, "eps": float(eps), "margin": int(margin), "min_views": int(min_views),
            "face_rule": face_rule, "stride": int(stride)}


def cull_sides(sides: Sequence[Dict], config, params: Dict, device="cuda:0", batch: int = 32):
    """Several {id: mesh} dicts culled against the config's sequence in ONE pass over the frames -> ([culled dict per
    side], [old_of_new dict per side], report) with report = {"parameters", "frames", "sides": [per-object sizes]}."""
    c = _config(config)
    views, n = count_views(list(sides), frame_batches(c, params["stride"], batch), intrinsics_of(c), params["z_min"],
                           params["eps"], params["margin"], device)
    out, back = [], []
    for d, vw in zip(sides, views):
        cd, b = cull(d, vw, params["min_views"], params["face_rule"], device)
        out.append(cd)
        back.append(b)
    return out, back, {"parameters": dict(params), "frames": int(n), "sides": [_sizes(d, cd) for d, cd in zip(sides, out)]}


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--config", required=True, help="the scene's config (dataset path, format, camera)")
    ap.add_argument("--in", dest="src", required=True, help="reads DIR/obj_<id>.ply")
    ap.add_argument("--out", required=True, help="writes DIR/obj_<id>.ply and DIR/cull.json")
    add_arguments(ap)
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None):
    from .map_eval import mesh_files
    a = _parser().parse_args(argv)
    files = mesh_files(a.src)
    if not files:
        raise FileNotFoundError(f"no obj_<id>.ply under {a.src}")
    raw = {k: mesh.read_ply(f) for k, f in files.items()}
    meshes = {k: (r[0].astype(np.float64), r[3]) for k, r in raw.items()}
    params = parameters(a.stride, a.eps, a.min_views, a.margin, a.face_rule)
    (culled,), (back,), report = cull_sides([meshes], a.config, params, a.device)
    os.makedirs(a.out, exist_ok=True)
    for k, (v, f) in culled.items():
        _, normals, rgba, _ = raw[k]
        m = mesh.TriMesh(v, f, None if normals is None else normals[back[k]])
        if rgba is not None:
            m.visual.vertex_colors = rgba[back[k]]
        m.export(os.path.join(a.out, f"obj_{k}.ply"))
    res = {"parameters": report["parameters"], "frames": report["frames"], "objects": report["sides"][0]}
    with open(os.path.join(a.out, "cull.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    nv = sum(o["vertices"][1] for o in res["objects"].values())
    print(f"{len(culled)} objects, {res['frames']} frames, {nv} vertices kept -> {a.out}")
    return res


if __name__ == "__main__":
    main()
