"""Geometry evaluation of a finished map: accuracy, completion and completion ratio between two sets of meshes.

    python -m openobj_amd.map_eval --logdir OUT (--gt-dir DIR | --ref-logdir OTHER) [--gt-scene mesh.ply]
        [--samples N] [--scene-samples N] [--thresholds 0.05 0.01] [--seed S] [--out FILE] [--device cuda:0]
        [--cull-config scene.json [--cull-stride N] [--cull-eps E] [--cull-min-views M] [--cull-margin PX]
         [--cull-face-rule all|any]]

This is vMAP's measure (points sampled on the reconstructed and on the ground-truth meshes, nearest neighbours both
ways); the reference dropped that step, so nothing here has a counterpart in it.  It reads OUT/map_vis/obj_<id>.ply
(what `python -m openobj_amd.map_vis` writes) and the other side from DIR/obj_<id>.ply or OTHER/map_vis/, and writes
eval_geometry.json.  With --ref-logdir it compares two runs of the mapper against each other: no dataset needed.

All points are drawn by ONE ops.mesh_sample call (objnerf_mesh_sample), the nearest points are exact
(ops.NearestPlan, objnerf_nearest) and the sums run in a fixed order (ops.seg_stats): the same inputs and seed give the
same file, bit for bit.

    accuracy              mean distance from a predicted sample to the nearest ground-truth sample, in metres
    completion            mean distance from a ground-truth sample to the nearest predicted sample
    completion_ratio@t    the share of ground-truth samples with a predicted sample nearer than t
    chamfer               the mean of accuracy and completion

per object over the ids both sides hold (ids on one side only are listed as missing_pred / missing_gt), and once at
scene level with every object of a side as one surface.  The sample counts (10 000 per object, 200 000 per scene) are
ASSUMED sizes: vMAP's evaluation script is not part of the reference and was not available; they set the resolution of
the measure (a sample-to-sample distance cannot fall below the spacing of the samples), so compare only runs made with
the same counts.

With --cull-config every side (the run, the other side, --gt-scene) is first culled to the surface the frames of that
scene's sequence observed, in one pass over the frames (openobj_amd/map_cull.py): without it a real ground truth charges
the run for geometry the sensor never saw.  The file then gains a "cull" entry (parameters, frames, sizes per side);
an object left empty on a side counts as absent.  Without the option the file is what it was before.
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import re
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import map_cull, mesh, ops

N_SAMPLES = 10000           # per object and side: an assumed size (see the module docstring)
N_SCENE_SAMPLES = 200000    # per side at scene level: likewise


# ------------------------------------------------------------------------------------------------------------ metrics
def _stats_row(d, thresholds) -> np.ndarray:
    """The row ops.seg_stats writes for one segment, on the host: [n finite, n non-finite, sum, sum of squares, max,
    counts of d < thr]."""
    d = np.asarray(torch.as_tensor(d).detach().cpu().numpy() if isinstance(d, torch.Tensor) else d, np.float64).reshape(-1)
    fin = d[np.isfinite(d)]
    row = [float(fin.size), float(d.size - fin.size), float(fin.sum()), float((fin * fin).sum()),
           float(fin.max()) if fin.size else -math.inf]
    return np.array(row + [float((fin < t).sum()) for t in thresholds], np.float64)


def _metrics_from_stats(acc: np.ndarray, comp: np.ndarray, thresholds: Sequence[float]) -> Dict:
    """acc / comp: seg_stats rows of the pred -> gt and gt -> pred distances.  Means run over the finite distances; a
    non-finite one (no point on the other side) counts as a miss in the ratios.  None where nothing can be said."""
    def mean(r):
        return float(r[2] / r[0]) if r[0] > 0 else None
    a, c = mean(acc), mean(comp)
    n_gt = comp[0] + comp[1]
    out = {"accuracy": a, "completion": c, "chamfer": None if a is None or c is None else 0.5 * (a + c)}
    for t, thr in enumerate(thresholds):
        out[f"completion_ratio@{thr:g}"] = float(comp[5 + t] / n_gt) if n_gt > 0 else None
    out["n_pred"] = int(acc[0] + acc[1])
    out["n_gt"] = int(n_gt)
    out["n_nonfinite"] = int(acc[1] + comp[1])
    return out


def metrics_from_distances(d_pred_to_gt, d_gt_to_pred, thresholds: Sequence[float] = (0.05, 0.01)) -> Dict:
    """The metrics of one object (or scene) from its two arrays of nearest-point distances (not squares), numpy arrays
    or tensors on any device; host code only."""
    return _metrics_from_stats(_stats_row(d_pred_to_gt, thresholds), _stats_row(d_gt_to_pred, thresholds), thresholds)


# ------------------------------------------------------------------------------------------------------------ compare
def _as_mesh(m):
    v, f = (m.vertices, m.faces) if isinstance(m, mesh.TriMesh) else m
    v, f = np.ascontiguousarray(v, np.float64).reshape(-1, 3), np.ascontiguousarray(f, np.int64).reshape(-1, 3)
    return v, f


def compare(pred, gt, n_samples: int = N_SAMPLES, thresholds: Sequence[float] = (0.05, 0.01), seed: int = 0,
            n_scene_samples: int = N_SCENE_SAMPLES, device="cuda:0", cell: Optional[float] = None, per_object: bool = True,
            return_samples: bool = False) -> Dict:
    """pred, gt: {obj_id: (vertices [V, 3], faces [F, 3]) or mesh.TriMesh}.  -> {"objects": {id: metrics}, "scene":
    metrics, "missing_pred": [...], "missing_gt": [...], ...} (see the module docstring).  A mesh without a face counts
    as absent.  n_samples / n_scene_samples default to ASSUMED sizes (module docstring).

    The mesh_sample call has 2 K + 2 segments for the K common ids in ascending order: pred objects, gt objects (n_samples
    each), then all of pred and all of gt as one surface each (n_scene_samples each, which spreads them over the objects
    by area).  per_object = False leaves the 2 K object segments out (a whole-scene ground truth has no ids).
    cell: the search grid's cell side (None: chosen per search; the result does not depend on it)."""
    thresholds = [float(t) for t in thresholds]
    dev = torch.device(device)
    sides = []
    for d in (pred, gt):
        ms = {k: _as_mesh(m) for k, m in d.items()}
        sides.append({k: m for k, m in ms.items() if len(m[1])})
    P, G = sides
    common = sorted(set(P) & set(G)) if per_object else []
    missing_pred = [int(k) for k in sorted(set(G) - set(P))] if per_object else []        # (plain ints: json.dump)
    missing_gt = [int(k) for k in sorted(set(P) - set(G))] if per_object else []
    K = len(common)

    # vertices once (pred ids ascending, then gt ids), faces once per segment that uses them
    verts, base, row = [], {}, 0
    for si, side in enumerate((P, G)):
        for k in sorted(side):
            base[(si, k)] = row
            verts.append(side[k][0])
            row += len(side[k][0])
    faces, face_off, samp_off = [], [0], [0]

    def segment(items, n):
        nf = 0
        for si, k in items:
            faces.append(sides[si][k][1] + base[(si, k)])
            nf += len(sides[si][k][1])
        face_off.append(face_off[-1] + nf)
        samp_off.append(samp_off[-1] + (int(n) if nf else 0))

    for si in (0, 1):
        for k in common:
            segment([(si, k)], n_samples)
    for si in (0, 1):
        segment([(si, k) for k in sorted(sides[si])], n_scene_samples)
    V = torch.from_numpy(np.concatenate(verts) if verts else np.zeros((0, 3))).to(dev)
    Fc = torch.from_numpy((np.concatenate(faces) if faces else np.zeros((0, 3), np.int64)).astype(np.int32)).to(dev)
    pts, tri = ops.mesh_sample(V, Fc, face_off, samp_off, seed)

    def both_ways(s0, s1, g0, g1):
        """Segments [s0, s1) of pred against [g0, g1) of gt -> the seg_stats rows (accuracy, completion)."""
        po = np.asarray(samp_off[s0:s1 + 1]) - samp_off[s0]
        go = np.asarray(samp_off[g0:g1 + 1]) - samp_off[g0]
        pp, gp = pts[samp_off[s0]:samp_off[s1]], pts[samp_off[g0]:samp_off[g1]]
        acc = torch.sqrt(ops.NearestPlan(gp, go, cell).query(pp, po)[0])
        comp = torch.sqrt(ops.NearestPlan(pp, po, cell).query(gp, go)[0])
        return (ops.seg_stats(acc, po, thresholds).cpu().numpy(), ops.seg_stats(comp, go, thresholds).cpu().numpy())

    res = {"objects": {}, "scene": None, "missing_pred": missing_pred, "missing_gt": missing_gt,
           "n_samples": int(n_samples), "n_scene_samples": int(n_scene_samples), "thresholds": thresholds, "seed": int(seed)}
    if K:
        a, c = both_ways(0, K, K, 2 * K)
        for j, k in enumerate(common):
            res["objects"][int(k)] = _metrics_from_stats(a[j], c[j], thresholds)
    a, c = both_ways(2 * K, 2 * K + 1, 2 * K + 1, 2 * K + 2)
    res["scene"] = _metrics_from_stats(a[0], c[0], thresholds)
    if return_samples:
        res["samples"] = {"pts": pts, "tri": tri, "samp_off": list(samp_off), "face_off": list(face_off), "verts": V,
                          "faces": Fc}
    return res


# ---------------------------------------------------------------------------------------------------------------- CLI
def mesh_files(path: str) -> Dict[int, str]:
    """{id: file} of the obj_<id>.ply files in a directory."""
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "obj_*.ply"))):
        m = re.fullmatch(r"obj_(-?\d+)\.ply", os.path.basename(f))
        if m:
            out[int(m.group(1))] = f
    return out


def read_mesh_dir(path: str) -> Dict[int, tuple]:
    """{id: (vertices, faces)} of the obj_<id>.ply files in a directory."""
    out = {}
    for k, f in mesh_files(path).items():
        v, _, _, faces = mesh.read_ply(f)
        out[k] = (v.astype(np.float64), faces)
    return out


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--logdir", required=True, help="the run to score: reads LOGDIR/map_vis/obj_<id>.ply")
    other = ap.add_mutually_exclusive_group()
    other.add_argument("--gt-dir", default=None, help="ground-truth meshes, DIR/obj_<id>.ply")
    other.add_argument("--ref-logdir", default=None, help="another run to compare with (OTHER/map_vis/)")
    ap.add_argument("--gt-scene", default=None, help="one whole-scene ground-truth mesh (.ply): scene level only")
    ap.add_argument("--samples", type=int, default=N_SAMPLES, help="per object and side (an assumed size)")
    ap.add_argument("--scene-samples", type=int, default=N_SCENE_SAMPLES, help="per side at scene level (an assumed size)")
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.05, 0.01], help="metres; at most 4")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="default: LOGDIR/eval_geometry.json")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--cull-config", default=None, help="a scene config: cull every side to what its frames observed "
                    "(openobj_amd.map_cull) before comparing")
    map_cull.add_arguments(ap, "cull-")
    return ap


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    if not (a.gt_dir or a.ref_logdir or a.gt_scene):
        ap.error("one of --gt-dir, --ref-logdir or --gt-scene is required")
    pred = read_mesh_dir(os.path.join(a.logdir, "map_vis"))
    if not pred:
        raise FileNotFoundError(f"no obj_<id>.ply under {os.path.join(a.logdir, 'map_vis')}: run openobj_amd.map_vis first")
    kw = dict(n_samples=a.samples, thresholds=a.thresholds, seed=a.seed, n_scene_samples=a.scene_samples, device=a.device)
    res = {}
    other = scene = None
    if a.gt_dir or a.ref_logdir:
        other = read_mesh_dir(a.gt_dir if a.gt_dir else os.path.join(a.ref_logdir, "map_vis"))
    if a.gt_scene:
        v, _, _, faces = mesh.read_ply(a.gt_scene)
        scene = {0: (v.astype(np.float64), faces)}
    culled = None
    if a.cull_config:
        # every side in ONE pass over the frames
        given = {"pred": pred, "other": other, "gt_scene": scene}
        names = [n for n, s in given.items() if s is not None]
        params = map_cull.parameters(a.cull_stride, a.cull_eps, a.cull_min_views, a.cull_margin, a.cull_face_rule)
        sides, _, rep = map_cull.cull_sides([given[n] for n in names], a.cull_config, params, a.device)
        by_name = dict(zip(names, sides))
        pred, other, scene = by_name["pred"], by_name.get("other"), by_name.get("gt_scene")
        culled = {"parameters": rep["parameters"], "frames": rep["frames"]}
        for n, sizes in zip(names, rep["sides"]):
            culled[n] = {"vertices": [sum(o["vertices"][j] for o in sizes.values()) for j in (0, 1)],
                         "faces": [sum(o["faces"][j] for o in sizes.values()) for j in (0, 1)], "objects": sizes}
    if other is not None:
        res = compare(pred, other, **kw)
    if scene is not None:
        whole = compare(pred, scene, per_object=False, **kw)
        if res:
            res["scene_vs_gt_scene"] = whole["scene"]
        else:
            res = whole
    if culled is not None:
        res["cull"] = culled
    res["objects"] = {str(k): v for k, v in res["objects"].items()}
    out = a.out or os.path.join(a.logdir, "eval_geometry.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    s = res["scene"]
    print(f"{len(res['objects'])} objects, scene accuracy {s['accuracy']} completion {s['completion']} -> {out}")
    return res


if __name__ == "__main__":
    main()
