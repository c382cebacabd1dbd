"""Open-vocabulary queries over an exported map (openobj_amd.query.MapQuery on map_vis.pkl.gz):

    python -m openobj_amd.map_query --logdir DIR --mode {rgb,class,instance,partpca,object,part}
        [--clip-query F.npy --sbert-query F.npy --part-query F.npy --top N --color-yaml PATH
         --dataset Replica|Scannet --scene NAME --compact
         --regions [--region-frac F | --region-min-cos C] [--region-min-area A]] --out DIR

--compact reads map_vis_compact.pkl.gz (python -m openobj_amd.map_vis --compact); without the flag the dense
map_vis.pkl.gz is read if it is there, else the compact file.

Writes one coloured obj_<id>.ply per visible object (uint8 colours round(c * 255)) and query.json (mode, the visible
ids, the ranked object ids with their similarities, the top-k ids).  --dataset Replica hides the "ceiling" objects as
the reference's viewer does by default (vis_interaction.py:181-184); without --dataset every object is written.
--mode part --regions also writes regions.json (one record per connected patch of the part query on the top objects:
vertices, faces, area, centroid, normal, axes, extent, box, peak; MapQuery.part_regions) and
obj_<id>_regions.ply per top object (a palette colour per region, darkened RGB elsewhere).  --region-frac F (default
0.75, an assumed value) keeps the vertices at or above F of the object's own similarity range, --region-min-cos C
those with a cosine >= C; --region-min-area A [m^2] drops smaller regions.  Without --regions every file is as before.
Every argument, query file and query width is checked before the device is touched."""
from __future__ import annotations

import argparse
import gzip
import json
import os
import pickle

import numpy as np

MODES = ("rgb", "class", "instance", "partpca", "object", "part")
NEEDS = {"object": ("clip_query", "sbert_query"), "part": ("clip_query", "sbert_query", "part_query"),
         "class": ("color_yaml",)}


DENSE_FILE, COMPACT_FILE = "map_vis.pkl.gz", "map_vis_compact.pkl.gz"        # (map_vis.py writes them)


def _width(all_obj, key):
    for o in all_obj.values():
        if key == "part_feat" and o.get("part_head") is not None:      # a compact map: the head's C
            return int(np.shape(o["part_head"])[0])
        f = o.get(key)
        if f is not None and np.size(f):
            return int(np.shape(f)[-1])
    return None


def add_map_arguments(ap, extra_modes=()) -> None:
    """The arguments that name the map, the colouring and its queries (shared with map_raster's CLI)."""
    ap.add_argument("--logdir", required=True)
    ap.add_argument("--mode", required=True, choices=MODES + tuple(extra_modes))
    ap.add_argument("--clip-query")
    ap.add_argument("--sbert-query")
    ap.add_argument("--part-query")
    ap.add_argument("--top", type=int, default=None)
    ap.add_argument("--color-yaml")
    ap.add_argument("--dataset", choices=("Replica", "Scannet"))
    ap.add_argument("--scene", default="room_0")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--compact", action="store_true", help="read map_vis_compact.pkl.gz")


def _parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    add_map_arguments(ap)
    ap.add_argument("--regions", action="store_true", help="--mode part: also write regions.json and obj_<id>_regions.ply")
    ap.add_argument("--region-frac", type=float, default=None)
    ap.add_argument("--region-min-cos", type=float, default=None)
    ap.add_argument("--region-min-area", type=float, default=None)
    a = ap.parse_args(argv)
    given = [n for n in ("region_frac", "region_min_cos", "region_min_area") if getattr(a, n) is not None]
    if a.regions and a.mode != "part":
        ap.error("--regions needs --mode part")
    if given and not a.regions:
        ap.error(f"--{given[0].replace('_', '-')} needs --regions")
    if a.region_frac is not None and a.region_min_cos is not None:
        ap.error("--region-frac and --region-min-cos exclude each other")
    if a.region_frac is not None and not 0.0 <= a.region_frac <= 1.0:
        ap.error(f"--region-frac {a.region_frac} outside [0, 1]")
    if a.region_min_cos is not None and not -1.0 <= a.region_min_cos <= 1.0:
        ap.error(f"--region-min-cos {a.region_min_cos} outside [-1, 1]")
    if a.region_min_area is not None and not a.region_min_area >= 0.0:
        ap.error(f"--region-min-area {a.region_min_area} is negative")
    all_obj, queries = check_map_arguments(ap, a)
    return a, all_obj, queries


def check_map_arguments(ap, a):
    """The checks of add_map_arguments' values (ap.error on the first that fails) -> (all_obj: the map file's dict,
    queries: name -> fp32 vector, the ones the mode needs); a.map_file is set."""
    for k in NEEDS.get(a.mode, ()):
        v = getattr(a, k)
        if v is None:
            ap.error(f"--mode {a.mode} needs --{k.replace('_', '-')}")
        if not os.path.isfile(v):
            ap.error(f"--{k.replace('_', '-')}: no such file {v}")
    path = os.path.join(a.logdir, COMPACT_FILE if a.compact else DENSE_FILE)
    if not a.compact and not os.path.isfile(path) and os.path.isfile(os.path.join(a.logdir, COMPACT_FILE)):
        path = os.path.join(a.logdir, COMPACT_FILE)
    if not os.path.isfile(path):
        ap.error(f"{path} is missing: run python -m openobj_amd.map_vis --logdir {a.logdir}"
                 f"{' --compact' if a.compact else ''} first")
    a.map_file = path
    with gzip.open(path, "rb") as fh:
        all_obj = pickle.load(fh)
    queries = {}
    for k, feat in (("clip_query", "clip_feat"), ("sbert_query", "caption_feat"), ("part_query", "part_feat")):
        if getattr(a, k) is None or k not in NEEDS.get(a.mode, ()):
            continue
        q = np.load(getattr(a, k)).astype(np.float32).reshape(-1)
        w = _width(all_obj, feat)
        if w is None or q.size != w:
            ap.error(f"--{k.replace('_', '-')}: width {q.size} does not match the map's {feat} width {w}")
        queries[k] = q
    return all_obj, queries


def colors_for_mode(mq, mode: str, q, top=None, color_yaml=None):
    """The mode -> colours dispatch of the CLIs: -> [V, 3] on the device.  q: check_map_arguments' queries."""
    if mode == "rgb":
        return mq.color_by_rgb()
    if mode == "class":
        return mq.color_by_class(color_yaml)
    if mode == "instance":
        return mq.color_by_instance()
    if mode in ("partpca", "partfeat"):                     # (map_raster's CLI takes either name)
        return mq.color_by_partfeat()
    if mode == "object":
        return mq.color_by_object_query(q["clip_query"], q["sbert_query"], 0 if top is None else top)
    if mode == "part":
        return mq.color_by_part_query(q["clip_query"], q["sbert_query"], q["part_query"], 1 if top is None else top)
    raise ValueError(f"colors_for_mode: mode {mode!r}: one of {MODES}")


def main(argv=None):
    a, all_obj, q = _parse(argv)
    from . import mesh as omesh
    from . import query as oquery
    mq = oquery.MapQuery(all_obj, a.device)
    col = colors_for_mode(mq, a.mode, q, a.top, a.color_yaml)
    hidden = set(mq.hidden_sets(a.dataset, a.scene)["hidden"]) if a.dataset else set()
    os.makedirs(a.out, exist_ok=True)
    visible = []
    for p, (k, c) in enumerate(zip(mq.keys, mq.split(col))):
        if p in hidden:
            continue
        m = all_obj[k]["mesh"]
        out = omesh.TriMesh(m.vertices, m.faces, m.vertex_normals)
        out.visual.vertex_colors = np.round(c.cpu().numpy().astype(np.float64) * 255).astype(np.uint8)
        out.export(os.path.join(a.out, f"obj_{k}.ply"))
        visible.append(k)
    rank = mq.last_ranking or []
    top = [k for k, _ in rank[: (1 if a.top is None else a.top) if a.mode == "part" else (a.top or 0)]]
    doc = {"mode": a.mode, "visible": [int(k) for k in visible],
           "ranking": [{"id": int(k), "similarity": s} for k, s in rank], "top": [int(k) for k in top]}
    with open(os.path.join(a.out, "query.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    if a.regions:
        from . import map_regions
        pos = [mq.keys.index(k) for k in top]
        reg = mq.part_regions(q["part_query"], objects=pos, frac=0.75 if a.region_frac is None else a.region_frac,
                              min_cos=a.region_min_cos, min_area=a.region_min_area or 0.0)
        map_regions.write_regions(a.out, mq, reg, pos)
        print(f"{len(reg)} regions on {len(pos)} objects -> {os.path.join(a.out, 'regions.json')}")
    print(f"{len(visible)} objects -> {a.out}")
    return doc


if __name__ == "__main__":
    main()
