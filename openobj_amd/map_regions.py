"""Part regions: the connected surface patches a part query selects on the map's meshes, as entities with a pose
(objnerf_mapregions.hip).  MapQuery.part_regions (query.py) drives the device side; everything here is
host arithmetic on the integer table and needs no device:

  thresholds          thr[s] = fp32(mn + fp32(frac * fp32(mx - mn))) per object, the rainbow's own normalisation; or min_cos
  regions_from_table  every derived value (area, centroid, normal, axes, extent, box, peak) from the int64 table, in fp64
  filter_rows         the min_area / min_vertices filter and the old row -> new row map
  PartRegions         the result
  write_regions       regions.json and obj_<id>_regions.ply of the CLI

The table's columns and the per-face sequence stand in include/objnerf_hip.h."""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Sequence

import numpy as np

ROW = 32                                # OBJNERF_REGION_ROW
C_ROOT, C_OBJ, C_NV, C_NF, C_AREA, C_M1, C_NRM, C_MIN, C_MAX, C_PEAK, C_CEN, C_M2 = 0, 1, 2, 3, 4, 5, 8, 11, 14, 17, 18, 21
C_RES = 27
SCALE = float(2 ** 44)
DEFAULT_FRAC = 0.75                     # an ASSUMED default, not a measured one
FIELDS = ("key", "object", "root", "n_vertices", "n_faces", "area", "centroid", "normal", "axes", "extent", "box_min",
          "box_max", "peak_vertex", "peak_cos")


def thresholds(minmax, frac: float = DEFAULT_FRAC, min_cos: Optional[float] = None,
               objects: Optional[Sequence[int]] = None) -> np.ndarray:
    """minmax [S, 2] (min, max of the cosine per object) -> thr fp32 [S]: fp32(mn + fp32(frac * fp32(mx - mn))), every
    operation in fp32 (the vertex with normalised similarity >= frac, in the rainbow's own arithmetic); min_cos given: that
    value; NaN (selects nothing) for the objects left out of `objects` (positions; None: all)."""
    mm = np.asarray(minmax, np.float32).reshape(-1, 2)
    S = mm.shape[0]
    if min_cos is not None:
        thr = np.full(S, np.float32(min_cos), np.float32)
    else:
        if not 0.0 <= float(frac) <= 1.0:
            raise ValueError(f"part regions: frac {frac} outside [0, 1]")
        with np.errstate(invalid="ignore", over="ignore"):
            span = (mm[:, 1] - mm[:, 0]).astype(np.float32)
            thr = (mm[:, 0] + (np.float32(frac) * span).astype(np.float32)).astype(np.float32)
    if objects is not None:
        keep = np.zeros(S, bool)
        keep[[int(p) for p in objects]] = True
        thr = np.where(keep, thr, np.float32("nan")).astype(np.float32)
    return thr


def key_to_float(keys) -> np.ndarray:
    """The fp32 behind an order-preserving key (key = ~bits for a set sign bit, else bits | 0x80000000) -> fp64."""
    k = np.asarray(keys, np.int64).astype(np.uint64).astype(np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


def frame_from_covariance(cov: np.ndarray):
    """numpy.linalg.eigh of a symmetric 3 x 3 -> (axes [3, 3] rows by decreasing eigenvalue, extent = sqrt(max(l, 0))).
    Sign: the largest-magnitude component of each axis is made positive, then the third axis is flipped if the frame
    is left-handed."""
    w, U = np.linalg.eigh(cov)
    order = [2, 1, 0]
    axes = U[:, order].T.copy()
    for a in axes:
        if a[int(np.argmax(np.abs(a)))] < 0:
            a *= -1.0
    if np.dot(np.cross(axes[0], axes[1]), axes[2]) < 0:
        axes[2] *= -1.0
    return axes, np.sqrt(np.maximum(w[order], 0.0))


def regions_from_table(table, anchors, keys: Optional[Sequence] = None) -> Dict[str, np.ndarray]:
    """table int64 [R, 32] (objnerf_regions_table's), anchors fp64 [S, 3] (the first vertex of every object), keys: the
    map's object keys by position (None: the positions) -> the fields of PartRegions as numpy arrays, rows in the
    table's order ((object, root) ascending).  All in fp64 from the integers:
      area = area_q / 2^44;  centroid = (anchor + the device's centroid column) + residual / area_q: the column is
      m1 / area_q in fp64, the residual the first moments pass B found about it, so the error is one rounding of 2^-45
      per face over the area wherever the anchor lies (a region without area: the centre of its box);
      normal = the summed area-weighted normal at unit length (zero if the sum is zero);
      covariance = second moments / area_q (zero without area) -> axes, extent (frame_from_covariance)."""
    t = np.asarray(table, np.int64).reshape(-1, ROW)
    anchors = np.asarray(anchors, np.float64).reshape(-1, 3)
    R = t.shape[0]
    obj = t[:, C_OBJ].astype(np.int64)
    area_q = t[:, C_AREA].astype(np.float64)
    has = area_q > 0
    safe = np.where(has, area_q, 1.0)
    box_min = key_to_float(t[:, C_MIN:C_MIN + 3]).reshape(R, 3)
    box_max = key_to_float(t[:, C_MAX:C_MAX + 3]).reshape(R, 3)
    anc = anchors[obj] if R else np.zeros((0, 3))
    cen0 = np.ascontiguousarray(t[:, C_CEN:C_CEN + 3]).view(np.float64).reshape(R, 3)
    centroid = np.where(has[:, None], (anc + cen0) + t[:, C_RES:C_RES + 3].astype(np.float64) / safe[:, None],
                        0.5 * (box_min + box_max))
    n = t[:, C_NRM:C_NRM + 3].astype(np.float64)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    normal = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
    m2 = np.where(has[:, None], t[:, C_M2:C_M2 + 6].astype(np.float64) / safe[:, None], 0.0)
    axes, extent = np.zeros((R, 3, 3)), np.zeros((R, 3))
    for r in range(R):
        xx, xy, xz, yy, yz, zz = m2[r]
        axes[r], extent[r] = frame_from_covariance(np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]))
    peak = t[:, C_PEAK].astype(np.uint64)
    peak_vertex = ((~peak) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    peak_cos = key_to_float((peak >> np.uint64(32)).astype(np.int64))
    key = np.array([keys[p] for p in obj]) if keys is not None and R else obj.copy()
    return {"key": key, "object": obj, "root": t[:, C_ROOT].astype(np.int64), "n_vertices": t[:, C_NV].astype(np.int64),
            "n_faces": t[:, C_NF].astype(np.int64), "area": area_q / SCALE, "centroid": centroid, "normal": normal,
            "axes": axes, "extent": extent, "box_min": box_min, "box_max": box_max, "peak_vertex": peak_vertex,
            "peak_cos": peak_cos}


def filter_rows(area, n_vertices, min_area: float = 0.0, min_vertices: int = 1):
    """-> (keep: the rows that stay, ascending; remap int32 [R + 1]: old row -> new row or -1, with remap[R] = -1 so that
    a label of -1 indexes it)."""
    area, nv = np.asarray(area, np.float64), np.asarray(n_vertices, np.int64)
    ok = (area >= float(min_area)) & (nv >= int(min_vertices))
    keep = np.nonzero(ok)[0]
    remap = np.full(len(ok) + 1, -1, np.int32)
    remap[keep] = np.arange(len(keep), dtype=np.int32)
    return keep, remap


class PartRegions:
    """The regions of one part query.  label: device int32 [V], the row of the vertex's region (after the filter) or -1.
    Per region, numpy, rows sorted by (object, root): key (the map's object key), object (its position), root (the
    smallest packed vertex id), n_vertices, n_faces, area [m^2], centroid [3], normal [3] (unit, or zero), axes [3, 3]
    (rows: principal directions by decreasing spread, right-handed), extent [3] (the standard deviations along them),
    box_min / box_max [3] (of the vertices, at fp32), peak_vertex (packed id), peak_cos.  thr: the thresholds used, fp32
    [S]; status: the device status word (bit 0 / 1: a face with a bad / foreign vertex id was ignored, bit 2: a
    non-finite contribution counted as 0)."""

    def __init__(self, label, fields: Dict[str, np.ndarray], thr: np.ndarray, status: int = 0):
        self.label = label
        for f in FIELDS:
            setattr(self, f, fields[f])
        self.thr = thr
        self.status = int(status)

    def __len__(self) -> int:
        return int(len(self.root))

    def vertices(self, r: int):
        """The packed vertex ids of region r, ascending (a device int64 tensor)."""
        import torch
        return torch.nonzero(self.label == int(r)).reshape(-1)

    def records(self):
        """One plain dict per region (lists and numbers: what regions.json holds)."""
        out = []
        for r in range(len(self)):
            rec = {}
            for f in FIELDS:
                v = getattr(self, f)[r]
                rec[f] = v.tolist() if isinstance(v, np.ndarray) else v.item() if hasattr(v, "item") else v
            out.append(rec)
        return out


def region_colors(label: np.ndarray, rgb: np.ndarray, n_regions: int, dark: float) -> np.ndarray:
    """Per vertex uint8 [n, 3]: instance_palette per region row, RGB x dark where unselected."""
    from .query import instance_palette
    pal = instance_palette(max(int(n_regions), 1))
    col = np.asarray(rgb, np.float64)[:, :3] / 255.0 * dark
    sel = label >= 0
    col[sel] = pal[label[sel]]
    return np.round(col * 255).astype(np.uint8)


def write_regions(out_dir: str, mq, regions: PartRegions, positions: Sequence[int]) -> Dict:
    """regions.json (one record per region) and obj_<id>_regions.ply for the objects at `positions`."""
    from . import mesh as omesh
    from .query import DARK
    doc = {"thr": {str(mq.keys[p]): float(regions.thr[p]) for p in positions}, "status": regions.status,
           "regions": regions.records()}
    with open(os.path.join(out_dir, "regions.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    label = regions.label.cpu().numpy()
    for p in positions:
        k = mq.keys[p]
        r0, r1 = int(mq.seg_host[p]), int(mq.seg_host[p + 1])
        m = mq.all_obj[k]["mesh"]
        out = omesh.TriMesh(m.vertices, m.faces, m.vertex_normals)
        rgb = np.asarray(mq.all_obj[k]["color"], np.uint8).reshape(r1 - r0, -1)
        out.visual.vertex_colors = region_colors(label[r0:r1], rgb, len(regions), DARK)
        out.export(os.path.join(out_dir, f"obj_{k}_regions.ply"))
    return doc


__all__ = ["PartRegions", "thresholds", "regions_from_table", "filter_rows", "frame_from_covariance", "key_to_float",
           "region_colors", "write_regions", "ROW", "DEFAULT_FRAC", "FIELDS"]
