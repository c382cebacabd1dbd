"""Label arbitrary 3-D points against the whole map on the GPU: which object does each point belong to, what class is it,
and what are its colour and 512-d part feature?

    python -m openobj_amd.map_points --logdir DIR --points cloud.{npy,npz,ply} --out DIR
                                     [--color] [--feat] [--gt-class labels.npy] [--bg-ids 0 2 3]

The 3-D counterpart of the z-buffer merge of train.py:550-612 over the checkpoints the mapper writes
(<logdir>/ckpt/<id>/obj_<id>.pth, vmap.py:556-576).  For N world points and K objects in a fixed order:

* point n is a CANDIDATE of object k iff |R_k^T (p_n - c_k)| <= extent_k / 2 component-wise, in fp32 (the object's fitted
  box, "bbox" of the checkpoint);
* its SCORE is alpha = 10 * raw of OccupancyMap.forward (model.py:88) at p_n - obj_center_k; occupied means alpha > 0,
  i.e. occ > 0.5 (trainer.py:71).  The ranking is by alpha, not sigmoid(alpha), which saturates to exactly 1.0f;
* only occupied candidates can WIN.  An occupied foreground candidate beats every background one (train.py:593-594: the
  background never hides an object); the largest alpha wins, equal alphas go to the object that comes first in the
  list.  A point without an occupied candidate gets label -1, colour 0, feature 0 and the largest candidate alpha (or
  -inf without a candidate).

Every object sees only the points inside its box (objnerf_mappoints.hip: count / emit candidate lists, a ragged fused
evaluation of the hidden-32 objects, the wider background through objnerf_eval_points_ws, one 64-bit atomicMax per pair,
and the 512-d head for the winners only) -- against K evaluations of the whole cloud with Trainer.eval_points.

MapPoints.surface and label(want_normal=True) differentiate the map in position (objnerf_mapalign.hip):
d alpha / d p of every candidate pair, the object whose surface is nearest to a point, the outward normal; map_align.py
aligns a cloud to the map with them.

The CLI writes labels.npz (obj, obj_id, class_id, alpha and, when asked for, color, part_feat), instances.ply and
classes.ply (the cloud coloured per instance / per class with query.instance_palette) and, with --gt-class, eval.json
(per-class IoU, mIoU, accuracy)."""
from __future__ import annotations

import argparse
import json
import os
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, mesh, ops, query

DEFAULT_PAIR_BUDGET = 1 << 30          # bytes of per-pair buffers label() keeps alive at once (it halves a chunk that needs more)
DEFAULT_G_MIN = 1e-3                   # ASSUMED default: the floor of |d alpha / d p| (alpha units per metre) in d = alpha / |grad|
FIELD_CHUNK = 1 << 18                  # pairs per round of the layer-wise gradient chain of a wide network


@dataclass
class MapObject:
    """One object of the map: a Trainer holding its network, its oriented box (.center [3], .R [3, 3], .extent [3], as
    stored under "bbox" in obj_<id>.pth), its ids, and the obj_center offset (0 as in map_vis.export)."""
    trainer: object
    bbox: object
    obj_id: int = -1
    class_id: int = -1
    obj_center: float = 0.0


def box_record(bbox, obj_center: float = 0.0) -> np.ndarray:
    """[16] fp32: centre | R row-major | extent / 2 | obj_center -- the form the kernels (and the specification) test."""
    c = np.asarray(bbox.center, np.float64).reshape(-1)
    R = np.asarray(bbox.R, np.float64)
    e = np.asarray(bbox.extent, np.float64).reshape(-1)
    if c.shape != (3,) or R.shape != (3, 3) or e.shape != (3,):
        raise _lib.ObjnerfError(f"map points: a box needs center [3], R [3, 3], extent [3]; got {c.shape}, {R.shape}, {e.shape}")
    rec = np.empty(16, np.float32)
    rec[0:3] = c.astype(np.float32)
    rec[3:12] = R.astype(np.float32).reshape(9)
    rec[12:15] = e.astype(np.float32) * np.float32(0.5)
    rec[15] = np.float32(obj_center)
    return rec


def outward_normal(grad: torch.Tensor) -> torch.Tensor:
    """-grad / |grad| (alpha grows into the object), 0 where |grad| = 0."""
    nrm = grad.norm(dim=-1, keepdim=True)
    return torch.where(nrm > 0, -grad / nrm.clamp(min=1e-30), torch.zeros_like(grad))


def confusion(pred_class: torch.Tensor, gt_class: torch.Tensor, n_classes: int, ignore: int = -1) -> torch.Tensor:
    """[n_classes, n_classes + 1] int64, rows = ground truth, columns = prediction; the last column counts the
    predictions outside [0, n_classes) (an unlabelled point, -1): such a point is a miss of its ground-truth class and a
    false positive of none, and row sums stay the ground-truth counts.  Points whose ground truth is `ignore` or outside
    [0, n_classes) are left out."""
    pred = torch.as_tensor(pred_class).reshape(-1).long()
    gt = torch.as_tensor(gt_class).reshape(-1).long()
    if pred.shape != gt.shape:
        raise ValueError(f"confusion: {tuple(pred.shape)} predictions for {tuple(gt.shape)} labels")
    n = int(n_classes)
    keep = (gt != ignore) & (gt >= 0) & (gt < n)
    pred, gt = pred[keep], gt[keep]
    hit = (pred >= 0) & (pred < n)
    conf = torch.bincount(gt[hit] * n + pred[hit], minlength=n * n).reshape(n, n)
    # the missed points of every class, kept as an extra column so that row sums stay the ground-truth counts
    missed = torch.bincount(gt[~hit], minlength=n).reshape(n, 1)
    return torch.cat([conf, missed], dim=1)


def miou(conf: torch.Tensor):
    """confusion() -> dict: iou [n] (NaN for a class in neither ground truth nor prediction), miou over the others,
    accuracy = correct / counted points."""
    conf = torch.as_tensor(conf).double()
    n = conf.shape[0]
    sq = conf[:, :n]
    tp = sq.diag()
    gt_tot = conf.sum(1)                      # with the missed column
    pred_tot = sq.sum(0)
    union = gt_tot + pred_tot - tp
    iou = torch.where(union > 0, tp / union.clamp(min=1), torch.full_like(tp, float("nan")))
    seen = union > 0
    total = conf.sum()
    return {"iou": iou, "miou": float(iou[seen].mean()) if bool(seen.any()) else float("nan"),
            "accuracy": float(tp.sum() / total) if total > 0 else float("nan")}


class _Pass:
    """Times one pass of label() with device events into stats[name] (ms, summed over chunks); nothing without stats."""

    def __init__(self, stats, name):
        self.stats, self.name = stats, name

    def __enter__(self):
        if self.stats is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if self.stats is not None and exc[0] is None:
            self.e1.record()
            self.e1.synchronize()
            self.stats[self.name] = self.stats.get(self.name, 0.0) + self.e0.elapsed_time(self.e1)


def split_arenas(objects: Sequence[MapObject], stacked, dev):
    """The networks of a map, copied to dev: -> (ONE arena of the hidden-32 objects whose trainer stacked() admits, or None;
    row_of {k: its row there}; own {k: an arena of one row} for every other object)."""
    small = [k for k, o in enumerate(objects) if stacked(o.trainer)]
    row_of = {k: row for row, k in enumerate(small)}
    shape = lambda t: ops.NetShape(int(t.hidden_feature_size), int(t.clip_point_feature_size), t.n_unidir_funcs + 1)
    arena = None
    if small:
        arena = ops.ParamArena(len(small), shape(objects[small[0]].trainer), dev)
        with torch.no_grad():
            for row, k in enumerate(small):
                t = objects[k].trainer
                arena.params[row].copy_(t.arena.params[0].to(dev))
                arena.scale[row] = float(t.obj_scale)
        arena.version += 1
    own = {}
    for k, o in enumerate(objects):
        if k not in row_of:
            t = o.trainer
            own[k] = ops.ParamArena(1, shape(t), dev)
            with torch.no_grad():
                own[k].params.copy_(t.arena.params.to(dev))
                own[k].scale.fill_(float(t.obj_scale))
    return arena, row_of, own


class MapPoints:
    def __init__(self, objects: Sequence[MapObject], device=None, bg_ids: Iterable[int] = (0,),
                 pair_budget_bytes: int = DEFAULT_PAIR_BUDGET):
        objects = list(objects)
        if not objects:
            raise _lib.ObjnerfError("MapPoints: no object")
        for o in objects:
            if o.bbox is None:
                raise _lib.ObjnerfError(f"MapPoints: object {o.obj_id} has no box (from_logdir skips such checkpoints)")
        self.device = torch.device(device if device is not None else objects[0].trainer.device)
        self.objects = objects
        self.K = len(objects)
        self.pair_budget_bytes = int(pair_budget_bytes)
        self._keep_pairs = False         # diagnostic, not part of the interface: keep the last call's (seg, pair_pt,
        self._last_pairs = None          # pair_alpha) in _last_pairs (the tests compare pair values with the oracle)
        bg = set(int(b) for b in bg_ids)
        self.is_bg = [int(o.obj_id) in bg for o in objects]
        self.feat_dim = int(objects[0].trainer.clip_point_feature_size)
        for o in objects:
            h = int(o.trainer.hidden_feature_size)
            if h % 32 != 0:
                raise _lib.ObjnerfError(f"MapPoints: hidden width {h} of object {o.obj_id} is not a multiple of 32")
            if int(o.trainer.clip_point_feature_size) != self.feat_dim:
                raise _lib.ObjnerfError("MapPoints: the objects disagree on the feature width")
        dev = self.device
        self.boxes = torch.from_numpy(np.stack([box_record(o.bbox, o.obj_center) for o in objects])).to(dev)
        self.obj_ids = torch.tensor([int(o.obj_id) for o in objects], dtype=torch.int64, device=dev)
        self.class_ids = torch.tensor([-1 if o.class_id is None else int(o.class_id) for o in objects], dtype=torch.int64,
                                      device=dev)
        # the hidden-32 objects in ONE arena, wider ones (the background) each on its own
        self.arena, row_of, self.wide_arena = split_arenas(objects, lambda t: int(t.hidden_feature_size) == 32, dev)
        self.wide = sorted(self.wide_arena)
        info = np.full((self.K, 2), -1, np.int32)
        info[:, 1] = np.asarray(self.is_bg, np.int32)
        for k, row in row_of.items():
            info[k, 0] = row
        self.info_host = info
        self.info = torch.from_numpy(info).to(dev)

    @classmethod
    def from_logdir(cls, logdir: str, device="cuda:0", bg_ids: Iterable[int] = (0,), **kw) -> "MapPoints":
        from . import map_vis
        objects = []
        for obj_id, t, ck, box in map_vis.iter_checkpoints(logdir, device):
            sem = ck.get("semantic_id")
            objects.append(MapObject(t, box, obj_id=obj_id, class_id=-1 if sem is None else int(sem)))
        return cls(objects, device=device, bg_ids=bg_ids, **kw)

    # ------------------------------------------------------------------------------------------------------------
    def _pair_bytes(self, seg: List[int], want_color: bool, want_feat: bool, want_normal: bool = False) -> int:
        per = 8 + (12 if want_color else 0) + (128 if want_feat else 0)        # pair_pt, alpha | colour | hidden-32 rows
        total = seg[-1] * per
        for k in self.wide:
            total += ops.mappoints_wide_bytes(self.wide_arena[k], seg[k + 1] - seg[k], want_feat)
        if want_normal:
            total += self._field_bytes(seg) - 4 * seg[-1]                       # (pair_pt is counted above)
        return total

    def _field_bytes(self, seg: List[int]) -> int:
        """pair_pt, pair_alpha, pair_grad, and the layer-wise chain of the widest chunk of a wide segment."""
        total = seg[-1] * 20
        wide = [ops.field_grad_layerwise_bytes(self.wide_arena[k], seg[k + 1] - seg[k], FIELD_CHUNK) for k in self.wide]
        return total + (max(wide) if wide else 0)

    def _pair_field(self, p: torch.Tensor, seg_off: torch.Tensor, seg: List[int], pair_pt: torch.Tensor, stats=None):
        """pair_alpha [M] and pair_grad [M, 3] = d alpha / d p of every candidate pair: the hidden-32 objects in one fused
        launch (objnerf_mappoints_grad), a wider network (the hidden-128 background) through the layer-wise chain on its
        contiguous segment -- the slow path, in chunks of FIELD_CHUNK pairs."""
        dev, M = p.device, seg[-1]
        pair_alpha, pair_grad = torch.empty(M, device=dev), torch.empty(M, 3, device=dev)
        with _Pass(stats, "grad32_ms"):
            if self.arena is not None and M:
                ops.mappoints_grad(self.arena, p, self.boxes, self.info, seg_off, pair_pt, pair_alpha, pair_grad)
        with _Pass(stats, "grad_wide_ms"):
            for k in self.wide:
                a, b = seg[k], seg[k + 1]
                if b > a:
                    gpts = ops.mappoints_gather(p, pair_pt[a:b], self.objects[k].obj_center)
                    pair_alpha[a:b], pair_grad[a:b] = ops.field_grad_layerwise(self.wide_arena[k], gpts, FIELD_CHUNK)
        return pair_alpha, pair_grad

    def _label_range(self, pts: torch.Tensor, out, lo: int, hi: int, want_color: bool, want_feat: bool, stats=None,
                     want_normal: bool = False) -> None:
        """Points [lo, hi): split in halves while the pair buffers would exceed the budget or the pairs the 31 bits of the
        keys (a point's result does not depend on which other points share its call)."""
        p = pts[lo:hi]
        with _Pass(stats, "candidates_ms"):
            seg_off, seg, ws = ops.mappoints_count(p, self.boxes)
        # decided on the counts alone, before anything of M entries exists: too many pairs for the keys, or for the budget
        if hi - lo > 1 and (seg[-1] > ops.MAPPOINTS_MAX_PAIRS or
                            self._pair_bytes(seg, want_color, want_feat, want_normal) > self.pair_budget_bytes):
            del ws
            mid = (lo + hi) // 2
            self._label_range(pts, out, lo, mid, want_color, want_feat, stats, want_normal)
            self._label_range(pts, out, mid, hi, want_color, want_feat, stats, want_normal)
            return
        with _Pass(stats, "candidates_ms"):
            pair_pt = ops.mappoints_emit(p, self.boxes, ws, seg[-1])
        del ws
        dev, n, M = p.device, hi - lo, seg[-1]
        best = torch.zeros(n, dtype=torch.int64, device=dev)
        pair_alpha = torch.empty(M, device=dev)
        pair_color = torch.empty(M, 3, device=dev) if want_color else None
        pair_hfeat = torch.empty(M, 32, device=dev) if (want_feat and self.arena is not None) else None
        if stats is not None:
            stats["pairs"] = stats.get("pairs", 0) + M
            stats["pairs32"] = stats.get("pairs32", 0) + sum(seg[k + 1] - seg[k] for k in range(self.K) if k not in self.wide_arena)
            stats["calls"] = stats.get("calls", 0) + 1
        with _Pass(stats, "eval32_ms"):
            if self.arena is not None and M:
                ops.mappoints_eval(self.arena, p, self.boxes, self.info, seg_off, pair_pt, pair_alpha, pair_color,
                                   pair_hfeat, best)
        wide_h = {}
        with _Pass(stats, "wide_ms"):
            for k in self.wide:
                wide_h[k] = ops.mappoints_wide(self.wide_arena[k], p, pair_pt, seg[k], seg[k + 1] - seg[k],
                                               self.objects[k].obj_center, self.is_bg[k], pair_alpha, pair_color,
                                               want_feat, best)
        if self._keep_pairs:
            self._last_pairs = dict(seg=seg, pair_pt=pair_pt, pair_alpha=pair_alpha)
        with _Pass(stats, "resolve_ms"):
            obj, alpha, win, color = ops.mappoints_resolve(best, seg_off, pair_color, M, want_pair=want_normal)
        out["obj"][lo:hi] = obj
        out["alpha"][lo:hi] = alpha
        if want_normal:
            # the winner's d alpha / d p: the gradients of every pair (their own alpha buffer: pair_alpha above stays as
            # it is), read at the winning pair
            grad = torch.zeros(n, 3, device=dev)
            if M:
                _, pair_grad = self._pair_field(p, seg_off, seg, pair_pt, stats)
                if self._keep_pairs:
                    self._last_pairs["pair_grad"] = pair_grad
                    self._last_pairs["out_pair"] = win
                grad = torch.where((win >= 0)[:, None], pair_grad[win.clamp(min=0).long()], grad)
            out["grad"][lo:hi] = grad
        if want_color:
            out["color"][lo:hi] = color
        if want_feat and M:
            heads = []
            for k in range(self.K):
                a = self.wide_arena[k] if k in self.wide_arena else self.arena
                row = 0 if k in self.wide_arena else int(self.info_host[k, 0])
                v = a.views()
                hf, row0 = (wide_h[k], seg[k]) if k in self.wide_arena else (pair_hfeat, 0)
                heads.append((v[16][row], v[17][row], hf, row0, a.net.hidden))
            with _Pass(stats, "head_ms"):
                ops.mappoints_head(best, seg_off, pair_pt, heads, self.feat_dim, out["part_feat"][lo:hi])

    def label(self, points, want_color: bool = False, want_feat: bool = False, normalise_feat: bool = False,
              chunk: Optional[int] = None, stats: Optional[dict] = None, want_normal: bool = False):
        """points [N, 3] -> dict of device tensors: obj int32 [N] (position in the object list, -1 unlabelled), obj_id and
        class_id int64 [N] (-1 unlabelled), alpha fp32 [N], color [N, 3] (want_color), part_feat [N, C] (want_feat; the raw
        out_clip output of the winner, L2-normalised per labelled point with normalise_feat, as map_vis does).
        chunk: points per call (None: the whole cloud); a call whose pair buffers would exceed pair_budget_bytes is halved
        until they fit.  Chunked and unchunked results are bit-equal.
        stats: DIAGNOSTIC, for tools/mappoints_bench.py -- a dict that receives the time of every pass (device events and a
        synchronise per pass, which a normal call does not pay), the number of pairs and of calls.
        want_normal: two more outputs -- grad [N, 3], the winner's d alpha / d p, and normal [N, 3] = -grad / |grad| (outward:
        alpha grows into the object; the sign of ops.marching_cubes); 0 for an unlabelled point or |grad| = 0.  Without the
        flag the call issues exactly the launches it issued before the flag existed."""
        pts = torch.as_tensor(points)
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise _lib.ObjnerfError(f"MapPoints.label: expected points [N, 3], got {tuple(pts.shape)}")
        if chunk is not None and int(chunk) < 1:
            raise _lib.ObjnerfError(f"MapPoints.label: chunk = {chunk}")
        pts = pts.to(self.device, torch.float32).contiguous()
        N, dev = int(pts.shape[0]), self.device
        out = {"obj": torch.empty(N, dtype=torch.int32, device=dev), "alpha": torch.empty(N, device=dev)}
        if want_color:
            out["color"] = torch.empty(N, 3, device=dev)
        if want_feat:
            out["part_feat"] = torch.zeros(N, self.feat_dim, device=dev)
        if want_normal:
            out["grad"] = torch.zeros(N, 3, device=dev)
        step = N if chunk is None else int(chunk)
        with torch.no_grad():
            for lo in range(0, N, max(step, 1)):
                self._label_range(pts, out, lo, min(lo + step, N), want_color, want_feat, stats, want_normal)
            if want_normal:
                out["normal"] = outward_normal(out["grad"])
            o = out["obj"].long()
            lab = o >= 0
            out["obj_id"] = torch.where(lab, self.obj_ids[o.clamp(min=0)], torch.full_like(o, -1))
            out["class_id"] = torch.where(lab, self.class_ids[o.clamp(min=0)], torch.full_like(o, -1))
            if want_feat and normalise_feat:
                f = out["part_feat"]
                nrm = f.norm(dim=-1, keepdim=True)
                out["part_feat"] = torch.where(lab[:, None], f / nrm.clamp(min=1e-30), f)      # map_vis.py:69; unlabelled rows stay 0
        return out

    # ------------------------------------------------------------------------------------------------------------
    def _surface_range(self, pts: torch.Tensor, out, lo: int, hi: int, g_min: float, stats=None) -> None:
        """Points [lo, hi) of surface(): halved like _label_range while the pair buffers exceed the budget."""
        p = pts[lo:hi]
        with _Pass(stats, "candidates_ms"):
            seg_off, seg, ws = ops.mappoints_count(p, self.boxes)
        if hi - lo > 1 and (seg[-1] > ops.MAPPOINTS_MAX_PAIRS or self._field_bytes(seg) > self.pair_budget_bytes):
            del ws
            mid = (lo + hi) // 2
            self._surface_range(pts, out, lo, mid, g_min, stats)
            self._surface_range(pts, out, mid, hi, g_min, stats)
            return
        with _Pass(stats, "candidates_ms"):
            pair_pt = ops.mappoints_emit(p, self.boxes, ws, seg[-1])
        del ws
        n, M = hi - lo, seg[-1]
        if stats is not None:
            stats["pairs"] = stats.get("pairs", 0) + M
            stats["pairs32"] = stats.get("pairs32", 0) + sum(seg[k + 1] - seg[k] for k in range(self.K) if k not in self.wide_arena)
            stats["calls"] = stats.get("calls", 0) + 1
        pair_alpha, pair_grad = self._pair_field(p, seg_off, seg, pair_pt, stats)
        best = torch.full((n,), -1, dtype=torch.int64, device=p.device)          # all ones: no pair yet
        with _Pass(stats, "select_ms"):
            ops.mapalign_select(n, pair_pt, pair_alpha, pair_grad, g_min, best)
            obj, pair, d, alpha, grad = ops.mapalign_resolve(best, seg_off, pair_alpha, pair_grad, g_min,
                                                             want_pair=self._keep_pairs)
        if self._keep_pairs:
            self._last_pairs = dict(seg=seg, pair_pt=pair_pt, pair_alpha=pair_alpha, pair_grad=pair_grad, out_pair=pair)
        out["obj"][lo:hi] = obj
        out["d"][lo:hi] = d
        out["alpha"][lo:hi] = alpha
        out["grad"][lo:hi] = grad

    def surface(self, points, g_min: float = DEFAULT_G_MIN, chunk: Optional[int] = None, stats: Optional[dict] = None):
        """points [N, 3] -> dict of device tensors: for every point the candidate object whose surface (the zero level set
        of alpha) is nearest -- obj int32 [N] (position in the list) and obj_id int64 [N]; d [N], the signed distance
        estimate alpha / max(|grad|, g_min) in metres, positive inside; normal [N, 3] = -grad / |grad| (outward); alpha [N]
        and grad [N, 3] = d alpha / d p of that object.  A point in no box gets -1 / inf / 0.  The smallest |d| wins, equal
        |d| goes to the object that comes first in the list.  g_min keeps d finite where the field is flat."""
        pts = torch.as_tensor(points)
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise _lib.ObjnerfError(f"MapPoints.surface: expected points [N, 3], got {tuple(pts.shape)}")
        if chunk is not None and int(chunk) < 1:
            raise _lib.ObjnerfError(f"MapPoints.surface: chunk = {chunk}")
        if not g_min > 0:
            raise _lib.ObjnerfError(f"MapPoints.surface: g_min = {g_min}")
        pts = pts.to(self.device, torch.float32).contiguous()
        N, dev = int(pts.shape[0]), self.device
        out = {"obj": torch.empty(N, dtype=torch.int32, device=dev), "d": torch.empty(N, device=dev),
               "alpha": torch.empty(N, device=dev), "grad": torch.empty(N, 3, device=dev)}
        step = N if chunk is None else int(chunk)
        with torch.no_grad():
            for lo in range(0, N, max(step, 1)):
                self._surface_range(pts, out, lo, min(lo + step, N), float(g_min), stats)
            o = out["obj"].long()
            out["obj_id"] = torch.where(o >= 0, self.obj_ids[o.clamp(min=0)], torch.full_like(o, -1))
            out["normal"] = outward_normal(out["grad"])
        return out


# ----------------------------------------------------------------------------------------------------------------- CLI
def read_points(path: str) -> np.ndarray:
    if path.endswith(".npy"):
        p = np.load(path)
    elif path.endswith(".npz"):
        d = np.load(path)
        p = d["points"] if "points" in d.files else d[d.files[0]]
    elif path.endswith(".ply"):
        p = mesh.read_ply(path)[0]
    else:
        raise ValueError(f"--points: unsupported extension in {path} (.npy, .npz or .ply)")
    p = np.asarray(p, np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"--points: expected [N, 3], got {p.shape}")
    return np.ascontiguousarray(p)


def write_cloud(path: str, points: np.ndarray, ids: np.ndarray) -> None:
    """The cloud coloured by id through query.instance_palette (grey for -1), with the existing PLY writer."""
    uniq = np.unique(ids[ids >= 0])
    pal = query.instance_palette(len(uniq))
    col = np.full((len(points), 3), 0.4)
    if len(uniq):
        pos = np.searchsorted(uniq, np.where(ids >= 0, ids, uniq[0]))
        col = np.where((ids >= 0)[:, None], pal[pos], col)
    m = mesh.TriMesh(points, np.zeros((0, 3), np.int64))
    m.visual.vertex_colors = (col * 255).astype(np.uint8)
    m.export(path)


def evaluate(pred_class: torch.Tensor, gt_class: torch.Tensor, n_classes: Optional[int] = None, ignore: int = -1):
    pred, gt = torch.as_tensor(pred_class).cpu().long(), torch.as_tensor(gt_class).cpu().long()
    if n_classes is None:
        n_classes = int(max(int(pred.max()), int(gt.max()))) + 1
    r = miou(confusion(pred, gt, n_classes, ignore))
    return {"n_classes": int(n_classes), "miou": r["miou"], "accuracy": r["accuracy"],
            "iou": [None if bool(torch.isnan(v)) else float(v) for v in r["iou"]]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--logdir", required=True)
    ap.add_argument("--points", required=True, help="cloud.npy / .npz / .ply, [N, 3] world coordinates")
    ap.add_argument("--out", required=True)
    ap.add_argument("--color", action="store_true")
    ap.add_argument("--feat", action="store_true")
    ap.add_argument("--gt-class", default=None, help="labels.npy, int [N]; -1 is ignored")
    ap.add_argument("--bg-ids", type=int, nargs="*", default=[0])
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    points = read_points(a.points)
    mp = MapPoints.from_logdir(a.logdir, a.device, bg_ids=a.bg_ids)
    res = mp.label(points, want_color=a.color, want_feat=a.feat, normalise_feat=a.feat, chunk=a.chunk)
    os.makedirs(a.out, exist_ok=True)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    np.savez(os.path.join(a.out, "labels.npz"), **host)
    write_cloud(os.path.join(a.out, "instances.ply"), points, host["obj_id"])
    write_cloud(os.path.join(a.out, "classes.ply"), points, host["class_id"])
    print(f"{len(points)} points, {int((host['obj'] >= 0).sum())} labelled, {mp.K} objects")
    if a.gt_class:
        gt = np.load(a.gt_class).reshape(-1)
        if gt.shape[0] != len(points):
            raise ValueError(f"--gt-class: {gt.shape[0]} labels for {len(points)} points")
        ev = evaluate(res["class_id"], torch.from_numpy(gt.astype(np.int64)))
        with open(os.path.join(a.out, "eval.json"), "w") as fh:
            json.dump(ev, fh, indent=1)
        print(f"mIoU {ev['miou']:.4f}, accuracy {ev['accuracy']:.4f}")
    return res


if __name__ == "__main__":
    main()
