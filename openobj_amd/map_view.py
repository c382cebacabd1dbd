"""A novel view of the whole map in one launch chain on the GPU: the colour, depth and mask-id images of the reference's
`cfg.if_render` loop (train.py:550-612) over the checkpoints the mapper writes (<logdir>/ckpt/<id>/obj_<id>.pth).

    python -m openobj_amd.map_view --logdir DIR --config scene.json [--frames a:b:s] --out DIR [--bg-ids 0]
                                   [--queries FILE.npz [--save-sims]]

The loop renders one object at a time (sceneObject.render_2D_syn: the box test over every pixel, a read-back, one
launch, three copies to the host) and merges four [W, H] images per object in numpy.  MapView.render does the same view
in three stages (objnerf_mapview.hip):

1. the candidate rays of ALL objects in one pass -- a CSR over the objects in their order, ascending in the pixel
   p = w * H + h inside an object, one read-back (seg_off) per view; an object with at most one hit ray is dropped, as
   the reference drops it (trainer.py:164-165);
2. ONE segmented launch of the fused renderer over every hidden-32 fp32 object; an object that kernel does not take (a
   wider network such as the hidden-128 background, trainer.render_bf16 = True) runs the launches render_2D_syn runs
   for it -- the layer-wise chain in ray chunks, or the bf16 renderer -- on its own segment of the CSR;
3. the merge on the device in closed form (render_view.merge_closed_form states and argues it): integer atomicMin /
   atomicMax only, so the images do not depend on scheduling.

With the same draws the images equal render_view.render_view's bit for bit, in every object order; in a seeded run too,
since every object that renders takes its Philox draw counter at its turn in the order, as the loop does.

The CLI writes rgb_<id>.png, depth_<id>.png and maskid_<id>.png per frame, transposed back to [H, W] as train.py:599-611
does (depth_<id>.png is what cv2.imwrite makes of the float image there: metres rounded and saturated to 8 bits;
--depth-scale S writes round(depth * S) in 16 bits instead).  The contour overlay mask_<id>.png of train.py:588-590,612
needs OpenCV's findContours / drawContours and is not written.

The 512-d part-feature image (render_2D_syn's render_partfeat) is never stored densely: it is 1.6 GB per 1200 x 680
view.  MapView.render(want_feat=True) keeps the composited H-wide feature hidden of every entry instead; the head is
linear, so one kernel over the winning entries (objnerf_view_query) forms each pixel's feature in
registers and writes only what is asked for: MapView.query -- cosines against up to 16 query vectors per launch and
the arg-max label image -- and MapView.features -- the raw rows for a pixel list.

    ... --queries FILE.npz [--save-sims]

FILE.npz holds feats [Q, 512] (text or image embeddings computed elsewhere) and optionally names [Q]; per frame
label_<id>.png is written (uint8 [H, W]: the best-matching query + 1, 0 = nothing painted) and, with --save-sims,
sim_<id>.npy (fp32 [Q, H, W], NaN where nothing painted); without that flag the cosines never leave the device."""
from __future__ import annotations

import argparse
import os
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from .map_points import MapObject, _Pass, split_arenas
from .render_view import ViewBuffers

N_BINS = 150          # Trainer.sample_points_bbox(do_eval=True), trainer.py:145-146


def view_box_record(bbox, T_WC: torch.Tensor) -> torch.Tensor:
    """[16] fp32 on the host: T_OC rows 0..2 | extent / 2 | 0 -- formed as Trainer.sample_points_bbox forms them
    (trainer.py:67-72 here: T_OC = inverse(T_WO) @ T_WC in fp32 on the CPU, the half extent halved in fp64)."""
    T_WO = torch.eye(4)
    T_WO[:3, :3] = torch.as_tensor(np.asarray(bbox.R))
    T_WO[:3, 3] = torch.as_tensor(np.asarray(bbox.center))
    T_OC = torch.inverse(T_WO) @ T_WC
    half = torch.as_tensor(np.asarray(bbox.extent, np.float64) / 2.0).float()
    rec = torch.zeros(16)
    rec[:12] = T_OC[:3].reshape(12)
    rec[12:15] = half.reshape(3)
    return rec


class MapView:
    def __init__(self, objects: Sequence[MapObject], device=None, bg_ids: Iterable[int] = (0,),
                 class_of: Optional[Dict[int, int]] = None):
        """objects: the map IN THE ORDER TO RENDER (the dict order of train.py:570: the merge depends on it).  bg_ids:
        objects that paint colour and id but never depth (train.py:593-594).  class_of: obj_id -> the id written into
        the mask-id image (mapping_class of train.py:592; an object it does not name writes its obj_id).  The networks
        are copied here: a later change of a trainer's weights does not reach this MapView."""
        objects = list(objects)
        if not objects:
            raise _lib.ObjnerfError("MapView: no object")
        for o in objects:
            if o.bbox is None:
                raise _lib.ObjnerfError(f"MapView: object {o.obj_id} has no box (from_logdir skips such checkpoints)")
        self.device = dev = torch.device(device if device is not None else objects[0].trainer.device)
        self.objects, self.K = objects, len(objects)
        self.order = [int(o.obj_id) for o in objects]
        bg = set(int(b) for b in bg_ids)
        self.is_bg = [i in bg for i in self.order]
        class_of = class_of or {}
        info = np.zeros((self.K, 2), np.int32)
        info[:, 0] = np.asarray(self.is_bg, np.int32)
        info[:, 1] = [int(class_of.get(i, i)) for i in self.order]
        self.info = torch.from_numpy(info).to(dev)
        self.feat_dim = int(objects[0].trainer.clip_point_feature_size)

        def fused(t):       # what objnerf_render_fwd_segmented takes
            return int(t.hidden_feature_size) == 32 and int(t.n_unidir_funcs) + 1 == 6 and \
                int(t.clip_point_feature_size) == self.feat_dim and not bool(getattr(t, "render_bf16", False))

        self.arena, self.row_of, self.own_arena = split_arenas(objects, fused, dev)
        self.own_bf16 = {k: bool(getattr(objects[k].trainer, "render_bf16", False)) for k in self.own_arena}
        # out_clip of every object (of_w [C, H], of_b [C]) as tensors of their own: objnerf_view_query reads them with
        # 128-bit loads, which an arena offset does not promise
        self.heads = []
        for k in range(self.K):
            v = self.arena.views() if k in self.row_of else self.own_arena[k].views()
            r = self.row_of.get(k, 0)
            self.heads.append((v[16][r].clone().contiguous(), v[17][r].clone().contiguous()))
        self.winner = self.seg_off = self.seg = self.csr = self.own_hfeat = None
        self._shape = None

    @classmethod
    def from_logdir(cls, logdir: str, device="cuda:0", bg_ids: Iterable[int] = (0,), class_of=None,
                    semantic_ids: bool = False) -> "MapView":
        """The checkpoints of <logdir>/ckpt in ascending id order (map_vis.load_object).  semantic_ids: write each
        object's semantic_id into the mask-id image where class_of does not name it."""
        from . import map_vis
        objects, class_of = [], dict(class_of or {})
        for obj_id, t, ck, box in map_vis.iter_checkpoints(logdir, device):
            sem = ck.get("semantic_id")
            if semantic_ids and sem is not None:
                class_of.setdefault(obj_id, int(sem))
            objects.append(MapObject(t, box, obj_id=obj_id, class_id=-1 if sem is None else int(sem)))
        return cls(objects, device=device, bg_ids=bg_ids, class_of=class_of)

    # ------------------------------------------------------------------------------------------------------------
    def _render_own(self, k: int, origin, dirs_W, near, far, u, seed: int, draw: int, csr, want_feat: bool = False):
        """Object k on its own segment of the CSR with the launches sceneObject.render_2D_syn runs for it
        (vmap.py:322-348 here): the bf16 renderer, or -- a wider network -- the layer-wise chain in ray chunks.
        want_feat: -> the composited feature hidden [n, H] of the segment, as render_part=True gets it there."""
        from . import vmap
        a, lo, hi = self.own_arena[k], self.seg[k], self.seg[k + 1]
        dW, nr, fr = dirs_W[lo:hi], near[lo:hi], far[lo:hi]
        if a.net.hidden == 32 and a.net.n_freqs == 6:
            o = ops.render_fwd(a, origin, dW, nr, fr, u, N_BINS, seed=seed, draw=draw, want_hfeat=want_feat,
                               bf16=self.own_bf16[k])
            csr["depth"][lo:hi], csr["opacity"][lo:hi], csr["rgb"][lo:hi] = o["depth"], o["opacity"], o["rgb"]
            return o["vals"]
        n, S = hi - lo, N_BINS - 1
        z, pts = ops.box_points(origin, dW, nr, fr, u, N_BINS, seed=seed, draw=draw)
        rays_per_chunk = max(1, vmap.RENDER_SAMPLES_PER_CHUNK // S)
        fh = torch.empty(n, a.net.hidden, device=self.device) if want_feat else None
        for r0 in range(0, n, rays_per_chunk):
            r1 = min(n, r0 + rays_per_chunk)
            alpha, color, hfeat, _ = ops.eval_points(a, pts[r0:r1].reshape(1, -1, 3), want_hfeat=want_feat)
            o = ops.composite(alpha.reshape(r1 - r0, S), color.reshape(r1 - r0, S, 3), z[r0:r1],
                              vals=hfeat.reshape(r1 - r0, S, -1) if want_feat else None)
            csr["depth"][lo + r0:lo + r1], csr["opacity"][lo + r0:lo + r1] = o["depth"], o["opacity"]
            csr["rgb"][lo + r0:lo + r1] = o["rgb"]
            if want_feat:
                fh[r0:r1] = o["vals"]
        return fh

    def render(self, T_WC, rays_dir, draws: Optional[Dict[int, object]] = None, to_host: bool = True,
               stats: Optional[dict] = None, _workgroups: int = 0, want_feat: bool = False):
        """T_WC [4, 4], rays_dir [W, H, 3] (cameraInfo.rays_dir_cache) -> ViewBuffers (rgb uint8 [W, H, 3], maskid int32
        [W, H], depth fp32 [W, H]; to_host=False: a dict of the same three as device tensors plus "winner").
        draws: obj_id -> [n_hit, 150] injected uniforms replacing the stratified draws of that object (tests); an
        object without an entry draws inside the kernels under the process seed and its own draw counter.
        Afterwards .seg_off / .seg (the CSR offsets over .order, device / list), .csr (pix, dirs_W, near, far, depth,
        opacity, rgb per entry) and .winner (int32 [W, H]: the entry that painted the pixel, -1 = none) describe the
        view.  want_feat: also keep the composited feature hidden of every entry -- .csr["hfeat"] [M, 32] for the objects of
        the segmented launch, .own_hfeat[k] [n_k, H] for every other object k (position in .order) -- which .query and
        .features need; the images keep their bytes.  stats: DIAGNOSTIC, for tools/view_bench.py -- receives the time of every stage (device events and a
        synchronise per stage, which a normal call does not pay) and the entry counts."""
        dev = self.device
        rays = torch.as_tensor(rays_dir)
        if rays.dim() != 3 or rays.shape[2] != 3:
            raise _lib.ObjnerfError(f"MapView.render: expected rays_dir [W, H, 3], got {tuple(rays.shape)}")
        W, H = int(rays.shape[0]), int(rays.shape[1])
        with torch.no_grad():
            with _Pass(stats, "rays_ms"):
                dirs_C = rays.to(dev, torch.float32).reshape(-1, 3).contiguous()
                T = torch.as_tensor(T_WC, dtype=torch.float32).cpu().reshape(4, 4)
                boxes = torch.stack([view_box_record(o.bbox, T) for o in self.objects]).to(dev)
                T_dev = T.to(dev)
                seg_off, seg, ws = ops.view_rays_count(T_dev, boxes, dirs_C)           # the one host sync of the view
                M = seg[-1]
                pix, dirs_W, near, far = ops.view_rays_emit(T_dev, boxes, dirs_C, ws, M)
            del ws
            self.seg_off, self.seg = seg_off, seg
            origin = T[:3, 3]
            csr = dict(pix=pix, dirs_W=dirs_W, near=near, far=far, depth=torch.empty(M, device=dev),
                       opacity=torch.empty(M, device=dev), rgb=torch.empty(M, 3, device=dev))
            seed = ops._seed_of(None)
            rows, u_parts, u_lo, own_hfeat = [], [], 0, {}
            # dict order, AFTER the count: an object that renders takes its draw counter at its turn (one with at most
            # one hit takes none), so a seeded run draws what the per-object loop draws
            with _Pass(stats, "own_ms"):
                for k, o in enumerate(self.objects):
                    n = seg[k + 1] - seg[k]
                    if n == 0:
                        continue
                    u = None if draws is None else draws.get(o.obj_id)
                    if u is not None:
                        u = torch.as_tensor(u).to(dev, torch.float32).contiguous()
                        if tuple(u.shape) != (n, N_BINS):
                            raise _lib.ObjnerfError(f"MapView.render: draws[{o.obj_id}] is {tuple(u.shape)}, the object "
                                                    f"has {n} rays of {N_BINS} bins")
                    draw = 0 if u is not None else (ops._next_offset() & 0x1FFFFFFF)
                    if k in self.row_of:
                        rows.append((self.row_of[k], seg[k], seg[k + 1], u_lo if u is not None else None, draw))
                        if u is not None:
                            u_parts.append(u)
                            u_lo += n
                    else:
                        own_hfeat[k] = self._render_own(k, origin, dirs_W, near, far, u, seed, draw, csr, want_feat)
            with _Pass(stats, "render32_ms"):
                if rows:
                    u_all = (u_parts[0] if len(u_parts) == 1 else torch.cat(u_parts)) if u_parts else None
                    if want_feat:
                        csr["hfeat"] = torch.empty(M, 32, device=dev)
                    ops.render_fwd_segmented(self.arena, origin, dirs_W, near, far, rows, u_all, N_BINS, seed=seed, out=csr,
                                             _workgroups=_workgroups, want_hfeat=want_feat)
            with _Pass(stats, "merge_ms"):
                out = ops.view_merge(seg_off, pix, csr["depth"], csr["opacity"], csr["rgb"], near, far, self.info, W * H,
                                     any_background=any(self.is_bg))
            if stats is not None:
                stats["entries"] = stats.get("entries", 0) + M
                stats["entries32"] = stats.get("entries32", 0) + sum(r[2] - r[1] for r in rows)
            self.csr = csr
            self.own_hfeat = own_hfeat if want_feat else None
            self._shape = (W, H)
            self.winner = out["winner"].reshape(W, H)
            res = dict(rgb=out["rgb"].reshape(W, H, 3), maskid=out["maskid"].reshape(W, H), depth=out["depth"].reshape(W, H),
                       winner=self.winner)
            if not to_host:
                return res
            with _Pass(stats, "to_host_ms"):
                buf = ViewBuffers.__new__(ViewBuffers)
                buf.rgb, buf.maskid, buf.depth = (res[k].cpu().numpy() for k in ("rgb", "maskid", "depth"))
            return buf

    # ------------------------------------------------------------------------------------------------------------
    def _view_heads(self):
        """The head table of the last view for ops.view_query."""
        if self.csr is None or self.own_hfeat is None:
            raise _lib.ObjnerfError("MapView: the last view was not rendered with want_feat=True")
        heads = []
        for k, (of_w, of_b) in enumerate(self.heads):
            if self.seg[k + 1] == self.seg[k]:
                heads.append((of_w, of_b, None, 0))
            elif k in self.row_of:
                heads.append((of_w, of_b, self.csr["hfeat"], 0))            # CSR-aligned: row = entry
            else:
                heads.append((of_w, of_b, self.own_hfeat[k], self.seg[k]))
        return heads

    def query(self, queries, want_sims: bool = True, _workgroups: int = 0) -> Dict[str, Optional[torch.Tensor]]:
        """The last rendered view (want_feat=True) against queries [Q, C] (any length; normalised here, as
        MapQuery._query does): -> dict(sims [Q, W, H] | None (want_sims), label int32 [W, H] = the first arg-max over the
        queries, best [W, H] = that cosine) as device tensors; NaN / -1 where nothing painted.  The 512-d feature of a
        pixel exists in registers only (objnerf_view_query); more than 16 queries run in chunks of 16."""
        heads = self._view_heads()
        q = (queries if torch.is_tensor(queries) else torch.as_tensor(np.asarray(queries, np.float32))).to(self.device, torch.float32)
        if q.dim() != 2 or int(q.shape[1]) != self.feat_dim or int(q.shape[0]) < 1:
            raise _lib.ObjnerfError(f"MapView.query: queries [Q >= 1, {self.feat_dim}], got {tuple(q.shape)}")
        q = (q / q.norm(dim=-1, keepdim=True)).contiguous()
        (W, H), c = self._shape, self.csr
        sims, label, best = [], None, None
        for q0 in range(0, int(q.shape[0]), ops.VIEW_QUERY_MAX):
            o = ops.view_query(self.seg_off, c["pix"], c["opacity"], self.winner, heads, q[q0:q0 + ops.VIEW_QUERY_MAX],
                               want_sims=want_sims, _workgroups=_workgroups)
            sims.append(o["sims"])
            if label is None:
                label, best = o["label"], o["best"]
            else:       # the first arg-max across chunks: a later chunk wins only if strictly better (or the first NaN)
                better = (o["best"] > best) | (torch.isnan(o["best"]) & ~torch.isnan(best))
                label = torch.where(better, o["label"] + q0, label)
                best = torch.where(better, o["best"], best)
        return dict(sims=torch.cat(sims).reshape(-1, W, H) if want_sims else None, label=label.reshape(W, H),
                    best=best.reshape(W, H))

    def features(self, pixels) -> torch.Tensor:
        """The part feature (render_2D_syn's render_partfeat, vmap.py:678) at chosen pixels of the last rendered view
        (want_feat=True).  pixels: [n, 2] as (w, h), or flat p = w * H + h -> [n, C] on the device; a pixel outside the
        view or one nothing painted gets zeros."""
        heads = self._view_heads()
        W, H = self._shape
        px = torch.as_tensor(pixels).to(self.device)
        if px.dim() == 2 and int(px.shape[1]) == 2:
            w, h = px[:, 0].long(), px[:, 1].long()
            px = torch.where((w >= 0) & (w < W) & (h >= 0) & (h < H), w * H + h, torch.full_like(w, -1))
        elif px.dim() != 1:
            raise _lib.ObjnerfError(f"MapView.features: pixels [n, 2] as (w, h) or flat [n], got {tuple(px.shape)}")
        c = self.csr
        return ops.view_query(self.seg_off, c["pix"], c["opacity"], self.winner, heads, pixels=px.long().contiguous())["feat"]


# ----------------------------------------------------------------------------------------------------------------- CLI
def depth_png(depth: np.ndarray, scale: Optional[float]) -> np.ndarray:
    """The depth image as written: 8 bits, metres rounded to nearest-even and saturated (what cv2.imwrite makes of the
    float image of train.py:610), or round(depth * scale) saturated to 16 bits."""
    if scale is None:
        return np.clip(np.rint(depth), 0, 255).astype(np.uint8)
    return np.clip(np.rint(depth.astype(np.float64) * float(scale)), 0, 65535).astype(np.uint16)


def write_view(out_dir: str, frame_id: int, buf: ViewBuffers, depth_scale: Optional[float] = None) -> None:
    """rgb_<id>.png, depth_<id>.png, maskid_<id>.png, transposed back to [H, W] (train.py:599-611); mask ids above 255
    wrap as the reference's uint8 image does."""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    Image.fromarray(np.ascontiguousarray(buf.rgb.transpose(1, 0, 2))).save(os.path.join(out_dir, f"rgb_{frame_id}.png"))
    Image.fromarray(np.ascontiguousarray(depth_png(buf.depth, depth_scale).T)).save(os.path.join(out_dir, f"depth_{frame_id}.png"))
    Image.fromarray(np.ascontiguousarray(buf.maskid.astype(np.uint8).T)).save(os.path.join(out_dir, f"maskid_{frame_id}.png"))


LABEL_PNG_MAX = 255       # queries a label_<id>.png can tell apart: label + 1 in 8 bits, 0 = nothing painted


def label_png(label: np.ndarray) -> np.ndarray:
    """The label image as written: uint8, label + 1, 0 where nothing painted (label -1); [W, H] -> [H, W]."""
    label = np.asarray(label)
    if label.size and (int(label.min()) < -1 or int(label.max()) >= LABEL_PNG_MAX):
        raise ValueError(f"label_png: labels outside -1 .. {LABEL_PNG_MAX - 1}")
    return np.ascontiguousarray((label + 1).astype(np.uint8).T)


def load_queries(path: str, feat_dim: int):
    """FILE.npz of --queries: feats [Q, C] and optionally names [Q] -> (feats fp32, names: a list of str)."""
    with np.load(path, allow_pickle=False) as z:
        if "feats" not in z.files:
            raise ValueError(f"--queries: {path} holds no array 'feats'")
        feats = np.asarray(z["feats"], np.float32)
        names = [str(n) for n in z["names"]] if "names" in z.files else None
    if feats.ndim != 2 or feats.shape[1] != feat_dim or not 1 <= feats.shape[0] <= LABEL_PNG_MAX:
        raise ValueError(f"--queries: feats must be [1 .. {LABEL_PNG_MAX}, {feat_dim}], got {feats.shape}")
    if names is None:
        names = [str(i) for i in range(feats.shape[0])]
    if len(names) != feats.shape[0]:
        raise ValueError(f"--queries: {len(names)} names for {feats.shape[0]} vectors")
    return feats, names


def parse_frames(spec: Optional[str], n: int) -> range:
    """"a:b:s" (each part optional, as a Python slice) over the n samples of the dataset."""
    if not spec:
        return range(n)
    parts = [int(p) if p.strip() else None for p in spec.split(":")]
    if len(parts) > 3:
        raise ValueError(f"--frames: {spec!r}: expected a:b:s")
    return range(n)[slice(*parts)] if len(parts) > 1 else range(n)[parts[0]:parts[0] + 1]


def main(argv=None):
    from . import dataset, vmap
    from .cfg import Config
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--logdir", required=True, help="reads DIR/ckpt/<id>/obj_<id>.pth")
    ap.add_argument("--config", required=True, help="the scene's config (dataset path, format, camera)")
    ap.add_argument("--frames", default=None, help="a:b:s over the samples of the config's dataset (default: all)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--bg-ids", type=int, nargs="*", default=[0])
    ap.add_argument("--semantic-ids", action="store_true", help="write semantic ids, not object ids, into maskid_<id>.png")
    ap.add_argument("--depth-scale", type=float, default=None, help="16-bit depth PNGs of round(depth * S)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--queries", default=None, help="FILE.npz with feats [Q, 512] (and names [Q]): also writes "
                    "label_<id>.png, the best-matching query + 1 per pixel (0 = nothing painted)")
    ap.add_argument("--save-sims", action="store_true", help="with --queries: sim_<id>.npy, the cosines [Q, H, W]")
    a = ap.parse_args(argv)
    if a.save_sims and not a.queries:
        ap.error("--save-sims needs --queries")
    c = Config(a.config)
    if c.dataset_format not in ("Replica", "ScanNet"):
        raise ValueError("Dataset format {} not found".format(c.dataset_format))
    ds = (dataset.Replica if c.dataset_format == "Replica" else dataset.ScanNet)(c)
    rays = vmap.cameraInfo(c).rays_dir_cache
    mv = MapView.from_logdir(a.logdir, a.device, bg_ids=a.bg_ids, semantic_ids=a.semantic_ids)
    feats = names = None
    if a.queries:
        feats, names = load_queries(a.queries, mv.feat_dim)
        print("queries: " + ", ".join(f"{i + 1} = {n}" for i, n in enumerate(names)))
    for i in parse_frames(a.frames, len(ds)):
        frame_id = int(ds.start + i * ds.stride)
        buf = mv.render(np.asarray(ds.depth_and_pose(i)[1], np.float32), rays, want_feat=feats is not None)
        write_view(a.out, frame_id, buf, a.depth_scale)
        print(f"frame {frame_id}: {int((buf.maskid != 0).sum())} pixels painted, {mv.seg[-1]} candidate rays")
        if feats is not None:
            from PIL import Image
            q = mv.query(feats, want_sims=a.save_sims)
            Image.fromarray(label_png(q["label"].cpu().numpy())).save(os.path.join(a.out, f"label_{frame_id}.png"))
            if a.save_sims:
                np.save(os.path.join(a.out, f"sim_{frame_id}.npy"), q["sims"].cpu().numpy().transpose(0, 2, 1))


if __name__ == "__main__":
    main()
