"""Novel-view rendering of a whole scene: every object is rendered inside its own oriented box
(sceneObject.render_2D_syn) and the per-object images are merged by depth -- the loop of train.py:550-612
(`cfg.if_render`).  Images are stored transposed, [W, H, ...], like everything else in the reference."""
from typing import Dict, Iterable, Optional

import numpy as np


class ViewBuffers:
    """rendered_rgb_image / rendered_depth_image / rendered_maskid_image of train.py:558-566."""

    def __init__(self, W: int, H: int):
        self.rgb = np.zeros((W, H, 3), dtype=np.uint8)
        self.maskid = np.zeros((W, H), dtype=np.int32)
        self.depth = np.ones((W, H), dtype=np.float32) * 100        # "set the depth image large first" (:566)

    def merge(self, obj_mask: np.ndarray, render_depth: np.ndarray, render_color: np.ndarray, class_id: int,
              is_background: bool) -> np.ndarray:
        """z-buffer test of one object's render against what is already there (train.py:581-598).  Background
        objects paint colour but do not write depth, so that they never hide a foreground object (:596-597).
        Returns the boolean image of the pixels this object won."""
        this_depth = np.ones_like(self.depth) * 100
        this_rgb = np.zeros_like(self.rgb)
        this_depth[obj_mask] = render_depth
        this_rgb[obj_mask] = render_color
        ok = self.depth > this_depth
        self.rgb[ok] = this_rgb[ok]
        self.maskid[ok] = class_id
        if not is_background:
            self.depth[ok] = this_depth[ok]
        return ok


def render_view(vis_dict: Dict[int, object], T_WC: np.ndarray, rays_dir, intrinsic_open3d=None,
                bg_ids: Iterable[int] = (0,), class_of: Optional[Dict[int, int]] = None, W: Optional[int] = None,
                H: Optional[int] = None, draws: Optional[Dict[int, object]] = None) -> ViewBuffers:
    """Render every object of `vis_dict` (obj_id -> sceneObject, dict order as train.py:570) from pose T_WC and
    merge.  class_of maps obj_id -> the id written into the mask-id image (mapping_class of train.py:592)."""
    first = next(iter(vis_dict.values()))
    W = W or first.trainer.W_vis
    H = H or first.trainer.H_vis
    bg_ids = set(bg_ids)
    buf = ViewBuffers(W, H)
    for obj_id, obj_k in vis_dict.items():
        res = obj_k.render_2D_syn(T_WC, intrinsic_open3d, rays_dir, chunk_size=3000, do_fine=False,
                                  draws=None if draws is None else draws.get(obj_id))
        if res[1] is None:
            continue
        obj_mask, render_depth, render_color = res[0], res[1], res[2]
        buf.merge(obj_mask, render_depth, render_color, (class_of or {}).get(obj_id, obj_id), obj_id in bg_ids)
    return buf


def merge_closed_form(obj_masks, depths, class_ids, is_background):
    """What the fold of ViewBuffers.merge over K objects IN ORDER leaves behind, without the fold -- the rule
    objnerf_view_merge implements on the device.  obj_masks [K, W, H] bool: the pixels each object's
    render kept; depths [K, W, H] float32: its depth there (anything elsewhere); class_ids [K]; is_background [K].

    An object is OFFERED at a pixel iff its mask is set and its depth < 100 (the depth image starts at 100 and only a
    strictly smaller depth paints).  W = the offered FOREGROUND object of smallest depth, the earliest among equal
    depths: foreground depths only ever lower the depth image, strictly, so the first object that reaches the minimum
    is the last foreground object that paints.  The depth image ends as W's depth (100 without W): a background never
    writes it.  A background object paints iff its depth is below the depth image AT ITS TURN; before W's turn it is
    painted over by W, after W's turn the depth image is W's depth for good.  So the painter is the LAST offered
    background object behind W in the order whose depth < W's depth (without W: the last offered one), otherwise W.

    -> (painter [W, H] int64: the position of the painting object in the order, -1 = none; depth [W, H] float32;
    maskid [W, H] int32, 0 = none).  The colour image is the painter's colour."""
    m = np.asarray(obj_masks, bool)
    d = np.asarray(depths, np.float32)
    bg = np.asarray(is_background, bool).reshape(-1, 1, 1)
    K = m.shape[0]
    offered = m & (d < np.float32(100))
    big = np.float32(np.inf)
    d_fg = np.where(offered & ~bg, d, big)
    w = np.argmin(d_fg, axis=0)                               # the first minimum: the earliest object
    d_w = np.take_along_axis(d_fg, w[None], axis=0)[0]
    has_w = d_w < big
    depth = np.where(has_w, d_w, np.float32(100)).astype(np.float32)
    order = np.arange(K).reshape(-1, 1, 1)
    cand = offered & bg & (d < depth[None]) & (~has_w[None] | (order > w[None]))
    last_bg = np.where(cand, order, -1).max(axis=0)
    painter = np.where(last_bg >= 0, last_bg, np.where(has_w, w, -1)).astype(np.int64)
    ids = np.asarray(class_ids, np.int32)
    maskid = np.where(painter >= 0, ids[np.maximum(painter, 0)], 0).astype(np.int32)
    return painter, depth, maskid


def render_view_batched(vis_dict: Dict[int, object], T_WC: np.ndarray, rays_dir, intrinsic_open3d=None,
                        bg_ids: Iterable[int] = (0,), class_of: Optional[Dict[int, int]] = None,
                        W: Optional[int] = None, H: Optional[int] = None,
                        draws: Optional[Dict[int, object]] = None) -> ViewBuffers:
    """render_view in one launch chain (map_view.MapView over the objects' networks and their get_bound(final=True)
    boxes): the same arguments, the same ViewBuffers bit for bit -- with injected draws, and in a seeded run too, since
    every object that renders takes its draw counter at its turn in dict order as the loop does."""
    from . import map_view
    first = next(iter(vis_dict.values()))
    W = W or first.trainer.W_vis
    H = H or first.trainer.H_vis
    if tuple(rays_dir.shape[:2]) != (W, H):
        raise ValueError(f"render_view_batched: rays_dir {tuple(rays_dir.shape)} for a {W} x {H} view")
    objects = [map_view.MapObject(o.trainer, o.get_bound(intrinsic_open3d, final=True)[1], obj_id=obj_id)
               for obj_id, o in vis_dict.items()]
    mv = map_view.MapView(objects, device=first.training_device, bg_ids=bg_ids,
                          class_of={i: (class_of or {}).get(i, i) for i in vis_dict})
    return mv.render(T_WC, rays_dir, draws=draws)
