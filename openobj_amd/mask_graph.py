"""Cross-frame mask association: the reference's maskclustering/mask_graph.py on the GPU (objnerf_maskgraph.hip).

The script turns per-frame 2-D masks into object ids that agree across views; its output (instance_our/, class_our/,
object_clipfeat.pkl, object_capfeat.pkl, object_caption.pkl) is what openobj_amd.dataset reads.  The reference runs it
through open3d, OpenCV and python-louvain; here the data-parallel parts are HIP kernels and the rest is numpy:

  mask clouds     project_mask_pc (:337-462): per frame one CSR of the masks' connected components; ops.mask_points,
                  ops.mask_hist, ops.point_bounds; pcd_denoise_dbscan (:244-316): ops.DbscanPlan, one launch chain for
                  all clouds, the fallback chain min_points 100 -> 20 -> 10 -> keep all re-running only the clouds that
                  found no cluster;
  affinities      the five N x N matrices and their weighted sum (:501-735, :46): ops.mask_ray_boxes for
                  compute_2d_iou_matrix's ray / box pass, ops.mask_affinity for W and its edges;
  clustering      Louvain through networkx (seeded), the rare-id filter, the per-cluster features (host);
  merge           compute_similarity_matrix_thre (:820-895): ops.cloud_overlap for all pairs of clouds, then the
                  reference's mapping loop as written;
  files           write_outputs / main: the id images and pickles openobj_amd.dataset reads.

DBSCAN labels are those of a sequential DBSCAN that visits the points in index order (scikit-learn's).  open3d's
cluster_dbscan numbers clusters the same way; its treatment of a pair at exactly eps cannot be checked without open3d.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

BG_WALL, BG_FLOOR, BG_CEILING = 1, 2, 3        # compute_similarity_matrix_thre's background ids; the counter starts at 4
RARE_ID = 999                                   # filter_id's id of a cluster seen too rarely; mapped to 0 at the end


# ------------------------------------------------------------------------------------------- mask clouds: DBSCAN policy
def largest_cluster(labels: np.ndarray) -> Optional[np.ndarray]:
    """The mask of the largest cluster (Counter.most_common(1) without -1: on a tie the label that occurs first in point
    order); None when there is no cluster."""
    labels = np.asarray(labels)
    pos = np.flatnonzero(labels >= 0)
    if pos.size == 0:
        return None
    lab = labels[pos]
    count = np.bincount(lab)
    first = np.full(count.size, labels.size, np.int64)
    np.minimum.at(first, lab, pos)
    best = np.flatnonzero(count == count.max())
    return labels == best[np.argmin(first[best])]


def denoise_clouds(pts: torch.Tensor, seg_off, eps: float = 0.05, chain: Sequence[int] = (100, 20, 10)):
    """pcd_denoise_dbscan for S clouds at once (pts fp64 [n, 3] on the GPU, cloud s = rows seg_off[s] .. seg_off[s+1]):
    DBSCAN at chain[0]; the clouds without a cluster again at chain[1], ...; of each cloud the largest cluster, or every
    point when no run found one.  -> (keep bool [n] numpy, min_points that decided per cloud, 0 = kept all)."""
    off = np.asarray(torch.as_tensor(seg_off).cpu().numpy(), np.int64)
    S = off.size - 1
    plan = ops.DbscanPlan(pts, off, eps)
    keep = np.ones(int(off[-1]), bool)
    used = np.zeros(S, np.int64)
    todo = off[1:] > off[:-1]
    for mp in chain:
        if not todo.any():
            break
        labels = plan.run(np.where(todo, int(mp), 0)).cpu().numpy()
        for s in np.flatnonzero(todo):
            m = largest_cluster(labels[off[s]:off[s + 1]])
            if m is not None:
                keep[off[s]:off[s + 1]] = m
                used[s] = mp
                todo[s] = False
    return keep, used


# ------------------------------------------------------------------------------------------------ 2-D boxes of the masks
def mask_boxes_2d(depth_raw: np.ndarray, twc: np.ndarray, boxes: np.ndarray, intrinsics, device) -> torch.Tensor:
    """[F, N, 4] int32 (row_min, col_min, row_max + 1, col_max + 1): the every-10th-pixel rays of frame f that hit mask
    box n (depth_raw: the uint16 depth images [F, H, W]; intrinsics (fx, fy, cx, cy))."""
    depth_raw = np.ascontiguousarray(depth_raw)
    if depth_raw.dtype != np.uint16:
        raise TypeError("mask_boxes_2d: the raw uint16 depth images (the reference divides them by its literal 1000)")
    if depth_raw.shape[1] % 10 or depth_raw.shape[2] % 10:
        raise ValueError("mask_boxes_2d: image width and height must be multiples of 10 (the reference's view() fails)")
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    d = torch.from_numpy(depth_raw.view(np.int16)).to(device)
    return ops.mask_ray_boxes(d, torch.from_numpy(np.ascontiguousarray(twc, np.float64)).to(device),
                              torch.from_numpy(np.ascontiguousarray(boxes, np.float64)).to(device), fx, fy, cx, cy)


# ------------------------------------------------------------------------------------------------- clustering and merge
def filter_rare(ids: Sequence[int], frame_count: int) -> List[int]:
    """filter_id(cluster_ids, int(frame_count / 50)): ids observed in at most that many masks become 999."""
    ids = [int(i) for i in ids]
    limit = int(frame_count / 50)
    u, c = np.unique(np.asarray(ids, np.int64), return_counts=True) if ids else ((), ())
    rare = {int(a) for a, b in zip(u, c) if b <= limit}
    return [RARE_ID if i in rare else i for i in ids]


def mode_first(values: np.ndarray) -> int:
    """statistics.mode: the most frequent value, a tie going to the value met first in raster order."""
    values = np.asarray(values).ravel()
    u, first, count = np.unique(values, return_index=True, return_counts=True)
    best = np.flatnonzero(count == count.max())
    return int(u[best[np.argmin(first[best])]])


def check_similarity(bg_feats: np.ndarray, feat: np.ndarray, threshold: float) -> bool:
    return bool((np.asarray(bg_feats) @ np.asarray(feat) > threshold).any())


def vector_dbscan(x: np.ndarray, eps: float, min_samples: int) -> np.ndarray:
    """A small host DBSCAN over a few hundred feature vectors (sklearn.cluster.DBSCAN's labels): sequential, in index
    order, one cluster expanded at a time."""
    x = np.asarray(x, np.float64)
    n = len(x)
    near = []
    for i in range(n):
        near.append(np.flatnonzero(np.sqrt(((x - x[i]) ** 2).sum(axis=1)) <= eps))
    core = np.array([len(v) >= min_samples for v in near], bool)
    labels = np.full(n, -1, np.int64)
    cur = 0
    for i in range(n):
        if labels[i] != -1 or not core[i]:
            continue
        stack = [i]
        labels[i] = cur
        while stack:
            p = stack.pop()
            if not core[p]:
                continue
            for q in near[p]:
                if labels[q] == -1:
                    labels[q] = cur
                    stack.append(int(q))
        cur += 1
    return labels


def majority_mean(vectors: np.ndarray, eps: float = 0.2, min_samples: int = 2) -> np.ndarray:
    """get_majority_cluster_mean (:605-619): the mean of the most frequent DBSCAN label's vectors (np.unique order: the
    noise label -1 wins a tie)."""
    vectors = np.asarray(vectors)
    labels = vector_dbscan(vectors, eps, min_samples)
    u, c = np.unique(labels, return_counts=True)
    return np.mean(vectors[labels == u[np.argmax(c)]], axis=0)


def cloud_similarity(clouds: Sequence[np.ndarray], dis_thre: float, device) -> np.ndarray:
    """similarity_pc [C, C] fp64 = max(count[a][b] / n_a, count[b][a] / n_b), zero diagonal (:835-846)."""
    n = np.array([len(c) for c in clouds], np.int64)
    off = np.concatenate([[0], np.cumsum(n)])
    pts = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds]) if len(clouds) else np.zeros((0, 3))
    count = ops.cloud_overlap(torch.from_numpy(np.ascontiguousarray(pts)).to(device), off, dis_thre).cpu().numpy()
    with np.errstate(all="ignore"):
        ratio = count / n[:, None].astype(np.float64)       # np.mean over an empty cloud: NaN, which passes no threshold
    sim = np.maximum(ratio, ratio.T)                        # (numpy's maximum carries the NaN, as Python's max may not)
    np.fill_diagonal(sim, 0.0)
    return sim


def merge_mapping(keys: Sequence[int], sim_pc: np.ndarray, capft: Sequence[np.ndarray], color: Sequence[np.ndarray],
                  wall: np.ndarray, floor: np.ndarray, ceiling: np.ndarray, cap_thre: float = 0.8, weight_pc: float = 0.7,
                  weightcaption: float = 0.7, weightcolor: float = 0.7) -> Tuple[Dict[int, int], int]:
    """compute_similarity_matrix_thre's mapping (:852-895) as written, its `continue` order included: a background row i
    ends the pair before j is looked at; a background j ends it before the similarity is."""
    n = len(keys)
    cap = np.stack([np.asarray(v, np.float64) for v in capft]) if n else np.zeros((0, 1))
    col = np.stack([np.asarray(v, np.float64) for v in color]) if n else np.zeros((0, 1))
    sim_cap, sim_col = cap @ cap.T, col @ col.T
    sim = (sim_pc > weight_pc) & (sim_cap > weightcaption) & (sim_col > weightcolor) | (sim_pc > 0.9)
    bg = []
    for i in range(n):
        b = 0
        for ident, feats in ((BG_WALL, wall), (BG_FLOOR, floor), (BG_CEILING, ceiling)):
            if check_similarity(feats, capft[i], cap_thre):
                b = ident
                break
        bg.append(b)
    mapping: Dict[int, int] = {}
    counter = 4
    for i in range(n):
        for j in range(i + 1, n):
            if bg[i]:
                mapping[keys[i]] = bg[i]
                continue
            if bg[j]:
                mapping[keys[j]] = bg[j]
                continue
            if sim[i, j]:
                if keys[i] not in mapping:
                    mapping[keys[i]] = counter
                    counter += 1
                if keys[j] not in mapping:
                    mapping[keys[j]] = mapping[keys[i]]
    for i in range(n):
        if keys[i] not in mapping:
            mapping[keys[i]] = counter
            counter += 1
    mapping[RARE_ID] = 0
    return mapping, counter


# ---------------------------------------------------------------------------------------------- voxel_down_sample
_KEY_MASK = (1 << 21) - 1


def voxel_down(pts: torch.Tensor, seg_off, voxel: float):
    """open3d's voxel_down_sample of S clouds at once: voxel index floor((p - (min - voxel / 2)) / voxel), one point per
    occupied voxel = the fp64 sum of its points in input order / their count.  open3d returns the
    voxels in its hash map's order; here they come in ascending (iz, iy, ix) order.  -> (points fp64 [V, 3], offsets)."""
    off = np.asarray(torch.as_tensor(seg_off).cpu().numpy(), np.int64)
    S, n = off.size - 1, int(off[-1])
    dev = pts.device
    if n == 0:
        return pts.new_zeros((0, 3)), np.zeros(S + 1, np.int64)
    if S >= 1 << 21:
        raise ops.ObjnerfError("voxel_down: at most 2^21 - 1 clouds a call")
    keys, _ = ops.cell_keys(pts, off, voxel, 0.5 * voxel, "voxel_down")
    seg = torch.repeat_interleave(torch.arange(S, device=dev), torch.from_numpy(np.diff(off)).to(dev))
    ix, iy, iz = keys >> 42, (keys >> 21) & _KEY_MASK, keys & _KEY_MASK
    nx = torch.zeros(S, dtype=torch.int64, device=dev).scatter_reduce(0, seg, ix, "amax") + 1
    ny = torch.zeros(S, dtype=torch.int64, device=dev).scatter_reduce(0, seg, iy, "amax") + 1
    nz = torch.zeros(S, dtype=torch.int64, device=dev).scatter_reduce(0, seg, iz, "amax") + 1
    if float((nx.double() * ny.double() * nz.double()).max().item()) >= 2.0 ** 42:
        raise ops.ObjnerfError("voxel_down: a cloud spans more than 2^42 voxels")
    lin = (seg << 42) | (ix + nx[seg] * (iy + ny[seg] * iz))
    skeys, perm = torch.sort(lin, stable=True)                 # equal keys keep the points' order
    cen, _, first = ops.run_centroids(skeys, perm, pts, S)
    V = int(cen.shape[0])
    first_h = first.cpu().numpy()
    new_off = np.full(S + 1, V, np.int64)
    for s in range(S - 1, -1, -1):                             # an empty cloud starts where the next one does
        new_off[s] = first_h[s] if first_h[s] >= 0 else new_off[s + 1]
    return cen, new_off


# -------------------------------------------------------------------------------------------- mask clouds of one frame
MIN_COMPONENT = 100        # project_mask_pc :393
MIN_POINTS_KEPT = 10       # :428


def _components(mask: np.ndarray) -> List[np.ndarray]:
    """The 8-connected components of a mask as flat pixel indices in raster order, ordered by their first pixel."""
    from scipy import ndimage
    lab, k = ndimage.label(mask, structure=np.ones((3, 3), np.int32))
    if k == 0:
        return []
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    order = np.argsort(flat[idx], kind="stable")
    idx, labs = idx[order], flat[idx][order]
    parts = np.split(idx, np.flatnonzero(np.diff(labs)) + 1)
    return sorted(parts, key=lambda p: int(p[0]))


def frame_depth(depth_raw: np.ndarray, depth_scale: float, min_depth: float = 0.07, max_depth: float = 10.0) -> np.ndarray:
    """:341-350: depth / depth_scale rounded to fp32, values below min_depth or above max_depth set to 0."""
    d = (np.asarray(depth_raw) / depth_scale).astype(np.float32)
    if min_depth > 0:
        d[d < min_depth] = 0
    if max_depth > 0:
        d[d > max_depth] = 0
    return d


def project_masks(masks: Sequence[np.ndarray], depth_raw: np.ndarray, bgr: np.ndarray, pose: np.ndarray,
                  depth_scale: float, intrinsics, device, if_filter: bool = True):
    """project_mask_pc (:337-462) for one frame -> (points list, boxes list, histograms list, filtered masks list,
    mask_ok bool [M]); the lists hold the masks with mask_ok only, as the reference's."""
    depth = frame_depth(depth_raw, depth_scale)
    H, W = depth.shape
    if bgr.shape[:2] != (H, W):
        raise NotImplementedError("mask_graph: an image whose size differs from the depth image (the reference resizes "
                                  "it with OpenCV's nearest-neighbour rule)")
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    valid = depth > 0
    M = len(masks)
    mask_ok = np.ones(M, bool)
    segs: List[Tuple[int, np.ndarray]] = []                     # (mask, pixel indices) of every component with a pixel
    for m, mask in enumerate(masks):
        mask = np.asarray(mask)
        if mask.shape != (H, W):
            raise NotImplementedError("mask_graph: a mask whose size differs from the depth image (the reference "
                                      "resizes it with OpenCV's nearest-neighbour rule)")
        mask = mask.astype(bool)
        if not (mask & valid).any():
            mask_ok[m] = False
            continue
        vflat = valid.ravel()
        for comp in _components(mask):
            comp = comp[vflat[comp]]
            if comp.size:
                segs.append((m, comp))
    out_pts, out_box, out_hist, out_mask = [], [], [], []
    if not segs:
        return out_pts, out_box, out_hist, out_mask, mask_ok
    n_seg = np.array([len(c) for _, c in segs], np.int64)
    seg_mask = np.array([m for m, _ in segs], np.int64)
    seg_off = np.concatenate([[0], np.cumsum(n_seg)])
    pix_h = np.concatenate([c for _, c in segs]).astype(np.int32)
    pix = torch.from_numpy(pix_h).to(device)
    pts = ops.mask_points(pix, torch.from_numpy(depth).to(device),
                          torch.from_numpy(np.ascontiguousarray(pose, np.float64)).to(device), fx, fy, cx, cy)
    live = np.flatnonzero(mask_ok)
    mask_off = np.concatenate([[0], np.cumsum([n_seg[seg_mask == m].sum() for m in live])])
    hist = ops.mask_hist(pix, mask_off, torch.from_numpy(np.ascontiguousarray(bgr, np.uint8)).to(device)).cpu().numpy()
    # the components DBSCAN sees: at least MIN_COMPONENT valid pixels
    big = np.flatnonzero(n_seg >= MIN_COMPONENT)
    rows = np.concatenate([np.arange(seg_off[s], seg_off[s + 1]) for s in big]) if big.size else np.zeros(0, np.int64)
    sub = pts[torch.from_numpy(rows).to(device)] if rows.size else pts[:0]
    sub_off = np.concatenate([[0], np.cumsum(n_seg[big])])
    if if_filter:
        keep = denoise_clouds(sub, sub_off, 0.05, (100, 20, 10))[0] if rows.size else np.zeros(0, bool)
        kept = sub[torch.from_numpy(np.flatnonzero(keep)).to(device)] if rows.size else sub
        kept_n = np.array([keep[sub_off[t]:sub_off[t + 1]].sum() for t in range(big.size)], np.int64)
    else:
        down, down_off = voxel_down(sub, sub_off, 0.025)
        keep_d = denoise_clouds(down, down_off, 0.05, (10, 2, 1))[0] if rows.size else np.zeros(0, bool)
        kept = down[torch.from_numpy(np.flatnonzero(keep_d)).to(device)] if rows.size else sub
        kept_n = np.array([keep_d[down_off[t]:down_off[t + 1]].sum() for t in range(big.size)], np.int64)
    # per mask: its components' kept points in component order
    per_mask_n = np.array([kept_n[seg_mask[big] == m].sum() for m in live], np.int64)
    kept_off = np.concatenate([[0], np.cumsum(per_mask_n)])
    boxes = ops.point_bounds(kept, kept_off).cpu().numpy() if live.size else np.zeros((0, 6))
    kept_h = kept.cpu().numpy()
    for t, m in enumerate(live):
        if per_mask_n[t] < MIN_POINTS_KEPT:
            mask_ok[m] = False
            continue
        new = np.asarray(masks[m]).astype(bool) & valid
        if if_filter:
            flat = new.ravel()
            for s in np.flatnonzero(seg_mask == m):
                if n_seg[s] < MIN_COMPONENT:
                    flat[pix_h[seg_off[s]:seg_off[s + 1]]] = False
            for u in np.flatnonzero(seg_mask[big] == m):
                s = big[u]
                flat[pix_h[seg_off[s]:seg_off[s + 1]]] = keep[sub_off[u]:sub_off[u + 1]]
        out_pts.append(kept_h[kept_off[t]:kept_off[t + 1]])
        out_box.append(boxes[t])
        out_hist.append(hist[t])
        out_mask.append(new)
    return out_pts, out_box, out_hist, out_mask, mask_ok


# --------------------------------------------------------------------------------------------------- the whole pipeline
class MaskGraph:
    """The reference's __main__ (:897-1280) from the loaded mask file on: cfg is its yaml as a dict (weight_geo,
    weight_cap, weight_clip, weight_color, weight_geo_2d, graph_method, if_filter, if_bg, cap_thre, dis_thre, weight_pc,
    weightcaption, weightcolor, depth_scale, gt_*_id; `seed` for the Louvain step, default 0), intrinsics
    (fx, fy, cx, cy).  Louvain is networkx's louvain_communities with a seed: the reference calls python-louvain
    unseeded, so no parity with its partition is claimed."""

    def __init__(self, cfg: dict, intrinsics, device=None):
        self.cfg = dict(cfg)
        if self.cfg.get("graph_method", "weighted") != "weighted":
            raise NotImplementedError("mask_graph: only graph_method: weighted is supported (got %r)"
                                      % self.cfg.get("graph_method"))
        self.intrinsics = tuple(float(v) for v in intrinsics)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def affinity(self, boxes, capfeat, clipfeat, color, depth, Twc):
        """-> (W, edges, weights) of the N kept masks (torch tensors on the device)."""
        cfg, dev = self.cfg, self.device
        w2 = float(cfg.get("weight_geo_2d", 0.0))
        boxes2d = None
        if w2 > 0:
            parts = [mask_boxes_2d(np.stack(depth[f0:f0 + 32]), Twc[f0:f0 + 32], boxes, self.intrinsics, dev)
                     for f0 in range(0, len(depth), 32)]
            boxes2d = torch.cat(parts)
        weights = (cfg["weight_geo"], cfg["weight_cap"], cfg["weight_clip"], cfg["weight_color"], w2 if w2 > 0 else 0.0)
        W, ij, ew, _ = ops.mask_affinity(torch.from_numpy(np.ascontiguousarray(boxes, np.float64)).to(dev),
                                         torch.from_numpy(np.ascontiguousarray(capfeat, np.float32)).to(dev),
                                         torch.from_numpy(np.ascontiguousarray(clipfeat, np.float32)).to(dev),
                                         torch.from_numpy(np.ascontiguousarray(color, np.float32)).to(dev), boxes2d, weights)
        return W, ij, ew

    def cluster(self, n_nodes: int, edges: np.ndarray, weights: np.ndarray) -> List[int]:
        import networkx as nx
        g = nx.Graph()
        g.add_nodes_from(range(n_nodes))
        g.add_weighted_edges_from((int(i), int(j), float(w)) for (i, j), w in zip(edges, weights))
        comms = nx.community.louvain_communities(g, weight="weight", seed=int(self.cfg.get("seed", 0)))
        ids = [0] * n_nodes
        for c, members in enumerate(sorted(comms, key=min)):      # numbered by their smallest node: a fixed order
            for v in members:
                ids[v] = c
        return ids

    def run(self, masks, capfeat, clipfeat, captions, depth, rgb, Twc, bg_feats, semantic=None):
        """masks / capfeat / clipfeat / captions: per frame, per mask; depth: the raw uint16 images; rgb: uint8 [H, W, 3]
        RGB images; Twc [F, 4, 4]; bg_feats {"wall", "floor", "ceiling"}: unit caption features [k, D] of the
        background captions (the text encoder stays outside); semantic: the ground-truth class images for if_bg.
        -> (id images int32 [H, W] per frame, clip dicts, caption-feature dicts, caption dicts per frame)."""
        cfg, dev = self.cfg, self.device
        F = len(masks)
        wall, floor, ceiling = (np.asarray(bg_feats[k]) for k in ("wall", "floor", "ceiling"))
        if_bg = bool(cfg.get("if_bg", 0))
        if if_bg and semantic is None:
            raise ValueError("mask_graph: if_bg needs the ground-truth semantic images")
        Twc = np.asarray(Twc, np.float64)
        all_pc, all_hist, all_mask, boxes = [], [], [], []
        cap_l, clip_l, text_l, raw_l = [], [], [], []
        for f in range(F):
            pc, box, hist, kept, ok = project_masks(masks[f], depth[f], np.asarray(rgb[f])[..., ::-1], Twc[f],
                                                    cfg["depth_scale"], self.intrinsics, dev, bool(cfg.get("if_filter", 1)))
            all_pc.append(pc), all_hist.append(hist), all_mask.append(kept), boxes.extend(box)
            cap_l.append([v for v, k in zip(capfeat[f], ok) if k])
            clip_l.append([v for v, k in zip(clipfeat[f], ok) if k])
            text_l.append([v for v, k in zip(captions[f], ok) if k])
            raw_l.append([np.asarray(v).astype(bool) for v, k in zip(masks[f], ok) if k])
        N = len(boxes)
        H, W_img = np.asarray(depth[0]).shape
        if N == 0:
            return [np.zeros((H, W_img), np.int32) for _ in range(F)], [{} for _ in range(F)], [{} for _ in range(F)], \
                   [{} for _ in range(F)]
        cap_s = np.stack([np.asarray(v, np.float32).reshape(-1) for fr in cap_l for v in fr])
        clip_s = np.stack([np.asarray(v, np.float32).reshape(-1) for fr in clip_l for v in fr])
        color_s = np.stack([h for fr in all_hist for h in fr])
        _, ij, ew = self.affinity(np.stack(boxes), cap_s, clip_s, color_s, depth, Twc)
        ids = filter_rare(self.cluster(N, ij.cpu().numpy(), ew.cpu().numpy()), F)
        # per-cluster global data (:1106-1187)
        thr = cfg["cap_thre"]
        g_pc: Dict[int, list] = {}
        g_cap: Dict[int, list] = {}
        g_col: Dict[int, list] = {}
        frame_ids, at = [], 0
        for f in range(F):
            frame_ids.append(ids[at:at + len(all_mask[f])])
            for j in range(len(all_mask[f])):
                this = ids[at + j]
                if this == RARE_ID:
                    continue
                feat = np.asarray(cap_l[f][j]).reshape(-1)
                if if_bg:
                    gt = mode_first(np.asarray(semantic[f]).astype(np.int32)[raw_l[f][j]])
                    feat = wall[0] if gt == cfg["gt_wall_id"] else floor[0] if gt == cfg["gt_floor_id"] else \
                        ceiling[0] if gt == cfg["gt_ceiling_id"] else feat
                elif check_similarity(wall, feat, thr):
                    feat = wall[0]
                elif check_similarity(floor, feat, thr):
                    feat = floor[0]
                elif check_similarity(ceiling, feat, thr):
                    feat = ceiling[0]
                g_pc.setdefault(this, []).append(all_pc[f][j])
                g_cap.setdefault(this, []).append(np.asarray(feat, np.float64))
                g_col.setdefault(this, []).append(np.asarray(all_hist[f][j]))
            at += len(all_mask[f])
        keys = list(g_pc.keys())
        mapping = {RARE_ID: 0}
        if keys:
            sizes = [sum(len(p) for p in g_pc[k]) for k in keys]
            off = np.concatenate([[0], np.cumsum(sizes)])
            cat = torch.from_numpy(np.concatenate([p for k in keys for p in g_pc[k]])).to(dev)
            down, down_off = voxel_down(cat, off, 0.01)
            down_h = down.cpu().numpy()
            clouds = [down_h[down_off[c]:down_off[c + 1]] for c in range(len(keys))]
            cap_g, col_g = [], []
            for k in keys:
                c = g_cap[k][0]
                if len(g_cap[k]) > 1:                              # (np.ndim == 2: more than one mask)
                    c = majority_mean(np.stack(g_cap[k]))
                    c = c / np.linalg.norm(c)
                cap_g.append(c)
                h = g_col[k][0]
                if len(g_col[k]) > 1:
                    h = np.mean(np.stack(g_col[k]), axis=0)
                    h = h / np.linalg.norm(h)
                col_g.append(h)
            sim_pc = cloud_similarity(clouds, cfg["dis_thre"], dev)
            mapping, _ = merge_mapping(keys, sim_pc, cap_g, col_g, wall, floor, ceiling, cfg["cap_thre"], cfg["weight_pc"],
                                       cfg["weightcaption"], cfg["weightcolor"])
        images, clip_d, cap_d, text_d = [], [], [], []
        for f in range(F):
            img = np.zeros((H, W_img), np.int32)
            cd, pd, td = {}, {}, {}
            for j, m in enumerate(all_mask[f]):
                new = mapping[frame_ids[f][j]]
                if new != 0:
                    img[m] = new
                    cd[new], pd[new], td[new] = clip_l[f][j], cap_l[f][j], text_l[f][j]
            images.append(img), clip_d.append(cd), cap_d.append(pd), text_d.append(td)
        return images, clip_d, cap_d, text_d


# -------------------------------------------------------------------------------------------------------------- files
def write_outputs(output_dir: str, images, clip_d, cap_d, text_d, debug_images: bool = False) -> None:
    """instance_our/semantic_instance_<i>.png, class_our/semantic_class_<i>.png (the same id image, 16-bit PNG) and the
    three pickles, the layout openobj_amd.dataset reads (:1240-1280)."""
    import os
    import pickle
    from PIL import Image
    for sub, stem in (("class_our", "semantic_class_"), ("instance_our", "semantic_instance_")):
        os.makedirs(os.path.join(output_dir, sub), exist_ok=True)
        for i, img in enumerate(images):
            if img.max(initial=0) > 65535:
                raise ValueError("mask_graph: an object id above 65535 does not fit the 16-bit id image")
            Image.fromarray(img.astype(np.uint16)).save(os.path.join(output_dir, sub, "%s%d.png" % (stem, i)))
    for name, val in (("object_clipfeat.pkl", clip_d), ("object_capfeat.pkl", cap_d), ("object_caption.pkl", text_d)):
        with open(os.path.join(output_dir, name), "wb") as f:
            pickle.dump(val, f)
    if debug_images:
        os.makedirs(os.path.join(output_dir, "debug"), exist_ok=True)
        lut = np.random.RandomState(0).randint(0, 256, (65536, 3)).astype(np.uint8)
        lut[0] = 0
        for i, img in enumerate(images):
            Image.fromarray(lut[img]).save(os.path.join(output_dir, "debug", "inst_%d.png" % i))


def pose_rotation(cfg: dict) -> np.ndarray:
    """R_total = R_x R_y R_z of the yaml's x_the, y_the, z_the (degrees), 4 x 4 (:963-988)."""
    tx, ty, tz = (np.radians(cfg.get(k, 0.0)) for k in ("x_the", "y_the", "z_the"))
    rx = np.array([[1, 0, 0, 0], [0, np.cos(tx), -np.sin(tx), 0], [0, np.sin(tx), np.cos(tx), 0], [0, 0, 0, 1]])
    ry = np.array([[np.cos(ty), 0, np.sin(ty), 0], [0, 1, 0, 0], [-np.sin(ty), 0, np.cos(ty), 0], [0, 0, 0, 1]])
    rz = np.array([[np.cos(tz), -np.sin(tz), 0, 0], [np.sin(tz), np.cos(tz), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    return np.dot(np.dot(rx, ry), rz)


def load_inputs(cfg: dict, input_mask: str, dataset_dir: str):
    """The reference's input handling (:920-1002): the mask file's lists (start / use_num), the natural-sorted depth,
    rgb and semantic files sliced [0:-1:skip], the poses rotated by R_total^T and sliced the same way."""
    import glob
    import os
    import pickle
    from .dataset import _natural_key, _read_image
    with open(input_mask, "rb") as f:
        info = pickle.load(f)
    skip, use_num, start = int(cfg["skip"]), int(cfg.get("use_num", -1)), int(cfg.get("start", 0))
    sel = (lambda v: v[start:start + use_num]) if use_num != -1 else (lambda v: v)
    masks, caps, capft, clipft = (sel(info[k]) for k in ("mask", "caption", "capfeat", "clipfeat"))

    def files(sub):
        return sorted(glob.glob(os.path.join(dataset_dir, sub, "*.png")), key=_natural_key)[0:-1:skip]

    twc = np.loadtxt(os.path.join(dataset_dir, "traj_w_c.txt"), delimiter=" ").reshape([-1, 4, 4])
    rt = pose_rotation(cfg).T
    twc = np.stack([np.dot(rt, t) for t in twc])[0:-1:skip]
    twc = sel(twc)
    n = len(masks)
    depth = [_read_image(p).astype(np.uint16) for p in files("depth")[:n]]
    rgb = [_read_image(p).astype(np.uint8) for p in files("rgb")[:n]]
    semantic = None
    if cfg.get("if_bg", 0):
        semantic = [_read_image(p).astype(np.int32) for p in files("semantic_class")[:n]]
    return masks, capft, clipft, caps, depth, rgb, twc, semantic


def main(argv=None) -> int:
    import argparse
    import yaml
    ap = argparse.ArgumentParser(prog="python -m openobj_amd.mask_graph",
                                 description="Cross-frame mask association: per-frame masks -> consistent object ids")
    ap.add_argument("config", help="the reference's mask_graph yaml")
    ap.add_argument("--input-mask", required=True, help="mask_init_all.pkl (mask, caption, capfeat, clipfeat per frame)")
    ap.add_argument("--dataset-dir", required=True, help="depth/, rgb/, traj_w_c.txt (semantic_class/ with if_bg)")
    ap.add_argument("--bg-feats", required=True, help=".npz with wall, floor, ceiling: unit caption features [k, D]")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--debug-images", action="store_true", help="also write coloured id images under debug/")
    a = ap.parse_args(argv)
    with open(a.config) as f:
        cfg = yaml.safe_load(f)
    graph = MaskGraph(cfg, (cfg["fx"], cfg["fy"], cfg["cx"], cfg["cy"]))
    bg = np.load(a.bg_feats)
    masks, capft, clipft, caps, depth, rgb, twc, semantic = load_inputs(cfg, a.input_mask, a.dataset_dir)
    out = graph.run(masks, capft, clipft, caps, depth, rgb, twc, {k: bg[k] for k in ("wall", "floor", "ceiling")}, semantic)
    write_outputs(a.output_dir, *out, debug_images=a.debug_images)
    print("mask_graph: %d frames, %d object ids -> %s" % (len(out[0]), len({k for d in out[1] for k in d}), a.output_dir))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
