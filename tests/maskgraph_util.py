"""numpy / scipy restatement of every stage of the mask graph (maskclustering/mask_graph.py of the reference), for the
tests of openobj_amd.mask_graph.  It shares no code with the module under test: DBSCAN through cKDTree and
connected_components, the ray / box pass and the 2-D running mean as the reference writes them, the fp64 affinity,
the cKDTree overlap and the host policies (largest cluster, rare ids, mode, merge)."""
from collections import Counter

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


# ----------------------------------------------------------------------------------------------------------- DBSCAN
def dbscan_labels(x, eps, min_points):
    """Labels of a DBSCAN that visits the points in index order: core = at least min_points points within eps (itself
    included, d <= eps); clusters = connected components of the core points, numbered by their smallest core index; a
    border point takes the lowest cluster among its core neighbours; the rest is -1."""
    x = np.asarray(x, np.float64)
    n = len(x)
    labels = np.full(n, -1, np.int32)
    if n == 0:
        return labels
    near = cKDTree(x).query_ball_point(x, eps)            # d <= eps, the point itself included
    lens = np.array([len(v) for v in near])
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([np.asarray(v, np.int64) for v in near])
    core = lens >= min_points
    idx = np.flatnonzero(core)
    if idx.size == 0:
        return labels
    cc = core[rows] & core[cols]
    g = coo_matrix((np.ones(int(cc.sum()), np.int8), (rows[cc], cols[cc])), shape=(n, n))
    ncomp, comp = connected_components(g, directed=False)
    first = np.full(ncomp, n, np.int64)
    np.minimum.at(first, comp[idx], idx)                 # a component's smallest core index
    order = np.unique(first[comp[idx]])                  # ascending: the cluster numbering
    labels[idx] = np.searchsorted(order, first[comp[idx]])
    bc = ~core[rows] & core[cols]                        # (border or noise point, core neighbour)
    low = np.full(n, np.iinfo(np.int32).max, np.int64)
    np.minimum.at(low, rows[bc], labels[cols[bc]])
    got = ~core & (low < np.iinfo(np.int32).max)
    labels[got] = low[got]
    return labels


def min_gap_to_radius(x, r):
    """The smallest | d - r | over all pairs of points (the tests keep it away from the comparison's edge)."""
    x = np.asarray(x, np.float64)
    if len(x) < 2:
        return np.inf
    tree = cKDTree(x)
    pairs = tree.query_pairs(r * 1.001 + 1e-6, output_type="ndarray")
    if len(pairs) == 0:
        return np.inf
    d = np.linalg.norm(x[pairs[:, 0]] - x[pairs[:, 1]], axis=1)
    return float(np.abs(d - r).min())


def largest_cluster_mask(labels):
    """pcd_denoise_dbscan's choice: Counter.most_common(1) without -1 (a tie: the label met first); None: no cluster."""
    counter = Counter(np.asarray(labels).tolist())
    counter.pop(-1, None)
    if not counter:
        return None
    lab, _ = counter.most_common(1)[0]
    return np.asarray(labels) == lab


def denoise(x, eps, chain):
    """The fallback chain of pcd_denoise_dbscan: the first min_points of `chain` that finds a cluster; else keep all."""
    for mp in chain:
        m = largest_cluster_mask(dbscan_labels(x, eps, mp))
        if m is not None:
            return m
    return np.ones(len(x), bool)


def majority_mean(vectors, eps=0.2, min_samples=2):
    """get_majority_cluster_mean with the restated DBSCAN (np.unique sorts: noise, -1, wins a tie)."""
    vectors = np.asarray(vectors)
    labels = dbscan_labels(vectors, eps, min_samples)
    u, c = np.unique(labels, return_counts=True)
    return vectors[labels == u[np.argmax(c)]].mean(axis=0)


# ------------------------------------------------------------------------------------------------------ ray / box pass
def ray_boxes(depth_raw, twc, boxes, fx, fy, cx, cy):
    """compute_2d_iou_matrix's per-frame 2-D boxes [F, N, 4] int32, and per (frame, mask) whether some ray lies within
    1e-9 relative of the hit test's edges (near == far, far == 0)."""
    F, H, W = depth_raw.shape
    ix, iy = np.meshgrid(np.arange(0, W, 10), np.arange(0, H, 10), indexing="xy")
    d32 = np.stack([(ix.astype(np.float32) - np.float32(cx)) / np.float32(fx),
                    (iy.astype(np.float32) - np.float32(cy)) / np.float32(fy),
                    np.ones(ix.shape, np.float32)], -1)
    out = np.zeros((F, len(boxes), 4), np.int32)
    edge = np.zeros((F, len(boxes)), bool)
    for f in range(F):
        depth = depth_raw[f].astype(np.uint16) / 1000.0
        dw = (d32.astype(np.float64) * depth[::10, ::10, None]).reshape(-1, 3)
        R = twc[f][:3, :3]
        dw = np.stack([dw[:, 0] * R[c, 0] + dw[:, 1] * R[c, 1] + dw[:, 2] * R[c, 2] for c in range(3)], -1)
        o = twc[f][:3, 3]
        with np.errstate(all="ignore"):
            tmin = (boxes[None, :, :3] - o[None, None]) / dw[:, None]
            tmax = (boxes[None, :, 3:] - o[None, None]) / dw[:, None]
            near = np.max(np.minimum(tmin, tmax), axis=2)        # numpy's minimum / maximum / max / min carry NaNs, as torch's
            far = np.min(np.maximum(tmin, tmax), axis=2)
            hit = ((near <= far) & (far > 0)).T                  # [N, rays]
            scale = np.maximum(np.abs(near), np.abs(far))
            close = (np.abs(near - far) <= 1e-9 * scale) | (np.abs(far) <= 1e-9 * np.maximum(scale, 1e-300))
            close &= np.isfinite(near) & np.isfinite(far)
        edge[f] = close.T.any(axis=1)
        hm = hit.reshape(len(boxes), H // 10, W // 10)
        for m in range(len(boxes)):
            r, c = np.nonzero(hm[m])
            if len(r):
                out[f, m] = (r.min(), c.min(), r.max() + 1, c.max() + 1)
    return out, edge


def iou_2d(b):
    """compute_iou_2d on int32 boxes: integer areas, a true division in fp32, NaN -> 0."""
    b = b.astype(np.int64)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = (x2 - x1) * (y2 - y1)
    inter = (np.clip(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]), 0, None)
             * np.clip(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]), 0, None))
    union = area[:, None] + area[None] - inter
    with np.errstate(all="ignore"):
        iou = inter.astype(np.float32) / union.astype(np.float32)
    iou[np.isnan(iou)] = 0
    return iou


def geo2d_mean(boxes2d):
    """m = (m * f + iou_f) / (f + 1) in fp32, in frame order."""
    N = boxes2d.shape[1]
    m = np.zeros((N, N), np.float32)
    for f in range(boxes2d.shape[0]):
        m = (m * np.float32(f) + iou_2d(boxes2d[f])) / np.float32(f + 1)
    return m


# ------------------------------------------------------------------------------------------------------------ affinity
def geo_matrix(boxes):
    """compute_3d_iou_matrix: intersection volume / the smaller volume, NaN -> 0 (fp64)."""
    b = np.asarray(boxes, np.float64)
    vol = (b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2])
    inter = np.ones((len(b), len(b)))
    for c in range(3):
        inter = inter * np.maximum(0, np.minimum.outer(b[:, 3 + c], b[:, 3 + c]) - np.maximum.outer(b[:, c], b[:, c]))
    with np.errstate(all="ignore"):
        out = inter / np.minimum.outer(vol, vol)
    out[np.isnan(out)] = 0
    return out


def cosine_matrix(x):
    x = np.asarray(x, np.float64)
    nrm = np.linalg.norm(x, axis=1)
    with np.errstate(all="ignore"):
        return (x @ x.T) / (nrm[:, None] * nrm[None])


# ------------------------------------------------------------------------------------------------------------- overlap
def overlap_counts(clouds, thr):
    """count[a][b] = points of a whose nearest point of b is nearer than thr (compute_point_cloud_distance < dis_thre);
    also the smallest | d - thr | met."""
    C = len(clouds)
    out = np.zeros((C, C), np.int64)
    gap = np.inf
    for b in range(C):
        if len(clouds[b]) == 0:
            continue
        tree = cKDTree(clouds[b])
        for a in range(C):
            if len(clouds[a]) == 0:
                continue
            d, _ = tree.query(clouds[a])
            out[a, b] = int((d < thr).sum())
            gap = min(gap, float(np.abs(d - thr).min()))
    return out, gap


# -------------------------------------------------------------------------------------------------------- host policies
def filter_rare(ids, min_count):
    """filter_id: ids seen at most min_count times become 999."""
    c = Counter(ids)
    return [999 if c[i] <= min_count else i for i in ids]


def mode_first(values):
    """The most frequent value; a tie goes to the value met first in raster order."""
    values = np.asarray(values).ravel()
    best, best_n, seen = None, 0, {}
    for v in values.tolist():
        seen[v] = seen.get(v, 0) + 1
    for v in values.tolist():
        if seen[v] > best_n:
            best, best_n = v, seen[v]
    return best


def check_similarity(bg, v, threshold):
    return any(float(np.dot(b, v)) > threshold for b in bg)


def merge_mapping(keys, sim_pc, capft, color, wall, floor, ceiling, cap_thre, weight_pc, weightcaption, weightcolor):
    """compute_similarity_matrix_thre's mapping loop, as written (its `continue` order included)."""
    n = len(keys)
    sim_cap = np.zeros((n, n)); sim_col = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            sim_cap[i, j] = sim_cap[j, i] = np.dot(capft[i], capft[j])
            sim_col[i, j] = sim_col[j, i] = np.dot(color[i], color[j])
    sim = (sim_pc > weight_pc) & (sim_cap > weightcaption) & (sim_col > weightcolor) | (sim_pc > 0.9)
    mapping, counter = {}, 4
    for i in range(n):
        for j in range(i + 1, n):
            if check_similarity(wall, capft[i], cap_thre):
                mapping[keys[i]] = 1
                continue
            elif check_similarity(floor, capft[i], cap_thre):
                mapping[keys[i]] = 2
                continue
            elif check_similarity(ceiling, capft[i], cap_thre):
                mapping[keys[i]] = 3
                continue
            if check_similarity(wall, capft[j], cap_thre):
                mapping[keys[j]] = 1
                continue
            elif check_similarity(floor, capft[j], cap_thre):
                mapping[keys[j]] = 2
                continue
            elif check_similarity(ceiling, capft[j], cap_thre):
                mapping[keys[j]] = 3
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
    mapping[999] = 0
    return mapping, counter


# ------------------------------------------------------------------------------------------- mask clouds of one frame
def voxel_down(points, voxel):
    """open3d's voxel_down_sample: index floor((p - (min - voxel / 2)) / voxel), the voxel's points averaged in input
    order; voxels in ascending (iz, iy, ix) order (open3d's own order is its hash map's)."""
    if len(points) == 0:
        return points
    vmin = points.min(axis=0) - voxel * 0.5
    idx = np.floor((points - vmin) / voxel).astype(np.int64)
    order = np.lexsort((idx[:, 0], idx[:, 1], idx[:, 2]))          # stable: equal voxels keep the input order
    s = idx[order]
    head = np.ones(len(s), bool)
    head[1:] = (s[1:] != s[:-1]).any(axis=1)
    out = []
    for a, b in zip(np.flatnonzero(head), list(np.flatnonzero(head)[1:]) + [len(s)]):
        acc = np.zeros(3)
        for p in points[order[a:b]]:
            acc = acc + p
        out.append(acc / float(b - a))
    return np.array(out)


def project_masks(masks, depth_raw, bgr, pose, depth_scale, intr, if_filter=True):
    """project_mask_pc for one frame -> (points, boxes, histograms, filtered masks, mask_ok)."""
    from scipy import ndimage
    fx, fy, cx, cy = (np.float32(v) for v in intr)
    depth = (depth_raw / depth_scale).astype(np.float32)
    depth[depth < 0.07] = 0
    depth[depth > 10] = 0
    valid = depth > 0
    P = np.asarray(pose, np.float64)
    pcs, boxes, hists, outs, ok = [], [], [], [], np.ones(len(masks), bool)
    for i, raw in enumerate(masks):
        mask = raw & valid
        if not mask.any():
            ok[i] = False
            continue
        lab, k = ndimage.label(raw, structure=np.ones((3, 3), int))
        comps = sorted(range(1, k + 1), key=lambda c: int(np.flatnonzero(lab.ravel() == c)[0]))
        new = mask.copy()
        pts = []
        for c in comps:
            cm = (lab == c) & valid
            if cm.sum() < 100:
                if if_filter:
                    new[cm] = False
                continue
            v, u = np.nonzero(cm)
            d = depth[cm]
            x = (u.astype(np.float32) - cx) * d / fx
            y = (v.astype(np.float32) - cy) * d / fy
            x, y, z = x.astype(np.float64), y.astype(np.float64), d.astype(np.float64)
            w = np.stack([((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)], axis=1)
            if if_filter:
                keep = denoise(w, 0.05, (100, 20, 10))
                new[cm] = keep
                pts.append(w[keep])
            else:
                w = voxel_down(w, 0.025)
                pts.append(w[denoise(w, 0.05, (10, 2, 1))])
        pc = np.concatenate(pts) if pts else np.zeros((0, 3))
        if len(pc) < 10:
            ok[i] = False
            continue
        pcs.append(pc)
        boxes.append(np.concatenate([pc.min(axis=0), pc.max(axis=0)]))
        hists.append(np.concatenate([np.bincount(bgr[..., c][mask] >> 3, minlength=32) for c in range(3)]).astype(np.float32))
        outs.append(new)
    return pcs, boxes, hists, outs, ok
