"""Object bounds from keyframes: sceneObject.get_bound (vmap.py:287-384) for a list of objects at once.

The reference builds each object's oriented 3-D box on the CPU, one object at a time, with open3d 0.16
(create_from_depth_image + voxel_down_sample(0.05)) and trimesh 4.1.4 (bounds.oriented_bounds(points, ordered=True)).
Neither library is used here; this restates the algorithm:

1. Back-projection (objnerf_voxel_scan / objnerf_voxel_emit, on the device keyframe stores): the pixels of keyframe
   slots 0 .. n_keyframes-1 whose state byte is 1 and whose depth z > 0 (NaN is dropped);
   x = (j - cx) z / fx, y = (i - cy) z / fy in fp64, p = camera_pose (x, y, z, 1) with camera_pose = inv64(inv32(twc))
   (the reference inverts twc in float32, open3d inverts that again in double); points in (slot, row i, column j) order.
2. voxel_down_sample: vmin = min(points) - voxel / 2, voxel index floor((p - vmin) / voxel), one point per occupied voxel
   = the fp64 sum of its points in input order / their count (a stable sort of the voxel keys, objnerf_voxel_heads /
   objnerf_voxel_centroids).  Voxel membership is exact against a numpy statement of the same formulas.
3. oriented_bounds: the convex hull of the centroids (scipy / qhull on the host; the sets are small), then for every
   candidate (hull-facet normal n, hull edge e) the box with axes u = e projected onto the plane normal to n, v = n x u,
   n; the smallest volume wins (objnerf_obb_search).  A set that qhull rejects as flat takes trimesh's coplanar route: the
   SVD plane normal, the minimum-AREA rectangle over the edges of the 2-D hull in that plane, thickness 0.  A set of
   rank < 2 (or empty) has no box: (None, None), where the reference prints "too few pcs obj".
   Deliberate deviation: trimesh tries one facet normal per 0.1-rad bucket of spherical angles (angle_digits=1), the
   first in qhull's facet order.  Here EVERY distinct facet normal is tried (normals equal within 1e-9 are one): a
   superset of trimesh's candidates, so the box is never larger than the reference's and is the same box whenever the
   bucket's representative was the optimal facet.  This is not parity with trimesh.
   For one normal only the silhouette edges are candidates (edges whose two facets face opposite ways along n, or one of
   them edge-on within 1e-12): the edges of the projection's 2-D hull are projections of those, and the minimum-area
   rectangle has a side on a 2-D hull edge, so nothing is lost.
4. ordered=True: extents ascending, axes permuted with them, the last axis negated when det R < 0; each extent floored
   at min_extent (0.10); the 8 corners as vmap.py:350-361.  The second box (open3d's, vmap.py:365-369) shares centre and
   R, with extents floored at 0.05.

Every step is deterministic (no float atomics; ties broken by the lowest candidate index): the same keyframes give the
same bytes, and an object's box does not depend on which other objects share the call."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import ObbArgs, ObjnerfError, VoxelArgs, check, lib
from .utils import BoundingBox

VOXEL_BYTES_PER_POINT = 80       # emitted point 24 + key 8; sorted key 8 + permutation 8; the sort's scratch ~32
DEFAULT_BUDGET = 3 << 29         # device bytes of the points of one chunk of objects (1.5 GiB: under 2 GiB with the rest)
KEY_BITS = 42                    # linear voxel index bits of the sort key (objnerf_voxel_emit)
EDGE_ON = 1e-12                  # |n . n_f| below this: facet f is edge-on along n (its edges are silhouette candidates)
NORMAL_EQ = 1e-9                 # facet normals equal within this are one candidate


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def camera_poses(twc) -> np.ndarray:
    """[..., 4, 4] camera-to-world poses -> open3d's camera_pose = inv64(inv32(twc)) (vmap.py:309-310 then
    CreatePointCloudFromFloatDepthImage's extrinsic.inverse())."""
    t = np.asarray(twc, dtype=np.float32)
    return np.linalg.inv(np.linalg.inv(t).astype(np.float64))


def intrinsics_of(intrinsic_open3d, obj) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy): from any object with a 3x3 `intrinsic_matrix` (open3d's PinholeCameraIntrinsic), else the
    object's own camera (its config's)."""
    if intrinsic_open3d is None:
        return tuple(float(v) for v in obj.intrinsics)
    m = np.asarray(intrinsic_open3d.intrinsic_matrix, dtype=np.float64)
    return float(m[0, 0]), float(m[1, 1]), float(m[0, 2]), float(m[1, 2])


# ---------------------------------------------------------------------------------------------------- voxel centroids
def objects_voxels(objects, intrinsic_open3d=None, voxel: float = 0.05, budget: int = DEFAULT_BUDGET,
                   stats: Optional[dict] = None) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Steps 1-2 for a list of sceneObjects: -> per object (voxel indices int64 [n, 3], centroids fp64 [n, 3]) in
    ascending linear-key order.  Objects sharing (slots, W, H, intrinsics) share one launch chain; the point work is
    chunked over objects so that at most `budget` device bytes hold points at once."""
    out: List[Optional[Tuple[np.ndarray, np.ndarray]]] = [None] * len(objects)
    groups = {}
    for i, o in enumerate(objects):
        # (dense and cropped keyframe stores go to separate launches: they are read through different descriptors)
        key = (o.keyframe_buffer_size, o.frames_width, o.frames_height, intrinsics_of(intrinsic_open3d, o),
               getattr(o, "crops", None) is not None)
        groups.setdefault(key, []).append(i)
    for (F, W, H, intr, _), idx in groups.items():
        res = _voxels_group([objects[i] for i in idx], F, W, H, intr, float(voxel), int(budget), stats)
        for i, r in zip(idx, res):
            out[i] = r
    return out


def _voxels_group(objs, F, W, H, intr, voxel, budget, stats):
    from . import ops
    K = len(objs)
    dev = objs[0].data_device
    table = ops.keyframe_table([o.keyframe_store() for o in objs])
    nk = [int(o.n_keyframes) for o in objs]
    if any(n < 0 or n > F for n in nk):
        raise ObjnerfError("object_bounds: n_keyframes outside the keyframe buffer")
    twc = torch.stack([o.t_wc_batch for o in objs]).cpu().numpy()            # [K, F, 4, 4]: one device -> host copy
    poses = np.zeros((K, F, 4, 4), np.float64)
    for k in range(K):
        if nk[k]:
            poses[k, :nk[k]] = camera_poses(twc[k, :nk[k]])
    poses_d = torch.from_numpy(poses).to(dev)
    nk_d = torch.tensor(nk, dtype=torch.int32).to(dev)
    fx, fy, cx, cy = intr
    cropped = table.shape[1] == 5                   # ops.keyframe_table of KeyframeCropStores: objnerf_kf_crops rows
    a = VoxelArgs(K, F, W, H, fx, fy, cx, cy, voxel, None if cropped else table.data_ptr(), nk_d.data_ptr(),
                  poses_d.data_ptr(), table.data_ptr() if cropped else None)
    nbytes = int(lib().objnerf_voxel_workspace_bytes(K, F, W, H))
    if nbytes == 0:
        raise ObjnerfError("objnerf_voxel_workspace_bytes returned 0")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    total = torch.empty(K, dtype=torch.int64, device=dev)
    minmax = torch.empty(K, 6, dtype=torch.float64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if stats is not None else None
    if ev:
        ev[0].record()
    check(lib().objnerf_voxel_scan(C.byref(a), _ptr(ws), nbytes, _ptr(total), _ptr(minmax), _stream()),
          "objnerf_voxel_scan")
    if ev:
        ev[1].record()
    tot = total.cpu().numpy()                                                 # the scan's one host sync
    if ev:
        stats["scan_ms"] = stats.get("scan_ms", 0.0) + ev[0].elapsed_time(ev[1])
        px = sum(int(o.crops.rect_host[:n, 2:].prod(axis=1).sum()) for o, n in zip(objs, nk)) if cropped else sum(nk) * W * H
        stats["scan_bytes"] = stats.get("scan_bytes", 0) + px * 8                  # depth + the rgbs line of the state
        stats["points"] = stats.get("points", 0) + int(tot.sum())
    mm = minmax.cpu().numpy()
    vmin = np.zeros((K, 3), np.float64)
    dims = np.ones((K, 3), np.int64)
    for k in range(K):
        if tot[k] == 0:
            continue
        if not np.isfinite(mm[k]).all():
            raise ObjnerfError(f"object_bounds: object {k} has non-finite points (depth inf)")
        vmin[k] = mm[k, :3] - voxel * 0.5                                     # open3d: min_bound - voxel_size3 * 0.5
        dims[k] = np.floor((mm[k, 3:] - vmin[k]) / voxel).astype(np.int64) + 1
        if float(np.prod(dims[k].astype(np.float64))) >= 2.0 ** KEY_BITS:
            raise ObjnerfError(f"object_bounds: object {k} spans {dims[k].tolist()} voxels (more than 2^{KEY_BITS})")
    vmin_d = torch.from_numpy(vmin).to(dev)
    dims_d = torch.from_numpy(np.ascontiguousarray(dims[:, :2])).to(dev)
    res: List[Tuple[np.ndarray, np.ndarray]] = [(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.float64))] * K
    per_chunk = max(1, budget // VOXEL_BYTES_PER_POINT)
    k = 0
    while k < K:                                    # chunks of consecutive objects: at least one, at most per_chunk points
        k0, n = k, 0
        while k < K and (k == k0 or n + int(tot[k]) <= per_chunk):
            n += int(tot[k])
            k += 1
        k1 = k
        if n == 0:
            continue
        base = np.zeros(K, np.int64)
        base[k0:k1] = np.concatenate([[0], np.cumsum(tot[k0:k1])[:-1]])
        base_d = torch.from_numpy(base).to(dev)
        if ev:
            ev[0].record()
        pts = torch.empty(n, 3, dtype=torch.float64, device=dev)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        check(lib().objnerf_voxel_emit(C.byref(a), _ptr(ws), nbytes, k0, k1, _ptr(base_d), _ptr(vmin_d), _ptr(dims_d), n,
                                       _ptr(pts), _ptr(keys), _stream()), "objnerf_voxel_emit")
        skeys, perm = torch.sort(keys, stable=True)          # equal keys keep the points' (slot, row, column) order
        del keys
        cen, vkeys, first = ops.run_centroids(skeys, perm, pts, k1 - k0)
        V = int(cen.shape[0])
        if ev:
            ev[1].record()
            ev[1].synchronize()
            stats["centroid_ms"] = stats.get("centroid_ms", 0.0) + ev[0].elapsed_time(ev[1])
            stats["voxels"] = stats.get("voxels", 0) + V
            stats["peak_points"] = max(stats.get("peak_points", 0), n)
            stats["chunks"] = stats.get("chunks", 0) + 1
        del pts, skeys, perm
        cen_h, vk_h, first_h = cen.cpu().numpy(), vkeys.cpu().numpy(), first.cpu().numpy()
        starts = [(int(first_h[j]), k0 + j) for j in range(k1 - k0) if first_h[j] >= 0]
        for t, (s, kk) in enumerate(starts):
            e = starts[t + 1][0] if t + 1 < len(starts) else V
            lk = vk_h[s:e]
            nx, ny = int(dims[kk, 0]), int(dims[kk, 1])
            idx = np.stack([lk % nx, (lk // nx) % ny, lk // (nx * ny)], axis=1)
            res[kk] = (idx, cen_h[s:e])
    return res


# ---------------------------------------------------------------------------------------------- oriented-box search
def _distinct_rows(N: np.ndarray) -> np.ndarray:
    """Indices of the rows of N kept as distinct, in their original order: in lexicographic order, a row equal within
    NORMAL_EQ to the row before it is dropped."""
    order = np.lexsort(N.T[::-1])
    s = N[order]
    keep = np.ones(len(order), bool)
    keep[1:] = np.abs(np.diff(s, axis=0)).max(axis=1) > NORMAL_EQ
    return np.sort(order[keep])


def hull_problem(points: np.ndarray):
    """The search's input for one point set -> dict(mode, offset, verts, normals, edges, cand) or None (rank < 2, or
    no point).  verts are relative to `offset` (the points' mean); edges index verts; cand = (normal row, edge row)."""
    from scipy.spatial import ConvexHull
    from scipy.spatial import QhullError
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(P) == 0:
        return None
    off = P.mean(axis=0)
    q = P - off
    try:
        h = ConvexHull(q)
    except QhullError:
        return _coplanar_problem(q, off)
    N = h.equations[:, :3]
    nd = _distinct_rows(N)
    normals = N[nd]
    # hull edges with their two facets: the edge opposite vertex j of facet f borders f and neighbors[f, j]
    f = np.repeat(np.arange(len(h.simplices)), 3)
    j = np.tile(np.arange(3), len(h.simplices))
    g = h.neighbors[f, j]
    sel = f < g
    f, j, g = f[sel], j[sel], g[sel]
    a = h.simplices[f, (j + 1) % 3]
    b = h.simplices[f, (j + 2) % 3]
    remap = np.full(len(q), -1, np.int64)
    remap[h.vertices] = np.arange(len(h.vertices))
    edges = np.stack([remap[a], remap[b]], axis=1).astype(np.int32)
    cand = []
    for c0 in range(0, len(normals), 256):                       # silhouette edges of every normal
        S = normals[c0:c0 + 256] @ N.T                           # [nn, n_facets]
        sa, sb = S[:, f], S[:, g]
        sil = (sa * sb <= 0) | (np.abs(sa) <= EDGE_ON) | (np.abs(sb) <= EDGE_ON)
        r, c = np.nonzero(sil)
        cand.append(np.stack([r + c0, c], axis=1))
    cand = np.concatenate(cand).astype(np.int32)
    return dict(mode=0, offset=off, verts=q[h.vertices], normals=normals, edges=edges, cand=cand)


def _coplanar_problem(q: np.ndarray, off: np.ndarray):
    """trimesh's coplanar route: the SVD plane of the demeaned points and the 2-D hull in it; None for rank < 2."""
    from scipy.spatial import ConvexHull
    from scipy.spatial import QhullError
    if len(q) < 3:
        return None
    _, _, vh = np.linalg.svd(q, full_matrices=False)
    p2 = q @ vh[:2].T
    try:
        h2 = ConvexHull(p2)
    except QhullError:
        return None
    remap = np.full(len(q), -1, np.int64)
    remap[h2.vertices] = np.arange(len(h2.vertices))
    edges = remap[h2.simplices].astype(np.int32)
    cand = np.stack([np.zeros(len(edges), np.int64), np.arange(len(edges))], axis=1).astype(np.int32)
    return dict(mode=1, offset=off, verts=q[h2.vertices], normals=vh[2][None].copy(), edges=edges, cand=cand)


def obb_search(problems: Sequence, device,
               stats: Optional[dict] = None) -> List[Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]]]:
    """objnerf_obb_search over the non-None problems in ONE launch -> per problem (R [3,3] with the box axes as
    columns u, v, n; extents [3]; centre [3] in world coordinates), unordered and unfloored; None where there is no box."""
    live = [i for i, p in enumerate(problems) if p is not None]
    out: List[Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]]] = [None] * len(problems)
    if not live:
        return out
    P = [problems[i] for i in live]
    K = len(P)
    nv = np.array([len(p["verts"]) for p in P], np.int64)
    nn = np.array([len(p["normals"]) for p in P], np.int64)
    ne = np.array([len(p["edges"]) for p in P], np.int64)
    nc = np.array([len(p["cand"]) for p in P], np.int64)
    n_off = np.concatenate([[0], np.cumsum(nn)[:-1]])
    e_off = np.concatenate([[0], np.cumsum(ne)[:-1]])
    cand = np.concatenate([p["cand"].astype(np.int64) + np.array([n_off[k], e_off[k]]) for k, p in enumerate(P)])
    if cand.max(initial=0) > 2 ** 31 - 1:
        raise ObjnerfError("obb_search: candidate index overflow")
    T = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(device)
    verts = T(np.concatenate([p["verts"] for p in P]), np.float64)
    normals = T(np.concatenate([p["normals"] for p in P]), np.float64)
    edges = T(np.concatenate([p["edges"] for p in P]), np.int32)
    cand_d = T(cand, np.int32)
    vert_off = T(np.concatenate([[0], np.cumsum(nv)]), np.int64)
    cand_off = T(np.concatenate([[0], np.cumsum(nc)]), np.int64)
    mode = T([p["mode"] for p in P], np.int32)
    n_split = int(max(1, min(64, (int(nc.max()) + 255) // 256)))
    ws = torch.empty(2 * K * n_split, dtype=torch.float64, device=device)
    res = torch.empty(K, 16, dtype=torch.float64, device=device)
    a = ObbArgs(K, 0, verts.data_ptr(), vert_off.data_ptr(), normals.data_ptr(), edges.data_ptr(), cand_d.data_ptr(),
                cand_off.data_ptr(), mode.data_ptr())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib().objnerf_obb_search(C.byref(a), n_split, _ptr(ws), _ptr(res), _stream()), "objnerf_obb_search")
    e1.record()
    r = res.cpu().numpy()
    if stats is not None:
        stats["search_ms"] = e0.elapsed_time(e1)
    for k, i in enumerate(live):
        if not np.isfinite(r[k, 15]):
            continue
        R = r[k, :9].reshape(3, 3).copy()
        ext = r[k, 9:12].copy()
        c = r[k, 12:15].copy()
        if P[k]["mode"] == 1:                           # trimesh: thickness 0, the centre in the points' mean plane
            n = R[:, 2]
            c = c - n * float(c @ n)
            ext[2] = 0.0
        out[i] = (R, ext, c + P[k]["offset"])
    return out


def finish_box(R: np.ndarray, ext: np.ndarray, c: np.ndarray, min_extent: float = 0.10):
    """ordered=True (extents ascending, det R = +1), the floor and the corners of vmap.py:340-370 -> (bbox3d, bbox)."""
    order = np.argsort(ext, kind="stable")
    R = R[:, order].copy()
    ext = ext[order].copy()
    if np.linalg.det(R) < 0:
        R[:, 2] = -R[:, 2]
    bbox = BoundingBox()
    bbox.center = np.asarray(c, np.float64).copy()
    bbox.R = R
    bbox.extent = np.maximum(ext, min_extent)
    half = bbox.extent / 2
    offs = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1],
                     [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]])
    bbox.points3d = np.dot(offs * half, bbox.R.T) + bbox.center
    bbox3d = BoundingBox()                                  # open3d's OrientedBoundingBox of vmap.py:365-369
    bbox3d.center, bbox3d.R = bbox.center.copy(), bbox.R.copy()
    bbox3d.extent = np.maximum(0.05, bbox.extent)
    bbox3d.points3d = np.dot(offs * (bbox3d.extent / 2), bbox3d.R.T) + bbox3d.center
    return bbox3d, bbox


def object_bounds(objects, intrinsic_open3d=None, voxel: float = 0.05, min_extent: float = 0.10,
                  budget: int = DEFAULT_BUDGET, stats: Optional[dict] = None):
    """sceneObject.get_bound's box for every object -> [(bbox3d, bbox) | (None, None)] (see the module docstring)."""
    import time
    t0 = time.perf_counter()
    vox = objects_voxels(objects, intrinsic_open3d, voxel, budget, stats)
    t1 = time.perf_counter()
    problems = [hull_problem(c) for _, c in vox]
    t2 = time.perf_counter()
    dev = objects[0].data_device if objects else "cuda"
    boxes = obb_search(problems, dev, stats)
    t3 = time.perf_counter()
    if stats is not None:
        stats.update(voxels_s=t1 - t0, hull_s=t2 - t1, search_s=t3 - t2,
                     hull_vertices=[0 if p is None else len(p["verts"]) for p in problems],
                     candidates=[0 if p is None else len(p["cand"]) for p in problems])
    return [(None, None) if b is None else finish_box(*b, min_extent=min_extent) for b in boxes]
