"""Test helper: a numpy / scipy statement of sceneObject.get_bound (vmap.py:287-384), written independently of
openobj_amd/bounds.py.  The reference runs open3d 0.16 (create_from_depth_image, voxel_down_sample) and trimesh 4.1.4
(bounds.oriented_bounds(points, ordered=True)); neither is available, so this restates them:

  back-projection   pixels (row i, column j) with state == 1 and depth z > 0, x = (j - cx) z / fx, y = (i - cy) z / fy
                    in fp64, p = camera_pose (x, y, z, 1), camera_pose = inv64(inv32(twc)); (slot, i, j) order
  voxel_down        vmin = min - voxel / 2, index floor((p - vmin) / voxel), centroid = in-order sum / count
  oriented_bounds   for every distinct hull-facet normal n (equal within 1e-9 = one): the minimum-area rectangle of the
                    hull vertices' projection onto the plane normal to n over the edges of that projection's 2-D hull
                    (trimesh's oriented_bounds_2D) x the height along n; the smallest volume.  No bucketing of normals
                    (trimesh's angle_digits=1 keeps one per 0.1-rad bucket): this candidate set contains trimesh's.
                    A set qhull rejects: trimesh's coplanar route (SVD plane, 2-D box, thickness 0); rank < 2: None.
  ordering          extents ascending, det R = +1; floor at 0.10; corners as vmap.py:350-361."""
import numpy as np
from scipy.spatial import ConvexHull, QhullError

CORNERS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1],
                    [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]])


def camera_pose(twc):
    return np.linalg.inv(np.linalg.inv(np.asarray(twc, np.float32)).astype(np.float64))


def backproject(depth_wh, state_wh, twc, fx, fy, cx, cy):
    """depth_wh f32 [W, H], state_wh u8 [W, H] (the store's transposed layout), twc [4, 4] -> fp64 [n, 3]."""
    P = camera_pose(twc)
    d = np.asarray(depth_wh, np.float32).T.copy()                   # [H, W]
    d[np.asarray(state_wh).T != 1] = 0
    ii, jj = np.nonzero(d > 0)                                      # row-major: i, then j
    z = d[ii, jj].astype(np.float64)
    x = (jj.astype(np.float64) - cx) * z / fx
    y = (ii.astype(np.float64) - cy) * z / fy
    return np.stack([P[r, 0] * x + P[r, 1] * y + P[r, 2] * z + P[r, 3] for r in range(3)], axis=1)


def object_points(depth, state, twc, n_keyframes, intr):
    """The concatenated cloud of slots 0 .. n_keyframes-1 (depth [F, W, H], state [F, W, H], twc [F, 4, 4])."""
    pts = [backproject(depth[k], state[k], twc[k], *intr) for k in range(n_keyframes)]
    return np.concatenate(pts) if pts else np.zeros((0, 3))


def voxel_down(points, voxel=0.05):
    """-> (voxel indices int64 [n, 3] in lexicographic order, centroids [n, 3])."""
    if len(points) == 0:
        return np.zeros((0, 3), np.int64), np.zeros((0, 3))
    vmin = points.min(axis=0) - voxel * 0.5
    idx = np.floor((points - vmin) / voxel).astype(np.int64)
    uniq, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv).astype(np.float64)
    cen = np.stack([np.bincount(inv, weights=points[:, c]) for c in range(3)], axis=1) / cnt[:, None]
    return uniq, cen


def distinct_normals(N, tol=1e-9):
    """Facet normals, one per group of rows equal within tol (lexicographic neighbours)."""
    order = np.lexsort(N.T[::-1])
    s = N[order]
    keep = np.ones(len(order), bool)
    keep[1:] = np.abs(np.diff(s, axis=0)).max(axis=1) > tol
    return N[np.sort(order[keep])]


def _plane_basis(n):
    a = np.cross(n, [1.0, 0, 0] if abs(n[0]) < 0.9 else [0, 1.0, 0])
    a /= np.linalg.norm(a)
    return a, np.cross(n, a)


def _min_rect(V, n):
    """Minimum-area rectangle of V's projection onto the plane normal to n -> (area, u, v) (u, v world unit axes)."""
    a, b = _plane_basis(n)
    P2 = np.stack([V @ a, V @ b], axis=1)
    h = ConvexHull(P2)
    e = P2[h.simplices[:, 1]] - P2[h.simplices[:, 0]]
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    pu = P2 @ e.T                                                   # [nv, ne]
    pv = P2 @ np.stack([-e[:, 1], e[:, 0]], axis=1).T
    area = np.ptp(pu, axis=0) * np.ptp(pv, axis=0)
    i = int(np.argmin(area))
    u = e[i, 0] * a + e[i, 1] * b
    return float(area[i]), u, np.cross(n, u)


def oriented_bounds(points):
    """-> (R [3,3] columns = axes, extents [3] ascending unfloored, centre [3]) or None."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    if len(P) == 0:
        return None
    mean = P.mean(axis=0)
    q = P - mean
    try:
        hull = ConvexHull(q)
    except QhullError:
        if len(q) < 3:
            return None
        _, _, vh = np.linalg.svd(q, full_matrices=False)
        n = vh[2]
        try:
            _, u, v = _min_rect(q, n)
        except QhullError:
            return None
        R = np.stack([u, v, n], axis=1)
        loc = q @ R
        ext = np.array([np.ptp(loc[:, 0]), np.ptp(loc[:, 1]), 0.0])
        mid = np.array([(loc[:, 0].max() + loc[:, 0].min()) / 2, (loc[:, 1].max() + loc[:, 1].min()) / 2, 0.0])
        return _ordered(R, ext, R @ mid + mean)
    V = q[hull.vertices]
    best = None
    for n in distinct_normals(hull.equations[:, :3]):
        area, u, v = _min_rect(V, n)
        vol = area * np.ptp(V @ n)
        if best is None or vol < best[0]:
            best = (vol, u, v, n)
    _, u, v, n = best
    R = np.stack([u, v, n], axis=1)
    loc = V @ R
    lo, hi = loc.min(axis=0), loc.max(axis=0)
    return _ordered(R, hi - lo, R @ ((lo + hi) / 2) + mean)


def _ordered(R, ext, c):
    o = np.argsort(ext, kind="stable")
    R, ext = R[:, o].copy(), ext[o].copy()
    if np.linalg.det(R) < 0:
        R[:, 2] = -R[:, 2]
    return R, ext, c


def corners(R, extent, center):
    return np.dot(CORNERS * (np.asarray(extent) / 2), np.asarray(R).T) + center


def get_bound(points, voxel=0.05, min_extent=0.10):
    """Steps 2-4 on a raw cloud -> (R, extent floored, centre, corners) or None."""
    _, cen = voxel_down(points, voxel)
    ob = oriented_bounds(cen)
    if ob is None:
        return None
    R, ext, c = ob
    ext = np.maximum(ext, min_extent)
    return R, ext, c, corners(R, ext, c)


def box_contains(R, extent, center, points, tol=1e-9):
    loc = (np.asarray(points) - center) @ R
    return bool((np.abs(loc) <= np.asarray(extent) / 2 + tol).all())
