"""Test helper: numpy restatements of objnerf_meshcull.hip and the small scenes its tests share.

views_ref is the visibility rule, every operation a separate numpy fp64 operation in the kernel's order (numpy does not
contract); compact_ref is the compaction.  The GPU tests compare with array_equal: no tolerance."""
import numpy as np

import scene_files as SF

INTR = (SF.FX, SF.FY, SF.CX, SF.CY)


def views_ref(verts, T_CW, depth, intrinsics, z_min=0.0, eps=0.05, margin=0):
    """verts [V, 3] f64, T_CW [B, 3, 4] f64, depth [B, W, H] f32 -> int32 [V], the number of frames that see each vertex."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    T_CW = np.asarray(T_CW, np.float64).reshape(-1, 3, 4)
    depth = np.asarray(depth, np.float32)
    fx, fy, cx, cy = (np.float64(x) for x in intrinsics)
    B, W, H = depth.shape
    px, py, pz = verts[:, 0], verts[:, 1], verts[:, 2]
    views = np.zeros(len(verts), np.int32)
    with np.errstate(all="ignore"):
        for f in range(len(T_CW)):
            M = T_CW[f].reshape(12)
            row = lambda r: ((M[4 * r] * px + M[4 * r + 1] * py) + M[4 * r + 2] * pz) + M[4 * r + 3]
            xc, yc, zc = row(0), row(1), row(2)
            front = zc > z_min
            u = (fx * xc) / zc + cx
            v = (fy * yc) / zc + cy
            iu, iv = np.floor(u + 0.5), np.floor(v + 0.5)
            inside = front & (iu >= margin) & (iu <= W - 1 - margin) & (iv >= margin) & (iv <= H - 1 - margin)
            ii = np.where(inside, iu, 0.0).astype(np.int64)
            jj = np.where(inside, iv, 0.0).astype(np.int64)
            d = depth[f][ii, jj].astype(np.float64)
            views += (inside & (d > 0) & (zc <= d + np.float64(eps))).astype(np.int32)
    return views


def compact_ref(keep_v, faces, rule="all"):
    """-> dict(new_of_old int32 [V], old_of_new int32 [Vn], faces int32 [Fn, 3], face_old int32 [Fn], bad bool)."""
    keep_v = np.asarray(keep_v).astype(bool).reshape(-1)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(keep_v)
    ok = ((faces >= 0) & (faces < V)).all(axis=1)
    k = keep_v[np.where(ok[:, None], faces, 0)] if V else np.zeros(faces.shape, bool)
    stay = ok & (k.all(axis=1) if rule == "all" else k.any(axis=1))
    face_old = np.flatnonzero(stay)
    used = np.zeros(V, bool)
    used[faces[stay].reshape(-1)] = True
    old_of_new = np.flatnonzero(used)
    new_of_old = np.full(V, -1, np.int64)
    new_of_old[old_of_new] = np.arange(len(old_of_new))
    return {"new_of_old": new_of_old.astype(np.int32), "old_of_new": old_of_new.astype(np.int32),
            "faces": new_of_old[faces[stay]].astype(np.int32).reshape(-1, 3), "face_old": face_old.astype(np.int32),
            "bad": bool((~ok).any())}


def to_cw(T_WC):
    """[B, 4, 4] -> the [B, 3, 4] rows the rule takes: inverted on the host in float64, as map_cull.world_to_camera does."""
    return np.ascontiguousarray(np.linalg.inv(np.asarray(T_WC, np.float64).reshape(-1, 4, 4))[:, :3, :])


# ------------------------------------------------------------------------------------------------------------- scenes
def scene_depth(n_frames=4, as_loaded=False):
    """The depth images of scene_files' frames 0, 10, 20, ... in the project's layout [B, W, H] f32 metres, and their
    poses [B, 4, 4] (a pan of 0.02 m a frame).  Millimetres / 1000 (the wall at exactly 3 m, the boxes at 1.5 and 2 m);
    as_loaded: millimetres * fp32(0.001) as dataset.py scales them (the wall at 3.0000002 m)."""
    depth, poses = [], []
    for i in range(n_frames):
        _, d, _ = SF._frame(i, None)
        d = d.astype(np.float32)
        depth.append((d * np.float32(1.0 / 1000.0) if as_loaded else d / np.float32(1000.0)).T)
        T = np.eye(4)
        T[0, 3] = 0.02 * i
        poses.append(T)
    return np.stack(poses), np.ascontiguousarray(np.stack(depth))


def backproject(iu, iv, z):
    """The camera-frame point of frame 0 that projects to (iu, iv) (real-valued pixel coordinates) at depth z."""
    return np.array([(iu - SF.CX) * z / SF.FX, (iv - SF.CY) * z / SF.FY, z], np.float64)


def grid_mesh(nx, ny, x0, x1, y0, y1, z):
    """An nx x ny vertex grid over [x0, x1] x [y0, y1] at depth z, row-major in y then x; two triangles a cell."""
    xs, ys = np.linspace(x0, x1, nx), np.linspace(y0, y1, ny)
    X, Y = np.meshgrid(xs, ys)
    v = np.stack([X.ravel(), Y.ravel(), np.full(X.size, float(z))], 1)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).ravel()
    f = np.stack([np.stack([i, i + 1, i + nx], 1), np.stack([i + 1, i + nx + 1, i + nx], 1)], 1).reshape(-1, 3)
    return v, f.astype(np.int64)


def plane(z=3.0):
    return grid_mesh(97, 97, -2.0, 2.0, -1.5, 1.5, z)


def box_mesh(lo, hi):
    """A closed box: 8 corners, 12 triangles."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float64)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.int64)
    return v, f


def boundary_vertices():
    """(vertices [n, 3], expected seen [n] under margin 0, names): the single-vertex facts of the rule on frame 0 of the
    scene (wall at 3 m, box at 1.5 m over columns 8..27, rows 10..33), eps = 0.05."""
    rows = [
        ("wall pixel", backproject(2, 20, 3.0), True),
        ("behind the box", backproject(15, 20, 3.0), False),
        ("on the box", backproject(15, 20, 1.5), True),
        ("in front of the box", backproject(15, 20, 1.0), True),
        ("eps behind the wall", np.array([0.0, 0.0, 3.05]), True),
        ("one ulp more", np.array([0.0, 0.0, np.nextafter(3.05, 4.0)]), False),
        ("z = 0", np.array([0.1, 0.1, 0.0]), False),
        ("z < 0", np.array([0.1, 0.1, -2.0]), False),
        ("nan x", np.array([np.nan, 0.0, 3.0]), False),
        ("nan z", np.array([0.0, 0.0, np.nan]), False),
        ("+inf z", np.array([0.0, 0.0, np.inf]), False),
        ("-inf x", np.array([-np.inf, 0.0, 3.0]), False),
        ("+inf y", np.array([0.0, np.inf, 3.0]), False),
        ("1e300", np.array([1e300, 1e300, 1e300]), False),
        ("huge over tiny", np.array([1e30, 1e30, 1e-300]), False),
        ("u = 63.49", backproject(63.49, 20, 3.0), True),
        ("u above 63.5", backproject(63.5001, 20, 3.0), False),
        ("u = -0.49", backproject(-0.49, 20, 3.0), True),
        ("u below -0.5", backproject(-0.5001, 20, 3.0), False),
        ("v = 47.49", backproject(40, 47.49, 3.0), True),
        ("v above 47.5", backproject(40, 47.5001, 3.0), False),
        ("column 1", backproject(1, 20, 3.0), True),
        ("column 2", backproject(2, 5, 3.0), True),
    ]
    return np.stack([r[1] for r in rows]), np.array([r[2] for r in rows]), [r[0] for r in rows]
