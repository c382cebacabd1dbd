"""Rigid alignment of a point cloud, or of a depth frame, to the finished map on the GPU.

    python -m openobj_amd.map_align --logdir DIR --points cloud.{npy,npz,ply} [--init T.txt] --out DIR
    python -m openobj_amd.map_align --logdir DIR --config scene.json [--frames a:b:s] [--stride n] --out DIR

A cloud that is almost in the map's frame -- a ground-truth mesh with a small offset, a second session, a robot that
re-enters the room with an approximate pose -- is brought into it by Gauss-Newton on the map's own field.  Every object
is an occupancy network whose alpha = 10 * raw (model.py:88) is positive inside and zero on the surface, so for a point q

    d(q) = alpha(q) / max(|grad alpha(q)|, g_min)          (metres, positive inside; first-order distance to the surface)

of the candidate object with the smallest |d| (MapPoints.surface) is the residual, and with n = grad / max(|grad|, g_min)
its derivative in a small motion (omega, v) of the cloud about a pivot c is J = [(q - c) x n, n].  Per iteration:

1. q = float32(T p), formed in fp64 on the device;
2. the candidate lists of the map at q, the field gradients of every segment, the selection (MapPoints.surface);
3. the normal equations A = sum J J^T, b = sum J d over the inliers |d| <= tau, about a pivot fixed at the first
   iteration's centroid (objnerf_mapalign_accumulate: 29 doubles, summed in an order that depends on N alone);
4. one read-back of the 29 doubles; on the host, in fp64, (A + damping diag A) xi = -b and T <- Exp(xi) about the pivot . T.

Host synchronisations of an iteration: that read-back, and the read-back of the segment offsets in ops.mappoints_count
(once per call of the candidate lists, i.e. once more for every halving under the pair budget); the first iteration
also reads the pivot back.  It stops when both the rotation and the translation of a step fall below tol.  Two runs on
the same device give the same bits: the kernels' sums have an order fixed by N; the pivot alone is a torch reduction
(`mean` in fp64, which torch computes without atomics, so it repeats run to run but its order is torch's, not this
project's; any pivot gives a valid step, it only conditions A).

Points may be given on the host or on the device: like MapPoints.label, fit moves them to the map's device; a map that
is not on a GPU is rejected (there is no CPU path).  The reference has no counterpart: it takes its poses from an external
SLAM and never differentiates a network in position.

--points writes align.json (T, history) and aligned.ply; --config refines the poses of a sequence against the map, frame
by frame from the dataset's own poses, and writes poses_refined.txt (one row-major 4 x 4 T_WC per line, the format of
the dataset's traj_w_c.txt, one line per refined frame) and align_frames.json."""
from __future__ import annotations

import argparse
import json
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from .map_points import DEFAULT_G_MIN, MapPoints

DEFAULT_TAU = 0.1            # ASSUMED default: the inlier gate on |d|, metres (DEFAULT_G_MIN, likewise assumed: map_points.py)
MIN_INLIERS = 6
MAX_COND = 1e12              # one plane or one sphere leaves directions of the pose undetermined


def hat(w) -> np.ndarray:
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], np.float64)


def exp_se3(xi) -> np.ndarray:
    """xi = (omega [3], v [3]) -> the 4 x 4 matrix exponential of [[hat(omega), v], [0, 0]] in closed form (Rodrigues; the
    series of the coefficients below 1e-4 rad, where the closed forms cancel)."""
    xi = np.asarray(xi, np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    W = hat(w)
    W2 = W @ W
    if th < 1e-4:
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th ** 3)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * W + b * W2
    T[:3, 3] = (np.eye(3) + b * W + c * W2) @ v
    return T


def about(T: np.ndarray, pivot) -> np.ndarray:
    """The motion T expressed about `pivot`: x -> pivot + T (x - pivot)."""
    c = np.asarray(pivot, np.float64).reshape(3)
    P, Pi = np.eye(4), np.eye(4)
    P[:3, 3], Pi[:3, 3] = c, -c
    return P @ T @ Pi


def unpack_sums(sums):
    """The 29 doubles of objnerf_mapalign_accumulate -> (A [6, 6] symmetric, b [6], sum d^2, inliers)."""
    s = np.asarray(sums, np.float64).reshape(29)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    A = A + np.triu(A, 1).T
    return A, s[21:27].copy(), float(s[27]), int(round(float(s[28])))


def gauss_newton_step(sums, damping: float):
    """-> (xi or None, info): None for fewer than MIN_INLIERS inliers or cond(A) > MAX_COND."""
    A, b, ss, n_in = unpack_sums(sums)
    info = {"inliers": n_in, "rms": float(np.sqrt(ss / n_in)) if n_in else float("nan"), "cond": float("inf")}
    if n_in < MIN_INLIERS or not np.isfinite(A).all() or not np.isfinite(b).all():
        return None, info
    info["cond"] = float(np.linalg.cond(A))
    if not info["cond"] <= MAX_COND:
        return None, info
    xi = np.linalg.solve(A + float(damping) * np.diag(np.diag(A)), -b)
    return xi, info


class MapAlign:
    def __init__(self, mp: MapPoints):
        self.mp = mp

    def fit(self, points, T0=None, iters: int = 20, tau: float = DEFAULT_TAU, g_min: float = DEFAULT_G_MIN,
            damping: float = 1e-6, tol: Sequence[float] = (1e-7, 1e-7), stats: Optional[dict] = None):
        """points [N, 3] in their own frame, T0 an initial 4 x 4 (identity) -> dict(T fp64 [4, 4] taking the points into the
        map's frame, converged, history: per iteration inliers, rms of d (m), the step's rotation (rad) and translation (m),
        cond(A)).  Fewer than 6 inliers or cond(A) > 1e12 ends the run with converged = False and the last valid T.
        Points on the host are moved to the map's device (MapPoints.label's contract); a map on the CPU raises."""
        pts = torch.as_tensor(points)
        if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
            raise _lib.ObjnerfError(f"MapAlign.fit: expected points [N >= 1, 3], got {tuple(pts.shape)}")
        if not pts.is_cuda and torch.device(self.mp.device).type != "cuda":
            raise _lib.ObjnerfError("MapAlign.fit: expected a GPU map (there is no CPU path)")
        if not (tau >= 0 and g_min > 0 and damping >= 0 and iters >= 0):
            raise _lib.ObjnerfError(f"MapAlign.fit: tau = {tau}, g_min = {g_min}, damping = {damping}, iters = {iters}")
        pts = pts.to(self.mp.device, torch.float32).contiguous()
        T = np.eye(4) if T0 is None else np.array(T0, np.float64).reshape(4, 4)
        if not np.isfinite(T).all():
            raise _lib.ObjnerfError("MapAlign.fit: T0 is not finite")
        pivot, history, converged = None, [], False
        sums = torch.empty(ops.MAPALIGN_SUMS, dtype=torch.float64, device=pts.device)
        with torch.no_grad():
            for _ in range(int(iters)):
                q = ops.mapalign_transform(pts, T)
                if pivot is None:                                   # fixed for the whole run: the first centroid
                    pivot = q.double().mean(dim=0).cpu().numpy()
                s = self.mp.surface(q, g_min=g_min, stats=stats)
                ops.mapalign_accumulate(q, s["obj"], s["alpha"], s["grad"], pivot, tau, g_min, out=sums)
                xi, info = gauss_newton_step(sums.cpu().numpy(), damping)      # the iteration's one read-back
                if xi is None:
                    history.append(dict(info, rot=float("nan"), trans=float("nan")))
                    break
                T = about(exp_se3(xi), pivot) @ T
                rot, trans = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]))
                history.append(dict(info, rot=rot, trans=trans))
                if rot < tol[0] and trans < tol[1]:
                    converged = True
                    break
        return {"T": T, "converged": converged, "history": history}

    def fit_frame(self, depth, T_WC0, rays_dir, stride: int = 4, **kw):
        """One depth frame against the map: depth [W, H] (metres, 0 = invalid), rays_dir [W, H, 3] the z-depth rays of
        vmap.cameraInfo (p_C = depth * ray), T_WC0 the approximate pose.  Every `stride`-th pixel of both axes with a valid
        depth is back-projected into the camera frame and fitted: T is the refined T_WC."""
        dev = self.mp.device
        d = torch.as_tensor(np.asarray(depth) if not torch.is_tensor(depth) else depth).to(dev, torch.float32)
        rays = torch.as_tensor(rays_dir).to(dev, torch.float32)
        if d.dim() != 2 or tuple(rays.shape) != (*d.shape, 3) or int(stride) < 1:
            raise _lib.ObjnerfError(f"MapAlign.fit_frame: depth [W, H], rays_dir [W, H, 3], stride >= 1; got {tuple(d.shape)}, "
                                    f"{tuple(rays.shape)}, {stride}")
        d, rays = d[::stride, ::stride], rays[::stride, ::stride]
        ok = torch.isfinite(d) & (d > 0)
        pts_c = (d[..., None] * rays)[ok]
        if pts_c.shape[0] == 0:
            return {"T": np.array(T_WC0, np.float64).reshape(4, 4), "converged": False, "history": []}
        return self.fit(pts_c, T0=T_WC0, **kw)


# ----------------------------------------------------------------------------------------------------------------- CLI
def parse_frames(spec: Optional[str], n: int):
    """'a:b:s' (python slice syntax, any part may be empty) over the dataset's n samples."""
    if spec is None:
        return list(range(n))
    parts = spec.split(":")
    if len(parts) > 3 or len(parts) < 1:
        raise ValueError(f"--frames: expected a:b:s, got {spec!r}")
    vals = [int(x) if x.strip() else None for x in parts] + [None] * (3 - len(parts))
    if len(parts) == 1:
        if vals[0] is None:
            raise ValueError(f"--frames: expected a:b:s, got {spec!r}")
        vals = [vals[0], vals[0] + 1, None]
    if vals[2] is not None and vals[2] < 1:
        raise ValueError("--frames: the step must be positive")
    return list(range(n))[slice(*vals)]


def read_pose(path: str) -> np.ndarray:
    T = np.loadtxt(path, dtype=np.float64).reshape(-1)
    if T.size != 16:
        raise ValueError(f"--init: expected 16 numbers (a row-major 4 x 4), got {T.size}")
    return T.reshape(4, 4)


def write_poses(path: str, poses) -> None:
    """One row-major 4 x 4 per line, space-separated: the format of the dataset's traj_w_c.txt."""
    np.savetxt(path, np.asarray(poses, np.float64).reshape(-1, 16), delimiter=" ", fmt="%.17g")


def _history_json(h):
    return [{k: (None if isinstance(v, float) and not np.isfinite(v) else v) for k, v in it.items()} for it in h]


def align_points(mp: MapPoints, points: np.ndarray, T0, out_dir: str, **kw):
    from . import mesh
    res = MapAlign(mp).fit(points, T0=T0, **kw)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "align.json"), "w") as fh:
        json.dump({"T": res["T"].tolist(), "converged": bool(res["converged"]), "history": _history_json(res["history"])},
                  fh, indent=1)
    moved = np.asarray(points, np.float64) @ res["T"][:3, :3].T + res["T"][:3, 3]
    mesh.TriMesh(moved, np.zeros((0, 3), np.int64)).export(os.path.join(out_dir, "aligned.ply"))
    return res


def align_frames(mp: MapPoints, cfg, frames: Optional[str], stride: int, out_dir: str, **kw):
    from . import dataset, map_cull
    c = map_cull._config(cfg)
    if c.dataset_format not in ("Replica", "ScanNet"):
        raise ValueError("Dataset format {} not found".format(c.dataset_format))
    ds = (dataset.Replica if c.dataset_format == "Replica" else dataset.ScanNet)(c)
    ids = parse_frames(frames, len(ds))
    fx, fy, cx, cy = map_cull.intrinsics_of(c)
    rays, al = None, MapAlign(mp)
    poses, report = [], []
    for i in ids:
        depth, T_WC = ds.depth_and_pose(i)
        if rays is None:
            rays = ops.rays_dirs(int(depth.shape[0]), int(depth.shape[1]), fx, fy, cx, cy, mp.device)
        res = al.fit_frame(depth, T_WC, rays, stride=stride, **kw)
        poses.append(res["T"])
        report.append({"frame": int(i), "converged": bool(res["converged"]), "history": _history_json(res["history"])})
    os.makedirs(out_dir, exist_ok=True)
    write_poses(os.path.join(out_dir, "poses_refined.txt"), poses)
    with open(os.path.join(out_dir, "align_frames.json"), "w") as fh:
        json.dump({"frames": report}, fh, indent=1)
    return poses, report


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--logdir", required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--points", help="cloud.npy / .npz / .ply, [N, 3] in the cloud's own frame")
    src.add_argument("--config", help="scene.json: refine the poses of the sequence's frames against the map")
    ap.add_argument("--init", default=None, help="T.txt: the initial 4 x 4 of --points (identity)")
    ap.add_argument("--frames", default=None, help="a:b:s over the dataset's samples (--config)")
    ap.add_argument("--stride", type=int, default=4, help="pixel stride of the back-projection (--config)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tau", type=float, default=DEFAULT_TAU, help="inlier gate on |d| in metres (an assumed default)")
    ap.add_argument("--g-min", type=float, default=DEFAULT_G_MIN, help="floor of |grad alpha| (an assumed default)")
    ap.add_argument("--damping", type=float, default=1e-6)
    ap.add_argument("--bg-ids", type=int, nargs="*", default=[0])
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None, _map_factory=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.init is not None and a.points is None:
        ap.error("--init goes with --points")
    if a.frames is not None and a.config is None:
        ap.error("--frames goes with --config")
    if a.stride < 1:
        ap.error("--stride must be positive")
    kw = dict(iters=a.iters, tau=a.tau, g_min=a.g_min, damping=a.damping)
    make = _map_factory or (lambda: MapPoints.from_logdir(a.logdir, a.device, bg_ids=a.bg_ids))
    if a.points is not None:
        from .map_points import read_points
        points = read_points(a.points)
        T0 = read_pose(a.init) if a.init else None
        res = align_points(make(), points, T0, a.out, **kw)
        last = res["history"][-1] if res["history"] else {}
        print(f"{len(points)} points, converged {res['converged']}, {len(res['history'])} iterations, "
              f"{last.get('inliers', 0)} inliers, rms {last.get('rms', float('nan')):.3g} m")
        return res
    poses, report = align_frames(make(), a.config, a.frames, a.stride, a.out, **kw)
    print(f"{len(poses)} frames, {sum(r['converged'] for r in report)} converged")
    return poses, report


if __name__ == "__main__":
    main()
