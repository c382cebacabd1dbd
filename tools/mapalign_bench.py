"""Field gradients and rigid alignment against the native map (openobj_amd/map_align.py, objnerf_mapalign.hip)
-> profiles/mapalign_bench.txt.

    python tools/mapalign_bench.py [--points 2000000] [--out profiles/mapalign_bench.txt] [--reps 7]

Shape: the native map of tools/mappoints_bench.py (synthetic.native_bound_map: 50 hidden-32 objects and the hidden-128
background, randomly initialised, out_alpha.bias = 1).  Two clouds:
  surface  tools/mappoints_bench.py's "surface" cloud, 2 M points by default -- an ASSUMPTION about the order of a room
           mesh's vertex count, not a measured figure;
  frame    one 1200 x 680 depth frame at stride 1 (816 000 points): the generator's smooth depth surface back-projected
           with its intrinsics, as MapAlign.fit_frame does.

Records, per cloud: the device-event time of every pass of ONE iteration (candidate lists, hidden-32 gradients, the
background's layer-wise chain, select + resolve, transform, accumulate; a synchronise per pass, median of reps calls); the
whole 10-iteration fit on the host clock, ending in a synchronise (tol = 0, so that all ten iterations run; the number that
ran is recorded); objnerf_mappoints_grad's pairs/s beside mp_eval_kernel's (ops.mappoints_eval without colour output
and without the feature) on the same pairs in the same process; and the baseline: the same iteration restated in torch on
the device -- the density trunk as torch ops on the same weights, autograd on the points, every object over ALL points, box
masks, a running arg-min of |d|, the normal equations in fp64, one read-back, the same host solve.  The baseline iteration
and the fit ALTERNATE in one process after a warm-up; every sample covers at least 0.3 s; median / min / max of reps
samples.  The networks are random, so the fit does not converge to anything: only its cost is measured here."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mappoints_bench as MB  # noqa: E402
from openobj_amd import map_align, map_points, ops  # noqa: E402

ITERS = 10


def frame_cloud(dev, W=1200, H=680):
    xs = torch.arange(W, device=dev, dtype=torch.float32)[:, None]
    ys = torch.arange(H, device=dev, dtype=torch.float32)[None, :]
    depth = 2.5 + 0.3 * torch.sin(xs / 150.0) + 0.2 * torch.cos(ys / 120.0)          # synthetic.native_bound_map, frame 0
    rays = ops.rays_dirs(W, H, 600.0, 600.0, (W - 1) / 2.0, (H - 1) / 2.0, dev)
    return (depth[..., None] * rays).reshape(-1, 3).contiguous()


def torch_nets(objects, dev):
    nets = []
    for o in objects:
        v = [t[0].detach().to(dev) for t in o.trainer.arena.views()]
        nets.append(dict(W0=v[0], b0=v[1], W1=v[2], b1=v[3], W2=v[4], b2=v[5], W3=v[6], b3=v[7], Wa=v[8], ba=v[9], B=v[18],
                         scale=float(o.trainer.obj_scale), oc=float(o.obj_center)))
    return nets


def torch_field(net, q):
    """alpha and d alpha / d q of one network in torch: octaves 0..3 only (the density trunk reads nothing else)."""
    q = q.detach().requires_grad_(True)
    t = (q - net["oc"]) / net["scale"]
    proj = t @ net["B"].t()
    bands = 2.0 ** torch.arange(4, device=q.device, dtype=torch.float32)
    x1 = torch.cat([t, torch.sin((proj[:, None, :] * bands[:, None]).reshape(q.shape[0], -1) * np.pi)], dim=1)
    h1 = torch.relu(x1 @ net["W0"].t() + net["b0"])
    h2 = torch.relu(h1 @ net["W1"].t() + net["b1"])
    h3 = torch.relu(torch.cat([h2, x1], dim=1) @ net["W2"].t() + net["b2"])
    h4 = torch.relu(h3 @ net["W3"].t() + net["b3"])
    alpha = ((h4 @ net["Wa"].t() + net["ba"]) * 10.0).squeeze(-1)
    (grad,) = torch.autograd.grad(alpha.sum(), q)
    return alpha.detach(), grad


def baseline_iteration(nets, mp, pts, T, pivot, tau, g_min, damping):
    dev = pts.device
    Td = torch.as_tensor(T, device=dev)
    q = (pts.double() @ Td[:3, :3].t() + Td[:3, 3]).float()
    N = q.shape[0]
    best = torch.full((N,), float("inf"), device=dev)
    b_alpha, b_grad = torch.zeros(N, device=dev), torch.zeros(N, 3, device=dev)
    for k, net in enumerate(nets):
        alpha, grad = torch_field(net, q)
        rec = mp.boxes[k]
        inside = (((q - rec[0:3]) @ rec[3:12].view(3, 3)).abs() <= rec[12:15]).all(dim=1)
        d = (alpha / grad.norm(dim=1).clamp(min=g_min)).abs()
        better = inside & (d < best)
        best = torch.where(better, d, best)
        b_alpha = torch.where(better, alpha, b_alpha)
        b_grad = torch.where(better[:, None], grad, b_grad)
    g = b_grad.double()
    den = g.norm(dim=1).clamp(min=g_min)
    d = b_alpha.double() / den
    keep = torch.isfinite(best) & (d.abs() <= tau)
    n = g / den[:, None]
    J = torch.cat([torch.linalg.cross(q.double() - torch.as_tensor(pivot, device=dev), n), n], dim=1)[keep]
    d = d[keep]
    A = J.t() @ J
    iu = torch.triu_indices(6, 6, device=dev)
    sums = torch.cat([A[iu[0], iu[1]], J.t() @ d, (d * d).sum()[None], keep.sum()[None].double()]).cpu().numpy()
    xi, info = map_align.gauss_newton_step(sums, damping)
    torch.cuda.synchronize()
    return xi, info


def sampled(fn, window=MB.WINDOW_S):
    """fn ends in a synchronise; -> calls per sample so that a sample covers `window` seconds."""
    fn()
    t0 = time.perf_counter()
    fn()
    return max(1, int(np.ceil(window / max(time.perf_counter() - t0, 1e-6))))


def measure(kind, pts, objects, mp, nets, a):
    dev = pts.device
    N = int(pts.shape[0])
    al = map_align.MapAlign(mp)
    g_min, tau = map_points.DEFAULT_G_MIN, map_align.DEFAULT_TAU
    r = {"cloud": kind, "points": N, "objects": mp.K, "hidden32_objects": mp.K - len(mp.wide)}
    # one iteration, pass by pass
    mp.surface(pts)
    runs = []
    for _ in range(a.reps):
        st = {}
        s = mp.surface(pts, stats=st)
        runs.append(st)
    for key, name in (("candidates_ms", "lists_ms"), ("grad32_ms", "grad_hidden32_ms"), ("grad_wide_ms", "grad_background_chain_ms"),
                      ("select_ms", "select_resolve_ms")):
        r[name] = round(float(np.median([x[key] for x in runs])), 3)
    r["pairs"], r["pairs32"], r["calls_per_iteration"] = runs[0]["pairs"], runs[0]["pairs32"], runs[0]["calls"]
    pivot = pts.double().mean(dim=0).cpu().numpy()
    r["transform_ms"] = round(MB.events(lambda: ops.mapalign_transform(pts, np.eye(4)), a.reps) * 1e3, 4)
    r["accumulate_ms"] = round(MB.events(lambda: ops.mapalign_accumulate(pts, s["obj"], s["alpha"], s["grad"], pivot, tau, g_min),
                                         a.reps) * 1e3, 4)
    r["inliers_first_iteration"] = int(ops.mapalign_accumulate(pts, s["obj"], s["alpha"], s["grad"], pivot, tau, g_min)[28].item())
    # the gradient kernel beside mp_eval_kernel on the same pairs
    seg_off, seg, pair_pt = ops.mappoints_candidates(pts, mp.boxes)
    M = seg[-1]
    pa, pg = torch.empty(M, device=dev), torch.empty(M, 3, device=dev)
    best = torch.zeros(N, dtype=torch.int64, device=dev)
    t_grad = MB.events(lambda: ops.mappoints_grad(mp.arena, pts, mp.boxes, mp.info, seg_off, pair_pt, pa, pg), a.reps)
    t_eval = MB.events(lambda: ops.mappoints_eval(mp.arena, pts, mp.boxes, mp.info, seg_off, pair_pt, pa, None, None, best), a.reps)
    r["mappoints_grad_pairs_per_s"] = round(r["pairs32"] / t_grad, 1)
    r["mp_eval_kernel_pairs_per_s"] = round(r["pairs32"] / t_eval, 1)
    r["grad_over_eval"] = round(t_eval / t_grad, 3)
    r["mfma_per_tile_grad_over_eval"] = [288, 184]
    del pa, pg, best, pair_pt
    # the 10-iteration fit and the baseline iteration, alternating

    def fit():
        res = al.fit(pts, iters=ITERS, tol=(0.0, 0.0))
        torch.cuda.synchronize()
        return res

    def base():
        return baseline_iteration(nets, mp, pts, np.eye(4), pivot, tau, g_min, 1e-6)

    r["fit_iterations_run"] = len(fit()["history"])
    n_fit, n_base = sampled(fit), sampled(base)
    ts = ([], [])
    for _ in range(a.reps):
        for i, (fn, n) in enumerate(((fit, n_fit), (base, n_base))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) / n)
    r["fit_10_iterations_s"] = round(float(np.median(ts[0])), 5)
    r["fit_10_iterations_s_min_max"] = [round(min(ts[0]), 5), round(max(ts[0]), 5)]
    r["baseline_one_iteration_s"] = round(float(np.median(ts[1])), 5)
    r["baseline_one_iteration_s_min_max"] = [round(min(ts[1]), 5), round(max(ts[1]), 5)]
    r["calls_per_sample"] = [n_fit, n_base]
    r["fit_per_iteration_s"] = round(r["fit_10_iterations_s"] / max(r["fit_iterations_run"], 1), 5)
    r["speedup_per_iteration"] = round(r["baseline_one_iteration_s"] / r["fit_per_iteration_s"], 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapalign_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = "cuda:0"
    objects = MB.make_map(dev)
    mp = map_points.MapPoints(objects, device=dev, bg_ids=(0,), pair_budget_bytes=8 << 30)
    nets = torch_nets(objects, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    clouds = [("surface", MB.make_cloud("surface", objects, a.points, dev, g)), ("frame", frame_cloud(dev))]
    res = {"device": torch.cuda.get_device_name(0),
           "cloud_size_note": "2 M points is an assumption about the order of a room mesh, not a measured figure",
           "defaults_note": "tau = 0.1 m and g_min = 1e-3 are assumed defaults",
           "clouds": [measure(kind, pts, objects, mp, nets, a) for kind, pts in clouds]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("tools/mapalign_bench.py -- see its docstring for the shape, the two clouds and what each figure is\n")
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
