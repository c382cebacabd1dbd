"""A whole novel view of a map at the native shape: map_view.MapView.render (one launch chain) against the per-object loop
render_view.render_view on the same map, ms per view and per stage.

    python tools/view_bench.py [--views 5] [--loop-only] [--objects 50] [--no-bg]

The scene is SYNTHETIC and stated here, not measured anywhere: 50 hidden-32 objects plus the hidden-128 background
(obj 0) seen by a 1200 x 680 camera with f = 600 at the origin, looking down +z.
  * background: a box of 9 x 6 x 5 m centred at (0, 0, 3): every pixel's ray enters it (816 000 candidate rays).
  * objects: a 10 x 5 grid in the image, column c at x / z = linspace(-0.85, 0.85, 10)[c], row r at
    y / z = linspace(-0.45, 0.45, 5)[r], depth z ~ U(1.5, 4.0) m, extent per axis ~ U(0.2, 0.8) m -- an ASSUMED
    distribution of object sizes (table-top to furniture), not one measured on a dataset -- turned about the y axis by
    U(-30, 30) degrees; RandomState(0).
Networks are freshly initialised (torch.manual_seed(obj_id)) with out_alpha.bias lowered by 1 as tools/render_bench.py
does.  Draws are seeded; both paths restart the process-wide draw counter per view, so they draw the same numbers and
the tool asserts that their images are equal bytes.

Times: a host clock around one view that ends in a device synchronise, after one warm-up view per path; median and
min .. max over --views views, the two paths alternating.  The stage split of MapView.render comes from a further view
with device events around every stage (MapView.render(stats=...), which synchronises per stage and is not part of the
timed views).  --loop-only runs on a tree without map_view (the baseline at the parent commit)."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from openobj_amd import cfg as ocfg, ops, render_view, trainer, vmap as ovmap      # noqa: E402

W, H, F = 1200, 680, 600.0


def rot_y(deg):
    t = np.deg2rad(deg)
    return np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])


def layout(n_objects):
    rs = np.random.RandomState(0)
    boxes = {0: types.SimpleNamespace(center=np.array([0.0, 0.0, 3.0]), R=np.eye(3), extent=np.array([9.0, 6.0, 5.0]))}
    xs, ys = np.linspace(-0.85, 0.85, 10), np.linspace(-0.45, 0.45, 5)
    for i in range(n_objects):
        z = rs.uniform(1.5, 4.0)
        ext = rs.uniform(0.2, 0.8, 3)
        deg = rs.uniform(-30, 30)
        boxes[i + 1] = types.SimpleNamespace(center=np.array([xs[i % 10] * z, ys[(i // 10) % 5] * z, z]), R=rot_y(deg), extent=ext)
    return boxes


class Obj:
    render_2D_syn = ovmap.sceneObject.render_2D_syn

    def __init__(self, dev, obj_id, bx):
        c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev)))
        c.obj_id, c.W, c.H = obj_id, W, H
        c.hidden_feature_size = 128 if obj_id == 0 else 32
        torch.manual_seed(obj_id)
        self.trainer = trainer.Trainer(c)
        with torch.no_grad():
            self.trainer.fc_occ_map.out_alpha.bias.add_(-1.0)
        self.training_device, self.box = dev, bx

    def get_bound(self, *a, **k):
        return None, self.box


def timed(fn):
    ops._draw_offset[0] = 0                   # both paths draw the same numbers in every view
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(name, ms):
    ms = sorted(ms)
    print(f"{name}: median {ms[len(ms) // 2]:.1f} ms  min {ms[0]:.1f}  max {ms[-1]:.1f}  ({len(ms)} views)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--objects", type=int, default=50)
    ap.add_argument("--no-bg", action="store_true", help="leave the hidden-128 background out")
    ap.add_argument("--loop-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("view_bench: no GPU")
    dev = torch.device("cuda:0")
    boxes = layout(a.objects)
    if a.no_bg:
        del boxes[0]
    vis = {k: Obj(dev, k, bx) for k, bx in boxes.items()}
    rays = ops.rays_dirs(W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, dev)
    T_WC = np.eye(4, dtype=np.float32)
    loop = lambda: render_view.render_view(vis, T_WC, rays, bg_ids=(0,))
    print(f"view {W}x{H}, {len(vis)} objects ({sum(int(o.trainer.hidden_feature_size) == 32 for o in vis.values())} hidden 32)")
    t_loop, t_new = [], []
    _, ref = timed(loop)                                                       # warm-up
    if not a.loop_only:
        from openobj_amd import map_view
        mv = map_view.MapView([map_view.MapObject(o.trainer, o.box, obj_id=k) for k, o in vis.items()], device=dev, bg_ids=(0,))
        new = lambda: mv.render(T_WC, rays)
        _, got = timed(new)                                                    # warm-up
        for k in ("rgb", "maskid", "depth"):
            assert np.array_equal(getattr(got, k), getattr(ref, k)), f"{k}: the batched view differs from the loop"
        print(f"images equal: {int((ref.maskid != 0).sum())} pixels painted, {mv.seg[-1]} candidate rays, "
              f"{mv.seg[-1] - sum(mv.seg[k + 1] - mv.seg[k] for k in mv.own_arena)} of them in the segmented launch")
    for _ in range(a.views):
        t_loop.append(timed(loop)[0])
        if not a.loop_only:
            t_new.append(timed(new)[0])
    spread("render_view (per-object loop)", t_loop)
    if not a.loop_only:
        spread("MapView.render (to_host=True)", t_new)
        stats = {}
        ops._draw_offset[0] = 0
        mv.render(T_WC, rays, stats=stats)
        print("MapView.render stages (device events, one view): " +
              "  ".join(f"{k} {v:.2f}" if k.endswith("_ms") else f"{k} {v}" for k, v in stats.items()))
    print(f"peak mem {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


if __name__ == "__main__":
    main()
