"""Scoring a rendered view against a frame at the native shape: ops.view_compare (objnerf_view_compare, one launch)
against the same chain restated in torch on the same device, and against the MapView.render time of the view it scores.

    python tools/vieweval_bench.py [--objects 50] [--iters 500] [--windows 7] [--views 3]

The map is the SYNTHETIC one of tools/view_bench.py (its docstring states the layout: 50 hidden-32 objects in a 10 x 5
grid plus the hidden-128 background, 1200 x 680, f = 600): the mask-id image of its view holds up to 51 ids.  The frame it
is scored against is that view perturbed -- seeded noise of +-20 on the colour, 5 cm added to the depth, the ids
unchanged -- so every column of the tables is exercised.  Two further frames are reported SEPARATELY: one where a single
id covers the whole image on both sides (every pixel adds to one row and one confusion cell: the worst case for atomic
contention), scored with the 51-row tables (reduced in LDS first) and with a 70-row lut (above the LDS cap: wave-
aggregated global atomics).

Times: device events around `iters` back-to-back calls, after a warm-up window of the same calls; median and min .. max
over `windows` windows, per call; beside each the host's time to issue one call (a kernel this short can finish before
the next call is issued: then the two figures meet and the event time bounds the kernel's from above).  The torch restatement (int64 moments by shifted sums, the fp64 sequence, index_add_
for the tables) is timed the same way with fewer calls; its tables are asserted equal to the kernel's.  MapView.render:
a host clock around one view (to_host=False) that ends in a device synchronise, after one warm-up view."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import view_bench as VB                                                        # noqa: E402
from openobj_amd import map_view, map_view_eval as E, ops                      # noqa: E402

C1, C2 = 6.5025, 58.5225


def window_sums(a, taps):
    W, H = a.shape[0], a.shape[1]
    a1 = sum(t * a[:, k:H - 10 + k] for k, t in enumerate(taps))
    return sum(t * a1[k:W - 10 + k] for k, t in enumerate(taps))


def torch_compare(rgb_r, depth_r, id_r, painted, rgb_g, depth_g, id_g, lut, G):
    """The chain of include/objnerf_hip.h in torch on the tensors' device -> (acc [G + 1, 9], conf [G, G + 1])."""
    dev, (W, H) = rgb_r.device, rgb_r.shape[:2]
    x, y = rgb_r.long(), rgb_g.long()
    taps = list(E.TAPS)
    m = [window_sums(v, taps).double() * 2.0 ** -32 for v in (x, y, x * x, y * y, x * y)]
    mxmx, mymy, mxmy = m[0] * m[0], m[1] * m[1], m[0] * m[1]
    vx, vy, cv = m[2] - mxmx, m[3] - mymy, m[4] - mxmy
    s = (((2.0 * mxmy) + C1) * ((2.0 * cv) + C2)) / (((mxmx + mymy) + C1) * ((vx + vy) + C2))
    q = torch.zeros(W, H, dtype=torch.int64, device=dev)
    q[5:W - 5, 5:H - 5] = torch.floor((((s[..., 0] + s[..., 1]) + s[..., 2]) / 3.0) * 4294967296.0).long()
    interior = torch.zeros(W, H, dtype=torch.int64, device=dev)
    interior[5:W - 5, 5:H - 5] = 1
    d = x - y
    se, pt = (d * d).sum(-1), painted.long()
    f4 = depth_g > 0
    f5 = f4 & (depth_r < 100)
    dq = torch.floor((depth_r - depth_g).abs().clamp(max=4194304.0).double() * 1048576.0).long() * f5.long()

    def rows(ids):
        ids = ids.long()
        r = lut.long()[ids.clamp(0, lut.shape[0] - 1)]
        return torch.where((ids >= 0) & (ids < lut.shape[0]) & (r >= 0) & (r < G), r, torch.full_like(r, G))

    rg, rp = rows(id_g).reshape(-1), rows(id_r).reshape(-1)
    cols = torch.stack([torch.ones_like(se), pt, se, se * pt, f4.long(), f5.long(), dq, interior, q], -1).reshape(-1, 9)
    acc = torch.zeros(G + 1, 9, dtype=torch.int64, device=dev).index_add_(0, rg, cols)
    keep = rg < G
    conf = torch.bincount(rg[keep] * (G + 1) + rp[keep], minlength=G * (G + 1)).reshape(G, G + 1)
    return acc, conf


def event_ms(fn, iters, windows, tables=()):
    """tables: zeroed before every window, outside the events (the calls add; a long run would wrap the int64 sums)."""
    for _ in range(iters):                                                     # warm-up window
        fn()
    torch.cuda.synchronize()
    ms, host = [], []
    for _ in range(windows):
        for t in tables:
            t.zero_()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        h0 = time.perf_counter()
        for _ in range(iters):
            fn()
        host.append((time.perf_counter() - h0) * 1e3 / iters)                  # issuing the calls, before any wait
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / iters)
    return sorted(ms), sorted(host)[len(host) // 2]


def line(name, timed):
    """The device-event time per call; beside it what the host took to ISSUE a call: where the two are equal the calls
    were issued no faster than they ran and the figure is an upper bound of the kernel's time."""
    ms, host = timed
    print(f"{name}: median {ms[len(ms) // 2]:.3f} ms  min {ms[0]:.3f}  max {ms[-1]:.3f}  ({len(ms)} windows; "
          f"host issue {host:.3f} ms per call)")
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=50)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--views", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vieweval_bench: no GPU")
    dev = torch.device("cuda:0")
    W, H = VB.W, VB.H
    vis = {k: VB.Obj(dev, k, bx) for k, bx in VB.layout(a.objects).items()}
    rays = ops.rays_dirs(W, H, VB.F, VB.F, W / 2 - 0.5, H / 2 - 0.5, dev)
    T_WC = np.eye(4, dtype=np.float32)
    # the mask-id image holds obj_id + 1, so that the background (obj 0) is told from "nothing painted"
    mv = map_view.MapView([map_view.MapObject(o.trainer, o.box, obj_id=k) for k, o in vis.items()], device=dev, bg_ids=(0,),
                          class_of={k: k + 1 for k in vis})
    render = lambda: mv.render(T_WC, rays, to_host=False)
    t_render = []
    for i in range(a.views + 1):
        ms, view = VB.timed(render)
        if i:
            t_render.append(ms)
    ev = E.ViewEval.from_map(mv)
    G, lut = ev.G, ev.lut
    rgb, depth, mid = view["rgb"], view["depth"], view["maskid"]
    painted = view["winner"] >= 0
    g = torch.Generator().manual_seed(0)
    noise = torch.randint(-20, 21, (W, H, 3), generator=g, dtype=torch.int32).to(dev)
    rgb_g = (rgb.int() + noise).clamp(0, 255).to(torch.uint8)
    depth_g = (depth + 0.05).contiguous()
    print(f"view {W}x{H}, {len(vis)} objects, G = {G} ids, {int(painted.sum())} pixels painted, "
          f"{int(torch.unique(mid).numel())} distinct mask ids in the view")

    def tables(n):
        return (torch.zeros(n + 1, 9, dtype=torch.int64, device=dev), torch.zeros(n, n + 1, dtype=torch.int64, device=dev))

    def kernel(id_r, id_g, lut_, n, acc, conf, ssim_map=False):
        return lambda: ops.view_compare(rgb, depth, id_r, painted, rgb_g, depth_g, id_g, lut_, n, acc, conf,
                                        want_ssim_map=ssim_map)

    # equal tables first
    acc, conf = tables(G)
    kernel(mid, mid, lut, G, acc, conf)()
    acc_t, conf_t = torch_compare(rgb, depth, mid, painted, rgb_g, depth_g, mid, lut, G)
    assert torch.equal(acc, acc_t) and torch.equal(conf, conf_t), "the kernel's tables differ from the torch restatement"
    f = E.figures(acc.sum(0).cpu().numpy())
    print(f"tables equal to the torch restatement; the frame: PSNR {f['psnr']:.2f} dB, SSIM {f['ssim']:.4f}, "
          f"depth L1 {f['depth_l1']:.4f} m")
    spread = lambda ms: f"median {ms[len(ms) // 2]:.1f} ms  min {ms[0]:.1f}  max {ms[-1]:.1f}"
    t_render.sort()
    print(f"MapView.render (to_host=False): {spread(t_render)}  ({len(t_render)} views)")
    k_all = line(f"view_compare, {G} ids, acc + conf", event_ms(kernel(mid, mid, lut, G, acc, conf), a.iters, a.windows, (acc, conf)))
    line(f"view_compare, {G} ids, acc + conf + ssim_map", event_ms(kernel(mid, mid, lut, G, acc, conf, True), a.iters, a.windows, (acc, conf)))
    line(f"view_compare, {G} ids, acc only", event_ms(kernel(mid, mid, lut, G, acc, None), a.iters, a.windows, (acc,)))
    t_all = line("torch restatement (int64 / fp64), same frame",
                 event_ms(lambda: torch_compare(rgb, depth, mid, painted, rgb_g, depth_g, mid, lut, G), max(1, a.iters // 10), a.windows))
    print(f"the torch restatement takes {t_all / k_all:.0f} x view_compare; view_compare is "
          f"{100 * k_all / t_render[len(t_render) // 2]:.3f} % of rendering the view")
    # the single-id frame, reported separately
    one = torch.full((W, H), int(ev.ids[1]), dtype=torch.int32, device=dev)
    acc1, conf1 = tables(G)
    kernel(one, one, lut, G, acc1, conf1)()
    assert int(acc1[1, 0]) == W * H == int(conf1[1, 1])
    row_one = acc1[1].clone()                                                   # (the timed calls below go on adding)
    k_one = line(f"single-id frame, {G} ids (LDS tables)", event_ms(kernel(one, one, lut, G, acc1, conf1), a.iters, a.windows, (acc1, conf1)))
    big = ops.VIEW_EVAL_LDS_ROWS + 6
    lut_big = torch.arange(big, dtype=torch.int32, device=dev)
    acc2, conf2 = tables(big)
    kernel(one, one, lut_big, big, acc2, conf2)()
    r = int(ev.ids[1])
    assert int(acc2[r, 0]) == W * H == int(conf2[r, r]) and torch.equal(acc2[r], row_one)
    k_big = line(f"single-id frame, {big} ids (global atomics)", event_ms(kernel(one, one, lut_big, big, acc2, conf2), a.iters, a.windows, (acc2, conf2)))
    accm, confm = tables(big)
    line(f"the view's ids, {big} ids (global atomics)", event_ms(kernel(mid, mid, lut_big, big, accm, confm), a.iters, a.windows, (accm, confm)))
    print(f"single-id frame against the view's own ids: {k_one / k_all:.2f} x (LDS tables), {k_big / k_all:.2f} x (global atomics)")


if __name__ == "__main__":
    main()
