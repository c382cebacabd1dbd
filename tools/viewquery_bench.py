"""Part features and open-vocabulary queries of a map view at the native shape: MapView.render(want_feat=True), .query and
.features (objnerf_view_query) against the old route to the same numbers -- the per-object loop
sceneObject.render_2D_syn(render_part=True), the fold of train.py:581-598 carrying a 512-d row per pixel on the host, and
F.cosine_similarity over the painted pixels.

    python tools/viewquery_bench.py [--views 5] [--reps 20] [--objects 50] [--no-bg] [--existing-only]

The scene is the SYNTHETIC one tools/view_bench.py states (1200 x 680, 50 hidden-32 objects on a grid with ASSUMED box
sizes, the hidden-128 background); the queries are 16 random unit vectors (RandomState(1)).

The tool first ASSERTS that both routes agree: the same painters (rgb, maskid, depth equal as bytes), every feature
element of a sample of painted pixels within 2 x 64 x 2^-24 (|of_w| . |h| + |of_b| opacity) (both sides are fp32 heads on
the same hidden rows), every cosine within 2 x 1e-5 max(1, A / |F|), the label image exactly the first arg-max of the
returned cosines -- then times.

Times: a host clock around a call that ends in a device synchronise, after a warm-up call; median and min .. max.
--existing-only times nothing but MapView.render without want_feat (one figure per process: the median of --views views
after a warm-up view) and runs on the parent commit's tree as well: the gate on the existing path alternates five
processes of each tree."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from view_bench import F, H, W, Obj, layout, timed      # noqa: E402  (also puts the repository root on sys.path)
from openobj_amd import _lib, map_view, ops, render_view      # noqa: E402

U24 = 2.0 ** -24


def stat(name, ms, unit="ms"):
    ms = sorted(ms)
    print(f"{name}: median {ms[len(ms) // 2]:.2f} {unit}  min {ms[0]:.2f}  max {ms[-1]:.2f}  ({len(ms)} runs)")
    return ms[len(ms) // 2]


def clock(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def old_route(vis, T_WC, rays, q_dev):
    """The loop with render_part=True, the fold carrying features, the cosines of the painted pixels.
    -> (ViewBuffers, feature image [W, H, 512] on the host, cosines [Q, n_painted] on the device, seconds per part)."""
    t0 = time.perf_counter()
    buf = render_view.ViewBuffers(W, H)
    img = np.zeros((W, H, 512), np.float32)
    for oid, o in vis.items():
        mask, depth, colour, feat = (o.render_2D_syn(T_WC, None, rays, chunk_size=3000, do_fine=False, render_part=True) + (None,))[:4]
        if depth is None:
            continue
        ok = buf.merge(mask, depth, colour, oid, oid == 0)
        img[ok] = feat[ok[mask]]                      # (ok lies inside mask: only a depth below 100 paints)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    rows = torch.from_numpy(img[buf.maskid != 0]).to(q_dev.device)
    cos = torch.stack([torch.nn.functional.cosine_similarity(rows, q[None], dim=1, eps=1e-8) for q in q_dev])
    torch.cuda.synchronize()
    return buf, img, cos, (t1 - t0, time.perf_counter() - t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--objects", type=int, default=50)
    ap.add_argument("--no-bg", action="store_true")
    ap.add_argument("--existing-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("viewquery_bench: no GPU")
    dev = torch.device("cuda:0")
    boxes = layout(a.objects)
    if a.no_bg:
        del boxes[0]
    vis = {k: Obj(dev, k, bx) for k, bx in boxes.items()}
    rays = ops.rays_dirs(W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, dev)
    T_WC = np.eye(4, dtype=np.float32)
    mv = map_view.MapView([map_view.MapObject(o.trainer, o.box, obj_id=k) for k, o in vis.items()], device=dev, bg_ids=(0,))
    plain = lambda: mv.render(T_WC, rays)
    timed(plain)                                                               # warm-up
    if a.existing_only:
        ms = sorted(timed(plain)[0] for _ in range(a.views))
        print(f"existing path: MapView.render median {ms[len(ms) // 2]:.1f} ms  min {ms[0]:.1f}  max {ms[-1]:.1f}")
        return
    print(f"view {W}x{H}, {len(vis)} objects; workgroups of the segmented renderer per compute unit as the runtime places "
          f"them: {_lib.lib().objnerf_render_fwd_segmented_occupancy(0)} without, "
          f"{_lib.lib().objnerf_render_fwd_segmented_occupancy(1)} with the feature hidden")
    q = np.random.RandomState(1).standard_normal((16, 512)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q_dev = torch.from_numpy(q).to(dev)
    # ------------------------------------------------------------------------------------------------- agreement
    feat_view = lambda: mv.render(T_WC, rays, want_feat=True)
    _, got = timed(feat_view)
    ops._draw_offset[0] = 0
    buf, img, cos_old, _ = old_route(vis, T_WC, rays, q_dev)                    # (also the old route's warm-up)
    for k in ("rgb", "maskid", "depth"):
        assert np.array_equal(getattr(got, k), getattr(buf, k)), f"{k}: the views differ"
    painted = torch.from_numpy((buf.maskid != 0).reshape(-1)).to(dev)
    pp = painted.nonzero(as_tuple=True)[0]
    o = mv.query(q_dev)
    sims = o["sims"].reshape(16, -1)
    nan = torch.isnan(sims)
    first = torch.where(nan.all(0), torch.full_like(o["label"].reshape(-1), -1),
                        torch.where(nan, torch.full_like(sims, float("inf")), sims).argmax(0).to(torch.int32))
    assert torch.equal(o["label"].reshape(-1), first), "label is not the first arg-max of the returned cosines"
    assert torch.equal(~nan.any(0), painted)
    # A = |of_w| . |h| + |of_b| opacity of a sample of painted pixels, from the view's own hidden rows, in fp64
    sample = pp[torch.from_numpy(np.random.RandomState(2).choice(pp.numel(), min(20000, pp.numel()), replace=False)).to(dev)]
    e = mv.winner.reshape(-1)[sample].long()
    obj = torch.searchsorted(mv.seg_off, e, right=True) - 1
    A = torch.zeros(sample.numel(), 512, dtype=torch.float64, device=dev)
    for k, (of_w, of_b, hf, row0) in enumerate(mv._view_heads()):
        m = obj == k
        if hf is None or not bool(m.any()):
            continue
        h, op = hf[e[m] - row0].double().abs(), mv.csr["opacity"][e[m]].double()
        A[m] = h @ of_w.double().abs().T + op[:, None] * of_b.double().abs()[None]
    new_rows = mv.features(sample).double()
    old_rows = torch.from_numpy(img.reshape(-1, 512)[sample.cpu().numpy()]).to(dev).double()
    ef = ((new_rows - old_rows).abs() / (2 * 64 * U24 * A)).max().item()
    assert ef <= 1.0, f"a feature element is {ef:.2f} x its bound off the old route"
    cond = torch.clamp(A.norm(dim=1) / old_rows.norm(dim=1), min=1.0)
    pos = torch.searchsorted(pp, sample)
    ec = ((sims[:, sample].double() - cos_old[:, pos].double()).abs() / (2e-5 * cond[None])).max().item()
    assert ec <= 1.0, f"a cosine is {ec:.2f} x its bound off the old route"
    agree = float((o["label"].reshape(-1)[pp] == cos_old.argmax(0).to(torch.int32)).float().mean())
    print(f"both routes agree: {pp.numel()} painted pixels, {mv.seg[-1]} candidate rays; on {sample.numel()} sampled pixels the "
          f"worst feature element is {ef:.3f} of its bound, the worst cosine {ec:.3f} of its bound (A / |F| up to "
          f"{cond.max().item():.1f}); the label images agree on {100 * agree:.3f} % of the painted pixels")
    del img, old_rows, new_rows, A
    # ---------------------------------------------------------------------------------------------------- times
    t_plain, t_feat = [], []
    for _ in range(a.views):
        t_plain.append(timed(plain)[0])
        t_feat.append(timed(feat_view)[0])
    stat("MapView.render", t_plain)
    stat("MapView.render(want_feat=True)", t_feat)
    stats = {}
    ops._draw_offset[0] = 0
    mv.render(T_WC, rays, stats=stats, want_feat=True)
    print("  stages with want_feat (device events, one view): " +
          "  ".join(f"{k} {v:.2f}" if k.endswith("_ms") else f"{k} {v}" for k, v in stats.items()))
    for Q in (1, 16):
        stat(f"MapView.query, Q = {Q} (cosines, label, best)", clock(lambda: mv.query(q_dev[:Q]), a.reps))
        stat(f"MapView.query, Q = {Q}, want_sims=False", clock(lambda: mv.query(q_dev[:Q], want_sims=False), a.reps))
    for n in (1000, 100000, pp.numel()):
        px = pp[:n].contiguous()
        stat(f"MapView.features, {px.numel()} painted pixels", clock(lambda: mv.features(px), a.reps))
    old = []
    for _ in range(2):
        ops._draw_offset[0] = 0
        old.append(old_route(vis, T_WC, rays, q_dev)[3])
    print("old route (render_2D_syn(render_part=True) per object + host fold with features | cosine_similarity, 16 "
          "queries, painted pixels), s per view: " + "  ".join(f"{x:.2f} | {y:.3f}" for x, y in old))
    print(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


if __name__ == "__main__":
    main()
