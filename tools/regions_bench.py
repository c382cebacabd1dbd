"""Part regions at the native map (openobj_amd/map_regions.py, objnerf_mapregions.hip) -> profiles/regions_bench.txt.

    python tools/regions_bench.py [--out profiles/regions_bench.txt] [--reps 5] [--objects 51]

Shape (ASSUMED sizes, as in tools/query_bench.py): 51 objects, each a 400 x 250 vertex sheet = 100 000 vertices and
198 702 faces in cell order (the order marching cubes emits), 5.1 M vertices and 10.1 M faces in all.  The planted query's
cosine is cos(2 pi x / 100) cos(2 pi y / 125) over the sheet: smooth bumps, so a threshold at the (1 - share) quantile
selects that share of the vertices as a few compact patches per object (1 %, 10 %) or as one patch with holes (90 %).

Timed with device events around windows of calls of about 0.3 s (after a warm-up call; median, min .. max over --reps
windows): the labelling (ops.regions_label: select, union, flatten, compaction, spread), the table passes
(ops.regions_table), and the whole MapQuery.part_regions call (cosines, thresholds, both of the above, the read-backs and
the host's 3 x 3 eigenproblems; wall clock).  Beside them, with outputs asserted EQUAL:
  torch   label propagation restated in torch on the device: every vertex takes the minimum label over its faces
          (scatter amin), then pointer jumping, until nothing changes; timed once per share after a warm-up run
  scipy   scipy.sparse.csgraph.connected_components on the host over the edges between selected vertices (wall clock,
          one run), where scipy is importable; otherwise the row is dropped and the file says so."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openobj_amd import ops, query  # noqa: E402
from openobj_amd.mesh import TriMesh  # noqa: E402

WINDOW_S = 0.3
SHEET_W, SHEET_H, CELL = 400, 250, 0.004
D = 8


def timed(fn, reps):
    """-> (median, min, max, calls per window) ms per call: device events around windows of about WINDOW_S."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    inner = max(1, int(np.ceil(WINDOW_S / max(time.perf_counter() - t0, 1e-6))))
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ts)), float(min(ts)), float(max(ts)), inner


def sheet_faces(w, h):
    y, x = np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing="ij")
    v = (y * w + x).reshape(-1)
    f = np.stack([np.stack([v, v + 1, v + w + 1], 1), np.stack([v, v + w + 1, v + w], 1)], 1)
    return f.reshape(-1, 3).astype(np.int64)


def native_map(n_obj, seed=0):
    """-> (all_obj dense with D-wide part features whose cosine with q is the planted pattern, q, the pattern [V])."""
    rs = np.random.RandomState(seed)
    i = np.arange(SHEET_W * SHEET_H)
    x, y = i % SHEET_W, i // SHEET_W
    faces = sheet_faces(SHEET_W, SHEET_H)
    q, b = np.eye(D)[0], np.eye(D)[1]
    out, cols = {}, []
    for p in range(n_obj):
        c = 0.98 * np.cos(2 * np.pi * (x + 7 * p) / 100.0) * np.cos(2 * np.pi * (y + 3 * p) / 125.0)
        z = 0.02 * np.sin(x / 17.0) * np.cos(y / 23.0)
        v = np.stack([x * CELL + 2.0 * (p % 8), y * CELL + 1.5 * (p // 8), z + 0.5], axis=1)
        m = TriMesh(v, faces)
        m.visual.vertex_colors = rs.randint(0, 256, (len(v), 4)).astype(np.uint8)
        pf = (c[:, None] * q[None] + np.sqrt(1 - c * c)[:, None] * b[None]).astype(np.float32)
        out[p] = {"clip_feat": None, "caption_feat": None, "class_id": p, "mesh": m, "color": m.visual.vertex_colors,
                  "part_feat": pf}
        cols.append(c)
    return out, q, np.concatenate(cols)


def torch_labels(faces, sel):
    """Minimum-label propagation over the faces whose ends are selected, with pointer jumping -> (root int32 [V], rounds)."""
    V = sel.numel()
    idx = torch.arange(V, device=sel.device, dtype=torch.int64)
    big = torch.full_like(idx, V)
    L = torch.where(sel, idx, big)
    f = faces.long()
    rounds = 0
    while True:
        rounds += 1
        before = L
        lf = L[f]                                                  # [F, 3]; V = not selected, so the minimum skips it
        m = lf.min(dim=1, keepdim=True).values.expand(-1, 3)
        L = L.scatter_reduce(0, f.reshape(-1), torch.where(lf < V, m, lf).reshape(-1), reduce="amin")
        for _ in range(3):                                         # pointer jumping: L[v] <- L[L[v]]
            L = torch.where(sel, L[L.clamp(max=V - 1)], big)
        if torch.equal(L, before):
            break
    return torch.where(sel, L, torch.full_like(L, -1)).to(torch.int32), rounds


def scipy_labels(faces, sel):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    V = len(sel)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [0, 2]]])
    e = e[sel[e[:, 0]] & sel[e[:, 1]]]
    g = coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(V, V)).tocsr()
    _, comp = connected_components(g, directed=False)
    first = np.full(comp.max() + 1, V, np.int64)
    np.minimum.at(first, comp, np.arange(V))
    return np.where(sel, first[comp], -1).astype(np.int32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--objects", type=int, default=51)
    ap.add_argument("--no-baselines", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    all_obj, q, col = native_map(a.objects)
    mq = query.MapQuery(all_obj, dev)
    verts, faces, face_off, _ = mq.mesh_buffers()
    V, F, S = mq.V, int(faces.shape[0]), mq.S
    vmax = int(np.diff(mq.seg_host).max())
    sims, _ = mq.part_similarity(torch.from_numpy(q.astype(np.float32))[None])
    sims_h = sims[:, 0].cpu().numpy()
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    lines = [f"part regions at the native map: {S} objects x {SHEET_W} x {SHEET_H} sheet = {V} vertices, {F} faces (assumed sizes)",
             f"{torch.cuda.get_device_name(0)}; device events, windows of ~{WINDOW_S} s, {a.reps} windows: median (min .. max) ms",
             "torch = label propagation restated in torch on the device, scipy = csgraph.connected_components on the host; "
             "outputs asserted equal" + ("" if have_scipy else "; scipy is not importable here: that row is dropped")]
    faces_h = faces.cpu().numpy() if have_scipy and not a.no_baselines else None
    for share in (0.01, 0.10, 0.90):
        cut = float(np.quantile(sims_h, 1.0 - share))
        thr = torch.full((S,), cut, device=dev)
        ws = torch.empty(ops.regions_workspace_bytes(V, F, S), dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lab = lambda: ops.regions_label(mq.seg_off, face_off, faces, sims, 0, thr, vmax=vmax, status=status, ws=ws)
        root, label, reg_off, _ = lab()
        R = int(reg_off[-1])
        tab = lambda: ops.regions_table(mq.seg_off, face_off, verts, faces, sims, 0, root, label, R, status)
        table = tab()
        assert int(status.item()) == 0
        n_sel = int((root >= 0).sum())
        t_lab, t_tab = timed(lab, a.reps), timed(tab, a.reps)
        assert torch.equal(tab(), table) and torch.equal(lab()[1], label)
        walls = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reg = mq.part_regions(q, min_cos=cut)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        walls = walls[1:]
        assert len(reg) == R and torch.equal(reg.label, label)
        lines.append(f"share {share:4.0%}: {n_sel} vertices selected, {R} regions, largest {int(table[:, 3].max())} faces")
        lines.append(f"  label        {t_lab[0]:8.3f} ({t_lab[1]:.3f} .. {t_lab[2]:.3f}) ms   [{t_lab[3]} calls a window]")
        lines.append(f"  table        {t_tab[0]:8.3f} ({t_tab[1]:.3f} .. {t_tab[2]:.3f}) ms   [{t_tab[3]} calls a window]")
        lines.append(f"  part_regions {np.median(walls):8.3f} ({min(walls):.3f} .. {max(walls):.3f}) ms wall, with the cosines, "
                     f"read-backs and {R} host eigenproblems")
        if a.no_baselines:
            continue
        sel = sims[:, 0] >= thr[0]
        torch_labels(faces, sel)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        troot, rounds = torch_labels(faces, sel)
        e1.record()
        e1.synchronize()
        t_torch = e0.elapsed_time(e1)
        assert torch.equal(troot, root), "torch label propagation disagrees"
        lines.append(f"  torch labels {t_torch:8.3f} ms ({rounds} rounds) = {t_torch / t_lab[0]:.1f} x label")
        if have_scipy:
            t0 = time.perf_counter()
            sroot = scipy_labels(faces_h, sims_h >= np.float32(cut))
            t_sc = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(sroot, root.cpu().numpy()), "scipy connected_components disagrees"
            lines.append(f"  scipy labels {t_sc:8.1f} ms wall on the host = {t_sc / t_lab[0]:.0f} x label "
                         f"(without moving {V * 4 + F * 12} bytes to the host)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
