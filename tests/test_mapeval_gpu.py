"""GPU: objnerf_mapeval.hip against the numpy restatements of tests/mapeval_util.py (checked on their own, on the CPU, by
tests/test_mapeval.py) -- the mesh sampler and the exact nearest-point search bit for bit, the segment statistics to
1e-12 -- and openobj_amd/map_eval.py end to end.  Outputs are written into buffers with guard rows on both sides."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import mapeval_util as U
from conftest import T
from openobj_amd import _lib, map_eval, mesh, ops

pytestmark = pytest.mark.gpu

GUARD = 8


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def guarded(shape, dtype, dev, fill):
    buf = torch.full((shape[0] + 2 * GUARD,) + tuple(shape[1:]), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + shape[0]]


def guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def gpu_nearest(dev, qry, q_off, ref, r_off, cell, **kw):
    qry, ref = np.asarray(qry, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    plan = ops.NearestPlan(T(ref).to(dev), r_off, cell)
    bd, d2 = guarded((len(qry),), torch.float64, dev, -7.0)
    bi, idx = guarded((len(qry),), torch.int64, dev, -77)
    plan.query(T(qry).to(dev), q_off, out=(d2, idx), **kw)
    assert guards_intact(bd, -7.0) and guards_intact(bi, -77)
    return d2.cpu().numpy(), idx.cpu().numpy()


def check_nearest(dev, qry, q_off, ref, r_off, cell, **kw):
    d2, idx = gpu_nearest(dev, qry, q_off, ref, r_off, cell, **kw)
    rd2, ridx = U.nearest_ref(qry, q_off, ref, r_off)
    assert np.array_equal(bits(d2), bits(rd2))
    assert np.array_equal(idx, ridx)
    return d2, idx


# ------------------------------------------------------------------------------------------------------------ nearest
def test_nearest_one_point(dev):
    d2, idx = check_nearest(dev, [[0.5, 0.25, -1.0]], [0, 1], [[0.0, 0.25, 1.0]], [0, 1], 0.1)
    assert d2[0] == 4.25 and idx[0] == 0


def test_nearest_segments_empty_reference_and_no_queries(dev):
    rng = np.random.default_rng(0)
    nr0, nq0 = 3 * 256 + 5, 2 * 256 + 7
    ref = rng.uniform(-1, 1, (nr0 + 40, 3))
    qry = rng.uniform(-1.2, 1.2, (nq0 + 30, 3))
    r_off, q_off = [0, nr0, nr0, nr0 + 40], [0, nq0, nq0 + 30, nq0 + 30]
    d2, idx = check_nearest(dev, qry, q_off, ref, r_off, 0.2)
    assert np.all(np.isinf(d2[nq0:])) and np.all(idx[nq0:] == -1)
    assert np.all(idx[:nq0] < nr0)


def test_nearest_lattice_ties_and_exact_ring_distances(dev):
    """Points at multiples of 0.25 with cell = 0.25: they sit on cell faces, ties abound, and a query on a lattice point
    the reference lacks is exactly 1 or 2 cells from its answers."""
    g = np.arange(8) * 0.25
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    i = np.rint(lat / 0.25).astype(int)
    ref = lat[(i[:, 0] + 2 * i[:, 1] + 3 * i[:, 2]) % 7 < 2]
    half = lat[: 200] + 0.125
    out = ref[ref[:, 0] == 0.0] - [0.5, 0.0, 0.0]             # outside the grid, exactly 2 cells from their answer
    qry = np.concatenate([lat, half, out])
    d2, idx = check_nearest(dev, qry, [0, len(qry)], ref, [0, len(ref)], 0.25)
    d = np.sqrt(d2)
    assert np.any(d == 0.25) and np.any(d == 0.0) and np.any(d == 0.5)
    assert not U.unique_minimum(qry, [0, len(qry)], ref, [0, len(ref)], d2).all()


def test_nearest_is_the_same_for_every_cell_side(dev):
    rng = np.random.default_rng(1)
    ref = rng.uniform(0, 1, (800, 3))
    qry = rng.uniform(-0.4, 1.4, (811, 3))
    # 0.01: nearly every point in a cell of its own and queries up to 40 cells from any reference point: tier 1 gives
    # up and brute force finishes; 0.15: a few points a cell; 10: one cell holds everything
    a = check_nearest(dev, qry, [0, 811], ref, [0, 800], 0.01)
    b = gpu_nearest(dev, qry, [0, 811], ref, [0, 800], 0.15)
    c = gpu_nearest(dev, qry, [0, 811], ref, [0, 800], 10.0)
    for o in (b, c):
        assert np.array_equal(bits(a[0]), bits(o[0])) and np.array_equal(a[1], o[1])
    for rings in (1, 5):                                       # where tier 1 hands over does not matter either
        o = gpu_nearest(dev, qry, [0, 811], ref, [0, 800], 0.15, max_rings=rings)
        assert np.array_equal(bits(a[0]), bits(o[0])) and np.array_equal(a[1], o[1])


def test_nearest_queries_outside_the_reference_box(dev):
    rng = np.random.default_rng(2)
    ref = rng.uniform(0, 1, (300, 3)) * [1.0, 0.5, 0.25] + [2.0, -1.0, 0.0]
    lo, hi = ref.min(0), ref.max(0)
    ext = hi - lo
    q = [lo - 0.01, hi + 0.01, lo - 1e-9, lo - 1e3 * ext, hi + 1e3 * ext]
    for c in range(3):
        for sgn in (-1, 1):
            p = 0.5 * (lo + hi)
            p[c] += sgn * (0.5 + 0.3) * ext[c]
            q.append(p.copy())
            p[c] += sgn * 1e3 * ext[c]
            q.append(p)
    q = np.array(q)
    for cell in (0.05, 0.3):
        check_nearest(dev, q, [0, len(q)], ref, [0, 300], cell)


def test_nearest_coincident_and_duplicated_points(dev):
    rng = np.random.default_rng(3)
    ref = rng.uniform(0, 1, (500, 3))
    ref[400] = ref[17]                                          # a duplicate: the lower row wins
    ref[77] = ref[431]
    d2, idx = check_nearest(dev, ref, [0, 500], ref, [0, 500], 0.1)
    assert np.all(d2 == 0.0)
    assert idx[400] == 17 and idx[17] == 17 and idx[431] == 77 and idx[77] == 77
    assert np.array_equal(np.delete(idx, [400, 431]), np.delete(np.arange(500), [400, 431]))


def test_nearest_two_calls_write_the_same_bytes(dev):
    rng = np.random.default_rng(4)
    ref, qry = rng.normal(size=(2000, 3)), rng.normal(size=(1500, 3))
    a = gpu_nearest(dev, qry, [0, 700, 1500], ref, [0, 1200, 2000], 0.07)
    b = gpu_nearest(dev, qry, [0, 700, 1500], ref, [0, 1200, 2000], 0.07)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_nearest_rejects_bad_input(dev):
    ref = T(np.random.default_rng(5).uniform(0, 1, (50, 3))).to(dev)
    q = ref.clone()
    q[7, 1] = float("nan")
    plan = ops.NearestPlan(ref, [0, 50], 0.1)
    with pytest.raises(_lib.ObjnerfError):
        plan.query(q, [0, 50])
    with pytest.raises(_lib.ObjnerfError):                      # the reference spans 10^7 > 2^21 cells
        ops.NearestPlan(T(np.array([[0.0, 0, 0], [1.0, 0, 0]])).to(dev), [0, 2], 1e-7)
    with pytest.raises(_lib.ObjnerfError):
        plan.query(ref, [0, 20, 50])                            # another number of segments
    with pytest.raises(_lib.ObjnerfError):
        ops.NearestPlan(ref, [0, 50], 0.0)


def test_nearest_medium_against_kdtree(dev):
    """20 000 x 20 000 in 4 uneven segments, the automatic cell side: many workgroups; against scipy's k-d tree."""
    rng = np.random.default_rng(6)
    r_off, q_off = [0, 9000, 9100, 15000, 20000], [0, 3000, 11000, 11050, 20000]
    ref = rng.normal(size=(20000, 3)) * [1.0, 0.6, 0.3]
    qry = rng.normal(size=(20000, 3)) * [1.1, 0.6, 0.3]
    for s in range(4):
        ref[r_off[s]:r_off[s + 1]] += [3.0 * s, 0, 0]
        qry[q_off[s]:q_off[s + 1]] += [3.0 * s, 0, 0]
    d2, idx = gpu_nearest(dev, qry, q_off, ref, r_off, None)
    for s in range(4):
        R, Q = ref[r_off[s]:r_off[s + 1]], qry[q_off[s]:q_off[s + 1]]
        dt, it = cKDTree(R).query(Q, k=2)
        d = np.sqrt(d2[q_off[s]:q_off[s + 1]])
        assert np.all(np.abs(d - dt[:, 0]) <= 1e-12 * dt[:, 0])
        uniq = dt[:, 1] > dt[:, 0] * (1 + 1e-9)
        assert uniq.mean() > 0.99
        assert np.array_equal(idx[q_off[s]:q_off[s + 1]][uniq], it[uniq, 0] + r_off[s])


# ------------------------------------------------------------------------------------------------------------ sampler
def gpu_sample(dev, verts, faces, face_off, samp_off, seed):
    N = int(samp_off[-1])
    bp, pts = guarded((N, 3), torch.float64, dev, -7.0)
    bt, tri = guarded((N,), torch.int32, dev, -77)
    ops.mesh_sample(T(np.asarray(verts, np.float64)).to(dev), T(np.asarray(faces, np.int32)).to(dev), face_off, samp_off, seed,
                    out=(pts, tri))
    assert guards_intact(bp, -7.0) and guards_intact(bt, -77)
    return pts.cpu().numpy(), tri.cpu().numpy()


def check_sample(dev, verts, faces, face_off, samp_off, seed):
    pts, tri = gpu_sample(dev, verts, faces, face_off, samp_off, seed)
    rp, rt = U.mesh_sample_ref(verts, faces, face_off, samp_off, seed)
    assert np.array_equal(tri, rt)
    assert np.array_equal(bits(pts), bits(rp))
    return pts, tri


def test_sampler_one_triangle_one_draw(dev):
    pts, tri = check_sample(dev, [[0, 0, 0], [1, 0, 0.5], [0, 2, 0]], [[0, 1, 2]], [0, 1], [0, 1], seed=1)
    assert tri[0] == 0


def test_sampler_segments_zero_area_repeated_face_and_no_samples(dev):
    rng = np.random.default_rng(7)
    verts = rng.normal(size=(30, 3))
    faces = rng.integers(0, 30, (40, 3))
    faces[3] = [5, 5, 9]                                        # zero area
    faces[12] = faces[11]                                       # a repeated face
    face_off, samp_off = [0, 15, 25, 40], [0, 1000, 1000, 2000]
    pts, tri = check_sample(dev, verts, faces, face_off, samp_off, seed=(7 << 32) | 9)
    assert not np.any(tri == 3) and np.any(tri == 11) and np.any(tri == 12)
    assert np.all(tri[:1000] < 15) and np.all(tri[1000:] >= 25)


def test_sampler_segment_across_scan_tiles(dev):
    rng = np.random.default_rng(8)
    F = 2 * 1024 * 4 + 3                                        # more than two tiles of the workgroup scan
    verts = rng.uniform(0, 1, (500, 3))
    faces = rng.integers(0, 500, (F + 10, 3))
    pts, tri = check_sample(dev, verts, faces, [0, 10, F + 10], [0, 50, 3050], seed=2)
    assert tri[50:].max() > 2 * 1024 * 4 and tri[50:].min() < 10 + 1024


def test_sampler_seed_and_prefix_property(dev):
    v, f = U_QUAD
    a = gpu_sample(dev, v, f, [0, 4], [0, 1000], seed=3)
    b = gpu_sample(dev, v, f, [0, 4], [0, 100], seed=3)
    assert np.array_equal(bits(a[0][:100]), bits(b[0])) and np.array_equal(a[1][:100], b[1])
    c = gpu_sample(dev, v, f, [0, 4], [0, 100], seed=4)
    assert not np.array_equal(b[1], c[1]) and not np.array_equal(bits(b[0]), bits(c[0]))
    assert not np.any(a[1] == 3)                                # the zero-area face


def test_sampler_rejects_bad_input(dev):
    v, f = U_QUAD
    with pytest.raises(_lib.ObjnerfError, match="no area"):
        gpu_sample(dev, v, [[0, 6, 6], [1, 1, 1]], [0, 2], [0, 5], seed=0)
    bad = np.array(f)
    bad[1, 2] = 7                                               # V = 7
    with pytest.raises(_lib.ObjnerfError, match="outside"):
        gpu_sample(dev, v, bad, [0, 4], [0, 5], seed=0)
    bad[1, 2] = -1
    with pytest.raises(_lib.ObjnerfError, match="outside"):
        gpu_sample(dev, v, bad, [0, 4], [0, 5], seed=0)


U_QUAD = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [3, 0, 0], [3, 2, 0], [1, 2, 0]], np.float64),
          np.array([[0, 1, 2], [1, 3, 2], [1, 4, 5], [0, 6, 6]], np.int64))


# -------------------------------------------------------------------------------------------------------------- stats
def test_seg_stats(dev):
    rng = np.random.default_rng(9)
    d = np.abs(rng.normal(size=3000)) * 0.05
    d[[5, 700, 2999]] = [np.inf, np.nan, np.inf]
    off, thr = [0, 1300, 1300, 3000], (0.05, 0.01, 0.2)
    outs = []
    for _ in range(2):
        buf, out = guarded((3, 8), torch.float64, dev, -7.0)
        ops.seg_stats(T(d).to(dev), off, thr, out=out)
        assert guards_intact(buf, -7.0)
        outs.append(out.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    for s in range(3):
        seg = d[off[s]:off[s + 1]]
        fin = seg[np.isfinite(seg)]
        row = outs[0][s]
        assert row[0] == fin.size and row[1] == seg.size - fin.size
        assert row[2] == pytest.approx(fin.sum(), rel=1e-12) and row[3] == pytest.approx((fin * fin).sum(), rel=1e-12)
        assert row[4] == (fin.max() if fin.size else -np.inf)
        assert [row[5 + t] for t in range(3)] == [np.count_nonzero(fin < x) for x in thr]
    with pytest.raises(_lib.ObjnerfError):
        ops.seg_stats(T(d).to(dev), off, (1, 2, 3, 4, 5))


# --------------------------------------------------------------------------------------------------------- end to end
H = 0.05
SQ_F = np.array([[0, 1, 2], [1, 3, 2]], np.int64)


def square(z):
    return np.array([[0, 0, z], [1, 0, z], [0, 1, z], [1, 1, z]], np.float64), SQ_F


def test_compare_two_squares_equals_the_restated_pipeline(dev):
    n, thr = 2000, (0.04, 0.1)
    res = map_eval.compare({3: square(0.0)}, {3: mesh.TriMesh(*square(H))}, n_samples=n, thresholds=thr, seed=5,
                           n_scene_samples=n, device=dev, return_samples=True)
    # the restated pipeline: vertices of pred then gt; segments pred object, gt object, pred scene, gt scene
    verts = np.concatenate([square(0.0)[0], square(H)[0]])
    faces = np.concatenate([SQ_F, SQ_F + 4, SQ_F, SQ_F + 4])
    samp_off = [0, n, 2 * n, 3 * n, 4 * n]
    rp, rt = U.mesh_sample_ref(verts, faces, [0, 2, 4, 6, 8], samp_off, 5)
    s = res["samples"]
    assert s["samp_off"] == samp_off
    assert np.array_equal(bits(s["pts"].cpu().numpy()), bits(rp)) and np.array_equal(s["tri"].cpu().numpy(), rt)
    for name, (p0, g0) in {"object": (0, n), "scene": (2 * n, 3 * n)}.items():
        P, G = rp[p0:p0 + n], rp[g0:g0 + n]
        acc = np.sqrt(U.nearest_ref(P, [0, n], G, [0, n])[0])
        comp = np.sqrt(U.nearest_ref(G, [0, n], P, [0, n])[0])
        ref = U.metrics_ref(acc, comp, thr)
        got = res["objects"][3] if name == "object" else res["scene"]
        for k, v in ref.items():
            assert got[k] == pytest.approx(v, rel=1e-12, abs=0), (name, k)
        assert got["accuracy"] >= H and got["completion"] >= H
        assert got["completion_ratio@0.04"] == 0.0
        # a miss needs an in-plane gap above sqrt(0.1^2 - 0.05^2) = 0.087 among 2000 uniform samples
        assert got["completion_ratio@0.1"] > 0.9 and got["completion_ratio@0.1"] == ref["completion_ratio@0.1"]
        assert got["chamfer"] == pytest.approx(0.5 * (got["accuracy"] + got["completion"]), rel=1e-15)
        assert (got["n_pred"], got["n_gt"], got["n_nonfinite"]) == (n, n, 0)
    assert res["missing_pred"] == [] and res["missing_gt"] == []


def test_command_line_on_two_map_vis_directories(dev, tmp_path):
    a, b = tmp_path / "run_a", tmp_path / "run_b"
    for d, z, ids in ((a, 0.0, (1, 4, 9)), (b, H, (1, 4))):
        os.makedirs(d / "map_vis")
        for k in ids:
            v, f = square(z)
            mesh.TriMesh(v + [2.0 * k, 0, 0], f).export(str(d / "map_vis" / f"obj_{k}.ply"))
    out = tmp_path / "eval_geometry.json"
    map_eval.main(["--logdir", str(a), "--ref-logdir", str(b), "--samples", "500", "--scene-samples", "800",
                   "--thresholds", "0.1", "--seed", "2", "--out", str(out), "--device", str(dev)])
    r = json.load(open(out))
    assert sorted(r["objects"]) == ["1", "4"] and r["missing_gt"] == [9] and r["missing_pred"] == []
    for m in r["objects"].values():
        assert m["n_pred"] == 500 and m["n_gt"] == 500 and H <= m["accuracy"] < 0.1 and m["completion_ratio@0.1"] > 0.8
    s = r["scene"]
    assert s["n_pred"] == 800 and s["n_gt"] == 800 and s["completion"] >= H * (1 - 1e-6)
    assert s["accuracy"] > 0.2                                  # a third of pred's surface is object 9, 2 m from the rest
    # without --out the file lands in the log directory; the scene-only form against one whole mesh
    v = np.concatenate([square(H)[0] + [2.0 * k, 0, 0] for k in (1, 4)])
    mesh.TriMesh(v, np.concatenate([SQ_F, SQ_F + 4])).export(str(tmp_path / "scene.ply"))
    map_eval.main(["--logdir", str(a), "--gt-scene", str(tmp_path / "scene.ply"), "--scene-samples", "800",
                   "--device", str(dev)])
    r2 = json.load(open(a / "eval_geometry.json"))
    assert r2["objects"] == {} and r2["scene"]["n_gt"] == 800 and r2["scene"]["accuracy"] > 0.2
