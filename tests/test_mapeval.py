"""CPU: the numpy restatements the GPU tests of objnerf_mapeval.hip compare against (tests/mapeval_util.py) are checked
on their own -- nearest points against scipy's k-d tree, the sampler's geometry and statistics -- and the host side of
openobj_amd/map_eval.py: the metrics, the interface and the command line."""
import os

import numpy as np
import pytest
import torch
from scipy import stats
from scipy.spatial import cKDTree

import mapeval_util as U
from openobj_amd import _lib, map_eval, ops


# ------------------------------------------------------------------------------------------------------------ nearest
def _against_tree(qry, ref):
    d2, idx = U.nearest_ref(qry, [0, len(qry)], ref, [0, len(ref)])
    dt, it = cKDTree(ref).query(qry)
    assert np.all(np.abs(np.sqrt(d2) - dt) <= 1e-12 * np.maximum(dt, 1e-300))
    uniq = U.unique_minimum(qry, [0, len(qry)], ref, [0, len(ref)], d2)
    assert np.array_equal(idx[uniq], it[uniq])
    return uniq


def test_nearest_restatement_matches_kdtree_random():
    rng = np.random.default_rng(0)
    uniq = _against_tree(rng.uniform(-1, 1, (5000, 3)), rng.uniform(-1, 1, (3000, 3)))
    assert uniq.all()


def test_nearest_restatement_matches_kdtree_lattice_with_ties():
    g = np.arange(6) * 0.25
    ref = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    qry = np.stack(np.meshgrid(g[:-1] + 0.125, g[:-1] + 0.125, g, indexing="ij"), -1).reshape(-1, 3)     # 4-way ties
    uniq = _against_tree(qry, ref)
    assert not uniq.any()
    d2, idx = U.nearest_ref(qry, [0, len(qry)], ref, [0, len(ref)])
    d = ref[None] - qry[:, None]
    m = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
    assert np.array_equal(idx, np.array([np.flatnonzero(r == r.min())[0] for r in m]))     # the smallest row of a tie


def test_nearest_restatement_segments_and_empty_reference():
    rng = np.random.default_rng(1)
    ref, qry = rng.normal(size=(7, 3)), rng.normal(size=(9, 3))
    d2, idx = U.nearest_ref(qry, [0, 4, 6, 9], ref, [0, 5, 5, 7])
    assert np.all(np.isinf(d2[4:6])) and np.all(idx[4:6] == -1)
    assert np.all((idx[:4] >= 0) & (idx[:4] < 5)) and np.all((idx[6:] >= 5) & (idx[6:] < 7))


# ------------------------------------------------------------------------------------------------------------ sampler
# four faces with areas 0.5 / 0.5 / 2 / 0 (the last one repeats a vertex)
QUAD_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [3, 0, 0], [3, 2, 0], [1, 2, 0]], np.float64)
QUAD_F = np.array([[0, 1, 2], [1, 3, 2], [1, 4, 5], [0, 6, 6]], np.int64)


def test_sampler_restatement_points_lie_in_their_triangles():
    rng = np.random.default_rng(2)
    verts = rng.normal(size=(40, 3))
    faces = rng.integers(0, 40, (60, 3))
    faces[7] = [3, 3, 9]                                       # zero area
    pts, tri = U.mesh_sample_ref(verts, faces, [0, 25, 60], [0, 700, 1500], seed=5)
    assert np.all(tri[:700] < 25) and np.all(tri[700:] >= 25)
    area, _ = U.face_weights(verts, faces)
    assert np.all(area[tri] > 0) and not np.any(tri == 7)
    A, B, C = verts[faces[tri, 0]], verts[faces[tri, 1]], verts[faces[tri, 2]]
    # every point: p - A = v (B - A) + w (C - A) solved through an orthonormal basis of the triangle's plane (QR)
    e1, e2, r = B - A, C - A, pts - A
    n1 = np.linalg.norm(e1, axis=1)
    q1 = e1 / n1[:, None]
    k = (e2 * q1).sum(1)
    h = e2 - k[:, None] * q1
    n2 = np.linalg.norm(h, axis=1)
    q2 = h / n2[:, None]
    w = (r * q2).sum(1) / n2
    v = ((r * q1).sum(1) - w * k) / n1
    assert len(pts) == 1500
    res = np.linalg.norm(v[:, None] * e1 + w[:, None] * e2 - r, axis=1)
    assert np.all(res <= 1e-12 * (1 + np.linalg.norm(r, axis=1)))               # in the plane
    for x in (v, w, 1 - v - w):
        assert np.all(x >= -1e-12) and np.all(x <= 1 + 1e-12)


def test_sampler_restatement_face_counts_follow_the_areas():
    n = 200000
    _, tri = U.mesh_sample_ref(QUAD_V, QUAD_F, [0, 4], [0, n], seed=11)
    cnt = np.bincount(tri, minlength=4)
    assert cnt[3] == 0                                         # a zero-area face is never drawn
    exp = n * np.array([0.5, 0.5, 2.0]) / 3.0
    chi2 = float(((cnt[:3] - exp) ** 2 / exp).sum())
    assert chi2 < 13.8, chi2                                   # the 99.9 % quantile of chi-square on 2 degrees of freedom
    assert stats.chi2.ppf(0.999, 2) == pytest.approx(13.8, abs=0.02)


def test_sampler_restatement_prefix_property():
    p1, t1 = U.mesh_sample_ref(QUAD_V, QUAD_F, [0, 4], [0, 1000], seed=3)
    p2, t2 = U.mesh_sample_ref(QUAD_V, QUAD_F, [0, 4], [0, 100], seed=3)
    assert np.array_equal(p1[:100], p2) and np.array_equal(t1[:100], t2)
    p3, _ = U.mesh_sample_ref(QUAD_V, QUAD_F, [0, 4], [0, 100], seed=4)
    assert not np.array_equal(p2, p3)


# ------------------------------------------------------------------------------------------------------------ metrics
def test_metrics_from_distances():
    acc = np.array([0.01, 0.03, np.inf, 0.02])
    comp = torch.tensor([0.005, 0.2, float("nan"), 0.04, 0.009], dtype=torch.float64)
    m = map_eval.metrics_from_distances(acc, comp, thresholds=(0.05, 0.01))
    assert m["accuracy"] == pytest.approx(0.02, rel=1e-15)
    assert m["completion"] == pytest.approx((0.005 + 0.2 + 0.04 + 0.009) / 4, rel=1e-15)
    assert m["chamfer"] == pytest.approx(0.5 * (m["accuracy"] + m["completion"]), rel=1e-15)
    assert m["completion_ratio@0.05"] == 3 / 5 and m["completion_ratio@0.01"] == 2 / 5      # the NaN counts as a miss
    assert (m["n_pred"], m["n_gt"], m["n_nonfinite"]) == (4, 5, 2)
    r = U.metrics_ref(acc, comp.numpy(), (0.05, 0.01))
    for k, v in r.items():
        assert m[k] == pytest.approx(v, rel=1e-12), k


def test_metrics_of_an_empty_object():
    m = map_eval.metrics_from_distances(np.zeros(0), np.zeros(0), thresholds=(0.05,))
    assert m["accuracy"] is None and m["completion"] is None and m["chamfer"] is None
    assert m["completion_ratio@0.05"] is None and m["n_pred"] == 0 and m["n_gt"] == 0
    m = map_eval.metrics_from_distances(np.array([np.inf, np.inf]), np.zeros(0), thresholds=())
    assert m["accuracy"] is None and m["n_pred"] == 2 and m["n_nonfinite"] == 2


# ---------------------------------------------------------------------------------------------------------- interface
NAMES = ["objnerf_mesh_sample_workspace_bytes", "objnerf_mesh_sample", "objnerf_nearest_workspace_bytes", "objnerf_nearest",
         "objnerf_seg_stats"]


def test_entry_points_are_declared_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES, n
        assert hasattr(l, n), n
    assert l.objnerf_abi_version() == 14                       # additive: the ABI number does not move
    assert l.objnerf_nearest_workspace_bytes(1000, 3) > 0 and l.objnerf_mesh_sample_workspace_bytes(1000, 3) >= 8000


def test_cpu_tensors_are_rejected():
    p = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(_lib.ObjnerfError):
        ops.nearest(p, [0, 4], p, [0, 4])
    with pytest.raises(_lib.ObjnerfError):
        ops.mesh_sample(p, torch.zeros(1, 3, dtype=torch.int32), [0, 1], [0, 2], 0)
    with pytest.raises(_lib.ObjnerfError):
        ops.seg_stats(torch.zeros(4, dtype=torch.float64), [0, 4], (0.1,))
    with pytest.raises(_lib.ObjnerfError):
        ops.NearestPlan(p, [0, 4])


def test_command_line_parses(capsys):
    with pytest.raises(SystemExit) as e:
        map_eval.main(["--help"])
    assert e.value.code == 0
    assert "--ref-logdir" in capsys.readouterr().out
    a = map_eval._parser().parse_args(["--logdir", "x", "--gt-dir", "y", "--samples", "50", "--thresholds", "0.1", "0.2"])
    assert (a.samples, a.thresholds, a.scene_samples, a.seed) == (50, [0.1, 0.2], map_eval.N_SCENE_SAMPLES, 0)
    with pytest.raises(SystemExit):
        map_eval._parser().parse_args(["--logdir", "x", "--gt-dir", "y", "--ref-logdir", "z"])
