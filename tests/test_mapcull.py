"""CPU: the numpy restatements the GPU tests of objnerf_meshcull.hip compare against (tests/mapcull_util.py) are checked
on their own -- the visibility rule on single vertices and on a plane, the compaction's counts and its invariant -- and
the host side of openobj_amd/map_cull.py: the dataset method, the frame batches, the interface and the command lines."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mapcull_util as U
import scene_files as SF
from conftest import ROOT
from openobj_amd import _lib, cfg, dataset, map_cull, map_eval, ops


@pytest.fixture(scope="module")
def frames():
    T_WC, depth = U.scene_depth(4)
    return U.to_cw(T_WC), depth


def seen0(frames, p, **kw):
    """Whether frame 0 sees the single vertex p."""
    return bool(U.views_ref(np.asarray(p, np.float64).reshape(1, 3), frames[0][:1], frames[1][:1], U.INTR, **kw)[0])


# ----------------------------------------------------------------------------------------------- the rule, one vertex
def test_scene_is_the_one_the_facts_are_about(frames):
    d = frames[1][0]
    assert d.shape == (SF.W, SF.H) and d.dtype == np.float32
    assert d[2, 20] == 3.0 and d[15, 20] == 1.5 and d[8, 10] == 1.5 and d[27, 33] == 1.5 and d[7, 10] == 3.0 and d[28, 34] == 3.0


def test_rule_depth_test(frames):
    assert seen0(frames, U.backproject(2, 20, 3.0))
    assert not seen0(frames, U.backproject(15, 20, 3.0))            # behind the box
    assert seen0(frames, U.backproject(15, 20, 1.5))
    assert seen0(frames, U.backproject(15, 20, 1.0))                # free space in front of the surface: seen
    assert seen0(frames, [0.0, 0.0, 3.05])                          # <=
    assert not seen0(frames, [0.0, 0.0, np.nextafter(3.05, 4.0)])
    assert not seen0(frames, [0.0, 0.0, 3.0], eps=-0.001) and seen0(frames, [0.0, 0.0, 3.0], eps=0.0)


def test_rule_front_and_non_finite(frames):
    for p in ([0.1, 0.1, 0.0], [0.1, 0.1, -2.0], [np.nan, 0, 3], [0, np.nan, 3], [0, 0, np.nan], [np.inf, 0, 3],
              [0, -np.inf, 3], [0, 0, np.inf], [0, 0, -np.inf], [1e300, 1e300, 1e300], [1e30, 1e30, 1e-300]):
        assert not seen0(frames, p), p
    assert seen0(frames, U.backproject(40, 5, 2.5)) and not seen0(frames, U.backproject(40, 5, 2.5), z_min=2.5)
    assert seen0(frames, U.backproject(40, 5, 2.5), z_min=np.nextafter(2.5, 0.0))


def test_rule_image_border_and_margin(frames):
    assert seen0(frames, U.backproject(63.49, 20, 3.0)) and not seen0(frames, U.backproject(63.5001, 20, 3.0))
    assert seen0(frames, U.backproject(-0.49, 20, 3.0)) and not seen0(frames, U.backproject(-0.5001, 20, 3.0))
    assert seen0(frames, U.backproject(40, 47.49, 3.0)) and not seen0(frames, U.backproject(40, 47.5001, 3.0))
    assert seen0(frames, U.backproject(40, -0.49, 3.0)) and not seen0(frames, U.backproject(40, -0.5001, 3.0))
    assert not seen0(frames, U.backproject(1, 20, 3.0), margin=2) and seen0(frames, U.backproject(2, 20, 3.0), margin=2)
    assert seen0(frames, U.backproject(61, 20, 3.0), margin=2) and not seen0(frames, U.backproject(62, 20, 3.0), margin=2)
    assert not seen0(frames, U.backproject(40, 1, 3.0), margin=2) and seen0(frames, U.backproject(40, 45, 3.0), margin=2)
    assert not seen0(frames, U.backproject(40, 46, 3.0), margin=2)


def test_boundary_vertices_helper_states_the_same_facts(frames):
    v, want, names = U.boundary_vertices()
    got = U.views_ref(v, frames[0][:1], frames[1][:1], U.INTR) > 0
    assert [n for n, g, w in zip(names, got, want) if g != w] == []


def test_rule_non_square_depth_catches_a_transposed_index():
    W, H = 7, 5
    depth = (1.0 + np.arange(W * H, dtype=np.float32).reshape(1, W, H))          # depth[iu, iv] = 1 + iu * H + iv
    intr = (10.0, 12.0, 3.0, 2.0)
    T = U.to_cw(np.eye(4)[None])
    for iu in range(W):
        for iv in range(H):
            d = float(depth[0, iu, iv])
            on = np.array([[(iu - 3.0) * d / 10.0, (iv - 2.0) * d / 12.0, d]])
            assert U.views_ref(on, T, depth, intr, eps=0.25)[0] == 1
            assert U.views_ref(on + [0, 0, 0.5] + [[(iu - 3.0) * 0.05, (iv - 2.0) / 24.0, 0]], T, depth, intr, eps=0.25)[0] == 0


# ------------------------------------------------------------------------------------------- plane and compaction
def test_plane_counts(frames):
    v, f = U.plane(3.0)
    assert v.shape == (9409, 3) and f.shape == (18432, 3)
    views = U.views_ref(v, *frames, U.INTR)
    assert int((views > 0).sum()) == 4570
    assert np.bincount(views, minlength=5).tolist() == [4839, 317, 355, 359, 3539]
    assert not U.views_ref(U.plane(3.06)[0], *frames, U.INTR).any()
    # a pose with a rotation: the same as moving the vertices the other way
    R = np.eye(4)
    c, s = np.cos(0.3), np.sin(0.3)
    R[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    R[:3, 3] = [0.2, -0.1, 0.05]
    moved = v @ R[:3, :3].T + R[:3, 3]
    a = U.views_ref(moved, U.to_cw(R[None]), frames[1][:1], U.INTR)
    b = U.views_ref(v, frames[0][:1], frames[1][:1], U.INTR)
    assert (a != b).mean() < 0.01 and (a > 0).sum() > 3000          # (equal up to rounding at pixel borders)


def test_plane_compaction(frames):
    v, f = U.plane(3.0)
    keep = U.views_ref(v, *frames, U.INTR) >= 1
    for rule, nv, nf in (("all", 4570, 8600), ("any", 5106, 9678)):
        r = U.compact_ref(keep, f, rule)
        assert (len(r["old_of_new"]), len(r["faces"])) == (nv, nf) and not r["bad"]
        assert np.array_equal(r["old_of_new"][r["faces"]], f[r["face_old"]])
        assert np.all(np.diff(r["old_of_new"]) > 0) and np.all(np.diff(r["face_old"]) > 0)
        assert np.array_equal(r["new_of_old"][r["old_of_new"]], np.arange(nv))
        assert (r["new_of_old"] >= 0).sum() == nv
        k = keep[f[r["face_old"]]]
        assert k.all() if rule == "all" else k.any(axis=1).all()
    assert keep[U.compact_ref(keep, f, "all")["old_of_new"]].all()
    assert not keep[U.compact_ref(keep, f, "any")["old_of_new"]].all()


def test_compaction_restatement_edge_cases():
    f = np.array([[0, 1, 2], [2, 3, 3], [2, 1, 0], [0, 1, 2], [4, 5, 1], [6, 0, 1], [-1, 0, 1]])
    r = U.compact_ref([1, 1, 1, 1, 0, 1], f, "all")
    assert r["bad"] and r["face_old"].tolist() == [0, 1, 2, 3] and r["old_of_new"].tolist() == [0, 1, 2, 3]
    r = U.compact_ref([0, 0, 0, 0, 1, 0], f[:5], "any")
    assert not r["bad"] and r["face_old"].tolist() == [4] and r["old_of_new"].tolist() == [1, 4, 5]
    assert r["faces"].tolist() == [[1, 2, 0]] and r["new_of_old"].tolist() == [-1, 0, -1, -1, 1, 2]
    r = U.compact_ref([1], np.zeros((0, 3)), "all")
    assert r["new_of_old"].tolist() == [-1] and len(r["old_of_new"]) == 0 and r["faces"].shape == (0, 3)


# --------------------------------------------------------------------------------------------------------- host logic
def scene_config(root, fmt):
    return cfg.Config(cfg.replica_room0_config(**{
        "dataset.path": str(root), "dataset.format": fmt, "trainer.part_mode": 0, "camera.w": SF.W, "camera.h": SF.H,
        "camera.fx": SF.FX, "camera.fy": SF.FY, "camera.cx": SF.CX, "camera.cy": SF.CY}))


@pytest.mark.parametrize("fmt", ["Replica", "ScanNet"])
def test_depth_and_pose_equals_the_sample(tmp_path, fmt):
    SF.write_scene(str(tmp_path), fmt, n_frames=30)
    ds = (dataset.Replica if fmt == "Replica" else dataset.ScanNet)(scene_config(tmp_path, fmt))
    assert len(ds) == 3
    for i in range(len(ds)):
        d, T = ds.depth_and_pose(i)
        s = ds[i]
        assert d.dtype == np.float32 and d.shape == (SF.W, SF.H)
        assert np.array_equal(d, s["depth"]) and np.array_equal(T, s["T"])
    assert ds.depth_and_pose(2)[1][0, 3] == 0.04


def test_depth_and_pose_reads_nothing_but_the_depth_image(tmp_path, monkeypatch):
    SF.write_scene(str(tmp_path), "Replica", n_frames=20)
    ds = dataset.Replica(scene_config(tmp_path, "Replica"))
    read = []
    real = dataset._read_image
    monkeypatch.setattr(dataset, "_read_image", lambda p: (read.append(os.path.relpath(p, str(tmp_path))), real(p))[1])
    ds.depth_and_pose(1)
    assert read == [os.path.join("depth", "depth_10.png")]


def test_frame_batches_shapes_ragged_tail_and_stride(tmp_path, frames):
    SF.write_scene(str(tmp_path), "Replica", n_frames=50)
    c = scene_config(tmp_path, "Replica")
    got = list(map_cull.frame_batches(c, batch=2))
    assert [(t.shape, d.shape) for t, d in got] == [((2, 4, 4), (2, SF.W, SF.H))] * 2 + [((1, 4, 4), (1, SF.W, SF.H))]
    assert all(t.dtype == np.float64 and d.dtype == np.float32 for t, d in got)
    T = np.concatenate([t for t, _ in got])
    assert T[:, 0, 3].tolist() == [0.0, 0.02, 0.04, 0.06, 0.08]
    T_WC, depth = U.scene_depth(5, as_loaded=True)
    assert np.array_equal(np.concatenate([d for _, d in got]), depth) and np.array_equal(T, T_WC)
    got = list(map_cull.frame_batches(c, stride=2, batch=32))
    assert len(got) == 1 and got[0][0][:, 0, 3].tolist() == [0.0, 0.04, 0.08]
    assert np.array_equal(got[0][1], depth[::2])
    assert map_cull.intrinsics_of(c) == U.INTR
    assert np.array_equal(map_cull.world_to_camera(T_WC), U.to_cw(T_WC))


NAMES = ["objnerf_vertex_views", "objnerf_mesh_cull_workspace_bytes", "objnerf_mesh_cull_count", "objnerf_mesh_cull_emit"]


def test_entry_points_are_declared_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "objnerf_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert n in _lib.SIGNATURES, n
        assert hasattr(l, n), n
        assert re.search(r"\b%s\s*\(" % n, header), n
    assert l.objnerf_abi_version() == 14                       # additive: the ABI number does not move
    assert l.objnerf_mesh_cull_workspace_bytes(1000, 2000) >= 1000 + 4 * (4 + 1) + 4 * (8 + 1)
    assert l.objnerf_mesh_cull_workspace_bytes(0, 0) > 0 and l.objnerf_mesh_cull_workspace_bytes(-1, 0) == 0


def test_cpu_tensors_are_rejected():
    v, t, d = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(1, 3, 4, dtype=torch.float64), torch.zeros(1, 8, 6)
    with pytest.raises(_lib.ObjnerfError):
        ops.vertex_views(v, t, d, U.INTR)
    with pytest.raises(_lib.ObjnerfError):
        ops.mesh_compact(torch.ones(4, dtype=torch.uint8), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.mesh_compact(torch.ones(4, dtype=torch.uint8), torch.zeros(1, 3, dtype=torch.int32), rule="most")


def test_map_cull_imports_without_a_gpu():
    code = ("import sys, openobj_amd.map_cull as m; assert m.EPS == 0.05 and m.MIN_VIEWS == 1 and m.MARGIN == 0; "
            "assert 'openobj_amd.ops' not in sys.modules and 'openobj_amd._lib' not in sys.modules")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    assert subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT).returncode == 0


def test_command_lines_parse(capsys):
    a = map_eval._parser().parse_args(["--logdir", "x", "--gt-dir", "y"])
    assert (a.samples, a.scene_samples, a.thresholds, a.seed, a.out, a.device, a.gt_scene, a.ref_logdir) == \
        (map_eval.N_SAMPLES, map_eval.N_SCENE_SAMPLES, [0.05, 0.01], 0, None, "cuda:0", None, None)
    assert a.cull_config is None
    assert (a.cull_stride, a.cull_eps, a.cull_min_views, a.cull_margin, a.cull_face_rule) == (1, 0.05, 1, 0, "all")
    a = map_eval._parser().parse_args(["--logdir", "x", "--gt-dir", "y", "--cull-config", "s.json", "--cull-stride", "5",
                                       "--cull-eps", "0.1", "--cull-min-views", "2", "--cull-margin", "3",
                                       "--cull-face-rule", "any"])
    assert (a.cull_config, a.cull_stride, a.cull_eps, a.cull_min_views, a.cull_margin, a.cull_face_rule) == \
        ("s.json", 5, 0.1, 2, 3, "any")
    with pytest.raises(SystemExit):
        map_eval._parser().parse_args(["--logdir", "x", "--cull-face-rule", "most"])
    a = map_cull._parser().parse_args(["--config", "s.json", "--in", "a", "--out", "b"])
    assert (a.config, a.src, a.out, a.stride, a.eps, a.min_views, a.margin, a.face_rule, a.device) == \
        ("s.json", "a", "b", 1, 0.05, 1, 0, "all", "cuda:0")
    assert map_cull.parameters(a.stride, a.eps, a.min_views, a.margin, a.face_rule) == \
        {"z_min": 0.0, "eps": 0.05, "margin": 0, "min_views": 1, "face_rule": "all", "stride": 1}
    with pytest.raises(SystemExit) as e:
        map_cull.main(["--help"])
    assert e.value.code == 0 and "--face-rule" in capsys.readouterr().out
