"""CPU: the ray caster's specification against itself (tests/maprays_util.py) -- the gates (b) and (d)
reject nothing the triangle sequence accepts, a tree walk with the header's pruning rule equals brute force, -0 never
reaches a key, the ray specification and the raster specification name the same face through view_rays -- and the host
side of openobj_amd/map_rays.py: the ray generators, the CLI's argument checks, `sight` with cast stubbed by the
specification."""
import functools
import gzip
import json
import os
import pickle
import types

import numpy as np
import pytest

from openobj_amd import map_rays
try:
    from tests import maprays_util as U, mapraster_util as RU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import maprays_util as U
    import mapraster_util as RU

SIX = ("dense", "coarse", "interpenetrating", "giant", "on_samples", "duplicate")


@functools.lru_cache(maxsize=None)
def scene(name):
    return U.scene_of(name)


def through(m, targets):
    eye = np.asarray(m["cam"], np.float64)
    return np.broadcast_to(eye, targets.shape).copy(), targets - eye


# ------------------------------------------------------------------------------------------------ 1. the specification
@pytest.mark.parametrize("name", SIX)
def test_gates_reject_no_face_the_triangle_sequence_accepts(name):
    """Over the pixel rays and the rays through every vertex and every edge midpoint: 0 of the accepted pairs."""
    m = scene(name)
    o1, d1 = U.view_rays(m["T_WC"], m["intr"], m["W"], m["H"])
    o2, d2 = through(m, np.asarray(m["verts"], np.float64))
    o3, d3 = through(m, U.edge_midpoints(m))
    o, d = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])
    r = U.brute_force(m, o, d, count_rejected=True)
    hits = int((r["key"] != U.EMPTY).sum())
    print(f"{name}: {len(o)} rays, {hits} hit, {r['rejected']} pairs rejected by the gates alone")
    assert hits >= 3000 and r["rejected"] == 0


@pytest.mark.parametrize("name", SIX)
def test_tree_walk_equals_brute_force(name):
    m = scene(name)
    o, d = U.scene_rays(m)
    sel = np.arange(0, len(o), max(len(o) // 333, 1))
    o, d = o[sel], d[sel]
    a, ab = U.segments_of(m, 60)
    full = U.brute_force(m, o, d)
    seg = U.brute_force(m, a, ab, 0.0, 1.0)
    assert (full["key"] != U.EMPTY).sum() > len(o) // 2 and 0 < (seg["key"] != U.EMPTY).sum() < len(a)
    P = full["P"]
    for leaf in (1, 4, 8):
        tree = U.build_tree(P, leaf)
        for i in range(len(o)):
            assert U.tree_walk(P, tree, o[i], d[i], 0.0, np.inf)[0] == full["key"][i], (leaf, i)
        for i in range(len(a)):
            assert U.tree_walk(P, tree, a[i], ab[i], 0.0, 1.0)[0] == seg["key"][i], (leaf, "segment", i)


def test_tree_walk_on_parallel_and_vertex_rays():
    """The 4 000 vertex and axis-parallel rays of the issue's check, thinned to what a test may cost: every special ray
    of `coarse` (infinite inv, parallel axes exactly on box faces, origins on faces, bad rays), segments included."""
    m = scene("coarse")
    o, d = U.special_rays(m, n_each=120)
    full = U.brute_force(m, o, d)
    P = full["P"]
    tree = U.build_tree(P, 4)
    visits = 0
    for i in range(len(o)):
        k, v = U.tree_walk(P, tree, o[i], d[i], 0.0, np.inf)
        visits += v
        assert k == full["key"][i], i
    assert visits < len(o) * (2 * tree["size"] - 1)                   # (the walk prunes at all)
    seg = U.brute_force(m, o, d, 0.0, 1.0)
    for i in range(len(o)):
        assert U.tree_walk(P, tree, o[i], d[i], 0.0, 1.0)[0] == seg["key"][i], i


def test_origin_on_a_plane_gives_plus_zero():
    """T = -0 (an origin exactly on the face's plane, seen from the side where the signs fall that way) must not become
    a key with the sign bit set: such a key orders after every positive t and a farther face would win."""
    verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 2.0], [1.0, 0.0, 2.0], [0.0, 1.0, 2.0]])
    found = False
    for faces in ([[0, 1, 2], [3, 4, 5]], [[0, 2, 1], [3, 5, 4]]):
        for dz in (1.0, -1.0):
            m = {"verts": verts, "faces": np.array(faces, np.int32), "face_off": np.array([0, 2]), "ids": np.array([7], np.int32)}
            o, d = np.array([[0.25, 0.25, 0.0]]), np.array([[0.0, 0.0, dz]])
            P = U.prepare(m, 0.0)
            with np.errstate(all="ignore"):
                _, det, _, _, T, _ = U.triangle(o, d, P["p0"][:1], P["e1"][:1], P["e2"][:1])
                found |= bool(np.signbit(T / det)[0])
            r = U.run_spec(m, o, d, pad=0.0)
            assert r["t"].view(np.uint32)[0] == 0 and r["face"][0] == 0, (faces, dz)        # +0, the near face
            assert np.array_equal(r["point"][0], o[0])
    assert found                                                      # (one of the four cases does produce -0 before + 0.0)


@pytest.mark.parametrize("name", ["coarse", "giant", "on_samples", "dense"])
def test_ray_specification_against_raster_specification(name):
    """Through view_rays of the scene's camera the two specifications name the same face: at every pixel of coarse, giant
    and on_samples; on dense wherever the hit's smallest barycentric coordinate is at least 1e-3 (at least 3 100 of the
    3 150 pixels).  The depths differ because the rasteriser snaps vertices to 1 / 256 pixel: at most 2e-4 m."""
    m = scene(name)
    o, d = map_rays.view_rays(m["T_WC"], m["intr"], m["W"], m["H"])
    o2, d2 = U.view_rays(m["T_WC"], m["intr"], m["W"], m["H"])
    assert np.array_equal(o, o2) and np.array_equal(d, d2)
    ray = U.run_spec(m, o, d, t_min=m["z_near"])
    key, _, _ = RU.visibility(m, m["T_CW"], m["intr"], m["W"], m["H"], m["z_near"], m["hide"])
    key = RU.key_array(key).reshape(-1)
    face = np.where(key != U.EMPTY, key & np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFFFF)).astype(np.uint32).astype(np.int32)
    depth = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
    if name == "dense":
        with np.errstate(invalid="ignore"):
            u, v = ray["bary"][:, 0], ray["bary"][:, 1]
            inner = (np.minimum(np.minimum(u, v), (1.0 - u) - v) >= 1e-3) | (ray["face"] < 0)
        keep = inner
        print(f"dense: {int(keep.sum())} of {len(keep)} pixels kept")
        assert keep.sum() >= 3100
    else:
        keep = np.ones(len(face), bool)
    same = ray["face"] == face
    assert same[keep].all(), f"{name}: {int((~same & keep).sum())} pixels name another face"
    both = keep & same & (face >= 0)
    gap = np.abs(depth[both].astype(np.float64) - ray["t"][both].astype(np.float64))
    print(f"{name}: {int(both.sum())} pixels hit, the largest depth gap {gap.max():.3g}")
    assert both.sum() > len(face) // 2 and gap.max() <= 2e-4


# ------------------------------------------------------------------------------------------------ 2. the ray generators
def test_view_rays_shapes_and_values():
    T = RU.look_at((1.0, 2.0, -3.0), (0.5, 0.0, 0.0), up=(0.0, -1.0, 0.0))
    o, d = map_rays.view_rays(T, (60.0, 50.0, 34.5, 22.0), 7, 5)
    assert o.shape == (35, 3) and d.shape == (35, 3) and o.dtype == np.float64 and d.dtype == np.float64
    assert np.all(o == T[:3, 3])
    dc = d @ T[:3, :3]                                                 # back in the camera frame
    i, j = 3, 4
    assert np.allclose(dc[i * 5 + j], [(3 - 34.5) / 60.0, (4 - 22.0) / 50.0, 1.0], atol=1e-14)
    # a point at depth z along ray (i, j) projects back onto the sample point of pixel (i, j)
    p = o[i * 5 + j] + 2.5 * d[i * 5 + j]
    pc = np.linalg.inv(T) @ np.append(p, 1.0)
    assert abs(pc[2] - 2.5) < 1e-12 and abs(60.0 * pc[0] / pc[2] + 34.5 - i) < 1e-10 and abs(50.0 * pc[1] / pc[2] + 22.0 - j) < 1e-10
    for bad in (dict(T_WC=np.eye(3)), dict(intrinsics=(1.0, 2.0, 3.0)), dict(W=0), dict(intrinsics=(0.0, 1.0, 0.0, 0.0))):
        kw = dict(T_WC=T, intrinsics=(60.0, 50.0, 34.5, 22.0), W=7, H=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            map_rays.view_rays(**kw)


def test_lidar_rays_shapes_and_values():
    T = np.eye(4)
    T[:3, 3] = (1.0, 2.0, 3.0)
    o, d = map_rays.lidar_rays(T, 8, 3, -30.0, 30.0)
    assert o.shape == (24, 3) and d.shape == (24, 3) and np.all(o == (1.0, 2.0, 3.0))
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-15)
    assert np.allclose(d[1], [1.0, 0.0, 0.0], atol=1e-15)             # azimuth 0, the middle elevation 0
    assert np.allclose(d[2 * 3 + 1], [0.0, 1.0, 0.0], atol=1e-15)     # azimuth 90 degrees
    assert np.allclose(d[0], [np.cos(np.pi / 6), 0.0, -0.5], atol=1e-15) and np.allclose(d[2, 2], 0.5, atol=1e-15)
    R = RU.look_at((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))[:3, :3]
    T2 = np.eye(4)
    T2[:3, :3] = R
    d2 = map_rays.lidar_rays(T2, 8, 3, -30.0, 30.0)[1]
    assert np.allclose(d2, d @ R.T, atol=1e-15)
    assert map_rays.lidar_rays(T, 4, 1, 10.0, 20.0)[1].shape == (4, 3)
    for kw in (dict(n_az=0), dict(el_min=40.0), dict(el_max=91.0), dict(T_WS=np.full((4, 4), np.nan))):
        a = dict(T_WS=T, n_az=8, n_el=3, el_min=-30.0, el_max=30.0)
        a.update(kw)
        with pytest.raises(ValueError):
            map_rays.lidar_rays(**a)


# ---------------------------------------------------------------------------------------------------------- 3. the CLI
def two_sheets():
    """Object 11: a wall at z = 0; object 12: a small sheet behind it at z = 1; object 13: a sheet beside the wall."""
    wall = RU.sheet_object(4, 4, (2.0, 2.0), centre=(0.0, 0.0, 0.0))
    behind = RU.sheet_object(3, 3, (0.5, 0.5), centre=(0.0, 0.0, 1.0))
    beside = RU.sheet_object(3, 3, (0.5, 0.5), centre=(3.0, 0.0, 1.0))
    m = RU.scene([wall, behind, beside], ids=[11, 12, 13])
    meshes = [types.SimpleNamespace(vertices=v, faces=f) for v, f in (wall, behind, beside)]
    mq = types.SimpleNamespace(keys=[11, 12, 13], S=3, all_obj={k: {"mesh": g} for k, g in zip((11, 12, 13), meshes)})
    return m, mq


def spec_cast(m):
    def cast(origins, dirs, t_min=0.0, t_max=np.inf, hide=()):
        h = np.zeros(len(m["face_off"]) - 1, np.uint8)
        h[[int(x) for x in hide]] = 1
        r = U.run_spec(m, origins, dirs, t_min, t_max, hide=h)
        r["hit"] = r["hit"] != 0
        return r
    return cast


def test_sight_on_a_hand_made_nav():
    m, mq = two_sheets()
    nav = {"objects": [{"id": 11, "goal": [0.0, 0.0, -2.0]}, {"id": 12, "goal": [0.0, 0.0, -2.0]},
                       {"id": 13, "goal": [3.0, 0.0, -2.5]}, {"id": 12, "goal": None}, {"id": 99, "goal": [0.0, 0.0, 0.0]}]}
    rows = map_rays.sight_records(spec_cast(m), mq, nav, eye_height=0.5, up_axis=2)
    assert [r["id"] for r in rows] == [11, 12, 13, 12, 99]
    assert [r["sees"] for r in rows] == [True, False, True, None, None]
    assert [r["blocker"] for r in rows] == [None, 11, None, None, None]
    assert rows[0]["eye"] == [0.0, 0.0, -1.5] and rows[2]["eye"] == [3.0, 0.0, -2.0]
    v = np.asarray(mq.all_obj[12]["mesh"].vertices)
    assert rows[1]["target"] == v[np.argmin(((v - np.array(rows[1]["eye"])) ** 2).sum(axis=1))].tolist()
    # with the wall hidden the sheet behind it is seen
    rows = map_rays.sight_records(spec_cast(m), mq, nav, 0.5, 2, hide=[0])
    assert [r["sees"] for r in rows] == [True, True, True, None, None]
    json.dumps(rows)


def test_cli_argument_checks(tmp_path, capsys):
    log = tmp_path / "log"
    os.makedirs(log)
    with gzip.open(log / "map_vis.pkl.gz", "wb") as fh:
        pickle.dump({1: {}, 2: {}}, fh)
    np.save(tmp_path / "rays.npy", np.zeros((5, 6)))
    np.save(tmp_path / "flat.npy", np.zeros((5, 5)))
    np.savetxt(tmp_path / "pose.txt", np.eye(4))
    with open(tmp_path / "nav.json", "w") as fh:
        json.dump({"objects": []}, fh)
    with open(tmp_path / "other.json", "w") as fh:
        json.dump([1, 2], fh)
    base = ["--logdir", str(log), "--out", str(tmp_path / "out")]
    rays, lidar = ["--rays", str(tmp_path / "rays.npy")], ["--lidar", str(tmp_path / "pose.txt"), "--beams", "8", "2", "-10", "10"]
    bad = [
        ["cast"] + base,                                               # neither --rays nor --lidar
        ["cast"] + base + rays + lidar,
        ["cast"] + base + ["--rays", str(tmp_path / "nope.npy")],
        ["cast"] + base + ["--rays", str(tmp_path / "flat.npy")],
        ["cast"] + base + ["--lidar", str(tmp_path / "pose.txt")],     # no --beams
        ["cast"] + base + ["--lidar", str(tmp_path / "pose.txt"), "--beams", "8.5", "2", "-10", "10"],
        ["cast"] + base + ["--lidar", str(tmp_path / "pose.txt"), "--beams", "8", "2", "20", "10"],
        ["cast"] + base + rays + ["--beams", "8", "2", "-10", "10"],
        ["cast"] + base + rays + ["--t-min", "-1"],
        ["cast"] + base + rays + ["--t-min", "2", "--t-max", "1"],
        ["cast"] + base + rays + ["--nav", str(tmp_path / "nav.json")],
        ["cast"] + base + rays + ["--leaf", "0"],
        ["cast"] + base + rays + ["--hide", "walls"],
        ["cast"] + base + rays + ["--hide", "ceiling"],                # a named set needs --dataset
        ["cast"] + base + rays + ["--hide", "2"],                      # two objects: positions 0 and 1
        ["cast", "--logdir", str(tmp_path / "nolog"), "--out", str(tmp_path / "out")] + rays,
        ["cast"] + base + rays + ["--mode", "part"],                   # the mode needs its queries
        ["sight"] + base,
        ["sight"] + base + ["--nav", str(tmp_path / "nope.json")],
        ["sight"] + base + ["--nav", str(tmp_path / "other.json")],
        ["sight"] + base + ["--nav", str(tmp_path / "nav.json")] + rays,
        ["sight"] + base + ["--nav", str(tmp_path / "nav.json"), "--up-axis", "3"],
        ["sight"] + base + ["--nav", str(tmp_path / "nav.json"), "--eye-height", "nan"],
        ["look"] + base,
    ]
    for argv in bad:
        with pytest.raises(SystemExit):
            map_rays._parse(argv)
    capsys.readouterr()
    a, all_obj, _ = map_rays._parse(["cast"] + base + lidar + ["--hide", "1"])
    assert a.origins.shape == (16, 3) and a.dirs.shape == (16, 3) and a.mode == "rgb" and len(all_obj) == 2
    a, _, _ = map_rays._parse(["cast"] + base + rays)
    assert a.origins.shape == (5, 3) and a.t_min == 0.0 and a.t_max == float("inf")
    a, _, _ = map_rays._parse(["sight"] + base + ["--nav", str(tmp_path / "nav.json"), "--eye-height", "1.2"])
    assert a.nav_doc == {"objects": []} and a.eye_height == 1.2 and a.up_axis == 2


def test_points_ply(tmp_path):
    p = tmp_path / "p.ply"
    map_rays.write_points_ply(str(p), [[0.5, 1.0, -2.0], [1e-3, 2.0, 3.0]], [[1, 2, 3], [255, 0, 9]])
    lines = open(p).read().splitlines()
    assert lines[0] == "ply" and "element vertex 2" in lines and lines[-2:] == ["0.5 1.0 -2.0 1 2 3", "0.001 2.0 3.0 255 0 9"]
