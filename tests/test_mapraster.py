"""CPU: the specification of the mesh rasteriser (tests/mapraster_util.py) is watertight and stays inside
fp64's exact integers; the host arithmetic of openobj_amd.map_raster (the camera rows, pick's points), its CLI's argument
checks, and map_query's colour dispatch after it moved into a function."""
import gzip
import itertools
import os
import pickle

import numpy as np
import pytest

from openobj_amd import map_cull, map_query, map_raster
try:
    from tests import mapraster_util as U, mapregions_util as RU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import mapraster_util as U
    import mapregions_util as RU


# ------------------------------------------------------------------------------------------------ 1. the specification
@pytest.mark.parametrize("n,jitter,tilt,seed", [((9, 7), 0.6, 0.5, 0), ((40, 38), 0.6, 0.5, 1), ((5, 4), 0.5, -0.4, 2)])
def test_specification_is_watertight(n, jitter, tilt, seed):
    """A jittered, tilted sheet whose two triangles per cell have opposite orientations overhangs the screen: every one of
    the 70 x 45 pixels is painted, by a face of the sheet, at a depth between the sheet's nearest and farthest vertex."""
    m = U.overhang_sheet(n, jitter, tilt, seed)
    o = U.run_spec(m)
    assert np.all(o["key"] != np.uint64(U.EMPTY)) and np.all(o["winner"] == 0) and o["counts"].tolist() == [U.W0 * U.H0]
    assert o["status"] == 0 and int(o["stats"].sum()) == len(m["faces"])
    zc = m["verts"] @ m["T_CW"][2, :3] + m["T_CW"][2, 3]
    assert zc.min() * (1 - 1e-6) <= o["depth"].min() and o["depth"].max() <= zc.max() * (1 + 1e-6)
    assert np.all(o["maskid"] == m["ids"][0]) and np.all(o["face"] >= 0)
    # the vertex under a pixel is a corner of the face under it
    assert all(o["vertex"][i, j] in m["faces"][o["face"][i, j]] for i in range(U.W0) for j in range(U.H0))


def test_both_sides_are_drawn_and_orientation_decides_nothing():
    m = U.overhang_sheet((9, 7), 0.6, 0.5, 0)
    a, b = U.run_spec(m), U.run_spec(U.reversed_faces(m))
    for k in ("key", "depth", "maskid", "winner", "face", "counts", "stats", "vertex", "rgb"):
        assert np.array_equal(a[k], b[k]), k


def test_edge_functions_stay_below_2_to_53_at_the_bound():
    """Corners anywhere on the 2^25 bound, sample points anywhere on the largest screen: every edge function and the
    area stay below 2^53, so (double) w is exact."""
    B, P = 2 ** 25, 256 * 65535
    worst = 0
    for ax, ay, bx, by in itertools.product((-B, B), repeat=4):
        for px, py in itertools.product((0, P), repeat=2):
            worst = max(worst, abs(U.edge(ax, ay, bx, by, px, py)))
        for cx, cy in itertools.product((-B, B), repeat=2):
            worst = max(worst, abs((bx - ax) * (cy - ay) - (by - ay) * (cx - ax)))
    assert 2 ** 51 < worst < 2 ** 53
    # and the specification itself, on a triangle with corners at the bound: the tracked maximum agrees
    T = np.eye(4)
    v = np.array([[-B / 256.0, -B / 256.0, 1.0], [B / 256.0, -B / 256.0, 1.0], [0.0, B / 256.0, 1.0]])
    m = U.scene([(v, np.array([[0, 1, 2]]))], T_WC=T, intr=(1.0, 1.0, 0.0, 0.0), W=9, H=7)
    seen = []
    key, stats, _ = U.visibility(m, m["T_CW"], m["intr"], 9, 7, m["z_near"], track_w=seen)
    assert stats[U.ST["large"]] == 1 and U.painted(key) == 63 and 2 ** 50 < seen[0] < 2 ** 53
    v[0, 0] -= 1.0                                                   # one step past the bound: dropped, and counted so
    m = U.scene([(v, np.array([[0, 1, 2]]))], T_WC=T, intr=(1.0, 1.0, 0.0, 0.0), W=9, H=7)
    key, stats, _ = U.visibility(m, m["T_CW"], m["intr"], 9, 7, m["z_near"])
    assert stats[U.ST["bound"]] == 1 and U.painted(key) == 0


def test_scene_claims_hold_in_the_specification():
    """What tests/test_mapraster_gpu.py claims of its scenes, checked here from the specification alone."""
    for name, (m, claims) in U.make_scenes().items():
        key, stats, status = U.visibility(m, m["T_CW"], m["intr"], m["W"], m["H"], m["z_near"], m["hide"])
        assert sum(stats) == len(m["faces"]) and status == 0, name
        for c in claims:
            if c == "half":
                assert 2 * U.painted(key) >= m["W"] * m["H"], name
            elif c == "both":
                assert stats[U.ST["small"]] >= 1 and stats[U.ST["large"]] >= 1, name
            else:
                assert stats[U.ST[c]] >= 1, (name, c)
    key, stats, status = (lambda m: U.visibility(m, m["T_CW"], m["intr"], m["W"], m["H"], m["z_near"]))(U.bad_index_scene())
    assert status == 1 and stats[U.ST["bad_index"]] == 2


# -------------------------------------------------------------------------------------------------- 2. host arithmetic
def test_camera_rows():
    T = U.look_at((0.3, -1.0, 2.0), (0.1, 0.2, 0.0))
    M = map_raster.camera_rows(T)
    assert M.shape == (3, 4) and M.dtype == np.float64 and M.flags["C_CONTIGUOUS"]
    assert np.array_equal(M, map_cull.world_to_camera(T[None])[0]) and np.array_equal(M, U.world_to_camera(T))
    np.testing.assert_allclose(np.vstack([M, [0, 0, 0, 1]]) @ T, np.eye(4), atol=1e-14)
    np.testing.assert_allclose(M[:, :3] @ T[:3, 3] + M[:, 3], 0.0, atol=1e-14)         # the camera centre maps to 0
    assert np.array_equal(map_raster.camera_rows(T.astype(np.float32)), map_raster.camera_rows(T.astype(np.float32).astype(np.float64)))
    for bad in (np.eye(3), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError):
            map_raster.camera_rows(bad)


def test_pick_points_equal_the_specification():
    m, _ = U.make_scenes()["interpenetrating"]
    o = U.run_spec(m)
    px = np.array([(i, j) for i in range(m["W"]) for j in range(m["H"])])
    faces = o["face"].reshape(-1)
    assert np.all(faces >= 0)
    corners = m["verts"][m["faces"][faces]]
    pts, b = map_raster.pick_points(corners, px, m["T_CW"], m["intr"], m["z_near"])
    assert np.array_equal(pts, o["point"].reshape(-1, 3))
    assert np.all(b >= 0) and np.abs(b.sum(1) - 1).max() < 1e-12
    # the point lies on its face and projects back onto its pixel
    X, Y, _, zc = map_raster.project_vertices(pts, m["T_CW"], m["intr"])
    assert np.abs(X / 256.0 - px[:, 0]).max() < 0.01 and np.abs(Y / 256.0 - px[:, 1]).max() < 0.01
    np.testing.assert_allclose(zc, o["depth"].reshape(-1), rtol=1e-6)
    # a pixel the face does not cover, a degenerate face and a face behind the camera give NaN rows
    far = corners[:1] + np.array([50.0, 0.0, 0.0])
    flat = np.repeat(corners[:1, :1], 3, axis=1)
    back = corners[:1] - np.array([0.0, 0.0, 10.0])
    for c in (far, flat, back):
        assert np.isnan(map_raster.pick_points(c, px[:1], m["T_CW"], m["intr"], m["z_near"])[0]).all()
    assert map_raster.pick_points(np.zeros((0, 3, 3)), np.zeros((0, 2)), m["T_CW"], m["intr"])[0].shape == (0, 3)


class FakeMap:
    """Records what a colour dispatch asks of a MapQuery."""
    dev = "cpu"

    def __init__(self, all_obj=None):
        self.all_obj = all_obj or {}
        self.keys = list(self.all_obj)
        self.S = len(self.keys)

    def color_by_rgb(self):
        return ("rgb",)

    def color_by_class(self, y):
        return ("class", y)

    def color_by_instance(self):
        return ("instance",)

    def color_by_partfeat(self):
        return ("partpca",)

    def color_by_object_query(self, c, s, top):
        return ("object", c, s, top)

    def color_by_part_query(self, c, s, p, top):
        return ("part", c, s, p, top)

    def hidden_sets(self, dataset, scene):
        return {"ceiling": [1], "most": [0, 2], "hidden": [1] if dataset == "Replica" else []}


def test_colour_dispatch_is_what_map_query_did():
    q = {"clip_query": "C", "sbert_query": "S", "part_query": "P"}
    mq = FakeMap()
    f = map_query.colors_for_mode
    assert f(mq, "rgb", q) == ("rgb",) and f(mq, "instance", q) == ("instance",)
    assert f(mq, "class", q, color_yaml="y.yaml") == ("class", "y.yaml")
    assert f(mq, "partpca", q) == ("partpca",) == f(mq, "partfeat", q)
    assert f(mq, "object", q) == ("object", "C", "S", 0) and f(mq, "object", q, top=3) == ("object", "C", "S", 3)
    assert f(mq, "part", q) == ("part", "C", "S", "P", 1) and f(mq, "part", q, top=2) == ("part", "C", "S", "P", 2)
    with pytest.raises(ValueError):
        f(mq, "nothing", q)


def test_ids_and_hide():
    objs = {10: {"class_id": 4}, 13: {"class_id": 7}, 21: {}}
    mr = map_raster.MapRaster(FakeMap(objs), "Replica")
    assert mr.ids_of("obj").tolist() == [10, 13, 21] and mr.ids_of("class").tolist() == [4, 7, 0]
    assert mr.ids_of([1, 2, 3]).dtype == np.int32
    for bad in ("nothing", [1, 2]):
        with pytest.raises(ValueError):
            mr.ids_of(bad)
    assert mr.hide_mask(()).tolist() == [0, 0, 0] and mr.hide_mask([2]).tolist() == [0, 0, 1]
    assert mr.hide_mask("ceiling").tolist() == [0, 1, 0] and mr.hide_mask(["most", "1"]).tolist() == [1, 1, 1]
    assert mr.hide_mask(["hidden"]).tolist() == [0, 1, 0]
    for bad in ([3], ["floor"], [-1]):
        with pytest.raises(ValueError):
            mr.hide_mask(bad)
    with pytest.raises(RuntimeError):
        mr.visible()


# ---------------------------------------------------------------------------------------------------------- 3. the CLI
@pytest.fixture(scope="module")
def logdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("raster_cli")
    all_obj, _, q, info = RU.planted_map()
    with gzip.open(d / map_query.COMPACT_FILE, "wb") as fh:
        pickle.dump(all_obj, fh)
    np.savetxt(d / "pose.txt", U.look_at((2.6, 0.42, -1.0), (2.6, 0.42, 0.4), up=(0.0, -1.0, 0.0)))
    np.savetxt(d / "short.txt", np.arange(15.0))
    np.savetxt(d / "singular.txt", np.zeros((4, 4)))
    np.save(d / "c.npy", info["clip_query"])
    np.save(d / "s.npy", info["sbert_query"])
    np.save(d / "p.npy", q.astype(np.float32))
    np.save(d / "narrow.npy", np.zeros(7, np.float32))
    return d


def cli(d, *extra, pose="pose.txt", mode="rgb"):
    base = ["--logdir", str(d), "--out", str(d / "out"), "--mode", mode]
    if pose:
        base += ["--pose", str(d / pose), "--size", "70", "45", "--intrinsics", "60", "60", "34.5", "22"]
    return base + list(extra)


def test_cli_arguments(logdir, capsys):
    d = logdir
    a, all_obj, q = map_raster._parse(cli(d, "--hide", "1", "--shading", "none"))
    assert a.T_WC.shape == (4, 4) and a.size == [70, 45] and a.hide == ["1"] and a.shading == "none" and q == {}
    assert list(all_obj) == [10, 13] and a.map_file.endswith(map_query.COMPACT_FILE) and a.z_near == map_raster.Z_NEAR
    a, _, q = map_raster._parse(cli(d, "--clip-query", str(d / "c.npy"), "--sbert-query", str(d / "s.npy"), "--part-query",
                                    str(d / "p.npy"), "--hide", "ceiling", "--dataset", "Replica", mode="part"))
    assert set(q) == {"clip_query", "sbert_query", "part_query"} and q["part_query"].shape == (512,)
    assert map_raster._parse(cli(d, mode="partfeat"))[0].mode == "partfeat"
    bad = [
        cli(d, pose=None),                                                            # no camera
        cli(d, "--config", str(d / "pose.txt")),                                      # two cameras
        ["--logdir", str(d), "--out", "o", "--mode", "rgb", "--pose", str(d / "pose.txt")],          # no size
        cli(d, "--frames", "0:2"),                                                    # frames without a dataset
        cli(d, pose="nothing.txt"), cli(d, pose="short.txt"), cli(d, pose="singular.txt"),
        cli(d, "--hide", "ceiling"),                                                  # a named set without --dataset
        cli(d, "--hide", "floor", "--dataset", "Replica"), cli(d, "--hide", "2"), cli(d, "--hide", "-1"),
        cli(d, "--z-near", "0"), cli(d, "--depth-scale", "-1"), cli(d, "--shading", "phong"),
        cli(d, mode="part"),                                                          # the queries are missing
        cli(d, "--clip-query", str(d / "narrow.npy"), "--sbert-query", str(d / "s.npy"), mode="object"),
        ["--logdir", str(d / "nothing"), "--out", "o", "--mode", "rgb", "--pose", str(d / "pose.txt"), "--size", "7", "5",
         "--intrinsics", "1", "1", "0", "0"],
        cli(d, "--config", str(d / "nothing.json"), pose=None),
        ["--logdir", str(d), "--out", "o", "--mode", "rgb", "--pose", str(d / "pose.txt"), "--size", "0", "5",
         "--intrinsics", "1", "1", "0", "0"],
    ]
    for argv in bad:
        with pytest.raises(SystemExit):
            map_raster._parse(argv)
    capsys.readouterr()


def test_map_query_still_parses_as_before(logdir, capsys):
    d = logdir
    base = ["--logdir", str(d), "--out", str(d / "q"), "--clip-query", str(d / "c.npy"), "--sbert-query", str(d / "s.npy"),
            "--part-query", str(d / "p.npy")]
    a, all_obj, q = map_query._parse(base + ["--mode", "part", "--regions", "--region-frac", "0.5"])
    assert a.regions and a.region_frac == 0.5 and list(all_obj) == [10, 13] and sorted(q) == ["clip_query", "part_query", "sbert_query"]
    a, _, q = map_query._parse(base + ["--mode", "object"])
    assert sorted(q) == ["clip_query", "sbert_query"] and a.top is None and a.device == "cuda:0" and not a.compact
    for argv in (base + ["--mode", "rgb", "--regions"], base + ["--mode", "partfeat"],
                 ["--logdir", str(d), "--out", "o", "--mode", "part"]):
        with pytest.raises(SystemExit):
            map_query._parse(argv)
    capsys.readouterr()
