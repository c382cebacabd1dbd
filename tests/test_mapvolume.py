"""The navigation volume without a GPU: the specification of tests/mapvolume_util.py on shapes whose answer is known by
hand, and the host logic of openobj_amd.map_volume (the grid from boxes, r2, the limits, the npz round trip, the CLI's
argument errors)."""
import numpy as np
import pytest

import mapvolume_util as V
from openobj_amd import _lib, map_volume


# ------------------------------------------------------------------------------------------------- the specification
def test_spec_single_site_closed_form():
    dims = (7, 5, 3)
    label = np.full((3, 5, 7), -1, np.int32)
    label[1, 3, 2] = 0
    d2, site = V.clearance(label)
    x, y, z = V.coords(dims)
    assert np.array_equal(d2.reshape(-1), (x - 2) ** 2 + (y - 3) ** 2 + (z - 1) ** 2)
    assert np.all(site == (1 * 5 + 3) * 7 + 2)


def test_spec_equidistant_sites_take_the_lower_index():
    label = np.full((1, 1, 5), -1, np.int32)
    label[0, 0, 0] = 1
    label[0, 0, 4] = 0
    d2, site = V.clearance(label)
    assert d2.reshape(-1).tolist() == [0, 1, 4, 1, 0]
    assert site.reshape(-1).tolist() == [0, 0, 0, 4, 4]           # the middle voxel is 2 from both: index 0 wins
    # the same along y and z, where the lower index is the lower y / z
    for shape, far in (((1, 5, 1), 4), ((5, 1, 1), 4)):
        lab = np.full(shape, -1, np.int32)
        lab.reshape(-1)[0] = 0
        lab.reshape(-1)[far] = 0
        assert V.clearance(lab)[1].reshape(-1)[2] == 0


def test_spec_empty_grid_sentinels():
    d2, site = V.clearance(np.full((2, 3, 4), -1, np.int32))
    assert np.all(d2 == V.INT32_MAX) and np.all(site == -1)
    cost = V.reach(np.full((2, 3, 4), -1, np.int32), d2, 0, 0)
    assert cost.max() < V.INF_COST and cost.reshape(-1)[0] == 0


def test_spec_wall_with_one_gap():
    # 5 x 3 x 1: a wall at x = 2 over y = 0, 1, the gap at y = 2.  From (0, 0) to (4, 0): two rows up and two down in four
    # columns, so every one of the four moves is an edge move of 4
    label = np.full((1, 3, 5), -1, np.int32)
    label[0, 0:2, 2] = 0
    d2, site = V.clearance(label)
    cost = V.reach(label, d2, 0, 0)
    assert cost[0, 0, 4] == 16
    assert cost[0, 2, 2] == 8 and cost[0, 0, 1] == 3 and cost[0, 0, 2] == V.INF_COST
    p = V.path(label, d2, cost, 0, 4)
    assert p == [4, 1 * 5 + 3, 2 * 5 + 2, 1 * 5 + 1, 0]
    # a robot that needs dist2 >= 2 does not fit through the gap (its voxel is 1 from the wall)
    assert V.reach(label, d2, 2, 0)[0, 0, 4] == V.INF_COST
    voxel, gd2, gc = V.goals(label, d2, site, cost, 0, 2)
    assert voxel.tolist() == [1, -1] and gd2.tolist() == [1, -1] and gc.tolist() == [3, V.INF_COST]


def test_spec_project():
    label = np.full((2, 2, 3), -1, np.int32)
    label[1, 0, 2] = 5
    label[0, 1, 2] = 3
    label[0, 1, 0] = 7
    assert V.project(label, 0).reshape(2, 2).tolist() == [[-1, 7], [5, -1]]
    assert V.project(label, 2).reshape(2, 3).tolist() == [[-1, -1, 5], [7, -1, 3]]
    assert V.project(label, 1).shape == (2, 1, 3)


# ------------------------------------------------------------------------------------------------------ host logic
def test_grid_from_boxes_fp64():
    eye = np.eye(3)
    origin, dims = map_volume.grid_from_boxes([(0.1, 0.0, 0.0)], [eye], [(1.0, 2.0, 3.0)], 0.25, pad=0.05)
    assert dims == (5, 10, 14)
    assert origin.dtype == np.float64 and np.array_equal(origin, [-0.5, -1.25, -1.75])
    # a quarter turn about z swaps the x and y extents; two boxes give the hull of both
    rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    origin, dims = map_volume.grid_from_boxes([(0, 0, 0)], [rz], [(1.0, 2.0, 3.0)], 0.4)
    assert dims == (6, 4, 8) and np.allclose(origin, [-1.2, -0.8, -1.6])
    origin, dims = map_volume.grid_from_boxes([(0, 0, 0), (2.0, 0, 0)], [eye, eye], [(1, 1, 1), (1, 1, 1)], 0.5)
    assert dims == (6, 2, 2) and np.array_equal(origin, [-0.5, -0.5, -0.5])
    origin, dims = map_volume.grid_from_bounds([0.0, 0.0, 0.0, 1.0, 0.55, 0.1], 0.1)
    assert dims == (10, 6, 1) and np.array_equal(origin, [0, 0, 0])


def test_radius_to_r2():
    assert map_volume.radius_to_r2(0.0, 0.1) == 0
    assert map_volume.radius_to_r2(0.25, 0.1) == 7                # 2.5^2 = 6.25
    assert map_volume.radius_to_r2(0.2, 0.1) in (4, 5)            # fp64: (0.2 / 0.1)^2 may land just above 4
    assert map_volume.radius_to_r2(0.2, 0.1) == int(np.ceil((0.2 / 0.1) ** 2))
    assert map_volume.radius_to_r2(1.0, 0.5) == 4
    with pytest.raises(_lib.ObjnerfError):
        map_volume.radius_to_r2(-1.0, 0.1)
    with pytest.raises(_lib.ObjnerfError):
        map_volume.radius_to_r2(1e6, 1e-3)


def test_limits_raise():
    for dims in ((1025, 1, 1), (1, 0, 1), (1024, 1024, 1024 * 2), (4, 4)):
        with pytest.raises(_lib.ObjnerfError):
            map_volume.MapVolume(None, (0, 0, 0), 0.1, dims, device="cpu")
    with pytest.raises(_lib.ObjnerfError):
        map_volume.MapVolume(None, (0, 0, 0), 0.0, (4, 4, 4), device="cpu")
    with pytest.raises(_lib.ObjnerfError):
        map_volume.grid_from_boxes([(0, 0, 0)], [np.eye(3)], [(300.0, 1, 1)], 0.25)      # 1200 voxels along x
    with pytest.raises(_lib.ObjnerfError):
        map_volume.grid_from_bounds([0, 0, 0, 1, 0, 1], 0.1)
    v = map_volume.MapVolume(None, (0, 0, 0), 0.1, (1024, 1024, 1), device="cpu")
    assert v.n_voxels == 1 << 20 and v.shape == (1, 1024, 1024)
    with pytest.raises(_lib.ObjnerfError):
        v.set_label(np.zeros((1, 4, 4), np.int32))
    with pytest.raises(_lib.ObjnerfError):
        v.clearance()                                             # no labels yet


def test_voxel_of_and_centres():
    v = map_volume.MapVolume(None, (-0.3, 0.1, 2.0), 0.07, (5, 4, 3), device="cpu")
    idx = np.arange(v.n_voxels)
    c = v.position(idx)
    assert c.dtype == np.float32 and np.array_equal(c, V.centres((-0.3, 0.1, 2.0), 0.07, (5, 4, 3)))
    assert [v.voxel_of(p) for p in c.astype(np.float64)] == idx.tolist()
    assert v.voxel_of((-0.31, 0.2, 2.1)) == -1 and v.voxel_of((0.0, 0.2, 2.0 + 3 * 0.07 + 1e-3)) == -1


def test_npz_round_trip(tmp_path):
    label = V.random_grid((6, 5, 4), 0.3, seed=2)
    v = map_volume.MapVolume(None, (0.5, -1.0, 0.25), 0.125, (6, 5, 4), device="cpu", label=label, obj_ids=[0, 4, 9, 11],
                             class_ids=[0, 3, 3, -1])
    import torch
    v.dist2 = torch.from_numpy(V.clearance(label)[0])
    path = v.save(str(tmp_path))
    assert path.endswith("volume.npz")
    w = map_volume.MapVolume.load(str(tmp_path), device="cpu")
    assert w.dims == v.dims and w.voxel == v.voxel and np.array_equal(w.origin, v.origin)
    assert np.array_equal(w.label.numpy(), label) and np.array_equal(w.dist2.numpy(), v.dist2.numpy())
    assert w.obj_ids.tolist() == [0, 4, 9, 11] and w.class_ids.tolist() == [0, 3, 3, -1]
    assert w.site is None and w.cost is None


@pytest.mark.parametrize("argv", [
    ["--logdir", "x", "--out", "y"],                                              # no --voxel
    ["--logdir", "x", "--out", "y", "--voxel", "0"],
    ["--logdir", "x", "--out", "y", "--voxel", "0.1", "--radius", "0.2"],           # no --start
    ["--logdir", "x", "--out", "y", "--voxel", "0.1", "--start", "0", "0", "0"],    # no --radius
    ["--logdir", "x", "--out", "y", "--voxel", "0.1", "--project-axis", "3"],
    ["--logdir", "x", "--out", "y", "--voxel", "0.1", "--goal-ids", "3"],
    ["--logdir", "x", "--out", "y", "--voxel", "0.1", "--bounds", "0", "0", "0", "1", "1", "0"],
    ["--logdir", "x", "--out", "y", "--voxel", "0.1", "--radius", "-1", "--start", "0", "0", "0"],
])
def test_cli_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        map_volume.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_arguments():
    a = map_volume.parse_args(["--logdir", "x", "--out", "y", "--voxel", "0.1", "--radius", "0.25", "--start", "0", "1", "2",
                               "--goal-ids", "3", "7", "--project-axis", "2"])
    assert a.start == [0.0, 1.0, 2.0] and a.goal_ids == [3, 7] and a.project_axis == 2 and a.bounds is None
