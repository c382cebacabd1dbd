"""openobj_amd.map_volume on the GPU against the specification of tests/mapvolume_util.py: every volume is integer and has
one right answer, so every comparison is for equality.

Shapes: no axis is a multiple of a tile (8 for reach, 32 outputs / 64 sources for the distance passes) or of 64; 70 is longer
than a wavefront and than a source chunk, on each axis in turn; one shape has an axis of length 1; (19, 17, 21) spans three
reach tiles per axis."""
import functools

import numpy as np
import pytest
import torch

import mappoints_util as U
import mapvolume_util as V
from openobj_amd import _lib, cfg as ocfg
from openobj_amd import map_points, map_volume, ops, trainer, utils

pytestmark = pytest.mark.gpu

BIG = (19, 17, 21)
SHAPES = [BIG, (70, 5, 3), (5, 70, 3), (3, 5, 70), (1, 9, 11), (13, 13, 13)]


def volume(label, dev, voxel=0.1, origin=(0.0, 0.0, 0.0), K=4):
    nz, ny, nx = label.shape
    return map_volume.MapVolume(None, origin, voxel, (nx, ny, nz), device=dev, label=label, obj_ids=list(range(K)))


def host(t):
    return t.cpu().numpy()


def check_clearance(label, dev):
    vol = volume(label, dev)
    d2, site = vol.clearance()
    rd2, rsite = V.clearance(label)
    assert d2.dtype == torch.int32 and site.dtype == torch.int32
    assert np.array_equal(host(d2), rd2)
    assert np.array_equal(host(site), rsite)
    return vol


# ------------------------------------------------------------------------------------------------------------ labels
def _trainer(obj, dev):
    c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev)))
    c.obj_id, c.hidden_feature_size, c.clip_point_feature_size = int(obj["obj_id"]), int(obj["hidden"]), 512
    c.obj_scale = float(obj["scale"])
    t = trainer.Trainer(c)
    with torch.no_grad():
        for q, v in zip(t.fc_occ_map.parameters(), obj["p"]):
            q.copy_(v.to(dev))
        t.pe.B_layer.weight.copy_(obj["B"].to(dev))
    return t


def _map(objs, dev):
    def box(o):
        b = utils.BoundingBox()
        b.center, b.R, b.extent = o["center"].copy(), o["R"].copy(), o["extent"].copy()
        return b
    return map_points.MapPoints([map_points.MapObject(_trainer(o, dev), box(o), o["obj_id"], o["class_id"], o["obj_center"])
                                 for o in objs], device=dev, bg_ids=(0,))


# the grid of the label tests: 13^3 voxels of 0.2 m over the cube the scenes' clouds fill, its origin moved off the round
# value by an offset chosen so that few centres are ambiguous for the specification or near a box face
LABEL_DIMS, LABEL_VOXEL, LABEL_ORIGIN = (13, 13, 13), 0.2, (-1.3 + 0.013, -1.3 + 0.007, -1.3 - 0.011)


@functools.lru_cache(maxsize=None)
def label_reference(scene):
    """The specification's labels of the grid's centres (the oracle, on the CPU) and the voxels left out of the comparison."""
    objs = U.main_scene()[0] if scene == "main" else U.background_scene(128)[0]
    centres = V.centres(LABEL_ORIGIN, LABEL_VOXEL, LABEL_DIMS)
    cand = U.candidate_mask(centres, objs)
    alpha, _, _ = U.oracle_eval(centres, objs, want_feat=False)
    spec = U.label_spec(alpha, cand, [o["obj_id"] == 0 for o in objs])
    ext = min(float(np.min(o["extent"])) for o in objs)
    near = torch.zeros(len(centres), dtype=torch.bool)
    for o in objs:
        l, half = U.box_locals(centres, o, torch.float64)
        near |= (l.abs() - half).abs().min(dim=1).values < U.FACE_MARGIN * ext
    return objs, centres, spec["obj"].numpy(), (spec["ambiguous"] | near).numpy()


@pytest.mark.parametrize("scene", ["main", "background128"])
def test_labels(dev, scene):
    objs, centres, spec_obj, excluded = label_reference(scene)
    # a condition of the comparison, on the specification alone
    assert excluded.mean() <= U.AMBIGUOUS_CAP, f"{excluded.sum()} of {len(excluded)} voxels excluded"
    mp = _map(objs, dev)
    vol = map_volume.MapVolume(mp, LABEL_ORIGIN, LABEL_VOXEL, LABEL_DIMS)
    got_centres = host(vol.centres())
    assert np.array_equal(got_centres.view(np.uint32), centres.view(np.uint32))
    assert np.array_equal(host(vol.centres(5, 3)), centres.reshape(13, 169, 3)[5:8].reshape(-1, 3))
    label = vol.voxelise(slab_points=4 * 169)                       # four planes a slab: 4, 4, 4, 1
    assert label.dtype == torch.int32 and tuple(label.shape) == (13, 13, 13)
    direct = mp.label(torch.from_numpy(centres).to(dev))["obj"]
    assert torch.equal(label.view(-1), direct)
    lab = host(label).reshape(-1)
    assert np.array_equal(lab[~excluded], spec_obj[~excluded])
    assert (lab >= 0).any() and (lab < 0).any()
    assert vol.obj_ids.tolist() == [o["obj_id"] for o in objs] and vol.class_ids.tolist() == [o["class_id"] for o in objs]


# --------------------------------------------------------------------------------------------------------- clearance
@pytest.mark.parametrize("density", [0.02, 0.3, 0.9])
@pytest.mark.parametrize("dims", SHAPES)
def test_clearance_random(dev, dims, density):
    check_clearance(V.random_grid(dims, density, seed=int(density * 100) + dims[0]), dev)


@pytest.mark.parametrize("dims", [BIG, (70, 5, 3), (1, 9, 11)])
def test_clearance_empty_full_corner(dev, dims):
    nx, ny, nz = dims
    vol = check_clearance(np.full((nz, ny, nx), -1, np.int32), dev)
    assert int(vol.dist2.min()) == V.INT32_MAX and int(vol.site.max()) == -1
    vol = check_clearance(np.zeros((nz, ny, nx), np.int32), dev)
    assert int(vol.dist2.max()) == 0 and np.array_equal(host(vol.site).reshape(-1), np.arange(nx * ny * nz))
    for corner in (0, nx * ny * nz - 1):
        label = np.full((nz, ny, nx), -1, np.int32)
        label.reshape(-1)[corner] = 2
        vol = check_clearance(label, dev)
        assert int(vol.dist2.max()) == (nx - 1) ** 2 + (ny - 1) ** 2 + (nz - 1) ** 2


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_clearance_projected(dev, axis):
    label = V.random_grid(BIG, 0.02, seed=5)
    vol = volume(label, dev)
    flat = vol.project(axis)
    want = V.project(label, axis)
    assert flat.dims[axis] == 1 and tuple(flat.label.shape) == want.shape
    assert np.array_equal(host(flat.label), want)
    d2, site = flat.clearance()
    rd2, rsite = V.clearance(want)
    assert np.array_equal(host(d2), rd2) and np.array_equal(host(site), rsite)


# ------------------------------------------------------------------------------------------------------------- reach
def start_of(vol, label, rd2, r2, near):
    """The world centre of the traversable voxel closest in index to `near`."""
    trav = np.nonzero(V.traversable(label, rd2, r2).reshape(-1))[0]
    u = int(trav[np.abs(trav - near).argmin()])
    return u, V.centres(vol.origin, vol.voxel, vol.dims, [u])[0]


def check_reach(label, dev, radius, near, voxel=0.1):
    vol = volume(label, dev, voxel=voxel)
    rd2, rsite = V.clearance(label)
    r2 = map_volume.radius_to_r2(radius, float(vol.voxel))
    u, start = start_of(vol, label, rd2, r2, near)
    stats = {}
    vol.reach(start, radius, stats=stats)
    assert vol.start_voxel == u and vol.r2 == r2
    want = V.reach(label, rd2, r2, u)
    got = vol.cost_u32()
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    print(f"reach {vol.dims} r2 {r2}: {stats['rounds']} rounds in {stats['batches']} batches, cap {stats['round_cap']}, "
          f"{int((want != V.INF_COST).sum())} of {stats['traversable']} traversable voxels reached")
    assert stats["rounds"] <= stats["round_cap"]
    return vol, want, (rd2, rsite, r2, u)


# r2 = 2: a voxel with an occupied face neighbour is closed.  At this density the specification reaches about half of the
# traversable voxels (asserted below, on the specification alone: a condition of the test, not a result)
HALF_DENSITY = 0.25


@pytest.mark.parametrize("dims", [BIG, (70, 5, 3), (1, 9, 11)])
def test_reach_random(dev, dims):
    density = HALF_DENSITY if dims == BIG else 0.1
    label = V.random_grid(dims, density, seed=21)
    vol, want, (rd2, _, r2, _) = check_reach(label, dev, 0.14, near=dims[0] * dims[1] * dims[2] // 2)
    assert r2 == 2
    if dims == BIG:
        frac = (want != V.INF_COST).sum() / V.traversable(label, rd2, r2).sum()
        assert 0.25 <= frac <= 0.75, frac


def test_reach_maze(dev):
    label = V.maze_grid(BIG)
    vol, want, _ = check_reach(label, dev, 0.0, near=0)
    far = want[BIG[2] - 1, BIG[1] - 1, BIG[0] - 1]
    # the straight way to the far corner is at most max(BIG) - 1 corner moves of 5; the maze doubles back between walls
    assert far != V.INF_COST and far > 2 * 5 * (max(BIG) - 1)


def test_reach_sealed_pocket(dev):
    label = V.pocket_grid(BIG)
    vol, want, _ = check_reach(label, dev, 0.0, near=0)
    nx, ny, nz = BIG
    inside = want[nz // 4 + 1:nz - nz // 4 - 1, ny // 4 + 1:ny - ny // 4 - 1, nx // 4 + 1:nx - nx // 4 - 1]
    assert inside.size > 0 and np.all(inside == V.INF_COST)
    assert np.all(vol.cost_u32()[nz // 4 + 1:nz - nz // 4 - 1, ny // 4 + 1:ny - ny // 4 - 1, nx // 4 + 1:nx - nx // 4 - 1]
                  == V.INF_COST)


def test_reach_radius_closes_a_gap(dev):
    # a wall across x = 9 with a gap of 3 x 3 voxels, whose middle is 2 voxels from the wall (dist2 = 4): radius 0 and 0.1 m
    # (r2 = 1) pass, 0.21 m (r2 = 5) does not fit
    nx, ny, nz = BIG
    label = np.full((nz, ny, nx), -1, np.int32)
    label[:, :, 9] = 1
    label[9:12, 7:10, 9] = -1
    far = (nz - 1, ny - 1, nx - 1)
    for radius, passes in ((0.0, True), (0.1, True), (0.21, False)):
        _, want, _ = check_reach(label, dev, radius, near=0)
        assert (want[far] != V.INF_COST) == passes, radius


def test_reach_start_raises(dev):
    label = V.random_grid(BIG, 0.3, seed=3)
    vol = volume(label, dev)
    occupied = int(np.nonzero(label.reshape(-1) >= 0)[0][0])
    with pytest.raises(_lib.ObjnerfError, match="not traversable"):
        vol.reach(V.centres(vol.origin, vol.voxel, vol.dims, [occupied])[0], 0.0)
    with pytest.raises(_lib.ObjnerfError, match="outside"):
        vol.reach((-0.05, 0.05, 0.05), 0.0)
    # free, but closer to an obstacle than the radius
    rd2, _ = V.clearance(label)
    tight = int(np.nonzero((label.reshape(-1) < 0) & (rd2.reshape(-1) < 4))[0][0])
    with pytest.raises(_lib.ObjnerfError, match="not traversable"):
        vol.reach(V.centres(vol.origin, vol.voxel, vol.dims, [tight])[0], 0.2)


# --------------------------------------------------------------------------------------------------- goals and paths
@pytest.fixture(scope="module")
def reached(dev):
    label = V.random_grid(BIG, 0.05, seed=8, K=5)
    label[label == 3] = -1                                       # object 3 occupies nothing: no goal
    vol, want, (rd2, rsite, r2, u) = check_reach(label, dev, 0.1, near=BIG[0] * BIG[1] * BIG[2] // 2)
    vol.obj_ids, vol.class_ids = np.arange(5), np.arange(5)
    return vol, label, rd2, rsite, want, r2, u


def test_goals(reached):
    vol, label, rd2, rsite, cost, r2, u = reached
    g = vol.goals()
    voxel, gd2, gc = V.goals(label, rd2, rsite, cost, r2, 5)
    assert np.array_equal(g["voxel"], voxel) and np.array_equal(g["dist2"], gd2) and np.array_equal(g["cost"], gc)
    assert voxel[3] == -1 and (voxel[[0, 1, 2, 4]] >= 0).all()
    has = voxel >= 0
    assert np.array_equal(g["position"][has], V.centres(vol.origin, vol.voxel, vol.dims, voxel[has]))
    assert np.isnan(g["position"][~has]).all()


def test_paths(reached):
    vol, label, rd2, rsite, cost, r2, u = reached
    voxel, _, _ = V.goals(label, rd2, rsite, cost, r2, 5)
    flat = cost.reshape(-1)
    far = int(np.where(flat == V.INF_COST, 0, flat).argmax())        # the costliest voxel: the longest walk
    unreached = int(np.nonzero(flat == V.INF_COST)[0][0])
    goals = [int(v) for v in voxel] + [far, u, unreached]
    paths = vol.paths(goals)
    for gv, p in zip(goals, paths):
        assert p.tolist() == V.path(label, rd2, cost, r2, gv), gv
        if gv < 0 or flat[gv] == V.INF_COST:
            assert len(p) == 0
            continue
        assert p[0] == gv and p[-1] == u
        x, y, z = p % BIG[0], (p // BIG[0]) % BIG[1], p // (BIG[0] * BIG[1])
        step = 2 + np.abs(np.diff(x)) + np.abs(np.diff(y)) + np.abs(np.diff(z))
        assert np.all((step >= 3) & (step <= 5))
        assert np.array_equal(flat[p[:-1]].astype(np.int64) - flat[p[1:]].astype(np.int64), step)
    assert len(paths[-2]) == 1 and len(paths[5]) > 10


def test_paths_small_buffer(dev, reached):
    vol, label, rd2, rsite, cost, r2, u = reached
    flat = cost.reshape(-1)
    far = int(np.where(flat == V.INF_COST, 0, flat).argmax())
    full = V.path(label, rd2, cost, r2, far)
    cap, G, guard = 4, 2, 16
    assert len(full) > cap
    buf = torch.full((G * cap + guard,), -7, dtype=torch.int32, device=dev)
    out, ln = vol.paths_raw([far, u], cap, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    assert host(ln).tolist() == [-len(full), 1]
    b = host(buf)
    assert b[:cap].tolist() == full[:cap] and b[cap] == u and np.all(b[cap + 1:2 * cap] == -7)
    assert np.all(b[G * cap:] == -7)                                   # the guard words
    out, ln = vol.paths_raw([far], len(full))                          # exactly enough
    assert host(ln).tolist() == [len(full)] and host(out)[0].tolist() == full


# --------------------------------------------------------------------------------------------------- reproducibility
def test_two_runs_same_bytes(dev):
    label = V.random_grid(BIG, HALF_DENSITY, seed=21)
    runs = []
    for _ in range(2):
        vol = volume(label, dev)
        d2, site = vol.clearance()
        rd2, _ = V.clearance(label)
        _, start = start_of(vol, label, rd2, 2, BIG[0] * BIG[1] * BIG[2] // 2)
        cost = vol.reach(start, 0.14)
        table = ops.volume_goals(vol.label, d2, site, cost, vol.dims, vol.r2, vol.K)
        runs.append([host(t).tobytes() for t in (d2, site, cost, table)])
    assert runs[0] == runs[1]
    # the batch size of the round loop changes how often the host looks, not what the rounds compute
    other = ops.volume_reach(vol.label, vol.dist2, vol.dims, vol.r2, vol.start_voxel, batch=3)
    assert host(other).tobytes() == runs[0][2]


# -------------------------------------------------------------------------------------------------------- end to end
def test_cli_from_checkpoints(dev, tmp_path, capsys):
    import json
    import os
    objs = U.reference("cli")["objs"]
    logdir, out1, out2 = tmp_path / "log", tmp_path / "out1", tmp_path / "out2"
    for o in objs:
        t = _trainer(o, dev)
        d = logdir / "ckpt" / str(o["obj_id"])
        os.makedirs(d)
        b = utils.BoundingBox()
        b.center, b.R, b.extent = o["center"].copy(), o["R"].copy(), o["extent"].copy()
        torch.save({"epoch": 0, "FC_state_dict": t.fc_occ_map.state_dict(), "PE_state_dict": t.pe.state_dict(),
                    "obj_id": o["obj_id"], "bbox": b, "obj_scale": t.obj_scale, "clip_feat": None, "caption_feat": None,
                    "semantic_id": o["class_id"]}, str(d / f"obj_{o['obj_id']}.pth"))
    common = ["--logdir", str(logdir), "--voxel", "0.2", "--bounds", "-1.3", "-1.3", "-1.3", "1.3", "1.3", "1.3",
              "--device", str(dev)]
    map_volume.main(common + ["--out", str(out1)])
    vol = map_volume.MapVolume.load(str(out1), device=dev)
    assert vol.dims == (13, 13, 13) and vol.obj_ids.tolist() == [o["obj_id"] for o in objs]
    label, d2 = host(vol.label), host(vol.dist2)
    rd2, rsite = V.clearance(label)
    assert np.array_equal(d2, rd2) and (label >= 0).any() and (label < 0).any()
    # the start: the free voxel farthest from every obstacle; radius 0.1 m at a voxel of 0.2 m is r2 = 1
    u = int(np.where(label.reshape(-1) < 0, rd2.reshape(-1), -1).argmax())
    start = V.centres(vol.origin, vol.voxel, vol.dims, [u])[0]
    ids = [objs[2]["obj_id"], objs[0]["obj_id"]]
    map_volume.main(common + ["--out", str(out2), "--radius", "0.1", "--start"] + [repr(float(v)) for v in start]
                    + ["--goal-ids"] + [str(i) for i in ids])
    capsys.readouterr()
    assert np.array_equal(np.load(out2 / "volume.npz")["label"], label)
    nav = json.load(open(out2 / "nav.json"))
    assert nav["r2"] == 1 and [o["id"] for o in nav["objects"]] == ids
    cost = V.reach(label, rd2, 1, u)
    voxel, gd2, gc = V.goals(label, rd2, rsite, cost, 1, len(objs))
    for rec, k in zip(nav["objects"], (2, 0)):
        assert rec["class"] == objs[k]["class_id"]
        if voxel[k] < 0:
            assert rec["goal"] is None and rec["cost"] is None and rec["path"] == []
            continue
        want = V.path(label, rd2, cost, 1, int(voxel[k]))[::-1]
        assert rec["cost"] == gc[k] and rec["clearance_m"] == float(np.sqrt(gd2[k]) * float(vol.voxel))
        assert np.array_equal(np.asarray(rec["goal"], np.float32), V.centres(vol.origin, vol.voxel, vol.dims, [voxel[k]])[0])
        assert np.array_equal(np.asarray(rec["path"], np.float32), V.centres(vol.origin, vol.voxel, vol.dims, want))
    assert any(rec["goal"] is not None for rec in nav["objects"])
