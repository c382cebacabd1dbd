"""GPU: objnerf_meshcull.hip against the numpy restatements of tests/mapcull_util.py (checked on their own, on the CPU, by
tests/test_mapcull.py), EXACTLY -- both sides are the same fp64 operations in the same order, or integers -- and
openobj_amd/map_cull.py and map_eval's --cull-config end to end.  Outputs are written into buffers with guard rows on
both sides; every call is made twice and must write the same bytes."""
import json
import os

import numpy as np
import pytest
import torch

import mapcull_util as U
import scene_files as SF
from conftest import T
from openobj_amd import _lib, cfg, map_cull, map_eval, mesh, ops

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = -77
GRID_CAP_THREADS = 4096 * 256           # VV_GRID_CAP x CULL_WG of objnerf_meshcull.hip: above it a thread takes a second vertex


def guarded(shape, dev):
    buf = torch.full((shape[0] + 2 * GUARD,) + tuple(shape[1:]), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + shape[0]]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------ vertex views
def gpu_views(dev, verts, T_CW, depth, intr, start=None, **kw):
    """Two calls into guarded buffers (the counts are ADDED to `start`, zeros by default) -> int32 [V]."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    dv, dt, dd = T(verts).to(dev), T(np.asarray(T_CW, np.float64).reshape(-1, 3, 4)).to(dev), T(np.asarray(depth, np.float32)).to(dev)
    outs = []
    for _ in range(2):
        buf, out = guarded((len(verts),), dev)
        out[:] = 0 if start is None else T(np.asarray(start, np.int32)).to(dev)
        assert ops.vertex_views(dv, dt, dd, intr, out=out, **kw) is out
        assert guards_intact(buf)
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


def check_views(dev, verts, T_CW, depth, intr, **kw):
    got = gpu_views(dev, verts, T_CW, depth, intr, **kw)
    want = U.views_ref(verts, T_CW, depth, intr, **kw)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    return got


NONFINITE = np.array([[np.nan, 0, 3], [0, np.nan, 3], [0, 0, np.nan], [np.inf, 0, 3], [0, -np.inf, 3], [0, 0, np.inf],
                      [0, 0, -np.inf], [np.inf, np.inf, np.inf], [1e300, 1e300, 1e300], [-1e300, 0, 1e300], [1e30, 1e30, 1e-300],
                      [np.nan, np.nan, np.nan], [1e300, 0, 1.0], [0, -1e300, 2.0]], np.float64)


def random_case(seed, V, B, W=37, H=23, intr=(41.0, 33.0, 17.6, 11.2)):
    """Rotated and translated poses, depth with zeros, and vertices back-projected through real-valued pixels of some
    frame (a few pixels outside the image included) at 0.5 .. 1.5 x the measured depth or behind the camera; for V > 1
    the non-finite rows overwrite the head of the array."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = intr
    nb = max(B, 1)
    T_WC = np.tile(np.eye(4), (nb, 1, 1))
    for b in range(nb):
        a, bb, c = rng.uniform(-0.4, 0.4, 3)
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(bb), 0, np.sin(bb)], [0, 1, 0], [-np.sin(bb), 0, np.cos(bb)]])
        Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        T_WC[b, :3, :3] = Rx @ Ry @ Rz
        T_WC[b, :3, 3] = rng.uniform(-0.5, 0.5, 3)
    depth = rng.uniform(1.0, 4.0, (nb, W, H)).astype(np.float32)
    depth[rng.random((nb, W, H)) < 0.15] = 0.0
    f = rng.integers(0, nb, V)
    u, v = rng.uniform(-4.0, W + 3.0, V), rng.uniform(-4.0, H + 3.0, V)
    d = depth[f, np.clip(np.rint(u), 0, W - 1).astype(int), np.clip(np.rint(v), 0, H - 1).astype(int)].astype(np.float64)
    z = np.where(d > 0, d, 2.0) * rng.choice([0.5, 0.9, 1.0, 1.01, 1.03, 1.5, -1.0], V)
    pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    verts = np.einsum("nij,nj->ni", T_WC[f, :3, :3], pc) + T_WC[f, :3, 3]
    k = min(V, len(NONFINITE)) if V > 1 else 0
    verts[:k] = NONFINITE[:k]
    return verts, U.to_cw(T_WC[:B]), depth[:B], intr


@pytest.mark.parametrize("V", [0, 1, 64 * 1024 + 5, GRID_CAP_THREADS + 77])
def test_views_sizes_at_one_frame(dev, V):
    verts, T_CW, depth, intr = random_case(V, V, 1)
    got = check_views(dev, verts, T_CW, depth, intr)
    if V > 1000:
        assert 0.1 < (got > 0).mean() < 0.9 and not got[:len(NONFINITE)].any()
        assert got[-50:].any()                                  # the vertices past the grid cap were visited too


def test_views_no_frames(dev):
    verts, T_CW, depth, intr = random_case(1, 300, 0)
    assert T_CW.shape == (0, 3, 4) and depth.shape == (0, 37, 23)
    start = np.arange(300, dtype=np.int32)
    assert np.array_equal(gpu_views(dev, verts, T_CW, depth, intr, start=start), start)


def test_views_batches_accumulate(dev):
    verts, T_CW, depth, intr = random_case(2, 5000, 5)
    whole = check_views(dev, verts, T_CW, depth, intr)
    assert whole.max() >= 2 and (whole == 0).any()
    acc = np.zeros(5000, np.int32)
    for b0, b1 in ((0, 2), (2, 4), (4, 5)):
        acc = gpu_views(dev, verts, T_CW[b0:b1], depth[b0:b1], intr, start=acc)
    assert np.array_equal(acc, whole)


def test_views_wrapper_chunks_long_batches(dev, monkeypatch):
    verts, T_CW, depth, intr = random_case(3, 3000, 5)
    whole = check_views(dev, verts, T_CW, depth, intr)
    monkeypatch.setattr(ops, "VIEWS_MAX_BATCH", 2)
    assert np.array_equal(gpu_views(dev, verts, T_CW, depth, intr), whole)


@pytest.mark.parametrize("margin", [0, 3])
def test_views_margin_z_min_and_eps(dev, margin):
    verts, T_CW, depth, intr = random_case(4 + margin, 20000, 3)
    a = check_views(dev, verts, T_CW, depth, intr, margin=margin)
    b = check_views(dev, verts, T_CW, depth, intr, margin=margin, z_min=1.7, eps=0.0)
    assert (b <= a).all() and (b < a).any()
    if margin:
        assert (a <= U.views_ref(verts, T_CW, depth, intr)).all() and (a < U.views_ref(verts, T_CW, depth, intr)).any()


def test_views_boundaries_of_the_scene_camera(dev):
    """The single-vertex facts of tests/test_mapcull.py, the plane and the non-finite rows on the scene's four frames."""
    T_WC, depth = U.scene_depth(4)
    T_CW = U.to_cw(T_WC)
    bv, want, names = U.boundary_vertices()
    got = check_views(dev, bv, T_CW[:1], depth[:1], U.INTR)
    assert [n for n, g, w in zip(names, got > 0, want) if g != w] == []
    m2 = np.stack([U.backproject(1, 20, 3.0), U.backproject(2, 20, 3.0), U.backproject(61, 20, 3.0), U.backproject(62, 20, 3.0),
                   U.backproject(40, 1, 3.0), U.backproject(40, 2, 3.0), U.backproject(40, 45, 3.0), U.backproject(40, 46, 3.0)])
    assert check_views(dev, m2, T_CW[:1], depth[:1], U.INTR, margin=2).tolist() == [0, 1, 1, 0, 0, 1, 1, 0]
    plane = U.plane(3.0)[0]
    allv = np.concatenate([bv, NONFINITE, plane, m2])
    got = check_views(dev, allv, T_CW, depth, U.INTR)
    pv = got[len(bv) + len(NONFINITE):][:len(plane)]
    assert np.bincount(pv, minlength=5).tolist() == [4839, 317, 355, 359, 3539]
    assert not got[len(bv):len(bv) + len(NONFINITE)].any()
    assert not check_views(dev, U.plane(3.06)[0], T_CW, depth, U.INTR).any()


def test_views_non_square_depth_index(dev):
    W, H = 7, 5
    depth = 1.0 + np.arange(W * H, dtype=np.float32).reshape(1, W, H)
    intr = (10.0, 12.0, 3.0, 2.0)
    iu, iv = [x.ravel().astype(np.float64) for x in np.meshgrid(np.arange(W), np.arange(H), indexing="ij")]
    d = depth[0].ravel().astype(np.float64)
    on = np.stack([(iu - 3.0) * d / 10.0, (iv - 2.0) * d / 12.0, d], 1)
    behind = np.stack([(iu - 3.0) * (d + 0.5) / 10.0, (iv - 2.0) * (d + 0.5) / 12.0, d + 0.5], 1)
    got = check_views(dev, np.concatenate([on, behind]), U.to_cw(np.eye(4)[None]), depth, intr, eps=0.25)
    assert got.tolist() == [1] * 35 + [0] * 35


def test_views_rejects_bad_input(dev):
    verts, T_CW, depth, intr = random_case(5, 10, 2)
    v, t, d = T(verts).to(dev), T(T_CW).to(dev), T(depth).to(dev)
    ops.vertex_views(v, t, d, intr)
    for bad in (lambda: ops.vertex_views(v.cpu(), t, d, intr), lambda: ops.vertex_views(v, t.cpu(), d, intr),
                lambda: ops.vertex_views(v, t, d.cpu(), intr), lambda: ops.vertex_views(v.float(), t, d, intr),
                lambda: ops.vertex_views(v, t.float(), d, intr), lambda: ops.vertex_views(v, t, d.double(), intr),
                lambda: ops.vertex_views(v, t, d[:1], intr), lambda: ops.vertex_views(v, t, d[0], intr),
                lambda: ops.vertex_views(v[:, :2], t, d, intr), lambda: ops.vertex_views(v, t[:, :, :3], d, intr),
                lambda: ops.vertex_views(v, t, d, intr, margin=-1),
                lambda: ops.vertex_views(v, t, d, intr, out=torch.zeros(11, dtype=torch.int32, device=dev)),
                lambda: ops.vertex_views(v, t, d, intr, out=torch.zeros(10, dtype=torch.int64, device=dev))):
        with pytest.raises(_lib.ObjnerfError):
            bad()


# -------------------------------------------------------------------------------------------------------- compaction
KEYS = ("new_of_old", "old_of_new", "faces", "face_old")


def check_compact(dev, keep, faces, rule):
    keep, faces = np.asarray(keep).astype(np.uint8).reshape(-1), np.asarray(faces, np.int64).reshape(-1, 3)
    want = U.compact_ref(keep, faces, rule)
    assert not want["bad"]
    dk, df = T(keep).to(dev), T(faces.astype(np.int32)).to(dev)
    bufs = {k: guarded(want[k].shape, dev) for k in KEYS}
    got = ops.mesh_compact(dk, df, rule, out={k: b[1] for k, b in bufs.items()})
    again = ops.mesh_compact(dk.bool(), df, rule)              # fresh tensors; a bool mask
    for k in KEYS:
        assert guards_intact(bufs[k][0]), k
        g = got[k].cpu().numpy()
        assert g.dtype == np.int32 and g.shape == want[k].shape and np.array_equal(g, want[k]), (rule, k)
        assert np.array_equal(again[k].cpu().numpy(), g), k
    return want


@pytest.mark.parametrize("rule", ["all", "any"])
def test_compact_everything_and_nothing(dev, rule):
    v, f = U.grid_mesh(20, 30, 0, 1, 0, 1, 0)
    r = check_compact(dev, np.ones(len(v)), f, rule)
    assert np.array_equal(r["new_of_old"], np.arange(len(v))) and np.array_equal(r["faces"], f)
    r = check_compact(dev, np.zeros(len(v)), f, rule)
    assert len(r["old_of_new"]) == 0 and len(r["face_old"]) == 0 and (r["new_of_old"] == -1).all()
    for keep in ([1], [0]):
        r = check_compact(dev, keep, np.zeros((0, 3)), rule)   # V = 1, F = 0
        assert r["new_of_old"].tolist() == [-1]
    check_compact(dev, np.zeros(0), np.zeros((0, 3)), rule)    # V = F = 0


@pytest.mark.parametrize("rule", ["all", "any"])
def test_compact_random_mask_on_a_grid(dev, rule):
    v, f = U.plane()
    keep = np.random.default_rng(0).random(len(v)) < (0.8 if rule == "all" else 0.1)
    r = check_compact(dev, keep, f, rule)
    assert 0 < len(r["face_old"]) < len(f) and 0 < len(r["old_of_new"]) < len(v)
    assert np.array_equal(r["old_of_new"][r["faces"]], f[r["face_old"]])
    T_WC, depth = U.scene_depth(4)
    keep = U.views_ref(v, U.to_cw(T_WC), depth, U.INTR) >= 1
    r = check_compact(dev, keep, f, rule)
    assert (len(r["old_of_new"]), len(r["face_old"])) == ((4570, 8600) if rule == "all" else (5106, 9678))


@pytest.mark.parametrize("rule", ["all", "any"])
def test_compact_strip_across_three_scan_tiles(dev, rule):
    """A triangle strip whose per-workgroup totals (2051 workgroups of 256 for the vertices, and for the faces) span three
    tiles of the one-workgroup scan (256 x WG_SCAN_ITEMS = 1024 totals a tile); kept runs of 1000 out of every 1777 cross
    workgroup and tile boundaries."""
    V = 2 * 1024 * 256 + 600
    i = np.arange(V - 2)
    f = np.stack([i, i + 1, i + 2], 1)
    keep = (np.arange(V) % 1777) < 1000
    keep[256 * 1024 - 3:256 * 1024 + 3] = True                  # a run across the first tile boundary
    keep[2 * 256 * 1024 - 300:] = True                          # and one from the second tile into the third, to the end
    r = check_compact(dev, keep, f, rule)
    assert r["old_of_new"][-1] == V - 1 and r["face_old"][-1] == V - 3
    assert len(r["old_of_new"]) > 256 * 1024 and len(r["face_old"]) > 256 * 1024


@pytest.mark.parametrize("rule", ["all", "any"])
def test_compact_unused_vertices_repeated_and_degenerate_faces(dev, rule):
    rng = np.random.default_rng(1)
    V = 700
    f = rng.integers(0, 400, (900, 3))                          # vertices 400 .. 699 belong to no face
    f[10] = f[9]                                                # a repeated face
    f[20] = [5, 5, 9]                                           # degenerate faces
    f[21] = [7, 7, 7]
    keep = rng.random(V) < 0.7
    keep[[5, 9, 7]] = True
    keep[f[9]] = True
    r = check_compact(dev, keep, f, rule)
    assert {9, 10, 20, 21} <= set(r["face_old"].tolist())
    assert (r["new_of_old"][400:] == -1).all() and keep[400:].any()
    j = np.flatnonzero(r["face_old"] == 20)[0]
    assert r["faces"][j, 0] == r["faces"][j, 1] != r["faces"][j, 2]


@pytest.mark.parametrize("rule", ["all", "any"])
def test_compact_face_outside_the_vertices_raises(dev, rule):
    v, f = U.grid_mesh(9, 9, 0, 1, 0, 1, 0)
    keep = np.random.default_rng(2).random(len(v)) < 0.6
    good = check_compact(dev, keep, f, rule)
    dk = T(keep.astype(np.uint8)).to(dev)
    for row, val in ((17, len(v)), (40, -1), (0, 2 ** 31 - 1), (127, -2 ** 31)):
        bad = f.copy()
        bad[row, 1] = val
        with pytest.raises(_lib.ObjnerfError, match="outside"):
            ops.mesh_compact(dk, T(bad.astype(np.int32)).to(dev), rule)
    # with the offending faces removed the result is the restated one again
    bad = np.concatenate([f[:17], [[0, len(v), 1]], f[17:], [[-1, 0, 1]]])
    with pytest.raises(_lib.ObjnerfError, match="outside"):
        ops.mesh_compact(dk, T(bad.astype(np.int32)).to(dev), rule)
    r = check_compact(dev, keep, np.delete(bad, [17, len(bad) - 1], axis=0), rule)
    assert all(np.array_equal(r[k], good[k]) for k in KEYS)
    with pytest.raises(_lib.ObjnerfError):
        ops.mesh_compact(dk, T(f.astype(np.int64)).to(dev), rule)
    with pytest.raises(_lib.ObjnerfError):
        ops.mesh_compact(dk, T(f.astype(np.int32)).to(dev)[:, :2], rule)


@pytest.mark.parametrize("rule", ["all", "any"])
def test_compact_two_meshes_back_to_back(dev, rule):
    rng = np.random.default_rng(3)
    (va, fa), (vb, fb) = U.grid_mesh(23, 17, 0, 1, 0, 1, 0), U.grid_mesh(31, 29, 0, 1, 0, 1, 1)
    ka, kb = rng.random(len(va)) < 0.7, rng.random(len(vb)) < 0.5
    both = check_compact(dev, np.concatenate([ka, kb]), np.concatenate([fa, fb + len(va)]), rule)
    a, b = U.compact_ref(ka, fa, rule), U.compact_ref(kb, fb, rule)
    nv = np.searchsorted(both["old_of_new"], [0, len(va), len(va) + len(vb)])
    nf = np.searchsorted(both["face_old"], [0, len(fa), len(fa) + len(fb)])
    assert nv.tolist() == [0, len(a["old_of_new"]), len(a["old_of_new"]) + len(b["old_of_new"])]
    assert nf.tolist() == [0, len(a["face_old"]), len(a["face_old"]) + len(b["face_old"])]
    assert np.array_equal(both["old_of_new"][nv[1]:] - len(va), b["old_of_new"])
    assert np.array_equal(both["faces"][:nf[1]], a["faces"]) and np.array_equal(both["faces"][nf[1]:] - nv[1], b["faces"])


# --------------------------------------------------------------------------------------------------------- end to end
def scene_json(root, path):
    d = cfg.replica_room0_config(**{
        "dataset.path": str(root), "dataset.format": "Replica", "trainer.part_mode": 0, "camera.w": SF.W, "camera.h": SF.H,
        "camera.fx": SF.FX, "camera.fy": SF.FY, "camera.cx": SF.CX, "camera.cy": SF.CY})
    with open(path, "w") as fh:
        json.dump(d, fh)
    return str(path)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The scene_files Replica scene, 50 files = 5 frames at the config's stride 10; its config; the frames as loaded."""
    root = tmp_path_factory.mktemp("mapcull_scene")
    SF.write_scene(str(root / "data"), "Replica", n_frames=50)
    T_WC, depth = U.scene_depth(5, as_loaded=True)
    return {"config": scene_json(root / "data", root / "scene.json"), "T_CW": U.to_cw(T_WC), "depth": depth}


def f32(v):
    return np.asarray(v, np.float32).astype(np.float64)        # what a .ply holds


# a closed box in front of and behind the wall, between the two objects of the scene: its front is seen, its back is not
BOX = ([-0.06, -0.4, 2.5], [0.1, 0.3, 3.5])


def the_meshes():
    return {3: U.plane(3.0), 8: mesh.TriMesh(*U.box_mesh(*BOX)), 11: U.plane(3.2)}


def restated_cull(meshes, scene, sl=slice(None), min_views=1, rule="all", **kw):
    """{id: (v, f)} -> ({id: (v, f)} culled, {id: old_of_new}, {id: views}), by views_ref and compact_ref per mesh."""
    out, back, views = {}, {}, {}
    for k, m in meshes.items():
        v, f = map_cull._as_mesh(m)
        views[k] = U.views_ref(v, scene["T_CW"][sl], scene["depth"][sl], U.INTR, **kw)
        r = U.compact_ref(views[k] >= min_views, f, rule)
        out[k], back[k] = (v[r["old_of_new"]], r["faces"].astype(np.int64)), r["old_of_new"].astype(np.int64)
    return out, back, views


@pytest.mark.parametrize("rule,min_views", [("all", 1), ("any", 3)])
def test_count_views_and_cull_equal_the_restated_pipeline(dev, scene, rule, min_views):
    meshes = the_meshes()
    batches = list(map_cull.frame_batches(scene["config"], batch=2))
    assert [len(t) for t, _ in batches] == [2, 2, 1]           # a ragged last batch
    views, n = map_cull.count_views(meshes, batches, U.INTR, device=dev)
    want, back, wviews = restated_cull(meshes, scene, min_views=min_views, rule=rule)
    assert n == 5 and list(views) == [3, 8, 11]
    for k in meshes:
        assert views[k].dtype == np.int32 and np.array_equal(views[k], wviews[k])
    got, old = map_cull.cull(meshes, views, min_views, rule, device=dev)
    for k in meshes:
        assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), k
        assert np.array_equal(old[k], back[k]) and got[k][1].dtype == np.int64 and got[k][0].dtype == np.float64
    assert 0 < len(got[3][1]) < len(meshes[3][1]) and 0 < len(got[8][1]) < 12
    assert got[11][0].shape == (0, 3) and got[11][1].shape == (0, 3)          # 0.2 m behind the wall: returned empty
    # several dicts at once: one pass, the same numbers
    two, n2 = map_cull.count_views([{1: meshes[3]}, {1: meshes[8], 2: meshes[11]}], batches, U.INTR, device=dev)
    assert n2 == 5 and np.array_equal(two[0][1], views[3]) and np.array_equal(two[1][1], views[8])
    assert np.array_equal(two[1][2], views[11])


def test_command_line_writes_culled_meshes_and_report(dev, scene, tmp_path):
    src, dst = tmp_path / "in", tmp_path / "out"
    os.makedirs(src)
    meshes = the_meshes()
    colours = {}
    for k, m in meshes.items():
        v, f = map_cull._as_mesh(m)
        tm = mesh.TriMesh(v, f)
        if k != 8:                                              # object 8 has no colours
            colours[k] = np.stack([np.arange(len(v)) % 251, np.arange(len(v)) // 251, np.full(len(v), k), np.full(len(v), 255)],
                                  1).astype(np.uint8)
            tm.visual.vertex_colors = colours[k]
        tm.export(str(src / f"obj_{k}.ply"))
    res = map_cull.main(["--config", scene["config"], "--in", str(src), "--out", str(dst), "--stride", "2", "--eps", "0.03",
                         "--margin", "1", "--face-rule", "any", "--device", str(dev)])
    held = {k: (f32(map_cull._as_mesh(m)[0]), map_cull._as_mesh(m)[1]) for k, m in meshes.items()}
    want, back, _ = restated_cull(held, scene, sl=slice(0, None, 2), rule="any", eps=0.03, margin=1)
    rep = json.load(open(dst / "cull.json"))
    assert rep == res and rep["frames"] == 3
    assert rep["parameters"] == {"z_min": 0.0, "eps": 0.03, "margin": 1, "min_views": 1, "face_rule": "any", "stride": 2}
    for k in meshes:
        v, _, rgba, f = mesh.read_ply(str(dst / f"obj_{k}.ply"))
        assert np.array_equal(v.astype(np.float64), want[k][0]) and np.array_equal(f, want[k][1]), k
        assert rep["objects"][str(k)] == {"vertices": [len(held[k][0]), len(want[k][0])], "faces": [len(held[k][1]), len(want[k][1])]}
        if k in colours:
            assert np.array_equal(rgba, colours[k][back[k]])
        else:
            assert rgba is None
    assert 0 < rep["objects"]["3"]["faces"][1] < rep["objects"]["3"]["faces"][0] and rep["objects"]["11"]["faces"][1] == 0


def test_map_eval_with_cull_config_equals_compare_on_the_restated_meshes(dev, scene, tmp_path, monkeypatch):
    a, b = tmp_path / "run_a", tmp_path / "run_b"
    box = U.box_mesh(*BOX)
    sides = {a: {3: U.plane(3.0), 8: box, 11: U.plane(3.2)}, b: {3: U.plane(3.02), 8: box, 5: U.plane(2.9)}}
    for d, ms in sides.items():
        os.makedirs(d / "map_vis")
        for k, (v, f) in ms.items():
            mesh.TriMesh(v, f).export(str(d / "map_vis" / f"obj_{k}.ply"))
    gv, gf = U.plane(3.01)
    mesh.TriMesh(gv, gf).export(str(tmp_path / "scene.ply"))
    real, samples = map_eval.compare, []

    def spy(*args, **kw):
        r = real(*args, return_samples=True, **kw)
        samples.append(r.pop("samples"))
        return r

    monkeypatch.setattr(map_eval, "compare", spy)
    args = ["--logdir", str(a), "--ref-logdir", str(b), "--gt-scene", str(tmp_path / "scene.ply"), "--samples", "400",
            "--scene-samples", "600", "--thresholds", "0.1", "--seed", "3", "--device", str(dev)]
    map_eval.main(args + ["--cull-config", scene["config"], "--cull-min-views", "2"])
    got = json.load(open(a / "eval_geometry.json"))
    held = [{k: (f32(v), f) for k, (v, f) in sides[d].items()} for d in (a, b)] + [{0: (f32(gv), gf)}]
    pred, other, whole = (restated_cull(h, scene, min_views=2)[0] for h in held)
    kw = dict(n_samples=400, thresholds=[0.1], seed=3, n_scene_samples=600, device=dev)
    want = [real(pred, other, return_samples=True, **kw), real(pred, whole, per_object=False, return_samples=True, **kw)]
    assert len(samples) == 2
    for s, w in zip(samples, want):
        assert s["samp_off"] == w["samples"]["samp_off"] and s["face_off"] == w["samples"]["face_off"]
        for k in ("pts", "tri", "verts", "faces"):
            assert torch.equal(s[k], w["samples"][k]), k
    assert sorted(got["objects"]) == ["3", "8"] and got["missing_gt"] == [] and got["missing_pred"] == [5]    # 11 is empty now
    for k in ("3", "8"):
        for name, val in want[0]["objects"][int(k)].items():
            assert got["objects"][k][name] == pytest.approx(val, rel=1e-12, abs=0), (k, name)
    for name, val in want[0]["scene"].items():
        assert got["scene"][name] == pytest.approx(val, rel=1e-12, abs=0), name
    for name, val in want[1]["scene"].items():
        assert got["scene_vs_gt_scene"][name] == pytest.approx(val, rel=1e-12, abs=0), name
    c = got["cull"]
    assert c["frames"] == 5 and c["parameters"] == {"z_min": 0.0, "eps": 0.05, "margin": 0, "min_views": 2, "face_rule": "all",
                                                    "stride": 1}
    for name, h, r in zip(("pred", "other", "gt_scene"), held, (pred, other, whole)):
        assert c[name]["vertices"] == [sum(len(m[0]) for m in h.values()), sum(len(m[0]) for m in r.values())]
        assert c[name]["faces"] == [sum(len(m[1]) for m in h.values()), sum(len(m[1]) for m in r.values())]
        assert c[name]["faces"][1] < c[name]["faces"][0]
    # without the option: exactly the keys of before, and every mesh whole
    map_eval.main(args)
    plain = json.load(open(a / "eval_geometry.json"))
    assert sorted(plain) == sorted(["objects", "scene", "missing_pred", "missing_gt", "n_samples", "n_scene_samples", "thresholds",
                                    "seed", "scene_vs_gt_scene"])
    assert plain["missing_gt"] == [11] and plain["missing_pred"] == [5]
    assert samples[2]["faces"].shape[0] > samples[0]["faces"].shape[0]
