"""Object bounds from keyframes on the GPU (sceneObject.get_bound, vmap.py:287-384; objnerf_bounds.hip) against the
numpy statement in tests/bound_util.py, analytic shapes and the mapping loop end to end."""
import os

import numpy as np
import pytest
import torch

from openobj_amd import bounds, ops, synthetic
from openobj_amd import cfg as ocfg
from openobj_amd import vmap as ovmap
try:
    from tests import bound_util as BU
    from tests import scene_files as SF
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import bound_util as BU
    import scene_files as SF

pytestmark = pytest.mark.gpu


def _store_cloud(o):
    """The statement's raw cloud of a keyframe-store object (slots 0 .. n_keyframes-1)."""
    nk = o.n_keyframes
    st = o.rgbs_batch[:nk, :, :, 3].cpu().numpy()
    d = o.depth_batch[:nk].cpu().numpy()
    t = o.t_wc_batch[:nk].cpu().numpy()
    return BU.object_points(d, st, t, nk, o.intrinsics)


def _lex(idx, cen):
    o = np.lexsort(idx.T[::-1])
    return idx[o], cen[o]


def _check_voxels(o, got, voxel=0.05):
    idx_w, cen_w = BU.voxel_down(_store_cloud(o), voxel)
    idx_g, cen_g = _lex(*got)
    assert np.array_equal(idx_g, idx_w)
    assert np.abs(cen_g - cen_w).max(initial=0) <= 1e-12


def _rand_rot(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q * np.sign(np.linalg.det(q))


def test_voxel_centroids_match_the_statement(dev):
    """5 objects in one call: different n_keyframes (a full ring, none), states 0 / 1 / 2, depth 0 and NaN; 300 columns
    (two column chunks) and a 70-row image (a partial row band)."""
    rs = np.random.RandomState(0)
    F, W, H = 6, 300, 70
    intr = (150.0, 140.0, 149.5, 34.5)
    objs = []
    for k, nk in enumerate([1, 3, F, 5, 0]):
        o = synthetic.KeyframeObject(dev, F, W, H, intr, nk)
        st = rs.choice([0, 1, 2], size=(F, W, H), p=[0.3, 0.5, 0.2]).astype(np.uint8)
        d = rs.uniform(0.5, 4.0, (F, W, H)).astype(np.float32)
        d[rs.rand(F, W, H) < 0.05] = 0.0
        d[rs.rand(F, W, H) < 0.05] = np.nan
        t = np.tile(np.eye(4, dtype=np.float32), (F, 1, 1))
        for f in range(F):
            t[f, :3, :3] = _rand_rot(rs)
            t[f, :3, 3] = rs.randn(3)
        o.rgbs_batch[..., 3] = torch.from_numpy(st).to(dev)
        o.depth_batch.copy_(torch.from_numpy(d).to(dev))
        o.t_wc_batch.copy_(torch.from_numpy(t).to(dev))
        objs.append(o)
    vox = ops.objects_voxels(objs)
    assert len(vox[4][0]) == 0
    for o, got in zip(objs, vox):
        _check_voxels(o, got)
    # a tiny chunk budget (one object per chunk) gives the same bytes
    vox2 = ops.objects_voxels(objs, budget=1)
    for a, b in zip(vox, vox2):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _run_lengths(rs, m):
    """Seeded run lengths 1 .. 7 that sum to m (the last one cut to fit)."""
    ln = rs.randint(1, 8, size=m)
    ln = ln[:int(np.searchsorted(np.cumsum(ln), m)) + 1]
    ln[-1] -= ln.sum() - m
    return ln


@pytest.mark.parametrize("tile", [1024, 4096])
def test_heads_scan_carries_across_tiles(dev, tile):
    """objnerf_voxel_heads + objnerf_voxel_centroids called directly on tile * 1024 + 1029 sorted keys: tile + 2 head
    blocks of 1024 keys, so a one-workgroup scan of the block counts in tiles of `tile` elements carries from its first
    tile into a second (4096 = objnerf_wg.h's 1024 threads x 4 elements; 1024 = a tile of one element a thread).
    One run straddles a block boundary (keys 1022 .. 1025), one the tile boundary (keys 1024 tile - 2 .. + 2).
    Integer coordinates: the fp64 sums are exact, every output is compared bit for bit."""
    from openobj_amd._lib import check, lib
    rs = np.random.RandomState(7)
    B, n = 1024, tile * 1024 + 1029
    t0 = tile * B - 2
    ln = np.concatenate([_run_lengths(rs, 1022), [4], _run_lengths(rs, t0 - 1026), [5], _run_lengths(rs, n - t0 - 5)])
    assert ln.sum() == n and ln.min() >= 1 and ln.max() <= 7
    V = len(ln)
    start = np.concatenate([[0], np.cumsum(ln)[:-1]])
    assert 1022 in start and t0 in start
    local = np.cumsum(rs.randint(1, 4, size=V)).astype(np.int64)            # ascending voxel keys with gaps
    group = np.repeat(np.array([0, 2, 3], np.int64), [V // 3, V // 3, V - 2 * (V // 3)])    # group 1 has no key
    keys = np.repeat((group << 42) | local, ln)
    pts = rs.randint(-8, 9, size=(n, 3)).astype(np.float64)
    head = np.zeros(n, np.int64)
    head[start] = 1
    nb = (n + B - 1) // B
    blk = np.add.reduceat(head, np.arange(0, n, B))
    assert nb == tile + 2 and blk.sum() == V
    keys_d, pts_d = torch.from_numpy(keys).to(dev), torch.from_numpy(pts).to(dev)
    perm_d = torch.arange(n, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert int(lib().objnerf_voxel_heads_workspace_bytes(n)) == 8 * (nb + 1)
    ws = torch.full((nb + 1,), -1, dtype=torch.int64, device=dev)
    check(lib().objnerf_voxel_heads(n, keys_d.data_ptr(), ws.data_ptr(), st), "objnerf_voxel_heads")
    ws_h = ws.cpu().numpy()
    assert np.array_equal(ws_h[:nb], np.cumsum(blk) - blk)
    assert ws_h[nb] == V
    cen = torch.empty(V, 3, dtype=torch.float64, device=dev)
    vkeys = torch.empty(V, dtype=torch.int64, device=dev)
    first = torch.full((4,), -1, dtype=torch.int64, device=dev)
    check(lib().objnerf_voxel_centroids(n, keys_d.data_ptr(), perm_d.data_ptr(), pts_d.data_ptr(), ws.data_ptr(), V,
                                        cen.data_ptr(), vkeys.data_ptr(), first.data_ptr(), st), "objnerf_voxel_centroids")
    uniq = np.unique(keys)
    assert np.array_equal((group << 42) | vkeys.cpu().numpy(), uniq) and np.array_equal(uniq & ((1 << 42) - 1), local)
    want = np.add.reduceat(pts, start, axis=0) / ln[:, None].astype(np.float64)
    assert np.array_equal(cen.cpu().numpy(), want)
    assert first.cpu().numpy().tolist() == [0, -1, V // 3, 2 * (V // 3)]


def test_search_matches_the_statement(dev):
    rs = np.random.RandomState(1)
    clouds = [rs.randn(50, 3) * [0.5, 0.3, 0.1], rs.randn(600, 3) * [1.0, 0.4, 0.3], rs.randn(3000, 3)]
    for n in (2000, 2500):                                      # every point a hull vertex (2500: tiled through LDS)
        s = rs.randn(n, 3)
        clouds.append(s / np.linalg.norm(s, axis=1, keepdims=True) * [0.7, 0.4, 0.3])
    clouds = [c @ _rand_rot(rs).T + rs.randn(3) * 3 for c in clouds]
    flat = np.concatenate([rs.rand(300, 2) * [0.6, 0.2], np.zeros((300, 1))], axis=1) @ _rand_rot(rs).T + 1.0
    clouds.append(flat)
    problems = [bounds.hull_problem(c) for c in clouds]
    assert len(problems[4]["verts"]) == 2500 and problems[-1]["mode"] == 1
    got = bounds.obb_search(problems, dev)
    for c, g in zip(clouds, got):
        R, ext, ctr = g
        Rw, extw, cw = BU.oriented_bounds(c)
        crit = lambda e: np.prod(np.sort(e)[1:]) if min(e) == 0 else np.prod(e)      # flat: the area
        assert crit(ext) == pytest.approx(crit(extw), rel=1e-9)
        assert BU.box_contains(R, ext, ctr, c, 1e-9)
    again = bounds.obb_search(problems, dev)
    for a, b in zip(got, again):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ analytic cuboid
CUBOID = np.array([0.60, 0.40, 0.25])
W3, H3, F3 = 160, 120, 150.0


def _cfg(dev, root="", **kw):
    over = {"dataset.path": str(root), "dataset.format": "Replica", "trainer.part_mode": 0, "camera.w": SF.W,
            "camera.h": SF.H, "camera.fx": SF.FX, "camera.fy": SF.FY, "camera.cx": SF.CX, "camera.cy": SF.CY,
            "render.iters_per_frame": 30, "render.n_per_optim_bg": 240, "render.depth_range": [0.0, 8.0]}
    over.update(kw)
    return ocfg.Config(ocfg.replica_room0_config(train_device=str(dev), **over))


def _look_at(pos, target):
    z = target - pos
    z /= np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, :3] = np.stack([x, np.cross(z, x), z], axis=1)
    T[:3, 3] = pos
    return T.astype(np.float32)


def _render_cuboid(Rb, C, twc):
    """z-depth [H, W] of the cuboid (axes Rb columns, extents CUBOID, centre C) seen from twc (0 = missed)."""
    cx, cy = (W3 - 1) / 2.0, (H3 - 1) / 2.0
    jj, ii = np.meshgrid(np.arange(W3), np.arange(H3))
    dc = np.stack([(jj - cx) / F3, (ii - cy) / F3, np.ones_like(jj, dtype=np.float64)], axis=-1)
    T = twc.astype(np.float64)
    dw = dc @ T[:3, :3].T
    ob = Rb.T @ (T[:3, 3] - C)
    db = dw @ Rb
    h = CUBOID / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-h - ob) / db, (h - ob) / db
    tn = np.nanmax(np.minimum(t1, t2), axis=-1)
    tf = np.nanmin(np.maximum(t1, t2), axis=-1)
    hit = (tn < tf) & (tn > 0)
    return np.where(hit, tn, 0.0).astype(np.float32)


def _cuboid_object(dev, Rb, C, obj_id=1):
    c = _cfg(dev, **{"camera.w": W3, "camera.h": H3, "camera.fx": F3, "camera.fy": F3, "camera.cx": (W3 - 1) / 2.0,
                     "camera.cy": (H3 - 1) / 2.0, "model.keyframe_step": 10})      # / stride 10: every frame
    dirs = [(1, 0.3, 0.2), (-1, 0.2, -0.3), (0.2, 1, 0.3), (0.3, -1, -0.2), (-0.2, 0.3, 1), (0.3, -0.2, -1)]
    so = None
    for f, dvec in enumerate(dirs):
        pos = C + 1.5 * np.asarray(dvec) / np.linalg.norm(dvec)
        twc = _look_at(pos, C)
        depth = _render_cuboid(Rb, C, twc)                               # [H, W]
        assert (depth > 0).sum() > 500
        mask = torch.from_numpy((depth > 0).T.astype(np.uint8)).to(dev)
        rgb = torch.zeros(W3, H3, 3, dtype=torch.uint8, device=dev)
        args = (rgb, torch.from_numpy(np.ascontiguousarray(depth.T)).to(dev), mask, torch.zeros(4, device=dev),
                torch.from_numpy(twc).to(dev))
        if so is None:
            so = ovmap.sceneObject(c, obj_id, *args, f)
        else:
            so.append_keyframe(*args, frame_id=f)
    assert so.n_keyframes == 6
    return so


def _cuboid_pose(seed):
    rs = np.random.RandomState(seed)
    return _rand_rot(rs), np.array([0.3, -0.2, 2.5]) + rs.randn(3) * 0.2


def test_analytic_cuboid(dev):
    Rb, C = _cuboid_pose(2)
    so = _cuboid_object(dev, Rb, C)
    b3, b = so.get_bound()
    order = np.argsort(CUBOID)                                           # the box's extents are ascending
    for q in range(3):
        cos = abs(float(b.R[:, q] @ Rb[:, order[q]]))
        assert cos > np.cos(np.radians(3.0)), (q, np.degrees(np.arccos(min(1.0, cos))))
    np.testing.assert_allclose(b.extent, CUBOID[order], atol=0.05)
    assert np.linalg.norm(b.center - C) < 0.03
    assert abs(np.linalg.det(b.R) - 1) < 1e-9 and b.points3d.shape == (8, 3)
    assert so.bbox3dour is b and so.bbox3d is b3 and not so.bbox_final


def _reset(o):
    o.bbox_final, o.bbox3dour, o.bbox3d, o._computed_bound = False, None, None, None


def _box_bytes(b):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in (b.center, b.R, b.extent, b.points3d))


def test_batched_equals_single_and_is_reproducible(dev):
    objs = [_cuboid_object(dev, *_cuboid_pose(s), obj_id=s) for s in (3, 4, 5)]
    batched = [b for _, b in ovmap.get_bounds(objs)]
    for o in objs:
        _reset(o)
    single = [o.get_bound()[1] for o in objs]
    for o in objs:
        _reset(o)
    again = [b for _, b in ovmap.get_bounds(objs)]
    for a, s, g in zip(batched, single, again):
        assert _box_bytes(a) == _box_bytes(s) == _box_bytes(g)


def test_assigned_and_loaded_boxes_are_kept(dev, tmp_path):
    Rb, C = _cuboid_pose(6)
    so = _cuboid_object(dev, Rb, C)
    mine = type("Box", (), {})()
    mine.center, mine.R, mine.extent = np.zeros(3), np.eye(3), np.ones(3)
    so.bbox3dour = mine
    assert so.get_bound()[1] is mine and ovmap.get_bounds([so])[0][1] is mine and so.bbox3dour is mine
    _reset(so)
    _, b = so.get_bound(final=True)
    assert so.bbox_final and so.get_bound()[1] is b                       # final: cached
    d = tmp_path / "ck"
    d.mkdir()
    so.save_checkpoints(str(d), 0)
    _reset(so)
    so.load_checkpoints(str(d / ("obj_%d.pth" % so.obj_id)))
    loaded = so.bbox3dour
    assert so.bbox_final and _box_bytes(loaded) == _box_bytes(b)
    assert so.get_bound()[1] is loaded


def test_files_to_map_bounds_and_meshes_without_hand_made_boxes(dev, tmp_path):
    """The planar helper scene: IncrementalMapper.run, compute_bounds, render_view inside the computed boxes, and the
    checkpoints -> map_vis.export with no manual step."""
    from openobj_amd import dataset as ods
    from openobj_amd import map_vis, mapping
    from openobj_amd import render_view as orv
    root = tmp_path / "scene"
    SF.write_scene(str(root), "Replica", n_frames=50)
    c = _cfg(dev, root, **{"render.iters_per_frame": 80})
    torch.manual_seed(5)
    m = mapping.IncrementalMapper(c)
    m.run(ods.init_loader(c, multi_worker=False))
    boxes = m.compute_bounds()
    assert sorted(boxes) == [0, 4, 7]
    for oid, depth in ((4, 1.5), (7, 2.0)):
        so = m.vis_dict[oid]
        b = boxes[oid][1]
        assert b is so.bbox3dour
        assert b.extent[0] == pytest.approx(0.10) and abs(abs(b.R[2, 0]) - 1) < 1e-6        # flat, normal along z
        assert abs(b.center[2] - depth) < 0.03
        P = _store_cloud(so)                                              # union of the keyframes' footprints
        assert np.abs(P[:, 2] - depth).max() < 1e-6
        want = np.sort(np.ptp(P[:, :2], axis=0))
        np.testing.assert_allclose(np.sort(b.extent[1:]), want, atol=0.06)
    rgb, depth_mm, inst = SF._frame(4, None)                              # the last frame (index 40), [H, W]
    cam_x = 0.02 * 4
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = cam_x
    buf = orv.render_view(m.vis_dict, T, m.cam_info.rays_dir_cache, bg_ids=(0,))
    got = buf.rgb.transpose(1, 0, 2).astype(np.float64)
    inner = np.zeros(inst.shape, bool)
    for k in (4, 7):
        ys, xs = np.nonzero(inst == k)
        inner[ys.min() + 3:ys.max() - 2, xs.min() + 3:xs.max() - 2] = True
    mse = ((got - rgb.astype(np.float64))[inner] ** 2).mean()
    psnr = 10 * np.log10(255.0 ** 2 / mse)
    assert psnr > 28.0, psnr
    assert (buf.maskid.T[inner] == inst[inner]).mean() > 0.95
    log = tmp_path / "log"
    m.save_checkpoints(str(log), need_bound=True)
    out = map_vis.export(str(log), grid_dim=64, device=str(dev))
    for oid in (4, 7):
        ck = torch.load(str(log / "ckpt" / str(oid) / ("obj_%d.pth" % oid)), weights_only=False)
        b = ck["bbox"]
        assert b is not None and os.path.exists(log / "map_vis" / ("obj_%d.ply" % oid))
        v = np.asarray(out[oid]["mesh"].vertices, np.float64)
        assert len(v) > 0
        # Trainer.meshing's 64^3 grid spans the box scaled by 1 / bound_extent (0.9 for an object, trainer.py:25-28,51):
        # every vertex lies in that grid, within one cell
        loc = (v - b.center) @ np.asarray(b.R)
        half = np.asarray(b.extent) / (2 * 0.9)
        assert (np.abs(loc) <= half + 2 * half / 63 + 1e-6).all()


def test_native_shape(dev):
    """51 objects x 20 keyframes of 1200 x 680 in one compute call, under the 2 GiB workspace bound; the background and
    one object against the statement."""
    objs = synthetic.native_bound_map(dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    stats = {}
    res = ops.object_bounds(objs, stats=stats)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < 2 << 30, extra
    assert all(b is not None for _, b in res)
    vox = ops.objects_voxels(objs[:1] + objs[7:8])
    for o, got in zip([objs[0], objs[7]], vox):
        _check_voxels(o, got)
