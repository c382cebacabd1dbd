"""The cropped keyframe store on the GPU (kf_store.py; objnerf_ingest_frame_crops, objnerf_sample_rays_crops, the
`crops` form of objnerf_voxel_scan / objnerf_voxel_emit) against the dense store: whatever reads keyframes -- ingest,
the samplers, get_bound, the mapping loop -- gives the same bits from either kind."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from openobj_amd import _lib, mapping, ops
from openobj_amd import cfg as ocfg
from openobj_amd import dataset as ods
from openobj_amd import part_maps as pm
from openobj_amd import vmap as ovmap
from openobj_amd.kf_store import KeyframeCropStore, crop_rect, grown_cap
try:
    from tests import scene_files as SF
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import scene_files as SF

pytestmark = pytest.mark.gpu

W, H, F = 48, 40, 5
PD, PC = 4, 8                    # part maps: 12 x 10 x 8
N_FRAMES, N_PX = 6, 8
IDS = [4, 7, 9]

# per frame: object -> (instance rectangle: columns x0 .. x1, rows y0 .. y1 inclusive; its 2-D box)
OBJ4 = [((5, 9, 7, 12), (4.0, 10.0, 6.0, 13.0)),            # 7 x 8 px crop: the first capacity (256)
        ((4, 30, 6, 30), (3.0, 31.0, 5.0, 31.0)),           # 29 x 27 px: the arena grows
        ((4, 11, 6, 20), (3.7, 11.2, 5.5, 20.25))]          # a fractional box
OBJ4 += [((5 + i, 12 + i, 8, 18), (4.0 + i, 13.0 + i, 7.0, 19.0)) for i in range(3, 7)]
OBJ7 = [((31, 47, 26, 39), (30.0, 47.0, 25.0, 39.0)),       # ends at the last column and the last row
        ((33, 47, 27, 39), (32.5, 47.0, 26.25, 39.0))]
OBJ9 = {5: ((6, 8, 33, 35), (5.0, 9.0, 32.0, 36.0)),        # appears late: two keyframes
        6: ((7, 7, 34, 34), (7.0, 7.0, 34.0, 34.0))}        # a degenerate box: lo == hi on both axes


def _sample(i, narrow=False):
    rs = np.random.RandomState(100 + i)
    rgb = rs.randint(0, 256, (W, H, 3)).astype(np.uint8)
    depth = rs.uniform(1.0, 2.0, (W, H)).astype(np.float32)
    depth[rs.rand(W, H) < 0.05] = 0.0
    inst = np.ones((W, H), np.int32)                        # 1: a wall nobody gave a box
    inst[0:2, :] = -1                                       # an unknown strip
    boxes = {}
    per = {4: OBJ4[min(i, 6)], 7: OBJ7[i % 2]}
    if i in OBJ9 or i > 6:
        per[9] = OBJ9[min(i, 6)]
    if narrow:                                              # object 4's box is narrower than its instance
        per[4] = ((5, 20, 8, 18), (8.0, 15.0, 8.0, 18.0))
    for oid, ((x0, x1, y0, y1), box) in per.items():
        inst[x0:x1 + 1, y0:y1 + 1] = oid
        boxes[oid] = torch.tensor(box)
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = 0.05 * i
    f = lambda k, n: (np.eye(n)[k % n] + 0.01 * rs.randn(n)).astype(np.float32)
    return {"image": rgb, "depth": depth, "obj": inst, "T": T, "bbox_dict": boxes, "frame_id": 10 * i,
            "obj_clip": {k: f(k, 16)[None] for k in per}, "obj_cap": {k: f(k + 1, 12) for k in per},
            "part_feat": rs.randn(W // PD, H // PD, PC).astype(np.float32)}


def _cfg(dev, kind):
    over = {"camera.w": W, "camera.h": H, "camera.fx": 40.0, "camera.fy": 40.0, "camera.cx": 23.5, "camera.cy": 19.5,
            "model.keyframe_buffer_size": F, "model.keyframe_step": 10, "model.keyframe_step_bg": 10,
            "trainer.part_mode": 1, "trainer.part_down": PD, "model.keyframe_store": kind}
    return ocfg.Config(ocfg.replica_room0_config(train_device=str(dev), **over))


def _build(dev, kind, n=7):
    """A mapper with n frames ingested: every frame a keyframe, so the 5-slot rings of objects 4 and 7 fill and prune."""
    m = mapping.IncrementalMapper(_cfg(dev, kind))
    for i in range(n):
        m.ingest(_sample(i), i)
    return m


@pytest.fixture()
def oldest_pruned(monkeypatch):
    """Pruning is random in the reference; here both kinds drop the oldest entry."""
    monkeypatch.setattr(ovmap.sceneObject, "prune_keyframe", lambda self: list(self.kf_id_dict.items())[:-2][0])


@pytest.fixture(scope="module")
def pair(dev):
    """(dense mapper, crop mapper) after the same 7 frames; shared by the tests that only read the stores."""
    keep = ovmap.sceneObject.prune_keyframe
    ovmap.sceneObject.prune_keyframe = lambda self: list(self.kf_id_dict.items())[:-2][0]
    try:
        out = _build(dev, "dense"), _build(dev, "crop")
    finally:
        ovmap.sceneObject.prune_keyframe = keep
    torch.cuda.synchronize()
    return out


def _same_slots(md, mc):
    for oid in IDS:
        d, c = md.obj_dict[oid], mc.obj_dict[oid]
        assert d.crops is None and isinstance(c.crops, KeyframeCropStore) and not hasattr(c, "rgbs_batch")
        assert (c.n_keyframes, c.kf_pointer, c.kf_id_dict, c.lastest_kf_queue) == \
            (d.n_keyframes, d.kf_pointer, d.kf_id_dict, d.lastest_kf_queue)
        used = sorted(d.kf_id_dict.values())
        assert len(used) == (2 if oid == 9 else F)                # (a full ring keeps the pruned entry until it is rewritten)
        for slot in (used if oid == 9 else range(F)):           # (the rings of 4 and 7 have written every slot)
            x0, y0, cw, ch = crop_rect(d.bbox[slot], W, H)
            assert c.crops.rect[slot].tolist() == [x0, y0, cw, ch] == c.crops.rect_host[slot].tolist()
            rgbs, depth = c.crops.frame(slot)
            want = torch.zeros_like(d.rgbs_batch[slot])
            want[x0:x0 + cw, y0:y0 + ch] = d.rgbs_batch[slot, x0:x0 + cw, y0:y0 + ch]
            want_d = torch.zeros_like(d.depth_batch[slot])
            want_d[x0:x0 + cw, y0:y0 + ch] = d.depth_batch[slot, x0:x0 + cw, y0:y0 + ch]
            assert torch.equal(rgbs, want) and torch.equal(depth, want_d), (oid, slot)
            assert bool((d.rgbs_batch[slot, :, :, 3] == 1).sum() == (rgbs[..., 3] == 1).sum())    # no state-1 pixel lost
        assert torch.equal(c.t_wc_batch[used], d.t_wc_batch[used]) and torch.equal(c.bbox[used], d.bbox[used])
        assert c.crops.t_wc is c.t_wc_batch and c.crops.bbox is c.bbox


# ---------------------------------------------------------------------------------------------------------- ingest
def test_ingest_equals_dense_and_counts_lost_pixels(dev, oldest_pruned):
    md, mc = _build(dev, "dense"), _build(dev, "crop")
    assert list(md.obj_dict) == list(mc.obj_dict) == IDS and md.scene_bg is None
    _same_slots(md, mc)
    c4 = mc.obj_dict[4].crops
    # object 4: 56 px, then 783 px -> one growth to ceil(1.5 * 783 / 256) * 256, nothing larger afterwards
    assert (c4.cap, c4.version) == (grown_cap(29 * 27), 2) and grown_cap(7 * 8) == 256
    assert mc.obj_dict[7].crops.version == 1 and mc.obj_dict[9].crops.cap == 256
    assert list(mc._outside_ids) == IDS and mc._outside[:3].tolist() == [0, 0, 0]
    assert mc.store_bytes() == sum(F * mc.obj_dict[i].crops.cap * 8 for i in IDS) < md.store_bytes() == 3 * F * W * H * 8
    mc.compute_bounds()                                          # nothing lost: no complaint
    assert md._outside is None
    # one more frame whose box for object 4 is narrower than its instance
    s = _sample(7, narrow=True)
    md.ingest(s, 7)
    mc.ingest(s, 7)
    x0, y0, cw, ch = crop_rect(s["bbox_dict"][4], W, H)
    mine = s["obj"] == 4
    lost = int(mine.sum() - mine[x0:x0 + cw, y0:y0 + ch].sum())
    assert lost == 16 * 11 - 8 * 11
    assert mc._outside[:3].tolist() == [lost, 0, 0]
    slot = mc.obj_dict[4].kf_id_dict[70]
    rgbs, depth = mc.obj_dict[4].crops.frame(slot)
    d = md.obj_dict[4]
    assert torch.equal(rgbs[x0:x0 + cw, y0:y0 + ch], d.rgbs_batch[slot, x0:x0 + cw, y0:y0 + ch])
    assert torch.equal(depth[x0:x0 + cw, y0:y0 + ch], d.depth_batch[slot, x0:x0 + cw, y0:y0 + ch])
    with pytest.raises(ValueError, match=r"\{4: %d\}" % lost):
        mc.compute_bounds()
    with pytest.raises(ValueError):
        mc.save_checkpoints("unused")
    md.compute_bounds()                                          # the dense store holds the whole frame
    # a frame without object 4: the frame's items are no longer the first objects of the map, the counts are scattered
    s = _sample(8)
    s["obj"][s["obj"] == 4] = 1
    for key in ("bbox_dict", "obj_clip", "obj_cap"):
        del s[key][4]
    s["bbox_dict"][7] = torch.tensor((35.0, 47.0, 30.0, 39.0))
    mc.ingest(s, 8)
    x0, y0, cw, ch = crop_rect(s["bbox_dict"][7], W, H)
    mine = s["obj"] == 7
    lost7 = int(mine.sum() - mine[x0:x0 + cw, y0:y0 + ch].sum())
    assert lost7 > 0 and mc._outside[:3].tolist() == [lost, lost7, 0]


def test_pair_fixture_slots(pair):
    _same_slots(*pair)


# --------------------------------------------------------------------------------------------------------- sampler
def _part_sources(dev):
    """None, a dense [7, 12, 10, 8] map and a PartStore of 7 frames (tables of 3 .. 9 rows)."""
    rs = np.random.RandomState(5)
    dense = torch.from_numpy(rs.randn(7, W // PD, H // PD, PC).astype(np.float32)).to(dev)
    store = pm.PartStore(dev)
    for i in range(7):
        m = 3 + i
        store.append(torch.from_numpy(rs.randint(0, m + 1, (W // PD, H // PD)).astype(np.int32)),
                     torch.cat([torch.zeros(1, PC), torch.from_numpy(rs.randn(m, PC).astype(np.float32))]))
    return {"none": None, "dense": dense, "store": store}


def _eq(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _eq(x, y, (what, i))
    else:
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what


@pytest.mark.parametrize("part", ["none", "dense", "store"])
def test_samplers_equal_dense(dev, pair, monkeypatch, part):
    md, mc = pair
    src = _part_sources(dev)[part]
    od, oc = list(md.obj_dict.values()), list(mc.obj_dict.values())
    assert [o.n_keyframes for o in oc] == [4, 4, 2]              # the "latest two" rule on and off
    sd, sc = ovmap.StackedSampler(od), ovmap.StackedSampler(oc)
    assert sd.table.shape == (3, 4) and sc.table.shape == (3, 5)
    cache = md.cam_info.rays_dir_cache
    torch.manual_seed(11)
    draws = sd.draw(N_FRAMES, N_PX)
    draws["u_w"][:, 0, 0] = draws["u_h"][:, 0, 0] = 0.0                      # both ends of every box
    draws["u_w"][:, 1, 1] = draws["u_h"][:, 1, 1] = 1.0 - 2.0 ** -24
    assert int(draws["kf_ids"][2].max()) <= 1 and draws["kf_ids"][0, -2:].tolist() == od[0].lastest_kf_queue[-2:]
    # injected draws: stacked, then every object alone
    a, b = sd.sample(N_FRAMES, N_PX, cache, src, draws=draws), sc.sample(N_FRAMES, N_PX, cache, src, draws=draws)
    _eq(a, b, "stacked injected")
    assert (a[6] is None) == (part == "none") and bool(a[3].eq(1).any()) and bool(a[1].gt(0).any())
    for k in range(3):
        one = {key: v[k] for key, v in draws.items()}
        x = od[k].get_training_samples(N_FRAMES, N_PX, cache, src, draws=one)
        y = oc[k].get_training_samples(N_FRAMES, N_PX, cache, src, draws=one)
        _eq(x, y, ("single injected", k))
        for i in range(6):
            assert torch.equal(y[i].reshape(-1), b[i][k].reshape(-1)), (k, i)
    # seeded draws, with the record of what was drawn (out_kf, out_px); both point forms
    meta = torch.tensor([o.kf_meta() for o in od], dtype=torch.int32).to(dev)
    o0 = od[0]
    pf = lambda s_: s_._partfeat_args(src)
    for want_pts in (True, False):
        args = (F, W, H, cache)
        tail = (N_FRAMES, N_PX, o0.n_bins_cam2surface, o0.n_bins, o0.surface_eps, o0.stop_eps, float(o0.min_bound), 0.0)
        kw = dict(seed=77, draw=3, want_pts=want_pts, record=True)
        x = ops.sample_rays_seeded(sd.table, *args, meta, *tail, partfeat=pf(sd), **kw)
        y = ops.sample_rays_seeded(sc.table, *args, meta, *tail, partfeat=pf(sc), **kw)
        assert sorted(x) == sorted(y)
        for key in x:
            _eq(x[key], y[key], ("stacked seeded", key))
        assert x["kf"].shape == (3, N_FRAMES) and x["px"].shape == (3, N_FRAMES * N_PX, 2)
        for k in range(3):
            xs = ops.sample_rays_seeded(od[k].keyframe_store(), *args, meta[k], *tail, partfeat=od[k]._partfeat_args(src), **kw)
            ys = ops.sample_rays_seeded(oc[k].keyframe_store(), *args, meta[k], *tail, partfeat=oc[k]._partfeat_args(src), **kw)
            for key in xs:
                _eq(xs[key], ys[key], ("single seeded", k, key))
                _eq(ys[key], None if y[key] is None else y[key][k], ("single seeded is the stacked row", k, key))
    # the public seeded forms (their draw counter is per process: both kinds start from the same value)
    for compact in (False, True):
        monkeypatch.setattr(ops, "_draw_offset", [40])
        x = sd.sample(N_FRAMES, N_PX, cache, src, seed=5, compact=compact)
        xs = [o.get_training_samples(N_FRAMES, N_PX, cache, src, seed=5, compact=compact) for o in od]
        monkeypatch.setattr(ops, "_draw_offset", [40])
        y = sc.sample(N_FRAMES, N_PX, cache, src, seed=5, compact=compact)
        ys = [o.get_training_samples(N_FRAMES, N_PX, cache, src, seed=5, compact=compact) for o in oc]
        _eq(x, y, ("sample seeded", compact))
        _eq(xs, ys, ("get_training_samples seeded", compact))


def test_stacked_sampler_follows_a_moved_arena(dev, oldest_pruned):
    """A store that grows after the sampler was built: the table is rebuilt from the new arena by itself."""
    md, mc = _build(dev, "dense", n=1), _build(dev, "crop", n=1)
    sd, sc = ovmap.StackedSampler(md.obj_dict.values()), ovmap.StackedSampler(mc.obj_dict.values())
    before = sc.table.clone()
    for i in (1, 2):
        md.ingest(_sample(i), i)
        mc.ingest(_sample(i), i)                                 # frame 1: object 4's arena grows
    cache = md.cam_info.rays_dir_cache
    torch.manual_seed(3)
    draws = sd.draw(N_FRAMES, N_PX)
    _eq(sd.sample(N_FRAMES, N_PX, cache, None, draws=draws), sc.sample(N_FRAMES, N_PX, cache, None, draws=draws), "grown")
    assert int(sc.table[0, 1]) == grown_cap(29 * 27) > int(before[0, 1]) and not torch.equal(sc.table, before)
    with pytest.raises(ValueError):
        ovmap.StackedSampler([md.obj_dict[4], mc.obj_dict[7]])   # one kind per stack


# ---------------------------------------------------------------------------------------------------------- bounds
def test_bounds_equal_dense(dev, pair):
    md, mc = pair
    od, oc = list(md.obj_dict.values()), list(mc.obj_dict.values())
    sx, sy = {}, {}
    vd, vc = ops.objects_voxels(od, stats=sx), ops.objects_voxels(oc, stats=sy)
    assert sx["points"] == sy["points"] > 500 and sx["voxels"] == sy["voxels"] > 10
    assert sy["scan_bytes"] < sx["scan_bytes"]
    for (ia, ca), (ib, cb) in zip(vd, vc):
        assert np.array_equal(ia, ib) and ca.tobytes() == cb.tobytes()
    assert len(vd[0][0]) > 10 and len(vd[1][0]) > 10
    bd, bc = ovmap.get_bounds(od), ovmap.get_bounds(oc)
    assert bd[0][1] is not None and bd[1][1] is not None
    for (a3, a), (b3, b) in zip(bd, bc):
        for x, y in ((a3, b3), (a, b)):
            assert (x is None) == (y is None)
            if x is not None:
                for key in ("center", "R", "extent", "points3d"):
                    assert np.asarray(getattr(x, key)).tobytes() == np.asarray(getattr(y, key)).tobytes(), key


# ------------------------------------------------------------------------------------------------ mapper end to end
def _same(a, b, what):
    if torch.is_tensor(a):
        assert torch.equal(a, b), what
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), what
    elif isinstance(a, dict):
        assert list(a) == list(b), what
        for k in a:
            _same(a[k], b[k], (what, k))
    elif hasattr(a, "points3d"):
        _same(vars(a), vars(b), what)
    else:
        assert a == b, what


def test_mapping_crop_equals_dense(dev, tmp_path, monkeypatch):
    """The scene of tests/scene_files.py, 4 frames with part features, once per kind under the same seed (and the same
    per-process draw counter): identical parameters and checkpoints."""
    root = tmp_path / "scene"
    SF.write_scene(str(root), "Replica", n_frames=40, part_dim=512, part_down=4)     # (the networks' feature width)
    over = {"dataset.path": str(root), "dataset.format": "Replica", "trainer.part_mode": 1, "trainer.part_down": 4,
            "camera.w": SF.W, "camera.h": SF.H, "camera.fx": SF.FX, "camera.fy": SF.FY, "camera.cx": SF.CX,
            "camera.cy": SF.CY, "render.iters_per_frame": 10, "render.n_per_optim_bg": 240, "render.depth_range": [0.0, 8.0]}
    runs = {}
    for kind in ("dense", "crop"):
        c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev), **dict(over, **{"model.keyframe_store": kind})))
        torch.manual_seed(1234)
        monkeypatch.setattr(ops, "_draw_offset", [0])
        m = mapping.IncrementalMapper(c)
        m.run(ods.init_loader(c, multi_worker=False), n_frames=4)
        log = tmp_path / kind
        m.save_checkpoints(str(log), need_bound=True)
        runs[kind] = (m, {i: torch.load(str(log / "ckpt" / str(i) / ("obj_%d.pth" % i)), weights_only=False)
                          for i in m.vis_dict})
    (md, cd), (mc, cc) = runs["dense"], runs["crop"]
    assert list(md.obj_dict) == list(mc.obj_dict) == [4, 7] and sorted(cd) == sorted(cc) == [0, 4, 7]
    assert mc.scene_bg.crops is None and all(o.crops is not None for o in mc.obj_dict.values())
    assert torch.equal(md.loop.arena.params, mc.loop.arena.params)
    assert torch.equal(md.scene_bg.trainer.arena.params, mc.scene_bg.trainer.arena.params)
    for i in mc.vis_dict:
        assert torch.equal(md.vis_dict[i].trainer.arena.params, mc.vis_dict[i].trainer.arena.params)
        _same(cd[i], cc[i], i)
    assert cc[4]["bbox"] is not None and cc[7]["bbox"] is not None
    # the growth rule's own bound on what the crop run holds
    ds = ods.Replica(mc.cfg)
    biggest = {i: max(np.prod(crop_rect(ds[f]["bbox_dict"][i], SF.W, SF.H)[2:]) for f in range(4)) for i in (4, 7)}
    Fb = mc.cfg.keyframe_buffer_size
    bg = Fb * SF.W * SF.H * 8
    assert mc.store_bytes() <= sum(Fb * (1.5 * biggest[i] + 256) * 8 for i in (4, 7)) + bg
    assert md.store_bytes() == 3 * bg and mc.store_bytes() < md.store_bytes()
    assert mc._outside[:2].tolist() == [0, 0]


def test_command_line_option(dev, tmp_path):
    root = tmp_path / "scene"
    SF.write_scene(str(root), "Replica", n_frames=20)
    import json
    cfgd = ocfg.replica_room0_config(train_device=str(dev), **{
        "dataset.path": str(root), "dataset.format": "Replica", "trainer.part_mode": 0, "camera.w": SF.W, "camera.h": SF.H,
        "camera.fx": SF.FX, "camera.fy": SF.FY, "camera.cx": SF.CX, "camera.cy": SF.CY, "render.iters_per_frame": 2,
        "render.n_per_optim_bg": 240, "vis.if_ckpt": 0})
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfgd))
    m = mapping.main(["--config", str(path), "--logdir", str(tmp_path / "log"), "--frames", "2", "--single-worker",
                      "--keyframe-store", "crop"])
    assert m.cfg.keyframe_store == "crop" and all(o.crops is not None for o in m.obj_dict.values())
    assert m.scene_bg.crops is None and m.store_bytes() > 0


# ------------------------------------------------------------------------------------------------ argument checking
def test_new_entry_points_reject_bad_arguments(dev):
    lib = _lib.lib()
    z = torch.zeros(64, device=dev)
    zi = torch.full((8,), 7, dtype=torch.int32, device=dev)
    p = z.data_ptr()
    # objnerf_ingest_frame_crops: the status codes of objnerf_ingest_frame
    assert lib.objnerf_ingest_frame_crops(4, 4, None, None, None, None, 1, None, None, None) == -22
    assert lib.objnerf_ingest_frame_crops(4, 4, p, p, p, p, 0, p, zi.data_ptr(), None) == -22
    assert lib.objnerf_ingest_frame_crops(4, 4, p, p, p, p, 70000, p, zi.data_ptr(), None) == -22
    assert lib.objnerf_ingest_frame_crops(0, 4, p, p, p, p, 1, p, zi.data_ptr(), None) == -22
    assert lib.objnerf_ingest_frame_crops(4, 4, p, p, p, p, 1, p, None, None) == -22
    # objnerf_sample_rays_crops: those of objnerf_sample_rays_stacked
    a = _lib.SampleArgs()
    assert lib.objnerf_sample_rays_crops(C.byref(a), 1, None, None) == -22
    assert lib.objnerf_sample_rays_crops(C.byref(a), 1, p, None) == -22          # empty arguments
    assert lib.objnerf_sample_rays_crops(None, 1, p, None) == -22
    assert lib.objnerf_sample_rays_crops(C.byref(a), 0, p, None) == -22
    # objnerf_voxel_scan / emit: neither dense tables nor crops
    nb = int(lib.objnerf_voxel_workspace_bytes(1, 2, 8, 8))
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    v = _lib.VoxelArgs(1, 2, 8, 8, 1.0, 1.0, 0.0, 0.0, 0.05, None, p, p, None)
    assert lib.objnerf_voxel_scan(C.byref(v), ws.data_ptr(), nb, p, p, None) == -22
    assert lib.objnerf_voxel_emit(C.byref(v), ws.data_ptr(), nb, 0, 1, p, p, p, 4, p, p, None) == -22
    v = _lib.VoxelArgs(1, 2, 8, 8, 1.0, 1.0, 0.0, 0.0, 0.05, None, p, p, p)
    assert lib.objnerf_voxel_scan(C.byref(v), ws.data_ptr(), nb - 1, p, p, None) == -22
    torch.cuda.synchronize()
    assert bool((zi == 7).all()) and not bool(z.any())                           # nothing was launched
    # host-side checks of the wrappers
    st = KeyframeCropStore(3, 8, 6, dev)
    rgb = torch.zeros(8, 6, 3, dtype=torch.uint8, device=dev)
    depth = torch.ones(8, 6, device=dev)
    inst = torch.full((8, 6), 5, dtype=torch.int32, device=dev)
    twc = torch.eye(4, device=dev)
    out = torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.ObjnerfError):
        ops.keyframe_table([st])                                                 # no keyframe yet
    with pytest.raises(_lib.ObjnerfError):
        ops.ingest_frame_crops(rgb, depth, inst, twc, [(st, 3, 5, [0, 1, 2, 3])], out)      # slot out of range
    with pytest.raises(_lib.ObjnerfError):
        ops.ingest_frame_crops(rgb, depth[:, :5].contiguous(), inst, twc, [(st, 0, 5, [0, 1, 2, 3])], out)
    with pytest.raises(_lib.ObjnerfError):
        ops.ingest_frame_crops(rgb, depth, inst, twc, [(st, 0, 5, [0, 1, 2, 3])] * 3, out)  # more items than counters
    with pytest.raises(_lib.ObjnerfError):
        ops.ingest_frame_crops(rgb, depth, inst, twc, [(st, 0, 5, [0, 1, 2, 3])] * 2, out)  # one slot twice
    with pytest.raises(_lib.ObjnerfError):
        ops.ingest_frame_crops(rgb, depth, inst, twc, [(st, 0, 5, [0, 1, 2, 3])], out.long())
    ops.ingest_frame_crops(rgb, depth, inst, twc, [(st, 2, 5, [0, 7, 0, 5]), (st, 1, 9, [1.5, 2, 3, 4.5])], out)
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0] and st.rect.tolist() == [[0, 0, 0, 0], [1, 3, 2, 2], [0, 0, 8, 6]]
    assert bool((st.frame(2)[0][..., 3] == 1).all()) and not bool(st.frame(1)[0][..., 3].any())
    with pytest.raises(_lib.ObjnerfError):
        ops.keyframe_table([st, (rgb, depth, twc, twc)])                         # kinds mixed
