"""GPU: a whole map view in one launch chain (openobj_amd/map_view.py, objnerf_mapview.hip) against the code it
batches, stage by stage and bit for bit: the candidate rays against ops.box_rays, the segmented renderer against
ops.render_fwd, the whole view against render_view.render_view -- and, like test_render_view_per_pixel, against the
reference's merge in numpy (render_util.view_ref).  Views are 80 x 60."""
import numpy as np
import pytest
import torch

import render_util as R
from render_util import EXCLUDE_CAP, MARGIN, box, draws_for, make_net, view_ref, view_scene
from openobj_amd import map_view, ops, render_view, trainer
from openobj_amd import cfg as ocfg
from openobj_amd import vmap as ovmap

pytestmark = pytest.mark.gpu

BAR = 1e-4        # "1e-4 parity" of include/objnerf_hip.h, mode 0
ORDERS = ([1, 0, 2, 4, 3], [3, 4, 2, 0, 1], [0, 1, 2, 3, 4])


class SceneObj:
    """What render_2D_syn needs of a sceneObject: a trainer, a device and a box."""
    render_2D_syn = ovmap.sceneObject.render_2D_syn

    def __init__(self, dev, fc, B, scale, bx, hidden, W, H, obj_id):
        c = ocfg.Config(ocfg.replica_room0_config(train_device=str(dev)))
        c.obj_id, c.W, c.H, c.hidden_feature_size, c.obj_scale = obj_id, W, H, hidden, float(scale)
        self.trainer = trainer.Trainer(c)
        with torch.no_grad():
            for p, q in zip(self.trainer.fc_occ_map.parameters(), fc):
                p.copy_(q)
            self.trainer.pe.B_layer.weight.copy_(B)
        self.training_device = dev
        self.box = bx

    def get_bound(self, *a, **k):
        return None, self.box


_SCENE = {}


def scene():
    """render_util.view_scene() (hidden-128 background 0, objects 1 to 3) plus object 4, a SECOND background of hidden
    32 in front of part of the scene."""
    if not _SCENE:
        v = view_scene()
        full = torch.ones(v["W"], v["H"], dtype=torch.bool)
        bx = box((0.1, 0.0, 2.0), (2.0, 1.6, 0.5), axis=(0, 1, 1), deg=10)
        fc, B = make_net("mixed", hidden=32, seed=14, alpha_bias=-0.1)
        objects = dict(v["objects"])
        objects[4] = dict(fc=fc, B=B, scale=2.0, box=bx, hidden=32)
        draws = dict(v["draws"])
        draws[4] = draws_for(v["T_WC"], v["rays_dir"], full, bx, 44)
        class_of = dict(v["class_of"])
        class_of[4] = 11
        _SCENE.update(v, objects=objects, draws=draws, class_of=class_of, bg_ids=(0, 4))
    return _SCENE


_VIS = {}


def vis_objects(dev):
    if not _VIS:
        s = scene()
        for k, o in s["objects"].items():
            _VIS[k] = SceneObj(dev, o["fc"], o["B"], o["scale"], o["box"], o["hidden"], s["W"], s["H"], k)
    return _VIS


def t_oc_half(bx, T_WC):
    """The lines of Trainer.sample_points_bbox that form what objnerf_box_rays takes."""
    T_WO = torch.eye(4)
    T_WO[:3, :3] = torch.as_tensor(np.asarray(bx.R))
    T_WO[:3, 3] = torch.as_tensor(np.asarray(bx.center))
    return torch.inverse(T_WO) @ T_WC, torch.as_tensor(np.asarray(bx.extent, np.float64) / 2.0).float()


def candidate_rays(dev, boxes):
    s = scene()
    T = torch.as_tensor(s["T_WC"], dtype=torch.float32)
    dirs_C = s["rays_dir"].to(dev, torch.float32).reshape(-1, 3).contiguous()
    recs = torch.stack([map_view.view_box_record(b, T) for b in boxes]).to(dev)
    seg_off, seg, ws = ops.view_rays_count(T.to(dev), recs, dirs_C)
    pix, dirs_W, near, far = ops.view_rays_emit(T.to(dev), recs, dirs_C, ws, seg[-1])
    return T, dirs_C, seg_off, seg, pix, dirs_W, near, far


def test_candidate_rays_equal_box_rays(dev):
    """D1: the five boxes of the scene, a box behind the camera (0 hits) and a 1 cm box around one pixel's ray at 2 m
    (exactly 1 hit): seg_off, pix, dirs_W, near, far bit-equal to ops.box_rays + nonzero per object; the 0-hit and the
    1-hit object have empty segments."""
    s = scene()
    T = torch.as_tensor(s["T_WC"], dtype=torch.float32)
    d = s["rays_dir"][40, 30].double().numpy()
    centre = T[:3, 3].double().numpy() + T[:3, :3].double().numpy() @ d * (2.0 / d[2])
    boxes = [s["objects"][k]["box"] for k in range(5)]
    boxes.insert(2, box((0.3, 0.1, -3.0), (1.3, 0.9, 0.8)))                 # behind the camera
    boxes.insert(4, box(centre, (0.01, 0.01, 0.01)))                          # one pixel's ray
    T, dirs_C, seg_off, seg, pix, dirs_W, near, far = candidate_rays(dev, boxes)
    assert seg_off.dtype == torch.int64 and seg_off.tolist() == seg and seg[0] == 0
    n_hits = []
    for k, bx in enumerate(boxes):
        T_OC, half = t_oc_half(bx, T)
        dW, nr, fr, hit = ops.box_rays(T, T_OC, half, dirs_C)
        idx = hit.nonzero(as_tuple=True)[0]
        n_hits.append(int(idx.shape[0]))
        lo, hi = seg[k], seg[k + 1]
        if n_hits[-1] <= 1:
            assert hi == lo, (k, n_hits[-1])
            continue
        assert hi - lo == n_hits[-1]
        assert torch.equal(pix[lo:hi].long(), idx)
        assert torch.equal(dirs_W[lo:hi], dW[idx]) and torch.equal(near[lo:hi], nr[idx]) and torch.equal(far[lo:hi], fr[idx])
    assert n_hits[2] == 0 and n_hits[4] == 1
    assert sorted(n_hits[k] for k in (1, 3, 5, 6)) == [110, 1059, 1556, 3981]
    assert pix.shape[0] == seg[-1] == sum(n for n in n_hits if n > 1)


def small_objects(dev):
    """The four hidden-32 objects: their stacked arena, a single-object arena each, and their CSR."""
    s = scene()
    ids = [1, 2, 3, 4]
    T, dirs_C, seg_off, seg, pix, dirs_W, near, far = candidate_rays(dev, [s["objects"][k]["box"] for k in ids])
    stacked = ops.ParamArena(len(ids), ops.NetShape(), dev)
    stacked.load_stacked([torch.stack([s["objects"][k]["fc"][i] for k in ids]) for i in range(18)] +
                         [torch.stack([s["objects"][k]["B"] for k in ids])])
    singles = []
    for row, k in enumerate(ids):
        a = ops.ParamArena(1, ops.NetShape(), dev)
        R.load_arena(a, s["objects"][k]["fc"], s["objects"][k]["B"])
        a.scale.fill_(1.5 + 0.25 * row)
        stacked.scale[row] = 1.5 + 0.25 * row
        singles.append(a)
    return ids, T[:3, 3], seg, dirs_W, near, far, stacked, singles


@pytest.mark.parametrize("seeded", [False, True])
def test_segmented_render_equals_render_fwd(dev, seeded):
    """D2: depth, opacity and rgb of every object bit-equal to ops.render_fwd on the same rays -- with injected u and
    seeded with consecutive draw counters; segments of 110, 1059, 1556 and 3981 rays (none a multiple of 16); one
    workgroup that restages across all four objects, and the default grid."""
    s = scene()
    ids, origin, seg, dirs_W, near, far, stacked, singles = small_objects(dev)
    sizes = [seg[i + 1] - seg[i] for i in range(len(ids))]
    assert sorted(sizes) == [110, 1059, 1556, 3981] and all(n % 16 for n in sizes)
    seed, u_all, rows, ref = 987654321, None, [], []
    if not seeded:
        us = [s["draws"][k].to(dev) for k in ids]
        u_all = torch.cat(us)
    u_lo = 0
    for row, k in enumerate(ids):
        lo, hi = seg[row], seg[row + 1]
        rows.append((row, lo, hi, None if seeded else u_lo, 17 + row))
        ref.append(ops.render_fwd(singles[row], origin, dirs_W[lo:hi], near[lo:hi], far[lo:hi],
                                  None if seeded else us[row], 150, seed=seed, draw=17 + row, want_hfeat=False))
        u_lo += hi - lo
    outs = []
    for wgs in (1, 0):
        o = ops.render_fwd_segmented(stacked, origin, dirs_W, near, far, rows, u_all, 150, seed=seed, _workgroups=wgs)
        for row in range(len(ids)):
            lo, hi = seg[row], seg[row + 1]
            for key in ("depth", "opacity", "rgb"):
                assert torch.equal(o[key][lo:hi], ref[row][key]), (wgs, row, key)
        outs.append(o)
    for key in ("depth", "opacity", "rgb"):
        assert torch.equal(outs[0][key], outs[1][key])
    if seeded:      # another draw counter is another image
        assert not torch.equal(ref[0]["depth"], ops.render_fwd(singles[0], origin, dirs_W[:seg[1]], near[:seg[1]], far[:seg[1]],
                                                               None, 150, seed=seed, draw=99, want_hfeat=False)["depth"])


def ordered(order):
    s = scene()
    return {k: s["objects"][k] for k in order}


_BATCHED = {}


def batched_view(dev, order):
    """render_view_batched of one dict order, rendered once and shared by D3 and D4."""
    key = tuple(order)
    if key not in _BATCHED:
        s, vis = scene(), vis_objects(dev)
        _BATCHED[key] = render_view.render_view_batched({k: vis[k] for k in order}, s["T_WC"], s["rays_dir"],
                                                        bg_ids=s["bg_ids"], class_of=s["class_of"], draws=s["draws"])
    return _BATCHED[key]


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "".join(map(str, o)))
def test_batched_view_equals_the_loop(dev, order):
    """D3: render_view_batched against render_view.render_view on the same injected draws, two backgrounds (hidden 128
    and hidden 32), three dict orders: rgb, maskid and depth equal as arrays."""
    s, vis = scene(), vis_objects(dev)
    loop = render_view.render_view({k: vis[k] for k in order}, s["T_WC"], s["rays_dir"], bg_ids=s["bg_ids"],
                                   class_of=s["class_of"], draws=s["draws"])
    got = batched_view(dev, order)
    print(f"\norder {order}: class 11 paints {int((loop.maskid == 11).sum())} pixels, "
          f"{int((loop.maskid == 0).sum())} unpainted")
    assert got.rgb.dtype == np.uint8 and got.maskid.dtype == np.int32 and got.depth.dtype == np.float32
    assert np.array_equal(got.maskid, loop.maskid)
    assert np.array_equal(got.depth, loop.depth)
    assert np.array_equal(got.rgb, loop.rgb)
    assert (loop.maskid == 11).any() and (loop.maskid == 7).any()            # both backgrounds paint somewhere


def test_the_order_rule_is_exercised(dev):
    """The three orders of D3 give different images: how much the second background paints depends on what comes after
    it."""
    n11 = [int((batched_view(dev, o).maskid == 11).sum()) for o in ORDERS]
    print(f"\nclass 11 pixels per order: {n11}")
    assert len(set(n11)) == 3 and min(n11) < max(n11) // 4


_ORACLE = {}


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "".join(map(str, o)))
def test_batched_view_against_the_reference_merge(dev, order, monkeypatch):
    """D4: the same three orders against render_util.view_ref, judged as test_render_view_per_pixel judges: maskid
    equal, rgb within 1, depth under the 1e-4 bar on the pixels whose margin is at least MARGIN, and at most
    EXCLUDE_CAP of the pixels are not."""
    real = R.O.render_2d_syn

    def cached(*a, **k):          # an object's reference render does not depend on the order: computed once
        if k["obj_id"] not in _ORACLE:
            _ORACLE[k["obj_id"]] = real(*a, **k)
        return _ORACLE[k["obj_id"]]

    monkeypatch.setattr(R.O, "render_2d_syn", cached)
    s = scene()
    ref = view_ref(ordered(order), s["T_WC"], s["rays_dir"], s["bg_ids"], s["class_of"], s["draws"])
    buf = batched_view(dev, order)
    ok = ref["margin"] >= MARGIN
    assert (~ok).mean() <= EXCLUDE_CAP
    dc = int(np.abs(buf.rgb[ok].astype(int) - ref["rgb"][ok].astype(int)).max())
    de = R.scaled_err(buf.depth[ok], ref["depth"][ok])
    print(f"\norder {order}: {int((~ok).sum())} pixels left out, colour {dc}, depth {de:.2e}")
    assert np.array_equal(buf.maskid[ok], ref["maskid"][ok])
    assert dc <= 1 and de < BAR


def test_mapview_render_is_reproducible_and_exposes_the_winner(dev):
    """D5: MapView.render twice: the same bytes; to_host=False: the same images as device tensors; winner: the depth of
    the CSR entry that painted equals the depth image wherever a foreground object painted, the pixel of that entry is
    the pixel, and its object's id is the mask id."""
    s, vis = scene(), vis_objects(dev)
    order = ORDERS[0]
    objs = [map_view.MapObject(vis[k].trainer, vis[k].box, obj_id=k) for k in order]
    mv = map_view.MapView(objs, device=dev, bg_ids=s["bg_ids"], class_of=s["class_of"])
    assert mv.order == list(order)
    a = mv.render(s["T_WC"], s["rays_dir"], draws=s["draws"])
    b = mv.render(s["T_WC"], s["rays_dir"], draws=s["draws"])
    for key in ("rgb", "maskid", "depth"):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes()
    first = batched_view(dev, order)
    assert np.array_equal(a.rgb, first.rgb) and np.array_equal(a.maskid, first.maskid) and np.array_equal(a.depth, first.depth)
    t = mv.render(s["T_WC"], s["rays_dir"], draws=s["draws"], to_host=False)
    assert all(t[k].is_cuda for k in ("rgb", "maskid", "depth", "winner"))
    for key in ("rgb", "maskid", "depth"):
        assert np.array_equal(t[key].cpu().numpy(), getattr(a, key))
    win = mv.winner.cpu().numpy()
    assert win.shape == (s["W"], s["H"]) and win.dtype == np.int32
    assert np.array_equal(win >= 0, a.maskid != 0)
    seg = np.asarray(mv.seg)
    assert mv.seg_off.tolist() == mv.seg
    e = win[win >= 0]
    obj = np.searchsorted(seg, e, side="right") - 1
    flat = np.flatnonzero((win >= 0).reshape(-1))
    assert np.array_equal(mv.csr["pix"].cpu().numpy()[e], flat)
    ids = np.array([s["class_of"][k] for k in order])
    assert np.array_equal(ids[obj], a.maskid[win >= 0])
    fg = ~np.isin(np.array(order)[obj], s["bg_ids"])
    assert fg.any() and (~fg).any()
    assert np.array_equal(mv.csr["depth"].cpu().numpy()[e][fg], a.depth[win >= 0][fg])
    assert (a.depth[a.maskid == 0] == 100).all()


def test_cli_writes_the_reference_images(dev, tmp_path, capsys):
    """python -m openobj_amd.map_view end to end: checkpoints (a hidden-128 background, two hidden-32 objects, one
    without a box) and a Replica scene on disk -> rgb_ / depth_ / maskid_<frame id>.png in [H, W], equal to an in-process
    MapView.render of the same poses."""
    import json
    import os
    from PIL import Image
    import scene_files as SF
    from openobj_amd import dataset, vmap
    SF.write_scene(str(tmp_path / "data"), "Replica", n_frames=30)
    d = ocfg.replica_room0_config(**{"dataset.path": str(tmp_path / "data"), "dataset.format": "Replica", "trainer.part_mode": 0,
                                     "camera.w": SF.W, "camera.h": SF.H, "camera.fx": SF.FX, "camera.fy": SF.FY,
                                     "camera.cx": SF.CX, "camera.cy": SF.CY})
    with open(tmp_path / "scene.json", "w") as fh:
        json.dump(d, fh)
    s = scene()
    logdir, outdir = tmp_path / "log", tmp_path / "out"
    boxes = {0: s["objects"][0]["box"], 1: s["objects"][1]["box"], 3: s["objects"][3]["box"], 2: None}   # (the camera pans near the origin)
    for k, bx in boxes.items():
        t = vis_objects(dev)[k].trainer
        os.makedirs(logdir / "ckpt" / str(k))
        torch.save({"epoch": 0, "FC_state_dict": t.fc_occ_map.state_dict(), "PE_state_dict": t.pe.state_dict(), "obj_id": k,
                    "bbox": bx, "obj_scale": t.obj_scale, "clip_feat": None, "caption_feat": None, "semantic_id": 40 + k},
                   str(logdir / "ckpt" / str(k) / f"obj_{k}.pth"))
    ops._draw_offset[0] = 0            # the process-wide draw counter: the in-process renders below restart it too
    map_view.main(["--logdir", str(logdir), "--config", str(tmp_path / "scene.json"), "--frames", "1:3", "--out", str(outdir),
                   "--semantic-ids", "--device", str(dev)])
    out = capsys.readouterr().out
    assert "obj 2: the checkpoint carries no box, skipped" in out
    c = ocfg.Config(str(tmp_path / "scene.json"))
    ds = dataset.Replica(c)
    rays = vmap.cameraInfo(c).rays_dir_cache
    mv = map_view.MapView.from_logdir(str(logdir), str(dev), semantic_ids=True)
    assert mv.order == [0, 1, 3] and mv.info.cpu().tolist() == [[1, 40], [0, 41], [0, 43]]
    assert sorted(os.listdir(outdir)) == sorted(f"{n}_{int(ds.start + i * ds.stride)}.png" for i in (1, 2)
                                                for n in ("rgb", "depth", "maskid"))
    ops._draw_offset[0] = 0
    painted = 0
    for i in (1, 2):
        fid = int(ds.start + i * ds.stride)
        buf = mv.render(np.asarray(ds.depth_and_pose(i)[1], np.float32), rays)
        rgb, dep, mid = (np.asarray(Image.open(outdir / f"{n}_{fid}.png")) for n in ("rgb", "depth", "maskid"))
        assert rgb.shape == (SF.H, SF.W, 3) and dep.shape == (SF.H, SF.W) and mid.shape == (SF.H, SF.W)
        assert np.array_equal(rgb, buf.rgb.transpose(1, 0, 2)) and np.array_equal(mid, buf.maskid.T)
        assert np.array_equal(dep, np.clip(np.rint(buf.depth.T), 0, 255).astype(np.uint8))
        assert set(np.unique(mid)) <= {0, 40, 41, 43} and f"frame {fid}:" in out
        painted += int((mid != 0).sum())
    assert painted > 0
