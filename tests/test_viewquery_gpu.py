"""GPU: part features and open-vocabulary queries in a map view (MapView.render(want_feat=True), .query, .features;
objnerf_render_fwd_segmented_feat, objnerf_view_query).  The feature hidden of the segmented renderer against
ops.render_fwd bit for bit, the images of a want_feat view against the plain view byte for byte, the query kernel on a
hand-built CSR against fp64, the whole chain against the per-object loop, and the CLI.  Views are 80 x 60, the scene is
the one of tests/test_mapview_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

import test_mapview_gpu as TM
import viewquery_util as VQ
from openobj_amd import _lib, map_view, ops, render_view
from openobj_amd import cfg as ocfg

pytestmark = pytest.mark.gpu

GUARD = 64
# forward bound of a 33-term fp32 dot product in any order, doubled for the MFMA's internal order: per element of F,
# times |of_w| . |h| + |of_b| opacity
F_BOUND = 64 * VQ.U24
COS_BAR = 1e-5          # what the project holds objnerf_project's cosine to (tests/test_query_gpu.py)


def guarded(shape, dev, dtype=torch.float32):
    """A contiguous tensor of `shape` with GUARD NaN rows (-7 for integers) before and after it."""
    fill = float("nan") if dtype.is_floating_point else -7
    big = torch.full((shape[0] + 2 * GUARD,) + tuple(shape[1:]), fill, dtype=dtype, device=dev)
    return big, big[GUARD:GUARD + shape[0]]


def guards_hold(big, n):
    g = torch.cat([big[:GUARD], big[GUARD + n:]])
    return bool(torch.isnan(g).all()) if big.dtype.is_floating_point else bool((g == -7).all())


# ------------------------------------------------------------------------------------------------------------- Q1
@pytest.mark.parametrize("seeded", [False, True])
def test_segmented_hfeat_equals_render_fwd(dev, seeded):
    """Q1: the composited feature hidden of the segmented launch, bit-equal per object to ops.render_fwd(want_hfeat=True)
    on the same rays (injected and seeded draws; segments of 110, 1059, 1556, 3981 rays, every last group ragged);
    depth / opacity / rgb bit-equal to the launch without it; one workgroup restaging across all four objects equals the
    default grid; NaN guard rows around every output stay NaN; two calls write the same bits."""
    s = TM.scene()
    ids, origin, seg, dirs_W, near, far, stacked, singles = TM.small_objects(dev)
    M = seg[-1]
    assert all((seg[i + 1] - seg[i]) % 16 for i in range(len(ids)))
    seed, u_all, rows, ref, u_lo = 987654321, None, [], [], 0
    us = [s["draws"][k].to(dev) for k in ids]
    if not seeded:
        u_all = torch.cat(us)
    for row in range(len(ids)):
        lo, hi = seg[row], seg[row + 1]
        rows.append((row, lo, hi, None if seeded else u_lo, 17 + row))
        ref.append(ops.render_fwd(singles[row], origin, dirs_W[lo:hi], near[lo:hi], far[lo:hi], None if seeded else us[row],
                                  150, seed=seed, draw=17 + row, want_hfeat=True))
        u_lo += hi - lo
    plain = ops.render_fwd_segmented(stacked, origin, dirs_W, near, far, rows, u_all, 150, seed=seed)
    outs = []
    for wgs in (1, 0, 0):
        bigs, out = {}, {}
        for key, shp in (("depth", (M,)), ("opacity", (M,)), ("rgb", (M, 3)), ("hfeat", (M, 32))):
            bigs[key], out[key] = guarded(shp, dev)
        o = ops.render_fwd_segmented(stacked, origin, dirs_W, near, far, rows, u_all, 150, seed=seed, out=out,
                                     _workgroups=wgs, want_hfeat=True)
        assert o["hfeat"].data_ptr() == out["hfeat"].data_ptr()
        for key in bigs:
            assert guards_hold(bigs[key], M), (wgs, key)
        for row in range(len(ids)):
            lo, hi = seg[row], seg[row + 1]
            assert torch.equal(o["hfeat"][lo:hi], ref[row]["vals"]), (wgs, row)
            for key in ("depth", "opacity", "rgb"):
                assert torch.equal(o[key][lo:hi], ref[row][key]), (wgs, row, key)
        for key in ("depth", "opacity", "rgb"):
            assert torch.equal(o[key], plain[key]), (wgs, key)
        outs.append(o)
    assert not bool(torch.isnan(outs[0]["hfeat"]).any()) and float(outs[0]["hfeat"].abs().max()) > 0
    for other in outs[1:]:
        for key in ("depth", "opacity", "rgb", "hfeat"):
            assert torch.equal(outs[0][key], other[key]), key


# ------------------------------------------------------------------------------------------------------------- Q2
def make_view(dev, order, bf16_ids=()):
    s, vis = TM.scene(), TM.vis_objects(dev)
    for k in bf16_ids:
        vis[k].trainer.render_bf16 = True
    try:
        objs = [map_view.MapObject(vis[k].trainer, vis[k].box, obj_id=k) for k in order]
        return map_view.MapView(objs, device=dev, bg_ids=s["bg_ids"], class_of=s["class_of"])
    finally:
        for k in bf16_ids:
            vis[k].trainer.render_bf16 = False


@pytest.mark.parametrize("order", TM.ORDERS, ids=lambda o: "".join(map(str, o)))
@pytest.mark.parametrize("seeded", [False, True])
def test_want_feat_keeps_the_images(dev, order, seeded):
    """Q2: rgb, maskid, depth and winner of a want_feat view are the bytes of the plain view, in every order, with
    injected draws and in a seeded run; the process-wide draw counter ends where the plain view leaves it."""
    s = TM.scene()
    mv = make_view(dev, order)
    res, counters = [], []
    for want in (False, True):
        ops._draw_offset[0] = 1000
        res.append(mv.render(s["T_WC"], s["rays_dir"], draws=None if seeded else s["draws"], to_host=False, want_feat=want))
        counters.append(ops._draw_offset[0])
        assert (mv.own_hfeat is not None) == want and ("hfeat" in mv.csr) == want
    assert counters[0] == counters[1] == (1000 + len(order) if seeded else 1000)
    for key in ("rgb", "maskid", "depth", "winner"):
        assert torch.equal(res[0][key], res[1][key]), key
    assert bool((res[1]["maskid"] != 0).any())
    k0 = order.index(0)
    assert mv.csr["hfeat"].shape == (mv.seg[-1], 32) and mv.own_hfeat[k0].shape == (mv.seg[k0 + 1] - mv.seg[k0], 128)


# ------------------------------------------------------------------------------------------------------------- Q3
_KC = {}


def kernel_case(dev):
    """viewquery_util.kernel_case on the device, with its fp64 evaluation from the same inputs; shared, never changed."""
    if not _KC:
        c = VQ.kernel_case()
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        shared = None
        heads = []
        for of_w, of_b, hfeat, row0 in c["heads"]:
            if row0 == 0 and hfeat.shape[0] == c["pix"].shape[0]:
                shared = t(hfeat) if shared is None else shared
                heads.append((t(of_w), t(of_b), shared, 0))
            else:
                heads.append((t(of_w), t(of_b), t(hfeat), row0))
        _KC.update(c, dev=dict(seg_off=t(c["seg"]), pix=t(c["pix"]), opacity=t(c["opacity"]), winner=t(c["winner"]),
                               heads=heads))
    return _KC


def run_query(c, q=None, pixels=None, wgs=0, **kw):
    d = c["dev"]
    return ops.view_query(d["seg_off"], d["pix"], d["opacity"], d["winner"], list(d["heads"]), queries=q, pixels=pixels,
                          _workgroups=wgs, **kw)


def test_kernel_case_has_what_it_claims(dev):
    c = kernel_case(dev)
    seg, pix, win = c["seg"], c["pix"], c["winner"]
    assert np.diff(seg).tolist() == [1, 15, 16, 17, 65, 40, 33] and [h[0].shape[1] for h in c["heads"]] == [32] * 6 + [128]
    M = int(seg[-1])
    live = np.zeros(M, bool)
    ok = (pix >= 0) & (pix < VQ.KERNEL_P)
    live[ok] = win[pix[ok]] == np.flatnonzero(ok)
    obj = np.searchsorted(seg, np.arange(M), side="right") - 1
    assert not live[obj == VQ.NEVER_WINS].any()
    assert all(live[obj == k].any() for k in range(7) if k != VQ.NEVER_WINS)      # the 1-entry segment and H = 128 too
    chunks = live[:M - M % 16].reshape(-1, 16)
    assert (~chunks.any(axis=1)).any() and chunks.any(axis=1).any()              # a 16-entry group with no live lane
    assert any(len(set(obj[16 * j:16 * j + 16][live[16 * j:16 * j + 16]])) > 1 for j in range(M // 16))   # two objects in one group
    assert pix[win[c["p_foreign"]]] != c["p_foreign"] and pix[c["e_outside"]] >= VQ.KERNEL_P
    assert (win < 0).sum() > 5


@pytest.mark.parametrize("Q", [1, 3, 16])
def test_view_query_against_fp64(dev, Q):
    """Q3: sims within 1e-5 max(1, A / |F|) of the fp64 evaluation of the same device inputs, label EXACTLY the first
    arg-max of the returned sims, best that maximum, NaN / -1 where nothing painted (the foreign winner included), guard
    rows intact, one workgroup and two calls bit-equal to the default."""
    c = kernel_case(dev)
    P = VQ.KERNEL_P
    q = VQ.unit_queries(np.random.RandomState(Q), Q, VQ.KERNEL_C)
    ref = VQ.view_query_ref(c["seg"], c["pix"], c["opacity"], c["winner"], c["heads"], q)
    painted = ref["painted"]
    assert not painted[c["p_foreign"]] and painted.sum() > 60
    qd = torch.from_numpy(q).to(dev)
    outs = []
    for wgs in (0, 1, 0):
        o = run_query(c, qd, wgs=wgs)
        outs.append(o)
    for o in outs[1:]:
        for key in ("sims", "label", "best"):
            assert o[key].cpu().numpy().tobytes() == outs[0][key].cpu().numpy().tobytes(), key
    sims, label, best = (outs[0][k].cpu().numpy() for k in ("sims", "label", "best"))
    assert sims.shape == (Q, P) and label.dtype == np.int32 and label.shape == (P,)
    assert np.isnan(sims[:, ~painted]).all() and (label[~painted] == -1).all() and np.isnan(best[~painted]).all()
    assert not np.isnan(sims[:, painted]).any()
    Fn = np.linalg.norm(ref["F"][painted], axis=1)
    tol = COS_BAR * np.maximum(1.0, np.linalg.norm(ref["A"][painted], axis=1) / Fn)
    err = np.abs(sims[:, painted] - ref["sims"][:, painted])
    print(f"\nQ = {Q}: cosine error max {err.max():.2e} (bound {tol.min():.2e} .. {tol.max():.2e}), A / |F| max {tol.max() / COS_BAR:.1f}")
    assert (err <= tol[None]).all()
    assert np.array_equal(label, VQ.first_argmax(sims))
    assert np.array_equal(best[painted], sims[:, painted].max(axis=0))
    without = run_query(c, qd, want_sims=False, want_best=False)
    assert without["sims"] is None and without["best"] is None and torch.equal(without["label"], outs[0]["label"])


def test_view_query_feature_rows(dev):
    """Q3: the raw feature rows for a pixel list -- every pixel, repeats, out-of-range pixels: per element within
    64 * 2^-24 (|of_w| . |h| + |of_b| opacity) of fp64, zeros for unpainted and out-of-range pixels; int32 and int64
    lists, one workgroup and a second call give the same bits."""
    c = kernel_case(dev)
    P = VQ.KERNEL_P
    ref = VQ.view_query_ref(c["seg"], c["pix"], c["opacity"], c["winner"], c["heads"])
    px = np.concatenate([np.arange(P), [-1, P, P + 5, 2 ** 31 + 3, 7, 7, c["p_foreign"]], np.arange(P)[::-3]]).astype(np.int64)
    pd = torch.from_numpy(px).to(dev)
    a = run_query(c, pixels=pd)["feat"]
    assert a.shape == (px.shape[0], VQ.KERNEL_C) and run_query(c, pixels=pd)["label"] is None
    for other in (run_query(c, pixels=pd, wgs=1)["feat"], run_query(c, pixels=pd)["feat"]):
        assert torch.equal(a, other)
    inside = (px >= 0) & (px < P)
    assert torch.equal(a[torch.from_numpy(inside).to(dev)],
                       run_query(c, pixels=torch.from_numpy(px[inside].astype(np.int32)).to(dev))["feat"])
    a = a.cpu().numpy()
    want, bound = np.zeros_like(a, np.float64), np.zeros_like(a, np.float64)
    want[inside], bound[inside] = ref["F"][px[inside]], F_BOUND * ref["A"][px[inside]]
    zero = ~inside | ~np.where(inside, ref["painted"][np.clip(px, 0, P - 1)], False)
    assert (a[zero] == 0).all() and zero.sum() > 10 and (~zero).sum() > 100
    err = np.abs(a - want)
    print(f"\nfeature rows: max error / bound {np.max(err[~zero] / bound[~zero]):.3f}")
    assert (err <= bound).all()
    # guard rows around a feature output and around the query outputs: the library writes inside its buffers only
    d = c["dev"]
    arr, table = ops._view_heads(list(d["heads"]), VQ.KERNEL_C, dev)
    import ctypes as C
    n, Q, M = px.shape[0], 3, int(c["seg"][-1])
    q = torch.from_numpy(VQ.unit_queries(np.random.RandomState(3), Q, VQ.KERNEL_C)).to(dev)
    bf, feat = guarded((n, VQ.KERNEL_C), dev)
    bs, sim = guarded((Q * P,), dev)
    bl, lab = guarded((P,), dev, torch.int32)
    bb, bst = guarded((P,), dev)
    p32 = torch.where((pd >= 0) & (pd < P), pd, torch.full_like(pd, -1)).to(torch.int32)
    rc = _lib.lib().objnerf_view_query(P, 7, M, VQ.KERNEL_C, Q, d["seg_off"].data_ptr(), d["pix"].data_ptr(),
                                       d["opacity"].data_ptr(), d["winner"].data_ptr(), table.data_ptr(), C.addressof(arr),
                                       q.data_ptr(), sim.data_ptr(), lab.data_ptr(), bst.data_ptr(), n, p32.data_ptr(),
                                       feat.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert guards_hold(bf, n) and guards_hold(bs, Q * P) and guards_hold(bl, P) and guards_hold(bb, P)
    assert np.array_equal(feat.cpu().numpy(), a)
    assert torch.equal(sim.reshape(Q, P).nan_to_num(7.0), run_query(c, q)["sims"].nan_to_num(7.0))


def test_view_query_return_codes(dev):
    """Q = 0 and Q = 17 and a hidden width of 48 are EINVAL; a width of 96 (a multiple of 32 the build lacks) is ENOTSUP,
    never a wrong answer; M = 0 is only the unpainted fill."""
    c = kernel_case(dev)
    d = c["dev"]
    for Q in (0, 17):
        with pytest.raises(_lib.ObjnerfError, match="-22"):
            run_query(c, torch.zeros(Q, VQ.KERNEL_C, device=dev))
    q = torch.from_numpy(VQ.unit_queries(np.random.RandomState(0), 2, VQ.KERNEL_C)).to(dev)
    for H, code in ((48, "-22"), (96, "-95")):
        heads = list(d["heads"])
        heads[2] = (torch.zeros(VQ.KERNEL_C, H, device=dev), heads[2][1], torch.zeros(16, H, device=dev), int(c["seg"][2]))
        with pytest.raises(_lib.ObjnerfError, match=code):
            ops.view_query(d["seg_off"], d["pix"], d["opacity"], d["winner"], heads, queries=q)
    empty = ops.view_query(torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                           torch.zeros(0, device=dev), torch.full((50,), -1, dtype=torch.int32, device=dev),
                           [(h[0], h[1], None, 0) for h in d["heads"][:2]], queries=q,
                           pixels=torch.arange(4, device=dev))
    assert bool(torch.isnan(empty["sims"]).all()) and bool((empty["label"] == -1).all()) and bool((empty["feat"] == 0).all())


# ------------------------------------------------------------------------------------------------------------- Q4
def loop_features(dev, order, bf16_ids=()):
    """The per-object loop: SceneObj.render_2D_syn(render_part=True) per object, folded as train.py:581-598 folds."""
    s, vis = TM.scene(), TM.vis_objects(dev)
    results = {}
    for k in bf16_ids:
        vis[k].trainer.render_bf16 = True
    try:
        for oid in order:
            results[oid] = vis[oid].render_2D_syn(s["T_WC"], None, s["rays_dir"], render_part=True, draws=s["draws"][oid])
            if results[oid][1] is None:
                results[oid] = (None, None, None, None)
    finally:
        for k in bf16_ids:
            vis[k].trainer.render_bf16 = False
    buf = render_view.ViewBuffers(s["W"], s["H"])
    return buf, VQ.fold_features(buf, results, order, s["bg_ids"], s["class_of"], 512)


def view_bound(mv):
    """Per pixel and channel |of_w| . |h| + |of_b| opacity of the painter, from the view's own device tensors."""
    heads = [(w.cpu().numpy(), b.cpu().numpy(), None if h is None else h.cpu().numpy(), r0) for w, b, h, r0 in mv._view_heads()]
    return VQ.view_query_ref(mv.seg, mv.csr["pix"].cpu().numpy(), mv.csr["opacity"].cpu().numpy(), mv.winner.cpu().numpy(),
                             heads)


@pytest.mark.parametrize("order,bf16_ids", [(TM.ORDERS[0], ()), (TM.ORDERS[1], ()), (TM.ORDERS[2], (2,))],
                         ids=["10243", "34201", "01234-bf16"])
def test_features_of_every_pixel_equal_the_loop(dev, order, bf16_ids):
    """Q4: MapView.features over every pixel of the view against the per-object loop's render_partfeat folded by the
    reference's merge, per element within twice the Q3 bound (both sides are fp32 heads on identical hidden rows); two
    dict orders; with object 2 on the bf16 renderer the loop's own bf16 feature is the yardstick, within the same
    bound."""
    s = TM.scene()
    W, H = s["W"], s["H"]
    buf, want = loop_features(dev, order, bf16_ids)
    mv = make_view(dev, order, bf16_ids)
    assert [mv.own_bf16.get(order.index(k), False) for k in bf16_ids] == [True] * len(bf16_ids)
    got_img = mv.render(s["T_WC"], s["rays_dir"], draws=s["draws"], want_feat=True)
    assert np.array_equal(got_img.maskid, buf.maskid) and np.array_equal(got_img.depth, buf.depth) and \
        np.array_equal(got_img.rgb, buf.rgb)                                    # the painters are the same, bit for bit
    feat = mv.features(torch.arange(W * H, device=dev)).cpu().numpy().reshape(W, H, 512)
    wh = torch.stack(torch.meshgrid(torch.arange(W), torch.arange(H), indexing="ij"), -1).reshape(-1, 2)
    assert np.array_equal(mv.features(wh).cpu().numpy().reshape(W, H, 512), feat)                # the (w, h) form
    ref = view_bound(mv)
    painted = buf.maskid != 0
    assert np.array_equal(ref["painted"].reshape(W, H), painted)
    assert (feat[~painted] == 0).all() and (want[~painted] == 0).all()
    bound = 2 * F_BOUND * ref["A"].reshape(W, H, 512)
    err = np.abs(feat.astype(np.float64) - want.astype(np.float64))
    print(f"\norder {order} bf16 {bf16_ids}: {int(painted.sum())} painted pixels, max error / bound "
          f"{np.max(err[painted] / bound[painted]):.3f}, |F| median {np.median(np.linalg.norm(want[painted], axis=1)):.3f}")
    assert (err <= bound).all()
    assert len(set(np.unique(got_img.maskid[painted]))) >= 4                    # several objects (both widths) painted


def test_query_of_a_view(dev):
    """MapView.query: shapes and dtypes, un-normalised queries are normalised, 20 queries (two launches) give the first
    arg-max over all of them, and a view rendered without want_feat refuses."""
    s = TM.scene()
    W, H = s["W"], s["H"]
    mv = make_view(dev, TM.ORDERS[0])
    mv.render(s["T_WC"], s["rays_dir"], draws=s["draws"], to_host=False)
    with pytest.raises(_lib.ObjnerfError, match="want_feat"):
        mv.query(np.ones((1, 512), np.float32))
    res = mv.render(s["T_WC"], s["rays_dir"], draws=s["draws"], to_host=False, want_feat=True)
    q = np.random.RandomState(5).standard_normal((20, 512)).astype(np.float32)
    o = mv.query(q)
    sims, label, best = o["sims"].cpu().numpy(), o["label"].cpu().numpy(), o["best"].cpu().numpy()
    assert sims.shape == (20, W, H) and label.shape == (W, H) and label.dtype == np.int32 and best.shape == (W, H)
    painted = res["maskid"].cpu().numpy() != 0
    assert np.array_equal(~np.isnan(best), painted) and np.array_equal(label >= 0, painted)
    assert np.array_equal(label.reshape(-1), VQ.first_argmax(sims.reshape(20, -1)))
    assert np.array_equal(best[painted], sims[:, painted].max(axis=0))
    assert (label[painted] >= 16).any() and (label[painted] < 16).any()      # both launches own some pixels
    F = mv.features(torch.arange(W * H, device=dev)).double().cpu().numpy()
    qn = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    cos = (qn @ F.T) / np.maximum(np.linalg.norm(F, axis=1), 1e-8)[None]
    assert np.abs(cos.reshape(20, W, H)[:, painted] - sims[:, painted]).max() < 1e-4
    assert mv.query(q, want_sims=False)["sims"] is None


# ------------------------------------------------------------------------------------------------------------- Q5
def test_cli_writes_label_images(dev, tmp_path, capsys):
    """Q5: python -m openobj_amd.map_view --queries on a two-frame scene: label_<id>.png (uint8 [H, W]) equals
    MapView.query's label + 1 of an in-process render of the same poses, sim_<id>.npy only with --save-sims."""
    from PIL import Image
    import scene_files as SF
    from openobj_amd import dataset, vmap
    SF.write_scene(str(tmp_path / "data"), "Replica", n_frames=20)
    d = ocfg.replica_room0_config(**{"dataset.path": str(tmp_path / "data"), "dataset.format": "Replica", "trainer.part_mode": 0,
                                     "camera.w": SF.W, "camera.h": SF.H, "camera.fx": SF.FX, "camera.fy": SF.FY,
                                     "camera.cx": SF.CX, "camera.cy": SF.CY})
    with open(tmp_path / "scene.json", "w") as fh:
        json.dump(d, fh)
    s = TM.scene()
    logdir = tmp_path / "log"
    for k in (0, 1, 3):
        t = TM.vis_objects(dev)[k].trainer
        os.makedirs(logdir / "ckpt" / str(k))
        torch.save({"epoch": 0, "FC_state_dict": t.fc_occ_map.state_dict(), "PE_state_dict": t.pe.state_dict(), "obj_id": k,
                    "bbox": s["objects"][k]["box"], "obj_scale": t.obj_scale, "clip_feat": None, "caption_feat": None,
                    "semantic_id": 40 + k}, str(logdir / "ckpt" / str(k) / f"obj_{k}.pth"))
    feats = np.random.RandomState(8).standard_normal((3, 512)).astype(np.float32)
    np.savez(str(tmp_path / "q.npz"), feats=feats, names=np.array(["handle", "seat", "leg"]))
    common = ["--logdir", str(logdir), "--config", str(tmp_path / "scene.json"), "--frames", "0:2", "--device", str(dev),
              "--queries", str(tmp_path / "q.npz")]
    c = ocfg.Config(str(tmp_path / "scene.json"))
    ds = dataset.Replica(c)
    fids = [int(ds.start + i * ds.stride) for i in (0, 1)]
    ops._draw_offset[0] = 0
    map_view.main(common + ["--out", str(tmp_path / "a")])
    assert "1 = handle, 2 = seat, 3 = leg" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}_{f}.png" for f in fids for n in ("rgb", "depth", "maskid", "label"))
    ops._draw_offset[0] = 0
    map_view.main(common + ["--out", str(tmp_path / "b"), "--save-sims"])
    mv = map_view.MapView.from_logdir(str(logdir), str(dev))
    rays = vmap.cameraInfo(c).rays_dir_cache
    ops._draw_offset[0] = 0
    labelled = 0
    for i, fid in enumerate(fids):
        buf = mv.render(np.asarray(ds.depth_and_pose(i)[1], np.float32), rays, want_feat=True)
        o = mv.query(feats)
        want = (o["label"].cpu().numpy() + 1).astype(np.uint8).T
        for out in ("a", "b"):
            png = np.asarray(Image.open(tmp_path / out / f"label_{fid}.png"))
            assert png.dtype == np.uint8 and png.shape == (SF.H, SF.W) and np.array_equal(png, want)
        # (the background's id is 0 here, so the mask-id image does not tell painted from unpainted: the winner does)
        assert np.array_equal(want != 0, mv.winner.cpu().numpy().T >= 0) and set(np.unique(want)) <= {0, 1, 2, 3}
        assert (want[buf.maskid.T != 0] != 0).all()
        sim = np.load(tmp_path / "b" / f"sim_{fid}.npy")
        assert sim.shape == (3, SF.H, SF.W) and np.array_equal(sim, o["sims"].cpu().numpy().transpose(0, 2, 1), equal_nan=True)
        labelled += int((want != 0).sum())
    assert labelled > 0
