"""GPU: objnerf_view_compare / ops.view_compare and openobj_amd/map_view_eval.py against the specification in
tests/vieweval_util.py.  acc and conf are EQUAL to the specification's integers; ssim_map is equal to the specification's
fp64 per-pixel value rounded to fp32 (its NaNs in the same places), which together with column 8 (the sum of q per row)
pins q -- test_q_per_pixel gives every pixel a row of its own, where column 8 IS the per-pixel q."""
import json
import os

import numpy as np
import pytest
import torch

import vieweval_util as U
from render_util import view_scene
from openobj_amd import cfg as ocfg
from openobj_amd import map_view, map_view_eval as E, ops, trainer
from openobj_amd import vmap as ovmap

pytestmark = pytest.mark.gpu

T = ops.VIEW_EVAL_TILE
SIZES = [(11, 11), (10, 13), (13, 10), (12, 11), (T + 1, T + 1), (2 * T + 3, T + 7), (T + 7, 2 * T + 3), (80, 60)]
IDS5 = [7, 3, 0, 12, 5]                                    # G = 5; lut has 13 entries
DRAWN = [7, 3, 0, 12, 5, 4, 9, -1, -7, 13, 400, 1 << 30]     # in the lut, missing from it, negative, past n_lut


def frame(W, H, kind="noise", seed=0, values=DRAWN, block=3):
    x, y = U.images(W, H, kind, seed)
    dr, dg = U.depths(W, H, seed)
    ir, ig = U.id_images(W, H, values, seed, block)
    g = torch.Generator().manual_seed(seed + 3000)
    painted = torch.rand(W, H, generator=g) < 0.7
    return dict(rgb_r=x, depth_r=dr, id_r=ir, painted=painted, rgb_g=y, depth_g=dg, id_g=ig)


_SPEC = {}


def spec(key, f, lut, G, painted=True):
    """U.compare once per (key): shared among the tests, never modified."""
    if key not in _SPEC:
        _SPEC[key] = U.compare(f["rgb_r"], f["depth_r"], f["id_r"], f["painted"] if painted else None, f["rgb_g"],
                               f["depth_g"], f["id_g"], lut, G)
    return _SPEC[key]


def run(dev, f, lut, G, painted=True, conf=True, ssim=True, wgs=0, acc=None, conf_t=None):
    d = lambda t: t.to(dev)
    acc = torch.zeros(G + 1, 9, dtype=torch.int64, device=dev) if acc is None else acc
    if conf and conf_t is None:
        conf_t = torch.zeros(G, G + 1, dtype=torch.int64, device=dev)
    m = ops.view_compare(d(f["rgb_r"]), d(f["depth_r"]), d(f["id_r"]), d(f["painted"]) if painted else None, d(f["rgb_g"]),
                         d(f["depth_g"]), d(f["id_g"]), torch.as_tensor(lut).to(dev), G, acc, conf_t if conf else None,
                         want_ssim_map=ssim, _workgroups=wgs)
    return acc, conf_t, m


def assert_equal(got, s, what=""):
    acc, conf, m = got
    assert torch.equal(acc.cpu(), s["acc"]), f"{what}: acc\n{acc.cpu() - s['acc']}"
    if conf is not None:
        assert torch.equal(conf.cpu(), s["conf"]), f"{what}: conf"
    if m is not None:
        m, want = m.cpu(), s["value"].float()
        assert m.dtype == torch.float32 and torch.equal(torch.isnan(m), torch.isnan(want)), f"{what}: the map's NaNs"
        ok = ~torch.isnan(want)
        assert torch.equal(m[ok], want[ok]), f"{what}: ssim_map"


@pytest.mark.parametrize("W,H", SIZES, ids=lambda v: str(v))
def test_sizes(dev, W, H):
    """Every size of the list with seeded noise, G = 5 with ids missing from the lut, negative and past n_lut on both
    sides, the three depth cases and an explicit painted mask."""
    f, lut = frame(W, H, "noise", seed=W * 100 + H), E.build_lut(IDS5)
    s = spec(("size", W, H), f, lut, 5)
    got = run(dev, f, lut, 5)
    assert_equal(got, s, f"{W} x {H}")
    acc = got[0].cpu()
    n_int = max(W - 10, 0) * max(H - 10, 0)
    assert int(acc[:, 0].sum()) == W * H and int(acc[:, 7].sum()) == n_int
    if n_int == 0:
        assert not bool(acc[:, 7:].any()) and bool(torch.isnan(got[2]).all())
    assert int(acc[5, 0]) > 0 and 0 < int(acc[:, 5].sum()) < int(acc[:, 4].sum()) < W * H    # every depth case occurs
    both = (f["depth_g"] == 0) & (f["depth_r"] == 100)
    assert bool(both.any()) and int(acc[:, 6].sum()) == int(s["acc"][:, 6].sum()) > 0


@pytest.mark.parametrize("kind", ["extreme", "identical", "inverted", "noise"])
def test_content(dev, kind):
    W, H = T + 13, T + 7                                    # four tiles, none whole
    f, lut = frame(W, H, kind, seed=11), E.build_lut(IDS5)
    s = spec(("content", kind), f, lut, 5)
    got = run(dev, f, lut, 5)
    assert_equal(got, s, kind)
    acc, m = got[0].cpu(), got[2].cpu()
    if kind == "identical":
        assert int(acc[:, 2].sum()) == 0 and torch.equal(acc[:, 8], acc[:, 7] << 32)
        assert bool((m[5:W - 5, 5:H - 5] == 1.0).all()) and bool((s["q"][5:W - 5, 5:H - 5] == 1 << 32).all())
    if kind == "extreme":
        assert int(acc[:, 2].sum()) == W * H * 3 * 65025
    if kind == "inverted":
        assert int(s["q"].min()) < 0 and int(acc[:, 8].sum()) < 0


def test_q_per_pixel(dev):
    """Every pixel a row of its own (G = 391, the global-atomic path, conf NULL): column 8 is q per pixel, column 7 the
    interior, column 2 the squared error per pixel."""
    W, H = 23, 17
    f = frame(W, H, "noisy", seed=4)
    f["id_g"] = torch.arange(W * H, dtype=torch.int32).reshape(W, H)
    lut = np.arange(W * H, dtype=np.int32)
    s = spec("per pixel", f, lut, W * H)
    got = run(dev, f, lut, W * H, conf=False)
    assert got[1] is None
    assert_equal(got, s, "per pixel")
    assert torch.equal(got[0].cpu()[:W * H, 8], s["q"].reshape(-1)) and int(s["q"].abs().max()) > 0
    inv = dict(f)
    inv["rgb_g"] = 255 - f["rgb_r"]
    s = spec("per pixel inverted", inv, lut, W * H)
    got = run(dev, inv, lut, W * H, conf=False, ssim=False)
    assert got[2] is None and torch.equal(got[0].cpu()[:W * H, 8], s["q"].reshape(-1)) and int(s["q"].min()) < 0


def test_one_row(dev):
    """G = 1."""
    f, lut = frame(T + 1, 15, "noisy", seed=2), E.build_lut([3])
    assert_equal(run(dev, f, lut, 1), spec("G1", f, lut, 1), "G = 1")


@pytest.mark.parametrize("G", [3, ops.VIEW_EVAL_LDS_ROWS + 6])
def test_every_pixel_one_id(dev, G):
    """The worst case for contention, on both paths: one row and one confusion cell take the whole frame."""
    W, H = 80, 60
    f = frame(W, H, "noisy", seed=6, values=[2])
    lut = np.arange(G, dtype=np.int32)
    s = spec(("one id", G), f, lut, G)
    got = run(dev, f, lut, G)
    assert_equal(got, s, f"one id, G = {G}")
    assert int(got[0][2, 0]) == W * H == int(got[1][2, 2]) and int(got[1].sum()) == W * H


def test_fallback_equals_the_lds_path(dev):
    """The same data with G = 70 (above the LDS cap: wave-aggregated global atomics) and G = 40 (below it): both equal the
    specification, the shared rows and cells are equal, and what has no row at G = 40 is folded into the last row and the
    last column."""
    hi, lo = ops.VIEW_EVAL_LDS_ROWS + 6, 40
    W, H = 2 * T + 3, T + 7
    f = frame(W, H, "noisy", seed=8, values=list(range(hi)) + [-1, 500], block=2)
    lut = np.arange(hi, dtype=np.int32)
    a = run(dev, f, lut, hi)
    b = run(dev, f, lut, lo)
    assert_equal(a, spec("fallback hi", f, lut, hi), "G = 70")
    assert_equal(b, spec("fallback lo", f, lut, lo), "G = 40")
    acc_a, acc_b, conf_a, conf_b = a[0].cpu(), b[0].cpu(), a[1].cpu(), b[1].cpu()
    assert torch.equal(acc_a[:lo], acc_b[:lo]) and torch.equal(acc_a[lo:].sum(0), acc_b[lo])
    assert torch.equal(conf_a[:lo, :lo], conf_b[:, :lo]) and torch.equal(conf_a[:lo, lo:].sum(1), conf_b[:, lo])
    assert int((conf_a[:lo, lo:hi]).sum()) > 0 and torch.equal(a[2].cpu().view(torch.int32), b[2].cpu().view(torch.int32))
    c = run(dev, f, lut, hi, conf=False, ssim=False)       # conf NULL on the fallback path
    assert c[1] is None and torch.equal(c[0].cpu(), acc_a)


def test_painted_null_against_a_mask(dev):
    f, lut = frame(T + 5, 21, "noisy", seed=9), E.build_lut(IDS5)
    null = run(dev, f, lut, 5, painted=False)
    assert_equal(null, spec("painted null", f, lut, 5, painted=False), "painted NULL")
    ones = dict(f, painted=torch.ones_like(f["painted"]))
    full = run(dev, ones, lut, 5)
    assert torch.equal(full[0], null[0]) and torch.equal(full[1], null[1])
    u8 = dict(f, painted=f["painted"].to(torch.uint8) * 200)                # any non-zero byte is "painted"
    mask, mask_u8 = run(dev, f, lut, 5), run(dev, u8, lut, 5)
    assert_equal(mask, spec("painted mask", f, lut, 5), "mask")
    assert torch.equal(mask[0], mask_u8[0])
    same = [0, 2, 4, 5, 6, 7, 8]
    assert torch.equal(mask[0][:, same], null[0][:, same]) and not torch.equal(mask[0][:, [1, 3]], null[0][:, [1, 3]])
    assert torch.equal(null[0][:, 0], null[0][:, 1]) and torch.equal(null[0][:, 2], null[0][:, 3])


def test_accumulation_order_and_grid(dev):
    """The tables are added to, never cleared; two frames in one table = the sum of two tables; three grids (1, an odd
    count, the default), both frame orders and a repeated call give the same bytes."""
    W, H = 2 * T + 3, T + 7
    lut = E.build_lut(IDS5)
    f1, f2 = frame(W, H, "noisy", seed=21), frame(W, H, "inverted", seed=22)
    s1, s2 = spec("acc f1", f1, lut, 5), spec("acc f2", f2, lut, 5)
    a1, a2 = run(dev, f1, lut, 5), run(dev, f2, lut, 5)
    assert_equal(a1, s1, "frame 1")
    assert_equal(a2, s2, "frame 2")
    tables = []
    for wgs in (1, 3, 0):
        for order in ((f1, f2), (f2, f1)):
            acc, conf, _ = run(dev, order[0], lut, 5, wgs=wgs)
            acc_b, conf_b, _ = run(dev, order[1], lut, 5, wgs=wgs, acc=acc, conf_t=conf)
            assert acc_b is acc and conf_b is conf
            tables.append((acc.cpu(), conf.cpu()))
    for acc, conf in tables:
        assert acc.numpy().tobytes() == tables[0][0].numpy().tobytes() and conf.numpy().tobytes() == tables[0][1].numpy().tobytes()
    assert torch.equal(tables[0][0], s1["acc"] + s2["acc"]) and torch.equal(tables[0][1], s1["conf"] + s2["conf"])
    assert torch.equal(tables[0][0], a1[0].cpu() + a2[0].cpu())
    again = run(dev, f1, lut, 5)
    assert again[0].cpu().numpy().tobytes() == a1[0].cpu().numpy().tobytes()
    assert again[2].cpu().numpy().tobytes() == a1[2].cpu().numpy().tobytes()
    pre = torch.full((6, 9), 5, dtype=torch.int64, device=dev)             # not cleared: 5 stays under what is added
    got = run(dev, f1, lut, 5, acc=pre, ssim=False)
    assert torch.equal(got[0].cpu(), s1["acc"] + 5)


def test_bad_arguments(dev):
    from openobj_amd import _lib
    f, lut = frame(12, 11), E.build_lut(IDS5)
    with pytest.raises(_lib.ObjnerfError):
        run(dev, f, lut, 5, acc=torch.zeros(5, 9, dtype=torch.int64, device=dev))
    with pytest.raises(_lib.ObjnerfError):
        run(dev, f, lut, 5, conf_t=torch.zeros(5, 5, dtype=torch.int64, device=dev))
    with pytest.raises(_lib.ObjnerfError):
        run(dev, dict(f, depth_g=f["depth_g"][:, :5]), lut, 5)
    with pytest.raises(_lib.ObjnerfError):
        run(dev, f, lut, 0, acc=torch.zeros(1, 9, dtype=torch.int64, device=dev), conf=False)


# ------------------------------------------------------------------------------------------------------ end to end
class SceneObj:
    """What MapObject needs of a scene object, built as tests/test_mapview_gpu.py builds it."""
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


_MAP = {}


def the_map(dev):
    """render_util.view_scene() as a MapView, its objects and one view rendered to the device; built once."""
    if not _MAP:
        s = view_scene()
        vis = {k: SceneObj(dev, o["fc"], o["B"], o["scale"], o["box"], o["hidden"], s["W"], s["H"], k)
               for k, o in s["objects"].items()}
        mv = map_view.MapView([map_view.MapObject(vis[k].trainer, vis[k].box, obj_id=k) for k in s["objects"]], device=dev,
                              bg_ids=s["bg_ids"], class_of=s["class_of"])
        view = mv.render(s["T_WC"], s["rays_dir"], draws=s["draws"], to_host=False)
        _MAP.update(scene=s, vis=vis, mv=mv, view=view)
    return _MAP


def test_a_view_against_itself_is_perfect(dev):
    m = the_map(dev)
    view = m["view"]
    before = {k: view[k].clone() for k in ("rgb", "maskid", "depth")}
    ev = E.ViewEval.from_map(m["mv"])
    assert ev.ids == [7, 3, 5, 9]
    ev.add(view, {"image": view["rgb"], "depth": view["depth"], "obj": view["maskid"]})
    r = ev.result()
    img = r["image"]
    assert img["psnr"] == float("inf") and img["psnr_painted"] == float("inf") and img["ssim"] == 1.0 and img["depth_l1"] == 0.0
    assert r["miou"] == 1.0 and r["accuracy"] == 1.0 and 0.0 < img["painted_share"] <= 1.0 and img["depth_coverage"] < 1.0
    assert int(r["acc"][:, 0].sum()) == 80 * 60 and int(r["acc"][:, 5].sum()) > 0
    for k, t in before.items():
        assert view[k].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), k


def test_a_view_against_a_perturbed_frame(dev):
    """Seeded noise on the colour, a depth offset on a rectangle, the ids of object 3 swapped for 5: equal to the
    specification, IoU of the swapped id 0; per_frame keeps the frame's integers; the view keeps its bytes."""
    m = the_map(dev)
    view = m["view"]
    before = {k: view[k].clone() for k in ("rgb", "maskid", "depth")}
    rgb, depth, mid = view["rgb"].cpu(), view["depth"].cpu(), view["maskid"].cpu()
    g = torch.Generator().manual_seed(5)
    image = (rgb.int() + torch.randint(-20, 21, rgb.shape, generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
    d_g = depth.clone()
    d_g[20:50, 10:40] += 0.25
    obj = mid.clone()
    assert bool((mid == 3).any()) and bool((mid == 5).any())
    obj[mid == 3] = 5
    ev = E.ViewEval.from_map(m["mv"], per_frame=True)
    ev.add(view, {"image": image.numpy(), "depth": d_g.numpy(), "obj": obj.numpy()}, ssim_map=True)
    r = ev.result()
    s = U.compare(rgb, depth, mid, view["winner"].cpu() >= 0, image, d_g, obj, E.build_lut(ev.ids), 4)
    assert torch.equal(torch.from_numpy(r["acc"]), s["acc"]) and torch.equal(torch.from_numpy(r["conf"]), s["conf"])
    assert_equal((ev.acc, ev.conf, ev.ssim_map), s, "perturbed")
    assert r["per_id"][3]["iou"] == 0.0 and 0.0 < r["per_id"][5]["iou"] < 1.0 and r["miou"] < 1.0
    assert 20.0 < r["image"]["psnr"] < 40.0 and 0.0 < r["image"]["ssim"] < 1.0 and 0.0 < r["image"]["depth_l1"] < 0.25
    assert np.array_equal(r["frame_rows"], r["acc"].sum(0)[None]) and r["per_frame"][0] == r["image"] and r["frames"] == 1
    for k, t in before.items():
        assert view[k].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), k


def test_cli(dev, tmp_path, capsys):
    """python -m openobj_amd.map_view_eval over the scene and checkpoints of test_cli_writes_the_reference_images, frames
    1:3: eval_views.json equals an in-process ViewEval; a second run writes the same file; --write-images then --renders
    on that directory gives the same colour and id figures."""
    import scene_files as SF
    from openobj_amd import dataset, vmap
    SF.write_scene(str(tmp_path / "data"), "Replica", n_frames=30)
    d = ocfg.replica_room0_config(**{"dataset.path": str(tmp_path / "data"), "dataset.format": "Replica", "trainer.part_mode": 0,
                                     "camera.w": SF.W, "camera.h": SF.H, "camera.fx": SF.FX, "camera.fy": SF.FY,
                                     "camera.cx": SF.CX, "camera.cy": SF.CY})
    cfg_file = str(tmp_path / "scene.json")
    with open(cfg_file, "w") as fh:
        json.dump(d, fh)
    m = the_map(dev)
    s, logdir = m["scene"], tmp_path / "log"
    for k, bx in {0: s["objects"][0]["box"], 1: s["objects"][1]["box"], 3: s["objects"][3]["box"], 2: None}.items():
        t = m["vis"][k].trainer
        os.makedirs(logdir / "ckpt" / str(k))
        torch.save({"epoch": 0, "FC_state_dict": t.fc_occ_map.state_dict(), "PE_state_dict": t.pe.state_dict(), "obj_id": k,
                    "bbox": bx, "obj_scale": t.obj_scale, "clip_feat": None, "caption_feat": None, "semantic_id": 40 + k},
                   str(logdir / "ckpt" / str(k) / f"obj_{k}.pth"))
    common = ["--logdir", str(logdir), "--config", cfg_file, "--frames", "1:3", "--device", str(dev)]

    def cli(out, *more):
        ops._draw_offset[0] = 0            # the process-wide draw counter: every run restarts it
        E.main(common + ["--out", str(tmp_path / out)] + list(more))
        with open(tmp_path / out / "eval_views.json", "rb") as fh:
            raw = fh.read()
        return raw, json.loads(raw)

    raw_a, rep = cli("a", "--write-images", "--ssim-maps")
    out = capsys.readouterr().out
    c = ocfg.Config(cfg_file)
    ds = dataset.Replica(c)
    rays = vmap.cameraInfo(c).rays_dir_cache
    fids = [int(ds.start + i * ds.stride) for i in (1, 2)]
    assert rep["frames"] == fids and rep["ids"] == [0, 1, 3] and rep["taps"] == U.TAPS and all(f"frame {i}:" in out for i in fids)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(["eval_views.json"] + [f"{n}_{i}.png" for i in fids
                                                                                for n in ("rgb", "depth", "maskid", "ssim")])
    mv = map_view.MapView.from_logdir(str(logdir), str(dev))
    ev = E.ViewEval.from_map(mv, per_frame=True)
    ops._draw_offset[0] = 0
    for i in (1, 2):
        sample = ds[i]
        ev.add(mv.render(np.asarray(sample["T"], np.float32), rays, to_host=False), sample)
    r = ev.result()
    assert rep["acc"] == r["acc"].tolist() and rep["conf"] == r["conf"].tolist() and rep["frame_rows"] == r["frame_rows"].tolist()
    plain = E._plain({k: r[k] for k in ("image", "other", "per_id", "per_frame", "miou", "accuracy")})
    assert all(rep[k] == plain[k] for k in plain) and isinstance(rep["image"]["psnr"], float)
    assert int(r["acc"][:, 0].sum()) == 2 * SF.W * SF.H and int(r["acc"][:, 1].sum()) > 0
    raw_b, _ = cli("b", "--write-images", "--ssim-maps")
    assert raw_b == raw_a
    for name in os.listdir(tmp_path / "a"):
        with open(tmp_path / "a" / name, "rb") as fa, open(tmp_path / "b" / name, "rb") as fb:
            assert fa.read() == fb.read(), name
    _, ren = cli("c", "--renders", str(tmp_path / "a"))
    assert ren["source"] == "renders" and ren["depth_scored"] is False and ren["image"]["depth_l1"] is None
    acc_a, acc_c = np.asarray(rep["acc"]), np.asarray(ren["acc"])
    assert np.array_equal(acc_a[:, [0, 2, 7, 8]], acc_c[:, [0, 2, 7, 8]]) and ren["conf"] == rep["conf"]
    assert ren["image"]["psnr"] == rep["image"]["psnr"] and ren["image"]["ssim"] == rep["image"]["ssim"]
    assert ren["miou"] == rep["miou"] and ren["accuracy"] == rep["accuracy"]
