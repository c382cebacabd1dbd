"""GPU: the mesh rasteriser (objnerf_mapraster.hip) against the specification of tests/mapraster_util.py.
Every pixel of every scene is compared: key, depth (bits), maskid, winner, face, vertex, counts, stats and status for
EQUALITY, rgb within one level (the device may blend in another order than the fp64 specification; an error far below
1 / 255 moves the quantiser by at most one level).  MapRaster and the CLI run end to end on the map with two planted
blobs."""
import functools
import gzip
import json
import os
import pickle

import numpy as np
import pytest
import torch

from openobj_amd import _lib, map_raster, ops, query
try:
    from tests import mapraster_util as U, mapregions_util as RU, partcompact_util as PU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import mapraster_util as U
    import mapregions_util as RU
    import partcompact_util as PU

pytestmark = pytest.mark.gpu

EXACT = ("key", "depth", "maskid", "winner", "face", "vertex", "counts", "stats")
SCENES = ("dense", "coarse", "interpenetrating", "giant", "on_samples", "duplicate", "z_near", "bound", "zero_area", "nan",
          "hidden", "empty", "sees_nothing")


@functools.lru_cache(maxsize=None)
def scenes():
    return U.make_scenes()


@functools.lru_cache(maxsize=None)
def spec(name, small=U.SMALL_DEFAULT, shading=True):
    """The specification of a scene, computed once and shared (nothing changes it)."""
    m = U.bad_index_scene() if name == "bad_index" else scenes()[name][0]
    return U.run_spec(m, small=small, shading=shading, background=(255, 255, 255) if shading else (9, 80, 200))


def run_device(dev, m, small=-1, shading=True, background=(255, 255, 255), ambient=0.35):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    verts, faces, foff = t(m["verts"]), t(np.asarray(m["faces"], np.int32).reshape(-1, 3)), t(m["face_off"])
    key, stats, status, ws = ops.raster_visibility(verts, faces, foff, t(m["hide"]), t(m["T_CW"]), m["intr"], m["W"], m["H"],
                                                   m["z_near"], _small_box=small)
    out = ops.raster_resolve(verts, faces, foff, t(m["ids"]), t(m["colors"]), ws, key, m["cam"], ambient, shading, background)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(key=key.cpu().numpy().view(np.uint64), stats=stats.cpu().numpy(), status=int(status.item()))
    return res


def assert_equal(got, want, names=EXACT, what=""):
    for k in names:
        a, b = got[k], want[k]
        if k == "depth":
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {k} differs at {int((a != b).sum())} places"
    assert got["status"] == want["status"], what


def assert_rgb(got, want, what=""):
    d = np.abs(got["rgb"].astype(np.int32) - want["rgb"].astype(np.int32))
    assert d.max(initial=0) <= 1, f"{what}: rgb off by {d.max()} levels at {int((d > 1).sum())} values"
    return int((d != 0).sum())


# ------------------------------------------------------------------------------------------ 1. the scenes, every pixel
@pytest.mark.parametrize("name", SCENES)
def test_scene_equals_the_specification(dev, name):
    m, claims = scenes()[name]
    want = spec(name)
    n_pix = m["W"] * m["H"]
    # from the specification alone: what the scene claims to exercise
    assert len(m["faces"]) <= 3000 and int(want["stats"].sum()) == len(m["faces"])
    for c in claims:
        if c == "half":
            assert 2 * int((want["winner"] >= 0).sum()) >= n_pix
        elif c == "both":
            assert want["stats"][U.ST["small"]] >= 1 and want["stats"][U.ST["large"]] >= 1
        else:
            assert want["stats"][U.ST[c]] >= 1, c
    if name in ("empty", "sees_nothing"):
        assert np.all(want["key"] == np.uint64(U.EMPTY)) and np.all(want["winner"] == -1) and np.all(want["depth"] == 100)
        assert np.all(want["rgb"] == 255) and np.all(want["maskid"] == 0)
    if name == "duplicate":                                 # two identical sheets: the first object's faces win everywhere
        assert np.all(want["winner"] == 0) and want["counts"].tolist() == [n_pix, 0]
    if name == "hidden":                                    # the hidden object lies in front and paints nothing
        assert want["counts"][1] == 0 and np.all(want["winner"] == 0)
    if name == "interpenetrating":
        assert min(want["counts"]) > n_pix // 4
    got = run_device(dev, m)
    assert_equal(got, want, what=name)
    off = assert_rgb(got, want, name)
    print(f"{name}: {len(m['faces'])} faces, stats {dict(zip(U.STATS, want['stats'].tolist()))}, "
          f"{int((want['winner'] >= 0).sum())} of {n_pix} pixels painted, {off} colour values off by one level")


def test_bad_index_raises_status_and_leaves_the_rest(dev):
    m = U.bad_index_scene()
    want, clean = spec("bad_index"), spec("coarse")
    assert want["status"] == ops.RASTER_STATUS_BAD_ID and want["stats"][U.ST["bad_index"]] == 2 and clean["status"] == 0
    for k in ("key", "depth", "maskid", "winner", "face", "vertex", "counts", "rgb"):       # in the specification already
        assert np.array_equal(want[k], clean[k]), k
    got = run_device(dev, m)
    assert_equal(got, want, what="bad_index")
    assert_rgb(got, want)
    # status is OR-ed into the caller's word
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = torch.tensor([4], dtype=torch.int32, device=dev)
    ops.raster_visibility(t(m["verts"]), t(m["faces"]), t(m["face_off"]), t(m["hide"]), t(m["T_CW"]), m["intr"], m["W"], m["H"],
                          status=st)
    assert int(st.item()) == 5


def test_unshaded_colours_and_background(dev):
    for name in ("interpenetrating", "z_near"):
        m = scenes()[name][0]
        want = spec(name, shading=False)
        got = run_device(dev, m, shading=False, background=(9, 80, 200))
        assert_equal(got, want, what=name)
        assert_rgb(got, want, name)
    blank = want["winner"] < 0
    assert blank.any() and np.all(got["rgb"][blank] == np.array([9, 80, 200], np.uint8))
    # shading only ever darkens, and by no more than the ambient floor allows (one level of slack for the quantiser)
    lit = run_device(dev, m)["rgb"].astype(np.int32)[~blank]
    raw = got["rgb"].astype(np.int32)[~blank]
    assert np.all(lit <= raw + 1) and np.all(lit >= np.floor(0.35 * raw) - 1)


# ---------------------------------------------------------------------------------------------------- 2. properties
@pytest.mark.parametrize("name", ["dense", "interpenetrating", "on_samples", "giant"])
def test_small_path_knob_leaves_the_bytes_alone(dev, name):
    """Every face through the large path, every face through the small one, and the default: the same images; only the
    two `drawn` counters move, and they equal the specification run with the same threshold."""
    m = scenes()[name][0]
    want = spec(name)
    images = ("key", "depth", "maskid", "winner", "face", "vertex", "counts")
    runs, rgb = {}, run_device(dev, m)["rgb"]
    drawn = int(want["stats"][0] + want["stats"][1])
    for small in (0, ops.RASTER_SMALL_MAX, -1, 1, 7):
        got = run_device(dev, m, small=small)
        assert_equal(got, want, images, what=f"{name} small={small}")
        assert np.array_equal(got["rgb"], rgb)
        assert np.array_equal(got["stats"][2:], want["stats"][2:]) and int(got["stats"][0] + got["stats"][1]) == drawn
        runs[small] = got["stats"][:2].tolist()
    assert runs[0] == [0, drawn] and runs[ops.RASTER_SMALL_MAX] == [drawn, 0] and runs[-1] == want["stats"][:2].tolist()
    for small in (1, 7):
        assert runs[small] == spec(name, small=small)["stats"][:2].tolist()


def test_two_runs_give_the_same_bytes(dev):
    for name in ("dense", "interpenetrating"):
        m = scenes()[name][0]
        a, b = run_device(dev, m), run_device(dev, m)
        assert_equal(a, b, EXACT, what=name)
        assert np.array_equal(a["rgb"], b["rgb"])


@pytest.mark.parametrize("name", ["dense", "interpenetrating", "duplicate"])
def test_face_order_and_orientation_decide_nothing(dev, name):
    m = scenes()[name][0]
    want = spec(name)
    kept = ("depth", "maskid", "winner", "counts")
    for other in (U.permuted(m), U.reversed_faces(m), U.reversed_faces(U.permuted(m, seed=9))):
        got = run_device(dev, other)
        assert_equal(got, want, kept, what=name)
        assert np.array_equal(got["stats"], want["stats"])                    # (the same faces, each in its own category)


def test_range_checks(dev):
    m = scenes()["coarse"][0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    verts, faces, foff, hide, T = t(m["verts"]), t(m["faces"]), t(m["face_off"]), t(m["hide"]), t(m["T_CW"])
    vis = lambda **kw: ops.raster_visibility(kw.get("verts", verts), kw.get("faces", faces), kw.get("foff", foff),
                                             kw.get("hide", hide), kw.get("T", T), kw.get("intr", m["intr"]), kw.get("W", 70),
                                             kw.get("H", 45), kw.get("z_near", 0.05), ws=kw.get("ws"))
    for kw in ({"verts": verts.float()}, {"verts": verts.cpu()}, {"faces": faces.long()}, {"hide": hide[:0]}, {"T": T[:2]},
               {"T": T.float()}, {"W": 0}, {"H": 65537}, {"z_near": 0.0}, {"z_near": float("nan")}, {"intr": (1.0, 2.0, 3.0)},
               {"ws": torch.empty(16, dtype=torch.uint8, device=dev)}, {"foff": foff[:0]}, {"verts": verts[:, :2]}):
        with pytest.raises((_lib.ObjnerfError, ValueError)):
            vis(**kw)
    key, stats, status, ws = vis()
    ids, col = t(m["ids"]), t(m["colors"])
    res = lambda **kw: ops.raster_resolve(verts, faces, foff, kw.get("ids", ids), kw.get("col", col), kw.get("ws", ws),
                                          kw.get("key", key), kw.get("cam", m["cam"]), kw.get("ambient", 0.35), True,
                                          kw.get("bg", (255, 255, 255)))
    for kw in ({"ids": ids.long()}, {"col": col[:-1]}, {"col": col.double()}, {"ws": ws[:16]}, {"key": key.int()},
               {"key": key.reshape(-1)}, {"cam": (0.0, 1.0)}, {"ambient": 1.5}, {"bg": (0, 0, 256)}):
        with pytest.raises((_lib.ObjnerfError, ValueError)):
            res(**kw)
    assert ops.raster_workspace_bytes(-1, 0) == 0 and ops.raster_workspace_bytes(0, 2 ** 31) == 0
    assert ops.raster_workspace_bytes(100, 10) >= 100 * 16 + 10 * 4


# ------------------------------------------------------------------------------------- 3. MapRaster on the planted map
@pytest.fixture(scope="module")
def planted():
    all_obj, Xs, q, info = RU.planted_map()
    return all_obj, PU.dense_of(all_obj, Xs), q, info


POSE = U.look_at((2.6, 0.42, -1.0), (2.6, 0.42, 0.4), up=(0.0, -1.0, 0.0))
SIZE = (70, 45)


def planted_scene(mq, colors, hide=(0, 0)):
    verts, faces, face_off, _ = mq.mesh_buffers()
    m = {"verts": verts.cpu().numpy(), "faces": faces.cpu().numpy(), "face_off": face_off.cpu().numpy()}
    m.update(T_WC=POSE, T_CW=U.world_to_camera(POSE), cam=POSE[:3, 3], W=SIZE[0], H=SIZE[1], intr=U.INTR0, z_near=0.05,
             ids=np.asarray(mq.keys, np.int32), hide=np.asarray(hide, np.uint8), colors=colors.cpu().numpy())
    return m


def test_map_raster_end_to_end(dev, planted):
    from openobj_amd import map_view_eval
    compact, dense, q, info = planted
    p, k = info["position"], info["key"]
    mq = query.MapQuery(dense, dev)
    mr = map_raster.MapRaster(mq)
    col = mq.color_by_part_query(info["clip_query"], info["sbert_query"], q, 1)
    buf = mr.render(POSE, U.INTR0, *SIZE, colors=col)
    want = U.run_spec(planted_scene(mq, col))
    assert 4 * int((want["winner"] >= 0).sum()) >= SIZE[0] * SIZE[1] and (want["winner"] < 0).any()
    assert buf.rgb.shape == (70, 45, 3) and buf.rgb.dtype == np.uint8 and buf.maskid.dtype == np.int32 and buf.depth.dtype == np.float32
    assert np.array_equal(buf.maskid, want["maskid"]) and np.array_equal(buf.depth.view(np.uint32), want["depth"].view(np.uint32))
    assert np.abs(buf.rgb.astype(np.int32) - want["rgb"]).max() <= 1
    last = {n: v.cpu().numpy() for n, v in mr.last.items()}
    for n in ("winner", "face", "vertex", "counts", "stats"):
        assert np.array_equal(last[n], want[n]), n
    assert set(np.unique(buf.maskid)) == {0, k} and mr.visible() == {k: int(want["counts"][p])}
    assert mr.visible(min_pixels=10 ** 6) == {}
    # pick: a pixel over each blob centre leads back to the vertex, its part feature and its region
    reg = mq.part_regions(q, min_cos=0.5)
    X, Y, _, _ = map_raster.project_vertices(np.array(info["centres"]), U.world_to_camera(POSE), U.INTR0)
    px = np.stack([np.rint(X / 256.0), np.rint(Y / 256.0)], axis=1).astype(np.int64)
    pk = mr.pick(np.concatenate([px, [[0, 0], [-3, 5], [70, 0]]]))
    assert pk["key"].tolist() == [k, k, -1, -1, -1] and pk["object"].tolist() == [p, p, -1, -1, -1]
    assert pk["face"][2:].tolist() == [-1] * 3 and pk["vertex"][2:].tolist() == [-1] * 3 and np.isnan(pk["point"][2:]).all()
    assert np.all(pk["depth"][2:] == 100)
    for i in range(2):
        w, h = px[i]
        assert pk["face"][i] == want["face"][w, h] and pk["vertex"][i] == want["vertex"][w, h]
        assert np.array_equal(pk["point"][i], want["point"][w, h]) and pk["depth"][i] == want["depth"][w, h]
        assert np.linalg.norm(pk["point"][i] - np.array(info["centres"][i])) <= RU.CELL
    feats = mq.features(pk["vertex"][:2]).cpu().numpy().astype(np.float64)
    cos = feats @ q / np.linalg.norm(feats, axis=1)
    assert np.all(cos > 0.8)                                                   # 0.894 at a centre, ~0 far from both
    labels = reg.label.cpu().numpy()[pk["vertex"][:2]]
    assert np.all(labels >= 0) and labels[0] != labels[1]
    # the device dict goes into ViewEval as MapView's does
    view = mr.render(POSE, U.INTR0, *SIZE, colors=col, to_host=False)
    assert {"rgb", "maskid", "depth", "winner", "face", "vertex", "counts", "stats", "status"} <= set(view)
    ev = map_view_eval.ViewEval([k], dev)
    ev.add(view, {"image": buf.rgb, "depth": buf.depth, "obj": buf.maskid})
    res = ev.result()                                                         # the view against its own read-back
    assert res["frames"] == 1 and res["image"]["psnr"] == float("inf") and res["per_id"][k]["iou"] == pytest.approx(1.0)    # hiding the planted object by position; the compact map; default colours; ids by class
    hid = mr.render(POSE, U.INTR0, *SIZE, colors=col, hide=[p])
    assert np.all(hid.maskid == 0) and np.all(hid.depth == 100) and mr.visible() == {}
    mc = map_raster.MapRaster(query.MapQuery(compact, dev))
    b2 = mc.render(POSE, U.INTR0, *SIZE, ids="class", shading="none", background=(0, 0, 0))
    assert np.array_equal(b2.depth, buf.depth) and set(np.unique(b2.maskid)) == {0, 1}
    rgb = U.run_spec(planted_scene(mq, mq.color_by_rgb()), shading=False, background=(0, 0, 0))["rgb"]
    assert np.abs(b2.rgb.astype(np.int32) - rgb).max() <= 1
    with pytest.raises(ValueError):
        mr.render(POSE, U.INTR0, *SIZE, colors=col[:-1])
    with pytest.raises(ValueError):
        mr.render(POSE, U.INTR0, *SIZE, shading="phong")


def test_cli(dev, planted, tmp_path):
    from PIL import Image
    compact, dense, q, info = planted
    k = info["key"]
    log = tmp_path / "log"
    os.makedirs(log)
    with gzip.open(log / "map_vis.pkl.gz", "wb") as fh:
        pickle.dump(dense, fh)
    np.savetxt(tmp_path / "pose.txt", POSE)
    for n, v in (("c", info["clip_query"]), ("s", info["sbert_query"]), ("p", q.astype(np.float32))):
        np.save(tmp_path / f"{n}.npy", v)
    doc = map_raster.main(["--logdir", str(log), "--mode", "part", "--clip-query", str(tmp_path / "c.npy"), "--sbert-query",
                           str(tmp_path / "s.npy"), "--part-query", str(tmp_path / "p.npy"), "--device", str(dev), "--pose",
                           str(tmp_path / "pose.txt"), "--size", "70", "45", "--intrinsics", *[str(x) for x in U.INTR0],
                           "--depth-scale", "1000", "--out", str(tmp_path / "out")])
    assert set(os.listdir(tmp_path / "out")) == {"rgb_0.png", "depth_0.png", "maskid_0.png", "visible.json"}
    mq = query.MapQuery(dense, dev)
    want = U.run_spec(planted_scene(mq, mq.color_by_part_query(info["clip_query"], info["sbert_query"], q, 1)))
    rgb = np.asarray(Image.open(tmp_path / "out" / "rgb_0.png"))
    mid = np.asarray(Image.open(tmp_path / "out" / "maskid_0.png"))
    dep = np.asarray(Image.open(tmp_path / "out" / "depth_0.png"))
    assert rgb.shape == (45, 70, 3) and np.abs(rgb.astype(np.int32) - want["rgb"].transpose(1, 0, 2)).max() <= 1
    assert np.array_equal(mid, want["maskid"].T.astype(np.uint8))
    assert np.array_equal(dep, np.clip(np.rint(want["depth"].astype(np.float64) * 1000), 0, 65535).astype(np.uint16).T)
    with open(tmp_path / "out" / "visible.json") as fh:
        assert json.load(fh) == doc
    fr = doc["frames"]
    assert len(fr) == 1 and fr[0]["frame"] == 0 and fr[0]["visible"] == [{"id": k, "pixels": int(want["counts"][1])}]
    assert fr[0]["stats"] == dict(zip(U.STATS, want["stats"].tolist())) and fr[0]["status"] == 0
