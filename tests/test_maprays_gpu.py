"""GPU: the ray caster (objnerf_maprays.hip) against the specification of tests/maprays_util.py.  Every
output of every ray is compared for EQUALITY (floats by their bits): key, t, hit, face, winner, maskid, vertex, bary,
point, normal, status and the rays / hits / bad-rays counters.  The hierarchy decides nothing: leaf sizes, traversal
orders, face orders and repeated builds give the same bytes.  MapRays and the CLI run end to end on a map of two planted
objects, one in front of the other."""
import copy
import functools
import gzip
import json
import os
import pickle

import numpy as np
import pytest
import torch

from openobj_amd import _lib, map_raster, map_rays, ops, query
try:
    from tests import maprays_util as U, mapraster_util as RU, mapregions_util as GU, partcompact_util as PU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import maprays_util as U
    import mapraster_util as RU
    import mapregions_util as GU
    import partcompact_util as PU

pytestmark = pytest.mark.gpu

SCENES = ("dense", "coarse", "interpenetrating", "giant", "on_samples", "duplicate", "zero_area", "nan", "hidden", "empty",
          "bad_index")
FIELDS = ("key", "t", "hit", "face", "winner", "maskid", "vertex", "bary", "point", "normal")


@functools.lru_cache(maxsize=None)
def scene(name):
    return U.scene_of(name)


@functools.lru_cache(maxsize=None)
def rays(name, n_each=300):
    """The pixel rays of the scene's camera plus the special rays: about 5 000."""
    return U.scene_rays(scene(name), n_each=n_each)


@functools.lru_cache(maxsize=None)
def spec(name):
    """The specification of a scene over its rays, computed once and shared (nothing changes it)."""
    o, d = rays(name)
    return U.run_spec(scene(name), o, d)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


class Device:
    """A scene on the device with its hierarchy."""

    def __init__(self, dev, m, leaf=-1, pad=None):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.dev, self.m, self.leaf = dev, m, leaf
        self.verts, self.faces, self.foff = t(np.asarray(m["verts"], np.float64).reshape(-1, 3)), t(np.asarray(m["faces"], np.int32).reshape(-1, 3)), t(m["face_off"])
        self.ids, self.hide = t(m["ids"]), t(m["hide"])
        self.pad = U.default_pad(m["verts"]) if pad is None else pad
        assert pad is not None or ops.rays_default_pad(self.verts) == self.pad
        self.ws, self.build_status = ops.rays_build(self.verts, self.faces, self.foff, self.pad, leaf)

    def nodes(self):
        n = ops.rays_node_count(len(self.m["faces"]), self.leaf) * ops.RAYS_NODE_BYTES
        return self.ws[:n].cpu().numpy()

    def cast(self, o, d, t_min=0.0, t_max=float("inf"), hide=None, any_hit=False, fixed=False):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        win = [t(w) if isinstance(w, np.ndarray) else w for w in (t_min, t_max)]
        od, dd = t(o), t(d)
        key, stats, status = ops.rays_cast(self.verts, self.faces, self.foff, self.hide if hide is None else t(hide), self.ws,
                                           self.pad, od, dd, win[0], win[1], self.leaf, any_hit, self.build_status.clone(),
                                           _fixed_order=fixed)
        if any_hit:
            return {"hit": key.cpu().numpy(), "stats": stats.cpu().numpy(), "status": int(status.item())}
        out = {k: v.cpu().numpy() for k, v in ops.rays_resolve(self.verts, self.faces, self.foff, self.ids, od, dd, key).items()}
        out.update(key=key.cpu().numpy().view(np.uint64), stats=stats.cpu().numpy(), status=int(status.item()))
        return out


def assert_equal(got, want, what=""):
    for k in FIELDS:
        a, b = bits(got[k]), bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {k} differs at {int((a != b).sum())} places"
    assert got["status"] == want["status"], what
    assert got["stats"][:3].tolist() == want["counters"].tolist(), what


# -------------------------------------------------------------------------------------------- 1. the scenes, every ray
@pytest.mark.parametrize("name", SCENES)
def test_scene_equals_the_specification(dev, name):
    m, (o, d), want = scene(name), rays(name), spec(name)
    n_hit, n_bad = int(want["hit"].sum()), int(U.bad_rays(o, d).sum())
    # from the specification alone: what the scene and its rays exercise
    assert len(m["faces"]) <= 2886 + 2 and 3000 <= len(o) <= 5400 and want["counters"][2] == n_bad >= 7 and want["status"] & 2
    if name == "empty":
        assert n_hit == 0 and np.all(want["face"] == -1) and np.all(np.isinf(want["t"])) and np.all(want["maskid"] == 0)
    else:
        assert n_hit > len(o) // 2 and n_hit < len(o)
        assert (want["t"].view(np.uint32) == 0).any()                 # origins on faces: t = +0
    assert (want["status"] & 1) == (name == "bad_index")
    if name == "duplicate":
        assert np.all(want["winner"][want["hit"] != 0] == 0)          # two identical sheets: the lowest face id wins
    if name == "hidden":
        assert np.all(want["winner"] <= 0)
    s = Device(dev, m)
    got = s.cast(o, d)
    assert_equal(got, want, name)
    fixed = s.cast(o, d, fixed=True)
    assert_equal(fixed, want, name + " (fixed order)")
    for f in (False, True):                                           # any-hit: whether a key exists
        a = s.cast(o, d, any_hit=True, fixed=f)
        assert np.array_equal(a["hit"], want["hit"]) and a["status"] == want["status"]
        assert a["stats"][:3].tolist() == want["counters"].tolist()
        assert a["stats"][3] <= got["stats"][3] or f
    print(f"{name}: {len(m['faces'])} faces, {len(o)} rays, {n_hit} hit; a ray visits {got['stats'][3] / len(o):.1f} nodes and "
          f"tests {got['stats'][4] / len(o):.1f} faces nearer child first, {fixed['stats'][3] / len(o):.1f} and "
          f"{fixed['stats'][4] / len(o):.1f} in fixed order")


@pytest.mark.parametrize("name", ["dense", "interpenetrating", "coarse", "hidden", "nan"])
def test_windows_and_segments(dev, name):
    """Windows that cut off the first hit, a per-ray t_max, a scalar window, segments (d = b - a, window [0, 1])."""
    m = scene(name)
    o, d = rays(name, 100)
    sel = np.arange(0, len(o), 3)
    o, d = o[sel], d[sel]
    first = U.run_spec(m, o, d)
    s = Device(dev, m)
    rs = np.random.RandomState(3)
    t_first = np.where(first["hit"] != 0, first["t"].astype(np.float64), 1.0)
    cut = np.nextafter(t_first, np.inf) * (1.0 + 1e-6)                                # just behind the first hit
    t_max = np.where(rs.rand(len(o)) < 0.5, t_first * rs.uniform(0.5, 1.5, len(o)), np.inf)
    t_max[::7] = t_first[::7]                                                         # exactly the fp32 t of the hit
    cases = ((cut, np.inf), (0.0, t_max), (cut, np.maximum(t_max, cut) * 1.5), (float(np.median(t_first)), float(np.median(t_first)) * 1.2))
    changed = 0
    for t0, t1 in cases:
        want = U.run_spec(m, o, d, t0, t1)
        changed += int((want["key"] != first["key"]).sum())
        assert_equal(s.cast(o, d, t0, t1), want, name)
        assert np.array_equal(s.cast(o, d, t0, t1, any_hit=True)["hit"], want["hit"])
    assert changed > len(o) // 2                                                      # (the windows do cut hits off)
    a, ab = U.segments_of(m, 400)
    want = U.run_spec(m, a, ab, 0.0, 1.0)
    assert 0 < want["hit"].sum() < len(a)
    assert_equal(s.cast(a, ab, 0.0, 1.0), want, name + " segments")
    assert np.array_equal(s.cast(a, ab, 0.0, 1.0, any_hit=True)["hit"], want["hit"])


def test_no_pad(dev):
    """pad = 0: a parallel axis of a ray through a vertex lies exactly on the faces of the boxes around it."""
    m = scene("coarse")
    o, d = U.special_rays(m)
    want = U.run_spec(m, o, d, pad=0.0)
    assert 0 < want["hit"].sum() < len(o)
    for leaf in (1, 4):
        assert_equal(Device(dev, m, leaf, pad=0.0).cast(o, d), want, f"leaf {leaf}")


# --------------------------------------------------------------------------------------- 2. the hierarchy decides nothing
@pytest.mark.parametrize("name", ["dense", "interpenetrating", "bad_index"])
def test_leaf_size_leaves_the_bytes_alone(dev, name):
    m, (o, d), want = scene(name), rays(name), spec(name)
    visits = {}
    for leaf in (1, 4, 8, len(m["faces"]) + 1):
        s = Device(dev, m, leaf)
        got = s.cast(o, d)
        assert_equal(got, want, f"{name} leaf {leaf}")
        assert_equal(s.cast(o, d, fixed=True), want, f"{name} leaf {leaf} (fixed order)")
        visits[leaf] = int(got["stats"][3])
    assert visits[len(m["faces"]) + 1] == len(o) - int(U.bad_rays(o, d).sum())      # one node: the root is the only leaf
    assert visits[1] > visits[8] > visits[len(m["faces"]) + 1]


@pytest.mark.parametrize("name", ["dense", "duplicate"])
def test_face_order_and_orientation(dev, name):
    """Permuted and reversed faces equal the specification of the permuted mesh; under a permutation alone, what does
    not name a face equals the original's."""
    m, (o, d), base = scene(name), rays(name), spec(name)
    sel = np.arange(0, len(o), 3)
    o, d = o[sel], d[sel]
    for n, other in enumerate((RU.permuted(m), RU.reversed_faces(m), RU.reversed_faces(RU.permuted(m, seed=9)))):
        want = U.run_spec(other, o, d)
        assert_equal(Device(dev, other).cast(o, d), want, name)
        for k in ("hit", "t", "winner", "maskid") if n == 0 else ():  # (another corner order rounds otherwise)
            assert np.array_equal(bits(want[k]), bits(base[k][sel])), k


def test_two_builds_and_two_casts_give_the_same_bytes(dev):
    for name in ("dense", "interpenetrating"):
        m, (o, d) = scene(name), rays(name)
        a, b = Device(dev, m), Device(dev, m)
        na, nb = a.nodes(), b.nodes()
        assert len(na) == ops.rays_node_count(len(m["faces"])) * 32 and np.array_equal(na, nb)
        assert np.array_equal(a.ws.cpu().numpy(), b.ws.cpu().numpy())
        boxes = na.view(np.float32).reshape(-1, 8)
        assert np.all(boxes[1, :3] <= boxes[1, 3:6]) and np.isfinite(boxes[1, :6]).all()        # the root holds the scene
        lo, hi = np.asarray(m["verts"]).min(axis=0), np.asarray(m["verts"]).max(axis=0)
        assert np.all(boxes[1, :3] <= lo) and np.all(boxes[1, 3:6] >= hi)
        x, y = a.cast(o, d), a.cast(o, d)
        for k in FIELDS + ("stats",):
            assert np.array_equal(bits(x[k]), bits(y[k])), k
        z = b.cast(o, d)
        for k in FIELDS + ("stats",):
            assert np.array_equal(bits(x[k]), bits(z[k])), k


def test_hide_changes_without_a_rebuild(dev):
    m = scene("hidden")                                                # object 1 lies in front and is hidden
    o, d = rays("hidden")
    s = Device(dev, m)
    nodes = s.nodes().copy()
    seen = set()
    for hide in ([0, 1], [0, 0], [1, 0], [1, 1], [0, 1]):
        want = U.run_spec(m, o, d, hide=np.array(hide, np.uint8))
        assert_equal(s.cast(o, d, hide=np.array(hide, np.uint8)), want, str(hide))
        seen.add(tuple(np.unique(want["winner"]).tolist()))
    assert seen == {(-1, 0), (-1, 0, 1), (-1, 1), (-1,)}
    assert np.array_equal(s.nodes(), nodes)


def test_empty_inputs(dev):
    m = scene("coarse")
    s = Device(dev, m)
    none = s.cast(np.zeros((0, 3)), np.zeros((0, 3)))
    assert all(len(none[k]) == 0 for k in FIELDS) and none["stats"].tolist() == [0] * 5 and none["status"] == 0
    assert len(s.cast(np.zeros((0, 3)), np.zeros((0, 3)), any_hit=True)["hit"]) == 0
    e = Device(dev, scene("empty"))                                    # F = 0: one empty node
    assert ops.rays_node_count(0) == 2 and len(e.nodes()) == 64
    o, d = rays("empty")
    got = e.cast(o, d)
    assert_equal(got, spec("empty"), "empty")
    assert got["stats"][3] == len(o) - int(U.bad_rays(o, d).sum()) and got["stats"][4] == 0


def test_range_checks(dev):
    m = scene("coarse")
    s = Device(dev, m)
    o, d = (torch.from_numpy(x).to(dev) for x in rays("coarse"))
    build = lambda **kw: ops.rays_build(kw.get("verts", s.verts), kw.get("faces", s.faces), kw.get("foff", s.foff),
                                        kw.get("pad", s.pad), kw.get("leaf", -1), ws=kw.get("ws"))
    for kw in ({"verts": s.verts.float()}, {"verts": s.verts.cpu()}, {"faces": s.faces.long()}, {"foff": s.foff[:0]},
               {"verts": s.verts[:, :2]}, {"pad": -1.0}, {"pad": float("nan")}, {"pad": float("inf")}, {"leaf": 0},
               {"ws": torch.empty(16, dtype=torch.uint8, device=dev)}):
        with pytest.raises((_lib.ObjnerfError, ValueError)):
            build(**kw)
    cast = lambda **kw: ops.rays_cast(s.verts, s.faces, s.foff, kw.get("hide", s.hide), kw.get("ws", s.ws), kw.get("pad", s.pad),
                                      kw.get("o", o), kw.get("d", d), kw.get("t_min", 0.0), kw.get("t_max", 1.0), kw.get("leaf", -1))
    for kw in ({"hide": s.hide[:0]}, {"ws": s.ws[:16]}, {"o": o[:-1]}, {"o": o.float()}, {"d": d[:, :2]}, {"t_min": -1.0},
               {"t_min": float("nan")}, {"t_max": float("nan")}, {"t_min": torch.zeros(3, dtype=torch.float64, device=dev)},
               {"t_max": torch.zeros(len(o), dtype=torch.float32, device=dev)}, {"leaf": 1}, {"pad": -1.0}):
        with pytest.raises((_lib.ObjnerfError, ValueError)):
            cast(**kw)
    key = cast()[0]
    for kw in ({"ids": s.ids.long()}, {"ids": s.ids[:0]}, {"key": key[:-1]}, {"key": key.int()}):
        with pytest.raises((_lib.ObjnerfError, ValueError)):
            ops.rays_resolve(s.verts, s.faces, s.foff, kw.get("ids", s.ids), o, d, kw.get("key", key))
    assert ops.rays_workspace_bytes(-1) == 0 and ops.rays_workspace_bytes(2 ** 31) == 0 and ops.rays_workspace_bytes(10, 0) == 0
    assert ops.rays_workspace_bytes(10, 4) == 512 and ops.rays_workspace_bytes(100, 1) >= 256 * 32 + 100 * 8
    # status is OR-ed into the caller's word
    st = torch.tensor([4], dtype=torch.int32, device=dev)
    ops.rays_cast(s.verts, s.faces, s.foff, s.hide, s.ws, s.pad, o, d, status=st)
    assert int(st.item()) == 6


def test_raster_and_rays_name_the_same_face(dev):
    """On the `coarse` scene and its camera the rasteriser's visibility and the caster's keys, both from the device, name
    the same face at every pixel (the two specifications do: tests/test_maprays.py)."""
    m = scene("coarse")
    s = Device(dev, m)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    key, _, _, ws = ops.raster_visibility(s.verts, s.faces, s.foff, s.hide, t(m["T_CW"]), m["intr"], m["W"], m["H"], m["z_near"])
    ras = ops.raster_resolve(s.verts, s.faces, s.foff, s.ids, t(m["colors"]), ws, key, m["cam"])
    o, d = map_rays.view_rays(m["T_WC"], m["intr"], m["W"], m["H"])
    got = s.cast(o, d, t_min=m["z_near"])
    face = ras["face"].cpu().numpy().reshape(-1)
    assert (face >= 0).sum() * 2 > len(face) and np.array_equal(got["face"], face)
    assert np.array_equal(got["winner"], ras["winner"].cpu().numpy().reshape(-1))


# -------------------------------------------------------------------------- 3. MapRays on a map of two planted objects
POSE = RU.look_at((2.6, 0.42, -1.0), (2.6, 0.42, 0.4), up=(0.0, -1.0, 0.0))
SIZE = (70, 45)


@pytest.fixture(scope="module")
def planted():
    """The two-object map of test_mapraster_gpu.py with object 0 (key 10) moved in front of the first blob of object 1
    (key 13), as seen from POSE: its sheet spans x 2.0 .. 2.55, y 0 .. 0.4 at z = 0; the planted sheet lies at z = 0.4."""
    all_obj, Xs, q, info = GU.planted_map()
    all_obj = copy.deepcopy(all_obj)
    all_obj[10]["mesh"].apply_translation((2.0, 0.0, -0.4))
    return PU.dense_of(all_obj, Xs), q, info


def planted_scene(mq):
    verts, faces, face_off, _ = mq.mesh_buffers()
    return {"verts": verts.cpu().numpy(), "faces": faces.cpu().numpy(), "face_off": face_off.cpu().numpy(), "T_WC": POSE,
            "T_CW": RU.world_to_camera(POSE), "cam": POSE[:3, 3], "W": SIZE[0], "H": SIZE[1], "intr": RU.INTR0, "z_near": 0.05,
            "ids": np.asarray(mq.keys, np.int32), "hide": np.zeros(2, np.uint8)}


def test_map_rays_end_to_end(dev, planted):
    dense, q, info = planted
    p, k = info["position"], info["key"]
    mq = query.MapQuery(dense, dev)
    mr = map_rays.MapRays(mq)
    m = planted_scene(mq)
    assert mr.pad == U.default_pad(m["verts"]) and mr.leaf == 4
    c = np.array(info["centres"])                                      # blob 0 lies behind object 0, blob 1 beside it
    eye = np.array([[2.3, 0.3, -1.0], [2.9, 0.6, -1.0]])
    # cast: a ray at each blob centre -> vertex -> the part feature and the region
    r = mr.cast(eye, c - eye, hide=[0])
    assert r["hit"].all() and r["winner"].tolist() == [p, p] and r["maskid"].tolist() == [k, k] and r["status"] == 0
    assert np.abs(r["point"] - c).max() < 1e-9 and np.abs(r["t"] - 1.0).max() < 1e-6
    assert np.allclose(r["normal"], [[0.0, 0.0, -1.0]] * 2) and r["stats"]["rays"] == 2 and r["stats"]["hits"] == 2
    feats = mq.features(r["vertex"]).cpu().numpy().astype(np.float64)
    assert np.all(feats @ q / np.linalg.norm(feats, axis=1) > 0.8)                  # 0.894 at a centre, ~0 far from both
    labels = mq.part_regions(q, min_cos=0.5).label.cpu().numpy()[r["vertex"]]
    assert np.all(labels >= 0) and labels[0] != labels[1]
    verts = m["verts"]
    assert np.linalg.norm(verts[r["vertex"]] - c, axis=1).max() <= GU.CELL
    # the whole dict against the specification, ids by class
    o, d = map_rays.view_rays(POSE, RU.INTR0, *SIZE)
    want = U.run_spec(m, o, d, ids=[0, 1])
    got = mr.cast(o, d, ids="class", to_host=False)
    for f in FIELDS:
        assert np.array_equal(bits(got[f].cpu().numpy().view(np.uint64) if f == "key" else got[f].cpu().numpy().astype(want[f].dtype)),
                              bits(want[f])), f
    assert set(np.unique(want["winner"]).tolist()) == {-1, 0, 1}
    # occluded and sees: blob 0 lies behind object 0, blob 1 does not
    short, far = eye + (c - eye) * 0.99, eye + (c - eye) * 1.01        # (a segment that ends ON the sheet: t = 1 up to rounding)
    assert mr.occluded(eye, far).tolist() == [True, True]
    assert mr.occluded(eye, short).tolist() == [True, False] and mr.occluded(eye, short, hide=[0]).tolist() == [False, False]
    assert mr.occluded(eye, far, hide=[0, 1]).tolist() == [False, False]
    assert mr.sees(eye, c, [p, p]).tolist() == [False, True]
    assert mr.sees(eye, c, [p, p], hide=[0]).tolist() == [True, True] and mr.sees(eye, far, [0, 0]).tolist() == [True, False]
    assert mr.sees(eye, short, [p, p]).tolist() == [False, True]
    # against MapRaster on the same view: the two name the same face wherever their specifications do
    view = map_raster.MapRaster(mq).render(POSE, RU.INTR0, *SIZE, to_host=False)
    key, _, _ = RU.visibility(m, m["T_CW"], m["intr"], *SIZE, m["z_near"], m["hide"])
    key = RU.key_array(key).reshape(-1)
    ras = np.where(key != U.EMPTY, key & np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFFFF)).astype(np.uint32).astype(np.int32)
    near = U.run_spec(m, o, d, t_min=0.05)
    agree = ras == near["face"]
    assert agree.sum() >= len(agree) - 30                              # (a sample exactly on an edge: the snapped vertices decide)
    face = mr.cast(o, d, t_min=0.05, to_host=False)["face"]
    assert torch.equal(face[torch.from_numpy(agree).to(dev)], view["face"].reshape(-1)[torch.from_numpy(agree).to(dev)])
    with pytest.raises(ValueError):
        mr.cast(o, d[:-1])
    with pytest.raises(ValueError):
        mr.cast(o, d, t_min=-1.0)
    with pytest.raises(ValueError):
        mr.sees(eye, c, [p])
    with pytest.raises(ValueError):
        map_rays.MapRays(mq, leaf=0)


def test_cli(dev, planted, tmp_path):
    dense, q, info = planted
    log = tmp_path / "log"
    os.makedirs(log)
    with gzip.open(log / "map_vis.pkl.gz", "wb") as fh:
        pickle.dump(dense, fh)
    mq = query.MapQuery(dense, dev)
    m = planted_scene(mq)
    T = np.eye(4)
    T[:3, 3] = (2.6, 0.42, -0.5)
    np.savetxt(tmp_path / "pose.txt", T)
    r = map_rays.main(["cast", "--logdir", str(log), "--device", str(dev), "--lidar", str(tmp_path / "pose.txt"), "--beams", "16",
                       "9", "40", "90", "--out", str(tmp_path / "out")])
    assert set(os.listdir(tmp_path / "out")) == {"hits.npz", "hits.ply"}
    o, d = map_rays.lidar_rays(T, 16, 9, 40.0, 90.0)
    want = U.run_spec(m, o, d)
    z = np.load(tmp_path / "out" / "hits.npz")
    assert 0 < want["hit"].sum() < len(o) and np.array_equal(z["hit"], want["hit"] != 0)
    for f in ("t", "face", "winner", "maskid", "vertex", "bary", "point"):
        assert np.array_equal(bits(z[f]), bits(want[f])) and np.array_equal(bits(r[f]), bits(want[f])), f
    lines = open(tmp_path / "out" / "hits.ply").read().splitlines()
    assert f"element vertex {int(want['hit'].sum())}" in lines
    rgb = np.round(mq.color_by_rgb().cpu().numpy().astype(np.float64)[want["vertex"][want["hit"] != 0]] * 255).astype(int)
    first = lines[lines.index("end_header") + 1].split()
    assert [float(x) for x in first[:3]] == want["point"][want["hit"] != 0][0].tolist() and [int(x) for x in first[3:]] == rgb[0].tolist()
    np.save(tmp_path / "rays.npy", np.concatenate([o, d], axis=1))
    r2 = map_rays.main(["cast", "--logdir", str(log), "--device", str(dev), "--rays", str(tmp_path / "rays.npy"), "--out",
                        str(tmp_path / "out2"), "--hide", "0", "--t-max", "2.0"])
    assert np.array_equal(r2["face"], U.run_spec(m, o, d, 0.0, 2.0, hide=np.array([1, 0], np.uint8))["face"])
    # sight: object 13's goal under its first blob is blocked by object 10; beside it, it is seen
    nav = {"objects": [{"id": 13, "goal": [2.32, 0.31, -1.0]}, {"id": 10, "goal": [2.32, 0.31, -1.0]}, {"id": 13, "goal": None}]}
    with open(tmp_path / "nav.json", "w") as fh:
        json.dump(nav, fh)
    doc = map_rays.main(["sight", "--logdir", str(log), "--device", str(dev), "--nav", str(tmp_path / "nav.json"), "--eye-height",
                         "0.2", "--out", str(tmp_path / "out3")])
    with open(tmp_path / "out3" / "sight.json") as fh:
        assert json.load(fh) == doc
    assert [x["sees"] for x in doc["objects"]] == [False, True, None] and doc["objects"][0]["blocker"] == 10
    assert doc["objects"][0]["eye"] == [2.32, 0.31, -0.8] and doc["objects"][0]["target"] == pytest.approx([2.3, 0.3, 0.4])
    doc = map_rays.main(["sight", "--logdir", str(log), "--device", str(dev), "--nav", str(tmp_path / "nav.json"), "--hide", "0",
                         "--out", str(tmp_path / "out3")])
    assert [x["sees"] for x in doc["objects"]] == [True, True, None]
