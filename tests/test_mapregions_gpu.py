"""GPU: the part regions (objnerf_mapregions.hip) against the specification of tests/mapregions_util.py.
Labels, offsets and every int64 of the table are compared for EQUALITY; the naive float path bounds the table from the
outside; MapQuery.part_regions and the CLI run end to end on a map with two planted blobs."""
import gzip
import json
import os
import pickle

import numpy as np
import pytest
import torch

from openobj_amd import _lib, map_regions as mr, ops, query
try:
    from tests import mapregions_util as U, partcompact_util as PU, query_util as QU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import mapregions_util as U
    import partcompact_util as PU
    import query_util as QU

pytestmark = pytest.mark.gpu

Q_COLS, Q_USED = 3, 1                   # the similarity is column 1 of 3: the row stride is exercised


# ------------------------------------------------------------------------------------------------------------ inputs
def five_objects(seed=0, scale=0.05, offset=50.0):
    """The five-object map: a 64 x 64 sheet, an empty object, a one-vertex object without a face, a 5-vertex object, a
    33 x 7 sheet offset by 50 m (so the anchor matters).  Coordinates from a seeded generator: the sheet's grid plus a
    jitter of a third of a cell, a random height; a few metres across."""
    rs = np.random.RandomState(seed)

    def sheet_obj(w, h, shift):
        x, y = U.sheet_xy(w, h)
        v = np.stack([x * scale, y * scale, np.zeros(w * h)], axis=1) + rs.uniform(-scale / 3, scale / 3, (w * h, 3))
        return v + shift, U.sheet(w, h)
    none = np.zeros((0, 3), np.int64)
    return [sheet_obj(64, 64, [0.3, -1.2, 0.7]), (np.zeros((0, 3)), none), (rs.rand(1, 3) * 3, none),
            (rs.rand(5, 3) * 3, np.array([(0, 1, 2), (2, 3, 4)])), sheet_obj(33, 7, [offset, 1.0, -2.0])]


def selection(name):
    """Per object a bool array over the ORIGINAL vertex order."""
    x0, y0 = U.sheet_xy(64, 64)
    x4, y4 = U.sheet_xy(33, 7)
    one, five = np.ones(1, bool), np.ones(5, bool)
    if name == "stripes":
        return [x0 % 4 < 2, np.zeros(0, bool), one, np.arange(5) % 2 == 0, x4 % 4 < 2]
    if name == "checkerboard":          # the sheet's diagonal joins (x, y) and (x + 1, y + 1): every other vertex both ways
        return [(x0 % 2 == 0) & (y0 % 2 == 0), np.zeros(0, bool), one, np.array([1, 0, 0, 0, 1], bool),
                (x4 % 2 == 0) & (y4 % 2 == 0)]
    if name == "all":
        return [np.ones(4096, bool), np.zeros(0, bool), one, five, np.ones(231, bool)]
    if name == "none":
        return [np.zeros(4096, bool), np.zeros(0, bool), ~one, ~five, np.zeros(231, bool)]
    if name == "spiral":
        return [U.spiral(64, 64).reshape(-1), np.zeros(0, bool), one, five, U.spiral(33, 7).reshape(-1)]
    raise KeyError(name)


def sims_of(col, rs=None):
    """[V, Q_COLS] fp32 with `col` in column Q_USED and decoys (that would select differently) in the others."""
    col = np.asarray(col, np.float32)
    s = np.zeros((len(col), Q_COLS), np.float32)
    s[:, 0], s[:, 2] = 1.0 - col, 5.0
    s[:, Q_USED] = col
    return s


def run_device(dev, m, sims, thr, q=Q_USED, table=True):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    voff, foff, faces, sd = t(m["vert_off"]), t(m["face_off"]), t(m["faces"]), t(sims)
    root, label, reg_off, status = ops.regions_label(voff, foff, faces, sd, q, t(np.asarray(thr, np.float32)))
    out = {"root": root.cpu().numpy(), "label": label.cpu().numpy(), "reg_off": reg_off.cpu().numpy()}
    if table:
        R = int(out["reg_off"][-1])
        out["table"] = ops.regions_table(voff, foff, t(m["verts"]), faces, sd, q, root, label, R, status).cpu().numpy()
    out["status"] = int(status.item())
    return out


def spec(m, sims, thr, q=Q_USED, table=True):
    sel = U.selected(sims[:, q], thr, m["vert_off"])
    root, status = U.components(m, sel)
    reg_off, label = U.rows(root, m["vert_off"])
    out = {"root": root, "label": label, "reg_off": reg_off, "status": status}
    if table:
        out["table"], out["status"] = U.table(m, sims[:, q], root, label)
    return out


def assert_same(got, want, what=("root", "label", "reg_off", "table")):
    for k in what:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.nonzero(got[k] != want[k])
        assert len(bad[0]) == 0, f"{k}: {len(bad[0])} differ, first at {[int(b[0]) for b in bad]}: " \
                                 f"{got[k][tuple(b[0] for b in bad)]} != {want[k][tuple(b[0] for b in bad)]}"
    assert got["status"] == want["status"]


# ------------------------------------------------------------------------------------------------------ 1. labels
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("name", ["stripes", "checkerboard", "all", "none", "spiral"])
def test_labels_equal_the_specification(dev, name, permuted):
    m = U.pack(five_objects(), permute_seed=7 if permuted else None)
    sims = sims_of(U.per_vertex(m, selection(name)))
    thr = np.full(5, 0.5, np.float32)
    want = spec(m, sims, thr, table=False)
    n_reg = np.diff(want["reg_off"])
    if name == "checkerboard":          # every selected vertex is its own region: 64 rows in a wave of the vertex launch
        assert n_reg.tolist() == [1024, 0, 1, 2, 17 * 4]
    if name == "spiral":                # one region whose path crosses every workgroup of the sheet
        assert n_reg.tolist() == [1, 0, 1, 1, 1] and 1000 < (want["root"][:4096] >= 0).sum() < 3000
    if name == "none":
        assert want["reg_off"][-1] == 0
    got = run_device(dev, m, sims, thr, table=False)
    assert_same(got, want, ("root", "label", "reg_off"))


# ------------------------------------------------------------------------------------------------------ 2. tables
_CACHE = {}


def tables_case(dev, case):
    """(m, sims, thr, device result, specification), computed once per case and left unchanged."""
    if case in _CACHE:
        return _CACHE[case]
    rs = np.random.RandomState(11)
    if case == "soup":                  # 200 disjoint triangles, all selected: 64 lanes of the face launch, 64 rows
        v = rs.rand(600, 3) * 0.4 + [1.0, 2.0, 3.0]
        m = U.pack([(v, np.arange(600).reshape(-1, 3)), (rs.rand(4, 3), [(0, 1, 2), (1, 2, 3)])])
        col, thr = rs.randint(0, 4, len(m["verts"])) / 4.0, np.full(2, -1.0, np.float32)
    else:
        m = U.pack(five_objects(seed=3), permute_seed=5 if case == "random" else None)
        V = len(m["verts"])
        col = rs.randint(0, 6, V) / 5.0                               # exact ties, at the maximum too: the peak rule
        thr = np.full(5, 0.5 if case == "random" else -1.0, np.float32)     # "all": one region of 7938 faces on the sheet
    sims = sims_of(col)
    want = spec(m, sims, thr)
    got = run_device(dev, m, sims, thr)
    _CACHE[case] = (m, sims, thr, got, want)
    return _CACHE[case]


@pytest.mark.parametrize("case", ["random", "all", "soup"])
def test_tables_equal_the_specification(dev, case):
    m, sims, thr, got, want = tables_case(dev, case)
    t = want["table"]
    if case == "random":
        assert len(t) > 50 and (t[:, U.C_NF] > 0).sum() > 20
        peak_v = (~t[:, U.C_PEAK]) & 0xFFFFFFFF
        tied = [r for r in range(len(t)) if (sims[want["label"] == r, Q_USED] == sims[peak_v[r], Q_USED]).sum() > 1]
        assert len(tied) > 10                                           # the smallest-index rule decides these
        for r in tied[:10]:
            ids = np.nonzero((want["label"] == r) & (sims[:, Q_USED] == sims[peak_v[r], Q_USED]))[0]
            assert peak_v[r] == ids.min()
    if case == "all":
        assert t[0, U.C_NF] == 7938 >= 4000 and t[:, U.C_NF].tolist() == [7938, 0, 2, 384]
    if case == "soup":
        assert len(t) == 201 and np.all(t[:200, U.C_NF] == 1)
    assert want["status"] == 0
    assert_same(got, want)


# ------------------------------------------------------------------------------- 3. order and run independence
def test_face_order_and_repetition_leave_the_bytes_alone(dev):
    m, sims, thr, got, _ = tables_case(dev, "random")
    again = run_device(dev, m, sims, thr)
    shuffled = U.pack(five_objects(seed=3), permute_seed=5, shuffle_seed=21)
    assert np.array_equal(shuffled["verts"], m["verts"]) and not np.array_equal(shuffled["faces"], m["faces"])
    other = run_device(dev, shuffled, sims, thr)
    for o in (again, other):
        for k in ("root", "label", "reg_off", "table"):
            assert o[k].tobytes() == got[k].tobytes(), k
        assert o["status"] == got["status"] == 0


# ------------------------------------------------------------------------------------------------ 4. special inputs
def small_map():
    rs = np.random.RandomState(2)
    x, y = U.sheet_xy(9, 6)
    v = np.stack([x * 0.1, y * 0.1, 0.02 * rs.randn(54)], axis=1)
    return [(v, U.sheet(9, 6)), (v[:20] + [3.0, 0, 0], U.sheet(5, 4))]


def test_nan_selects_nothing(dev):
    m = U.pack(small_map())
    col = np.ones(len(m["verts"]), np.float32)
    col[[3, 4, 13, 22, 30]] = np.nan
    sims = sims_of(col)
    for thr in (np.array([0.5, np.nan], np.float32), np.array([np.nan, 0.5], np.float32)):
        got, want = run_device(dev, m, sims, thr), spec(m, sims, thr)
        assert_same(got, want)
        dead = 1 if np.isnan(thr[1]) else 0
        assert np.all(got["root"][m["vert_off"][dead]:m["vert_off"][dead + 1]] == -1)
        if dead == 1:
            assert np.all(got["root"][[3, 4, 13, 22, 30]] == -1) and (got["root"][:54] >= 0).sum() == 49


def test_repeated_vertex_joins_and_adds_no_area(dev):
    objs = small_map()
    v, f = objs[0]
    sel = np.zeros(54, bool)
    sel[[0, 1, 9, 10, 43, 44, 52, 53]] = True                       # two far corners of the sheet
    objs[0] = (v, np.concatenate([f, [(0, 0, 53)]]))
    m = U.pack(objs)
    sims = sims_of(np.concatenate([sel, np.zeros(20, bool)]))
    thr = np.full(2, 0.5, np.float32)
    got, want = run_device(dev, m, sims, thr), spec(m, sims, thr)
    assert want["reg_off"].tolist() == [0, 1, 1] and want["table"][0, U.C_NV] == 8 and want["table"][0, U.C_NF] == 5
    assert_same(got, want)
    plain = run_device(dev, U.pack(small_map()), sims, thr)
    assert plain["reg_off"].tolist() == [0, 2, 2]
    assert plain["table"][:, U.C_AREA].sum() == got["table"][0, U.C_AREA]      # the degenerate face added nothing


@pytest.mark.parametrize("bad,bit", [((2, 74 + 5, 3), 1), ((-3, 2, 3), 1), ((2, 3, 2 ** 31 - 1), 1), ((2, 3, 60), 2)])
def test_bad_faces_raise_status_and_are_ignored(dev, bad, bit):
    """An id outside [0, V) raises bit 0, an id of another object bit 1; the face joins nothing and adds nothing.  The
    vertex buffers are exactly V long, so a read through the bad id would be out of range."""
    m0 = U.pack(small_map())
    m = dict(m0, faces=np.insert(m0["faces"], 40, bad, axis=0).astype(np.int32), face_off=m0["face_off"] + [0, 1, 1])
    assert len(m["verts"]) == 74 and len(m["faces"]) == len(m0["faces"]) + 1 and tuple(m["faces"][40]) == bad
    sims = sims_of(np.ones(74, np.float32))
    thr = np.full(2, 0.5, np.float32)
    got, want = run_device(dev, m, sims, thr), spec(m, sims, thr)
    assert want["status"] == bit
    assert_same(got, want)
    clean = run_device(dev, m0, sims, thr)
    assert clean["status"] == 0 and clean["table"].tobytes() == got["table"].tobytes()


def test_range_checks(dev):
    m = U.pack(small_map())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    voff, foff, faces = t(m["vert_off"]), t(m["face_off"]), t(m["faces"])
    thr = t(np.full(2, 0.5, np.float32))
    ok = torch.ones(74, 16, device=dev)
    ops.regions_label(voff, foff, faces, ok, 15, thr)
    for sims, q in ((ok, 16), (ok, -1), (torch.ones(74, 17, device=dev), 0), (torch.ones(74, 3, device=dev), 3)):
        with pytest.raises(_lib.ObjnerfError, match="EINVAL"):
            ops.regions_label(voff, foff, faces, sims, q, thr)
    need = ops.regions_workspace_bytes(74, len(m["faces"]), 2)
    assert need > 0
    with pytest.raises(_lib.ObjnerfError, match="EINVAL"):
        ops.regions_label(voff, foff, faces, ok, 0, thr, ws=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    root, label, reg_off, status = ops.regions_label(voff, foff, faces, ok, 0, thr,
                                                     ws=torch.empty(need, dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.ObjnerfError, match="EINVAL"):
        ops.regions_table(voff, foff, t(m["verts"]), faces, ok, 16, root, label, int(reg_off[-1]), status)


# ------------------------------------------------------------------------------------- 5. the naive float path
@pytest.mark.parametrize("case", ["random", "all", "soup"])
def test_table_lies_within_the_bounds_of_the_naive_path(dev, case):
    """Per region with F_r faces: |area - sum area_f| <= F_r 2^-45 + F_r 2^-52 sum area_f (one rounding of at most half a
    unit of 2^-44 per face, an fp64 sum of F_r terms); the centroid: the same bound divided by the area, plus a relative
    2^-50.  From the definition, not tuned."""
    m, sims, thr, got, want = tables_case(dev, case)
    anchors = np.array([m["verts"][o] if o < len(m["verts"]) else np.zeros(3) for o in m["vert_off"][:-1]])
    r = mr.regions_from_table(got["table"], anchors)
    area, cen, nf = U.naive_regions(m, got["label"])
    assert np.array_equal(nf, r["n_faces"])
    worst = [0.0, 0.0]
    for i in np.nonzero(nf > 0)[0]:
        bound = nf[i] * 2.0 ** -45 + nf[i] * 2.0 ** -52 * area[i]
        assert abs(r["area"][i] - area[i]) <= bound, (i, r["area"][i], area[i], bound)
        cb = bound / area[i] + 2.0 ** -50 * np.abs(cen[i])
        assert np.all(np.abs(r["centroid"][i] - cen[i]) <= cb), (i, r["centroid"][i], cen[i], cb)
        worst = [max(worst[0], abs(r["area"][i] - area[i]) / bound), max(worst[1], np.max(np.abs(r["centroid"][i] - cen[i]) / cb))]
    print(f"{case}: {int((nf > 0).sum())} regions, worst error / bound: area {worst[0]:.3g}, centroid {worst[1]:.3g}")


# ------------------------------------------------------------------------------------ 6. MapQuery.part_regions
@pytest.fixture(scope="module")
def planted():
    all_obj, Xs, q, info = U.planted_map()
    return all_obj, PU.dense_of(all_obj, Xs), q, info


def test_part_regions_end_to_end(dev, planted):
    compact, dense, q, info = planted
    p, k = info["position"], info["key"]
    # no vertex of the planted object lies within 1e-3 of either threshold, on the dense cosines, on the CPU
    c = QU.cosine(q, dense[k]["part_feat"]).astype(np.float32)
    thr_frac = mr.thresholds([[c.min(), c.max()]], 0.75)[0]
    assert np.abs(c - 0.5).min() > 1e-3 and np.abs(c - thr_frac).min() > 1e-3
    mq = query.MapQuery(dense, dev)
    assert mq._mesh_dev is None                                      # built by the first call, not by the constructor
    reg = mq.part_regions(q, min_cos=0.5)
    assert mq._mesh_dev is not None and reg.status == 0
    assert len(reg) == 2 and reg.object.tolist() == [p, p] and reg.key.tolist() == [k, k]
    r0 = int(mq.seg_host[p])
    lab = reg.label.cpu().numpy()
    assert reg.label.dtype == torch.int32 and np.array_equal(lab[r0:] >= 0, c >= 0.5) and np.all(lab[:r0] == -1)
    order = [int(np.argmin([np.linalg.norm(reg.centroid[r] - np.array(ce)) for r in range(2)])) for ce in info["centres"]]
    assert sorted(order) == [0, 1]
    for ce, r in zip(info["centres"], order):
        assert np.linalg.norm(reg.centroid[r] - np.array(ce)) <= U.CELL               # within one sheet cell
        ids = reg.vertices(r).cpu().numpy()
        assert reg.peak_vertex[r] in ids and len(ids) == reg.n_vertices[r] and ids.min() == reg.root[r]
        assert reg.peak_cos[r] == pytest.approx(float(c[reg.peak_vertex[r] - r0]), abs=1e-5)
        np.testing.assert_allclose(np.abs(reg.normal[r]), [0, 0, 1], atol=1e-9)       # a flat sheet
        assert reg.extent[r][2] < 1e-6 and np.linalg.det(reg.axes[r]) == pytest.approx(1.0, abs=1e-9)
        assert np.all(reg.box_min[r] <= reg.centroid[r] + 1e-6) and np.all(reg.centroid[r] <= reg.box_max[r] + 1e-6)
    big, small = order[0], order[1]
    assert reg.area[big] > reg.area[small] > 0
    # objects=[p]: the same two regions through the rainbow's own normalisation; another object: none of these
    only = mq.part_regions(q, objects=[p], frac=0.75)
    assert len(only) == 2 and only.object.tolist() == [p, p] and np.isnan(only.thr[0]) and only.thr[p] == pytest.approx(thr_frac, abs=1e-5)
    assert np.array_equal(only.label.cpu().numpy()[r0:] >= 0, c >= thr_frac)
    other = mq.part_regions(q, objects=[1 - p], min_cos=0.5)
    assert len(other) == 0 and int((other.label >= 0).sum()) == 0
    # min_area drops the smaller blob; the label image is remapped to the rows that stay
    cut = mq.part_regions(q, min_cos=0.5, min_area=0.5 * (reg.area[big] + reg.area[small]))
    assert len(cut) == 1 and cut.root.tolist() == [reg.root[big]] and cut.area[0] == reg.area[big]
    lc = cut.label.cpu().numpy()
    assert np.array_equal(lc == 0, lab == big) and np.array_equal(lc == -1, lab != big)
    assert len(mq.part_regions(q, min_cos=0.5, min_vertices=10 ** 6)) == 0
    # the compact form of the same map gives the same labels
    mc = query.MapQuery(compact, dev)
    assert mc.compact is not None
    for kw in ({"min_cos": 0.5}, {"objects": [p], "frac": 0.75}):
        a, b = mq.part_regions(q, **kw), mc.part_regions(q, **kw)
        assert torch.equal(a.label, b.label) and np.array_equal(a.root, b.root)
        assert np.array_equal(a.area, b.area) and np.array_equal(a.centroid, b.centroid)
    with pytest.raises(ValueError):
        mq.part_regions(q, frac=1.5)
    with pytest.raises(ValueError):
        mq.part_regions(q, objects=[2])


# --------------------------------------------------------------------------------------------------------- 7. CLI
def test_cli_regions(dev, planted, tmp_path):
    from openobj_amd import map_query
    compact, dense, q, info = planted
    log = tmp_path / "log"
    os.makedirs(log)
    with gzip.open(log / map_query.DENSE_FILE, "wb") as fh:
        pickle.dump(dense, fh)
    np.save(tmp_path / "c.npy", info["clip_query"])
    np.save(tmp_path / "s.npy", info["sbert_query"])
    np.save(tmp_path / "p.npy", q.astype(np.float32))
    base = ["--logdir", str(log), "--mode", "part", "--clip-query", str(tmp_path / "c.npy"), "--sbert-query",
            str(tmp_path / "s.npy"), "--part-query", str(tmp_path / "p.npy"), "--device", str(dev)]
    doc_a = map_query.main(base + ["--out", str(tmp_path / "a"), "--regions", "--region-min-cos", "0.5"])
    doc_b = map_query.main(base + ["--out", str(tmp_path / "b")])
    k = info["key"]
    assert doc_a == doc_b and doc_a["top"] == [k]
    fa, fb = set(os.listdir(tmp_path / "a")), set(os.listdir(tmp_path / "b"))
    assert fa - fb == {"regions.json", f"obj_{k}_regions.ply"} and fb <= fa and fb == {"query.json", "obj_10.ply", f"obj_{k}.ply"}
    for f in fb:                                                     # without the flag every file keeps its bytes
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    with open(tmp_path / "a" / "regions.json") as fh:
        doc = json.load(fh)
    assert doc["status"] == 0 and len(doc["regions"]) == 2 and doc["thr"] == {str(k): 0.5}
    reg = query.MapQuery(dense, dev).part_regions(q, objects=[info["position"]], min_cos=0.5)
    for rec, r in zip(doc["regions"], range(2)):
        assert set(rec) == set(mr.FIELDS) and rec["key"] == k and rec["object"] == info["position"]
        assert rec["root"] == reg.root[r] and rec["n_vertices"] == reg.n_vertices[r] and rec["area"] == reg.area[r]
        assert rec["centroid"] == reg.centroid[r].tolist() and rec["axes"] == reg.axes[r].tolist()
        assert rec["peak_vertex"] == reg.peak_vertex[r]
    from openobj_amd.mesh import read_ply
    ply = read_ply(str(tmp_path / "a" / f"obj_{k}_regions.ply"))
    assert ply is not None
