"""CPU: the host side of the part regions (openobj_amd/map_regions.py) -- everything derived from the
integer table, the threshold arithmetic, the filter, the CLI's argument checks -- and the specification against itself."""
import os

import numpy as np
import pytest

import mapregions_util as U
from openobj_amd import map_regions as mr


def _spec_table(objects, sims=None, thr=None, **kw):
    m = U.pack(objects, **kw)
    V = len(m["verts"])
    sims = np.ones(V, np.float32) if sims is None else np.asarray(sims, np.float32)
    thr = np.zeros(len(objects), np.float32) if thr is None else thr
    root, _ = U.components(m, U.selected(sims, thr, m["vert_off"]))
    reg_off, label = U.rows(root, m["vert_off"])
    t, status = U.table(m, sims, root, label)
    anchors = np.array([m["verts"][o] if o < V else np.zeros(3) for o in m["vert_off"][:-1]])
    return m, t, anchors, label, status


def test_columns_agree_with_the_specification_and_the_wrappers():
    from openobj_amd import ops
    names = ("ROW", "C_ROOT", "C_OBJ", "C_NV", "C_NF", "C_AREA", "C_M1", "C_NRM", "C_MIN", "C_MAX", "C_PEAK", "C_CEN", "C_M2", "C_RES")
    assert [getattr(mr, n) for n in names] == [getattr(U, n) for n in names]
    assert ops.REGION_ROW == mr.ROW == 32 and mr.DEFAULT_FRAC == 0.75


def test_flat_unit_square():
    """Area 1, normal +-z, the smallest extent 0, a right-handed frame, the centroid and the box -- at an offset, so the
    anchor is exercised."""
    off = np.array([3.0, -2.0, 0.5])
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float64) + off
    m, t, anchors, _, status = _spec_table([(v, [(0, 1, 3), (0, 3, 2)])])
    assert status == 0 and t.shape == (1, mr.ROW)
    r = mr.regions_from_table(t, anchors, keys=[17])
    assert r["key"].tolist() == [17] and r["object"].tolist() == [0] and r["root"].tolist() == [0]
    assert r["n_vertices"].tolist() == [4] and r["n_faces"].tolist() == [2]
    assert r["area"][0] == 1.0
    np.testing.assert_allclose(r["centroid"][0], off + [0.5, 0.5, 0.0], atol=1e-12)
    assert np.array_equal(np.abs(r["normal"][0]), [0.0, 0.0, 1.0])
    np.testing.assert_allclose(r["extent"][0], [np.sqrt(1 / 12), np.sqrt(1 / 12), 0.0], atol=1e-7)
    assert r["extent"][0][2] == 0.0
    A = r["axes"][0]
    np.testing.assert_allclose(A @ A.T, np.eye(3), atol=1e-12)
    assert np.linalg.det(A) == pytest.approx(1.0, abs=1e-12)
    np.testing.assert_allclose(np.abs(A[2]), [0, 0, 1], atol=1e-12)
    assert np.array_equal(r["box_min"][0], off.astype(np.float32).astype(np.float64))
    assert np.array_equal(r["box_max"][0], (off + [1, 1, 0]).astype(np.float32).astype(np.float64))


def test_sign_rule_of_the_frame():
    """The largest-magnitude component of an axis is positive; the third axis gives way to right-handedness."""
    rs = np.random.RandomState(0)
    for _ in range(20):
        B = rs.randn(3, 3)
        axes, ext = mr.frame_from_covariance(B @ np.diag([3.0, 2.0, 1.0]) @ B.T)
        assert ext[0] >= ext[1] >= ext[2] >= 0
        assert np.linalg.det(axes) == pytest.approx(1.0, abs=1e-9)
        for a in axes[:2]:
            assert a[np.argmax(np.abs(a))] > 0


def test_zero_area_regions_are_finite():
    """A single selected vertex and a face with a repeated vertex: zero area, a zero normal, finite outputs, the centroid
    at the centre of the box."""
    v = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [2, 2, 2]], np.float64)
    sims = np.array([1, 0, 1, 1], np.float32)
    m, t, anchors, label, status = _spec_table([(v, [(2, 3, 3)])], sims=sims, thr=np.array([0.5], np.float32))
    assert status == 0 and label.tolist() == [0, -1, 1, 1]
    r = mr.regions_from_table(t, anchors)
    assert r["n_vertices"].tolist() == [1, 2] and r["n_faces"].tolist() == [0, 1]
    for f in mr.FIELDS:
        assert np.all(np.isfinite(np.asarray(r[f], np.float64))), f
    assert np.array_equal(r["area"], [0.0, 0.0]) and np.array_equal(r["normal"], np.zeros((2, 3)))
    assert np.array_equal(r["extent"], np.zeros((2, 3)))
    assert np.array_equal(r["centroid"], [[1, 2, 3], [4.5, 5, 5.5]])
    assert r["peak_vertex"].tolist() == [0, 2] and r["peak_cos"].tolist() == [1.0, 1.0]
    assert mr.regions_from_table(np.zeros((0, mr.ROW), np.int64), np.zeros((1, 3)))["area"].shape == (0,)


def test_threshold_arithmetic_is_fp32():
    rs = np.random.RandomState(1)
    mn = rs.uniform(-0.3, 0.2, 50).astype(np.float32)
    mx = (mn + rs.uniform(0.01, 0.9, 50)).astype(np.float32)
    mm = np.stack([mn, mx], axis=1)
    for frac in (0.0, 0.3, 0.75, 1.0):
        want = np.array([np.float32(a + np.float32(np.float32(frac) * np.float32(b - a))) for a, b in zip(mn, mx)], np.float32)
        got = mr.thresholds(mm, frac)
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(mr.thresholds(mm, 0.0), mn)
    got = mr.thresholds(mm, 0.75, min_cos=0.31)
    assert np.array_equal(got, np.full(50, np.float32(0.31)))
    got = mr.thresholds(mm, 0.5, objects=[3, 7])
    assert np.isnan(got[[i for i in range(50) if i not in (3, 7)]]).all() and np.array_equal(got[[3, 7]], mr.thresholds(mm, 0.5)[[3, 7]])
    # an empty object's (inf, -inf) and a left-out object's NaN give NaN: nothing is selected
    odd = mr.thresholds(np.array([[np.inf, -np.inf], [np.nan, np.nan]], np.float32), 0.75)
    assert np.isnan(odd).all()
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            mr.thresholds(mm, bad)


def test_filter_and_remap():
    area = np.array([0.5, 0.01, 0.2, 0.0, 0.3])
    nv = np.array([10, 3, 1, 1, 7])
    keep, remap = mr.filter_rows(area, nv)
    assert keep.tolist() == [0, 1, 2, 3, 4] and remap.tolist() == [0, 1, 2, 3, 4, -1]
    keep, remap = mr.filter_rows(area, nv, min_area=0.1)
    assert keep.tolist() == [0, 2, 4] and remap.tolist() == [0, -1, 1, -1, 2, -1]
    keep, remap = mr.filter_rows(area, nv, min_area=0.1, min_vertices=2)
    assert keep.tolist() == [0, 4] and remap.tolist() == [0, -1, -1, -1, 1, -1]
    label = np.array([-1, 0, 4, 2, 1, -1, 4])
    assert remap[label].tolist() == [-1, 0, 1, -1, -1, -1, 1]          # (-1 indexes the last entry)
    assert remap.dtype == np.int32


def test_region_colors():
    rgb = np.array([[255, 0, 0, 255], [0, 255, 0, 255], [10, 20, 30, 255]], np.uint8)
    col = mr.region_colors(np.array([1, -1, 0]), rgb, 2, 0.5)
    from openobj_amd.query import instance_palette
    pal = np.round(instance_palette(2) * 255).astype(np.uint8)
    assert col.dtype == np.uint8 and col[0].tolist() == pal[1].tolist() and col[2].tolist() == pal[0].tolist()
    assert col[1].tolist() == [0, 128, 0]


@pytest.mark.parametrize("extra,msg", [
    (["--mode", "rgb", "--regions"], "--regions needs --mode part"),
    (["--mode", "part", "--regions", "--region-frac", "0.5", "--region-min-cos", "0.3"], "exclude each other"),
    (["--mode", "part", "--regions", "--region-frac", "1.5"], "outside [0, 1]"),
    (["--mode", "part", "--regions", "--region-frac", "-0.1"], "outside [0, 1]"),
    (["--mode", "part", "--region-frac", "0.5"], "needs --regions"),
    (["--mode", "part", "--regions", "--region-min-area", "-1"], "negative"),
])
def test_cli_argument_errors_come_before_the_device(tmp_path, monkeypatch, capsys, extra, msg):
    from openobj_amd import map_query, query

    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(query.MapQuery, "__init__", boom)
    with pytest.raises(SystemExit) as e:
        map_query.main(["--logdir", str(tmp_path), "--out", str(tmp_path / "o")] + extra)
    assert e.value.code == 2
    assert msg in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "o")


def test_workspace_bytes_is_zero_out_of_range():
    from openobj_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert ops.regions_workspace_bytes(1000, 2000, 5) > 0
    assert ops.regions_workspace_bytes(1, 0, 1) > 0
    assert ops.regions_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1, 65535) > 0
    for V, F, S in ((0, 10, 1), (-1, 10, 1), (2 ** 31, 10, 1), (10, -1, 1), (10, 2 ** 31, 1), (10, 10, 0), (10, 10, 65536),
                    (2 ** 40, 10, 1)):
        assert ops.regions_workspace_bytes(V, F, S) == 0, (V, F, S)


def _five_objects(rs):
    def sheet_obj(w, h):
        x, y = U.sheet_xy(w, h)
        return np.stack([x * 0.1, y * 0.1, 0.05 * rs.randn(w * h)], axis=1), U.sheet(w, h)
    return [sheet_obj(16, 12), (np.zeros((0, 3)), np.zeros((0, 3), np.int64)), (rs.rand(1, 3), np.zeros((0, 3), np.int64)),
            (rs.rand(5, 3), [(0, 1, 2), (2, 3, 4)]), sheet_obj(9, 5)]


def test_specification_agrees_with_itself_under_a_permutation():
    """The same regions as sets of (original) vertices whatever the vertex order and the face order; the roots are the
    minima; the areas agree to rounding."""
    rs = np.random.RandomState(5)
    objs = _five_objects(rs)
    sel0 = [rs.rand(len(v)) < 0.6 for v, _ in objs]
    outs = []
    for kw in ({}, {"permute_seed": 3}, {"permute_seed": 4, "shuffle_seed": 9}):
        m = U.pack(objs, **kw)
        sel = U.per_vertex(m, sel0)
        root, status = U.components(m, sel)
        assert status == 0
        for reg in U.region_sets(root):
            assert {int(root[v]) for v in reg} == {min(reg)}
        # back to original ids: inverse of the permutation, object by object
        inv = np.concatenate([np.argsort(p) + o for p, o in zip(m["perm"], m["vert_off"][:-1])])
        sets = {frozenset(int(inv[v]) for v in reg) for reg in U.region_sets(root)}
        reg_off, label = U.rows(root, m["vert_off"])
        t, _ = U.table(m, sel.astype(np.float32), root, label)
        assert reg_off[-1] == len(sets) == len(t) and np.all(np.diff(t[:, U.C_ROOT]) > 0)
        assert int(t[:, U.C_NV].sum()) == int(sel.sum())
        by_set = {frozenset(int(inv[v]) for v in np.nonzero(label == r)[0]): t[r, U.C_AREA] for r in range(len(t))}
        outs.append((sets, by_set))
    assert outs[0][0] == outs[1][0] == outs[2][0] and len(outs[0][0]) > 5
    for k, a in outs[0][1].items():
        for o in outs[1:]:
            assert abs(int(o[1][k]) - int(a)) <= 64            # (a few units of 2^-44 m^2: the anchor moved)
