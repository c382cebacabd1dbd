"""CPU: the map-query restatement (tests/query_util.py) against matplotlib / sklearn, the host bookkeeping of
openobj_amd.query against it, the exported "rainbow" table and the CLI's refusals (vis_interaction.py)."""
import gzip
import os
import pickle

import numpy as np
import pytest

from openobj_amd import _lib, ops, query
try:
    from tests import query_util as QU
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import query_util as QU


def _lib_built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def test_rainbow_restatement_and_exported_lut_match_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps["rainbow"]
    cmap(0.5)                                                  # _init: builds _lut
    ref = cmap._lut[:256, :3]
    assert np.array_equal(QU.rainbow_lut(), ref)
    _lib_built()
    got = ops.rainbow_lut()
    assert got.dtype == np.float32 and got.tobytes() == ref.astype(np.float32).tobytes()


def test_rainbow_indexing_matches_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps["rainbow"]
    rs = np.random.RandomState(0)
    edge = [0.0, -0.0, 1.0, -1e-9, -0.3, 1.0000001, 7.0, np.nan, np.inf, -np.inf, 255 / 256, np.nextafter(1, 0),
            np.nextafter(255 / 256, 0), 1 / 256, np.nextafter(1 / 256, 0)]
    x = np.concatenate([rs.rand(5000), (np.arange(256) + 0.5) / 256, edge]).astype(np.float32)
    assert np.array_equal(QU.rainbow(x), cmap(x)[..., :3])


def test_pca_restatement_matches_sklearn():
    pytest.importorskip("sklearn")
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    rs = np.random.RandomState(1)
    X = rs.randn(400, 40) @ np.diag(np.linspace(3, 0.1, 40)) + 5.0
    X[:, 7] = 2.0                                              # a constant column: std 0 -> 1 in both
    want = QU.sign_rule(PCA(n_components=3, svd_solver="full").fit_transform(StandardScaler().fit_transform(X)))
    got = QU.pca_scores(X)
    np.testing.assert_allclose(got, want, atol=1e-8, rtol=0)
    np.testing.assert_allclose(QU.pca_colors(got), QU.pca_colors(want), atol=1e-8, rtol=0)


def test_pca_weights_from_moments_equal_the_restatement():
    """query.pca_weights (the host step between the two device passes) on fp64 moments gives the restated scores."""
    rs = np.random.RandomState(2)
    X = rs.randn(300, 24) @ np.diag(np.linspace(4, 0.2, 24)) + rs.randn(24)
    m = X.mean(axis=0)
    C = (X - m).T @ (X - m)
    W, b = query.pca_weights(m[None], C[None], [len(X)])
    np.testing.assert_allclose(QU.sign_rule(X @ W[0] + b[0]), QU.pca_scores(X), atol=1e-9, rtol=0)


def test_bookkeeping_matches_the_restatement():
    pytest.importorskip("sklearn")
    import torch
    all_obj = QU.synthetic_map(3, D=16, Dc=12, Ds=8)
    ranked, clip, cap = query.reduce_object_features(all_obj)
    assert ranked == [0, 1, 3, 4]                              # position 2 carries no feature: out of the ranking
    from openobj_amd.mapping import get_majority_cluster_mean
    for i, p in enumerate(ranked):
        o = all_obj[list(all_obj)[p]]
        np.testing.assert_allclose(clip[i], get_majority_cluster_mean(o["clip_feat"], 0.2, 2), rtol=1e-6)
        np.testing.assert_allclose(clip[i], o["clip_feat"][:4].mean(axis=0), rtol=1e-5)   # the outlier view is dropped
    rs = np.random.RandomState(4)
    cq, sq = rs.randn(12), rs.randn(8)
    sim = QU.object_similarity(cq, sq, clip, cap)
    for k in (1, 2, 3, 9):
        assert query.top_positions(torch.from_numpy(sim), ranked, k) == [ranked[i] for i in QU.top_indices(sim, k)]
    assert query.top_positions(torch.from_numpy(sim), ranked, 0) == []
    colors = [o["color"] for o in all_obj.values()]
    want = QU.object_query_colors(sim, ranked, colors, 2)
    top = set(query.top_positions(torch.from_numpy(sim), ranked, 2))
    assert 2 not in top and np.array_equal(want[2], QU.rgb_colors(colors[2], 0.5))
    for p in range(len(colors)):
        assert (p in top) == np.array_equal(want[p], np.tile([1.0, 0, 0], (len(colors[p]), 1)))
    # class, instance colours and hidden sets
    mapping = {i: (i * 7) % 11 for i in range(100)}
    mapped = {i: [i / 11, 1 - i / 11, 0.5] for i in range(11)}
    np.testing.assert_array_equal(query.class_colors(all_obj, mapping, mapped), np.stack(QU.class_colors(all_obj, mapping, mapped)))
    np.testing.assert_array_equal(query.instance_palette(7), QU.instance_palette(7))
    pal = query.instance_palette(51)
    assert len({tuple(np.round(c, 6)) for c in pal}) == 51 and pal.min() >= 1 / 3 - 1e-12 and pal.max() <= 1
    for ds, sc in (("Replica", "room_0"), ("Replica", "room_2"), ("Replica", "office_0"), ("Scannet", "scene0000_00"),
                   ("Scannet", "611")):
        h = query.hidden_sets(all_obj, ds, sc)
        c, m, b = QU.hidden_sets(all_obj, ds, sc)
        assert h["ceiling"] == c and h["most"] == m
        assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(h["boxes"], b))
        assert h["hidden"] == (c if ds == "Replica" else [])
    assert query.hidden_sets(all_obj, "Replica", "room_0")["ceiling"] == [1, 3]


def test_color_yaml_is_read_as_the_reference_writes_it(tmp_path):
    pytest.importorskip("yaml")
    p = tmp_path / "colors.yaml"
    p.write_text("mapping:\n  0: 0   # unknown\n  1: 2\nmapped_colors:\n  0:\n  - 0\n  - 0\n  - 0\n  2:\n  - 0.25\n  - 0.5\n"
                 "  - 1.0\n")
    mapping, mapped = query.load_color_yaml(str(p))
    assert mapping == {0: 0, 1: 2} and mapped[2] == [0.25, 0.5, 1.0]
    assert np.array_equal(query.class_colors({5: {"class_id": 0}}, mapping, mapped), [[0.25, 0.5, 1.0]])


def _write_map(tmp_path):
    all_obj = QU.synthetic_map(5, sizes=(30, 12), D=40, Dc=12, Ds=8, missing=(), z0=(0.0, 0.0), classes=(1, 2))
    log = tmp_path / "log"
    log.mkdir()
    with gzip.open(str(log / "map_vis.pkl.gz"), "wb") as fh:
        pickle.dump(all_obj, fh)
    return log


def test_cli_refuses_bad_input_before_the_device(tmp_path, monkeypatch):
    import torch
    from openobj_amd import map_query
    log = _write_map(tmp_path)
    np.save(str(tmp_path / "clip.npy"), np.ones(12, np.float32))
    np.save(str(tmp_path / "sbert.npy"), np.ones(8, np.float32))
    np.save(str(tmp_path / "part_bad.npy"), np.ones(41, np.float32))
    np.save(str(tmp_path / "sbert_bad.npy"), np.ones(384, np.float32))

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(query, "MapQuery", no_device)
    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    base = ["--logdir", str(log), "--out", str(tmp_path / "out")]
    bad = [["--mode", "nope"],
           ["--mode", "object", "--clip-query", str(tmp_path / "missing.npy"), "--sbert-query", str(tmp_path / "sbert.npy")],
           ["--mode", "object", "--clip-query", str(tmp_path / "clip.npy")],
           ["--mode", "object", "--clip-query", str(tmp_path / "clip.npy"), "--sbert-query", str(tmp_path / "sbert_bad.npy")],
           ["--mode", "part", "--clip-query", str(tmp_path / "clip.npy"), "--sbert-query", str(tmp_path / "sbert.npy"),
            "--part-query", str(tmp_path / "part_bad.npy")],
           ["--mode", "class"],
           ["--mode", "rgb", "--logdir", str(tmp_path / "nolog")]]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            map_query.main(base + extra)
        assert e.value.code == 2, extra
    assert not os.path.exists(tmp_path / "out")
