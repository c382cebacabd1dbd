"""CPU: the host side of openobj_amd.mask_graph and the restatement the GPU tests compare against
(tests/maskgraph_util.py): the restated DBSCAN against scikit-learn, the merge mapping, the rare-id filter, the mode
tie rule, the refusals and the writer / dataset round trip."""
import os

import numpy as np
import pytest

from openobj_amd import dataset as ods
from openobj_amd import mask_graph as MG
try:
    from tests import maskgraph_util as U
    from tests import scene_files as SF
    from tests.test_dataset import make_cfg
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import maskgraph_util as U
    import scene_files as SF
    from test_dataset import make_cfg


def _border_between_two_clusters():
    """Two tight groups of 8 points 0.08 apart and one point midway: within eps = 0.05 of the two nearest points of
    each group, so core of neither at min_points 8 (it sees 2 + 2 points and itself) and a border point of both."""
    far = [[-0.02, 0.0, 0.0], [-0.02, 0.01, 0.0], [-0.02, 0.0, 0.01], [-0.02, 0.01, 0.01], [-0.03, 0.0, 0.0], [-0.03, 0.01, 0.0]]
    a = np.array([[0.0, 0.0, 0.0], [0.0, 0.01, 0.0]] + far)
    b = a * [-1.0, 1.0, 1.0] + [0.08, 0.0, 0.0]
    mid = np.array([[0.04, 0.002, 0.002]])
    return np.concatenate([b, mid, a])          # the cluster numbered 0 is b: the border point must take 0


@pytest.mark.parametrize("case", ["tiny", "border", "noise", "single", "blobs300", "blobs3000"])
def test_restated_dbscan_equals_sklearn(case):
    cluster = pytest.importorskip("sklearn.cluster")
    rs = np.random.RandomState(5)
    eps, mp = 0.05, 6
    if case == "tiny":
        x, mp = rs.rand(5, 3) * 0.05, 3
    elif case == "border":
        x, mp = _border_between_two_clusters(), 8
    elif case == "noise":
        x = rs.rand(200, 3) * 5.0
    elif case == "single":
        x = rs.randn(150, 3) * 0.01
    elif case == "blobs300":
        x = np.concatenate([rs.randn(120, 3) * 0.03, rs.randn(120, 3) * 0.03 + [0.3, 0, 0], rs.rand(60, 3)])
        x = x[rs.permutation(len(x))]
    else:
        x = np.concatenate([rs.randn(900, 3) * 0.06 + c for c in ([0, 0, 0], [0.35, 0, 0], [0, 0.5, 0])] + [rs.rand(300, 3)])
        x, mp = x[rs.permutation(len(x))], 20
    want = cluster.DBSCAN(eps=eps, min_samples=mp).fit_predict(x)
    got = U.dbscan_labels(x, eps, mp)
    assert np.array_equal(got, want)
    if case == "border":
        assert want[8] == 0 and want.max() == 1 and (want[:8] == 0).all() and (want[9:] == 1).all()
    if case == "noise":
        assert (want == -1).all()
    if case == "single":
        assert (want == 0).all()
    if case.startswith("blobs"):
        assert want.max() >= 1 and (want == -1).any()


def test_vector_dbscan_and_majority_mean_equal_sklearn():
    """The majority mean's DBSCAN over 384-d unit vectors (eps 0.2, min_samples 2): the module's host version and the
    restatement both equal scikit-learn's labels."""
    cluster = pytest.importorskip("sklearn.cluster")
    rs = np.random.RandomState(2)
    base = rs.randn(3, 384)
    x = np.concatenate([base[0] + 0.004 * rs.randn(9, 384), base[1] + 0.004 * rs.randn(5, 384), base[2][None],
                        rs.randn(3, 384)])
    x = (x / np.linalg.norm(x, axis=1, keepdims=True))[rs.permutation(len(x))]
    want = cluster.DBSCAN(eps=0.2, min_samples=2).fit_predict(x)
    assert want.max() == 1 and (want == -1).sum() == 4
    assert np.array_equal(MG.vector_dbscan(x, 0.2, 2), want)
    assert np.array_equal(U.dbscan_labels(x, 0.2, 2), want)
    u, c = np.unique(want, return_counts=True)
    mean = x[want == u[np.argmax(c)]].mean(axis=0)
    assert np.array_equal(MG.majority_mean(x), mean)
    assert np.allclose(U.majority_mean(x), mean, rtol=0, atol=1e-15)
    # every vector on its own: noise is the majority (np.unique lists -1 first), the mean is over all of them
    y = np.eye(384)[:4]
    assert np.array_equal(MG.majority_mean(y), y.mean(axis=0))


def test_largest_cluster_tie_goes_to_the_label_met_first():
    assert MG.largest_cluster(np.array([-1, -1])) is None
    assert MG.largest_cluster(np.array([-1, 1, 0, 0, 1, -1])).tolist() == [False, True, False, False, True, False]
    assert MG.largest_cluster(np.array([0, 1, 1, 1, 0])).tolist() == [False, True, True, True, False]
    for lab in ([-1, 1, 0, 0, 1, -1], [2, 2, 0, 0, 1, 1, -1], [0]):
        assert np.array_equal(MG.largest_cluster(np.array(lab)), U.largest_cluster_mask(lab))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def test_merge_mapping_wall_and_chain():
    """Six clusters: 10 is a wall; 11-12 and 12-13 overlap (a chain a-b, b-c: c joins b's id, which is a's); 14 overlaps
    13 in points but not in caption; 15 stands alone.  The reference's `continue` order: the wall row maps itself and
    ends its pairs; as the LAST key a wall would only be seen as j."""
    wall, floor, ceiling = _unit([1, 0, 0, 0, 0, 0])[None], _unit([0, 1, 0, 0, 0, 0])[None], _unit([0, 0, 1, 0, 0, 0])[None]
    obj, other = _unit([0, 0, 0, 1, 0.1, 0]), _unit([0, 0, 0, 0, 0, 1])
    keys = [10, 11, 12, 13, 14, 15]
    cap = [_unit([1, 0.05, 0, 0, 0, 0]), obj, obj, obj, other, other]
    col = [_unit([1, 1, 1])] * 6
    sim = np.zeros((6, 6))
    for a, b, v in ((1, 2, 0.8), (2, 3, 0.8), (3, 4, 0.8), (0, 1, 0.95)):
        sim[a, b] = sim[b, a] = v
    got, counter = MG.merge_mapping(keys, sim, cap, col, wall, floor, ceiling, 0.8, 0.7, 0.7, 0.7)
    want, wcounter = U.merge_mapping(keys, sim, cap, col, wall, floor, ceiling, 0.8, 0.7, 0.7, 0.7)
    assert got == want and counter == wcounter
    assert got == {10: 1, 11: 4, 12: 4, 13: 4, 14: 5, 15: 6, 999: 0} and counter == 7
    # a floor cluster in the last place is met only as j, by the first row that is no background
    keys2, cap2 = keys[1:] + [16], cap[1:] + [_unit([0, 1, 0, 0.02, 0, 0])]
    sim2 = np.zeros((6, 6))
    sim2[0, 1] = sim2[1, 0] = 0.95
    got2, _ = MG.merge_mapping(keys2, sim2, cap2, col, wall, floor, ceiling, 0.8, 0.7, 0.7, 0.7)
    assert got2 == U.merge_mapping(keys2, sim2, cap2, col, wall, floor, ceiling, 0.8, 0.7, 0.7, 0.7)[0]
    assert got2[16] == 2 and got2[11] == got2[12] == 4


def test_rare_ids_become_999():
    ids = [3, 3, 3, 5, 5, 7, 3, 9, 9, 9]
    assert MG.filter_rare(ids, 100) == [3, 3, 3, 999, 999, 999, 3, 9, 9, 9]          # limit int(100 / 50) = 2
    assert MG.filter_rare(ids, 49) == ids                                             # limit 0
    assert MG.filter_rare(ids, 150) == [3, 3, 3, 999, 999, 999, 3, 999, 999, 999]     # limit 3
    assert MG.filter_rare(ids, 100) == U.filter_rare(ids, 2)


def test_mode_tie_goes_to_the_first_value_in_raster_order():
    assert MG.mode_first(np.array([[7, 2], [2, 7]])) == 7
    assert MG.mode_first(np.array([[2, 7], [7, 2]])) == 2
    assert MG.mode_first(np.array([5, 1, 1, 5, 1])) == 1
    rs = np.random.RandomState(0)
    for _ in range(20):
        v = rs.randint(0, 4, (5, 6))
        assert MG.mode_first(v) == U.mode_first(v)


def test_refusals(tmp_path):
    with pytest.raises(NotImplementedError):
        MG.MaskGraph({"graph_method": "threshold"}, (1.0, 1.0, 0.0, 0.0), device="cpu")
    import yaml
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"graph_method": "threshold", "fx": 1.0, "fy": 1.0, "cx": 0.0, "cy": 0.0}))
    with pytest.raises(NotImplementedError):
        MG.main([str(cfg), "--input-mask", "none.pkl", "--dataset-dir", str(tmp_path), "--bg-feats", "none.npz",
                 "--output-dir", str(tmp_path / "out")])
    depth = np.full((30, 40), 1000, np.uint16)
    bgr = np.zeros((30, 40, 3), np.uint8)
    with pytest.raises(NotImplementedError):            # a mask of another size (the reference resizes it)
        MG.project_masks([np.ones((15, 20), bool)], depth, bgr, np.eye(4), 1000.0, (30.0, 30.0, 20.0, 15.0), "cpu")
    with pytest.raises(NotImplementedError):            # an image of another size
        MG.project_masks([np.ones((30, 40), bool)], depth, np.zeros((60, 80, 3), np.uint8), np.eye(4), 1000.0,
                         (30.0, 30.0, 20.0, 15.0), "cpu")
    with pytest.raises(ValueError):                     # 35 rows: not a multiple of 10
        MG.mask_boxes_2d(np.zeros((1, 35, 40), np.uint16), np.eye(4)[None], np.zeros((1, 6)), (30.0, 30.0, 20.0, 15.0), "cpu")


def test_written_ids_are_read_back_by_the_dataset(tmp_path):
    """write_outputs -> dataset.Replica: the id images come back as the ids that were written."""
    SF.write_scene(str(tmp_path), "Replica", n_frames=20)
    images = []
    for i in range(2):
        _, _, inst = SF._frame(i, None)
        img = inst.astype(np.int32)
        img[img == 7] = 300                                # an id past 8 bits
        images.append(img)
    f = lambda k, n: np.eye(n, dtype=np.float32)[k % n]
    clip = [{k: f(k, 16)[None] for k in (1, 4, 300, 5)} for _ in range(2)]
    cap = [{k: f(k + 1, 12) for k in (1, 4, 300, 5)} for _ in range(2)]
    text = [{k: "object %d" % k for k in (1, 4, 300, 5)} for _ in range(2)]
    MG.write_outputs(str(tmp_path), images, clip, cap, text)
    assert not os.path.exists(os.path.join(str(tmp_path), "debug"))
    ds = ods.Replica(make_cfg(tmp_path, "Replica"))
    for i in range(2):
        s = ds[i]
        obj = np.asarray(s["obj"]).T
        assert set(np.unique(obj)) == {-1, 0, 4, 300}
        assert np.array_equal(obj == 300, images[i] == 300) and np.array_equal(obj == 4, images[i] == 4)
        assert np.array_equal(obj == 0, images[i] == 1)
        assert sorted(s["obj_clip"]) == [0, 4, 300] and np.array_equal(s["obj_cap"][300], cap[i][300])
    MG.write_outputs(str(tmp_path), images, clip, cap, text, debug_images=True)
    assert os.path.exists(os.path.join(str(tmp_path), "debug", "inst_1.png"))
