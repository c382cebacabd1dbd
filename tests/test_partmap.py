"""Compact part-level feature maps (openobj_amd/part_maps.py), host side: the mask-loop semantics and crop boxes against
the reference's own run (fixture G17), the file format, the dataset loader and the PartStore bookkeeping.  No GPU."""
import numpy as np
import pytest
import torch

from openobj_amd import cfg as ocfg
from openobj_amd import dataset as ods
from openobj_amd import part_maps as pm
try:
    from tests import partmap_util as PU
    from tests import scene_files as SF
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import partmap_util as PU
    import scene_files as SF

DOWN = 4                     # the helper scene is 64 x 48: 16 x 12 part maps


def make_cfg(root, fmt, **kw):
    over = {"dataset.path": str(root), "dataset.format": fmt, "trainer.part_mode": 1, "trainer.part_down": DOWN,
            "camera.w": SF.W, "camera.h": SF.H, "camera.fx": SF.FX, "camera.fy": SF.FY, "camera.cx": SF.CX,
            "camera.cy": SF.CY}
    over.update(kw)
    return ocfg.Config(ocfg.replica_room0_config(train_device="cpu", **over))


def g17_strided(g):
    d = int(g["down_sample"])
    return g["segmentation"][:, ::d, ::d]


@pytest.mark.parametrize("tag", ["fp32", "fp16"])
def test_restatement_and_package_match_g17(golden, tag):
    """The saved array of the reference's main() against the numpy restatement and against the package's host path
    (feature_table -> compact -> densify_host), bit for bit, for fp32 and fp16 features."""
    g = golden("g17_partmap")
    feat, score, want = g["feat_" + tag], g["stability_score"], g["dense_" + tag]
    assert feat.dtype == (np.float32 if tag == "fp32" else np.float16) and want.dtype == np.float32
    masks = g17_strided(g)
    assert np.array_equal(PU.reference_loop(masks, feat, score), want)
    table = pm.feature_table(feat, score).numpy()
    assert table.dtype == np.float32
    assert np.array_equal(table, np.stack([PU.scaled_row(feat[i], score[i]) for i in range(len(score))]))
    index, tab = pm.compact(PU.last_mask(masks), table)
    assert np.array_equal(pm.densify_host(index, tab), want)
    i2, t2 = PU.compact_of(masks, feat, score)
    assert np.array_equal(index, i2) and np.array_equal(tab, t2)
    assert np.array_equal(pm.strided_masks({"segmentation": g["segmentation"]}, 5), masks.astype(np.uint8))


def test_crop_boxes_match_g17(golden):
    """bbox_getter: the crops CLIP's preprocess was given in the reference run have crop_box's shapes; the two widths
    whose 1.3-fold ends in .5 round to even (15 -> 20, 5 -> 6) and the growth is clipped at the border."""
    g = golden("g17_partmap")
    H, W = g["segmentation"].shape[1:]
    boxes = [pm.crop_box([int(v) for v in b], H, W) for b in g["bbox"]]
    assert [(b[3] - b[1], b[2] - b[0]) for b in boxes] == [tuple(s) for s in g["crop_shapes"].tolist()]
    assert boxes[0] == [0, 0, 23, 23]                  # at the corner: grows right and down only
    assert boxes[2] == [8, 7, 27, 33]                  # 15 -> 20 (19.5 to even), increment round(2.5) = 2
    assert boxes[3] == [30, 5, 35, 10]                 # 5 -> 6 (6.5 to even), increment round(0.5) = 0
    assert boxes[5] == [43, 23, 60, 40]                # right / bottom border
    assert all(0 <= b[0] <= b[2] <= W and 0 <= b[1] <= b[3] <= H for b in boxes)


def test_unused_rows_are_dropped_and_renumbered(golden):
    g = golden("g17_partmap")
    masks, feat, score = g17_strided(g), g["feat_fp32"], g["stability_score"]
    last = PU.last_mask(masks)
    used = sorted(set(last[last >= 0].tolist()))
    assert used == [0, 2, 5, 6]        # 1 is covered by 2, 3 is empty, 4 misses the stride
    index, table = pm.compact(last, pm.feature_table(feat, score).numpy())
    assert index.dtype == np.int16 and table.shape == (4, feat.shape[1])
    for new, old in enumerate(used):
        assert np.array_equal(table[new], PU.scaled_row(feat[old], score[old]))
        assert np.array_equal(index == new, last == old)
    assert np.array_equal(index == -1, last == -1) and (last == -1).any()


def test_file_round_trip(tmp_path):
    rs = np.random.RandomState(1)
    fr = PU.synthetic_frame(rs, 20, 30, 5, 6)
    index, table = PU.compact_of(fr["segmentation"][:, ::5, ::5], fr["feat"], fr["stability_score"])
    path = str(tmp_path / "7.npz")
    pm.save_compact(path, index, table)
    with np.load(path) as d:
        assert sorted(d.files) == ["index", "table"] and d["index"].dtype == np.int16 and d["table"].dtype == np.float32
    i2, t2 = pm.load_compact(path)
    assert np.array_equal(i2, index) and np.array_equal(t2, table)
    idx, tab = pm.shifted(i2, t2)
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and not tab[0].any() and tab.shape[0] == table.shape[0] + 1
    assert np.array_equal(pm.densify_host(i2, t2),
                          PU.reference_loop(fr["segmentation"][:, ::5, ::5], fr["feat"], fr["stability_score"]))
    np.savez(str(tmp_path / "bad.npz"), index=np.full((2, 2), 3, np.int16), table=np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError):
        pm.load_compact(str(tmp_path / "bad.npz"))


def test_bad_shapes_and_no_masks():
    with pytest.raises(ValueError):
        pm.strided_masks({"segmentation": np.zeros((2, 41, 60), bool)}, 5)         # H % d != 0
    with pytest.raises(ValueError):
        pm.strided_masks({"segmentation": np.zeros((2, 40, 61), bool)}, 5)         # W % d != 0
    pre = np.zeros((2, 8, 12), bool)
    assert pm.strided_masks({"segmentation_strided": pre}, 5).shape == (2, 8, 12)   # already on the stride
    with pytest.raises(ValueError):
        pm.feature_table(np.zeros((3, 4), np.float32), np.ones(2))
    # M = 0: an all-zero map (the reference itself fails there)
    masks = pm.strided_masks({"segmentation": np.zeros((0, 40, 60), bool)}, 5)
    table = pm.feature_table(np.zeros((0, 16), np.float16), np.zeros(0)).numpy()
    index, tab = pm.compact(PU.last_mask(masks), table)
    assert masks.shape == (0, 8, 12) and (index == -1).all() and tab.shape == (0, 16)
    assert not pm.densify_host(index, tab).any() and pm.densify_host(index, tab).shape == (8, 12, 16)


def test_loader_prefers_the_dense_file(tmp_path):
    SF.write_scene(str(tmp_path), "Replica", n_frames=20)
    PU.write_part_files(str(tmp_path), [0, 10], SF.H, SF.W, DOWN, 6, "dense", seed=1)
    PU.write_part_files(str(tmp_path), [0, 10], SF.H, SF.W, DOWN, 6, "compact", seed=2)     # different content
    s = ods.Replica(make_cfg(tmp_path, "Replica"))[1]
    assert "part_index" not in s and "part_table" not in s
    want = np.load(str(tmp_path / "partlevel" / "10.npy")).transpose(1, 0, 2)
    assert s["part_feat"].dtype == torch.float32 and np.array_equal(s["part_feat"].numpy(), want)


@pytest.mark.parametrize("fmt", ["Replica", "ScanNet"])
def test_loader_returns_the_compact_form(tmp_path, fmt):
    SF.write_scene(str(tmp_path), fmt, n_frames=20)
    pairs = PU.write_part_files(str(tmp_path), [0, 10], SF.H, SF.W, DOWN, 6, "compact", seed=3)
    c = make_cfg(tmp_path, fmt)
    ds = ods.Replica(c) if fmt == "Replica" else ods.ScanNet(c)
    for i, (index, table) in enumerate(pairs):
        s = ds[i]
        assert "part_feat" not in s
        pi, pt = s["part_index"], s["part_table"]
        assert pi.dtype == torch.int32 and tuple(pi.shape) == (SF.W // DOWN, SF.H // DOWN) and pi.is_contiguous()
        assert np.array_equal(pi.numpy(), index.T.astype(np.int32) + 1)          # transposed, 0 = none
        assert pt.dtype == torch.float32 and tuple(pt.shape) == (table.shape[0] + 1, 6)
        assert not pt[0].any() and np.array_equal(pt[1:].numpy(), table)
    s = list(ods.init_loader(c, multi_worker=False))[1]
    assert torch.is_tensor(s["part_index"]) and s["part_index"].dtype == torch.int32 and "part_feat" not in s


def test_scannet_halving_densifies_on_the_host(tmp_path):
    """part_down 10 (the stored maps are halved on load): a compact file gives the tensor the dense file gives."""
    got = {}
    for form in ("dense", "compact"):
        root = tmp_path / form
        SF.write_scene(str(root), "ScanNet", n_frames=20)
        PU.write_part_files(str(root), [0, 10], SF.H, SF.W, DOWN, 6, form, seed=4)
        s = ods.ScanNet(make_cfg(root, "ScanNet", **{"trainer.part_down": 10}))[1]
        assert "part_index" not in s
        got[form] = s["part_feat"]
    assert got["dense"].shape == (SF.W // DOWN // 2, SF.H // DOWN // 2, 6) and got["dense"].abs().sum() > 0
    assert torch.equal(got["dense"], got["compact"])


def test_part_store_bookkeeping():
    """Two frames with different table sizes on the host: the second frame's indices move by its base row, row 0 stays
    zero, and table[index] is each frame's own dense map; the buffers grow past their first capacity."""
    rs = np.random.RandomState(5)
    store = pm.PartStore("cpu")
    assert store.index is None and store.nbytes() == 0
    dense = []
    for k in range(11):                                  # more than the 8 frames / 64 rows of the first buffers
        fr = PU.synthetic_frame(rs, 12, 16, 3 + 2 * k, 6)
        masks = fr["segmentation"][:, ::2, ::2]
        index, table = PU.compact_of(masks, fr["feat"], fr["stability_score"])
        idx, tab = pm.shifted(index, table)
        store.append(idx.t().contiguous(), tab)
        dense.append(PU.reference_loop(masks, fr["feat"], fr["stability_score"]).transpose(1, 0, 2))
    assert store.index.shape == (11, 8, 6) and store.index.dtype == torch.int32 and store.n_rows == store.table.shape[0]
    assert not store.table[0].any() and store.n_rows > 64
    assert int(store.index.max()) < store.n_rows and int(store.index[1:].max()) > int(store.index[0].max())
    for k, want in enumerate(dense):
        assert np.array_equal(store.table[store.index[k].long()].numpy(), want), k
    assert store.nbytes() == 4 * (store.index.numel() + store.table.numel())
    with pytest.raises(pm.ops.ObjnerfError):
        store.append(torch.zeros(3, 3, dtype=torch.int32), torch.zeros(1, 6))       # another frame shape
    with pytest.raises(pm.ops.ObjnerfError):
        store.append(torch.zeros(8, 6, dtype=torch.int64), torch.zeros(1, 6))       # wrong dtype
