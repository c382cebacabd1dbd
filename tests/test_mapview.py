"""CPU: the two host-side pieces of the batched map view (openobj_amd/map_view.py) -- the closed form of
the z-buffer merge against the fold it replaces, and the tile list of the segmented renderer."""
import numpy as np

from openobj_amd import ops, render_view

DEPTHS = np.array([0.5, 1.0, 1.0, 2.0, 3.0, 100.0, 150.0], np.float32)      # ties, and entries that can never paint


def fold(masks, depths, colors, class_ids, is_bg):
    """ViewBuffers.merge over the objects in order, as render_view.render_view drives it; painter = the last object that
    won each pixel."""
    K, W, H = masks.shape
    buf = render_view.ViewBuffers(W, H)
    painter = np.full((W, H), -1, np.int64)
    for k in range(K):
        ok = buf.merge(masks[k], depths[k][masks[k]], colors[k][masks[k]], int(class_ids[k]), bool(is_bg[k]))
        painter[ok] = k
    return painter, buf


def test_merge_closed_form_equals_the_fold():
    """C1: K = 1..7 objects over 6 pixels, depths from a set with ties and with values >= 100, a random share of
    backgrounds at any position: painter, depth, mask id and colour of the closed form equal the sequential fold."""
    rs = np.random.RandomState(20240611)
    seen_bg_paint = seen_tie = 0
    for case in range(2500):
        K = int(rs.randint(1, 8))
        W, H = 6, 1
        masks = rs.uniform(size=(K, W, H)) < rs.uniform(0.3, 1.0)
        depths = DEPTHS[rs.randint(0, len(DEPTHS), size=(K, W, H))]
        colors = rs.randint(0, 256, size=(K, W, H, 3)).astype(np.uint8)
        is_bg = rs.uniform(size=K) < rs.uniform(0.0, 1.0)
        class_ids = np.arange(1, K + 1, dtype=np.int32) * 3
        painter_f, buf = fold(masks, depths, colors, class_ids, is_bg)
        painter, depth, maskid = render_view.merge_closed_form(masks, depths, class_ids, is_bg)
        assert np.array_equal(painter, painter_f), case
        assert np.array_equal(depth, buf.depth), case
        assert np.array_equal(maskid, buf.maskid), case
        rgb = np.where((painter >= 0)[..., None],
                       np.take_along_axis(colors, np.maximum(painter, 0)[None, ..., None], axis=0)[0], 0).astype(np.uint8)
        assert np.array_equal(rgb, buf.rgb), case
        seen_bg_paint += int((is_bg[np.maximum(painter, 0)] & (painter >= 0)).sum())
        off = np.where(masks & ~is_bg[:, None, None] & (depths < 100), depths, np.inf)
        seen_tie += int(((off == off.min(axis=0)) & np.isfinite(off)).sum(axis=0).max() > 1)
    assert seen_bg_paint > 500 and seen_tie > 200        # the cases do contain painting backgrounds and tied minima


def test_render_tiles_cover_every_group_once():
    """C2: segments of 0, 2, 15, 16, 17 and 1059 rays: every 16-ray group of every segment is in exactly one tile, no
    tile straddles an object, the tiles of a row are adjacent and ascending, empty segments have none."""
    sizes = [0, 2, 15, 16, 17, 1059]
    rows = [(10 + i, n) for i, n in enumerate(sizes)]
    for tg in (1, 4, 5):
        tiles = ops.render_tiles(rows, tile_groups=tg)
        assert tiles.dtype == np.int32 and tiles.shape[1] == 3
        assert (tiles[:, 2] >= 1).all() and (tiles[:, 2] <= tg).all()
        seen_rows = []
        for row, n in rows:
            t = tiles[tiles[:, 0] == row]
            groups = (n + 15) // 16
            if n == 0:
                assert len(t) == 0
                continue
            covered = np.concatenate([np.arange(f, f + g) for _, f, g in t])
            assert np.array_equal(covered, np.arange(groups)), (row, tg)      # each group once, ascending, none beyond
            seen_rows.append(row)
        # adjacency: the row column changes exactly len(seen_rows) - 1 times, in the order given
        change = np.flatnonzero(np.diff(tiles[:, 0]) != 0)
        assert len(change) == len(seen_rows) - 1
        assert list(tiles[np.r_[0, change + 1], 0]) == seen_rows
    assert ops.render_tiles([(0, 0), (1, 0)]).shape == (0, 3)
    assert ops.render_tiles([]).shape == (0, 3)


def test_cli_helpers(tmp_path):
    """--frames parsing, the depth image as cv2.imwrite would store it, and the three files in [H, W]."""
    from PIL import Image
    from openobj_amd import map_view
    assert list(map_view.parse_frames(None, 5)) == [0, 1, 2, 3, 4]
    assert list(map_view.parse_frames("1:4", 5)) == [1, 2, 3] and list(map_view.parse_frames("::2", 5)) == [0, 2, 4]
    assert list(map_view.parse_frames("3", 5)) == [3] and list(map_view.parse_frames("2:", 5)) == [2, 3, 4]
    d = np.array([[0.4, 0.5, 1.5], [2.5, 100.0, 300.0]], np.float32)
    assert map_view.depth_png(d, None).tolist() == [[0, 0, 2], [2, 100, 255]] and map_view.depth_png(d, None).dtype == np.uint8
    assert map_view.depth_png(d, 1000.0).tolist() == [[400, 500, 1500], [2500, 65535, 65535]]
    buf = render_view.ViewBuffers(3, 2)
    buf.rgb[2, 1] = (10, 20, 30)
    buf.maskid[0, 1] = 7
    buf.depth[1, 0] = 2.4
    map_view.write_view(str(tmp_path), 17, buf)
    rgb, dep, mid = (np.asarray(Image.open(tmp_path / f"{n}_17.png")) for n in ("rgb", "depth", "maskid"))
    assert rgb.shape == (2, 3, 3) and rgb[1, 2].tolist() == [10, 20, 30]
    assert mid.shape == (2, 3) and mid[1, 0] == 7 and dep[0, 1] == 2 and dep[1, 1] == 100
