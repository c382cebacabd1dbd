"""The mask front end on the GPU (objnerf_maskprep.hip): component labels against scipy.ndimage.label per id, gaps against
numpy brute force, MaskPrep end to end against its host form and the reference's own mask_gen.py (fixture G18), the CLIP
crops against PIL + numpy fp32, and reproducibility.  Every comparison is an equality."""
import numpy as np
import pytest
import torch

from openobj_amd import mask_prep as MP
from openobj_amd import ops
try:
    from tests import maskprep_util as U
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import maskprep_util as U

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------- components
def spiral(h, w):
    """A one-pixel line spiralling inwards, one pixel of background between its turns."""
    m = np.zeros((h, w), bool)
    inside = lambda y, x: 0 <= y < h and 0 <= x < w
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    for _ in range(h * w):
        blocked = lambda dy, dx: not inside(y + dy, x + dx) or m[y + dy, x + dx] or \
            (inside(y + 2 * dy, x + 2 * dx) and m[y + 2 * dy, x + 2 * dx])
        if blocked(dy, dx):
            dy, dx = dx, -dy
            if blocked(dy, dx):
                break
        y, x = y + dy, x + dx
        m[y, x] = True
    return m


def component_frames():
    """int32 [2, 70, 90] (tiles are 32 x 32: 3 x 3 of them, the last ones partial); the second frame is the first turned
    by 180 degrees, so a wrong batch offset cannot pass."""
    a = np.zeros((70, 90), np.int32)
    a[0:40, 0:70][spiral(40, 70)] = 1                         # five tiles
    a[42:70, 2:4] = a[68:70, 2:80] = a[42:70, 78:80] = 2      # a U through the three bottom tiles
    a[60:64, 60:64] = a[64:67, 64:67] = 3                     # joined only through (63, 63) - (64, 64): the tile corner
    a[60:64, 32:36] = a[64:67, 29:32] = 4                     # the other diagonal, (63, 32) - (64, 31)
    a[44:51, 10:21], a[44:51, 21:31] = 5, 6                   # two ids that touch
    yy, xx = np.mgrid[44:59, 50:76]
    a[44:59, 50:76] = 7 + (yy + xx) % 2                       # a checkerboard of two ids across the tile edge x = 64
    return np.stack([a, a[::-1, ::-1]])


def test_labels_equal_scipy_per_id(dev):
    ids = component_frames()
    want = np.stack([U.label_oracle(f) for f in ids])
    for c, k in ((1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1)):       # what the shapes are meant to be
        assert len(np.unique(want[0][ids[0] == c])) == k
    d_ids = torch.from_numpy(ids).to(dev)
    label = ops.cc_label(d_ids)
    assert label.dtype == torch.int32 and np.array_equal(label.cpu().numpy(), want)
    # the table: the components in raster order of their first pixel, with id, area and box
    packed, slot = ops.cc_table(d_ids, label, 64)
    host = packed.cpu().numpy()
    off = host[:3]
    table = host[3:].view(np.int32).reshape(-1, ops.CC_ROW)
    for f in range(2):
        roots = np.flatnonzero(want[f].ravel() == np.arange(70 * 90))
        rows = table[off[f]:off[f + 1]]
        assert off[f + 1] - off[f] == len(roots) == 8 and np.array_equal(rows[:, 0], roots)
        for r in rows:
            ys, xs = np.nonzero(want[f] == r[0])
            assert r[1] == ids[f].ravel()[r[0]] and r[2] == len(ys) and r[7] == f
            assert r[3:7].tolist() == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
        s = slot[f].cpu().numpy().ravel()
        assert np.array_equal(np.flatnonzero(s >= 0), roots) and np.array_equal(s[roots], np.arange(off[f], off[f + 1]))
    # a table that outgrows its capacity says so and writes nothing past it
    packed, _ = ops.cc_table(d_ids, label, 5)
    host = packed.cpu().numpy()
    assert host[2] == 16 and len(host) == 3 + 4 * 5 and np.array_equal(host[3:].view(np.int32).reshape(5, 8), table[:5])


def test_labels_of_random_images(dev):
    """Dense random ids (many small components, many unions per tile border) at a size that is no multiple of the tile."""
    rs = np.random.RandomState(3)
    ids = (rs.randint(0, 3, (3, 45, 101)) * (rs.rand(3, 45, 101) < 0.8)).astype(np.int32)
    got = ops.cc_label(torch.from_numpy(ids).to(dev)).cpu().numpy()
    assert np.array_equal(got, np.stack([U.label_oracle(f) for f in ids]))


# -------------------------------------------------------------------------------------------------------------- gaps
def gaps_of(dev, ids, pairs_of_roots):
    """The kernels' d2 for pairs of components given by their first pixels."""
    d = torch.from_numpy(ids[None]).to(dev)
    label = ops.cc_label(d)
    packed, slot = ops.cc_table(d, label, 64)
    host = packed.cpu().numpy()
    table = host[2:].view(np.int32).reshape(-1, ops.CC_ROW)[:host[1]]
    row = {int(r[0]): i for i, r in enumerate(table)}
    sel = np.full(len(table), -1, np.int32)
    used = sorted({r for p in pairs_of_roots for r in p})
    for s, r in enumerate(used):
        sel[row[r]] = s
    boff, bpix = ops.cc_boundary(label, slot, torch.from_numpy(sel).to(dev), len(used), int(table[sel >= 0, 2].sum()))
    pairs = np.array([[used.index(a), used.index(b)] for a, b in pairs_of_roots], np.int32)
    return ops.cc_gaps(torch.from_numpy(pairs).to(dev), boff, bpix).cpu().numpy(), np.diff(boff.cpu().numpy())


def test_gaps_equal_brute_force(dev):
    """A ring whose boundary lists span several LDS tiles, a disc inside it, a block outside."""
    H, W = 110, 120
    yy, xx = np.mgrid[0:H, 0:W]
    r2 = (yy - 52) ** 2 + (xx - 50) ** 2
    ring, disc = (r2 <= 45 ** 2) & (r2 >= 38 ** 2), r2 <= 9 ** 2
    block = np.zeros((H, W), bool)
    block[97:108, 103:118] = True
    ids = (ring | disc | block).astype(np.int32)
    first = lambda m: int(np.flatnonzero(m.ravel())[0])
    pairs = [(first(ring), first(disc)), (first(disc), first(ring)), (first(ring), first(block)), (first(disc), first(block))]
    got, counts = gaps_of(dev, ids, pairs)
    assert counts.max() > 256 and counts.min() > 0
    want = [U.gap2_oracle(ring, disc), U.gap2_oracle(disc, ring), U.gap2_oracle(ring, block), U.gap2_oracle(disc, block)]
    assert got.tolist() == want and want[0] == want[1]


def test_threshold_is_exact_in_integers(dev):
    """H + W = 130: eps^2 = 169.  A mask whose two blocks are 13 px apart (d2 = 169) stays one; one whose blocks are
    (11, 7) apart (d2 = 170) is split; the same through the host form."""
    H, W = 60, 70
    ids = np.zeros((H, W), np.int32)
    ids[0:12, 0:12] = ids[0:12, 24:36] = 1                    # columns 11 and 24: dx = 13
    ids[30:42, 0:12] = ids[48:60, 22:34] = 2                  # rows 41 and 48, columns 11 and 22: (7, 11)
    got, _ = gaps_of(dev, ids, [(0, 24), (30 * W, 48 * W + 22)])
    assert got.tolist() == [169, 170]
    prep = MP.MaskPrep(dev)
    fr = prep.split(torch.from_numpy(ids[None]).to(dev))[0]
    assert not fr.host_form and fr.ids.tolist() == [1, 2, 3]
    img = fr.id_image
    assert img[5, 5] == 1 and img[5, 30] == 1 and img[35, 5] == 2 and img[50, 25] == 3
    host = MP.filter_boxes_host(MP.split_host(ids))[0]
    assert np.array_equal(img, host)


# -------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_equals_host_form_and_g18(golden, dev):
    g = golden("g18_maskprep")
    frames = U.g18_frames(g)
    prep = MP.MaskPrep(dev)
    res = prep.frames([f[0] for f in frames], [f[1] for f in frames])
    for f, (fr, (pm, sc, masks, boxes, _, _)) in enumerate(zip(res, frames)):
        assert fr.host_form == U.g18_collides(f)
        got = fr.masks()
        assert len(got) == len(masks) and all(np.array_equal(a, b) for a, b in zip(got, masks)), f
        assert fr.boxes.dtype == np.intp and np.array_equal(fr.boxes, boxes), f
        host = MP.frame_host(pm, sc)
        assert fr.id_image.dtype == np.uint8 and np.array_equal(fr.id_image, host.id_image), f
        assert np.array_equal(fr.ids, host.ids)
    # three read-backs for the batch, and one for the frames that went to the host form
    assert prep.stats["host_frames"] == 2 and prep.stats["frames"] == 5 and prep.stats["readbacks"] == 3 + 1
    # masks as device tensors, uint8
    again = prep.frames([torch.from_numpy(f[0].view(np.uint8)).to(dev) for f in frames], [torch.from_numpy(f[1]) for f in frames])
    assert all(np.array_equal(a.id_image, b.id_image) for a, b in zip(res, again))


def test_component_table_regrows(golden, dev):
    """A table that outgrows max_components is built again at the size it needs, which is kept: the same results as with
    the default, one read-back more on the first call and none more on the second."""
    frames = U.g18_frames(golden("g18_maskprep"))
    args = [f[0] for f in frames], [f[1] for f in frames]
    want = MP.MaskPrep(dev).frames(*args)
    small = MP.MaskPrep(dev, max_components=4)
    got = small.frames(*args)
    assert small.cap > 4 and small.stats["readbacks"] == 3 + 1 + 1
    again = small.frames(*args)
    assert small.stats["readbacks"] == 2 * (3 + 1) + 1
    for a, b, c in zip(want, got, again):
        for o in (b, c):
            assert np.array_equal(a.id_image, o.id_image) and np.array_equal(a.ids, o.ids) and np.array_equal(a.boxes, o.boxes)
            assert a.host_form == o.host_form


def test_uint8_masks_are_set_where_they_equal_one(dev):
    """mask_gen.py:295 tests `== 1`: a uint8 mask's other values are not set, on both paths."""
    m = np.zeros((2, 40, 40), np.uint8)
    m[0, 2:20, 2:20], m[1, 10:30, 10:30], m[1, 25:30, 25:30] = 1, 2, 1
    s = np.array([0.9, 0.8], np.float32)
    want = np.zeros((40, 40), np.int32)
    want[2:20, 2:20], want[25:30, 25:30] = 1, 2
    assert np.array_equal(MP.paint_host(m, MP.rank_order(s)), want)
    prep = MP.MaskPrep(dev)
    for masks in (m, torch.from_numpy(m).to(dev)):
        assert np.array_equal(prep.paint(masks, s).cpu().numpy(), want)


def test_too_many_ids_raise(dev):
    prep = MP.MaskPrep(dev)
    with pytest.raises(ValueError):
        prep.frames([np.zeros((256, 8, 8), bool)], [np.ones(256, np.float32)])
    H, W = 40, 3 * 254                                        # 255 ids in the image and one of them in three far parts
    img = np.zeros((H, W), np.int32)
    for i in range(253):
        img[0:2, 3 * i:3 * i + 2] = i + 1
    img[10:20, 0:10] = img[10:20, 300:310] = img[10:20, 600:610] = 254
    img[30:32, 0:2] = 255
    with pytest.raises(ValueError):
        prep.split(torch.from_numpy(img[None]).to(dev))
    with pytest.raises(ValueError):
        MP.split_host(img)


# -------------------------------------------------------------------------------------------------------------- crops
def check_crops(dev, image, boxes, pad=20):
    want = U.clip_oracle(image, boxes, pad)
    got = MP.MaskPrep(dev, pad=pad).crops(image, boxes)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(boxes), 3, 224, 224)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert np.array_equal(MP.crops_host(image, boxes, pad), want)


def test_crops_equal_pil_small_image(dev):
    """An upscaled 12 x 15 box, boxes on all four borders and in the corners, a side of exactly 224 after the padding
    (that pass is a copy), aspect 1 : 12."""
    image = np.random.RandomState(1).randint(0, 256, (300, 260, 3)).astype(np.uint8)
    boxes = [U.box(100, 120, 112, 135), U.box(0, 50, 30, 90), U.box(230, 50, 260, 90), U.box(60, 0, 90, 25),
             U.box(60, 270, 90, 300), U.box(0, 0, 12, 12), U.box(248, 288, 260, 300),
             U.box(20, 40, 204, 70), U.box(30, 30, 60, 214), U.box(20, 20, 204, 204)]
    plan = MP.CropPlan(boxes, 300, 260)
    assert plan.sizes[0].tolist() == [55, 52] and plan.sizes[7].tolist() == [70, 224] and plan.sizes[9].tolist() == [224, 224]
    assert plan.desc[7, 6] == -1 and plan.desc[7, 7] == -1 and plan.desc[8, 6] == -1      # 224 is the LONG side: resampled
    assert plan.desc[9, 6] == 0 and plan.desc[9, 7] == 0                                  # both passes are copies
    check_crops(dev, image, boxes)
    check_crops(dev, image, [U.box(100, 20, 120, 260), U.box(10, 100, 250, 120), U.box(5, 5, 229, 250),
                             U.box(5, 5, 250, 229)], pad=0)                                # 1 : 12 both ways; a copied pass


def test_crops_equal_pil_downscaled(dev):
    """A 300 x 500 box of a 340 x 600 image: 340 x 540 with the padding, both passes downscale."""
    image = np.random.RandomState(2).randint(0, 256, (340, 600, 3)).astype(np.uint8)
    boxes = [U.box(50, 20, 550, 320), U.box(0, 0, 600, 340)]
    assert MP.CropPlan(boxes, 340, 600).sizes.tolist() == [[340, 540], [340, 600]]
    check_crops(dev, image, boxes)


# ---------------------------------------------------------------------------------------------------- reproducibility
def test_two_runs_and_permuted_frames_agree(golden, dev):
    frames = U.g18_frames(golden("g18_maskprep"))
    rs = np.random.RandomState(9)
    noisy = [(f[0] & (rs.rand(*f[0].shape) < 0.97), f[1]) for f in frames]          # ragged parts: many components
    prep = MP.MaskPrep(dev)
    a = prep.frames([f[0] for f in noisy], [f[1] for f in noisy])
    b = prep.frames([f[0] for f in noisy], [f[1] for f in noisy])
    perm = [3, 0, 4, 2, 1]
    c = prep.frames([noisy[i][0] for i in perm], [noisy[i][1] for i in perm])
    for f in range(5):
        for other in (b[f], c[perm.index(f)]):
            assert a[f].id_image.tobytes() == other.id_image.tobytes() and a[f].host_form == other.host_form
            assert np.array_equal(a[f].ids, other.ids) and a[f].boxes.tobytes() == other.boxes.tobytes()
        host = MP.frame_host(*noisy[f])
        assert np.array_equal(a[f].id_image, host.id_image) and np.array_equal(a[f].boxes, host.boxes)
    image = rs.randint(0, 256, (96, 128, 3)).astype(np.uint8)
    x, y = prep.crops(image, a[0].boxes), prep.crops(image, a[0].boxes)
    assert torch.equal(x, y)


def test_arguments_are_checked(dev):
    ids = torch.zeros(1, 8, 8, dtype=torch.int32, device=dev)
    with pytest.raises(ops.ObjnerfError):
        ops.cc_label(ids[0])
    with pytest.raises(ops.ObjnerfError):
        ops.cc_label(ids.cpu())
    with pytest.raises(ops.ObjnerfError):
        ops.cc_table(ids, ops.cc_label(ids), 0)
    with pytest.raises(ValueError):
        MP.MaskPrep("cpu")
