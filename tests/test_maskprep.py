"""The mask front end without a GPU: the host form of openobj_amd.mask_prep against the reference's own mask_gen.py
(fixture G18), the integer restatement of PIL's resample against PIL, the ValueError cases, and write_mask_init read
back through mask_graph.load_inputs."""
import os

import numpy as np
import pytest

from openobj_amd import mask_graph as MG
from openobj_amd import mask_prep as MP
try:
    from tests import maskprep_util as U
except ImportError:          # plain `pytest tests/` puts tests/ itself, not the repository root, on sys.path
    import maskprep_util as U


def test_host_form_equals_g18(golden):
    """Masks, boxes, the crop sizes CLIP was handed and the prompts TAP was handed, for every frame of the fixture: the
    two colliding frames included."""
    g = golden("g18_maskprep")
    for f, (pm, sc, masks, boxes, crop_shapes, prompts) in enumerate(U.g18_frames(g)):
        fr = MP.frame_host(pm, sc)
        got = fr.masks()
        assert len(got) == len(masks) and all(np.array_equal(a, b) for a, b in zip(got, masks)), f
        assert fr.boxes.dtype == np.intp and np.array_equal(fr.boxes, boxes), f
        assert fr.id_image.dtype == np.uint8
        plan = MP.CropPlan(fr.boxes, *pm.shape[1:])
        assert np.array_equal(plan.sizes, crop_shapes), f
        p = MP.tap_box_prompts(fr.boxes, float(g["tap_scale"]))
        assert p.dtype == np.float32 and np.array_equal(p, prompts), f


def test_fixture_covers_its_cases(golden):
    """What G18 is meant to pin is in it: a mask split in three, a chain of four kept whole, both collisions."""
    fr = U.g18_frames(golden("g18_maskprep"))
    assert len(fr[0][2]) == 6 and len(fr[0][0]) == 5          # 4 masks above the threshold, one of them split in three
    assert len(fr[4][2]) == 2                                 # the chain stays one mask
    for f in (2, 3):
        img = MP.paint_host(fr[f][0], MP.rank_order(fr[f][1]))
        ids = np.unique(img)
        assert len(ids) in ids[ids > 0]                       # the first fresh id is an id of the image
        mixed = [m for m in fr[f][2] if len(np.unique(img[m])) > 1]
        assert len(mixed) == (1 if f == 2 else 0)             # frame 2: a final mask made of parts of two predicted ones
    img = MP.paint_host(fr[3][0], MP.rank_order(fr[3][1]))    # frame 3: the part comes BEFORE the mask it met
    assert np.unique(img[fr[3][2][-2]]).tolist() == [3] and np.unique(img[fr[3][2][-1]]).tolist() == [4]


def test_stable_rank_and_threshold():
    s = np.array([0.7, 0.9, 0.5, 0.7, 0.4999], np.float32)
    assert MP.rank_order(s).tolist() == [1, 0, 3, 2]          # the tie keeps the masks' order; 0.5 is kept
    m = np.zeros((5, 4, 4), bool)
    m[0, :2], m[3, 1:3], m[1, 0, 0] = True, True, True
    img = MP.paint_host(m, MP.rank_order(s))
    assert img[0, 0] == 2 and img[1, 0] == 3 and img[2, 0] == 3 and img[3, 0] == 0       # the later (lower) mask wins


def test_value_errors():
    many = np.zeros((256, 2, 2), bool)
    with pytest.raises(ValueError):
        MP.rank_order(np.ones(256, np.float32))
    assert len(MP.rank_order(np.ones(255, np.float32))) == 255
    with pytest.raises(ValueError):
        MP.frame_host(many, np.ones(256, np.float32))
    # a fresh id above 255: 254 ids + 0 in the image, and one id in three far parts
    H, W = 40, 3 * 254
    img = np.zeros((H, W), np.int32)
    for i in range(254):
        img[0:2, 3 * i:3 * i + 2] = i + 1                     # (small: they only occupy the ids)
    img[10:20, 0:10] = img[10:20, 300:310] = img[10:20, 600:610] = 254
    assert len(np.unique(img)) == 255
    with pytest.raises(ValueError):
        MP.split_host(img, 100)
    img[img == 1] = 0                                         # one id fewer: the fresh ids are 254 and 255
    assert len(np.unique(img)) == 254
    out = MP.split_host(img, 100)
    assert out[15, 305] == 254 and out[15, 605] == 255 and out[15, 5] == 254             # 254 meets itself: the collision
    with pytest.raises(ValueError):
        MP.CropPlan([U.box(0, 0, 10, 50)], 40, 40)


@pytest.mark.parametrize("w,h", [(12, 15), (500, 300), (224, 300), (300, 224), (20, 240), (224, 224), (31, 7), (640, 480)])
def test_restated_resample_equals_pil(w, h):
    """crops_host (integer tables, two passes, the kept rows and columns only) == PIL + numpy fp32, bit for bit, up- and
    downscaling, a pass skipped, both passes skipped."""
    rs = np.random.RandomState(w * 1000 + h)
    image = rs.randint(0, 256, (h + 13, w + 9, 3)).astype(np.uint8)
    boxes = [U.box(4, 6, 4 + w, 6 + h)]
    want = U.clip_oracle(image, boxes, pad=0)
    got = MP.crops_host(image, boxes, pad=0)
    assert got.dtype == np.float32 and got.shape == (1, 3, 224, 224) and np.array_equal(got, want)


def test_crop_padding_is_clipped_at_the_borders():
    rs = np.random.RandomState(5)
    image = rs.randint(0, 256, (96, 128, 3)).astype(np.uint8)
    boxes = [U.box(0, 0, 12, 12), U.box(116, 84, 128, 96), U.box(5, 30, 40, 60), U.box(100, 3, 125, 50)]
    plan = MP.CropPlan(boxes, 96, 128)
    assert plan.sizes.tolist() == [[32, 32], [32, 32], [70, 60], [70, 48]]
    assert np.array_equal(MP.crops_host(image, boxes), U.clip_oracle(image, boxes))


def test_write_mask_init_round_trips_through_load_inputs(golden, tmp_path):
    from PIL import Image
    g = golden("g18_maskprep")
    frames = [MP.frame_host(pm, sc) for pm, sc, *_ in U.g18_frames(g)]
    rs = np.random.RandomState(0)
    caps = [["thing %d" % i for i in range(len(fr.ids))] for fr in frames]
    capft = [rs.randn(len(fr.ids), 8).astype(np.float32) for fr in frames]
    clipft = [[rs.randn(1, 6).astype(np.float32) for _ in fr.ids] for fr in frames]
    path = str(tmp_path / "mask_init_all.pkl")
    MP.write_mask_init(path, frames, caps, capft, clipft)
    data = tmp_path / "scene"
    F = len(frames)
    for sub in ("depth", "rgb"):
        (data / sub).mkdir(parents=True)
        for i in range(2 * F + 1):            # [0:-1:2] keeps F files
            arr = np.zeros((96, 128), np.uint16) if sub == "depth" else np.zeros((96, 128, 3), np.uint8)
            Image.fromarray(arr).save(str(data / sub / ("%d.png" % i)))
    np.savetxt(str(data / "traj_w_c.txt"), np.tile(np.eye(4).reshape(1, 16), (2 * F + 1, 1)))
    masks, capf, clipf, captions, depth, rgb, twc, _ = MG.load_inputs({"skip": 2}, path, str(data))
    assert len(masks) == F == len(depth) == len(rgb) and twc.shape == (F, 4, 4)
    for f, fr in enumerate(frames):
        assert all(m.dtype == bool and np.array_equal(m, w) for m, w in zip(masks[f], fr.masks()))
        assert captions[f] == caps[f]
        assert np.allclose(np.linalg.norm(capf[f], axis=1), 1.0, atol=1e-6)
        assert np.allclose(capf[f] * np.linalg.norm(capft[f], axis=1, keepdims=True), capft[f], atol=1e-6)
        assert all(v.shape == (1, 6) and abs(np.linalg.norm(v) - 1.0) < 1e-6 for v in clipf[f])
    assert os.path.getsize(path) > 0
