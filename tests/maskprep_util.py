"""Shared by tests/test_maskprep.py and tests/test_maskprep_gpu.py: the G18 frames, and the oracles the tests are held to
(PIL + numpy fp32 for the CLIP crops, scipy.ndimage.label per id for the components, numpy brute force for the gaps)."""
import numpy as np

from openobj_amd import mask_prep as MP


def g18_frames(g):
    """-> [(pred_masks, scores, masks, boxes, crop shapes, prompts)] per frame of the fixture."""
    return [tuple(g["%s_%d" % (k, f)] for k in ("pred_masks", "scores", "mask", "bbox", "crop_shapes", "prompts"))
            for f in range(int(g["n_frames"]))]


def g18_collides(f):
    return f in (2, 3)              # no zero pixel; a fully overpainted mask (make_g18_maskprep.py)


def clip_oracle(image, boxes, pad=20):
    """mask_gen.py:495-516 with CLIP's transform written out: PIL crop, PIL bicubic resize of the short side to 224,
    centre crop, / 255 and (x - mean) / std in numpy fp32 -> fp32 [n, 3, 224, 224]."""
    from PIL import Image
    im = Image.fromarray(image)
    Wd, Ht = im.size
    out = []
    for b in np.asarray(boxes):
        x0, y0, x1, y1 = int(b[0, 0]), int(b[0, 1]), int(b[2, 0]), int(b[2, 1])
        x0, y0, x1, y1 = x0 - min(pad, x0), y0 - min(pad, y0), x1 + min(pad, Wd - x1), y1 + min(pad, Ht - y1)
        crop = im.crop((x0, y0, x1, y1))
        w, h = crop.size
        ow, oh = (224, int(224 * h / w)) if w <= h else (int(224 * w / h), 224)
        crop = crop.resize((ow, oh), Image.BICUBIC)
        left, top = int(round((ow - 224) / 2.0)), int(round((oh - 224) / 2.0))
        a = np.asarray(crop.crop((left, top, left + 224, top + 224)))
        x = a.astype(np.float32) / np.float32(255.0)
        x = (x - np.array(MP.CLIP_MEAN, np.float32)) / np.array(MP.CLIP_STD, np.float32)
        out.append(np.ascontiguousarray(x.transpose(2, 0, 1)))
    return np.stack(out)


def box(x0, y0, x1, y1):
    return MP.rect_of(x0, y0, x1, y1)


def label_oracle(ids):
    """Per id scipy.ndimage.label with 8-connectivity -> int32 [H, W]: the flat index of the component's first pixel in
    raster order, -1 where the id is 0."""
    from scipy import ndimage
    H, W = ids.shape
    out = np.full(H * W, -1, np.int32)
    for c in np.unique(ids):
        if c == 0:
            continue
        lab, k = ndimage.label(ids == c, structure=np.ones((3, 3), np.int32))
        flat = lab.ravel()
        for i in range(1, k + 1):
            px = np.flatnonzero(flat == i)
            out[px] = px[0]
    return out.reshape(H, W)


def gap2_oracle(a, b):
    """The minimum squared distance between two bool images, by brute force."""
    pa, pb = np.argwhere(a).astype(np.int64), np.argwhere(b).astype(np.int64)
    return int(((pa[:, None, :] - pb[None, :, :]) ** 2).sum(axis=2).min())
