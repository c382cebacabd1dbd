#!/usr/bin/env python3
"""Fixture G17: the reference's OWN partlevel/sam_clip_dir.py main() on synthetic masks and seeded features, on the CPU.

Run where the reference is checked out only:   python tests/golden/make_g17_partmap.py REFERENCE_DIR

sam_clip_dir.py imports packages and models this project does not ship.  They are replaced, for this script only:
  cv2                imread = a seeded 40 x 60 image (no file is read), cvtColor = channel flip
  clip               load -> (model, preprocess): preprocess records the size of the crop it is given, encode_image
                     returns the next row of a seeded [M, 16] feature matrix in the requested dtype
  segment_anything, natsort, tqdm, matplotlib     stand-ins; mask_getter returns the synthetic masks below
So G17 pins the reference's LOGIC from the masks on: bbox_getter's crop boxes, which masks are used, the product with
the stability score in the feature's dtype, the assignment order, the strided mask and the saved array -- not SAM or CLIP.
main() is run twice, with fp32 and with fp16 features.

The masks (40 x 60 image, down_sample 5), in SAM's order:
  0  x 0..19,  y 0..19    touches the image border (bbox_getter clips the growth); overlapped by 2
  1  x 12..17, y 12..17   every pixel is overwritten by mask 2 -> its row ends up unused
  2  x 10..24, y 10..29   width 15: 15 * 1.3 = 19.5 rounds to 20 (half to even, up)
  3  empty                (bbox 30,5 5x5: 5 * 1.3 = 6.5 rounds to 6, down)
  4  x 41..44, y 6..9     covers no pixel on the stride
  5  x 45..59, y 25..39   touches the right and bottom borders
  6  x 30..34, y 30..34   width 5; one pixel (30, 30) on the stride
predicted_iou is above 0.9 for some and below for others: the reference's filter changes nothing.
"""
import argparse
import os
import sys
import tempfile
import types
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, D, C = 40, 60, 5, 16

RECTS = [(0, 0, 20, 20), (12, 12, 6, 6), (10, 10, 15, 20), None, (41, 6, 4, 4), (45, 25, 15, 15), (30, 30, 5, 5)]
BBOX = [(0, 0, 20, 20), (12, 12, 6, 6), (10, 10, 15, 20), (30, 5, 5, 5), (41, 6, 4, 4), (45, 25, 15, 15), (30, 30, 5, 5)]
SCORE = [0.97, 0.93, 0.88, 0.99, 0.95, 0.91, 0.96]
IOU = [0.95, 0.85, 0.92, 0.99, 0.80, 0.91, 0.89]


def synthetic_masks():
    out = []
    for rect, bbox, s, iou in zip(RECTS, BBOX, SCORE, IOU):
        seg = np.zeros((H, W), bool)
        if rect is not None:
            x, y, w, h = rect
            seg[y:y + h, x:x + w] = True
        out.append({"segmentation": seg, "bbox": list(bbox), "stability_score": float(np.float32(s)),
                    "predicted_iou": float(np.float32(iou))})
    return out


def run_reference(ref_dir, feat, out_dir):
    """sam_clip_dir.main with the stand-ins; feat [M, C] in the dtype encode_image is to return."""
    crops = []
    rows = iter(range(feat.shape[0]))

    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2RGB = 4
    cv2.imread = lambda path: np.random.RandomState(3).randint(0, 256, (H, W, 3)).astype(np.uint8)
    cv2.cvtColor = lambda img, code: img[..., ::-1].copy()

    def preprocess(pil):
        crops.append((pil.size[1], pil.size[0]))           # (height, width) of the crop CLIP would see
        return torch.zeros(3, 4, 4)

    model = types.SimpleNamespace(encode_image=lambda x: torch.from_numpy(feat[next(rows)][None].copy()))
    clip = types.ModuleType("clip")
    clip.load = lambda name, device=None: (model, preprocess)
    sa = types.ModuleType("segment_anything")
    sa.sam_model_registry = {}
    sag = types.ModuleType("segment_anything.automatic_mask_generator")
    sag.SamAutomaticMaskGenerator = MagicMock()
    natsort = types.ModuleType("natsort")
    natsort.natsorted = sorted
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it: it
    stand_ins = {"cv2": cv2, "clip": clip, "segment_anything": sa, "segment_anything.automatic_mask_generator": sag,
                 "natsort": natsort, "tqdm": tqdm, "matplotlib": MagicMock(), "matplotlib.pyplot": MagicMock()}
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    sys.path.insert(0, os.path.join(ref_dir, "partlevel"))
    try:
        sys.modules.pop("sam_clip_dir", None)
        import sam_clip_dir
        sam_clip_dir.mask_getter = lambda image: synthetic_masks()
        # natsorted(input_image)[0:-1:10] keeps the first of two names; the file is saved as str(0 * 10) + '.npy'
        sam_clip_dir.main(argparse.Namespace(input_image=["0.png", "1.png"], output_dir=out_dir, down_sample=D))
    finally:
        sys.path.pop(0)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return np.load(os.path.join(out_dir, "0.npy")), np.array(crops, np.int32)


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OPENOBJ_REFERENCE")
    if not ref_dir:
        raise SystemExit("usage: make_g17_partmap.py REFERENCE_DIR")
    masks = synthetic_masks()
    feat32 = np.random.RandomState(17).randn(len(masks), C).astype(np.float32)
    feat16 = feat32.astype(np.float16)
    out = {"segmentation": np.stack([m["segmentation"] for m in masks]),
           "bbox": np.array([m["bbox"] for m in masks], np.int32),
           "stability_score": np.array([m["stability_score"] for m in masks], np.float64),
           "predicted_iou": np.array([m["predicted_iou"] for m in masks], np.float64),
           "down_sample": np.int32(D), "feat_fp32": feat32, "feat_fp16": feat16}
    for tag, feat in (("fp32", feat32), ("fp16", feat16)):
        with tempfile.TemporaryDirectory() as tmp:
            dense, crops = run_reference(ref_dir, feat, tmp)
        assert dense.dtype == np.float32 and dense.shape == (H // D, W // D, C)
        out["dense_" + tag] = dense
        out["crop_shapes"] = crops                          # (the same for both runs)
    np.savez_compressed(os.path.join(HERE, "g17_partmap.npz"), **out)
    print("g17_partmap.npz:", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
