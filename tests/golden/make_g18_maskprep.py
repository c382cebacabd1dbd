#!/usr/bin/env python3
"""Fixture G18: the reference's OWN maskclustering/mask_gen.py, run as __main__ on synthetic masks, on the CPU.

Run where the reference is checked out only:   python tests/golden/make_g18_maskprep.py REFERENCE_DIR

mask_gen.py imports packages and models this project does not ship.  They are replaced, for this script only:
  demo_cropformer.predictor   VisualizationDemo.run_on_image returns the synthetic masks and scores of the next frame
  detectron2, mask2former     read_image = a seeded 96 x 128 image (no file is read); configuration and logging stand-ins
  cv2                         connectedComponentsWithStats = scipy.ndimage.label (8-connectivity) + areas, boundingRect =
                              min / max of the points; the drawing calls do nothing
  tokenize_anything           im_rescale returns the scale 1.5; get_outputs records the box prompts it is given
  spacy, sentence_transformers, clip   stand-ins; CLIP's preprocess records the size of the crop it is given
  natsort, tqdm               stand-ins
So G18 pins the reference's LOGIC from the model outputs on: the painted order, split_mask (scipy's cKDTree and
scikit-learn's DBSCAN are the real ones), the area filters, min_rect_bbox, the padded crop boxes and the TAP prompts.

closest_distance draws a random tenth of each component, so main is run under 64 numpy seeds and ONE outcome is asserted:
the layouts below keep every pair of parts either 4 px apart or 37 px and more (eps is (96 + 128) / 10 = 22.4).

Frames (12 x 12 blocks unless said), masks in the predictor's order:
  0  A 20 x 20 overlapped by B 20 x 20 with the lower score (B wins); two blocks 4 px apart (stays one); three blocks
     41 px and more apart (becomes three); a block below the confidence threshold
  1  two near blocks plus one far; a block with a 6 x 6 part (the part is zeroed); an 8 x 8 mask (zeroed); blocks in the
     bottom-right and top-left corners (the crop padding is clipped)
  2  NO ZERO PIXEL: a mask over the whole frame, a mask of two far blocks, two single blocks: the ids are 1..4, the first
     fresh id is 4 and meets mask 4, whose block lies 4 px from the part: the two stay one mask
  3  A FULLY OVERPAINTED MASK: ids 0, 2, 3, 4; the first fresh id is 4 again; mask 4 lies far from the part, is split
     from it on its own visit and ends up AFTER it
  4  four blocks in a row 4 px apart: the first and the last are 37 px apart and join through the chain
"""
import os
import runpy
import sys
import tempfile
import types
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, B = 96, 128, 12
SCALE = 1.5
SEEDS = 64


def blocks(*at, size=B):
    m = np.zeros((H, W), bool)
    for y, x in at:
        m[y:y + size, x:x + size] = True
    return m


def frames():
    """[(masks bool [M, H, W], scores fp32 [M])]; the scores of a frame are distinct (torch.sort is not stable)."""
    f0 = [(blocks((4, 4), size=20), .95), (blocks((14, 14), size=20), .85), (blocks((40, 4), (40, 20)), .90),
          (blocks((4, 60), (4, 112), (70, 60)), .80), (blocks((80, 4)), .30)]
    f1 = [(blocks((4, 4), (4, 20), (70, 90)), .90), (blocks((30, 4)) | blocks((30, 60), size=6), .80),
          (blocks((50, 50), size=8), .70), (blocks((84, 116)), .60), (blocks((0, 0)), .55)]
    f2 = [(np.ones((H, W), bool), .99), (blocks((4, 4), (4, 100)), .90), (blocks((50, 50)), .80), (blocks((20, 100)), .70)]
    f3 = [(blocks((4, 4)), .90), (blocks((2, 2), size=18), .80), (blocks((50, 4), (50, 100)), .70), (blocks((80, 50)), .60)]
    f4 = [(blocks((4, 4), (4, 20), (4, 36), (4, 52)), .75), (blocks((60, 60), (60, 76)), .97)]
    return [(np.stack([m for m, _ in f]), np.array([s for _, s in f], np.float32)) for f in (f0, f1, f2, f3, f4)]


def make_cv2():
    from scipy import ndimage
    cv2 = types.ModuleType("cv2")
    cv2.CC_STAT_AREA, cv2.FONT_HERSHEY_SIMPLEX, cv2.COLOR_RGB2BGR, cv2.COLOR_BGR2RGB = 4, 0, 4, 4

    def components(mask, connectivity=8):
        assert connectivity == 8
        lab, k = ndimage.label(mask, structure=np.ones((3, 3), np.int32))
        stats = np.zeros((k + 1, 5), np.int32)
        stats[:, 4] = np.bincount(lab.ravel(), minlength=k + 1)
        return k + 1, lab, stats, None

    def bounding_rect(pts):
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        return int(lo[0]), int(lo[1]), int(hi[0] - lo[0] + 1), int(hi[1] - lo[1] + 1)

    cv2.connectedComponentsWithStats = components
    cv2.boundingRect = bounding_rect
    cv2.cvtColor = lambda img, code: img
    cv2.getTextSize = lambda *a, **k: ((10, 10), 0)
    cv2.rectangle = cv2.putText = cv2.drawContours = cv2.imwrite = lambda *a, **k: None
    return cv2


def run_reference(ref_dir, seed):
    """-> (the pickled dict, the crop sizes CLIP saw per frame, the prompts TAP saw per frame)."""
    data = frames()
    F = len(data)
    crops, prompts = [[] for _ in range(F)], []
    state = {"frame": 0, "clip": 0}

    class Demo:
        def __init__(self, cfg):
            pass

        def run_on_image(self, img):
            m, s = data[state["frame"]]
            state["frame"] += 1
            return {"instances": types.SimpleNamespace(pred_masks=torch.from_numpy(m.copy()), scores=torch.from_numpy(s.copy()))}

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    def read_image(path, format=None):
        return np.random.RandomState(int(os.path.splitext(path)[0])).randint(0, 256, (H, W, 3)).astype(np.uint8)

    class Tap:
        concept_projector = MagicMock()
        text_decoder = MagicMock()
        pixel_mean_value = 0

        def get_inputs(self, d):
            return dict(d)

        def get_features(self, d):
            return {}

        def get_outputs(self, inputs):
            prompts.append(np.array(inputs["points"], np.float32))
            n = len(inputs["points"])
            return {"iou_pred": torch.zeros(n, 4), "sem_tokens": torch.zeros(n, 4, 8)}

        def generate_text(self, tokens):
            return ["thing %d" % i for i in range(tokens.shape[0])]

    class Sbert:
        def __init__(self, path):
            pass

        def encode(self, captions, convert_to_tensor=True, device=None):
            return torch.from_numpy(np.random.RandomState(len(captions)).randn(len(captions), 8).astype(np.float32))

    class Pre:                                              # what preprocess returns: .unsqueeze(0).to("cuda")
        def unsqueeze(self, d):
            return self

        def to(self, d):
            return self

    def preprocess(pil):
        crops[state["clip_frame"]].append((pil.size[1], pil.size[0]))
        return Pre()

    class ClipModel:
        def encode_image(self, x):
            state["clip"] += 1
            return torch.from_numpy(np.random.RandomState(state["clip"]).randn(1, 8).astype(np.float32))

    def rgb_reader(path, format=None):                      # every loop reads the frame first: preprocess knows whose crop it sees
        state["clip_frame"] = int(os.path.splitext(path)[0]) // 10
        return read_image(path)

    stand_ins = {
        "cv2": make_cv2(),
        "natsort": mod("natsort", natsorted=lambda v: sorted(v, key=lambda p: int(os.path.splitext(p)[0]))),
        "tqdm": mod("tqdm", tqdm=lambda it, **k: it, trange=range),
        "detectron2": mod("detectron2"), "detectron2.config": mod("detectron2.config", get_cfg=MagicMock()),
        "detectron2.data": mod("detectron2.data"),
        "detectron2.data.detection_utils": mod("detectron2.data.detection_utils", read_image=rgb_reader),
        "detectron2.data.datasets": mod("detectron2.data.datasets"),
        "detectron2.data.datasets.builtin_meta": mod("detectron2.data.datasets.builtin_meta",
                                                     COCO_CATEGORIES=[{"color": [i, i, i]} for i in range(256)]),
        "detectron2.projects": mod("detectron2.projects"),
        "detectron2.projects.deeplab": mod("detectron2.projects.deeplab", add_deeplab_config=MagicMock()),
        "detectron2.utils": mod("detectron2.utils"),
        "detectron2.utils.logger": mod("detectron2.utils.logger", setup_logger=MagicMock()),
        "mask2former": mod("mask2former", add_maskformer2_config=MagicMock()),
        "demo_cropformer": mod("demo_cropformer"),
        "demo_cropformer.predictor": mod("demo_cropformer.predictor", VisualizationDemo=Demo),
        "spacy": mod("spacy", load=lambda name: (lambda text: types.SimpleNamespace(noun_chunks=[]))),
        "tokenize_anything": mod("tokenize_anything", model_registry={"tap_vit_l": lambda checkpoint=None: Tap()}),
        "tokenize_anything.utils": mod("tokenize_anything.utils"),
        "tokenize_anything.utils.image": mod("tokenize_anything.utils.image",
                                             im_rescale=lambda img, scales, max_size: ([img], [(SCALE, SCALE)]),
                                             im_vstack=lambda *a, **k: None),
        "sentence_transformers": mod("sentence_transformers", SentenceTransformer=Sbert, util=None),
        "clip": mod("clip", load=lambda name, device=None: (ClipModel(), preprocess)),
    }
    saved = {k: sys.modules.get(k) for k in stand_ins}
    argv = sys.argv
    sys.modules.update(stand_ins)
    np.random.seed(seed)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "o") + os.sep
            os.makedirs(out)
            # natsorted(input)[0:-1:10]: 10 * (F - 1) + 2 names give F frames, named 0, 10, 20, ...
            names = ["%d.png" % i for i in range(10 * (F - 1) + 2)]
            sys.argv = ["mask_gen.py", "--output", out, "--input"] + names
            runpy.run_path(os.path.join(ref_dir, "maskclustering", "mask_gen.py"), run_name="__main__")
            import pickle
            with open(out + "mask_init_all.pkl", "rb") as f:
                result = pickle.load(f)
    finally:
        sys.argv = argv
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return result, crops, prompts


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OPENOBJ_REFERENCE")
    if not ref_dir:
        raise SystemExit("usage: make_g18_maskprep.py REFERENCE_DIR")
    data = frames()
    first = None
    for seed in range(SEEDS):
        result, crops, prompts = run_reference(ref_dir, seed)
        got = ([np.stack(m) for m in result["mask"]], [np.stack(b) for b in result["bbox"]],
               [np.array(c, np.int32) for c in crops], prompts)
        if first is None:
            first = got
            continue
        for a, b in zip(first, got):                        # a condition of the fixture, not a measurement
            assert len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b)), \
                "seed %d gives another outcome: move the parts further from eps" % seed
    out = {"n_frames": np.int32(len(data)), "tap_scale": np.float32(SCALE), "seeds": np.int32(SEEDS)}
    for f, (m, s) in enumerate(data):
        out["pred_masks_%d" % f], out["scores_%d" % f] = m, s
        out["mask_%d" % f], out["bbox_%d" % f] = first[0][f], first[1][f].astype(np.int64)
        out["crop_shapes_%d" % f], out["prompts_%d" % f] = first[2][f], first[3][f]
        assert first[1][f].dtype == np.intp and len(first[0][f]) == len(first[1][f]) == len(first[2][f]) == len(first[3][f])
    np.savez_compressed(os.path.join(HERE, "g18_maskprep.npz"), **out)
    print("g18_maskprep.npz:", {k: (v.shape, str(v.dtype)) for k, v in out.items()})
    print("masks per frame:", [len(m) for m in first[0]])


if __name__ == "__main__":
    main()
