"""The mask front end at the reference's native shape: 1200 x 680 frames in batches of 16, 60 predicted masks per frame
(an ASSUMED figure: CropFormer's count depends on the scene).  Reports, per frame,
  * the split chain on the GPU (labels, component table, boundary lists and gaps, relabel; the painted id images
    resident), its read-backs and the bytes it moved, on TWO data sets: "overpainted" (random masks as drawn: some mask
    is always painted over entirely, so the ids have a gap and the frames collide) and "gap-free" (the same masks
    without those that keep no pixel, and with a zero pixel: no fresh id can meet an id, the kernels' result is the
    result); how many frames took the host form is stated for each,
  * the paint step from masks in pageable host memory,
  * the CLIP crops of a frame's boxes: MaskPrep.crops (the host's coefficient tables and their upload included) and
    objnerf_clip_crops alone with the tables resident,
  * the module's own host form (scipy.ndimage.label per id and exact distances; PIL's resize and numpy), with a pool of
    16 threads over the frames of the batch.
The outputs of the two forms are asserted equal before anything is timed.  The split chain and the crop kernel are
bracketed by device events (for the chain the host work between its kernels is inside the bracket); everything that
copies from host memory or computes on the host is a host clock ending in a synchronise.  Medians of 5 windows after a
warm-up (3 for the host forms).  Writes profiles/maskprep_bench.txt (or --out).  Run on the GPU."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openobj_amd import mask_prep as MP  # noqa: E402
from openobj_amd import ops  # noqa: E402

W, H, FRAMES, MASKS, THREADS, WINDOWS = 1200, 680, 16, 60, 16, 5


def synthetic_frame(rs):
    """CropFormer-like output: a floor-like mask over the lower part, ellipses of 2 - 30 % of the image side, every fifth
    mask in two parts (a near and a far pair alternate), a few specks; scores in (0.3, 1)."""
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((MASKS, H, W), bool)
    masks[0, H // 2:] = True
    for m in range(1, MASKS):
        a, b = rs.randint(W // 50, W // 6), rs.randint(H // 50, H // 4)
        cx, cy = rs.randint(0, W), rs.randint(0, H)
        e = ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1.0
        masks[m] = e
        if m % 5 == 0:
            shift = 40 if m % 10 == 0 else 400
            masks[m] |= np.roll(e, shift + 2 * W // 6, axis=1)
        if m % 7 == 0:
            y, x = rs.randint(0, H - 3), rs.randint(0, W - 3)
            masks[m, y:y + 3, x:x + 3] = True
    scores = rs.uniform(0.3, 1.0, MASKS).astype(np.float32)
    scores[0] = 0.99
    return masks, scores


def without_overpainted(masks, scores):
    """The masks that keep at least one pixel of the painted image (dropping one uncovers pixels, never covers any)."""
    order = MP.rank_order(scores)
    img = MP.paint_host(masks, order)
    assert (img == 0).any()
    keep = np.sort(order[np.unique(img[img > 0]) - 1])
    ids = np.unique(MP.paint_host(masks[keep], MP.rank_order(scores[keep])))
    assert np.array_equal(ids, np.arange(len(ids)))                       # exactly 0..n: no fresh id can meet an id
    return masks[keep], scores[keep]


def sync_windows(fn, reps=WINDOWS):
    """A host clock around work that starts on the host and ends in a device synchronise."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def gpu_windows(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def host_windows(fn, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def per_frame(ts):
    return "%.3f ms (%.3f - %.3f)" % (statistics.median(ts) / FRAMES, min(ts) / FRAMES, max(ts) / FRAMES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "maskprep_bench.txt"))
    args = ap.parse_args()
    torch.set_num_threads(THREADS)
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    drawn = [synthetic_frame(rs) for _ in range(FRAMES)]
    sets = {"overpainted": drawn, "gap-free": [without_overpainted(*d) for d in drawn]}
    images = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(FRAMES)]
    prep = MP.MaskPrep(dev)
    pool = ThreadPoolExecutor(THREADS)
    lines = ["mask front end, %d x %d, batches of %d frames, %d masks a frame drawn (assumed), %s"
             % (W, H, FRAMES, MASKS, torch.cuda.get_device_name(0)),
             "per frame, median of %d windows (min - max); host forms: %d threads over the frames, median of 3" % (WINDOWS, THREADS),
             ""]
    raw = {}
    for name, data in sets.items():
        # ---- equality first
        res = prep.frames([d[0] for d in data], [d[1] for d in data])
        host = list(pool.map(lambda d: MP.frame_host(*d), data))
        for a, b in zip(res, host):
            assert np.array_equal(a.id_image, b.id_image) and np.array_equal(a.ids, b.ids) and np.array_equal(a.boxes, b.boxes)
        host_frames = sum(r.host_form for r in res)
        ids = torch.stack([prep.paint(*d) for d in data])
        painted = [MP.paint_host(d[0], MP.rank_order(d[1])) for d in data]
        assert np.array_equal(ids.cpu().numpy(), np.stack(painted))
        before = dict(prep.stats)
        t_split = gpu_windows(lambda: prep.split(ids))
        moved = {k: (prep.stats[k] - before[k]) / (WINDOWS + 1) for k in ("readbacks", "bytes_down", "bytes_up")}
        t_host = host_windows(lambda: list(pool.map(lambda p: MP.filter_boxes_host(MP.split_host(p)), painted)))
        n_boxes = sum(len(r.boxes) for r in res)
        lines += ["data set: %s (%.1f masks a frame kept, %.1f final masks)" % (name, np.mean([len(d[1]) for d in data]),
                                                                               n_boxes / FRAMES),
                  "  split chain (GPU, id images resident)    %s" % per_frame(t_split),
                  "    frames that took the host form         %d of %d" % (host_frames, FRAMES),
                  "    read-backs per batch                   %.1f" % moved["readbacks"],
                  "    bytes device -> host per batch         %d" % moved["bytes_down"],
                  "    bytes host -> device per batch         %d" % moved["bytes_up"],
                  "  split + filter, host form                %s" % per_frame(t_host),
                  ""]
        raw[name] = {"split_ms": t_split, "host_split_ms": t_host, "moved_per_batch": moved, "host_frames": int(host_frames),
                     "boxes": n_boxes}

    # ---- paint and crops, on the gap-free set
    data = sets["gap-free"]
    boxes = [r.boxes for r in res]
    t_paint = sync_windows(lambda: [prep.paint(*d) for d in data])
    crops = prep.crops(images[0], boxes[0])
    assert np.array_equal(crops.cpu().numpy(), MP.crops_host(images[0], boxes[0]))

    def pil_crops(image, bxs):
        from PIL import Image
        im, out = Image.fromarray(image), []
        for b in bxs:
            x0, y0, x1, y1 = int(b[0, 0]), int(b[0, 1]), int(b[2, 0]), int(b[2, 1])
            c = im.crop((x0 - min(20, x0), y0 - min(20, y0), x1 + min(20, W - x1), y1 + min(20, H - y1)))
            w, h = c.size
            ow, oh = (224, int(224 * h / w)) if w <= h else (int(224 * w / h), 224)
            c = c.resize((ow, oh), Image.BICUBIC)
            left, top = int(round((ow - 224) / 2.0)), int(round((oh - 224) / 2.0))
            out.append(np.asarray(c.crop((left, top, left + 224, top + 224))))
        return MP.normalize_host(np.stack(out))

    assert np.array_equal(crops.cpu().numpy(), pil_crops(images[0], boxes[0]))
    dev_images = [torch.from_numpy(i).to(dev) for i in images]
    t_crops = sync_windows(lambda: [prep.crops(i, b) for i, b in zip(dev_images, boxes)])
    plans = [MP.CropPlan(b, H, W) for b in boxes]
    tabs = [[torch.from_numpy(t).to(dev) for t in (p.desc, p.hb, p.hk, p.vb, p.vk)] for p in plans]
    t_kernel = gpu_windows(lambda: [ops.clip_crops(i, *t, p.tmp_rows) for i, t, p in zip(dev_images, tabs, plans)])
    t_pil = host_windows(lambda: list(pool.map(lambda a: pil_crops(*a), zip(images, boxes))))
    n_boxes = sum(len(b) for b in boxes)
    lines += ["paint from pageable host masks (upload included, host clock)     %s" % per_frame(t_paint),
              "CLIP crops, %.1f boxes a frame" % (n_boxes / FRAMES),
              "  MaskPrep.crops (host tables + upload + kernels, host clock)     %s" % per_frame(t_crops),
              "  objnerf_clip_crops alone, tables resident (device events)       %s" % per_frame(t_kernel),
              "  PIL + numpy                                                     %s" % per_frame(t_pil),
              ""]
    raw.update({"paint_ms": t_paint, "crops_ms": t_crops, "crops_kernel_ms": t_kernel, "pil_crops_ms": t_pil})
    text = "\n".join(lines + [json.dumps(raw)]) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
